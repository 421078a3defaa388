// percentile_approx / median_approx finish on the device: the reference casts the edges=True
// count grid to float64, runs np.cumsum over its last axis and calls grid_find_edges per cell
// and percentage (dataframe.py:1419-1555, vaexfast.cpp:1574-1628).  Here the count grid stays
// in HBM and one kernel reads it at most twice:
//
//   pass 1  every thread sums one segment of one cell's percentile axis (int64); an exclusive
//           prefix over the segments gives each segment's starting cumulative and the total
//   pass 2  every thread walks its segment again with the running cumulative and records, for
//           the thresholds floor(v) / ceil(v) of every percentage, the first entry whose
//           cumulative reaches it (F = #{j : cum[j] < t}, with cum[F-1] and cum[F]); the
//           thresholds are sorted (the host sorts the percentages), so this is a merge, and a
//           segment stops reading once all of them are behind it
//   finish  left = clamp(F-1, 0, N-1), right = min(F, N-1) and the reference's interpolation,
//           in float64 with its operation order (-ffp-contract=off: no fused multiply-add)
//
// The cumulative is kept in int64 and converted where the reference reads it: counts are below
// 2^53, so that equals np.cumsum of the float grid bit for bit, and cum < t compares integers
// (t is integer-valued).
//
// Two thread mappings of the same kernel, chosen on the host by the outer cell count:
//   cells (64 cells x 4 or 8 segments)  lanes = consecutive outer cells (stride 1 in memory,
//           the percentile axis has stride S = prod(outer shapes)): every load is one
//           contiguous 512-byte row per wave, the waves of a workgroup split the axis
//   axis  (1 cell x 1024 segments)      fewer than 64 outer cells (no binby: one cell, P up to
//           65536): one workgroup per cell, threads along the axis, a block scan of the totals
#include <algorithm>
#include <cmath>
#include <numeric>

#include "engine.hpp"

using namespace vh;

namespace {
constexpr int PCT_MAX = 16;   // percentages per launch
constexpr int PCT_CPB = 64;   // cells mapping: outer cells per workgroup (one per lane)
constexpr int PCT_AXIS_THREADS = 1024;
constexpr int PCT_UNROLL = 8;  // loads in flight per lane in pass 2

struct PctPlan {
    int32_t nd_outer, np;     // outer axes; percentages of this launch (sorted ascending)
    uint32_t N, seglen;       // cumulative entries per cell (P + 2); entries per segment
    uint64_t S;               // stride of the percentile axis (items)
    uint64_t ncell;           // outer central cells
    double lo, hi;
    uint64_t cshape[MAX_DIM];  // central shape (shape - 3) of every outer axis
    uint64_t stride[MAX_DIM];
    double pct[PCT_MAX];
    uint32_t row[PCT_MAX];    // output row of each percentage
};

constexpr size_t pct_tot_items(int cpb, int nseg) { return cpb == 1 ? (size_t)nseg / 64 : (size_t)nseg * cpb; }
// s_tot, then per (floor | ceil, percentage, cell): threshold, cum[left], cum[right] (int64), F (int32)
constexpr size_t pct_lds_bytes(int cpb, int nseg, int np) {
    return pct_tot_items(cpb, nseg) * 8 + (size_t)2 * np * cpb * (3 * 8 + 4);
}

// dataframe.py:1492-1495: values = (totalcounts + 1) * p / 100., values[empty] = 0
__device__ inline double pct_value(int64_t total, double p) {
    const double v = ((double)total + 1.0) * p / 100.0;
    return total == 0 ? 0.0 : v;
}

// calculate_x (dataframe.py:1509-1519) for one cell with edges left = clamp(F-1, 0, N-1),
// right = min(F, N-1), cl = cum[left], cr = cum[right]
__device__ inline double pct_x(double t, uint32_t F, int64_t cl, int64_t cr, uint32_t N, double lo, double hi) {
    const uint32_t left = F == 0 ? 0u : F - 1, right = F < N ? F : N - 1;
    const double u = (t - (double)cl) / ((double)cr - (double)cl);
    const double den = (double)((int64_t)N - 3);
    const double xl = lo + (((double)left - 0.5) * (hi - lo)) / den;
    const double xr = lo + (((double)right - 0.5) * (hi - lo)) / den;
    return xl + (xr - xl) * u;
}

template <int CPB, int NSEG>
__global__ __launch_bounds__(CPB *NSEG) void k_percentile(const int64_t *__restrict__ grid, const PctPlan pl,
                                                           double *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char pct_smem[];
    const int np = pl.np;
    int64_t *s_tot = reinterpret_cast<int64_t *>(pct_smem);
    int64_t *s_thr = s_tot + pct_tot_items(CPB, NSEG);  // [2][np][CPB]
    int64_t *s_below = s_thr + 2 * np * CPB;
    int64_t *s_above = s_below + 2 * np * CPB;
    uint32_t *s_F = reinterpret_cast<uint32_t *>(s_above + 2 * np * CPB);

    const int tid = threadIdx.x, ci = tid % CPB, seg = tid / CPB;
    const uint64_t cell = (uint64_t)blockIdx.x * CPB + ci;
    const bool valid = cell < pl.ncell;
    const uint32_t N = pl.N;
    // the 3 edge slots of every outer axis are skipped by index decode
    uint64_t base = 0;
    if (valid) {
        uint64_t o = cell;
        for (int d = 0; d < pl.nd_outer; d++) {
            const uint64_t i = o % pl.cshape[d];
            o /= pl.cshape[d];
            base += (i + 2) * pl.stride[d];
        }
    }
    const uint64_t S = pl.S;
    const int64_t *col = grid + base + S;  // entry k of the cell (slot k + 1: the NaN slot is dropped)
    const uint32_t k0 = min((uint32_t)seg * pl.seglen, N), k1 = min(k0 + pl.seglen, N);

    // ---- pass 1: segment sums, exclusive prefix over the segments --------------------------
    int64_t sum = 0;
    if (valid) {
#pragma unroll 8
        for (uint32_t k = k0; k < k1; k++) sum += col[(uint64_t)k * S];
    }
    int64_t pre = 0, total = 0;
    if constexpr (CPB == 1) {
        const int lane = tid & 63, wave = tid >> 6;
        long long inc = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long y = __shfl_up(inc, off, 64);
            if (lane >= off) inc += y;
        }
        if (lane == 63) s_tot[wave] = inc;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NSEG / 64; w++) {
            const int64_t v = s_tot[w];
            pre += w < wave ? v : 0;
            total += v;
        }
        pre += inc - sum;
    } else {
        s_tot[seg * CPB + ci] = sum;
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NSEG; s++) {
            const int64_t v = s_tot[s * CPB + ci];
            pre += s < seg ? v : 0;
            total += v;
        }
    }

    // ---- thresholds; records start as "never reached": F = N, left = right = N - 1 ----------
    for (int j = seg; j < np; j += NSEG) {
        const double v = pct_value(total, pl.pct[j]);
        s_thr[j * CPB + ci] = (int64_t)floor(v);
        s_thr[(np + j) * CPB + ci] = (int64_t)ceil(v);
        for (int h = 0; h < 2; h++) {
            const int idx = (h * np + j) * CPB + ci;
            s_F[idx] = N;
            s_below[idx] = total;
            s_above[idx] = total;
        }
    }
    __syncthreads();

    // ---- pass 2: first entry whose cumulative reaches each threshold -----------------------
    if (valid && k0 < k1) {
        const int64_t *tf = s_thr + ci, *tg = s_thr + np * CPB + ci;
        int jf = 0, jg = 0;
        if (seg > 0) {  // pre = cum[k0 - 1] >= t: reached in an earlier segment
            while (jf < np && tf[jf * CPB] <= pre) jf++;
            while (jg < np && tg[jg * CPB] <= pre) jg++;
        }
        int64_t cum = pre, prev = pre;
        for (uint32_t k = k0; k < k1 && (jf < np || jg < np); k += PCT_UNROLL) {
            int64_t c[PCT_UNROLL];
#pragma unroll
            for (int u = 0; u < PCT_UNROLL; u++) c[u] = k + u < k1 ? col[(uint64_t)(k + u) * S] : 0;
#pragma unroll
            for (int u = 0; u < PCT_UNROLL; u++) {
                // an entry past the segment adds 0: every threshold <= cum is already taken
                cum += c[u];
                const int64_t below = k + u ? prev : cum;  // F = 0: left = right = 0
                while (jf < np && cum >= tf[jf * CPB]) {
                    const int idx = jf * CPB + ci;
                    s_F[idx] = k + u;
                    s_below[idx] = below;
                    s_above[idx] = cum;
                    jf++;
                }
                while (jg < np && cum >= tg[jg * CPB]) {
                    const int idx = (np + jg) * CPB + ci;
                    s_F[idx] = k + u;
                    s_below[idx] = below;
                    s_above[idx] = cum;
                    jg++;
                }
                prev = cum;
            }
        }
    }
    __syncthreads();

    // ---- finish (dataframe.py:1486-1525) ----------------------------------------------------
    for (int j = seg; j < np; j += NSEG) {
        if (!valid) continue;
        const double p = pl.pct[j];
        double r;
        if (p == 0.0) {
            r = pl.lo;
        } else if (p == 100.0) {
            r = pl.hi;
        } else {
            const double v = pct_value(total, p), f = floor(v), g = ceil(v);
            const int a = j * CPB + ci, b = (np + j) * CPB + ci;
            const double x1 = pct_x(f, s_F[a], s_below[a], s_above[a], N, pl.lo, pl.hi);
            const double x2 = pct_x(g, s_F[b], s_below[b], s_above[b], N, pl.lo, pl.hi);
            r = x1 + (x2 - x1) * (v - f);
        }
        out[(uint64_t)pl.row[j] * pl.ncell + cell] = r;
    }
}

template <int CPB, int NSEG> void launch_percentile(const int64_t *grid, PctPlan &pl, double *out) {
    pl.seglen = (pl.N + NSEG - 1) / NSEG;
    const uint64_t blocks = (pl.ncell + CPB - 1) / CPB;
    hipLaunchKernelGGL((k_percentile<CPB, NSEG>), dim3((unsigned)blocks), dim3(CPB * NSEG),
                       pct_lds_bytes(CPB, NSEG, pl.np), stream(), grid, pl, out);
}
static_assert(pct_lds_bytes(PCT_CPB, 8, PCT_MAX) <= 64 * 1024, "k_percentile: dynamic LDS above the default limit");
}  // namespace

extern "C" int vh_agg_percentile(vh_agg *a, const double *percentages, int npct, double lo, double hi, double *out,
                                 uint64_t out_items) {
    VH_API_BEGIN
    if (!a || !a->grid) fail(VH_ERR_ARG, "percentile: no aggregator");
    std::lock_guard<std::mutex> lk(a->grid->mu);
    const vh_grid *g = a->grid;
    if (a->kind != VH_AGG_COUNT || a->grid_dtype != VH_I64) fail(VH_ERR_ARG, "percentile: not an AggCount with an int64 grid");
    const int nd = (int)g->binners.size();
    if (nd < 1) fail(VH_ERR_ARG, "percentile: the grid has no binners (the last one is the percentile axis)");
    if (nd > MAX_DIM) fail(VH_ERR_ARG, "percentile: too many binners");
    if (npct < 1 || !percentages) fail(VH_ERR_ARG, "percentile: no percentages");
    for (int i = 0; i < npct; i++)
        if (!(percentages[i] >= 0.0 && percentages[i] <= 100.0))
            fail(VH_ERR_ARG, "percentile: percentage " + std::to_string(percentages[i]) + " outside [0, 100]");
    if (g->shapes[nd - 1] < 4 || g->shapes[nd - 1] - 1 > 0xffffffffull) fail(VH_ERR_ARG, "percentile: bad percentile axis");

    PctPlan pl{};
    pl.nd_outer = nd - 1;
    pl.N = (uint32_t)(g->shapes[nd - 1] - 1);
    pl.S = g->strides[nd - 1];
    pl.lo = lo;
    pl.hi = hi;
    pl.ncell = 1;
    for (int d = 0; d < nd - 1; d++) {
        pl.cshape[d] = g->shapes[d] >= 3 ? g->shapes[d] - 3 : 0;
        pl.stride[d] = g->strides[d];
        pl.ncell *= pl.cshape[d];
    }
    if (out_items != (uint64_t)npct * pl.ncell) fail(VH_ERR_ARG, "percentile: output size mismatch");
    if (pl.ncell == 0) return VH_OK;
    if (!out) fail(VH_ERR_ARG, "percentile: no output");
    if (pl.ncell > 0x7fffffffull) fail(VH_ERR_ARG, "percentile: too many outer cells");  // one launch's workgroups

    // ascending percentages: the thresholds of one cell are then ascending too
    std::vector<int> order(npct);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return percentages[x] < percentages[y]; });

    DevBuf dout;
    dout.ensure(out_items * 8);
    const auto *grid = static_cast<const int64_t *>(a->g.ptr);
    {
        TimedScope ts("percentile_finish");
        for (int first = 0; first < npct; first += PCT_MAX) {
            pl.np = std::min(PCT_MAX, npct - first);
            for (int j = 0; j < pl.np; j++) {
                pl.pct[j] = percentages[order[first + j]];
                pl.row[j] = (uint32_t)order[first + j];
            }
            if (pl.ncell < (uint64_t)PCT_CPB) launch_percentile<1, PCT_AXIS_THREADS>(grid, pl, dout.as<double>());
            else if (pl.N >= 256) launch_percentile<PCT_CPB, 8>(grid, pl, dout.as<double>());
            else launch_percentile<PCT_CPB, 4>(grid, pl, dout.as<double>());
            VH_HIP(hipGetLastError());
        }
    }
    copy_to_host(out, dout.ptr, out_items * 8, stream());
    VH_HIP(hipStreamSynchronize(stream()));
    VH_API_END
}
