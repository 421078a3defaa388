// mutual_information finish on the device: the reference counts over [x, y] + binby, casts the
// grid to float64 and calls kld.mutual_information on the x-y slab of every binby cell in a
// Python loop (dataframe.py:622-718, kld.py:13-21, utils.py:119-142).  Here the edges=True count
// grid stays in HBM and is read at most twice; only one float64 per binby cell is read back.
//
// Binners 0 and 1 are the x and y axes (x has stride 1, y has stride Mx + 3: one outer cell's
// x-y slab is contiguous), binners 2.. the outer axes.  Per outer central cell, over the central
// Mx x My part of its slab (every edge slot of every axis is skipped by index arithmetic):
//
//   pass 1  T = sum a, rx[i] = sum_j a[i,j], cy[j] = sum_i a[i,j], all int64 (exact, so integer
//           atomics are used freely)
//   pass 2  for a > 0: p = a / T, q = (double(rx[i]) * double(cy[j])) / (T * T), term p * log(p / q)
//           in float64 (-ffp-contract=off); T * T is the closed form of the reference's Q.sum()
//
// Both passes sweep a region the same way: a wave takes 64 / XP rows at a time, XP = the power
// of two >= min(Mx, 64) lanes along x (stride 1, so a wave's load is one contiguous run per
// row), and steps along x in XP-wide chunks.  A row belongs to one wave, which reduces its sum
// with xor shuffles; rx goes through int64 LDS atomics (distinct addresses within a wave).
// The float64 terms are summed per lane in sweep order, per wave by a shuffle tree, over the
// waves and tiles in index order: a fixed order given the shape, no floating-point atomics.
//
// Two mappings, chosen on the host from the slab size alone:
//   cell   Mx * My <= MI_CELL_ITEMS: one 256-thread workgroup per outer cell, one launch, the
//          marginals in LDS, the slab's second read expected from the CU's L1 or the L2
//   split  larger slabs: the slab is cut into tiles of <= MI_TILE_W columns and about
//          MI_TILE_ITEMS entries, one workgroup per (cell, tile): k_mi_marginals adds the tile's
//          marginals into a zeroed int64 scratch [T, rx, cy] per cell (rx through LDS, one global
//          atomic per column, row and tile), k_mi_terms writes one partial per workgroup,
//          k_mi_sum adds a cell's partials (lanes strided over the tiles, shuffle tree)
#include <algorithm>
#include <cmath>

#include "engine.hpp"

using namespace vh;

namespace {
constexpr int MI_THREADS = 256;
constexpr uint64_t MI_CELL_ITEMS = 4096;  // central slab entries up to which one workgroup takes a cell
constexpr uint32_t MI_TILE_W = 1024;      // split mapping: columns per tile (8 KB of LDS for rx)
constexpr uint32_t MI_TILE_ITEMS = 4096;  // split mapping: entries per tile (16 per thread)

struct MiPlan {
    int32_t nd_outer, xp_log2;  // outer axes; log2 of the lanes along x
    uint32_t Mx, My;            // central bins of the x and y axes
    uint32_t tw, th, ntx, nty;  // split mapping: tile width / height, tiles along x / y
    uint64_t sy;                // stride of the y axis (Mx + 3)
    uint64_t ncell;             // outer central cells
    uint64_t cshape[MAX_DIM];   // central shape (shape - 3) of every outer axis
    uint64_t stride[MAX_DIM];
};

// central entry (0, 0) of an outer cell's slab: the 3 edge slots of every axis are skipped
__device__ inline const int64_t *mi_slab(const int64_t *grid, const MiPlan &pl, uint64_t cell) {
    uint64_t base = 2 + 2 * pl.sy;
    for (int d = 0; d < pl.nd_outer; d++) {
        const uint64_t i = cell % pl.cshape[d];
        cell /= pl.cshape[d];
        base += (i + 2) * pl.stride[d];
    }
    return grid + base;
}

__device__ inline void mi_add(int64_t *p, int64_t v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}

// marginals of the region [i0, i1) x [j0, j1): s_rx[i - i0] (LDS) and cy[j] (LDS: stored, a row
// has one owner; GLOBAL: added, other tiles hold the rest of the row); returns the sum of the
// rows this lane reported (non-zero on the first lane of a row only)
template <bool GLOBAL>
__device__ inline int64_t mi_pass1(const int64_t *slab, const MiPlan &pl, uint32_t i0, uint32_t i1, uint32_t j0,
                                   uint32_t j1, int64_t *s_rx, int64_t *cy) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const uint32_t xp = 1u << pl.xp_log2, rows = 64u >> pl.xp_log2;
    const uint32_t lx = lane & (xp - 1), sub = lane >> pl.xp_log2;
    int64_t tot = 0;
    for (uint32_t jb = j0 + wave * rows; jb < j1; jb += nw * rows) {
        const uint32_t j = jb + sub;
        const bool rv = j < j1;
        const int64_t *row = slab + (uint64_t)j * pl.sy;
        long long rs = 0;
#pragma unroll 4
        for (uint32_t ib = i0; ib < i1; ib += xp) {
            const uint32_t i = ib + lx;
            const int64_t a = rv && i < i1 ? row[i] : 0;
            rs += a;
            if (a) mi_add(&s_rx[i - i0], a);
        }
        for (uint32_t off = xp >> 1; off; off >>= 1) rs += __shfl_xor(rs, (int)off, 64);
        if (rv && lx == 0) {
            if constexpr (GLOBAL) {
                if (rs) mi_add(&cy[j], rs);
            } else {
                cy[j] = rs;
            }
            tot += rs;
        }
    }
    return tot;
}

// this lane's terms of the region, summed in sweep order; rx and cy are indexed by i and j
__device__ inline double mi_pass2(const int64_t *slab, const MiPlan &pl, uint32_t i0, uint32_t i1, uint32_t j0,
                                  uint32_t j1, const int64_t *rx, const int64_t *cy, int64_t T) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const uint32_t xp = 1u << pl.xp_log2, rows = 64u >> pl.xp_log2;
    const uint32_t lx = lane & (xp - 1), sub = lane >> pl.xp_log2;
    const double dT = (double)T, TT = dT * dT;
    double acc = 0.0;
    for (uint32_t jb = j0 + wave * rows; jb < j1; jb += nw * rows) {
        const uint32_t j = jb + sub;
        const bool rv = j < j1;
        const int64_t *row = slab + (uint64_t)j * pl.sy;
        const double dcy = rv ? (double)cy[j] : 0.0;
#pragma unroll 4
        for (uint32_t ib = i0; ib < i1; ib += xp) {
            const uint32_t i = ib + lx;
            const int64_t a = rv && i < i1 ? row[i] : 0;
            if (a > 0) {
                const double p = (double)a / dT;
                const double q = ((double)rx[i] * dcy) / TT;
                acc += p * log(p / q);
            }
        }
    }
    return acc;
}

// the workgroup's sum of acc, waves in index order; valid in thread 0
__device__ inline double mi_block_sum(double acc, double *s_part) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int off = 32; off; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) s_part[wave] = acc;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0)
        for (uint32_t w = 0; w < nw; w++) r += s_part[w];
    return r;
}

// ---- cell mapping: one workgroup per outer cell, marginals in LDS ----------------------------
constexpr size_t mi_cell_lds(uint64_t Mx, uint64_t My) { return (Mx + My + 1) * 8 + (MI_THREADS / 64) * 8; }

__global__ __launch_bounds__(MI_THREADS) void k_mi_cell(const int64_t *__restrict__ grid, const MiPlan pl,
                                                        double *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char mi_smem[];
    int64_t *s_rx = reinterpret_cast<int64_t *>(mi_smem);
    int64_t *s_cy = s_rx + pl.Mx, *s_tot = s_cy + pl.My;
    double *s_part = reinterpret_cast<double *>(s_tot + 1);
    const uint64_t cell = blockIdx.x;
    const int64_t *slab = mi_slab(grid, pl, cell);
    for (uint32_t k = threadIdx.x; k <= pl.Mx + pl.My; k += MI_THREADS) s_rx[k] = 0;  // rx, cy and the total
    __syncthreads();
    const int64_t tot = mi_pass1<false>(slab, pl, 0, pl.Mx, 0, pl.My, s_rx, s_cy);
    if (tot) mi_add(s_tot, tot);
    __syncthreads();
    const double r = mi_block_sum(mi_pass2(slab, pl, 0, pl.Mx, 0, pl.My, s_rx, s_cy, *s_tot), s_part);
    if (threadIdx.x == 0) out[cell] = r;
}

// ---- split mapping: one workgroup per (cell, tile), marginals in a global int64 scratch -------
struct MiTile {
    uint64_t cell;
    uint32_t i0, i1, j0, j1;
};
__device__ inline MiTile mi_tile(const MiPlan &pl) {
    const uint32_t ntiles = pl.ntx * pl.nty;
    const uint32_t t = blockIdx.x % ntiles, tx = t % pl.ntx, ty = t / pl.ntx;
    MiTile m;
    m.cell = blockIdx.x / ntiles;
    m.i0 = tx * pl.tw;
    m.i1 = min(m.i0 + pl.tw, pl.Mx);
    m.j0 = ty * pl.th;
    m.j1 = min(m.j0 + pl.th, pl.My);
    return m;
}

// scratch per cell: [T, rx[Mx], cy[My]], zeroed before the launch
__global__ __launch_bounds__(MI_THREADS) void k_mi_marginals(const int64_t *__restrict__ grid, const MiPlan pl,
                                                             int64_t *__restrict__ scratch) {
    __shared__ int64_t s_rx[MI_TILE_W];
    __shared__ int64_t s_tot;
    const MiTile m = mi_tile(pl);
    int64_t *cs = scratch + m.cell * (1 + (uint64_t)pl.Mx + pl.My);
    const uint32_t w = m.i1 - m.i0;
    for (uint32_t k = threadIdx.x; k < w; k += MI_THREADS) s_rx[k] = 0;
    if (threadIdx.x == 0) s_tot = 0;
    __syncthreads();
    const int64_t tot = mi_pass1<true>(mi_slab(grid, pl, m.cell), pl, m.i0, m.i1, m.j0, m.j1, s_rx, cs + 1 + pl.Mx);
    if (tot) mi_add(&s_tot, tot);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < w; k += MI_THREADS)
        if (s_rx[k]) mi_add(&cs[1 + m.i0 + k], s_rx[k]);
    if (threadIdx.x == 0 && s_tot) mi_add(cs, s_tot);
}

__global__ __launch_bounds__(MI_THREADS) void k_mi_terms(const int64_t *__restrict__ grid, const MiPlan pl,
                                                         const int64_t *__restrict__ scratch,
                                                         double *__restrict__ partials) {
    __shared__ double s_part[MI_THREADS / 64];
    const MiTile m = mi_tile(pl);
    const int64_t *cs = scratch + m.cell * (1 + (uint64_t)pl.Mx + pl.My);
    const double acc = mi_pass2(mi_slab(grid, pl, m.cell), pl, m.i0, m.i1, m.j0, m.j1, cs + 1, cs + 1 + pl.Mx, cs[0]);
    const double r = mi_block_sum(acc, s_part);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// one wave per cell: lane l adds the partials of tiles l, l + 64, ..., then a shuffle tree
__global__ __launch_bounds__(MI_THREADS) void k_mi_sum(const double *__restrict__ partials, uint32_t ntiles,
                                                       uint64_t ncell, double *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t cell = (uint64_t)blockIdx.x * (MI_THREADS / 64) + (threadIdx.x >> 6);
    if (cell >= ncell) return;
    const double *p = partials + cell * ntiles;
    double acc = 0.0;
    for (uint32_t t = lane; t < ntiles; t += 64) acc += p[t];
#pragma unroll
    for (int off = 32; off; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) out[cell] = acc;
}

int log2_ceil(uint32_t v) {
    int l = 0;
    while ((1u << l) < v) l++;
    return l;
}
static_assert(mi_cell_lds(MI_CELL_ITEMS, 1) <= 64 * 1024, "k_mi_cell: dynamic LDS above the default limit");
}  // namespace

extern "C" int vh_agg_mutual_information(vh_agg *a, double *out, uint64_t out_items) {
    VH_API_BEGIN
    if (!a || !a->grid) fail(VH_ERR_ARG, "mutual_information: no aggregator");
    std::lock_guard<std::mutex> lk(a->grid->mu);
    const vh_grid *g = a->grid;
    if (a->kind != VH_AGG_COUNT || a->grid_dtype != VH_I64)
        fail(VH_ERR_ARG, "mutual_information: not an AggCount with an int64 grid");
    const int nd = (int)g->binners.size();
    if (nd < 2) fail(VH_ERR_ARG, "mutual_information: fewer than 2 binners (the first two are the x and y axes)");
    if (nd > MAX_DIM) fail(VH_ERR_ARG, "mutual_information: too many binners");
    for (int d = 0; d < 2; d++)
        if (g->shapes[d] < 4 || g->shapes[d] - 3 > 0x3fffffffull)
            fail(VH_ERR_ARG, std::string("mutual_information: bad ") + (d ? "y" : "x") + " axis (shape " +
                                 std::to_string(g->shapes[d]) + ", at least 4 with the 3 edge slots)");

    MiPlan pl{};
    pl.nd_outer = nd - 2;
    pl.Mx = (uint32_t)(g->shapes[0] - 3);
    pl.My = (uint32_t)(g->shapes[1] - 3);
    pl.sy = g->strides[1];
    pl.ncell = 1;
    for (int d = 2; d < nd; d++) {
        pl.cshape[d - 2] = g->shapes[d] >= 3 ? g->shapes[d] - 3 : 0;
        pl.stride[d - 2] = g->strides[d];
        pl.ncell *= pl.cshape[d - 2];
    }
    if (out_items != pl.ncell) fail(VH_ERR_ARG, "mutual_information: output size mismatch");
    if (pl.ncell == 0) return VH_OK;
    if (!out) fail(VH_ERR_ARG, "mutual_information: no output");

    const uint64_t items = (uint64_t)pl.Mx * pl.My;
    const bool split = items > MI_CELL_ITEMS;
    pl.tw = std::min(pl.Mx, MI_TILE_W);
    pl.th = std::min(pl.My, std::max(1u, MI_TILE_ITEMS / pl.tw));
    pl.ntx = (pl.Mx + pl.tw - 1) / pl.tw;
    pl.nty = (pl.My + pl.th - 1) / pl.th;
    pl.xp_log2 = log2_ceil(std::min(pl.tw, 64u));
    const uint64_t ntiles = (uint64_t)pl.ntx * pl.nty;
    const uint64_t blocks = split ? pl.ncell * ntiles : pl.ncell;
    // one launch: its threads (workgroups x MI_THREADS) must stay below 2^32
    if (ntiles > 0xffffffffull / MI_THREADS || blocks > 0xffffffffull / MI_THREADS)
        fail(VH_ERR_ARG, "mutual_information: too many cells for one launch (" + std::to_string(blocks) + " workgroups)");

    DevBuf dout, scratch, partials;
    dout.ensure(out_items * 8);
    const auto *grid = static_cast<const int64_t *>(a->g.ptr);
    {
        TimedScope ts("mutual_information_finish");
        if (!split) {
            hipLaunchKernelGGL(k_mi_cell, dim3((unsigned)blocks), dim3(MI_THREADS), mi_cell_lds(pl.Mx, pl.My), stream(),
                               grid, pl, dout.as<double>());
        } else {
            const uint64_t sbytes = pl.ncell * (1 + (uint64_t)pl.Mx + pl.My) * 8;
            scratch.ensure(sbytes);
            partials.ensure(blocks * 8);
            VH_HIP(hipMemsetAsync(scratch.ptr, 0, sbytes, stream()));
            hipLaunchKernelGGL(k_mi_marginals, dim3((unsigned)blocks), dim3(MI_THREADS), 0, stream(), grid, pl,
                               scratch.as<int64_t>());
            hipLaunchKernelGGL(k_mi_terms, dim3((unsigned)blocks), dim3(MI_THREADS), 0, stream(), grid, pl,
                               scratch.as<int64_t>(), partials.as<double>());
            const uint64_t sum_blocks = (pl.ncell + MI_THREADS / 64 - 1) / (MI_THREADS / 64);
            hipLaunchKernelGGL(k_mi_sum, dim3((unsigned)sum_blocks), dim3(MI_THREADS), 0, stream(),
                               partials.as<double>(), (uint32_t)ntiles, pl.ncell, dout.as<double>());
        }
        VH_HIP(hipGetLastError());
    }
    copy_to_host(out, dout.ptr, out_items * 8, stream());
    VH_HIP(hipStreamSynchronize(stream()));
    VH_API_END
}
