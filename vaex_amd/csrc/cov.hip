// AggCov -- the reference's OP_COV statistic (op_cov, vaexfast.cpp:1070-1104, driven by
// TaskStatistic, tasks.py:191-201) as a superagg aggregator: N float64 value columns, per grid
// cell the counts, sums, pairwise counts and pairwise product sums that DataFrame.cov /
// covar / correlation finish on the host.  A row's cell comes from this project's binners
// (NaN, underflow and overflow slots included), not from statisticNd's own scaling.
//
// The HBM grid keeps only the distinct accumulators (engine.hpp: 2N + N^2 float64 per cell,
// contiguous); cov_download / cov_upload translate to and from the reference's 2N + 2N^2
// fields.  Counts are float64 like the reference's (exact below 2^53 rows).
//
// Three regimes:
//   k_cov0       no binners (L == 1), N <= 4: accumulators in registers over a grid-stride
//                sweep, wave + workgroup reduction, one atomic per accumulator and workgroup
//   k_cov_cells<LDS>   the accumulators of the whole grid fit LDS_AGG_MAX_BYTES: a
//                per-workgroup sub-grid in LDS (replicated when it is tiny, so the lanes of a
//                wave do not queue on one address), flushed once per workgroup
//   k_cov_cells<!LDS>  everything larger: global float64 atomics on the cell's accumulators
#include "common.hpp"
#include "engine.hpp"

namespace vh {
namespace {

// Every accumulator one row feeds, as add(k, term, pred): k is the accumulator's index in the
// cell.  NT > 0 fixes N at compile time; NT == 0 takes it from `nrt`, with the loops unrolled to
// COV_MAX_N and guarded so `v` is only ever indexed by constants (it stays in registers).  A row
// the data mask drops arrives as all-NaN values: it feeds nothing.
template <int NT, typename F>
__device__ __forceinline__ void cov_terms(int nrt, const double (&v)[NT ? NT : COV_MAX_N], F &&add) {
    constexpr int M = NT ? NT : COV_MAX_N;
    const int N = NT ? NT : nrt;
    const int pc0 = 2 * N, ps0 = 2 * N + N * (N - 1) / 2;
#pragma unroll
    for (int c = 0; c < M; c++) {
        if (c < N) {
            const bool nc = v[c] == v[c];
            add(c, 1.0, nc);
            add(N + c, v[c], nc);
#pragma unroll
            for (int r = 0; r <= c; r++) {
                const bool both = nc && v[r] == v[r];
                if (r < c) add(pc0 + c * (c - 1) / 2 + r, 1.0, both);
                // float64 product, -ffp-contract=off: inf * 0 is a NaN term like the reference's
                add(ps0 + c * (c + 1) / 2 + r, v[r] * v[c], both);
            }
        }
    }
}

__device__ __forceinline__ double cov_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// ---- no binners: registers ---------------------------------------------------------------
template <int N> __global__ __launch_bounds__(256) void k_cov0(CovDev cd, uint64_t n, int vec) {
    constexpr int C = (int)cov_accs(N);
    double acc[C];
#pragma unroll
    for (int k = 0; k < C; k++) acc[k] = 0.0;
    auto add = [&](int k, double x, bool p) { acc[k] += p ? x : 0.0; };
    const uint64_t tid = blockIdx.x * 256ull + threadIdx.x, step = gridDim.x * 256ull;
    if (vec) {
        // every column 16-byte aligned: two rows per load
        const uint64_t n2 = n >> 1;
        for (uint64_t j = tid; j < n2; j += step) {
            double2 w[N];
#pragma unroll
            for (int c = 0; c < N; c++) w[c] = reinterpret_cast<const double2 *>(cd.col[c])[j];
            bool k0 = true, k1 = true;
            if (cd.mask) {
                k0 = cd.mask[2 * j] == 1;
                k1 = cd.mask[2 * j + 1] == 1;
            }
            double v[N];
#pragma unroll
            for (int c = 0; c < N; c++) v[c] = k0 ? w[c].x : cov_nan();
            cov_terms<N>(N, v, add);
#pragma unroll
            for (int c = 0; c < N; c++) v[c] = k1 ? w[c].y : cov_nan();
            cov_terms<N>(N, v, add);
        }
        if ((n & 1) && tid == 0) {
            const bool k0 = !cd.mask || cd.mask[n - 1] == 1;
            double v[N];
#pragma unroll
            for (int c = 0; c < N; c++) v[c] = k0 ? cd.col[c][n - 1] : cov_nan();
            cov_terms<N>(N, v, add);
        }
    } else {
        for (uint64_t j = tid; j < n; j += step) {
            const bool k0 = !cd.mask || cd.mask[j] == 1;
            double v[N];
#pragma unroll
            for (int c = 0; c < N; c++) v[c] = k0 ? cd.col[c][j] : cov_nan();
            cov_terms<N>(N, v, add);
        }
    }
    // wave reduction, then the workgroup's four waves, then one atomic per accumulator
    __shared__ double part[4][C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < C; k++) {
        double x = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if (lane == 0) part[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < C) {
        const double s = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        if (s != 0.0) atomicAdd(cd.grid + threadIdx.x, s);
    }
}

// ---- grids: LDS sub-grid per workgroup, or global atomics ---------------------------------
// LDS: accumulator k of cell c in replica q lives at lds[c * cstride + k * R + q], R = 1 <<
// rep_log2 replicas, a lane adds into replica lane % R: lanes of one wave whose rows share a
// cell hit consecutive words instead of one.  cstride = (C | 1) * R, an odd number of R-word
// groups: with an even one (N = 2: 8 accumulators = 64 B) the same accumulator of every cell
// falls on a few LDS banks and the lanes of a wave, each in another cell, queue on them
// (measured, 128 bins, 1e8 rows: N = 2 1.63 ms -> 0.65 ms; N = 3, whose 15 is odd, 1.15 ms).
// An odd stride in words instead would undo the replicas' spread (4 bins: 0.37 -> 0.55 ms).
// The flush folds the replicas and skips zeros (an untouched accumulator).
template <int NT, bool LDS>
__global__ __launch_bounds__(256) void k_cov_cells(CovDev cd, const uint16_t *cells, const uint64_t *idx, uint64_t n,
                                                   uint64_t L, uint32_t rep_log2) {
    constexpr int M = NT ? NT : COV_MAX_N;
    const int N = NT ? NT : cd.n;
    const uint32_t C = (uint32_t)(2 * N + N * N);
    extern __shared__ __align__(16) double lds[];
    const uint32_t tot = LDS ? (uint32_t)L * C : 0;
    const uint32_t cstride = (C | 1) << rep_log2;
    if constexpr (LDS) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)L * cstride; i += 256) lds[i] = 0.0;
        __syncthreads();
    }
    const uint32_t rep = threadIdx.x & ((1u << rep_log2) - 1);
    const uint64_t step = gridDim.x * 256ull;
    for (uint64_t j = blockIdx.x * 256ull + threadIdx.x; j < n; j += step) {
        const bool keep = !cd.mask || cd.mask[j] == 1;
        const uint64_t cell = cells ? (uint64_t)cells[j] : idx ? idx[j] : 0;
        double v[M];
#pragma unroll
        for (int c = 0; c < M; c++) v[c] = (c < N && keep) ? cd.col[c][j] : cov_nan();
        if constexpr (LDS) {
            double *base = lds + (uint32_t)cell * cstride + rep;
            cov_terms<NT>(N, v, [&](int k, double x, bool p) {
                if (p) atomicAdd(base + ((uint32_t)k << rep_log2), x);
            });
        } else {
            double *base = cd.grid + cell * C;
            cov_terms<NT>(N, v, [&](int k, double x, bool p) {
                if (p) atomicAdd(base + k, x);
            });
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < tot; i += 256) {
            const double *src = lds + (i / C) * cstride + ((i % C) << rep_log2);
            double s = 0.0;
            for (uint32_t q = 0; q < (1u << rep_log2); q++) s += src[q];
            if (s != 0.0) atomicAdd(cd.grid + i, s);
        }
    }
}

// ---- the reference's field layout <-> the distinct accumulators -----------------------------
__global__ __launch_bounds__(256) void k_cov_expand(const double *acc, double *out, uint64_t L, int N) {
    const uint64_t C = cov_accs(N), F = cov_fields(N), NN = (uint64_t)N * N;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < L * F; i += gridDim.x * 256ull) {
        const uint64_t cell = i / F, f = i % F;
        const double *a = acc + cell * C;
        double x;
        if (f < 2ull * N) {
            x = a[f];
        } else {
            const bool sums = f >= 2ull * N + NN;
            const uint64_t e = f - 2ull * N - (sums ? NN : 0), r = e % N, c = e / N;
            const uint64_t lo = r < c ? r : c, hi = r < c ? c : r;
            if (sums) x = a[2 * N + N * (N - 1) / 2 + hi * (hi + 1) / 2 + lo];
            else x = lo == hi ? a[lo] : a[2 * N + hi * (hi - 1) / 2 + lo];
        }
        out[i] = x;
    }
}

// the upper triangle's entries are taken (index r + c * N, r <= c); the diagonal pair counts
// are the column counts
__global__ __launch_bounds__(256) void k_cov_compress(const double *in, double *acc, uint64_t L, int N) {
    const uint64_t C = cov_accs(N), F = cov_fields(N), NN = (uint64_t)N * N;
    const uint64_t npc = (uint64_t)N * (N - 1) / 2;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < L * C; i += gridDim.x * 256ull) {
        const uint64_t cell = i / C, k = i % C;
        const double *src = in + cell * F;
        double x;
        if (k < 2ull * N) {
            x = src[k];
        } else {
            const bool sums = k >= 2ull * N + npc;
            const uint64_t p = k - 2ull * N - (sums ? npc : 0);
            uint64_t hi = sums ? 0 : 1;  // counts: hi(hi-1)/2 <= p; sums: hi(hi+1)/2 <= p
            while ((sums ? (hi + 1) * (hi + 2) / 2 : (hi + 1) * hi / 2) <= p) hi++;
            const uint64_t lo = p - (sums ? hi * (hi + 1) / 2 : hi * (hi - 1) / 2);
            x = src[2ull * N + (sums ? NN : 0) + lo + hi * N];
        }
        acc[i] = x;
    }
}

}  // namespace

void cov_bin(const CovDev &cd, const uint16_t *cells, const uint64_t *idx, uint64_t len, uint64_t L) {
    if (!len) return;
    const int N = cd.n;
    const uint64_t C = cov_accs(N);
    const dim3 blk(256);
    if (L == 1 && N <= 4) {
        bool vec = true;
        for (int c = 0; c < N; c++) vec = vec && (reinterpret_cast<uintptr_t>(cd.col[c]) & 15) == 0;
        TimedScope ts("bin_cov_reduce");
        const dim3 grd(blocks_for((len + 1) / 2, 256, 8));
        switch (N) {
        case 1: hipLaunchKernelGGL(k_cov0<1>, grd, blk, 0, stream(), cd, len, (int)vec); break;
        case 2: hipLaunchKernelGGL(k_cov0<2>, grd, blk, 0, stream(), cd, len, (int)vec); break;
        case 3: hipLaunchKernelGGL(k_cov0<3>, grd, blk, 0, stream(), cd, len, (int)vec); break;
        default: hipLaunchKernelGGL(k_cov0<4>, grd, blk, 0, stream(), cd, len, (int)vec);
        }
        VH_HIP(hipGetLastError());
        return;
    }
    if (L > 1 && !cells && !idx) fail(VH_ERR_RUNTIME, "internal: AggCov without row cells");
    if (cov_fits_lds(L, N)) {
        // replicas while the sub-grid stays within 16 KB (several workgroups per CU)
        const uint64_t padded = L * (C | 1) * 8;  // one replica with the kernel's cell stride
        uint32_t rep_log2 = 0;
        while (rep_log2 < 6 && (padded << (rep_log2 + 1)) <= 16 * 1024) rep_log2++;
        const size_t shm = (size_t)(padded << rep_log2);
        const unsigned per_cu = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(8, (128 * 1024) / shm));
        const dim3 grd(blocks_for(len, 256, per_cu));
        TimedScope ts("bin_cov_lds");
        switch (N) {
        case 2: hipLaunchKernelGGL((k_cov_cells<2, true>), grd, blk, shm, stream(), cd, cells, idx, len, L, rep_log2); break;
        case 3: hipLaunchKernelGGL((k_cov_cells<3, true>), grd, blk, shm, stream(), cd, cells, idx, len, L, rep_log2); break;
        default: hipLaunchKernelGGL((k_cov_cells<0, true>), grd, blk, shm, stream(), cd, cells, idx, len, L, rep_log2);
        }
        VH_HIP(hipGetLastError());
        return;
    }
    TimedScope ts("bin_cov_global");
    const dim3 grd(blocks_for(len, 256, 8));
    switch (N) {
    case 2: hipLaunchKernelGGL((k_cov_cells<2, false>), grd, blk, 0, stream(), cd, cells, idx, len, L, 0u); break;
    case 3: hipLaunchKernelGGL((k_cov_cells<3, false>), grd, blk, 0, stream(), cd, cells, idx, len, L, 0u); break;
    default: hipLaunchKernelGGL((k_cov_cells<0, false>), grd, blk, 0, stream(), cd, cells, idx, len, L, 0u);
    }
    VH_HIP(hipGetLastError());
}

void cov_download(vh_agg *a, void *host, uint64_t bytes) {
    const uint64_t L = a->grid->length1d, items = L * cov_fields(a->moment);
    if (bytes != items * 8) fail(VH_ERR_ARG, "download size mismatch");
    if (!items) return;
    DevBuf tmp;
    tmp.ensure(bytes);
    hipLaunchKernelGGL(k_cov_expand, dim3(blocks_for(items, 256)), dim3(256), 0, stream(), a->g.as<double>(),
                       tmp.as<double>(), L, (int)a->moment);
    VH_HIP(hipGetLastError());
    copy_to_host(host, tmp.ptr, bytes, stream());
    VH_HIP(hipStreamSynchronize(stream()));
}

void cov_upload(vh_agg *a, const void *host, uint64_t bytes) {
    const uint64_t L = a->grid->length1d, items = L * cov_fields(a->moment);
    if (bytes != items * 8) fail(VH_ERR_ARG, "upload size mismatch");
    if (!items) return;
    DevBuf tmp;
    tmp.ensure(bytes);
    VH_HIP(hipMemcpyAsync(tmp.ptr, host, bytes, hipMemcpyHostToDevice, stream()));
    hipLaunchKernelGGL(k_cov_compress, dim3(blocks_for(L * cov_accs(a->moment), 256)), dim3(256), 0, stream(),
                       tmp.as<double>(), a->g.as<double>(), L, (int)a->moment);
    VH_HIP(hipGetLastError());
    VH_HIP(hipStreamSynchronize(stream()));
}

}  // namespace vh
