// Selections on HBM columns: the lasso's point-in-polygon test (vaexfast.cpp:1757-1775 pnpoly,
// driven by SelectionLasso.evaluate, selections.py:172-204) fused with the selection mode, and
// the mode combine of two masks (selections.py:11-36 _select_functions).
//
// k_pnpoly: every lane holds PP_RPT consecutive rows in registers and walks the edge list, which
// a workgroup stages in LDS in chunks of PP_CHUNK edges (every lane reads the same edge: the
// read broadcasts).  The crossing parity is carried across chunks, so nvert is not bounded by
// LDS.  A row outside the radius (or past n) gets testy = NaN: it straddles no edge, and a wave
// none of whose rows is inside skips the walk.  The quotient is evaluated only under the
// straddle test (the branch is skipped wave-wide when no lane takes it), so a horizontal edge's
// 0 / 0 never reaches the mask.  The arithmetic is the reference's, operation for operation, in
// float64 (-ffp-contract=off, IEEE division): masks are bit-identical to the C loop.
#include "common.hpp"

namespace vh {

constexpr int PP_THREADS = 256;
constexpr int PP_RPT = ROWS8;                  // rows per lane (consecutive: one wide load per column)
constexpr int PP_TILE = PP_THREADS * PP_RPT;   // rows per workgroup and step
constexpr int PP_CHUNK = 512;                  // edges staged in LDS at a time (16 KiB)

// edge i of the walk `for (i = 0, j = nvert - 1; i < nvert; j = i++)`: vertex i, the y of vertex
// j and vertx[j] - vertx[i] (formed on the host: the same subtraction, the same bits)
struct alignas(16) PpEdge {
    double vx, vy, vyj, dx;
};

enum { PP_LDS = 0, PP_GLOBAL = 1, PP_NOSKIP = 2 };  // 1, 2: the A/B variants of scripts/exp_select_lasso.py

__device__ __forceinline__ bool mode_apply(int mode, bool has_prev, bool p, bool c) {
    if (!has_prev) return mode == VH_SELECT_SUBTRACT ? !c : c;
    switch (mode) {
    case VH_SELECT_AND: return p && c;
    case VH_SELECT_OR: return p || c;
    case VH_SELECT_XOR: return p != c;
    case VH_SELECT_SUBTRACT: return p && !c;
    default: return c;  // replace
    }
}

__device__ __forceinline__ void store_mask8(uint8_t *out, uint64_t j, uint32_t cnt, bool al, const uint8_t (&m)[ROWS8]) {
    if (al && cnt == ROWS8) {
        uint2 w;
        __builtin_memcpy(&w, m, 8);
        *reinterpret_cast<uint2 *>(out + j) = w;
    } else {
#pragma unroll
        for (int u = 0; u < ROWS8; u++)
            if ((uint32_t)u < cnt) out[j + u] = m[u];
    }
}

// edges [e0, e1) against the lane's rows: bit u of c flips per crossing of row u
template <int VAR>
__device__ __forceinline__ uint32_t pp_walk(const PpEdge *edge, int e0, int e1, const double (&tx)[PP_RPT],
                                            const double (&ty)[PP_RPT], uint32_t c) {
    for (int e = e0; e < e1; e++) {
        const PpEdge E = edge[e];
#pragma unroll
        for (int u = 0; u < PP_RPT; u++) {
            const bool straddle = (E.vy > ty[u]) != (E.vyj > ty[u]);
            if (VAR == PP_NOSKIP) {
                const double q = E.dx * (ty[u] - E.vy) / (E.vyj - E.vy) + E.vx;
                c ^= (uint32_t)(straddle && tx[u] < q) << u;
            } else if (straddle) {
                const double q = E.dx * (ty[u] - E.vy) / (E.vyj - E.vy) + E.vx;
                if (tx[u] < q) c ^= 1u << u;
            }
        }
    }
    return c;
}

template <typename TX, typename TY, int VAR>
__global__ __launch_bounds__(PP_THREADS) void k_pnpoly(const TX *x, const TY *y, uint64_t n, const PpEdge *edges, int nvert,
                                                       double meanx, double meany, double r2, const uint8_t *prev,
                                                       int mode, uint8_t *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    PpEdge *s_edge = reinterpret_cast<PpEdge *>(s_raw);
    const bool al_x = aligned_rows8(x, sizeof(TX)), al_y = aligned_rows8(y, sizeof(TY));
    const bool al_p = prev && aligned_rows8(prev, 1), al_o = aligned_rows8(out, 1);
    const int nchunks = VAR == PP_GLOBAL ? 1 : (nvert + PP_CHUNK - 1) / PP_CHUNK;
    auto stage = [&](int e0, int e1) {
        for (int e = e0 + (int)threadIdx.x; e < e1; e += PP_THREADS) s_edge[e - e0] = edges[e];
    };
    if (VAR != PP_GLOBAL && nchunks == 1) {
        stage(0, nvert);
        __syncthreads();
    }
    const uint64_t tiles = (n + PP_TILE - 1) / PP_TILE;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t j = t * PP_TILE + (uint64_t)threadIdx.x * PP_RPT;
        const uint32_t cnt = j >= n ? 0u : (uint32_t)(n - j < PP_RPT ? n - j : PP_RPT);
        TX rx[PP_RPT];
        TY ry[PP_RPT];
        load_rows8(x, j, cnt, al_x, rx);
        load_rows8(y, j, cnt, al_y, ry);
        double tx[PP_RPT], ty[PP_RPT];
        bool any = false;
#pragma unroll
        for (int u = 0; u < PP_RPT; u++) {
            tx[u] = (double)rx[u];
            ty[u] = (double)ry[u];
            const double d = (tx[u] - meanx) * (tx[u] - meanx) + (ty[u] - meany) * (ty[u] - meany);
            const bool in = (uint32_t)u < cnt && d < r2;
            if (!in) ty[u] = __builtin_nan("");
            any = any || in;
        }
        const bool wave_any = __ballot(any) != 0;
        uint32_t c = 0;
        if (VAR == PP_GLOBAL) {
            if (wave_any) c = pp_walk<VAR>(edges, 0, nvert, tx, ty, c);
        } else if (nchunks == 1) {
            if (wave_any) c = pp_walk<VAR>(s_edge, 0, nvert, tx, ty, c);
        } else {
            for (int ch = 0; ch < nchunks; ch++) {
                const int e0 = ch * PP_CHUNK, e1 = min(nvert, e0 + PP_CHUNK);
                __syncthreads();  // the walkers of the chunk before
                stage(e0, e1);
                __syncthreads();
                if (wave_any) c = pp_walk<VAR>(s_edge, 0, e1 - e0, tx, ty, c);
            }
        }
        uint8_t pv[ROWS8] = {};
        if (prev) load_rows8(prev, j, cnt, al_p, pv);
        uint8_t m[ROWS8];
#pragma unroll
        for (int u = 0; u < PP_RPT; u++) m[u] = mode_apply(mode, prev != nullptr, pv[u] == 1, (c >> u) & 1u) ? 1 : 0;
        store_mask8(out, j, cnt, al_o, m);
    }
}

// out = mode(a == 1, b == 1); b null: out = !(a == 1).  out may be a or b.
__global__ __launch_bounds__(256) void k_mask_combine(const uint8_t *a, const uint8_t *b, int mode, uint64_t n, uint8_t *out) {
    const bool al_a = aligned_rows8(a, 1), al_b = b && aligned_rows8(b, 1), al_o = aligned_rows8(out, 1);
    for (uint64_t j = (blockIdx.x * 256ull + threadIdx.x) * ROWS8; j < n; j += (uint64_t)gridDim.x * 256 * ROWS8) {
        const uint32_t cnt = (uint32_t)(n - j < ROWS8 ? n - j : ROWS8);
        uint8_t va[ROWS8], vb[ROWS8] = {}, m[ROWS8];
        load_rows8(a, j, cnt, al_a, va);
        if (b) load_rows8(b, j, cnt, al_b, vb);
#pragma unroll
        for (int u = 0; u < ROWS8; u++) m[u] = (b ? mode_apply(mode, true, va[u] == 1, vb[u] == 1) : va[u] != 1) ? 1 : 0;
        store_mask8(out, j, cnt, al_o, m);
    }
}

static int pp_variant() {  // VH_PNPOLY_VARIANT=1 / 2: the A/B kernels (float64 columns only)
    const char *e = getenv("VH_PNPOLY_VARIANT");
    return e && (e[0] == '1' || e[0] == '2') && e[1] == 0 ? e[0] - '0' : PP_LDS;
}

template <typename TX, typename TY, int VAR>
static void pp_launch(const void *x, const void *y, uint64_t n, const PpEdge *edges, int nvert, double meanx, double meany,
                      double r2, const uint8_t *prev, int mode, uint8_t *out) {
    const size_t lds = VAR == PP_GLOBAL ? 0 : sizeof(PpEdge) * (size_t)std::min(nvert, PP_CHUNK);
    const uint64_t tiles = (n + PP_TILE - 1) / PP_TILE;
    const unsigned grid = (unsigned)std::min<uint64_t>(tiles, (uint64_t)cu_count() * 8);
    hipLaunchKernelGGL((k_pnpoly<TX, TY, VAR>), dim3(grid), dim3(PP_THREADS), lds, stream(), static_cast<const TX *>(x),
                       static_cast<const TY *>(y), n, edges, nvert, meanx, meany, r2, prev, mode, out);
    VH_HIP(hipGetLastError());
}

template <typename TX, typename TY>
static void pp_dispatch(int var, const void *x, const void *y, uint64_t n, const PpEdge *edges, int nvert, double meanx,
                        double meany, double r2, const uint8_t *prev, int mode, uint8_t *out) {
    if constexpr (std::is_same<TX, double>::value && std::is_same<TY, double>::value) {
        if (var == PP_GLOBAL) return pp_launch<TX, TY, PP_GLOBAL>(x, y, n, edges, nvert, meanx, meany, r2, prev, mode, out);
        if (var == PP_NOSKIP) return pp_launch<TX, TY, PP_NOSKIP>(x, y, n, edges, nvert, meanx, meany, r2, prev, mode, out);
    }
    pp_launch<TX, TY, PP_LDS>(x, y, n, edges, nvert, meanx, meany, r2, prev, mode, out);
}

}  // namespace vh

using namespace vh;

extern "C" int vh_pnpoly(const void *x, int x_dtype, const void *y, int y_dtype, uint64_t n, const double *vertx,
                         const double *verty, int nvert, double meanx, double meany, double radius, const uint8_t *prev,
                         int mode, uint8_t *out) {
    VH_API_BEGIN
    if ((x_dtype != VH_F64 && x_dtype != VH_F32) || (y_dtype != VH_F64 && y_dtype != VH_F32))
        fail(VH_ERR_ARG, "vh_pnpoly: x and y must be float64 or float32 columns");
    if (nvert < 0 || (nvert > 0 && (!vertx || !verty))) fail(VH_ERR_ARG, "vh_pnpoly: bad vertex arrays");
    if (mode < VH_SELECT_REPLACE || mode > VH_SELECT_SUBTRACT) fail(VH_ERR_ARG, "vh_pnpoly: unknown mode");
    if (n == 0) return VH_OK;
    if (!x || !y || !out) fail(VH_ERR_ARG, "vh_pnpoly: null column");
    DevBuf dev;
    if (nvert) {
        std::vector<PpEdge> edges((size_t)nvert);
        for (int i = 0, j = nvert - 1; i < nvert; j = i++) edges[i] = PpEdge{vertx[i], verty[i], verty[j], vertx[j] - vertx[i]};
        dev.ensure(sizeof(PpEdge) * (uint64_t)nvert);
        // pageable source: staged by the runtime before the call returns, so `edges` may go
        VH_HIP(hipMemcpyAsync(dev.ptr, edges.data(), sizeof(PpEdge) * (size_t)nvert, hipMemcpyHostToDevice, stream()));
    }
    TimedScope ts("pnpoly");
    const int var = pp_variant();
    const double r2 = radius * radius;
    const PpEdge *e = dev.as<PpEdge>();
    if (x_dtype == VH_F64 && y_dtype == VH_F64) pp_dispatch<double, double>(var, x, y, n, e, nvert, meanx, meany, r2, prev, mode, out);
    else if (x_dtype == VH_F64) pp_dispatch<double, float>(var, x, y, n, e, nvert, meanx, meany, r2, prev, mode, out);
    else if (y_dtype == VH_F64) pp_dispatch<float, double>(var, x, y, n, e, nvert, meanx, meany, r2, prev, mode, out);
    else pp_dispatch<float, float>(var, x, y, n, e, nvert, meanx, meany, r2, prev, mode, out);
    VH_API_END
}

extern "C" int vh_mask_combine(const uint8_t *a, const uint8_t *b, int mode, uint64_t n, uint8_t *out) {
    VH_API_BEGIN
    if (mode < VH_SELECT_REPLACE || mode > VH_SELECT_SUBTRACT) fail(VH_ERR_ARG, "vh_mask_combine: unknown mode");
    if (n == 0) return VH_OK;
    if (!a || !out) fail(VH_ERR_ARG, "vh_mask_combine: null mask");
    TimedScope ts("mask_combine");
    hipLaunchKernelGGL(k_mask_combine, dim3(blocks_for((n + ROWS8 - 1) / ROWS8, 256)), dim3(256), 0, stream(), a, b, mode, n, out);
    VH_HIP(hipGetLastError());
    VH_API_END
}
