// Row order on the GPU: vh_argsort (the stable lexicographic order of up to SORT_MAX_KEYS key
// columns, over every row or over an ascending row list) and vh_mask_rows (that row list: the
// kept row numbers of a byte mask).  DataFrame.sort / extract (sort.py) and the compaction of
// evaluate on a filtered HBM frame are these two plus vh_take; Grouper(sort=True) orders its
// set's keys with the same argsort.
//
// The order is np.lexsort(keys[::-1]) (one key: np.argsort(kind="stable")): stable, NaN after
// every number and all NaN equal, -0.0 == 0.0.  descending = the exact reverse of it.
//
// The digit passes are rocprim::radix_sort_pairs.  What it cannot know is how few bits the
// keys need and how many keys fit one sort; that is decided here:
//   k_sort_range   one launch over all key columns (through `rows` when given): per key the
//                  min / max order-preserving code of the non-NaN rows and an any-NaN flag,
//                  reduced per wave, then one atomic per wave and key on a small HBM record.
//   sort_plan.hpp  (host) per key lo and span -> width; rounds of trailing keys whose widths
//                  sum to <= 64 bits; a round of <= 32 bits sorts 32-bit words.
//   k_sort_encode  per round: output position i reads its row (round 1: rows[i] or i; later the
//                  current permutation's entry), packs `code - lo` of the round's keys into
//                  one word (NaN packs `span`) and writes word and row.  SE_RPT consecutive
//                  positions per lane, 16-byte stores.  Later rounds gather their keys through
//                  the permutation: the only uncoalesced read of the pipeline.
//   rocPRIM then sorts (word, row) pairs over exactly bits [0, sum) of the round.
// descending: position i of the first round takes input position m-1-i and every round stores
// the complement of the word within its bits; the stable ascending sort of that is the exact
// reverse of the ascending result, with no extra pass.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.hpp"
#include "sort_plan.hpp"

namespace vh {

constexpr int SE_RPT = 4;  // consecutive output positions per lane (k_sort_encode): one tile = 1024
constexpr int SORT_THREADS = 256;
constexpr int SORT_REC_WORDS = 3;  // per key: min code, max code, any-NaN; then one word: a row out of range

// the switch of VH_DISPATCH_DTYPE for device code (an unknown code was refused on the host)
#define SORT_DEVICE_DTYPE(code, T, ...)                                                     \
    switch (code) {                                                                         \
    case VH_F64: { using T = double; __VA_ARGS__; break; }                                  \
    case VH_F32: { using T = float; __VA_ARGS__; break; }                                   \
    case VH_I64: { using T = int64_t; __VA_ARGS__; break; }                                 \
    case VH_I32: { using T = int32_t; __VA_ARGS__; break; }                                 \
    case VH_I16: { using T = int16_t; __VA_ARGS__; break; }                                 \
    case VH_I8: { using T = int8_t; __VA_ARGS__; break; }                                   \
    case VH_U64: { using T = uint64_t; __VA_ARGS__; break; }                                \
    case VH_U32: { using T = uint32_t; __VA_ARGS__; break; }                                \
    case VH_U16: { using T = uint16_t; __VA_ARGS__; break; }                                \
    case VH_U8: { using T = uint8_t; __VA_ARGS__; break; }                                  \
    case VH_BOOL: { using T = ::vh::vbool; __VA_ARGS__; break; }                            \
    default: break;                                                                         \
    }

// The order-preserving code of a key: unsigned integers as they are, signed integers with the
// sign bit of their own width flipped, floats with -0.0 folded to +0.0 and the sign-dependent
// flip in their own width (a float32 key needs at most 32 bits), bool 0 / 1.  Returns whether
// the key is NaN (it has no code then).
template <typename T> __device__ __forceinline__ bool sort_code(T v, uint64_t &code) {
    if constexpr (std::is_same_v<T, double>) {
        if (v != v) return true;
        const uint64_t u = v == 0.0 ? 0ULL : __builtin_bit_cast(uint64_t, v);
        code = (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
    } else if constexpr (std::is_same_v<T, float>) {
        if (v != v) return true;
        const uint32_t u = v == 0.0f ? 0u : __builtin_bit_cast(uint32_t, v);
        code = (u >> 31) ? (uint32_t)~u : (u | 0x80000000u);
    } else if constexpr (std::is_same_v<T, vbool>) {
        code = v.v ? 1 : 0;
    } else if constexpr (std::is_signed_v<T>) {
        using U = std::make_unsigned_t<T>;
        code = (U)((U)v ^ (U)((U)1 << (8 * sizeof(T) - 1)));
    } else {
        code = (uint64_t)v;
    }
    return false;
}

// ---- range ------------------------------------------------------------------------------------
struct SortKeys {
    const void *col[SORT_MAX_KEYS];
    int dtype[SORT_MAX_KEYS];
    int nkeys;
};

template <typename T, typename R>
__device__ __forceinline__ void sort_range_key(const T *col, const R *rows, uint64_t n, uint64_t m, uint64_t &lo,
                                               uint64_t &hi, bool &nan, bool &bad) {
    const uint64_t stride = (uint64_t)gridDim.x * SORT_THREADS;
    for (uint64_t i0 = blockIdx.x * (uint64_t)SORT_THREADS + threadIdx.x; i0 < m; i0 += SE_RPT * stride) {
        uint64_t row[SE_RPT];
        bool ok[SE_RPT];
        T v[SE_RPT];
        // the row numbers, then the keys, of SE_RPT strided positions are in flight together
#pragma unroll
        for (int u = 0; u < SE_RPT; u++) {
            const uint64_t i = i0 + u * stride;
            ok[u] = i < m;
            row[u] = !ok[u] ? 0 : rows ? (uint64_t)(int64_t)rows[i] : i;
            if (ok[u] && row[u] >= n) {  // a negative entry too: it was sign-extended
                bad = true;
                ok[u] = false;
            }
        }
#pragma unroll
        for (int u = 0; u < SE_RPT; u++) v[u] = ok[u] ? col[row[u]] : T{};
#pragma unroll
        for (int u = 0; u < SE_RPT; u++) {
            uint64_t c = 0;
            const bool isnan = sort_code(v[u], c);
            if (!ok[u]) continue;
            if (isnan) {
                nan = true;
            } else {
                lo = min(lo, c);
                hi = max(hi, c);
            }
        }
    }
}

template <typename R>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_range(SortKeys a, const R *rows, uint64_t n, uint64_t m,
                                                             unsigned long long *rec) {
    const int lane = threadIdx.x & 63;
    bool bad = false;
    for (int k = 0; k < a.nkeys; k++) {
        uint64_t lo = ~0ULL, hi = 0;
        bool nan = false;
        SORT_DEVICE_DTYPE(a.dtype[k], T, sort_range_key<T, R>(static_cast<const T *>(a.col[k]), rows, n, m, lo, hi, nan, bad));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo = min(lo, (uint64_t)__shfl_xor((unsigned long long)lo, off, 64));
            hi = max(hi, (uint64_t)__shfl_xor((unsigned long long)hi, off, 64));
        }
        const bool any_nan = __ballot(nan) != 0;
        if (lane == 0) {
            if (lo <= hi) {
                atomicMin(&rec[SORT_REC_WORDS * k], (unsigned long long)lo);
                atomicMax(&rec[SORT_REC_WORDS * k + 1], (unsigned long long)hi);
            }
            if (any_nan) atomicOr(&rec[SORT_REC_WORDS * k + 2], 1ULL);
        }
    }
    const bool any_bad = __ballot(bad) != 0;
    if (any_bad && lane == 0) atomicOr(&rec[SORT_REC_WORDS * a.nkeys], 1ULL);
}

// ---- encode -----------------------------------------------------------------------------------
struct SortEncodeArgs {
    const void *col[SORT_MAX_KEYS];
    uint64_t lo[SORT_MAX_KEYS], span[SORT_MAX_KEYS];
    int dtype[SORT_MAX_KEYS], shift[SORT_MAX_KEYS];
    int nkeys;       // keys of this round that have a width (0: only the rows are written)
    int bits;        // the round's width
    int descending;
    int first;       // src is the caller's row list (NULL: every row), read backwards when descending
};

template <typename T, typename W>
__device__ __forceinline__ void sort_pack(const T *col, const uint64_t (&row)[SE_RPT], uint32_t cnt, uint64_t lo, uint64_t span,
                                          int shift, W (&word)[SE_RPT]) {
    T v[SE_RPT];
#pragma unroll
    for (int r = 0; r < SE_RPT; r++) v[r] = (uint32_t)r < cnt ? col[row[r]] : T{};
#pragma unroll
    for (int r = 0; r < SE_RPT; r++) {
        uint64_t c = 0;
        const bool isnan = sort_code(v[r], c);
        const uint64_t rel = isnan ? span : c - lo;  // positions past cnt pack anything: they are not stored
        word[r] |= (W)(rel << shift);
    }
}

template <typename V> __device__ __forceinline__ void sort_store4(V *dst, uint64_t j, uint32_t cnt, const V (&val)[SE_RPT]) {
    if (cnt == SE_RPT && aligned_to(dst + j, 16)) {
        uint4 w[sizeof(V) / 4];
        __builtin_memcpy(w, val, sizeof(val));
#pragma unroll
        for (int k = 0; k < (int)sizeof(V) / 4; k++) reinterpret_cast<uint4 *>(dst + j)[k] = w[k];
    } else {
#pragma unroll
        for (int r = 0; r < SE_RPT; r++)
            if ((uint32_t)r < cnt) dst[j + r] = val[r];
    }
}

template <typename W, typename R>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_encode(SortEncodeArgs a, const R *src, uint64_t m, W *words, R *rows_out) {
    const W field = a.bits >= (int)(8 * sizeof(W)) ? (W)~(W)0 : (W)(((W)1 << a.bits) - 1);
    const bool backwards = a.first && a.descending;
    const uint64_t tile = (uint64_t)SORT_THREADS * SE_RPT;
    for (uint64_t t0 = blockIdx.x * tile; t0 < m; t0 += (uint64_t)gridDim.x * tile) {
        const uint64_t j = t0 + (uint64_t)threadIdx.x * SE_RPT;
        if (j >= m) continue;
        const uint32_t cnt = (uint32_t)min<uint64_t>(SE_RPT, m - j);
        uint64_t row[SE_RPT];
        if (!backwards && src && cnt == SE_RPT && aligned_to(src + j, 16)) {
            R raw[SE_RPT];
            uint4 w[sizeof(R) / 4];
#pragma unroll
            for (int k = 0; k < (int)sizeof(R) / 4; k++) w[k] = reinterpret_cast<const uint4 *>(src + j)[k];
            __builtin_memcpy(raw, w, sizeof(raw));
#pragma unroll
            for (int r = 0; r < SE_RPT; r++) row[r] = (uint64_t)raw[r];
        } else {
#pragma unroll
            for (int r = 0; r < SE_RPT; r++) {
                const uint64_t p = backwards ? m - 1 - (j + r) : j + r;  // used only while r < cnt: j + r < m
                row[r] = (uint32_t)r >= cnt ? 0 : src ? (uint64_t)src[p] : p;
            }
        }
        W word[SE_RPT] = {0, 0, 0, 0};
        for (int k = 0; k < a.nkeys; k++)
            SORT_DEVICE_DTYPE(a.dtype[k], T,
                              sort_pack<T, W>(static_cast<const T *>(a.col[k]), row, cnt, a.lo[k], a.span[k], a.shift[k], word));
        R rw[SE_RPT];
#pragma unroll
        for (int r = 0; r < SE_RPT; r++) {
            if (a.descending) word[r] = (W)(~word[r] & field);
            rw[r] = (R)row[r];
        }
        if (words) sort_store4<W>(words, j, cnt, word);
        sort_store4<R>(rows_out, j, cnt, rw);
    }
}

// ---- mask rows --------------------------------------------------------------------------------
// flag[i] = mask[i] != 0, eight rows per lane
__global__ __launch_bounds__(256) void k_mask_flags(const uint8_t *mask, uint64_t n, uint8_t *flag) {
    const bool al = aligned_rows8(mask, 1) && aligned_rows8(flag, 1);
    const uint64_t tile = 256ull * ROWS8;
    for (uint64_t t0 = blockIdx.x * tile; t0 < n; t0 += (uint64_t)gridDim.x * tile) {
        const uint64_t j = t0 + (uint64_t)threadIdx.x * ROWS8;
        if (j >= n) continue;
        const uint32_t cnt = (uint32_t)min<uint64_t>(ROWS8, n - j);
        uint8_t v[ROWS8];
        load_rows8<uint8_t>(mask, j, cnt, al, v);
#pragma unroll
        for (int u = 0; u < ROWS8; u++) v[u] = v[u] != 0;
        if (al && cnt == ROWS8) {
            uint2 w;
            __builtin_memcpy(&w, v, 8);
            *reinterpret_cast<uint2 *>(flag + j) = w;
        } else {
#pragma unroll
            for (int u = 0; u < ROWS8; u++)
                if ((uint32_t)u < cnt) flag[j + u] = v[u];
        }
    }
}

// pos[i] = kept rows before i (< the number of kept rows <= n: inside rows_out)
template <typename R>
__global__ __launch_bounds__(256) void k_mask_scatter(const uint8_t *flag, const uint64_t *pos, uint64_t n, R *rows_out) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        if (flag[i]) rows_out[pos[i]] = (R)i;
}

// ---- host -------------------------------------------------------------------------------------
template <typename W, typename R>
static void sort_digits(DevBuf &tmp, const void *words_in, void *words_out, const void *rows_in, void *rows_out, uint64_t m,
                        int bits) {
    hipStream_t st = stream();
    size_t tb = 0;
    VH_HIP(rocprim::radix_sort_pairs(nullptr, tb, static_cast<const W *>(words_in), static_cast<W *>(words_out),
                                     static_cast<const R *>(rows_in), static_cast<R *>(rows_out), (size_t)m, 0, bits, st));
    tmp.ensure(std::max<size_t>(tb, 16));
    tb = tmp.bytes;
    VH_HIP(rocprim::radix_sort_pairs(tmp.ptr, tb, static_cast<const W *>(words_in), static_cast<W *>(words_out),
                                     static_cast<const R *>(rows_in), static_cast<R *>(rows_out), (size_t)m, 0, bits, st));
}

template <typename R>
static void sort_run(int nkeys, const void *const *keys, const int *dtypes, uint64_t n, const R *rows, uint64_t m,
                     int descending, R *perm_out) {
    hipStream_t st = stream();
    // ranges
    SortKeys sk{};
    sk.nkeys = nkeys;
    std::vector<unsigned long long> rec(SORT_REC_WORDS * nkeys + 1, 0ULL);
    for (int k = 0; k < nkeys; k++) {
        sk.col[k] = keys[k];
        sk.dtype[k] = dtypes[k];
        rec[SORT_REC_WORDS * k] = ~0ULL;
    }
    DevBuf drec;
    drec.ensure(rec.size() * 8);
    VH_HIP(hipMemcpyAsync(drec.ptr, rec.data(), rec.size() * 8, hipMemcpyHostToDevice, st));
    {
        TimedScope ts("sort_range");
        hipLaunchKernelGGL(k_sort_range<R>, dim3(blocks_for((m + SE_RPT - 1) / SE_RPT, SORT_THREADS)), dim3(SORT_THREADS), 0, st,
                           sk, rows, n, m, drec.as<unsigned long long>());
        VH_HIP(hipGetLastError());
    }
    VH_HIP(hipMemcpyAsync(rec.data(), drec.ptr, rec.size() * 8, hipMemcpyDeviceToHost, st));
    VH_HIP(hipStreamSynchronize(st));
    if (rec[SORT_REC_WORDS * nkeys]) fail(VH_ERR_ARG, "argsort: rows holds a row number outside [0, n)");
    std::vector<SortRange> ranges(nkeys);
    for (int k = 0; k < nkeys; k++)
        ranges[k] = SortRange{rec[SORT_REC_WORDS * k], rec[SORT_REC_WORDS * k + 1], rec[SORT_REC_WORDS * k + 2] != 0};
    const SortPlan plan = sort_plan(ranges.data(), nkeys, m);

    std::vector<const SortRound *> run;
    bool any_wide = false;
    for (const SortRound &r : plan.rounds)
        if (r.bits > 0) {
            run.push_back(&r);
            any_wide |= r.wide;
        }
    const dim3 grd(blocks_for((m + SE_RPT - 1) / SE_RPT, SORT_THREADS)), blk(SORT_THREADS);
    if (run.empty()) {
        // every key is constant: the order is the row list itself (backwards when descending)
        SortEncodeArgs a{};
        a.descending = descending;
        a.first = 1;
        TimedScope ts("sort_encode");
        hipLaunchKernelGGL((k_sort_encode<uint32_t, R>), grd, blk, 0, st, a, rows, m, (uint32_t *)nullptr, perm_out);
        VH_HIP(hipGetLastError());
        VH_HIP(hipStreamSynchronize(st));
        return;
    }
    DevBuf words_a, words_b, rows_a, rows_b, tmp;
    words_a.ensure(m * (any_wide ? 8 : 4));
    words_b.ensure(m * (any_wide ? 8 : 4));
    rows_a.ensure(m * sizeof(R));
    if (run.size() > 1) rows_b.ensure(m * sizeof(R));
    const R *cur = rows;
    for (size_t e = 0; e < run.size(); e++) {
        const SortRound &r = *run[e];
        SortEncodeArgs a{};
        for (int k = r.key0; k < r.key1; k++) {
            if (!plan.keys[k].width) continue;
            const int s = a.nkeys++;
            a.col[s] = keys[k];
            a.dtype[s] = dtypes[k];
            a.lo[s] = plan.keys[k].lo;
            a.span[s] = plan.keys[k].span;
            a.shift[s] = r.shift[k - r.key0];
        }
        a.bits = r.bits;
        a.descending = descending;
        a.first = e == 0;
        {
            TimedScope ts("sort_encode");
            if (r.wide) hipLaunchKernelGGL((k_sort_encode<uint64_t, R>), grd, blk, 0, st, a, cur, m, words_a.as<uint64_t>(), rows_a.as<R>());
            else hipLaunchKernelGGL((k_sort_encode<uint32_t, R>), grd, blk, 0, st, a, cur, m, words_a.as<uint32_t>(), rows_a.as<R>());
            VH_HIP(hipGetLastError());
        }
        R *out = e + 1 == run.size() ? perm_out : rows_b.as<R>();
        {
            TimedScope ts("sort_digits");
            if (r.wide) sort_digits<uint64_t, R>(tmp, words_a.ptr, words_b.ptr, rows_a.ptr, out, m, r.bits);
            else sort_digits<uint32_t, R>(tmp, words_a.ptr, words_b.ptr, rows_a.ptr, out, m, r.bits);
        }
        cur = out;
    }
    VH_HIP(hipStreamSynchronize(st));
}

}  // namespace vh

using namespace vh;

extern "C" {

int vh_argsort(int nkeys, const void *const *keys, const int *dtypes, uint64_t n, const void *rows, int rows_itemsize,
               uint64_t m, int descending, void *perm_out) {
    VH_API_BEGIN
    if (nkeys < 1 || nkeys > SORT_MAX_KEYS) fail(VH_ERR_ARG, "argsort: 1 to " + std::to_string(SORT_MAX_KEYS) + " keys");
    if (rows_itemsize != 4 && rows_itemsize != 8) fail(VH_ERR_ARG, "argsort: rows_itemsize must be 4 or 8");
    if (rows_itemsize == 4 && n >= (uint64_t(1) << 31)) fail(VH_ERR_ARG, "argsort: 2^31 rows and more need 8-byte row numbers");
    if (n >= (uint64_t(1) << 62)) fail(VH_ERR_ARG, "argsort: row numbers past 2^62");
    if (!rows && m != n) fail(VH_ERR_ARG, "argsort: without rows, m must equal n");
    if (m > n) fail(VH_ERR_ARG, "argsort: more rows than the columns hold");
    for (int k = 0; k < nkeys; k++) dtype_itemsize(dtypes[k]);
    if (!m) return VH_OK;
    for (int k = 0; k < nkeys; k++)
        if (!keys[k] || resolve_loc(keys[k], VH_LOC_AUTO) != VH_LOC_DEVICE) fail(VH_ERR_ARG, "argsort: device buffers only");
    if (!perm_out || resolve_loc(perm_out, VH_LOC_AUTO) != VH_LOC_DEVICE || (rows && resolve_loc(rows, VH_LOC_AUTO) != VH_LOC_DEVICE))
        fail(VH_ERR_ARG, "argsort: device buffers only");
    if (rows_itemsize == 4)
        sort_run<int32_t>(nkeys, keys, dtypes, n, static_cast<const int32_t *>(rows), m, descending != 0, static_cast<int32_t *>(perm_out));
    else
        sort_run<int64_t>(nkeys, keys, dtypes, n, static_cast<const int64_t *>(rows), m, descending != 0, static_cast<int64_t *>(perm_out));
    VH_API_END
}

int vh_mask_rows(const uint8_t *mask, uint64_t n, int out_itemsize, void *rows_out, uint64_t *m) {
    VH_API_BEGIN
    if (out_itemsize != 4 && out_itemsize != 8) fail(VH_ERR_ARG, "mask_rows: out_itemsize must be 4 or 8");
    if (out_itemsize == 4 && n >= (uint64_t(1) << 31)) fail(VH_ERR_ARG, "mask_rows: 2^31 rows and more need 8-byte row numbers");
    if (m) *m = 0;
    if (!n) return VH_OK;
    if (!mask || !rows_out || resolve_loc(mask, VH_LOC_AUTO) != VH_LOC_DEVICE || resolve_loc(rows_out, VH_LOC_AUTO) != VH_LOC_DEVICE)
        fail(VH_ERR_ARG, "mask_rows: device buffers only");
    hipStream_t st = stream();
    TimedScope ts("mask_rows");
    DevBuf flag, pos, tmp;
    flag.ensure(n + 1);  // byte flags, 64-bit offsets: 9 bytes of temporary per row (as vh_index_matched)
    pos.ensure((n + 1) * 8);
    VH_HIP(hipMemsetAsync(flag.as<uint8_t>() + n, 0, 1, st));
    hipLaunchKernelGGL(k_mask_flags, dim3(blocks_for((n + ROWS8 - 1) / ROWS8, 256)), dim3(256), 0, st, mask, n, flag.as<uint8_t>());
    VH_HIP(hipGetLastError());
    size_t tb = 0;
    VH_HIP(rocprim::exclusive_scan(nullptr, tb, flag.as<uint8_t>(), pos.as<uint64_t>(), (uint64_t)0, (size_t)(n + 1),
                                   rocprim::plus<uint64_t>(), st));
    tmp.ensure(std::max<size_t>(tb, 16));
    tb = tmp.bytes;
    VH_HIP(rocprim::exclusive_scan(tmp.ptr, tb, flag.as<uint8_t>(), pos.as<uint64_t>(), (uint64_t)0, (size_t)(n + 1),
                                   rocprim::plus<uint64_t>(), st));
    const dim3 grd(blocks_for(n, 256)), blk(256);
    if (out_itemsize == 4)
        hipLaunchKernelGGL(k_mask_scatter<int32_t>, grd, blk, 0, st, flag.as<uint8_t>(), pos.as<uint64_t>(), n, static_cast<int32_t *>(rows_out));
    else
        hipLaunchKernelGGL(k_mask_scatter<int64_t>, grd, blk, 0, st, flag.as<uint8_t>(), pos.as<uint64_t>(), n, static_cast<int64_t *>(rows_out));
    VH_HIP(hipGetLastError());
    uint64_t total = 0;
    VH_HIP(hipMemcpyAsync(&total, pos.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    VH_HIP(hipStreamSynchronize(st));
    if (m) *m = total;
    VH_API_END
}

}  // extern "C"
