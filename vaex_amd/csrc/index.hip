// index_hash_<dtype> on the GPU: key -> the first row it was seen at, plus the remaining rows
// of duplicated keys (packages/vaex-core/src/hash_primitives.hpp:623-900), the hash map behind
// DataFrame.join (join.py:124-292); and the device gather (vh_take) and the inner join's
// stream compaction (vh_index_matched) that a join needs next to it.
//
// Table: the ordered set's open-address table in HBM (hashset.hpp): 16-byte slots {key bits
// zero-extended (EMPTY = ~0), first row}, linear probing from hash64(bits).  The 8-byte key
// whose bits equal EMPTY lives in a side slot ("special").  Key identity is the other hash
// engines': every NaN is the one NaN entry, rows whose mask byte is set are the null entry,
// every other key compares by bit pattern (-0.0 and 0.0 are two keys).
//
// update: one set_claim (a CAS on the key word) and one atomicMin of the row per regular row,
//   straight on the HBM table -- the indexed side of a join is the small side, so there is no
//   hash-partitioned build here.  A probe sequence past SET_MAX_PROBE raises the overflow flag;
//   the host grows the table x4, rehashes it and runs the chunk again (atomicMin is idempotent,
//   so there is no scratch table; the chunk's row counts are zeroed before every attempt, the
//   count of distinct keys is cumulative because a failed attempt's keys stay in the table).
//   nan_value / null_value are the largest NaN / null row over all updates (the rule is stated
//   in vaexhip.h: row numbers decide for every entry, not the order of the calls).  The handle keeps a device
//   copy of each chunk's keys, and a flag byte per row (0 regular or NaN, 1 null, 2 not
//   selected) when a mask or a select was given: the duplicates finish and merge need them.
//   has_duplicates = regular rows seen > distinct regular keys, both counted by the kernel.
//
// seal (implicit on the first probe): the probe LUT in the set's SetDev layout -- 8-byte slots
//   (row << 32 | key bits) for keys of <= 4 bytes while every row number is below 2^31, else
//   the {bits, row} table itself.  With duplicates also a CSR of the extra rows: every retained
//   regular row r with slot s and first[s] != r gets the sort key s (every other row a
//   sentinel past the last slot), one stable radix sort by s brings the extras to the front
//   grouped by slot with rows in input order, and dup_begin[s] / dup_count[s] index them.
//   The special key's slot number is `cap`.  The retained chunks are freed at seal.
//
// map_index (the hot kernel): each lane takes IX_RPT consecutive rows with wide loads and
//   issues the home-slot reads of all of them before it uses any; stragglers continue with
//   linear probing (<= SET_MAX_PROBE); a lane's IX_RPT results leave in wide stores; the unknown
//   flag takes one atomic per workgroup.  A LUT of <= IX_LDS_BYTES (64 KiB: 4096 keys of <= 4
//   bytes, 2048 of 8 bytes, at half load) is staged in LDS once per workgroup and probed there
//   (0.33 ms against 0.56 ms per 1e8 int32 rows at 1e2 keys).  A packed LUT read
//   from HBM takes the one-row-per-lane form of the same kernel instead (ix_launch_map).
//
// map_index_duplicates: count per left row (dup_count of its key's slot), an exclusive scan,
//   then one thread per output pair finds its left row by binary search in the offsets:
//   pairs in left-row order, extras ascending within a key, the same on every run.  The pairs
//   stay on the device in the handle; a second call with output pointers copies them out.
#include <algorithm>
#include <memory>
#include <mutex>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.hpp"
#include "hashset.hpp"
#include "lds_table.hpp"
#include "slot_table.hpp"

using namespace vh;

enum { X_OVERFLOW = 0, X_DISTINCT, X_ROWS, X_NAN_CNT, X_NULL_CNT, X_SPEC_CNT, X_NAN_LAST, X_NULL_LAST, X_SPEC_FIRST, X_N };

struct IxChunk {
    DevBuf keys, flags;
    uint64_t n = 0, row0 = 0;
    bool has_flags = false;
};

struct vh_index {
    std::recursive_mutex mu;
    int dtype = VH_I64;
    bool explicit_cap = false;
    uint64_t cap = 0;
    DevBuf tab, lut, ctr;
    std::vector<std::unique_ptr<IxChunk>> chunks;
    uint64_t distinct = 0;      // regular keys in the table (the device counter's value)
    uint64_t regular_rows = 0;  // regular rows seen, the special key's included
    uint64_t special_rows = 0;
    int64_t special_first = -1;
    int64_t nan_count = 0, null_count = 0, nan_value = -1, null_value = -1;
    uint64_t max_row = 0;  // one past the largest row number seen
    bool sealed = false, packed = false;
    DevBuf dup_begin, dup_count, dup_rows;  // u32[cap + 1], u32[cap + 1], i64[extras]
    uint64_t extras = 0;
    // the pairs of the last map_index_duplicates count call
    DevBuf pair_left, pair_right;
    uint64_t pairs = 0;
    bool pairs_ready = false;

    uint64_t distinct_all() const { return distinct + (special_rows ? 1 : 0); }
    bool has_duplicates() const { return regular_rows > distinct_all(); }
};

namespace vh {

constexpr int IX_RPT = 8;  // consecutive rows per lane and step (map_index, update reads one): one load_rows8 group
static_assert(IX_RPT == ROWS8, "load_rows8 / store_rows8 take 8 rows");
constexpr int IX_THREADS = 256;
constexpr uint64_t IX_LDS_BYTES = uint64_t(1) << 16;  // the LDS image of a LUT: 8192 packed or 4096 16-byte slots
constexpr uint64_t IX_MIN_HBM_CAP = uint64_t(1) << 16;
constexpr uint64_t IX_DEFAULT_CAP = 256;  // the first table; every update sizes it for its rows
constexpr uint64_t IX_MAX_PRESIZE = uint64_t(1) << 28;

struct IxParams {
    const void *keys;
    const uint8_t *mask, *select, *flags_in;
    uint8_t *flags_out;
    uint64_t n, row0;
    uint64_t *tab;
    uint64_t cap_mask;
    uint32_t max_probe;
    uint64_t *ctr;
};

// ---- update ---------------------------------------------------------------------------------
template <typename T> __global__ __launch_bounds__(IX_THREADS) void k_ix_update(IxParams p) {
    __shared__ uint32_t s_new, s_rows, s_nan, s_null, s_spec;
    __shared__ unsigned long long s_nan_last, s_null_last, s_spec_first;
    if (threadIdx.x == 0) {
        s_new = s_rows = s_nan = s_null = s_spec = 0;
        s_nan_last = s_null_last = 0;
        s_spec_first = ~0ULL;
    }
    __syncthreads();
    const T *keys = static_cast<const T *>(p.keys);
    uint32_t rows = 0, nans = 0, nulls = 0, specs = 0;
    unsigned long long nan_last = 0, null_last = 0, spec_first = ~0ULL;  // last: row + 1, 0 = none
    for (uint64_t i = blockIdx.x * (uint64_t)IX_THREADS + threadIdx.x; i < p.n; i += (uint64_t)gridDim.x * IX_THREADS) {
        uint8_t f;
        if (p.flags_in) f = p.flags_in[i];
        else f = (p.select && !p.select[i]) ? 2 : (p.mask && p.mask[i]) ? 1 : 0;
        if (p.flags_out) p.flags_out[i] = f;
        if (f == 2) continue;  // filtered out / not selected: not seen at all
        const uint64_t row = p.row0 + i;
        if (f == 1) {
            nulls++;
            null_last = max(null_last, (unsigned long long)row + 1);
            continue;
        }
        const T v = keys[i];
        if (is_nan_v(v)) {
            nans++;
            nan_last = max(nan_last, (unsigned long long)row + 1);
            continue;
        }
        const uint64_t kb = key_bits(v);
        rows++;
        if (kb == SET_EMPTY) {  // 8-byte keys only: the side slot
            specs++;
            spec_first = min(spec_first, (unsigned long long)row);
            continue;
        }
        set_claim(p.tab, p.cap_mask, p.max_probe, kb, &s_new, &p.ctr[X_OVERFLOW], [&](uint64_t *first) {
            if (__hip_atomic_load(first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > row)
                atomicMin((unsigned long long *)first, (unsigned long long)row);
        });
    }
    if (rows) atomicAdd(&s_rows, rows);
    if (nans) {
        atomicAdd(&s_nan, nans);
        atomicMax(&s_nan_last, nan_last);
    }
    if (nulls) {
        atomicAdd(&s_null, nulls);
        atomicMax(&s_null_last, null_last);
    }
    if (specs) {
        atomicAdd(&s_spec, specs);
        atomicMin(&s_spec_first, spec_first);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long *c = reinterpret_cast<unsigned long long *>(p.ctr);
        if (s_new) atomicAdd(&c[X_DISTINCT], (unsigned long long)s_new);
        if (s_rows) atomicAdd(&c[X_ROWS], (unsigned long long)s_rows);
        if (s_nan) {
            atomicAdd(&c[X_NAN_CNT], (unsigned long long)s_nan);
            atomicMax(&c[X_NAN_LAST], s_nan_last);
        }
        if (s_null) {
            atomicAdd(&c[X_NULL_CNT], (unsigned long long)s_null);
            atomicMax(&c[X_NULL_LAST], s_null_last);
        }
        if (s_spec) {
            atomicAdd(&c[X_SPEC_CNT], (unsigned long long)s_spec);
            atomicMin(&c[X_SPEC_FIRST], s_spec_first);
        }
    }
}

// ---- seal -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ix_pack_lut(const uint64_t *tab, uint64_t cap, uint64_t *lut) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * 256) {
        const ulonglong2 e = reinterpret_cast<const ulonglong2 *>(tab)[i];
        lut[i] = e.x == SET_EMPTY ? SET_EMPTY : (e.y << 32) | (e.x & 0xffffffffULL);
    }
}

// slot of a key in the {bits, row} table, `cap` for the special key, -1 when absent
__device__ inline int64_t ix_find_slot(const uint64_t *tab, uint64_t cap_mask, uint32_t max_probe, uint64_t kb) {
    if (kb == SET_EMPTY) return (int64_t)(cap_mask + 1);
    uint64_t pos = hash64(kb) & cap_mask;
    for (uint32_t p = 0; p <= max_probe; p++) {
        const uint64_t k = tab[2 * pos];
        if (k == kb) return (int64_t)pos;
        if (k == SET_EMPTY) return -1;
        pos = (pos + 1) & cap_mask;
    }
    return -1;
}

// sort key of every retained row: its slot when it is an extra row of its key, else `sentinel`
template <typename T>
__global__ __launch_bounds__(256) void k_ix_dup_keys(const T *keys, const uint8_t *flags, uint64_t n, uint64_t row0,
                                                     const uint64_t *tab, uint64_t cap_mask, uint32_t max_probe,
                                                     int64_t special_first, uint32_t sentinel, uint32_t *skey,
                                                     int64_t *srow) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        uint32_t sk = sentinel;
        const int64_t row = (int64_t)(row0 + i);
        const T v = keys[i];
        if (!(flags && flags[i]) && !is_nan_v(v)) {
            const uint64_t kb = key_bits(v);
            const int64_t s = ix_find_slot(tab, cap_mask, max_probe, kb);
            if (s >= 0) {
                const int64_t first = kb == SET_EMPTY ? special_first : (int64_t)tab[2 * s + 1];
                if (first != row) sk = (uint32_t)s;
            }
        }
        skey[i] = sk;
        srow[i] = row;
    }
}

__global__ __launch_bounds__(256) void k_ix_dup_csr(const uint32_t *skey, uint64_t extras, uint32_t sentinel,
                                                    uint32_t *dup_begin, uint32_t *dup_count) {
    for (uint64_t j = blockIdx.x * 256ull + threadIdx.x; j < extras; j += (uint64_t)gridDim.x * 256) {
        const uint32_t s = skey[j];
        if (s >= sentinel) continue;  // never, unless the rows were miscounted (the host checks and fails)
        atomicAdd(&dup_count[s], 1u);
        if (j == 0 || skey[j - 1] != s) dup_begin[s] = (uint32_t)j;
    }
}

// ---- map_index ------------------------------------------------------------------------------
// LDS: a LUT of <= IX_LDS_BYTES is staged in LDS once per workgroup (the grid is a few
// workgroups per CU, each striding over many tiles) and probed there.
// CONSEC: a lane takes R = 8 consecutive rows with wide loads and stores; else row
// r * IX_THREADS + lane of the tile (every load / store instruction covers whole lines).
template <typename T, typename O, bool WIDE, bool LDS, int R, bool CONSEC>
__global__ __launch_bounds__(IX_THREADS) void k_ix_map(const T *keys, const uint8_t *mask, uint64_t n, SetDev s, O *out,
                                                      uint32_t *unknown) {
    static_assert(!CONSEC || R == IX_RPT, "the wide loads take 8 rows");
    using E = std::conditional_t<WIDE, ulonglong2, uint64_t>;
    const E *lut = reinterpret_cast<const E *>(s.lut);
    extern __shared__ __align__(16) unsigned char ix_lds_raw[];
    E *ix_lds = reinterpret_cast<E *>(ix_lds_raw);
    if constexpr (LDS) {
        for (uint64_t i = threadIdx.x; i <= s.cap_mask; i += IX_THREADS) ix_lds[i] = lut[i];
        __syncthreads();
    }
    auto load_slot = [&](uint64_t ps, uint64_t &x, uint64_t &y) {
        if constexpr (WIDE) {
            const ulonglong2 t = LDS ? ix_lds[ps] : lut[ps];  // one 16-byte load
            x = t.x;
            y = t.y;
        } else {
            x = LDS ? ix_lds[ps] : lut[ps];
            y = 0;
        }
    };
    // CONSEC: every lane's rows start at a multiple of 8: the base addresses decide the alignment
    const bool al = aligned_rows8(keys, sizeof(T)) && (!mask || aligned_rows8(mask, 1)) && aligned_rows8(out, sizeof(O));
    bool unk = false;
    const uint64_t tile = (uint64_t)IX_THREADS * R;
    for (uint64_t t0 = blockIdx.x * tile; t0 < n; t0 += (uint64_t)gridDim.x * tile) {
        T v[R];
        uint8_t m[R];
        bool ok[R];
        uint64_t j = 0;
        uint32_t cnt = 0;
        if constexpr (CONSEC) {
            j = t0 + (uint64_t)threadIdx.x * R;
            if (j >= n) continue;
            cnt = (uint32_t)min<uint64_t>(R, n - j);
            load_rows8<T>(keys, j, cnt, al, v);
            if (mask) load_rows8<uint8_t>(mask, j, cnt, al, m);
#pragma unroll
            for (int r = 0; r < R; r++) ok[r] = (uint32_t)r < cnt;
        } else {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const uint64_t i = t0 + (uint64_t)r * IX_THREADS + threadIdx.x;
                ok[r] = i < n;
                v[r] = ok[r] ? keys[i] : T{};
                m[r] = (mask && ok[r]) ? mask[i] : 0;
            }
        }
        uint64_t kb[R], pos[R];
        uint64_t ex[R], ey[R];  // the slot's words (packed: ex only); scalars, not a vector-type array
        // the home slots of all R rows are read before any is used (rows past the end read
        // the slot of a zero key: inside the table)
#pragma unroll
        for (int r = 0; r < R; r++) {
            kb[r] = key_bits(v[r]);
            pos[r] = hash64(kb[r]) & s.cap_mask;
            load_slot(pos[r], ex[r], ey[r]);
        }
        O o[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            int64_t res = -1;
            if (is_nan_v(v[r])) {
                res = s.nan_ord;
            } else if (mask && m[r]) {
                res = s.null_ord;
            } else if (kb[r] == SET_EMPTY) {
                res = s.special_ord;
            } else {
                uint64_t x = ex[r], y = ey[r], ps = pos[r];
                for (int pr = 0; pr <= SET_MAX_PROBE; pr++) {
                    if constexpr (WIDE) {
                        if (x == kb[r]) {
                            res = (int64_t)y;
                            break;
                        }
                        if (x == SET_EMPTY) break;
                    } else {
                        if (x == SET_EMPTY) break;
                        if ((uint32_t)x == (uint32_t)kb[r]) {
                            res = (int64_t)(x >> 32);
                            break;
                        }
                    }
                    ps = (ps + 1) & s.cap_mask;
                    load_slot(ps, x, y);
                }
            }
            unk |= ok[r] && res < 0;
            o[r] = (O)res;
        }
        if constexpr (CONSEC) {
            if constexpr (R == IX_RPT) store_rows8<O>(out, j, cnt, al, o);
        } else {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (ok[r]) out[t0 + (uint64_t)r * IX_THREADS + threadIdx.x] = o[r];
        }
    }
    if (__syncthreads_or(unk) && threadIdx.x == 0) atomicOr(unknown, 1u);
}

// ---- map_index_duplicates -------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_ix_dup_count(const T *keys, const uint8_t *mask, uint64_t n, const uint64_t *tab,
                                                      uint64_t cap_mask, uint32_t max_probe, const uint32_t *dup_begin,
                                                      const uint32_t *dup_count, uint32_t *cnt, uint32_t *beg) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        uint32_t c = 0, b = 0;
        const T v = keys[i];
        if (!is_nan_v(v) && !(mask && mask[i])) {  // NaN and masked keys are skipped (:769-771)
            const int64_t s = ix_find_slot(tab, cap_mask, max_probe, key_bits(v));
            if (s >= 0) {
                c = dup_count[s];
                b = dup_begin[s];
            }
        }
        cnt[i] = c;
        beg[i] = b;
    }
}

// pair j belongs to the last left row whose offset is <= j (rows without extras share their
// offset with the next row, so they are never the last)
__global__ __launch_bounds__(256) void k_ix_dup_fill(const uint64_t *off, const uint32_t *beg, uint64_t n, uint64_t total,
                                                     uint64_t start_index, const int64_t *dup_rows, int64_t *left,
                                                     int64_t *right) {
    for (uint64_t j = blockIdx.x * 256ull + threadIdx.x; j < total; j += (uint64_t)gridDim.x * 256) {
        uint64_t lo = 0, hi = n;  // off[lo] <= j < off[hi] (off[n] = total)
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (off[mid] <= j) lo = mid;
            else hi = mid;
        }
        left[j] = (int64_t)(start_index + lo);
        right[j] = dup_rows[beg[lo] + (j - off[lo])];
    }
}

// ---- take -----------------------------------------------------------------------------------
constexpr int TK_COLS = 8;  // columns per launch: idx is read once for all of them
constexpr int TK_RPT = 4;   // consecutive rows per lane and step
struct TakeArgs {
    void *dst[TK_COLS];
    const void *src[TK_COLS];
    int isz[TK_COLS];
    int ncols;
};

template <typename V>
__device__ __forceinline__ void tk_column(V *dst, const V *src, uint64_t j, uint32_t cnt, const int64_t (&ix)[TK_RPT]) {
    V val[TK_RPT];
#pragma unroll
    for (int r = 0; r < TK_RPT; r++) val[r] = ((uint32_t)r < cnt && ix[r] >= 0) ? src[ix[r]] : V(0);
    if (cnt == TK_RPT && aligned_to(dst, TK_RPT * sizeof(V))) {
        using W = std::conditional_t<sizeof(V) == 8, uint4, std::conditional_t<sizeof(V) == 4, uint4,
                  std::conditional_t<sizeof(V) == 2, uint2, uint32_t>>>;
        constexpr int NW = TK_RPT * sizeof(V) / sizeof(W);
        W w[NW];
        __builtin_memcpy(w, val, sizeof(val));
#pragma unroll
        for (int k = 0; k < NW; k++) reinterpret_cast<W *>(dst + j)[k] = w[k];
    } else {
#pragma unroll
        for (int r = 0; r < TK_RPT; r++)
            if ((uint32_t)r < cnt) dst[j + r] = val[r];
    }
}

template <typename I>
__global__ __launch_bounds__(256) void k_take(TakeArgs a, const I *idx, uint64_t n, uint8_t *mask_out) {
    const bool al = aligned_to(idx, TK_RPT * sizeof(I));
    const uint64_t tile = 256ull * TK_RPT;
    for (uint64_t t0 = blockIdx.x * tile; t0 < n; t0 += (uint64_t)gridDim.x * tile) {
        const uint64_t j = t0 + (uint64_t)threadIdx.x * TK_RPT;
        if (j >= n) continue;
        const uint32_t cnt = (uint32_t)min<uint64_t>(TK_RPT, n - j);
        I raw[TK_RPT];
        if (al && cnt == TK_RPT) {
            uint4 w[sizeof(I) / 4];
#pragma unroll
            for (int k = 0; k < (int)sizeof(I) / 4; k++) w[k] = reinterpret_cast<const uint4 *>(idx + j)[k];
            __builtin_memcpy(raw, w, sizeof(raw));
        } else {
#pragma unroll
            for (int r = 0; r < TK_RPT; r++) raw[r] = (uint32_t)r < cnt ? idx[j + r] : (I)-1;
        }
        int64_t ix[TK_RPT];
#pragma unroll
        for (int r = 0; r < TK_RPT; r++) ix[r] = (int64_t)raw[r];
        if (mask_out) {
#pragma unroll
            for (int r = 0; r < TK_RPT; r++)
                if ((uint32_t)r < cnt) mask_out[j + r] = ix[r] < 0;
        }
#pragma unroll
        for (int c = 0; c < TK_COLS; c++) {
            if (c >= a.ncols) break;
            switch (a.isz[c]) {
            case 8: tk_column<uint64_t>((uint64_t *)a.dst[c], (const uint64_t *)a.src[c], j, cnt, ix); break;
            case 4: tk_column<uint32_t>((uint32_t *)a.dst[c], (const uint32_t *)a.src[c], j, cnt, ix); break;
            case 2: tk_column<uint16_t>((uint16_t *)a.dst[c], (const uint16_t *)a.src[c], j, cnt, ix); break;
            default: tk_column<uint8_t>((uint8_t *)a.dst[c], (const uint8_t *)a.src[c], j, cnt, ix);
            }
        }
    }
}

// ---- matched (inner join) ---------------------------------------------------------------------
template <typename I> __global__ __launch_bounds__(256) void k_matched_flags(const I *idx, uint64_t n, uint8_t *flag) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) flag[i] = idx[i] >= 0;
}
template <typename I>
__global__ __launch_bounds__(256) void k_matched_scatter(const I *idx, const uint64_t *pos, uint64_t n, int64_t *left_rows,
                                                         I *idx_out) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const I v = idx[i];
        if (v < 0) continue;
        left_rows[pos[i]] = (int64_t)i;
        idx_out[pos[i]] = v;
    }
}

// ---- host -----------------------------------------------------------------------------------
// one device-resident chunk into the table; `flags_in` (a retained chunk of another index)
// replaces mask / select
static void ix_chunk(vh_index *x, const void *keys, const uint8_t *mask, const uint8_t *select, const uint8_t *flags_in,
                     uint8_t *flags_out, uint64_t n, uint64_t row0) {
    hipStream_t st = stream();
    // a join index holds mostly distinct keys: room for every row at <= 1/2 load, unless the
    // caller chose the first table's size
    if (!x->explicit_cap) {
        uint64_t want = std::min<uint64_t>(next_pow2(2 * (x->distinct + n)), IX_MAX_PRESIZE);
        // a table too large for the probe's LDS image gets at least the ordered set's 2^16 slots:
        // 1e8 probes into a few hundred hot lines queue up (both routes took 1.0 ms at 4096 keys
        // in 8192 slots against 0.87 ms at 1e5 keys)
        if (want * (dtype_itemsize(x->dtype) > 4 ? 16 : 8) > IX_LDS_BYTES) want = std::max<uint64_t>(want, IX_MIN_HBM_CAP);
        if (want > x->cap) slots_grow(x->tab, x->cap, want);
    }
    std::vector<uint64_t> c;
    for (int attempt = 0;; attempt++) {
        uint64_t init[X_N] = {0};
        init[X_DISTINCT] = x->distinct;
        init[X_SPEC_FIRST] = ~0ULL;
        VH_HIP(hipMemcpyAsync(x->ctr.ptr, init, sizeof(init), hipMemcpyHostToDevice, st));
        IxParams p{keys, mask, select, flags_in, flags_out, n, row0, x->tab.as<uint64_t>(), x->cap - 1, slots_max_probe(x->cap),
                   x->ctr.as<uint64_t>()};
        {
            TimedScope ts("index_update");
            VH_DISPATCH_DTYPE(x->dtype, T,
                              hipLaunchKernelGGL(k_ix_update<T>, dim3(blocks_for(n, IX_THREADS)), dim3(IX_THREADS), 0, st, p));
            VH_HIP(hipGetLastError());
        }
        c = slots_read_ctr(x->ctr, X_N);
        x->distinct = c[X_DISTINCT];  // a failed attempt's keys stay in the table
        if (!c[X_OVERFLOW]) break;
        if (attempt > 24) fail(VH_ERR_RUNTIME, "index_hash could not grow enough");
        slots_grow(x->tab, x->cap, x->cap * 4);
    }
    if (x->distinct * 2 > x->cap) slots_grow(x->tab, x->cap, next_pow2(x->distinct * 2));
    x->regular_rows += c[X_ROWS];
    x->special_rows += c[X_SPEC_CNT];
    if (c[X_SPEC_CNT]) x->special_first = x->special_first < 0 ? (int64_t)c[X_SPEC_FIRST]
                                                              : std::min<int64_t>(x->special_first, (int64_t)c[X_SPEC_FIRST]);
    x->nan_count += (int64_t)c[X_NAN_CNT];
    x->null_count += (int64_t)c[X_NULL_CNT];
    if (c[X_NAN_CNT]) x->nan_value = std::max<int64_t>(x->nan_value, (int64_t)c[X_NAN_LAST] - 1);
    if (c[X_NULL_CNT]) x->null_value = std::max<int64_t>(x->null_value, (int64_t)c[X_NULL_LAST] - 1);
    x->max_row = std::max(x->max_row, row0 + n);
}

static void ix_update(vh_index *x, const void *keys, const uint8_t *mask, const uint8_t *select, uint64_t n,
                      uint64_t start_index, int loc) {
    if (x->sealed) fail(VH_ERR_RUNTIME, "index_hash is sealed (it was probed), cannot update");
    if (!n) return;
    if (start_index + n > (uint64_t(1) << 62)) fail(VH_ERR_ARG, "index_hash: row numbers past 2^62");
    loc = resolve_loc(keys, loc);
    const int isz = dtype_itemsize(x->dtype);
    const uint64_t CH = loc == VH_LOC_HOST ? (uint64_t(1) << 24) : n;
    hipStream_t st = stream();
    const hipMemcpyKind kind = loc == VH_LOC_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    HostStage stage;
    for (uint64_t r0 = 0; r0 < n; r0 += CH) {
        const uint64_t len = std::min(CH, n - r0);
        std::unique_ptr<IxChunk> ch(new IxChunk());
        ch->n = len;
        ch->row0 = start_index + r0;
        ch->has_flags = mask || select;
        ch->keys.ensure(len * isz);
        VH_HIP(hipMemcpyAsync(ch->keys.ptr, reinterpret_cast<const char *>(keys) + r0 * isz, len * isz, kind, st));
        if (ch->has_flags) ch->flags.ensure(len);
        const uint8_t *dm = mask ? mask + r0 : nullptr, *ds = select ? select + r0 : nullptr;
        // mask / select are staged when they are host arrays, wherever the keys are
        if (mask && (loc == VH_LOC_HOST || resolve_loc(mask, VH_LOC_AUTO) == VH_LOC_HOST))
            dm = static_cast<const uint8_t *>(HostStage::copy(stage.mask, dm, len));
        if (select && (loc == VH_LOC_HOST || resolve_loc(select, VH_LOC_AUTO) == VH_LOC_HOST))
            ds = static_cast<const uint8_t *>(HostStage::copy(stage.select, ds, len));
        ix_chunk(x, ch->keys.ptr, dm, ds, nullptr, ch->has_flags ? ch->flags.as<uint8_t>() : nullptr, len, ch->row0);
        x->chunks.push_back(std::move(ch));
    }
}

static void ix_seal(vh_index *x) {
    if (x->sealed) return;
    hipStream_t st = stream();
    const int isz = dtype_itemsize(x->dtype);
    x->packed = isz <= 4 && x->max_row < (uint64_t(1) << 31);
    if (x->packed) {
        x->lut.ensure(x->cap * 8);
        hipLaunchKernelGGL(k_ix_pack_lut, dim3(blocks_for(x->cap, 256)), dim3(256), 0, st, x->tab.as<uint64_t>(), x->cap,
                           x->lut.as<uint64_t>());
        VH_HIP(hipGetLastError());
    }
    if (x->has_duplicates()) {
        TimedScope ts("index_seal_duplicates");
        uint64_t R = 0;
        for (auto &ch : x->chunks) R += ch->n;
        const uint64_t E = x->regular_rows - x->distinct_all();
        if (E >= (uint64_t(1) << 32) || x->cap + 1 >= (uint64_t(1) << 32))
            fail(VH_ERR_RUNTIME, "index_hash: more than 2^32 duplicate rows");
        const uint32_t sentinel = (uint32_t)(x->cap + 1);
        DevBuf skey, srow, skey2, srow2, tmp;
        skey.ensure(R * 4);
        srow.ensure(R * 8);
        skey2.ensure(R * 4);
        srow2.ensure(R * 8);
        uint64_t off = 0;
        for (auto &ch : x->chunks) {
            VH_DISPATCH_DTYPE(x->dtype, T,
                              hipLaunchKernelGGL(k_ix_dup_keys<T>, dim3(blocks_for(ch->n, 256)), dim3(256), 0, st,
                                                 ch->keys.as<T>(), ch->has_flags ? ch->flags.as<uint8_t>() : nullptr, ch->n,
                                                 ch->row0, x->tab.as<uint64_t>(), x->cap - 1, slots_max_probe(x->cap),
                                                 x->special_first, sentinel, skey.as<uint32_t>() + off,
                                                 srow.as<int64_t>() + off));
            VH_HIP(hipGetLastError());
            off += ch->n;
        }
        int bits = 1;
        while ((uint64_t(1) << bits) <= sentinel) bits++;
        size_t tb = 0;
        VH_HIP(rocprim::radix_sort_pairs(nullptr, tb, skey.as<uint32_t>(), skey2.as<uint32_t>(), srow.as<int64_t>(),
                                         srow2.as<int64_t>(), (size_t)R, 0, bits, st));
        tmp.ensure(std::max<size_t>(tb, 16));
        tb = tmp.bytes;
        VH_HIP(rocprim::radix_sort_pairs(tmp.ptr, tb, skey.as<uint32_t>(), skey2.as<uint32_t>(), srow.as<int64_t>(),
                                         srow2.as<int64_t>(), (size_t)R, 0, bits, st));
        x->dup_begin.ensure((x->cap + 1) * 4);
        x->dup_count.ensure((x->cap + 1) * 4);
        x->dup_rows.ensure(E * 8);
        VH_HIP(hipMemsetAsync(x->dup_begin.ptr, 0, (x->cap + 1) * 4, st));
        VH_HIP(hipMemsetAsync(x->dup_count.ptr, 0, (x->cap + 1) * 4, st));
        VH_HIP(hipMemcpyAsync(x->dup_rows.ptr, srow2.ptr, E * 8, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_ix_dup_csr, dim3(blocks_for(E, 256)), dim3(256), 0, st, skey2.as<uint32_t>(), E, sentinel,
                           x->dup_begin.as<uint32_t>(), x->dup_count.as<uint32_t>());
        VH_HIP(hipGetLastError());
        // the sort put exactly E rows in front of the sentinel rows
        uint32_t edge[2] = {0, sentinel};
        VH_HIP(hipMemcpyAsync(&edge[0], skey2.as<uint32_t>() + E - 1, 4, hipMemcpyDeviceToHost, st));
        if (E < R) VH_HIP(hipMemcpyAsync(&edge[1], skey2.as<uint32_t>() + E, 4, hipMemcpyDeviceToHost, st));
        VH_HIP(hipStreamSynchronize(st));
        if (edge[0] == sentinel || edge[1] != sentinel) fail(VH_ERR_RUNTIME, "index_hash: duplicate rows miscounted (internal error)");
        x->extras = E;
    }
    VH_HIP(hipStreamSynchronize(st));
    x->chunks.clear();  // the retained key copies are not needed past this point
    x->sealed = true;
}

static SetDev ix_view(vh_index *x) {
    SetDev d{};
    d.lut = x->packed ? x->lut.as<uint64_t>() : x->tab.as<uint64_t>();
    d.wide = !x->packed;
    d.cap_mask = x->cap - 1;
    d.nan_ord = x->nan_count > 0 ? x->nan_value : -1;
    d.null_ord = x->null_count > 0 ? x->null_value : -1;
    d.special_ord = x->special_first;
    return d;
}

// keys (and mask) of a probe call of n > 0 rows on the device: staged when they are host
// arrays (a host mask also when the keys are on the device)
struct IxProbeIn {
    HostStage stage;
    const void *keys;
    const uint8_t *mask;
};
static void ix_stage(vh_index *x, IxProbeIn &in, const void *keys, const uint8_t *mask, uint64_t n, int loc) {
    in.keys = loc == VH_LOC_HOST ? HostStage::copy(in.stage.keys, keys, n * dtype_itemsize(x->dtype)) : keys;
    in.mask = mask;
    if (mask && (loc == VH_LOC_HOST || resolve_loc(mask, VH_LOC_AUTO) == VH_LOC_HOST))
        in.mask = static_cast<const uint8_t *>(HostStage::copy(in.stage.mask, mask, n));
}

// The form per lookup table, from the A/B of DESIGN.md 5.18 (same process, 1e8 rows): the
// 8-consecutive-rows form where the table is staged in LDS and for every 16-byte table; the
// one-row-per-lane form for a packed table read from HBM (it ties k_set_map_ordinal at 1e5 and
// 1e7 keys, the 8-row form is 17 % behind at 1e7).
template <typename T, typename O>
static void ix_launch_map(const SetDev &sd, const void *keys, const uint8_t *mask, uint64_t n, void *out, uint32_t *unknown) {
    const uint64_t bytes = (sd.cap_mask + 1) * (sd.wide ? 16 : 8);
    const bool lds = bytes <= IX_LDS_BYTES;
    const T *k = static_cast<const T *>(keys);
    O *o = static_cast<O *>(out);
    const dim3 blk(IX_THREADS), grd8(blocks_for((n + IX_RPT - 1) / IX_RPT, IX_THREADS)), grd1(blocks_for(n, IX_THREADS));
    if (sd.wide && lds) hipLaunchKernelGGL((k_ix_map<T, O, true, true, IX_RPT, true>), grd8, blk, bytes, stream(), k, mask, n, sd, o, unknown);
    else if (sd.wide) hipLaunchKernelGGL((k_ix_map<T, O, true, false, IX_RPT, true>), grd8, blk, 0, stream(), k, mask, n, sd, o, unknown);
    else if (lds) hipLaunchKernelGGL((k_ix_map<T, O, false, true, IX_RPT, true>), grd8, blk, bytes, stream(), k, mask, n, sd, o, unknown);
    else hipLaunchKernelGGL((k_ix_map<T, O, false, false, 1, false>), grd1, blk, 0, stream(), k, mask, n, sd, o, unknown);
}

}  // namespace vh

extern "C" {

int vh_index_create(int dtype, uint64_t initial_capacity, vh_index **out) {
    VH_API_BEGIN
    dtype_itemsize(dtype);
    if (initial_capacity && (initial_capacity < 16 || (initial_capacity & (initial_capacity - 1))))
        fail(VH_ERR_ARG, "index_hash initial_capacity must be 0 or a power of two >= 16");
    std::unique_ptr<vh_index> x(new vh_index());
    x->dtype = dtype;
    x->explicit_cap = initial_capacity != 0;
    x->ctr.ensure(8 * (X_N + 1));  // + the probe's unknown flag
    slots_grow(x->tab, x->cap, initial_capacity ? initial_capacity : IX_DEFAULT_CAP);
    *out = x.release();
    VH_API_END
}

int vh_index_destroy(vh_index *x) {
    VH_API_BEGIN
    if (x) (void)hipStreamSynchronize(stream());
    delete x;
    VH_API_END
}

int vh_index_update(vh_index *x, const void *keys, const uint8_t *mask, const uint8_t *select, uint64_t n,
                    uint64_t start_index, int loc) {
    VH_API_BEGIN
    std::lock_guard<std::recursive_mutex> lk(x->mu);
    ix_update(x, keys, mask, select, n, start_index, loc);
    VH_API_END
}

int vh_index_merge(vh_index *x, vh_index *other) {
    VH_API_BEGIN
    if (x == other) fail(VH_ERR_ARG, "index_hash cannot merge with itself");
    std::lock_guard<std::recursive_mutex> lk(x->mu), lk2(other->mu);
    if (x->dtype != other->dtype) fail(VH_ERR_ARG, "index_hash merge: key dtypes differ");
    if (x->sealed || other->sealed) fail(VH_ERR_RUNTIME, "index_hash is sealed (it was probed), cannot merge");
    const int isz = dtype_itemsize(x->dtype);
    for (auto &src : other->chunks) {
        std::unique_ptr<IxChunk> ch(new IxChunk());
        ch->n = src->n;
        ch->row0 = src->row0;
        ch->has_flags = src->has_flags;
        ch->keys.ensure(src->n * isz);
        VH_HIP(hipMemcpyAsync(ch->keys.ptr, src->keys.ptr, src->n * isz, hipMemcpyDeviceToDevice, stream()));
        if (ch->has_flags) {
            ch->flags.ensure(src->n);
            VH_HIP(hipMemcpyAsync(ch->flags.ptr, src->flags.ptr, src->n, hipMemcpyDeviceToDevice, stream()));
        }
        ix_chunk(x, ch->keys.ptr, nullptr, nullptr, ch->has_flags ? ch->flags.as<uint8_t>() : nullptr, nullptr, ch->n,
                 ch->row0);
        x->chunks.push_back(std::move(ch));
    }
    VH_API_END
}

int vh_index_info(vh_index *x, int64_t *length, int64_t *nan_count, int64_t *null_count, int64_t *nan_value,
                  int64_t *null_value, int *has_duplicates) {
    VH_API_BEGIN
    std::lock_guard<std::recursive_mutex> lk(x->mu);
    if (length) *length = (int64_t)x->regular_rows + (x->nan_count > 0) + (x->null_count > 0);
    if (nan_count) *nan_count = x->nan_count;
    if (null_count) *null_count = x->null_count;
    if (nan_value) *nan_value = x->nan_count > 0 ? x->nan_value : -1;
    if (null_value) *null_value = x->null_count > 0 ? x->null_value : -1;
    if (has_duplicates) *has_duplicates = x->has_duplicates();
    VH_API_END
}

int vh_index_map_index(vh_index *x, const void *keys, const uint8_t *mask, uint64_t n, int loc, void *out,
                       int out_itemsize, int out_loc, int *found_unknown) {
    VH_API_BEGIN
    std::lock_guard<std::recursive_mutex> lk(x->mu);
    if (out_itemsize != 4 && out_itemsize != 8) fail(VH_ERR_ARG, "map_index: out_itemsize must be 4 or 8");
    if (out_itemsize == 4 && x->max_row > (uint64_t(1) << 31))
        fail(VH_ERR_ARG, "map_index: row numbers of 2^31 and more need an int64 output");
    ix_seal(x);
    if (found_unknown) *found_unknown = 0;
    if (!n) return VH_OK;
    loc = resolve_loc(keys, loc);
    out_loc = resolve_loc(out, out_loc);
    hipStream_t st = stream();
    IxProbeIn in;
    ix_stage(x, in, keys, mask, n, loc);
    DevBuf dout;
    void *dout_p = out;
    if (out_loc == VH_LOC_HOST) {
        dout.ensure(n * out_itemsize);
        dout_p = dout.ptr;
    }
    uint32_t *unknown = reinterpret_cast<uint32_t *>(x->ctr.as<uint64_t>() + X_N);
    VH_HIP(hipMemsetAsync(unknown, 0, 8, st));
    const SetDev sd = ix_view(x);
    {
        TimedScope ts("index_map_index");
        VH_DISPATCH_DTYPE(x->dtype, T, {
            if (out_itemsize == 4) ix_launch_map<T, int32_t>(sd, in.keys, in.mask, n, dout_p, unknown);
            else ix_launch_map<T, int64_t>(sd, in.keys, in.mask, n, dout_p, unknown);
        });
        VH_HIP(hipGetLastError());
    }
    if (out_loc == VH_LOC_HOST) VH_HIP(hipMemcpyAsync(out, dout_p, n * out_itemsize, hipMemcpyDeviceToHost, st));
    uint32_t u = 0;
    VH_HIP(hipMemcpyAsync(&u, unknown, 4, hipMemcpyDeviceToHost, st));
    VH_HIP(hipStreamSynchronize(st));
    if (found_unknown) *found_unknown = u != 0;
    VH_API_END
}

int vh_index_map_index_duplicates(vh_index *x, const void *keys, const uint8_t *mask, uint64_t n, uint64_t start_index,
                                  int loc, uint64_t *n_out, int64_t *left_out, int64_t *right_out) {
    VH_API_BEGIN
    std::lock_guard<std::recursive_mutex> lk(x->mu);
    hipStream_t st = stream();
    if (left_out || right_out) {
        // the second call: the pairs the count call left on the device
        if (!x->pairs_ready) fail(VH_ERR_RUNTIME, "map_index_duplicates: no counted pairs to read (call with NULL outputs first)");
        if (!left_out || !right_out) fail(VH_ERR_ARG, "map_index_duplicates: both outputs or none");
        if (x->pairs) {
            const hipMemcpyKind kl = resolve_loc(left_out, VH_LOC_AUTO) == VH_LOC_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
            const hipMemcpyKind kr = resolve_loc(right_out, VH_LOC_AUTO) == VH_LOC_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
            VH_HIP(hipMemcpyAsync(left_out, x->pair_left.ptr, x->pairs * 8, kl, st));
            VH_HIP(hipMemcpyAsync(right_out, x->pair_right.ptr, x->pairs * 8, kr, st));
            VH_HIP(hipStreamSynchronize(st));
        }
        if (n_out) *n_out = x->pairs;
        x->pair_left.release();
        x->pair_right.release();
        x->pairs = 0;
        x->pairs_ready = false;
        return VH_OK;
    }
    ix_seal(x);
    x->pairs = 0;
    x->pairs_ready = true;
    if (n_out) *n_out = 0;
    if (!n || !x->extras) return VH_OK;
    loc = resolve_loc(keys, loc);
    IxProbeIn in;
    ix_stage(x, in, keys, mask, n, loc);
    DevBuf cnt, off, beg, tmp;
    cnt.ensure((n + 1) * 4);
    off.ensure((n + 1) * 8);
    beg.ensure(n * 4);
    TimedScope ts("index_map_duplicates");
    VH_HIP(hipMemsetAsync(cnt.as<uint32_t>() + n, 0, 4, st));
    VH_DISPATCH_DTYPE(x->dtype, T,
                      hipLaunchKernelGGL(k_ix_dup_count<T>, dim3(blocks_for(n, 256)), dim3(256), 0, st,
                                         static_cast<const T *>(in.keys), in.mask, n, x->tab.as<uint64_t>(), x->cap - 1,
                                         slots_max_probe(x->cap), x->dup_begin.as<uint32_t>(), x->dup_count.as<uint32_t>(),
                                         cnt.as<uint32_t>(), beg.as<uint32_t>()));
    VH_HIP(hipGetLastError());
    // off[i] = pairs before left row i, off[n] = all pairs
    size_t tb = 0;
    VH_HIP(rocprim::exclusive_scan(nullptr, tb, cnt.as<uint32_t>(), off.as<uint64_t>(), (uint64_t)0, (size_t)(n + 1),
                                   rocprim::plus<uint64_t>(), st));
    tmp.ensure(std::max<size_t>(tb, 16));
    tb = tmp.bytes;
    VH_HIP(rocprim::exclusive_scan(tmp.ptr, tb, cnt.as<uint32_t>(), off.as<uint64_t>(), (uint64_t)0, (size_t)(n + 1),
                                   rocprim::plus<uint64_t>(), st));
    uint64_t total = 0;
    VH_HIP(hipMemcpyAsync(&total, off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    VH_HIP(hipStreamSynchronize(st));
    if (total) {
        x->pair_left.ensure(total * 8);
        x->pair_right.ensure(total * 8);
        hipLaunchKernelGGL(k_ix_dup_fill, dim3(blocks_for(total, 256)), dim3(256), 0, st, off.as<uint64_t>(),
                           beg.as<uint32_t>(), n, total, start_index, x->dup_rows.as<int64_t>(), x->pair_left.as<int64_t>(),
                           x->pair_right.as<int64_t>());
        VH_HIP(hipGetLastError());
        VH_HIP(hipStreamSynchronize(st));
    }
    x->pairs = total;
    if (n_out) *n_out = total;
    VH_API_END
}

int vh_take(int ncols, void *const *dsts, const void *const *srcs, const int *itemsizes, const void *idx, int idx_itemsize,
            uint64_t n, uint8_t *mask_out) {
    VH_API_BEGIN
    if (ncols < 0) fail(VH_ERR_ARG, "take: ncols < 0");
    if (idx_itemsize != 4 && idx_itemsize != 8) fail(VH_ERR_ARG, "take: idx_itemsize must be 4 or 8");
    for (int c = 0; c < ncols; c++)
        if (itemsizes[c] != 1 && itemsizes[c] != 2 && itemsizes[c] != 4 && itemsizes[c] != 8)
            fail(VH_ERR_ARG, "take: itemsizes must be 1, 2, 4 or 8");
    if (!n) return VH_OK;
    hipStream_t st = stream();
    TimedScope ts("take");
    const dim3 grd(blocks_for((n + TK_RPT - 1) / TK_RPT, 256)), blk(256);
    bool first = true;
    for (int c0 = 0; c0 < ncols || (first && mask_out); c0 += TK_COLS) {
        TakeArgs a{};
        a.ncols = std::max(0, std::min(TK_COLS, ncols - c0));
        for (int c = 0; c < a.ncols; c++) {
            a.dst[c] = dsts[c0 + c];
            a.src[c] = srcs[c0 + c];
            a.isz[c] = itemsizes[c0 + c];
        }
        uint8_t *mo = first ? mask_out : nullptr;
        if (idx_itemsize == 4) hipLaunchKernelGGL(k_take<int32_t>, grd, blk, 0, st, a, static_cast<const int32_t *>(idx), n, mo);
        else hipLaunchKernelGGL(k_take<int64_t>, grd, blk, 0, st, a, static_cast<const int64_t *>(idx), n, mo);
        VH_HIP(hipGetLastError());
        first = false;
    }
    VH_HIP(hipStreamSynchronize(st));
    VH_API_END
}

int vh_index_matched(const void *idx, int idx_itemsize, uint64_t n, uint64_t *m, int64_t *left_rows_out, void *idx_out) {
    VH_API_BEGIN
    if (idx_itemsize != 4 && idx_itemsize != 8) fail(VH_ERR_ARG, "matched: idx_itemsize must be 4 or 8");
    if (m) *m = 0;
    if (!n) return VH_OK;
    hipStream_t st = stream();
    TimedScope ts("index_matched");
    DevBuf flag, pos, tmp;
    flag.ensure(n + 1);  // byte flags, 64-bit offsets: 9 bytes of temporary per row
    pos.ensure((n + 1) * 8);
    VH_HIP(hipMemsetAsync(flag.as<uint8_t>() + n, 0, 1, st));
    const dim3 grd(blocks_for(n, 256)), blk(256);
    if (idx_itemsize == 4) hipLaunchKernelGGL(k_matched_flags<int32_t>, grd, blk, 0, st, static_cast<const int32_t *>(idx), n, flag.as<uint8_t>());
    else hipLaunchKernelGGL(k_matched_flags<int64_t>, grd, blk, 0, st, static_cast<const int64_t *>(idx), n, flag.as<uint8_t>());
    VH_HIP(hipGetLastError());
    size_t tb = 0;
    VH_HIP(rocprim::exclusive_scan(nullptr, tb, flag.as<uint8_t>(), pos.as<uint64_t>(), (uint64_t)0, (size_t)(n + 1),
                                   rocprim::plus<uint64_t>(), st));
    tmp.ensure(std::max<size_t>(tb, 16));
    tb = tmp.bytes;
    VH_HIP(rocprim::exclusive_scan(tmp.ptr, tb, flag.as<uint8_t>(), pos.as<uint64_t>(), (uint64_t)0, (size_t)(n + 1),
                                   rocprim::plus<uint64_t>(), st));
    if (idx_itemsize == 4)
        hipLaunchKernelGGL(k_matched_scatter<int32_t>, grd, blk, 0, st, static_cast<const int32_t *>(idx), pos.as<uint64_t>(), n,
                           left_rows_out, static_cast<int32_t *>(idx_out));
    else
        hipLaunchKernelGGL(k_matched_scatter<int64_t>, grd, blk, 0, st, static_cast<const int64_t *>(idx), pos.as<uint64_t>(), n,
                           left_rows_out, static_cast<int64_t *>(idx_out));
    VH_HIP(hipGetLastError());
    uint64_t total = 0;
    VH_HIP(hipMemcpyAsync(&total, pos.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    VH_HIP(hipStreamSynchronize(st));
    if (m) *m = total;
    VH_API_END
}

}  // extern "C"
