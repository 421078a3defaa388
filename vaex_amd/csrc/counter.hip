// counter_<dtype> on the GPU: key -> occurrence count
// (packages/vaex-core/src/hash_primitives.hpp:328-415), the hash map behind
// value_counts (expression.py:946-1061).
//
// Table: one open-address table in HBM, 16-byte slots {key bits zero-extended (EMPTY = ~0),
// int64 count}, linear probing from hash64(bits) as hashset.hpp.  64-bit keys whose bits
// equal EMPTY (int64 -1, uint64 max) are counted in a side counter ("special"); NaN rows and
// null (masked) rows have counters of their own.  Key identity is the ordered set's
// (hashset.hip si_row): every NaN is the one NaN entry, rows whose mask byte is set are the
// null entry, every other key compares by bit pattern (-0.0 and 0.0 are two keys).
//
// update: each workgroup owns a row range and counts it into an LDS table of CT_LT slots
//   {key bits, 32-bit count} (NaN / null / all-ones keys in LDS side words), 8 consecutive
//   rows per lane loaded wide, equal neighbours of a lane's 8 rows combined before the LDS
//   atomic.  At the end of the range every LDS slot with a count goes to the HBM table once:
//   a CAS on the key and one 64-bit atomicAdd of its count.  Inside the range the workgroup
//   looks up every CT_SEG_ROWS rows and flushes in the same way, then continues, when more
//   than half of the LDS slots are in use (the keys are dropped as well: a sorted column
//   keeps moving on to new keys) or before it has counted `flush_rows` rows since its last
//   flush (the host's bound, 2^20: no 32-bit count can come near wrapping).  512 workgroups
//   flushing the same 1e3 keys took ~0.1 ms per flush (same-address HBM atomics queue up),
//   so a flush every 2^16 rows was not kept.  A key that finds no LDS slot
//   in CT_LDS_PROBES probes goes straight to the HBM table.
//
// Growth never double counts: a chunk is counted into a SCRATCH table and merged only on
//   success.  Adds are not idempotent, so a chunk whose table fills up cannot be re-run on
//   top of what it already added; instead every chunk (of update and of add) counts into
//   the scratch table, with its NaN / null / special counts in scratch counters.  An insert
//   whose probe sequence passes SET_MAX_PROBE, or a flush that finds the table more than 3/4
//   full, raises the overflow flag: the scratch table is thrown away, allocated x4 and the
//   chunk counted again from its first row.  Only a chunk that ran to its end is committed:
//   the scratch table becomes the counter's table when that is still empty (one chunk, the
//   common case, is never copied), else the counter's table is first grown (rehashed with
//   its counts) until it can take every scratch key at <= 1/2 load, so that the merge
//   (unbounded probing) cannot be refused, and the host counters are added last.  A failed
//   allocation throws before anything is committed: no result is ever partial.
//   For chunks of >= CT_SAMPLE_MIN rows the scratch table is sized before the pass from a
//   sample (2^16 pseudo-random rows counted into the scratch table, Chao1 estimate of the
//   distinct keys from the keys seen once and twice), so a retry is the exception.
//
// read (the device finish): occupied slots are compacted to (order-preserving transform of
//   the key bits, count), the special key appended, the pairs radix-sorted by key (numeric
//   order, -0.0 before 0.0), NaN put at index 0 and null at the next index
//   (key_offset / null_offset, hash_primitives.hpp:338-348, expression.py:1026-1044), then
//   for order 1 / 2 a stable ascending radix sort by count (order 2 its exact reverse:
//   np.argsort(counts)[::-1], expression.py:1046-1050).  Only the answer is read back.
#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>
#include <type_traits>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.hpp"
#include "hashset.hpp"
#include "lds_table.hpp"
#include "slot_table.hpp"

using namespace vh;

enum { K_OVERFLOW = 0, K_NEW, K_NAN, K_NULL, K_SPECIAL, K_CURSOR, K_NULL_INDEX, K_BAD, K_D, K_F1, K_F2, K_N };

struct CtTable {
    DevBuf buf;
    uint64_t cap = 0;
    uint64_t distinct = 0;
    bool clean = false;  // every slot {EMPTY, 0}
};

struct vh_counter {
    std::recursive_mutex mu;  // counter.update may be called from several threads (cpu.py map)
    int dtype = VH_I64;
    uint64_t initial_cap = 0;
    CtTable main, scratch;
    DevBuf ctr;
    HostStage stage;
    int64_t nan_count = 0, null_count = 0, special_count = 0;
};

namespace vh {

constexpr uint32_t CT_LT_LOG2 = 13;
constexpr uint32_t CT_LT = 1u << CT_LT_LOG2;  // LDS slots: 64 KiB (<= 4-byte keys), 96 KiB (8-byte keys)
constexpr int CT_RPT = 8;                     // consecutive rows per lane and step: one load_rows8 group
static_assert(CT_RPT == ROWS8, "load_rows8 takes 8 rows");
constexpr int CT_LDS_PROBES = 16;
constexpr uint64_t CT_SEG_ROWS = uint64_t(1) << 16;    // a workgroup looks at its LDS fill this often
constexpr uint64_t CT_FLUSH_ROWS = uint64_t(1) << 20;  // most rows of a workgroup between two flushes
constexpr uint64_t CT_MIN_WG_ROWS = uint64_t(1) << 17;  // a workgroup's range is at least this long
constexpr uint64_t CT_DEFAULT_CAP = uint64_t(1) << 16;
constexpr uint64_t CT_SAMPLE_MIN = uint64_t(1) << 20;
constexpr uint64_t CT_SAMPLE_ROWS = uint64_t(1) << 16;

// 8-byte keys: one 1024-lane workgroup per CU (96 KiB of LDS); else two of 512 (64 KiB each)
template <typename KB> constexpr int ct_threads() { return sizeof(KB) == 8 ? 1024 : 512; }
template <typename KB> constexpr size_t ct_lds_bytes() { return (sizeof(KB) + 4) * (size_t)CT_LT; }

struct CtDev {
    uint64_t *tab;
    uint64_t cap_mask, max_probe, limit;
    uint64_t *ctr;
};

struct CtParams {
    const void *keys;
    const uint8_t *mask, *select;
    uint64_t n, rows_per_wg, seg_rows, flush_rows;
};

// (key, count) into the HBM table: CAS on the key, one 64-bit add of the count.  New keys are
// counted per workgroup in LDS (`wg_new`).  A probe sequence past max_probe raises overflow.
__device__ inline void ct_insert(const CtDev &g, uint64_t kb, uint64_t cnt, uint32_t *wg_new) {
    set_claim(g.tab, g.cap_mask, g.max_probe, kb, wg_new, &g.ctr[K_OVERFLOW],
              [&](uint64_t *count) { atomicAdd((unsigned long long *)count, (unsigned long long)cnt); });
}

template <typename KB> struct CtLds {
    KB *keys;
    uint32_t *cnt;
    uint32_t *used, *wg_new;
};

// `run` occurrences of a regular key into the LDS table, or straight to HBM when no slot
template <typename KB> __device__ inline void ct_lds_add(const CtLds<KB> &t, const CtDev &g, KB k, uint32_t run) {
    constexpr KB EMPTY = ~KB(0);
    uint32_t h = lds_hash((uint64_t)k) & (CT_LT - 1);
    for (int pr = 0; pr < CT_LDS_PROBES; pr++) {
        KB cur = t.keys[h];
        if (cur == EMPTY) {
            cur = lds_cas(&t.keys[h], EMPTY, k);
            if (cur == EMPTY) {
                atomicAdd(t.used, 1u);
                cur = k;
            }
        }
        if (cur == k) {
            atomicAdd(&t.cnt[h], run);
            return;
        }
        h = (h + 1) & (CT_LT - 1);
    }
    ct_insert(g, (uint64_t)k, run, t.wg_new);  // run > 1: equal neighbours of the lane's 8 rows
}

template <typename T>
__global__ __launch_bounds__(ct_threads<kb_t<T>>()) void k_ct_count(CtParams p, CtDev g) {
    using KB = kb_t<T>;
    constexpr int THREADS = ct_threads<KB>();
    constexpr KB EMPTY = ~KB(0);
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ uint32_t s_nan, s_null, s_top, s_used, s_new, s_stop;
    CtLds<KB> t;
    t.keys = reinterpret_cast<KB *>(lds_raw);
    t.cnt = reinterpret_cast<uint32_t *>(lds_raw + sizeof(KB) * CT_LT);
    t.used = &s_used;
    t.wg_new = &s_new;
    for (uint32_t i = threadIdx.x; i < CT_LT; i += THREADS) {
        t.keys[i] = EMPTY;
        t.cnt[i] = 0;
    }
    if (threadIdx.x == 0) s_nan = s_null = s_top = s_used = s_new = s_stop = 0;
    __syncthreads();
    const T *keys = static_cast<const T *>(p.keys);
    // rows_per_wg and seg_rows are multiples of the step, so every lane's 8 rows start at a
    // multiple of 8: the columns' base addresses decide the alignment
    const bool al = aligned_rows8(keys, sizeof(T)) && (!p.mask || aligned_rows8(p.mask, 1)) &&
                    (!p.select || aligned_rows8(p.select, 1));
    const uint64_t r0 = blockIdx.x * p.rows_per_wg, r1 = min(p.n, r0 + p.rows_per_wg);
    uint64_t since = 0;  // rows counted into LDS since the last flush
    for (uint64_t s0 = r0; s0 < r1; s0 += p.seg_rows) {
        const uint64_t s1 = min(r1, s0 + p.seg_rows);
        for (uint64_t b0 = s0; b0 < s1; b0 += (uint64_t)THREADS * CT_RPT) {
            const uint64_t j = b0 + (uint64_t)threadIdx.x * CT_RPT;
            if (j >= s1) continue;
            const uint32_t cnt = (uint32_t)min<uint64_t>(CT_RPT, s1 - j);
            T v[CT_RPT];
            uint8_t m[CT_RPT], sel[CT_RPT];
            load_rows8<T>(keys, j, cnt, al, v);
            if (p.mask) load_rows8<uint8_t>(p.mask, j, cnt, al, m);
            if (p.select) load_rows8<uint8_t>(p.select, j, cnt, al, sel);
            KB pk = 0;
            uint32_t run = 0;  // the lane's current run of equal regular keys
#pragma unroll
            for (int u = 0; u < CT_RPT; u++) {
                if ((uint32_t)u >= cnt) continue;
                if (p.select && !sel[u]) continue;  // filtered out / not selected: not seen
                if (p.mask && m[u]) {
                    atomicAdd(&s_null, 1u);
                    continue;
                }
                if (is_nan_v(v[u])) {
                    atomicAdd(&s_nan, 1u);
                    continue;
                }
                const KB k = (KB)key_bits(v[u]);
                if (k == EMPTY) {  // the LDS EMPTY pattern: 8-byte keys the special key, else a regular one
                    atomicAdd(&s_top, 1u);
                    continue;
                }
                if (run && k == pk) {
                    run++;
                    continue;
                }
                if (run) ct_lds_add<KB>(t, g, pk, run);
                pk = k;
                run = 1;
            }
            if (run) ct_lds_add<KB>(t, g, pk, run);
        }
        __syncthreads();
        // flush when the range is done, when more than half of the LDS slots are in use (then
        // the keys are dropped too: a sorted column keeps moving on to new keys), or before
        // the rows since the last flush could pass the host's bound on a 32-bit count
        since += s1 - s0;
        const bool clear = s_used > CT_LT / 2;  // uniform: read between two barriers
        if (!(s1 >= r1 || clear || since + p.seg_rows > p.flush_rows)) {
            __syncthreads();  // s_used is read by every lane before the next segment changes it
            continue;
        }
        since = 0;
        for (uint32_t i = threadIdx.x; i < CT_LT; i += THREADS) {
            const uint32_t c = t.cnt[i];
            if (c) {
                ct_insert(g, (uint64_t)t.keys[i], c, &s_new);
                t.cnt[i] = 0;
            }
            if (clear) t.keys[i] = EMPTY;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (clear) s_used = 0;
            if (s_nan) atomicAdd((unsigned long long *)&g.ctr[K_NAN], (unsigned long long)s_nan);
            if (s_null) atomicAdd((unsigned long long *)&g.ctr[K_NULL], (unsigned long long)s_null);
            if (s_top) {
                if constexpr (sizeof(KB) == 8) atomicAdd((unsigned long long *)&g.ctr[K_SPECIAL], (unsigned long long)s_top);
                else ct_insert(g, (uint64_t)EMPTY, s_top, &s_new);
            }
            s_nan = s_null = s_top = 0;
            // the keys this workgroup added: past the limit the chunk is counted again in a
            // larger table, and every workgroup stops at its next flush
            uint64_t total = 0;
            if (s_new) total = atomicAdd((unsigned long long *)&g.ctr[K_NEW], (unsigned long long)s_new) + s_new;
            s_new = 0;
            if (total > g.limit) atomicOr((unsigned long long *)&g.ctr[K_OVERFLOW], 1ULL);
            s_stop = __hip_atomic_load(&g.ctr[K_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        }
        __syncthreads();
        if (s_stop) break;
    }
}

// row i adds counts[i] (vh_counter_add: merge and un-pickle)
template <typename T>
__global__ __launch_bounds__(256) void k_ct_add(const T *keys, const uint8_t *mask, const int64_t *counts, uint64_t n, CtDev g) {
    __shared__ uint32_t s_new;
    if (threadIdx.x == 0) s_new = 0;
    __syncthreads();
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const int64_t c = counts[i];
        if (c <= 0) {
            if (c < 0) atomicOr((unsigned long long *)&g.ctr[K_BAD], 1ULL);
            continue;
        }
        if (mask && mask[i]) {
            atomicAdd((unsigned long long *)&g.ctr[K_NULL], (unsigned long long)c);
            continue;
        }
        const T v = keys[i];
        if (is_nan_v(v)) {
            atomicAdd((unsigned long long *)&g.ctr[K_NAN], (unsigned long long)c);
            continue;
        }
        const uint64_t kb = key_bits(v);
        if (kb == SET_EMPTY) {
            atomicAdd((unsigned long long *)&g.ctr[K_SPECIAL], (unsigned long long)c);
            continue;
        }
        ct_insert(g, kb, (uint64_t)c, &s_new);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_new) atomicAdd((unsigned long long *)&g.ctr[K_NEW], (unsigned long long)s_new);
}

// the sample: pseudo-random rows' regular keys, each with a count of 1
template <typename T>
__global__ __launch_bounds__(256) void k_ct_sample(const T *keys, const uint8_t *mask, const uint8_t *select, uint64_t n,
                                                   uint64_t m, CtDev g) {
    __shared__ uint32_t s_new;
    if (threadIdx.x == 0) s_new = 0;
    __syncthreads();
    for (uint64_t s = blockIdx.x * 256ull + threadIdx.x; s < m; s += (uint64_t)gridDim.x * 256) {
        const uint64_t i = hash64(s * 0x9E3779B97F4A7C15ULL + 1) % n;
        if (select && !select[i]) continue;
        if (mask && mask[i]) continue;
        const T v = keys[i];
        if (is_nan_v(v)) continue;
        const uint64_t kb = key_bits(v);
        if (kb == SET_EMPTY) continue;
        ct_insert(g, kb, 1, &s_new);
    }
}

// every occupied slot of `src` into the table of `g` (rehash with counts; scratch -> counter)
__global__ __launch_bounds__(256) void k_ct_merge(const uint64_t *src, uint64_t scap, CtDev g) {
    __shared__ uint32_t s_new;
    if (threadIdx.x == 0) s_new = 0;
    __syncthreads();
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < scap; i += (uint64_t)gridDim.x * 256) {
        const ulonglong2 e = reinterpret_cast<const ulonglong2 *>(src)[i];
        if (e.x == SET_EMPTY) continue;
        ct_insert(g, e.x, e.y, &s_new);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_new) atomicAdd((unsigned long long *)&g.ctr[K_NEW], (unsigned long long)s_new);
}

// ---- finish ---------------------------------------------------------------------------------
// key bits (zero-extended) <-> a u64 whose unsigned order is the key's numeric order; floats
// by their bit pattern, so -0.0 sorts just before 0.0
template <typename T> __host__ __device__ inline uint64_t ct_ordered(uint64_t b) {
    if constexpr (std::is_same_v<T, double>) {
        return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
    } else if constexpr (std::is_same_v<T, float>) {
        const uint32_t u = (uint32_t)b;
        return (u >> 31) ? (uint32_t)~u : (u | 0x80000000u);
    } else if constexpr (is_signed_int_t<T>::value) {
        int64_t s;
        if constexpr (sizeof(T) == 8) s = (int64_t)b;
        else if constexpr (sizeof(T) == 4) s = (int32_t)(uint32_t)b;
        else if constexpr (sizeof(T) == 2) s = (int16_t)(uint16_t)b;
        else s = (int8_t)(uint8_t)b;
        return (uint64_t)s ^ 0x8000000000000000ULL;
    } else {
        return b;
    }
}

template <typename T> __host__ __device__ inline uint64_t ct_unordered(uint64_t o) {
    if constexpr (std::is_same_v<T, double>) {
        return (o >> 63) ? (o & 0x7fffffffffffffffULL) : ~o;
    } else if constexpr (std::is_same_v<T, float>) {
        const uint32_t u = (uint32_t)o;
        return (u >> 31) ? (u & 0x7fffffffu) : (uint32_t)~u;
    } else if constexpr (is_signed_int_t<T>::value) {
        return o ^ 0x8000000000000000ULL;  // the low sizeof(T) bytes are the key
    } else {
        return o;
    }
}

// what the finish keeps of an occupied slot: the key's sortable form and its count
template <typename T> struct CtCompact {
    static constexpr bool WIDE = true;
    uint64_t *okey, *cnt;
    __device__ void operator()(uint64_t j, uint64_t, uint64_t kb, uint64_t count) const {
        okey[j] = ct_ordered<T>(kb);
        cnt[j] = count;
    }
};

// the answer: entry j of the (count-sorted, maybe reversed) list as a typed key and a count
template <typename T>
__global__ __launch_bounds__(256) void k_ct_emit(const uint64_t *okey, const uint64_t *cnt, const uint64_t *order,
                                                 uint64_t n, int64_t nan_pos, int64_t null_pos, int reverse, T *out_keys,
                                                 int64_t *out_counts, uint64_t *ctr) {
    for (uint64_t j = blockIdx.x * 256ull + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256) {
        const uint64_t src = order ? order[j] : j;
        const uint64_t dst = reverse ? n - 1 - j : j;
        T k{};  // the null entry's key value is the dtype's zero
        if ((int64_t)src == nan_pos) {
            if constexpr (is_float_t<T>::value) k = (T)__builtin_nan("");
        } else if ((int64_t)src == null_pos) {
            ctr[K_NULL_INDEX] = dst;
        } else {
            const uint64_t b = ct_unordered<T>(okey[src]);
            __builtin_memcpy(&k, &b, sizeof(T));
        }
        out_keys[dst] = k;
        out_counts[dst] = (int64_t)cnt[src];
    }
}

// ---- host -------------------------------------------------------------------------------------
static void ct_clear(CtTable &t) {
    if (t.clean || !t.cap) return;
    slots_fresh(t.buf, t.cap, SlotPayload::ZERO);
    t.clean = true;
    t.distinct = 0;
}

// a fresh, clean table of `cap` slots (the old one is released first: it holds nothing kept)
static void ct_alloc(CtTable &t, uint64_t cap) {
    t.buf.release();
    t.cap = 0;
    t.distinct = 0;
    t.clean = false;
    t.buf.ensure(cap * 16);
    t.cap = cap;
    ct_clear(t);
}

static CtDev ct_dev(vh_counter *c, const CtTable &t, bool unbounded) {
    CtDev g;
    g.tab = t.buf.as<uint64_t>();
    g.cap_mask = t.cap - 1;
    g.max_probe = unbounded ? t.cap : slots_max_probe(t.cap);
    g.limit = unbounded ? ~0ULL : t.cap / 4 * 3;
    g.ctr = c->ctr.as<uint64_t>();
    return g;
}

static void ct_zero_ctr(vh_counter *c) { VH_HIP(hipMemsetAsync(c->ctr.ptr, 0, 8 * K_N, stream())); }

// One chunk (device-resident) through `launch`, which counts it into the table it is given.
// Transactional: see "Growth never double counts" at the top of the file.
template <typename F> static void ct_chunk(vh_counter *c, uint64_t want_cap, F &&launch) {
    hipStream_t st = stream();
    CtTable &S = c->scratch;
    if (S.cap < want_cap) ct_alloc(S, want_cap);
    std::vector<uint64_t> k;
    for (;;) {
        ct_clear(S);
        ct_zero_ctr(c);
        S.clean = false;
        launch(ct_dev(c, S, false));
        VH_HIP(hipGetLastError());
        k = slots_read_ctr(c->ctr, K_N);
        if (k[K_BAD]) fail(VH_ERR_ARG, "counter add: negative count");
        if (!k[K_OVERFLOW]) break;
        ct_alloc(S, S.cap * 4);
    }
    S.distinct = k[K_NEW];
    CtTable &M = c->main;
    if (M.distinct == 0) {
        // the counter's table holds nothing: the scratch table becomes it
        M.buf.swap(S.buf);
        std::swap(M.cap, S.cap);
        std::swap(M.distinct, S.distinct);
        std::swap(M.clean, S.clean);
    } else if (S.distinct) {
        const uint64_t need = M.distinct + S.distinct;
        uint64_t ncap = M.cap;
        while (ncap < 2 * need) ncap *= 2;
        // the new table is allocated before anything changes: a failure leaves the counter as it was
        if (ncap != M.cap) slots_grow(M.buf, M.cap, ncap, SlotPayload::ZERO);
        ct_zero_ctr(c);
        hipLaunchKernelGGL(k_ct_merge, dim3(blocks_for(S.cap, 256)), dim3(256), 0, st, S.buf.as<uint64_t>(), S.cap,
                           ct_dev(c, M, true));
        VH_HIP(hipGetLastError());
        const auto k2 = slots_read_ctr(c->ctr, K_N);
        if (k2[K_OVERFLOW]) fail(VH_ERR_RUNTIME, "counter merge: table full (internal error)");
        M.distinct += k2[K_NEW];
        M.clean = false;
    }
    c->nan_count += (int64_t)k[K_NAN];
    c->null_count += (int64_t)k[K_NULL];
    c->special_count += (int64_t)k[K_SPECIAL];
}

// slots for the scratch table of a chunk of n rows: from a sample for long chunks
template <typename T>
static uint64_t ct_size_from_sample(vh_counter *c, const T *keys, const uint8_t *mask, const uint8_t *select, uint64_t n) {
    uint64_t cap = c->initial_cap;
    if (n < CT_SAMPLE_MIN) return cap;
    CtTable &S = c->scratch;
    if (S.cap < 4 * CT_SAMPLE_ROWS) ct_alloc(S, 4 * CT_SAMPLE_ROWS);
    ct_clear(S);
    ct_zero_ctr(c);
    S.clean = false;
    hipLaunchKernelGGL(k_ct_sample<T>, dim3(blocks_for(CT_SAMPLE_ROWS, 256)), dim3(256), 0, stream(), keys, mask, select, n,
                       CT_SAMPLE_ROWS, ct_dev(c, S, true));
    static_assert(K_F1 == K_D + 1 && K_F2 == K_D + 2, "k_sample_stats adds to three consecutive counters");
    hipLaunchKernelGGL(k_sample_stats<SampleSlotCounts>, dim3(blocks_for(S.cap, 256)), dim3(256), 0, stream(),
                       SampleSlotCounts{S.buf.as<uint64_t>()}, S.cap, c->ctr.as<unsigned long long>() + K_D);
    VH_HIP(hipGetLastError());
    const auto k = slots_read_ctr(c->ctr, K_N);
    const double d = (double)k[K_D], f1 = (double)k[K_F1], f2 = (double)k[K_F2];
    // Chao1; with no key seen twice every sampled key may be distinct: as many as the rows
    double est = f2 > 0 ? d + f1 * f1 / (2 * f2) : (f1 > 0 ? (double)n : d);
    est = std::min(est, (double)n);
    // under 1/2 of the 3/4 limit, and not past 2^28 slots (4 GiB): a larger table is grown into
    cap = std::max(cap, std::min<uint64_t>(next_pow2((uint64_t)(est * 3) + 1), uint64_t(1) << 28));
    return cap;
}

template <typename T>
static void ct_count_chunk(vh_counter *c, const void *keys, const uint8_t *mask, const uint8_t *select, uint64_t n) {
    using KB = kb_t<T>;
    constexpr int THREADS = ct_threads<KB>();
    constexpr uint64_t STEP = (uint64_t)THREADS * CT_RPT;
    constexpr size_t lds = ct_lds_bytes<KB>();
    const uint64_t want = ct_size_from_sample<T>(c, static_cast<const T *>(keys), mask, select, n);
    int bpc = 0;
    VH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, reinterpret_cast<const void *>(k_ct_count<T>), THREADS, lds));
    bpc = std::max(1, bpc);
    const uint64_t W = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)cu_count() * bpc,
                                                                 (n + CT_MIN_WG_ROWS - 1) / CT_MIN_WG_ROWS));
    CtParams p{};
    p.keys = keys;
    p.mask = mask;
    p.select = select;
    p.n = n;
    p.rows_per_wg = ((n + W - 1) / W + STEP - 1) / STEP * STEP;
    p.seg_rows = (CT_SEG_ROWS + STEP - 1) / STEP * STEP;
    // the bound on a 32-bit LDS count: at most this many rows between two flushes
    p.flush_rows = CT_FLUSH_ROWS;
    static_assert(CT_FLUSH_ROWS < (uint64_t(1) << 31) && CT_SEG_ROWS <= CT_FLUSH_ROWS, "32-bit LDS counts");
    ct_chunk(c, want, [&](const CtDev &g) {
        TimedScope ts("counter_update");
        hipLaunchKernelGGL(k_ct_count<T>, dim3((unsigned)W), dim3(THREADS), lds, stream(), p, g);
    });
}

static void ct_update(vh_counter *c, const void *keys, const uint8_t *mask, const uint8_t *select, const int64_t *counts,
                      uint64_t n, int loc) {
    loc = resolve_loc(keys, loc);
    // host columns are staged per 16 Mi rows; device columns are one chunk
    c->stage.chunks({keys, mask, select, counts}, dtype_itemsize(c->dtype), n, loc, uint64_t(1) << 24, std::max<uint64_t>(n, 1),
                    [&](const HashCols &d, uint64_t len, uint64_t) {
                        if (counts) {
                            VH_DISPATCH_DTYPE(c->dtype, T, ct_chunk(c, std::max<uint64_t>(c->initial_cap, 16), [&](const CtDev &g) {
                                                  hipLaunchKernelGGL(k_ct_add<T>, dim3(blocks_for(len, 256)), dim3(256), 0, stream(),
                                                                     static_cast<const T *>(d.keys), d.mask, d.counts, len, g);
                                              }));
                        } else {
                            VH_DISPATCH_DTYPE(c->dtype, T, ct_count_chunk<T>(c, d.keys, d.mask, d.select, len));
                        }
                    });
}

template <typename T>
static void ct_read(vh_counter *c, int order, bool dropnan, bool dropmissing, void *keys_out, int64_t *counts_out,
                    uint64_t *n_out, int64_t *null_index) {
    hipStream_t st = stream();
    CtTable &M = c->main;
    const bool has_nan = c->nan_count > 0 && !dropnan, has_null = c->null_count > 0 && !dropmissing;
    const bool has_special = c->special_count > 0;
    const uint64_t H = (has_nan ? 1 : 0) + (has_null ? 1 : 0);
    const uint64_t m = M.distinct + (has_special ? 1 : 0);
    const uint64_t N = H + m;
    *n_out = N;
    *null_index = -1;
    if (!N) return;
    TimedScope ts("counter_read");
    DevBuf ck, cc, lk, lc, tmp, idx, scnt, sidx, okeys, ocnt;
    ck.ensure(std::max<uint64_t>(m, 1) * 8);
    cc.ensure(std::max<uint64_t>(m, 1) * 8);
    lk.ensure(N * 8);
    lc.ensure(N * 8);
    // 1. compact the occupied slots, 2. append the special key
    ct_zero_ctr(c);
    if (M.distinct) {
        slots_compact(M.buf, M.cap, c->ctr.as<uint64_t>() + K_CURSOR, CtCompact<T>{ck.as<uint64_t>(), cc.as<uint64_t>()});
    }
    uint64_t head[4] = {0, 0, 0, 0};  // outlives the asynchronous copies below (synchronised before return)
    if (has_special) {
        head[0] = ct_ordered<T>(SET_EMPTY);
        head[1] = (uint64_t)c->special_count;
        VH_HIP(hipMemcpyAsync(ck.as<uint64_t>() + M.distinct, &head[0], 8, hipMemcpyHostToDevice, st));
        VH_HIP(hipMemcpyAsync(cc.as<uint64_t>() + M.distinct, &head[1], 8, hipMemcpyHostToDevice, st));
    }
    // 3. ascending key order, written behind the NaN / null entries
    if (m) {
        size_t tb = 0;
        VH_HIP(rocprim::radix_sort_pairs(nullptr, tb, ck.as<uint64_t>(), lk.as<uint64_t>() + H, cc.as<uint64_t>(),
                                         lc.as<uint64_t>() + H, (size_t)m, 0, 64, st));
        tmp.ensure(std::max<size_t>(tb, 16));
        tb = tmp.bytes;
        VH_HIP(rocprim::radix_sort_pairs(tmp.ptr, tb, ck.as<uint64_t>(), lk.as<uint64_t>() + H, cc.as<uint64_t>(),
                                         lc.as<uint64_t>() + H, (size_t)m, 0, 64, st));
    }
    // 4. NaN at index 0, null at the next
    const int64_t nan_pos = has_nan ? 0 : -1, null_pos = has_null ? (has_nan ? 1 : 0) : -1;
    if (has_nan) head[2] = (uint64_t)c->nan_count;
    if (has_null) head[2 + null_pos] = (uint64_t)c->null_count;
    if (H) {
        VH_HIP(hipMemsetAsync(lk.ptr, 0, H * 8, st));
        VH_HIP(hipMemcpyAsync(lc.ptr, &head[2], H * 8, hipMemcpyHostToDevice, st));
    }
    // 5. stable ascending sort by count
    const uint64_t *ord = nullptr;
    if (order != 0) {
        idx.ensure(N * 8);
        scnt.ensure(N * 8);
        sidx.ensure(N * 8);
        hipLaunchKernelGGL(k_iota<uint64_t>, dim3(blocks_for(N, 256)), dim3(256), 0, st, idx.as<uint64_t>(), N);
        VH_HIP(hipGetLastError());
        size_t tb = 0;
        VH_HIP(rocprim::radix_sort_pairs(nullptr, tb, lc.as<uint64_t>(), scnt.as<uint64_t>(), idx.as<uint64_t>(),
                                         sidx.as<uint64_t>(), (size_t)N, 0, 64, st));
        if (tb > tmp.bytes) {
            VH_HIP(hipStreamSynchronize(st));  // the key sort may still use it
            tmp.ensure(tb);
        }
        tb = tmp.bytes;
        VH_HIP(rocprim::radix_sort_pairs(tmp.ptr, tb, lc.as<uint64_t>(), scnt.as<uint64_t>(), idx.as<uint64_t>(),
                                         sidx.as<uint64_t>(), (size_t)N, 0, 64, st));
        ord = sidx.as<uint64_t>();
    }
    okeys.ensure(N * sizeof(T));
    ocnt.ensure(N * 8);
    hipLaunchKernelGGL(k_ct_emit<T>, dim3(blocks_for(N, 256)), dim3(256), 0, st, lk.as<uint64_t>(), lc.as<uint64_t>(), ord, N,
                       nan_pos, null_pos, order == 2 ? 1 : 0, okeys.as<T>(), ocnt.as<int64_t>(), c->ctr.as<uint64_t>());
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemcpyAsync(keys_out, okeys.ptr, N * sizeof(T), hipMemcpyDeviceToHost, st));
    VH_HIP(hipMemcpyAsync(counts_out, ocnt.ptr, N * 8, hipMemcpyDeviceToHost, st));
    const auto k = slots_read_ctr(c->ctr, K_N);
    if (has_null) *null_index = (int64_t)k[K_NULL_INDEX];
}

}  // namespace vh

extern "C" {

int vh_counter_create(int dtype, uint64_t initial_capacity, vh_counter **out) {
    VH_API_BEGIN
    dtype_itemsize(dtype);
    if (initial_capacity && (initial_capacity < 16 || (initial_capacity & (initial_capacity - 1))))
        fail(VH_ERR_ARG, "counter initial_capacity must be 0 or a power of two >= 16");
    std::unique_ptr<vh_counter> c(new vh_counter());
    c->dtype = dtype;
    c->initial_cap = initial_capacity ? initial_capacity : CT_DEFAULT_CAP;
    c->ctr.ensure(8 * K_N);
    *out = c.release();
    VH_API_END
}

int vh_counter_destroy(vh_counter *c) {
    VH_API_BEGIN
    if (c) (void)hipStreamSynchronize(stream());
    delete c;
    VH_API_END
}

int vh_counter_update(vh_counter *c, const void *keys, const uint8_t *mask, const uint8_t *select, uint64_t n, int loc) {
    VH_API_BEGIN
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    ct_update(c, keys, mask, select, nullptr, n, loc);
    VH_API_END
}

int vh_counter_add(vh_counter *c, const void *keys, const uint8_t *mask, const int64_t *counts, uint64_t n, int loc) {
    VH_API_BEGIN
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!counts && n) fail(VH_ERR_ARG, "counter add: counts is NULL");
    ct_update(c, keys, mask, nullptr, counts, n, loc);
    VH_API_END
}

int vh_counter_info(vh_counter *c, int64_t *length, int64_t *nan_count, int64_t *null_count) {
    VH_API_BEGIN
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (length)
        *length = (int64_t)c->main.distinct + (c->special_count > 0) + (c->nan_count > 0) + (c->null_count > 0);
    if (nan_count) *nan_count = c->nan_count;
    if (null_count) *null_count = c->null_count;
    VH_API_END
}

int vh_counter_read(vh_counter *c, int order, int dropnan, int dropmissing, void *keys_out, int64_t *counts_out,
                    uint64_t *n_out, int64_t *null_index) {
    VH_API_BEGIN
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (order < 0 || order > 2) fail(VH_ERR_ARG, "counter read: order must be 0, 1 or 2");
    uint64_t n = 0;
    int64_t ni = -1;
    VH_DISPATCH_DTYPE(c->dtype, T, ct_read<T>(c, order, dropnan != 0, dropmissing != 0, keys_out, counts_out, &n, &ni));
    if (n_out) *n_out = n;
    if (null_index) *null_index = ni;
    VH_API_END
}

}  // extern "C"
