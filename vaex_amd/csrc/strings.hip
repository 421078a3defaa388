// Device string columns (Arrow layout: n + 1 int32 / int64 offsets into a byte buffer, all in
// HBM): the offset check, the element-wise kernels (vh_str_len, vh_str_match), the byte-exact
// gather (vh_str_take) and the dictionary encoder (vh_strset_*, the reference's
// superutils.ordered_set_string).  The per-string functions are str_dev.hpp; DESIGN.md 5.25.
//
// Every kernel takes the offsets as checked by vh_str_validate (non-negative, non-decreasing,
// the last at most the buffer's length): a row's bytes then lie inside the buffer, whose
// allocation is 8-aligned and carries at least 16 bytes of slack, which is what load_word needs.
//
// The row kernels (hash + insert, verify, map_ordinal, copy) come in two forms, chosen on the
// host from the mean length bytes / rows.  Lane per row: short strings; neighbouring rows are
// neighbouring bytes, so a wave's loads fall into a contiguous span.  Wave per row: the 64 lanes
// share one string's words (hash terms add up, comparisons vote), for long strings.
//
// The encoder.  A level is a 16-byte slot table (slot_table.hpp) whose key is the string's
// 64-bit hash under the level's seed and whose payload is the string: while an update runs,
// ROWFLAG | the first row of the column holding it (folded with atomicMin), afterwards its
// index in the set's own dictionary (int64 offsets + bytes in HBM), so the set outlives the
// column.  Round r of an update: every unresolved row claims (hash_r, row) in level r; a verify
// pass compares each row's bytes with its slot's string; equal rows are resolved, unequal rows
// are true hash collisions and are compacted into the next round's list.  The slot's first row
// is itself resolved, so every round resolves at least one distinct string and the loop ends;
// the host reads one counter pair per round.  No lane ever waits for another: no spin loop.
// A string sits at level r only if every lower level holds a different string at its hash, so a
// probe walks level 0, 1, ... and stops at the first level without its hash: absent.
#include <rocprim/device/device_radix_sort.hpp>

#include <atomic>
#include <deque>

#include "common.hpp"
#include "hashset.hpp"
#include "slot_table.hpp"
#include "str_col.hpp"

namespace vh {

constexpr uint64_t ROWFLAG = 1ULL << 62;  // payload: a row of the column being added (else a dictionary index)
constexpr int STRSET_MAX_LEVELS = 64;

static std::atomic<uint64_t> g_strset_rounds{0}, g_strset_form{0};
uint64_t stat_strset_rounds(bool reset) { return reset ? g_strset_rounds.exchange(0) : g_strset_rounds.load(); }
uint64_t stat_strset_form(bool reset) { return reset ? g_strset_form.exchange(0) : g_strset_form.load(); }

// p / len are the same in every lane of a wave in the wave forms
template <bool WAVE> __device__ inline uint64_t row_hash(const uint8_t *p, uint64_t len, uint64_t seed, int bits) {
    if constexpr (!WAVE) {
        return str::slot_key(str::hash(p, len, seed), bits);
    } else {
        const uint64_t sk = str::seed_key(seed), nw = (len + 7) >> 3;
        uint64_t sum = 0;
        for (uint64_t k = threadIdx.x & 63; k < nw; k += 64) sum += str::hash_term(str::load_word(p, len, k), k, sk);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t lo = __shfl_xor((uint32_t)sum, o, 64), hi = __shfl_xor((uint32_t)(sum >> 32), o, 64);
            sum += (uint64_t)hi << 32 | lo;
        }
        return str::slot_key(str::hash_finish(sum, len, sk), bits);
    }
}
template <bool WAVE> __device__ inline bool row_equal(const uint8_t *a, const uint8_t *b, uint64_t len) {
    if constexpr (!WAVE) {
        return str::equal(a, b, len);
    } else {
        const uint64_t nw = (len + 7) >> 3;
        bool diff = false;
        for (uint64_t k = threadIdx.x & 63; k < nw && !diff; k += 64) diff = str::load_word(a, len, k) != str::load_word(b, len, k);
        return __ballot(diff) == 0;
    }
}

// payload word of the slot holding key h, or SET_EMPTY when the table has no such key
__device__ inline uint64_t slot_find(const uint64_t *tab, uint64_t cap_mask, uint32_t max_probe, uint64_t h, uint64_t *pos_out = nullptr) {
    uint64_t pos = hash64(h) & cap_mask;
    for (uint32_t p = 0; p <= max_probe; p++) {
        const uint64_t k = tab[2 * pos];
        if (k == h) {
            if (pos_out) *pos_out = pos;
            return tab[2 * pos + 1];
        }
        if (k == SET_EMPTY) return SET_EMPTY;
        pos = (pos + 1) & cap_mask;
    }
    return SET_EMPTY;
}

// ---- offsets -----------------------------------------------------------------------------------
// bad |= 1: a negative offset, 2: a decreasing pair, 4: the last offset past the buffer
template <typename O> __global__ __launch_bounds__(256) void k_str_validate(const O *off, uint64_t n, uint64_t nbytes, uint32_t *bad) {
    uint32_t b = 0;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * 256) {
        const O o = off[i];
        if (o < 0) b |= 1;
        if (i < n && off[i + 1] < o) b |= 2;
        if (i == n && o >= 0 && (uint64_t)o > nbytes) b |= 4;
    }
    if (b) atomicOr(bad, b);
}

// ---- element-wise ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_str_len(StrCol c, uint64_t n, int kind, int64_t *out) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint8_t *p;
        uint64_t len;
        row_range(c, i, p, len);
        out[i] = (int64_t)(kind == str::LEN_CODEPOINTS ? str::count_codepoints(p, len) : len);
    }
}

// the pattern (<= 1024 bytes) is staged in LDS, zero-padded to whole words
__global__ __launch_bounds__(256) void k_str_match(StrCol c, uint64_t n, int op, const uint8_t *pat, uint32_t m, uint8_t *out) {
    __shared__ uint64_t s_pat[STR_MAX_PATTERN / 8 + 2];
    uint8_t *sp = reinterpret_cast<uint8_t *>(s_pat);
    for (uint32_t k = threadIdx.x; k < sizeof(s_pat); k += 256) sp[k] = k < m ? pat[k] : 0;
    __syncthreads();
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint8_t *p;
        uint64_t len;
        row_range(c, i, p, len);
        out[i] = str::match(op, p, len, sp, m) ? 1 : 0;
    }
}

// ---- take ---------------------------------------------------------------------------------------
// lens[j] = bytes of row idx[j] (an index outside [0, nsrc): 0, like vh_take), lens[m] = 0
template <typename I> __global__ __launch_bounds__(256) void k_take_len(StrCol c, uint64_t nsrc, const I *idx, uint64_t m, uint64_t *lens) {
    for (uint64_t j = blockIdx.x * 256ull + threadIdx.x; j <= m; j += (uint64_t)gridDim.x * 256) {
        uint64_t len = 0;
        if (j < m) {
            const int64_t r = (int64_t)idx[j];
            if (r >= 0 && (uint64_t)r < nsrc) len = (uint64_t)(col_off(c, r + 1) - col_off(c, r));
        }
        lens[j] = len;
    }
}
// the bytes of row idx[j] to out_bytes[base + pos[j] ..), and out offsets [first + j] = base + pos[j]
// (j <= m; written by the unit of row j, the last by the unit of row 0)
template <bool WAVE, typename I>
__global__ __launch_bounds__(256) void k_take_copy(StrCol c, uint64_t nsrc, const I *idx, uint64_t m, const uint64_t *pos,
                                                   uint64_t base, uint8_t *out_bytes, void *out_off, int out_wide, uint64_t first) {
    for (uint64_t j = unit_id<WAVE>(); j < m; j += unit_stride<WAVE>()) {
        const int64_t r = (int64_t)idx[j];
        const uint64_t at = base + pos[j];
        if (unit_leader<WAVE>()) {
            if (out_wide) static_cast<int64_t *>(out_off)[first + j] = (int64_t)at;
            else static_cast<int32_t *>(out_off)[first + j] = (int32_t)at;
            if (j == 0) {
                if (out_wide) static_cast<int64_t *>(out_off)[first + m] = (int64_t)(base + pos[m]);
                else static_cast<int32_t *>(out_off)[first + m] = (int32_t)(base + pos[m]);
            }
        }
        if (r < 0 || (uint64_t)r >= nsrc) continue;
        const uint8_t *p;
        uint64_t len;
        row_range(c, (uint64_t)r, p, len);
        if constexpr (WAVE) {
            for (uint64_t k = threadIdx.x & 63; k < len; k += 64) out_bytes[at + k] = p[k];
        } else {
            for (uint64_t k = 0; k < len; k++) out_bytes[at + k] = p[k];
        }
    }
}

using TakeScratch = LenScratch;
LenScratch &plan_scratch() {
    thread_local LenScratch scratch;
    return scratch;
}
// pos[0 .. m] = exclusive scan of the taken rows' lengths; returns the total
template <typename I>
static uint64_t take_plan(const StrCol &c, uint64_t nsrc, const I *idx, uint64_t m, uint64_t *pos, TakeScratch &s) {
    hipLaunchKernelGGL(k_take_len<I>, dim3(blocks_for(m + 1, 256)), dim3(256), 0, stream(), c, nsrc, idx, m, s.lengths(m));
    VH_HIP(hipGetLastError());
    return scan_lengths(s, m, pos);
}
template <typename I>
static void take_copy(const StrCol &c, uint64_t nsrc, const I *idx, uint64_t m, const uint64_t *pos, uint64_t total,
                      uint64_t base, uint8_t *out_bytes, void *out_off, int out_wide, uint64_t first) {
    if (!m) return;
    if (wave_form(total, m)) {
        hipLaunchKernelGGL((k_take_copy<true, I>), dim3(unit_blocks<true>(m)), dim3(256), 0, stream(), c, nsrc, idx, m, pos,
                           base, out_bytes, out_off, out_wide, first);
    } else {
        hipLaunchKernelGGL((k_take_copy<false, I>), dim3(unit_blocks<false>(m)), dim3(256), 0, stream(), c, nsrc, idx, m, pos,
                           base, out_bytes, out_off, out_wide, first);
    }
    VH_HIP(hipGetLastError());
}

// ---- the encoder --------------------------------------------------------------------------------
struct LevelsDev {
    const uint64_t *tab[STRSET_MAX_LEVELS];
    uint64_t mask[STRSET_MAX_LEVELS];
    uint32_t probe[STRSET_MAX_LEVELS];
    int n, bits;
    const int64_t *doff;
    const uint8_t *dbytes;
};

// round r, insert: every listed row claims (hash_r, ROWFLAG | row) in the level's table.
// ctr[0]: overflow (stops the pass), ctr[1]: new keys
template <bool WAVE>
__global__ __launch_bounds__(256) void k_ss_insert(StrCol c, const uint32_t *list, uint64_t m, uint64_t *tab, uint64_t cap_mask,
                                                   uint32_t max_probe, uint64_t seed, int bits, uint64_t *ctr) {
    __shared__ uint32_t wg_new;
    if (threadIdx.x == 0) wg_new = 0;
    __syncthreads();
    for (uint64_t j = unit_id<WAVE>(); j < m; j += unit_stride<WAVE>()) {
        if (__ballot(__hip_atomic_load(&ctr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) break;
        const uint64_t row = list ? list[j] : j;
        const uint8_t *p;
        uint64_t len;
        row_range(c, row, p, len);
        const uint64_t h = row_hash<WAVE>(p, len, seed, bits);
        if (unit_leader<WAVE>())
            set_claim(tab, cap_mask, max_probe, h, &wg_new, &ctr[0],
                      [&](uint64_t *pay) {
                          // the payload only falls: a row that cannot lower it skips the atomic (with few
                          // distinct strings nearly every row; same-address atomics serialise)
                          const uint64_t mine = ROWFLAG | row;
                          if (__hip_atomic_load(pay, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mine)
                              atomicMin((unsigned long long *)pay, (unsigned long long)mine);
                      });
    }
    __syncthreads();
    if (threadIdx.x == 0 && wg_new) atomicAdd((unsigned long long *)&ctr[1], (unsigned long long)wg_new);
}

// round r, verify: a listed row whose bytes equal its slot's string is resolved; the slot's own
// first row goes to reps (the new distinct strings), a row that differs to next (a collision).
// ctr[2]: rows in next, ctr[3]: rows in reps (running over the rounds of one update)
template <bool WAVE>
__global__ __launch_bounds__(256) void k_ss_verify(StrCol c, const uint32_t *list, uint64_t m, const uint64_t *tab,
                                                   uint64_t cap_mask, uint32_t max_probe, uint64_t seed, int bits,
                                                   const int64_t *doff, const uint8_t *dbytes, uint32_t *next, uint32_t *reps,
                                                   unsigned long long *ctr) {
    __shared__ uint32_t s_w[4];
    __shared__ unsigned long long s_base;
    constexpr uint64_t TILE = WAVE ? 4 : 256;
    const uint64_t u = WAVE ? threadIdx.x >> 6 : threadIdx.x;
    for (uint64_t t0 = blockIdx.x * TILE; t0 < m; t0 += (uint64_t)gridDim.x * TILE) {
        const uint64_t j = t0 + u;
        bool coll = false, rep = false;
        uint64_t row = 0;
        if (j < m) {
            row = list ? list[j] : j;
            const uint8_t *p;
            uint64_t len;
            row_range(c, row, p, len);
            const uint64_t h = row_hash<WAVE>(p, len, seed, bits);
            const uint64_t pay = slot_find(tab, cap_mask, max_probe, h);
            if (pay == SET_EMPTY) {
                coll = true;  // cannot happen after an insert pass that did not overflow
            } else if (pay & ROWFLAG) {
                const uint64_t r2 = pay & ~ROWFLAG;
                if (r2 == row) {
                    rep = true;
                } else {
                    const uint8_t *q;
                    uint64_t qlen;
                    row_range(c, r2, q, qlen);
                    coll = !(qlen == len && row_equal<WAVE>(p, q, len));
                }
            } else {
                const uint64_t qlen = (uint64_t)(doff[pay + 1] - doff[pay]);
                coll = !(qlen == len && row_equal<WAVE>(p, dbytes + doff[pay], len));
            }
        }
        const bool lead = unit_leader<WAVE>();
        const uint64_t a = block_reserve<256>((lead && coll) ? 1u : 0u, s_w, &s_base, &ctr[2]);
        if (lead && coll) next[a] = (uint32_t)row;
        const uint64_t b = block_reserve<256>((lead && rep) ? 1u : 0u, s_w, &s_base, &ctr[3]);
        if (lead && rep) reps[b] = (uint32_t)row;
    }
}

// after the rounds: the slot of the j-th new string (first row rows[j], ascending) gets its
// dictionary index first + j
__global__ __launch_bounds__(256) void k_ss_assign(StrCol c, const uint32_t *rows, uint64_t m, LevelsDev L, uint64_t first) {
    for (uint64_t j = blockIdx.x * 256ull + threadIdx.x; j < m; j += (uint64_t)gridDim.x * 256) {
        const uint64_t row = rows[j];
        const uint8_t *p;
        uint64_t len;
        row_range(c, row, p, len);
        for (int r = 0; r < L.n; r++) {
            const uint64_t h = row_hash<false>(p, len, (uint64_t)r, L.bits);
            uint64_t pos = 0;
            const uint64_t pay = slot_find(L.tab[r], L.mask[r], L.probe[r], h, &pos);
            if (pay == (ROWFLAG | row)) {
                const_cast<uint64_t *>(L.tab[r])[2 * pos + 1] = first + j;
                break;
            }
            if (pay == SET_EMPTY) break;
        }
    }
}

// ordinal of every row (int32), -1 for a string the set does not hold
template <bool WAVE> __global__ __launch_bounds__(256) void k_ss_map(StrCol c, uint64_t n, LevelsDev L, int32_t *out) {
    for (uint64_t i = unit_id<WAVE>(); i < n; i += unit_stride<WAVE>()) {
        const uint8_t *p;
        uint64_t len;
        row_range(c, i, p, len);
        int32_t code = -1;
        for (int r = 0; r < L.n; r++) {
            const uint64_t h = row_hash<WAVE>(p, len, (uint64_t)r, L.bits);
            const uint64_t pay = slot_find(L.tab[r], L.mask[r], L.probe[r], h);
            if (pay == SET_EMPTY || (pay & ROWFLAG)) break;
            const uint64_t qlen = (uint64_t)(L.doff[pay + 1] - L.doff[pay]);
            if (qlen == len && row_equal<WAVE>(p, L.dbytes + L.doff[pay], len)) {
                code = (int32_t)pay;
                break;
            }
        }
        if (unit_leader<WAVE>()) out[i] = code;
    }
}

}  // namespace vh

using namespace vh;

struct vh_strset {
    struct Level {
        DevBuf tab;
        uint64_t cap = 0, count = 0;
    };
    int bits = 64;
    uint64_t initial_capacity = 0;
    std::deque<Level> levels;  // a DevBuf does not move
    DevBuf doff, dbytes;  // the dictionary: count + 1 int64 offsets, bytes (+ slack)
    uint64_t count = 0, dict_bytes = 0;
    bool broken = false;  // an update failed half way: slots may name rows of a column that is gone
    DevBuf ctr, list[2], reps, sorted, tmp;
    TakeScratch take;
    DevBuf pos;
};

namespace vh {

static LevelsDev levels_view(const vh_strset *s) {
    LevelsDev L{};
    L.n = (int)s->levels.size();
    L.bits = s->bits;
    for (int r = 0; r < L.n; r++) {
        L.tab[r] = s->levels[r].tab.as<uint64_t>();
        L.mask[r] = s->levels[r].cap - 1;
        L.probe[r] = slots_max_probe(s->levels[r].cap);
    }
    L.doff = s->doff.as<int64_t>();
    L.dbytes = s->dbytes.as<uint8_t>();
    return L;
}

// `buf` holds at least `need` bytes and keeps its first `keep` bytes
static void grow_keep(DevBuf &buf, uint64_t need, uint64_t keep) {
    if (need <= buf.bytes) return;
    DevBuf nb;
    nb.ensure(std::max(need, buf.bytes * 2));
    if (keep) VH_HIP(hipMemcpyAsync(nb.ptr, buf.ptr, keep, hipMemcpyDeviceToDevice, stream()));
    VH_HIP(hipStreamSynchronize(stream()));
    buf.swap(nb);
}

template <bool WAVE> static void strset_update(vh_strset *s, const StrCol &c, uint64_t n) {
    hipStream_t st = stream();
    s->ctr.ensure(4 * 8);
    uint64_t *ctr = s->ctr.as<uint64_t>();
    VH_HIP(hipMemsetAsync(ctr, 0, 32, st));
    s->reps.ensure(n * 4);
    const uint32_t *list = nullptr;
    uint64_t m = n, rounds = 0, nreps = 0;
    for (int r = 0; m > 0; r++) {
        if (r >= STRSET_MAX_LEVELS) fail(VH_ERR_RUNTIME, "string set: more than 64 collision levels");
        if ((int)s->levels.size() <= r) {
            s->levels.emplace_back();
            const uint64_t cap0 = s->initial_capacity ? s->initial_capacity : (r == 0 ? (1ull << 16) : (1ull << 10));
            slots_grow(s->levels[r].tab, s->levels[r].cap, std::max<uint64_t>(64, next_pow2(cap0)));
        }
        vh_strset::Level &lv = s->levels[r];
        for (;;) {
            VH_HIP(hipMemsetAsync(ctr, 0, 16, st));
            hipLaunchKernelGGL(k_ss_insert<WAVE>, dim3(unit_blocks<WAVE>(m)), dim3(256), 0, st, c, list, m, lv.tab.as<uint64_t>(),
                               lv.cap - 1, slots_max_probe(lv.cap), (uint64_t)r, s->bits, ctr);
            VH_HIP(hipGetLastError());
            const std::vector<uint64_t> v = slots_read_ctr(s->ctr, 2);
            lv.count += v[1];
            if (v[0]) {  // a probe sequence ran out: a larger table, and the rows again (claims are idempotent)
                slots_grow(lv.tab, lv.cap, lv.cap * 4);
                continue;
            }
            while (lv.count * 2 > lv.cap) slots_grow(lv.tab, lv.cap, lv.cap * 4);
            break;
        }
        DevBuf &next = s->list[r & 1];
        next.ensure(m * 4);
        VH_HIP(hipMemsetAsync(ctr + 2, 0, 8, st));
        hipLaunchKernelGGL(k_ss_verify<WAVE>, dim3(unit_blocks<WAVE>(m)), dim3(256), 0, st, c, list, m, lv.tab.as<uint64_t>(),
                           lv.cap - 1, slots_max_probe(lv.cap), (uint64_t)r, s->bits, s->doff.as<int64_t>(),
                           s->dbytes.as<uint8_t>(), next.as<uint32_t>(), s->reps.as<uint32_t>(),
                           reinterpret_cast<unsigned long long *>(ctr));
        VH_HIP(hipGetLastError());
        const std::vector<uint64_t> v = slots_read_ctr(s->ctr, 4);
        // a level this update created resolves at least its slots' first rows; a level from an
        // earlier update may resolve none (every row differs from the strings it holds): the
        // level count bounds the loop
        m = v[2];
        nreps = v[3];
        list = next.as<uint32_t>();
        rounds++;
    }
    uint64_t prev = g_strset_rounds.load();
    while (prev < rounds && !g_strset_rounds.compare_exchange_weak(prev, rounds)) {}
    if (!nreps) return;
    if (s->count + nreps >= (1ull << 31)) fail(VH_ERR_RUNTIME, "string set: more than 2^31 distinct strings");
    // the new strings in the order of their first rows: their ordinals
    s->sorted.ensure(nreps * 4);
    size_t tb = 0;
    VH_HIP(rocprim::radix_sort_keys(nullptr, tb, s->reps.as<uint32_t>(), s->sorted.as<uint32_t>(), (size_t)nreps, 0, 32, st));
    s->tmp.ensure(tb ? tb : 8);
    VH_HIP(rocprim::radix_sort_keys(s->tmp.ptr, tb, s->reps.as<uint32_t>(), s->sorted.as<uint32_t>(), (size_t)nreps, 0, 32, st));
    // their bytes into the dictionary
    s->pos.ensure((nreps + 1) * 8);
    const uint64_t total = take_plan(c, n, s->sorted.as<uint32_t>(), nreps, s->pos.as<uint64_t>(), s->take);
    grow_keep(s->doff, (s->count + nreps + 1) * 8, s->count ? (s->count + 1) * 8 : 0);
    grow_keep(s->dbytes, s->dict_bytes + total + 16, s->dict_bytes);
    take_copy(c, n, s->sorted.as<uint32_t>(), nreps, s->pos.as<uint64_t>(), total, s->dict_bytes, s->dbytes.as<uint8_t>(),
              s->doff.ptr, 1, s->count);
    hipLaunchKernelGGL(k_ss_assign, dim3(blocks_for(nreps, 256)), dim3(256), 0, st, c, s->sorted.as<uint32_t>(), nreps,
                       levels_view(s), s->count);
    VH_HIP(hipGetLastError());
    VH_HIP(hipStreamSynchronize(st));
    s->count += nreps;
    s->dict_bytes += total;
}

}  // namespace vh

extern "C" {

int vh_str_validate(const void *offsets, int off_itemsize, uint64_t n, uint64_t nbytes, int *bad) {
    VH_API_BEGIN
    make_col(offsets, off_itemsize, nullptr);
    thread_local DevBuf flag;
    flag.ensure(8);
    hipStream_t st = stream();
    VH_HIP(hipMemsetAsync(flag.ptr, 0, 8, st));
    if (off_itemsize == 8)
        hipLaunchKernelGGL(k_str_validate<int64_t>, dim3(blocks_for(n + 1, 256)), dim3(256), 0, st,
                           static_cast<const int64_t *>(offsets), n, nbytes, flag.as<uint32_t>());
    else
        hipLaunchKernelGGL(k_str_validate<int32_t>, dim3(blocks_for(n + 1, 256)), dim3(256), 0, st,
                           static_cast<const int32_t *>(offsets), n, nbytes, flag.as<uint32_t>());
    VH_HIP(hipGetLastError());
    uint32_t b = 0;
    VH_HIP(hipMemcpyAsync(&b, flag.ptr, 4, hipMemcpyDeviceToHost, st));
    VH_HIP(hipStreamSynchronize(st));
    *bad = (int)b;
    VH_API_END
}

int vh_str_len(const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n, int kind, int64_t *out) {
    VH_API_BEGIN
    const StrCol c = make_col(offsets, off_itemsize, bytes);
    if (kind != str::LEN_BYTES && kind != str::LEN_CODEPOINTS) fail(VH_ERR_ARG, "vh_str_len: unknown kind");
    if (!n) return VH_OK;
    TimedScope ts("str_len");
    hipLaunchKernelGGL(k_str_len, dim3(blocks_for(n, 256, 16)), dim3(256), 0, stream(), c, n, kind, out);
    VH_HIP(hipGetLastError());
    VH_API_END
}

int vh_str_match(const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n, int op, const uint8_t *pattern,
                 uint64_t pattern_len, uint8_t *out) {
    VH_API_BEGIN
    const StrCol c = make_col(offsets, off_itemsize, bytes);
    if (op < 0 || op >= str::N_MATCH_OPS) fail(VH_ERR_ARG, "vh_str_match: unknown op");
    if (pattern_len > (uint64_t)STR_MAX_PATTERN) fail(VH_ERR_ARG, "vh_str_match: a pattern holds at most 1024 bytes");
    if (!n) return VH_OK;
    thread_local DevBuf pat;
    pat.ensure(STR_MAX_PATTERN);
    hipStream_t st = stream();
    if (pattern_len) {
        VH_HIP(hipMemcpyAsync(pat.ptr, pattern, pattern_len, hipMemcpyHostToDevice, st));
        VH_HIP(hipStreamSynchronize(st));  // the caller's pattern buffer may go after the call
    }
    TimedScope ts("str_match");
    hipLaunchKernelGGL(k_str_match, dim3(blocks_for(n, 256, 16)), dim3(256), 0, st, c, n, op, pat.as<uint8_t>(),
                       (uint32_t)pattern_len, out);
    VH_HIP(hipGetLastError());
    VH_API_END
}

int vh_str_take_plan(const void *offsets, int off_itemsize, uint64_t n, const void *indices, int idx_itemsize, uint64_t m,
                     uint64_t *pos, uint64_t *total) {
    VH_API_BEGIN
    const StrCol c = make_col(offsets, off_itemsize, nullptr);
    TakeScratch &scratch = plan_scratch();
    if (idx_itemsize == 8) *total = take_plan(c, n, static_cast<const int64_t *>(indices), m, pos, scratch);
    else if (idx_itemsize == 4) *total = take_plan(c, n, static_cast<const int32_t *>(indices), m, pos, scratch);
    else fail(VH_ERR_ARG, "vh_str_take_plan: indices are int32 or int64");
    VH_API_END
}

int vh_str_take(const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n, const void *indices,
                int idx_itemsize, uint64_t m, const uint64_t *pos, uint64_t total, void *out_offsets, int out_itemsize,
                uint8_t *out_bytes) {
    VH_API_BEGIN
    const StrCol c = make_col(offsets, off_itemsize, bytes);
    if (out_itemsize != 4 && out_itemsize != 8) fail(VH_ERR_ARG, "vh_str_take: output offsets are int32 or int64");
    if (out_itemsize == 4 && str::take_needs_wide(false, total)) fail(VH_ERR_ARG, "vh_str_take: int32 offsets overflow");
    if (!m) {
        VH_HIP(hipMemsetAsync(out_offsets, 0, out_itemsize, stream()));
        return VH_OK;
    }
    TimedScope ts("str_take");
    if (idx_itemsize == 8)
        take_copy(c, n, static_cast<const int64_t *>(indices), m, pos, total, 0, out_bytes, out_offsets, out_itemsize == 8, 0);
    else if (idx_itemsize == 4)
        take_copy(c, n, static_cast<const int32_t *>(indices), m, pos, total, 0, out_bytes, out_offsets, out_itemsize == 8, 0);
    else fail(VH_ERR_ARG, "vh_str_take: indices are int32 or int64");
    VH_API_END
}

int vh_strset_create(int hash_bits, uint64_t initial_capacity, void **out) {
    VH_API_BEGIN
    if (hash_bits < 0 || hash_bits > 64) fail(VH_ERR_ARG, "vh_strset_create: hash_bits is 0 .. 64");
    vh_strset *s = new vh_strset;
    s->bits = hash_bits;
    s->initial_capacity = initial_capacity;
    *out = s;
    VH_API_END
}

int vh_strset_destroy(void *set) {
    VH_API_BEGIN
    delete static_cast<vh_strset *>(set);
    VH_API_END
}

int vh_strset_update(void *set, const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n) {
    VH_API_BEGIN
    vh_strset *s = static_cast<vh_strset *>(set);
    const StrCol c = make_col(offsets, off_itemsize, bytes);
    if (n >= (1ull << 32)) fail(VH_ERR_ARG, "vh_strset_update: at most 2^32 - 1 rows per call");
    if (!n) return VH_OK;
    if (s->broken) fail(VH_ERR_RUNTIME, "string set: an earlier update failed; the set cannot be used");
    TimedScope ts("strset_update");
    const bool wave = wave_form(col_span(c, n), n);
    g_strset_form.store(wave ? 1 : 0);
    s->broken = true;
    if (wave) strset_update<true>(s, c, n);
    else strset_update<false>(s, c, n);
    s->broken = false;
    VH_API_END
}

int vh_strset_info(void *set, int64_t *count, int64_t *dict_bytes, int64_t *levels, int64_t *table_bytes) {
    VH_API_BEGIN
    const vh_strset *s = static_cast<const vh_strset *>(set);
    *count = (int64_t)s->count;
    *dict_bytes = (int64_t)s->dict_bytes;
    *levels = (int64_t)s->levels.size();
    uint64_t tb = 0;
    for (const auto &lv : s->levels) tb += lv.cap * 16;
    *table_bytes = (int64_t)tb;
    VH_API_END
}

int vh_strset_dict(void *set, int64_t *offsets_out, uint8_t *bytes_out) {
    VH_API_BEGIN
    const vh_strset *s = static_cast<const vh_strset *>(set);
    hipStream_t st = stream();
    if (s->count) {
        VH_HIP(hipMemcpyAsync(offsets_out, s->doff.ptr, (s->count + 1) * 8, hipMemcpyDeviceToHost, st));
        if (s->dict_bytes) VH_HIP(hipMemcpyAsync(bytes_out, s->dbytes.ptr, s->dict_bytes, hipMemcpyDeviceToHost, st));
        VH_HIP(hipStreamSynchronize(st));
    } else {
        offsets_out[0] = 0;
    }
    VH_API_END
}

int vh_strset_map_ordinal(void *set, const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n, int32_t *out) {
    VH_API_BEGIN
    const vh_strset *s = static_cast<const vh_strset *>(set);
    const StrCol c = make_col(offsets, off_itemsize, bytes);
    if (s->broken) fail(VH_ERR_RUNTIME, "string set: an earlier update failed; the set cannot be used");
    if (!n) return VH_OK;
    TimedScope ts("strset_map");
    const bool wave = wave_form(col_span(c, n), n);
    g_strset_form.store(wave ? 1 : 0);
    const LevelsDev L = levels_view(s);
    if (wave) hipLaunchKernelGGL(k_ss_map<true>, dim3(unit_blocks<true>(n)), dim3(256), 0, stream(), c, n, L, out);
    else hipLaunchKernelGGL(k_ss_map<false>, dim3(unit_blocks<false>(n)), dim3(256), 0, stream(), c, n, L, out);
    VH_HIP(hipGetLastError());
    VH_API_END
}

}  // extern "C"
