// The open-address hash table in HBM, device side: hash64, key_bits, the slot claim of a 16-byte
// {key, payload} table (set_claim: hashset.hip's ordered_set, counter.hip's hash counter,
// index.hip's join index; hashagg.hip's struct-of-arrays table has a claim of its own), the key
// sample of hashagg.hip, hashset.hip and counter.hip, and the sealed lookup table (SetDev) that
// hashset.hip and index.hip build and that the fused set-ordinal binner of binning.hip, the
// tile path (tiled.hip), hashagg.hip's set rank and index.hip's probe read.  The table's host
// side (fresh table, growth, compaction, counter words, host staging) is slot_table.hpp, the
// engines' LDS table lds_table.hpp, their host plan hash_plan.hpp.
//
// Layout in HBM: `tab[cap]` of 16-byte slots {key bits zero-extended (EMPTY = ~0),
// first row the key was seen at (the ordinal order)}, so an insert probe and its
// first-row update touch one cache line; after sealing, a lookup table (below).
// Linear probing from _hash64(bits) (the reference's splitmix64 finaliser,
// hash.hpp:25-30).
// 64-bit integer keys whose bits equal EMPTY (int64 -1, uint64 max) live in a
// side slot ("special").  NaN and null keys get their own ordinals like the
// reference's nan_value/null_value (hash_primitives.hpp:436-450).
#pragma once
#include "common.hpp"
#include "hash_plan.hpp"

namespace vh {

constexpr uint64_t SET_EMPTY = ~0ULL;
constexpr int SET_MAX_PROBE = 256;

__host__ __device__ inline uint64_t hash64(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

template <typename T> __device__ inline uint64_t key_bits(T v) {
    if constexpr (sizeof(T) == 8) {
        uint64_t u;
        __builtin_memcpy(&u, &v, 8);
        return u;
    } else if constexpr (sizeof(T) == 4) {
        uint32_t u;
        __builtin_memcpy(&u, &v, 4);
        return u;
    } else if constexpr (sizeof(T) == 2) {
        uint16_t u;
        __builtin_memcpy(&u, &v, 2);
        return u;
    } else {
        uint8_t u;
        __builtin_memcpy(&u, &v, 1);
        return u;
    }
}

// Claim the 16-byte {key, payload} slot of `kb` in an open-address HBM table `tab` (CAS on an
// EMPTY key word, linear probing over at most max_probe + 1 slots) and call fold(payload word)
// on it: the caller's atomicMin of a row or atomicAdd of a count.  A probe sequence that runs
// out raises *overflow instead (the host grows the table and runs the chunk again).  New keys
// are counted per workgroup in LDS (`wg_new`): one global counter bumped by every new key
// serialises.
template <typename Probe, typename Fold>
__device__ inline void set_claim(uint64_t *tab, uint64_t cap_mask, Probe max_probe, uint64_t kb, uint32_t *wg_new,
                                 uint64_t *overflow, Fold &&fold) {
    uint64_t pos = hash64(kb) & cap_mask;
    for (Probe p = 0; p <= max_probe; p++) {
        const uint64_t k = __hip_atomic_load(&tab[2 * pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool mine = k == kb;
        if (!mine && k == SET_EMPTY) {
            const uint64_t old = atomicCAS((unsigned long long *)&tab[2 * pos], (unsigned long long)SET_EMPTY,
                                           (unsigned long long)kb);
            if (old == SET_EMPTY) atomicAdd(wg_new, 1u);
            mine = old == SET_EMPTY || old == kb;
        }
        if (mine) {
            fold(&tab[2 * pos + 1]);
            return;
        }
        pos = (pos + 1) & cap_mask;
    }
    atomicOr((unsigned long long *)overflow, 1ULL);
}

// ---- the key sample of the hash engines (hashagg.hip, hashset.hip, counter.hip) -----------
// one sampled key into the sample's HBM table: keys[smask + 1] (EMPTY = free) with a count of
// its occurrences per slot; a key that finds no slot within the probe limit is not counted
constexpr int SAMPLE_MAX_PROBE = 1 << 14;
__device__ inline void sample_insert(uint64_t *skeys, uint32_t *scnt, uint64_t smask, uint64_t key) {
    uint64_t pos = hash64(key) & smask;
#pragma nounroll
    for (int p = 0; p < SAMPLE_MAX_PROBE; p++) {
        uint64_t cur = __hip_atomic_load(&skeys[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == SET_EMPTY)
            cur = atomicCAS((unsigned long long *)&skeys[pos], (unsigned long long)SET_EMPTY, (unsigned long long)key);
        if (cur == SET_EMPTY || cur == key) {
            atomicAdd(&scnt[pos], 1u);
            break;
        }
        pos = (pos + 1) & smask;
    }
}

// the sample buffer (hash_sample_layout) ready for a sample on `st`: keys EMPTY, the rest zero
struct SampleBuf {
    uint64_t *skeys;
    uint32_t *scnt;
    unsigned long long *fine, *stats;
};
inline SampleBuf sample_reset(DevBuf &buf, hipStream_t st) {
    const HashSampleLayout sl = hash_sample_layout();
    buf.ensure(sl.bytes);
    unsigned char *b = buf.as<unsigned char>();
    VH_HIP(hipMemsetAsync(b + sl.skeys, 0xff, sl.scnt - sl.skeys, st));
    VH_HIP(hipMemsetAsync(b + sl.scnt, 0, sl.bytes - sl.scnt, st));
    return {reinterpret_cast<uint64_t *>(b + sl.skeys), reinterpret_cast<uint32_t *>(b + sl.scnt),
            reinterpret_cast<unsigned long long *>(b + sl.fine), reinterpret_cast<unsigned long long *>(b + sl.stats)};
}

// occurrence counts of a sample table's slots (0 = free slot), as k_sample_stats reads them
struct SampleCounts {  // a count array next to the keys
    const uint32_t *cnt;
    __device__ uint64_t operator()(uint64_t i) const { return cnt[i]; }
};
struct SampleSlotCounts {  // 16-byte {key, count} slots
    const uint64_t *tab;
    __device__ uint64_t operator()(uint64_t i) const {
        const ulonglong2 e = reinterpret_cast<const ulonglong2 *>(tab)[i];
        return e.x == SET_EMPTY ? 0 : e.y;
    }
};

// distinct keys of the sample, and how many were seen once / twice (Chao1 inputs), added to
// stats[0..2]
template <typename Counts>
__global__ __launch_bounds__(256) void k_sample_stats(Counts counts, uint64_t slots, unsigned long long *stats) {
    __shared__ uint32_t part[3][4];
    uint32_t d = 0, f1 = 0, f2 = 0;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * 256) {
        const uint64_t c = counts(i);
        d += c != 0;
        f1 += c == 1;
        f2 += c == 2;
    }
    for (int off = 32; off > 0; off >>= 1) {
        d += __shfl_down(d, off, 64);
        f1 += __shfl_down(f1, off, 64);
        f2 += __shfl_down(f2, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {  // one atomic per block and counter, not per wave
        part[0][threadIdx.x >> 6] = d;
        part[1][threadIdx.x >> 6] = f1;
        part[2][threadIdx.x >> 6] = f2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t v = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        if (v) atomicAdd(&stats[threadIdx.x], (unsigned long long)v);
    }
}

// Lookup table built when the set is sealed: one 8-byte slot (ordinal << 32 | key bits)
// for keys of <= 4 bytes, one 16-byte slot {key bits, ordinal} for 8-byte keys, so a
// probe touches one cache line; EMPTY slots are all ones.
struct SetDev {
    const uint64_t *lut;
    int wide;             // 0: packed 8-byte slots, 1: {key, ord} 16-byte slots
    uint64_t cap_mask;
    int64_t nan_ord;      // ordinal of NaN (0x7fffffff when absent, as the reference)
    int64_t null_ord;     // ordinal of null / masked keys (-1 when absent)
    int64_t special_ord;  // ordinal of the EMPTY-bits key, -1 when absent
};

// ordinal of a key, -1 if unknown (hash_primitives.hpp:567-580)
__device__ inline int64_t set_lookup_bits(const SetDev &s, uint64_t kb) {
    if (kb == SET_EMPTY) return s.special_ord;
    uint64_t pos = hash64(kb) & s.cap_mask;
    if (!s.wide) {
        for (int p = 0; p <= SET_MAX_PROBE; p++) {
            const uint64_t e = s.lut[pos];
            if (e == SET_EMPTY) return -1;
            if ((uint32_t)e == (uint32_t)kb) return (int64_t)(e >> 32);
            pos = (pos + 1) & s.cap_mask;
        }
    } else {
        for (int p = 0; p <= SET_MAX_PROBE; p++) {
            const ulonglong2 e = reinterpret_cast<const ulonglong2 *>(s.lut)[pos];
            if (e.x == kb) return (int64_t)e.y;
            if (e.x == SET_EMPTY) return -1;
            pos = (pos + 1) & s.cap_mask;
        }
    }
    return -1;
}

template <typename T> __device__ inline int64_t set_lookup(const SetDev &s, T v) {
    if (is_nan_v(v)) return s.nan_ord;
    return set_lookup_bits(s, key_bits(v));
}

}  // namespace vh

// host-side view used by binning.hip to build a SetDev for a binner
struct vh_set;
namespace vh {
SetDev set_device_view(vh_set *set);  // seals the set if needed
int set_dtype(const vh_set *set);
}  // namespace vh
