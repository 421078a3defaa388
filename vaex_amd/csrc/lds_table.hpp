// The LDS key table shared by the hash engines (hashagg.hip, hashset.hip; counter.hip takes
// the primitives only): key-bits types, the LDS hash and CAS, and the two-choice table's
// find / insert / add_many, written once over a small table type.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace vh {

// key bits: uint32_t for keys of <= 4 bytes, uint64_t for 8-byte keys.  The all-ones pattern
// marks an EMPTY LDS slot; keys whose bits are the top two patterns live in side records
template <typename K> using kb_t = std::conditional_t<sizeof(K) == 8, uint64_t, uint32_t>;
template <typename KB> __host__ __device__ constexpr KB kb_empty() { return ~KB(0); }
template <typename KB> __host__ __device__ constexpr KB kb_closed() { return ~KB(0) - 1; }

// murmur3 finaliser
__host__ __device__ inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// LDS slot hash of 64 key bits: a 32-bit mixer, cheaper than hash64's 64-bit multiplies and
// independent of the bucket bits (which come from hash64)
__device__ inline uint32_t lds_hash(uint64_t kb) { return fmix32((uint32_t)kb ^ (uint32_t)(kb >> 32) * 0x9e3779b9u); }

__device__ inline uint32_t lds_cas(uint32_t *p, uint32_t cmp, uint32_t val) { return atomicCAS(p, cmp, val); }
__device__ inline uint64_t lds_cas(uint64_t *p, uint64_t cmp, uint64_t val) {
    return atomicCAS(reinterpret_cast<unsigned long long *>(p), (unsigned long long)cmp, (unsigned long long)val);
}

// workgroup barrier that waits for LDS traffic only (global stores stay in flight)
__device__ inline void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// four consecutive key slots: one ds_read_b128 (4-byte keys) or two (8-byte keys)
template <typename KB> struct alignas(16) KB4 {
    KB v[4];
};

// Two-choice LDS table: a key lives in one of two 4-slot groups, g1 from its hash and g2 from
// a second mix of it, both read at once, so a lookup almost never needs a second round trip:
// with ~2300 keys in 1024 groups the less loaded of two groups is rarely full (one-group
// linear probing displaced ~5 % of the keys, and the lanes holding them serialised every
// wave: 4.6 of hashagg's 7.3 ms pass B, VH_HA_DEBUG ablation).  A new key is CASed into the
// first EMPTY slot of the group with more room; two lanes that insert one key at once may
// place it in both groups -- harmless, both records merge into the key's one HBM slot.  A key
// whose groups are both full goes straight to the HBM table; keys whose bits are EMPTY /
// CLOSED live in the two side records after the slots.
//
// A table type Tab supplies
//   Tab::KB, Tab::SLOTS      key bits type, slot count (side records are SLOTS, SLOTS + 1)
//   t.keys()                 KB[SLOTS], 16-byte aligned
//   t.groups(kb, g1, g2)     the key's two groups
//   t.hit(slot, payload)     fold a row's payload into a slot that holds its key
//   t.spill(kb, payload)     the row straight into the HBM table
template <typename KB> __device__ inline uint32_t lt2_find(const KB4<KB> &q1, const KB4<KB> &q2, uint32_t g1, uint32_t g2,
                                                         KB kb) {
    uint32_t slot = ~0u;
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        if (q2.v[j] == kb) slot = 4 * g2 + j;
        if (q1.v[j] == kb) slot = 4 * g1 + j;
    }
    return slot;
}

// a key not found in either group: insert it (or find it, if another lane just did)
template <typename Tab, typename Payload> __device__ inline void lt2_insert(const Tab &t, typename Tab::KB kb, const Payload &pl) {
    using KB = typename Tab::KB;
    constexpr KB EMPTY = kb_empty<KB>();
    KB *keys = t.keys();
    uint32_t g1, g2;
    t.groups(kb, g1, g2);
    for (int it = 0; it < 64; it++) {
        const KB4<KB> q1 = *reinterpret_cast<const KB4<KB> *>(keys + 4 * g1);
        const KB4<KB> q2 = *reinterpret_cast<const KB4<KB> *>(keys + 4 * g2);
        const uint32_t hit = lt2_find(q1, q2, g1, g2, kb);
        if (hit != ~0u) {
            t.hit(hit, pl);
            return;
        }
        int e1 = 0, e2 = 0, f1 = -1, f2 = -1;
#pragma unroll
        for (int j = 3; j >= 0; j--) {
            if (q1.v[j] == EMPTY) {
                e1++;
                f1 = j;
            }
            if (q2.v[j] == EMPTY) {
                e2++;
                f2 = j;
            }
        }
        if (e1 == 0 && e2 == 0) break;
        const uint32_t pos = e1 >= e2 ? 4 * g1 + f1 : 4 * g2 + f2;
        const KB cur = lds_cas(&keys[pos], EMPTY, kb);
        if (cur == EMPTY || cur == kb) {
            t.hit(pos, pl);
            return;
        }
        // another key took the slot: read the groups again
    }
    t.spill(kb, pl);
}

// M entries at once: both group reads of every entry are issued before any is used and the
// hits folded with fire-and-forget LDS atomics; only keys new to the table take lt2_insert.
// pl[i] is entry i's payload.
template <int M, typename Tab, typename Payloads>
__device__ inline void lt2_add_many(const Tab &t, const typename Tab::KB *kb, const Payloads &pl, const bool *valid) {
    using KB = typename Tab::KB;
    const KB *keys = t.keys();
    KB4<KB> q1[M], q2[M];
    uint32_t g1[M], g2[M];
#pragma unroll
    for (int i = 0; i < M; i++) {
        t.groups(kb[i], g1[i], g2[i]);
        q1[i] = *reinterpret_cast<const KB4<KB> *>(keys + 4 * g1[i]);
        q2[i] = *reinterpret_cast<const KB4<KB> *>(keys + 4 * g2[i]);
    }
    bool slow[M];
#pragma unroll
    for (int i = 0; i < M; i++) {
        uint32_t slot = lt2_find(q1[i], q2[i], g1[i], g2[i], kb[i]);
        if (kb[i] >= kb_closed<KB>()) slot = Tab::SLOTS + (uint32_t)(kb[i] - kb_closed<KB>());
        slow[i] = valid[i] && slot == ~0u;
        if (valid[i] && slot != ~0u) t.hit(slot, pl[i]);
    }
#pragma unroll
    for (int i = 0; i < M; i++)
        if (slow[i]) lt2_insert(t, kb[i], pl[i]);
}

}  // namespace vh
