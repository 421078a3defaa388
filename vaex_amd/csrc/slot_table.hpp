// The HBM slot table of hashset.hip (ordered_set), counter.hip (the hash counter) and
// index.hip (the join index), host side: `tab[cap]` of 16-byte slots {key bits zero-extended
// (EMPTY = ~0), payload}, cap a power of two, linear probing from hash64(bits); the device
// side (set_claim, the layout's rationale) is hashset.hpp.  The payload is a first row (set,
// index: folded with atomicMin, so a free slot holds all ones) or a count (counter: folded
// with atomicAdd, so a free slot holds 0).  Here: a fresh table, growth by rehash, the
// compaction of the occupied slots, the read-back of an engine's counter words, and the
// staging of host columns that the three engines' entry points share.
#pragma once
#include <algorithm>

#include "common.hpp"
#include "hashset.hpp"

namespace vh {

// probes past the home slot that an insert or a find may take
inline uint32_t slots_max_probe(uint64_t cap) { return (uint32_t)std::min<uint64_t>(cap - 1, SET_MAX_PROBE); }

enum class SlotPayload { ONES, ZERO };  // a free slot's payload word

static __global__ __launch_bounds__(256) void k_slots_clear(uint64_t *tab, uint64_t cap) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * 256)
        reinterpret_cast<ulonglong2 *>(tab)[i] = make_ulonglong2(SET_EMPTY, 0);
}

// `tab` holds `cap` free slots (on the library stream; the buffer is kept when large enough)
inline void slots_fresh(DevBuf &tab, uint64_t cap, SlotPayload payload) {
    tab.ensure(cap * 16);
    if (payload == SlotPayload::ONES) {
        VH_HIP(hipMemsetAsync(tab.ptr, 0xff, cap * 16, stream()));
    } else {
        hipLaunchKernelGGL(k_slots_clear, dim3(blocks_for(cap, 256)), dim3(256), 0, stream(), tab.as<uint64_t>(), cap);
        VH_HIP(hipGetLastError());
    }
}

// every occupied slot of the old table into the new, larger one with its payload (unbounded
// probing: the new table has room for every key)
static __global__ __launch_bounds__(256) void k_slots_rehash(const uint64_t *otab, uint64_t ocap, uint64_t *ntab,
                                                             uint64_t ncap_mask) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < ocap; i += (uint64_t)gridDim.x * 256) {
        const ulonglong2 e = reinterpret_cast<const ulonglong2 *>(otab)[i];
        if (e.x == SET_EMPTY) continue;
        uint64_t pos = hash64(e.x) & ncap_mask;
        for (;;) {
            const uint64_t old = atomicCAS((unsigned long long *)&ntab[2 * pos], (unsigned long long)SET_EMPTY,
                                           (unsigned long long)e.x);
            if (old == SET_EMPTY) break;
            pos = (pos + 1) & ncap_mask;
        }
        ntab[2 * pos + 1] = e.y;
    }
}

// the table becomes one of new_cap slots holding what it held (cap == 0: a first, free table).
// The new table is allocated before anything changes, and the stream is drained before the
// old one is freed.
inline void slots_grow(DevBuf &tab, uint64_t &cap, uint64_t new_cap, SlotPayload payload = SlotPayload::ONES) {
    DevBuf nt;
    slots_fresh(nt, new_cap, payload);
    if (cap) {
        hipLaunchKernelGGL(k_slots_rehash, dim3(blocks_for(cap, 256)), dim3(256), 0, stream(), tab.as<uint64_t>(), cap,
                           nt.as<uint64_t>(), new_cap - 1);
        VH_HIP(hipGetLastError());
    }
    VH_HIP(hipStreamSynchronize(stream()));
    tab.swap(nt);
    cap = new_cap;
}

// The occupied slots, compacted: emit(j, i, key bits, payload) for the j-th of them, slot i, j
// from a cursor word that the caller zeroed (its value afterwards: how many).  8 consecutive
// slots per thread; output positions are reserved once per workgroup and tile (one cursor add
// per wave was one same-address atomic per 64 slots).  Emit::WIDE: the slots are read whole
// (16-byte loads, 8 payloads held over the reservation); else the key words only, and an
// occupied slot's payload when it is emitted (the set's three output columns: 16 VGPRs less,
// which keeps 8 waves per SIMD).
template <typename Emit>
__global__ __launch_bounds__(256) void k_slots_compact(const uint64_t *tab, uint64_t cap, unsigned long long *cursor,
                                                       Emit emit) {
    __shared__ uint32_t s_w[4];
    __shared__ unsigned long long s_base;
    constexpr int R = 8;
    const uint64_t tile = 256ull * R, step = (uint64_t)gridDim.x * tile;
    for (uint64_t t0 = blockIdx.x * tile; t0 < cap; t0 += step) {
        const uint64_t i0 = t0 + (uint64_t)threadIdx.x * R;
        uint64_t kb[R], pay[Emit::WIDE ? R : 1];
        uint32_t occ = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            if constexpr (Emit::WIDE) {
                const ulonglong2 e = i0 + r < cap ? reinterpret_cast<const ulonglong2 *>(tab)[i0 + r] : make_ulonglong2(SET_EMPTY, 0);
                kb[r] = e.x;
                pay[r] = e.y;
            } else {
                kb[r] = i0 + r < cap ? tab[2 * (i0 + r)] : SET_EMPTY;
            }
            if (kb[r] != SET_EMPTY) occ |= 1u << r;
        }
        uint64_t j = block_reserve<256>((uint32_t)__popc(occ), s_w, &s_base, cursor);
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (!((occ >> r) & 1)) continue;
            const uint64_t i = i0 + r;
            if constexpr (Emit::WIDE) emit(j, i, kb[r], pay[r]);
            else emit(j, i, kb[r], tab[2 * i + 1]);
            j++;
        }
    }
}
template <typename Emit> inline void slots_compact(const DevBuf &tab, uint64_t cap, uint64_t *cursor, Emit emit) {
    hipLaunchKernelGGL(k_slots_compact<Emit>, dim3(blocks_for((cap + 7) / 8, 256)), dim3(256), 0, stream(), tab.as<uint64_t>(),
                       cap, reinterpret_cast<unsigned long long *>(cursor), emit);
    VH_HIP(hipGetLastError());
}

// the first n of an engine's counter words, after everything queued on the library stream
inline std::vector<uint64_t> slots_read_ctr(const DevBuf &ctr, int n) {
    std::vector<uint64_t> c(n);
    VH_HIP(hipMemcpyAsync(c.data(), ctr.ptr, 8 * (uint64_t)n, hipMemcpyDeviceToHost, stream()));
    VH_HIP(hipStreamSynchronize(stream()));
    return c;
}

// ---- host columns ---------------------------------------------------------------------------
// The columns of one update call (any but the keys may be absent), and the stage buffers a
// handle keeps for them: a host column reaches the kernels through a copy on the library
// stream, one chunk of rows at a time, a device column is handed on as it is.
struct HashCols {
    const void *keys;
    const uint8_t *mask, *select;
    const int64_t *counts;
};
struct HostStage {
    DevBuf keys, mask, select, counts;
    // `bytes` of a host array into `buf`; the device pointer
    static void *copy(DevBuf &buf, const void *src, uint64_t bytes) {
        buf.ensure(bytes);
        VH_HIP(hipMemcpyAsync(buf.ptr, src, bytes, hipMemcpyHostToDevice, stream()));
        return buf.ptr;
    }
    // f(chunk's columns on the device, its rows, its first row) over the n rows of `c` (keys of
    // isz bytes), host_chunk rows at a time when they are host arrays, else dev_chunk
    template <typename F>
    void chunks(const HashCols &c, int isz, uint64_t n, int loc, uint64_t host_chunk, uint64_t dev_chunk, F &&f) {
        const uint64_t CH = loc == VH_LOC_HOST ? host_chunk : dev_chunk;
        for (uint64_t r0 = 0; r0 < n; r0 += CH) {
            const uint64_t len = std::min(CH, n - r0);
            HashCols d{static_cast<const char *>(c.keys) + r0 * isz, c.mask ? c.mask + r0 : nullptr,
                       c.select ? c.select + r0 : nullptr, c.counts ? c.counts + r0 : nullptr};
            if (loc == VH_LOC_HOST) {
                d.keys = copy(keys, d.keys, len * isz);
                if (d.mask) d.mask = static_cast<const uint8_t *>(copy(mask, d.mask, len));
                if (d.select) d.select = static_cast<const uint8_t *>(copy(select, d.select, len));
                if (d.counts) d.counts = static_cast<const int64_t *>(copy(counts, d.counts, len * 8));
            }
            f(d, len, r0);
        }
    }
};

}  // namespace vh
