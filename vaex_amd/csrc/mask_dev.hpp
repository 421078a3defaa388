// Bit arithmetic between an Arrow validity bitmap (bit i of byte i / 8, LSB first, 1 = valid) and
// a byte mask (one uint8 per row, 1 = missing: numpy's convention and set_data_mask's), shared by
// the device kernels (missing.hip) and the host check program (tests/host/mask_check.hip), which
// compares each with a naive bit loop.
//
// Everything works on groups of 8 rows: the unit of one lane of the kernels.  A group reads only
// the bitmap bytes that hold one of its rows' bits (one byte, or two when the bit offset is not
// a multiple of 8), so nothing past byte (bit_offset + n - 1) / 8 of the bitmap is touched.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VH_MASK_HD __host__ __device__ inline
#else
#define VH_MASK_HD inline
#endif

namespace vh {
namespace mask {

constexpr uint64_t ONES = 0x0101010101010101ULL;

// the validity bits of the rows [row, row + cnt), 1 <= cnt <= 8, in bits 0 .. cnt-1 (the bits from
// cnt up are unspecified); `first` is the bit number of row 0 in `bits`
VH_MASK_HD uint32_t valid_bits8(const uint8_t *bits, uint64_t first, uint64_t row, uint32_t cnt) {
    const uint64_t b = first + row;
    const uint64_t k = b >> 3;
    const uint32_t s = (uint32_t)(b & 7);
    uint32_t w = bits[k];
    if (s + cnt > 8) w |= (uint32_t)bits[k + 1] << 8;  // the group straddles two bytes
    return (w >> s) & 0xFFu;
}

// 8 validity bits -> 8 mask bytes, row u in byte u (little endian): 1 where bit u is 0
VH_MASK_HD uint64_t expand8(uint32_t valid) {
    uint64_t x = (uint64_t)(~valid & 0xFFu);
    x = (x * ONES) & 0x8040201008040201ULL;              // byte u keeps bit u alone
    return ((x + 0x7F7F7F7F7F7F7F7FULL) >> 7) & ONES;    // a non-zero byte becomes 1
}

// 8 mask bytes (row u in byte u; any non-zero byte is missing) -> 8 validity bits; the rows from
// cnt up read as padding: 0
VH_MASK_HD uint32_t pack8(uint64_t m, uint32_t cnt) {
    const uint64_t nz = ((((m & 0x7F7F7F7F7F7F7F7FULL) + 0x7F7F7F7F7F7F7F7FULL) | m) >> 7) & ONES;  // 1 per non-zero byte
    const uint32_t missing = (uint32_t)((nz * 0x0102040810204080ULL) >> 56);                       // byte u -> bit u
    return ~missing & ((1u << cnt) - 1u) & 0xFFu;
}

// the number of non-zero bytes of a word
VH_MASK_HD uint32_t count8(uint64_t m) {
    const uint64_t nz = ((((m & 0x7F7F7F7F7F7F7F7FULL) + 0x7F7F7F7F7F7F7F7FULL) | m) >> 7) & ONES;
    return (uint32_t)((nz * ONES) >> 56);
}

// the rows [row, row + cnt) of a byte mask as one word, the bytes from cnt up zero
VH_MASK_HD uint64_t load_bytes(const uint8_t *mask, uint64_t row, uint32_t cnt) {
    uint64_t w = 0;
    for (uint32_t u = 0; u < cnt; u++) w |= (uint64_t)mask[row + u] << (8 * u);
    return w;
}

// ---- whole arrays, group by group: what a kernel's lanes do, in a loop (the host check drives
// these, so the grouping and the tails are checked too) ---------------------------------------
VH_MASK_HD void unpack_group(const uint8_t *bits, uint64_t bit_offset, uint64_t n, uint64_t g, uint8_t *out) {
    const uint64_t row = g * 8;
    const uint32_t cnt = (uint32_t)(n - row < 8 ? n - row : 8);
    const uint64_t w = expand8(valid_bits8(bits, bit_offset, row, cnt));
    for (uint32_t u = 0; u < cnt; u++) out[row + u] = (uint8_t)(w >> (8 * u));
}

VH_MASK_HD void pack_group(const uint8_t *mask, uint64_t n, uint64_t g, uint8_t *out_bits) {
    const uint64_t row = g * 8;
    const uint32_t cnt = (uint32_t)(n - row < 8 ? n - row : 8);
    out_bits[g] = (uint8_t)pack8(load_bytes(mask, row, cnt), cnt);
}

}  // namespace mask
}  // namespace vh
