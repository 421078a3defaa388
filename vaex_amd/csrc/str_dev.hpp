// Pure functions over one string of an Arrow-layout column (a byte range), shared by the
// device kernels (strings.hip) and the host check program (tests/host/str_check.hip), which
// compares each with a naive byte loop.
//
// Reads go through load_word: the k-th 8-byte word of the string, little endian, bytes past
// the end zero.  It is assembled from the one or two ALIGNED 8-byte words of memory that hold
// those bytes, and touches an aligned word only when that word holds a byte of the string; so
// nothing before the 8-aligned word of the first byte or after the 8-aligned word of the last
// byte is read (a column's byte buffer starts 8-aligned and carries slack after its end), and a
// string's words do not depend on where it starts.  An empty string reads nothing.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VH_STR_HD __host__ __device__ inline
#else
#define VH_STR_HD inline
#endif

namespace vh {
namespace str {

enum MatchOp : int { OP_EQ = 0, OP_NE = 1, OP_STARTSWITH = 2, OP_ENDSWITH = 3, OP_CONTAINS = 4, N_MATCH_OPS = 5 };
enum LenKind : int { LEN_BYTES = 0, LEN_CODEPOINTS = 1 };

VH_STR_HD uint64_t mix64(uint64_t x) {  // the splitmix64 finaliser
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

VH_STR_HD uint64_t aligned_word(const uint8_t *a) {  // a is 8-aligned
    uint64_t w;
    __builtin_memcpy(&w, __builtin_assume_aligned(a, 8), 8);
    return w;
}

// word k (8 * k < len) of the string p[0 .. len)
VH_STR_HD uint64_t load_word(const uint8_t *p, uint64_t len, uint64_t k) {
    const uint8_t *q = p + 8 * k;
    const unsigned s = (unsigned)(reinterpret_cast<uintptr_t>(q) & 7);
    const uint8_t *a = q - s;
    const uint64_t rem = len - 8 * k;
    const unsigned nb = rem < 8 ? (unsigned)rem : 8u;
    uint64_t w = aligned_word(a) >> (8 * s);
    if (s && nb > 8 - s) w |= aligned_word(a + 8) << (64 - 8 * s);  // the head was masked by the shift
    if (nb < 8) w &= (1ULL << (8 * nb)) - 1;                         // the tail
    return w;
}

// The seeded 64-bit hash: a sum of one mixed term per word (so a wave can share the words of a
// long string among its lanes and add up), finished with the length.
VH_STR_HD uint64_t seed_key(uint64_t seed) { return mix64(seed + 0x9e3779b97f4a7c15ULL); }
VH_STR_HD uint64_t hash_term(uint64_t w, uint64_t k, uint64_t sk) { return mix64((w ^ sk) + 0x9e3779b97f4a7c15ULL * (k + 1)); }
VH_STR_HD uint64_t hash_finish(uint64_t sum, uint64_t len, uint64_t sk) { return mix64(sum ^ (len * 0xff51afd7ed558ccdULL) ^ sk); }
VH_STR_HD uint64_t hash(const uint8_t *p, uint64_t len, uint64_t seed) {
    const uint64_t sk = seed_key(seed), nw = (len + 7) >> 3;
    uint64_t sum = 0;
    for (uint64_t k = 0; k < nw; k++) sum += hash_term(load_word(p, len, k), k, sk);
    return hash_finish(sum, len, sk);
}
// the key a slot table holds for a hash: its low `bits` bits (64: all of them; fewer is the
// encoder's test seam), never the table's EMPTY word
VH_STR_HD uint64_t slot_key(uint64_t h, int bits) {
    if (bits < 64) h = bits > 0 ? h & ((1ULL << bits) - 1) : 0;
    return h == ~0ULL ? 0x7fffffffffffffffULL : h;
}

// a[0 .. len) == b[0 .. len)
VH_STR_HD bool equal(const uint8_t *a, const uint8_t *b, uint64_t len) {
    const uint64_t nw = (len + 7) >> 3;
    for (uint64_t k = 0; k < nw; k++)
        if (load_word(a, len, k) != load_word(b, len, k)) return false;
    return true;
}

// the bytes of a word of nb valid bytes that are no UTF-8 continuation byte (10xxxxxx)
VH_STR_HD unsigned word_codepoints(uint64_t w, unsigned nb) {
    const uint64_t cont = (w >> 7) & ~(w >> 6) & 0x0101010101010101ULL;  // masked-off bytes are 0: not counted
    return nb - (unsigned)__builtin_popcountll(cont);
}
VH_STR_HD uint64_t count_codepoints(const uint8_t *p, uint64_t len) {
    const uint64_t nw = (len + 7) >> 3;
    uint64_t n = 0;
    for (uint64_t k = 0; k < nw; k++) {
        const uint64_t rem = len - 8 * k;
        n += word_codepoints(load_word(p, len, k), rem < 8 ? (unsigned)rem : 8u);
    }
    return n;
}

// the first position of pat[0 .. m) in p[0 .. len), -1 when there is none (an empty pattern is
// found at 0); byte reads inside the two ranges only
VH_STR_HD int64_t find(const uint8_t *p, uint64_t len, const uint8_t *pat, uint64_t m) {
    if (m == 0) return 0;
    if (m > len) return -1;
    const uint8_t c0 = pat[0];
    for (uint64_t i = 0; i + m <= len; i++) {
        if (p[i] != c0) continue;
        uint64_t j = 1;
        while (j < m && p[i + j] == pat[j]) j++;
        if (j == m) return (int64_t)i;
    }
    return -1;
}

// pat is read by words too: it lies in a buffer of its own with the column buffer's contract
VH_STR_HD bool match(int op, const uint8_t *p, uint64_t len, const uint8_t *pat, uint64_t m) {
    switch (op) {
    case OP_EQ: return len == m && equal(p, pat, m);
    case OP_NE: return !(len == m && equal(p, pat, m));
    case OP_STARTSWITH: return len >= m && equal(p, pat, m);
    case OP_ENDSWITH: return len >= m && equal(p + (len - m), pat, m);
    default: return find(p, len, pat, m) >= 0;
    }
}

// offsets of a taken column: the input's width, int64 once the bytes reach 2^31
inline bool take_needs_wide(bool input_wide, uint64_t total_bytes) { return input_wide || total_bytes >= (1ULL << 31); }

}  // namespace str
}  // namespace vh
