// Pure functions over one string of an Arrow-layout column (a byte range), shared by the
// device kernels (strings.hip, strfn.hip) and the host check programs (tests/host/str_check.hip,
// tests/host/strfn_check.hip), which compare each with a naive byte loop.
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

// ---- transforms -----------------------------------------------------------------
// A transform maps one row to a new string.  Each is a pair over the row and a parameter block:
// out_len<OP> (the byte length of the result) and write<OP> (the result's bytes into a
// destination of exactly that length).  Reads are load_word over a range inside the row or
// single-byte reads inside the row; constants (pattern, replacement, the other side of a cat)
// are read by bytes inside their own ranges; the destination is written by bytes.
enum Transform : int {
    TF_LOWER = 0, TF_UPPER = 1, TF_SLICE = 2, TF_STRIP = 3, TF_PAD = 4, TF_REPEAT = 5, TF_CAT = 6, TF_REPLACE = 7,
    N_TRANSFORMS = 8
};
enum : int { SIDE_LEFT = 1, SIDE_RIGHT = 2, SIDE_BOTH = 3 };
enum : int {
    FN_ASCII = 1,          // lower / upper: a-z / A-Z only, no table
    FN_HAS_STOP = 1,       // slice: b is the stop (else to the end)
    FN_CONST_FIRST = 1,    // cat: the constant comes before the row
    FN_SECOND_COLUMN = 2,  // cat: the other side is the same row of a second column
};
constexpr uint32_t FN_MAX_TABLE = 2048;  // (code point, image) pairs of a case table

struct FnParams {
    int64_t a, b;     // slice: start, stop; pad: width; repeat: repeats; replace: n
    int32_t flags;    // FN_* of the op; strip / pad: SIDE_*
    uint32_t fill;    // pad: the fill byte
    uint64_t set[2];  // strip: bit c is set when the byte c < 128 is stripped
    const uint8_t *c0;  // replace: the pattern; cat: the constant
    const uint8_t *c1;  // replace: the replacement
    const uint32_t *table;  // lower / upper: pairs sorted by code point, code points >= 128 only
    uint32_t n0, n1, ntable;
};

// a word whose bytes are all below 0x80
VH_STR_HD uint64_t ascii_lower_word(uint64_t w) {
    const uint64_t ge_A = w + 0x3f3f3f3f3f3f3f3fULL, gt_Z = w + 0x2525252525252525ULL;
    return w | ((ge_A & ~gt_Z & 0x8080808080808080ULL) >> 2);
}
VH_STR_HD uint64_t ascii_upper_word(uint64_t w) {
    const uint64_t ge_a = w + 0x1f1f1f1f1f1f1f1fULL, gt_z = w + 0x0505050505050505ULL;
    return w ^ ((ge_a & ~gt_z & 0x8080808080808080ULL) >> 2);
}

// the image of a code point under a case table (a binary search), itself when the table lacks it
VH_STR_HD uint32_t case_image(const uint32_t *table, uint32_t n, uint32_t cp) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1, k = table[2 * mid];
        if (k == cp) return table[2 * mid + 1];
        if (k < cp) lo = mid + 1;
        else hi = mid;
    }
    return cp;
}

VH_STR_HD unsigned utf8_size(uint32_t cp) { return cp < 0x80 ? 1 : cp < 0x800 ? 2 : cp < 0x10000 ? 3 : 4; }
VH_STR_HD void utf8_put(uint32_t cp, unsigned size, uint8_t *d) {
    if (size == 1) {
        d[0] = (uint8_t)cp;
    } else if (size == 2) {
        d[0] = (uint8_t)(0xC0 | cp >> 6);
        d[1] = (uint8_t)(0x80 | (cp & 0x3F));
    } else if (size == 3) {
        d[0] = (uint8_t)(0xE0 | cp >> 12);
        d[1] = (uint8_t)(0x80 | (cp >> 6 & 0x3F));
        d[2] = (uint8_t)(0x80 | (cp & 0x3F));
    } else {
        d[0] = (uint8_t)(0xF0 | cp >> 18);
        d[1] = (uint8_t)(0x80 | (cp >> 12 & 0x3F));
        d[2] = (uint8_t)(0x80 | (cp >> 6 & 0x3F));
        d[3] = (uint8_t)(0x80 | (cp & 0x3F));
    }
}

// The unit that starts at the non-ASCII byte p[i]: the bytes (2 .. 4) of a well-formed sequence
// with its code point in cp, or 1 byte with cp = ~0 for anything else (a stray continuation byte,
// a lead byte whose sequence the row cuts short or a non-continuation byte interrupts, an
// overlong form, a value past U+10FFFF): such a byte is copied through.  Reads stay below len.
VH_STR_HD unsigned utf8_unit(const uint8_t *p, uint64_t len, uint64_t i, uint32_t &cp) {
    const uint8_t b = p[i];
    cp = ~0u;
    unsigned size;
    uint32_t v, least;
    if (b >= 0xC0 && b < 0xE0) {
        size = 2, v = b & 0x1Fu, least = 0x80;
    } else if (b >= 0xE0 && b < 0xF0) {
        size = 3, v = b & 0x0Fu, least = 0x800;
    } else if (b >= 0xF0 && b < 0xF8) {
        size = 4, v = b & 0x07u, least = 0x10000;
    } else {
        return 1;
    }
    if (i + size > len) return 1;
    for (unsigned j = 1; j < size; j++) {
        const uint8_t c = p[i + j];
        if ((c & 0xC0) != 0x80) return 1;
        v = v << 6 | (c & 0x3Fu);
    }
    if (v < least || v > 0x10FFFF) return 1;
    cp = v;
    return size;
}

// lower / upper: the bytes of the result (written to dst when WRITE).  Runs of ASCII go a word
// at a time; a code point >= 128 goes through the table and may change its UTF-8 length.
template <bool UPPER, bool WRITE>
VH_STR_HD uint64_t case_map(const FnParams &P, const uint8_t *p, uint64_t len, uint8_t *dst) {
    uint64_t i = 0, o = 0;
    while (i < len) {
        const uint64_t rem = len - i;
        const unsigned nb = rem < 8 ? (unsigned)rem : 8u;
        uint64_t w = load_word(p + i, rem, 0);
        const uint64_t high = w & 0x8080808080808080ULL;
        const unsigned na = high ? (unsigned)__builtin_ctzll(high) >> 3 : nb;  // the leading ASCII bytes
        if (na) {
            if (WRITE) {
                if (na < 8) w &= (1ULL << (8 * na)) - 1;
                w = UPPER ? ascii_upper_word(w) : ascii_lower_word(w);
                for (unsigned j = 0; j < na; j++) dst[o + j] = (uint8_t)(w >> (8 * j));
            }
            o += na;
            i += na;
        }
        if (!high) continue;
        uint32_t cp;
        const unsigned size = utf8_unit(p, len, i, cp);
        if (cp != ~0u && !(P.flags & FN_ASCII)) {
            const uint32_t image = case_image(P.table, P.ntable, cp);
            const unsigned osize = utf8_size(image);
            if (WRITE) utf8_put(image, osize, dst + o);
            o += osize;
        } else {
            if (WRITE)
                for (unsigned j = 0; j < size; j++) dst[o + j] = p[i + j];
            o += size;
        }
        i += size;
    }
    return o;
}

// the byte position at which code point k of p[0 .. len) starts (a code point starts at every
// byte that is no continuation byte): 0 for k == 0, len for k at or past the count
VH_STR_HD uint64_t codepoint_offset(const uint8_t *p, uint64_t len, uint64_t k) {
    if (k == 0) return 0;
    const uint64_t nw = (len + 7) >> 3;
    uint64_t seen = 0;
    for (uint64_t kw = 0; kw < nw; kw++) {
        const uint64_t rem = len - 8 * kw;
        const unsigned nb = rem < 8 ? (unsigned)rem : 8u;
        const uint64_t w = load_word(p, len, kw);
        const unsigned c = word_codepoints(w, nb);
        if (seen + c > k) {
            for (unsigned j = 0; j < nb; j++) {
                if (((w >> (8 * j)) & 0xC0) == 0x80) continue;
                if (seen == k) return 8 * kw + j;
                seen++;
            }
        }
        seen += c;
    }
    return len;
}

// What the copying transforms (slice, strip, pad, repeat, cat) write: lfill fill bytes, the
// bytes pre[0 .. npre), the row's bytes [b0, b1) rep times, suf[0 .. nsuf), rfill fill bytes.
struct Pieces {
    uint64_t lfill, npre, b0, b1, rep, nsuf, rfill;
    const uint8_t *pre, *suf;
    uint8_t fill;
};
// sums and products that stop at LEN_SATURATED: repeats and widths are any int64, so a result's
// length may not fit; the plan refuses a saturated length and nothing is written for it
constexpr uint64_t LEN_SATURATED = ~0ULL;
VH_STR_HD uint64_t sat_add(uint64_t a, uint64_t b) {
    uint64_t r;
    return __builtin_add_overflow(a, b, &r) ? LEN_SATURATED : r;
}
VH_STR_HD uint64_t sat_mul(uint64_t a, uint64_t b) {
    uint64_t r;
    return __builtin_mul_overflow(a, b, &r) ? LEN_SATURATED : r;
}
VH_STR_HD uint64_t pieces_len(const Pieces &s) {
    return sat_add(sat_add(sat_add(s.lfill, s.npre), sat_mul(s.b1 - s.b0, s.rep)), sat_add(s.nsuf, s.rfill));
}

// s[start:stop] of Python, counted in code points
VH_STR_HD void slice_range(const FnParams &P, const uint8_t *p, uint64_t len, uint64_t &b0, uint64_t &b1) {
    int64_t start = P.a, stop = P.b;
    const bool has_stop = P.flags & FN_HAS_STOP;
    if (start < 0 || (has_stop && stop < 0)) {
        const int64_t n = (int64_t)count_codepoints(p, len);
        if (start < 0) start = start + n < 0 ? 0 : start + n;
        if (has_stop && stop < 0) stop = stop + n < 0 ? 0 : stop + n;
    }
    b0 = codepoint_offset(p, len, (uint64_t)start);
    b1 = has_stop ? codepoint_offset(p, len, (uint64_t)stop) : len;
    if (b1 < b0) b1 = b0;
}
VH_STR_HD bool in_set(const FnParams &P, uint8_t c) { return c < 128 && (P.set[c >> 6] >> (c & 63) & 1); }

// q / qlen: the same row of the second column (cat with FN_SECOND_COLUMN), else unused.
// TF_REPEAT and TF_CAT take their lengths from len / qlen alone: the plan pass reads no byte.
template <int OP>
VH_STR_HD Pieces pieces(const FnParams &P, const uint8_t *p, uint64_t len, const uint8_t *q, uint64_t qlen) {
    Pieces s{0, 0, 0, len, 1, 0, 0, nullptr, nullptr, (uint8_t)P.fill};
    if (OP == TF_SLICE) {
        slice_range(P, p, len, s.b0, s.b1);
    } else if (OP == TF_STRIP) {
        if (P.flags & SIDE_LEFT)
            while (s.b0 < s.b1 && in_set(P, p[s.b0])) s.b0++;
        if (P.flags & SIDE_RIGHT)
            while (s.b1 > s.b0 && in_set(P, p[s.b1 - 1])) s.b1--;
    } else if (OP == TF_PAD) {
        const int64_t n = (int64_t)count_codepoints(p, len);
        const uint64_t margin = P.a > n ? (uint64_t)(P.a - n) : 0;
        // selects, not stores to the one or the other member (those become an indexed store to scratch)
        const uint64_t half = margin / 2 + (margin & (uint64_t)P.a & 1);  // CPython's str.center
        s.lfill = P.flags == SIDE_LEFT ? margin : P.flags == SIDE_RIGHT ? 0 : half;
        s.rfill = margin - s.lfill;
    } else if (OP == TF_REPEAT) {
        s.rep = P.a > 0 ? (uint64_t)P.a : 0;
    } else if (OP == TF_CAT) {
        const bool second = P.flags & FN_SECOND_COLUMN, first = !second && (P.flags & FN_CONST_FIRST);
        s.pre = P.c0;
        s.npre = first ? P.n0 : 0;
        s.suf = second ? q : P.c0;
        s.nsuf = second ? qlen : first ? 0 : P.n0;
    }
    return s;
}
// Section [o, o + n) of the destination from src[0 .. n): the positions that are first modulo
// STRIDE.  STRIDE 1 is the whole section (a lane per row); a wave per row gives lane l the
// positions l modulo 64.  A null src writes the fill byte.
template <unsigned STRIDE>
VH_STR_HD void section_write(uint8_t *dst, uint64_t o, const uint8_t *src, uint64_t n, uint8_t fill, unsigned first) {
    const unsigned r = (unsigned)(o % STRIDE);
    uint64_t k = first >= r ? first - r : first + STRIDE - r;
    if (src)
        for (; k < n; k += STRIDE) dst[o + k] = src[k];
    else
        for (; k < n; k += STRIDE) dst[o + k] = fill;
}
template <unsigned STRIDE> VH_STR_HD void pieces_write(const Pieces &s, const uint8_t *p, uint8_t *dst, unsigned first) {
    uint64_t o = 0;
    section_write<STRIDE>(dst, o, nullptr, s.lfill, s.fill, first);
    o += s.lfill;
    section_write<STRIDE>(dst, o, s.pre, s.npre, 0, first);
    o += s.npre;
    const uint64_t w = s.b1 - s.b0;
    for (uint64_t r = 0; w && r < s.rep; r++, o += w) section_write<STRIDE>(dst, o, p + s.b0, w, 0, first);
    section_write<STRIDE>(dst, o, s.suf, s.nsuf, 0, first);
    o += s.nsuf;
    section_write<STRIDE>(dst, o, nullptr, s.rfill, s.fill, first);
}

// literal, leftmost, non-overlapping; P.a < 0: every occurrence.  The pattern is not empty.
template <bool WRITE> VH_STR_HD uint64_t replace(const FnParams &P, const uint8_t *p, uint64_t len, uint8_t *dst) {
    uint64_t i = 0, o = 0;
    for (int64_t left = P.a; left != 0; left -= left > 0) {
        const int64_t f = find(p + i, len - i, P.c0, P.n0);
        if (f < 0) break;
        if (WRITE) {
            for (int64_t k = 0; k < f; k++) dst[o + k] = p[i + k];
            for (uint32_t k = 0; k < P.n1; k++) dst[o + f + k] = P.c1[k];
        }
        o += (uint64_t)f + P.n1;
        i += (uint64_t)f + P.n0;
    }
    if (WRITE)
        for (uint64_t k = i; k < len; k++) dst[o + k - i] = p[k];
    return o + (len - i);
}

constexpr bool is_copy_transform(int op) { return op >= TF_SLICE && op <= TF_CAT; }

template <int OP> VH_STR_HD uint64_t out_len(const FnParams &P, const uint8_t *p, uint64_t len, const uint8_t *q, uint64_t qlen) {
    if (OP == TF_LOWER) return case_map<false, false>(P, p, len, nullptr);
    if (OP == TF_UPPER) return case_map<true, false>(P, p, len, nullptr);
    if (OP == TF_REPLACE) return replace<false>(P, p, len, nullptr);
    return pieces_len(pieces<OP>(P, p, len, q, qlen));
}
template <int OP>
VH_STR_HD void write(const FnParams &P, const uint8_t *p, uint64_t len, const uint8_t *q, uint64_t qlen, uint8_t *dst) {
    if (OP == TF_LOWER) case_map<false, true>(P, p, len, dst);
    else if (OP == TF_UPPER) case_map<true, true>(P, p, len, dst);
    else if (OP == TF_REPLACE) replace<true>(P, p, len, dst);
    else pieces_write<1>(pieces<OP>(P, p, len, q, qlen), p, dst, 0);
}

}  // namespace str
}  // namespace vh
