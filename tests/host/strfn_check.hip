// Runs every out_len / write pair of csrc/str_dev.hpp (the string transforms) on
// the CPU and compares it with a naive byte loop (tests/test_strfn_check.py checks every line):
// the same functions the device kernels of strfn.hip inline, compiled for the host.  No GPU and
// no HIP runtime call.
//
// Every input row sits in a heap block of exactly its bytes (from the 8-aligned word of its
// first byte) rounded up to 8, every constant in a block of exactly its bytes, and every
// destination in a block of exactly out_len bytes, so that a build with -fsanitize=address
// reports any read outside the row's aligned words and any write past the result.
//
// stdout: one line per (function, input), `<function> <input> ok` or `... FAIL <variant>`; the
// last line is `cases <n> failed <m>`.  Exit status 1 when a case failed.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "str_dev.hpp"

using namespace vh::str;

static int g_cases = 0, g_failed = 0;
static void report(const char *fn, const std::string &name, const std::string &bad) {
    g_cases++;
    if (!bad.empty()) g_failed++;
    std::printf("%s %s %s%s%s\n", fn, name.c_str(), bad.empty() ? "ok" : "FAIL", bad.empty() ? "" : " ", bad.c_str());
}

// s at byte `align` of a block of (align + size) rounded up to 8 bytes
struct Row {
    uint8_t *mem;
    const uint8_t *p;
    uint64_t len;
    Row(const std::string &s, unsigned align) {
        const size_t sz = (align + s.size() + 7) / 8 * 8;
        mem = static_cast<uint8_t *>(std::malloc(sz));
        if (sz) std::memset(mem, 0xAB, sz);  // what surrounds the row must not matter
        if (!s.empty()) std::memcpy(mem + align, s.data(), s.size());
        p = mem + align;
        len = s.size();
    }
    ~Row() { std::free(mem); }
};
// exactly the bytes of s
static uint8_t *exact(const std::string &s) {
    uint8_t *b = static_cast<uint8_t *>(std::malloc(s.size()));
    if (!s.empty()) std::memcpy(b, s.data(), s.size());
    return b;
}

// ---- the naive side ---------------------------------------------------------------------------
using Table = std::vector<uint32_t>;  // (code point, image) pairs, sorted
static const Table LOWER = {0xC9, 0xE9, 0x130, 0x69, 0x1E9E, 0xDF, 0x2C6F, 0x250, 0x10400, 0x10428};
static const Table UPPER = {0xDF, 0x1E9E, 0xE9, 0xC9, 0x250, 0x2C6F, 0x10428, 0x10400};

static std::string naive_utf8(uint32_t cp) {
    std::string o;
    if (cp < 0x80) {
        o += (char)cp;
    } else if (cp < 0x800) {
        o += (char)(0xC0 | cp >> 6);
        o += (char)(0x80 | (cp & 63));
    } else if (cp < 0x10000) {
        o += (char)(0xE0 | cp >> 12);
        o += (char)(0x80 | (cp >> 6 & 63));
        o += (char)(0x80 | (cp & 63));
    } else {
        o += (char)(0xF0 | cp >> 18);
        o += (char)(0x80 | (cp >> 12 & 63));
        o += (char)(0x80 | (cp >> 6 & 63));
        o += (char)(0x80 | (cp & 63));
    }
    return o;
}
static std::string naive_case(const std::string &s, bool upper, bool ascii, const Table &t) {
    std::string o;
    size_t i = 0;
    while (i < s.size()) {
        const uint8_t b = (uint8_t)s[i];
        if (b < 0x80) {
            if (upper) o += (char)((b >= 'a' && b <= 'z') ? b - 32 : b);
            else o += (char)((b >= 'A' && b <= 'Z') ? b + 32 : b);
            i++;
            continue;
        }
        const size_t size = (b & 0xE0) == 0xC0 ? 2 : (b & 0xF0) == 0xE0 ? 3 : (b & 0xF8) == 0xF0 ? 4 : 0;
        bool good = size && i + size <= s.size();
        uint32_t cp = good ? b & (0xFFu >> (size + 1)) : 0;
        for (size_t j = 1; good && j < size; j++) {
            good = ((uint8_t)s[i + j] & 0xC0) == 0x80;
            cp = cp << 6 | ((uint8_t)s[i + j] & 63);
        }
        good = good && naive_utf8(cp).size() == size && cp <= 0x10FFFF;
        if (!good) {  // copied through, one byte
            o += (char)b;
            i++;
            continue;
        }
        uint32_t image = cp;
        for (size_t k = 0; !ascii && k < t.size(); k += 2)
            if (t[k] == cp) image = t[k + 1];
        o += naive_utf8(image);
        i += size;
    }
    return o;
}
static std::vector<size_t> starts(const std::string &s) {
    std::vector<size_t> v;
    for (size_t i = 0; i < s.size(); i++)
        if (((uint8_t)s[i] & 0xC0) != 0x80) v.push_back(i);
    return v;
}
static std::string naive_slice(const std::string &s, int64_t start, bool has_stop, int64_t stop) {
    const std::vector<size_t> st = starts(s);
    const int64_t n = (int64_t)st.size();
    if (!has_stop) stop = n;
    if (start < 0) start = std::max<int64_t>(0, start + n);
    if (stop < 0) stop = std::max<int64_t>(0, stop + n);
    auto at = [&](int64_t k) { return k == 0 ? (size_t)0 : k < n ? st[k] : s.size(); };
    const size_t b0 = at(start), b1 = at(stop);
    return b1 > b0 ? s.substr(b0, b1 - b0) : std::string();
}
static std::string naive_strip(const std::string &s, const std::string &set, int sides) {
    size_t b0 = 0, b1 = s.size();
    if (sides & SIDE_LEFT)
        while (b0 < b1 && set.find(s[b0]) != std::string::npos) b0++;
    if (sides & SIDE_RIGHT)
        while (b1 > b0 && set.find(s[b1 - 1]) != std::string::npos) b1--;
    return s.substr(b0, b1 - b0);
}
static std::string naive_pad(const std::string &s, int64_t width, int side, char fill) {
    const int64_t n = (int64_t)starts(s).size();
    const int64_t margin = width > n ? width - n : 0;
    int64_t left = side == SIDE_LEFT ? margin : side == SIDE_RIGHT ? 0 : margin / 2 + (margin & width & 1);
    return std::string((size_t)left, fill) + s + std::string((size_t)(margin - left), fill);
}
static std::string naive_repeat(const std::string &s, int64_t k) {
    std::string o;
    for (int64_t i = 0; i < k; i++) o += s;
    return o;
}
static std::string naive_replace(const std::string &s, const std::string &pat, const std::string &repl, int64_t n) {
    std::string o;
    size_t i = 0;
    while (n != 0) {
        const size_t f = s.find(pat, i);
        if (f == std::string::npos) break;
        o += s.substr(i, f - i) + repl;
        i = f + pat.size();
        if (n > 0) n--;
    }
    return o + s.substr(i);
}

// ---- one comparison ---------------------------------------------------------------------------
template <int OP>
static bool same(const FnParams &P, const Row &r, const Row *second, const std::string &expect) {
    const uint8_t *q = second ? second->p : nullptr;
    const uint64_t qlen = second ? second->len : 0;
    const uint64_t n = out_len<OP>(P, r.p, r.len, q, qlen);
    if (n != expect.size()) return false;
    uint8_t *dst = static_cast<uint8_t *>(std::malloc(n));  // exactly out_len bytes: a sanitizer build sees any write past them
    write<OP>(P, r.p, r.len, q, qlen, dst);
    bool ok = n == 0 || std::memcmp(dst, expect.data(), n) == 0;
    // the plain build's own check of "exactly out_len bytes": the destination inside a block
    // pre-filled with a byte (two different ones in turn, so no result byte can hide a gap), with
    // guard bytes before and after it that must keep the fill
    constexpr size_t GUARD = 16;
    uint8_t *wide = static_cast<uint8_t *>(std::malloc(n + 2 * GUARD));
    auto filled = [&](uint8_t fill) {
        bool good = n == 0 || std::memcmp(wide + GUARD, expect.data(), n) == 0;
        for (size_t k = 0; k < GUARD; k++) good = good && wide[k] == fill && wide[GUARD + n + k] == fill;
        return good;
    };
    for (uint8_t fill : {(uint8_t)0xEE, (uint8_t)0x11}) {
        std::memset(wide, fill, n + 2 * GUARD);
        write<OP>(P, r.p, r.len, q, qlen, wide + GUARD);
        ok = ok && filled(fill);
        if (is_copy_transform(OP)) {  // the wave-per-row form: 64 lanes, each every 64th byte
            const Pieces s = pieces<OP>(P, r.p, r.len, q, qlen);
            ok = ok && pieces_len(s) == n;
            std::memset(wide, fill, n + 2 * GUARD);
            for (unsigned lane = 0; lane < 64; lane++) pieces_write<64>(s, r.p, wide + GUARD, lane);
            ok = ok && filled(fill);
        }
    }
    if (is_copy_transform(OP)) {  // and into the exact block
        const Pieces s = pieces<OP>(P, r.p, r.len, q, qlen);
        for (unsigned lane = 0; lane < 64; lane++) pieces_write<64>(s, r.p, dst, lane);
        ok = ok && (n == 0 || std::memcmp(dst, expect.data(), n) == 0);
    }
    std::free(wide);
    std::free(dst);
    return ok;
}

static void check_all(const std::string &name, const std::string &s, unsigned align, bool full) {
    const Row r(s, align);
    std::string bad;
    char buf[96];
    // lower / upper
    for (int upper = 0; upper < 2; upper++) {
        bad.clear();
        for (int ascii = 0; ascii < 2; ascii++) {
            const Table &t = upper ? UPPER : LOWER;
            uint32_t *tab = static_cast<uint32_t *>(std::malloc(t.size() * 4));
            std::memcpy(tab, t.data(), t.size() * 4);
            FnParams P{};
            P.flags = ascii ? FN_ASCII : 0;
            P.table = ascii ? nullptr : tab;
            P.ntable = ascii ? 0 : (uint32_t)(t.size() / 2);
            const std::string e = naive_case(s, upper, ascii, t);
            const bool ok = upper ? same<TF_UPPER>(P, r, nullptr, e) : same<TF_LOWER>(P, r, nullptr, e);
            if (!ok) bad += ascii ? " ascii" : " table";
            std::free(tab);
        }
        report(upper ? "upper" : "lower", name, bad);
    }
    // slice
    bad.clear();
    const int64_t bounds[] = {0, 1, 2, 3, 5, 8, 17, 18, 100000, -1, -2, -3, -9, -18, -100000};
    for (int64_t a : bounds) {
        for (int hs = 0; hs < 2; hs++) {
            for (int64_t b : bounds) {
                if ((!hs && b != 0) || (!full && (a > 8 || a < -3 || b > 8 || b < -3))) continue;
                FnParams P{};
                P.a = a, P.b = b, P.flags = hs ? FN_HAS_STOP : 0;
                if (!same<TF_SLICE>(P, r, nullptr, naive_slice(s, a, hs, b))) {
                    std::snprintf(buf, sizeof buf, " [%" PRId64 ":%" PRId64 "%s]", a, b, hs ? "" : " none");
                    bad += buf;
                }
            }
        }
    }
    report("slice", name, bad);
    // strip
    bad.clear();
    const std::string sets[] = {" \t\n\v\f\r", "", "a", "xf\x01z", "\x7f!"};
    for (const std::string &set : sets) {
        for (int side = SIDE_LEFT; side <= SIDE_BOTH; side++) {
            FnParams P{};
            P.flags = side;
            for (char c : set) P.set[(uint8_t)c >> 6] |= 1ULL << (c & 63);
            if (!same<TF_STRIP>(P, r, nullptr, naive_strip(s, set, side))) {
                std::snprintf(buf, sizeof buf, " set%zu/side%d", set.size(), side);
                bad += buf;
            }
        }
    }
    report("strip", name, bad);
    // pad
    bad.clear();
    const int64_t widths[] = {-1, 0, 1, 4, 5, 9, 16, 17, 18, 19, 40};
    for (int64_t w : widths) {
        for (int side = SIDE_LEFT; side <= SIDE_BOTH; side++) {
            if (!full && w > 9) continue;
            FnParams P{};
            P.a = w, P.flags = side, P.fill = '*';
            if (!same<TF_PAD>(P, r, nullptr, naive_pad(s, w, side, '*'))) {
                std::snprintf(buf, sizeof buf, " w%" PRId64 "/side%d", w, side);
                bad += buf;
            }
        }
    }
    report("pad", name, bad);
    // repeat
    bad.clear();
    for (int64_t k : {-2, 0, 1, 3}) {
        FnParams P{};
        P.a = k;
        if (!same<TF_REPEAT>(P, r, nullptr, naive_repeat(s, k))) {
            std::snprintf(buf, sizeof buf, " x%" PRId64, k);
            bad += buf;
        }
    }
    report("repeat", name, bad);
    // cat: a constant after, a constant before, a second column's row
    bad.clear();
    for (const std::string &c : {std::string(), std::string("_"), std::string("\xc3\xa9suffix9")}) {
        for (int first = 0; first < 2; first++) {
            uint8_t *k = exact(c);
            FnParams P{};
            P.flags = first ? FN_CONST_FIRST : 0;
            P.c0 = k, P.n0 = (uint32_t)c.size();
            if (!same<TF_CAT>(P, r, nullptr, first ? c + s : s + c)) bad += first ? " const+s" : " s+const";
            std::free(k);
        }
        for (unsigned a2 = 0; a2 < 8; a2 += 3) {
            const Row r2(c, a2);
            FnParams P{};
            P.flags = FN_SECOND_COLUMN;
            if (!same<TF_CAT>(P, r, &r2, s + c)) bad += " s+t";
        }
    }
    report("cat", name, bad);
    // replace
    bad.clear();
    const std::string pats[] = {"a", "aa", "ab", "f", "\x01", "\xc3\xa9", "zzzzzzzzzzzzzzzzzzzz"};
    const std::string repls[] = {"", "X", "a", "longer than the pattern"};
    for (const std::string &pat : pats) {
        for (const std::string &repl : repls) {
            for (int64_t n : {-1, 0, 1, 2}) {
                uint8_t *kp = exact(pat), *kr = exact(repl);
                FnParams P{};
                P.a = n, P.c0 = kp, P.n0 = (uint32_t)pat.size(), P.c1 = kr, P.n1 = (uint32_t)repl.size();
                if (!same<TF_REPLACE>(P, r, nullptr, naive_replace(s, pat, repl, n))) {
                    std::snprintf(buf, sizeof buf, " pat%zu/repl%zu/n%" PRId64, pat.size(), repl.size(), n);
                    bad += buf;
                }
                std::free(kp);
                std::free(kr);
            }
        }
    }
    report("replace", name, bad);
}

int main() {
    // lengths 0 .. 17 at every start alignment 0 .. 7 (the edge strings of tests/strings_np.py)
    for (int L = 0; L <= 17; L++) {
        for (int A = 0; A < 8; A++) {
            std::string s;
            for (int i = 0; i < L; i++) s += (char)(1 + (i * 7 + L * 13 + A) % 126);
            check_all("edge_len" + std::to_string(L) + "_at" + std::to_string(A), s, (unsigned)A, true);
        }
    }
    struct Named {
        const char *name;
        std::string s;
    };
    const Named special[] = {
        {"nul", std::string("a\0b", 3)},
        {"nuls", std::string("\0\0\0", 3)},
        {"aaaa", "aaaa"},
        {"aaab", "aaab"},
        {"spaces", " \t\n\v\f\r "},
        {"space_mid", "  a b  "},
        {"fs_us", "\x1c x \x1f"},
        {"nbsp", "\xc2\xa0x\xc2\xa0"},
        {"minus5", "-5"},
        {"MiXed", "MiXed Case 09 az AZ @[`{"},
        {"e_acute", "\xc3\xa9"},
        {"E_acute_x", "\xc3\x89x\xc3\x89"},
        {"euro", "\xe2\x82\xac"},
        {"clef", "\xf0\x9d\x84\x9e"},
        {"mix", "a\xc3\xa9\xe2\x82\xac\xf0\x9d\x84\x9ez"},
        {"dotted_I_shrinks", "x\xc4\xb0y\xc4\xb0"},               // U+0130 -> i: 2 bytes -> 1
        {"sharp_s_grows", "stra\xc3\x9f" "e\xc3\x9f"},            // U+00DF -> U+1E9E: 2 -> 3
        {"capital_sharp_s", "\xe1\xba\x9e"},                      // U+1E9E -> U+00DF: 3 -> 2
        {"turned_a", "\xc9\x90\xe2\xb1\xaf"},                     // U+0250 <-> U+2C6F
        {"deseret", "\xf0\x90\x90\x80\xf0\x90\x90\xa8"},          // U+10400 <-> U+10428 (4 bytes)
        {"word_edge", "abcdefg\xc3\xa9hijklmn\xe2\x82\xacopqrstu\xf0\x90\x90\x80"},
        {"truncated2", "ab\xc3"},
        {"truncated3", "ab\xe2\x82"},
        {"truncated4", "abcdefg\xf0\x90\x90"},
        {"truncated4_1", "\xf0"},
        {"stray", "\xa9" "ab\x80"},
        {"stray_end", "abcdefgh\xa9"},
        {"interrupted", "\xe2" "a\x82\xac"},
        {"overlong", "\xc1\x81\xe0\x83\x9f"},
        {"surrogate", "\xed\xa0\x80x"},
        {"past_10ffff", "\xf4\x90\x80\x80\xf8\x88\x80\x80\x80"},
    };
    for (const Named &c : special)
        for (unsigned A = 0; A < 8; A++) check_all(std::string(c.name) + "_at" + std::to_string(A), c.s, A, true);
    // one row of 70,000 bytes, with multi-byte code points sprinkled in
    std::string big = "x";
    for (int i = 0; big.size() < 69990; i++) {
        big += (char)(97 + (i * 31 + i / 251) % 26);
        if (i % 997 == 0) big += "\xc3\x9f";
        if (i % 4001 == 0) big += " \xf0\x90\x90\xa8";
    }
    big.resize(70000, 'A');
    check_all("long70000_at0", big, 0, false);
    check_all("long70000_at5", big, 5, false);

    // lengths that do not fit saturate instead of wrapping (the plan refuses them; nothing is written)
    {
        const Row r("abcd", 3);
        FnParams P{};
        std::string bad;
        P.a = (int64_t)1 << 62;  // 4 * 2^62 == 2^64
        if (out_len<TF_REPEAT>(P, r.p, r.len, nullptr, 0) != LEN_SATURATED) bad += " 4x2^62";
        P.a = INT64_MAX;
        if (out_len<TF_REPEAT>(P, r.p, r.len, nullptr, 0) != LEN_SATURATED) bad += " 4xmax";
        P.a = ((int64_t)1 << 61) - 1;  // fits: 2^63 - 4
        if (out_len<TF_REPEAT>(P, r.p, r.len, nullptr, 0) != (1ULL << 63) - 4) bad += " fits";
        const Row e("", 0);
        P.a = INT64_MAX;
        if (out_len<TF_REPEAT>(P, e.p, e.len, nullptr, 0) != 0) bad += " empty";
        report("repeat", "saturates", bad);
        bad.clear();
        for (int side = SIDE_LEFT; side <= SIDE_BOTH; side++) {
            P.a = INT64_MAX, P.flags = side, P.fill = ' ';
            if (out_len<TF_PAD>(P, r.p, r.len, nullptr, 0) != (uint64_t)INT64_MAX) bad += " max";  // margin + row: no wrap
        }
        if (sat_add(~0ULL - 1, 2) != LEN_SATURATED || sat_add(~0ULL - 1, 1) != ~0ULL || sat_mul(1ULL << 32, 1ULL << 32) != LEN_SATURATED ||
            sat_mul(1ULL << 32, (1ULL << 32) - 1) != ((1ULL << 32) - 1) << 32 || sat_mul(0, ~0ULL) != 0)
            bad += " sat";
        report("pad", "saturates", bad);
    }

    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
