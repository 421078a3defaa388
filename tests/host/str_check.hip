// Runs the per-string functions of csrc/str_dev.hpp on the CPU and compares each with a naive
// byte loop over a column of edge strings (tests/test_str_check.py checks every line): the same
// functions the device kernels inline, compiled for the host.  No GPU and no HIP runtime call.
//
// The column's byte buffer is a heap block of exactly the bytes rounded up to 8, and every
// pattern lies in a block of its own of that kind: the least the functions' contract allows (an
// 8-aligned start; the aligned word of the last byte readable), so that a build with
// -fsanitize=address reports any read before the first or after the last such word.
//
// stdout: one line per case, `<function> <case> ok` or `<function> <case> FAIL ...`; the last
// line is `cases <n> failed <m>`.  Exit status 1 when a case failed.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "str_dev.hpp"

using namespace vh::str;

static int g_cases = 0, g_failed = 0;
static void report(const char *fn, const std::string &name, bool ok, const std::string &more = "") {
    g_cases++;
    if (!ok) g_failed++;
    std::printf("%s %s %s%s%s\n", fn, name.c_str(), ok ? "ok" : "FAIL", more.empty() ? "" : " ", more.c_str());
}

// a block with the contract's least size holding s
static uint8_t *block(const std::string &s) {
    const size_t sz = (s.size() + 7) / 8 * 8;
    uint8_t *b = static_cast<uint8_t *>(std::malloc(sz));
    if (sz) std::memset(b, 0xAB, sz);  // what follows the string must not matter
    if (!s.empty()) std::memcpy(b, s.data(), s.size());
    return b;
}

// ---- the naive side ---------------------------------------------------------------------------
static uint64_t naive_word(const uint8_t *p, uint64_t len, uint64_t k) {
    uint64_t w = 0;
    for (uint64_t j = 0; j < 8 && 8 * k + j < len; j++) w |= (uint64_t)p[8 * k + j] << (8 * j);
    return w;
}
static uint64_t naive_hash(const uint8_t *p, uint64_t len, uint64_t seed) {
    const uint64_t sk = seed_key(seed);
    uint64_t sum = 0;
    for (uint64_t k = 0; 8 * k < len; k++) sum += hash_term(naive_word(p, len, k), k, sk);
    return hash_finish(sum, len, sk);
}
static uint64_t naive_codepoints(const uint8_t *p, uint64_t len) {
    uint64_t n = 0;
    for (uint64_t i = 0; i < len; i++) n += (p[i] & 0xC0) != 0x80;
    return n;
}
static int64_t naive_find(const uint8_t *p, uint64_t len, const uint8_t *pat, uint64_t m) {
    for (uint64_t i = 0; i + m <= len; i++) {
        uint64_t j = 0;
        while (j < m && p[i + j] == pat[j]) j++;
        if (j == m) return (int64_t)i;
    }
    return -1;
}
static bool naive_match(int op, const uint8_t *p, uint64_t len, const uint8_t *pat, uint64_t m) {
    bool eq = len == m;
    for (uint64_t i = 0; eq && i < m; i++) eq = p[i] == pat[i];
    bool sw = len >= m, ew = len >= m;
    for (uint64_t i = 0; sw && i < m; i++) sw = p[i] == pat[i];
    for (uint64_t i = 0; ew && i < m; i++) ew = p[len - m + i] == pat[i];
    switch (op) {
    case OP_EQ: return eq;
    case OP_NE: return !eq;
    case OP_STARTSWITH: return sw;
    case OP_ENDSWITH: return ew;
    default: return naive_find(p, len, pat, m) >= 0;
    }
}

int main() {
    // ---- the edge strings ------------------------------------------------------------------------
    std::vector<std::string> strs;
    std::vector<std::string> names;
    size_t cur = 0;
    auto add = [&](const std::string &s, const std::string &name) {
        strs.push_back(s);
        names.push_back(name);
        cur += s.size();
    };
    // lengths 0 .. 17 at every start alignment 0 .. 7 (a filler string moves the start)
    for (int L = 0; L <= 17; L++)
        for (int a = 0; a < 8; a++) {
            const size_t pad = (a + 8 - cur % 8) % 8;
            if (pad) add(std::string(pad, 'f'), "filler");
            std::string s(L, 0);
            for (int i = 0; i < L; i++) s[i] = (char)((i * 7 + L * 13 + a) & 0xff);  // NUL and high bytes occur
            add(s, "len" + std::to_string(L) + "_at" + std::to_string(a));
        }
    add("a", "prefix_a");
    add("ab", "prefix_ab");
    add(std::string("a\0", 2), "prefix_a_nul");
    add(std::string("a\0b", 3), "prefix_a_nul_b");
    add(std::string("\0\0\0", 3), "nuls");
    add("\xc3\xa9", "utf8_2");
    add("\xe2\x82\xac", "utf8_3");
    add("\xf0\x9d\x84\x9e", "utf8_4");
    add("a\xc3\xa9\xe2\x82\xac\xf0\x9d\x84\x9ez", "utf8_mixed");
    add("aaab", "aaab");
    add("xxaab", "ends_aab");
    {
        std::string big(70000, 0);
        for (size_t i = 0; i < big.size(); i++) big[i] = (char)('a' + (i * 31 + i / 251) % 26);
        add(big, "long70000");
        big[69999] ^= 1;
        add(big, "long70000_last_differs");
    }
    for (int r = 0; r < 4; r++) {
        std::string s(300 + r, 0);
        for (size_t i = 0; i < s.size(); i++) s[i] = (char)('A' + (i + r) % 50);
        add(s, "len" + std::to_string(300 + r));
    }
    add("", "empty_last");

    std::string all;
    std::vector<uint64_t> off{0};
    for (const auto &s : strs) {
        all += s;
        off.push_back(all.size());
    }
    uint8_t *buf = block(all);
    const size_t n = strs.size();

    // ---- load_word, hash, code points ------------------------------------------------------------
    for (size_t i = 0; i < n; i++) {
        const uint8_t *p = buf + off[i];
        const uint64_t len = off[i + 1] - off[i];
        const std::string name = std::to_string(i) + "_" + names[i];
        bool ok = true;
        for (uint64_t k = 0; 8 * k < len; k++) ok = ok && load_word(p, len, k) == naive_word(p, len, k);
        report("load_word", name, ok);
        ok = true;
        for (uint64_t seed = 0; seed < 3; seed++) ok = ok && hash(p, len, seed) == naive_hash(p, len, seed);
        report("hash", name, ok);
        const uint64_t cp = count_codepoints(p, len), want = naive_codepoints(p, len);
        report("count_codepoints", name, cp == want, cp == want ? "" : std::to_string(cp) + " != " + std::to_string(want));
    }
    report("slot_key", "full", slot_key(~0ULL, 64) != ~0ULL && slot_key(5, 64) == 5);
    report("slot_key", "bits0", slot_key(0x1234, 0) == 0);
    report("slot_key", "bits4", slot_key(0x1234, 4) == 4);

    // ---- equality: every pair of equal length (the long ones against each other only) -------------
    for (size_t i = 0; i < n; i++) {
        const uint64_t len = off[i + 1] - off[i];
        bool ok = true;
        for (size_t j = 0; j < n; j++) {
            if (off[j + 1] - off[j] != len) continue;
            const bool want = std::memcmp(buf + off[i], buf + off[j], len) == 0;
            ok = ok && equal(buf + off[i], buf + off[j], len) == want;
        }
        report("equal", std::to_string(i) + "_" + names[i], ok);
    }

    // ---- find / match against literal patterns ----------------------------------------------------
    std::vector<std::pair<std::string, std::string>> pats = {
        {"empty", ""}, {"a", "a"}, {"ab", "ab"}, {"aab", "aab"}, {"nul", std::string("\0", 1)},
        {"a_nul", std::string("a\0", 2)}, {"utf8_2", "\xc3\xa9"}, {"utf8_cont", "\x82\xac"}, {"f7", "fffffff"},
        {"nine", std::string(strs[8 * 9 + 9 + 3].empty() ? "x" : strs[8 * 9 + 9 + 3])},
    };
    {
        const std::string &big = strs[n - 7];  // long70000
        pats.push_back({"long_tail1024", big.substr(big.size() - 1024)});
        pats.push_back({"long_head1024", big.substr(0, 1024)});
        pats.push_back({"long_mid17", big.substr(35000, 17)});
    }
    for (const auto &pp : pats) {
        uint8_t *pat = block(pp.second);
        const uint64_t m = pp.second.size();
        bool okf = true;
        bool okm[N_MATCH_OPS] = {true, true, true, true, true};
        for (size_t i = 0; i < n; i++) {
            const uint8_t *p = buf + off[i];
            const uint64_t len = off[i + 1] - off[i];
            okf = okf && find(p, len, pat, m) == naive_find(p, len, pat, m);
            for (int op = 0; op < N_MATCH_OPS; op++) okm[op] = okm[op] && match(op, p, len, pat, m) == naive_match(op, p, len, pat, m);
        }
        report("find", pp.first, okf);
        static const char *opn[N_MATCH_OPS] = {"eq", "ne", "startswith", "endswith", "contains"};
        for (int op = 0; op < N_MATCH_OPS; op++) report("match", std::string(opn[op]) + "_" + pp.first, okm[op]);
        std::free(pat);
    }
    // every string is found in itself, ends at its last byte, and matches itself
    {
        bool ok = true;
        for (size_t i = 0; i < n; i++) {
            const uint64_t len = off[i + 1] - off[i];
            if (len > 1024) continue;
            uint8_t *pat = block(strs[i]);
            for (size_t j = 0; j < n; j++) {
                const uint8_t *p = buf + off[j];
                const uint64_t lj = off[j + 1] - off[j];
                if (lj > 2048) continue;
                for (int op = 0; op < N_MATCH_OPS; op++) ok = ok && match(op, p, lj, pat, len) == naive_match(op, p, lj, pat, len);
            }
            std::free(pat);
        }
        report("match", "all_pairs", ok);
    }
    report("take_needs_wide", "below", !take_needs_wide(false, (1ULL << 31) - 1));
    report("take_needs_wide", "at_2_31", take_needs_wide(false, 1ULL << 31));
    report("take_needs_wide", "wide_input", take_needs_wide(true, 0));

    std::free(buf);
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
