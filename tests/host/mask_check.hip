// Runs the bit arithmetic of csrc/mask_dev.hpp on the CPU and compares it with a naive bit loop
// (tests/test_mask_check.py checks every line): the same functions the kernels of missing.hip
// inline, compiled for the host, driven group by group as the kernels' lanes drive them.  No GPU
// and no HIP runtime call.
//
// Every bitmap is a heap block of exactly (bit_offset + n + 7) / 8 bytes and every mask one of
// exactly n bytes (at least 1), so that a build with -fsanitize=address reports any read or
// write past them.
//
// stdout: one line per case, `<function> <case> ok` or `<function> <case> FAIL ...`; the last
// line is `cases <n> failed <m>`.  Exit status 1 when a case failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "mask_dev.hpp"

using namespace vh::mask;

static int g_cases = 0, g_failed = 0;
static void report(const char *fn, const std::string &name, bool ok) {
    g_cases++;
    if (!ok) g_failed++;
    std::printf("%s %s %s\n", fn, name.c_str(), ok ? "ok" : "FAIL");
}

static uint64_t g_state = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1DULL) >> 33);
}

static uint8_t *alloc(size_t n) { return static_cast<uint8_t *>(std::malloc(n ? n : 1)); }

int main() {
    const uint64_t lengths[] = {0, 1, 7, 8, 9, 63, 64, 65, 2051};
    // the word functions on every byte value
    {
        bool ok = true;
        for (uint32_t v = 0; v < 256; v++) {
            const uint64_t w = expand8(v);
            for (int u = 0; u < 8; u++) ok = ok && ((w >> (8 * u)) & 0xFF) == (((v >> u) & 1) ? 0u : 1u);
            for (uint32_t cnt = 1; cnt <= 8; cnt++) {
                const uint64_t kept = cnt == 8 ? w : (w & ((1ULL << (8 * cnt)) - 1));
                ok = ok && pack8(kept, cnt) == (v & ((1u << cnt) - 1));
            }
            ok = ok && count8(w) == 8u - (uint32_t)__builtin_popcount(v);
        }
        report("expand8", "every_byte", ok);
        // any non-zero byte is missing
        bool nz = true;
        for (int k = 0; k < 2000; k++) {
            uint64_t m = 0;
            uint32_t expect = 0, cnt = 0;
            for (int u = 0; u < 8; u++) {
                const uint32_t r = rnd();
                const uint8_t b = (r & 3) ? 0 : (uint8_t)(((r >> 8) & 0xFF) ? (r >> 8) : 1);
                m |= (uint64_t)b << (8 * u);
                if (b == 0) expect |= 1u << u; else cnt++;
            }
            nz = nz && pack8(m, 8) == expect && count8(m) == cnt;
        }
        report("pack8", "any_nonzero_byte", nz);
    }
    for (uint64_t off = 0; off < 16; off++) {
        for (uint64_t n : lengths) {
            const std::string name = "off" + std::to_string(off) + "_len" + std::to_string(n);
            const size_t nbits = (size_t)((off + n + 7) / 8);
            uint8_t *bits = alloc(nbits);
            for (size_t k = 0; k < nbits; k++) bits[k] = (uint8_t)rnd();
            // naive: row i is missing when bit (off + i) is 0
            uint8_t *expect = alloc(n), *got = alloc(n);
            for (uint64_t i = 0; i < n; i++) expect[i] = ((bits[(off + i) >> 3] >> ((off + i) & 7)) & 1) ? 0 : 1;
            std::memset(got, 0xAB, n ? n : 1);
            for (uint64_t g = 0; g * 8 < n; g++) unpack_group(bits, off, n, g, got);
            report("unpack", name, std::memcmp(expect, got, n) == 0);
            // pack: the naive bitmap of the mask, padding bits 0
            const size_t nout = (size_t)((n + 7) / 8);
            uint8_t *pexpect = alloc(nout), *pgot = alloc(nout);
            std::memset(pexpect, 0, nout ? nout : 1);
            std::memset(pgot, 0xAB, nout ? nout : 1);
            for (uint64_t i = 0; i < n; i++)
                if (!expect[i]) pexpect[i >> 3] |= (uint8_t)(1u << (i & 7));
            for (uint64_t g = 0; g * 8 < n; g++) pack_group(expect, n, g, pgot);
            report("pack", name, std::memcmp(pexpect, pgot, nout) == 0);
            // the round trip: unpack(pack(mask)) at offset 0 is the mask
            uint8_t *back = alloc(n);
            std::memset(back, 0xAB, n ? n : 1);
            for (uint64_t g = 0; g * 8 < n; g++) unpack_group(pgot, 0, n, g, back);
            report("roundtrip", name, std::memcmp(expect, back, n) == 0);
            uint64_t count = 0, naive = 0;
            for (uint64_t g = 0; g * 8 < n; g++) count += count8(load_bytes(expect, g * 8, (uint32_t)(n - g * 8 < 8 ? n - g * 8 : 8)));
            for (uint64_t i = 0; i < n; i++) naive += expect[i];
            report("count", name, count == naive);
            std::free(bits); std::free(expect); std::free(got); std::free(pexpect); std::free(pgot); std::free(back);
        }
    }
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
