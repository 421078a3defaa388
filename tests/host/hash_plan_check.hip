// Check program of the hash partition's host planner (vaex_amd/csrc/hash_plan.hpp), which
// hashagg.hip and hashset.hip share: no kernels, no HIP runtime call, no link to the library.
// It walks a matrix of sample read-backs through the planner as each engine calls it and
// prints one line per case with every decision, which tests/test_hash_plan.py compares with
// tests/golden/hash_plan_cases.txt (recorded from the two engines' own arithmetic before it
// was moved into the header).  Every accepted case is also checked against the planner's
// invariants on its own: region offsets increase, capacities are multiples of 8 of at most
// rows_per_wg + 8, the units tile [0, W) per bucket without gaps, and the pieces of the meta
// buffers do not overlap.
#include <cstdio>
#include <string>
#include <vector>

#include "hash_plan.hpp"

using namespace vh;

// what differs between the two engines, as they pass it
struct Engine {
    const char *name;
    bool set;            // hashset: a sample over every batch is exact, the estimate is >= 1
    uint64_t sample_blocks;
    double target_keys;
    bool repart;         // hashagg: sub-buckets when P is at its cap
};
static const Engine ENGINES[] = {
    {"ha-wide", false, 256, 2300, true}, {"ha-narrow", false, 256, 4608, true}, {"set", true, 128, 4096, false}};
constexpr uint32_t MAX_P_LOG2 = 11, MAX_SUBS = 64;
constexpr int B_THREADS = 1024;  // pass B / direct workgroup

struct Case {
    std::string name;
    const Engine *eng;
    uint64_t n;
    std::vector<uint64_t> fine;  // [HP_FINE] the sample histogram, then ds, f1, f2
    int cu, bpc;
};

static uint64_t fnv(const void *p, size_t bytes) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < bytes; i++) h = (h ^ static_cast<const unsigned char *>(p)[i]) * 1099511628211ull;
    return h;
}

// every decision of one case, as plain values
struct Out {
    uint64_t sblocks, bstride, sampled;
    double dest;
    uint32_t p_log2;
    uint64_t W, rows_per_wg;  // direct mode when p_log2 == 0
    bool ok;
    uint64_t stride;
    std::vector<uint32_t> cap;
    std::vector<uint64_t> toff;
    std::vector<HashUnit> units;
    uint64_t meta[5];  // toff units cap fills end
    uint32_t S_sub;
    uint64_t total2;
    std::vector<uint64_t> rbase, toff2;
    std::vector<uint32_t> rcap, cap2;
    std::vector<HashUnit> units_b;
    uint64_t meta2[7];  // rbase toff2 units rcap cap2 fills2 end
};

// ---- the planner under test
static void plan_case(const Case &c, Out &o) {
    const Engine &e = *c.eng;
    const uint64_t *fh = c.fine.data();
    const HashSampleGeom sg = hash_sample_geom(c.n, e.sample_blocks);
    o.sblocks = sg.sblocks, o.bstride = sg.bstride;
    o.sampled = hash_sampled_rows(fh);
    o.dest = hash_estimate_keys(o.sampled, (double)fh[HP_FINE], (double)fh[HP_FINE + 1], (double)fh[HP_FINE + 2], c.n,
                                e.set && sg.sblocks == sg.nbatch, e.set);
    o.p_log2 = hash_p_log2(o.dest, e.target_keys, MAX_P_LOG2);
    o.ok = true;
    o.S_sub = 1;
    if (o.p_log2 == 0) {
        const HashDirect d = hash_plan_direct(c.n, c.cu, c.bpc, B_THREADS);
        o.W = d.W, o.rows_per_wg = d.rows_per_wg;
        return;
    }
    const std::vector<uint64_t> bh = hash_fold_fine(fh, o.p_log2);
    HashPlan pl;
    o.ok = hash_plan_partition(c.n, c.cu, c.bpc, o.p_log2, bh, o.sampled, pl);
    o.W = pl.W, o.rows_per_wg = pl.rows_per_wg, o.stride = pl.stride;
    if (!o.ok) return;
    o.cap = pl.cap, o.toff = pl.toff, o.units = pl.units;
    const HashMetaLayout &m = pl.meta;
    const uint64_t meta[5] = {m.toff, m.units, m.cap, m.fills, m.bytes};
    for (int i = 0; i < 5; i++) o.meta[i] = meta[i];
    if (e.repart) o.S_sub = hash_repart_subs(o.dest, o.p_log2, MAX_P_LOG2, e.target_keys, MAX_SUBS);
    if (o.S_sub > 1) {
        HashRepart rp;
        hash_plan_repart(c.n, pl, bh, o.sampled, o.S_sub, rp);
        o.total2 = rp.total;
        o.rbase = rp.rbase, o.rcap = rp.rcap, o.toff2 = rp.toff2, o.cap2 = rp.cap2, o.units_b = rp.units_b;
        const HashRepartLayout &q = rp.meta;
        const uint64_t meta2[7] = {q.rbase, q.toff2, q.units, q.rcap, q.cap2, q.fills2, q.bytes};
        for (int i = 0; i < 7; i++) o.meta2[i] = meta2[i];
    }
}
// ---- end of the planner under test

// the planner's invariants for an accepted partition, checked here on their own
static const char *broken_invariant(const Out &o) {
    const uint32_t P = 1u << o.p_log2;
    if (o.cap.size() != P || o.toff.size() != P) return "sizes";
    for (uint32_t t = 0; t < P; t++) {
        if (t && !(o.toff[t] > o.toff[t - 1])) return "toff not increasing";
        if (t && o.toff[t] != o.toff[t - 1] + o.cap[t - 1]) return "regions overlap or leave a gap";
        if (o.cap[t] % 8 || o.cap[t] > o.rows_per_wg + 8) return "cap";
    }
    if (o.toff[P - 1] + o.cap[P - 1] != o.stride) return "stride";
    size_t k = 0;
    for (uint32_t t = 0; t < P; t++) {  // the units of bucket t, in order, tile [0, W)
        uint32_t w = 0;
        for (; k < o.units.size() && o.units[k].bucket == t; k++) {
            if (o.units[k].w_begin != w || o.units[k].w_end <= w) return "units leave a gap or are empty";
            w = o.units[k].w_end;
        }
        if (w != o.W) return "units do not reach W";
    }
    if (k != o.units.size()) return "units out of bucket order";
    const uint64_t size[4] = {8ull * P, sizeof(HashUnit) * o.units.size(), 4ull * P, 4ull * P * o.W};
    for (int i = 0; i < 4; i++)
        if (o.meta[i] + size[i] > o.meta[i + 1]) return "meta pieces overlap";
    if (o.meta[0] % 8 || o.meta[1] % 4 || o.meta[2] % 4 || o.meta[3] % 4) return "meta alignment";
    if (o.S_sub > 1) {
        const uint64_t U = o.units.size(), P2 = U * o.S_sub;
        if (o.units_b.size() != P2 || o.toff2.size() != P2 || o.cap2.size() != P2) return "repart sizes";
        for (uint64_t g = 0; g < P2; g++) {
            if (g && o.toff2[g] != o.toff2[g - 1] + o.cap2[g - 1]) return "sub-regions overlap or leave a gap";
            if (o.cap2[g] % 8) return "cap2";
            if (o.units_b[g].bucket != g || o.units_b[g].w_begin != 0 || o.units_b[g].w_end != 1) return "units_b";
        }
        if (o.toff2[P2 - 1] + o.cap2[P2 - 1] != o.total2) return "total2";
        const uint64_t size2[6] = {8 * U, 8 * P2, sizeof(HashUnit) * P2, 4 * U, 4 * P2, 4 * P2};
        for (int i = 0; i < 6; i++)
            if (o.meta2[i] + size2[i] > o.meta2[i + 1]) return "meta2 pieces overlap";
    }
    return nullptr;
}

static void print_case(const Case &c, const Out &o) {
    printf("%s sb=%llu bs=%llu smp=%llu dest=%.17g p=%u W=%llu rw=%llu", c.name.c_str(), (unsigned long long)o.sblocks,
           (unsigned long long)o.bstride, (unsigned long long)o.sampled, o.dest, o.p_log2, (unsigned long long)o.W,
           (unsigned long long)o.rows_per_wg);
    if (o.p_log2 == 0) {
        printf(" direct\n");
        return;
    }
    if (!o.ok) {
        printf(" str=%llu refused: region table too large\n", (unsigned long long)o.stride);
        return;
    }
    printf(" str=%llu cap=%016llx toff=%016llx nu=%llu u=%016llx meta=", (unsigned long long)o.stride,
           (unsigned long long)fnv(o.cap.data(), 4 * o.cap.size()), (unsigned long long)fnv(o.toff.data(), 8 * o.toff.size()),
           (unsigned long long)o.units.size(), (unsigned long long)fnv(o.units.data(), sizeof(HashUnit) * o.units.size()));
    for (int i = 0; i < 5; i++) printf("%s%llu", i ? "," : "", (unsigned long long)o.meta[i]);
    // the first, a middle and the last region and unit in full
    const size_t P = o.cap.size(), nu = o.units.size();
    for (size_t t : {size_t(0), P / 2, P - 1}) printf(" r%zu=%llu+%u", t, (unsigned long long)o.toff[t], o.cap[t]);
    for (size_t k : {size_t(0), nu / 2, nu - 1}) printf(" u%zu=%u:%u-%u", k, o.units[k].bucket, o.units[k].w_begin, o.units[k].w_end);
    if (c.eng->repart) printf(" S=%u", o.S_sub);
    if (o.S_sub > 1) {
        printf(" tot2=%llu rbase=%016llx rcap=%016llx toff2=%016llx cap2=%016llx ub=%016llx meta2=", (unsigned long long)o.total2,
               (unsigned long long)fnv(o.rbase.data(), 8 * o.rbase.size()), (unsigned long long)fnv(o.rcap.data(), 4 * o.rcap.size()),
               (unsigned long long)fnv(o.toff2.data(), 8 * o.toff2.size()), (unsigned long long)fnv(o.cap2.data(), 4 * o.cap2.size()),
               (unsigned long long)fnv(o.units_b.data(), sizeof(HashUnit) * o.units_b.size()));
        for (int i = 0; i < 7; i++) printf("%s%llu", i ? "," : "", (unsigned long long)o.meta2[i]);
    }
    printf("\n");
}

// ---- the matrix
// sample histograms as k_*_sample would leave them: `sampled` rows over the fine bins
static const char *const HISTS[] = {"uniform", "gaps", "hot"};
static std::vector<uint64_t> make_fine(int kind, uint64_t sampled) {
    std::vector<uint64_t> f(HP_FINE + 3, 0);
    uint64_t left = sampled;
    if (kind == 2) {  // one fine bin holds nine tenths of the rows
        f[1234] = sampled - sampled / 10;
        left = sampled / 10;
    }
    // kind 1: a third of the 64 top-level hash ranges saw no row (whole buckets empty at P >= 64)
    uint32_t live = 0;
    for (uint32_t i = 0; i < HP_FINE; i++) live += !(kind == 1 && (i >> 6) % 3 == 1);
    uint32_t k = 0;
    for (uint32_t i = 0; i < HP_FINE; i++) {
        if (kind == 1 && (i >> 6) % 3 == 1) continue;
        f[i] += left / live + (k < left % live ? 1 : 0);
        k++;
    }
    return f;
}

// the sample's distinct keys and the keys seen once / twice: which estimate comes out
struct Est {
    const char *name;
    uint64_t ds, f1, f2;
};
static const Est ESTS[] = {
    {"few", 100, 10, 5},                 // 110 keys: p_log2 = 0
    {"p1", 5000, 0, 0},                  // f2 == 0 without singletons: ds itself, p_log2 = 1 (2 at the wide target)
    {"p1w", 4000, 0, 0},                 // p_log2 = 1 at the wide target, 0 at the others
    {"f2zero", 1000, 1000, 0},           // f2 == 0: ds + f1 (f1 - 1) / 2 = 500500, above a small n
    {"cap", 1000000, 400000, 20000},     // 5e6 keys: p_log2 at its cap, no repartition
    {"mid", 1000000, 500000, 10000},     // 1.35e7 keys: a few sub-buckets
    {"huge", 1000000, 900000, 1000},     // 4e8 keys: above most n (clamped); 64 sub-buckets at n = 2^30
};

static void build_matrix(std::vector<Case> &out) {
    const uint64_t NS[] = {1, 7, 4095, 4096, 4097, 1000000, 1ull << 30};
    const int CUS[] = {1, 256}, BPCS[] = {1, 4, 9};
    for (const Engine &e : ENGINES)
        for (uint64_t n : NS)
            for (const Est &est : ESTS)
                for (int hk = 0; hk < 3; hk++)
                    for (int cu : CUS)
                        for (int bpc : BPCS)
                            for (int part = 0; part < 3; part++) {
                                // part 0: the sample's blocks reach every row; 1: a tenth of them are not regular keys
                                // (masked / NaN rows of a set chunk: fewer sampled than n); 2: a sample of a larger chunk
                                const uint64_t reach = std::min<uint64_t>(n, e.sample_blocks * HP_BATCH);
                                if (part == 2 && reach == n) continue;
                                if (part != 2 && reach < n) continue;
                                if (part == 1 && !e.set) continue;
                                // pruned to what bears on the decision: the geometry varies on the large chunks, the
                                // histogram where there is more than one bucket to fill
                                const bool big = n >= 1000000;
                                const std::string en = est.name;
                                // small chunks: the sample geometry and the clamp to n, at two geometries
                                if (!big && !((cu == 256 && bpc == 4) || (cu == 1 && bpc == 1 && n >= 4095))) continue;
                                if (!big && (hk != 0 || !(en == "few" || en == "huge"))) continue;
                                // large chunks: every cu x bpc on the two largest estimates with a uniform histogram,
                                // and on the hot bucket at 2^30 rows; the other histograms at the largest estimate only
                                const bool geom = cu == 256 && bpc == 4;
                                if (big && !geom && !((en == "huge" || en == "cap") && hk == 0) && !(en == "huge" && hk == 2 && n > 1000000))
                                    continue;
                                if (big && hk != 0 && en != "huge") continue;
                                const uint64_t sampled = part == 1 ? reach - reach / 10 : reach;
                                Case c;
                                c.eng = &e, c.n = n, c.cu = cu, c.bpc = bpc;
                                c.fine = make_fine(hk, sampled);
                                c.fine[HP_FINE] = est.ds, c.fine[HP_FINE + 1] = est.f1, c.fine[HP_FINE + 2] = est.f2;
                                c.name = std::string(e.name) + "/n" + std::to_string(n) + "/" + est.name + "/" + HISTS[hk] + "/cu" +
                                         std::to_string(cu) + "x" + std::to_string(bpc) + (part == 1 ? "/masked" : part == 2 ? "/partial" : "/all");
                                out.push_back(c);
                            }
}

int main() {
    const HashSampleLayout sl = hash_sample_layout();
    printf("sample-layout skeys=%llu scnt=%llu fine=%llu stats=%llu bytes=%llu\n", (unsigned long long)sl.skeys,
           (unsigned long long)sl.scnt, (unsigned long long)sl.fine, (unsigned long long)sl.stats, (unsigned long long)sl.bytes);
    int bad = sl.skeys + 8 * HP_SAMPLE_SLOTS > sl.scnt || sl.scnt + 4 * HP_SAMPLE_SLOTS > sl.fine || sl.fine + 8 * HP_FINE > sl.stats ||
              sl.stats + 64 > sl.bytes;
    std::vector<Case> cases;
    build_matrix(cases);
    for (const Case &c : cases) {
        Out o{};
        plan_case(c, o);
        print_case(c, o);
        if (o.p_log2 == 0 || !o.ok) continue;
        if (const char *why = broken_invariant(o)) fprintf(stderr, "%s: INVARIANT %s\n", c.name.c_str(), why), bad++;
    }
    return bad ? 1 : 0;
}
