// Host plan of the hash partition shared by hashagg.hip (fused groupby) and hashset.hip
// (ordered set): sample a chunk's keys, estimate its distinct keys, pick P = 2^p hash buckets,
// size the per-(pass-A workgroup, bucket) regions and cut pass B into work units.  Plain
// arithmetic: no HIP runtime call, no environment, no statics -- numbers and vectors in,
// structs out (tests/host/hash_plan_check.hip walks it without a GPU).  What differs between
// the two engines (sample blocks, target keys per bucket, the estimate's clamps) is an argument.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

namespace vh {

constexpr uint64_t HP_SAMPLE_SLOTS = 1ull << 21;  // the sample's HBM key table
constexpr uint32_t HP_FINE_LOG2 = 12;             // sample histogram: top 12 bits of the key hash
constexpr uint32_t HP_FINE = 1u << HP_FINE_LOG2;
constexpr uint64_t HP_BATCH = 4096;               // rows of a pass-A batch (512 lanes x 8 rows)
constexpr uint64_t HP_DEST_OVER = 0x80000000u;    // region offsets stay below this bit (pass A flags with it)

// pass-B work unit: bucket `bucket`, the regions of pass-A workgroups [w_begin, w_end)
struct HashUnit {
    uint32_t bucket, w_begin, w_end, pad;
};

// ---- sample -------------------------------------------------------------------------------
// sample buffer: skeys u64[slots] | scnt u32[slots] | fine u64[FINE] | stats (64 bytes)
struct HashSampleLayout {
    uint64_t skeys, scnt, fine, stats, bytes;  // byte offsets; scnt .. end is zeroed, skeys set to EMPTY
};
inline HashSampleLayout hash_sample_layout() {
    constexpr uint64_t S = HP_SAMPLE_SLOTS;
    return {0, 8 * S, 12 * S, 12 * S + 8 * HP_FINE, 12 * S + 8 * HP_FINE + 64};
}

struct HashSampleGeom {
    uint64_t nbatch, sblocks, bstride;  // batches of the chunk; sample workgroups; their seed stride
};
inline HashSampleGeom hash_sample_geom(uint64_t n, uint64_t sample_blocks) {
    const uint64_t nbatch = (n + HP_BATCH - 1) / HP_BATCH, sblocks = std::min<uint64_t>(nbatch, sample_blocks);
    return {nbatch, sblocks, std::max<uint64_t>(HP_BATCH, n / sblocks)};
}

// rows the sample histogram counted
inline uint64_t hash_sampled_rows(const uint64_t *fine) { return std::accumulate(fine, fine + HP_FINE, uint64_t(0)); }

// Distinct keys of the chunk from the sample's `ds` distinct keys, of which f1 were seen once
// and f2 twice (Chao1); exact when every row was sampled.  whole_chunk: the caller's sample
// blocks covered every batch, which it takes as exact too (hashset; hashagg passes false).
// at_least_one: clamp the estimate to >= 1 (hashset; hashagg passes false).
inline double hash_estimate_keys(uint64_t sampled, double ds, double f1, double f2, uint64_t n, bool whole_chunk,
                                 bool at_least_one) {
    double dest;
    if (sampled >= n || whole_chunk) dest = ds;  // every row sampled: exact
    else dest = f2 > 0 ? ds + f1 * f1 / (2 * f2) : ds + f1 * (f1 - 1) / 2;  // Chao1
    if (at_least_one) dest = std::max(dest, 1.0);
    return std::min<double>(dest, (double)n);
}

// P = 2^p_log2 buckets of about target_keys keys each, p_log2 <= max_p_log2
inline uint32_t hash_p_log2(double dest, double target_keys, uint32_t max_p_log2) {
    uint32_t p_log2 = 0;
    while (p_log2 < max_p_log2 && dest / (double)(1u << p_log2) > target_keys) p_log2++;
    return p_log2;
}

// the fine histogram folded into P buckets
inline std::vector<uint64_t> hash_fold_fine(const uint64_t *fine, uint32_t p_log2) {
    std::vector<uint64_t> bh(size_t(1) << p_log2, 0);
    for (uint32_t i = 0; i < HP_FINE; i++) bh[i >> (HP_FINE_LOG2 - p_log2)] += fine[i];
    return bh;
}

// ---- direct mode (P == 1): one LDS table per workgroup over a contiguous row range ---------
struct HashDirect {
    uint64_t W, rows_per_wg;
};
inline HashDirect hash_plan_direct(uint64_t n, int cu, int bpc, int threads) {
    const uint64_t W = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)cu * bpc, (n + 4 * threads - 1) / (4 * threads)));
    return {W, (n + W - 1) / W};
}

// ---- pass A / pass B ------------------------------------------------------------------------
// meta buffer: toff u64[P] | units HashUnit[nunits] | cap u32[P] | fills u32[P][W]
struct HashMetaLayout {
    uint64_t toff, units, cap, fills, bytes;
};

struct HashPlan {
    uint32_t p_log2 = 0, P = 1, W = 0;
    uint64_t rows_per_wg = 0;
    uint64_t stride = 0;         // entries of one pass-A workgroup's regions
    std::vector<uint32_t> cap;   // [P] region capacity
    std::vector<uint64_t> toff;  // [P] region offset inside a workgroup's stride
    std::vector<HashUnit> units;
    HashMetaLayout meta{};
};

// bpc: resident pass-A workgroups per CU (occupancy query); bh: hash_fold_fine.  Returns false
// when the region table is too large for 31-bit region offsets (the caller refuses the update).
inline bool hash_plan_partition(uint64_t n, int cu, int bpc, uint32_t p_log2, const std::vector<uint64_t> &bh, uint64_t sampled,
                                HashPlan &pl) {
    const uint32_t P = 1u << p_log2;
    pl.p_log2 = p_log2;
    pl.P = P;
    const uint32_t W = pl.W = std::min<uint32_t>(1024, (uint32_t)cu * std::min(bpc, 4));
    // pass-A workgroup w takes batches w, w + W, ...: at most ceil(batches / W) of them
    const uint64_t nbatch = (n + HP_BATCH - 1) / HP_BATCH;
    const uint64_t rows_per_wg = pl.rows_per_wg = (nbatch + W - 1) / W * HP_BATCH;
    pl.cap.resize(P);
    pl.toff.resize(P);
    uint64_t stride = 0;
    for (uint32_t t = 0; t < P; t++) {
        const double e = (double)rows_per_wg * (double)bh[t] / (double)std::max<uint64_t>(sampled, 1);
        uint64_t c = (uint64_t)(e * 1.04 + 6.0 * std::sqrt(e + 1.0)) + 32;
        c = std::min<uint64_t>((c + 7) & ~uint64_t(7), rows_per_wg + 8);
        pl.cap[t] = (uint32_t)c;
        pl.toff[t] = stride;
        stride += c;
    }
    pl.stride = stride;
    if (stride + rows_per_wg >= HP_DEST_OVER) return false;
    // pass-B units: a unit merges each of its keys into the HBM table once, so split a bucket
    // over ranges of workgroups only as far as the CUs need work
    pl.units.clear();
    const double target = std::max(1.0, (double)n / ((double)cu * 2));
    for (uint32_t t = 0; t < P; t++) {
        const double e = (double)n * (double)bh[t] / (double)std::max<uint64_t>(sampled, 1);
        const uint32_t gq = (uint32_t)std::min<double>(W, std::max(1.0, std::ceil(e / target)));
        for (uint32_t k = 0; k < gq; k++)
            pl.units.push_back({t, (uint32_t)((uint64_t)W * k / gq), (uint32_t)((uint64_t)W * (k + 1) / gq), 0});
    }
    const uint64_t o_units = 8 * (uint64_t)P, o_cap = o_units + sizeof(HashUnit) * pl.units.size(), o_fills = o_cap + 4 * (uint64_t)P;
    pl.meta = {0, o_units, o_cap, o_fills, o_fills + 4 * (uint64_t)P * W + 256};
    return true;
}

// ---- hashagg's repartition: more keys per bucket than an LDS table holds (P at its cap) ------
// sub-buckets per pass-B unit (1: no repartition)
inline uint32_t hash_repart_subs(double dest, uint32_t p_log2, uint32_t max_p_log2, double target_keys, uint32_t max_subs) {
    const double kpb = dest / (double)(1u << p_log2);
    if (p_log2 != max_p_log2 || !(kpb > target_keys * 1.25)) return 1;
    return std::min<uint32_t>(max_subs, (uint32_t)std::ceil(kpb / target_keys));
}

// meta buffer: rbase u64[U] | toff2 u64[P2] | units HashUnit[P2] | rcap u32[U] | cap2 u32[P2] | fills2 u32[P2]
struct HashRepartLayout {
    uint64_t rbase, toff2, units, rcap, cap2, fills2, bytes;
};

// every unit of `pl` scatters its entries into S_sub sub-bucket regions of rcap[unit] entries
// from rbase[unit]; pass B then runs over the P2 = U * S_sub regions as buckets of one
// "workgroup" (W = 1, stride 0): units_b[i] = {i, 0, 1}
struct HashRepart {
    uint32_t S_sub = 1;
    uint64_t total = 0;  // entries of all sub-bucket regions
    std::vector<uint64_t> rbase, toff2;
    std::vector<uint32_t> rcap, cap2;
    std::vector<HashUnit> units_b;
    HashRepartLayout meta{};
};
inline void hash_plan_repart(uint64_t n, const HashPlan &pl, const std::vector<uint64_t> &bh, uint64_t sampled, uint32_t S_sub,
                             HashRepart &rp) {
    const uint32_t U = (uint32_t)pl.units.size();
    rp.S_sub = S_sub;
    rp.rbase.resize(U);
    rp.rcap.resize(U);
    uint64_t total2 = 0;
    for (uint32_t ui = 0; ui < U; ui++) {
        const HashUnit &un = pl.units[ui];
        // the unit's entries: at most its regions' capacities; expected ~ n p_b * share
        const double e = (double)n * (double)bh[un.bucket] / (double)std::max<uint64_t>(sampled, 1) *
                         (double)(un.w_end - un.w_begin) / (double)pl.W;
        const double es = e / S_sub;
        uint64_t c = (uint64_t)(es * 1.05 + 8.0 * std::sqrt(es + 1.0)) + 64;
        c = (c + 7) & ~uint64_t(7);
        rp.rcap[ui] = (uint32_t)c;
        rp.rbase[ui] = total2;
        total2 += c * S_sub;
    }
    rp.total = total2;
    const uint64_t P2 = (uint64_t)U * S_sub;
    rp.units_b.resize(P2);
    rp.toff2.resize(P2);
    rp.cap2.resize(P2);
    for (uint32_t ui = 0; ui < U; ui++)
        for (uint32_t q = 0; q < S_sub; q++) {
            const uint64_t gi = (uint64_t)ui * S_sub + q;
            rp.units_b[gi] = {(uint32_t)gi, 0, 1, 0};
            rp.toff2[gi] = rp.rbase[ui] + (uint64_t)q * rp.rcap[ui];
            rp.cap2[gi] = rp.rcap[ui];
        }
    const uint64_t o_toff2 = 8 * (uint64_t)U, o_units = o_toff2 + 8 * P2, o_rcap = o_units + sizeof(HashUnit) * P2;
    const uint64_t o_cap2 = o_rcap + 4 * (uint64_t)U, o_fills2 = o_cap2 + 4 * P2;
    rp.meta = {0, o_toff2, o_units, o_rcap, o_cap2, o_fills2, o_fills2 + 4 * P2 + 256};
}

}  // namespace vh
