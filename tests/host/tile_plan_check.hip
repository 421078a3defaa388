// Check program of the tiled engine's host planner (vaex_amd/csrc/tile_plan.hpp): no kernels
// of its own, no HIP runtime call.  It walks a matrix of plans (pointers are made-up addresses,
// never dereferenced) through the planner's three stages and prints one line per case with
// every field, which tests/test_tile_plan.py compares with tests/golden/tile_plan_cases.txt
// (recorded from the decision code before it was split out of tiled.hip).
//   tile_plan_check           print the cases; every accepted case is also checked against the
//                             kernel / plan invariant on its own
//   tile_plan_check resolve   every pass-A / pass-B descriptor the matrix produced resolves to a
//                             kernel of libvaexhip.so (addresses only; nothing is launched)
//   tile_plan_check rounds NAME=ROWS ...   the most rounds a pass-B unit of plan NAME walks over ROWS
//                             rows at occupancy 1..4 (rounds_mode below)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tile_plan.hpp"

using namespace vh;

struct Case {
    std::string name;
    BinPlan plan;
    FusedAggs fa;
    uint64_t n, cells;
    int nd_f64;
    bool rowmask;
    TileSwitches sw;
};

// ---- the records printed (plain values only)
struct Rec1 {
    int nv, val_slot[4], cnt_slot[4], flags_mode, s_log2, T, lds_off[4];
    uint64_t lds_b;
    int vnarrow, vfloat, vsigned, vpacked, vdt[2], sb, vbytes, wide, lds_cap;
    uint64_t lds_a;
    int a_family, a_nd, a_nv, a_sb, a_ct, a_vt, a_mk, a_set, a_vn, a_dt0, a_dt1;
    int b_nv, b_narrow, b_mm, b_pk, b_mg;
    int mm_simple, mm_cnt_nn, mgeneric, mmk, mm_off[4];
};
struct Rec2 {
    uint64_t W, kbat, rows_per_wg, ncw, stream_layout, stream_stride, g_min, max_units, sblocks, bstride;
    uint64_t meta[11];  // hist hist2 toff sstart scap sfill cap fills units brange end
};
struct Rec3 {
    int ok, monotone;
    uint64_t sampled, stride, stotal, h_cap, h_toff, h_scap, h_sstart, nunits, h_units;
};

static uint64_t fnv(const void *p, size_t bytes) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < bytes; i++) h = (h ^ static_cast<const unsigned char *>(p)[i]) * 1099511628211ull;
    return h;
}

// ---- the planner under test
struct Ctx {
    TilePlan tp;
    TileLaunch L;
};
static bool stage1(const Case &c, Ctx &x, Rec1 &r) {
    if (!plan_tiles(c.plan, c.fa, c.n, c.cells, c.nd_f64, c.rowmask, c.sw, x.tp)) return false;
    const TileParams &t = x.tp.tp;
    r = Rec1{};
    r.nv = (int)t.nvals;
    for (int k = 0; k < 4; k++) r.val_slot[k] = t.val_slot[k], r.cnt_slot[k] = t.cnt_slot[k], r.lds_off[k] = (int)x.tp.lds_off[k], r.mm_off[k] = t.mm_off[k];
    r.flags_mode = (int)t.flags_mode, r.s_log2 = (int)t.s_log2, r.T = (int)t.ntiles, r.lds_b = x.tp.lds_b;
    r.vnarrow = (int)t.vnarrow, r.vfloat = (int)t.vfloat, r.vsigned = (int)t.vsigned, r.vpacked = (int)t.vpacked;
    r.vdt[0] = t.vdt[0], r.vdt[1] = t.vdt[1], r.sb = x.tp.sb, r.vbytes = x.tp.vbytes, r.wide = (int)t.wide, r.lds_cap = (int)t.lds_cap, r.lds_a = x.tp.lds_a;
    const PassAKernel &a = x.tp.a;
    r.a_family = a.family, r.a_nd = a.nd, r.a_nv = a.nv, r.a_sb = a.sb, r.a_ct = a.ct, r.a_vt = a.vt, r.a_mk = a.mk;
    r.a_set = a.set, r.a_vn = a.vn, r.a_dt0 = a.dt0, r.a_dt1 = a.dt1;
    r.b_nv = x.tp.b.nv, r.b_narrow = x.tp.b.narrow, r.b_mm = x.tp.b.mm, r.b_pk = x.tp.b.pk, r.b_mg = x.tp.b.mg;
    r.mm_simple = (int)t.mm_simple, r.mm_cnt_nn = (int)t.mm_cnt_nn, r.mgeneric = (int)t.mgeneric, r.mmk = (int)t.mmk;
    return true;
}
static void stage2(const Case &c, Ctx &x, int cus, int occupancy, Rec2 &r) {
    const TileLaunch &L = x.L = plan_launch(x.tp, c.n, cus, occupancy, c.sw);
    const MetaLayout &m = L.meta;
    r = Rec2{L.W, L.kbat, L.rows_per_wg, L.ncw, L.stream_layout, L.stream_layout ? L.stream_stride : 0, L.g_min, L.max_units, L.sblocks, L.bstride,
             {m.hist, m.hist + 8 * x.tp.tp.ntiles, m.toff, m.sstart, m.scap, m.sfill, m.cap, m.fills, m.units, m.brange, m.bytes}};
}
static void stage3(const Case &c, Ctx &x, int cus, const uint64_t *hist, const uint32_t *brange, Rec3 &r) {
    TileRegions reg;
    std::vector<WorkUnit> units;
    r = Rec3{};
    r.monotone = sample_monotone(brange, x.L.sblocks);
    r.ok = size_regions(x.tp, x.L, c.n, hist, brange, reg);
    r.sampled = reg.sampled;
    if (!r.ok) return;
    plan_units(x.tp, x.L, c.n, cus, hist, reg.sampled, units);
    const size_t T = x.tp.tp.ntiles;
    r.stride = reg.stride, r.stotal = reg.stotal;
    r.h_cap = fnv(reg.cap.data(), 4 * T), r.h_toff = fnv(reg.toff.data(), 8 * T);
    r.h_scap = fnv(reg.scap.data(), 4 * T), r.h_sstart = fnv(reg.sstart.data(), 8 * T);
    r.nunits = units.size(), r.h_units = fnv(units.data(), sizeof(WorkUnit) * units.size());
}
static bool resolves(const Ctx &x) { return pass_a_kernel(x.tp.a) && pass_b_kernel(x.tp.b); }
// ---- end of the planner under test

// the kernel / plan invariant, checked here on its own: a non-generic kernel's compiled-in
// column and value types (and the ordinal kernels' SET) are the plan's, a generic kernel over
// anything but float64 scalar binners has ND <= 0 and takes no row mask (its values go through
// the per-dtype dispatch: nothing compiled in to compare)
static bool invariant_holds(const Case &c, const Rec1 &r) {
    if (r.a_family == PassAKernel::GENERIC && r.a_mk) return false;
    if (r.a_family == PassAKernel::FAST && r.a_nd != c.plan.nb) return false;
    if (r.a_family == PassAKernel::ORDINAL && c.plan.nb != 1) return false;
    for (int d = 0; d < c.plan.nb; d++) {
        const BinnerDev &b = c.plan.b[d];
        if (r.a_family == PassAKernel::FAST && (b.kind != 0 || b.dtype != r.a_ct)) return false;
        if (r.a_family == PassAKernel::ORDINAL &&
            !(b.kind == 1 ? b.dtype == VH_I32 && !r.a_set : b.kind == 2 && r.a_set && dtype_itemsize(b.dtype) == 4))
            return false;
        if (r.a_family == PassAKernel::GENERIC && r.a_nd > 0 && (b.kind != 0 || b.dtype != VH_F64)) return false;
    }
    for (int a = 0; a < c.fa.na; a++) {
        const FusedAgg &f = c.fa.a[a];
        if (f.kind == VH_AGG_COUNT || r.a_family == PassAKernel::GENERIC) continue;
        const int want = r.a_family == PassAKernel::FAST ? r.a_vt : (r.val_slot[a] == 0 ? r.a_dt0 : r.a_dt1);
        if (want >= 0 && f.dtype != want) return false;
    }
    return true;
}

static void print1(const Rec1 &r) {
    printf(" nv=%d vs=%d,%d,%d,%d cs=%d,%d,%d,%d fl=%d s=%d T=%d lo=%d,%d,%d,%d lb=%llu vn=%d vf=%d vg=%d vp=%d vdt=%d,%d sb=%d vb=%d wd=%d cap=%d la=%llu"
           " A=%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d B=%d:%d:%d:%d:%d mm=%d,%d,%d,%d mo=%d,%d,%d,%d",
           r.nv, r.val_slot[0], r.val_slot[1], r.val_slot[2], r.val_slot[3], r.cnt_slot[0], r.cnt_slot[1], r.cnt_slot[2], r.cnt_slot[3],
           r.flags_mode, r.s_log2, r.T, r.lds_off[0], r.lds_off[1], r.lds_off[2], r.lds_off[3], (unsigned long long)r.lds_b, r.vnarrow, r.vfloat,
           r.vsigned, r.vpacked, r.vdt[0], r.vdt[1], r.sb, r.vbytes, r.wide, r.lds_cap, (unsigned long long)r.lds_a, r.a_family, r.a_nd, r.a_nv,
           r.a_sb, r.a_ct, r.a_vt, r.a_mk, r.a_set, r.a_vn, r.a_dt0, r.a_dt1, r.b_nv, r.b_narrow, r.b_mm, r.b_pk, r.b_mg, r.mm_simple,
           r.mm_cnt_nn, r.mgeneric, r.mmk, r.mm_off[0], r.mm_off[1], r.mm_off[2], r.mm_off[3]);
}
static void print2(int occ, const Rec2 &r) {
    printf(" | occ%d W=%llu kb=%llu rw=%llu ncw=%llu st=%llu ss=%llu g=%llu mu=%llu sbk=%llu bs=%llu meta=", occ, (unsigned long long)r.W,
           (unsigned long long)r.kbat, (unsigned long long)r.rows_per_wg, (unsigned long long)r.ncw, (unsigned long long)r.stream_layout,
           (unsigned long long)r.stream_stride, (unsigned long long)r.g_min, (unsigned long long)r.max_units, (unsigned long long)r.sblocks,
           (unsigned long long)r.bstride);
    for (int i = 0; i < 11; i++) printf("%s%llu", i ? "," : "", (unsigned long long)r.meta[i]);
}
static void print3(const char *sample, const Rec3 &r) {
    printf(" | %s ok=%d mono=%d smp=%llu", sample, r.ok, r.monotone, (unsigned long long)r.sampled);
    if (r.ok)
        printf(" str=%llu sto=%llu cap=%016llx toff=%016llx scap=%016llx sst=%016llx nu=%llu u=%016llx", (unsigned long long)r.stride,
               (unsigned long long)r.stotal, (unsigned long long)r.h_cap, (unsigned long long)r.h_toff, (unsigned long long)r.h_scap,
               (unsigned long long)r.h_sstart, (unsigned long long)r.nunits, (unsigned long long)r.h_units);
}

// ---- synthetic samples: hist[2 T] and brange[2 sblocks] as k_tile_sample would leave them
static void make_sample(int kind, uint32_t T, uint64_t sblocks, std::vector<uint64_t> &hist, std::vector<uint32_t> &brange) {
    hist.assign(2 * (size_t)T, 0);
    brange.assign(2 * (size_t)sblocks + 2, 0);
    const uint64_t B = TA_BATCH;
    for (uint64_t b = 0; b < sblocks; b++) {
        if (kind == 0 || kind == 1 || kind == 4) {  // shuffled rows: every block over all tiles
            brange[2 * b] = 0, brange[2 * b + 1] = T - 1;
            for (uint32_t t = 0; t < T; t++) {
                uint64_t c = B / T + (t < B % T ? 1 : 0);                 // uniform
                if (kind == 1) c = t == T / 3 ? B / 2 + c / 2 : c / 2;    // one hot tile
                if (kind == 4 && t % 5 == 1) c = 0;                       // tiles the sample missed
                hist[t] += c, hist[T + t] += c * c;
            }
        } else if (kind == 2 || kind == 3) {  // a block in one tile: clustered (2), sorted (3)
            const uint32_t t = kind == 2 ? (uint32_t)((b * 7919u + 13u) % T) : (uint32_t)(b * T / sblocks);
            brange[2 * b] = brange[2 * b + 1] = t;
            hist[t] += B, hist[T + t] += B * B;
        }  // kind 5: an empty sample
    }
}
static const char *const SAMPLES[] = {"uniform", "hot", "clustered", "sorted", "missed", "empty"};

// ---- the matrix
static const void *addr(int column, int align) { return reinterpret_cast<const void *>((uintptr_t)0x100000000ull * (column + 1) + (align == 16 ? 0 : align)); }

static BinnerDev scalar_binner(int dtype, int column, int align = 16) {
    BinnerDev b{};
    b.kind = 0, b.dtype = dtype, b.data = addr(column, align), b.vmin = 0, b.scale = 1, b.bins = 1024, b.stride = 1;
    return b;
}
static FusedAgg agg(int kind, int dtype = VH_F64, int column = -1, int align = 16, uint32_t moment = 0) {
    FusedAgg a{};
    a.kind = kind, a.dtype = dtype, a.moment = moment;
    a.data = column < 0 ? nullptr : static_cast<const double *>(addr(column, align));
    a.vint = kind == VH_AGG_SUM && dtype != VH_F64 && dtype != VH_F32;
    a.grid = const_cast<void *>(addr(40 + column, 16));
    return a;
}
struct AggSet {
    const char *name;
    std::vector<FusedAgg> a;
};
static std::vector<AggSet> agg_sets(int vdt) {  // vdt: the dtype "the" value column has in this plan
    const int V = 20, V2 = 21, V3 = 22;
    return {
        {"count", {agg(VH_AGG_COUNT)}},
        {"count+sum", {agg(VH_AGG_COUNT), agg(VH_AGG_SUM, vdt, V)}},
        {"count+2sum", {agg(VH_AGG_COUNT), agg(VH_AGG_SUM, vdt, V), agg(VH_AGG_SUM, vdt, V2)}},
        {"sumf32", {agg(VH_AGG_SUM, VH_F32, V)}},
        {"sumi8", {agg(VH_AGG_SUM, VH_I8, V)}},
        {"sum+countv", {agg(VH_AGG_SUM, vdt, V), agg(VH_AGG_COUNT, vdt, V)}},
        {"count+countv", {agg(VH_AGG_COUNT), agg(VH_AGG_COUNT, VH_F64, V)}},
        {"min+max", {agg(VH_AGG_MIN, VH_F64, V), agg(VH_AGG_MAX, VH_F64, V)}},
        {"count+sum+min+max", {agg(VH_AGG_COUNT), agg(VH_AGG_SUM, VH_F64, V), agg(VH_AGG_MIN, VH_F64, V), agg(VH_AGG_MAX, VH_F64, V)}},
        {"mini16", {agg(VH_AGG_MIN, VH_I16, V)}},
        {"moment2", {agg(VH_AGG_COUNT), agg(VH_AGG_SUM_MOMENT, VH_F64, V, 16, 2)}},
        {"moment3", {agg(VH_AGG_SUM_MOMENT, VH_F64, V, 16, 3)}},
        {"2sumi8f32", {agg(VH_AGG_SUM, VH_I8, V), agg(VH_AGG_SUM, VH_F32, V2)}},
        {"3sum", {agg(VH_AGG_SUM, VH_F64, V), agg(VH_AGG_SUM, VH_F64, V2), agg(VH_AGG_SUM, VH_F64, V3)}},
    };
}

static Case make_case(const std::string &name, const std::vector<BinnerDev> &bs, const std::vector<FusedAgg> &as, uint64_t n, uint64_t cells) {
    Case c{};
    c.name = name;
    c.plan.nb = (int)bs.size();
    for (size_t d = 0; d < bs.size(); d++) c.plan.b[d] = bs[d];
    c.fa.na = (int)as.size();
    c.nd_f64 = (int)bs.size();
    for (size_t k = 0; k < as.size(); k++) {
        c.fa.a[k] = as[k];
        if (as[k].data && as[k].dtype != VH_F64) c.fa.generic_vals = 1;
    }
    for (const BinnerDev &b : bs)
        if (!(b.kind == 0 && b.dtype == VH_F64 && !b.flip)) c.nd_f64 = 0;  // scalar_f64_dims (binning.hip)
    c.n = n, c.cells = cells, c.rowmask = false;
    return c;
}

static const uint8_t *const MASK = reinterpret_cast<const uint8_t *>(0x7000000000ull);
static const uint64_t CELLS[] = {2 * 4096 - 5, 1027 * 1027, 4096ull * 8192 - 70000, 4096ull * 8192 * 2 + 1};  // T = 2, ~245, ~4090, > 4096
static const uint64_t N = 1ull << 26;

static void build_matrix(std::vector<Case> &out) {
    auto add = [&](Case c) { out.push_back(c); };
    auto with_mask = [&](Case c, int which) {  // 1: every aggregator's mask (the shared-mask retry), 2: the first one's only
        if (which == 1) c.rowmask = true, c.name += "/rowmask";
        if (which == 2) c.fa.a[0].mask = MASK, c.name += "/mask0";
        return c;
    };
    const int bdts[] = {VH_F64, VH_F32, VH_I32, VH_I64, VH_I16};
    const char *bnames[] = {"f64", "f32", "i32", "i64", "i16"};
    // scalar binners x dimensions x aggregator sets x tiles
    for (int bi = 0; bi < 5; bi++)
        for (int nd = 1; nd <= 4; nd++) {
            std::vector<BinnerDev> bs;
            for (int d = 0; d < nd; d++) bs.push_back(scalar_binner(bdts[bi], d));
            for (int vdt : {VH_F64, VH_F32}) {
                const auto sets = agg_sets(vdt);
                for (size_t si = 0; si < sets.size(); si++) {
                    if (vdt == VH_F32 && !(si == 1 || si == 2 || si == 5)) continue;  // sets without "the" value column: once
                    for (int ci = 0; ci < 4; ci++) {
                        // pruned to what the planner reads: dimensions and binner dtypes vary on the count / sum
                        // plans, the other aggregator sets on the 2-d float grids, the tile counts there and on int32
                        if (si > 2 && (nd != 2 || bi > 1)) continue;
                        if (ci != 1 && (nd != 2 || bi > 2 || (si > 1 && si != 7))) continue;
                        Case c = make_case(std::string(bnames[bi]) + "x" + std::to_string(nd) + "/" + sets[si].name + (vdt == VH_F32 ? "f32" : "") + "/c" +
                                               std::to_string(ci), bs, sets[si].a, N, CELLS[ci]);
                        add(c);
                        if (ci == 1 && si <= 1 && nd <= 3 && bi <= 2 && (nd == 2 || si == 1)) add(with_mask(c, 1)), add(with_mask(c, 2));
                    }
                }
            }
        }
    // binner variations of the 2-d count+sum plan: flip, mask, alignment; odd n
    const auto sets = agg_sets(VH_F64);
    for (int bi = 0; bi < 3; bi++) {
        for (int var = 0; var < 6; var++) {
            std::vector<BinnerDev> bs = {scalar_binner(bdts[bi], 0), scalar_binner(bdts[bi], 1, var == 2 ? 8 : var == 3 ? 4 : 16)};
            if (var == 0) bs[1].flip = 1;
            if (var == 1) bs[0].mask = MASK;
            std::vector<FusedAgg> as = sets[1].a;
            if (var == 4) as[1] = agg(VH_AGG_SUM, VH_F64, 20, 8);
            Case c = make_case(std::string(bnames[bi]) + "x2/count+sum/var" + std::to_string(var), bs, as, var == 5 ? N + 1 : N, CELLS[1]);
            add(c);
            add(with_mask(c, 1));
        }
    }
    // ordinal binners: int32, int64, set-ordinal int32 / uint32 / wide
    for (int ob = 0; ob < 5; ob++) {
        BinnerDev b = scalar_binner(ob == 1 ? VH_I64 : ob == 3 ? VH_U32 : VH_I32, 0, 8);
        b.kind = ob >= 2 ? 2 : 1;
        b.ordinal_count = 1000000;
        if (ob == 4) b.set.wide = 1;
        const char *onames[] = {"ord32", "ord64", "set32", "setu32", "setwide"};
        for (int vdt : {VH_F64, VH_F32, VH_I32}) {
            const auto osets = agg_sets(vdt);
            for (size_t si = 0; si < osets.size(); si++) {
                if (vdt != VH_F64 && !(si == 1 || si == 2 || si == 5)) continue;
                if (ob != 0 && ob != 2 && (si > 1 || vdt != VH_F64)) continue;  // int64 / uint32 / wide keys: count / sum only
                if (ob == 2 && vdt == VH_I32) continue;
                for (int ci = 1; ci < 3; ci++) {
                    if (ci == 2 && (si > 2 || ob != 0)) continue;
                    Case c = make_case(std::string(onames[ob]) + "/" + osets[si].name + (vdt == VH_F32 ? "f32" : vdt == VH_I32 ? "i32" : "") + "/c" +
                                           std::to_string(ci), {b}, osets[si].a, N, CELLS[ci]);
                    add(c);
                    if (ci == 1 && si <= 2 && (ob == 0 || ob == 2)) add(with_mask(c, 1)), add(with_mask(c, 2));
                }
            }
        }
    }
    // each switch off in turn (and the wide bits, a stream pad) on plans it bears on.  VH_TILE_ROWMASK
    // is not the planner's: try_tiled_impl reads it before it strips the shared mask
    const struct { const char *plan; int sw; } picks[] = {
        {"f64x2/count+sum/c1", 3}, {"f64x2/count+sum/c1", 5}, {"f64x2/count+sum/c1", 6}, {"f64x2/count+sum/c1", 7},
        {"f32x2/count+2sumf32/c1", 1}, {"f32x2/count+2sumf32/c1", 2}, {"f32x2/count+2sumf32/c1", 3}, {"f32x2/count+2sumf32/c1", 4},
        {"f32x2/count+sumf32/c1", 1}, {"i32x2/count/c1", 1}, {"i32x2/count/c1", 5}, {"f64x2/count+sum/c1/rowmask", 5},
        {"ord32/count+2sumf32/c1", 2}, {"ord32/count+2sumf32/c1", 4}, {"ord32/2sumi8f32/c1", 2}, {"ord32/2sumi8f32/c1", 4}};
    const size_t base = out.size();
    for (const auto &pk : picks)
        for (size_t i = 0; i < base; i++) {
            if (out[i].name != pk.plan) continue;
            Case o = out[i];
            const int s = pk.sw;
            if (s == 1) o.sw.f32 = false;
            if (s == 2) o.sw.narrow = false;
            if (s == 3) o.sw.stream = false;
            if (s == 4) o.sw.pack = false;
            if (s == 5) o.sw.wide = 0;
            if (s == 6) o.sw.wide = 3;
            if (s == 7) o.sw.wgpad = 1001;
            o.name += "/sw" + std::to_string(s);
            add(o);
        }
}

// plans that go on to stage 3, and the row counts that reach the spill shrink and the position limit
static bool stage3_pick(const std::string &n) {
    return n == "f64x2/count+sum/c1" || n == "f64x2/count/c1" || n == "f64x2/count+countv/c1" || n == "f64x2/count+sum/c1/sw3" ||
           n == "f32x2/count+sumf32/c2" || n == "ord32/count+sum/c1" || n == "f64x2/count+sum/c0";
}

// ---- rounds mode: the plans of tests/test_gpu_stream_rounds.py (tests/stream_rounds_cases.py names
// them and gives each its row count).  A sample of cold tiles -- every tile but three hot ones holds
// about half of the n / (4 cus) rows at which plan_units starts to split a tile -- goes through stages 1-3 at
// occupancy 1..4, and the most rounds a unit walks (max_unit_rounds) is printed per occupancy, with
// whether pass A's workgroups differ in their commit counts (the tile table's empty tail rows).
static void make_cold_sample(uint32_t T, uint64_t sblocks, int cus, std::vector<uint64_t> &hist, std::vector<uint32_t> &brange) {
    hist.assign(2 * (size_t)T, 0);
    brange.assign(2 * (size_t)sblocks + 2, 0);
    const uint64_t B = TA_BATCH, cold = B * 7 / (10 * 4 * (uint64_t)cus);
    const uint32_t h0 = T / 2 - 1;
    for (uint64_t b = 0; b < sblocks; b++) {
        brange[2 * b] = 0, brange[2 * b + 1] = T - 1;
        for (uint32_t t = 0; t < T; t++) {
            const uint64_t c = t >= h0 && t < h0 + 3 ? (B - cold * (T - 3)) / 3 : cold;
            hist[t] += c, hist[T + t] += c * c;
        }
    }
}

static bool rounds_plan(const std::string &name, Case &c) {
    const int V = 20, V2 = 21;
    // 1024^2, 700^2 and 64^3 bins with their edge cells; ~1e6 keys with the sampled range's margin.  700^2: plans
    // of 20 or more LDS bytes per cell have 4096-cell tiles, and past 136 tiles the staging of three batches
    // leaves no room for the wide stream-out, which the stream layout needs
    const uint64_t c2 = 1027 * 1027, c7 = 703 * 703, c3 = 67 * 67 * 67, cg = 1062600;
    std::vector<BinnerDev> f64x2 = {scalar_binner(VH_F64, 0), scalar_binner(VH_F64, 1)};
    std::vector<BinnerDev> f64x3 = {scalar_binner(VH_F64, 0), scalar_binner(VH_F64, 1), scalar_binner(VH_F64, 2)};
    std::vector<BinnerDev> f32x2 = {scalar_binner(VH_F32, 0), scalar_binner(VH_F32, 1)};
    BinnerDev key = scalar_binner(VH_I32, 0, 8);
    key.kind = 1, key.ordinal_count = 1062597;
    const FusedAgg cnt = agg(VH_AGG_COUNT), sum = agg(VH_AGG_SUM, VH_F64, V), sum2 = agg(VH_AGG_SUM, VH_F64, V2);
    const FusedAgg cntv = agg(VH_AGG_COUNT, VH_F64, V), mn = agg(VH_AGG_MIN, VH_F64, V), mx = agg(VH_AGG_MAX, VH_F64, V);
    if (name == "c2") c = make_case(name, f64x2, {cnt, sum}, 0, c2);
    else if (name == "mm_simple") c = make_case(name, f64x2, {cnt, sum, mn, mx}, 0, c7);
    else if (name == "minmax") c = make_case(name, f64x2, {mn, mx}, 0, c2);
    else if (name == "2sum2d") c = make_case(name, f64x2, {cnt, sum, sum2}, 0, c2);
    else if (name == "2sum3d") c = make_case(name, f64x3, {cnt, sum, sum2}, 0, c3);
    else if (name == "var") c = make_case(name, f64x2, {agg(VH_AGG_SUM_MOMENT, VH_F64, V, 16, 2), sum, cntv}, 0, c7);
    else if (name == "moment3") c = make_case(name, f64x2, {cntv, sum, agg(VH_AGG_SUM_MOMENT, VH_F64, V, 16, 3)}, 0, c7);
    else if (name == "f32") c = make_case(name, f32x2, {cnt, agg(VH_AGG_SUM, VH_F32, V)}, 0, c2);
    else if (name == "ord_f64") c = make_case(name, {key}, {sum, cnt}, 0, cg);
    else if (name == "ord_i8f32")  // with the groupby's own count(*): 20 bytes per cell, so half the key range
        c = make_case(name, {key}, {agg(VH_AGG_SUM, VH_I8, V), agg(VH_AGG_SUM, VH_F32, V2), cnt}, 0, cg / 2);
    else if (name == "ord_f64_mask") c = make_case(name, {key}, {sum, cnt}, 0, cg), c.rowmask = true;
    else return false;
    return true;
}

static int rounds_mode(int argc, char **argv) {
    const int cus = 256;
    int bad = 0;
    printf("TB_SEGS=%u ceiling=%llu\n", TB_SEGS, (unsigned long long)(TB_ROUNDS * TB_THREADS / TB_SEGS));
    for (int i = 2; i < argc; i++) {
        const std::string arg = argv[i];
        const size_t eq = arg.find('=');
        Case c;
        if (eq == std::string::npos || !rounds_plan(arg.substr(0, eq), c)) {
            printf("%s unknown\n", arg.c_str());
            bad++;
            continue;
        }
        c.n = strtoull(arg.c_str() + eq + 1, nullptr, 10);
        // try_tiled (tiled.hip): the pair-load kernels tile all rows but the last of an odd n
        if ((c.n & 1) && !c.fa.generic_vals && (c.nd_f64 > 0 || ord_fast_ok(c.plan, c.fa))) c.n--;
        Ctx x;
        Rec1 r1;
        if (!stage1(c, x, r1)) {
            printf("%s -\n", c.name.c_str());
            bad++;
            continue;
        }
        printf("%s n=%llu T=%d sb=%d", c.name.c_str(), (unsigned long long)c.n, r1.T, r1.sb);
        for (int occ = 1; occ <= 4; occ++) {
            Rec2 r2;
            stage2(c, x, cus, occ, r2);
            std::vector<uint64_t> hist;
            std::vector<uint32_t> brange;
            make_cold_sample((uint32_t)r1.T, r2.sblocks, cus, hist, brange);
            TileRegions reg;
            std::vector<WorkUnit> units;
            uint32_t rounds = 0;
            if (size_regions(x.tp, x.L, c.n, hist.data(), brange.data(), reg)) {
                plan_units(x.tp, x.L, c.n, cus, hist.data(), reg.sampled, units);
                rounds = max_unit_rounds(x.L, units);
            }
            // workgroup w takes batches w, w + W, ...: the commit counts of the first and the last differ
            const uint64_t nb = (c.n + TA_BATCH - 1) / TA_BATCH, W = r2.W, sb = (uint64_t)r1.sb;
            const uint64_t last = nb >= W ? (nb - (W - 1) + W - 1) / W : 0;
            const int tail = (r2.kbat + sb - 1) / sb != (last + sb - 1) / sb;
            printf(" | occ%d W=%llu ncw=%llu st=%llu g=%llu rounds=%u tail=%d", occ, (unsigned long long)r2.W, (unsigned long long)r2.ncw,
                   (unsigned long long)r2.stream_layout, (unsigned long long)r2.g_min, rounds, tail);
        }
        printf("\n");
    }
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "rounds") return rounds_mode(argc, argv);
    const bool resolve = argc > 1 && std::string(argv[1]) == "resolve";
    std::vector<Case> cases;
    build_matrix(cases);
    const int cus = 256;
    int bad = 0, nres = 0;
    for (const Case &c : cases) {
        Ctx x;
        Rec1 r1;
        bool ok = false;
        std::string err;
        try {
            ok = stage1(c, x, r1);
        } catch (const std::exception &e) {
            err = e.what();
        }
        if (resolve) {
            if (!ok) continue;
            nres++;
            if (!resolves(x)) printf("unresolved: %s\n", c.name.c_str()), bad++;
            continue;
        }
        printf("%s", c.name.c_str());
        if (!err.empty()) {
            printf(" ERROR %s\n", err.c_str());
            bad++;
            continue;
        }
        if (!ok) {
            printf(" -\n");
            continue;
        }
        print1(r1);
        if (!invariant_holds(c, r1)) printf(" INVARIANT"), bad++;
        // stages 2 and 3 read T, the staging, n and two switches only: three occupancies on a few plans,
        // one on the switch variants, none on the rest
        const bool occs = stage3_pick(c.name) || c.name == "f32x2/count+sumf32/c1" || c.name == "i32x2/count/c1" ||
                          c.name == "f64x3/count+2sum/c1" || c.name == "ord32/count+2sumf32/c1";
        for (int occ : {1, 2, 4}) {
            if (!occs && (occ != 1 || c.name.find("/sw") == std::string::npos)) continue;
            Rec2 r2;
            stage2(c, x, cus, occ, r2);
            print2(occ, r2);
            if (occ == 2 || !stage3_pick(c.name)) continue;
            for (uint64_t n3 : {c.n, (uint64_t)6e10, (uint64_t)5e11}) {
                if (n3 != c.n && occ != 1) continue;
                Case c3 = c;
                c3.n = n3;
                Ctx x3 = x;
                Rec2 r23;
                stage2(c3, x3, cus, occ, r23);
                std::vector<uint64_t> hist;
                std::vector<uint32_t> brange;
                for (int kind = 0; kind < 6; kind++) {
                    if (n3 != c.n && kind != 0 && kind != 2) continue;
                    make_sample(kind, (uint32_t)r1.T, r23.sblocks, hist, brange);
                    Rec3 r3;
                    stage3(c3, x3, cus, hist.data(), brange.data(), r3);
                    print3((std::string(SAMPLES[kind]) + (n3 == c.n ? "" : n3 == (uint64_t)6e10 ? "@6e10" : "@5e11")).c_str(), r3);
                }
            }
        }
        printf("\n");
    }
    if (!resolve) {  // a shared keep mask never reaches a generic kernel, which would not apply it (4-d float64 grids)
        std::vector<BinnerDev> bs;
        for (int d = 0; d < 4; d++) bs.push_back(scalar_binner(VH_F64, d));
        Case c = make_case("f64x4/count+sum/rowmask", bs, agg_sets(VH_F64)[1].a, N, CELLS[1]);
        c.rowmask = true;
        Ctx x;
        Rec1 r1;
        if (stage1(c, x, r1)) fprintf(stderr, "%s: accepted with a row mask\n", c.name.c_str()), bad++;
    }
    if (resolve) printf("%d accepted plans, %d with a descriptor that names no kernel\n", nres, bad);
    return bad ? 1 : 0;
}
