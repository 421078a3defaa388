// Host planner of the tiled engine (tiled.hip): which kernels a plan takes and how its
// scratch is laid out, as plain arithmetic -- no HIP runtime calls, no environment, no
// statics -- so every decision can be exercised without a GPU (tests/host/tile_plan_check.hip).
//   stage 1  plan_tiles    plan + aggregators + switches -> TilePlan (slots, tiles, LDS, kernels)
//   stage 2  plan_launch   + CU count and pass A's occupancy -> TileLaunch (grid, meta layout)
//   stage 3  size_regions / plan_units   + the sample -> region capacities, pass-B work units
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "engine.hpp"

namespace vh {

#ifndef VH_TA_THREADS
#define VH_TA_THREADS 512
#endif
#ifndef VH_TA_RPT
#define VH_TA_RPT 8
#endif
#ifndef VH_TB_THREADS
#define VH_TB_THREADS 1024
#endif
#ifndef VH_TILE_LDS_KB
#define VH_TILE_LDS_KB 96
#endif
constexpr int TA_THREADS = VH_TA_THREADS;
constexpr int TA_RPT = VH_TA_RPT;
constexpr int TA_BATCH = TA_THREADS * TA_RPT;
constexpr int TB_THREADS = VH_TB_THREADS;
constexpr uint64_t TILE_LDS_BUDGET = VH_TILE_LDS_KB * 1024;
constexpr uint32_t TILE_MAX_TILES = 4096;
constexpr size_t LDS_MAX_BYTES = 160 * 1024;  // per workgroup on gfx950
constexpr int TA_WG_PER_CU = 4;
constexpr int SAMPLE_BLOCKS = 512;
// stream layout: a pass-B unit walks its (workgroup, commit) segments in rounds of TB_SEGS (two per
// thread), at most TB_ROUNDS * TB_THREADS segments per unit (a cold tile's single unit would walk
// all W x ncw segments in one workgroup): TB_ROUNDS * TB_THREADS / TB_SEGS rounds at the most
#ifndef VH_TB_ROUNDS
#define VH_TB_ROUNDS 6
#endif
constexpr uint64_t TB_ROUNDS = VH_TB_ROUNDS;
constexpr uint32_t TB_SEGS = 2 * TB_THREADS;

enum : int32_t { CNT_ALWAYS = -2, CNT_FLAG = -1 };

// local cell of a padding entry (tiles hold at most 2^15 cells when runs are padded)
constexpr uint32_t DUMMY_CELL = 0xffffu;
constexpr uint32_t DEST_OVERFLOW = 0x80000000u;  // | tile: region and spill full, global atomics
constexpr uint32_t DEST_SPILL = 0x40000000u;     // | entry of the spill areas

struct WorkUnit { uint32_t tile, w_begin, w_end, pad; };

__host__ __device__ inline bool is_minmax(int kind) { return kind == VH_AGG_MIN || kind == VH_AGG_MAX; }
// 4-byte LDS cells for min / max of <= 4-byte columns (ds_min/max_i32 / _u32: half the LDS
// of the 64-bit form, and 32-bit LDS atomics): signed as int32, unsigned as uint32, float32
// as order-preserving bits
__host__ __device__ inline bool mm_cell32(int dt) {
    return dt == VH_F32 || dt == VH_I32 || dt == VH_U32 || dt == VH_I16 || dt == VH_U16 || dt == VH_I8 || dt == VH_U8;
}

// LDS bytes of the generic pass A (must match scatter_lds)
__host__ __device__ inline size_t scatter_lds_bytes(int nv, uint32_t T) {
    return (size_t)8 * nv * TA_BATCH + (size_t)8 * TA_BATCH + 24 * (size_t)T + 64;
}

// rows per thread of one commit of the fast f64 pass A: with sums, SB batches are ranked
// into one commit, so each (workgroup, tile) run is SB times longer (fewer, longer region
// stores; the kernel already runs one workgroup per CU on registers)
#ifndef VH_TA_SB
#define VH_TA_SB 3
#endif
#ifndef VH_TA_SB0
#define VH_TA_SB0 2  // count-only commits (same-process A/B: 1 -> 2 is 3.99 -> 3.87 ms, 3 is 4.08)
#endif
__host__ __device__ constexpr int fast_sb(int nv) { return nv == 0 ? VH_TA_SB0 : nv == 1 ? VH_TA_SB : (VH_TA_SB < 2 ? VH_TA_SB : 2); }
// the 3-d f64 pass A carries a third binner column: fewer batches per commit keep its
// registers out of scratch memory (three batches of one value slot spilled 17 VGPRs)
__host__ __device__ constexpr int fast_sb_nd(int nv, int nd) {
    return nd < 3 ? fast_sb(nv) : nv >= 2 ? 1 : (fast_sb(nv) < 2 ? fast_sb(nv) : 2);
}
// narrow (4-byte) value slots staged as 4 bytes: two carried columns still fit three batches
__host__ __device__ constexpr int fast_sb_narrow(int nv) { return nv == 0 ? VH_TA_SB0 : VH_TA_SB; }

// LDS of the fast kernels: staged values (vbytes each: 8, or 4 for narrow slots) | staged
// 4-byte keys | tile arrays
__host__ __device__ inline size_t fast_lds_bytes(int nv, uint32_t T, uint32_t cap, int vbytes = 8) {
    return (size_t)vbytes * nv * cap + (size_t)4 * cap + 24 * (size_t)T + 64;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// In the stream layout pass A is queued before the sample comes back, so what toff and cap
// point at is not yet uploaded while it runs (stale scratch of an earlier call), and the fills
// its epilogue derives from them mean nothing: the stream layout reads none of the three
// (scatter_lds_init and pass B go by tp.stream and the table).
struct TileParams {
    uint32_t s_log2, ntiles, flags_mode, nvals;
    uint64_t cells;
    uint32_t W;                // pass-A workgroups
    uint32_t pad;
    uint64_t rows_per_wg;      // upper bound (region sizing): batches of a workgroup x TA_BATCH
    uint64_t wg_stride;        // entries of one workgroup's regions
    const uint32_t *cap;       // [T]
    const uint64_t *toff;      // [T] region offset inside a workgroup's block
    uint32_t *fills;           // [T][W] entries produced (may exceed cap)
    // spill areas: rows past their (workgroup, tile) region go to their tile's spill area
    // (one atomic reservation per tile and commit), read by pass B like one more region;
    // past the spill area too (should not happen): global atomics
    uint32_t *spill_fill;         // [T] entries reserved (may exceed spill_cap)
    const uint32_t *spill_cap;    // [T]
    const uint64_t *spill_start;  // [T] entry index of the area, relative to spill_base
    uint64_t spill_base;          // first entry of the spill areas (after the W regions)
    void *entries;             // u16 / u32, W * wg_stride
    double *values[2];         // per value slot, W * wg_stride
    int32_t val_slot[MAX_FUSED_AGGS];  // sum agg k -> value slot
    int32_t cnt_slot[MAX_FUSED_AGGS];  // count agg k -> CNT_ALWAYS / CNT_FLAG / value slot
    const double *vdata[2];    // value slot -> source column (fast kernel)
    uint32_t debug;            // experiment switches (VH_TILE_DEBUG), ablation build only (DBG)
    // 4-byte value slots (every summed column <= 4 bytes: int8/16/32, uint8/16/32, bool,
    // float32 -- exact): slot s is float32 bits when bit s of vfloat is set, else the low 32
    // bits of the int64 slot, sign-extended back when bit s of vsigned is set
    uint32_t vnarrow, vfloat, vsigned;
    // two narrow slots in one array: values[0] holds, per 8 entries, their 8 slot-0 values then
    // their 8 slot-1 values (the narrow ordinal pass A with two carried columns: one write
    // stream, not two; pass B still reads each slot as 32 contiguous bytes)
    uint32_t vpacked;
    int32_t vdt[2];            // value slot -> column dtype (fast ordinal kernel)
    // min / max aggregator k: pass B flushes its LDS cells with native global atomics into
    // mmtmp[k] (cells x 4 or 8 bytes of the LDS cell form, identity-filled), merged into the
    // typed grid afterwards by k_mm_merge (a CAS per cell on 1- and 2-byte grids serialised
    // on the shared words)
    void *mmtmp[MAX_FUSED_AGGS];
    // pass B with min / max / moment: mgeneric, a moment other than 2 (per-entry form); mmk, bit
    // k set when aggregator k is a min / max (its cells are read ahead of each chunk)
    uint32_t mgeneric, mmk;
    // wide stream-out of the fast kernels (batch_commit_fast): every (workgroup, tile) run of
    // a commit is padded to a multiple of 8 entries with DUMMY_CELL entries, so runs start
    // 8-aligned in the region and a lane stores 8 cells / 2 float64 values / 4 narrow slots
    // per 16-byte store; pass B skips the dummies.  lds_cap: staged entries per value slot
    uint32_t wide, lds_cap;
    // min / max pass B on one float64 value slot with at most one count, sum, min and max
    // aggregator of it (no moments, no integer sums): a branch-light entry loop (mm_simple);
    // LDS byte offsets of the count / sum / min / max cells (-1: absent), the count keyed on
    // the slot's non-NaN values (mm_cnt_nn) or on every entry
    uint32_t mm_simple, mm_cnt_nn;
    int32_t mm_off[4];
    // stream layout of the fast kernels (stream = 1): each pass-A workgroup appends every
    // commit's padded, tile-sorted entries to ONE contiguous stream (w * wg_stride on), instead
    // of T private per-tile regions, and records where each tile's run of the commit starts:
    // tab[(w * (T + 1) + t) * ncw + c] = stream offset of tile t's run of commit c (row T: the
    // commit's end; commits past a workgroup's last: its final offset, i.e. empty runs).  Pass B
    // gathers a tile's (workgroup, commit) segments through the table.  256-512 write streams
    // instead of T x W regions: the region pattern's cost and its dependence on where the
    // scratch lands in HBM (r05: 6.2-7.4 ms for one C2 pass A) go away (scripts/bw_probe6.hip)
    uint32_t stream, ncw;
    uint32_t *tab;
    // one keep mask shared by every aggregator (a selection or filter; 1 = keep) applied by the
    // fast pass A per row: masked rows are dropped before the exchange (MK instantiations)
    const uint8_t *rowmask;
    // host-image mirror (pass B's epilogue): image[k] is the device-side address of aggregator
    // k's registered page-locked host image, null when it is not mirrored.  Every unit of tile
    // t draws a ticket from tickets[t] (zeroed per launch) after its flush; the unit that draws
    // tile_units[t] - 1 is the tile's last and copies the tile's finished cells from the device
    // grid to the images.  tickets null: no aggregator of the launch is mirrored
    void *image[MAX_FUSED_AGGS];
    uint32_t *tickets;           // [T]
    const uint32_t *tile_units;  // [T] units planned for the tile
};

// The VH_TILE_* environment switches (A/B runs), read on every call by tiled.hip
struct TileSwitches {
    // VH_TILE_<NAME>=0 turns one off: ROWMASK, a shared keep mask on the MK kernels; F32, the float32 /
    // mixed / integer fast kernels; NARROW, 4-byte value slots; STREAM, the stream layout; PACK, two
    // narrow slots in one array
    bool rowmask = true, f32 = true, narrow = true, stream = true, pack = true;
    bool host_image = true;  // VH_HOST_IMAGE=0: pass B mirrors no tile into a registered host image
    uint32_t wide = 7;    // VH_TILE_WIDE: bit 0 wide stream-out, bit 1 / 2 non-temporal cell / value stores
    uint64_t wgpad = 0;   // VH_TILE_WGPAD: extra entries between the workgroups' streams
    uint32_t debug = 0;   // VH_TILE_DEBUG (ablation build only)
};

// One pass-A instantiation.  pass_a_kernel() (tiled.hip) turns it into the kernel's address.
struct PassAKernel {
    enum Family { GENERIC, FAST, ORDINAL };
    // GENERIC  k_tile_scatter<ND, NV>: any plan.  ND > 0: float64 scalar binners read as float64;
    //          0: per-dimension dispatch; -1: the per-row form of plans with a set-ordinal binner
    // FAST     k_tile_scatter_f64<ND, NV, SB, CT, MK, VT>: scalar binners of type ct, values of vt
    // ORDINAL  k_tile_scatter_ord<NV, SB, SET, DT0, DT1, VN, MK>: one 4-byte (set-)ordinal binner;
    //          dt0 / dt1: the slots' dtypes compiled in (VH_ORD_COMBOS), -1: read at run time
    Family family = GENERIC;
    int nd = 0, nv = 0, sb = 1, ct = VH_F64, vt = VH_F64, dt0 = VH_F64, dt1 = VH_F64;
    bool mk = false, set = false, vn = false;
    // the timing scope of the launch (bench.py and scripts/ read these names)
    const char *scope() const {
        if (family == GENERIC) return "tile_scatter";
        if (family == ORDINAL) return set ? "tile_scatter_set" : "tile_scatter_ord";
        if (ct == VH_I32 || ct == VH_I64) return "tile_scatter_int";
        return ct != vt ? "tile_scatter_mixed" : ct == VH_F32 ? "tile_scatter_f32" : "tile_scatter_f64";
    }
};
const void *pass_a_kernel(const PassAKernel &k);  // tiled.hip; nullptr: no such instantiation

// One pass-B instantiation: k_tile_reduce<NV, NARROW, MM, PK, MG>
struct PassBKernel { int nv = 0; bool narrow = false, mm = false, pk = false, mg = false; };
const void *pass_b_kernel(const PassBKernel &k);

// Stage 1's result.  tp: the kernel parameters a plan fixes (slots, tiles, value-slot forms, wide,
// lds_cap, pass B's min / max fields); the executor adds the launch's and the scratch pointers
struct TilePlan {
    TileParams tp;
    uint32_t lds_off[MAX_FUSED_AGGS];  // pass B: byte offset of agg k's cells in the LDS tile
    uint64_t lds_a, lds_b;             // pass A's / pass B's LDS bytes
    int sb, vbytes;                    // pass A's staging: batches per commit, bytes per staged value
    PassAKernel a;
    PassBKernel b;
};

// the fast ordinal pass A applies: one native int32 BinnerOrdinal (or a 4-byte set-ordinal
// binner) without mask, every value column aligned for pair loads, no aggregator masks, no
// counts of columns that are not summed
inline bool ord_fast_ok(const BinPlan &plan, const FusedAggs &fa) {
    if (plan.nb != 1) return false;
    const BinnerDev &b = plan.b[0];
    const bool set_ok = b.kind == 2 && (b.dtype == VH_I32 || b.dtype == VH_U32) && !b.set.wide;
    if (!(b.kind == 1 && b.dtype == VH_I32) && !set_ok) return false;
    if (b.flip || b.mask || (reinterpret_cast<uintptr_t>(b.data) & 7)) return false;
    for (int k = 0; k < fa.na; k++) {
        const FusedAgg &a = fa.a[k];
        if (a.mask) return false;
        if (a.kind != VH_AGG_COUNT) {
            // any native value dtype; pair loads need 2 x itemsize alignment
            if (!a.data) return false;
            const int isz = a.dtype == VH_F64 ? 16 : 2 * dtype_itemsize(a.dtype);
            if (reinterpret_cast<uintptr_t>(a.data) % isz) return false;
        } else if (a.data) {
            bool keyed = false;  // count(v) of a summed column rides on that sum's value
            for (int j = 0; j < fa.na; j++)
                if (fa.a[j].kind != VH_AGG_COUNT && fa.a[j].data == a.data) keyed = true;
            if (!keyed) return false;
        }
    }
    return true;
}

// The ordinal kernels' compiled-in value dtypes X(dt0, dt1, has a narrow kernel), in match order
// (h2o's int8 / float32 sums; else the run-time switch, -1), for the planner here and the lookup
// in tiled.hip.  Set-ordinal kernels: float64 and -1 only.  Below two slots DT1 is VH_F64.
#define VH_ORD_COMBOS(X)                                                                            \
    X(VH_F64, VH_F64, 0) X(VH_I8, VH_I8, 1) X(VH_I8, VH_F32, 1) X(VH_F32, VH_I8, 1) X(VH_F32, VH_F32, 1) \
    X(VH_I32, VH_I32, 1) X(VH_I32, VH_F64, 0) X(VH_F32, VH_F64, 0) X(-1, -1, 1)
inline void ord_value_types(int nv, bool set, bool vn, int raw0, int raw1, int &dt0, int &dt1) {
    dt0 = dt1 = -1;
#define VH_ORD(a, b, narrow) \
    if (dt0 < 0 && (a) >= 0 && (!set || (a) == VH_F64) && (!vn || narrow) && raw0 == (a) && (nv < 2 || raw1 == (b))) dt0 = (a), dt1 = nv < 2 ? VH_F64 : (b);
    VH_ORD_COMBOS(VH_ORD)
#undef VH_ORD
}

// The invariant between a plan and the pass-A kernel chosen for it: a kernel reads columns as
// the types compiled into it, so a mismatch reads out of bounds.  Never a launch.
inline void check_pass_a(const BinPlan &plan, const FusedAggs &fa, const TilePlan &pl) {
    const PassAKernel &k = pl.a;
    const bool fast = k.family == PassAKernel::FAST, generic = k.family == PassAKernel::GENERIC;
    auto bad = [](const char *what) { fail(VH_ERR_RUNTIME, std::string("tiled binning: pass-A kernel does not match the plan: ") + what); };
    for (int d = 0; d < plan.nb; d++) {
        const BinnerDev &b = plan.b[d];
        if (fast && (b.kind != 0 || b.dtype != k.ct || b.mask || b.flip)) bad("binner column type");
        if (generic && k.nd > 0 && (b.kind != 0 || b.dtype != VH_F64)) bad("generic ND > 0 over a non-float64 binner");
        if (!fast && !generic && !(b.kind == 1 ? b.dtype == VH_I32 && !k.set : b.kind == 2 && k.set && dtype_itemsize(b.dtype) == 4))
            bad("ordinal binner");
    }
    if (!generic && (fast ? k.nd != plan.nb : plan.nb != 1)) bad("dimensions");
    if (k.nv != (int)pl.tp.nvals) bad("value slots");
    if (generic && k.mk) bad("row mask on a generic kernel");
    for (int a = 0; a < fa.na && !generic; a++) {
        if (fa.a[a].mask) bad("aggregator mask");
        if (fa.a[a].kind == VH_AGG_COUNT) continue;
        const int want = fast ? k.vt : (pl.tp.val_slot[a] == 0 ? k.dt0 : k.dt1);
        if (want >= 0 && fa.a[a].dtype != want) bad("value column type");
        if (k.vn && dtype_itemsize(fa.a[a].dtype) > 4) bad("narrow slots over a wide column");
    }
}

// ---- stage 1: slots, tiles, LDS and kernels.  false: the plan is not eligible (the caller
// falls back to the global-atomic path).  rowmask: the aggregators' shared keep mask was taken
// off them and is applied per row by an MK kernel (try_tiled_impl).
inline bool plan_tiles(const BinPlan &plan, const FusedAggs &fa, uint64_t n, uint64_t cells, int nd_f64, bool rowmask,
                       const TileSwitches &sw, TilePlan &out) {
    out = TilePlan{};
    TileParams &tp = out.tp;
    // carried values: one slot per distinct value column (sum / min / max of one column share
    // it: same data, mask, dtype and integer-sum encoding); counts keyed on a matching value
    int nv = 0;
    for (int k = 0; k < fa.na; k++) {
        tp.val_slot[k] = -1;
        tp.cnt_slot[k] = CNT_ALWAYS;
        if (fa.a[k].kind == VH_AGG_COUNT) continue;
        for (int j = 0; j < k && tp.val_slot[k] < 0; j++)
            if (tp.val_slot[j] >= 0 && same_value_slot(fa.a[j], fa.a[k])) tp.val_slot[k] = tp.val_slot[j];
        if (tp.val_slot[k] < 0) tp.val_slot[k] = nv++;
    }
    if (nv > 2) return false;
    tp.nvals = nv, tp.cells = cells, tp.vdt[0] = tp.vdt[1] = VH_F64;
    bool flags_mode = false;
    for (int k = 0; k < fa.na; k++) {
        const FusedAgg &a = fa.a[k];
        if (a.kind != VH_AGG_COUNT || (!a.data && !a.mask)) continue;
        if (!a.mask && a.dtype != VH_F64 && a.dtype != VH_F32) continue;  // integers: never NaN
        tp.cnt_slot[k] = CNT_FLAG;
        for (int j = 0; j < fa.na; j++)
            if (fa.a[j].kind != VH_AGG_COUNT && fa.a[j].data == a.data && fa.a[j].mask == a.mask && a.data && !fa.a[j].vint)
                tp.cnt_slot[k] = tp.val_slot[j];
        if (tp.cnt_slot[k] == CNT_FLAG) flags_mode = true;
    }
    if (flags_mode)
        for (int k = 0; k < fa.na; k++)
            if (fa.a[k].kind == VH_AGG_COUNT) tp.cnt_slot[k] = CNT_FLAG;
    tp.flags_mode = flags_mode ? 1 : 0;
    // LDS bytes per cell of pass B: u32 counts, 8-byte sums, min / max 4 or 8 (mm_cell32)
    auto cell_bytes = [](const FusedAgg &a) -> uint64_t { return a.kind == VH_AGG_COUNT || (is_minmax(a.kind) && mm_cell32(a.dtype)) ? 4 : 8; };
    uint64_t per_cell = 0;
    for (int k = 0; k < fa.na; k++) per_cell += cell_bytes(fa.a[k]);
    // pass B's LDS tile: 96 KB for count / sum plans; wider cells (min / max / moment) get up
    // to 128 KB so their tiles keep 4096 cells (fewer tiles: longer pass-A runs per region)
    const uint64_t budget = per_cell > 12 ? std::max<uint64_t>(TILE_LDS_BUDGET, 128 * 1024) : TILE_LDS_BUDGET;
    uint32_t s_log2 = 0;
    while (s_log2 < 16 && ((uint64_t)2 << s_log2) * per_cell <= budget) s_log2++;
    const uint64_t S = 1ull << s_log2;
    const uint64_t T64 = (cells + S - 1) / S;
    if (T64 > TILE_MAX_TILES || T64 < 2) return false;
    const uint32_t T = (uint32_t)T64;
    tp.s_log2 = s_log2, tp.ntiles = T;
    uint64_t off = 0;
    for (int k = 0; k < fa.na; k++) {
        off = (off + 7) & ~uint64_t(7);
        out.lds_off[k] = (uint32_t)off;
        off += S * cell_bytes(fa.a[k]);
    }
    out.lds_b = (off + 15) & ~uint64_t(15);

    // ---- pass A.  The fast float64 kernels: native f64 binners and sums, no masks, 16-byte aligned columns
    bool fast = nd_f64 > 0 && !flags_mode;
    bool has_set = false;
    for (int d = 0; d < plan.nb; d++) has_set = has_set || plan.b[d].kind == 2;
    for (int d = 0; d < plan.nb && fast; d++) fast = !plan.b[d].mask && aligned16(plan.b[d].data);
    for (int k = 0; k < fa.na; k++) {
        if (fa.a[k].mask) fast = false;
        if (fa.a[k].kind != VH_AGG_COUNT) fast = fast && fa.a[k].data && fa.a[k].dtype == VH_F64 && aligned16(fa.a[k].data);
        if (fa.a[k].kind == VH_AGG_COUNT && fa.a[k].data && fa.a[k].dtype != VH_F64) fast = false;
    }
    // the same kernels over other column types: float32 / int32 / int64 scalar binners (one type)
    // without masks, float32 or float64 sums (one type), counts of every row or of a summed column,
    // columns aligned for pair loads, n even.  They replace the generic pass A's per-dimension
    // dispatch (C2 on float32 columns: 11.3 ms, profiles/r06_f32.txt)
    int bt = -1, vt = -1;
    bool typed = false;  // bt binners with vt values have a fast kernel
    if (!fast && !flags_mode && n % 2 == 0 && plan.nb >= 1 && plan.nb <= 3 && sw.f32) {
        bool ok = true;
        for (int d = 0; d < plan.nb; d++) {
            const BinnerDev &b = plan.b[d];
            const int dt = b.dtype;
            ok = ok && b.kind == 0 && (dt == VH_F32 || dt == VH_F64 || dt == VH_I32 || dt == VH_I64) && (bt < 0 || dt == bt) &&
                 !b.flip && !b.mask && (dt == VH_F64 || dt == VH_I64 ? aligned16(b.data) : aligned8(b.data));
            bt = dt;
        }
        for (int k = 0; k < fa.na; k++) {
            const FusedAgg &a = fa.a[k];
            ok = ok && !a.mask;
            if (a.kind == VH_AGG_COUNT) continue;
            ok = ok && a.kind == VH_AGG_SUM && a.data && (a.dtype == VH_F32 || a.dtype == VH_F64) && (vt < 0 || a.dtype == vt) &&
                 (a.dtype == VH_F64 ? aligned16(a.data) : aligned8(a.data));
            vt = a.dtype;
        }
        if (vt < 0) vt = bt;
        for (int k = 0; k < fa.na; k++)  // counts of a column: the summed one (flags_mode otherwise)
            if (fa.a[k].kind == VH_AGG_COUNT && fa.a[k].data) ok = ok && fa.a[k].dtype == vt;
        if (vt == VH_I32 || vt == VH_I64) vt = VH_F64;  // integer binners, no values: the float64 form
        // integer binners: 1- and 2-d only; float64 binners with float64 values are `fast` or generic
        typed = ok && (bt == VH_I32 || bt == VH_I64 ? plan.nb <= 2 : bt == VH_F32 || vt == VH_F32);
    }
    const bool ord = !fast && n % 2 == 0 && ord_fast_ok(plan, fa);
    if (ord)
        for (int k = 0; k < fa.na; k++)
            if (fa.a[k].kind != VH_AGG_COUNT) tp.vdt[tp.val_slot[k]] = fa.a[k].dtype;
    // 4-byte value slots when every summed column of a generic plan is <= 4 bytes (exact)
    bool vnarrow = fa.generic_vals && nv > 0 && !fast && sw.narrow;
    for (int k = 0; k < fa.na && vnarrow; k++) {
        if (fa.a[k].kind == VH_AGG_COUNT) continue;
        const int dt = fa.a[k].dtype, s = tp.val_slot[k];
        if (dtype_itemsize(dt) > 4) vnarrow = false;
        if (dt == VH_F32) tp.vfloat |= 1u << s;
        if (dt == VH_I32 || dt == VH_I16 || dt == VH_I8) tp.vsigned |= 1u << s;
    }
    tp.vnarrow = vnarrow ? 1u : 0u;
    // staging of a commit: several batches when that fits the LDS; the ordinal kernel with
    // narrow slots and the kernels with float32 values stage 4-byte values
    const bool vf32 = typed && vt == VH_F32;
    const int sb_typed = vf32 ? fast_sb_narrow(nv) : fast_sb_nd(nv, plan.nb);
    const bool typed_ok = typed && (nv == 0 || vnarrow == vf32) &&
                          fast_lds_bytes(nv, T, (uint32_t)(sb_typed * TA_BATCH), vf32 ? 4 : 8) <= LDS_MAX_BYTES;
    const bool narrow_ord = !typed_ok && ord && vnarrow &&
                            fast_lds_bytes(nv, T, (uint32_t)(fast_sb_narrow(nv) * TA_BATCH), 4) <= LDS_MAX_BYTES;
    const int sb_f64 = fast_sb_nd(nv, fast ? nd_f64 : 1);
    const bool batched = !typed_ok && (fast || ord) && !narrow_ord &&
                         fast_lds_bytes(nv, T, (uint32_t)(sb_f64 * TA_BATCH)) <= LDS_MAX_BYTES;
    const bool any_fast = typed_ok || fast || ord;
    out.sb = typed_ok ? sb_typed : narrow_ord ? fast_sb_narrow(nv) : batched ? sb_f64 : 1;
    out.vbytes = narrow_ord || (typed_ok && vf32) ? 4 : 8;
    // the kernel.  A plan the fast kernels do not take goes to the generic kernel of its
    // float64 dimensions (cell_of reads them as float64), else to the dispatch (0) or set-
    // ordinal (-1) form: never to an ND > 0 generic kernel over other column types
    PassAKernel &ka = out.a;
    ka.nv = nv;
    const int nd_k = nd_f64 > 0 ? nd_f64 : typed_ok ? plan.nb : (has_set ? -1 : 0);
    if (ord) {
        ka.family = PassAKernel::ORDINAL, ka.set = has_set, ka.mk = rowmask;
        if (rowmask) {  // shared keep mask: int32 key, float64 values (or none), batched commits
            if (has_set || (nv > 0 && !(batched && tp.vdt[0] == VH_F64 && (nv < 2 || tp.vdt[1] == VH_F64)))) return false;
            ka.sb = nv == 0 ? 1 : fast_sb(nv);
        } else {
            ka.vn = narrow_ord && !has_set;
            ka.sb = nv == 0 ? 1 : ka.vn ? fast_sb_narrow(nv) : batched ? fast_sb(nv) : 1;
            ord_value_types(nv, has_set, ka.vn, tp.vdt[0], tp.vdt[1], ka.dt0, ka.dt1);
        }
    } else if (any_fast && nd_k >= 1 && nd_k <= 3) {
        ka.family = PassAKernel::FAST, ka.nd = nd_k, ka.sb = out.sb, ka.mk = rowmask;
        ka.ct = typed_ok ? bt : VH_F64, ka.vt = typed_ok ? vt : VH_F64;
        // a shared keep mask runs only on the batched float64 and the float32 MK kernels
        if (rowmask && !(typed_ok ? bt == VH_F32 && vt == VH_F32 : batched)) return false;
    } else {
        ka.nd = nd_k >= 1 && nd_k <= 3 ? nd_k : nd_k == -1 ? -1 : 0;
        if (rowmask) return false;  // no generic kernel applies a row mask
    }
    // wide stream-out: needs 8 T more staged entries of LDS and tiles below DUMMY_CELL cells
    const uint32_t cap0 = (uint32_t)(out.sb * TA_BATCH);
    const bool wide = (sw.wide & 1) && any_fast && !flags_mode && S < DUMMY_CELL &&
                      fast_lds_bytes(nv, T, cap0 + 8 * T, out.vbytes) <= LDS_MAX_BYTES;
    tp.wide = wide ? sw.wide : 0u;
    tp.lds_cap = wide ? cap0 + 8 * T : cap0;
    out.lds_a = any_fast ? fast_lds_bytes(nv, T, tp.lds_cap, out.vbytes) : scatter_lds_bytes(nv, T);
    if (out.lds_a > LDS_MAX_BYTES) return false;  // very many tiles: the global-atomic path
    tp.vpacked = (out.vbytes == 4 && nv == 2 && !flags_mode && sw.pack) ? 1u : 0u;

    // ---- pass B.  MM: min / max cells or moment terms (the extended run form; a moment other
    // than 2 takes the per-entry form, MG)
    bool mm = false;
    for (int k = 0; k < fa.na; k++) {
        const FusedAgg &a = fa.a[k];
        mm = mm || is_minmax(a.kind) || a.kind == VH_AGG_SUM_MOMENT;
        if (a.kind == VH_AGG_SUM_MOMENT && a.moment != 2) tp.mgeneric = 1;
        if (is_minmax(a.kind)) tp.mmk |= 1u << k;
    }
    // the branch-light form (TileParams::mm_simple): LDS offsets of its count / sum / min / max cells
    bool simple = mm && !tp.mgeneric && nv == 1 && !vnarrow && !flags_mode;
    int *moff = tp.mm_off;
    moff[0] = moff[1] = moff[2] = moff[3] = -1;
    for (int k = 0; k < fa.na && simple; k++) {
        const FusedAgg &a = fa.a[k];
        const int slot = a.kind == VH_AGG_COUNT ? -1 : tp.val_slot[k];
        int r = -1;
        if (a.kind == VH_AGG_COUNT) {
            r = 0;
            if (tp.cnt_slot[k] == 0) tp.mm_cnt_nn = 1;
            else if (tp.cnt_slot[k] != CNT_ALWAYS) simple = false;
        } else if (a.kind == VH_AGG_SUM && !a.vint && a.dtype == VH_F64 && slot == 0) r = 1;
        else if (a.kind == VH_AGG_MIN && a.dtype == VH_F64 && slot == 0) r = 2;
        else if (a.kind == VH_AGG_MAX && a.dtype == VH_F64 && slot == 0) r = 3;
        else simple = false;
        if (r >= 0) {
            if (moff[r] >= 0) simple = false;  // two of one kind
            else moff[r] = (int)out.lds_off[k];
        }
    }
    tp.mm_simple = simple ? 1u : 0u;
    out.b.nv = nv, out.b.pk = nv == 2 && tp.vpacked, out.b.narrow = nv > 0 && (vnarrow || out.b.pk);
    out.b.mm = nv > 0 && mm, out.b.mg = out.b.mm && tp.mgeneric;
    check_pass_a(plan, fa, out);
    return true;
}

// ---- stage 2: pass A's grid, commits and layout, pass B's unit bound, the meta scratch
struct MetaLayout {  // byte offsets into the meta buffer; [T] arrays unless noted
    uint64_t hist;    // [2][T]: rows, and squared per-block rows
    uint64_t toff, sstart, scap, sfill, cap;
    uint64_t fills, units, brange;  // [T][W], [max_units] WorkUnit, [SAMPLE_BLOCKS][2]
    uint64_t bytes;                 // end of the arrays above
    // the host-image mirror's arrays follow them (TileParams::tickets, tile_units), so the
    // offsets above are what they were without the mirror; alloc: the buffer's size
    uint64_t tickets, tunits;
    uint64_t alloc;
};
struct TileLaunch {
    uint32_t W = 0;                             // pass-A workgroups
    uint64_t kbat = 0, rows_per_wg = 0, ncw = 0;  // per workgroup (at most): batches, rows, commits
    bool stream_layout = false;
    uint64_t stream_stride = 0;                 // stream layout: entries of one workgroup's stream
    uint64_t g_min = 1, max_units = 0;          // pass-B units per tile (at least), in all (at most)
    uint64_t sblocks = 0, bstride = 0;          // sample: blocks and their row stride
    MetaLayout meta;
};

inline TileLaunch plan_launch(const TilePlan &pl, uint64_t n, int cus, int blocks_per_cu, const TileSwitches &sw) {
    TileLaunch L;
    const uint32_t T = pl.tp.ntiles;
    const int bpc = std::max(1, std::min(blocks_per_cu, TA_WG_PER_CU));
    const uint32_t W = L.W = std::min<uint32_t>(1024, (uint32_t)cus * bpc);
    const uint64_t nb = (n + TA_BATCH - 1) / TA_BATCH;
    L.kbat = (nb + W - 1) / W;
    L.rows_per_wg = L.kbat * TA_BATCH;
    L.ncw = (L.kbat + pl.sb - 1) / pl.sb;
    // stream layout (TileParams::stream): one exactly sized stream per workgroup.  Count-only plans
    // keep the per-tile regions: their 2-byte entries make a segment's partial lines a large share
    // of pass B's reads (pass B 0.8 -> 1.2 ms), while value-carrying plans gain in pass A (C2
    // count+sum 7.56 -> 6.93 ms, C3 4.68 -> 4.14 ms; scripts/exp_stream.py, profiles/r06_stream.txt)
    L.stream_layout = pl.tp.wide && pl.tp.nvals > 0 && sw.stream && (uint64_t)W * (T + 1) * L.ncw < (1ull << 31);
    L.stream_stride = ((L.rows_per_wg + 7 * L.ncw * T + 8 + 7) & ~uint64_t(7)) + ((sw.wgpad + 7) & ~uint64_t(7));
    const uint64_t wpu = std::max<uint64_t>(1, (uint64_t)TB_THREADS * TB_ROUNDS / std::max<uint64_t>(L.ncw, 1));
    L.g_min = L.stream_layout ? (W + wpu - 1) / wpu : 1;
    // pass-B work units: sum over tiles of max(g_min, ceil(e_t / (n / 4 cu))) <= T g_min + 4 cu
    L.max_units = (uint64_t)T * L.g_min + 4 * (uint64_t)cus + 16;
    L.sblocks = std::min<uint64_t>(nb, SAMPLE_BLOCKS);
    L.bstride = std::max<uint64_t>(TA_BATCH, n / L.sblocks);
    MetaLayout &m = L.meta;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { const uint64_t at = o; o += bytes; return at; };
    m.hist = take(16 * (uint64_t)T);
    m.toff = take(8 * (uint64_t)T);
    m.sstart = take(8 * (uint64_t)T);
    m.scap = take(4 * (uint64_t)T);
    m.sfill = take(4 * (uint64_t)T);
    m.cap = take(4 * (uint64_t)((T + 3) & ~3u));                          // fills and units 16-byte aligned
    m.fills = take(4 * ((uint64_t)T * W + 4 - ((uint64_t)T * W) % 4));
    m.units = take(sizeof(WorkUnit) * L.max_units);
    m.brange = take(8 * (uint64_t)SAMPLE_BLOCKS);
    m.bytes = o;
    o = (o + 15) & ~uint64_t(15);
    m.tickets = take(4 * (uint64_t)T);
    m.tunits = take(4 * (uint64_t)T);
    m.alloc = o;
    return L;
}

// ---- stage 3: the sample sizes pass A's regions and pass B's work units.
// hist[t] / hist[T + t]: rows (and squared per-block rows) of tile t in the sample's blocks;
// brange[2 b], brange[2 b + 1]: first and last tile of sample block b.
// sample_monotone: blocks whose tile ranges follow each other (a column sorted, up or down, along the
// grid index): each workgroup's evenly spaced batches then meet a tile floor or ceil of K p_t
// times, and p_t is exact to a block
inline bool sample_monotone(const uint32_t *brange, uint64_t sblocks) {
    uint64_t up = 0, down = 0;
    for (uint64_t b = 0; b + 1 < sblocks; b++) {
        up += brange[2 * b + 1] > brange[2 * b + 2];  // block b ends past block b + 1's start
        down += brange[2 * b] < brange[2 * b + 3];
    }
    return sblocks > 8 && std::min(up, down) * 100 <= sblocks;
}

struct TileRegions {
    std::vector<uint32_t> cap, scap;      // [T] entries of a workgroup's region / of the tile's spill area
    std::vector<uint64_t> toff, sstart;   // [T] their offsets
    uint64_t stride = 0, stotal = 0, sampled = 0;  // entries of a workgroup's regions / all spill areas; sampled rows
};

// Region capacities per workgroup.  Pass-A workgroup w takes batches w, w + W, w + 2W, ...
// (TA_BATCH rows each), so its tile distribution is the global one whatever the row order (a
// sorted or clustered column would otherwise overflow the regions of a few tiles).  Regions are
// sized for shuffled rows (Poisson spread); rows past a region go to the tile's spill area, sized
// from the spread the sample measures per batch-sized block -- half the tile's expected rows when
// the rows are clustered (each block all in or all out of a tile).  Stream layout: all zero.
// false: not eligible (an empty sample, or regions past pass A's 30-bit positions)
inline bool size_regions(const TilePlan &pl, const TileLaunch &L, uint64_t n, const uint64_t *hist, const uint32_t *brange,
                         TileRegions &r) {
    const uint32_t T = pl.tp.ntiles, W = L.W;
    const uint64_t rows_per_wg = L.rows_per_wg, kbat = L.kbat;
    const bool wide = pl.tp.wide != 0, monotone = sample_monotone(brange, L.sblocks);
    uint64_t sampled = 0;
    for (uint32_t t = 0; t < T; t++) sampled += hist[t];
    r.sampled = sampled;
    if (!sampled) return false;
    // wide stream-out: up to 7 padding entries per (workgroup, tile) and commit
    const uint64_t pad_wg = wide ? 7 * L.ncw : 0;
    r.cap.assign(T, 0), r.scap.assign(T, 0);
    r.toff.assign(T, 0), r.sstart.assign(T, 0);
    uint64_t stride = 0, stotal = 0;
    const double blocks = (double)L.sblocks;  // every sample block is TA_BATCH rows, like a batch
    // clustered rows (block variance well above the Poisson value: each sample block all in
    // or all out of a tile) anywhere in the sample
    bool any_clustered = false;
    for (uint32_t t = 0; t < T; t++) {
        const double m = (double)hist[t] / blocks, var_b = std::max(0.0, (double)hist[T + t] / blocks - m * m);
        any_clustered = any_clustered || var_b > 4.0 * m + 1.0;
    }
    for (uint32_t t = 0; t < T && !L.stream_layout; t++) {
        const double p = (double)hist[t] / (double)sampled, e = (double)rows_per_wg * p;
        const double m = (double)hist[t] / blocks, var_b = std::max(0.0, (double)hist[T + t] / blocks - m * m);
        const bool clustered = var_b > 4.0 * m + 1.0;
        // a clustered tile gets one batch of slack: a workgroup's evenly spaced batches meet a
        // sorted column's tile floor or ceil of K p_t times
        uint64_t c = (uint64_t)(e * 1.04 + 6.0 * std::sqrt(e + 1.0)) + 32 + (clustered ? TA_BATCH : 0) + pad_wg;
        c = std::min<uint64_t>((c + 7) & ~uint64_t(7), rows_per_wg + pad_wg + 8);
        r.cap[t] = (uint32_t)c;
        r.toff[t] = stride;
        stride += c;
        uint64_t sc = (uint64_t)(0.02 * (double)n * p) + TA_BATCH;
        // a tile the sample missed between two clustered sample blocks holds at most the rows
        // between them
        if (any_clustered && hist[t] == 0) sc = std::min<uint64_t>(n, L.bstride) + TA_BATCH;
        if (clustered && !monotone) {
            // whole batches land in a tile: a workgroup's batches in tile t ~ Poisson(K p_hi)
            // (p_hi: p plus two standard errors of a block sample); spill = the expected
            // excess over the region, x 2, for all workgroups (<= 1.25 n p_hi)
            const double p_hi = std::min(1.0, p + 2.0 * std::sqrt(p * (1.0 - p) / blocks));
            const double lam = (double)kbat * p_hi;
            double excess = 0.0, pk = std::exp(-lam);
            for (uint64_t x = 0; x <= kbat && (double)x <= lam + 12.0 * std::sqrt(lam) + 12.0; x++) {
                if (x) pk *= lam / (double)x;
                excess += pk * std::max(0.0, (double)x * TA_BATCH - (double)c);
            }
            sc = (uint64_t)std::min(1.25 * (double)n * p_hi, 2.0 * (double)W * excess) + 4 * TA_BATCH;
        }
        if (wide) sc += sc / 4 + 8 * (uint64_t)W;  // padding of the spilled runs
        r.scap[t] = (uint32_t)std::min<uint64_t>((sc + 7) & ~uint64_t(7), (uint64_t)n + 8 * (uint64_t)W + 8);
        r.sstart[t] = stotal;
        stotal += r.scap[t];
    }
    // pass A keeps region positions in u32 (destination | overflow bit), spill entries below
    // DEST_SPILL
    if (stride + rows_per_wg + pad_wg >= (uint64_t)DEST_SPILL) return false;
    if (stotal >= (uint64_t)DEST_SPILL) {  // very large launches: shrink the spill areas
        const double f = (double)(DEST_SPILL - 8 * (uint64_t)T) / (double)stotal;
        stotal = 0;
        for (uint32_t t = 0; t < T; t++) {
            r.scap[t] = (uint32_t)(((uint64_t)(r.scap[t] * f)) & ~uint64_t(7));
            r.sstart[t] = stotal;
            stotal += r.scap[t];
        }
    }
    r.stride = stride, r.stotal = stotal;
    return true;
}

// Pass-B work units: tiles split over ranges of pass-A workgroups by expected size; unit k of g
// of a tile also reads slice k of g of the tile's spill area.  Stream layout: largest units
// first (they start before the small ones fill the chip's tail)
inline void plan_units(const TilePlan &pl, const TileLaunch &L, uint64_t n, int cus, const uint64_t *hist, uint64_t sampled,
                       std::vector<WorkUnit> &units) {
    const uint32_t T = pl.tp.ntiles, W = L.W;
    const double target = std::max(1.0, (double)n / ((double)cus * 4));
    std::vector<double> unit_rows;
    units.clear();
    for (uint32_t t = 0; t < T; t++) {
        const double e = (double)n * (double)hist[t] / (double)sampled;
        uint32_t g = (uint32_t)std::min<double>(W, std::max((double)L.g_min, std::ceil(e / target)));
        for (uint32_t k = 0; k < g; k++) {
            units.push_back({t, (uint32_t)((uint64_t)W * k / g), (uint32_t)((uint64_t)W * (k + 1) / g), k | (g << 16)});
            unit_rows.push_back(e / g);
        }
    }
    if (L.stream_layout) {
        std::vector<uint32_t> ord(units.size());
        for (uint32_t i = 0; i < ord.size(); i++) ord[i] = i;
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return unit_rows[a] > unit_rows[b]; });
        std::vector<WorkUnit> sorted(units.size());
        for (uint32_t i = 0; i < ord.size(); i++) sorted[i] = units[ord[i]];
        units.swap(sorted);
    }
    if (units.size() > L.max_units) fail(VH_ERR_RUNTIME, "tiled binning: work-unit table overflow");
}

// Host-image mirror: the units planned per tile (TileParams::tile_units; the unit that draws
// ticket counts[t] - 1 is tile t's last and copies the tile to the images).  Returns the most
// units on one tile.  A tile without a unit is never mirrored by the kernel: the caller copies
// its cells itself (mirror_uncovered)
inline uint32_t count_tile_units(const std::vector<WorkUnit> &units, uint32_t T, std::vector<uint32_t> &counts) {
    counts.assign(T, 0);
    uint32_t most = 0;
    for (const WorkUnit &u : units)
        if (u.tile < T) most = std::max(most, ++counts[u.tile]);
    return most;
}
// Launch order of a mirrored pass B.  plan_units puts the largest units first, so the coldest
// tiles' units end the launch and their tiles all complete in its last microseconds: their
// mirrors (64 KB per tile of a count + sum plan, ~7 MB for the ~110 cold tiles of C2) then
// queue on the 52 GB/s host link when the reduce work is over (+0.13 ms of pass B, DESIGN
// §5.21).  The units of tiles whose units hold fewer than 1 / MIRROR_COLD_DIV of the split
// target (n / 4 cus rows) go first instead, where the link is idle; their reduce work is too
// small to have balanced the tail, which keeps every other unit in plan_units' order.  The
// units themselves, and so the results, are what plan_units returned.
constexpr double MIRROR_COLD_DIV = 64;
inline void mirror_order_units(uint64_t n, int cus, const uint64_t *hist, uint64_t sampled, const std::vector<uint32_t> &counts,
                               std::vector<WorkUnit> &units) {
    const double target = std::max(1.0, (double)n / ((double)cus * 4));
    std::stable_partition(units.begin(), units.end(), [&](const WorkUnit &u) {
        const double e = (double)n * (double)hist[u.tile] / (double)sampled;
        return e / (double)std::max<uint32_t>(counts[u.tile], 1) < target / MIRROR_COLD_DIV;
    });
}
// cells [first, first + n) of tile t: every cell of the grid lies in exactly one tile
inline void tile_cells(const TileParams &tp, uint32_t t, uint64_t &first, uint64_t &n) {
    first = (uint64_t)t << tp.s_log2;
    n = first < tp.cells ? std::min<uint64_t>((uint64_t)1 << tp.s_log2, tp.cells - first) : 0;
}
// maximal runs [first, first + n) of cells whose tiles no unit covers, in grid order
struct CellRange { uint64_t first, n; };
inline std::vector<CellRange> mirror_uncovered(const TileParams &tp, const std::vector<uint32_t> &counts) {
    std::vector<CellRange> out;
    for (uint32_t t = 0; t < tp.ntiles; t++) {
        if (counts[t]) continue;
        uint64_t first, n;
        tile_cells(tp, t, first, n);
        if (!n) continue;
        if (!out.empty() && out.back().first + out.back().n == first) out.back().n += n;
        else out.push_back({first, n});
    }
    return out;
}

// Rounds of pass B's segment walk over one work unit (k_tile_reduce: its `rounds`).  Stream layout:
// the unit's (w_end - w_begin) * ncw segments in rounds of TB_SEGS; regions: one round.
inline uint32_t unit_rounds(const TileLaunch &L, const WorkUnit &u) {
    if (!L.stream_layout) return 1;
    return (uint32_t)(((uint64_t)(u.w_end - u.w_begin) * L.ncw + TB_SEGS - 1) / TB_SEGS);
}
// the most rounds any unit of a launch walks (vh_stat_read("tile_stream_rounds") records it for
// stream-layout launches).  A cold tile (g = g_min units) walks the most: about
// ceil(n / TA_BATCH) / sb segments, so more than one round takes n > TB_SEGS * TA_BATCH * sb rows
inline uint32_t max_unit_rounds(const TileLaunch &L, const std::vector<WorkUnit> &units) {
    uint32_t r = 0;
    for (const WorkUnit &u : units) r = std::max(r, unit_rounds(L, u));
    return r;
}

}  // namespace vh
