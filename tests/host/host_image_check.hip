// Check program of the host-image mirror's host arithmetic (vaex_amd/csrc/tile_plan.hpp:
// count_tile_units, tile_cells, mirror_uncovered): no kernels, no HIP runtime call.  Plans
// (made-up column addresses, never dereferenced) go through the planner's three stages with
// synthetic samples; for each, and for hand-made unit tables with tiles left out, it checks
//   * the per-tile unit counts add up to the planned units, their maximum is what
//     count_tile_units returns, and a unit of a tile outside the plan is not counted;
//   * every cell of the grid is written exactly once: by the kernel (the tiles that have a
//     unit: the last of their units copies tile_cells) or by the host (mirror_uncovered's
//     ranges, which are maximal, ascending and disjoint);
//   * the launch order of a mirrored pass B (mirror_order_units) holds plan_units' units, each
//     once: those of the cold tiles first, either group in plan_units' order;
//   * the planner's meta offsets end where they did before the mirror's arrays were added
//     behind them, and those arrays lie inside the buffer, 16-byte aligned, without overlap.
// Prints one line per case; exit status 1 when a check failed (tests/test_host_image_plan.py).
#include <cstdio>
#include <string>
#include <vector>

#include "tile_plan.hpp"

using namespace vh;

static int failures = 0;
static void expect(bool ok, const std::string &what) {
    if (ok) return;
    failures++;
    printf("FAILED: %s\n", what.c_str());
}

static const void *addr(int column) { return reinterpret_cast<const void *>((uintptr_t)0x100000000ull * (column + 1)); }

// the mirror's view of one unit table: cells written per writer
static void check_cover(const std::string &name, const TileParams &tp, const std::vector<WorkUnit> &units) {
    const uint32_t T = tp.ntiles;
    std::vector<uint32_t> counts;
    const uint32_t most = count_tile_units(units, T, counts);
    uint64_t total = 0, inside = 0;
    uint32_t mx = 0;
    for (uint32_t t = 0; t < T; t++) total += counts[t], mx = std::max(mx, counts[t]);
    for (const WorkUnit &u : units) inside += u.tile < T;
    expect(counts.size() == T, name + ": one count per tile");
    expect(total == inside, name + ": counts add up to the units");
    expect(most == mx, name + ": the returned maximum");
    std::vector<uint8_t> written(tp.cells, 0);
    bool in_range = true;
    for (uint32_t t = 0; t < T; t++) {
        if (!counts[t]) continue;  // the tile's last unit copies these cells
        uint64_t first, n;
        tile_cells(tp, t, first, n);
        in_range = in_range && first + n <= tp.cells && (first * 8) % 16 == 0;
        for (uint64_t c = first; c < first + n && c < tp.cells; c++) written[c]++;
    }
    const std::vector<CellRange> host = mirror_uncovered(tp, counts);
    uint64_t host_cells = 0;
    for (size_t i = 0; i < host.size(); i++) {
        in_range = in_range && host[i].n > 0 && host[i].first + host[i].n <= tp.cells;
        if (i) expect(host[i - 1].first + host[i - 1].n < host[i].first, name + ": host ranges ascending, disjoint, maximal");
        for (uint64_t c = host[i].first; c < host[i].first + host[i].n && c < tp.cells; c++) written[c]++;
        host_cells += host[i].n;
    }
    expect(in_range, name + ": every copy inside the grid, tiles 16-byte aligned");
    uint64_t once = 0;
    for (uint64_t c = 0; c < tp.cells; c++) once += written[c] == 1;
    expect(once == tp.cells, name + ": every cell written exactly once");
    uint32_t uncovered = 0;
    for (uint32_t t = 0; t < T; t++) uncovered += counts[t] == 0;
    printf("%s T=%u units=%zu most=%u uncovered=%u host_ranges=%zu host_cells=%llu\n", name.c_str(), T, units.size(), most, uncovered,
           host.size(), (unsigned long long)host_cells);
}

int main() {
    struct PlanCase { const char *name; int na; uint64_t n, cells; bool stream; };
    const PlanCase plans[] = {{"count+sum/257x257", 2, (1ull << 20) + 4096, 257 * 257, true},
                              {"count+sum/257x257/regions", 2, (1ull << 20) + 4096, 257 * 257, false},
                              {"count/257x257", 1, (1ull << 20) + 4096, 257 * 257, true},
                              {"count+sum/1027x1027", 2, 1ull << 26, 1027 * 1027, true},
                              {"count+sum/odd-cells", 2, 1ull << 22, 2 * 8192 + 1, true}};
    for (const PlanCase &pc : plans) {
        BinPlan plan{};
        plan.nb = 2;
        for (int d = 0; d < 2; d++) {
            BinnerDev &b = plan.b[d];
            b.kind = 0, b.dtype = VH_F64, b.data = addr(d), b.vmin = 0, b.scale = 1, b.bins = 1024, b.stride = 1;
        }
        FusedAggs fa{};
        fa.na = pc.na;
        fa.a[0].kind = VH_AGG_COUNT, fa.a[0].dtype = VH_F64, fa.a[0].grid = const_cast<void *>(addr(40));
        fa.a[1].kind = VH_AGG_SUM, fa.a[1].dtype = VH_F64, fa.a[1].data = static_cast<const double *>(addr(20));
        fa.a[1].grid = const_cast<void *>(addr(41));
        TileSwitches sw;
        sw.stream = pc.stream;
        TilePlan tpl;
        if (!plan_tiles(plan, fa, pc.n, pc.cells, 2, false, sw, tpl)) {
            expect(false, std::string(pc.name) + ": plan accepted");
            continue;
        }
        for (int k = 0; k < MAX_FUSED_AGGS; k++) expect(tpl.tp.image[k] == nullptr, std::string(pc.name) + ": no image unless the executor sets one");
        expect(tpl.tp.tickets == nullptr && tpl.tp.tile_units == nullptr, std::string(pc.name) + ": no tickets unless mirrored");
        const int cus = 256;
        const TileLaunch L = plan_launch(tpl, pc.n, cus, 1, sw);
        const MetaLayout &m = L.meta;
        const uint32_t T = tpl.tp.ntiles;
        expect(m.bytes == m.brange + 8 * (uint64_t)SAMPLE_BLOCKS, std::string(pc.name) + ": the planner's arrays end at the sample ranges");
        expect(m.tickets >= m.bytes && m.tickets % 16 == 0 && m.tunits >= m.tickets + 4 * (uint64_t)T && m.alloc >= m.tunits + 4 * (uint64_t)T,
               std::string(pc.name) + ": tickets and unit counts behind them, inside the buffer");
        // samples: uniform, one hot tile, tiles the sample missed, rows in two tiles only
        for (int kind = 0; kind < 4; kind++) {
            std::vector<uint64_t> hist(2 * (size_t)T, 0);
            std::vector<uint32_t> brange(2 * (size_t)L.sblocks + 2, 0);
            for (uint64_t b = 0; b < L.sblocks; b++) {
                brange[2 * b] = 0, brange[2 * b + 1] = T - 1;
                for (uint32_t t = 0; t < T; t++) {
                    uint64_t c = TA_BATCH / T;
                    if (kind == 1) c = t == T / 3 ? TA_BATCH / 2 : c / 2;
                    if (kind == 2 && t % 3 == 1) c = 0;
                    if (kind == 3) c = t < 2 ? TA_BATCH / 2 : 0;
                    hist[t] += c, hist[T + t] += c * c;
                }
            }
            TileRegions reg;
            if (!size_regions(tpl, L, pc.n, hist.data(), brange.data(), reg)) {
                expect(false, std::string(pc.name) + ": regions sized");
                continue;
            }
            std::vector<WorkUnit> units;
            plan_units(tpl, L, pc.n, cus, hist.data(), reg.sampled, units);
            const std::string name = std::string(pc.name) + "/sample" + std::to_string(kind);
            check_cover(name, tpl.tp, units);
            std::vector<uint32_t> counts;
            count_tile_units(units, T, counts);
            bool all = true;
            for (uint32_t t = 0; t < T; t++) all = all && counts[t] >= 1;
            expect(all, name + ": the planner gives every tile a unit");
            if (kind == 1) expect(counts[T / 3] >= 2, name + ": the hot tile is split over several units");
            // the mirrored launch order: the same units, the cold tiles' first, each group in plan_units' order
            {
                std::vector<WorkUnit> ordered = units;
                mirror_order_units(pc.n, cus, hist.data(), reg.sampled, counts, ordered);
                const double thr = std::max(1.0, (double)pc.n / (cus * 4.0)) / MIRROR_COLD_DIV;
                auto cold = [&](const WorkUnit &u) { return (double)pc.n * (double)hist[u.tile] / (double)reg.sampled / counts[u.tile] < thr; };
                auto same = [](const WorkUnit &a, const WorkUnit &b) { return a.tile == b.tile && a.w_begin == b.w_begin && a.w_end == b.w_end && a.pad == b.pad; };
                std::vector<WorkUnit> want;
                for (const WorkUnit &u : units) if (cold(u)) want.push_back(u);
                const size_t ncold = want.size();
                for (const WorkUnit &u : units) if (!cold(u)) want.push_back(u);
                bool eq = want.size() == ordered.size();
                for (size_t i = 0; eq && i < want.size(); i++) eq = same(want[i], ordered[i]);
                expect(eq, name + ": cold tiles' units first, nothing added or dropped, order kept within each group");
                printf("%s/order cold_units=%zu of %zu\n", name.c_str(), ncold, units.size());
            }
            // the same table with tiles left out: first, last, a run in the middle, every other one
            for (int drop = 0; drop < 4; drop++) {
                std::vector<WorkUnit> some;
                for (const WorkUnit &u : units) {
                    const uint32_t t = u.tile;
                    const bool out = drop == 0 ? t == 0 : drop == 1 ? t == T - 1 : drop == 2 ? (t >= T / 3 && t < T / 3 + 3) : (t & 1);
                    if (!out) some.push_back(u);
                }
                some.push_back({T + 7, 0, 1, 1u << 16});  // not a tile of this plan: ignored
                check_cover(name + "/drop" + std::to_string(drop), tpl.tp, some);
            }
        }
        check_cover(std::string(pc.name) + "/no-units", tpl.tp, {});
    }
    printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
