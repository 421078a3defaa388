// Check program of the argsort's host planner (vaex_amd/csrc/sort_plan.hpp): no kernels, no
// HIP runtime call, no link to the library.  It reads one case per line from standard input,
//   m  lo hi nan  lo hi nan ...
// (m rows, then per key the min and max code of its non-NaN rows and whether it holds a NaN,
// as k_sort_range leaves them; lo > hi: the key has no non-NaN row) and prints the plan,
//   keys lo:span:width ... | rounds key0-key1:bits:w32|w64:shift,shift ...
// which tests/test_sort_plan.py compares with tests/sort_np.py's plan of the same ranges.
#include <cinttypes>
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "sort_plan.hpp"

using namespace vh;

int main() {
    char buf[4096];
    int bad = 0;
    while (fgets(buf, sizeof(buf), stdin)) {
        std::istringstream in(buf);
        uint64_t m;
        if (!(in >> m)) continue;
        std::vector<SortRange> ranges;
        uint64_t lo, hi;
        int nan;
        while (in >> lo >> hi >> nan) ranges.push_back(SortRange{lo, hi, nan != 0});
        if (ranges.empty() || (int)ranges.size() > SORT_MAX_KEYS) {
            printf("bad case\n");
            bad++;
            continue;
        }
        const SortPlan p = sort_plan(ranges.data(), (int)ranges.size(), m);
        printf("keys");
        for (const SortKeyPlan &k : p.keys) printf(" %" PRIu64 ":%" PRIu64 ":%d", k.lo, k.span, k.width);
        printf(" | rounds");
        int covered = (int)ranges.size();
        for (const SortRound &r : p.rounds) {
            printf(" %d-%d:%d:%s:", r.key0, r.key1, r.bits, r.wide ? "w64" : "w32");
            for (size_t s = 0; s < r.shift.size(); s++) printf("%s%d", s ? "," : "", r.shift[s]);
            // the planner's invariants, on their own: the rounds tile the key list from the back,
            // fit 64 bits, and the fields of a round do not overlap
            int sum = 0;
            for (int k = r.key1 - 1; k >= r.key0; k--) {
                if (r.shift[k - r.key0] != sum) bad++;
                sum += p.keys[k].width;
            }
            if (r.key1 != covered || r.key0 >= r.key1 || sum != r.bits || sum > 64 || r.wide != (sum > 32)) bad++;
            covered = r.key0;
        }
        if (covered != 0) bad++;
        printf("\n");
    }
    return bad ? 1 : 0;
}
