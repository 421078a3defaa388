// The host plan of vh_argsort (sort.hip): from each key's range of order-preserving codes to
// the radix rounds that run.  No HIP call in here: tests/host/sort_plan_check.hip compiles it
// into a stand-alone program (tests/test_sort_plan.py compares it with tests/sort_np.py).
//
// A key's code is an unsigned integer that orders like the key (sort.hip sort_code).  Over the
// rows that are sorted, the non-NaN codes span [lo, hi]; a row packs `code - lo`, a NaN row
// packs `span` = hi - lo + 1 (NaN sorts last, all NaN are equal; without NaN, span = hi - lo).
// The key needs width = bit_length(span) bits: 0 for a constant key, an all-NaN key or no rows.
// span cannot overflow: only floats have NaN, and the float64 codes of -inf / +inf lie more
// than 2^52 inside the ends of the 64-bit range.
//
// Rounds are least-significant first (a stable sort per round, the last key first): each takes
// the longest run of the remaining trailing keys whose widths sum to at most 64, the earliest
// key of the run in the highest bits.  A round of at most 32 bits sorts 32-bit words; a round
// of 0 bits sorts nothing.  Every round sorts exactly bits [0, sum).
#pragma once
#include <cstdint>
#include <vector>

namespace vh {

constexpr int SORT_MAX_KEYS = 16;

struct SortRange {  // what k_sort_range leaves per key
    uint64_t lo, hi;  // min / max code over the non-NaN rows; lo > hi: there is none
    bool any_nan;
};

struct SortKeyPlan {
    uint64_t lo = 0, span = 0;
    int width = 0;
};

struct SortRound {
    int key0 = 0, key1 = 0;  // keys [key0, key1) of the key list, key0 in the highest bits
    int bits = 0;            // sum of their widths: the sort runs over bits [0, bits)
    bool wide = false;       // 64-bit words (bits > 32)
    std::vector<int> shift;  // per key of the run: where its field starts
};

struct SortPlan {
    std::vector<SortKeyPlan> keys;
    std::vector<SortRound> rounds;  // in execution order: the last keys first
};

inline int sort_bit_length(uint64_t v) {
    int b = 0;
    while (v) {
        b++;
        v >>= 1;
    }
    return b;
}

inline SortPlan sort_plan(const SortRange *ranges, int nkeys, uint64_t m) {
    SortPlan p;
    p.keys.resize(nkeys);
    for (int k = 0; k < nkeys; k++) {
        SortKeyPlan &kp = p.keys[k];
        const bool any_value = m > 0 && ranges[k].lo <= ranges[k].hi;
        if (any_value) {
            kp.lo = ranges[k].lo;
            kp.span = ranges[k].hi - ranges[k].lo + (ranges[k].any_nan ? 1 : 0);
        }
        kp.width = sort_bit_length(kp.span);
    }
    int end = nkeys;
    while (end > 0) {
        int begin = end, sum = 0;
        while (begin > 0 && sum + p.keys[begin - 1].width <= 64) sum += p.keys[--begin].width;
        SortRound r;
        r.key0 = begin;
        r.key1 = end;
        r.bits = sum;
        r.wide = sum > 32;
        r.shift.resize(end - begin);
        int at = 0;
        for (int k = end - 1; k >= begin; k--) {
            r.shift[k - begin] = at;
            at += p.keys[k].width;
        }
        p.rounds.push_back(r);
        end = begin;
    }
    return p;
}

}  // namespace vh
