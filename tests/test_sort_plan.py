"""The argsort's host planner (vaex_amd/csrc/sort_plan.hpp) without a GPU, through its check
program (tests/host/sort_plan_check.hip, built by the default make next to the library): fed
(min code, max code, any NaN) triples, its keys (lo, span, width) and rounds (keys, bits, word
size, shifts) equal those of the NumPy restatement (tests/sort_np.py), character for character.
The program also checks on its own that the rounds tile the key list from the back, fit 64 bits
and do not overlap their fields."""
import os
import subprocess

import sort_np as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "vaex_amd", "sort_plan_check")

U64 = 2 ** 64 - 1


def key_of_width(w, lo=0):
    """A (lo, hi, any NaN) triple whose width is w bits."""
    lo = min(lo, U64 - (2 ** w - 1))
    return (lo, lo, False) if w == 0 else (lo, lo + 2 ** w - 1, False)


WIDTH_LISTS = [[0], [1], [32], [33], [64], [32, 32], [32, 32, 1], [2, 64], [64, 2], [0, 2], [64, 32, 64, 64]]


def cases():
    out = [(10, [key_of_width(w, lo=3 * i) for i, w in enumerate(ws)]) for ws in WIDTH_LISTS]
    out += [
        (10, [(5, 5, True)]),                        # a constant with NaN: span 1, width 1
        (10, [(U64, 0, True)]),                      # all NaN: width 0
        (10, [(U64, 0, False), (0, 1, False)]),      # no row at all in the first key's range
        (0, [(0, U64, False), (0, 255, True)]),      # m = 0: every width is 0
        (10, [(0, 2 ** 32 - 2, True)]),              # NaN takes span to 2^32 - 1: still 32 bits
        (10, [(0, 2 ** 32 - 1, True)]),              # ... and to 2^32: 33 bits
        (10, [(0x000FFFFFFFFFFFFF, 0xFFF0000000000000, True)]),  # float64 -inf .. +inf with NaN
        (10, [(0, U64, False)]),                     # full-range uint64
        (10, [(7, 8, False)] * 16),                  # 16 one-bit keys: one round
        (10, [(0, 2 ** 31, False)] * 3),             # 32 + 32, then 32
        (10, [(0, 1, False), (0, U64, False), (0, 1, False), (0, 0, False)]),
    ]
    return out


def test_rounds_equal_the_numpy_restatement():
    cs = cases()
    text = "".join(f"{m} " + " ".join(f"{lo} {hi} {int(nan)}" for lo, hi, nan in ranges) + "\n" for m, ranges in cs)
    res = subprocess.run([CHECK], input=text, capture_output=True, text=True, timeout=60)
    got = res.stdout.splitlines()
    assert len(got) == len(cs)
    for (m, ranges), line in zip(cs, got):
        assert line == sn.plan_text(ranges, m), (m, ranges)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]


def test_the_width_lists_give_the_rounds_worked_by_hand():
    """(key0, key1, bits, 64-bit words) per round, in execution order."""
    want = {
        (0,): [(0, 1, 0, False)], (1,): [(0, 1, 1, False)], (32,): [(0, 1, 32, False)], (33,): [(0, 1, 33, True)],
        (64,): [(0, 1, 64, True)], (32, 32): [(0, 2, 64, True)], (32, 32, 1): [(1, 3, 33, True), (0, 1, 32, False)],
        (2, 64): [(1, 2, 64, True), (0, 1, 2, False)], (64, 2): [(1, 2, 2, False), (0, 1, 64, True)],
        (0, 2): [(0, 2, 2, False)], (64, 32, 64, 64): [(3, 4, 64, True), (2, 3, 64, True), (1, 2, 32, False), (0, 1, 64, True)],
    }
    assert sorted(want) == sorted(tuple(w) for w in WIDTH_LISTS)
    for ws in WIDTH_LISTS:
        keys, rounds = sn.plan([key_of_width(w) for w in ws], 10)
        assert [w for _, _, w in keys] == ws
        assert [r[:4] for r in rounds] == want[tuple(ws)], ws
