"""tests/sort_np.py, the NumPy restatement of the device argsort's code / span / width / rounds
/ packing, against ``np.lexsort`` / ``np.argsort(kind="stable")``, and its frame operations
against the hand-worked frames of tests/sort_cases.py.  No GPU; every comparison is exact."""
import numpy as np
import pytest

import sort_np as sn
from sort_cases import (EXTRACT_CASES, FRAME, SORT_CASES, TAKE_FILTER, TAKE_INDICES, TAKE_KEPT, TAKE_VISIBLE, as_list, keep_mask,
                        rows_of)


def float_key(dtype, n, seed):
    """NaN in a seventh of the rows, +-inf, +-0.0, +-denormals and the extremes."""
    rng = np.random.default_rng(seed)
    fi = np.finfo(dtype)
    v = rng.normal(size=n).astype(dtype)
    special = np.array([np.inf, -np.inf, 0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny / 2, -fi.tiny / 2,
                        fi.max, fi.min], dtype=dtype)
    where = rng.integers(0, n, n // 3)
    v[where] = special[rng.integers(0, len(special), len(where))]
    v[::7] = np.nan
    return v


def int_key(dtype, n, seed):
    """The full range with both extremes present."""
    ii = np.iinfo(dtype)
    v = np.random.default_rng(seed).integers(ii.min, ii.max, n, dtype=dtype, endpoint=True)
    v[n // 3], v[n // 2] = ii.min, ii.max
    return v


N = 1500
KEYS = {
    "float64": float_key(np.float64, N, 1), "float32": float_key(np.float32, N, 2),
    "int64": int_key(np.int64, N, 3), "int32": int_key(np.int32, N, 4), "uint64": int_key(np.uint64, N, 5),
    "bool": np.random.default_rng(6).random(N) < 0.5,
    "u8x3": np.random.default_rng(7).integers(0, 3, N).astype(np.uint8),
    "const": np.full(N, 7, np.int16), "allnan": np.full(N, np.nan, np.float32),
    "i32b": int_key(np.int32, N, 8),
}
KEY_LISTS = {
    "two-int32 (64 bits)": ["int32", "i32b"],
    "two-int32 + bool (65 bits)": ["int32", "i32b", "bool"],
    "int64 + u8x3 (66 bits)": ["int64", "u8x3"],
    "u8x3 + int64": ["u8x3", "int64"],
    "four keys": ["u8x3", "bool", "float32", "float64"],
    "const + allnan + f64": ["const", "allnan", "float64"],
    "bool + const": ["bool", "const"],
}


def check(keys, rows=None):
    for ascending in (True, False):
        got = sn.argsort_np(keys, rows, ascending)
        want = sn.reference_order(keys, rows, ascending)
        assert got.tolist() == want.tolist()


@pytest.mark.parametrize("name", sorted(KEYS))
def test_one_key_equals_stable_argsort(name):
    check([KEYS[name]])
    check([KEYS[name]], np.arange(0, N, 2))
    check([KEYS[name]], np.arange(0))
    check([KEYS[name]], np.array([N - 1]))
    check([KEYS[name][:0]])
    check([KEYS[name][:1]])


@pytest.mark.parametrize("name", sorted(KEY_LISTS))
def test_key_lists_equal_lexsort(name):
    keys = [KEYS[k] for k in KEY_LISTS[name]]
    check(keys)
    check(keys, np.flatnonzero(np.random.default_rng(9).random(N) < 0.4))


def test_descending_is_the_exact_reverse_and_nan_is_last():
    k = KEYS["float32"]
    up, down = sn.argsort_np([k], None, True), sn.argsort_np([k], None, False)
    assert up.tolist() == down[::-1].tolist()
    nnan = int(np.isnan(k).sum())
    assert nnan > 0 and np.isnan(k[up[-nnan:]]).all() and not np.isnan(k[up[:-nnan]]).any()
    # all NaN are equal: they keep their row order
    assert up[-nnan:].tolist() == np.flatnonzero(np.isnan(k)).tolist()
    # -0.0 == 0.0: the zeros keep their row order whatever their sign
    z = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0])
    assert sn.argsort_np([z]).tolist() == [5, 0, 1, 3, 4, 2]


def test_widths_and_rounds():
    def widths_rounds(names, rows=None):
        keys, rounds = sn.plan([sn.key_range(KEYS[k], rows) for k in names], N)
        return [w for _, _, w in keys], [(k0, k1, bits, wide) for k0, k1, bits, wide, _ in rounds]

    assert widths_rounds(["const"]) == ([0], [(0, 1, 0, False)])
    assert widths_rounds(["allnan"]) == ([0], [(0, 1, 0, False)])
    assert widths_rounds(["bool"]) == ([1], [(0, 1, 1, False)])
    assert widths_rounds(["int32"]) == ([32], [(0, 1, 32, False)])
    assert widths_rounds(["int64"]) == ([64], [(0, 1, 64, True)])
    assert widths_rounds(["uint64"]) == ([64], [(0, 1, 64, True)])
    # float32 with NaN and both extremes: the codes of -max .. +inf and one more for NaN
    assert widths_rounds(["float32"])[0] == [32]
    assert widths_rounds(["float64"])[0] == [64]
    assert widths_rounds(["int32", "i32b"]) == ([32, 32], [(0, 2, 64, True)])  # 64: one round
    assert widths_rounds(["int32", "i32b", "bool"]) == ([32, 32, 1], [(1, 3, 33, True), (0, 1, 32, False)])  # 65
    assert widths_rounds(["int64", "u8x3"]) == ([64, 2], [(1, 2, 2, False), (0, 1, 64, True)])  # 66
    assert widths_rounds(["u8x3", "int64"]) == ([2, 64], [(1, 2, 64, True), (0, 1, 2, False)])
    # zero-width keys ride along in any round
    assert widths_rounds(["const", "int64", "allnan"]) == ([0, 64, 0], [(0, 3, 64, True)])
    # no rows: the width is 0, whether the range says so (lo > hi) or m does
    assert widths_rounds(["int64"], np.arange(0))[0] == [0]
    assert sn.plan([(0, 2 ** 64 - 1, False)], 0)[0] == [(0, 0, 0)]
    # shifts: the last key of a round sits at bit 0
    _, rounds = sn.plan([(0, 2, False), (5, 5, False), (0, 255, True)], 10)
    assert rounds == [(0, 3, 2 + 0 + 9, False, [9, 9, 0])]


def test_span_of_the_float64_extremes_fits():
    k = np.array([-np.inf, np.inf, np.nan])
    lo, hi, any_nan = sn.key_range(k)
    assert any_nan and hi - lo + 1 < 2 ** 64
    assert sn.plan([(lo, hi, any_nan)], 3)[0][0][2] == 64


@pytest.mark.parametrize("name, flt, by, ascending, rows", SORT_CASES, ids=[c[0] for c in SORT_CASES])
def test_sort_frame_against_the_hand_worked_cases(name, flt, by, ascending, rows):
    cols = dict(FRAME)
    if "-x" in (by if isinstance(by, str) else ""):
        cols["-x"] = -FRAME["x"]
    got = sn.sort_frame_np(cols, by, keep_mask(flt), ascending)
    assert {k: as_list(got[k]) for k in FRAME} == rows_of(rows)


@pytest.mark.parametrize("flt, rows", EXTRACT_CASES, ids=[str(c[0]) for c in EXTRACT_CASES])
def test_extract_against_the_hand_worked_cases(flt, rows):
    got = sn.extract_np(FRAME, keep_mask(flt))
    assert {k: as_list(v) for k, v in got.items()} == rows_of(rows)


def test_take_against_the_hand_worked_case():
    kept = sn.extract_np(FRAME, keep_mask(TAKE_FILTER))
    got = {k: v[np.asarray(TAKE_INDICES)] for k, v in kept.items()}
    assert {k: as_list(v) for k, v in got.items()} == rows_of(TAKE_KEPT)
    assert np.flatnonzero(keep_mask(TAKE_FILTER)[TAKE_INDICES]).tolist() == TAKE_VISIBLE
