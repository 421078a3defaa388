"""Pins tests/value_counts_np.py (the yardstick of the GPU counter tests) on cases worked out
by hand from the reference: counter layout packages/vaex-core/src/hash_primitives.hpp:338-348,
value_counts packages/vaex-core/vaex/expression.py:946-1061, unique
packages/vaex-core/vaex/dataframe.py:542-619.  No GPU."""
import numpy as np
import pytest

import value_counts_np as vc

nan = float("nan")
X = np.array([0, 1, 1, 2, 2, 2, nan])     # the reference's small case: 0 once, 1 twice, 2 three times, one NaN
XM = np.ma.array(X, mask=[1, 1, 0, 0, 0, 0, 0])  # its masked copy: the 0 and one 1 are missing


def series(s):
    return s.index.tolist(), s.tolist()


def check(s, labels, counts):
    got_labels, got_counts = series(s)
    assert vc.same_labels(got_labels, labels), got_labels
    assert got_counts == counts


def test_counter_layout():
    # hash_primitives.hpp:338-348: NaN at 0, then the regular keys (no null: offset 1)
    keys, counts, null_index = vc.counter_np(X)
    assert vc.same_labels(keys.tolist(), [nan, 0.0, 1.0, 2.0])
    assert counts.tolist() == [1, 1, 2, 3] and counts.dtype == np.int64 and null_index == -1
    # with a null entry: NaN 0, null 1 (expression.py:1027-1030 null_offset), key value zero
    keys, counts, null_index = vc.counter_np(XM)
    assert vc.same_labels(keys.tolist(), [nan, 0.0, 1.0, 2.0])
    assert counts.tolist() == [1, 2, 1, 3] and null_index == 1
    # no NaN: the null entry is at 0
    keys, counts, null_index = vc.counter_np(np.array([4, 4, 9], np.int32), mask=[0, 1, 0])
    assert keys.tolist() == [0, 4, 9] and counts.tolist() == [1, 1, 1] and null_index == 0 and keys.dtype == np.int32


@pytest.mark.parametrize("dropna,ascending,labels,counts", [
    # expression.py:1046-1050: argsort of [1, 1, 2, 3] (stable) is [0, 1, 2, 3], reversed when not ascending
    (False, False, [2.0, 1.0, 0.0, nan], [3, 2, 1, 1]),
    (False, True, [nan, 0.0, 1.0, 2.0], [1, 1, 2, 3]),
    # expression.py:1033-1034,1039: the NaN entry (index 0) is deleted first
    (True, False, [2.0, 1.0, 0.0], [3, 2, 1]),
    (True, True, [0.0, 1.0, 2.0], [1, 2, 3]),
])
def test_value_counts_nan(dropna, ascending, labels, counts):
    check(vc.value_counts_np(X, dropna=dropna, ascending=ascending), labels, counts)
    check(vc.value_counts_np(X, dropnan=dropna, ascending=ascending), labels, counts)


def test_value_counts_masked():
    # counter: keys [nan, null, 1, 2], counts [1, 2, 1, 3].  Stable argsort: [0, 2, 1, 3]; reversed
    # [3, 1, 2, 0] -> [2, null, 1, nan] / [3, 2, 1, 1]; then "missing" moves to the front
    # with its count (expression.py:1052-1059)
    check(vc.value_counts_np(XM), ["missing", 2.0, 1.0, nan], [2, 3, 1, 1])
    # ascending: [nan, 1, null, 2] / [1, 1, 2, 3] -> missing first
    check(vc.value_counts_np(XM, ascending=True), ["missing", nan, 1.0, 2.0], [2, 1, 1, 3])
    # dropmissing (expression.py:1031-1032 deletes null_offset): [nan, 1, 2] / [1, 1, 3]
    check(vc.value_counts_np(XM, dropmissing=True), [2.0, 1.0, nan], [3, 1, 1])
    check(vc.value_counts_np(XM, dropmissing=True, ascending=True), [nan, 1.0, 2.0], [1, 1, 3])
    # dropnan only: [null, 1, 2] / [2, 1, 3] -> argsort [1, 0, 2] reversed [2, 0, 1]
    check(vc.value_counts_np(XM, dropnan=True), ["missing", 2.0, 1.0], [2, 3, 1])
    check(vc.value_counts_np(XM, dropna=True), [2.0, 1.0], [3, 1])
    # a mask given beside the values is the same thing
    check(vc.value_counts_np(X, mask=np.ma.getmaskarray(XM)), ["missing", 2.0, 1.0, nan], [2, 3, 1, 1])


def test_ties_are_stable():
    # keys [3, 5, 7], counts [2, 2, 1]: stable argsort [2, 0, 1]; descending is its exact reverse
    v = np.array([5, 3, 5, 3, 7], np.int64)
    check(vc.value_counts_np(v, ascending=True), [7, 3, 5], [1, 2, 2])
    check(vc.value_counts_np(v), [5, 3, 7], [2, 2, 1])


def test_signed_zero_keys():
    keys, counts, _ = vc.counter_np(np.array([0.0, -0.0, 0.0]))
    assert vc.same_labels(keys.tolist(), [-0.0, 0.0]) and counts.tolist() == [1, 2]
    assert not vc.same_labels([0.0], [-0.0])
    keys, counts, _ = vc.counter_np(np.array([0.0, -0.0, -1.5, 2.5], np.float32))
    assert vc.same_labels(keys.tolist(), [-1.5, -0.0, 0.0, 2.5]) and keys.dtype == np.float32


def test_integer_extremes():
    lo = np.iinfo(np.int64).min
    keys, counts, _ = vc.counter_np(np.array([-1, -1, 0, lo], np.int64))
    assert keys.tolist() == [lo, -1, 0] and counts.tolist() == [1, 2, 1]
    hi = np.iinfo(np.uint64).max
    keys, counts, _ = vc.counter_np(np.array([hi, 0, hi], np.uint64))
    assert keys.tolist() == [0, hi] and counts.tolist() == [1, 2] and keys.dtype == np.uint64
    check(vc.value_counts_np(np.array([hi, 0, hi], np.uint64)), [hi, 0], [2, 1])


def test_select_rows_are_not_seen():
    keys, counts, null_index = vc.counter_np(np.array([1.0, nan, 3.0, 3.0]), mask=[0, 0, 1, 0], select=[1, 0, 0, 1])
    assert keys.tolist() == [1.0, 3.0] and counts.tolist() == [1, 1] and null_index == -1


def test_nan_payloads_are_one_key():
    v = np.array([0x7ff8000000000000, 0xfff8000000000001, 0x7ff0000000000123, 0x3ff0000000000000], np.uint64).view(np.float64)
    keys, counts, _ = vc.counter_np(v)
    assert vc.same_labels(keys.tolist(), [nan, 1.0]) and counts.tolist() == [3, 1]


def test_unique():
    # dataframe.py:599-614 over a set filled by one update call: regular keys in first-appearance
    # order, then NaN, then the (masked) null entry
    assert vc.same_labels(vc.unique_np(X), [0.0, 1.0, 2.0, nan])
    assert vc.same_labels(vc.unique_np(XM), [1.0, 2.0, nan, None])
    assert vc.same_labels(vc.unique_np(XM, dropnan=True), [1.0, 2.0, None])
    assert vc.same_labels(vc.unique_np(XM, dropmissing=True), [1.0, 2.0, nan])
    assert vc.same_labels(vc.unique_np(XM, dropna=True), [1.0, 2.0])
    assert vc.unique_np(np.array([7, 3, 7, 5], np.int16)) == [7, 3, 5]
