"""tests/join_np.py, the NumPy restatement of the reference's index_hash and DataFrame.join,
against cases worked out by hand from the reference (tests/join_cases.py; CPU only)."""
import numpy as np
import pytest

import join_np as jn
from join_cases import CASES, as_list, expected_list, filter_array


@pytest.mark.parametrize("name", sorted(CASES))
def test_case(name):
    case = CASES[name]
    kw = dict(case["kw"], left_filter=filter_array(case["left"], case.get("left_filter")),
              right_filter=filter_array(case["right"], case.get("right_filter")))
    if "raises" in case:
        with pytest.raises(case["raises"][0], match=case["raises"][1]):
            jn.join_np(case["left"], case["right"], **kw)
        return
    cols, keep = jn.join_np(case["left"], case["right"], **kw)
    assert list(cols) == list(case["expect"])
    for k, v in case["expect"].items():
        assert as_list(cols[k]) == expected_list(v), k
    visible = case.get("visible")
    assert (None if keep is None else np.where(keep)[0].tolist()) == visible


def test_unsupported_how_and_dtypes():
    with pytest.raises(ValueError, match="join type not supported: outer"):
        jn.join_np({"x": np.arange(3)}, {"x": np.arange(3)}, on="x", how="outer")
    with pytest.raises(TypeError):
        jn.join_np({"x": np.arange(3, dtype=np.int32)}, {"x": np.arange(3, dtype=np.int64)}, on="x")


def test_index_np_rules():
    """first row / overflow order / last NaN and null / length (hash_primitives.hpp:636-674)."""
    v = np.array([4.0, np.nan, 4.0, 5.0, np.nan, 4.0, 6.0])
    m = np.array([0, 0, 0, 0, 0, 0, 1], bool)
    ix = jn.index_np(v, m, start_index=10)
    four, five = np.float64(4.0).view("u8"), np.float64(5.0).view("u8")
    assert ix.first == {four: 10, five: 13} and ix.extras == {four: [12, 15]}
    assert (ix.nan_value, ix.null_value, ix.nan_count, ix.null_count) == (14, 16, 2, 1)
    assert ix.has_duplicates and ix.length == 2 + 2 + 1 + 1
    out, unknown = jn.map_index_np(ix, np.array([5.0, 7.0, np.nan, 4.0]), np.array([0, 0, 0, 1], bool))
    assert out.tolist() == [13, -1, 14, 16] and unknown
    left, right = jn.map_index_duplicates_np(ix, np.array([5.0, 4.0, np.nan, 4.0]), np.array([0, 0, 0, 1], bool), 100)
    assert left.tolist() == [101, 101] and right.tolist() == [12, 15]
    # select: the unselected rows are not seen at all; -0.0 and 0.0 are two keys
    ix = jn.index_np(np.array([0.0, -0.0, 0.0]), select=np.array([0, 1, 1], bool))
    assert ix.first == {np.float64(-0.0).view("u8"): 1, 0: 2} and not ix.has_duplicates
    assert jn.map_index_np(jn.index_np(np.array([1, 2])), np.array([np.nan]))[0].tolist() == [-1]
