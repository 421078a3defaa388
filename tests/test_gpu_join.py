"""``DataFrame.join`` / ``take`` / ``_index`` on host and HBM frames against the NumPy restatement
of the reference (tests/join_np.py) and the hand-worked cases of tests/join_cases.py.  Every
comparison is exact, column order included."""
import numpy as np
import pytest

import join_np as jn
from join_cases import CASES, as_list, expected_list, filter_array

pytestmark = pytest.mark.gpu


def frame(columns, hbm, filter_expression=None):
    """A host frame, or an HBM frame (masked columns have no HBM form and stay on the host)."""
    import vaex_amd
    from vaex_amd.device import DeviceArray
    cols = {k: (DeviceArray.from_numpy(np.ascontiguousarray(v)) if hbm and not np.ma.isMaskedArray(v) else v)
            for k, v in columns.items()}
    df = vaex_amd.from_arrays(**cols)
    return df if filter_expression is None else df.filter(filter_expression)


def is_hbm(column):
    from vaex_amd.device import DeviceArray
    return isinstance(column, DeviceArray)


def check_frame(res, cols, keep):
    """The joined frame against join_np's (columns over all rows, carried filter)."""
    assert list(res.columns) == list(cols)
    n = len(next(iter(cols.values())))
    assert res.length_unfiltered() == n
    for k, v in cols.items():
        assert as_list(res.columns[k]) == as_list(v), k
        assert np.dtype(res.columns[k].dtype) == np.asarray(v).dtype, k
    assert res.filtered == (keep is not None)
    if keep is not None:
        assert len(res) == int(keep.sum())


@pytest.mark.parametrize("hbm", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_worked_case(name, hbm):
    case = CASES[name]
    left = frame(case["left"], hbm, case.get("left_filter"))
    right = frame(case["right"], hbm, case.get("right_filter"))
    if "raises" in case:
        with pytest.raises(case["raises"][0], match=case["raises"][1]):
            left.join(right, **case["kw"])
        return
    res = left.join(right, **case["kw"])
    assert list(res.columns) == list(case["expect"])
    for k, v in case["expect"].items():
        assert as_list(res.columns[k]) == expected_list(v), k
    visible = case.get("visible")
    assert res.filtered == (visible is not None)
    if visible is not None:
        first = next(iter(case["expect"]))
        assert as_list(res.evaluate(first)) == expected_list([case["expect"][first][i] for i in visible])
    # the inputs are untouched
    assert list(left.columns) == list(case["left"]) and list(right.columns) == list(case["right"])


def random_tables(n_left=3000, n_right=700, seed=0):
    rng = np.random.default_rng(seed)
    right = dict(k=rng.permutation(2 * n_right)[:n_right].astype(np.int32), g=rng.integers(0, 9, n_right).astype(np.int64),
                 w=rng.normal(size=n_right))
    left = dict(k=rng.integers(0, 2 * n_right, n_left).astype(np.int32), v=rng.normal(size=n_left),
                s=rng.integers(0, 100, n_left).astype(np.int16))
    return left, right


@pytest.mark.parametrize("hbm", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("right_filter", [None, "g < 6"])
@pytest.mark.parametrize("left_filter", [None, "s >= 30"])
@pytest.mark.parametrize("how", ["left", "right", "inner"])
def test_how_and_filters(how, left_filter, right_filter, hbm):
    left, right = random_tables()
    # a right join indexes the left table, whose keys repeat
    kw = dict(on="k", how=how, allow_duplication=how == "right")
    cols, keep = jn.join_np(left, right, left_filter=filter_array(left, left_filter),
                            right_filter=filter_array(right, right_filter), **kw)
    res = frame(left, hbm, left_filter).join(frame(right, hbm, right_filter), **kw)
    check_frame(res, cols, keep)
    if how == "inner" and hbm:
        assert all(is_hbm(c) for c in res.columns.values())  # nothing is masked: all stays in HBM


@pytest.mark.parametrize("hbm", [False, True], ids=["host", "hbm"])
def test_duplication(hbm):
    rng = np.random.default_rng(3)
    right = dict(k=rng.integers(0, 300, 900).astype(np.int64), w=rng.normal(size=900))
    left = dict(k=rng.integers(0, 400, 2000).astype(np.int64), v=np.arange(2000, dtype=np.float32))
    for how, lf in (("left", None), ("inner", None), ("left", "v < 1500")):
        cols, keep = jn.join_np(left, right, on="k", how=how, allow_duplication=True, left_filter=filter_array(left, lf))
        res = frame(left, hbm, lf).join(frame(right, hbm), on="k", how=how, allow_duplication=True)
        check_frame(res, cols, keep)
    with pytest.raises(ValueError, match="allow_duplication=True"):
        frame(left, hbm).join(frame(right, hbm), on="k")


def test_all_matched_stays_in_hbm_and_unmatched_is_masked_on_host():
    left, right = random_tables()
    known = np.isin(left["k"], right["k"])
    matched = {k: v[known] for k, v in left.items()}
    res = frame(matched, True).join(frame(right, True), on="k")
    assert all(is_hbm(c) for c in res.columns.values())
    check_frame(res, *jn.join_np(matched, right, on="k"))
    res = frame(left, True).join(frame(right, True), on="k")
    assert all(is_hbm(res.columns[k]) for k in left)
    assert all(np.ma.isMaskedArray(res.columns[k]) for k in ("g", "w"))
    assert np.ma.getmaskarray(res.columns["g"]).tolist() == (~known).tolist()
    check_frame(res, *jn.join_np(left, right, on="k"))


def test_errors():
    import vaex_amd
    left, right = random_tables(50, 20)
    l, r = frame(left, True), frame(right, True)
    with pytest.raises(ValueError, match="join type not supported: outer"):
        l.join(r, on="k", how="outer")
    with pytest.raises(TypeError, match="dtypes differ"):
        l.join(frame(dict(k=right["k"].astype(np.int64), w=right["w"]), True), on="k")
    with pytest.raises(ValueError, match="column name collision: v"):
        l.join(frame(dict(k=right["k"], v=right["w"]), True), on="k")
    with pytest.raises(ValueError, match="differ in length"):
        l.join(frame(dict(z=np.arange(20.0)), True))
    # a rename that an expression depends on is refused: expressions are not rewritten
    rv = frame(dict(k=right["k"], v=right["w"]), False)
    rv.add_virtual_column("v2", "v * 2")
    with pytest.raises(NotImplementedError, match="expression rewriting"):
        frame(left, False).join(rv, on="k", rsuffix="_r")
    with pytest.raises(NotImplementedError):
        l.filter("s > 3").take(np.arange(3))
    assert isinstance(l, vaex_amd.DataFrame)


@pytest.mark.parametrize("hbm", [False, True], ids=["host", "hbm"])
def test_virtual_columns_variables_and_expression_keys(hbm):
    left, right = random_tables(500, 100)
    r = frame(right, hbm)
    r.add_virtual_column("w2", "w * scale")
    r.add_variable("scale", 3.0)
    l = frame(left, hbm)
    res = l.join(r, left_on=l.k, right_on=r["k"], how="inner")  # Expression-typed keys
    assert res.virtual_columns == {"w2": "w * scale"} and res.variables["scale"] == 3.0
    cols, _ = jn.join_np(left, right, on="k", how="inner")
    got = res.evaluate("w2")
    assert np.array_equal(got.to_numpy() if is_hbm(got) else np.asarray(got), cols["w"] * 3.0)


@pytest.mark.parametrize("hbm", [False, True], ids=["host", "hbm"])
def test_twelve_column_right_frame(hbm):
    """More columns than one gather launch takes (8), of every item size."""
    rng = np.random.default_rng(5)
    dts = [np.float64, np.int8, np.int16, np.float32, np.uint64, np.bool_, np.uint16, np.int32, np.int64, np.uint8,
           np.uint32, np.float64]
    right = dict(k=rng.permutation(500).astype(np.int64))
    right.update({f"c{i}": rng.integers(0, 100, 500).astype(dt) for i, dt in enumerate(dts)})
    for lo, hi in ((0, 500), (0, 800)):  # all matched / some unknown
        left = dict(k=rng.integers(lo, hi, 3001).astype(np.int64))
        res = frame(left, hbm).join(frame(right, hbm), on="k")
        check_frame(res, *jn.join_np(left, right, on="k"))


@pytest.mark.parametrize("hbm", [False, True], ids=["host", "hbm"])
def test_take(hbm):
    left, _ = random_tables(1000, 10)
    idx = np.random.default_rng(6).integers(0, 1000, 777)
    df = frame(left, hbm)
    df.add_virtual_column("v2", "v + 1")
    from vaex_amd.device import DeviceArray
    for indices in (idx, idx.astype(np.int32), DeviceArray.from_numpy(idx)):
        t = df.take(indices)
        assert t.length_unfiltered() == 777 and t.virtual_columns == {"v2": "v + 1"}
        for k, v in left.items():
            assert is_hbm(t.columns[k]) == hbm and as_list(t.columns[k]) == v[idx].tolist()
    f = df.filter("s >= 50").take(idx, filtered=False, dropfilter=False)
    assert f.filtered and len(f) == int((left["s"][idx] >= 50).sum())
    with pytest.raises(IndexError):
        df.take(np.array([0, 1000]))


@pytest.mark.parametrize("hbm", [False, True], ids=["host", "hbm"])
def test_index_of_filtered_frame(hbm):
    left, _ = random_tables(2000, 10)
    ix = frame(left, hbm, "s >= 30")._index("k")
    ref = jn.index_np(left["k"], select=left["s"] >= 30)
    assert (len(ix), ix.has_duplicates) == (ref.length, ref.has_duplicates)
    probe = np.arange(-3, 30, dtype=np.int32)
    assert ix.map_index(probe).tolist() == jn.map_index_np(ref, probe)[0].tolist()


@pytest.mark.parametrize("hbm", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("all_matched", [True, False], ids=["matched", "masked"])
def test_joined_frame_feeds_groupby_and_binby(all_matched, hbm):
    """A groupby / sum(binby=...) over a joined dimension column equals the same computed from
    join_np's arrays, on the all-matched path (columns stay where they were) and on the masked
    path (unmatched rows are missing: they fall out of the groups and the bins)."""
    import vaex_amd
    left, right = random_tables()
    if all_matched:
        known = np.isin(left["k"], right["k"])
        left = {k: v[known] for k, v in left.items()}
    cols, _ = jn.join_np(left, right, on="k")
    res = frame(left, hbm).join(frame(right, hbm), on="k")
    g, v = np.ma.asarray(cols["g"]), cols["v"]
    ok = ~np.ma.getmaskarray(g)
    exp_sum = np.array([v[ok & (g.filled(-1) == j)].sum() for j in range(9)])
    exp_cnt = np.array([int((ok & (g.filled(-1) == j)).sum()) for j in range(9)])
    # sums of ~330 standard-normal float64 values in another order: at most about
    # (n - 1) * 2^-53 * sum|v| = 330 * 1.1e-16 * 270 = 1e-11 apart
    tol = dict(rtol=0, atol=1e-10)
    got = res.sum("v", binby="g", limits=[-0.5, 8.5], shape=9)
    assert np.allclose(np.asarray(got), exp_sum, **tol)
    # the same groupby over a host frame of join_np's arrays: the same groups (the missing
    # group, when there is one, in the same place and form), counts and sums
    agg = {"n": vaex_amd.agg.count(), "s": vaex_amd.agg.sum("v")}
    dfg = res.groupby("g", agg=agg, sort=True)
    ref = vaex_amd.from_arrays(**cols).groupby("g", agg=agg, sort=True)
    assert list(dfg.columns) == list(ref.columns)
    assert as_list(dfg.columns["g"]) == as_list(ref.columns["g"])
    assert as_list(dfg.columns["n"]) == as_list(ref.columns["n"])
    assert np.allclose(np.asarray(dfg.columns["s"]), np.asarray(ref.columns["s"]), **tol)
    # and against numpy for the groups 0..8
    keys = as_list(dfg.columns["g"])
    for j in range(9):
        if exp_cnt[j]:
            i = keys.index(j)
            assert np.asarray(dfg.columns["n"])[i] == exp_cnt[j]
            assert np.isclose(np.asarray(dfg.columns["s"])[i], exp_sum[j], **tol)
        else:
            assert j not in keys
