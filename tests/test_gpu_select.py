"""Selections on an HBM frame: select_lasso (vh_pnpoly), chains of modes, undo / redo and the
per-block mask cache, through the aggregations that take a selection.  Grids against the
oracle with the NumPy mask of tests/pnpoly_np.py: counts exact, sums within the project's 1e-6
relative tolerance."""
import numpy as np
import pytest

from oracle import oracle
from pnpoly_np import pnpoly_np

pytestmark = pytest.mark.gpu

N = 200_003
LIM = [[-4, 4], [-4, 4]]
BINS = 64
LASSO = ([-1.5, 0.25, 2.0, 1.0, 2.5, -0.5, -2.0], [-1.0, -2.5, -0.5, 0.25, 2.0, 1.0, 2.25])  # concave
LASSO2 = ([-3.0, 0.0, 3.0, 0.0], [0.0, -1.0, 0.0, 1.0])


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(42)
    x, y, w = rng.normal(size=N), rng.normal(size=N), rng.random(N)
    x[::1013], y[7::1019] = np.nan, np.nan
    k = rng.integers(-3, 4, N).astype(np.int32)
    d = dict(x=x, y=y, w=w, k=k)
    for a in d.values():
        a.setflags(write=False)
    d["lasso"] = pnpoly_np(x, y, *LASSO)
    d["lasso2"] = pnpoly_np(x, y, *LASSO2)
    assert 0.1 < d["lasso"].mean() < 0.9 and 0.1 < d["lasso2"].mean() < 0.9
    return d


@pytest.fixture
def df(data):
    import vaex_amd
    from vaex_amd.device import DeviceArray
    return vaex_amd.from_arrays(**{c: DeviceArray.from_numpy(data[c]) for c in "xywk"})


def grids(data, keep):
    ob = [oracle.Binner("scalar", data[c], vmin=-4, vmax=4, bins=BINS) for c in "xy"]
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    count = oracle.extract_central_part(oracle.compute_grid(ob, "count", mask=keep))
    total = oracle.extract_central_part(oracle.compute_grid(ob, "sum", data=data["w"], mask=keep))
    return count, total


def check_grids(df, data, keep, selection=True):
    count, total = grids(data, keep)
    kw = dict(binby=["x", "y"], limits=LIM, shape=BINS, selection=selection)
    np.testing.assert_array_equal(np.asarray(df.count(**kw)), count)
    np.testing.assert_allclose(np.asarray(df.sum("w", **kw)), total, rtol=1e-6, atol=1e-9)
    with np.errstate(all="ignore"):
        np.testing.assert_allclose(np.asarray(df.mean("w", **kw)), total / count, rtol=1e-6, atol=1e-9, equal_nan=True)


def test_lasso_grids(df, data):
    df.select_lasso("x", "y", *LASSO)
    check_grids(df, data, data["lasso"])
    assert df.selected_length() == int(data["lasso"].sum())
    assert int(df.count(selection=df.get_selection())) == int(data["lasso"].sum())  # a Selection object
    counts = np.asarray(df.count(selection=[True, "w > 0.5", None]))
    assert counts.tolist() == [int(data["lasso"].sum()), int((data["w"] > 0.5).sum()), N]


def test_chain(df, data):
    """expression -> lasso (and) -> expression (subtract) -> inverse."""
    df.select("w > 0.25")
    df.select_lasso("x", "y", *LASSO, mode="and")
    df.select("x > 0.5", mode="subtract")
    keep = (data["w"] > 0.25) & data["lasso"] & ~(data["x"] > 0.5)
    check_grids(df, data, keep)
    df.select_inverse()
    check_grids(df, data, ~keep)
    for mode, want in [("or", data["lasso2"] | ~keep), ("xor", data["lasso2"] ^ ~keep)]:
        df.select_lasso("x", "y", *LASSO2, mode=mode)
        assert df.selected_length() == int(want.sum())
        df.selection_undo()


def test_lasso_on_filtered_frame(df, data):
    dff = df[df.w < 0.7]
    dff.select_lasso("x", "y", *LASSO)
    check_grids(dff, data, data["lasso"] & (data["w"] < 0.7))
    lo, hi = dff.minmax("w", selection=True)  # the inverted mask of the min / max kernel
    sel = data["w"][data["lasso"] & (data["w"] < 0.7)]
    assert (lo, hi) == (sel.min(), sel.max())


def test_cast_path(df, data):
    """An int32 x expression and a float expression: evaluated (and cast to float64) on the device."""
    poly = ([-2.5, 1.5, 1.5, -2.5], [-1.0, -1.0, 1.0, 1.0])
    df.select_lasso("k", "y", *poly)
    check_grids(df, data, pnpoly_np(data["k"], data["y"], *poly))
    df.select_lasso("x * 2", "k + y", *poly)
    with np.errstate(all="ignore"):
        check_grids(df, data, pnpoly_np(data["x"] * 2, data["k"] + data["y"], *poly))


def test_value_counts_minmax_percentile(df, data):
    import vaex_amd
    from vaex_amd.device import DeviceArray
    df.select_lasso("x", "y", *LASSO)
    keep = data["lasso"]
    vc = df.value_counts("k", selection=True)
    keys, counts = np.unique(data["k"][keep], return_counts=True)
    assert dict(zip(vc.index.tolist(), vc.values.tolist())) == dict(zip(keys.tolist(), counts.tolist()))
    assert sorted(df.unique("k", selection=True)) == keys.tolist()
    lo, hi = df.minmax("w", selection=True)
    assert (lo, hi) == (data["w"][keep].min(), data["w"][keep].max())
    # the same rows as a frame of their own give the same count grid, so the same percentiles
    sub = vaex_amd.from_arrays(w=DeviceArray.from_numpy(data["w"][keep]))
    kw = dict(percentile_limits=[0, 1], percentile_shape=1024)
    got = df.percentile_approx("w", [25, 50, 90], selection=True, **kw)
    np.testing.assert_array_equal(got, sub.percentile_approx("w", [25, 50, 90], **kw))
    np.testing.assert_allclose(got, np.percentile(data["w"][keep], [25, 50, 90]), atol=2e-3)


def test_undo_redo(df, data):
    df.select_lasso("x", "y", *LASSO)
    df.select_lasso("x", "y", *LASSO2, mode="and")
    both = int((data["lasso"] & data["lasso2"]).sum())
    assert df.selected_length() == both
    df.selection_undo()
    assert df.selected_length() == int(data["lasso"].sum())
    df.selection_redo()
    assert df.selected_length() == both
    df.selection_undo()
    df.selection_undo()
    assert not df.has_selection() and df.selection_can_redo()


def test_mask_cache(df, data, monkeypatch):
    """The per-block cache keys a lasso by its to_dict(): the same lasso is evaluated once,
    other vertices give a new mask."""
    from vaex_amd import superutils
    calls = []
    real = superutils.pnpoly
    monkeypatch.setattr(superutils, "pnpoly", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    kw = dict(binby=["x", "y"], limits=LIM, shape=BINS, selection=True)
    df.select_lasso("x", "y", *LASSO)
    first = np.asarray(df.count(**kw))
    assert len(calls) == 1
    np.testing.assert_array_equal(np.asarray(df.count(**kw)), first)
    df.sum("w", **kw)
    assert len(calls) == 1
    df.select_lasso("x", "y", *LASSO2)
    np.testing.assert_array_equal(np.asarray(df.count(**kw)), grids(data, data["lasso2"])[0])
    assert len(calls) == 2
    df.selection_undo()  # the first lasso again: its mask is still there
    np.testing.assert_array_equal(np.asarray(df.count(**kw)), first)
    assert len(calls) == 2
    np.testing.assert_array_equal(first, grids(data, data["lasso"])[0])


def test_folded_chain_is_one_expression(df, data, monkeypatch):
    """An expression-only chain gives the grids of the hand-written combined expression, and
    runs as that one device expression: no lasso kernel, no mask combine."""
    from vaex_amd import superutils
    from vaex_amd.dataframe import DataFrame
    exprs = []
    real = DataFrame._eval_device
    monkeypatch.setattr(DataFrame, "_eval_device", lambda self, e, i1, i2: exprs.append(e) or real(self, e, i1, i2))
    monkeypatch.setattr(superutils, "pnpoly", None)
    monkeypatch.setattr(superutils, "mask_combine", None)
    df.select("w > 0.3")
    kw = dict(binby=["x", "y"], limits=LIM, shape=BINS)
    plain = np.asarray(df.count(selection=True, **kw))
    assert exprs == ["(w > 0.3)"]  # the plain selection: the expression, and the cache key, as before
    df.select("x < 0.5", mode="or")
    df.select("y > 1", mode="subtract")
    df.select("k == 2", mode="xor")
    df.select_inverse()
    del exprs[:]
    got = np.asarray(df.count(selection=True, **kw))
    hand = "~((((w > 0.3) | (x < 0.5)) & ~(y > 1)) ^ (k == 2))"
    assert exprs == ["(%s)" % hand]
    np.testing.assert_array_equal(got, np.asarray(df.count(selection=hand, **kw)))
    with np.errstate(all="ignore"):
        keep = ~((((data["w"] > 0.3) | (data["x"] < 0.5)) & ~(data["y"] > 1)) ^ (data["k"] == 2))
    np.testing.assert_array_equal(got, grids(data, keep)[0])
    np.testing.assert_array_equal(plain, grids(data, data["w"] > 0.3)[0])
    df.select_box(["x", "y"], [(-1, 0.5), (2, -0.25)])
    df.select_circle("x", "y", 0.25, -0.5, 1.25, mode="or")
    with np.errstate(all="ignore"):
        keep = ((data["x"] >= -1) & (data["x"] <= 0.5) & (data["y"] >= -0.25) & (data["y"] <= 2)) | \
            ((data["x"] - 0.25) ** 2 + (data["y"] + 0.5) ** 2 <= 1.25 ** 2)
    np.testing.assert_array_equal(np.asarray(df.count(selection=True, **kw)), grids(data, keep)[0])


def test_lasso_moves_only_vertices(df, data, monkeypatch):
    """A lasso selection on an HBM frame copies nothing but the vertex arrays (inside
    vh_pnpoly) to the device and reads nothing back."""
    from vaex_amd import _lib
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real(name, *a))
    dff = df[df.w < 0.7]
    dff.select("w > 0.1")
    dff.select_lasso("k", "y", *LASSO, mode="and")
    dff.select_inverse()
    mask = dff.device_keep_mask(0, N, True)
    monkeypatch.undo()
    assert "vh_pnpoly" in names and "vh_mask_combine" in names
    assert not [name for name in names if "memcpy" in name or "download" in name]
    with np.errstate(all="ignore"):
        want = (data["w"] < 0.7) & ~((data["w"] > 0.1) & pnpoly_np(data["k"], data["y"], *LASSO))
    np.testing.assert_array_equal(mask.to_numpy().view(np.uint8), want.view(np.uint8))


def test_select_non_missing(df, data):
    df.select_non_missing()
    assert df.selected_length() == int((~np.isnan(data["x"]) & ~np.isnan(data["y"])).sum())
    df.select_non_missing(drop_nan=False)  # HBM columns carry no masks: every row
    assert df.selected_length() == N
    df.select_lasso("x", "y", *LASSO)
    df.select_non_missing(column_names=["x"], mode="or")
    assert df.selected_length() == int((data["lasso"] | ~np.isnan(data["x"])).sum())
