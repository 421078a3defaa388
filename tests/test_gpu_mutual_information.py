"""mutual_information: the device finish of a count grid (vh_agg_mutual_information) against the
NumPy restatement of the reference's finish (tests/mutual_information_np.py) applied to
``np.asarray`` of the same count grid, within the restatement's derived per-cell tolerance
``(n + 64) * 2**-52 * (1 + sum|t|)``; empty cells and repeated calls compare exactly.

The host picks the kernel mapping from the central slab alone (csrc/mutual_information.hip):
``Mx * My <= MI_CELL_ITEMS = 4096`` takes one workgroup per outer cell, larger slabs are split
into tiles of at most ``MI_TILE_W = 1024`` columns and about 4096 entries over several
workgroups per cell.  ``test_mapping_boundaries`` sits just below, at and just above both."""
import numpy as np
import pytest

import mutual_information_np as mi_np

pytestmark = pytest.mark.gpu


def vx():
    import vaex_amd
    return vaex_amd


def make_count(Mx, My, outer_bins=()):
    """An AggCount_int64 over scalar binners: x, y, then the outer axes."""
    from vaex_amd import superagg
    binners = [superagg.BinnerScalar_float64("x", 0, 1, Mx), superagg.BinnerScalar_float64("y", 0, 1, My)]
    binners += [superagg.BinnerScalar_float64("o%d" % i, 0, 1, b) for i, b in enumerate(outer_bins)]
    grid = superagg.Grid(binners)
    return grid, superagg.AggCount_int64(grid)


def special_slab(kind, Mx, My, rng):
    slab = np.zeros((Mx, My), np.int64)
    if kind == "onebin":
        slab[Mx // 2, My // 3] = 1000
    elif kind == "diagonal":
        k = np.arange(min(Mx, My))
        slab[k, k] = 7
    elif kind == "big":  # totals below 2^53, marginal products above it
        slab[...] = rng.integers(0, 4, size=(Mx, My)).astype(np.int64) << 40
    elif kind == "product":
        slab[...] = np.outer(rng.integers(1, 9, size=Mx), rng.integers(1, 9, size=My))
    # "empty": all zero
    return slab


SPECIALS = ("empty", "onebin", "diagonal", "big", "product")


def fill(agg, Mx, My, outer_bins, rng, specials=()):
    """Random non-zero junk in every edge slot of x, y and the outer axes (a finish that reads one
    of them is off by far more than the tolerance), sparse random counts in the central part, and
    the special slabs in every other central cell from the second on.  Returns the live view and
    the outer cells that hold the specials."""
    view = np.asarray(agg)
    shape = (Mx + 3, My + 3) + tuple(b + 3 for b in outer_bins)
    assert view.shape == shape
    view[...] = rng.integers(1, 20, size=shape)
    central = rng.integers(0, 20, size=(Mx, My) + tuple(outer_bins))
    central[rng.random(central.shape) < 0.3] = 0
    view[(slice(2, -1),) * len(shape)] = central
    cells = list(np.ndindex(*outer_bins))
    placed = {}
    if specials:
        assert len(cells) >= 2 * len(specials)
        for kind, cell in zip(specials, cells[1::2]):
            view[(slice(2, -1), slice(2, -1)) + tuple(i + 2 for i in cell)] = special_slab(kind, Mx, My, rng)
            placed[kind] = cell
    return view, placed


def check(agg, view):
    expected, tol = mi_np.mutual_information_from_counts(view.copy())
    got = agg.mutual_information()
    assert got.shape == expected.shape and got.dtype == np.float64 and got.flags["C_CONTIGUOUS"]
    err = np.abs(got - expected)
    assert (err <= tol).all(), (float(err.max()), float(tol.min()), got, expected)
    assert (got[expected == 0.0] == 0.0).all()
    return got, expected, tol


# ---- grids written through the live view (no binning) ------------------------------------------
@pytest.mark.parametrize("Mx,My", [(1, 1), (1, 33), (33, 1), (2, 3), (61, 67), (64, 64), (256, 256), (300, 40),
                                   (520, 523)])
def test_no_outer_axis(Mx, My):
    """Below a wave, odd sizes, Mx != My and longer than a workgroup row; 520 x 523 takes 75
    tiles of one cell (more than the 64 lanes of the final sum)."""
    rng = np.random.default_rng(Mx * 1000 + My)
    grid, agg = make_count(Mx, My)
    got, expected, _ = check(agg, fill(agg, Mx, My, (), rng)[0])
    assert got.ndim == 0
    if Mx == 1 or My == 1:
        assert abs(got) < 1e-13  # 0 by arithmetic


@pytest.mark.parametrize("Mx,My", [(16, 12), (35, 35)])
@pytest.mark.parametrize("outer", [(5,), (63,), (64,), (65,), (5, 3), (3, 4, 5), (2, 2, 2, 2)])
def test_outer_axes(outer, Mx, My):
    rng = np.random.default_rng(len(outer) * 1000 + sum(outer) + Mx)
    grid, agg = make_count(Mx, My, outer)
    got, _, _ = check(agg, fill(agg, Mx, My, outer, rng)[0])
    assert got.shape == outer


def test_many_small_cells():
    rng = np.random.default_rng(200)
    grid, agg = make_count(8, 8, (200,))
    check(agg, fill(agg, 8, 8, (200,), rng)[0])


@pytest.mark.parametrize("Mx,My", [(16, 12), (70, 130)])
def test_mixed_cells(Mx, My):
    """An empty cell, one occupied bin, a diagonal, counts of k << 40 and an outer-product cell
    among random ones, in the per-cell mapping (16 x 12) and in the split one (70 x 130)."""
    rng = np.random.default_rng(Mx)
    grid, agg = make_count(Mx, My, (11,))
    view, placed = fill(agg, Mx, My, (11,), rng, SPECIALS)
    got, expected, tol = check(agg, view)
    assert got[placed["empty"]] == 0.0 and np.signbit(got[placed["empty"]]) == False  # noqa: E712
    assert abs(got[placed["onebin"]]) <= tol[placed["onebin"]]
    assert abs(got[placed["diagonal"]] - np.log(min(Mx, My))) <= tol[placed["diagonal"]]
    assert abs(got[placed["product"]]) <= tol[placed["product"]]
    assert got[placed["big"]] > 0
    others = [c for c in np.ndindex(11) if c not in placed.values()]
    assert all(got[c] > 0 for c in others)


@pytest.mark.parametrize("Mx,My,outer", [(63, 65, (3,)), (64, 64, (3,)), (65, 64, (3,)),
                                         (1023, 5, ()), (1024, 5, ()), (1025, 5, (2,))])
def test_mapping_boundaries(Mx, My, outer):
    """MI_CELL_ITEMS = 4096 entries: 63 x 65 = 4095 and 64 x 64 take one workgroup per cell,
    65 x 64 = 4160 the split mapping.  MI_TILE_W = 1024 columns: 1023 and 1024 are one tile wide,
    1025 two (and, at 4 rows per tile, two tiles high)."""
    rng = np.random.default_rng(Mx * 7 + My)
    grid, agg = make_count(Mx, My, outer)
    check(agg, fill(agg, Mx, My, outer, rng)[0])


@pytest.mark.parametrize("Mx,My,outer", [(520, 523, ()), (35, 35, (5, 3))])
def test_deterministic(Mx, My, outer):
    """Two calls on one grid agree bit for bit, in the split and in the per-cell mapping."""
    rng = np.random.default_rng(99)
    grid, agg = make_count(Mx, My, outer)
    fill(agg, Mx, My, outer, rng)
    first = agg.mutual_information()
    np.testing.assert_array_equal(agg.mutual_information(), first)
    np.testing.assert_array_equal(agg.mutual_information(), first)


# ---- binned grids -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 5, 2000, 200000])
def test_binned_grid(n):
    from vaex_amd import superagg
    from vaex_amd.device import DeviceArray
    rng = np.random.default_rng(n + 1)
    x, o = rng.normal(size=n), rng.normal(size=n)
    y = 0.5 * x + rng.normal(size=n)
    x[rng.random(n) < 0.03] = np.nan
    binners = [superagg.BinnerScalar_float64("x", -3, 3, 32), superagg.BinnerScalar_float64("y", -3, 3, 32),
               superagg.BinnerScalar_float64("o", -2, 2, 5)]
    for b, col in zip(binners, (x, y, o)):
        b.set_data(DeviceArray.from_numpy(col))
    grid = superagg.Grid(binners)
    agg = superagg.AggCount_int64(grid)
    grid.bin([agg], n)
    got = agg.mutual_information()
    counts = np.asarray(agg)
    assert counts.sum() == n
    expected, tol = mi_np.mutual_information_from_counts(counts)
    assert expected.shape == (5,)
    if n == 200000:  # a condition on the inputs: the comparison is not 0 against 0
        assert np.isfinite(expected).all() and (expected > 0).all()
    assert (np.abs(got - expected) <= tol).all()


# ---- DataFrame level ---------------------------------------------------------------------------
def restated(df, x, y, binby=(), limits=None, shape=128, mi_shape=256, mi_limits=None, selection=False):
    """The restatement fed by df.count(..., edges=True) over [x, y] + binby."""
    binby = list(binby)
    sel = selection if selection else None
    mi_limits = mi_limits or [[float(v) for v in df.limits(e, "minmax", selection=sel)] for e in (x, y)]
    outer_limits = list(limits) if limits is not None else [None] * len(binby)  # None: minmax (or a category)
    shapes = list(shape) if isinstance(shape, (list, tuple)) else [shape] * len(binby)
    mi_shapes = list(mi_shape) if isinstance(mi_shape, (list, tuple)) else [mi_shape] * 2
    counts = df.count(binby=[x, y] + binby, limits=list(mi_limits) + outer_limits, shape=mi_shapes + shapes,
                      selection=selection, edges=True)
    return mi_np.mutual_information_from_counts(np.asarray(counts))


def close(got, expected_tol):
    expected, tol = expected_tol
    got = np.asarray(got)
    assert got.shape == expected.shape
    assert (np.abs(got - expected) <= tol).all(), (got, expected, tol)


@pytest.fixture(scope="module")
def frame():
    """100 000 normal rows: x (3 % NaN), y, w = y + noise, a float32 and an int32 column, a
    category; HBM."""
    from vaex_amd.device import DeviceArray
    rng = np.random.default_rng(7)
    n = 100000
    cols = dict(x=rng.normal(size=n), y=rng.normal(size=n),
                f=rng.normal(size=n).astype(np.float32), i=rng.integers(-500, 500, size=n).astype(np.int32),
                c=rng.integers(0, 4, size=n).astype(np.int64))
    cols["w"] = cols["y"] + 0.3 * rng.normal(size=n)
    cols["x"][rng.random(n) < 0.03] = np.nan
    return cols, vx().from_arrays(**{k: DeviceArray.from_numpy(v) for k, v in cols.items()})


def test_df_known_answer():
    """tests/agg_test.py:442-447."""
    x = np.arange(10.)
    df = vx().from_arrays(x=x, y=x ** 2)
    got = df.mutual_information("x", "y", mi_shape=32)
    assert np.ndim(got) == 0
    np.testing.assert_almost_equal(got, 2.043192, 6)
    close(df.mutual_information("x", "y", mi_shape=32, mi_limits=[[0, 9], [0, 81]]),
          restated(df, "x", "y", mi_shape=32))


def test_df_one_pair_and_dependence(frame):
    cols, df = frame
    got = df.mutual_information("x", "y")
    assert isinstance(got, np.ndarray) and got.ndim == 0
    close(got, restated(df, "x", "y"))
    dependent = df.mutual_information("y", "w", mi_shape=64)
    independent = df.mutual_information("y", "f", mi_shape=64)
    close(dependent, restated(df, "y", "w", mi_shape=64))
    # rho = 0.96: -log(1 - rho^2) / 2 = 1.25, a little less on 64 bins; independent columns leave
    # the estimator's bias, about (bins - 1)^2 / (2 n) = 0.02
    assert dependent > 0.8 > 0.1 > independent > 0


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_df_binby(frame, nd):
    """The shapes of the reference's test (tests/agg_test.py:449-462): (2,), (2, 3), (2, 3, 4)."""
    cols, df = frame
    binby, limits, shape = ["y", "f", "i"][:nd], [[-2, 2], [-2, 2], [-500, 500]][:nd], (2, 3, 4)[:nd]
    got = df.mutual_information("x", "w", mi_shape=(32, 24), binby=binby, limits=limits, shape=shape)
    assert got.shape == shape
    close(got, restated(df, "x", "w", binby=binby, limits=limits, shape=shape, mi_shape=(32, 24)))
    if nd == 1:
        default = df.mutual_information("x", "w", mi_shape=(32, 24), binby="y", shape=2)  # minmax limits
        close(default, restated(df, "x", "w", binby=["y"], shape=2, mi_shape=(32, 24)))


def test_df_lists_pairs_and_sort(frame):
    cols, df = frame
    pairs = [["x", "y"], ["y", "w"], ["x", "f"]]
    each = [restated(df, a, b, mi_shape=64) for a, b in pairs]
    lists = df.mutual_information(["x", "y", "x"], ["y", "w", "f"], mi_shape=64)
    paired = df.mutual_information(pairs, mi_shape=64)
    assert lists.shape == (3,) and paired.shape == (3,)
    np.testing.assert_array_equal(lists, paired)
    for k in range(3):
        close(paired[k], each[k])
    one = df.mutual_information([["y", "w"]], mi_shape=64)
    assert one.shape == (1,) and one[0] == paired[1]
    values, order = df.mutual_information(pairs, mi_shape=64, sort=True)
    assert (np.diff(values) <= 0).all() and order[0] == ["y", "w"]
    assert sorted(map(tuple, order)) == sorted(map(tuple, pairs))
    for v, pair in zip(values, order):
        assert v == paired[pairs.index(pair)]
    with pytest.raises(ValueError, match="binby"):  # per-cell values have no order over the pairs
        df.mutual_information(pairs, mi_shape=16, binby="y", limits=[-2, 2], shape=3, sort=True)
    binned = df.mutual_information(pairs, mi_shape=16, binby="y", limits=[-2, 2], shape=3)
    assert binned.shape == (3, 3)
    close(binned[1], restated(df, "y", "w", binby=["y"], limits=[[-2, 2]], shape=3, mi_shape=16))


def test_df_explicit_limits(frame):
    cols, df = frame
    lims = [[-1.5, 2.0], [-1.0, 1.0]]
    got = df.mutual_information("x", "y", mi_limits=lims, mi_shape=40)
    close(got, restated(df, "x", "y", mi_limits=lims, mi_shape=40))
    assert got != df.mutual_information("x", "y", mi_shape=40)
    close(df.mutual_information("x", "y", mi_limits="minmax", mi_shape=40), restated(df, "x", "y", mi_shape=40))
    per_pair = df.mutual_information([["x", "y"], ["y", "w"]], mi_limits=[lims, [[-2, 2], [-3, 3]]], mi_shape=40)
    assert per_pair[0] == got
    close(per_pair[1], restated(df, "y", "w", mi_limits=[[-2, 2], [-3, 3]], mi_shape=40))


def test_df_selection_and_filter(frame):
    cols, df = frame
    df = df.copy()
    df.select("y > 0.5")
    got = df.mutual_information("x", "w", selection=True, mi_shape=48)
    close(got, restated(df, "x", "w", selection=True, mi_shape=48))
    assert got != df.mutual_information("x", "w", mi_shape=48)
    dff = df.filter("y < 0")
    gotf = dff.mutual_information("x", "w", binby="f", shape=4, limits=[-1, 1], mi_shape=48)
    assert gotf.shape == (4,)
    close(gotf, restated(dff, "x", "w", binby=["f"], limits=[[-1, 1]], shape=4, mi_shape=48))


def test_df_host_columns(frame):
    cols, _ = frame
    df = vx().from_arrays(**{k: v[:20000] for k, v in cols.items()})
    got = df.mutual_information("x", "w", binby="y", shape=7, limits=[-2, 2], mi_shape=20)
    close(got, restated(df, "x", "w", binby=["y"], limits=[[-2, 2]], shape=7, mi_shape=20))


def test_df_float32_and_int32(frame):
    cols, df = frame
    got = df.mutual_information("f", "i", mi_shape=50)
    close(got, restated(df, "f", "i", mi_shape=50))
    assert got > 0


def test_df_categorised_binby(frame):
    cols, df = frame
    dfc = df.categorize("c", min_value=0, max_value=3)
    got = dfc.mutual_information("y", "w", binby="c", mi_shape=32)
    assert got.shape == (4,)
    close(got, restated(dfc, "y", "w", binby=["c"], mi_shape=32))
    assert (got > 0.5).all()


def test_df_delay(frame):
    cols, df = frame
    p = df.mutual_information("y", "w", mi_shape=32, delay=True)
    q = df.mutual_information([["y", "w"]], mi_shape=32, delay=True)
    df.execute()
    assert p.get().ndim == 0 and p.get() == q.get()[0]
    assert p.get() == df.mutual_information("y", "w", mi_shape=32)


# ---- argument errors ---------------------------------------------------------------------------
def test_argument_errors():
    from vaex_amd import _lib, superagg
    grid, agg = make_count(16, 12, (5,))
    np.asarray(agg)[...] = 1
    L = _lib.lib()
    out = np.empty(5, np.float64)

    def rc(a, items, ptr=out.ctypes.data):
        return L.vh_agg_mutual_information(a._handle, ptr, items)

    assert rc(agg, 5) == 0
    assert rc(agg, 4) == 4 and b"size" in L.vh_last_error()
    assert rc(agg, 5, None) == 4 and b"output" in L.vh_last_error()
    total = superagg.AggSum_float64(grid)
    assert rc(total, 5) == 4 and b"AggCount" in L.vh_last_error()
    # an int64 grid that is not a count grid (every AggCount grid is int64, so the kind decides)
    assert rc(superagg.AggMax_int64(grid), 5) == 4 and b"AggCount" in L.vh_last_error()
    one = superagg.AggCount_int64(superagg.Grid([superagg.BinnerScalar_float64("x", 0, 1, 8)]))
    assert rc(one, 1) == 4 and b"2 binners" in L.vh_last_error()
    assert rc(superagg.AggCount_int64(superagg.Grid([])), 1) == 4 and b"2 binners" in L.vh_last_error()
    for Mx, My, axis in [(0, 8, b"x axis"), (8, 0, b"y axis")]:  # shape 3: no central bin
        _, thin = make_count(Mx, My)
        assert rc(thin, 1) == 4 and axis in L.vh_last_error()
    # no outer central cell: nothing to write, also without an output
    _, none = make_count(8, 8, (0,))
    assert rc(none, 0, None) == 0
    assert rc(none, 1) == 4
    # more than MAX_DIM (16) binners never reach the finish: the grid refuses them
    with pytest.raises(_lib.HipError):
        superagg.Grid([superagg.BinnerScalar_float64("b%d" % i, 0, 1, 1) for i in range(17)])
    with pytest.raises(_lib.HipError):
        total.mutual_information()
    with pytest.raises(_lib.HipError):
        one.mutual_information()


def test_df_limits_resolved_once(frame, monkeypatch):
    """An expression that occurs in several pairs gets one min/max pass per call, not one per pair."""
    cols, df = frame
    df = df.copy()
    calls = []
    minmax = df.minmax
    monkeypatch.setattr(df, "minmax", lambda e, **kw: (calls.append(str(e)), minmax(e, **kw))[1])
    pairs = [["x", "y"], ["y", "w"], ["x", "w"]]
    got = df.mutual_information(pairs, mi_shape=32)
    assert sorted(calls) == ["w", "x", "y"]
    for k, (a, b) in enumerate(pairs):
        close(got[k], restated(df, a, b, mi_shape=32))
