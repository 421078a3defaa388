"""percentile_approx / median_approx: the device finish of a count grid (vh_agg_percentile)
against the NumPy restatement of the reference's finish (tests/percentile_np.py) applied to
``np.asarray`` of the same count grid.  Every comparison is bit-exact (NaN equal to NaN): the
kernel does the reference's float64 operations in the reference's order."""
import numpy as np
import pytest

import percentile_np

pytestmark = pytest.mark.gpu

PCTS = [0, 1, 25, 50, 75, 99, 99.9, 100]
LO, HI = -1.25, 3.5


def vx():
    import vaex_amd
    return vaex_amd


def make_count(outer_bins, P):
    """An AggCount_int64 over scalar binners: the outer axes, then the percentile axis."""
    from vaex_amd import superagg
    binners = [superagg.BinnerScalar_float64("o%d" % i, 0, 1, b) for i, b in enumerate(outer_bins)]
    binners.append(superagg.BinnerScalar_float64("p", LO, HI, P))
    grid = superagg.Grid(binners)
    return grid, superagg.AggCount_int64(grid)


def special_row(kind, P, rng):
    """One cell's percentile axis (P + 3 slots), the NaN slot non-zero in every kind."""
    row = np.zeros(P + 3, np.int64)
    if kind == "onebin":  # all the mass in one bin
        row[2 + P // 2] = 1000
    elif kind == "big":  # counts of 2^40 (totals stay below 2^53)
        row[1:] = rng.integers(0, 4, size=P + 2).astype(np.int64) << 40
    elif kind == "exact" and P >= 4:
        # total 9: p = 50 gives v = t = 5 = cum at slot 3 exactly (the strict `<` of the edge
        # search decides the edges); p = 25 / 75 give 2.5 / 7.5
        row[2], row[3], row[5] = 3, 2, 4
    # "zero": an empty cell
    row[0] = 7
    return row


def fill(agg, outer_bins, P, rng, specials=("onebin", "zero", "big", "exact")):
    """Random counts in every slot (NaN, underflow, overflow and the outer edge cells, which the
    finish must ignore, included), then the special cells in the first central cells."""
    view = np.asarray(agg)
    shape = tuple(b + 3 for b in outer_bins) + (P + 3,)
    assert view.shape == shape
    view[...] = rng.integers(0, 20, size=shape)
    cells = list(np.ndindex(*outer_bins))
    if len(cells) >= 2 * len(specials):
        for kind, cell in zip(specials, cells[1::2]):
            view[tuple(i + 2 for i in cell)] = special_row(kind, P, rng)
    return view


def check(agg, view, pcts=PCTS):
    expected = percentile_np.percentile_from_counts(view.copy(), pcts, LO, HI)
    got = agg.percentile(pcts, LO, HI)
    assert got.shape == expected.shape and got.dtype == np.float64
    np.testing.assert_array_equal(got, expected)
    return expected


# ---- grids written through the live view (no binning) ------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 3, 61, 256, 1024, 65536])
def test_no_outer_axis(P):
    rng = np.random.default_rng(P)
    grid, agg = make_count((), P)
    check(agg, fill(agg, (), P, rng))


@pytest.mark.parametrize("kind", ["onebin", "zero", "big", "exact"])
@pytest.mark.parametrize("P", [61, 1024])
def test_no_outer_axis_special_cells(P, kind):
    rng = np.random.default_rng(5)
    grid, agg = make_count((), P)
    view = np.asarray(agg)
    view[...] = special_row(kind, P, rng)
    expected = check(agg, view)
    if kind == "zero":
        assert np.isnan(expected[1:-1]).all() and expected[0] == LO and expected[-1] == HI


@pytest.mark.parametrize("P", [16, 61])
@pytest.mark.parametrize("cells", [1, 63, 64, 65, 200])
def test_one_outer_axis(cells, P):
    """63 cells and fewer: one workgroup per cell along the axis; 64 and more: lanes over cells."""
    rng = np.random.default_rng(cells * 100 + P)
    grid, agg = make_count((cells,), P)
    check(agg, fill(agg, (cells,), P, rng))


@pytest.mark.parametrize("outer,P", [((5, 3), 64), ((67, 9), 64), ((3, 4, 5), 16), ((70,), 300)])
def test_outer_axes(outer, P):
    """Two and three outer axes (the 3 edge cells per axis row skipped by index decode, not a
    multiple of the 64-cell workgroup); (70,) x 300: the 8-segment split of a long axis."""
    rng = np.random.default_rng(len(outer) * 1000 + P)
    grid, agg = make_count(outer, P)
    check(agg, fill(agg, outer, P, rng))


def test_many_unsorted_percentages():
    """More than one launch's 16 percentages, unsorted and repeated: each lands in its own row."""
    rng = np.random.default_rng(11)
    pcts = [50, 99.9, 0, 3, 75, 50, 100, 12.5, 1, 97, 25, 0.1, 66, 33, 10, 90, 5, 95, 42, 50.5, 80]
    for outer in [(), (66,)]:
        grid, agg = make_count(outer, 40)
        check(agg, fill(agg, outer, 40, rng), pcts)


# ---- binned grids -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 5, 2000, 200000])
def test_binned_grid(n):
    from vaex_amd import superagg
    from vaex_amd.device import DeviceArray
    rng = np.random.default_rng(n + 1)
    x, y, z = rng.normal(size=n), rng.normal(size=n), rng.normal(size=n)
    z[rng.random(n) < 0.03] = np.nan
    lo, hi = (float(np.nanmin(z)), float(np.nanmax(z))) if n else (0.0, 1.0)
    binners = [superagg.BinnerScalar_float64("x", -2, 2, 5), superagg.BinnerScalar_float64("y", -2, 2, 3),
               superagg.BinnerScalar_float64("z", lo, hi, 64)]
    for b, col in zip(binners, (x, y, z)):
        b.set_data(DeviceArray.from_numpy(col))
    grid = superagg.Grid(binners)
    agg = superagg.AggCount_int64(grid)
    grid.bin([agg], n)
    got = agg.percentile(PCTS, lo, hi)
    counts = np.asarray(agg)
    assert counts.sum() == n
    expected = percentile_np.percentile_from_counts(counts, PCTS, lo, hi)
    assert expected.shape == (len(PCTS), 5, 3)
    if n >= 20000:  # a condition on the inputs: the comparison is not NaN against NaN
        assert np.isfinite(expected[[2, 3, 4]]).all()
        assert np.isfinite(expected).mean() >= 0.9
    np.testing.assert_array_equal(got, expected)


# ---- DataFrame level ---------------------------------------------------------------------------
def restated(df, expr, pcts, binby=(), limits=None, shape=128, percentile_shape=1024, selection=False):
    """The restatement fed by df.count(..., edges=True) over binby + [expr]."""
    binby = list(binby)
    plim = [float(v) for v in df.limits(expr, "minmax", selection=selection if selection else None)]
    outer_limits = list(limits) if limits is not None else [None] * len(binby)  # None: minmax (or a category)
    shapes = list(shape) if isinstance(shape, (list, tuple)) else [shape] * len(binby)
    counts = df.count(binby=binby + [expr], limits=outer_limits + [plim], shape=shapes + [percentile_shape],
                      selection=selection, edges=True)
    return percentile_np.percentile_from_counts(np.asarray(counts), pcts, plim[0], plim[1])


@pytest.fixture(scope="module")
def frame():
    """100 000 normal rows: x (3 % NaN), y, a float32 and an int32 column, a category; HBM."""
    from vaex_amd.device import DeviceArray
    rng = np.random.default_rng(7)
    n = 100000
    cols = dict(x=rng.normal(size=n), y=rng.normal(size=n),
                f=rng.normal(size=n).astype(np.float32), i=rng.integers(-500, 500, size=n).astype(np.int32),
                c=rng.integers(0, 4, size=n).astype(np.int64))
    cols["x"][rng.random(n) < 0.03] = np.nan
    return cols, vx().from_arrays(**{k: DeviceArray.from_numpy(v) for k, v in cols.items()})


@pytest.mark.parametrize("values,side", [([0, 0, 10, 100, 200], "below"), ([0, 0, 90, 100, 200], "above")])
def test_df_median_reference_cases(values, side):
    """tests/percentile_approx_test.py:30-39."""
    df = vx().from_arrays(x=np.array(values, dtype="f8"))
    got = df.median_approx("x")
    assert np.ndim(got) == 0
    np.testing.assert_array_equal(got, restated(df, "x", [50.], percentile_shape=256)[0])
    assert (got < 10 and abs(got - 9.80392157) < 1e-8) if side == "below" else (got > 90 and abs(got - 90.58823529) < 1e-8)


def test_df_percentiles_fine_axis(frame):
    cols, df = frame
    pcts = [0, 25, 50, 75, 100]
    got = df.percentile_approx("x", pcts, percentile_shape=65536)
    assert got.shape == (5,)
    np.testing.assert_array_equal(got, restated(df, "x", pcts, percentile_shape=65536))
    # the approximation itself: close to the exact percentiles of the column
    exact = np.nanpercentile(cols["x"], [25, 50, 75])
    np.testing.assert_allclose(got[1:4], exact, atol=1e-3)


def test_df_two_expressions_two_percentages(frame):
    cols, df = frame
    got = df.percentile_approx(["x", "y"], [10, 90])
    assert got.shape == (2, 2)
    for k, e in enumerate(["x", "y"]):
        np.testing.assert_array_equal(got[k], restated(df, e, [10, 90]))
    one = df.percentile_approx(["x", "y"], 10)
    np.testing.assert_array_equal(one, got[:, 0])


def test_df_binby_minmax_limits(frame):
    cols, df = frame
    got = df.percentile_approx("x", [0, 50, 100], binby=["y"], shape=100, limits="minmax", percentile_shape=128)
    assert got.shape == (3, 100)
    exp = restated(df, "x", [0, 50, 100], binby=["y"], limits=["minmax"], shape=100, percentile_shape=128)
    np.testing.assert_array_equal(got, exp)
    assert (got[0] == got[0, 0]).all() and (got[2] == got[2, 0]).all()  # p = 0 / 100 broadcast
    med = df.median_approx("x", binby=["y", "f"], shape=(6, 5), limits=[[-2, 2], [-2, 2]])
    assert med.shape == (6, 5)
    np.testing.assert_array_equal(med, restated(df, "x", [50.], binby=["y", "f"], limits=[[-2, 2], [-2, 2]],
                                                shape=(6, 5), percentile_shape=256)[0])


def test_df_selection_and_filter(frame):
    cols, df = frame
    df = df.copy()
    df.select("y > 0.5")
    got = df.percentile_approx("x", [25, 75], selection=True, percentile_shape=512)
    np.testing.assert_array_equal(got, restated(df, "x", [25, 75], selection=True, percentile_shape=512))
    keep = cols["x"][cols["y"] > 0.5]
    np.testing.assert_allclose(got, np.nanpercentile(keep, [25, 75]), atol=0.05)
    dff = df.filter("y < 0")
    gotf = dff.percentile_approx("x", [25, 75], binby="f", shape=4, limits=[-1, 1], percentile_shape=512)
    assert gotf.shape == (2, 4)
    np.testing.assert_array_equal(gotf, restated(dff, "x", [25, 75], binby=["f"], limits=[[-1, 1]], shape=4,
                                                 percentile_shape=512))


def test_df_host_columns(frame):
    cols, _ = frame
    df = vx().from_arrays(**{k: v[:20000] for k, v in cols.items()})
    got = df.percentile_approx("x", [5, 50, 95], binby="y", shape=7, limits=[-2, 2], percentile_shape=200)
    np.testing.assert_array_equal(got, restated(df, "x", [5, 50, 95], binby=["y"], limits=[[-2, 2]], shape=7,
                                                percentile_shape=200))


@pytest.mark.parametrize("column", ["f", "i"])
def test_df_float32_and_int32(frame, column):
    cols, df = frame
    got = df.percentile_approx(column, [10, 50, 90], percentile_shape=300)
    np.testing.assert_array_equal(got, restated(df, column, [10, 50, 90], percentile_shape=300))
    np.testing.assert_allclose(got, np.percentile(cols[column].astype("f8"), [10, 50, 90]),
                               atol=0.05 if column == "f" else 5)


def test_df_categorised_binby(frame):
    cols, df = frame
    dfc = df.categorize("c", min_value=0, max_value=3)
    got = dfc.median_approx("y", binby="c")
    assert got.shape == (4,)
    np.testing.assert_array_equal(got, restated(dfc, "y", [50.], binby=["c"], percentile_shape=256)[0])
    for k in range(4):
        assert abs(got[k] - np.median(cols["y"][cols["c"] == k])) < 0.05


def test_df_delay(frame):
    cols, df = frame
    p = df.percentile_approx("y", 50, delay=True)
    q = df.median_approx("y", percentile_shape=1024, delay=True)
    df.execute()
    np.testing.assert_array_equal(p.get(), q.get())


# ---- argument errors ---------------------------------------------------------------------------
def test_argument_errors():
    from vaex_amd import _lib, superagg
    grid, agg = make_count((5,), 16)
    np.asarray(agg)[...] = 1
    L = _lib.lib()
    out = np.empty(2 * 5, np.float64)

    def rc(a, pcts, items):
        p = np.array(pcts, np.float64)
        return L.vh_agg_percentile(a._handle, p.ctypes.data, len(p), 0.0, 1.0, out.ctypes.data, items)

    assert rc(agg, [50, 75], 10) == 0
    assert rc(agg, [50, 101], 10) == 4 and b"percentage" in L.vh_last_error()
    assert rc(agg, [50, np.nan], 10) == 4
    assert rc(agg, [50, -0.5], 10) == 4
    assert rc(agg, [50, 75], 9) == 4 and b"size" in L.vh_last_error()
    assert L.vh_agg_percentile(agg._handle, out.ctypes.data, 0, 0.0, 1.0, out.ctypes.data, 0) == 4
    total = superagg.AggSum_float64(grid)
    assert rc(total, [50, 75], 10) == 4 and b"AggCount" in L.vh_last_error()
    grid0 = superagg.Grid([])
    assert rc(superagg.AggCount_int64(grid0), [50, 75], 2) == 4
    for bad in (lambda: agg.percentile([101], 0, 1), lambda: agg.percentile([np.nan], 0, 1),
                lambda: total.percentile([50], 0, 1)):
        with pytest.raises(_lib.HipError):
            bad()
