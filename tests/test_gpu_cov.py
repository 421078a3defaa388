"""AggCov (``superagg.AggCov_float64``) and ``DataFrame.cov / covar / correlation`` against the
NumPy yardstick of the reference's OP_COV statistic (tests/cov_np.py).

Exact tier: integer values in [-1000, 1000] stored as float64 and at most 2**20 rows, so every
partial sum is an integer below 2**53 and no result depends on the order of the additions:
grids and finished statistics must be bit-equal.  Tolerance tier: uniform values in [0.5, 1.5]
(no sum cancels), the project's 1e-6 relative tolerance for float64 sums, counts exact."""
import concurrent.futures as cf

import numpy as np
import pytest

import cov_np
from oracle import oracle

pytestmark = pytest.mark.gpu

LDS_BYTES = 96 * 1024  # the small-grid budget the accumulators (2N + N*N float64 per cell) must fit


def sa():
    import vaex_amd.superagg as m
    return m


def dev(a):
    from vaex_amd.device import DeviceArray
    return DeviceArray.from_numpy(a)


def int_columns(N, n, seed=1, nans=True):
    rng = np.random.default_rng(seed)
    cols = [rng.integers(-1000, 1001, n).astype(np.float64) for _ in range(N)]
    if nans and n:
        cols[0][rng.random(n) < 0.05] = np.nan          # x only
        if N > 1:
            cols[1][rng.random(n) < 0.05] = np.nan      # y only, both by chance
            cols[0][n // 2] = cols[1][n // 2] = np.nan  # both
    return cols


def key_column(n, seed=2):
    """Uniform over [-0.1, 1.1] (under- and overflow of limits [0, 1]) with some NaN (slot 0)."""
    rng = np.random.default_rng(seed)
    k = rng.uniform(-0.1, 1.1, n)
    k[rng.random(n) < 0.02] = np.nan
    return k


def make_binners(specs):
    from vaex_amd.utils import find_type_from_dtype
    out = []
    for s in specs:
        if s.kind == "scalar":
            b = find_type_from_dtype(sa(), "BinnerScalar_", s.data.dtype)("k", s.vmin, s.vmax, s.bins)
        else:
            b = find_type_from_dtype(sa(), "BinnerOrdinal_", s.data.dtype)("k", s.ordinal_count, s.min_value)
        b.set_data(s.data)
        out.append(b)
    return out


def gpu_grid(specs, cols, n, keep=None, on_device=False, mask_on_device=False):
    grid = sa().Grid(make_binners(specs))
    agg = sa().AggCov_float64(grid, len(cols))
    for i, c in enumerate(cols):
        agg.set_data(dev(c) if on_device and isinstance(c, np.ndarray) else c, i)
    if keep is not None:
        agg.set_data_mask(dev(keep.astype(np.uint8)) if mask_on_device else keep)
    grid.bin([agg], n)
    return np.asarray(agg).copy()


def want_grid(specs, cols, n, keep=None):
    shape = oracle.grid_shape(specs)
    L = int(np.prod(shape, dtype=np.int64)) if specs else 1
    idx = oracle.bin_indices(specs, n) if specs else np.zeros(n, np.uint64)
    return cov_np.grid_view(cov_np.op_cov(idx, L, [np.asarray(c)[:n] for c in cols], keep), shape)


def check_symmetry(g, N):
    cnt = g[..., 2 * N:2 * N + N * N].reshape(g.shape[:-1] + (N, N))
    s = g[..., 2 * N + N * N:].reshape(g.shape[:-1] + (N, N))
    np.testing.assert_array_equal(cnt, np.swapaxes(cnt, -1, -2))
    np.testing.assert_array_equal(s, np.swapaxes(s, -1, -2))
    np.testing.assert_array_equal(np.diagonal(cnt, axis1=-2, axis2=-1), g[..., :N])


def scalar(n, bins, seed=2):
    return oracle.Binner("scalar", key_column(n, seed), vmin=0.0, vmax=1.0, bins=bins)


def ordinal(n, count, seed=4):
    k = np.random.default_rng(seed).integers(-2, count + 2, n).astype(np.int32)  # under / overflow too
    return oracle.Binner("ordinal", k, ordinal_count=count, min_value=0)


def lds_boundary_bins(N):
    return LDS_BYTES // ((2 * N + N * N) * 8) - 3


REGIMES = {
    "none": lambda n: [],
    "1bin": lambda n: [scalar(n, 1)],
    "4bins": lambda n: [scalar(n, 4)],
    "128bins": lambda n: [scalar(n, 128)],
    "lds_max": lambda n: [scalar(n, lds_boundary_bins(2))],
    "lds_max+1": lambda n: [scalar(n, lds_boundary_bins(2) + 1)],
    "64x64": lambda n: [scalar(n, 64), scalar(n, 64, seed=3)],
    "ordinal": lambda n: [ordinal(n, 20)],
    "scalar_x_ordinal": lambda n: [scalar(n, 9), ordinal(n, 6)],
}


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("N", [2, 3])
def test_exact_grid_regimes(regime, N):
    n = 100_003
    specs = REGIMES[regime](n)
    cols = int_columns(N, n)
    got = gpu_grid(specs, cols, n)
    assert got.shape == oracle.grid_shape(specs) + (cov_np.fields(N),) and got.dtype == np.float64
    np.testing.assert_array_equal(got, want_grid(specs, cols, n))
    check_symmetry(got, N)
    # column counts, pair counts and the diagonal all differ on this data
    flat = got.reshape(-1, got.shape[-1]).sum(axis=0)
    assert flat[0] != flat[1] and flat[2 * N + 1] < min(flat[0], flat[1])


def test_both_sides_of_the_lds_boundary_take_their_kernel():
    from vaex_amd import _lib
    n, N = 20_011, 2
    cols = int_columns(N, n)
    _lib.timing_enable(True)
    try:
        for bins, kernel in ((lds_boundary_bins(N), "bin_cov_lds"), (lds_boundary_bins(N) + 1, "bin_cov_global")):
            _lib.timing_reset()
            specs = [scalar(n, bins)]
            np.testing.assert_array_equal(gpu_grid(specs, cols, n), want_grid(specs, cols, n))
            assert _lib.timing_read(kernel)[0] == 1, (bins, kernel)
    finally:
        _lib.timing_enable(False)


@pytest.mark.parametrize("regime", ["none", "4bins", "128bins", "64x64"])
@pytest.mark.parametrize("N", [1, 5, 8])
def test_exact_other_column_counts(regime, N):
    n = 20_011
    specs = REGIMES[regime](n)
    cols = int_columns(N, n, seed=N)
    got = gpu_grid(specs, cols, n)
    np.testing.assert_array_equal(got, want_grid(specs, cols, n))
    check_symmetry(got, N)


@pytest.mark.parametrize("regime", ["none", "4bins"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 100_003, 300_007])
def test_exact_row_counts(regime, n):
    specs = REGIMES[regime](n)
    cols = int_columns(2, n, seed=n + 1, nans=n > 2)
    np.testing.assert_array_equal(gpu_grid(specs, cols, n), want_grid(specs, cols, n))


@pytest.mark.parametrize("n", [1, 65, 300_007])
def test_exact_row_counts_three_columns_no_binners(n):
    cols = int_columns(3, n, seed=n, nans=n > 2)
    np.testing.assert_array_equal(gpu_grid([], cols, n), want_grid([], cols, n))


def test_host_columns_span_two_pipeline_chunks():
    """Host columns are staged in chunks of 2**24 rows: the second chunk's value columns, key and
    mask come from the other pipeline buffer (sums stay exact: 2**24 * 1e6 < 2**53)."""
    n = (1 << 24) + 1003
    rng = np.random.default_rng(21)
    cols = [rng.integers(-1000, 1001, n).astype(np.float64) for _ in range(2)]
    cols[1][::7] = np.nan
    keep = np.ones(n, bool)
    keep[1::5] = False
    specs = [oracle.Binner("scalar", rng.uniform(-0.1, 1.1, n), vmin=0.0, vmax=1.0, bins=4)]
    np.testing.assert_array_equal(gpu_grid(specs, cols, n, keep=keep), want_grid(specs, cols, n, keep))


def test_errors():
    b = sa().BinnerScalar_float64("k", 0, 1, 4)
    b.set_data(np.zeros(8))
    grid = sa().Grid([b])
    with pytest.raises(RuntimeError, match="1 to 8 value columns"):
        sa().AggCov_float64(grid, 9)
    with pytest.raises(RuntimeError, match="1 to 8 value columns"):
        sa().AggCov_float64(grid, 0)
    agg = sa().AggCov_float64(grid, 2)
    agg.set_data(np.zeros(8), 0)
    with pytest.raises(RuntimeError, match="data1 not set"):
        grid.bin([agg])
    with pytest.raises(RuntimeError, match="outside its 2 columns"):
        agg.set_data(np.zeros(8), 2)
    with pytest.raises(RuntimeError, match="Itemsize"):
        agg.set_data(np.zeros(8, np.float32), 1)


def test_special_cells():
    """One cell holds +inf, one an inf * 0 row, one only NaN."""
    n = 4_001
    k = np.random.default_rng(5).uniform(0, 1, n)
    x, y = int_columns(2, n, nans=False)
    cell = np.minimum((k * 4).astype(int), 3)
    x[np.flatnonzero(cell == 0)[0]] = np.inf
    i = np.flatnonzero(cell == 1)[0]
    x[i], y[i] = np.inf, 0.0
    x[cell == 2] = np.nan
    y[cell == 2] = np.nan
    specs = [oracle.Binner("scalar", k, vmin=0.0, vmax=1.0, bins=4)]
    got = gpu_grid(specs, [x, y], n)
    np.testing.assert_array_equal(got, want_grid(specs, [x, y], n))
    central = got[2:-1]
    assert central[0, 2] == np.inf and np.isnan(central[1, -2]) and not central[2].any() and np.isfinite(central[3]).all()


@pytest.mark.parametrize("regime", ["none", "128bins", "64x64"])
@pytest.mark.parametrize("mask_on_device", [False, True])
def test_data_mask(regime, mask_on_device):
    n = 50_021
    specs = REGIMES[regime](n)
    cols = int_columns(2, n)
    keep = np.random.default_rng(6).random(n) < 0.5
    got = gpu_grid(specs, cols, n, keep=keep, on_device=mask_on_device, mask_on_device=mask_on_device)
    np.testing.assert_array_equal(got, want_grid(specs, cols, n, keep))


@pytest.mark.parametrize("regime", ["none", "4bins", "64x64"])
def test_host_and_hbm_columns_agree(regime):
    n = 50_021
    specs = REGIMES[regime](n)
    cols = int_columns(3, n)
    np.testing.assert_array_equal(gpu_grid(specs, cols, n, on_device=True), gpu_grid(specs, cols, n))


@pytest.mark.parametrize("regime", ["none", "4bins"])
@pytest.mark.parametrize("shifted", [(0,), (0, 2), (0, 1, 2)])
def test_hbm_columns_8_byte_aligned_only(regime, shifted):
    n = 50_021
    specs = REGIMES[regime](n)
    full = int_columns(3, n + 1)
    cols = [dev(c)[1:] if i in shifted else dev(c[1:]) for i, c in enumerate(full)]
    assert all(cols[i].ptr % 16 == 8 for i in shifted)
    host = [c[1:] for c in full]
    np.testing.assert_array_equal(gpu_grid(specs, cols, n), want_grid(specs, host, n))


@pytest.mark.parametrize("regime", ["none", "128bins", "64x64"])
def test_accumulate_reduce_and_live_view(regime):
    n = 40_009
    specs = REGIMES[regime](n)
    cols = int_columns(2, n)
    want = want_grid(specs, cols, n)
    h = n // 2 + 1

    def half(lo, hi, base=None):
        sub = [oracle.Binner(s.kind, s.data[lo:hi], vmin=s.vmin, vmax=s.vmax, bins=s.bins) for s in specs]
        grid = sa().Grid(make_binners(sub))
        agg = sa().AggCov_float64(grid, 2)
        view = np.asarray(agg)
        if base is not None:
            view[...] = base  # written through the live view before bin
        for i, c in enumerate(cols):
            agg.set_data(c[lo:hi], i)
        grid.bin([agg], hi - lo)
        return grid, agg, view

    # two bin calls on one aggregator == one call on the concatenation
    grid, agg, view = half(0, h)
    for s, b in zip(specs, grid.binners):
        b.set_data(s.data[h:])
    for i, c in enumerate(cols):
        agg.set_data(c[h:], i)
    grid.bin([agg], n - h)
    np.testing.assert_array_equal(view, want)
    # reduce of two halves
    _, a, va = half(0, h)
    _, b, _ = half(h, n)
    a.reduce([b])
    np.testing.assert_array_equal(va, want)
    # a grid written through the view is kept: start from the first half's result
    first = want_grid([oracle.Binner(s.kind, s.data[:h], vmin=s.vmin, vmax=s.vmax, bins=s.bins) for s in specs],
                      [c[:h] for c in cols], h)
    _, _, v = half(h, n, base=first)
    np.testing.assert_array_equal(v, want)


@pytest.mark.parametrize("regime", ["none", "128bins", "64x64"])
def test_tolerance_tier(regime):
    n, N = 300_007, 3
    specs = REGIMES[regime](n)
    rng = np.random.default_rng(8)
    cols = [rng.uniform(0.5, 1.5, n) for _ in range(N)]
    cols[1][::97] = np.nan
    got, want = gpu_grid(specs, cols, n, on_device=True), want_grid(specs, cols, n)
    counts = np.r_[0:N, 2 * N:2 * N + N * N]
    np.testing.assert_array_equal(got[..., counts], want[..., counts])
    np.testing.assert_allclose(got, want, rtol=1e-6)


# ---- through the DataFrame ------------------------------------------------------------------
N_DF = 30_011


@pytest.fixture(scope="module")
def frame():
    x, y, z = int_columns(3, N_DF, seed=11)
    rng = np.random.default_rng(12)
    return {"x": x, "y": y, "z": z, "b": key_column(N_DF, 13), "c": key_column(N_DF, 14),
            "f": rng.integers(-1000, 1001, N_DF).astype(np.float32), "i": rng.integers(-1000, 1001, N_DF).astype(np.int32)}


def want_cov(data, names, binby=(), limits=(), shapes=(), keep=None):
    n = len(data[names[0]])
    specs = [oracle.Binner("scalar", data[b], vmin=l[0], vmax=l[1], bins=s) for b, l, s in zip(binby, limits, shapes)]
    cols = [data[c].astype(np.float64) for c in names]
    g = want_grid(specs, cols, n, keep)
    g = g[(slice(2, -1),) * len(specs)]
    return cov_np.cov_finish(g, len(names))


@pytest.mark.parametrize("on_device", [False, True])
def test_df_cov_shapes_and_values(frame, on_device):
    import vaex_amd
    df = vaex_amd.DataFrame({k: dev(v) for k, v in frame.items()} if on_device else frame)
    c = df.cov(["x", "y", "z"])
    assert c.shape == (3, 3)
    np.testing.assert_array_equal(c, want_cov(frame, ["x", "y", "z"]))
    c = df.cov("x", "y", binby="b", limits=[0, 1], shape=8)
    assert c.shape == (8, 2, 2)
    np.testing.assert_array_equal(c, want_cov(frame, ["x", "y"], ["b"], [[0, 1]], [8]))
    c = df.cov("x", "y", binby=["b", "c"], limits=[[0, 1], [0.2, 0.9]], shape=[5, 6])
    assert c.shape == (5, 6, 2, 2)
    np.testing.assert_array_equal(c, want_cov(frame, ["x", "y"], ["b", "c"], [[0, 1], [0.2, 0.9]], [5, 6]))


def test_df_covar_and_correlation(frame):
    import vaex_amd
    df = vaex_amd.DataFrame(frame)
    cxy, cxz = want_cov(frame, ["x", "y"]), want_cov(frame, ["x", "z"])
    np.testing.assert_array_equal(df.covar("x", "y"), cxy[0, 1])
    got = df.covar(["x", "x"], ["y", "z"], binby="b", limits=[0, 1], shape=4)
    wb = [want_cov(frame, ["x", k], ["b"], [[0, 1]], [4])[..., 0, 1] for k in ("y", "z")]
    assert got.shape == (2, 4)
    np.testing.assert_array_equal(got, np.array(wb))
    np.testing.assert_array_equal(df.correlation("x", "y"), cov_np.correlation_finish(cxy))
    np.testing.assert_array_equal(df.correlation(df.x, df.y), cov_np.correlation_finish(cxy))
    pairs = [["x", "y"], ["x", "z"]]
    want = np.array([cov_np.correlation_finish(cxy), cov_np.correlation_finish(cxz)])
    np.testing.assert_array_equal(df.correlation(pairs), want)
    np.testing.assert_array_equal(df.correlation(["x", "y"]), want[:1])
    values, sorted_x = df.correlation(pairs, sort=True)
    order = np.argsort(np.abs(want))[::-1]
    np.testing.assert_array_equal(values, want[order])
    assert sorted_x == [pairs[k] for k in order]
    with pytest.raises(ValueError, match="expected to be a list or tuple"):
        df.correlation("x")
    with pytest.raises(ValueError, match="list of lists with length 2"):
        df.correlation(["x", "y", "z"])
    with pytest.raises(ValueError, match="expected to be sequence"):
        df.cov("x")


def test_df_selection_filter_dtypes_masked_delay(frame):
    import vaex_amd
    df = vaex_amd.DataFrame(frame)
    keep = frame["z"] > 0
    with np.errstate(invalid="ignore"):
        want = want_cov(frame, ["x", "y"], ["b"], [[0, 1]], [4], keep=keep)
    df.select("z > 0")
    kw = dict(binby="b", limits=[0, 1], shape=4)
    np.testing.assert_array_equal(df.cov("x", "y", selection=True, **kw), want)
    np.testing.assert_array_equal(df.cov("x", "y", selection="z > 0", **kw), want)
    np.testing.assert_array_equal(df.filter("z > 0").cov("x", "y", **kw), want)
    np.testing.assert_array_equal(df.cov("x", "y", **kw), want_cov(frame, ["x", "y"], ["b"], [[0, 1]], [4]))
    # float32 and int32 columns are cast to float64, as var does
    np.testing.assert_array_equal(df.cov(["x", "f", "i"]), want_cov(frame, ["x", "f", "i"]))
    # a masked host column: masked rows contribute to no column
    m = np.random.default_rng(15).random(N_DF) < 0.3
    dm = vaex_amd.DataFrame(dict(frame, y=np.ma.array(frame["y"], mask=m)))
    np.testing.assert_array_equal(dm.cov("x", "y", **kw), want_cov(frame, ["x", "y"], ["b"], [[0, 1]], [4], keep=~m))
    # delay
    p = df.correlation("x", "y", delay=True, **kw)
    q = df.cov(["x", "y", "z"], delay=True)
    df.execute()
    np.testing.assert_array_equal(p.get(), cov_np.correlation_finish(want_cov(frame, ["x", "y"], ["b"], [[0, 1]], [4])))
    np.testing.assert_array_equal(q.get(), want_cov(frame, ["x", "y", "z"]))


def test_df_reference_known_answers():
    """tests/agg_test.py:54-99 of the reference, on its frame x = arange(10), y = x**2."""
    import vaex_amd
    x = np.arange(10, dtype=np.float64)
    y = x ** 2
    df = vaex_amd.DataFrame({"x": x, "y": y})

    def correlation(x, y):
        c = np.cov([x, y], bias=1)
        return c[0, 1] / (c[0, 0] * c[1, 1]) ** 0.5

    aae = np.testing.assert_array_almost_equal
    aae(df.correlation(df.y, df.y), 1.0)
    aae(df.correlation(df.y, -df.y), -1.0)
    aae(df.correlation([["x", "y"], ["x", "x**2"]], selection=None), [correlation(x, y), correlation(x, x ** 2)])
    df.select("x < 5")
    aae(df.correlation("x", "y", selection=None), correlation(x, y))
    aae(df.correlation("x", "y", selection=True), correlation(x[:5], y[:5]))
    task = df.correlation("x", "y", selection=True, delay=True)
    df.execute()
    aae(task.get(), correlation(x[:5], y[:5]))
    aae(df.correlation("x", "y", selection=None, binby=["x"], limits=[0, 10], shape=1), [correlation(x, y)])
    aae(df.correlation("x", "y", selection=True, binby=["y"], limits=[0, 9 ** 2 + 1], shape=1), [correlation(x[:5], y[:5])])
    i = 7
    aae(df.correlation("x", "y", selection=None, binby=["y"], limits=[0, 9 ** 2 + 1], shape=2),
        [correlation(x[:i], y[:i]), correlation(x[i:], y[i:])])
    aae(df.correlation("x", "y", selection=True, binby=["y"], limits=[0, 9 ** 2 + 1], shape=2), [correlation(x[:5], y[:5]), np.nan])
    i = 5
    aae(df.correlation("x", "y", selection=None, binby=["x"], limits=[0, 10], shape=2),
        [correlation(x[:i], y[:i]), correlation(x[i:], y[i:])])
    aae(df.correlation("x", "y", selection=True, binby=["x"], limits=[0, 10], shape=2), [correlation(x[:i], y[:i]), np.nan])
    aae(df.correlation("x", "y", selection=True, binby=["x"], limits=[[0, 10]], shape=2), [correlation(x[:i], y[:i]), np.nan])
    # an empty cell's correlation is NaN
    assert np.isnan(df.correlation("x", "y", binby="x", limits=[0, 20], shape=2)[1])


# ---- distributed ----------------------------------------------------------------------------
def _cov_rank(c, n):
    from vaex_amd.distributed import allreduce_aggs, shard_range
    s = slice(*shard_range(n, c.rank, c.world))
    b = sa().BinnerScalar_float64("k", 0.0, 1.0, 61)
    b.set_data(key_column(n)[s])
    grid = sa().Grid([b])
    agg = sa().AggCov_float64(grid, 3)
    for i, col in enumerate(int_columns(3, n)):
        agg.set_data(col[s], i)
    grid.bin([agg])
    allreduce_aggs([agg], c)
    return np.asarray(agg).copy()


def test_loopback_allreduce_world_2():
    from vaex_amd import comm as vcomm
    n, world = 60_013, 2
    specs = [scalar(n, 61)]
    want = want_grid(specs, int_columns(3, n), n)
    comms = vcomm.loopback_group(world)
    try:
        with cf.ThreadPoolExecutor(world) as ex:
            futs = [ex.submit(_cov_rank, c, n) for c in comms]
            got = [f.result(timeout=300) for f in futs]
    finally:
        for c in comms:
            c.close()
    for g in got:
        np.testing.assert_array_equal(g, want)
