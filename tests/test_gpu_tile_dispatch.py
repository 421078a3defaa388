"""Which pass-A family the tiled engine (tiled.hip) runs for a plan, pinned per plan through
the timing scopes: the expected ``tile_scatter*`` scope has at least one launch and each of
the six others none, so a plan that drifts to another kernel family (the generic pass A
above all: same grids, only slower) fails here.  Every plan's grids are also checked against
the oracle (counts exact, sums within 1e-6 relative).  n = 2^20 rows, the smallest the tiled
engine takes; 2^20 + 1 where the last row goes through the global-atomic path."""
import functools

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

N = 1 << 20
SCOPES = ("tile_scatter", "tile_scatter_f64", "tile_scatter_f32", "tile_scatter_mixed", "tile_scatter_int",
          "tile_scatter_ord", "tile_scatter_set")


def sa():
    import vaex_amd.superagg as m
    return m


@functools.lru_cache(maxsize=None)
def _columns():
    """x, y, w (float64, NaNs in each), integer x / y, a keep mask and ordinal keys: N + 1 rows,
    generated once and never written to."""
    rng = np.random.default_rng(2024)
    n = N + 1
    x, y, w = rng.normal(size=n), rng.normal(size=n), rng.random(n)
    x[::997] = np.nan
    w[::101] = np.nan
    ix, iy = rng.integers(-100, 1200, n).astype(np.int32), rng.integers(-100, 1200, n).astype(np.int32)
    keep = (rng.random(n) < 0.6).astype(np.uint8)
    keys = rng.integers(-3, (1 << 20) + 5, n).astype(np.int32)
    cols = dict(x=x, y=y, w=w, ix=ix, iy=iy, keep=keep, keys=keys)
    for a in cols.values():
        a.setflags(write=False)
    return cols


def _pinned(expected, run):
    """run() bins once; returns its result after requiring that only `expected` launched
    (None: no pass A at all, the tiled engine refused the plan)."""
    from vaex_amd import _lib
    _lib.timing_enable(True)
    _lib.timing_reset()
    try:
        out = run()
        _lib.synchronize()
        got = {s: _lib.timing_read(s)[0] for s in SCOPES}
    finally:
        _lib.timing_enable(False)
    print("pass A launches:", got)
    if expected is not None:
        assert got[expected] >= 1, f"{expected} did not run: {got}"
    for s in SCOPES:
        if s != expected:
            assert got[s] == 0, f"{s} ran, expected only {expected}: {got}"
    return out


def _scalar_plan(expected, n, bdt, vdt, bins=1024, nd=2, sum_mask=None, count_mask=None, lim=(-4, 4), src=("x", "y")):
    """count(*) (+ a sum of w as vdt) over nd scalar binners of dtype bdt, against the oracle."""
    from vaex_amd.device import DeviceArray
    c = _columns()
    xs = [np.ascontiguousarray(c[name][:n].astype(bdt)) for name in src[:nd]]
    w = None if vdt is None else np.ascontiguousarray(c["w"][:n].astype(vdt))

    def run():
        bs = []
        for i, x in enumerate(xs):
            b = getattr(sa(), "BinnerScalar_" + bdt)(f"x{i}", lim[0], lim[1], bins)
            b.set_data(DeviceArray.from_numpy(x))
            bs.append(b)
        grid = sa().Grid(bs)
        aggs = [sa().AggCount_int64(grid)]
        if w is not None:
            s = getattr(sa(), "AggSum_" + vdt)(grid)
            s.set_data(DeviceArray.from_numpy(w), 0)
            aggs.append(s)
        dev_masks = {}  # one device copy per mask: a mask shared on the host is shared on the device
        for a, m in zip(aggs, (count_mask, sum_mask)):
            if m is not None:
                a.set_data_mask(dev_masks.setdefault(id(m), DeviceArray.from_numpy(m)))
        grid.bin(aggs)
        return [np.asarray(a).copy() for a in aggs]

    out = _pinned(expected, run)
    ob = [oracle.Binner("scalar", x, vmin=lim[0], vmax=lim[1], bins=bins) for x in xs]
    np.testing.assert_array_equal(out[0], oracle.compute_grid(ob, "count", mask=count_mask))
    if w is not None:
        np.testing.assert_allclose(out[1], oracle.compute_grid(ob, "sum", data=w, mask=sum_mask), rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("n", [N, N + 1])
def test_float64_count_sum_runs_the_f64_kernel(n):
    """Odd n: all rows but the last through the fast kernel, the last through global atomics."""
    _scalar_plan("tile_scatter_f64", n, "float64", "float64")


def test_float32_count_sum_runs_the_f32_kernel():
    _scalar_plan("tile_scatter_f32", N, "float32", "float32")


@pytest.mark.parametrize("bdt,vdt", [("float32", "float64"), ("float64", "float32")])
def test_mixed_column_types_run_the_mixed_kernel(bdt, vdt):
    _scalar_plan("tile_scatter_mixed", N, bdt, vdt)


def test_int32_binners_run_the_int_kernel():
    _scalar_plan("tile_scatter_int", N, "int32", None, bins=1000, lim=(0, 1000), src=("ix", "iy"))


def test_mask_on_the_sum_only_runs_the_generic_kernel():
    keep = np.ascontiguousarray(_columns()["keep"][:N])
    _scalar_plan("tile_scatter", N, "float64", "float64", sum_mask=keep)


def test_shared_mask_runs_the_f64_kernel_unless_switched_off(monkeypatch):
    keep = np.ascontiguousarray(_columns()["keep"][:N])
    _scalar_plan("tile_scatter_f64", N, "float64", "float64", sum_mask=keep, count_mask=keep)
    monkeypatch.setenv("VH_TILE_ROWMASK", "0")
    _scalar_plan("tile_scatter", N, "float64", "float64", sum_mask=keep, count_mask=keep)


@pytest.mark.parametrize("bins,expected", [(4092 * 8192 - 3, "tile_scatter"), (1 << 25, None)])
def test_float32_plan_past_the_fast_kernels_lds_runs_the_generic_kernel(bins, expected):
    """4092 tiles of 8192 cells: past the fast kernels' LDS, the most the generic pass A's LDS
    holds with one value slot.  The plan must reach the generic dispatch kernel, not an ND > 0
    kernel that would read its float32 column as float64.  2^25 bins (+ 3 cells) are 4097
    tiles: the tiled engine refuses the plan and no pass A runs (the global-atomic path)."""
    _scalar_plan(expected, N, "float32", "float32", bins=bins, nd=1)


def test_float32_plan_with_the_f32_kernels_switched_off(monkeypatch):
    monkeypatch.setenv("VH_TILE_F32", "0")
    _scalar_plan("tile_scatter", N, "float32", "float32")


def _ordinal_plan(expected, make_binner, ordinals, count):
    from vaex_amd.device import DeviceArray
    w = np.ascontiguousarray(_columns()["w"][:N])

    def run():
        grid = sa().Grid([make_binner()])
        aggs = [sa().AggCount_int64(grid), sa().AggSum_float64(grid)]
        aggs[1].set_data(DeviceArray.from_numpy(w), 0)
        grid.bin(aggs)
        return [np.asarray(a).copy() for a in aggs]

    out = _pinned(expected, run)
    ob = [oracle.Binner("ordinal", ordinals, ordinal_count=count, min_value=0)]
    np.testing.assert_array_equal(out[0], oracle.compute_grid(ob, "count"))
    np.testing.assert_allclose(out[1], oracle.compute_grid(ob, "sum", data=w), rtol=1e-6, atol=1e-12)


def test_int32_ordinal_binner_runs_the_ordinal_kernel():
    from vaex_amd.device import DeviceArray
    keys = np.ascontiguousarray(_columns()["keys"][:N])

    def binner():
        b = sa().BinnerOrdinal_int32("k", 1 << 20, 0)
        b.set_data(DeviceArray.from_numpy(keys))
        return b

    _ordinal_plan("tile_scatter_ord", binner, keys, 1 << 20)


def test_set_ordinal_binner_runs_the_set_kernel():
    from vaex_amd import superutils
    from vaex_amd.device import DeviceArray
    keys = (np.random.default_rng(7).permutation(N) * 3 - 1000).astype(np.int32)  # 2^20 distinct keys
    s = superutils.ordered_set_int32()
    s.update(keys)
    assert len(s) == N

    def binner():
        b = sa().BinnerSetOrdinal("k", s, len(s))
        b.set_data(DeviceArray.from_numpy(keys))
        return b

    _ordinal_plan("tile_scatter_set", binner, np.asarray(s.map_ordinal(keys)), len(s))
