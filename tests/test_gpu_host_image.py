"""Registered host images (vh_agg_set_host_image): pass B's last unit of a tile
copies the tile's finished cells into the aggregator's page-locked image, so the read-back of
a count / sum grid is a stream wait.

Shapes: n = 2^20 + 4096 rows (the tile path starts at 2^20), 2-d float64 binners of 254 bins
(grids of 257^2 x 8 B = 528 KB, above the 256 KiB from which images are registered), integer-
valued float64 weights so every sum is exact.  Every cell is compared without tolerance with
the oracle and with the same query under VH_HOST_IMAGE=0, and every positive case reads
`host_image_bins` so that a silent fallback to the copy cannot pass."""
import functools

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

N = (1 << 20) + 4096
BINS = 254
LO, HI = -4.0, 4.0


def sa():
    import vaex_amd.superagg as m
    return m


def stat(name, reset=True):
    from vaex_amd import _lib
    return _lib.stat_read(name, reset)


def _bin_center(b):
    return LO + (np.asarray(b) + 0.5) * (HI - LO) / BINS


@functools.lru_cache(maxsize=None)
def _rows(n, seed=0, band=None):
    """x, y, w (read-only).  band = (b0, b1): y only in bins b0 .. b1 - 1."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=n)
    y = rng.normal(size=n) if band is None else _bin_center(rng.integers(band[0], band[1], n))
    x[::991] = np.nan
    x[5::1013] = 9.0  # overflow slot
    w = rng.integers(-50, 50, n).astype(np.float64)
    for a in (x, y, w):
        a.setflags(write=False)
    return x, y, w


def _obinners(x, y):
    return [oracle.Binner("scalar", x, vmin=LO, vmax=HI, bins=BINS), oracle.Binner("scalar", y, vmin=LO, vmax=HI, bins=BINS)]


@functools.lru_cache(maxsize=None)
def _expected(n, seed=0, band=None, masked=False):
    x, y, w = _rows(n, seed, band)
    keep = _keep(n) if masked else None
    ob = _obinners(x, y)
    c, s = oracle.compute_grid(ob, "count", mask=keep), oracle.compute_grid(ob, "sum", data=w, mask=keep)
    c.setflags(write=False), s.setflags(write=False)
    return c, s


@functools.lru_cache(maxsize=None)
def _keep(n):
    k = (np.random.default_rng(77).random(n) < 0.6).astype(np.uint8)
    k.setflags(write=False)
    return k


def _setup(x, y, w=None, keep=None, device=True):
    """grid, [count (, sum)] over the columns, not yet binned."""
    from vaex_amd.device import DeviceArray
    col = DeviceArray.from_numpy if device else (lambda a: a)
    bx, by = sa().BinnerScalar_float64("x", LO, HI, BINS), sa().BinnerScalar_float64("y", LO, HI, BINS)
    bx.set_data(col(x))
    by.set_data(col(y))
    grid = sa().Grid([bx, by])
    aggs = [sa().AggCount_int64(grid)]
    if w is not None:
        s = sa().AggSum_float64(grid)
        s.set_data(col(w), 0)
        aggs.append(s)
    if keep is not None:
        dk = col(keep)
        for a in aggs:
            a.set_data_mask(dk)
    return grid, aggs


def _query(x, y, w=None, keep=None):
    grid, aggs = _setup(x, y, w, keep)
    grid.bin(aggs)
    return [np.asarray(a).copy() for a in aggs]


def _check(monkeypatch, n, with_sum=True, masked=False, seed=0, band=None, env=()):
    for k, v in env:
        monkeypatch.setenv(k, v)
    x, y, w = _rows(n, seed, band)
    keep = _keep(n) if masked else None
    want = _expected(n, seed, band, masked)
    stat("host_image_bins")
    got = _query(x, y, w if with_sum else None, keep)
    assert stat("host_image_bins") == 1
    np.testing.assert_array_equal(got[0], want[0])
    if with_sum:
        np.testing.assert_array_equal(got[1], want[1])
    monkeypatch.setenv("VH_HOST_IMAGE", "0")
    off = _query(x, y, w if with_sum else None, keep)
    assert stat("host_image_bins") == 0
    for g, o in zip(got, off):
        np.testing.assert_array_equal(g, o)


@pytest.mark.parametrize("n", [N, N + 1])
@pytest.mark.parametrize("layout", ["stream", "regions", "count-only"])
def test_count_sum_mirrored(monkeypatch, layout, n):
    """count + sum(w) on the stream layout and on per-tile regions, and count alone (which
    keeps the regions layout); n odd: the last row's add is queued ahead of pass B."""
    _check(monkeypatch, n, with_sum=layout != "count-only", env=[("VH_TILE_STREAM", "0")] if layout == "regions" else [])


def test_shared_keep_mask(monkeypatch):
    """One keep mask on every aggregator: the row-masked fast pass A."""
    _check(monkeypatch, N, masked=True)


def test_uncovered_tiles_accumulation_and_hand_over():
    """Rows in a narrow band of y (two tiles' worth of cells), binned twice into the same
    aggregators: the image after the second bin is exactly twice the first result and zero
    elsewhere (tiles without rows reach the image too), and the array handed out after the
    first bin -- the image itself, as TaskPartAggregation.get_result hands it over -- is not
    written by the second."""
    band = (18, 39)  # y slots 20 .. 40: cells 5140 .. 10536, tiles 0 and 1 of 8192 cells
    x, y, w = _rows(N, 3, band)
    want_c, want_s = _expected(N, 3, band)
    assert np.count_nonzero(want_c.ravel(order="F")[2 * 8192:]) == 0 and want_c.sum() == N
    grid, aggs = _setup(x, y, w)
    stat("host_image_bins")
    grid.bin(aggs)
    first = []
    for a in aggs:
        view = np.asarray(a)
        image = a._host
        a._release_host()
        first.append((view, image, view.copy()))
    np.testing.assert_array_equal(first[0][0], want_c)
    np.testing.assert_array_equal(first[1][0], want_s)
    grid.bin(aggs)
    assert stat("host_image_bins") == 2
    second = [np.asarray(a) for a in aggs]
    np.testing.assert_array_equal(second[0], 2 * want_c)
    np.testing.assert_array_equal(second[1], 2 * want_s)
    for (view, image, saved), a in zip(first, aggs):
        assert a._host is not image
        np.testing.assert_array_equal(view, saved)


def test_several_units_on_one_tile(monkeypatch):
    """2^22 rows inside one tile over a thin uniform background: the hot tile's ticket is
    shared by several units, the other tiles have one unit each."""
    n = 1 << 22
    rng = np.random.default_rng(5)
    x = rng.uniform(LO, HI, n)
    y = _bin_center(rng.integers(5, 25, n))  # y slots 7 .. 26: cells below 8192, tile 0
    back = slice(0, n, 64)
    y[back] = rng.uniform(LO, HI, len(y[back]))
    w = rng.integers(-50, 50, n).astype(np.float64)
    ob = _obinners(x, y)
    stat("host_image_bins"), stat("host_image_tile_units")
    got = _query(x, y, w)
    assert stat("host_image_bins") == 1
    assert stat("host_image_tile_units") >= 2
    np.testing.assert_array_equal(got[0], oracle.compute_grid(ob, "count"))
    np.testing.assert_array_equal(got[1], oracle.compute_grid(ob, "sum", data=w))
    monkeypatch.setenv("VH_HOST_IMAGE", "0")
    off = _query(x, y, w)
    assert stat("host_image_bins") == 0
    np.testing.assert_array_equal(got[0], off[0])
    np.testing.assert_array_equal(got[1], off[1])


def test_min_max_not_mirrored():
    """Min / max are merged after pass B: they register no image, a bin of them alone leaves
    host_image_bins at 0, and count + min + max on one grid equals the oracle."""
    from vaex_amd.device import DeviceArray
    x, y, w = _rows(N)
    ob = _obinners(x, y)
    dw = DeviceArray.from_numpy(w)

    def minmax(grid):
        mn, mx = sa().AggMin_float64(grid), sa().AggMax_float64(grid)
        mn.set_data(dw, 0)
        mx.set_data(dw, 0)
        return [mn, mx]

    grid, _ = _setup(x, y)
    mm = minmax(grid)
    stat("host_image_bins")
    grid.bin(mm)
    assert stat("host_image_bins") == 0
    assert all(a._image_ptr is None for a in mm)
    np.testing.assert_array_equal(np.asarray(mm[0]), oracle.compute_grid(ob, "min", data=w))
    np.testing.assert_array_equal(np.asarray(mm[1]), oracle.compute_grid(ob, "max", data=w))
    grid, aggs = _setup(x, y)
    aggs += minmax(grid)
    stat("host_image_bins")
    grid.bin(aggs)
    assert stat("host_image_bins") == 1  # the count, mirrored by the min / max form of pass B
    assert aggs[0]._image_ptr is not None
    assert all(a._image_ptr is None for a in aggs[1:])
    np.testing.assert_array_equal(np.asarray(aggs[0]), _expected(N)[0])
    np.testing.assert_array_equal(np.asarray(aggs[1]), oracle.compute_grid(ob, "min", data=w))
    np.testing.assert_array_equal(np.asarray(aggs[2]), oracle.compute_grid(ob, "max", data=w))


def test_device_ptr_drops_the_image():
    """device_grid_ptr() hands the grid to writers the library cannot see: a write through it
    after a mirrored bin is what the next read returns."""
    from vaex_amd import _lib
    x, y, w = _rows(N)
    want_c, want_s = _expected(N)
    grid, aggs = _setup(x, y, w)
    stat("host_image_bins")
    grid.bin(aggs)
    assert stat("host_image_bins") == 1
    cells = want_c.size
    patch = np.arange(cells, dtype=np.int64)
    _lib.call("vh_memcpy_htod", aggs[0].device_grid_ptr(), patch.ctypes.data, patch.nbytes)
    np.testing.assert_array_equal(np.asarray(aggs[0]).ravel(order="F"), patch)
    np.testing.assert_array_equal(np.asarray(aggs[1]), want_s)  # still served by its image
    grid.bin(aggs)  # the count no longer registers an image: its read-back is the copy
    assert aggs[0]._image_ptr is None
    np.testing.assert_array_equal(np.asarray(aggs[0]).ravel(order="F"), patch + want_c.ravel(order="F"))
    np.testing.assert_array_equal(np.asarray(aggs[1]), 2 * want_s)


def _allreduce_rank(c, n):
    """One loopback rank: its shard of the rows binned over device columns (mirrored), the
    grids all-reduced across the ranks, then read back."""
    from vaex_amd.distributed import allreduce_aggs, shard_range
    x, y, w = (a[slice(*shard_range(n, c.rank, c.world))] for a in _rows(n, 11))
    grid, aggs = _setup(np.ascontiguousarray(x), np.ascontiguousarray(y), np.ascontiguousarray(w))
    grid.bin(aggs)
    registered = [a._image_ptr is not None for a in aggs]
    allreduce_aggs(aggs, c)
    return registered, [np.asarray(a).copy() for a in aggs]


def test_allreduce_after_a_mirrored_bin():
    """vh_comm_agg_allreduce rewrites the device grid in place: the read-back after it is the
    sum over all ranks' rows, not this rank's mirrored partial grid.  Two loopback ranks, each
    with at least 2^20 device rows, one mirrored bin per rank."""
    import concurrent.futures as cf
    from vaex_amd import comm as vcomm
    world, n = 2, 2 * N
    want_c, want_s = _expected(n, 11)
    stat("host_image_bins")
    comms = vcomm.loopback_group(world)
    try:
        with cf.ThreadPoolExecutor(world) as ex:
            futs = [ex.submit(_allreduce_rank, c, n) for c in comms]
            res = [f.result(timeout=120) for f in futs]
    finally:
        for c in comms:
            c.close()
    assert stat("host_image_bins") == world  # one mirrored bin per rank
    for registered, (got_c, got_s) in res:
        assert all(registered)
        np.testing.assert_array_equal(got_c, want_c)
        np.testing.assert_array_equal(got_s, want_s)


def test_write_through_the_live_view_then_bin():
    """A write through np.asarray(agg) after a mirrored bin is uploaded before the next bin,
    whose mirror then carries it."""
    x, y, w = _rows(N)
    want_c, want_s = _expected(N)
    grid, aggs = _setup(x, y, w)
    grid.bin(aggs)
    vc, vs = np.asarray(aggs[0]), np.asarray(aggs[1])
    np.testing.assert_array_equal(vc, want_c)
    vc[3, 5] += 1000
    vs[...] = 0.5
    stat("host_image_bins")
    grid.bin(aggs)
    assert stat("host_image_bins") == 1
    exp_c = 2 * want_c
    exp_c[3, 5] += 1000
    np.testing.assert_array_equal(np.asarray(aggs[0]), exp_c)
    np.testing.assert_array_equal(np.asarray(aggs[1]), want_s + 0.5)


def test_small_bin_after_a_mirrored_one():
    """A second bin of 1000 rows takes a route that mirrors nothing: the read-back after it
    is the copy, with both bins' rows."""
    from vaex_amd.device import DeviceArray
    x, y, w = _rows(N)
    want_c, want_s = _expected(N)
    grid, aggs = _setup(x, y, w)
    grid.bin(aggs)
    np.testing.assert_array_equal(np.asarray(aggs[0]), want_c)
    m = 1000
    for b, col in zip(grid.binners, (x, y)):
        b.set_data(DeviceArray.from_numpy(np.ascontiguousarray(col[:m])))
    aggs[1].set_data(DeviceArray.from_numpy(np.ascontiguousarray(w[:m])), 0)
    stat("host_image_bins")
    grid.bin(aggs)
    assert stat("host_image_bins") == 0
    ob = _obinners(x[:m], y[:m])
    np.testing.assert_array_equal(np.asarray(aggs[0]), want_c + oracle.compute_grid(ob, "count"))
    np.testing.assert_array_equal(np.asarray(aggs[1]), want_s + oracle.compute_grid(ob, "sum", data=w[:m]))


def test_host_columns_register_nothing():
    x, y, w = _rows(N)
    want_c, want_s = _expected(N)
    grid, aggs = _setup(x, y, w, device=False)
    stat("host_image_bins")
    grid.bin(aggs)
    assert stat("host_image_bins") == 0
    assert all(a._image_ptr is None for a in aggs)
    np.testing.assert_array_equal(np.asarray(aggs[0]), want_c)
    np.testing.assert_array_equal(np.asarray(aggs[1]), want_s)


def test_registration_is_checked():
    """vh_agg_set_host_image refuses pageable memory, a wrong size and an unaligned address."""
    from vaex_amd import _lib
    x, y, _ = _rows(N)
    grid, aggs = _setup(x, y)
    a = aggs[0]
    pageable = np.zeros(a._nbytes // 8 + 2, np.int64)
    pinned = _lib.pinned_empty(a._nbytes // 8 + 2, np.int64)
    for ptr, nbytes in ((pageable.ctypes.data, a._nbytes), (pinned.ctypes.data, a._nbytes - 8), (pinned.ctypes.data + 8, a._nbytes)):
        with pytest.raises(Exception):
            _lib.call("vh_agg_set_host_image", a._handle, ptr, nbytes)
    _lib.call("vh_agg_set_host_image", a._handle, pinned.ctypes.data, a._nbytes)
    _lib.call("vh_agg_set_host_image", a._handle, None, 0)
