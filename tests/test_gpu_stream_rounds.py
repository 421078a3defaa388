"""Pass B of the tiled engine walking a work unit in several rounds (k_tile_reduce's stream
walk: `fetch(r + 1)`, `stream_round(r > 0)`, the reuse of s_fill / s_pre / s_a between two
barriers and the (r * SEGS + kk) / ncw workgroup arithmetic), cell by cell
against the oracle, once per pass-B instantiation family the stream layout reaches.

Only a cold tile's single unit holds enough (workgroup, commit) segments for a second round,
and only past 2048 * 4096 * sb rows, so every case here has 8.6 to 25.2 M rows
(tests/stream_rounds_cases.py; tests/test_tile_plan.py shows on the CPU that each pair reaches
its rounds at every pass-A occupancy) and mixes a hot core -- a narrow normal, a few tiles of
many one-round units -- with a thin uniform background over the whole range, under / overflow
and NaN binner rows included, that keeps every other tile below the n / (4 CUs) rows at which
the planner splits a tile, with still a few rows in each segment.

Every test resets vh_stat_read("tile_stream_rounds"), runs the query and asserts that a unit
walked at least two rounds (exactly three where the pair is meant for the ceiling).  Value
columns hold integer-valued floats with NaN every 101st row, so cell sums, and sums of squares
(below 2^53), are exact in any association order: counts, sums, min, max, var and std are
compared with assert_array_equal, no tolerance."""
import os

import numpy as np
import pytest

from oracle import oracle
from stream_rounds_cases import CASES

pytestmark = pytest.mark.gpu

BG2, BG3 = 0.09, 0.05  # background share of the rows: 2-d plans and the dense key (>= 121 tiles), 64^3 (74 tiles)
LIM = (-4.0, 4.0)


def sa():
    import vaex_amd.superagg as m
    return m


def _dev(a):
    from vaex_amd.device import DeviceArray
    return DeviceArray.from_numpy(a)


def _rounds_reset():
    from vaex_amd import _lib
    _lib.stat_read("tile_stream_rounds", reset=True)


def _assert_rounds(case):
    """The query since _rounds_reset() walked a unit in the rounds the case is there for."""
    from vaex_amd import _lib
    got = _lib.stat_read("tile_stream_rounds", reset=True)
    want = CASES[case][2]
    print(f"{case}: tile_stream_rounds = {got}")
    if want is None:
        assert got >= 2, f"{case}: pass B walked {got} round(s): the test checks nothing it is there for"
    else:
        assert got == want, f"{case}: pass B walked {got} round(s), not {want}"


def _mixed(rng, n, sigma, bg):
    """A binner column: normal(0, sigma) core, a share bg of uniform rows just past both limits,
    a NaN every 9973rd row."""
    v = rng.normal(0.0, sigma, n)
    rows = np.flatnonzero(rng.random(n) < bg)
    v[rows] = rng.uniform(LIM[0] - 0.02, LIM[1] + 0.02, len(rows))
    v[int(rng.integers(0, 9973))::9973] = np.nan
    return v


def _values(rng, n, dtype="float64", lim=1000):
    w = rng.integers(-lim, lim + 1, n).astype(dtype)
    w[::101] = np.nan
    return w


class Rows:
    """One row order of a data set: host columns, their HBM copies (made on first use, shared
    by the tests and never written), and the oracle's cell index of every row per grid."""

    def __init__(self, cols, binby):
        self.cols, self.binby = cols, binby
        self.n = len(next(iter(cols.values())))
        self._dev, self._idx = {}, {}

    def dev(self, name, n=None):
        if name not in self._dev:
            self._dev[name] = _dev(self.cols[name])
        return self._dev[name] if n is None else self._dev[name][:n]

    def binners(self, bins, n=None):
        return [oracle.Binner("scalar", self.cols[b][:n], vmin=LIM[0], vmax=LIM[1], bins=bins) for b in self.binby]

    def idx(self, bins, n=None):
        if bins not in self._idx:
            self._idx[bins] = oracle.bin_indices(self.binners(bins), self.n)
        return self._idx[bins][:n]

    def grid(self, bins, kind, data=None, n=None, moment=2):
        """oracle.compute_grid over the first n rows, on the cell indices computed once; data: a
        column's name, or an array."""
        n = self.n if n is None else n
        shape = (bins + 3,) * len(self.binby)
        if isinstance(data, str):
            data = self.cols[data]
        dname = None if data is None else str(data.dtype)
        g, _ = oracle.new_grid(kind, dname or "int64", shape)
        oracle.aggregate(kind, self.idx(bins, n), g, data=None if data is None else data[:n], moment=moment, dtype=dname)
        return g.reshape(shape, order="F")

    def gpu_grid(self, bins, n=None, dtype="float64"):
        bs = []
        for b in self.binby:
            g = getattr(sa(), "BinnerScalar_" + dtype)(b, LIM[0], LIM[1], bins)
            g.set_data(self.dev(b, n))
            bs.append(g)
        return sa().Grid(bs)


_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_rows():
    """The data sets live for this module only (a few GB of host memory and of HBM)."""
    yield
    _cache.clear()


def _shared(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def rows_2d():
    def make():
        rng = np.random.default_rng(510)
        n = CASES["c2"][1]
        cols = {"x": _mixed(rng, n, 0.05, BG2), "y": _mixed(rng, n, 0.05, BG2), "w": _values(rng, n)}
        cols["w2"] = np.roll(cols["w"], 50) * 2.0  # a second value column, its NaNs in other rows
        return Rows(cols, ["x", "y"])
    return _shared("2d", make)


def rows_2d_sorted():
    """rows_2d ordered by y's bin, then x's (two stable 16-bit radix passes over the 1024^2 cell
    index): whole tiles, and within them whole cells, in consecutive rows."""
    def make():
        r = rows_2d()
        idx = r.idx(1024)
        o = np.argsort((idx % 1027).astype(np.uint16), kind="stable")
        o = o[np.argsort((idx[o] // 1027).astype(np.uint16), kind="stable")]
        s = Rows({k: v[o] for k, v in r.cols.items()}, r.binby)
        s._idx[1024] = idx[o]
        return s
    return _shared("2d_sorted", make)


def rows_f32():
    def make():
        r = rows_2d()
        return Rows({k: v.astype(np.float32) for k, v in r.cols.items()}, r.binby)
    return _shared("f32", make)


def rows_3d():
    def make():
        rng = np.random.default_rng(511)
        n = CASES["two_slots_3d"][1]
        cols = {k: _mixed(rng, n, 0.1, BG3) for k in ("x", "y", "z")}
        cols["a"] = _values(rng, n)
        cols["b"] = np.roll(cols["a"], 50) * 2.0  # its NaNs in other rows than a's
        return Rows(cols, ["x", "y", "z"])
    return _shared("3d", make)


def _bin(grid, aggs):
    grid.bin(aggs)
    return [np.asarray(a).copy() for a in aggs]


def _count_sum(r, n=None):
    grid = r.gpu_grid(1024, n)
    c, s = sa().AggCount_int64(grid), sa().AggSum_float64(grid)
    s.set_data(r.dev("w", n), 0)
    return _bin(grid, [c, s])


# ---- 1. the C2 shape


def test_c2_count_sum_two_rounds():
    """1024^2, count + sum(w) of float64 columns: the plain-sum pass B (NV = 1)."""
    r = rows_2d()
    _rounds_reset()
    c, s = _count_sum(r)
    _assert_rounds("c2")
    np.testing.assert_array_equal(c, r.grid(1024, "count"))
    np.testing.assert_array_equal(s, r.grid(1024, "sum", "w"))
    # the same columns through the per-(workgroup, tile) regions, in this process
    os.environ["VH_TILE_STREAM"] = "0"
    try:
        c0, s0 = _count_sum(r)
    finally:
        os.environ.pop("VH_TILE_STREAM", None)
    np.testing.assert_array_equal(c0, c)
    np.testing.assert_array_equal(s0, s)


# ---- 2. min / max


def test_count_sum_min_max_one_column():
    """count + sum + min + max of one float64 column: the branch-light mm_simple entry loop.
    On 700^2 bins: with 28 LDS bytes per cell the 1024^2 grid has 258 tiles, which leaves pass A
    no LDS for the wide stream-out, and so no stream layout."""
    r = rows_2d()
    grid = r.gpu_grid(700)
    aggs = [sa().AggCount_int64(grid), sa().AggSum_float64(grid), sa().AggMin_float64(grid), sa().AggMax_float64(grid)]
    for a in aggs[1:]:
        a.set_data(r.dev("w"), 0)
    _rounds_reset()
    c, s, mn, mx = _bin(grid, aggs)
    _assert_rounds("mm_simple")
    np.testing.assert_array_equal(c, r.grid(700, "count"))
    np.testing.assert_array_equal(s, r.grid(700, "sum", "w"))
    np.testing.assert_array_equal(mn, r.grid(700, "min", "w"))
    np.testing.assert_array_equal(mx, r.grid(700, "max", "w"))


@pytest.mark.parametrize("order", ["shuffled", "sorted_y"])
def test_min_max_alone(order):
    """min + max without a count or sum: the extended run form, whose runs of one cell's
    entries cross chunk and round boundaries when whole cells lie in consecutive rows."""
    r = rows_2d() if order == "shuffled" else rows_2d_sorted()
    grid = r.gpu_grid(1024)
    mn, mx = sa().AggMin_float64(grid), sa().AggMax_float64(grid)
    mn.set_data(r.dev("w"), 0)
    mx.set_data(r.dev("w"), 0)
    _rounds_reset()
    mn, mx = _bin(grid, [mn, mx])
    _assert_rounds("minmax")
    np.testing.assert_array_equal(mn, r.grid(1024, "min", "w"))
    np.testing.assert_array_equal(mx, r.grid(1024, "max", "w"))


# ---- 3. two value slots


def _two_slots(r, bins, n, va, vb):
    grid = r.gpu_grid(bins, n)
    c, a, b = sa().AggCount_int64(grid), sa().AggSum_float64(grid), sa().AggSum_float64(grid)
    a.set_data(r.dev(va, n), 0)
    b.set_data(r.dev(vb, n), 0)
    got = _bin(grid, [c, a, b])
    return got, [r.grid(bins, "count", n=n), r.grid(bins, "sum", va, n=n), r.grid(bins, "sum", vb, n=n)]


def test_two_value_slots_2d():
    """count + sum(w) + sum(w2) on 1024^2: two float64 value slots, one batch per commit (two
    do not fit pass A's LDS with 258 tiles), over the first 8.6 M rows."""
    r, n = rows_2d(), CASES["two_slots_2d"][1]
    _rounds_reset()
    got, want = _two_slots(r, 1024, n, "w", "w2")
    _assert_rounds("two_slots_2d")
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_two_value_slots_3d_three_rounds():
    """count + sum(a) + sum(b) on 64^3 (one batch per commit) at the three-round ceiling."""
    r = rows_3d()
    _rounds_reset()
    got, want = _two_slots(r, 64, None, "a", "b")
    _assert_rounds("two_slots_3d")
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


# ---- 7. odd n, workgroups with different commit counts


def test_odd_rows_and_uneven_commit_counts():
    """An odd row count that is no multiple of the batch, nor its batches of the workgroups:
    the last row is binned alone, the last workgroups hold one commit less than the first (the
    table's empty tail rows), at two rounds."""
    r, n = rows_3d(), CASES["odd_tail"][1]
    assert n % 2 == 1 and n % 4096 and -(-n // 4096) % 256
    _rounds_reset()
    got, want = _two_slots(r, 64, n, "a", "b")
    _assert_rounds("odd_tail")
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


# ---- 4. moments


@pytest.mark.parametrize("stat", ["var", "std"])
def test_var_std_moment_2(stat):
    """df.var / df.std (the moment-2 run form beside sum and count of the column): the finish is
    the oracle's expression operation for operation (hostops.variance), and its three grids are
    exact, so the result is too."""
    import vaex_amd
    r = rows_2d()
    df = vaex_amd.from_arrays(x=r.dev("x"), y=r.dev("y"), w=r.dev("w"))
    _rounds_reset()
    got = np.asarray(getattr(df, stat)("w", binby=["x", "y"], limits=[list(LIM), list(LIM)], shape=700))
    _assert_rounds("var")
    m2, s, c = r.grid(700, "sum_moment", "w"), r.grid(700, "sum", "w"), r.grid(700, "count", "w")
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = s / c
        want = oracle.extract_central_part(m2 / c - mean ** 2)
        if stat == "std":
            want = np.sqrt(want)
    np.testing.assert_array_equal(got, want)


def test_moment_3_per_entry_form():
    """count(w) + sum(w) + AggSumMoment(w, 3): the per-entry pass B (MG).  Counts and sums are
    exact.  A term is pow(v, 3) on both sides, exact in the oracle (an integer below 2^30) and
    within 1 ulp on the device (the documented accuracy of its pow), after which a cell's
    partial sums are no integers any more and each addition may round: a cell of c terms is
    within 2 c eps of the sum of its |v|^3.  Cold cells hold a few rows, so there the bound is
    far below the smallest term a lost or repeated entry would change."""
    r = rows_2d()
    grid = r.gpu_grid(700)
    aggs = [sa().AggCount_float64(grid), sa().AggSum_float64(grid), sa().AggSumMoment_float64(grid, 3)]
    for a in aggs:
        a.set_data(r.dev("w"), 0)
    _rounds_reset()
    c, s, m3 = _bin(grid, aggs)
    _assert_rounds("moment3")
    want_c = r.grid(700, "count", "w")
    np.testing.assert_array_equal(c, want_c)
    np.testing.assert_array_equal(s, r.grid(700, "sum", "w"))
    bound = 2 * want_c * np.finfo(np.float64).eps * r.grid(700, "sum_moment", np.abs(r.cols["w"]), moment=3)
    err = np.abs(m3 - r.grid(700, "sum_moment", "w", moment=3))
    print("moment 3: largest error", err.max(), "largest error / bound", np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound)


# ---- 5. float32


def test_float32_binners_and_values():
    """float32 binners with float32 values: the typed pass A, 4-byte staged values (narrow
    slots in pass B)."""
    r = rows_f32()
    grid = r.gpu_grid(1024, dtype="float32")
    c, s = sa().AggCount_int64(grid), sa().AggSum_float32(grid)
    s.set_data(r.dev("w"), 0)
    _rounds_reset()
    c, s = _bin(grid, [c, s])
    _assert_rounds("f32")
    np.testing.assert_array_equal(c, r.grid(1024, "count"))
    np.testing.assert_array_equal(s, r.grid(1024, "sum", "w"))


# ---- 6. the dense groupby grid


def dense_rows():
    """int32 keys over about 1e6 values (key2: the same over half the range), a hot core of a few
    tiles and the uniform background; float64 / int8 / float32 values and a float64 column to
    filter on."""
    def make():
        rng = np.random.default_rng(512)
        n = CASES["dense_f64"][1]
        keys = np.rint(rng.normal(500_000, 5_000, n)).astype(np.int32)
        rows = np.flatnonzero(rng.random(n) < BG2)
        keys[rows] = rng.integers(5, 1_000_005, len(rows), dtype=np.int32)
        cols = {"key": keys, "key2": keys >> 1, "v": _values(rng, n), "i8": rng.integers(-100, 101, n).astype(np.int8),
                "f32": _values(rng, n, "float32"), "f": rng.integers(-1000, 1001, n).astype(np.float64)}
        return Rows(cols, ["key"])
    return _shared("dense", make)


def _dense_want(r, value, keep=None, key="key"):
    """(keys, count(*), sum(value)) per occupied key, in key order, as np.unique / np.bincount
    give them in test_dense_groupby_grid (NaN values left out of the sums)."""
    keys, v = r.cols[key], r.cols[value].astype(np.float64)
    if keep is not None:
        keys, v = keys[keep], v[keep]
    kmin = int(keys.min())
    cnt = np.bincount(keys - kmin)
    tot = np.bincount(keys - kmin, weights=np.where(np.isnan(v), 0.0, v), minlength=len(cnt))
    occ = np.flatnonzero(cnt)
    return occ + kmin, cnt[occ], tot[occ]


def test_dense_groupby_float64():
    """The dense-key groupby (ordinal pass A), sum + count(*) of a float64 column."""
    import vaex_amd
    r = dense_rows()
    df = vaex_amd.from_arrays(key=r.dev("key"), v=r.dev("v"))
    _rounds_reset()
    g = df.groupby("key", agg={"v": ["sum", "count"]}, sort=True)
    _assert_rounds("dense_f64")
    uk, cnt, tot = _dense_want(r, "v")
    np.testing.assert_array_equal(g["key"].to_numpy(), uk)
    np.testing.assert_array_equal(g["v"].to_numpy(), cnt)
    np.testing.assert_array_equal(g["v_sum"].to_numpy(), tot)


def test_dense_groupby_int8_float32_packed():
    """int8 + float32 sums: narrow 4-byte slots, two packed in one stream (PK).  On half the
    key range: the groupby's own count(*) rides along, and with 20 LDS bytes per cell about
    1e6 cells are 260 tiles, which leaves pass A no LDS for the wide stream-out, and so no
    stream layout."""
    import vaex_amd
    r = dense_rows()
    df = vaex_amd.from_arrays(key2=r.dev("key2"), i8=r.dev("i8"), f32=r.dev("f32"))
    _rounds_reset()
    g = df.groupby("key2", agg={"i8": "sum", "f32": "sum"}, sort=True)
    _assert_rounds("dense_i8_f32")
    uk, _, tot8 = _dense_want(r, "i8", key="key2")
    np.testing.assert_array_equal(g["key2"].to_numpy(), uk)
    np.testing.assert_array_equal(g["i8"].to_numpy().astype(np.float64), tot8)
    np.testing.assert_array_equal(g["f32"].to_numpy().astype(np.float64), _dense_want(r, "f32", key="key2")[2])


def test_dense_groupby_filtered_shared_mask():
    """A filtered frame on the dense route: the filter is every aggregator's keep mask, applied
    per row by the ordinal pass A (MK); masked rows leave their segments shorter, not fewer."""
    import vaex_amd
    r = dense_rows()
    base = vaex_amd.from_arrays(key=r.dev("key"), v=r.dev("v"), f=r.dev("f"))
    _rounds_reset()
    g = base[base.f > -400].groupby("key", agg={"v": ["sum", "count"]}, sort=True)
    _assert_rounds("dense_f64_filtered")
    uk, cnt, tot = _dense_want(r, "v", keep=r.cols["f"] > -400)
    np.testing.assert_array_equal(g["key"].to_numpy(), uk)
    np.testing.assert_array_equal(g["v"].to_numpy(), cnt)
    np.testing.assert_array_equal(g["v_sum"].to_numpy(), tot)
