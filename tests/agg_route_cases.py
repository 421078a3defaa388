"""Inputs and references for tests/test_gpu_agg_routes.py -- NumPy and the CPU oracle only.

Every case is deterministic (seeds are ``zlib.crc32`` of the case name) and importable
without a GPU; tests/test_agg_route_cases.py checks on the CPU that the cases satisfy what the
GPU tests rely on (sums that fit, coverage of the edge cells and the special values, ...).

A *grid case* (``grid_case``) holds the binner columns of one of the five grids of the bin
routes; a *value case* (``value_case``) holds the aggregator columns of one dtype over it:

=========  ================================================================  ==========
grid       binners                                                           cells
=========  ================================================================  ==========
small1     BinnerScalar_float64(-3, 3, 32) with a binner mask                35
small2     BinnerOrdinal_int8(100, 5) with a mask x byte-swapped
           BinnerScalar_int32(-1000, 1000, 20)                               103 x 23
setord     BinnerSetOrdinal over an ordered_set_int32 of 50 keys             53
large      BinnerOrdinal_int32(20000, 0), ~300 distinct keys                 20 003
zero_d     none (Grid([]), explicit length)                                  1
=========  ================================================================  ==========
"""
import functools
import math
import zlib
from fractions import Fraction

import numpy as np

from oracle import oracle

DTYPES = list(oracle.DTYPES)
GRIDS = ("small1", "small2", "setord", "large", "zero_d")
KINDS = ("count", "sum", "min", "max", "sum_moment", "first")
MOMENTS = (0, 1, 2, 3)
N_MAIN = 20011  # no multiple of 8, more than 9 x 2048, far below the tile engine's 2**20
TAILS = (1, 7, 8, 9, 2047, 2048, 2049)  # around RU = 8 and the 2048-row step of k_first_small
N_TWO_CHUNKS = 2 ** 24 + 9  # host rows: two stager chunks
MASK_BYTES = np.array([0, 1, 1, 1, 2, 255], dtype=np.uint8)  # only 1 keeps (aggregator) / masks (binner)

# ---- the exclusions (the only ones; each GPU test that applies one names its flag) ----------
# The reference's AggSumMoment swaps the *upcast* 64-bit value (superagg.cpp:415-417), so a
# byte-swapped column narrower than 8 bytes yields garbage by design: not compared.
SWAPPED_MOMENT_NEEDS_8_BYTES = True
# The reference's AggFirst ignores masks ("TODO: masked support"): first runs without one.
FIRST_TAKES_NO_MASK = True
# +-finfo(float64).max overflows a float64 sum in an order-dependent way: left out of the
# columns that sum and sum_moment read.
SUMS_LEAVE_OUT_F64_MAX = True
# Whether subnormal float64 addends survive the hardware float64 atomics is unmeasured (its
# own issue): left out of the columns that sum and sum_moment of float64 read.
SUMS_LEAVE_OUT_F64_SUBNORMALS = True
# A uint64 cell that holds iinfo.max overflows with any other non-zero addend, and a second
# value >= 2**63 overflows it too: on a one-cell grid the sums carry 2**63 + 12345 only.
U64_MAX_NEEDS_ITS_OWN_CELL = True

# integer AggSumMoment inputs: |v| <= 2**20 for moments 0-2, <= 2**10 for moments 3 and 4, so
# that every cell's exact total stays below 2**53 and the reference's detour through double
# (grid = (G)((double)grid + pow(...))) is exact and order-free
MOMENT_BOUND = {0: 2 ** 20, 1: 2 ** 20, 2: 2 ** 20, 3: 2 ** 10, 4: 2 ** 10}


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def swapped(a):
    """The same values in big-endian byte order (1-byte dtypes have none: unchanged)."""
    return a.astype(a.dtype.newbyteorder(">"))


def native(a):
    return a.astype(a.dtype.newbyteorder("="))


def mask_bytes(name, n):
    return MASK_BYTES[rng_for(name).integers(0, len(MASK_BYTES), n)]


# ---- grids ---------------------------------------------------------------------------------
class GridCase:
    """binners: dicts for the GPU test (kind scalar / ordinal / set, data, mask, parameters);
    specs: the oracle binners; idx: the cell of every row; edge_cells: per dimension the edge
    indices (0 NaN / masked, 1 underflow, shape - 1 overflow) the inputs must reach."""

    def __init__(self, name, n, binners, specs, edge_cells):
        self.name, self.n, self.binners, self.specs, self.edge_cells = name, n, binners, specs, edge_cells
        self.shape = oracle.grid_shape(specs)
        self.length = int(np.prod(self.shape)) if self.shape else 1
        self.idx = (oracle.bin_indices(specs, n) if specs else np.zeros(n, np.uint64)).astype(np.int64)
        self.idx.setflags(write=False)

    def dim_index(self, d):
        """Every row's index along dimension d."""
        stride = oracle.grid_strides(self.specs)[d]
        return (self.idx // stride) % self.shape[d]


def _scatter(rng, base, specials, every):
    """base with the specials scattered (cyclically) over about 1 / every of its rows."""
    n = len(base)
    rows = rng.choice(n, size=(n + every - 1) // every, replace=False)
    base[rows] = np.array(specials, dtype=base.dtype)[np.arange(len(rows)) % len(specials)]
    return base


SET_KEYS = 50


@functools.lru_cache(maxsize=None)
def grid_case(name, n=N_MAIN):
    rng = rng_for(f"grid-{name}-{n}")
    if name == "small1":
        x = _scatter(rng, rng.normal(0, 1.5, n),
                     [np.nan, np.inf, -np.inf, -3.0, 3.0, np.nextafter(3.0, -np.inf)], 10)
        m = mask_bytes(f"bmask-{name}-{n}", n)
        binners = [dict(kind="scalar", dtype="float64", data=x, mask=m, vmin=-3, vmax=3, bins=32)]
        specs = [oracle.Binner("scalar", x, vmin=-3, vmax=3, bins=32, mask=m)]
        edges = [(0, 1, 34)]
    elif name == "small2":
        k8 = _scatter(rng, rng.integers(-20, 126, n).astype(np.int8), [-128, 127, 4, 5, 104, 105], 50)  # around [5, 105)
        m = mask_bytes(f"bmask-{name}-{n}", n)
        k32 = swapped(rng.integers(-1100, 1100, n).astype(np.int32))  # around [-1000, 1000)
        binners = [dict(kind="ordinal", dtype="int8", data=k8, mask=m, count=100, min=5),
                   dict(kind="scalar", dtype="int32", data=k32, mask=None, vmin=-1000, vmax=1000, bins=20)]
        specs = [oracle.Binner("ordinal", k8, ordinal_count=100, min_value=5, mask=m),
                 oracle.Binner("scalar", k32, vmin=-1000, vmax=1000, bins=20)]
        edges = [(0, 1, 102), (1, 22)]  # an unmasked integer scalar binner has no NaN cell
    elif name == "setord":
        pool = rng.choice(np.arange(-10 ** 6, 10 ** 6), size=SET_KEYS + 10, replace=False).astype(np.int32)
        pool[0], pool[1] = np.iinfo(np.int32).min, np.iinfo(np.int32).max
        set_keys = pool[:SET_KEYS].copy()  # the other 10 keys of the column are not in the set
        keys = pool[rng.integers(0, len(pool), n)]
        ref = oracle.OrderedSet(nmaps=1)  # first-appearance ordinals, as the GPU set assigns them
        ref.update(set_keys)
        ordinals = ref.map_ordinal(keys)  # -1: not in the set -> the underflow cell
        binners = [dict(kind="set", dtype="int32", data=keys, mask=None, set_keys=set_keys, ordinals=ordinals)]
        specs = [oracle.Binner("ordinal", ordinals, ordinal_count=SET_KEYS, min_value=0)]
        edges = [(1,)]
    elif name == "large":
        distinct = rng.choice(20000, size=300, replace=False).astype(np.int32)
        keys = _scatter(rng, distinct[rng.integers(0, len(distinct), n)],
                        [-1, -5, np.iinfo(np.int32).min, 20000, 20001, np.iinfo(np.int32).max], 20)
        binners = [dict(kind="ordinal", dtype="int32", data=keys, mask=None, count=20000, min=0)]
        specs = [oracle.Binner("ordinal", keys, ordinal_count=20000, min_value=0)]
        edges = [(1, 20002)]
    elif name == "zero_d":
        binners, specs, edges = [], [], []
    else:
        raise ValueError(name)
    for b in binners:
        for key in ("data", "mask"):
            if b[key] is not None:
                b[key].setflags(write=False)
    return GridCase(name, n, binners, specs, edges)


# ---- value columns -------------------------------------------------------------------------
def palette(dtype, for_sum=False):
    """The special values of a dtype (64-bit integer extremes are placed by _place_64)."""
    dt = np.dtype(dtype)
    if dt.kind == "b":
        return [False, True]
    if dt.kind in "iu":
        info = np.iinfo(dt)
        small = ([-1] if dt.kind == "i" else []) + [0, 1]
        return small if dt.itemsize == 8 else [info.min, info.max] + small
    fi = np.finfo(dt)
    sub, half = fi.smallest_subnormal, fi.tiny / 2
    out = [np.nan, np.inf, -np.inf, 0.0, -0.0]
    if not (for_sum and dt.itemsize == 8 and SUMS_LEAVE_OUT_F64_SUBNORMALS):
        out += [sub, -sub, half, -half]  # float32 subnormals are exact in the float64 accumulator
    if not (for_sum and dt.itemsize == 8 and SUMS_LEAVE_OUT_F64_MAX):
        out += [fi.max, -fi.max]
    return [dt.type(v) for v in out]


def _random_values(rng, dt, n):
    if dt.kind == "b":
        return rng.random(n) < 0.5
    if dt.kind == "f":
        return rng.normal(0, 1, n).astype(dt)
    info = np.iinfo(dt)
    if dt.itemsize == 8:  # a small range: the extremes are placed per cell (_place_64)
        return rng.integers(-1000 if dt.kind == "i" else 0, 1000, n).astype(dt)
    return rng.integers(info.min, int(info.max) + 1, n, dtype=np.int64 if dt.kind == "i" else np.uint64).astype(dt)


def _extreme(v):
    dt = v.dtype
    if dt.kind == "f":
        return np.isinf(v) | (np.abs(v) == np.finfo(dt).max)
    if dt.kind in "iu" and dt.itemsize < 8:
        return (v == np.iinfo(dt).min) | (v == np.iinfo(dt).max)
    return np.zeros(len(v), bool)


U64_HIGH = 2 ** 63 + 12345


def _place_64(values, idx, keep):
    """Put iinfo.max / iinfo.min (uint64: iinfo.max / 2**63 + 12345) of a 64-bit column into one
    kept row each, in cells of their own whose other rows cannot carry the cell's sum (of the
    kept rows, of all rows, or of any subset) out of range."""
    dt = values.dtype
    info = np.iinfo(dt)
    cells, counts = np.unique(idx[keep == 1], return_counts=True)
    if len(cells) == 0:
        raise ValueError("no kept row")
    if (counts >= 3).sum() >= 2:  # the least crowded cells that still hold other kept rows
        cells, counts = cells[counts >= 3], counts[counts >= 3]
    cells = cells[np.argsort(counts, kind="stable")]
    row_of = lambda c: int(np.flatnonzero((idx == c) & (keep == 1))[0])
    if len(cells) == 1:
        if dt.kind == "i":  # max + min = -1: both fit one cell
            rows = np.flatnonzero((idx == cells[0]) & (keep == 1))
            values[rows[0]], values[rows[1]] = info.max, info.min
        else:  # U64_MAX_NEEDS_ITS_OWN_CELL
            values[row_of(cells[0])] = U64_HIGH
        return values
    a, b = cells[0], cells[1]
    if dt.kind == "i":
        values[idx == a] = -np.abs(values[idx == a])  # max + (<= 0)
        values[idx == b] = np.abs(values[idx == b])   # min + (>= 0)
        values[row_of(a)], values[row_of(b)] = info.max, info.min
    else:
        values[idx == a] = 0
        values[row_of(a)], values[row_of(b)] = info.max, U64_HIGH
    return values


class ValueCase:
    """The aggregator columns of one dtype over one grid case:

    values   the whole palette (count, min, max, first);
    sums     what sum and float sum_moment read (the SUMS_LEAVE_OUT_* flags applied; the
             same array as ``values`` where they change nothing);
    bounded  {bound: integer column with |v| <= bound} for integer sum_moment;
    order    AggFirst's order column: few distinct values, the dtype's max, NaN and +-0.0;
    keep     the aggregator keep mask."""

    def __init__(self, grid, dtype):
        self.grid, self.dtype = grid, dtype
        dt = np.dtype(dtype)
        n, name = grid.n, f"{grid.name}-{dtype}-{grid.n}"
        self.keep = mask_bytes(f"keep-{name}", n)

        def column(for_sum):
            rng = rng_for(f"values-{name}")  # the same stream: the columns differ in the specials only
            v = _scatter(rng, _random_values(rng, dt, n), palette(dt, for_sum), 5)
            # The extremes (+-inf, +-finfo.max, iinfo.min / max) decide a cell's min, max and
            # float sum alone.  They stay out of every other occupied cell, so that half the
            # cells are decided by ordinary values; `tame` has none at all (one-cell grids,
            # where that half does not exist, run it beside the full column).
            tame = v.copy()
            ext = _extreme(v)
            tame[ext] = _random_values(rng, dt, int(ext.sum()))
            occupied = np.unique(grid.idx)
            calm = ext & np.isin(grid.idx, occupied[1::2])
            v[calm] = tame[calm]
            if dt.kind in "iu" and dt.itemsize == 8:
                v = _place_64(v, grid.idx, self.keep)
            return v, tame

        self.values, self.tame = column(False)
        self.sums, self.tame_sums = column(True) if dt.kind == "f" and dt.itemsize == 8 else (self.values, self.tame)
        self.tame.setflags(write=False)
        self.tame_sums.setflags(write=False)
        self.bounded = {}
        if dt.kind in "iu":
            info = np.iinfo(dt)
            for bound in sorted(set(MOMENT_BOUND.values())):
                rng = rng_for(f"bounded-{bound}-{name}")
                lo, hi = max(int(info.min), -bound), min(int(info.max), bound)
                v = rng.integers(lo, hi + 1, n).astype(dt)
                self.bounded[bound] = _scatter(rng, v, [lo, hi] + ([-1] if dt.kind == "i" else []) + [0, 1], 5)
        rng = rng_for(f"order-{name}")
        if dt.kind == "b":
            self.order = rng.random(n) < 0.5
        elif dt.kind == "f":
            pool = np.array([-1.5, -0.0, 0.0, 2.0, np.nan, np.finfo(dt).max], dtype=dt)
            self.order = pool[rng.choice(len(pool), size=n, p=[0.3, 0.2, 0.2, 0.1, 0.1, 0.1])]
        else:
            info = np.iinfo(dt)
            pool = np.array(([info.min, -1] if dt.kind == "i" else []) + [0, 3, info.max], dtype=dt)
            p = [0.3, 0.2, 0.2, 0.2, 0.1] if dt.kind == "i" else [0.5, 0.4, 0.1]
            self.order = pool[rng.choice(len(pool), size=n, p=p)]
        for a in (self.keep, self.values, self.sums, self.order, *self.bounded.values()):
            a.setflags(write=False)

    def moment_column(self, moment):
        """What sum_moment of this dtype reads for `moment`."""
        if np.dtype(self.dtype).kind in "iu":
            return self.bounded[MOMENT_BOUND[moment]]
        return self.sums  # floats; bool is 0 / 1

    def column(self, kind, moment=None):
        if kind == "sum":
            return self.sums
        if kind == "sum_moment":
            return self.moment_column(moment)
        return self.values

    def variants(self, kind, moment=None):
        """[(label, column)] a kind runs over: its column, and on a one-cell grid the tame one
        too (there the extremes of the full column decide the only cell)."""
        col = self.column(kind, moment)
        out = [("full", col)]
        if self.grid.length == 1 and kind != "first":
            tame = self.tame_sums if col is self.sums else self.tame if col is self.values else None
            if tame is not None and not np.array_equal(_bits_of(tame), _bits_of(col)):
                out.append(("tame", tame))
        return out


def _bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def value_case(grid_name, dtype, n=N_MAIN):
    return ValueCase(grid_case(grid_name, n), dtype)


class TwoChunkCase:
    """small1 over N_TWO_CHUNKS host rows (two stager chunks: narrow partials flush twice into
    one grid): the main case's columns repeated cyclically, which costs no generator pass."""

    def __init__(self):
        main, vc = grid_case("small1"), value_case("small1", "int16")
        b = main.binners[0]
        x, m = np.resize(b["data"], N_TWO_CHUNKS), np.resize(b["mask"], N_TWO_CHUNKS)
        self.grid = GridCase("small1", N_TWO_CHUNKS, [dict(b, data=x, mask=m)],
                             [oracle.Binner("scalar", x, vmin=-3, vmax=3, bins=32, mask=m)], main.edge_cells)
        self.values, self.keep = np.resize(vc.values, N_TWO_CHUNKS), np.resize(vc.keep, N_TWO_CHUNKS)


@functools.lru_cache(maxsize=None)
def two_chunk_case():
    return TwoChunkCase()


# ---- references ----------------------------------------------------------------------------
def expected(grid, kind, data=None, data2=None, mask=None, moment=2, rows=None, init=None):
    """(grid, order grid or None) of the CPU oracle, flat in the grid's 1-d cell order, over
    the rows `rows` (a slice; default all) of the grid case; init: the cells the value grid
    holds before the rows (default: the aggregator's fill)."""
    sl = slice(None) if rows is None else rows
    idx = grid.idx[sl].astype(np.uint64)
    name = None if data is None else oracle._dtype_info(np.asarray(data))[0]
    g, g2 = oracle.new_grid(kind, name or "int64", grid.shape)
    if init is not None:
        g[:] = init
    cut = lambda a: None if a is None else np.ascontiguousarray(a[sl])
    oracle.aggregate(kind, idx, g, data=cut(data), data2=cut(data2), mask=cut(mask), moment=moment, grid2=g2,
                     dtype=name)
    return g, g2


def shaped(grid, flat):
    """A flat cell array as the aggregator's array view shows it (Fortran order)."""
    return flat.reshape(grid.shape, order="F") if grid.shape else flat.reshape(())


class FloatSumRef:
    """Per-cell exact reference of a float sum: fsum over the kept, non-NaN terms (float64),
    their count m and sum of magnitudes, and which cells hold a non-finite term."""

    def __init__(self, exact, count, abssum, nonfinite, allowance):
        self.exact, self.count, self.abssum, self.nonfinite, self.allowance = exact, count, abssum, nonfinite, allowance

    def bound(self):
        """Any float64 summation order of m addends errs by at most (m - 1) 2^-53 sum|v| to
        first order; m 2^-52 sum|v| leaves room for the two-level sum (LDS partial, then the
        global grid) and the second-order terms.  Plus the per-term allowance (moment 3)."""
        return self.count * 2.0 ** -52 * self.abssum + self.allowance


def float_sum_reference(idx, length, data, mask=None, moment=None):
    """FloatSumRef of sum(data) (moment None) or of sum_moment(data, moment) over the cells
    idx.  Terms: v upcast to float64 (exact), 1, v, v * v (the product the kernel computes, which
    is the correctly rounded square), or the exact v**3 with 4 ulp of |v|**3 allowed per term --
    the bound this project holds the device pow to (tests/expr_np.py)."""
    v = native(np.asarray(data)).astype(np.float64)
    ok = ~np.isnan(v)
    if mask is not None:
        ok &= np.asarray(mask) == 1
    rows = np.flatnonzero(ok)
    rows = rows[np.argsort(idx[rows], kind="stable")]
    cells, starts = np.unique(idx[rows], return_index=True)
    ends = np.append(starts[1:], len(rows))
    exact, count = np.zeros(length), np.zeros(length)
    abssum, allowance, nonfinite = np.zeros(length), np.zeros(length), np.zeros(length, bool)
    with np.errstate(over="ignore", invalid="ignore"):
        if moment in (None, 1):
            terms = v
        elif moment == 0:
            terms = np.ones_like(v)
        elif moment == 2:
            terms = v * v
        else:
            assert moment == 3, moment
            terms = v ** 3  # magnitudes, allowance and the non-finite cells; the sum below is exact
    for c, s, e in zip(cells.tolist(), starts.tolist(), ends.tolist()):
        r = rows[s:e]
        t = terms[r]
        count[c] = len(r)
        if not np.isfinite(t).all():
            nonfinite[c] = True
            continue
        abssum[c] = math.fsum(np.abs(t).tolist())
        if moment == 3:
            exact[c] = float(sum(Fraction(x) ** 3 for x in v[r].tolist()))
            allowance[c] = math.fsum((4 * np.spacing(np.abs(t))).tolist())
        else:
            exact[c] = math.fsum(t.tolist())
    return FloatSumRef(exact, count, abssum, nonfinite, allowance)


def check_float_sum(got, oracle_flat, ref, what=""):
    """The comparison rule of float sums and float moments: a cell with a kept +-inf equals the
    oracle exactly (inf, -inf, or NaN where both signs meet: order-independent while the finite
    addends stay below 1e300); every other cell lies within ref.bound() of the exact sum --
    an untouched cell (bound 0) keeps its 0."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, order="F")
    nf = ref.nonfinite
    np.testing.assert_array_equal(got[nf], oracle_flat[nf], err_msg=f"{what}: cells with a non-finite addend")
    err = np.abs(got[~nf] - ref.exact[~nf])
    bad = ~(err <= ref.bound()[~nf])  # NaN fails
    assert not bad.any(), (f"{what}: {int(bad.sum())} cells off the exact sum by more than m * 2^-52 * sum|v|; "
                           f"worst {err[bad].max() if bad.any() else 0} at cell {np.flatnonzero(~nf)[bad][:5]}")


def check_exact(got, exp_flat, grid, what="", bits_where_nonzero=False):
    """assert_array_equal (NaN == NaN, -0.0 == 0.0) against the oracle's flat grid; with
    bits_where_nonzero also bit for bit wherever the expected value is not a zero (the
    reference's winner between -0.0 and 0.0 depends on the row order, which the GPU has not)."""
    got = np.asarray(got)
    exp = shaped(grid, exp_flat)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    np.testing.assert_array_equal(got, exp, err_msg=what)
    if bits_where_nonzero and got.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        nz = ~(exp == 0)
        np.testing.assert_array_equal(np.ascontiguousarray(got)[nz].view(u), np.ascontiguousarray(exp)[nz].view(u),
                                      err_msg=what + " (bits)")


def check_bits(got, exp_flat, grid, what=""):
    """Bit for bit (AggFirst's value and order grids)."""
    got = np.ascontiguousarray(np.asarray(got))
    exp = np.ascontiguousarray(shaped(grid, exp_flat))
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    np.testing.assert_array_equal(got.reshape(-1).view(u), exp.reshape(-1).view(u), err_msg=what)
