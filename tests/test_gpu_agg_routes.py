"""Every small-grid and generic aggregation route of vh_grid_bin at edge values.

Each test bins a case of tests/agg_route_cases.py once, asserts from the TimedScope counters
that the route it names ran (and no other), and only then compares with the CPU oracle:

route (kernel)                          forced by                                 counters
--------------------------------------  ----------------------------------------  ---------------------------------
cells (k_cells_dim + k_agg_lds_c,       small1 / small2 / zero_d, one non-fusable bin_cells >= 1, bin_aggregate_lds
wide and NARROW)                        aggregator per bin                        == 1
fused small (k_small_fused)             small1, eight count / sum aggregators     bin_aggregate_lds == 1
fused small, budget split               small2, the same eight                    bin_aggregate_lds == 3
plan-index LDS (k_agg_lds)              setord, one non-fusable aggregator        bin_aggregate_lds == 1, no cells
global atomics (k_idx_dim + k_agg)      large, one aggregator                     bin_indices == 1, bin_aggregate == 1
fused float64, generic plan             small2 / setord, count(*) + masked        bin_fused_lds == 1
(k_fused<true, 0>)                      count(float64) + sum(float64)
fused, global (k_fused<false, 0>)       large, the same three                     bin_fused_global == 1
first, LDS (k_first_small)              small1 / small2 / zero_d                  bin_first_lds == 1
first, index path (k_first_a/b/c)       large, setord                             bin_indices == 1, bin_aggregate == 1

A native float64 count or sum is *fusable*: alone it takes k_fused (or k_reduce0), never the
routes above.  It reaches k_agg_lds_c / k_agg_lds / k_agg only beside a non-fusable aggregator
in the same bin, so those two run with a companion AggMax (same mask: a masked sum beside an
unmasked max on the large grid is split off and fused again) and the aggregate counters read 2.

Comparison rules: counts, integer sums and integer moments equal the oracle exactly; min / max
by assert_array_equal (-0.0 == 0.0: the reference's winner between the zeros depends on the
row order) and bit for bit where the expected value is not a zero; first bit for bit, value
and order grid; float sums and float moments against the per-cell math.fsum within
m * 2^-52 * sum|v| (agg_route_cases.FloatSumRef.bound), cells holding +-inf exactly as the
oracle."""
import numpy as np
import pytest

import agg_route_cases as arc

pytestmark = pytest.mark.gpu

COUNTERS = ("bin_cells", "bin_indices", "bin_aggregate", "bin_aggregate_lds", "bin_first_lds", "bin_fused_lds",
            "bin_fused_global", "bin_small_f64", "bin_reduce0", "tile_reduce", "first_scatter")
CELL_GRIDS = ("small1", "small2", "zero_d")
AGG_NAME = {"count": "AggCount_", "sum": "AggSum_", "min": "AggMin_", "max": "AggMax_", "first": "AggFirst_",
            "sum_moment": "AggSumMoment_"}
# (kind, moment) of the main sweep
KIND_LIST = [("count", None), ("sum", None), ("min", None), ("max", None)] + \
            [("sum_moment", m) for m in arc.MOMENTS] + [("first", None)]


def sa():
    import vaex_amd.superagg as m
    return m


def _agg_cls(kind, dtype, flip):
    return getattr(sa(), AGG_NAME[kind] + np.dtype(dtype).newbyteorder("=").name + ("_non_native" if flip else ""))


def _binner_cls(prefix, data):
    from vaex_amd.utils import find_type_from_dtype
    return find_type_from_dtype(sa(), prefix, data.dtype)


class Columns:
    """Hands the columns of one test to the binners and aggregators: as they are (host), or as
    DeviceArrays -- one upload per column -- `offsets[role]` elements past an aligned
    allocation (roles: binner, bmask, value, order, keep)."""

    def __init__(self, loc="device", offsets=None):
        self.loc, self.offsets, self.cache = loc, offsets or {}, {}

    def put(self, role, a):
        if self.loc == "host":
            return a
        from vaex_amd.device import DeviceArray
        off = self.offsets.get(role, 0)
        key = (id(a), off)
        if key not in self.cache:
            padded = np.zeros(len(a) + off, dtype=a.dtype)
            padded[off:] = a
            self.cache[key] = (DeviceArray.from_numpy(padded)[off:], a)  # (a: keeps id(a) unique)
        return self.cache[key][0]


_SETS = {}


def _gpu_set(b):
    from vaex_amd import superutils
    key = b["set_keys"].tobytes()
    if key not in _SETS:
        s = superutils.ordered_set_int32()
        s.update(b["set_keys"])
        assert len(s) == len(b["set_keys"])
        # first-appearance ordinals, -1 for the keys that are not in the set: what the oracle binner reads
        np.testing.assert_array_equal(np.asarray(s.map_ordinal(b["data"])), b["ordinals"])
        _SETS[key] = s
    return _SETS[key]


def _make_grid(g, cols):
    binners = []
    for i, b in enumerate(g.binners):
        if b["kind"] == "scalar":
            gb = _binner_cls("BinnerScalar_", b["data"])(f"b{i}", b["vmin"], b["vmax"], b["bins"])
        elif b["kind"] == "ordinal":
            gb = _binner_cls("BinnerOrdinal_", b["data"])(f"b{i}", b["count"], b["min"])
        else:
            s = _gpu_set(b)
            gb = sa().BinnerSetOrdinal(f"b{i}", s, len(s))
        gb.set_data(cols.put("binner", b["data"]))
        if b["mask"] is not None:
            gb.set_data_mask(cols.put("bmask", b["mask"]))
        binners.append(gb)
    return sa().Grid(binners)


def _spec(kind, data=None, mask=None, data2=None, moment=None, flip=False, dtype=None, prefill=None):
    return dict(kind=kind, data=data, mask=mask, data2=data2, moment=moment, flip=flip,
                dtype=dtype if data is None else data.dtype, prefill=prefill)


def _bin(g, specs, cols=None, rows=None):
    """One Grid.bin of the aggregators `specs` over the grid case g (rows: a slice of it, device
    columns only); returns ([(value grid, order grid or None)], counters, aggregators)."""
    from vaex_amd import _lib
    cols = cols or Columns()
    cut = (lambda d: d) if rows is None else (lambda d: d[rows])
    grid = _make_grid(g, cols)
    if rows is not None:
        for gb, b in zip(grid.binners, g.binners):
            gb.set_data(cut(cols.put("binner", b["data"])))
            if b["mask"] is not None:
                gb.set_data_mask(cut(cols.put("bmask", b["mask"])))
    aggs = []
    for s in specs:
        a = _agg_cls(s["kind"], s["dtype"], s["flip"])(grid, *([s["moment"]] if s["kind"] == "sum_moment" else []))
        if s["data"] is not None:
            a.set_data(cut(cols.put("value", s["data"])), 0)
        if s["kind"] == "first":
            a.set_data(cut(cols.put("order", s["data2"])), 1)
        if s["mask"] is not None:
            a.set_data_mask(cut(cols.put("keep", s["mask"])))
        if s["prefill"] is not None:
            np.asarray(a)[...] = arc.shaped(g, s["prefill"])
        aggs.append(a)
    n = g.n if rows is None else len(range(*rows.indices(g.n)))
    _lib.timing_enable(True)
    _lib.timing_reset()
    try:
        grid.bin(aggs, *([] if g.binners else [n]))
        _lib.synchronize()
        counters = {c: _lib.timing_read(c)[0] for c in COUNTERS}
    finally:
        _lib.timing_enable(False)
    outs = [(np.asarray(a).copy(), a.order_grid() if s["kind"] == "first" else None) for a, s in zip(aggs, specs)]
    return outs, counters, aggs


def _assert_route(counters, what, **expect):
    """Every counter equals its expected number (0 where not named); ('>=', k) for at least k."""
    for c in COUNTERS:
        e = expect.get(c, 0)
        ok = counters[c] >= e[1] if isinstance(e, tuple) else counters[c] == e
        assert ok, f"{what}: {c} = {counters[c]}, expected {e}; all counters: {counters}"


def _fusable(kind, col, flip):
    return kind in ("count", "sum") and col.dtype == np.float64 and not flip


def _route(grid_name, kind, naggs=1, chunks=1):
    """The counters of `naggs` non-fusable aggregators of one kind, one bin, `chunks` chunks."""
    if kind == "first":
        if grid_name in CELL_GRIDS:
            return dict(bin_cells=chunks, bin_first_lds=naggs * chunks)
        return dict(bin_indices=chunks, bin_aggregate=naggs * chunks)  # k_first_a/b/c; first_scatter stays 0
    if grid_name in CELL_GRIDS:
        return dict(bin_cells=chunks, bin_aggregate_lds=naggs * chunks)
    if grid_name == "setord":
        return dict(bin_aggregate_lds=naggs * chunks)
    return dict(bin_indices=chunks, bin_aggregate=naggs * chunks)


_EXPECTED = {}


def _expected(g, vc, kind, moment, masked, label, col, rows=None, init=None):
    """The oracle's grids (and the exact float reference) of one aggregation, computed once."""
    key = (g.name, g.n, vc.dtype, kind, moment, masked, label, None if rows is None else (rows.start, rows.stop),
           None if init is None else init.tobytes())
    if key not in _EXPECTED:
        mask = vc.keep if masked else None
        exp, exp2 = arc.expected(g, kind, data=col, data2=vc.order if kind == "first" else None, mask=mask,
                                 moment=moment if moment is not None else 2, rows=rows, init=init)
        ref = None
        if kind in ("sum", "sum_moment") and col.dtype.kind == "f" and rows is None and init is None:
            ref = arc.float_sum_reference(g.idx, g.length, col, mask, moment if kind == "sum_moment" else None)
        _EXPECTED[key] = (exp, exp2, ref)
    return _EXPECTED[key]


def _compare(kind, out, g, exp, exp2, ref, what):
    got, got2 = out
    if kind == "first":
        arc.check_bits(got, exp, g, what + " value grid")
        arc.check_bits(got2, exp2, g, what + " order grid")
    elif ref is not None:
        assert got.dtype == np.float64 and got.shape == g.shape, what
        arc.check_float_sum(got, exp, ref, what)
    else:
        arc.check_exact(got, exp, g, what, bits_where_nonzero=kind in ("min", "max"))


_SWAPPED = {}


def _as(col, flip):
    """The column in the byte order the aggregator reads (1-byte dtypes have one order only:
    their _non_native classes still run the kernels' flip branch, over the same bytes)."""
    if not flip or col.dtype.itemsize == 1:
        return col
    if id(col) not in _SWAPPED:
        _SWAPPED[id(col)] = (arc.swapped(col), col)
    return _SWAPPED[id(col)][0]


def _sweep(grid_name, dtype, n=arc.N_MAIN, loc="device", offsets=None, kinds=KIND_LIST, flips=(False, True),
           chunks=1):
    """Every kind x byte order x {no mask, keep mask} of one dtype over one grid, one
    aggregator per bin (a fusable one beside its companion), route asserted, then compared."""
    g, vc = arc.grid_case(grid_name, n), arc.value_case(grid_name, dtype, n)
    cols = Columns(loc, offsets)
    ran = 0
    for kind, moment in kinds:
        for flip in flips:
            if kind == "sum_moment" and flip and np.dtype(dtype).itemsize < 8:
                assert arc.SWAPPED_MOMENT_NEEDS_8_BYTES  # garbage by design, superagg.cpp:415-417
                continue
            for masked in (False, True):
                if kind == "first" and masked:
                    assert arc.FIRST_TAKES_NO_MASK
                    continue
                for label, col in vc.variants(kind, moment):
                    what = f"{grid_name} n={n} {dtype} {kind}{'' if moment is None else moment} " \
                           f"{'swapped' if flip else 'native'} {'masked' if masked else 'unmasked'} {label} {loc}"
                    mask = vc.keep if masked else None
                    specs = [_spec(kind, _as(col, flip), mask, _as(vc.order, flip) if kind == "first" else None,
                                   moment, flip)]
                    if _fusable(kind, col, flip):
                        specs.append(_spec("max", vc.values, mask))
                    outs, counters, _ = _bin(g, specs, cols)
                    _assert_route(counters, what, **_route(grid_name, kind, len(specs), chunks))
                    exp, exp2, ref = _expected(g, vc, kind, moment, masked, label, col)
                    _compare(kind, outs[0], g, exp, exp2, ref, what)
                    ran += 1
    return ran


# ---- every dtype x kind x byte order x mask on every route ----------------------------------
@pytest.mark.parametrize("dtype", arc.DTYPES)
@pytest.mark.parametrize("grid_name", arc.GRIDS)
def test_route_every_kind(grid_name, dtype):
    """HBM columns, n = 20011: cells (small1, small2, zero_d), plan-index LDS (setord), global
    atomics (large); AggFirst on its LDS and index routes; swapped columns on every kernel
    that has a flip line; keep masks of bytes {0, 1, 2, 255}; integer moments 0-3."""
    ran = _sweep(grid_name, dtype)
    wide = np.dtype(dtype).itemsize == 8
    assert ran >= (4 * 4 + 4 * (4 if wide else 2) + 2), ran  # nothing skipped but the named exclusions


# ---- tails ----------------------------------------------------------------------------------
TAIL_KINDS = [("count", None), ("sum", None), ("min", None), ("max", None), ("sum_moment", 2), ("first", None)]


@pytest.mark.parametrize("dtype", ["int8", "int16", "int32", "float64", "bool"])
@pytest.mark.parametrize("n", arc.TAILS)
def test_tails(n, dtype):
    """Row counts around RU = 8 (the per-row tail of load_rows8) and around the 2048-row step of
    k_first_small, on the cells and first-LDS routes."""
    for grid_name in ("small1", "small2"):
        _sweep(grid_name, dtype, n=n, kinds=TAIL_KINDS, flips=(False,))


# ---- unaligned device pointers --------------------------------------------------------------
UNALIGNED = [{r: off} for r in ("binner", "bmask", "value", "order", "keep") for off in (1, 3)] + \
            [dict(binner=1, bmask=3, value=1, order=3, keep=1), dict(binner=3, bmask=1, value=3, order=1, keep=3)]
UNALIGNED_KINDS = [("count", None), ("sum", None), ("max", None), ("sum_moment", 2), ("first", None)]


@pytest.mark.parametrize("dtype", ["int8", "int16", "float32", "float64"])
@pytest.mark.parametrize("grid_name", ["small1", "small2"])
def test_unaligned_device_pointers(grid_name, dtype):
    """DeviceArray slices [1:] and [3:] of the binner column, the value column, the order
    column, the keep mask and the binner mask, one at a time and all together: the per-row
    fallback of load_rows8 in k_cells_dim, k_agg_lds_c and k_first_small's plain loads."""
    for offsets in UNALIGNED:
        _sweep(grid_name, dtype, offsets=offsets, kinds=UNALIGNED_KINDS, flips=(False,))


# ---- host columns ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint8", "int16", "float32"])
@pytest.mark.parametrize("grid_name", ["small1", "large"])
def test_host_columns(grid_name, dtype):
    """The stager with narrow itemsizes: host columns on the cells and global routes."""
    _sweep(grid_name, dtype, loc="host", flips=(False,))


def test_host_two_chunks_narrow_partials_flush_twice():
    """2**24 + 9 host rows of int16 on small1: two stager chunks, so the 32-bit LDS partials of
    the NARROW sum (and the min / max cells) flush twice into one grid."""
    tc = arc.two_chunk_case()
    g = tc.grid
    cols = Columns("host")
    for kind in ("sum", "min", "max"):
        for mask in (None, tc.keep):
            what = f"two chunks int16 {kind} {'unmasked' if mask is None else 'masked'}"
            outs, counters, _ = _bin(g, [_spec(kind, tc.values, mask)], cols)
            _assert_route(counters, what, bin_cells=2, bin_aggregate_lds=2)
            exp, _ = arc.expected(g, kind, data=tc.values, mask=mask)
            arc.check_exact(outs[0][0], exp, g, what)


# ---- the fused passes -----------------------------------------------------------------------
def _eight(grid_name, flip, all_masked):
    """count(*), count(int32), count(float32 with NaN), sum(int8), sum(uint16), sum(int32),
    sum(float32), masked sum(float64) -- as (spec, value case, kind, column)."""
    vcs = {d: arc.value_case(grid_name, d) for d in ("int32", "float32", "int8", "uint16", "float64")}
    out = []
    for kind, d in (("count", None), ("count", "int32"), ("count", "float32"), ("sum", "int8"), ("sum", "uint16"),
                    ("sum", "int32"), ("sum", "float32"), ("sum", "float64")):
        vc = vcs[d or "int32"]
        col = None if d is None else vc.column(kind)
        masked = all_masked or d == "float64"
        out.append((_spec(kind, None if col is None else _as(col, flip), vc.keep if masked else None,
                          flip=flip and d is not None, dtype="int64"), vc, kind, col, masked))
    return out


def _check_fused(g, items, outs, what):
    for (spec, vc, kind, col, masked), out in zip(items, outs):
        w = f"{what} {kind}({'*' if col is None else vc.dtype})"
        if col is None:
            exp, _ = arc.expected(g, "count", mask=vc.keep if masked else None)
            arc.check_exact(out[0], exp, g, w)
        else:
            exp, exp2, ref = _expected(g, vc, kind, None, masked, "full", col)
            _compare(kind, out, g, exp, exp2, ref, w)


@pytest.mark.parametrize("variant", ["native", "swapped_all_masked"])
@pytest.mark.parametrize("grid_name", ["small1", "small2"])
def test_fused_small(grid_name, variant):
    """k_small_fused: eight count / sum aggregators in one bin.  On small1 all eight sub-grids
    fit one launch; on small2 a wide sub-grid is 18 952 B, so the 48 KiB budget splits them:
    {count(*), count(int32) sharing it, count(float32), sum(int8), sum(uint16)} (narrow cells),
    {sum(int32), sum(float32)}, and the float64 sum alone through k_agg_lds_c -- three launches.
    Swapped and all masked, nothing is shared and the 8/16-bit sums have wide cells, which moves
    the split ({three counts, sum(int8)}, {sum(uint16), sum(int32)}, {sum(float32),
    sum(float64)}) but not the number of launches."""
    g = arc.grid_case(grid_name)
    flip = variant != "native"
    items = _eight(grid_name, flip, flip)
    outs, counters, _ = _bin(g, [it[0] for it in items])
    if grid_name == "small1":
        _assert_route(counters, variant, bin_cells=1, bin_aggregate_lds=1)
    else:
        _assert_route(counters, variant, bin_cells=1, bin_aggregate_lds=(">=", 2))
        assert counters["bin_aggregate_lds"] == 3, counters
    _check_fused(g, items, outs, f"fused small {grid_name} {variant}")


@pytest.mark.parametrize("offsets", UNALIGNED, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_fused_small_unaligned(offsets):
    """sf_rows' per-row loads: the eight aggregators over columns at [1:] / [3:]."""
    g = arc.grid_case("small1")
    items = _eight("small1", False, True)
    outs, counters, _ = _bin(g, [it[0] for it in items], Columns("device", offsets))
    _assert_route(counters, str(offsets), bin_cells=1, bin_aggregate_lds=1)
    _check_fused(g, items, outs, f"fused small unaligned {offsets}")


@pytest.mark.parametrize("grid_name", ["small2", "setord", "large"])
def test_fused_float64_over_a_generic_plan(grid_name):
    """count(*) + masked count(float64) + sum(float64): k_fused<true, 0> on small grids whose
    binners are not float64 scalars, k_fused<false, 0> (global atomics) on the large one."""
    g, vc = arc.grid_case(grid_name), arc.value_case(grid_name, "float64")
    specs = [_spec("count", dtype="int64"), _spec("count", vc.values, vc.keep), _spec("sum", vc.sums)]
    outs, counters, _ = _bin(g, specs)
    _assert_route(counters, grid_name, **({"bin_fused_global": 1} if grid_name == "large" else {"bin_fused_lds": 1}))
    arc.check_exact(outs[0][0], arc.expected(g, "count")[0], g, "count(*)")
    arc.check_exact(outs[1][0], _expected(g, vc, "count", None, True, "full", vc.values)[0], g, "masked count(float64)")
    exp, exp2, ref = _expected(g, vc, "sum", None, False, "full", vc.sums)
    _compare("sum", outs[2], g, exp, exp2, ref, "sum(float64)")


# ---- reduce ---------------------------------------------------------------------------------
REDUCE_KINDS = [("count", None), ("sum", None), ("min", None), ("max", None), ("sum_moment", 2), ("sum_moment", 3),
                ("first", None)]


@pytest.mark.parametrize("dtype", arc.DTYPES)
def test_reduce_parts(dtype):
    """vh_agg_reduce for every dtype and kind: small1 in three row ranges (cut off the 8-row
    grid, so the parts read unaligned slices), each into its own aggregator, then
    parts[0].reduce(parts[1:]) against the oracle over the whole column; AggFirst compares the
    order grid too, and its ties go to the earlier part."""
    g, vc = arc.grid_case("small1"), arc.value_case("small1", dtype)
    cuts = [slice(0, 6667), slice(6667, 13339), slice(13339, g.n)]
    cols = Columns()
    for kind, moment in REDUCE_KINDS:
        for masked in ((False,) if kind == "first" else (False, True)):
            col = vc.column(kind, moment)
            what = f"reduce {dtype} {kind}{'' if moment is None else moment} {'masked' if masked else 'unmasked'}"
            keep = []  # the grids and aggregators of all parts stay alive until the reduce
            parts = []
            for rows in cuts:
                spec = _spec(kind, col, vc.keep if masked else None, vc.order if kind == "first" else None, moment)
                extra = [_spec("max", vc.values, spec["mask"])] if _fusable(kind, col, False) else []
                outs, counters, aggs = _bin(g, [spec] + extra, cols, rows=rows)
                _assert_route(counters, what, **_route("small1", kind, 1 + len(extra)))
                keep.append(aggs)
                parts.append(aggs[0])
            parts[0].reduce(parts[1:])
            out = (np.asarray(parts[0]).copy(), parts[0].order_grid() if kind == "first" else None)
            exp, exp2, ref = _expected(g, vc, kind, moment, masked, "full", col)
            _compare(kind, out, g, exp, exp2, ref, what)


# ---- a pre-filled grid ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int8", "float32"])
@pytest.mark.parametrize("grid_name", ["small1", "large"])
def test_prefilled_grid(grid_name, dtype):
    """Values written into the live view before the bin: min / max / sum / first fold into
    them.  Every cell gets a middling value; for min / max one occupied cell holds the LDS fill
    value itself (iinfo.min / -inf for max, iinfo.max / +inf for min -- where a workgroup skips
    the flush of an LDS cell that still equals the fill, the grid's cell must survive) and
    another the opposite extreme, which no row can move."""
    g, vc = arc.grid_case(grid_name), arc.value_case(grid_name, dtype)
    dt = np.dtype(dtype)
    lo, hi = (-np.inf, np.inf) if dt.kind == "f" else (np.iinfo(dt).min, np.iinfo(dt).max)
    occupied = np.unique(g.idx[vc.keep == 1])
    cols = Columns()
    for kind in ("min", "max", "sum", "first"):
        for masked in ((False,) if kind == "first" else (False, True)):
            col = vc.column(kind)
            gdt = arc.expected(g, kind, data=col[:1], data2=vc.order[:1], rows=slice(0, 1))[0].dtype
            init = np.full(g.length, 5, dtype=gdt)
            if kind in ("min", "max"):
                init[occupied[0]] = lo if kind == "max" else hi   # the LDS fill value
                init[occupied[1]] = hi if kind == "max" else lo   # cannot move
            what = f"prefilled {grid_name} {dtype} {kind} {'masked' if masked else 'unmasked'}"
            spec = _spec(kind, col, vc.keep if masked else None, vc.order if kind == "first" else None, prefill=init)
            outs, counters, _ = _bin(g, [spec], cols)
            _assert_route(counters, what, **_route(grid_name, kind))
            exp, exp2, _ = _expected(g, vc, kind, None, masked, "full", col, init=init)
            if kind == "sum" and dt.kind == "f":
                # the pre-filled 5 is one more addend of every cell: the same bound with m + 1
                ref = arc.float_sum_reference(g.idx, g.length, col, vc.keep if masked else None)
                ref.exact, ref.count, ref.abssum = ref.exact + 5, ref.count + 1, ref.abssum + 5
                arc.check_float_sum(outs[0][0], exp, ref, what)
            else:
                _compare(kind, outs[0], g, exp, exp2, None, what)
