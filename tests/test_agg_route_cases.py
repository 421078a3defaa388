"""The cases of tests/agg_route_cases.py, checked on the CPU: the reference alone satisfies
every condition tests/test_gpu_agg_routes.py relies on, so a vacuous or ill-defined case fails
here, before it reaches a GPU."""
import numpy as np
import pytest

import agg_route_cases as arc
from oracle import oracle

INT_DTYPES = [d for d in arc.DTYPES if np.dtype(d).kind in "iub"]
FLOAT_DTYPES = ["float64", "float32"]
CASES = [(g, d) for g in arc.GRIDS for d in arc.DTYPES]
ids = lambda cases: ["-".join(map(str, c)) for c in cases]


def _py_sums(idx, length, values, keep=None):
    """Per-cell totals with Python ints (no overflow, no rounding)."""
    tot = np.zeros(length, dtype=object)
    rows = np.arange(len(idx)) if keep is None else np.flatnonzero(keep == 1)
    np.add.at(tot, idx[rows], arc.native(values)[rows].astype(object))
    return tot


def _upcast_info(dtype):
    return np.iinfo(oracle.UPCAST[dtype])


@pytest.mark.parametrize("grid,dtype", [c for c in CASES if c[1] in INT_DTYPES], ids=ids([c for c in CASES if c[1] in INT_DTYPES]))
def test_integer_sums_fit_and_match_python_ints(grid, dtype):
    """Exact per-cell sums (Python ints) fit int64 / uint64 -- no signed-overflow UB in the C
    oracle -- with and without the keep mask, and the oracle equals them."""
    g, vc = arc.grid_case(grid), arc.value_case(grid, dtype)
    info = _upcast_info(dtype)
    for keep in (None, vc.keep):
        tot = _py_sums(g.idx, g.length, vc.sums.astype(np.int64) if dtype == "bool" else vc.sums, keep)
        assert all(info.min <= t <= info.max for t in tot.tolist())
        for col in (vc.sums, arc.swapped(vc.sums)):
            got, _ = arc.expected(g, "sum", data=col, mask=keep)
            assert got.tolist() == tot.tolist()


@pytest.mark.parametrize("grid,dtype", [c for c in CASES if c[1] in INT_DTYPES], ids=ids([c for c in CASES if c[1] in INT_DTYPES]))
def test_integer_moments_are_bounded_and_exact(grid, dtype):
    """|v| <= 2**20 (moments 0-2) / 2**10 (moments 3, 4); every cell's exact total of |v|**m
    stays below 2**53, so the reference's detour through double is exact and order-free: the
    oracle grid equals the Python-int total."""
    g, vc = arc.grid_case(grid), arc.value_case(grid, dtype)
    for moment in (0, 1, 2, 3, 4):
        col = vc.moment_column(moment)
        v = arc.native(col).astype(object)
        assert max(abs(x) for x in v.tolist()) <= arc.MOMENT_BOUND[moment]
        for keep in (None, vc.keep):
            mag = _py_sums(g.idx, g.length, np.array([abs(int(x)) ** moment for x in v.tolist()], dtype=object), keep)
            assert max(mag.tolist()) < 2 ** 53
            tot = _py_sums(g.idx, g.length, np.array([int(x) ** moment for x in v.tolist()], dtype=object), keep)
            cols = [col] + ([arc.swapped(col)] if col.dtype.itemsize == 8 else [])  # SWAPPED_MOMENT_NEEDS_8_BYTES
            for c in cols:
                got, _ = arc.expected(g, "sum_moment", data=c, mask=keep, moment=moment)
                assert got.tolist() == tot.tolist(), (moment, c.dtype)


@pytest.mark.parametrize("grid,dtype", [c for c in CASES if c[1] in FLOAT_DTYPES], ids=ids([c for c in CASES if c[1] in FLOAT_DTYPES]))
def test_float_sums_cannot_overflow_and_the_oracle_meets_the_bound(grid, dtype):
    """The finite addends of every cell satisfy sum|v| < 1e300 (sums and moments 0-3), so no
    finite sum overflows and a cell with +-inf is order-independent; the oracle's own serial
    sum passes the comparison the GPU is held to, and a grid off by more than the bound fails."""
    g, vc = arc.grid_case(grid), arc.value_case(grid, dtype)
    assert arc.SUMS_LEAVE_OUT_F64_MAX and arc.SUMS_LEAVE_OUT_F64_SUBNORMALS
    if dtype == "float64":
        fin = vc.sums[np.isfinite(vc.sums)]
        assert np.abs(fin).max() < 1e3 and not ((fin != 0) & (np.abs(fin) < np.finfo(np.float64).tiny)).any()
    else:
        assert vc.sums is vc.values  # float32 keeps its subnormals and its max
    for keep in (None, vc.keep):
        for moment in (None, 0, 1, 2, 3):
            kind = "sum" if moment is None else "sum_moment"
            seen_nonfinite = seen_finite = False
            for label, col in vc.variants(kind, moment):
                ref = arc.float_sum_reference(g.idx, g.length, col, keep, moment)
                assert ref.abssum.max() < 1e300
                got, _ = arc.expected(g, kind, data=col, mask=keep, moment=moment or 0)
                arc.check_float_sum(arc.shaped(g, got), got, ref, f"{moment} {label}")
                seen_nonfinite |= bool(ref.nonfinite.any())
                contended = np.flatnonzero(~ref.nonfinite & (ref.count >= 2))
                if len(contended):
                    seen_finite = True
                    c = int(contended[0])
                    off = got.copy()
                    off[c] += 4 * ref.bound()[c] + np.spacing(off[c]) * 4
                    with pytest.raises(AssertionError):
                        arc.check_float_sum(arc.shaped(g, off), got, ref)
            assert (seen_nonfinite or moment == 0) and seen_finite  # (inf ** 0 is 1); both rules of the comparison have cells to bite on


def _bits(a):
    a = np.ascontiguousarray(arc.native(a))
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize("grid,dtype", CASES, ids=ids(CASES))
def test_coverage(grid, dtype):
    g, vc = arc.grid_case(grid), arc.value_case(grid, dtype)
    kept = vc.keep == 1
    # the NaN / masked, underflow and overflow cells of every binner receive rows
    for d, edges in enumerate(g.edge_cells):
        present = set(np.unique(g.dim_index(d)).tolist())
        assert set(edges) <= present, (d, edges)
    # contended cells
    _, counts = np.unique(g.idx[kept], return_counts=True)
    assert (counts >= 2).mean() >= 0.25
    # the keep mask
    assert 0.4 <= kept.mean() <= 0.8
    assert (vc.keep == 2).any() and (vc.keep == 255).any() and (vc.keep == 0).any()
    # every special in a kept row, bit for bit (-0.0 is not 0.0 here)
    for col, for_sum in ((vc.values, False), (vc.sums, True)):
        want = list(arc.palette(dtype, for_sum))
        dt = np.dtype(dtype)
        if dt.kind in "iu" and dt.itemsize == 8:
            info = np.iinfo(dt)
            if dt.kind == "i":
                want += [info.min, info.max]
            else:
                want += [arc.U64_HIGH] + ([info.max] if g.length > 1 else [])  # U64_MAX_NEEDS_ITS_OWN_CELL
        have = set(_bits(col[kept]).tolist())
        for s in want:
            assert int(_bits(np.array([s], dtype=dt))[0]) in have, s
    # AggFirst: ties at the minimum order of at least a quarter of the occupied cells
    v, o = vc.values, vc.order
    ok = np.ones(g.n, bool) if np.dtype(dtype).kind != "f" else ~(np.isnan(v) | np.isnan(o))
    cells = g.idx[ok]
    lo = np.full(g.length, o[ok].max(), dtype=o.dtype)
    np.minimum.at(lo, cells, o[ok])
    ties = np.bincount(cells[o[ok] == lo[cells]], minlength=g.length)
    occupied = np.bincount(cells, minlength=g.length) > 0
    assert (ties[occupied] >= 2).mean() >= 0.25
    if np.dtype(dtype).kind != "b":
        top = np.finfo(dtype).max if np.dtype(dtype).kind == "f" else np.iinfo(dtype).max
        assert (o == top).any()  # never taken: the comparison is a strict <
    if np.dtype(dtype).kind == "f":
        assert np.isnan(o).any() and (_bits(o) == _bits(np.array([-0.0], dtype))[0]).any() and \
            (_bits(o) == 0).any()


@pytest.mark.parametrize("grid,dtype", CASES, ids=ids(CASES))
def test_oracle_agrees_with_numpy(grid, dtype):
    """Counts, integer sums, min and max of the oracle against a NumPy restatement (np.add.at,
    np.minimum.at, boolean indexing), native and byte-swapped columns."""
    g, vc = arc.grid_case(grid), arc.value_case(grid, dtype)
    dt = np.dtype(dtype)
    v = vc.values
    notnan = ~np.isnan(v) if dt.kind == "f" else np.ones(g.n, bool)
    for keep in (None, vc.keep):
        rows = notnan if keep is None else notnan & (keep == 1)
        for col in (v, arc.swapped(v)):
            got, _ = arc.expected(g, "count", data=col, mask=keep)
            np.testing.assert_array_equal(got, np.bincount(g.idx[rows], minlength=g.length))
            for kind, fn in (("min", np.minimum), ("max", np.maximum)):
                ref, _ = oracle.new_grid(kind, dtype, g.shape)
                fn.at(ref, g.idx[rows], v[rows])
                got, _ = arc.expected(g, kind, data=col, mask=keep)
                np.testing.assert_array_equal(got, ref)
            if dt.kind in "iub":
                ref = np.zeros(g.length, oracle.UPCAST[dtype])
                np.add.at(ref, g.idx[rows], vc.sums[rows].astype(ref.dtype))
                got, _ = arc.expected(g, "sum", data=arc.swapped(vc.sums) if col is not v else vc.sums, mask=keep)
                np.testing.assert_array_equal(got, ref)
    if keep is not None:  # count(*) under a mask
        got, _ = arc.expected(g, "count", mask=vc.keep)
        np.testing.assert_array_equal(got, np.bincount(g.idx[vc.keep == 1], minlength=g.length))


@pytest.mark.parametrize("n", arc.TAILS)
def test_tail_cases_build(n):
    """The tail sizes build for the dtypes the GPU tests run them with, deterministically."""
    for grid in ("small1", "small2"):
        g = arc.grid_case(grid, n)
        assert g.n == n and len(g.idx) == n
        for dtype in ("int8", "int16", "int32", "float64", "bool"):
            vc = arc.value_case(grid, dtype, n)
            again = arc.ValueCase(g, dtype)
            assert _bits(vc.values).tolist() == _bits(again.values).tolist() and len(vc.order) == n


def test_set_ordinals_cover_members_and_strangers():
    b = arc.grid_case("setord").binners[0]
    assert len(np.unique(b["set_keys"])) == arc.SET_KEYS
    assert set(np.unique(b["ordinals"]).tolist()) == set(range(-1, arc.SET_KEYS))


def test_grid_sizes_select_the_routes():
    """The cell counts the routes are selected by: LDS_AGG_MAX_BYTES = 96 KiB of 8-byte cells,
    SF_LDS_BUDGET = 48 KiB (two wide small2 sub-grids of 18 952 B fit one launch, three do not)."""
    L = {name: arc.grid_case(name).length for name in arc.GRIDS}
    assert L == {"small1": 35, "small2": 103 * 23, "setord": 53, "large": 20003, "zero_d": 1}
    assert L["large"] * 8 > 96 * 1024 >= L["small2"] * 8
    assert 2 * L["small2"] * 8 <= 48 * 1024 < 3 * L["small2"] * 8
