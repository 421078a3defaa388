"""Masked HBM columns (DeviceMaskedArray) on the GPU: the column type and its Arrow bitmap kernels,
the expression layer against the rule (tests/missing_np.py), and the frame plumbing against the
same call on the host frame holding the same ``np.ma`` columns.

N = 2051: more than one 2048-row block of the 8-rows-per-lane kernels and one interpreter block,
ragged; every evaluate also runs once from row 1, the misaligned path.  The data under a missing
row is unspecified and never looked at."""
import numpy as np
import pytest

import expr_np
import missing_np
import vaex_amd
from vaex_amd import DeviceArray, DeviceMaskedArray

pytestmark = pytest.mark.gpu

N = missing_np.N


def _device(columns):
    return vaex_amd.from_arrays(**{k: (DeviceMaskedArray.from_numpy(v) if np.ma.isMaskedArray(v) else DeviceArray.from_numpy(v))
                                   for k, v in columns.items()})


def _parts(v):
    if isinstance(v, DeviceMaskedArray):
        return v.data.to_numpy(), v.mask.to_numpy().astype(bool)
    assert isinstance(v, DeviceArray), type(v)
    return v.to_numpy(), None


_FRAMES = {}


def _frames(kind="mixed"):
    """(columns, host frame, device frame) of the small columns plus two integer keys, built once"""
    if kind not in _FRAMES:
        rng = np.random.default_rng(11)
        cols = dict(missing_np.small_columns(kind))
        cols["k"] = np.ma.array(rng.integers(0, 9, N).astype(np.int32) * 1000 - 3000, mask=missing_np.mask_of(kind, N, 5),
                                shrink=False)
        cols["k2"] = rng.integers(0, 4, N).astype(np.int64)
        cols["y"] = np.ma.array(rng.normal(size=N), mask=missing_np.mask_of(kind, N, 6), shrink=False)
        cols["o"] = rng.permutation(N).astype(np.int64)
        for v in cols.values():
            v.setflags(write=False)
        _FRAMES[kind] = (cols, vaex_amd.from_arrays(**cols), _device(cols))
    return _FRAMES[kind]


# ---- the column type -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", missing_np.MASK_KINDS)
def test_numpy_round_trip(kind):
    cols = missing_np.small_columns(kind)
    for name in ("a", "x", "p"):
        d = DeviceMaskedArray.from_numpy(cols[name])
        back = d.to_numpy()
        m = np.ma.getmaskarray(cols[name])
        assert np.ma.isMaskedArray(back) and back.mask.shape == (N,) and back.dtype == cols[name].dtype
        assert np.array_equal(back.mask, m) and np.array_equal(back.data[~m], cols[name].data[~m], equal_nan=name == "x")
        assert d.null_count == int(m.sum()) and d[1:].null_count == int(m[1:].sum())
        assert len(d) == N and d.dtype == cols[name].dtype and d.nbytes == N * (d.dtype.itemsize + 1)
        assert np.array_equal(d[5:77].to_numpy().mask, m[5:77])
    plain = DeviceMaskedArray.from_numpy(np.ma.array(np.arange(9.0)))  # nomask: all zeros
    assert plain.null_count == 0 and plain.to_numpy().mask.shape == (9,)
    assert DeviceMaskedArray.from_numpy(np.arange(3)).null_count == 0


@pytest.mark.parametrize("offset", [0, 1, 7, 8, 9])
@pytest.mark.parametrize("dtype", ["float64", "int32", "uint8", "bool"])
def test_arrow_round_trip(offset, dtype):
    pa = pytest.importorskip("pyarrow")
    rng = np.random.default_rng(offset)
    n = N + offset
    values = (rng.random(n) < 0.5) if dtype == "bool" else rng.integers(0, 100, n).astype(dtype)
    null = missing_np.mask_of("mixed", n, 1)
    for nulls in (null, np.zeros(n, bool), np.ones(n, bool), None):
        ar = pa.array(values, mask=nulls)[offset:]
        assert ar.offset == offset
        d = DeviceMaskedArray.from_arrow(ar)
        assert len(d) == N and d.dtype == values.dtype
        want = np.asarray(ar.is_null())
        assert np.array_equal(d.mask.to_numpy().astype(bool), want)  # bit-exact validity
        assert d.null_count == ar.null_count
        assert np.array_equal(d.data.to_numpy()[~want], values[offset:][~want])
        back = d.to_arrow()
        assert back.type == ar.type and back.null_count == ar.null_count
        assert np.array_equal(np.asarray(back.is_null()), want) and back.equals(ar)
        # the packed bitmap: the padding bits of the last byte are 0
        bitmap = np.frombuffer(back.buffers()[0], np.uint8)[:(N + 7) // 8]
        assert np.array_equal(np.unpackbits(bitmap, bitorder="little")[:N], ~want)
        assert bitmap[-1] >> (N % 8) == 0


def test_arrow_short_and_misaligned_lengths():
    pa = pytest.importorskip("pyarrow")
    for n in (0, 1, 7, 8, 9, 63, 64, 65):
        nulls = missing_np.mask_of("mixed", n + 3, 2)
        ar = pa.array(np.arange(n + 3, dtype=np.int64), mask=nulls)[3:]
        d = DeviceMaskedArray.from_arrow(ar)
        assert np.array_equal(d.mask.to_numpy().astype(bool), nulls[3:]) and d.to_arrow().equals(ar)
        assert d[1:].to_arrow().equals(ar[1:])  # a mask that starts off an 8-byte boundary


# ---- expressions ------------------------------------------------------------------------------
EXPRESSIONS = missing_np.OPERATORS + missing_np.WHERES + missing_np.FUNCTIONS + missing_np.CONSTANTS


def _check_evaluate(df, e, columns, ulp=None):
    got = df.evaluate(e)
    data, mask = _parts(got)
    missing_np.check(e, data, mask, columns, ulp=ulp)
    tail = {k: v[1:] for k, v in columns.items()}  # from row 1: every input off its 8-row alignment
    data1, mask1 = _parts(df.evaluate(e, 1, N))
    missing_np.check(e, data1, mask1, tail, ulp=ulp)


@pytest.mark.parametrize("kind", missing_np.MASK_KINDS)
def test_expressions_follow_the_rule(kind):
    columns, _, df = _frames(kind)
    for e in EXPRESSIONS:
        _check_evaluate(df, e, columns, ulp=4 if "sqrt" in e else None)


@pytest.mark.parametrize("kind", missing_np.MASK_KINDS)
def test_every_dtype(kind):
    columns = dict(missing_np.edge_columns(kind))
    df = _device(columns)
    for first, other in expr_np._SECOND.items():
        dt = np.ma.getdata(columns[first]).dtype
        exprs = [f"{first} == {other}", f"where({first} == {other}, {first}, {other})", f"ismissing({first})",
                 f"notmissing({first})", f"fillmissing({first}, 1)", f"isna({first})", f"notna({first})",
                 f"isnan({first})", f"fillnan({first}, 1)", f"fillna({first}, 1)"]
        exprs += [f"{first} & {other}", f"~{first}"] if dt.kind == "b" else [f"{first} + {other}", f"minimum({first}, {other})"]
        for e in exprs:
            _check_evaluate(df, e, columns)


FILL_COLUMNS = ["x", "f", "i", "i32", "u64", "u32", "i16", "u8", "b"]  # the last three: narrow items, the interpreter


@pytest.mark.parametrize("kind", missing_np.MASK_KINDS)
def test_fused_fill_kernel_on_and_off(kind, monkeypatch):
    """fillmissing(column, constant) runs a kernel of its own for 4- and 8-byte items;
    VH_EXPR_FILL=0 (read per call) sends the shape to the interpreter.  Bit-identical to each other
    and to the rule, from row 0 and from row 1 (data, mask and destination off their alignment)."""
    columns = dict(missing_np.edge_columns(kind))
    df = _device(columns)
    for name in FILL_COLUMNS:
        for value in ("1", "0"):
            e = f"fillmissing({name}, {value})"
            results = {}
            for switch in ("1", "0"):
                monkeypatch.setenv("VH_EXPR_FILL", switch)
                for i1 in (0, 1):
                    got = df.evaluate(e, i1, N)
                    assert isinstance(got, DeviceArray), e
                    results[switch, i1] = got.to_numpy()
                    missing_np.check(e, results[switch, i1], None, {k: v[i1:] for k, v in columns.items()})
            for i1 in (0, 1):
                a, b = results["1", i1], results["0", i1]
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (e, i1)
    monkeypatch.delenv("VH_EXPR_FILL")
    small, _, sdf = _frames(kind)
    for e in ("fillmissing(x, 1.5)", "fillmissing(a, 7)", "fillmissing(b, -3)"):
        missing_np.check(e, sdf.evaluate(e).to_numpy(), None, small)


def test_expression_api_and_to_numpy():
    columns, host, df = _frames()
    got = (df.a + df.u).to_numpy()
    want = host.evaluate("a + u")
    assert np.ma.isMaskedArray(got) and np.array_equal(got.mask, np.ma.getmaskarray(want))
    assert np.array_equal(got.data[~got.mask], want.data[~got.mask])
    assert np.array_equal(df.x.fillna(-1.0).to_numpy(), host.evaluate("fillna(x, -1.0)"))
    assert np.array_equal(df.a.ismissing().to_numpy(), np.ma.getmaskarray(columns["a"]))
    assert np.array_equal(df.x.isna().to_numpy(), host.evaluate("isna(x)"))
    df2 = df.copy()
    df2.add_variable("fill", 5)
    assert np.array_equal(df2.evaluate("fillmissing(a, fill)").to_numpy(), host.evaluate("fillmissing(a, 5)"))
    with pytest.raises(NotImplementedError, match="cannot hold"):
        df.evaluate("fillmissing(a, 1.5)")


# ---- booleans as row masks ---------------------------------------------------------------------
FILTERS = ["x > 50", "(x > 30) & (a <= 60)", "p", "~p", "p | q", "(a < b) | (u > 50)",
           "(x > 30) & (u <= 60) & (b != 7)"]


@pytest.mark.parametrize("e", FILTERS)
def test_keep_mask_is_data_and_not_mask(e):
    columns, host, df = _frames()
    data, mask = missing_np.evaluate(e, columns)
    want = data & ~mask
    assert np.array_equal(df.filter(e).evaluate_filter_mask(0, N).to_numpy().astype(bool), want)
    assert np.array_equal(df.filter(e).evaluate_filter_mask(1, N).to_numpy().astype(bool), want[1:])
    assert len(df.filter(e)) == int(want.sum()) == len(host.filter(e))
    assert int(df.count(selection=e)) == int(want.sum()) == int(host.count(selection=e))
    df2 = df.copy()
    df2.select(e)
    df2.select("u < 70", mode="and")
    assert df2.selected_length() == int((want & (columns["u"] < 70)).sum())
    df2.select_inverse()
    h2 = host.copy()
    h2.select(e)
    h2.select("u < 70", mode="and")
    h2.select_inverse()
    assert df2.selected_length() == h2.selected_length()
    # the skip mask of the min / max pre-pass is the complement of the keep mask
    skip = df.device_keep_mask(0, N, e, invert=True).to_numpy().astype(bool)
    assert np.array_equal(skip, ~want)


# ---- aggregations against the host frame ------------------------------------------------------
def _same(got, want, exact):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if exact:
        assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f")
    else:
        assert np.allclose(got, want, rtol=1e-6, atol=0, equal_nan=True)


AGGS = [("count", True), ("sum", False), ("mean", False), ("var", False), ("min", True), ("max", True)]
GRIDS = [dict(), dict(binby="u", limits=[0, 100], shape=128), dict(binby=["u", "o"], limits=[[0, 100], [0, N]], shape=(16, 16)),
         dict(binby="y", limits=[-2, 2], shape=128),          # the binby expression itself masked: the null bin
         dict(binby=["y", "b"], limits=[[-2, 2], [0, 100]], shape=(16, 16))]


@pytest.mark.parametrize("grid", range(len(GRIDS)))
@pytest.mark.parametrize("kind", ["mixed", "missing"])
def test_aggregations_match_the_host_frame(grid, kind):
    _, host, df = _frames(kind)
    kw = GRIDS[grid]
    for value in ("x", "a", "x + a"):
        for name, exact in AGGS:
            for extra in (dict(), dict(selection="q"), dict(selection="(u > 20) & (b < 80)")):
                got = getattr(df, name)(value, **kw, **extra)
                want = getattr(host, name)(value, **kw, **extra)
                _same(got, want, exact or (name == "sum" and value == "a"))
    _same(df.count(**kw), host.count(**kw), True)  # count() with no expression counts every row
    edges = dict(kw, edges=True) if kw else kw
    _same(df.count("x", **edges), host.count("x", **edges), True)


@pytest.mark.parametrize("grid", [0, 1, 3])
def test_filtered_and_selected_aggregations(grid):
    _, host, df = _frames()
    kw = GRIDS[grid]
    hf, dfl = host.filter("(u > 10) & (y < 1)"), df.filter("(u > 10) & (y < 1)")
    for value in ("x", "a"):
        for name, exact in AGGS:
            _same(getattr(dfl, name)(value, selection="p", **kw), getattr(hf, name)(value, selection="p", **kw),
                  exact or (name == "sum" and value == "a"))
    _same(dfl.count(**kw), hf.count(**kw), True)
    _same(dfl.count(selection=["p", "x > 50"], **kw), hf.count(selection=["p", "x > 50"], **kw), True)


def test_minmax_first_nunique():
    columns, host, df = _frames()
    for value in ("x", "a", "y"):
        _same(df.minmax(value), host.minmax(value), True)
        _same(df.minmax(value, selection="q"), host.minmax(value, selection="q"), True)
        _same(df.filter("u > 30").minmax(value), host.filter("u > 30").minmax(value), True)
    _same(df.minmax("a", binby="u", limits=[0, 100], shape=16), host.minmax("a", binby="u", limits=[0, 100], shape=16), True)
    # a filter plus a selection together
    hf, dfl = host.filter("(u > 10) & (y < 1)"), df.filter("(u > 10) & (y < 1)")
    for value in ("x", "a"):
        _same(dfl.minmax(value, selection="q"), hf.minmax(value, selection="q"), True)
    # first: the aggregator takes no masks, so a masked value or order is refused; the rows
    # without a missing value, extracted, answer (the value at the lowest order among them)
    for call in (lambda: df.first("x", "o"), lambda: df.first("u", "b"),
                 lambda: dfl.first("x", "o", selection="p", binby="u", limits=[0, 100], shape=16)):
        with pytest.raises(NotImplementedError, match="first over the masked expression"):
            call()
    x, o = columns["x"], columns["o"]
    rows = np.flatnonzero(~np.ma.getmaskarray(x) & ~np.isnan(x.data))
    got = df.dropna(["x"]).extract().first("fillmissing(x, 0.0)", "o")
    assert float(got) == x.data[rows[np.argmin(o[rows])]]
    # a lasso selection (not an expression: its mask and the valid rows are and-ed on the device)
    xs, ys = [10.0, 90.0, 90.0, 10.0], [100.0, 100.0, 1800.0, 1800.0]
    hl, dl = host.copy(), df.copy()
    for frame in (hl, dl):
        frame.select_lasso("u * 1.0", "o * 1.0", xs, ys)  # the lasso takes float coordinates
    assert 0 < dl.selected_length() == hl.selected_length() < N
    for value in ("x", "a"):
        _same(dl.minmax(value, selection=True), hl.minmax(value, selection=True), True)
        _same(dl.sum(value, selection=True), hl.sum(value, selection=True), value == "a")
    for kw in GRIDS[:4]:
        for extra in (dict(), dict(selection="q")):
            _same(df._compute_agg("nunique", "a", **kw, **extra), host._compute_agg("nunique", "a", **kw, **extra), True)
        # under a filter: with a selection as on the host frame; without one the engine cannot tell a
        # missing value the filter keeps from a row it drops, so that is refused, and the extracted
        # frame answers as the host frame does
        _same(df.filter("u > 30")._compute_agg("nunique", "k", selection="q", **kw),
              host.filter("u > 30")._compute_agg("nunique", "k", selection="q", **kw), True)
        with pytest.raises(NotImplementedError, match="'k'"):
            df.filter("u > 30")._compute_agg("nunique", "k", **kw)
        _same(df.filter("u > 30").extract()._compute_agg("nunique", "k", **kw),
              host.filter("u > 30")._compute_agg("nunique", "k", **kw), True)
    assert df.limits("x", "minmax") == host.limits("x", "minmax")


# ---- sets and counters ------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [dict(), dict(dropmissing=True), dict(dropna=True), dict(dropnan=True)])
def test_value_counts_unique_nunique(drop):
    _, host, df = _frames()
    for name in ("k", "a", "x"):
        got, want = df.value_counts(name, **drop), host.value_counts(name, **drop)
        assert list(got.index.map(str)) == list(want.index.map(str)) and got.tolist() == want.tolist()
        got, want = df[name].unique(array_type="numpy", **drop), host[name].unique(array_type="numpy", **drop)
        assert np.array_equal(np.ma.getmaskarray(got), np.ma.getmaskarray(want))
        keep = ~np.ma.getmaskarray(want)
        assert np.array_equal(np.ma.getdata(got)[keep], np.ma.getdata(want)[keep], equal_nan=True)
        assert df[name].nunique(**drop) == host[name].nunique(**drop)
    got, want = df.filter("u > 40").value_counts("k", selection="q", **drop), host.filter("u > 40").value_counts("k", selection="q", **drop)
    assert list(got.index.map(str)) == list(want.index.map(str)) and got.tolist() == want.tolist()
    keys, inverse = df.unique("k", return_inverse=True, array_type="numpy")
    hkeys, hinverse = host.unique("k", return_inverse=True, array_type="numpy")
    assert np.array_equal(inverse, hinverse) and np.array_equal(np.ma.getmaskarray(keys), np.ma.getmaskarray(hkeys))


# ---- groupby ----------------------------------------------------------------------------------
def _sorted_groups(res, keys):
    cols = {k: np.ma.asarray(res.columns[k] if not isinstance(res.columns[k], DeviceArray) else res.columns[k].to_numpy())
            for k in res.columns}
    order = np.lexsort([np.ma.getdata(cols[k]) for k in reversed(keys)] + [np.ma.getmaskarray(cols[k]) for k in reversed(keys)])
    return {k: v[order] for k, v in cols.items()}


@pytest.mark.parametrize("by,sparse", [(["k"], "auto"), (["k", "k2"], "auto"), (["k", "k2"], True)])
def test_groupby_by_a_masked_key(by, sparse):
    columns, host, df = _frames()
    agg = {"n": vaex_amd.agg.count(), "nx": vaex_amd.agg.count("x"), "sx": vaex_amd.agg.sum("x"), "mx": vaex_amd.agg.mean("x"),
           "sa": vaex_amd.agg.sum("a")}
    key = by[0] if len(by) == 1 else by
    got = _sorted_groups(df.groupby(key, agg=agg, assume_sparse=sparse), by)
    want = _sorted_groups(host.groupby(key, agg=agg, assume_sparse=sparse), by)
    assert set(got) == set(want)
    # the null group is there: one group per distinct (missing, value) combination, sizes by numpy
    mk = np.ma.getmaskarray(columns["k"])
    ids = np.where(mk, 10 ** 6, columns["k"].data).astype(np.int64) * 10 + (columns["k2"] if len(by) == 2 else 0)
    _, sizes = np.unique(ids, return_counts=True)
    assert sorted(np.ma.getdata(got["n"]).tolist()) == sorted(sizes.tolist())
    null = np.ma.getmaskarray(want["k"])
    assert np.array_equal(np.ma.getmaskarray(got["k"]), null)  # a masked label wherever the host frame has one
    if sparse is True:
        assert null.sum() == len(np.unique(columns["k2"][mk]))
    for name in got:
        g, w = got[name], want[name]
        m = np.ma.getmaskarray(w)
        assert np.array_equal(np.ma.getmaskarray(g), m), name
        if name in ("sx", "mx"):
            assert np.allclose(np.ma.getdata(g)[~m], np.ma.getdata(w)[~m], rtol=1e-6, atol=0, equal_nan=True), name
        else:
            assert np.array_equal(np.ma.getdata(g)[~m], np.ma.getdata(w)[~m]), name
    small = {"n": vaex_amd.agg.count(), "sx": vaex_amd.agg.sum("x")}
    got = _sorted_groups(df.filter("u > 30").groupby(key, agg=small, assume_sparse=sparse), by)
    _, sizes = np.unique(ids[columns["u"] > 30], return_counts=True)
    assert sorted(np.ma.getdata(got["n"]).tolist()) == sorted(sizes.tolist())
    if sparse is not True:  # the host frame's combined-key route refuses np.ma values under a filter
        want = _sorted_groups(host.filter("u > 30").groupby(key, agg=small, assume_sparse=sparse), by)
        assert np.array_equal(got["n"], want["n"]) and np.allclose(got["sx"], want["sx"], rtol=1e-6, atol=0, equal_nan=True)


def test_groupby_masked_values_by_an_unmasked_key():
    _, host, df = _frames()
    agg = {"n": vaex_amd.agg.count("a"), "sa": vaex_amd.agg.sum("a"), "mx": vaex_amd.agg.mean("x")}
    got, want = _sorted_groups(df.groupby("k2", agg=agg), ["k2"]), _sorted_groups(host.groupby("k2", agg=agg), ["k2"])
    for name in want:
        assert np.allclose(np.ma.getdata(got[name]), np.ma.getdata(want[name]), rtol=1e-6, atol=0), name


# ---- take / extract / sort --------------------------------------------------------------------
def _assert_masked_equal(got, want, name=""):
    assert isinstance(got, DeviceMaskedArray), (name, type(got))
    g = got.to_numpy()
    m = np.ma.getmaskarray(want)
    assert np.array_equal(g.mask, m), name
    assert np.array_equal(g.data[~m], np.ma.getdata(want)[~m], equal_nan=True), name


def test_take_with_missing_lookups():
    columns, _, df = _frames()
    rng = np.random.default_rng(3)
    lookup = rng.integers(0, N, 3001)
    lookup[::13] = -1
    for rows in (lookup.astype(np.int64), DeviceArray.from_numpy(lookup.astype(np.int32))):
        taken = df.take(rows)
        assert len(taken) == len(lookup)
        for name in ("a", "x", "p", "y"):
            col = columns[name]
            want = np.ma.array(col.data[np.where(lookup < 0, 0, lookup)], mask=np.ma.getmaskarray(col)[lookup] | (lookup < 0))
            _assert_masked_equal(taken.columns[name], want, name)
        assert isinstance(taken.columns["u"], DeviceArray)
        assert np.array_equal(taken.columns["u"].to_numpy()[lookup >= 0], columns["u"][lookup[lookup >= 0]])
    assert int(df.take(lookup).count("a")) == int((~np.ma.getmaskarray(columns["a"])[lookup] & (lookup >= 0)).sum())


def test_extract_and_filtered_evaluate():
    columns, host, df = _frames()
    e = "(u > 25) & (x < 90)"
    data, mask = missing_np.evaluate(e, columns)
    keep = data & ~mask
    ex = df.filter(e).extract()
    assert len(ex) == int(keep.sum()) and not ex.filtered
    for name in ("a", "x", "q"):
        _assert_masked_equal(ex.columns[name], columns[name][keep], name)
    got = df.filter(e).evaluate("a + u")  # the kept rows as np.ma
    want = host.filter(e).evaluate("a + u")
    assert np.ma.isMaskedArray(got) and np.array_equal(got.mask, np.ma.getmaskarray(want))
    assert np.array_equal(got.data[~got.mask], want.data[~got.mask])
    assert np.array_equal(df.filter(e).evaluate("fillmissing(a, 0)"), host.filter(e).evaluate("fillmissing(a, 0)"))


def test_sort_carries_masked_payloads():
    columns, _, df = _frames()
    order = np.argsort(columns["o"], kind="stable")
    s = df.sort("o")
    for name in ("a", "x", "p"):
        _assert_masked_equal(s.columns[name], columns[name][order], name)
    s = df.filter("u > 50").sort(["k2", "o"], ascending=False)
    keep = np.flatnonzero(columns["u"] > 50)
    order = keep[np.lexsort([columns["o"][keep], columns["k2"][keep]])][::-1]
    _assert_masked_equal(s.columns["a"], columns["a"][order], "a")


# ---- the frame methods ------------------------------------------------------------------------
def test_drop_and_fill_against_numpy_ma():
    columns, _, df = _frames()
    ma, mx, mb = (np.ma.getmaskarray(columns[k]) for k in ("a", "x", "b"))
    nan = np.isnan(columns["x"].data)
    u = columns["u"]
    assert np.array_equal(df.dropmissing(["a", "x"]).evaluate("u"), u[~ma & ~mx])
    assert np.array_equal(df.dropnan(["a", "x"]).evaluate("u"), u[~(nan & ~mx)])
    assert np.array_equal(df.dropna(["a", "x"]).evaluate("u"), u[~ma & ~mx & ~nan])
    every = np.zeros(N, bool)
    for v in columns.values():
        every |= np.ma.getmaskarray(v)
    assert len(df.dropmissing()) == int((~every).sum())
    assert len(df.filter("u > 50").dropna(["b"])) == int(((u > 50) & ~mb).sum())
    d2 = df.copy()
    d2.select_non_missing(column_names=["a", "x"])
    assert d2.selected_length() == int((~ma & ~mx & ~nan).sum())
    d2.select_non_missing(drop_nan=False, column_names=["a", "x"])
    assert d2.selected_length() == int((~ma & ~mx).sum())
    filled = df.fillna(-1, ["a", "x"])
    assert not filled.is_masked("a") and filled.is_masked("b")
    assert np.array_equal(filled.evaluate("a").to_numpy(), np.where(ma, -1, columns["a"].data))
    assert np.array_equal(filled.evaluate("x").to_numpy(), np.where(mx | nan, -1.0, columns["x"].data))
    assert float(filled.sum("x")) == pytest.approx(float(np.where(mx | nan, -1.0, columns["x"].data).sum()), rel=1e-9)
    assert df.is_masked("a") and "__original_a" in filled.columns and "a" in df.columns


# ---- what does not take masks yet raises -----------------------------------------------------
def test_out_of_scope_raises_naming_the_column():
    columns, _, df = _frames()
    other = vaex_amd.from_arrays(k2=DeviceArray.from_numpy(np.arange(4, dtype=np.int64)), z=DeviceArray.from_numpy(np.arange(4.0)))
    t = np.datetime64("2020-01-01", "s") + np.arange(N).astype("m8[s]") * 3600
    dft = vaex_amd.from_arrays(t=DeviceMaskedArray.from_numpy(np.ma.array(t, mask=missing_np.mask_of("mixed"))),
                               v=DeviceArray.from_numpy(np.arange(N, dtype=np.float64)))
    from vaex_amd.dataframe import DataFrame
    from vaex_amd.execution import ExecutorLocal

    class TwoRanks(ExecutorLocal):
        world = 2

    ranks = DataFrame(df.columns, executor=TwoRanks())
    pa = pytest.importorskip("pyarrow")
    with pytest.raises(NotImplementedError, match="nulls"):  # nulls in a string column
        vaex_amd.DeviceStringArray.from_arrow(pa.array(["a", None, "c"]))
    calls = [
        ("a", lambda: ranks.sum("u")),                                  # a multi-rank frame
        ("a", lambda: df.join(other, on="k2")),                         # a masked payload column
        ("a", lambda: other.join(df, on="k2")),
        ("a", lambda: df.join(df, left_on="k", right_on="k", rsuffix="_r")),  # a masked key: the frame's first masked column
        ("k", lambda: df._index("k")),
        ("x", lambda: df.sort("x")),                                    # a masked sort key
        ("a + u", lambda: df.sort(["u", "a + u"])),
        ("x", lambda: df.percentile_approx("x", 50)),
        ("x", lambda: df.median_approx("x")),
        ("y", lambda: df.percentile_approx("u", 50, binby="y", limits=[-2, 2], shape=4)),
        ("x", lambda: df.mutual_information("x", "u")),
        ("x", lambda: df.cov("u", "x")),
        ("x", lambda: df.covar("x", "u")),
        ("x", lambda: df.correlation("u", "x")),
        ("a", lambda: df.export_hdf5("/dev/null")),
        ("a", lambda: df.export_arrow("/dev/null")),
        ("t", lambda: vaex_amd.BinnerTime.per_day(dft.t)),
        ("fillmissing(t, 0)", lambda: dft.evaluate("fillmissing(t, 0)")),               # NaT / datetime fills are not a mask yet
    ]
    for name, call in calls:
        with pytest.raises(NotImplementedError) as err:
            call()
        assert repr(name) in str(err.value), (name, str(err.value))
    # an unmasked expression over the same frame still computes
    assert np.isfinite(df.percentile_approx("u", 50)) and np.isfinite(df.correlation("u", "o"))
    assert np.isfinite(df.covar("fillna(x, 0.0)", "u"))
