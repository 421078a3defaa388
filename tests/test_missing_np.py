"""tests/missing_np.py (the numpy restatement of the missing-value rule) against ``np.ma`` where
the two agree, and the host-frame functions (``ismissing`` ... ``fillna``) against the
reference's definitions on ``np.ma`` inputs.  No GPU."""
import numpy as np
import pytest

import expr_np
import missing_np
import vaex_amd


def _ma_namespace(columns):
    ns = dict(np=np, minimum=np.ma.minimum, maximum=np.ma.maximum, abs=np.ma.abs, floor=np.ma.floor)
    ns.update(columns)
    return ns


@pytest.mark.parametrize("kind", missing_np.MASK_KINDS)
@pytest.mark.parametrize("expression", missing_np.OPERATORS)
def test_restatement_equals_numpy_ma(expression, kind):
    # values in [1, 100] and no NaN: np.ma adds no domain mask
    columns = missing_np.small_columns(kind, nan=False)
    data, mask = missing_np.evaluate(expression, columns)
    want = eval(expression, {"__builtins__": {}}, _ma_namespace(columns))  # noqa: S307
    assert np.ma.isMaskedArray(want), expression
    assert np.array_equal(np.ma.getmaskarray(want), mask), expression  # exactly equal
    valid = ~mask
    assert data.dtype == want.dtype, (expression, data.dtype, want.dtype)
    assert np.array_equal(np.ma.getdata(want)[valid], data[valid]), expression


def test_every_operator_of_the_rule_is_compared():
    text = " ".join(missing_np.OPERATORS)
    for op in ("+", "-", "*", "<", "<=", "==", "!=", "&", "|", "~", "minimum", "maximum", "abs", "floor", "-a"):
        assert op in text, op


@pytest.mark.parametrize("kind", missing_np.MASK_KINDS)
def test_where_follows_the_chosen_branch(kind):
    columns = missing_np.small_columns(kind)
    p, a, b = columns["p"], columns["a"], columns["b"]
    data, mask = missing_np.evaluate("where(p, a, b)", columns)
    mp, ma, mb = (np.ma.getmaskarray(v) for v in (p, a, b))
    want = mp | np.where(p.data, ma, mb)
    assert np.array_equal(mask, want)
    assert np.array_equal(data[~mask], np.where(p.data, a.data, b.data)[~mask])


def test_edge_columns_cover_every_dtype_and_mask_kind():
    for kind in missing_np.MASK_KINDS:
        cols = missing_np.edge_columns(kind)
        assert set(cols) == set(expr_np.edge_columns())
        for name, col in cols.items():
            m = np.ma.getmaskarray(col)
            assert len(m) == expr_np.N
            assert m.all() if kind == "missing" else (not m.any() if kind == "valid" else 0 < m.sum() < len(m))
    m = missing_np.mask_of("mixed")
    words = m[:2048].reshape(-1, 8)
    assert len({tuple(w) for w in words}) > 16  # the 8-row words mix


# ---- the host-frame functions --------------------------------------------------------------
def _reference(name, x, value=None):
    """what the reference's functions (functions.py:146-268) are documented to give on a np.ma /
    numpy array, written from their rule: missing = the mask; NaN = a NaN at a row that is not
    missing; NA = either; a fill writes the value where the condition holds"""
    def ismissing(x):
        return np.ma.getmaskarray(x).copy() if np.ma.isMaskedArray(x) else np.zeros(len(x), dtype=bool)

    def isnan(x):
        data = np.ma.getdata(x)
        nan = np.isnan(data) if data.dtype.kind == "f" else np.zeros(len(data), bool)
        return nan & ~ismissing(x)

    def isna(x):
        return isnan(x) | ismissing(x)

    def fill(mask):
        if not np.any(mask):
            return x
        ar = x.data.copy() if np.ma.isMaskedArray(x) else x.copy()
        ar[mask] = value
        return ar

    if name == "ismissing":
        return ismissing(x)
    if name == "notmissing":
        return ~ismissing(x)
    if name == "isna":
        return isna(x)
    if name == "notna":
        return ~isna(x)
    if name == "fillmissing":
        return fill(ismissing(x))
    if name == "fillna":
        return fill(isna(x))
    assert name == "fillnan"
    if x.dtype.kind != "f":
        return x
    mask = isnan(x)
    if not np.any(mask):
        return x
    ar = x.copy()  # a masked array keeps its mask
    ar[mask] = value
    return ar


@pytest.mark.parametrize("kind", missing_np.MASK_KINDS)
@pytest.mark.parametrize("name", ["ismissing", "notmissing", "isna", "notna", "fillmissing", "fillnan", "fillna"])
@pytest.mark.parametrize("column", ["a", "x", "u"])
def test_host_functions_equal_the_reference(name, column, kind):
    columns = missing_np.small_columns(kind)
    df = vaex_amd.from_arrays(**columns)
    fills = name.startswith("fill")
    e = f"{name}({column}, 3)" if fills else f"{name}({column})"
    got = df.evaluate(e)
    want = _reference(name, columns[column], 3)
    gm, wm = np.ma.getmaskarray(got), np.ma.getmaskarray(want)
    assert np.array_equal(gm, wm), e
    assert np.ma.getdata(got).dtype == np.ma.getdata(want).dtype
    g, w = np.ma.getdata(got)[~wm], np.ma.getdata(want)[~wm]
    assert np.array_equal(g, w, equal_nan=w.dtype.kind == "f"), e
    if name in ("fillmissing", "fillna") or not fills:
        assert not gm.any()
    # and the restatement agrees with both
    data, mask = missing_np.evaluate(e, columns)
    assert np.array_equal(mask if mask is not None else np.zeros(len(data), bool), wm), e
    assert np.array_equal(data[~wm], w, equal_nan=w.dtype.kind == "f"), e


def test_isnan_is_false_at_missing_rows_and_fillnan_keeps_the_mask():
    x = np.ma.array([1.0, np.nan, np.nan, 4.0], mask=[False, False, True, True])
    df = vaex_amd.from_arrays(x=x)
    assert df.evaluate("isna(x)").tolist() == [False, True, True, True]
    assert df.evaluate("isnan(x)").tolist() == [False, True, False, False]
    f = df.evaluate("fillnan(x, 9.0)")
    assert np.ma.isMaskedArray(f) and np.ma.getmaskarray(f).tolist() == [False, False, True, True]
    assert f.data[:2].tolist() == [1.0, 9.0]
    assert str(df.x.fillna(0)) == "fillna(x, 0)" and str(df.x.ismissing()) == "ismissing(x)"
    assert df.is_masked("x") and df.x.is_masked


def test_host_filter_keeps_nothing_at_missing_rows():
    """a host filter whose expression is masked keeps data & ~mask, as a selection does"""
    p = np.ma.array([True, True, False, False, True], mask=[False, True, False, True, False])
    x = np.ma.array([5.0, 6.0, 7.0, 8.0, 1.0], mask=[False, False, True, False, False])
    df = vaex_amd.from_arrays(p=p, x=x, u=np.arange(5))
    assert df.filter("p").evaluate("u").tolist() == [0, 4]
    assert df.filter("x > 2").evaluate("u").tolist() == [0, 1, 3]
    assert df.filter("p & (x > 2)").evaluate("u").tolist() == [0]
    assert df.filter("~p").evaluate("u").tolist() == [2]
    assert df.filter("u > 1").evaluate("u").tolist() == [2, 3, 4]  # unmasked: as before
    assert df.filter("x > 2").evaluate_filter_mask(0, 5).tolist() == df._expression_mask("x > 2", 0, 5).tolist()


def test_virtual_columns_match_as_whole_words():
    """a virtual column is looked up by name, not by substring: `x` reading `__original_x` (what
    fillna builds) or `xx` does not evaluate itself"""
    df = vaex_amd.from_arrays(a=np.arange(4.0))
    df.add_virtual_column("xx", "a + 1")
    df.add_virtual_column("x", "xx * 2")
    df.add_virtual_column("x_2", "x + xx")
    assert df.evaluate("x").tolist() == [2.0, 4.0, 6.0, 8.0]
    assert df.evaluate("x_2").tolist() == [3.0, 6.0, 9.0, 12.0]
    assert df.evaluate("x + x_2").tolist() == [5.0, 10.0, 15.0, 20.0]
    filled = vaex_amd.from_arrays(x=np.ma.array([1.0, 2.0], mask=[False, True])).fillna(np.float64(9.0))
    assert filled.virtual_columns["x"] == "fillna(__original_x, 9.0)"  # a numpy scalar as its Python value
    assert filled.evaluate("x").tolist() == [1.0, 9.0]
    assert str(filled.x.fillmissing(np.int32(3))) == "fillmissing(x, 3)"


def test_host_frame_drop_and_fill():
    x = np.ma.array([1.0, np.nan, 3.0, 4.0, 5.0], mask=[False, False, True, False, False])
    i = np.ma.array([1, 2, 3, 4, 5], mask=[True, False, False, False, False])
    df = vaex_amd.from_arrays(x=x, i=i, u=np.arange(5))
    assert df.dropmissing().evaluate("u").tolist() == [1, 3, 4]
    assert df.dropnan().evaluate("u").tolist() == [0, 2, 3, 4]
    assert df.dropna().evaluate("u").tolist() == [3, 4]
    assert df.dropna(["x"]).evaluate("u").tolist() == [0, 3, 4]
    filled = df.fillna(-1)
    assert filled.evaluate("x").tolist() == [1.0, -1.0, -1.0, 4.0, 5.0]
    assert filled.evaluate("i").tolist() == [-1, 2, 3, 4, 5]
    assert "__original_x" in filled.columns and "x" not in filled.columns and "u" in filled.columns
    assert "x" in df.columns  # not in place
