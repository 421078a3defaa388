"""The device expression compiler on masked HBM columns (no GPU: programs are compiled, not run).
Compiling allocates nothing, so the columns are DeviceMaskedArrays around DeviceArrays that
point nowhere; the value program and the mask program are run through ``expr_np.run_model`` (the
kernel's model) on the host arrays and compared with the rule (tests/missing_np.py)."""
import numpy as np
import pytest

import expr_np
import missing_np
import vaex_amd
from vaex_amd.device import DeviceArray, DeviceMaskedArray
from vaex_amd.expr import MAX_COLS, OP, Program, UnsupportedExpression, compile_expression


def _stand_in(col):
    """a device column of the dtype and length of ``col`` that owns no memory"""
    n = len(col)
    data = DeviceArray(n, np.ma.getdata(col).dtype, _ptr=8)
    return DeviceMaskedArray(data, DeviceArray(n, np.uint8, _ptr=8)) if np.ma.isMaskedArray(col) else data


def _frame(columns):
    return vaex_amd.from_arrays(**{k: _stand_in(v) for k, v in columns.items()})


def _inputs(columns):
    """what the programs bind: name -> data, ("mask", name) -> the mask as a bool column"""
    ins = {k: np.ma.getdata(v) for k, v in columns.items()}
    ins.update({("mask", k): np.ma.getmaskarray(v) for k, v in columns.items() if np.ma.isMaskedArray(v)})
    return ins


class _MaskProgram:
    """the mask program of a Program, as run_model takes one"""

    def __init__(self, p):
        self.code, self.consts, self.columns, self.dtype = p.mask_code, p.consts, p.columns, np.dtype(bool)


def _run(p, columns):
    ins = _inputs(columns)
    data = expr_np.run_model(p, ins)
    mask = expr_np.run_model(_MaskProgram(p), ins) if p.mask_code is not None else None
    return data, mask


EXACT = missing_np.OPERATORS + missing_np.WHERES + missing_np.FUNCTIONS + \
    [e for e in missing_np.CONSTANTS if "sqrt" not in e]


@pytest.mark.parametrize("kind", missing_np.MASK_KINDS)
@pytest.mark.parametrize("expression", EXACT)
def test_value_and_mask_program_follow_the_rule(expression, kind):
    columns = missing_np.small_columns(kind)
    p = Program(_frame(columns), expression)
    data, mask = _run(p, columns)
    missing_np.check(expression, data, mask, columns)


@pytest.mark.parametrize("kind", missing_np.MASK_KINDS)
def test_every_dtype_propagates(kind):
    """x + x', unary minus, a comparison and fillmissing over every dtype of the edge frame"""
    columns = dict(missing_np.edge_columns(kind))
    df = _frame(columns)
    second = expr_np._SECOND
    for first, other in second.items():
        dt = np.ma.getdata(columns[first]).dtype
        exprs = [f"{first} == {other}", f"where({first} == {other}, {first}, {other})", f"ismissing({first})",
                 f"fillmissing({first}, 1)", f"isna({first})"]
        if dt.kind != "b":
            exprs += [f"{first} + {other}", f"minimum({first}, {other})"]
        else:
            exprs += [f"{first} & {other}", f"~{first}"]
        for e in exprs:
            p = Program(df, e)
            data, mask = _run(p, columns)
            missing_np.check(e, data, mask, columns)


def test_a_masked_column_binds_two_inputs():
    columns = missing_np.small_columns()
    df = _frame(columns)
    p = Program(df, "a + u")
    assert p.columns == ["a", ("mask", "a"), "u"]
    assert p.mask_code == [OP["COL"] | 1 << 8]
    assert Program(df, "u + 1").mask_code is None
    # a column read twice is one mask term; two columns are OR-ed
    assert Program(df, "a * a + a").mask_code == [OP["COL"] | 1 << 8]
    assert [c & 0xFF for c in Program(df, "a + b").mask_code] == [OP["COL"], OP["COL"], OP["OR_I"]]
    # the consumers give unmasked results in the existing opcodes
    assert Program(df, "ismissing(a)").code == [OP["COL"] | 1 << 8] and Program(df, "ismissing(a)").mask_code is None
    assert Program(df, "ismissing(u)").mask_code is None and Program(df, "ismissing(u)").consts == [0]
    assert [c & 0xFF for c in Program(df, "fillmissing(a, 7)").code] == [OP["COL"], OP["CONST"], OP["COL"], OP["WHERE"]]
    assert Program(df, "fillnan(x, 0.0)").mask_code is not None  # keeps the mask
    assert Program(df, "fillna(x, 0.0)").mask_code is None


def test_keep_program_has_the_terms_shape():
    columns = dict(missing_np.small_columns(), y=np.arange(missing_np.N, dtype=np.int32))
    df = _frame(columns)
    p = Program(df, "(x > 3) & (y <= 2)", keep=True)
    assert p.mask_code is None and p.dtype == np.bool_
    ops = [c & 0xFF for c in p.code]
    term = lambda cmp: [OP["COL"], OP["CONST"], OP[cmp]]  # noqa: E731
    # T (T AND)*: the shape the comparison-terms kernel takes, the mask as one more `== 0` term
    assert ops == term("GT_F") + term("LE_I") + [OP["AND_I"]] + term("EQ_I") + [OP["AND_I"]]
    assert p.columns[p.code[7] >> 8] == ("mask", "x") and p.consts[p.code[8] >> 8] == 0
    got = expr_np.run_model(p, _inputs(columns))
    x, y = columns["x"], columns["y"]
    with np.errstate(invalid="ignore"):
        want = (x.data > 3) & (y <= 2) & ~np.ma.getmaskarray(x)
    assert np.array_equal(got, want)
    # the same expression as a value keeps its mask; without masked operands keep changes nothing
    assert Program(df, "(x > 3) & (y <= 2)").mask_code is not None
    assert Program(df, "y <= 2", keep=True).code == Program(df, "y <= 2").code
    # any boolean keeps value & ~mask
    for e in ("p | q", "~p", "where(p, q, u > 50)", "(a < b) | (x > 50)"):
        got = expr_np.run_model(Program(df, e, keep=True), _inputs(columns))
        data, mask = missing_np.evaluate(e, columns)
        assert np.array_equal(got, data & ~mask), e
    with pytest.raises(UnsupportedExpression):
        Program(df, "a + b", keep=True)  # not a boolean


@pytest.mark.parametrize("expression", ["fillmissing(a, 1.5)", "fillmissing(a, 2147483648)", "fillna(a, nan)",
                                        "fillmissing(p, 2)", "fillmissing(a, b)", "fillmissing(a)", "ismissing(a, b)",
                                        "fillnan(a, 0.5)"])
def test_a_fill_value_the_dtype_cannot_hold_is_refused(expression):
    df = _frame(missing_np.small_columns())
    with pytest.raises(UnsupportedExpression):
        Program(df, expression)


def test_fill_values_convert_as_numpy_assignment():
    columns = missing_np.small_columns()
    df = _frame(columns)
    df.add_variable("v", 4)
    assert Program(df, "fillmissing(a, 3.0)").consts == [3]  # an integral float into an int column
    assert Program(df, "fillmissing(a, v)").consts == [4]  # a frame variable
    assert Program(df, "fillmissing(a, True)").consts == [1]
    assert Program(df, "fillmissing(x, 1)").consts == [int(np.array(1.0).view(np.uint64))]
    f = dict(columns, f=np.ma.array(np.ones(missing_np.N, np.float32), mask=missing_np.mask_of("mixed")))
    p = Program(_frame(f), "fillmissing(f, 0.1)")  # rounded to the column's float32
    assert p.consts == [int(np.array(float(np.float32(0.1))).view(np.uint64))] and p.dtype == np.float32


def test_the_cache_tells_masked_from_unmasked():
    columns = missing_np.small_columns()
    df = _frame(columns)
    masked = compile_expression(df, "a + 1")
    assert masked.mask_code is not None
    df.columns["a"] = df.columns["a"].data  # the same name and dtype, unmasked
    plain = compile_expression(df, "a + 1")
    assert plain is not masked and plain.mask_code is None and plain.columns == ["a"]
    assert compile_expression(df, "a + 1") is plain
    # and a row mask from the value of the same text
    assert compile_expression(df, "p & q", keep=True) is not compile_expression(df, "p & q")


def test_fifteen_masked_inputs_overflow_the_columns():
    n = 8
    cols = {f"c{k}": np.ma.array(np.ones(n), mask=np.zeros(n, bool), shrink=False) for k in range(15)}
    df = _frame(cols)
    assert len(Program(df, " + ".join(f"c{k}" for k in range(MAX_COLS // 2))).columns) == MAX_COLS
    with pytest.raises(UnsupportedExpression, match="too many columns"):
        Program(df, " + ".join(cols))


def test_frame_plumbing_without_a_device():
    columns = missing_np.small_columns()
    df = _frame(columns)
    assert df.is_device_resident() and df.is_masked("a") and not df.is_masked("u")
    assert df.is_masked("a + u") and not df.is_masked("fillmissing(a, 0) + u") and df.is_masked(df.a + 1)
    assert df.data_type("fillna(x, 0.0)") == np.float64
    assert df.dropmissing()._filter == "notmissing(a) & notmissing(b) & notmissing(x) & notmissing(p) & notmissing(q)"
    assert df.dropnan()._filter == "~isnan(x)"
    assert df.dropna(["x", "u"])._filter == "notmissing(x) & ~isnan(x)"
    assert df.dropmissing(["u"])._filter is None
    filled = df.fillna(0, ["a"])
    assert filled.virtual_columns == {"a": "fillna(__original_a, 0)"} and list(filled.columns)[0] == "__original_a"
    assert not filled.is_masked("a") and filled.data_type("a") == np.int32
    sliced = df.columns["a"][3:11]
    assert isinstance(sliced, DeviceMaskedArray) and len(sliced) == 8 and sliced.shape == (8,) and sliced.ndim == 1
    assert sliced.data.ptr == 8 + 3 * 4 and sliced.mask.ptr == 8 + 3 and sliced.nbytes == 8 * 5
    with pytest.raises(TypeError):
        np.asarray(df.columns["a"])  # a path that does not know masks fails, it does not drop one
    assert not isinstance(df.columns["a"], DeviceArray)
