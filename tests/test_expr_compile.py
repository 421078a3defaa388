"""Host side of the device expression evaluator (vaex_amd/expr.py), no GPU: the compiled
program's result dtype is numpy 2's for every expression (NEP 50 weak scalars, float32
rounding, narrow-int wrap), unsupported syntax is refused, and the numpy model of the stack
machine (tests/expr_np.py, one entry per opcode) run on the program reproduces numpy's own
evaluation bit for bit, on tame data and over the edge-value frame and expression matrix that
tests/test_gpu_expr_edges.py runs on the GPU; the opcode tables of expr.py, expr.hip and the
model are held in step."""
import numpy as np
import pytest

import expr_np
import vaex_amd
from vaex_amd import expr

OP = expr.OP
INV = {v: k for k, v in OP.items()}


def _frame():
    rng = np.random.default_rng(0)
    n = 257
    return vaex_amd.from_arrays(
        x=rng.normal(size=n), y=rng.normal(size=n) + 2, f=rng.normal(size=n).astype(np.float32),
        i=rng.integers(-50, 50, n).astype(np.int64), i32=rng.integers(-1000, 1000, n).astype(np.int32),
        i8=rng.integers(-100, 100, n).astype(np.int8), u8=rng.integers(0, 255, n).astype(np.uint8),
        b=rng.random(n) > 0.5)


def _run(prog, df):
    """the numpy model of csrc/expr.hip's stack machine (tests/expr_np.py) on a frame's columns."""
    return expr_np.run_model(prog, {k: np.asarray(v) for k, v in df.columns.items()})


EXPRESSIONS = [
    "x + y", "x * 2 - y / 3", "(x > 0) & (y < 2.5)", "x ** 2 + sqrt(abs(y))", "i % 7", "i // 3", "-i", "~b",
    "where(x > 0, x, -x)", "i8 + i8", "i8 * 3", "f * 2.5 + f", "i32 / 2", "x // 0.7", "x % -1.3",
    "minimum(x, y)", "u8 + 1", "i << 2", "x ** 3 - x ** 0.5", "b & (i > 3)", "f + i8", "f + i32", "i32 + i8",
    "np.floor(x) + 1", "isnan(log(x))", "u8 > 200", "i == 3", "b | ~b", "x + 1 - 1", "where(b, i8, i32)",
    "astype(i32, 'float64')", "astype(i, 'float64') ** 2", "astype(x * 100, 'int32')", "astype(i32, 'int8')",
    "astype(f, 'float64') + x", "astype(x, 'float32')", "astype(u8, 'int16') - 300", "astype(x, 'float64')",
]


@pytest.mark.parametrize("e", EXPRESSIONS)
def test_program_matches_numpy(e):
    df = _frame()
    prog = expr.compile_expression(df, e)
    ns = dict(np=np, sqrt=np.sqrt, abs=np.abs, where=np.where, minimum=np.minimum, isnan=np.isnan, log=np.log,
              astype=lambda a, d: np.asarray(a).astype(d))
    ns.update({k: np.asarray(v) for k, v in df.columns.items()})
    with np.errstate(all="ignore"):
        expected = np.asarray(eval(e, {"__builtins__": {}}, ns))  # noqa: S307
    assert prog.dtype == expected.dtype, (e, prog.dtype, expected.dtype)
    got = _run(prog, df)
    np.testing.assert_array_equal(got, expected)


@pytest.mark.parametrize("e", ["x.mean()", "[x]", "lambda: 1", "unknown + 1", "x if y else 1", "sum(x)", "x @ y"])
def test_unsupported_is_refused(e):
    with pytest.raises(expr.UnsupportedExpression):
        expr.Program(_frame(), e)


def test_virtual_columns_and_variables_inline():
    df = _frame()
    df["z"] = df.x + df.y
    df.variables["k"] = 3
    prog = expr.compile_expression(df, "z * k")
    assert prog.columns == ["x", "y"] and prog.dtype == np.float64
    np.testing.assert_array_equal(_run(prog, df), (np.asarray(df.columns["x"]) + np.asarray(df.columns["y"])) * 3)


def test_stack_depth_limit():
    deep = "x" + "".join(f" + (y * (x - {k}" for k in range(9)) + ")" * 18
    with pytest.raises(expr.UnsupportedExpression):
        expr.Program(_frame(), deep)


def test_chained_comparison_is_a_conjunction():
    df = _frame()
    x = np.asarray(df.columns["x"])
    np.testing.assert_array_equal(_run(expr.compile_expression(df, "0 < x < 1"), df), (0 < x) & (x < 1))


# ---- the model, the opcode tables and the edge-value matrix (tests/expr_np.py) ---------------

def test_model_implements_every_opcode():
    """The numpy model has a branch for every opcode the compiler can emit, and agrees with the
    compiler on which of them pop two slots."""
    assert set(OP) - expr_np.IMPLEMENTED == set(), "opcodes without a model"
    assert expr_np.IMPLEMENTED - set(OP) == set(), "model entries that are no opcode"
    assert {INV[c] for c in expr.BINARY} == set(expr_np.BINARY)


def test_opcode_tables_agree():
    """expr.OP and the enum of csrc/expr.hip (kept in step by hand): the same names and numbers;
    is_binary of expr.hip admits what expr.BINARY lists."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(expr.__file__), "csrc", "expr.hip")).read()
    block = re.search(r"enum\s*:\s*uint32_t\s*\{(.*?)\};", src, re.S).group(1)
    table = {name: int(num) for name, num in re.findall(r"OP_(\w+)\s*=\s*(\d+)", block)}
    assert table == OP
    assert len(set(OP.values())) == len(OP), "two opcodes share a number"
    assert all(0 <= v < 256 for v in OP.values())  # op | arg << 8

    def is_binary(op):  # expr.hip, restated
        return (OP["ADD_F"] <= op <= OP["MOD_F32"] and op not in (OP["NEG_F"], OP["ABS_F"])) or \
               (OP["ADD_I"] <= op <= OP["POW_I"] and op not in (OP["NEG_I"], OP["ABS_I"], OP["INV_I"])) or \
               (OP["LT_F"] <= op <= OP["GE_U"]) or (OP["FLOORDIV_U"] <= op <= OP["POW_U"])
    body = re.search(r"inline bool is_binary\(uint32_t op\) \{(.*?)\n\}", src, re.S).group(1)
    assert re.findall(r"OP_(\w+)", body) == ["ADD_F", "MOD_F32", "NEG_F", "ABS_F", "ADD_I", "POW_I", "NEG_I", "ABS_I",
                                            "INV_I", "LT_F", "GE_U", "FLOORDIV_U", "POW_U"], "is_binary changed: restate it"
    assert {v for v in OP.values() if is_binary(v)} == set(expr.BINARY)


def _edge_frame():
    return vaex_amd.from_arrays(**expr_np.edge_columns())


def test_edge_matrix_emits_every_opcode():
    """The expressions that tests/test_gpu_expr_edges.py runs on the GPU, compiled against the
    edge frame, use every opcode: none goes unexercised there."""
    df = _edge_frame()
    seen = set()
    for e in expr_np.ALL + expr_np.TERMS:
        seen |= {INV[ins & 0xFF] for ins in expr.Program(df, e).code}
    assert set(OP) - seen == set()


@pytest.mark.parametrize("e", expr_np.ALL + expr_np.TERMS)
def test_edge_matrix_matches_numpy(e):
    """The compiled program, run by the model over the edge frame (+-0.0, +-inf, NaN, integer
    extremes, values beyond 2**53 and 2**63, inexact float32 constants), against numpy's own
    evaluation: dtype and every row (expr_np.check)."""
    cols = expr_np.edge_columns()
    prog = expr.Program(_edge_frame(), e)
    expr_np.check(e, expr_np.run_model(prog, cols), cols, prog.dtype)


@pytest.mark.parametrize("e", expr_np.REFUSED)
def test_what_numpy_refuses_is_unsupported(e):
    """A Python int outside the column's dtype in arithmetic, minimum / maximum, where, shifts;
    dtype pairs without a loop; float16 results: UnsupportedExpression, never numpy's own error."""
    with pytest.raises(expr.UnsupportedExpression):
        expr.Program(_edge_frame(), e)


def test_float32_weak_scalar_is_rounded_on_the_host():
    """`f > 0.1` compares with float32(0.1): the constant pushed is already the float32 value,
    so the program keeps the COL CONST CMP shape of the comparison-terms kernel."""
    prog = expr.Program(_edge_frame(), "f > 0.1")
    assert [INV[i & 0xFF] for i in prog.code] == ["COL", "CONST", "GT_F"]
    assert np.array(prog.consts, np.uint64).view(np.float64)[0] == float(np.float32(0.1))
    prog = expr.Program(_edge_frame(), "x > 0.1")
    assert np.array(prog.consts, np.uint64).view(np.float64)[0] == 0.1


def test_mixed_sign_comparison_is_exact():
    cols = dict(i=np.array([2**53 + 1, 2**62 + 1, -1, -1], np.int64), u=np.array([2**53, 2**62, 2**64 - 1, 0], np.uint64))
    df = vaex_amd.from_arrays(**cols)
    np.testing.assert_array_equal(expr_np.run_model(expr.Program(df, "i > u"), cols), [True, True, False, False])
    np.testing.assert_array_equal(expr_np.run_model(expr.Program(df, "u <= i"), cols), [True, True, False, False])
    np.testing.assert_array_equal(expr_np.run_model(expr.Program(df, "i != u"), cols), [True, True, True, True])


def test_unused_constants_are_dropped():
    prog = expr.Program(_edge_frame(), "where(f > 0.1, f * 0.1, 0.1) + 0.1")
    assert len(prog.consts) == 1 and max(i >> 8 for i in prog.code if i & 0xFF == OP["CONST"]) == 0


def _terms_shape(code):
    """match_terms of csrc/expr.hip, restated: T (T COMB)* [NOT_B] with T = COL [cvt] CONST [cvt]
    CMP and one COMB kind; (number of terms, ucol slots used, ucon slots used) or None."""
    names = [INV[i & 0xFF] for i in code]
    cvt = {"I2F", "U2F", "ROUND_F32", "WRAP"}
    cmp = {k for k, v in OP.items() if OP["LT_F"] <= v <= OP["GE_U"]}
    i = nt = ucol = ucon = 0
    comb = None
    while i < len(names) and names[i] == "COL" and nt < 8:
        i += 1
        if i < len(names) and names[i] in cvt:
            ucol, i = ucol + 1, i + 1
        if i >= len(names) or names[i] != "CONST":
            return None
        i += 1
        if i < len(names) and names[i] in cvt:
            ucon, i = ucon + 1, i + 1
        if i >= len(names) or names[i] not in cmp:
            return None
        i += 1
        nt += 1
        if nt > 1:
            if i >= len(names) or names[i] not in ("AND_I", "OR_I") or comb not in (None, names[i]):
                return None
            comb, i = names[i], i + 1
    if i < len(names) and names[i] == "NOT_B":
        i += 1
    return (nt, ucol, ucon) if nt and i == len(names) else None


def test_terms_expressions_have_the_terms_kernel_shape():
    """Every expr_np.TERMS program is one that match_terms accepts, so the three-way GPU test does
    compare k_expr_terms with the interpreter; the list reaches 8 terms and uses both conversion
    slots.  Shapes that match_terms refuses are told apart."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(expr.__file__), "csrc", "expr.hip")).read()
    lam = re.search(r"auto cvt = \[\]\(uint32_t op\) \{(.*?)\};", src, re.S).group(1)
    assert sorted(re.findall(r"OP_(\w+)", lam)) == ["I2F", "ROUND_F32", "U2F", "WRAP"], "match_terms changed: restate it"
    assert "op >= OP_LT_F && op <= OP_GE_U" in re.search(r"auto cmp = .*?;", src).group(0)
    assert "constexpr int EX_MAX_TERMS = 8;" in src
    df = _edge_frame()
    shapes = {e: _terms_shape(expr.Program(df, e).code) for e in expr_np.TERMS}
    assert [e for e, s in shapes.items() if s is None] == []
    assert max(s[0] for s in shapes.values()) == 8
    assert any(s[1] for s in shapes.values()) and any(s[2] for s in shapes.values())
    for e in ["x != x", "x + 1 > 2", "(x > 0) & (y < 1) | (f > 2)", "b", "i > j"]:
        assert _terms_shape(expr.Program(df, e).code) is None, e
    nine = " & ".join(f"({c} > 0)" for c in ["x", "y", "f", "g", "i", "j", "i32", "i16", "i8"])
    assert _terms_shape(expr.Program(df, nine).code) is None
