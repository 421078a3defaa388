"""Device expression evaluation at edge values (csrc/expr.hip: the interpreter k_expr and the
comparison-terms kernel k_expr_terms) against numpy 2 on the same host columns.

The frame, the expression matrix and the comparison rule live in tests/expr_np.py, which
tests/test_expr_compile.py runs through a numpy model of the kernel without a GPU; here the
kernels themselves run.  2051 rows: more than one k_expr<false,4> block (1024 rows) and more
than one k_expr_terms block (2048 rows), with a ragged tail; +-0.0, +-inf, NaN, subnormals,
integer extremes, uint64 beyond 2**63, int64 beyond 2**53, float32(0.1) and its neighbours.

Rule (expr_np.check): numpy's dtype; every row bit for bit (NaN matches NaN, the sign of zero
counts); for pow / exp / log / trigonometric / hyperbolic functions the rows where numpy gives
NaN, +-inf or +-0 exactly, the finite rows within 4 ulp (float64) or within 1 ulp of the float64
evaluation of the float32 inputs rounded once (one float32 function node)."""
import numpy as np
import pytest

import expr_np
from oracle import oracle

pytestmark = pytest.mark.gpu


def _device(columns):
    import vaex_amd
    from vaex_amd.device import DeviceArray
    return vaex_amd.from_arrays(**{k: DeviceArray.from_numpy(v) for k, v in columns.items()})


@pytest.fixture(scope="module")
def frame():
    return _device(expr_np.edge_columns())


def _evaluate(df, e):
    from vaex_amd.device import DeviceArray
    got = df.evaluate(e)
    assert isinstance(got, DeviceArray), "evaluated off the GPU"
    return got.to_numpy()


@pytest.mark.parametrize("e", expr_np.ALL)
def test_edge_expression_matches_numpy(frame, e):
    expr_np.check(e, _evaluate(frame, e), expr_np.edge_columns())


@pytest.mark.parametrize("e", expr_np.TERMS)
def test_terms_kernel_interpreter_and_numpy_agree(frame, monkeypatch, e):
    """T (& T)* / T (| T)* [~] over 1-, 2-, 4- and 8-byte columns, with the column conversion
    slot (integer column against a float constant), the constant conversion slot (a constant cast
    by astype), host-rounded float32 constants, out-of-range integer constants, a disjunction,
    negations and 8 terms: k_expr_terms, the interpreter (VH_EXPR_TERMS=0) and numpy, byte for
    byte.  test_expr_compile.py checks that each program has the shape match_terms accepts."""
    terms = _evaluate(frame, e)
    monkeypatch.setenv("VH_EXPR_TERMS", "0")
    interp = _evaluate(frame, e)
    expected = expr_np.numpy_eval(e, expr_np.edge_columns())
    assert terms.dtype == interp.dtype == expected.dtype == np.bool_
    np.testing.assert_array_equal(terms.view(np.uint8), expected.view(np.uint8))
    np.testing.assert_array_equal(interp.view(np.uint8), terms.view(np.uint8))


OFFSETS = [0, 1, 3, 5, 7]
LENGTHS = [1, 7, 8, 9, 255, 257, 1024, 2044]


@pytest.mark.parametrize("e", [
    "where(b, f * 0.1, g) + i8",  # k_expr<false,4>
    "x ** y",                     # k_expr<true,1>
    # k_expr_terms: 1-, 2-, 4-, 8-byte columns, signed and unsigned
    "(u8 > 200) | (i8 < -3)", "(i16 >= 3) & (u16 != 7)", "(f >= 0.1) | (u32 < 7) | (i32 == 3)",
    "(x > 0.1) & (u64 > 5) & (i < 9007199254740993)",
])
def test_tails_and_alignment(e):
    """Views frame[o:o+m] (load_slots8 takes 16-byte loads only from a 16-aligned address, the
    8-byte store only to an 8-aligned output) into a sentinel-filled buffer at the same offset:
    numpy on the same host slice, and not a byte written before the view or past m."""
    import vaex_amd
    from vaex_amd import expr
    from vaex_amd.device import DeviceArray
    cols = expr_np.edge_columns()
    full = {k: DeviceArray.from_numpy(v) for k, v in cols.items()}
    slack = 64
    for o in OFFSETS:
        for m in LENGTHS:
            view = {k: v[o:o + m] for k, v in cols.items()}
            df = vaex_amd.from_arrays(**{k: d[o:o + m] for k, d in full.items()})
            prog = expr.Program(df, e)
            size = prog.dtype.itemsize
            buf = DeviceArray.from_numpy(np.full((o + m + slack) * size, 0xAB, np.uint8).view(
                prog.dtype if prog.dtype.kind != "b" else np.uint8))
            prog.evaluate(df, 0, m, out=buf[o:o + m])
            raw = buf.to_numpy().view(np.uint8)
            assert (raw[:o * size] == 0xAB).all() and (raw[(o + m) * size:] == 0xAB).all(), (e, o, m, "wrote outside")
            got = raw[o * size:(o + m) * size].view(prog.dtype)
            expr_np.check(e, got, view, ulp=4 if e == "x ** y" else None)


def test_float32_constants_through_the_frame():
    """Where a user meets it: selection, filter and binby over a float32 column that holds many
    copies of float32(0.1) and of its neighbours, with the constant 0.1 (numpy compares and
    multiplies with float32(0.1), not with the float64 0.1)."""
    rng = np.random.default_rng(7)
    m = np.float32(0.1)
    near = np.array([m, np.nextafter(m, np.float32(1)), np.nextafter(m, np.float32(0))], np.float32)
    f = np.concatenate([np.tile(near, 1000), rng.random(3001).astype(np.float32)])
    rng.shuffle(f)
    df = _device(dict(f=f))
    assert int(df.count(selection="f > 0.1")) == int((f > 0.1).sum())
    assert int((f > 0.1).sum()) != int((f.astype(np.float64) > 0.1).sum())  # the data tells the two apart
    assert len(df[df.f == 0.1]) == int((f == 0.1).sum()) >= 1000
    prod = f * 0.1  # float32
    naive = (f.astype(np.float64) * 0.1).astype(np.float32)
    lo = float(prod[prod > naive].min())  # a bin edge on a value that the float64 constant misses from below
    assert (naive < prod).any()
    got = df.count(binby="f * 0.1", limits=[lo, 0.1], shape=64)
    exp = oracle.extract_central_part(oracle.compute_grid(
        [oracle.Binner("scalar", prod, vmin=lo, vmax=0.1, bins=64)], "count"))
    wrong = oracle.extract_central_part(oracle.compute_grid(
        [oracle.Binner("scalar", naive, vmin=lo, vmax=0.1, bins=64)], "count"))
    assert not np.array_equal(exp, wrong)
    np.testing.assert_array_equal(got, exp)
