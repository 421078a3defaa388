"""What the expression tests share, with and without a GPU (not a conftest):

* ``run_model``: a numpy model of csrc/expr.hip's stack machine, one entry per opcode of
  ``expr.OP`` with the kernel's semantics (64-bit slots as uint64 bit patterns), so that a
  compiled program can be checked against numpy where there is no GPU;
* ``edge_columns``: the edge-value frame (2051 rows: more than one interpreter block of 1024
  rows and more than one comparison-terms block of 2048, with a ragged tail);
* the expression matrix (``EXACT``, ``ULP64``, ``ULP32``, ``TERMS``, ``REFUSED``), numpy's
  own evaluation of an expression (``numpy_eval``) and the comparison rule (``check``).

Left out of the frame, by building the columns without them (never by masking rows):
float -> integer casts of NaN, +-inf or values outside the target range (undefined in C,
platform-dependent in numpy), negative shift counts (undefined in numpy), and integer **
with a negative exponent column (numpy raises)."""
import functools

import numpy as np

from vaex_amd import expr

OP = expr.OP
INV = {v: k for k, v in OP.items()}
N = 2051
M64 = 0xFFFFFFFFFFFFFFFF

# ---- the model --------------------------------------------------------------------------


def _f(u):
    return u.view(np.float64)


def _g(d):
    return np.ascontiguousarray(d, np.float64).view(np.uint64)


def _i(u):
    return u.view(np.int64)


def _h(v):
    return np.ascontiguousarray(v, np.int64).view(np.uint64)


def _b(m):
    return m.astype(np.uint64)


def _slot(c):
    """load_slot: floats as float64 bits, integers sign- / zero-extended (a uint64 column
    keeps its bits: no trip through int64 values)."""
    c = np.asarray(c)
    if c.dtype.kind == "f":
        return _g(c.astype(np.float64))
    if c.dtype.kind == "i":
        return _h(c.astype(np.int64))
    return c.astype(np.uint64)


def _wrap(x, arg):
    bits, sgn = arg & 0xFF, arg >> 8
    m = np.uint64(M64 if bits >= 64 else (1 << bits) - 1)
    u = x & m
    if sgn and bits < 64:
        neg = ((u >> np.uint64(bits - 1)) & np.uint64(1)) != 0
        u = np.where(neg, u | ~m, u)
    return u


def _divmod_f(a, b):
    """divmod_f of expr.hip (numpy's npy_divmod), in float64."""
    mod = np.fmod(a, b)
    div = (a - mod) / b
    adj = (mod != 0) & ((b < 0) != (mod < 0))
    mod2 = np.where(mod != 0, np.where(adj, mod + b, mod), np.copysign(0.0, b))
    div = np.where(adj, div - 1.0, div)
    fl = np.floor(div)
    fl = np.where(div - fl > 0.5, fl + 1.0, fl)
    fl = np.where(div != 0, fl, np.copysign(0.0, a / b))
    zero = b == 0
    return np.where(zero, a / b, fl), np.where(zero, mod, mod2)


def _floordiv_i(a, b):
    ia, ib = _i(a), _i(b)
    special = (ib == 0) | (ib == -1)
    q = _h(np.floor_divide(ia, np.where(special, 1, ib)))
    return np.where(ib == 0, np.uint64(0), np.where(ib == -1, np.uint64(0) - a, q))


def _mod_i(a, b):
    ia, ib = _i(a), _i(b)
    special = (ib == 0) | (ib == -1)
    return np.where(special, np.uint64(0), _h(np.remainder(ia, np.where(special, 1, ib))))


def _pow_u(a, e):
    r = np.ones_like(a)
    a, e = a.copy(), e.copy()
    for _ in range(64):
        r = np.where((e & np.uint64(1)) != 0, r * a, r)
        a = a * a
        e = e >> np.uint64(1)
    return r


def _shift(a, b, fn, big):
    ok = b < np.uint64(64)  # the kernel's (ib < 0 || ib >= 64), b read as unsigned
    return np.where(ok, fn(a, np.where(ok, b, np.uint64(0))), big(a))


def _min_f(a, b):
    fa, fb = _f(a), _f(b)
    return np.where(np.isnan(fa) | np.isnan(fb), np.where(np.isnan(fa), a, b), np.where(fa < fb, a, b))


def _max_f(a, b):
    fa, fb = _f(a), _f(b)
    return np.where(np.isnan(fa) | np.isnan(fb), np.where(np.isnan(fa), a, b), np.where(fa > fb, a, b))


def _fun(fn):
    return lambda x, arg: _g(fn(_f(x)))


UNARY = {
    "I2F": lambda x, arg: _g(_i(x).astype(np.float64)),
    "U2F": lambda x, arg: _g(x.astype(np.float64)),
    "I2F32": lambda x, arg: _g(_i(x).astype(np.float32).astype(np.float64)),
    "U2F32": lambda x, arg: _g(x.astype(np.float32).astype(np.float64)),
    "F2I": lambda x, arg: _h(_f(x).astype(np.int64)),
    "F2U": lambda x, arg: _f(x).astype(np.uint64),
    "ROUND_F32": lambda x, arg: _g(_f(x).astype(np.float32).astype(np.float64)),
    "WRAP": _wrap,
    "NEG_F": _fun(np.negative), "ABS_F": _fun(np.abs),
    "NEG_I": lambda x, arg: np.uint64(0) - x,
    "ABS_I": lambda x, arg: np.where(_i(x) < 0, np.uint64(0) - x, x),
    "INV_I": lambda x, arg: ~x,
    "NOT_B": lambda x, arg: _b(x == 0),
    "ISNAN": lambda x, arg: _b(np.isnan(_f(x))),
    "ISFINITE": lambda x, arg: _b(np.isfinite(_f(x))),
    "ISINF": lambda x, arg: _b(np.isinf(_f(x))),
}
UNARY.update({opname: _fun(ufunc) for ufunc, opname in expr.FUNCTIONS.values()})

_CMP = {"LT": np.less, "LE": np.less_equal, "GT": np.greater, "GE": np.greater_equal, "EQ": np.equal,
        "NE": np.not_equal}
BINARY = {
    "ADD_F": lambda a, b: _g(_f(a) + _f(b)), "SUB_F": lambda a, b: _g(_f(a) - _f(b)),
    "MUL_F": lambda a, b: _g(_f(a) * _f(b)), "DIV_F": lambda a, b: _g(_f(a) / _f(b)),
    "FLOORDIV_F": lambda a, b: _g(_divmod_f(_f(a), _f(b))[0]),
    "MOD_F": lambda a, b: _g(_divmod_f(_f(a), _f(b))[1]),
    "FLOORDIV_F32": lambda a, b: _g(_divmod_f(_f(a).astype(np.float32), _f(b).astype(np.float32))[0]),
    "MOD_F32": lambda a, b: _g(_divmod_f(_f(a).astype(np.float32), _f(b).astype(np.float32))[1]),
    "POW_F": lambda a, b: _g(np.power(_f(a), _f(b))),
    "MIN_F": _min_f, "MAX_F": _max_f,
    "ARCTAN2": lambda a, b: _g(np.arctan2(_f(a), _f(b))),
    "ADD_I": lambda a, b: a + b, "SUB_I": lambda a, b: a - b, "MUL_I": lambda a, b: a * b,
    "FLOORDIV_I": _floordiv_i, "MOD_I": _mod_i,
    "AND_I": lambda a, b: a & b, "OR_I": lambda a, b: a | b, "XOR_I": lambda a, b: a ^ b,
    "MIN_I": lambda a, b: np.where(_i(a) < _i(b), a, b),
    "MAX_I": lambda a, b: np.where(_i(a) > _i(b), a, b),
    "SHL_I": lambda a, b: _shift(a, b, np.left_shift, np.zeros_like),
    "SHR_I": lambda a, b: _shift(a, b, lambda x, s: _h(_i(x) >> s.astype(np.int64)),
                                 lambda x: np.where(_i(x) < 0, np.uint64(M64), np.uint64(0))),
    "POW_I": lambda a, b: np.where(_i(b) < 0, np.uint64(0), _pow_u(a, b)),
    "FLOORDIV_U": lambda a, b: np.where(b == 0, np.uint64(0), a // np.where(b == 0, np.uint64(1), b)),
    "MOD_U": lambda a, b: np.where(b == 0, np.uint64(0), a % np.where(b == 0, np.uint64(1), b)),
    "MIN_U": lambda a, b: np.where(a < b, a, b), "MAX_U": lambda a, b: np.where(a > b, a, b),
    "SHR_U": lambda a, b: _shift(a, b, np.right_shift, np.zeros_like),
    "POW_U": _pow_u,
}
for _name, _fn in _CMP.items():
    BINARY[_name + "_F"] = (lambda fn: lambda a, b: _b(fn(_f(a), _f(b))))(_fn)
    BINARY[_name + "_I"] = (lambda fn: lambda a, b: _b(fn(_i(a), _i(b))))(_fn)
    if _name not in ("EQ", "NE"):
        BINARY[_name + "_U"] = (lambda fn: lambda a, b: _b(fn(a, b)))(_fn)

IMPLEMENTED = set(UNARY) | set(BINARY) | {"COL", "CONST", "WHERE"}


def run_model(prog, columns):
    """The result of ``prog`` over ``columns`` (name -> numpy array), as k_expr computes it."""
    n = len(next(iter(columns.values())))
    st = []
    with np.errstate(all="ignore"):
        for ins in prog.code:
            op, arg = INV[ins & 0xFF], ins >> 8
            if op == "COL":
                st.append(_slot(columns[prog.columns[arg]]))
            elif op == "CONST":
                st.append(np.full(n, prog.consts[arg], np.uint64))
            elif op == "WHERE":
                b_, a_, c_ = st.pop(), st.pop(), st.pop()
                st.append(np.where(c_ != 0, a_, b_))
            elif op in BINARY:
                b_, a_ = st.pop(), st.pop()
                st.append(BINARY[op](a_, b_))
            else:
                st.append(UNARY[op](st.pop(), arg))
        assert len(st) == 1
        v = st[0]
        dt = prog.dtype
        if dt == np.float64:
            return _f(v).copy()
        if dt == np.float32:
            return _f(v).astype(np.float32)
        return v.astype(np.dtype(f"u{dt.itemsize}")).view(dt)  # the low bytes, as the kernel stores them


# ---- the edge frame ---------------------------------------------------------------------

def _float_edges(dt):
    fi = np.finfo(dt)
    e = [0.0, -0.0, np.inf, -np.inf, np.nan, fi.smallest_subnormal, fi.max, -fi.max, 1 + fi.eps, 1 - fi.epsneg,
         0.5, -0.5, 1.0, -1.0, 2.0, 3.0, -3.0, 6.0, 0.25]
    e = [dt(v) for v in e]
    for c in (0.1, 0.3, 0.7):  # float32(c) and its two neighbours (in float64: c as it is, too)
        m = dt(c)
        e += [m, np.nextafter(m, dt(np.inf)), np.nextafter(m, dt(-np.inf))]
    return np.array(e, dt)


def _int_edges(dt):
    ii = np.iinfo(dt)
    if dt == np.int64:
        e = [ii.min, ii.min + 1, -1, 0, 1, ii.max, 2**53 + 1, -(2**53 + 1), 2**53 + 2**29 + 1, -(2**53 + 2**29 + 1),
             2**62 + 1, 3, 2**53, 2**62, -7]
    elif dt == np.uint64:
        e = [0, 1, ii.max, 2**63 - 1, 2**63, 2**63 + 5, 2**63 + 2**39 + 1, 2**53 + 1, 2**53, 2**62, 3, 10,
             2**62 + 1, 2**53 + 2**29 + 1]
    elif ii.min < 0:
        e = [ii.min, ii.min + 1, -1, 0, 1, ii.max, 2, 3, -3, 7]
    else:
        e = [0, 1, ii.max, ii.max - 1, 2, 3, 7, 10]
    return np.array(e, dt)


_K = 32  # rows [0, _K * _K) hold every pair of a first column's and a second column's edge values


def _layout(edges, fill, second):
    """Edge values first (all pairs of a first and a second column), then the seeded fill with
    an edge value in every third row, through the ragged tail."""
    k = len(edges)
    assert k <= _K
    r = np.arange(N)
    col = fill.copy()
    head = r < _K * _K
    idx = np.where(head, (r % _K) if second else (r // _K), (r // 3 * 5 + 2) if second else (r // 3)) % k
    put = head | (r % 3 == 0)
    col[put] = edges[idx[put]]
    return col


@functools.lru_cache(maxsize=None)
def edge_columns():
    """name -> read-only numpy column.  First / second column per dtype: x y (float64), f g
    (float32), i j (int64), i32 j32, i16 j16, i8 j8, u64 v64, u32 v32, u16 v16, u8 v8, b c
    (bool); y and g double as divisor columns (+-0.0, +-inf, 0.5, 2, 3: exact quotients).
    sh: shift counts; ex: exponents >= 0; xs fs: floats that every integer cast can take."""
    rng = np.random.default_rng(20251)
    cols = {}
    for dt, names in ((np.float64, "xy"), (np.float32, "fg")):
        for second, name in enumerate(names):
            fill = (rng.normal(size=N) * 10.0 ** rng.uniform(-3, 3, N)).astype(dt)
            cols[name] = _layout(_float_edges(dt), fill, second)
    for dt, names in ((np.int64, ("i", "j")), (np.int32, ("i32", "j32")), (np.int16, ("i16", "j16")),
                      (np.int8, ("i8", "j8")), (np.uint64, ("u64", "v64")), (np.uint32, ("u32", "v32")),
                      (np.uint16, ("u16", "v16")), (np.uint8, ("u8", "v8"))):
        ii = np.iinfo(dt)
        for second, name in enumerate(names):
            wide = rng.integers(ii.min, ii.max, N, dtype=dt, endpoint=True)
            small = rng.integers(max(ii.min, -50), 50, N).astype(dt)
            cols[name] = _layout(_int_edges(dt), np.where(rng.random(N) < 0.5, wide, small), second)
    cols["b"] = _layout(np.array([False, True]), rng.random(N) < 0.5, False)
    cols["c"] = _layout(np.array([False, True]), rng.random(N) < 0.5, True)
    # 0, width - 1, width and 63 for every width; 64, the width of the 64-bit columns, included
    cols["sh"] = _layout(np.array([0, 1, 7, 8, 15, 16, 31, 32, 63, 64], np.uint8),
                         rng.integers(0, 64, N, endpoint=True).astype(np.uint8), True)
    cols["ex"] = _layout(np.arange(10, dtype=np.uint8), rng.integers(0, 10, N).astype(np.uint8), True)
    safe = [0.0, -0.0, 0.5, -0.5, 0.99999, -0.99999, 1.0, -1.0, 1.5, 2.5, -2.5, 100.0, -100.0, 127.0, -128.0, 5e-324]
    cols["xs"] = _layout(np.array(safe), rng.uniform(-100, 100, N), False)
    cols["fs"] = _layout(np.array(safe, np.float32), rng.uniform(-100, 100, N).astype(np.float32), False)
    for v in cols.values():
        assert len(v) == N
        v.setflags(write=False)
    return cols


# ---- the expression matrix ----------------------------------------------------------------

_ARITH = ["+", "-", "*", "/", "//", "%"]
_CMPS = ["<", "<=", ">", ">=", "==", "!="]
_INTS = ["i", "i32", "i16", "i8", "u64", "u32", "u16", "u8"]
_SECOND = {"x": "y", "f": "g", "i": "j", "i32": "j32", "i16": "j16", "i8": "j8", "u64": "v64", "u32": "v32",
           "u16": "v16", "u8": "v8", "b": "c"}


def _exact():
    e = []
    # float arithmetic: float64; float32 against float32, integers and inexact constants
    for op in _ARITH:
        e += [f"x {op} y", f"f {op} g", f"f {op} j8", f"f {op} j32", f"f {op} j", f"f {op} v64", f"j16 {op} f"]
        e += [f"x {op} {c}" for c in ("0.1", "0.7")] + [f"f {op} {c}" for c in ("0.1", "0.3", "0.7", "1.7")]
        e += [f"{c} {op} f" for c in ("0.1", "1.7")]
    e += ["f + 16777217", "f * 3", "x ** 2", "f ** 2", "x ** 0.5", "f ** 0.5", "x ** -1", "f ** -1", "f ** 1", "i32 ** 2.0"]
    # integer arithmetic: every width against itself, a narrower and a wider column; wrap-around
    for a in _INTS:
        for op in ["+", "-", "*", "//", "%", "/"]:
            e.append(f"{a} {op} {_SECOND[a]}")
        e += [f"-{a}", f"abs({a})", f"~{a}", f"{a} * 3", f"{a} - 1", f"{a} // 3", f"{a} % 10", f"{a} // -1" if a[0] == "i"
              else f"{a} // 1", f"{a} ** 2", f"{a} ** 3", f"{a} & {_SECOND[a]}", f"{a} | {_SECOND[a]}", f"{a} ^ {_SECOND[a]}",
              f"minimum({a}, {_SECOND[a]})", f"maximum({a}, {_SECOND[a]})", f"minimum({a}, 7)", f"maximum({a}, 3)"]
        dt = str(edge_columns()[a].dtype)
        e += [f"{a} << astype(sh, '{dt}')", f"{a} >> astype(sh, '{dt}')", f"{a} >> 1", f"{a} << 3",
              f"{a} ** astype(ex, '{dt}')"]
    e += ["i8 + j32", "i32 * j8", "i8 * j", "u8 + j8", "u8 - v32", "i16 // j8", "i32 % j16", "u16 // v8", "u32 % v16",
          "i % j32", "i // j8", "i % -1", "u64 + j8", "u64 * v8", "u64 // v32", "u64 % v8", "u64 >> v8", "u64 >> sh",
          "u64 << sh", "u64 / 2", "u64 - v32", "maximum(u64, v32)", "minimum(v8, u64)", "i8 << sh", "u8 >> sh", "i >> sh",
          "b + c", "b * c", "b + 1", "b * 2.5", "i8 + b", "i32 * -1", "u8 * u8", "i8 * i8", "u32 * u32"]
    # comparisons: same kind, int64 against uint64, inexact constants, ints against float constants
    for op in _CMPS:
        e += [f"{a} {op} {b}" for a, b in _SECOND.items()]
        e += [f"i {op} v64", f"u64 {op} j", f"i8 {op} v64", f"u64 {op} j32", f"i8 {op} v8", f"u32 {op} j", f"x {op} g",
              f"f {op} j", f"x {op} v64", f"u64 {op} y"]
        e += [f"x {op} {c}" for c in ("0.1", "0.7")] + [f"f {op} {c}" for c in ("0.1", "0.3", "0.7")]
        e += [f"0.1 {op} f", f"i32 {op} 2.5", f"u64 {op} 0.5", f"i {op} 9007199254740993.0", f"f {op} 16777217",
              f"f {op} 1", f"b {op} 1", f"b {op} c"]
        # Python ints outside the column's dtype: numpy 2 answers as for exact integers
        e += [f"u8 {op} 300", f"u8 {op} -1", f"i8 {op} 200", f"i8 {op} -129", f"u64 {op} -1", f"-1 {op} u64",
              f"i {op} 9223372036854775808", f"i {op} 18446744073709551615", f"18446744073709551615 {op} i",
              f"u64 {op} 18446744073709551615", f"u64 {op} 9223372036854775808", f"i32 {op} 4294967296",
              f"u32 {op} -4294967296", f"i16 {op} 9223372036854775808", f"u64 {op} 9223372036854775807"]
    # logic, where, minimum / maximum, predicates
    e += ["b & c", "b | c", "b ^ c", "~b", "b and c", "b or c", "not b", "(x > 0) and (y < 1) or not c",
          "0 < x < 1", "-1 <= f <= 0.1", "0 < i <= v64", "0.1 <= f < 0.7", "where(b, x, y)", "where(b, f, i8)",
          "where(b, i8, j32)", "where(c, u8, j8)", "where(b, u64, j)", "where(b, f, 0.1)", "where(b, 0.3, g)",
          "where(x > y, i, 3)", "where(b, b, c)", "where(b, u64, 7)", "where(f > 0.1, f, 0.1)",
          "minimum(x, y)", "maximum(x, y)", "minimum(f, g)", "maximum(f, g)", "minimum(f, 0.1)", "maximum(0.7, f)",
          "minimum(x, 0.0)", "maximum(x, -0.0)", "minimum(f, j8)", "maximum(u64, j)", "minimum(x, g)"]
    for p in expr.PREDICATES:
        e += [f"{p}(x)", f"{p}(f)", f"{p}(i)", f"{p}(u8)", f"{p}(x / y)"]
    # astype between every pair of kinds (float -> int from the columns built for it)
    kinds = ["float64", "float32", "int64", "int32", "int16", "int8", "uint64", "uint32", "uint16", "uint8", "bool"]
    for src in ["x", "f", "i", "i32", "i8", "u64", "u32", "u8", "b"]:
        e += [f"astype({src}, '{k}')" for k in kinds if k.startswith(("f", "b"))]
    for src in ["i", "i32", "i16", "i8", "u64", "u32", "u16", "u8", "b"]:
        e += [f"astype({src}, '{k}')" for k in kinds if k[0] in "iu"]
    e += [f"astype({src}, '{k}')" for src in ("xs", "fs") for k in kinds if k.startswith("int")]
    e += [f"astype(abs({src}), '{k}')" for src in ("xs", "fs") for k in kinds if k.startswith("uint")]
    e += ["astype(abs(xs) * 1e17, 'uint64')", "astype(xs * 7e16, 'int64')", "astype(astype(i, 'float32'), 'float64') + x",
          "astype(u64, 'float32') * 2", "astype(x * 0, 'bool')", "astype(i8, 'bool') & b"]
    # the exact functions
    for fn in ("sqrt", "floor", "ceil", "trunc", "rint", "abs", "fabs"):
        e += [f"{fn}(x)", f"{fn}(f)"]
    e += ["sqrt(i)", "sqrt(u64)", "sqrt(i16)", "fabs(i)", "fabs(i16)", "np.floor(x) + 1", "-x", "-f",
          "x + np.pi", "f * np.e", "where(isnan(x), inf, x)", "x + nan", "x != x", "f == f",
          # a constant cast by astype is a numpy scalar of that dtype: strong, not a weak Python scalar
          "f + astype(0.1, 'float64')", "f * astype(0.1, 'float32')", "i8 + astype(1, 'int32')", "u8 > astype(3, 'int64')",
          "x + astype(0.1, 'float32')", "where(b, f, astype(2, 'int64'))"]
    return list(dict.fromkeys(e))


_MATH = [k for k in expr.FUNCTIONS if k not in ("sqrt", "floor", "ceil", "trunc", "rint")]


def _ulp64():
    e = [f"{fn}(x)" for fn in _MATH] + ["x ** y", "arctan2(x, y)", "x ** 1.7", "x ** 3", "2.0 ** x", "exp(i32)",
                                        "log(u64)", "arctan2(i, v64)", "i ** 0.3", "sin(x) * cos(y)", "x ** j8"]
    # ** beside the other arithmetic: float32 against wider integer columns is float64 (I2F / U2F)
    e += ["f ** j32", "f ** j", "f ** v64", "j ** f", "v64 ** f", "x ** 0.1", "x ** 0.7", "x ** g", "0.1 ** x"]
    return e


def _ulp32():
    """(expression, the same in float64 over the float32 inputs): one float32 function node."""
    w = float(np.float32(1.7))
    e = [(f"{fn}(f)", f"{fn}(F)") for fn in _MATH]
    e += [("f ** g", "F ** G"), ("arctan2(f, g)", "arctan2(F, G)"), ("f ** 1.7", f"F ** {w!r}"), ("f ** 3", "F ** 3.0"),
          ("arctan2(f, 0.3)", f"arctan2(F, {float(np.float32(0.3))!r})"), ("exp(i16)", "exp(I16)"),
          ("f ** j16", "F ** J16"), ("f ** j8", "F ** J8"), ("j8 ** f", "J8 ** F")]
    e += [(f"f ** {c}", f"F ** {float(np.float32(c))!r}") for c in ("0.1", "0.3", "0.7")]
    e += [("0.3 ** f", f"{float(np.float32(0.3))!r} ** F")]
    return e


EXACT = _exact()
ULP64 = _ulp64()
ULP32 = _ulp32()
ALL = EXACT + ULP64 + [e for e, _ in ULP32]

# comparison terms, T (& T)* or T (| T)*, optionally negated: k_expr_terms
TERMS = [
    "u8 > 200", "i8 < -3", "b == 1", "u8 > 300", "i8 == 200",                      # 1-byte columns
    "i16 >= -32768", "u16 < 65535", "(i16 > 0) | (u16 == 7)",                        # 2-byte
    "f > 0.1", "f == 0.1", "f <= 0.3", "g != 0.7", "i32 > 2.5", "u32 >= 4294967295", "f >= 16777217",  # 4-byte, ucon / ucol
    "x > 0.1", "x != 0.5", "i < 9007199254740993", "i == 4611686018427387905", "u64 > 9223372036854775807",
    "u64 >= 9223372036854775813", "u64 == 18446744073709551615", "u64 < 0.5", "i > 9007199254740993.0",  # 8-byte
    # a conversion after the constant (the ucon slot): only a constant cast by astype still has one
    "x > astype(3, 'int64')", "f <= astype(2, 'int64')", "(y < astype(7, 'uint64')) & (i32 > astype(1, 'int8'))",
    "(x > 0.3) & (f < 0.7)", "(x > 0.3) | (i32 == 3)", "~(y <= 2)", "~((f > 0.1) | (u64 > 5))",
    "(i >= -20) & (i < 30) & (u8 > 1)",
    "(x > 0) & (f >= 0.1) & (i > -5) & (i32 < 7) & (i16 != 3) & (i8 <= 1) & (u64 > 0) & (u16 < 65535)",  # 8 terms
    "(x > 0) | (f >= 0.1) | (i > 5) | (i32 < -7) | (i16 == 3) | (i8 <= -100) | (u64 > 9223372036854775808) | (u8 == 255)",
]

# refused with UnsupportedExpression (numpy raises, or wraps silently in np.where)
REFUSED = ["u8 + 300", "300 + u8", "i8 * 200", "u8 - (-1)", "minimum(u8, 300)", "maximum(-1, u64)", "u64 + (-1)",
           "where(b, u8, 300)", "u8 >> 300", "u64 & -1", "i8 ** 200", "u64 >> j", "u64 & j", "b < 9223372036854775808",
           "sqrt(i8)", "arctan2(i8, j8)", "astype(x, 'float16')", "i ** -1", "f + 1180591620717411303424", "fmin(x, y)", "~x",
           "floor(i32)"]  # numpy returns the integers unchanged; not a device function of integers


def namespace(columns):
    ns = dict(np=np, nan=np.nan, inf=np.inf, astype=lambda a, d: np.asarray(a).astype(d), abs=np.abs,
              absolute=np.abs, fabs=np.fabs, minimum=np.minimum, maximum=np.maximum, where=np.where,
              arctan2=np.arctan2)
    ns.update({k: v[0] for k, v in expr.FUNCTIONS.items()})
    ns.update({k: v[0] for k, v in expr.PREDICATES.items()})
    ns.update(columns)
    return ns


def numpy_eval(e, columns):
    """numpy's own evaluation of ``e`` (and / or / not as the element-wise operations)."""
    import ast

    class Logic(ast.NodeTransformer):
        def visit_BoolOp(self, node):
            self.generic_visit(node)
            out = node.values[0]
            for v in node.values[1:]:
                out = ast.BinOp(out, ast.BitAnd() if isinstance(node.op, ast.And) else ast.BitOr(), v)
            return out

        def visit_UnaryOp(self, node):
            self.generic_visit(node)
            return ast.UnaryOp(ast.Invert(), node.operand) if isinstance(node.op, ast.Not) else node

        def visit_Compare(self, node):
            self.generic_visit(node)
            left, out = node.left, None
            for op, right in zip(node.ops, node.comparators):
                t = ast.Compare(left, [op], [right])
                out = t if out is None else ast.BinOp(out, ast.BitAnd(), t)
                left = right
            return out

    tree = ast.fix_missing_locations(Logic().visit(ast.parse(e, mode="eval")))
    with np.errstate(all="ignore"):
        v = eval(compile(tree, "<expr>", "eval"), {"__builtins__": {}}, namespace(columns))  # noqa: S307
    v = np.asarray(v)
    n = len(next(iter(columns.values())))
    return np.broadcast_to(v, (n,)) if v.ndim == 0 else v


def reference(e, columns):
    """(expected, rule): rule 'exact', or the ulp bound for the finite, non-zero rows."""
    for e32, e64 in ULP32:
        if e == e32:
            up = {k: (v.astype(np.float64) if v.dtype.kind in "fiu" else v) for k, v in columns.items()}
            ns = {k.upper(): v for k, v in up.items()}
            with np.errstate(all="ignore"):
                v = eval(e64, {"__builtins__": {}}, namespace(ns))  # noqa: S307
                return np.asarray(v, np.float64).astype(np.float32), 1
    return numpy_eval(e, columns), (4 if e in ULP64 else "exact")


def _bits(a):
    return a.view(np.dtype(f"u{a.dtype.itemsize}"))


def check(e, got, columns, dtype=None, ulp=None):
    """The comparison rule: numpy's dtype; bit for bit (NaN matches NaN, the sign of zero
    counts) except for the finite non-zero results of transcendental functions, which keep
    an ulp bound (4 for float64; 1 for one float32 node against the float64 evaluation of the
    float32 inputs rounded once)."""
    expected, rule = reference(e, columns)
    if ulp is not None:  # a transcendental expression outside the lists
        rule = ulp
    got = np.asarray(got)
    assert (dtype or got.dtype) == expected.dtype, (e, dtype or got.dtype, expected.dtype)
    assert got.dtype == expected.dtype and got.shape == expected.shape, (e, got.dtype, got.shape)
    expected = np.ascontiguousarray(expected)
    if expected.dtype.kind != "f":
        bad = np.flatnonzero(_bits(got) != _bits(expected))
    else:
        nan_e, nan_g = np.isnan(expected), np.isnan(got)
        same = (_bits(got) == _bits(expected)) | (nan_e & nan_g)
        if rule != "exact":
            special = nan_e | np.isinf(expected) | (expected == 0)  # fixed by IEEE 754 / C Annex F: exact
            # ordered integer images of the floats (Python ints: no overflow): the distance in ulp
            it = np.dtype(f"i{got.dtype.itemsize}")
            sign = int(np.iinfo(it).min)

            def order(a):
                return np.array([sign - v if v < 0 else v for v in a.view(it).tolist()], object)
            close = np.array([abs(d) <= rule for d in order(got) - order(expected)], bool)
            same = same | (~special & np.isfinite(got) & close)
        bad = np.flatnonzero(~same)
    if len(bad):
        r = bad[:5]
        used = [k for k in columns if k in e.replace("'", " ").replace("(", " ").replace(")", " ").replace(",", " ").split()]
        raise AssertionError(f"{e}: {len(bad)} of {len(got)} rows differ; rows {r.tolist()}: got {got[r]!r}, "
                             f"expected {expected[r]!r}, inputs { {k: columns[k][r] for k in used} }")
