"""The rule for missing values on HBM frames, restated in numpy.

A missing mask is one bool per row, True = missing.  The value of an expression is what the
unmasked expression computes on the data (``expr_np``'s namespace); its mask is the OR of the
masks of the masked columns the expression reads, with these special cases:

* ``where(c, a, b)`` is missing where ``c`` is, and otherwise where the chosen branch is;
* ``ismissing / notmissing / isna / notna`` and ``isnan`` are never missing (``isnan`` is False at
  missing rows); ``fillmissing / fillna`` are never missing; ``fillnan`` keeps its argument's mask.

This is deliberately not ``np.ma``: no domain masks (``x / 0``, ``log(0)`` ...), and ``where``
keeps masks.  tests/test_missing_np.py checks the restatement against ``np.ma`` where the two
agree.  The data under a missing row is unspecified: compare with :func:`check`."""
import ast
import functools

import numpy as np

import expr_np

N = expr_np.N
MASK_KINDS = ("valid", "missing", "mixed")


def mask_of(kind, n=N, shift=0):
    """all valid; all missing; a pattern of period 3 XOR period 7, so that 8-row words mix"""
    r = np.arange(n) + shift
    if kind == "valid":
        return np.zeros(n, bool)
    if kind == "missing":
        return np.ones(n, bool)
    return (r % 3 == 0) ^ (r % 7 < 2)


@functools.lru_cache(maxsize=None)
def edge_columns(kind="mixed"):
    """name -> np.ma array: every column of ``expr_np.edge_columns()`` with a mask of ``kind``
    (the mixed pattern is shifted per column, so two columns of an expression differ)."""
    out = {}
    for k, (name, col) in enumerate(expr_np.edge_columns().items()):
        m = np.ma.array(col, mask=mask_of(kind, len(col), shift=k), shrink=False)
        out[name] = m
    return out


def _or(*masks):
    out = None
    for m in masks:
        if m is not None:
            out = m.copy() if out is None else (out | m)
    return out


_SPECIAL = ("where", "ismissing", "notmissing", "isna", "notna", "isnan", "fillmissing", "fillnan", "fillna")


def evaluate(e, columns):
    """(data, mask) of the expression ``e`` over ``columns`` (name -> numpy or np.ma array) by the
    rule above; mask is a bool array, or None for a result that is never missing."""
    n = len(next(iter(columns.values())))
    data = {k: np.ma.getdata(v) for k, v in columns.items()}
    masks = {k: np.ma.getmaskarray(v) for k, v in columns.items() if np.ma.isMaskedArray(v)}

    def plain(node):
        """a tree without special calls: numpy's value on the data, the OR of the masks it reads"""
        v = np.asarray(expr_np.numpy_eval(ast.unparse(node), data))
        names = [x.id for x in ast.walk(node) if isinstance(x, ast.Name)]
        return np.broadcast_to(v, (n,)), _or(*[masks.get(k) for k in names])

    def fill(x, cond, v):
        out = np.array(x, copy=True)
        out[cond] = v  # numpy's assignment conversion
        return out

    class Special(ast.NodeTransformer):
        """bottom-up: every special call becomes a temporary column holding its value and mask"""

        def visit_Call(self, node):
            self.generic_visit(node)
            name = node.func.id if isinstance(node.func, ast.Name) else None
            if name not in _SPECIAL:
                return node
            args = [plain(a) for a in node.args[:1 if name != "where" else 3]]
            if name == "where":
                (c, mc), (a, ma), (b, mb) = args
                d = plain(node)[0]  # numpy's own where on the data (its dtype rules)
                chosen = np.where(c, False if ma is None else ma, False if mb is None else mb)
                m = None if (mc is None and ma is None and mb is None) else (chosen | (False if mc is None else mc))
            else:
                x, mx = args[0]
                miss = mx if mx is not None else np.zeros(n, bool)
                nan = (x != x) & ~miss if x.dtype.kind == "f" else np.zeros(n, bool)
                m = None
                if name in ("fillmissing", "fillnan", "fillna"):
                    v = ast.literal_eval(node.args[1])
                    cond = {"fillmissing": miss, "fillnan": nan, "fillna": nan | miss}[name]
                    d = fill(x, cond, v) if (name != "fillnan" or x.dtype.kind == "f") else x
                    m = mx if name == "fillnan" else None
                else:
                    d = {"ismissing": miss.copy(), "notmissing": ~miss, "isnan": nan, "isna": nan | miss,
                         "notna": ~(nan | miss)}[name]
            key = f"_t{len(data)}"
            data[key] = np.ascontiguousarray(d)
            if m is not None:
                masks[key] = np.asarray(m, bool)
            return ast.copy_location(ast.Name(id=key, ctx=ast.Load()), node)

    tree = ast.fix_missing_locations(Special().visit(ast.parse(e, mode="eval")))
    return plain(tree.body)


def check(e, got_data, got_mask, columns, ulp=None):
    """``got`` against the rule: the masks exactly equal, the data equal at the valid rows by
    ``expr_np.check``'s rule (bit for bit; transcendental functions within their ulp bound)."""
    want_data, want_mask = evaluate(e, columns)
    if want_mask is None:
        assert got_mask is None, (e, "a result that is never missing came back masked")
        valid = np.ones(len(want_data), bool)
    else:
        assert got_mask is not None, (e, "the mask was dropped")
        got_mask = np.asarray(got_mask, bool)
        assert np.array_equal(got_mask, want_mask), (e, np.flatnonzero(got_mask != want_mask)[:5])
        valid = ~want_mask
    got_data = np.asarray(got_data)
    assert got_data.dtype == want_data.dtype, (e, got_data.dtype, want_data.dtype)
    g, w = got_data[valid], np.ascontiguousarray(want_data[valid])
    if w.dtype.kind == "f":
        same = (g.view(f"u{w.itemsize}") == w.view(f"u{w.itemsize}")) | (np.isnan(g) & np.isnan(w))
        if ulp:
            it = np.dtype(f"i{w.itemsize}")
            close = np.abs(g.view(it).astype(np.float64) - w.view(it).astype(np.float64)) <= ulp
            same |= np.isfinite(w) & (w != 0) & np.isfinite(g) & close & (np.sign(g) == np.sign(w))
    else:
        same = g == w
    bad = np.flatnonzero(~same)
    assert not len(bad), (e, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


# the operators np.ma agrees with (on columns in [1, 100]: no domain masks) -- and the device list
OPERATORS = ["a + b", "a - b", "a * b", "a < b", "a <= b", "a == b", "a != b", "-a", "abs(a)", "minimum(a, b)",
             "maximum(a, b)", "p & q", "p | q", "~p", "floor(x)", "a + u", "x * a + b", "(a < b) & p"]
# Python constants and a division: np.ma promotes the constant as an array (int64) and divides with
# a domain mask, so these are compared with the rule alone
CONSTANTS = ["a + 1", "x / 2", "x > 50.5", "b // 3", "sqrt(x)", "a % 7 == 0"]
WHERES = ["where(p, a, b)", "where(a < b, x, 1.5)", "where(q, a, u)", "where(p & q, 2, b)"]
FUNCTIONS = ["ismissing(a)", "notmissing(x)", "ismissing(u)", "ismissing(a + b)", "isnan(x)", "isnan(a)", "isna(x)",
             "notna(x)", "isna(a)", "notna(u + 1)", "fillmissing(a, 7)", "fillmissing(x, 1.5)", "fillmissing(u, 3)",
             "fillmissing(p, True)", "fillnan(x, 2.0)", "fillnan(a, 2)", "fillna(x, -1.0)", "fillna(a, 0)",
             "isfinite(x)", "isinf(x)", "fillmissing(a + b, 0) * 2", "where(ismissing(a), b, a)"]


def small_columns(kind="mixed", n=N, nan=True):
    """a b (int32 / int64 in [1, 100]), x (float64 in [1, 100]; nan: NaN in every 11th row, under
    valid and missing rows), p q (bool): masked; u (int32): unmasked"""
    rng = np.random.default_rng(7)
    x = rng.uniform(1, 100, n)
    if nan:
        x[::11] = np.nan
    cols = {
        "a": np.ma.array(rng.integers(1, 100, n).astype(np.int32), mask=mask_of(kind, n, 0), shrink=False),
        "b": np.ma.array(rng.integers(1, 100, n).astype(np.int64), mask=mask_of(kind, n, 1), shrink=False),
        "x": np.ma.array(x, mask=mask_of(kind, n, 2), shrink=False),
        "p": np.ma.array(rng.random(n) < 0.5, mask=mask_of(kind, n, 3), shrink=False),
        "q": np.ma.array(rng.random(n) < 0.5, mask=mask_of(kind, n, 4), shrink=False),
        "u": rng.integers(1, 100, n).astype(np.int32),
    }
    return cols
