"""Device evaluation of vaex expressions over HBM columns (``vh_expr_eval``, csrc/expr.hip).

The reference evaluates virtual columns, selections and filters with numpy, chunk by chunk
(``dataframe.py`` ``evaluate``, ``cpu.py:542-581``, ``execution.py:337-341``).  For a
DataFrame whose columns live in HBM this module compiles the expression once into a small
stack program and evaluates it with one HIP kernel per chunk, writing a new HBM column
(or a uint8 mask for selections / filters) -- no host round trip.

Semantics follow numpy 2: the result dtype of every node is numpy's own (found by running
the numpy operation on empty arrays / Python scalars, so NEP 50 weak scalars hold: a Python
constant in a float32 node is converted to float32 before the operation), float32 nodes
are rounded to float32 after each operation (``//`` and ``%`` run in float32) and narrow
integer nodes wrap, like numpy's; uint64 nodes run unsigned operations, integers of any two
dtypes compare exactly (int64 against uint64, a Python int outside the column's dtype), and
a 64-bit integer becomes float32 in one rounding.  Everything but the transcendental
functions is numpy's result bit for bit; those are within 4 ulp in float64 (a float32 node:
the float64 result rounded once), exact where the result is NaN, infinite or zero
(tests/expr_np.py).  Undefined in numpy and not pinned: float -> integer
casts of NaN, infinities or values outside the target type, negative shift counts, integer
``**`` with a negative exponent in a column.

Missing values: a masked HBM column (``device.DeviceMaskedArray``) binds its data and its mask
(a bool column, 1 = missing).  Every node carries an optional mask program over the same inputs:
a result is missing where a masked input the node reads is, ``where`` follows the chosen branch,
and ``ismissing / notmissing / isna / notna / isnan / fillmissing / fillnan / fillna`` consume
masks (:data:`MISSING_FUNCTIONS`).  ``Program.mask_code`` is that program (None: never missing);
a boolean compiled as a row mask (``keep``) is ``value & ~mask``.  No domain masks are added and
``where`` keeps masks: this is not ``np.ma``.

Supported: columns, virtual columns, variables, Python int / float / bool
constants, ``+ - * / // % **``, unary ``- ~``, comparisons (chained too), ``& | ^ << >>``,
``and / or / not`` on booleans, and the functions in :data:`FUNCTIONS` (also as ``np.f``).
Anything else raises :class:`UnsupportedExpression`, which callers turn into the host path
or an error (there is no silent fallback for HBM columns); so does what numpy itself refuses
(a Python int outside the dtype in arithmetic, ``minimum`` / ``maximum``, shifts or
``where``; dtype pairs without a loop), integers beyond 64 bits and float16 results.
"""
import ast
import ctypes

import numpy as np

from . import _lib

# opcodes (csrc/expr.hip)
OP = dict(COL=0, CONST=1, I2F=2, F2I=3, ROUND_F32=4, WRAP=5, U2F=6, I2F32=7, U2F32=8, F2U=9,
          ADD_F=10, SUB_F=11, MUL_F=12, DIV_F=13, FLOORDIV_F=14, MOD_F=15, POW_F=16, NEG_F=17, ABS_F=18,
          MIN_F=19, MAX_F=20, ARCTAN2=21, FLOORDIV_F32=22, MOD_F32=23,
          ADD_I=30, SUB_I=31, MUL_I=32, FLOORDIV_I=33, MOD_I=34, NEG_I=35, ABS_I=36, AND_I=37, OR_I=38,
          XOR_I=39, INV_I=40, MIN_I=41, MAX_I=42, SHL_I=43, SHR_I=44, POW_I=45,
          LT_F=50, LE_F=51, GT_F=52, GE_F=53, EQ_F=54, NE_F=55,
          LT_I=60, LE_I=61, GT_I=62, GE_I=63, EQ_I=64, NE_I=65, LT_U=66, LE_U=67, GT_U=68, GE_U=69,
          NOT_B=70,
          SQRT=80, EXP=81, LOG=82, LOG10=83, SIN=84, COS=85, TAN=86, ARCSIN=87, ARCCOS=88, ARCTAN=89,
          SINH=90, COSH=91, TANH=92, FLOOR=93, CEIL=94, ISNAN=95, ISFINITE=96, ISINF=97, LOG1P=98, EXPM1=99,
          LOG2=100, EXP2=101, TRUNC=102, RINT=103,
          WHERE=110,
          FLOORDIV_U=120, MOD_U=121, MIN_U=122, MAX_U=123, SHR_U=124, POW_U=125)
# datetime64 / timedelta64 opcodes (the second enum of csrc/expr.hip; unary, an immediate each)
DT_OP = dict(DT_FIELD=104, DT_CAST=105, TD_FIELD=106)
# the opcodes that pop two slots and push one (expr.hip is_binary)
BINARY = frozenset(OP[k] for k in (
    "ADD_F SUB_F MUL_F DIV_F FLOORDIV_F MOD_F POW_F MIN_F MAX_F ARCTAN2 FLOORDIV_F32 MOD_F32 "
    "ADD_I SUB_I MUL_I FLOORDIV_I MOD_I AND_I OR_I XOR_I MIN_I MAX_I SHL_I SHR_I POW_I "
    "LT_F LE_F GT_F GE_F EQ_F NE_F LT_I LE_I GT_I GE_I EQ_I NE_I LT_U LE_U GT_U GE_U "
    "FLOORDIV_U MOD_U MIN_U MAX_U SHR_U POW_U").split())
MAX_CODE, MAX_CONST, MAX_COLS, MAX_DEPTH = 128, 32, 16, 8

# float -> float functions (numpy ufunc, opcode)
FUNCTIONS = {
    "sqrt": (np.sqrt, "SQRT"), "exp": (np.exp, "EXP"), "log": (np.log, "LOG"), "log10": (np.log10, "LOG10"),
    "log2": (np.log2, "LOG2"), "exp2": (np.exp2, "EXP2"), "log1p": (np.log1p, "LOG1P"),
    "expm1": (np.expm1, "EXPM1"), "sin": (np.sin, "SIN"), "cos": (np.cos, "COS"), "tan": (np.tan, "TAN"),
    "arcsin": (np.arcsin, "ARCSIN"), "arccos": (np.arccos, "ARCCOS"), "arctan": (np.arctan, "ARCTAN"),
    "sinh": (np.sinh, "SINH"), "cosh": (np.cosh, "COSH"), "tanh": (np.tanh, "TANH"),
    "floor": (np.floor, "FLOOR"), "ceil": (np.ceil, "CEIL"), "trunc": (np.trunc, "TRUNC"), "rint": (np.rint, "RINT"),
}
PREDICATES = {"isnan": (np.isnan, "ISNAN"), "isfinite": (np.isfinite, "ISFINITE"), "isinf": (np.isinf, "ISINF")}


# datetime64 / timedelta64 (csrc/datetime_dev.hpp mirrors these numbers): the units, the dt_*
# fields (int32, is_leap_year bool: pandas 2's dtypes) and the td_* fields
DT_UNITS = ["ns", "us", "ms", "s", "m", "h", "D", "W", "M", "Y"]
DT_FIELD_UNITS = DT_UNITS[:7]  # field functions take these; coarser columns are cast first
DT_FIELDS = ["year", "month", "day", "dayofweek", "dayofyear", "quarter", "halfyear", "hour", "minute", "second",
             "is_leap_year", "weekofyear"]
TD_FIELDS = {"days": (0, np.int64), "seconds": (1, np.int32), "microseconds": (2, np.int32),
             "nanoseconds": (3, np.int32), "total_seconds": (4, np.float64)}
INT64_MIN = -(1 << 63)  # NaT


class UnsupportedExpression(ValueError):
    pass


def _unit(dt):
    """the index of a datetime64 / timedelta64 dtype's unit in DT_UNITS"""
    unit, count = np.datetime_data(dt)
    if count != 1 or unit not in DT_UNITS:
        raise UnsupportedExpression(f"dtype {dt}: units are {', '.join(DT_UNITS)}")
    return DT_UNITS.index(unit)


def column_has_nat(col):
    """Whether a datetime64 / timedelta64 column holds NaT (INT64_MIN).  An HBM column answers
    from the device min / max pass over its int64 bits; that pass reports float64, in which the
    512 values from INT64_MIN up are one number, so a minimum that low is settled exactly by a
    device `== INT64_MIN` mask and its maximum."""
    from .device import DeviceArray, DeviceMaskedArray
    if isinstance(col, DeviceMaskedArray):
        col = col.data  # NaT is not a mask: one under a missing row refuses the column as well
    if not isinstance(col, DeviceArray):
        return bool(np.isnat(np.asarray(col)).any())
    n = len(col)
    if n == 0:
        return False
    lo, hi = ctypes.c_double(), ctypes.c_double()
    code = _lib.DTYPE_CODE["int64"]
    _lib.call("vh_minmax", col.ptr, n, code, 0, None, _lib.LOC_DEVICE, ctypes.byref(lo), ctypes.byref(hi))
    if lo.value > float(INT64_MIN):
        return False
    mask = DeviceArray.empty(n, np.uint8)
    prog = (ctypes.c_uint32 * 3)(OP["COL"], OP["CONST"], OP["EQ_I"])
    _lib.call("vh_expr_eval", prog, 3, (ctypes.c_uint64 * 1)(1 << 63), 1, (ctypes.c_void_p * 1)(col.ptr),
              (ctypes.c_int * 1)(code), 1, n, _lib.DTYPE_CODE["uint8"], mask.ptr)
    _lib.call("vh_minmax", mask.ptr, n, _lib.DTYPE_CODE["uint8"], 0, None, _lib.LOC_DEVICE, ctypes.byref(lo),
              ctypes.byref(hi))
    return hi.value > 0


class _Typed:
    """A compiled sub-expression: its code and numpy dtype (or a Python scalar for a
    constant, which numpy 2 promotes as a weak scalar)."""

    def __init__(self, code, dtype, scalar=None, mask=None, own_mask=False):
        self.code = code
        self.dtype = np.dtype(dtype)
        self.scalar = scalar  # the Python value of a constant leaf
        # the mask program: None (never missing), or the distinct bool sub-programs (tuples of
        # instructions over the same inputs) whose OR is 1 on the rows where the value is missing
        self.mask = mask
        self.own_mask = own_mask  # the node set its mask itself (where, the mask consumers)

    @property
    def proto(self):
        """What numpy sees for type resolution: the Python scalar or an empty array."""
        return self.scalar if self.scalar is not None else np.empty(0, self.dtype)


def _kind(dt):
    return "f" if dt.kind == "f" else ("u" if dt.kind == "u" else ("b" if dt.kind == "b" else "i"))


# the functions that consume masks (the reference's functions.py:146-268): name -> arguments
MISSING_FUNCTIONS = {"ismissing": 1, "notmissing": 1, "isna": 1, "notna": 1, "fillmissing": 2, "fillnan": 2, "fillna": 2}


def _mask_or(*masks):
    """the OR of mask programs: their distinct terms in order of first use, None for none"""
    out = []
    for m in masks:
        for term in m or ():
            if term not in out:
                out.append(term)
    return tuple(out) or None


def _mask_code(mask):
    """the instructions of a mask program: its terms joined by OR_I"""
    code = []
    for k, term in enumerate(mask):
        code += list(term) + ([OP["OR_I"]] if k else [])
    return code


class Compiler:
    def __init__(self, df):
        self.df = df
        self.columns = []      # column names in slot order
        self.consts = []       # uint64 bit patterns
        self._depth = 0
        self._masks = {}       # id(ast node) -> (node, mask program) of every node visited

    # ---- leaves -------------------------------------------------------------------
    def _const(self, value):
        if isinstance(value, bool):
            bits, dt = int(value), np.bool_
        elif isinstance(value, (int, np.integer)) and not isinstance(value, np.timedelta64):
            value = int(value)
            if not -(1 << 63) <= value < (1 << 64):
                raise UnsupportedExpression("integer constant out of 64-bit range")
            bits, dt = value & 0xFFFFFFFFFFFFFFFF, np.int64
        elif isinstance(value, (float, np.floating)):
            bits, dt = int(np.array(float(value)).view(np.uint64)), np.float64
        elif isinstance(value, (np.datetime64, np.timedelta64)):
            if np.isnat(value):
                raise UnsupportedExpression("a NaT constant")
            _unit(value.dtype)
            bits = int(value.astype(np.int64)) & 0xFFFFFFFFFFFFFFFF
            if bits not in self.consts:
                self.consts.append(bits)
            # a numpy scalar with a unit: strong in promotion, converted on the host by _to_unit
            return _Typed([OP["CONST"] | self.consts.index(bits) << 8], value.dtype, scalar=value)
        else:
            raise UnsupportedExpression(f"constant {value!r}")
        # the pool may hold constants that no instruction uses in the end (a weak scalar is
        # re-pushed in the node's dtype): Program drops those and checks MAX_CONST
        if bits not in self.consts:
            self.consts.append(bits)
        idx = self.consts.index(bits)
        return _Typed([OP["CONST"] | idx << 8], dt, scalar=value if not isinstance(value, np.generic) else value.item())

    def _string_column(self, node):
        """the name of the string column (strings.DeviceStringArray) an ast node names, else None"""
        from .strings import DeviceStringArray
        if isinstance(node, ast.Name) and isinstance(self.df.columns.get(node.id), DeviceStringArray):
            return node.id
        return None

    def _string_source(self, node, depth=0):
        """The plan of a string-valued ast node, else None.  String-valued: a string column's
        name, a virtual column whose expression is string-valued, a transform call
        (``strings.TRANSFORMS``) whose first argument is string-valued, and ``+`` with a
        string-valued side (``str_cat``).  A plan is ``("col", name)`` or ``("fn", method, plan,
        args, kwargs)`` for a ``DeviceStringArray`` method, hashable; :func:`evaluate_string`
        computes it for a row range."""
        from . import strings
        if depth > 32:
            raise UnsupportedExpression("string expression too deeply nested")
        if isinstance(node, ast.Expression):
            return self._string_source(node.body, depth)
        if isinstance(node, ast.Name):
            if self._string_column(node):
                return ("col", node.id)
            if node.id not in self.df.columns and node.id in self.df.virtual_columns:
                try:
                    tree = ast.parse(self.df.virtual_columns[node.id], mode="eval")
                except SyntaxError as e:
                    raise UnsupportedExpression(str(e))
                return self._string_source(tree, depth + 1)
            return None
        if isinstance(node, ast.BinOp) and isinstance(node.op, ast.Add):
            a, b = node.left, node.right
            lit_a = isinstance(a, ast.Constant) and isinstance(a.value, str)
            lit_b = isinstance(b, ast.Constant) and isinstance(b.value, str)
            sa = None if lit_a else self._string_source(a, depth + 1)
            sb = None if lit_b else self._string_source(b, depth + 1)
            if sa is None and sb is None:
                return None
            if sa is not None and sb is not None:
                return self._transform_plan("cat", sa, (("plan", sb),), {})
            if sa is not None and lit_b:
                return self._transform_plan("cat", sa, (b.value,), {})
            if sb is not None and lit_a:
                return self._transform_plan("cat", sb, (a.value,), {"first": True})
            raise UnsupportedExpression("+ of a string expression takes a str constant or a string expression")
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in strings.TRANSFORMS:
            name = node.func.id
            args = list(node.args)
            kwargs = {}
            if name == "str_cat" and len(args) == 2 and isinstance(args[0], ast.Constant) and isinstance(args[0].value, str):
                args = [args[1], args[0]]  # the reference's form of 'lit' + s: str_cat('lit', s)
                kwargs["first"] = True
            src = self._string_source(args[0], depth + 1) if args else None
            if src is None:
                raise UnsupportedExpression(f"{name} takes a string column or a string-valued expression")
            values = []
            for a in args[1:]:
                other = self._string_source(a, depth + 1) if name == "str_cat" and not isinstance(a, ast.Constant) else None
                values.append(("plan", other) if other is not None else self._literal(name, a))
            for k in node.keywords:
                if k.arg is None or k.arg == "first":
                    raise UnsupportedExpression(f"{name}: keyword arguments by name")
                kwargs[k.arg] = self._literal(name, k.value)
            return self._transform_plan(strings.TRANSFORMS[name], src, tuple(values), kwargs, name)
        return None

    @staticmethod
    def _literal(name, node):
        try:
            v = ast.literal_eval(node)
        except (ValueError, TypeError, SyntaxError):
            raise UnsupportedExpression(f"{name}: arguments after the first are constants")
        if v is not None and not isinstance(v, (str, int, bool)):
            raise UnsupportedExpression(f"{name}: argument {v!r}")
        return v

    @staticmethod
    def _transform_plan(method, src, args, kwargs, name=None):
        """the plan of ``src.method(*args, **kwargs)``, the arguments checked now: a wrong
        signature is UnsupportedExpression; what the method itself refuses (a regular expression,
        a fill of two characters ...) raises its NotImplementedError / ValueError here"""
        from . import strings
        dry = [strings.COLUMN if isinstance(a, tuple) else a for a in args]
        try:
            strings.transform_arguments(method, *dry, **kwargs)
        except TypeError as e:
            raise UnsupportedExpression(f"{name or method}: {e}")
        return ("fn", method, src, args, tuple(sorted(kwargs.items())))

    def _string_input(self, fn, source, arg=None):
        """A string function of a string-valued source (``str_*``, strings.py) as one more input
        column of the program: the string kernel fills it for the rows [i1, i2) at evaluate time
        (Program.evaluate), a bool mask for the predicates, int64 for the lengths."""
        from . import strings
        if fn in strings.MATCH_OPS:
            if not isinstance(arg, str):
                raise UnsupportedExpression(f"{fn}: the pattern is a str constant")
            strings._pattern(arg)  # NotImplementedError past 1024 bytes
        key = ("str", fn, source, arg)
        if key not in self.columns:
            if len(self.columns) >= MAX_COLS:
                raise UnsupportedExpression("too many columns")
            self.columns.append(key)
        return _Typed([OP["COL"] | self.columns.index(key) << 8], np.int64 if fn in strings.LEN_KINDS else np.bool_)

    def _column(self, name):
        col = self.df.columns[name]
        if self._string_column(ast.Name(id=name)):
            raise UnsupportedExpression(f"string column {name!r}: strings compute through str_* functions and "
                                        "comparisons with a str constant")
        dt = np.dtype(col.dtype)
        if dt.kind not in "biufmM" or not dt.isnative:
            raise UnsupportedExpression(f"column {name!r} of dtype {dt}")
        if np.ma.isMaskedArray(col):
            raise UnsupportedExpression(f"masked column {name!r}")
        from .device import DeviceMaskedArray
        masked = isinstance(col, DeviceMaskedArray)
        if dt.kind in "mM":
            # a program has one result dtype and does plain int64 arithmetic: pandas answers NaT
            # rows with NaN, numpy propagates NaT, so only NaT-free columns compute here
            _unit(dt)
            if self.df._column_has_nat(name):
                raise UnsupportedExpression(f"column {name!r} holds NaT (not-a-time) values")
        if name not in self.columns:
            if len(self.columns) >= MAX_COLS:
                raise UnsupportedExpression("too many columns")
            self.columns.append(name)
        mask = None
        if masked:  # the mask is one more input: a bool column
            key = ("mask", name)
            if key not in self.columns:
                if len(self.columns) >= MAX_COLS:
                    raise UnsupportedExpression("too many columns")
                self.columns.append(key)
            mask = ((OP["COL"] | self.columns.index(key) << 8,),)
        return _Typed([OP["COL"] | self.columns.index(name) << 8], dt, mask=mask)

    # ---- conversions -----------------------------------------------------------------
    def _to_float(self, t, dt):
        """code leaving t's value as float64 bits, for an operand of a node that numpy
        computes in the float dtype ``dt``."""
        dt = np.dtype(dt)
        if t.scalar is not None:
            # a weak scalar (NEP 50) is converted to the node's dtype before the operation:
            # `f32 * 0.1` multiplies by float32(0.1).  numpy does the conversion itself here
            with np.errstate(all="ignore"):
                v = float((np.ones(1, dt) * t.scalar)[0])
            return list(self._const(v).code)
        k = _kind(t.dtype)
        if k == "f":
            return list(t.code)
        wide = t.dtype.itemsize == 8
        if dt == np.float32 and wide:  # one rounding, as (float)int64: not int -> double -> float
            return list(t.code) + [OP["U2F32" if k == "u" else "I2F32"]]
        return list(t.code) + [OP["U2F" if (k == "u" and wide) else "I2F"]]

    @staticmethod
    def _resolve(fn, *protos):
        """numpy's result dtype of ``fn(*protos)``; what numpy refuses is UnsupportedExpression
        (TypeError: no loop for the dtypes; OverflowError: a Python int outside the dtype)."""
        with np.errstate(all="ignore"):
            try:
                return np.result_type(fn(*protos))
            except (TypeError, OverflowError) as e:
                raise UnsupportedExpression(str(e))

    @staticmethod
    def _finish(code, dtype):
        """the node's own rounding / wrap-around (numpy computes in the result dtype)."""
        dtype = np.dtype(dtype)
        if dtype.kind == "f" and dtype.itemsize not in (4, 8):
            raise UnsupportedExpression(f"{dtype} result (numpy computes sqrt(int8), say, in float16)")
        if dtype == np.float32:
            return code + [OP["ROUND_F32"]]
        if dtype.kind in "iu" and dtype.itemsize < 8:
            return code + [OP["WRAP"] | ((dtype.itemsize * 8) | ((dtype.kind == "i") << 8)) << 8]
        return code

    # ---- nodes ---------------------------------------------------------------------
    def visit(self, node):
        m = getattr(self, "v_" + type(node).__name__, None)
        if m is None:
            raise UnsupportedExpression(f"unsupported syntax {type(node).__name__}")
        t = m(node)
        if not (t.own_mask or isinstance(node, (ast.Name, ast.Expression))):
            # propagation: missing where an operand the node reads is missing
            mask = _mask_or(*[self._masks[id(c)][1] for c in ast.iter_child_nodes(node) if id(c) in self._masks])
            if mask != t.mask:
                t = _Typed(t.code, t.dtype, t.scalar, mask)
        self._masks[id(node)] = (node, t.mask)
        return t

    def v_Expression(self, node):
        return self.visit(node.body)

    def v_Constant(self, node):
        return self._const(node.value)

    def v_Name(self, node):
        name = node.id
        if name in self.df.columns:
            return self._column(name)
        if name in self.df.virtual_columns:
            return self.visit(ast.parse(self.df.virtual_columns[name], mode="eval"))
        if name in self.df.variables:
            v = self.df.variables[name]
            if isinstance(v, (np.datetime64, np.timedelta64)):
                return self._const(v)
            if isinstance(v, (bool, int, float, np.integer, np.floating, np.bool_)):
                return self._const(v.item() if isinstance(v, np.generic) else v)
            raise UnsupportedExpression(f"variable {name!r} is not a scalar")
        if name in ("True", "False"):
            return self._const(name == "True")
        if name in ("nan", "inf"):
            return self._const(float(name))
        raise UnsupportedExpression(f"unknown name {name!r}")

    def v_Attribute(self, node):
        # np.nan, np.inf, np.pi, np.e
        if isinstance(node.value, ast.Name) and node.value.id in ("np", "numpy"):
            if node.attr in ("nan", "inf", "pi", "e"):
                return self._const(float(getattr(np, node.attr)))
        raise UnsupportedExpression("attribute access")

    def _arith(self, opname, a, b):
        ufunc = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.true_divide, "//": np.floor_divide,
                 "%": np.remainder, "**": np.power}[opname]
        dt = self._resolve(ufunc, a.proto, b.proto)
        if a.scalar is not None and b.scalar is not None:
            with np.errstate(all="ignore"):
                v = ufunc(a.scalar, b.scalar)
            if isinstance(v, (np.datetime64, np.timedelta64)):
                return self._const(v)
            return self._const(v.item() if isinstance(v, np.generic) else v)
        if a.dtype.kind in "mM" or b.dtype.kind in "mM":
            return self._arith_time(opname, a, b, dt)
        if dt.kind == "b":  # numpy: bool + bool = or, bool * bool = and
            if opname in ("+", "*"):
                return _Typed(a.code + b.code + [OP["OR_I" if opname == "+" else "AND_I"]], dt)
            raise UnsupportedExpression(f"boolean {opname}")
        if dt.kind == "f" and opname == "**" and b.scalar is not None and a.scalar is None \
                and not isinstance(b.scalar, bool) and b.scalar in (2, 0.5, -1, 1):
            # numpy's fast_scalar_power: x**2 = square, x**0.5 = sqrt, x**-1 = reciprocal
            x = self._to_float(a, dt)
            if b.scalar == 2:
                code = x + x + [OP["MUL_F"]]
            elif b.scalar == 0.5:
                code = x + [OP["SQRT"]]
            elif b.scalar == -1:
                code = self._const(1.0).code + x + [OP["DIV_F"]]
            else:
                code = x
        elif dt.kind == "f":
            code = self._to_float(a, dt) + self._to_float(b, dt)
            op = {"+": "ADD_F", "-": "SUB_F", "*": "MUL_F", "/": "DIV_F", "//": "FLOORDIV_F", "%": "MOD_F",
                  "**": "POW_F"}[opname]
            if dt == np.float32 and opname in ("//", "%"):
                # + - * / and sqrt in float64, rounded once, equal the float32 operation; the
                # several steps of floor_divide / remainder do not, so they run in float32
                op += "32"
            code.append(OP[op])
        else:
            if opname == "**" and b.scalar is not None and b.scalar < 0:
                raise UnsupportedExpression("integers to negative integer powers")
            code = a.code + b.code
            op = {"+": "ADD_I", "-": "SUB_I", "*": "MUL_I", "//": "FLOORDIV_I", "%": "MOD_I", "**": "POW_I"}[opname]
            if dt == np.uint64 and op in ("FLOORDIV_I", "MOD_I", "POW_I"):
                op = op[:-1] + "U"  # a slot holds 64 bits: only uint64 nodes can exceed the signed range
            code.append(OP[op])
        return _Typed(self._finish(code, dt), dt)

    def _to_unit(self, t, dtype):
        """code leaving the datetime64 / timedelta64 value t in the unit of ``dtype`` (of t's
        kind): a constant is converted on the host, a column expression by DT_CAST."""
        dtype = np.dtype(dtype)
        if t.dtype == dtype:
            return list(t.code)
        if t.scalar is not None:
            v = t.scalar.astype(dtype)
            if v.astype(t.dtype) != t.scalar and _unit(dtype) < _unit(t.dtype):
                raise UnsupportedExpression(f"constant {t.scalar!r} overflows {dtype}")
            return list(self._const(v).code)
        arg = _unit(t.dtype) | _unit(dtype) << 4 | (t.dtype.kind == "m") << 8
        return list(t.code) + [DT_OP["DT_CAST"] | arg << 8]

    def _arith_time(self, opname, a, b, dt):
        """datetime64 / timedelta64 arithmetic as numpy types it (dt is numpy's result dtype):
        M - M -> m, M +- m, m +- m, m * int, m // int, m // m -> int64, m / m -> float64.  Mixed
        units meet in numpy's result unit: a DT_CAST on the coarser column operand."""
        ka, kb = a.dtype.kind, b.dtype.kind
        if opname in ("+", "-") and ka in "mM" and kb in "mM":
            # the operands in the result's unit, each in its own kind
            unit = np.datetime_data(dt)[0]
            x = self._to_unit(a, f"{ka}8[{unit}]")
            y = self._to_unit(b, f"{kb}8[{unit}]")
            return _Typed(x + y + [OP["ADD_I" if opname == "+" else "SUB_I"]], dt)
        int_a = ka in "iu" and (a.scalar is None or type(a.scalar) is int)
        int_b = kb in "iu" and (b.scalar is None or type(b.scalar) is int)
        if opname == "*" and dt.kind == "m" and ((ka == "m" and int_b) or (kb == "m" and int_a)):
            return _Typed(a.code + b.code + [OP["MUL_I"]], dt)
        if opname == "//" and ka == "m" and int_b and dt.kind == "m":
            # numpy's timedelta64 // integer is C's truncating division (timedelta64 //
            # timedelta64 floors): the floor plus one where the remainder is not zero and the
            # signs differ
            zero = self._const(0).code
            return _Typed(a.code + b.code + [OP["FLOORDIV_I"]] + a.code + b.code + [OP["MOD_I"]] + zero + [OP["NE_I"]]
                          + a.code + b.code + [OP["XOR_I"]] + zero + [OP["LT_I"], OP["AND_I"], OP["ADD_I"]], dt)
        if opname in ("//", "/") and ka == "m" and kb == "m":
            common = self._resolve(np.result_type, a.dtype, b.dtype)
            x, y = self._to_unit(a, common), self._to_unit(b, common)
            if opname == "//":
                return _Typed(x + y + [OP["FLOORDIV_I"]], dt)
            return _Typed(x + [OP["I2F"]] + y + [OP["I2F"], OP["DIV_F"]], dt)
        raise UnsupportedExpression(f"{a.dtype} {opname} {b.dtype}")

    def _bitwise(self, opname, a, b):
        ufunc = {"&": np.bitwise_and, "|": np.bitwise_or, "^": np.bitwise_xor,
                 "<<": np.left_shift, ">>": np.right_shift}[opname]
        dt = self._resolve(ufunc, a.proto, b.proto)
        op = {"&": "AND_I", "|": "OR_I", "^": "XOR_I", "<<": "SHL_I", ">>": "SHR_I"}[opname]
        if dt == np.uint64 and op == "SHR_I":
            op = "SHR_U"
        return _Typed(self._finish(a.code + b.code + [OP[op]], dt), dt)

    def v_BinOp(self, node):
        a, b = self.visit(node.left), self.visit(node.right)
        sym = {ast.Add: "+", ast.Sub: "-", ast.Mult: "*", ast.Div: "/", ast.FloorDiv: "//", ast.Mod: "%",
               ast.Pow: "**", ast.BitAnd: "&", ast.BitOr: "|", ast.BitXor: "^", ast.LShift: "<<",
               ast.RShift: ">>"}.get(type(node.op))
        if sym is None:
            raise UnsupportedExpression(f"operator {type(node.op).__name__}")
        if sym in ("&", "|", "^", "<<", ">>"):
            return self._bitwise(sym, a, b)
        return self._arith(sym, a, b)

    def v_UnaryOp(self, node):
        a = self.visit(node.operand)
        if isinstance(node.op, ast.USub):
            if a.dtype.kind == "M":
                raise UnsupportedExpression("negation of a datetime")
            if a.scalar is not None:
                return self._const(-a.scalar)
            if a.dtype.kind == "b":
                raise UnsupportedExpression("negation of a boolean")
            if a.dtype.kind == "f":
                return _Typed(self._finish(a.code + [OP["NEG_F"]], a.dtype), a.dtype)
            return _Typed(self._finish(a.code + [OP["NEG_I"]], a.dtype), a.dtype)
        if isinstance(node.op, ast.UAdd):
            return a
        if isinstance(node.op, (ast.Invert, ast.Not)):
            if a.dtype.kind == "b":
                return _Typed(a.code + [OP["NOT_B"]], np.bool_)
            if isinstance(node.op, ast.Not) or a.dtype.kind in "fmM":  # numpy: no invert loop for them
                raise UnsupportedExpression(f"not / ~ of {a.dtype}")
            return _Typed(self._finish(a.code + [OP["INV_I"]], a.dtype), a.dtype)
        raise UnsupportedExpression("unary operator")

    _MIRROR = {"LT": "GT", "LE": "GE", "GT": "LT", "GE": "LE", "EQ": "EQ", "NE": "NE"}

    def _compare(self, op, a, b):
        sym = {ast.Lt: "LT", ast.LtE: "LE", ast.Gt: "GT", ast.GtE: "GE", ast.Eq: "EQ", ast.NotEq: "NE"}.get(type(op))
        if sym is None:
            raise UnsupportedExpression("comparison operator")

        def is_int(t):
            return t.scalar is not None and not isinstance(t.scalar, bool) and isinstance(t.scalar, int)

        if a.dtype.kind in "mM" or b.dtype.kind in "mM":
            if a.dtype.kind != b.dtype.kind:
                raise UnsupportedExpression(f"comparison of {a.dtype} with {b.dtype}")
            # like kinds meet in numpy's result unit; a column against a constant of its own
            # unit stays COL CONST CMP, the shape of the comparison-terms kernel
            common = self._resolve(np.result_type, a.dtype, b.dtype)
            return _Typed(self._to_unit(a, common) + self._to_unit(b, common) + [OP[sym + "_I"]], np.bool_)
        # integers compare exactly in numpy 2, whatever the two dtypes
        if is_int(b) and a.scalar is None and a.dtype.kind in "iub":
            return self._compare_int_const(sym, a, b)
        if is_int(a) and b.scalar is None and b.dtype.kind in "iub":
            return self._compare_int_const(self._MIRROR[sym], b, a)
        if a.scalar is None and b.scalar is None and {a.dtype.kind, b.dtype.kind} == {"i", "u"} \
                and np.uint64 in (a.dtype, b.dtype):
            if a.dtype.kind == "i":
                return self._compare_signed_unsigned(sym, a, b)
            return self._compare_signed_unsigned(self._MIRROR[sym], b, a)
        dt = self._resolve(np.result_type, a.proto, b.proto)
        if dt.kind == "f":
            return _Typed(self._to_float(a, dt) + self._to_float(b, dt) + [OP[sym + "_F"]], np.bool_)
        unsigned = dt == np.uint64 and sym not in ("EQ", "NE")
        return _Typed(a.code + b.code + [OP[sym + ("_U" if unsigned else "_I")]], np.bool_)

    def _compare_int_const(self, sym, col, con):
        """``col sym con`` for an integer / boolean column expression and a Python int, which
        may lie outside the column's dtype: numpy 2 answers as if both were exact integers."""
        v = con.scalar
        if col.dtype.kind == "b" and not -(1 << 63) <= v < (1 << 63):
            raise UnsupportedExpression("boolean compared with an integer outside int64")  # numpy raises
        if col.dtype == np.uint64:
            if v < 0:  # every value is greater
                return _Typed(self._const(sym in ("GT", "GE", "NE")).code, np.bool_)
            return _Typed(col.code + con.code + [OP[sym + ("_I" if sym in ("EQ", "NE") else "_U")]], np.bool_)
        # any other slot is a sign- / zero-extended value within int64
        if v >= (1 << 63):  # every value is less
            return _Typed(self._const(sym in ("LT", "LE", "NE")).code, np.bool_)
        return _Typed(col.code + con.code + [OP[sym + "_I"]], np.bool_)

    def _compare_signed_unsigned(self, sym, s, u):
        """``s sym u`` for a signed expression and a uint64 one, exactly (numpy 2 does not go
        through float64 here): a negative s is below every u, otherwise both compare unsigned."""
        zero = self._const(0).code
        if sym in ("LT", "LE", "NE"):
            first, second, comb = "LT_I", sym + ("_I" if sym == "NE" else "_U"), "OR_I"
        else:
            first, second, comb = "GE_I", sym + ("_I" if sym == "EQ" else "_U"), "AND_I"
        return _Typed(s.code + zero + [OP[first]] + s.code + u.code + [OP[second], OP[comb]], np.bool_)

    def v_Compare(self, node):
        if len(node.ops) == 1 and isinstance(node.ops[0], (ast.Eq, ast.NotEq)):
            # string expression == / != 'constant' (either side): str_equals / str_notequals
            a, b = node.left, node.comparators[0]
            for col, con in ((a, b), (b, a)):
                if isinstance(con, ast.Constant) and isinstance(con.value, str) and not isinstance(col, ast.Constant):
                    source = self._string_source(col)
                    if source is not None:
                        return self._string_input("str_equals" if isinstance(node.ops[0], ast.Eq) else "str_notequals",
                                                  source, con.value)
        left = self.visit(node.left)
        out = None
        for op, comp in zip(node.ops, node.comparators):
            right = self.visit(comp)
            t = self._compare(op, left, right)
            out = t if out is None else _Typed(out.code + t.code + [OP["AND_I"]], np.bool_)
            left = right
        return out

    def v_BoolOp(self, node):
        vals = [self.visit(v) for v in node.values]
        if any(v.dtype.kind != "b" for v in vals):
            raise UnsupportedExpression("and / or of non-booleans")
        op = OP["AND_I"] if isinstance(node.op, ast.And) else OP["OR_I"]
        code = list(vals[0].code)
        for v in vals[1:]:
            code += v.code + [op]
        return _Typed(code, np.bool_)

    def v_Call(self, node):
        f = node.func
        if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id in ("np", "numpy"):
            name = f.attr
        elif isinstance(f, ast.Name):
            name = f.id
        else:
            raise UnsupportedExpression("call")
        from . import strings
        if name in strings.FUNCTIONS:
            return self._string_call(name, node)
        if name in strings.TRANSFORMS:
            self._string_source(node)  # its own refusals first
            raise UnsupportedExpression(f"{name} gives strings: a program computes numbers (its str_* predicates and "
                                        "lengths take it as their argument)")
        if node.keywords:
            raise UnsupportedExpression("keyword arguments")
        if name == "astype" and len(node.args) == 2:
            return self._astype(node.args[0], node.args[1])
        if name in ("datetime64", "timedelta64", "scalar_datetime", "scalar_timedelta"):
            # np.datetime64('2015-06-01') (the repr of a numpy 2 scalar), functions.py:274-281
            try:
                values = [ast.literal_eval(a) for a in node.args]
                make = np.datetime64 if name.endswith("datetime64") or name == "scalar_datetime" else np.timedelta64
                return self._const(make(*values))
            except (ValueError, TypeError) as e:
                raise UnsupportedExpression(f"{name}: {e}")
        if name in MISSING_FUNCTIONS:
            return self._missing_call(name, node.args)
        args = [self.visit(a) for a in node.args]
        if name.startswith("dt_") and name[3:] in DT_FIELDS and len(args) == 1:
            a = args[0]
            if a.dtype.kind != "M" or a.scalar is not None or np.datetime_data(a.dtype)[0] not in DT_FIELD_UNITS:
                raise UnsupportedExpression(f"{name} of {a.dtype} (a datetime64 expression in ns .. D)")
            arg = DT_FIELDS.index(name[3:]) | _unit(a.dtype) << 4
            return _Typed(a.code + [DT_OP["DT_FIELD"] | arg << 8], np.bool_ if name == "dt_is_leap_year" else np.int32)
        if name.startswith("td_") and name[3:] in TD_FIELDS and len(args) == 1:
            a = args[0]
            if a.dtype.kind != "m" or a.scalar is not None or np.datetime_data(a.dtype)[0] not in DT_FIELD_UNITS:
                raise UnsupportedExpression(f"{name} of {a.dtype} (a timedelta64 expression in ns .. D)")
            field, dt = TD_FIELDS[name[3:]]
            return _Typed(a.code + [DT_OP["TD_FIELD"] | (field | _unit(a.dtype) << 4) << 8], dt)
        if any(a.dtype.kind in "mM" for a in args) and name not in ("minimum", "maximum", "where"):
            raise UnsupportedExpression(f"function {name} of a datetime64 / timedelta64 value")
        if name in FUNCTIONS and len(args) == 1:
            ufunc, op = FUNCTIONS[name]
            a = args[0]
            dt = self._resolve(ufunc, a.proto)
            if dt.kind != "f":
                raise UnsupportedExpression(f"{name} of {a.dtype}")
            return _Typed(self._finish(self._to_float(a, dt) + [OP[op]], dt), dt)
        if name in PREDICATES and len(args) == 1:
            a = args[0]
            # isnan consumes the mask (functions.py:238-251: unmasked, False at missing rows);
            # isfinite / isinf propagate it
            own = name == "isnan"
            if a.dtype.kind != "f":  # integers are never nan / inf: a constant column
                return _Typed(self._const(name == "isfinite").code, np.bool_, own_mask=own)
            code = a.code + [OP[PREDICATES[name][1]]]
            if own and a.mask:
                code += _mask_code(a.mask) + [OP["NOT_B"], OP["AND_I"]]
            return _Typed(code, np.bool_, own_mask=own)
        if name in ("abs", "absolute", "fabs") and len(args) == 1:
            a = args[0]
            if a.dtype.kind == "f" or name == "fabs":
                dt = self._resolve(np.fabs, a.proto) if name == "fabs" else a.dtype
                return _Typed(self._finish(self._to_float(a, dt) + [OP["ABS_F"]], dt), dt)
            if a.dtype.kind in "ub":  # the identity; ABS_I would read a uint64 >= 2**63 as negative
                return a
            return _Typed(self._finish(a.code + [OP["ABS_I"]], a.dtype), a.dtype)
        if name in ("minimum", "maximum", "fmin", "fmax", "arctan2") and len(args) == 2:
            a, b = args
            if name in ("fmin", "fmax"):
                raise UnsupportedExpression(name)
            dt = self._resolve(getattr(np, name), a.proto, b.proto)
            if dt.kind in "mM":
                if a.dtype.kind != b.dtype.kind or name == "arctan2":
                    raise UnsupportedExpression(f"{name} of {a.dtype} and {b.dtype}")
                op = {"minimum": "MIN_I", "maximum": "MAX_I"}[name]
                return _Typed(self._to_unit(a, dt) + self._to_unit(b, dt) + [OP[op]], dt)
            if dt.kind == "f":
                op = {"minimum": "MIN_F", "maximum": "MAX_F", "arctan2": "ARCTAN2"}[name]
                return _Typed(self._finish(self._to_float(a, dt) + self._to_float(b, dt) + [OP[op]], dt), dt)
            if name == "arctan2":
                raise UnsupportedExpression(f"arctan2 of {dt}")
            op = {"minimum": "MIN", "maximum": "MAX"}[name] + ("_U" if dt == np.uint64 else "_I")
            return _Typed(self._finish(a.code + b.code + [OP[op]], dt), dt)
        if name == "where" and len(args) == 3:
            c, a, b = args
            if c.dtype.kind != "b":
                raise UnsupportedExpression("where condition must be boolean")
            dt = self._resolve(np.where, np.empty(0, bool), a.proto, b.proto)
            for t in (a, b):  # np.where wraps such a value silently; every other operation refuses it
                if dt.kind in "iu" and isinstance(t.scalar, int) and not isinstance(t.scalar, bool) \
                        and not np.iinfo(dt).min <= t.scalar <= np.iinfo(dt).max:
                    raise UnsupportedExpression(f"Python integer {t.scalar} out of bounds for {dt}")
            if dt.kind in "mM" or a.dtype.kind in "mM" or b.dtype.kind in "mM":
                if a.dtype.kind != b.dtype.kind or dt.kind not in "mM":
                    raise UnsupportedExpression(f"where of {a.dtype} and {b.dtype}")
                code = c.code + self._to_unit(a, dt) + self._to_unit(b, dt) + [OP["WHERE"]]
            elif dt.kind == "f":
                code = c.code + self._to_float(a, dt) + self._to_float(b, dt) + [OP["WHERE"]]
            else:
                code = c.code + a.code + b.code + [OP["WHERE"]]
            # missing where the condition is, and otherwise where the chosen branch is
            mask = c.mask
            if a.mask or b.mask:
                false = self._const(False).code
                term = c.code + (_mask_code(a.mask) if a.mask else false) + (_mask_code(b.mask) if b.mask else false)
                mask = _mask_or(mask, (tuple(term + [OP["WHERE"]]),))
            return _Typed(self._finish(code, dt), dt, mask=mask, own_mask=True)
        raise UnsupportedExpression(f"function {name}")

    def _fill_const(self, name, dt, value):
        """the code of the fill value in the column's dtype, converted as numpy's assignment
        ``ar[mask] = value`` converts it; a value the dtype cannot hold is refused"""
        if isinstance(value, np.generic):
            value = value.item()
        if not isinstance(value, (bool, int, float)):
            raise UnsupportedExpression(f"{name}: the value is an int, float or bool, not {value!r}")
        ar = np.zeros(1, dt)
        with np.errstate(all="ignore"):
            try:
                ar[np.array([True])] = value
            except (OverflowError, TypeError, ValueError) as e:
                raise UnsupportedExpression(f"{name}: {value!r} does not fit {dt}: {e}")
        got = ar[0].item()
        if dt.kind in "iub" and got != value:  # numpy truncates 1.5 to 1 and takes 2 for True silently
            raise UnsupportedExpression(f"{name}: {dt} cannot hold {value!r}")
        return list(self._const(got).code)

    def _missing_call(self, name, nodes):
        """ismissing / notmissing / isna / notna (unmasked booleans; the constants for an unmasked
        argument without NaN), fillmissing / fillna (unmasked, the argument's dtype) and fillnan
        (NaN of float nodes replaced, the mask kept), in the existing opcodes."""
        if len(nodes) != MISSING_FUNCTIONS[name]:
            raise UnsupportedExpression(f"{name} takes {MISSING_FUNCTIONS[name]} argument(s)")
        a = self.visit(nodes[0])
        if a.dtype.kind in "mM":
            raise UnsupportedExpression(f"{name} of a datetime64 / timedelta64 value")
        missing = _mask_code(a.mask) if a.mask else None
        nan = list(a.code) + [OP["ISNAN"]] if a.dtype.kind == "f" else None
        na = nan + missing + [OP["OR_I"]] if nan and missing else (nan or missing)
        if name in ("ismissing", "notmissing", "isna", "notna"):
            cond = missing if name.endswith("missing") else na
            negate = name.startswith("not")
            if cond is None:
                return _Typed(self._const(negate).code, np.bool_, own_mask=True)
            return _Typed(cond + ([OP["NOT_B"]] if negate else []), np.bool_, own_mask=True)
        v = self.visit(nodes[1])
        if v.scalar is None or a.scalar is not None:
            raise UnsupportedExpression(f"{name}(x, value): x is a column expression, value a constant or a variable")
        fill = self._fill_const(name, a.dtype, v.scalar)
        cond = {"fillmissing": missing, "fillnan": nan, "fillna": na}[name]
        mask = a.mask if name == "fillnan" else None
        if cond is None:
            return _Typed(list(a.code), a.dtype, mask=mask, own_mask=True)
        return _Typed(cond + fill + list(a.code) + [OP["WHERE"]], a.dtype, mask=mask, own_mask=True)

    def _string_call(self, name, node):
        """``str_len(s)`` / ``str_byte_length(s)`` / ``str_<predicate>(s, 'literal')`` over a string
        column or a string-valued expression (``str_contains`` also with ``regex=False`` or a third
        positional False)."""
        from . import strings
        col = self._string_source(node.args[0]) if node.args else None
        if col is None:
            raise UnsupportedExpression(f"{name} takes a string column")
        rest = list(node.args[1:])
        if name == "str_contains":
            flags = [k.value for k in node.keywords if k.arg == "regex"] + rest[1:2]
            if len(flags) > 1 or len(node.keywords) > len(flags) or len(rest) > 2:
                raise UnsupportedExpression("str_contains(s, pattern, regex=False)")
            for f in flags:
                if not (isinstance(f, ast.Constant) and f.value is False):
                    raise NotImplementedError("str_contains: regular expressions are not supported (regex=False)")
            rest = rest[:1]
        elif node.keywords:
            raise UnsupportedExpression("keyword arguments")
        if name in strings.LEN_KINDS:
            if rest:
                raise UnsupportedExpression(f"{name} takes one argument")
            return self._string_input(name, col)
        if len(rest) != 1 or not isinstance(rest[0], ast.Constant):
            raise UnsupportedExpression(f"{name}(s, 'literal')")
        return self._string_input(name, col, rest[0].value)

    def _astype(self, value_node, dtype_node):
        """``astype(x, 'dtype')`` (the reference's ``Expression.astype``, expression.py;
        ``agg.py:197-201`` casts var/std inputs this way): numpy ``ndarray.astype``
        semantics -- float -> int truncates toward zero, integers wrap."""
        if not (isinstance(dtype_node, ast.Constant) and isinstance(dtype_node.value, str)):
            raise UnsupportedExpression("astype needs a constant dtype string")
        try:
            dt = np.dtype(dtype_node.value)
        except TypeError as e:
            raise UnsupportedExpression(str(e))
        if dt.kind not in "biufmM" or dt.itemsize > 8:
            raise UnsupportedExpression(f"astype to {dt}")
        a = self.visit(value_node)
        if dt.kind in "mM" or a.dtype.kind in "mM":
            return self._astype_time(a, dt)
        if a.dtype == dt and a.scalar is None:
            return a
        if a.scalar is not None:
            # numpy's result is a scalar of dtype dt: strong in promotion, unlike a Python scalar
            # (`f32 + astype(0.1, 'float64')` is float64), so the constant keeps dt and no scalar
            self._finish([], dt)  # refuses float16
            with np.errstate(all="ignore"):
                return _Typed(self._const(np.array(a.scalar).astype(dt).item()).code, dt)
        if dt.kind == "f":
            return _Typed(self._finish(self._to_float(a, dt), dt), dt)
        if dt.kind == "b":
            if a.dtype.kind == "f":
                code = list(a.code) + self._const(0.0).code + [OP["NE_F"]]
            else:
                code = a.code + self._const(0).code + [OP["NE_I"]]
            return _Typed(code, dt)
        # float -> uint64 reaches 2**64, beyond F2I's int64
        code = list(a.code) + ([OP["F2U" if dt == np.uint64 else "F2I"]] if a.dtype.kind == "f" else [])
        return _Typed(self._finish(code, dt), dt)


    def _astype_time(self, a, dt):
        """Unit casts of datetime64 / timedelta64 (DT_CAST: finer -> coarser floors, to M / Y
        through the civil date, as numpy), and the reinterpreting casts to and from int64.
        What numpy refuses (a timedelta64 cast across the M / Y boundary, datetime64 <->
        timedelta64) is refused."""
        if dt.kind in "mM":
            _unit(dt)
        with np.errstate(all="ignore"):
            try:
                np.empty(0, a.dtype).astype(dt)
            except TypeError as e:
                raise UnsupportedExpression(str(e))
        if a.dtype.kind in "mM" and dt.kind in "mM":
            if a.dtype.kind != dt.kind or (dt.kind == "m" and (_unit(a.dtype) >= 8) != (_unit(dt) >= 8)):
                raise UnsupportedExpression(f"astype of {a.dtype} to {dt}")  # numpy: no m8 cast across M / Y
            if a.scalar is not None:
                return _Typed(self._to_unit(a, dt), dt, scalar=a.scalar.astype(dt))
            return _Typed(self._to_unit(a, dt), dt)
        if (a.dtype.kind in "mM" and dt == np.int64) or (dt.kind in "mM" and a.dtype == np.int64 and
                                                        not isinstance(a.scalar, bool)):
            if a.scalar is not None:
                v = np.asarray(a.scalar).astype(dt)[()]
                return self._const(v) if dt.kind in "mM" else _Typed(self._const(int(v)).code, dt)
            return _Typed(list(a.code), dt)  # the ticks themselves
        raise UnsupportedExpression(f"astype of {a.dtype} to {dt}")


def _stack_depth(code):
    binary = BINARY
    d = m = 0
    for ins in code:
        op = ins & 0xFF
        if op in (OP["COL"], OP["CONST"]):
            d += 1
        elif op == OP["WHERE"]:
            d -= 2
        elif op in binary:
            d -= 1
        m = max(m, d)
    return m


class Program:
    """A compiled expression: evaluate(df, i1, i2) -> DeviceArray of ``dtype``, or a
    DeviceMaskedArray when the result can be missing (``mask_code`` is set: a bool program over
    the same inputs and constants, 1 = missing).  keep: the expression is wanted as a row mask
    (a filter, a selection): a missing value selects nothing, so the program is ``value & ~mask``
    and has no mask program."""

    def __init__(self, df, expression, keep=False):
        self.expression = str(expression)
        c = Compiler(df)
        try:
            tree = ast.parse(self.expression, mode="eval")
        except SyntaxError as e:
            raise UnsupportedExpression(str(e))
        t = c.visit(tree)
        code = list(t.code)  # a constant expression is broadcast by the kernel
        mask_code = _mask_code(t.mask) if t.mask else None
        if keep and mask_code is not None:
            if t.dtype.kind != "b":
                raise UnsupportedExpression(f"a row mask is boolean, not {t.dtype}")
            # value & (m == 0) & ...: a conjunction of comparisons stays one (the shape of the
            # comparison-terms kernel); any other mask term is negated as it is
            zero = c._const(0).code
            for term in t.mask:
                if len(term) == 1 and term[0] & 0xFF == OP["COL"]:
                    code += list(term) + zero + [OP["EQ_I"], OP["AND_I"]]
                else:
                    code += list(term) + [OP["NOT_B"], OP["AND_I"]]
            mask_code = None
        for prog in (code, mask_code or []):
            if len(prog) > MAX_CODE:
                raise UnsupportedExpression("expression too long for the device program")
            if _stack_depth(prog) > MAX_DEPTH:
                raise UnsupportedExpression("expression too deeply nested")
        # keep the constants that the programs use, in the order of first use
        used = []
        for prog in (code, mask_code or []):
            for k, ins in enumerate(prog):
                if ins & 0xFF == OP["CONST"]:
                    if ins >> 8 not in used:
                        used.append(ins >> 8)
                    prog[k] = OP["CONST"] | used.index(ins >> 8) << 8
        if len(used) > MAX_CONST:
            raise UnsupportedExpression("too many constants")
        self.code = code
        self.mask_code = mask_code
        self.consts = [c.consts[k] for k in used]
        self.columns = list(c.columns)
        self.dtype = t.dtype  # bool results are 0 / 1 bytes (numpy bool)
        self.is_bool = t.dtype.kind == "b"

    def evaluate(self, df, i1, i2, out=None):
        from .device import DeviceArray, DeviceMaskedArray
        n = i2 - i1
        cols = []
        keep = []
        strings = {}  # the transformed sources of this evaluation, each computed once
        for name in self.columns:
            if isinstance(name, tuple) and name[0] == "mask":  # a masked column's mask (Compiler._column)
                cols.append(df.columns[name[1]].mask[i1:i2])
                continue
            if isinstance(name, tuple):  # a string function's column (Compiler._string_input)
                _, fn, source, arg = name
                scol = evaluate_string(df, source, i1, i2, strings)
                cols.append(scol.match(fn, arg) if arg is not None else scol.len(fn))
                continue
            col = df.columns[name]
            if isinstance(col, DeviceMaskedArray):
                col = col.data[i1:i2]
            elif not isinstance(col, DeviceArray):
                col = DeviceArray.from_numpy(np.ascontiguousarray(col[i1:i2]))
                keep.append(col)
            else:
                col = col[i1:i2]
            cols.append(col)
        if out is None:
            out = DeviceArray.empty(n, self.dtype)
        k = max(1, len(cols))
        consts = (ctypes.c_uint64 * max(1, len(self.consts)))(*self.consts)
        ptrs = (ctypes.c_void_p * k)(*[c.ptr for c in cols])
        dts = (ctypes.c_int * k)(*[_lib.dtype_code(c.dtype)[0] for c in cols])
        code = (ctypes.c_uint32 * len(self.code))(*self.code)
        _lib.call("vh_expr_eval", code, len(self.code), consts, len(self.consts), ptrs, dts, len(cols), n,
                  _lib.dtype_code(self.dtype)[0], out.ptr)
        if self.mask_code is not None:
            # the mask program: a second launch of the same kernel over the same inputs (its
            # input bytes do not overlap the value program's: one pass would save only a launch)
            mask = DeviceArray.empty(n, np.uint8)
            code = (ctypes.c_uint32 * len(self.mask_code))(*self.mask_code)
            _lib.call("vh_expr_eval", code, len(self.mask_code), consts, len(self.consts), ptrs, dts, len(cols), n,
                      _lib.DTYPE_CODE["uint8"], mask.ptr)
            out = DeviceMaskedArray(out, mask)
        if keep:
            _lib.synchronize()  # the staged columns are freed on return
        return out


def string_plan(df, expression):
    """The plan of a string-valued expression on ``df`` (``Compiler._string_source``), None for
    any other expression."""
    try:
        tree = ast.parse(str(expression), mode="eval")
    except SyntaxError:
        return None
    return Compiler(df)._string_source(tree)


def plan_columns(plan):
    """the names of the string columns a plan reads, in order, each once"""
    if plan[0] == "col":
        return [plan[1]]
    names = plan_columns(plan[2])
    for a in plan[3]:
        if isinstance(a, tuple):
            names += [n for n in plan_columns(a[1]) if n not in names]
    return names


def evaluate_string(df, plan, i1, i2, memo=None):
    """The DeviceStringArray of a plan for the rows [i1, i2): transforms are row-local, so the
    source columns are sliced (views) and every transform runs over the slice.  ``memo`` (plan ->
    column, for one row range) lets the plans of one evaluation share what they have in common:
    ``str_lower(s)`` runs once under two predicates."""
    if plan[0] == "col":
        return df.columns[plan[1]][i1:i2]
    if memo is not None and plan in memo:
        return memo[plan]
    _, method, src, args, kwargs = plan
    col = evaluate_string(df, src, i1, i2, memo)
    args = [evaluate_string(df, a[1], i1, i2, memo) if isinstance(a, tuple) else a for a in args]
    out = getattr(col, method)(*args, **dict(kwargs))
    if memo is not None:
        memo[plan] = out
    return out


_CACHE = {}


def compile_expression(df, expression, keep=False):
    """The Program of ``expression`` on ``df`` (cached per frame structure); keep: as a row mask
    (``Program``)."""
    from .device import DeviceMaskedArray
    key = (id(df), str(expression), bool(keep), tuple(sorted(df.virtual_columns.items())),
           tuple(sorted((k, repr(v)) for k, v in df.variables.items() if np.isscalar(v))),
           tuple((k, str(getattr(v, "dtype", "")), isinstance(v, DeviceMaskedArray)) for k, v in df.columns.items()))
    p = _CACHE.get(key)
    if p is not None:
        for name in p.columns:  # the key names dtypes, not column objects: a new column may hold NaT
            if isinstance(name, tuple):
                continue
            if np.dtype(df.columns[name].dtype).kind in "mM" and df._column_has_nat(name):
                raise UnsupportedExpression(f"column {name!r} holds NaT (not-a-time) values")
    if p is None:
        p = Program(df, expression, keep=keep)
        if len(_CACHE) > 256:
            _CACHE.clear()
        _CACHE[key] = p
    return p
