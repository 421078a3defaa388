"""A DataFrame exposing the reference's binned-statistics API on the GPU path.

Restates the parts of ``packages/vaex-core/vaex/dataframe.py`` that drive this hot
path -- ``count/sum/mean/min/max/std/var/first`` (``:741-1000``), ``minmax``
(``:1276-1333``), ``median_approx`` / ``percentile_approx`` (``:1399-1555``),
``cov`` / ``covar`` / ``correlation`` (``:1067-1272``), ``mutual_information``
(``:622-718``), ``limits`` (``:1617+``), ``_binner*``/``_create_binners``
(``:5251-5295``), ``_agg``, ``_set`` (``:474``), ``categorize`` (``:5487-5533``), ``unique`` (``:542-619``; with
``Expression.value_counts`` / ``unique`` / ``nunique``, ``expression.py:946-1093``),
``groupby``/``binby`` (``:6622-6683``) and the binner specs ``BinnerScalar`` /
``BinnerOrdinal`` (``:6737-6800``) -- over columns that are numpy arrays (staged to
HBM per chunk) or :class:`~vaex_amd.device.DeviceArray` (HBM-resident).

The reference's lazy expression engine is out of scope: expressions
here are column names, or numpy expressions over host columns evaluated per chunk.
"""
import ast
import re
import threading
import weakref

import numpy as np

from . import agg as vagg
from . import selections
from .device import DeviceArray, DeviceMaskedArray
from .strings import STRING, DeviceStringArray
from .execution import default_executor
from .promise import Promise, delayed
from .tasks import TaskMinMax, TaskSetCreate, TaskValueCounts
from .utils import _expand_limits, _expand_shape, listify, unlistify

default_shape = 128


class RowLimitException(ValueError):
    pass


_mask_cache_lock = threading.Lock()


def _column_ref(col):
    """A callable giving the column while it is alive: a weak reference where the type has one."""
    try:
        return weakref.ref(col)
    except TypeError:
        return lambda: col


def _variable_value(v):
    """What the mask cache remembers of a variable: a scalar's type and value (its repr also
    tells -0.0 from 0.0 and matches NaN with NaN); any other object itself, compared by identity
    and held so that its id() cannot be handed out again."""
    if v is None or isinstance(v, (bool, int, float, complex, str, bytes, np.generic)):
        return (type(v), repr(v))
    return (None, v)


def _same_variables(a, b):
    return len(a) == len(b) and all(x[0] is y[0] and (x[1] == y[1] if x[0] is not None else x[1] is y[1])
                                    for x, y in zip(a, b))


def _ensure_string(e):
    return str(e) if isinstance(e, Expression) else e


def _ensure_strings(es):
    if isinstance(es, (list, tuple)):
        return [_ensure_string(e) for e in es]
    return _ensure_string(es)


def _literal(value):
    """a fill value as expression text: a numpy scalar as its Python value (``repr`` of one is a call)"""
    return repr(value.item() if isinstance(value, np.generic) else value)


def _issequence(x):
    return isinstance(x, (tuple, list, np.ndarray))


class BinnerScalar:
    """Spec of a scalar binner (dataframe.py:6749-6775)."""
    kind = "scalar"

    def __init__(self, expression, minimum, maximum, count, dtype):
        self.expression = str(expression)
        self.minimum = minimum
        self.maximum = maximum
        self.count = count
        self.dtype = np.dtype(dtype)

    def __hash__(self):
        return hash((self.kind, self.expression, self.minimum, self.maximum, self.count, self.dtype))

    def __eq__(self, rhs):
        return isinstance(rhs, BinnerScalar) and (self.expression, self.minimum, self.maximum, self.count,
                                                  self.dtype) == (rhs.expression, rhs.minimum, rhs.maximum,
                                                                  rhs.count, rhs.dtype)


class BinnerOrdinal:
    """Spec of an ordinal binner (dataframe.py:6778-6800)."""
    kind = "ordinal"

    def __init__(self, expression, minimum, count, dtype):
        self.expression = str(expression)
        self.minimum = minimum
        self.count = count
        self.dtype = np.dtype(dtype)

    def __hash__(self):
        return hash((self.kind, self.expression, self.minimum, self.count, self.dtype))

    def __eq__(self, rhs):
        return isinstance(rhs, BinnerOrdinal) and (self.expression, self.minimum, self.count, self.dtype) == (
            rhs.expression, rhs.minimum, rhs.count, rhs.dtype)


class Expression:
    """A column reference or host numpy expression bound to a DataFrame."""

    def __init__(self, df, expression):
        self.df = df
        self.expression = str(expression)

    def __str__(self):
        return self.expression

    def __repr__(self):
        return f"Expression({self.expression!r})"

    def _binop(self, other, op, reverse=False):
        o = other.expression if isinstance(other, Expression) else repr(other)
        s = f"({o} {op} {self.expression})" if reverse else f"({self.expression} {op} {o})"
        return Expression(self.df, s)

    def __add__(self, o): return self._binop(o, "+")
    def __radd__(self, o): return self._binop(o, "+", True)
    def __sub__(self, o): return self._binop(o, "-")
    def __rsub__(self, o): return self._binop(o, "-", True)
    def __mul__(self, o): return self._binop(o, "*")
    def __rmul__(self, o): return self._binop(o, "*", True)
    def __truediv__(self, o): return self._binop(o, "/")
    def __pow__(self, o): return self._binop(o, "**")
    def __lt__(self, o): return self._binop(o, "<")
    def __le__(self, o): return self._binop(o, "<=")
    def __gt__(self, o): return self._binop(o, ">")
    def __ge__(self, o): return self._binop(o, ">=")
    def __eq__(self, o):
        if isinstance(o, str):  # functions.py str_equals: a string column against a literal
            return Expression(self.df, f"str_equals({self.expression}, {o!r})")
        return self._binop(o, "==")

    def __ne__(self, o):
        if isinstance(o, str):
            return Expression(self.df, f"str_notequals({self.expression}, {o!r})")
        return self._binop(o, "!=")

    def __and__(self, o): return self._binop(o, "&")
    def __or__(self, o): return self._binop(o, "|")
    def __neg__(self): return Expression(self.df, f"(-{self.expression})")
    def __invert__(self): return Expression(self.df, f"(~{self.expression})")
    __hash__ = object.__hash__

    def astype(self, data_type):
        """expression.py ``Expression.astype``: the expression ``astype(x, 'dtype')``."""
        return Expression(self.df, f"astype({self.expression}, {str(np.dtype(data_type))!r})")

    # the functions that consume missing values (functions.py:146-268), as expressions
    def _missing(self, name, *args):
        return Expression(self.df, f"{name}({', '.join([self.expression] + [_literal(a) for a in args])})")

    def ismissing(self):
        return self._missing("ismissing")

    def notmissing(self):
        return self._missing("notmissing")

    def isna(self):
        return self._missing("isna")

    def notna(self):
        return self._missing("notna")

    def fillmissing(self, value):
        return self._missing("fillmissing", value)

    def fillnan(self, value):
        return self._missing("fillnan", value)

    def fillna(self, value):
        return self._missing("fillna", value)

    @property
    def is_masked(self):
        return self.df.is_masked(self.expression)

    @property
    def dtype(self):
        return self.df.data_type(self.expression)

    @property
    def dt(self):
        """expression.py ``DateTime`` accessor: ``df.t.dt.hour`` is ``dt_hour(t)`` (datetime.py)."""
        from .datetime import DateTime
        return DateTime(self)

    @property
    def td(self):
        """expression.py ``TimeDelta`` accessor: ``df.d.td.days`` is ``td_days(d)``."""
        from .datetime import TimeDelta
        return TimeDelta(self)

    @property
    def str(self):
        """expression.py ``StringOperations`` accessor: ``df.s.str.contains('x')`` is
        ``str_contains(s, 'x')`` (strings.py; the device string kernels)."""
        return StringOperations(self)

    @property
    def values(self):
        return self.df.evaluate(self.expression)

    def to_numpy(self):
        v = self.values
        if isinstance(v, (DeviceArray, DeviceMaskedArray, DeviceStringArray)):
            return v.to_numpy()
        return v if np.ma.isMaskedArray(v) else np.asarray(v)  # masked columns stay masked

    def tolist(self):
        return self.to_numpy().tolist()

    def sum(self, *args, **kw): return self.df.sum(self.expression, *args, **kw)
    def count(self, *args, **kw): return self.df.count(self.expression, *args, **kw)
    def mean(self, *args, **kw): return self.df.mean(self.expression, *args, **kw)
    def min(self, *args, **kw): return self.df.min(self.expression, *args, **kw)
    def max(self, *args, **kw): return self.df.max(self.expression, *args, **kw)
    def std(self, *args, **kw): return self.df.std(self.expression, *args, **kw)
    def var(self, *args, **kw): return self.df.var(self.expression, *args, **kw)
    def minmax(self, *args, **kw): return self.df.minmax(self.expression, *args, **kw)

    def value_counts(self, dropna=False, dropnan=False, dropmissing=False, ascending=False, progress=False, axis=None):
        """expression.py:946-1061: a pandas Series of the counts of the unique values, most
        frequent first (``ascending=False``); a missing entry is labelled "missing" and comes
        first.  NaN and missing values are reported unless dropped (pandas drops them)."""
        return self.df.value_counts(self.expression, dropna=dropna, dropnan=dropnan, dropmissing=dropmissing,
                                    ascending=ascending, progress=progress, axis=axis)

    def unique(self, dropna=False, dropnan=False, dropmissing=False, selection=None, axis=None, array_type="list",
               delay=False):
        """expression.py:1064-1073."""
        return self.df.unique(self.expression, dropna=dropna, dropnan=dropnan, dropmissing=dropmissing,
                              selection=selection, array_type=array_type, axis=axis, delay=delay)

    def nunique(self, dropna=False, dropnan=False, dropmissing=False, selection=None, axis=None, delay=False):
        """expression.py:1075-1093: ``len(df.x.unique()) == df.x.nunique()``."""
        keys = self.unique(dropna=dropna, dropnan=dropnan, dropmissing=dropmissing, selection=selection, axis=axis,
                           array_type=None, delay=delay)
        if isinstance(keys, Promise):
            return keys.then(len)
        return len(keys)


class StringOperations:
    """``Expression.str``: the string functions that run on the device, each as the reference's
    function form (``functions.py`` ``str_*``) over the expression's text."""

    def __init__(self, expression):
        self.expression = expression

    def _call(self, name, *args):
        e = self.expression
        return Expression(e.df, f"{name}({', '.join([e.expression] + [repr(a) for a in args])})")

    def len(self): return self._call("str_len")
    def byte_length(self): return self._call("str_byte_length")
    def equals(self, other): return self._call("str_equals", other)
    def startswith(self, pat): return self._call("str_startswith", pat)
    def endswith(self, pat): return self._call("str_endswith", pat)

    def contains(self, pat, regex=False):
        if regex:
            raise NotImplementedError("str.contains: regular expressions are not supported (regex=False)")
        return self._call("str_contains", pat)

    # the string-producing functions (strings.TRANSFORMS; csrc/strfn.hip): each gives a string
    # expression again, so they chain (df.s.str.strip().str.lower().str.startswith('id'))
    def lower(self): return self._call("str_lower")
    def upper(self, ascii=False): return self._call("str_upper", ascii) if ascii else self._call("str_upper")
    def slice(self, start=0, stop=None): return self._call("str_slice", start, stop)
    def strip(self, to_strip=None): return self._call("str_strip", to_strip)
    def lstrip(self, to_strip=None): return self._call("str_lstrip", to_strip)
    def rstrip(self, to_strip=None): return self._call("str_rstrip", to_strip)
    def pad(self, width, side="left", fillchar=" "): return self._call("str_pad", width, side, fillchar)
    def ljust(self, width, fillchar=" "): return self._call("str_ljust", width, fillchar)
    def rjust(self, width, fillchar=" "): return self._call("str_rjust", width, fillchar)
    def center(self, width, fillchar=" "): return self._call("str_center", width, fillchar)
    def zfill(self, width): return self._call("str_zfill", width)
    def repeat(self, repeats): return self._call("str_repeat", repeats)

    def cat(self, other):
        e = self.expression
        o = other.expression if isinstance(other, Expression) else repr(other)
        return Expression(e.df, f"str_cat({e.expression}, {o})")

    def replace(self, pat, repl, n=-1, flags=0, regex=False):
        if regex or flags:
            raise NotImplementedError("str.replace: regular expressions are not supported (regex=False, flags=0)")
        return self._call("str_replace", pat, repl, n)


def _ordinal_values(x, ordered_set):
    """functions.py:2441-2448 (host evaluation; the bin kernel fuses it instead)."""
    return ordered_set.map_ordinal(x)


def _host_functions():
    """The functions of the host expression namespace besides ``np``."""
    from .datetime import FUNCTIONS
    ns = {"_ordinal_values": _ordinal_values, "astype": _astype}
    ns.update(FUNCTIONS)
    ns.update(MISSING_FUNCTIONS)
    return ns


# ---- the functions that consume missing values on host chunks, as the reference defines them
# on numpy / np.ma arrays (functions.py:146-268)
def _ismissing(x):
    if np.ma.isMaskedArray(x):
        return np.ma.getmaskarray(x) == 1
    return np.zeros(len(x), dtype=bool)


def _isnan(x):
    """functions.py:238-251: unmasked, False at the missing rows"""
    if np.ma.isMaskedArray(x):
        w = x.data != x.data
        w[np.ma.getmaskarray(x)] = False
        return w
    x = np.asarray(x)
    return x != x


def _isna(x):
    return _isnan(x) | _ismissing(x)


def _fill(x, mask, value, keep_mask=False):
    if not np.any(mask):
        return x if keep_mask or not np.ma.isMaskedArray(x) else x.data
    ar = x.copy() if keep_mask or not np.ma.isMaskedArray(x) else x.data.copy()
    ar[mask] = value
    return ar


def _fillmissing(x, value):
    return _fill(x, _ismissing(x), value) if np.ma.isMaskedArray(x) else x


def _fillnan(x, value):
    """functions.py:165-179: NaN of float arrays replaced; a masked array keeps its mask"""
    if np.ma.getdata(x).dtype.kind != "f":
        return x
    return _fill(x, _isnan(x), value, keep_mask=True)


def _fillna(x, value):
    return _fill(x, _isna(x), value)


MISSING_FUNCTIONS = {"ismissing": _ismissing, "notmissing": lambda x: ~_ismissing(x), "isna": _isna,
                     "notna": lambda x: ~_isna(x), "fillmissing": _fillmissing, "fillnan": _fillnan, "fillna": _fillna,
                     "isnan": _isnan, "notnan": lambda x: ~_isnan(x)}  # what dropnan / dropna filter by


# whether a live datetime64 / timedelta64 column holds NaT: (column reference, answer), the
# column held weakly like the mask cache's (an entry with a dead column goes)
_nat_cache = []


def _astype(x, data_type):
    """functions.py ``astype`` on host chunks (numpy ``ndarray.astype``)."""
    return np.asarray(x).astype(data_type) if not np.ma.isMaskedArray(x) else x.astype(data_type)


class DataFrame:
    def __init__(self, columns, executor=None):
        self.columns = dict(columns)
        self.variables = {}
        self.virtual_columns = {}
        self._categories = {}
        self.selection_histories = {}         # name -> the selections made under it, oldest first
        self.selection_history_indices = {}   # name -> index of the current one, -1: none
        self._filter = None
        self.executor = executor or default_executor
        lengths = {len(v) for v in self.columns.values()}
        if len(lengths) > 1:
            raise ValueError(f"columns have different lengths: {lengths}")
        self._length = lengths.pop() if lengths else 0

    # ---- structure ---------------------------------------------------------------
    def __len__(self):
        if self._filter is None:
            return self._length
        return int(self.count())

    def length_unfiltered(self):
        return self._length

    @property
    def filtered(self):
        return self._filter is not None

    def is_device_resident(self):
        return any(isinstance(c, (DeviceArray, DeviceMaskedArray, DeviceStringArray)) for c in self.columns.values())

    def _is_string(self, expression):
        """Whether the expression is string-valued: a string column (strings.DeviceStringArray),
        or a transform of one / a virtual column of that kind (expr.py ``_string_source``)."""
        expression = str(expression)
        if expression in self.columns:
            return isinstance(self.columns[expression], DeviceStringArray)
        return self._string_plan(expression) is not None

    def _string_plan(self, expression):
        """The plan of a string-valued expression (expr.string_plan), None for any other; a
        frame without string columns has none.  Plans are kept per expression text while the
        frame's structure (which columns are strings, the virtual columns) stays the same, so
        evaluate / data_type / _is_string parse and check an expression once."""
        structure = tuple((k, isinstance(c, DeviceStringArray)) for k, c in self.columns.items())
        if not any(is_string for _, is_string in structure):
            return None
        expression = str(expression)
        key = (structure, tuple(sorted(self.virtual_columns.items())))
        cache = self.__dict__.setdefault("_string_plans", [None, {}])
        if cache[0] != key:
            cache[:] = [key, {}]
        if expression in cache[1]:
            return cache[1][expression]
        from .expr import UnsupportedExpression, string_plan
        try:
            plan = string_plan(self, expression)
        except UnsupportedExpression as e:
            raise NotImplementedError(f"expression {expression!r} over HBM columns: {e}") from None
        if len(cache[1]) > 256:
            cache[1].clear()
        cache[1][expression] = plan
        return plan

    @staticmethod
    def _hidden_name(name):
        """the hidden codes column of the string key ``name`` (a column name or an expression)"""
        if name.isidentifier():
            return f"__str_{name}"
        import hashlib
        return "__str_expr_" + hashlib.sha1(name.encode("utf-8", "surrogatepass")).hexdigest()[:16]

    def get_column_names(self):
        return list(self.columns) + list(self.virtual_columns)

    def copy(self):
        df = DataFrame(self.columns, executor=self.executor)
        df.variables = dict(self.variables)
        df.virtual_columns = dict(self.virtual_columns)
        df._categories = dict(self._categories)
        df._copy_selections(self)
        df._filter = self._filter
        # copies share the filter-mask cache (its entries name the filter and the column objects,
        # so a copy that changes either misses; groupby works on a copy)
        df._filter_mask_cache = self.__dict__.setdefault("_filter_mask_cache", [])
        return df

    def add_column(self, name, data):
        if len(data) != self._length and self.columns:
            raise ValueError("column length mismatch")
        self.columns[name] = data
        if not self._length:
            self._length = len(data)

    def __setitem__(self, name, value):
        if isinstance(value, Expression):
            self.virtual_columns[name] = value.expression
        else:
            self.add_column(name, value)

    def add_virtual_column(self, name, expression):
        self.virtual_columns[name] = str(expression)

    def add_variable(self, name, value, unique=False):
        if unique:
            base, i = name, 0
            while name in self.variables:
                i += 1
                name = f"{base}_{i}"
        self.variables[name] = value
        return name

    def __getitem__(self, item):
        if isinstance(item, Expression) and str(item) not in self.columns and \
                str(item) not in self.virtual_columns and self.data_type(item).kind == "b":
            return self.filter(item)  # df[df.x > 0] (dataframe.py __getitem__: boolean expression = filter)
        if isinstance(item, (str, Expression)):
            return Expression(self, str(item))
        raise TypeError(item)

    def __getattr__(self, name):
        if name.startswith("_") or name in ("columns", "variables", "virtual_columns"):
            raise AttributeError(name)
        if name in self.__dict__.get("columns", {}) or name in self.__dict__.get("virtual_columns", {}):
            return Expression(self, name)
        raise AttributeError(name)

    def filter(self, expression):
        df = self.copy()
        e = str(expression)
        df._filter = e if self._filter is None else f"({self._filter}) & ({e})"
        return df

    def is_category(self, expression):
        return str(expression) in self._categories

    def categorize(self, column, min_value=0, max_value=None, labels=None, inplace=False):
        """dataframe.py:5487-5533: mark an integer column as categorical with N labels."""
        df = self if inplace else self.copy()
        column = str(column)
        if labels is None:
            vmin, vmax = df.minmax(column)
            min_value = int(vmin) if min_value is None else min_value
            max_value = int(vmax) if max_value is None else max_value
            labels = list(range(min_value, max_value + 1))
        N = len(labels)
        df._categories[column] = dict(labels=labels, N=N, min_value=min_value)
        return df

    def category_labels(self, column):
        return self._categories[str(column)]["labels"]

    # ---- evaluation --------------------------------------------------------------
    def _namespace(self, i1, i2, filter_mask=None):
        ns = {"np": np, **_host_functions()}
        for name, col in self.columns.items():
            ns[name] = col
        ns.update(self.variables)
        return ns

    def _eval_host(self, expression, i1, i2, filter_mask=None):
        expression = str(expression)
        if isinstance(filter_mask, DeviceArray):
            # HBM frame: chunks stay whole, the parts apply the filter as a row mask
            filter_mask = None
        if expression in self.columns:
            col = self.columns[expression]
            if isinstance(col, (DeviceArray, DeviceMaskedArray, DeviceStringArray)):
                if filter_mask is not None:
                    raise NotImplementedError("filtered DataFrames need host columns")
                return col[i1:i2]
            block = col[i1:i2]
            return block[filter_mask] if filter_mask is not None else block
        if self.is_device_resident():
            plan = self._string_plan(expression)
            if plan is not None:  # string-valued: a temporary DeviceStringArray of the rows
                from .expr import evaluate_string
                return evaluate_string(self, plan, i1, i2)
            return self._eval_device(expression, i1, i2)
        if expression in self.virtual_columns:
            return self._eval_host(self.virtual_columns[expression], i1, i2, filter_mask)
        ns = {"np": np, **_host_functions()}
        ns.update(self.variables)
        for name, col in self.columns.items():
            if name in expression:
                if isinstance(col, (DeviceArray, DeviceMaskedArray)):
                    raise NotImplementedError(
                        f"expression {expression!r} over an HBM column: only plain columns bin in place")
                ns[name] = col[i1:i2]
        for name, vexpr in self.virtual_columns.items():
            # as a whole word: fillna's virtual column x reads the hidden column __original_x
            if name in expression and re.search(r"(?<![\w.])%s(?!\w)" % re.escape(name), expression):
                ns[name] = self._eval_host(vexpr, i1, i2, None)
        with np.errstate(all="ignore"):
            value = eval(expression, {"__builtins__": {}}, ns)  # noqa: S307 (host-side expressions)
        if np.isscalar(value):
            value = np.full(i2 - i1, value)
        value = np.asarray(value) if not np.ma.isMaskedArray(value) else value
        return value[filter_mask] if filter_mask is not None else value

    def _eval_device(self, expression, i1, i2):
        """An expression over HBM columns, evaluated by the device expression kernel into
        a new HBM column (expr.py); unsupported syntax raises rather than leaving the GPU."""
        from .expr import UnsupportedExpression, compile_expression
        try:
            return compile_expression(self, expression).evaluate(self, i1, i2)
        except UnsupportedExpression as e:
            raise NotImplementedError(f"expression {expression!r} over HBM columns: {e}") from None

    def _eval_device_keep(self, expression, i1, i2):
        """A boolean expression over HBM columns as a row mask (a filter, a selection): a missing
        value selects nothing, so the program is ``value & ~mask`` (expr.Program ``keep``) and the
        result is a plain byte mask.  Without masked operands it is the expression's own program."""
        from .expr import UnsupportedExpression, compile_expression
        try:
            return compile_expression(self, expression, keep=True).evaluate(self, i1, i2)
        except UnsupportedExpression as e:
            raise NotImplementedError(f"expression {expression!r} over HBM columns: {e}") from None

    def _eval_row_mask(self, expression, i1, i2):
        """the device mask of a filter / selection expression: with masked columns in the frame a
        missing value selects nothing (_eval_device_keep), else the expression's own program"""
        if self._has_masked():
            return self._eval_device_keep(expression, i1, i2)
        return self._eval_device(expression, i1, i2)

    def _masked_names(self):
        """the names of the masked HBM columns (DeviceMaskedArray)"""
        return [k for k, c in self.columns.items() if isinstance(c, DeviceMaskedArray)]

    def _has_masked(self):
        return bool(self._masked_names())

    def _refuse_masked(self, what, expressions):
        """NotImplementedError for a method that does not take missing values yet when one of the
        expressions can be missing on an HBM frame: no number is computed as if the mask were
        not there."""
        if not self._has_masked():
            return
        for e in expressions:
            e = _ensure_string(e)
            if e not in (None, "", "*") and not self._is_string(e) and self.is_masked(e):
                reads = [k for k in self._masked_names() if re.search(r"(?<![\w.])%s(?!\w)" % re.escape(k), e)]
                raise NotImplementedError(f"{what} over the masked column {(reads or [e])[0]!r} (expression {e!r}) is "
                                          "not supported: fillmissing / dropmissing first")

    def is_masked(self, column):
        """dataframe.py:2099: whether the column (or expression) can hold missing values: a
        ``np.ma`` host column, a DeviceMaskedArray, or an expression whose program has a mask."""
        column = _ensure_string(column)
        if column in self.columns:
            return np.ma.isMaskedArray(self.columns[column]) or isinstance(self.columns[column], DeviceMaskedArray)
        if self.is_device_resident():
            if self._is_string(column):
                return False
            from .expr import UnsupportedExpression, compile_expression
            try:
                return compile_expression(self, column).mask_code is not None
            except UnsupportedExpression as e:
                raise NotImplementedError(f"expression {column!r} over HBM columns: {e}") from None
        return np.ma.isMaskedArray(self._eval_host(column, 0, min(self._length, 16)))

    def evaluate_chunk(self, expression, i1, i2, filter_mask=None):
        return self._eval_host(expression, i1, i2, filter_mask)

    def evaluate(self, expression, i1=None, i2=None, filtered=True):
        i1 = 0 if i1 is None else i1
        i2 = self._length if i2 is None else i2
        fm = self.evaluate_filter_mask(i1, i2) if (filtered and self.filtered) else None
        if isinstance(fm, DeviceArray):
            # the filtered rows of an HBM frame: an HBM value is compacted on the device
            # (mask_rows + vh_take) and only the kept rows are read back
            v = self._eval_host(expression, i1, i2)
            if isinstance(v, DeviceStringArray):
                from .superutils import mask_rows
                return v.take(mask_rows(fm)).to_numpy()
            if isinstance(v, (DeviceArray, DeviceMaskedArray)):
                from .sort import compact_device
                return compact_device(v, fm).to_numpy()  # a masked value: the kept rows as np.ma
            return np.asarray(v)[fm.to_numpy().astype(bool)]
        return self._eval_host(expression, i1, i2, fm)

    def evaluate_filter_mask(self, i1, i2):
        if self.is_device_resident():
            # the device mask of the filter, per (i1, i2) block, kept while the frame's columns,
            # virtual columns and variables stay the same objects (the reference keeps filter
            # masks per block too: _selection_mask_caches[FILTER_SELECTION_NAME],
            # dataframe.py:4161,5967, dropped by _invalidate_selection_cache)
            return self._cached_device_mask(self._filter, i1, i2)
        return self._expression_mask(self._filter, i1, i2)  # a missing value keeps nothing, as in a selection

    def _cached_device_mask(self, expr, i1, i2, compute=None):
        # An entry is (key, column references, variable values, mask).  A hit needs the frame's
        # current column objects to be the live ones the mask was computed from and its variables
        # to hold the same values: a device pointer or an id() names whatever was allocated there
        # last (the block cache and CPython's free lists hand both out again), so neither is
        # remembered.  Columns are held weakly: a replaced column's HBM is not kept alive here,
        # and an entry with a dead column goes, its mask with it.
        key = (expr, i1, i2, tuple(self.columns), tuple(sorted(self.virtual_columns.items())), tuple(self.variables))
        cols, values = list(self.columns.values()), [_variable_value(v) for v in self.variables.values()]
        cache = self.__dict__.setdefault("_filter_mask_cache", [])
        with _mask_cache_lock:
            cache[:] = [e for e in cache if all(r() is not None for r in e[1])]
            for k, refs, vals, m in cache:
                if k == key and all(r() is c for r, c in zip(refs, cols)) and _same_variables(vals, values):
                    return m
        # expr: the expression string, or (with compute) the hashable form of a selection that
        # is evaluated node by node
        m = self._eval_row_mask(expr, i1, i2) if compute is None else compute()
        with _mask_cache_lock:
            if len(cache) >= 8:
                del cache[:]
            cache.append((key, [_column_ref(c) for c in cols], values, m))
        return m

    def _column_has_nat(self, name):
        """Whether the datetime64 / timedelta64 column ``name`` holds NaT, asked by the device
        expression compiler (expr.py: such a column does not compute on the device).  An HBM
        column answers from a device min / max pass over its int64 bits, once per live column
        object.  Like the mask cache, the answer is not told of writes into a column: a host
        array that gets a NaT written in place afterwards keeps its "no NaT" answer, and the
        device path would then compute an unspecified number for that row.  Columns are treated
        as immutable; replace the column (a new array object) to change its values."""
        from .expr import column_has_nat
        col = self.columns[name]
        with _mask_cache_lock:
            _nat_cache[:] = [e for e in _nat_cache if e[0]() is not None]
            for ref, answer in _nat_cache:
                if ref() is col:
                    return answer
        answer = column_has_nat(col)
        with _mask_cache_lock:
            _nat_cache.append((_column_ref(col), answer))
        return answer

    def data_type(self, expression):
        expression = str(expression)
        if self._is_string(expression):
            return STRING
        if expression in self.columns:
            return np.dtype(self.columns[expression].dtype)
        if self.is_device_resident():
            from .expr import UnsupportedExpression, compile_expression
            try:
                return compile_expression(self, expression).dtype
            except UnsupportedExpression as e:
                raise NotImplementedError(f"expression {expression!r} over HBM columns: {e}") from None
        v = self._eval_host(expression, 0, min(self._length, 16))
        return np.dtype(v.dtype)

    def _resolve_selection(self, selection):
        """A ``selection=`` argument (True / a name / an expression string / an Expression / a
        Selection object) as an expression string, or as the Selection when its chain does not
        fold into one (it holds a lasso, or a drop-na on a host frame)."""
        if selection is True:
            selection = "default"
        if isinstance(selection, str):
            selection = self.get_selection(selection) or selection
        if isinstance(selection, selections.Selection):
            folded = selection.fold(self)
            return selection if folded is None else folded
        return str(selection)

    def device_keep_mask(self, i1, i2, selection=None, invert=False, cache=False):
        """HBM frame: one device mask of the rows a part takes (filter & selection), or its
        complement (invert: the skip mask of the min/max kernel); None = every row.  cache:
        kept per block like the filter mask (the reference's aggregation parts ask for cached
        selection masks, cpu.py:548).  A selection that folds into an expression is evaluated
        with the filter as one device program; one that holds a lasso node by node
        (``Selection.evaluate_device``), the filter's mask and-ed in after."""
        parts = []
        if self._filter is not None:
            parts.append(f"({self._filter})")
        if selection not in (None, False):
            selection = self._resolve_selection(selection)
            if isinstance(selection, selections.Selection):
                return self._device_selection_mask(selection, i1, i2, invert, cache)
            parts.append(f"({selection})")
        if not parts:
            return None
        expr = " & ".join(parts)
        if invert and self._has_masked():
            # a missing value selects nothing: the skip mask is ~(value & ~mask), so the keep
            # program is complemented as a mask, not the expression before it is compiled
            from .superutils import mask_combine

            def compute():
                return mask_combine(self._eval_device_keep(expr, i1, i2), None)
            return self._cached_device_mask(("skip", expr), i1, i2, compute) if cache else compute()
        expr = f"~({expr})" if invert else expr
        return self._cached_device_mask(expr, i1, i2) if cache else self._eval_row_mask(expr, i1, i2)

    def _device_selection_mask(self, selection, i1, i2, invert, cache):
        from .superutils import mask_combine

        def compute():
            mask = selection.evaluate_device(self, i1, i2)
            if self._filter is not None:
                mask = mask_combine(self.evaluate_filter_mask(i1, i2), mask, "and")
            return mask_combine(mask, None) if invert else mask

        if not cache:
            return compute()
        return self._cached_device_mask(("selection", selection.key(), self._filter, invert), i1, i2, compute)

    def _expression_mask(self, expression, i1, i2, filter_mask=None):
        """Host frame: a boolean expression over the rows that pass filter_mask, as a bool
        array; a masked value selects nothing."""
        mask = self._eval_host(str(expression), i1, i2, filter_mask)
        if np.ma.isMaskedArray(mask):
            mask = mask.data & ~np.ma.getmaskarray(mask)
        return np.asarray(mask, dtype=bool)

    # ---- selections --------------------------------------------------------------
    @property
    def selection_expressions(self):
        """{name: expression} of the current selections whose chain holds only expressions and
        inversions, folded into one string (``Selection.fold``)."""
        out = {}
        for name in self.selection_histories:
            selection = self.get_selection(name)
            folded = selection.fold() if selection is not None else None
            if folded is not None:
                out[name] = folded
        return out

    def _selection_dependencies(self):
        """Every expression a current selection is evaluated from (a lasso's x / y included)."""
        return [e for name in self.selection_histories if self.get_selection(name) is not None
                for e in self.get_selection(name).dependencies()]

    def _copy_selections(self, other):
        self.selection_histories = {k: list(v) for k, v in other.selection_histories.items()}
        self.selection_history_indices = dict(other.selection_history_indices)

    def get_selection(self, name="default"):
        """The current Selection object under ``name``, or None."""
        index = self.selection_history_indices.get(name, -1)
        return None if index == -1 else self.selection_histories[name][index]

    def has_selection(self, name="default"):
        return self.get_selection(name) is not None

    def _selection(self, create_selection, name):
        """dataframe.py:4937-4951: the new selection is built on the current one and appended
        after it; what could be redone is dropped.  (After undoing every selection the
        reference builds on the LAST entry of the history; here on none.)"""
        history = self.selection_histories.setdefault(name, [])
        index = self.selection_history_indices.get(name, -1)
        selection = create_selection(history[index] if index >= 0 else None)
        del history[index + 1:]
        history.append(selection)
        self.selection_history_indices[name] = index + 1

    def selection_undo(self, name="default"):
        if not self.selection_can_undo(name):
            raise ValueError(f"selection {name!r} has nothing to undo")
        self.selection_history_indices[name] -= 1

    def selection_redo(self, name="default"):
        if not self.selection_can_redo(name):
            raise ValueError(f"selection {name!r} has nothing to redo")
        self.selection_history_indices[name] += 1

    def selection_can_undo(self, name="default"):
        return self.selection_history_indices.get(name, -1) > -1

    def selection_can_redo(self, name="default"):
        return self.selection_history_indices.get(name, -1) + 1 < len(self.selection_histories.get(name, []))

    def select(self, boolean_expression, mode="replace", name="default"):
        """dataframe.py:4712-4730: select the rows where the boolean expression holds, combined
        with the current selection under ``name`` by ``mode`` (replace / and / or / xor /
        subtract).  Selections are recorded per name (``selection_undo`` / ``selection_redo``).
        ``None`` clears the selection; it is not recorded when there is none to clear."""
        selections._check_mode(mode)
        boolean_expression = _ensure_string(boolean_expression)
        if boolean_expression is None and not self.has_selection(name):
            return

        def create(current):
            return selections.SelectionExpression(boolean_expression, current, mode) if boolean_expression else None
        self._selection(create, name)

    def select_nothing(self, name="default"):
        self.select(None, name=name)

    def select_inverse(self, name="default"):
        """Select what is not selected (ValueError when nothing is)."""
        self._selection(selections.SelectionInvert, name)

    def select_non_missing(self, drop_nan=True, drop_masked=True, column_names=None, mode="replace", name="default"):
        """dataframe.py:4732-4748: the rows without a NaN (float columns) / masked value in any
        of ``column_names`` (default: every real column)."""
        column_names = _ensure_strings(list(column_names or self.columns))
        self._selection(lambda current: selections.SelectionDropNa(drop_nan, drop_masked, column_names, current, mode),
                        name)

    def _drop(self, column_names, missing, nan):
        """dataframe.py:4750-4789 ``_filter_all``: a copy whose filter also asks every named column
        (default: every real column) to be there: ``notmissing(c)`` for the columns that can be
        missing, ``~isnan(c)`` for the float ones -- a conjunction, so on an HBM frame the filter
        stays one device program."""
        names = _ensure_strings(list(column_names)) if column_names is not None else list(self.columns)
        terms = []
        for c in names:
            if self._is_string(c):
                continue  # string columns hold neither nulls nor NaN
            if missing and self.is_masked(c):
                terms.append(f"notmissing({c})")
            if nan and self.data_type(c).kind == "f":
                terms.append(f"~isnan({c})")
        return self.filter(" & ".join(terms)) if terms else self.copy()

    def dropmissing(self, column_names=None):
        """dataframe.py:4750: the rows without a missing value in ``column_names``."""
        return self._drop(column_names, True, False)

    def dropnan(self, column_names=None):
        """dataframe.py:4758: the rows without a NaN in ``column_names``."""
        return self._drop(column_names, False, True)

    def dropna(self, column_names=None):
        """dataframe.py:4766: the rows with neither a missing value nor a NaN in ``column_names``."""
        return self._drop(column_names, True, True)

    def fillna(self, value, column_names=None, prefix="__original_", inplace=False):
        """dataframe.py:4595: missing values and NaN of the named columns (default: every real
        column that can hold either) replaced by ``value``.  Each such column becomes the virtual
        column ``fillna(__original_<name>, value)``; the original moves to that hidden name, so
        no data is lost.  On an HBM frame the value must fit the column's dtype (expr.py
        ``fillmissing``)."""
        df = self if inplace else self.copy()
        names = _ensure_strings(list(column_names)) if column_names is not None else list(df.columns)
        for name in names:
            if name not in df.columns:
                raise KeyError(f"fillna: {name!r} is not a real column")
            if df._is_string(name) or name.startswith(prefix):
                continue
            if column_names is None and not (df.is_masked(name) or df.data_type(name).kind == "f"):
                continue  # holds neither missing values nor NaN
            hidden = prefix + name
            df.columns = {(hidden if k == name else k): v for k, v in df.columns.items()}
            df.virtual_columns[name] = f"fillna({hidden}, {_literal(value)})"
        return df

    def select_rectangle(self, x, y, limits, mode="replace", name="default"):
        """dataframe.py:4794-4806: ``select_box([x, y], [(x1, x2), (y1, y2)])``."""
        self.select_box([x, y], limits, mode=mode, name=name)

    def select_box(self, spaces, limits, mode="replace", name="default"):
        """dataframe.py:4808-4825: the n-dimensional box ``[(x1, x2), (y1, y2), ...]``, both ends
        included.  As in the reference the limits enter the expression through ``%f``: six
        digits after the point, so a limit is rounded to 1e-6 and one beyond about 1e15 loses
        its low digits."""
        sorted_limits = [(min(l), max(l)) for l in limits]
        expressions = ["((%s) >= %f) & ((%s) <= %f)" % (expression, lmin, expression, lmax) for
                       (expression, (lmin, lmax)) in zip(_ensure_strings(list(spaces)), sorted_limits)]
        self.select("&".join(expressions), mode=mode, name=name)

    def select_circle(self, x, y, xc, yc, r, mode="replace", name="default", inclusive=True):
        """dataframe.py:4827-4851: ``(x - xc)**2 + (y - yc)**2 <= r**2`` (``<`` when not
        inclusive); the constants enter with ``repr()`` and so keep every bit."""
        x, y = _ensure_string(x), _ensure_string(y)
        xc, yc, r2 = repr(float(xc)), repr(float(yc)), repr(float(r) ** 2)
        op = "<=" if inclusive else "<"
        self.select(f"((({x}) - {xc}) ** 2 + (({y}) - {yc}) ** 2) {op} {r2}", mode=mode, name=name)

    def select_ellipse(self, x, y, xc, yc, width, height, angle=0, mode="replace", name="default", radians=False,
                       inclusive=True):
        """dataframe.py:4853-4894: the ellipse centred on (xc, yc) with the diameters width and
        height, turned by ``angle`` (degrees unless ``radians``; the reference leaves the angle
        undefined for ``radians=True``).  Constants enter with ``repr()``."""
        x, y = _ensure_string(x), _ensure_string(y)
        alpha = float(angle) if radians else float(np.deg2rad(angle))
        xr, yr = width / 2, height / 2
        r = max(xr, yr)
        a2, b2, r2 = repr(float((xr / r) ** 2)), repr(float((yr / r) ** 2)), repr(float(r) ** 2)
        cos, sin = repr(float(np.cos(alpha))), repr(float(np.sin(alpha)))
        dx, dy = f"(({x}) - {float(xc)!r})", f"(({y}) - {float(yc)!r})"
        op = "<=" if inclusive else "<"
        self.select(f"(({dx} * {cos} + {dy} * {sin}) ** 2 / {a2} + ({dx} * {sin} - {dy} * {cos}) ** 2 / {b2}) {op} {r2}",
                    mode=mode, name=name)

    def select_lasso(self, expression_x, expression_y, xsequence, ysequence, mode="replace", name="default"):
        """dataframe.py:4896-4911: the rows whose (x, y) lies inside the polygon with the
        vertices (xsequence[k], ysequence[k]), the reference's pnpoly test.  On an HBM frame it
        runs as one kernel over the two columns; only the vertices go to the device."""
        expression_x, expression_y = _ensure_string(expression_x), _ensure_string(expression_y)
        self._selection(lambda current: selections.SelectionLasso(expression_x, expression_y, xsequence, ysequence,
                                                                  current, mode), name)

    def set_selection(self, selection, name="default"):
        """Make the Selection object the current selection under ``name``."""
        self._selection(lambda current: selection, name)

    def selected_length(self, selection="default"):
        """The number of selected rows (dataframe.py:6612-6614)."""
        return int(np.asarray(self.count(selection=selection)).item())

    def evaluate_selection_mask(self, selection, i1=0, i2=None, filter_mask=None, cache=False):
        i2 = self._length if i2 is None else i2
        if isinstance(filter_mask, DeviceArray) or (filter_mask is None and self.is_device_resident()):
            # HBM frame: the device mask of (filter &) selection over the whole chunk
            return self.device_keep_mask(i1, i2, selection, cache=cache)
        selection = self._resolve_selection(selection)
        if isinstance(selection, selections.Selection):
            return selection.evaluate(self, i1, i2, filter_mask)
        return self._expression_mask(selection, i1, i2, filter_mask)

    # ---- execution ---------------------------------------------------------------
    def execute(self):
        self.executor.execute()

    def _delay(self, delay, value):
        if delay:
            return value
        self.execute()
        return value.get() if isinstance(value, Promise) else value

    # ---- binners -----------------------------------------------------------------
    def _binner_scalar(self, expression, limits, shape):
        return BinnerScalar(expression, limits[0], limits[1], shape, self.data_type(expression))

    def _binner_ordinal(self, expression, ordinal_count, min_value=0):
        if str(expression).startswith("_ordinal_values("):
            from .taskparts import parse_ordinal_values
            key_expr, _ = parse_ordinal_values(expression)
            dtype = self.data_type(key_expr)
        else:
            dtype = self.data_type(expression)
        return BinnerOrdinal(expression, min_value, ordinal_count, dtype)

    def _binner(self, expression, limits=None, shape=None, selection=None):
        """dataframe.py:5251-5265 (limits resolved eagerly)."""
        expression = str(expression)
        if expression in self._categories:
            N = self._categories[expression]["N"]
            min_value = self._categories[expression]["min_value"]
            return self._binner_ordinal(expression, N, min_value)
        lim = self.limits(expression, limits, selection=selection)
        return self._binner_scalar(expression, lim, shape)

    def _create_binners(self, binby, limits, shape, selection=None):
        """dataframe.py:5275-5295."""
        binbys = binby if isinstance(binby, (list, tuple)) else [binby]
        binbys = [str(b) for b in _ensure_strings(binbys) if b is not None and str(b) != ""]
        limits = _expand_limits(limits, len(binbys)) if binbys else []
        shapes = _expand_shape(shape, len(binbys))
        return tuple(self._binner(b, l, s, selection) for b, l, s in zip(binbys, limits, shapes))

    # ---- limits ------------------------------------------------------------------
    def limits(self, expression, value=None, square=False, selection=None, delay=False, shape=None):
        """dataframe.py:1617-1699 for one expression: explicit [lo, hi], 'minmax' (the GPU
        min/max pre-pass) and percentages ('99.7%', '90percent'; the '%s' / 'percentsquare'
        forms too, whose square flag the reference ignores).  'Nsigma' raises like the
        reference, which calls a limits_sigma it does not define."""
        if value is None or (isinstance(value, str) and value == "minmax"):
            vmin, vmax = self.minmax(expression, selection=selection)
            return [vmin, vmax]
        if isinstance(value, str):
            match = re.match(r"([\d.]*)(\D*)", value)
            number, kind = match.groups()
            kind = kind.strip()
            if kind in ("%", "percent", "%s", "%square", "percentsquare"):
                return list(self.limits_percentage(expression, ast.literal_eval(number), selection=selection))
            if kind in ("s", "sigma", "ss", "sigmasquare"):
                raise AttributeError("'DataFrame' object has no attribute 'limits_sigma'")
            raise ValueError("limit %r not understood" % value)
        return list(value)

    def limits_percentage(self, expression, percentage=99.73, square=False, selection=False, delay=False):
        """dataframe.py:1570-1614: the range around the median holding about `percentage` %
        of the rows, read off the cumulative 16384-bin histogram over [min, max] (both
        passes on the GPU)."""
        waslist, [expressions] = listify(_ensure_strings(expression))
        sel = None if selection in (None, False) else selection
        out = []
        for expr in expressions:
            vmin, vmax = self.minmax(expr, selection=sel)
            size = 1024 * 16
            counts = np.asarray(self.count(binby=expr, shape=size, limits=[vmin, vmax], selection=selection))
            cumcounts = np.concatenate([[0], np.cumsum(counts)])
            cumcounts = cumcounts / cumcounts.max()
            f = (1 - percentage / 100.) / 2
            x = np.linspace(vmin, vmax, size + 1)
            out.append(np.interp([f, 1 - f], cumcounts, x))
        return unlistify(waslist, out)

    def median_approx(self, expression, percentage=50., binby=[], limits=None, shape=default_shape,
                      percentile_shape=256, percentile_limits="minmax", selection=False, delay=False):
        """dataframe.py:1399-1416: the approximate median (always the 50th percentile, whatever
        ``percentage`` says, like the reference), possibly on a grid defined by binby."""
        return self.percentile_approx(expression, 50, binby=binby, limits=limits, shape=shape,
                                      percentile_shape=percentile_shape, percentile_limits=percentile_limits,
                                      selection=selection, delay=delay)

    def percentile_approx(self, expression, percentage=50., binby=[], limits=None, shape=default_shape,
                          percentile_shape=1024, percentile_limits="minmax", selection=False, delay=False):
        """dataframe.py:1419-1555: the percentile(s) given by ``percentage``, read off the
        cumulative histogram of the expression over ``percentile_limits`` in ``percentile_shape``
        bins, possibly per cell of a grid defined by binby.  The count grid
        (binby + [expression], with edges) stays in HBM and is finished there
        (``Aggregator.percentile``); only the percentiles are read back.

        A scalar percentage gives the outer (binby) shape, a list of percentages
        ``(len(percentage),) + outer``, a list of expressions a leading axis over them.  Unlike
        the reference (which returns a ragged list there), percentages 0 and 100 with binby are
        broadcast to the outer shape."""
        from . import hostops
        from .taskparts import DeviceResult
        waslist, [expressions] = listify(_ensure_strings(expression))
        binbys = binby if isinstance(binby, (list, tuple)) else [binby]
        binbys = [str(b) for b in _ensure_strings(binbys) if b is not None and str(b) != ""]
        self._refuse_masked("percentile_approx / median_approx", expressions + binbys)
        waslist_percentage, [percentages] = listify(percentage)
        percentages = [float(p) for p in percentages]
        sel = None if selection in (None, False) else selection
        percentile_shapes = _expand_shape(percentile_shape, len(expressions))
        if percentile_limits:
            percentile_limits = _expand_limits(percentile_limits, len(expressions))
        else:
            percentile_limits = (None,) * len(expressions)
        outer = self._create_binners(binbys, limits, shape, selection=sel)
        counts, plimits = [], []
        for expr, pshape, plim in zip(expressions, percentile_shapes, percentile_limits):
            plim = [float(v) for v in self.limits(expr, plim, selection=sel)]
            # count(*) over binby + [expression] with edges; keep_device: the part returns the
            # aggregator (a DeviceResult), its grid still in HBM
            desc = vagg.count(selection=sel, edges=True)
            desc.keep_device = True
            counts.append(desc.add_tasks(self, outer + (self._binner_scalar(expr, plim, pshape),))[1])
            plimits.append(plim)

        @delayed
        def finish(*grids):
            results = []
            for grid, (lo, hi) in zip(grids, plimits):
                if isinstance(grid, DeviceResult):
                    value = grid.agg.percentile(percentages, lo, hi)
                else:  # keep_device not honoured: the same arithmetic on the host grid
                    value = hostops.percentile_finish(np.asarray(grid), percentages, lo, hi)
                results.append(unlistify(waslist_percentage, value))
            return unlistify(waslist, np.array(results))

        return self._delay(delay, finish(*counts))

    def mutual_information(self, x, y=None, mi_limits=None, mi_shape=256, binby=[], limits=None, shape=default_shape,
                           sort=False, selection=False, delay=False):
        """dataframe.py:622-718: the mutual information between x and y, estimated on a grid of
        ``mi_shape`` bins over ``mi_limits``, possibly per cell of a grid defined by binby.  The
        count grid ([x, y] + binby, with edges) stays in HBM and is finished there
        (``Aggregator.mutual_information``); one float64 per binby cell is read back.

        ``x`` with ``y`` is one pair (a 0-d result, or the binby shape); two equally long lists, or
        a list of pairs in ``x`` alone, give a leading axis over the pairs.  ``mi_limits``:
        ``[[xlo, xhi], [ylo, yhi]]`` (or ``"minmax"``, the default) for every pair, or a list of
        those, one per pair.  ``sort=True`` returns the values in descending order and the pairs
        in that order; combined with binby it raises ValueError (the reference's argsort over
        the per-cell values does not order pairs).  Unlike the reference, binby is not limited
        to 3 axes.  The limits of an expression are resolved once per call, however many pairs
        it occurs in."""
        from . import hostops
        from .taskparts import DeviceResult
        if y is None:
            waslist, [pairs] = listify(x)
        else:
            waslist, [xs, ys] = listify(x, y)
            if len(xs) != len(ys):
                raise ValueError("x and y hold %d and %d expressions" % (len(xs), len(ys)))
            pairs = list(zip(xs, ys))
        for pair in pairs:
            if not _issequence(pair) or len(pair) != 2:
                raise ValueError("mutual_information wants pairs of expressions, not %r" % (pair,))
        pairs = [_ensure_strings(list(pair)) for pair in pairs]
        self._refuse_masked("mutual_information", [e for pair in pairs for e in pair] + list(listify(binby)[1][0]))

        def one_pair_limits(value):  # [xlim, ylim], each None, a string or [lo, hi]
            return _issequence(value) and len(value) == 2 and all(
                v is None or isinstance(v, str) or (_issequence(v) and len(v) == 2 and not _issequence(v[0]))
                for v in value)

        if mi_limits is None or isinstance(mi_limits, str) or one_pair_limits(mi_limits):
            pair_limits = [_expand_limits(mi_limits, 2)] * len(pairs)
        else:
            if len(mi_limits) != len(pairs):
                raise ValueError("mi_limits holds %d entries for %d pairs" % (len(mi_limits), len(pairs)))
            pair_limits = [_expand_limits(lim, 2) for lim in mi_limits]
        mi_shapes = _expand_shape(mi_shape, 2)
        binbys = binby if isinstance(binby, (list, tuple)) else [binby]
        binbys = [str(b) for b in _ensure_strings(binbys) if b is not None and str(b) != ""]
        if sort and binbys:
            raise ValueError("sort=True orders scalar values: it cannot be combined with binby")
        sel = None if selection in (None, False) else selection
        outer = self._create_binners(binbys, limits, shape, selection=sel)
        resolved = {}  # (expression, limit) -> [lo, hi]: one min/max pass per distinct one

        def axis_limits(e, lim):
            key = (e, lim if lim is None or isinstance(lim, str) else tuple(float(v) for v in lim))
            if key not in resolved:
                resolved[key] = [float(v) for v in self.limits(e, lim, selection=sel)]
            return resolved[key]

        counts = []
        for pair, plims in zip(pairs, pair_limits):
            axes = tuple(self._binner_scalar(e, axis_limits(e, lim), s) for e, lim, s in zip(pair, plims, mi_shapes))
            # count(*) over [x, y] + binby with edges; keep_device: the part returns the
            # aggregator (a DeviceResult), its grid still in HBM
            desc = vagg.count(selection=sel, edges=True)
            desc.keep_device = True
            counts.append(desc.add_tasks(self, axes + outer)[1])

        @delayed
        def finish(*grids):
            values = []
            for grid in grids:
                if isinstance(grid, DeviceResult):
                    values.append(grid.agg.mutual_information())
                else:  # keep_device not honoured: the same arithmetic on the host grid
                    values.append(hostops.mutual_information_finish(np.asarray(grid)))
            if sort:
                mi_list = np.array(values)
                indices = np.argsort(mi_list)[::-1]
                return mi_list[indices], [pairs[k] for k in indices]
            return np.array(unlistify(waslist, values))

        return self._delay(delay, finish(*counts))

    def minmax(self, expression, binby=[], limits=None, shape=default_shape, selection=False, delay=False,
               progress=None):
        """dataframe.py:1276-1333: NaN-ignoring min/max, cast back to the column dtype.  With
        binby, per cell of the grid (the last dimension holds [min, max]); an empty cell reads
        [inf, -inf], the OP_MIN_MAX initial values (tasks.py:173-185)."""
        if binby:
            return self._minmax_binby(expression, binby, limits, shape, selection, delay)
        expression = _ensure_strings(expression)
        waslist, [expressions] = listify(expression)
        sel = selection if selection not in (None, False) else None
        dtype0 = self.data_type(expressions[0])
        if dtype0.kind in "mM":
            # datetime64 / timedelta64 scalars of the column's unit, exact: the min / max
            # aggregators keep int64 (the float64 pre-pass below rounds ns ticks of this century
            # to 256 ns)
            parts = [(self.min(e, selection=selection, delay=True), self.max(e, selection=selection, delay=True))
                     for e in expressions]

            @delayed
            def finish_time(*values):
                v = np.array([np.asarray(x)[()] for x in values]).reshape(len(expressions), 2)
                return unlistify(waslist, v) if waslist else v[0]

            return self._delay(delay, finish_time(*[p for pair in parts for p in pair]))
        tasks = [self.executor.schedule(TaskMinMax(self, str(e), sel)) for e in expressions]

        @delayed
        def finish(*values):
            v = np.array(values)
            if dtype0.kind in "iu" and not np.isnan(v).any():
                v = v.astype(dtype0)
            return unlistify(waslist, v) if waslist else v[0]

        return self._delay(delay, finish(*tasks))

    def _minmax_binby(self, expression, binby, limits, shape, selection, delay):
        waslist, [expressions] = listify(_ensure_strings(expression))
        dtypes = [self.data_type(e) for e in expressions]
        if any(d.kind != dtypes[0].kind for d in dtypes):
            raise TypeError("cannot mix different dtypes in 1 minmax call")
        kw = dict(binby=binby, limits=limits, shape=shape, selection=selection, delay=True)
        parts = [(self.min(e, **kw), self.max(e, **kw), self.count(e, **kw)) for e in expressions]
        self.execute()
        values = []
        for mn, mx, cnt in parts:
            mn, mx, cnt = (np.asarray(p.get()) for p in (mn, mx, cnt))
            v = np.stack([mn.astype(np.float64), mx.astype(np.float64)], axis=-1)
            v[cnt == 0] = [np.inf, -np.inf]
            values.append(v)
        value = unlistify(waslist, np.array(values))
        return self._delay(delay, np.asarray(value).astype(dtypes[0]))

    # ---- aggregations ------------------------------------------------------------
    def _compute_agg(self, name, expression, binby=[], limits=None, shape=default_shape, selection=False,
                     delay=False, edges=False, progress=None, extra_expressions=None, array_type=None):
        """dataframe.py:741-827."""
        expression = _ensure_strings(expression)
        if extra_expressions:
            extra_expressions = _ensure_strings(extra_expressions)
        waslist, [expressions] = listify(expression)
        sel = None if selection is False else selection
        binners = self._create_binners(binby, limits, shape, selection=sel)
        results = []
        for expr in expressions:
            if self._is_string(expr):
                if name != "count":  # a string column has no nulls: its count is the row count
                    raise TypeError(f"{name} of the string column {expr!r}: numeric aggregators take numbers")
                expr = "*"
            if expr in ("*", None):
                aggd = vagg.aggregates[name](selection=sel, edges=edges)
            elif extra_expressions:
                aggd = vagg.aggregates[name](expr, *extra_expressions, selection=sel, edges=edges)
            else:
                aggd = vagg.aggregates[name](expr, selection=sel, edges=edges)
            _, result = aggd.add_tasks(self, binners)
            results.append(result)

        @delayed
        def finish(*counts):
            counts = [np.asarray(c) for c in counts]
            if array_type == "list":
                return unlistify(waslist, np.asarray(counts) if waslist else counts[0]).tolist()
            return np.asarray(counts) if waslist else counts[0]

        return self._delay(delay, finish(*results))

    def count(self, expression=None, binby=[], limits=None, shape=default_shape, selection=False, delay=False,
              edges=False, progress=None, array_type=None):
        """dataframe.py:830-853 (None or '*' counts rows, an expression counts non-NaN values)."""
        return self._compute_agg("count", "*" if expression is None else expression, binby, limits, shape, selection,
                                 delay, edges, progress, array_type=array_type)

    def sum(self, expression, binby=[], limits=None, shape=default_shape, selection=False, delay=False,
            progress=None, edges=False, array_type=None):
        return self._compute_agg("sum", expression, binby, limits, shape, selection, delay, edges, progress,
                                 array_type=array_type)

    def mean(self, expression, binby=[], limits=None, shape=default_shape, selection=False, delay=False,
             progress=None, edges=False, array_type=None):
        return self._compute_agg("mean", expression, binby, limits, shape, selection, delay, edges, progress,
                                 array_type=array_type)

    def min(self, expression, binby=[], limits=None, shape=default_shape, selection=False, delay=False,
            progress=None, edges=False, array_type=None):
        return self._compute_agg("min", expression, binby, limits, shape, selection, delay, edges, progress,
                                 array_type=array_type)

    def max(self, expression, binby=[], limits=None, shape=default_shape, selection=False, delay=False,
            progress=None, edges=False, array_type=None):
        return self._compute_agg("max", expression, binby, limits, shape, selection, delay, edges, progress,
                                 array_type=array_type)

    def std(self, expression, binby=[], limits=None, shape=default_shape, selection=False, delay=False,
            progress=None, edges=False, array_type=None):
        return self._compute_agg("std", expression, binby, limits, shape, selection, delay, edges, progress,
                                 array_type=array_type)

    def var(self, expression, binby=[], limits=None, shape=default_shape, selection=False, delay=False,
            progress=None, edges=False, array_type=None):
        return self._compute_agg("var", expression, binby, limits, shape, selection, delay, edges, progress,
                                 array_type=array_type)

    def _cov_values(self, pairs, binby, limits, shape, selection):
        """One AggCov per expression list in ``pairs`` on the shared binby grid: the delayed
        covariance matrices ``outer + (N, N)`` (one pass over the columns for all of them)."""
        from . import hostops
        sel = None if selection is False else selection
        self._refuse_masked("cov / covar / correlation", [e for expressions in pairs for e in expressions] + list(listify(binby)[1][0]))
        binners = self._create_binners(binby, limits, shape, selection=sel)
        results = []
        for expressions in pairs:
            N = len(expressions)
            _, values = vagg._cov(list(expressions), selection=sel).add_tasks(self, binners)
            results.append(delayed(lambda v, N=N: hostops.cov_finish(np.asarray(v), N))(values))
        return results

    def cov(self, x, y=None, binby=[], limits=None, shape=default_shape, selection=False, delay=False, progress=None):
        """dataframe.py:1192-1272: the covariance matrix of x and y, or of the expressions in the
        sequence x, possibly per cell of a grid defined by binby: shape ``outer + (N, N)``.
        One fused pass (AggCov) over the N columns and the binby columns; the cell of a row
        comes from the binners every other method here uses."""
        selection = _ensure_strings(selection)
        if y is None:
            if not isinstance(x, (list, tuple, np.ndarray)):
                raise ValueError("if y argument is not given, x is expected to be sequence, not %r" % (x,))
            expressions = list(x)
        else:
            expressions = [x, y]
        expressions = _ensure_strings(expressions)
        [value] = self._cov_values([expressions], binby, limits, shape, selection)
        return self._delay(delay, value)

    def covar(self, x, y, binby=[], limits=None, shape=default_shape, selection=False, delay=False, progress=None):
        """dataframe.py:1067-1118: the covariance cov[x, y] = mean(x * y) - mean(x) * mean(y),
        possibly on a grid defined by binby; lists in x and y give a leading axis.  It is
        element ``[..., 0, 1]`` of :meth:`cov`'s fused pass: the means over the non-NaN values of
        each column, mean(x * y) over the rows where both are non-NaN; no product column is
        formed.  Unlike the reference, whose count of the product column drops a row where
        ``x * y`` is NaN although neither factor is (``inf * 0``), that row stays in the pair
        count here."""
        waslist, [xlist, ylist] = listify(_ensure_strings(x), _ensure_strings(y))
        selection = _ensure_strings(selection)
        covs = self._cov_values(list(zip(xlist, ylist)), binby, limits, shape, selection)

        @delayed
        def finish(*covs):
            return np.array(unlistify(waslist, [c[..., 0, 1] for c in covs]))

        return self._delay(delay, finish(*covs))

    def correlation(self, x, y=None, binby=[], limits=None, shape=default_shape, sort=False, sort_key=np.abs,
                    selection=False, delay=False, progress=None):
        """dataframe.py:1121-1189: the correlation coefficient cov[x, y] / (std[x] * std[y]),
        possibly on a grid defined by binby.  With y None, x is a pair or a list of pairs; with
        ``sort`` the result is ``(correlations[indices], sorted_x)``, ordered by descending
        ``sort_key``.  Each pair is one AggCov (N = 2) on the shared grid."""
        if y is None:
            if not isinstance(x, (tuple, list)):
                raise ValueError("if y not given, x is expected to be a list or tuple, not %r" % x)
            if _issequence(x) and not _issequence(x[0]) and len(x) == 2:
                x = [x]
            if not (_issequence(x) and all([_issequence(k) and len(k) == 2 for k in x])):
                raise ValueError("if y not given, x is expected to be a list of lists with length 2, not %r" % x)
            waslist = True
            xlist, ylist = zip(*x)
        else:
            waslist, [xlist, ylist] = listify(x, y)
        xlist = _ensure_strings(list(xlist))
        ylist = _ensure_strings(list(ylist))
        selection = _ensure_strings(selection)
        covs = self._cov_values(list(zip(xlist, ylist)), binby, limits, shape, selection)

        @delayed
        def finish(*covs):
            with np.errstate(divide="ignore", invalid="ignore"):  # nan for an empty cell is fine
                correlations = [c[..., 0, 1] / (c[..., 0, 0] * c[..., 1, 1]) ** 0.5 for c in covs]
            if sort:
                correlations = np.array(correlations)
                indices = np.argsort(sort_key(correlations) if sort_key else correlations)[::-1]
                sorted_x = list([x[k] for k in indices])
                return correlations[indices], sorted_x
            return np.array(unlistify(waslist, correlations))

        return self._delay(delay, finish(*covs))

    def first(self, expression, order_expression, binby=[], limits=None, shape=default_shape, selection=False,
              delay=False, edges=False, progress=None, array_type=None):
        return self._compute_agg("first", expression, binby, limits, shape, selection, delay, edges, progress,
                                 extra_expressions=[order_expression], array_type=array_type)

    def _agg(self, aggregator, binners=(), delay=False, progress=None):
        """dataframe.py:5232-5249."""
        tasks, result = aggregator.add_tasks(self, binners)
        return self._delay(delay, result)

    def _set(self, expression, progress=False, selection=None, flatten=True, delay=False, unique_limit=None,
             return_inverse=False):
        """dataframe.py:474-480: the GPU ordered set of an expression's values."""
        task = self.executor.schedule(TaskSetCreate(self, str(expression), unique_limit=unique_limit,
                                                    selection=selection))
        return self._delay(delay, task)

    def _key_dtype(self, expression):
        """The dtype an expression's set / counter keys are handed back as (datetimes are
        hashed as int64)."""
        dt = self.data_type(expression)
        return dt.newbyteorder("=") if dt.byteorder not in "<=|" else dt

    def value_counts(self, expression, dropna=False, dropnan=False, dropmissing=False, ascending=False, progress=False,
                     axis=None, selection=None, delay=False):
        """Expression.value_counts (expression.py:946-1061) over the GPU counter: the column is
        counted in one pass and the drop / sort-by-count finish runs on the device."""
        from pandas import Series
        if axis is not None:
            raise ValueError("only axis=None is supported")
        if dropna:
            dropnan = dropmissing = True
        expression = _ensure_string(expression)
        if self._is_string(expression):
            return self._delay(delay, self._string_value_counts(expression, ascending, selection))
        dtype = self._key_dtype(expression)
        task = self.executor.schedule(TaskValueCounts(self, expression, selection=selection))

        @delayed
        def finish(counter):
            keys, counts, null_index = counter.sorted_counts(ascending=ascending, dropnan=dropnan,
                                                             dropmissing=dropmissing)
            if dtype.kind in "mM":
                keys = keys.view(dtype)
            if null_index < 0:
                # no missing entry: the index keeps the key dtype (through keys.tolist(), as the
                # reference builds it, a call took 150 ms at 1e6 keys; the labels are the same)
                return Series(counts, index=keys, dtype=np.int64)
            labels = list(keys) if dtype.kind in "mM" else keys.tolist()
            counts = counts.tolist()
            labels.pop(null_index)  # expression.py:1052-1059: the missing entry goes first
            labels = ["missing"] + labels
            counts = [counts.pop(null_index)] + counts
            return Series(counts, index=labels, dtype=np.int64)

        return self._delay(delay, finish(task))

    def unique(self, expression, return_inverse=False, dropna=False, dropnan=False, dropmissing=False, progress=False,
               selection=None, axis=None, delay=False, array_type="python"):
        """dataframe.py:542-619 over the GPU ordered set: the unique values in first-appearance
        order; the missing entry is masked unless dropped.  return_inverse: also the ordinal of
        every (unfiltered) row in the set, ``null_value`` for masked rows."""
        if dropna:
            dropnan = dropmissing = True
        if axis is not None:
            raise ValueError("only axis=None is supported")
        if array_type not in ("python", "list", "numpy", None):
            raise ValueError(f"unknown array_type {array_type!r}")
        expression = _ensure_string(expression)
        if self._is_string(expression):
            return self._delay(delay, self._string_unique(expression, return_inverse, selection, array_type))
        dtype = self._key_dtype(expression)
        task = self._set(expression, progress=progress, selection=selection, flatten=axis is None, delay=True)

        @delayed
        def finish(ordered_set):
            keys = ordered_set.key_array()
            if dtype.kind in "mM":
                keys = keys.view(dtype)
            deletes = []  # dataframe.py:598-614
            if dropmissing and ordered_set.has_null:
                deletes.append(ordered_set.null_value)
            if dropnan and ordered_set.has_nan:
                deletes.append(ordered_set.nan_value)
            if not dropmissing and ordered_set.has_null:
                # masked before the NaN ordinal is deleted, so the mask stays on the null entry
                mask = np.zeros(len(keys), dtype=bool)
                mask[ordered_set.null_value] = True
                keys = np.ma.array(np.delete(keys, deletes), mask=np.delete(mask, deletes))
            else:
                keys = np.delete(keys, deletes)
            if array_type in ("python", "list"):
                keys = keys.tolist()
            if not return_inverse:
                return keys
            # dataframe.py:563-578: map_ordinal over every row of the frame
            values = self.evaluate(expression, filtered=False)
            if isinstance(values, DeviceMaskedArray):
                inverse = ordered_set.map_ordinal(values.data).to_numpy().astype(np.int64)
                inverse[values.mask.to_numpy().astype(bool)] = ordered_set.null_value
            elif isinstance(values, DeviceArray):
                inverse = ordered_set.map_ordinal(values).to_numpy().astype(np.int64)
            else:
                inverse = ordered_set.map_ordinal(values).astype(np.int64)
                if np.ma.isMaskedArray(values):
                    inverse[np.ma.getmaskarray(values)] = ordered_set.null_value
            return keys, inverse

        return self._delay(delay, finish(task))

    # ---- string keys ---------------------------------------------------------------
    def _encoded(self, names):
        """(frame, {hidden column: dictionary keys}): a copy in which each string key in
        ``names`` (a string column or a string-valued expression) has a hidden int32 column of
        its first-appearance codes beside it (the dictionary encoder, strings.encode), named
        ``_hidden_name(name)``.  An expression is materialised over the frame once, encoded and
        dropped.  Codes are kept per key text while its plan (which spells out the virtual
        columns it goes through) is the same and its source columns are the same live objects."""
        from .expr import evaluate_string, plan_columns
        from .strings import encode
        df = self.copy()
        cache = self.__dict__.setdefault("_string_codes", {})
        keys = {}
        for name in names:
            plan = ("col", name) if name in self.columns else self._string_plan(name)
            sources = [self.columns[n] for n in plan_columns(plan)]
            hit = cache.get(name)
            if hit is None or hit[0] != plan or len(hit[1]) != len(sources) or any(a is not b for a, b in zip(hit[1], sources)):
                codes, sset = encode(evaluate_string(self, plan, 0, self._length))
                hit = cache[name] = (plan, sources, codes, sset.key_array())
            hidden = self._hidden_name(name)
            df.columns[hidden] = hit[2]
            keys[hidden] = hit[3]
        return df, keys

    def _string_value_counts(self, expression, ascending, selection):
        """value_counts of a string column: the column is encoded, the codes are counted by the
        integer counter, and the order is the numeric rule's (keys ascending bytewise, then a
        stable sort by count; descending is the exact reverse)."""
        from pandas import Series
        from .strings import bytewise_order
        df, keys = self._encoded([expression])
        (hidden, keys), = keys.items()
        order = bytewise_order(keys)
        rank = np.empty(len(keys), np.int64)
        rank[order] = np.arange(len(keys))
        counts = df.value_counts(hidden, ascending=ascending, selection=selection)
        codes = counts.index.to_numpy()
        # the counter ordered the codes numerically; the rule orders the strings
        pos = np.argsort(rank[codes], kind="stable")
        c = counts.to_numpy()[pos]
        codes = codes[pos]
        by_count = np.argsort(c, kind="stable")
        if not ascending:
            by_count = by_count[::-1]
        return Series(c[by_count], index=keys[codes[by_count]], dtype=np.int64)

    def _string_unique(self, expression, return_inverse, selection, array_type):
        """unique of a string column: the first-appearance order of the kept rows' codes."""
        df, keys = self._encoded([expression])
        (hidden, keys), = keys.items()
        codes = np.asarray(df.unique(hidden, selection=selection, array_type="numpy"), dtype=np.int64)
        out = keys[codes]
        if array_type in ("python", "list"):
            out = out.tolist()
        if not return_inverse:
            return out
        # every (unfiltered) row's position in `out`; -1 for a row whose string only rows outside
        # the filter / selection hold, as the numeric route's map_ordinal through the kept set
        position = np.full(len(keys), -1, np.int64)
        position[codes] = np.arange(len(codes))
        return out, position[df.columns[hidden].to_numpy()]

    # ---- groupby -----------------------------------------------------------------
    def groupby(self, by=None, agg=None, sort=False, assume_sparse="auto", row_limit=None, copy=True,
                progress=None, delay=False, _speculate=True):
        """dataframe.py:6622-6683."""
        from .groupby import DenseRangeMiss, GroupBy, GroupByDeferred, _dense_range, groupby_multikey, parse_actions
        bys = [_ensure_string(b) for b in (by if isinstance(by, (list, tuple)) else [by])]
        if agg is not None and any(self._is_string(b) for b in bys):
            from .groupby import groupby_string_keys
            return groupby_string_keys(self, bys, isinstance(by, (list, tuple)), agg, sort=sort,
                                       assume_sparse=assume_sparse, row_limit=row_limit)
        if agg is None:  # df.groupby(by).agg(...): the same routes as groupby(by, agg=...)
            return GroupByDeferred(self, by, sort=sort, assume_sparse=assume_sparse, row_limit=row_limit)
        dense_ranges = {}
        multikey = isinstance(by, (list, tuple)) and len(by) > 1
        if multikey:
            # assume_sparse is the reference's combine flag (dataframe.py:6679 ->
            # GroupBy(combine=assume_sparse), groupby.py:313-333): True combines the keys into
            # one grouper, 'auto' when rows / cells < 10, False bins the cartesian grid
            combine = True if assume_sparse is True else (False if assume_sparse is False else "auto")
            res = groupby_multikey(self, by, agg, sort=sort, row_limit=row_limit, combine=combine)
            if res is not None:
                return res
        if agg is not None and assume_sparse != True:  # noqa: E712
            # A single integer key: a dense value range bins like a categorical (min/max
            # pass + BinnerOrdinal grid, GrouperDense); otherwise count/sum/mean run as one
            # hash-partitioned pass (hashagg.py).
            from .hashagg import eligible_key, try_groupby
            # a filtered frame takes the dense route too (its groups: the occupied cells of the
            # filtered counts); the fused hash pass has no filter
            key = eligible_key(self, by, allow_filtered=True)
            if key is not None:
                rng = _dense_range(self, key, speculative=_speculate)
                if rng is not None:
                    dense_ranges[key] = rng
                elif not self.filtered:
                    res = try_groupby(self, by, agg, lambda a, g: parse_actions(self, a, g), sort=sort,
                                      row_limit=row_limit)
                    if res is not None:
                        return res
        if agg is not None and assume_sparse == True and not multikey:  # noqa: E712
            # the ordered_set grouper's result (groups in first-appearance order, or sorted).
            # count / sum / mean of an integer key: one hash-partitioned pass, the groups
            # ordered by the row their key first appears at (hashagg.order_first); other
            # aggregators over a dense key range: the BinnerOrdinal grid (tile path), then the
            # same ordering (vh_dense_first_order)
            from .groupby import first_appearance_order
            from .hashagg import eligible_key, try_groupby
            res = try_groupby(self, by, agg, lambda a, g: parse_actions(self, a, g), sort=sort, row_limit=row_limit,
                              first_order=not sort)
            if res is not None:
                return res
            key = eligible_key(self, by)
            if key is not None and getattr(self.executor, "world", 1) == 1:
                rng = _dense_range(self, key, speculative=_speculate)
                if rng is not None:
                    try:
                        gb = GroupBy(self, by=by, sort=sort, row_limit=row_limit, dense_ranges={key: rng}, first_order=not sort)
                        res = gb.agg(agg)
                    except DenseRangeMiss:
                        return self.groupby(by, agg=agg, sort=sort, assume_sparse=assume_sparse, row_limit=row_limit,
                                            _speculate=False)
                    return res if sort or gb.device_finish else first_appearance_order(self, key, res)
        groupby = GroupBy(self, by=by, sort=sort, row_limit=row_limit,
                          dense=assume_sparse != True or multikey,  # noqa: E712
                          dense_ranges=dense_ranges)
        try:
            return groupby.agg(agg)
        except DenseRangeMiss:
            # the sampled key range missed rows: the exact min / max pass decides the route
            dense_ranges.clear()
            return self.groupby(by, agg=agg, sort=sort, assume_sparse=assume_sparse, row_limit=row_limit,
                                _speculate=False)

    # ---- join ----------------------------------------------------------------------
    def _index(self, expression, prime_growth=False, cardinality=None):
        """dataframe.py:482-539: the GPU ``index_hash`` of an expression over all rows, built in
        executor chunks (key -> first row, plus the other rows of duplicated keys).  A filter
        goes in as the update's ``select``: filtered-out rows never enter, and row numbers stay
        unfiltered row numbers.  ``cardinality`` only sizes the first table."""
        from .join import index
        return index(self, expression, prime_growth=prime_growth, cardinality=cardinality)

    def take(self, indices, filtered=True, dropfilter=True):
        """A new frame of the rows ``indices`` (a host array or a DeviceArray of int32 / int64):
        HBM columns are gathered on the device (``vh_take``), host columns on the host threads;
        virtual columns, variables, categories and selections carry over.  On a filtered frame
        only ``filtered=False, dropfilter=False`` is supported: the indices are unfiltered row
        numbers and the filter stays on the result (the other forms raise NotImplementedError);
        ``df.extract().take(indices)`` takes from the kept rows."""
        from .join import take
        return take(self, indices, filtered=filtered, dropfilter=dropfilter)

    def extract(self):
        """dataframe.py:4216-4233: a frame of the rows the filter keeps, with the filter dropped
        (a copy for an unfiltered frame).  HBM columns are compacted in HBM (``mask_rows`` of the
        filter's device mask, then ``vh_take``); a host frame uses boolean indexing."""
        from .sort import extract
        return extract(self)

    def sort(self, by, ascending=True, kind="quicksort"):
        """dataframe.py:4420-4461: the rows in the order of ``by``, an expression or a list /
        tuple of expressions (the first the most significant).  The order is
        ``np.argsort(kind="stable")`` / ``np.lexsort``: stable (``kind`` is accepted, and stable
        is a valid answer for every NumPy kind), NaN last, ``-0.0 == 0.0``; ``ascending=False``
        is the exact reverse.  datetime keys sort as int64.  The result goes through ``take``:
        virtual columns, variables, categories and selections carry over, and on a filtered
        frame it holds only the kept rows, with the filter dropped.  On a frame with HBM columns
        the keys are argsorted on the device (``vh_argsort`` over the kept rows) and HBM columns
        are gathered in HBM; a frame with no HBM column is ordered by NumPy."""
        from .sort import sort
        return sort(self, by, ascending=ascending, kind=kind)

    def join(self, other, on=None, left_on=None, right_on=None, lprefix="", rprefix="", lsuffix="", rsuffix="",
             how="left", allow_duplication=False, prime_growth=False, cardinality_other=None, inplace=False):
        """DataFrame.join (join.py:124-292): attach the columns of ``other`` to the rows of this
        frame whose ``left_on`` key equals ``other``'s ``right_on`` key (``on``: the same name
        in both; no key at all: a row-wise merge of frames of equal length).

        ``how`` is 'left', 'right' (the sides and their prefixes swap) or 'inner'.  Columns
        present in both frames are renamed with the prefixes / suffixes (the join column is not
        added twice); a collision without a proper prefix / suffix raises ValueError.  The key
        dtypes must be equal (datetimes join as int64), else TypeError.  ``other`` is indexed on
        the GPU (``_index``; its filter removes rows from the index), every unfiltered row of
        this frame is mapped to its first matching row, and this frame's filter stays on the
        result.  Duplicated keys in ``other`` raise ValueError unless ``allow_duplication``: then
        the extra matches are appended after all original rows, in left-row order.
        ``cardinality_other`` only sizes the index's first table.

        Every column of ``other`` is gathered where it lives: HBM columns on the device (eight per
        pass, int32 lookups while ``other`` has fewer than 2^31 rows), host columns on the host.
        Keys compare by bit pattern with one NaN (``-0.0`` and ``0.0`` differ).

        Limit: HBM frames carry no masks.  When a row of a 'left' / 'right' join finds no match,
        the joined columns come back masked: host columns as ``np.ma`` arrays, and HBM columns
        READ BACK to the host as ``np.ma`` arrays (with the mask the gather kernel built), so the
        result is then a mixed host / HBM frame.  When every row matches, and always for
        'inner', HBM columns stay in HBM.  A rename of a column that a virtual column, filter or
        selection uses raises NotImplementedError (expressions are not rewritten)."""
        from .join import join
        return join(self, other, on=on, left_on=left_on, right_on=right_on, lprefix=lprefix, rprefix=rprefix,
                    lsuffix=lsuffix, rsuffix=rsuffix, how=how, allow_duplication=allow_duplication,
                    prime_growth=prime_growth, cardinality_other=cardinality_other, inplace=inplace)

    def export_hdf5(self, path, **kwargs):
        """dataframe.py export_hdf5: numeric columns (host or HBM) as vaex's HDF5 layout
        version 2, contiguous and 4 KiB aligned so the file maps back without copies."""
        from .hdf5 import export_hdf5
        self._refuse_export()
        export_hdf5(self, path)

    def export_arrow(self, path, **kwargs):
        import pyarrow as pa
        self._refuse_export()
        cols = {}
        for name in self.get_column_names():
            v = self.columns.get(name)
            v = v.to_numpy() if isinstance(v, DeviceArray) else np.asarray(self.evaluate(name) if v is None else v)
            cols[name] = pa.array(v)
        with pa.OSFile(str(path), "wb") as sink:
            table = pa.table(cols)
            with pa.ipc.new_file(sink, table.schema) as w:
                w.write_table(table)

    def _refuse_export(self):
        if self._has_masked():
            raise NotImplementedError(f"export of the masked HBM column {self._masked_names()[0]!r} is not supported")

    def binby(self, by=None, agg=None, sort=False, copy=True, delay=False, progress=None):
        from .groupby import BinBy
        binby = BinBy(self, by=by, sort=sort)
        if agg is None:
            return binby
        return binby.agg(agg)

    # ---- small conveniences used by tests ----------------------------------------
    def to_dict(self):
        out = {}
        for k, v in self.columns.items():
            out[k] = v.to_numpy() if isinstance(v, (DeviceArray, DeviceMaskedArray)) else np.asarray(v)
        return out

    def __repr__(self):
        return f"DataFrame({self._length} rows, columns={self.get_column_names()})"


def from_arrays(**arrays):
    """vaex.from_arrays: numpy arrays (host) or DeviceArray (HBM-resident) columns."""
    cols = {}
    for k, v in arrays.items():
        if isinstance(v, (DeviceArray, DeviceMaskedArray, DeviceStringArray)) or np.ma.isMaskedArray(v):
            cols[k] = v
        else:
            cols[k] = np.asarray(v)
    return DataFrame(cols)


def from_dict(d):
    return from_arrays(**d)
