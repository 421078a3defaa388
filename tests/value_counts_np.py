"""NumPy restatement of the reference's counter / value_counts / unique, the yardstick of
the GPU hash counter tests (the repository has no CPU counter).

* ``counter_np``: ``counter_<dtype>`` (packages/vaex-core/src/hash_primitives.hpp:328-415)
  read as ``key_array()`` / ``counts()``: NaN at index 0 when present, the null entry at the
  next index (``key_offset``, hash_primitives.hpp:338-348), then the regular keys.  The
  reference lists the regular keys in its hash maps' iteration order, which value_counts
  never exposes (it sorts by count); here they are in ascending key order, floats ordered
  and told apart by their bit pattern, so -0.0 comes just before 0.0 and is its own key
  (``np.unique`` on the floats would merge them).
* ``value_counts_np``: ``Expression.value_counts`` (packages/vaex-core/vaex/expression.py:946-1061),
  with ``np.argsort(kind="stable")`` where the reference's argsort leaves ties open.
* ``unique_np``: ``DataFrame.unique`` (packages/vaex-core/vaex/dataframe.py:542-619) over an
  ordered set filled by ONE update call: regular keys in first-appearance order, then NaN,
  then null (hash_primitives.hpp:248-274 flushes NaN / null after the call's regular keys).
"""
import numpy as np
import pandas as pd


def ordered_bits(values):
    """uint64 whose unsigned order is the keys' numeric order; floats by bit pattern."""
    values = np.asarray(values)
    dt = values.dtype
    if dt.kind == "f":
        nbits = dt.itemsize * 8
        u = values.view(f"u{dt.itemsize}").astype(np.uint64)
        top = np.uint64(1 << (nbits - 1))
        full = np.uint64((1 << nbits) - 1)
        return np.where((u & top) != 0, (~u) & full, u | top)
    if dt.kind == "i":
        return values.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    return values.astype(np.uint64)


def _split(values, mask, select):
    if np.ma.isMaskedArray(values):
        m = np.ma.getmaskarray(values)
        mask = m if mask is None else (np.asarray(mask, bool) | m)
        values = values.data
    values = np.asarray(values)
    if values.dtype.kind in "mM":
        values = values.view(np.int64)
    keep = np.ones(len(values), bool) if select is None else np.asarray(select).astype(bool)
    null = keep & (np.zeros(len(values), bool) if mask is None else np.asarray(mask).astype(bool))
    nan = keep & ~null & (values != values) if values.dtype.kind == "f" else np.zeros(len(values), bool)
    regular = keep & ~null & ~nan
    return values, regular, int(nan.sum()), int(null.sum())


def counter_np(values, mask=None, select=None):
    """(keys, counts, null_index) in key order; null_index is -1 without a null entry."""
    values, regular, nan_count, null_count = _split(values, mask, select)
    reg = values[regular]
    _, first, cnt = np.unique(ordered_bits(reg), return_index=True, return_counts=True)
    keys = [reg[first]]
    counts = [cnt.astype(np.int64)]
    null_index = -1
    if null_count:  # hash_primitives.hpp:341-343: behind NaN, before the regular keys
        keys.insert(0, np.zeros(1, values.dtype))
        counts.insert(0, np.array([null_count], np.int64))
        null_index = 1 if nan_count else 0
    if nan_count:
        keys.insert(0, np.full(1, np.nan, values.dtype))
        counts.insert(0, np.array([nan_count], np.int64))
    return np.concatenate(keys).astype(values.dtype), np.concatenate(counts), null_index


def sorted_counts_np(values, mask=None, select=None, ascending=False, dropnan=False, dropmissing=False):
    """(keys, counts, null_index) after the drops and the sort by count (expression.py:1026-1050)."""
    keys, counts, null_index = counter_np(values, mask, select)
    has_nan = keys.dtype.kind == "f" and len(keys) > 0 and bool(np.isnan(keys[0]))
    deletes = []
    if dropmissing and null_index >= 0:
        deletes.append(null_index)
        null_index = -1
    if dropnan and has_nan:
        deletes.append(0)
        if null_index >= 0:
            null_index -= 1
    keys, counts = np.delete(keys, deletes), np.delete(counts, deletes)
    order = np.argsort(counts, kind="stable")
    if not ascending:
        order = order[::-1]
    if null_index >= 0:
        null_index = int(np.nonzero(order == null_index)[0][0])
    return keys[order], counts[order], null_index


def value_counts_np(values, mask=None, select=None, dropna=False, dropnan=False, dropmissing=False, ascending=False):
    """The pandas Series of Expression.value_counts; "missing" first (expression.py:1052-1059)."""
    if dropna:
        dropnan = dropmissing = True
    dtype = (values.data if np.ma.isMaskedArray(values) else np.asarray(values)).dtype
    keys, counts, null_index = sorted_counts_np(values, mask, select, ascending, dropnan, dropmissing)
    labels = list(keys.view(dtype)) if dtype.kind in "mM" else keys.tolist()
    counts = counts.tolist()
    if null_index >= 0:
        labels.pop(null_index)
        labels = ["missing"] + labels
        counts = [counts.pop(null_index)] + counts
    return pd.Series(counts, index=labels, dtype=np.int64)


def unique_np(values, mask=None, select=None, dropna=False, dropnan=False, dropmissing=False):
    """A list: regular keys in first-appearance order, NaN, then None for the missing entry."""
    if dropna:
        dropnan = dropmissing = True
    values, regular, nan_count, null_count = _split(values, mask, select)
    reg = values[regular]
    _, first = np.unique(ordered_bits(reg), return_index=True)
    out = reg[np.sort(first)].tolist()
    if nan_count and not dropnan:
        out.append(float("nan"))
    if null_count and not dropmissing:
        out.append(None)
    return out


def _same_label(a, b):
    if isinstance(a, str) or isinstance(b, str) or a is None or b is None:
        return type(a) is type(b) and a == b
    fa, fb = isinstance(a, (float, np.floating)), isinstance(b, (float, np.floating))
    if fa != fb:
        return False
    if fa:
        if np.isnan(a) or np.isnan(b):
            return bool(np.isnan(a) and np.isnan(b))
        return a == b and np.signbit(a) == np.signbit(b)
    return a == b


def same_labels(a, b):
    """Exact equality of two label lists: NaN equals NaN, -0.0 differs from 0.0."""
    a, b = list(a), list(b)
    return len(a) == len(b) and all(_same_label(x, y) for x, y in zip(a, b))


def assert_series_same(got, expected):
    assert same_labels(got.index.tolist(), expected.index.tolist()), (got.index.tolist()[:20], expected.index.tolist()[:20])
    assert got.dtype == expected.dtype == np.int64
    assert got.tolist() == expected.tolist()
