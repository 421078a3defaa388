"""``DataFrame._index`` / ``take`` / ``join`` over the GPU index (``superutils.index_hash_<dtype>``)
and the device gather -- the reference's join (``packages/vaex-core/vaex/join.py:124-292``,
``dataframe.py:482-539``): index the right side's key, map every left row to a right row, gather
the right columns through that lookup.  Columns are gathered where they live: HBM columns by
``vh_take`` (eight per pass over the lookup), host columns by ``hostops.take_columns``."""
import re

import numpy as np

from . import _lib, hostops
from .device import DeviceArray, DeviceMaskedArray
from .superutils import index_matched, index_type_from_dtype, mask_combine, take_device


def _ensure_string(e):
    return None if e is None else str(e)


def _next_pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def _chunks(df):
    n = df.length_unfiltered()
    if tuple(df.executor.row_range(df)) != (0, n):
        # a distributed executor owns a shard of the rows: a join over one shard would be wrong
        raise NotImplementedError("join / _index with a multi-rank executor is not supported")
    cs = max(1, df.executor.chunk_size_for(df))
    return [(i1, min(n, i1 + cs)) for i1 in range(0, n, cs)]


def _key_dtype(dt):
    dt = np.dtype(dt)
    return np.dtype(np.int64) if dt.kind in "mM" else dt.newbyteorder("=")


# ---- _index -----------------------------------------------------------------------------------
def index(df, expression, prime_growth=False, cardinality=None):
    """dataframe.py:482-539: one index_hash over every row of ``expression``, in executor chunks.
    A filter goes in as the update's ``select``: filtered-out rows never enter and row numbers
    stay unfiltered row numbers (the reference's ``right.extract()`` without the compaction)."""
    expression = _ensure_string(expression)
    cls = index_type_from_dtype(_key_dtype(df.data_type(expression)), prime_growth=prime_growth)
    cap = 0 if cardinality is None else max(16, _next_pow2(2 * int(cardinality)))
    ix = cls(initial_capacity=cap)
    for i1, i2 in _chunks(df):
        ar = df._eval_host(expression, i1, i2)
        if isinstance(ar, DeviceMaskedArray):
            raise NotImplementedError(f"an index over the masked HBM expression {expression!r} is not supported")
        select = None
        if df.filtered:
            select = df.device_keep_mask(i1, i2) if df.is_device_resident() else df.evaluate_filter_mask(i1, i2)
            if isinstance(select, DeviceArray) and select.dtype.itemsize != 1:
                raise TypeError("filter mask is not a byte mask")
        ix.update(ar, start_index=i1, select=select)
    return ix


# ---- take ---------------------------------------------------------------------------------------
def _host_indices(indices):
    return indices.to_numpy() if isinstance(indices, DeviceArray) else np.asarray(indices)


def _device_indices(indices, length):
    if isinstance(indices, DeviceArray):
        return indices
    indices = np.ascontiguousarray(indices)
    if indices.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        indices = indices.astype(np.int64)
    if len(indices) and (indices.min() < -1 or indices.max() >= length):
        raise IndexError("take: index out of range")
    return DeviceArray.from_numpy(indices)


def gather(columns, lookup, length, masked=False):
    """{name: column[lookup]} for host and HBM columns of ``length`` rows; ``lookup`` (host or
    DeviceArray, int32 / int64) may hold -1 only with masked=True, and every column then comes
    back as a host ``np.ma`` array with those rows masked (an HBM column is read back together
    with the mask the gather kernel wrote).  A masked HBM column (DeviceMaskedArray) is gathered as
    data plus mask, the mask one more uint8 column of ``vh_take``, and stays in HBM; a row whose
    lookup is -1 is missing in it.  masked=True (the join's unmatched rows) does not take one."""
    out = {}
    from .strings import DeviceStringArray
    dev_names = [k for k, c in columns.items() if isinstance(c, DeviceArray)]
    str_names = [k for k, c in columns.items() if isinstance(c, DeviceStringArray)]
    mdev_names = [k for k, c in columns.items() if isinstance(c, DeviceMaskedArray)]
    host_names = [k for k in columns if k not in dev_names and k not in str_names and k not in mdev_names]
    if mdev_names:
        if masked:
            raise NotImplementedError(f"masked HBM column {mdev_names[0]!r}: a gather that leaves rows unmatched (join) "
                                      "is not supported")
        dl = _device_indices(lookup, length)
        cols = [columns[k].data for k in mdev_names] + [columns[k].mask for k in mdev_names]
        res, miss = take_device(cols, dl, with_mask=True)
        for j, k in enumerate(mdev_names):
            out[k] = DeviceMaskedArray(res[j], mask_combine(res[len(mdev_names) + j], miss, "or"))
    if str_names:  # string columns: the byte-exact device gather (vh_str_take)
        if masked:
            raise NotImplementedError("string columns carry no nulls: a gather that leaves rows unmatched")
        dl = _device_indices(lookup, length)
        for k in str_names:
            out[k] = columns[k].take(dl)
    if dev_names:
        dl = _device_indices(lookup, length)
        cols = [columns[k] for k in dev_names]  # vh_take launches once per eight columns
        if masked:
            res, mask = take_device(cols, dl, with_mask=True)
        else:
            res = take_device(cols, dl)
        out.update(zip(dev_names, res))
        if masked:
            m = mask.to_numpy().astype(bool)
            for k in dev_names:
                out[k] = np.ma.array(out[k].to_numpy(), mask=m)
    if host_names:
        hl = _host_indices(lookup).astype(np.int64, copy=False)
        if len(hl) and (hl.min() < -1 or hl.max() >= length):
            raise IndexError("take: index out of range")
        miss = hl < 0
        safe = np.where(miss, 0, hl) if masked else hl
        datas = [np.ma.getdata(columns[k]) for k in host_names]
        taken = hostops.take_columns(datas, safe) if length else [np.zeros(len(hl), d.dtype) for d in datas]
        for k, t in zip(host_names, taken):
            c = columns[k]
            if np.ma.isMaskedArray(c):
                cm = np.ma.getmaskarray(c)[safe] if length else np.zeros(len(hl), bool)
                t = np.ma.array(t, mask=(cm | miss) if masked else cm)
            elif masked:
                t = np.array(t)
                t[miss] = 0
                t = np.ma.array(t, mask=miss)
            out[k] = t
    return {k: out[k] for k in columns}


def _like(df, columns):
    """A frame of new columns with the virtual columns, variables, categories, selections and
    the filter of ``df``."""
    from .dataframe import DataFrame
    new = DataFrame(columns, executor=df.executor)
    new.variables = dict(df.variables)
    new.virtual_columns = dict(df.virtual_columns)
    new._categories = dict(df._categories)
    new._copy_selections(df)
    new._filter = df._filter
    if not columns:
        new._length = 0
    return new


def take_rows(df, indices, dropfilter=False):
    """A new frame of the unfiltered rows ``indices`` (host array or DeviceArray of int32 /
    int64) with the virtual columns, variables, categories and selections of ``df``; its filter
    stays on the result unless ``dropfilter`` (``sort`` / ``extract`` drop it: sort.py)."""
    cols = gather(df.columns, indices, df.length_unfiltered())
    new = _like(df, cols)
    new._length = len(indices)
    if dropfilter:
        new._filter = None
    return new


def take(df, indices, filtered=True, dropfilter=True):
    """dataframe.py take: a new frame of the rows ``indices`` (host array or DeviceArray of
    int32 / int64; unfiltered row numbers).  On a filtered frame only ``filtered=False,
    dropfilter=False`` is supported (what the join needs): the indices address unfiltered rows
    and the filter stays on the result.  ``df.extract().take(indices)`` takes from the kept rows."""
    if df.filtered and (filtered or dropfilter):
        raise NotImplementedError("take on a filtered frame: only filtered=False, dropfilter=False")
    return take_rows(df, indices)


def _concat(a, b):
    if isinstance(a, DeviceArray):
        out = DeviceArray(len(a) + len(b), a.dtype)
        if a.nbytes:
            _lib.call("vh_memcpy_dtod", out.ptr, a.ptr, a.nbytes)
        if b.nbytes:
            _lib.call("vh_memcpy_dtod", out.ptr + a.nbytes, b.ptr, b.nbytes)
        return out
    if np.ma.isMaskedArray(a) or np.ma.isMaskedArray(b):
        return np.ma.concatenate([a, b])
    return np.concatenate([a, b])


# ---- join ---------------------------------------------------------------------------------------
def _mangle(prefix, name, suffix):  # join.py:223-227
    if name.startswith("__"):
        return "__" + prefix + name[2:] + suffix
    return prefix + name + suffix


def _valid_name(name, used):  # utils.py:560-570
    if name in used:
        nr = 1
        while name + ("_%d" % nr) in used:
            nr += 1
        name = name + ("_%d" % nr)
    return name


def _uses(expression, name):
    return re.search(r"(?<![\w.])%s(?!\w)" % re.escape(name), str(expression)) is not None


def _rename(df, old, new):
    """Rename a column in place, keeping its position.  Expressions are not rewritten: a
    virtual column, filter or selection that uses the old name raises."""
    if old == new:
        return
    # _selection_dependencies: also the x / y expressions of a lasso, which has no folded string
    users = [e for e in list(df.virtual_columns.values()) + list(df.selection_expressions.values())
             + df._selection_dependencies() + [df._filter] if e is not None and _uses(e, old)]
    if users:
        raise NotImplementedError(
            f"join renames column {old!r} to {new!r}, but the expression {users[0]!r} uses it: expression rewriting "
            "is not supported, rename the column or pass other prefixes / suffixes")
    for attr in ("columns", "virtual_columns"):
        d = getattr(df, attr)
        if old in d:
            setattr(df, attr, {(new if k == old else k): v for k, v in d.items()})
    if old in df._categories:
        df._categories[new] = df._categories.pop(old)


def _names(df):
    return list(df.columns) + list(df.virtual_columns)


def join(df, other, on=None, left_on=None, right_on=None, lprefix="", rprefix="", lsuffix="", rsuffix="", how="left",
         allow_duplication=False, prime_growth=False, cardinality_other=None, inplace=False):
    left, right = df, other
    inner = False
    for frame in (df, other):  # masked HBM columns do not join yet, as a key or as a payload
        if frame._has_masked():
            raise NotImplementedError(f"join of a frame with the masked HBM column {frame._masked_names()[0]!r} is "
                                      "not supported")
    if how == "right":  # join.py:136-140
        left, right = right, left
        lprefix, rprefix = rprefix, lprefix
        lsuffix, rsuffix = rsuffix, lsuffix
        left_on, right_on = right_on, left_on
    elif how == "inner":
        inner = True
    elif how != "left":
        raise ValueError("join type not supported: {}, only left and right".format(how))
    target = left if inplace else None
    left = left.copy()
    right = right.copy()  # renames below must not reach `other`
    on, left_on, right_on = _ensure_string(on), _ensure_string(left_on), _ensure_string(right_on)
    left_on = left_on or on
    right_on = right_on or on
    for name in _names(right):  # join.py:152-157
        if left_on and (rprefix + name + rsuffix == lprefix + left_on + lsuffix):
            continue  # it's ok when we join on the same column name
        if name in _names(left) and rprefix + name + rsuffix == lprefix + name + lsuffix:
            raise ValueError("column name collision: {} exists in both column, and no proper suffix given".format(name))

    n_right = right.length_unfiltered()
    lookup, masked = None, False
    if left_on is None and right_on is None:
        # a row-wise join: the frames are merged
        if right.filtered:
            raise NotImplementedError("row-wise join with a filtered right frame")
        if left.length_unfiltered() != n_right:
            raise ValueError("row-wise join: the frames differ in length ({} and {})".format(left.length_unfiltered(), n_right))
    else:
        if left_on is None or right_on is None:
            raise ValueError("join needs both left_on and right_on (or on)")
        ldt, rdt = left.data_type(left_on), right.data_type(right_on)
        if _key_dtype(ldt) != _key_dtype(rdt) or (ldt.kind in "mM") != (rdt.kind in "mM"):
            raise TypeError(f"join key dtypes differ: {left_on} is {ldt}, {right_on} is {rdt}")
        ix = index(right, right_on, prime_growth=prime_growth, cardinality=cardinality_other)
        duplicates_right = ix.has_duplicates
        if duplicates_right and not allow_duplication:
            raise ValueError("This join will lead to duplication of rows which is disabled, pass allow_duplication=True")
        lookup_dtype = np.int32 if n_right < 2 ** 31 else np.int64
        n_left = left.length_unfiltered()
        # the lookup covers every unfiltered left row (ignore_filter=True, join.py:207) and lives
        # where the left key column does
        probe = left._eval_host(left_on, 0, min(n_left, 1))
        on_device = isinstance(probe, DeviceArray)
        if on_device and duplicates_right:
            lookup_dtype = np.int64  # the duplicate pairs are int64 and are appended in HBM as they are
        lookup = DeviceArray(n_left, lookup_dtype) if on_device else np.empty(n_left, lookup_dtype)
        extra = []
        for i1, i2 in _chunks(left):
            ar = left._eval_host(left_on, i1, i2)
            if np.ma.isMaskedArray(ar):
                mask = np.ma.getmaskarray(ar)
                masked |= ix.map_index_masked(ar.data, mask, lookup[i1:i2])
                if duplicates_right:
                    extra.append(ix.map_index_duplicates(ar.data, mask, i1))
            else:
                masked |= ix.map_index(ar, lookup[i1:i2])
                if duplicates_right:  # HBM keys: the pairs stay in HBM
                    extra.append(ix.map_index_duplicates(ar, i1, on_device=on_device))
        # join.py:208-213: the extra rows come after all original rows
        for lookup_left, lookup_right in extra:
            if not len(lookup_left):
                continue
            n_now = left.length_unfiltered()
            more = take_rows(left, lookup_left)
            left = _like(left, {k: _concat(c, more.columns[k]) for k, c in left.columns.items()})
            left._length = n_now + len(lookup_left)
            lookup = _concat(lookup, lookup_right if on_device else lookup_right.astype(lookup_dtype))
        if inner:  # join.py:215-220
            if on_device:
                rows, lookup = index_matched(lookup)
            else:
                matched = lookup != -1
                rows, lookup = np.where(matched)[0], lookup[matched]
            # the indices can still refer to filtered rows, so the filter is not dropped
            left = take_rows(left, rows)
            masked = False

    # renaming, so that all column names are unique (join.py:229-253)
    right_names, left_names = _names(right), _names(left)
    for name in list(right_names):
        if name in left_names:
            all_names = list(set(right_names + left_names))
            all_names.append(_mangle(lprefix, name, lsuffix))  # we do not want to steal the left's name
            all_names.remove(name)
            new_name = _mangle(rprefix, name, rsuffix)
            if new_name != left_on:  # the join column is not added twice
                if new_name in all_names:
                    new_name = _valid_name(new_name, all_names)
                _rename(right, name, new_name)
                right_names[right_names.index(name)] = new_name
            all_names = list(set(right_names + left_names))
            all_names.remove(name)
            new_name = _mangle(lprefix, name, lsuffix)
            if new_name in all_names:
                new_name = _valid_name(new_name, all_names)
            _rename(left, name, new_name)
            left_names[left_names.index(name)] = new_name

    # the right's columns are added to the left (join.py:255-276)
    take_cols = {}
    for name in _names(right):
        if name == left_on and name in left_names:
            continue  # skip when it's the join column
        assert name not in left_names
        if name in right.virtual_columns:
            left.virtual_columns[name] = right.virtual_columns[name]
        else:
            take_cols[name] = right.columns[name]
    for name, value in right.variables.items():
        left.variables.setdefault(name, value)
    for name, cat in right._categories.items():
        if name in take_cols or name in right.virtual_columns:
            left._categories.setdefault(name, cat)
    if lookup is not None:
        take_cols = gather(take_cols, lookup, n_right, masked=masked)
    for name, col in take_cols.items():
        left.columns[name] = col
    if not left._length and left.columns:
        left._length = len(next(iter(left.columns.values())))
    if target is not None:
        target.__dict__.update(left.__dict__)
        return target
    return left
