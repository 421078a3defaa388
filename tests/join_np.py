"""NumPy restatement of the reference's index_hash and DataFrame.join, the yardstick of the GPU
index and join tests (the repository has no CPU index).

The contract is the single-threaded, one-map, rows-in-order reference (``nmaps = 1``, one
thread walking the rows of each ``update`` call in order):

* ``IndexNp`` / ``index_np``: ``index_hash_<dtype>`` (packages/vaex-core/src/hash_primitives.hpp:623-900).
  A key maps to the first row it was seen at (``add_new``, :662-666), its later rows go to the
  key's overflow list in the order seen (``add_existing``, :668-674), ``nan_value`` /
  ``null_value`` are the LAST NaN / null row (``add_nan`` / ``add_null`` overwrite, :652-660),
  ``length`` counts every regular row plus one for NaN and one for null (:636-645,
  hash.hpp:208-249).  Keys are told apart by bit pattern with one NaN entry (the GPU engines'
  rule: -0.0 and 0.0 are two keys; the reference compares with ``==``), and a NaN / null
  lookup in an index without one gives -1 (the reference leaves it uninitialised).
* ``map_index_np``: ``map_index`` / ``map_index_with_mask`` (:679-754).
* ``map_index_duplicates_np``: ``map_index_duplicates[_with_mask]`` (:756-848).
* ``join_np``: ``DataFrame.join`` (packages/vaex-core/vaex/join.py:124-292) over dicts of
  columns, in the reference's column order.
"""
import numpy as np


def _bits(values):
    values = np.ascontiguousarray(values)
    if values.dtype.kind in "mM":
        values = values.view(np.int64)
    return values.view(f"u{values.dtype.itemsize}")


def _isnan(values):
    values = np.asarray(values)
    return np.isnan(values) if values.dtype.kind == "f" else np.zeros(len(values), bool)


def _split(values, mask):
    if np.ma.isMaskedArray(values):
        m = np.ma.getmaskarray(values)
        mask = m if mask is None else (np.asarray(mask, bool) | m)
        values = values.data
    return np.asarray(values), (None if mask is None else np.asarray(mask, bool))


class IndexNp:
    def __init__(self):
        self.first = {}    # key bits -> first row
        self.extras = {}   # key bits -> later rows, in the order seen
        self.nan_value = -1
        self.null_value = -1
        self.nan_count = 0
        self.null_count = 0

    def update(self, values, mask=None, select=None, start_index=0):
        values, mask = _split(values, mask)
        bits, nan = _bits(values).tolist(), _isnan(values)
        for i in range(len(values)):
            if select is not None and not select[i]:
                continue  # a filtered-out row is not seen at all
            row = start_index + i
            if mask is not None and mask[i]:
                self.null_value = row  # :657-660
                self.null_count += 1
            elif nan[i]:
                self.nan_value = row  # :652-655
                self.nan_count += 1
            elif bits[i] not in self.first:
                self.first[bits[i]] = row  # :662-666
            else:
                self.extras.setdefault(bits[i], []).append(row)  # :668-674
        return self

    @property
    def has_duplicates(self):
        return bool(self.extras)

    @property
    def length(self):
        return (len(self.first) + sum(len(v) for v in self.extras.values())
                + (self.nan_count > 0) + (self.null_count > 0))

    def __len__(self):
        return self.length


def index_np(values, mask=None, select=None, start_index=0):
    """One ``update`` call: an IndexNp with ``first``, ``extras``, ``nan_value``,
    ``null_value``, ``has_duplicates`` and ``length``."""
    return IndexNp().update(values, mask, select, start_index)


def map_index_np(index, values, mask=None):
    """(lookup int64, found_unknown) (:679-754: NaN is tested before the mask)."""
    values, mask = _split(values, mask)
    bits, nan = _bits(values).tolist(), _isnan(values)
    out = np.empty(len(values), np.int64)
    for i in range(len(values)):
        if nan[i]:
            out[i] = index.nan_value
        elif mask is not None and mask[i]:
            out[i] = index.null_value
        else:
            out[i] = index.first.get(bits[i], -1)
    return out, bool((out == -1).any())


def map_index_duplicates_np(index, values, mask=None, start_index=0):
    """(left_indices, right_indices), int64 (:756-848): NaN and masked keys are skipped."""
    values, mask = _split(values, mask)
    bits, nan = _bits(values).tolist(), _isnan(values)
    left, right = [], []
    for i in range(len(values)):
        if nan[i] or (mask is not None and mask[i]):
            continue
        for r in index.extras.get(bits[i], ()):
            left.append(start_index + i)
            right.append(r)
    return np.array(left, np.int64), np.array(right, np.int64)


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


def take_np(column, lookup, masked):
    """dataset.take(lookup, masked=...): -1 entries become masked."""
    column, cmask = _split(column, None)
    lookup = np.asarray(lookup, np.int64)
    out = column[np.where(lookup < 0, 0, lookup)] if len(column) else np.zeros(len(lookup), column.dtype)
    m = lookup < 0
    if cmask is not None:
        m = m | cmask[np.where(lookup < 0, 0, lookup)]
        masked = True
    if not masked:
        return out
    out = out.copy()
    out[lookup < 0] = 0
    return np.ma.array(out, mask=m)


def join_np(left_cols, right_cols, on=None, left_on=None, right_on=None, lprefix="", rprefix="", lsuffix="", rsuffix="",
            how="left", allow_duplication=False, left_filter=None, right_filter=None):
    """DataFrame.join over dicts ``name -> array`` (join.py:124-292).  Returns
    ``(columns, filter)``: the joined columns over ALL rows of the result (possibly masked
    arrays, in the reference's column order) and the left frame's filter carried onto those
    rows (None without one); a right filter removes rows from the index (``right.extract()``,
    join.py:159, without renumbering -- the same result)."""
    left, right = dict(left_cols), dict(right_cols)
    if how == "right":  # join.py:136-140
        left, right = right, left
        lprefix, rprefix = rprefix, lprefix
        lsuffix, rsuffix = rsuffix, lsuffix
        left_on, right_on = right_on, left_on
        left_filter, right_filter = right_filter, left_filter
    elif how not in ("left", "inner"):
        raise ValueError("join type not supported: {}, only left and right".format(how))
    left_on = left_on or on
    right_on = right_on or on
    for name in right:  # join.py:152-157
        if left_on and (rprefix + name + rsuffix == lprefix + left_on + lsuffix):
            continue
        if name in left and rprefix + name + rsuffix == lprefix + name + lsuffix:
            raise ValueError("column name collision: {} exists in both column, and no proper suffix given".format(name))
    n_left = len(next(iter(left.values())))
    keep = None if left_filter is None else np.asarray(left_filter, bool)
    lookup, masked = None, False
    if left_on is not None or right_on is not None:
        lk, rk = left[left_on], right[right_on]
        if np.asarray(lk).dtype != np.asarray(rk).dtype:
            raise TypeError("join key dtypes differ")
        index = index_np(rk, select=right_filter)
        if index.has_duplicates and not allow_duplication:
            raise ValueError("This join will lead to duplication of rows which is disabled, pass allow_duplication=True")
        lookup, masked = map_index_np(index, lk)  # every unfiltered left row (ignore_filter=True, join.py:207)
        if index.has_duplicates:  # join.py:208-213
            ll, lr = map_index_duplicates_np(index, lk, None, 0)
            left = {k: (np.ma.concatenate if np.ma.isMaskedArray(v) else np.concatenate)([v, v[ll]]) for k, v in left.items()}
            lookup = np.concatenate([lookup, lr])
            if keep is not None:
                keep = np.concatenate([keep, keep[ll]])
        if how == "inner":  # join.py:215-220
            matched = lookup != -1
            lookup = lookup[matched]
            left = {k: v[matched] for k, v in left.items()}
            if keep is not None:
                keep = keep[matched]
            masked = False
    elif n_left != len(next(iter(right.values()))):
        raise ValueError("row-wise join of frames of different lengths")
    # renaming (join.py:229-253)
    right_names, left_names = list(right), list(left)
    for name in list(right_names):
        if name in left_names:
            all_names = list(set(right_names + left_names))
            all_names.append(_mangle(lprefix, name, lsuffix))
            all_names.remove(name)
            new_name = _mangle(rprefix, name, rsuffix)
            if new_name != left_on:
                if new_name in all_names:
                    new_name = _valid_name(new_name, all_names)
                right_names[right_names.index(name)] = new_name
            all_names = list(set(right_names + left_names))
            all_names.remove(name)
            new_name = _mangle(lprefix, name, lsuffix)
            if new_name in all_names:
                new_name = _valid_name(new_name, all_names)
            left_names[left_names.index(name)] = new_name
    out = {new: left[old] for new, old in zip(left_names, left)}
    for new, old in zip(right_names, right):  # join.py:255-276
        if new == left_on and new in left_names:
            continue
        assert new not in out
        col = right[old]
        out[new] = col if lookup is None else take_np(col, lookup, masked)
    return out, keep
