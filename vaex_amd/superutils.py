"""``vaex.superutils.ordered_set_<dtype>`` over the GPU hash set of libvaexhip.

Mirrors ``ordered_set`` (``packages/vaex-core/src/hash_primitives.hpp:417-621``;
bindings ``hash_primitives.cpp:26-73``): ``update``, ``key_array``, ``map_ordinal``,
``isin``, ``merge``, ``seal``, ``nan_count``/``null_count``/``has_nan``/``has_null``,
``nan_value``/``null_value``, ``fingerprint``, ``len()``, the ``create`` constructor
``ordered_set_<t>(keys, null_value, nan_count, null_count, fingerprint)`` and
``flatten_values``.  ``counter_<dtype>`` (``hash_primitives.hpp:328-415``), the key -> count map
of ``value_counts``, sits beside it over the library's hash counter, and ``index_hash_<dtype>``
(``hash_primitives.hpp:623-900``), the key -> row map of ``DataFrame.join``, over the library's
index, with the device gather (``take_device``) and the inner join's compaction
(``index_matched``) a join needs next to it.  ``argsort_device`` and ``mask_rows`` are the two
primitives of ``DataFrame.sort`` / ``extract`` (sort.py): the stable
lexicographic order of device key columns and the kept rows of a device mask.

Ordinals are assigned in first-appearance order over all ``update`` calls -- what a
single-threaded reference ``update`` with ``nmaps = 1`` produces.  (With threads the
reference's order depends on interleaving and ``nmaps``; groupby results are compared
as key -> value maps)
"""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray
from .superagg import _column

DTYPES = _lib.DTYPES


class _HashBase:
    """What the three hash handles share: the C handle (``<prefix>_create`` / ``_destroy``),
    ``<prefix>_info`` (length, nan_count, null_count, then the engine's own words), the
    parsing of ``update(keys[, mask], ...)`` and where a mask / select column has to be."""
    _dtype = "int64"
    _prefix = None    # vh_set / vh_counter / vh_index
    _info_words = 5   # int64 words <prefix>_info writes

    def _create(self, *args):
        h = ctypes.c_void_p()
        _lib.call(self._prefix + "_create", _lib.DTYPE_CODE[self._dtype], *args, ctypes.byref(h))
        self._handle = h.value

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            try:
                _lib.call(self._prefix + "_destroy", h)
            except Exception:
                pass
            self._handle = None

    def _info(self, *more):
        vals = [ctypes.c_int64() for _ in range(self._info_words)]
        _lib.call(self._prefix + "_info", self._handle, *[ctypes.byref(v) for v in vals], *more)
        return [v.value for v in vals]

    def __len__(self):
        return self._info()[0]

    def length(self):
        return len(self)

    def __sizeof__(self):
        return len(self) * 16

    nan_count = property(lambda self: self._info()[1])
    null_count = property(lambda self: self._info()[2])
    has_nan = property(lambda self: self._info()[1] > 0)
    has_null = property(lambda self: self._info()[2] > 0)

    @staticmethod
    def _update_args(ar, args, kwargs):
        """``(ar, *args, **kwargs)`` of an update call as (keys, mask, the other positional
        arguments); a masked array gives its data and adds its mask.  Pops ``mask`` from kwargs."""
        mask = None
        rest = list(args)
        if rest and (isinstance(rest[0], (np.ndarray, list, DeviceArray)) or rest[0] is None):
            mask = rest.pop(0)
        mask = kwargs.pop("mask", mask)
        if np.ma.isMaskedArray(ar):
            m = np.ma.getmaskarray(ar)
            mask = m if mask is None else (np.asarray(mask, bool) | m)
            ar = ar.data
        return ar, mask, rest

    @staticmethod
    def _side(a, device):
        """A mask / select column where the keys are: (object kept alive, pointer)."""
        if a is None:
            return None, None
        if device:
            if not isinstance(a, DeviceArray):
                a = DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=np.uint8))
            return a, a.ptr
        if isinstance(a, DeviceArray):
            a = a.to_numpy()
        a = np.ascontiguousarray(a, dtype=np.uint8)
        return a, a.ctypes.data


class _OrderedSetBase(_HashBase):
    _prefix = "vh_set"

    def __init__(self, *args):
        self._create()
        self.fingerprint = ""
        self.sealed = False
        if len(args) >= 4:
            # ordered_set::create(keys, null_value, nan_count, null_count, fingerprint)
            # (hash_primitives.hpp:468-516): keys in order get ordinals 0..n-1
            keys, null_value, nan_count, null_count = args[:4]
            keys = np.asarray(keys, dtype=self._dtype)
            mask = None
            if null_count:
                mask = np.zeros(len(keys), np.uint8)
                mask[int(null_value)] = 1
            self.update(keys, mask)
            if len(self) != len(keys):
                raise RuntimeError(f"key array of length {len(keys)} does not match expected length of {len(self)}")
            if bool(nan_count) != self.has_nan:
                raise RuntimeError("NaN found in data, while claiming there should be none" if self.has_nan
                                   else "no NaN found in data, while claiming there should be")
            if len(args) >= 5 and args[4] is not None:
                self.fingerprint = args[4]
            self.sealed = True

    # ---- building --------------------------------------------------------------
    def update(self, ar, *args, **kwargs):
        """update(keys[, mask], start_index=0, chunk_size=..., bucket_size=..., return_values=False)"""
        ar, mask, _ = self._update_args(ar, args, kwargs)
        # select (this build): only rows where select != 0 enter the set (a filtered or
        # selected chunk, evaluated on the device, without compacting it)
        select = kwargs.pop("select", None)
        return_values = kwargs.get("return_values", False)
        if not isinstance(ar, DeviceArray):
            ar = np.ascontiguousarray(ar, dtype=self._dtype)
        kptr, n, _, _, loc, keep = _column(ar)
        mptr = None
        mkeep = None
        if mask is not None:
            mkeep = np.ascontiguousarray(mask, dtype=np.uint8) if not isinstance(mask, DeviceArray) else mask
            mptr = mkeep.ctypes.data if isinstance(mkeep, np.ndarray) else mkeep.ptr
        if select is not None:
            skeep = select if isinstance(select, DeviceArray) else np.ascontiguousarray(select, dtype=np.uint8)
            sptr = skeep.ptr if isinstance(skeep, DeviceArray) else skeep.ctypes.data
            _lib.call("vh_set_update_selected", self._handle, kptr, mptr, sptr, n, loc)
        else:
            _lib.call("vh_set_update", self._handle, kptr, mptr, n, loc)
        if return_values:
            ordinals = self.map_ordinal(ar).astype(np.int64)
            if mask is not None:
                ordinals[np.asarray(mask, bool)] = self.null_value
            return ordinals, np.zeros(len(ordinals), np.int16)
        return None

    def merge(self, others):
        if self.sealed:
            raise RuntimeError("hashmap is sealed, cannot merge")
        for o in others:
            keys = o.key_array()
            mask = None
            if o.has_null:
                mask = np.zeros(len(keys), np.uint8)
                mask[o.null_value] = 1
            self.update(keys, mask)

    def seal(self):
        self.sealed = True

    # ---- reading ---------------------------------------------------------------
    nan_value = property(lambda self: self._info()[3])
    null_value = property(lambda self: self._info()[4])

    def key_array(self):
        n = len(self)
        out = np.empty(n, dtype=self._dtype)
        if n:
            _lib.call("vh_set_key_array", self._handle, out.ctypes.data)
        return out

    def keys(self):
        ka = self.key_array().tolist()
        if self.has_null:
            ka[self.null_value] = None
        return ka

    def _ordinal_dtype(self):
        n = len(self)
        return np.int8 if n < 2 ** 7 else np.int16 if n < 2 ** 15 else np.int32 if n < 2 ** 31 else np.int64

    def map_ordinal(self, keys):
        """key -> ordinal, -1 for unknown keys; dtype sized by len(set) (hash_primitives.hpp:543-583)."""
        out_dtype = np.dtype(self._ordinal_dtype())
        if isinstance(keys, DeviceArray):
            out = DeviceArray(len(keys), out_dtype)
            _lib.call("vh_set_map_ordinal", self._handle, keys.ptr, len(keys), _lib.LOC_DEVICE, out.ptr,
                      out_dtype.itemsize, _lib.LOC_DEVICE)
            return out
        if np.ma.isMaskedArray(keys):
            keys = keys.data
        keys = np.ascontiguousarray(keys, dtype=self._dtype)
        out = np.empty(len(keys), out_dtype)
        if len(keys):
            _lib.call("vh_set_map_ordinal", self._handle, keys.ctypes.data, len(keys), _lib.LOC_HOST,
                      out.ctypes.data, out_dtype.itemsize, _lib.LOC_HOST)
        return out

    def isin(self, values):
        return self.map_ordinal(np.asarray(values, dtype=self._dtype)) >= 0

    def flatten_values(self, values, map_index, out):
        out[:] = values  # one map: offsets are all 0 (hash_common::flatten_values)
        return out

    def __reduce__(self):
        keys = self.key_array()
        return (type(self), (keys, self.null_value, self.nan_count, self.null_count, self.fingerprint))


# slots of the LDS table a workgroup counts into (counter.hip CT_LT)
COUNTER_LDS_SLOTS = 8192


class _CounterBase(_HashBase):
    """``counter_<dtype>`` (``hash_primitives.hpp:328-415``; bindings ``hash_primitives.cpp``
    ``init_hash_``): key -> occurrence count over the GPU hash counter of libvaexhip.

    ``key_array()`` and ``counts()`` are in key order: NaN at index 0 when present, the null
    entry next (``key_offset``, hash_primitives.hpp:338-348), then the regular keys ascending
    (the reference's order is its hash maps' iteration order; value_counts sorts by count).
    ``counter_<t>(keys, counts, null_index)`` rebuilds one (``__reduce__``);
    ``counter_<t>(initial_capacity=16)`` starts the table at 16 slots."""
    _prefix = "vh_counter"
    _info_words = 3

    def __init__(self, *args, initial_capacity=0):
        if len(args) == 1 and isinstance(args[0], (int, np.integer)):
            args = ()  # counter(nmaps): one table on the GPU
        self._create(int(initial_capacity))
        if len(args) >= 2:
            keys, counts = args[:2]
            null_index = args[2] if len(args) > 2 else -1
            keys = np.asarray(keys, dtype=self._dtype)
            mask = None
            if null_index is not None and null_index >= 0:
                mask = np.zeros(len(keys), np.uint8)
                mask[int(null_index)] = 1
            self._add(keys, mask, counts)

    # ---- building --------------------------------------------------------------
    def update(self, ar, *args, **kwargs):
        """update(keys[, mask], select=None): rows where select == 0 are not seen at all."""
        ar, mask, _ = self._update_args(ar, args, kwargs)
        select = kwargs.pop("select", None)
        if not isinstance(ar, DeviceArray):
            ar = np.ascontiguousarray(ar, dtype=self._dtype)
        device = isinstance(ar, DeviceArray)
        if device and ar.dtype.itemsize != np.dtype(self._dtype).itemsize:
            raise TypeError(f"counter_{self._dtype} cannot take a {ar.dtype} column")
        kptr, n, _, _, loc, keep = _column(ar)
        mkeep, mptr = self._side(mask, device)
        skeep, sptr = self._side(select, device)
        if n:
            _lib.call("vh_counter_update", self._handle, kptr, mptr, sptr, n, loc)

    def _add(self, keys, mask, counts):
        keys = np.ascontiguousarray(keys, dtype=self._dtype)
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        if len(keys) != len(counts):
            raise ValueError("keys and counts differ in length")
        mkeep, mptr = self._side(mask, False)
        if len(keys):
            _lib.call("vh_counter_add", self._handle, keys.ctypes.data, mptr, counts.ctypes.data, len(keys), _lib.LOC_HOST)

    def merge(self, other):
        """counter::merge (hash_primitives.hpp:394-415): add every count of ``other``."""
        keys, counts, null_index = other._read(0, False, False)
        mask = None
        if null_index >= 0:
            mask = np.zeros(len(keys), np.uint8)
            mask[null_index] = 1
        self._add(keys, mask, counts)

    # ---- reading ---------------------------------------------------------------
    def _read(self, order, dropnan, dropmissing):
        n = len(self)
        keys = np.empty(n, dtype=self._dtype)
        counts = np.empty(n, dtype=np.int64)
        n_out, null_index = ctypes.c_uint64(), ctypes.c_int64(-1)
        _lib.call("vh_counter_read", self._handle, int(order), int(bool(dropnan)), int(bool(dropmissing)),
                  keys.ctypes.data, counts.ctypes.data, ctypes.byref(n_out), ctypes.byref(null_index))
        return keys[:n_out.value], counts[:n_out.value], null_index.value

    def key_array(self):
        return self._read(0, False, False)[0]

    def counts(self):
        return self._read(0, False, False)[1]

    @property
    def null_index(self):
        """Index of the null entry in key_array() / counts(), -1 when absent."""
        return int(self.has_nan) if self.has_null else -1

    def extract(self):
        """{regular key: count} (hash_base::extract)."""
        keys, counts, _ = self._read(0, True, True)
        return dict(zip(keys.tolist(), counts.tolist()))

    def sorted_counts(self, ascending=False, dropnan=False, dropmissing=False):
        """The device finish of value_counts: (keys, counts, null_index) with the NaN / null
        entries dropped as asked and the rest stably sorted by count (ascending), or the exact
        reverse of that (expression.py:1026-1050); only the answer crosses the host link."""
        return self._read(1 if ascending else 2, dropnan, dropmissing)

    def __reduce__(self):
        keys, counts, null_index = self._read(0, False, False)
        return (type(self), (keys, counts, null_index))


# keys of <= 4 bytes the index probe's LDS route holds (index.hip IX_LDS_BYTES = 64 KiB = 8192
# packed slots, at half load; 8-byte keys: half as many): up to this many distinct keys (in an update of as many rows) the
# sealed lookup table is staged in LDS once per workgroup, past it the probe reads it from HBM
INDEX_LDS_KEYS = 4096


class _IndexHashBase(_HashBase):
    """``index_hash_<dtype>`` (``hash_primitives.hpp:623-900``; bindings
    ``hash_primitives.cpp:53-69``): key -> the first row it was seen at, plus the other rows
    of duplicated keys, over the GPU index of libvaexhip -- the hash map of ``DataFrame.join``.

    The contract is the single-threaded, one-map, rows-in-order reference: a key maps to its
    first row, ``nan_value`` / ``null_value`` to the last NaN / null row.  Key identity is the
    other GPU hash engines': by bit pattern, with one NaN entry, so ``-0.0`` and ``0.0`` are two
    keys (the reference compares keys with ``==``).  ``map_index`` of a NaN / null key when the
    index holds none gives ``-1`` (the reference leaves that entry uninitialised).  The first
    probe seals the index: ``update`` and ``merge`` raise after it.
    ``index_hash_<t>(initial_capacity=16)`` starts the table at 16 slots."""
    _prefix = "vh_index"

    def __init__(self, *args, initial_capacity=0):
        self._create(int(initial_capacity))

    # ---- building --------------------------------------------------------------
    def _keys(self, ar):
        if np.ma.isMaskedArray(ar):
            ar = ar.data
        if isinstance(ar, DeviceArray):
            if ar.dtype.itemsize != np.dtype(self._dtype).itemsize:
                raise TypeError(f"index_hash_{self._dtype} cannot take a {ar.dtype} column")
            return ar
        ar = np.asarray(ar)
        if ar.dtype.kind in "mM":
            ar = ar.view(np.int64)
        return np.ascontiguousarray(ar, dtype=self._dtype)

    def update(self, ar, *args, **kwargs):
        """update(keys[, mask], start_index=0, select=None): row i is row ``start_index + i``;
        rows where select == 0 are not seen at all."""
        ar, mask, rest = self._update_args(ar, args, kwargs)
        start_index = kwargs.pop("start_index", rest.pop(0) if rest else 0)
        select = kwargs.pop("select", None)
        ar = self._keys(ar)
        device = isinstance(ar, DeviceArray)
        kptr, n, _, _, loc, keep = _column(ar)
        mkeep, mptr = self._side(mask, device)
        skeep, sptr = self._side(select, device)
        if n:
            _lib.call("vh_index_update", self._handle, kptr, mptr, sptr, n, int(start_index), loc)

    def merge(self, other):
        """index_hash::merge (hash_primitives.hpp:850-894): every row ``other`` has seen,
        under the same row number.  Raises once either index was probed."""
        _lib.call("vh_index_merge", self._handle, other._handle)

    # ---- reading ---------------------------------------------------------------
    def _info(self):
        dup = ctypes.c_int()
        return super()._info(ctypes.byref(dup)) + [bool(dup.value)]

    nan_value = property(lambda self: self._info()[3])
    null_value = property(lambda self: self._info()[4])
    has_duplicates = property(lambda self: self._info()[5])

    def _map(self, values, mask, out):
        values = self._keys(values)
        device = isinstance(values, DeviceArray)
        n = len(values)
        if out is None:
            out = DeviceArray(n, np.int64) if device else np.empty(n, np.int64)
        if len(out) != n:
            raise ValueError("map_index: out and values differ in length")
        odt = np.dtype(out.dtype)
        if odt not in (np.dtype(np.int32), np.dtype(np.int64)):
            raise TypeError("map_index: out must be int32 or int64")
        if isinstance(out, DeviceArray):
            optr, oloc = out.ptr, _lib.LOC_DEVICE
        else:
            if not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.flags.writeable):
                raise TypeError("map_index: out must be a contiguous writeable array")
            optr, oloc = out.ctypes.data, _lib.LOC_HOST
        mkeep, mptr = self._side(mask, device)
        if mkeep is not None and len(mkeep) != n:
            raise ValueError("map_index: mask and values differ in length")
        found = ctypes.c_int(0)
        kptr = values.ptr if device else values.ctypes.data
        _lib.call("vh_index_map_index", self._handle, kptr, mptr, n, _lib.LOC_DEVICE if device else _lib.LOC_HOST,
                  optr, odt.itemsize, oloc, ctypes.byref(found))
        return out, bool(found.value)

    def map_index(self, values, out=None):
        """key -> first row, -1 for unknown keys (hash_primitives.hpp:679-714).  Without ``out``
        returns int64 (a DeviceArray for a DeviceArray of keys); with ``out`` (int32 / int64,
        host or device) writes into it and returns whether any -1 was written."""
        res, found = self._map(values, None, out)
        return res if out is None else found

    def map_index_masked(self, values, mask, out=None):
        """map_index with a mask (1 = null -> null_value; hash_primitives.hpp:715-754)."""
        res, found = self._map(values, mask, out)
        return res if out is None else found

    def map_index_duplicates(self, values, *args, on_device=False):
        """map_index_duplicates(values[, mask], start_index) -> (left_indices, right_indices):
        one pair per duplicate row of each left row's key, in left-row order, duplicates
        ascending (hash_primitives.hpp:756-848).  Host int64 arrays; on_device=True: int64
        DeviceArrays (the pairs never leave HBM)."""
        rest = list(args)
        mask = None
        if rest and not isinstance(rest[0], (int, np.integer)):
            mask = rest.pop(0)
        start_index = int(rest.pop(0)) if rest else 0
        values = self._keys(values)
        device = isinstance(values, DeviceArray)
        mkeep, mptr = self._side(mask, device)
        n_out = ctypes.c_uint64(0)
        kptr = values.ptr if device else values.ctypes.data
        # the pairs are counted and kept in the library, then read with a second call
        _lib.call("vh_index_map_index_duplicates", self._handle, kptr, mptr, len(values), start_index,
                  _lib.LOC_DEVICE if device else _lib.LOC_HOST, ctypes.byref(n_out), None, None)
        if on_device:
            left, right = DeviceArray(n_out.value, np.int64), DeviceArray(n_out.value, np.int64)
            lptr, rptr = left.ptr, right.ptr
        else:
            left, right = np.empty(n_out.value, np.int64), np.empty(n_out.value, np.int64)
            lptr, rptr = left.ctypes.data, right.ctypes.data
        _lib.call("vh_index_map_index_duplicates", self._handle, None, None, 0, 0, _lib.LOC_HOST, ctypes.byref(n_out),
                  lptr, rptr)
        return left, right

def take_device(columns, indices, with_mask=False):
    """Device gather (vh_take): ``[c[indices] for c in columns]`` for DeviceArray columns and a
    DeviceArray of int32 / int64 indices; a negative index gives 0.  Eight columns share one
    pass over the indices.  with_mask: also the DeviceArray of ``indices < 0`` (uint8)."""
    n = len(indices)
    if np.dtype(indices.dtype) not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise TypeError("take: indices must be int32 or int64")
    outs = [DeviceArray(n, c.dtype) for c in columns]
    mask = DeviceArray(n, np.uint8) if with_mask else None
    k = len(columns)
    dsts = (ctypes.c_void_p * max(k, 1))(*[o.ptr for o in outs])
    srcs = (ctypes.c_void_p * max(k, 1))(*[c.ptr for c in columns])
    isz = (ctypes.c_int * max(k, 1))(*[c.dtype.itemsize for c in columns])
    _lib.call("vh_take", k, dsts, srcs, isz, indices.ptr, indices.dtype.itemsize, n, mask.ptr if with_mask else None)
    return (outs, mask) if with_mask else outs


def index_matched(lookup):
    """The inner join's compaction (vh_index_matched): for a DeviceArray lookup, the positions
    with ``lookup >= 0`` (int64 DeviceArray) and the lookup entries there."""
    n = len(lookup)
    rows = DeviceArray(n, np.int64)
    out = DeviceArray(n, lookup.dtype)
    m = ctypes.c_uint64(0)
    _lib.call("vh_index_matched", lookup.ptr, lookup.dtype.itemsize, n, ctypes.byref(m), rows.ptr, out.ptr)
    return rows[:m.value], out[:m.value]


# output positions a workgroup of the argsort's encode kernel takes per step (sort.hip: 256
# lanes of SE_RPT = 4) and the most key columns one argsort takes (sort_plan.hpp SORT_MAX_KEYS)
SORT_ENCODE_TILE = 1024
SORT_MAX_KEYS = 16


def _row_dtype(n):
    """Row numbers of a column of n rows: int32 while they fit (they feed ``take_device``)."""
    return np.dtype(np.int32 if n < 2 ** 31 else np.int64)


def mask_rows(mask):
    """The kept rows of a device byte mask (``vh_mask_rows``): ``np.flatnonzero(mask)`` as a
    DeviceArray of int32 (int64 from 2^31 rows)."""
    mask = _device_mask(mask)
    n = len(mask)
    rows = DeviceArray(n, _row_dtype(n))
    m = ctypes.c_uint64(0)
    _lib.call("vh_mask_rows", mask.ptr, n, rows.dtype.itemsize, rows.ptr, ctypes.byref(m))
    return rows[:m.value]


def argsort_device(keys, rows=None, ascending=True):
    """Stable argsort of DeviceArray key columns on the device (``vh_argsort``): the row
    numbers (DeviceArray of int32, int64 from 2^31 rows) in the order of
    ``np.lexsort(keys[::-1])`` -- one key: ``np.argsort(kind="stable")`` -- so the first key is
    the most significant, NaN sorts last and ``-0.0 == 0.0``; ``ascending=False`` gives the
    exact reverse.  ``rows``: an ascending DeviceArray of row numbers (``mask_rows``); only
    those rows are sorted.  datetime keys sort as int64."""
    keys = [keys] if isinstance(keys, DeviceArray) else list(keys)
    if not 1 <= len(keys) <= SORT_MAX_KEYS:
        raise ValueError(f"argsort takes 1 to {SORT_MAX_KEYS} key columns")
    for c in keys:
        if not isinstance(c, DeviceArray):
            raise TypeError("argsort_device takes DeviceArray key columns")
    n = len(keys[0])
    if any(len(c) != n for c in keys):
        raise ValueError("key columns differ in length")
    rdt = _row_dtype(n)
    if rows is not None:
        if not isinstance(rows, DeviceArray) or np.dtype(rows.dtype) != rdt:
            raise TypeError(f"rows must be a DeviceArray of {rdt} (what mask_rows returns)")
    m = n if rows is None else len(rows)
    out = DeviceArray(m, rdt)
    k = len(keys)
    kptr = (ctypes.c_void_p * k)(*[c.ptr for c in keys])
    codes = (ctypes.c_int * k)(*[_lib.dtype_code(c.dtype)[0] for c in keys])
    _lib.call("vh_argsort", k, kptr, codes, n, None if rows is None else rows.ptr, rdt.itemsize, m,
              0 if ascending else 1, out.ptr)
    return out


# edges of a lasso a workgroup stages in LDS at a time (select.hip PP_CHUNK) and the rows a
# workgroup takes per step (PP_TILE: 256 lanes of 8 rows)
PNPOLY_LDS_EDGES = 512
PNPOLY_WG_ROWS = 2048


def _device_mask(a):
    """A mask as a DeviceArray of bytes (a host mask is staged)."""
    if isinstance(a, DeviceArray):
        if a.dtype.itemsize != 1:
            raise TypeError("a mask holds one byte per row")
        return a
    return DeviceArray.from_numpy(np.ascontiguousarray(a).view(np.uint8) if np.asarray(a).dtype == np.bool_
                                  else np.ascontiguousarray(a, dtype=np.uint8))


def pnpoly(x, y, xseq, yseq, prev=None, mode="replace"):
    """The lasso: ``mode(prev == 1, inside(x, y))`` for the polygon with the vertices
    (xseq[k], yseq[k]), ``inside`` being vaexfast.pnpoly (vaexfast.cpp:1757-1775) with the
    mean / radius pre-test of SelectionLasso.evaluate (selections.py:182-185).  DeviceArray
    columns (float64 / float32, each its own dtype; a mixed pair stages the host one) go to the
    kernel (``vh_pnpoly``) and give a DeviceArray of bool: only the vertices cross to the
    device, nothing comes back.  NumPy columns take the host path (``hostops.pnpoly``) and give
    a bool array.  ``prev``: a mask of which only bytes equal to 1 count; without it, and / or /
    xor give the new mask and subtract its complement.  An empty polygon holds no point."""
    from . import hostops
    from .selections import _select_functions
    if mode not in _lib.SELECT_MODE:
        raise ValueError(f"unknown selection mode {mode!r}")
    vx = np.ascontiguousarray(xseq, dtype=np.float64)
    vy = np.ascontiguousarray(yseq, dtype=np.float64)
    if vx.ndim != 1 or vx.shape != vy.shape:
        raise ValueError("xseq and yseq must be two sequences of equal length")
    if len(x) != len(y) or (prev is not None and len(prev) != len(x)):
        raise ValueError("x, y and prev differ in length")
    meanx, meany, radius = hostops.lasso_bounds(vx, vy)
    if not isinstance(x, DeviceArray) and not isinstance(y, DeviceArray):
        mask = hostops.pnpoly(x, y, vx, vy, meanx, meany, radius)
        if prev is not None:
            prev = prev.to_numpy() if isinstance(prev, DeviceArray) else np.asarray(prev)
            prev = prev.view(np.uint8) == 1 if prev.dtype == np.bool_ else prev == 1
        return _select_functions[mode](prev, mask)
    cols = []
    for c in (x, y):
        if not isinstance(c, DeviceArray):
            c = np.asarray(c)
            c = DeviceArray.from_numpy(c if c.dtype == np.float32 else c.astype(np.float64))
        if c.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError(f"pnpoly takes float64 / float32 columns, not {c.dtype}")
        cols.append(c)
    pkeep = None if prev is None else _device_mask(prev)
    out = DeviceArray(len(x), np.bool_)
    dp = ctypes.POINTER(ctypes.c_double)
    _lib.call("vh_pnpoly", cols[0].ptr, _lib.dtype_code(cols[0].dtype)[0], cols[1].ptr, _lib.dtype_code(cols[1].dtype)[0],
              len(x), vx.ctypes.data_as(dp), vy.ctypes.data_as(dp), len(vx), meanx, meany, radius,
              None if pkeep is None else pkeep.ptr, _lib.SELECT_MODE[mode], out.ptr)
    return out


def mask_combine(a, b=None, mode="and"):
    """``mode(a == 1, b == 1)`` of two device masks as a new DeviceArray of bool
    (``vh_mask_combine``); ``b`` None: the complement of ``a``."""
    a = _device_mask(a)
    bkeep = None if b is None else _device_mask(b)
    if bkeep is not None and len(bkeep) != len(a):
        raise ValueError("masks differ in length")
    out = DeviceArray(len(a), np.bool_)
    _lib.call("vh_mask_combine", a.ptr, None if bkeep is None else bkeep.ptr, _lib.SELECT_MODE[mode], len(a), out.ptr)
    return out


def _register():
    ns = globals()
    for dtype in DTYPES:
        name = "index_hash_" + dtype
        ns[name] = type(name, (_IndexHashBase,), {"_dtype": dtype, "__module__": __name__})
        name = "ordered_set_" + dtype
        ns[name] = type(name, (_OrderedSetBase,), {"_dtype": dtype, "__module__": __name__})
        name = "counter_" + dtype
        ns[name] = type(name, (_CounterBase,), {"_dtype": dtype, "__module__": __name__})


_register()


def counter_type_from_dtype(dtype, transient=True):
    """vaex.hash.counter_type_from_dtype for primitive dtypes (datetimes count as int64)."""
    dt = np.dtype(dtype)
    name = "int64" if dt.kind in "mM" else dt.newbyteorder("=").name
    return globals()["counter_" + name]


def index_type_from_dtype(dtype, transient=True, prime_growth=False):
    """vaex.hash.index_type_from_dtype for primitive dtypes (datetimes index as int64);
    transient and prime_growth have no meaning for the one GPU table."""
    dt = np.dtype(dtype)
    name = "int64" if dt.kind in "mM" else dt.newbyteorder("=").name
    return globals()["index_hash_" + name]


def ordered_set_type_from_dtype(dtype):
    """vaex.hash.ordered_set_type_from_dtype for primitive dtypes."""
    dt = np.dtype(dtype)
    if dt.kind in "mM":
        name = "int64"
    else:
        name = dt.newbyteorder("=").name
    return globals()["ordered_set_" + name]
