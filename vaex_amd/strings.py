"""String columns in HBM: :class:`DeviceStringArray` (the reference's ``ColumnStringArrow``,
``column.py:602-754``), the dictionary encoder :class:`ordered_set_string`
(``superutils.ordered_set_string`` over ``hash_string.hpp``), the device string functions
(``functions.py`` ``str_*``: ``str_len``, ``str_byte_length``, ``str_equals``, ``str_notequals``,
``str_startswith``, ``str_endswith``, ``str_contains`` with a literal pattern), the byte-exact
gather, and the helpers that let the integer engines run on encoded string keys
(``value_counts`` / ``unique`` / ``groupby`` / ``sort``).

A column is the Arrow layout: ``length + 1`` int32 / int64 offsets and a byte buffer, both in
HBM.  The byte buffer's allocation carries :data:`SLACK` bytes after the last byte and slices
share their parent's allocation, so the kernels may read whole aligned words.  Offsets handed
in by a caller are checked on the device before anything dereferences them.  Nulls are not
supported (as NaT and masks are not for datetimes): input with a null raises
``NotImplementedError``."""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray

SLACK = 16            # bytes allocated after a column's last byte
MAX_PATTERN = 1024    # bytes of a literal pattern (strings.hip stages it in LDS)
MATCH_OPS = {"str_equals": 0, "str_notequals": 1, "str_startswith": 2, "str_endswith": 3, "str_contains": 4}
LEN_KINDS = {"str_byte_length": 0, "str_len": 1}
FUNCTIONS = tuple(MATCH_OPS) + tuple(LEN_KINDS)


class _StringType:
    """The ``data_type`` of a string column: equal to ``str``, ``kind == "T"``."""
    kind = "T"
    name = "string"

    def __eq__(self, other):
        return other is str or isinstance(other, _StringType) or other in ("str", "string")

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(str)

    def __repr__(self):
        return "string"


STRING = _StringType()


def take_offset_dtype(input_dtype, total_bytes):
    """The offset dtype of a taken column: the input's, int64 once the bytes reach 2^31
    (``take_needs_wide`` of csrc/str_dev.hpp)."""
    if np.dtype(input_dtype) == np.int64 or total_bytes >= 2 ** 31:
        return np.dtype(np.int64)
    return np.dtype(np.int32)


def _bytes_buffer(data):
    """A uint8 DeviceArray holding ``data`` (a uint8 array) with SLACK bytes allocated after it."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    full = DeviceArray(len(data) + SLACK, np.uint8)
    if len(data):
        _lib.call("vh_memcpy_htod", full.ptr, data.ctypes.data, len(data))
    return full, len(data)


class DeviceStringArray:
    """``length`` strings in HBM.  ``offsets``: DeviceArray of int32 / int64, ``length + 1``
    entries; ``bytes``: DeviceArray of uint8 (the parent's whole buffer for a slice, whose first
    offset then need not be 0)."""
    dtype = STRING

    def __init__(self, offsets, bytes, _checked=False, _root=None):
        if not isinstance(offsets, DeviceArray) or not isinstance(bytes, DeviceArray):
            raise TypeError("offsets and bytes are DeviceArrays")
        if np.dtype(offsets.dtype) not in (np.dtype(np.int32), np.dtype(np.int64)) or len(offsets) < 1:
            raise ValueError("offsets: length + 1 entries of int32 or int64")
        if np.dtype(bytes.dtype) != np.uint8:
            raise ValueError("bytes: a uint8 buffer")
        self.offsets = offsets
        self.length = len(offsets) - 1
        if _root is None:
            # a caller's buffer: copy it into an allocation with the slack the kernels rely on
            full = DeviceArray(len(bytes) + SLACK, np.uint8)
            if len(bytes):
                _lib.call("vh_memcpy_dtod", full.ptr, bytes.ptr, len(bytes))
            _root = (full, len(bytes))
        self._root = _root  # (the allocation, the bytes of it that offsets may address)
        if not _checked:
            bad = ctypes.c_int(0)
            _lib.call("vh_str_validate", offsets.ptr, offsets.dtype.itemsize, self.length, self._root[1], ctypes.byref(bad))
            if bad.value:
                what = [w for b, w in ((1, "negative"), (2, "decreasing"), (4, "past the end of the bytes")) if bad.value & b]
                raise ValueError("string offsets are " + ", ".join(what))

    @property
    def bytes(self):
        full, n = self._root
        return full[:n]

    # ---- construction -----------------------------------------------------------------------------
    @classmethod
    def _from_host(cls, offsets, data):
        full, n = _bytes_buffer(data)
        return cls(DeviceArray.from_numpy(offsets), full, _checked=True, _root=(full, n))

    @classmethod
    def from_arrow(cls, ar):
        import pyarrow as pa
        if isinstance(ar, pa.ChunkedArray):
            ar = ar.combine_chunks() if ar.num_chunks != 1 else ar.chunk(0)
        if not (pa.types.is_string(ar.type) or pa.types.is_large_string(ar.type)):
            raise TypeError(f"from_arrow takes a string or large_string array, not {ar.type}")
        if ar.null_count:
            raise NotImplementedError("string columns with nulls are not supported")
        odt = np.int64 if pa.types.is_large_string(ar.type) else np.int32
        n = len(ar)
        bufs = ar.buffers()
        offsets = np.frombuffer(bufs[1], dtype=odt, count=n + 1, offset=ar.offset * np.dtype(odt).itemsize) \
            if bufs[1] is not None and n + 1 > 0 and bufs[1].size else np.zeros(1, odt)
        data = np.frombuffer(bufs[2], dtype=np.uint8) if bufs[2] is not None and bufs[2].size else np.zeros(0, np.uint8)
        lo, hi = int(offsets[0]), int(offsets[-1])
        return cls._from_host(np.ascontiguousarray(offsets - lo, dtype=odt), data[lo:hi])

    @classmethod
    def from_list(cls, values, large=False):
        enc = []
        for v in values:
            if v is None:
                raise NotImplementedError("string columns with nulls are not supported")
            if not isinstance(v, str):
                raise TypeError(f"a string column holds str, not {type(v).__name__}")
            enc.append(v.encode("utf-8", "surrogatepass"))
        lens = np.fromiter((len(b) for b in enc), dtype=np.int64, count=len(enc))
        offsets = np.zeros(len(enc) + 1, np.int64)
        np.cumsum(lens, out=offsets[1:])
        odt = np.int64 if large or offsets[-1] >= 2 ** 31 else np.int32
        return cls._from_host(offsets.astype(odt), np.frombuffer(b"".join(enc), dtype=np.uint8))

    @classmethod
    def from_numpy(cls, ar, large=False):
        ar = np.asarray(ar)
        if ar.dtype.kind not in "OU" or ar.ndim != 1:
            raise TypeError("from_numpy takes a 1-d object or unicode array")
        return cls.from_list(ar.tolist(), large=large)

    # ---- a DeviceArray's surface ------------------------------------------------------------------
    def __len__(self):
        return self.length

    @property
    def shape(self):
        return (self.length,)

    @property
    def ndim(self):
        return 1

    @property
    def nbytes(self):
        """offsets plus the bytes this column's rows span"""
        lo, hi = self._span()
        return self.offsets.nbytes + (hi - lo)

    def _span(self):
        o = self.offsets
        ends = np.concatenate([o[:1].to_numpy(), o[self.length:].to_numpy()])
        return int(ends[0]), int(ends[-1])

    def __getitem__(self, item):
        if not isinstance(item, slice):
            raise TypeError("DeviceStringArray only supports contiguous slices")
        start, stop, step = item.indices(self.length)
        if step != 1:
            raise TypeError("DeviceStringArray only supports contiguous slices")
        stop = max(start, stop)
        return DeviceStringArray(self.offsets[start:stop + 1], self._root[0], _checked=True, _root=self._root)

    # ---- readers ------------------------------------------------------------------------------------
    def _host(self):
        offsets = self.offsets.to_numpy()
        lo, hi = int(offsets[0]), int(offsets[-1])
        data = self._root[0][lo:hi].to_numpy()
        return offsets - offsets[0], data

    def to_arrow(self):
        import pyarrow as pa
        offsets, data = self._host()
        typ = pa.large_string() if offsets.dtype == np.int64 else pa.string()
        return pa.Array.from_buffers(typ, self.length, [None, pa.py_buffer(offsets), pa.py_buffer(data)])

    def tolist(self):
        offsets, data = self._host()
        raw = data.tobytes()
        o = offsets.tolist()
        return [raw[o[i]:o[i + 1]].decode("utf-8", "surrogatepass") for i in range(self.length)]

    def to_numpy(self):
        out = np.empty(self.length, dtype=object)
        out[:] = self.tolist()
        return out

    def __array__(self, dtype=None, copy=None):
        return self.to_numpy()

    def __repr__(self):
        return f"DeviceStringArray(length={self.length}, offsets={self.offsets.dtype})"

    # ---- kernels ------------------------------------------------------------------------------------
    def _args(self):
        return self.offsets.ptr, self.offsets.dtype.itemsize, self._root[0].ptr

    def take(self, indices):
        """``column[indices]`` for a DeviceArray of int32 / int64 row numbers (``vh_str_take``):
        byte-exact; the offsets keep their width unless the bytes reach 2^31."""
        if not isinstance(indices, DeviceArray) or np.dtype(indices.dtype) not in (np.dtype(np.int32), np.dtype(np.int64)):
            raise TypeError("take: indices are a DeviceArray of int32 or int64")
        m = len(indices)
        pos = DeviceArray(m + 1, np.uint64)
        total = ctypes.c_uint64(0)
        optr, oisz, bptr = self._args()
        _lib.call("vh_str_take_plan", optr, oisz, self.length, indices.ptr, indices.dtype.itemsize, m, pos.ptr,
                  ctypes.byref(total))
        odt = take_offset_dtype(self.offsets.dtype, total.value)
        out_off = DeviceArray(m + 1, odt)
        full = DeviceArray(total.value + SLACK, np.uint8)
        _lib.call("vh_str_take", optr, oisz, bptr, self.length, indices.ptr, indices.dtype.itemsize, m, pos.ptr, total.value,
                  out_off.ptr, odt.itemsize, full.ptr)
        return DeviceStringArray(out_off, full, _checked=True, _root=(full, total.value))

    def len(self, kind="str_len"):
        """int64 DeviceArray: code points (``str_len``) or bytes (``str_byte_length``)."""
        out = DeviceArray(self.length, np.int64)
        optr, oisz, bptr = self._args()
        _lib.call("vh_str_len", optr, oisz, bptr, self.length, LEN_KINDS[kind], out.ptr)
        return out

    def match(self, op, pattern):
        """bool DeviceArray: every row against the literal ``pattern`` (``op``: a key of MATCH_OPS)."""
        pat = _pattern(pattern)
        out = DeviceArray(self.length, np.bool_)
        optr, oisz, bptr = self._args()
        _lib.call("vh_str_match", optr, oisz, bptr, self.length, MATCH_OPS[op], pat, len(pat), out.ptr)
        return out


def _pattern(pattern):
    if not isinstance(pattern, str):
        raise TypeError("a string pattern is a str")
    pat = pattern.encode("utf-8", "surrogatepass")
    if len(pat) > MAX_PATTERN:
        raise NotImplementedError(f"a pattern of {len(pat)} bytes: the device kernel takes at most {MAX_PATTERN}")
    return pat


class ordered_set_string:
    """``superutils.ordered_set_string`` on the GPU: the distinct strings of the columns it was
    updated with, numbered in first-appearance order, held in a dictionary of its own in HBM.
    ``hash_bits`` < 64 keeps only the low bits of the hash (a test seam: collisions are then
    resolved by the exact rounds); ``initial_capacity``: slots of a fresh table."""

    def __init__(self, hash_bits=64, initial_capacity=0):
        h = ctypes.c_void_p()
        _lib.call("vh_strset_create", int(hash_bits), int(initial_capacity), ctypes.byref(h))
        self._handle = h.value
        self._keys = None

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            try:
                _lib.call("vh_strset_destroy", h)
            except Exception:
                pass
            self._handle = None

    def _info(self):
        vals = [ctypes.c_int64() for _ in range(4)]
        _lib.call("vh_strset_info", self._handle, *[ctypes.byref(v) for v in vals])
        return [v.value for v in vals]

    def __len__(self):
        return self._info()[0]

    def __sizeof__(self):
        count, dict_bytes, _, table_bytes = self._info()
        return table_bytes + dict_bytes + 8 * (count + 1)

    @property
    def levels(self):
        return self._info()[2]

    def update(self, ar):
        if not isinstance(ar, DeviceStringArray):
            raise TypeError("ordered_set_string.update takes a DeviceStringArray")
        optr, oisz, bptr = ar._args()
        _lib.call("vh_strset_update", self._handle, optr, oisz, bptr, len(ar))
        self._keys = None

    def map_ordinal(self, ar):
        """int32 DeviceArray of the ordinals, -1 for a string that is not in the set."""
        if not isinstance(ar, DeviceStringArray):
            raise TypeError("ordered_set_string.map_ordinal takes a DeviceStringArray")
        out = DeviceArray(len(ar), np.int32)
        optr, oisz, bptr = ar._args()
        _lib.call("vh_strset_map_ordinal", self._handle, optr, oisz, bptr, len(ar), out.ptr)
        return out

    def key_array(self):
        """The dictionary as an object array of ``str``, in ordinal order."""
        if self._keys is None:
            count, dict_bytes = self._info()[:2]
            offsets = np.zeros(count + 1, np.int64)
            data = np.zeros(max(dict_bytes, 1), np.uint8)
            _lib.call("vh_strset_dict", self._handle, offsets.ctypes.data, data.ctypes.data)
            raw = data.tobytes()
            o = offsets.tolist()
            keys = np.empty(count, dtype=object)
            keys[:] = [raw[o[i]:o[i + 1]].decode("utf-8", "surrogatepass") for i in range(count)]
            self._keys = keys
        return self._keys

    def keys(self):
        return self.key_array().tolist()


def bytewise_order(keys):
    """The ascending order of ``str`` keys: Python's ``str`` order is the order of the code
    points, which is the bytewise order of their UTF-8."""
    return sorted(range(len(keys)), key=keys.__getitem__)


def encode(column):
    """(codes, set): the int32 first-appearance codes of a DeviceStringArray and its set."""
    s = ordered_set_string()
    s.update(column)
    return s.map_ordinal(column), s


def rank_codes(codes, keys):
    """Codes remapped to the rank of their string in ascending order (``vh_take`` over the
    rank table); the dictionary's distinct strings are ordered on the host."""
    from .superutils import take_device
    order = bytewise_order(keys)
    rank = np.empty(len(keys), np.int32)
    rank[order] = np.arange(len(keys), dtype=np.int32)
    if not len(keys):
        return codes, order
    return take_device([DeviceArray.from_numpy(rank)], codes)[0], order
