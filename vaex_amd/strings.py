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
# the string-producing functions (functions.py ``str_*``) -> the DeviceStringArray method that
# computes them; each takes the reference's arguments after the column
TRANSFORMS = {"str_lower": "lower", "str_upper": "upper", "str_slice": "slice", "str_strip": "strip",
              "str_lstrip": "lstrip", "str_rstrip": "rstrip", "str_pad": "pad", "str_ljust": "ljust",
              "str_rjust": "rjust", "str_center": "center", "str_zfill": "zfill", "str_repeat": "repeat",
              "str_cat": "cat", "str_replace": "replace"}
TRANSFORM_OPS = {"lower": 0, "upper": 1, "slice": 2, "strip": 3, "pad": 4, "repeat": 5, "cat": 6, "replace": 7}  # str_dev.hpp
SIDES = {"left": 1, "right": 2, "both": 3}
WHITESPACE = " \t\n\v\f\r"   # C isspace: what strip() without an argument strips (string_utils.hpp:265-306)
TOO_LONG = 2 ** 64 - 1          # vh_str_fn_plan's total when the result cannot fit (VH_STR_FN_TOO_LONG)
MAX_CASE_TABLE = 2048          # pairs of a case table (strfn.hip stages it in LDS)


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


# ---- the case tables ------------------------------------------------------------------------------
def case_mapping(upper):
    """{code point: image} over the code points >= 128 that lower (``upper`` False) or upper
    changes, one code point to one code point: ``pyarrow.compute.utf8_lower`` / ``utf8_upper``,
    which is what the reference calls (functions.py:1528-1558, 2102-2138).  Without pyarrow:
    Python's ``str.lower`` / ``str.upper`` where the result is one code point, the identity
    elsewhere.  ASCII is mapped inline by the kernel."""
    cps = np.concatenate([np.arange(0x80, 0xD800, dtype=np.uint32), np.arange(0xE000, 0x110000, dtype=np.uint32)])
    try:
        import pyarrow as pa
        import pyarrow.compute as pc
    except ImportError:
        out = {}
        for cp in cps.tolist():
            t = chr(cp).upper() if upper else chr(cp).lower()
            if len(t) == 1 and ord(t) != cp:
                out[cp] = ord(t)
        return out
    ar = pa.array(cps.view("<U1"), type=pa.string())
    images = (pc.utf8_upper if upper else pc.utf8_lower)(ar)
    changed = pc.and_(pc.equal(pc.utf8_length(images), 1), pc.not_equal(images, ar)).to_numpy(zero_copy_only=False)
    rows = np.flatnonzero(changed)
    return {int(cps[i]): ord(t) for i, t in zip(rows.tolist(), images.take(pa.array(rows)).to_pylist())}


def pack_case_table(mapping):
    """The kernel's layout of a mapping: a uint32 array of (code point, image) pairs sorted by
    code point (a binary search in LDS, str_dev.hpp ``case_image``)."""
    if any(k < 0x80 for k in mapping):
        raise ValueError("a case table holds code points from 128 on")
    if len(mapping) > MAX_CASE_TABLE:
        raise NotImplementedError(f"a case table of {len(mapping)} pairs: the device kernel takes at most {MAX_CASE_TABLE}")
    out = np.empty((len(mapping), 2), np.uint32)
    for i, k in enumerate(sorted(mapping)):
        out[i] = k, mapping[k]
    return out.reshape(-1)


def unpack_case_table(table):
    pairs = np.asarray(table, np.uint32).reshape(-1, 2)
    return {int(k): int(v) for k, v in pairs}


_case_tables = {}


def case_table(upper):
    """The packed table of :func:`case_mapping`, built once per process."""
    t = _case_tables.get(bool(upper))
    if t is None:
        t = _case_tables[bool(upper)] = pack_case_table(case_mapping(upper))
    return t


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

    # ---- transforms: a new column each (csrc/strfn.hip) ---------------------------
    def _transform(self, op, a=0, b=0, flags=0, c0=b"", c1=b"", table=None, other=None):
        """The plan (every row's result length, scanned into positions on the device) and the
        write, with the output sized in between, like :meth:`take`."""
        n = self.length
        pos = DeviceArray(n + 1, np.uint64)
        total = ctypes.c_uint64(0)
        second = other._args() if other is not None else (None, 0, None)
        tptr, nt = (table.ctypes.data, len(table) // 2) if table is not None and len(table) else (None, 0)
        optr, oisz, bptr = self._args()
        args = (optr, oisz, bptr, n) + second + (TRANSFORM_OPS[op], int(a), int(b), int(flags), c0, len(c0), c1, len(c1),
                                                 tptr, nt)
        _lib.call("vh_str_fn_plan", *args, pos.ptr, ctypes.byref(total))
        if total.value == TOO_LONG:
            # repeats and widths are any int64: the device found a row, or the sum, past what
            # offsets can address, and nothing is allocated or written
            raise MemoryError(f"str {op}: the result's bytes do not fit (a row past 2^62 / rows)")
        widths = [self.offsets.dtype] + ([other.offsets.dtype] if other is not None else [])
        odt = take_offset_dtype(max(widths, key=lambda dt: np.dtype(dt).itemsize), total.value)
        out_off = DeviceArray(n + 1, odt)
        try:
            full = DeviceArray(total.value + SLACK, np.uint8)
        except _lib.HipError as e:
            raise MemoryError(f"str {op}: a result of {total.value} bytes: {e}") from None
        _lib.call("vh_str_fn", *args, pos.ptr, total.value, out_off.ptr, odt.itemsize, full.ptr)
        return DeviceStringArray(out_off, full, _checked=True, _root=(full, total.value))

    def lower(self):
        """``str_lower``: one code point to one code point (``pyarrow.compute.utf8_lower``)."""
        return self._transform(**transform_arguments("lower"))

    def upper(self, ascii=False):
        """``str_upper``; ``ascii=True`` maps only a-z."""
        return self._transform(**transform_arguments("upper", ascii))

    def slice(self, start=0, stop=None):
        """``str_slice``: ``s[start:stop]`` counted in code points, negative bounds as Python's."""
        return self._transform(**transform_arguments("slice", start, stop))

    def strip(self, to_strip=None):
        """``str_strip``: without an argument the six bytes of C ``isspace`` (not Unicode white
        space); with one, a set of ASCII characters; ``''`` strips nothing."""
        return self._transform(**transform_arguments("strip", to_strip))

    def lstrip(self, to_strip=None):
        return self._transform(**transform_arguments("lstrip", to_strip))

    def rstrip(self, to_strip=None):
        return self._transform(**transform_arguments("rstrip", to_strip))

    def pad(self, width, side="left", fillchar=" "):
        """``str_pad``: to ``width`` code points with one ASCII ``fillchar`` on ``side`` ('left',
        'right', 'both': CPython's ``center`` split)."""
        return self._transform(**transform_arguments("pad", width, side, fillchar))

    def ljust(self, width, fillchar=" "):
        return self._transform(**transform_arguments("ljust", width, fillchar))

    def rjust(self, width, fillchar=" "):
        return self._transform(**transform_arguments("rjust", width, fillchar))

    def center(self, width, fillchar=" "):
        return self._transform(**transform_arguments("center", width, fillchar))

    def zfill(self, width):
        """``str_zfill``: left padding with '0' and nothing more ('-5' at 4 is '00-5')."""
        return self._transform(**transform_arguments("zfill", width))

    def repeat(self, repeats):
        """``str_repeat``; ``repeats <= 0`` gives empty strings."""
        return self._transform(**transform_arguments("repeat", repeats))

    def cat(self, other, first=False):
        """``str_cat``: ``self + other`` for a str constant or a second column of the same
        length; ``first=True`` puts a constant before the rows (``'lit' + s``)."""
        kw = transform_arguments("cat", other, first)
        if kw.get("other") is not None:
            if other.length != self.length:
                raise ValueError(f"cat of columns of {self.length} and {other.length} rows")
            if first:
                return other.cat(self)
        return self._transform(**kw)

    def replace(self, pat, repl, n=-1, flags=0, regex=False):
        """``str_replace``: literal, leftmost, non-overlapping; ``n < 0``: every occurrence."""
        return self._transform(**transform_arguments("replace", pat, repl, n, flags, regex))


def _pattern(pattern):
    if not isinstance(pattern, str):
        raise TypeError("a string pattern is a str")
    pat = pattern.encode("utf-8", "surrogatepass")
    if len(pat) > MAX_PATTERN:
        raise NotImplementedError(f"a pattern of {len(pat)} bytes: the device kernel takes at most {MAX_PATTERN}")
    return pat


# ---- the transforms' arguments ---------------------------------------------------------------------
# One checker per method of TRANSFORMS, with the method's signature after the column: it raises
# what the method refuses and returns the keywords of DeviceStringArray._transform.  The methods
# call them, and so does expr.py when it compiles a transform call (with COLUMN where an argument
# is another string expression), so an expression is refused when it is made, with the method's
# own error.
COLUMN = object()


def _pad_arguments(width, side="left", fillchar=" "):
    if side not in SIDES:
        raise ValueError(f"side is 'left', 'right' or 'both', not {side!r}")
    return dict(op="pad", a=_int(width, "width"), flags=SIDES[side], c0=_fillchar(fillchar))


def _strip_arguments(side, to_strip=None):
    return dict(op="strip", flags=SIDES[side], c0=_strip_set(to_strip))


def _slice_arguments(start=0, stop=None):
    start = 0 if start is None else _int(start, "start")
    if stop is None:
        return dict(op="slice", a=start)
    return dict(op="slice", a=start, b=_int(stop, "stop"), flags=1)


def _cat_arguments(other, first=False):
    if other is COLUMN or isinstance(other, DeviceStringArray):
        return dict(op="cat", flags=2, other=other)
    return dict(op="cat", flags=1 if first else 0, c0=_pattern(other))


def _replace_arguments(pat, repl, n=-1, flags=0, regex=False):
    if regex or flags:
        raise NotImplementedError("str_replace: regular expressions are not supported (regex=False, flags=0)")
    pat, repl = _pattern(pat), _pattern(repl)
    if not pat:
        raise ValueError("str_replace: the pattern is not empty")
    return dict(op="replace", a=_int(n, "n"), c0=pat, c1=repl)


_ARGUMENTS = {
    "lower": lambda: dict(op="lower", table=case_table(False)),
    "upper": lambda ascii=False: dict(op="upper", flags=1) if ascii else dict(op="upper", table=case_table(True)),
    "slice": _slice_arguments,
    "strip": lambda to_strip=None: _strip_arguments("both", to_strip),
    "lstrip": lambda to_strip=None: _strip_arguments("left", to_strip),
    "rstrip": lambda to_strip=None: _strip_arguments("right", to_strip),
    "pad": _pad_arguments,
    "ljust": lambda width, fillchar=" ": _pad_arguments(width, "right", fillchar),
    "rjust": lambda width, fillchar=" ": _pad_arguments(width, "left", fillchar),
    "center": lambda width, fillchar=" ": _pad_arguments(width, "both", fillchar),
    "zfill": lambda width: _pad_arguments(width, "left", "0"),
    "repeat": lambda repeats: dict(op="repeat", a=_int(repeats, "repeats")),
    "cat": _cat_arguments,
    "replace": _replace_arguments,
}


def transform_arguments(method, *args, **kwargs):
    """The ``_transform`` keywords of ``column.method(*args, **kwargs)``, the arguments checked."""
    return _ARGUMENTS[method](*args, **kwargs)


def _int(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"{what} is an integer, not {value!r}")
    if not -(1 << 63) <= int(value) < (1 << 63):
        raise ValueError(f"{what} out of the int64 range")
    return int(value)


def _strip_set(to_strip):
    """the bytes strip removes: ASCII only (the reference strips bytes, which would cut a code
    point of more than one byte in half)"""
    if to_strip is None:
        to_strip = WHITESPACE
    chars = _pattern(to_strip)
    if any(c >= 0x80 for c in chars):
        raise NotImplementedError("strip: to_strip holds ASCII characters only")
    return chars


def _fillchar(fillchar):
    if not isinstance(fillchar, str):
        raise TypeError("fillchar is a str")
    fill = fillchar.encode("utf-8", "surrogatepass")
    if len(fill) != 1 or fill[0] >= 0x80:
        raise ValueError("fillchar is exactly one ASCII character")
    return fill


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
