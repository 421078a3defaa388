"""HBM-resident columns.

A :class:`DeviceArray` is a 1-d column living in the MI355X's HBM (allocated by
``libvaexhip``).  DataFrames built from DeviceArrays are binned in place: the
executor hands the device pointers straight to ``vh_grid_bin`` (no host staging),
which is how the 1e9-row benchmark columns stay resident.
"""
import ctypes

import numpy as np

from . import _lib


class DeviceArray:
    def __init__(self, length, dtype, _ptr=None, _owner=None):
        self.dtype = np.dtype(dtype)
        self.length = int(length)
        self._owner = _owner
        if _ptr is None:
            p = ctypes.c_void_p()
            _lib.call("vh_malloc", ctypes.byref(p), max(1, self.nbytes))
            self.ptr = p.value
            self._owns = True
        else:
            self.ptr = _ptr
            self._owns = False

    # ---- construction -------------------------------------------------------
    @classmethod
    def empty(cls, length, dtype):
        return cls(length, dtype)

    @classmethod
    def from_numpy(cls, ar):
        ar = np.ascontiguousarray(ar)
        if ar.ndim != 1:
            raise ValueError("Expected a 1d array")
        d = cls(len(ar), ar.dtype)
        if d.nbytes:
            _lib.call("vh_memcpy_htod", d.ptr, ar.ctypes.data, d.nbytes)
        return d

    @classmethod
    def random(cls, length, dist="normal", seed=0, a=0.0, b=1.0, dtype="float64"):
        """Synthetic column generated in HBM: dist 'uniform' [a, b), 'normal' (mean a, sd b),
        'randint' [a, b) (int32/int64), or the sorted layouts 'sorted_normal' (ascending normal
        quantiles, mean a, sd b) and 'sorted_int' ([a, b) in equal consecutive runs)."""
        d = cls(length, dtype)
        code = {"uniform": 0, "normal": 1, "randint": 2, "sorted_normal": 3, "sorted_int": 4}[dist]
        dcode, _ = _lib.dtype_code(d.dtype)
        _lib.call("vh_fill_random", d.ptr, d.length, dcode, code, seed, float(a), float(b))
        return d

    # ---- views / copies -----------------------------------------------------
    @property
    def nbytes(self):
        return self.length * self.dtype.itemsize

    @property
    def itemsize(self):
        return self.dtype.itemsize

    @property
    def ndim(self):
        return 1

    @property
    def shape(self):
        return (self.length,)

    def __len__(self):
        return self.length

    def __getitem__(self, item):
        if not isinstance(item, slice):
            raise TypeError("DeviceArray only supports contiguous slices")
        start, stop, step = item.indices(self.length)
        if step != 1:
            raise TypeError("DeviceArray only supports contiguous slices")
        stop = max(start, stop)
        return DeviceArray(stop - start, self.dtype, _ptr=self.ptr + start * self.itemsize,
                           _owner=self if self._owner is None else self._owner)

    def to_numpy(self, pinned=False):
        """A host copy; pinned: into page-locked memory from the library's block cache (read
        back by the copy kernel at the link rate; a pageable copy runs at ~17 GB/s)."""
        if pinned:
            from .hostops import _empty
            out = _empty(self.length, self.dtype)
        else:
            out = np.empty(self.length, self.dtype)
        if self.nbytes:
            _lib.call("vh_memcpy_dtoh", out.ctypes.data, self.ptr, self.nbytes)
        return out

    def __array__(self, dtype=None, copy=None):
        a = self.to_numpy()
        return a if dtype is None else a.astype(dtype)

    def __del__(self):
        if getattr(self, "_owns", False) and self.ptr:
            try:
                _lib.call("vh_free", self.ptr)
            except Exception:
                pass
            self.ptr = None

    def __repr__(self):
        return f"DeviceArray(length={self.length}, dtype={self.dtype})"


class DeviceMaskedArray:
    """An HBM column with missing values: ``data`` (a DeviceArray) and ``mask`` (a DeviceArray of
    uint8 or bool, 1 = missing: numpy's convention, the one ``set_data_mask`` takes), of one
    length.  The mask holds 0 and 1 only (what ``from_numpy``, ``from_arrow`` and every expression
    write): the engine counts bytes equal to 1 as set, so any other value is undefined.  The data
    under a missing row is unspecified.  Deliberately not a DeviceArray: code
    that has not been taught about masks fails its ``isinstance`` check instead of dropping one."""

    def __init__(self, data, mask):
        if not isinstance(data, DeviceArray) or not isinstance(mask, DeviceArray):
            raise TypeError("DeviceMaskedArray(data, mask) takes two DeviceArrays")
        if mask.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)):
            raise TypeError(f"the mask is uint8 or bool, not {mask.dtype}")
        if len(mask) != len(data):
            raise ValueError(f"data holds {len(data)} rows, the mask {len(mask)}")
        self.data = data
        self.mask = mask

    # ---- construction -------------------------------------------------------
    @classmethod
    def from_numpy(cls, ar):
        """A numpy (masked) array; ``np.ma.nomask`` and a plain array give an all-zero mask."""
        mask = np.ma.getmaskarray(ar) if np.ma.isMaskedArray(ar) else np.zeros(len(ar), bool)
        return cls(DeviceArray.from_numpy(np.ma.getdata(ar)), DeviceArray.from_numpy(mask.view(np.uint8)))

    @classmethod
    def from_arrow(cls, ar):
        """A primitive numeric / bool ``pyarrow.Array`` with or without nulls.  The values buffer
        and the validity bitmap are uploaded as they are (the bitmap: n / 8 bytes) and the byte
        mask is expanded on the device (``vh_mask_unpack_bits``); the array's offset is honoured."""
        import pyarrow as pa
        if isinstance(ar, pa.ChunkedArray):
            ar = ar.combine_chunks()
        t = ar.type
        n, offset = len(ar), ar.offset
        validity, values = ar.buffers()[:2] if len(ar.buffers()) == 2 else (None, None)
        if not (pa.types.is_integer(t) or pa.types.is_floating(t) or pa.types.is_boolean(t)) or values is None:
            raise TypeError(f"from_arrow takes primitive numeric / bool arrays, not {t}")
        if pa.types.is_boolean(t):  # bit-packed values: expanded like the bitmap, then inverted
            packed = np.frombuffer(values, np.uint8)[offset // 8:(offset + n + 7) // 8]
            data = DeviceArray.empty(n, np.bool_)
            if n:
                bits = DeviceArray.from_numpy(packed)
                _lib.call("vh_mask_unpack_bits", bits.ptr, offset % 8, n, data.ptr)
                _lib.call("vh_mask_combine", data.ptr, None, 0, n, data.ptr)
        else:
            dtype = np.dtype(t.to_pandas_dtype())
            if dtype.itemsize not in (1, 2, 4, 8) or dtype.kind not in "iuf" or dtype == np.float16:
                raise TypeError(f"from_arrow: {t}")
            data = DeviceArray.from_numpy(np.frombuffer(values, dtype)[offset:offset + n])
        mask = DeviceArray.empty(n, np.uint8)
        if validity is None or ar.null_count == 0:
            if n:
                _lib.call("vh_memset", mask.ptr, 0, n)
        else:
            bits = DeviceArray.from_numpy(np.frombuffer(validity, np.uint8)[offset // 8:(offset + n + 7) // 8])
            _lib.call("vh_mask_unpack_bits", bits.ptr, offset % 8, n, mask.ptr)
        _lib.synchronize()  # the uploaded bitmaps are freed on return
        return cls(data, mask)

    # ---- views / copies -----------------------------------------------------
    @property
    def dtype(self):
        return self.data.dtype

    @property
    def length(self):
        return self.data.length

    @property
    def nbytes(self):
        return self.data.nbytes + self.mask.nbytes

    @property
    def ndim(self):
        return 1

    @property
    def shape(self):
        return (self.data.length,)

    def __len__(self):
        return self.data.length

    def __getitem__(self, item):
        return DeviceMaskedArray(self.data[item], self.mask[item])

    @property
    def null_count(self):
        """the number of missing rows (a device reduction over the mask)"""
        count = ctypes.c_uint64()
        _lib.call("vh_mask_count", self.mask.ptr, len(self), ctypes.byref(count))
        return count.value

    def to_numpy(self, pinned=False):
        return np.ma.array(self.data.to_numpy(pinned=pinned), mask=self.mask.to_numpy().astype(bool), shrink=False)

    def to_arrow(self):
        """A ``pyarrow.Array`` of the column; the validity bitmap is packed on the device
        (``vh_mask_pack_bits``) and read back as n / 8 bytes."""
        import pyarrow as pa
        n = len(self)
        bits = DeviceArray.empty((n + 7) // 8, np.uint8)
        if n:
            _lib.call("vh_mask_pack_bits", self.mask.ptr, n, bits.ptr)
        validity = pa.py_buffer(bits.to_numpy().tobytes())
        data = self.data.to_numpy()
        if self.dtype.kind == "b":
            return pa.Array.from_buffers(pa.bool_(), n, [validity, pa.py_buffer(np.packbits(data, bitorder="little").tobytes())])
        return pa.Array.from_buffers(pa.from_numpy_dtype(self.dtype), n, [validity, pa.py_buffer(data.tobytes())])

    def __array__(self, dtype=None, copy=None):
        raise TypeError("a DeviceMaskedArray does not convert to a plain array (its mask would be dropped): to_numpy()")

    def __repr__(self):
        return f"DeviceMaskedArray(length={len(self)}, dtype={self.dtype})"


def is_masked_column(col):
    """a host ``np.ma`` column or a masked HBM column: the routes that take neither ask this"""
    return np.ma.isMaskedArray(col) or isinstance(col, DeviceMaskedArray)


def is_device_array(x):
    return isinstance(x, DeviceArray)
