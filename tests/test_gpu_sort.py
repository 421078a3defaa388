"""The device argsort (``superutils.argsort_device``), the kept-row list (``mask_rows``) and
``DataFrame.sort`` / ``extract`` on host, HBM and mixed frames, against NumPy
(``np.lexsort`` / ``np.argsort(kind="stable")`` / ``np.flatnonzero`` through tests/sort_np.py)
and the hand-worked frames of tests/sort_cases.py.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import sort_np as sn
from sort_cases import (EXTRACT_CASES, FRAME, SORT_CASES, TAKE_FILTER, TAKE_INDICES, TAKE_KEPT, TAKE_VISIBLE, as_list, keep_mask,
                        rows_of)

pytestmark = pytest.mark.gpu

TILE = 1024  # superutils.SORT_ENCODE_TILE: the output positions one encode workgroup takes per step
# one lane, one wave, one workgroup, one encode tile and several workgroups, and their edges
ROW_COUNTS = [0, 1, 2, 255, 256, 257, TILE - 1, TILE, TILE + 1, 70_001]
DTYPES = ["float64", "float32", "int64", "int32", "int16", "int8", "uint64", "uint32", "uint16", "uint8", "bool"]


@functools.lru_cache(maxsize=None)
def key(name, n):
    """A key column of n rows (read-only): the eleven dtypes with their extremes present, floats
    with NaN in a seventh of the rows, +-inf, +-0.0 and denormals; and the special keys."""
    rng = np.random.default_rng(sum(map(ord, name)) * 100_003 + n)
    if name == "u8x3":  # three values: stability decides nearly every position
        v = rng.integers(0, 3, n).astype(np.uint8)
    elif name == "const":
        v = np.full(n, -5, np.int32)
    elif name == "allnan":
        v = np.full(n, np.nan, np.float64)
    elif name == "bool":
        v = rng.random(n) < 0.5
    elif name.rstrip("b") in ("float64", "float32"):
        dt = np.dtype(name.rstrip("b"))
        fi = np.finfo(dt)
        v = rng.normal(size=n).astype(dt)
        special = np.array([np.inf, -np.inf, 0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny / 2,
                            -fi.tiny / 2, fi.max, fi.min], dtype=dt)
        where = rng.integers(0, max(n, 1), n // 3)
        v[where] = special[rng.integers(0, len(special), len(where))]
        v[::7] = np.nan
    else:  # "int32b": a second, independent column of the dtype
        dt = np.dtype(name.rstrip("b"))
        ii = np.iinfo(dt)
        v = rng.integers(ii.min, ii.max, n, dtype=dt, endpoint=True)
        if n >= 2:
            v[n // 3], v[n // 2] = ii.min, ii.max
    v.setflags(write=False)
    return v


KEY_LISTS = {
    "32 bits": ["int16", "uint16"],
    "33 bits": ["int32", "bool"],
    "64 bits": ["int32", "int32b"],
    "65 bits": ["int32", "int32b", "bool"],
    "int64-u8": ["int64", "uint8"],
    "u8-int64": ["uint8", "int64"],
    "four keys": ["u8x3", "bool", "float32", "float64"],
    "const-allnan-f64": ["const", "allnan", "float64"],
    "stability": ["u8x3"],
    "const": ["const"],
    "allnan": ["allnan"],
}


def row_lists(n):
    """None (every row), every second row, no row, one row."""
    return [None, np.arange(0, n, 2), np.arange(0), np.arange(n)[n // 2:n // 2 + 1]]


def check_argsort(names, n):
    from vaex_amd.device import DeviceArray
    from vaex_amd.superutils import argsort_device
    host = [key(k, n) for k in names]
    dev = [DeviceArray.from_numpy(k) for k in host]
    rdt = np.int32  # n < 2^31
    for rows in row_lists(n):
        drows = None if rows is None else DeviceArray.from_numpy(rows.astype(rdt))
        for ascending in (True, False):
            got = argsort_device(dev, rows=drows, ascending=ascending)
            assert got.dtype == rdt and len(got) == (n if rows is None else len(rows))
            want = sn.reference_order(host, rows, ascending)
            assert np.array_equal(got.to_numpy(), want), (names, n, None if rows is None else len(rows), ascending)


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_argsort_every_dtype(n):
    for dt in DTYPES:
        check_argsort([dt], n)


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_argsort_key_lists(n):
    for names in KEY_LISTS.values():
        check_argsort(names, n)


def test_the_key_lists_reach_the_rounds_they_are_named_for():
    n = 70_001
    bits = {name: [r[2] for r in sn.plan([sn.key_range(key(k, n)) for k in names], n)[1]] for name, names in KEY_LISTS.items()}
    assert bits["32 bits"] == [32] and bits["33 bits"] == [33] and bits["64 bits"] == [64] and bits["65 bits"] == [33, 32]
    assert bits["int64-u8"] == [8, 64] and bits["u8-int64"] == [64, 8]
    assert bits["const"] == [0] and bits["allnan"] == [0] and bits["stability"] == [2]


def test_argsort_refuses_rows_out_of_range_and_bad_arguments():
    from vaex_amd import _lib
    from vaex_amd.device import DeviceArray
    from vaex_amd.superutils import SORT_MAX_KEYS, argsort_device
    k = DeviceArray.from_numpy(key("int32", 257))
    for bad in ([0, 5, 257], [-1, 3]):
        with pytest.raises(_lib.HipError, match="outside"):
            argsort_device([k], rows=DeviceArray.from_numpy(np.array(bad, np.int32)))
    with pytest.raises(TypeError):
        argsort_device([k], rows=DeviceArray.from_numpy(np.array([0], np.int64)))  # int32 while n < 2^31
    with pytest.raises(TypeError):
        argsort_device([key("int32", 257)])
    with pytest.raises(ValueError):
        argsort_device([k] * (SORT_MAX_KEYS + 1))
    with pytest.raises(ValueError):
        argsort_device([k, DeviceArray.from_numpy(key("int32", 256))])
    assert len(argsort_device([k] * SORT_MAX_KEYS)) == 257


@pytest.mark.parametrize("n", [0, 1, 257, TILE + 1, 70_001])
def test_int64_row_numbers_through_the_c_abi(n):
    """The wrappers choose int32 row numbers below 2^31 rows; frames past that get the int64
    forms of the same kernels, which the C ABI also takes at any size: 8-byte ``rows``,
    ``perm_out`` and ``vh_mask_rows`` output."""
    import ctypes

    from vaex_amd import _lib
    from vaex_amd.device import DeviceArray
    names = ["int32", "bool", "float64"]  # two rounds: float64 alone (64 bits), then int32 + bool (33)
    host = [key(k, n) for k in names]
    dev = [DeviceArray.from_numpy(k) for k in host]
    kptr = (ctypes.c_void_p * 3)(*[c.ptr for c in dev])
    codes = (ctypes.c_int * 3)(*[_lib.dtype_code(c.dtype)[0] for c in dev])
    mask = np.random.default_rng(n).random(n) < 0.6
    rows = DeviceArray(n, np.int64)
    m = ctypes.c_uint64(0)
    _lib.call("vh_mask_rows", DeviceArray.from_numpy(mask).ptr, n, 8, rows.ptr, ctypes.byref(m))
    rows = rows[:m.value]
    assert np.array_equal(rows.to_numpy(), np.flatnonzero(mask))
    for r in (None, rows):
        for descending in (0, 1):
            out = DeviceArray(n if r is None else len(r), np.int64)
            _lib.call("vh_argsort", 3, kptr, codes, n, None if r is None else r.ptr, 8, len(out), descending, out.ptr)
            want = sn.reference_order(host, None if r is None else np.flatnonzero(mask), not descending)
            assert np.array_equal(out.to_numpy(), want)
    # 4-byte row numbers are refused from 2^31 rows (nothing is read: the check comes first)
    with pytest.raises(_lib.HipError, match="8-byte"):
        _lib.call("vh_argsort", 3, kptr, codes, 2 ** 31, None, 4, 2 ** 31, 0, rows.ptr)
    with pytest.raises(_lib.HipError, match="8-byte"):
        _lib.call("vh_mask_rows", rows.ptr, 2 ** 31, 4, rows.ptr, ctypes.byref(m))


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_mask_rows(n):
    from vaex_amd.device import DeviceArray
    from vaex_amd.superutils import mask_rows
    rng = np.random.default_rng(n)
    last = np.zeros(n, np.uint8)
    last[-1:] = 1
    masks = [np.ones(n, np.uint8), np.zeros(n, np.uint8), last, (rng.random(n) < 0.3).astype(np.uint8),
             (rng.integers(0, 256, n) * (rng.random(n) < 0.5)).astype(np.uint8),  # any non-zero byte keeps its row
             rng.random(n) < 0.9]
    for m in masks:
        got = mask_rows(DeviceArray.from_numpy(m))
        assert got.dtype == np.int32
        assert np.array_equal(got.to_numpy(), np.flatnonzero(m))
    # a host mask is staged; an unaligned device view takes the per-row path
    assert np.array_equal(mask_rows(masks[3]).to_numpy(), np.flatnonzero(masks[3]))
    if n > 3:
        assert np.array_equal(mask_rows(DeviceArray.from_numpy(masks[3])[3:]).to_numpy(), np.flatnonzero(masks[3][3:]))


# ---- frames -------------------------------------------------------------------------------------
FLAVOURS = ["host", "hbm", "mixed"]


def frame(columns, flavour, flt=None):
    """host: every column on the host; hbm: the unmasked columns in HBM and no other; mixed: the
    unmasked columns in HBM, the masked ones (which have no HBM form) on the host."""
    import vaex_amd
    from vaex_amd.device import DeviceArray
    cols = {}
    for k, v in columns.items():
        if np.ma.isMaskedArray(v):
            if flavour != "hbm":
                cols[k] = v
        else:
            cols[k] = v if flavour == "host" else DeviceArray.from_numpy(np.ascontiguousarray(v))
    df = vaex_amd.from_arrays(**cols)
    return df if flt is None else df.filter(flt)


def is_hbm(column):
    from vaex_amd.device import DeviceArray
    return isinstance(column, DeviceArray)


def same_bits(got, want):
    """Two unmasked columns hold the same dtype and the same bytes (NaN and the sign of zero
    included); the large frames use this instead of lists."""
    got = got.to_numpy() if is_hbm(got) else np.asarray(got)
    want = np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def check_rows(res, src, rows):
    """``res`` holds FRAME's rows ``rows``, every column where the source frame has it."""
    want = rows_of(rows)
    assert list(res.columns) == list(src.columns)
    assert res.length_unfiltered() == len(rows)
    for k, c in res.columns.items():
        assert as_list(c) == want[k], k
        assert np.dtype(c.dtype) == FRAME[k].dtype, k
        assert is_hbm(c) == is_hbm(src.columns[k]), k  # HBM columns stay in HBM
        assert np.ma.isMaskedArray(c) == np.ma.isMaskedArray(src.columns[k]), k


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("name, flt, by, ascending, rows", SORT_CASES, ids=[c[0] for c in SORT_CASES])
def test_sort_hand_worked(name, flt, by, ascending, rows, flavour):
    df = frame(FRAME, flavour, flt)
    res = df.sort(by, ascending=ascending)
    check_rows(res, df, rows)
    assert not res.filtered and len(res) == len(rows)
    assert df.filtered == (flt is not None) and df.length_unfiltered() == 8  # the input is untouched
    # kind is accepted, and Expression keys too
    if isinstance(by, str) and by in FRAME:
        check_rows(df.sort(df[by], ascending=ascending, kind="mergesort"), df, rows)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_sort_carries_virtual_columns_variables_categories_and_selections(flavour):
    df = frame(FRAME, flavour)
    df.add_virtual_column("p2", "p * k")
    df.add_variable("k", 2)
    df.categorize("g", labels=["no", "yes"], inplace=True)
    df.select("p > 13")
    res = df.filter("p != 15").sort(["g", "x"], ascending=False)
    rows = [r for r in [6, 0, 2, 4, 1, 7, 5, 3] if r != 5]
    check_rows(res, df, rows)
    assert res.virtual_columns == {"p2": "p * k"} and res.variables["k"] == 2
    assert res.is_category("g") and res.category_labels("g") == ["no", "yes"]
    assert not res.filtered and res.has_selection()
    assert as_list(res.evaluate("p2")) == [2 * FRAME["p"][r] for r in rows]
    assert int(res.count(selection=True)) == sum(FRAME["p"][r] > 13 for r in rows)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("flt, rows", EXTRACT_CASES, ids=[str(c[0]) for c in EXTRACT_CASES])
def test_extract_hand_worked(flt, rows, flavour):
    df = frame(FRAME, flavour, flt)
    df.add_virtual_column("p2", "p + 1")
    res = df.extract()
    check_rows(res, df, rows)
    assert not res.filtered and len(res) == len(rows) and res.virtual_columns == {"p2": "p + 1"}
    assert res is not df and df.filtered == (flt is not None)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_take_from_the_kept_rows_goes_through_extract(flavour):
    """``take`` keeps its contract (on a filtered frame only unfiltered row numbers with the
    filter kept); indices that address the kept rows are taken from ``extract()``."""
    from vaex_amd.device import DeviceArray
    df = frame(FRAME, flavour, TAKE_FILTER)
    for indices in (TAKE_INDICES, np.array(TAKE_INDICES, np.int32), DeviceArray.from_numpy(np.array(TAKE_INDICES, np.int64))):
        res = df.extract().take(indices)
        check_rows(res, df, TAKE_KEPT)
        assert not res.filtered
        res = df.take(indices, filtered=False, dropfilter=False)
        check_rows(res, df, TAKE_INDICES)
        assert res.filtered and as_list(res.evaluate("p")) == [int(FRAME["p"][TAKE_INDICES[i]]) for i in TAKE_VISIBLE]
    with pytest.raises(IndexError):
        df.extract().take(np.array([0, 4]))  # four kept rows


def random_frame(n, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=n)
    x[::11] = np.nan
    return dict(a=rng.integers(0, 40, n).astype(np.int32), x=x, b=rng.integers(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32),
                w=rng.integers(0, 100, n).astype(np.int8), v=rng.normal(size=n).astype(np.float32))


@pytest.mark.parametrize("flavour", ["host", "hbm"])
def test_sort_equals_take_of_argsort_on_a_larger_frame(flavour):
    """Several workgroups, one and two rounds, both directions, filtered and not; and
    ``sort(by)`` is ``take(argsort)``."""
    from vaex_amd import sort as vsort
    n = 70_001
    cols = random_frame(n)
    keep = cols["w"] < 60
    for flt, by, ascending in ((None, "x", True), (None, ["a", "x"], False), ("w < 60", ["a", "b"], True),
                               ("w < 60", ["b", "a", "x"], False), ("w < 60", "x", False)):
        df = frame(cols, flavour, flt)
        res = df.sort(by, ascending=ascending)
        want = sn.sort_frame_np(cols, by, None if flt is None else keep, ascending)
        assert not res.filtered and list(res.columns) == list(cols)
        for k in cols:
            assert is_hbm(res.columns[k]) == (flavour == "hbm")
            assert same_bits(res.columns[k], want[k]), (k, flt, by)
        order = vsort.argsort(df, by, ascending)
        assert is_hbm(order) == (flavour == "hbm")
        again = frame(cols, flavour).take(order)  # the order holds unfiltered row numbers
        for k in cols:
            assert same_bits(again.columns[k], want[k]), (k, flt, by)
    # extract, and take through the kept rows, at this size
    df = frame(cols, flavour, "w < 60")
    ex = df.extract()
    idx = np.random.default_rng(4).integers(0, int(keep.sum()), 5000)
    tk = ex.take(idx)
    for k in cols:
        assert same_bits(ex.columns[k], cols[k][keep]), k
        assert same_bits(tk.columns[k], cols[k][np.flatnonzero(keep)[idx]]), k
    # evaluate on the filtered frame gives the kept rows, on the host, as before
    got = df.evaluate("x")
    assert isinstance(got, np.ndarray) and same_bits(got, cols["x"][keep])


@pytest.mark.parametrize("flavour", ["host", "hbm"])
def test_datetime_keys_sort_as_int64(flavour):
    t = np.array(["2020-01-03", "1960-05-01", "2020-01-03", "1999-12-31", "1960-05-01"], dtype="datetime64[ns]")
    cols = dict(t=t, i=np.arange(5, dtype=np.int16))
    res = frame(cols, flavour).sort("t")
    assert as_list(res.columns["i"]) == [1, 4, 3, 0, 2]
    assert as_list(frame(cols, flavour).sort(["t", "i"], ascending=False).columns["i"]) == [2, 0, 3, 4, 1]
