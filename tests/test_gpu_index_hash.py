"""The GPU index (``superutils.index_hash_<dtype>``), the device gather (``take_device``) and the
inner join's compaction (``index_matched``) against the NumPy restatement of the reference
(tests/join_np.py).  Every comparison is exact.

Shapes are the smallest at which the kernels can go wrong: a probe lane takes 8 consecutive rows
and a workgroup 2048 (tables staged in LDS, 16-byte tables) or 1 row and 256 (packed tables in
HBM), a gather lane takes 4; ragged and misaligned columns; table sizes either
side of 4096 keys; growth from a 16-slot table; keys that collide in their low 32 bits; the
EMPTY bit patterns; row numbers past 2^31; duplicate lists of very different lengths."""
import numpy as np
import pytest

import join_np as jn

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32", "int64", "int32", "int16", "int8", "uint64", "uint32", "uint16", "uint8", "bool"]


def su():
    import vaex_amd.superutils as m
    return m


def dev(a):
    from vaex_amd.device import DeviceArray
    return DeviceArray.from_numpy(np.ascontiguousarray(a))


def host(a):
    from vaex_amd.device import DeviceArray
    return a.to_numpy() if isinstance(a, DeviceArray) else np.asarray(a)


def index(dtype, **kw):
    return su().index_type_from_dtype(dtype)(**kw)


def check_info(ix, ref):
    assert len(ix) == ref.length and ix.length() == ref.length
    assert ix.has_duplicates == ref.has_duplicates
    assert (ix.nan_count, ix.null_count) == (ref.nan_count, ref.null_count)
    assert (ix.has_nan, ix.has_null) == (ref.nan_count > 0, ref.null_count > 0)
    assert (ix.nan_value, ix.null_value) == (ref.nan_value, ref.null_value)


def check_map(ix, ref, values, mask=None, device=False, out_dtype=np.int64):
    """map_index[_masked] (returned and written into `out`) and map_index_duplicates."""
    exp, exp_unknown = jn.map_index_np(ref, values, mask)
    v = dev(values) if device else values
    m = None if mask is None else (dev(mask.astype(np.uint8)) if device else mask)
    got = ix.map_index(v) if mask is None else ix.map_index_masked(v, m)
    assert host(got).dtype == np.int64 and host(got).tolist() == exp.tolist()
    if device:
        from vaex_amd.device import DeviceArray
        out = DeviceArray(len(values), out_dtype)
    else:
        out = np.full(len(values), 77, out_dtype)
    unknown = ix.map_index(v, out) if mask is None else ix.map_index_masked(v, m, out)
    assert host(out).tolist() == exp.tolist() and unknown == exp_unknown
    el, er = jn.map_index_duplicates_np(ref, values, mask, 11)
    gl, gr = ix.map_index_duplicates(v, 11) if mask is None else ix.map_index_duplicates(v, m, 11)
    assert gl.dtype == np.int64 and gr.dtype == np.int64
    assert gl.tolist() == el.tolist() and gr.tolist() == er.tolist()


def make_pool(dtype, distinct, seed):
    """Up to `distinct` different keys of a dtype (floats: +-0, +-inf among them)."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "b":
        return np.array([False, True])
    if dt.kind == "f":
        return np.unique(np.concatenate([rng.normal(size=distinct - 4) * 1e3, [0.0, -0.0, np.inf, -np.inf]]).astype(dt)
                         .view(f"u{dt.itemsize}")).view(dt)
    info = np.iinfo(dt)
    span = min(distinct, int(info.max) - int(info.min) + 1)
    return np.unique(np.concatenate([np.array([info.min, info.max], dt),
                                     rng.integers(info.min, info.max, span - 2, dtype=dt, endpoint=True)]))


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_dtypes(dtype, device):
    n = 5000
    rng = np.random.default_rng(5)
    pool = rng.permutation(make_pool(dtype, 2000, seed=1))
    half = pool[:max(1, len(pool) // 2)]  # the right side knows half of the keys
    right = half[rng.integers(0, len(half), n)]
    left = pool[rng.integers(0, len(pool), n)]
    if np.dtype(dtype).kind == "f":
        right[rng.random(n) < 0.02] = np.nan
        left[rng.random(n) < 0.02] = np.nan
    rmask, lmask = rng.random(n) < 0.05, rng.random(n) < 0.05
    ix = index(dtype)
    ix.update(dev(right) if device else right, dev(rmask.astype(np.uint8)) if device else rmask)
    ref = jn.index_np(right, rmask)
    check_info(ix, ref)
    check_map(ix, ref, left, lmask, device=device)
    check_map(ix, ref, left, None, device=device, out_dtype=np.int32)


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("keys", [3000, 9000], ids=["lds-8-rows-per-lane", "hbm-1-row-per-lane"])
@pytest.mark.parametrize("n", [0, 1, 7, 255, 256, 257, 2047, 2048, 2049])
def test_probe_sizes(n, keys, device):
    """n around the rows of a lane (8 or 1) and of a workgroup (2048 or 256), for the form that
    probes a table staged in LDS and the form that probes a packed table in HBM."""
    rng = np.random.default_rng(n)
    right = rng.permutation(keys).astype(np.int32)
    left = rng.integers(0, 2 * keys, n).astype(np.int32)
    ix = index("int32")
    ix.update(right)
    ref = jn.index_np(right)
    for out_dtype in (np.int32, np.int64):
        check_map(ix, ref, left, device=device, out_dtype=out_dtype)
    check_map(ix, ref, left, rng.random(n) < 0.3, device=device)


@pytest.mark.parametrize("dtype", ["int32", "int64", "uint8"])
def test_misaligned_slice(dtype):
    """DeviceArray[1:] keys, mask and output: every wide access falls back to per-row."""
    from vaex_amd.device import DeviceArray
    rng = np.random.default_rng(2)
    right = rng.permutation(200).astype(dtype)
    left = rng.integers(0, 256, 4100).astype(dtype)
    mask = rng.random(4100) < 0.2
    ix = index(dtype)
    ix.update(dev(right)[1:], start_index=1)
    ref = jn.index_np(right[1:], start_index=1)
    check_info(ix, ref)
    for out_dtype in (np.int32, np.int64):
        out = DeviceArray(4100, out_dtype)
        unknown = ix.map_index_masked(dev(left)[1:], dev(mask.astype(np.uint8))[1:], out[1:])
        exp, eu = jn.map_index_np(ref, left[1:], mask[1:])
        assert out.to_numpy()[1:].tolist() == exp.tolist() and unknown == eu


@pytest.mark.parametrize("distinct", [1, 4095, 4096, 4097, 16384])
def test_table_sizes(distinct):
    """Distinct keys either side of 4096 (64 KiB of packed slots at half load) and 4x that."""
    assert su().INDEX_LDS_KEYS == 4096  # the sizes above are L - 1, L, L + 1 and 4L
    rng = np.random.default_rng(distinct)
    right = (rng.permutation(distinct) * 7 - 3).astype(np.int32)
    left = (rng.integers(-2, distinct + distinct // 2 + 2, 6000) * 7 - 3).astype(np.int32)
    ix = index("int32")
    ix.update(dev(right))
    ref = jn.index_np(right)
    check_info(ix, ref)
    check_map(ix, ref, left, device=True, out_dtype=np.int32)


def test_growth_from_16_slots():
    n = 100_000
    rng = np.random.default_rng(0)
    keys = rng.permutation(n).astype(np.int64) * 1_000_003
    ix = index("int64", initial_capacity=16)
    ix.update(keys)
    assert len(ix) == n and not ix.has_duplicates
    assert np.array_equal(ix.map_index(keys), np.arange(n))
    out = np.empty(n, np.int32)
    assert ix.map_index(keys + 1, out) is True and (out == -1).all()


@pytest.mark.parametrize("dtype", ["int64", "uint64"])
def test_keys_equal_in_low_32_bits(dtype):
    base = np.arange(300, dtype=np.uint64)
    right = np.concatenate([base | (np.uint64(k) << np.uint64(32)) for k in (0, 1, 2, 0x7fffffff)]).astype(np.uint64).view(dtype)
    left = np.concatenate([right[::-1], (base | (np.uint64(5) << np.uint64(32))).view(dtype)])
    ix = index(dtype)
    ix.update(right)
    ref = jn.index_np(right)
    check_info(ix, ref)
    check_map(ix, ref, left, device=True)


@pytest.mark.parametrize("dtype,value", [("int64", -1), ("uint64", 2 ** 64 - 1), ("int32", -1), ("uint32", 2 ** 32 - 1)])
def test_empty_bit_patterns(dtype, value):
    """Keys whose bits are all ones: the side slot of 8-byte keys, a regular key otherwise."""
    v = np.array([value], dtype)[0]
    right = np.array([3, v, 5, v, 7, v], dtype)
    left = np.array([v, 3, 4, v, 7], dtype)
    ix = index(dtype)
    ix.update(right)
    ref = jn.index_np(right)
    check_info(ix, ref)
    assert ref.has_duplicates and ref.length == 6
    check_map(ix, ref, left)
    check_map(ix, ref, left, device=True, out_dtype=np.int32)
    # and without the all-ones key in the index it is unknown
    ix2 = index(dtype)
    ix2.update(np.array([3, 5], dtype))
    assert ix2.map_index(left).tolist() == [-1, 0, -1, -1, -1]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_nan_payloads_and_signed_zero(dtype):
    u = f"u{np.dtype(dtype).itemsize}"
    quiet = np.array([np.nan], dtype)
    other = (quiet.view(u) | np.array([0x55], u)).view(dtype)  # another payload
    neg = -quiet
    right = np.concatenate([np.array([1.5, -0.0], dtype), quiet, np.array([0.0], dtype), other, np.array([2.5], dtype)])
    left = np.concatenate([neg, np.array([0.0, -0.0, 1.5, 9.0], dtype), other])
    ix = index(dtype)
    ix.update(right)
    ref = jn.index_np(right)
    check_info(ix, ref)
    assert (ref.nan_count, ref.nan_value, ref.has_duplicates) == (2, 4, False)  # NaNs are never duplicates
    check_map(ix, ref, left)
    assert ix.map_index(left).tolist() == [4, 3, 1, 0, -1, 4]
    # no NaN in the index: a NaN key is unmatched
    ix2 = index(dtype)
    ix2.update(np.array([1.5], dtype))
    out = np.empty(len(left), np.int64)
    assert ix2.map_index(left, out) is True and out.tolist() == [-1, -1, -1, 0, -1, -1]


def test_last_nan_and_null_across_updates():
    a = np.array([np.nan, 1.0, np.nan, 2.0])
    b = np.array([3.0, np.nan, 4.0, 5.0])
    ma, mb = np.array([0, 1, 0, 0], bool), np.array([0, 0, 1, 1], bool)
    ix = index("float64")
    ref = jn.IndexNp()
    ix.update(a, ma, start_index=0)
    ref.update(a, ma, start_index=0)
    check_info(ix, ref)
    assert (ref.nan_value, ref.null_value) == (2, 1)
    ix.update(b, mb, start_index=4)
    ref.update(b, mb, start_index=4)
    check_info(ix, ref)
    assert (ref.nan_value, ref.null_value, ref.length) == (5, 7, 4)
    check_map(ix, ref, np.array([np.nan, 2.0, 3.0, 4.0]), np.array([0, 0, 1, 0], bool))


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_two_updates_equal_one(device):
    rng = np.random.default_rng(9)
    keys = rng.integers(0, 3000, 5000).astype(np.int32)
    mask = rng.random(5000) < 0.05
    up = (lambda a: dev(a)) if device else (lambda a: a)
    one, two = index("int32"), index("int32")
    one.update(up(keys), up(mask.astype(np.uint8)))
    two.update(up(keys[:1777]), up(mask[:1777].astype(np.uint8)))
    two.update(up(keys[1777:]), up(mask[1777:].astype(np.uint8)), start_index=1777)
    ref = jn.index_np(keys, mask)
    left = rng.integers(0, 4000, 5000).astype(np.int32)
    for ix in (one, two):
        check_info(ix, ref)
        check_map(ix, ref, left, device=device)


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_select_excludes_rows(device):
    rng = np.random.default_rng(10)
    keys = rng.integers(0, 500, 3000).astype(np.int64)
    mask = rng.random(3000) < 0.1
    select = rng.random(3000) < 0.4
    ix = index("int64")
    if device:
        ix.update(dev(keys), dev(mask.astype(np.uint8)), select=dev(select.astype(np.uint8)))
    else:
        ix.update(keys, mask, select=select)
    ref = jn.index_np(keys, mask, select)
    check_info(ix, ref)
    check_map(ix, ref, np.arange(-5, 520, dtype=np.int64), device=device)
    # nothing selected: an empty index
    ix0 = index("int64")
    ix0.update(keys, select=np.zeros(3000, bool))
    assert len(ix0) == 0 and (ix0.map_index(keys) == -1).all()


def test_duplicates_multiplicities():
    """Keys seen once, twice and 5000 times in one index; the rows of a key ascending."""
    rng = np.random.default_rng(11)
    right = rng.permutation(np.concatenate([np.arange(100), np.arange(50, 100), np.full(4999, 70)])).astype(np.int32)
    left = np.array([70, 3, 60, 70, 1000, 99], np.int32)
    ix = index("int32")
    ix.update(right)
    ref = jn.index_np(right)
    check_info(ix, ref)
    assert len(ref.extras[70]) == 5000
    check_map(ix, ref, left)
    check_map(ix, ref, left, device=True, out_dtype=np.int32)


def test_duplicates_span_updates_and_skip_null_keys():
    a = np.array([1.0, 2.0, np.nan, 1.0, 3.0])
    b = np.array([2.0, 1.0, np.nan, 4.0, 3.0, 3.0])
    mb = np.array([0, 0, 0, 0, 1, 0], bool)
    ix = index("float64")
    ref = jn.IndexNp()
    ix.update(a)
    ref.update(a)
    ix.update(b, mb, start_index=5)
    ref.update(b, mb, start_index=5)
    check_info(ix, ref)
    assert ref.extras == {np.float64(1.0).view("u8"): [3, 6], np.float64(2.0).view("u8"): [5], np.float64(3.0).view("u8"): [10]}
    left = np.array([1.0, np.nan, 3.0, 1.0, 2.0, 7.0])
    check_map(ix, ref, left)
    check_map(ix, ref, left, np.array([0, 0, 0, 1, 0, 0], bool), device=True)  # a masked / NaN left key is skipped


def test_duplicates_many_pairs_and_rows():
    """More than 2^16 pairs, and more left rows with extras than one scan block holds."""
    rng = np.random.default_rng(12)
    right = rng.permutation(np.repeat(np.arange(3000), 4)).astype(np.int64)  # 3 extras per key
    left = rng.integers(0, 4000, 30_000).astype(np.int64)                  # ~22500 rows with extras
    ix = index("int64")
    ix.update(dev(right))
    ref = jn.index_np(right)
    check_info(ix, ref)
    el, er = jn.map_index_duplicates_np(ref, left, None, 5)
    assert len(el) > 2 ** 16
    for v in (left, dev(left)):
        gl, gr = ix.map_index_duplicates(v, 5)
        assert np.array_equal(gl, el) and np.array_equal(gr, er)


def test_row_numbers_past_2_31():
    """start_index puts the rows past 2^31: the 16-byte LUT, and an int32 output is refused."""
    from vaex_amd._lib import HipError
    start = 2 ** 31 + 5
    right = np.array([10, 20, 30, 20, -1], np.int32)
    ix = index("int32")
    ix.update(right, start_index=start)
    ref = jn.index_np(right, start_index=start)
    check_info(ix, ref)
    left = np.array([20, 30, 40, -1, 10], np.int32)
    exp, _ = jn.map_index_np(ref, left)
    assert exp.tolist() == [start + 1, start + 2, -1, start + 4, start]
    assert ix.map_index(left).tolist() == exp.tolist()
    assert host(ix.map_index(dev(left))).tolist() == exp.tolist()
    gl, gr = ix.map_index_duplicates(left, 0)
    assert (gl.tolist(), gr.tolist()) == ([0], [start + 3])
    with pytest.raises(HipError, match="int64"):
        ix.map_index(left, np.empty(5, np.int32))


def test_merge_and_seal():
    from vaex_amd._lib import HipError
    rng = np.random.default_rng(13)
    a, b = rng.integers(0, 400, 1000).astype(np.int16), rng.integers(200, 600, 1000).astype(np.int16)
    mb = rng.random(1000) < 0.1
    x, y = index("int16"), index("int16")
    x.update(a)
    y.update(b, mb, start_index=1000)
    x.merge(y)
    ref = jn.IndexNp().update(a).update(b, mb, start_index=1000)
    check_info(x, ref)
    check_map(x, ref, np.arange(-10, 610, dtype=np.int16))
    with pytest.raises(HipError, match="sealed"):
        x.update(a)
    with pytest.raises(HipError, match="sealed"):
        y.merge(x)


# ---- vh_take ---------------------------------------------------------------------------------
@pytest.mark.parametrize("idx_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("ncols", [1, 8, 9])
def test_take(ncols, idx_dtype):
    """Item sizes 1, 2, 4, 8 over 1, 8 and 9 columns; -1 entries give 0 and set the mask; n is
    no multiple of the 4 rows of a lane."""
    rng = np.random.default_rng(ncols)
    m, n = 1000, 4099
    dts = [np.float64, np.int8, np.int16, np.float32, np.uint64, np.bool_, np.uint16, np.int32, np.int64][:ncols]
    cols = [rng.integers(1, 100, m).astype(dt) for dt in dts]
    idx = rng.integers(-1, m, n).astype(idx_dtype)
    idx[:3] = [-1, 0, m - 1]
    outs, mask = su().take_device([dev(c) for c in cols], dev(idx), with_mask=True)
    assert mask.to_numpy().tolist() == (idx < 0).tolist()
    for c, o in zip(cols, outs):
        exp = np.where(idx < 0, np.zeros(1, c.dtype), c[np.where(idx < 0, 0, idx)])
        assert o.dtype == c.dtype and o.to_numpy().tolist() == exp.tolist()
    outs = su().take_device([dev(c) for c in cols], dev(idx)[1:])  # a misaligned index slice, no mask
    for c, o in zip(cols, outs):
        exp = np.where(idx[1:] < 0, np.zeros(1, c.dtype), c[np.where(idx[1:] < 0, 0, idx[1:])])
        assert o.to_numpy().tolist() == exp.tolist()


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1024, 1025])
def test_take_sizes(n):
    col = np.arange(50, dtype=np.float64) * 1.5
    idx = (np.arange(n) * 7 % 50).astype(np.int32)
    out, = su().take_device([dev(col)], dev(idx))
    assert out.to_numpy().tolist() == col[idx].tolist()


# ---- vh_index_matched ------------------------------------------------------------------------
@pytest.mark.parametrize("idx_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("kind", ["none", "all", "alternating", "random"])
def test_matched(kind, idx_dtype):
    n = 5001
    rng = np.random.default_rng(14)
    idx = rng.integers(0, 1000, n).astype(idx_dtype)
    if kind == "none":
        idx[:] = -1
    elif kind == "alternating":
        idx[::2] = -1
    elif kind == "random":
        idx[rng.random(n) < 0.5] = -1
    rows, out = su().index_matched(dev(idx))
    exp_rows = np.where(idx != -1)[0]
    assert rows.dtype == np.int64 and out.dtype == np.dtype(idx_dtype)
    assert rows.to_numpy().tolist() == exp_rows.tolist() and out.to_numpy().tolist() == idx[exp_rows].tolist()
