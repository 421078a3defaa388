"""The GPU hash counter (``superutils.counter_<dtype>``) and ``value_counts / unique / nunique``
against the NumPy restatement of the reference (tests/value_counts_np.py).  Every comparison
is exact: keys (NaN equals NaN, -0.0 differs from 0.0), counts and order.

Shapes are chosen where the kernel can go wrong, not for speed: distinct-key counts around the
LDS table size, one key over several segments and past the flush bound, a sorted column that
makes a workgroup drop its LDS keys, ragged and misaligned columns, keys
that collide in their low 32 bits, the EMPTY bit patterns, growth from a 16-slot table."""
import pickle

import numpy as np
import pytest

import value_counts_np as vc

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32", "int64", "int32", "int16", "int8", "uint64", "uint32", "uint16", "uint8", "bool"]


def su():
    import vaex_amd.superutils as m
    return m


def dev(a):
    from vaex_amd.device import DeviceArray
    return DeviceArray.from_numpy(a)


def counter(dtype, **kw):
    return su().counter_type_from_dtype(dtype)(**kw)


def check_counter(c, values, mask=None, select=None):
    """key_array / counts / info and both sorted reads of `c` against the restatement."""
    keys, counts, null_index = vc.counter_np(values, mask, select)
    assert vc.same_labels(c.key_array().tolist(), keys.tolist())
    assert c.key_array().dtype == keys.dtype
    assert c.counts().tolist() == counts.tolist() and c.counts().dtype == np.int64
    assert len(c) == len(keys) and c.null_index == null_index
    assert c.null_count == (counts[null_index] if null_index >= 0 else 0)
    for ascending in (True, False):
        for drop in (False, True):
            k, n, ni = c.sorted_counts(ascending=ascending, dropnan=drop, dropmissing=drop)
            ek, en, eni = vc.sorted_counts_np(values, mask, select, ascending, drop, drop)
            assert vc.same_labels(k.tolist(), ek.tolist()) and n.tolist() == en.tolist() and ni == eni


def make_column(dtype, n, distinct, seed=0):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "b":
        return rng.integers(0, 2, n).astype(bool)
    if dt.kind == "f":
        pool = np.concatenate([rng.normal(size=distinct - 4) * 1e3, [0.0, -0.0, np.inf, -np.inf]]).astype(dt)
        v = pool[rng.integers(0, distinct, n)]
        v[rng.random(n) < 0.03] = np.nan
        return v
    info = np.iinfo(dt)
    span = min(distinct, int(info.max) - int(info.min) + 1)
    pool = np.concatenate([np.array([info.min, info.max], dt), rng.integers(info.min, info.max, span - 2, dtype=dt, endpoint=True)])
    return pool.astype(dt)[rng.integers(0, span, n)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_dtypes(dtype):
    v = make_column(dtype, 5000, 50, seed=3)
    mask = np.random.default_rng(4).random(5000) < 0.1
    c = counter(dtype)
    c.update(v, mask)
    check_counter(c, v, mask)
    c2 = counter(dtype)
    c2.update(dev(v))  # HBM column, no mask
    check_counter(c2, v)
    if np.dtype(dtype).kind != "f":  # a dict cannot tell -0.0 from 0.0
        keys, counts, _ = vc.counter_np(v[~mask])
        assert c.extract() == dict(zip(keys.tolist(), counts.tolist()))


@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("which", ["1", "2", "S-1", "S", "S+1", "4S"])
def test_distinct_around_lds_table(dtype, which):
    S = su().COUNTER_LDS_SLOTS
    d = {"1": 1, "2": 2, "S-1": S - 1, "S": S, "S+1": S + 1, "4S": 4 * S}[which]
    rng = np.random.default_rng(d)
    keys = (rng.permutation(1 << 20)[:d].astype(np.int64) * 2654435761 % (1 << 31) - (1 << 30)).astype(dtype)
    v = np.repeat(keys, 8)
    rng.shuffle(v)
    c = counter(dtype)
    c.update(dev(v))
    check_counter(c, v)


@pytest.mark.parametrize("dtype", ["int32", "float64"])
def test_one_key_many_segments(dtype):
    # 2**20 rows of one key: 8 workgroups of 2**17 rows, each two segments of 2**16 rows
    v = np.full(1 << 20, 7, dtype)
    c = counter(dtype)
    c.update(dev(v))
    assert c.key_array().tolist() == [7] and c.counts().tolist() == [1 << 20] and len(c) == 1


def test_one_key_flush_and_continue():
    # A workgroup flushes inside its range before it has counted 2**20 rows since its last flush
    # (the host's bound on the 32-bit LDS counts).  Only a column of more than 512 * 2**20 rows
    # gives a workgroup that many: 6e8 one-byte rows of one key, filled on the device.
    from vaex_amd import _lib
    from vaex_amd.device import DeviceArray
    n = 600_000_000
    col = DeviceArray.empty(n, np.int8)
    _lib.call("vh_memset", col.ptr, 7, n)
    c = counter("int8")
    c.update(col)
    assert c.key_array().tolist() == [7] and c.counts().tolist() == [n] and len(c) == 1


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_sorted_column_drops_lds_keys(dtype):
    # sorted, 8 rows per key: every 2**16-row segment brings 8192 new keys, so the workgroup
    # flushes, drops its LDS keys and continues at every segment
    v = np.repeat(np.arange(-20000, 20000).astype(dtype), 8)
    c = counter(dtype)
    c.update(dev(v))
    check_counter(c, v)


def test_many_keys_sampled_table():
    # >= 2**20 rows: the table is sized from a sample; 200k distinct keys all pass the LDS table by
    v = (np.random.default_rng(5).integers(0, 200_000, 1 << 20) * 7919).astype(np.int32)
    c = counter("int32")
    c.update(dev(v))
    keys, counts, _ = vc.counter_np(v)
    assert np.array_equal(c.key_array(), keys) and np.array_equal(c.counts(), counts)


@pytest.mark.parametrize("dtype", ["int8", "uint16", "int32", "float64"])
def test_ragged_and_misaligned(dtype):
    n = 3 * 4096 + 5  # not a multiple of the 8 rows a lane takes, nor of a workgroup's step
    v = make_column(dtype, n + 1, 40, seed=6)
    mask = np.random.default_rng(7).random(n + 1) < 0.2
    sel = np.random.default_rng(8).random(n + 1) < 0.7
    dv, dm, ds = dev(v), dev(mask.astype(np.uint8)), dev(sel.astype(np.uint8))
    c = counter(dtype)
    c.update(dv[1:], dm[1:], select=ds[1:])  # starts at row 1: no wide loads
    check_counter(c, v[1:], mask[1:], sel[1:])
    c = counter(dtype)
    c.update(dv[:n])
    check_counter(c, v[:n])


@pytest.mark.parametrize("dtype", ["int64", "uint64", "float64"])
def test_keys_sharing_low_32_bits(dtype):
    hi = np.random.default_rng(9).integers(0, 300, 4000).astype(np.uint64)
    v = ((hi << np.uint64(32)) | np.uint64(0x3ff00007)).view(dtype) if dtype != "float64" else \
        ((hi << np.uint64(32)) | np.uint64(7)).view(np.float64)
    v = np.ascontiguousarray(v)
    c = counter(dtype)
    c.update(v)
    check_counter(c, v)


@pytest.mark.parametrize("dtype,top", [("int64", -1), ("uint64", 2 ** 64 - 1), ("int32", -1), ("uint32", 2 ** 32 - 1)])
def test_all_ones_key(dtype, top):
    # int64 -1 / uint64 max: the HBM table's EMPTY pattern (side counter); 4-byte: the LDS table's
    alone = np.full(100, top, dtype)
    c = counter(dtype)
    c.update(alone)
    check_counter(c, alone)
    assert c.extract() == {top: 100}
    among = np.concatenate([alone, np.arange(-50, 50).astype(dtype), alone[:3]])
    c = counter(dtype)
    c.update(dev(among))
    c.update(among[:10])
    check_counter(c, np.concatenate([among, among[:10]]))


def test_nan_payloads_and_signed_zero():
    b64 = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000001, 0xfff0000000000001,
                    0x0000000000000000, 0x8000000000000000, 0x8000000000000000, 0x3ff0000000000000], np.uint64)
    v = np.tile(b64.view(np.float64), 100)
    c = counter("float64")
    c.update(v)
    check_counter(c, v)
    assert c.nan_count == 400 and vc.same_labels(c.key_array().tolist(), [float("nan"), -0.0, 0.0, 1.0])
    assert c.counts().tolist() == [400, 200, 100, 100]
    b32 = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x00000000, 0x80000000, 0x3f800000], np.uint32)
    v = np.tile(b32.view(np.float32), 100)
    c = counter("float32")
    c.update(dev(v))
    check_counter(c, v)
    assert c.nan_count == 400 and len(c) == 4


def frames(n=6000):
    import vaex_amd
    rng = np.random.default_rng(11)
    x = rng.integers(0, 40, n).astype(np.float64)
    x[rng.random(n) < 0.05] = np.nan
    xm = np.ma.array(x, mask=rng.random(n) < 0.1)
    y = rng.integers(0, 100, n).astype(np.int32)
    host = vaex_amd.from_arrays(x=x, xm=xm, y=y)
    hbm = vaex_amd.from_arrays(x=dev(x), xm=xm, y=dev(y))
    return host, hbm, x, xm, y


@pytest.mark.parametrize("case", ["plain", "masked", "selection", "filter", "all"])
def test_frames_host_and_hbm(case):
    host, hbm, x, xm, y = frames()
    col = "xm" if case in ("masked", "all") else "x"
    values = xm if col == "xm" else x
    keep = np.ones(len(x), bool)
    selection = None
    if case in ("filter", "all"):
        host, hbm = host[host.y > 20], hbm[hbm.y > 20]
        keep &= y > 20
    if case in ("selection", "all"):
        selection = "y < 80"
        keep &= y < 80
    for kw in ({}, {"ascending": True}, {"dropna": True}, {"dropmissing": True}):
        expected = vc.value_counts_np(values, select=keep, **kw)
        a = host.value_counts(col, selection=selection, **kw)
        b = hbm.value_counts(col, selection=selection, **kw)
        vc.assert_series_same(a, expected)
        vc.assert_series_same(b, expected)
        vc.assert_series_same(a, b)
    if selection is None:
        vc.assert_series_same(host[col].value_counts(), vc.value_counts_np(values, select=keep))
        vc.assert_series_same(hbm[col].value_counts(), vc.value_counts_np(values, select=keep))


def test_growth_does_not_double_count():
    keys = (np.random.default_rng(12).permutation(1 << 16)[:5000] - 30000).astype(np.int32)
    c = counter("int32", initial_capacity=16)
    c.update(keys)
    assert len(c) == 5000
    c.update(dev(keys[::-1].copy()))
    assert len(c) == 5000
    assert c.counts().tolist() == [2] * 5000
    assert np.array_equal(c.key_array(), np.sort(keys))
    # the add path (merge, un-pickle) grows the same way
    c2 = counter("int32", initial_capacity=16)
    c2.merge(c)
    c2.merge(c)
    assert len(c2) == 5000 and c2.counts().tolist() == [4] * 5000


def test_merge_and_pickle():
    rng = np.random.default_rng(13)
    a = rng.integers(0, 60, 3000).astype(np.float32)
    b = rng.integers(30, 90, 2000).astype(np.float32)
    a[::50] = np.nan
    b[::40] = np.nan
    ma, mb = rng.random(3000) < 0.1, rng.random(2000) < 0.1
    ca, cb = counter("float32"), counter("float32")
    ca.update(a, ma)
    cb.update(b, mb)
    ca.merge(cb)
    both, mboth = np.concatenate([a, b]), np.concatenate([ma, mb])
    check_counter(ca, both, mboth)
    check_counter(cb, b, mb)  # the merged-from counter is unchanged
    back = pickle.loads(pickle.dumps(ca))
    assert type(back) is type(ca)
    check_counter(back, both, mboth)
    empty = pickle.loads(pickle.dumps(counter("int16")))
    assert len(empty) == 0 and empty.key_array().tolist() == []
    k = counter("uint64")  # no NaN: the null entry is at index 0 through the round trip
    k.update(np.array([5, 5, 2 ** 64 - 1], np.uint64), np.array([0, 1, 0], bool))
    back = pickle.loads(pickle.dumps(k))
    assert back.key_array().tolist() == [0, 5, 2 ** 64 - 1] and back.counts().tolist() == [1, 1, 1] and back.null_index == 0


def test_chunks_equal_one_call():
    v = make_column("float64", 20000, 300, seed=14)
    mask = np.random.default_rng(15).random(20000) < 0.05
    one, many = counter("float64"), counter("float64")
    one.update(v, mask)
    for i in range(0, 20000, 3333):
        many.update(v[i:i + 3333], mask[i:i + 3333])
    assert vc.same_labels(one.key_array().tolist(), many.key_array().tolist())
    assert one.counts().tolist() == many.counts().tolist()
    check_counter(many, v, mask)


@pytest.mark.parametrize("dtype", ["float64", "int64", "uint8", "bool"])
def test_len_equals_ordered_set(dtype):
    v = make_column(dtype, 5000, 120, seed=16)
    if dtype == "int64":
        v[:5] = -1
    mask = np.random.default_rng(17).random(5000) < 0.05
    c = counter(dtype)
    s = su().ordered_set_type_from_dtype(dtype)()
    c.update(v, mask)
    s.update(v, mask)
    assert len(c) == len(s) and c.nan_count == s.nan_count and c.null_count == s.null_count


def test_value_counts_equals_groupby_count():
    import vaex_amd
    key = np.random.default_rng(18).integers(-500, 500, 50_000).astype(np.int32)
    for df in (vaex_amd.from_arrays(key=key), vaex_amd.from_arrays(key=dev(key))):
        s = df.key.value_counts()
        g = df.groupby("key", agg="count")
        gmap = dict(zip(g["key"].to_numpy().tolist(), g["count"].to_numpy().tolist()))
        assert dict(zip(s.index.tolist(), s.tolist())) == gmap
        assert (np.diff(s.to_numpy()) <= 0).all()  # most frequent first


def test_unique_nunique():
    import vaex_amd
    rng = np.random.default_rng(19)
    x = rng.integers(0, 30, 4000).astype(np.float64)
    x[rng.random(4000) < 0.05] = np.nan
    xm = np.ma.array(x, mask=rng.random(4000) < 0.1)
    y = rng.integers(0, 100, 4000).astype(np.int32)
    for df in (vaex_amd.from_arrays(x=x, xm=xm, y=y), vaex_amd.from_arrays(x=dev(x), xm=xm, y=dev(y))):
        for col, values in (("x", x), ("xm", xm)):
            for kw in ({}, {"dropna": True}, {"dropnan": True}, {"dropmissing": True}):
                expected = vc.unique_np(values, **kw)
                assert vc.same_labels(df.unique(col, **kw), expected)
                assert vc.same_labels(df[col].unique(**kw), expected)
                assert df[col].nunique(**kw) == len(expected)
        assert vc.same_labels(df.x.unique(selection="y < 50"), vc.unique_np(x, select=y < 50))
        assert df.y.nunique() == len(np.unique(y))
        # array_type: 'python' / 'list' give lists, 'numpy' / None arrays (masked with a missing entry)
        assert isinstance(df.unique("y", array_type="python"), list) and isinstance(df.y.unique(), list)
        for at in ("numpy", None):
            u = df.unique("y", array_type=at)
            assert isinstance(u, np.ndarray) and u.dtype == np.int32 and u.tolist() == vc.unique_np(y)
            um = df.unique("xm", array_type=at)
            assert np.ma.isMaskedArray(um) and vc.same_labels(um.tolist(), vc.unique_np(xm))
        with pytest.raises(ValueError):
            df.unique("y", array_type="arrow")
        with pytest.raises(ValueError):
            df.unique("y", axis=0)
        # return_inverse: keys[inverse] rebuilds the column; masked rows map to the null entry
        keys, inverse = df.unique("y", return_inverse=True, array_type="numpy")
        assert inverse.dtype == np.int64 and np.array_equal(keys[inverse], y)
        keys, inverse = df.unique("xm", return_inverse=True)
        m = np.ma.getmaskarray(xm)
        assert all(keys[i] is None for i in inverse[m][:50]) and None not in [keys[i] for i in inverse[~m][:200]]
        assert vc.same_labels([keys[i] for i in inverse[~m]], xm.data[~m].tolist())


def test_api_small_case():
    import vaex_amd
    nan = float("nan")
    x = np.array([0, 1, 1, 2, 2, 2, nan])
    xm = np.ma.array(x, mask=[1, 1, 0, 0, 0, 0, 0])
    for df in (vaex_amd.from_arrays(x=x, xm=xm), vaex_amd.from_arrays(x=dev(x), xm=xm)):
        s = df.x.value_counts()
        assert vc.same_labels(s.index.tolist(), [2.0, 1.0, 0.0, nan]) and s.tolist() == [3, 2, 1, 1]
        s = df.x.value_counts(dropna=True, ascending=True)
        assert s.index.tolist() == [0.0, 1.0, 2.0] and s.tolist() == [1, 2, 3]
        s = df.xm.value_counts()
        assert vc.same_labels(s.index.tolist(), ["missing", 2.0, 1.0, nan]) and s.tolist() == [2, 3, 1, 1]
        s = df.value_counts("xm", dropmissing=True)
        assert vc.same_labels(s.index.tolist(), [2.0, 1.0, nan]) and s.tolist() == [3, 1, 1]
        with pytest.raises(ValueError):
            df.x.value_counts(axis=0)
        assert df.x.nunique() == 4 and df.x.nunique(dropna=True) == 3 and df.xm.nunique() == 4


def test_datetime_keys():
    import vaex_amd
    t = np.array(["2020-01-02", "2020-01-01", "2020-01-02", "1969-12-31"], "datetime64[ns]")
    df = vaex_amd.from_arrays(t=t)
    s = df.t.value_counts()
    assert s.index.dtype == t.dtype and s.tolist() == [2, 1, 1]
    assert s.index.tolist() == vc.value_counts_np(t).index.tolist()
    assert df.unique("t", array_type="numpy").dtype == t.dtype
