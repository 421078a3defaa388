"""String columns on the device (vaex_amd/strings.py, csrc/strings.hip): the column type, the
offset check, the dictionary encoder with its collision rounds and table growth, the byte-exact
gather, the literal predicates and lengths, and the string keys of value_counts / unique /
groupby / sort -- codes, masks and lengths bit for bit against the plain-Python restatement
(tests/strings_np.py), group results as maps like the integer groupby tests."""
import numpy as np
import pyarrow as pa
import pytest

import strings_np
import vaex_amd
from vaex_amd import DeviceArray, _lib
from vaex_amd.strings import DeviceStringArray, ordered_set_string

pytestmark = pytest.mark.gpu

EDGE = strings_np.edge_strings()


def _col(values, large=False):
    return DeviceStringArray.from_list(list(values), large=large)


def _ids(n, k, fmt="id%03d", seed=0):
    rng = np.random.default_rng(seed)
    return [fmt % v for v in rng.integers(0, k, size=n).tolist()]


def _encoded(values, large=False, **kw):
    col = _col(values, large=large)
    s = ordered_set_string(**kw)
    s.update(col)
    return s, s.map_ordinal(col).to_numpy()


# ---- the column type ------------------------------------------------------------------------------
@pytest.mark.parametrize("large", [False, True])
def test_round_trip_and_shape(large):
    col = _col(EDGE, large=large)
    assert len(col) == len(EDGE) and col.shape == (len(EDGE),) and col.ndim == 1
    assert col.offsets.dtype == (np.int64 if large else np.int32)
    nbytes = int(strings_np.byte_length(EDGE).sum())
    assert col.nbytes == (len(EDGE) + 1) * col.offsets.dtype.itemsize + nbytes
    assert col.tolist() == EDGE
    assert col.to_numpy().dtype == object and col.to_numpy().tolist() == EDGE
    back = col.to_arrow()
    assert back.type == (pa.large_string() if large else pa.string()) and back.to_pylist() == EDGE
    typ = pa.large_string() if large else pa.string()
    assert DeviceStringArray.from_arrow(pa.array(EDGE, type=typ)).tolist() == EDGE
    assert DeviceStringArray.from_arrow(pa.chunked_array([pa.array(EDGE[:5], type=typ), pa.array(EDGE[5:], type=typ)])).tolist() == EDGE
    assert DeviceStringArray.from_arrow(pa.array(EDGE, type=typ)[7:40]).tolist() == EDGE[7:40]
    assert DeviceStringArray.from_numpy(np.array(EDGE[:50], dtype=object)).tolist() == EDGE[:50]
    assert DeviceStringArray.from_numpy(np.array(["ab", "c", ""])).tolist() == ["ab", "c", ""]


def test_empty_and_one_row():
    for values in ([], ["only"], [""]):
        col = _col(values)
        assert len(col) == len(values) and col.tolist() == values
        assert col.len().to_numpy().tolist() == [len(v) for v in values]
        assert col.match("str_contains", "n").to_numpy().tolist() == ["n" in v for v in values]
        s, codes = _encoded(values)
        assert len(s) == len(set(values)) and s.keys() == list(dict.fromkeys(values)) and codes.tolist() == [0] * len(values)
        assert col.take(DeviceArray.from_numpy(np.zeros(0, np.int32))).tolist() == []


def test_slice_is_a_view_with_an_unaligned_first_offset():
    col = _col(EDGE)
    starts = np.concatenate([[0], np.cumsum(strings_np.byte_length(EDGE))])
    i1 = next(i for i in range(3, len(EDGE)) if starts[i] % 8 not in (0,) and starts[i] > 0)
    part = col[i1:i1 + 120]
    assert part._root[0] is col._root[0]  # zero-copy: the parent's allocation
    assert int(part.offsets.to_numpy()[0]) == starts[i1] and starts[i1] % 8 != 0
    want = EDGE[i1:i1 + 120]
    assert part.tolist() == want
    assert np.array_equal(part.len("str_byte_length").to_numpy(), strings_np.byte_length(want))
    assert np.array_equal(part.match("str_endswith", "b").to_numpy(), strings_np.endswith(want, "b"))
    s = ordered_set_string()
    s.update(part)
    codes, keys = strings_np.encode(want)
    assert s.keys() == keys and np.array_equal(s.map_ordinal(part).to_numpy(), codes)
    assert part[5:9].tolist() == want[5:9] and part[200:].tolist() == []


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_bad_offsets_raise_before_any_byte_is_read(dtype):
    data = DeviceArray.from_numpy(np.frombuffer(b"abcdefgh", dtype=np.uint8))
    ok = DeviceStringArray(DeviceArray.from_numpy(np.array([0, 3, 3, 8], dtype)), data)
    assert ok.tolist() == ["abc", "", "defgh"]
    for bad in ([0, 5, 3, 8], [0, 3, 9], [0, 3, 1 << 30], [-1, 3, 8], [4, 3]):
        with pytest.raises(ValueError, match="offsets"):
            DeviceStringArray(DeviceArray.from_numpy(np.array(bad, dtype)), data)


# ---- lengths and predicates -----------------------------------------------------------------------
@pytest.mark.parametrize("large", [False, True])
def test_lengths_on_the_edge_strings(large):
    col = _col(EDGE, large=large)
    assert np.array_equal(col.len("str_len").to_numpy(), strings_np.length(EDGE))
    assert np.array_equal(col.len("str_byte_length").to_numpy(), strings_np.byte_length(EDGE))
    assert (strings_np.length(EDGE) != strings_np.byte_length(EDGE)).any()


PATTERNS = ["", "a", "ab", "aab", "\0", "a\0", "a\0b", "é", "€z", "\U0001d11e", "f" * 7, "zz-not-there", "x" * 40,
            EDGE[100], EDGE[-3][-1024:], EDGE[-3][:1024], EDGE[-3][35000:35017]]


@pytest.mark.parametrize("k", range(len(PATTERNS)))
def test_predicates_on_the_edge_strings(k):
    pat = PATTERNS[k]
    col = _col(EDGE)
    for op, fn in strings_np.PREDICATES.items():
        got = col.match(op, pat)
        assert got.dtype == np.bool_
        assert np.array_equal(got.to_numpy(), fn(EDGE, pat)), (op, pat[:20])


@pytest.mark.parametrize("large", [False, True])
def test_predicate_special_cases(large):
    col = _col(EDGE, large=large)
    for op, fn in strings_np.PREDICATES.items():
        assert np.array_equal(col.match(op, "ab").to_numpy(), fn(EDGE, "ab")), op
    col = _col(["aaab", "aab", "ab", "xaab", "", "b"], large=large)
    assert col.match("str_contains", "aab").to_numpy().tolist() == [True, True, False, True, False, False]
    assert col.match("str_contains", "").to_numpy().all() and col.match("str_startswith", "").to_numpy().all()
    assert col.match("str_contains", "aaabb").to_numpy().tolist() == [False] * 6  # longer than every string
    assert col.match("str_endswith", "b").to_numpy().tolist() == [True, True, True, True, False, True]
    big = "q" * 1024
    col = _col([big, big[:-1], "p" + big, big + "p"], large=large)
    assert col.match("str_contains", big).to_numpy().tolist() == [True, False, True, True]
    assert col.match("str_equals", big).to_numpy().tolist() == [True, False, False, False]
    with pytest.raises(NotImplementedError, match="1024"):
        col.match("str_contains", "q" * 1025)


def _frame(n=5000, seed=1):
    rng = np.random.default_rng(seed)
    ids = _ids(n, 40, seed=seed)
    v = rng.integers(0, 10, size=n).astype(np.int64)
    w = rng.normal(size=n)
    df = vaex_amd.from_arrays(id1=_col(ids), v=DeviceArray.from_numpy(v), w=DeviceArray.from_numpy(w))
    return df, np.array(ids, dtype=object), v, w


def test_expression_surface():
    df, ids, v, w = _frame()
    assert df.data_type("id1") == str and df.id1.dtype.kind == "T"
    assert str(df.id1 == "id016") == "str_equals(id1, 'id016')" and str(df.id1 != "x") == "str_notequals(id1, 'x')"
    assert str(df.id1.str.contains("d01")) == "str_contains(id1, 'd01')"
    assert str(df.id1.str.len()) == "str_len(id1)" and str(df.id1.str.byte_length()) == "str_byte_length(id1)"
    with pytest.raises(NotImplementedError):
        df.id1.str.contains("d.1", regex=True)
    with pytest.raises(NotImplementedError):
        df.evaluate("str_contains(id1, 'd.1', regex=True)")
    assert np.array_equal(df.evaluate(df.id1.str.startswith("id01")).to_numpy(), strings_np.startswith(ids, "id01"))
    assert np.array_equal(df.evaluate(df.id1.str.endswith("7")).to_numpy(), strings_np.endswith(ids, "7"))
    assert np.array_equal(df.evaluate(df.id1.str.equals("id007")).to_numpy(), ids == "id007")
    assert np.array_equal(df.evaluate("str_len(id1) + v").to_numpy(), 5 + v)
    assert df.evaluate("id1", 10, 20).tolist() == ids[10:20].tolist()  # a bare string column: the slice
    assert df.id1.tolist() == ids.tolist()
    assert int(df.count("id1")) == len(ids) and int(df.count()) == len(ids)
    for name in ("sum", "mean", "min", "max", "std"):
        with pytest.raises(TypeError):
            getattr(df, name)("id1")
    with pytest.raises(NotImplementedError, match="1024"):
        df.evaluate(df.id1.str.contains("q" * 1025))


def test_predicate_mixed_with_numbers_as_filter_and_selection():
    df, ids, v, w = _frame()
    keep = (ids == "id016") & (v > 3)
    # a chunk of the executor that does not start at row 0
    assert np.array_equal(df.evaluate('(id1 == "id016") & (v > 3)', 1003, 4001).to_numpy(), keep[1003:4001])
    f = df[(df.id1 == "id016") & (df.v > 3)]
    assert len(f) == keep.sum() and np.isclose(float(f.sum("w")), w[keep].sum())
    assert f.evaluate("id1").tolist() == ids[keep].tolist()
    keep2 = strings_np.contains(ids, "d01") | (w > 1)
    df.select('str_contains(id1, "d01") | (w > 1)')
    assert int(df.count(selection=True)) == keep2.sum()
    assert np.isclose(float(df.sum("w", selection=True)), w[keep2].sum())
    df.select(df.id1 != "id003", mode="and")
    assert int(df.count(selection=True)) == (keep2 & (ids != "id003")).sum()
    df.add_virtual_column("hit", 'str_startswith(id1, "id00") & (v < 5)')
    assert int(df.sum("hit")) == (strings_np.startswith(ids, "id00") & (v < 5)).sum()


# ---- the encoder ------------------------------------------------------------------------------------
def _check_set(values, s, got_codes):
    codes, keys = strings_np.encode(values)
    assert len(s) == len(keys)
    assert s.keys() == keys
    assert got_codes.dtype == np.int32 and np.array_equal(got_codes, codes)


@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("form", ["lane", "wave"])
def test_encoder_on_the_edge_strings_in_both_forms(form, large, monkeypatch):
    monkeypatch.setenv("VH_STR_FORM", form)  # read per call; the 70,000-byte string runs in both
    s, codes = _encoded(EDGE * 2, large=large)
    _check_set(EDGE * 2, s, codes)
    assert _lib.stat_read("strset_form") == (form == "wave")
    idx = np.arange(len(EDGE) - 1, -1, -1).astype(np.int32)
    assert _col(EDGE).take(DeviceArray.from_numpy(idx)).tolist() == EDGE[::-1]
    assert s.__sizeof__() > 0 and s.key_array().dtype == object


def test_short_strings_take_the_lane_form():
    short = [e for e in EDGE if len(e) < 100]
    _lib.stat_read("strset_form")
    s, codes = _encoded(short * 2)
    _check_set(short * 2, s, codes)
    assert _lib.stat_read("strset_form") == 0


def test_encoder_many_rows_few_keys():
    values = _ids(300_000, 1000)
    _lib.stat_read("strset_rounds")
    s, codes = _encoded(values)
    _check_set(values, s, codes)
    assert _lib.stat_read("strset_rounds") == 1  # the full hash: one round


def test_encoder_all_distinct_with_growth():
    n = 1 << 17
    values = ["k%07d" % ((i * 7919) % n) for i in range(n)]
    s, codes = _encoded(values, initial_capacity=64)
    assert len(s) == n and np.array_equal(codes, np.arange(n, dtype=np.int32))
    assert s.keys() == values


def test_encoder_all_equal():
    s, codes = _encoded(["same-string"] * 10_000)
    assert s.keys() == ["same-string"] and not codes.any()


def test_encoder_wave_form_on_long_strings():
    values = strings_np.long_strings(4000, mean=300)
    assert 250 < strings_np.byte_length(values).mean() < 350
    _lib.stat_read("strset_form")
    s, codes = _encoded(values)
    assert _lib.stat_read("strset_form") == 1  # wave per row
    _check_set(values, s, codes)
    col = _col(values)
    assert np.array_equal(col.match("str_endswith", "07").to_numpy(), strings_np.endswith(values, "07"))
    idx = np.random.default_rng(3).integers(0, len(values), size=1000).astype(np.int32)
    assert col.take(DeviceArray.from_numpy(idx)).tolist() == [values[i] for i in idx]


@pytest.mark.parametrize("hash_bits", [64, 4])
def test_two_updates_and_absent_strings(hash_bits):
    a = _ids(3000, 30, seed=1) + EDGE[:60]
    b = _ids(3000, 60, seed=2) + EDGE[30:120] + ["brand-new"]
    s = ordered_set_string(hash_bits=hash_bits)
    s.update(_col(a))
    codes_a, keys_a = strings_np.encode(a)
    assert s.keys() == keys_a
    s.update(_col(b))
    codes_b, keys = strings_np.encode(b, keys_a)
    assert s.keys() == keys and keys[:len(keys_a)] == keys_a
    assert np.array_equal(s.map_ordinal(_col(a)).to_numpy(), codes_a)
    assert np.array_equal(s.map_ordinal(_col(b)).to_numpy(), codes_b)
    other = ["id001", "absent", "", "id0", "id0011", "a\0", "a\0c", "brand-new", "brand-ne"]
    assert np.array_equal(s.map_ordinal(_col(other)).to_numpy(), strings_np.map_ordinal(other, keys))
    assert (strings_np.map_ordinal(other, keys) == -1).sum() >= 4


def test_collision_rounds_equal_the_full_hash():
    values = _ids(5000, 40, seed=5)
    full, codes_full = _encoded(values)
    assert len(full) == 40
    _lib.stat_read("strset_rounds")
    s0, codes0 = _encoded(values, hash_bits=0)  # every string collides: one level per distinct string
    assert _lib.stat_read("strset_rounds") == 40 and s0.levels == 40
    assert s0.keys() == full.keys() and np.array_equal(codes0, codes_full)
    s0.update(_col(["new-a", "id001", "new-b", "new-a"]))  # a later update walks the levels, then adds two
    assert s0.keys() == full.keys() + ["new-a", "new-b"] and s0.levels == 42
    assert s0.map_ordinal(_col(["new-b", "nope", values[0]])).to_numpy().tolist() == [41, -1, 0]
    values = _ids(5000, 300, seed=6)
    full, codes_full = _encoded(values)
    _lib.stat_read("strset_rounds")  # a running maximum: reset, the 42 levels above are still in it
    s4, codes4 = _encoded(values, hash_bits=4)
    assert _lib.stat_read("strset_rounds") > 1
    assert s4.keys() == full.keys() and np.array_equal(codes4, codes_full)
    _check_set(values, s4, codes4)


# ---- take --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("idt", [np.int32, np.int64])
def test_take_is_byte_exact(large, idt):
    col = _col(EDGE, large=large)
    idx = np.random.default_rng(0).integers(0, len(EDGE), size=700).astype(idt)
    idx[:3] = [len(EDGE) - 3, 0, len(EDGE) - 3]  # the 70,000-byte string, twice
    out = col.take(DeviceArray.from_numpy(idx))
    assert out.offsets.dtype == col.offsets.dtype
    assert out.tolist() == [EDGE[i] for i in idx]
    assert out.take(DeviceArray.from_numpy(np.arange(699, -1, -1).astype(idt))).tolist() == [EDGE[i] for i in idx[::-1]]


# ---- value_counts / unique / nunique -------------------------------------------------------------------
def test_value_counts_unique_nunique():
    df, ids, v, w = _frame(20_000, seed=7)
    for ascending in (False, True):
        vc = df.id1.value_counts(ascending=ascending)
        keys, counts = strings_np.value_counts(ids, ascending=ascending)
        assert vc.index.tolist() == keys and np.array_equal(vc.to_numpy(), counts)
    assert df.id1.unique() == strings_np.unique(ids)
    assert df.id1.nunique() == 40
    keys, inverse = df.unique("id1", return_inverse=True)
    assert np.array_equal(inverse, strings_np.encode(ids)[0]) and keys == strings_np.unique(ids)
    keep = v > 6
    f = df[df.v > 6]
    vc = f.id1.value_counts()
    keys, counts = strings_np.value_counts(ids[keep])
    assert vc.index.tolist() == keys and np.array_equal(vc.to_numpy(), counts)
    assert f.id1.unique() == strings_np.unique(ids[keep]) and f.id1.nunique() == len(set(ids[keep]))
    # return_inverse on a filtered frame indexes the kept uniques; a row whose string no kept row holds gets -1
    keys, inverse = df[df.id1 != "id003"].unique("id1", return_inverse=True)
    assert keys == strings_np.unique(ids[ids != "id003"])
    assert np.array_equal(inverse, strings_np.map_ordinal(ids, keys)) and (inverse == -1).sum() == (ids == "id003").sum()
    df.select(df.v < 3)
    assert df.id1.unique(selection=True) == strings_np.unique(ids[v < 3])
    vc = df.value_counts("id1", selection=True)
    keys, counts = strings_np.value_counts(ids[v < 3])
    assert vc.index.tolist() == keys and np.array_equal(vc.to_numpy(), counts)


# ---- groupby ---------------------------------------------------------------------------------------------
def _groups(res, by):
    cols = {k: np.asarray(c) for k, c in res.columns.items()}
    n = len(cols[by[0]])
    keys = list(zip(*[cols[b].tolist() for b in by]))
    assert len(set(keys)) == n
    return keys, {k: {name: cols[name][i] for name in cols if name not in by} for i, k in enumerate(keys)}


def _want(bycols, v, w):
    want = {}
    for i, k in enumerate(zip(*[c.tolist() for c in bycols])):
        e = want.setdefault(k, [0, 0, 0.0, np.inf])
        e[0] += 1
        e[1] += int(v[i])
        e[2] += float(w[i])
        e[3] = min(e[3], float(w[i]))
    return want


def _check_groups(res, by, bycols, v, w):
    keys, got = _groups(res, by)
    want = _want(bycols, v, w)
    assert set(keys) == set(want)
    for k, e in want.items():
        g = got[k]
        assert int(g["count"]) == e[0] and int(g["v_sum"]) == e[1], k
        assert np.isclose(float(g["w_sum"]), e[2], rtol=1e-9, atol=1e-9) and float(g["w_min"]) == e[3], k
    return keys


AGG = {"count": "count", "v_sum": vaex_amd.agg.sum("v"), "w_sum": vaex_amd.agg.sum("w"), "w_min": vaex_amd.agg.min("w")}


@pytest.mark.parametrize("assume_sparse", ["auto", True, False])
@pytest.mark.parametrize("sort", [False, True])
def test_groupby_one_string_key(sort, assume_sparse):
    df, ids, v, w = _frame(20_000, seed=9)
    res = df.groupby("id1", agg=AGG, sort=sort, assume_sparse=assume_sparse)
    keys = [k[0] for k in _check_groups(res, ["id1"], [ids], v, w)]
    assert keys == (sorted(set(ids)) if sort else strings_np.unique(ids))  # sorted, or first-appearance order
    keep = v >= 5
    res = df[df.v >= 5].groupby("id1", agg=AGG, sort=sort, assume_sparse=assume_sparse)
    _check_groups(res, ["id1"], [ids[keep]], v[keep], w[keep])


@pytest.mark.parametrize("assume_sparse", ["auto", True, False])
@pytest.mark.parametrize("sort", [False, True])
def test_groupby_two_string_keys_and_a_mixed_pair(sort, assume_sparse):
    n = 20_000
    rng = np.random.default_rng(11)
    id1 = np.array(_ids(n, 12, seed=1), dtype=object)
    id2 = np.array(_ids(n, 7, fmt="é%d", seed=2), dtype=object)
    k3 = rng.integers(-3, 4, size=n).astype(np.int32)
    v = rng.integers(0, 10, size=n).astype(np.int64)
    w = rng.normal(size=n)
    df = vaex_amd.from_arrays(id1=_col(id1), id2=_col(id2), k3=DeviceArray.from_numpy(k3), v=DeviceArray.from_numpy(v),
                              w=DeviceArray.from_numpy(w))
    res = df.groupby(["id1", "id2"], agg=AGG, sort=sort, assume_sparse=assume_sparse)
    keys = _check_groups(res, ["id1", "id2"], [id1, id2], v, w)
    if sort:
        assert keys == sorted(keys)
    res = df.groupby(["id1", "k3"], agg=AGG, sort=sort, assume_sparse=assume_sparse)
    keys = _check_groups(res, ["id1", "k3"], [id1, k3], v, w)
    if sort:
        assert keys == sorted(keys)


def test_groupby_without_agg_defers_to_the_agg_route():
    df, ids, v, w = _frame(6000, seed=19)
    gb = df.groupby("id1", sort=True)
    keys = [k[0] for k in _check_groups(gb.agg(AGG), ["id1"], [ids], v, w)]
    assert keys == sorted(set(ids))
    with pytest.raises(NotImplementedError, match="string key"):
        gb.by  # the grouper-based GroupBy reads numeric keys


# ---- take / extract / sort ---------------------------------------------------------------------------------
def test_take_extract_sort_carry_string_columns():
    df, ids, v, w = _frame(6000, seed=13)
    idx = np.random.default_rng(1).integers(0, len(ids), size=500)
    t = df.take(idx)
    assert t.id1.tolist() == ids[idx].tolist() and np.array_equal(t.v.to_numpy(), v[idx])
    e = df[df.v > 7].extract()
    assert len(e) == (v > 7).sum() and e.id1.tolist() == ids[v > 7].tolist()
    s = df.sort("w")
    order = np.argsort(w, kind="stable")
    assert s.id1.tolist() == ids[order].tolist()


@pytest.mark.parametrize("ascending", [True, False])
def test_sort_by_string_keys_is_stable(ascending):
    df, ids, v, w = _frame(6000, seed=17)
    rows = np.arange(len(ids))
    df.add_column("row", DeviceArray.from_numpy(rows))
    s = df.sort("id1", ascending=ascending)
    order = strings_np.argsort(ids, ascending=ascending)  # 40 keys over 6000 rows: ties everywhere
    assert np.array_equal(s.row.to_numpy(), order) and s.id1.tolist() == ids[order].tolist()
    s = df.sort(["v", "id1"], ascending=ascending)
    assert np.array_equal(s.row.to_numpy(), strings_np.lexsort([v, ids], ascending=ascending))
    s = df.sort(["id1", "v"], ascending=ascending)
    assert np.array_equal(s.row.to_numpy(), strings_np.lexsort([ids, v], ascending=ascending))
    # strings whose order differs from their first-appearance order, multi-byte ones included
    vals = np.array(["b", "é", "a", "ab", "", "a\0", "€", "a", "b", "aa"] * 30, dtype=object)
    d2 = vaex_amd.from_arrays(s=_col(vals), row=DeviceArray.from_numpy(np.arange(len(vals))))
    assert np.array_equal(d2.sort("s", ascending=ascending).row.to_numpy(), strings_np.argsort(vals, ascending=ascending))
    f = df[df.v > 4].sort("id1", ascending=ascending)
    keep = np.flatnonzero(v > 4)
    assert np.array_equal(f.row.to_numpy(), keep[strings_np.argsort(ids[keep], ascending=ascending)])
