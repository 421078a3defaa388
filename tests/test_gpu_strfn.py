"""String transforms on the device (vaex_amd/strings.py, csrc/strfn.hip): lower, upper, slice,
strip, pad, repeat, cat and replace, byte for byte and offset for offset against the
plain-Python restatement (tests/strfn_np.py), and through expressions, virtual columns and the
string keys of value_counts / groupby / sort."""
import numpy as np
import pytest

import strfn_np
import strings_np
import vaex_amd
from vaex_amd import DeviceArray
from vaex_amd.strings import DeviceStringArray

pytestmark = pytest.mark.gpu

EDGE = strings_np.edge_strings() + ["  a b \t", " \t\n\v\f\r", "\x1c x\xa0", "MiXed É ß İ ɐ Ɐ ẞ \U00010400\U00010428", "-5",
                                    "aaaa", "xaax", ""]


def _col(values, large=False):
    return DeviceStringArray.from_list(list(values), large=large)


def _view(values):
    """the values as a slice view whose first offset is not 0 (and not 8-aligned)"""
    col = _col(["pad", "é"] + list(values) + ["tail"])
    part = col[2:2 + len(values)]
    assert int(part.offsets.to_numpy()[0]) == 5
    return part


def _same(col, want):
    """the column holds exactly `want`: offsets (from its first) and bytes"""
    offsets, data = col._host()
    woff, wdata = strfn_np.column_bytes(want)
    assert offsets.dtype == col.offsets.dtype and len(offsets) == len(want) + 1
    assert np.array_equal(offsets, woff), np.flatnonzero(offsets != woff)[:5]
    assert np.array_equal(data, wdata), np.flatnonzero(data != wdata)[:5]


# (method, args, model function, model args) over one input column
CASES = [("lower", (), strfn_np.lower, ()), ("upper", (), strfn_np.upper, ()), ("upper", (True,), strfn_np.upper, (True,))]
CASES += [("slice", a, strfn_np.slice_, a) for a in [(0, 3), (2,), (-3,), (1, -1), (-5, -2), (5, 2), (0, 100000), (100000,),
                                                       (-100000, 4), (3, 3), (0, 0)]]
CASES += [(m, a, getattr(strfn_np, m), a) for m in ("strip", "lstrip", "rstrip") for a in [(), ("a",), ("fx \x01",), ("",)]]
CASES += [("pad", (w, side, "*"), strfn_np.pad, (w, side, "*")) for w in (0, 3, 4, 5, 19) for side in ("left", "right", "both")]
CASES += [("ljust", (6,), strfn_np.ljust, (6,)), ("rjust", (6, "."), strfn_np.rjust, (6, ".")),
          ("center", (7, "-"), strfn_np.center, (7, "-")), ("center", (6, "-"), strfn_np.center, (6, "-")),
          ("zfill", (4,), strfn_np.zfill, (4,))]
CASES += [("repeat", (k,), strfn_np.repeat, (k,)) for k in (0, 3, -1)]
CASES += [("cat", ("_x",), strfn_np.cat, ("_x",)), ("cat", ("é_", True), lambda col, c, first: strfn_np.cat(c, col), ("é_", True)),
          ("cat", ("",), strfn_np.cat, ("",))]
CASES += [("replace", a, strfn_np.replace, a) for a in [("a", "XY"), ("aa", "b"), ("aa", "b", 1), ("aa", "b", 0), ("a", "", -1),
                                                         ("é", "e"), ("f", "longer than it", 2), ("zz-not-there", "q")]]


@pytest.fixture(scope="module")
def edge_inputs():
    return {"int32": _col(EDGE), "int64": _col(EDGE, large=True), "view": _view(EDGE)}


@pytest.fixture(scope="module")
def edge_wanted():
    return [model(EDGE, *margs) for _, _, model, margs in CASES]


@pytest.mark.parametrize("layout", ["int32", "int64", "view"])
def test_every_transform_on_the_edge_strings(layout, edge_inputs, edge_wanted):
    col = edge_inputs[layout]
    for (method, args, _, _), want in zip(CASES, edge_wanted):
        out = getattr(col, method)(*args)
        assert out.offsets.dtype == col.offsets.dtype
        try:
            _same(out, want)
        except AssertionError as e:
            raise AssertionError(f"{method}{args}: {e}") from None


def test_parameter_edges_by_hand():
    col = _col(["aaaa", "  x  ", " \t\n", "-5", "é€", "abc"])
    assert col.replace("aa", "b").tolist() == ["bb", "  x  ", " \t\n", "-5", "é€", "abc"]
    assert col.replace("aa", "b", n=1).tolist()[0] == "baa" and col.replace("aa", "b", n=0).tolist()[0] == "aaaa"
    assert col.strip().tolist() == ["aaaa", "x", "", "-5", "é€", "abc"]
    assert col.zfill(4).tolist() == ["aaaa", "  x  ", "0 \t\n", "00-5", "00é€", "0abc"]
    assert col.center(6, "*").tolist()[3:] == ["**-5**", "**é€**", "*abc**"] and "abc".center(6, "*") == "*abc**"
    assert col.center(5, "*").tolist()[3:] == ["**-5*", "**é€*", "*abc*"] and "-5".center(5, "*") == "**-5*"
    assert col.slice(1, -1).tolist() == ["aa", " x ", "\t", "", "", "b"]
    assert col.repeat(0).tolist() == [""] * 6 and col.repeat(3).tolist()[3] == "-5-5-5"
    assert col.upper().tolist()[4:] == ["É€", "ABC"] and col.upper(ascii=True).tolist()[4:] == ["é€", "ABC"]


def test_cat_of_two_columns():
    other = [s[::-1][:9] + "é" for s in EDGE]
    a = _col(EDGE)
    for b in (_col(other), _col(other, large=True), _view(other)):
        out = a.cat(b)
        assert out.offsets.dtype == b.offsets.dtype  # a's are int32: the wider of the two
        _same(out, strfn_np.cat(EDGE, other))
    _same(_view(EDGE).cat(_view(other)), strfn_np.cat(EDGE, other))
    with pytest.raises(ValueError):
        a.cat(_col(["x"]))


def test_many_workgroups_and_a_partial_one():
    rng = np.random.default_rng(3)
    ids = [("Id%03d " if v % 3 else " ID%05dé") % v for v in rng.integers(0, 2000, size=100_003).tolist()]
    col = _col(ids)
    _same(col.lower(), strfn_np.lower(ids))
    _same(col.slice(0, 3), strfn_np.slice_(ids, 0, 3))
    _same(col.strip(), strfn_np.strip(ids))
    _same(col.cat("_k"), strfn_np.cat(ids, "_k"))
    _same(col.replace("d0", "D"), strfn_np.replace(ids, "d0", "D"))
    _same(col.rjust(9, "0"), strfn_np.rjust(ids, 9, "0"))
    _same(col.cat(col), strfn_np.cat(ids, ids))


@pytest.fixture(scope="module")
def long_rows():
    vals = strings_np.long_strings(2000, mean=300)
    vals[7] = "  " + vals[7] + " \t"
    vals[8] = ""
    want = [strfn_np.slice_(vals, 3, -2), strfn_np.strip(vals), strfn_np.rstrip(vals, "0123456789"),
            strfn_np.center(vals, 341, "*"), strfn_np.repeat(vals, 3), strfn_np.cat(vals, "-é"), strfn_np.cat("é-", vals),
            strfn_np.cat(vals, vals), strfn_np.upper(vals), strfn_np.replace(vals, "abc", "é")]
    return vals, want


@pytest.mark.parametrize("form", ["lane", "wave"])
def test_long_rows_in_both_forms(form, long_rows, monkeypatch):
    monkeypatch.setenv("VH_STR_FORM", form)  # read per call
    vals, want = long_rows
    col = _col(vals)
    got = [col.slice(3, -2), col.strip(), col.rstrip("0123456789"), col.center(341, "*"), col.repeat(3), col.cat("-é"),
           col.cat("é-", first=True), col.cat(col), col.upper(), col.replace("abc", "é")]
    for k, (g, w) in enumerate(zip(got, want)):
        try:
            _same(g, w)
        except AssertionError as e:
            raise AssertionError(f"transform {k}: {e}") from None


def test_empty_and_one_row_columns():
    for values in ([], ["Only one "], [""]):
        col = _col(values)
        _same(col.lower(), strfn_np.lower(values))
        _same(col.slice(1, 4), strfn_np.slice_(values, 1, 4))
        _same(col.strip(), strfn_np.strip(values))
        _same(col.center(12), strfn_np.center(values, 12))
        _same(col.repeat(2), strfn_np.repeat(values, 2))
        _same(col.cat("x"), strfn_np.cat(values, "x"))
        _same(col.cat(col), strfn_np.cat(values, values))
        _same(col.replace("n", "NN"), strfn_np.replace(values, "n", "NN"))
    part = _col(EDGE)[5:5]
    assert part.lower().tolist() == [] and part.cat("x").tolist() == []


def test_refusals():
    col = _col(["abc", "déf"])
    with pytest.raises(NotImplementedError):
        col.replace("a", "b", regex=True)
    with pytest.raises(NotImplementedError):
        col.replace("a", "b", flags=2)
    with pytest.raises(NotImplementedError):
        col.strip("é")
    with pytest.raises(ValueError):
        col.pad(5, fillchar="é")
    with pytest.raises(ValueError):
        col.pad(5, fillchar="ab")
    with pytest.raises(ValueError):
        col.pad(5, side="middle")
    with pytest.raises(ValueError):
        col.replace("", "x")
    with pytest.raises(NotImplementedError):
        col.replace("a" * 1025, "x")
    with pytest.raises(NotImplementedError):
        col.cat("a" * 1025)
    assert col.tolist() == ["abc", "déf"]


def test_a_result_that_cannot_fit_is_refused_before_anything_is_written():
    """repeats and widths are any int64: a length that wraps 64 bits (4 bytes x 2^62), a row past
    what the sum of all rows may hold, and a sum that would wrap are each refused by the plan."""
    col = _col(["abcd", "efgh", ""])
    for call in (lambda: col.repeat(2 ** 62), lambda: col.repeat(2 ** 63 - 1), lambda: col.ljust(2 ** 63 - 1),
                 lambda: col.center(2 ** 62, "*"), lambda: col.zfill(2 ** 61), lambda: _col(["ab"] * 5).rjust(2 ** 60)):
        with pytest.raises(MemoryError):
            call()
    with pytest.raises(ValueError):
        col.repeat(2 ** 63)  # not an int64
    assert _col(["", ""]).repeat(2 ** 62).tolist() == ["", ""]  # nothing to repeat: fits
    assert col.repeat(2).tolist() == ["abcdabcd", "efghefgh", ""]  # the column and the scratch are as they were


# ---- through the frame -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame():
    rng = np.random.default_rng(5)
    n = 20_011
    raw = [(" Id%03d " if k % 3 else "ID%03dé") % k for k in rng.integers(0, 60, size=n).tolist()]
    other = ["%d" % (k % 7) for k in range(n)]
    v = rng.integers(0, 10, size=n).astype(np.int64)
    df = vaex_amd.from_arrays(s=_col(raw), t=_col(other), v=DeviceArray.from_numpy(v))
    return df, raw, other, v


def test_transforms_feed_predicates_and_lengths(frame):
    df, raw, other, v = frame
    clean = strfn_np.lower(strfn_np.strip(raw))
    mask = strings_np.startswith(clean, "id00")
    e = df.s.str.strip().str.lower().str.startswith("id00")
    assert np.array_equal(df.evaluate(e).to_numpy(), mask) and df.data_type(e) == np.bool_
    assert np.array_equal(df.evaluate("str_startswith(str_lower(str_strip(s)), 'id00')").to_numpy(), mask)
    f = df[e]  # as a filter
    assert len(f) == mask.sum() and int(f.sum("v")) == v[mask].sum()
    assert f.evaluate("s").tolist() == [r for r, m in zip(raw, mask) if m]
    assert f.evaluate(df.s.str.strip()).tolist() == [r.strip() for r, m in zip(raw, mask) if m]
    df.select(e)  # as a selection
    assert int(df.count(selection=True)) == mask.sum() and int(df.sum("v", selection=True)) == v[mask].sum()
    df.select(df.s.str.strip() == "Id007", mode="or")
    mask2 = mask | (np.array(strfn_np.strip(raw), dtype=object) == "Id007")
    assert int(df.count(selection=True)) == mask2.sum()
    assert np.array_equal(df.evaluate("str_len(str_strip(s)) + v").to_numpy(), strings_np.length(strfn_np.strip(raw)) + v)
    assert np.array_equal(df.evaluate("str_byte_length(s + t)").to_numpy(), strings_np.byte_length(strfn_np.cat(raw, other)))
    assert np.array_equal(df.evaluate("(str_slice(s, 1, 3) != 'Id') & (v > 2)").to_numpy(),
                          (np.array(strfn_np.slice_(raw, 1, 3), dtype=object) != "Id") & (v > 2))


def test_a_shared_source_is_transformed_once_per_evaluation(frame, monkeypatch):
    df, raw, other, v = frame
    calls = []
    lower = DeviceStringArray.lower
    monkeypatch.setattr(DeviceStringArray, "lower", lambda self: calls.append(len(self)) or lower(self))
    got = df.evaluate("str_startswith(str_lower(s), ' id00') | str_endswith(str_lower(s), 'é')", 100, 5100).to_numpy()
    low = strfn_np.lower(raw[100:5100])
    assert np.array_equal(got, strings_np.startswith(low, " id00") | strings_np.endswith(low, "é")) and got.any() and not got.all()
    assert calls == [5000]
    with pytest.raises(MemoryError):
        df.evaluate("str_len(str_repeat(s, 4611686018427387904))")


def test_evaluate_gives_string_columns_and_sub_ranges(frame):
    df, raw, other, v = frame
    out = df.evaluate("str_lower(s)")
    assert isinstance(out, DeviceStringArray) and df.data_type("str_lower(s)") == str and df.s.str.lower().dtype == str
    _same(out, strfn_np.lower(raw))
    for i1, i2 in ((0, 1), (1003, 4001), (20_000, 20_011), (77, 77)):
        _same(df.evaluate("str_slice(str_strip(s), 0, 3)", i1, i2), strfn_np.slice_(strfn_np.strip(raw[i1:i2]), 0, 3))
        _same(df.evaluate(df.s + "_" + df.t, i1, i2), strfn_np.cat(strfn_np.cat(raw[i1:i2], "_"), other[i1:i2]))
        _same(df.evaluate("k" + df.t, i1, i2), strfn_np.cat("k", other[i1:i2]))
    assert df.evaluate("str_cat('k', t)", 0, 9).tolist() == ["k" + o for o in other[:9]]
    assert df.evaluate(df.s.str.cat(df.t), 0, 9).tolist() == [a + b for a, b in zip(raw[:9], other[:9])]
    assert df.evaluate(df.t.str.zfill(3).str.replace("00", "x").str.center(5, "*").str.repeat(2), 0, 7).tolist() == \
        strfn_np.repeat(strfn_np.center(strfn_np.replace(strfn_np.zfill(other[:7], 3), "00", "x"), 5, "*"), 2)
    assert df.s.str.rstrip().str.upper().tolist()[:5] == strfn_np.upper(strfn_np.rstrip(raw[:5]))
    with pytest.raises(NotImplementedError):
        df.evaluate("str_lower(s) + 1")
    with pytest.raises(NotImplementedError):
        df.evaluate("str_lower(v)")


def test_string_virtual_column_and_keys(frame):
    df, raw, other, v = frame
    df = df.copy()
    df["k"] = df.s.str.strip().str.slice(0, 3)
    df["kt"] = df.k.str.lower() + df.t
    k = strfn_np.slice_(strfn_np.strip(raw), 0, 3)
    kt = strfn_np.cat(strfn_np.lower(k), other)
    assert df.data_type("k") == str and df.k.tolist() == k and df.evaluate("kt", 5, 50).tolist() == kt[5:50]
    assert np.array_equal(df.evaluate("k == 'ID0'").to_numpy(), np.array(k, dtype=object) == "ID0")
    for key, want in (("k", k), ("kt", kt), ("str_lower(s)", strfn_np.lower(raw))):
        for ascending in (False, True):
            vc = df.value_counts(key, ascending=ascending)
            keys, counts = strings_np.value_counts(want, ascending=ascending)
            assert vc.index.tolist() == keys and np.array_equal(vc.to_numpy(), counts), key
        assert df.unique(key) == strings_np.unique(want) and df[key].nunique() == len(set(want))
    # the codes of a key are kept while its sources are the same objects; a new source column drops them
    assert df.value_counts("k").index.tolist() == strings_np.value_counts(k)[0]
    df.columns["s"] = _col([r.replace("I", "J") for r in raw])
    k2 = strfn_np.slice_(strfn_np.strip([r.replace("I", "J") for r in raw]), 0, 3)
    assert df.value_counts("k").index.tolist() == strings_np.value_counts(k2)[0]
    taken = df.take(np.arange(100, 200))  # virtual columns carry over
    assert taken.k.tolist() == k2[100:200]


@pytest.mark.parametrize("sort", [False, True])
def test_groupby_a_transformed_key(frame, sort):
    df, raw, other, v = frame
    key = strfn_np.slice_(strfn_np.lower(strfn_np.strip(raw)), 0, 4)
    by = df.s.str.strip().str.lower().str.slice(0, 4)
    res = df.groupby(by, agg={"count": "count", "v_sum": vaex_amd.agg.sum("v")}, sort=sort)
    cols = {name: np.asarray(c) for name, c in res.columns.items()}
    assert set(cols) == {str(by), "count", "v_sum"}
    want = {}
    for s, x in zip(key, v.tolist()):
        e = want.setdefault(s, [0, 0])
        e[0] += 1
        e[1] += x
    got = {s: [int(c), int(t)] for s, c, t in zip(cols[str(by)].tolist(), cols["count"], cols["v_sum"])}
    assert got == want
    assert cols[str(by)].tolist() == (sorted(want) if sort else strings_np.unique(key))
    two = df.groupby([by, "t"], agg={"count": "count"}, sort=True)
    pairs = sorted(set(zip(key, other)))
    assert list(zip(np.asarray(two.columns[str(by)]).tolist(), np.asarray(two.columns["t"]).tolist())) == pairs


def test_sort_by_a_transformed_key(frame):
    df, raw, other, v = frame
    d2 = vaex_amd.from_arrays(s=df.columns["s"], t=df.columns["t"], row=DeviceArray.from_numpy(np.arange(len(raw))))
    for ascending in (True, False):
        got = d2.sort(d2.s.str.strip().str.upper(), ascending=ascending).row.to_numpy()
        assert np.array_equal(got, strings_np.argsort(strfn_np.upper(strfn_np.strip(raw)), ascending=ascending))
    got = d2.sort(["str_slice(s, 1, 4)", "row"]).row.to_numpy()
    assert np.array_equal(got, strings_np.lexsort([strfn_np.slice_(raw, 1, 4), np.arange(len(raw))]))


def test_refusals_through_expressions(frame):
    df, raw, other, v = frame
    with pytest.raises(NotImplementedError):
        df.evaluate("str_replace(s, 'a', 'b', regex=True)")
    with pytest.raises(NotImplementedError):
        df.s.str.replace("a", "b", regex=True)
    with pytest.raises(NotImplementedError):
        df.evaluate(df.s.str.strip("é"))
    with pytest.raises(ValueError):
        df.evaluate(df.s.str.pad(9, fillchar="éé"))
    with pytest.raises(ValueError):
        df.evaluate(df.s.str.replace("", "x"))
    with pytest.raises(NotImplementedError):
        df.evaluate("str_slice(s, 0, 6, 2)")  # no step
    with pytest.raises(NotImplementedError):
        df.groupby("str_strip(s, 'é')", agg="count")
