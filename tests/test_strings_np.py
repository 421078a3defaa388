"""tests/strings_np.py (the restatement the GPU string tests compare with) against pandas on the
edge strings, plus what needs no GPU of vaex_amd.strings: the offset promotion of a taken
column and the refusal of nulls."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import strings_np

EDGE = strings_np.edge_strings()
SHORT = [s for s in EDGE if len(s) < 1000]
PATTERNS = ["", "a", "ab", "aab", "\0", "a\0", "é", "€z", "f" * 7, "zz-not-there", "x" * 40]


def _series(col):
    return pd.Series(np.array(list(col), dtype=object))


def test_edge_strings_cover_the_cases():
    bl = strings_np.byte_length(EDGE)
    assert "" in EDGE and bl.max() == 70000
    starts = np.concatenate([[0], np.cumsum(bl)[:-1]])
    for length in range(18):
        assert {int(s) % 8 for s, b in zip(starts, bl) if b == length} >= set(range(8)), length
    assert any(strings_np.length([s])[0] != strings_np.byte_length([s])[0] for s in EDGE)
    assert {len(s.encode()) for s in ("é", "€", "\U0001d11e")} == {2, 3, 4}


def test_lengths():
    s = _series(EDGE)
    assert np.array_equal(strings_np.length(EDGE), s.str.len().to_numpy())
    assert np.array_equal(strings_np.byte_length(EDGE), s.str.encode("utf-8").str.len().to_numpy())


@pytest.mark.parametrize("pat", PATTERNS)
def test_predicates(pat):
    s = _series(EDGE)
    assert np.array_equal(strings_np.equals(EDGE, pat), (s == pat).to_numpy())
    assert np.array_equal(strings_np.notequals(EDGE, pat), (s != pat).to_numpy())
    assert np.array_equal(strings_np.startswith(EDGE, pat), s.str.startswith(pat).to_numpy(dtype=bool))
    assert np.array_equal(strings_np.endswith(EDGE, pat), s.str.endswith(pat).to_numpy(dtype=bool))
    assert np.array_equal(strings_np.contains(EDGE, pat), s.str.contains(pat, regex=False).to_numpy(dtype=bool))


def test_contains_overlap():
    assert strings_np.contains(["aaab", "aab", "ab", "xaab"], "aab").tolist() == [True, True, False, True]


def test_encode_is_factorize():
    # pandas' factorize hashes object strings as C strings: it ends them at the first NUL and so
    # merges "a", "a\0" and "a\0b".  It is the reference for the strings without a NUL; those
    # with one are checked against the definition itself below.
    col = [s for s in SHORT if "\0" not in s] * 3
    codes, keys = strings_np.encode(col)
    pcodes, pkeys = pd.factorize(_series(col))
    assert np.array_equal(codes, pcodes) and keys == list(pkeys)
    col = SHORT * 3
    codes, keys = strings_np.encode(col)
    assert len(keys) == len(set(col)) and [keys[c] for c in codes] == col
    assert all(col.index(k) < col.index(keys[i + 1]) for i, k in enumerate(keys[:-1]))  # first-appearance order
    # a second update goes on from the dictionary; absent strings map to -1
    more = ["new1", "a", "new2", "new1"]
    codes2, keys2 = strings_np.encode(more, keys)
    assert keys2[:len(keys)] == keys and keys2[len(keys):] == ["new1", "new2"]
    assert strings_np.map_ordinal(["a", "nope"], keys).tolist() == [keys.index("a"), -1]


@pytest.mark.parametrize("ascending", [False, True])
def test_value_counts_as_a_map(ascending):
    col = SHORT * 2 + SHORT[::3]
    keys, counts = strings_np.value_counts(col, ascending=ascending)
    want = _series(col).value_counts()
    assert dict(zip(keys, counts.tolist())) == want.to_dict()
    assert np.all(np.diff(counts) >= 0) if ascending else np.all(np.diff(counts) <= 0)
    # ties: ascending bytewise key order (reversed when descending)
    k2, c2 = strings_np.value_counts(col, ascending=not ascending)
    assert k2 == keys[::-1] and np.array_equal(c2, counts[::-1])


def test_sort_is_stable_sort_values():
    col = SHORT * 2
    order = strings_np.argsort(col)
    want = _series(col).sort_values(kind="stable").index.to_numpy()
    assert np.array_equal(order, want)
    assert np.array_equal(strings_np.argsort(col, ascending=False), want[::-1])
    # str order is the order of the UTF-8 bytes
    assert sorted(set(col)) == strings_np.bytewise_sorted(set(col))
    x = np.arange(len(col)) % 3
    assert np.array_equal(strings_np.lexsort([x, col]), np.lexsort([np.array(col, dtype=object), x]))


# ---- vaex_amd.strings without a GPU ----------------------------------------------------------------
def test_take_offset_promotion():
    from vaex_amd.strings import take_offset_dtype
    assert take_offset_dtype(np.int32, 2 ** 31 - 1) == np.int32
    assert take_offset_dtype(np.int32, 2 ** 31) == np.int64
    assert take_offset_dtype(np.int64, 0) == np.int64


def test_from_arrow_refuses_nulls():
    from vaex_amd.strings import DeviceStringArray
    for typ in (pa.string(), pa.large_string()):
        with pytest.raises(NotImplementedError, match="nulls"):
            DeviceStringArray.from_arrow(pa.array(["a", None, "b"], type=typ))
    with pytest.raises(NotImplementedError, match="nulls"):
        DeviceStringArray.from_arrow(pa.chunked_array([pa.array(["a"]), pa.array([None], type=pa.string())]))
    with pytest.raises(NotImplementedError, match="nulls"):
        DeviceStringArray.from_list(["a", None])


def test_string_type_marker():
    from vaex_amd.strings import STRING
    assert STRING == str and STRING.kind == "T" and not (STRING != str) and STRING != np.dtype("float64")
