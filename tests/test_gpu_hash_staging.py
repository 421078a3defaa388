"""Host columns longer than one staging chunk through the three hash engines.

A host column is copied to the device 2^24 rows at a time.  ``n = 2^24 + 1003`` is the smallest
size with a second chunk; everything that tells the second chunk from the first sits past row
2^24: keys 1000, 1001 and 1002 appear only there, the one null row and the one unselected row
too (the unselected row holds the only occurrence of key 1002).  A chunk loop that hands a
kernel the wrong keys, mask, select or counts pointer, or numbers the second chunk's rows from
the wrong row, changes an asserted value.  Every comparison against NumPy is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CH = 2 ** 24
N = CH + 1003
NULL_ROW = CH + 7
UNSELECTED_ROW = CH + 9


def su():
    import vaex_amd.superutils as m
    return m


@pytest.fixture(scope="module")
def col():
    """keys, mask, select and what NumPy makes of the visible rows; read-only."""
    keys = (np.arange(N, dtype=np.int64) % 1000).astype(np.int32)
    keys[CH + 1] = 1000
    keys[CH + 5] = 1001
    keys[CH + 500] = 1001
    keys[UNSELECTED_ROW] = 1002
    mask = np.zeros(N, np.uint8)
    mask[NULL_ROW] = 1
    select = np.ones(N, np.uint8)
    select[UNSELECTED_ROW] = 0
    regular = (select != 0) & (mask == 0)
    rows = np.flatnonzero(regular)
    uniq, first, counts = np.unique(keys[regular], return_index=True, return_counts=True)
    for a in (keys, mask, select):
        a.flags.writeable = False
    return dict(keys=keys, mask=mask, select=select, uniq=uniq, first_row=rows[first], counts=counts)


def test_ordered_set(col):
    s = su().ordered_set_int32()
    s.update(col["keys"], col["mask"], select=col["select"])
    # first-appearance order; the null entry takes the ordinal after the regular keys of the
    # update call that saw it (one call here), its key reads -1
    order = col["uniq"][np.argsort(col["first_row"], kind="stable")]
    assert order.tolist() == list(range(1002))
    exp = np.append(order, np.int32(-1))
    assert s.key_array().tolist() == exp.tolist()
    assert s.null_count == 1
    assert s.null_value == len(order)
    assert len(s) == len(exp) and s.length() == len(exp)
    assert s.nan_count == 0
    # map_ordinal of a host column that is itself longer than one chunk
    q = (np.arange(CH + 5, dtype=np.int64) % 1004).astype(np.int32)
    lookup = {int(k): o for o, k in enumerate(order.tolist())}
    table = np.array([lookup.get(k, -1) for k in range(1004)], np.int64)
    got = s.map_ordinal(q)
    assert got.dtype == np.int16
    assert np.array_equal(got.astype(np.int64), table[q])
    assert table[1002] == -1 and table[1003] == -1 and got[1002] == -1 and got[CH + 4] == table[q[CH + 4]]


def test_counter(col):
    m = su()
    c = m.counter_int32()
    c.update(col["keys"], col["mask"], select=col["select"])
    assert c.null_index == 0 and c.null_count == 1 and c.nan_count == 0
    exp_keys = np.insert(col["uniq"], c.null_index, 0)  # the null entry's key reads 0
    exp_counts = np.insert(col["counts"], c.null_index, 1)
    assert len(c) == len(exp_keys)
    assert c.key_array().tolist() == exp_keys.tolist()
    assert c.counts().tolist() == exp_counts.tolist()
    # counter(keys, counts): the counts column is staged in chunks next to the keys
    k2 = col["keys"][:CH + 3]
    r = m.counter_int32(k2, np.ones(len(k2), np.int64))
    uk, uc = np.unique(k2, return_counts=True)
    assert 1000 in uk.tolist()
    assert r.key_array().tolist() == uk.tolist()
    assert r.counts().tolist() == uc.tolist()
    assert r.null_count == 0 and r.null_index == -1
    u = m.counter_int32()
    u.update(k2)
    assert u.key_array().tolist() == r.key_array().tolist() and u.counts().tolist() == r.counts().tolist()


def test_index_hash(col):
    ix = su().index_hash_int32()
    ix.update(col["keys"], col["mask"], start_index=5, select=col["select"])
    exp = np.full(1004, -1, np.int64)
    exp[col["uniq"]] = col["first_row"] + 5
    assert exp[1000] == CH + 1 + 5 and exp[1001] == CH + 5 + 5
    got = ix.map_index(np.arange(1004, dtype=np.int32))
    assert got.dtype == np.int64 and got.tolist() == exp.tolist()
    assert got[1002] == -1 and got[1003] == -1
    assert ix.null_value == NULL_ROW + 5 and ix.null_count == 1
    assert ix.has_duplicates is True
    assert ix.nan_count == 0


def test_index_hash_float64_nan_rows(col):
    keys = col["keys"].astype(np.float64)
    keys[3] = np.nan
    keys[CH + 1] = np.nan
    ix = su().index_hash_float64()
    ix.update(keys)
    assert ix.nan_value == CH + 1
    assert ix.nan_count == 2
