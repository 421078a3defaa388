"""NumPy restatement of the device argsort (vaex_amd/csrc/sort.hip, sort_plan.hpp) and of
``DataFrame.sort`` / ``extract``, the yardstick of the GPU sort tests.

* ``code``: the order-preserving unsigned code of a key column and its NaN flags (unsigned
  integers as they are, signed integers with their sign bit flipped, floats with -0.0 folded
  to +0.0 and the sign-dependent flip in their own width, bool 0 / 1).
* ``key_range`` / ``plan``: per key (lo, hi, any NaN) over the sorted rows, then lo / span /
  width and the rounds: trailing keys while their widths sum to at most 64, the earliest key of
  a run in the highest bits; a round of at most 32 bits sorts 32-bit words, one of 0 bits
  sorts nothing.
* ``argsort_np``: the rounds themselves, each a stable sort of the packed words (NaN packs
  ``span``; descending: the first round reads the rows backwards and every round sorts the
  complement within its bits).  The result has to equal ``reference_order``.
* ``reference_order``: ``np.lexsort(keys[::-1])`` over the rows (one key:
  ``np.argsort(kind="stable")``), reversed for descending -- the reference's ``sort``
  (dataframe.py:4420-4461).
* ``sort_frame_np`` / ``extract_np``: the frame operations over dicts of columns.
"""
import numpy as np

MAX_KEYS = 16


def _native(values):
    values = np.ascontiguousarray(values)
    if values.dtype.kind in "mM":
        values = values.view(np.int64)
    return values


def code(values):
    """(uint64 codes, NaN flags); the code of a NaN row is meaningless."""
    v = _native(values)
    nan = np.isnan(v) if v.dtype.kind == "f" else np.zeros(len(v), bool)
    if v.dtype.kind == "b":
        return v.astype(np.uint64), nan
    if v.dtype.kind == "u":
        return v.astype(np.uint64), nan
    bits = 8 * v.dtype.itemsize
    U = np.dtype(f"u{v.dtype.itemsize}")
    top = U.type(1 << (bits - 1))
    if v.dtype.kind == "i":
        return (v.view(U) ^ top).astype(np.uint64), nan
    assert v.dtype.kind == "f"
    u = np.where(v == 0, v.dtype.type(0), v).view(U)  # -0.0 -> +0.0
    u = np.where(u & top, ~u, u | top)
    return u.astype(np.uint64), nan


def key_range(values, rows=None):
    """(lo, hi, any_nan) of the codes over ``rows`` (None: every row); lo > hi: no non-NaN row."""
    c, nan = code(values)
    if rows is not None:
        c, nan = c[rows], nan[rows]
    c = c[~nan]
    if not len(c):
        return 2 ** 64 - 1, 0, bool(nan.any())
    return int(c.min()), int(c.max()), bool(nan.any())


def plan(ranges, m):
    """(keys, rounds) of a list of (lo, hi, any_nan): keys as (lo, span, width), rounds in
    execution order as (key0, key1, bits, wide, shifts)."""
    keys = []
    for lo, hi, any_nan in ranges:
        if m > 0 and lo <= hi:
            span = hi - lo + (1 if any_nan else 0)
        else:
            lo, span = 0, 0
        assert span < 2 ** 64
        keys.append((lo, span, int(span).bit_length()))
    rounds = []
    end = len(keys)
    while end > 0:
        begin, total = end, 0
        while begin > 0 and total + keys[begin - 1][2] <= 64:
            begin -= 1
            total += keys[begin][2]
        shifts, at = [0] * (end - begin), 0
        for k in range(end - 1, begin - 1, -1):
            shifts[k - begin] = at
            at += keys[k][2]
        rounds.append((begin, end, total, total > 32, shifts))
        end = begin
    return keys, rounds


def plan_text(ranges, m):
    """The plan in the words of the check program (tests/host/sort_plan_check.hip)."""
    keys, rounds = plan(ranges, m)
    return ("keys " + " ".join(f"{lo}:{span}:{w}" for lo, span, w in keys) + " | rounds "
            + " ".join(f"{k0}-{k1}:{bits}:{'w64' if wide else 'w32'}:{','.join(map(str, sh))}"
                       for k0, k1, bits, wide, sh in rounds))


def argsort_np(keys, rows=None, ascending=True):
    """The device pipeline in NumPy: row numbers of the columns, in sorted order."""
    keys = [_native(k) for k in keys]
    n = len(keys[0])
    src = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    m = len(src)
    kplan, rounds = plan([key_range(k, src) for k in keys], m)
    codes = [code(k) for k in keys]
    perm = src if ascending else src[::-1]  # the first round reads the rows backwards when descending
    for k0, k1, bits, wide, shifts in rounds:
        if bits == 0:
            continue
        assert bits <= 64 and wide == (bits > 32)
        word = np.zeros(m, np.uint64)
        for k in range(k0, k1):
            lo, span, width = kplan[k]
            if not width:
                continue
            c, nan = codes[k][0][perm], codes[k][1][perm]
            rel = np.where(nan, np.uint64(span), c - np.uint64(lo))
            assert not len(rel) or int(rel.max()) <= span
            word |= rel << np.uint64(shifts[k - k0])
        field = np.uint64(2 ** bits - 1)
        assert not len(word) or int(word.max()) <= int(field)
        if not ascending:
            word = ~word & field
        perm = perm[np.argsort(word, kind="stable")]
    return perm


def reference_order(keys, rows=None, ascending=True):
    """np.lexsort / np.argsort(kind="stable") over the rows, reversed for descending."""
    keys = [_native(k) for k in keys]
    if rows is None:
        rows = np.arange(len(keys[0]), dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    sub = [k[rows] for k in keys]
    if len(sub) == 1:
        order = np.argsort(sub[0], kind="stable")
    else:
        order = np.lexsort(sub[::-1])
    if not ascending:
        order = order[::-1]
    return rows[order]


# ---- frames: dicts of columns (np.ma columns keep their masks), keep = the filter's mask or None ---
def _take_columns(columns, rows):
    return {k: v[rows] for k, v in columns.items()}


def sort_frame_np(columns, by, keep=None, ascending=True):
    """``sort``: the kept rows in the order of the key columns ``by`` (names), the filter dropped."""
    by = [by] if isinstance(by, str) else list(by)
    rows = None if keep is None else np.flatnonzero(keep)
    order = reference_order([np.ma.getdata(columns[b]) for b in by], rows, ascending)
    return _take_columns(columns, order)


def extract_np(columns, keep=None):
    """``extract``: the kept rows, the filter dropped."""
    if keep is None:
        return dict(columns)
    return _take_columns(columns, np.flatnonzero(keep))
