"""Hand-worked frames for ``DataFrame.sort`` / ``extract`` (the reference's
dataframe.py:4216-4233,4420-4461), shared by tests/test_sort_np.py (which holds tests/sort_np.py
to them) and tests/test_gpu_sort.py (which holds the frames to them).  Every expectation is a
list of row numbers of FRAME, worked out by hand in the comments."""
import numpy as np

nan, inf = float("nan"), float("inf")

#  row      0     1     2     3     4     5     6     7
FRAME = dict(
    x=np.array([3.0, nan, 1.0, -0.0, 0.0, 1.0, inf, 2.0]),
    g=np.array([1, 0, 1, 0, 1, 0, 1, 0], dtype=np.int32),
    p=np.array([10, 11, 12, 13, 14, 15, 16, 17], dtype=np.int64),
    # a masked column has no HBM form: it stays on the host, the frame is mixed then
    h=np.ma.array(np.arange(8) * 1.5, mask=[0, 0, 1, 0, 0, 0, 1, 0]),
)

# (name, filter expression or None, by, ascending, expected rows)
SORT_CASES = [
    # -0.0 == 0.0 keep their order (3, 4), the two 1.0 keep theirs (2, 5), then 2, 3, inf, NaN last
    ("x", None, "x", True, [3, 4, 2, 5, 7, 0, 6, 1]),
    # the exact reverse: ties in reverse row order, NaN first
    ("x-desc", None, "x", False, [1, 6, 0, 7, 5, 2, 4, 3]),
    # p > 11 keeps rows 2..7: the same order without rows 0 and 1
    ("x-filtered", "p > 11", "x", True, [3, 4, 2, 5, 7, 6]),
    ("x-filtered-desc", "p > 11", "x", False, [6, 7, 5, 2, 4, 3]),
    # g = 0: rows 1, 3, 5, 7 with x = NaN, -0.0, 1, 2 -> 3, 5, 7, 1; g = 1: rows 0, 2, 4, 6 with
    # x = 3, 1, 0, inf -> 4, 2, 0, 6
    ("g-x", None, ["g", "x"], True, [3, 5, 7, 1, 4, 2, 0, 6]),
    ("g-x-desc", None, ["g", "x"], False, [6, 0, 2, 4, 1, 7, 5, 3]),
    # x first: the ties (3, 4) and (2, 5) are decided by g: g[3] = 0 < g[4] = 1, g[5] = 0 < g[2] = 1
    ("x-g", None, ("x", "g"), True, [3, 4, 5, 2, 7, 0, 6, 1]),
    # a one-key list is a lexsort of one key: the same stable order
    ("x-list", None, ["x"], True, [3, 4, 2, 5, 7, 0, 6, 1]),
    # g == 1 keeps rows 0, 2, 4, 6; by an expression: -x = -3, -1, -0.0, -inf -> 6, 0, 2, 4
    ("neg-x-filtered", "g == 1", "-x", True, [6, 0, 2, 4]),
    # a filter that keeps nothing, and one that keeps one row
    ("none-kept", "p > 99", "x", True, []),
    ("one-kept", "p == 13", ["g", "x"], False, [3]),
]

# (filter expression or None, expected rows)
EXTRACT_CASES = [
    (None, [0, 1, 2, 3, 4, 5, 6, 7]),
    ("p > 11", [2, 3, 4, 5, 6, 7]),
    ("g == 1", [0, 2, 4, 6]),
    ("x > 0", [0, 2, 5, 6, 7]),  # NaN compares false
    ("p > 99", []),
]

# The frame filtered by g == 1 keeps rows 0, 2, 4, 6.  The indices 3, 0, 0, 2 into its kept rows
# (``extract().take``) are rows 6, 0, 0, 4; the same indices as unfiltered row numbers with the
# filter kept (``take(filtered=False, dropfilter=False)``) are rows 3, 0, 0, 2, of which the
# filter hides the first (g[3] = 0).
TAKE_FILTER = "g == 1"
TAKE_INDICES = [3, 0, 0, 2]
TAKE_KEPT = [6, 0, 0, 4]
TAKE_VISIBLE = [1, 2, 3]


def keep_mask(expression):
    """The filter expressions above over FRAME, by hand."""
    if expression is None:
        return None
    x, g, p = FRAME["x"], FRAME["g"], FRAME["p"]
    with np.errstate(invalid="ignore"):
        return {"p > 11": p > 11, "g == 1": g == 1, "x > 0": x > 0, "p > 99": p > 99, "p == 13": p == 13}[expression]


def as_list(column):
    """A column (host, np.ma or DeviceArray) as a list: NaN as "nan", masked as None, and the
    sign of a zero kept."""
    if hasattr(column, "to_numpy"):
        column = column.to_numpy()
    mask = np.ma.getmaskarray(column) if np.ma.isMaskedArray(column) else np.zeros(len(column), bool)
    out = []
    for v, m in zip(np.ma.getdata(column).tolist(), mask.tolist()):
        if m:
            out.append(None)
        elif isinstance(v, float) and v != v:
            out.append("nan")
        elif isinstance(v, float) and v == 0:
            out.append("-0.0" if np.signbit(v) else "0.0")
        else:
            out.append(v)
    return out


def rows_of(rows):
    """FRAME's columns at the row numbers ``rows``, as lists."""
    rows = np.asarray(rows, dtype=np.int64)
    return {k: as_list(v[rows]) for k, v in FRAME.items()}
