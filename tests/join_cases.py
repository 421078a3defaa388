"""Hand-worked join cases shared by tests/test_join_np.py (the NumPy restatement, CPU) and
tests/test_gpu_join.py (DataFrame.join on host and HBM frames).  Each expected result was
worked out by hand from the cited lines of the reference (packages/vaex-core/vaex/join.py,
packages/vaex-core/src/hash_primitives.hpp); None marks a masked entry.

A case: left / right columns, join keyword arguments, optional filter expressions, and either
``expect`` (name -> values over ALL rows of the result, in column order) with ``visible`` (the
rows the left frame's filter keeps, None = all), or ``raises`` (exception, message part)."""
import numpy as np

NAN = np.nan

LEFT = dict(x=np.array([1, 2, 5], np.int64), a=np.array([1.0, 2.0, 3.0]))
RIGHT = dict(x=np.array([2, 1, 7], np.int64), b=np.array([10, 20, 30], np.int32))

CASES = {
    # x=1 is right row 1, x=2 right row 0, x=5 is unknown: -1, so the columns are taken masked
    # (map_index hash_primitives.hpp:679-714, take(masked=any(lookup_masked)) join.py:283)
    "left_unmatched": dict(left=LEFT, right=RIGHT, kw=dict(on="x"),
                           expect=dict(x=[1, 2, 5], a=[1.0, 2.0, 3.0], b=[20, 10, None])),
    # keys 1.0 -> row 2; NaN -> nan_value 0 (:697-699); masked -> null_value 1 (:737-739); 3.0 -> -1
    "null_and_nan_keys": dict(
        left=dict(k=np.ma.array([1.0, NAN, 2.0, 3.0], mask=[0, 0, 1, 0]), a=np.array([1, 2, 3, 4], np.int16)),
        right=dict(k=np.ma.array([NAN, 5.0, 1.0, 9.0], mask=[0, 1, 0, 0]), v=np.array([100, 200, 300, 400], np.int64)),
        kw=dict(on="k"),
        expect=dict(k=[1.0, NAN, None, 3.0], a=[1, 2, 3, 4], v=[300, 100, 200, None])),
    # right key 2 is at rows 0, 2, 3: first row 0, overflow [2, 3] (add_existing :668-674);
    # left row 1 gets the extra pairs (1, 2), (1, 3) (:756-848), appended after the original
    # rows (left.concat(left.take(lookup_left)), join.py:208-213)
    "duplicates": dict(
        left=dict(x=np.array([1, 2, 3], np.int32), a=np.array([10, 20, 30], np.int64)),
        right=dict(x=np.array([2, 1, 2, 2], np.int32), b=np.array([1.0, 2.0, 3.0, 4.0])),
        kw=dict(on="x", allow_duplication=True),
        expect=dict(x=[1, 2, 3, 2, 2], a=[10, 20, 30, 20, 20], b=[2.0, 1.0, None, 3.0, 4.0])),
    "duplicates_refused": dict(  # join.py:172-173
        left=dict(x=np.array([1, 2, 3], np.int32)), right=dict(x=np.array([2, 1, 2, 2], np.int32), b=np.arange(4.0)),
        kw=dict(on="x"), raises=(ValueError, "duplication of rows")),
    # inner keeps the matched rows only, nothing is masked (join.py:215-220)
    "inner": dict(left=LEFT, right=RIGHT, kw=dict(on="x", how="inner"),
                  expect=dict(x=[1, 2], a=[1.0, 2.0], b=[20, 10])),
    # right swaps the sides (join.py:136-140): the right frame's rows, the left's columns taken
    "right": dict(left=LEFT, right=RIGHT, kw=dict(on="x", how="right"),
                  expect=dict(x=[2, 1, 7], b=[10, 20, 30], a=[2.0, 1.0, None])),
    # both frames have x and y; the right's get the suffix, and x_r != left_on is added too
    # (join.py:229-253, 259-262)
    "suffix": dict(
        left=dict(x=np.array([1, 2], np.int64), y=np.array([5.0, 6.0])),
        right=dict(x=np.array([2, 1], np.int64), y=np.array([7.0, 8.0])),
        kw=dict(on="x", rsuffix="_r"), expect=dict(x=[1, 2], y=[5.0, 6.0], x_r=[1, 2], y_r=[8.0, 7.0])),
    "prefix": dict(
        left=dict(x=np.array([1, 2], np.int64), y=np.array([5.0, 6.0])),
        right=dict(x=np.array([2, 1], np.int64), y=np.array([7.0, 8.0])),
        kw=dict(on="x", lprefix="l_", rprefix="r_"),
        expect=dict(l_x=[1, 2], l_y=[5.0, 6.0], r_x=[1, 2], r_y=[8.0, 7.0])),
    "collision": dict(  # join.py:155-157
        left=dict(x=np.array([1, 2], np.int64), y=np.array([5.0, 6.0])),
        right=dict(x=np.array([2, 1], np.int64), y=np.array([7.0, 8.0])),
        kw=dict(on="x"), raises=(ValueError, "column name collision: y")),
    # the right frame's filter b > 10 leaves rows 1 (x=1) and 2 (x=7) in the index, under their
    # unfiltered row numbers (right.extract(), join.py:159, without the compaction)
    "filtered_right": dict(left=LEFT, right=RIGHT, right_filter="b > 10", kw=dict(on="x"),
                           expect=dict(x=[1, 2, 5], a=[1.0, 2.0, 3.0], b=[20, None, None])),
    # the lookup covers all unfiltered left rows (ignore_filter=True, join.py:207); the left
    # frame's filter a > 1.5 stays on the result and shows rows 1 and 2
    "filtered_left": dict(left=LEFT, right=RIGHT, left_filter="a > 1.5", kw=dict(on="x"),
                          expect=dict(x=[1, 2, 5], a=[1.0, 2.0, 3.0], b=[20, 10, None]), visible=[1, 2]),
    # different key names; the right's key column is an ordinary column of the result
    "left_on_right_on": dict(
        left=dict(i=np.array([3, 4], np.uint8)), right=dict(j=np.array([4, 3], np.uint8), w=np.array([1.5, 2.5], np.float32)),
        kw=dict(left_on="i", right_on="j"), expect=dict(i=[3, 4], j=[3, 4], w=[2.5, 1.5])),
    # no key: a row-wise merge (join.py:163-164, 279-284)
    "row_wise": dict(left=dict(a=np.array([1, 2, 3], np.int8)), right=dict(b=np.array([4.0, 5.0, 6.0])), kw={},
                     expect=dict(a=[1, 2, 3], b=[4.0, 5.0, 6.0])),
}


def as_list(column):
    """A column (host, masked or HBM) as a list, None for masked entries, NaN as 'nan'."""
    if hasattr(column, "to_numpy"):
        column = column.to_numpy()
    out = np.ma.asarray(column).tolist()
    return ["nan" if isinstance(v, float) and v != v else v for v in out]


def expected_list(values):
    return ["nan" if isinstance(v, float) and v != v else v for v in values]


def filter_array(columns, expression):
    return None if expression is None else np.asarray(eval(expression, {"__builtins__": {}}, dict(columns)), bool)
