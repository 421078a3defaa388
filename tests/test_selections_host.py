"""The selection model on host frames, without a GPU: modes, history, folding, serialisation,
the geometric selectors and the lasso.  Restates the reference's test_selection_basics (minus
its "default | inverse" line: selection names inside expressions are out of scope),
test_selection_history, test_selection_serialize and test_lasso (tests/selection_test.py) with
the aggregations taken over ``evaluate_selection_mask`` (a host frame's count / sum stage
their chunks to the GPU; tests/test_gpu_select.py runs them)."""
import numpy as np
import pytest

from pnpoly_np import MODES, combine, pnpoly_np

X = np.arange(10.0)


@pytest.fixture
def df():
    import vaex_amd
    return vaex_amd.from_arrays(x=X.copy(), y=X ** 2, m=np.ma.array(X.copy(), mask=X == 9))


def mask(df, selection=True):
    return np.asarray(df.evaluate_selection_mask(selection, 0, len(X)))


def count(df, selection=True):
    return int(mask(df, selection).sum())


def total(df, selection=True):
    return X[mask(df, selection)].sum()


def test_selection_basics(df):
    from vaex_amd import selections
    df.select("x > 5")
    df.select("x <= 5", name="inverse")
    assert [count(df, s) for s in ["default", "inverse", "x > 5"]] == [4, 6, 4]
    df.select("x <= 1", name="inverse", mode="subtract")
    assert [count(df, s) for s in ["default", "inverse"]] == [4, 4]
    assert total(df) < X.sum()
    for mode in selections._select_functions:
        df.select("x > 5")
        df.select("x > 5", mode)  # the second positional argument is the mode
        df.select(None)
        df.select("x > 5", mode)
    df.select("x > 5")
    subset = total(df)
    df.select_inverse()
    inverse = total(df)
    df.select("x <= 5")
    assert inverse == total(df) and inverse + subset == X.sum()
    df.select("x > 5")
    df.select("x <= 5", name="inverse")
    df.select_inverse(name="inverse")
    assert [count(df, s) for s in ["default", "inverse"]] == [4, 4]


def test_selection_history(df):
    def state():
        return df.has_selection(), df.selection_can_undo(), df.selection_can_redo()

    assert state() == (False, False, False)
    df.select_nothing()  # a None on an empty history is not recorded
    assert state() == (False, False, False)
    df.select("x > 5")
    subset = total(df)
    assert subset < X.sum() and state() == (True, True, False)
    df.select("x < 7", mode="and")
    subset2 = total(df)
    assert subset2 < subset and state() == (True, True, False)
    df.selection_undo()
    assert total(df) == subset and state() == (True, True, True)
    df.selection_redo()
    assert total(df) == subset2 and state() == (True, True, False)
    df.selection_undo()
    df.selection_undo()
    assert state() == (False, False, True)
    df.selection_redo()
    assert state() == (True, True, True)
    df.select("x < 7", mode="and")  # clips the redo tail
    assert state() == (True, True, False) and total(df) == subset2
    df.select_nothing()
    assert state() == (False, True, False)
    df.selection_undo()
    assert state() == (True, True, True)
    with pytest.raises(ValueError):
        df.selection_undo(name="never used")
    # after undoing everything a new selection builds on nothing
    df.selection_undo()
    df.selection_undo()
    df.select("x < 2", mode="and")
    assert df.get_selection().previous_selection is None and count(df) == 2


def test_selection_serialize(df):
    from vaex_amd import selections
    selection_expression = selections.SelectionExpression("x > 5", None, "and")
    df.set_selection(selection_expression)
    subset = total(df)
    df.select("x > 5")
    assert total(df) == subset
    values = selection_expression.to_dict()
    assert values == dict(type="expression", boolean_expression="x > 5", mode="and", previous_selection=None)
    df.set_selection(selections.selection_from_dict(values))
    assert total(df) == subset
    lasso = selections.SelectionLasso("x", "y", [0, 10, 10, 0], [-1, -1, 100, 100], selection_expression, "and")
    df.set_selection(lasso)
    assert total(df) == subset
    assert total(df, lasso) == subset  # a Selection object as the selection= argument
    # every node type round-trips through to_dict / selection_from_dict
    chain = selections.SelectionDropNa(True, True, ["x", "m"], selections.SelectionInvert(lasso), "or")
    again = selections.selection_from_dict(chain.to_dict())
    assert again.to_dict() == chain.to_dict() and again.key() == chain.key()
    assert again.previous_selection.previous_selection.xseq == [0, 10, 10, 0]
    assert sorted(chain.dependencies()) == ["m", "x", "x", "x > 5", "y"]
    hash(chain.key())
    with pytest.raises(ValueError):
        selections.selection_from_dict(dict(type="polygon", previous_selection=None))


@pytest.mark.parametrize("mode", MODES)
def test_modes_and_folding(df, mode):
    p, n = X > 5, X < 7
    # without a previous selection
    df.select("x < 7", mode)
    np.testing.assert_array_equal(mask(df), combine(None, n, mode))
    assert df.selection_expressions == {"default": "~(x < 7)" if mode == "subtract" else "x < 7"}
    # with one
    df.select("x > 5")
    df.select("x < 7", mode=mode)
    np.testing.assert_array_equal(mask(df), combine(p, n, mode))
    folded = {"replace": "x < 7", "and": "(x > 5) & (x < 7)", "or": "(x > 5) | (x < 7)", "xor": "(x > 5) ^ (x < 7)",
              "subtract": "(x > 5) & ~(x < 7)"}[mode]
    assert df.selection_expressions == {"default": folded}
    assert df.get_selection().fold() == folded
    assert (df.get_selection().previous_selection is None) == (mode == "replace")
    df.select_inverse()
    assert df.selection_expressions == {"default": "~(%s)" % folded}
    np.testing.assert_array_equal(mask(df), ~combine(p, n, mode))
    # the same modes node by node: a lasso before it keeps the chain from folding
    df.select_lasso("x", "y", [-1, 6.5, 6.5, -1], [-1, -1, 50, 50])
    lasso = pnpoly_np(X, X ** 2, [-1, 6.5, 6.5, -1], [-1, -1, 50, 50])
    df.select("x < 3", mode=mode)
    assert (df.get_selection().fold() is None) == (mode != "replace")  # replace drops the lasso
    np.testing.assert_array_equal(mask(df), combine(lasso, X < 3, mode))
    df.select_inverse()
    np.testing.assert_array_equal(mask(df), ~combine(lasso, X < 3, mode))
    with pytest.raises(ValueError):
        df.select("x < 3", mode="nand")


def test_plain_select_is_the_expression_itself(df):
    """df.select(expr) folds to expr: the route, and on an HBM frame the mask-cache key and
    the kernels, of the one-string selection it replaces."""
    df.select("x < 3")
    assert df.selection_expressions == {"default": "x < 3"}
    assert df._resolve_selection(True) == "x < 3" and df._resolve_selection("default") == "x < 3"
    assert df._resolve_selection("x > 2") == "x > 2"  # not a name: an expression
    assert df._resolve_selection(df.x > 2) == "(x > 2)"
    df.select(df.x < 4, name="other")
    assert df.selection_expressions == {"default": "x < 3", "other": "(x < 4)"}
    df.select_lasso("x", "y", [0, 1, 1], [0, 0, 1], name="other")
    assert df.selection_expressions == {"default": "x < 3"}  # expression-only selections
    assert df._selection_dependencies() == ["x < 3", "x", "y"]
    df.select_nothing()
    assert df.selection_expressions == {} and not df.has_selection() and df.has_selection("other")
    with pytest.raises(ValueError):
        df.select_inverse()  # nothing to invert


def test_mode_combines_on_device_keep_mask_as_one_expression(monkeypatch):
    """An expression-only chain reaches the device evaluation as one string, together with
    the filter (stubbed evaluation: no GPU)."""
    import vaex_amd
    from vaex_amd.dataframe import DataFrame
    calls = []
    monkeypatch.setattr(DataFrame, "_eval_device", lambda self, expr, i1, i2: calls.append(expr) or object())
    monkeypatch.setattr(DataFrame, "is_device_resident", lambda self: True)
    df = vaex_amd.from_arrays(x=X, w=X / 10).filter("x > 0")
    df.select("w > 0.3")
    df.device_keep_mask(0, 10, True)
    df.select("w < 0.8", mode="and")
    df.select_inverse()
    df.device_keep_mask(0, 10, "default", invert=True)
    df.select_non_missing(column_names=["x", "w"], mode="and")
    df.evaluate_selection_mask(True, 0, 10)
    assert calls == ["(x > 0) & (w > 0.3)", "~((x > 0) & (~((w > 0.3) & (w < 0.8))))",
                     "(x > 0) & ((~((w > 0.3) & (w < 0.8))) & (~isnan(x) & ~isnan(w)))"]


def test_box_circle_ellipse(df):
    df.select_box(["x", "y"], [(7.5, 1), (50, 3.25)])
    np.testing.assert_array_equal(mask(df), (X >= 1) & (X <= 7.5) & (X ** 2 >= 3.25) & (X ** 2 <= 50))
    assert df.selection_expressions["default"] == \
        "((x) >= 1.000000) & ((x) <= 7.500000)&((y) >= 3.250000) & ((y) <= 50.000000)"
    df.select_rectangle(df.x, "y", [(2, 3), (0, 100)], mode="subtract")
    np.testing.assert_array_equal(mask(df), (X >= 1) & (X <= 7) & (X ** 2 >= 3.25) & ~((X >= 2) & (X <= 3)))
    xc, yc, r = 4.1, 16.3, 10.7
    d = (X - xc) ** 2 + (X ** 2 - yc) ** 2
    df.select_circle("x", "y", xc, yc, r)
    np.testing.assert_array_equal(mask(df), d <= r ** 2)
    assert repr(xc) in df.selection_expressions["default"] and repr(r ** 2) in df.selection_expressions["default"]
    df.select_circle("x", "y", 3, 9, 5, inclusive=False)  # row 4 lies at distance 7.07, row 3 at 0
    np.testing.assert_array_equal(mask(df), (X - 3) ** 2 + (X ** 2 - 9) ** 2 < 25)
    df.select_circle("x", "y", 0, 0, np.sqrt(2.0) ** 2 / 2 * 2, inclusive=True)
    assert count(df) == 2
    for angle, radians in [(0, False), (30, False), (0.4, True)]:
        for inclusive in (True, False):
            alpha = angle if radians else np.deg2rad(angle)
            width, height = 9.0, 40.0
            xr, yr = width / 2, height / 2
            rr = max(xr, yr)
            a, b = xr / rr, yr / rr
            lhs = ((X - xc) * np.cos(alpha) + (X ** 2 - yc) * np.sin(alpha)) ** 2 / a ** 2 + \
                ((X - xc) * np.sin(alpha) - (X ** 2 - yc) * np.cos(alpha)) ** 2 / b ** 2
            df.select_ellipse("x", "y", xc, yc, width, height, angle, radians=radians, inclusive=inclusive)
            np.testing.assert_array_equal(mask(df), lhs <= rr ** 2 if inclusive else lhs < rr ** 2)
            assert 0 < count(df) < 10


def test_lasso(df):
    """The reference's test_lasso: known sums, then the masked column m (row 9 masked)."""
    df.select_lasso("x", "y", [-0.1, 5.1, 5.1, -0.1], [-0.1, -0.1, 4.1, 4.1])
    assert total(df) == 0 + 1 + 2 and (X ** 2)[mask(df)].sum() == 0 + 1 + 4
    df.select_lasso("m", "y", [8 - 0.1, 9 + 0.1, 9 + 0.1, 8 - 0.1], [-0.1, -0.1, 1000, 1000])
    assert mask(df).tolist() == [False] * 8 + [True, False]
    df.select_lasso("x", "y", [8 - 0.1, 9 + 0.1, 9 + 0.1, 8 - 0.1], [-0.1, -0.1, 1000, 1000], mode="or")
    assert mask(df).tolist() == [False] * 8 + [True, True]
    # an integer column, an expression, an empty lasso
    df.add_column("k", np.arange(10, dtype=np.int32))
    df.select_lasso("k", "x * x", [-0.1, 5.1, 5.1, -0.1], [-0.1, -0.1, 4.1, 4.1])
    assert total(df) == 3
    df.select_lasso("x", "y", [], [])
    assert count(df) == 0
    with pytest.raises(ValueError):
        df.select_lasso("x", "y", [0, 1, 2], [0, 1])


def test_lasso_on_filtered_frame(df):
    """x / y are evaluated on the rows that pass the filter; the mask is over those rows."""
    dff = df.filter("x >= 2")
    dff.select("x < 8")
    dff.select_lasso("x", "y", [-0.1, 5.1, 5.1, -0.1], [-0.1, -0.1, 30, 30], mode="and")
    fm = dff.evaluate_filter_mask(0, 10)
    got = np.asarray(dff.evaluate_selection_mask(True, 0, 10, filter_mask=fm))
    keep = X >= 2
    want = (X < 8) & pnpoly_np(X, X ** 2, [-0.1, 5.1, 5.1, -0.1], [-0.1, -0.1, 30, 30])
    assert got.shape == (8,) and got.tolist() == want[keep].tolist() and got.sum() == 4
    assert not df.has_selection()  # filter() copied the frame first


def test_select_non_missing(df):
    df.add_column("f", np.where(X == 2, np.nan, X))
    df.select_non_missing()
    assert mask(df).tolist() == ((X != 2) & (X != 9)).tolist()
    df.select_non_missing(drop_nan=False, column_names=["f", "m"])
    assert mask(df).tolist() == (X != 9).tolist()
    df.select_non_missing(drop_masked=False, mode="subtract", column_names=["f"])
    assert mask(df).tolist() == ((X != 9) & (X == 2)).tolist()
    assert df.get_selection().fold(df) is None  # a host frame: node by node
    dff = df.filter("x > 0")
    dff.select_non_missing()
    assert np.asarray(dff.evaluate_selection_mask(True, 0, 10, filter_mask=X > 0)).tolist() == \
        ((X != 2) & (X != 9))[1:].tolist()


def test_selected_length_and_copy(df, monkeypatch):
    from vaex_amd.dataframe import DataFrame
    # count(selection=) over the mask: a host frame's count itself needs the GPU
    monkeypatch.setattr(DataFrame, "count", lambda self, selection=None: np.array(count(self, selection)))
    df.select("x > 5")
    df.select_lasso("x", "y", [6.5, 20, 20, 6.5], [0, 0, 70, 70], mode="subtract", name="second")
    assert df.selected_length() == 4 and df.selected_length("second") == 8
    df.select("x > 7", mode="and")
    df.selection_undo()
    dfc = df.copy()
    assert dfc.selection_can_redo() and dfc.selected_length() == 4 and dfc.selected_length("second") == 8
    dfc.selection_redo()
    dfc.select_nothing(name="second")
    assert dfc.selected_length() == 2 and not dfc.has_selection("second")
    assert df.selected_length() == 4 and df.has_selection("second")  # histories are not shared


def test_join_carries_selections_and_sees_lasso_columns():
    import vaex_amd
    from vaex_amd import join
    df = vaex_amd.from_arrays(x=X.copy(), y=X ** 2)
    df.select("x > 5")
    df.select_lasso("x", "y", [0, 1, 1], [0, 0, 1], name="lasso")
    new = join._like(df, dict(df.columns))
    assert new.selection_expressions == {"default": "x > 5"} and new.has_selection("lasso")
    new.select_nothing()
    assert df.has_selection()
    with pytest.raises(NotImplementedError, match="uses it"):
        join._rename(df, "y", "y_right")  # only the lasso uses y
