"""The device expression compiler on datetime64 / timedelta64 columns (no GPU: programs are
compiled, not run) and the host-frame path of the same functions, end to end."""
import numpy as np
import pytest

import dt_np
import vaex_amd
from vaex_amd.expr import DT_OP, OP, Program, UnsupportedExpression

N = 64


def _frame():
    return vaex_amd.from_arrays(
        t=dt_np.edge_datetimes("ns", N), t2=dt_np.edge_datetimes("ns", N, seed=3), ts=dt_np.edge_datetimes("s", N),
        td=dt_np.edge_timedeltas("ns", N), tds=dt_np.edge_timedeltas("s", N), v=np.arange(N, dtype=np.int64))


def _np_ns(df):
    ns = {k: v for k, v in df.columns.items()}
    ns.update(np=np, astype=lambda x, d: x.astype(d), where=np.where, minimum=np.minimum, maximum=np.maximum)
    return ns


EXPRESSIONS = [
    "t2 - t", "t + td", "t - td", "td + td", "td - tds", "-td", "td * 3", "2 * td", "td // 7", "td // tds", "td / tds",
    "t < t2", "t <= ts", "t == t2", "t != t2", "ts > t", "td >= tds", "where(t < t2, t, t2)", "minimum(t, ts)",
    "maximum(td, tds)", "astype(t, 'datetime64[D]')", "astype(t, 'datetime64[M]')", "astype(ts, 'datetime64[ns]')",
    "astype(td, 'timedelta64[h]')", "astype(t, 'int64')", "astype(v, 'datetime64[s]')", "astype(td, 'int')",
    "t > np.datetime64('2015-06-01')", "t + np.timedelta64(90, 'm')", "(t2 - t) / np.timedelta64(1, 's')",
    "td // np.timedelta64(1, 'h')", "ts - ts",
]


@pytest.mark.parametrize("expression", EXPRESSIONS)
def test_result_dtype_is_numpys(expression):
    df = _frame()
    want = eval(expression, {"__builtins__": {}}, _np_ns(df))
    assert Program(df, expression).dtype == want.dtype, expression


def test_field_function_dtypes_and_fused_shape():
    df = _frame()
    for k, name in enumerate(dt_np.DT_FIELDS):
        p = Program(df, f"dt_{name}(t)")
        assert p.dtype == (np.bool_ if name == "is_leap_year" else np.int32)
        # COL DT_FIELD: the shape vh_expr_eval gives to the fused field kernel
        assert p.code == [OP["COL"], DT_OP["DT_FIELD"] | (k | 0 << 4) << 8]
    assert Program(df, "dt_hour(ts)").code[1] == DT_OP["DT_FIELD"] | (7 | 3 << 4) << 8
    want = {"days": np.int64, "seconds": np.int32, "microseconds": np.int32, "nanoseconds": np.int32,
            "total_seconds": np.float64}
    for name, dt in want.items():
        assert Program(df, f"td_{name}(td)").dtype == dt
    assert str(df.t.dt.hour) == "dt_hour(t)" and str(df.td.td.total_seconds) == "td_total_seconds(td)"


def test_date_filter_keeps_the_terms_shape():
    df = _frame()
    for e in ("t > np.datetime64('2015-06-01')", str(df.t > np.datetime64("2015-06-01", "ns")),
              "t > scalar_datetime('2015-06-01')"):
        p = Program(df, e)
        assert [c & 0xFF for c in p.code] == [OP["COL"], OP["CONST"], OP["GT_I"]], e
        assert p.consts == [int(np.datetime64("2015-06-01", "ns").astype(np.int64))]
    df.add_variable("t0", np.datetime64("1969-07-20", "D"))
    p = Program(df, "t >= t0")
    assert [c & 0xFF for c in p.code] == [OP["COL"], OP["CONST"], OP["GE_I"]]
    assert p.consts == [int(np.datetime64("1969-07-20", "ns").astype(np.int64)) & 0xFFFFFFFFFFFFFFFF]


def test_mixed_units_cast_the_coarser_side():
    df = _frame()
    cast = DT_OP["DT_CAST"] | (3 | 0 << 4) << 8  # s -> ns, datetime
    assert Program(df, "t < ts").code == [OP["COL"], OP["COL"] | 1 << 8, cast, OP["LT_I"]]
    assert Program(df, "ts - t").code == [OP["COL"], cast, OP["COL"] | 1 << 8, OP["SUB_I"]]
    tdcast = DT_OP["DT_CAST"] | (3 | 0 << 4 | 1 << 8) << 8
    assert Program(df, "td + tds").code == [OP["COL"], OP["COL"] | 1 << 8, tdcast, OP["ADD_I"]]


@pytest.mark.parametrize("expression", [
    "t > np.datetime64('NaT')", "t + t2", "astype(td, 'timedelta64[M]')", "astype(t, 'timedelta64[ns]')", "t * 2",
    "td * 1.5", "t < td", "-t", "~td", "~t", "dt_hour(td)", "td_days(t)", "sqrt(td)", "dt_year(astype(t, 'datetime64[M]'))"])
def test_refusals(expression):
    with pytest.raises(UnsupportedExpression):
        Program(_frame(), expression)


def test_masked_and_nat_columns_are_refused():
    t = dt_np.edge_datetimes("ns", N)
    df = vaex_amd.from_arrays(t=np.ma.array(t, mask=np.arange(N) % 2 == 0))
    with pytest.raises(UnsupportedExpression, match="masked"):
        Program(df, "dt_year(t)")
    t = t.copy()
    t[5] = np.datetime64("NaT")
    df = vaex_amd.from_arrays(t=t)
    with pytest.raises(UnsupportedExpression, match="NaT"):
        Program(df, "dt_year(t)")


@pytest.mark.parametrize("unit", dt_np.UNITS)
def test_host_frame_fields(unit):
    df = vaex_amd.from_arrays(t=dt_np.edge_datetimes(unit, 300), d=dt_np.edge_timedeltas(unit, 300))
    for name in dt_np.DT_FIELDS:
        got, want = getattr(df.t.dt, name).values, dt_np.dt_field(name, df.columns["t"])
        assert got.dtype == want.dtype and np.array_equal(got, want), (unit, name)
    for name in dt_np.TD_FIELDS:
        got, want = getattr(df.d.td, name).values, dt_np.td_field(name, df.columns["d"])
        assert got.dtype == want.dtype and np.array_equal(got, want), (unit, name)


def test_host_frame_expressions():
    df = _frame()
    m = df.evaluate("t > np.datetime64('2015-06-01')")
    assert np.array_equal(m, df.columns["t"] > np.datetime64("2015-06-01"))
    assert np.array_equal(df.evaluate("dt_hour(t + scalar_timedelta(90, 'm'))"),
                          dt_np.dt_field("hour", df.columns["t"] + np.timedelta64(90, "m")))
