"""The numpy restatement of the datetime semantics (tests/dt_np.py) equals pandas 2 for every
field, unit and edge row, dtype included, and a stored known-answer file written once from
pandas (so the test still means something where pandas is absent)."""
import json
import os

import numpy as np
import pytest

import dt_np

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "dt_kats.json")


def _pandas_field(pd, name, x):
    s = pd.Series(x).dt
    if name == "weekofyear":
        return s.isocalendar().week.to_numpy().astype(np.int32)  # UInt32 there; the reference's .dt.weekofyear is gone
    if name == "halfyear":
        return ((s.quarter - 1) // 2 + 1).to_numpy()
    return getattr(s, name).to_numpy()


@pytest.mark.parametrize("unit", dt_np.UNITS)
def test_datetime_fields_equal_pandas(unit):
    pd = pytest.importorskip("pandas")
    x = dt_np.edge_datetimes(unit, 300)
    if unit == "ns":
        x = x[np.abs(x.astype(np.int64)) < dt_np.I64.max - 10 ** 12]  # pandas rejects ns near the int64 ends
    for name in dt_np.DT_FIELDS:
        want = _pandas_field(pd, name, x)
        got = dt_np.dt_field(name, x)
        if name != "weekofyear":
            assert got.dtype == want.dtype, (name, got.dtype, want.dtype)
        assert np.array_equal(got, want), (unit, name)


@pytest.mark.parametrize("unit", dt_np.UNITS)
def test_timedelta_fields_equal_pandas(unit):
    pd = pytest.importorskip("pandas")
    x = dt_np.edge_timedeltas(unit, 300)
    if unit == "ns":
        x = x[np.abs(x.astype(np.int64)) < dt_np.I64.max - 10 ** 12]
    s = pd.Series(x).dt
    for name in dt_np.TD_FIELDS:
        want = s.total_seconds().to_numpy() if name == "total_seconds" else getattr(s, name).to_numpy()
        got = dt_np.td_field(name, x)
        assert got.dtype == want.dtype, (name, got.dtype, want.dtype)
        assert np.array_equal(got, want), (unit, name)


def test_known_answers():
    with open(GOLDEN) as f:
        kats = json.load(f)
    assert len(kats["datetime"]) >= 40 and len(kats["timedelta"]) >= 10
    for unit, ticks, fields in kats["datetime"]:
        x = np.array([ticks], np.int64).view(f"M8[{unit}]")
        for name, want in fields.items():
            assert int(dt_np.dt_field(name, x)[0]) == want, (unit, ticks, name)
    for unit, ticks, fields in kats["timedelta"]:
        x = np.array([ticks], np.int64).view(f"m8[{unit}]")
        for name, want in fields.items():
            assert dt_np.td_field(name, x)[0] == want, (unit, ticks, name)


def test_minus_one_nanosecond():
    x = np.array([-1], "m8[ns]")
    assert [int(dt_np.td_field(n, x)[0]) for n in dt_np.TD_FIELDS[:4]] == [-1, 86399, 999999, 999]


def test_iso_weeks():
    days = np.array(["2016-01-03", "2018-12-31", "2020-12-31", "2021-01-03", "2021-01-04"], "M8[D]")
    assert dt_np.dt_field("weekofyear", days).tolist() == [53, 1, 53, 53, 1]
