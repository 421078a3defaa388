"""Datetime and timedelta functions for host frames (the reference's ``dt_*`` / ``td_*``,
functions.py), written with numpy unit casts instead of pandas so that host frames and the
device kernels (csrc/datetime_dev.hpp) share one definition: numpy's casts floor, before 1970
too.  Result dtypes are pandas 2's: the ``dt`` fields int32, ``is_leap_year`` bool,
``td_days`` int64, the other ``td`` fields int32, ``total_seconds`` float64.

``dt_weekofyear`` is the ISO-8601 week, pandas' ``dt.isocalendar().week``; the reference calls
``.dt.weekofyear``, which pandas 2 removed.  NaT rows are not supported (the device path
refuses such columns; here they give unspecified numbers).
"""
import numpy as np

_PER_DAY = {"ns": 86400 * 10 ** 9, "us": 86400 * 10 ** 6, "ms": 86400 * 10 ** 3, "s": 86400, "m": 1440, "h": 24, "D": 1}
_SECONDS_PER = {"s": 1, "m": 60, "h": 3600, "D": 86400}
_PER_SECOND = {"ns": 10 ** 9, "us": 10 ** 6, "ms": 10 ** 3, "s": 1}


def scalar_datetime(datetime_str):
    return np.datetime64(datetime_str)


def scalar_timedelta(amount, unit):
    return np.timedelta64(amount, unit)


def _i64(x):
    return x.astype(np.int64)


def _parts(x):
    x = np.asarray(x)
    if x.dtype.kind != "M":
        raise TypeError(f"a datetime64 value is needed, not {x.dtype}")
    unit = np.datetime_data(x.dtype)[0]
    if unit in _PER_DAY:
        # the day by an int64 floor division: numpy's own ns -> D cast overflows within a day of INT64_MIN
        D = (_i64(x) // _PER_DAY[unit]).astype("M8[D]")
    else:
        D = x.astype("M8[D]")
    return x, D.astype("M8[Y]"), D.astype("M8[M]"), D


def dt_year(x):
    return (_i64(_parts(x)[1]) + 1970).astype(np.int32)


def dt_month(x):
    x, Y, M, D = _parts(x)
    return (_i64(M) - _i64(Y.astype("M8[M]")) + 1).astype(np.int32)


def dt_day(x):
    x, Y, M, D = _parts(x)
    return (_i64(D) - _i64(M.astype("M8[D]")) + 1).astype(np.int32)


def dt_dayofweek(x):
    return ((_i64(_parts(x)[3]) + 3) % 7).astype(np.int32)  # 1970-01-01 is a Thursday; Monday = 0


def dt_dayofyear(x):
    x, Y, M, D = _parts(x)
    return (_i64(D) - _i64(Y.astype("M8[D]")) + 1).astype(np.int32)


def dt_quarter(x):
    return ((dt_month(x) - 1) // 3 + 1).astype(np.int32)


def dt_halfyear(x):
    return ((dt_quarter(x) - 1) // 2 + 1).astype(np.int32)


def _second_of_day(x):
    x, Y, M, D = _parts(x)
    if np.datetime_data(x.dtype)[0] in ("D", "W", "M", "Y"):
        return np.zeros(x.shape, np.int64)
    unit = np.datetime_data(x.dtype)[0]
    if unit in ("h", "m"):
        return (_i64(x) - _i64(D.astype(x.dtype))) * _SECONDS_PER[unit]
    return (_i64(x) - _i64(D) * _PER_DAY[unit]) // _PER_SECOND[unit]


def dt_hour(x):
    return (_second_of_day(x) // 3600).astype(np.int32)


def dt_minute(x):
    return (_second_of_day(x) // 60 % 60).astype(np.int32)


def dt_second(x):
    return (_second_of_day(x) % 60).astype(np.int32)


def dt_is_leap_year(x):
    y = _i64(_parts(x)[1]) + 1970
    return (y % 4 == 0) & ((y % 100 != 0) | (y % 400 == 0))


def dt_weekofyear(x):
    """The ISO-8601 week (pandas' ``dt.isocalendar().week``): the week of the year of the
    Thursday of the value's week."""
    days = _i64(_parts(x)[3])
    thursday = (days - (days + 3) % 7 + 3).astype("M8[D]")
    return ((_i64(thursday) - _i64(thursday.astype("M8[Y]").astype("M8[D]"))) // 7 + 1).astype(np.int32)


def _ticks(x):
    x = np.asarray(x)
    if x.dtype.kind != "m":
        raise TypeError(f"a timedelta64 value is needed, not {x.dtype}")
    unit = np.datetime_data(x.dtype)[0]
    if unit not in _PER_DAY:
        raise TypeError(f"timedelta fields of {x.dtype}: cast to a unit from ns to D first")
    return _i64(x), unit, _PER_DAY[unit]


def td_days(x):
    v, unit, per_day = _ticks(x)
    return v // per_day


def _ns_of_day(x):
    """(second of the day, nanoseconds below the second), both non-negative"""
    v, unit, per_day = _ticks(x)
    tod = v - (v // per_day) * per_day
    if unit in _PER_SECOND:
        pps = _PER_SECOND[unit]
        return tod // pps, tod % pps * (10 ** 9 // pps)
    return tod * (86400 // per_day), np.zeros(v.shape, np.int64)


def td_seconds(x):
    return _ns_of_day(x)[0].astype(np.int32)


def td_microseconds(x):
    return (_ns_of_day(x)[1] // 1000).astype(np.int32)


def td_nanoseconds(x):
    return (_ns_of_day(x)[1] % 1000).astype(np.int32)


def td_total_seconds(x):
    """pandas: the ticks divided by the ticks per second in float64; from a second up the
    exact integer of seconds, converted once."""
    v, unit, per_day = _ticks(x)
    if unit in _PER_SECOND:
        return v / _PER_SECOND[unit]
    return (v * _SECONDS_PER[unit]).astype(np.float64)


DT_NAMES = ["year", "month", "day", "dayofweek", "dayofyear", "quarter", "halfyear", "hour", "minute", "second",
            "is_leap_year", "weekofyear"]
TD_NAMES = ["days", "seconds", "microseconds", "nanoseconds", "total_seconds"]

# what the host expression namespace gets
FUNCTIONS = {"scalar_datetime": scalar_datetime, "scalar_timedelta": scalar_timedelta}
FUNCTIONS.update({"dt_" + n: globals()["dt_" + n] for n in DT_NAMES})
FUNCTIONS.update({"td_" + n: globals()["td_" + n] for n in TD_NAMES})


class _Accessor:
    """``df.t.dt.hour`` is the expression ``dt_hour(t)``, as the reference's accessors build it."""
    prefix, names = "", ()

    def __init__(self, expression):
        self.expression = expression

    def __getattr__(self, name):
        if name.startswith("_") or name not in self.names:
            raise AttributeError(name)
        return type(self.expression)(self.expression.df, f"{self.prefix}_{name}({self.expression.expression})")

    def __dir__(self):
        return list(self.names)


class DateTime(_Accessor):
    prefix, names = "dt", tuple(DT_NAMES)


class TimeDelta(_Accessor):
    prefix, names = "td", tuple(TD_NAMES)
