"""numpy restatement of the datetime / timedelta semantics the device kernels pin (DESIGN.md
5.24), the edge columns and the expression lists shared by the datetime tests.

Fields come from ``astype('M8[Y]')`` / ``'M8[M]'`` / ``'M8[D]'`` arithmetic (numpy's casts
floor, before 1970 too), the ISO week from the Thursday rule, timedelta fields from floor
division; dtypes are pandas 2's.  tests/test_dt_np.py checks all of it against pandas and a
stored known-answer file.
"""
import numpy as np

UNITS = ["ns", "us", "ms", "s", "m", "h", "D"]        # column units
CAST_UNITS = UNITS + ["W", "M", "Y"]
UNIT_CODE = {u: i for i, u in enumerate(CAST_UNITS)}  # csrc/datetime_dev.hpp Unit
DT_FIELDS = ["year", "month", "day", "dayofweek", "dayofyear", "quarter", "halfyear", "hour", "minute", "second",
             "is_leap_year", "weekofyear"]            # in the order of datetime_dev.hpp Field
TD_FIELDS = ["days", "seconds", "microseconds", "nanoseconds", "total_seconds"]
PER_DAY = {"ns": 86400 * 10 ** 9, "us": 86400 * 10 ** 6, "ms": 86400 * 10 ** 3, "s": 86400, "m": 1440, "h": 24, "D": 1}
PER_SECOND = {"ns": 10 ** 9, "us": 10 ** 6, "ms": 10 ** 3, "s": 1}
I64 = np.iinfo(np.int64)

_EDGE_DATES = [
    "1970-01-01T00:00:00", "1969-12-31T23:59:59", "1970-01-01T23:59:59", "1970-01-02T00:00:00",
    "1969-12-31T00:00:00", "1969-12-30T23:59:59", "2015-06-01T00:00:00", "2015-05-31T23:59:59",
    "1900-02-28T12:00:00", "1900-03-01T00:00:00", "2000-02-29T23:59:59", "2100-02-28T00:00:00", "2100-03-01T06:30:15",
    "2015-12-31T23:59:59", "2016-01-01T00:00:00", "2016-12-31T11:11:11", "2017-01-01T00:00:00", "1968-12-31T01:02:03",
    "1969-01-01T00:00:00", "2016-01-03T10:00:00", "2018-12-31T10:00:00", "2020-12-31T10:00:00", "2021-01-03T10:00:00",
    "2021-01-04T10:00:00", "1972-02-29T00:00:00", "1968-02-29T13:14:15",
]


def edge_datetimes(unit, n=0, seed=7):
    """The edge column of a unit as datetime64[unit], filled with seeded random dates of
    1600..2250 (within every unit's range) up to n rows."""
    vals = [np.datetime64(d).astype(f"M8[{unit}]").astype(np.int64) for d in _EDGE_DATES]
    vals += [-1, 0, 1]
    if PER_DAY[unit] > 1:
        vals += [PER_DAY[unit] - 1, PER_DAY[unit], -PER_DAY[unit], -PER_DAY[unit] - 1, -PER_DAY[unit] + 1]
    if unit == "ns":
        vals += [I64.min + 1, I64.max]
    if unit in ("s", "m", "h", "D"):
        vals += [np.datetime64("0001-01-01T00:00:00").astype(f"M8[{unit}]").astype(np.int64),
                 np.datetime64("9999-12-31T23:59:59").astype(f"M8[{unit}]").astype(np.int64)]
    vals = np.array(vals, np.int64)
    if n > len(vals):
        rng = np.random.default_rng(seed + UNITS.index(unit))
        lo, hi = -135140 * PER_DAY[unit], 102268 * PER_DAY[unit]  # 1600-01-01 .. 2250-01-01
        if unit == "ns":
            lo, hi = I64.min + 1, I64.max
        vals = np.concatenate([vals, rng.integers(lo, hi, n - len(vals), dtype=np.int64)])
    return vals.view(f"M8[{unit}]")


def edge_timedeltas(unit, n=0, seed=11):
    day = PER_DAY[unit]
    vals = [0, 1, -1, day, -day, day - 1, -day + 1, day + 1, -day - 1, 90061 * PER_SECOND.get(unit, 1) + 1,
            -90061 * PER_SECOND.get(unit, 1) - 1, 1001, -1001, 999999999, -999999999, 1000000001]
    if unit == "ns":
        vals += [I64.min + 1, I64.max]
    vals = np.array(vals, np.int64)
    if n > len(vals):
        rng = np.random.default_rng(seed + UNITS.index(unit))
        span = min(I64.max, 400000 * day)
        vals = np.concatenate([vals, rng.integers(-span, span, n - len(vals), dtype=np.int64)])
    return vals.view(f"m8[{unit}]")


def dt_field(name, x):
    """The datetime field ``name`` of a datetime64 array, with pandas 2's dtype."""
    x = np.asarray(x)
    unit = np.datetime_data(x.dtype)[0]
    # the day by an int64 floor division: numpy's own ns -> D cast overflows within a day of
    # INT64_MIN (it biases the dividend); from the day on its casts are exact
    days = x.astype(np.int64) // PER_DAY[unit]
    D = days.astype("M8[D]")
    Y, M = D.astype("M8[Y]"), D.astype("M8[M]")
    y = Y.astype(np.int64) + 1970
    month = (M - Y.astype("M8[M]")).astype(np.int64) + 1
    if unit in ("D",):
        sod = np.zeros(x.shape, np.int64)
    else:
        sod = (x.astype(np.int64) - days * PER_DAY[unit])  # ticks within the day, floor semantics
        sod = sod // PER_SECOND[unit] if unit in PER_SECOND else sod * (86400 // PER_DAY[unit])
    dow = (days + 3) % 7
    if name == "year":
        r = y
    elif name == "month":
        r = month
    elif name == "day":
        r = (D - M.astype("M8[D]")).astype(np.int64) + 1
    elif name == "dayofweek":
        r = dow
    elif name == "dayofyear":
        r = (D - Y.astype("M8[D]")).astype(np.int64) + 1
    elif name == "quarter":
        r = (month - 1) // 3 + 1
    elif name == "halfyear":
        r = ((month - 1) // 3) // 2 + 1
    elif name == "hour":
        r = sod // 3600
    elif name == "minute":
        r = sod // 60 % 60
    elif name == "second":
        r = sod % 60
    elif name == "is_leap_year":
        return (y % 4 == 0) & ((y % 100 != 0) | (y % 400 == 0))
    elif name == "weekofyear":
        # ISO-8601: the week belongs to the year of its Thursday; week 1 holds the first Thursday
        thursday = (days - dow + 3).astype("M8[D]")
        r = (thursday - thursday.astype("M8[Y]").astype("M8[D]")).astype(np.int64) // 7 + 1
    else:
        raise KeyError(name)
    return r.astype(np.int32)


def td_field(name, x):
    """The timedelta field ``name`` of a timedelta64 array, pandas' definitions and dtypes."""
    x = np.asarray(x)
    unit = np.datetime_data(x.dtype)[0]
    v = x.astype(np.int64)
    day = PER_DAY[unit]
    days = v // day
    tod = v - days * day
    if unit in PER_SECOND:
        sec, sub_ns = tod // PER_SECOND[unit], tod % PER_SECOND[unit] * (10 ** 9 // PER_SECOND[unit])
    else:
        sec, sub_ns = tod * (86400 // day), np.zeros(v.shape, np.int64)
    if name == "days":
        return days
    if name == "seconds":
        return sec.astype(np.int32)
    if name == "microseconds":
        return (sub_ns // 1000).astype(np.int32)
    if name == "nanoseconds":
        return (sub_ns % 1000).astype(np.int32)
    if name == "total_seconds":
        # pandas: asi8 / periods_per_second (a float64 true division); pandas stores units above
        # the second as seconds, an exact integer converted once
        return v / PER_SECOND[unit] if unit in PER_SECOND else (v * (86400 // day)).astype(np.float64)
    raise KeyError(name)


def cast_pairs(kind):
    """(from, to) unit pairs numpy casts between for datetime64 ('M') / timedelta64 ('m')."""
    out = []
    for a in CAST_UNITS:
        for b in CAST_UNITS:
            if a == b or (kind == "m" and ((a in "MY") != (b in "MY"))):
                continue
            out.append((a, b))
    return out


def castable(x, to):
    """The rows of a datetime64 / timedelta64 array whose cast to unit ``to`` stays well inside
    int64 and inside years 0001..9999 (overflowing casts are not pinned)."""
    kind = x.dtype.kind
    frm = np.datetime_data(x.dtype)[0]
    v = x.astype(np.int64).astype(object)
    approx_ns = {"ns": 1, "us": 10 ** 3, "ms": 10 ** 6, "s": 10 ** 9, "m": 6 * 10 ** 10, "h": 36 * 10 ** 11,
                 "D": 864 * 10 ** 11, "W": 6048 * 10 ** 11, "M": 31 * 864 * 10 ** 11, "Y": 366 * 864 * 10 ** 11}
    ns = v * approx_ns[frm]
    ok = np.array([abs(t) // approx_ns[to] < 2 ** 62 for t in ns])
    # numpy's flooring cast biases the dividend: it overflows within one target tick of the int64 ends
    ok &= np.array([abs(t) < 2 ** 63 - max(1, approx_ns[to] // approx_ns[frm]) for t in v])
    if kind == "M":
        ok &= np.array([-62135596800 * 10 ** 9 <= t < 253402300800 * 10 ** 9 - approx_ns[frm] * 12 for t in ns])
    return x[ok]
