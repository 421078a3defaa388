"""datetime64 / timedelta64 expressions on HBM frames: the dt / td field functions through the
fused field kernel, the interpreter and the element-wise (misaligned) path, unit casts,
arithmetic and comparisons, NaT refusal, groupby keys, BinnerTime and minmax -- each against
the numpy restatement (tests/dt_np.py) or numpy itself, bit for bit, dtype included."""
import numpy as np
import pytest

import dt_np
import vaex_amd
from vaex_amd import DeviceArray

pytestmark = pytest.mark.gpu

N = 2051  # more than one 2048-row block of the 8-rows-per-lane kernel and one 1024-row interpreter block, ragged
GPU_UNITS = ["ns", "us", "ms", "s", "D"]


def _dev(**cols):
    return vaex_amd.from_arrays(**{k: DeviceArray.from_numpy(np.ascontiguousarray(v)) for k, v in cols.items()})


def _same(got, want, what):
    assert isinstance(got, DeviceArray), what
    got = got.to_numpy()
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (what, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("route", ["fused", "interpreter", "misaligned"])
@pytest.mark.parametrize("unit", GPU_UNITS)
def test_datetime_fields(unit, route, monkeypatch):
    if route == "interpreter":
        monkeypatch.setenv("VH_EXPR_DTFIELD", "0")
    t = dt_np.edge_datetimes(unit, N)
    df = _dev(t=t)
    i1 = 1 if route == "misaligned" else 0
    for name in dt_np.DT_FIELDS:
        _same(df.evaluate(f"dt_{name}(t)", i1, N), dt_np.dt_field(name, t[i1:]), (unit, route, name))


@pytest.mark.parametrize("unit", GPU_UNITS)
def test_timedelta_fields(unit):
    d = dt_np.edge_timedeltas(unit, N)
    df = _dev(d=d)
    for name in dt_np.TD_FIELDS:
        _same(df.evaluate(f"td_{name}(d)"), dt_np.td_field(name, d), (unit, name))
    if unit == "ns":
        one = _dev(d=np.array([-1] * 3, "m8[ns]"))
        assert [int(one.evaluate(f"td_{n}(d)").to_numpy()[0]) for n in dt_np.TD_FIELDS[:4]] == [-1, 86399, 999999, 999]


@pytest.mark.parametrize("kind", ["M", "m"])
def test_casts(kind):
    for a, b in dt_np.cast_pairs(kind):
        if a in dt_np.UNITS:
            x = dt_np.edge_datetimes(a, 300) if kind == "M" else dt_np.edge_timedeltas(a, 300)
        else:
            x = np.concatenate([np.arange(-60, 60), [-23000, 23000]]).astype(np.int64).view(f"{kind}8[{a}]")
        x = dt_np.castable(x, b)
        name = ("datetime64" if kind == "M" else "timedelta64") + f"[{b}]"
        _same(_dev(x=x).evaluate(f"astype(x, {name!r})"), x.astype(name), (kind, a, b))


def test_arithmetic_and_comparisons():
    t1, t2 = dt_np.edge_datetimes("us", N, seed=1), dt_np.edge_datetimes("us", N, seed=2)
    ts, tn = dt_np.edge_datetimes("s", N, seed=3), dt_np.edge_datetimes("ns", N, seed=4)
    tn = np.clip(tn.astype(np.int64), -2 ** 62, 2 ** 62).view("M8[ns]")
    td = t2 - t1
    df = _dev(t1=t1, t2=t2, ts=ts, tn=tn, td=td, v=np.arange(N, dtype=np.float64))
    with np.errstate(all="ignore"):
        cases = {
            "t2 - t1": t2 - t1, "t1 + np.timedelta64(90, 'm')": t1 + np.timedelta64(90, "m"),
            "(t2 - t1) / np.timedelta64(1, 's')": (t2 - t1) / np.timedelta64(1, "s"),
            "td // np.timedelta64(1, 'h')": td // np.timedelta64(1, "h"), "ts < tn": ts < tn, "tn - ts": tn - ts,
            "-td": -td, "td * 3": td * 3, "td // 7": td // 7, "minimum(t1, t2)": np.minimum(t1, t2),
            "where(t1 < t2, t1, t2)": np.where(t1 < t2, t1, t2), "astype(td, 'int')": td.astype(np.int64),
            "dt_hour(t1 + scalar_timedelta(90, 'm'))": dt_np.dt_field("hour", t1 + np.timedelta64(90, "m")),
        }
    for e, want in cases.items():
        _same(df.evaluate(e), want, e)
    c = np.datetime64("2015-06-01")
    assert len(df[df.t1 > c]) == int((t1 > c).sum())
    df.select(df.t1 <= np.datetime64("1969-12-31T23:59:59"))
    assert int(df.count(selection=True)) == int((t1 <= np.datetime64("1969-12-31T23:59:59")).sum())
    assert float(df.sum("v", selection="t1 > scalar_datetime('2015-06-01')")) == float(df.columns["v"].to_numpy()[t1 > c].sum())


def test_nat_is_refused():
    t1 = dt_np.edge_datetimes("ns", N)
    t2 = t1.copy()
    t2[1000] = np.datetime64("NaT")
    df = _dev(t1=t1, t2=t2)
    _same(df.evaluate("dt_year(t1)"), dt_np.dt_field("year", t1), "no NaT next to INT64_MIN + 1")
    for e in ("dt_year(t2)", "t2 - t1"):
        with pytest.raises(NotImplementedError, match="NaT"):
            df.evaluate(e)


def _days_frame():
    rng = np.random.default_rng(5)
    t = (np.datetime64("1968-01-01T00:00:00", "s") + rng.integers(0, 5 * 366 * 86400, N).astype("m8[s]")).astype("M8[s]")
    t[:4] = np.array(["1968-01-01T00:00:00", "1972-12-31T23:59:59", "1968-02-29T12:00:00", "1969-12-31T23:59:59"], "M8[s]")
    return t, rng.integers(0, 100, N)


def test_groupby_field_keys():
    t, v = _days_frame()
    df = _dev(t=t, v=v)
    r = df.groupby(df.t.dt.hour, agg={"n": "count", "s": vaex_amd.agg.sum("v")})
    hour = dt_np.dt_field("hour", t)
    keys = np.asarray(r.columns["dt_hour(t)"])
    order = np.argsort(keys)
    assert np.array_equal(keys[order], np.flatnonzero(np.bincount(hour)))
    assert np.array_equal(np.asarray(r.columns["n"])[order], np.bincount(hour)[np.bincount(hour) > 0])
    assert np.array_equal(np.asarray(r.columns["s"])[order], np.bincount(hour, weights=v).astype(np.int64)[np.bincount(hour) > 0])
    r = df.groupby([df.t.dt.dayofweek, df.t.dt.month], agg={"n": "count"})
    dow, month = dt_np.dt_field("dayofweek", t), dt_np.dt_field("month", t)
    want = np.bincount(dow.astype(np.int64) * 13 + month, minlength=7 * 13)
    got = np.zeros(7 * 13, np.int64)
    got[np.asarray(r.columns["dt_dayofweek(t)"]).astype(np.int64) * 13 + np.asarray(r.columns["dt_month(t)"])] = r.columns["n"]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("how", ["per_day", "per_week", "per_month", "per_quarter", "per_year"])
def test_binner_time(how):
    t, v = _days_frame()
    df = _dev(t=t, v=v)
    r = df.groupby(getattr(vaex_amd.BinnerTime, how)(df.t), agg={"n": "count", "s": vaex_amd.agg.sum("v")})
    res, every = {"per_day": ("D", 1), "per_week": ("W", 1), "per_month": ("M", 1), "per_quarter": ("M", 3),
                  "per_year": ("Y", 1)}[how]
    tr = t.astype(f"M8[{res}]")
    bins = (tr - tr.min()).astype(np.int64) // every
    labels = np.asarray(r.columns["t"])
    assert labels.dtype == np.dtype(f"M8[{res}]")
    assert np.array_equal(labels, np.arange(tr.min(), tr.max() + 1, every))  # every bin, the empty ones too
    assert np.array_equal(np.asarray(r.columns["n"]), np.bincount(bins, minlength=len(labels)))
    assert np.array_equal(np.asarray(r.columns["s"]), np.bincount(bins, weights=v, minlength=len(labels)).astype(np.int64))
    host = vaex_amd.from_arrays(t=t, v=v)
    h = host.groupby(getattr(vaex_amd.BinnerTime, how)(host.t), agg={"n": "count"})
    assert np.array_equal(np.asarray(h.columns["t"]), labels) and np.array_equal(np.asarray(h.columns["n"]), np.asarray(r.columns["n"]))


def _ragged_frame():
    """1968-11-15 .. 1972-03-10: 41 months, 4 years and 1211 days across the epoch, a multiple
    of none of the bin widths below, so the last bin is short and N has to round up."""
    rng = np.random.default_rng(9)
    lo, hi = np.datetime64("1968-11-15T00:00:00", "s"), np.datetime64("1972-03-10T23:59:59", "s")
    t = (lo + rng.integers(0, (hi - lo).astype(np.int64) + 1, N).astype("m8[s]")).astype("M8[s]")
    t[:2] = [lo, hi]
    return t, rng.integers(0, 100, N)


@pytest.mark.parametrize("make, res, every, nbins", [
    (lambda e: vaex_amd.BinnerTime.per_quarter(e, every=2), "M", 6, 7),   # 41 months: 6 whole bins and 5 months
    (lambda e: vaex_amd.BinnerTime(e, "M", every=5), "M", 5, 9),          # 8 whole bins and 1 month
    (lambda e: vaex_amd.BinnerTime(e, "D", every=100), "D", 100, 13),     # 1212 days: 12 whole bins and 12 days
    (lambda e: vaex_amd.BinnerTime(e, "Y", every=2), "Y", 2, 3),          # 1968 .. 1972: 2 whole bins and 1 year
    (lambda e: vaex_amd.BinnerTime(e, "W", every=4), "W", 4, 44),         # 174 weeks: 43 whole bins and 2 weeks
])
def test_binner_time_every(make, res, every, nbins):
    """``every`` units per bin over a span that is no multiple of it: N rounds up, the labels
    step by ``every`` and the short last bin holds its rows; device and host frames against a
    numpy bincount."""
    t, v = _ragged_frame()
    tr = t.astype(f"M8[{res}]")
    span = (tr.max() - tr.min()).astype(np.int64) + 1
    assert span % every != 0
    want_n = -(-span // every)  # the ceiling
    if nbins is not None:
        assert want_n == nbins
    bins = (tr - tr.min()).astype(np.int64) // every
    want_labels = tr.min() + np.arange(want_n) * np.timedelta64(every, res)
    assert bins.max() == want_n - 1
    for df in (_dev(t=t, v=v), vaex_amd.from_arrays(t=t, v=v)):
        binner = make(df.t)
        assert binner.N == want_n
        r = df.groupby(binner, agg={"n": "count", "s": vaex_amd.agg.sum("v")})
        labels = np.asarray(r.columns["t"])
        assert labels.dtype == np.dtype(f"M8[{res}]") and np.array_equal(labels, want_labels)
        assert np.array_equal(np.asarray(r.columns["n"]), np.bincount(bins, minlength=want_n))
        assert np.array_equal(np.asarray(r.columns["s"]), np.bincount(bins, weights=v, minlength=want_n).astype(np.int64))


def test_binner_time_reference_example():
    t = np.arange("2015-01-01", "2015-02-01", dtype=np.datetime64)
    for df in (vaex_amd.from_arrays(t=t, y=np.arange(len(t))), _dev(t=t, y=np.arange(len(t)))):
        r = df.groupby(vaex_amd.BinnerTime.per_week(df.t), agg={"y": "sum"})
        assert np.asarray(r.columns["y"]).tolist() == [21, 70, 119, 168, 87]
        assert np.asarray(r.columns["t"]).astype("M8[D]").tolist() == np.arange("2015-01-01", "2015-02-01", 7, dtype="M8[D]").tolist()


def test_minmax_returns_datetimes():
    t = dt_np.edge_datetimes("ns", N)
    for df in (_dev(t=t), vaex_amd.from_arrays(t=t)):
        lo, hi = df.minmax("t")
        assert lo.dtype == t.dtype and lo == t.min() and hi == t.max()  # exact: no float64 on the way
