"""csrc/datetime_dev.hpp on the CPU: the check program (tests/host/datetime_check.hip, built by
the default make next to the library) runs the header's field, timedelta-field and cast
functions -- the ones the device kernels inline -- on the edge columns; every value must equal
the numpy restatement (tests/dt_np.py)."""
import os
import subprocess

import numpy as np
import pytest

import dt_np

CHECK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vaex_amd", "datetime_check")


def _run(lines):
    assert os.path.exists(CHECK), f"{CHECK} is missing: build the library (make -C vaex_amd/csrc)"
    out = subprocess.run([CHECK], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    got = [int(v) for v in out.split()]
    assert len(got) == len(lines)
    return np.array(got, np.int64)


@pytest.mark.parametrize("unit", dt_np.UNITS)
def test_datetime_fields(unit):
    x = dt_np.edge_datetimes(unit, 400)
    ticks = x.astype(np.int64)
    for f, name in enumerate(dt_np.DT_FIELDS):
        got = _run([f"f {dt_np.UNIT_CODE[unit]} {f} {t}" for t in ticks])
        want = dt_np.dt_field(name, x).astype(np.int64)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (unit, name, ticks[bad[:5]], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("unit", dt_np.UNITS)
def test_timedelta_fields(unit):
    x = dt_np.edge_timedeltas(unit, 400)
    ticks = x.astype(np.int64)
    for f, name in enumerate(dt_np.TD_FIELDS):
        got = _run([f"t {dt_np.UNIT_CODE[unit]} {f} {t}" for t in ticks])
        want = dt_np.td_field(name, x)
        want = want.view(np.int64) if want.dtype == np.float64 else want.astype(np.int64)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (unit, name, ticks[bad[:5]], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("kind", ["M", "m"])
def test_casts(kind):
    for a, b in dt_np.cast_pairs(kind):
        if a in dt_np.UNITS:
            x = dt_np.edge_datetimes(a, 200) if kind == "M" else dt_np.edge_timedeltas(a, 200)
        else:  # W / M / Y sources: counts around the epoch and at the ends of the year range
            x = np.concatenate([np.arange(-60, 60), [-23000, 23000, -1969 * (12 if a == "M" else 1 if a == "Y" else 52)]])
            x = x.astype(np.int64).view(f"{kind}8[{a}]")
        x = dt_np.castable(x, b)
        assert len(x) > 20
        got = _run([f"c {dt_np.UNIT_CODE[a]} {dt_np.UNIT_CODE[b]} {t}" for t in x.astype(np.int64)])
        want = x.astype(f"{kind}8[{b}]").astype(np.int64)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (kind, a, b, x[bad[:5]], got[bad[:5]], want[bad[:5]])
