"""Times the datetime field kernel: dt_hour(t) / dt_dayofweek(t) / dt_year(t)
over 2^27 datetime64[ns] rows in HBM through (a) the fused kernel and (b) the interpreter
(VH_EXPR_DTFIELD=0), and for scale (c) `t > c`, the comparison-terms kernel (8 B read, 1 B
written per row); then groupby(t.dt.hour).agg(count) against a groupby of a stored int32 hour
column.

The variants alternate window by window (a, b, c, a, b, c, ...), so drift hits them alike.  A
window is REPS back-to-back calls closed by one synchronisation, and gives two figures per
call: the wall clock of the whole call (Python evaluate, output allocation and kernel) and the
library's own HIP-event time of the kernel launch (vh_timing, the "expr" scope).  Median
[min .. max] over ROUNDS windows, after two warm-up windows.

    python scripts/exp_datetime.py [log2 rows] > profiles/datetime_ab.txt
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vaex_amd  # noqa: E402
from vaex_amd import DeviceArray, _lib  # noqa: E402

ROUNDS, REPS = 12, 25


def window(fn, env):
    """(wall ms per call, kernel ms per call) of REPS calls"""
    if env is None:
        os.environ.pop("VH_EXPR_DTFIELD", None)
    else:
        os.environ["VH_EXPR_DTFIELD"] = env
    _lib.synchronize()
    _lib.timing_reset()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    _lib.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / REPS
    calls, ms = _lib.timing_read("expr")
    return wall, (ms / calls if calls else float("nan"))


def fmt(values):
    return f"{statistics.median(values):7.3f} [{min(values):7.3f} .. {max(values):7.3f}]"


def main():
    n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 27)
    rng = np.random.default_rng(0)
    t = (np.datetime64("2009-01-01", "ns").astype(np.int64) + rng.integers(0, 7 * 365 * 86400 * 10 ** 9, n)).view("M8[ns]")
    df = vaex_amd.from_arrays(t=DeviceArray.from_numpy(t))
    _lib.timing_enable(True)
    print(f"rows {n}, datetime64[ns] in HBM; per call, median [min .. max] ms of {ROUNDS} alternating windows of {REPS} calls")
    print(f"{'expression':18s} {'variant':12s} {'wall clock of the call':28s} {'kernel (HIP events)':28s} kernel GB/s")
    for e in ("dt_hour(t)", "dt_dayofweek(t)", "dt_year(t)"):
        variants = [("fused", lambda: df.evaluate(e), None, 12), ("interpreter", lambda: df.evaluate(e), "0", 12),
                    ("t > c (terms)", lambda: df.evaluate("t > np.datetime64('2012-06-01')"), None, 9)]
        got = {name: ([], []) for name, _, _, _ in variants}
        for r in range(ROUNDS + 2):
            for name, fn, env, _ in variants:
                wall, kern = window(fn, env)
                if r >= 2:
                    got[name][0].append(wall)
                    got[name][1].append(kern)
        for name, _, _, bpr in variants:
            wall, kern = got[name]
            print(f"{e:18s} {name:12s} {fmt(wall):28s} {fmt(kern):28s} {n * bpr / statistics.median(kern) / 1e6:8.1f} at {bpr} B/row")
    os.environ.pop("VH_EXPR_DTFIELD", None)
    _lib.timing_enable(False)
    hour = df.evaluate("dt_hour(t)")
    df2 = vaex_amd.from_arrays(t=df.columns["t"], hour=hour)
    a, b = [], []
    for r in range(ROUNDS + 2):
        for out, fn in ((a, lambda: df2.groupby(df2.t.dt.hour, agg="count")), (b, lambda: df2.groupby("hour", agg="count"))):
            _lib.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                fn()
            _lib.synchronize()
            if r >= 2:
                out.append((time.perf_counter() - t0) * 1e3 / 5)
    print(f"groupby(t.dt.hour).agg(count), wall per call      {fmt(a)}")
    print(f"groupby(stored int32 hour, count), wall per call  {fmt(b)}")


if __name__ == "__main__":
    main()
