"""DataFrame.correlation / cov through the fused AggCov pass against the composed route (five
delayed means of x, y, (x)*(y), (x)*(x), (y)*(y) over the same binby), on HBM-resident float64
columns: per case the median of warm repeats of the call's wall time (ending in a device
synchronise) and of the library's HIP-event kernel time, and for the fused cases the achieved
bytes per second over the algorithmic bytes, 8 B x (N + binby columns) per row, as a share of
the streaming read rate DESIGN.md 5.1 records.  The composed leg also runs where the frame has
no cov (the parent of this feature).  usage: python scripts/exp_cov.py [rows] [repeats]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vaex_amd  # noqa: E402
from vaex_amd import _lib  # noqa: E402
from vaex_amd.device import DeviceArray  # noqa: E402

STREAM_READ_TBS = 6.38  # contiguous float64 reads sustained on this chip, TB/s
KERNELS = ["bin_cov_reduce", "bin_cov_lds", "bin_cov_global", "bin_cells", "bin_indices", "bin_reduce0", "bin_small_f64",
           "bin_fused_lds", "bin_fused_global", "bin_aggregate", "bin_aggregate_lds", "tile_sample", "tile_scatter",
           "tile_scatter_f64", "tile_reduce", "expr", "minmax"]

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10 ** 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
df = vaex_amd.from_arrays(x=DeviceArray.random(n, "normal", seed=1), y=DeviceArray.random(n, "normal", seed=2),
                          z=DeviceArray.random(n, "normal", seed=3), b=DeviceArray.random(n, "uniform", seed=4),
                          c=DeviceArray.random(n, "uniform", seed=5))
BINBYS = {"none": dict(), "shape4": dict(binby="b", limits=[0, 1], shape=4),
          "shape128": dict(binby="b", limits=[0, 1], shape=128),
          "128x128": dict(binby=["b", "c"], limits=[[0, 1], [0, 1]], shape=128)}


def composed(kw):
    ps = [df.mean(e, delay=True, **kw) for e in ("x", "y", "(x)*(y)", "(x)*(x)", "(y)*(y)")]
    df.execute()
    mx, my, mxy, mxx, myy = (p.get() for p in ps)
    return (mxy - mx * my) / ((mxx - mx * mx) * (myy - my * my)) ** 0.5


def timed(fn):
    fn()  # warm: code objects, scratch and pinned blocks
    wall, kern, per = [], [], {}
    for _ in range(reps):
        _lib.synchronize()
        _lib.timing_reset()
        _lib.timing_enable(True)
        t0 = time.perf_counter()
        fn()
        _lib.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        _lib.timing_enable(False)
        per = {k: round(_lib.timing_read(k)[1], 3) for k in KERNELS if _lib.timing_read(k)[0]}
        kern.append(sum(per.values()))
    return statistics.median(wall), statistics.median(kern), per


for name, kw in BINBYS.items():
    nb = 0 if "binby" not in kw else len(kw["binby"]) if isinstance(kw["binby"], list) else 1
    cases = [("composed", 2, lambda: composed(kw))]
    if hasattr(df, "correlation"):
        cases += [("correlation", 2, lambda: df.correlation("x", "y", **kw)), ("cov3", 3, lambda: df.cov(["x", "y", "z"], **kw))]
    for label, N, fn in cases:
        wall, kern, per = timed(fn)
        row = {"binby": name, "case": label, "rows": n, "wall_ms": round(wall, 3), "kernel_ms": round(kern, 3), "kernels": per}
        if label != "composed":
            gbs = 8.0 * (N + nb) * n / (kern * 1e-3) / 1e9 if kern else None
            row["algorithmic_GBps"] = None if gbs is None else round(gbs, 1)
            row["share_of_stream_read"] = None if gbs is None else round(gbs / (STREAM_READ_TBS * 1e3), 3)
        print(json.dumps(row), flush=True)
