"""In-process A/B of the host-image mirror (profiles/host_image_ab.txt section 4): the
bench's C2 step (bin + read-back of both grids) and the count-only step with VH_HOST_IMAGE=0 / 1
alternated in one process, so both settings see the same placement.  Per setting and round: wall
time per step over 10 steps without timers, then the kernels' HIP-event times over 10 instrumented
steps; residual = wall - sum of the three kernels; bins_stat = host_image_bins over the 20 steps.
usage: python scripts/exp_host_image.py [rows=1e9] [settings=0,1]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from vaex_amd import _lib, superagg  # noqa: E402
from vaex_amd.device import DeviceArray  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10 ** 9
MODES = sys.argv[2].split(",") if len(sys.argv) > 2 else ["0", "1"]
bins = 1024
x = DeviceArray.random(n, "normal", seed=2)
y = DeviceArray.random(n, "normal", seed=3)
w = DeviceArray.random(n, "uniform", seed=4)


def step(with_sum=True):
    bx = superagg.BinnerScalar_float64("x", -4.0, 4.0, bins)
    by = superagg.BinnerScalar_float64("y", -4.0, 4.0, bins)
    bx.set_data(x)
    by.set_data(y)
    grid = superagg.Grid([bx, by])
    aggs = [superagg.AggCount_int64(grid)]
    if with_sum:
        s = superagg.AggSum_float64(grid)
        s.set_data(w, 0)
        aggs.append(s)
    grid.bin(aggs)
    return [np.asarray(a) for a in aggs]


for mode in MODES:  # warm both settings
    os.environ["VH_HOST_IMAGE"] = mode
    for _ in range(3):
        step()
for with_sum in (True, False):
    for rep in range(4):
        for mode in MODES:
            os.environ["VH_HOST_IMAGE"] = mode
            _lib.synchronize()
            _lib.stat_read("host_image_bins")
            t0 = time.perf_counter()
            for _ in range(10):
                step(with_sum)
            _lib.synchronize()
            wall = (time.perf_counter() - t0) / 10 * 1e3
            _lib.timing_reset()
            _lib.timing_enable(True)
            for _ in range(10):
                step(with_sum)
            _lib.synchronize()
            _lib.timing_enable(False)
            per = {}
            for k in ("tile_sample", "tile_scatter_f64", "tile_reduce"):
                c, ms = _lib.timing_read(k)
                per[k] = round(ms / max(c, 1), 4)
            print(f"{'count+sum' if with_sum else 'count'} rep {rep} VH_HOST_IMAGE={mode} wall_ms {wall:.3f} kernels {per} "
                  f"residual {wall - sum(per.values()):.3f} bins_stat {_lib.stat_read('host_image_bins')}", flush=True)
