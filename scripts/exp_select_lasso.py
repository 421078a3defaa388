"""The lasso kernel (vh_pnpoly, csrc/select.hip) on HBM columns: rows/s and read bytes/s per
vertex count, against the streaming ceiling of DESIGN.md 5.1, with the A/B variants of the
kernel (VH_PNPOLY_VARIANT: 1 = edges read from global memory with uniform loads in place of
LDS staging, 2 = the divide evaluated for every edge and row in place of only under the
straddle test) and the host path (hostops.pnpoly) on a 1e7-row prefix.

Times are HIP-event times of the kernel (vh_timing_read("pnpoly")), the best of --repeat runs.
The polygon is a regular nvert-gon of a quarter of the unit square's area around its centre;
x / y are uniform in the unit square.
usage: python scripts/exp_select_lasso.py [--rows 1e9] [--repeat 5] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaex_amd import _lib, hostops, superutils  # noqa: E402
from vaex_amd.device import DeviceArray  # noqa: E402

STREAM_CEILING = 4.64e12  # bytes/s read by scripts/bw_probe.hip's read 16 B + write 2 B loop
VARIANTS = {"0": "LDS staging + straddle-only divide (the product kernel)", "1": "uniform global loads",
            "2": "divide for every edge"}


def polygon(nvert):
    area = 0.25
    r = np.sqrt(area / (nvert / 2 * np.sin(2 * np.pi / nvert)))
    a = 2 * np.pi * (np.arange(nvert) + 0.25) / nvert
    return 0.5 + r * np.cos(a), 0.5 + r * np.sin(a)


def kernel_ms(x, y, poly, repeat):
    best = None
    for _ in range(repeat + 1):  # the first run warms up
        _lib.timing_reset()
        out = superutils.pnpoly(x, y, *poly)
        _lib.synchronize()
        launches, ms = _lib.timing_read("pnpoly")
        assert launches == 1
        best = ms if best is None else min(best, ms)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e9)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(*a):
        line = " ".join(str(v) for v in a)
        print(line, flush=True)
        lines.append(line)

    rows = int(args.rows)
    _lib.call("vh_set_device", 0)
    _lib.timing_enable(True)
    x = DeviceArray.random(rows, "uniform", seed=1)
    y = DeviceArray.random(rows, "uniform", seed=2)
    say(f"vh_pnpoly: {rows:.3g} float64 row pairs, best of {args.repeat} (HIP events); reads 16 B + writes 1 B per row;")
    say(f"streaming ceiling {STREAM_CEILING / 1e12:.2f} TB/s of reads (bw_probe: read 16 B + write 2 B)")
    say("variant nvert rows ms Grows/s read_TB/s ceiling_fraction selected_fraction")
    for nvert in (4, 64, 1024, 8192):
        # compute-bound: fewer rows time the same rate
        n = rows if nvert <= 64 else min(rows, 100_000_000 if nvert <= 1024 else 20_000_000)
        reference = None
        for variant in VARIANTS:
            os.environ["VH_PNPOLY_VARIANT"] = variant
            ms, out = kernel_ms(x[:n], y[:n], polygon(nvert), args.repeat)
            mask = out[:1_000_000].to_numpy()
            if reference is None:
                reference = mask
            assert np.array_equal(mask, reference), "the variants differ"
            rate = n / (ms * 1e-3)
            say(variant, nvert, n, round(ms, 3), round(rate / 1e9, 2), round(rate * 16 / 1e12, 3),
                round(rate * 16 / STREAM_CEILING, 3), round(float(mask.mean()), 4))
        os.environ["VH_PNPOLY_VARIANT"] = "0"
    for k, v in VARIANTS.items():
        say(f"variant {k}: {v}")
    say("the product kernel between the memory-bound and the compute-bound end: nvert ms read_TB/s ceiling_fraction")
    for nvert in (3, 6, 8, 12, 16, 24, 32):
        ms, _ = kernel_ms(x, y, polygon(nvert), args.repeat)
        say(nvert, round(ms, 3), round(rows * 16 / (ms * 1e-3) / 1e12, 3), round(rows * 16 / (ms * 1e-3) / STREAM_CEILING, 3))
    m = min(rows, 10_000_000)
    hx, hy = x[:m].to_numpy(), y[:m].to_numpy()
    say(f"hostops.pnpoly: {m:.3g} rows, {hostops._threads()} threads, best of 3 (1 at 1024 vertices; host clock)")
    for nvert in (4, 64, 1024):
        poly = polygon(nvert)
        bounds = hostops.lasso_bounds(*poly)
        ts = []
        for _ in range(3 if nvert <= 64 else 1):
            t0 = time.perf_counter()
            mask = hostops.pnpoly(hx, hy, *poly, *bounds)
            ts.append(time.perf_counter() - t0)
        dev = superutils.pnpoly(x[:m], y[:m], *poly).to_numpy()
        assert np.array_equal(mask, dev), "host and device masks differ"
        say("host", nvert, m, round(min(ts) * 1e3, 1), "ms", round(m / min(ts) / 1e9, 4), "Grows/s")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
