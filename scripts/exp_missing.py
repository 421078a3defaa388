"""Missing values on HBM frames, measured: 2^27 float64 rows, 10 % missing.

1. fillmissing(x, 0.0): the fused 8-rows-per-lane kernel against the expression interpreter
   (VH_EXPR_FILL=0, read per call), GB/s against the bytes read (8 data + 1 mask) and written (8).
2. df.sum("x") on the masked column, cold (the `mask == 0` keep mask is computed) and with the
   keep mask cached, against the same sum on the unmasked data and under a precomputed
   selection of equal selectivity.
3. from_arrow of an array with nulls: bitmap upload + the unpack kernel, against expanding the
   mask on the host and uploading bytes.

The variants alternate in one process after a warm-up; every figure is the median of REPEAT
runs with the min .. max spread.  Usage: python scripts/exp_missing.py [log2 rows] [repeat]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import vaex_amd  # noqa: E402
from vaex_amd import DeviceArray, DeviceMaskedArray, _lib  # noqa: E402
from vaex_amd.expr import compile_expression  # noqa: E402

LOG2 = int(sys.argv[1]) if len(sys.argv) > 1 else 27
REPEAT = int(sys.argv[2]) if len(sys.argv) > 2 else 9
N = 1 << LOG2


def timed(fn):
    _lib.synchronize()
    t0 = time.perf_counter()
    out = fn()
    _lib.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def report(name, ms, nbytes=None):
    ms = np.array(ms)
    line = f"{name:<46} median {np.median(ms):9.3f} ms   min {ms.min():9.3f}   max {ms.max():9.3f}"
    if nbytes:
        line += f"   {nbytes / np.median(ms) / 1e6:8.1f} GB/s"
    print(line, flush=True)


def main():
    print(f"rows 2^{LOG2} = {N}, float64, 10 % missing, {REPEAT} runs per variant (alternating)", flush=True)
    x = DeviceArray.random(N, "normal", seed=1)
    r = DeviceArray.random(N, "uniform", seed=2)
    frame = vaex_amd.from_arrays(r=r)
    mask = frame.evaluate("r < 0.1")                      # 1 = missing
    sel = frame.evaluate("r >= 0.1")                      # the precomputed selection of equal selectivity
    masked = vaex_amd.from_arrays(x=DeviceMaskedArray(x, mask))
    plain = vaex_amd.from_arrays(x=x, s=sel)
    print(f"missing rows: {masked.columns['x'].null_count}", flush=True)

    # 1. fillmissing through the interpreter
    out = DeviceArray.empty(N, np.float64)
    prog = compile_expression(masked, "fillmissing(x, 0.0)")
    for _ in range(2):
        prog.evaluate(masked, 0, N, out=out)
    times = {"fillmissing(x, 0.0)  fused kernel": [], "fillmissing(x, 0.0)  interpreter (VH_EXPR_FILL=0)": []}
    for _ in range(REPEAT):
        for k, switch in zip(times, ("1", "0")):
            os.environ["VH_EXPR_FILL"] = switch
            times[k].append(timed(lambda: prog.evaluate(masked, 0, N, out=out))[0])
    os.environ.pop("VH_EXPR_FILL")
    for k, ms in times.items():
        report(k, ms, N * 17)

    # 2. sum over the masked column
    def cold():
        masked.__dict__.get("_filter_mask_cache", []).clear()
        return masked.sum("x")

    variants = {"sum(x) masked, cold (keep mask computed)": cold,
                "sum(x) masked, keep mask cached": lambda: masked.sum("x"),
                "sum(x) unmasked data": lambda: plain.sum("x"),
                "sum(x) precomputed selection 's'": lambda: plain.sum("x", selection="s")}
    for fn in variants.values():
        fn()
    times = {k: [] for k in variants}
    for _ in range(REPEAT):
        for k, fn in variants.items():
            times[k].append(timed(fn)[0])
    for k, ms in times.items():
        report(k, ms)

    # 3. from_arrow
    import pyarrow as pa
    values = np.random.default_rng(0).normal(size=N)
    nulls = np.random.default_rng(1).random(N) < 0.1
    ar = pa.array(values, mask=nulls)

    def host_expand():
        m = np.asarray(ar.is_null())  # the byte mask expanded on the host, uploaded as N bytes
        return DeviceMaskedArray(DeviceArray.from_numpy(np.frombuffer(ar.buffers()[1], np.float64)[:N]),
                                 DeviceArray.from_numpy(m.view(np.uint8)))

    def values_only():
        return DeviceArray.from_numpy(np.frombuffer(ar.buffers()[1], np.float64)[:N])

    variants = {"from_arrow: bitmap upload + unpack kernel": lambda: DeviceMaskedArray.from_arrow(ar),
                "host is_null() + byte upload": host_expand,
                "(the values upload alone)": values_only}
    for fn in variants.values():
        fn()
    times = {k: [] for k in variants}
    for _ in range(REPEAT):
        for k, fn in variants.items():
            times[k].append(timed(fn)[0])
    for k, ms in times.items():
        report(k, ms)
    d = DeviceMaskedArray.from_arrow(ar)
    assert d.null_count == int(nulls.sum())
    ms = [timed(lambda: d.to_arrow())[0] for _ in range(3)]
    report("to_arrow: pack kernel + read back", ms)


if __name__ == "__main__":
    main()
