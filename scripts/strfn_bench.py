"""Times the device string transforms on HBM columns:

  1. lower, slice(0, 3), strip, cat with a constant and replace over ROWS rows of "id%03d" keys
     (100 distinct, 5 bytes) and of "id%010d" keys (10^6 distinct, 12 bytes): the wall clock of
     the whole call (plan kernel, scan, the total's read-back, the output's allocation, write
     kernel) ending in a device synchronisation, next to the matching pyarrow.compute kernel on
     the host and to the HBM floor: one read of the input's offsets and bytes plus one write of
     the output's, at the 8 TB/s peak;
  2. groupby-sum by str_lower(s) against the same groupby by s, the key encoded every time.

Every figure is median [min .. max] over REPS repetitions after one warm-up; the variants of a
comparison alternate.

    python scripts/strfn_bench.py [rows, default 100000000] > profiles/strfn_ab.txt
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vaex_amd  # noqa: E402
from vaex_amd import DeviceArray, _lib  # noqa: E402
from vaex_amd.strings import DeviceStringArray  # noqa: E402

REPS = 5
HBM = 8.0e12  # bytes / s, the MI355X's peak


def fixed_width(ids, prefix, digits):
    """(offsets, bytes uint8) of prefix + zero-padded decimal ids, built with NumPy"""
    n = len(ids)
    width = len(prefix) + digits
    data = np.empty((n, width), np.uint8)
    data[:, :len(prefix)] = np.frombuffer(prefix.encode(), np.uint8)
    v = ids.astype(np.int64)
    for k in range(digits):
        data[:, width - 1 - k] = 48 + v % 10
        v //= 10
    return (np.arange(n + 1, dtype=np.int64) * width).astype(np.int32 if n * width < 2 ** 31 else np.int64), data.reshape(-1)


def timed(fn, reps=REPS, sync=True):
    fn()
    if sync:
        _lib.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        if sync:
            _lib.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        del r
    return out


def fmt(ms):
    return f"{statistics.median(ms):9.2f} [{min(ms):9.2f} .. {max(ms):9.2f}] ms"


def main():
    import pyarrow as pa
    import pyarrow.compute as pc
    rows = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    if _lib.device_count() < 1:
        raise SystemExit("strfn_bench needs a GPU")
    rng = np.random.default_rng(0)
    print(f"rows {rows}, reps {REPS}, HBM peak {HBM / 1e12:.1f} TB/s; device figures: the whole call ending in a synchronise")
    ops = [
        ("lower", lambda c: c.lower(), lambda a: pc.utf8_lower(a)),
        ("slice(0, 3)", lambda c: c.slice(0, 3), lambda a: pc.utf8_slice_codeunits(a, 0, 3)),
        ("strip", lambda c: c.strip(), lambda a: pc.ascii_trim_whitespace(a)),
        ("cat '_x'", lambda c: c.cat("_x"), lambda a: pc.binary_join_element_wise(a, pa.scalar("_x", a.type), pa.scalar("", a.type))),
        ("replace id->key", lambda c: c.replace("id", "key"), lambda a: pc.replace_substring(a, "id", "key")),
    ]
    frames = {}
    for label, prefix, digits, distinct in (("id%03d", "id", 3, 100), ("id%010d", "id", 10, 10 ** 6)):
        ids = rng.integers(0, distinct, size=rows)
        offsets, data = fixed_width(ids, prefix, digits)
        col = DeviceStringArray._from_host(offsets, data)
        typ = pa.large_string() if offsets.dtype == np.int64 else pa.string()
        host = pa.Array.from_buffers(typ, rows, [None, pa.py_buffer(offsets), pa.py_buffer(data)])
        in_bytes = offsets.nbytes + data.nbytes
        print(f"\n{label}: {rows} rows, {data.nbytes / 1e9:.2f} GB of bytes, {offsets.dtype} offsets")
        print(f"{'op':18s} {'device':>40s} {'pyarrow.compute (host)':>40s} {'floor':>9s} {'device/floor':>12s} {'host/device':>11s}")
        for name, dev, cpu in ops:
            out = dev(col)
            _lib.synchronize()
            out_bytes = out.offsets.nbytes + out._root[1]
            got = out[:1000].tolist()
            want = cpu(host.slice(0, 1000)).to_pylist()
            assert got == want, (name, got[:3], want[:3])  # the two sides compute the same column
            del out
            floor = (in_bytes + out_bytes) / HBM * 1e3
            d = timed(lambda: dev(col))
            h = timed(lambda: cpu(host), reps=2, sync=False)
            print(f"{name:18s} {fmt(d):>40s} {fmt(h):>40s} {floor:6.2f} ms {statistics.median(d) / floor:11.1f}x "
                  f"{statistics.median(h) / statistics.median(d):10.0f}x")
        frames[label] = (col, ids)
        del host

    print("\ngroupby-sum, the string key encoded on every call (the frame's cached codes dropped)")
    v = DeviceArray.from_numpy(rng.integers(0, 10, size=rows).astype(np.int64))
    for label, (col, ids) in frames.items():
        df = vaex_amd.from_arrays(s=col, v=v)

        def run(key):
            df.__dict__.pop("_string_codes", None)
            return df.groupby(key, agg={"v": vaex_amd.agg.sum("v")})

        a, b = [], []
        run("s"), run("str_lower(s)")
        _lib.synchronize()
        for _ in range(REPS):  # alternating
            for key, out in (("s", a), ("str_lower(s)", b)):
                t0 = time.perf_counter()
                run(key)
                _lib.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
        print(f"{label:10s} by s {fmt(a)}   by str_lower(s) {fmt(b)}   ratio {statistics.median(b) / statistics.median(a):.2f}")


if __name__ == "__main__":
    main()
