"""Times the device string path on HBM columns:

  1. the dictionary encode (ordered_set_string.update + map_ordinal) of ROWS rows of "id%03d"
     keys with 100 distinct values and of "id%010d" keys with 10^6 distinct values, each also
     as a fraction of the HBM time for the bytes it must read once (offsets + bytes, at 8 TB/s),
     and the same two encodes by pyarrow.compute.dictionary_encode on the host;
  2. groupby-sum by the string key against the same groupby by the pre-encoded int32 codes
     (encoding every time, and with the frame's cached codes);
  3. str_contains at both mean lengths;
  4. the two row-kernel forms (lane per row, wave per row; VH_STR_FORM pins one) across mean
     lengths 4 .. 512 at a fixed 2^29 bytes, 1000 distinct keys: the switch point.

Every figure is the wall clock of calls that end in a device synchronisation, median
[min .. max] over REPS repetitions after one warm-up; variants alternate.

    python scripts/str_bench.py [rows, default 100000000] > profiles/strings_ab.txt
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vaex_amd  # noqa: E402
from vaex_amd import DeviceArray, _lib  # noqa: E402
from vaex_amd.strings import DeviceStringArray, ordered_set_string  # noqa: E402

REPS = 3
HBM = 8.0e12  # bytes / s, the MI355X's peak


def fixed_width(ids, prefix, digits):
    """(offsets int32, bytes uint8) of prefix + zero-padded decimal ids, built with NumPy"""
    n = len(ids)
    width = len(prefix) + digits
    data = np.empty((n, width), np.uint8)
    data[:, :len(prefix)] = np.frombuffer(prefix.encode(), np.uint8)
    v = ids.astype(np.int64)
    for k in range(digits):
        data[:, width - 1 - k] = 48 + v % 10
        v //= 10
    return (np.arange(n + 1, dtype=np.int64) * width).astype(np.int32 if n * width < 2 ** 31 else np.int64), data.reshape(-1)


def timed(fn, reps=REPS):
    fn()
    _lib.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        _lib.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def fmt(ms):
    return f"{statistics.median(ms):9.2f} [{min(ms):9.2f} .. {max(ms):9.2f}] ms"


def encode(col):
    s = ordered_set_string()
    s.update(col)
    return s.map_ordinal(col), s


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    rng = np.random.default_rng(0)
    print(f"rows {n}; wall clock per call, median [min .. max] of {REPS} after one warm-up")
    cases = [("id%03d, 100 distinct", "id", 3, 100), ("id%010d, 1e6 distinct", "id", 10, 1_000_000)]
    import pyarrow as pa
    import pyarrow.compute as pc
    v = DeviceArray.from_numpy(rng.normal(size=n))
    for label, prefix, digits, distinct in cases:
        ids = rng.integers(0, distinct, size=n)
        offsets, data = fixed_width(ids, prefix, digits)
        col = DeviceStringArray._from_host(offsets, data)
        nbytes = offsets.nbytes + data.nbytes
        floor_ms = nbytes / HBM * 1e3
        print(f"\n== {label}: mean length {len(data) / n:.0f} B, offsets + bytes {nbytes / 1e9:.2f} GB, "
              f"one read at 8 TB/s {floor_ms:.3f} ms")
        ms = timed(lambda: encode(col))
        print(f"encode (update + map_ordinal)      {fmt(ms)}   HBM floor / time = {floor_ms / statistics.median(ms):.3f}")
        s = ordered_set_string()
        ms = timed(lambda: ordered_set_string().update(col))
        print(f"  update alone                     {fmt(ms)}")
        s.update(col)
        ms = timed(lambda: s.map_ordinal(col))
        print(f"  map_ordinal alone                {fmt(ms)}")
        arr = pa.Array.from_buffers(pa.string() if offsets.dtype == np.int32 else pa.large_string(), n,
                                    [None, pa.py_buffer(offsets), pa.py_buffer(data)])
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            d = pc.dictionary_encode(arr)
            t.append((time.perf_counter() - t0) * 1e3)
        assert len(d.dictionary) == len(s)
        print(f"pyarrow dictionary_encode (host)   {fmt(t)}")
        del arr, d
        df = vaex_amd.from_arrays(k=col, v=v)
        codes = s.map_ordinal(col)
        dfc = vaex_amd.from_arrays(k=codes, v=v)
        agg = {"s": vaex_amd.agg.sum("v")}

        def by_string_cold():
            df.__dict__.pop("_string_codes", None)
            return df.groupby("k", agg=agg)

        a, b, c = [], [], []
        by_string_cold(), dfc.groupby("k", agg=agg)
        for _ in range(REPS):
            a += timed(by_string_cold, 1)
            b += timed(lambda: df.groupby("k", agg=agg), 1)
            c += timed(lambda: dfc.groupby("k", agg=agg), 1)
        print(f"groupby-sum by the string key      {fmt(a)}   (encodes every time)")
        print(f"groupby-sum, codes cached          {fmt(b)}")
        print(f"groupby-sum by int32 codes         {fmt(c)}   string / codes = {statistics.median(a) / statistics.median(c):.2f}")
        ms = timed(lambda: col.match("str_contains", "d05"))
        print(f"str_contains 'd05'                 {fmt(ms)}   HBM floor / time = {(nbytes + n) / HBM * 1e3 / statistics.median(ms):.3f}")
        ms = timed(lambda: col.len("str_len"))
        print(f"str_len                            {fmt(ms)}")
        del df, dfc, codes, col, s

    total = 1 << 29
    print(f"\n== the two forms of the row kernels: {total >> 20} MiB of bytes, 1000 distinct keys; encode (update + map_ordinal)")
    print(f"{'mean length':>12s} {'rows':>10s}   {'lane per row':38s} {'wave per row':38s} lane / wave")
    for length in (4, 8, 16, 32, 48, 64, 96, 128, 256, 512):
        rows = total // length
        keys = rng.integers(97, 123, size=(1000, length), dtype=np.uint8)
        k = np.arange(1000)
        keys[:, 0], keys[:, 1], keys[:, 2] = 97 + k % 26, 97 + k // 26 % 26, 97 + k // 676  # distinct
        ids = rng.integers(0, 1000, size=rows)
        data = keys[ids].reshape(-1)
        offsets = (np.arange(rows + 1, dtype=np.int64) * length).astype(np.int32)
        col = DeviceStringArray._from_host(offsets, data)
        lane, wave = [], []
        for form in ("lane", "wave"):
            os.environ["VH_STR_FORM"] = form
            encode(col)
        for _ in range(REPS):
            os.environ["VH_STR_FORM"] = "lane"
            lane += timed(lambda: encode(col), 1)
            os.environ["VH_STR_FORM"] = "wave"
            wave += timed(lambda: encode(col), 1)
        os.environ.pop("VH_STR_FORM", None)
        print(f"{length:12d} {rows:10d}   {fmt(lane):38s} {fmt(wave):38s} {statistics.median(lane) / statistics.median(wave):.2f}")
        del col


if __name__ == "__main__":
    main()
