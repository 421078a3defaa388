"""value_counts on HBM-resident columns: the table of DESIGN.md 5.16.

Per case (int32 keys with 10 / 1e3 / 1e5 / 1e6 distinct values, float64 keys with 1e3, the
int32 1e3 case with a selection), 2 warm-ups and then the best and worst of 5 timed calls of
  counter  -- counter_<dtype>(): update(column[, select]) + sorted_counts(), wall time ending in
              the read-back of the answer (a device synchronise),
  api      -- df.key.value_counts() (the task, the counter and the pandas Series),
  groupby  -- df.groupby(key, agg='count') at the integer shapes (the yardstick; its code is
              the parent commit's, this feature does not touch it),
with the library's HIP-event time of the update and finish kernels of the last counter call,
and the column's read time at the streaming read rate DESIGN.md 5.1 records.
usage: python scripts/exp_value_counts.py [rows]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vaex_amd  # noqa: E402
from vaex_amd import _lib, superutils  # noqa: E402
from vaex_amd.device import DeviceArray  # noqa: E402

STREAM_READ_TBS = 6.38  # contiguous reads sustained on this chip, TB/s
WARM, REPS = 2, 5

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10 ** 8
cols = {f"k{d}": DeviceArray.random(n, "randint", seed=d, a=0, b=d, dtype="int32") for d in (10, 10 ** 3, 10 ** 5, 10 ** 6)}
cols["s"] = DeviceArray.random(n, "uniform", seed=7)
df = vaex_amd.from_arrays(**cols)
df.add_column("f1000", df.evaluate("astype(k1000, 'float64')"))


def timed(fn):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(REPS):
        _lib.synchronize()
        t0 = time.perf_counter()
        fn()
        _lib.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(min(t), 3), round(max(t), 3)


def counter_call(col, select=None):
    c = superutils.counter_type_from_dtype(col.dtype)()
    c.update(col, select=select)
    return c.sorted_counts()


def kernel_ms(fn):
    _lib.synchronize()
    _lib.timing_reset()
    _lib.timing_enable(True)
    fn()
    _lib.synchronize()
    _lib.timing_enable(False)
    return {k: round(_lib.timing_read(k)[1], 3) for k in ("counter_update", "counter_read") if _lib.timing_read(k)[0]}


CASES = [("int32", "k10", 10, None), ("int32", "k1000", 10 ** 3, None), ("int32", "k100000", 10 ** 5, None),
         ("int32", "k1000000", 10 ** 6, None), ("float64", "f1000", 10 ** 3, None), ("int32", "k1000", 10 ** 3, "s < 0.5")]
for dtype, name, distinct, selection in CASES:
    col = df.columns[name]
    keep = df.device_keep_mask(0, n, selection) if selection else None
    row = {"dtype": dtype, "distinct": distinct, "selection": selection, "rows": n,
           "column_read_ms_at_stream_rate": round(col.nbytes / (STREAM_READ_TBS * 1e12) * 1e3, 3)}
    row["counter_ms_best_worst"] = timed(lambda: counter_call(col, keep))
    row["kernels_ms"] = kernel_ms(lambda: counter_call(col, keep))
    row["api_ms_best_worst"] = timed(lambda: df.value_counts(name, selection=selection))
    if dtype != "float64" and selection is None:
        row["groupby_ms_best_worst"] = timed(lambda: df.groupby(name, agg="count"))
    keys, counts, _ = counter_call(col, keep)
    row["distinct_found"], row["rows_counted"] = len(keys), int(counts.sum())
    print(json.dumps(row), flush=True)
