"""DataFrame.join on HBM-resident frames: the table of DESIGN.md 5.18.

The left frame has `rows` rows (default 1e8) with an int32 and an int64 key column; the right
frames have 1e2 / 4096 / 1e5 / 1e7 unique keys and 1 or 4 float64 payload columns; one more right frame
has every key twice (allow_duplication=True, a left frame of rows / 10).  Per shape, 2 warm-ups
and then the best and worst of 5 timed calls (wall time around a device synchronise) of
  build   -- right._index(key),
  probe   -- index.map_index(left keys, int32 lookup in HBM),
  ordinal -- ordered_set.map_ordinal on the same key column and keys (the yardstick: the same
             lookup per row with the parent commit's kernel),
  gather  -- take_device(payload columns, lookup),
  join    -- the whole left.join(right, on=key),
with the library's HIP-event kernel times of the last call, and the probe's and the gather's
compulsory bytes (keys + lookup; lookup + payload) at the streaming rate DESIGN.md 5.1 records.
usage: python scripts/exp_join.py [rows]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vaex_amd  # noqa: E402
from vaex_amd import _lib, superutils  # noqa: E402
from vaex_amd.device import DeviceArray  # noqa: E402

STREAM_TBS = 6.38  # contiguous reads sustained on this chip, TB/s
WARM, REPS = 2, 5
KERNELS = ("index_update", "index_seal_duplicates", "index_map_index", "index_map_duplicates", "index_matched", "take",
           "set_map_ordinal")

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10 ** 8


def timed(fn, warm=WARM):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(REPS):
        _lib.synchronize()
        t0 = time.perf_counter()
        fn()
        _lib.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(min(t), 3), round(max(t), 3)


def kernel_ms(fn):
    _lib.synchronize()
    _lib.timing_reset()
    _lib.timing_enable(True)
    fn()
    _lib.synchronize()
    _lib.timing_enable(False)
    return {k: round(_lib.timing_read(k)[1], 3) for k in KERNELS if _lib.timing_read(k)[0]}


def stream_ms(nbytes):
    return round(nbytes / (STREAM_TBS * 1e12) * 1e3, 3)


def right_frame(keys, dtype, ncols, seed):
    cols = {"k": DeviceArray.from_numpy(keys.astype(dtype))}
    for c in range(ncols):
        cols[f"p{c}"] = DeviceArray.random(len(keys), "uniform", seed=seed + c)
    return vaex_amd.from_arrays(**cols)


rng = np.random.default_rng(0)
for dtype in ("int32", "int64"):
    for R in (10 ** 2, 4096, 10 ** 5, 10 ** 7):
        left_keys = DeviceArray.random(n, "randint", seed=R % 97, a=0, b=R, dtype=dtype)
        left = vaex_amd.from_arrays(k=left_keys, v=DeviceArray.random(n, "uniform", seed=5))
        keys = rng.permutation(R)
        for ncols in (1, 4):
            right = right_frame(keys, dtype, ncols, seed=11)
            payload = [right.columns[f"p{c}"] for c in range(ncols)]
            lookup = DeviceArray(n, np.int32)
            ix = right._index("k")
            oset = superutils.ordered_set_type_from_dtype(dtype)()
            oset.update(right.columns["k"])
            isz = np.dtype(dtype).itemsize
            row = {"key": dtype, "right_rows": R, "payload_columns": ncols, "left_rows": n}
            row["build_ms_best_worst"] = timed(lambda: right._index("k"))
            row["probe_ms_best_worst"] = timed(lambda: ix.map_index(left_keys, lookup))
            row["ordinal_ms_best_worst"] = timed(lambda: oset.map_ordinal(left_keys))
            row["ordinal_out_itemsize"] = np.dtype(oset._ordinal_dtype()).itemsize
            row["gather_ms_best_worst"] = timed(lambda: superutils.take_device(payload, lookup))
            row["join_ms_best_worst"] = timed(lambda: left.join(right, on="k"))
            row["kernels_ms_of_one_join"] = kernel_ms(lambda: left.join(right, on="k"))
            row["kernels_ms_of_one_ordinal"] = kernel_ms(lambda: oset.map_ordinal(left_keys))
            row["probe_stream_ms"] = stream_ms(n * (isz + 4))
            row["gather_stream_ms"] = stream_ms(n * (4 + 8 * ncols))
            row["probe_over_stream"] = round(row["probe_ms_best_worst"][0] / row["probe_stream_ms"], 2)
            row["gather_over_stream"] = round(row["gather_ms_best_worst"][0] / row["gather_stream_ms"], 2)
            res = left.join(right, on="k")
            row["result_columns"] = list(res.columns)
            row["result_in_hbm"] = all(isinstance(c, DeviceArray) for c in res.columns.values())
            print(json.dumps(row), flush=True)
            del res, lookup, ix, oset, right, payload
        del left, left_keys

# every right key twice: the duplicates path (pairs are read back and the left frame extended)
nd = max(1, n // 10)
R = 10 ** 5
left = vaex_amd.from_arrays(k=DeviceArray.random(nd, "randint", seed=3, a=0, b=R, dtype="int32"),
                            v=DeviceArray.random(nd, "uniform", seed=5))
right = right_frame(np.concatenate([rng.permutation(R), rng.permutation(R)]), "int32", 1, seed=21)
row = {"key": "int32", "right_rows": 2 * R, "every_key_twice": True, "payload_columns": 1, "left_rows": nd}
row["build_ms_best_worst"] = timed(lambda: right._index("k"))
row["join_ms_best_worst"] = timed(lambda: left.join(right, on="k", allow_duplication=True), warm=1)
row["kernels_ms_of_one_join"] = kernel_ms(lambda: left.join(right, on="k", allow_duplication=True))
row["result_rows"] = left.join(right, on="k", allow_duplication=True).length_unfiltered()
print(json.dumps(row), flush=True)
del left, right
