"""Compare `bench.py --dump-outputs` directories (count.npy, sum.npy) with the first one:
whether the counts are identical, how many sum cells differ and by how much (relative).
usage: python scripts/dump_cmp.py DIR [DIR ...]   (profiles/host_image_ab.txt section 3)"""
import os
import sys

import numpy as np


def rel(a, b):
    m = np.maximum(np.abs(a), np.abs(b))
    ok = m > 0
    return float(np.max(np.abs(a - b)[ok] / m[ok])) if ok.any() else 0.0


dirs = sys.argv[1:]
c0, s0 = (np.load(os.path.join(dirs[0], f)) for f in ("count.npy", "sum.npy"))
for d in dirs:
    c, s = (np.load(os.path.join(d, f)) for f in ("count.npy", "sum.npy"))
    print(f"{os.path.basename(d.rstrip('/'))} vs {os.path.basename(dirs[0].rstrip('/'))}: count identical {np.array_equal(c, c0)}  "
          f"sum cells differing {int((s != s0).sum())}  max rel diff {rel(s, s0):.3e}  total {s.sum():.9f}")
