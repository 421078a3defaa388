"""A/B of ``DataFrame.sort`` on an HBM frame: this tree against a checkout of another commit.

    python scripts/sort_ab.py [--parent DIR] [--rows N] [--rounds R] [--repeats K] [--out FILE]

``--parent DIR`` is the root of a built checkout of the commit to compare with (it needs
``vaex_amd/`` with its ``libvaexhip.so``).  Each tree runs in a fresh child process, the two
trees alternating ``--rounds`` times (other work shares the host, so the spread between rounds
of one tree is printed next to the difference between the trees).  A child builds the frames
from a seed, warms each case up once, then times ``--repeats`` calls of ``df.sort`` with a host
clock around the call and a device synchronise, and prints a checksum of the sorted frame so
that the two trees can be seen to agree.  The stage times (the library's ``TimedScope`` events
for range / encode / digits / take) come from one more call with timing on, outside the timed
window.

Cases (2^24 rows by default, four HBM columns each):
  f64      by a float64 key (normal, NaN in every 97th row), three payload columns
  i32x2    by [a, b]: a int32 over 1 000 values, b int32 over its full range: 10 + 32 bits,
           one round of 64-bit words
  i32x2w   the same order with a stretched past 32 bits (a * 2^23 as int64: 33 + 32 = 65 bits,
           two rounds): what packing both keys into one round is worth
A tree whose ``sort`` takes no list of keys (the parent of the commit that added it) reports
the list cases as unsupported.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ["mask_rows", "sort_range", "sort_encode", "sort_digits", "take"]


def child(args):
    sys.path.insert(0, args.tree)
    import numpy as np

    import vaex_amd
    from vaex_amd import _lib
    from vaex_amd.device import DeviceArray
    assert os.path.dirname(os.path.abspath(vaex_amd.__file__)) == os.path.join(os.path.abspath(args.tree), "vaex_amd")
    if _lib.device_count() < 1:
        raise SystemExit("sort_ab needs a GPU")
    n = args.rows
    rng = np.random.default_rng(11)
    x = rng.normal(size=n)
    x[::97] = np.nan
    a = rng.integers(0, 1000, n).astype(np.int32)
    b = rng.integers(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32)
    host = dict(x=x, a=a, b=b, aw=a.astype(np.int64) << 23, p=np.arange(n, dtype=np.int64), q=rng.normal(size=n).astype(np.float32))
    dev = {k: DeviceArray.from_numpy(v) for k, v in host.items()}
    cases = [("f64", ["x", "p", "q", "a"], "x"), ("i32x2", ["a", "b", "p", "q"], ["a", "b"]),
             ("i32x2w", ["aw", "b", "p", "q"], ["aw", "b"])]
    for name, names, by in cases:
        df = vaex_amd.from_arrays(**{k: dev[k] for k in names})
        rec = dict(tree=args.label, case=name, rows=n)

        def run():
            res = df.sort(by)
            _lib.synchronize()
            return res

        try:
            res = run()  # warm-up: code objects, rocPRIM's choices, the block caches
        except Exception as e:  # noqa: BLE001  (a tree without list keys)
            rec["unsupported"] = f"{type(e).__name__}: {e}"[:120]
            print(json.dumps(rec), flush=True)
            continue
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            res = run()
            times.append(time.perf_counter() - t0)
        rec["ms"] = [round(1e3 * t, 3) for t in times]
        rec["hbm_result"] = all(isinstance(c, DeviceArray) for c in res.columns.values())
        h = hashlib.sha256()
        for k in names:
            c = res.columns[k]
            h.update(np.ascontiguousarray(c.to_numpy() if isinstance(c, DeviceArray) else c).tobytes())
        rec["sha"] = h.hexdigest()[:16]
        _lib.timing_enable(True)
        _lib.timing_reset()
        run()
        rec["stages_ms"] = {s: round(_lib.timing_read(s)[1], 3) for s in STAGES if _lib.timing_read(s)[0]}
        _lib.timing_enable(False)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sort_ab.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    if args.child:
        return child(args)
    trees = [("this", HERE)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
    recs = []
    for _ in range(args.rounds):
        for label, tree in trees:  # alternating
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--label", label,
                                  "--rows", str(args.rows), "--repeats", str(args.repeats)],
                                 capture_output=True, text=True, timeout=900)
            if out.returncode:
                raise SystemExit(f"{label}: child failed\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
            recs += [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    lines = [f"sort_ab: {args.rows} rows, {args.rounds} rounds x {args.repeats} timed calls per tree and case (ms, host clock "
             "around df.sort + synchronise; one warm-up call before)"]
    for case in dict.fromkeys(r["case"] for r in recs):
        med = {}
        for label, _ in trees:
            rs = [r for r in recs if r["case"] == case and r["tree"] == label]
            if "unsupported" in rs[0]:
                lines.append(f"{case:7s} {label:6s} unsupported: {rs[0]['unsupported']}")
                continue
            per_round = [statistics.median(r["ms"]) for r in rs]
            every = [t for r in rs for t in r["ms"]]
            med[label] = statistics.median(every)
            lines.append(f"{case:7s} {label:6s} median {med[label]:9.3f}  rounds {per_round}  min {min(every):.3f} max {max(every):.3f}"
                         f"  hbm_result={rs[0]['hbm_result']} sha={rs[0]['sha']}")
            if rs[0]["stages_ms"]:
                lines.append(f"{'':14s} stages of one call: " + "  ".join(f"{k} {v:.3f}" for k, v in rs[0]["stages_ms"].items()))
        if len(med) == 2:
            same = len({r["sha"] for r in recs if r["case"] == case and "sha" in r}) == 1
            lines.append(f"{case:7s} parent / this = {med['parent'] / med['this']:.1f}x   results identical: {same}")
    this = {c: statistics.median([t for r in recs if r["case"] == c and r["tree"] == "this" and "ms" in r for t in r["ms"]])
            for c in ("i32x2", "i32x2w")}
    lines.append(f"two rounds / one round (i32x2w / i32x2, this tree) = {this['i32x2w'] / this['i32x2']:.2f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
