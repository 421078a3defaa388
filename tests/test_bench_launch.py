"""bench.py's own N-rank launcher (CPU, no GPU call): ``--gpus N`` without WORLD_SIZE starts N
rank processes with distinct RANK / LOCAL_RANK, one shared MASTER_ADDR / MASTER_PORT and
WORLD_SIZE = N, and fails when a rank fails.  ``--dry-launch`` stops every rank before it
imports vaex_amd.

On a GPU: a plain run prints the headline line only and ``--dump-outputs`` writes the last
timed step's grids; ``--full`` adds the roofline and the property checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, BENCH, *extra], capture_output=True, text=True, env=env, timeout=120)


def test_launcher_starts_n_ranks():
    r = _run("--gpus", "4", "--dry-launch")
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert sorted(l["rank"] for l in lines) == [0, 1, 2, 3]
    assert sorted(l["local_rank"] for l in lines) == [0, 1, 2, 3]
    assert {l["world"] for l in lines} == {4}
    assert {l["master_addr"] for l in lines} == {"127.0.0.1"}
    assert len({l["master_port"] for l in lines}) == 1
    assert len({l["pid"] for l in lines}) == 4 and os.getpid() not in {l["pid"] for l in lines}


def test_launcher_fails_when_a_rank_fails():
    r = _run("--gpus", "3", "--dry-launch", "--dry-launch-fail-rank", "2")
    assert r.returncode != 0
    assert "rank 2 exited" in r.stderr


def test_single_gpu_runs_in_process():
    r = _run("--gpus", "1", "--dry-launch")
    assert r.returncode == 0
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["world"] == 1 and lines[0]["rank"] == 0


def test_under_an_external_launcher_no_relaunch():
    env = dict(os.environ, WORLD_SIZE="2", RANK="1", LOCAL_RANK="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-launch"], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["rank"] == 1 and lines[0]["world"] == 2


def _result_line(r):
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


SMALL = ("--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", "300001", "--bins", "61")


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run holds the headline figure and none of the --full legs; the dumped grids are
    the timed step's (float64, every row in one cell, sum(w) of U[0, 1) draws), and a second
    run with the same arguments computes the same grids (counts exactly; the sums' atomic
    adds may reorder: 300001 float64 terms in [0, 1), far inside rtol 1e-12)."""
    d = _result_line(_run(*SMALL, "--dump-outputs", str(tmp_path / "a")))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "rows/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(300001 / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["roofline"] is None and d["cpu_baseline"] is None and "check" not in d
    for leg in ("zero_d", "count_only", "groupby", "c2_float32", "filtered", "aggs", "h2o", "c4", "c1"):
        assert leg not in d, leg
    assert sorted(os.listdir(tmp_path / "a")) == ["count.npy", "sum.npy"]
    count, total = np.load(tmp_path / "a" / "count.npy"), np.load(tmp_path / "a" / "sum.npy")
    assert count.dtype == np.float64 and total.dtype == np.float64
    assert count.shape == (64, 64) and total.shape == (64, 64)
    assert count.sum() == 300001
    assert 0.49 * 300001 < total.sum() < 0.51 * 300001
    assert np.all(total[count == 0] == 0)
    _result_line(_run(*SMALL, "--dump-outputs", str(tmp_path / "b")))
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "count.npy"), count)
    np.testing.assert_allclose(np.load(tmp_path / "b" / "sum.npy"), total, rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_full_run_adds_roofline_and_checks():
    d = _result_line(_run(*SMALL, "--full", "--no-cpu-baseline", "--no-groupby", "--no-layouts", "--no-aggs", "--no-set",
                          "--no-count-only", "--no-f32", "--no-filtered", "--host-rows", "0", "--c4-rows", "0",
                          "--h2o-rows", "0"))
    assert d["full"] is True and d["steps"] == 3
    assert d["roofline"]["bound"] == "hbm" and "per_kernel_ms" in d["roofline"]
    assert d["check"]["ok"] is True and d["check"]["count_equal"] is True
    assert d["zero_d"]["count_equal"] is True
