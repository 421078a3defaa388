"""The tiled engine's host planner (vaex_amd/csrc/tile_plan.hpp) without a GPU, through its
check program (tests/host/tile_plan_check.hip, built by the default make next to the library).

* Every decision of the three stages -- slots, tiles, LDS sizes, the pass-A / pass-B kernels,
  grid, layout, region capacities, work units -- over a matrix of plans equals, character for
  character, what the decision code gave before it was split out of tiled.hip
  (tests/golden/tile_plan_cases.txt, whose first line names that commit).  The program also
  checks each accepted case against the kernel / plan invariant on its own.
* Every kernel descriptor the matrix produces resolves to a kernel of libvaexhip.so."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "vaex_amd", "tile_plan_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tile_plan_cases.txt")


def _run(*args):
    return subprocess.run([CHECK, *args], capture_output=True, text=True, timeout=300)


def test_planner_decisions_match_the_recorded_ones():
    with open(GOLDEN) as f:
        header, *want = f.read().splitlines()
    assert header.startswith("# planner decisions of commit ")
    res = _run()
    got = res.stdout.splitlines()
    assert len(got) == len(want), f"{len(got)} cases printed, {len(want)} recorded"
    for g, w in zip(got, want):
        assert g == w, f"case {w.split(' ', 1)[0]} differs"
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]


def test_stream_round_shapes_walk_several_rounds():
    """The (plan, rows) pairs of tests/test_gpu_stream_rounds.py (tests/stream_rounds_cases.py)
    through stages 1-3 with a sample of cold tiles, 256 CUs, pass-A occupancy 1..4: each takes
    the stream layout and has a work unit of at least two rounds of TB_SEGS segments, the pairs
    meant for the ceiling exactly TB_ROUNDS * TB_THREADS / TB_SEGS, and the tail pairs leave
    pass-A workgroups with different commit counts -- so a change of VH_TA_SB, TA_BATCH or
    TB_ROUNDS cannot make the GPU tests vacuous unnoticed."""
    from stream_rounds_cases import CASES, TAIL_CASES
    res = _run("rounds", *[f"{plan}={n}" for plan, n, _ in CASES.values()])
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    head, *lines = res.stdout.splitlines()
    ceiling = int(head.split("ceiling=")[1])
    assert len(lines) == len(CASES)
    for (name, (plan, n, want)), line in zip(CASES.items(), lines):
        first, *occs = line.split(" | ")
        assert first.split()[0] == plan and f"n={n - n % 2}" in first.split(), line
        assert len(occs) == 4
        for occ in occs:
            f = dict(kv.split("=") for kv in occ.split()[1:])
            assert f["st"] == "1", f"{name}: no stream layout: {line}"
            if want is None:
                assert int(f["rounds"]) >= 2, f"{name}: {line}"
            else:
                assert int(f["rounds"]) == want == ceiling, f"{name}: {line}"
            if name in TAIL_CASES:
                assert f["tail"] == "1", f"{name}: equal commit counts: {line}"


def test_every_kernel_descriptor_resolves():
    res = _run("resolve")
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    accepted = int(res.stdout.split()[0])
    assert accepted > 200, res.stdout
