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


def test_every_kernel_descriptor_resolves():
    res = _run("resolve")
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    accepted = int(res.stdout.split()[0])
    assert accepted > 200, res.stdout
