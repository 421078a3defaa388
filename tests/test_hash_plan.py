"""The hash partition's host planner (vaex_amd/csrc/hash_plan.hpp), shared by the fused hash
groupby and the ordered set, without a GPU, through its check program
(tests/host/hash_plan_check.hip, built by the default make next to the library).

Every decision -- sample geometry, distinct-key estimate, p_log2, pass-A grid, region
capacities and offsets, the refusal of a region table that is too large, pass-B units, the meta
layouts, hashagg's repartition -- over a matrix of sample read-backs equals, character for
character, what the two engines' own arithmetic gave before it was moved into the header
(tests/golden/hash_plan_cases.txt, whose first line names that commit).  The program also
checks the planner's invariants on every accepted case on its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "vaex_amd", "hash_plan_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "hash_plan_cases.txt")


def test_planner_decisions_match_the_recorded_ones():
    with open(GOLDEN) as f:
        header, *want = f.read().splitlines()
    assert header.startswith("# planner decisions of commit ")
    res = subprocess.run([CHECK], capture_output=True, text=True, timeout=300)
    got = res.stdout.splitlines()
    assert len(got) == len(want), f"{len(got)} cases printed, {len(want)} recorded"
    for g, w in zip(got, want):
        assert g == w, f"case {w.split(' ', 1)[0]} differs"
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    # the matrix reaches what it is there for
    assert sum("refused: region table too large" in w for w in want) > 0
    assert {" p=0 ", " p=1 ", " p=11 "} <= {f" {t} " for w in want for t in w.split() if t.startswith("p=")}
    assert {"S=1", "S=64"} <= {t for w in want for t in w.split() if t.startswith("S=")}
