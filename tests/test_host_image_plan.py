"""The host arithmetic of the host-image mirror (vaex_amd/csrc/tile_plan.hpp: count_tile_units,
tile_cells, mirror_uncovered) without a GPU, through its check program
(tests/host/host_image_check.hip, built by the default make next to the library): over
count / count+sum plans on the stream and the regions layout, samples with hot, missed and
empty tiles, and unit tables with tiles left out, the per-tile unit counts add up to the
planned units, every cell of the grid is written exactly once -- by the last unit of its
tile or by one of the host's copies -- and the mirrored launch order is a permutation of the
planned units with the cold tiles' units first."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "vaex_amd", "host_image_check")


def test_unit_counts_and_cell_cover():
    res = subprocess.run([CHECK], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert lines[-1] == "ok"
    cases = [ln for ln in lines[:-1] if not ln.startswith("FAILED")]
    assert len(cases) == len(lines) - 1 and len(cases) > 100
    order = [ln for ln in cases if "/order " in ln]
    cases = [ln for ln in cases if "/order " not in ln]
    fields = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in cases]
    planned = [f for ln, f in zip(cases, fields) if "/drop" not in ln and "/no-units" not in ln]
    assert planned and all(f["uncovered"] == "0" and f["host_cells"] == "0" for f in planned)  # plan_units covers every tile
    assert any(int(f["most"]) >= 2 for f in planned)              # tickets shared by several units
    assert any(int(f["uncovered"]) >= 2 and f["host_ranges"] == "1" for f in fields)  # adjacent tiles: one copy
    assert any(int(f["host_ranges"]) >= 2 for f in fields)
    # the mirrored launch order moved cold tiles' units to the front in some case, and not all of them
    moved = [int(ln.split("cold_units=")[1].split()[0]) for ln in order]
    assert len(order) == len(planned) and any(m > 0 for m in moved)
