"""The string transforms of csrc/str_dev.hpp on the CPU: the check program
(tests/host/strfn_check.hip, built by the default make next to the library) runs every
out_len / write pair -- the functions the kernels of csrc/strfn.hip inline -- against naive byte
loops, each input in a block of exactly its aligned words and each destination in a block of
exactly out_len bytes; every line it prints must end in ok."""
import os
import subprocess

CHECK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vaex_amd", "strfn_check")
FUNCTIONS = ("lower", "upper", "slice", "strip", "pad", "repeat", "cat", "replace")


def test_every_case_is_ok():
    assert os.path.exists(CHECK), f"{CHECK} is missing: build the library (make -C vaex_amd/csrc)"
    p = subprocess.run([CHECK], capture_output=True, text=True)
    lines = p.stdout.splitlines()
    assert lines and lines[-1].startswith("cases "), p.stdout[-500:] + p.stderr[-500:]
    cases = lines[:-1]
    bad = [ln for ln in cases if not ln.endswith(" ok")]
    assert not bad, bad[:10]
    assert p.returncode == 0
    assert lines[-1] == f"cases {len(cases)} failed 0"
    # every transform over every alignment of every short length, the multi-byte and malformed
    # rows, and the long row
    assert "repeat saturates ok" in cases and "pad saturates ok" in cases
    for fn in FUNCTIONS:
        for length in range(18):
            for align in range(8):
                assert f"{fn} edge_len{length}_at{align} ok" in cases, (fn, length, align)
        for name in ("dotted_I_shrinks", "sharp_s_grows", "turned_a", "deseret", "euro", "clef", "truncated2", "truncated3",
                     "truncated4", "stray", "stray_end", "interrupted", "overlong", "long70000"):
            assert any(ln.startswith(f"{fn} {name}_at") for ln in cases), (fn, name)
