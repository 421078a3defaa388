"""csrc/str_dev.hpp on the CPU: the check program (tests/host/str_check.hip, built by the
default make next to the library) compares the header's hash, equality, code-point count and
literal search -- the functions the device string kernels inline -- with naive byte loops over
the edge strings; every line it prints must end in ok."""
import os
import subprocess

CHECK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vaex_amd", "str_check")


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
    # every function of the header is covered, at every alignment of every short length
    for fn in ("load_word", "hash", "equal", "count_codepoints", "find", "match", "slot_key", "take_needs_wide"):
        assert any(ln.startswith(fn + " ") for ln in cases), fn
    for length in range(18):
        for align in range(8):
            assert any(ln.startswith("hash ") and ln.endswith(f"_len{length}_at{align} ok") for ln in cases), (length, align)
    assert any("long70000" in ln for ln in cases)
