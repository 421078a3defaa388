"""csrc/mask_dev.hpp on the CPU: the check program (tests/host/mask_check.hip, built by the
default make next to the library) compares the header's validity-bitmap unpack / pack and the
missing count -- the functions the kernels of missing.hip inline -- with a naive bit loop; every
line it prints must end in ok."""
import os
import subprocess

CHECK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vaex_amd", "mask_check")


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
    assert "expand8 every_byte ok" in cases and "pack8 any_nonzero_byte ok" in cases
    # every bit offset at every length, both directions and the round trip
    for fn in ("unpack", "pack", "roundtrip", "count"):
        for offset in range(16):
            for length in (0, 1, 7, 8, 9, 63, 64, 65, 2051):
                assert f"{fn} off{offset}_len{length} ok" in cases, (fn, offset, length)
