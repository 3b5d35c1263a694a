"""CPU: the per-threshold cutoff of the two-bitmap AND kernel's weight bound (mrk::bm_wmax_cut, csrc/mrk_kcommon.h), host code under
AddressSanitizer + UBSan (tests/cpp/bm_cut.cpp, a stand-alone program).  `x < bm_wmax_cut(..)` decides as the kernel's former per-word
expression, kept verbatim in the program, for every bin geometry of the grid (index weights 1 .. 65535, field weights of either sign and
zero, bin_lo < 0 and T <= 0, shifts 0 .. 22, ranges up against the int32 ends the planner accepts), every tau_bin of 0, 1, 2, 511, 1022,
1023, at the cutoff's neighbours, the ends of the reachable range and seeded random values."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only program")
def test_cutoff_equals_parent_expression(tmp_path):
    # (the library's own arithmetic flags: no contraction)
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
             "-fno-sanitize-recover=undefined"]
    obj = str(tmp_path / "bm_cut.o")
    subprocess.check_call([HIPCC] + flags + ["-c", os.path.join(HERE, "cpp", "bm_cut.cpp"), "-o", obj])
    exe = str(tmp_path / "bm_cut")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize", obj, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    lines = out.stdout.split("\n")
    assert lines[0].startswith("compared ") and lines[1] == "ok", out.stdout
    f = lines[0].split()
    # compared N geometries G lo<0 A T<=0 B
    assert int(f[1]) > 2_000_000 and int(f[3]) > 1000 and int(f[5]) > 100 and int(f[7]) > 100, out.stdout
