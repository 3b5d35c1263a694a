"""CPU: a query's decline mask -- which of its three exchange rows (narrow, wide, order) leave a batch with MRK_ROW_DECLINED.  The host
function (csrc/mrk_host_int.h: row_decline_mask) is compiled into tests/cpp/row_declines.cpp, host only, under ASan + UBSan, and held
there against a table written out from the rule, over every combination of status, order kind, sort bits and the weight-first switch."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only program")
def test_decline_mask_equals_the_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "row_declines")
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(HERE, "cpp", "row_declines.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.splitlines()[-1] == "ok row declines 32 combinations", out.stdout[-3000:]
