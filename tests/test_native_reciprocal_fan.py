"""Runs the C test program of spfft_amd_multi_transform_reciprocal_fan_out / fan_in (tests/
native/test_reciprocal_fan.c, built by spfft_amd.build): the exported symbols of both
precisions, three transforms on two consecutive calls against single apply_reciprocal
calls, the values output, the error codes for a repeated grid, null arrays, a null entry,
a bad scaling, unequal transforms and a null handle, n = 0 and n = 1, the fused query,
and on the GPU box the same with host pointers."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "spfft_amd", "_native")


def _run():
    prog = os.path.join(NATIVE, "spfft_reciprocal_fan_test")
    assert os.path.exists(prog), "spfft_reciprocal_fan_test not built"
    r = subprocess.run([prog], cwd=NATIVE, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failed" in out, out[-4000:]
    return out


def test_native_reciprocal_fan_host():
    out = _run()
    for op in ("fan_out", "fan_in"):
        assert f"reciprocal_{op} double host complex 1 scaling 1 rep 1" in out
        assert f"reciprocal_{op} float host complex 1 scaling 1 rep 1" in out


@pytest.mark.gpu
def test_native_reciprocal_fan_gpu(gpu):
    out = _run()
    assert "SKIP" not in out
    for op in ("fan_out", "fan_in"):
        assert f"reciprocal_{op} double gpu complex 1 scaling 1 rep 1" in out
        assert f"reciprocal_{op} float gpu complex 1 scaling 1 rep 1" in out
