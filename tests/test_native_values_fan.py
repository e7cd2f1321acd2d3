"""Runs the C test program of spfft_amd_multi_transform_accumulate_density_fan / apply_local_fan
(tests/native/test_values_fan.c, built by spfft_amd.build): the exported symbols of both
precisions, three transforms on two consecutive calls against single accumulate_density /
apply_local calls on premultiplied values, the error codes for a repeated grid, null
arrays, a null input, output, density or potential, a bad scaling, unequal transforms and
a null handle, n = 0 and n = 1, the fused query, and on the GPU box the same with host
pointers."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "spfft_amd", "_native")


def _run():
    prog = os.path.join(NATIVE, "spfft_values_fan_test")
    assert os.path.exists(prog), "spfft_values_fan_test not built"
    r = subprocess.run([prog], cwd=NATIVE, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failed" in out, out[-4000:]
    return out


def test_native_values_fan_host():
    out = _run()
    for real in ("double", "float"):
        assert f"density_fan {real} host complex 1 null 1 rep 1" in out
        assert f"apply_local_fan {real} host complex 1 null 1 scaling 1 rep 1" in out


@pytest.mark.gpu
def test_native_values_fan_gpu(gpu):
    out = _run()
    assert "SKIP" not in out
    for real in ("double", "float"):
        assert f"density_fan {real} gpu complex 1 null 1 rep 1" in out
        assert f"apply_local_fan {real} gpu complex 1 null 1 scaling 1 rep 1" in out
