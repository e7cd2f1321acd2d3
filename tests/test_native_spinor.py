"""Runs the C test program of spfft_amd_multi_transform_apply_local_spinor /
accumulate_spin_density (tests/native/test_spinor.c, built by spfft_amd.build): the exported
symbols of both precisions, two spinors on two consecutive calls (bit for bit) against direct
sums, both scalings, out == in, repeated potential pointers, the error codes for an R2C
member, a repeated grid, unequal transforms, null arrays and entries, equal density
pointers, a bad scaling and a null handle, nSpinors = 0, the fused query, and on the GPU box
the same with host pointers (composed) and with device pointers (the fused x kernels)."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "spfft_amd", "_native")


def _run():
    prog = os.path.join(NATIVE, "spfft_spinor_test")
    assert os.path.exists(prog), "spfft_spinor_test not built"
    r = subprocess.run([prog], cwd=NATIVE, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failed" in out, out[-4000:]
    return out


def test_native_spinor_host():
    out = _run()
    for real in ("double", "float"):
        assert f"apply_local_spinor {real} host case 2 rep 1" in out
        assert f"accumulate_spin_density {real} host rep 1" in out


@pytest.mark.gpu
def test_native_spinor_gpu(gpu):
    out = _run()
    assert "SKIP" not in out
    for real in ("double", "float"):
        for where in ("gpu-host", "gpu-device"):
            assert f"apply_local_spinor {real} {where} case 2 rep 1" in out
            assert f"accumulate_spin_density {real} {where} rep 1" in out
