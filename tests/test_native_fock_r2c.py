"""Runs the C test program of spfft_amd_transform_fock_r2c_fused (tests/native/
test_fock_r2c.c, built by spfft_amd.build): the exported symbols of both precisions, the
error codes for a null fused pointer and a null handle, a host R2C transform that reports 0,
and on the GPU box a 64x13x5 R2C transform that reports 1 and whose accumulate_fock with
host pointers agrees on two consecutive calls with the composition of the public forward,
a host loop over the values, backward and a host loop."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "spfft_amd", "_native")


def _run():
    prog = os.path.join(NATIVE, "spfft_fock_r2c_test")
    assert os.path.exists(prog), "spfft_fock_r2c_test not built"
    r = subprocess.run([prog], cwd=NATIVE, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failed" in out, out[-4000:]
    return out


def test_native_fock_r2c_host():
    assert "fock_r2c_fused host: 0" in _run()


@pytest.mark.gpu
def test_native_fock_r2c_gpu(gpu):
    out = _run()
    assert "accumulate_fock r2c gpu complex 1 scaling 1 rep 1" in out and "SKIP" not in out
