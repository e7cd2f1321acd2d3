"""Runs the C test program of spfft_amd_transform_accumulate_fock (tests/native/
test_fock.c, built by spfft_amd.build): the exported symbols, the host composition
against direct sums on two consecutive calls, the error codes for null arrays, a
null kernel, a bad scaling, a null handle and a null fused pointer, and on the GPU
box the fused path with host pointers."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "spfft_amd", "_native")


def _run():
    prog = os.path.join(NATIVE, "spfft_fock_test")
    assert os.path.exists(prog), "spfft_fock_test not built"
    r = subprocess.run([prog], cwd=NATIVE, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failed" in out, out[-4000:]
    return out


def test_native_fock_host():
    assert "accumulate_fock host complex 1 scaling 1 rep 1" in _run()


@pytest.mark.gpu
def test_native_fock_gpu(gpu):
    out = _run()
    assert "accumulate_fock gpu complex 1 scaling 1 rep 1" in out and "SKIP" not in out
