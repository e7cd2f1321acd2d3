"""Runs the C test program of spfft_amd_transform_apply_reciprocal (tests/native/
test_reciprocal.c, built by spfft_amd.build): the exported symbols, the host
composition against direct sums, the error codes for a null kernel, a null handle
and a null fused pointer, and on the GPU box the fused path."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "spfft_amd", "_native")


def _run():
    prog = os.path.join(NATIVE, "spfft_reciprocal_test")
    assert os.path.exists(prog), "spfft_reciprocal_test not built"
    r = subprocess.run([prog], cwd=NATIVE, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failed" in out, out[-4000:]
    return out


def test_native_reciprocal_host():
    assert "apply_reciprocal host complex 1 scaling 1 rep 1" in _run()


@pytest.mark.gpu
def test_native_reciprocal_gpu(gpu):
    out = _run()
    assert "apply_reciprocal gpu complex 1 scaling 1 rep 1" in out and "SKIP" not in out
