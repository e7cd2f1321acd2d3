"""Runs the C test program of spfft_amd_multi_transform_accumulate_fock (tests/native/
test_fock_multi.c, built by spfft_amd.build): the exported symbols of both precisions,
three transforms into one acc on two consecutive calls against the same pairs as single
calls, the error codes for a repeated grid, null arrays, a null entry, a bad scaling and a
null handle, n = 0, and on the GPU box the same with host pointers."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "spfft_amd", "_native")


def _run():
    prog = os.path.join(NATIVE, "spfft_fock_multi_test")
    assert os.path.exists(prog), "spfft_fock_multi_test not built"
    r = subprocess.run([prog], cwd=NATIVE, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failed" in out, out[-4000:]
    return out


def test_native_fock_multi_host():
    out = _run()
    assert "multi_accumulate_fock double host complex 1 scaling 1 rep 1" in out
    assert "multi_accumulate_fock float host complex 1 scaling 1 rep 1" in out


@pytest.mark.gpu
def test_native_fock_multi_gpu(gpu):
    out = _run()
    assert "multi_accumulate_fock double gpu complex 1 scaling 1 rep 1" in out and "SKIP" not in out
    assert "multi_accumulate_fock float gpu complex 1 scaling 1 rep 1" in out
