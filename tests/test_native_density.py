"""Runs the C test program of spfft_amd_transform_accumulate_density (tests/native/
test_density.c, built by spfft_amd.build): the exported symbols, the host
composition against a direct sum, the error codes for a null density and a null
handle, and on the GPU box the fused path."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "spfft_amd", "_native")


def _run():
    prog = os.path.join(NATIVE, "spfft_density_test")
    assert os.path.exists(prog), "spfft_density_test not built"
    r = subprocess.run([prog], cwd=NATIVE, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failed" in out, out[-4000:]
    return out


def test_native_density_host():
    assert "accumulate_density host rep 2" in _run()


@pytest.mark.gpu
def test_native_density_gpu(gpu):
    out = _run()
    assert "accumulate_density gpu rep 2" in out and "SKIP" not in out
