"""Randomised sweeps of tools/fuzz_ops.py inside the suites: apply_local,
accumulate_density, apply_reciprocal and accumulate_fock over every engine path, type,
precision, 1-3 ranks with random (skewed, empty) distributions, every exchange type, forced
exchange chunks, capped intermediates, host pointers and multi_transform batches, against
the dense numpy oracle in double precision.

Bounds: the sweep's 1e-10 (fp64) and 2e-4 (fp32 or a *_FLOAT exchange) on max_rel_error.
Every test prints its largest error per precision (-s). Measured over 1400 random cases
of the command-line sweep, lengths 8192 and 4099 included: at most 7.0e-15 (fp64) and
1.5e-6 (fp32 or a *_FLOAT exchange) on the MI355X, 2.6e-15 and 1.5e-6 on the host engine
for the pinned cases; accumulate_density and accumulate_fock are the largest."""
import importlib.util
import os
import sys
import time

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPS = ("local", "density", "reciprocal", "fock")
SEEDS = {"local": 368, "density": 40, "reciprocal": 203, "fock": 81}
BLOCKS, PER_BLOCK = 4, 24
MAX_ELEMS = 1 << 16


def _mod():
    name = "fuzz_ops"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "tools", "fuzz_ops.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def _cases(op):
    """The pinned configurations of one operator, BLOCKS x PER_BLOCK."""
    mod = _mod()
    rng = np.random.default_rng(SEEDS[op])
    return [mod.draw_case(rng, op, MAX_ELEMS) for _ in range(BLOCKS * PER_BLOCK)]


def _coverage(cfgs):
    """How many of the drawn configurations have each property the sweep must reach."""
    mod = _mod()
    n = dict.fromkeys(["unbuffered", "float exchange", "r2c distributed", "fp32 distributed",
                       "planes but no sticks", "sticks but no planes", "long y or z beside short x",
                       "long x", "z fill 1.0", "forced chunks", "capped intermediate", "multi"], 0)
    for c in cfgs:
        P, dist = c["P"], c["P"] > 1
        planes = mod.planes_of(c)
        nx, ny, nz = c["dims"]
        n["unbuffered"] += dist and c["exchange"] == "UNBUFFERED"
        n["float exchange"] += dist and c["exchange"].endswith("FLOAT")
        n["r2c distributed"] += dist and c["r2c"]
        n["fp32 distributed"] += dist and c["single"]
        n["planes but no sticks"] += any(planes[r] > 0 and c["stick_dist"][r] == 0 for r in range(P))
        n["sticks but no planes"] += any(planes[r] == 0 and c["stick_dist"][r] > 0 for r in range(P))
        n["long y or z beside short x"] += (not c["r2c"] and nx in mod.SHORT
                                            and (ny in mod.LONG or nz in mod.LONG))
        n["long x"] += nx in mod.LONG
        n["z fill 1.0"] += c["z_fill"] == 1.0
        n["forced chunks"] += dist and c["chunks"] > 1
        n["capped intermediate"] += c["cap_planes"] > 0
        n["multi"] += c["multi"]
    return n


@pytest.mark.parametrize("op", OPS)
def test_draw_coverage(op):
    """The pinned seed of each operator draws every configuration class at least once
    (judged from the drawn choices alone, no library call)."""
    cov = _coverage(_cases(op))
    print(op, cov)
    if op in ("reciprocal", "fock"):
        assert cov.pop("multi") == 0  # no multi_transform entry point for these
    missing = [k for k, v in cov.items() if v < 1]
    assert not missing, missing


_RESULTS = {}  # (op, block, host) -> (seconds, [(desc, err, tol, facts)])


def _run_block(op, block, host):
    key = (op, block, host)
    if key not in _RESULTS:
        mod = _mod()
        out = []
        t0 = time.time()
        for cfg in _cases(op)[block * PER_BLOCK:(block + 1) * PER_BLOCK]:
            out.append(mod.run_case(cfg, host=host))  # an exception fails the test
        _RESULTS[key] = (time.time() - t0, out)
    return _RESULTS[key]


def _check(op, blocks, host):
    bad, worst = [], {}
    for b in blocks:
        seconds, out = _run_block(op, b, host)
        print(f"{op} block {b} {'host' if host else 'gpu'}: {len(out)} cases in {seconds:.2f} s")
        for desc, err, tol, _ in out:
            if not err < tol:
                bad.append(f"{desc} err={err:.2e} tol={tol:.0e}")
            key = "fp32 or float exchange" if tol > 1e-6 else "fp64"
            worst[key] = max(worst.get(key, 0.0), err)
    for key, e in sorted(worst.items()):
        print(f"largest error {op} {key}: {e:.2e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("op", OPS)
def test_fuzz_ops_host(op):
    """The pinned cases on the host engine: the plain compositions on skewed splits, and
    an independent engine inside the bounds on exactly these inputs."""
    _check(op, range(BLOCKS), True)


@pytest.mark.gpu
@pytest.mark.parametrize("block", range(BLOCKS))
@pytest.mark.parametrize("op", OPS)
def test_fuzz_ops_gpu(gpu, op, block):
    _check(op, [block], False)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_fuzz_ops_gpu_paths(gpu, op):
    """The paths the sweep exists for really ran: peer writes, K > 1 plane chunks, fused
    and composed plans, ranks without planes and without values; and the z stage never
    runs fused under peer writes or a *_FLOAT exchange."""
    cfgs = _cases(op)
    seen = dict.fromkeys(["peer writes", "chunks > 1", "fused", "composed", "z fused", "z composed",
                          "zero planes", "zero values"], 0)
    for b in range(BLOCKS):
        _, out = _run_block(op, b, False)
        for cfg, (desc, _, _, facts) in zip(cfgs[b * PER_BLOCK:(b + 1) * PER_BLOCK], out):
            for f in facts:
                K, _, peer, _ = f["plan"]
                seen["peer writes"] += peer
                seen["chunks > 1"] += K > 1
                seen["fused"] += f["fused"]
                seen["composed"] += not f["fused"]
                seen["z fused"] += f["reciprocal_fused"]
                seen["z composed"] += not f["reciprocal_fused"]
                seen["zero planes"] += f["planes"] == 0
                seen["zero values"] += f["values"] == 0
                if peer or (cfg["P"] > 1 and cfg["exchange"].endswith("FLOAT")):
                    assert f["reciprocal_fused"] is False, desc
    print(op, seen)
    if op in ("local", "density"):  # their calls have no z stage of their own
        del seen["z fused"], seen["z composed"]
    missing = [k for k, v in seen.items() if v < 1]
    assert not missing, missing
