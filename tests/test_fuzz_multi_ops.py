"""Randomised sweeps of tools/fuzz_multi_ops.py inside the suites: the seven operators on
multi_transform member lists (accumulate_fock, reciprocal fan-out and fan-in, the density
and apply-local value fans, the spinor potential and the spin density) over every engine
path, type, precision, 1-3 ranks with random (skewed, empty) distributions, every exchange
type, forced exchange chunks, capped intermediates, host pointers, member counts inside,
at the edge of and beyond one batch, None and repeated kernels, shared and in-place arrays,
against the dense numpy oracle in double precision.

Bounds: the project's pinned-test bounds 1e-12 (fp64) and 2e-5 (fp32 or a *_FLOAT exchange)
on max_rel_error. Every test prints its largest error per precision (-s).

Measured largest errors, fp64 / fp32 or a *_FLOAT exchange, none above a tenth of its bound:

                 pinned cases, MI355X   pinned cases, host     700 random cases (--seed 1)
                                                               MI355X               host
    fock_multi   1.15e-15 / 5.82e-07    1.08e-15 / 4.30e-07    1.15e-15 / 6.66e-07  1.00e-15 / 4.38e-07
    fan_out      1.18e-15 / 4.84e-07    1.42e-15 / 3.95e-07    1.14e-15 / 5.11e-07  1.13e-15 / 3.61e-07
    fan_in       1.18e-15 / 5.78e-07    1.18e-15 / 3.78e-07    1.47e-15 / 5.14e-07  1.21e-15 / 3.60e-07
    density_fan  2.31e-15 / 4.82e-07    1.96e-15 / 3.94e-07    2.49e-15 / 1.26e-06  3.04e-15 / 1.04e-06
    local_fan    1.33e-15 / 4.58e-07    1.14e-15 / 3.21e-07    9.62e-16 / 4.79e-07  1.28e-15 / 4.29e-07
    spinor_local 1.32e-15 / 4.73e-07    1.27e-15 / 4.09e-07    1.18e-15 / 5.43e-07  1.20e-15 / 4.27e-07
    spin_density 1.42e-15 / 5.75e-07    1.42e-15 / 4.63e-07    1.56e-15 / 6.18e-07  1.56e-15 / 4.23e-07

The 700 random cases of the command-line sweep (100 per operator) all pass on both engines,
and so do 700 more at --seed 2, 350 at --seed 3 --max-elems 262144 and 1400 each at --seed 4
and --seed 5 on the MI355X (at most 2.69e-15 and 1.06e-06).

Time on the MI355X, one run of the whole suite: the slowest block of test_fuzz_ops_gpu takes
0.65 s (local-1; 0.98 s for local-0 when the module runs alone and its first call warms the
library up). The slowest blocks here, in seconds: fock_multi 0.43, fan_out 0.31, fan_in 0.29,
density_fan 0.36, local_fan 0.35, spinor_local 0.38, spin_density 0.53 (0.61 for fock_multi-0
with the warm-up when this module runs alone). Times vary by a factor of about 1.6 between
machines. The host sweep of the seven operators takes 25 s.

With one line of a batch path broken in a scratch build (another member's kernel in the pair
batch's z stage, in the fan-in sum and in the density fan's z fan-out; up and down swapped in
the spinor x stage) 4, 6, 5 and 8 of the operator's pinned GPU blocks fail, counted when the
96 cases ran as 8 blocks of 12.
"""
import importlib.util
import os
import sys
import time

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPS = ("fock_multi", "fan_out", "fan_in", "density_fan", "local_fan", "spinor_local", "spin_density")
SEEDS = {"fock_multi": 104, "fan_out": 200, "fan_in": 300, "density_fan": 401, "local_fan": 505,
         "spinor_local": 600, "spin_density": 702}
# BLOCKS[op] blocks of PER_BLOCK[op] cases. A case runs up to ten grids per rank, so the
# blocks are a third as long as those of test_fuzz_ops.py and there are three times as many:
# at 8 cases every operator's slowest block stays near the slowest block of
# test_fuzz_ops_gpu (the times above), where the limit for a new test is twice that.
PER_BLOCK = dict.fromkeys(OPS, 8)
BLOCKS = dict.fromkeys(OPS, 12)
MAX_ELEMS = 1 << 16
FANS = ("fan_out", "fan_in")
VALUE_FANS = ("density_fan", "local_fan")
SPINORS = ("spinor_local", "spin_density")


def _mod():
    name = "fuzz_multi_ops"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "tools", "fuzz_multi_ops.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def _cases(op, seed=None):
    """The pinned configurations of one operator, BLOCKS x PER_BLOCK."""
    mod = _mod()
    rng = np.random.default_rng(SEEDS[op] if seed is None else seed)
    return [mod.draw_case(rng, op, MAX_ELEMS) for _ in range(BLOCKS[op] * PER_BLOCK[op])]


def _batch_candidate(mod, c):
    """Whether the drawn choices allow the batch path: one rank, device arrays, lengths of
    one workgroup, the whole intermediate, a member count of one batch, simple sticks where
    the z stage must be fused, C2C where the batch is C2C only."""
    op, n = c["op"], c["n"]
    ok = (c["P"] == 1 and not c["host_ptrs"] and not c["unaligned"] and all(d in mod.SHORT for d in c["dims"])
          and (c["cap_planes"] == 0 or c["cap_planes"] >= c["dims"][2]))
    if op in SPINORS:
        return ok
    ok = ok and c["z_fill"] == 1.0 and n <= mod.MAX_BATCH
    if op in VALUE_FANS:
        return ok and not c["r2c"]
    return ok and n >= 2 and (op != "fock_multi" or not c["r2c"] or c["dims"][0] % 2 == 0)


def _coverage(op, cfgs):
    """How many of the drawn configurations have each property the sweep must reach."""
    mod = _mod()
    keys = ["unbuffered", "float exchange", "fp32 distributed", "planes but no sticks",
            "sticks but no planes", "long y or z beside short x", "long x", "z fill 1.0",
            "forced chunks", "capped intermediate", "host pointers", "n = 1", "largest batch",
            "beyond one batch", "batch candidates", "composed candidates on one rank"]
    if op in mod.R2C_OPS:
        keys += ["r2c distributed"]
    if op in FANS:
        keys += ["real kernels", "complex kernels", "repeated kernel"]
    if op == "fan_out":
        keys += ["values output", "no values output", "space passed", "space pre-filled"]
    if op == "fan_in":
        keys += ["spaces in full", "a None space", "host space domains"]
    if op in VALUE_FANS:
        keys += ["real kernels", "complex kernels", "grad kernels", "None kernel", "None kernel of member 0"]
    if op == "local_fan":
        keys += ["shared potential", "distinct potentials", "output is values", "None output kernel"]
    if op in SPINORS:
        keys += ["four arrays", "one [4, z, y, x] array"]
    if op == "spinor_local":
        keys += ["output is input"]
    if op == "fock_multi":
        keys += ["real kernels", "complex kernels", "shared b", "b per member", "a is b", "one kernel",
                 "kernel per member", "unaligned a", "unaligned b", "unaligned acc"]
    cov = dict.fromkeys(keys, 0)
    most = mod.MAX_SPINORS if op in SPINORS else mod.MAX_BATCH

    def add(key, hit):
        if key in cov:
            cov[key] += bool(hit)

    for c in cfgs:
        P, dist, n = c["P"], c["P"] > 1, c["n"]
        planes = mod.planes_of(c)
        nx, ny, nz = c["dims"]
        add("unbuffered", dist and c["exchange"] == "UNBUFFERED")
        add("float exchange", dist and c["exchange"].endswith("FLOAT"))
        add("r2c distributed", dist and c["r2c"])
        add("fp32 distributed", dist and c["single"])
        add("planes but no sticks", any(planes[r] > 0 and c["stick_dist"][r] == 0 for r in range(P)))
        add("sticks but no planes", any(planes[r] == 0 and c["stick_dist"][r] > 0 for r in range(P)))
        add("long y or z beside short x", not c["r2c"] and nx in mod.SHORT and (ny in mod.LONG or nz in mod.LONG))
        add("long x", nx in mod.LONG)
        add("z fill 1.0", c["z_fill"] == 1.0)
        add("forced chunks", dist and c["chunks"] > 1)
        add("capped intermediate", c["cap_planes"] > 0)
        add("host pointers", len(c["host_ptrs"]) > 0)
        add("n = 1", n == 1)
        add("largest batch", n == most)
        add("beyond one batch", n > most)
        add("batch candidates", _batch_candidate(mod, c))
        add("composed candidates on one rank",
            P == 1 and (c["host_ptrs"] or n > most or 0 < c["cap_planes"] < nz))
        add("real kernels", c["kind"] == "real")
        add("complex kernels", c["kind"] == "complex")
        add("grad kernels", c["kind"] == "grad")
        add("repeated kernel", c["repeat"])
        add("values output", c["values"])
        add("no values output", not c["values"])
        add("space passed", not c["prefill"])
        add("space pre-filled", c["prefill"])
        add("spaces in full", c["none_space"] < 0)
        add("a None space", c["none_space"] >= 0)
        add("host space domains", "space" in c["host_ptrs"])
        add("None kernel", any(c["none_in"][:n]))
        add("None kernel of member 0", c["none_in"][0])
        add("None output kernel", any(c["none_out"][:n]))
        add("shared potential", c["shared_pot"] and n > 1)
        add("distinct potentials", not c["shared_pot"] and n > 1)
        add("output is values", c["out_is_in"])
        add("output is input", c["out_is_in"])
        add("four arrays", c["four_list"])
        add("one [4, z, y, x] array", not c["four_list"])
        add("shared b", c["shared_b"] and n > 1)
        add("b per member", not c["shared_b"] and n > 1)
        add("a is b", any(c["same"][:n]))
        add("one kernel", not c["kernel_list"] and n > 1)
        add("kernel per member", c["kernel_list"] and n > 1)
        for name in ("a", "b", "acc"):
            add("unaligned " + name, c["unaligned"] == name)
    return cov


# more than one of what the GPU path test needs, so that a candidate the plans refuse (a
# length whose engine does not fit, a clamped chunk count) leaves another
AT_LEAST = {"unbuffered": 2, "forced chunks": 2, "batch candidates": 4, "composed candidates on one rank": 2,
            "planes but no sticks": 2, "sticks but no planes": 2}


def _missing(cov):
    return [k for k, v in cov.items() if v < AT_LEAST.get(k, 1)]


@pytest.mark.parametrize("op", OPS)
def test_draw_coverage(op):
    """The pinned seed of each operator draws every configuration class at least once
    (judged from the drawn choices alone, no library call)."""
    cov = _coverage(op, _cases(op))
    print(op, cov)
    assert not _missing(cov), _missing(cov)


_RESULTS = {}  # (op, block, host) -> (seconds, [(desc, err, tol, facts)])


def _run_block(op, block, host):
    key = (op, block, host)
    if key not in _RESULTS:
        mod = _mod()
        out = []
        t0 = time.time()
        for cfg in _cases(op)[block * PER_BLOCK[op]:(block + 1) * PER_BLOCK[op]]:
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
def test_fuzz_multi_ops_host(op):
    """The pinned cases on the host engine: the plain compositions on skewed splits, and
    an independent engine inside the bounds on exactly these inputs."""
    _check(op, range(BLOCKS[op]), True)


@pytest.mark.gpu
@pytest.mark.parametrize("op,block", [(op, b) for op in OPS for b in range(BLOCKS[op])])
def test_fuzz_multi_ops_gpu(gpu, op, block):
    _check(op, [block], False)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_fuzz_multi_ops_gpu_paths(gpu, op):
    """The paths the sweep exists for really ran: the batch launch, the composition on one
    GPU, peer writes, K > 1 plane chunks, ranks without planes and without values; and on
    one GPU with device arrays the plan flag and the route agree: a true flag and a member
    count of one batch run the batch scope once per call and group (fan-out and fan-in of
    one member are apply_reciprocal and run none; the pair operator batches groups of two
    and more members of batchable plans with a fused z stage), a false flag runs none, and
    no distributed plan has the flag."""
    mod = _mod()
    cfgs = _cases(op)
    scope = mod.BATCH_SCOPE[op]
    seen = dict.fromkeys(["batch", "composed on one GPU", "peer writes", "chunks > 1", "zero planes",
                          "zero values"], 0)
    wrong = []
    for b in range(BLOCKS[op]):
        _, out = _run_block(op, b, False)
        for cfg, (desc, _, _, facts) in zip(cfgs[b * PER_BLOCK[op]:(b + 1) * PER_BLOCK[op]], out):
            for f in facts:
                K, _, peer, _ = f["plan"]
                seen["peer writes"] += bool(peer)
                seen["chunks > 1"] += K > 1
                seen["zero planes"] += f["planes"] == 0
                seen["zero values"] += f["values"] == 0
                if cfg["P"] > 1:
                    # (fock_fused and reciprocal_fused, which a fan of one member follows, tell
                    # of one transform's own stages and hold on distributed plans too)
                    if f["flag"] and op != "fock_multi" and not (op in FANS and cfg["n"] == 1):
                        wrong.append(f"{desc}: a distributed plan has the flag")
                    continue
                ran = f["counts"].get(scope, 0)
                seen["batch"] += ran > 0
                seen["composed on one GPU"] += ran == 0
                if not f["device"]:
                    continue
                expect = f["calls"] * f["groups"]
                if op == "fock_multi":
                    # the flag tells of the x stages alone: the batch also needs the fused z
                    # stage and a batchable plan, which the plan flags prove only one way
                    if not (f["flag"] and f["reciprocal_fused"]):
                        expect = 0
                    elif not f["batchable"]:
                        expect = ran if ran in (0, expect) else expect
                elif not f["flag"]:
                    expect = 0
                if ran != expect:
                    wrong.append(f"{desc}: flag {f['flag']}, {scope} ran {ran} times, expected {expect}")
    print(op, seen)
    assert not wrong, "\n".join(wrong)
    missing = [k for k, v in seen.items() if v < 1]
    assert not missing, missing


# ------------------------------------------------------------- pinned by hand
# The splits of three ranks with a rank that holds planes and no sticks, sticks and no planes,
# or neither (the class that once broke apply_local), at the largest member count of one
# batch, with peer writes and with a *_FLOAT exchange; dims with an odd y length and a z
# length the ranks split unevenly.
EMPTY_RANK_SPLITS = [((0, 1, 2), (1, 0, 2), "UNBUFFERED"), ((2, 0, 1), (0, 0, 1), "BUFFERED_FLOAT")]


def _fixed(op, sticks, planes, exchange, **choices):
    mod = _mod()
    n = mod.MAX_SPINORS if op in SPINORS else mod.MAX_BATCH
    return mod.fixed_case(op, (12, 11, 10), sticks, planes, exchange=exchange, n=n, nul=True, **choices)


def _check_fixed(op, host):
    mod = _mod()
    for sticks, planes, exchange in EMPTY_RANK_SPLITS:
        for single in (False, True):
            cfg = _fixed(op, sticks, planes, exchange, single=single, z_fill=1.0 if single else 0.8)
            desc, err, tol, facts = mod.run_case(cfg, host=host)
            print(desc, err)
            assert err < tol, desc
            assert tol == (2e-5 if single or exchange.endswith("FLOAT") else 1e-12)
            assert [f["planes"] for f in facts] == mod.planes_of(cfg) and 0 in [f["planes"] for f in facts]
            assert 0 in [f["values"] for f in facts]


@pytest.mark.parametrize("op", OPS)
def test_fixed_empty_rank_splits_host(op):
    _check_fixed(op, True)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_fixed_empty_rank_splits_gpu(gpu, op):
    _check_fixed(op, False)


def test_fixed_case_arguments():
    mod = _mod()
    cfg = mod.fixed_case("fan_in", (8, 4, 2), n=2, kind="real")
    assert cfg["n"] == 2 and cfg["kind"] == "real" and cfg["P"] == 1 and mod.members_of(cfg) == 2
    assert mod.members_of(mod.fixed_case("spin_density", (8, 4, 2))) == 4
    with pytest.raises(ValueError):
        mod.fixed_case("fan_in", (8, 4, 2), members=3)
    with pytest.raises(ValueError):
        mod.fixed_case("fan_in", (8, 4, 2), (1, 1), (1,))
    with pytest.raises(ValueError):
        mod.fixed_case("local", (8, 4, 2))
