"""accumulate_fock and multi_transform_accumulate_fock on R2C transforms whose half-length
dimX / 2 has a compile-time engine: the packed-real pair x stages. The forward x stage forms
the packed rows a[2m] b[2m] + i a[2m+1] b[2m+1] in its row loads, the accumulating backward x
stage updates pairs of acc straight from LDS, and the real space domain is neither written
nor read. fock_r2c_fused says so; fock_fused stays the C2C flag. Odd dimX, run-time
half-lengths, SPFFT_R2C_PACKED=0 and SPFFT_R2C_FUSE=0 stay composed, and so does the half
of a call whose a, b or acc is not aligned to two elements.

Oracle: tests/test_fock.py::_oracle with r2c=True (dense_forward / dense_backward in double
precision): a, b and acc0 real random fields, acc0 scaled to max|update|, the Gaussian
('real') and the translation-phase ('complex') kernel. Bounds: the project's 1e-12 (fp64)
and 2e-5 (fp32) on max_rel_error. Every check makes two consecutive calls and compares the
whole acc and acc - acc0 against acc0 + n * update (tests/test_fock.py::_twice).

Index sets and seeds are those of tests/test_r2c_fused.py (every column 0..h holds sticks,
asserted with numpy; (1024, 3, 2) asserts column 0 and the Nyquist column only).

The library reads its environment switches when a grid or transform is created, so the
tests set them around the creation only."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import spfft_amd as sp  # noqa: E402
from spfft_amd.utils.indices import create_value_indices  # noqa: E402
from spfft_amd.utils.oracle import max_rel_error  # noqa: E402
from test_fock import (GPU, HOST, TOL32, TOL64, W, _acc0, _field, _kernel, _oracle,  # noqa: E402
                       _scaling, _twice)
from test_fock_multi import WEIGHTS, _scope_counts, _update  # noqa: E402
from test_r2c_fused import (SHAPES, _columns, _fill_space, _random_indices, _sphere,  # noqa: E402
                            _transform)

KINDS = ("real", "complex")


def _tol(single):
    return TOL32 if single else TOL64


def _np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _check_pair(gpu, t, dims, idx, single=False, seed=160, sentinel=True, host=False):
    """Both kernel kinds, both scalings and a is b, each on two consecutive calls against the
    oracle; the values output against the oracle's scaled forward values; a, b and K
    bit-identical afterwards; a sentinel-filled space domain bit-identical afterwards."""
    import torch
    rng = np.random.default_rng(seed)
    a, b = _field(rng, dims, True, single), _field(rng, dims, True, single)
    untouched = _fill_space(t) if sentinel else (lambda: True)

    def dev(x):
        return x.copy() if host else torch.as_tensor(x, device=gpu)

    da, db = dev(a), dev(b)
    cdt = np.complex64 if single else np.complex128
    for kind in KINDS:
        k = _kernel(idx, dims, kind, single)
        dk = dev(k)
        for full, same in ((False, False), (True, False), (kind == "real", True)):
            bb, dbb = (a, da) if same else (b, db)
            upd, wvals = _oracle(idx, a, bb, k, dims, r2c=True, full=full)
            acc0 = _acc0(rng, upd).astype(a.dtype)
            dacc = dev(acc0)
            vals = dev(np.full(len(idx), -1, dtype=cdt))
            label = f"{dims} {'fp32' if single else 'fp64'} {kind} full={full} a_is_b={same}"
            _twice(lambda: t.accumulate_fock(da, dbb, dk, W, dacc, values=vals, scaling=_scaling(full)),
                   lambda: _np(dacc), acc0, upd, _tol(single), label)
            e_vals = max_rel_error(_np(vals), wvals)
            print(label, "values", e_vals)
            assert e_vals < _tol(single)
        assert _np(dk).tobytes() == k.tobytes()
    assert _np(da).tobytes() == a.tobytes() and _np(db).tobytes() == b.tobytes()
    assert untouched(), "the fused call wrote the space domain"


def _logged_fock(capfd):
    """fock= of the last plan line SPFFT_LOG printed, as a flag."""
    m = re.findall(r"density=\w+ reciprocal=\w+ fock=(\w+)", capfd.readouterr().err)
    assert m, "no SPFFT_LOG line"
    return m[-1] == "fused"


# ------------------------------------------------------------------------- host
def test_host_r2c_reports_false_and_matches_oracle():
    dims = (32, 13, 5)
    idx = _random_indices(dims, 3)
    t = _transform(HOST, dims, idx)
    assert t.fock_r2c_fused is False and t.fock_fused is False
    rng = np.random.default_rng(161)
    a, b = _field(rng, dims, True), _field(rng, dims, True)
    for kind in KINDS:
        k = _kernel(idx, dims, kind)
        for full in (False, True):
            upd, wvals = _oracle(idx, a, b, k, dims, r2c=True, full=full)
            acc0 = _acc0(rng, upd)
            acc = acc0.copy()
            vals = np.full(len(idx), -1, dtype=np.complex128)
            _twice(lambda: t.accumulate_fock(a, b, k, W, acc, values=vals, scaling=_scaling(full)),
                   lambda: acc, acc0, upd, TOL64, f"host {kind} full={full}")
            assert max_rel_error(vals, wvals) < TOL64


# ------------------------------------------------------------------------ flags
@pytest.mark.gpu
def test_gpu_flags(gpu):
    dims = (64, 13, 5)
    idx = _random_indices(dims, 1)
    t = _transform(GPU, dims, idx)
    assert t.fock_r2c_fused is True and t.fock_fused is False
    c = _transform(GPU, dims, create_value_indices(np.random.default_rng(2), [1.0], 0.7, 0.8, *dims,
                                                   False)[0], r2c=False)
    assert c.fock_r2c_fused is False and c.fock_fused is True
    # run-time half-lengths (8, 20) and odd dimX
    for other in ((16, 12, 10), (40, 9, 4), (33, 8, 4)):
        o = create_value_indices(np.random.default_rng(2), [1.0], 0.7, 0.8, *other, True)[0]
        u = _transform(GPU, other, o)
        assert u.fock_r2c_fused is False and u.fock_fused is False, other
    for env in ({"SPFFT_R2C_PACKED": "0"}, {"SPFFT_R2C_FUSE": "0"}):
        u = _transform(GPU, dims, idx, env=env)
        assert u.fock_r2c_fused is False and u.fock_fused is False, env


# ----------------------------------------------------------------------- shapes
@pytest.mark.gpu
@pytest.mark.parametrize("dims,single,seed", SHAPES)
def test_gpu_shapes(gpu, dims, single, seed, capfd):
    idx = _random_indices(dims, seed)  # (asserts which columns hold sticks)
    t = _transform(GPU, dims, idx, single=single, env={"SPFFT_LOG": "1"})
    assert t.fock_r2c_fused is _logged_fock(capfd)
    assert t.fock_fused is False
    if dims[0] != 1024:  # (the 1024-long shapes: right whatever the flag says)
        assert t.fock_r2c_fused is True
    _check_pair(gpu, t, dims, idx, single=single, sentinel=t.fock_r2c_fused)


@pytest.mark.gpu
@pytest.mark.parametrize("centred", [False, True])
def test_gpu_columns_without_sticks(gpu, centred):
    """The Nyquist column and the columns 20..32 hold no sticks: the forward stage stores
    nothing there, the backward stage reads zeros there."""
    dims, idx = _sphere(centred)
    cols = _columns(idx, dims)
    assert dims[0] // 2 not in cols and not cols & set(range(20, 33))
    t = _transform(GPU, dims, idx)
    assert t.fock_r2c_fused is True
    _check_pair(gpu, t, dims, idx, seed=162)


# ------------------------------------------------------- fused against composed
def _off_by_one(gpu, x):
    """A copy of x one element off the 16-byte pair alignment."""
    import torch
    buf = torch.empty(x.size + 1, dtype=torch.float64, device=gpu)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(*x.shape)
    view.copy_(torch.as_tensor(x, device=gpu))
    assert view.data_ptr() % 16 == 8
    return view


@pytest.mark.gpu
def test_gpu_fused_matches_composed_and_unaligned(gpu):
    import torch
    dims = (64, 13, 5)
    idx = _random_indices(dims, 1)
    fused = _transform(GPU, dims, idx)
    composed = _transform(GPU, dims, idx, env={"SPFFT_R2C_FUSE": "0"})
    assert fused.fock_r2c_fused is True and composed.fock_r2c_fused is False
    rng = np.random.default_rng(163)
    a, b = _field(rng, dims, True), _field(rng, dims, True)
    k = _kernel(idx, dims, "complex")
    upd, _ = _oracle(idx, a, b, k, dims, r2c=True)
    acc0 = _acc0(rng, upd)
    want = acc0 + upd
    da, db, dk = (torch.as_tensor(x, device=gpu) for x in (a, b, k))

    def run(t, xa, xb, xacc):
        return t.accumulate_fock(xa, xb, dk, W, xacc).cpu().numpy()

    rf = run(fused, da, db, torch.as_tensor(acc0, device=gpu))
    rc = run(composed, da, db, torch.as_tensor(acc0, device=gpu))
    assert max_rel_error(rf, rc) < TOL64
    assert max_rel_error(rf, want) < TOL64 and max_rel_error(rc, want) < TOL64
    assert max_rel_error(rf - acc0, upd) < TOL64 and max_rel_error(rc - acc0, upd) < TOL64
    # a, then b, then acc one element off the pair alignment: the half of the call that
    # uses the array runs composed (the documented fall-back), which shows in the sentinel-
    # filled space domain, a composed half's scratch, being overwritten; the result is the same
    ua, ub = _off_by_one(gpu, a), _off_by_one(gpu, b)
    for xa, xb, unaligned_acc in ((ua, db, False), (da, ub, False), (da, db, True)):
        xacc = _off_by_one(gpu, acc0) if unaligned_acc else torch.as_tensor(acc0, device=gpu)
        untouched = _fill_space(fused)
        r = run(fused, xa, xb, xacc)
        assert not untouched(), "an unaligned array went through the pair kernels"
        assert max_rel_error(r, rf) < TOL64 and max_rel_error(r, want) < TOL64
        assert max_rel_error(r - acc0, upd) < TOL64
    # the next aligned call is fused again: the space domain stays untouched
    untouched = _fill_space(fused)
    assert max_rel_error(run(fused, da, db, torch.as_tensor(acc0, device=gpu)), want) < TOL64
    assert untouched()


def _multi_scopes(call):
    sp.timing_reset()
    sp.timing_enable(True, gpu_stages=False)
    try:
        call()
        return _scope_counts(sp.timing_json())
    finally:
        sp.timing_enable(False)


@pytest.mark.gpu
def test_gpu_unaligned_member_of_a_multi_call(gpu):
    """Three clones with a fused z stage. All aligned: one batch. a[0] off the pair alignment:
    that member runs per transform and composed (its space domain is overwritten), the other
    two still batch. acc off the alignment: every member runs per transform."""
    import torch
    dims = (64, 13, 5)
    idx = create_value_indices(np.random.default_rng(1), [1.0], 0.7, 1.0, *dims, True)[0]
    assert _columns(idx, dims) == set(range(dims[0] // 2 + 1))
    t0 = _transform(GPU, dims, idx)
    ts = [t0, t0.clone(), t0.clone()]
    assert all(t.fock_r2c_fused and t.reciprocal_fused for t in ts)
    rng = np.random.default_rng(168)
    a = [_field(rng, dims, True) for _ in ts]
    b = _field(rng, dims, True)
    k = _kernel(idx, dims, "complex")
    upd = _update(idx, a, [b] * 3, [k] * 3, WEIGHTS, dims, r2c=True)
    acc0 = _acc0(rng, upd)
    da = [torch.as_tensor(x, device=gpu) for x in a]
    db, dk = torch.as_tensor(b, device=gpu), torch.as_tensor(k, device=gpu)

    def check(xa, dacc):
        spaces = [_fill_space(t) for t in ts]
        counts = _multi_scopes(lambda: sp.multi_transform_accumulate_fock(ts, xa, [db] * 3, dk, WEIGHTS,
                                                                          dacc))
        got = dacc.cpu().numpy()
        assert max_rel_error(got, acc0 + upd) < TOL64 and max_rel_error(got - acc0, upd) < TOL64
        return counts, [s() for s in spaces]

    counts, untouched = check(da, torch.as_tensor(acc0, device=gpu))
    assert counts.get("gpu_accumulate_fock_batch") == 1, counts
    assert "gpu_fock_forward_xy" not in counts and "gpu_fock_backward_xy" not in counts, counts
    assert untouched == [True, True, True]
    counts, untouched = check([_off_by_one(gpu, a[0])] + da[1:], torch.as_tensor(acc0, device=gpu))
    assert counts.get("gpu_accumulate_fock_batch") == 1, counts
    assert counts.get("gpu_fock_forward_xy") == 1 and counts.get("gpu_fock_backward_xy") == 1, counts
    assert untouched == [False, True, True]
    counts, untouched = check(da, _off_by_one(gpu, acc0))
    assert "gpu_accumulate_fock_batch" not in counts, counts
    assert counts.get("gpu_fock_forward_xy") == 3 and counts.get("gpu_fock_backward_xy") == 3, counts
    assert untouched == [False, False, False]


# ---------------------------------------------------------------------- batches
# (64, 13, 5): partial row blocks; (32, 64, 4): full blocks
@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["1", "0"])
@pytest.mark.parametrize("dims,seed", [((64, 13, 5), 1), ((32, 64, 4), 1)])
def test_gpu_multi_transform(gpu, dims, seed, batch):
    import torch
    batching = batch != "0"
    # z fill 1.0: simple sticks, the fused z stage, which a batch needs; every column holds sticks
    idx = create_value_indices(np.random.default_rng(seed), [1.0], 0.7, 1.0, *dims, True)[0]
    assert _columns(idx, dims) == set(range(dims[0] // 2 + 1))
    t0 = _transform(GPU, dims, idx, env={"SPFFT_BATCH": batch})
    saved = os.environ.get("SPFFT_BATCH")
    os.environ["SPFFT_BATCH"] = batch
    try:
        ts = [t0, t0.clone(), t0.clone()]
    finally:
        if saved is None:
            os.environ.pop("SPFFT_BATCH")
        else:
            os.environ["SPFFT_BATCH"] = saved
    assert all(t.fock_r2c_fused and t.reciprocal_fused and not t.fock_fused for t in ts)
    checks = [_fill_space(t) for t in ts]
    rng = np.random.default_rng(164)
    a = [_field(rng, dims, True) for _ in ts]
    bs = [_field(rng, dims, True) for _ in ts]
    k = _kernel(idx, dims, "complex")
    da = [torch.as_tensor(x, device=gpu) for x in a]
    dbs = [torch.as_tensor(x, device=gpu) for x in bs]
    dk = torch.as_tensor(k, device=gpu)
    calls = 0
    sp.timing_reset()
    sp.timing_enable(True, gpu_stages=False)
    try:
        for distinct in (False, True):  # b shared by the members, then one b each; K shared
            b = bs if distinct else [bs[0]] * 3
            db = dbs if distinct else [dbs[0]] * 3
            upd = _update(idx, a, b, [k] * 3, WEIGHTS, dims, r2c=True)
            acc0 = _acc0(rng, upd)
            results = []
            for rep in range(2):
                dacc = torch.as_tensor(acc0, device=gpu)
                assert sp.multi_transform_accumulate_fock(ts, da, db, dk, WEIGHTS, dacc) is dacc
                calls += 1
                results.append(dacc.cpu().numpy().copy())
                assert max_rel_error(results[-1], acc0 + upd) < TOL64
                assert max_rel_error(results[-1] - acc0, upd) < TOL64
            assert results[0].tobytes() == results[1].tobytes()  # the same call, the same bits
            sp.multi_transform_accumulate_fock(ts, da, db, dk, WEIGHTS, dacc)  # on top
            calls += 1
            assert max_rel_error(dacc.cpu().numpy(), acc0 + 2 * upd) < TOL64
            assert max_rel_error(dacc.cpu().numpy() - acc0, 2 * upd) < TOL64
        counts = _scope_counts(sp.timing_json())
    finally:
        sp.timing_enable(False)
    print("scopes", {n: c for n, c in counts.items() if "fock" in n})
    assert counts.get("multi_accumulate_fock") == calls
    if batching:
        assert counts.get("gpu_accumulate_fock_batch") == calls
        assert "gpu_fock_forward_xy" not in counts and "gpu_fock_backward_xy" not in counts
    else:
        assert "gpu_accumulate_fock_batch" not in counts
        assert counts.get("gpu_fock_forward_xy") == 3 * calls
        assert counts.get("gpu_fock_backward_xy") == 3 * calls
    for x, d in zip(a + bs, da + dbs):
        assert d.cpu().numpy().tobytes() == x.tobytes()
    assert all(c() for c in checks), "a fused call wrote a space domain"


# ------------------------------------------------------------------ other paths
@pytest.mark.gpu
def test_gpu_host_arrays(gpu):
    """numpy a, b, K, acc and values on a GPU transform: staged through device buffers, the
    fused stages."""
    dims = (64, 13, 5)
    idx = _random_indices(dims, 1)
    t = _transform(GPU, dims, idx)
    assert t.fock_r2c_fused is True
    _check_pair(gpu, t, dims, idx, seed=165, host=True)


@pytest.mark.gpu
def test_gpu_capped_intermediate(gpu, capfd):
    """An intermediate capped below the local planes: several plane ranges, the pair stages
    in each."""
    dims = (64, 18, 6)
    nx, ny, nz = dims
    idx = _random_indices(dims, 1)
    t = _transform(GPU, dims, idx, env={"SPFFT_INTER_BYTES": str(nx * (ny + 8) * 16), "SPFFT_LOG": "1"})
    planes = int(re.findall(r"inter_planes=(\d+) apply_local=fused density=fused reciprocal=\w+ fock=fused",
                            capfd.readouterr().err)[-1])
    assert -(-nz // planes) >= 2, planes
    assert t.fock_r2c_fused is True
    _check_pair(gpu, t, dims, idx, seed=166)


# Three virtual ranks of one GPU under the pipelined COMPACT_BUFFERED exchange, 2 plane
# chunks x 2 stick blocks forced; the second split leaves rank 1 without planes. The bound is
# the sweep's (tools/fuzz_ops.py, fp64).
@pytest.mark.gpu
@pytest.mark.parametrize("planes", [[1, 1, 1], [1, 0, 2]])
def test_gpu_virtual_ranks_pipelined(gpu, planes):
    import importlib.util
    if "fuzz_ops" not in sys.modules:
        spec = importlib.util.spec_from_file_location("fuzz_ops", os.path.join(REPO, "tools", "fuzz_ops.py"))
        sys.modules["fuzz_ops"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules["fuzz_ops"])
    mod = sys.modules["fuzz_ops"]
    desc, err, tol, facts = mod.run_case(mod.fixed_case("fock", r2c=True, dims=(32, 18, 30),
                                                        stick_dist=[1, 1, 1], plane_dist=planes,
                                                        exchange="COMPACT_BUFFERED", chunks=2, blocks=2))
    print(desc, err, facts)
    assert tol == 1e-10 and err < 1e-10
    assert len(facts) == 3
    assert any(f["planes"] == 0 for f in facts) == (0 in planes)
    for f in facts:
        assert f["r2c_fused"] is True and f["fused"] is False, f
        assert f["plan"][:3] == (2, 2, False), f


@pytest.mark.gpu
@pytest.mark.parametrize("zfill", [1.0, 0.7])
def test_gpu_stage_timing_names(gpu, zfill):
    """The stage names of the C2C fused path: forward x_pair+y, backward y+x_fock, each once
    per call; the z and exchange names are apply_reciprocal's."""
    import torch
    dims = (64, 13, 5)
    rng = np.random.default_rng(167)
    idx = create_value_indices(rng, [1.0], 1.0, zfill, *dims, True)[0]
    t = _transform(GPU, dims, idx)
    assert t.fock_r2c_fused is True and t.reciprocal_fused is (zfill == 1.0)
    da, db = (torch.as_tensor(_field(rng, dims, True), device=gpu) for _ in range(2))
    dacc = torch.zeros_like(da)
    dk = torch.as_tensor(_kernel(idx, dims, "real"), device=gpu)
    sp.timing_reset()
    sp.timing_enable(True)
    try:
        for _ in range(3):
            t.accumulate_fock(da, db, dk, W, dacc)
        t.synchronize()
        tree = sp.timing_json()
    finally:
        sp.timing_enable(False)
    gpu_node = [n for n in tree["timings"] if n["identifier"] == "gpu"]
    assert gpu_node, tree
    dirs = {d["identifier"]: {s["identifier"]: s for s in d["sub-timings"]}
            for d in gpu_node[0]["sub-timings"]}
    if zfill == 1.0:
        assert set(dirs["forward"]) == {"x_pair+y", "exchange", "z_reciprocal"}, dirs
        assert set(dirs["backward"]) == {"y+x_fock", "exchange"}, dirs
    else:
        assert set(dirs["forward"]) == {"x_pair+y", "exchange", "z", "multiply"}, dirs
        assert set(dirs["backward"]) == {"y+x_fock", "z", "exchange"}, dirs
    for d in dirs.values():
        for node in d.values():
            assert node["count"] == 3, node
