"""multi_transform_accumulate_fock: acc += sum_i w_i a_i backward_i(K_i (scale forward_i(conj(a_i)
b_i))) of several transforms into one shared acc, the pairs of one band of the exchange
operator in one call, against the dense oracle
acc0 + sum_i w_i a_i dense_backward(idx, K_i dense_forward(conj(a_i) b_i, idx, dims, scale), dims).

Identical GPU plans with fused pair x stages and a fused z stage run as batches: one launch
per stage, the members over the grid's z extent in the forward x and the z stage, looped over
inside the workgroup that owns a tile of acc in the accumulating x stage. Everything else
(R2C, run-table sticks, host pointers, host transforms, SPFFT_BATCH=0, distributed grids) runs
per transform with the phases interleaved, each update of acc ordered behind the previous one.

Inputs as tests/test_fock.py: a and b of unit variance, |K| <= 1, acc0 random and scaled to
max|update|; the weights have both signs. Every accuracy case runs the call twice and checks
the whole acc against acc0 + n * update and acc - acc0 against n * update alone, and that the
inputs are unchanged.

Bounds: 1e-12 (fp64) and 2e-5 (fp32) on max_rel_error, those of tests/test_fock.py. The sum of
n <= 10 pair updates with |w| <= 2.75 adds at most n roundings per element to the single
pair's error (<= 6e-16 fp64, <= 3e-7 fp32 for the update alone, see there).

Run as a program (python tests/test_fock_multi.py CASE) it executes the cases that need their
own process, because the library reads SPFFT_BATCH when a transform is created."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import spfft_amd as sp  # noqa: E402
from spfft_amd.utils.indices import create_value_indices, sphere_indices  # noqa: E402
from spfft_amd.utils.oracle import dense_backward, dense_forward, max_rel_error  # noqa: E402
from test_fock import (GPU, HOST, TOL32, TOL64, _acc0, _dtype, _field, _kernel,  # noqa: E402
                       _scaling, _transform, _twice)

WEIGHTS = [-0.75, 0.5, -1.25]


def _update(idx, a, b, k, weights, dims, r2c=False, full=False):
    """sum_i w_i a_i u_i in double precision; a, b, k are lists of one entry per pair."""
    wide = np.float64 if r2c else np.complex128
    total = 0
    for ai, bi, ki, w in zip(a, b, k, weights):
        a64, b64 = np.asarray(ai).astype(wide), np.asarray(bi).astype(wide)
        vals = dense_forward(np.conj(a64) * b64, idx, dims, r2c=r2c, scale=full)
        u = dense_backward(idx, np.asarray(ki).astype(np.complex128) * vals, dims, r2c=r2c)
        total = total + w * a64 * u
    return total


def _clones(pu, dims, idx, n, r2c=False, single=False):
    t0 = _transform(pu, dims, idx, r2c=r2c, single=single)
    return [t0] + [t0.clone() for _ in range(n - 1)]


def _scope_counts(tree):
    """identifier -> summed call count over the whole timing tree."""
    counts = {}

    def walk(nodes):
        for n in nodes:
            counts[n["identifier"]] = counts.get(n["identifier"], 0) + n["count"]
            walk(n.get("sub-timings", []))

    walk(tree["timings"])
    return counts


# ------------------------------------------------------------------------- host
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("r2c", [False, True])
def test_host_three_clones(r2c, kind):
    dims = (12, 11, 8)
    rng = np.random.default_rng(170)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, r2c)[0]
    ts = _clones(HOST, dims, idx, 3, r2c=r2c)
    a = [_field(rng, dims, r2c) for _ in ts]
    b = _field(rng, dims, r2c)
    k = _kernel(idx, dims, kind)
    a_in, b_in, k_in = [x.copy() for x in a], b.copy(), k.copy()
    for full in (False, True):
        upd = _update(idx, a, [b] * 3, [k] * 3, WEIGHTS, dims, r2c=r2c, full=full)
        acc0 = _acc0(rng, upd).astype(_dtype(r2c, False))
        acc = acc0.copy()
        assert sp.multi_transform_accumulate_fock(ts, a, [b] * 3, k, WEIGHTS, acc,
                                                  scaling=_scaling(full)) is acc
        acc[...] = acc0
        _twice(lambda: sp.multi_transform_accumulate_fock(ts, a, [b] * 3, k, WEIGHTS, acc,
                                                          scaling=_scaling(full)),
               lambda: acc, acc0, upd, TOL64, f"host multi r2c={r2c} {kind} full={full}")
        # the same pairs as three single calls
        single = acc0.copy()
        for t, ai, w in zip(ts, a, WEIGHTS):
            t.accumulate_fock(ai, b, k, w, single, scaling=_scaling(full))
        acc[...] = acc0
        sp.multi_transform_accumulate_fock(ts, a, [b] * 3, k, WEIGHTS, acc, scaling=_scaling(full))
        e = max_rel_error(acc, single)
        eu = max_rel_error(acc - acc0, single - acc0)
        print("against single calls", e, eu)
        assert e < TOL64 and eu < TOL64
    assert all(np.array_equal(x, y) for x, y in zip(a, a_in))
    assert np.array_equal(b, b_in) and np.array_equal(k, k_in)


def test_host_distinct_b_and_kernels():
    """One b and one kernel per transform; a[0] is b[0]."""
    dims = (12, 11, 8)
    rng = np.random.default_rng(171)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, False)[0]
    ts = _clones(HOST, dims, idx, 3)
    a = [_field(rng, dims) for _ in ts]
    b = [a[0]] + [_field(rng, dims) for _ in ts[1:]]
    ks = [_kernel(idx, dims, "complex") * s for s in (1.0, 0.5, -0.25)]
    upd = _update(idx, a, b, ks, WEIGHTS, dims, full=True)
    acc0 = _acc0(rng, upd)
    acc = acc0.copy()
    _twice(lambda: sp.multi_transform_accumulate_fock(ts, a, b, ks, WEIGHTS, acc,
                                                      scaling=sp.Scaling.FULL),
           lambda: acc, acc0, upd, TOL64, "host distinct")


def test_arguments_are_checked():
    rng = np.random.default_rng(172)
    dims = (6, 5, 4)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    ts = _clones(HOST, dims, idx, 2)
    a = [_field(rng, dims) for _ in ts]
    b = _field(rng, dims)
    k = _kernel(idx, dims, "real")
    w = WEIGHTS[:2]
    acc = np.zeros_like(b)
    multi = sp.multi_transform_accumulate_fock
    with pytest.raises(sp.InvalidParameterError):  # a repeated grid
        multi([ts[0], ts[0]], a, [b, b], k, w, acc)
    for bad in (lambda: multi(ts, a[:1], [b, b], k, w, acc),  # mismatched lengths
                lambda: multi(ts, a, [b], k, w, acc),
                lambda: multi(ts, a, [b, b], k, w[:1], acc),
                lambda: multi(ts, a, [b, b], [k], w, acc),
                lambda: multi(ts, a, [b, b], k[:-1], w, acc),
                lambda: multi(ts, a, [b, b], k, w, acc, scaling=7)):  # a bad scaling
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):  # a null acc never reaches the library from Python
        multi(ts, a, [b, b], k, w, None)
    with pytest.raises(TypeError):  # real and complex kernels in one call
        multi(ts, a, [b, b], [k, _kernel(idx, dims, "complex")], w, acc)
    with pytest.raises(TypeError):
        multi(ts, a, [b, b], k, w, acc.astype(np.complex64))
    # mixed precision
    tf = _transform(HOST, dims, idx, single=True)
    with pytest.raises(TypeError):
        multi([ts[0], tf], a, [b, b], k, w, acc)
    # mismatched space shapes
    dims2 = (6, 5, 6)
    other = _transform(HOST, dims2, create_value_indices(rng, [1.0], 1.0, 1.0, *dims2, False)[0])
    with pytest.raises(ValueError):
        multi([ts[0], other], a, [b, b], k, w, acc)
    # all C2C or all R2C
    treal = _transform(HOST, dims, create_value_indices(rng, [1.0], 1.0, 1.0, *dims, True)[0],
                       r2c=True)
    with pytest.raises(ValueError):
        multi([ts[0], treal], a, [b, b], k, w, acc)
    assert not acc.any()
    # the native checks (the Python layer never passes a null array or a bad scaling)
    import ctypes
    from spfft_amd.ops._lib import lib
    from spfft_amd.types import ErrorCode
    fn = lib().spfft_amd_multi_transform_accumulate_fock
    invalid = int(ErrorCode.INVALID_PARAMETER)
    hs = (ctypes.c_void_p * 2)(ts[0].handle.value, ts[1].handle.value)
    twice = (ctypes.c_void_p * 2)(ts[0].handle.value, ts[0].handle.value)
    odd = (ctypes.c_void_p * 2)(ts[0].handle.value, other.handle.value)
    pa = (ctypes.c_void_p * 2)(a[0].ctypes.data, a[1].ctypes.data)
    pb = (ctypes.c_void_p * 2)(b.ctypes.data, b.ctypes.data)
    pk = (ctypes.c_void_p * 2)(k.ctypes.data, k.ctypes.data)
    holes = (ctypes.c_void_p * 2)(k.ctypes.data, None)
    ws = (ctypes.c_double * 2)(*w)
    pw, pacc = ctypes.cast(ws, ctypes.c_void_p), acc.ctypes.data
    assert fn(2, twice, pa, pb, pk, 0, pw, pacc, 0) == invalid
    assert fn(2, odd, pa, pb, pk, 0, pw, pacc, 0) == invalid
    assert fn(2, None, pa, pb, pk, 0, pw, pacc, 0) == invalid
    assert fn(2, hs, None, pb, pk, 0, pw, pacc, 0) == invalid
    assert fn(2, hs, pa, None, pk, 0, pw, pacc, 0) == invalid
    assert fn(2, hs, pa, pb, None, 0, pw, pacc, 0) == invalid
    assert fn(2, hs, pa, pb, pk, 0, None, pacc, 0) == invalid
    assert fn(2, hs, pa, pb, pk, 0, pw, None, 0) == invalid
    assert fn(2, hs, pa, pb, holes, 0, pw, pacc, 0) == invalid
    assert fn(2, hs, holes, pb, pk, 0, pw, pacc, 0) == invalid
    assert fn(2, hs, pa, pb, pk, 0, pw, pacc, 7) == invalid
    assert not acc.any()
    # and the transforms still work
    upd = _update(idx, a, [b, b], [k, k], w, dims)
    assert max_rel_error(multi(ts, a, [b, b], k, w, acc), upd) < TOL64


def test_zero_and_one_transform():
    rng = np.random.default_rng(173)
    dims = (6, 5, 4)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    t = _transform(HOST, dims, idx)
    a, b = _field(rng, dims), _field(rng, dims)
    k = _kernel(idx, dims, "complex")
    acc = np.ones_like(a)
    assert sp.multi_transform_accumulate_fock([], [], [], k, [], acc) is acc
    assert np.array_equal(acc, np.ones_like(a))
    from spfft_amd.ops._lib import lib
    assert lib().spfft_amd_multi_transform_accumulate_fock(0, None, None, None, None, 0, None,
                                                           None, 0) == 0
    upd = _update(idx, [a], [b], [k], [WEIGHTS[0]], dims)
    acc0 = _acc0(rng, upd)
    acc = acc0.copy()
    _twice(lambda: sp.multi_transform_accumulate_fock([t], [a], [b], k, WEIGHTS[:1], acc),
           lambda: acc, acc0, upd, TOL64, "n = 1")
    single = acc0.copy()
    t.accumulate_fock(a, b, k, WEIGHTS[0], single)
    t.accumulate_fock(a, b, k, WEIGHTS[0], single)
    assert acc.tobytes() == single.tobytes()  # one transform: the single call's path


def _two_ranks(pu, exchange):
    """Each rank passes its slab of the pairs' a, of b and of acc, and its part of K; two
    transforms per rank (the rank's transform of two distributed grids)."""
    from spfft_amd.parallel import make_distributed, run_ranks
    dims = (12, 11, 8)
    gidx = sphere_indices(*dims, 0.5)
    rng = np.random.default_rng(174)
    a = [_field(rng, dims) for _ in range(2)]
    b = _field(rng, dims)
    w = WEIGHTS[:2]
    upd = _update(gidx, a, [b, b], [_kernel(gidx, dims, "complex")] * 2, w, dims, full=True)
    acc0 = _acc0(rng, upd)

    def body(rank, comm):
        if pu == GPU:
            import torch
            torch.cuda.set_device(0)
        ss = [make_distributed(comm, dims, gidx, processing_unit=pu, exchange_type=exchange)
              for _ in range(2)]
        s = ss[0]
        ts = [x.transform for x in ss]
        k = _kernel(s.indices, dims, "complex")
        z = slice(s.z_offset, s.z_offset + s.z_length)
        sa = [np.ascontiguousarray(x[z]) for x in a]
        sb = np.ascontiguousarray(b[z])
        acc = acc0[z].copy()
        if pu == GPU:
            import torch
            sa = [torch.as_tensor(x, device="cuda") for x in sa]
            sb, acc, k = (torch.as_tensor(x, device="cuda") for x in (sb, acc, k))
        host = (lambda x: x.cpu().numpy()) if pu == GPU else (lambda x: x)
        errs = []
        scale = float(np.max(np.abs(upd)))  # a rank's slab against the global scale
        for n in (1, 2):
            sp.multi_transform_accumulate_fock(ts, sa, [sb, sb], k, w, acc, scaling=sp.Scaling.FULL)
            if s.z_length:
                got = host(acc)
                errs.append(float(np.max(np.abs(got - (acc0[z] + n * upd[z])))) /
                            float(np.max(np.abs(acc0 + n * upd))))
                errs.append(float(np.max(np.abs((got - acc0[z]) - n * upd[z]))) / (n * scale))
        return max(errs)

    return run_ranks(2, body)


def test_host_two_ranks():
    for err in _two_ranks(HOST, sp.ExchangeType.COMPACT_BUFFERED):
        assert err < TOL64


# -------------------------------------------------------------------------- GPU
def _check_batch(gpu, dims, idx, single=False, kind="complex", seed=180, distinct_b=False,
                 same=False, kernels="shared", n=3, fused=True, zfused=True, r2c=False,
                 host=()):
    """n clones, twice per scaling against the oracle; `host`: the arrays passed as host
    pointers ('a', 'b', 'acc'). Returns the transforms."""
    import torch
    rng = np.random.default_rng(seed)
    assert len(idx) > 0
    ts = _clones(GPU, dims, idx, n, r2c=r2c, single=single)
    for t in ts:
        assert t.fock_fused is fused and t.reciprocal_fused is zfused
    weights = [WEIGHTS[i % 3] * (1 + i // 3) for i in range(n)]
    a = [_field(rng, dims, r2c, single) for _ in ts]
    if distinct_b:
        b = [_field(rng, dims, r2c, single) for _ in ts]
    else:
        b = [_field(rng, dims, r2c, single)] * n
    if same:
        b = [a[0]] + b[1:]
    k0 = _kernel(idx, dims, kind, single)
    ks = [k0 * (1.0 - 0.25 * i) for i in range(n)] if kernels == "each" else [k0] * n
    ks = [x.astype(k0.dtype) for x in ks]

    def dev(x, where):
        return x if where in host else torch.as_tensor(x, device=gpu)

    cache = {}

    def once(x, where):  # one device tensor per distinct host array
        if id(x) not in cache:
            cache[id(x)] = dev(x, where)
        return cache[id(x)]

    da = [once(x, "a") for x in a]
    db = [once(x, "b") if not (same and i == 0) else da[0] for i, x in enumerate(b)]
    dk = [once(x, "k") for x in ks]
    karg = dk if kernels == "each" else dk[0]
    tol = TOL32 if single else TOL64
    for full in (True, False):
        upd = _update(idx, a, b, ks, weights, dims, r2c=r2c, full=full)
        acc0 = _acc0(rng, upd).astype(_dtype(r2c, single))
        dacc = acc0.copy() if "acc" in host else torch.as_tensor(acc0, device=gpu)
        label = f"{dims} {'fp32' if single else 'fp64'} {kind} {'full' if full else 'none'}"
        _twice(lambda: sp.multi_transform_accumulate_fock(ts, da, db, karg, weights, dacc,
                                                          scaling=_scaling(full)),
               lambda: dacc if "acc" in host else dacc.cpu().numpy(), acc0, upd, tol, label)
    for x, d in zip(a + b + ks, da + db + dk):
        assert np.array_equal(x, d if isinstance(d, np.ndarray) else d.cpu().numpy())
    return ts


def _batch_scopes(call):
    sp.timing_reset()
    sp.timing_enable(True, gpu_stages=False)
    try:
        call()
        return _scope_counts(sp.timing_json())
    finally:
        sp.timing_enable(False)


# ny = 35 gives full row blocks and a partial last block; nx = 64 is a compile-time engine,
# nx = 100 a run-time engine, 67 Bluestein in LDS (test_fock.py::test_gpu_fused_prime_lengths),
# fp32 nx = 1024 the widest compile-time engine. z fill 1.0: simple sticks, the fused z stage.
@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,single", [(64, 35, False), (64, 35, True), (100, 35, False),
                                          (67, 13, False), (1024, 3, True)])
def test_gpu_batched(gpu, nx, ny, single):
    dims = (nx, ny, 2)
    rng = np.random.default_rng(181)
    idx = create_value_indices(rng, [1.0], 0.7, 1.0, *dims, False)[0]
    _check_batch(gpu, dims, idx, single=single)


@pytest.mark.gpu
@pytest.mark.parametrize("columns", ["dense", "sparse"])
def test_gpu_batched_index_sets(gpu, columns):
    dims = (32, 16, 8)
    if columns == "dense":
        idx = sphere_indices(*dims, 0.5)
    else:
        idx = create_value_indices(np.random.default_rng(182), [1.0], 0.7, 1.0, *dims, False)[0]
    _check_batch(gpu, dims, idx, kind="real")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["distinct_b", "a_is_b", "kernels"])
def test_gpu_batched_variants(gpu, variant):
    dims = (64, 35, 2)
    idx = create_value_indices(np.random.default_rng(183), [1.0], 0.7, 1.0, *dims, False)[0]
    _check_batch(gpu, dims, idx, distinct_b=variant == "distinct_b", same=variant == "a_is_b",
                 kernels="each" if variant == "kernels" else "shared")


@pytest.mark.gpu
def test_gpu_batch_ran(gpu):
    """The in-process cases above run as one batch of three: the scope says so."""
    import torch
    dims = (64, 35, 2)
    rng = np.random.default_rng(184)
    idx = create_value_indices(rng, [1.0], 0.7, 1.0, *dims, False)[0]
    ts = _clones(GPU, dims, idx, 3)
    a = [torch.as_tensor(_field(rng, dims), device=gpu) for _ in ts]
    b = torch.as_tensor(_field(rng, dims), device=gpu)
    k = torch.as_tensor(_kernel(idx, dims, "real"), device=gpu)
    acc = torch.zeros_like(b)
    counts = _batch_scopes(lambda: sp.multi_transform_accumulate_fock(ts, a, [b] * 3, k, WEIGHTS,
                                                                      acc))
    assert counts.get("gpu_accumulate_fock_batch") == 1, counts
    assert "gpu_fock_forward_xy" not in counts and "gpu_fock_backward_xy" not in counts


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["r2c", "runtable", "host_acc", "host_ab"])
def test_gpu_fallbacks_inside_one_call(gpu, case):
    """What does not batch runs per transform, and the scopes say so."""
    import torch
    if case == "r2c":
        dims = (16, 12, 10)
        idx = create_value_indices(np.random.default_rng(185), [1.0], 0.8, 1.0, *dims, True)[0]
        kw = dict(r2c=True, fused=False, zfused=True)
    else:
        dims = (64, 13, 5)
        zfill = 0.7 if case == "runtable" else 1.0
        idx = create_value_indices(np.random.default_rng(185), [1.0], 0.7, zfill, *dims, False)[0]
        kw = dict(zfused=case != "runtable")
        if case == "host_acc":
            kw["host"] = ("acc",)
        if case == "host_ab":
            kw["host"] = ("a", "b")
    ts = _check_batch(gpu, dims, idx, **kw)
    # the same kind of call once more, counted
    rng = np.random.default_rng(186)
    r2c = case == "r2c"
    a = [_field(rng, dims, r2c) for _ in ts]
    b = _field(rng, dims, r2c)
    acc = np.zeros_like(b)
    k = torch.as_tensor(_kernel(idx, dims, "real"), device=gpu)
    if case != "host_ab":
        a, b = [torch.as_tensor(x, device=gpu) for x in a], torch.as_tensor(b, device=gpu)
    if case != "host_acc":
        acc = torch.as_tensor(acc, device=gpu)
    counts = _batch_scopes(lambda: sp.multi_transform_accumulate_fock(ts, a, [b] * 3, k, WEIGHTS,
                                                                      acc))
    assert "gpu_accumulate_fock_batch" not in counts, counts
    assert counts.get("gpu_fock_forward_xy") == 3 and counts.get("gpu_fock_backward_xy") == 3


def _subprocess_case(case, env):
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], cwd=REPO, env=e,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "CASE OK" in r.stdout, (r.stdout + r.stderr)[-4000:]
    return r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["0", "1"])
def test_gpu_ten_plans(gpu, batch):
    _subprocess_case("multi", {"SPFFT_BATCH": batch})


@pytest.mark.gpu
def test_gpu_three_streams(gpu):
    _subprocess_case("streams", {})


@pytest.mark.gpu
def test_gpu_two_ranks(gpu):
    for err in _two_ranks(GPU, sp.ExchangeType.COMPACT_BUFFERED):
        assert err < TOL64


@pytest.mark.gpu
def test_gpu_exchange_operator_groups(gpu):
    """PlaneWaveModel.exchange_operator with three of four bands occupied in groups of two:
    a multi call of two pairs and a single call per band, equal to the composition."""
    import torch
    from spfft_amd.models.planewave import PlaneWaveBasis, PlaneWaveModel
    basis = PlaneWaveBasis(alat=6.0, ecut=2.0)
    model = PlaneWaveModel(basis, num_transforms=1)
    rng = np.random.default_rng(187)
    nb = 4
    psi = [rng.standard_normal(basis.num_pw) + 1j * rng.standard_normal(basis.num_pw)
           for _ in range(nb)]
    psi = [torch.as_tensor(p / np.linalg.norm(p), device=gpu) for p in psi]
    occ = [2.0, 1.0, 0.0, 0.5]
    composed = model.exchange_operator(psi, occ, unfused=True)
    out = {}
    counts = _batch_scopes(lambda: out.update(x=model.exchange_operator(psi, occ, max_batch=2)))
    assert model.exchange_transform.fock_fused is True
    assert len(out["x"]) == nb
    for x, y in zip(out["x"], composed):
        e = max_rel_error(x.cpu().numpy(), y.cpu().numpy())
        print("exchange operator", e)
        assert e < TOL64
    # per band: one multi call of two pairs and one single call
    assert counts.get("multi_accumulate_fock") == nb, counts
    assert counts.get("accumulate_fock") == nb, counts
    if model.exchange_transform.reciprocal_fused:
        assert counts.get("gpu_accumulate_fock_batch") == nb, counts


# ------------------------------------------------- cases run in their own process
def _ten(seed):
    """A transform plus 9 clones at (32, 16, 8) with simple sticks, one a per pair, a shared
    b and kernel, weights of both signs, acc0 and the oracle's update of one call."""
    dims = (32, 16, 8)
    rng = np.random.default_rng(seed)
    idx = create_value_indices(rng, [1.0], 0.7, 1.0, *dims, False)[0]
    ts = _clones(GPU, dims, idx, 10)
    a = [_field(rng, dims) for _ in ts]
    b = _field(rng, dims)
    k = _kernel(idx, dims, "complex")
    weights = [(-1) ** i * (0.5 + 0.25 * i) for i in range(len(ts))]
    upd = _update(idx, a, [b] * 10, [k] * 10, weights, dims, full=True)
    return ts, a, b, k, weights, _acc0(rng, upd), upd


def _case_multi():
    """Ten identical plans into one acc: with batching on, the call runs two batches (8 + 2
    members, in order) and no per-transform pair stage; with SPFFT_BATCH=0 ten of each
    per-transform stage. Both meet the oracle; with batching on a second call accumulates on
    top of the first and the same call from the same acc0 gives the same bits."""
    import torch
    batching = os.environ.get("SPFFT_BATCH", "1") != "0"
    ts, a, b, k, weights, acc0, upd = _ten(190)
    for t in ts:
        assert t.fock_fused is True and t.reciprocal_fused is True
    da = [torch.as_tensor(x, device="cuda") for x in a]
    db, dk = torch.as_tensor(b, device="cuda"), torch.as_tensor(k, device="cuda")

    def call(dacc):
        return sp.multi_transform_accumulate_fock(ts, da, [db] * 10, dk, weights, dacc,
                                                  scaling=sp.Scaling.FULL)

    dacc = torch.as_tensor(acc0, device="cuda")
    counts = _batch_scopes(lambda: call(dacc))
    first = dacc.cpu().numpy().copy()
    e, eu = max_rel_error(first, acc0 + upd), max_rel_error(first - acc0, upd)
    print("multi", e, eu)
    assert e < TOL64 and eu < TOL64
    print("scopes", {x: n for x, n in counts.items() if "fock" in x})
    assert counts.get("multi_accumulate_fock") == 1
    if batching:
        assert counts.get("gpu_accumulate_fock_batch") == 2
        assert "gpu_fock_forward_xy" not in counts and "gpu_fock_backward_xy" not in counts
    else:
        assert "gpu_accumulate_fock_batch" not in counts
        assert counts.get("gpu_fock_forward_xy") == 10
        assert counts.get("gpu_fock_backward_xy") == 10
    # on top of the first result
    call(dacc)
    second = dacc.cpu().numpy()
    e, eu = max_rel_error(second, acc0 + 2 * upd), max_rel_error(second - acc0, 2 * upd)
    print("multi second", e, eu)
    assert e < TOL64 and eu < TOL64
    # the same call from the same acc0: the same bits
    for _ in range(3):
        again = torch.as_tensor(acc0, device="cuda")
        call(again)
        assert again.cpu().numpy().tobytes() == first.tobytes()
    assert all(np.array_equal(x, d.cpu().numpy()) for x, d in zip(a, da))
    assert np.array_equal(b, db.cpu().numpy()) and np.array_equal(k, dk.cpu().numpy())


def _case_streams():
    """The clones on three distinct torch streams (asynchronous): the updates of acc on
    different streams are ordered by events, the result meets the oracle and two runs agree
    bit for bit."""
    import torch
    ts, a, b, k, weights, acc0, upd = _ten(191)
    da = [torch.as_tensor(x, device="cuda") for x in a]
    db, dk = torch.as_tensor(b, device="cuda"), torch.as_tensor(k, device="cuda")
    streams = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    for i, t in enumerate(ts):
        t.set_stream(streams[i % 3], synchronous=False)
    results = []
    for _ in range(2):
        dacc = torch.as_tensor(acc0, device="cuda")
        torch.cuda.synchronize()
        sp.multi_transform_accumulate_fock(ts, da, [db] * 10, dk, weights, dacc,
                                           scaling=sp.Scaling.FULL)
        torch.cuda.synchronize()
        results.append(dacc.cpu().numpy().copy())
        e = max_rel_error(results[-1], acc0 + upd)
        eu = max_rel_error(results[-1] - acc0, upd)
        print("streams", e, eu)
        assert e < TOL64 and eu < TOL64
    assert results[0].tobytes() == results[1].tobytes()


if __name__ == "__main__":
    {"multi": _case_multi, "streams": _case_streams}[sys.argv[1]]()
    print("CASE OK")
