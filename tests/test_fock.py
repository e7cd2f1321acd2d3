"""accumulate_fock: acc += w * a * backward(K * (scale * forward(conj(a) * b))) in one
call, the exchange (Fock) pair operator of hybrid functionals, against the dense oracle
acc0 + w * a * dense_backward(idx, K * dense_forward(conj(a) * b, idx, dims, scale), dims).
Host transforms run the plain composition. GPU C2C transforms whose x lines fit one
workgroup run the fused x stages (the forward x stage stages conj(a) * b into LDS, the
backward x stage accumulates from LDS; the space domain is never formed); R2C and long x
lines pass through the space domain with one pointwise kernel at either end. The z stage
between them is apply_reciprocal's, fused or composed independently.

Inputs: a and b of unit variance; K the real Gaussian or the complex integer translation
phase of tests/test_reciprocal.py (|K| <= 1); w = -0.75; acc0 random, scaled to
max|update|. Every result is checked on two consecutive calls, the whole acc against the
oracle and acc - acc0 against the update alone, so that neither a dropped acc0 nor a wrong
weight can hide.

Bounds: the project's 1e-12 (fp64) and 2e-5 (fp32) on max_rel_error. A CPU emulation of
the composition in working precision gives 1.5e-7 to 3e-7 (fp32) and <= 6e-16 (fp64) for
the update alone, <= 7e-8 and <= 2e-16 for the whole acc.

Run as a program (python tests/test_fock.py CASE) it executes the case that needs its own
process, because the library reads SPFFT_INTER_BYTES and SPFFT_LOG when a grid or
transform is created."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import spfft_amd as sp  # noqa: E402
from spfft_amd.utils.indices import (center_indices, create_value_indices,  # noqa: E402
                                     sphere_indices)
from spfft_amd.utils.oracle import dense_backward, dense_forward, max_rel_error  # noqa: E402

GPU = sp.ProcessingUnit.GPU
HOST = sp.ProcessingUnit.HOST
TOL64, TOL32 = 1e-12, 2e-5
SHIFT = (1, 2, 3)  # (s_x, s_y, s_z) of the translation kernel
W = -0.75


def _centred(idx, dims):
    idx = np.asarray(idx).reshape(-1, 3).astype(np.int64)
    return np.stack([np.where(idx[:, d] > dims[d] // 2, idx[:, d] - dims[d], idx[:, d])
                     for d in range(3)], axis=1)


def _kernel(idx, dims, kind, single=False):
    """'real': Gaussian on centred G; 'complex': integer translation phase."""
    g = _centred(idx, dims).astype(np.float64)
    if kind == "real":
        c = max(1.0, sum(n * n for n in dims) / 16.0)
        return np.exp(-(g ** 2).sum(axis=1) / c).astype(np.float32 if single else np.float64)
    ph = sum(g[:, d] * SHIFT[d] / dims[d] for d in range(3))
    return np.exp(-2j * np.pi * ph).astype(np.complex64 if single else np.complex128)


def _field(rng, dims, r2c=False, single=False):
    """Unit variance, [z][y][x]."""
    nx, ny, nz = dims
    if r2c:
        return rng.standard_normal((nz, ny, nx)).astype(np.float32 if single else np.float64)
    f = (rng.standard_normal((nz, ny, nx)) + 1j * rng.standard_normal((nz, ny, nx))) / np.sqrt(2)
    return f.astype(np.complex64 if single else np.complex128)


def _oracle(idx, a, b, k, dims, r2c=False, full=False):
    """(update w * a * u, scaled forward values c(G)) in double precision."""
    wide = np.float64 if r2c else np.complex128
    a64, b64 = np.asarray(a).astype(wide), np.asarray(b).astype(wide)
    vals = dense_forward(np.conj(a64) * b64, idx, dims, r2c=r2c, scale=full)
    u = dense_backward(idx, np.asarray(k).astype(np.complex128) * vals, dims, r2c=r2c)
    return W * a64 * u, vals


def _acc0(rng, upd):
    """Random, scaled to max|update|, in the update's dtype class."""
    x = rng.uniform(-1, 1, upd.shape)
    if np.iscomplexobj(upd):
        x = x + 1j * rng.uniform(-1, 1, upd.shape)
    return x * np.max(np.abs(upd))


def _twice(call, fetch, acc0, upd, tol, label=""):
    """Two consecutive calls: the whole acc against acc0 + n * update, and acc - acc0
    against n * update alone. `acc0` is what the accumulated array held before (in its
    own precision)."""
    acc0 = np.asarray(acc0)
    for n in (1, 2):
        call()
        got = fetch()
        e_acc = max_rel_error(got.astype(upd.dtype), acc0.astype(upd.dtype) + n * upd)
        e_upd = max_rel_error(got.astype(upd.dtype) - acc0.astype(upd.dtype), n * upd)
        print(label, "call", n, "acc", e_acc, "update", e_upd)
        assert e_acc < tol
        assert e_upd < tol


def _transform(pu, dims, idx, r2c=False, single=False):
    nx, ny, nz = dims
    G = sp.GridFloat if single else sp.Grid
    grid = G(nx, ny, nz, nx * ny, pu, 1)
    return grid.create_transform(pu, sp.TransformType.R2C if r2c else sp.TransformType.C2C,
                                 nx, ny, nz, nz, idx)


def _scaling(full):
    return sp.Scaling.FULL if full else sp.Scaling.NONE


def _dtype(r2c, single):
    if r2c:
        return np.float32 if single else np.float64
    return np.complex64 if single else np.complex128


# ------------------------------------------------------------------------- host
@pytest.mark.parametrize("r2c", [False, True])
def test_roll_identity_host(r2c):
    """The translation kernel on the dense index set with full scaling rolls the pair
    density: acc0 + w a roll(conj(a) b), an oracle that needs no FFT."""
    dims = (12, 10, 14)
    rng = np.random.default_rng(70)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, r2c)[0]
    a, b = _field(rng, dims, r2c), _field(rng, dims, r2c)
    k = _kernel(idx, dims, "complex")
    upd = W * a * np.roll(np.conj(a) * b, (SHIFT[2], SHIFT[1], SHIFT[0]), axis=(0, 1, 2))
    ref, _ = _oracle(idx, a, b, k, dims, r2c=r2c, full=True)
    assert max_rel_error(ref, upd) < TOL64
    acc0 = _acc0(rng, upd)
    acc = acc0.copy()
    t = _transform(HOST, dims, idx, r2c=r2c)
    assert t.fock_fused is False
    a_in, b_in = a.copy(), b.copy()
    _twice(lambda: t.accumulate_fock(a, b, k, W, acc, scaling=sp.Scaling.FULL), lambda: acc, acc0,
           upd, TOL64, "roll")
    assert np.array_equal(a, a_in) and np.array_equal(b, b_in)


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("dims,r2c,single", [((11, 12, 13), False, False),
                                             ((16, 32, 64), False, False),
                                             ((12, 10, 14), True, False),
                                             ((32, 32, 32), False, True)])
def test_host_accumulate_fock(dims, r2c, single, kind):
    rng = np.random.default_rng(71)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, r2c)[0]
    a, b = _field(rng, dims, r2c, single), _field(rng, dims, r2c, single)
    k = _kernel(idx, dims, kind, single)
    t = _transform(HOST, dims, idx, r2c=r2c, single=single)
    tol = TOL32 if single else TOL64
    for full in (False, True):
        upd, wvals = _oracle(idx, a, b, k, dims, r2c=r2c, full=full)
        acc0 = _acc0(rng, upd).astype(_dtype(r2c, single))
        acc = acc0.copy()
        vals = np.full(len(idx), -1, dtype=np.complex64 if single else np.complex128)
        assert t.accumulate_fock(a, b, k, W, acc, values=vals, scaling=_scaling(full)) is acc
        verr = max_rel_error(vals, wvals)
        print(dims, kind, "full" if full else "none", "values", verr)
        assert verr < tol
        acc[...] = acc0
        # (without the values output)
        _twice(lambda: t.accumulate_fock(a, b, k, W, acc, scaling=_scaling(full)), lambda: acc,
               acc0, upd, tol, f"{dims} {kind} {'full' if full else 'none'}")


def test_arguments_are_checked():
    rng = np.random.default_rng(72)
    dims = (6, 5, 4)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    a, b = _field(rng, dims), _field(rng, dims)
    k = _kernel(idx, dims, "real")
    t = _transform(HOST, dims, idx)
    acc = np.zeros_like(a)
    with pytest.raises(TypeError):
        t.accumulate_fock(a.astype(np.complex64), b, k, W, acc)
    with pytest.raises(TypeError):
        t.accumulate_fock(a, b.real.copy(), k, W, acc)
    with pytest.raises(TypeError):
        t.accumulate_fock(a, b, k, W, acc.astype(np.complex64))
    with pytest.raises(TypeError):
        t.accumulate_fock(a, b, k.astype(np.float32), W, acc)
    with pytest.raises(ValueError):
        t.accumulate_fock(a[:-1], b, k, W, acc)
    with pytest.raises(ValueError):
        t.accumulate_fock(a, b, k, W, acc.reshape(-1))
    with pytest.raises(ValueError):
        t.accumulate_fock(a, b, k[:-1], W, acc)
    with pytest.raises(ValueError):
        t.accumulate_fock(a, b, k, W, acc, values=np.zeros(len(idx) - 1, dtype=np.complex128))
    with pytest.raises(TypeError):
        t.accumulate_fock(a, b, k, W, acc, values=np.zeros(len(idx), dtype=np.complex64))
    with pytest.raises(ValueError):
        t.accumulate_fock(a, b, k, W, acc, scaling=7)
    assert not acc.any()
    # the native checks (the Python layer never passes a null array or a bad scaling)
    from spfft_amd.ops._lib import lib
    from spfft_amd.types import ErrorCode
    fn = lib().spfft_amd_transform_accumulate_fock
    pa, pb, pk, pacc = a.ctypes.data, b.ctypes.data, k.ctypes.data, acc.ctypes.data
    assert fn(t.handle, pa, pb, pk, 0, W, None, None, 0) == int(ErrorCode.INVALID_PARAMETER)
    assert fn(t.handle, pa, pb, None, 0, W, pacc, None, 0) == int(ErrorCode.INVALID_PARAMETER)
    assert fn(t.handle, None, pb, pk, 0, W, pacc, None, 0) == int(ErrorCode.INVALID_PARAMETER)
    assert fn(t.handle, pa, pb, pk, 0, W, pacc, None, 7) == int(ErrorCode.INVALID_PARAMETER)
    assert not acc.any()
    # and the transform still works
    upd, _ = _oracle(idx, a, b, k, dims)
    assert max_rel_error(t.accumulate_fock(a, b, k, W, acc), upd) < TOL64


def _rank_body(pu, dims, gidx, a, b, acc0, upd, kind, exchange):
    """Each rank passes its slab of a, b and acc and its part of K."""
    from spfft_amd.parallel import make_distributed

    def body(rank, comm):
        kw = {"exchange_type": exchange} if exchange is not None else {}
        if pu == GPU:
            import torch
            torch.cuda.set_device(0)
        s = make_distributed(comm, dims, gidx, processing_unit=pu, **kw)
        t = s.transform
        k = _kernel(s.indices, dims, kind)
        z = slice(s.z_offset, s.z_offset + s.z_length)
        sa, sb = np.ascontiguousarray(a[z]), np.ascontiguousarray(b[z])
        acc = acc0[z].copy()  # (the ranks share acc0 and compare against it)
        wvals = dense_forward(np.conj(a) * b, s.indices, dims, scale=True)
        if pu == GPU:
            import torch
            sa, sb, acc, k = (torch.as_tensor(x, device="cuda") for x in (sa, sb, acc, k))
            vals = torch.zeros(len(s.indices), dtype=torch.complex128, device="cuda")
        else:
            vals = np.zeros(len(s.indices), dtype=np.complex128)
        host = (lambda x: x.cpu().numpy()) if pu == GPU else (lambda x: x)
        errs = []
        scale = float(np.max(np.abs(upd)))  # a rank's slab against the global scale
        for n in (1, 2):
            t.accumulate_fock(sa, sb, k, W, acc, values=vals, scaling=sp.Scaling.FULL)
            if s.z_length:
                got = host(acc)
                errs.append(float(np.max(np.abs(got - (acc0[z] + n * upd[z])))) /
                            float(np.max(np.abs(acc0 + n * upd))))
                errs.append(float(np.max(np.abs((got - acc0[z]) - n * upd[z]))) / (n * scale))
            errs.append(max_rel_error(host(vals), wvals))
        plan = t.exchange_plan() if pu == GPU else None
        return max(errs), t.fock_fused, t.reciprocal_fused, plan, s.z_length

    return body


def _distributed(P, pu, dims, exchange, kind="complex", seed=73):
    from spfft_amd.parallel import run_ranks
    gidx = sphere_indices(*dims, 0.5)
    rng = np.random.default_rng(seed)
    a, b = _field(rng, dims), _field(rng, dims)
    upd, _ = _oracle(gidx, a, b, _kernel(gidx, dims, kind), dims, full=True)
    acc0 = _acc0(rng, upd)
    return run_ranks(P, _rank_body(pu, dims, gidx, a, b, acc0, upd, kind, exchange))


def test_host_two_ranks():
    for err, fused, _, _, _ in _distributed(2, HOST, (12, 11, 8), None):
        assert fused is False
        assert err < TOL64


# -------------------------------------------------------------------------- GPU
def _check_gpu(gpu, dims, idx, kind, r2c=False, single=False, seed=80, fused=True,
               zfused=None, scalings=(True, False), same=False):
    """Per scaling: twice against the oracle with a sentinel-filled space domain (fused
    plans must leave it bit-identical), then the values output."""
    import torch
    rng = np.random.default_rng(seed)
    assert len(idx) > 0
    a = _field(rng, dims, r2c, single)
    b = a if same else _field(rng, dims, r2c, single)
    k = _kernel(idx, dims, kind, single)
    t = _transform(GPU, dims, idx, r2c=r2c, single=single)
    assert t.fock_fused is fused
    if zfused is not None:
        assert t.reciprocal_fused is zfused
    da, dk = torch.as_tensor(a, device=gpu), torch.as_tensor(k, device=gpu)
    db = da if same else torch.as_tensor(b, device=gpu)
    tol = TOL32 if single else TOL64
    space = t.space_domain(GPU)
    for full in scalings:
        upd, wvals = _oracle(idx, a, b, k, dims, r2c=r2c, full=full)
        acc0 = _acc0(rng, upd).astype(_dtype(r2c, single))
        dacc = torch.as_tensor(acc0, device=gpu)
        space.fill_(-7.25)
        sentinel = space.clone()
        label = f"{dims} {'fp32' if single else 'fp64'} {kind} {'full' if full else 'none'}"
        _twice(lambda: t.accumulate_fock(da, db, dk, W, dacc, scaling=_scaling(full)),
               lambda: dacc.cpu().numpy(), acc0, upd, tol, label)
        if fused:
            flat = (lambda x: x if r2c else torch.view_as_real(x))
            assert torch.equal(flat(space), flat(sentinel))
        vals = torch.full((len(idx),), -1, dtype=t._prec.torch_complex, device=gpu)
        t.accumulate_fock(da, db, dk, W, dacc, values=vals, scaling=_scaling(full))
        verr = max_rel_error(vals.cpu().numpy(), wvals)
        print(label, "values", verr)
        assert verr < tol
        assert torch.equal(da, torch.as_tensor(a, device=gpu))
        assert torch.equal(db, torch.as_tensor(b, device=gpu))
    return t


# x length by engine: 16 / 64 FftCT, 60 / 240 FftMR, 11 / 100 run-time; ny = 13 leaves the
# last y block partial, ny = 3 has fewer rows than one block. Sticks and z fill 0.7: some x
# hold no column, and the run-table sticks make the z stage run composed while the x stages
# run fused.
@pytest.mark.gpu
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("ny", [13, 3])
@pytest.mark.parametrize("nx", [16, 64, 60, 240, 11, 100])
def test_gpu_fused_x_lengths(gpu, nx, ny, centered):
    dims = (nx, ny, 5)
    rng = np.random.default_rng(81)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    if centered:
        idx = center_indices(dims, [idx])[0]
    _check_gpu(gpu, dims, idx, "complex" if centered else "real", scalings=(True,))
    _check_gpu(gpu, dims, idx, "real" if centered else "complex", scalings=(False,))


# simple sticks (z fill 1.0): the fused z stage between the fused x stages
@pytest.mark.gpu
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("ny", [13, 3])
@pytest.mark.parametrize("nx", [64, 60])
def test_gpu_fused_simple_sticks(gpu, nx, ny, centered):
    dims = (nx, ny, 5)
    rng = np.random.default_rng(82)
    idx = create_value_indices(rng, [1.0], 0.7, 1.0, *dims, False)[0]
    if centered:
        idx = center_indices(dims, [idx])[0]
    _check_gpu(gpu, dims, idx, "complex", zfused=True)


# run-time engine with a generic prime pass: 17 (one pass), 51 = 3 x 17 (two passes); 67:
# Bluestein in LDS
@pytest.mark.gpu
@pytest.mark.parametrize("ny", [13, 3])
@pytest.mark.parametrize("nx", [17, 51, 67])
def test_gpu_fused_prime_lengths(gpu, nx, ny):
    dims = (nx, ny, 5)
    rng = np.random.default_rng(83)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    _check_gpu(gpu, dims, idx, "complex")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_gpu_fused_dense_columns(gpu, kind):
    """A sphere of radius N/2: every x holds a column, the x stages skip the column table."""
    dims = (32, 32, 32)
    _check_gpu(gpu, dims, sphere_indices(*dims, 0.5), kind)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(32, 32, 32), (512, 3, 5), (240, 6, 10)])
def test_gpu_fused_fp32(gpu, dims):
    rng = np.random.default_rng(84)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    _check_gpu(gpu, dims, idx, "complex", single=True)
    _check_gpu(gpu, dims, idx, "real", single=True, scalings=(True,))


# R2C (packed-real x stage) and x lines beyond one workgroup run composed through the
# space domain
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("dims,r2c", [((16, 12, 10), True), ((2048, 3, 5), False)])
def test_gpu_composed_fallbacks(gpu, dims, r2c, kind):
    rng = np.random.default_rng(85)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, r2c)[0]
    _check_gpu(gpu, dims, idx, kind, r2c=r2c, fused=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_gpu_matches_torch_composition(gpu, kind):
    """Against product -> apply_reciprocal -> addcmul_ on the same transform; then host
    pointers for every array; then a is b."""
    import torch
    dims = (64, 13, 5)
    rng = np.random.default_rng(86)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    a, b = _field(rng, dims), _field(rng, dims)
    k = _kernel(idx, dims, kind)
    t = _transform(GPU, dims, idx)
    assert t.fock_fused is True
    da, db, dk = (torch.as_tensor(x, device=gpu) for x in (a, b, k))
    for full in (False, True):
        upd, wvals = _oracle(idx, a, b, k, dims, full=full)
        acc0 = _acc0(rng, upd)
        cvals = torch.zeros(len(idx), dtype=torch.complex128, device=gpu)
        u = t.apply_reciprocal(dk, space=da.conj() * db, values=cvals, scaling=_scaling(full))
        composed = torch.as_tensor(acc0, device=gpu).addcmul_(da, u, value=W)
        dacc = torch.as_tensor(acc0, device=gpu)
        vals = torch.zeros_like(cvals)
        assert t.accumulate_fock(da, db, dk, W, dacc, values=vals, scaling=_scaling(full)) is dacc
        assert max_rel_error(dacc.cpu().numpy(), composed.cpu().numpy()) < TOL64
        assert max_rel_error((dacc - torch.as_tensor(acc0, device=gpu)).cpu().numpy(),
                             (composed - torch.as_tensor(acc0, device=gpu)).cpu().numpy()) < TOL64
        assert max_rel_error(vals.cpu().numpy(), cvals.cpu().numpy()) < TOL64
        # host pointers for a, b, K, acc and values
        hacc, hvals = acc0.copy(), np.zeros(len(idx), dtype=np.complex128)
        a_in, b_in = a.copy(), b.copy()
        _twice(lambda: t.accumulate_fock(a, b, k, W, hacc, values=hvals, scaling=_scaling(full)),
               lambda: hacc, acc0, upd, TOL64, "host pointers")
        assert max_rel_error(hvals, wvals) < TOL64
        assert np.array_equal(a, a_in) and np.array_equal(b, b_in)
    # a is b: the pair density |a|^2, device and host pointers
    t2 = _check_gpu(gpu, dims, idx, kind, same=True, scalings=(True,))
    upd, _ = _oracle(idx, a, a, k, dims, full=True)
    acc0 = _acc0(rng, upd)
    hacc = acc0.copy()
    _twice(lambda: t2.accumulate_fock(a, a, k, W, hacc, scaling=sp.Scaling.FULL), lambda: hacc,
           acc0, upd, TOL64, "a is b, host")


@pytest.mark.gpu
def test_gpu_stream_order(gpu):
    import torch
    dims = (64, 13, 5)
    rng = np.random.default_rng(87)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    a, b = _field(rng, dims), _field(rng, dims)
    k = _kernel(idx, dims, "complex")
    upd, wvals = _oracle(idx, a, b, k, dims)
    acc0 = _acc0(rng, upd)
    t = _transform(GPU, dims, idx)
    da, db, dk, dacc = (torch.as_tensor(x, device=gpu) for x in (a, b, k, acc0))
    t.set_stream(torch.cuda.current_stream(), synchronous=False)
    vals = torch.zeros(len(idx), dtype=torch.complex128, device=gpu)
    for n in (1, 2):  # successive calls update acc in call order
        out = t.accumulate_fock(da, db, dk, W, dacc, values=vals)
        doubled, vdoubled = out * 2, vals * 2  # ordered after the call by the stream alone
        torch.cuda.synchronize()
        assert max_rel_error(doubled.cpu().numpy(), 2 * (acc0 + n * upd)) < TOL64
        assert max_rel_error(doubled.cpu().numpy() - 2 * acc0, 2 * n * upd) < TOL64
        assert max_rel_error(vdoubled.cpu().numpy(), 2 * wvals) < TOL64


def _stage_names(t, call):
    sp.timing_reset()
    sp.timing_enable(True)
    try:
        for _ in range(3):
            call()
        t.synchronize()
        tree = sp.timing_json()
    finally:
        sp.timing_enable(False)
    gpu_node = [n for n in tree["timings"] if n["identifier"] == "gpu"]
    assert gpu_node, tree
    return {d["identifier"]: {s["identifier"]: s for s in d["sub-timings"]}
            for d in gpu_node[0]["sub-timings"]}


@pytest.mark.gpu
@pytest.mark.parametrize("dims,r2c,zfill", [((64, 13, 5), False, 1.0), ((64, 13, 5), False, 0.7),
                                            ((16, 12, 10), True, 1.0)])
def test_gpu_stage_timing_names(gpu, dims, r2c, zfill):
    """Fused x stages: forward x_pair+y, backward y+x_fock. Composed (R2C): forward pair
    and x+y, backward y+x and fock. The z and exchange names are apply_reciprocal's."""
    import torch
    rng = np.random.default_rng(88)
    idx = create_value_indices(rng, [1.0], 0.7 if not r2c else 1.0, zfill, *dims, r2c)[0]
    t = _transform(GPU, dims, idx, r2c=r2c)
    da, db = (torch.as_tensor(_field(rng, dims, r2c), device=gpu) for _ in range(2))
    dacc = torch.zeros_like(da)
    dk = torch.as_tensor(_kernel(idx, dims, "real"), device=gpu)
    dirs = _stage_names(t, lambda: t.accumulate_fock(da, db, dk, W, dacc))
    assert t.fock_fused is (not r2c)
    assert t.reciprocal_fused is (zfill == 1.0)
    fwd = {"x_pair+y"} if t.fock_fused else {"pair", "x+y"}
    bwd = {"y+x_fock"} if t.fock_fused else {"y+x", "fock"}
    if t.reciprocal_fused:
        assert set(dirs["forward"]) == fwd | {"exchange", "z_reciprocal"}, dirs
        assert set(dirs["backward"]) == bwd | {"exchange"}, dirs
    else:
        assert set(dirs["forward"]) == fwd | {"exchange", "z", "multiply"}, dirs
        assert set(dirs["backward"]) == bwd | {"z", "exchange"}, dirs
    for d in dirs.values():
        for node in d.values():
            assert node["count"] == 3, node


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_gpu_two_ranks(gpu, kind):
    results = _distributed(2, GPU, (12, 11, 8), sp.ExchangeType.COMPACT_BUFFERED, kind)
    for err, fused, _, _, _ in results:
        assert fused
        assert err < TOL64


# The pipelined exchange under accumulate_fock: the pair x stage and y forward of plane
# chunk k release it for the forward exchange, y backward and the accumulating x stage of
# chunk k start when it has arrived back. Three virtual ranks of one GPU, K plane chunks x
# I stick blocks forced; "capped" also caps the intermediate at one full plane, so each
# chunk of 5 planes runs as at least 3 plane ranges.
@pytest.mark.gpu
@pytest.mark.parametrize("chunks,blocks,capped", [(1, 1, False), (2, 2, False), (2, 1, True)])
def test_gpu_virtual_ranks_pipelined(gpu, chunks, blocks, capped, monkeypatch):
    dims = (20, 18, 30)
    nx, ny, nz = dims
    monkeypatch.setenv("SPFFT_EXCH_CHUNKS", str(chunks))
    monkeypatch.setenv("SPFFT_EXCH_STICK_BLOCKS", str(blocks))
    if capped:
        monkeypatch.setenv("SPFFT_INTER_BYTES", str(nx * (ny + 8) * 16))
    results = _distributed(3, GPU, dims, sp.ExchangeType.COMPACT_BUFFERED, seed=89)
    for err, fused, zfused, plan, planes in results:
        print("K x I", plan[:2], "peer writes", plan[2], "planes", planes, "z fused", zfused, err)
        assert fused
        assert plan[:3] == (chunks, blocks, False), plan
        assert err < TOL64


@pytest.mark.gpu
def test_gpu_pipelined_stage_timing_names(gpu, monkeypatch):
    """A fused call under the pipelined exchange (2 plane chunks x 2 stick blocks, three
    virtual ranks): forward x_pair+y, exchange-tail, z_reciprocal, then backward
    exchange+y+x_fock, once per call and rank."""
    import torch
    from spfft_amd.parallel import make_distributed, run_ranks
    dims, P, calls = (20, 18, 30), 3, 3
    monkeypatch.setenv("SPFFT_EXCH_CHUNKS", "2")
    monkeypatch.setenv("SPFFT_EXCH_STICK_BLOCKS", "2")
    gidx = sphere_indices(*dims, 0.5)
    rng = np.random.default_rng(93)
    a, b = _field(rng, dims), _field(rng, dims)

    def body(rank, comm):
        torch.cuda.set_device(0)
        s = make_distributed(comm, dims, gidx, processing_unit=GPU,
                             exchange_type=sp.ExchangeType.COMPACT_BUFFERED)
        t = s.transform
        z = slice(s.z_offset, s.z_offset + s.z_length)
        dk = torch.as_tensor(_kernel(s.indices, dims, "real"), device="cuda")
        da, db = (torch.as_tensor(np.ascontiguousarray(x[z]), device="cuda") for x in (a, b))
        dacc = torch.zeros_like(da)
        for _ in range(calls):
            t.accumulate_fock(da, db, dk, W, dacc)
        t.synchronize()
        return t.fock_fused, t.reciprocal_fused, t.exchange_plan()

    sp.timing_reset()
    sp.timing_enable(True)
    try:
        results = run_ranks(P, body)
        tree = sp.timing_json()
    finally:
        sp.timing_enable(False)
    for fused, zfused, plan in results:
        assert plan[:3] == (2, 2, False), plan
        assert fused and zfused
    gpu_node = [n for n in tree["timings"] if n["identifier"] == "gpu"]
    assert gpu_node, tree
    dirs = {d["identifier"]: {x["identifier"]: x for x in d["sub-timings"]}
            for d in gpu_node[0]["sub-timings"]}
    # (exchange-span: the data plane's own interval next to the stages, not a stage)
    assert set(dirs["forward"]) - {"exchange-span"} == {"x_pair+y", "exchange-tail",
                                                        "z_reciprocal"}, dirs
    assert set(dirs["backward"]) - {"exchange-span"} == {"exchange+y+x_fock"}, dirs
    for d in dirs.values():
        for name, node in d.items():
            if name != "exchange-span":
                assert node["count"] == calls * P, node


def _subprocess_case(case, env):
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], cwd=REPO, env=e,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "CASE OK" in r.stdout, (r.stdout + r.stderr)[-4000:]
    return r.stdout + r.stderr


@pytest.mark.gpu
def test_gpu_capped_intermediate(gpu):
    """An intermediate capped at two full planes of (16, 16, 12): at least three plane
    ranges (the plan's inter_planes, from its SPFFT_LOG line), each with its own pair of
    launches in either direction; the plan line names the fock choice after reciprocal=."""
    import re
    out = _subprocess_case("capped", {"SPFFT_INTER_BYTES": str(2 * 16 * (16 + 8) * 16),
                                      "SPFFT_LOG": "1"})
    assert "fused True" in out
    m = re.search(r"inter_planes=(\d+) apply_local=fused density=fused reciprocal=\w+ fock=fused \|",
                  out)
    assert m, out[-2000:]
    assert -(-12 // int(m.group(1))) >= 3, m.group(0)


@pytest.mark.gpu
def test_gpu_exchange_operator(gpu):
    """PlaneWaveModel.exchange_operator: the fused calls against the torch composition and
    against the dense oracle of one pair."""
    import torch
    from spfft_amd.models.planewave import PlaneWaveBasis, PlaneWaveModel
    basis = PlaneWaveBasis(alat=6.0, ecut=2.0)
    model = PlaneWaveModel(basis, num_transforms=1)
    rng = np.random.default_rng(90)
    nb = 3
    psi = [rng.standard_normal(basis.num_pw) + 1j * rng.standard_normal(basis.num_pw)
           for _ in range(nb)]
    psi = [torch.as_tensor(p / np.linalg.norm(p), device=gpu) for p in psi]
    occ = [2.0, 1.0, 0.0]
    fused = model.exchange_operator(psi, occ)
    composed = model.exchange_operator(psi, occ, unfused=True)
    assert model.exchange_transform.fock_fused is True
    assert len(fused) == nb
    for x, y in zip(fused, composed):
        assert x.shape == psi[0].shape
        assert max_rel_error(x.cpu().numpy(), y.cpu().numpy()) < TOL64
    # band 1 against the dense oracle: sum over occupied a of -f_a a u_ab, projected
    dims = basis.fft_dims
    real = [dense_backward(basis.indices, p.cpu().numpy(), dims) for p in psi]
    pidx, pk = model.exchange_indices, model.exchange_kernel_host
    acc = np.zeros_like(real[1])
    for f, a in zip(occ, real):
        if f == 0.0:
            continue
        c = dense_forward(np.conj(a) * real[1], pidx, dims, scale=True)
        acc += -f * a * dense_backward(pidx, pk * c, dims)
    want = dense_forward(acc, basis.indices, dims, scale=True)
    assert max_rel_error(fused[1].cpu().numpy(), want) < TOL64


def test_host_exchange_operator():
    from spfft_amd.models.planewave import PlaneWaveBasis, PlaneWaveModel
    basis = PlaneWaveBasis(alat=6.0, ecut=2.0)
    model = PlaneWaveModel(basis, processing_unit=HOST, num_transforms=1)
    rng = np.random.default_rng(91)
    psi = [rng.standard_normal(basis.num_pw) + 1j * rng.standard_normal(basis.num_pw)
           for _ in range(2)]
    occ = [2.0, 1.0]
    x, y = model.exchange_operator(psi, occ), model.exchange_operator(psi, occ, unfused=True)
    assert model.exchange_transform.fock_fused is False
    for p, q in zip(x, y):
        assert max_rel_error(p, q) < TOL64


# ---------------------------------------------- pinned cases of tools/fuzz_ops.py
# The operator sweep (tests/test_fuzz_ops.py) reaches these by chance; here they always run:
# its case runner on hand-written configurations (two calls, the whole acc and acc minus its
# start against the dense oracle, the values output, a, b and K unchanged, a sentinel-filled
# space domain bit-identical on a fused plan), under the sweep's bound of 1e-10. Every stick
# is full (z fill 1.0), so nothing but the exchange decides between the fused and the
# composed z stage.
SKEWED = [((4, 32, 6), [1, 2, 1], [1, 0, 2]), ((3, 128, 4), [0, 1, 1], [1, 1, 0]),
          ((2, 64, 5), [1, 0], [0, 1])]


def _pinned(**choices):
    import importlib.util
    if "fuzz_ops" not in sys.modules:
        spec = importlib.util.spec_from_file_location("fuzz_ops",
                                                      os.path.join(REPO, "tools", "fuzz_ops.py"))
        sys.modules["fuzz_ops"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules["fuzz_ops"])
    mod = sys.modules["fuzz_ops"]
    desc, err, tol, facts = mod.run_case(mod.fixed_case("fock", z_fill=1.0, **choices))
    print(desc, err, facts)
    assert err < tol
    return facts


@pytest.mark.gpu
@pytest.mark.parametrize("dims,sticks,planes", SKEWED)
def test_gpu_unbuffered_skewed_distributions(gpu, dims, sticks, planes):
    """UNBUFFERED (peer writes) on the skewed splits of test_gpu_transform's test of that
    name: the fused pair x stages on peer-written sides around the composed z stage; ranks
    without planes pass empty a, b and acc, ranks without sticks an empty K and values."""
    for f in _pinned(dims=dims, stick_dist=sticks, plane_dist=planes, exchange="UNBUFFERED"):
        assert f["plan"][2] is True, f
        assert f["fused"] is True and f["reciprocal_fused"] is False, f


@pytest.mark.gpu
@pytest.mark.parametrize("dims,sticks,planes", SKEWED)
def test_gpu_compact_chunks_skewed_distributions(gpu, dims, sticks, planes):
    """The same splits under the pipelined COMPACT_BUFFERED exchange, two plane chunks
    forced: ranks with fewer planes than chunks run empty chunks, ranks without sticks
    launch the fused z stage over an empty range."""
    for f in _pinned(dims=dims, stick_dist=sticks, plane_dist=planes, chunks=2):
        assert f["plan"][0] == 2 and f["plan"][2] is False, f
        assert f["fused"] is True and f["reciprocal_fused"] is True, f


@pytest.mark.gpu
@pytest.mark.parametrize("dims,fused,zfused", [((16, 2048, 4), True, True), ((4, 4, 4096), True, None),
                                               ((2048, 4, 16), False, True)])
def test_gpu_beside_a_long_axis(gpu, dims, fused, zfused):
    """The fused x stages between four-step y passes and behind a long z; the fused z stage
    between composed x stages."""
    (f,) = _pinned(dims=dims)
    assert f["fused"] is fused, f
    if zfused is not None:
        assert f["reciprocal_fused"] is zfused, f


# ------------------------------------------------- cases run in their own process
def _case_capped():
    dims = (16, 16, 12)
    rng = np.random.default_rng(92)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    t = _check_gpu("cuda", dims, idx, "complex")
    print("fused", t.fock_fused)


if __name__ == "__main__":
    {"capped": _case_capped}[sys.argv[1]]()
    print("CASE OK")
