"""multi_transform_reciprocal_fan_out / fan_in against the dense oracle, per member.

Fan-out: c = scale * forward_0(f); space_i = backward_i(K_i * c). Fan-in: space_0 =
backward_0(sum_i K_i * (scale * forward_i(f_i))), the other members' space domains
unchanged. Host transforms, distributed grids, run-table sticks, host arrays and n > 8
run the composition per transform; identical GPU plans with the fused z stage whose z
line region fits a workgroup's LDS twice run the fan kernels (one workgroup per stick
block looping over the members).

Kernels with |K| <= 1: the real Gaussian exp(-|G|^2 / c_i) and the complex integer
translation phase with a different shift per member; on the dense index set with full
scaling the phase rolls the field, an oracle that needs no FFT.

Bounds: the project's 1e-12 (fp64) and 2e-5 (fp32) on max_rel_error. Every result is
checked on two consecutive calls. The i G_d kernels of the model are not bounded by 1:
the model tests normalise nothing, because the host composition meets 1e-12 against the
dense oracle on the shape they use (max_rel_error divides by the largest modulus of the
reference, and the kernel's growth scales reference and error alike; measured 4e-16 to
1.1e-15 on the host engine before the bound was fixed).

Run as a program (python tests/test_reciprocal_fan.py CASE) it executes the case that
needs its own process, because the library reads SPFFT_BATCH when a transform is created."""
import ctypes
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
# (s_x, s_y, s_z) of member i's translation kernel
SHIFTS = [(1, 2, 3), (-2, 1, 0), (0, -1, 2), (3, 0, -1), (2, 2, 2), (-1, -3, 1), (1, 0, 0),
          (0, 4, -2), (-3, 1, 1)]
fan_out = sp.multi_transform_reciprocal_fan_out
fan_in = sp.multi_transform_reciprocal_fan_in


def _centred(idx, dims):
    idx = np.asarray(idx).reshape(-1, 3).astype(np.int64)
    return np.stack([np.where(idx[:, d] > dims[d] // 2, idx[:, d] - dims[d], idx[:, d])
                     for d in range(3)], axis=1)


def _kernel(idx, dims, kind, member=0, single=False):
    """'real': Gaussian on centred G, narrower per member; 'complex': member's translation."""
    g = _centred(idx, dims).astype(np.float64)
    if kind == "real":
        c = max(1.0, sum(n * n for n in dims) / 16.0) / (1 + member)
        return np.exp(-(g ** 2).sum(axis=1) / c).astype(np.float32 if single else np.float64)
    s = SHIFTS[member]
    ph = sum(g[:, d] * s[d] / dims[d] for d in range(3))
    return np.exp(-2j * np.pi * ph).astype(np.complex64 if single else np.complex128)


def _kernels(idx, dims, kind, n, single=False):
    return [_kernel(idx, dims, kind, i, single) for i in range(n)]


def _field(rng, dims, r2c=False, single=False):
    nx, ny, nz = dims
    f = rng.standard_normal((nz, ny, nx))
    if r2c:
        return f.astype(np.float32 if single else np.float64)
    f = f + 1j * rng.standard_normal((nz, ny, nx))
    return f.astype(np.complex64 if single else np.complex128)


def _wide(f, r2c):
    return np.asarray(f).astype(np.float64 if r2c else np.complex128)


def _oracle_out(idx, f, ks, dims, r2c=False, full=False):
    """(per member space result, scaled forward values) in double precision."""
    vals = dense_forward(_wide(f, r2c), idx, dims, r2c=r2c, scale=full)
    return [dense_backward(idx, np.asarray(k).astype(np.complex128) * vals, dims, r2c=r2c)
            for k in ks], vals


def _oracle_in(idx, fs, ks, dims, r2c=False, full=False):
    s = 0
    for f, k in zip(fs, ks):
        s = s + np.asarray(k).astype(np.complex128) * dense_forward(_wide(f, r2c), idx, dims,
                                                                    r2c=r2c, scale=full)
    return dense_backward(idx, s, dims, r2c=r2c)


def _transform(pu, dims, idx, r2c=False, single=False):
    nx, ny, nz = dims
    G = sp.GridFloat if single else sp.Grid
    grid = G(nx, ny, nz, nx * ny, pu, 1)
    return grid.create_transform(pu, sp.TransformType.R2C if r2c else sp.TransformType.C2C,
                                 nx, ny, nz, nz, idx)


def _clones(pu, dims, idx, n, r2c=False, single=False):
    t0 = _transform(pu, dims, idx, r2c=r2c, single=single)
    return [t0] + [t0.clone() for _ in range(n - 1)]


def _scaling(full):
    return sp.Scaling.FULL if full else sp.Scaling.NONE


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _scope_counts(tree):
    counts = {}

    def walk(nodes):
        for n in nodes:
            counts[n["identifier"]] = counts.get(n["identifier"], 0) + n["count"]
            walk(n.get("sub-timings", []))

    walk(tree["timings"])
    return counts


# ------------------------------------------------------------------------- host
@pytest.mark.parametrize("r2c", [False, True])
def test_roll_identities_host(r2c):
    """Translation kernels on the dense index set with full scaling: fan-out gives
    np.roll(f, shift_i) per member, fan-in the sum of the rolled members."""
    dims = (12, 10, 14)
    n = 3
    rng = np.random.default_rng(400)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, r2c)[0]
    ks = _kernels(idx, dims, "complex", n)
    ts = _clones(HOST, dims, idx, n, r2c=r2c)
    f = _field(rng, dims, r2c)
    fs = [_field(rng, dims, r2c) for _ in range(n)]

    def roll(a, i):
        s = SHIFTS[i]
        return np.roll(a, (s[2], s[1], s[0]), axis=(0, 1, 2))

    for _ in range(2):
        outs = fan_out(ts, ks, space=f, scaling=sp.Scaling.FULL)
        for i, o in enumerate(outs):
            assert max_rel_error(o, roll(f, i)) < TOL64
    want = sum(roll(x, i) for i, x in enumerate(fs))
    for _ in range(2):
        out = fan_in(ts, ks, spaces=fs, scaling=sp.Scaling.FULL)
        assert max_rel_error(out, want) < TOL64
        for t, x in zip(ts[1:], fs[1:]):  # the other members' space domains are only read
            assert np.array_equal(t.space_domain(HOST), x)


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("dims,r2c,single,n", [((11, 12, 13), False, False, 3),
                                               ((12, 10, 14), True, False, 2),
                                               ((16, 8, 32), False, True, 3)])
def test_host_against_oracle(dims, r2c, single, n, kind):
    rng = np.random.default_rng(401)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, r2c)[0]
    ks = _kernels(idx, dims, kind, n, single)
    ts = _clones(HOST, dims, idx, n, r2c=r2c, single=single)
    assert ts[0].reciprocal_fan_fused(n) is False
    f = _field(rng, dims, r2c, single)
    fs = [_field(rng, dims, r2c, single) for _ in range(n)]
    tol = TOL32 if single else TOL64
    for full in (False, True):
        wants, wvals = _oracle_out(idx, f, ks, dims, r2c=r2c, full=full)
        for rep in range(2):
            vals = np.full(len(idx), -1, dtype=np.complex64 if single else np.complex128)
            outs = fan_out(ts, ks, space=f, values=vals, scaling=_scaling(full))
            assert max_rel_error(vals, wvals) < tol  # the scaled forward values
            for o, w in zip(outs, wants):
                assert max_rel_error(o, w) < tol
        want = _oracle_in(idx, fs, ks, dims, r2c=r2c, full=full)
        for rep in range(2):
            assert max_rel_error(fan_in(ts, ks, spaces=fs, scaling=_scaling(full)), want) < tol


def test_adjointness():
    """sum_i <fan_out(f)_i, g_i> = <f, fan_in_{conj K}(g)> on random data: fan-in with the
    conjugate kernels is the adjoint of fan-out (without scaling both sides carry the
    same factor N)."""
    dims = (9, 8, 10)
    n = 3
    rng = np.random.default_rng(402)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, False)[0]
    ks = _kernels(idx, dims, "complex", n)
    ts = _clones(HOST, dims, idx, n)
    f = _field(rng, dims)
    gs = [_field(rng, dims) for _ in range(n)]
    outs = [np.array(o) for o in fan_out(ts, ks, space=f)]
    lhs = sum(np.vdot(o, g) for o, g in zip(outs, gs))
    back = np.array(fan_in(ts, [np.conj(k) for k in ks], spaces=gs))
    rhs = np.vdot(f, back)
    assert abs(lhs - rhs) < TOL64 * abs(lhs)


def test_zero_and_one_transform():
    rng = np.random.default_rng(403)
    dims = (6, 5, 4)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    t = _transform(HOST, dims, idx)
    f = _field(rng, dims)
    k = _kernel(idx, dims, "complex")
    # n == 0: a no-op
    assert fan_out([], []) == []
    assert fan_in([], []) is None
    from spfft_amd.ops._lib import lib
    assert lib().spfft_amd_multi_transform_reciprocal_fan_out(0, None, int(HOST), None, 0, None, 0) == 0
    assert lib().spfft_amd_multi_transform_reciprocal_fan_in(0, None, int(HOST), None, 0, 0) == 0
    # n == 1: apply_reciprocal, bit for bit
    vals, vals1 = (np.zeros(len(idx), dtype=np.complex128) for _ in range(2))
    single = np.array(t.apply_reciprocal(k, space=f, values=vals1, scaling=sp.Scaling.FULL))
    (out,) = fan_out([t], [k], space=f, values=vals, scaling=sp.Scaling.FULL)
    assert np.array(out).tobytes() == single.tobytes() and vals.tobytes() == vals1.tobytes()
    out = fan_in([t], [k], spaces=[f], scaling=sp.Scaling.FULL)
    assert np.array(out).tobytes() == single.tobytes()


def test_errors_leave_the_transforms_usable():
    from spfft_amd.ops._lib import lib
    from spfft_amd.types import ErrorCode
    rng = np.random.default_rng(404)
    dims = (6, 5, 4)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    ts = _clones(HOST, dims, idx, 2)
    ks = _kernels(idx, dims, "complex", 2)
    f, fs = _field(rng, dims), [_field(rng, dims) for _ in range(2)]
    dims2 = (4, 5, 6)
    other = _transform(HOST, dims2, create_value_indices(rng, [1.0], 1.0, 1.0, *dims2, False)[0])
    fewer = _transform(HOST, dims, idx[:-3])  # equal dims, another element count
    treal = _transform(HOST, dims, create_value_indices(rng, [1.0], 1.0, 1.0, *dims, True)[0],
                       r2c=True)
    invalid = int(ErrorCode.INVALID_PARAMETER)
    out_fn = lib().spfft_amd_multi_transform_reciprocal_fan_out
    in_fn = lib().spfft_amd_multi_transform_reciprocal_fan_in

    def handles(*t):
        return (ctypes.c_void_p * len(t))(*[x.handle.value for x in t])

    pk = (ctypes.c_void_p * 2)(ks[0].ctypes.data, ks[1].ctypes.data)
    holes = (ctypes.c_void_p * 2)(ks[0].ctypes.data, None)
    host = int(HOST)

    def both(hs, kp, scaling=0, location=host):
        assert out_fn(2, hs, location, kp, 1, None, scaling) == invalid
        assert in_fn(2, hs, location, kp, 1, scaling) == invalid
        check()

    def check():  # the transforms still give a right result
        wants, _ = _oracle_out(idx, f, ks, dims)
        for o, w in zip(fan_out(ts, ks, space=f), wants):
            assert max_rel_error(o, w) < TOL64
        assert max_rel_error(fan_in(ts, ks, spaces=fs), _oracle_in(idx, fs, ks, dims)) < TOL64

    check()
    both(handles(ts[0], ts[0]), pk)        # a repeated grid
    both(None, pk)                         # null transforms with n > 0
    both(handles(*ts), None)               # null kernels with n > 0
    both(handles(*ts), holes)              # a null kernels[i] with local values
    both(handles(*ts), pk, scaling=7)      # a bad scaling
    both(handles(ts[0], other), pk)        # unequal dimensions
    both(handles(ts[0], fewer), pk)        # unequal local element counts
    both(handles(ts[0], treal), pk)        # unequal types
    both(handles(*ts), pk, location=int(GPU))  # host transforms have no device space domain
    # the Python layer's own checks
    with pytest.raises(ValueError):
        fan_out(ts, ks[:1], space=f)
    with pytest.raises(TypeError):
        fan_out(ts, [ks[0], _kernel(idx, dims, "real", 1)], space=f)
    with pytest.raises(sp.InvalidParameterError):
        fan_in([ts[0], ts[0]], ks, spaces=fs)
    with pytest.raises(ValueError):
        fan_out(ts, ks, space=f, values=np.zeros(len(idx) - 1, dtype=np.complex128))
    check()
    # the query's arguments
    q = lib().spfft_amd_transform_reciprocal_fan_fused
    flag = ctypes.c_int(-1)
    assert q(ts[0].handle, 3, ctypes.byref(flag)) == 0 and flag.value == 0
    assert q(ts[0].handle, 3, None) == invalid
    assert q(None, 3, ctypes.byref(flag)) == int(ErrorCode.INVALID_HANDLE)


def _two_ranks(pu, exchange, n=2):
    """Each rank passes its slabs and its part of the kernels; n transforms per rank (the
    rank's transforms of n distributed grids)."""
    from spfft_amd.parallel import make_distributed, run_ranks
    dims = (12, 11, 8)
    gidx = sphere_indices(*dims, 0.5)
    rng = np.random.default_rng(405)
    f = _field(rng, dims)
    fs = [_field(rng, dims) for _ in range(n)]
    gks = _kernels(gidx, dims, "complex", n)
    wants, _ = _oracle_out(gidx, f, gks, dims, full=True)
    want_in = _oracle_in(gidx, fs, gks, dims, full=True)

    def body(rank, comm):
        if pu == GPU:
            import torch
            torch.cuda.set_device(0)
        ss = [make_distributed(comm, dims, gidx, processing_unit=pu, exchange_type=exchange)
              for _ in range(n)]
        s = ss[0]
        ts = [x.transform for x in ss]
        ks = _kernels(s.indices, dims, "complex", n)
        z = slice(s.z_offset, s.z_offset + s.z_length)
        sf = np.ascontiguousarray(f[z])
        sfs = [np.ascontiguousarray(x[z]) for x in fs]
        if pu == GPU:
            import torch
            ks = [torch.as_tensor(k, device="cuda") for k in ks]
            sf = torch.as_tensor(sf, device="cuda")
            sfs = [torch.as_tensor(x, device="cuda") for x in sfs]
        errs = [0.0]
        if pu == GPU:
            sp.timing_enable(True, gpu_stages=False)
        for _ in range(2):
            outs = fan_out(ts, ks, space=sf, scaling=sp.Scaling.FULL)
            for o, w in zip(outs, wants):  # a rank's slab against the global scale
                if s.z_length:
                    errs.append(float(np.max(np.abs(_np(o) - w[z]))) / float(np.max(np.abs(w))))
            out = fan_in(ts, ks, spaces=sfs, scaling=sp.Scaling.FULL)
            if s.z_length:
                errs.append(float(np.max(np.abs(_np(out) - want_in[z]))) /
                            float(np.max(np.abs(want_in))))
        return max(errs), ts[0].reciprocal_fan_fused(n)

    return run_ranks(2, body)


def test_host_two_ranks():
    for err, fused in _two_ranks(HOST, sp.ExchangeType.COMPACT_BUFFERED):
        assert fused is False
        assert err < TOL64


# ------------------------------------------------------------------------ model
def _model(pu):
    from spfft_amd.models.planewave import PlaneWaveBasis, PlaneWaveModel
    basis = PlaneWaveBasis(alat=6.0, ecut=4.0)
    return basis, PlaneWaveModel(basis, processing_unit=pu, num_transforms=1)


def _check_model(pu, to_dev):
    basis, model = _model(pu)
    n0, n1, n2 = basis.fft_dims
    unit = 2 * np.pi / basis.alat
    # a single plane wave exp(i G.r), G = unit * (1, -2, 1): its gradient is i G_d times it
    kvec = (1, -2, 1)
    z, y, x = np.meshgrid(np.arange(n2) / n2, np.arange(n1) / n1, np.arange(n0) / n0,
                          indexing="ij")
    wave = np.exp(2j * np.pi * (kvec[0] * x + kvec[1] * y + kvec[2] * z))
    for unfused in (False, True):
        for _ in range(2):
            grads = model.gradient(to_dev(wave), unfused=unfused)
            for d in range(3):
                assert max_rel_error(_np(grads[d]), 1j * unit * kvec[d] * wave) < TOL64
    # random data against the dense oracle with K_d = i G_d, and div(grad f) against
    # apply_reciprocal with -|G|^2
    rng = np.random.default_rng(406)
    f = _field(rng, (n0, n1, n2))
    idx = model.exchange_indices
    ks = [1j * unit * idx[:, d].astype(np.float64) for d in range(3)]
    wants, _ = _oracle_out(idx, f, ks, basis.fft_dims, full=True)
    lap = -(unit ** 2) * (idx.astype(np.float64) ** 2).sum(axis=1)
    t = model.exchange_transform
    want_lap = np.array(_np(t.apply_reciprocal(to_dev(lap), space=to_dev(f),
                                               scaling=sp.Scaling.FULL)))
    for unfused in (False, True):
        grads = model.gradient(to_dev(f), unfused=unfused)
        for g, w in zip(grads, wants):
            err = max_rel_error(_np(g), w)
            print("gradient", "composed" if unfused else "fused", err)
            assert err < TOL64
        div = model.divergence(grads, unfused=unfused)
        err = max_rel_error(_np(div), want_lap)
        print("div grad", "composed" if unfused else "fused", err)
        assert err < TOL64
        assert max_rel_error(_np(div), _oracle_in(idx, wants, ks, basis.fft_dims, full=True)) < TOL64
    return model


def test_host_model_gradient_and_divergence():
    _check_model(HOST, lambda a: a)


# -------------------------------------------------------------------------- GPU
def _check_gpu(gpu, dims, idx, kind, n, r2c=False, single=False, seed=410, fused=True,
               scalings=(True,), host=False, ts=None):
    """Fan-out (with the values output, member 0 in place over the input) and fan-in, twice
    per scaling against the oracle per member; fan-in twice more for identical bits. The
    timing-scope counts tell which path ran. `host`: host arrays at location HOST."""
    import torch
    rng = np.random.default_rng(seed)
    assert len(idx) > 0
    if ts is None:
        ts = _clones(GPU, dims, idx, n, r2c=r2c, single=single)
    t0 = ts[0]
    if fused is not None:
        assert t0.reciprocal_fan_fused(n) is fused
    ks = _kernels(idx, dims, kind, n, single)
    f = _field(rng, dims, r2c, single)
    fs = [_field(rng, dims, r2c, single) for _ in range(n)]
    if host:
        dks, df, dfs, loc = ks, f, fs, HOST
    else:
        dks = [torch.as_tensor(k, device=gpu) for k in ks]
        df, dfs, loc = torch.as_tensor(f, device=gpu), [torch.as_tensor(x, device=gpu) for x in fs], GPU
    tol = TOL32 if single else TOL64
    calls = 0
    sp.timing_reset()
    sp.timing_enable(True, gpu_stages=False)
    try:
        for full in scalings:
            wants, wvals = _oracle_out(idx, f, ks, dims, r2c=r2c, full=full)
            want_in = _oracle_in(idx, fs, ks, dims, r2c=r2c, full=full)
            for rep in range(2):
                if host:
                    vals = np.full(len(idx), -1, dtype=t0._prec.complex)
                else:
                    vals = torch.full((len(idx),), -1, dtype=t0._prec.torch_complex, device=gpu)
                outs = fan_out(ts, dks, space=df, values=vals, location=loc, scaling=_scaling(full))
                verr = max_rel_error(_np(vals), wvals)
                errs = [max_rel_error(_np(o), w) for o, w in zip(outs, wants)]
                print(dims, n, kind, "fan-out", rep, max(errs), verr)
                assert verr < tol
                assert max(errs) < tol
                got = [np.array(_np(fan_in(ts, dks, spaces=dfs, location=loc, scaling=_scaling(full))))
                       for _ in range(2)]
                err = max_rel_error(got[0], want_in)
                print(dims, n, kind, "fan-in", rep, err)
                assert err < tol
                assert got[0].tobytes() == got[1].tobytes()  # the sum order is fixed
                for t, x in zip(ts[1:], fs[1:]):  # the other members' space domains are only read
                    assert np.array_equal(_np(t.space_domain(loc)), x)
                calls += 1
        # without the values output
        outs = fan_out(ts, dks, space=df, location=loc, scaling=_scaling(scalings[-1]))
        assert max(max_rel_error(_np(o), w) for o, w in zip(outs, wants)) < tol
        counts = _scope_counts(sp.timing_json())
    finally:
        sp.timing_enable(False)
    if fused is not None:
        assert counts.get("multi_reciprocal_fan_out") == calls + 1
        assert counts.get("multi_reciprocal_fan_in") == 2 * calls
        if fused:
            assert counts.get("gpu_reciprocal_fan_out_batch") == calls + 1, counts
            assert counts.get("gpu_reciprocal_fan_in_batch") == 2 * calls, counts
        else:
            assert "gpu_reciprocal_fan_out_batch" not in counts, counts
            assert "gpu_reciprocal_fan_in_batch" not in counts, counts
    return ts


def _sticks(rng, dims, r2c=False, fill=0.7):
    return create_value_indices(rng, [1.0], fill, 1.0, *dims, r2c)[0]


# z length by engine: 16 / 64 compile-time, 60 mixed radix, 11 run-time, 17 one prime pass
# (its result lands in the second region of the line LDS), 67 Bluestein. (5, 13) with fill
# 0.7 leaves the last stick block partial.
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("nz", [16, 64, 60, 11, 17, 67])
def test_gpu_fused_z_lengths(gpu, nz, n, centered, kind):
    dims = (5, 13, nz)
    rng = np.random.default_rng(411)
    idx = _sticks(rng, dims)
    if centered:
        idx = center_indices(dims, [idx])[0]
    ts = _check_gpu(gpu, dims, idx, kind, n, scalings=(True, False) if n == 3 else (True,))
    assert ts[0].reciprocal_fused is True


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("dims", [(32, 32, 32), (6, 10, 240)])
def test_gpu_fused_fp32(gpu, dims, kind):
    rng = np.random.default_rng(412)
    idx = sphere_indices(*dims, 0.5) if dims == (32, 32, 32) else _sticks(rng, dims, fill=1.0)
    _check_gpu(gpu, dims, idx, kind, 3, single=True)


# the (0, 0) stick of an R2C transform: the hermitian fill per member (fan-out) and of the
# sum (fan-in) inside the fan kernels
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("case", ["full", "sphere"])
def test_gpu_fused_r2c_zero_stick(gpu, case, kind):
    rng = np.random.default_rng(413)
    if case == "full":
        dims = (16, 12, 10)
        idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, True)[0]
    else:
        dims = (32, 32, 32)
        idx = sphere_indices(*dims, 0.5, r2c=True)
    assert np.any((idx[:, 0] == 0) & (idx[:, 1] == 0))
    _check_gpu(gpu, dims, idx, kind, 3, r2c=True, scalings=(True, False))


@pytest.mark.gpu
def test_gpu_fan_out_overwrites_its_input(gpu):
    """Member 0's result is right although its stick array and space domain are the
    input's, and the roll identity holds on the GPU."""
    import torch
    dims = (12, 10, 16)
    n = 3
    rng = np.random.default_rng(414)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    ts = _clones(GPU, dims, idx, n)
    assert ts[0].reciprocal_fan_fused(n) is True
    dks = [torch.as_tensor(k, device=gpu) for k in _kernels(idx, dims, "complex", n)]
    f = _field(rng, dims)
    space0 = ts[0].space_domain(GPU)
    for _ in range(2):
        space0.copy_(torch.as_tensor(f, device=gpu))
        outs = fan_out(ts, dks, scaling=sp.Scaling.FULL)  # the input already in place
        assert outs[0].data_ptr() == space0.data_ptr()
        for i, o in enumerate(outs):
            s = SHIFTS[i]
            assert max_rel_error(o.cpu().numpy(), np.roll(f, (s[2], s[1], s[0]), axis=(0, 1, 2))) < TOL64


# ------------------------------------------------------------- composed routes
@pytest.mark.gpu
def test_gpu_nine_members_run_composed(gpu):
    dims = (5, 13, 16)
    rng = np.random.default_rng(415)
    ts = _check_gpu(gpu, dims, _sticks(rng, dims), "complex", 9, fused=False)
    assert ts[0].reciprocal_fan_fused(8) is True


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_gpu_run_table_sticks_run_composed(gpu, kind):
    """Sticks that are not simple (z fill 0.7): the composition, whatever the plan says."""
    dims = (13, 5, 64)
    rng = np.random.default_rng(416)
    idx = create_value_indices(rng, [1.0], 0.8, 0.7, *dims, False)[0]
    ts = _clones(GPU, dims, idx, 3)
    fused = ts[0].reciprocal_fan_fused(3)
    assert fused is ts[0].reciprocal_fused
    _check_gpu(gpu, dims, idx, kind, 3, fused=fused, ts=ts)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_gpu_host_arrays_run_composed(gpu, kind):
    dims = (5, 13, 64)
    rng = np.random.default_rng(417)
    idx = _sticks(rng, dims)
    ts = _clones(GPU, dims, idx, 3)
    assert ts[0].reciprocal_fan_fused(3) is True  # the plans would; host arrays do not
    import torch
    sp.timing_reset()
    sp.timing_enable(True, gpu_stages=False)
    try:
        ks = _kernels(idx, dims, kind, 3)
        f = _field(rng, dims)
        fs = [_field(rng, dims) for _ in range(3)]
        wants, wvals = _oracle_out(idx, f, ks, dims, full=True)
        want_in = _oracle_in(idx, fs, ks, dims, full=True)
        for _ in range(2):
            # host kernels and host values at the device space domains
            vals = np.zeros(len(idx), dtype=np.complex128)
            outs = fan_out(ts, ks, space=torch.as_tensor(f, device=gpu), values=vals,
                           scaling=sp.Scaling.FULL)
            assert max_rel_error(vals, wvals) < TOL64
            for o, w in zip(outs, wants):
                assert max_rel_error(o.cpu().numpy(), w) < TOL64
            out = fan_in(ts, ks, spaces=[torch.as_tensor(x, device=gpu) for x in fs],
                         scaling=sp.Scaling.FULL)
            assert max_rel_error(out.cpu().numpy(), want_in) < TOL64
        counts = _scope_counts(sp.timing_json())
    finally:
        sp.timing_enable(False)
    assert "gpu_reciprocal_fan_out_batch" not in counts and "gpu_reciprocal_fan_in_batch" not in counts
    # everything on the host side, space domains included
    _check_gpu(gpu, dims, idx, kind, 3, fused=None, host=True, ts=ts)


@pytest.mark.gpu
def test_gpu_two_virtual_ranks_run_composed(gpu):
    sp.timing_reset()
    try:
        results = _two_ranks(GPU, sp.ExchangeType.COMPACT_BUFFERED)
        counts = _scope_counts(sp.timing_json())
    finally:
        sp.timing_enable(False)
    for err, fused in results:
        assert fused is False
        assert err < TOL64
    assert counts.get("multi_reciprocal_fan_out") == 4 and counts.get("multi_reciprocal_fan_in") == 4
    assert "gpu_reciprocal_fan_out_batch" not in counts and "gpu_reciprocal_fan_in_batch" not in counts


# The hold adds one more copy of the z lines of a stick block to the workgroup's LDS.
# fp64: a run-time line of 4096 elements takes 64 KB in place and 64 KB more for the hold,
# the longest length a probe of the plans found fused (some shorter lengths with ping-pong
# passes, such as 3456, are already out). 5103 = 3^6 x 7 is the longest length probed
# that has the fused z stage of apply_reciprocal (5119, the longest line of one
# workgroup, is prime and runs the long path) but no room for the hold: composed.
@pytest.mark.gpu
@pytest.mark.parametrize("nz,fused", [(512, True), (4096, True), (3456, False), (5103, False)])
def test_gpu_long_z(gpu, nz, fused):
    dims = (4, 4, nz)
    rng = np.random.default_rng(418)
    idx = _sticks(rng, dims, fill=1.0)
    ts = _clones(GPU, dims, idx, 2)
    assert ts[0].reciprocal_fused is True
    _check_gpu(gpu, dims, idx, "complex", 2, fused=fused, ts=ts)


def _subprocess_case(case, env):
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], cwd=REPO, env=e,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "CASE OK" in r.stdout, (r.stdout + r.stderr)[-4000:]
    return r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["0", "1"])
def test_gpu_batch_switch(gpu, batch):
    _subprocess_case("multi", {"SPFFT_BATCH": batch})


@pytest.mark.gpu
def test_gpu_model_gradient_and_divergence(gpu):
    import torch
    model = _check_model(GPU, lambda a: torch.as_tensor(a, device=gpu))
    assert model.exchange_transform.reciprocal_fan_fused(3) is True


# ------------------------------------------------- cases run in their own process
def _case_multi():
    """Three identical plans: with batching on the fan kernels run, with SPFFT_BATCH=0 the
    composition does; the query follows."""
    batching = os.environ.get("SPFFT_BATCH", "1") != "0"
    dims = (5, 13, 64)
    rng = np.random.default_rng(419)
    idx = _sticks(rng, dims)
    for kind in ("real", "complex"):
        ts = _check_gpu("cuda", dims, idx, kind, 3, fused=batching)
        assert ts[0].reciprocal_fused is True


if __name__ == "__main__":
    {"multi": _case_multi}[sys.argv[1]]()
    print("CASE OK")
