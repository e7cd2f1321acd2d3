"""multi_transform_apply_local_spinor / multi_transform_accumulate_spin_density against the
dense oracle.

A call takes S two-component spinors as 2S transforms (up_0, dn_0, up_1, dn_1, ...). With
psi = backward(input), potential = (v_uu, v_dd, v_ud_re, v_ud_im), v_ud = v_ud_re + i v_ud_im:

    out_up = scale * forward(v_uu psi_up + v_ud psi_dn)
    out_dn = scale * forward(conj(v_ud) psi_up + v_dd psi_dn)
    n_uu += sum_s w_s |psi_up|^2, n_dd += sum_s w_s |psi_dn|^2, n_ud += sum_s w_s psi_up conj(psi_dn)

Host transforms, host arrays, distributed grids, long x lines, x engines that do not fit a
workgroup's LDS twice and SPFFT_BATCH=0 run the composition per spinor; identical C2C GPU
plans with device arrays run the spinor x kernels (both components of a tile in LDS)
between the batched z and y launches, at most 4 spinors per launch.

Bounds: the project's 1e-12 (fp64) and 2e-5 (fp32) on max_rel_error against dense_backward /
dense_forward in double precision. Every result is checked on two consecutive calls, and
the two results must agree bit for bit.

The fits predicate (the engine's line LDS twice plus the x -> column table within 160 KiB)
holds for every compile-time length up to 512 in both precisions (the 512-long fp64 shape
takes 70528 B); the smallest length that fails it is 1024, which test_gpu_engine_too_large
runs.

Run as a program (python tests/test_spinor.py CASE) it executes the case that needs its own
process, because the library reads SPFFT_BATCH when a transform is created."""
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
apply_spinor = sp.multi_transform_apply_local_spinor
spin_density = sp.multi_transform_accumulate_spin_density
WEIGHTS = [1.0, 0.5, 0.25, 0.75, 0.125]


def _centred(idx, dims):
    idx = np.asarray(idx).reshape(-1, 3).astype(np.int64)
    return np.stack([np.where(idx[:, d] > dims[d] // 2, idx[:, d] - dims[d], idx[:, d])
                     for d in range(3)], axis=1)


def _values_at(idx, dims, member, single=False):
    """Frequency values as a function of the index and the member alone (ranks agree)."""
    g = _centred(idx, dims).astype(np.float64)
    a = (0.37 + 0.1 * member) * g[:, 0] + 0.71 * g[:, 1] + 1.13 * g[:, 2] + 0.2 * g[:, 0] * g[:, 1]
    b = 0.5 + 0.5 * np.cos(0.9 * g[:, 0] - (0.4 + 0.05 * member) * g[:, 2] + 0.3 * g[:, 1] * g[:, 2])
    return (b * np.exp(1j * a)).astype(np.complex64 if single else np.complex128)


def _rand_vals(rng, count, single=False):
    v = rng.standard_normal(count) + 1j * rng.standard_normal(count)
    return v.astype(np.complex64 if single else np.complex128)


def _potential(rng, dims, single=False):
    nx, ny, nz = dims
    return rng.uniform(-1, 1, (4, nz, ny, nx)).astype(np.float32 if single else np.float64)


def _spaces(idx, ins, dims):
    return [dense_backward(idx, np.asarray(c).astype(np.complex128), dims) for c in ins]


def _oracle_apply(idx, ins, pot, dims, full, out_idx=None, spaces=None):
    pot = np.asarray(pot).astype(np.float64)
    vud = pot[2] + 1j * pot[3]
    spaces = _spaces(idx, ins, dims) if spaces is None else spaces
    oi = idx if out_idx is None else out_idx
    outs = []
    for u, d in zip(spaces[0::2], spaces[1::2]):
        outs.append(dense_forward(pot[0] * u + vud * d, oi, dims, scale=full))
        outs.append(dense_forward(np.conj(vud) * u + pot[1] * d, oi, dims, scale=full))
    return outs


def _oracle_density(idx, ins, ws, dims, start=None, spaces=None):
    spaces = _spaces(idx, ins, dims) if spaces is None else spaces
    m = np.zeros((4,) + spaces[0].shape) if start is None else np.asarray(start).astype(np.float64).copy()
    for u, d, w in zip(spaces[0::2], spaces[1::2], ws):
        ud = u * np.conj(d)
        m[0] += w * np.abs(u) ** 2
        m[1] += w * np.abs(d) ** 2
        m[2] += w * ud.real
        m[3] += w * ud.imag
    return m


def _transform(pu, dims, idx, r2c=False, single=False):
    nx, ny, nz = dims
    G = sp.GridFloat if single else sp.Grid
    grid = G(nx, ny, nz, nx * ny, pu, 1)
    return grid.create_transform(pu, sp.TransformType.R2C if r2c else sp.TransformType.C2C,
                                 nx, ny, nz, nz, idx)


def _clones(pu, dims, idx, n, single=False):
    t0 = _transform(pu, dims, idx, single=single)
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


def _err_many(got, want):
    return max(max_rel_error(_np(g), w) for g, w in zip(got, want))


# ------------------------------------------------------------------------- host
@pytest.mark.parametrize("dims,single", [((11, 12, 13), False), ((12, 10, 14), True)])
def test_host_against_oracle(dims, single):
    rng = np.random.default_rng(600)
    idx = create_value_indices(rng, [1.0], 0.7, 0.8, *dims, False)[0]
    tol = TOL32 if single else TOL64
    pot = _potential(rng, dims, single)
    for S in (1, 3):
        ts = _clones(HOST, dims, idx, 2 * S, single=single)
        assert ts[0].spinor_fused is False
        ins = [_rand_vals(rng, len(idx), single) for _ in range(2 * S)]
        spaces = _spaces(idx, ins, dims)
        ws = WEIGHTS[:S]
        start = rng.random(pot.shape).astype(pot.dtype)
        want_m = _oracle_density(idx, ins, ws, dims, start, spaces=spaces)
        got = []
        for rep in range(2):
            m = start.copy()
            assert spin_density(ts, ins, ws, m) is m
            err = max_rel_error(m, want_m)
            print(dims, S, "density", rep, err)
            assert err < tol
            got.append(m)
        assert got[0].tobytes() == got[1].tobytes()
        for full in (False, True):
            want = _oracle_apply(idx, ins, pot, dims, full, spaces=spaces)
            outs = []
            for rep in range(2):
                out = [np.array(o) for o in apply_spinor(ts, ins, pot, scaling=_scaling(full))]
                err = _err_many(out, want)
                print(dims, S, "apply", full, rep, err)
                assert err < tol
                outs.append(out)
            for a, b in zip(*outs):
                assert a.tobytes() == b.tobytes()


def test_constant_matrices_without_fft():
    """A constant potential matrix M on a sparse index set with full scaling: out = M c
    exactly (forward(backward(c)) is c on the index set), an oracle that needs no FFT."""
    dims = (9, 8, 10)
    rng = np.random.default_rng(601)
    idx = create_value_indices(rng, [1.0], 0.6, 0.7, *dims, False)[0]
    nx, ny, nz = dims
    ts = _clones(HOST, dims, idx, 4)
    ins = [_rand_vals(rng, len(idx)) for _ in range(4)]
    for vuu, vdd, vre, vim in [(1.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, -1.0),
                               (1.0, -1.0, 0.0, 0.0), (0.75, -0.5, 0.25, 1.5)]:
        pot = np.stack([np.full((nz, ny, nx), v) for v in (vuu, vdd, vre, vim)])
        vud = vre + 1j * vim
        for _ in range(2):
            out = apply_spinor(ts, ins, pot, scaling=sp.Scaling.FULL)
            for s in range(2):
                u, d = ins[2 * s], ins[2 * s + 1]
                assert max_rel_error(out[2 * s], vuu * u + vud * d) < TOL64
                assert max_rel_error(out[2 * s + 1], np.conj(vud) * u + vdd * d) < TOL64


def test_energy_identity():
    """sum_G sum_s conj(c_s) out_s = (1/N) sum_r [v_uu n_uu + v_dd n_dd + 2 (v_ud_re n_ud_re +
    v_ud_im n_ud_im)] with w = 1 and full scaling: both calls and both sign conventions."""
    dims = (9, 8, 10)
    rng = np.random.default_rng(602)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, False)[0]
    ts = _clones(HOST, dims, idx, 2)
    ins = [_rand_vals(rng, len(idx)) for _ in range(2)]
    pot = _potential(rng, dims)
    out = apply_spinor(ts, ins, pot, scaling=sp.Scaling.FULL)
    m = np.zeros_like(pot)
    spin_density(ts, ins, [1.0], m)
    lhs = sum(np.vdot(c, o) for c, o in zip(ins, out))
    rhs = (pot[0] * m[0] + pot[1] * m[1] + 2 * (pot[2] * m[2] + pot[3] * m[3])).sum() / np.prod(dims)
    assert abs(lhs.imag) < TOL64 * abs(lhs)  # the matrix is Hermitian
    assert abs(lhs.real - rhs) < TOL64 * abs(rhs)


def test_out_is_in_and_repeated_potential_pointers():
    dims = (9, 8, 10)
    rng = np.random.default_rng(603)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, False)[0]
    ts = _clones(HOST, dims, idx, 4)
    ins = [_rand_vals(rng, len(idx)) for _ in range(4)]
    pot = _potential(rng, dims)
    want = _oracle_apply(idx, ins, pot, dims, True)
    for _ in range(2):
        bufs = [c.copy() for c in ins]
        res = apply_spinor(ts, bufs, pot, outputs=bufs, scaling=sp.Scaling.FULL)
        assert all(r is b for r, b in zip(res, bufs))
        assert _err_many(bufs, want) < TOL64
    keep = [c.copy() for c in ins]
    apply_spinor(ts, ins, pot)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ins, keep))  # inputs otherwise unchanged
    # one array for all four entries
    v = pot[0]
    same = np.stack([v, v, v, v])
    want = _oracle_apply(idx, ins, same, dims, True)
    for _ in range(2):
        assert _err_many(apply_spinor(ts, ins, [v, v, v, v], scaling=sp.Scaling.FULL), want) < TOL64


def test_zero_spinors():
    from spfft_amd.ops._lib import lib
    assert apply_spinor([], [], None) == []
    m = np.ones((4, 4, 5, 6))
    assert spin_density([], [], [], m) is m and np.all(m == 1)
    for pre in ("spfft_amd_", "spfft_amd_float_"):
        assert getattr(lib(), pre + "multi_transform_apply_local_spinor")(0, None, None, None, None, 0) == 0
        assert getattr(lib(), pre + "multi_transform_accumulate_spin_density")(0, None, None, None, None) == 0


def test_errors_leave_the_transforms_usable():
    from spfft_amd.ops._lib import lib
    from spfft_amd.types import ErrorCode
    rng = np.random.default_rng(605)
    dims = (6, 5, 4)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    ts = _clones(HOST, dims, idx, 2)
    ins = [_rand_vals(rng, len(idx)) for _ in range(2)]
    outs = [np.zeros_like(c) for c in ins]
    pot = _potential(rng, dims)
    m = np.zeros_like(pot)
    ws = (ctypes.c_double * 1)(1.0)
    dims2 = (4, 5, 6)
    other = _transform(HOST, dims2, create_value_indices(rng, [1.0], 1.0, 1.0, *dims2, False)[0])
    fewer = _transform(HOST, dims, idx[:-3])  # equal dims, another element count
    treal = _transform(HOST, dims, create_value_indices(rng, [1.0], 1.0, 1.0, *dims, True)[0], r2c=True)
    invalid = int(ErrorCode.INVALID_PARAMETER)
    a_fn = lib().spfft_amd_multi_transform_apply_local_spinor
    d_fn = lib().spfft_amd_multi_transform_accumulate_spin_density

    def handles(*t):
        return (ctypes.c_void_p * len(t))(*[x.handle.value for x in t])

    def ptrs(*a):
        return (ctypes.c_void_p * len(a))(*[None if x is None else x.ctypes.data for x in a])

    iv, ov = ptrs(*ins), ptrs(*outs)
    pv, mv = ptrs(*pot), ptrs(*m)
    wv = ctypes.cast(ws, ctypes.c_void_p)

    def check():  # the transforms still give a right result
        assert _err_many(apply_spinor(ts, ins, pot), _oracle_apply(idx, ins, pot, dims, False)) < TOL64
        r = np.zeros_like(pot)
        spin_density(ts, ins, [1.0], r)
        assert max_rel_error(r, _oracle_density(idx, ins, [1.0], dims)) < TOL64

    def both(hs):
        assert a_fn(1, hs, iv, pv, ov, 0) == invalid
        assert d_fn(1, hs, iv, wv, mv) == invalid
        check()

    check()
    both(handles(ts[0], ts[0]))    # a repeated grid
    both(None)                     # null transforms with nSpinors > 0
    both(handles(ts[0], other))    # unequal dimensions
    both(handles(ts[0], fewer))    # unequal local element counts
    both(handles(ts[0], treal))    # an R2C member
    treal2 = treal.clone()
    both(handles(treal, treal2))   # two R2C members
    hs = handles(*ts)
    for args in ((None, pv, ov, 0),                         # null inputs
                 (iv, None, ov, 0),                         # null potential
                 (iv, pv, None, 0),                         # null outputs
                 (ptrs(ins[0], None), pv, ov, 0),           # a null input with local values
                 (iv, pv, ptrs(None, outs[1]), 0),          # a null output with local values
                 (iv, ptrs(pot[0], pot[1], None, pot[3]), ov, 0),  # a null potential entry
                 (iv, pv, ov, 7)):                          # a bad scaling
        assert a_fn(1, hs, *args) == invalid
        check()
    assert a_fn(-1, hs, iv, pv, ov, 0) == invalid
    for args in ((None, wv, mv),                            # null inputs
                 (iv, None, mv),                            # null weights
                 (iv, wv, None),                            # null density
                 (ptrs(None, ins[1]), wv, mv),              # a null input with local values
                 (iv, wv, ptrs(m[0], None, m[2], m[3])),    # a null density entry
                 (iv, wv, ptrs(m[0], m[1], m[2], m[0]))):   # equal density pointers
        assert d_fn(1, hs, *args) == invalid
        check()
    assert np.all(m == 0) and all(np.all(o == 0) for o in outs)  # no failed call wrote anything
    # the Python layer's own checks
    with pytest.raises(ValueError):
        apply_spinor(ts[:1], ins[:1], pot)          # an odd number of transforms
    with pytest.raises(ValueError):
        apply_spinor(ts, ins[:1], pot)
    with pytest.raises(ValueError):
        apply_spinor(ts, ins, pot[:3])
    with pytest.raises(ValueError):
        spin_density(ts, ins, [1.0, 2.0], m)
    with pytest.raises(TypeError):
        spin_density(ts, ins, [1.0], m.astype(np.float32))
    with pytest.raises(sp.InvalidParameterError):
        spin_density(ts, ins, [1.0], [m[0], m[1], m[2], m[1]])
    with pytest.raises(sp.InvalidParameterError):
        apply_spinor([ts[0], ts[0]], ins, pot)
    check()
    # the query's arguments
    q = lib().spfft_amd_transform_spinor_fused
    flag = ctypes.c_int(-1)
    assert q(ts[0].handle, ctypes.byref(flag)) == 0 and flag.value == 0
    assert q(ts[0].handle, None) == invalid
    assert q(None, ctypes.byref(flag)) == int(ErrorCode.INVALID_HANDLE)


def _two_ranks(pu, S=2):
    """Each rank passes its values and its slabs of the four arrays; 2S transforms per rank
    (the rank's transforms of 2S distributed grids)."""
    from spfft_amd.parallel import make_distributed, run_ranks
    dims = (12, 11, 8)
    gidx = sphere_indices(*dims, 0.5)
    rng = np.random.default_rng(606)
    gins = [_values_at(gidx, dims, i) for i in range(2 * S)]
    pot = _potential(rng, dims)
    ws = WEIGHTS[:S]
    gspaces = _spaces(gidx, gins, dims)
    want_m = _oracle_density(gidx, gins, ws, dims, spaces=gspaces)

    def body(rank, comm):
        if pu == GPU:
            import torch
            torch.cuda.set_device(0)
        ss = [make_distributed(comm, dims, gidx, processing_unit=pu,
                               exchange_type=sp.ExchangeType.COMPACT_BUFFERED) for _ in range(2 * S)]
        s = ss[0]
        ts = [x.transform for x in ss]
        ins = [_values_at(s.indices, dims, i) for i in range(2 * S)]
        z = slice(s.z_offset, s.z_offset + s.z_length)
        v = np.ascontiguousarray(pot[:, z])
        want = _oracle_apply(gidx, gins, pot, dims, True, out_idx=s.indices, spaces=gspaces)
        dev = (lambda a: a)
        if pu == GPU:
            import torch
            dev = (lambda a: torch.as_tensor(a, device="cuda"))
            sp.timing_enable(True, gpu_stages=False)
        dins, dv = [dev(c) for c in ins], dev(v)
        errs = [0.0]
        for _ in range(2):
            out = apply_spinor(ts, dins, dv, scaling=sp.Scaling.FULL)
            if len(s.indices):
                errs.append(_err_many(out, want))
            m = dev(np.zeros((4, s.z_length, dims[1], dims[0])))
            spin_density(ts, dins, ws, m)
            if s.z_length:  # a rank's slab against the global scale
                errs.append(float(np.max(np.abs(_np(m) - want_m[:, z]))) / float(np.max(np.abs(want_m))))
        return max(errs), ts[0].spinor_fused

    return run_ranks(2, body)


def test_host_two_ranks():
    for err, fused in _two_ranks(HOST):
        assert fused is False
        assert err < TOL64


# ------------------------------------------------------------------------ model
def _check_model(pu, to_dev, S=3):
    from spfft_amd.models.planewave import PlaneWaveBasis, PlaneWaveModel
    basis = PlaneWaveBasis(alat=6.0, ecut=4.0)
    model = PlaneWaveModel(basis, processing_unit=pu, num_transforms=2)
    dims = basis.fft_dims
    idx = basis.indices
    rng = np.random.default_rng(607)
    spinors = [(_rand_vals(rng, len(idx)), _rand_vals(rng, len(idx))) for _ in range(S)]
    occ = WEIGHTS[:S]
    v4 = _potential(rng, dims)
    flat = [c for s in spinors for c in s]
    spaces = _spaces(idx, flat, dims)
    want_h = _oracle_apply(idx, flat, v4, dims, True, spaces=spaces)
    # psi^+ (1, sigma) psi from the oracle's space domains
    want = [0, 0, 0, 0]
    for (u, d), w in zip(zip(spaces[0::2], spaces[1::2]), occ):
        want[0] = want[0] + w * (np.abs(u) ** 2 + np.abs(d) ** 2)
        want[1] = want[1] + w * 2 * (np.conj(u) * d).real            # sigma_x
        want[2] = want[2] + w * 2 * (np.conj(u) * d).imag            # sigma_y
        want[3] = want[3] + w * (np.abs(u) ** 2 - np.abs(d) ** 2)    # sigma_z
    dsp = [(to_dev(u), to_dev(d)) for u, d in spinors]
    got = {}
    for unfused in (False, True):
        for _ in range(2):
            nm = [_np(a) for a in model.spin_density(dsp, occ, unfused=unfused)]
            for a, w, name in zip(nm, want, ("n", "m_x", "m_y", "m_z")):
                err = float(np.max(np.abs(a - w))) / float(np.max(np.abs(want[0])))
                print(name, "composed" if unfused else "fused", err)
                assert err < TOL64
            hs = [np.array(_np(c)) for pair in model.apply_spinor_potential(dsp, to_dev(v4), unfused=unfused)
                  for c in pair]
            err = _err_many(hs, want_h)
            print("spinor", "composed" if unfused else "fused", err)
            assert err < TOL64
        got[unfused] = (nm, hs)
    for a, b in zip(got[False][0], got[True][0]):
        assert float(np.max(np.abs(a - b))) < TOL64 * float(np.max(np.abs(want[0])))
    assert _err_many(got[False][1], got[True][1]) < TOL64
    assert len(model.transforms) == 2  # the band groups of the other operators are unchanged
    return model


def test_host_model_spinor_potential_and_spin_density():
    _check_model(HOST, lambda a: a)


# -------------------------------------------------------------------------- GPU
SENTINEL = -7.25


def _check_gpu(gpu, dims, idx, S, single=False, seed=610, fused=True, scalings=(True,), host=False,
               ts=None):
    """Both calls twice per scaling against the oracle, the two results bit for bit; the
    timing scopes and GPU stage names tell which path ran; on the fused path the space
    domains keep a sentinel. `host`: host arrays."""
    import torch
    rng = np.random.default_rng(seed)
    assert len(idx) > 0
    if ts is None:
        ts = _clones(GPU, dims, idx, 2 * S, single=single)
    if fused is not None:
        assert ts[0].spinor_fused is fused
    ins = [_rand_vals(rng, len(idx), single) for _ in range(2 * S)]
    pot = _potential(rng, dims, single)
    ws = WEIGHTS[:S]
    start = rng.random(pot.shape).astype(pot.dtype)
    dev = (lambda a: a) if host else (lambda a: torch.as_tensor(a, device=gpu))
    dins, dpot = [dev(c) for c in ins], dev(pot)
    tol = TOL32 if single else TOL64
    spaces = [t.space_domain(GPU) for t in ts]
    for s in spaces:
        s.fill_(SENTINEL)
    ref = _spaces(idx, ins, dims)
    want_m = _oracle_density(idx, ins, ws, dims, start, spaces=ref)
    calls = 0
    sp.timing_reset()
    sp.timing_enable(True)
    try:
        for full in scalings:
            want = _oracle_apply(idx, ins, pot, dims, full, spaces=ref)
            outs, ms = [], []
            for rep in range(2):
                out = apply_spinor(ts, dins, dpot, scaling=_scaling(full))
                outs.append([np.array(_np(o)) for o in out])
                m = dev(start.copy())
                spin_density(ts, dins, ws, m)
                ms.append(np.array(_np(m)))
                err, merr = _err_many(outs[-1], want), max_rel_error(ms[-1], want_m)
                print(dims, S, "apply", err, "density", merr)
                assert err < tol
                assert merr < tol
                calls += 1
            for a, b in zip(*outs):
                assert a.tobytes() == b.tobytes()
            assert ms[0].tobytes() == ms[1].tobytes()  # the sum order is fixed
        for t in ts:
            t.synchronize()
        counts = _scope_counts(sp.timing_json())
    finally:
        sp.timing_enable(False)
    for d, c in zip(dins, ins):
        assert np.array_equal(_np(d), c)  # the inputs are not modified
    if fused is not None:
        assert counts.get("multi_apply_local_spinor") == calls
        assert counts.get("multi_accumulate_spin_density") == calls
        groups = (S + 3) // 4
        if fused:
            assert counts.get("gpu_apply_local_spinor_batch") == groups * calls, counts
            assert counts.get("gpu_accumulate_spin_density_batch") == groups * calls, counts
            assert counts.get("x_spinor_apply") == groups * calls, counts
            assert counts.get("x_spinor_density") == groups * calls, counts
            for name in counts:  # no scalar x stage, no multiply pass
                assert "x_apply" not in name and "x_density" not in name, counts
                assert name not in ("mul", "multiply", "density"), counts
            for s in spaces:  # the space domains are untouched
                assert bool((s == SENTINEL).all())
        else:
            assert "gpu_apply_local_spinor_batch" not in counts, counts
            assert "gpu_accumulate_spin_density_batch" not in counts, counts
            assert "x_spinor_apply" not in counts and "x_spinor_density" not in counts, counts
    return ts


def _sticks(rng, dims, fill=0.7):
    return create_value_indices(rng, [1.0], fill, 1.0, *dims, False)[0]


# x length by engine: 16 / 64 compile-time powers of two, 100 / 60 mixed radix, 11 run-time,
# 17 one prime pass (its result lands in the second half of a line region), 67 Bluestein.
# 7 rows leave a partial tile; fill 0.7 leaves x columns without sticks (the x -> column
# table), 1.0 is the dense case.
@pytest.mark.gpu
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("fill", [0.7, 1.0])
@pytest.mark.parametrize("nx", [16, 64, 100, 60, 11, 17, 67])
def test_gpu_fused_x_lengths(gpu, nx, fill, centered):
    dims = (nx, 7, 6)
    rng = np.random.default_rng(611)
    idx = _sticks(rng, dims, fill)
    if centered:
        idx = center_indices(dims, [idx])[0]
    ts = _check_gpu(gpu, dims, idx, 2, scalings=(True, False) if fill == 1.0 else (True,))
    assert ts[0].apply_local_fused and ts[0].density_fused


# full tiles of compile-time engines: the density's register path (64 x 16 rows) and the
# 512-thread shapes, whose two regions take most of a workgroup's LDS
@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(64, 16, 3), (128, 16, 2), (512, 8, 2), (480, 4, 2)])
def test_gpu_fused_full_tiles(gpu, dims):
    rng = np.random.default_rng(612)
    _check_gpu(gpu, dims, _sticks(rng, dims), 3)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 4, 5])
def test_gpu_fused_spinor_counts(gpu, S):
    """1, 2 and 4 spinors in one launch; 5 run as 4 + 1."""
    dims = (20, 9, 6)
    rng = np.random.default_rng(613)
    _check_gpu(gpu, dims, _sticks(rng, dims), S)


@pytest.mark.gpu
def test_gpu_fused_fp32(gpu):
    dims = (32, 32, 32)
    _check_gpu(gpu, dims, sphere_indices(*dims, 0.5), 2, single=True, scalings=(True, False))


@pytest.mark.gpu
def test_gpu_out_is_in(gpu):
    import torch
    dims = (12, 10, 16)
    rng = np.random.default_rng(614)
    idx = _sticks(rng, dims)
    ts = _clones(GPU, dims, idx, 4)
    assert ts[0].spinor_fused is True
    ins = [_rand_vals(rng, len(idx)) for _ in range(4)]
    pot = _potential(rng, dims)
    want = _oracle_apply(idx, ins, pot, dims, True)
    dpot = torch.as_tensor(pot, device=gpu)
    for _ in range(2):
        bufs = [torch.as_tensor(c, device=gpu) for c in ins]
        res = apply_spinor(ts, bufs, dpot, outputs=bufs, scaling=sp.Scaling.FULL)
        assert all(r is b for r, b in zip(res, bufs))
        assert _err_many(bufs, want) < TOL64
    # repeated potential pointers
    v = dpot[1]
    want = _oracle_apply(idx, ins, np.stack([pot[1]] * 4), dims, True)
    dins = [torch.as_tensor(c, device=gpu) for c in ins]
    assert _err_many(apply_spinor(ts, dins, [v, v, v, v], scaling=sp.Scaling.FULL), want) < TOL64


@pytest.mark.gpu
def test_gpu_density_order_is_fixed(gpu):
    """S = 4 in one call equals, bit for bit, the same call repeated, and matches four S = 1
    calls within the bound."""
    import torch
    dims = (20, 9, 6)
    rng = np.random.default_rng(615)
    idx = _sticks(rng, dims)
    ts = _clones(GPU, dims, idx, 8)
    ins = [_rand_vals(rng, len(idx)) for _ in range(8)]
    dins = [torch.as_tensor(c, device=gpu) for c in ins]
    ws = WEIGHTS[:4]
    res = []
    for _ in range(2):
        m = torch.zeros((4, dims[2], dims[1], dims[0]), dtype=torch.float64, device=gpu)
        spin_density(ts, dins, ws, m)
        res.append(m.cpu().numpy())
    assert res[0].tobytes() == res[1].tobytes()
    one = torch.zeros_like(m)
    for s in range(4):
        spin_density(ts[:2], dins[2 * s:2 * s + 2], ws[s:s + 1], one)
    assert max_rel_error(res[0], one.cpu().numpy()) < TOL64
    assert max_rel_error(res[0], _oracle_density(idx, ins, ws, dims)) < TOL64


# ------------------------------------------------------------- composed routes
@pytest.mark.gpu
def test_gpu_long_x_runs_composed(gpu):
    dims = (2048, 4, 4)
    rng = np.random.default_rng(616)
    ts = _check_gpu(gpu, dims, _sticks(rng, dims, fill=0.5), 1, fused=False)
    assert ts[0].apply_local_fused is False


@pytest.mark.gpu
def test_gpu_engine_too_large_runs_composed(gpu):
    """The smallest x length whose engine does not fit a workgroup's LDS twice (1024: 140160
    B per region in fp64): the scalar x stages are fused, the spinor stages are not."""
    dims = (1024, 4, 2)
    rng = np.random.default_rng(617)
    ts = _check_gpu(gpu, dims, _sticks(rng, dims, fill=0.5), 1, fused=False)
    assert ts[0].apply_local_fused is True and ts[0].density_fused is True
    assert _transform(GPU, (512, 4, 2), _sticks(rng, (512, 4, 2), fill=0.5)).spinor_fused is True


@pytest.mark.gpu
def test_gpu_host_arrays_run_composed(gpu):
    dims = (20, 9, 6)
    rng = np.random.default_rng(618)
    idx = _sticks(rng, dims)
    ts = _clones(GPU, dims, idx, 4)
    assert ts[0].spinor_fused is True  # the plans would; host arrays do not
    sp.timing_reset()
    _check_gpu(gpu, dims, idx, 2, fused=None, host=True, ts=ts)
    counts = _scope_counts(sp.timing_json())
    assert counts.get("multi_apply_local_spinor") == 2 and counts.get("multi_accumulate_spin_density") == 2
    assert "gpu_apply_local_spinor_batch" not in counts and "gpu_accumulate_spin_density_batch" not in counts


@pytest.mark.gpu
def test_gpu_two_virtual_ranks_run_composed(gpu):
    sp.timing_reset()
    try:
        results = _two_ranks(GPU)
        counts = _scope_counts(sp.timing_json())
    finally:
        sp.timing_enable(False)
    for err, fused in results:
        assert fused is False
        assert err < TOL64
    assert counts.get("multi_apply_local_spinor") == 4 and counts.get("multi_accumulate_spin_density") == 4
    assert "gpu_apply_local_spinor_batch" not in counts and "gpu_accumulate_spin_density_batch" not in counts


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
def test_gpu_model_spinor_potential_and_spin_density(gpu):
    import torch
    model = _check_model(GPU, lambda a: torch.as_tensor(a, device=gpu), S=5)
    assert model.transforms[0].spinor_fused is True


# ------------------------------------------------- cases run in their own process
def _case_multi():
    """Two spinors on identical plans: with batching on the spinor x kernels run, with
    SPFFT_BATCH=0 the composition does; the query follows."""
    batching = os.environ.get("SPFFT_BATCH", "1") != "0"
    dims = (20, 9, 6)
    rng = np.random.default_rng(620)
    _check_gpu("cuda", dims, _sticks(rng, dims), 2, fused=batching)


if __name__ == "__main__":
    {"multi": _case_multi}[sys.argv[1]]()
    print("CASE OK")
