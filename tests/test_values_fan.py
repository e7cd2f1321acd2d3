"""multi_transform_accumulate_density_fan / multi_transform_apply_local_fan against the
dense oracle.

Density fan: density += sum_i w_i |backward_i(K_i * values)|^2. Apply-local fan: output =
sum_i L_i * (scale * forward_i(V_i * backward_i(K_i * values))), both in list order, None
kernels the identity. Host transforms, R2C, distributed grids, run-table sticks, host
arrays, long x lines, n > 8 and SPFFT_BATCH=0 run the composition per member; identical
C2C GPU plans with simple sticks and fused x stages whose z line region fits a workgroup's
LDS twice run the value fan z kernels (one workgroup per stick block looping over the
members) around the batched y and x launches.

Kernels with |K|, |L| <= 1: the real Gaussian exp(-|G|^2 / c_i), the complex integer
translation phase with a different shift per member, and i G_d / (N_d / 2); potentials
uniform in [-1, 1]. On the dense index set with full scaling, translation kernels K_i,
L_i = conj(K_i) and constant potentials c_i the operator is (sum_i c_i) * values, an
oracle that needs no FFT.

Bounds: the project's 1e-12 (fp64) and 2e-5 (fp32) on max_rel_error against dense_backward /
dense_forward in double precision. Every result is checked on two consecutive calls.

Run as a program (python tests/test_values_fan.py CASE) it executes the case that needs
its own process, because the library reads SPFFT_BATCH when a transform is created."""
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
density_fan = sp.multi_transform_accumulate_density_fan
apply_fan = sp.multi_transform_apply_local_fan


def _centred(idx, dims):
    idx = np.asarray(idx).reshape(-1, 3).astype(np.int64)
    return np.stack([np.where(idx[:, d] > dims[d] // 2, idx[:, d] - dims[d], idx[:, d])
                     for d in range(3)], axis=1)


def _kernel(idx, dims, kind, member=0, single=False):
    """'real': Gaussian on centred G, narrower per member; 'complex': the member's
    translation; 'grad': i G_d / (N_d / 2), d = member mod 3."""
    g = _centred(idx, dims).astype(np.float64)
    if kind == "real":
        c = max(1.0, sum(n * n for n in dims) / 16.0) / (1 + member)
        return np.exp(-(g ** 2).sum(axis=1) / c).astype(np.float32 if single else np.float64)
    if kind == "grad":
        d = member % 3
        k = 1j * g[:, d] / (dims[d] / 2)
    else:
        s = SHIFTS[member]
        k = np.exp(-2j * np.pi * sum(g[:, d] * s[d] / dims[d] for d in range(3)))
    return k.astype(np.complex64 if single else np.complex128)


def _kernels(idx, dims, kind, n, single=False, none0=False, first=0):
    ks = [_kernel(idx, dims, kind, first + i, single) for i in range(n)]
    if none0 and n:
        ks[0] = None
    return ks


def _values_at(idx, dims, single=False):
    """Frequency values as a function of the index alone (ranks agree on them)."""
    g = _centred(idx, dims).astype(np.float64)
    a = 0.37 * g[:, 0] + 0.71 * g[:, 1] + 1.13 * g[:, 2] + 0.2 * g[:, 0] * g[:, 1]
    b = 0.5 + 0.5 * np.cos(0.9 * g[:, 0] - 0.4 * g[:, 2] + 0.3 * g[:, 1] * g[:, 2])
    return (b * np.exp(1j * a)).astype(np.complex64 if single else np.complex128)


def _rand_vals(rng, count, single=False):
    v = rng.standard_normal(count) + 1j * rng.standard_normal(count)
    return v.astype(np.complex64 if single else np.complex128)


def _potentials(rng, dims, n, single=False):
    nx, ny, nz = dims
    return [rng.uniform(-1, 1, (nz, ny, nx)).astype(np.float32 if single else np.float64)
            for _ in range(n)]


def _wide(k):
    return 1.0 if k is None else np.asarray(k).astype(np.complex128)


def _oracle_density(idx, vals, ks, ws, dims, r2c=False):
    vals = np.asarray(vals).astype(np.complex128)
    rho = 0
    for k, w in zip(ks, ws):
        s = dense_backward(idx, _wide(k) * vals, dims, r2c=r2c)
        rho = rho + w * (s * s if r2c else s.real ** 2 + s.imag ** 2)
    return rho


def _oracle_apply(idx, vals, kin, pots, kout, dims, r2c=False, full=False, out_idx=None):
    """The sum over the members; `out_idx`: the indices of `kout` and of the result (a
    rank's own), by default `idx`."""
    vals = np.asarray(vals).astype(np.complex128)
    out = 0
    for k, v, l in zip(kin, pots, kout):
        s = dense_backward(idx, _wide(k) * vals, dims, r2c=r2c) * np.asarray(v).astype(np.float64)
        out = out + _wide(l) * dense_forward(s, idx if out_idx is None else out_idx, dims, r2c=r2c,
                                             scale=full)
    return out


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


WEIGHTS = [1.0, 0.5, 0.25, 0.75, 0.125, 1.0, 0.5, 0.25, 0.75]


# ------------------------------------------------------------------------- host
@pytest.mark.parametrize("none0", [False, True])
@pytest.mark.parametrize("kind", ["real", "complex", "grad"])
@pytest.mark.parametrize("dims,r2c,single", [((11, 12, 13), False, False),
                                             ((12, 10, 14), True, False),
                                             ((12, 10, 14), False, True),
                                             ((11, 12, 13), True, True)])
def test_host_against_oracle(dims, r2c, single, kind, none0):
    rng = np.random.default_rng(500)
    idx = create_value_indices(rng, [1.0], 0.7, 0.8, *dims, r2c)[0]
    vals = _rand_vals(rng, len(idx), single)
    tol = TOL32 if single else TOL64
    real = np.float32 if single else np.float64
    for n in (1, 2, 4):
        ts = _clones(HOST, dims, idx, n, r2c=r2c, single=single)
        assert ts[0].values_fan_fused(n) is False
        kin = _kernels(idx, dims, kind, n, single, none0)
        kout = _kernels(idx, dims, kind, n, single, none0, first=2)
        pots = _potentials(rng, dims, n, single)
        ws = WEIGHTS[:n]
        rho0 = rng.random(pots[0].shape).astype(real)
        want_rho = rho0.astype(np.float64) + _oracle_density(idx, vals, kin, ws, dims, r2c=r2c)
        for rep in range(2):
            rho = rho0.copy()
            assert density_fan(ts, vals, kin, ws, rho) is rho
            err = max_rel_error(rho, want_rho)
            print(dims, n, kind, "density", rep, err)
            assert err < tol
        for full in (False, True):
            want = _oracle_apply(idx, vals, kin, pots, kout, dims, r2c=r2c, full=full)
            for rep in range(2):
                out = np.array(apply_fan(ts, vals, kin, pots, kout, scaling=_scaling(full)))
                err = max_rel_error(out, want)
                print(dims, n, kind, "apply", full, rep, err)
                assert err < tol


def test_identities_without_fft():
    """Dense index set, full scaling, translation kernels K_i, L_i = conj(K_i), constant
    potentials c_i: the operator is (sum c_i) * values; the density fan sums the rolled
    |psi|^2."""
    dims = (12, 10, 14)
    n = 4
    rng = np.random.default_rng(501)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    vals = _rand_vals(rng, len(idx))
    ks = _kernels(idx, dims, "complex", n)
    ls = [np.conj(k) for k in ks]
    cs = [0.75, -0.5, 0.25, 1.0]
    nx, ny, nz = dims
    pots = [np.full((nz, ny, nx), c) for c in cs]
    ts = _clones(HOST, dims, idx, n)
    psi2 = np.abs(dense_backward(idx, vals, dims)) ** 2
    ws = WEIGHTS[:n]
    want_rho = sum(w * np.roll(psi2, (s[2], s[1], s[0]), axis=(0, 1, 2)) for w, s in zip(ws, SHIFTS))
    for _ in range(2):
        out = apply_fan(ts, vals, ks, pots, ls, scaling=sp.Scaling.FULL)
        assert max_rel_error(out, sum(cs) * vals) < TOL64
        rho = np.zeros((nz, ny, nx))
        density_fan(ts, vals, ks, ws, rho)
        assert max_rel_error(rho, want_rho) < TOL64


def test_adjointness():
    """<u, A v> = <A^+ u, v> with A^+ the call whose kernel lists are swapped and
    conjugated (V is real; without scaling backward and forward are adjoint)."""
    dims = (9, 8, 10)
    n = 3
    rng = np.random.default_rng(502)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, False)[0]
    kin = _kernels(idx, dims, "complex", n)
    kout = _kernels(idx, dims, "grad", n, first=1)
    pots = _potentials(rng, dims, n)
    ts = _clones(HOST, dims, idx, n)
    u, v = _rand_vals(rng, len(idx)), _rand_vals(rng, len(idx))
    av = np.array(apply_fan(ts, v, kin, pots, kout))
    atu = np.array(apply_fan(ts, u, [np.conj(k) for k in kout], pots, [np.conj(k) for k in kin]))
    lhs, rhs = np.vdot(u, av), np.vdot(atu, v)
    assert abs(lhs - rhs) < TOL64 * abs(lhs)


def test_input_is_output_host():
    dims = (9, 8, 10)
    n = 3
    rng = np.random.default_rng(503)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, False)[0]
    kin, kout = _kernels(idx, dims, "complex", n), _kernels(idx, dims, "grad", n)
    pots = _potentials(rng, dims, n)
    ts = _clones(HOST, dims, idx, n)
    vals = _rand_vals(rng, len(idx))
    want = _oracle_apply(idx, vals, kin, pots, kout, dims, full=True)
    for _ in range(2):
        buf = vals.copy()
        assert apply_fan(ts, buf, kin, pots, kout, output=buf, scaling=sp.Scaling.FULL) is buf
        assert max_rel_error(buf, want) < TOL64
    keep = vals.copy()
    apply_fan(ts, vals, kin, pots, kout)
    assert vals.tobytes() == keep.tobytes()  # the input is otherwise not modified


def test_zero_and_one_transform():
    from spfft_amd.ops._lib import lib
    rng = np.random.default_rng(504)
    dims = (6, 5, 4)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    t = _transform(HOST, dims, idx)
    vals = _rand_vals(rng, len(idx))
    (v,) = _potentials(rng, dims, 1)
    # n == 0: a no-op
    assert apply_fan([], None, [], [], []) is None
    rho = np.ones((4, 5, 6))
    assert density_fan([], None, [], [], rho) is rho and np.all(rho == 1)
    assert lib().spfft_amd_multi_transform_apply_local_fan(0, None, None, None, None, None, 0, None, 0) == 0
    assert lib().spfft_amd_multi_transform_accumulate_density_fan(0, None, None, None, 0, None, None) == 0
    # n == 1 with None kernels: apply_local / accumulate_density
    single = np.array(t.apply_local(vals, v, scaling=sp.Scaling.FULL))
    out = np.array(apply_fan([t], vals, [None], [v], [None], scaling=sp.Scaling.FULL))
    assert max_rel_error(out, single) < TOL64
    assert max_rel_error(out, _oracle_apply(idx, vals, [None], [v], [None], dims, full=True)) < TOL64
    rho1, rho2 = np.zeros((4, 5, 6)), np.zeros((4, 5, 6))
    t.accumulate_density(vals, 0.5, rho1)
    density_fan([t], vals, [None], [0.5], rho2)
    assert max_rel_error(rho2, rho1) < TOL64


def test_errors_leave_the_transforms_usable():
    from spfft_amd.ops._lib import lib
    from spfft_amd.types import ErrorCode
    rng = np.random.default_rng(505)
    dims = (6, 5, 4)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    ts = _clones(HOST, dims, idx, 2)
    ks = _kernels(idx, dims, "complex", 2)
    pots = _potentials(rng, dims, 2)
    vals = _rand_vals(rng, len(idx))
    out = np.zeros_like(vals)
    rho = np.zeros((4, 5, 6))
    ws = (ctypes.c_double * 2)(1.0, 0.5)
    dims2 = (4, 5, 6)
    other = _transform(HOST, dims2, create_value_indices(rng, [1.0], 1.0, 1.0, *dims2, False)[0])
    fewer = _transform(HOST, dims, idx[:-3])  # equal dims, another element count
    treal = _transform(HOST, dims, create_value_indices(rng, [1.0], 1.0, 1.0, *dims, True)[0],
                       r2c=True)
    invalid = int(ErrorCode.INVALID_PARAMETER)
    a_fn = lib().spfft_amd_multi_transform_apply_local_fan
    d_fn = lib().spfft_amd_multi_transform_accumulate_density_fan

    def handles(*t):
        return (ctypes.c_void_p * len(t))(*[x.handle.value for x in t])

    pk = (ctypes.c_void_p * 2)(ks[0].ctypes.data, ks[1].ctypes.data)
    pv = (ctypes.c_void_p * 2)(pots[0].ctypes.data, pots[1].ctypes.data)
    vhole = (ctypes.c_void_p * 2)(pots[0].ctypes.data, None)
    iv, ov, rv = vals.ctypes.data, out.ctypes.data, rho.ctypes.data
    wv = ctypes.cast(ws, ctypes.c_void_p)

    def check():  # the transforms still give a right result
        got = apply_fan(ts, vals, ks, pots, ks)
        assert max_rel_error(got, _oracle_apply(idx, vals, ks, pots, ks, dims)) < TOL64
        r = np.zeros((4, 5, 6))
        density_fan(ts, vals, ks, [1.0, 0.5], r)
        assert max_rel_error(r, _oracle_density(idx, vals, ks, [1.0, 0.5], dims)) < TOL64

    def both(hs):
        assert a_fn(2, hs, iv, pk, pv, pk, 1, ov, 0) == invalid
        assert d_fn(2, hs, iv, pk, 1, wv, rv) == invalid
        check()

    check()
    both(handles(ts[0], ts[0]))            # a repeated grid
    both(None)                             # null transforms with n > 0
    both(handles(ts[0], other))            # unequal dimensions
    both(handles(ts[0], fewer))            # unequal local element counts
    both(handles(ts[0], treal))            # unequal types
    hs = handles(*ts)
    for args in ((iv, None, pv, pk, 1, ov, 0),     # null kernelsIn
                 (iv, pk, None, pk, 1, ov, 0),     # null potentials
                 (iv, pk, pv, None, 1, ov, 0),     # null kernelsOut
                 (None, pk, pv, pk, 1, ov, 0),     # null input with local values
                 (iv, pk, pv, pk, 1, None, 0),     # null output with local values
                 (iv, pk, vhole, pk, 1, ov, 0),    # a null potentials[i] with local planes
                 (iv, pk, pv, pk, 1, ov, 7)):      # a bad scaling
        assert a_fn(2, hs, *args) == invalid
        check()
    for args in ((iv, None, 1, wv, rv),    # null kernels
                 (iv, pk, 1, None, rv),    # null weights
                 (None, pk, 1, wv, rv),    # null input with local values
                 (iv, pk, 1, wv, None)):   # null density with local planes
        assert d_fn(2, hs, *args) == invalid
        check()
    assert np.all(rho == 0) and np.all(out == 0)  # no failed call wrote anything
    # the Python layer's own checks
    with pytest.raises(ValueError):
        apply_fan(ts, vals, ks[:1], pots, ks)
    with pytest.raises(ValueError):
        density_fan(ts, vals, ks, [1.0], rho)
    with pytest.raises(TypeError):
        apply_fan(ts, vals, ks, pots, [ks[0], _kernel(idx, dims, "real", 1)])
    with pytest.raises(sp.InvalidParameterError):
        density_fan([ts[0], ts[0]], vals, ks, [1.0, 0.5], rho)
    with pytest.raises(ValueError):
        apply_fan(ts, vals[:-1], ks, pots, ks)
    check()
    # the query's arguments
    q = lib().spfft_amd_transform_values_fan_fused
    flag = ctypes.c_int(-1)
    assert q(ts[0].handle, 3, ctypes.byref(flag)) == 0 and flag.value == 0
    assert q(ts[0].handle, 3, None) == invalid
    assert q(None, 3, ctypes.byref(flag)) == int(ErrorCode.INVALID_HANDLE)


def _two_ranks(pu, exchange, n=3):
    """Each rank passes its values, its part of the kernels and its slabs; n transforms per
    rank (the rank's transforms of n distributed grids)."""
    from spfft_amd.parallel import make_distributed, run_ranks
    dims = (12, 11, 8)
    gidx = sphere_indices(*dims, 0.5)
    rng = np.random.default_rng(506)
    gvals = _values_at(gidx, dims)
    pots = _potentials(rng, dims, n)
    ws = WEIGHTS[:n]
    gkin = _kernels(gidx, dims, "complex", n, none0=True)
    want_rho = _oracle_density(gidx, gvals, gkin, ws, dims)

    def body(rank, comm):
        if pu == GPU:
            import torch
            torch.cuda.set_device(0)
        ss = [make_distributed(comm, dims, gidx, processing_unit=pu, exchange_type=exchange)
              for _ in range(n)]
        s = ss[0]
        ts = [x.transform for x in ss]
        kin = _kernels(s.indices, dims, "complex", n, none0=True)
        kout = _kernels(s.indices, dims, "grad", n, none0=True)
        vals = _values_at(s.indices, dims)
        z = slice(s.z_offset, s.z_offset + s.z_length)
        vs = [np.ascontiguousarray(v[z]) for v in pots]
        want = _oracle_apply(gidx, gvals, gkin, pots, kout, dims, full=True, out_idx=s.indices)
        dev = (lambda a: a)
        if pu == GPU:
            import torch
            dev = (lambda a: None if a is None else torch.as_tensor(a, device="cuda"))
            sp.timing_enable(True, gpu_stages=False)
        dkin, dkout, dvals, dvs = [dev(k) for k in kin], [dev(k) for k in kout], dev(vals), [dev(v) for v in vs]
        errs = [0.0]
        for _ in range(2):
            out = apply_fan(ts, dvals, dkin, dvs, dkout, scaling=sp.Scaling.FULL)
            if len(s.indices):
                errs.append(float(np.max(np.abs(_np(out) - want))) / float(np.max(np.abs(want))))
            rho = dev(np.zeros((s.z_length, dims[1], dims[0])))
            density_fan(ts, dvals, dkin, ws, rho)
            if s.z_length:  # a rank's slab against the global scale
                errs.append(float(np.max(np.abs(_np(rho) - want_rho[z]))) / float(np.max(np.abs(want_rho))))
        return max(errs), ts[0].values_fan_fused(n)

    return run_ranks(2, body)


def test_host_two_ranks():
    for err, fused in _two_ranks(HOST, sp.ExchangeType.COMPACT_BUFFERED):
        assert fused is False
        assert err < TOL64


# ------------------------------------------------------------------------ model
def _check_model(pu, to_dev):
    from spfft_amd.models.planewave import PlaneWaveBasis, PlaneWaveModel
    basis = PlaneWaveBasis(alat=6.0, ecut=4.0)
    model = PlaneWaveModel(basis, processing_unit=pu, num_transforms=2)
    dims = basis.fft_dims
    idx = basis.indices
    unit = 2 * np.pi / basis.alat
    rng = np.random.default_rng(507)
    psi = [_rand_vals(rng, len(idx)) for _ in range(2)]
    occ = [2.0, 0.5]
    v_r, v_tau = _potentials(rng, dims, 2)
    ks = [1j * unit * idx[:, d].astype(np.float64) for d in range(3)]
    want_tau = sum(_oracle_density(idx, c, ks, [0.5 * w] * 3, dims) for c, w in zip(psi, occ))
    want_h = [_oracle_apply(idx, c, [None] + ks, [v_r] + [v_tau] * 3, [None] + [-0.5 * k for k in ks],
                            dims, full=True) for c in psi]
    dpsi = [to_dev(c) for c in psi]
    got = {}
    for unfused in (False, True):
        for _ in range(2):
            tau = _np(model.kinetic_energy_density(dpsi, occ, unfused=unfused))
            err = max_rel_error(tau, want_tau)
            print("tau", "composed" if unfused else "fused", err)
            assert err < TOL64
            hs = [np.array(_np(h)) for h in model.meta_gga_local(dpsi, to_dev(v_r), to_dev(v_tau),
                                                                unfused=unfused)]
            for h, w in zip(hs, want_h):
                err = max_rel_error(h, w)
                print("mgga", "composed" if unfused else "fused", err)
                assert err < TOL64
        got[unfused] = (tau, hs)
    # each against its own unfused=True
    assert max_rel_error(got[False][0], got[True][0]) < TOL64
    for a, b in zip(got[False][1], got[True][1]):
        assert max_rel_error(a, b) < TOL64
    assert len(model.transforms) == 2  # the band groups of the other operators are unchanged
    return model


def test_host_model_tau_and_meta_gga():
    _check_model(HOST, lambda a: a)


# -------------------------------------------------------------------------- GPU
SENTINEL = -7.25


def _check_gpu(gpu, dims, idx, kind, n, r2c=False, single=False, seed=510, fused=True, none0=False,
               scalings=(True,), host=False, ts=None):
    """Both fans twice per scaling against the oracle, the two results bit for bit; the
    timing scopes and GPU stage names tell which path ran; on the fused path the space
    domains keep a sentinel. `host`: host arrays."""
    import torch
    rng = np.random.default_rng(seed)
    assert len(idx) > 0
    if ts is None:
        ts = _clones(GPU, dims, idx, n, r2c=r2c, single=single)
    t0 = ts[0]
    if fused is not None:
        assert t0.values_fan_fused(n) is fused
    kin = _kernels(idx, dims, kind, n, single, none0)
    kout = _kernels(idx, dims, "grad" if kind == "complex" else kind, n, single, none0, first=1)
    vals = _rand_vals(rng, len(idx), single)
    pots = _potentials(rng, dims, n, single)
    ws = WEIGHTS[:n]
    rho0 = rng.random(pots[0].shape).astype(pots[0].dtype)
    dev = (lambda a: a) if host else (lambda a: None if a is None else torch.as_tensor(a, device=gpu))
    dkin, dkout, dvals, dpots = [dev(k) for k in kin], [dev(k) for k in kout], dev(vals), [dev(v) for v in pots]
    tol = TOL32 if single else TOL64
    spaces = [t.space_domain(GPU) for t in ts]
    for s in spaces:
        s.fill_(SENTINEL)
    want_rho = rho0.astype(np.float64) + _oracle_density(idx, vals, kin, ws, dims, r2c=r2c)
    calls = 0
    sp.timing_reset()
    sp.timing_enable(True)
    try:
        for full in scalings:
            want = _oracle_apply(idx, vals, kin, pots, kout, dims, r2c=r2c, full=full)
            outs, rhos = [], []
            for rep in range(2):
                out = apply_fan(ts, dvals, dkin, dpots, dkout, scaling=_scaling(full))
                outs.append(np.array(_np(out)))
                rho = dev(rho0.copy())
                density_fan(ts, dvals, dkin, ws, rho)
                rhos.append(np.array(_np(rho)))
                err, rerr = max_rel_error(outs[-1], want), max_rel_error(rhos[-1], want_rho)
                print(dims, n, kind, "apply", err, "density", rerr)
                assert err < tol
                assert rerr < tol
                calls += 1
            assert outs[0].tobytes() == outs[1].tobytes()  # the sum order is fixed
            assert rhos[0].tobytes() == rhos[1].tobytes()
        for t in ts:
            t.synchronize()
        counts = _scope_counts(sp.timing_json())
    finally:
        sp.timing_enable(False)
    assert np.array_equal(_np(dvals), vals)  # the input is not modified
    if fused is not None:
        assert counts.get("multi_apply_local_fan") == calls
        assert counts.get("multi_accumulate_density_fan") == calls
        if fused:
            assert counts.get("gpu_apply_local_fan_batch") == calls, counts
            assert counts.get("gpu_accumulate_density_fan_batch") == calls, counts
            assert counts.get("z_fan_out") == 2 * calls, counts  # once per call of either fan
            assert counts.get("z_fan_in") == calls, counts
            assert "z" not in counts, counts  # no plain z stage
            for s in spaces:  # the space domains are untouched
                assert bool((s == SENTINEL).all())
        else:
            assert "gpu_apply_local_fan_batch" not in counts, counts
            assert "gpu_accumulate_density_fan_batch" not in counts, counts
            assert "z_fan_out" not in counts and "z_fan_in" not in counts, counts
    return ts


def _sticks(rng, dims, r2c=False, fill=0.7):
    return create_value_indices(rng, [1.0], fill, 1.0, *dims, r2c)[0]


# z length by engine: 16 / 64 compile-time, 60 mixed radix, 11 run-time, 17 one prime pass
# (its result lands in the second region of the line LDS), 67 Bluestein. (5, 13) with fill
# 0.7 leaves the last stick block partial. n = 4 runs with None at member 0.
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("nz", [16, 64, 60, 11, 17, 67])
def test_gpu_fused_z_lengths(gpu, nz, n, centered, kind):
    dims = (5, 13, nz)
    rng = np.random.default_rng(511)
    idx = _sticks(rng, dims)
    if centered:
        idx = center_indices(dims, [idx])[0]
    ts = _check_gpu(gpu, dims, idx, kind, n, none0=(n == 4), scalings=(True, False) if n == 2 else (True,))
    assert ts[0].apply_local_fused and ts[0].density_fused


# x length by engine of the fused x stages between the fans
@pytest.mark.gpu
@pytest.mark.parametrize("nx", [16, 100, 67])
def test_gpu_fused_x_lengths(gpu, nx):
    dims = (nx, 7, 6)
    rng = np.random.default_rng(512)
    _check_gpu(gpu, dims, _sticks(rng, dims), "complex", 3)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("dims", [(32, 32, 32), (6, 10, 240)])
def test_gpu_fused_fp32(gpu, dims, kind):
    rng = np.random.default_rng(513)
    idx = sphere_indices(*dims, 0.5) if dims == (32, 32, 32) else _sticks(rng, dims, fill=1.0)
    _check_gpu(gpu, dims, idx, kind, 3, single=True, none0=(kind == "real"))


@pytest.mark.gpu
def test_gpu_input_is_output(gpu):
    import torch
    dims = (12, 10, 16)
    n = 3
    rng = np.random.default_rng(514)
    idx = _sticks(rng, dims)
    ts = _clones(GPU, dims, idx, n)
    assert ts[0].values_fan_fused(n) is True
    kin, kout = _kernels(idx, dims, "complex", n), _kernels(idx, dims, "grad", n)
    pots = _potentials(rng, dims, n)
    vals = _rand_vals(rng, len(idx))
    want = _oracle_apply(idx, vals, kin, pots, kout, dims, full=True)
    dev = lambda a: torch.as_tensor(a, device=gpu)  # noqa: E731
    dkin, dkout, dpots = [dev(k) for k in kin], [dev(k) for k in kout], [dev(v) for v in pots]
    for _ in range(2):
        buf = dev(vals)
        assert apply_fan(ts, buf, dkin, dpots, dkout, output=buf, scaling=sp.Scaling.FULL) is buf
        assert max_rel_error(buf.cpu().numpy(), want) < TOL64


# ------------------------------------------------------------- composed routes
@pytest.mark.gpu
def test_gpu_nine_members_run_composed(gpu):
    dims = (5, 13, 16)
    rng = np.random.default_rng(515)
    ts = _check_gpu(gpu, dims, _sticks(rng, dims), "complex", 9, fused=False, none0=True)
    assert ts[0].values_fan_fused(8) is True


@pytest.mark.gpu
def test_gpu_run_table_sticks_run_composed(gpu):
    """Four z runs per stick: not simple sticks, so the composition."""
    dims = (13, 5, 64)
    zs = [0, 1, 5, 6, 7, 20, 21, 22, 40, 41]
    idx = np.array([(x, y, z) for x in range(13) for y in range(5) if (x + y) % 3 for z in zs],
                   dtype=np.int32)
    ts = _clones(GPU, dims, idx, 3)
    assert ts[0].reciprocal_fused is False
    _check_gpu(gpu, dims, idx, "complex", 3, fused=False, ts=ts)


@pytest.mark.gpu
def test_gpu_host_arrays_run_composed(gpu):
    dims = (5, 13, 64)
    rng = np.random.default_rng(517)
    idx = _sticks(rng, dims)
    ts = _clones(GPU, dims, idx, 3)
    assert ts[0].values_fan_fused(3) is True  # the plans would; host arrays do not
    sp.timing_reset()
    _check_gpu(gpu, dims, idx, "complex", 3, fused=None, host=True, ts=ts, none0=True)
    counts = _scope_counts(sp.timing_json())
    assert counts.get("multi_apply_local_fan") == 2 and counts.get("multi_accumulate_density_fan") == 2
    assert "gpu_apply_local_fan_batch" not in counts and "gpu_accumulate_density_fan_batch" not in counts


@pytest.mark.gpu
def test_gpu_r2c_runs_composed(gpu):
    dims = (16, 12, 10)
    rng = np.random.default_rng(518)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, True)[0]
    _check_gpu(gpu, dims, idx, "complex", 3, r2c=True, fused=False)


@pytest.mark.gpu
def test_gpu_long_x_runs_composed(gpu):
    dims = (2048, 4, 4)
    rng = np.random.default_rng(519)
    _check_gpu(gpu, dims, _sticks(rng, dims, fill=0.5), "complex", 2, fused=False)


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
    assert counts.get("multi_apply_local_fan") == 4 and counts.get("multi_accumulate_density_fan") == 4
    assert "gpu_apply_local_fan_batch" not in counts and "gpu_accumulate_density_fan_batch" not in counts


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
def test_gpu_model_tau_and_meta_gga(gpu):
    import torch
    model = _check_model(GPU, lambda a: torch.as_tensor(a, device=gpu))
    assert model.transforms[0].values_fan_fused(4) is True


# ------------------------------------------------- cases run in their own process
def _case_multi():
    """Three identical plans: with batching on the fan kernels run, with SPFFT_BATCH=0 the
    composition does; the query follows."""
    batching = os.environ.get("SPFFT_BATCH", "1") != "0"
    dims = (5, 13, 64)
    rng = np.random.default_rng(520)
    idx = _sticks(rng, dims)
    for kind in ("real", "complex"):
        _check_gpu("cuda", dims, idx, kind, 3, fused=batching)


if __name__ == "__main__":
    {"multi": _case_multi}[sys.argv[1]]()
    print("CASE OK")
