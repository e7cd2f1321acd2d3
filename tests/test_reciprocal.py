"""apply_reciprocal: the space domain f becomes backward(K * (scale * forward(f))) in one
call, against the dense oracle dense_backward(idx, K * dense_forward(f, idx, dims, r2c,
scale), dims, r2c). Host transforms run the plain composition; GPU transforms with simple
sticks whose z lines fit one workgroup run the fused z stage (forward z FFT, K multiply,
inverse z FFT in LDS, in place on the stick side); run-table plans, long z lines, fp32
exchange buffers and peer-written stick sides fall back to the composition.

Kernels: the real Gaussian exp(-|G|^2 / c) on centred G, and the complex integer
translation phase exp(-2 pi i (g_x s_x / n_x + g_y s_y / n_y + g_z s_z / n_z)), which is
exactly hermitian and real at the Nyquist planes; with the dense index set and full
scaling its result is np.roll(f, (s_z, s_y, s_x)), an oracle independent of any FFT.

Bounds: the project's 1e-12 (fp64) and 2e-5 (fp32) on max_rel_error. Every result is
checked on two consecutive calls.

Run as a program (python tests/test_reciprocal.py CASE) it executes the case that needs
its own process, because the library reads SPFFT_LOG when a transform is created."""
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
    nx, ny, nz = dims
    f = rng.standard_normal((nz, ny, nx))
    if r2c:
        return f.astype(np.float32 if single else np.float64)
    f = f + 1j * rng.standard_normal((nz, ny, nx))
    return f.astype(np.complex64 if single else np.complex128)


def _oracle(idx, f, k, dims, r2c=False, full=False):
    """(space result, scaled forward values) in double precision."""
    vals = dense_forward(np.asarray(f).astype(np.complex128 if not r2c else np.float64), idx, dims,
                         r2c=r2c, scale=full)
    return dense_backward(idx, np.asarray(k).astype(np.complex128) * vals, dims, r2c=r2c), vals


def _transform(pu, dims, idx, r2c=False, single=False):
    nx, ny, nz = dims
    G = sp.GridFloat if single else sp.Grid
    grid = G(nx, ny, nz, nx * ny, pu, 1)
    return grid.create_transform(pu, sp.TransformType.R2C if r2c else sp.TransformType.C2C,
                                 nx, ny, nz, nz, idx)


def _scaling(full):
    return sp.Scaling.FULL if full else sp.Scaling.NONE


# ------------------------------------------------------------------------- host
@pytest.mark.parametrize("r2c", [False, True])
def test_roll_identity_host(r2c):
    """The translation kernel on the dense index set with full scaling rolls the field: the
    oracle that needs no FFT, checked on the host engine and on the dense oracle itself."""
    dims = (12, 10, 14)
    rng = np.random.default_rng(40)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, r2c)[0]
    f = _field(rng, dims, r2c)
    k = _kernel(idx, dims, "complex")
    want = np.roll(f, (SHIFT[2], SHIFT[1], SHIFT[0]), axis=(0, 1, 2))
    ref, _ = _oracle(idx, f, k, dims, r2c=r2c, full=True)
    assert max_rel_error(ref, want) < TOL64
    t = _transform(HOST, dims, idx, r2c=r2c)
    for _ in range(2):
        out = t.apply_reciprocal(k, space=f, scaling=sp.Scaling.FULL)
        assert max_rel_error(out, want) < TOL64


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("dims,r2c,single", [((11, 12, 13), False, False),
                                             ((16, 32, 64), False, False),
                                             ((12, 10, 14), True, False),
                                             ((32, 32, 32), False, True)])
def test_host_apply_reciprocal(dims, r2c, single, kind):
    rng = np.random.default_rng(41)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, r2c)[0]
    f = _field(rng, dims, r2c, single)
    k = _kernel(idx, dims, kind, single)
    t = _transform(HOST, dims, idx, r2c=r2c, single=single)
    assert t.reciprocal_fused is False
    tol = TOL32 if single else TOL64
    for full in (False, True):
        want, wvals = _oracle(idx, f, k, dims, r2c=r2c, full=full)
        for rep in range(2):
            vals = np.full(len(idx), -1, dtype=np.complex64 if single else np.complex128)
            out = t.apply_reciprocal(k, space=f, values=vals, scaling=_scaling(full))
            err, verr = max_rel_error(out, want), max_rel_error(vals, wvals)
            print(dims, "r2c" if r2c else "c2c", kind, "full" if full else "none", rep, err, verr)
            assert err < tol
            assert verr < tol
        # without the values output
        assert max_rel_error(t.apply_reciprocal(k, space=f, scaling=_scaling(full)), want) < tol


def test_arguments_are_checked():
    rng = np.random.default_rng(42)
    dims = (6, 5, 4)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    f = _field(rng, dims)
    k = _kernel(idx, dims, "real")
    t = _transform(HOST, dims, idx)
    with pytest.raises(TypeError):
        t.apply_reciprocal(k.astype(np.float32), space=f)
    with pytest.raises(TypeError):
        t.apply_reciprocal(_kernel(idx, dims, "complex", single=True), space=f)
    with pytest.raises(TypeError):
        t.apply_reciprocal(np.arange(len(idx)), space=f)
    with pytest.raises(ValueError):
        t.apply_reciprocal(k[:-1], space=f)
    with pytest.raises(ValueError):
        t.apply_reciprocal(k, space=f, values=np.zeros(len(idx) - 1, dtype=np.complex128))
    with pytest.raises(TypeError):
        t.apply_reciprocal(k, space=f, values=np.zeros(len(idx), dtype=np.complex64))
    with pytest.raises(sp.InvalidParameterError):
        t.apply_reciprocal(k, space=f, scaling=7)
    # the native null-kernel check (the Python layer never passes one)
    from spfft_amd.ops._lib import lib
    code = lib().spfft_amd_transform_apply_reciprocal(t.handle, int(HOST), None, 0, None, 0)
    from spfft_amd.types import ErrorCode
    assert code == int(ErrorCode.INVALID_PARAMETER)
    # and the transform still works
    want, _ = _oracle(idx, f, k, dims)
    assert max_rel_error(t.apply_reciprocal(k, space=f), want) < TOL64


def _two_ranks(pu, exchange=None, kind="complex"):
    """apply_reciprocal on 2 in-process ranks at (12, 11, 8): each rank passes its slab of
    the field and its part of K."""
    from spfft_amd.parallel import make_distributed, run_ranks
    dims = (12, 11, 8)
    gidx = sphere_indices(*dims, 0.5)
    rng = np.random.default_rng(43)
    f = _field(rng, dims)
    want, wvals = _oracle(gidx, f, _kernel(gidx, dims, kind), dims, full=True)
    return run_ranks(2, _rank_body(pu, dims, gidx, f, want, kind, exchange))


def _rank_body(pu, dims, gidx, f, want, kind, exchange):
    from spfft_amd.parallel import make_distributed

    def body(rank, comm):
        kw = {"exchange_type": exchange} if exchange is not None else {}
        if pu == GPU:
            import torch
            torch.cuda.set_device(0)
        s = make_distributed(comm, dims, gidx, processing_unit=pu, **kw)
        t = s.transform
        k = _kernel(s.indices, dims, kind)
        slab = np.ascontiguousarray(f[s.z_offset:s.z_offset + s.z_length])
        mine = want[s.z_offset:s.z_offset + s.z_length]
        wvals = dense_forward(f, s.indices, dims, scale=True)
        errs = []
        for _ in range(2):
            if pu == GPU:
                import torch
                vals = torch.zeros(len(s.indices), dtype=torch.complex128, device="cuda")
                out = t.apply_reciprocal(torch.as_tensor(k, device="cuda"),
                                         space=torch.as_tensor(slab, device="cuda"), values=vals,
                                         scaling=sp.Scaling.FULL).cpu().numpy()
                vals = vals.cpu().numpy()
            else:
                vals = np.zeros(len(s.indices), dtype=np.complex128)
                out = t.apply_reciprocal(k, space=slab, values=vals, scaling=sp.Scaling.FULL)
            # a rank's slab against the global scale of the result
            errs.append(float(np.max(np.abs(out - mine))) / float(np.max(np.abs(want)))
                        if mine.size else 0.0)
            errs.append(max_rel_error(vals, wvals))
        plan = t.exchange_plan() if pu == GPU else None
        return max(errs), t.reciprocal_fused, plan

    return body


def test_host_apply_reciprocal_two_ranks():
    for err, fused, _ in _two_ranks(HOST):
        assert fused is False
        assert err < TOL64


# -------------------------------------------------------------------------- GPU
def _check_gpu(gpu, dims, idx, kind, r2c=False, single=False, seed=50, fused=True,
               scalings=(True, False)):
    """Twice per scaling against the oracle, space result and values output."""
    import torch
    rng = np.random.default_rng(seed)
    assert len(idx) > 0
    f = _field(rng, dims, r2c, single)
    k = _kernel(idx, dims, kind, single)
    t = _transform(GPU, dims, idx, r2c=r2c, single=single)
    if fused is not None:
        assert t.reciprocal_fused is fused
    df, dk = torch.as_tensor(f, device=gpu), torch.as_tensor(k, device=gpu)
    tol = TOL32 if single else TOL64
    for full in scalings:
        want, wvals = _oracle(idx, f, k, dims, r2c=r2c, full=full)
        for rep in range(2):
            vals = torch.full((len(idx),), -1, dtype=t._prec.torch_complex, device=gpu)
            out = t.apply_reciprocal(dk, space=df, values=vals, scaling=_scaling(full))
            err = max_rel_error(out.cpu().numpy(), want)
            verr = max_rel_error(vals.cpu().numpy(), wvals)
            print(dims, "fp32" if single else "fp64", kind, "full" if full else "none", rep, err,
                  verr)
            assert err < tol
            assert verr < tol
    return t, f, k, df, dk


def _simple_sticks(rng, dims, r2c=False, sticks=0.8):
    return create_value_indices(rng, [1.0], sticks, 1.0, *dims, r2c)[0]


# z length by engine: 16 / 64 FftCT, 60 / 240 FftMR, 11 / 100 run-time; (13, 5) leaves the
# last stick block partial, (3, 2) has fewer sticks than one block
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("nxy", [(13, 5), (3, 2)])
@pytest.mark.parametrize("nz", [16, 64, 60, 240, 11, 100])
def test_gpu_fused_z_lengths(gpu, nz, nxy, centered, kind):
    dims = (nxy[0], nxy[1], nz)
    rng = np.random.default_rng(51)
    idx = _simple_sticks(rng, dims, sticks=1.0 if nxy == (3, 2) else 0.8)
    if centered:
        idx = center_indices(dims, [idx])[0]
    _check_gpu(gpu, dims, idx, kind, scalings=(True,))


# run-time engine with a generic prime pass: 17 (one pass, the result lands in the second
# LDS region), 51 = 3 x 17 (two passes); 67: Bluestein in LDS. At (3, 2) the block has
# fewer sticks than lines: the multiply zeroes the absent lines in the region (or the
# padded Bluestein lines) the inverse FFT reads.
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("nxy", [(13, 5), (3, 2)])
@pytest.mark.parametrize("nz", [17, 51, 67])
def test_gpu_fused_prime_lengths(gpu, nz, nxy, centered, kind):
    dims = (nxy[0], nxy[1], nz)
    rng = np.random.default_rng(52)
    idx = _simple_sticks(rng, dims, sticks=1.0 if nxy == (3, 2) else 0.8)
    if centered:
        idx = center_indices(dims, [idx])[0]
    _check_gpu(gpu, dims, idx, kind)


@pytest.mark.gpu
def test_gpu_fused_fp64_1024(gpu):
    dims = (3, 2, 1024)
    rng = np.random.default_rng(53)
    _check_gpu(gpu, dims, _simple_sticks(rng, dims, sticks=1.0), "complex")


# (5, 3, 512): the forward and backward stages pick different fp32 shapes at N = 512
@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(5, 3, 512), (3, 2, 1024), (6, 10, 240)])
def test_gpu_fused_fp32(gpu, dims):
    rng = np.random.default_rng(54)
    _check_gpu(gpu, dims, _simple_sticks(rng, dims, sticks=1.0), "complex", single=True)
    _check_gpu(gpu, dims, _simple_sticks(rng, dims, sticks=1.0), "real", single=True,
               scalings=(True,))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_gpu_fused_sphere_masks_the_sparse_set(gpu, kind):
    """Partially filled sticks (two z-runs per stick): positions outside the sparse set
    are dropped between the two FFTs."""
    dims = (16, 16, 16)
    _check_gpu(gpu, dims, sphere_indices(*dims, 0.5), kind)


# the (0, 0) stick of an R2C transform: the hermitian fill inside the fused kernel
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("case", ["full", "sphere"])
def test_gpu_fused_r2c_zero_stick(gpu, case, kind):
    rng = np.random.default_rng(55)
    if case == "full":
        dims = (16, 12, 10)
        idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, True)[0]
    else:
        dims = (32, 32, 32)
        idx = sphere_indices(*dims, 0.5, r2c=True)
    assert np.any((idx[:, 0] == 0) & (idx[:, 1] == 0))
    _check_gpu(gpu, dims, idx, kind, r2c=True)


@pytest.mark.gpu
def test_gpu_roll_identity(gpu):
    import torch
    dims = (12, 10, 16)
    rng = np.random.default_rng(56)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    f = _field(rng, dims)
    t = _transform(GPU, dims, idx)
    assert t.reciprocal_fused is True
    dk = torch.as_tensor(_kernel(idx, dims, "complex"), device=gpu)
    want = np.roll(f, (SHIFT[2], SHIFT[1], SHIFT[0]), axis=(0, 1, 2))
    for _ in range(2):
        out = t.apply_reciprocal(dk, space=torch.as_tensor(f, device=gpu), scaling=sp.Scaling.FULL)
        assert max_rel_error(out.cpu().numpy(), want) < TOL64


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_gpu_matches_composition(gpu, kind):
    """Against forward, a torch multiply and backward on the same transform; host
    pointers for K and values; the values output against forward()."""
    import torch
    dims = (13, 5, 64)
    rng = np.random.default_rng(57)
    idx = _simple_sticks(rng, dims)
    t, f, k, df, dk = _check_gpu(gpu, dims, idx, kind)
    for full in (False, True):
        vals = t.forward(space=df, scaling=_scaling(full)).clone()
        composed = t.backward(vals * dk).clone()
        out_vals = torch.zeros_like(vals)
        fused = t.apply_reciprocal(dk, space=df, values=out_vals, scaling=_scaling(full))
        assert max_rel_error(fused.cpu().numpy(), composed.cpu().numpy()) < TOL64
        assert max_rel_error(out_vals.cpu().numpy(), vals.cpu().numpy()) < TOL64
        # host pointers for K and values, host space domain
        hvals = np.zeros(len(idx), dtype=np.complex128)
        hout = t.apply_reciprocal(k, space=f, values=hvals, location=HOST, scaling=_scaling(full))
        assert max_rel_error(hout, composed.cpu().numpy()) < TOL64
        assert max_rel_error(hvals, vals.cpu().numpy()) < TOL64
        # without the values output
        again = t.apply_reciprocal(dk, space=df, scaling=_scaling(full))
        assert max_rel_error(again.cpu().numpy(), composed.cpu().numpy()) < TOL64


def _subprocess_case(case, env):
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], cwd=REPO, env=e,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "CASE OK" in r.stdout, (r.stdout + r.stderr)[-4000:]
    return r.stdout + r.stderr


@pytest.mark.gpu
def test_gpu_run_table_sticks(gpu):
    """Sticks that are not simple: correct either way, and reciprocal_fused tells what the
    plan's SPFFT_LOG line tells."""
    import re
    out = _subprocess_case("runtable", {"SPFFT_LOG": "1"})
    flag = re.search(r"reciprocal_fused (True|False)", out).group(1)
    field = re.search(r"density=\w+ reciprocal=(fused|composed)", out).group(1)
    assert (flag == "True") == (field == "fused"), out[-2000:]


# z lines beyond one workgroup run composed. 5120 is the smallest fp64 z length on the long
# path (one more than the longest line the LDS holds, max_device_fft_length). 2048, the
# smallest long x length, is not long on z: the z stage takes a run-time engine with one line
# per workgroup (needs_long_path keeps that rule to the x and y axes), so by the plan rule
# (simple sticks, z lines of one workgroup) that local grid is fused, and reciprocal_fused
# says so.
@pytest.mark.gpu
@pytest.mark.parametrize("nz,fused", [(2048, True), (5120, False)])
def test_gpu_long_z_falls_back(gpu, nz, fused):
    dims = (3, 5, nz)
    rng = np.random.default_rng(58)
    _check_gpu(gpu, dims, _simple_sticks(rng, dims), "complex", fused=fused)


@pytest.mark.gpu
def test_gpu_stream_order(gpu):
    import torch
    dims = (13, 5, 64)
    rng = np.random.default_rng(59)
    idx = _simple_sticks(rng, dims)
    f = _field(rng, dims)
    k = _kernel(idx, dims, "complex")
    t = _transform(GPU, dims, idx)
    df, dk = torch.as_tensor(f, device=gpu), torch.as_tensor(k, device=gpu)
    t.set_stream(torch.cuda.current_stream(), synchronous=False)
    vals = torch.zeros(len(idx), dtype=torch.complex128, device=gpu)
    out = t.apply_reciprocal(dk, space=df, values=vals)
    doubled, vdoubled = out * 2, vals * 2  # ordered after the call by the stream alone
    torch.cuda.synchronize()
    want, wvals = _oracle(idx, f, k, dims)
    assert max_rel_error(doubled.cpu().numpy(), 2 * want) < TOL64
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
@pytest.mark.parametrize("dims", [(13, 5, 64), (3, 5, 5120)])
def test_gpu_stage_timing_names(gpu, dims):
    """A fused call: forward x+y, exchange, z_reciprocal, then backward exchange, y+x. A
    composed call ((3, 5, 5120): long z): the stages of forward and backward plus multiply."""
    import torch
    rng = np.random.default_rng(60)
    idx = _simple_sticks(rng, dims)
    t = _transform(GPU, dims, idx)
    df = torch.as_tensor(_field(rng, dims), device=gpu)
    dk = torch.as_tensor(_kernel(idx, dims, "real"), device=gpu)
    dirs = _stage_names(t, lambda: t.apply_reciprocal(dk, space=df))
    assert t.reciprocal_fused is (dims[2] == 64)
    if t.reciprocal_fused:
        assert set(dirs["forward"]) == {"x+y", "exchange", "z_reciprocal"}, dirs
        assert set(dirs["backward"]) == {"exchange", "y+x"}, dirs
    else:
        assert set(dirs["forward"]) == {"x+y", "exchange", "z", "multiply"}, dirs
        assert set(dirs["backward"]) == {"z", "exchange", "y+x"}, dirs
    for d in dirs.values():
        for node in d.values():
            assert node["count"] == 3, node


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_gpu_two_ranks(gpu, kind):
    for err, fused, plan in _two_ranks(GPU, sp.ExchangeType.COMPACT_BUFFERED, kind):
        assert isinstance(fused, bool)
        if not plan[2]:  # no peer writes: forward and backward share the stick side
            assert fused
        assert err < TOL64


# The pipelined exchange under apply_reciprocal: the fused z stage runs per stick block,
# after the block's forward messages have arrived and before its backward messages leave.
# Three virtual ranks of one GPU, K plane chunks x I stick blocks forced.
@pytest.mark.gpu
@pytest.mark.parametrize("chunks,blocks,exchange", [
    (1, 1, "COMPACT_BUFFERED"), (2, 2, "COMPACT_BUFFERED"), (1, 2, "COMPACT_BUFFERED"),
    (2, 1, "BUFFERED"), (2, 2, "COMPACT_BUFFERED_FLOAT")])
def test_gpu_virtual_ranks_pipelined(gpu, chunks, blocks, exchange, monkeypatch):
    from spfft_amd.parallel import run_ranks
    dims = (20, 18, 30)
    monkeypatch.setenv("SPFFT_EXCH_CHUNKS", str(chunks))
    monkeypatch.setenv("SPFFT_EXCH_STICK_BLOCKS", str(blocks))
    gidx = sphere_indices(*dims, 0.5)
    rng = np.random.default_rng(61)
    f = _field(rng, dims)
    want, _ = _oracle(gidx, f, _kernel(gidx, dims, "complex"), dims, full=True)
    body = _rank_body(GPU, dims, gidx, f, want, "complex", getattr(sp.ExchangeType, exchange))
    # fp32 exchange buffers: the fp32 bound
    tol = TOL32 if exchange.endswith("FLOAT") else TOL64
    for err, fused, plan in run_ranks(3, body):
        print(exchange, "K x I", plan[:2], "peer writes", plan[2], "fused", fused, err)
        assert isinstance(fused, bool)
        assert plan[:2] == (chunks, blocks), plan
        if not plan[2] and not exchange.endswith("FLOAT"):
            # no peer writes, stick side in the transform's precision: the fused z stage
            # runs per stick block
            assert fused
        assert err < tol


@pytest.mark.gpu
def test_gpu_pipelined_stage_timing_names(gpu, monkeypatch):
    """A fused call under the pipelined exchange (2 plane chunks x 2 stick blocks, three
    virtual ranks): forward x+y, exchange-tail, z_reciprocal, then backward exchange+y+x,
    once per call and rank."""
    import torch
    from spfft_amd.parallel import make_distributed, run_ranks
    dims, P, calls = (20, 18, 30), 3, 3
    monkeypatch.setenv("SPFFT_EXCH_CHUNKS", "2")
    monkeypatch.setenv("SPFFT_EXCH_STICK_BLOCKS", "2")
    gidx = sphere_indices(*dims, 0.5)
    f = _field(np.random.default_rng(65), dims)

    def body(rank, comm):
        torch.cuda.set_device(0)
        s = make_distributed(comm, dims, gidx, processing_unit=GPU,
                             exchange_type=sp.ExchangeType.COMPACT_BUFFERED)
        t = s.transform
        dk = torch.as_tensor(_kernel(s.indices, dims, "real"), device="cuda")
        slab = torch.as_tensor(np.ascontiguousarray(f[s.z_offset:s.z_offset + s.z_length]),
                               device="cuda")
        for _ in range(calls):
            t.apply_reciprocal(dk, space=slab)
        t.synchronize()
        return t.reciprocal_fused, t.exchange_plan()

    sp.timing_reset()
    sp.timing_enable(True)
    try:
        results = run_ranks(P, body)
        tree = sp.timing_json()
    finally:
        sp.timing_enable(False)
    for fused, plan in results:
        assert plan[:3] == (2, 2, False), plan
        assert fused
    gpu_node = [n for n in tree["timings"] if n["identifier"] == "gpu"]
    assert gpu_node, tree
    dirs = {d["identifier"]: {x["identifier"]: x for x in d["sub-timings"]}
            for d in gpu_node[0]["sub-timings"]}
    # (exchange-span: the data plane's own interval next to the stages, not a stage)
    assert set(dirs["forward"]) - {"exchange-span"} == {"x+y", "exchange-tail", "z_reciprocal"}, dirs
    assert set(dirs["backward"]) - {"exchange-span"} == {"exchange+y+x"}, dirs
    for d in dirs.values():
        for name, node in d.items():
            if name != "exchange-span":
                assert node["count"] == calls * P, node


@pytest.mark.gpu
def test_gpu_hartree_potential(gpu):
    import torch
    from spfft_amd.models.planewave import PlaneWaveBasis, PlaneWaveModel
    basis = PlaneWaveBasis(alat=6.0, ecut=4.0)
    model = PlaneWaveModel(basis, num_transforms=1)
    assert model.transforms[0].reciprocal_fused is True
    n0, n1, n2 = basis.fft_dims
    rng = np.random.default_rng(62)
    rho = torch.as_tensor(rng.random((n2, n1, n0)), device=gpu)
    for _ in range(2):
        fused = model.hartree_potential(rho)
        composed = model.hartree_potential(rho, unfused=True)
        assert fused.shape == rho.shape and not fused.is_complex()
        assert max_rel_error(fused.cpu().numpy(), composed.cpu().numpy()) < TOL64
    # and against the dense oracle: K = 4 pi / |G|^2, K(0) = 0
    g2 = basis.g2
    k = np.where(g2 > 0, 4 * np.pi / np.where(g2 > 0, g2, 1.0), 0.0)
    want, _ = _oracle(basis.indices, rho.cpu().numpy().astype(np.complex128), k, basis.fft_dims,
                      full=True)
    assert max_rel_error(fused.cpu().numpy(), want.real) < TOL64


def test_host_hartree_potential():
    from spfft_amd.models.planewave import PlaneWaveBasis, PlaneWaveModel
    basis = PlaneWaveBasis(alat=6.0, ecut=4.0)
    model = PlaneWaveModel(basis, processing_unit=HOST, num_transforms=1)
    n0, n1, n2 = basis.fft_dims
    rho = np.random.default_rng(63).random((n2, n1, n0))
    a, b = model.hartree_potential(rho), model.hartree_potential(rho, unfused=True)
    assert a.dtype == np.float64 and max_rel_error(a, b) < TOL64


# ---------------------------------------------- pinned cases of tools/fuzz_ops.py
# The operator sweep (tests/test_fuzz_ops.py) reaches these by chance; here they always run:
# its case runner on hand-written configurations (two calls against the dense oracle, the
# values output, K and the input slab unchanged), under the sweep's bound of 1e-10. Every
# stick is full (z fill 1.0), so nothing but the exchange decides between the fused and
# the composed z stage. (apply_reciprocal has no fused x stage.)
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
    desc, err, tol, facts = mod.run_case(mod.fixed_case("reciprocal", z_fill=1.0, **choices))
    print(desc, err, facts)
    assert err < tol
    return facts


@pytest.mark.gpu
@pytest.mark.parametrize("dims,sticks,planes", SKEWED)
def test_gpu_unbuffered_skewed_distributions(gpu, dims, sticks, planes):
    """UNBUFFERED (peer writes) on the skewed splits of test_gpu_transform's test of that
    name: forward and backward address a peer-written stick side differently, so the z
    stage runs composed; ranks without sticks pass an empty K and values."""
    for f in _pinned(dims=dims, stick_dist=sticks, plane_dist=planes, exchange="UNBUFFERED"):
        assert f["plan"][2] is True, f
        assert f["reciprocal_fused"] is False, f


@pytest.mark.gpu
@pytest.mark.parametrize("dims,sticks,planes", SKEWED)
def test_gpu_compact_chunks_skewed_distributions(gpu, dims, sticks, planes):
    """The same splits under the pipelined COMPACT_BUFFERED exchange, two plane chunks
    forced: the fused z stage, ranks without sticks launch it over an empty range."""
    for f in _pinned(dims=dims, stick_dist=sticks, plane_dist=planes, chunks=2):
        assert f["plan"][0] == 2 and f["plan"][2] is False, f
        assert f["reciprocal_fused"] is True, f


@pytest.mark.gpu
@pytest.mark.parametrize("dims,zfused", [((16, 2048, 4), True), ((4, 4, 4096), None),
                                         ((2048, 4, 16), True)])
def test_gpu_beside_a_long_axis(gpu, dims, zfused):
    """The z stage beside four-step y passes and beside a long x; a long z itself."""
    (f,) = _pinned(dims=dims)
    if zfused is not None:
        assert f["reciprocal_fused"] is zfused, f


# ------------------------------------------------- cases run in their own process
def _case_runtable():
    dims = (13, 5, 64)
    rng = np.random.default_rng(64)
    idx = create_value_indices(rng, [1.0], 0.8, 0.7, *dims, False)[0]
    for kind in ("real", "complex"):
        t = _check_gpu("cuda", dims, idx, kind, fused=None)[0]
    print("reciprocal_fused", t.reciprocal_fused)


if __name__ == "__main__":
    {"runtable": _case_runtable}[sys.argv[1]]()
    print("CASE OK")
