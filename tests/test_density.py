"""accumulate_density: rho += w |backward(values)|^2 in one call, against the dense oracle
rho0 + sum_b w_b |dense_backward(idx, vals_b, dims)|^2 in fp64, with a random nonzero rho0
and weights of both signs. Host transforms run the plain composition; GPU C2C transforms
run the fused x density stage (inverse x FFT in LDS, read-modify-write of the workgroup's
rows of rho), which never touches the space domain; R2C and long x lines run backward and
one pass over the space domain. Every case runs twice, the second call on top of the
first result.

Bounds: the project's 1e-12 (fp64) and 2e-5 (fp32) on max_rel_error.

Run as a program (python tests/test_density.py CASE) it executes one of the cases that
need their own process, because the library reads the environment switch under test
(SPFFT_INTER_BYTES, SPFFT_BATCH) when a grid or transform is created."""
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
WEIGHTS = (0.75, -1.25)  # of the first and of the second call


def _rand_vals(rng, n, single=False):
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return v.astype(np.complex64 if single else np.complex128)


def _rho0(rng, dims, single=False):
    nx, ny, nz = dims
    return (rng.standard_normal((nz, ny, nx)) * 3).astype(np.float32 if single else np.float64)


def _mod2(idx, vals, dims, r2c=False):
    """|backward(values)|^2 in fp64 ([z][y][x])."""
    s = dense_backward(idx, np.asarray(vals).astype(np.complex128), dims, r2c=r2c)
    return s.real ** 2 + s.imag ** 2


def _transform(pu, dims, idx, r2c=False, single=False):
    nx, ny, nz = dims
    G = sp.GridFloat if single else sp.Grid
    grid = G(nx, ny, nz, nx * ny, pu, 1)
    return grid.create_transform(pu, sp.TransformType.R2C if r2c else sp.TransformType.C2C,
                                 nx, ny, nz, nz, idx)


def _r2c_values(rng, dims, idx):
    """Frequency values of a real field (hermitian-consistent input of the C2R stage)."""
    nx, ny, nz = dims
    return dense_forward(rng.standard_normal((nz, ny, nx)), idx, dims, r2c=True, scale=True)


def _twice(call, rho0, mod2, tol, to_numpy=np.asarray, label=""):
    """call(weight) accumulates into the array that starts as rho0: two calls, each result
    against the oracle."""
    want = rho0.astype(np.float64)
    for rep, w in enumerate(WEIGHTS):
        got = call(w)
        want = want + w * mod2
        err = max_rel_error(to_numpy(got).astype(np.float64), want)
        print(label, "rep", rep, err)
        assert err < tol
    return want


# ------------------------------------------------------------------------- host
@pytest.mark.parametrize("dims,r2c,single", [((11, 12, 13), False, False),
                                             ((16, 32, 64), False, False),
                                             ((12, 10, 14), True, False),
                                             ((32, 32, 32), False, True)])
def test_host_density(dims, r2c, single):
    rng = np.random.default_rng(41)
    nx, ny, nz = dims
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, nx, ny, nz, r2c)[0]
    vals = (_r2c_values(rng, dims, idx) if r2c else _rand_vals(rng, len(idx)))
    vals = vals.astype(np.complex64 if single else np.complex128)
    t = _transform(HOST, dims, idx, r2c=r2c, single=single)
    assert t.density_fused is False
    rho0 = _rho0(rng, dims, single)
    rho = rho0.copy()
    keep = vals.copy()

    def call(w):
        out = t.accumulate_density(vals, w, rho)
        assert out is rho
        return rho

    _twice(call, rho0, _mod2(idx, vals, dims, r2c=r2c), TOL32 if single else TOL64, label=dims)
    assert vals.tobytes() == keep.tobytes()  # the values are not modified


def test_density_argument_is_checked():
    rng = np.random.default_rng(43)
    dims = (6, 5, 4)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    vals = _rand_vals(rng, len(idx))
    t = _transform(HOST, dims, idx)
    rho0 = _rho0(rng, dims)
    rho = rho0.copy()
    with pytest.raises(sp.InvalidParameterError):
        t.accumulate_density(vals, 1.0, None)
    with pytest.raises(ValueError):
        t.accumulate_density(vals, 1.0, rho.reshape(dims[0], dims[1], dims[2]))
    with pytest.raises(ValueError):
        t.accumulate_density(vals, 1.0, rho[:-1])
    with pytest.raises(ValueError):  # not contiguous: never a silent copy
        t.accumulate_density(vals, 1.0, np.zeros((dims[2], dims[1], 2 * dims[0]))[:, :, ::2])
    with pytest.raises(TypeError):
        t.accumulate_density(vals, 1.0, rho.astype(np.float32))
    with pytest.raises(TypeError):
        t.accumulate_density(vals, 1.0, rho.astype(np.complex128))
    with pytest.raises(sp.InvalidParameterError):
        sp.multi_transform_accumulate_density([t], [vals], [1.0], None)
    with pytest.raises(ValueError):
        sp.multi_transform_accumulate_density([t], [vals], [1.0, 2.0], rho)
    assert rho.tobytes() == rho0.tobytes()
    # and the transform still works
    _twice(lambda w: t.accumulate_density(vals, w, rho), rho0, _mod2(idx, vals, dims), TOL64)
    # the multi call on the host: two transforms into one rho
    t2 = t.clone()
    vals2 = _rand_vals(rng, len(idx))
    rho = rho0.copy()
    sp.multi_transform_accumulate_density([t, t2], [vals, vals2], [0.5, -2.0], rho)
    want = rho0 + 0.5 * _mod2(idx, vals, dims) - 2.0 * _mod2(idx, vals2, dims)
    assert max_rel_error(rho, want) < TOL64


def _two_ranks(pu, exchange=None):
    """accumulate_density on 2 in-process ranks at (12, 11, 8): each rank passes its slab."""
    from spfft_amd.parallel import make_distributed, run_ranks
    from spfft_amd.utils.indices import distribute_sticks
    dims = (12, 11, 8)
    gidx = sphere_indices(*dims, 0.5)
    rng = np.random.default_rng(44)
    vals = _rand_vals(rng, len(gidx))
    rho0 = _rho0(rng, dims)
    mod2 = _mod2(gidx, vals, dims)
    parts = distribute_sticks(gidx, 2, dims)

    def body(rank, comm):
        kw = {"exchange_type": exchange} if exchange is not None else {}
        if pu == GPU:
            import torch
            torch.cuda.set_device(0)
        s = make_distributed(comm, dims, gidx, processing_unit=pu, **kw)
        start = sum(len(p) for p in parts[:rank])
        mine = np.ascontiguousarray(vals[start:start + len(s.indices)])
        z = slice(s.z_offset, s.z_offset + s.z_length)
        want = rho0[z].copy()
        errs = []
        if pu == GPU:
            import torch
            mine = torch.as_tensor(mine, device="cuda")
            rho = torch.as_tensor(np.ascontiguousarray(rho0[z]), device="cuda")
        else:
            rho = np.ascontiguousarray(rho0[z])
        for w in WEIGHTS:
            s.transform.accumulate_density(mine, w, rho)
            want = want + w * mod2[z]
            errs.append(max_rel_error(rho.cpu().numpy() if pu == GPU else rho, want))
        return max(errs), s.transform.density_fused

    return run_ranks(2, body)


def test_host_density_two_ranks():
    for err, fused in _two_ranks(HOST):
        assert not fused
        assert err < TOL64


def _model_case(pu):
    from spfft_amd.models import PlaneWaveBasis, PlaneWaveModel
    basis = PlaneWaveBasis(alat=6.0, ecut=4.0)
    model = PlaneWaveModel(basis, processing_unit=pu, num_transforms=3)
    rng = np.random.default_rng(45)
    psi = [_rand_vals(rng, basis.num_pw) for _ in range(5)]
    weights = [2.0, 1.5, -0.5, 1.0, 0.25]
    if pu == GPU:
        import torch
        psi = [torch.as_tensor(p, device="cuda") for p in psi]
    rho = model.density(psi, weights)
    ref = model.density(psi, weights, unfused=True)
    nx, ny, nz = basis.fft_dims
    assert tuple(rho.shape) == (nz, ny, nx)
    if pu == GPU:
        assert rho.is_cuda and rho.dtype == torch.float64
        rho, ref = rho.cpu().numpy(), ref.cpu().numpy()
    else:
        assert isinstance(rho, np.ndarray) and rho.dtype == np.float64
    assert max_rel_error(rho, ref) < TOL64


def test_model_density_host():
    _model_case(HOST)


# -------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_model_density_gpu(gpu):
    _model_case(GPU)


def _check_fused(gpu, dims, idx, single=False, seed=51):
    """Fused plan: twice against the oracle, and the space domain stays bit-identical."""
    import torch
    rng = np.random.default_rng(seed)
    vals = _rand_vals(rng, len(idx), single)
    rho0 = _rho0(rng, dims, single)
    t = _transform(GPU, dims, idx, single=single)
    assert t.density_fused is True
    space = t.space_domain(GPU)
    sentinel = torch.full_like(space, complex(-7.25, 3.5))
    space.copy_(sentinel)
    torch.cuda.synchronize()
    mod2 = _mod2(idx, vals, dims)
    dv, drho = torch.as_tensor(vals, device=gpu), torch.as_tensor(rho0, device=gpu)

    def call(w):
        assert t.accumulate_density(dv, w, drho) is drho
        return drho

    want = _twice(call, rho0, mod2, TOL32 if single else TOL64, lambda x: x.cpu().numpy(),
                  label=(dims, "fp32" if single else "fp64"))
    assert space.cpu().numpy().tobytes() == sentinel.cpu().numpy().tobytes()
    assert dv.cpu().numpy().tobytes() == vals.tobytes()
    return t, dv, vals, rho0, mod2, want


# x length by engine: 16 / 64 FftCT, 60 / 240 FftMR, 11 / 100 run-time; ny = 13 leaves the
# last y block partial, ny = 3 has fewer rows than one block; some x hold no sticks
@pytest.mark.gpu
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("ny", [13, 3])
@pytest.mark.parametrize("nx", [16, 64, 60, 240, 11, 100])
def test_gpu_fused_c2c(gpu, nx, ny, centered):
    dims = (nx, ny, 5)
    rng = np.random.default_rng(50)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, nx, ny, 5, False)[0]
    if centered:
        idx = center_indices(dims, [idx])[0]
    _check_fused(gpu, dims, idx)


# run-time engine with a generic prime pass: 17 (one pass, the result lands in the second
# LDS region), 51 = 3 x 17 (two passes); 67: Bluestein in LDS
@pytest.mark.gpu
@pytest.mark.parametrize("nx", [17, 51, 67])
def test_gpu_fused_prime_lengths(gpu, nx):
    dims = (nx, 13, 5)
    rng = np.random.default_rng(59)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    _check_fused(gpu, dims, idx)


@pytest.mark.gpu
def test_gpu_fused_dense_columns(gpu):
    """Every x holds a column (sphere of radius N/2): the x_dense shortcut."""
    dims = (32, 32, 32)
    _check_fused(gpu, dims, sphere_indices(*dims, 0.5))


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(32, 32, 32), (512, 3, 5), (240, 6, 10)])
def test_gpu_fused_fp32(gpu, dims):
    rng = np.random.default_rng(52)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    _check_fused(gpu, dims, idx, single=True)


@pytest.mark.gpu
def test_gpu_fused_matches_composed_and_host_pointer(gpu):
    import torch
    dims = (64, 13, 5)
    rng = np.random.default_rng(53)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    t, dv, vals, rho0, mod2, _ = _check_fused(gpu, dims, idx)
    w = 1.5
    want = rho0 + w * mod2
    fused = t.accumulate_density(dv, w, torch.as_tensor(rho0, device=gpu))
    s = t.backward(dv)
    composed = torch.as_tensor(rho0, device=gpu) + w * (s.real ** 2 + s.imag ** 2)
    assert max_rel_error(composed.cpu().numpy(), want) < TOL64
    assert max_rel_error(fused.cpu().numpy(), want) < TOL64
    assert max_rel_error(fused.cpu().numpy(), composed.cpu().numpy()) < TOL64
    # a host rho is staged through a device buffer: same kernels, same bits
    host = rho0.copy()
    assert t.accumulate_density(vals, w, host) is host
    assert max_rel_error(host, want) < TOL64
    assert host.tobytes() == fused.cpu().numpy().tobytes()


# R2C (packed-real x stage) and x lines beyond one workgroup run composed. 2048 is the
# smallest fp64 x length on the long path (see tests/test_apply_local.py).
@pytest.mark.gpu
@pytest.mark.parametrize("dims,r2c", [((16, 12, 10), True), ((2048, 3, 5), False)])
def test_gpu_composed_fallbacks(gpu, dims, r2c):
    import torch
    rng = np.random.default_rng(55)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, r2c)[0]
    vals = (_r2c_values(rng, dims, idx) if r2c else _rand_vals(rng, len(idx)))
    vals = vals.astype(np.complex128)
    t = _transform(GPU, dims, idx, r2c=r2c)
    assert t.density_fused is False
    rho0 = _rho0(rng, dims)
    dv, drho = torch.as_tensor(vals, device=gpu), torch.as_tensor(rho0, device=gpu)
    _twice(lambda w: t.accumulate_density(dv, w, drho), rho0, _mod2(idx, vals, dims, r2c=r2c),
           TOL64, lambda x: x.cpu().numpy(), label=dims)


@pytest.mark.gpu
def test_gpu_stream_order(gpu):
    import torch
    dims = (64, 13, 5)
    rng = np.random.default_rng(56)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    vals = _rand_vals(rng, len(idx))
    rho0 = _rho0(rng, dims)
    t = _transform(GPU, dims, idx)
    dv, drho = torch.as_tensor(vals, device=gpu), torch.as_tensor(rho0, device=gpu)
    t.set_stream(torch.cuda.current_stream(), synchronous=False)
    mod2 = _mod2(idx, vals, dims)
    want = rho0.astype(np.float64)
    for w in WEIGHTS:
        out = t.accumulate_density(dv, w, drho)
        doubled = out * 2  # ordered after the call by the stream alone
        torch.cuda.synchronize()
        want = want + w * mod2
        assert max_rel_error(doubled.cpu().numpy(), 2 * want) < TOL64


@pytest.mark.gpu
def test_gpu_stage_timing_names_the_fused_stage(gpu):
    """GPU stage times of accumulate_density: backward z, exchange and y+x_density, once
    per call, and no forward direction."""
    import torch
    dims = (64, 13, 5)
    rng = np.random.default_rng(60)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    t = _transform(GPU, dims, idx)
    dv = torch.as_tensor(_rand_vals(rng, len(idx)), device=gpu)
    drho = torch.as_tensor(_rho0(rng, dims), device=gpu)
    sp.timing_reset()
    sp.timing_enable(True)
    try:
        for _ in range(3):
            t.accumulate_density(dv, 0.5, drho)
        t.synchronize()
        tree = sp.timing_json()
    finally:
        sp.timing_enable(False)
    gpu_node = [n for n in tree["timings"] if n["identifier"] == "gpu"]
    assert gpu_node, tree
    dirs = {d["identifier"]: {s["identifier"]: s for s in d["sub-timings"]}
            for d in gpu_node[0]["sub-timings"]}
    assert set(dirs) == {"backward"}, dirs
    assert set(dirs["backward"]) == {"z", "exchange", "y+x_density"}, dirs
    for node in dirs["backward"].values():
        assert node["count"] == 3, node


@pytest.mark.gpu
def test_gpu_two_ranks(gpu):
    for err, fused in _two_ranks(GPU, sp.ExchangeType.COMPACT_BUFFERED):
        assert fused
        assert err < TOL64


# The pipelined exchange under accumulate_density: y backward and x density of plane chunk
# k start when the chunk has arrived. Three virtual ranks of one GPU, K plane chunks x I
# stick blocks forced; "capped" also caps the intermediate at one full plane, so each chunk
# of 5 planes runs as at least 3 plane ranges.
@pytest.mark.gpu
@pytest.mark.parametrize("chunks,blocks,exchange,capped", [
    (1, 1, "COMPACT_BUFFERED", False), (3, 1, "COMPACT_BUFFERED", False),
    (2, 2, "COMPACT_BUFFERED", False), (2, 1, "BUFFERED", False),
    (2, 1, "COMPACT_BUFFERED", True)])
def test_gpu_virtual_ranks_pipelined(gpu, chunks, blocks, exchange, capped, monkeypatch):
    import torch
    from spfft_amd.parallel import make_distributed, run_ranks
    from spfft_amd.utils.indices import distribute_sticks
    dims = (20, 18, 30)
    nx, ny, nz = dims
    P = 3
    monkeypatch.setenv("SPFFT_EXCH_CHUNKS", str(chunks))
    monkeypatch.setenv("SPFFT_EXCH_STICK_BLOCKS", str(blocks))
    if capped:
        monkeypatch.setenv("SPFFT_INTER_BYTES", str(nx * (ny + 8) * 16))
    gidx = sphere_indices(*dims, 0.5)
    rng = np.random.default_rng(61)
    vals = _rand_vals(rng, len(gidx))
    rho0 = _rho0(rng, dims)
    mod2 = _mod2(gidx, vals, dims)
    parts = distribute_sticks(gidx, P, dims)

    def body(rank, comm):
        torch.cuda.set_device(0)
        s = make_distributed(comm, dims, gidx, processing_unit=GPU,
                             exchange_type=getattr(sp.ExchangeType, exchange))
        t = s.transform
        start = sum(len(p) for p in parts[:rank])
        mine = torch.as_tensor(vals[start:start + len(s.indices)], device="cuda")
        z = slice(s.z_offset, s.z_offset + s.z_length)
        rho = torch.as_tensor(np.ascontiguousarray(rho0[z]), device="cuda")
        want = rho0[z].copy()
        errs = []
        for w in WEIGHTS:
            t.accumulate_density(mine, w, rho)
            want = want + w * mod2[z]
            errs.append(max_rel_error(rho.cpu().numpy(), want))
        return max(errs), t.density_fused, t.exchange_plan(), s.z_length

    for err, fused, plan, planes in run_ranks(P, body):
        print(exchange, "K x I", plan[:2], "peer writes", plan[2], "planes", planes, err)
        assert fused
        assert plan[:3] == (chunks, blocks, False), plan
        assert err < TOL64


def _subprocess_case(case, env):
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], cwd=REPO, env=e,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "CASE OK" in r.stdout, (r.stdout + r.stderr)[-4000:]
    return r.stdout + r.stderr


@pytest.mark.gpu
def test_gpu_capped_intermediate(gpu):
    """An intermediate capped at two full planes of (16, 16, 12): at least three plane
    ranges (the plan's inter_planes, from its SPFFT_LOG line), each with its own y backward
    and x density launch."""
    import re
    out = _subprocess_case("capped", {"SPFFT_INTER_BYTES": str(2 * 16 * (16 + 8) * 16),
                                      "SPFFT_LOG": "1"})
    assert "fused True" in out
    planes = int(re.search(r"inter_planes=(\d+) apply_local=fused density=fused", out).group(1))
    assert -(-12 // planes) >= 3, planes


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["0", "1"])
def test_gpu_multi_transform_density(gpu, batch):
    _subprocess_case("multi", {"SPFFT_BATCH": batch})


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["0", "1"])
def test_gpu_multi_transform_density_three_streams(gpu, batch):
    _subprocess_case("streams", {"SPFFT_BATCH": batch})


# Batches in process (batching is on by default). ny = 35 gives full row blocks, where a
# compile-time engine sums the bands in registers, and a partial last block, where the bands
# update rho one after another; nx = 100 is a run-time engine; fp32 nx = 1024 is the engine
# whose batches run one single-band x density launch per band (DensityBandLoop)
@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,single", [(64, 35, False), (64, 35, True), (100, 35, False),
                                          (1024, 3, True)])
def test_gpu_multi_transform_density_batched(gpu, nx, ny, single):
    import torch
    dims = (nx, ny, 2)
    rng = np.random.default_rng(63)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    t0 = _transform(GPU, dims, idx, single=single)
    ts = [t0, t0.clone(), t0.clone()]
    vals = [_rand_vals(rng, len(idx), single=single) for _ in ts]
    weights = [1.5, -0.5, 0.25]
    rho0 = _rho0(rng, dims, single=single)
    mod2 = sum(w * _mod2(idx, x, dims) for w, x in zip(weights, vals))
    dvals = [torch.as_tensor(x, device=gpu) for x in vals]
    drho = torch.as_tensor(rho0, device=gpu)
    want = rho0.astype(np.float64)
    for rep in range(2):
        sp.multi_transform_accumulate_density(ts, dvals, weights, drho)
        want = want + mod2
        err = max_rel_error(drho.cpu().numpy().astype(np.float64), want)
        print(dims, "fp32" if single else "fp64", "multi rep", rep, err)
        assert err < (TOL32 if single else TOL64)


# ---------------------------------------------- pinned cases of tools/fuzz_ops.py
# The operator sweep (tests/test_fuzz_ops.py) reaches these by chance; here they always run:
# its case runner on hand-written configurations (two calls, the whole rho and rho minus its
# start against the dense oracle, the values unchanged, a sentinel-filled space domain
# bit-identical on a fused plan), under the sweep's bound of 1e-10.
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
    desc, err, tol, facts = mod.run_case(mod.fixed_case("density", **choices))
    print(desc, err, facts)
    assert err < tol
    return facts


@pytest.mark.gpu
@pytest.mark.parametrize("dims,sticks,planes", SKEWED)
def test_gpu_unbuffered_skewed_distributions(gpu, dims, sticks, planes):
    """UNBUFFERED (peer writes) on the skewed splits of test_gpu_transform's test of that
    name: the fused x density stage on a peer-written slab side; ranks without planes pass
    an empty rho, ranks without sticks no values."""
    for f in _pinned(dims=dims, stick_dist=sticks, plane_dist=planes, exchange="UNBUFFERED"):
        assert f["plan"][2] is True, f
        assert f["fused"] is True and f["reciprocal_fused"] is False, f


@pytest.mark.gpu
@pytest.mark.parametrize("dims,sticks,planes", SKEWED)
def test_gpu_compact_chunks_skewed_distributions(gpu, dims, sticks, planes):
    """The same splits under the pipelined COMPACT_BUFFERED exchange, two plane chunks
    forced: ranks with fewer planes than chunks run empty chunks."""
    for f in _pinned(dims=dims, stick_dist=sticks, plane_dist=planes, chunks=2):
        assert f["plan"][0] == 2 and f["plan"][2] is False, f
        assert f["fused"] is True, f


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(16, 2048, 4), (4, 4, 4096)])
def test_gpu_fused_beside_a_long_axis(gpu, dims):
    """The fused x stage after a four-step y pass, and behind a long z."""
    (f,) = _pinned(dims=dims)
    assert f["fused"] is True, f


# ------------------------------------------------- cases run in their own process
def _case_capped():
    import torch
    dims = (16, 16, 12)
    rng = np.random.default_rng(57)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    vals = _rand_vals(rng, len(idx))
    rho0 = _rho0(rng, dims)
    t = _transform(GPU, dims, idx)
    print("fused", t.density_fused)
    dv, drho = torch.as_tensor(vals, device="cuda"), torch.as_tensor(rho0, device="cuda")
    _twice(lambda w: t.accumulate_density(dv, w, drho), rho0, _mod2(idx, vals, dims), TOL64,
           lambda x: x.cpu().numpy(), label="capped")


def _scope_counts(tree):
    """identifier -> summed call count over the whole timing tree."""
    counts = {}

    def walk(nodes):
        for n in nodes:
            counts[n["identifier"]] = counts.get(n["identifier"], 0) + n["count"]
            walk(n.get("sub-timings", []))

    walk(tree["timings"])
    return counts


def _ten(seed):
    """A transform plus 9 clones at (32, 16, 8), their values, weights of both signs, rho0
    and the oracle of one call."""
    dims = (32, 16, 8)
    rng = np.random.default_rng(seed)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    t0 = _transform(GPU, dims, idx)
    ts = [t0] + [t0.clone() for _ in range(9)]
    vals = [_rand_vals(rng, len(idx)) for _ in ts]
    weights = [(-1) ** b * (0.5 + 0.25 * b) for b in range(len(ts))]
    rho0 = _rho0(rng, dims)
    want = rho0.astype(np.float64)
    for x, w in zip(vals, weights):
        want = want + w * _mod2(idx, x, dims)
    return ts, vals, weights, rho0, want


def _case_multi():
    """Ten identical plans into one rho: with batching on, the call runs two batches
    (8 + 2 members, in order) and no per-transform density stage; with SPFFT_BATCH=0 ten
    per-transform stages, ordered by events. The same call from the same rho0 gives the
    same bits, and a second call accumulates on top of the first."""
    import torch
    batching = os.environ.get("SPFFT_BATCH", "1") != "0"
    ts, vals, weights, rho0, want = _ten(58)
    dvals = [torch.as_tensor(x, device="cuda") for x in vals]
    sp.timing_reset()
    sp.timing_enable(True, gpu_stages=False)
    try:
        drho = torch.as_tensor(rho0, device="cuda")
        assert sp.multi_transform_accumulate_density(ts, dvals, weights, drho) is drho
        counts = _scope_counts(sp.timing_json())
    finally:
        sp.timing_enable(False)
    first = drho.cpu().numpy().copy()
    err = max_rel_error(first, want)
    print("multi", err)
    assert err < TOL64
    print("scopes", {k: n for k, n in counts.items() if "density" in k})
    assert counts.get("multi_accumulate_density") == 1
    if batching:
        assert counts.get("gpu_accumulate_density_batch") == 2
        assert "gpu_accumulate_density_xy" not in counts
    else:
        assert "gpu_accumulate_density_batch" not in counts
        assert counts.get("gpu_accumulate_density_xy") == 10
    # on top of the first result
    sp.multi_transform_accumulate_density(ts, dvals, weights, drho)
    err = max_rel_error(drho.cpu().numpy(), 2 * want - rho0)
    print("multi second", err)
    assert err < TOL64
    # the same call from the same rho0: the same bits
    for _ in range(2):
        again = torch.as_tensor(rho0, device="cuda")
        sp.multi_transform_accumulate_density(ts, dvals, weights, again)
        assert again.cpu().numpy().tobytes() == first.tobytes()
    # a host rho goes through the per-transform path
    host = rho0.copy()
    sp.multi_transform_accumulate_density(ts, vals, weights, host)
    assert max_rel_error(host, want) < TOL64


def _case_streams():
    """The clones on three distinct torch streams (asynchronous): the density stages of
    different streams are ordered by events, the result meets the oracle and two runs
    agree bit for bit."""
    import torch
    ts, vals, weights, rho0, want = _ten(62)
    dvals = [torch.as_tensor(x, device="cuda") for x in vals]
    streams = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    for i, t in enumerate(ts):
        t.set_stream(streams[i % 3], synchronous=False)
    results = []
    for _ in range(2):
        drho = torch.as_tensor(rho0, device="cuda")
        torch.cuda.synchronize()
        sp.multi_transform_accumulate_density(ts, dvals, weights, drho)
        torch.cuda.synchronize()
        results.append(drho.cpu().numpy().copy())
        err = max_rel_error(results[-1], want)
        print("streams", err)
        assert err < TOL64
    assert results[0].tobytes() == results[1].tobytes()


if __name__ == "__main__":
    {"capped": _case_capped, "multi": _case_multi, "streams": _case_streams}[sys.argv[1]]()
    print("CASE OK")
