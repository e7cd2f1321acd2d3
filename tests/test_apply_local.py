"""apply_local: forward(V * backward(values)) in one call, against the dense oracle
dense_forward(dense_backward(idx, vals, dims) * V, idx, dims). Host transforms run the
plain composition; GPU C2C transforms run the fused x apply stage (inverse x FFT, V
multiply, forward x FFT in LDS), which never touches the space domain; R2C and long x
lines fall back to the composition through the space domain.

Bounds: the project's 1e-12 (fp64) and 2e-5 (fp32) on max_rel_error.

Run as a program (python tests/test_apply_local.py CASE) it executes one of the cases
that need their own process, because the library reads the environment switch under
test (SPFFT_INTER_BYTES, SPFFT_BATCH) when a grid or transform is created."""
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


def _rand_vals(rng, n, single=False):
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return v.astype(np.complex64 if single else np.complex128)


def _potential(rng, dims, single=False):
    nx, ny, nz = dims
    return (0.5 + rng.random((nz, ny, nx))).astype(np.float32 if single else np.float64)


def _oracle(idx, vals, v, dims, r2c=False, full=False):
    space = dense_backward(idx, np.asarray(vals).astype(np.complex128), dims, r2c=r2c)
    return dense_forward(space * v.astype(np.float64), idx, dims, r2c=r2c, scale=full)


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


# ------------------------------------------------------------------------- host
@pytest.mark.parametrize("dims,r2c,single", [((11, 12, 13), False, False),
                                             ((16, 32, 64), False, False),
                                             ((12, 10, 14), True, False),
                                             ((32, 32, 32), False, True)])
def test_host_apply_local(dims, r2c, single):
    rng = np.random.default_rng(11)
    nx, ny, nz = dims
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, nx, ny, nz, r2c)[0]
    vals = (_r2c_values(rng, dims, idx) if r2c else _rand_vals(rng, len(idx)))
    vals = vals.astype(np.complex64 if single else np.complex128)
    v = _potential(rng, dims, single)
    t = _transform(HOST, dims, idx, r2c=r2c, single=single)
    assert t.apply_local_fused is False
    tol = TOL32 if single else TOL64
    for full in (False, True):
        out = t.apply_local(vals, v, scaling=sp.Scaling.FULL if full else sp.Scaling.NONE)
        err = max_rel_error(out, _oracle(idx, vals, v, dims, r2c=r2c, full=full))
        print(dims, "r2c" if r2c else "c2c", "full" if full else "none", err)
        assert err < tol


def test_host_apply_local_in_place():
    rng = np.random.default_rng(12)
    dims = (11, 12, 13)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, False)[0]
    vals = _rand_vals(rng, len(idx))
    v = _potential(rng, dims)
    t = _transform(HOST, dims, idx)
    ref = _oracle(idx, vals, v, dims)
    buf = vals.copy()
    out = t.apply_local(buf, v, output=buf)
    assert out is buf
    assert max_rel_error(buf, ref) < TOL64


def test_potential_is_checked():
    rng = np.random.default_rng(13)
    dims = (6, 5, 4)
    idx = create_value_indices(rng, [1.0], 1.0, 1.0, *dims, False)[0]
    vals = _rand_vals(rng, len(idx))
    v = _potential(rng, dims)
    t = _transform(HOST, dims, idx)
    with pytest.raises(sp.InvalidParameterError):
        t.apply_local(vals, None)
    with pytest.raises(ValueError):
        t.apply_local(vals, v.reshape(dims[0], dims[1], dims[2]))
    with pytest.raises(ValueError):
        t.apply_local(vals, v[:-1])
    with pytest.raises(TypeError):
        t.apply_local(vals, v.astype(np.float32))
    with pytest.raises(TypeError):
        t.apply_local(vals, v.astype(np.complex128))
    with pytest.raises(sp.InvalidParameterError):
        sp.multi_transform_apply_local([t], [vals], [None])
    # and the transform still works
    assert max_rel_error(t.apply_local(vals, v), _oracle(idx, vals, v, dims)) < TOL64


def _two_ranks(pu, exchange=None):
    """apply_local on 2 in-process ranks at (12, 11, 8): each rank passes its slab of V."""
    from spfft_amd.parallel import make_distributed, run_ranks
    from spfft_amd.utils.indices import distribute_sticks
    dims = (12, 11, 8)
    gidx = sphere_indices(*dims, 0.5)
    rng = np.random.default_rng(14)
    vals = _rand_vals(rng, len(gidx))
    v = _potential(rng, dims)
    space = dense_backward(gidx, vals, dims) * v
    parts = distribute_sticks(gidx, 2, dims)

    def body(rank, comm):
        kw = {"exchange_type": exchange} if exchange is not None else {}
        if pu == GPU:
            import torch
            torch.cuda.set_device(0)
        s = make_distributed(comm, dims, gidx, processing_unit=pu, **kw)
        start = sum(len(p) for p in parts[:rank])
        mine = np.ascontiguousarray(vals[start:start + len(s.indices)])
        slab = np.ascontiguousarray(v[s.z_offset:s.z_offset + s.z_length])
        want = dense_forward(space, s.indices, dims, scale=True)
        errs = []
        for _ in range(2):
            if pu == GPU:
                import torch
                out = s.transform.apply_local(torch.as_tensor(mine, device="cuda"),
                                              torch.as_tensor(slab, device="cuda"),
                                              scaling=sp.Scaling.FULL).cpu().numpy()
            else:
                out = s.transform.apply_local(mine, slab, scaling=sp.Scaling.FULL)
            errs.append(max_rel_error(out, want))
        return max(errs), s.transform.apply_local_fused

    return run_ranks(2, body)


def test_host_apply_local_two_ranks():
    for err, fused in _two_ranks(HOST):
        assert not fused
        assert err < TOL64


# -------------------------------------------------------------------------- GPU
def _check_fused(gpu, dims, idx, single=False, seed=21):
    """Fused plan: twice against the oracle, and the space domain stays bit-identical."""
    import torch
    rng = np.random.default_rng(seed)
    vals = _rand_vals(rng, len(idx), single)
    v = _potential(rng, dims, single)
    t = _transform(GPU, dims, idx, single=single)
    assert t.apply_local_fused is True
    space = t.space_domain(GPU)
    sentinel = torch.full_like(space, complex(-7.25, 3.5))
    space.copy_(sentinel)
    torch.cuda.synchronize()
    want = _oracle(idx, vals, v, dims)
    dv, dpot = torch.as_tensor(vals, device=gpu), torch.as_tensor(v, device=gpu)
    tol = TOL32 if single else TOL64
    for rep in range(2):
        out = t.apply_local(dv, dpot)
        err = max_rel_error(out.cpu().numpy(), want)
        print(dims, "fp32" if single else "fp64", "rep", rep, err)
        assert err < tol
    assert space.cpu().numpy().tobytes() == sentinel.cpu().numpy().tobytes()
    return t, dv, dpot, want


# x length by engine: 16 / 64 FftCT, 60 / 240 FftMR, 11 / 100 run-time; ny = 13 leaves the
# last y block partial, ny = 3 has fewer rows than one block; some x hold no sticks
@pytest.mark.gpu
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("ny", [13, 3])
@pytest.mark.parametrize("nx", [16, 64, 60, 240, 11, 100])
def test_gpu_fused_c2c(gpu, nx, ny, centered):
    dims = (nx, ny, 5)
    rng = np.random.default_rng(20)
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
    rng = np.random.default_rng(29)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    _check_fused(gpu, dims, idx)


@pytest.mark.gpu
def test_gpu_fused_dense_columns(gpu):
    """Every x holds a column (sphere of radius N/2): the x_dense shortcut."""
    dims = (32, 32, 32)
    _check_fused(gpu, dims, sphere_indices(*dims, 0.5))


# (512, 3, 5): the backward and forward stages pick different fp32 shapes at N = 512
@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(32, 32, 32), (512, 3, 5), (240, 6, 10)])
def test_gpu_fused_fp32(gpu, dims):
    rng = np.random.default_rng(22)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    _check_fused(gpu, dims, idx, single=True)


@pytest.mark.gpu
def test_gpu_matches_unfused_composition(gpu):
    import torch
    dims = (64, 13, 5)
    rng = np.random.default_rng(23)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    t, dv, dpot, want = _check_fused(gpu, dims, idx)
    space = t.backward(dv)
    space.mul_(dpot)
    composed = t.forward()
    assert max_rel_error(composed.cpu().numpy(), want) < TOL64
    assert max_rel_error(t.apply_local(dv, dpot).cpu().numpy(), want) < TOL64
    # host pointers and output == input
    buf = dv.cpu().numpy().copy()
    t.apply_local(buf, dpot.cpu().numpy(), output=buf)
    assert max_rel_error(buf, want) < TOL64
    dbuf = dv.clone()
    t.apply_local(dbuf, dpot, output=dbuf)
    assert max_rel_error(dbuf.cpu().numpy(), want) < TOL64
    assert torch.equal(dbuf, t.apply_local(dv, dpot))


@pytest.mark.gpu
def test_gpu_full_scaling_identity(gpu):
    import torch
    dims = (60, 13, 5)
    rng = np.random.default_rng(24)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    vals = _rand_vals(rng, len(idx))
    t = _transform(GPU, dims, idx)
    ones = torch.ones((dims[2], dims[1], dims[0]), dtype=torch.float64, device=gpu)
    out = t.apply_local(torch.as_tensor(vals, device=gpu), ones, scaling=sp.Scaling.FULL)
    assert max_rel_error(out.cpu().numpy(), vals) < TOL64


# R2C (packed-real x stage) and x lines beyond one workgroup run unfused. 2048 is the
# smallest fp64 x length on the long path: a power of two without a compile-time kernel
# whose run-time engine holds one line per workgroup (needs_long_path, long_fft.hip).
@pytest.mark.gpu
@pytest.mark.parametrize("dims,r2c", [((16, 12, 10), True), ((2048, 3, 5), False)])
def test_gpu_unfused_fallbacks(gpu, dims, r2c):
    import torch
    rng = np.random.default_rng(25)
    idx = create_value_indices(rng, [1.0], 0.8, 0.8, *dims, r2c)[0]
    vals = (_r2c_values(rng, dims, idx) if r2c else _rand_vals(rng, len(idx)))
    vals = vals.astype(np.complex128)
    v = _potential(rng, dims)
    t = _transform(GPU, dims, idx, r2c=r2c)
    assert t.apply_local_fused is False
    want = _oracle(idx, vals, v, dims, r2c=r2c)
    for _ in range(2):
        out = t.apply_local(torch.as_tensor(vals, device=gpu), torch.as_tensor(v, device=gpu))
        assert max_rel_error(out.cpu().numpy(), want) < TOL64


@pytest.mark.gpu
def test_gpu_stream_order(gpu):
    import torch
    dims = (64, 13, 5)
    rng = np.random.default_rng(26)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    vals = _rand_vals(rng, len(idx))
    v = _potential(rng, dims)
    t = _transform(GPU, dims, idx)
    dv, dpot = torch.as_tensor(vals, device=gpu), torch.as_tensor(v, device=gpu)
    t.set_stream(torch.cuda.current_stream(), synchronous=False)
    out = t.apply_local(dv, dpot)
    doubled = out * 2  # ordered after the transform by the stream alone
    torch.cuda.synchronize()
    assert max_rel_error(doubled.cpu().numpy(), 2 * _oracle(idx, vals, v, dims)) < TOL64


@pytest.mark.gpu
def test_gpu_stage_timing_names_the_fused_stage(gpu):
    """GPU stage times of apply_local: backward z, exchange and y+x_apply+y, then forward
    exchange and z, once per call."""
    import torch
    dims = (64, 13, 5)
    rng = np.random.default_rng(30)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    t = _transform(GPU, dims, idx)
    dv = torch.as_tensor(_rand_vals(rng, len(idx)), device=gpu)
    dpot = torch.as_tensor(_potential(rng, dims), device=gpu)
    sp.timing_reset()
    sp.timing_enable(True)
    try:
        for _ in range(3):
            t.apply_local(dv, dpot)
        t.synchronize()
        tree = sp.timing_json()
    finally:
        sp.timing_enable(False)
    gpu_node = [n for n in tree["timings"] if n["identifier"] == "gpu"]
    assert gpu_node, tree
    dirs = {d["identifier"]: {s["identifier"]: s for s in d["sub-timings"]}
            for d in gpu_node[0]["sub-timings"]}
    assert set(dirs["backward"]) == {"z", "exchange", "y+x_apply+y"}, dirs
    assert set(dirs["forward"]) == {"exchange", "z"}, dirs
    for d in dirs.values():
        for node in d.values():
            assert node["count"] == 3, node


@pytest.mark.gpu
def test_gpu_two_ranks(gpu):
    for err, fused in _two_ranks(GPU, sp.ExchangeType.COMPACT_BUFFERED):
        assert fused
        assert err < TOL64


# The pipelined exchange under apply_local: y backward, x apply and y forward of plane
# chunk k start when the chunk has arrived and release it for the forward exchange, and
# the z stages run per stick block. Three virtual ranks of one GPU move their blocks by
# device copies (not peer writes), the own block in place. K plane chunks x I stick
# blocks are forced (the padded BUFFERED layout fits 2 chunks in these grids' buffers, a
# third is refused by the plan); "capped" also caps the intermediate at one full plane, so each
# chunk of 5 planes runs as at least 3 plane ranges.
@pytest.mark.gpu
@pytest.mark.parametrize("chunks,blocks,exchange,capped", [
    (1, 1, "COMPACT_BUFFERED", False), (3, 1, "COMPACT_BUFFERED", False),
    (2, 2, "COMPACT_BUFFERED", False), (1, 2, "COMPACT_BUFFERED", False),
    (2, 1, "BUFFERED", False), (2, 2, "COMPACT_BUFFERED_FLOAT", False),
    (2, 1, "COMPACT_BUFFERED", True), (2, 2, "BUFFERED", True)])
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
    rng = np.random.default_rng(31)
    vals = _rand_vals(rng, len(gidx))
    v = _potential(rng, dims)
    space = dense_backward(gidx, vals, dims) * v
    parts = distribute_sticks(gidx, P, dims)

    def body(rank, comm):
        torch.cuda.set_device(0)
        s = make_distributed(comm, dims, gidx, processing_unit=GPU,
                             exchange_type=getattr(sp.ExchangeType, exchange))
        t = s.transform
        start = sum(len(p) for p in parts[:rank])
        mine = torch.as_tensor(vals[start:start + len(s.indices)], device="cuda")
        slab = torch.as_tensor(np.ascontiguousarray(v[s.z_offset:s.z_offset + s.z_length]),
                               device="cuda")
        want = dense_forward(space, s.indices, dims, scale=True)
        errs = [max_rel_error(t.apply_local(mine, slab, scaling=sp.Scaling.FULL).cpu().numpy(),
                              want) for _ in range(2)]
        return max(errs), t.apply_local_fused, t.exchange_plan(), s.z_length

    # fp32 exchange buffers: the fp32 bound
    tol = TOL32 if exchange.endswith("FLOAT") else TOL64
    for err, fused, plan, planes in run_ranks(P, body):
        print(exchange, "K x I", plan[:2], "peer writes", plan[2], "planes", planes, err)
        assert fused
        assert plan[:3] == (chunks, blocks, False), plan
        assert err < tol


def _subprocess_case(case, env):
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], cwd=REPO, env=e,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "CASE OK" in r.stdout, (r.stdout + r.stderr)[-4000:]
    return r.stdout + r.stderr


@pytest.mark.gpu
def test_gpu_capped_intermediate(gpu):
    """An intermediate capped at two full planes of (16, 16, 12): at least three plane
    ranges (the plan's inter_planes, from its SPFFT_LOG line), the fused stage in place
    in each."""
    import re
    out = _subprocess_case("capped", {"SPFFT_INTER_BYTES": str(2 * 16 * (16 + 8) * 16),
                                      "SPFFT_LOG": "1"})
    assert "fused True" in out
    planes = int(re.search(r"inter_planes=(\d+) apply_local=fused", out).group(1))
    assert -(-12 // planes) >= 3, planes


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["0", "1"])
def test_gpu_multi_transform_apply_local(gpu, batch):
    _subprocess_case("multi", {"SPFFT_BATCH": batch})


# ---------------------------------------------- pinned cases of tools/fuzz_ops.py
# The operator sweep (tests/test_fuzz_ops.py) reaches these by chance; here they always run:
# its case runner on hand-written configurations (two calls against the dense oracle, the
# inputs unchanged, a sentinel-filled space domain bit-identical on a fused plan), under the
# sweep's bound of 1e-10.
SKEWED = [((4, 32, 6), [1, 2, 1], [1, 0, 2]), ((3, 128, 4), [0, 1, 1], [1, 1, 0]),
          ((2, 64, 5), [1, 0], [0, 1])]


def _pinned(host=False, **choices):
    import importlib.util
    if "fuzz_ops" not in sys.modules:
        spec = importlib.util.spec_from_file_location("fuzz_ops",
                                                      os.path.join(REPO, "tools", "fuzz_ops.py"))
        sys.modules["fuzz_ops"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules["fuzz_ops"])
    mod = sys.modules["fuzz_ops"]
    desc, err, tol, facts = mod.run_case(mod.fixed_case("local", **choices), host=host)
    print(desc, err, facts)
    assert err < tol
    return facts


@pytest.mark.gpu
@pytest.mark.parametrize("dims,sticks,planes", SKEWED)
def test_gpu_unbuffered_skewed_distributions(gpu, dims, sticks, planes):
    """UNBUFFERED (peer writes) on the skewed splits of test_gpu_transform's test of that
    name: the y forward stage of the fused call stores through the remote column tables
    while y backward reads the local ones; ranks without planes pass an empty potential."""
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
    """The fused x stage between four-step y passes, and behind a long z."""
    (f,) = _pinned(dims=dims)
    assert f["fused"] is True, f


def test_host_rank_without_planes_passes_no_potential():
    """A rank without local planes has an empty space domain: a null potential is accepted
    there (a zero-element device tensor has a null address), and still refused on a rank
    that holds planes. Found by tools/fuzz_ops.py."""
    from spfft_amd.ops._lib import lib
    from spfft_amd.parallel import run_ranks
    from spfft_amd.types import ErrorCode
    dims, sticks, planes = (2, 64, 5), [1.0, 0.0], [0, 5]
    rng = np.random.default_rng(15)
    parts = create_value_indices(rng, sticks, 0.9, 0.8, *dims, False)
    ms = len(np.unique(parts[0][:, 0].astype(np.int64) * dims[1] + parts[0][:, 1]))
    vals = _rand_vals(rng, len(parts[0]))
    v = _potential(rng, dims)
    want = _oracle(parts[0], vals, v, dims)
    fn = lib().spfft_amd_transform_apply_local

    def body(rank, comm):
        grid = sp.Grid(*dims, ms, HOST, 1, max_local_z_length=5, comm=comm)
        t = grid.create_transform(HOST, sp.TransformType.C2C, *dims, planes[rank], parts[rank])
        mine = vals.copy() if rank == 0 else np.zeros(0, dtype=np.complex128)
        out = np.zeros_like(mine)
        refused = None
        if rank == 1:  # checked before anything collective starts
            refused = fn(t.handle, mine.ctypes.data, None, out.ctypes.data, 0)
        code = fn(t.handle, mine.ctypes.data, None if rank == 0 else v.ctypes.data, out.ctypes.data, 0)
        return code, refused, out

    (code0, _, out0), (code1, refused1, _) = run_ranks(2, body)
    assert code0 == 0 and code1 == 0
    assert refused1 == int(ErrorCode.INVALID_PARAMETER)
    assert max_rel_error(out0, want) < TOL64


# ------------------------------------------------- cases run in their own process
def _case_capped():
    import torch
    dims = (16, 16, 12)
    rng = np.random.default_rng(27)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    vals = _rand_vals(rng, len(idx))
    v = _potential(rng, dims)
    t = _transform(GPU, dims, idx)
    print("fused", t.apply_local_fused)
    want = _oracle(idx, vals, v, dims)
    for _ in range(2):
        out = t.apply_local(torch.as_tensor(vals, device="cuda"), torch.as_tensor(v, device="cuda"))
        err = max_rel_error(out.cpu().numpy(), want)
        print("capped", err)
        assert err < TOL64


def _scope_counts(tree):
    """identifier -> summed call count over the whole timing tree."""
    counts = {}

    def walk(nodes):
        for n in nodes:
            counts[n["identifier"]] = counts.get(n["identifier"], 0) + n["count"]
            walk(n.get("sub-timings", []))

    walk(tree["timings"])
    return counts


def _case_multi():
    """Three identical plans: distinct potentials, then one shared potential, then host
    arrays. With batching on, the device-pointer calls run apply_local_batch (one launch
    per stage; the scope around the x apply launch names the streamed or shared-potential
    kernel variant); with SPFFT_BATCH=0 no call does."""
    import torch
    batching = os.environ.get("SPFFT_BATCH", "1") != "0"
    dims = (32, 16, 8)
    rng = np.random.default_rng(28)
    idx = create_value_indices(rng, [1.0], 0.7, 0.7, *dims, False)[0]
    t0 = _transform(GPU, dims, idx)
    ts = [t0, t0.clone(), t0.clone()]
    vals = [_rand_vals(rng, len(idx)) for _ in ts]
    pots = [_potential(rng, dims) for _ in ts]
    dvals = [torch.as_tensor(x, device="cuda") for x in vals]
    dpots = [torch.as_tensor(x, device="cuda") for x in pots]
    sp.timing_reset()
    sp.timing_enable(True, gpu_stages=False)
    try:
        for rep in range(2):
            outs = sp.multi_transform_apply_local(ts, dvals, dpots)
            for o, x, p in zip(outs, vals, pots):
                err = max_rel_error(o.cpu().numpy(), _oracle(idx, x, p, dims))
                print("distinct", rep, err)
                assert err < TOL64
        outs = sp.multi_transform_apply_local(ts, dvals, [dpots[0]] * 3,
                                              scalings=[sp.Scaling.FULL] * 3)
        for o, x in zip(outs, vals):
            err = max_rel_error(o.cpu().numpy(), _oracle(idx, x, pots[0], dims, full=True))
            print("shared", err)
            assert err < TOL64
        counts = _scope_counts(sp.timing_json())
        # host arrays go through the per-transform path
        outs = sp.multi_transform_apply_local(ts, vals, pots)
        for o, x, p in zip(outs, vals, pots):
            assert max_rel_error(o.cpu().numpy(), _oracle(idx, x, p, dims)) < TOL64
        after_host = _scope_counts(sp.timing_json())
    finally:
        sp.timing_enable(False)
    print("scopes", {k: n for k, n in counts.items() if "apply" in k})
    assert counts.get("multi_apply_local") == 3
    if batching:
        assert counts.get("gpu_apply_local_batch") == 3
        assert counts.get("x_apply_streamed_potential") == 2
        assert counts.get("x_apply_shared_potential") == 1
        assert "gpu_apply_local_xy" not in counts
        # the host-array call added per-transform stages and no batch
        assert after_host.get("gpu_apply_local_batch") == 3
        assert after_host.get("gpu_apply_local_xy") == 3
    else:
        assert "gpu_apply_local_batch" not in counts
        assert counts.get("gpu_apply_local_xy") == 9


if __name__ == "__main__":
    {"capped": _case_capped, "multi": _case_multi}[sys.argv[1]]()
    print("CASE OK")
