"""apply_local and accumulate_density on R2C transforms whose half-length dimX / 2 has a
compile-time engine: the fused packed-real x stages (C2R pre-pass, inverse half-length FFT,
the pointwise step on the rows s[2m] + i s[2m+1] in LDS and, for the operator, forward
half-length FFT and R2C post pass), which never touch the real space domain. Odd dimX,
run-time half-lengths, SPFFT_R2C_PACKED=0 and SPFFT_R2C_FUSE=0 stay composed.

Oracle: dense_backward / dense_forward with r2c=True on hermitian-consistent values (the
frequency values of a real field). Bounds: the project's 1e-12 (fp64) and 2e-5 (fp32) on
max_rel_error; density weights (0.75, -1.25) over two calls.

Index sets: create_value_indices(rng, [1.0], 0.7, 0.8, ..., True) with seeds chosen (from the
indices alone) so that every column 0..h holds sticks, the Nyquist column included; the
assertion is made with numpy in every case. (1024, 3, 2) is the exception: with three rows a
column is empty with probability 0.027, so no seed fills all 513 columns; there the Nyquist
column and column 0 are asserted to hold sticks and the empty columns run the xCol = -1
branches. The sphere sets leave the Nyquist column and further columns empty.

The library reads its environment switches when a grid or transform is created, so the
tests set them around the creation only."""
import os
import re
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
SENTINEL = -7.25

# dims, fp32, seed of the index set. (32, 13, 5): smallest compile-time half-length, partial
# row block; (64, 35, 3): full blocks and a partial one; half-lengths 48 and 100 are
# mixed-radix engines; 512 is the largest half-length
SHAPES = [((32, 13, 5), False, 3), ((64, 35, 3), False, 1), ((96, 12, 4), False, 1),
          ((200, 7, 3), False, 1), ((128, 13, 3), True, 1), ((1024, 3, 2), False, 1),
          ((1024, 3, 2), True, 1)]


def _tol(single):
    return TOL32 if single else TOL64


def _columns(idx, dims):
    """x columns (storage order) that hold sticks."""
    x = np.asarray(idx)[:, 0].astype(np.int64)
    return set(np.where(x < 0, x + dims[0], x).tolist())


def _random_indices(dims, seed):
    idx = create_value_indices(np.random.default_rng(seed), [1.0], 0.7, 0.8, *dims, True)[0]
    cols, h = _columns(idx, dims), dims[0] // 2
    if dims[0] == 1024:
        assert 0 in cols and h in cols, "column 0 and the Nyquist column must hold sticks"
        assert len(cols) < h + 1  # three rows: some columns are empty
    else:
        assert cols == set(range(h + 1)), sorted(set(range(h + 1)) - cols)
    return idx


def _sphere(centred):
    """Sphere of radius 0.3 in (64, 20, 6): columns 0..19 hold sticks, 20..32 (the Nyquist
    column among them) hold none."""
    dims = (64, 20, 6)
    idx = sphere_indices(*dims, 0.3, r2c=True)
    if centred:
        idx = center_indices(dims, [idx])[0]
    cols = _columns(idx, dims)
    assert dims[0] // 2 not in cols and cols == set(range(max(cols) + 1)) and max(cols) < 24
    return dims, idx


def _values(rng, dims, idx, single=False):
    """Frequency values of a real field (hermitian-consistent input of the C2R stage)."""
    nx, ny, nz = dims
    v = dense_forward(rng.standard_normal((nz, ny, nx)), idx, dims, r2c=True, scale=True)
    return v.astype(np.complex64 if single else np.complex128)


def _potential(rng, dims, single=False):
    nx, ny, nz = dims
    return (0.5 + rng.random((nz, ny, nx))).astype(np.float32 if single else np.float64)


def _rho0(rng, dims, single=False):
    nx, ny, nz = dims
    return (rng.standard_normal((nz, ny, nx)) * 3).astype(np.float32 if single else np.float64)


def _oracle(idx, vals, v, dims, full=False):
    space = dense_backward(idx, np.asarray(vals).astype(np.complex128), dims, r2c=True)
    return dense_forward(space * v.astype(np.float64), idx, dims, r2c=True, scale=full)


def _mod2(idx, vals, dims):
    s = dense_backward(idx, np.asarray(vals).astype(np.complex128), dims, r2c=True)
    return s.real ** 2 + s.imag ** 2


def _transform(pu, dims, idx, single=False, r2c=True, env=None):
    """A transform on its own grid, created under the environment `env`."""
    nx, ny, nz = dims
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        G = sp.GridFloat if single else sp.Grid
        grid = G(nx, ny, nz, nx * ny, pu, 1)
        return grid.create_transform(pu, sp.TransformType.R2C if r2c else sp.TransformType.C2C,
                                     nx, ny, nz, nz, idx)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _fill_space(t):
    """Fills the (real) space domain with a sentinel; returns the check that it is unchanged."""
    import torch
    space = t.space_domain(GPU)
    space.fill_(SENTINEL)
    torch.cuda.synchronize()
    before = space.cpu().numpy().tobytes()
    return lambda: space.cpu().numpy().tobytes() == before


def _check_operator(gpu, t, dims, idx, single, seed=71):
    """Both scalings, each call twice, against the oracle; the values are unchanged, output
    == input works and a sentinel-filled space domain is bit-identical afterwards."""
    import torch
    rng = np.random.default_rng(seed)
    vals = _values(rng, dims, idx, single)
    v = _potential(rng, dims, single)
    untouched = _fill_space(t)
    dv, dpot = torch.as_tensor(vals, device=gpu), torch.as_tensor(v, device=gpu)
    for full in (False, True):
        want = _oracle(idx, vals, v, dims, full=full)
        scaling = sp.Scaling.FULL if full else sp.Scaling.NONE
        for rep in range(2):
            out = t.apply_local(dv, dpot, scaling=scaling)
            err = max_rel_error(out.cpu().numpy(), want)
            print(dims, "fp32" if single else "fp64", "full" if full else "none", "rep", rep, err)
            assert err < _tol(single)
        assert dv.cpu().numpy().tobytes() == vals.tobytes()
        assert dpot.cpu().numpy().tobytes() == v.tobytes()
        buf = dv.clone()
        assert t.apply_local(buf, dpot, output=buf, scaling=scaling) is buf
        assert max_rel_error(buf.cpu().numpy(), want) < _tol(single)
    assert untouched(), "the fused call wrote the space domain"
    return vals, v


def _check_density(gpu, t, dims, idx, single, seed=72):
    """Two calls with WEIGHTS, each result against the oracle; values and space unchanged."""
    import torch
    rng = np.random.default_rng(seed)
    vals = _values(rng, dims, idx, single)
    rho0 = _rho0(rng, dims, single)
    mod2 = _mod2(idx, vals, dims)
    untouched = _fill_space(t)
    dv, drho = torch.as_tensor(vals, device=gpu), torch.as_tensor(rho0, device=gpu)
    want = rho0.astype(np.float64)
    for rep, w in enumerate(WEIGHTS):
        assert t.accumulate_density(dv, w, drho) is drho
        want = want + w * mod2
        err = max_rel_error(drho.cpu().numpy().astype(np.float64), want)
        print(dims, "fp32" if single else "fp64", "rep", rep, err)
        assert err < _tol(single)
    assert dv.cpu().numpy().tobytes() == vals.tobytes()
    assert untouched(), "the fused call wrote the space domain"
    return vals, rho0, mod2


def _logged(capfd):
    """(apply_local, density) of the last plan line SPFFT_LOG printed."""
    m = re.findall(r"apply_local=(\w+) density=(\w+)", capfd.readouterr().err)
    assert m, "no SPFFT_LOG line"
    return m[-1][0] == "fused", m[-1][1] == "fused"


# ------------------------------------------------------------------------- host
def test_host_r2c_stays_composed():
    dims = (32, 13, 5)
    idx = _random_indices(dims, 3)
    rng = np.random.default_rng(70)
    vals, v, rho0 = _values(rng, dims, idx), _potential(rng, dims), _rho0(rng, dims)
    t = _transform(HOST, dims, idx)
    assert t.apply_local_fused is False and t.density_fused is False
    for full in (False, True):
        out = t.apply_local(vals, v, scaling=sp.Scaling.FULL if full else sp.Scaling.NONE)
        assert max_rel_error(out, _oracle(idx, vals, v, dims, full=full)) < TOL64
    rho, want, mod2 = rho0.copy(), rho0.copy(), _mod2(idx, vals, dims)
    for w in WEIGHTS:
        t.accumulate_density(vals, w, rho)
        want = want + w * mod2
        assert max_rel_error(rho, want) < TOL64


# ------------------------------------------------------------------------ flags
@pytest.mark.gpu
def test_gpu_flags(gpu):
    dims = (64, 13, 5)
    idx = _random_indices(dims, 1)
    t = _transform(GPU, dims, idx)
    assert t.apply_local_fused is True and t.density_fused is True
    # the C2C-only operators stay composed on the fused R2C plan
    assert t.fock_fused is False
    assert t.spinor_fused is False
    assert t.values_fan_fused(3) is False
    # run-time half-lengths (8, 20) and odd dimX
    for other in ((16, 12, 10), (40, 9, 4), (33, 8, 4)):
        o = create_value_indices(np.random.default_rng(2), [1.0], 0.7, 0.8, *other, True)[0]
        u = _transform(GPU, other, o)
        assert u.apply_local_fused is False and u.density_fused is False, other
    for env in ({"SPFFT_R2C_PACKED": "0"}, {"SPFFT_R2C_FUSE": "0"}):
        u = _transform(GPU, dims, idx, env=env)
        assert u.apply_local_fused is False and u.density_fused is False, env


# ------------------------------------------------------- operator and density
@pytest.mark.gpu
@pytest.mark.parametrize("dims,single,seed", SHAPES)
def test_gpu_operator(gpu, dims, single, seed, capfd):
    idx = _random_indices(dims, seed)
    t = _transform(GPU, dims, idx, single=single, env={"SPFFT_LOG": "1"})
    logged = _logged(capfd)
    assert (t.apply_local_fused, t.density_fused) == logged
    if dims[0] != 1024:  # (the 1024-long shapes: right whatever the flag says)
        assert t.apply_local_fused is True
    if t.apply_local_fused:
        _check_operator(gpu, t, dims, idx, single)
    else:
        import torch
        rng = np.random.default_rng(71)
        vals, v = _values(rng, dims, idx, single), _potential(rng, dims, single)
        dv, dpot = torch.as_tensor(vals, device=gpu), torch.as_tensor(v, device=gpu)
        for full in (False, True):
            want = _oracle(idx, vals, v, dims, full=full)
            for _ in range(2):
                out = t.apply_local(dv, dpot, scaling=sp.Scaling.FULL if full else sp.Scaling.NONE)
                assert max_rel_error(out.cpu().numpy(), want) < _tol(single)
            assert dv.cpu().numpy().tobytes() == vals.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dims,single,seed", SHAPES)
def test_gpu_density(gpu, dims, single, seed, capfd):
    idx = _random_indices(dims, seed)
    t = _transform(GPU, dims, idx, single=single, env={"SPFFT_LOG": "1"})
    logged = _logged(capfd)
    assert (t.apply_local_fused, t.density_fused) == logged
    if dims[0] != 1024:
        assert t.density_fused is True
    if t.density_fused:
        _check_density(gpu, t, dims, idx, single)
    else:
        import torch
        rng = np.random.default_rng(72)
        vals, rho0 = _values(rng, dims, idx, single), _rho0(rng, dims, single)
        mod2 = _mod2(idx, vals, dims)
        dv, drho = torch.as_tensor(vals, device=gpu), torch.as_tensor(rho0, device=gpu)
        want = rho0.astype(np.float64)
        for w in WEIGHTS:
            t.accumulate_density(dv, w, drho)
            want = want + w * mod2
            assert max_rel_error(drho.cpu().numpy().astype(np.float64), want) < _tol(single)


@pytest.mark.gpu
@pytest.mark.parametrize("centred", [False, True])
def test_gpu_columns_without_sticks(gpu, centred):
    """The Nyquist column and the columns next to it hold no sticks: they read as zero in
    the pre-pass and the post pass stores nothing there."""
    dims, idx = _sphere(centred)
    t = _transform(GPU, dims, idx)
    assert t.apply_local_fused is True and t.density_fused is True
    _check_operator(gpu, t, dims, idx, False)
    _check_density(gpu, t, dims, idx, False)


# ------------------------------------------------------- fused against composed
@pytest.mark.gpu
def test_gpu_fused_matches_composed_and_unaligned(gpu):
    import torch
    dims = (64, 13, 5)
    nx, ny, nz = dims
    idx = _random_indices(dims, 1)
    fused = _transform(GPU, dims, idx)
    composed = _transform(GPU, dims, idx, env={"SPFFT_R2C_FUSE": "0"})
    assert fused.apply_local_fused is True and composed.apply_local_fused is False
    assert fused.density_fused is True and composed.density_fused is False
    rng = np.random.default_rng(73)
    vals, v, rho0 = _values(rng, dims, idx), _potential(rng, dims), _rho0(rng, dims)
    dv = torch.as_tensor(vals, device=gpu)
    dpot = torch.as_tensor(v, device=gpu)
    a = fused.apply_local(dv, dpot).cpu().numpy()
    b = composed.apply_local(dv, dpot).cpu().numpy()
    want = _oracle(idx, vals, v, dims)
    assert max_rel_error(a, b) < TOL64
    assert max_rel_error(a, want) < TOL64 and max_rel_error(b, want) < TOL64
    ra = fused.accumulate_density(dv, 1.5, torch.as_tensor(rho0, device=gpu)).cpu().numpy()
    rb = composed.accumulate_density(dv, 1.5, torch.as_tensor(rho0, device=gpu)).cpu().numpy()
    assert max_rel_error(ra, rb) < TOL64
    assert max_rel_error(ra, rho0 + 1.5 * _mod2(idx, vals, dims)) < TOL64
    # a potential / rho one element off the pair alignment: that call runs composed, the
    # space domain is then written (the documented fall-back) and the result is the same
    off = torch.empty(nz * ny * nx + 1, dtype=torch.float64, device=gpu)
    assert off.data_ptr() % 16 == 0
    upot = off[1:].view(nz, ny, nx)
    upot.copy_(dpot)
    assert upot.data_ptr() % 16 == 8
    u = fused.apply_local(dv, upot).cpu().numpy()
    assert max_rel_error(u, b) < TOL64 and max_rel_error(u, want) < TOL64
    off2 = torch.empty(nz * ny * nx + 1, dtype=torch.float64, device=gpu)
    urho = off2[1:].view(nz, ny, nx)
    urho.copy_(torch.as_tensor(rho0, device=gpu))
    assert fused.accumulate_density(dv, 1.5, urho) is urho
    assert max_rel_error(urho.cpu().numpy(), rb) < TOL64
    # unaligned arrays in a multi call take the per-transform path
    clone = fused.clone()
    outs = sp.multi_transform_apply_local([fused, clone], [dv, dv], [upot, upot])
    for o in outs:
        assert max_rel_error(o.cpu().numpy(), want) < TOL64
    # and the aligned call is fused again: the space domain stays untouched
    untouched = _fill_space(fused)
    assert max_rel_error(fused.apply_local(dv, dpot).cpu().numpy(), want) < TOL64
    assert untouched()


# ---------------------------------------------------------------------- batches
def _scope_counts(tree):
    """identifier -> summed call count over the whole timing tree."""
    counts = {}

    def walk(nodes):
        for n in nodes:
            counts[n["identifier"]] = counts.get(n["identifier"], 0) + n["count"]
            walk(n.get("sub-timings", []))

    walk(tree["timings"])
    return counts


# (64, 13, 5): partial row blocks, the bands update rho one after another; (32, 64, 4): full
# blocks, the bands are summed in registers
@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["1", "0"])
@pytest.mark.parametrize("dims,seed", [((64, 13, 5), 1), ((32, 64, 4), 1)])
def test_gpu_multi_transform(gpu, dims, seed, batch):
    import torch
    batching = batch != "0"
    idx = _random_indices(dims, seed)
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
    assert all(t.apply_local_fused and t.density_fused for t in ts)
    checks = [_fill_space(t) for t in ts]
    rng = np.random.default_rng(74)
    vals = [_values(rng, dims, idx) for _ in ts]
    pots = [_potential(rng, dims) for _ in ts]
    weights = [1.5, -0.5, 0.25]
    rho0 = _rho0(rng, dims)
    dvals = [torch.as_tensor(x, device=gpu) for x in vals]
    dpots = [torch.as_tensor(x, device=gpu) for x in pots]
    sp.timing_reset()
    sp.timing_enable(True, gpu_stages=False)
    try:
        first = None
        for rep in range(2):
            outs = sp.multi_transform_apply_local(ts, dvals, dpots)
            for o, x, p in zip(outs, vals, pots):
                assert max_rel_error(o.cpu().numpy(), _oracle(idx, x, p, dims)) < TOL64
            bits = [o.cpu().numpy().tobytes() for o in outs]
            assert first is None or bits == first  # the same call, the same bits
            first = bits
        outs = sp.multi_transform_apply_local(ts, dvals, [dpots[0]] * 3,
                                              scalings=[sp.Scaling.FULL] * 3)
        for o, x in zip(outs, vals):
            assert max_rel_error(o.cpu().numpy(), _oracle(idx, x, pots[0], dims, full=True)) < TOL64
        want = rho0.astype(np.float64)
        for x, w in zip(vals, weights):
            want = want + w * _mod2(idx, x, dims)
        results = []
        for rep in range(2):
            drho = torch.as_tensor(rho0, device=gpu)
            assert sp.multi_transform_accumulate_density(ts, dvals, weights, drho) is drho
            results.append(drho.cpu().numpy().copy())
            assert max_rel_error(results[-1], want) < TOL64
        assert results[0].tobytes() == results[1].tobytes()
        # on top of the first result
        sp.multi_transform_accumulate_density(ts, dvals, weights, drho)
        assert max_rel_error(drho.cpu().numpy(), 2 * want - rho0) < TOL64
        counts = _scope_counts(sp.timing_json())
    finally:
        sp.timing_enable(False)
    print("scopes", {k: n for k, n in counts.items() if "apply" in k or "density" in k})
    assert counts.get("multi_apply_local") == 3 and counts.get("multi_accumulate_density") == 3
    if batching:
        assert counts.get("gpu_apply_local_batch") == 3
        assert counts.get("x_apply_streamed_potential") == 2
        assert counts.get("x_apply_shared_potential") == 1
        assert counts.get("gpu_accumulate_density_batch") == 3
        assert "gpu_apply_local_xy" not in counts and "gpu_accumulate_density_xy" not in counts
    else:
        assert "gpu_apply_local_batch" not in counts and "gpu_accumulate_density_batch" not in counts
        assert counts.get("gpu_apply_local_xy") == 9
        assert counts.get("gpu_accumulate_density_xy") == 9
    assert all(c() for c in checks), "a fused call wrote a space domain"


# ------------------------------------------------------------------ other paths
@pytest.mark.gpu
def test_gpu_host_arrays(gpu):
    """numpy inputs on a GPU transform: staged through device buffers, the fused stages."""
    dims = (64, 13, 5)
    idx = _random_indices(dims, 1)
    t = _transform(GPU, dims, idx)
    assert t.apply_local_fused is True and t.density_fused is True
    rng = np.random.default_rng(75)
    vals, v, rho0 = _values(rng, dims, idx), _potential(rng, dims), _rho0(rng, dims)
    untouched = _fill_space(t)
    keep = vals.copy()
    for full in (False, True):
        out = t.apply_local(vals, v, scaling=sp.Scaling.FULL if full else sp.Scaling.NONE)
        out = out if isinstance(out, np.ndarray) else out.cpu().numpy()
        assert max_rel_error(out, _oracle(idx, vals, v, dims, full=full)) < TOL64
    rho, want, mod2 = rho0.copy(), rho0.copy(), _mod2(idx, vals, dims)
    for w in WEIGHTS:
        assert t.accumulate_density(vals, w, rho) is rho
        want = want + w * mod2
        assert max_rel_error(rho, want) < TOL64
    assert vals.tobytes() == keep.tobytes()
    assert untouched()


@pytest.mark.gpu
def test_gpu_capped_intermediate(gpu, capfd):
    """An intermediate capped below the local planes: several plane ranges, the fused stage
    in place in each."""
    dims = (64, 18, 6)
    nx, ny, nz = dims
    idx = _random_indices(dims, 1)
    t = _transform(GPU, dims, idx, env={"SPFFT_INTER_BYTES": str(nx * (ny + 8) * 16), "SPFFT_LOG": "1"})
    planes = int(re.findall(r"inter_planes=(\d+) apply_local=fused density=fused",
                            capfd.readouterr().err)[-1])
    assert -(-nz // planes) >= 2, planes
    assert t.apply_local_fused is True and t.density_fused is True
    _check_operator(gpu, t, dims, idx, False)
    _check_density(gpu, t, dims, idx, False)


def _pinned(op, **choices):
    """The case runner of tools/fuzz_ops.py on a hand-written configuration: two calls against
    the dense oracle, the inputs unchanged, a sentinel-filled space domain bit-identical."""
    import importlib.util
    if "fuzz_ops" not in sys.modules:
        spec = importlib.util.spec_from_file_location("fuzz_ops",
                                                      os.path.join(REPO, "tools", "fuzz_ops.py"))
        sys.modules["fuzz_ops"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules["fuzz_ops"])
    mod = sys.modules["fuzz_ops"]
    desc, err, _, facts = mod.run_case(mod.fixed_case(op, r2c=True, **choices))
    print(desc, err, facts)
    assert err < TOL64
    return facts


# Three virtual ranks of one GPU under the pipelined COMPACT_BUFFERED exchange, 2 plane
# chunks x 2 stick blocks forced; the second split leaves rank 1 without planes
@pytest.mark.gpu
@pytest.mark.parametrize("op", ["local", "density"])
@pytest.mark.parametrize("planes", [[1, 1, 1], [1, 0, 2]])
def test_gpu_virtual_ranks_pipelined(gpu, op, planes):
    facts = _pinned(op, dims=(32, 18, 30), stick_dist=[1, 1, 1], plane_dist=planes,
                    exchange="COMPACT_BUFFERED", chunks=2, blocks=2)
    assert len(facts) == 3
    assert any(f["planes"] == 0 for f in facts) == (0 in planes)
    for f in facts:
        assert f["fused"] is True, f
        assert f["plan"][:3] == (2, 2, False), f


@pytest.mark.gpu
def test_gpu_stage_timing_names_the_fused_stages(gpu):
    """backward holds y+x_apply+y (operator) and y+x_density (density) once per call."""
    import torch
    dims = (64, 13, 5)
    idx = _random_indices(dims, 1)
    t = _transform(GPU, dims, idx)
    rng = np.random.default_rng(76)
    dv = torch.as_tensor(_values(rng, dims, idx), device=gpu)
    dpot = torch.as_tensor(_potential(rng, dims), device=gpu)
    drho = torch.as_tensor(_rho0(rng, dims), device=gpu)

    def stages(call):
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
        dirs = {d["identifier"]: {s["identifier"]: s for s in d["sub-timings"]}
                for d in gpu_node[0]["sub-timings"]}
        for d in dirs.values():
            for node in d.values():
                assert node["count"] == 3, node
        return dirs

    dirs = stages(lambda: t.apply_local(dv, dpot))
    assert set(dirs["backward"]) == {"z", "exchange", "y+x_apply+y"}, dirs
    assert set(dirs["forward"]) == {"exchange", "z"}, dirs
    dirs = stages(lambda: t.accumulate_density(dv, 0.5, drho))
    assert set(dirs) == {"backward"}, dirs
    assert set(dirs["backward"]) == {"z", "exchange", "y+x_density"}, dirs
