#!/usr/bin/env python3
"""Randomised correctness sweep of the multi_transform member-list operators against the
dense numpy oracle.

A sibling of tools/fuzz_ops.py for the seven operators that take a list of transforms:

    fock_multi    multi_transform_accumulate_fock
    fan_out       multi_transform_reciprocal_fan_out
    fan_in        multi_transform_reciprocal_fan_in
    density_fan   multi_transform_accumulate_density_fan
    local_fan     multi_transform_apply_local_fan
    spinor_local  multi_transform_apply_local_spinor
    spin_density  multi_transform_accumulate_spin_density

Each case draws what tools/fuzz_ops.py draws (dimensions over every engine path, type,
precision, 1-3 virtual ranks with skewed and empty splits, exchange type, index fills,
centring, scaling, host pointers, forced exchange chunks and stick blocks, a capped y/x
intermediate) and the operator's own choices: the member count (one batch, its edge and
beyond it), kernel kinds, None and repeated kernels, shared arrays, in-place outputs, the
four-array forms of the spinor operators, a is b, and arrays off the pair alignment. Every
member is a transform on its own grid: a transform and its clones on one rank, the rank's
transforms of n distributed grids otherwise.

draw_case() holds every random choice and calls no library, so the coverage of a seed can
be judged without running anything; run_case() runs one drawn configuration.

    python tools/fuzz_multi_ops.py --cases 700 [--op all|fock_multi|fan_out|fan_in|density_fan|
                                   local_fan|spinor_local|spin_density]
                                   [--seed 1] [--max-elems 65536] [--pu gpu|host]

Every case makes two consecutive calls against the oracle (the accumulating operators both
as the whole array and as the update alone), checks that every input is bit-identical
afterwards, that the two calls of a non-accumulating operator return the same bits and, for
the pair operator on fused x plans, that a sentinel-filled space domain of every member
stays bit-identical. Prints one line per case and the largest error per operator and
precision; exit status 1 on any failure.
"""
import argparse
import contextlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fuzz_gpu import EXCHANGES, LONG, SHORT, draw_dims  # noqa: E402,F401
from fuzz_ops import ENV, PAD, _centred, _like, kernel_of, planes_of  # noqa: E402,F401

OPS = ("fock_multi", "fan_out", "fan_in", "density_fan", "local_fan", "spinor_local", "spin_density")
TOL64, TOL32 = 1e-12, 2e-5  # the project's pinned-test bounds on max_rel_error
MAX_BATCH, MAX_SPINORS = 8, 4  # members of one batch launch, spinors of one spinor launch
# member counts: one, inside a batch, the largest batch, beyond one batch (spinor operators:
# spinors, two members each)
COUNTS = {"fock_multi": (1, 2, 3, 8, 10), "fan_out": (1, 2, 3, 4, 8, 9), "fan_in": (1, 2, 3, 4, 8, 9),
          "density_fan": (1, 2, 3, 4, 8, 9), "local_fan": (1, 2, 3, 4, 8, 9),
          "spinor_local": (1, 2, 4, 5), "spin_density": (1, 2, 4, 5)}
R2C_OPS = ("fock_multi", "fan_out", "fan_in", "density_fan", "local_fan")
KINDS = {"fock_multi": ("real", "complex"), "fan_out": ("real", "complex"), "fan_in": ("real", "complex"),
         "density_fan": ("real", "complex", "grad"), "local_fan": ("real", "complex", "grad"),
         "spinor_local": ("none",), "spin_density": ("none",)}
# arrays of each operator that may be host pointers on a GPU transform (one name covers the
# arrays of every member)
HOST_ARRAYS = {"fock_multi": ("a", "b", "kernel", "acc"),
               "fan_out": ("kernel", "values", "space"),
               "fan_in": ("kernel", "space"),
               "density_fan": ("values", "kernel", "rho"),
               "local_fan": ("values", "kernel", "potential", "output"),
               "spinor_local": ("values", "potential", "output"),
               "spin_density": ("values", "rho")}
BATCH_SCOPE = {"fock_multi": "gpu_accumulate_fock_batch", "fan_out": "gpu_reciprocal_fan_out_batch",
               "fan_in": "gpu_reciprocal_fan_in_batch", "density_fan": "gpu_accumulate_density_fan_batch",
               "local_fan": "gpu_apply_local_fan_batch", "spinor_local": "gpu_apply_local_spinor_batch",
               "spin_density": "gpu_accumulate_spin_density_batch"}
# (s_x, s_y, s_z) of member i's translation kernel
SHIFTS = [(1, 2, 3), (-2, 1, 0), (0, -1, 2), (3, 0, -1), (2, 2, 2), (-1, -3, 1), (1, 0, 0),
          (0, 4, -2), (-3, 1, 1), (2, -1, -2), (-1, 1, 4)]
MAX_MEMBERS = 10


def draw_case(rng, op, max_elems):
    """Every random choice of one case, as a dict. No library call. Every operator draws the
    same sequence; the choices an operator has no use for are ignored."""
    dims = draw_dims(rng, max_elems)
    r2c = bool(rng.random() < 0.4) and op in R2C_OPS
    single = bool(rng.random() < 0.4)
    P = int(rng.choice([1, 1, 2, 3]))
    exchange = str(rng.choice(EXCHANGES))
    stick_dist = [float(rng.integers(0, 3)) for _ in range(P)]
    if sum(stick_dist) == 0:
        stick_dist[0] = 1.0
    plane_dist = [float(rng.integers(0, 3)) for _ in range(P)]
    if sum(plane_dist) == 0:
        plane_dist[-1] = 1.0
    stick_fill = float(rng.uniform(0.3, 1.0))
    z_fill = 1.0 if rng.random() < 0.34 else float(rng.uniform(0.4, 1.0))
    centred = bool(rng.random() < 0.3)
    full = bool(rng.random() < 0.5)
    host_ptrs = []
    if rng.random() < 0.25:
        host_ptrs = [n for n in HOST_ARRAYS[op] if rng.random() < 0.5]
    chunks = int(rng.choice([0, 0, 2, 3]))  # 0: unset
    blocks = int(rng.choice([0, 0, 2]))
    if P == 1:
        chunks = blocks = 0
    cap_planes = int(rng.choice([1, 2])) if rng.random() < 0.2 else 0
    n = int(rng.choice(COUNTS[op]))
    kind = str(rng.choice(KINDS[op]))
    if kind == "grad" and r2c:  # i G_d is not Hermitian-consistent input of the composed R2C path
        kind = "complex"
    weights = [float(rng.choice([-1.0, 1.0]) * rng.uniform(0.25, 1.5)) for _ in range(MAX_MEMBERS)]
    want_values = bool(rng.random() < 0.5)       # fan_out: the values output
    prefill = bool(rng.random() < 0.4)           # fan_out: the input already in place
    none_space = int(rng.integers(n)) if rng.random() < 0.4 else -1  # fan_in: spaces[i] is None
    repeat = n > 1 and bool(rng.random() < 0.3)  # fans: members 0 and 1 get one kernel object
    none_in = [bool(rng.random() < 0.25) for _ in range(MAX_MEMBERS)]   # value fans: identity K
    none_out = [bool(rng.random() < 0.25) for _ in range(MAX_MEMBERS)]  # local_fan: identity L
    shared_pot = bool(rng.random() < 0.4)        # local_fan: one potential n times
    out_is_in = bool(rng.random() < 0.25)        # local_fan, spinor_local
    four_list = bool(rng.random() < 0.5)         # spinors: four arrays, not one [4, z, y, x]
    shared_b = bool(rng.random() < 0.5)          # fock_multi
    same = [bool(rng.random() < 0.25) for _ in range(MAX_MEMBERS)]  # fock_multi: a[i] is b[i]
    kernel_list = bool(rng.random() < 0.5)       # fock_multi: one kernel per member
    nul = bool(rng.random() < 0.5)               # None, not empty arrays, on a rank without them
    unaligned = ""
    if op == "fock_multi" and P == 1 and r2c and rng.random() < 0.35:
        unaligned = str(rng.choice(["a", "b", "acc"]))
        host_ptrs = []
    return {"op": op, "dims": dims, "r2c": r2c, "single": single, "P": P, "exchange": exchange,
            "stick_dist": stick_dist, "plane_dist": plane_dist, "stick_fill": stick_fill,
            "z_fill": z_fill, "centred": centred, "full": full, "host_ptrs": host_ptrs,
            "chunks": chunks, "blocks": blocks, "cap_planes": cap_planes, "n": n, "kind": kind,
            "weights": weights, "values": want_values, "prefill": prefill, "none_space": none_space,
            "repeat": repeat, "none_in": none_in, "none_out": none_out, "shared_pot": shared_pot,
            "out_is_in": out_is_in, "four_list": four_list, "shared_b": shared_b, "same": same,
            "kernel_list": kernel_list, "nul": nul, "unaligned": unaligned,
            "data_seed": int(rng.integers(1 << 31))}


def fixed_case(op, dims, stick_dist=(1.0,), plane_dist=(1.0,), **choices):
    """A configuration written by hand (the pinned tests): three members (two spinors), C2C
    fp64 with complex kernels, full scaling, device arrays, every optional output present,
    nothing shared, repeated, in place or None, and no forced environment, unless `choices`
    says so."""
    cfg = {"op": op, "dims": tuple(dims), "r2c": False, "single": False, "P": len(stick_dist),
           "exchange": "COMPACT_BUFFERED", "stick_dist": [float(s) for s in stick_dist],
           "plane_dist": [float(p) for p in plane_dist], "stick_fill": 0.9, "z_fill": 0.8,
           "centred": False, "full": True, "host_ptrs": [], "chunks": 0, "blocks": 0, "cap_planes": 0,
           "n": 2 if op in ("spinor_local", "spin_density") else 3,
           "kind": "none" if op in ("spinor_local", "spin_density") else "complex",
           "weights": [-0.75, 0.5, -1.25, 1.0, 0.25, -0.5, 0.75, 1.5, -1.0, 0.375],
           "values": True, "prefill": False, "none_space": -1, "repeat": False,
           "none_in": [False] * MAX_MEMBERS, "none_out": [False] * MAX_MEMBERS, "shared_pot": False,
           "out_is_in": False, "four_list": False, "shared_b": False, "same": [False] * MAX_MEMBERS,
           "kernel_list": True, "nul": False, "unaligned": "", "data_seed": 64}
    unknown = set(choices) - set(cfg)
    if unknown or len(plane_dist) != len(stick_dist) or op not in OPS:
        raise ValueError(f"fixed_case: {sorted(unknown) or 'one share per rank, a known operator'}")
    cfg.update(choices)
    return cfg


def members_of(cfg):
    """Transforms of one call: n, or two per spinor."""
    return 2 * cfg["n"] if cfg["op"] in ("spinor_local", "spin_density") else cfg["n"]


def describe(cfg):
    op, n = cfg["op"], cfg["n"]
    d = (f"{op}: n={n} dims={cfg['dims']} {'R2C' if cfg['r2c'] else 'C2C'} "
         f"{'fp32' if cfg['single'] else 'fp64'} P={cfg['P']} "
         f"{cfg['exchange'] if cfg['P'] > 1 else 'local'} sticks={cfg['stick_dist']} "
         f"planes={cfg['plane_dist']} fill={cfg['stick_fill']:.2f}/{cfg['z_fill']:.2f}")
    d += " centred" if cfg["centred"] else ""
    d += " full" if cfg["full"] else ""
    if cfg["kind"] != "none":
        d += f" K={cfg['kind']}"
    if op in ("fan_out", "fan_in"):
        d += " repeat" if cfg["repeat"] else ""
    if op == "fan_out":
        d += (" values" if cfg["values"] else "") + (" prefilled" if cfg["prefill"] else "")
    if op == "fan_in" and cfg["none_space"] >= 0:
        d += f" spaces[{cfg['none_space']}]=None"
    if op in ("density_fan", "local_fan"):
        d += " Kin=" + "".join("-" if x else "k" for x in cfg["none_in"][:n])
    if op == "local_fan":
        d += " Kout=" + "".join("-" if x else "k" for x in cfg["none_out"][:n])
        d += " shared_pot" if cfg["shared_pot"] else ""
    if op in ("local_fan", "spinor_local") and cfg["out_is_in"]:
        d += " out_is_in"
    if op in ("spinor_local", "spin_density"):
        d += " four_arrays" if cfg["four_list"] else " [4,z,y,x]"
    if op == "fock_multi":
        d += " shared_b" if cfg["shared_b"] else ""
        d += " a_is_b=" + "".join("1" if x else "0" for x in cfg["same"][:n])
        d += " kernels" if cfg["kernel_list"] else " one_kernel"
        d += f" unaligned:{cfg['unaligned']}" if cfg["unaligned"] else ""
    if cfg["host_ptrs"]:
        d += " host:" + ",".join(cfg["host_ptrs"])
    if cfg["chunks"] or cfg["blocks"]:
        d += f" KxI={cfg['chunks'] or '-'}x{cfg['blocks'] or '-'}"
    if cfg["cap_planes"]:
        d += f" inter={cfg['cap_planes']}pl"
    d += " nul" if cfg["nul"] and cfg["P"] > 1 else ""
    return d + f" seed={cfg['data_seed']}"


def member_kernel(idx, dims, kind, member):
    """Member's kernel in double precision, |K| <= 1. 'real': Gaussian on centred G, narrower
    per member; 'complex': the member's translation phase; 'grad': i G_d / (N_d / 2) with
    d = member mod 3."""
    g = _centred(idx, dims).astype(np.float64)
    if kind == "real":
        c = max(1.0, sum(n * n for n in dims) / 16.0) / (1 + member)
        return np.exp(-(g ** 2).sum(axis=1) / c)
    if kind == "grad":
        d = member % 3
        return 1j * g[:, d] / (dims[d] / 2)
    s = SHIFTS[member % len(SHIFTS)]
    return np.exp(-2j * np.pi * sum(g[:, d] * s[d] / dims[d] for d in range(3)))


@contextlib.contextmanager
def forced_environment(cfg, rdt):
    """The switches the library reads when a grid or transform is created."""
    nx, ny, _ = cfg["dims"]
    env = {}
    if cfg["chunks"]:
        env["SPFFT_EXCH_CHUNKS"] = str(cfg["chunks"])
    if cfg["blocks"]:
        env["SPFFT_EXCH_STICK_BLOCKS"] = str(cfg["blocks"])
    if cfg["cap_planes"]:
        env["SPFFT_INTER_BYTES"] = str(cfg["cap_planes"] * nx * (ny + PAD) * 2 * np.dtype(rdt).itemsize)
    saved = {n: os.environ.get(n) for n in ENV}
    try:
        for n in ENV:
            os.environ.pop(n, None)
        os.environ.update(env)
        yield
    finally:
        for n, v in saved.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


def _scope_counts(tree):
    counts = {}

    def walk(nodes):
        for n in nodes:
            counts[n["identifier"]] = counts.get(n["identifier"], 0) + n["count"]
            walk(n.get("sub-timings", []))

    walk(tree["timings"])
    return counts


def run_case(cfg, host=False):
    """Runs one drawn configuration. Returns (desc, err, tol, facts); facts holds one dict
    per rank: flag (the operator's plan flag for the drawn n), reciprocal_fused, batchable
    (a plan flag that implies batchable() is set), plan (exchange_plan() of a GPU
    transform), planes, values, device (no argument is a host pointer), calls, groups (batch
    launches per call if the batch path runs) and, on one GPU rank, counts (the timing
    scopes of the calls)."""
    import spfft_amd as sp
    from spfft_amd.parallel import run_ranks
    from spfft_amd.utils.indices import create_value_indices
    from spfft_amd.utils.oracle import dense_backward, dense_forward, max_rel_error
    if not host:
        import torch

    op, dims, r2c, single, P = cfg["op"], cfg["dims"], cfg["r2c"], cfg["single"], cfg["P"]
    nx, ny, nz = dims
    n, M = cfg["n"], members_of(cfg)
    exchange, kind, full = cfg["exchange"], cfg["kind"], cfg["full"]
    hostp = set() if host else set(cfg["host_ptrs"])
    unaligned = "" if host else cfg["unaligned"]
    ws = cfg["weights"][:n]
    rng = np.random.default_rng(cfg["data_seed"])
    parts = create_value_indices(rng, cfg["stick_dist"], cfg["stick_fill"], cfg["z_fill"], nx, ny, nz, r2c)
    if cfg["centred"]:  # the same index set in centred form (negative frequencies)
        half = np.array([nx // 2, ny // 2, nz // 2])
        n3 = np.array([nx, ny, nz])
        parts = [np.where(p > half, p - n3, p).astype(np.int32) for p in parts]
    planes = planes_of(cfg)
    offsets = np.concatenate([[0], np.cumsum(planes)])
    starts = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    all_idx = np.concatenate(parts)
    N = nx * ny * nz

    rdt = np.float32 if single else np.float64
    cdt = np.complex64 if single else np.complex128
    sdt = rdt if r2c else cdt  # of arrays over the space domain
    wide = np.float64 if r2c else np.complex128
    scaling = sp.Scaling.FULL if full else sp.Scaling.NONE

    def field():
        """Unit variance, [z][y][x]."""
        if r2c:
            return rng.standard_normal((nz, ny, nx))
        return (rng.standard_normal((nz, ny, nx)) + 1j * rng.standard_normal((nz, ny, nx))) / np.sqrt(2)

    def values_of(f):
        """Values of a real-space field (consistent R2C input), unit variance."""
        return (dense_forward(f.astype(wide), all_idx, dims, r2c=r2c) / np.sqrt(N)).astype(cdt)

    def back(v):
        return dense_backward(all_idx, np.asarray(v).astype(np.complex128), dims, r2c=r2c)

    def fwd(f, scale=full):
        return dense_forward(f, all_idx, dims, r2c=r2c, scale=scale)

    def kernels_of(first=0, count=M):
        kdt = rdt if kind == "real" else cdt
        return [member_kernel(all_idx, dims, kind, first + i).astype(kdt) for i in range(count)]

    def k64(k):
        return 1.0 if k is None else k.astype(np.complex128)

    # inputs in working precision, oracles in double precision from those inputs; every
    # global input array has a name, the arrays of a member list one name and one list
    g_in = {}     # name -> global array, or list of global arrays (entries may repeat or be None)
    want = {}     # name -> oracle of a result (lists per member)
    if op in ("fan_out", "fan_in"):
        ks = kernels_of()
        if cfg["repeat"]:
            ks[1] = ks[0]
        g_in["kernel"] = ks
        if op == "fan_out":
            f = field().astype(sdt)
            g_in["space"] = [f]
            want["values"] = fwd(f.astype(wide))
            want["space"] = [back(k64(k) * want["values"]) for k in ks]
        else:
            fs = [field().astype(sdt) for _ in range(n)]
            g_in["space"] = fs
            want["space"] = [back(sum(k64(k) * fwd(f.astype(wide)) for k, f in zip(ks, fs)))]
    elif op in ("density_fan", "local_fan"):
        vals = values_of(field().astype(sdt))
        kin = [None if cfg["none_in"][i] else k for i, k in enumerate(kernels_of())]
        g_in["values"], g_in["kernel"] = [vals], kin
        psi = [back(k64(k) * vals.astype(np.complex128)) for k in kin]
        if op == "density_fan":
            upd = sum(w * (np.abs(s) ** 2) for w, s in zip(ws, psi))
            start = _like(rng, upd).astype(rdt)
        else:
            kout = [None if cfg["none_out"][i] else k for i, k in enumerate(kernels_of(first=2))]
            pots = [rng.uniform(-1, 1, (nz, ny, nx)).astype(rdt) for _ in range(1 if cfg["shared_pot"] else n)]
            pots = pots * n if cfg["shared_pot"] else pots
            g_in["kernel_out"], g_in["potential"] = kout, pots
            want["output"] = sum(k64(l) * fwd(s * v.astype(np.float64)) for l, s, v in zip(kout, psi, pots))
    elif op in ("spinor_local", "spin_density"):
        ins = [values_of(field().astype(sdt)) for _ in range(M)]
        g_in["values"] = ins
        psi = [back(c) for c in ins]
        if op == "spinor_local":
            pot = rng.uniform(-1, 1, (4, nz, ny, nx)).astype(rdt)
            g_in["potential"] = [pot]
            p64 = pot.astype(np.float64)
            vud = p64[2] + 1j * p64[3]
            want["output"] = []
            for u, d in zip(psi[0::2], psi[1::2]):
                want["output"].append(fwd(p64[0] * u + vud * d))
                want["output"].append(fwd(np.conj(vud) * u + p64[1] * d))
        else:
            upd = np.zeros((4, nz, ny, nx))
            for u, d, w in zip(psi[0::2], psi[1::2], ws):
                ud = u * np.conj(d)
                upd[0] += w * np.abs(u) ** 2
                upd[1] += w * np.abs(d) ** 2
                upd[2] += w * ud.real
                upd[3] += w * ud.imag
            start = _like(rng, upd).astype(rdt)
    else:
        a_in = [field().astype(sdt) for _ in range(n)]
        b0 = field().astype(sdt)
        b_in = []
        for i in range(n):
            if cfg["same"][i]:
                b_in.append(a_in[i])
            else:
                b_in.append(b0 if cfg["shared_b"] else field().astype(sdt))
        k0 = kernel_of(all_idx, dims, kind).astype(rdt if kind == "real" else cdt)
        ks = [(k0 / (1.0 + 0.25 * i)).astype(k0.dtype) for i in range(n)] if cfg["kernel_list"] else [k0] * n
        g_in["a"], g_in["b"], g_in["kernel"] = a_in, b_in, ks
        upd = 0
        for ai, bi, ki, w in zip(a_in, b_in, ks, ws):
            a64, b64 = ai.astype(wide), bi.astype(wide)
            upd = upd + w * a64 * back(k64(ki) * fwd(np.conj(a64) * b64))
        start = _like(rng, upd).astype(sdt)

    ttype = sp.TransformType.R2C if r2c else sp.TransformType.C2C
    PU = sp.ProcessingUnit.HOST if host else sp.ProcessingUnit.GPU
    HOSTPU = sp.ProcessingUnit.HOST
    nthreads = 2 if host else 1
    G = sp.GridFloat if single else sp.Grid
    tol = TOL32 if (single or (P > 1 and exchange.endswith("FLOAT"))) else TOL64

    def arr(x, name, off=False):
        """Argument array: numpy on the host engine or for a host pointer, else a GPU tensor;
        `off`: one element off the pair alignment."""
        x = np.ascontiguousarray(x)
        if host or name in hostp:
            return x.copy()
        if off:
            buf = torch.empty(x.size + 1, dtype=torch.as_tensor(x[:0]).dtype, device="cuda")
            y = buf[1:].view(*x.shape)
            y.copy_(torch.as_tensor(x, device="cuda"))
            assert y.data_ptr() % (2 * x.itemsize) == x.itemsize
        else:
            y = torch.as_tensor(x, device="cuda")  # (a copy: x is host memory)
        torch.cuda.synchronize()
        return y

    def npy(y):
        return y if isinstance(y, np.ndarray) else y.cpu().numpy()

    def same_bits(x, ref):
        return npy(x).tobytes() == np.ascontiguousarray(ref).tobytes()

    def flag_of(t):
        if op in ("fan_out", "fan_in"):
            return bool(t.reciprocal_fan_fused(n))
        if op in ("density_fan", "local_fan"):
            return bool(t.values_fan_fused(n))
        if op in ("spinor_local", "spin_density"):
            return bool(t.spinor_fused)
        return bool(t.fock_fused or t.fock_r2c_fused)

    def body(rank, comm):
        if not host:
            torch.cuda.set_device(0)
        if P == 1:
            grid = G(nx, ny, nz, nx * ny, PU, nthreads)
            t0 = grid.create_transform(PU, ttype, nx, ny, nz, planes[rank], parts[rank])
            ts = [t0] + [t0.clone() for _ in range(M - 1)]
        else:
            ms = max(len(np.unique(p[:, 0].astype(np.int64) * ny + p[:, 1])) if len(p) else 0 for p in parts)
            ts = []
            for _ in range(M):
                grid = G(nx, ny, nz, max(1, ms), PU, nthreads, max_local_z_length=max(planes),
                         comm=comm, exchange_type=getattr(sp.ExchangeType, exchange))
                ts.append(grid.create_transform(PU, ttype, nx, ny, nz, planes[rank], parts[rank]))
        t0 = ts[0]
        z = slice(offsets[rank], offsets[rank + 1])
        g = slice(starts[rank], starts[rank + 1])
        nvals, nplanes = len(parts[rank]), int(planes[rank])
        # a rank without values or planes passes None where the call takes it
        no_vals = cfg["nul"] and nvals == 0
        no_planes = cfg["nul"] and nplanes == 0

        def cut(x, name):
            """A rank's part of a global array: values and kernels by value range, arrays over
            the space domain by z range (the four-array forms keep their leading axis)."""
            if x is None:
                return None
            if name in ("values", "kernel", "kernel_out", "output"):
                return x[g]
            return x[:, z] if x.ndim == 4 else x[z]

        def local(name, off_member=-1):
            """Argument arrays of one name, one per distinct global array (repeats stay
            repeats), and the rank's parts they must still equal afterwards."""
            cache, out, refs = {}, [], []
            hname = "kernel" if name == "kernel_out" else name
            for i, x in enumerate(g_in[name]):
                if x is None:
                    out.append(None)
                    continue
                if id(x) not in cache:
                    part = cut(x, name)
                    cache[id(x)] = arr(part, hname, off=i == off_member)
                    refs.append((cache[id(x)], part))
                out.append(cache[id(x)])
            return out, refs

        def unchanged(refs):
            return all(same_bits(y, part) for y, part in refs)

        def accumulated(call, fetch, start_r, upd_r):
            """Two consecutive calls: the whole array and the array minus its start."""
            errs = []
            s64 = start_r.astype(upd_r.dtype)
            for c in (1, 2):
                call()
                got = npy(fetch()).astype(upd_r.dtype)
                errs.append(max_rel_error(got, s64 + c * upd_r))
                errs.append(max_rel_error(got - s64, c * upd_r))
            return errs

        timed = P == 1 and not host
        if timed:
            sp.timing_reset()
            sp.timing_enable(True, gpu_stages=False)
        errs, ok, groups = [], True, 0
        untouched = lambda: True  # noqa: E731
        try:
            if op == "fan_out":
                ks, krefs = local("kernel")
                loc = HOSTPU if (host or "space" in hostp) else PU
                slab = arr(g_in["space"][0][z], "space")
                res = []
                for _ in range(2):
                    out = arr(np.full(nvals, -1, dtype=cdt), "values") if cfg["values"] else None
                    if cfg["prefill"]:
                        d0 = t0.space_domain(loc)
                        if isinstance(d0, np.ndarray):
                            d0[...] = npy(slab).reshape(d0.shape)
                        else:
                            d0.copy_(slab.reshape(d0.shape))
                        spaces = sp.multi_transform_reciprocal_fan_out(ts, ks, values=out, location=loc,
                                                                       scaling=scaling)
                    else:
                        spaces = sp.multi_transform_reciprocal_fan_out(ts, ks, space=slab, values=out,
                                                                       location=loc, scaling=scaling)
                    got = [np.array(npy(s)) for s in spaces]
                    errs += [max_rel_error(s, w[z]) for s, w in zip(got, want["space"])]
                    if out is not None:
                        errs.append(max_rel_error(npy(out), want["values"][g]))
                        got.append(np.array(npy(out)))
                    res.append(b"".join(x.tobytes() for x in got))
                ok = unchanged(krefs) and same_bits(slab, g_in["space"][0][z]) and res[0] == res[1]
                groups = 1 if 2 <= n <= MAX_BATCH else 0
            elif op == "fan_in":
                ks, krefs = local("kernel")
                loc = HOSTPU if (host or "space" in hostp) else PU
                slabs, srefs = local("space")
                j = cfg["none_space"]
                res = []
                for _ in range(2):
                    given = list(slabs)
                    if j >= 0:
                        dj = ts[j].space_domain(loc)
                        if isinstance(dj, np.ndarray):
                            dj[...] = npy(slabs[j]).reshape(dj.shape)
                        else:
                            dj.copy_(slabs[j].reshape(dj.shape))
                        given[j] = None
                    got = np.array(npy(sp.multi_transform_reciprocal_fan_in(ts, ks, spaces=given, location=loc,
                                                                            scaling=scaling)))
                    errs.append(max_rel_error(got, want["space"][0][z]))
                    res.append(got.tobytes())
                    # the other members' space domains are only read
                    ok = ok and all(same_bits(t.space_domain(loc), f[z])
                                    for t, f in zip(ts[1:], g_in["space"][1:]))
                ok = ok and unchanged(krefs) and unchanged(srefs) and res[0] == res[1]
                groups = 1 if 2 <= n <= MAX_BATCH else 0
            elif op == "density_fan":
                ks, krefs = local("kernel")
                v = None if no_vals else arr(g_in["values"][0][g], "values")
                rho = None if no_planes else arr(start[z], "rho")
                fn = sp.multi_transform_accumulate_density_fan
                if rho is None:
                    for _ in range(2):
                        fn(ts, v, ks, ws, None)
                else:
                    errs += accumulated(lambda: fn(ts, v, ks, ws, rho), lambda: rho, start[z], upd[z])
                ok = unchanged(krefs) and (v is None or same_bits(v, g_in["values"][0][g]))
                groups = 1 if n <= MAX_BATCH else 0
            elif op == "local_fan":
                kin, krefs = local("kernel")
                kout, lrefs = local("kernel_out")
                if no_planes:
                    pots, prefs = [None] * n, []
                else:
                    pots, prefs = local("potential")
                res = []
                for _ in range(2):
                    v = None if no_vals else arr(g_in["values"][0][g], "values")
                    if cfg["out_is_in"]:
                        out = v
                    else:
                        out = None if no_vals else arr(np.full(nvals, -1, dtype=cdt), "output")
                    ret = sp.multi_transform_apply_local_fan(ts, v, kin, pots, kout, output=out, scaling=scaling)
                    if out is not None and ret is not out:
                        ok = False
                    got = np.array(npy(ret))
                    errs.append(max_rel_error(got, want["output"][g]))
                    res.append(got.tobytes())
                    if v is not None and not cfg["out_is_in"]:
                        ok = ok and same_bits(v, g_in["values"][0][g])
                ok = ok and unchanged(krefs) and unchanged(lrefs) and unchanged(prefs) and res[0] == res[1]
                groups = 1 if n <= MAX_BATCH else 0
            elif op == "spinor_local":
                pot_r = g_in["potential"][0][:, z]
                if cfg["four_list"]:
                    pot = [None] * 4 if no_planes else [arr(pot_r[k], "potential") for k in range(4)]
                    prefs = [] if no_planes else [(p, pot_r[k]) for k, p in enumerate(pot)]
                else:
                    pot = arr(pot_r, "potential")
                    prefs = [(pot, pot_r)]
                res = []
                for _ in range(2):
                    vs = [None if no_vals else arr(c[g], "values") for c in g_in["values"]]
                    if cfg["out_is_in"]:
                        outs = vs
                    else:
                        outs = [None if no_vals else arr(np.full(nvals, -1, dtype=cdt), "output") for _ in vs]
                    ret = sp.multi_transform_apply_local_spinor(ts, vs, pot, outputs=outs, scaling=scaling)
                    if any(r is not o for r, o in zip(ret, outs)):
                        ok = False
                    got = [np.zeros(0, dtype=cdt) if r is None else np.array(npy(r)) for r in ret]
                    errs += [max_rel_error(x, w[g]) for x, w in zip(got, want["output"])]
                    res.append(b"".join(x.tobytes() for x in got))
                    if not cfg["out_is_in"]:
                        ok = ok and all(x is None or same_bits(x, c[g]) for x, c in zip(vs, g_in["values"]))
                ok = ok and unchanged(prefs) and res[0] == res[1]
                groups = (n + MAX_SPINORS - 1) // MAX_SPINORS
            elif op == "spin_density":
                vs, vrefs = local("values")
                if no_vals:
                    vs, vrefs = [None] * M, []
                fn = sp.multi_transform_accumulate_spin_density
                start_r, upd_r = start[:, z], upd[:, z]
                if cfg["four_list"]:
                    if no_planes:
                        for _ in range(2):
                            fn(ts, vs, ws, [None] * 4)
                    else:
                        m = [arr(start_r[k], "rho") for k in range(4)]
                        errs += accumulated(lambda: fn(ts, vs, ws, m), lambda: np.stack([npy(x) for x in m]),
                                            start_r, upd_r)
                else:
                    m = arr(start_r, "rho")
                    errs += accumulated(lambda: fn(ts, vs, ws, m), lambda: m, start_r, upd_r)
                ok = unchanged(vrefs)
                groups = (n + MAX_SPINORS - 1) // MAX_SPINORS
            else:
                fused_x = bool(t0.fock_fused or t0.fock_r2c_fused)
                a, arefs = local("a", off_member=0 if unaligned == "a" else -1)
                # b entries that are a's stay a's (a[i] is b[i]); the others are b's own arrays
                cache, b, brefs = {id(x): y for x, y in zip(g_in["a"], a)}, [], []
                for i, x in enumerate(g_in["b"]):
                    if id(x) not in cache:
                        cache[id(x)] = arr(x[z], "b", off=unaligned == "b" and not brefs)
                        brefs.append((cache[id(x)], x[z]))
                    b.append(cache[id(x)])
                ks, krefs = local("kernel")
                karg = ks if cfg["kernel_list"] else ks[0]
                acc = arr(start[z], "acc", off=unaligned == "acc")
                if not host and fused_x and not unaligned and not hostp & {"a", "b", "acc"}:
                    # fused x plans never form the space domain
                    doms = [t.space_domain(PU) for t in ts]
                    for d in doms:
                        d.fill_(-7.25)
                    before = [d.cpu().numpy().tobytes() for d in doms]
                    untouched = lambda: all(d.cpu().numpy().tobytes() == x  # noqa: E731
                                            for d, x in zip(doms, before))
                errs += accumulated(lambda: sp.multi_transform_accumulate_fock(ts, a, b, karg, ws, acc,
                                                                               scaling=scaling),
                                    lambda: acc, start[z], upd[z])
                ok = unchanged(arefs) and unchanged(brefs) and unchanged(krefs)
                # members a batch may take (an R2C member with a misaligned array runs composed),
                # in groups of at most MAX_BATCH; a group of one runs per transform
                if not host:
                    def aligned(y):
                        return isinstance(y, np.ndarray) or y.data_ptr() % (2 * y.element_size()) == 0
                    free = [not r2c or (aligned(a[i]) and aligned(b[i]) and aligned(acc)) for i in range(n)]
                    m = sum(free)
                    groups = m // MAX_BATCH + (1 if m % MAX_BATCH >= 2 else 0)
            counts = _scope_counts(sp.timing_json()) if timed else None
        finally:
            if timed:
                sp.timing_enable(False)
        if not ok:
            errs.append(float("inf"))  # an input changed, or two calls differ in their bits
        if not untouched():
            errs.append(float("inf"))  # a fused x plan wrote the space domain
        gpu = not host
        facts = {"flag": flag_of(t0), "reciprocal_fused": bool(t0.reciprocal_fused),
                 "batchable": bool(gpu and (t0.spinor_fused or t0.values_fan_fused(1)
                                            or t0.reciprocal_fan_fused(2))),
                 "plan": t0.exchange_plan() if gpu else None, "planes": nplanes, "values": nvals,
                 "device": not hostp, "calls": 2, "groups": groups, "counts": counts}
        return max(errs, default=0.0), facts

    with forced_environment(cfg, rdt):
        results = [body(0, None)] if P == 1 else run_ranks(P, body)
    return describe(cfg), max(e for e, _ in results), tol, [f for _, f in results]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", choices=("all",) + OPS, default="all")
    ap.add_argument("--cases", type=int, default=70, help="in all, shared by the operators in turn")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-elems", type=int, default=1 << 16)
    ap.add_argument("--pu", choices=["gpu", "host"], default="gpu",
                    help="host: the same sweep on SPFFT_PU_HOST (runs without a GPU)")
    a = ap.parse_args()
    ops = OPS if a.op == "all" else (a.op,)
    rng = np.random.default_rng(a.seed)
    bad = 0
    worst = {}
    t0 = time.time()
    for c in range(a.cases):
        cfg = draw_case(rng, ops[c % len(ops)], a.max_elems)
        try:
            desc, err, tol, _ = run_case(cfg, host=a.pu == "host")
        except Exception as e:  # an exception is a failure, never a skip
            desc, err, tol = f"{describe(cfg)}: {type(e).__name__}: {e}", float("inf"), 0.0
        ok = err < tol
        bad += 0 if ok else 1
        if ok:
            key = (cfg["op"], "fp32/float exchange" if tol > 1e-6 else "fp64")
            worst[key] = max(worst.get(key, 0.0), err)
        print(f"{'ok  ' if ok else 'FAIL'} case {c}: {desc} err={err:.2e} tol={tol:.0e}", flush=True)
    for (op, prec), e in sorted(worst.items()):
        print(f"largest error {op} {prec}: {e:.2e}")
    print(f"{a.cases - bad}/{a.cases} passed in {time.time() - t0:.0f} s", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
