#!/usr/bin/env python3
"""Randomised correctness sweep of the fused operators against the dense numpy oracle.

A sibling of tools/fuzz_gpu.py (which sweeps backward and forward) for apply_local,
accumulate_density, apply_reciprocal and accumulate_fock. Each case draws dimensions from
the same lengths (every engine path, long lines included), a transform type, a precision,
1-3 virtual ranks with random stick / plane distributions (empty ranks included) and an
exchange type, then the operator's own choices: kernel kind, scaling, weight, the optional
values output, a is b, host pointers on a GPU transform, forced exchange chunks and stick
blocks, a capped y/x intermediate, and multi_transform batches of three.

draw_case() holds every random choice and calls no library, so the coverage of a seed can
be judged without running anything; run_case() runs one drawn configuration.

    python tools/fuzz_ops.py --cases 400 [--op all|local|density|reciprocal|fock]
                             [--seed 1] [--max-elems 65536] [--pu gpu|host]

Every case makes two consecutive calls, checks the accumulating operators both as the whole
array and as the update alone, checks that the inputs are unchanged and, on a fused x plan,
that a sentinel-filled space domain stays bit-identical. Prints one line per case and the
largest error per operator and precision; exit status 1 on any failure.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fuzz_gpu import EXCHANGES, LONG, SHORT, draw_dims  # noqa: E402,F401

OPS = ("local", "density", "reciprocal", "fock")
SHIFT = (1, 2, 3)  # (s_x, s_y, s_z) of the translation kernel
PAD = 8  # y padding of one plane of the y/x intermediate (SPFFT_INTER_BYTES counts it)
# arrays of each operator that may be host pointers on a GPU transform
HOST_ARRAYS = {"local": ("values", "potential", "output"),
               "density": ("values", "rho"),
               "reciprocal": ("kernel", "values", "space"),
               "fock": ("a", "b", "kernel", "acc", "values")}
ENV = ("SPFFT_EXCH_CHUNKS", "SPFFT_EXCH_STICK_BLOCKS", "SPFFT_INTER_BYTES")


def draw_case(rng, op, max_elems):
    """Every random choice of one case, as a dict. No library call."""
    dims = draw_dims(rng, max_elems)
    r2c = bool(rng.random() < 0.4)
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
    kind = str(rng.choice(["real", "complex"]))
    full = bool(rng.random() < 0.5)
    weight = float(rng.choice([-1.0, 1.0]) * rng.uniform(0.25, 1.5))
    want_values = bool(rng.random() < 0.5)
    same = bool(rng.random() < 0.25)
    host_ptrs = []
    if rng.random() < 0.25:
        host_ptrs = [n for n in HOST_ARRAYS[op] if rng.random() < 0.5]
    chunks = int(rng.choice([0, 0, 2, 3]))  # 0: unset
    blocks = int(rng.choice([0, 0, 2]))
    if P == 1:
        chunks = blocks = 0
    cap_planes = int(rng.choice([1, 2])) if rng.random() < 0.2 else 0
    multi = P == 1 and op in ("local", "density") and bool(rng.random() < 0.25)
    if multi:
        host_ptrs = []
    return {"op": op, "dims": dims, "r2c": r2c, "single": single, "P": P, "exchange": exchange,
            "stick_dist": stick_dist, "plane_dist": plane_dist, "stick_fill": stick_fill,
            "z_fill": z_fill, "centred": centred, "kind": kind, "full": full, "weight": weight,
            "values": want_values, "same": same, "host_ptrs": host_ptrs, "chunks": chunks,
            "blocks": blocks, "cap_planes": cap_planes, "multi": multi,
            "data_seed": int(rng.integers(1 << 31))}


def fixed_case(op, dims, stick_dist=(1.0,), plane_dist=(1.0,), **choices):
    """A configuration written by hand (the pinned tests): C2C fp64 with the complex kernel,
    full scaling, the values output and no forced environment, unless `choices` says so."""
    cfg = {"op": op, "dims": tuple(dims), "r2c": False, "single": False, "P": len(stick_dist),
           "exchange": "COMPACT_BUFFERED", "stick_dist": [float(s) for s in stick_dist],
           "plane_dist": [float(p) for p in plane_dist], "stick_fill": 0.9, "z_fill": 0.8,
           "centred": False, "kind": "complex", "full": True, "weight": -0.75, "values": True,
           "same": False, "host_ptrs": [], "chunks": 0, "blocks": 0, "cap_planes": 0,
           "multi": False, "data_seed": 64}
    unknown = set(choices) - set(cfg)
    if unknown or len(plane_dist) != len(stick_dist):
        raise ValueError(f"fixed_case: {sorted(unknown) or 'one share per rank'}")
    cfg.update(choices)
    return cfg


def planes_of(cfg):
    """Local xy planes per rank of a drawn configuration."""
    from spfft_amd.utils.indices import calculate_num_local_xy_planes
    return [calculate_num_local_xy_planes(r, cfg["dims"][2], cfg["plane_dist"])
            for r in range(cfg["P"])]


def describe(cfg):
    d = (f"{cfg['op']}: dims={cfg['dims']} {'R2C' if cfg['r2c'] else 'C2C'} "
         f"{'fp32' if cfg['single'] else 'fp64'} P={cfg['P']} "
         f"{cfg['exchange'] if cfg['P'] > 1 else 'local'} sticks={cfg['stick_dist']} "
         f"planes={cfg['plane_dist']} fill={cfg['stick_fill']:.2f}/{cfg['z_fill']:.2f}")
    d += " centred" if cfg["centred"] else ""
    d += " full" if cfg["full"] else ""
    if cfg["op"] in ("reciprocal", "fock"):
        d += f" K={cfg['kind']}" + (" values" if cfg["values"] else "")
    if cfg["op"] in ("density", "fock"):
        d += f" w={cfg['weight']:.3f}"
    if cfg["op"] == "fock" and cfg["same"]:
        d += " a_is_b"
    if cfg["host_ptrs"]:
        d += " host:" + ",".join(cfg["host_ptrs"])
    if cfg["chunks"] or cfg["blocks"]:
        d += f" KxI={cfg['chunks'] or '-'}x{cfg['blocks'] or '-'}"
    if cfg["cap_planes"]:
        d += f" inter={cfg['cap_planes']}pl"
    d += " multi_transform x3" if cfg["multi"] else ""
    return d + f" seed={cfg['data_seed']}"


def _centred(idx, dims):
    idx = np.asarray(idx).reshape(-1, 3).astype(np.int64)
    return np.stack([np.where(idx[:, d] > dims[d] // 2, idx[:, d] - dims[d], idx[:, d])
                     for d in range(3)], axis=1)


def kernel_of(idx, dims, kind):
    """'real': Gaussian on centred G; 'complex': integer translation phase (|K| <= 1)."""
    g = _centred(idx, dims).astype(np.float64)
    if kind == "real":
        c = max(1.0, sum(n * n for n in dims) / 16.0)
        return np.exp(-(g ** 2).sum(axis=1) / c)
    ph = sum(g[:, d] * SHIFT[d] / dims[d] for d in range(3))
    return np.exp(-2j * np.pi * ph)


def _like(rng, ref):
    """Random start of an accumulated array, scaled to max|ref|, in ref's dtype class."""
    x = rng.uniform(-1, 1, ref.shape)
    if np.iscomplexobj(ref):
        x = x + 1j * rng.uniform(-1, 1, ref.shape)
    return x * (np.max(np.abs(ref)) if ref.size else 0.0)


def run_case(cfg, host=False):
    """Runs one drawn configuration. Returns (desc, err, tol, facts); facts holds one dict
    per rank: fused (the operator's x plan), r2c_fused (fock: the packed-real pair x
    stages of an R2C plan), reciprocal_fused, plan (exchange_plan() of a
    GPU transform), planes, values."""
    import spfft_amd as sp
    from spfft_amd.parallel import run_ranks
    from spfft_amd.utils.indices import create_value_indices
    from spfft_amd.utils.oracle import dense_backward, dense_forward, max_rel_error
    if not host:
        import torch

    op, dims, r2c, single, P = cfg["op"], cfg["dims"], cfg["r2c"], cfg["single"], cfg["P"]
    nx, ny, nz = dims
    exchange, kind, full, w = cfg["exchange"], cfg["kind"], cfg["full"], cfg["weight"]
    multi, hostp = cfg["multi"], set() if host else set(cfg["host_ptrs"])
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

    def field():
        """Unit variance, [z][y][x]."""
        if r2c:
            return rng.standard_normal((nz, ny, nx))
        return (rng.standard_normal((nz, ny, nx)) + 1j * rng.standard_normal((nz, ny, nx))) / np.sqrt(2)

    rdt = np.float32 if single else np.float64
    cdt = np.complex64 if single else np.complex128
    sdt = rdt if r2c else cdt  # of arrays over the space domain
    wide = np.float64 if r2c else np.complex128
    scaling = sp.Scaling.FULL if full else sp.Scaling.NONE
    k_all = kernel_of(all_idx, dims, kind).astype(rdt if kind == "real" else cdt)

    # inputs in working precision, oracles in double precision from those inputs
    f_in = field().astype(sdt)
    if op in ("local", "density"):
        # values of a real-space field (consistent R2C input), unit variance
        vals = (dense_forward(f_in.astype(wide), all_idx, dims, r2c=r2c) / np.sqrt(N)).astype(cdt)
        psi = dense_backward(all_idx, vals.astype(np.complex128), dims, r2c=r2c)
    if op == "local":
        pot = (0.5 + rng.random((nz, ny, nx))).astype(rdt)
        want = dense_forward(psi * pot.astype(np.float64), all_idx, dims, r2c=r2c, scale=full)
    elif op == "density":
        upd = w * (np.abs(psi) ** 2)
        start = _like(rng, upd).astype(rdt)
    elif op == "reciprocal":
        wvals = dense_forward(f_in.astype(wide), all_idx, dims, r2c=r2c, scale=full)
        want = dense_backward(all_idx, k_all.astype(np.complex128) * wvals, dims, r2c=r2c)
    else:
        a_in = f_in
        b_in = a_in if cfg["same"] else field().astype(sdt)
        a64, b64 = a_in.astype(wide), b_in.astype(wide)
        wvals = dense_forward(np.conj(a64) * b64, all_idx, dims, r2c=r2c, scale=full)
        upd = w * a64 * dense_backward(all_idx, k_all.astype(np.complex128) * wvals, dims, r2c=r2c)
        start = _like(rng, upd).astype(sdt)

    ttype = sp.TransformType.R2C if r2c else sp.TransformType.C2C
    PU = sp.ProcessingUnit.HOST if host else sp.ProcessingUnit.GPU
    nthreads = 2 if host else 1
    G = sp.GridFloat if single else sp.Grid
    tol = 2e-4 if (single or (P > 1 and exchange.endswith("FLOAT"))) else 1e-10
    fused_flag = {"local": "apply_local_fused", "density": "density_fused",
                  "reciprocal": "reciprocal_fused", "fock": "fock_fused"}[op]
    # the pair operator's packed-real x stages on R2C plans have a flag of their own
    r2c_flag = "fock_r2c_fused" if op == "fock" else None

    def arr(x, name):
        """Argument array: numpy on the host engine or for a host pointer, else a GPU tensor."""
        x = np.ascontiguousarray(x)
        if host or name in hostp:
            return x.copy()
        y = torch.as_tensor(x, device="cuda")  # (a copy: x is host memory)
        torch.cuda.synchronize()
        return y

    def npy(y):
        return y if isinstance(y, np.ndarray) else y.cpu().numpy()

    def same_bits(x, ref):
        return npy(x).tobytes() == np.ascontiguousarray(ref).tobytes()

    def facts_of(t, rank):
        return {"fused": bool(getattr(t, fused_flag)), "reciprocal_fused": bool(t.reciprocal_fused),
                "r2c_fused": bool(r2c_flag and getattr(t, r2c_flag)),
                "plan": None if host else t.exchange_plan(), "planes": int(planes[rank]),
                "values": int(len(parts[rank]))}

    def sentinel_of(t):
        """Fills the space domain of a fused x plan with a sentinel; returns its check."""
        if host or op == "reciprocal" or not (getattr(t, fused_flag) or (r2c_flag and getattr(t, r2c_flag))):
            return lambda: True
        space = t.space_domain(PU)
        space.fill_(-7.25)
        before = space.cpu().numpy().tobytes()
        return lambda: space.cpu().numpy().tobytes() == before

    def accumulated(call, fetch, start_r, upd_r, factor=1.0):
        """Two consecutive calls: the whole array and the array minus its start."""
        errs = []
        s64 = start_r.astype(upd_r.dtype)
        for n in (1, 2):
            call()
            got = npy(fetch()).astype(upd_r.dtype)
            errs.append(max_rel_error(got, s64 + n * factor * upd_r))
            errs.append(max_rel_error(got - s64, n * factor * upd_r))
        return errs

    def body(rank, comm):
        if not host:
            torch.cuda.set_device(0)
        if P == 1:
            grid = G(nx, ny, nz, nx * ny, PU, nthreads)
        else:
            ms = max(len(np.unique(p[:, 0].astype(np.int64) * ny + p[:, 1])) if len(p) else 0 for p in parts)
            grid = G(nx, ny, nz, max(1, ms), PU, nthreads, max_local_z_length=max(planes),
                     comm=comm, exchange_type=getattr(sp.ExchangeType, exchange))
        t = grid.create_transform(PU, ttype, nx, ny, nz, planes[rank], parts[rank])
        z = slice(offsets[rank], offsets[rank + 1])
        g = slice(starts[rank], starts[rank + 1])
        nvals = len(parts[rank])
        untouched = sentinel_of(t)
        errs = []
        if op == "local":
            v, p = arr(vals[g], "values"), arr(pot[z], "potential")
            for _ in range(2):
                out = arr(np.full(nvals, -1, dtype=cdt), "output")
                ret = t.apply_local(v, p, output=out, scaling=scaling)
                errs.append(max_rel_error(npy(out), want[g]) if ret is out else float("inf"))
            ok = same_bits(v, vals[g]) and same_bits(p, pot[z])
        elif op == "density":
            v, rho = arr(vals[g], "values"), arr(start[z], "rho")
            errs += accumulated(lambda: t.accumulate_density(v, w, rho), lambda: rho, start[z], upd[z])
            ok = same_bits(v, vals[g])
        elif op == "reciprocal":
            k = arr(k_all[g], "kernel")
            loc = sp.ProcessingUnit.HOST if (host or "space" in hostp) else PU
            slab = arr(f_in[z], "space")
            for _ in range(2):
                out = arr(np.full(nvals, -1, dtype=cdt), "values") if cfg["values"] else None
                got = t.apply_reciprocal(k, space=slab, values=out, location=loc, scaling=scaling)
                errs.append(max_rel_error(npy(got), want[z]))
                if out is not None:
                    errs.append(max_rel_error(npy(out), wvals[g]))
            ok = same_bits(k, k_all[g]) and same_bits(slab, f_in[z])
        else:
            k = arr(k_all[g], "kernel")
            a = arr(a_in[z], "a")
            b = a if cfg["same"] else arr(b_in[z], "b")
            acc = arr(start[z], "acc")
            out = arr(np.full(nvals, -1, dtype=cdt), "values") if cfg["values"] else None
            errs += accumulated(lambda: t.accumulate_fock(a, b, k, w, acc, values=out, scaling=scaling),
                                lambda: acc, start[z], upd[z])
            if out is not None:
                errs.append(max_rel_error(npy(out), wvals[g]))
            ok = same_bits(k, k_all[g]) and same_bits(a, a_in[z]) and same_bits(b, b_in[z])
        if not ok:
            errs.append(float("inf"))  # an input changed
        if not untouched():
            errs.append(float("inf"))  # a fused x plan wrote the space domain
        return max(errs), facts_of(t, rank)

    FACTORS = (1.0, -0.5, 2.0)  # of the three inputs of a multi_transform call

    def multi_body():
        # three transforms of the same problem on their own grids, one multi_transform call
        ts = []
        for _ in range(3):
            grid = G(nx, ny, nz, nx * ny, PU, nthreads)
            ts.append((grid, grid.create_transform(PU, ttype, nx, ny, nz, nz, parts[0])))
        tr = [t for _, t in ts]
        checks = [sentinel_of(t) for t in tr]
        ins = [arr(c * vals, "values") for c in FACTORS]
        errs = []
        if op == "local":
            p = arr(pot, "potential")
            for _ in range(2):
                outs = sp.multi_transform_apply_local(tr, ins, [p] * 3, scalings=[scaling] * 3)
                errs += [max_rel_error(npy(o), c * want) for o, c in zip(outs, FACTORS)]
            ok = same_bits(p, pot)
        else:
            rho = arr(start, "rho")
            ws = [w, 0.5 * w, -0.25 * w]
            total = sum(x / w * c * c for x, c in zip(ws, FACTORS))
            errs += accumulated(lambda: sp.multi_transform_accumulate_density(tr, ins, ws, rho),
                                lambda: rho, start, upd, total)
            ok = True
        ok = ok and all(same_bits(i, (c * vals).astype(cdt)) for i, c in zip(ins, FACTORS))
        if not ok or not all(c() for c in checks):
            errs.append(float("inf"))
        return max(errs), facts_of(tr[0], 0)

    # the library reads these when a grid or transform is created
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
        if multi:
            results = [multi_body()]
        else:
            results = [body(0, None)] if P == 1 else run_ranks(P, body)
    finally:
        for n, v in saved.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
    return describe(cfg), max(e for e, _ in results), tol, [f for _, f in results]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", choices=("all",) + OPS, default="all")
    ap.add_argument("--cases", type=int, default=100, help="in all, shared by the operators in turn")
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
