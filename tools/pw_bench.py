"""Plane-wave workload throughput on one GPU: H_loc psi for many bands
(PlaneWaveModel.apply_local_potential: one apply_local per band, num_transforms
bands per multi_transform call). Prints one JSON line.

    python tools/pw_bench.py --ecut 20 --alat 10 --bands 64 --transforms 8
(SPFFT_BATCH=0 in the environment disables batched launches for comparison;
--unfused times the composition backward, V(r) multiply, forward instead of the
fused apply_local; --op density times PlaneWaveModel.density, rho = sum_b w_b
|psi_b|^2 with one accumulate_density per band, and with --unfused today's
composition of backward and torch passes; --op hartree times
PlaneWaveModel.hartree_potential, one apply_reciprocal per call, against its
composition forward, K(G) multiply, backward in alternating rounds of one
process, and prints the GPU stage times of both and the modelled bytes of the two
z stages; with --r2c on an R2C transform; --op local / density with --r2c time
--transforms bands per call on R2C transforms over the hermitian half of the sphere,
three variants in alternating rounds of one process: multi_transform_backward, torch
passes and multi_transform_forward; the library's composed path (transforms created under
SPFFT_R2C_FUSE=0); the fused call; --op fock times one exchange pair,
accumulate_fock on the model's pair-density transform (the sphere |G|^2/2 <= 4
ecut) against torch product, apply_reciprocal, torch addcmul_, with the same
protocol and the modelled bytes of both; with --transforms T > 1 it times T
pairs of one band per multi_transform_accumulate_fock call against the same T
pairs as T single accumulate_fock calls into one acc, pairs per second of both;
with --r2c it times T pairs of real fields into one acc on R2C transforms over the
hermitian half of the pair sphere, three variants in alternating rounds of one
process: the torch composition (product, apply_reciprocal, addcmul_), the
library's composed path (transforms created under SPFFT_R2C_FUSE=0) and the
fused call, with the stage times of both library variants;
--op gradient / divergence times PlaneWaveModel's three-component gradient and
divergence on the density sphere, one multi_transform_reciprocal_fan_out / fan_in
call against three apply_reciprocal calls with their copies and against the best
composition of forward, multiply and backward, with --r2c on R2C transforms;
--op tau / mgga times the kinetic-energy density and the local meta-GGA operator
of one band on the wavefunction sphere, one multi_transform_accumulate_density_fan
/ multi_transform_apply_local_fan call against the best composition of torch
multiplies and multi_transform_accumulate_density / multi_transform_apply_local;
--op spinor / spin_density times the 2x2 local potential on two-component spinors
and their spin density matrix, --transforms spinors (1 to 4) per
multi_transform_apply_local_spinor / multi_transform_accumulate_spin_density call
against multi_transform_backward, torch passes over the space domains and
multi_transform_forward, and for the operator also against six apply_local
members per spinor.)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ecut", type=float, default=20.0)
    ap.add_argument("--alat", type=float, default=10.0)
    ap.add_argument("--bands", type=int, default=64)
    ap.add_argument("--transforms", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--unfused", action="store_true")
    ap.add_argument("--op", choices=("local", "density", "hartree", "fock", "gradient", "divergence",
                                     "tau", "mgga", "spinor", "spin_density"), default="local")
    ap.add_argument("--grid", type=int, default=0,
                    help="FFT grid N^3 instead of the density grid of the cutoff (the cutoff "
                         "sphere may then reach N/2, the transforms' own minimum grid)")
    ap.add_argument("--r2c", action="store_true",
                    help="--op hartree, local, density, fock, gradient, divergence on R2C transforms "
                         "(hermitian half of the sphere)")
    a = ap.parse_args()
    import torch

    import spfft_amd as sp
    from spfft_amd.models import PlaneWaveBasis, PlaneWaveModel
    basis = PlaneWaveBasis(alat=a.alat, ecut=a.ecut,
                           fft_dims=(a.grid,) * 3 if a.grid else None)
    model = PlaneWaveModel(basis, processing_unit=sp.ProcessingUnit.GPU,
                           num_transforms=1 if a.op in ("fock", "gradient", "divergence", "tau", "mgga",
                                                        "spinor", "spin_density")
                           else a.transforms)
    if a.op in ("spinor", "spin_density"):
        spinor(a, basis, model)
        return
    if a.op in ("tau", "mgga"):
        values_fan(a, basis, model)
        return
    if a.op in ("gradient", "divergence"):
        fan(a, basis, model)
        return
    if a.op == "fock":
        if a.r2c:
            fock_r2c(a, basis, model)
        elif a.transforms > 1:
            fock_multi(a, basis, model)
        else:
            fock(a, basis, model)
        return
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    psi = [torch.randn(basis.num_pw, dtype=torch.complex128, device=dev, generator=g)
           for _ in range(a.bands)]
    nx, ny, nz = basis.fft_dims
    v_r = torch.rand((nz, ny, nx), dtype=torch.float64, device=dev, generator=g)
    if a.op == "hartree":
        hartree(a, basis, model, v_r)  # (a real field stands in for rho)
        return
    if a.r2c:
        r2c_ops(a, basis, v_r)
        return
    if a.op == "density":
        weights = [1.0 + 0.01 * b for b in range(a.bands)]

        def step():
            return model.density(psi, weights, unfused=a.unfused)
    else:
        def step():
            return model.apply_local_potential(psi, v_r, unfused=a.unfused)
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if a.op == "density":
        print(json.dumps({"workload": "plane-wave density", "fft_dims": list(basis.fft_dims),
                          "num_pw": basis.num_pw, "bands": a.bands, "transforms": a.transforms,
                          "batch": os.environ.get("SPFFT_BATCH", "1"),
                          "path": "unfused" if a.unfused else "accumulate_density",
                          "bands_per_s": a.bands * a.reps / dt}), flush=True)
        return
    print(json.dumps({"workload": "plane-wave H_loc psi", "fft_dims": list(basis.fft_dims),
                      "num_pw": basis.num_pw, "bands": a.bands, "transforms": a.transforms,
                      "batch": os.environ.get("SPFFT_BATCH", "1"),
                      "path": "unfused" if a.unfused else "apply_local",
                      "bands_per_s": a.bands * a.reps / dt,
                      "transforms_per_s": 2 * a.bands * a.reps / dt}), flush=True)


def _gpu_stage_medians(tree):
    """gpu/<direction>/<stage> -> median seconds, from the native timing tree."""
    out = {}
    for n in tree["timings"]:
        if n["identifier"] != "gpu":
            continue
        for d in n["sub-timings"]:
            for st in d["sub-timings"]:
                out[d["identifier"] + "/" + st["identifier"]] = st["median"]
    return out


def _hermitian_half(basis):
    """The half of the model's sphere an R2C transform takes: x >= 0, and of the x = 0
    plane y >= 0 (of the (0,0) stick z >= 0)."""
    import numpy as np
    idx = basis.indices
    keep = (idx[:, 0] > 0) | ((idx[:, 0] == 0) & ((idx[:, 1] > 0) |
                                                 ((idx[:, 1] == 0) & (idx[:, 2] >= 0))))
    return np.ascontiguousarray(idx[keep])


def r2c_ops(a, basis, v_r):
    """--op local / density --r2c: B = --transforms bands per call on R2C transforms over
    the hermitian half of the sphere. Variants, alternating in one process (medians over the
    rounds): "torch" multi_transform_backward, torch passes over the real space domains,
    (multi_transform_forward); "composed" the library's composed path on transforms created
    under SPFFT_R2C_FUSE=0; "fused" the call on the default plan. Then the GPU stage medians
    of the single-transform call of each library variant, and the byte model of the x part
    (columns c = nx/2+1 of ny rows per plane, 16 B per element, real rows of nx * 8 B)."""
    import numpy as np
    import torch

    import spfft_amd as sp
    nx, ny, nz = basis.fft_dims
    idx = _hermitian_half(basis)
    B = max(1, a.transforms)

    def make(env):
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            ts = []
            for _ in range(B):
                grid = sp.Grid(nx, ny, nz, nx * ny, sp.ProcessingUnit.GPU, 1)
                ts.append(grid.create_transform(sp.ProcessingUnit.GPU, sp.TransformType.R2C,
                                                nx, ny, nz, nz, idx))
            return ts
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    fused_ts, composed_ts = make({}), make({"SPFFT_R2C_FUSE": "0"})
    # hermitian-consistent values: the forward transform of real fields
    g = torch.Generator(device="cuda")
    g.manual_seed(6)
    psi = []
    for _ in range(B):
        f = torch.randn((nz, ny, nx), dtype=torch.float64, device="cuda", generator=g)
        psi.append(fused_ts[0].forward(space=f, scaling=sp.Scaling.FULL).clone())
    weights = [1.0 + 0.01 * b for b in range(B)]
    rho = torch.zeros((nz, ny, nx), dtype=torch.float64, device="cuda")
    pots = [v_r] * B
    density = a.op == "density"

    def call(variant):
        if variant == "torch":
            spaces = sp.multi_transform_backward(fused_ts, psi)
            if density:
                for s, w in zip(spaces, weights):
                    rho.addcmul_(s, s, value=w)
                return rho
            for s in spaces:
                s.mul_(v_r)
            return sp.multi_transform_forward(fused_ts)
        ts = fused_ts if variant == "fused" else composed_ts
        if density:
            return sp.multi_transform_accumulate_density(ts, psi, weights, rho)
        return sp.multi_transform_apply_local(ts, psi, pots)

    variants = ("torch", "composed", "fused")
    rounds, calls = max(3, a.reps), 10
    times = {v: [] for v in variants}
    for v in variants:
        call(v)
    for _ in range(rounds):
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call(v)
            torch.cuda.synchronize()
            times[v].append((time.perf_counter() - t0) / calls)
    med = {v: sorted(x)[len(x) // 2] for v, x in times.items()}
    stages = {}
    for v, ts in (("composed", composed_ts), ("fused", fused_ts)):
        sp.timing_reset()
        sp.timing_enable(True)
        try:
            for _ in range(calls):
                if density:
                    ts[0].accumulate_density(psi[0], 1.0, rho)
                else:
                    ts[0].apply_local(psi[0], v_r)
            ts[0].synchronize()
            torch.cuda.synchronize()
            stages[v] = _gpu_stage_medians(sp.timing_json())
        finally:
            sp.timing_enable(False)
    inter, real = (nx // 2 + 1) * ny * nz * 16, nx * ny * nz * 8
    if density:
        model = {"composed": inter + real + 3 * real, "fused": inter + 2 * real}
    else:
        model = {"composed": (inter + real) + 3 * real + (real + inter), "fused": 2 * inter + real}
    best = min(med["torch"], med["composed"])
    print(json.dumps({"workload": "plane-wave " + ("density" if density else "H_loc psi"), "type": "r2c",
                      "fft_dims": list(basis.fft_dims), "num_values": int(len(idx)), "bands_per_call": B,
                      "fused": bool(fused_ts[0].density_fused if density else fused_ts[0].apply_local_fused),
                      "us_per_call": {v: 1e6 * x for v, x in med.items()},
                      "range_us": {v: [1e6 * min(x), 1e6 * max(x)] for v, x in times.items()},
                      "ratio_best_other_over_fused": best / med["fused"],
                      "gpu_stage_median_s": stages,
                      "model_x_bytes": model,
                      "model_x_ratio": model["composed"] / model["fused"]}), flush=True)


def hartree(a, basis, model, rho):
    """Fused and composed calls in alternating rounds of one process (medians over the
    rounds), then the GPU stage times of each variant from the timing tree. --r2c runs
    the same operator on an R2C transform over the hermitian half of the model's sphere
    (the hermitian fill of the (0,0) stick runs inside the fused kernel)."""
    import numpy as np
    import torch

    import spfft_amd as sp
    nx, ny, nz = basis.fft_dims
    if a.r2c:
        idx = basis.indices
        # the half the R2C transform takes: x >= 0, and of the x = 0 plane y >= 0 (of the
        # (0,0) stick z >= 0)
        keep = (idx[:, 0] > 0) | ((idx[:, 0] == 0) & ((idx[:, 1] > 0) |
                                                     ((idx[:, 1] == 0) & (idx[:, 2] >= 0))))
        idx, g2 = np.ascontiguousarray(idx[keep]), basis.g2[keep]
        grid = sp.Grid(nx, ny, nz, nx * ny, sp.ProcessingUnit.GPU, 1)
        t = grid.create_transform(sp.ProcessingUnit.GPU, sp.TransformType.R2C, nx, ny, nz, nz, idx)
        k = torch.as_tensor(np.where(g2 > 0, 4 * np.pi / np.where(g2 > 0, g2, 1.0), 0.0), device="cuda")

        def call(unfused):
            if not unfused:
                return t.apply_reciprocal(k, space=rho, scaling=sp.Scaling.FULL).clone()
            c = t.forward(space=rho, scaling=sp.Scaling.FULL)
            c.mul_(k)
            return t.backward(c).clone()
    else:
        idx = basis.indices
        t = model.transforms[0]

        def call(unfused):
            return model.hartree_potential(rho, unfused=unfused)
    rounds, calls = max(3, a.reps), 20
    times = {"fused": [], "composed": []}
    for unfused in (False, True):
        call(unfused)
    for _ in range(rounds):
        for name, unfused in (("fused", False), ("composed", True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call(unfused)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / calls)
    med = {k_: sorted(v)[len(v) // 2] for k_, v in times.items()}
    stages = {}
    for name, unfused in (("fused", False), ("composed", True)):
        sp.timing_reset()
        sp.timing_enable(True)
        try:
            for _ in range(calls):
                call(unfused)
            t.synchronize()
            torch.cuda.synchronize()
            stages[name] = _gpu_stage_medians(sp.timing_json())
        finally:
            sp.timing_enable(False)
    key = idx[:, 0].astype("int64") * (2 * ny + 1) + idx[:, 1]
    sticks = len(set(key.tolist()))
    stick_bytes, value_bytes = sticks * nz * 16, len(idx) * 16
    # z stages only: composed reads and writes the sticks and the values once per
    # direction and multiplies the values in between (with a real K);
    # fused reads and writes the sticks once and reads K
    print(json.dumps({"workload": "plane-wave Hartree potential", "type": "r2c" if a.r2c else "c2c",
                      "fft_dims": list(basis.fft_dims),
                      "num_values": len(idx), "sticks": sticks,
                      "reciprocal_fused": t.reciprocal_fused,
                      "calls_per_s": {k_: 1.0 / v for k_, v in med.items()},
                      "min_s": {k_: min(v) for k_, v in times.items()},
                      "ratio_composed_over_fused": med["composed"] / med["fused"],
                      "gpu_stage_median_s": stages,
                      "model_z_bytes": {"composed": 2 * stick_bytes + 4 * value_bytes + value_bytes // 2,
                                        "fused": 2 * stick_bytes + value_bytes // 2}}), flush=True)


def fock(a, basis, model):
    """One exchange pair (a, b) on the model's pair-density transform: accumulate_fock
    against its composition (torch product into the space domain, apply_reciprocal, torch
    addcmul_) in alternating rounds of one process (medians over the rounds), then the
    GPU stage times of each variant from the timing tree, and the modelled bytes."""
    import torch

    import spfft_amd as sp
    nx, ny, nz = basis.fft_dims
    t = model.exchange_transform
    idx = model.exchange_indices
    k = model._exchange_setup()[3]
    g = torch.Generator(device="cuda")
    g.manual_seed(6)
    shape = (nz, ny, nx)
    pa, pb = (torch.randn(shape, dtype=torch.complex128, device="cuda", generator=g) for _ in range(2))
    acc = torch.zeros(shape, dtype=torch.complex128, device="cuda")
    space = t.space_domain(sp.ProcessingUnit.GPU)

    def call(unfused):
        if not unfused:
            return t.accumulate_fock(pa, pb, k, -1.0, acc, scaling=sp.Scaling.FULL)
        torch.mul(pa.conj(), pb, out=space)  # the product written into the space domain
        u = t.apply_reciprocal(k, scaling=sp.Scaling.FULL)
        return acc.addcmul_(pa, u, value=-1.0)
    rounds, calls = max(3, a.reps), 20
    times = {"fused": [], "composed": []}
    for unfused in (False, True):
        call(unfused)
    for _ in range(rounds):
        for name, unfused in (("fused", False), ("composed", True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call(unfused)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / calls)
    med = {k_: sorted(v)[len(v) // 2] for k_, v in times.items()}
    stages = {}
    for name, unfused in (("fused", False), ("composed", True)):
        sp.timing_reset()
        sp.timing_enable(True)
        try:
            for _ in range(calls):
                call(unfused)
            t.synchronize()
            torch.cuda.synchronize()
            stages[name] = _gpu_stage_medians(sp.timing_json())
        finally:
            sp.timing_enable(False)
    key = idx[:, 0].astype("int64") * (2 * ny + 1) + idx[:, 1]
    sticks = len(set(key.tolist()))
    columns = len(set(idx[:, 0].tolist()))
    grid_bytes = nx * ny * nz * 16
    # apply_reciprocal itself: the space domain read and written once, the [z][column][y]
    # intermediate and the stick array written and read once per direction, K read
    inter_bytes, stick_bytes = columns * ny * nz * 16, sticks * nz * 16
    reciprocal = 2 * grid_bytes + 4 * inter_bytes + 4 * stick_bytes + len(idx) * 8
    # composed: product (read 2, write 1) and addcmul_ (read 3, write 1) on top; fused: a
    # and b instead of the space domain forward, a and acc read and acc written instead of
    # the space domain backward
    model_bytes = {"composed": reciprocal + 7 * grid_bytes, "fused": reciprocal + 3 * grid_bytes}
    print(json.dumps({"workload": "plane-wave exchange pair", "fft_dims": list(basis.fft_dims),
                      "num_values": len(idx), "sticks": sticks,
                      "fock_fused": t.fock_fused, "reciprocal_fused": t.reciprocal_fused,
                      "calls_per_s": {k_: 1.0 / v for k_, v in med.items()},
                      "min_s": {k_: min(v) for k_, v in times.items()},
                      "ratio_composed_over_fused": med["composed"] / med["fused"],
                      "gpu_stage_median_s": stages,
                      "model_bytes": model_bytes,
                      "model_ratio": model_bytes["composed"] / model_bytes["fused"]}), flush=True)


def _scope_medians(tree, names):
    """identifier -> median seconds of the named host scopes, wherever they sit in the tree."""
    out = {}

    def walk(nodes):
        for n in nodes:
            if n["identifier"] in names:
                out[n["identifier"]] = n["median"]
            walk(n.get("sub-timings", []))

    walk(tree["timings"])
    return out


def fock_multi(a, basis, model):
    """T = --transforms exchange pairs (a_i, b) of one band b into one acc: one
    multi_transform_accumulate_fock call on the pair-density transform and its clones
    against the same T pairs as T single accumulate_fock calls, in alternating rounds of
    one process (medians over at least 7 rounds, per pair), then the timing tree of each
    variant (GPU stage times of the single calls, which mark their stages; host scopes of
    both) and the modelled bytes per pair."""
    import torch

    import spfft_amd as sp
    nx, ny, nz = basis.fft_dims
    T = a.transforms
    ts = model._exchange_transforms(T)
    t = ts[0]
    idx = model.exchange_indices
    k = model._exchange_setup()[3]
    g = torch.Generator(device="cuda")
    g.manual_seed(6)
    shape = (nz, ny, nx)
    pas = [torch.randn(shape, dtype=torch.complex128, device="cuda", generator=g) for _ in range(T)]
    pb = torch.randn(shape, dtype=torch.complex128, device="cuda", generator=g)
    acc = torch.zeros(shape, dtype=torch.complex128, device="cuda")
    weights = [-1.0 - 0.125 * i for i in range(T)]

    def call(multi):
        if multi:
            return sp.multi_transform_accumulate_fock(ts, pas, [pb] * T, k, weights, acc,
                                                      scaling=sp.Scaling.FULL)
        for pa, w in zip(pas, weights):
            t.accumulate_fock(pa, pb, k, w, acc, scaling=sp.Scaling.FULL)
        return acc
    rounds, calls = max(7, a.reps), max(2, 20 // T)
    times = {"multi": [], "single": []}
    for multi in (True, False):
        call(multi)
    for _ in range(rounds):
        for name, multi in (("multi", True), ("single", False)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call(multi)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / (calls * T))
    med = {k_: sorted(v)[len(v) // 2] for k_, v in times.items()}
    stages, scopes = {}, {}
    for name, multi in (("multi", True), ("single", False)):
        sp.timing_reset()
        sp.timing_enable(True)
        try:
            for _ in range(calls):
                call(multi)
            torch.cuda.synchronize()
            tree = sp.timing_json()
            stages[name] = _gpu_stage_medians(tree)
            scopes[name] = _scope_medians(tree, {"multi_accumulate_fock", "accumulate_fock",
                                                 "gpu_accumulate_fock_batch", "gpu_fock_forward_xy",
                                                 "gpu_reciprocal_z", "gpu_fock_backward_xy"})
        finally:
            sp.timing_enable(False)
    key = idx[:, 0].astype("int64") * (2 * ny + 1) + idx[:, 1]
    sticks = len(set(key.tolist()))
    columns = len(set(idx[:, 0].tolist()))
    grid_bytes = nx * ny * nz * 16
    inter_bytes, stick_bytes = columns * ny * nz * 16, sticks * nz * 16
    # per pair, both variants: the intermediate and the stick array written and read once
    # per direction, K read, a read by either x stage. A single call also reads b and
    # reads and writes acc; a batch reads b and reads and writes acc once for its T pairs
    # (the members' revisits of a tile stay in the caches).
    common = 4 * inter_bytes + 4 * stick_bytes + len(idx) * 8 + 2 * grid_bytes
    model_bytes = {"single": common + 3 * grid_bytes, "multi": common + 3 * grid_bytes / T}
    print(json.dumps({"workload": "plane-wave exchange pairs", "fft_dims": list(basis.fft_dims),
                      "pairs_per_call": T, "num_values": len(idx), "sticks": sticks,
                      "batch": os.environ.get("SPFFT_BATCH", "1"),
                      "fock_fused": t.fock_fused, "reciprocal_fused": t.reciprocal_fused,
                      "rounds": rounds, "calls_per_round": calls,
                      "pairs_per_s": {k_: 1.0 / v for k_, v in med.items()},
                      "min_s_per_pair": {k_: min(v) for k_, v in times.items()},
                      "ratio_single_over_multi": med["single"] / med["multi"],
                      "gpu_stage_median_s": stages, "host_scope_median_s": scopes,
                      "model_bytes_per_pair": model_bytes,
                      "model_ratio": model_bytes["single"] / model_bytes["multi"]}), flush=True)


def fock_r2c(a, basis, model):
    """--op fock --r2c: T = --transforms exchange pairs (a_i, b) of real fields into one acc
    on R2C transforms over the hermitian half of the pair sphere. Variants, alternating in
    one process (medians and ranges over the rounds): "torch" the composition product into
    the space domain, apply_reciprocal, addcmul_, pair by pair; "composed" the library's
    composed path on transforms created under SPFFT_R2C_FUSE=0; "fused" the call on the
    default plans. Then the GPU stage medians of the single-pair call of each library
    variant, and the byte model of the x part per pair (G = nx ny nz 8 B, the real grid; I
    = columns ny nz 16 B, the intermediate): composed 9 G + 2 I (pair pass 3 G, R2C x stage
    G + I, C2R x stage I + G, accumulating pass 4 G), fused 5 G + 2 I."""
    import numpy as np
    import torch

    import spfft_amd as sp
    nx, ny, nz = basis.fft_dims
    full, khost = model.exchange_indices, model.exchange_kernel_host
    keep = (full[:, 0] > 0) | ((full[:, 0] == 0) & ((full[:, 1] > 0) |
                                                   ((full[:, 1] == 0) & (full[:, 2] >= 0))))
    idx = np.ascontiguousarray(full[keep])
    k = torch.as_tensor(np.ascontiguousarray(khost[keep]), device="cuda")
    T = max(1, a.transforms)

    def make(env):
        saved = {k_: os.environ.get(k_) for k_ in env}
        os.environ.update(env)
        try:
            ts = []
            for _ in range(T):
                grid = sp.Grid(nx, ny, nz, nx * ny, sp.ProcessingUnit.GPU, 1)
                ts.append(grid.create_transform(sp.ProcessingUnit.GPU, sp.TransformType.R2C,
                                                nx, ny, nz, nz, idx))
            return ts
        finally:
            for k_, v in saved.items():
                if v is None:
                    os.environ.pop(k_, None)
                else:
                    os.environ[k_] = v

    fused_ts, composed_ts = make({}), make({"SPFFT_R2C_FUSE": "0"})
    g = torch.Generator(device="cuda")
    g.manual_seed(6)
    shape = (nz, ny, nx)
    pas = [torch.randn(shape, dtype=torch.float64, device="cuda", generator=g) for _ in range(T)]
    pb = torch.randn(shape, dtype=torch.float64, device="cuda", generator=g)
    acc = torch.zeros(shape, dtype=torch.float64, device="cuda")
    weights = [-1.0 - 0.125 * i for i in range(T)]
    space = fused_ts[0].space_domain(sp.ProcessingUnit.GPU)

    def call(variant):
        if variant == "torch":
            for pa, w in zip(pas, weights):
                torch.mul(pa, pb, out=space)  # the product written into the space domain
                u = fused_ts[0].apply_reciprocal(k, scaling=sp.Scaling.FULL)
                acc.addcmul_(pa, u, value=w)
            return acc
        ts = fused_ts if variant == "fused" else composed_ts
        if T == 1:
            return ts[0].accumulate_fock(pas[0], pb, k, weights[0], acc, scaling=sp.Scaling.FULL)
        return sp.multi_transform_accumulate_fock(ts, pas, [pb] * T, k, weights, acc,
                                                  scaling=sp.Scaling.FULL)

    variants = ("torch", "composed", "fused")
    rounds, calls = max(3, a.reps), max(2, 10 // T)
    times = {v: [] for v in variants}
    for v in variants:
        call(v)
    for _ in range(rounds):
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call(v)
            torch.cuda.synchronize()
            times[v].append((time.perf_counter() - t0) / calls)
    med = {v: sorted(x)[len(x) // 2] for v, x in times.items()}
    stages = {}
    for v, ts in (("composed", composed_ts), ("fused", fused_ts)):
        sp.timing_reset()
        sp.timing_enable(True)
        try:
            for _ in range(10):
                ts[0].accumulate_fock(pas[0], pb, k, weights[0], acc, scaling=sp.Scaling.FULL)
            ts[0].synchronize()
            torch.cuda.synchronize()
            stages[v] = _gpu_stage_medians(sp.timing_json())
        finally:
            sp.timing_enable(False)
    columns = len(set(idx[:, 0].tolist()))
    inter, real = columns * ny * nz * 16, nx * ny * nz * 8
    model_x = {"composed": 9 * real + 2 * inter, "fused": 5 * real + 2 * inter}
    best = min(med["torch"], med["composed"])
    t = fused_ts[0]
    print(json.dumps({"workload": "plane-wave exchange pairs", "type": "r2c",
                      "fft_dims": list(basis.fft_dims), "num_values": int(len(idx)), "columns": columns,
                      "pairs_per_call": T, "batch": os.environ.get("SPFFT_BATCH", "1"),
                      "fock_r2c_fused": bool(t.fock_r2c_fused), "reciprocal_fused": bool(t.reciprocal_fused),
                      "rounds": rounds, "calls_per_round": calls,
                      "us_per_call": {v: 1e6 * x for v, x in med.items()},
                      "range_us": {v: [1e6 * min(x), 1e6 * max(x)] for v, x in times.items()},
                      "ratio_best_other_over_fused": best / med["fused"],
                      "gpu_stage_median_s": stages,
                      "model_x_bytes_per_pair": model_x,
                      "model_x_ratio": model_x["composed"] / model_x["fused"]}), flush=True)


def fan(a, basis, model):
    """--op gradient / divergence: the three components on the density sphere (the
    pair-density transform and two clones; --r2c: R2C transforms over its hermitian half)
    with K_d = i G_d and full scaling, three variants in alternating rounds of one process
    (medians over at least 7 rounds):
      fused     one multi_transform_reciprocal_fan_out / fan_in call;
      single    three apply_reciprocal calls with the copies they need (the field copied in
                per call; gradient: each result cloned out; divergence: the results summed
                on the grid);
      composed  the best composition of the existing calls: gradient, one forward, then per
                component multiply, backward and clone; divergence, three forwards, the
                multiply-add of the values, one backward.
    Prints calls per second, the ratios against `fused`, the host scopes of the fused call
    and the modelled bytes of every variant (G grid array, I intermediate, S stick array, V
    values, K kernel; a forward or backward y+x pass G + 2 I + S, a fused z stage 2 S + K, a
    z stage S + V, a grid copy 2 G)."""
    import numpy as np
    import torch

    import spfft_amd as sp
    nx, ny, nz = basis.fft_dims
    idx = model.exchange_indices
    unit = 2 * np.pi / basis.alat
    if a.r2c:
        keep = (idx[:, 0] > 0) | ((idx[:, 0] == 0) & ((idx[:, 1] > 0) |
                                                     ((idx[:, 1] == 0) & (idx[:, 2] >= 0))))
        idx = np.ascontiguousarray(idx[keep])
        grid = sp.Grid(nx, ny, nz, nx * ny, sp.ProcessingUnit.GPU, 1)
        t0 = grid.create_transform(sp.ProcessingUnit.GPU, sp.TransformType.R2C, nx, ny, nz, nz, idx)
        ts = [t0, t0.clone(), t0.clone()]
    else:
        ts = model._exchange_transforms(3)
    t = ts[0]
    ks = [torch.as_tensor(1j * unit * idx[:, d].astype(np.float64), device="cuda") for d in range(3)]
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    dtype = torch.float64 if a.r2c else torch.complex128
    f = torch.randn((nz, ny, nx), dtype=dtype, device="cuda", generator=g)
    hs = [torch.randn((nz, ny, nx), dtype=dtype, device="cuda", generator=g) for _ in range(3)]
    full = sp.Scaling.FULL
    gradient = a.op == "gradient"

    def call(variant):
        if gradient:
            if variant == "fused":
                return sp.multi_transform_reciprocal_fan_out(ts, ks, space=f, scaling=full)
            if variant == "single":
                return [t.apply_reciprocal(k, space=f, scaling=full).clone() for k in ks]
            c = t.forward(space=f, scaling=full)
            return [t.backward(c * k).clone() for k in ks]
        if variant == "fused":
            return sp.multi_transform_reciprocal_fan_in(ts, ks, spaces=hs, scaling=full)
        if variant == "single":
            acc = None
            for h, k in zip(hs, ks):
                out = t.apply_reciprocal(k, space=h, scaling=full)
                acc = out.clone() if acc is None else acc.add_(out)
            return acc
        s = None
        for h, k in zip(hs, ks):
            c = t.forward(space=h, scaling=full)
            s = c * k if s is None else torch.addcmul(s, c, k)
        return t.backward(s)
    variants = ("fused", "single", "composed")
    rounds, calls = max(7, a.reps), 10
    times = {v: [] for v in variants}
    for v in variants:
        call(v)
    for r in range(rounds):
        for v in (variants if r % 2 == 0 else variants[::-1]):  # mirrored orders
            torch.cuda.synchronize()
            t0_ = time.perf_counter()
            for _ in range(calls):
                call(v)
            torch.cuda.synchronize()
            times[v].append((time.perf_counter() - t0_) / calls)
    med = {v: sorted(x)[len(x) // 2] for v, x in times.items()}
    sp.timing_reset()
    sp.timing_enable(True)
    try:
        for _ in range(calls):
            call("fused")
        torch.cuda.synchronize()
        scopes = _scope_medians(sp.timing_json(), {
            "multi_reciprocal_fan_out", "multi_reciprocal_fan_in", "gpu_reciprocal_fan_out_batch",
            "gpu_reciprocal_fan_in_batch"})
    finally:
        sp.timing_enable(False)
    key = idx[:, 0].astype("int64") * (2 * ny + 1) + idx[:, 1]
    sticks = len(set(key.tolist()))
    columns = len(set(idx[:, 0].tolist()))
    G = nx * ny * nz * (8 if a.r2c else 16)
    I, S, V = columns * ny * nz * 16, sticks * nz * 16, len(idx) * 16
    K = V
    xy = G + 2 * I + S
    if gradient:
        model_bytes = {"fused": 2 * G + xy + (4 * S + 3 * K) + 3 * xy,
                       "single": 3 * (2 * G + xy + (2 * S + K) + xy + 2 * G),
                       "composed": 2 * G + xy + (S + V) + 3 * ((2 * V + K) + (V + S) + xy + 2 * G)}
    else:
        model_bytes = {"fused": 3 * (2 * G + xy) + (4 * S + 3 * K) + xy,
                       "single": 3 * (2 * G + xy + (2 * S + K) + xy) + 2 * G + 2 * 3 * G,
                       "composed": 3 * (2 * G + xy + (S + V)) + 3 * (2 * V + K) + 2 * 3 * V + (V + S) + xy}
    print(json.dumps({"workload": "plane-wave " + a.op, "type": "r2c" if a.r2c else "c2c",
                      "fft_dims": list(basis.fft_dims), "num_values": len(idx), "sticks": sticks,
                      "batch": os.environ.get("SPFFT_BATCH", "1"),
                      "reciprocal_fused": t.reciprocal_fused,
                      "reciprocal_fan_fused": t.reciprocal_fan_fused(3),
                      "rounds": rounds, "calls_per_round": calls,
                      "median_us": {v: 1e6 * x for v, x in med.items()},
                      "min_us": {v: 1e6 * min(x) for v, x in times.items()},
                      "ratio_single_over_fused": med["single"] / med["fused"],
                      "ratio_composed_over_fused": med["composed"] / med["fused"],
                      "host_scope_median_s": scopes,
                      "model_bytes": model_bytes,
                      "model_ratio_single": model_bytes["single"] / model_bytes["fused"],
                      "model_ratio_composed": model_bytes["composed"] / model_bytes["fused"]}),
          flush=True)


def values_fan(a, basis, model):
    """--op tau / mgga: one band on the wavefunction sphere with K_d = i G_d, two variants in
    alternating rounds of one process (medians over at least 7 rounds):
      fused     tau: one multi_transform_accumulate_density_fan call on three transforms;
                mgga: one multi_transform_apply_local_fan call on four transforms, member 0
                with None kernels and V, members 1..3 with i G_d, V_tau and -1/2 i G_d;
      composed  the best composition of the existing calls: tau, three torch multiplies of
                the values and one multi_transform_accumulate_density call; mgga, three
                multiplies, one multi_transform_apply_local call of four members and three
                torch.addcmul of the outputs.
    Prints microseconds per call, the ratio, the host scopes of the fused call and the
    modelled bytes of both (V values, K kernel, S stick array, I intermediate, R real grid
    array; a z stage V + S, a fan z stage V + sum of (K + S) with the values counted once, a
    y stage S + I, the x density stage I per member and 2 R, the x apply stage 2 I + R, a
    torch multiply 2 V + K, an addcmul 3 V + K)."""
    import numpy as np
    import torch

    import spfft_amd as sp
    nx, ny, nz = basis.fft_dims
    idx = basis.indices
    tau = a.op == "tau"
    n = 3 if tau else 4
    ts = model._wave_transforms(n)
    t = ts[0]
    ks = model.wave_gradient_kernels()
    ls = [-0.5 * k for k in ks]
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    c = torch.randn(basis.num_pw, dtype=torch.complex128, device="cuda", generator=g)
    v_r, v_tau = (torch.rand((nz, ny, nx), dtype=torch.float64, device="cuda", generator=g) for _ in range(2))
    rho = torch.zeros((nz, ny, nx), dtype=torch.float64, device="cuda")
    out = torch.empty_like(c)
    pots = [v_r, v_tau, v_tau, v_tau]
    ws = [0.5] * 3
    full = sp.Scaling.FULL

    def call(variant):
        if tau:
            if variant == "fused":
                return sp.multi_transform_accumulate_density_fan(ts, c, ks, ws, rho)
            return sp.multi_transform_accumulate_density(ts, [k * c for k in ks], ws, rho)
        if variant == "fused":
            return sp.multi_transform_apply_local_fan(ts, c, [None] + ks, pots, [None] + ls, output=out,
                                                      scaling=full)
        res = sp.multi_transform_apply_local(ts, [c] + [k * c for k in ks], pots, scalings=[full] * 4)
        h = res[0]
        for l, r in zip(ls, res[1:]):
            h = torch.addcmul(h, l, r)
        return h
    variants = ("fused", "composed")
    rounds, calls = max(7, a.reps), 10
    times = {v: [] for v in variants}
    for v in variants:
        call(v)
    for r in range(rounds):
        for v in (variants if r % 2 == 0 else variants[::-1]):  # mirrored orders
            torch.cuda.synchronize()
            t0_ = time.perf_counter()
            for _ in range(calls):
                call(v)
            torch.cuda.synchronize()
            times[v].append((time.perf_counter() - t0_) / calls)
    med = {v: sorted(x)[len(x) // 2] for v, x in times.items()}
    sp.timing_reset()
    sp.timing_enable(True)
    try:
        for _ in range(calls):
            call("fused")
        torch.cuda.synchronize()
        scopes = _scope_medians(sp.timing_json(), {
            "multi_accumulate_density_fan", "multi_apply_local_fan", "gpu_accumulate_density_fan_batch",
            "gpu_apply_local_fan_batch"})
    finally:
        sp.timing_enable(False)
    key = idx[:, 0].astype("int64") * (2 * ny + 1) + idx[:, 1]
    sticks = len(set(key.tolist()))
    columns = len(set(idx[:, 0].tolist()))
    R = nx * ny * nz * 8
    I, S, V = columns * ny * nz * 16, sticks * nz * 16, len(idx) * 16
    K = V
    if tau:
        middle = 3 * ((S + I) + I) + 2 * R
        model_bytes = {"fused": V + 3 * (K + S) + middle,
                       "composed": 3 * (2 * V + K) + 3 * (V + S) + middle}
    else:
        middle = 4 * ((S + I) + (2 * I + R) + (I + S))
        model_bytes = {"fused": (V + 3 * K + 4 * S) + middle + (4 * S + 3 * K + V),
                       "composed": 3 * (2 * V + K) + 4 * (V + S) + middle + 4 * (S + V) + 3 * (3 * V + K)}
    print(json.dumps({"workload": "plane-wave " + a.op, "fft_dims": list(basis.fft_dims),
                      "num_values": len(idx), "sticks": sticks, "members": n,
                      "batch": os.environ.get("SPFFT_BATCH", "1"),
                      "values_fan_fused": t.values_fan_fused(n),
                      "rounds": rounds, "calls_per_round": calls,
                      "median_us": {v: 1e6 * x for v, x in med.items()},
                      "min_us": {v: 1e6 * min(x) for v, x in times.items()},
                      "ratio_composed_over_fused": med["composed"] / med["fused"],
                      "host_scope_median_s": scopes,
                      "model_bytes": model_bytes,
                      "model_ratio_composed": model_bytes["composed"] / model_bytes["fused"]}),
          flush=True)


def spinor(a, basis, model):
    """--op spinor / spin_density: S = --transforms two-component spinors per call on the
    wavefunction sphere, in alternating rounds of one process (medians over at least 7
    rounds):
      fused     one multi_transform_apply_local_spinor / multi_transform_accumulate_spin_density
                call on 2 S transforms;
      composed  multi_transform_backward of the 2 S members, torch passes over the space
                domains (operator: per component one multiply and one addcmul with the
                complex off-diagonal field formed beforehand, and a copy back; density:
                four in-place updates), and for the operator multi_transform_forward;
      six       (operator) one multi_transform_apply_local call of 6 S members, v_uu, v_ud_re
                and v_ud_im on the one component and v_ud_re, v_ud_im and v_dd on the other,
                combined by torch passes over the values.
    Prints microseconds per call, the ratio against the faster composition, the host scopes
    of the fused call and the modelled x stage bytes per grid point (fp64: operator fused
    2*16 read + 2*16 write of the intermediates + 4*8 potential = 96 B, composed 2*32
    x_backward + 2*32 x_forward + at least 2*16 + 4*8 + 2*16 for the mix = 224 B; density
    fused 2*16 + 4*2*8 = 96 B, composed 2*32 + at least 2*16 + 4*2*8 = 160 B)."""
    import torch

    import spfft_amd as sp
    nx, ny, nz = basis.fft_dims
    S = max(1, min(4, a.transforms))
    op = a.op == "spinor"
    ts = model._wave_transforms(2 * S)
    ts6 = model._wave_transforms(6 * S) if op else None
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    cs = [torch.randn(basis.num_pw, dtype=torch.complex128, device="cuda", generator=g) for _ in range(2 * S)]
    v4 = torch.rand((4, nz, ny, nx), dtype=torch.float64, device="cuda", generator=g)
    vud = torch.complex(v4[2], v4[3])
    vdu = vud.conj().resolve_conj()
    m4 = torch.zeros((4, nz, ny, nx), dtype=torch.float64, device="cuda")
    outs = [torch.empty_like(c) for c in cs]
    ws = [1.0 + 0.25 * s for s in range(S)]
    full = sp.Scaling.FULL
    pots6 = [v4[0], v4[2], v4[3], v4[2], v4[3], v4[1]] * S

    def call(variant):
        if variant == "fused":
            if op:
                return sp.multi_transform_apply_local_spinor(ts, cs, v4, outputs=outs, scaling=full)
            return sp.multi_transform_accumulate_spin_density(ts, cs, ws, m4)
        if variant == "six":
            ins = []
            for s in range(S):
                u, d = cs[2 * s], cs[2 * s + 1]
                ins += [u, d, d, u, u, d]
            r = sp.multi_transform_apply_local(ts6, ins, pots6, scalings=[full] * (6 * S))
            res = []
            for s in range(S):
                q = r[6 * s:6 * s + 6]
                res.append(torch.add(q[0] + q[1], q[2], alpha=1j))
                res.append(torch.add(q[3] + q[5], q[4], alpha=-1j))
            return res
        spaces = sp.multi_transform_backward(ts, cs)
        if op:
            for u, d in zip(spaces[0::2], spaces[1::2]):
                nu = torch.addcmul(u * v4[0], d, vud)
                nd = torch.addcmul(d * v4[1], u, vdu)
                u.copy_(nu)
                d.copy_(nd)
            return sp.multi_transform_forward(ts, outputs=outs, scalings=[full] * (2 * S))
        for u, d, w in zip(spaces[0::2], spaces[1::2], ws):
            ur, dr = torch.view_as_real(u), torch.view_as_real(d)
            m4[0].add_((ur * ur).sum(-1), alpha=w)
            m4[1].add_((dr * dr).sum(-1), alpha=w)
            ud = torch.view_as_real(u * d.conj())
            m4[2].add_(ud[..., 0], alpha=w)
            m4[3].add_(ud[..., 1], alpha=w)
        return m4
    variants = ("fused", "composed", "six") if op else ("fused", "composed")
    rounds, calls = max(7, a.reps), 10
    times = {v: [] for v in variants}
    for v in variants:
        call(v)
    for r in range(rounds):
        for v in (variants if r % 2 == 0 else variants[::-1]):  # mirrored orders
            torch.cuda.synchronize()
            t0_ = time.perf_counter()
            for _ in range(calls):
                call(v)
            torch.cuda.synchronize()
            times[v].append((time.perf_counter() - t0_) / calls)
    med = {v: sorted(x)[len(x) // 2] for v, x in times.items()}
    sp.timing_reset()
    sp.timing_enable(True)
    try:
        for _ in range(calls):
            call("fused")
        torch.cuda.synchronize()
        tree = sp.timing_json()
        scopes = _scope_medians(tree, {
            "multi_apply_local_spinor", "multi_accumulate_spin_density", "gpu_apply_local_spinor_batch",
            "gpu_accumulate_spin_density_batch"})
        stages = _gpu_stage_medians(tree)
    finally:
        sp.timing_enable(False)
    best = min(med[v] for v in variants if v != "fused")
    model_bytes = {"fused": 96, "composed": 224} if op else {"fused": 96, "composed": 160}
    print(json.dumps({"workload": "plane-wave " + a.op, "fft_dims": list(basis.fft_dims),
                      "num_values": basis.num_pw, "spinors": S,
                      "batch": os.environ.get("SPFFT_BATCH", "1"),
                      "spinor_fused": ts[0].spinor_fused,
                      "rounds": rounds, "calls_per_round": calls,
                      "median_us": {v: 1e6 * x for v, x in med.items()},
                      "min_us": {v: 1e6 * min(x) for v, x in times.items()},
                      "max_us": {v: 1e6 * max(x) for v, x in times.items()},
                      "ratio_best_composition_over_fused": best / med["fused"],
                      "host_scope_median_s": scopes,
                      "gpu_stage_median_s": stages,
                      "model_x_stage_bytes_per_point": model_bytes,
                      "model_ratio_composed": model_bytes["composed"] / model_bytes["fused"]}),
          flush=True)


if __name__ == "__main__":
    main()
