"""Plane-wave application model: the workload SpFFT exists for.

Electronic-structure codes expand wavefunctions in plane waves
psi(r) = sum_G c_G exp(i G.r) with |G|^2 / 2 <= E_cut: a spherical set of
frequency indices (the sparse input of the transforms). The two hot operations
per band are:

  * local potential application, H_loc psi = FFT^-1 [ V(r) * FFT[psi](r) ]:
    backward transform, pointwise multiply in real space, forward transform;
  * density accumulation, rho(r) = sum_b w_b |psi_b(r)|^2: backward transforms.

Hybrid functionals add the exact-exchange operator, whose cost grows with the
square of the number of occupied bands: per pair (a, b) a forward transform of
conj(psi_a) psi_b, a multiply by K(G) and a backward transform, accumulated with
psi_a (exchange_operator, the pairs of a band in groups through
multi_transform_accumulate_fock).

Both run fully on the GPU with the space domain kept resident in the Grid's HBM
slab, several bands at once through multi_transform.

Units: a cubic cell of side `alat` (bohr), E_cut in hartree; G = 2 pi / alat * k.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

from ..types import ProcessingUnit, Scaling, TransformType


def _good_fft_size(n: int) -> int:
    """Smallest m >= n of the form 2^a 3^b 5^c (fast lengths for the FFT engines)."""
    m = max(1, n)
    while True:
        r = m
        for p in (2, 3, 5):
            while r % p == 0:
                r //= p
        if r == 1:
            return m
        m += 1


@dataclass
class PlaneWaveBasis:
    """Plane waves with |G|^2/2 <= ecut in a cubic cell; FFT grid holds |G| <= 2 Gmax
    (density / potential products) unless `fft_dims` is given."""
    alat: float
    ecut: float
    fft_dims: tuple = None

    def __post_init__(self):
        gmax = np.sqrt(2.0 * self.ecut)
        kmax = int(np.floor(gmax * self.alat / (2 * np.pi)))
        if self.fft_dims is None:
            n = _good_fft_size(4 * kmax + 1)
            self.fft_dims = (n, n, n)
        n0, n1, n2 = self.fft_dims
        if min(self.fft_dims) < 2 * kmax + 1:
            raise ValueError("FFT grid too small for the cutoff")
        ks = np.arange(-kmax, kmax + 1)
        kx, ky, kz = np.meshgrid(ks, ks, ks, indexing="ij")
        g2 = (2 * np.pi / self.alat) ** 2 * (kx ** 2 + ky ** 2 + kz ** 2)
        m = 0.5 * g2 <= self.ecut + 1e-12
        trip = np.stack([kx[m], ky[m], kz[m]], axis=1).astype(np.int32)
        # stick-major order (x, y storage key, then z): the layout the plan prefers
        key = (np.where(trip[:, 0] < 0, trip[:, 0] + n0, trip[:, 0]).astype(np.int64) * n1
               + np.where(trip[:, 1] < 0, trip[:, 1] + n1, trip[:, 1])) * n2 \
            + np.where(trip[:, 2] < 0, trip[:, 2] + n2, trip[:, 2])
        self.indices = trip[np.argsort(key, kind="stable")]
        self.g2 = (2 * np.pi / self.alat) ** 2 * (self.indices.astype(np.float64) ** 2).sum(axis=1)

    @property
    def num_pw(self) -> int:
        return len(self.indices)


class PlaneWaveModel:
    """Band-parallel local-potential and density operations on one device.

    `num_transforms` transforms (one Grid each, identical plans: a transform and
    its clones) process that many bands per multi_transform call. On the GPU
    the library runs such a group batched, one launch per stage for up to 8
    bands (multi_transform.cpp), so small grids are not launch bound."""

    def __init__(self, basis: PlaneWaveBasis, processing_unit=ProcessingUnit.GPU,
                 num_transforms: int = 8, single: bool = False):
        from ..grid import Grid, GridFloat
        self.basis = basis
        self.pu = processing_unit
        n0, n1, n2 = basis.fft_dims
        cls = GridFloat if single else Grid
        g = cls(n0, n1, n2, n0 * n1, processing_unit, -1)
        t0 = g.create_transform(processing_unit, TransformType.C2C, n0, n1, n2, n2, basis.indices)
        self.transforms = [t0] + [t0.clone() for _ in range(max(1, num_transforms) - 1)]
        self.volume_points = n0 * n1 * n2

    def apply_local_potential(self, psi: Sequence, v_r, unfused: bool = False) -> List:
        """H_loc psi_b for every band b: FFT^-1[V(r) FFT[psi_b](r)] (band coefficients in,
        band coefficients out). `v_r` is the real-space potential [z][y][x].

        One multi_transform_apply_local call per group of bands (on the GPU the x
        stage multiplies by V(r) in LDS and the space domain is never formed);
        `unfused` runs the composition backward, V(r) multiply, forward instead."""
        from ..grid import (multi_transform_apply_local, multi_transform_backward,
                            multi_transform_forward)
        out = []
        T = len(self.transforms)
        if not unfused:
            # the potential in the transforms' precision, where the transforms run
            real = self.transforms[0]._prec
            if hasattr(v_r, "mul_"):
                v = v_r.to(real.torch_real).contiguous()
            else:
                v = np.ascontiguousarray(v_r, dtype=real.real)
        for start in range(0, len(psi), T):
            group = list(psi[start:start + T])
            ts = self.transforms[:len(group)]
            if not unfused:
                out.extend(multi_transform_apply_local(ts, group, [v] * len(ts),
                                                       scalings=[Scaling.FULL] * len(ts)))
                continue
            spaces = multi_transform_backward(ts, group)
            for s in spaces:
                if hasattr(s, "mul_"):
                    s.mul_(v_r)
                else:
                    np.multiply(s, v_r, out=s)
            res = multi_transform_forward(ts, scalings=[Scaling.FULL] * len(ts))
            out.extend(r.clone() if hasattr(r, "clone") else np.array(r) for r in res)
        return out

    def density(self, psi: Sequence, weights: Sequence[float], unfused: bool = False):
        """rho(r) = sum_b w_b |psi_b(r)|^2 on the real-space grid [z][y][x].

        One multi_transform_accumulate_density call per group of bands into a
        zeroed rho of the transforms' precision, allocated where the transforms
        run (on the GPU the x stage adds w |psi|^2 to its rows of rho from LDS and
        the space domain is never formed); `unfused` runs the composition
        backward, |psi|^2, sum instead."""
        from ..grid import multi_transform_accumulate_density, multi_transform_backward
        rho = None
        T = len(self.transforms)
        psi, weights = list(psi), list(weights)
        if not unfused:
            t0 = self.transforms[0]
            if self.pu == ProcessingUnit.GPU:
                import torch
                dev = psi[0].device if psi and getattr(psi[0], "is_cuda", False) else "cuda"
                rho = torch.zeros(t0.space_domain_shape(), dtype=t0._prec.torch_real, device=dev)
            else:
                rho = np.zeros(t0.space_domain_shape(), dtype=t0._prec.real)
            for start in range(0, len(psi), T):
                group = psi[start:start + T]
                multi_transform_accumulate_density(self.transforms[:len(group)], group,
                                                   weights[start:start + T], rho)
            return rho
        for start in range(0, len(psi), T):
            group = psi[start:start + T]
            spaces = multi_transform_backward(self.transforms[:len(group)], group)
            for s, w in zip(spaces, weights[start:start + T]):
                contrib = (s.real ** 2 + s.imag ** 2) * w
                rho = contrib if rho is None else rho + contrib
        return rho

    def hartree_kernel(self):
        """K(G) = 4 pi / |G|^2 on the model's plane waves, K(0) = 0 (real, in the
        transforms' precision, where the transforms run)."""
        k = getattr(self, "_hartree_kernel", None)
        if k is None:
            g2 = self.basis.g2
            k = np.where(g2 > 0, 4.0 * np.pi / np.where(g2 > 0, g2, 1.0), 0.0)
            k = k.astype(self.transforms[0]._prec.real)
            if self.pu == ProcessingUnit.GPU:
                import torch
                k = torch.as_tensor(k, device=f"cuda:{self.transforms[0].device_id}")
            self._hartree_kernel = k
        return k

    def hartree_potential(self, rho, unfused: bool = False):
        """V_H(r) = FFT^-1[ 4 pi / |G|^2 * FFT[rho](G) ] on the model's plane waves
        (the G = 0 term dropped), as a new real array [z][y][x].

        One apply_reciprocal call (on the GPU the z stage multiplies by K(G) in LDS
        between its two FFTs and the coefficients never go through memory);
        `unfused` runs the composition forward, K(G) multiply, backward instead."""
        t = self.transforms[0]
        k = self.hartree_kernel()
        if not unfused:
            v = t.apply_reciprocal(k, space=rho, scaling=Scaling.FULL)
        else:
            c = t.forward(space=rho, scaling=Scaling.FULL)
            if hasattr(c, "mul_"):
                c.mul_(k)
            else:
                c *= k
            v = t.backward(c)
        return v.real.clone() if hasattr(v, "clone") else np.array(v.real)

    def _exchange_setup(self):
        """The transform of the exchange operator, built on first use: the pair densities
        conj(psi_a) psi_b hold |G| <= 2 Gmax, so its index set is the sphere |G|^2/2 <=
        4 ecut (clipped to the FFT grid), with K(G) = 4 pi / |G|^2 and K(0) = 0."""
        if getattr(self, "_exchange", None) is not None:
            return self._exchange
        b = self.basis
        dims = b.fft_dims
        unit = (2 * np.pi / b.alat) ** 2
        kmax = int(np.floor(2.0 * np.sqrt(2.0 * b.ecut) * b.alat / (2 * np.pi)))
        axes = [np.arange(-min(kmax, (n - 1) // 2), min(kmax, (n - 1) // 2) + 1) for n in dims]
        kx, ky, kz = np.meshgrid(*axes, indexing="ij")
        g2 = unit * (kx ** 2 + ky ** 2 + kz ** 2)
        m = 0.5 * g2 <= 4.0 * b.ecut + 1e-12
        trip = np.stack([kx[m], ky[m], kz[m]], axis=1).astype(np.int32)
        # stick-major order, as PlaneWaveBasis
        st = [np.where(trip[:, d] < 0, trip[:, d] + dims[d], trip[:, d]).astype(np.int64)
              for d in range(3)]
        trip = trip[np.argsort((st[0] * dims[1] + st[1]) * dims[2] + st[2], kind="stable")]
        g2 = unit * (trip.astype(np.float64) ** 2).sum(axis=1)
        t0 = self.transforms[0]
        khost = np.where(g2 > 0, 4.0 * np.pi / np.where(g2 > 0, g2, 1.0), 0.0).astype(t0._prec.real)
        from ..grid import Grid, GridFloat
        n0, n1, n2 = dims
        g = (GridFloat if t0._prec.single else Grid)(n0, n1, n2, n0 * n1, self.pu, -1)
        t = g.create_transform(self.pu, TransformType.C2C, n0, n1, n2, n2, trip)
        k = khost
        if self.pu == ProcessingUnit.GPU:
            import torch
            k = torch.as_tensor(khost, device=f"cuda:{t.device_id}")
        self._exchange = (t, trip, khost, k)
        return self._exchange

    @property
    def exchange_transform(self):
        return self._exchange_setup()[0]

    @property
    def exchange_indices(self):
        return self._exchange_setup()[1]

    @property
    def exchange_kernel_host(self):
        return self._exchange_setup()[2]

    def _exchange_transforms(self, count: int):
        """The pair-density transform and `count` - 1 clones of it (made on first use)."""
        tx = self._exchange_setup()[0]
        clones = self.__dict__.setdefault("_exchange_clones", [])
        while len(clones) < count - 1:
            clones.append(tx.clone())
        return [tx] + clones[:count - 1]

    def exchange_operator(self, psi: Sequence, occupations: Sequence[float],
                          unfused: bool = False, max_batch: int = 8) -> List:
        """Exact-exchange (Fock) operator of hybrid functionals on every band b, up to the
        cell-volume prefactor: the coefficients of
        sum_a -f_a psi_a(r) FFT^-1[ K(G) FFT[conj(psi_a) psi_b](G) ](r)
        over the occupied bands a (f_a != 0), projected back on the basis.

        The bands go to real space once with the model's transforms; the pairs (a, b) of
        a band b then go through multi_transform_accumulate_fock in groups of up to
        `max_batch` occupied bands a, on the pair-density transform and its clones, into
        the band's accumulator (a group of one is a plain accumulate_fock call). On the
        GPU the forward x stage forms conj(a) b in its loads, the backward x stage adds
        -f_a a u to its rows of the accumulator from LDS, no pair array goes through
        memory, and a group shares one launch per stage; the sum over a runs in band
        order whatever the grouping. `unfused` runs the composition product,
        apply_reciprocal, addcmul, one pair at a time."""
        from ..grid import multi_transform_accumulate_fock
        t0 = self.transforms[0]
        tx, _, _, k = self._exchange_setup()
        psi, occupations = list(psi), [float(f) for f in occupations]
        real = []
        for c in psi:
            s = t0.backward(c)
            real.append(s.clone() if hasattr(s, "clone") else np.array(s))
        occupied = [(f, a) for f, a in zip(occupations, real) if f != 0.0]
        step = max(1, int(max_batch))
        groups = [occupied[g:g + step] for g in range(0, len(occupied), step)]
        out = []
        for b in real:
            acc = b.new_zeros(b.shape) if hasattr(b, "new_zeros") else np.zeros_like(b)
            for grp in ([] if unfused else groups):
                if len(grp) == 1:
                    tx.accumulate_fock(grp[0][1], b, k, -grp[0][0], acc, scaling=Scaling.FULL)
                else:
                    multi_transform_accumulate_fock(
                        self._exchange_transforms(len(grp)), [a for _, a in grp], [b] * len(grp), k,
                        [-f for f, _ in grp], acc, scaling=Scaling.FULL)
            for f, a in (occupied if unfused else []):
                # the product written straight into the space domain
                space = tx.space_domain(self.pu)
                if hasattr(acc, "addcmul_"):
                    import torch
                    torch.mul(a.conj(), b, out=space)
                    acc.addcmul_(a, tx.apply_reciprocal(k, scaling=Scaling.FULL), value=-f)
                else:
                    np.multiply(np.conj(a), b, out=space)
                    acc += -f * a * tx.apply_reciprocal(k, scaling=Scaling.FULL)
            c = t0.forward(space=acc, scaling=Scaling.FULL)
            out.append(c.clone() if hasattr(c, "clone") else np.array(c))
        return out

    def gradient_kernels(self):
        """K_d(G) = i G_d, d = x, y, z, on the density sphere |G|^2/2 <= 4 ecut (the index
        set of the pair-density transform): complex, in the transforms' precision, where
        the transforms run."""
        ks = getattr(self, "_gradient_kernels", None)
        if ks is None:
            t, trip, _, _ = self._exchange_setup()
            unit = 2 * np.pi / self.basis.alat
            ks = [(1j * unit * trip[:, d].astype(np.float64)).astype(t._prec.complex)
                  for d in range(3)]
            if self.pu == ProcessingUnit.GPU:
                import torch
                ks = [torch.as_tensor(k, device=f"cuda:{t.device_id}") for k in ks]
            self._gradient_kernels = ks
        return ks

    @staticmethod
    def _copy(a):
        return a.clone() if hasattr(a, "clone") else np.array(a)

    def gradient(self, f, unfused: bool = False) -> List:
        """(d_x f, d_y f, d_z f) of a grid function f [z][y][x] on the density sphere:
        d_d f = FFT^-1[ i G_d FFT[f](G) ], as three new complex arrays.

        One multi_transform_reciprocal_fan_out call on the pair-density transform and two
        clones (on the GPU one forward transform, one z kernel that transforms each stick
        block once and feeds three inverse z FFTs, and one launch per backward stage for
        the three components); `unfused` runs the composition forward, then per component
        multiply and backward."""
        from ..grid import multi_transform_reciprocal_fan_out
        ts = self._exchange_transforms(3)
        ks = self.gradient_kernels()
        if not unfused:
            return [self._copy(s) for s in
                    multi_transform_reciprocal_fan_out(ts, ks, space=f, scaling=Scaling.FULL)]
        t = ts[0]
        c = self._copy(t.forward(space=f, scaling=Scaling.FULL))
        return [self._copy(t.backward(c * k)) for k in ks]

    def divergence(self, fields: Sequence, unfused: bool = False):
        """div h = sum_d FFT^-1[ i G_d FFT[h_d](G) ] of a vector field (h_x, h_y, h_z) of
        grid functions [z][y][x] on the density sphere, as a new complex array.

        One multi_transform_reciprocal_fan_in call on the pair-density transform and two
        clones (on the GPU one launch per forward stage for the three components, one z
        kernel that sums i G_d c_d per stick block in LDS, and one backward transform);
        `unfused` runs three forward transforms, the multiply-add of the values and one
        backward transform."""
        from ..grid import multi_transform_reciprocal_fan_in
        fields = list(fields)
        if len(fields) != 3:
            raise ValueError("divergence: three fields (x, y, z components)")
        ts = self._exchange_transforms(3)
        ks = self.gradient_kernels()
        if not unfused:
            return self._copy(multi_transform_reciprocal_fan_in(ts, ks, spaces=fields,
                                                                scaling=Scaling.FULL))
        t = ts[0]
        s = None
        for h, k in zip(fields, ks):
            c = t.forward(space=h, scaling=Scaling.FULL) * k
            s = c if s is None else s + c
        return self._copy(t.backward(s))

    def wave_gradient_kernels(self):
        """K_d(G) = i G_d, d = x, y, z, on the wavefunction sphere |G|^2/2 <= ecut (the index
        set of the model's transforms): complex, in the transforms' precision, where the
        transforms run."""
        ks = getattr(self, "_wave_gradient_kernels", None)
        if ks is None:
            t = self.transforms[0]
            unit = 2 * np.pi / self.basis.alat
            ks = [(1j * unit * self.basis.indices[:, d].astype(np.float64)).astype(t._prec.complex)
                  for d in range(3)]
            if self.pu == ProcessingUnit.GPU:
                import torch
                ks = [torch.as_tensor(k, device=f"cuda:{t.device_id}") for k in ks]
            self._wave_gradient_kernels = ks
        return ks

    def _wave_transforms(self, count: int):
        """`count` identical wavefunction transforms: the model's, then clones kept for the
        value fans (the model's own list, and with it the band groups, stays as it is)."""
        extra = getattr(self, "_wave_clones", None)
        if extra is None:
            extra = self._wave_clones = []
        while len(self.transforms) + len(extra) < count:
            extra.append(self.transforms[0].clone())
        return (self.transforms + extra)[:count]

    def _real_field(self, v):
        real = self.transforms[0]._prec
        if hasattr(v, "mul_"):
            return v.to(real.torch_real).contiguous()
        return np.ascontiguousarray(v, dtype=real.real)

    def kinetic_energy_density(self, psi: Sequence, weights: Sequence[float], unfused: bool = False):
        """tau(r) = 1/2 sum_b w_b sum_d |FFT^-1[i G_d c_b](r)|^2 on the real-space grid
        [z][y][x], in a zeroed array of the transforms' precision where the transforms run.

        One multi_transform_accumulate_density_fan call per band on three wavefunction
        transforms (on the GPU one z kernel that reads the band's coefficients and feeds
        three inverse z FFTs, then one launch per later stage for the three components);
        `unfused` multiplies the coefficients by the three kernels and runs
        multi_transform_accumulate_density."""
        from ..grid import multi_transform_accumulate_density, multi_transform_accumulate_density_fan
        ts = self._wave_transforms(3)
        ks = self.wave_gradient_kernels()
        t0 = ts[0]
        psi, weights = list(psi), list(weights)
        if self.pu == ProcessingUnit.GPU:
            import torch
            dev = psi[0].device if psi and getattr(psi[0], "is_cuda", False) else "cuda"
            tau = torch.zeros(t0.space_domain_shape(), dtype=t0._prec.torch_real, device=dev)
        else:
            tau = np.zeros(t0.space_domain_shape(), dtype=t0._prec.real)
        for c, w in zip(psi, weights):
            if not unfused:
                multi_transform_accumulate_density_fan(ts, c, ks, [0.5 * w] * 3, tau)
            else:
                multi_transform_accumulate_density(ts, [k * c for k in ks], [0.5 * w] * 3, tau)
        return tau

    def meta_gga_local(self, psi: Sequence, v_r, v_tau, unfused: bool = False) -> List:
        """The local part of a meta-GGA Hamiltonian for every band b (band coefficients in,
        band coefficients out): FFT[V FFT^-1[c_b]] - 1/2 sum_d i G_d FFT[V_tau FFT^-1[i G_d c_b]]
        with the real-space potentials `v_r` and `v_tau` [z][y][x].

        One multi_transform_apply_local_fan call per band on four wavefunction transforms:
        member 0 with no kernels and V, members 1..3 with i G_d in front, V_tau and
        -1/2 i G_d behind (on the GPU one z kernel in, the batched y and x launches, one z
        kernel that sums the four results); `unfused` multiplies the coefficients, runs
        multi_transform_apply_local and combines the four outputs."""
        from ..grid import multi_transform_apply_local, multi_transform_apply_local_fan
        ts = self._wave_transforms(4)
        ks = self.wave_gradient_kernels()
        ls = getattr(self, "_wave_gradient_kernels_out", None)
        if ls is None:
            ls = self._wave_gradient_kernels_out = [-0.5 * k for k in ks]
        v, vt = self._real_field(v_r), self._real_field(v_tau)
        pots = [v, vt, vt, vt]
        out = []
        for c in psi:
            if not unfused:
                out.append(self._copy(multi_transform_apply_local_fan(
                    ts, c, [None] + ks, pots, [None] + ls, scaling=Scaling.FULL)))
                continue
            res = multi_transform_apply_local(ts, [c] + [k * c for k in ks], pots,
                                              scalings=[Scaling.FULL] * 4)
            h = self._copy(res[0])
            for l, r in zip(ls, res[1:]):
                h = h + l * r
            out.append(h)
        return out

    # spinors per multi_transform_*_spinor call (the library's launches take up to 4)
    SPINOR_GROUP = 4

    def _four_fields(self, v4):
        """(v_uu, v_dd, v_ud_re, v_ud_im) as one contiguous [4, z, y, x] array of the
        transforms' precision, where it is."""
        real = self.transforms[0]._prec
        if hasattr(v4, "mul_"):
            return v4.to(real.torch_real).contiguous()
        if isinstance(v4, np.ndarray):
            return np.ascontiguousarray(v4, dtype=real.real)
        parts = [self._real_field(v) for v in v4]
        if hasattr(parts[0], "mul_"):
            import torch
            return torch.stack(parts).contiguous()
        return np.ascontiguousarray(np.stack(parts))

    def apply_spinor_potential(self, spinors: Sequence, v4, unfused: bool = False) -> List:
        """The 2x2 Hermitian local potential on two-component spinors (non-collinear
        magnetism, spin-orbit coupling): for every spinor (c_up, c_dn) the coefficients of
        v_uu psi_up + v_ud psi_dn and conj(v_ud) psi_up + v_dd psi_dn, as a list of pairs.
        `v4` holds (v_uu, v_dd, v_ud_re, v_ud_im) [4][z][y][x]; for V + B . sigma:
        v_uu = V + B_z, v_dd = V - B_z, v_ud_re = B_x, v_ud_im = -B_y.

        One multi_transform_apply_local_spinor call per group of 4 spinors on wavefunction
        transforms (on the GPU the x stage holds both components of a tile in LDS and mixes
        them there; the space domains are never formed); `unfused` runs the composition
        multi_transform_backward of both components, the mix as array passes over the two
        space domains, multi_transform_forward."""
        from ..grid import (multi_transform_apply_local_spinor, multi_transform_backward,
                            multi_transform_forward)
        spinors = [tuple(s) for s in spinors]
        v = self._four_fields(v4)
        out = []
        if unfused:
            vud = v[2] + 1j * v[3]
            vdu = vud.conj() if hasattr(vud, "conj") else np.conj(vud)
        for start in range(0, len(spinors), self.SPINOR_GROUP):
            group = spinors[start:start + self.SPINOR_GROUP]
            ts = self._wave_transforms(2 * len(group))
            flat = [c for s in group for c in s]
            if not unfused:
                res = multi_transform_apply_local_spinor(ts, flat, v, scaling=Scaling.FULL)
            else:
                spaces = multi_transform_backward(ts, flat)
                for u, d in zip(spaces[0::2], spaces[1::2]):
                    nu = v[0] * u + vud * d
                    nd = vdu * u + v[1] * d
                    if hasattr(u, "copy_"):
                        u.copy_(nu)
                        d.copy_(nd)
                    else:
                        u[...] = nu
                        d[...] = nd
                res = multi_transform_forward(ts, scalings=[Scaling.FULL] * len(ts))
            res = [self._copy(r) for r in res]
            out.extend(zip(res[0::2], res[1::2]))
        return out

    def spin_density(self, spinors: Sequence, weights: Sequence[float], unfused: bool = False):
        """(n, m_x, m_y, m_z)(r) = sum_s w_s psi_s^+ (1, sigma) psi_s of two-component
        spinors (c_up, c_dn) on the real-space grid [z][y][x], as four new real arrays of the
        transforms' precision where the transforms run.

        One multi_transform_accumulate_spin_density call per group of 4 spinors into the
        zeroed spin density matrix (n_uu, n_dd, n_ud_re, n_ud_im), from which n = n_uu +
        n_dd, m_z = n_uu - n_dd, m_x = 2 n_ud_re, m_y = -2 n_ud_im (on the GPU the x stage
        updates its rows of the four arrays from LDS); `unfused` runs the composition
        multi_transform_backward and array passes over the two space domains."""
        from ..grid import multi_transform_accumulate_spin_density, multi_transform_backward
        spinors, weights = [tuple(s) for s in spinors], [float(w) for w in weights]
        t0 = self.transforms[0]
        shape = (4,) + tuple(t0.space_domain_shape())
        if self.pu == ProcessingUnit.GPU:
            import torch
            first = spinors[0][0] if spinors else None
            dev = first.device if getattr(first, "is_cuda", False) else "cuda"
            m = torch.zeros(shape, dtype=t0._prec.torch_real, device=dev)
        else:
            m = np.zeros(shape, dtype=t0._prec.real)
        for start in range(0, len(spinors), self.SPINOR_GROUP):
            group = spinors[start:start + self.SPINOR_GROUP]
            ws = weights[start:start + self.SPINOR_GROUP]
            ts = self._wave_transforms(2 * len(group))
            flat = [c for s in group for c in s]
            if not unfused:
                multi_transform_accumulate_spin_density(ts, flat, ws, m)
                continue
            spaces = multi_transform_backward(ts, flat)
            for u, d, w in zip(spaces[0::2], spaces[1::2], ws):
                ud = u * (d.conj() if hasattr(d, "conj") else np.conj(d))
                m[0] += w * (u.real ** 2 + u.imag ** 2)
                m[1] += w * (d.real ** 2 + d.imag ** 2)
                m[2] += w * ud.real
                m[3] += w * ud.imag
        return m[0] + m[1], 2 * m[2], -2 * m[3], m[0] - m[1]

    def kinetic(self, psi: Sequence) -> List:
        """T psi_b = |G|^2/2 c_G (diagonal in the plane-wave basis)."""
        g2 = self.basis.g2
        out = []
        for c in psi:
            if type(c).__module__.startswith("torch"):
                import torch
                out.append(c * torch.as_tensor(0.5 * g2, device=c.device, dtype=c.real.dtype))
            else:
                out.append(np.asarray(c) * (0.5 * g2))
        return out
