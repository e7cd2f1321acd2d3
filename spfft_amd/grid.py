"""Pythonic front end of the native library: Grid / Transform (and single-precision twins).

Mirrors the C++ API of SpFFT (reference: include/spfft/grid.hpp, transform.hpp,
multi_transform.hpp). Arrays may be numpy arrays (host memory) or torch tensors
(host or device memory). The space domain of a GPU transform is returned as a
zero-copy torch view of the Grid's HBM slab.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from .ops._lib import lib
from .types import ExchangeType, IndexFormat, ProcessingUnit, Scaling, TransformType, raise_for

try:  # torch is optional for host-only use
    import torch
except Exception:  # pragma: no cover
    torch = None


_SHUTDOWN = [False]


def _at_exit():
    # objects still alive at interpreter exit are not destroyed through the native
    # library: the HIP runtime may already be tearing down.
    _SHUTDOWN[0] = True


import atexit  # noqa: E402

atexit.register(_at_exit)


def _check(code: int) -> None:
    if code != 0:
        msg = lib().spfft_amd_last_error_message()
        raise_for(code, msg.decode() if msg else "")


def _is_torch(a) -> bool:
    return torch is not None and isinstance(a, torch.Tensor)


class _Precision:
    def __init__(self, single: bool):
        self.single = single
        self.prefix = "spfft_float_" if single else "spfft_"
        self.amd = "spfft_amd_float_" if single else "spfft_amd_"
        self.real = np.float32 if single else np.float64
        self.complex = np.complex64 if single else np.complex128

    def fn(self, name):
        return getattr(lib(), self.prefix + name)

    def amd_fn(self, name):
        return getattr(lib(), self.amd + name)

    @property
    def torch_complex(self):
        return torch.complex64 if self.single else torch.complex128

    @property
    def torch_real(self):
        return torch.float32 if self.single else torch.float64


def _data_ptr(a, prec: _Precision, writable: bool, what: str):
    """Returns (address, keepalive) of a complex array argument."""
    if a is None:
        return None, None
    if _is_torch(a):
        if a.dtype in (torch.complex64, torch.complex128):
            if a.dtype != prec.torch_complex:
                raise TypeError(f"{what}: expected {prec.torch_complex}, got {a.dtype}")
        elif a.dtype != prec.torch_real:
            raise TypeError(f"{what}: expected {prec.torch_complex}, got {a.dtype}")
        if not a.is_contiguous():
            if writable:
                raise ValueError(f"{what} must be contiguous")
            a = a.contiguous()
        return a.data_ptr(), a
    arr = np.asarray(a)
    if arr.dtype not in (prec.complex, prec.real) or not arr.flags.c_contiguous:
        if writable:
            raise TypeError(f"{what}: expected a C-contiguous {np.dtype(prec.complex)} array")
        arr = np.ascontiguousarray(arr, dtype=prec.complex)
    return arr.ctypes.data, arr


def _potential_ptr(v, prec: _Precision, shape):
    """Returns (address, keepalive) of a real potential of the space domain's shape."""
    if v is None:
        return None, None
    if _is_torch(v):
        if v.dtype != prec.torch_real:
            raise TypeError(f"potential: expected {prec.torch_real}, got {v.dtype}")
        if tuple(v.shape) != tuple(shape):
            raise ValueError(f"potential: expected shape {tuple(shape)}, got {tuple(v.shape)}")
        v = v.contiguous()
        return v.data_ptr(), v
    arr = np.asarray(v)
    if arr.dtype != prec.real:
        raise TypeError(f"potential: expected {np.dtype(prec.real)}, got {arr.dtype}")
    if tuple(arr.shape) != tuple(shape):
        raise ValueError(f"potential: expected shape {tuple(shape)}, got {tuple(arr.shape)}")
    arr = np.ascontiguousarray(arr)
    return arr.ctypes.data, arr


def _density_ptr(rho, prec: _Precision, shape):
    """Returns (address, keepalive) of a real density of the space domain's shape. The
    array is written, so it is never copied: a wrong dtype is a TypeError, a wrong shape
    or a non-contiguous array a ValueError."""
    if rho is None:
        return None, None
    if _is_torch(rho):
        if rho.dtype != prec.torch_real:
            raise TypeError(f"density: expected {prec.torch_real}, got {rho.dtype}")
        if tuple(rho.shape) != tuple(shape):
            raise ValueError(f"density: expected shape {tuple(shape)}, got {tuple(rho.shape)}")
        if not rho.is_contiguous():
            raise ValueError("density must be contiguous")
        return rho.data_ptr(), rho
    if not isinstance(rho, np.ndarray) or rho.dtype != prec.real:
        raise TypeError(f"density: expected a {np.dtype(prec.real)} array, got "
                        f"{getattr(rho, 'dtype', type(rho).__name__)}")
    if tuple(rho.shape) != tuple(shape):
        raise ValueError(f"density: expected shape {tuple(shape)}, got {tuple(rho.shape)}")
    if not rho.flags.c_contiguous or not rho.flags.writeable:
        raise ValueError("density must be a writable C-contiguous array")
    return rho.ctypes.data, rho


def _kernel_ptr(k, prec: _Precision, count: int):
    """Returns (address, keepalive, is_complex) of a reciprocal-space kernel: a real or
    complex array of the transform's precision with one entry per local value."""
    if _is_torch(k):
        if k.dtype not in (prec.torch_real, prec.torch_complex):
            raise TypeError(f"kernel: expected {prec.torch_real} or {prec.torch_complex}, got {k.dtype}")
        if k.numel() != count:
            raise ValueError(f"kernel: expected {count} entries, got {k.numel()}")
        k = k.contiguous()
        return k.data_ptr(), k, k.dtype == prec.torch_complex
    arr = np.asarray(k)
    if arr.dtype not in (prec.real, prec.complex):
        raise TypeError(f"kernel: expected {np.dtype(prec.real)} or {np.dtype(prec.complex)}, "
                        f"got {arr.dtype}")
    if arr.size != count:
        raise ValueError(f"kernel: expected {count} entries, got {arr.size}")
    arr = np.ascontiguousarray(arr)
    return arr.ctypes.data, arr, arr.dtype == prec.complex


def _space_array_ptr(x, prec: _Precision, shape, real: bool, what: str, writable: bool):
    """Returns (address, keepalive) of an array over the space domain: shape `shape`,
    complex (real for R2C) in the transform's precision. A wrong dtype is a TypeError, a
    wrong shape a ValueError; an array that is written is never copied."""
    if _is_torch(x):
        want = prec.torch_real if real else prec.torch_complex
        if x.dtype != want:
            raise TypeError(f"{what}: expected {want}, got {x.dtype}")
        if tuple(x.shape) != tuple(shape):
            raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(x.shape)}")
        if not x.is_contiguous():
            if writable:
                raise ValueError(f"{what} must be contiguous")
            x = x.contiguous()
        return x.data_ptr(), x
    want = np.dtype(prec.real if real else prec.complex)
    if not isinstance(x, np.ndarray) or x.dtype != want:
        raise TypeError(f"{what}: expected a {want} array, got "
                        f"{getattr(x, 'dtype', type(x).__name__)}")
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(x.shape)}")
    if writable and (not x.flags.c_contiguous or not x.flags.writeable):
        raise ValueError(f"{what} must be a writable C-contiguous array")
    x = np.ascontiguousarray(x)
    return x.ctypes.data, x


class _GridBase:
    _single = False

    def __init__(self, max_dim_x: int, max_dim_y: int, max_dim_z: int,
                 max_num_local_z_columns: int, processing_unit=ProcessingUnit.HOST,
                 max_num_threads: int = -1, *, max_local_z_length: Optional[int] = None,
                 comm=None, exchange_type=ExchangeType.DEFAULT, _handle=None):
        self._prec = _Precision(self._single)
        self._comm = comm
        if _handle is not None:
            self._h = _handle
            return
        h = ctypes.c_void_p()
        if comm is None:
            _check(self._prec.fn("grid_create")(ctypes.byref(h), max_dim_x, max_dim_y, max_dim_z,
                                                max_num_local_z_columns, int(processing_unit),
                                                max_num_threads))
        else:
            if max_local_z_length is None:
                raise ValueError("distributed grids need max_local_z_length")
            create = (lib().spfft_amd_float_grid_create_distributed if self._single
                      else lib().spfft_amd_grid_create_distributed)
            _check(create(ctypes.byref(h), max_dim_x, max_dim_y, max_dim_z,
                          max_num_local_z_columns, max_local_z_length, int(processing_unit),
                          max_num_threads, comm.handle, int(exchange_type)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and not _SHUTDOWN[0]:
            try:
                self._prec.fn("grid_destroy")(h)
            except Exception:
                pass
            self._h = None

    def _get(self, name):
        v = ctypes.c_int()
        _check(self._prec.fn("grid_" + name)(self._h, ctypes.byref(v)))
        return v.value

    max_dim_x = property(lambda self: self._get("max_dim_x"))
    max_dim_y = property(lambda self: self._get("max_dim_y"))
    max_dim_z = property(lambda self: self._get("max_dim_z"))
    max_num_local_z_columns = property(lambda self: self._get("max_num_local_z_columns"))
    max_local_z_length = property(lambda self: self._get("max_local_z_length"))
    processing_unit = property(lambda self: ProcessingUnit(self._get("processing_unit")))
    device_id = property(lambda self: self._get("device_id"))
    num_threads = property(lambda self: self._get("num_threads"))

    @property
    def exchange_type(self) -> ExchangeType:
        v = ctypes.c_int()
        _check(self._prec.amd_fn("grid_exchange_type")(self._h, ctypes.byref(v)))
        return ExchangeType(v.value)

    @property
    def data_plane(self) -> str:
        """GPU data plane of a distributed grid: "rccl", "ipc", "peer", "loopback",
        "rccl-self" or "none". Collective on first use (it creates the data plane)."""
        v = ctypes.c_char_p()
        _check(self._prec.amd_fn("grid_data_plane")(self._h, ctypes.byref(v)))
        return v.value.decode()

    @property
    def data_plane_info(self) -> dict:
        """The data plane's setup facts: "kind", and where they apply "self_test" /
        "self_test_ms" (route self-test), "devices" (PCI bus ids of every GPU the plane
        touches, relay GPUs included), "link_GBps_measured", "channel_priority" ("high",
        or "normal" when ranks share a GPU). Collective on first use."""
        import json
        v = ctypes.c_char_p()
        _check(self._prec.amd_fn("grid_data_plane_info")(self._h, ctypes.byref(v)))
        return json.loads(v.value.decode())

    @property
    def device_bytes(self) -> int:
        """Device memory the grid allocated (exchange buffers, y/x intermediate, space)."""
        v = ctypes.c_ulonglong()
        _check(self._prec.amd_fn("grid_device_bytes")(self._h, ctypes.byref(v)))
        return v.value

    @property
    def communicator(self):
        return self._comm

    def create_transform(self, processing_unit, transform_type, dim_x: int, dim_y: int,
                         dim_z: int, local_z_length: int, indices,
                         index_format=IndexFormat.TRIPLETS):
        """Plans a transform. `indices` is an (n, 3) or flat int array of (x, y, z) triplets."""
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int32).reshape(-1))
        if idx.size % 3:
            raise ValueError("indices must hold triplets")
        n = idx.size // 3
        h = ctypes.c_void_p()
        _check(self._prec.fn("transform_create")(
            ctypes.byref(h), self._h, int(processing_unit), int(transform_type), dim_x, dim_y,
            dim_z, local_z_length, n, int(index_format),
            idx.ctypes.data if n else None))
        cls = TransformFloat if self._single else Transform
        t = cls(h, self)
        in_process = getattr(self._comm, "in_process", False)
        if ProcessingUnit(processing_unit) == ProcessingUnit.GPU and torch is not None \
                and not in_process:
            # torch semantics: run on the current torch stream (ordered with torch work
            # on it, no cross-stream event per call); calls stay synchronous.
            # Ranks of an in-process group keep private streams: they share torch's
            # current stream, and one rank's exchange must not queue behind another's.
            t.set_stream(torch.cuda.current_stream(), synchronous=True)
        return t


class Grid(_GridBase):
    """Double-precision grid (spfft::Grid)."""

    _single = False


class GridFloat(_GridBase):
    """Single-precision grid (spfft::GridFloat)."""

    _single = True


class _TransformBase:
    _single = False

    def __init__(self, handle, grid):
        self._h = handle
        self._grid = grid  # keeps the grid (buffers) alive
        self._prec = _Precision(self._single)
        self._stream = None
        self._cache = {}
        self._views = {}
        self._step_keep = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and not _SHUTDOWN[0]:
            try:
                self._prec.fn("transform_destroy")(h)
            except Exception:
                pass
            self._h = None

    @property
    def handle(self):
        return self._h

    def _get(self, name, ll=False):
        # every getter of a transform is immutable after creation: cache it
        c = self._cache.get(name)
        if c is not None:
            return c
        v = ctypes.c_longlong() if ll else ctypes.c_int()
        _check(self._prec.fn("transform_" + name)(self._h, ctypes.byref(v)))
        self._cache[name] = v.value
        return v.value

    type = property(lambda self: TransformType(self._get("type")))
    dim_x = property(lambda self: self._get("dim_x"))
    dim_y = property(lambda self: self._get("dim_y"))
    dim_z = property(lambda self: self._get("dim_z"))
    local_z_length = property(lambda self: self._get("local_z_length"))
    local_z_offset = property(lambda self: self._get("local_z_offset"))
    local_slice_size = property(lambda self: self._get("local_slice_size"))
    global_size = property(lambda self: self._get("global_size", True))
    num_local_elements = property(lambda self: self._get("num_local_elements"))
    num_global_elements = property(lambda self: self._get("num_global_elements", True))
    processing_unit = property(lambda self: ProcessingUnit(self._get("processing_unit")))
    device_id = property(lambda self: self._get("device_id"))
    num_threads = property(lambda self: self._get("num_threads"))

    @property
    def grid(self):
        return self._grid

    def clone(self):
        h = ctypes.c_void_p()
        _check(self._prec.fn("transform_clone")(self._h, ctypes.byref(h)))
        t = type(self)(h, None)
        if self._stream is not None:
            t.set_stream(self._stream)
        return t

    # ---------------------------------------------------------------- data
    def space_domain_shape(self):
        return (self.local_z_length, self.dim_y, self.dim_x)

    def space_domain_ptr(self, location=ProcessingUnit.HOST) -> int:
        p = ctypes.c_void_p()
        _check(self._prec.fn("transform_get_space_domain")(self._h, int(location), ctypes.byref(p)))
        return p.value or 0

    def space_domain(self, location=ProcessingUnit.HOST):
        """View of the space-domain slab [local_z][y][x] (complex, or real for R2C).

        HOST: numpy array; GPU: torch tensor on the grid's device (zero copy).
        The view is created once per location and reused (the slab never moves)."""
        v = self._views.get(int(location))
        if v is None:
            v = self._make_view(location)
            self._views[int(location)] = v
        return v

    def _make_view(self, location):
        shape = self.space_domain_shape()
        real = self.type == TransformType.R2C
        ptr = self.space_domain_ptr(location)
        count = int(np.prod(shape))
        if ProcessingUnit(location) == ProcessingUnit.HOST:
            dtype = self._prec.real if real else self._prec.complex
            if count == 0 or not ptr:
                return np.zeros(shape, dtype=dtype)
            buf = (ctypes.c_byte * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            buf._owner = self  # the view keeps the transform (and its grid) alive
            arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
            return arr
        from .ops._dlpack import capsule_to_torch
        m = ctypes.c_void_p()
        _check(self._prec.amd_fn("transform_space_domain_dlpack")(self._h, int(location),
                                                                  ctypes.byref(m)))
        return capsule_to_torch(m.value)

    def _default_output(self):
        n = self.num_local_elements
        if self.processing_unit == ProcessingUnit.GPU and torch is not None:
            return torch.empty(n, dtype=self._prec.torch_complex, device=f"cuda:{self.device_id}")
        return np.empty(n, dtype=self._prec.complex)

    def backward(self, values, output_location=None):
        """Frequency -> space. Returns the space-domain view at `output_location`."""
        if output_location is None:
            output_location = self.processing_unit
        ptr, keep = _data_ptr(values, self._prec, False, "values")
        _check(self._prec.fn("transform_backward")(self._h, ptr, int(output_location)))
        del keep
        return self.space_domain(output_location)

    def forward(self, space=None, output=None, input_location=None, scaling=Scaling.NONE):
        """Space -> frequency. `space` (optional) is copied into the space domain first.

        Returns the frequency values (in index-triplet order)."""
        if input_location is None:
            input_location = self.processing_unit
        if space is not None:
            dst = self.space_domain(input_location)
            if _is_torch(dst):
                dst.copy_(space if _is_torch(space) else torch.as_tensor(np.asarray(space)))
            else:
                src = space.cpu().numpy() if _is_torch(space) else np.asarray(space)
                np.copyto(dst, src.reshape(dst.shape), casting="same_kind")
        if output is None:
            output = self._default_output()
        ptr, keep = _data_ptr(output, self._prec, True, "output")
        _check(self._prec.fn("transform_forward")(self._h, int(input_location), ptr, int(scaling)))
        del keep
        return output

    def apply_local(self, values, potential, output=None, scaling=Scaling.NONE):
        """Local operator in one call: forward(potential * backward(values)).

        `potential` is a real array (numpy or torch, host or device memory) of shape
        space_domain_shape() and the transform's precision. `output` may be `values`.
        The contents of the space domain are unspecified afterwards; fused plans
        (see apply_local_fused) never form it and leave it untouched. Returns the
        frequency values."""
        vptr, vkeep = _potential_ptr(potential, self._prec, self.space_domain_shape())
        iptr, ikeep = _data_ptr(values, self._prec, False, "values")
        if output is None:
            output = self._default_output()
        optr, okeep = _data_ptr(output, self._prec, True, "output")
        _check(self._prec.amd_fn("transform_apply_local")(self._h, iptr, vptr, optr, int(scaling)))
        # asynchronous execution (set_stream(..., synchronous=False)) may still read them
        self._step_keep = (ikeep, vkeep, okeep)
        return output

    @property
    def apply_local_fused(self) -> bool:
        """True if apply_local runs the fused x stage (GPU; C2C with x lines of one workgroup,
        or R2C with even dim_x whose half-length has a compile-time kernel)."""
        c = self._cache.get("apply_local_fused")
        if c is None:
            v = ctypes.c_int()
            _check(self._prec.amd_fn("transform_apply_local_fused")(self._h, ctypes.byref(v)))
            c = self._cache["apply_local_fused"] = bool(v.value)
        return c

    def accumulate_density(self, values, weight, density):
        """density += weight * |backward(values)|**2 in one call (R2C: weight * s**2).

        `density` is a real array (numpy or torch, host or device memory) of shape
        space_domain_shape() and the transform's precision; it is updated in place,
        never zeroed and never copied. `values` is not modified. The contents of the
        space domain are unspecified afterwards; fused plans (see density_fused) never
        form it and leave it untouched. Returns `density`."""
        rptr, rkeep = _density_ptr(density, self._prec, self.space_domain_shape())
        iptr, ikeep = _data_ptr(values, self._prec, False, "values")
        _check(self._prec.amd_fn("transform_accumulate_density")(self._h, iptr, float(weight), rptr))
        # asynchronous execution (set_stream(..., synchronous=False)) may still use them
        self._step_keep = (ikeep, rkeep)
        return density

    @property
    def density_fused(self) -> bool:
        """True if accumulate_density runs the fused x stage (GPU; C2C with x lines of one
        workgroup, or R2C with even dim_x whose half-length has a compile-time kernel)."""
        c = self._cache.get("density_fused")
        if c is None:
            v = ctypes.c_int()
            _check(self._prec.amd_fn("transform_density_fused")(self._h, ctypes.byref(v)))
            c = self._cache["density_fused"] = bool(v.value)
        return c

    def apply_reciprocal(self, kernel, space=None, values=None, location=None,
                         scaling=Scaling.NONE):
        """Reciprocal-space operator in one call: the space domain f becomes
        backward(kernel * forward(f, scaling)).

        `kernel` is a real or complex array (numpy or torch, host or device memory) of
        the transform's precision with one entry per local frequency value, in the order
        of the index triplets (the order of forward's output). `space` (optional) is
        copied into the space domain first. `values` (optional, complex, length
        num_local_elements) receives the scaled forward values before the multiply.
        `location` is where the space domain is read and written. Fused plans (see
        reciprocal_fused) run both z FFTs and the multiply in one kernel. Returns the
        space-domain view at `location`."""
        if location is None:
            location = self.processing_unit
        kptr, kkeep, cplx = _kernel_ptr(kernel, self._prec, self.num_local_elements)
        if values is not None:
            n = values.numel() if _is_torch(values) else np.asarray(values).size
            if _is_torch(values) and values.dtype != self._prec.torch_complex:
                raise TypeError(f"values: expected {self._prec.torch_complex}, got {values.dtype}")
            if not _is_torch(values) and np.asarray(values).dtype != self._prec.complex:
                raise TypeError(f"values: expected {np.dtype(self._prec.complex)}, "
                                f"got {np.asarray(values).dtype}")
            if n != self.num_local_elements:
                raise ValueError(f"values: expected {self.num_local_elements} entries, got {n}")
        vptr, vkeep = _data_ptr(values, self._prec, True, "values")
        if space is not None:
            dst = self.space_domain(location)
            if _is_torch(dst):
                dst.copy_(space if _is_torch(space) else torch.as_tensor(np.asarray(space)))
            else:
                src = space.cpu().numpy() if _is_torch(space) else np.asarray(space)
                np.copyto(dst, src.reshape(dst.shape), casting="same_kind")
        _check(self._prec.amd_fn("transform_apply_reciprocal")(self._h, int(location), kptr,
                                                               1 if cplx else 0, vptr, int(scaling)))
        # asynchronous execution (set_stream(..., synchronous=False)) may still use them
        self._step_keep = (kkeep, vkeep)
        return self.space_domain(location)

    @property
    def reciprocal_fused(self) -> bool:
        """True if apply_reciprocal runs the fused z stage (GPU, simple sticks, z lines of
        one workgroup, no *_FLOAT exchange of either precision, no peer-written stick side)."""
        c = self._cache.get("reciprocal_fused")
        if c is None:
            v = ctypes.c_int()
            _check(self._prec.amd_fn("transform_reciprocal_fused")(self._h, ctypes.byref(v)))
            c = self._cache["reciprocal_fused"] = bool(v.value)
        return c

    def reciprocal_fan_fused(self, n: int) -> bool:
        """True if this transform and n - 1 clones of it, called with device arrays, run the
        fused z kernel of multi_transform_reciprocal_fan_out / fan_in (reciprocal_fused
        plans on one GPU without exchange, 2 <= n <= 8, z lines that fit a workgroup's LDS
        twice, SPFFT_BATCH not 0); n == 1 follows reciprocal_fused."""
        v = ctypes.c_int()
        _check(self._prec.amd_fn("transform_reciprocal_fan_fused")(self._h, int(n), ctypes.byref(v)))
        return bool(v.value)

    @property
    def spinor_fused(self) -> bool:
        """True if this transform and a clone of it, called with device arrays, run the
        fused spinor x kernels of multi_transform_apply_local_spinor /
        multi_transform_accumulate_spin_density (C2C plans on one GPU without exchange,
        fused x stages, x lines that fit a workgroup's LDS twice, SPFFT_BATCH on)."""
        c = self._cache.get("spinor_fused")
        if c is None:
            v = ctypes.c_int()
            _check(self._prec.amd_fn("transform_spinor_fused")(self._h, ctypes.byref(v)))
            c = self._cache["spinor_fused"] = bool(v.value)
        return c

    def values_fan_fused(self, n: int) -> bool:
        """True if this transform and n - 1 clones of it, called with device arrays, run the
        fused z fan kernels of multi_transform_accumulate_density_fan /
        multi_transform_apply_local_fan (C2C plans on one GPU without exchange, simple
        sticks, fused x stages, 1 <= n <= 8, z lines that fit a workgroup's LDS twice,
        SPFFT_BATCH not 0)."""
        v = ctypes.c_int()
        _check(self._prec.amd_fn("transform_values_fan_fused")(self._h, int(n), ctypes.byref(v)))
        return bool(v.value)

    def accumulate_fock(self, a, b, kernel, weight, acc, values=None, scaling=Scaling.NONE):
        """Exchange (Fock) pair operator in one call:
        acc += weight * a * backward(kernel * forward(conj(a) * b, scaling)).

        `a`, `b` and `acc` are arrays (numpy or torch, host or device memory) of shape
        space_domain_shape() in the transform's precision: complex for C2C, real for R2C
        (conj is then the identity). `a` and `b` are not modified and may be the same
        array; `acc` is updated in place, never copied, and must not overlap them.
        `kernel` and `values` are as in apply_reciprocal; `values` receives the scaled
        forward values c(G) of the pair density. The contents of the space domain are
        unspecified afterwards; fused plans (see fock_fused for C2C and fock_r2c_fused for
        R2C) never form it and leave it untouched. On a fused R2C plan `a`, `b` and `acc`
        are accessed as pairs of elements: a device array not aligned to two elements makes
        the half of the call that uses it run composed, through the space domain. Returns
        `acc`."""
        shape = self.space_domain_shape()
        real = self.type == TransformType.R2C
        aptr, akeep = _space_array_ptr(a, self._prec, shape, real, "a", False)
        if b is a:
            bptr, bkeep = aptr, akeep
        else:
            bptr, bkeep = _space_array_ptr(b, self._prec, shape, real, "b", False)
        cptr, ckeep = _space_array_ptr(acc, self._prec, shape, real, "acc", True)
        kptr, kkeep, cplx = _kernel_ptr(kernel, self._prec, self.num_local_elements)
        if values is not None:
            n = values.numel() if _is_torch(values) else np.asarray(values).size
            if _is_torch(values) and values.dtype != self._prec.torch_complex:
                raise TypeError(f"values: expected {self._prec.torch_complex}, got {values.dtype}")
            if not _is_torch(values) and np.asarray(values).dtype != self._prec.complex:
                raise TypeError(f"values: expected {np.dtype(self._prec.complex)}, "
                                f"got {np.asarray(values).dtype}")
            if n != self.num_local_elements:
                raise ValueError(f"values: expected {self.num_local_elements} entries, got {n}")
        vptr, vkeep = _data_ptr(values, self._prec, True, "values")
        if Scaling(scaling) not in (Scaling.NONE, Scaling.FULL):
            raise ValueError(f"scaling: expected Scaling.NONE or Scaling.FULL, got {scaling}")
        _check(self._prec.amd_fn("transform_accumulate_fock")(
            self._h, aptr, bptr, kptr, 1 if cplx else 0, float(weight), cptr, vptr, int(scaling)))
        # asynchronous execution (set_stream(..., synchronous=False)) may still use them
        self._step_keep = (akeep, bkeep, kkeep, ckeep, vkeep)
        return acc

    @property
    def fock_fused(self) -> bool:
        """True if accumulate_fock runs the fused C2C pair x stages (GPU, C2C, x lines of one
        workgroup); its z stage follows reciprocal_fused. False on every R2C plan: see
        fock_r2c_fused."""
        c = self._cache.get("fock_fused")
        if c is None:
            v = ctypes.c_int()
            _check(self._prec.amd_fn("transform_fock_fused")(self._h, ctypes.byref(v)))
            c = self._cache["fock_fused"] = bool(v.value)
        return c

    @property
    def fock_r2c_fused(self) -> bool:
        """True if accumulate_fock runs the packed-real pair x stages (GPU, R2C with even
        dim_x whose half-length has a compile-time kernel; SPFFT_R2C_FUSE=0 or
        SPFFT_R2C_PACKED=0 at creation keeps the composed path)."""
        c = self._cache.get("fock_r2c_fused")
        if c is None:
            v = ctypes.c_int()
            _check(self._prec.amd_fn("transform_fock_r2c_fused")(self._h, ctypes.byref(v)))
            c = self._cache["fock_r2c_fused"] = bool(v.value)
        return c

    # --------------------------------------------------- streams / step API
    def set_stream(self, stream=None, synchronous: bool = True):
        """Execute on a HIP stream (int handle or torch.cuda.Stream; 0 = legacy default
        stream). None returns to the library's private stream."""
        if stream is None:
            self._stream = None
            _check(self._prec.amd_fn("transform_reset_stream")(self._h))
            return
        if not isinstance(stream, int):
            stream = stream.cuda_stream
        self._stream = stream
        _check(self._prec.amd_fn("transform_set_stream")(self._h, stream or None,
                                                        1 if synchronous else 0))

    def synchronize(self):
        _check(self._prec.amd_fn("transform_synchronize")(self._h))

    # Step-wise execution (spfft/amd.h): backward = backward_z, backward_exchange,
    # backward_xy; forward = forward_xy, forward_exchange, forward_z. Every rank calls
    # the same steps in the same order (the exchanges are collective); work that does
    # not depend on the exchange can be placed between the steps.
    def backward_z(self, values):
        ptr, keep = _data_ptr(values, self._prec, False, "values")
        _check(self._prec.amd_fn("transform_backward_z")(self._h, ptr))
        self._step_keep = keep  # until the next step: the z stage may still read it

    def backward_exchange(self, non_blocking: bool = False):
        _check(self._prec.amd_fn("transform_backward_exchange")(self._h, 1 if non_blocking else 0))

    def backward_xy(self, output_location=None):
        if output_location is None:
            output_location = self.processing_unit
        _check(self._prec.amd_fn("transform_backward_xy")(self._h, int(output_location)))
        self._step_keep = None
        return self.space_domain(output_location)

    def forward_xy(self, input_location=None):
        if input_location is None:
            input_location = self.processing_unit
        _check(self._prec.amd_fn("transform_forward_xy")(self._h, int(input_location)))

    def forward_exchange(self, non_blocking: bool = False):
        _check(self._prec.amd_fn("transform_forward_exchange")(self._h, 1 if non_blocking else 0))

    def forward_z(self, output=None, scaling=Scaling.NONE):
        if output is None:
            output = self._default_output()
        ptr, keep = _data_ptr(output, self._prec, True, "output")
        _check(self._prec.amd_fn("transform_forward_z")(self._h, ptr, int(scaling)))
        self._step_keep = keep
        return output

    def exchange_plan(self):
        """(plane chunks K, stick blocks I, peer writes, relay GPUs) of the GPU exchange."""
        k, i, pw, rl = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(self._prec.amd_fn("transform_exchange_plan")(self._h, ctypes.byref(k), ctypes.byref(i),
                                                            ctypes.byref(pw), ctypes.byref(rl)))
        return k.value, i.value, bool(pw.value), rl.value

    def rank_z_range(self, rank: int):
        off, ln = ctypes.c_int(), ctypes.c_int()
        _check(lib().spfft_amd_transform_local_z_offset_rank(self._h, rank, ctypes.byref(off),
                                                             ctypes.byref(ln)))
        return off.value, ln.value


class Transform(_TransformBase):
    _single = False


class TransformFloat(_TransformBase):
    _single = True


def _multi(transforms: Sequence[_TransformBase]):
    n = len(transforms)
    single = transforms[0]._single if n else False
    prec = _Precision(single)
    arr = (ctypes.c_void_p * max(1, n))(*[t.handle.value for t in transforms])
    return n, prec, arr


def multi_transform_backward(transforms, inputs, output_locations=None):
    """Backward transforms of several independent transforms (distinct grids), overlapped."""
    n, prec, arr = _multi(transforms)
    if output_locations is None:
        output_locations = [t.processing_unit for t in transforms]
    keeps, ptrs = [], (ctypes.c_void_p * max(1, n))()
    for i, v in enumerate(inputs):
        p, k = _data_ptr(v, prec, False, "values")
        ptrs[i] = p
        keeps.append(k)
    locs = (ctypes.c_int * max(1, n))(*[int(x) for x in output_locations])
    _check(prec.fn("multi_transform_backward")(n, arr, ptrs, locs))
    return [t.space_domain(loc) for t, loc in zip(transforms, output_locations)]


def multi_transform_forward(transforms, outputs=None, input_locations=None, scalings=None):
    n, prec, arr = _multi(transforms)
    if input_locations is None:
        input_locations = [t.processing_unit for t in transforms]
    if scalings is None:
        scalings = [Scaling.NONE] * n
    if outputs is None:
        outputs = [t._default_output() for t in transforms]
    keeps, ptrs = [], (ctypes.c_void_p * max(1, n))()
    for i, v in enumerate(outputs):
        p, k = _data_ptr(v, prec, True, "output")
        ptrs[i] = p
        keeps.append(k)
    locs = (ctypes.c_int * max(1, n))(*[int(x) for x in input_locations])
    scs = (ctypes.c_int * max(1, n))(*[int(x) for x in scalings])
    _check(prec.fn("multi_transform_forward")(n, arr, locs, ptrs, scs))
    return outputs


def multi_transform_apply_local(transforms, inputs, potentials, outputs=None, scalings=None):
    """apply_local of several independent transforms (distinct grids), overlapped;
    identical fused plans on one GPU share one launch per stage."""
    n, prec, arr = _multi(transforms)
    if len(inputs) != n or len(potentials) != n:
        raise ValueError("one input and one potential per transform")
    if scalings is None:
        scalings = [Scaling.NONE] * n
    if outputs is None:
        outputs = [t._default_output() for t in transforms]
    keeps = []
    iptrs, vptrs, optrs = ((ctypes.c_void_p * max(1, n))() for _ in range(3))
    for i, t in enumerate(transforms):
        vptrs[i], k = _potential_ptr(potentials[i], prec, t.space_domain_shape())
        keeps.append(k)
        iptrs[i], k = _data_ptr(inputs[i], prec, False, "values")
        keeps.append(k)
        optrs[i], k = _data_ptr(outputs[i], prec, True, "output")
        keeps.append(k)
    scs = (ctypes.c_int * max(1, n))(*[int(x) for x in scalings])
    _check(prec.amd_fn("multi_transform_apply_local")(n, arr, iptrs, vptrs, optrs, scs))
    for t in transforms:
        t._step_keep = keeps
    return outputs


def multi_transform_accumulate_density(transforms, inputs, weights, density):
    """density += sum_i weights[i] * |backward_i(inputs[i])|**2 of several independent
    transforms (distinct grids, one space domain shape) into one shared `density`,
    overlapped; identical fused plans on one GPU share one launch per stage. The sum
    order is fixed by the call. Returns `density`."""
    n, prec, arr = _multi(transforms)
    if len(inputs) != n or len(weights) != n:
        raise ValueError("one input and one weight per transform")
    if any(t._single != prec.single for t in transforms):
        raise TypeError("transforms of one call share one precision")
    shape = transforms[0].space_domain_shape() if n else None
    if any(tuple(t.space_domain_shape()) != tuple(shape) for t in transforms):
        raise ValueError("transforms of one call share one space domain shape")
    rptr, rkeep = _density_ptr(density, prec, shape) if n else (None, None)
    keeps = [rkeep]
    iptrs = (ctypes.c_void_p * max(1, n))()
    for i in range(n):
        iptrs[i], k = _data_ptr(inputs[i], prec, False, "values")
        keeps.append(k)
    ws = ((ctypes.c_float if prec.single else ctypes.c_double) * max(1, n))(
        *[float(w) for w in weights])
    _check(prec.amd_fn("multi_transform_accumulate_density")(
        n, arr, iptrs, ctypes.cast(ws, ctypes.c_void_p), rptr))
    for t in transforms:
        t._step_keep = keeps
    return density


def multi_transform_accumulate_fock(transforms, a, b, kernel, weights, acc, scaling=Scaling.NONE):
    """acc += sum_i weights[i] * a[i] * backward_i(kernel_i * forward_i(conj(a[i]) * b[i],
    scaling)) of several independent transforms (distinct grids, one space domain shape,
    all C2C or all R2C) into one shared `acc`: the exchange pairs of one band in one call.
    `a` and `b` hold one array per transform as in accumulate_fock (`b[i]` may be the same
    array for every i, and may be `a[i]`); `kernel` is one array or tensor shared by all
    transforms or a sequence of one per transform, all real or all complex. Identical
    fused plans on one GPU (fock_fused, or fock_r2c_fused on R2C) share one launch per
    stage, and their updates of `acc` run inside one workgroup per tile; the sum order is
    fixed by the call. An R2C member whose `a[i]`, `b[i]` or `acc` is not aligned to two
    elements runs per transform instead. Returns `acc`."""
    n, prec, arr = _multi(transforms)
    if len(a) != n or len(b) != n or len(weights) != n:
        raise ValueError("one a, one b and one weight per transform")
    if _is_torch(kernel) or isinstance(kernel, np.ndarray):
        kernels = [kernel] * n
    else:
        kernels = list(kernel)
        if len(kernels) != n:
            raise ValueError("one kernel for all transforms, or one per transform")
    if any(t._single != prec.single for t in transforms):
        raise TypeError("transforms of one call share one precision")
    shape = transforms[0].space_domain_shape() if n else None
    if any(tuple(t.space_domain_shape()) != tuple(shape) for t in transforms):
        raise ValueError("transforms of one call share one space domain shape")
    real = transforms[0].type == TransformType.R2C if n else False
    if any((t.type == TransformType.R2C) != real for t in transforms):
        raise ValueError("transforms of one call are all C2C or all R2C")
    if Scaling(scaling) not in (Scaling.NONE, Scaling.FULL):
        raise ValueError(f"scaling: expected Scaling.NONE or Scaling.FULL, got {scaling}")
    cptr, ckeep = _space_array_ptr(acc, prec, shape, real, "acc", True) if n else (None, None)
    keeps = [ckeep]
    aptrs, bptrs, kptrs = ((ctypes.c_void_p * max(1, n))() for _ in range(3))
    cplx = None
    for i, t in enumerate(transforms):
        aptrs[i], akeep = _space_array_ptr(a[i], prec, shape, real, "a", False)
        if b[i] is a[i]:
            bptrs[i], bkeep = aptrs[i], akeep
        elif i > 0 and b[i] is b[0]:
            bptrs[i], bkeep = bptrs[0], None
        else:
            bptrs[i], bkeep = _space_array_ptr(b[i], prec, shape, real, "b", False)
        if (i > 0 and kernels[i] is kernels[0]
                and t.num_local_elements == transforms[0].num_local_elements):
            kptrs[i], kkeep, c = kptrs[0], None, cplx  # one conversion, one pointer
        else:
            kptrs[i], kkeep, c = _kernel_ptr(kernels[i], prec, t.num_local_elements)
        if cplx is None:
            cplx = c
        elif c != cplx:
            raise TypeError("kernels of one call are all real or all complex")
        keeps += [akeep, bkeep, kkeep]
    ws = ((ctypes.c_float if prec.single else ctypes.c_double) * max(1, n))(
        *[float(w) for w in weights])
    _check(prec.amd_fn("multi_transform_accumulate_fock")(
        n, arr, aptrs, bptrs, kptrs, 1 if cplx else 0, ctypes.cast(ws, ctypes.c_void_p), cptr,
        int(scaling)))
    # asynchronous execution (set_stream(..., synchronous=False)) may still use them
    for t in transforms:
        t._step_keep = keeps
    return acc


def _fan_args(transforms, kernels, what):
    """Handles, kernel pointers and keepalives shared by the two fan operators."""
    n, prec, arr = _multi(transforms)
    if _is_torch(kernels) or isinstance(kernels, np.ndarray):
        raise TypeError(f"{what}: kernels is a sequence of one array per transform")
    kernels = list(kernels)
    if len(kernels) != n:
        raise ValueError(f"{what}: one kernel per transform")
    if any(t._single != prec.single for t in transforms):
        raise TypeError("transforms of one call share one precision")
    kptrs = (ctypes.c_void_p * max(1, n))()
    keeps, cplx, seen = [], None, {}
    for i, t in enumerate(transforms):
        first = seen.get(id(kernels[i]))
        if first is not None and t.num_local_elements == transforms[first].num_local_elements:
            kptrs[i], kkeep, c = kptrs[first], None, cplx  # one conversion, one pointer
        else:
            kptrs[i], kkeep, c = _kernel_ptr(kernels[i], prec, t.num_local_elements)
            seen[id(kernels[i])] = i
        if cplx is None:
            cplx = c
        elif c != cplx:
            raise TypeError("kernels of one call are all real or all complex")
        keeps.append(kkeep)
    return n, prec, arr, kptrs, bool(cplx), keeps


def _fill_space(t, space, location):
    dst = t.space_domain(location)
    if _is_torch(dst):
        dst.copy_(space if _is_torch(space) else torch.as_tensor(np.asarray(space)))
    else:
        src = space.cpu().numpy() if _is_torch(space) else np.asarray(space)
        np.copyto(dst, src.reshape(dst.shape), casting="same_kind")


def multi_transform_reciprocal_fan_out(transforms, kernels, space=None, values=None, location=None,
                                       scaling=Scaling.NONE):
    """Reciprocal fan-out (gradient-like) in one call: with c = forward(f, scaling) of the
    space domain f of transforms[0], the space domain of transforms[i] becomes
    backward(kernels[i] * c) for every i; member 0's space domain is input and result.

    The transforms live on distinct grids (a transform and its clones) and have equal
    dimensions, type and index sets sizes; `kernels` holds one real or complex array per
    transform as in apply_reciprocal (all real or all complex; the same array may be given
    several times). `space` (optional) is copied into member 0's space domain first,
    `values` (optional) receives c. `location` is where the space domains are read and
    written (default: member 0's processing unit). Identical fused plans on one GPU (see
    Transform.reciprocal_fan_fused) run one forward transform, one z kernel that writes
    every member's sticks, and one batched launch per backward stage. Returns the list of
    space-domain views at `location`."""
    n, prec, arr, kptrs, cplx, keeps = _fan_args(transforms, kernels, "reciprocal_fan_out")
    if n == 0:
        _check(prec.amd_fn("multi_transform_reciprocal_fan_out")(0, arr, 1, kptrs, 0, None, int(scaling)))
        return []
    if location is None:
        location = transforms[0].processing_unit
    if values is not None:
        t0 = transforms[0]
        cnt = values.numel() if _is_torch(values) else np.asarray(values).size
        dt = values.dtype if _is_torch(values) else np.asarray(values).dtype
        if dt != (prec.torch_complex if _is_torch(values) else prec.complex):
            raise TypeError(f"values: expected complex of the transforms' precision, got {dt}")
        if cnt != t0.num_local_elements:
            raise ValueError(f"values: expected {t0.num_local_elements} entries, got {cnt}")
    vptr, vkeep = _data_ptr(values, prec, True, "values")
    if space is not None:
        _fill_space(transforms[0], space, location)
    _check(prec.amd_fn("multi_transform_reciprocal_fan_out")(
        n, arr, int(location), kptrs, 1 if cplx else 0, vptr, int(scaling)))
    # asynchronous execution (set_stream(..., synchronous=False)) may still use them
    for t in transforms:
        t._step_keep = (keeps, vkeep)
    return [t.space_domain(location) for t in transforms]


def multi_transform_reciprocal_fan_in(transforms, kernels, spaces=None, location=None,
                                      scaling=Scaling.NONE):
    """Reciprocal fan-in (divergence-like) in one call: the space domain of transforms[0]
    becomes backward(sum_i kernels[i] * forward_i(f_i, scaling)) with f_i the space domain
    of transforms[i], summed in list order; the space domains of the other members are
    left unchanged.

    Transforms, `kernels`, `location` and the fused path are as in
    multi_transform_reciprocal_fan_out. `spaces` (optional) holds one array per transform
    (or None to keep a member's contents), copied into the space domains first. The sum
    order is fixed by the call: the same call on the same data gives the same bits.
    Returns the space-domain view of member 0 at `location`."""
    n, prec, arr, kptrs, cplx, keeps = _fan_args(transforms, kernels, "reciprocal_fan_in")
    if n == 0:
        _check(prec.amd_fn("multi_transform_reciprocal_fan_in")(0, arr, 1, kptrs, 0, int(scaling)))
        return None
    if location is None:
        location = transforms[0].processing_unit
    if spaces is not None:
        if len(spaces) != n:
            raise ValueError("reciprocal_fan_in: one space array (or None) per transform")
        for t, s in zip(transforms, spaces):
            if s is not None:
                _fill_space(t, s, location)
    _check(prec.amd_fn("multi_transform_reciprocal_fan_in")(
        n, arr, int(location), kptrs, 1 if cplx else 0, int(scaling)))
    for t in transforms:
        t._step_keep = (keeps,)
    return transforms[0].space_domain(location)


def _values_fan_kernels(transforms, prec, lists, what):
    """Kernel pointer arrays of the value fans: one array per list, None entries are the
    identity (a null pointer). Returns (pointer arrays, is_complex, keepalives)."""
    n = len(transforms)
    arrays, keeps, cplx = [], [], None
    for kernels in lists:
        if _is_torch(kernels) or isinstance(kernels, np.ndarray):
            raise TypeError(f"{what}: kernels is a sequence of one array (or None) per transform")
        kernels = list(kernels)
        if len(kernels) != n:
            raise ValueError(f"{what}: one kernel (or None) per transform")
        ptrs, seen = (ctypes.c_void_p * max(1, n))(), {}
        for i, t in enumerate(transforms):
            if kernels[i] is None:
                continue
            first = seen.get(id(kernels[i]))
            if first is not None:
                ptrs[i] = ptrs[first]  # one conversion, one pointer
                continue
            ptrs[i], kkeep, c = _kernel_ptr(kernels[i], prec, t.num_local_elements)
            seen[id(kernels[i])] = i
            keeps.append(kkeep)
            if cplx is None:
                cplx = c
            elif c != cplx:
                raise TypeError("kernels of one call are all real or all complex")
        arrays.append(ptrs)
    return arrays, bool(cplx), keeps


def _values_fan_common(transforms, values, what):
    n, prec, arr = _multi(transforms)
    if any(t._single != prec.single for t in transforms):
        raise TypeError("transforms of one call share one precision")
    if any(t.num_local_elements != transforms[0].num_local_elements for t in transforms):
        raise ValueError(f"{what}: transforms of one call share one index set size")
    if n and values is not None:
        cnt = values.numel() if _is_torch(values) else np.asarray(values).size
        if cnt != transforms[0].num_local_elements:
            raise ValueError(f"values: expected {transforms[0].num_local_elements} entries, got {cnt}")
    return n, prec, arr


def multi_transform_accumulate_density_fan(transforms, values, kernels, weights, density):
    """Density fan in one call: density += sum_i weights[i] * |backward_i(kernels[i] *
    values)|**2, in list order, for one array of frequency values and one kernel per
    transform (the kinetic-energy density with kernels i G_d).

    The transforms live on distinct grids (a transform and its clones) and have equal
    dimensions, type and index set sizes. `kernels` holds one real or complex array per
    transform as in apply_reciprocal (all real or all complex; the same array may be given
    several times); a None entry is the identity. `weights` and `density` are as in
    multi_transform_accumulate_density: `density` is updated in place and never zeroed;
    `values` is not modified. Identical fused plans on one GPU (see
    Transform.values_fan_fused) run one z kernel that writes every member's sticks and one
    launch per later stage. The sum order is fixed by the call. Returns `density`."""
    n, prec, arr = _values_fan_common(transforms, values, "accumulate_density_fan")
    if len(weights) != n:
        raise ValueError("accumulate_density_fan: one weight per transform")
    (kptrs,), cplx, keeps = _values_fan_kernels(transforms, prec, (kernels,), "accumulate_density_fan")
    shape = transforms[0].space_domain_shape() if n else None
    if any(tuple(t.space_domain_shape()) != tuple(shape) for t in transforms):
        raise ValueError("transforms of one call share one space domain shape")
    rptr, rkeep = _density_ptr(density, prec, shape) if n else (None, None)
    iptr, ikeep = _data_ptr(values, prec, False, "values") if n else (None, None)
    ws = ((ctypes.c_float if prec.single else ctypes.c_double) * max(1, n))(*[float(w) for w in weights])
    _check(prec.amd_fn("multi_transform_accumulate_density_fan")(
        n, arr, iptr, kptrs, 1 if cplx else 0, ctypes.cast(ws, ctypes.c_void_p), rptr))
    # asynchronous execution (set_stream(..., synchronous=False)) may still use them
    for t in transforms:
        t._step_keep = (keeps, ikeep, rkeep)
    return density


def multi_transform_apply_local_fan(transforms, values, kernels_in, potentials, kernels_out, output=None,
                                    scaling=Scaling.NONE):
    """Apply-local fan in one call: output = sum_i kernels_out[i] * forward_i(potentials[i] *
    backward_i(kernels_in[i] * values), scaling), in list order (the local part of a
    meta-GGA Hamiltonian: member 0 with None kernels is apply_local, the others carry
    i G_d on both sides and the potential V_tau).

    Transforms, kernel lists (None entries are the identity; both lists all real or all
    complex) and the fused path are as in multi_transform_accumulate_density_fan;
    `potentials` holds one real array of space_domain_shape() per transform (the same
    array may be given several times). `output` may be `values`; `values` is otherwise
    not modified. The sum order is fixed by the call. Returns the frequency values."""
    n, prec, arr = _values_fan_common(transforms, values, "apply_local_fan")
    potentials = list(potentials)
    if len(potentials) != n:
        raise ValueError("apply_local_fan: one potential per transform")
    (kin, kout), cplx, keeps = _values_fan_kernels(transforms, prec, (kernels_in, kernels_out),
                                                   "apply_local_fan")
    vptrs = (ctypes.c_void_p * max(1, n))()
    for i, t in enumerate(transforms):
        vptrs[i], k = _potential_ptr(potentials[i], prec, t.space_domain_shape())
        keeps.append(k)
    if n == 0:
        _check(prec.amd_fn("multi_transform_apply_local_fan")(0, arr, None, kin, vptrs, kout, 0, None,
                                                              int(scaling)))
        return output
    if output is None:
        output = transforms[0]._default_output()
    iptr, ikeep = _data_ptr(values, prec, False, "values")
    optr, okeep = _data_ptr(output, prec, True, "output")
    _check(prec.amd_fn("multi_transform_apply_local_fan")(
        n, arr, iptr, kin, vptrs, kout, 1 if cplx else 0, optr, int(scaling)))
    for t in transforms:
        t._step_keep = (keeps, ikeep, okeep)
    return output


def _four_arrays(x, prec, shape, what, ptr_fn):
    """Pointer array and keepalives of the four real space-domain arrays of a spinor call:
    a real [4, z, y, x] array or tensor, or a sequence of four arrays of `shape`."""
    if _is_torch(x) or isinstance(x, np.ndarray):
        if x.ndim != 4 or x.shape[0] != 4:
            raise ValueError(f"{what}: expected shape (4, {', '.join(str(d) for d in shape)}), "
                             f"got {tuple(x.shape)}")
        if not (x.is_contiguous() if _is_torch(x) else x.flags.c_contiguous):
            raise ValueError(f"{what} must be contiguous")
        parts = [x[k] for k in range(4)]
    else:
        parts = list(x)
        if len(parts) != 4:
            raise ValueError(f"{what}: expected four arrays, got {len(parts)}")
    ptrs, keeps = (ctypes.c_void_p * 4)(), []
    for k in range(4):
        ptrs[k], keep = ptr_fn(parts[k], prec, shape)
        keeps.append(keep)
    return ptrs, keeps


def _spinor_common(transforms, inputs, what):
    n, prec, arr = _multi(transforms)
    if n % 2:
        raise ValueError(f"{what}: two transforms (up, down) per spinor")
    if len(inputs) != n:
        raise ValueError(f"{what}: one input per transform")
    if any(t._single != prec.single for t in transforms):
        raise TypeError("transforms of one call share one precision")
    shape = transforms[0].space_domain_shape() if n else None
    if any(tuple(t.space_domain_shape()) != tuple(shape) for t in transforms):
        raise ValueError("transforms of one call share one space domain shape")
    iptrs, keeps = (ctypes.c_void_p * max(1, n))(), []
    for i in range(n):
        iptrs[i], k = _data_ptr(inputs[i], prec, False, "values")
        keeps.append(k)
    return n, prec, arr, shape, iptrs, keeps


def multi_transform_apply_local_spinor(transforms, inputs, potential, outputs=None, scaling=Scaling.NONE):
    """The 2x2 Hermitian local potential applied to two-component spinors in one call.

    `transforms` holds two C2C transforms per spinor on distinct grids (a transform and
    its clones), in the order up_0, dn_0, up_1, dn_1, ...; `inputs` and `outputs` one array
    of frequency values per transform in that order. `potential` is a contiguous real
    [4, z, y, x] array or tensor, or a sequence of four arrays of space_domain_shape():
    (v_uu, v_dd, v_ud_re, v_ud_im) with v_ud = v_ud_re + i v_ud_im and v_du = conj(v_ud);
    for V * 1 + B . sigma that is v_uu = V + B_z, v_dd = V - B_z, v_ud_re = B_x,
    v_ud_im = -B_y. Per spinor, with psi = backward(input):

        out_up = forward_up(v_uu * psi_up + v_ud * psi_dn, scaling)
        out_dn = forward_dn(conj(v_ud) * psi_up + v_dd * psi_dn, scaling)

    An output may be its input; inputs are otherwise not modified. Identical fused plans on
    one GPU (see Transform.spinor_fused) with device arrays run one x kernel that holds both
    components of a tile in LDS between the batched z and y launches. Returns the outputs."""
    n, prec, arr, shape, iptrs, keeps = _spinor_common(transforms, inputs, "apply_local_spinor")
    if Scaling(scaling) not in (Scaling.NONE, Scaling.FULL):
        raise ValueError(f"scaling: expected Scaling.NONE or Scaling.FULL, got {scaling}")
    fn = prec.amd_fn("multi_transform_apply_local_spinor")
    if n == 0:
        _check(fn(0, arr, None, None, None, int(scaling)))
        return [] if outputs is None else outputs
    if outputs is None:
        outputs = [t._default_output() for t in transforms]
    if len(outputs) != n:
        raise ValueError("apply_local_spinor: one output per transform")
    vptrs, vkeeps = _four_arrays(potential, prec, shape, "potential", _potential_ptr)
    optrs = (ctypes.c_void_p * n)()
    for i in range(n):
        optrs[i], k = _data_ptr(outputs[i], prec, True, "output")
        keeps.append(k)
    _check(fn(n // 2, arr, iptrs, vptrs, optrs, int(scaling)))
    # asynchronous execution (set_stream(..., synchronous=False)) may still use them
    for t in transforms:
        t._step_keep = (keeps, vkeeps)
    return outputs


def multi_transform_accumulate_spin_density(transforms, inputs, weights, density):
    """The spin density matrix of two-component spinors, accumulated in one call.

    `transforms` and `inputs` are as in multi_transform_apply_local_spinor; `weights` holds
    one weight per spinor. `density` is a contiguous real [4, z, y, x] array or tensor, or a
    sequence of four distinct arrays of space_domain_shape(): (n_uu, n_dd, n_ud_re,
    n_ud_im), updated in place and never zeroed:

        n_uu += sum_s w_s |psi_up|^2,  n_dd += sum_s w_s |psi_dn|^2,
        n_ud += sum_s w_s psi_up * conj(psi_dn)

    in list order (the same call on the same data gives the same bits). The charge and
    magnetisation densities are n = n_uu + n_dd, m_z = n_uu - n_dd, m_x = 2 n_ud_re,
    m_y = -2 n_ud_im. Returns `density`."""
    n, prec, arr, shape, iptrs, keeps = _spinor_common(transforms, inputs, "accumulate_spin_density")
    if 2 * len(weights) != n:
        raise ValueError("accumulate_spin_density: one weight per spinor")
    fn = prec.amd_fn("multi_transform_accumulate_spin_density")
    if n == 0:
        _check(fn(0, arr, None, None, None))
        return density
    rptrs, rkeeps = _four_arrays(density, prec, shape, "density", _density_ptr)
    ws = ((ctypes.c_float if prec.single else ctypes.c_double) * (n // 2))(*[float(w) for w in weights])
    _check(fn(n // 2, arr, iptrs, ctypes.cast(ws, ctypes.c_void_p), rptrs))
    for t in transforms:
        t._step_keep = (keeps, rkeeps)
    return density
