"""What the satellite plan families share above the C ABI: the opaque handle with its error plumbing, the checks that stand between a
caller's array or tensor and a kernel that trusts its pointer, the custom-window marshaller, and the plan cache of the one-shot functions.

Every check of a device tensor runs in one order: on the plan's device, then rank and batch > 0, then dtype and layout.  `_ffi` re-exports
the names; import them from there.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _ffi


def dtype_name(code: int) -> str:
    """The public name of a dtype code (F32 / F64)."""
    return "float32" if code == _ffi.F32 else "float64"


def custom_window(window):
    """(keep_alive_array, POINTER(c_double), length) of a WindowType's coefficients for a create call: (None, None, 0) unless the
    window is a custom one.  The caller keeps the array alive across the call."""
    if window.kind != _ffi.WIN_CUSTOM:
        return None, None, 0
    cw = np.ascontiguousarray(window.coefficients, dtype=np.float64)
    return cw, cw.ctypes.data_as(C.POINTER(C.c_double)), cw.size


class NativeHandle:
    """One opaque plan of a satellite family of the C ABI.  A subclass names the family's symbol prefix (`_prefix`, e.g. "sgx_mdct"),
    sets `_lib` and `_dt` (the plan's dtype code) and passes its create call's status and handle to `_create`, which also reads the
    device the plan was bound to; every later status goes through `_check`.  Creation errors are read from <prefix>_last_error(NULL),
    call errors from the plan."""

    _prefix = ""
    _h = None
    _device = _ffi.DEVICE_HOST_ONLY

    def _last_error(self, handle) -> str:
        return (getattr(self._lib, self._prefix + "_last_error")(handle) or b"").decode()

    def _create(self, status: int, handle) -> None:
        if status:
            raise _ffi._ERR.get(status, _ffi.InternalError)(self._last_error(None))
        self._h = handle
        if self._prefix + "_device" in _ffi.SIGNATURES:
            self._device = int(getattr(self._lib, self._prefix + "_device")(handle))

    def _check(self, status: int) -> None:
        if status:
            raise _ffi._ERR.get(status, _ffi.InternalError)(self._last_error(self._h))

    def __del__(self):
        if self._h:
            getattr(self._lib, self._prefix + "_destroy")(self._h)
            self._h = None

    device = property(lambda self: self._device, doc="HIP device ordinal the plan is bound to (-2: host-only plan)")
    dtype = property(lambda self: dtype_name(self._dt))

    # ---- the plan's types in numpy and torch: real, then complex ------------------------------------------------------------
    @property
    def _np(self):
        return _ffi.np_dtype(self._dt)

    @property
    def _cdt(self):
        return np.complex64 if self._dt == _ffi.F32 else np.complex128

    @property
    def _tdt(self):
        import torch
        return torch.float32 if self._dt == _ffi.F32 else torch.float64

    @property
    def _tcdt(self):
        import torch
        return torch.complex64 if self._dt == _ffi.F32 else torch.complex128

    # ---- what a call hands to the library -------------------------------------------------------------------------------------
    def _stream(self, stream: int = 0, device=None):
        """The `void *stream` of a call: `stream` if given, else torch's current stream on `device` (default: the plan's device);
        None for a host-only plan."""
        if stream:
            return C.c_void_p(stream)
        if device is None:
            if self._device < 0:
                return None
            device = self._device
        import torch
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def _host_rows(self, x, what: str, ndims=(1, 2), dtype=None):
        """Host input -> (rows, squeezed): a C-contiguous array of `dtype` (default: the plan's) with the batch axis in front, and
        whether that axis was added here (the caller then returns `out[0]`).  `what` names the argument and one row's layout,
        e.g. "samples (n,)"."""
        a = np.ascontiguousarray(x, dtype=dtype or self._np)
        if a.ndim not in ndims:
            name, _, row = what.partition(" (")  # "ir (taps,)" -> "ir must be 1-D (taps,) or 2-D (batch, taps)"
            raise ValueError(f"{name} must be {ndims[0]}-D ({row} or {ndims[1]}-D (batch, {row.rstrip(',)')})")
        rows = a[None] if a.ndim == ndims[0] else a
        if rows.shape[0] == 0:
            raise ValueError("batch must be > 0")
        return rows, a.ndim == ndims[0]

    def _on_device(self, t, what: str) -> None:
        # the kernels run on the plan's device with the plan's tables: a tensor that lives elsewhere would be a wild pointer there
        if not t.is_cuda or t.device.index != self._device:
            raise ValueError(f"{what} is on {t.device}, the plan is bound to cuda:{self._device}")

    def _check_tensor(self, t, what: str, ndim: int, rows_may_stride: bool = False, dtype=None) -> int:
        """Device input -> the stride between its rows in elements (a row: one run along the last axis).  In this order: on the plan's
        device; `ndim`-D with batch > 0; of `dtype` (default: the plan's real one) and contiguous, or with `rows_may_stride` a slice
        `X[..., a:b]` of a contiguous tensor (unit inner stride, a row stride >= the row, nothing else between the rows)."""
        self._on_device(t, what)
        if t.dim() != ndim or t.shape[0] == 0:
            raise ValueError(f"{what} must be {ndim}-D with batch > 0, got shape {tuple(t.shape)}")
        n = t.shape[-1]
        stride = t.stride(-2) if t.shape[-2] > 1 else max(n, 1)
        strided_ok = rows_may_stride and (n <= 1 or t.stride(-1) == 1) and stride >= n and all(
            t.shape[k] <= 1 or t.stride(k) == t.shape[k + 1] * (stride if k == ndim - 3 else t.stride(k + 1)) for k in range(ndim - 2))
        if t.dtype != (dtype or self._tdt) or not (t.is_contiguous() or strided_ok):
            raise ValueError(f"{what} must be a tensor of the plan's dtype, contiguous" + (" or with unit inner stride" if rows_may_stride else ""))
        return stride

    def _out_tensor(self, out, shape, device, dtype=None, what: str = "out"):
        """The tensor a call writes: a new one of `shape` on `device` when `out` is None; else `out`, which must be on the plan's device,
        of `dtype` (default: the plan's real one) and contiguous (ValueError), and of `shape` (DimensionMismatchError)."""
        shape = tuple(shape)
        if out is None:
            import torch
            return torch.empty(shape, dtype=dtype or self._tdt, device=device)
        self._on_device(out, what)
        if out.dtype != (dtype or self._tdt) or not out.is_contiguous():
            raise ValueError(f"{what} must be a contiguous tensor of the plan's dtype")
        if tuple(out.shape) != shape:
            raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {shape}, got {tuple(out.shape)}", shape, tuple(out.shape))
        return out

    def _out_array(self, out, shape, dtype=None):
        """The host twin of `_out_tensor`: shape first, as the streaming plans always checked it."""
        shape = tuple(shape)
        if out is None:
            return np.empty(shape, dtype or self._np)
        if tuple(out.shape) != shape:
            raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {shape}, got {tuple(out.shape)}", shape, tuple(out.shape))
        if out.dtype != (dtype or self._np) or not out.flags.c_contiguous:
            raise ValueError("out must be C-contiguous with the plan's dtype")
        return out


_CACHES = weakref.WeakSet()  # every PlanCache alive: what clear_plan_caches() (clear_fft_plan_cache) empties


class PlanCache:
    """Least-recently-used cache of the plans behind the one-shot functions: the most recently used entry last, evicted from the front."""

    def __init__(self, capacity: int = 16):
        self._capacity, self._d = capacity, {}
        _CACHES.add(self)

    def get(self, key, factory):
        """The entry of `key`, built by `factory()` on a miss."""
        if key in self._d:
            value = self._d.pop(key)
        else:
            value = factory()
            while len(self._d) >= self._capacity:
                self._d.pop(next(iter(self._d)))
        self._d[key] = value
        return value

    def clear(self) -> None:
        self._d.clear()

    def __len__(self) -> int:
        return len(self._d)

    def __iter__(self):
        return iter(self._d)


def clear_plan_caches() -> None:
    """Empty every plan cache, whichever family made it."""
    for c in list(_CACHES):
        c.clear()


def current_device_key() -> int:
    """The current-device component of a plan-cache key (-1 without a GPU)."""
    import torch
    return torch.cuda.current_device() if torch.cuda.is_available() else -1
