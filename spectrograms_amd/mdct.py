"""MDCT / IMDCT (src/mdct.rs; Python surface src/python/mdct.rs) over the sgx_mdct_* C ABI, batched.

`mdct` / `imdct` keep the reference's names and signatures (default dtype float64); `MdctPlan` adds batched calls ((batch, n) signals
in one launch), device-resident torch entry points, and the route the plan runs (`kernel_name`).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _ffi
from .params import WindowType, parse_dtype


class MdctParams:
    """MdctParams(window_size, hop_size, window) — src/mdct.rs:54-140.  window_size = 2N (even, >= 4); N coefficients per frame."""

    __slots__ = ("_window_size", "_hop_size", "_window")

    def __init__(self, window_size: int, hop_size: int, window: WindowType):
        ws, hs = int(window_size), int(hop_size)
        if ws <= 0:  # NonZeroUsize (src/python/mdct.rs:43-50)
            raise ValueError("window_size must be > 0")
        if hs <= 0:
            raise ValueError("hop_size must be > 0")
        _check_window_size(ws)
        if not isinstance(window, WindowType):
            raise TypeError("window must be a WindowType")
        self._window_size, self._hop_size, self._window = ws, hs, window

    @classmethod
    def sine_window(cls, window_size: int) -> "MdctParams":
        """Sine window w[k] = sin(pi (k + 1/2) / window_size) and hop window_size / 2 (the TDAC pair)."""
        ws = int(window_size)
        if ws <= 0:
            raise ValueError("window_size must be > 0")
        _check_window_size(ws)
        w = np.sin(np.pi * (np.arange(ws, dtype=np.float64) + 0.5) / ws)
        return cls(ws, ws // 2, WindowType.custom(w))

    @property
    def window_size(self) -> int:
        return self._window_size

    @property
    def hop_size(self) -> int:
        return self._hop_size

    @property
    def window(self) -> WindowType:
        return self._window

    @property
    def n_coefficients(self) -> int:
        return self._window_size // 2

    def __repr__(self) -> str:
        return (f"MdctParams(window_size={self._window_size}, hop_size={self._hop_size}, "
                f"n_coefficients={self.n_coefficients})")


def _check_window_size(ws: int) -> None:
    if ws % 2 != 0:
        raise _ffi.InvalidInputError(f"Invalid input: window_size must be even, got {ws}")
    if ws < 4:
        raise _ffi.InvalidInputError(f"Invalid input: window_size must be >= 4, got {ws}")


class MdctPlan(_ffi.NativeHandle):
    """One sgx_mdct (params + dtype + device).  Not thread-safe, like the reference's `&mut self` plans."""

    _prefix = "sgx_mdct"

    def __init__(self, params: MdctParams, dtype: Optional[str] = None, device: int = _ffi.DEVICE_CURRENT):
        self._lib = _ffi.lib()
        self.params = params
        self._dt = parse_dtype(dtype)
        w = params.window
        cw, clen = None, 0
        if w.kind == _ffi.WIN_CUSTOM:
            self._cw = np.ascontiguousarray(w.coefficients, dtype=np.float64)
            cw, clen = self._cw.ctypes.data_as(C.POINTER(C.c_double)), self._cw.size
        h = C.c_void_p()
        st = self._lib.sgx_mdct_create(params.window_size, params.hop_size, w.kind, w.param, cw, clen, self._dt, int(device),
                                       C.byref(h))
        self._create(st, h)
        self._device = int(self._lib.sgx_mdct_device(h))

    @property
    def device(self) -> int:
        return self._device

    @property
    def n_coefficients(self) -> int:
        return self.params.n_coefficients

    def output_shape(self, n_samples: int):
        """(N, n_frames) for a signal of n_samples samples."""
        nc, nf = C.c_size_t(), C.c_size_t()
        self._check(self._lib.sgx_mdct_output_shape(self._h, int(n_samples), C.byref(nc), C.byref(nf)))
        return nc.value, nf.value

    def inverse_length(self, n_frames: int) -> int:
        n = C.c_size_t()
        self._check(self._lib.sgx_mdct_inverse_length(self._h, int(n_frames), C.byref(n)))
        return n.value

    def kernel_name(self, inverse: bool = False) -> str:
        return self._lib.sgx_mdct_kernel_name(self._h, int(bool(inverse))).decode()

    def window(self) -> np.ndarray:
        out = np.empty(self.params.window_size, np.float64)
        self._check(self._lib.sgx_mdct_window(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def reserve(self, batch: int, n_samples: int, host_staging: bool = True) -> None:
        """Pre-size the plan-owned scratch so that calls of up to `batch` signals of `n_samples` samples do not allocate."""
        self._check(self._lib.sgx_mdct_reserve(self._h, int(batch), int(n_samples), int(host_staging)))

    # ---- host arrays ------------------------------------------------------------------------------------------------------
    def forward(self, x) -> np.ndarray:
        """1-D (n,) -> (N, n_frames); 2-D (batch, n) -> (batch, N, n_frames)."""
        a = np.ascontiguousarray(x, dtype=self._np)
        if a.ndim not in (1, 2):
            raise ValueError("samples must be 1-D (n,) or 2-D (batch, n)")
        xb = a[None] if a.ndim == 1 else a
        if xb.shape[0] == 0:
            raise ValueError("batch must be > 0")
        nc, nf = self.output_shape(xb.shape[1])
        out = np.empty((xb.shape[0], nc, nf), self._np)
        self._check(self._lib.sgx_mdct_forward(self._h, xb.ctypes.data, xb.shape[0], xb.shape[1], out.ctypes.data, out.size,
                                               _ffi.MEM_HOST, None))
        return out[0] if a.ndim == 1 else out

    def _rows(self, r: int) -> None:
        n = self.params.n_coefficients
        if r != n:  # src/mdct.rs:451-457
            raise _ffi.InvalidInputError(f"Invalid input: coefficients has {r} rows but params.n_coefficients() = {n}")

    def inverse(self, c, original_length: Optional[int] = None) -> np.ndarray:
        """2-D (N, n_frames) -> 1-D; 3-D (batch, N, n_frames) -> (batch, length)."""
        a = np.ascontiguousarray(c, dtype=self._np)
        if a.ndim not in (2, 3):
            raise ValueError("coefficients must be 2-D (N, n_frames) or 3-D (batch, N, n_frames)")
        cb = a[None] if a.ndim == 2 else a
        if cb.shape[0] == 0:
            raise ValueError("batch must be > 0")
        self._rows(cb.shape[1])
        length = self.inverse_length(cb.shape[2])
        out = np.empty((cb.shape[0], length), self._np)
        if length:
            self._check(self._lib.sgx_mdct_inverse(self._h, cb.ctypes.data, cb.shape[0], cb.shape[1], cb.shape[2], out.ctypes.data,
                                                   out.size, _ffi.MEM_HOST, None))
        if original_length is not None:  # Vec::truncate: a larger value keeps the length
            out = out[:, :int(original_length)]
        return out[0] if a.ndim == 2 else out

    # ---- device tensors (torch), on the current stream --------------------------------------------------------------------
    def _tensor(self, t, what: str, ndim: int):
        import torch
        tdt = self._tdt
        if not t.is_cuda or t.device.index != self._device:
            raise ValueError(f"{what} is on {t.device}, the plan is bound to cuda:{self._device}")
        if t.dtype != tdt or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous tensor of the plan's dtype")
        if t.dim() != ndim or t.shape[0] == 0:
            raise ValueError(f"{what} must be {ndim}-D with batch > 0, got shape {tuple(t.shape)}")
        return tdt

    def forward_torch(self, x, out=None):
        """(batch, n) device tensor -> (batch, N, n_frames), asynchronous on the current stream."""
        import torch
        tdt = self._tensor(x, "samples", 2)
        b, n = x.shape
        nc, nf = self.output_shape(n)
        if out is None:
            out = torch.empty((b, nc, nf), dtype=tdt, device=x.device)
        else:
            self._tensor(out, "out", 3)
            if tuple(out.shape) != (b, nc, nf):
                raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {(b, nc, nf)}, got {tuple(out.shape)}")
        s = torch.cuda.current_stream(x.device).cuda_stream
        self._check(self._lib.sgx_mdct_forward(self._h, x.data_ptr(), b, n, out.data_ptr(), out.numel(), _ffi.MEM_DEVICE,
                                               C.c_void_p(s)))
        return out

    def inverse_torch(self, c, out=None):
        """(batch, N, n_frames) device tensor -> (batch, hop n_frames + 2N - hop), asynchronous on the current stream."""
        import torch
        tdt = self._tensor(c, "coefficients", 3)
        b, r, nf = c.shape
        self._rows(r)
        length = self.inverse_length(nf)
        if out is None:
            out = torch.empty((b, length), dtype=tdt, device=c.device)
        else:
            self._tensor(out, "out", 2)
            if tuple(out.shape) != (b, length):
                raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {(b, length)}, got {tuple(out.shape)}")
        if length:
            s = torch.cuda.current_stream(c.device).cuda_stream
            self._check(self._lib.sgx_mdct_inverse(self._h, c.data_ptr(), b, r, nf, out.data_ptr(), out.numel(), _ffi.MEM_DEVICE,
                                                   C.c_void_p(s)))
        return out


# ---- one-shot functions with a plan cache (cleared by clear_fft_plan_cache) ---------------------------------------------------
_MDCT_CACHE = {}
_MDCT_CACHE_MAX = 16


def _plan(params: MdctParams, dtype) -> MdctPlan:
    from .functions import _key
    import torch
    dev = torch.cuda.current_device() if torch.cuda.is_available() else -1
    key = (_key(params), parse_dtype(dtype), dev)
    plan = _MDCT_CACHE.pop(key, None)
    if plan is None:
        plan = MdctPlan(params, dtype)
        while len(_MDCT_CACHE) >= _MDCT_CACHE_MAX:
            _MDCT_CACHE.pop(next(iter(_MDCT_CACHE)))
    _MDCT_CACHE[key] = plan  # most recently used last
    return plan


def clear_mdct_plan_cache() -> None:
    _MDCT_CACHE.clear()


def mdct(samples, params: MdctParams, dtype: Optional[str] = None) -> np.ndarray:
    """mdct (src/mdct.rs:387-440): 1-D samples -> (N, n_frames) in the chosen dtype (default float64)."""
    return _plan(params, dtype).forward(samples)


def imdct(coefficients, params: MdctParams, original_length: Optional[int] = None, dtype: Optional[str] = None) -> np.ndarray:
    """imdct (src/mdct.rs:442-497): (N, n_frames) -> the overlap-added signal, truncated to original_length if that is shorter."""
    return _plan(params, dtype).inverse(coefficients, original_length)


__all__ = ["MdctParams", "MdctPlan", "mdct", "imdct"]
