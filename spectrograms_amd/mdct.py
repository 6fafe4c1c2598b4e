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
        self._cw, cw, clen = _ffi.custom_window(w)
        h = C.c_void_p()
        st = self._lib.sgx_mdct_create(params.window_size, params.hop_size, w.kind, w.param, cw, clen, self._dt, int(device),
                                       C.byref(h))
        self._create(st, h)

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
        xb, squeezed = self._host_rows(x, "samples (n,)")
        nc, nf = self.output_shape(xb.shape[1])
        out = np.empty((xb.shape[0], nc, nf), self._np)
        self._check(self._lib.sgx_mdct_forward(self._h, xb.ctypes.data, xb.shape[0], xb.shape[1], out.ctypes.data, out.size,
                                               _ffi.MEM_HOST, None))
        return out[0] if squeezed else out

    def _rows(self, r: int) -> None:
        n = self.params.n_coefficients
        if r != n:  # src/mdct.rs:451-457
            raise _ffi.InvalidInputError(f"Invalid input: coefficients has {r} rows but params.n_coefficients() = {n}")

    def inverse(self, c, original_length: Optional[int] = None) -> np.ndarray:
        """2-D (N, n_frames) -> 1-D; 3-D (batch, N, n_frames) -> (batch, length)."""
        cb, squeezed = self._host_rows(c, "coefficients (N, n_frames)", (2, 3))
        self._rows(cb.shape[1])
        length = self.inverse_length(cb.shape[2])
        out = np.empty((cb.shape[0], length), self._np)
        if length:
            self._check(self._lib.sgx_mdct_inverse(self._h, cb.ctypes.data, cb.shape[0], cb.shape[1], cb.shape[2], out.ctypes.data,
                                                   out.size, _ffi.MEM_HOST, None))
        if original_length is not None:  # Vec::truncate: a larger value keeps the length
            out = out[:, :int(original_length)]
        return out[0] if squeezed else out

    # ---- device tensors (torch), on the current stream --------------------------------------------------------------------
    def forward_torch(self, x, out=None):
        """(batch, n) device tensor -> (batch, N, n_frames), asynchronous on the current stream."""
        self._check_tensor(x, "samples", 2)
        b, n = x.shape
        out = self._out_tensor(out, (b,) + self.output_shape(n), x.device)
        self._check(self._lib.sgx_mdct_forward(self._h, x.data_ptr(), b, n, out.data_ptr(), out.numel(), _ffi.MEM_DEVICE, self._stream()))
        return out

    def inverse_torch(self, c, out=None):
        """(batch, N, n_frames) device tensor -> (batch, hop n_frames + 2N - hop), asynchronous on the current stream."""
        self._check_tensor(c, "coefficients", 3)
        b, r, nf = c.shape
        self._rows(r)
        out = self._out_tensor(out, (b, self.inverse_length(nf)), c.device)
        if out.numel():
            self._check(self._lib.sgx_mdct_inverse(self._h, c.data_ptr(), b, r, nf, out.data_ptr(), out.numel(), _ffi.MEM_DEVICE,
                                                   self._stream()))
        return out


# ---- one-shot functions with a plan cache (cleared by clear_fft_plan_cache) ---------------------------------------------------
_MDCT_CACHE = _ffi.PlanCache()


def _plan(params: MdctParams, dtype) -> MdctPlan:
    from .functions import _key
    key = (_key(params), parse_dtype(dtype), _ffi.current_device_key())
    return _MDCT_CACHE.get(key, lambda: MdctPlan(params, dtype))


def mdct(samples, params: MdctParams, dtype: Optional[str] = None) -> np.ndarray:
    """mdct (src/mdct.rs:387-440): 1-D samples -> (N, n_frames) in the chosen dtype (default float64)."""
    return _plan(params, dtype).forward(samples)


def imdct(coefficients, params: MdctParams, original_length: Optional[int] = None, dtype: Optional[str] = None) -> np.ndarray:
    """imdct (src/mdct.rs:442-497): (N, n_frames) -> the overlap-added signal, truncated to original_length if that is shorter."""
    return _plan(params, dtype).inverse(coefficients, original_length)


__all__ = ["MdctParams", "MdctPlan", "mdct", "imdct"]
