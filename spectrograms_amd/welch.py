"""Welch spectrum estimates over the sgx_welch_* C ABI, batched: the averaged periodogram (`welch`), the cross-spectral density of two
signals (`csd`) and their magnitude-squared coherence (`coherence`).

The semantics are those of `scipy.signal.welch` / `csd` / `coherence` for real input with `nperseg = nfft = n_fft`,
`noverlap = n_fft - hop_size` and `average="mean"`: segments start at `s * hop_size`, nothing is padded, a tail that fills no segment is
ignored; each segment is detrended, then windowed, then transformed; the result is one-sided.  The conjugate of the cross spectrum is on
the first argument, as scipy's.  `WindowType.hanning` is the symmetric Hann window; scipy's string `"hann"` is the periodic one — hand
scipy `plan.window()` to compare.

Out of scope: `average="median"`; zero padding to `nfft > nperseg`; two-sided spectra and complex input; sums carried across calls
(streaming accumulation).  Signals shorter than `n_fft` are refused with `DimensionMismatchError` (scipy shrinks the segment instead).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _ffi
from .params import WindowType, parse_dtype

_KINDS = {"psd": _ffi.WELCH_PSD, "csd": _ffi.WELCH_CSD, "coherence": _ffi.WELCH_COHERENCE}
_DETRENDS = {None: _ffi.WELCH_DETREND_NONE, False: _ffi.WELCH_DETREND_NONE, "none": _ffi.WELCH_DETREND_NONE,
             "constant": _ffi.WELCH_DETREND_CONSTANT, "linear": _ffi.WELCH_DETREND_LINEAR}
_SCALINGS = {"density": _ffi.WELCH_DENSITY, "spectrum": _ffi.WELCH_SPECTRUM}
_ROUTES = {"auto": _ffi.WELCH_ROUTE_AUTO, "generic": _ffi.WELCH_ROUTE_GENERIC}


class WelchParams:
    """WelchParams(n_fft, hop_size, window=WindowType.hanning, sample_rate=1.0, detrend="constant", scaling="density").

    `detrend` is None, "constant" (subtract each segment's mean) or "linear" (subtract its least-squares line); `scaling` is "density"
    (1 / (sample_rate * sum w^2): a power spectral density) or "spectrum" (1 / (sum w)^2: a power spectrum)."""

    __slots__ = ("n_fft", "hop_size", "window", "sample_rate", "detrend", "scaling")

    def __init__(self, n_fft: int, hop_size: int, window=WindowType.hanning, sample_rate: float = 1.0, detrend: Optional[str] = "constant",
                 scaling: str = "density"):
        if int(n_fft) != n_fft or int(n_fft) < 1 or int(n_fft) >= 2 ** 32:
            raise _ffi.InvalidInputError(f"Invalid input: n_fft must be a positive integer, got {n_fft!r}")
        if int(hop_size) != hop_size or not 1 <= int(hop_size) <= int(n_fft):
            raise _ffi.InvalidInputError(f"Invalid input: hop_size must be in 1 .. n_fft = {int(n_fft)}, got {hop_size!r}")
        if isinstance(detrend, (list, dict, set, np.ndarray)) or detrend not in _DETRENDS:
            raise _ffi.InvalidInputError(f"Invalid input: detrend must be None, 'constant' or 'linear', got {detrend!r}")
        if not isinstance(scaling, str) or scaling not in _SCALINGS:
            raise _ffi.InvalidInputError(f"Invalid input: scaling must be 'density' or 'spectrum', got {scaling!r}")
        if not float(sample_rate) > 0.0 or not np.isfinite(float(sample_rate)):
            raise _ffi.InvalidInputError(f"Invalid input: sample_rate must be finite and > 0, got {sample_rate!r}")
        self.n_fft, self.hop_size, self.window = int(n_fft), int(hop_size), window
        self.sample_rate, self.detrend, self.scaling = float(sample_rate), detrend, scaling

    def __repr__(self) -> str:
        return (f"WelchParams(n_fft={self.n_fft}, hop_size={self.hop_size}, sample_rate={self.sample_rate}, detrend={self.detrend!r}, "
                f"scaling={self.scaling!r})")


class WelchPlan(_ffi.NativeHandle):
    """One sgx_welch (params + kind + dtype + device + route).  Not thread-safe, like every plan here.

    kind "psd": `compute(x)` -> Pxx; "csd": `compute(x, y)` -> complex Pxy (the conjugate on x); "coherence": `compute(x, y)` ->
    |Pxy|^2 / (Pxx Pyy).  route "auto" runs the fused kernel (`kernel_name == "k_welch"`) for n_fft a power of two 256 .. 4096 and the
    generic route otherwise; `max_scratch_bytes` caps each scratch buffer of the generic route (default 256 MiB).  A row's result
    does not depend on the batch it is in."""

    _prefix = "sgx_welch"

    def __init__(self, params: WelchParams, kind: str = "psd", dtype: Optional[str] = "float64", device: Optional[int] = None,
                 route: str = "auto", max_scratch_bytes: Optional[int] = None):
        if not isinstance(params, WelchParams):
            raise TypeError("params must be a WelchParams")
        if not isinstance(kind, str) or kind not in _KINDS:
            raise _ffi.InvalidInputError(f"Invalid input: kind must be 'psd', 'csd' or 'coherence', got {kind!r}")
        if not isinstance(route, str) or route not in _ROUTES:
            raise _ffi.InvalidInputError(f"Invalid input: route must be 'auto' or 'generic', got {route!r}")
        if max_scratch_bytes is not None and int(max_scratch_bytes) < 1:
            raise _ffi.InvalidInputError(f"Invalid input: max_scratch_bytes must be > 0, got {max_scratch_bytes!r}")
        self._lib = _ffi.lib()
        self.params, self.kind = params, kind
        self._dt = parse_dtype(dtype)
        p = _ffi.SgxParams()
        p.n_fft, p.hop_size, p.centre = params.n_fft, params.hop_size, 0
        p.window_kind, p.window_param = params.window.kind, params.window.param
        self._cw = None
        if params.window.kind == _ffi.WIN_CUSTOM:
            self._cw = np.ascontiguousarray(params.window.coefficients, np.float64)
            p.custom_window = self._cw.ctypes.data_as(C.POINTER(C.c_double))
            p.custom_window_len = self._cw.size
        p.sample_rate_hz = params.sample_rate
        p.freq_scale, p.amp_scale = _ffi.FREQ_LINEAR, _ffi.AMP_COMPLEX
        p.dtype, p.device = self._dt, _ffi.DEVICE_CURRENT if device is None else int(device)
        h = C.c_void_p()
        st = self._lib.sgx_welch_create(C.byref(p), _KINDS[kind], _DETRENDS[params.detrend], _SCALINGS[params.scaling], _ROUTES[route],
                                        0 if max_scratch_bytes is None else int(max_scratch_bytes), C.byref(h))
        self._create(st, h)
        self._device = int(self._lib.sgx_welch_device(h))
        self.n_bins = int(self._lib.sgx_welch_n_bins(h))

    device = property(lambda self: self._device)
    dtype = property(lambda self: "float32" if self._dt == _ffi.F32 else "float64")
    kernel_name = property(lambda self: self._lib.sgx_welch_kernel_name(self._h).decode(), doc='"k_welch" or "welch_generic"')
    tile = property(lambda self: int(self._lib.sgx_welch_tile(self._h)), doc="segments per workgroup tile of k_welch; 0 on the generic route")
    scale = property(lambda self: float(self._lib.sgx_welch_scale(self._h)), doc="1 / (sample_rate sum w^2) or 1 / (sum w)^2, in f64")
    allocations = property(lambda self: int(self._lib.sgx_welch_allocations(self._h)),
                           doc="how often the plan has allocated or replaced one of its own buffers (it stands still within what reserve() sized)")

    def frequencies(self) -> np.ndarray:
        """(n_bins,) f64: k * sample_rate / n_fft."""
        f = np.empty(self.n_bins, np.float64)
        self._check(self._lib.sgx_welch_frequencies(self._h, f.ctypes.data_as(C.POINTER(C.c_double))))
        return f

    def window(self) -> np.ndarray:
        """(n_fft,) f64: the window as built, before the cast to the plan's dtype."""
        w = np.empty(self.params.n_fft, np.float64)
        self._check(self._lib.sgx_welch_window(self._h, w.ctypes.data_as(C.POINTER(C.c_double))))
        return w

    def n_segments(self, n_samples: int) -> int:
        """m = 1 + (n_samples - n_fft) // hop_size; 0 for signals shorter than n_fft."""
        return int(self._lib.sgx_welch_n_segments(self._h, int(n_samples)))

    def reserve(self, batch: int, n_samples: int, host_staging: bool = True) -> None:
        """Pre-size the plan-owned scratch so that calls of up to `batch` rows of `n_samples` samples do not allocate."""
        self._check(self._lib.sgx_welch_reserve(self._h, int(batch), int(n_samples), int(host_staging)))

    def _pair_check(self, y):
        if self.kind == "psd" and y is not None:
            raise _ffi.InvalidInputError("Invalid input: y must be None for a 'psd' plan")
        if self.kind != "psd" and y is None:
            raise _ffi.InvalidInputError(f"Invalid input: y is required by a {self.kind!r} plan")

    # ---- host arrays ------------------------------------------------------------------------------------------------------
    def compute(self, x, y=None) -> np.ndarray:
        """(n,) or (batch, n) -> (n_bins,) or (batch, n_bins); complex for kind "csd"."""
        self._pair_check(y)
        a = np.ascontiguousarray(x, dtype=self._np)
        if a.ndim not in (1, 2):
            raise ValueError("x must be 1-D (n,) or 2-D (batch, n)")
        xb = a[None] if a.ndim == 1 else a
        if xb.shape[0] == 0:
            raise ValueError("batch must be > 0")
        yb = None
        if y is not None:
            yb = np.ascontiguousarray(y, dtype=self._np)
            if yb.shape != a.shape:
                raise _ffi.DimensionMismatchError(f"Dimension mismatch: x has shape {a.shape}, y {yb.shape}", expected=a.size, got=yb.size)
        b, n = xb.shape
        cplx = self.kind == "csd"
        out = np.empty((b, self.n_bins * (2 if cplx else 1)), self._np)
        self._check(self._lib.sgx_welch_execute(self._h, xb.ctypes.data, None if yb is None else yb.ctypes.data, b, n, n, out.ctypes.data,
                                                out.size, _ffi.MEM_HOST, None))
        if cplx:
            out = out.view(np.complex64 if self._dt == _ffi.F32 else np.complex128)
        return out[0] if a.ndim == 1 else out

    # ---- device tensors (torch), on the current stream --------------------------------------------------------------------
    def _rows(self, t, what):
        """-> the row stride in elements.  Rows may be a slice `X[:, a:b]` of a resident tensor (unit inner stride)."""
        if not t.is_cuda or t.device.index != self._device:
            raise ValueError(f"{what} is on {t.device}, the plan is bound to cuda:{self._device}")
        if t.dim() != 2 or t.shape[0] == 0:
            raise ValueError(f"{what} must be 2-D with batch > 0, got shape {tuple(t.shape)}")
        b, n = t.shape
        stride = t.stride(0) if b > 1 else max(n, 1)
        if t.dtype != self._tdt or not (t.is_contiguous() or ((n <= 1 or t.stride(1) == 1) and stride >= n)):
            raise ValueError(f"{what} must be a tensor of the plan's dtype, contiguous or with unit inner stride")
        return stride

    def compute_torch(self, x, y=None, out=None):
        """(batch, n) device tensors -> (batch, n_bins) (complex for kind "csd"), asynchronous on the current stream."""
        import torch
        self._pair_check(y)
        stride = self._rows(x, "x")
        b, n = x.shape
        if y is not None:
            if tuple(y.shape) != tuple(x.shape):
                raise _ffi.DimensionMismatchError(f"Dimension mismatch: x has shape {tuple(x.shape)}, y {tuple(y.shape)}")
            if self._rows(y, "y") != stride:
                raise ValueError("x and y must have the same row stride")
        cplx = self.kind == "csd"
        odt = self._tdt if not cplx else (torch.complex64 if self._dt == _ffi.F32 else torch.complex128)
        if out is None:
            out = torch.empty((b, self.n_bins), dtype=odt, device=x.device)
        else:
            if not out.is_cuda or out.device != x.device or out.dtype != odt or not out.is_contiguous():
                raise ValueError("out must be a contiguous tensor of the result's dtype on the plan's device")
            if tuple(out.shape) != (b, self.n_bins):
                raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {(b, self.n_bins)}, got {tuple(out.shape)}")
        s = torch.cuda.current_stream(x.device).cuda_stream
        self._check(self._lib.sgx_welch_execute(self._h, x.data_ptr(), None if y is None else y.data_ptr(), b, n, stride, out.data_ptr(),
                                                out.numel() * (2 if cplx else 1), _ffi.MEM_DEVICE, C.c_void_p(s)))
        return out


# ---- one-shot functions with a plan cache (cleared by clear_fft_plan_cache) ---------------------------------------------------
_WELCH_CACHE = {}
_WELCH_CACHE_MAX = 16


def _plan(params, kind, dtype) -> WelchPlan:
    from .functions import _key
    import torch
    if not isinstance(params, WelchParams):
        raise TypeError("params must be a WelchParams")
    dev = torch.cuda.current_device() if torch.cuda.is_available() else -1
    key = (_key(params), kind, parse_dtype(dtype), dev)
    plan = _WELCH_CACHE.pop(key, None)
    if plan is None:
        plan = WelchPlan(params, kind, dtype)
        while len(_WELCH_CACHE) >= _WELCH_CACHE_MAX:
            _WELCH_CACHE.pop(next(iter(_WELCH_CACHE)))
    _WELCH_CACHE[key] = plan  # most recently used last
    return plan


def clear_welch_plan_cache() -> None:
    _WELCH_CACHE.clear()


def welch(x, params: WelchParams, dtype: str = "float64"):
    """scipy.signal.welch on (n,) or (batch, n) rows -> (frequencies, Pxx)."""
    plan = _plan(params, "psd", dtype)
    return plan.frequencies(), plan.compute(x)


def csd(x, y, params: WelchParams, dtype: str = "float64"):
    """scipy.signal.csd -> (frequencies, Pxy), Pxy complex with the conjugate on x."""
    plan = _plan(params, "csd", dtype)
    return plan.frequencies(), plan.compute(x, y)


def coherence(x, y, params: WelchParams, dtype: str = "float64"):
    """scipy.signal.coherence -> (frequencies, Cxy), Cxy = |Pxy|^2 / (Pxx Pyy)."""
    plan = _plan(params, "coherence", dtype)
    return plan.frequencies(), plan.compute(x, y)


__all__ = ["WelchParams", "WelchPlan", "welch", "csd", "coherence"]
