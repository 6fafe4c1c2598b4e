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
        self._cw, p.custom_window, p.custom_window_len = _ffi.custom_window(params.window)
        p.sample_rate_hz = params.sample_rate
        p.freq_scale, p.amp_scale = _ffi.FREQ_LINEAR, _ffi.AMP_COMPLEX
        p.dtype, p.device = self._dt, _ffi.DEVICE_CURRENT if device is None else int(device)
        h = C.c_void_p()
        st = self._lib.sgx_welch_create(C.byref(p), _KINDS[kind], _DETRENDS[params.detrend], _SCALINGS[params.scaling], _ROUTES[route],
                                        0 if max_scratch_bytes is None else int(max_scratch_bytes), C.byref(h))
        self._create(st, h)
        self.n_bins = int(self._lib.sgx_welch_n_bins(h))

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
        xb, squeezed = self._host_rows(x, "x (n,)")
        yb = None
        if y is not None:
            if np.shape(y) != np.shape(x):
                raise _ffi.DimensionMismatchError(f"Dimension mismatch: x has shape {np.shape(x)}, y {np.shape(y)}",
                                                  expected=xb.size, got=int(np.prod(np.shape(y))))
            yb, _ = self._host_rows(y, "y (n,)")
        b, n = xb.shape
        cplx = self.kind == "csd"
        out = np.empty((b, self.n_bins * (2 if cplx else 1)), self._np)
        self._check(self._lib.sgx_welch_execute(self._h, xb.ctypes.data, None if yb is None else yb.ctypes.data, b, n, n, out.ctypes.data,
                                                out.size, _ffi.MEM_HOST, None))
        if cplx:
            out = out.view(self._cdt)
        return out[0] if squeezed else out

    # ---- device tensors (torch), on the current stream --------------------------------------------------------------------
    def compute_torch(self, x, y=None, out=None):
        """(batch, n) device tensors -> (batch, n_bins) (complex for kind "csd"), asynchronous on the current stream.  Rows may be a
        slice `X[:, a:b]` of a resident tensor (unit inner stride)."""
        self._pair_check(y)
        stride = self._check_tensor(x, "x", 2, rows_may_stride=True)
        b, n = x.shape
        if y is not None:
            if tuple(y.shape) != tuple(x.shape):
                raise _ffi.DimensionMismatchError(f"Dimension mismatch: x has shape {tuple(x.shape)}, y {tuple(y.shape)}")
            if self._check_tensor(y, "y", 2, rows_may_stride=True) != stride:
                raise ValueError("x and y must have the same row stride")
        cplx = self.kind == "csd"
        out = self._out_tensor(out, (b, self.n_bins), x.device, self._tcdt if cplx else None)
        self._check(self._lib.sgx_welch_execute(self._h, x.data_ptr(), None if y is None else y.data_ptr(), b, n, stride, out.data_ptr(),
                                                out.numel() * (2 if cplx else 1), _ffi.MEM_DEVICE, self._stream()))
        return out


# ---- one-shot functions with a plan cache (cleared by clear_fft_plan_cache) ---------------------------------------------------
_WELCH_CACHE = _ffi.PlanCache()


def _plan(params, kind, dtype) -> WelchPlan:
    from .functions import _key
    if not isinstance(params, WelchParams):
        raise TypeError("params must be a WelchParams")
    key = (_key(params), kind, parse_dtype(dtype), _ffi.current_device_key())
    return _WELCH_CACHE.get(key, lambda: WelchPlan(params, kind, dtype))


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
