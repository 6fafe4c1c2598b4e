"""The standalone constant-Q transform: cqt() / CqtResult (src/cqt.rs:517-709) over sgx_plan_create_cqt_transform, batched.

cqt() frames the signal itself: one frame is klen = min(n, 16384) samples, frame f starts at sample f hop (no centring, any hop),
the kernels are CqtKernel::generate(params, sr, klen) and the bins at or above Nyquist are dropped.  `cqt` keeps the reference's
name and argument order and returns the complex coefficients; `CqtTransformPlan` is the plan behind it for callers who keep one
(batched calls, device-resident torch tensors, the kernel it runs).  The CQT *spectrogram* plans of the planner stay what they
are: |Y|^2-derived values on the STFT's framing.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _ffi
from .params import CqtParams, LogParams
from .planner import Plan, signal_length

MAX_KERNEL_LENGTH = 16384  # src/cqt.rs:664
ROWS_MIN_BATCH = 4096  # one-frame calls take the rows route by themselves from this batch on (plan.hip kCqtRowsMinBatch)


class CqtResult:
    """CqtResult (src/cqt.rs:517-613): `data` is complex (n_bins, n_frames), or (batch, n_bins, n_frames) from a batched call."""

    def __init__(self, data: np.ndarray, frequencies: np.ndarray, sample_rate: float, hop_size: int):
        self._data, self._freqs, self.sample_rate, self.hop_size = data, np.asarray(frequencies, np.float64), float(sample_rate), int(hop_size)

    data = property(lambda s: s._data)
    dtype = property(lambda s: "float32" if str(s._data.dtype).endswith("complex64") else "float64")
    frequencies = property(lambda s: s._freqs.tolist())
    n_bins = property(lambda s: s._data.shape[-2])
    n_frames = property(lambda s: s._data.shape[-1])
    shape = property(lambda s: s._data.shape)

    @property
    def time_resolution(self) -> float:
        return self.hop_size / self.sample_rate

    def to_power(self) -> np.ndarray:
        """re re + im im, each product and the sum rounded in T (:606-612)."""
        re, im = self._data.real, self._data.imag
        return re * re + im * im

    def to_magnitude(self) -> np.ndarray:
        """sqrt(re re + im im) in T (:591-597)."""
        p = self.to_power()
        return np.sqrt(p) if isinstance(p, np.ndarray) else p.sqrt()

    def __array__(self, dtype=None, copy=None):
        a = self._data if isinstance(self._data, np.ndarray) else self._data.cpu().numpy()  # (a device tensor comes to the host)
        return a if dtype is None else a.astype(dtype)

    def __dlpack__(self, **kwargs):
        return self._data.__dlpack__(**kwargs)

    def __dlpack_device__(self):
        return self._data.__dlpack_device__()


class CqtTransformPlan(Plan):
    """One sgx_plan of sgx_plan_create_cqt_transform: frames of `kernel_length` (1 .. 16384) samples every `hop_size` samples from
    sample 0.  `amp` is _ffi.AMP_COMPLEX (the coefficients, the default), AMP_POWER, AMP_MAGNITUDE or AMP_DECIBELS (with `db`).
    Everything a Plan offers for the forward path serves it: kernel_name, reserve, output_shape, axes, compute_batch,
    compute_batch_resident, cqt_kernels.  A signal shorter than `kernel_length` gets the STFT's one zero-padded frame, which is not
    cqt() of that signal: that needs a plan of its own length (`cqt` picks it)."""

    def __init__(self, sample_rate: float, kernel_length: int, hop_size: int, cqt_params: CqtParams, amp: int = _ffi.AMP_COMPLEX,
                 db: Optional[LogParams] = None, dtype: Optional[str] = None, device: int = _ffi.DEVICE_CURRENT):
        if not isinstance(cqt_params, CqtParams):
            raise TypeError("cqt_params must be a CqtParams")
        klen, hop = int(kernel_length), int(hop_size)
        if klen <= 0 or hop <= 0:
            raise ValueError("kernel_length and hop_size must be > 0")  # NonZeroUsize
        p = _ffi.SgxParams()
        p.n_fft, p.hop_size, p.centre = klen, min(hop, 0xffffffff), 0
        p.window_kind = _ffi.WIN_RECTANGULAR  # (the STFT window has no part in a CQT)
        p.sample_rate_hz = float(sample_rate)
        p.freq_scale, p.amp_scale = _ffi.FREQ_CQT, amp
        p.has_log_params = int(db is not None)
        p.floor_db = db.floor_db if db is not None else 0.0
        cq = _ffi.SgxCqtParams(cqt_params.bins_per_octave, cqt_params.n_octaves, cqt_params.f_min, cqt_params.q_factor,
                               cqt_params.window.kind, cqt_params.window.param, cqt_params.sparsity_threshold, int(cqt_params.normalize))
        self._open(p, dtype, device, lambda L, pp, h: L.sgx_plan_create_cqt_transform(pp, C.byref(cq), h))
        self._params, self._mel, self._db, self._amp, self._mfcc, self._cw = None, cqt_params, db, amp, None, None
        self._sample_rate, self._hop = float(sample_rate), hop
        self.n_fft = klen

    kernel_length = property(lambda s: s.n_fft)
    hop_size = property(lambda s: s._hop)

    def set_route(self, route: int) -> None:
        """Test entry (sgx_cqt_set_route): 0 = automatic, 1 = per-signal tiles even for one-frame signals, 2 = rows tiles for every
        one-frame call."""
        _ffi.raise_status(self._lib.sgx_cqt_set_route(self._h, int(route)), self._h)

    def compute(self, samples):
        """(n,) or (batch, n) host samples -> CqtResult on a complex plan, the plain array otherwise."""
        a = np.asarray(samples)
        if a.size == 0:
            raise _ffi.InvalidInputError("Invalid input: samples must be non-empty")
        data = self.compute_batch(a[None, :] if a.ndim == 1 else a)
        data = data[0] if a.ndim == 1 else data
        return CqtResult(data, self.axes(1)[0], self._sample_rate, self._hop) if self.is_complex else data

    def compute_frame(self, samples, frame_idx: int):
        raise NotImplementedError("a CQT transform plan computes whole signals")


# ---- one-shot function with a plan cache (cleared by clear_fft_plan_cache) ------------------------------------------------------
_CQT_CACHE = _ffi.PlanCache()


def transform_plan(sample_rate, kernel_length, hop_size, cqt_params, amp, db, dtype, device=_ffi.DEVICE_CURRENT) -> CqtTransformPlan:
    """Cached CqtTransformPlan on `device` (default: the current one), by value."""
    from .functions import _key
    from .params import parse_dtype
    dev = int(device)
    if dev == _ffi.DEVICE_CURRENT:
        dev = _ffi.current_device_key()
    key = (float(sample_rate), int(kernel_length), int(hop_size), _key(cqt_params), amp, _key(db), parse_dtype(dtype), dev)
    return _CQT_CACHE.get(key, lambda: CqtTransformPlan(sample_rate, kernel_length, hop_size, cqt_params, amp, db, dtype, device))


def cqt(samples, sample_rate: float, params: CqtParams, hop_size: int, dtype: Optional[str] = None,
        device: int = _ffi.DEVICE_CURRENT) -> CqtResult:
    """cqt (src/cqt.rs:656-709): (n,) or (batch, n) samples -> CqtResult.  NumPy in, NumPy data out; a torch tensor on the current
    device in, a complex torch tensor in `data` out (nothing comes back to the host).  `device`: the HIP ordinal the plan is bound to
    (default: the current device); a tensor must live there."""
    n = signal_length(samples)
    plan = transform_plan(sample_rate, min(n, MAX_KERNEL_LENGTH), hop_size, params, _ffi.AMP_COMPLEX, None, dtype, device)
    if type(samples).__module__.startswith("torch"):
        data = plan.compute_batch(samples[None] if samples.dim() == 1 else samples)
        return CqtResult(data[0] if samples.dim() == 1 else data, plan.axes(1)[0], float(sample_rate), int(hop_size))
    return plan.compute(samples)


__all__ = ["CqtResult", "CqtTransformPlan", "cqt"]
