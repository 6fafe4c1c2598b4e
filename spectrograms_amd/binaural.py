"""Binaural ITD / IPD / ILD / ILR spectrograms (src/binaural.rs; Python surface python/spectrograms/__init__.pyi:466-2125) over the
sgx_binaural_* C ABI, batched over stereo pairs.

The one-shot `compute_*_spectrogram` functions keep the reference's names, defaults and signatures (default dtype float64) and return
result objects with the reference's accessors; `BinauralPlan` adds batched calls ((B, n) left and right rows in one call), device-resident
torch entry points and the route the plan runs (`kernel_name`).  Histograms run on the device (k_binaural_hist); the two `*_diff`
reductions are NumPy over the maps.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from . import _ffi
from .params import SpectrogramParams, parse_dtype


def _stft_struct(sp: SpectrogramParams, dtype: int, device: int):
    """sgx_params with the STFT fields of `sp` (the only ones sgx_binaural_create reads); returns (struct, custom window keep-alive)."""
    st = sp.stft
    p = _ffi.SgxParams()
    p.n_fft, p.hop_size, p.centre = st.n_fft, st.hop_size, int(st.centre)
    p.window_kind, p.window_param = st.window.kind, st.window.param
    cw, p.custom_window, p.custom_window_len = _ffi.custom_window(st.window)
    p.sample_rate_hz = sp.sample_rate
    p.freq_scale, p.amp_scale = _ffi.FREQ_LINEAR, _ffi.AMP_COMPLEX
    p.dtype, p.device = dtype, device
    return p, cw


class _BinauralParams:
    __slots__ = ("_sp", "_start", "_end")
    _KIND = -1

    def __init__(self, spectrogram_params: SpectrogramParams, start_freq: float, end_freq: float):
        if not isinstance(spectrogram_params, SpectrogramParams):
            raise TypeError("spectrogram_params must be a SpectrogramParams")
        self._sp, self._start, self._end = spectrogram_params, float(start_freq), float(end_freq)
        BinauralPlan(self, "float64", _ffi.DEVICE_HOST_ONLY)  # validation (texts of ITDSpectrogramParams::new and its siblings)

    def _c(self):
        return _ffi.SgxBinauralParams(self._KIND, self._start, self._end, 1, 0)

    @property
    def spectrogram_params(self) -> SpectrogramParams:
        return self._sp

    @property
    def start_freq(self) -> float:
        return self._start

    @property
    def end_freq(self) -> float:
        return self._end

    def __repr__(self) -> str:
        return f"{type(self).__name__}(start_freq={self._start}, end_freq={self._end})"


class ITDSpectrogramParams(_BinauralParams):
    """ITDSpectrogramParams(spectrogram_params, start_freq=50, end_freq=620, magphase_power=1) — src/binaural.rs:410-460."""

    __slots__ = ("_power",)
    _KIND = _ffi.BINAURAL_ITD

    def __init__(self, spectrogram_params: SpectrogramParams, start_freq: Optional[float] = 50.0, end_freq: Optional[float] = 620.0,
                 magphase_power: int = 1):
        p = int(magphase_power)
        if p < 0:
            raise ValueError("magphase_power must be >= 0")
        self._power = p if p > 0 else 1  # the binding maps 0 to 1 (NonZeroUsize)
        super().__init__(spectrogram_params, 50.0 if start_freq is None else start_freq, 620.0 if end_freq is None else end_freq)

    def _c(self):
        return _ffi.SgxBinauralParams(self._KIND, self._start, self._end, self._power, 0)

    @property
    def magphase_power(self) -> int:
        return self._power


class IPDSpectrogramParams(_BinauralParams):
    """IPDSpectrogramParams(spectrogram_params, start_freq=50, end_freq=620, wrapped=False) — src/binaural.rs (IPD)."""

    __slots__ = ("_wrapped",)
    _KIND = _ffi.BINAURAL_IPD

    def __init__(self, spectrogram_params: SpectrogramParams, start_freq: Optional[float] = 50.0, end_freq: Optional[float] = 620.0,
                 wrapped: bool = False):
        self._wrapped = bool(wrapped)
        super().__init__(spectrogram_params, 50.0 if start_freq is None else start_freq, 620.0 if end_freq is None else end_freq)

    def _c(self):
        return _ffi.SgxBinauralParams(self._KIND, self._start, self._end, 1, int(self._wrapped))

    @property
    def wrapped(self) -> bool:
        return self._wrapped


class ILDSpectrogramParams(_BinauralParams):
    """ILDSpectrogramParams(spectrogram_params, start_freq=1700, end_freq=4600) — src/binaural.rs (ILD)."""

    __slots__ = ()
    _KIND = _ffi.BINAURAL_ILD

    def __init__(self, spectrogram_params: SpectrogramParams, start_freq: Optional[float] = 1700.0, end_freq: Optional[float] = 4600.0):
        super().__init__(spectrogram_params, 1700.0 if start_freq is None else start_freq, 4600.0 if end_freq is None else end_freq)


class ILRSpectrogramParams(_BinauralParams):
    """ILRSpectrogramParams(spectrogram_params, start_freq=1700, end_freq=4600) — src/binaural.rs (ILR)."""

    __slots__ = ()
    _KIND = _ffi.BINAURAL_ILR

    def __init__(self, spectrogram_params: SpectrogramParams, start_freq: Optional[float] = 1700.0, end_freq: Optional[float] = 4600.0):
        super().__init__(spectrogram_params, 1700.0 if start_freq is None else start_freq, 4600.0 if end_freq is None else end_freq)


class BinauralPlan(_ffi.NativeHandle):
    """One sgx_binaural (params + dtype + device).  Not thread-safe, like the reference's `&mut self` plans."""

    _prefix = "sgx_binaural"

    def __init__(self, params: _BinauralParams, dtype: Optional[str] = None, device: int = _ffi.DEVICE_CURRENT):
        self._lib = _ffi.lib()
        self.params = params
        self._dt = parse_dtype(dtype)
        sp, self._cw = _stft_struct(params.spectrogram_params, self._dt, int(device))
        bp = params._c()
        h = C.c_void_p()
        st = self._lib.sgx_binaural_create(C.byref(sp), C.byref(bp), C.byref(h))
        self._create(st, h)

    @property
    def kernel_name(self) -> str:
        return self._lib.sgx_binaural_kernel_name(self._h).decode()

    def output_shape(self, n_samples: int):
        """(start_bin, n_bins, n_frames) for signals of n_samples samples."""
        sb, nb, nf = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self._lib.sgx_binaural_output_shape(self._h, int(n_samples), C.byref(sb), C.byref(nb), C.byref(nf)))
        return sb.value, nb.value, nf.value

    def axes(self, n_frames: int):
        """(frequencies [n_bins], times [n_frames]) in Hz and seconds."""
        _, nb, _ = self.output_shape(self.params.spectrogram_params.stft.n_fft)
        f, t = np.empty(nb, np.float64), np.empty(int(n_frames), np.float64)
        dp = C.POINTER(C.c_double)
        self._check(self._lib.sgx_binaural_axes(self._h, int(n_frames), f.ctypes.data_as(dp), t.ctypes.data_as(dp)))
        return f, t

    def reserve(self, batch: int, n_samples: int, host_staging: bool = True) -> None:
        """Pre-size the plan-owned scratch so that calls of up to `batch` pairs of `n_samples` samples do not allocate."""
        self._check(self._lib.sgx_binaural_reserve(self._h, int(batch), int(n_samples), int(host_staging)))

    # ---- host arrays ------------------------------------------------------------------------------------------------------
    def compute(self, left, right) -> np.ndarray:
        """1-D (n,) pair -> (n_bins, n_frames); 2-D (B, n) rows -> (B, n_bins, n_frames)."""
        shape, rshape = np.shape(left), np.shape(right)
        if len(shape) in (1, 2) and shape != rshape:
            raise _ffi.DimensionMismatchError(f"Dimension mismatch: left has shape {shape}, right {rshape}",
                                              expected=math.prod(shape), got=math.prod(rshape))
        if len(shape) in (1, 2) and 0 in shape:
            raise _ffi.InvalidInputError("Invalid input: samples must be non-empty")
        lb, squeezed = self._host_rows(left, "left / right (n,)")
        rb, _ = self._host_rows(right, "left / right (n,)")
        _, nb, nf = self.output_shape(lb.shape[1])
        out = np.empty((lb.shape[0], nb, nf), self._np)
        self._check(self._lib.sgx_binaural_execute(self._h, lb.ctypes.data, rb.ctypes.data, lb.shape[0], lb.shape[1], lb.shape[1],
                                                   out.ctypes.data, out.size, _ffi.MEM_HOST, None))
        return out[0] if squeezed else out

    def histogram(self, values, num_bins: int, lo: float, hi: float, exponent: int = 1, normalize: bool = False) -> np.ndarray:
        """Per-frame histograms of maps (n_bins, n_frames) or (B, n_bins, n_frames) -> (num_bins, n_frames) / (B, num_bins, n_frames) f64."""
        vb, squeezed = self._host_rows(values, "values (n_bins, n_frames)", (2, 3))
        _, nb, _ = self.output_shape(self.params.spectrogram_params.stft.n_fft)
        if vb.shape[1] != nb:
            raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {nb} rows, got {vb.shape[1]}", expected=nb, got=vb.shape[1])
        out = np.empty((vb.shape[0], int(num_bins), vb.shape[2]), np.float64)
        self._check(self._lib.sgx_binaural_histogram(self._h, vb.ctypes.data, vb.shape[0], vb.shape[2], int(num_bins), float(lo), float(hi),
                                                     int(exponent), int(bool(normalize)), out.ctypes.data, out.size, _ffi.MEM_HOST, None))
        return out[0] if squeezed else out

    # ---- device tensors (torch), on the current stream --------------------------------------------------------------------
    def compute_torch(self, left, right, out=None):
        """(B, n) device tensors -> (B, n_bins, n_frames), asynchronous on the current stream."""
        self._check_tensor(left, "left", 2)
        self._check_tensor(right, "right", 2)
        if tuple(left.shape) != tuple(right.shape):
            raise _ffi.DimensionMismatchError(f"Dimension mismatch: left has shape {tuple(left.shape)}, right {tuple(right.shape)}")
        b, n = left.shape
        out = self._out_tensor(out, (b,) + self.output_shape(n)[1:], left.device)
        self._check(self._lib.sgx_binaural_execute(self._h, left.data_ptr(), right.data_ptr(), b, n, n, out.data_ptr(), out.numel(),
                                                   _ffi.MEM_DEVICE, self._stream()))
        return out


# ---- result objects ---------------------------------------------------------------------------------------------------------------
class _BinauralSpectrogram:
    _RANGE = (0.0, 0.0)

    def __init__(self, data: np.ndarray, plan: BinauralPlan, params=None):
        self._data = data
        self._plan = plan
        self._params = plan.params if params is None else params
        self._freqs, self._times = plan.axes(data.shape[1])

    @property
    def data(self) -> np.ndarray:
        return self._data

    @property
    def dtype(self) -> str:
        return self._data.dtype.name

    @property
    def n_bins(self) -> int:
        return self._data.shape[0]

    @property
    def n_frames(self) -> int:
        return self._data.shape[1]

    @property
    def shape(self):
        return self._data.shape

    @property
    def frequencies(self) -> list:
        return self._freqs.tolist()

    @property
    def times(self) -> list:
        return self._times.tolist()

    def frequency_range(self):
        return float(self._freqs[0]), float(self._freqs[-1])

    def duration(self) -> float:
        return float(self._times[-1] - self._times[0]) if self._times.size > 1 else 0.0

    @property
    def params(self):
        return self._params

    def _hist(self, num_bins, rng, exponent, normalize) -> np.ndarray:
        lo, hi = self._RANGE if rng is None else (float(rng[0]), float(rng[1]))
        nb = 400 if num_bins is None else int(num_bins)
        if nb <= 0:
            raise ValueError("num_bins must be > 0")
        return self._plan.histogram(self._data, nb, lo, hi, exponent, normalize)

    def __array__(self, dtype=None, copy=None):
        return self._data if dtype is None else self._data.astype(dtype)

    def __repr__(self) -> str:
        return f"{type(self).__name__}(shape={self.shape}, dtype={self.dtype})"


class ItdSpectrogram(_BinauralSpectrogram):
    """ITD map in seconds (n_bins, n_frames)."""
    _RANGE = (-0.00088, 0.00088)

    def histogram(self, num_bins: Optional[int] = None, delay_range=None, energy_weighted: bool = False, normalize: bool = False):
        return self._hist(num_bins, delay_range, 1, normalize)  # energy_weighted: accepted and ignored, as in the reference


class IpdSpectrogram(_BinauralSpectrogram):
    """IPD map in radians (n_bins, n_frames)."""
    _RANGE = (-math.pi, math.pi)

    def histogram(self, num_bins: Optional[int] = None, phase_range=None, energy_weighted: bool = False, normalize: bool = False):
        return self._hist(num_bins, phase_range, 1, normalize)


class IldSpectrogram(_BinauralSpectrogram):
    """ILD map in dB (n_bins, n_frames); NaN where a channel is silent."""
    _RANGE = (-24.0, 24.0)

    def histogram(self, num_bins: Optional[int] = None, db_range=None, exponent: Optional[int] = None, energy_weighted: bool = False,
                  normalize: bool = False):
        return self._hist(num_bins, db_range, 3 if exponent is None else int(exponent), normalize)


class IlrSpectrogram(_BinauralSpectrogram):
    """ILR map in [-1, 1] (n_bins, n_frames); NaN where a channel is silent."""
    _RANGE = (-1.0, 1.0)

    def histogram(self, num_bins: Optional[int] = None, ratio_range=None, exponent: Optional[int] = None, energy_weighted: bool = False,
                  normalize: bool = False):
        return self._hist(num_bins, ratio_range, 3 if exponent is None else int(exponent), normalize)


# ---- one-shot functions with a plan cache (cleared by clear_fft_plan_cache) ---------------------------------------------------
_BIN_CACHE = _ffi.PlanCache()


def _plan(params, dtype) -> BinauralPlan:
    from .functions import _key
    key = (_key(params), parse_dtype(dtype), _ffi.current_device_key())
    return _BIN_CACHE.get(key, lambda: BinauralPlan(params, dtype))


def _pair(audio):
    """[left, right] (two 1-D arrays) or a (2, n) array -> (left, right) as f64 arrays of equal length."""
    if isinstance(audio, np.ndarray) and audio.ndim == 2:
        if audio.shape[0] != 2:
            raise ValueError(f"audio must have 2 channels, got {audio.shape[0]}")
        left, right = audio[0], audio[1]
    else:
        if len(audio) != 2:
            raise ValueError(f"audio must have 2 channels, got {len(audio)}")
        left, right = audio
    left, right = np.asarray(left), np.asarray(right)
    if left.ndim != 1 or right.ndim != 1:
        raise ValueError("each channel must be a 1-D array")
    if left.size != right.size:
        raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {left.size}, got {right.size}", expected=left.size, got=right.size)
    if left.size == 0:
        raise _ffi.InvalidInputError("Invalid input: samples must be non-empty")
    return left, right


def _compute(cls, klass, audio, params, dtype):
    if not isinstance(params, klass):
        raise TypeError(f"params must be a {klass.__name__}")
    left, right = _pair(audio)
    plan = _plan(params, dtype)
    return cls(plan.compute(left, right), plan, params)


def compute_itd_spectrogram(audio, params: ITDSpectrogramParams, dtype: str = "float64") -> ItdSpectrogram:
    """compute_itd_spectrogram (src/binaural.rs:472-560)."""
    return _compute(ItdSpectrogram, ITDSpectrogramParams, audio, params, dtype)


def compute_ipd_spectrogram(audio, params: IPDSpectrogramParams, dtype: str = "float64") -> IpdSpectrogram:
    """compute_ipd_spectrogram (src/binaural.rs:830-900)."""
    return _compute(IpdSpectrogram, IPDSpectrogramParams, audio, params, dtype)


def compute_ild_spectrogram(audio, params: ILDSpectrogramParams, dtype: str = "float64") -> IldSpectrogram:
    """compute_ild_spectrogram (src/binaural.rs:1187-1240)."""
    return _compute(IldSpectrogram, ILDSpectrogramParams, audio, params, dtype)


def compute_ilr_spectrogram(audio, params: ILRSpectrogramParams, dtype: str = "float64") -> IlrSpectrogram:
    """compute_ilr_spectrogram (src/binaural.rs:1530-1600)."""
    return _compute(IlrSpectrogram, ILRSpectrogramParams, audio, params, dtype)


def _median_finite(x: np.ndarray):
    v = np.sort(x[np.isfinite(x)])
    if v.size == 0:
        return x.dtype.type(np.nan)
    h = v.size // 2
    return v[h] if v.size % 2 else (v[h - 1] + v[h]) / x.dtype.type(2.0)


def compute_itd_spectrogram_diff(reference, test, params: ITDSpectrogramParams, dtype: str = "float64"):
    """compute_itd_spectrogram_diff (src/binaural.rs:1653-1690): (column means of test - reference over the bins,
    mean(|m| / 0.00086 * 90), median of the finite means)."""
    r = compute_itd_spectrogram(reference, params, dtype).data
    t = compute_itd_spectrogram(test, params, dtype).data
    T = r.dtype.type
    m = (t - r).sum(axis=0) / T(r.shape[0])
    mapped = np.abs(m) * T(1.0 / 0.00086) * T(90.0)
    return m, float(mapped.sum() / T(mapped.size)), float(_median_finite(m))


def compute_ilr_spectrogram_diff(reference, test, params: ILRSpectrogramParams, dtype: str = "float64"):
    """compute_ilr_spectrogram_diff (src/binaural.rs:1700-1740): (NaN-skipping column means of test - reference, NaN-skipping mean
    of their absolute values)."""
    r = compute_ilr_spectrogram(reference, params, dtype).data
    t = compute_ilr_spectrogram(test, params, dtype).data
    T = r.dtype.type
    d = t - r
    ok = ~np.isnan(d)
    cnt = ok.sum(axis=0)
    s = np.where(ok, d, T(0)).sum(axis=0)
    m = np.where(cnt > 0, s / np.maximum(cnt, 1).astype(r.dtype), T(np.nan)).astype(r.dtype)
    fin = m[~np.isnan(m)]
    mean = float(np.abs(fin).sum() / T(fin.size)) if fin.size else float("nan")
    return m, mean


__all__ = ["ITDSpectrogramParams", "IPDSpectrogramParams", "ILDSpectrogramParams", "ILRSpectrogramParams", "ItdSpectrogram",
           "IpdSpectrogram", "IldSpectrogram", "IlrSpectrogram", "BinauralPlan", "compute_itd_spectrogram", "compute_ipd_spectrogram",
           "compute_ild_spectrogram", "compute_ilr_spectrogram", "compute_itd_spectrogram_diff", "compute_ilr_spectrogram_diff"]
