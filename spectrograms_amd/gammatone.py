"""Time-domain gammatone IIR spectrograms (src/erb.rs:405-654) over the sgx_gammatone_* C ABI, batched.

`gammatone_iir_spectrogram` / `gammatone_center_frequencies` keep the reference's names and argument order (default dtype float64);
`GammatonePlan` adds batched calls ((batch, n) signals in one launch), device-resident torch entry points, the coefficients as built and
the kernel the plan runs (`kernel_name`).  The ERB spectrogram plans of the planner are the reference's frequency-domain approximation
of this filter bank; this is the filter bank itself.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _ffi
from .params import ErbParams, parse_dtype

N_COEFFS = 11  # SGX_GAMMATONE_COEFFS


class GammatonePlan(_ffi.NativeHandle):
    """One sgx_gammatone (sample rate, framing, ErbParams, dtype, device).  Not thread-safe, like the other plans."""

    _prefix = "sgx_gammatone"

    def __init__(self, sample_rate: float, frame_size: int, hop_size: int, erb_params: ErbParams, dtype: Optional[str] = None,
                 device: int = _ffi.DEVICE_CURRENT):
        if not isinstance(erb_params, ErbParams):
            raise TypeError("erb_params must be an ErbParams")
        fs, hs = int(frame_size), int(hop_size)
        if fs <= 0:  # NonZeroUsize
            raise ValueError("frame_size must be > 0")
        if hs <= 0:
            raise ValueError("hop_size must be > 0")
        self._lib = _ffi.lib()
        self.sample_rate, self.frame_size, self.hop_size, self.erb_params = float(sample_rate), fs, hs, erb_params
        self._dt = parse_dtype(dtype)
        floor = erb_params.db_floor
        h = C.c_void_p()
        st = self._lib.sgx_gammatone_create(self.sample_rate, fs, hs, erb_params.n_filters, erb_params.f_min, erb_params.f_max,
                                            1 if erb_params.spacing == "apple_tr35" else 0, int(floor is not None),
                                            0.0 if floor is None else float(floor), self._dt, int(device), C.byref(h))
        self._create(st, h)

    @property
    def n_bands(self) -> int:
        return self.erb_params.n_filters

    @property
    def kernel_name(self) -> str:
        return self._lib.sgx_gammatone_kernel_name(self._h).decode()

    @property
    def center_frequencies(self) -> np.ndarray:
        """Band centre frequencies in Hz, low to high."""
        out = np.empty(self.n_bands, np.float64)
        self._check(self._lib.sgx_gammatone_center_frequencies(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def coefficients(self) -> dict:
        """The filter coefficients as built (f64) and as the kernel reads them: `a` (n_bands, 4, 2) = (a0_k, a1_k) per section, section
        1 already divided by the gain; `b1`, `b2`, `gain` (n_bands,)."""
        raw = np.empty((self.n_bands, N_COEFFS), np.float64)
        self._check(self._lib.sgx_gammatone_coefficients(self._h, raw.ctypes.data_as(C.POINTER(C.c_double))))
        return {"a": raw[:, :8].reshape(self.n_bands, 4, 2).copy(), "b1": raw[:, 8].copy(), "b2": raw[:, 9].copy(),
                "gain": raw[:, 10].copy()}

    def output_shape(self, n_samples: int):
        """(n_bands, n_frames) for a signal of n_samples samples."""
        nb, nf = C.c_size_t(), C.c_size_t()
        self._check(self._lib.sgx_gammatone_output_shape(self._h, int(n_samples), C.byref(nb), C.byref(nf)))
        return nb.value, nf.value

    def reserve(self, batch: int, n_samples: int, host_staging: bool = True) -> None:
        """Pre-size the plan-owned host staging so that calls of up to `batch` signals of `n_samples` samples do not allocate."""
        self._check(self._lib.sgx_gammatone_reserve(self._h, int(batch), int(n_samples), int(host_staging)))

    # ---- host arrays ------------------------------------------------------------------------------------------------------
    def compute(self, x) -> np.ndarray:
        """1-D (n,) -> (n_bands, n_frames); 2-D (batch, n) -> (batch, n_bands, n_frames)."""
        a = np.asarray(x)
        if a.ndim not in (1, 2):
            raise ValueError("samples must be 1-D (n,) or 2-D (batch, n)")
        xb = a[None] if a.ndim == 1 else a
        if xb.shape[0] == 0:
            raise ValueError("batch must be > 0")
        b, n = xb.shape
        nb, nf = self.output_shape(n)
        es = np.dtype(self._np).itemsize
        # rows of a wider array keep their stride (no copy); anything else is made dense
        if xb.dtype != self._np or xb.strides[1] != es or (b > 1 and (xb.strides[0] % es or xb.strides[0] < n * es)):
            xb = np.ascontiguousarray(xb, dtype=self._np)
        stride = xb.strides[0] // es if b > 1 else n
        out = np.empty((b, nb, nf), self._np)
        self._check(self._lib.sgx_gammatone_execute(self._h, xb.ctypes.data, b, n, stride, out.ctypes.data, out.size, _ffi.MEM_HOST, None))
        return out[0] if a.ndim == 1 else out

    # ---- device tensors (torch), on the current stream --------------------------------------------------------------------
    def compute_torch(self, x, out=None):
        """(batch, n) device tensor (unit stride along n, any row stride >= n) -> (batch, n_bands, n_frames), asynchronous on the
        current stream."""
        stride = self._check_tensor(x, "samples", 2, rows_may_stride=True)
        b, n = x.shape
        out = self._out_tensor(out, (b,) + self.output_shape(n), x.device)
        self._check(self._lib.sgx_gammatone_execute(self._h, x.data_ptr(), b, n, stride, out.data_ptr(), out.numel(), _ffi.MEM_DEVICE,
                                                    self._stream()))
        return out


# ---- one-shot functions with a plan cache (cleared by clear_fft_plan_cache) ---------------------------------------------------
_GT_CACHE = _ffi.PlanCache()


def _plan(sample_rate, frame_size, hop_size, erb_params, dtype) -> GammatonePlan:
    from .functions import _key
    key = (float(sample_rate), int(frame_size), int(hop_size), _key(erb_params), parse_dtype(dtype), _ffi.current_device_key())
    return _GT_CACHE.get(key, lambda: GammatonePlan(sample_rate, frame_size, hop_size, erb_params, dtype))


def gammatone_iir_spectrogram(samples, sample_rate: float, frame_size: int, hop_size: int, erb_params: ErbParams,
                              dtype: Optional[str] = None):
    """gammatone_iir_spectrogram (src/erb.rs:603-654): mono samples -> ((n_bands, n_frames) in the chosen dtype, centre frequencies)."""
    if np.ndim(samples) != 1:
        raise ValueError("samples must be 1-D (mono)")
    plan = _plan(sample_rate, frame_size, hop_size, erb_params, dtype)
    return plan.compute(samples), plan.center_frequencies


def gammatone_center_frequencies(erb_params: ErbParams) -> np.ndarray:
    """gammatone_center_frequencies (src/erb.rs:585-601): the band centres in Hz, low to high, without running the filter bank."""
    return GammatonePlan(1.0, 2, 1, erb_params, device=_ffi.DEVICE_HOST_ONLY).center_frequencies


__all__ = ["GammatonePlan", "gammatone_iir_spectrogram", "gammatone_center_frequencies"]
