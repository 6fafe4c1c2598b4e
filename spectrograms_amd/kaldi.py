"""Kaldi-compatible filterbank (fbank) and MFCC features over the sgx_kaldi_* C ABI, batched.

The semantics are those of `torchaudio.compliance.kaldi.fbank` / `.mfcc` with `dither = 0` and `vtln_warp = 1`, one row per batch item:
frames of `int(fs * frame_length / 1000)` samples every `int(fs * frame_shift / 1000)`, each frame's mean removed, pre-emphasised and
windowed on its own, zero-padded to the next power of two, transformed, and folded by unnormalised triangles on Kaldi's mel scale; the
natural log with a machine-epsilon floor; for MFCC the orthonormal DCT-II and the lifter.  The output is `(frames, features)` per row.
The keyword names and defaults are torchaudio's.  The tables (window, bank, DCT, lifter) are built in extended precision and rounded to
float64 before the cast to the plan's dtype; torchaudio builds them in float32.

Out of scope (`InvalidInputError` names the field): `dither != 0`, VTLN (`vtln_warp != 1`), `kaldi.spectrogram`, `min_duration`,
push / flush streaming.  Signals shorter than one frame are refused with `DimensionMismatchError` (torchaudio returns an empty matrix).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional

import numpy as np

from . import _ffi
from .params import parse_dtype

_WINDOWS = {"hanning": _ffi.KALDI_WIN_HANNING, "hamming": _ffi.KALDI_WIN_HAMMING, "povey": _ffi.KALDI_WIN_POVEY,
            "rectangular": _ffi.KALDI_WIN_RECTANGULAR, "blackman": _ffi.KALDI_WIN_BLACKMAN}
_ROUTES = {"auto": _ffi.KALDI_ROUTE_AUTO, "generic": _ffi.KALDI_ROUTE_GENERIC}


@dataclasses.dataclass(frozen=True)
class KaldiParams:
    """torchaudio.compliance.kaldi.fbank / .mfcc keywords with their defaults.  `num_ceps = 0` is fbank; `num_ceps > 0` is MFCC (which
    reads neither `use_power` nor `use_log_fbank`: the cepstra are those of the log-power bank).  `vtln_low` / `vtln_high` are accepted
    for torchaudio's signature and unused at `vtln_warp = 1`."""

    blackman_coeff: float = 0.42
    cepstral_lifter: float = 22.0
    channel: int = -1
    dither: float = 0.0
    energy_floor: float = 1.0
    frame_length: float = 25.0
    frame_shift: float = 10.0
    high_freq: float = 0.0
    htk_compat: bool = False
    low_freq: float = 20.0
    min_duration: float = 0.0
    num_ceps: int = 0
    num_mel_bins: int = 23
    preemphasis_coefficient: float = 0.97
    raw_energy: bool = True
    remove_dc_offset: bool = True
    round_to_power_of_two: bool = True
    sample_frequency: float = 16000.0
    snip_edges: bool = True
    subtract_mean: bool = False
    use_energy: bool = False
    use_log_fbank: bool = True
    use_power: bool = True
    vtln_high: float = -500.0
    vtln_low: float = 100.0
    vtln_warp: float = 1.0
    window_type: str = "povey"
    spectrogram: bool = False
    streaming: bool = False

    def __post_init__(self):
        if not isinstance(self.window_type, str) or self.window_type not in _WINDOWS:
            raise _ffi.InvalidInputError(f"Invalid input: window_type must be one of {sorted(_WINDOWS)}, got {self.window_type!r}")
        if int(self.num_mel_bins) != self.num_mel_bins or not 0 <= int(self.num_mel_bins) < 2 ** 32:
            raise _ffi.InvalidInputError(f"Invalid input: num_mel_bins must be a non-negative integer, got {self.num_mel_bins!r}")
        if int(self.num_ceps) != self.num_ceps or not 0 <= int(self.num_ceps) < 2 ** 32:
            raise _ffi.InvalidInputError(f"Invalid input: num_ceps must be a non-negative integer, got {self.num_ceps!r}")
        if self.channel not in (-1, 0):
            raise _ffi.InvalidInputError("Invalid input: channel must be -1 or 0 (a row is one channel)")


class KaldiPlan(_ffi.NativeHandle):
    """One sgx_kaldi (params + dtype + device + route).  Not thread-safe, like every plan here.

    route "auto" runs the fused kernel (`kernel_name == "k_kaldi"`) for a padded window of 256, 512, 1024 or 2048 samples and the
    generic route otherwise; `max_scratch_bytes` caps each scratch buffer of the generic route (default 256 MiB).  A row's result
    does not depend on the batch it is in."""

    _prefix = "sgx_kaldi"

    def __init__(self, params: KaldiParams, dtype: Optional[str] = "float32", device: Optional[int] = None, route: str = "auto",
                 max_scratch_bytes: Optional[int] = None):
        if not isinstance(params, KaldiParams):
            raise TypeError("params must be a KaldiParams")
        if not isinstance(route, str) or route not in _ROUTES:
            raise _ffi.InvalidInputError(f"Invalid input: route must be 'auto' or 'generic', got {route!r}")
        if max_scratch_bytes is not None and int(max_scratch_bytes) < 1:
            raise _ffi.InvalidInputError(f"Invalid input: max_scratch_bytes must be > 0, got {max_scratch_bytes!r}")
        self._lib = _ffi.lib()
        self.params = params
        self._dt = parse_dtype(dtype)
        p = _ffi.SgxKaldiParams()
        p.sample_frequency, p.frame_length_ms, p.frame_shift_ms = params.sample_frequency, params.frame_length, params.frame_shift
        p.blackman_coeff, p.preemphasis_coefficient, p.energy_floor = params.blackman_coeff, params.preemphasis_coefficient, params.energy_floor
        p.low_freq, p.high_freq, p.dither, p.vtln_warp = params.low_freq, params.high_freq, params.dither, params.vtln_warp
        p.min_duration, p.cepstral_lifter = params.min_duration, params.cepstral_lifter
        p.window_type = _WINDOWS[params.window_type]
        for f in ("remove_dc_offset", "raw_energy", "round_to_power_of_two", "snip_edges", "use_energy", "use_power", "use_log_fbank",
                  "htk_compat", "subtract_mean", "spectrogram", "streaming"):
            setattr(p, f, int(bool(getattr(params, f))))
        p.num_mel_bins, p.num_ceps = int(params.num_mel_bins), int(params.num_ceps)
        p.dtype, p.device = self._dt, _ffi.DEVICE_CURRENT if device is None else int(device)
        h = C.c_void_p()
        st = self._lib.sgx_kaldi_create(C.byref(p), _ROUTES[route], 0 if max_scratch_bytes is None else int(max_scratch_bytes), C.byref(h))
        self._create(st, h)
        self.window_size = int(self._lib.sgx_kaldi_window_size(h))
        self.window_shift = int(self._lib.sgx_kaldi_window_shift(h))
        self.padded_window_size = int(self._lib.sgx_kaldi_padded_window_size(h))
        self.n_out = int(self._lib.sgx_kaldi_n_out(h))

    kernel_name = property(lambda self: self._lib.sgx_kaldi_kernel_name(self._h).decode(), doc='"k_kaldi" or "kaldi_generic"')
    tile = property(lambda self: int(self._lib.sgx_kaldi_tile(self._h)), doc="frames per workgroup tile of k_kaldi; 0 on the generic route")
    allocations = property(lambda self: int(self._lib.sgx_kaldi_allocations(self._h)),
                           doc="how often the plan has allocated or replaced one of its own buffers (it stands still within what reserve() sized)")

    def _table(self, fn, shape) -> np.ndarray:
        t = np.empty(shape, np.float64)
        if t.size:
            self._check(fn(self._h, t.ctypes.data_as(C.POINTER(C.c_double))))
        return t

    def window(self) -> np.ndarray:
        """(window_size,) f64: the window as built, before the cast to the plan's dtype."""
        return self._table(self._lib.sgx_kaldi_window, (self.window_size,))

    def mel_banks(self) -> np.ndarray:
        """(num_mel_bins, padded_window_size // 2 + 1) f64, dense; the last column (Nyquist) is zero."""
        return self._table(self._lib.sgx_kaldi_mel_banks, (int(self.params.num_mel_bins), self.padded_window_size // 2 + 1))

    def dct(self) -> np.ndarray:
        """(num_ceps, num_mel_bins) f64: the first rows of the orthonormal DCT-II."""
        return self._table(self._lib.sgx_kaldi_dct, (int(self.params.num_ceps), int(self.params.num_mel_bins)))

    def lifter(self) -> np.ndarray:
        """(num_ceps,) f64: 1 + Q / 2 sin(pi i / Q), ones for Q = 0."""
        return self._table(self._lib.sgx_kaldi_lifter, (int(self.params.num_ceps),))

    def n_frames(self, n_samples: int) -> int:
        """m for a row of n_samples; 0 for rows shorter than one frame."""
        return int(self._lib.sgx_kaldi_n_frames(self._h, int(n_samples)))

    def reserve(self, batch: int, n_samples: int, host_staging: bool = True) -> None:
        """Pre-size the plan-owned scratch so that calls of up to `batch` rows of `n_samples` samples do not allocate."""
        self._check(self._lib.sgx_kaldi_reserve(self._h, int(batch), int(n_samples), int(host_staging)))

    # ---- host arrays ------------------------------------------------------------------------------------------------------
    def compute(self, x) -> np.ndarray:
        """(n,) or (batch, n) -> (m, n_out) or (batch, m, n_out)."""
        xb, squeezed = self._host_rows(x, "waveform (n,)")
        b, n = xb.shape
        out = np.empty((b, self.n_frames(n), self.n_out), self._np)
        self._check(self._lib.sgx_kaldi_execute(self._h, xb.ctypes.data, b, n, n, out.ctypes.data, out.size, _ffi.MEM_HOST, None))
        return out[0] if squeezed else out

    # ---- device tensors (torch), on the current stream --------------------------------------------------------------------
    def compute_torch(self, x, out=None):
        """(batch, n) device tensor -> (batch, m, n_out), asynchronous on the current stream.  Rows may be a slice `X[:, a:b]` of a
        resident tensor (unit inner stride)."""
        stride = self._check_tensor(x, "waveform", 2, rows_may_stride=True)
        b, n = x.shape
        m = self.n_frames(n)
        if m == 0:
            raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {self.window_size}, got {n} (n_samples must be at least "
                                              "the window size)", self.window_size, n)
        out = self._out_tensor(out, (b, m, self.n_out), x.device)
        self._check(self._lib.sgx_kaldi_execute(self._h, x.data_ptr(), b, n, stride, out.data_ptr(), out.numel(), _ffi.MEM_DEVICE,
                                                self._stream()))
        return out


# ---- one-shot functions with a plan cache (cleared by clear_fft_plan_cache) ---------------------------------------------------
_KALDI_CACHE = _ffi.PlanCache()


def _one_shot(waveform, params: KaldiParams, dtype):
    if dtype is None:
        dtype = "float64" if getattr(waveform, "dtype", None) == np.float64 else "float32"
    key = (params, parse_dtype(dtype), _ffi.current_device_key())
    return _KALDI_CACHE.get(key, lambda: KaldiPlan(params, dtype)).compute(waveform)


def kaldi_fbank(waveform, dtype: Optional[str] = None, **kwargs):
    """torchaudio.compliance.kaldi.fbank on (n,) or (batch, n) host rows -> (m, n_out) or (batch, m, n_out).  The keywords are
    KaldiParams' (torchaudio's); dtype defaults to the waveform's when that is float64, else float32."""
    if kwargs.get("num_ceps", 0):
        raise _ffi.InvalidInputError("Invalid input: num_ceps is kaldi_mfcc's")
    return _one_shot(waveform, KaldiParams(**kwargs), dtype)


def kaldi_mfcc(waveform, dtype: Optional[str] = None, **kwargs):
    """torchaudio.compliance.kaldi.mfcc (num_ceps = 13 unless given) -> (m, num_ceps) or (batch, m, num_ceps)."""
    kwargs.setdefault("num_ceps", 13)
    if not kwargs["num_ceps"]:
        raise _ffi.InvalidInputError("Invalid input: num_ceps must be > 0 for kaldi_mfcc")
    return _one_shot(waveform, KaldiParams(**kwargs), dtype)


__all__ = ["KaldiParams", "KaldiPlan", "kaldi_fbank", "kaldi_mfcc"]
