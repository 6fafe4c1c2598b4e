"""Sample-rate conversion over the sgx_resample_* C ABI, batched: the step in front of every plan when the audio is not at the plan's rate.

`ResamplePlan` and `resample` take the arguments of `torchaudio.functional.resample` and keep its semantics (the windowed-sinc polyphase
filter; include/spectro_hip.h states the definition).  A plan resamples whole rows (`resample`), or rows that arrive in blocks
(`process` ... `flush`): every output is one fma chain over its own K samples, so the blocks' outputs, laid end to end, are bit for bit
those of one call on the whole rows.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _ffi
from .params import parse_dtype

_ROUTES = {"auto": _ffi.RESAMPLE_ROUTE_AUTO, "generic": _ffi.RESAMPLE_ROUTE_GENERIC}
_METHODS = {"sinc_interp_hann": _ffi.RESAMPLE_SINC_HANN, "sinc_interp_kaiser": _ffi.RESAMPLE_SINC_KAISER}
_KAISER_BETA = 14.769656459379492


class ResamplePlan(_ffi.NativeHandle):
    """One sgx_resample (rates + filter + dtype + device + route + the rows' last K - 1 samples).  Not thread-safe, like `FirPlan`.

    `resample` is the stateless form ((n,) or (batch, n) -> (..., out_len(n))); `process` hands new samples to `batch` rows that run in
    lock step and returns the outputs whose whole window is known, `flush` the rest (the future taken as zeros), after which the plan
    stands as after `reset`.  The first `process` after creation, `reset` or `flush` fixes the batch.
    """

    _prefix = "sgx_resample"

    def __init__(self, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                 resampling_method: str = "sinc_interp_hann", beta: Optional[float] = None, dtype: Optional[str] = None,
                 device: int = _ffi.DEVICE_CURRENT, route: str = "auto"):
        self._lib = _ffi.lib()
        self._dt = parse_dtype(dtype)
        if route not in _ROUTES:
            raise ValueError(f"route must be 'auto' or 'generic', got {route!r}")
        for name, v in (("orig_freq", orig_freq), ("new_freq", new_freq), ("lowpass_filter_width", lowpass_filter_width)):
            if int(v) != v:
                raise _ffi.InvalidInputError(f"Invalid input: {name} must be an integer, got {v!r}")
            if abs(int(v)) >= 2 ** 62:
                raise _ffi.InvalidInputError(f"Invalid input: {name} is out of range")
        if resampling_method not in _METHODS:
            raise _ffi.InvalidInputError(f"Invalid input: resampling_method must be sinc_interp_hann or sinc_interp_kaiser, got {resampling_method!r}")
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        lpw = max(-1, min(int(lowpass_filter_width), 2 ** 31 - 1))
        ptr = C.c_void_p()
        st = self._lib.sgx_resample_create(self.orig_freq, self.new_freq, lpw, float(rolloff), _METHODS[resampling_method],
                                           _KAISER_BETA if beta is None else float(beta), _ROUTES[route], self._dt, int(device), C.byref(ptr))
        self._create(st, ptr)
        self._rows = 0         # fixed by the first process(); reset() and flush() free it
        self._squeeze = False  # the blocks are 1-D: the outputs come back without the batch axis
        self._torch = None     # the device of the last processed tensor (None: NumPy blocks)

    up = property(lambda self: int(self._lib.sgx_resample_up(self._h)), doc="L = new_freq / gcd")
    down = property(lambda self: int(self._lib.sgx_resample_down(self._h)), doc="M = orig_freq / gcd")
    taps_per_phase = property(lambda self: int(self._lib.sgx_resample_taps_per_phase(self._h)), doc="K")
    tile = property(lambda self: int(self._lib.sgx_resample_tile(self._h)), doc="outputs per workgroup tile of k_resample_pp; 0 on the generic route")
    consumed = property(lambda self: int(self._lib.sgx_resample_consumed(self._h)), doc="samples per row since creation / reset / flush")
    emitted = property(lambda self: int(self._lib.sgx_resample_emitted(self._h)), doc="outputs per row since creation / reset / flush")
    allocations = property(lambda self: int(self._lib.sgx_resample_allocations(self._h)),
                           doc="how often the plan has allocated or replaced one of its own buffers (it stands still within what reserve() sized)")
    kernel_name = property(lambda self: self._lib.sgx_resample_kernel_name(self._h).decode())

    def taps(self) -> np.ndarray:
        """The (L, K) table c[p][k] as the plan's kernels read it: the T-valued coefficients, as float64."""
        t = np.empty((self.up, self.taps_per_phase), np.float64)
        self._check(self._lib.sgx_resample_taps(self._h, t.ctypes.data_as(C.POINTER(C.c_double))))
        return t

    def phase_offsets(self) -> np.ndarray:
        """j0(p), (L,) int64: output q L + p reads the samples q M + j0(p) + k, k < K."""
        j = np.empty(self.up, np.int64)
        self._check(self._lib.sgx_resample_phase_offsets(self._h, j.ctypes.data_as(C.POINTER(C.c_int64))))
        return j

    def out_len(self, n_samples: int) -> int:
        """ceil(n_samples L / M): the outputs of `resample` on rows of n_samples samples."""
        return int(self._lib.sgx_resample_out_len(self._h, int(n_samples)))

    def step(self, consumed: int, n_samples: int):
        """(outputs per row, samples consumed afterwards) of a `process` of n_samples samples on a stream that has consumed `consumed`;
        n_samples = 0 asks for the `flush` after `consumed` samples."""
        m, after = C.c_size_t(), C.c_size_t()
        self._check(self._lib.sgx_resample_step(self._h, int(consumed), int(n_samples), C.byref(m), C.byref(after)))
        return m.value, after.value

    def reset(self) -> None:
        """Zero history, nothing consumed, and the row count of the next `process` is free again."""
        self._check(self._lib.sgx_resample_reset(self._h, self._stream()))
        self._rows, self._squeeze, self._torch = 0, False, None

    def reserve(self, batch: int, max_block: int, host_staging: bool = True) -> None:
        """Pre-size the history and the host staging so that calls of up to `max_block` samples on `batch` rows do not allocate."""
        self._check(self._lib.sgx_resample_reserve(self._h, int(batch), int(max_block), int(host_staging)))

    # ---- host arrays ------------------------------------------------------------------------------------------------------
    def resample(self, x) -> np.ndarray:
        """Stateless: (n,) or (batch, n) -> (..., out_len(n)); the plan's history is not touched."""
        xb, sq = self._host_rows(x, "samples (n,)")
        b, n = xb.shape
        out = np.empty((b, self.out_len(n)), self._np)
        self._check(self._lib.sgx_resample_resample(self._h, xb.ctypes.data, b, n, n, out.ctypes.data, out.size, _ffi.MEM_HOST, None))
        return out[0] if sq else out

    def process(self, x) -> np.ndarray:
        """Streaming: (n,) or (batch, n) new samples -> the `step(consumed, n)[0]` outputs per row that became complete (possibly none)."""
        xb, sq = self._host_rows(x, "samples (n,)")
        b, n = xb.shape
        out = np.empty((b, self.step(self.consumed, n)[0] if n else 0), self._np)
        self._check(self._lib.sgx_resample_process(self._h, xb.ctypes.data, b, n, n, out.ctypes.data if out.size else None, out.size,
                                                   _ffi.MEM_HOST, None))
        self._rows, self._squeeze, self._torch = b, sq, None
        return out[0] if sq else out

    def flush(self) -> np.ndarray:
        """The outputs that were waiting for later samples (taken as zeros), shaped as `process` returns them; then as after `reset`."""
        if self._torch is not None:
            raise ValueError("the stream's blocks were tensors: use flush_torch()")
        rows, sq = max(self._rows, 1), self._squeeze or self._rows == 0
        out = np.empty((rows, self.step(self.consumed, 0)[0] if self._rows else 0), self._np)
        self._check(self._lib.sgx_resample_flush(self._h, out.ctypes.data if out.size else None, out.size, _ffi.MEM_HOST, None))
        self._rows, self._squeeze = 0, False
        return out[0] if sq else out

    # ---- device tensors (torch), on the current stream --------------------------------------------------------------------
    def resample_torch(self, x, out=None):
        """(batch, n) device tensor -> (batch, out_len(n)), asynchronous on the current stream.  `out` must not overlap `x`."""
        stride = self._check_tensor(x, "samples", 2, rows_may_stride=True)
        b, n = x.shape
        out = self._out_tensor(out, (b, self.out_len(n)), x.device)
        self._check(self._lib.sgx_resample_resample(self._h, x.data_ptr(), b, n, stride, out.data_ptr(), out.numel(), _ffi.MEM_DEVICE, self._stream()))
        return out

    def process_torch(self, x, out=None):
        """(batch, n) new samples on the device -> (batch, step(consumed, n)[0]), asynchronous on the current stream."""
        stride = self._check_tensor(x, "samples", 2, rows_may_stride=True)
        b, n = x.shape
        out = self._out_tensor(out, (b, self.step(self.consumed, n)[0] if n else 0), x.device)
        self._check(self._lib.sgx_resample_process(self._h, x.data_ptr(), b, n, stride, out.data_ptr() if out.numel() else None, out.numel(),
                                                   _ffi.MEM_DEVICE, self._stream()))
        self._rows, self._squeeze, self._torch = b, False, x.device
        return out

    def flush_torch(self, out=None):
        """(batch, m) on the device of the last `process_torch`, asynchronous on the current stream; then as after `reset`."""
        if self._torch is None:
            raise ValueError("flush_torch() follows process_torch()")
        out = self._out_tensor(out, (self._rows, self.step(self.consumed, 0)[0]), self._torch)
        self._check(self._lib.sgx_resample_flush(self._h, out.data_ptr() if out.numel() else None, out.numel(), _ffi.MEM_DEVICE, self._stream()))
        self._rows, self._squeeze, self._torch = 0, False, None
        return out


def resample(signal, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
             resampling_method: str = "sinc_interp_hann", beta: Optional[float] = None, dtype: Optional[str] = None) -> np.ndarray:
    """torchaudio.functional.resample's semantics on (n,) or (batch, n) rows: the band-limited signal at new_freq, ceil(n L / M) samples."""
    x = np.asarray(signal)
    if x.ndim not in (1, 2):
        raise ValueError("signal must be 1-D (n,) or 2-D (batch, n)")
    if x.shape[-1] == 0:
        raise _ffi.InvalidInputError("Invalid input: signal must not be empty")
    return ResamplePlan(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta, dtype).resample(x)


__all__ = ["ResamplePlan", "resample"]
