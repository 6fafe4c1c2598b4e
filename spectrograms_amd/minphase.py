"""Minimum-phase conversion of FIR impulse responses (src/min_phase.rs) over the sgx_minphase_* C ABI, batched.

`minimum_phase` and `minimum_phase_with` keep the reference's names and signatures (default dtype float64) and also take a whole bank
of responses, (batch, taps); `MinPhasePlan` adds device-resident torch entry points and the route the plan runs (`kernel_name`).
The arithmetic is float64 for both dtypes (include/spectro_hip.h): `dtype` is the type of the input and output rows.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _ffi
from .params import parse_dtype

_ROUTES = {"auto": _ffi.MINPHASE_ROUTE_AUTO, "generic": _ffi.MINPHASE_ROUTE_GENERIC}
DEFAULT_OVERSAMPLE = 8  # src/min_phase.rs:33


class MinPhasePlan(_ffi.NativeHandle):
    """One sgx_minphase (taps + output length + oversampling + dtype + device + route).  Not thread-safe.

    Every row of a call is one impulse response of `taps` samples; its minimum-phase equivalent comes out truncated to
    `output_length` = min(out_len, fft_size) samples (out_len None: taps).
    """

    _prefix = "sgx_minphase"

    def __init__(self, taps: int, out_len: Optional[int] = None, oversample: int = DEFAULT_OVERSAMPLE, dtype: Optional[str] = None,
                 device: int = _ffi.DEVICE_CURRENT, route: str = "auto"):
        self._lib = _ffi.lib()
        self._dt = parse_dtype(dtype)
        if route not in _ROUTES:
            raise ValueError(f"route must be 'auto' or 'generic', got {route!r}")
        taps, oversample = int(taps), int(oversample)
        out_len = taps if out_len is None else int(out_len)
        if taps < 0 or out_len < 0 or oversample < 0:
            raise ValueError("taps, out_len and oversample must not be negative")  # usize
        ptr = C.c_void_p()
        st = self._lib.sgx_minphase_create(taps, out_len, oversample, _ROUTES[route], self._dt, int(device), C.byref(ptr))
        self._create(st, ptr)

    taps = property(lambda self: int(self._lib.sgx_minphase_taps(self._h)))
    fft_size = property(lambda self: int(self._lib.sgx_minphase_fft_size(self._h)), doc="n = next_power_of_two(taps * max(oversample, 1))")
    output_length = property(lambda self: int(self._lib.sgx_minphase_output_length(self._h)), doc="min(out_len, fft_size)")
    kernel_name = property(lambda self: self._lib.sgx_minphase_kernel_name(self._h).decode())

    def reserve(self, batch: int, host_staging: bool = True) -> None:
        """Pre-size the plan-owned scratch so that calls of up to `batch` rows do not allocate."""
        self._check(self._lib.sgx_minphase_reserve(self._h, int(batch), int(host_staging)))

    def execute(self, ir) -> np.ndarray:
        """(taps,) or (batch, taps) host array -> (output_length,) or (batch, output_length)."""
        rows, squeezed = self._host_rows(ir, "ir (taps,)")
        if rows.shape[1] != self.taps:
            raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {self.taps}, got {rows.shape[1]}", self.taps, rows.shape[1])
        out = np.empty((rows.shape[0], self.output_length), self._np)
        self._check(self._lib.sgx_minphase_execute(self._h, rows.ctypes.data, rows.shape[0], out.ctypes.data, out.size, _ffi.MEM_HOST, None))
        return out[0] if squeezed else out

    def execute_torch(self, ir, out=None):
        """(batch, taps) device tensor -> (batch, output_length), asynchronous on the current stream.  `out` must not overlap `ir`."""
        self._check_tensor(ir, "ir", 2)
        b = ir.shape[0]
        if ir.shape[1] != self.taps:
            raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {self.taps}, got {ir.shape[1]}", self.taps, ir.shape[1])
        out = self._out_tensor(out, (b, self.output_length), ir.device)
        self._check(self._lib.sgx_minphase_execute(self._h, ir.data_ptr(), b, out.data_ptr(), out.numel(), _ffi.MEM_DEVICE, self._stream()))
        return out


def minimum_phase_with(ir, out_len: int, oversample: int, dtype: Optional[str] = None) -> np.ndarray:
    """minimum_phase_with (src/min_phase.rs:67-141): `ir` is (taps,) or (batch, taps); the first min(out_len, fft_size) samples of the
    minimum-phase response of every row, fft_size = next_power_of_two(taps * max(oversample, 1))."""
    np_dt = _ffi.np_dtype(parse_dtype(dtype))
    h = np.asarray(ir, dtype=np_dt)
    if h.ndim not in (1, 2):
        raise ValueError("ir must be 1-D (taps,) or 2-D (batch, taps)")
    return MinPhasePlan(h.shape[-1], out_len, oversample, dtype).execute(h)


def minimum_phase(ir, dtype: Optional[str] = None) -> np.ndarray:
    """minimum_phase (src/min_phase.rs:55-57): the same length as `ir`, oversampling 8."""
    h = np.asarray(ir)
    return minimum_phase_with(ir, h.shape[-1] if h.ndim else 0, DEFAULT_OVERSAMPLE, dtype)


__all__ = ["MinPhasePlan", "minimum_phase", "minimum_phase_with"]
