"""IIR filtering over the sgx_iir_* C ABI (include/spectro_hip_iir.h): cascades of second-order sections along whole rows, batched.

`sosfilt`, `sosfiltfilt` and `sosfilt_zi` keep scipy.signal's names, layouts (`sos` is (S, 6) rows of b0 b1 b2 a0 a1 a2 with a0 == 1,
the state (S, 2) per row) and results; `biquad` and the `*_biquad` coefficient helpers keep torchaudio.functional's names and the RBJ
cookbook formulas it uses (each helper returns one `sos` row; `biquad` does not clamp its output).  `IirPlan` adds batched calls
((batch, n) rows in one launch, one filter for all rows or one per row), streaming calls of any length with the state kept on the
device, zero-phase filtering without a flipped or extended copy, device-resident torch entry points, and the route the plan runs
(`kernel_name`).  Default dtype float64, as the other one-shot functions.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from . import _ffi
from .params import parse_dtype

_ROUTES = {"auto": _ffi.IIR_ROUTE_AUTO, "split": _ffi.IIR_ROUTE_SPLIT, "chain": _ffi.IIR_ROUTE_CHAIN}
_F64P = C.POINTER(C.c_double)


def _sos_array(sos) -> np.ndarray:
    s = np.ascontiguousarray(sos, dtype=np.float64)
    if s.ndim not in (2, 3) or s.shape[-1] != 6:
        raise ValueError(f"sos must be (n_sections, 6) or (rows, n_sections, 6), got shape {s.shape}")
    if s.ndim == 3 and s.shape[0] == 0:
        raise ValueError("sos must have at least one row")
    return s


class IirPlan(_ffi.NativeHandle):
    """One sgx_iir (sections + dtype + device + route).  Not thread-safe.

    `sos` is (S, 6) — one filter for every row — or (rows, S, 6) — one per row of every call.  `filter` is stateless (n in, n out, from
    zero state or `zi`), `process` the streaming form (the state moves on; pushes agree with one `filter` call over the concatenation to
    within rounding, not bit for bit: the block boundaries move with the pushes), `filtfilt` scipy's sosfiltfilt with odd padding.
    """

    _prefix = "sgx_iir"

    def __init__(self, sos, dtype: Optional[str] = None, device: int = _ffi.DEVICE_CURRENT, route: str = "auto"):
        self._lib = _ffi.lib()
        self._dt = parse_dtype(dtype)
        if route not in _ROUTES:
            raise ValueError(f"route must be 'auto', 'split' or 'chain', got {route!r}")
        s = _sos_array(sos)
        rows, n_sections = (1, s.shape[0]) if s.ndim == 2 else s.shape[:2]
        self._per_row, self._sos_rows = s.ndim == 3, rows
        ptr = C.c_void_p()
        st = self._lib.sgx_iir_create(s.ctypes.data_as(_F64P) if s.size else None, n_sections, rows, _ROUTES[route], self._dt, int(device),
                                      C.byref(ptr))
        self._create(st, ptr)
        self._device = int(self._lib.sgx_iir_device(ptr))  # (_create reads the device of the families in _ffi.SIGNATURES only)

    n_sections = property(lambda self: int(self._lib.sgx_iir_n_sections(self._h)))
    padlen = property(lambda self: int(self._lib.sgx_iir_padlen(self._h)), doc="filtfilt's default padlen (scipy's)")
    tile = property(lambda self: int(self._lib.sgx_iir_tile(self._h)), doc="samples per workgroup tile, 256 * block (0 on the chain route)")
    block = property(lambda self: int(self._lib.sgx_iir_block(self._h)), doc="L: samples per work item")
    allocations = property(lambda self: int(self._lib.sgx_iir_allocations(self._h)), doc="(re)allocations of plan-owned device buffers")
    kernel_name = property(lambda self: self._lib.sgx_iir_kernel_name(self._h).decode(), doc="the route of the last call")

    def transition(self, j: int) -> np.ndarray:
        """M^(2^j), j = 0 .. 7: the state-transition table of 2^j blocks, (2 S', 2 S') for the first S' = min(S, 8) sections."""
        d = 2 * min(self.n_sections, 8)
        m = np.empty((d, d), np.float64)
        self._check(self._lib.sgx_iir_transition(self._h, int(j), m.ctypes.data_as(_F64P)))
        return m

    def zi(self) -> np.ndarray:
        """scipy.signal.sosfilt_zi of the plan's filter(s): (S, 2) or (rows, S, 2)."""
        z = np.empty((self._sos_rows, self.n_sections, 2), np.float64)
        self._check(self._lib.sgx_iir_zi(self._h, z.ctypes.data_as(_F64P)))
        return z if self._per_row else z[0]

    def reset(self) -> None:
        """Zero state, and the row count of the next streaming call is free again."""
        self._check(self._lib.sgx_iir_reset(self._h, self._stream()))

    def reserve(self, batch: int, n_samples: int, host_staging: bool = True) -> None:
        """Pre-size the state and the plan-owned scratch so that calls of up to `batch` rows of `n_samples` samples do not allocate."""
        self._check(self._lib.sgx_iir_reserve(self._h, int(batch), int(n_samples), int(host_staging)))

    def state(self, rows: int) -> np.ndarray:
        """The streaming state of `rows` rows, (rows, S, 2) float64, behind everything queued on the current stream."""
        z = np.empty((int(rows), self.n_sections, 2), np.float64)
        self._check(self._lib.sgx_iir_state(self._h, z.ctypes.data_as(_F64P), z.size, self._stream()))
        return z

    def set_state(self, z) -> None:
        """Replace the streaming state by `z` (rows, S, 2); fixes the row count as a first `process` does."""
        z = np.ascontiguousarray(z, dtype=np.float64)
        if z.ndim != 3 or z.shape[1:] != (self.n_sections, 2) or z.shape[0] == 0:
            raise ValueError(f"state must be (rows, {self.n_sections}, 2), got shape {z.shape}")
        self._check(self._lib.sgx_iir_set_state(self._h, z.ctypes.data_as(_F64P), z.shape[0], self._stream()))

    def _pad(self, padlen) -> int:
        if padlen is None:
            return -1
        if int(padlen) < 0:
            raise ValueError("padlen must be >= 0")
        return int(padlen)

    def _state_shape(self, batch):
        return (batch, self.n_sections, 2)

    # ---- host arrays ------------------------------------------------------------------------------------------------------
    def filter(self, x, zi=None, return_zf: bool = False):
        """(n,) or (batch, n) -> the same shape, from zero state or from `zi` (S, 2) / (batch, S, 2); with `return_zf` (or a `zi`, as
        scipy) also the final state."""
        xb, squeezed = self._host_rows(x, "samples (n,)")
        b, n = xb.shape
        want_zf = return_zf or zi is not None
        zin = None
        if zi is not None:
            zin = np.ascontiguousarray(zi, dtype=np.float64)
            if squeezed and zin.ndim == 2:
                zin = zin[None]
            if zin.shape != self._state_shape(b):
                raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected zi of shape {self._state_shape(b)[0 if not squeezed else 1:]}, "
                                                  f"got {np.shape(zi)}", self._state_shape(b), np.shape(zi))
        out = np.empty((b, n), self._np)
        zf = np.empty(self._state_shape(b), np.float64) if want_zf else None
        self._check(self._lib.sgx_iir_filter(self._h, xb.ctypes.data, b, n, n, out.ctypes.data, out.size,
                                             zin.ctypes.data if zin is not None else None, zf.ctypes.data if want_zf else None,
                                             _ffi.MEM_HOST, None))
        y = out[0] if squeezed else out
        return (y, zf[0] if squeezed else zf) if want_zf else y

    def process(self, x) -> np.ndarray:
        """Streaming: (n,) or (batch, n) -> the same shape, n >= 0; the rows' state moves on."""
        xb, squeezed = self._host_rows(x, "samples (n,)")
        out = np.empty(xb.shape, self._np)
        self._check(self._lib.sgx_iir_process(self._h, xb.ctypes.data, xb.shape[0], xb.shape[1], xb.shape[1], out.ctypes.data, out.size,
                                              _ffi.MEM_HOST, None))
        return out[0] if squeezed else out

    def filtfilt(self, x, padlen: Optional[int] = None) -> np.ndarray:
        """Zero-phase: scipy.signal.sosfiltfilt(sos, x, padtype="odd", padlen=padlen) per row."""
        xb, squeezed = self._host_rows(x, "samples (n,)")
        out = np.empty(xb.shape, self._np)
        self._check(self._lib.sgx_iir_filtfilt(self._h, xb.ctypes.data, xb.shape[0], xb.shape[1], xb.shape[1], out.ctypes.data, out.size,
                                               self._pad(padlen), _ffi.MEM_HOST, None))
        return out[0] if squeezed else out

    # ---- device tensors (torch), on the current stream --------------------------------------------------------------------
    def _state_tensor(self, t, what, batch):
        import torch
        self._check_tensor(t, what, 3, dtype=torch.float64)
        if tuple(t.shape) != self._state_shape(batch):
            raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {what} of shape {self._state_shape(batch)}, got {tuple(t.shape)}",
                                              self._state_shape(batch), tuple(t.shape))
        return t.data_ptr()

    def filter_torch(self, x, zi=None, zf=None, out=None):
        """(batch, n) device tensor -> (batch, n), asynchronous on the current stream; `zi` and `zf` are float64 device tensors
        (batch, S, 2), the second written with the final state.  `out` must not overlap `x`."""
        self._check_tensor(x, "samples", 2)
        b, n = x.shape
        zin = self._state_tensor(zi, "zi", b) if zi is not None else None
        zout = self._state_tensor(zf, "zf", b) if zf is not None else None
        out = self._out_tensor(out, (b, n), x.device)
        self._check(self._lib.sgx_iir_filter(self._h, x.data_ptr(), b, n, n, out.data_ptr(), out.numel(), zin, zout, _ffi.MEM_DEVICE,
                                             self._stream()))
        return out

    def process_torch(self, x, out=None):
        """(batch, n) device tensor, n >= 0 -> (batch, n), asynchronous on the current stream; the state stays on the device."""
        self._on_device(x, "samples")
        if x.dim() == 2 and x.shape[0] > 0 and x.shape[1] == 0 and x.dtype == self._tdt:
            b, n = x.shape
        else:
            self._check_tensor(x, "samples", 2)
            b, n = x.shape
        out = self._out_tensor(out, (b, n), x.device)
        self._check(self._lib.sgx_iir_process(self._h, x.data_ptr(), b, n, n, out.data_ptr(), out.numel(), _ffi.MEM_DEVICE, self._stream()))
        return out

    def filtfilt_torch(self, x, padlen: Optional[int] = None, out=None):
        """(batch, n) device tensor -> (batch, n), zero-phase, asynchronous on the current stream."""
        self._check_tensor(x, "samples", 2)
        b, n = x.shape
        out = self._out_tensor(out, (b, n), x.device)
        self._check(self._lib.sgx_iir_filtfilt(self._h, x.data_ptr(), b, n, n, out.data_ptr(), out.numel(), self._pad(padlen),
                                               _ffi.MEM_DEVICE, self._stream()))
        return out


# ---- one-shot functions -------------------------------------------------------------------------------------------------------
_PLANS = _ffi.PlanCache()


def _plan(sos, dtype) -> IirPlan:
    s = _sos_array(sos)
    key = (s.shape, s.tobytes(), parse_dtype(dtype), _ffi.current_device_key())
    return _PLANS.get(key, lambda: IirPlan(s, dtype=dtype))


def sosfilt(sos, x, zi=None, dtype: Optional[str] = None):
    """scipy.signal.sosfilt along the last axis: `x` is (n,) or (batch, n); with `zi` returns (y, zf)."""
    return _plan(sos, dtype).filter(x, zi)


def sosfiltfilt(sos, x, padlen: Optional[int] = None, dtype: Optional[str] = None) -> np.ndarray:
    """scipy.signal.sosfiltfilt(sos, x, padtype="odd", padlen=padlen) along the last axis."""
    return _plan(sos, dtype).filtfilt(x, padlen)


def sosfilt_zi(sos) -> np.ndarray:
    """scipy.signal.sosfilt_zi: the state of the step response's steady state, (S, 2); solved on the host in long double."""
    return IirPlan(sos, dtype="float64", device=_ffi.DEVICE_HOST_ONLY).zi()


def _row(b0, b1, b2, a0, a1, a2) -> np.ndarray:
    return np.array([b0 / a0, b1 / a0, b2 / a0, 1.0, a1 / a0, a2 / a0], np.float64)


def biquad(x, b0: float, b1: float, b2: float, a0: float, a1: float, a2: float, dtype: Optional[str] = None) -> np.ndarray:
    """torchaudio.functional.biquad without its clamp: one section, normalised by a0."""
    if not a0:
        raise _ffi.InvalidInputError("Invalid input: a0 must not be 0")
    return sosfilt(_row(b0, b1, b2, a0, a1, a2)[None], x, dtype=dtype)


def _rbj(sample_rate: float, freq: float, Q: float):
    if not (sample_rate > 0 and 0 < freq < sample_rate / 2 and Q > 0):
        raise _ffi.InvalidInputError("Invalid input: need sample_rate > 0, 0 < frequency < sample_rate / 2 and Q > 0")
    w0 = 2.0 * math.pi * freq / sample_rate
    return math.cos(w0), math.sin(w0), math.sin(w0) / (2.0 * Q)


def lowpass_biquad(sample_rate: float, cutoff_freq: float, Q: float = 0.707) -> np.ndarray:
    c, _, al = _rbj(sample_rate, cutoff_freq, Q)
    return _row((1 - c) / 2, 1 - c, (1 - c) / 2, 1 + al, -2 * c, 1 - al)


def highpass_biquad(sample_rate: float, cutoff_freq: float, Q: float = 0.707) -> np.ndarray:
    c, _, al = _rbj(sample_rate, cutoff_freq, Q)
    return _row((1 + c) / 2, -1 - c, (1 + c) / 2, 1 + al, -2 * c, 1 - al)


def bandpass_biquad(sample_rate: float, central_freq: float, Q: float = 0.707, const_skirt_gain: bool = False) -> np.ndarray:
    c, s, al = _rbj(sample_rate, central_freq, Q)
    t = s / 2 if const_skirt_gain else al
    return _row(t, 0.0, -t, 1 + al, -2 * c, 1 - al)


def bandreject_biquad(sample_rate: float, central_freq: float, Q: float = 0.707) -> np.ndarray:
    c, _, al = _rbj(sample_rate, central_freq, Q)
    return _row(1.0, -2 * c, 1.0, 1 + al, -2 * c, 1 - al)


def allpass_biquad(sample_rate: float, central_freq: float, Q: float = 0.707) -> np.ndarray:
    c, _, al = _rbj(sample_rate, central_freq, Q)
    return _row(1 - al, -2 * c, 1 + al, 1 + al, -2 * c, 1 - al)


def equalizer_biquad(sample_rate: float, center_freq: float, gain: float, Q: float = 0.707) -> np.ndarray:
    c, _, al = _rbj(sample_rate, center_freq, Q)
    A = math.exp(gain / 40.0 * math.log(10.0))
    return _row(1 + al * A, -2 * c, 1 - al * A, 1 + al / A, -2 * c, 1 - al / A)


def preemphasis_sos(coeff: float = 0.97) -> np.ndarray:
    """y[n] = x[n] - coeff x[n - 1]"""
    return np.array([1.0, -float(coeff), 0.0, 1.0, 0.0, 0.0])


def deemphasis_sos(coeff: float = 0.97) -> np.ndarray:
    """y[n] = x[n] + coeff y[n - 1], the inverse of `preemphasis_sos`"""
    return np.array([1.0, 0.0, 0.0, 1.0, -float(coeff), 0.0])


__all__ = ["IirPlan", "sosfilt", "sosfiltfilt", "sosfilt_zi", "biquad", "lowpass_biquad", "highpass_biquad", "bandpass_biquad",
           "bandreject_biquad", "allpass_biquad", "equalizer_biquad", "preemphasis_sos", "deemphasis_sos"]
