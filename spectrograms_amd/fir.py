"""FIR filtering and deconvolution (src/convolution.rs) over the sgx_fir_* / sgx_deconv_* C ABI, batched.

`fft_convolve`, `fft_deconvolve` and `OverlapSaveConvolver` keep the reference's names and signatures (default dtype float64);
`FirPlan` adds batched calls ((batch, n) rows in one launch, one impulse response for all rows or one per row), streaming calls of any
length, device-resident torch entry points, and the route the plan runs (`kernel_name`).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _ffi
from .params import parse_dtype

_ROUTES = {"auto": _ffi.FIR_ROUTE_AUTO, "generic": _ffi.FIR_ROUTE_GENERIC}


class FirPlan(_ffi.NativeHandle):
    """One sgx_fir (impulse responses + dtype + device + route).  Not thread-safe, like the reference's `&mut self` convolver.

    `ir` is (taps,) — one response for every row — or (rows, taps) — one per row of every call.  `process` is the streaming form
    (n samples in, n out, the last taps - 1 samples kept as the rows' history), `convolve` the full one (n + taps - 1 out, no state).
    """

    _prefix = "sgx_fir"

    def __init__(self, ir, block_size: Optional[int] = None, dtype: Optional[str] = None, device: int = _ffi.DEVICE_CURRENT,
                 route: str = "auto"):
        self._lib = _ffi.lib()
        self._dt = parse_dtype(dtype)
        if route not in _ROUTES:
            raise ValueError(f"route must be 'auto' or 'generic', got {route!r}")
        if block_size is not None and int(block_size) <= 0:
            raise ValueError("block_size must be > 0")  # NonZeroUsize
        h = np.ascontiguousarray(ir, dtype=np.float64)
        if h.ndim not in (1, 2):
            raise ValueError("ir must be 1-D (taps,) or 2-D (rows, taps)")
        rows, taps = (1, h.shape[0]) if h.ndim == 1 else h.shape
        if h.ndim == 2 and rows == 0:
            raise ValueError("ir must have at least one row")
        self._block = None if block_size is None else int(block_size)
        ptr = C.c_void_p()
        st = self._lib.sgx_fir_create(h.ctypes.data_as(C.POINTER(C.c_double)) if h.size else None, taps, rows, self._block or 0,
                                      _ROUTES[route], self._dt, int(device), C.byref(ptr))
        self._create(st, ptr)

    taps = property(lambda self: int(self._lib.sgx_fir_taps(self._h)))
    fft_size = property(lambda self: int(self._lib.sgx_fir_fft_size(self._h)), doc="the plan's segment length P")
    step = property(lambda self: int(self._lib.sgx_fir_step(self._h)), doc="S = P - (taps - 1): output samples per segment")
    block_size = property(lambda self: self._block, doc="the caller's block hint (None: none given)")
    kernel_name = property(lambda self: self._lib.sgx_fir_kernel_name(self._h).decode())

    def reset(self) -> None:
        """Zero history, and the row count of the next streaming call is free again."""
        self._check(self._lib.sgx_fir_reset(self._h, self._stream()))

    def reserve(self, batch: int, n_samples: int, host_staging: bool = True) -> None:
        """Pre-size the history and the plan-owned scratch so that calls of up to `batch` rows of `n_samples` samples do not allocate."""
        self._check(self._lib.sgx_fir_reserve(self._h, int(batch), int(n_samples), int(host_staging)))

    # ---- host arrays ------------------------------------------------------------------------------------------------------
    def _host(self, x, fn, extra):
        xb, squeezed = self._host_rows(x, "samples (n,)")
        out = np.empty((xb.shape[0], xb.shape[1] + extra), self._np)
        self._check(fn(self._h, xb.ctypes.data, xb.shape[0], xb.shape[1], xb.shape[1], out.ctypes.data, out.size, _ffi.MEM_HOST, None))
        return out[0] if squeezed else out

    def process(self, x) -> np.ndarray:
        """Streaming: (n,) or (batch, n) -> the same shape; the rows' history moves on."""
        return self._host(x, self._lib.sgx_fir_process, 0)

    def convolve(self, x) -> np.ndarray:
        """Full: (n,) or (batch, n) -> (..., n + taps - 1) from zero history; the plan's history is not touched."""
        return self._host(x, self._lib.sgx_fir_convolve, self.taps - 1)

    # ---- device tensors (torch), on the current stream --------------------------------------------------------------------
    def _torch(self, x, out, fn, full):
        self._check_tensor(x, "samples", 2)
        b, n = x.shape
        out = self._out_tensor(out, (b, n + self.taps - 1 if full else n), x.device)
        self._check(fn(self._h, x.data_ptr(), b, n, n, out.data_ptr(), out.numel(), _ffi.MEM_DEVICE, self._stream()))
        return out

    def process_torch(self, x, out=None):
        """(batch, n) device tensor -> (batch, n), asynchronous on the current stream.  `out` must not overlap `x`."""
        return self._torch(x, out, self._lib.sgx_fir_process, False)

    def convolve_torch(self, x, out=None):
        """(batch, n) device tensor -> (batch, n + taps - 1), asynchronous on the current stream."""
        return self._torch(x, out, self._lib.sgx_fir_convolve, True)


class OverlapSaveConvolver(FirPlan):
    """OverlapSaveConvolver::new(ir, block) (src/convolution.rs:149-270): fixed blocks, one row.  `fft_size` is the plan's own segment
    length, not the reference's next_power_of_two(block + taps - 1); the samples do not depend on it."""

    def __init__(self, ir, block: int, dtype: Optional[str] = None):
        h = np.asarray(ir, dtype=np.float64)
        if h.ndim != 1:
            raise ValueError("ir must be 1-D")
        super().__init__(h, block_size=block, dtype=dtype)

    def process_block(self, input) -> np.ndarray:  # noqa: A002 (the reference's argument name)
        a = np.asarray(input)
        if a.ndim != 1 or a.shape[0] != self._block:  # :228-235 (the output is allocated here: its length is the block's)
            got = a.shape[0] if a.ndim == 1 else a.size
            raise _ffi.InvalidInputError(f"Invalid input: process_block expects input and output of length {self._block} (got {got} and {self._block})")
        return self.process(a)


class DeconvPlan(_ffi.NativeHandle):
    """One sgx_deconv (lengths + regularization + dtype + device)."""

    _prefix = "sgx_deconv"

    def __init__(self, n_len: int, d_len: int, regularization: float = 0.0, dtype: Optional[str] = None,
                 device: int = _ffi.DEVICE_CURRENT):
        self._lib = _ffi.lib()
        self._dt = parse_dtype(dtype)
        self.n_len, self.d_len = int(n_len), int(d_len)
        ptr = C.c_void_p()
        st = self._lib.sgx_deconv_create(self.n_len, self.d_len, float(regularization), self._dt, int(device), C.byref(ptr))
        self._create(st, ptr)

    output_length = property(lambda self: int(self._lib.sgx_deconv_output_length(self._h)))

    def reserve(self, batch: int, den_rows: int = 1, host_staging: bool = True) -> None:
        self._check(self._lib.sgx_deconv_reserve(self._h, int(batch), int(den_rows), int(host_staging)))

    def execute(self, numerator, denominator) -> np.ndarray:
        """numerator (n_len,) or (batch, n_len); denominator (d_len,) or (batch, d_len) -> (..., output_length)."""
        nshape, dshape = np.shape(numerator), np.shape(denominator)
        if len(nshape) in (1, 2) and len(dshape) in (1, 2) and (nshape[-1], dshape[-1]) != (self.n_len, self.d_len):
            raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {(self.n_len, self.d_len)}, got {(nshape[-1], dshape[-1])}")
        nb, squeezed = self._host_rows(numerator, "numerator (n,)")
        if len(dshape) == 2 and dshape[0] != nb.shape[0]:
            raise _ffi.DimensionMismatchError(f"Dimension mismatch: expected {nb.shape[0]}, got {dshape[0]}", nb.shape[0], dshape[0])
        db, _ = self._host_rows(denominator, "denominator (n,)")
        out = np.empty((nb.shape[0], self.output_length), self._np)
        self._check(self._lib.sgx_deconv_execute(self._h, nb.ctypes.data, db.ctypes.data, nb.shape[0], db.shape[0], out.ctypes.data,
                                                 out.size, _ffi.MEM_HOST, None))
        return out[0] if squeezed else out

    def execute_torch(self, numerator, denominator, out=None):
        """(batch, n_len) and (1 or batch, d_len) device tensors -> (batch, output_length), asynchronous on the current stream."""
        for t, what, w in ((numerator, "numerator", self.n_len), (denominator, "denominator", self.d_len)):
            self._check_tensor(t, what, 2)
            if t.shape[1] != w:
                raise ValueError(f"{what} must be a contiguous (rows, {w}) tensor of the plan's dtype")
        b = numerator.shape[0]
        out = self._out_tensor(out, (b, self.output_length), numerator.device)
        self._check(self._lib.sgx_deconv_execute(self._h, numerator.data_ptr(), denominator.data_ptr(), b, denominator.shape[0],
                                                 out.data_ptr(), out.numel(), _ffi.MEM_DEVICE, self._stream()))
        return out


def fft_convolve(a, b, dtype: Optional[str] = None) -> np.ndarray:
    """fft_convolve (src/convolution.rs:25-47): the full linear convolution, length a + b - 1.  `a` is (n,) or (batch, n), `b` (m,) or
    (batch, m); two 1-D operands take the shorter one as the impulse response."""
    np_dt = _ffi.np_dtype(parse_dtype(dtype))
    x, h = np.asarray(a, dtype=np_dt), np.asarray(b, dtype=np_dt)
    if x.ndim == 1 and h.ndim == 1 and x.shape[0] < h.shape[0]:
        x, h = h, x
    if h.ndim == 2 and x.ndim == 1:
        raise ValueError("a must be (batch, n) when b is (batch, m)")
    if x.shape[-1] == 0 or h.shape[-1] == 0:
        raise _ffi.InvalidInputError("Invalid input: inputs must not be empty")  # NonEmptySlice
    return FirPlan(h, dtype=dtype).convolve(x)


def fft_deconvolve(numerator, denominator, regularization: float = 0.0, dtype: Optional[str] = None) -> np.ndarray:
    """fft_deconvolve (src/convolution.rs:60-106): N conj(D) / (|D|^2 + regularization max |D|^2), inverse-transformed and truncated."""
    num, den = np.asarray(numerator), np.asarray(denominator)
    if num.ndim not in (1, 2) or den.ndim not in (1, 2) or (den.ndim == 2 and num.ndim == 1):
        raise ValueError("numerator must be (n,) or (batch, n), denominator (m,) or (batch, m)")
    if num.shape[-1] == 0 or den.shape[-1] == 0:
        raise _ffi.InvalidInputError("Invalid input: inputs must not be empty")
    return DeconvPlan(num.shape[-1], den.shape[-1], regularization, dtype).execute(num, den)


__all__ = ["FirPlan", "OverlapSaveConvolver", "DeconvPlan", "fft_convolve", "fft_deconvolve"]
