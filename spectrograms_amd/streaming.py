"""Streaming spectrogram plans over the sgx_stream_* C ABI: signals that arrive in blocks.

`StreamingPlan` takes the arguments of `Plan` and runs the same frames: `push(block)` hands `(B, C)` new samples to `B` rows that run
in lock step (any `C` per call) and returns the frames that became complete, `flush()` the ones the trailing padding completes.
After the flush the frames of all calls, laid end to end, are those of `Plan.compute_batch` on the whole signals: the same count in
the same order, equal to rounding (not bit for bit across different cuts: the frame count of a call decides the launch shape).  The
rows' pending samples stay on the device between calls; the first push after creation or `reset()` fixes `B`.

`StreamingInversePlan` (sgx_istream_*) is the synthesis half: frames in, the samples that no later frame can change out, the overlap
tail on the device.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _ffi
from .params import LogParams, MfccParams, SpectrogramParams, parse_dtype
from .planner import flatten_params


class StreamingPlan(_ffi.NativeHandle):
    """One sgx_stream (a plan's parameters + dtype + device + the rows' pending samples).  Not thread-safe, like `Plan`."""

    _prefix = "sgx_stream"

    def __init__(self, params: SpectrogramParams, amp: int, mel=None, db: Optional[LogParams] = None, dtype: Optional[str] = None,
                 device: int = _ffi.DEVICE_CURRENT, mfcc: Optional[MfccParams] = None):
        self._lib = _ffi.lib()
        self._dt = parse_dtype(dtype)
        self._complex = amp == _ffi.AMP_COMPLEX
        self._hop, self._sample_rate = params.stft.hop_size, params.sample_rate
        p, cw, _ = flatten_params(params, amp, mel, db, mfcc)  # (cw: the custom window stays alive across the create call)
        p.dtype, p.device = self._dt, int(device)
        ptr = C.c_void_p()
        self._create(self._lib.sgx_stream_create(C.byref(p), C.byref(ptr)), ptr)
        self._rows = 0          # fixed by the first push; reset() frees it
        self._squeeze = False   # the pushes are 1-D: the frames come back without the batch axis
        self._torch = None      # the device of the last pushed tensor (None: NumPy pushes)

    pending = property(lambda self: int(self._lib.sgx_stream_pending(self._h)), doc="virtual samples held back per row")
    frames_emitted = property(lambda self: int(self._lib.sgx_stream_frames_emitted(self._h)), doc="frames since creation / reset / flush")
    n_bins = property(lambda self: int(self._lib.sgx_stream_n_bins(self._h)))
    kernel_name = property(lambda self: self._lib.sgx_stream_kernel_name(self._h).decode(), doc="kernel_name of the plan that runs the frames")
    allocations = property(lambda self: int(self._lib.sgx_stream_allocations(self._h)),
                           doc="how often the stream has allocated or replaced one of its own buffers (it stands still within what reserve() sized)")
    is_complex = property(lambda self: self._complex)

    def frames(self, n_samples: int) -> int:
        """Frames a push of `n_samples` samples per row would return now."""
        f, after = C.c_size_t(), C.c_size_t()
        self._check(self._lib.sgx_stream_step(self._h, self.pending, int(n_samples), C.byref(f), C.byref(after)))
        return f.value

    def flush_frames(self) -> int:
        """Frames `flush()` would return now."""
        f = C.c_size_t()
        self._check(self._lib.sgx_stream_flush_frames(self._h, C.byref(f)))
        return f.value

    def times(self, f: int) -> np.ndarray:
        """Time axis (seconds) of the next `f` frames: (frames_emitted + i) hop / sample_rate, as the offline plan counts them."""
        return (self.frames_emitted + np.arange(int(f))) * (self._hop / self._sample_rate)

    def reset(self) -> None:
        """Drop the pending samples; the row count of the next push is free again."""
        self._check(self._lib.sgx_stream_reset(self._h, None))
        self._rows, self._squeeze, self._torch = 0, False, None

    def reserve(self, batch: int, max_block: int, host_staging: bool = True) -> None:
        """Pre-size the stream's buffers so that pushes of up to `max_block` samples on `batch` rows, and the flush, do not allocate.
        Call it on a stream without pending samples of earlier pushes (after creation, reset or flush)."""
        self._check(self._lib.sgx_stream_reserve(self._h, int(batch), int(max_block), int(host_staging)))

    # ---- calls ------------------------------------------------------------------------------------------------------------
    def _out_types(self):
        """(numpy, torch) dtype of the frames: complex for a complex plan."""
        return (self._cdt, self._tcdt) if self._complex else (self._np, self._tdt)

    def _elems(self, shape) -> int:
        return int(np.prod(shape)) * (2 if self._complex else 1)

    def push(self, block, out=None, stream: int = 0):
        """(C,) or (B, C) new samples -> the frames that became complete, (n_bins, f) or (B, n_bins, f) (complex for a complex plan;
        f may be 0).  NumPy in -> NumPy out (stream-owned staging, synchronous); a torch tensor on the plan's device -> a tensor
        there, asynchronous on `stream` / torch's current stream.  `out`, if given, has the shape and dtype of the return value."""
        if type(block).__module__.startswith("torch"):
            return self._push_torch(block, out, stream)
        xb, sq = self._host_rows(block, "block (n,)")
        b, c = xb.shape
        shape = (b, self.n_bins, self.frames(c))
        res = self._out_array(out.reshape(shape) if out is not None and sq and out.ndim == 2 else out, shape, self._out_types()[0])
        self._check(self._lib.sgx_stream_push(self._h, xb.ctypes.data, b, c, c, res.ctypes.data if res.size else None,
                                              self._elems(shape), _ffi.MEM_HOST, None))
        self._rows, self._squeeze, self._torch = b, sq, None
        return res[0] if sq else res

    def _push_torch(self, x, out, stream):
        if x.dim() not in (1, 2):
            raise ValueError("block must be 1-D (n,) or 2-D (batch, n)")
        sq = x.dim() == 1
        xb = x[None] if sq else x
        stride = self._check_tensor(xb, "block", 2, rows_may_stride=True)
        b, c = xb.shape
        shape = (b, self.n_bins, self.frames(c))
        res = self._out_tensor(out.reshape(shape) if out is not None and sq and out.dim() == 2 else out, shape, xb.device, self._out_types()[1])
        self._check(self._lib.sgx_stream_push(self._h, xb.data_ptr(), b, c, stride, res.data_ptr() if res.numel() else None,
                                              self._elems(shape), _ffi.MEM_DEVICE, self._stream(stream)))
        self._rows, self._squeeze, self._torch = b, sq, xb.device
        return res[0] if sq else res

    def flush(self, out=None, stream: int = 0):
        """The frames the trailing padding completes, shaped as `push` returns them for the fixed batch (as a tensor on `stream` /
        the current stream if the last push took one); the stream then starts over with the same row count."""
        shape = (max(self._rows, 1), self.n_bins, self.flush_frames())
        sq = self._squeeze or self._rows == 0
        if self._torch is not None:
            res = self._out_tensor(out.reshape(shape) if out is not None and sq and out.dim() == 2 else out, shape, self._torch, self._out_types()[1])
            args = (res.data_ptr() if res.numel() else None, self._elems(shape), _ffi.MEM_DEVICE, self._stream(stream))
        else:
            res = self._out_array(out.reshape(shape) if out is not None and sq and out.ndim == 2 else out, shape, self._out_types()[0])
            args = (res.ctypes.data if res.size else None, self._elems(shape), _ffi.MEM_HOST, None)
        self._check(self._lib.sgx_stream_flush(self._h, *args))
        return res[0] if sq else res


class StreamingInversePlan(_ffi.NativeHandle):
    """One sgx_istream: the inverse STFT of `params` (n_fft / hop / window / centre) for frames that arrive in runs.  `push(frames)`
    hands `(B, n_bins, f)` new frames to `B` rows that run in lock step (any `f >= 1` per call) and returns the samples no later frame
    can change, `flush()` the rest.  After the flush the samples of all calls, laid end to end, are those of `Plan.istft_batch` on all
    frames at once: `istft_length(F)` samples in the same order, equal to rounding (not bit for bit).  The unfinished overlap tail stays
    on the device between calls; the first push after creation or `reset()` fixes `B`.  Not thread-safe, like `Plan`."""

    _prefix = "sgx_istream"

    def __init__(self, params: SpectrogramParams, dtype: Optional[str] = None, device: int = _ffi.DEVICE_CURRENT):
        self._lib = _ffi.lib()
        self._dt = parse_dtype(dtype)
        self._n_bins = params.stft.n_fft // 2 + 1
        p, cw, _ = flatten_params(params, _ffi.AMP_COMPLEX, None, None, None)  # (cw: the custom window stays alive across the create call)
        p.dtype, p.device = self._dt, int(device)
        ptr = C.c_void_p()
        self._create(self._lib.sgx_istream_create(C.byref(p), C.byref(ptr)), ptr)
        self._rows = 0          # fixed by the first push; reset() frees it
        self._squeeze = False   # the pushes are 2-D: the samples come back without the batch axis
        self._torch = None      # the device of the last pushed tensor (None: NumPy pushes)

    frames_taken = property(lambda self: int(self._lib.sgx_istream_frames_taken(self._h)), doc="frames since creation / reset / flush")
    samples_emitted = property(lambda self: int(self._lib.sgx_istream_samples_emitted(self._h)), doc="samples returned per row since creation / reset / flush")
    pending = property(lambda self: int(self._lib.sgx_istream_pending(self._h)), doc="samples carried per row (at most n_fft)")
    n_bins = property(lambda self: self._n_bins)
    kernel_name = property(lambda self: self._lib.sgx_istream_kernel_name(self._h).decode(),
                           doc='the rows\' route of the last call + "+stream_ola"; "" before any call')
    allocations = property(lambda self: int(self._lib.sgx_istream_allocations(self._h)),
                           doc="how often the stream has allocated or replaced one of its own buffers (it stands still within what reserve() sized)")

    def samples(self, f: int) -> int:
        """Samples per row a push of `f >= 1` frames would return now."""
        if int(f) < 1:
            raise ValueError("f must be >= 1")
        m = C.c_size_t()
        self._check(self._lib.sgx_istream_step(self._h, self.frames_taken, int(f), C.byref(m)))
        return m.value

    def flush_samples(self) -> int:
        """Samples per row `flush()` would return now."""
        m = C.c_size_t()
        self._check(self._lib.sgx_istream_flush_samples(self._h, C.byref(m)))
        return m.value

    def reset(self) -> None:
        """Drop the carried tail; the row count of the next push is free again."""
        self._check(self._lib.sgx_istream_reset(self._h, None))
        self._rows, self._squeeze, self._torch = 0, False, None

    def reserve(self, batch: int, max_frames: int, host_staging: bool = True) -> None:
        """Pre-size the stream's buffers so that pushes of up to `max_frames` frames on `batch` rows, and the flush, do not allocate.
        Call it on a stream that carries nothing (after creation, reset or flush)."""
        self._check(self._lib.sgx_istream_reserve(self._h, int(batch), int(max_frames), int(host_staging)))

    # ---- calls ------------------------------------------------------------------------------------------------------------
    def push(self, frames, out=None, stream: int = 0):
        """(n_bins, f) or (B, n_bins, f) new complex frames -> the samples that became final, (m,) or (B, m) (m may be 0).  NumPy in ->
        NumPy out (stream-owned staging, synchronous); a torch tensor on the plan's device -> a tensor there, asynchronous on `stream`
        / torch's current stream; it may be a slice `S[:, :, a:b]` of a resident spectrogram (unit inner stride, the bin stride is
        taken from the tensor).  `out`, if given, has the shape and dtype of the return value."""
        if type(frames).__module__.startswith("torch"):
            return self._push_torch(frames, out, stream)
        xb, sq = self._host_rows(frames, "frames (n_bins, f)", (2, 3), self._cdt)
        b, nb, f = xb.shape
        shape = (b, self.samples(f) if f and nb == self._n_bins else 0)
        res = self._out_array(out.reshape(shape) if out is not None and sq and out.ndim == 1 else out, shape)
        self._check(self._lib.sgx_istream_push(self._h, xb.ctypes.data, b, nb, f, f, res.ctypes.data if res.size else None, res.size,
                                               _ffi.MEM_HOST, None))
        self._rows, self._squeeze, self._torch = b, sq, None
        return res[0] if sq else res

    def _push_torch(self, x, out, stream):
        if x.dim() not in (2, 3):
            raise ValueError("frames must be 2-D (n_bins, f) or 3-D (batch, n_bins, f)")
        sq = x.dim() == 2
        xb = x[None] if sq else x
        bin_stride = self._check_tensor(xb, "frames", 3, rows_may_stride=True, dtype=self._tcdt)
        b, nb, f = xb.shape
        shape = (b, self.samples(f) if f and nb == self._n_bins else 0)
        res = self._out_tensor(out.reshape(shape) if out is not None and sq and out.dim() == 1 else out, shape, xb.device)
        self._check(self._lib.sgx_istream_push(self._h, xb.data_ptr(), b, nb, f, bin_stride, res.data_ptr() if res.numel() else None,
                                               res.numel(), _ffi.MEM_DEVICE, self._stream(stream)))
        self._rows, self._squeeze, self._torch = b, sq, xb.device
        return res[0] if sq else res

    def flush(self, out=None, stream: int = 0):
        """The samples that were waiting for later frames, shaped as `push` returns them for the fixed batch (as a tensor on `stream` /
        the current stream if the last push took one); the stream then starts over with the same row count."""
        shape = (max(self._rows, 1), self.flush_samples())
        sq = self._squeeze or self._rows == 0
        if self._torch is not None:
            res = self._out_tensor(out.reshape(shape) if out is not None and sq and out.dim() == 1 else out, shape, self._torch)
            args = (res.data_ptr() if res.numel() else None, res.numel(), _ffi.MEM_DEVICE, self._stream(stream))
        else:
            res = self._out_array(out.reshape(shape) if out is not None and sq and out.ndim == 1 else out, shape)
            args = (res.ctypes.data if res.size else None, res.size, _ffi.MEM_HOST, None)
        self._check(self._lib.sgx_istream_flush(self._h, *args))
        return res[0] if sq else res


__all__ = ["StreamingPlan", "StreamingInversePlan"]
