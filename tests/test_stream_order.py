"""The contract around the 1-D device paths: stream order, `reserve`, and independence from the calls before.

Every batched 1-D entry point takes a `hip_stream` (named `stream` in the younger families); include/spectro_hip.h promises that a
device-pointer call is asynchronous on that stream, that a call which fits what `reserve` sized allocates nothing, and (single-caller
rule) that a plan can be reused call after call.  CASES holds one row per launch-chain shape of each entry point; every row asserts its
route names.  The families: the forward plans (sgx_execute), the inverse STFT (sgx_istft), MDCT, binaural maps and histograms,
gammatone, Welch (sgx_welch_execute: the fused kernel and its fold, the generic route's memset and chunk loop), Kaldi features
(sgx_kaldi_execute: the fused kernel, the generic chunk loop, the mean subtraction in place), the stateless resampler
(sgx_resample_resample), and the state-carrying ones — streaming spectrograms (sgx_stream_push / _flush), the streaming inverse
(sgx_istream_push / _flush) and the streaming resampler (sgx_resample_reset / _process / _flush) — as composite rows: one `call` is a
fixed schedule of calls on one plan that starts from and returns to the state after reset / flush, so that "a fresh plan's eager
result, bit for bit" stays the criterion.  FIR, deconvolution and minimum phase keep stream tests and a census of their own
(tests/test_fir.py, tests/test_minphase.py); the census here checks that they do.

  A  one operation of the caller's stream.  On a warm plan (one earlier call of the same size on OTHER data, so that every scratch
     buffer holds stale values), with NaN inputs and a sentinel output, a side stream gets: a producer of >= 10 ms whose last
     operation writes the samples, the call, a clone of the output, a sentinel fill.  Nothing synchronises in between.  The clone must
     equal a fresh plan's eager result bit for bit, the output must be the sentinel everywhere, and the producer must still be running
     when the host returns from the call (the hazard window existed; a case that cannot show it fails).
  B  a reserved call allocates nothing: on a fresh plan, after `reserve`, the call is captured into a graph (a linear chain on the
     side stream) and replayed on further inputs; an allocation, a synchronisation or a host copy breaks the capture, a launch on
     another stream is missing from the graph.
  C  a call does not depend on the calls before it: sizes up and down, host and device calls and both directions interleaved, a
     failed call in the middle, `reserve` after calls.  Every result and every route name equals a fresh plan's.

Everything here is bit equality (the kernels' only atomics are integer ones); each row's eager result is checked once against the f64
reference with the checker of the file that owns the route (tests/test_gpu_parity.py `check` for the forward plans — the bigfft rows
with tests/test_bigfft.py's bounds, MFCC and chroma with the expressions of tests/test_mfcc.py / tests/test_chroma.py —,
tests/test_istft_precision.py's per-sample bound, and the bound functions of test_mdct / test_binaural / test_gammatone / test_cqt;
tests/test_welch.py's `reference` and `ratio`, tests/kaldi_ref.py's, tests/test_resample.py's `check_bound`, and for the composite rows
the whole-signal checks of tests/test_streaming.py (`compare`), tests/test_streaming_inverse.py (`check_bound`) and
tests/test_resample.py on the slices laid end to end).
"""
import ctypes as C
import math
import os
import re
import time

import numpy as np
import pytest

import spectrograms_amd as sg
from oracle import oracle as orc
from spectrograms_amd import _ffi
from spectrograms_amd.binaural import BinauralPlan
from tests import helpers as H
from tests import test_binaural as TB
from tests import test_cqt as TC
from tests import test_gammatone as TG
from tests import test_gpu_parity as TP
from tests import test_istft_precision as TI
from tests import test_kaldi as TK
from tests import test_mdct as TM
from tests import test_resample as TR
from tests import test_streaming as TS
from tests import test_streaming_inverse as TSI
from tests import test_welch as TW
from tests import kaldi_ref as KR

SR = 16000.0
NP = {"float32": np.float32, "float64": np.float64}
CNP = {"float32": np.complex64, "float64": np.complex128}
F32, F64 = "float32", "float64"
SENTINEL = -1.2345678e30  # finite in both types, far from anything a case computes
PRODUCER_MIN_MS = 10.0
PRODUCER_AIM_MS = 25.0
TIMES = {}  # row id -> (producer ms, host ms from the end of the producer's enqueue to the return of the last enqueue)


def _noise(batch, n, dtype, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = 0.3 * rng.standard_normal((batch, n)) + 0.4 * np.sin(2 * np.pi * 440.0 * (1.0 + 0.1 * np.arange(batch))[:, None] * t[None, :])
    return x.astype(np.float32).astype(NP[dtype])  # f32-valued in both types


# ---- rows ------------------------------------------------------------------------------------------------------------------------------
class Row:
    """One launch-chain shape of one entry point.  `size` counts frames (of the input for forward rows, of the spectrum / coefficient
    tensor for inverse rows); `gen` makes host inputs, `call` the device call into `out`, `host` the same call on host arrays."""
    entry = ""  # (a composite row names every entry point of its schedule: a tuple)
    has_stream_arg = False
    scratch = False
    counts_allocations = False  # the plan has an `allocations` counter that B holds still across capture and replays
    batch = 4
    tiny = 3

    @property
    def entries(self):
        return (self.entry,) if isinstance(self.entry, str) else tuple(self.entry)

    def names(self, plan):
        raise NotImplementedError

    def dev(self, ins):
        import torch
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ins)


class ForwardRow(Row):
    """Plan.compute_batch (sgx_execute).  kind: power | db | complex | mfcc | chroma | cqt_lds | cqt_global | big (bigfft bounds)."""
    entry = "sgx_execute"
    has_stream_arg = True

    def __init__(self, dtype, n_fft, hop, kind, n_mels, nf, expect, batch=4, scratch=False, tag=""):
        self.dtype, self.n_fft, self.hop, self.kind, self.n_mels, self.size, self.expect = dtype, n_fft, hop, kind, n_mels, nf, expect
        self.batch, self.scratch = batch, scratch
        self.rid = f"execute-{dtype[5:]}-{n_fft}-{hop}-{kind}{n_mels or ''}-{expect[0]}{'-' + tag if tag else ''}"

    def _cqt(self):
        return TC.SHAPES["musical_1024_256" if self.kind == "cqt_lds" else "lds_overflow"]

    def fresh(self):
        st = sg.StftParams(self.n_fft, self.hop, sg.WindowType.hanning, True)
        if self.kind == "mfcc":
            return sg.SpectrogramPlanner().mfcc_plan(st, SR, self.n_mels, sg.MfccParams(13), dtype=self.dtype)
        if self.kind == "chroma":
            return sg.SpectrogramPlanner().chroma_plan(st, SR, sg.ChromaParams(440.0, 32.7, 4186.0, sg.ChromaNorm.l2), dtype=self.dtype)
        if self.kind.startswith("cqt"):
            cq, n_fft, hop, sr, centre, _, _ = self._cqt()
            return TC.gpu_plan(cq, n_fft, hop, sr, _ffi.AMP_POWER, None, self.dtype, centre)
        amp = "power" if self.kind == "big" else self.kind
        return TP.make(self.n_fft, self.hop, n_mels=self.n_mels, amp=amp, floor=-80.0 if amp == "db" else None, dtype=self.dtype)[0]

    def n_samples(self, nf):
        return (nf - 1) * self.hop + 1  # nf centred frames

    def gen(self, batch, nf, seed):
        return (_noise(batch, self.n_samples(nf), self.dtype, seed),)

    def alloc(self, plan, ins):
        import torch
        b, n = ins[0].shape
        nb, nf = plan.output_shape(n)
        return torch.empty((b, nb, nf, 2) if plan.is_complex else (b, nb, nf), dtype=ins[0].dtype, device="cuda")

    def call(self, plan, ins, out, stream=0):
        plan.compute_batch(ins[0], out=out, stream=stream)

    def host(self, plan, ins):
        y = plan.compute_batch(ins[0])
        return np.ascontiguousarray(y).view(NP[self.dtype]).reshape(y.shape + (2,)) if plan.is_complex else y

    def reserve(self, plan, batch, nf):
        plan.reserve(batch, self.n_samples(nf), host_staging=False)

    def names(self, plan):
        return (plan.kernel_name, plan.bank_stage_name)

    def check64(self, plan, ins, got):
        x64 = ins[0].astype(np.float64)
        dt = self.dtype
        if self.kind == "mfcc":  # tests/test_mfcc.py::test_gpu_mfcc_matches_oracle
            p = orc.Params(n_fft=self.n_fft, hop=self.hop, n_mels=self.n_mels, f_min=0.0, f_max=SR / 2, amp="db", floor_db=-80.0)
            mp = sg.MfccParams(13)
            ref = np.stack([orc.mfcc(p, r, mp.n_mfcc, mp.include_c0, mp.lifter) for r in x64])
            assert got.shape == ref.shape
            assert np.max(np.abs(got - ref)) < (1e-7 if dt == F64 else 2e-2) * max(1.0, np.max(np.abs(ref)) / 100)
        elif self.kind == "chroma":  # tests/test_chroma.py::test_gpu_chromagram_matches_oracle
            ref = np.stack([orc.chromagram(orc.Params(n_fft=self.n_fft, hop=self.hop), r, norm="l2") for r in x64])
            assert got.shape == ref.shape
            assert np.max(np.abs(got - ref)) < (1e-10 if dt == F64 else 3e-5) * max(1.0, np.max(np.abs(ref)))
        elif self.kind.startswith("cqt"):
            cq, n_fft, hop, sr, centre, _, _ = self._cqt()
            TC.check_output(got, x64, cq, n_fft, hop, sr, dt, _ffi.AMP_POWER, None, centre)
        elif self.kind == "big":  # tests/test_bigfft.py::test_gpu_stft_and_back, the power output
            refp = orc.spectrogram_batch(orc.Params(n_fft=self.n_fft, hop=self.hop), x64)
            assert got.shape == refp.shape
            m, m40 = refp > 1e-6 * refp.max(), refp > 1e-4 * refp.max()
            assert np.max(np.abs(got[m40] - refp[m40]) / refp[m40]) < (1e-9 if dt == F64 else 1e-4)
            assert np.max(np.abs(got[m] - refp[m]) / refp[m]) < (1e-9 if dt == F64 else 5e-3)
        else:  # tests/test_gpu_parity.py::run_case
            amp = self.kind
            op = TP.make(self.n_fft, self.hop, n_mels=self.n_mels, amp=amp, floor=-80.0 if amp == "db" else None, dtype=dt)[1]
            if amp == "complex":
                g = np.ascontiguousarray(got).view(CNP[dt])[..., 0]
                TP.check(g, orc.stft_batch(op, x64), "complex", dt)
            else:
                pow64 = None
                if amp == "db":
                    pow64 = orc.spectrogram_batch(orc.Params(**{**op.__dict__, "amp": "power", "floor_db": None, "_keep": []}), x64)
                TP.check(got, orc.spectrogram_batch(op, x64), amp, dt, -80.0 if amp == "db" else None, pow64)


class CqtRow(ForwardRow):
    def __init__(self, dtype, which, expect):
        cq, n_fft, hop, sr, centre, n, b = TC.SHAPES[which]
        super().__init__(dtype, n_fft, hop, "cqt_lds" if expect == "cqt_mfma_lds" else "cqt_global", 0, n // hop + 1, (expect, ""), batch=b)
        self.n = n
        self.rid = f"execute-{dtype[5:]}-{expect}"

    def n_samples(self, nf):
        return (nf - 1) * self.hop + self.n % self.hop

    def gen(self, batch, nf, seed):
        x = TC.signals(batch, self.n_samples(nf), SR, seed)
        return (x.astype(np.float32).astype(NP[self.dtype]),)


class IstftRow(Row):
    """Plan.istft_batch (sgx_istft): one row of tests/test_istft_precision.py's ROUTES per route name and type."""
    entry = "sgx_istft"
    has_stream_arg = True
    tiny = 1

    def __init__(self, route):
        self.dtype, self.n_fft, self.hop, self.centre, self.window, name, self.paired = route
        self.expect = (name,)
        self.size = 41 if self.n_fft <= 2048 else 13 if self.n_fft <= 8200 else 7
        self.scratch = name.endswith("+ola")
        self.rid = f"istft-{TI._rid(route)}"

    def fresh(self):
        return TI.make_plan(self.dtype, self.n_fft, self.hop, self.centre, self.window)

    def gen(self, batch, nf, seed):
        rng = np.random.default_rng(seed)
        nb = self.n_fft // 2 + 1
        return (np.ascontiguousarray(np.stack([TI.rand_spec(rng, nb, nf, self.n_fft, np.ones(nf)) for _ in range(batch)]).astype(CNP[self.dtype])),)

    def alloc(self, plan, ins):
        import torch
        b, _, nf = ins[0].shape
        return torch.empty((b, plan.istft_length(nf)), dtype=getattr(torch, self.dtype), device="cuda")

    def call(self, plan, ins, out, stream=0):
        plan.istft_batch(ins[0], out=out, stream=stream)

    def host(self, plan, ins):
        return plan.istft_batch(ins[0])

    def reserve(self, plan, batch, nf):
        n = (nf - 1) * self.hop + (1 if self.centre else self.n_fft)  # signals whose STFT has nf frames (even and odd n_fft)
        assert plan.output_shape(n)[1] == nf
        plan.reserve(batch, n, host_staging=False, inverse=True)

    def names(self, plan):
        return (plan.istft_kernel_name,)

    def check64(self, plan, ins, got):
        TI._check_signals(plan, ins[0], got, self.dtype, self.n_fft, self.hop, self.expect[0], self.paired, self.rid)


class MdctRow(Row):
    scratch = True
    tiny = 1

    def __init__(self, dtype, ws, inverse, expect):
        self.dtype, self.ws, self.hop, self.inverse, self.expect, self.size = dtype, ws, ws // 2, inverse, (expect,), 9
        self.entry = "sgx_mdct_inverse" if inverse else "sgx_mdct_forward"
        self.rid = f"mdct-{dtype[5:]}-{ws}-{expect}"

    def fresh(self):
        return sg.MdctPlan(sg.MdctParams.sine_window(self.ws), self.dtype)

    def n_samples(self, nf):
        return self.ws + self.hop * (nf - 1) + self.hop // 2

    def gen(self, batch, nf, seed):
        rng = np.random.default_rng(seed)
        if self.inverse:
            return (rng.standard_normal((batch, self.ws // 2, nf)).astype(NP[self.dtype]),)
        return (TM._signal(rng, batch, self.n_samples(nf), self.dtype),)

    def alloc(self, plan, ins):
        import torch
        b = ins[0].shape[0]
        shape = (b, plan.inverse_length(ins[0].shape[2])) if self.inverse else (b,) + tuple(plan.output_shape(ins[0].shape[1]))
        return torch.empty(shape, dtype=ins[0].dtype, device="cuda")

    def call(self, plan, ins, out, stream=0):
        (plan.inverse_torch if self.inverse else plan.forward_torch)(ins[0], out=out)

    def host(self, plan, ins):
        return plan.inverse(ins[0]) if self.inverse else plan.forward(ins[0])

    def reserve(self, plan, batch, nf):
        plan.reserve(batch, self.n_samples(nf), host_staging=False)

    def names(self, plan):
        return (plan.kernel_name(self.inverse),)

    def check64(self, plan, ins, got):  # tests/test_mdct.py::_check_forward / _check_inverse, on the device call's result
        w, p = plan.window(), plan.params
        if self.inverse:
            ref = TM.ola(TM.ref_frames_inv(ins[0], p.n_coefficients, self.dtype), w, p.hop_size)
            assert got.shape == ref.shape
            ratio = np.abs(got.astype(np.float64) - ref).max() / TM.inv_bound(ins[0], w, p.window_size, p.hop_size, self.dtype)
        else:
            ref = TM.ref_forward(ins[0], w, p.window_size, p.hop_size, self.dtype)
            assert got.shape == ref.shape
            ratio = (np.abs(got.astype(np.float64) - ref).max(axis=1) / TM.fwd_bound(ins[0], w, p.window_size, p.hop_size, self.dtype)).max()
        assert ratio <= 1.0, (self.rid, ratio)


class BinauralRow(Row):
    """BinauralPlan.compute_torch (sgx_binaural_execute), the wrapped IPD map over the default band."""
    entry = "sgx_binaural_execute"

    def __init__(self, dtype, n_fft, hop, expect, scratch):
        self.dtype, self.n_fft, self.hop, self.expect, self.scratch, self.size = dtype, n_fft, hop, (expect,), scratch, 23
        self.rid = f"binaural-{dtype[5:]}-{n_fft}-{hop}-{expect.replace('/', '_')}"

    def fresh(self):
        return BinauralPlan(TB.bparams("ipd", self.n_fft, self.hop, None, wrapped=True), self.dtype)

    def n_samples(self, nf):
        return self.hop * (nf - 1)

    def gen(self, batch, nf, seed):
        return TB.stereo(self.dtype, batch, self.n_samples(nf), seed=seed)

    def alloc(self, plan, ins):
        import torch
        _, nb, nf = plan.output_shape(ins[0].shape[1])
        return torch.empty((ins[0].shape[0], nb, nf), dtype=ins[0].dtype, device="cuda")

    def call(self, plan, ins, out, stream=0):
        plan.compute_torch(ins[0], ins[1], out=out)

    def host(self, plan, ins):
        return plan.compute(ins[0], ins[1])

    def reserve(self, plan, batch, nf):
        plan.reserve(batch, self.n_samples(nf), host_staging=False)

    def names(self, plan):
        return (plan.kernel_name,)

    def check64(self, plan, ins, got):  # tests/test_binaural.py::test_gpu_parity_within_the_per_frame_bound, kind "ipd"
        L, R = (a.astype(np.float64) for a in ins)
        n_fft, hop, dt = self.n_fft, self.hop, self.dtype
        w, u = TB.window(n_fft, hop), TB.U[dt]
        sb, nb, _ = plan.output_shape(L.shape[1])
        name = TB.route_of(plan)
        XL = np.stack([H.np_stft(r, n_fft, hop, w) for r in L])[:, sb:sb + nb]
        XR = np.stack([H.np_stft(r, n_fft, hop, w) for r in R])[:, sb:sb + nb]
        d = TB.frame_deltas(L, w, n_fft, hop, dt, name)[:, None, :]
        dR = TB.frame_deltas(R, w, n_fft, hop, dt, name)[:, None, :]
        with np.errstate(all="ignore"):
            rl, rr = d / np.abs(XL), dR / np.abs(XR)
        t = TB.truth("ipd", XL, XR, np.arange(sb, sb + nb), SR / n_fft, wrapped=True)
        good = (rl <= 1e-2) & (rr <= 1e-2)
        assert good.mean() >= 0.9
        err = TB.circ(got.astype(np.float64) - t, 2 * math.pi)
        bound = 1.01 * (rl + rr) + 16 * u * math.pi
        assert not (good & ~(err <= bound)).any(), float(np.max(np.where(good, err / bound, 0)))


class HistogramRow(Row):
    """sgx_binaural_histogram on device pointers (the Python wrapper only takes host arrays: the C entry point is called directly)."""
    entry = "sgx_binaural_histogram"
    NBINS = 37

    def __init__(self, dtype):
        self.dtype, self.size, self.expect = dtype, 23, ("r32x16_binaural_f32" if dtype == F32 else "binaural_epilogue/d32x16_f64",)
        self.rid = f"binaural-histogram-{dtype[5:]}"

    def fresh(self):
        return BinauralPlan(TB.bparams("ipd", 1024, 256, None, wrapped=True), self.dtype)

    def gen(self, batch, nf, seed):
        rng = np.random.default_rng(seed)
        nb = self.fresh().output_shape(1024)[1]
        v = rng.uniform(-1.1 * math.pi, 1.1 * math.pi, (batch, nb, nf))
        v[:, 0, 0] = np.nan
        return (v.astype(NP[self.dtype]),)

    def alloc(self, plan, ins):
        import torch
        return torch.empty((ins[0].shape[0], self.NBINS, ins[0].shape[2]), dtype=torch.float64, device="cuda")

    def call(self, plan, ins, out, stream=0):
        import torch
        v = ins[0]
        s = torch.cuda.current_stream().cuda_stream
        st = _ffi.lib().sgx_binaural_histogram(plan._h, v.data_ptr(), v.shape[0], v.shape[2], self.NBINS, -math.pi, math.pi, 1, 1,
                                               out.data_ptr(), out.numel(), _ffi.MEM_DEVICE, C.c_void_p(s))
        assert st == 0, plan._lib.sgx_binaural_last_error(plan._h)

    def host(self, plan, ins):
        return plan.histogram(ins[0], self.NBINS, -math.pi, math.pi, 1, True)

    def reserve(self, plan, batch, nf):
        plan.reserve(batch, 256 * (nf - 1), host_staging=False)

    def names(self, plan):
        return (plan.kernel_name,)

    def check64(self, plan, ins, got):  # tests/test_binaural.py::test_gpu_histograms
        for b in range(ins[0].shape[0]):
            ref = TB.hist_truth(ins[0][b], self.NBINS, -math.pi, math.pi, 1, True)
            assert np.all(np.abs(got[b] - ref) <= 4 * 2.0 ** -52 * self.NBINS * np.abs(ref))


class GammatoneRow(Row):
    entry = "sgx_gammatone_execute"
    scratch = True
    CASE = "bands_65"
    tiny = 1

    def __init__(self, dtype):
        self.dtype, self.expect = dtype, ("k_gammatone_iir",)
        self.sr, self.frame, self.hop, self.erb, self.batch, self.size = TG.CASES[self.CASE]
        self.rid = f"gammatone-{dtype[5:]}-{self.CASE}"

    def fresh(self):
        return sg.GammatonePlan(self.sr, self.frame, self.hop, self.erb, self.dtype)

    def n_samples(self, nf):
        return self.frame + self.hop * (nf - 1) + (self.hop - 1) // 2

    def gen(self, batch, nf, seed):
        if (batch, nf, seed) == (self.batch, self.size, 1):  # the owning file's input, which its cached long-double reference belongs to
            return (TG.case_input(self.CASE).astype(NP[self.dtype]),)
        return ((0.25 * np.random.default_rng(seed).standard_normal((batch, self.n_samples(nf)))).astype(np.float32).astype(NP[self.dtype]),)

    def alloc(self, plan, ins):
        import torch
        nb, nf = plan.output_shape(ins[0].shape[1])
        return torch.empty((ins[0].shape[0], nb, nf), dtype=ins[0].dtype, device="cuda")

    def call(self, plan, ins, out, stream=0):
        plan.compute_torch(ins[0], out=out)

    def host(self, plan, ins):
        return plan.compute(ins[0])

    def reserve(self, plan, batch, nf):
        plan.reserve(batch, self.n_samples(nf), host_staging=False)

    def names(self, plan):
        return (plan.kernel_name,)

    def check64(self, plan, ins, got):  # tests/test_gammatone.py::test_kernel_every_element
        ld, _ = TG.case_reference(self.CASE)
        bound = TG.rel_bound(self.CASE, self.dtype)[None, :, None]
        err = (np.abs(got.astype(TG.LD) - ld) / np.where(ld > 0, ld, TG.LD(1))).astype(np.float64)
        assert np.all(np.isfinite(got)) and np.max(err / bound) <= 1.0 and np.all(got[ld == 0] == 0)


def _status(plan, st):
    assert st == 0, plan._last_error(plan._h)


class WelchRow(Row):
    """WelchPlan.compute_torch (sgx_welch_execute); size counts segments, hop = n / 4.  The wrapper has no `stream=`: the
    explicit-stream call goes to the C entry point.  `chunk`: max_scratch_bytes as that many segments of the generic route."""
    entry = "sgx_welch_execute"
    has_stream_arg = True
    counts_allocations = True
    tiny = 1
    FS, DETREND, SCALING = 16000.0, "constant", "density"

    def __init__(self, dtype, n, kind, expect, scratch=False, chunk=0, tag=""):
        self.dtype, self.n, self.hop, self.kind, self.expect, self.scratch, self.size = dtype, n, n // 4, kind, (expect,), scratch, 41
        # one segment of the generic route, as tests/test_welch.py::test_generic_chunk_seam_inside_a_row states it for a PSD plan:
        # max(n, 2 (n / 2 + 1)) elements per buffer, once per channel
        per = (1 if kind == "psd" else 2) * max(n, 2 * (n // 2 + 1)) * np.dtype(NP[dtype]).itemsize
        self.max_scratch = chunk * per if chunk else None
        self.rid = f"welch-{dtype[5:]}-{n}-{kind}-{expect}{'-' + tag if tag else ''}"

    def fresh(self, device=None):
        wp = sg.WelchParams(self.n, self.hop, sg.WindowType.hanning, self.FS, self.DETREND, self.SCALING)
        return sg.WelchPlan(wp, self.kind, self.dtype, device=device, max_scratch_bytes=self.max_scratch)

    def n_samples(self, nf):
        return self.n + (nf - 1) * self.hop + 5  # a tail that fills no segment

    def gen(self, batch, nf, seed):
        x, y = TW.signals("noise", batch, self.n_samples(nf), self.dtype, seed)
        return (x,) if self.kind == "psd" else (x, y)

    def alloc(self, plan, ins):
        import torch
        dt = (torch.complex64 if self.dtype == F32 else torch.complex128) if self.kind == "csd" else ins[0].dtype
        return torch.empty((ins[0].shape[0], plan.n_bins), dtype=dt, device="cuda")

    def call(self, plan, ins, out, stream=0):
        x, y = ins[0], (ins[1] if len(ins) > 1 else None)
        if not stream:
            plan.compute_torch(x, y, out=out)
            return
        b, n = x.shape
        _status(plan, _ffi.lib().sgx_welch_execute(plan._h, x.data_ptr(), None if y is None else y.data_ptr(), b, n, n, out.data_ptr(),
                                                   out.numel() * (2 if self.kind == "csd" else 1), _ffi.MEM_DEVICE, C.c_void_p(stream)))

    def host(self, plan, ins):
        return plan.compute(*ins)

    def reserve(self, plan, batch, nf):
        plan.reserve(batch, self.n_samples(nf), host_staging=False)

    def names(self, plan):
        return (plan.kernel_name,)

    def reference(self, ins):
        """tests/test_welch.py's (reference, bound); the coherence bound's range condition is asserted inside."""
        x, y = ins[0], (ins[1] if len(ins) > 1 else None)
        w = self.fresh(device=_ffi.DEVICE_HOST_ONLY).window()
        return TW.reference(self.kind, x, y, w, self.n, self.hop, self.DETREND, self.SCALING, self.FS, self.dtype)

    def check64(self, plan, ins, got):
        ref, bound = self.reference(ins)
        assert got.shape == ref.shape
        r = TW.ratio(got, ref, bound)
        assert r <= 1.0, (self.rid, r)


class KaldiRow(Row):
    """KaldiPlan.compute_torch (sgx_kaldi_execute); size counts frames (N = 400, shift = 160).  `chunk`: max_scratch_bytes as that
    many frames of the generic route."""
    entry = "sgx_kaldi_execute"
    has_stream_arg = True
    counts_allocations = True
    tiny = 1

    def __init__(self, dtype, kw, expect, nf=35, scratch=False, route="auto", chunk=0, tag=""):
        self.dtype, self.kw, self.expect, self.size, self.scratch, self.route = dtype, kw, (expect,), nf, scratch, route
        # tests/test_kaldi.py::test_gpu_generic_chunks_do_not_change_the_bits: max(P, 2 (P / 2 + 1)) = 514 elements per frame and buffer
        self.max_scratch = chunk * 514 * np.dtype(NP[dtype]).itemsize if chunk else None
        self.rid = f"kaldi-{dtype[5:]}-{expect}-{tag}"

    def fresh(self, device=None):
        return sg.KaldiPlan(TK.KP(**self.kw), self.dtype, device=device, route=self.route, max_scratch_bytes=self.max_scratch)

    def n_samples(self, nf):
        return 400 + (nf - 1) * 160 + 7  # a ragged tail that no frame reads

    def gen(self, batch, nf, seed):
        return (TK.noise_rows(batch, self.n_samples(nf), self.dtype, seed),)

    def alloc(self, plan, ins):
        import torch
        b, n = ins[0].shape
        return torch.empty((b, plan.n_frames(n), plan.n_out), dtype=ins[0].dtype, device="cuda")

    def call(self, plan, ins, out, stream=0):
        x = ins[0]
        if not stream:
            plan.compute_torch(x, out=out)
            return
        b, n = x.shape
        _status(plan, _ffi.lib().sgx_kaldi_execute(plan._h, x.data_ptr(), b, n, n, out.data_ptr(), out.numel(), _ffi.MEM_DEVICE, C.c_void_p(stream)))

    def host(self, plan, ins):
        return plan.compute(ins[0])

    def reserve(self, plan, batch, nf):
        plan.reserve(batch, self.n_samples(nf), host_staging=False)

    def names(self, plan):
        return (plan.kernel_name,)

    def reference(self, ins):
        """tests/kaldi_ref.py's (reference, bound), its range condition r <= 0.1 asserted on the reference alone."""
        ref, bound, worst = KR.reference(ins[0], TK.KP(**self.kw), self.dtype)
        assert worst <= 0.1, f"{self.rid}: input outside the bound's range: r = {worst}"
        return ref, bound

    def check64(self, plan, ins, got):
        ref, bound = self.reference(ins)
        assert got.shape == ref.shape
        r = KR.ratio(got, ref, bound)
        assert r <= 1.0, (self.rid, r)


def _resample_n(ratio, dtype):
    """One and a half tiles of outputs (tests/test_resample.py::bound_inputs): more than one workgroup, a ragged last tile."""
    M, L, _, _, _, tile = TR.geometry(*ratio, dtype)
    return -(-3 * tile * M // (2 * L)) + 3


class ResampleRow(Row):
    """ResamplePlan.resample_torch (sgx_resample_resample); size counts input samples.  The device path owns no scratch."""
    entry = "sgx_resample_resample"
    has_stream_arg = True
    counts_allocations = True
    tiny = 1

    def __init__(self, dtype, ratio, expect):
        self.dtype, self.ratio, self.expect, self.size = dtype, ratio, (expect,), _resample_n(ratio, dtype)
        self.rid = f"resample-{dtype[5:]}-{ratio[0]}to{ratio[1]}-{expect}"

    def fresh(self, device=_ffi.DEVICE_CURRENT):
        return sg.ResamplePlan(*self.ratio, dtype=self.dtype, device=device)

    def gen(self, batch, n, seed):
        return (TR.noise(n, self.dtype, seed, batch),)

    def alloc(self, plan, ins):
        import torch
        b, n = ins[0].shape
        return torch.empty((b, plan.out_len(n)), dtype=ins[0].dtype, device="cuda")

    def call(self, plan, ins, out, stream=0):
        x = ins[0]
        if not stream:
            plan.resample_torch(x, out=out)
            return
        b, n = x.shape
        _status(plan, _ffi.lib().sgx_resample_resample(plan._h, x.data_ptr(), b, n, n, out.data_ptr(), out.numel(), _ffi.MEM_DEVICE, C.c_void_p(stream)))

    def reserve(self, plan, batch, n):
        plan.reserve(batch, n, host_staging=False)

    def names(self, plan):
        return (plan.kernel_name,)

    def check64(self, plan, ins, got):  # tests/test_resample.py::check_bound, per output sample
        TR.check_bound(got, ins[0], TR.geometry(*self.ratio, self.dtype), self.dtype)


class ScheduleRow(Row):
    """A state-carrying family: one `call` is a fixed schedule of calls on one plan that starts from and returns to the state after
    reset / flush, so it is a pure function of its input.  The inputs of the calls are views into one tensor, their outputs
    consecutive slices of one flat `out`; `counts(plan)` is the number of output elements (of the plan's real type) per call."""
    has_stream_arg = True
    counts_allocations = True

    def alloc(self, plan, ins):
        import torch
        return torch.empty(sum(self.counts(plan, ins[0].shape[0])), dtype=getattr(torch, self.dtype), device="cuda")

    def slices(self, plan, out, batch):
        at = np.cumsum([0] + self.counts(plan, batch))
        return [out[a:b] for a, b in zip(at[:-1], at[1:])]


class StreamRow(ScheduleRow):
    """StreamingPlan (sgx_stream_push, sgx_stream_flush): push 700 samples, push 1040 samples, flush.  Each push is k_stream_stage into
    the other work buffer and the plan's launch on it."""
    entry = ("sgx_stream_push", "sgx_stream_flush")
    CUTS = (700, 1040)

    def __init__(self, dtype, shape, output, expect):
        self.dtype, self.shape, self.output, self.expect, self.size = dtype, shape, output, (expect,), sum(self.CUTS)
        self.rid = f"stream-{dtype[5:]}-{shape[0]}-{shape[1]}-{'c' if shape[2] else 'n'}-{output}"

    def fresh(self, device=_ffi.DEVICE_CURRENT):
        """A stream reserved for the schedule.  The two work buffers take turns and each grows on its own (the header: "a larger one
        replaces a work buffer once (it waits for `stream` and the device)"); a schedule with an odd number of staging calls swaps
        their roles, so without the reserve the second schedule of A would still replace a buffer and wait, as documented."""
        stream = TS.make_pair(self.shape, self.output, self.dtype, device)[1]
        if device != _ffi.DEVICE_HOST_ONLY:
            stream.reserve(self.batch, max(self.CUTS), host_staging=False)
        return stream

    def frames(self):
        """Frames per call, by the header's arithmetic (the flush appends pad samples)."""
        n_fft, hop, centre = self.shape
        pad = n_fft // 2 if centre else 0
        p, out = pad, []
        for c in self.CUTS + (pad,):
            P = p + c
            f = (P - n_fft) // hop + 1 if P >= n_fft else 0
            p = P - f * hop
            out.append(f)
        return out

    def counts(self, plan, batch):
        return [batch * plan.n_bins * f * (2 if plan.is_complex else 1) for f in self.frames()]

    def gen(self, batch, n, seed):
        assert n == self.size
        return (_noise(batch, n, self.dtype, seed),)

    def _views(self, plan, out, batch):
        import torch
        views = []
        for s, f in zip(self.slices(plan, out, batch), self.frames()):
            views.append(torch.view_as_complex(s.view(batch, plan.n_bins, f, 2)) if plan.is_complex else s.view(batch, plan.n_bins, f))
        return views

    def call(self, plan, ins, out, stream=0):
        x = ins[0]
        views, frames, at = self._views(plan, out, x.shape[0]), self.frames(), 0
        for c, f, v in zip(self.CUTS, frames, views):
            assert plan.frames(c) == f > 0
            plan.push(x[:, at:at + c], out=v, stream=stream)
            at += c
        assert plan.flush_frames() == frames[-1]
        plan.flush(out=views[-1], stream=stream)

    def reserve(self, plan, batch, n):
        plan.reserve(batch, max(self.CUTS), host_staging=False)

    def names(self, plan):
        return (plan.kernel_name,)

    def check64(self, plan, ins, got):  # tests/test_streaming.py::test_frames_of_the_whole_signal
        b = ins[0].shape[0]
        parts = [s.reshape((b, plan.n_bins, f, 2) if plan.is_complex else (b, plan.n_bins, f)) for s, f in zip(self.slices(plan, got, b), self.frames())]
        whole = np.concatenate(parts, axis=2)
        if plan.is_complex:
            whole = np.ascontiguousarray(whole).view(CNP[self.dtype])[..., 0]
        ref, pow64 = TS.oracle_ref(self.shape, self.output, ins[0])
        assert whole.shape == ref.shape
        TS.compare(whole, ref, pow64, self.output, self.dtype)


class IstreamRow(ScheduleRow):
    """StreamingInversePlan (sgx_istream_push, sgx_istream_flush): push 3 frames, push 8 frames, flush.  Each call is the rows of the
    unfused inverse into the frame scratch, then k_istream_ola (carry + new frames -> out and the other carry buffer)."""
    entry = ("sgx_istream_push", "sgx_istream_flush")
    CUTS = (3, 8)

    def __init__(self, dtype, shape, expect):
        self.dtype, self.shape, self.expect, self.size = dtype, shape, (expect,), sum(self.CUTS)
        self.rid = f"istream-{dtype[5:]}-{shape[0]}-{shape[1]}-{'c' if shape[2] else 'n'}"

    def fresh(self, device=_ffi.DEVICE_CURRENT):
        return TSI.make_pair(self.dtype, *self.shape, "hanning", device)[1]

    def samples(self):
        """Samples per row and call: hi(F + f) - hi(F), and the flush up to E(F) - pad (include/spectro_hip.h)."""
        n_fft, hop, centre = self.shape
        pad, F, out = (n_fft // 2 if centre else 0), 0, []
        for f in self.CUTS:
            out.append(TSI.hi(n_fft, hop, pad, F + f) - TSI.hi(n_fft, hop, pad, F))
            F += f
        out.append((F - 1) * hop + n_fft - pad - TSI.hi(n_fft, hop, pad, F))
        return out

    def counts(self, plan, batch):
        return [batch * m for m in self.samples()]

    def gen(self, batch, nf, seed):
        assert nf == self.size
        rng = np.random.default_rng(seed)
        n_fft = self.shape[0]
        return (np.ascontiguousarray(np.stack([TI.rand_spec(rng, n_fft // 2 + 1, nf, n_fft, np.ones(nf)) for _ in range(batch)]).astype(CNP[self.dtype])),)

    def call(self, plan, ins, out, stream=0):
        S = ins[0]
        b, at = S.shape[0], 0
        views = [s.view(b, m) for s, m in zip(self.slices(plan, out, b), self.samples())]
        for f, v in zip(self.CUTS, views):
            assert plan.samples(f) == v.shape[1] > 0
            plan.push(S[:, :, at:at + f], out=v, stream=stream)
            at += f
        assert plan.flush_samples() == views[-1].shape[1]
        plan.flush(out=views[-1], stream=stream)

    def reserve(self, plan, batch, nf):
        plan.reserve(batch, max(self.CUTS), host_staging=False)

    def names(self, plan):
        return (plan.kernel_name,)

    def check64(self, plan, ins, got):  # tests/test_streaming_inverse.py::test_every_sample_of_every_call_within_the_f64_bound
        n_fft, hop, centre = self.shape
        b = ins[0].shape[0]
        whole = np.concatenate([s.reshape(b, m) for s, m in zip(self.slices(plan, got, b), self.samples())], axis=1)
        host = TI.make_plan(self.dtype, n_fft, hop, centre, "hanning", device=_ffi.DEVICE_HOST_ONLY)
        assert whole.shape == (b, host.istft_length(self.size))
        TSI.check_bound(whole, ins[0], list(self.CUTS), n_fft, hop, centre, TI.plan_window(host, self.dtype), self.dtype,
                        self.expect[0].replace("+stream_ola", ""), False, self.rid)


class ResampleStreamRow(ScheduleRow):
    """ResamplePlan's streaming calls (sgx_resample_reset, _process, _process, _flush).  The leading reset belongs to the call: its
    zeroing of the history is held to stream order too.  The wrappers have no `stream=`: the explicit-stream schedule goes to the C
    entry points."""
    entry = ("sgx_resample_reset", "sgx_resample_process", "sgx_resample_flush")

    def __init__(self, dtype, ratio, expect):
        self.dtype, self.ratio, self.expect, self.size = dtype, ratio, (expect,), _resample_n(ratio, dtype)
        self.first = TR.geometry(*ratio, dtype)[0] + 7  # M + 7 samples, then the rest
        self.rid = f"resample-stream-{dtype[5:]}-{ratio[0]}to{ratio[1]}-{expect}"

    def fresh(self, device=_ffi.DEVICE_CURRENT):
        return sg.ResamplePlan(*self.ratio, dtype=self.dtype, device=device)

    def cuts(self):
        return (self.first, self.size - self.first)

    def counts(self, plan, batch):
        c1, c2 = self.cuts()
        per = [plan.step(0, c1)[0], plan.step(c1, c2)[0], plan.step(c1 + c2, 0)[0]]
        assert sum(per) == plan.out_len(self.size) and min(per) > 0
        return [batch * m for m in per]

    def gen(self, batch, n, seed):
        assert n == self.size
        return (TR.noise(n, self.dtype, seed, batch),)

    def call(self, plan, ins, out, stream=0):
        x = ins[0]
        b, n = x.shape
        c1 = self.first
        views = [s.view(b, -1) for s in self.slices(plan, out, b)]
        if not stream:
            plan.reset()
            plan.process_torch(x[:, :c1], out=views[0])
            plan.process_torch(x[:, c1:], out=views[1])
            plan.flush_torch(out=views[2])
            return
        L, s, D = _ffi.lib(), C.c_void_p(stream), _ffi.MEM_DEVICE
        _status(plan, L.sgx_resample_reset(plan._h, s))
        _status(plan, L.sgx_resample_process(plan._h, x.data_ptr(), b, c1, n, views[0].data_ptr(), views[0].numel(), D, s))
        _status(plan, L.sgx_resample_process(plan._h, x[:, c1:].data_ptr(), b, n - c1, n, views[1].data_ptr(), views[1].numel(), D, s))
        _status(plan, L.sgx_resample_flush(plan._h, views[2].data_ptr(), views[2].numel(), D, s))

    def reserve(self, plan, batch, n):
        plan.reserve(batch, max(self.cuts()), host_staging=False)

    def names(self, plan):
        return (plan.kernel_name,)

    def check64(self, plan, ins, got):  # tests/test_resample.py: the calls laid end to end are the outputs of the whole rows
        b = ins[0].shape[0]
        whole = np.ascontiguousarray(np.concatenate([s.reshape(b, -1) for s in self.slices(plan, got, b)], axis=1))
        TR.check_bound(whole, ins[0], TR.geometry(*self.ratio, self.dtype), self.dtype)


def _istft_rows():
    rows = []
    for name in sorted(n for n in TI.NAMES if n.endswith("+ola") or n.startswith("istft")):
        for dt in (F32, F64):
            hit = [r for r in TI.ROUTES if r[0] == dt and r[5] == name]
            if hit:
                rows.append(IstftRow(hit[0]))
    return rows


# Shapes from tests/test_bank_readback.py's CASES (9 frames unless its table says "@41"), tests/test_gpu_parity.py, tests/test_bigfft.py,
# tests/test_cqt.py's SHAPES, tests/test_istft_precision.py's ROUTES, tests/test_mdct.py, tests/test_binaural.py, tests/test_gammatone.py.
CASES = [
    # one fused launch
    ForwardRow(F32, 1024, 256, "power", 0, 41, ("r32x16_f32", "")),
    ForwardRow(F32, 1024, 256, "db", 80, 41, ("r32x16_f32", "r32x16_sched")),
    ForwardRow(F32, 1024, 256, "complex", 0, 41, ("r32x16_f32", "")),
    ForwardRow(F64, 1024, 256, "power", 0, 41, ("d32x16_f64", "")),
    ForwardRow(F64, 1024, 256, "db", 128, 9, ("d32x16_f64", "d32x16_sched")),
    ForwardRow(F64, 1024, 256, "complex", 0, 41, ("d32x16_f64", "")),
    ForwardRow(F32, 1024, 256, "mfcc", 40, 9, ("r32x16_f32", "r32x16_sched_mfcc")),
    # packed tiles: 32 signals of 5 frames
    ForwardRow(F32, 1024, 256, "power", 80, 5, ("r32x16_f32", "r32x16_sched_packed"), batch=32, tag="packed"),
    # the bank stage, then a separate MFCC launch
    ForwardRow(F32, 512, 160, "mfcc", 40, 9, ("r32x16_f32", "r32x16_sched512+mfcc_acc"), scratch=True),
    ForwardRow(F64, 1024, 256, "mfcc", 40, 9, ("d32x16_f64", "d32x16_sched+mfcc_acc"), scratch=True),
    # split bank: per-bin power into plan scratch, then k_bank_rows
    ForwardRow(F32, 4096, 2048, "power", 80, 9, ("r64x32_f32", "bank_rows"), scratch=True),
    ForwardRow(F64, 2048, 512, "power", 300, 9, ("d32x32_f64", "bank_rows"), scratch=True),
    ForwardRow(F64, 2048, 512, "mfcc", 400, 9, ("d32x32_f64", "bank_rows+mfcc_rows"), scratch=True),
    # chroma: the kernel, then k_chroma_norm on the caller's buffer
    ForwardRow(F32, 1024, 256, "chroma", 0, 9, ("r32x16_f32", "r32x16_mfma")),
    ForwardRow(F64, 2048, 512, "chroma", 0, 9, ("d32x32_f64", "d32x32_sched")),
    # register-tiled kernel, chirp-z fused and split
    ForwardRow(F32, 400, 160, "power", 0, 9, ("reg_radix", "")),
    ForwardRow(F64, 400, 160, "power", 0, 9, ("reg_radix", "")),
    ForwardRow(F64, 400, 160, "power", 40, 9, ("reg_radix", "bank_rows"), scratch=True),
    ForwardRow(F32, 401, 160, "power", 40, 9, ("bluestein", "bluestein_rows")),
    ForwardRow(F64, 401, 160, "power", 40, 9, ("bluestein", "bank_rows"), scratch=True),
    ForwardRow(F32, 2003, 500, "power", 80, 9, ("bluestein", "bank_rows"), scratch=True),
    # transforms through global memory; the last one runs 1200 sequences of 512 KiB in three chunks of the 256 MiB scratch
    ForwardRow(F32, 65536, 16384, "big", 0, 5, ("big_four_step", ""), scratch=True),
    ForwardRow(F64, 65536, 16384, "big", 0, 5, ("big_four_step", ""), scratch=True),
    ForwardRow(F32, 9001, 2250, "big", 0, 7, ("big_chirpz", ""), scratch=True),
    ForwardRow(F64, 12000, 3000, "big", 0, 7, ("big_chirpz", ""), scratch=True),
    ForwardRow(F32, 9001, 2250, "power", 80, 7, ("big_chirpz", "bank_rows"), scratch=True),
    ForwardRow(F64, 12000, 3000, "big", 0, 11, ("big_chirpz", ""), batch=200, tag="chunks"),
    CqtRow(F32, "musical_1024_256", "cqt_mfma_lds"),
    CqtRow(F64, "musical_1024_256", "cqt_mfma_lds"),
    CqtRow(F32, "lds_overflow", "cqt_mfma_global"),
    CqtRow(F64, "lds_overflow", "cqt_mfma_global"),
    *_istft_rows(),
    MdctRow(F32, 2048, False, "k_mdct_fwd"), MdctRow(F64, 2048, False, "k_mdct_fwd"),
    MdctRow(F32, 2048, True, "k_imdct_ola"), MdctRow(F64, 2048, True, "k_imdct_ola"),
    MdctRow(F32, 1000, False, "mdct_generic"), MdctRow(F64, 1000, False, "mdct_generic"),
    MdctRow(F32, 1000, True, "imdct_generic"), MdctRow(F64, 1000, True, "imdct_generic"),
    BinauralRow(F32, 1024, 256, "r32x16_binaural_f32", False),
    BinauralRow(F64, 1024, 256, "binaural_epilogue/d32x16_f64", True),
    BinauralRow(F32, 512, 128, "binaural_epilogue/r32x16_f32", True),
    HistogramRow(F32), HistogramRow(F64),
    GammatoneRow(F32), GammatoneRow(F64),
]
EARLIER = len(CASES)
_KALDI_MFCC = dict(num_mel_bins=23, num_ceps=13, subtract_mean=True)
CASES += [
    # k_welch: one launch leaves a partial per tile in d_part, k_welch_fold adds a row's partials (41 segments: two tiles of 32)
    WelchRow(F32, 1024, "coherence", "k_welch"),
    WelchRow(F64, 1024, "csd", "k_welch"),
    WelchRow(F32, 256, "psd", "k_welch"),
    # welch_generic: the memset of d_part, then gather / transform / accumulate per chunk, then the fold; the last row cuts the
    # 164 segments of the batch into chunks of 60, 60 and 44 (the seams fall inside rows 1 and 2)
    WelchRow(F32, 400, "psd", "welch_generic", scratch=True),
    WelchRow(F64, 400, "coherence", "welch_generic", scratch=True),
    WelchRow(F32, 400, "psd", "welch_generic", scratch=True, chunk=60, tag="chunks"),
    # k_kaldi: one launch (35 frames: a tile of 32 and 3); with subtract_mean a second one, k_kaldi_cmn, in place on the caller's buffer
    KaldiRow(F32, dict(num_mel_bins=80), "k_kaldi", tag="fbank80"),
    KaldiRow(F64, dict(use_energy=True, **_KALDI_MFCC), "k_kaldi", tag="mfcc13-energy-cmn"),
    # kaldi_generic: k_kaldi_gather, the inner sgx_execute, k_kaldi_bank per chunk over scratch that the chunks share (+ k_kaldi_cmn);
    # the last row cuts the 80 frames of the batch into chunks of 25, 25, 25 and 5
    KaldiRow(F32, dict(num_mel_bins=80, round_to_power_of_two=False), "kaldi_generic", scratch=True, tag="P400-fbank80"),
    KaldiRow(F64, _KALDI_MFCC, "kaldi_generic", scratch=True, route="generic", tag="mfcc13-cmn"),
    KaldiRow(F32, dict(num_mel_bins=80), "kaldi_generic", nf=20, scratch=True, route="generic", chunk=25, tag="fbank80-chunks"),
    # the stateless resampler: one launch on either route
    ResampleRow(F32, (44100, 16000), "k_resample_pp"), ResampleRow(F64, (44100, 16000), "k_resample_pp"),
    ResampleRow(F32, TR.GENERIC_ONLY, "resample_generic"), ResampleRow(F64, TR.GENERIC_ONLY, "resample_generic"),
    # the state-carrying families, one fixed schedule per call
    StreamRow(F32, (1024, 256, True), "complex", "r32x16_f32"),
    StreamRow(F64, (400, 160, False), "mel_db", "reg_radix"),
    IstreamRow(F32, (512, 160, True), "c2r_reg+stream_ola"), IstreamRow(F64, (512, 160, True), "c2r_reg+stream_ola"),
    ResampleStreamRow(F32, (44100, 16000), "k_resample_pp"), ResampleStreamRow(F64, (44100, 16000), "k_resample_pp"),
]
IDS = [r.rid for r in CASES]
SCRATCH = [r for r in CASES if r.scratch]
NEW = CASES[EARLIER:]

# Prototypes with a stream parameter that no row exercises, each with the one reason that allows it
EXEMPT = {
    "sgx_fir_process": "own census",
    "sgx_fir_convolve": "own census",
    "sgx_fir_reset": "own census",
    "sgx_deconv_execute": "own census",
    "sgx_minphase_execute": "own census",
    "sgx_stream_reset": "enqueues nothing",
    "sgx_istream_reset": "enqueues nothing",
    "sgx_execute_timed": "synchronises",
    "sgx_clock_probe": "synchronises",
    "sgx_gather": "peer ranks",
    "sgx_shard_execute": "peer ranks",
    "sgx_shard_execute_chunked": "peer ranks",
    "sgx_fft2d_forward": "2-D family",
    "sgx_fft2d_inverse": "2-D family",
    "sgx_fft2d_convolve": "2-D family",
    "sgx_fft2d_filter": "2-D family",
}


# ---- CPU: every prototype with a stream parameter has a row or an allowed exemption ----------------------------------------------------
def _header():
    return open(os.path.join(os.path.dirname(__file__), "..", "include", "spectro_hip.h")).read()


def _stream_prototypes(src=None):
    """name -> (parameter list, the comment block right above the prototype) for every prototype with a `void *hip_stream` or a
    `void *stream`."""
    src = _header() if src is None else src
    found = {}
    for m in re.finditer(r"\bsgx_status\s+(\w+)\s*\(([^;{]*?)\)\s*;", src, re.S):
        if re.search(r"void\s*\*\s*(?:hip_)?stream\b", m.group(2)):
            above = re.search(r"/\*((?:(?!\*/).)*)\*/\s*$", src[:m.start()], re.S)
            found[m.group(1)] = (m.group(2), above.group(1) if above else "")
    return found


def _uncovered(protos, rows, exempt):
    """The stream-taking prototypes that neither a row nor an exemption names."""
    covered = {e for r in rows for e in r.entries}
    return set(protos) - covered - set(exempt)


def test_every_hip_stream_prototype_has_a_row_or_an_allowed_exemption():
    protos = _stream_prototypes()
    assert len(protos) >= 33 and "sgx_execute" in protos and "sgx_gammatone_execute" in protos  # the parser sees the header,
    assert "sgx_kaldi_execute" in protos and "sgx_istream_flush" in protos                      # both spellings of the parameter
    covered = {e for r in CASES for e in r.entries}
    assert covered <= set(protos), covered - set(protos)
    assert not (covered & set(EXEMPT))
    missing = _uncovered(protos, CASES, EXEMPT)
    assert not missing, f"stream entry points without a CASES row or an exemption: {sorted(missing)}"
    assert set(EXEMPT) <= set(protos), set(EXEMPT) - set(protos)
    from tests.test_fir import STREAM_COVERAGE as fir_census
    from tests.test_minphase import STREAM_COVERAGE as minphase_census
    for name, reason in EXEMPT.items():
        params, comment = protos[name]
        if reason == "synchronises":  # the prototype's own comment says so
            assert re.search(r"Synchronises the stream|waits for the stream", comment), name
        elif reason == "peer ranks":
            assert re.search(r"\bsgx_comm\s*\*\s*comm\b", params), name
        elif reason == "own census":  # the family's file keeps a census of its own, and the name is in it
            assert name in fir_census or name in minphase_census, name
        elif reason == "enqueues nothing":  # the prototype's own comment says so
            assert "nothing is enqueued" in comment, name
        else:
            assert reason == "2-D family" and name.startswith("sgx_fft2d_"), name


def test_the_census_reports_a_new_prototype_and_a_missing_row():
    """The comparison can fail: a prototype added to the header text, and a family whose rows are taken out of the table, are each
    reported by name, and nothing else is."""
    src = _header()
    assert not _uncovered(_stream_prototypes(src), CASES, EXEMPT)
    at = src.index("sgx_status sgx_kaldi_execute(")
    grown = src[:at] + "sgx_status sgx_new_thing(sgx_kaldi *plan, const void *x, size_t batch, void *out, void *stream);\n" + src[at:]
    assert _uncovered(_stream_prototypes(grown), CASES, EXEMPT) == {"sgx_new_thing"}
    older = src[:at] + "sgx_status sgx_old_thing(sgx_kaldi *plan, const void *x, size_t batch, void *out, void *hip_stream);\n" + src[at:]
    assert _uncovered(_stream_prototypes(older), CASES, EXEMPT) == {"sgx_old_thing"}
    without = [r for r in CASES if not isinstance(r, KaldiRow)]
    assert len(without) == len(CASES) - 5
    assert _uncovered(_stream_prototypes(src), without, EXEMPT) == {"sgx_kaldi_execute"}


def test_rows_name_their_routes_and_ids_are_unique():
    assert len(set(IDS)) == len(IDS)
    assert {r.expect[0] for r in CASES if isinstance(r, IstftRow)} == {n for n in TI.NAMES if n.endswith("+ola") or n.startswith("istft")}
    from tests.test_bank_readback import NAMES, SUFFIXES
    for r in CASES:
        if isinstance(r, ForwardRow) and r.expect[1]:
            stage, _, epi = r.expect[1].partition("+")
            assert stage in NAMES and (not epi or "+" + epi in SUFFIXES), r.rid


@pytest.mark.parametrize("row", [r for r in NEW if not isinstance(r, IstreamRow)], ids=[r.rid for r in NEW if not isinstance(r, IstreamRow)])
def test_new_rows_name_their_routes_on_a_host_only_plan(row):
    """(An inverse stream has no route name before its first call: its rows assert theirs on the GPU only.)"""
    plan = row.fresh(device=_ffi.DEVICE_HOST_ONLY)
    assert row.names(plan) == row.expect
    if isinstance(row, ScheduleRow):
        counts = row.counts(plan, row.batch)
        assert len(counts) == len(row.entries) + (0 if isinstance(row, ResampleStreamRow) else 1) and min(counts[:-1]) > 0
    if isinstance(row, StreamRow):  # the frames of the schedule are those of the whole signal
        assert sum(row.frames()) == orc.frame_count(row.size, *row.shape) and plan.frames(row.CUTS[0]) == row.frames()[0]
    if isinstance(row, KaldiRow):
        assert plan.n_frames(row.n_samples(row.size)) == row.size and plan.n_frames(row.n_samples(row.size) + 153) == row.size + 1
        assert (plan.tile > 0) == (row.expect == ("k_kaldi",)) and row.size % 32 != 0
    if isinstance(row, WelchRow):
        assert plan.n_segments(row.n_samples(row.size)) == row.size > plan.tile


def test_istream_rows_lay_the_whole_signal_end_to_end():
    for row in NEW:
        if isinstance(row, IstreamRow):
            n_fft, hop, centre = row.shape
            host = TI.make_plan(row.dtype, n_fft, hop, centre, "hanning", device=_ffi.DEVICE_HOST_ONLY)
            assert sum(row.samples()) == host.istft_length(row.size) and min(row.samples()) > 0
            assert row.fresh(device=_ffi.DEVICE_HOST_ONLY).samples(row.CUTS[0]) == row.samples()[0]


RANGED = [r for r in NEW if isinstance(r, (WelchRow, KaldiRow))]


@pytest.mark.parametrize("row", RANGED, ids=[r.rid for r in RANGED])
def test_new_rows_references_are_inside_their_bounds_range(row):
    """The coherence bound (tests/test_welch.py) and the Kaldi bound (tests/kaldi_ref.py, r <= 0.1) hold on a range of inputs only:
    each row's reference is inside it (asserted in `reference`), before any GPU is touched."""
    ins = row.gen(row.batch, row.size, 1)
    ref, bound = row.reference(ins)
    assert ref.shape == bound.shape and np.all(np.isfinite(bound)) and np.all(bound > 0)


# ---- GPU helpers -------------------------------------------------------------------------------------------------------------------------
def bits(t):
    """The tensor's bytes as integers (NaN-safe equality)."""
    import torch
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def where(a, b):
    """For a failure message: how many elements of two tensors of one shape differ, and the first and the last flat index."""
    import torch
    if a.shape != b.shape:
        return f" (shapes {tuple(a.shape)} and {tuple(b.shape)})"
    bad = torch.nonzero(bits(a).flatten() != bits(b).flatten()).flatten()
    return f" ({bad.numel()} of {bits(a).numel()} words differ, the first at {int(bad[0])}, the last at {int(bad[-1])})" if bad.numel() else ""


def np_same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def eager(row, ins):
    """A fresh plan called on the null stream, synchronised: (result, route names)."""
    import torch
    plan = row.fresh()
    out = row.alloc(plan, ins)
    row.call(plan, ins, out)
    torch.cuda.synchronize()
    return out, row.names(plan)


def fill_nan(t):
    t.fill_(complex(float("nan"), float("nan")) if t.is_complex() else float("nan"))


_PRODUCER = {}


def producer():
    """(buffer, operations): a chain of in-place additions on a 1 GiB buffer that takes about PRODUCER_AIM_MS on this device."""
    import torch
    if not _PRODUCER:
        big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
        for _ in range(4):
            big.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(16):
            big.add_(1.0)
        e1.record()
        torch.cuda.synchronize()
        per = e0.elapsed_time(e1) / 16.0
        _PRODUCER["big"], _PRODUCER["ops"] = big, max(8, int(math.ceil(PRODUCER_AIM_MS / per)))
    return _PRODUCER["big"], _PRODUCER["ops"]


# ---- the eager reference against f64, once per row -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("row", CASES, ids=IDS)
def test_gpu_eager_reference_meets_the_owning_files_f64_bound(row):
    ins = row.gen(row.batch, row.size, 1)
    if row.batch > 32:  # the many-sequence row: the bound on its first and last signals
        ins = tuple(np.concatenate([a[:2], a[-2:]]) for a in ins)
    out, names = eager(row, row.dev(ins))
    assert names == row.expect
    row.check64(row.fresh(), ins, out.cpu().numpy())


# ---- A: one operation of the caller's stream -----------------------------------------------------------------------------------------------
def _property_a(row, how):
    import torch
    big, ops = producer()
    ins = row.dev(row.gen(row.batch, row.size, 1))
    other = row.dev(row.gen(row.batch, row.size, 7))
    ref, ref_names = eager(row, ins)
    assert ref_names == row.expect
    plan = row.fresh()
    xin = tuple(torch.empty_like(a) for a in ins)
    out = row.alloc(plan, ins)
    sentinel = torch.full_like(out, SENTINEL)
    side = torch.cuda.Stream()
    arg = side.cuda_stream if how == "arg" else 0

    def call():
        if how == "arg":  # torch's current stream is the null stream; the call gets the side stream explicitly
            assert torch.cuda.current_stream().cuda_stream != side.cuda_stream
            row.call(plan, xin, out, stream=arg)
        else:
            with torch.cuda.stream(side):
                row.call(plan, xin, out)

    # warm: the same sequence on other data (scratch, code objects, the allocator's blocks of the side stream)
    with torch.cuda.stream(side):
        for x, a in zip(xin, other):
            x.copy_(a)
    call()
    with torch.cuda.stream(side):
        snap = out.clone()
        out.copy_(sentinel)
    torch.cuda.synchronize()
    assert not same(snap, ref)  # the warm call left other values in every buffer
    del snap
    # 1: NaN in, sentinel out
    for x in xin:
        fill_nan(x)
    out.copy_(sentinel)
    torch.cuda.synchronize()
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    # 2: the producer; its last operations write the samples
    with torch.cuda.stream(side):
        e0.record()
        for _ in range(ops):
            big.add_(1.0)
        for x, a in zip(xin, ins):
            x.copy_(a)
        e1.record()
    t0 = time.perf_counter()
    # 3: the call, a clone, the sentinel; no host synchronisation
    call()
    with torch.cuda.stream(side):
        snap = out.clone()
        out.copy_(sentinel)
        e2.record()
    # 4
    producer_done = e1.query()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    prod_ms, ret_ms = e0.elapsed_time(e1), (t1 - t0) * 1e3
    TIMES[f"{row.rid}/{how}"] = (prod_ms, ret_ms)
    print(f"\n{row.rid} [{how}]: producer {prod_ms:.1f} ms, call + clone + fill returned after {ret_ms:.3f} ms, producer done at return: {producer_done}")
    assert same(snap, ref), f"the result queued behind the producer differs from the fresh plan's eager result{where(snap, ref)}"
    assert same(out, sentinel), "something wrote the output after the work queued behind the call"
    assert row.names(plan) == ref_names
    assert prod_ms >= PRODUCER_MIN_MS, prod_ms
    assert producer_done is False, "the call returned only after its input existed: no hazard window was shown"


@pytest.mark.gpu
@pytest.mark.parametrize("row", CASES, ids=IDS)
def test_gpu_call_is_one_operation_of_torchs_current_stream(row):
    _property_a(row, "current")


@pytest.mark.gpu
@pytest.mark.parametrize("row", [r for r in CASES if r.has_stream_arg], ids=[r.rid for r in CASES if r.has_stream_arg])
def test_gpu_call_is_one_operation_of_the_stream_argument(row):
    _property_a(row, "arg")


# ---- B: a reserved call allocates nothing and can be captured -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("row", CASES, ids=IDS)
def test_gpu_reserved_call_is_captured_and_replayed(row):
    import torch
    first = row.gen(row.batch, row.size, 1)
    inputs = [row.dev(first), row.dev(tuple(np.ascontiguousarray(a[::-1]) for a in first)), row.dev(row.gen(row.batch, row.size, 2))]
    refs = [eager(row, i) for i in inputs]  # (also loads every code object the call launches)
    assert all(n == row.expect for _, n in refs)
    plan = row.fresh()
    row.reserve(plan, row.batch, row.size)
    count = plan.allocations if row.counts_allocations else None
    xin = tuple(a.clone() for a in inputs[0])
    out = row.alloc(plan, xin)
    sentinel = torch.full_like(out, SENTINEL)
    out.copy_(sentinel)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        row.call(plan, xin, out)
    assert row.names(plan) == row.expect
    for k in (1, 2, 0):
        for x, a in zip(xin, inputs[k]):
            x.copy_(a)
        out.copy_(sentinel)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, refs[k][0]), f"replay on input {k} differs from the eager result{where(out, refs[k][0])}"
    if row.counts_allocations:
        assert plan.allocations == count, "a call within what reserve sized moved the plan's allocation counter"


# ---- C: a call does not depend on the calls before it -------------------------------------------------------------------------------------
def _step(row, plan, batch, size, seed):
    import torch
    ins = row.dev(row.gen(batch, size, seed))
    ref, ref_names = eager(row, ins)
    out = row.alloc(plan, ins)
    row.call(plan, ins, out)
    torch.cuda.synchronize()
    assert same(out, ref), (row.rid, batch, size)
    assert row.names(plan) == ref_names, (row.rid, batch, size, row.names(plan), ref_names)
    return ref_names


@pytest.mark.gpu
@pytest.mark.parametrize("row", SCRATCH, ids=[r.rid for r in SCRATCH])
def test_gpu_sizes_up_and_down_on_one_plan(row):
    plan = row.fresh()
    n = row.size
    seen = [_step(row, plan, b, s, 10 + i) for i, (b, s) in enumerate([(3, n), (19, 4 * n), (1, row.tiny), (19, 4 * n), (3, n)])]
    assert seen[0] == seen[4] == row.expect and seen[1] == seen[3]


@pytest.mark.gpu
@pytest.mark.parametrize("row", SCRATCH, ids=[r.rid for r in SCRATCH])
def test_gpu_reserve_after_calls_smaller_and_larger(row):
    plan = row.fresh()
    n = row.size
    _step(row, plan, 5, 2 * n, 20)
    row.reserve(plan, 2, n)            # smaller than the calls so far: nothing may shrink under the next call
    _step(row, plan, 5, 2 * n, 21)
    row.reserve(plan, 19, 4 * n)       # larger
    _step(row, plan, 5, 2 * n, 22)
    _step(row, plan, 19, 4 * n, 23)
    _step(row, plan, 2, n, 24)


def _host_step(row, plan, batch, size, seed):
    ins = row.gen(batch, size, seed)
    ref_plan = row.fresh()
    ref = row.host(ref_plan, ins)
    got = row.host(plan, ins)
    assert np_same(got, ref), (row.rid, "host", batch, size)
    assert row.names(plan) == row.names(ref_plan)
    # the host path and the device path of one entry point compute the same bits
    dev, _ = eager(row, row.dev(ins))
    assert np_same(dev.cpu().numpy().reshape(np.asarray(ref).shape), ref), (row.rid, "host vs device", batch, size)


INTERLEAVE = [r for r in CASES if r.rid in {
    "execute-32-4096-2048-power80-r64x32_f32", "execute-64-2048-512-mfcc400-d32x32_f64", "execute-32-9001-2250-big-big_chirpz",
    "execute-64-400-160-power40-reg_radix", "mdct-32-1000-mdct_generic", "mdct-64-1000-imdct_generic", "mdct-32-2048-k_imdct_ola",
    "binaural-64-1024-256-binaural_epilogue_d32x16_f64", "binaural-32-1024-256-r32x16_binaural_f32", "binaural-histogram-64",
    "gammatone-32-bands_65", "gammatone-64-bands_65"} or (isinstance(r, IstftRow) and r.scratch and r.n_fft <= 1024)
    or (isinstance(r, (WelchRow, KaldiRow)) and (r.scratch or r.dtype == F64))]


def test_interleave_rows_exist():
    assert len(INTERLEAVE) >= 16 + 8, [r.rid for r in INTERLEAVE]
    assert {r.rid for r in SCRATCH if isinstance(r, (WelchRow, KaldiRow))} <= {r.rid for r in INTERLEAVE}
    assert {r.expect[0] for r in INTERLEAVE if isinstance(r, (WelchRow, KaldiRow))} == {"k_welch", "welch_generic", "k_kaldi", "kaldi_generic"}
    assert len([r for r in SCRATCH if isinstance(r, (WelchRow, KaldiRow))]) == 6


@pytest.mark.gpu
@pytest.mark.parametrize("row", INTERLEAVE, ids=[r.rid for r in INTERLEAVE])
def test_gpu_host_and_device_calls_interleaved_on_one_plan(row):
    plan = row.fresh()
    n = row.size
    _host_step(row, plan, 3, n, 30)
    _step(row, plan, 5, 2 * n, 31)
    _host_step(row, plan, 2, 3 * n, 32)
    _step(row, plan, 2, n, 33)
    _host_step(row, plan, 1, row.tiny, 34)
    _step(row, plan, 3, n, 35)


STFT_BOTH_WAYS = [(F32, 1024, 256, "r32x16_f32", "istft1024c"), (F64, 400, 160, "reg_radix", "c2r_reg+ola"), (F32, 1024, 63, "r32x16_f32", "c2r_reg+ola"),
                  (F32, 251, 62, "bluestein", "c2r_chirpz+ola"), (F64, 12000, 3000, "big_chirpz", "big+ola")]


def _stft_plan(dtype, n_fft, hop):
    return TI.make_plan(dtype, n_fft, hop, True, "hanning")


def _spec(dtype, n_fft, batch, nf, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([TI.rand_spec(rng, n_fft // 2 + 1, nf, n_fft, np.ones(nf)) for _ in range(batch)]).astype(CNP[dtype]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", STFT_BOTH_WAYS, ids=lambda c: f"{c[0][5:]}-{c[1]}-{c[2]}")
def test_gpu_forward_and_inverse_interleaved_host_and_device_on_one_plan(case):
    """One complex plan runs sgx_execute and sgx_istft on host and device pointers in turn (d_in / d_out are shared staging, the frame
    scratch and the flag word belong to the inverse): every result equals a fresh plan's."""
    import torch
    dtype, n_fft, hop, fwd_name, inv_name = case
    plan = _stft_plan(dtype, n_fft, hop)
    nfs = (9, 30, 2, 30, 9) if n_fft <= 1024 else (5, 12, 1, 12, 5)
    for i, (b, nf) in enumerate(zip((3, 7, 1, 7, 3), nfs)):
        x = _noise(b, (nf - 1) * hop + 1, dtype, 40 + i)
        S = _spec(dtype, n_fft, b, nf, 50 + i)
        f_ref = _stft_plan(dtype, n_fft, hop).compute_batch(x)
        i_fresh = _stft_plan(dtype, n_fft, hop)
        i_ref = i_fresh.istft_batch(S)
        host_first = i % 2 == 0
        for on_host in (host_first, not host_first):
            if on_host:
                assert np_same(plan.compute_batch(x), f_ref), (i, "forward host")
                assert np_same(plan.istft_batch(S), i_ref), (i, "inverse host")
            else:
                yf = plan.compute_batch(torch.from_numpy(x).cuda())
                yi = plan.istft_batch(torch.from_numpy(S).cuda())
                torch.cuda.synchronize()
                assert np_same(yf.cpu().numpy(), f_ref), (i, "forward device")
                assert np_same(yi.cpu().numpy(), i_ref), (i, "inverse device")
            assert plan.kernel_name == fwd_name and plan.istft_kernel_name == i_fresh.istft_kernel_name == inv_name


@pytest.mark.gpu
@pytest.mark.parametrize("case", STFT_BOTH_WAYS, ids=lambda c: f"{c[0][5:]}-{c[1]}-{c[2]}")
def test_gpu_failed_calls_in_the_middle_leave_no_trace(case):
    """A DimensionMismatchError, then on the host inverse path a spectrum with a non-zero imaginary DC bin — FFTBackendError AFTER the
    output was written —; the next clean calls succeed and equal a fresh plan's (the DC / Nyquist flag word is reset per call)."""
    import torch
    dtype, n_fft, hop, _, inv_name = case
    nf = 12 if n_fft <= 1024 else 5
    plan, fresh = _stft_plan(dtype, n_fft, hop), _stft_plan(dtype, n_fft, hop)
    x = _noise(3, (nf - 1) * hop + 1, dtype, 60)
    S = _spec(dtype, n_fft, 3, nf, 61)
    f_ref, i_ref = fresh.compute_batch(x), fresh.istft_batch(S)
    assert np_same(plan.compute_batch(x), f_ref) and np_same(plan.istft_batch(S), i_ref)
    with pytest.raises(sg.DimensionMismatchError):
        plan.compute_batch(x, out=np.empty((3, n_fft // 2 + 1, nf + 1), CNP[dtype]))
    with pytest.raises(sg.DimensionMismatchError):
        plan.istft_batch(S[:, :-1])
    assert np_same(plan.compute_batch(x), f_ref)
    bad = S.copy()
    bad[1, 0, nf // 2] += 1j * 1e-3
    out = np.full(i_ref.shape, SENTINEL, NP[dtype])
    with pytest.raises(sg.FFTBackendError, match="imaginary part"):
        plan.istft_batch(bad, out=out)
    assert np_same(out, i_ref)  # written, the imaginary part ignored in the arithmetic
    assert plan.istft_kernel_name == inv_name
    assert np_same(plan.istft_batch(S), i_ref)  # the flag does not outlive the failed call
    yd = plan.istft_batch(torch.from_numpy(S).cuda())
    torch.cuda.synchronize()
    assert np_same(yd.cpu().numpy(), i_ref) and np_same(plan.istft_batch(S), i_ref)
    # the device path does not report the flag, and a flagged device call does not leak into the next host call
    yb = plan.istft_batch(torch.from_numpy(bad).cuda())
    torch.cuda.synchronize()
    assert np_same(yb.cpu().numpy(), i_ref) and np_same(plan.istft_batch(S), i_ref)
    assert np_same(plan.compute_batch(x), f_ref) and plan.istft_kernel_name == inv_name


FAMILY_FAIL = [r for r in CASES if r.rid in {"mdct-32-1000-mdct_generic", "mdct-64-1000-imdct_generic", "binaural-64-1024-256-binaural_epilogue_d32x16_f64",
                                             "gammatone-32-bands_65", "binaural-histogram-64"}]


@pytest.mark.gpu
@pytest.mark.parametrize("row", FAMILY_FAIL, ids=[r.rid for r in FAMILY_FAIL])
def test_gpu_dimension_mismatch_in_the_middle_mdct_binaural_gammatone(row):
    """The C entry point refuses a wrong out_elems with SGX_DIM_MISMATCH (2) on device pointers; the calls around it are unchanged."""
    import torch
    plan = row.fresh()
    _step(row, plan, 3, row.size, 70)
    ins = row.dev(row.gen(3, row.size, 71))
    out = row.alloc(plan, ins)
    L, s, D = _ffi.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream), _ffi.MEM_DEVICE
    a, wrong = ins[0], out.numel() + 1
    if row.entry == "sgx_mdct_forward":
        st = L.sgx_mdct_forward(plan._h, a.data_ptr(), a.shape[0], a.shape[1], out.data_ptr(), wrong, D, s)
    elif row.entry == "sgx_mdct_inverse":
        st = L.sgx_mdct_inverse(plan._h, a.data_ptr(), a.shape[0], a.shape[1], a.shape[2], out.data_ptr(), wrong, D, s)
    elif row.entry == "sgx_binaural_execute":
        st = L.sgx_binaural_execute(plan._h, a.data_ptr(), ins[1].data_ptr(), a.shape[0], a.shape[1], a.shape[1], out.data_ptr(), wrong, D, s)
    elif row.entry == "sgx_binaural_histogram":
        st = L.sgx_binaural_histogram(plan._h, a.data_ptr(), a.shape[0], a.shape[2], row.NBINS, -math.pi, math.pi, 1, 1, out.data_ptr(), wrong, D, s)
    else:
        st = L.sgx_gammatone_execute(plan._h, a.data_ptr(), a.shape[0], a.shape[1], a.shape[1], out.data_ptr(), wrong, D, s)
    assert st == 2
    _step(row, plan, 3, row.size, 71)
    _host_step(row, plan, 2, row.size, 72)


WELCH_KALDI_FAIL = [r for r in SCRATCH if isinstance(r, (WelchRow, KaldiRow))]


@pytest.mark.gpu
@pytest.mark.parametrize("row", WELCH_KALDI_FAIL, ids=[r.rid for r in WELCH_KALDI_FAIL])
def test_gpu_dimension_mismatch_in_the_middle_welch_kaldi(row):
    """SGX_DIM_MISMATCH (2) on device pointers, twice: a wrong out_elems, and rows one sample shorter than a window.  The calls before
    and after equal a fresh plan's."""
    import torch
    plan = row.fresh()
    _step(row, plan, 3, row.size, 70)
    ins = row.dev(row.gen(3, row.size, 71))
    out = row.alloc(plan, ins)
    L, s, D = _ffi.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream), _ffi.MEM_DEVICE
    x, (b, n) = ins[0], ins[0].shape
    if isinstance(row, WelchRow):
        y, elems, window = (ins[1].data_ptr() if len(ins) > 1 else None), out.numel() * (2 if row.kind == "csd" else 1), row.n

        def execute(n_samples, out_elems):
            return L.sgx_welch_execute(plan._h, x.data_ptr(), y, b, n_samples, n, out.data_ptr(), out_elems, D, s)
    else:
        elems, window = out.numel(), plan.window_size

        def execute(n_samples, out_elems):
            return L.sgx_kaldi_execute(plan._h, x.data_ptr(), b, n_samples, n, out.data_ptr(), out_elems, D, s)
    assert execute(n, elems + 1) == 2
    assert execute(window - 1, elems) == 2
    _step(row, plan, 3, row.size, 71)
    _host_step(row, plan, 2, row.size, 72)
