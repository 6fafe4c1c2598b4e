"""The contract around the 1-D device paths: stream order, `reserve`, and independence from the calls before.

Every batched 1-D entry point takes a `hip_stream`; include/spectro_hip.h promises that a device-pointer call is asynchronous on that
stream, that a call which fits what `reserve` sized allocates nothing, and (single-caller rule) that a plan can be reused call after
call.  CASES holds one row per launch-chain shape of each entry point; every row asserts its route names.

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
tests/test_istft_precision.py's per-sample bound, and the bound functions of test_mdct / test_binaural / test_gammatone / test_cqt).
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
from tests import test_mdct as TM

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
    entry = ""
    has_stream_arg = False
    scratch = False
    batch = 4
    tiny = 3

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
IDS = [r.rid for r in CASES]
SCRATCH = [r for r in CASES if r.scratch]

# Prototypes with a `void *hip_stream` that no row exercises, each with the one reason that allows it
EXEMPT = {
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


# ---- CPU: every hip_stream prototype has a row or an allowed exemption ----------------------------------------------------------------
def _stream_prototypes():
    """name -> (parameter list, the comment block right above the prototype) for every prototype with a `void *hip_stream`."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "include", "spectro_hip.h")).read()
    found = {}
    for m in re.finditer(r"\bsgx_status\s+(\w+)\s*\(([^;{]*?)\)\s*;", src, re.S):
        if re.search(r"void\s*\*\s*hip_stream\b", m.group(2)):
            above = re.search(r"/\*((?:(?!\*/).)*)\*/\s*$", src[:m.start()], re.S)
            found[m.group(1)] = (m.group(2), above.group(1) if above else "")
    return found


def test_every_hip_stream_prototype_has_a_row_or_an_allowed_exemption():
    protos = _stream_prototypes()
    assert len(protos) >= 16 and "sgx_execute" in protos and "sgx_gammatone_execute" in protos  # the parser sees the header
    covered = {r.entry for r in CASES}
    assert covered <= set(protos), covered - set(protos)
    assert not (covered & set(EXEMPT))
    missing = set(protos) - covered - set(EXEMPT)
    assert not missing, f"hip_stream entry points without a CASES row or an exemption: {sorted(missing)}"
    assert set(EXEMPT) <= set(protos), set(EXEMPT) - set(protos)
    for name, reason in EXEMPT.items():
        params, comment = protos[name]
        if reason == "synchronises":  # the prototype's own comment says so
            assert re.search(r"Synchronises the stream|waits for the stream", comment), name
        elif reason == "peer ranks":
            assert re.search(r"\bsgx_comm\s*\*\s*comm\b", params), name
        else:
            assert reason == "2-D family" and name.startswith("sgx_fft2d_"), name


def test_rows_name_their_routes_and_ids_are_unique():
    assert len(set(IDS)) == len(IDS)
    assert {r.expect[0] for r in CASES if isinstance(r, IstftRow)} == {n for n in TI.NAMES if n.endswith("+ola") or n.startswith("istft")}
    from tests.test_bank_readback import NAMES, SUFFIXES
    for r in CASES:
        if isinstance(r, ForwardRow) and r.expect[1]:
            stage, _, epi = r.expect[1].partition("+")
            assert stage in NAMES and (not epi or "+" + epi in SUFFIXES), r.rid


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
    assert same(snap, ref), "the result queued behind the producer differs from the fresh plan's eager result"
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
        assert same(out, refs[k][0]), f"replay on input {k} differs from the eager result"


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
    "gammatone-32-bands_65", "gammatone-64-bands_65"} or (isinstance(r, IstftRow) and r.scratch and r.n_fft <= 1024)]


def test_interleave_rows_exist():
    assert len(INTERLEAVE) >= 16, [r.rid for r in INTERLEAVE]


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
