"""FIR plans (fft_convolve, OverlapSaveConvolver) and deconvolution plans (fft_deconvolve) against a NumPy f64 restatement of
src/convolution.rs.  Every output sample of every row is compared; nothing is left out.

Restatement: convolution is np.convolve (direct sums, no FFT) of the T-cast inputs widened to f64 — for f64 plans with taps <= 256 in
np.longdouble; streaming is the same over the concatenated chunks; deconvolution is the reference's formulas in f64 np.fft.

Deterministic normwise bounds, u_T = 2^-24 / 2^-53, c = 4 (tests/test_mdct.py's constant):
  convolution, per segment of the plan's own segmentation (P = fft_size, S = step read from the plan)
      max_n |dy[n]| <= c u_T log2(P) max_k |H_k| ||x_seg||_2
      x_seg = the P input samples (history included) the segment transforms, H = the f64 P-point transform of the taps.
      (forward error, product and inverse error are each at most u log2 P relative in the 2-norm, and the 2-norm bounds the max)
  deconvolution, with dd_k = |D_k|^2 + eps, g = max_k |D_k| / dd_k, r = max_k |N_k| / dd_k, q the full n-point quotient sequence
      max_n |dy[n]| <= c u_T log2(n) (g ||num||_2 + 3 r ||den||_2 + ||q||_2)
      on inputs with min_k |D_k| >= 0.1 max_k |D_k| or regularization >= 1e-3 (asserted before the GPU is touched).
A streamed signal against the one-call result: each is within its own bound of the restatement, so they differ by at most the sum of
the two bounds (never more than twice the larger).

The level step (10^6 : 1, loud first, in the middle of a segment) is the input that rules out carrying two segments in one complex
transform: the quiet segment right of the step then comes out with about 10^3 times its bound.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi

F32, F64 = "float32", "float64"
NP = {F32: np.float32, F64: np.float64}
U = {F32: 2.0 ** -24, F64: 2.0 ** -53}
CB = 4.0
WORST = {}
FUSED_TAPS = (1, 3, 64, 200, 1025, 2049)
GENERIC_ONLY_TAPS = (2050, 5000, 40000)
MAC_CAP = 1.2e9  # multiply-adds of one direct-sum reference (the one multi-segment 40 000-tap case is exempt)


def _record(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    print(f"{name}: worst ratio to bound {WORST[name]:.3g}")


def tcast(a, dtype):
    """The T-valued input, widened to f64."""
    return np.asarray(a, np.float64).astype(NP[dtype]).astype(np.float64)


# ---- restatement ---------------------------------------------------------------------------------------------------------------------
def ref_convolve(x, h, dtype):
    """Full linear convolution by direct sums, [n + taps - 1]; x, h T-valued f64."""
    if dtype == F64 and h.size <= 256:
        return np.convolve(x.astype(np.longdouble), h.astype(np.longdouble))
    return np.convolve(x, h)


def ref_stream(chunks, h, dtype):
    """Streaming from zero history: the convolution of the concatenated chunks, cut to their length."""
    x = np.concatenate(chunks)
    return ref_convolve(x, h, dtype)[:x.size]


def fft_overlap_save(x, hist, h, P, n_out):
    """The overlap-save form in f64 np.fft with segment length P, from history `hist` (taps - 1 samples): what the kernels compute."""
    L = h.size - 1
    S = P - L
    e = np.concatenate([hist, x, np.zeros(n_out + P)])
    Hs = np.fft.fft(h, P)
    out = np.zeros(n_out + S)
    for j in range(-(-n_out // S)):
        out[j * S:(j + 1) * S] = np.fft.ifft(np.fft.fft(e[j * S:j * S + P]) * Hs).real[L:]
    return out[:n_out]


def conv_bound(x, hist, h, P, S, n_out, dtype):
    """Per output sample: the bound of the segment that owns it."""
    L = h.size - 1
    assert S == P - L and hist.size == L
    e = np.concatenate([hist, x, np.zeros(n_out + P)])
    nseg = -(-n_out // S)
    win = np.lib.stride_tricks.sliding_window_view(e, P)[::S][:nseg]  # segment j transforms e[j S, j S + P)
    norms = np.sqrt(np.einsum("ij,ij->i", win, win))
    hmax = np.abs(np.fft.fft(h, P)).max()
    return np.repeat(CB * U[dtype] * math.log2(P) * hmax * norms, S)[:n_out]


def ratio_to_bound(got, ref, bound):
    d = np.abs(np.asarray(got, np.longdouble) - ref).astype(np.float64)
    assert d.shape == bound.shape
    assert np.all(np.isfinite(d))
    zero = bound == 0.0
    assert np.all(d[zero] == 0.0), "a segment of zeros must come out as zeros"
    return float(np.max(d[~zero] / bound[~zero])) if np.any(~zero) else 0.0


def ref_deconvolve(num, den, reg, dtype):
    """(y, bound): fft_deconvolve in f64 on the T-cast inputs, and the bound above."""
    n_len, d_len = num.size, den.size
    n = 1 << max(0, (max(n_len, d_len) - 1).bit_length())
    N, D = np.fft.rfft(num, n), np.fft.rfft(den, n)
    d2 = np.abs(D) ** 2
    eps = float(NP[dtype](reg)) * d2.max()
    dd = d2 + eps
    ok = dd != 0.0
    Q = np.zeros_like(N)
    Q[ok] = N[ok] * np.conj(D[ok]) / dd[ok]
    q = np.fft.irfft(Q, n) if n > 1 else Q.real.copy()
    out_len = max(1, n_len - d_len + 1 if n_len >= d_len else n_len)
    if not ok.all():
        return q[:out_len], None
    g, r = (np.abs(D) / dd).max(), (np.abs(N) / dd).max()
    bound = CB * U[dtype] * math.log2(max(n, 2)) * (g * np.linalg.norm(num) + 3.0 * r * np.linalg.norm(den) + np.linalg.norm(q))
    return q[:out_len], bound


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def make_ir(taps, seed, dtype):
    rng = np.random.default_rng(1000 + seed)
    k = np.arange(taps)
    return tcast(rng.standard_normal(taps) * np.exp(-k / (taps / 4.0 + 1.0)), dtype)


KINDS = ("noise", "tones", "step")


def make_signal(kind, n, seed, dtype, step_at=None):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == "noise":
        x = 0.5 * rng.standard_normal(n)
    elif kind == "tones":
        x = np.sin(2 * np.pi * 0.013 * t + 0.3 * seed) + 0.3 * np.cos(2 * np.pi * 0.21 * t)
    else:  # 10^6 : 1 level step, loud first
        x = rng.standard_normal(n) * np.where(t < (n * 2 // 5 if step_at is None else step_at), 1e6, 1.0)
    return tcast(x, dtype)


def dominant_denominator(d_len, seed, dtype):
    """Decaying noise with the first tap raised by the sum of the absolute taps: min |D| / max |D| is 0.4 - 0.8."""
    rng = np.random.default_rng(2000 + seed)
    d = rng.standard_normal(d_len) * np.exp(-np.arange(d_len) / (d_len / 5.0 + 1.0))
    d[0] += np.abs(d).sum()
    return tcast(d, dtype)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_exported():
    for name in ("FirPlan", "OverlapSaveConvolver", "DeconvPlan", "fft_convolve", "fft_deconvolve"):
        assert hasattr(sg, name) and name in sg.__all__
    L = _ffi.lib()
    for s in ("sgx_fir_create", "sgx_fir_process", "sgx_fir_convolve", "sgx_fir_reset", "sgx_fir_reserve", "sgx_deconv_create",
              "sgx_deconv_execute", "sgx_deconv_output_length"):
        assert s in _ffi.SYMBOLS and hasattr(L, s)
    assert L.sgx_abi_version() == 7


def test_validation_texts():
    with pytest.raises(sg.InvalidInputError, match="impulse response must not be empty"):
        sg.FirPlan(np.zeros(0), device=_ffi.DEVICE_HOST_ONLY)
    with pytest.raises(sg.InvalidInputError, match="impulse response must not be empty"):
        sg.OverlapSaveConvolver([], 128)
    with pytest.raises(ValueError, match="route must be"):
        sg.FirPlan(np.ones(4), route="fast", device=_ffi.DEVICE_HOST_ONLY)
    with pytest.raises(ValueError, match="block_size must be > 0"):
        sg.FirPlan(np.ones(4), block_size=0, device=_ffi.DEVICE_HOST_ONLY)
    with pytest.raises(sg.FFTBackendError, match="524288"):
        sg.FirPlan(np.ones((1 << 19) + 1), device=_ffi.DEVICE_HOST_ONLY)
    with pytest.raises(sg.InvalidInputError, match="must not be empty"):
        sg.DeconvPlan(0, 4, device=_ffi.DEVICE_HOST_ONLY)
    with pytest.raises(sg.InvalidInputError, match="regularization must be finite"):
        sg.DeconvPlan(8, 4, float("nan"), device=_ffi.DEVICE_HOST_ONLY)
    # C ABI: null arguments and the create error text without a plan
    L = _ffi.lib()
    ir = (C.c_double * 2)(1.0, 2.0)
    out = C.c_void_p()
    assert L.sgx_fir_create(ir, 2, 1, 0, 7, _ffi.F32, _ffi.DEVICE_HOST_ONLY, C.byref(out)) == _ffi.SGX_INVALID_INPUT
    assert b"unknown route" in L.sgx_fir_last_error(None) and not out.value
    assert L.sgx_fir_create(ir, 2, 1, 0, 0, 5, _ffi.DEVICE_HOST_ONLY, C.byref(out)) == _ffi.SGX_INVALID_INPUT
    assert b"dtype" in L.sgx_fir_last_error(None)


def test_process_block_length_text():
    # (host-only: the length check comes before any compute)
    conv = sg.OverlapSaveConvolver.__new__(sg.OverlapSaveConvolver)
    sg.FirPlan.__init__(conv, np.ones(3), block_size=128, dtype=F32, device=_ffi.DEVICE_HOST_ONLY)
    assert conv.block_size == 128 and conv.taps == 3
    with pytest.raises(sg.InvalidInputError, match=r"process_block expects input and output of length 128 \(got 100 and 128\)"):
        conv.process_block(np.zeros(100))


def test_host_only_plan_reports_shapes_and_refuses_compute():
    p = sg.FirPlan(np.ones(5), dtype=F32, device=_ffi.DEVICE_HOST_ONLY)
    assert (p.taps, p.fft_size, p.step, p.kernel_name, p.device, p.dtype, p.block_size) == (5, 256, 252, "k_fir_os", -2, F32, None)
    text = "plan has no HIP device \\(host-only plan\\)"
    with pytest.raises(sg.FFTBackendError, match=text):
        p.process(np.zeros(16))
    with pytest.raises(sg.FFTBackendError, match=text):
        p.convolve(np.zeros((2, 16)))
    with pytest.raises(sg.FFTBackendError, match=text):
        p.reserve(2, 16)
    p.reset()  # nothing to clear
    d = sg.DeconvPlan(8, 4, dtype=F64, device=_ffi.DEVICE_HOST_ONLY)
    with pytest.raises(sg.FFTBackendError, match=text):
        d.execute(np.ones(8), np.ones(4))
    # shape errors come before the device check
    L = _ffi.lib()
    x = np.zeros(16, np.float32)
    y = np.zeros(16, np.float32)
    assert L.sgx_fir_process(p._h, x.ctypes.data, 1, 16, 16, y.ctypes.data, 15, _ffi.MEM_HOST, None) == _ffi.SGX_DIM_MISMATCH
    assert b"expected 16, got 15" in L.sgx_fir_last_error(p._h)
    assert L.sgx_fir_convolve(p._h, x.ctypes.data, 1, 16, 16, y.ctypes.data, 16, _ffi.MEM_HOST, None) == _ffi.SGX_DIM_MISMATCH
    assert b"expected 20, got 16" in L.sgx_fir_last_error(p._h)
    assert L.sgx_fir_process(p._h, x.ctypes.data, 1, 16, 8, y.ctypes.data, 16, _ffi.MEM_HOST, None) == _ffi.SGX_INVALID_INPUT


@pytest.mark.parametrize("taps,dtype,route,fft_size,name", [
    (1, F32, "auto", 256, "k_fir_os"), (3, F64, "auto", 256, "k_fir_os"), (64, F32, "auto", 256, "k_fir_os"),
    (65, F32, "auto", 512, "k_fir_os"), (200, F64, "auto", 1024, "k_fir_os"), (512, F32, "auto", 2048, "k_fir_os"),
    (1025, F64, "auto", 4096, "k_fir_os"), (2049, F32, "auto", 4096, "k_fir_os"), (2050, F32, "auto", 8192, "fir_generic"),
    (5000, F64, "auto", 16384, "fir_generic"), (40000, F32, "auto", 131072, "fir_generic"), (1 << 19, F64, "auto", 1 << 20, "fir_generic"),
    (1, F32, "generic", 256, "fir_generic"), (200, F32, "generic", 512, "fir_generic"), (2049, F64, "generic", 8192, "fir_generic"),
])
def test_route_table(taps, dtype, route, fft_size, name):
    p = sg.FirPlan(np.ones(taps), dtype=dtype, route=route, device=_ffi.DEVICE_HOST_ONLY)
    assert (p.fft_size, p.step, p.kernel_name, p.taps) == (fft_size, fft_size - (taps - 1), name, taps)
    assert p.taps - 1 <= p.fft_size // 2 and p.step >= 1


@pytest.mark.parametrize("n_len,d_len,out_len,n", [(4159, 64, 4096, 8192), (31999, 2000, 30000, 32768), (1000, 1000, 1, 1024),
                                                   (100, 300, 100, 512), (1, 1, 1, 1), (1, 7, 1, 8), (5, 1, 5, 8)])
def test_deconvolution_output_length_table(n_len, d_len, out_len, n):
    d = sg.DeconvPlan(n_len, d_len, device=_ffi.DEVICE_HOST_ONLY)
    assert d.output_length == out_len
    y, _ = ref_deconvolve(np.ones(n_len), np.ones(d_len), 0.5, F64)
    assert y.size == out_len and 1 << (max(n_len, d_len) - 1).bit_length() == n


@pytest.mark.parametrize("taps,P", [(1, 256), (3, 256), (200, 1024), (200, 512), (1025, 4096)])
def test_restatement_fft_form_matches_direct_sums(taps, P):
    h = make_ir(taps, 0, F64)
    for kind in KINDS:
        x = make_signal(kind, 3 * P + 17, 5, F64)
        hist = make_signal("noise", taps - 1, 6, F64)
        full = ref_convolve(np.concatenate([hist, x]), h, F64)[taps - 1:taps - 1 + x.size]  # streaming from `hist`
        y = fft_overlap_save(x, hist, h, P, x.size)
        b = conv_bound(x, hist, h, P, P - (taps - 1), x.size, F64)
        assert ratio_to_bound(y, full, b) < 0.1  # f64 np.fft against long double sums, per segment
        tail = fft_overlap_save(x, np.zeros(taps - 1), h, P, x.size + taps - 1)
        assert np.allclose(tail, np.asarray(ref_convolve(x, h, F64), np.float64), rtol=0, atol=1e-9 * np.abs(x).max() * np.abs(h).sum())


def test_restatement_chunked_equals_whole():
    h = make_ir(64, 1, F32)
    x = make_signal("tones", 5000, 2, F32)
    whole = np.asarray(ref_stream([x], h, F32), np.float64)
    cuts = [0, 1, 8, 70, 71, 1000, 1003, 5000]
    hist = np.zeros(63)
    parts = []
    for a, b in zip(cuts, cuts[1:]):
        parts.append(fft_overlap_save(x[a:b], hist, h, 256, b - a))
        hist = np.concatenate([hist, x[a:b]])[-63:]  # a chunk shorter than taps - 1 shifts the old history
    assert np.allclose(np.concatenate(parts), whole, rtol=0, atol=1e-11)


def test_reference_deconvolution_case_in_the_restatement():
    x = np.array([1.0, 0.7, -0.3, 0.2, 0.9, -0.5, 0.1, 0.4])
    h = np.array([0.0, 0.0, 1.0, 0.5])
    y, _ = ref_deconvolve(np.convolve(x, h), x, 0.0, F64)
    assert y.size == 4 and np.max(np.abs(y - h)) < 1e-6  # src/convolution.rs:297-316
    z, b = ref_deconvolve(np.ones(8), np.zeros(4), 0.0, F64)
    assert b is None and np.all(z == 0.0)


@pytest.mark.parametrize("d_len", [64, 1000, 2000])
def test_dominant_denominator_meets_the_condition(d_len):
    D = np.abs(np.fft.rfft(dominant_denominator(d_len, 3, F32), 1 << (d_len - 1).bit_length()))
    assert D.min() >= 0.1 * D.max()


# ---- GPU: parity ------------------------------------------------------------------------------------------------------------------------
def _lengths(taps, S, batch):
    """Ragged lengths: shorter than taps - 1, shorter than S, a few segments, not a multiple of anything; capped by the reference's cost."""
    want = [max(1, taps - 2), max(1, S - 1), S + 1, 2 * S + 17, 5 * S + 3]
    cap = max(1, int(MAC_CAP / (batch * taps)))
    return sorted({min(n, cap) for n in want})


def _check_call(plan, hs, x, form, dtype, name):
    """One call on host arrays x [batch][n] from zero history against the restatement, every sample."""
    P, S, taps = plan.fft_size, plan.step, plan.taps
    got = (plan.process if form == "process" else plan.convolve)(x.astype(NP[dtype]))
    n_out = x.shape[1] + (taps - 1 if form == "convolve" else 0)
    assert got.shape == (x.shape[0], n_out) and got.dtype == NP[dtype]
    worst = 0.0
    for r in range(x.shape[0]):
        h = hs[r if hs.shape[0] > 1 else 0]
        ref = ref_convolve(x[r], h, dtype)[:n_out]
        worst = max(worst, ratio_to_bound(got[r], ref, conv_bound(x[r], np.zeros(taps - 1), h, P, S, n_out, dtype)))
    _record(name, worst)
    assert worst <= 1.0, (name, form, x.shape, worst)


PARITY = [(t, r) for t in FUSED_TAPS for r in ("auto", "generic")] + [(t, "auto") for t in GENERIC_ONLY_TAPS]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("taps,route", PARITY, ids=[f"{t}-{r}" for t, r in PARITY])
def test_gpu_parity(taps, route, dtype):
    shared = np.stack([make_ir(taps, 0, dtype)])
    per_row = np.stack([make_ir(taps, 10 + r, dtype) for r in range(5)])
    p1 = sg.FirPlan(shared[0], dtype=dtype, route=route)
    p5 = sg.FirPlan(per_row, dtype=dtype, route=route)
    assert p1.kernel_name == ("k_fir_os" if route == "auto" and taps <= 2049 else "fir_generic")
    S = p1.step
    name = f"{p1.kernel_name}-{dtype}"
    k = 0
    for n in _lengths(taps, S, 1):  # batch 1, one response
        for form in ("process", "convolve"):
            p1.reset()
            _check_call(p1, shared, make_signal(KINDS[k % 3], n, k, dtype, step_at=n // 2 + 7)[None], form, dtype, name)
            k += 1
    if taps == 40000:  # the long generic route over more than one segment (above the cost cap: one case)
        p1.reset()
        _check_call(p1, shared, make_signal("step", S + 1000, 99, dtype)[None], "process", dtype, name)
    for n in _lengths(taps, S, 5)[::2]:  # batch 5, a response per row, every kind of input in the batch
        x = np.stack([make_signal(KINDS[r % 3], n, 20 + r, dtype) for r in range(5)])
        for form in ("process", "convolve"):
            p5.reset()
            _check_call(p5, per_row, x, form, dtype, name)
    n = _lengths(taps, S, 64)[-1]  # batch 64, one response
    x = np.stack([make_signal(KINDS[r % 3], n, 40 + r, dtype) for r in range(64)])
    for form in ("process", "convolve"):
        p1.reset()
        _check_call(p1, shared, x, form, dtype, name)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
def test_gpu_level_step_inside_every_other_segment(dtype):
    """The step right behind the start of segments 1, 2 and 3 in turn: whichever way segments might share a transform, one of these
    puts a loud and a quiet one together."""
    taps = 200
    h = np.stack([make_ir(taps, 3, dtype)])
    for route in ("auto", "generic"):
        plan = sg.FirPlan(h[0], dtype=dtype, route=route)
        S = plan.step
        for j in (1, 2, 3):
            plan.reset()
            x = make_signal("step", 8 * S, 60 + j, dtype, step_at=j * S + 100)[None]
            _check_call(plan, h, x, "process", dtype, f"{plan.kernel_name}-{dtype}-step")


@pytest.mark.gpu
@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per_row"])
def test_gpu_generic_route_across_a_scratch_chunk_boundary(per_row):
    """f64, 3 taps on the generic route: P = 256, so a 256 MB chunk of scratch holds 65536 segments; 5 rows of 14 001 segments are two
    chunks with the boundary inside the last row (one response: the product fused into the forward store; per row: k_fir_mul)."""
    taps, batch = 3, 5
    hs = np.stack([make_ir(taps, 50 + r, F64) for r in range(batch if per_row else 1)])
    plan = sg.FirPlan(hs if per_row else hs[0], dtype=F64, route="generic")
    P, S = plan.fft_size, plan.step
    assert (P, S) == (256, 254) and batch * 14001 > (256 << 20) // (P * 16) > 4 * 14001
    n = 14000 * S + 17
    x = np.stack([make_signal(KINDS[r % 3], n, 300 + r, F64) for r in range(batch)])
    for form in ("process", "convolve"):
        plan.reset()
        _check_call(plan, hs, x, form, F64, "fir_generic-float64-chunks")


# ---- GPU: streaming -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("taps,route", [(200, "auto"), (200, "generic"), (1025, "auto"), (2050, "auto")])
def test_gpu_streaming_chunks_equal_one_call(taps, route, dtype):
    batch = 3
    hs = np.stack([make_ir(taps, 30 + r, dtype) for r in range(batch)])
    plan = sg.FirPlan(hs, dtype=dtype, route=route)
    P, S, L = plan.fft_size, plan.step, taps - 1
    sizes = [1, 7, taps - 2, S, S + 1, 4096]
    order = [3, 0, 5, 2, 1, 4, 0, 0, 2, 4, 1, 5, 3]  # mixed, the short ones after one another too
    chunks = [sizes[i] for i in order]
    total = sum(chunks)
    x = np.stack([make_signal(KINDS[r % 3], total, 70 + r, dtype) for r in range(batch)])
    one = sg.FirPlan(hs, dtype=dtype, route=route).process(x.astype(NP[dtype]))
    refs = [ref_stream([x[r]], hs[r], dtype) for r in range(batch)]
    b_one = np.stack([conv_bound(x[r], np.zeros(L), hs[r], P, S, total, dtype) for r in range(batch)])
    got, b_chunk, at = [], [], 0
    for c in chunks:
        got.append(plan.process(x[:, at:at + c].astype(NP[dtype])))
        hist = np.concatenate([np.zeros((batch, L)), x[:, :at]], axis=1)[:, at:at + L]  # the last L samples before `at`
        b_chunk.append(np.stack([conv_bound(x[r, at:at + c], hist[r], hs[r], P, S, c, dtype) for r in range(batch)]))
        at += c
    got, b_chunk = np.concatenate(got, axis=1), np.concatenate(b_chunk, axis=1)
    name = f"{plan.kernel_name}-{dtype}-stream"
    worst = max(ratio_to_bound(got[r], refs[r], b_chunk[r]) for r in range(batch))
    _record(name, worst)
    assert worst <= 1.0
    d = np.abs(got.astype(np.float64) - one.astype(np.float64))
    assert np.all(d <= b_chunk + b_one), float(np.max(d / np.maximum(b_chunk + b_one, 1e-300)))
    # reset restores the zero-history result bit for bit
    plan.reset()
    again = plan.process(x.astype(NP[dtype]))
    assert again.tobytes() == one.tobytes()
    # the history's rows are fixed until the next reset
    with pytest.raises(sg.DimensionMismatchError, match=f"expected {batch}, got 1"):
        _changed_batch(hs[0], dtype, route, batch)


def _changed_batch(h, dtype, route, batch):
    plan = sg.FirPlan(h, dtype=dtype, route=route)
    plan.process(np.zeros((batch, 50), NP[dtype]))
    plan.convolve(np.zeros((1, 50), NP[dtype]))  # the stateless form is free of the history's rows
    try:
        plan.process(np.zeros((1, 50), NP[dtype]))
    finally:
        plan.reset()
        assert plan.process(np.zeros((1, 50), NP[dtype])).shape == (1, 50)  # free again after reset


# ---- GPU: the reference's own unit tests through the engine (src/convolution.rs:281-385, their tolerances) ------------------------------
@pytest.mark.gpu
def test_gpu_reference_unit_impulse_shifts_the_input():
    out = sg.fft_convolve([1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 1.0])
    assert out.dtype == np.float64 and out.shape == (6,)
    assert np.max(np.abs(out - [0.0, 0.0, 1.0, 2.0, 3.0, 4.0])) < 1e-9


@pytest.mark.gpu
def test_gpu_reference_small_convolution_matches_direct():
    a, b = [1.0, -2.0, 0.5], [0.25, 1.0, -0.5, 2.0]
    out = sg.fft_convolve(a, b)
    assert out.shape == (6,) and np.max(np.abs(out - np.convolve(a, b))) < 1e-9
    assert np.max(np.abs(sg.fft_convolve(b, a) - np.convolve(a, b))) < 1e-9  # the shorter operand is the response either way
    both = sg.fft_convolve(np.stack([a, a]), np.stack([b, np.multiply(b, 2.0)]))
    assert np.max(np.abs(both - np.stack([np.convolve(a, b), 2.0 * np.convolve(a, b)]))) < 1e-9


@pytest.mark.gpu
def test_gpu_reference_overlap_save_streaming_case():
    taps, total, block = 200, 1024, 128
    k = np.arange(taps, dtype=np.float32)
    ir = (np.sin(k * np.float32(0.13)) * np.exp(-k / np.float32(60.0))).astype(np.float32)
    n = np.arange(total, dtype=np.float32)
    x = (np.sin(n * np.float32(0.05)) + np.float32(0.3) * np.cos(n * np.float32(0.21))).astype(np.float32)
    conv = sg.OverlapSaveConvolver(ir, block, dtype=F32)
    assert conv.block_size == block and conv.fft_size == 1024 and conv.kernel_name == "k_fir_os"
    got = np.concatenate([conv.process_block(x[s:s + block]) for s in range(0, total, block)])
    want = np.convolve(x.astype(np.float64), ir.astype(np.float64))[:total]
    assert got.dtype == np.float32 and np.max(np.abs(got - want)) < 1e-3
    conv.reset()
    assert conv.process_block(x[:block]).tobytes() == got[:block].tobytes()
    with pytest.raises(sg.InvalidInputError, match=r"length 128 \(got 127 and 128\)"):
        conv.process_block(x[:127])


@pytest.mark.gpu
def test_gpu_reference_deconvolution_recovers_the_response():
    x = [1.0, 0.7, -0.3, 0.2, 0.9, -0.5, 0.1, 0.4]
    h = [0.0, 0.0, 1.0, 0.5]
    y = sg.fft_convolve(x, h)
    rec = sg.fft_deconvolve(y, x, 0.0)
    assert rec.shape == (4,) and np.max(np.abs(rec - h)) < 1e-6


# ---- GPU: deconvolution ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("reg", [0.0, 1e-6, 1e-3])
@pytest.mark.parametrize("n_len,d_len", [(4159, 64), (31999, 2000), (1000, 1000), (100, 300)])
def test_gpu_deconvolution_parity(n_len, d_len, reg, dtype):
    for batch in (1, 16):
        dens = np.stack([dominant_denominator(d_len, 7 * r, dtype) for r in range(batch)])
        if n_len >= d_len:  # the full convolution of an excitation with the denominator, plus a little noise
            nums = np.stack([np.convolve(make_signal(KINDS[r % 2], n_len - d_len + 1, r, dtype), dens[r]) for r in range(batch)])
            nums = tcast(nums + 1e-3 * np.random.default_rng(n_len + batch).standard_normal(nums.shape), dtype)
        else:
            nums = np.stack([make_signal("noise", n_len, 50 + r, dtype) for r in range(batch)])
        n = 1 << (max(n_len, d_len) - 1).bit_length()
        for r in range(batch):  # the condition on the inputs, before the GPU is touched
            D = np.abs(np.fft.rfft(dens[r], n))
            assert D.min() >= 0.1 * D.max() or reg >= 1e-3
        refs = [ref_deconvolve(nums[r], dens[r], reg, dtype) for r in range(batch)]
        plan = sg.DeconvPlan(n_len, d_len, reg, dtype)
        got = plan.execute(nums.astype(NP[dtype]), dens.astype(NP[dtype]))
        assert got.shape == (batch, plan.output_length) and got.dtype == NP[dtype]
        worst = 0.0
        for r in range(batch):
            y, bound = refs[r]
            worst = max(worst, float(np.max(np.abs(got[r].astype(np.float64) - y))) / bound)
        _record(f"deconv-{dtype}", worst)
        assert worst <= 1.0, (n_len, d_len, reg, batch, worst)
        if batch == 1:  # the one-shot function, and one denominator for every row
            one = sg.fft_deconvolve(nums[0], dens[0], reg, dtype=dtype)
            assert one.tobytes() == got[0].tobytes()
        else:
            shared = plan.execute(nums.astype(NP[dtype]), dens[3].astype(NP[dtype]))
            assert shared[3].tobytes() == got[3].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n_len", [(F32, 30000), (F64, 16000), (F32, 100000), (F64, 100000)])
def test_gpu_deconvolution_past_the_on_chip_inverse_tile(dtype, n_len):
    """n = 32768 in f32 and 16384 in f64 are the lengths whose forward transform runs in LDS while the inverse rows go through global
    memory; 131072 runs both ways there."""
    den = dominant_denominator(500, 11, dtype)
    num = tcast(np.convolve(make_signal("tones", n_len - 499, 12, dtype), den), dtype)
    y, bound = ref_deconvolve(num, den, 1e-6, dtype)
    got = sg.fft_deconvolve(num, den, 1e-6, dtype=dtype)
    ratio = float(np.max(np.abs(got.astype(np.float64) - y))) / bound
    _record(f"deconv-{dtype}", ratio)
    assert got.shape == y.shape and ratio <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n_len,d_len", [(1, 1), (2, 1), (1, 7), (5, 1), (3, 3)])
def test_gpu_deconvolution_of_the_shortest_inputs(n_len, d_len, dtype):
    """Transforms of 1, 2, 4 and 8 points (the plan's n_fft goes down to 1)."""
    num = tcast(np.arange(1, n_len + 1) * 0.75, dtype)
    den = dominant_denominator(d_len, 5, dtype)
    y, bound = ref_deconvolve(num, den, 1e-3, dtype)
    got = sg.fft_deconvolve(num, den, 1e-3, dtype=dtype)
    assert got.shape == y.shape and np.max(np.abs(got.astype(np.float64) - y)) <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
def test_gpu_deconvolution_zero_denominator_gives_zeros(dtype):
    num = make_signal("noise", 500, 1, dtype)
    for reg in (0.0, 1e-3):
        out = sg.fft_deconvolve(np.stack([num, num]), np.zeros(100), reg, dtype=dtype)
        assert out.shape == (2, 401) and np.all(out == 0.0)


# ---- GPU: stream order, capture, repeatability ----------------------------------------------------------------------------------------
STREAM_ROWS = [(200, "auto", F32), (1025, "auto", F64), (200, "generic", F32), (5000, "auto", F64)]
STREAM_IDS = [f"{t}-{r}-{d}" for t, r, d in STREAM_ROWS]
SENTINEL = -1.2345678e30


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a.astype(NP[dtype]))).cuda()


def _same(a, b):
    import torch
    it = torch.int32 if a.element_size() == 4 else torch.int64
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _stream_case(taps, route, dtype, batch=4):
    hs = make_ir(taps, 80, dtype)
    n = 3 * sg.FirPlan(hs, dtype=dtype, route=route, device=_ffi.DEVICE_HOST_ONLY).step + 41
    xs = [np.stack([make_signal(KINDS[(r + k) % 3], n, 90 + 10 * k + r, dtype) for r in range(batch)]) for k in range(3)]
    return hs, n, [_dev(x, dtype) for x in xs]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["process", "convolve"])
@pytest.mark.parametrize("taps,route,dtype", STREAM_ROWS, ids=STREAM_IDS)
def test_gpu_call_is_one_operation_of_the_side_stream(taps, route, dtype, form):
    """Behind a producer of >= 10 ms on a side stream whose last operation writes the samples, with NaN inputs and a sentinel output
    until then: the result equals the default-stream result of a fresh plan, and nothing is written after the work queued behind it."""
    import torch
    hs, n, xs = _stream_case(taps, route, dtype)
    call = lambda plan, x, out=None: getattr(plan, form + "_torch")(x, out)  # noqa: E731
    ref = call(sg.FirPlan(hs, dtype=dtype, route=route), xs[0])
    torch.cuda.synchronize()
    plan = sg.FirPlan(hs, dtype=dtype, route=route)
    plan.reserve(xs[0].shape[0], n, host_staging=False)
    xin = torch.full_like(xs[0], float("nan"))
    out = torch.full_like(ref, SENTINEL)
    from tests.test_stream_order import producer
    big, ops = producer()  # in-place additions on a 1 GiB buffer, about 25 ms of them
    side = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        e0.record()
        for _ in range(ops):
            big.add_(1.0)
        xin.copy_(xs[0])
        e1.record()
        call(plan, xin, out)
        snap = out.clone()
        out.fill_(SENTINEL)
    done_at_return = e1.query()
    torch.cuda.synchronize()
    print(f"producer {e0.elapsed_time(e1):.1f} ms, done when the host returned from the call: {done_at_return}")
    assert _same(snap, ref), "the result queued behind the producer differs from the default-stream result"
    assert torch.all(out == SENTINEL), "something wrote the output after the work queued behind the call"
    assert e0.elapsed_time(e1) >= 10.0 and done_at_return is False, "no hazard window was shown"


@pytest.mark.gpu
@pytest.mark.parametrize("taps,route,dtype", STREAM_ROWS, ids=STREAM_IDS)
def test_gpu_reserved_streaming_call_is_captured_and_replayed(taps, route, dtype):
    """After reserve a streaming call allocates nothing, synchronises nothing and names the same buffers every time: captured once as a
    linear chain on a side stream, its replays on new chunks continue the stream — the history moves on under replay."""
    import torch
    hs, n, xs = _stream_case(taps, route, dtype)
    eager = sg.FirPlan(hs, dtype=dtype, route=route)
    refs = [eager.process_torch(x) for x in xs]  # one stream of three chunks (also loads every code object the call launches)
    torch.cuda.synchronize()
    plan = sg.FirPlan(hs, dtype=dtype, route=route)
    plan.reserve(xs[0].shape[0], n, host_staging=False)
    xin = xs[0].clone()
    out = torch.full_like(refs[0], SENTINEL)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.process_torch(xin, out)
    for k in range(3):
        xin.copy_(xs[k])
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out, refs[k]), f"replay {k} differs from the eager stream's chunk {k}"


@pytest.mark.gpu
@pytest.mark.parametrize("taps,route,dtype", STREAM_ROWS, ids=STREAM_IDS)
def test_gpu_repeated_calls_on_a_fresh_plan_are_bit_equal(taps, route, dtype):
    import torch
    hs, n, xs = _stream_case(taps, route, dtype)
    plan = sg.FirPlan(hs, dtype=dtype, route=route)
    a = plan.convolve_torch(xs[0])
    plan.process_torch(xs[1])  # a streaming call in between changes nothing for the stateless form
    b = plan.convolve_torch(xs[0])
    host = plan.convolve(xs[0].cpu().numpy())
    torch.cuda.synchronize()
    assert _same(a, b) and host.tobytes() == a.cpu().numpy().tobytes()
    first = sg.FirPlan(hs, dtype=dtype, route=route).process_torch(xs[0])
    second = sg.FirPlan(hs, dtype=dtype, route=route).process_torch(xs[0])
    torch.cuda.synchronize()
    assert _same(first, second)


@pytest.mark.gpu
@pytest.mark.parametrize("taps,route,dtype", STREAM_ROWS, ids=STREAM_IDS)
def test_gpu_reset_is_one_operation_of_the_side_stream(taps, route, dtype):
    """sgx_fir_reset on a side stream, between two streaming calls there and behind the producer: the second call starts from zero
    history (the bits of a fresh plan), so the zeroing ran after the first call's history update and before the second call's reads."""
    import torch
    from tests.test_stream_order import producer
    hs, n, xs = _stream_case(taps, route, dtype)
    ref = sg.FirPlan(hs, dtype=dtype, route=route).process_torch(xs[1])
    carried = sg.FirPlan(hs, dtype=dtype, route=route)
    carried.process_torch(xs[0])
    not_reset = carried.process_torch(xs[1])
    torch.cuda.synchronize()
    assert not _same(not_reset, ref)  # the history matters for this input
    plan = sg.FirPlan(hs, dtype=dtype, route=route)
    plan.reserve(xs[0].shape[0], n, host_staging=False)
    big, ops = producer()
    side = torch.cuda.Stream()
    e1 = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(ops):
            big.add_(1.0)
        e1.record()
        plan.process_torch(xs[0])
        plan.reset()  # torch's current stream: the side stream
        out = plan.process_torch(xs[1])
    done_at_return = e1.query()
    torch.cuda.synchronize()
    assert _same(out, ref) and done_at_return is False


DECONV_ROWS = [(4159, 64, F32), (31999, 2000, F64), (30000, 500, F32), (100, 300, F64)]
DECONV_IDS = [f"{a}-{b}-{d}" for a, b, d in DECONV_ROWS]


def _deconv_case(n_len, d_len, dtype, batch=4):
    dens = np.stack([dominant_denominator(d_len, 3 * r, dtype) for r in range(batch)])
    nums = [np.stack([make_signal(KINDS[(r + k) % 2], n_len, 500 + 10 * k + r, dtype) for r in range(batch)]) for k in range(3)]
    return dens, nums


@pytest.mark.gpu
@pytest.mark.parametrize("den_rows", [1, 4])
@pytest.mark.parametrize("n_len,d_len,dtype", DECONV_ROWS, ids=DECONV_IDS)
def test_gpu_deconvolution_device_call_on_a_side_stream_and_captured(n_len, d_len, dtype, den_rows):
    """sgx_deconv_execute on device pointers: the bits of the host path; one operation of a side stream behind a producer whose last
    operation writes the numerators; and after reserve captured as a linear chain and replayed on new numerators."""
    import torch
    from tests.test_stream_order import producer
    dens, nums = _deconv_case(n_len, d_len, dtype)
    dens = dens[:den_rows]
    host_plan = sg.DeconvPlan(n_len, d_len, 1e-6, dtype)
    refs = [host_plan.execute(x.astype(NP[dtype]), (dens if den_rows > 1 else dens[0]).astype(NP[dtype])) for x in nums]
    dden, dnums = _dev(dens, dtype), [_dev(x, dtype) for x in nums]
    eager = host_plan.execute_torch(dnums[0], dden)  # (also loads every code object the call launches)
    torch.cuda.synchronize()
    assert eager.cpu().numpy().tobytes() == refs[0].tobytes()
    # A: behind a producer on a side stream, NaN numerators and a sentinel output until then
    plan = sg.DeconvPlan(n_len, d_len, 1e-6, dtype)
    plan.reserve(4, den_rows, host_staging=False)
    xin = torch.full_like(dnums[0], float("nan"))
    out = torch.full_like(eager, SENTINEL)
    big, ops = producer()
    side = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        e0.record()
        for _ in range(ops):
            big.add_(1.0)
        xin.copy_(dnums[1])
        e1.record()
        plan.execute_torch(xin, dden, out)
        snap = out.clone()
        out.fill_(SENTINEL)
    done_at_return = e1.query()
    torch.cuda.synchronize()
    assert snap.cpu().numpy().tobytes() == refs[1].tobytes(), "the result queued behind the producer differs from the host path's"
    assert torch.all(out == SENTINEL), "something wrote the output after the work queued behind the call"
    assert e0.elapsed_time(e1) >= 10.0 and done_at_return is False, "no hazard window was shown"
    # B: a fresh plan, reserved, captured once and replayed
    plan = sg.DeconvPlan(n_len, d_len, 1e-6, dtype)
    plan.reserve(4, den_rows, host_staging=False)
    xin = dnums[0].clone()
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.execute_torch(xin, dden, out)
    for k in (2, 1, 0):
        xin.copy_(dnums[k])
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == refs[k].tobytes(), f"replay on input {k} differs from the host path's result"


# Every prototype of the FIR / deconvolution families that takes a stream, and the test above that puts it on a side stream.  (The
# header scan of tests/test_stream_order.py keys on its own table of rows; these entry points are covered here instead.)
STREAM_COVERAGE = {
    "sgx_fir_process": "test_gpu_call_is_one_operation_of_the_side_stream",
    "sgx_fir_convolve": "test_gpu_call_is_one_operation_of_the_side_stream",
    "sgx_fir_reset": "test_gpu_reset_is_one_operation_of_the_side_stream",
    "sgx_deconv_execute": "test_gpu_deconvolution_device_call_on_a_side_stream_and_captured",
}


def test_every_stream_taking_prototype_of_the_new_families_has_a_stream_test():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectro_hip.h")).read()
    found = {m.group(1) for m in re.finditer(r"\bsgx_status\s+(sgx_(?:fir|deconv)_\w+)\s*\(([^;{]*?)\)\s*;", hdr, re.S)
             if re.search(r"void\s*\*\s*(?:hip_)?stream\b", m.group(2))}
    assert found == set(STREAM_COVERAGE), found ^ set(STREAM_COVERAGE)
    for name, test in STREAM_COVERAGE.items():
        fn = globals()[test]
        assert any(mark.name == "gpu" for mark in getattr(fn, "pytestmark", [])), test
    # the Python layer hands every one of them torch's current stream (through the stream helper of the plans' shared base, which fetches it)
    src = open(os.path.join(os.path.dirname(_ffi.__file__), "fir.py")).read()
    base = open(os.path.join(os.path.dirname(_ffi.__file__), "_handle.py")).read()
    for name in STREAM_COVERAGE:
        assert name in src and "self._stream()" in src and "current_stream" in base
