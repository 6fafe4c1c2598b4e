"""Minimum-phase plans (minimum_phase, minimum_phase_with, MinPhasePlan) against a NumPy f64 restatement of src/min_phase.rs.  Every
output sample of every row is compared; nothing is left out.

Restatement, `ref(h, out_len, oversample, dtype)`: the reference's algorithm with np.fft in f64 on the T-cast input (the plans compute in
f64 for both dtypes: include/spectro_hip.h).  With n = next_power_of_two(taps max(oversample, 1)):
    H = FFT_n(h);  eps = 1e-20 max |H_k|^2 (1e-300 if 0);  L_k = 0.5 ln(|H_k|^2 + eps);  c = IFFT_n(L);  C = FFT_n(w c), w the fold
    weights (1 at 0 and n / 2, 2 between, 0 above; [1] for n = 1, [1, 1] for n = 2);  Hmin = exp(C);  y = Re IFFT_n(Hmin)[:min(out_len, n)]

Bound B, first order, u = 2^-53 for both dtypes, c = 4 (tests/test_fir.py's CB), lg = log2(max(n, 2)):
    eF   = c u lg ||H||_2                                        the forward transform, normwise
    a_k  = sqrt(|H_k|^2 + eps)
    dL_k = eF / a_k + eF / max|H| + u (2 + |L_k|)                the bin's own error, the error of eps through the maximum, the log
    dC   = circular_convolution(|FFT(w)| / n, dL) + 4 c u lg ||L||_2    the inverse, the fold and the forward transform of the cepstrum
    dH_k = |Hmin_k| (expm1(dC_k) + u (4 + |Re C_k| + |Im C_k|))  the exp, sin and cos and their argument reduction
    B    = ||dH||_2 / sqrt(n) + c u lg ||Hmin||_2 / sqrt(n),  plus 2^-24 |y_i| per sample for f32 plans (the one rounding to T)
and the assertion is |got_i - y_i| <= B.  An all-zero row has no max |H| to scale by; it is held to its own criterion instead: f64
finite with |y| < 1e-100 (y_0 = sqrt(1e-300)), f32 exact zeros.  The Hann-windowed low-pass of 1 and of 2 taps is such a row (the window is
zero at both ends).

What the bound amounts to, over the shapes below (asserted in test_bound_over_peak...): B / peak <= 5e-11 on the decaying-noise, noise
and impulse inputs and <= 3e-3 on the low-passes, where the spectral nulls dominate (7.6e-7 .. 2.9e-3 from 64 taps on).  An f32 restatement
(radix-2 complex64 transforms) stays at <= 0.012 of the u = 2^-24 form of the bound.  The f64 bound is sharp enough to catch a wrong
fold weight, a missing eps, a wrong 1 / n and an off-by-one at n / 2 (test_bound_catches_the_usual_mistakes).
"""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi

F32, F64 = "float32", "float64"
NP = {F32: np.float32, F64: np.float64}
U53 = 2.0 ** -53
CB = 4.0
WORST = {}
KINDS = ("decay", "noise", "lowpass", "impulse")
FUSED = [(1, 1), (2, 1), (5, 8), (64, 8), (200, 8), (512, 8), (64, 1), (4096, 1)]
# the remaining transform lengths of k_minphase, n = 4, 8, 16, 32, 128, 256, 1024 (run by tests/test_instance_census.py)
SHORT_FUSED = [(3, 1), (4, 1), (7, 1), (13, 1), (2, 8), (29, 1), (4, 8), (16, 8), (100, 1), (32, 8), (128, 8), (1000, 1)]
GENERIC = [(513, 8), (3000, 8)]
FORCED = [(64, 8), (200, 8), (512, 8)]
PARITY = [(t, o, "auto") for t, o in FUSED + GENERIC] + [(t, o, "generic") for t, o in FORCED]
SEEDS = (7, 8, 9)  # batch 3: one seed per row


def _record(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    print(f"{name}: worst ratio to bound {WORST[name]:.3g}")


def tcast(a, dtype):
    """The T-valued input, widened to f64."""
    return np.asarray(a, np.float64).astype(NP[dtype]).astype(np.float64)


def fft_len(taps, oversample):
    return 1 << max(0, (taps * max(oversample, 1) - 1).bit_length())


def fold_weights(n):
    w = np.zeros(n)
    w[0] = 1.0
    if n > 1:
        w[n // 2] = 1.0
        w[1:n // 2] = 2.0
    return w


# ---- restatement ---------------------------------------------------------------------------------------------------------------------
def pipeline(h, oversample, mistake=None):
    """The algorithm in f64 np.fft on the f64 row h: every intermediate.  `mistake` plants one of the errors the bound must catch."""
    n = fft_len(h.size, oversample)
    H = np.fft.fft(h, n)
    m2 = np.abs(H) ** 2
    mx = m2.max()
    eps = mx * 1e-20 if mx > 0 else 1e-300
    if mistake == "no_eps":
        eps = 1e-300
    L = 0.5 * np.log(m2 + eps)
    c = np.fft.ifft(L).real
    if mistake == "one_over_n":
        c = c * n / (n + 1.0)
    w = fold_weights(n)
    if mistake == "fold_weight" and n > 2:
        w[1] = 1.0
    if mistake == "nyquist_doubled" and n > 1:
        w[n // 2] = 2.0
    if mistake == "nyquist_dropped" and n > 2:
        w[n // 2] = 0.0
        w[n // 2 - 1] = 1.0
    Cs = np.fft.fft(c * w)
    Hm = np.exp(Cs)
    y = np.fft.ifft(Hm).real
    return dict(n=n, H=H, m2=m2, mx=mx, eps=eps, L=L, w=w, C=Cs, Hm=Hm, y=y)


def bound_of(p, u):
    """The scalar part of B (without the f32 output rounding) from the restatement's intermediates."""
    n, H, L, Hm, Cs = p["n"], p["H"], p["L"], p["Hm"], p["C"]
    lg = math.log2(max(n, 2))
    eF = CB * u * lg * np.linalg.norm(H)
    a = np.sqrt(p["m2"] + p["eps"])
    dL = eF / a + eF / math.sqrt(p["mx"]) + u * (2.0 + np.abs(L))
    wh = np.abs(np.fft.fft(p["w"])) / n
    dC = np.fft.ifft(np.fft.fft(wh) * np.fft.fft(dL)).real + 4.0 * CB * u * lg * np.linalg.norm(L)
    with np.errstate(over="ignore"):
        dH = np.abs(Hm) * (np.expm1(dC) + u * (4.0 + np.abs(Cs.real) + np.abs(Cs.imag)))
        return float(np.linalg.norm(dH) / math.sqrt(n) + CB * u * lg * np.linalg.norm(Hm) / math.sqrt(n))


def ref(h, out_len, oversample, dtype):
    """(y, B): the restatement on the T-cast row and the per-sample bound; B is None for an all-zero row."""
    p = pipeline(tcast(h, dtype), oversample)
    y = p["y"][:min(out_len, p["n"])]
    if p["mx"] == 0.0:
        return y, None
    B = np.full(y.shape, bound_of(p, U53))
    if dtype == F32:
        B = B + 2.0 ** -24 * np.abs(y)
    return y, B


# ---- inputs, seeded --------------------------------------------------------------------------------------------------------------------
def lowpass(taps, fc=0.15, hann=True):
    """The reference's own test filters (src/min_phase.rs:160-177, :196-208): a sinc of cutoff fc, Hann-windowed in the first."""
    k = np.arange(taps)
    x = k - (taps - 1) / 2.0
    s = np.where(np.abs(x) < 1e-9, 2.0 * fc, np.sin(2.0 * np.pi * fc * x) / (np.pi * np.where(np.abs(x) < 1e-9, 1.0, x)))
    return s * (0.5 - 0.5 * np.cos(2.0 * np.pi * k / max(taps - 1, 1))) if hann else s


def make_ir(kind, taps, seed):
    rng = np.random.default_rng(seed)
    k = np.arange(taps)
    if kind == "decay":
        return np.exp(-k / (taps / 6.0)) * rng.standard_normal(taps)
    if kind == "noise":
        return rng.standard_normal(taps)
    if kind == "lowpass":
        return lowpass(taps)
    h = np.zeros(taps)
    h[taps // 2] = 1.0
    return h


@functools.lru_cache(maxsize=None)
def case(kind, taps, oversample, dtype, out_len=None, seeds=SEEDS):
    """The rows of one parity case, their restatement and bounds: computed once, shared, not written to."""
    rows = np.stack([tcast(make_ir(kind, taps, s), dtype) for s in seeds])
    refs = [ref(r, taps if out_len is None else out_len, oversample, dtype) for r in rows]
    for a in (rows,) + tuple(x for yb in refs for x in yb if x is not None):
        a.setflags(write=False)
    return rows, refs


def check_rows(got, refs, dtype, name):
    """Every sample of every row against its bound; an all-zero row against its own criterion."""
    assert got.dtype == NP[dtype] and got.shape[0] == len(refs)
    worst = 0.0
    for g, (y, B) in zip(got, refs):
        assert g.shape == y.shape and np.all(np.isfinite(g))
        if B is None:
            assert np.all(g == 0.0) if dtype == F32 else np.all(np.abs(g) < 1e-100), (name, g[:4])
            continue
        worst = max(worst, float(np.max(np.abs(g.astype(np.float64) - y) / B)))
    _record(name, worst)
    assert worst <= 1.0, (name, worst)
    return worst


# ---- CPU -------------------------------------------------------------------------------------------------------------------------------
def test_symbols_exported():
    for name in ("MinPhasePlan", "minimum_phase", "minimum_phase_with"):
        assert hasattr(sg, name) and name in sg.__all__
    L = _ffi.lib()
    for s in ("sgx_minphase_create", "sgx_minphase_destroy", "sgx_minphase_execute", "sgx_minphase_reserve", "sgx_minphase_fft_size",
              "sgx_minphase_output_length", "sgx_minphase_taps", "sgx_minphase_kernel_name", "sgx_minphase_device", "sgx_minphase_last_error"):
        assert s in _ffi.SYMBOLS and hasattr(L, s)
    assert L.sgx_abi_version() == 7


def test_validation_texts():
    host = _ffi.DEVICE_HOST_ONLY
    with pytest.raises(sg.InvalidInputError, match="impulse response must not be empty"):
        sg.MinPhasePlan(0, device=host)
    with pytest.raises(sg.InvalidInputError, match="impulse response must not be empty"):
        sg.minimum_phase([])
    with pytest.raises(sg.InvalidInputError, match="impulse response must not be empty"):
        sg.minimum_phase_with(np.zeros((3, 0)), 4, 8)
    with pytest.raises(sg.InvalidInputError, match="out_len must be greater than zero"):
        sg.MinPhasePlan(8, out_len=0, device=host)
    with pytest.raises(sg.InvalidInputError, match="out_len must be greater than zero"):
        sg.minimum_phase_with(np.ones(8), 0, 8)
    with pytest.raises(ValueError, match="route must be"):
        sg.MinPhasePlan(8, route="fast", device=host)
    with pytest.raises(ValueError, match=r"ir must be 1-D \(taps,\) or 2-D \(batch, taps\)"):
        sg.minimum_phase(np.ones((2, 3, 4)))
    with pytest.raises(ValueError, match=r"ir must be 1-D \(taps,\) or 2-D \(batch, taps\)"):
        sg.MinPhasePlan(4, device=host).execute(np.ones((2, 3, 4)))
    with pytest.raises(ValueError, match="must not be negative"):
        sg.MinPhasePlan(8, oversample=-1, device=host)
    # C ABI: the create error text without a plan
    L = _ffi.lib()
    out = C.c_void_p()
    assert L.sgx_minphase_create(4, 4, 8, 7, _ffi.F32, host, C.byref(out)) == _ffi.SGX_INVALID_INPUT
    assert b"unknown route" in L.sgx_minphase_last_error(None) and not out.value
    assert L.sgx_minphase_create(4, 4, 8, 0, 5, host, C.byref(out)) == _ffi.SGX_INVALID_INPUT
    assert b"dtype" in L.sgx_minphase_last_error(None)
    assert L.sgx_minphase_create(0, 4, 8, 0, _ffi.F64, host, C.byref(out)) == _ffi.SGX_INVALID_INPUT
    assert L.sgx_minphase_last_error(None) == b"Invalid input: impulse response must not be empty"
    assert L.sgx_minphase_create(4, 0, 8, 0, _ffi.F64, host, C.byref(out)) == _ffi.SGX_INVALID_INPUT
    assert L.sgx_minphase_last_error(None) == b"Invalid input: out_len must be greater than zero"
    assert L.sgx_minphase_create(4, 4, 8, 0, _ffi.F64, host, None) == _ffi.SGX_INVALID_INPUT


def test_host_only_plan_reports_shapes_and_refuses_compute():
    p = sg.MinPhasePlan(5, dtype=F32, device=_ffi.DEVICE_HOST_ONLY)
    assert (p.taps, p.fft_size, p.output_length, p.kernel_name, p.device, p.dtype) == (5, 64, 5, "k_minphase", -2, F32)
    text = "plan has no HIP device \\(host-only plan\\)"
    with pytest.raises(sg.FFTBackendError, match=text):
        p.execute(np.zeros(5))
    with pytest.raises(sg.FFTBackendError, match=text):
        p.execute(np.zeros((2, 5)))
    with pytest.raises(sg.FFTBackendError, match=text):
        p.reserve(2)
    with pytest.raises(sg.DimensionMismatchError, match="expected 5, got 6"):
        p.execute(np.zeros(6))
    g = sg.MinPhasePlan(5, dtype=F64, route="generic", device=_ffi.DEVICE_HOST_ONLY)
    assert (g.fft_size, g.kernel_name, g.dtype) == (64, "minphase_generic", F64)
    with pytest.raises(sg.FFTBackendError, match=text):
        g.execute(np.zeros(5))
    # shape errors come before the device check
    L = _ffi.lib()
    x, y = np.zeros(10, np.float32), np.zeros(10, np.float32)
    assert L.sgx_minphase_execute(p._h, x.ctypes.data, 2, y.ctypes.data, 9, _ffi.MEM_HOST, None) == _ffi.SGX_DIM_MISMATCH
    assert b"expected 10, got 9" in L.sgx_minphase_last_error(p._h)
    assert L.sgx_minphase_execute(p._h, x.ctypes.data, 0, y.ctypes.data, 0, _ffi.MEM_HOST, None) == _ffi.SGX_INVALID_INPUT
    assert L.sgx_minphase_execute(p._h, x.ctypes.data, 65536, y.ctypes.data, 65536 * 5, _ffi.MEM_HOST, None) == _ffi.SGX_INVALID_INPUT
    assert b"1 .. 65535" in L.sgx_minphase_last_error(p._h)
    assert L.sgx_minphase_execute(None, x.ctypes.data, 1, y.ctypes.data, 5, _ffi.MEM_HOST, None) == _ffi.SGX_INVALID_INPUT


@pytest.mark.parametrize("taps,oversample,fft_size,name", [
    (1, 1, 1, "k_minphase"), (5, 8, 64, "k_minphase"), (512, 8, 4096, "k_minphase"), (4096, 1, 4096, "k_minphase"), (3, 0, 4, "k_minphase"),
    (513, 8, 8192, "minphase_generic"), (3000, 8, 32768, "minphase_generic"), (131072, 8, 1 << 20, "minphase_generic"),
])
def test_route_table(taps, oversample, fft_size, name):
    for dtype in (F32, F64):
        p = sg.MinPhasePlan(taps, oversample=oversample, dtype=dtype, device=_ffi.DEVICE_HOST_ONLY)
        assert (p.fft_size, p.kernel_name, p.taps, p.output_length) == (fft_size, name, taps, taps)
        assert fft_len(taps, oversample) == fft_size
    g = sg.MinPhasePlan(taps, oversample=oversample, route="generic", device=_ffi.DEVICE_HOST_ONLY)
    assert (g.fft_size, g.kernel_name) == (fft_size, "minphase_generic")


def test_more_than_2_pow_20_points_is_refused_at_create():
    for route in ("auto", "generic"):
        with pytest.raises(sg.FFTBackendError, match="1048576"):
            sg.MinPhasePlan(131073, oversample=8, route=route, device=_ffi.DEVICE_HOST_ONLY)
    with pytest.raises(sg.FFTBackendError, match="1048576"):
        sg.MinPhasePlan(3, oversample=2 ** 62, device=_ffi.DEVICE_HOST_ONLY)  # (no overflow in taps * oversample)
    assert sg.MinPhasePlan(1 << 20, oversample=1, device=_ffi.DEVICE_HOST_ONLY).fft_size == 1 << 20


@pytest.mark.parametrize("taps,oversample,out_len,want", [(64, 8, None, 64), (64, 8, 10, 10), (64, 8, 300, 300), (64, 8, 512, 512),
                                                          (64, 8, 5000, 512), (3, 1, 4, 4), (3, 1, 5, 4), (1, 1, 7, 1), (513, 8, 9000, 8192)])
def test_output_length_table(taps, oversample, out_len, want):
    p = sg.MinPhasePlan(taps, out_len, oversample, device=_ffi.DEVICE_HOST_ONLY)
    assert p.output_length == want == min(taps if out_len is None else out_len, p.fft_size)
    y, _ = ref(np.ones(taps), taps if out_len is None else out_len, oversample, F64)
    assert y.size == want


def test_restatement_self_checks():
    for os_, tol in ((1, 1e-12), (64, 1e-9)):
        for h in ([1.0, -0.5], [-0.5, 1.0]):  # a zero inside the unit circle, and its mirror image outside
            y, B = ref(np.array(h), 2, os_, F64)
            assert np.max(np.abs(y - [1.0, -0.5])) < tol and B is not None
    y, _ = ref(np.array([0.0, 0.0, 0.0, 1.0]), 4, 1, F64)
    assert np.max(np.abs(y - [1.0, 0.0, 0.0, 0.0])) < 1e-15
    y, _ = ref(np.array([-3.0]), 1, 1, F64)
    assert y.shape == (1,) and abs(y[0] - 3.0) < 1e-15
    y, B = ref(np.zeros(8), 8, 8, F64)
    assert B is None and np.all(np.abs(y) < 1e-100) and np.all(np.isfinite(y))


def mag_at(h, n, k):
    """DFT magnitude of a real sequence at k / n cycles, evaluated directly (src/min_phase.rs:149-156)."""
    return abs(np.sum(np.asarray(h, np.float64) * np.exp(-2j * np.pi * k / n * np.arange(len(h)))))


def centroid(h):
    e = np.asarray(h, np.float64) ** 2
    return float(np.sum(np.arange(e.size) * e) / np.sum(e))


def reference_unit_tests(convert):
    """The reference's two unit tests (src/min_phase.rs:158-227) with their own tolerances, on `convert` (f32 row -> f32 row)."""
    lin = lowpass(64).astype(np.float32)
    mp = convert(lin)
    assert mp.shape == lin.shape
    for k in range(257):
        a, b = mag_at(lin, 512, k), mag_at(mp, 512, k)
        assert abs(a - b) < 1e-2 + 1e-2 * a, (k, a, b)
    lin = lowpass(64, hann=False).astype(np.float32)
    mp = convert(lin)
    assert abs(centroid(lin) - 31.5) < 1e-6 and centroid(mp) < 0.5 * centroid(lin)
    return centroid(mp)


def test_reference_unit_tests_in_the_restatement():
    c = reference_unit_tests(lambda lin: ref(lin, lin.size, 8, F32)[0].astype(np.float32))
    assert abs(c - 5.36) < 0.01


def fft32(x, inverse=False):
    """Radix-2 decimation in time in complex64: what an f32 pipeline's transform rounds like."""
    x = x.astype(np.complex64)
    n = x.size
    if n == 1:
        return x
    lv = n.bit_length() - 1
    idx = np.arange(n)
    rev = np.zeros(n, int)
    for b in range(lv):
        rev |= ((idx >> b) & 1) << (lv - 1 - b)
    x = x[rev]
    s = 2
    while s <= n:
        tw = np.exp((2j if inverse else -2j) * np.pi * np.arange(s // 2) / s).astype(np.complex64)
        x = x.reshape(-1, s)
        a, b = x[:, :s // 2], x[:, s // 2:] * tw
        x = np.concatenate([a + b, a - b], 1).astype(np.complex64).reshape(-1)
        s *= 2
    return x


def f32_pipeline(h, oversample):
    h = np.asarray(h, np.float32)
    n = fft_len(h.size, oversample)
    b = np.zeros(n, np.complex64)
    b[:h.size] = h
    H = fft32(b)
    m2 = (H.real ** 2 + H.imag ** 2).astype(np.float32)
    eps = np.float32(m2.max() * np.float32(1e-20))
    L = (np.float32(0.5) * np.log(m2 + eps)).astype(np.float32)
    c = fft32(L, True) * np.float32(1.0 / n)
    Cs = fft32(c * fold_weights(n).astype(np.float32))
    mag = np.exp(Cs.real).astype(np.float32)
    Hm = (mag * np.cos(Cs.imag) + 1j * mag * np.sin(Cs.imag)).astype(np.complex64)
    return fft32(Hm, True).real * np.float32(1.0 / n)


@pytest.mark.parametrize("kind", KINDS)
def test_f32_restatement_is_a_small_fraction_of_the_f32_form_of_the_bound(kind):
    """The bound's form holds with room: with u = 2^-24 an all-f32 pipeline stays at <= 0.012 of it (where the nulls of a low-pass make
    expm1 overflow the f32 form is infinite, and says nothing)."""
    worst = 0.0
    for taps, os_ in FUSED + GENERIC:
        h = tcast(make_ir(kind, taps, 7), F32)
        p = pipeline(h, os_)
        if p["mx"] == 0.0:
            continue
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            got = f32_pipeline(h, os_)[:taps].astype(np.float64)
        B = bound_of(p, 2.0 ** -24)
        if not math.isfinite(B):
            continue
        worst = max(worst, float(np.max(np.abs(got - p["y"][:taps])) / B))
    print(f"{kind}: f32 restatement at {worst:.3g} of the u = 2^-24 bound")
    assert worst <= 0.012


@pytest.mark.parametrize("kind", KINDS)
def test_bound_over_peak_is_what_the_docstring_says(kind):
    """Over SHORT_FUSED as well: at n = 4 .. 32 the bound is no wider than at the long lengths (B / peak <= 4e-11 on every kind but
    the 4-tap low-pass, whose outer taps are the Hann window's zeros: 5.7e-6, inside the low-passes' 3e-3)."""
    lo, hi = math.inf, 0.0
    for taps, os_ in FUSED + SHORT_FUSED + GENERIC:
        for dtype in (F32, F64):
            rows, _ = case(kind, taps, os_, dtype)
            for row in rows:
                p = pipeline(row, os_)
                if p["mx"] == 0.0:
                    continue
                r = bound_of(p, U53) / np.abs(p["y"][:taps]).max()
                lo, hi = min(lo, r), max(hi, r)
    print(f"{kind}: B / peak {lo:.3g} .. {hi:.3g}")
    assert hi <= (3e-3 if kind == "lowpass" else 5e-11)


@pytest.mark.parametrize("mistake", ["fold_weight", "no_eps", "one_over_n", "nyquist_doubled", "nyquist_dropped"])
def test_bound_catches_the_usual_mistakes(mistake):
    """Each planted mistake leaves the bound on at least one of the parity inputs — by a wide margin."""
    worst = 0.0
    for kind in KINDS:
        for taps, os_ in ((5, 8), (64, 8), (64, 1), (200, 8)):
            rows, refs = case(kind, taps, os_, F64)
            y, B = refs[0]
            if B is None:
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                bad = pipeline(rows[0], os_, mistake)["y"][:taps]
            d = np.abs(bad - y) / B
            worst = max(worst, float(np.max(np.where(np.isfinite(d), d, np.inf))))
    print(f"{mistake}: worst ratio {worst:.3g}")
    assert worst > 100.0


# ---- GPU: parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("taps,oversample,route", PARITY, ids=[f"{t}-{o}-{r}" for t, o, r in PARITY])
def test_gpu_parity(taps, oversample, route, dtype):
    plan = sg.MinPhasePlan(taps, oversample=oversample, dtype=dtype, route=route)
    fused = route == "auto" and fft_len(taps, oversample) <= 4096
    assert plan.kernel_name == ("k_minphase" if fused else "minphase_generic") and plan.fft_size == fft_len(taps, oversample)
    for kind in KINDS:
        rows, refs = case(kind, taps, oversample, dtype)
        got = plan.execute(rows.astype(NP[dtype]))
        assert got.shape == (3, taps)
        check_rows(got, refs, dtype, f"{plan.kernel_name}-{dtype}-{kind}")
    # the one-shot functions and a single row: the same bits
    rows, _ = case("decay", taps, oversample, dtype)
    got = plan.execute(rows.astype(NP[dtype]))
    if fused:  # (a row's arithmetic does not depend on the batch around it)
        one = sg.minimum_phase_with(rows[1], taps, oversample, dtype=dtype)
        assert one.shape == (taps,) and one.tobytes() == got[1].tobytes()
        if oversample == 8:
            assert sg.minimum_phase(rows, dtype=dtype).tobytes() == got.tobytes()


@pytest.mark.gpu
def test_gpu_parity_at_the_longest_transform():
    """n = 2^20, f64, white noise, batch 2."""
    taps, os_ = 131072, 8
    rows, refs = case("noise", taps, os_, F64, seeds=(7, 8))
    plan = sg.MinPhasePlan(taps, oversample=os_, dtype=F64)
    assert (plan.fft_size, plan.kernel_name) == (1 << 20, "minphase_generic")
    check_rows(plan.execute(rows), refs, F64, "minphase_generic-float64-2^20")


# ---- GPU: further properties -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("route", ["auto", "generic"])
@pytest.mark.parametrize("out_len,want", [(10, 10), (300, 300), (5000, 512)])
def test_gpu_out_len(out_len, want, route, dtype):
    for kind in ("decay", "lowpass"):
        rows, refs = case(kind, 64, 8, dtype, out_len=out_len)
        plan = sg.MinPhasePlan(64, out_len, 8, dtype=dtype, route=route)
        got = plan.execute(rows.astype(NP[dtype]))
        assert got.shape == (3, want) and plan.output_length == want
        check_rows(got, refs, dtype, f"{plan.kernel_name}-{dtype}-out_len")
        assert sg.minimum_phase_with(rows, out_len, 8, dtype=dtype).shape == (3, want)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("taps,route", [(64, "auto"), (64, "generic"), (513, "auto")])
def test_gpu_eps_is_per_row(taps, route, dtype):
    """One batch whose rows are the same response scaled by 1, 10^6 and 10^-6: a maximum (or an eps) taken over the batch would put
    the quiet row's eps 10^4 above its own spectrum.  Each row is within its own bound, and the rows scaled back agree within the sum of
    their bounds (plus the difference of their restatements: the scaling itself rounds in T)."""
    scales = (1.0, 1e6, 1e-6)
    for kind in ("decay", "lowpass"):
        base = make_ir(kind, taps, 11)
        rows = np.stack([tcast(base * s, dtype) for s in scales])
        refs = [ref(r, taps, 8, dtype) for r in rows]
        plan = sg.MinPhasePlan(taps, dtype=dtype, route=route)
        got = plan.execute(rows.astype(NP[dtype]))
        check_rows(got, refs, dtype, f"{plan.kernel_name}-{dtype}-scaled")
        (y0, B0) = refs[0]
        for s, g, (y, B) in zip(scales[1:], got[1:], refs[1:]):
            d = np.abs(g.astype(np.float64) / s - got[0].astype(np.float64))
            assert np.all(d <= B0 + B / s + np.abs(y / s - y0)), (kind, s, float(np.max(d / (B0 + B / s))))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
def test_gpu_more_rows_than_compute_units(dtype):
    """600 rows x 64 taps: every row against its bound (the rows cycle through the four kinds with their own seeds)."""
    rows = np.stack([tcast(make_ir(KINDS[r % 4], 64, 100 + r), dtype) for r in range(600)])
    refs = [ref(r, 64, 8, dtype) for r in rows]
    plan = sg.MinPhasePlan(64, dtype=dtype)
    assert plan.kernel_name == "k_minphase"
    check_rows(plan.execute(rows.astype(NP[dtype])), refs, dtype, f"k_minphase-{dtype}-600rows")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("taps,route", [(64, "auto"), (64, "generic"), (1, "auto"), (2, "auto"), (513, "auto")])
def test_gpu_all_zero_row(taps, route, dtype):
    """f64: finite with |y| < 1e-100; f32: exact zeros; the rows beside it are what they are without it."""
    rows, refs = case("decay", taps, 8, dtype)
    with_zero = np.stack([rows[0], np.zeros(taps), rows[1], rows[2]])
    plan = sg.MinPhasePlan(taps, dtype=dtype, route=route)
    got = plan.execute(with_zero.astype(NP[dtype]))
    assert np.all(np.isfinite(got))
    if dtype == F32:
        assert np.all(got[1] == 0.0)
    else:
        assert np.all(np.abs(got[1]) < 1e-100)
    check_rows(got[[0, 2, 3]], refs, dtype, f"{plan.kernel_name}-{dtype}-beside-zeros")
    if plan.kernel_name == "k_minphase":  # a workgroup per row: the same bits whatever the batch
        alone = plan.execute(rows.astype(NP[dtype]))
        assert alone.tobytes() == got[[0, 2, 3]].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["auto", "generic"])
def test_gpu_reference_unit_tests(route):
    """magnitude_response_is_preserved and energy_is_front_loaded (src/min_phase.rs:158-227) through the engine in f32."""
    if route == "auto":
        c = reference_unit_tests(lambda lin: sg.minimum_phase(lin, dtype=F32))
    else:
        c = reference_unit_tests(lambda lin: sg.MinPhasePlan(64, dtype=F32, route="generic").execute(lin))
    print(f"energy centroid {c:.3f} (linear phase: 31.5)")
    mp = sg.minimum_phase(np.array([0.1, 0.2, 0.4, 0.2, 0.1], np.float32), dtype=F32)  # the doc example (:46-54)
    assert mp.shape == (5,) and mp.dtype == np.float32 and abs(mp[0]) >= abs(mp[-1])
    assert sg.minimum_phase([0.1, 0.2, 0.4, 0.2, 0.1]).dtype == np.float64


# ---- GPU: stream order, capture, repeatability ----------------------------------------------------------------------------------------
STREAM_ROWS = [(200, "auto", F32), (200, "auto", F64), (700, "auto", F32), (700, "auto", F64)]  # n = 2048 fused, n = 8192 generic
STREAM_IDS = [f"{t}-{r}-{d}" for t, r, d in STREAM_ROWS]
SENTINEL = -1.2345678e30


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a.astype(NP[dtype]))).cuda()


def _stream_case(taps, dtype, batch=4):
    xs = [np.stack([tcast(make_ir(KINDS[(r + k) % 4], taps, 200 + 10 * k + r), dtype) for r in range(batch)]) for k in range(3)]
    return xs, [_dev(x, dtype) for x in xs]


@pytest.mark.gpu
@pytest.mark.parametrize("taps,route,dtype", STREAM_ROWS, ids=STREAM_IDS)
def test_gpu_call_is_one_operation_of_the_side_stream(taps, route, dtype):
    """Behind a producer of >= 10 ms on a side stream whose last operation writes the responses, with NaN inputs and a sentinel output
    until then: the result equals the host path's, and nothing is written after the work queued behind it."""
    import torch
    from tests.test_stream_order import producer
    xs, dxs = _stream_case(taps, dtype)
    host = sg.MinPhasePlan(taps, dtype=dtype, route=route)
    assert host.kernel_name == ("k_minphase" if taps == 200 else "minphase_generic")
    ref_bits = host.execute(xs[0].astype(NP[dtype]))
    host.execute_torch(dxs[0])  # (also loads every code object the call launches)
    torch.cuda.synchronize()
    plan = sg.MinPhasePlan(taps, dtype=dtype, route=route)
    plan.reserve(dxs[0].shape[0], host_staging=False)
    xin = torch.full_like(dxs[0], float("nan"))
    out = torch.full((dxs[0].shape[0], plan.output_length), SENTINEL, dtype=dxs[0].dtype, device="cuda")
    big, ops = producer()  # in-place additions on a 1 GiB buffer, about 25 ms of them
    side = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        e0.record()
        for _ in range(ops):
            big.add_(1.0)
        xin.copy_(dxs[0])
        e1.record()
        plan.execute_torch(xin, out)
        snap = out.clone()
        out.fill_(SENTINEL)
    done_at_return = e1.query()
    torch.cuda.synchronize()
    print(f"producer {e0.elapsed_time(e1):.1f} ms, done when the host returned from the call: {done_at_return}")
    assert snap.cpu().numpy().tobytes() == ref_bits.tobytes(), "the result queued behind the producer differs from the host path's"
    assert torch.all(out == SENTINEL), "something wrote the output after the work queued behind the call"
    assert e0.elapsed_time(e1) >= 10.0 and done_at_return is False, "no hazard window was shown"


@pytest.mark.gpu
@pytest.mark.parametrize("taps,route,dtype", STREAM_ROWS, ids=STREAM_IDS)
def test_gpu_reserved_call_is_captured_and_replayed(taps, route, dtype):
    """After reserve a device call allocates nothing, synchronises nothing and names the same buffers every time: captured once on a side
    stream, its replays on new input equal the host path byte for byte."""
    import torch
    xs, dxs = _stream_case(taps, dtype)
    host = sg.MinPhasePlan(taps, dtype=dtype, route=route)
    refs = [host.execute(x.astype(NP[dtype])) for x in xs]
    host.execute_torch(dxs[0])  # (also loads every code object the call launches)
    torch.cuda.synchronize()
    plan = sg.MinPhasePlan(taps, dtype=dtype, route=route)
    plan.reserve(dxs[0].shape[0], host_staging=False)
    xin = dxs[0].clone()
    out = torch.full((dxs[0].shape[0], plan.output_length), SENTINEL, dtype=dxs[0].dtype, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.execute_torch(xin, out)
    for k in (2, 1, 0):
        xin.copy_(dxs[k])
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == refs[k].tobytes(), f"replay on input {k} differs from the host path's result"


@pytest.mark.gpu
@pytest.mark.parametrize("taps,route,dtype", STREAM_ROWS, ids=STREAM_IDS)
def test_gpu_repeated_calls_on_a_fresh_plan_are_bit_equal(taps, route, dtype):
    import torch
    xs, dxs = _stream_case(taps, dtype)
    plan = sg.MinPhasePlan(taps, dtype=dtype, route=route)
    a = plan.execute_torch(dxs[0])
    plan.execute_torch(dxs[1][:2].contiguous())  # a smaller call in between changes nothing
    b = plan.execute_torch(dxs[0])
    host = plan.execute(xs[0].astype(NP[dtype]))
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == host.tobytes()
    fresh = sg.MinPhasePlan(taps, dtype=dtype, route=route).execute_torch(dxs[0])
    torch.cuda.synchronize()
    assert fresh.cpu().numpy().tobytes() == host.tobytes()


# Every prototype of the minimum-phase family that takes a stream, and the tests above that put it on a side stream.  (The header scan
# of tests/test_stream_order.py keys on its own table of rows; this entry point is covered here instead.)
STREAM_COVERAGE = {
    "sgx_minphase_execute": ("test_gpu_call_is_one_operation_of_the_side_stream", "test_gpu_reserved_call_is_captured_and_replayed"),
}


def test_every_stream_taking_prototype_of_the_family_has_a_stream_test():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectro_hip.h")).read()
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(?:sgx_status|void|size_t|int32_t|const char \*)\s*(sgx_minphase_\w+)\s*\(([^;{]*?)\)\s*;", hdr, re.S)}
    assert len(protos) == 10 and "sgx_minphase_create" in protos  # the parser sees the header
    found = {name for name, params in protos.items() if re.search(r"void\s*\*\s*(?:hip_)?stream\b", params)}
    assert found == set(STREAM_COVERAGE), found ^ set(STREAM_COVERAGE)
    for name, tests in STREAM_COVERAGE.items():
        for test in tests:
            fn = globals()[test]
            assert any(mark.name == "gpu" for mark in getattr(fn, "pytestmark", [])), test
    # the Python layer hands it torch's current stream (through the stream helper of the plans' shared base, which fetches it)
    src = open(os.path.join(os.path.dirname(_ffi.__file__), "minphase.py")).read()
    base = open(os.path.join(os.path.dirname(_ffi.__file__), "_handle.py")).read()
    for name in STREAM_COVERAGE:
        assert name in src and "self._stream()" in src and "current_stream" in base
