"""Binaural ITD / IPD / ILD / ILR plans (src/binaural.rs) against an f64 NumPy restatement.

The truth is the reference's table evaluated in f64 over f64 rfft frames (tests/helpers.py framing, the plan's own window).  Per frame
f the library's spectrum is off by at most delta_f = c u_T log2 N sqrt N ||x_f w|| (the per-frame bound of test_frame_locality.py,
restated here; the routes that pair frames 2p / 2p + 1 in one transform use the pair's joint norm), so with rho_c = delta_f / |X_c[k]|
the phase of channel c is off by at most asin(rho_c) <= 1.01 rho_c (rho_c <= 1e-2) and its magnitude by a factor within 1 +- rho_c.
"""
import math

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from spectrograms_amd.binaural import BinauralPlan

from . import helpers as H

SR = 16000.0
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
NP = {"float32": np.float32, "float64": np.float64}
HOST = _ffi.DEVICE_HOST_ONLY
KINDS = ["itd", "ipd", "ild", "ilr"]
PCLS = {"itd": sg.ITDSpectrogramParams, "ipd": sg.IPDSpectrogramParams, "ild": sg.ILDSpectrogramParams, "ilr": sg.ILRSpectrogramParams}
RANGES = {"itd": (-0.00088, 0.00088), "ipd": (-math.pi, math.pi), "ild": (-24.0, 24.0), "ilr": (-1.0, 1.0)}
# frame-pairing routes (name, dtype, n_fft or None for every length), as read from the code; the partner of frame f is f ^ 1
PAIRED = [("r32x16_f32", "float32", 512), ("d512_f64", "float64", 512), ("bluestein", "float32", None), ("bluestein", "float64", None),
          ("big_four_step", "float32", None), ("big_four_step", "float64", None), ("big_chirpz", "float32", None), ("big_chirpz", "float64", None)]


def spec_params(n_fft, hop):
    return sg.SpectrogramParams(sg.StftParams(n_fft, hop, sg.WindowType.hanning, True), SR)


def bparams(kind, n_fft, hop, band=None, **kw):
    sp = spec_params(n_fft, hop)
    return PCLS[kind](sp, *band, **kw) if band else PCLS[kind](sp, **kw)


def window(n_fft, hop):
    return np.asarray(sg.Plan(spec_params(n_fft, hop), _ffi.AMP_COMPLEX, dtype="float64", device=HOST).window(), np.float64)


FUSED = "r32x16_binaural_f32"


def route_of(plan):
    """The complex STFT route whose spectra the map is made of (the fused route runs the tuned kernel's passes unchanged)."""
    name = plan.kernel_name
    if name == FUSED:
        return "r32x16_f32"
    assert name.startswith("binaural_epilogue/"), name
    return name.split("/", 1)[1]


def paired(name, dtype, n_fft):
    return any(r == name and d == dtype and (n is None or n == n_fft) for r, d, n in PAIRED)


def chirp_m(n):
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def frame_deltas(x64, w, n_fft, hop, dtype, name):
    """delta_f per (row, frame) for the route `name` (c = 4, chirp-z routes c = 12 at their convolution length; joint norm when paired)."""
    c = 12.0 if name in ("bluestein", "big_chirpz") else 4.0
    neff = chirp_m(n_fft) if name in ("bluestein", "big_chirpz") else n_fft
    fr = np.stack([H.np_frames(r, n_fft, hop, True) for r in x64]) * w[None, None, :]
    nrm2 = np.sum(fr ** 2, axis=-1)
    if paired(name, dtype, n_fft):
        nf = nrm2.shape[1]
        idx = np.arange(nf) ^ 1
        idx[idx >= nf] = np.arange(nf)[idx >= nf]
        nrm2 = nrm2 + np.where(idx != np.arange(nf), nrm2[:, idx], 0.0)
    return c * U[dtype] * math.log2(neff) * math.sqrt(neff) * np.sqrt(nrm2)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def bins_of(n_fft, f0, f1):
    """start_bin, stop_bin: (f / bw).round() as usize — Rust rounds half away from zero (NumPy's round would go to even)."""
    bw = SR / n_fft
    return int(math.floor(f0 / bw + 0.5)), int(math.floor(f1 / bw + 0.5))


def np_mod(x, m):
    return np.fmod(np.fmod(x, m) + m, m)


def truth(kind, XL, XR, k, bw, T=np.float64, wrapped=False, power=1):
    """The table of src/binaural.rs vectorised in precision T.  XL, XR: [..., n_bins, n_frames] complex (the band rows), k: their bins."""
    T = np.dtype(T).type
    kk = np.asarray(k, T).reshape((-1, 1))
    pi = T(np.pi)
    two_pi = T(2) * pi

    def mp(X):
        re, im = X.real.astype(T), X.imag.astype(T)
        with np.errstate(all="ignore"):
            msq = (re.astype(np.float64) * re + (im * im).astype(np.float64)).astype(T) if T is np.float32 else re * re + im * im
            zero = msq == 0
            mag = np.where(zero, T(0), np.sqrt(msq)).astype(T)
            inv = np.where(zero, T(1), T(1) / np.where(zero, T(1), mag)).astype(T)
            pre = np.where(zero, T(1), re * inv).astype(T)
            pim = np.where(zero, T(0), im * inv).astype(T)
            return mag, msq, np.arctan2(pim, pre).astype(T)

    (mL, sL, aL), (mR, sR, aR) = mp(XL), mp(XR)
    with np.errstate(all="ignore"):
        if kind == "itd":
            pw = {1: lambda m, s: m, 2: lambda m, s: s, 3: lambda m, s: s * m, 4: lambda m, s: s * s}.get(power, lambda m, s: m ** power)
            inten = pw(mL, sL) + pw(mR, sR)
            v = (np_mod(aL - aR + pi, two_pi) - pi) / (two_pi * T(bw) * kk)
            return np.where(inten > 0, v, T(0)).astype(T)
        if kind == "ipd":
            d = aL - aR
            return (np_mod(d + pi, two_pi) - pi if wrapped else d).astype(T)
        ok = (mL + mR > 0) & (mL > 0) & (mR > 0)
        r = mR / mL
        if kind == "ild":
            v = T(-20) * np.log10(r)
        else:
            v = np.where(r < 1, T(1) - r, -(T(1) - T(1) / r))
        return np.where(ok, v, T(np.nan)).astype(T)


def literal(kind, XL, XR, start_bin, bw, wrapped=False, power=1):
    """A per-element transcription of the reference's loops (f64), for the restatement's own check."""
    nb, nf = XL.shape
    out = np.zeros((nb, nf)) if kind == "itd" else np.full((nb, nf), np.nan) if kind in ("ild", "ilr") else np.zeros((nb, nf))
    pi, two_pi = math.pi, 2.0 * math.pi

    def magphase(c):
        msq = math.fma(c.real, c.real, c.imag * c.imag) if hasattr(math, "fma") else c.real * c.real + c.imag * c.imag
        if msq == 0.0:
            return 0.0, msq, complex(1.0, 0.0)
        m = math.sqrt(msq)
        inv = 1.0 / m
        return m, msq, complex(c.real * inv, c.imag * inv)

    def pow_mag(m, s, p):
        if p == 1:
            return m
        if p == 2:
            return s
        if p == 3:
            return s * m
        if p == 4:
            return s * s
        base, e, acc = m, p, 1.0
        while e > 0:
            if e & 1:
                acc *= base
            e >>= 1
            if e > 0:
                base *= base
        return acc

    def npmod(x, m):
        return math.fmod(math.fmod(x, m) + m, m)

    for b in range(nb):
        for f in range(nf):
            lm, ls, lp = magphase(complex(XL[b, f]))
            rm, rs, rp = magphase(complex(XR[b, f]))
            la, ra = math.atan2(lp.imag, lp.real), math.atan2(rp.imag, rp.real)
            if kind == "itd":
                lm, rm = (pow_mag(lm, ls, power) if ls != 0 else 0.0), (pow_mag(rm, rs, power) if rs != 0 else 0.0)
                if lm + rm > 0:
                    k = start_bin + b
                    w = npmod(la - ra + pi, two_pi) - pi
                    out[b, f] = w / (two_pi * bw * k) if k else (math.copysign(math.inf, w) if w else math.nan)
            elif kind == "ipd":
                d = la - ra
                out[b, f] = npmod(d + pi, two_pi) - pi if wrapped else d
            elif lm + rm > 0 and lm > 0 and rm > 0:
                r = rm / lm
                out[b, f] = -20.0 * math.log10(r) if kind == "ild" else (1.0 - r if r < 1.0 else -(1.0 - 1.0 / r))
    return out


def hist_truth(v, num_bins, lo, hi, exponent=1, normalize=False):
    """Histogram restatement: v [n_rows, n_frames] -> [num_bins, n_frames] f64."""
    v = np.asarray(v, np.float64)
    width = (hi - lo) / num_bins
    out = np.zeros((num_bins, v.shape[1]))
    with np.errstate(all="ignore"):
        ok = np.isfinite(v) & ~(v < lo) & ~(v > hi)
        q = np.floor((v - lo) / width)
    q = np.where(np.isnan(q) | (q < 0), 0, np.minimum(q, num_bins - 1)).astype(np.int64)
    for f in range(v.shape[1]):
        np.add.at(out[:, f], q[ok[:, f], f], 1.0)
    if exponent != 1:
        out = out ** exponent if exponent > 0 else np.where(out == 0, np.inf, 1.0 / out ** -exponent)
        if exponent == 0:
            out = np.ones_like(out)
    if normalize:
        s = out.sum(axis=0)
        out = np.where(s > 0, out / np.where(s > 0, s, 1.0), out)
    return out


def stereo(dtype, batch, n, seed=0, delay=3, gain=0.5):
    """Seeded pairs: R = gain * L delayed by `delay` samples + independent noise."""
    rng = np.random.default_rng(seed)
    L = rng.standard_normal((batch, n)) + 0.3 * np.sin(2 * np.pi * 440.0 * np.arange(n) / SR)[None]
    R = gain * np.roll(L, delay, axis=1) + 0.2 * rng.standard_normal((batch, n))
    return L.astype(NP[dtype]), R.astype(NP[dtype])


# ---- CPU tests -------------------------------------------------------------------------------------------------------------------------
def test_symbols_exported():
    for name in ["ITDSpectrogramParams", "IPDSpectrogramParams", "ILDSpectrogramParams", "ILRSpectrogramParams", "ItdSpectrogram",
                 "IpdSpectrogram", "IldSpectrogram", "IlrSpectrogram", "BinauralPlan", "compute_itd_spectrogram", "compute_ipd_spectrogram",
                 "compute_ild_spectrogram", "compute_ilr_spectrogram", "compute_itd_spectrogram_diff", "compute_ilr_spectrogram_diff"]:
        assert name in sg.__all__ and hasattr(sg, name), name
    L = _ffi.lib()
    for s in _ffi.SYMBOLS:
        if s.startswith("sgx_binaural_"):
            assert hasattr(L, s), s


def test_defaults_and_getters():
    sp = spec_params(1024, 256)
    p = sg.ITDSpectrogramParams(sp)
    assert (p.start_freq, p.end_freq, p.magphase_power) == (50.0, 620.0, 1) and p.spectrogram_params is sp
    assert sg.ITDSpectrogramParams(sp, magphase_power=0).magphase_power == 1  # the binding maps 0 to 1
    q = sg.IPDSpectrogramParams(sp)
    assert (q.start_freq, q.end_freq, q.wrapped) == (50.0, 620.0, False)
    for cls in (sg.ILDSpectrogramParams, sg.ILRSpectrogramParams):
        r = cls(sp)
        assert (r.start_freq, r.end_freq) == (1700.0, 4600.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("band,msg", [((0.0, 100.0), "Invalid input: Start and end frequencies must be positive."),
                                      ((100.0, -1.0), "Invalid input: Start and end frequencies must be positive."),
                                      ((500.0, 500.0), "Invalid input: Start frequency must be less than end frequency."),
                                      ((500.0, 100.0), "Invalid input: Start frequency must be less than end frequency."),
                                      ((100.0, 8000.5), "Invalid input: End frequency must be less than Nyquist frequency."),
                                      ((100.0, math.inf), "Invalid input: End frequency must be less than Nyquist frequency."),
                                      ((math.nan, 100.0), "Invalid input: Start and end frequencies must be finite."),
                                      ((100.0, math.nan), "Invalid input: Start and end frequencies must be finite."),
                                      ((10.0, 12.0), "Invalid input: Frequency range should have at least one bin")])
def test_validation_texts(kind, band, msg):
    with pytest.raises(sg.InvalidInputError) as e:
        bparams(kind, 1024, 256, band)
    assert str(e.value) == msg


def test_refusals_at_the_c_abi():
    L = _ffi.lib()
    from spectrograms_amd.binaural import _stft_struct
    import ctypes as C
    sp, _ = _stft_struct(spec_params(1024, 256), _ffi.F32, HOST)
    h = C.c_void_p()
    bp = _ffi.SgxBinauralParams(_ffi.BINAURAL_ITD, 100.0, 500.0, 0, 0)
    assert L.sgx_binaural_create(C.byref(sp), C.byref(bp), C.byref(h)) == _ffi.SGX_INVALID_INPUT and not h.value
    assert b"magphase_power" in L.sgx_binaural_last_error(None)
    bp = _ffi.SgxBinauralParams(7, 100.0, 500.0, 1, 0)
    assert L.sgx_binaural_create(C.byref(sp), C.byref(bp), C.byref(h)) == _ffi.SGX_INVALID_INPUT
    sp.n_fft = 0  # an sgx_plan_create check
    bp = _ffi.SgxBinauralParams(_ffi.BINAURAL_ITD, 100.0, 500.0, 1, 0)
    assert L.sgx_binaural_create(C.byref(sp), C.byref(bp), C.byref(h)) != _ffi.SGX_OK
    # a host-only plan validates and shapes but does not compute
    plan = BinauralPlan(bparams("ild", 1024, 256), "float32", HOST)
    assert plan.device == HOST
    with pytest.raises(sg.FFTBackendError):
        plan.compute(np.zeros(4096, np.float32), np.zeros(4096, np.float32))
    with pytest.raises(sg.DimensionMismatchError):
        plan.compute(np.zeros(4096, np.float32), np.zeros(4095, np.float32))
    with pytest.raises(sg.DimensionMismatchError):
        sg.compute_ild_spectrogram([np.zeros(4096), np.zeros(4000)], bparams("ild", 1024, 256))


@pytest.mark.parametrize("n_fft,f0,f1,expect", [
    (1024, 1.5 * 15.625, 10.5 * 15.625, (2, 11)),   # x.5 rounds away from zero (NumPy's round would give 2, 10)
    (1024, 2.5 * 15.625, 3.5 * 15.625, (3, 4)),
    (1000, 0.5 * 16.0, 500 * 16.0, (1, 500)),
    (256, 50.0, 620.0, (1, 10)),
    (1024, 1700.0, 4600.0, (109, 294)),
    (1001, 16000.0 / 1001 * 0.4, 8000.0, (0, 501)),  # an odd n_fft: the Nyquist end rounds to the last bin + 1
])
def test_band_rounding(n_fft, f0, f1, expect):
    assert bins_of(n_fft, f0, f1) == expect
    plan = BinauralPlan(bparams("itd", n_fft, n_fft // 4, (f0, f1)), "float64", HOST)
    sb, nb, _ = plan.output_shape(4 * n_fft)
    assert (sb, sb + nb) == expect


def test_axes():
    plan = BinauralPlan(bparams("ild", 1024, 256), "float32", HOST)
    sb, nb, nf = plan.output_shape(16000)
    assert nf == 16000 // 256 + 1
    f, t = plan.axes(nf)
    bw = SR / 1024
    assert np.array_equal(f, np.arange(sb, sb + nb) * bw)
    assert np.array_equal(t, np.arange(nf) * 256.0 / SR)


def test_route_names():
    for hop in (160, 255, 256, 512):  # f32 n_fft 1024: the fused route at every hop
        for kind in KINDS:
            assert BinauralPlan(bparams(kind, 1024, hop), "float32", HOST).kernel_name == FUSED
    for dtype, n_fft, hop in [("float64", 1024, 256), ("float32", 2048, 512), ("float32", 1000, 250), ("float64", 512, 128)]:
        plan = BinauralPlan(bparams("itd", n_fft, hop), dtype, HOST)
        mono = sg.Plan(spec_params(n_fft, hop), _ffi.AMP_COMPLEX, dtype=dtype, device=HOST).kernel_name
        assert plan.kernel_name == "binaural_epilogue/" + mono, (plan.kernel_name, mono)
    assert BinauralPlan(bparams("itd", 1024, 256), "float64", HOST).kernel_name == "binaural_epilogue/d32x16_f64"


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_matches_literal_loops(kind):
    rng = np.random.default_rng(3)
    XL = rng.standard_normal((6, 5)) + 1j * rng.standard_normal((6, 5))
    XR = rng.standard_normal((6, 5)) + 1j * rng.standard_normal((6, 5))
    XR[1, 2] = 0.0
    XL[2, 3] = 0.0
    XL[3, 1] = XR[3, 1] = 0.0
    XL[4, 4] = complex(np.nan, 0.0)
    XR[5, 0] = -XL[5, 0]
    bw = SR / 64
    for kw in ([{"wrapped": False}, {"wrapped": True}] if kind == "ipd" else [{"power": 1}, {"power": 2}, {"power": 5}] if kind == "itd"
               else [{}]):
        for sb in ((0, 3) if kind == "itd" else (3,)):
            t = truth(kind, XL, XR, np.arange(sb, sb + 6), bw, **kw)
            lit = literal(kind, XL, XR, sb, bw, **kw)
            assert np.array_equal(np.isnan(t), np.isnan(lit)), (kw, sb)
            m = np.isfinite(lit)
            assert np.array_equal(np.isinf(t), np.isinf(lit)) and np.allclose(t[m], lit[m], rtol=1e-14, atol=1e-15), (kw, sb)
    if kind == "itd":
        assert truth(kind, XL, XR, np.arange(6), bw)[4, 4] == 0.0  # a NaN spectrum gives ITD 0
    if kind in ("ild", "ilr"):
        assert np.isnan(truth(kind, XL, XR, np.arange(6), bw)[[1, 2, 3, 4], [2, 3, 1, 4]]).all()


def test_histogram_restatement_edge_cases():
    v = np.array([[np.nan, -1.0, 0.0, 1.0, 0.999999, np.inf, -np.inf, 2.0, -1.0000001, 0.5]]).T  # one frame
    h = hist_truth(v, 4, -1.0, 1.0)
    # -1 -> bin 0; 0 -> bin 2; 1 == hi -> floor(4) clamped to 3; 0.999999 -> 3; 0.5 -> 3; NaN / +-Inf / out of range skipped
    assert h[:, 0].tolist() == [1.0, 0.0, 1.0, 3.0]
    assert hist_truth(v, 4, -1.0, 1.0, exponent=3)[:, 0].tolist() == [1.0, 0.0, 1.0, 27.0]
    assert hist_truth(v, 4, -1.0, 1.0, exponent=0)[:, 0].tolist() == [1.0, 1.0, 1.0, 1.0]  # 0^0 = 1
    e = np.full((3, 2), np.nan)
    e[:, 1] = [0.1, 0.2, 0.9]
    n = hist_truth(e, 2, 0.0, 1.0, normalize=True)
    assert n[:, 0].tolist() == [0.0, 0.0] and n[:, 1].tolist() == [2.0 / 3.0, 1.0 / 3.0]  # an all-empty column stays 0
    n3 = hist_truth(e, 2, 0.0, 1.0, exponent=3, normalize=True)
    assert np.allclose(n3[:, 1], [8.0 / 9.0, 1.0 / 9.0]) and n3[:, 0].tolist() == [0.0, 0.0]


# ---- GPU tests -------------------------------------------------------------------------------------------------------------------------
N_FFTS = [256, 512, 1000, 1024, 2048]


def hops(n_fft):
    return [n_fft // 4, n_fft // 4 + 1 if (n_fft // 4) % 2 == 0 else n_fft // 4 + 2]


PARITY = [(k, d, n, h) for k in KINDS for d in ("float32", "float64") for n in N_FFTS for h in hops(n)]


def bands(kind, n_fft):
    bw = SR / n_fft
    out = [None, (bw, SR / 2)]
    if kind == "itd":
        out.append((0.3 * bw, 40 * bw))
    return out


def circ(e, period):
    e = np.mod(np.abs(e), period)
    return np.minimum(e, period - e)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARITY, ids=lambda c: f"{c[0]}-{c[1][5:]}-{c[2]}-{c[3]}")
def test_gpu_parity_within_the_per_frame_bound(case):
    kind, dtype, n_fft, hop = case
    nf = 23
    n = hop * (nf - 1)
    L, R = stereo(dtype, 2, n, seed=n_fft + hop)
    w = window(n_fft, hop)
    u = U[dtype]
    for band in bands(kind, n_fft):
        kw = {"wrapped": True} if kind == "ipd" and band is None else {}
        pr = bparams(kind, n_fft, hop, band, **kw)
        plan = BinauralPlan(pr, dtype)
        got = plan.compute(L, R).astype(np.float64)
        sb, nb, nfr = plan.output_shape(n)
        name = route_of(plan)
        assert got.shape == (2, nb, nfr) and nfr == nf
        k = np.arange(sb, sb + nb)
        XL = np.stack([H.np_stft(r, n_fft, hop, w) for r in L.astype(np.float64)])[:, sb:sb + nb]
        XR = np.stack([H.np_stft(r, n_fft, hop, w) for r in R.astype(np.float64)])[:, sb:sb + nb]
        d = frame_deltas(L.astype(np.float64), w, n_fft, hop, dtype, name)[:, None, :]
        dR = frame_deltas(R.astype(np.float64), w, n_fft, hop, dtype, name)[:, None, :]
        with np.errstate(all="ignore"):
            rl, rr = d / np.abs(XL), dR / np.abs(XR)
        t = truth(kind, XL, XR, k, SR / n_fft, **kw)
        good = (rl <= 1e-2) & (rr <= 1e-2)
        if kind == "itd" and sb == 0:  # bin 0 divides by zero: +-Inf or NaN wherever the intensity is > 0
            assert not np.isfinite(got[:, 0, :][np.abs(XL[:, 0, :]) + np.abs(XR[:, 0, :]) > 0]).any()
            good[:, 0, :] = False
        frac = good.mean()
        assert frac >= 0.9, (case, band, name, frac)
        bound_phase = 1.01 * (rl + rr) + 16 * u * math.pi
        if kind == "ipd":
            err = circ(got - t, 2 * math.pi)
            bound = bound_phase
        elif kind == "itd":
            s = 2 * math.pi * (SR / n_fft) * k[None, :, None]
            err = circ((got - t) * s, 2 * math.pi)
            bound = bound_phase + 8 * u * np.abs(t) * s
        elif kind == "ild":
            err = np.abs(got - t)
            bound = (20 / math.log(10)) * 1.01 * (rl + rr) + 8 * u * np.abs(t)
        else:
            err = np.abs(got - t)
            bound = 1.01 * (rl + rr) + 8 * u
        bad = good & ~(err <= bound)
        assert not bad.any(), (case, band, name, float(np.max(np.where(good, err / bound, 0))))


def masked_pair(dtype, n_fft, hop, nf, bad_value, where):
    """Right channel exactly zero over a stretch of ~3 frames; one non-finite sample in the left channel at `where` (a sample index)."""
    n = hop * (nf - 1)
    L, R = stereo(dtype, 2, n, seed=11)
    z0 = hop * (nf // 2)
    R[:, z0:z0 + 3 * n_fft] = 0.0
    Lb = L.copy()
    Lb[1, where] = bad_value
    return L, Lb, R


def reach(n_fft, hop, nf, s):
    """frames whose (centred) window covers sample s"""
    pad = n_fft // 2
    return np.array([f for f in range(nf) if f * hop - pad <= s < f * hop - pad + n_fft])


MASK_CASES = [("float32", 1024, 256), ("float32", 1024, 255), ("float64", 1024, 256), ("float32", 512, 128), ("float64", 512, 128),
              ("float32", 2048, 512), ("float32", 1000, 250), ("float64", 401, 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", MASK_CASES, ids=lambda c: f"{c[0][5:]}-{c[1]}-{c[2]}")
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_masks_and_locality(case, kind):
    dtype, n_fft, hop = case
    sidx = hop * 7 + 3
    L, Lb, R = masked_pair(dtype, n_fft, hop, 41, np.nan, sidx)
    w = window(n_fft, hop)
    pr = bparams(kind, n_fft, hop, (SR / n_fft, SR / 2))
    plan = BinauralPlan(pr, dtype)
    name = route_of(plan)
    pair = paired(name, dtype, n_fft)
    sb, nb, nf = plan.output_shape(L.shape[1])  # (an odd n_fft's centring may give one frame fewer)
    clean = plan.compute(L, R)
    got = plan.compute(Lb, R)
    XL = np.stack([H.np_stft(r, n_fft, hop, w) for r in Lb.astype(np.float64)])[:, sb:sb + nb]
    XR = np.stack([H.np_stft(r, n_fft, hop, w) for r in R.astype(np.float64)])[:, sb:sb + nb]
    t = truth(kind, XL, XR, np.arange(sb, sb + nb), SR / n_fft)
    # frames whose class (right all zero, left non-finite) differs from their partner's are exempt on pairing routes
    zR = np.all(XR == 0, axis=1)
    nL = ~np.all(np.isfinite(XL), axis=1)
    keep = np.ones_like(zR)
    if pair:
        idx = np.arange(nf) ^ 1
        idx[idx >= nf] = np.arange(nf)[idx >= nf]
        keep = (zR == zR[:, idx]) & (nL == nL[:, idx])
    K = np.broadcast_to(keep[:, None, :], t.shape)
    assert zR.any() and nL[1].any()
    if kind == "itd":
        assert np.array_equal((got == 0)[K], (t == 0)[K])
    else:
        assert np.array_equal(np.isnan(got)[K], np.isnan(t)[K]), (name, np.argwhere(np.isnan(got) != np.isnan(t)))
    # locality: frames outside the bad sample's reach (and, on pairing routes, its partner) equal the run with the clean sample
    r = reach(n_fft, hop, nf, sidx)
    hit = set(r.tolist()) | ({f ^ 1 for f in r if (f ^ 1) < nf} if pair else set())
    out = [f for f in range(nf) if f not in hit]
    assert np.array_equal(got[:, :, out], clean[:, :, out], equal_nan=True)
    assert np.array_equal(got[0], clean[0], equal_nan=True)
    # +-Inf at the same sample: the same locality
    for v in (np.inf, -np.inf):
        _, Li, _ = masked_pair(dtype, n_fft, hop, 41, v, sidx)
        gi = plan.compute(Li, R)
        assert np.array_equal(gi[:, :, out], clean[:, :, out], equal_nan=True)


ID_CASES = [("float32", 1024, 256), ("float32", 1024, 160), ("float64", 1024, 256), ("float32", 512, 128), ("float64", 512, 160),
            ("float32", 2048, 512), ("float64", 2048, 512), ("float32", 400, 160), ("float64", 400, 160), ("float32", 401, 160),
            ("float32", 4096, 1024), ("float32", 16, 4), ("float64", 15, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ID_CASES, ids=lambda c: f"{c[0][5:]}-{c[1]}-{c[2]}")
def test_gpu_identical_channels(case):
    dtype, n_fft, hop = case
    T = NP[dtype]
    L, _ = stereo(dtype, 2, hop * 30 + n_fft, seed=5)
    pi = T(np.pi)
    two_pi = T(2) * pi
    wrap0 = np_mod(T(0) + pi, two_pi) - pi  # the reference's wrap of a zero difference, in T (f32: -2^-22, f64: 0)
    for kind in KINDS:
        pr = bparams(kind, n_fft, hop, (SR / n_fft, SR / 2), **({"wrapped": False} if kind == "ipd" else {}))
        plan = BinauralPlan(pr, dtype)
        sb, nb, _ = plan.output_shape(L.shape[1])
        g = plan.compute(L, L)
        X = np.stack([H.np_stft(r, n_fft, hop, window(n_fft, hop)) for r in L.astype(np.float64)])[:, sb:sb + nb]
        nz = np.abs(X) > 1e-6 * np.abs(X).max()
        if kind == "ipd":
            assert np.all(g == 0)
        elif kind == "itd":
            k = np.arange(sb, sb + nb, dtype=T)[None, :, None]
            expect = np.broadcast_to(wrap0 / (two_pi * T(SR / n_fft) * k), g.shape)
            assert np.array_equal(g[nz], expect[nz]), plan.kernel_name
        else:
            assert np.all(g[nz] == 0) and np.all(np.signbit(g[nz])), (kind, plan.kernel_name)


ROUTE_CASES = [("float32", 256, 2.0), ("float32", 160, 2.0), ("float32", 255, 3.0), ("float32", 400, 2.0), ("float32", 512, 3.0),
               ("float32", 256, 0.1), ("float64", 256, 2.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROUTE_CASES, ids=lambda c: f"{c[0][5:]}-{c[1]}-{c[2]}s")
def test_gpu_fused_against_own_spectra(case):
    """The fused route (f32 n_fft 1024: hop 256, the staged form at 160 / 255, the per-lane loads at 400 / 512; several seconds, and a
    short signal) equals the kind function applied in f64 to the library's own complex STFT of each channel (`Plan`, complex amplitude),
    within the epilogue's rounding alone: magnitude, sqrt and division a few ulp, atan2 4 ulp of pi, log10 a few ulp; at bins with
    |X| >= 1e-3 max |X| of the frame.  The f64 case holds the generic route to the same."""
    dtype, hop, seconds = case
    n_fft = 1024
    u = U[dtype]
    L, R = stereo(dtype, 3, int(16000 * seconds), seed=9 + hop)
    cplx = sg.Plan(spec_params(n_fft, hop), _ffi.AMP_COMPLEX, dtype=dtype)
    XL = np.asarray(cplx.compute_batch(L)).astype(np.complex128)
    XR = np.asarray(cplx.compute_batch(R)).astype(np.complex128)
    for kind in KINDS:
        pr = bparams(kind, n_fft, hop, (SR / n_fft, SR / 2), **({"wrapped": True} if kind == "ipd" else {}))
        plan = BinauralPlan(pr, dtype)
        assert plan.kernel_name == (FUSED if dtype == "float32" else "binaural_epilogue/d32x16_f64")
        sb, nb, _ = plan.output_shape(L.shape[1])
        g = plan.compute(L, R).astype(np.float64)
        xl, xr = XL[:, sb:sb + nb], XR[:, sb:sb + nb]
        k = np.arange(sb, sb + nb)
        t = truth(kind, xl, xr, k, SR / n_fft, **({"wrapped": True} if kind == "ipd" else {}))
        m = (np.abs(xl) >= 1e-3 * np.abs(XL).max(axis=1, keepdims=True)) & (np.abs(xr) >= 1e-3 * np.abs(XR).max(axis=1, keepdims=True))
        if kind == "ipd":
            err, tol = circ(g - t, 2 * math.pi), 16 * u * math.pi
        elif kind == "itd":
            s = 2 * math.pi * (SR / n_fft) * k[None, :, None]
            err, tol = circ((g - t) * s, 2 * math.pi), 16 * u * math.pi + 8 * u * np.abs(t) * s
        elif kind == "ild":
            err, tol = np.abs(g - t), 8 * u * (np.abs(t) + 20 / math.log(10))
        else:
            err, tol = np.abs(g - t), 8 * u
        assert np.all((err <= tol)[m]), (kind, float(np.max(np.where(m, err / tol, 0))))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_gpu_bit_equality(dtype):
    import torch
    n_fft, hop, n = 1024, 256, 16000 * 3
    L, R = stereo(dtype, 129, n, seed=2)
    plan = BinauralPlan(bparams("itd", n_fft, hop), dtype)
    assert plan.kernel_name == (FUSED if dtype == "float32" else "binaural_epilogue/d32x16_f64")
    full = plan.compute(L, R)
    assert np.array_equal(full, plan.compute(L, R), equal_nan=True)  # repeat launch
    for i in (0, 1, 64, 128):
        assert np.array_equal(full[i], plan.compute(L[i], R[i]), equal_nan=True)  # batch 1
    assert np.array_equal(full[5:17], plan.compute(L[5:17], R[5:17]), equal_nan=True)  # position and size
    for kind in ("ipd", "ild", "ilr"):
        p2 = BinauralPlan(bparams(kind, n_fft, hop), dtype)
        a = p2.compute(L[:7], R[:7])
        ld, rd = torch.from_numpy(L[:7]).cuda(), torch.from_numpy(R[:7]).cuda()
        tdev = p2.compute_torch(ld, rd)
        torch.cuda.synchronize()
        assert np.array_equal(a, tdev.cpu().numpy(), equal_nan=True)  # host against device memory, torch against NumPy
        out = torch.empty_like(tdev)
        p2.compute_torch(ld, rd, out=out)
        torch.cuda.synchronize()
        assert torch.equal(torch.nan_to_num(out), torch.nan_to_num(tdev))
    one = sg.compute_itd_spectrogram(np.stack([L[3], R[3]]), bparams("itd", n_fft, hop), dtype=dtype)
    assert np.array_equal(np.asarray(one), full[3], equal_nan=True) and one.dtype == dtype


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_histograms(dtype, kind):
    n_fft, hop = 1024, 256
    L, R = stereo(dtype, 1, 16000, seed=4)
    pr = bparams(kind, n_fft, hop)
    spec = {"itd": sg.compute_itd_spectrogram, "ipd": sg.compute_ipd_spectrogram, "ild": sg.compute_ild_spectrogram,
            "ilr": sg.compute_ilr_spectrogram}[kind]([L[0], R[0]], pr, dtype=dtype)
    assert spec.shape == (spec.n_bins, spec.n_frames) and spec.dtype == dtype
    assert spec.frequency_range() == (spec.frequencies[0], spec.frequencies[-1])
    assert spec.duration() == pytest.approx(spec.times[-1]) and spec.params is pr
    data = spec.data.copy()
    data[0, 0] = np.nan
    data[1, 1] = RANGES[kind][1]  # v == hi
    data[2, 2] = RANGES[kind][1] * 2  # out of range
    data[:, 3] = np.nan  # an all-empty column
    plan = BinauralPlan(pr, dtype)
    lo, hi = RANGES[kind]
    for nbins, exponent, norm in [(400, 1, False), (400, 1, True), (37, 3, False), (37, 3, True), (400, 0, True), (5, 2, True)]:
        got = plan.histogram(data, nbins, lo, hi, exponent, norm)
        ref = hist_truth(data, nbins, lo, hi, exponent, norm)
        counts = hist_truth(data, nbins, lo, hi)
        assert np.array_equal(plan.histogram(data, nbins, lo, hi), counts)  # counts exact
        assert np.all(np.abs(got - ref) <= 4 * 2.0 ** -52 * nbins * np.abs(ref)), (nbins, exponent, norm)
    # the result objects' own histogram (default bins, range, exponent)
    h = spec.histogram(normalize=True)
    ref = hist_truth(spec.data, 400, lo, hi, 1 if kind in ("itd", "ipd") else 3, True)
    assert h.shape == (400, spec.n_frames) and np.all(np.abs(h - ref) <= 4 * 2.0 ** -52 * 400 * np.abs(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_gpu_diffs(dtype):
    T = NP[dtype]
    n_fft, hop = 1024, 256
    L, R = stereo(dtype, 2, 16000, seed=6)
    ref_a, test_a = [L[0], R[0]], [L[1], R[1]]
    p = bparams("itd", n_fft, hop)
    m, deg, med = sg.compute_itd_spectrogram_diff(ref_a, test_a, p, dtype=dtype)
    d = sg.compute_itd_spectrogram(test_a, p, dtype=dtype).data - sg.compute_itd_spectrogram(ref_a, p, dtype=dtype).data
    cm = d.sum(axis=0) / T(d.shape[0])
    assert np.array_equal(m, cm)
    assert deg == pytest.approx(float(np.mean(np.abs(cm.astype(np.float64)) / 0.00086 * 90.0)), rel=1e-5)
    assert med == pytest.approx(float(np.median(cm[np.isfinite(cm)].astype(np.float64))), rel=1e-5)
    q = bparams("ilr", n_fft, hop)
    m2, mean2 = sg.compute_ilr_spectrogram_diff(ref_a, test_a, q, dtype=dtype)
    d2 = (sg.compute_ilr_spectrogram(test_a, q, dtype=dtype).data - sg.compute_ilr_spectrogram(ref_a, q, dtype=dtype).data).astype(np.float64)
    with np.errstate(all="ignore"):
        cm2 = np.nanmean(d2, axis=0)
    assert np.allclose(m2, cm2, rtol=1e-5, atol=1e-6, equal_nan=True)
    assert mean2 == pytest.approx(float(np.nanmean(np.abs(cm2))), rel=1e-5)
