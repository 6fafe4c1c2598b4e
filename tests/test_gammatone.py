"""Gammatone IIR spectrogram plans (spectrograms_amd.gammatone, sgx_gammatone_*) against a NumPy restatement of src/erb.rs:405-654.

The restatement below is the definition written out again (centre frequencies, coefficients, the N - 1 Hann window, four Direct Form II
transposed sections from zero state, root mean square, dB floor), vectorised over (frames, bands) with a Python loop over the samples, and
runs in np.float64 and in np.longdouble.  It reads nothing but this file and tests/helpers.py.

Coefficients (CPU): per band the plain-f64 restatement's distance from the long-double one is measured over the band's 11 values; the
plan is allowed 8 times that, floor 2^-49 (16 ulp) -- the gain's x5 cancels its leading terms for low bands, so two correct f64
evaluations differ by far more than an ulp there, and the margin is for another libm and FMA contraction on the same formula.

Kernel (GPU): every output element, against the long-double recurrence on the plan's own coefficients (coefficients()) and the f64
windowed frames.  Per band, s_band = the larger relative deviation (over the band's frames) from the long-double result of two f64
restatements, `a1 x + z1 - b1 y` as the reference writes it and `(a1 x - b1 y) + z1`: what reordering and contraction of correct f64
arithmetic do to this recurrence on this input.  f64 plans get 8 s_band with a floor of 2^-46, f32 plans the same plus 2^-23 for the
rounding of their output (the inputs of every case are f32 values, fed exactly to both sides).  With a dB floor: |difference in dB| <=
10 / ln 10 times that bound plus 4 ulp of the dB value in T; where the long-double value lies below eps by more than the bound the output
must be T(db_floor) exactly (for the floors used 10 log10(T(10^(floor / 10))) rounds to T(floor), asserted in long double).
s_band stays below 1e-9 for every band of every case here but the four of S_BAND_ABOVE_1E9 (asserted and printed by
test_s_band_is_small on the CPU): the bands centred at 0 Hz (speech_standard at 16 kHz, 4.2e-8) and at 50, 68 and 88 Hz at 48 kHz (5.6e-9,
3.5e-9, 1.9e-9), whose four pole pairs lie within 1 - E ~ 0.005 of z = 1.  Those inputs are kept and the factor 8 with them;
what the bound is meant to exclude (a wrong sign, a swapped section, a state that is not reset, f32 arithmetic) errs by 1e-4 or more.

Worst ratios to the bound measured on an MI355X (error / bound, largest over a case's elements):
  f64 plans  0.265 (hop_gt_frame), 0.184 (48k_tr35_64), 0.146 (long_frame_40000), 0.142 (16k_speech_40), every other case <= 0.123
  f32 plans  0.43 .. 0.50 in every case (the output rounding: half an ulp of 2^-24 against the 2^-23 allowed)
  frame_2    0 (the N - 1 window of two samples is all zero, the output is exactly 0)
  dB         f32 0.415, f64 0.183 (both floors)
  coefficients (CPU)  <= 0.28 in every case
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests import helpers as H

HOST = _ffi.DEVICE_HOST_ONLY
NP = {"float32": np.float32, "float64": np.float64}
LD = np.longdouble
_PI_LD = LD("3.14159265358979323846264338327950288")
WORST = {}


def _record(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    print(f"{name}: worst ratio to bound {WORST[name]:.3g}")


# ---- restatement ---------------------------------------------------------------------------------------------------------------
def np_centres(n, f_min, f_max, spacing):
    return H.np_erb(16000.0, 16, n, f_min, f_max, 1 if spacing == "apple_tr35" else 0)[1]


def _cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def np_gain(cf, bval, t, dt):
    """iir_gain: complex values as (re, im) pairs of dt arrays, product / quotient / norm written out."""
    pi = _PI_LD if dt is LD else dt(np.pi)
    two = dt(2)
    angle = two * pi * cf * t
    cos1, sin1 = np.cos(angle), np.sin(angle)
    xe = (np.cos(two * angle), np.sin(two * angle))
    ebt = np.exp(-bval * t)
    x01 = (xe[0] * (-two * t), xe[1] * (-two * t))
    k02 = two * t * ebt
    x02 = (cos1 * k02, sin1 * k02)
    s1, s2 = np.sqrt(dt(3) - two * np.sqrt(two)), np.sqrt(dt(3) + two * np.sqrt(two))

    def xk(f):
        return (x01[0] + x02[0] * f, x01[1] + x02[1] * f)

    x1, x2, x3, x4 = xk(cos1 - s1 * sin1), xk(cos1 + s1 * sin1), xk(cos1 - s2 * sin1), xk(cos1 + s2 * sin1)
    e2 = ebt * ebt
    x5 = (-two * e2 - xe[0] * two + (dt(1) + xe[0]) * (two * ebt), -(xe[1] * two) + xe[1] * (two * ebt))
    num = _cmul(_cmul(_cmul(x1, x2), x3), x4)
    sq = _cmul(x5, x5)
    den = _cmul(sq, sq)
    n2 = den[0] * den[0] + den[1] * den[1]
    q = ((num[0] * den[0] + num[1] * den[1]) / n2, (num[1] * den[0] - num[0] * den[1]) / n2)
    return np.hypot(q[0], q[1])


def np_coeffs(cf64, sample_rate, dt):
    """make_iir_bank on given centre frequencies: (n_bands, 11) = a0_1, a1_1 (over the gain), a0_2, a1_2, a0_3, a1_3, a0_4, a1_4, b1, b2, gain."""
    cf = np.asarray(cf64, np.float64).astype(dt)
    pi = _PI_LD if dt is LD else dt(np.pi)
    two = dt(2)
    t = dt(1) / dt(sample_rate)
    erb = cf / dt(np.float64(9.26449)) + dt(np.float64(24.7))
    bval = dt(np.float64(1.019)) * two * pi * erb
    ebt = np.exp(-bval * t)
    angle = two * pi * cf * t
    cos1, sin1 = np.cos(angle), np.sin(angle)
    b1, b2 = -two * cos1 * ebt, np.exp(-two * bval * t)
    s1, s2 = np.sqrt(dt(3) - two * np.sqrt(two)), np.sqrt(dt(3) + two * np.sqrt(two))
    bsin = sin1 * t
    a11, a12 = -ebt * (t * cos1 + bsin * s2), -ebt * (t * cos1 - bsin * s2)
    a13, a14 = -ebt * (t * cos1 + bsin * s1), -ebt * (t * cos1 - bsin * s1)
    gain = np_gain(cf, bval, t, dt)
    a0 = np.full_like(cf, t)
    return np.stack([a0 / gain, a11 / gain, a0, a12, a0, a13, a0, a14, b1, b2, gain], axis=1)


def np_frames(x, frame, hop):
    """f64 windowed frames of the rows of x [batch][n] -> [batch * n_frames][frame], window 0.5 - 0.5 cos(2 pi i / (frame - 1))."""
    x = np.atleast_2d(np.asarray(x)).astype(np.float64)
    nf = 1 + (x.shape[1] - frame) // hop
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(frame, dtype=np.float64) / np.float64(frame - 1))
    idx = np.arange(nf)[:, None] * hop + np.arange(frame)[None, :]
    return (x[:, idx] * w).reshape(-1, frame), nf


def np_rms(frames64, coef64, dt, order=0):
    """The four cascaded sections and the root mean square, in dt: [n_rows][n_bands].  order 0: z0 = a1 x + z1 - b1 y (the reference);
    order 1: z0 = (a1 x - b1 y) + z1."""
    fr = frames64.astype(dt)
    c = coef64.astype(dt)
    R, N = fr.shape
    B = c.shape[0]
    a0 = [c[None, :, 2 * k] for k in range(4)]
    a1 = [c[None, :, 2 * k + 1] for k in range(4)]
    b1, b2 = c[None, :, 8], c[None, :, 9]
    z0 = [np.zeros((R, B), dt) for _ in range(4)]
    z1 = [np.zeros((R, B), dt) for _ in range(4)]
    acc = np.zeros((R, B), dt)
    for i in range(N):
        x = fr[:, i:i + 1]
        for k in range(4):
            y = a0[k] * x + z0[k]
            if order == 0:
                z0[k] = a1[k] * x + z1[k] - b1 * y
            else:
                z0[k] = (a1[k] * x - b1 * y) + z1[k]
            z1[k] = -b2 * y
            x = y
        acc = acc + x * x
    return np.sqrt(acc / dt(N))


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def _erb(n, lo, hi, spacing="linear"):
    return sg.ErbParams(n, lo, hi, spacing)


# name: (sample_rate, frame, hop, ErbParams, batch, n_frames)
CASES = {
    "48k_tr35_64": (48000.0, 3840, 960, _erb(64, 50.0, 16000.0, "apple_tr35"), 2, 6),
    "16k_speech_40": (16000.0, 1280, 320, sg.ErbParams.speech_standard(), 3, 7),  # 280 pairs per signal: a partial last workgroup
    "16k_400_160_32": (16000.0, 400, 160, _erb(32, 100.0, 7000.0), 1, 12),
    "music_standard": (44100.0, 1024, 512, sg.ErbParams.music_standard(44100.0), 2, 5),  # f_max at Nyquist
    "long_frame_40000": (44100.0, 40000, 12345, _erb(16, 80.0, 12000.0, "apple_tr35"), 1, 2),  # 20 LDS chunks per frame
    "frame_2": (8000.0, 2, 1, _erb(8, 100.0, 3000.0), 2, 30),
    "frame_3": (8000.0, 3, 2, _erb(8, 100.0, 3000.0), 2, 30),
    "hop_1": (16000.0, 64, 1, _erb(8, 200.0, 6000.0), 2, 41),
    "hop_gt_frame": (22050.0, 200, 333, _erb(24, 60.0, 9000.0, "apple_tr35"), 2, 4),
    "bands_2_many_frames": (16000.0, 256, 7, _erb(2, 300.0, 3000.0), 2, 300),  # 128 frames per workgroup, 30-sample chunks
    "bands_63": (16000.0, 256, 128, _erb(63, 50.0, 7500.0, "apple_tr35"), 2, 9),
    "bands_65": (16000.0, 256, 128, _erb(65, 50.0, 7500.0), 2, 9),
    "bands_200": (16000.0, 256, 128, _erb(200, 20.0, 7900.0), 2, 5),
    "one_frame": (16000.0, 512, 128, _erb(40, 0.0, 8000.0), 3, 1),
    "f_max_above_nyquist": (8000.0, 300, 100, _erb(12, 100.0, 6000.0), 1, 4),
}
TONE_CASES = ("48k_tr35_64", "16k_speech_40")


def case_n_samples(name):
    _, frame, hop, _, _, nf = CASES[name]
    return frame + hop * (nf - 1) + (hop - 1) // 2  # a tail that adds no frame


@functools.lru_cache(maxsize=None)
def case_input(name, quiet=1e-4):
    """f32-valued noise whose first third is `quiet` times the rest (bands and frames of very different level); in the tone cases the last
    row is a tone at a centre frequency instead."""
    sr, frame, hop, erb, batch, nf = CASES[name]
    n = case_n_samples(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    x = 0.25 * rng.standard_normal((batch, n))
    x[:, :(max(n // 3, frame) if nf > 1 else n // 3)] *= quiet  # (the first frame lies wholly in the quiet part)
    if name in TONE_CASES:
        cf = np_centres(erb.n_filters, erb.f_min, erb.f_max, erb.spacing)
        x[-1] = 0.5 * np.sin(2.0 * np.pi * cf[tone_band(name)] * np.arange(n) / sr)
    return x.astype(np.float32)


def tone_band(name):
    return (2 * CASES[name][3].n_filters) // 3


@functools.lru_cache(maxsize=None)
def case_reference(name, quiet=1e-4):
    """(long-double rms [batch][n_bands][n_frames], s_band [n_bands]) on the plan's own coefficients."""
    sr, frame, hop, erb, batch, nf = CASES[name]
    plan = sg.GammatonePlan(sr, frame, hop, erb, device=HOST)
    raw = plan_raw_coeffs(plan)
    fr, nf2 = np_frames(case_input(name, quiet), frame, hop)
    assert nf2 == nf
    ld = np_rms(fr, raw, LD)
    s = np.zeros(erb.n_filters)
    for order in (0, 1):
        d = np_rms(fr, raw, np.float64, order).astype(LD)
        assert np.all(d[ld == 0] == 0)  # (frame_size 2: the window is all zero)
        s = np.maximum(s, np.max(np.abs(d - ld) / np.where(ld > 0, ld, LD(1)), axis=0).astype(np.float64))
    assert np.all(np.isfinite(s))
    return ld.reshape(batch, nf, erb.n_filters).transpose(0, 2, 1), s


def plan_raw_coeffs(plan):
    c = plan.coefficients()
    return np.concatenate([c["a"].reshape(plan.n_bands, 8), c["b1"][:, None], c["b2"][:, None], c["gain"][:, None]], axis=1)


def rel_bound(name, dtype, quiet=1e-4):
    s = case_reference(name, quiet)[1]
    return np.maximum(8.0 * s, 2.0 ** -46) + (2.0 ** -23 if dtype == "float32" else 0.0)


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_error_texts_and_refusals():
    erb = _erb(8, 100.0, 3000.0)
    for sr in (0.0, -1.0, -math.inf):
        with pytest.raises(sg.InvalidInputError, match="sample_rate must be > 0"):
            sg.GammatonePlan(sr, 64, 16, erb, device=HOST)
    plan = sg.GammatonePlan(8000.0, 64, 16, erb, device=HOST)
    with pytest.raises(sg.InvalidInputError, match="signal is shorter than frame_size"):
        plan.output_shape(63)
    with pytest.raises(sg.InvalidInputError, match="signal is shorter than frame_size"):
        plan.compute(np.zeros(63))
    for sr in (math.nan, math.inf):
        with pytest.raises(sg.InvalidInputError, match="sample_rate"):
            sg.GammatonePlan(sr, 64, 16, erb, device=HOST)
    with pytest.raises(sg.InvalidInputError, match="frame_size must be >= 2"):
        sg.GammatonePlan(8000.0, 1, 1, erb, device=HOST)
    for fs, hs in ((0, 1), (64, 0), (-3, 1)):  # NonZeroUsize in the reference
        with pytest.raises(ValueError):
            sg.GammatonePlan(8000.0, fs, hs, erb, device=HOST)
    for floor in (math.nan, math.inf, -math.inf):
        with pytest.raises(sg.InvalidInputError, match="db_floor"):
            sg.GammatonePlan(8000.0, 64, 16, erb.with_db_floor(floor), device=HOST)
    # the raw ABI refuses hop 0 and a single filter too, without a plan
    L, h = _ffi.lib(), C.c_void_p()
    assert L.sgx_gammatone_create(8000.0, 64, 0, 8, 100.0, 3000.0, 0, 0, 0.0, _ffi.F64, HOST, C.byref(h)) == _ffi.SGX_INVALID_INPUT
    assert b"hop_size must be > 0" in L.sgx_gammatone_last_error(None) and not h.value
    assert L.sgx_gammatone_create(8000.0, 64, 16, 1, 100.0, 3000.0, 0, 0, 0.0, _ffi.F64, HOST, C.byref(h)) == _ffi.SGX_INVALID_INPUT
    assert b"n_filters must be >= 2" in L.sgx_gammatone_last_error(None)
    # f_max above Nyquist is not refused here (the reference does not), and a host-only plan refuses to compute
    sg.GammatonePlan(8000.0, 64, 16, _erb(8, 100.0, 7000.0), device=HOST)
    with pytest.raises(sg.FFTBackendError, match="no HIP device"):
        plan.compute(np.zeros(64))
    with pytest.raises(ValueError):
        plan.compute(np.zeros((2, 2, 64)))


@pytest.mark.parametrize("frame,hop,n", [(64, 16, 64), (64, 16, 79), (64, 16, 80), (64, 100, 64), (64, 100, 163), (64, 100, 164), (2, 1, 2),
                                         (3840, 960, 480000), (1280, 320, 160000), (40000, 1, 40007)])
def test_output_shape(frame, hop, n):
    plan = sg.GammatonePlan(16000.0, frame, hop, _erb(40, 0.0, 8000.0), device=HOST)
    assert plan.output_shape(n) == (40, 1 + (n - frame) // hop)
    assert plan.n_bands == 40 and plan.device == -2


@pytest.mark.parametrize("spacing", ["linear", "apple_tr35"])
@pytest.mark.parametrize("n,lo,hi", [(64, 50.0, 16000.0), (40, 0.0, 8000.0), (2, 100.0, 200.0), (200, 20.0, 7900.0), (63, 0.0, 22050.0)])
def test_center_frequencies(spacing, n, lo, hi):
    erb = sg.ErbParams(n, lo, hi, spacing)
    ref = np_centres(n, lo, hi, spacing)
    got = sg.GammatonePlan(16000.0, 64, 16, erb, device=HOST).center_frequencies
    assert got.shape == (n,) and np.all(np.diff(got) > 0)
    assert np.allclose(got, ref, rtol=1e-12, atol=0)
    assert np.array_equal(sg.gammatone_center_frequencies(erb), got)
    # the same axis as the ERB spectrogram plans (when those accept the range)
    if hi <= 8000.0:
        p = sg.SpectrogramParams(sg.StftParams(512, 128, sg.WindowType.hanning, True), 16000.0)
        assert np.array_equal(sg.Plan(p, _ffi.AMP_POWER, erb, None, "float64", device=HOST).axes(1)[0], got)


@pytest.mark.parametrize("name", sorted(CASES))
def test_coefficients_against_long_double(name):
    sr, frame, hop, erb, _, _ = CASES[name]
    plan = sg.GammatonePlan(sr, frame, hop, erb, device=HOST)
    got = plan_raw_coeffs(plan)
    cf = plan.center_frequencies
    ld = np_coeffs(cf, sr, LD)
    f64 = np_coeffs(cf, sr, np.float64).astype(LD)
    dev = np.max(np.abs(f64 - ld) / np.abs(ld), axis=1).astype(np.float64)  # per band, over its 11 values
    tol = np.maximum(8.0 * dev, 2.0 ** -49)
    err = (np.abs(got.astype(LD) - ld) / np.abs(ld)).astype(np.float64)
    ratio = np.max(err / tol[:, None])
    _record(f"coefficients {name}", ratio)
    print(f"  f64 restatement vs long double, worst band: {dev.max():.3g}; plan vs long double: {err.max():.3g}")
    assert ratio <= 1.0
    c = plan.coefficients()
    assert c["a"].shape == (erb.n_filters, 4, 2) and np.all(c["a"][:, 1:, 0] == 1.0 / sr) and np.all(c["b2"] < 1.0)
    assert np.array_equal(c["a"][:, 0, 0], (1.0 / sr) / c["gain"])


def test_erb_params_db_floor_does_not_reach_the_erb_plans():
    erb = sg.ErbParams(40, 50.0, 8000.0, "apple_tr35")
    assert erb.db_floor is None and sg.ErbParams.speech_standard().db_floor is None
    fl = erb.with_db_floor(-80.0)
    assert fl.db_floor == -80.0 and erb.db_floor is None and fl.spacing == "apple_tr35"
    assert fl.with_spacing("linear").db_floor == -80.0 and fl.with_spacing("linear").spacing == "linear"
    assert sg.GammatoneParams is sg.ErbParams
    p = sg.SpectrogramParams(sg.StftParams(512, 128, sg.WindowType.hanning, True), 16000.0)
    a = sg.Plan(p, _ffi.AMP_POWER, erb, None, "float64", device=HOST)
    b = sg.Plan(p, _ffi.AMP_POWER, fl, None, "float64", device=HOST)
    for u, v in zip(a.mel_weights(), b.mel_weights()):
        assert np.array_equal(u, v)
    for u, v in zip(a.axes(5), b.axes(5)):
        assert np.array_equal(u, v)
    assert a.kernel_name == b.kernel_name and a.output_shape(16000) == b.output_shape(16000)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_kernel_name_has_no_fallback(name, dtype):
    sr, frame, hop, erb, _, _ = CASES[name]
    assert sg.GammatonePlan(sr, frame, hop, erb, dtype, device=HOST).kernel_name == "k_gammatone_iir"
    assert sg.GammatonePlan(sr, frame, hop, erb.with_db_floor(-80.0), dtype, device=HOST).kernel_name == "k_gammatone_iir"


# bands whose s_band exceeds 1e-9 (pole pairs next to z = 1: see the module docstring); they stay in, under the same factor
S_BAND_ABOVE_1E9 = {"16k_speech_40": [0], "48k_tr35_64": [0, 1, 2]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_s_band_is_small(name):
    """The kernel bound's premise, on the CPU: s_band < 1e-9 for every case's input (both quiet levels the GPU tests use), but for
    the listed low bands, which stay below 1e-6."""
    for quiet in (1e-4, 1e-10):
        s = case_reference(name, quiet)[1]
        print(f"s_band {name} quiet={quiet:g}: max {s.max():.3g} (band {int(s.argmax())}), median {np.median(s):.3g}")
        above = S_BAND_ABOVE_1E9.get(name, [])
        assert np.all(np.delete(s, above) < 1e-9) and np.all(s < 1e-6)


@pytest.mark.gpu
def test_plan_cache_is_cleared():
    from spectrograms_amd import gammatone as g
    erb = _erb(8, 100.0, 3000.0)
    g._plan(8000.0, 64, 16, erb, "float32")
    g._plan(8000.0, 64, 16, erb.with_db_floor(-60.0), "float32")
    assert len(g._GT_CACHE) == 2
    sg.clear_fft_plan_cache()
    assert len(g._GT_CACHE) == 0


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def _dev(x, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=NP[dtype])).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_kernel_every_element(name, dtype):
    sr, frame, hop, erb, batch, nf = CASES[name]
    x = case_input(name)
    ld, _ = case_reference(name)
    plan = sg.GammatonePlan(sr, frame, hop, erb, dtype)
    assert plan.kernel_name == "k_gammatone_iir"
    assert np.array_equal(plan_raw_coeffs(plan), plan_raw_coeffs(sg.GammatonePlan(sr, frame, hop, erb, device=HOST)))
    out = plan.compute(x.astype(NP[dtype]))
    assert out.shape == (batch, erb.n_filters, nf) and out.dtype == NP[dtype]
    bound = rel_bound(name, dtype)[None, :, None]
    err = (np.abs(out.astype(LD) - ld) / np.where(ld > 0, ld, LD(1))).astype(np.float64)
    ratio = np.max(err / bound)
    _record(f"kernel {name} {dtype}", ratio)
    assert np.all(np.isfinite(out)) and ratio <= 1.0 and np.all(out[ld == 0] == 0)
    if name in TONE_CASES:  # the tone row: in every frame the loudest band is the tone's band or a neighbour
        assert np.all(np.abs(np.argmax(out[-1], axis=0) - tone_band(name)) <= 1)
    one, cf = sg.gammatone_iir_spectrogram(x[0].astype(NP[dtype]), sr, frame, hop, erb, dtype)
    assert np.array_equal(one, out[0]) and np.array_equal(cf, plan.center_frequencies)
    with pytest.raises(sg.InvalidInputError, match="signal is shorter than frame_size"):
        sg.gammatone_iir_spectrogram(x[0, :frame - 1], sr, frame, hop, erb, dtype)
    with pytest.raises(sg.InvalidInputError, match="sample_rate must be > 0"):
        sg.gammatone_iir_spectrogram(x[0, :frame - 1], 0.0, frame, hop, erb, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["48k_tr35_64", "16k_speech_40", "16k_400_160_32", "long_frame_40000", "bands_2_many_frames", "bands_65",
                                  "hop_gt_frame"])
@pytest.mark.parametrize("dtype,floor", [("float32", -80.0), ("float64", -80.0), ("float32", -60.0), ("float64", -60.0)])
def test_kernel_db_floor(name, dtype, floor):
    sr, frame, hop, erb, batch, nf = CASES[name]
    T = NP[dtype]
    quiet = 1e-10  # the quiet third falls below both floors
    x = case_input(name, quiet)
    ld, _ = case_reference(name, quiet)
    eps = T(10.0 ** (floor / 10.0))
    # the floor value of the reference, 10 log10(eps) in T, is T(floor) for these floors
    assert abs(LD(10) * np.log10(LD(eps)) - LD(floor)) < 0.25 * np.spacing(T(abs(floor)))
    out = sg.GammatonePlan(sr, frame, hop, erb.with_db_floor(floor), dtype).compute(x.astype(T))
    assert out.shape == (batch, erb.n_filters, nf) and out.dtype == T
    rb = rel_bound(name, dtype, quiet)[None, :, None]
    ref_db = (LD(10) * np.log10(np.maximum(ld, LD(eps)))).astype(np.float64)
    tol = 10.0 / math.log(10.0) * rb + 4.0 * np.spacing(np.abs(ref_db).astype(T)).astype(np.float64)
    err = np.abs(out.astype(np.float64) - ref_db)
    _record(f"kernel dB {name} {dtype} {floor:g}", np.max(err / tol))
    assert np.max(err / tol) <= 1.0
    below = (ld * (1 + rb.astype(LD))) < LD(eps)
    assert below.any() and (~below).any()
    assert np.all(out[below] == T(floor))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_all_zero_signal(dtype):
    for name in ("16k_speech_40", "bands_63", "long_frame_40000"):
        sr, frame, hop, erb, batch, nf = CASES[name]
        z = np.zeros((batch, case_n_samples(name)), NP[dtype])
        out = sg.GammatonePlan(sr, frame, hop, erb, dtype).compute(z)
        assert out.shape == (batch, erb.n_filters, nf) and np.all(out == 0) and not np.any(np.signbit(out))
        out = sg.GammatonePlan(sr, frame, hop, erb.with_db_floor(-80.0), dtype).compute(z)
        assert np.all(out == NP[dtype](-80.0))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_frame_independence_and_nan(dtype):
    sr, frame, hop, erb, _, nf = CASES["16k_400_160_32"]
    plan = sg.GammatonePlan(sr, frame, hop, erb, dtype)
    x = case_input("16k_400_160_32")[0].astype(NP[dtype])
    base = plan.compute(x)
    rng = np.random.default_rng(5)
    for f in (0, 4, nf - 1):
        y = x.copy()
        outside = np.ones(x.size, bool)
        outside[f * hop:f * hop + frame] = False
        y[outside] = rng.standard_normal(int(outside.sum())).astype(NP[dtype]) * 3
        assert np.array_equal(plan.compute(y)[:, f], base[:, f])
    for pos in (0, frame - 1, frame, 3 * hop + 17, x.size - 1, (nf - 1) * hop + frame - 1):
        y = x.copy()
        y[pos] = np.nan
        got = plan.compute(y)
        cols = np.array([f * hop <= pos < f * hop + frame for f in range(nf)])
        assert np.all(np.isnan(got[:, cols])) and np.array_equal(got[:, ~cols], base[:, ~cols])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["48k_tr35_64", "16k_speech_40", "bands_2_many_frames", "bands_200", "hop_gt_frame", "one_frame"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_batch_invariance_and_torch_entry(name, dtype):
    import torch
    sr, frame, hop, erb, batch, nf = CASES[name]
    plan = sg.GammatonePlan(sr, frame, hop, erb, dtype)
    x = case_input(name).astype(NP[dtype])
    n = x.shape[1]
    out = plan.compute(x)
    for r in range(batch):
        assert np.array_equal(plan.compute(x[r]), out[r])
        assert np.array_equal(plan.compute(x[r:r + 1])[0], out[r])
    xd = _dev(x, dtype)
    t = plan.compute_torch(xd)
    torch.cuda.synchronize()
    assert tuple(t.shape) == out.shape and np.array_equal(t.cpu().numpy(), out)
    # a row stride larger than n_samples, on the device and on the host; the padding holds NaN
    wide = np.full((batch, n + 37), np.nan, NP[dtype])
    wide[:, :n] = x
    assert np.array_equal(plan.compute(wide[:, :n]), out)
    wd = _dev(wide, dtype)
    pre = torch.full(out.shape, 7.0, dtype=xd.dtype, device="cuda")
    assert plan.compute_torch(wd[:, :n], out=pre) is pre
    torch.cuda.synchronize()
    assert np.array_equal(pre.cpu().numpy(), out)
    with pytest.raises(sg.DimensionMismatchError):
        plan.compute_torch(xd, out=torch.empty((batch, erb.n_filters, nf + 1), dtype=xd.dtype, device="cuda"))
    plan.reserve(batch, n)
    assert np.array_equal(plan.compute(x), out)
