"""Frame locality of the forward and inverse STFT routes: every output frame depends on its own n_fft samples only.

The forward kernels share tiles of 8 / 16 / 32 frames, trade data through LDS, put two frames into one complex transform on some routes,
run packed tiles on into the next signal, and the fused MFCC epilogue reads padding steps of the Mel-dB tile.  These tests pin:

1. ROUTES: one case per route (`sgx_kernel_name`, the two CQT names excepted) and output kind, its kernel name asserted.
2. Non-finite reach: one NaN / +Inf / -Inf sample in signal 1 at sample 0, at a tile boundary and at the last sample.  Every output of a
   frame that does not cover it (nor is that frame's documented partner, PAIRED) is bit-identical to the same plan's output with a 0
   there, in every signal.  NaN inputs follow the oracle's masks (and its floor for dB / MFCC); +-Inf poisons every bin of the
   covering frames and never makes a dB value NaN.  The oracle's own non-finite semantics are pinned on the CPU against NumPy.
3. Per-frame precision under level steps (rows 10^4 ... 10^10 apart, and a row switching between 1 and 10^-4): deterministic normwise
   bounds per frame, u_T = 2^-24 / 2^-53,  delta_f = c u_T log2(N) sqrt(N) ||x_f w||_2  (N = n_fft, c = 4 unless CB says otherwise):
     complex    max_k |dX[k, f]| <= delta_f          power  |dP| <= delta_f (2 |X| + delta_f)       magnitude  ||X^| - |X|| <= delta_f
     dB         |d dB| <= (10 / ln 10) ln(1 + dP / max(P, eps)) + the documented dB evaluation error (f32 2e-5 dB, f64 4e-15 + 3e-16 |dB|)
     band m     |dM_m| <= sum_k w_mk dP_k + L_m u_T sum_k w_mk P_k      (L_m = nonzero weights of band m)
   On the pairing routes ||x_f w|| is the pair's joint norm sqrt(||x_a w||^2 + ||x_b w||^2).  The CPU calibration shows the strict bound
   is neither loose nor vacuous: a per-frame f32 FFT meets it, a paired one (z = a + i b) breaks it and meets the joint one.
4. The inverse routes (one case per `Plan.istft_kernel_name`, asserted): a NaN / Inf bin in a middle and in the last frame of signal 1
   reaches the samples of that frame (and its partner's, on the pairing routes) and nothing else.
"""
import math

import numpy as np
import pytest
import torch

import spectrograms_amd as sg
from oracle import oracle as orc
from spectrograms_amd import _ffi
from tests import helpers as H

HOST = _ffi.DEVICE_HOST_ONLY
SR = 16000.0
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
NP = {"float32": np.float32, "float64": np.float64}
FLOOR = -120.0
WORST = {}

# ---- 1. routes ---------------------------------------------------------------------------------------------------------------------
# (dtype, n_fft, hop, output kind, kernel name); frames per signal: 41 (odd, no multiple of 8 / 16 / 32) unless a case says otherwise
ROUTES = [
    ("float32", 1024, 256, "complex", "r32x16_f32"),          # staged samples
    ("float32", 1024, 256, "power", "r32x16_f32"),
    ("float32", 1024, 256, "magnitude", "r32x16_f32"),
    ("float32", 1024, 256, "db", "r32x16_f32"),
    ("float32", 1024, 256, "db_nofloor", "r32x16_f32"),
    ("float32", 1024, 256, "mel", "r32x16_f32"),              # scheduled band stage
    ("float32", 1024, 256, "mel_db", "r32x16_f32"),
    ("float32", 1024, 256, "erb", "r32x16_f32"),
    ("float32", 1024, 256, "loghz", "r32x16_f32"),
    ("float32", 1024, 256, "chroma", "r32x16_f32"),
    ("float32", 1024, 256, "mfcc40", "r32x16_f32"),           # fused MFCC epilogue, 12 steps for 10 bands' worth
    ("float32", 1024, 256, "mfcc24", "r32x16_f32"),
    ("float32", 1024, 256, "mfcc80", "r32x16_f32"),
    ("float32", 1024, 400, "power", "r32x16_f32"),            # per-lane loads (hop > 272)
    ("float32", 1024, 400, "mfcc40", "r32x16_f32"),           # fused MFCC on the direct path
    ("float32", 1024, 255, "mel_db", "r32x16_f32"),           # odd hop
    ("float32", 1024, 256, "power@5", "r32x16_f32"),          # 5 frames per signal: packed tiles run on into the next signal
    ("float32", 512, 128, "complex", "r32x16_f32"),           # two frames per transform, staged
    ("float32", 512, 128, "power", "r32x16_f32"),
    ("float32", 512, 128, "mel_db", "r32x16_f32"),
    ("float32", 512, 150, "power", "r32x16_f32"),             # no staged variant: the packed form's per-lane loads
    ("float32", 512, 150, "power@5", "r32x16_f32"),
    ("float32", 512, 160, "mfcc40", "r32x16_f32"),            # k_mfcc_acc behind the Mel-dB launch
    ("float64", 512, 160, "complex", "d512_f64"),
    ("float64", 512, 160, "power", "d512_f64"),
    ("float64", 512, 160, "mel_db", "d512_f64"),
    ("float64", 512, 160, "mfcc40", "d512_f64"),
    ("float32", 2048, 512, "complex", "r32x32_f32"),
    ("float32", 2048, 512, "mel", "r32x32_f32"),
    ("float32", 4096, 1024, "power", "r64x32_f32"),
    ("float32", 4096, 1024, "mel", "r64x32_f32"),
    ("float32", 4096, 2048, "mel", "r64x32_f32"),             # per-bin power, then k_bank_rows
    ("float64", 1024, 256, "complex", "d32x16_f64"),
    ("float64", 1024, 256, "mel_db", "d32x16_f64"),
    ("float64", 1024, 256, "mfcc40", "d32x16_f64"),
    ("float64", 2048, 512, "power", "d32x32_f64"),
    ("float64", 2048, 512, "mel", "d32x32_f64"),              # k_bank_rows
    ("float32", 400, 160, "complex", "reg_radix"),
    ("float32", 400, 160, "mel_db", "reg_radix"),
    ("float32", 400, 161, "power", "reg_radix"),              # odd hop
    ("float64", 400, 160, "power", "reg_radix"),
    ("float64", 400, 160, "mel", "reg_radix"),                # f64 composite size: split bank
    ("float32", 16, 4, "power", "lds_radix2"),
    ("float64", 16, 4, "complex", "lds_radix2"),
    ("float32", 15, 4, "power", "two_factor_dft"),
    ("float64", 15, 4, "complex", "two_factor_dft"),
    ("float32", 13, 4, "power", "direct_dft"),
    ("float64", 13, 4, "complex", "direct_dft"),
    ("float32", 401, 160, "complex", "bluestein"),
    ("float32", 401, 160, "mel_db", "bluestein"),             # bank rows inside the kernel (M = 1024)
    ("float64", 401, 160, "power", "bluestein"),
    ("float64", 401, 160, "mel", "bluestein"),                # split path
    ("float32", 65536, 16384, "complex", "big_four_step"),
    ("float64", 32768, 8192, "power", "big_four_step"),
    ("float32", 9001, 2250, "power", "big_chirpz"),
    ("float64", 9001, 2250, "complex", "big_chirpz"),
    ("float32", 9001, 2250, "mel", "big_chirpz"),
]

# Routes that put frames 2p and 2p + 1 of one signal into ONE complex transform (an odd last frame rides alone), read from the code:
#   r32x16 n_fft 512 (kernels_r32x16.hip, HOP512 / PACK slots), k_d512 (kernels_d32x16.hip), k_bs_fused's full-length form
#   (bluestein.hip header: "TWO frames ride one complex transform"), bigfft (plan.hip set_geometry: a.ft = 2).
# (name, dtype, n_fft or None for every length); the partner of frame f is f ^ 1.
PAIRED = [("r32x16_f32", "float32", 512), ("d512_f64", "float64", 512), ("bluestein", "float32", None), ("bluestein", "float64", None),
          ("big_four_step", "float32", None), ("big_four_step", "float64", None), ("big_chirpz", "float32", None), ("big_chirpz", "float64", None)]


def paired(name, dtype, n_fft):
    return any(r == name and d == dtype and (n is None or n == n_fft) for r, d, n in PAIRED)


def _case_id(c):
    return f"{c[0][5:]}-{c[1]}-{c[2]}-{c[3]}"


def split_kind(kind):
    """'power@5' -> ('power', 5 frames per signal); default 41 frames."""
    k, _, nf = kind.partition("@")
    return k, int(nf) if nf else 41


def make_plan(dtype, n_fft, hop, kind, device=_ffi.DEVICE_CURRENT):
    params = sg.SpectrogramParams(sg.StftParams(n_fft, hop, sg.WindowType.hanning, True), SR)
    mel40 = sg.MelParams(40, 0.0, 8000.0)
    k = split_kind(kind)[0]
    if k.startswith("mfcc"):
        return sg.Plan(params, _ffi.AMP_DECIBELS, sg.MelParams(int(k[4:]), 0.0, 8000.0), sg.LogParams(-80.0), dtype, device=device,
                       mfcc=sg.MfccParams(13))
    spec = {"complex": (_ffi.AMP_COMPLEX, None, None), "power": (_ffi.AMP_POWER, None, None), "magnitude": (_ffi.AMP_MAGNITUDE, None, None),
            "db": (_ffi.AMP_DECIBELS, None, sg.LogParams(FLOOR)), "db_nofloor": (_ffi.AMP_DECIBELS, None, None),
            "db_low": (_ffi.AMP_DECIBELS, None, sg.LogParams(-300.0)), "mel": (_ffi.AMP_POWER, mel40, None),
            "mel_db": (_ffi.AMP_DECIBELS, mel40, sg.LogParams(FLOOR)), "erb": (_ffi.AMP_POWER, sg.ErbParams(32, 50.0, 8000.0), None),
            "loghz": (_ffi.AMP_POWER, sg.LogHzParams(48, 50.0, 8000.0), None), "chroma": (_ffi.AMP_MAGNITUDE, sg.ChromaParams(), None)}[k]
    return sg.Plan(params, spec[0], spec[1], spec[2], dtype, device=device)


def oracle_params(n_fft, hop, kind):
    k = split_kind(kind)[0]
    if k.startswith("mfcc"):
        return orc.Params(n_fft=n_fft, hop=hop, n_mels=int(k[4:]), f_min=0.0, f_max=8000.0, amp="db", floor_db=-80.0)
    kw = {"complex": {}, "power": {}, "db_nofloor": {}, "magnitude": {"amp": "magnitude"}, "db": {"amp": "db", "floor_db": FLOOR},
          "mel": {"n_mels": 40}, "mel_db": {"n_mels": 40, "amp": "db", "floor_db": FLOOR},
          "erb": {"n_mels": 32, "erb": True, "f_min": 50.0}, "loghz": {"n_mels": 48, "loghz": True, "f_min": 50.0}, "chroma": {}}[k]
    return orc.Params(n_fft=n_fft, hop=hop, **kw)


def oracle_out(n_fft, hop, kind, x64):
    """Oracle output of (batch, n) f64 samples in the plan's layout."""
    k = split_kind(kind)[0]
    op = oracle_params(n_fft, hop, kind)
    if k == "complex":
        return orc.stft_batch(op, x64)
    if k.startswith("mfcc"):
        return np.stack([orc.mfcc(op, r, 13, True, 22) for r in x64])
    if k == "chroma":
        return np.stack([orc.chromagram(op, r) for r in x64])
    return orc.spectrogram_batch(op, x64)


@pytest.mark.parametrize("case", ROUTES, ids=_case_id)
def test_route_table_selects_the_named_kernel(case):
    dtype, n_fft, hop, kind, name = case
    assert make_plan(dtype, n_fft, hop, kind, device=HOST).kernel_name == name


def test_route_table_reaches_every_stft_kernel_name():
    names = {c[4] for c in ROUTES}
    every = {"r32x16_f32", "r32x32_f32", "d32x16_f64", "d512_f64", "r64x32_f32", "d32x32_f64", "lds_radix2", "two_factor_dft", "reg_radix",
             "bluestein", "big_four_step", "big_chirpz", "direct_dft"}  # sgx_kernel_name (plan.hip) without cqt_mfma_lds / cqt_mfma_global
    assert names == every
    for r, d, n in PAIRED:
        assert r in every


# ---- signals -------------------------------------------------------------------------------------------------------------------
def n_samples(hop, n_fft, nf):
    """A centred signal of nf frames (nf odd: the last frame of a pairing route rides alone)."""
    return max(hop * (nf - 1) + hop // 3, n_fft // 2 + 1)


def frames_in(n_fft, hop, kind):
    nf = split_kind(kind)[1]
    if nf == 41:
        nf = min(41, max(5, 40000 // hop) | 1)
    return nf


def covering(s, n_fft, hop, nf):
    """Frames of a centred signal whose n_fft samples include sample s."""
    sp = s + n_fft // 2
    return [f for f in range(nf) if f * hop <= sp < f * hop + n_fft]


def reach(frames, name, dtype, n_fft, nf):
    out = set(frames)
    if paired(name, dtype, n_fft):
        out |= {f ^ 1 for f in frames if (f ^ 1) < nf}
    return sorted(out)


def bad_positions(n, n_fft, hop, nf):
    """Sample 0, a sample whose covering frames straddle a tile boundary (frame 32, 16 or nf // 2), and the last sample."""
    F = 32 if nf > 34 else 16 if nf > 18 else nf // 2
    mid = F * hop - n_fft // 2 + 1
    if not 0 < mid < n - 1:
        mid = n // 2
    return [0, mid, n - 1]


def locality_batch(dtype, n, seed=0):
    """4 rows: 0 and 3 ordinary, 1 the row that gets a bad sample, 2 that row's shape 10^4 quieter."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = np.stack([0.5 * np.sin(2 * np.pi * 440.0 * t) + 0.05 * rng.standard_normal(n), 0.3 * rng.standard_normal(n),
                  0.3e-4 * rng.standard_normal(n), 0.2 * np.sin(2 * np.pi * 1250.0 * t) + 0.1 * rng.standard_normal(n)])
    return x.astype(NP[dtype])


def nonfinite_cols(a, nb=None):
    """Per (row, ..., frame): non-finite.  Complex: real or imaginary part; bin 0 and Nyquist imaginary parts are not pinned."""
    if np.iscomplexobj(a):
        bad = ~np.isfinite(a.real) | ~np.isfinite(a.imag)
        bad[..., 0, :] = ~np.isfinite(a.real[..., 0, :])
        if nb is not None and nb % 2 == 0:
            bad[..., -1, :] = ~np.isfinite(a.real[..., -1, :])
        return bad
    return ~np.isfinite(a)


# ---- 2. non-finite reach (GPU) ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ROUTES, ids=_case_id)
def test_gpu_non_finite_sample_stays_in_its_frames(case):
    dtype, n_fft, hop, kind, name = case
    k = split_kind(kind)[0]
    nf = frames_in(n_fft, hop, kind)
    n = n_samples(hop, n_fft, nf)
    plan = make_plan(dtype, n_fft, hop, kind)
    assert plan.kernel_name == name
    x = locality_batch(dtype, n)
    pos = bad_positions(n, n_fft, hop, nf)
    x[1, pos] = 0
    base = np.array(plan.compute_batch(x))
    assert base.shape[-1] == nf and np.all(np.isfinite(base))
    assert np.array_equal(np.array(plan.compute_batch(x)), base, equal_nan=True)  # (repeat launches are bit-equal)
    db_kind = k in ("db", "mel_db")
    for s in pos:
        cov = covering(s, n_fft, hop, nf)
        out_of_reach = np.ones(nf, bool)
        out_of_reach[reach(cov, name, dtype, n_fft, nf)] = False
        pinned = out_of_reach.copy()  # frames whose values the oracle pins: all but the partners of covering frames
        pinned[cov] = True
        for v in (np.nan, np.inf, -np.inf):
            xb = x.copy()
            xb[1, s] = v
            got = np.array(plan.compute_batch(xb))
            where = f"{name} {kind} sample {s} = {v}: covering frames {cov}"
            # bit-identical wherever the bad sample is out of reach, in every signal
            for r in (0, 2, 3):
                assert np.array_equal(got[r], base[r]), f"{where}: reaches signal {r}"
            leak = ~np.all(got[1][..., out_of_reach] == base[1][..., out_of_reach], axis=tuple(range(got.ndim - 2)))
            assert not leak.any(), f"{where}: frames {np.flatnonzero(out_of_reach)[leak].tolist()} changed"
            bad = nonfinite_cols(got[1], plan.n_fft // 2 + 1)
            if db_kind:
                assert not np.isnan(got[1]).any(), f"{where}: NaN in a dB output"
            if np.isnan(v):
                ref = oracle_out(n_fft, hop, kind, xb.astype(np.float64)[1:2])[0]
                if k in ("db", "mel_db") or k.startswith("mfcc"):
                    assert np.all(np.isfinite(got[1])), f"{where}: non-finite values (the oracle's are all finite)"
                    assert np.all(np.isfinite(ref))
                    if k.startswith("mfcc"):  # (test_mfcc.py's tolerances)
                        tol = 2e-2 * max(1.0, np.max(np.abs(ref)) / 100) if dtype == "float32" else 1e-7
                    else:  # (test_gpu_parity.py's: every value here is the floor)
                        tol = 1e-3 if dtype == "float32" else 1e-8
                    assert np.max(np.abs(got[1][..., cov] - ref[..., cov])) <= tol, where
                else:
                    assert np.array_equal(bad[..., pinned], nonfinite_cols(ref, plan.n_fft // 2 + 1)[..., pinned]), \
                        f"{where}: non-finite mask differs from the oracle"
            elif k in ("complex", "power", "magnitude", "db_nofloor"):
                assert bad[..., cov].all(), f"{where}: a covering frame has finite bins"
            if not db_kind and not k.startswith("mfcc") and k != "chroma":
                # (chroma: the l2 normalisation leaves a NaN frame's values NaN — oracle mask above; MFCC of +-Inf dB: not pinned)
                assert not bad[..., out_of_reach].any()


# ---- the oracle's non-finite semantics (CPU) -------------------------------------------------------------------------------------
def _np_power(x64, n_fft, hop):
    w = orc.make_window("hanning", n_fft)
    X = np.stack([H.np_stft(r, n_fft, hop, w) for r in x64])
    return X, np.abs(X) ** 2


def _sparse_rows(W, P):
    """sum over the NONZERO weights only, like the reference's CSR rows: a NaN bin outside a band stays out of it."""
    out = np.zeros((P.shape[0], W.shape[0], P.shape[2]))
    for m in range(W.shape[0]):
        nz = np.flatnonzero(W[m])
        out[:, m, :] = np.einsum("k,bkf->bf", W[m, nz], P[:, nz, :])
    return out


@pytest.mark.parametrize("v", [np.nan, np.inf])
@pytest.mark.parametrize("kind", ["power", "magnitude", "db", "mel", "mel_db", "erb", "loghz", "mfcc40"])
def test_oracle_non_finite_semantics_match_numpy(kind, v):
    """NaN / Inf at sample 700 of signal 1: the oracle against np.fft + np.fmax (Rust's f64::max returns the non-NaN operand:
    10 log10(max(NaN, eps)) is the floor, src/spectrogram.rs:2019-2034)."""
    n_fft, hop, n = 512, 160, 4000
    x = locality_batch("float64", n)[:2].copy()
    x[1, 700] = v
    got = oracle_out(n_fft, hop, kind, x)
    X, P = _np_power(x, n_fft, hop)
    k = kind
    if k in ("mel", "mel_db", "erb", "loghz", "mfcc40"):
        plan = make_plan("float64", n_fft, hop, "mel" if k in ("mel_db", "mfcc40") else k, device=HOST)
        ptr, col, val = plan.mel_weights()
        W = np.zeros((ptr.size - 1, n_fft // 2 + 1))
        for m in range(ptr.size - 1):
            W[m, col[ptr[m]:ptr[m + 1]]] = val[ptr[m]:ptr[m + 1]]
        P = _sparse_rows(W, P)
    if k in ("db", "mel_db"):
        ref = 10.0 * np.log10(np.fmax(P, 10.0 ** (FLOOR / 10.0)))
    elif k == "mfcc40":
        D = 10.0 * np.log10(np.fmax(P, 1e-8))
        nm = D.shape[1]
        basis = np.cos(np.pi * np.arange(13)[:, None] * (np.arange(nm)[None, :] + 0.5) / nm)
        lift = 1.0 + 11.0 * np.sin(np.pi * np.arange(13) / 22.0)
        ref = np.einsum("ci,bif->bcf", basis, D) * lift[None, :, None]
    elif k == "magnitude":
        ref = np.sqrt(P)
    else:
        ref = P
    assert got.shape == ref.shape
    cov = covering(700, n_fft, hop, got.shape[2])
    if k in ("db", "mel_db", "mfcc40"):
        assert not np.isnan(got).any()
        if np.isnan(v):
            assert np.all(np.isfinite(got))  # NaN power -> the floor
        else:
            ref[:, :, cov] = got[:, :, cov]  # (+Inf or the floor per bin: depends on the FFT's Inf - Inf; not pinned)
    elif np.isnan(v):
        assert np.array_equal(np.isnan(got), np.isnan(ref))
    # non-finite exactly in the covering frames of signal 1 (every band / bin of them: all weights are read)
    assert np.array_equal(~np.isfinite(got), ~np.isfinite(ref))
    if k not in ("db", "mel_db", "mfcc40"):
        assert (~np.isfinite(got[1][:, cov])).all() and np.isfinite(np.delete(got[1], cov, axis=1)).all() and np.isfinite(got[0]).all()
    fin = np.isfinite(ref)
    assert np.max(np.abs(got[fin] - ref[fin])) <= 1e-9 * max(np.max(np.abs(ref[fin])), 1.0)


def test_oracle_chroma_non_finite_follows_the_reference():
    """src/chroma.rs:406-430: the l2 norm of a NaN frame is NaN, `norm > 0` is false, the frame keeps its NaN values; other frames are
    untouched.  The oracle's chromagram of the clean signal equals it outside the covering frames."""
    n_fft, hop, n = 1024, 256, 8000
    x = locality_batch("float64", n)[1].copy()
    p = oracle_params(n_fft, hop, "chroma")
    x[3000] = 0.0
    clean = orc.chromagram(p, x)
    x[3000] = np.nan
    got = orc.chromagram(p, x)
    cov = covering(3000, n_fft, hop, got.shape[1])
    assert np.isnan(got[:, cov]).all()
    rest = np.setdiff1d(np.arange(got.shape[1]), cov)
    assert np.array_equal(got[:, rest], clean[:, rest])


# ---- 3. per-frame precision under level steps ----------------------------------------------------------------------------------
# c per route family (c = 4 unless listed; no c above 16 without a derivation here)
#   chirp-z: three transforms of the padded length M >= 2N - 1 plus two chirp products; N -> M in delta_f and c = 3 x 4.
CB = {"bluestein": 12.0, "big_chirpz": 12.0}
PREC = sorted({(c[0], c[1], c[2], c[4]) for c in ROUTES if split_kind(c[3])[1] == 41})


def level_batch(dtype, n, n_fft, hop, seed=5):
    """Row 0: noise whose level switches between 1 and 1e-4 in blocks of 2 n_fft + hop / 2 + 7 samples (off the hop grid: whole quiet
    frames next to loud neighbours / partners); rows 1-4 scaled 1, 1e-4, 1e3, 1e-6 (f32) or 1, 1e-7, 1e5, 1e-10 (f64)."""
    rng = np.random.default_rng(seed)
    blk = 2 * n_fft + hop // 2 + 7
    step = np.where((np.arange(n) // blk) % 2 == 0, 1.0, 1e-4)
    scales = [1.0, 1e-4, 1e3, 1e-6] if dtype == "float32" else [1.0, 1e-7, 1e5, 1e-10]
    rows = [step * rng.standard_normal(n)] + [s * rng.standard_normal(n) for s in scales]
    return np.stack(rows).astype(NP[dtype])


def chirp_m(n):
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def frame_deltas(x64, w, n_fft, hop, dtype, c, Neff, joint):
    """delta_f per (row, frame): c u_T log2(Neff) sqrt(Neff) ||x_f w|| (joint: the pair's norm)."""
    fr = np.stack([H.np_frames(r, n_fft, hop, True) for r in x64]) * w[None, None, :]
    nrm2 = np.sum(fr ** 2, axis=-1)  # [b, nf]
    if joint:
        nf = nrm2.shape[1]
        idx = np.arange(nf) ^ 1
        idx[idx >= nf] = np.arange(nf)[idx >= nf]
        nrm2 = nrm2 + np.where(idx != np.arange(nf), nrm2[:, idx], 0.0)
    return c * U[dtype] * math.log2(Neff) * math.sqrt(Neff) * np.sqrt(nrm2)


def ratios(kind, got, X, d, dtype, W=None, eps=None):
    """Observed error / bound, elementwise.  X: f64 reference spectrum [b, bins, nf]; d: delta_f [b, nf]."""
    D = d[:, None, :]
    A = np.abs(X)
    P = A ** 2
    dP = D * (2 * A + D)
    if kind == "complex":
        return np.max(np.abs(got - X), axis=1) / d
    if kind == "power":
        return np.abs(got - P) / dP
    if kind == "magnitude":
        return np.abs(got - A) / D
    if kind == "db_low":
        ref = 10.0 * np.log10(np.maximum(P, eps))
        extra = 2e-5 if dtype == "float32" else 4e-15 + 3e-16 * np.abs(ref)
        return np.abs(got - ref) / ((10.0 / math.log(10.0)) * np.log1p(dP / np.maximum(P, eps)) + extra)
    if kind == "mel":
        L = np.count_nonzero(W, axis=1)[None, :, None]
        ref = np.einsum("mk,bkf->bmf", W, P)
        bound = np.einsum("mk,bkf->bmf", W, dP) + L * U[dtype] * ref
        return np.abs(got - ref) / np.maximum(bound, 1e-300)
    raise AssertionError(kind)


def bound_report(name, r):
    WORST[name] = max(WORST.get(name, 0.0), float(r))
    print(f"{name}: worst ratio to bound {WORST[name]:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("route", PREC, ids=lambda r: f"{r[0][5:]}-{r[1]}-{r[2]}-{r[3]}")
def test_gpu_per_frame_error_under_level_steps(route):
    dtype, n_fft, hop, name = route
    nf = min(41, max(5, 40000 // hop) | 1)
    n = n_samples(hop, n_fft, nf)
    x = level_batch(dtype, n, n_fft, hop)
    x64 = x.astype(np.float64)
    plan = make_plan(dtype, n_fft, hop, "complex")
    w = np.asarray(plan.window(), np.float64)
    X = np.stack([H.np_stft(r, n_fft, hop, w) for r in x64])
    pair = paired(name, dtype, n_fft)
    c = CB.get(name, 4.0)
    Neff = chirp_m(n_fft) if name in ("bluestein", "big_chirpz") else n_fft
    d = frame_deltas(x64, w, n_fft, hop, dtype, c, Neff, pair)
    kinds = ["complex", "power", "magnitude", "db_low"]
    if any(cc[:3] == route[:3] and cc[4] == name and split_kind(cc[3])[0] == "mel" for cc in ROUTES):
        kinds.append("mel")
    for kind in kinds:
        pl = make_plan(dtype, n_fft, hop, kind)
        if pl.kernel_name != name:  # (a filterbank of this shape may run elsewhere; its route is covered by its own case)
            continue
        got = np.array(pl.compute_batch(x)).astype(np.complex128 if kind == "complex" else np.float64)
        W = None
        if kind == "mel":
            ptr, col, val = pl.mel_weights()
            W = np.zeros((ptr.size - 1, n_fft // 2 + 1))
            for m in range(ptr.size - 1):
                W[m, col[ptr[m]:ptr[m + 1]]] = val[ptr[m]:ptr[m + 1]]
        r = ratios(kind, got, X, d, dtype, W, 1e-30)
        worst = float(np.max(r))
        tag = f"{dtype} {n_fft}/{hop} {name} {kind}{' (joint)' if pair else ''}"
        bound_report(tag, worst)
        if pair and kind == "complex":
            strict = float(np.max(ratios(kind, got, X, frame_deltas(x64, w, n_fft, hop, dtype, c, Neff, False), dtype)))
            bound_report(f"{dtype} {n_fft}/{hop} {name} complex (strict, information)", strict)
        assert worst <= 1.0, (tag, worst)


def _paired_rfft32(fr):
    """Two real f32 frames per complex f32 transform, split by Hermitian symmetry (the pairing routes' construction)."""
    nf, N = fr.shape
    out = np.empty((nf, N // 2 + 1), np.complex128)
    for p in range(0, nf, 2):
        b = fr[p + 1] if p + 1 < nf else np.zeros(N)
        z = torch.fft.fft(torch.complex(torch.from_numpy(fr[p].astype(np.float32)), torch.from_numpy(b.astype(np.float32)))).numpy()
        zc = np.conj(np.roll(z[::-1], 1)).astype(np.complex128)
        za = z.astype(np.complex128)
        out[p] = ((za + zc) / 2)[:N // 2 + 1]
        if p + 1 < nf:
            out[p + 1] = (-1j * (za - zc) / 2)[:N // 2 + 1]
    return out


def test_bound_calibration_per_frame_meets_paired_breaks():
    """The strict per-frame bound holds for a per-frame f32 FFT, fails for a paired one (loud partners of quiet frames), and the joint
    bound holds for that paired one: the bound separates the two designs."""
    n_fft, hop = 512, 160
    nf = 41
    n = n_samples(hop, n_fft, nf)
    x = level_batch("float32", n, n_fft, hop)[0]
    x64 = x.astype(np.float64)[None]
    w = orc.make_window("hanning", n_fft)
    fr = H.np_frames(x64[0], n_fft, hop, True) * w[None, :]
    X = np.fft.rfft(fr, axis=-1).T[None]
    per = torch.fft.rfft(torch.from_numpy(fr.astype(np.float32)), dim=-1).numpy().T[None].astype(np.complex128)
    pairx = _paired_rfft32(fr).T[None]
    strict = frame_deltas(x64, w, n_fft, hop, "float32", 4.0, n_fft, False)
    joint = frame_deltas(x64, w, n_fft, hop, "float32", 4.0, n_fft, True)
    r_per = np.max(ratios("complex", per, X, strict, "float32"))
    r_pair_strict = np.max(ratios("complex", pairx, X, strict, "float32"))
    r_pair_joint = np.max(ratios("complex", pairx, X, joint, "float32"))
    print(f"per-frame {r_per:.3g}, paired strict {r_pair_strict:.3g}, paired joint {r_pair_joint:.3g}")
    assert r_per <= 1.0 and r_pair_joint <= 1.0
    assert r_pair_strict > 1.0
    assert r_per > 1e-4  # not vacuous: the observed f32 error is within a few decades of the bound


# ---- 4. inverse routes ---------------------------------------------------------------------------------------------------------
# (dtype, n_fft, hop, inverse, frames pair up, Plan.istft_kernel_name); one case per inverse route name, pairing read from the code:
# k_istft_d512 (two frames per transform), the chirp-z rows (launch_c2r_bluestein's full form: nseq = row pairs) and bigfft
INVERSE = [("float32", 1024, 256, "k_istft1024c", False, "istft1024c"), ("float32", 2048, 512, "k_istft2048", False, "istft2048"),
           ("float64", 1024, 256, "k_istft_d1024", False, "istft_d1024"), ("float64", 512, 160, "k_istft_d512", True, "istft_d512"),
           ("float32", 512, 128, "k_c2r_reg", False, "istft_reg"), ("float32", 400, 160, "k_c2r_reg", False, "istft_reg"),
           ("float64", 32768, 8192, "bigfft", True, "big+ola"),
           ("float32", 251, 62, "k_bs_c2c", True, "c2r_chirpz+ola"), ("float64", 1009, 252, "k_bs_c2c", True, "c2r_chirpz+ola"),
           ("float64", 6000, 1500, "k_bs_c2c_half", False, "c2r_chirpz_half+ola"),
           ("float32", 8200, 2050, "k_bs_c2c_half", False, "c2r_chirpz_half+ola"),
           ("float32", 15, 4, "k_c2r_rows", False, "c2r_rows+ola"), ("float64", 13, 4, "k_c2r_rows", False, "c2r_rows+ola"),
           ("float64", 400, 160, "k_c2r_reg+ola", False, "c2r_reg+ola"), ("float32", 1024, 63, "k_c2r_reg+ola", False, "c2r_reg+ola"),
           ("float32", 9001, 2250, "bigfft", True, "big+ola")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", INVERSE, ids=lambda c: f"{c[3]}-{c[0][5:]}-{c[1]}-{c[2]}")
def test_gpu_inverse_non_finite_bin_stays_in_its_frame(case):
    dtype, n_fft, hop, _, pairs, route = case
    nf = min(41, max(5, 40000 // hop) | 1)
    n = n_samples(hop, n_fft, nf)
    plan = make_plan(dtype, n_fft, hop, "complex")
    S = np.ascontiguousarray(plan.compute_batch(locality_batch(dtype, n)))
    assert S.shape[2] == nf
    fm = nf // 2
    S[1, 5, fm] = 0
    S[1, 5, nf - 1] = 0
    base = plan.istft_batch(S)
    assert plan.istft_kernel_name == route
    L = base.shape[1]
    for f in (fm, nf - 1):
        own = np.zeros(L, bool)
        own[max(0, f * hop - n_fft // 2):max(0, min(L, f * hop + n_fft - n_fft // 2))] = True
        allowed = own.copy()
        if pairs and (f ^ 1) < nf:
            g = f ^ 1
            allowed[max(0, g * hop - n_fft // 2):max(0, min(L, g * hop + n_fft - n_fft // 2))] = True
        for v in (np.nan, np.inf):
            bad = S.copy()
            bad[1, 5, f] = v
            y = plan.istft_batch(bad)
            where = f"frame {f} of {nf}, bin 5 = {v}"
            assert np.array_equal(y[0], base[0]) and np.array_equal(y[2], base[2]), where
            assert np.array_equal(y[1][~allowed], base[1][~allowed]), f"{where}: samples {np.flatnonzero(y[1] != base[1])[:8]} ..."
            # the frame's own samples: every one non-finite (the overlap-add of a non-finite frame, spectrogram.rs:4906-4925)
            assert not np.isfinite(y[1][own]).any(), where
