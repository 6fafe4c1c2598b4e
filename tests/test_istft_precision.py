"""Inverse STFT per output sample against an f64 bound, on every route `run_istft` / `launch_c2r_frames` can take.

Route: `Plan.istft_kernel_name` (sgx_istft_kernel_name) names the route of the last successful istft / c2r call; ROUTES pins one
case per name and dtype, on both sides of every threshold of run_istft (hop 63 / 64 at f32 1024, 127 / 128 at 2048, 31 / 32 at f64 512,
63 / 64 at f64 1024, the 2 ov <= tile edge of the fused register-tiled kernel) and at hop = n_fft.

Bound, per untrimmed output sample t, u = 2^-24 / 2^-53 (f32 / f64):
  r_f    the f64 irfft of frame f's spectrum as passed (DC and Nyquist imaginary parts dropped); rho_f = ||r_f||_2, on a route that
         pairs frames 2p / 2p + 1 in one complex transform (PAIRED) the pair's joint norm sqrt(rho_2p^2 + rho_2p+1^2)
  sums over the K_t frames f covering t, j = t - f hop:
         A_t = sum w_j r_f[j],   W_t = sum w_j^2,   y_t = A_t / W_t if W_t > tau else A_t   (tau = T(1e-10), the reference's threshold)
  E_t  = sum |w_j| c u g rho_f + (K_t + 2) u sum |w_j r_f[j]|
  d_t  = E_t / W_t + (K_t + 3) u |y_t|  where the sample is divided,  d_t = E_t  where it is not
  g    = log2 N_eff for the FFT forms (N_eff = the convolution length M on the chirp-z rows and bigfft lengths that are no power of
         two), N for the direct sum, n1 + N / n1 for the two-factor rows.  c = 4 unless CB says otherwise.
  |y_gpu - y_ref| <= d_t on every sample of every signal; where |W_t - tau| <= 2 (K_t + 2) u W_t the threshold decision may go
  either way (f32 routes compare an f32 W_t with 1e-10f) and either branch's value is accepted.
The per-frame part |dr_j| <= ||dr||_2 <= c u g rho is the normwise FFT error bound; the rest is the windowed sum (K_t + 2 roundings
per term), the division and the window square sum (K_t + 3).  The reference is always f64 (NumPy); np.fft.irfft itself is pinned
against a long-double direct sum (u_64 log2 N rho: at most a quarter of the f64 budget).  The CPU calibration shows the bound is
neither vacuous nor blind: an f32 per-frame inverse meets it (worst ratio above 1e-4), an f32 paired one (z = X_a + i X_b) breaks it
on loud / quiet neighbours and meets the joint bound, and one that leaks one f32 rounding of a tile's loudest frame into the tile
breaks it.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import spectrograms_amd as sg
from spectrograms_amd import _ffi

HOST = _ffi.DEVICE_HOST_ONLY
SR = 16000.0
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
NP = {"float32": np.float32, "float64": np.float64}
CNP = {"float32": np.complex64, "float64": np.complex128}
TAU = {"float32": float(np.float32(1e-10)), "float64": 1e-10}
WORST = {}

# ---- routes --------------------------------------------------------------------------------------------------------------------
# (dtype, n_fft, hop, centre, window, sgx_istft_kernel_name, frames 2p / 2p + 1 share one complex transform)
ROUTES = [
    ("float32", 1024, 64, True, "hanning", "istft1024c", False),
    ("float32", 1024, 63, True, "hanning", "c2r_reg+ola", False),        # below the carry's hop: ov = 16
    ("float32", 1024, 1024, False, "hanning", "istft1024c", False),      # hop = n_fft: W_t below tau at the frame edges
    ("float32", 2048, 128, False, "hamming", "istft2048", False),
    ("float32", 2048, 127, True, "hanning", "c2r_reg+ola", False),
    ("float32", 2048, 2048, False, "hanning", "istft2048", False),
    ("float32", 512, 57, True, "hanning", "istft_reg", False),           # 16-frame tiles: ov = 8 = tile / 2
    ("float32", 512, 56, True, "hanning", "c2r_reg+ola", False),         # ov = 9
    ("float32", 400, 45, False, "hamming", "istft_reg", False),
    ("float32", 400, 44, False, "hamming", "c2r_reg+ola", False),
    ("float32", 400, 160, True, "blackman", "istft_reg", False),
    ("float32", 512, 512, False, "hanning", "istft_reg", False),
    ("float32", 4096, 1024, True, "blackman", "c2r_reg+ola", False),     # 2-frame tiles: fused from hop 2048
    ("float32", 4096, 2048, True, "hanning", "istft_reg", False),
    ("float32", 251, 62, True, "hanning", "c2r_chirpz+ola", True),
    ("float32", 1006, 300, True, "blackman", "c2r_chirpz+ola", True),
    ("float32", 8200, 2050, True, "hanning", "c2r_chirpz_half+ola", False),
    ("float32", 8, 3, True, "hanning", "c2r_rows+ola", False),           # radix-2
    ("float32", 15, 4, False, "hamming", "c2r_rows+ola", False),         # two factors
    ("float32", 13, 13, False, "hanning", "c2r_rows+ola", False),        # direct sum
    ("float32", 9001, 2250, True, "hanning", "big+ola", True),
    ("float32", 65536, 16384, True, "blackman", "big+ola", True),
    ("float64", 512, 32, True, "hanning", "istft_d512", True),
    ("float64", 512, 31, True, "hanning", "c2r_reg+ola", False),
    ("float64", 512, 512, False, "hanning", "istft_d512", True),
    ("float64", 512, 160, False, "blackman", "istft_d512", True),
    ("float64", 1024, 64, True, "hanning", "istft_d1024", False),
    ("float64", 1024, 63, False, "hamming", "c2r_reg+ola", False),
    ("float64", 1024, 1024, False, "hanning", "istft_d1024", False),
    ("float64", 400, 160, True, "blackman", "c2r_reg+ola", False),
    ("float64", 2048, 2048, False, "hanning", "c2r_reg+ola", False),
    ("float64", 251, 62, True, "hanning", "c2r_chirpz+ola", True),
    ("float64", 1009, 252, False, "hamming", "c2r_chirpz+ola", True),
    ("float64", 6000, 1500, True, "hanning", "c2r_chirpz_half+ola", False),
    ("float64", 8, 3, True, "hanning", "c2r_rows+ola", False),
    ("float64", 15, 4, True, "blackman", "c2r_rows+ola", False),
    ("float64", 13, 5, False, "hamming", "c2r_rows+ola", False),
    ("float64", 12000, 3000, True, "hanning", "big+ola", True),
    ("float64", 32768, 8192, False, "hamming", "big+ola", True),
]
# single frames (sgx_c2r): (dtype, n_fft, name)
SINGLE = [("float32", 512, "c2r_reg"), ("float32", 1024, "c2r_reg"), ("float64", 400, "c2r_reg"), ("float32", 251, "c2r_chirpz"),
          ("float64", 1009, "c2r_chirpz"), ("float32", 8200, "c2r_chirpz_half"), ("float64", 6000, "c2r_chirpz_half"),
          ("float32", 15, "c2r_rows"), ("float64", 13, "c2r_rows"), ("float64", 8, "c2r_rows"), ("float32", 9001, "big"),
          ("float64", 32768, "big")]
# every name run_istft / launch_c2r_frames can set (the list in plan.hip beside run_istft)
NAMES = {"istft1024c", "istft2048", "istft_d512", "istft_d1024", "istft_reg", "c2r_reg+ola", "c2r_chirpz+ola", "c2r_chirpz_half+ola",
         "c2r_rows+ola", "big+ola", "c2r_reg", "c2r_chirpz", "c2r_chirpz_half", "c2r_rows", "big"}
# c per route (c = 4 unless listed).  Chirp-z: three transforms of length M plus two chirp products, c = 3 x 4 (as the forward CB).
CB = {"c2r_chirpz": 12.0, "c2r_chirpz_half": 12.0, "big_chirpz": 12.0}
# frames per signal: odd and ragged against every tile (16 new frames, 32 frames in 16 slots, tile - ov blocks), and 1 and 2
NF_MAIN = 41


def _rid(c):
    return f"{c[5]}-{c[0][5:]}-{c[1]}-{c[2]}{'c' if c[3] else ''}-{c[4][:4]}"


def chirp_m(n):
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def two_factor_n1(n):
    best = 1
    d = 2
    while d * d <= n:
        if n % d == 0:
            best = d
        d += 1
    return best


def family(name, n):
    base = name.replace("+ola", "")
    if base == "big":
        return "big_chirpz" if n & (n - 1) else "big"
    return base


def g_of(name, n):
    fam = family(name, n)
    if fam == "c2r_rows":
        if n & (n - 1) == 0:
            return math.log2(n)
        n1 = two_factor_n1(n)
        return n1 + n // n1 if n1 > 1 else float(n)
    if fam in ("c2r_chirpz", "big_chirpz"):
        return math.log2(chirp_m(n))
    if fam == "c2r_chirpz_half":
        return math.log2(chirp_m(n // 2))
    return math.log2(n)


def c_of(name, n):
    return CB.get(family(name, n), 4.0)


def make_plan(dtype, n_fft, hop, centre=True, window="hanning", device=_ffi.DEVICE_CURRENT):
    params = sg.SpectrogramParams(sg.StftParams(n_fft, hop, getattr(sg.WindowType, window), centre), SR)
    return sg.Plan(params, _ffi.AMP_COMPLEX, None, None, dtype, device=device)


def plan_window(plan, dtype):
    return np.asarray(plan.window(), np.float64).astype(NP[dtype]).astype(np.float64)


# ---- the f64 reference and its bound ---------------------------------------------------------------------------------------
def frames_f64(S, n_fft):
    """[bins, frames] spectrum as passed -> f64 irfft rows [frames, n_fft], DC / Nyquist imaginary parts dropped."""
    X = np.array(S, np.complex128)
    X[0] = X[0].real
    if n_fft % 2 == 0:
        X[-1] = X[-1].real
    return np.fft.irfft(X, n_fft, axis=0).T


def frame_norms(r, paired, f0=0):
    rho2 = np.sum(r * r, axis=1)
    if paired:
        idx = (np.arange(rho2.size) + f0) ^ 1
        loc = idx - f0
        ok = (loc >= 0) & (loc < rho2.size)
        rho2 = rho2 + np.where(ok, rho2[np.clip(loc, 0, rho2.size - 1)], 0.0)
    return np.sqrt(rho2)


def ola_reference(r, rho, w, hop, dtype, c, g, f0=0, t0=None, t1=None):
    """Reference and bound on untrimmed samples [t0, t1) from frames f0 .. f0 + len(r) - 1 (which must hold every frame covering them).
    Returns y, d, and the other branch (y_alt, d_alt, band) for samples near the threshold."""
    nfr, n = r.shape
    if t0 is None:
        t0, t1 = f0 * hop, (f0 + nfr - 1) * hop + n
    L = t1 - t0
    A, W, K, Ew, Ar = (np.zeros(L) for _ in range(5))
    u = U[dtype]
    for i in range(nfr):
        s = (f0 + i) * hop - t0
        a, b = max(0, s), min(L, s + n)
        if a >= b:
            continue
        wj = w[a - s:b - s]
        rj = r[i, a - s:b - s]
        A[a:b] += wj * rj
        W[a:b] += wj * wj
        K[a:b] += 1
        Ew[a:b] += np.abs(wj) * rho[i]
        Ar[a:b] += np.abs(wj * rj)
    E = c * u * g * Ew + (K + 2) * u * Ar
    tau = TAU[dtype]
    div = W > tau
    Wd = np.where(W > 0, W, 1.0)
    yd, dd = A / Wd, E / Wd + (K + 3) * u * np.abs(A / Wd)
    y = np.where(div, yd, A)
    d = np.where(div, dd, E)
    y_alt = np.where(div, A, yd)
    d_alt = np.where(div, E, dd)
    band = (np.abs(W - tau) <= 2 * (K + 2) * u * W) & (W > 0)
    return y, d, y_alt, d_alt, band


def ratio(got, ref):
    y, d, y_alt, d_alt, band = ref
    got = np.asarray(got, np.float64)

    def one(yy, dd):
        e = np.abs(got - yy)
        return np.where(dd > 0, e / np.where(dd > 0, dd, 1.0), np.where(e == 0, 0.0, np.inf))

    r = one(y, d)
    return np.where(band, np.minimum(r, one(y_alt, d_alt)), r)


def signal_reference(S, n_fft, hop, w, dtype, name, paired, out_len):
    """f64 reference + bound of one signal's istft output (trimmed like the plan's)."""
    r = frames_f64(S, n_fft)
    rho = frame_norms(r, paired)
    ref = ola_reference(r, rho, w, hop, dtype, c_of(name, n_fft), g_of(name, n_fft))
    full = ref[0].size
    start = 0 if out_len == full else n_fft // 2
    return tuple(a[start:start + out_len] for a in ref)


def report(tag, worst):
    WORST[tag] = max(WORST.get(tag, 0.0), float(worst))
    print(f"{tag}: worst ratio to bound {WORST[tag]:.3g}")


# ---- signals ---------------------------------------------------------------------------------------------------------------------
def rand_spec(rng, nb, nf, n_fft, levels):
    """Random spectra [nb, nf] with real DC / Nyquist bins, frame f scaled by levels[f]."""
    X = rng.standard_normal((nb, nf)) + 1j * rng.standard_normal((nb, nf))
    X[0] = X[0].real
    if n_fft % 2 == 0:
        X[-1] = X[-1].real
    return X * np.asarray(levels)[None, :]


def level_batch(plan, dtype, n_fft, hop, centre, nf, seed=11):
    """4 signals of nf frames: 0 the plan's own STFT of a signal stepping between 1 and 1e-4 at a tile's first frame, its last frame and
    mid-tile; 1 random spectra with frame f at 10^(-4 (f mod 3)) (f64 10^(-8 (f mod 3))); 2 signal 1 x 1e-6 (f64 1e-12); 3 a quiet
    signal with one 1e4 frame in the ragged last tile."""
    rng = np.random.default_rng(seed)
    nb = n_fft // 2 + 1
    pad = n_fft // 2 if centre else 0
    n = max((nf - 1) * hop + (hop // 3 if centre else n_fft), 1)
    x = rng.standard_normal(n)
    lvl = np.ones(n)
    quiet = False
    prev = 0
    for f in [1, 15, 16, 24, 31, 32, 33, 40] + list(range(48, nf, 13)):
        s = min(max(f * hop - pad, 0), n)
        if quiet:
            lvl[prev:s] = 1e-4
        quiet, prev = not quiet, s
    if quiet:
        lvl[prev:] = 1e-4
    S0 = np.asarray(plan.compute_batch((x * lvl).astype(NP[dtype])[None]))[0]
    S0 = S0[:, :nf] if S0.shape[1] >= nf else np.pad(S0, ((0, 0), (0, nf - S0.shape[1])))
    e = 4.0 if dtype == "float32" else 8.0
    S1 = rand_spec(rng, nb, nf, n_fft, 10.0 ** (-e * (np.arange(nf) % 3)))
    S2 = S1 * (1e-6 if dtype == "float32" else 1e-12)
    lv3 = np.full(nf, 1e-3)
    lv3[max(nf - 2, 0)] = 1e4
    S3 = rand_spec(rng, nb, nf, n_fft, lv3)
    return np.ascontiguousarray(np.stack([S0, S1, S2, S3]).astype(CNP[dtype]))


def frames_for(dtype, n_fft, hop):
    """Main frame count: NF_MAIN, fewer at the longest lengths (a few seconds of signal)."""
    return NF_MAIN if n_fft <= 8200 else 7


# ---- CPU: names, reference pin, calibration -----------------------------------------------------------------------------------
def test_route_table_names_every_route_the_code_sets():
    src = open(os.path.join(os.path.dirname(__file__), "..", "spectrograms_amd", "csrc", "plan.hip")).read()
    # the inverse path: the table of fused inverses of single shapes (entries {"name", SGX_F32 / SGX_F64, ...}), the rows' launchers, run_istft
    body = src[src.index("const FusedInverse kFusedInverse[] = {"):src.index("sgx_status check_flag(")]
    code = (set(re.findall(r'(?:\*route|\br) = "([^"]+)"', body)) | set(re.findall(r'\{"[^"]+", "([^"]+)"\}', body))
            | set(re.findall(r'\{"([^"]+)", SGX_F(?:32|64),', body)))
    assert "route = r.tuned->route" in body  # (the table's names are reported from there)
    assert code == NAMES, code ^ NAMES
    table = {c[5] for c in ROUTES} | {c[2] for c in SINGLE}
    assert table == NAMES, table ^ NAMES
    for name in NAMES:  # every name in every dtype where it exists
        dts = {c[0] for c in ROUTES if c[5] == name} | {c[0] for c in SINGLE if c[2] == name}
        only = {"istft1024c": {"float32"}, "istft2048": {"float32"}, "istft_reg": {"float32"}, "istft_d512": {"float64"},
                "istft_d1024": {"float64"}}.get(name, {"float32", "float64"})
        assert dts == only, (name, dts)
    for hop_lo, hop_hi, dt, n in ((63, 64, "float32", 1024), (127, 128, "float32", 2048), (31, 32, "float64", 512), (63, 64, "float64", 1024)):
        lo = [c for c in ROUTES if c[:3] == (dt, n, hop_lo)]
        hi = [c for c in ROUTES if c[:3] == (dt, n, hop_hi)]
        assert lo and hi and lo[0][5] != hi[0][5]


def test_istft_kernel_name_is_empty_on_a_host_only_plan():
    pl = make_plan("float32", 1024, 256, device=HOST)
    assert pl.istft_kernel_name == ""
    assert make_plan("float64", 9001, 2250, device=HOST).istft_kernel_name == ""


@pytest.mark.parametrize("n", [8, 13, 15, 64, 251, 400, 1024, 1009])
def test_numpy_irfft_f64_is_pinned_by_a_long_double_direct_sum(n):
    rng = np.random.default_rng(n)
    X = rng.standard_normal(n // 2 + 1) + 1j * rng.standard_normal(n // 2 + 1)
    X[0] = X[0].real
    if n % 2 == 0:
        X[-1] = X[-1].real
    got = np.fft.irfft(X, n)
    ld = np.longdouble
    j = np.arange(n)
    acc = np.full(n, ld(X[0].real))
    for k in range(1, (n + 1) // 2):
        ang = (2 * np.pi * ((k * j) % n)).astype(ld) / ld(n)  # angle reduced in integers
        acc += 2 * (ld(X[k].real) * np.cos(ang) - ld(X[k].imag) * np.sin(ang))
    if n % 2 == 0:
        acc += ld(X[-1].real) * np.where(j % 2 == 0, 1, -1).astype(ld)
    ref = acc / ld(n)
    rho = float(np.sqrt(np.sum(ref * ref)))
    err = float(np.max(np.abs(got.astype(ld) - ref)))
    assert err <= U["float64"] * math.log2(n) * rho, (err, rho)


def _per_frame32(X):
    return torch.fft.irfft(torch.from_numpy(X.astype(np.complex64)), dim=0).numpy().astype(np.float64).T


def _paired32(X, n):
    """Frames 2p / 2p + 1 through one f32 complex inverse transform z = X_a + i X_b (the pairing routes' construction)."""
    Xf = X.astype(np.complex64)
    full = np.concatenate([Xf, np.conj(Xf[1:(n + 1) // 2][::-1])], axis=0)  # Hermitian extension [n, frames]
    nf = X.shape[1]
    out = np.empty((nf, n))
    for p in range(0, nf, 2):
        b = full[:, p + 1] if p + 1 < nf else np.zeros(n, np.complex64)
        z = torch.fft.ifft(torch.from_numpy(full[:, p]) + 1j * torch.from_numpy(b)).numpy()
        out[p] = z.real
        if p + 1 < nf:
            out[p + 1] = z.imag
    return out


def _cpu_istft(fr, w, hop, n, centre, dt=np.float32):
    """Window, overlap-add and division in `dt` from already inverted frames."""
    nf = fr.shape[0]
    full = (nf - 1) * hop + n
    A, W = np.zeros(full, dt), np.zeros(full, dt)
    for f in range(nf):
        A[f * hop:f * hop + n] += (w.astype(dt) * fr[f].astype(dt)).astype(dt)
        W[f * hop:f * hop + n] += (w.astype(dt) * w.astype(dt)).astype(dt)
    y = np.where(W > dt(1e-10), A / np.where(W > 0, W, dt(1)), A)
    return y


def test_bound_calibration_per_frame_meets_paired_and_leaky_break():
    """The strict per-sample bound holds for an f32 per-frame inverse (and is not vacuous), fails for a paired one on loud / quiet
    neighbours while the joint bound holds for it, and fails for one that leaks one f32 rounding of a tile's loudest frame into the
    tile's other frames."""
    n, nf = 512, 41
    rng = np.random.default_rng(7)
    worst = {}
    for hop, window in ((128, "hanning"), (512, "rectangular")):
        w = plan_window(make_plan("float32", n, hop, False, window, device=HOST), "float32")
        X = rand_spec(rng, n // 2 + 1, nf, n, 10.0 ** (-4.0 * (np.arange(nf) % 3))).astype(np.complex64)
        r = frames_f64(X, n)
        strict = ola_reference(r, frame_norms(r, False), w, hop, "float32", 4.0, math.log2(n))
        joint = ola_reference(r, frame_norms(r, True), w, hop, "float32", 4.0, math.log2(n))
        per = _cpu_istft(_per_frame32(X), w, hop, n, False)
        pair = _cpu_istft(_paired32(X, n), w, hop, n, False)
        leak = _per_frame32(X)
        for t0 in range(0, nf, 16):  # tiles of 16 frames: add one f32 rounding of the loudest frame to every frame of the tile
            loud = t0 + int(np.argmax(np.sum(leak[t0:t0 + 16] ** 2, axis=1)))
            leak[t0:t0 + 16] += U["float32"] * leak[loud][None, :]
        leaky = _cpu_istft(leak, w, hop, n, False)
        worst[hop] = (float(np.max(ratio(per, strict))), float(np.max(ratio(pair, strict))), float(np.max(ratio(pair, joint))),
                      float(np.max(ratio(leaky, strict))))
        print(f"hop {hop} {window}: per-frame {worst[hop][0]:.3g}, paired strict {worst[hop][1]:.3g}, paired joint {worst[hop][2]:.3g}, "
              f"leaky {worst[hop][3]:.3g}")
        assert worst[hop][0] <= 1.0 and worst[hop][2] <= 1.0
        assert worst[hop][0] > 1e-4  # not vacuous
    # frames that only their own samples cover (hop = n_fft): the loud partner's / tile's rounding shows in the quiet frames
    assert worst[512][1] > 1.0 and worst[512][3] > 1.0


# ---- GPU: route names and level steps ----------------------------------------------------------------------------------------
def _check_signals(plan, S, got, dtype, n_fft, hop, name, paired, tag):
    w = plan_window(plan, dtype)
    L = got.shape[1]
    worst = 0.0
    for i in range(S.shape[0]):
        ref = signal_reference(S[i], n_fft, hop, w, dtype, name, paired, L)
        r = ratio(got[i], ref)
        k = int(np.argmax(r))
        worst = max(worst, float(r[k]))
        assert r[k] <= 1.0, f"{tag}: signal {i} sample {k} of {L}: |dy| {abs(float(got[i][k]) - ref[0][k]):.3g} bound {ref[1][k]:.3g}"
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROUTES, ids=_rid)
def test_gpu_route_name_and_per_sample_bound_under_level_steps(case):
    dtype, n_fft, hop, centre, window, name, paired = case
    plan = make_plan(dtype, n_fft, hop, centre, window)
    assert plan.istft_kernel_name == ""
    worst = 0.0
    for nf in (frames_for(dtype, n_fft, hop), 1, 2):
        S = level_batch(plan, dtype, n_fft, hop, centre, nf)
        got = plan.istft_batch(S)
        assert plan.istft_kernel_name == name, (nf, plan.istft_kernel_name)
        worst = max(worst, _check_signals(plan, S, got, dtype, n_fft, hop, name, paired, f"{_rid(case)} nf {nf}"))
    report(f"{dtype} {name} {n_fft}/{hop}", worst)


# ---- GPU: basis sweep ----------------------------------------------------------------------------------------------------------
# (dtype, n_fft, route under a rectangular window, hop = n_fft, no centring)
BASIS = [("float32", 1024, "istft1024c"), ("float32", 2048, "istft2048"), ("float32", 512, "istft_reg"), ("float32", 400, "istft_reg"),
         ("float32", 4096, "istft_reg"), ("float32", 251, "c2r_chirpz+ola"), ("float32", 1006, "c2r_chirpz+ola"),
         ("float32", 8200, "c2r_chirpz_half+ola"), ("float32", 15, "c2r_rows+ola"), ("float32", 13, "c2r_rows+ola"),
         ("float32", 8, "c2r_rows+ola"), ("float32", 9001, "big+ola"), ("float32", 65536, "big+ola"),
         ("float64", 512, "istft_d512"), ("float64", 1024, "istft_d1024"), ("float64", 400, "c2r_reg+ola"), ("float64", 2048, "c2r_reg+ola"),
         ("float64", 1009, "c2r_chirpz+ola"), ("float64", 6000, "c2r_chirpz_half+ola"), ("float64", 15, "c2r_rows+ola"),
         ("float64", 13, "c2r_rows+ola"), ("float64", 12000, "big+ola"), ("float64", 32768, "big+ola")]


def basis_bins(n, name):
    nb = n // 2 + 1
    if not name.startswith("big"):
        return np.arange(nb)
    m1 = 1 << (int(math.log2(chirp_m(n) if n & (n - 1) else n)) // 2)
    ks = {0, 1, 2, nb - 2, nb - 1} | {k for k in range(0, nb, m1)} | {k - 1 for k in range(m1, nb, m1)} | set(range(0, nb, 1024))
    ks |= {k - 1 for k in range(1024, nb, 1024)} | set(np.random.default_rng(n).integers(0, nb, 64).tolist())
    return np.array(sorted(k for k in ks if 0 <= k < nb))


@pytest.mark.gpu
@pytest.mark.parametrize("case", BASIS, ids=lambda c: f"{c[2]}-{c[0][5:]}-{c[1]}")
def test_gpu_basis_sweep_every_bin_against_its_cosine(case):
    """Frame f holds a unit-modulus bin k_f (random phase; DC / Nyquist real), every other bin 0: each output frame is that bin's f64
    cosine.  One launch covers every bin (a subset at the bigfft lengths: block edges of the four-step split and of 1024)."""
    dtype, n, name = case
    plan = make_plan(dtype, n, n, False, "rectangular")
    ks = basis_bins(n, name)
    nf, nb = ks.size, n // 2 + 1
    rng = np.random.default_rng(100 + n)
    ph = np.exp(2j * np.pi * rng.random(nf))
    S = np.zeros((nb, nf), np.complex128)
    S[ks, np.arange(nf)] = ph
    S[0] = np.sign(S[0].real)
    if n % 2 == 0:
        S[-1] = np.sign(S[-1].real)
    S = S.astype(CNP[dtype])
    got = plan.istft_batch(S[None])[0].astype(np.float64)
    assert plan.istft_kernel_name == name
    j = np.arange(n)
    Sd = S.astype(np.complex128)
    r = np.empty((nf, n))
    for f, k in enumerate(ks):
        ang = 2 * np.pi * ((int(k) * j) % n) / n
        v = Sd[k, f]
        if k == 0 or 2 * k == n:
            r[f] = v.real * np.cos(ang) / n
        else:
            r[f] = 2 * (v.real * np.cos(ang) - v.imag * np.sin(ang)) / n
    w = plan_window(plan, dtype)
    ref = ola_reference(r, frame_norms(r, any(c[5] == name and c[6] for c in ROUTES)), w, n, dtype, c_of(name, n), g_of(name, n))
    rr = ratio(got, ref)
    k = int(np.argmax(rr))
    report(f"{dtype} {name} {n} basis", rr[k])
    assert rr[k] <= 1.0, f"bin {ks[k // n]} sample {k % n}: {got[k]!r} vs {ref[0][k]!r} (bound {ref[1][k]:.3g})"


# ---- GPU: DC / Nyquist imaginary parts ---------------------------------------------------------------------------------------
DCNY = [c for c in ROUTES if c[1] <= 9001 and c[2] != c[1]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DCNY, ids=_rid)
def test_gpu_dc_nyquist_imaginary_parts_raise_on_the_host_path_and_are_ignored_on_the_device(case):
    dtype, n_fft, hop, centre, window, name, _ = case
    plan = make_plan(dtype, n_fft, hop, centre, window)
    nf = frames_for(dtype, n_fft, hop)
    S = level_batch(plan, dtype, n_fft, hop, centre, nf)
    base = plan.istft_batch(S)
    assert plan.istft_kernel_name == name
    tiny = np.finfo(NP[dtype]).smallest_subnormal
    Sd = torch.from_numpy(S).cuda()
    ref_dev = plan.istft_batch(Sd).cpu().numpy()
    assert np.array_equal(ref_dev, base)
    bins = [0] + ([n_fft // 2] if n_fft % 2 == 0 else [])
    spots = [(0, 0), (0, min(16, nf - 1)), (S.shape[0] - 1, nf - 1)]
    for k in bins:
        for b, f in spots:
            for v in (1e-3, tiny, -tiny):
                bad = S.copy()
                bad[b, k, f] = bad[b, k, f].real + 1j * v
                with pytest.raises(sg.FFTBackendError, match="imaginary part"):
                    plan.istft_batch(bad)
                assert plan.istft_kernel_name == name
                y = plan.istft_batch(torch.from_numpy(bad).cuda()).cpu().numpy()  # ignored in the arithmetic
                assert np.array_equal(y, base), (k, b, f, v)
            neg0 = S.copy()
            neg0[b, k, f] = complex(neg0[b, k, f].real, -0.0)
            assert np.array_equal(plan.istft_batch(neg0), base)
    if n_fft % 2 == 1:  # the last bin of an odd length is ordinary data
        odd = S.copy()
        odd[0, -1, 0] += 1j * 1e-3
        y = plan.istft_batch(odd)
        assert not np.array_equal(y[0], base[0]) and np.array_equal(y[1:], base[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("case", SINGLE, ids=lambda c: f"{c[2]}-{c[0][5:]}-{c[1]}")
def test_gpu_single_frame_c2r_per_frame_bound_and_dc_nyquist(case):
    dtype, n, name = case
    plan = make_plan(dtype, n, n // 4 or 1)
    rng = np.random.default_rng(n)
    c, g, u = c_of(name, n), g_of(name, n), U[dtype]
    worst = 0.0
    for lvl in (1e-6, 1e-3, 1.0, 1e3, 1e6):
        X = (rand_spec(rng, n // 2 + 1, 1, n, [lvl])[:, 0]).astype(CNP[dtype])
        got = plan.c2r(X).astype(np.float64)
        assert plan.istft_kernel_name == name
        r = frames_f64(X[:, None], n)[0]
        rho = float(np.sqrt(np.sum(r * r)))
        worst = max(worst, float(np.max(np.abs(got - r))) / (c * u * g * rho))
        assert worst <= 1.0, (lvl, worst)
    report(f"{dtype} {name} {n} single frame", worst)
    X = (rand_spec(rng, n // 2 + 1, 1, n, [1.0])[:, 0]).astype(CNP[dtype])
    base = plan.c2r(X)
    for k in [0] + ([n // 2] if n % 2 == 0 else []):
        for v in (1e-3, np.finfo(NP[dtype]).smallest_subnormal):
            bad = X.copy()
            bad[k] = bad[k].real + 1j * v
            with pytest.raises(sg.FFTBackendError, match="imaginary part"):
                plan.c2r(bad)
        neg0 = X.copy()
        neg0[k] = complex(neg0[k].real, -0.0)
        assert np.array_equal(plan.c2r(neg0), base)
    if n % 2 == 1:
        odd = X.copy()
        odd[-1] += 1j * 1e-3
        assert not np.array_equal(plan.c2r(odd), base)


# ---- GPU: batch invariance ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ROUTES, ids=_rid)
def test_gpu_each_signal_alone_matches_its_slice_of_the_batch(case):
    dtype, n_fft, hop, centre, window, name, _ = case
    plan = make_plan(dtype, n_fft, hop, centre, window)
    nf = frames_for(dtype, n_fft, hop)
    S = np.concatenate([level_batch(plan, dtype, n_fft, hop, centre, nf, seed=3)[1:], level_batch(plan, dtype, n_fft, hop, centre, nf, seed=4)[:2]])
    Sd = torch.from_numpy(S).cuda()
    y = plan.istft_batch(Sd).cpu().numpy()
    assert plan.istft_kernel_name == name
    assert np.array_equal(plan.istft_batch(Sd).cpu().numpy(), y)
    for i in range(S.shape[0]):
        assert np.array_equal(plan.istft_batch(Sd[i:i + 1].contiguous()).cpu().numpy()[0], y[i]), i


# ---- GPU: the 32-bit frame-count guards of the fused kernels ---------------------------------------------------------------------
# (dtype, n_fft, hop, fused name, bytes per frame in the guard, the route one frame past it)
GUARDS = [("float32", 1024, 256, "istft1024c", 513 * 8, "istft_reg"), ("float32", 2048, 512, "istft2048", 1025 * 8, "c2r_reg+ola"),
          ("float64", 512, 128, "istft_d512", 257 * 16, "c2r_reg+ola"), ("float64", 1024, 256, "istft_d1024", 513 * 16, "c2r_reg+ola")]


def guard_limit(per_frame):
    """Largest n_frames with n_frames * per_frame < 2^31 - 1 (run_istft)."""
    return (0x7fffffff - 1) // per_frame


def test_guard_limits_match_the_code():
    assert [guard_limit(g[4]) for g in GUARDS] == [523265, 261888, 522247, 261632]


def _window_check(plan, Sd, y, b, dtype, n, hop, name, paired, L, full):
    """Output windows at the start, the middle and the last 2 n samples of signal b, against the covering frames only."""
    nf = Sd.shape[2]
    start = 0 if L == full else n // 2
    w = plan_window(plan, dtype)
    worst = 0.0
    for o0 in (0, L // 2, L - 2 * n):
        t0, t1 = o0 + start, o0 + start + 2 * n
        f0, f1 = max(0, (t0 - n) // hop), min(nf, t1 // hop + 1)
        f0, f1 = f0 - f0 % 2, min(nf, f1 + f1 % 2)  # whole pairs for the joint norm
        r = frames_f64(Sd[b, :, f0:f1].cpu().numpy(), n)
        ref = ola_reference(r, frame_norms(r, paired, f0), w, hop, dtype, c_of(name, n), g_of(name, n), f0, t0, t1)
        got = y[b, o0:o0 + 2 * n].cpu().numpy()
        rr = ratio(got, ref)
        worst = max(worst, float(np.max(rr)))
        assert np.max(rr) <= 1.0, (name, b, o0, int(np.argmax(rr)))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1], ids=["at", "past"])
@pytest.mark.parametrize("case", GUARDS, ids=lambda g: g[3])
def test_gpu_fused_kernel_frame_count_guard(case, side):
    dtype, n, hop, fused, per, past = case
    nf = guard_limit(per) + side
    name = past if side else fused
    plan = make_plan(dtype, n, hop, True, "hanning")
    gen = torch.Generator(device="cuda").manual_seed(nf)
    cdt = torch.complex64 if dtype == "float32" else torch.complex128
    S = torch.randn((1, n // 2 + 1, nf), dtype=cdt, device="cuda", generator=gen)
    S[:, 0] = S[:, 0].real.to(cdt)
    S[:, -1] = S[:, -1].real.to(cdt)
    y = plan.istft_batch(S)
    torch.cuda.synchronize()
    assert plan.istft_kernel_name == name
    worst = _window_check(plan, S, y, 0, dtype, n, hop, name, any(c[5] == name and c[6] for c in ROUTES), y.shape[1], (nf - 1) * hop + n)
    report(f"{dtype} {name} {n}/{hop} at {nf} frames", worst)
    del S, y
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_gpu_fused_guard_batch_of_two_puts_the_second_signal_past_2_31_bytes():
    dtype, n, hop, fused, per, _ = GUARDS[0]
    nf = guard_limit(per)
    plan = make_plan(dtype, n, hop, True, "hanning")
    gen = torch.Generator(device="cuda").manual_seed(5)
    S = torch.randn((2, n // 2 + 1, nf), dtype=torch.complex64, device="cuda", generator=gen)
    S[:, 0] = S[:, 0].real.to(torch.complex64)
    S[:, -1] = S[:, -1].real.to(torch.complex64)
    y = plan.istft_batch(S)
    torch.cuda.synchronize()
    assert plan.istft_kernel_name == fused
    for b in (0, 1):
        _window_check(plan, S, y, b, dtype, n, hop, fused, False, y.shape[1], (nf - 1) * hop + n)
    del S, y
    torch.cuda.empty_cache()
