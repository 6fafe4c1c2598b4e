"""NumPy restatement of the Kaldi fbank / MFCC semantics of include/spectro_hip.h (sgx_kaldi_*), and the per-element bound the GPU
cases of tests/test_kaldi.py hold the kernels to.  No test lives here.

The restatement runs in f64 on the inputs cast to the plan's type T.  For f64 plans it runs in np.longdouble with scipy.fft.rfft, as
tests/test_welch.py's spectra(wide=True) does and for the same reason: np.fft.rfft's own rounding error on an offset signal is of the
size of the bound.  The tables are formed in np.longdouble and rounded once to f64, which is what the library documents for its own.

`kp` is any object with torchaudio.compliance.kaldi's keyword names as attributes (spectrograms_amd.KaldiParams is one).

The bound (c = 4, u_T = 2^-24 / 2^-53; the project's normwise convention, tests/test_welch.py and tests/test_fir.py):
  frame     E_t  = c u_T log2(P) (||v_t||_2 + d ||w||_inf (1 + alpha) ||x_t||_2), v_t the preprocessed windowed frame, d = 1 when DC
            removal or pre-emphasis is on, else 0
  band      dE_b = sum_k B_bk (2 |X_k| E_t + E_t^2) + (nnz_b + 3) u_T E_b; in magnitude form E_t in place of the first bracket
  log       -log1p(-r_b) + 4 u_T max(|log E_b|, 1), r_b = dE_b / E_b (the second term: twice the one ulp HIP documents for logf / log)
  MFCC      lifter_i (sum_b |D_ib| dL_b + (B + 3) u_T sum_b |D_ib| |L_b|)
  energy    the same form on sum f^2, with N in place of nnz_b
  subtract_mean   + the mean of the bounds over the frames + (m + 3) u_T mean |L|
r <= 0.1 at every element is a condition of the bound: `reference` returns the largest r and the caller asserts it before the GPU is touched.
"""
import math

import numpy as np

CBOUND = 4.0
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
NP = {"float32": np.float32, "float64": np.float64}
LD = np.longdouble
PI = LD("3.141592653589793238462643383279502884")
WINDOWS = ("hanning", "hamming", "povey", "rectangular", "blackman")


def sizes(kp):
    """(N, shift, P)."""
    N = int(kp.sample_frequency * kp.frame_length * 0.001)
    shift = int(kp.sample_frequency * kp.frame_shift * 0.001)
    P = 1 << (N - 1).bit_length() if kp.round_to_power_of_two else N
    return N, shift, P


def n_frames(n, N, shift, snip_edges):
    if n < N:
        return 0
    return 1 + (n - N) // shift if snip_edges else (n + shift // 2) // shift


def frame_indices(n, N, shift, snip_edges):
    """(m, N) sample indices of every frame; mirrored at both ends without snip_edges."""
    m = n_frames(n, N, shift, snip_edges)
    t = np.arange(m, dtype=np.int64)[:, None]
    j = np.arange(N, dtype=np.int64)[None, :]
    if snip_edges:
        return t * shift + j
    i = t * shift + shift // 2 - N // 2 + j
    i = np.where(i < 0, -i - 1, i)
    i = np.where(i >= n, 2 * n - 1 - i, i)
    assert i.min() >= 0 and i.max() < n
    return i


def window(kind, N, blackman_coeff=0.42, wide=False):
    a = 2 * PI / LD(N - 1)
    aj = a * np.arange(N).astype(LD)
    if kind == "hanning":
        w = LD(0.5) - LD(0.5) * np.cos(aj)
    elif kind == "hamming":
        w = LD("0.54") - LD("0.46") * np.cos(aj)
    elif kind == "povey":
        w = np.power(LD(0.5) - LD(0.5) * np.cos(aj), LD("0.85"))
    elif kind == "rectangular":
        w = np.ones(N, LD)
    elif kind == "blackman":
        c = LD(blackman_coeff)
        w = c - LD(0.5) * np.cos(aj) + (LD(0.5) - c) * np.cos(2 * aj)
    else:
        raise ValueError(kind)
    return w if wide else w.astype(np.float64)


def mel(f):
    return LD(1127) * np.log(LD(1) + f / LD(700))


def mel_banks(bins, P, fs, low, high):
    """Dense (bins, P // 2 + 1) f64; the last column is zero."""
    if high <= 0:
        high += 0.5 * fs
    mlo, mhi = mel(LD(low)), mel(LD(high))
    delta = (mhi - mlo) / LD(bins + 1)
    melk = mel(LD(fs) / LD(P) * np.arange(P // 2).astype(LD))[None, :]
    b = np.arange(bins).astype(LD)[:, None]
    l, c, r = mlo + b * delta, mlo + (b + 1) * delta, mlo + (b + 2) * delta
    w = np.maximum(LD(0), np.minimum((melk - l) / (c - l), (r - melk) / (r - c)))
    out = np.zeros((bins, P // 2 + 1), np.float64)
    out[:, :P // 2] = w.astype(np.float64)
    return out


def dct(num_ceps, bins):
    i = np.arange(num_ceps).astype(LD)[:, None]
    b = np.arange(bins).astype(LD)[None, :]
    s = np.where(i == 0, np.sqrt(LD(0.5)), LD(1))
    return (s * np.sqrt(LD(2) / LD(bins)) * np.cos(PI / LD(bins) * (b + LD(0.5)) * i)).astype(np.float64)


def lifter(num_ceps, Q):
    if Q == 0:
        return np.ones(num_ceps)
    i = np.arange(num_ceps).astype(LD)
    return (LD(1) + LD(0.5) * LD(Q) * np.sin(PI * i / LD(Q))).astype(np.float64)


def preprocess(fr, kp, w):
    """frames (..., N) -> (f after DC removal, v = window x pre-emphasised f), in the type of fr."""
    f = fr - fr.mean(axis=-1, keepdims=True) if kp.remove_dc_offset else fr
    g = f
    if kp.preemphasis_coefficient != 0:
        prev = np.concatenate([f[..., :1], f[..., :-1]], axis=-1)  # the first sample is its own predecessor
        g = f - fr.dtype.type(kp.preemphasis_coefficient) * prev
    return f, g * w.astype(fr.dtype)


def _rfft(v, P, wide):
    if wide:
        import scipy.fft
        return scipy.fft.rfft(v, n=P, axis=-1)
    return np.fft.rfft(v, n=P, axis=-1)


def reference(x, kp, dtype):
    """(ref, bound, worst r) of a plan's result on rows x (rows, n): ref and bound (rows, m, n_out) f64."""
    T, u, wide = NP[dtype], U[dtype], dtype == "float64"
    Wt = LD if wide else np.float64
    eps = float(np.finfo(T).eps)
    xT = np.atleast_2d(np.asarray(x, T))
    N, shift, P = sizes(kp)
    n = xT.shape[-1]
    idx = frame_indices(n, N, shift, kp.snip_edges)
    m = idx.shape[0]
    fr = xT.astype(Wt)[:, idx]  # (rows, m, N)
    w = window(kp.window_type, N, kp.blackman_coeff)
    f, v = preprocess(fr, kp, w)
    alpha = float(kp.preemphasis_coefficient)
    d = 1.0 if (kp.remove_dc_offset or alpha != 0) else 0.0
    nrm = lambda a: np.linalg.norm(a.astype(np.float64), axis=-1)  # noqa: E731
    Et = CBOUND * u * math.log2(P) * (nrm(v) + d * np.max(np.abs(w)) * (1 + alpha) * nrm(fr))  # (rows, m)
    worst = 0.0

    def log_of(S, dS, count):
        """log(max(S, eps)) and its bound from a sum S of `count` terms known to dS."""
        nonlocal worst
        S64 = S.astype(np.float64)
        dS = dS + (count + 3) * u * S64
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(S64 > 0, dS / S64, np.inf)
        worst = max(worst, float(np.max(r)))
        L = np.log(np.maximum(S, Wt(eps))).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            dL = -np.log1p(-np.minimum(r, 0.999)) + 4 * u * np.maximum(np.abs(L), 1.0)
        return L, dL

    mfcc = int(kp.num_ceps) > 0
    use_power = True if mfcc else bool(kp.use_power)
    use_log = True if mfcc else bool(kp.use_log_fbank)
    X = _rfft(v, P, wide)
    mag = np.abs(X)
    spec = mag * mag if use_power else mag
    bank = mel_banks(int(kp.num_mel_bins), P, kp.sample_frequency, kp.low_freq, kp.high_freq)
    E = spec @ bank.T.astype(Wt)  # (rows, m, bins)
    mag64, e = mag.astype(np.float64), Et[..., None]
    first = (2 * mag64 * e + e * e) if use_power else np.broadcast_to(e, mag64.shape)
    dE = first @ bank.T
    nnz = np.count_nonzero(bank, axis=1)[None, None, :]
    if use_log:
        L, dL = log_of(E, dE, nnz)
    else:
        L, dL = E.astype(np.float64), dE + (nnz + 3) * u * E.astype(np.float64)

    loge = dloge = None
    if kp.use_energy:
        g = f if kp.raw_energy else v
        g64 = np.abs(g.astype(np.float64))
        loge, dloge = log_of(np.sum(g * g, axis=-1), np.sum(2 * g64 * e + e * e, axis=-1), N)
        if kp.energy_floor > 0:
            loge = np.maximum(loge, float(T(math.log(kp.energy_floor))))  # (1-Lipschitz: the bound stands)

    if not mfcc:
        ref, bound = L, dL
        if kp.use_energy:
            parts = ([L, loge[..., None]], [dL, dloge[..., None]]) if kp.htk_compat else ([loge[..., None], L], [dloge[..., None], dL])
            ref, bound = np.concatenate(parts[0], axis=-1), np.concatenate(parts[1], axis=-1)
    else:
        B = int(kp.num_mel_bins)
        D, lif = dct(int(kp.num_ceps), B), lifter(int(kp.num_ceps), kp.cepstral_lifter)
        if wide:
            ref = ((np.log(np.maximum(E, Wt(eps))) @ D.T.astype(Wt)) * lif.astype(Wt)).astype(np.float64)
        else:
            ref = (L @ D.T) * lif
        bound = lif * (dL @ np.abs(D).T + (B + 3) * u * (np.abs(L) @ np.abs(D).T))
        if kp.use_energy:
            ref[..., 0], bound[..., 0] = loge, dloge
        if kp.htk_compat:
            ref, bound = np.roll(ref, -1, axis=-1), np.roll(bound, -1, axis=-1)
    if kp.subtract_mean:
        bound = bound + bound.mean(axis=-2, keepdims=True) + (m + 3) * u * np.abs(ref).mean(axis=-2, keepdims=True)
        ref = ref - ref.mean(axis=-2, keepdims=True)
    return np.ascontiguousarray(ref, np.float64), np.ascontiguousarray(bound, np.float64), worst


def ratio(got, ref, bound):
    """max |got - ref| / bound; every element finite."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.all(np.isfinite(err)), "non-finite result"
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))
