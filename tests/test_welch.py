"""Welch PSD / CSD / coherence plans (spectrograms_amd.welch over sgx_welch_*).

Reference: a NumPy f64 restatement of scipy.signal.welch / csd / coherence (segments, detrend, window, rfft, mean, scale, one-sided
weights) on the inputs cast to the plan's dtype; a CPU test pins the restatement to scipy itself.  For f64 plans the detrend and the
transform of the restatement run in extended precision (`spectra`): in f64 the restatement's own rounding error is as large as the
kernel's.

Bound (the project's normwise convention, tests/test_fir.py): u_T = 2^-24 / 2^-53, c = 4.  Per segment
    E_s = c u_T log2(n) (||v_s||_2 + d ||w||_inf ||x_s||_2),   v_s the detrended windowed segment, d = 0 without detrend, 1 with it
    |dPxx[k]| <= g_k scale (mean_s(2 |X_s[k]| E_s + E_s^2) + (m + 3) u_T mean_s |X_s[k]|^2)
    |dPxy[k]| <= g_k scale (mean_s(|X_s| E^y_s + |Y_s| E^x_s + E^x_s E^y_s) + (m + 3) u_T mean_s |X_s| |Y_s|)
    |dC|      <= 2 ((2 |Pxy| b_xy + b_xy^2) / (Pxx Pyy) + C (b_xx / Pxx + b_yy / Pyy))
the last one only where the reference alone has b_xx / Pxx and b_yy / Pyy <= 0.1 at every bin (asserted).  Every test asserts
ratio = |got - ref| / bound <= 1 and prints the worst ratio.
"""
import ctypes as C
import math

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi

HOST = _ffi.DEVICE_HOST_ONLY
FUSED = (256, 512, 1024, 2048, 4096)
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
NP = {"float32": np.float32, "float64": np.float64}
CBOUND = 4.0


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def one_sided(n):
    g = np.full(n // 2 + 1, 2.0)
    g[0] = 1.0
    if n % 2 == 0:
        g[-1] = 1.0
    return g


def segments(x, n, hop):
    x = np.asarray(x, np.float64)
    m = 1 + (x.shape[-1] - n) // hop
    idx = np.arange(n)[None, :] + hop * np.arange(m)[:, None]
    return x[..., idx]  # (..., m, n)


def detrended(seg, detrend):
    """seg minus nothing / its mean / its least-squares line (the centred form: intercept = the mean, slope = sum jc x / sum jc^2)."""
    if detrend is None:
        return seg
    out = seg - seg.mean(axis=-1, keepdims=True)
    if detrend == "linear":
        n = seg.shape[-1]
        jc = np.arange(n, dtype=seg.dtype) - seg.dtype.type(n - 1) / 2
        out = out - (out @ jc / (jc @ jc))[..., None] * jc
    return out


def spectra(x, w, n, hop, detrend, wide):
    """(segments, detrended windowed segments, their rfft) in f64.  `wide`: the arithmetic runs in extended precision (scipy.fft
    transforms long doubles) and is rounded to f64 at the end.  An f64 plan is checked against that: np.fft.rfft's own rounding error
    on an offset signal is 20 u ||v||_2 at a bin for n = 1024, half of the bound, and it sits on the same bins as the kernel's."""
    seg = segments(x, n, hop)
    if not wide:
        v = detrended(seg, detrend) * w
        return seg, v, np.fft.rfft(v, axis=-1)
    import scipy.fft
    v = detrended(seg.astype(np.longdouble), detrend) * w.astype(np.longdouble)
    return seg, v.astype(np.float64), scipy.fft.rfft(v, axis=-1)  # (complex long doubles: ref_psd / ref_csd round at the end)


def ref_scale(w, fs, scaling):
    wl = np.asarray(w, np.float64).astype(np.longdouble)  # (summed in extended precision, rounded once)
    return float(1 / (np.longdouble(fs) * np.sum(wl * wl)) if scaling == "density" else 1 / np.sum(wl) ** 2)


class Ref:
    """Spectra of the rows of x (..., N) and what the bounds need, all f64."""

    def __init__(self, x, w, n, hop, detrend, u, wide=False):
        self.seg, self.v, self.X = spectra(x, w, n, hop, detrend, wide)  # X: (..., m, nb)
        self.Xw, self.X = self.X, self.X.astype(np.complex128)
        self.m = self.seg.shape[-2]
        d = 0.0 if detrend is None else 1.0
        self.E = CBOUND * u * math.log2(n) * (np.linalg.norm(self.v, axis=-1) + d * np.max(np.abs(w)) * np.linalg.norm(self.seg, axis=-1))
        self.E = self.E[..., None]  # (..., m, 1)
        self.u, self.n = u, n


def ref_psd(r, scale):
    """The means and products in extended precision, rounded once: the restatement's own roundings are not the kernel's."""
    g = one_sided(r.n)
    a = np.abs(r.Xw.astype(np.clongdouble))
    p = (g * scale * np.mean(a * a, axis=-2)).astype(np.float64)
    a = a.astype(np.float64)
    b = g * scale * (np.mean(2 * a * r.E + r.E ** 2, axis=-2) + (r.m + 3) * r.u * np.mean(a * a, axis=-2))
    return p, b


def ref_csd(rx, ry, scale):
    g = one_sided(rx.n)
    ax, ay = np.abs(rx.X), np.abs(ry.X)
    p = (g * scale * np.mean(np.conj(rx.Xw.astype(np.clongdouble)) * ry.Xw.astype(np.clongdouble), axis=-2)).astype(np.complex128)
    b = g * scale * (np.mean(ax * ry.E + ay * rx.E + rx.E * ry.E, axis=-2) + (rx.m + 3) * rx.u * np.mean(ax * ay, axis=-2))
    return p, b


def ref_coherence(rx, ry):
    pxx, bxx = ref_psd(rx, 1.0)
    pyy, byy = ref_psd(ry, 1.0)
    pxy, bxy = ref_csd(rx, ry, 1.0)
    c = np.abs(pxy) ** 2 / (pxx * pyy)
    cond = max(np.max(bxx / pxx), np.max(byy / pyy))
    b = 2.0 * ((2 * np.abs(pxy) * bxy + bxy ** 2) / (pxx * pyy) + c * (bxx / pxx + byy / pyy))
    return c, b, cond


def ratio(got, ref, bound):
    err = np.abs(np.asarray(got, np.complex128 if np.iscomplexobj(ref) else np.float64) - ref)
    assert np.all(np.isfinite(err)), "non-finite result"
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))


def reference(kind, x, y, w, n, hop, detrend, scaling, fs, dtype):
    """(ref, bound) of a plan's result on rows x (, y)."""
    u, wide = U[dtype], dtype == "float64"
    rx = Ref(x, w, n, hop, detrend, u, wide)
    scale = ref_scale(w, fs, scaling)
    if kind == "psd":
        return ref_psd(rx, scale)
    ry = Ref(y, w, n, hop, detrend, u, wide)
    if kind == "csd":
        return ref_csd(rx, ry, scale)
    c, b, cond = ref_coherence(rx, ry)
    assert cond <= 0.1, f"coherence input outside the bound's range: {cond}"
    return c, b


def signals(kind, rows, N, dtype, seed):
    """(x, y) rows (rows, N) of the plan's dtype: 'noise' (a shared component), 'dc' (noise + 1000), 'ramp' (a ramp + noise)."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((rows, N))
    x = s + 0.5 * rng.standard_normal((rows, N))
    y = 0.7 * s + 0.5 * rng.standard_normal((rows, N))
    if kind == "dc":
        x, y = x + 1000.0, y - 1000.0
    elif kind == "ramp":
        t = np.linspace(-1.0, 1.0, N)[None, :] * (1.0 + np.arange(rows))[:, None]
        x, y = x + 40.0 * t + 5.0, y - 25.0 * t
    elif kind == "smallramp":
        t = np.linspace(-1.0, 1.0, N)[None, :]
        x, y = x + 2.0 * t, y - 3.0 * t
    return x.astype(NP[dtype]), y.astype(NP[dtype])


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_listed():
    names = ["sgx_welch_create", "sgx_welch_destroy", "sgx_welch_n_bins", "sgx_welch_n_segments", "sgx_welch_frequencies", "sgx_welch_window",
             "sgx_welch_scale", "sgx_welch_execute", "sgx_welch_reserve", "sgx_welch_allocations", "sgx_welch_tile", "sgx_welch_kernel_name",
             "sgx_welch_device", "sgx_welch_last_error"]
    L = C.CDLL(_ffi.LIB_PATH)
    for s in names:
        assert s in _ffi.SYMBOLS and hasattr(L, s), s
    assert _ffi.lib().sgx_abi_version() == 7


def test_public_names():
    for name in ("WelchParams", "WelchPlan", "welch", "csd", "coherence"):
        assert name in sg.__all__ and hasattr(sg, name)


@pytest.mark.parametrize("detrend", [None, "constant", "linear"])
@pytest.mark.parametrize("scaling", ["density", "spectrum"])
@pytest.mark.parametrize("n,hop,m", [(64, 16, 9), (63, 20, 4), (128, 128, 1), (255, 255, 1), (100, 37, 6)])
def test_restatement_matches_scipy(n, hop, m, scaling, detrend):
    from scipy import signal
    fs = 16000.0
    N = n + (m - 1) * hop + min(hop - 1, 5)
    rng = np.random.default_rng(n + m)
    x = rng.standard_normal(N) + 3.0 + np.linspace(0, 4, N)
    y = 0.5 * x + rng.standard_normal(N)
    w = sg.WelchPlan(sg.WelchParams(n, hop, sg.WindowType.hanning, fs, detrend, scaling), device=HOST).window()
    kw = dict(fs=fs, window=w, nperseg=n, noverlap=n - hop, detrend=detrend if detrend else False, scaling=scaling)
    rx, ry = Ref(x, w, n, hop, detrend, U["float64"]), Ref(y, w, n, hop, detrend, U["float64"])
    assert rx.m == m
    scale = ref_scale(w, fs, scaling)
    f, pxx = signal.welch(x, **kw)
    assert np.allclose(f, np.fft.rfftfreq(n, 1.0 / fs), rtol=1e-15, atol=0)
    mine = ref_psd(rx, scale)[0]
    assert np.max(np.abs(mine - pxx)) <= 1e-12 * np.max(np.abs(pxx))
    _, pxy = signal.csd(x, y, **kw)
    mine = ref_csd(rx, ry, scale)[0]
    assert np.max(np.abs(mine - pxy)) <= 1e-12 * np.max(np.abs(pxy))
    if m > 1:  # (one segment: exactly 1 where defined, 0 / 0 elsewhere)
        kw.pop("scaling")
        _, cxy = signal.coherence(x, y, **kw)
        mine = ref_coherence(rx, ry)[0]
        assert np.max(np.abs(mine - cxy)) <= 1e-12 * np.max(np.abs(cxy))
    # the extended-precision evaluation the f64 plans are checked against is the same quantity
    wx = Ref(x, w, n, hop, detrend, U["float64"], wide=True)
    assert np.max(np.abs(ref_psd(wx, scale)[0] - pxx)) <= 1e-12 * np.max(np.abs(pxx))


@pytest.mark.parametrize("n,hop,window", [(1024, 256, None), (400, 160, "hamming"), (1023, 1, "kaiser"), (256, 256, "custom")])
def test_host_accessors_match_restatement(n, hop, window):
    fs = 44100.0
    wt = {None: sg.WindowType.hanning, "hamming": sg.WindowType.hamming, "kaiser": sg.WindowType.kaiser(6.0),
          "custom": sg.WindowType.custom(np.blackman(n) + 0.01)}[window]
    for scaling in ("density", "spectrum"):
        pl = sg.WelchPlan(sg.WelchParams(n, hop, wt, fs, "constant", scaling), "psd", "float32", device=HOST)
        w = pl.window()
        if window == "custom":
            assert np.array_equal(w, np.blackman(n) + 0.01)
        assert pl.n_bins == n // 2 + 1
        assert np.allclose(pl.frequencies(), np.fft.rfftfreq(n, 1.0 / fs), rtol=1e-14, atol=0)
        assert pl.scale == pytest.approx(ref_scale(w, fs, scaling), rel=5e-16, abs=0)
        for N in (n, n + hop - 1, n + hop, n + 7 * hop + 3, 10 * n + 37):
            assert pl.n_segments(N) == 1 + (N - n) // hop
        assert pl.n_segments(n - 1) == 0
        assert pl.device == HOST and pl.dtype == "float32"


def test_route_table():
    for dtype in ("float32", "float64"):
        for n in FUSED:
            pl = sg.WelchPlan(sg.WelchParams(n, n // 2), "csd", dtype, device=HOST)
            assert pl.kernel_name == "k_welch" and pl.tile >= 1
            # a PSD plan walks the same tiles as the pair kinds (csd(x, x) is welch(x) bit for bit)
            assert sg.WelchPlan(sg.WelchParams(n, n // 2), "psd", dtype, device=HOST).tile == pl.tile
            g = sg.WelchPlan(sg.WelchParams(n, n // 2), "psd", dtype, device=HOST, route="generic")
            assert g.kernel_name == "welch_generic" and g.tile == 0
        for n in (128, 400, 1000, 1023, 8192, 65536, 5003):
            pl = sg.WelchPlan(sg.WelchParams(n, max(1, n // 4)), "coherence", dtype, device=HOST)
            assert pl.kernel_name == "welch_generic" and pl.tile == 0


def _raw_create(n_fft=512, hop=128, centre=0, kind=0, detrend=1, scaling=0, route=0, dtype=_ffi.F64):
    L = _ffi.lib()
    p = _ffi.SgxParams()
    p.n_fft, p.hop_size, p.centre, p.window_kind, p.sample_rate_hz = n_fft, hop, centre, _ffi.WIN_HANNING, 16000.0
    p.dtype, p.device = dtype, HOST
    h = C.c_void_p()
    st = L.sgx_welch_create(C.byref(p), kind, detrend, scaling, route, 0, C.byref(h))
    text = (L.sgx_welch_last_error(None) or b"").decode()
    if h.value:
        L.sgx_welch_destroy(h)
    return st, text


def test_validation_refusals():
    assert _raw_create()[0] == _ffi.SGX_OK
    for kw, word in ((dict(centre=1), "centre"), (dict(hop=0), "hop_size"), (dict(hop=513), "hop_size"), (dict(kind=3), "kind"),
                     (dict(detrend=3), "detrend"), (dict(scaling=2), "scaling"), (dict(route=2), "route"), (dict(n_fft=0), "n_fft")):
        st, text = _raw_create(**kw)
        assert st == _ffi.SGX_INVALID_INPUT and word in text, (kw, text)
    with pytest.raises(sg.InvalidInputError, match="hop_size"):
        sg.WelchParams(512, 0)
    with pytest.raises(sg.InvalidInputError, match="hop_size"):
        sg.WelchParams(512, 513)
    with pytest.raises(sg.InvalidInputError, match="detrend"):
        sg.WelchParams(512, 128, detrend="quadratic")
    with pytest.raises(sg.InvalidInputError, match="scaling"):
        sg.WelchParams(512, 128, scaling="power")
    with pytest.raises(sg.InvalidInputError, match="sample_rate"):
        sg.WelchParams(512, 128, sample_rate=0.0)
    wp = sg.WelchParams(512, 128)
    with pytest.raises(sg.InvalidInputError, match="kind"):
        sg.WelchPlan(wp, "msc", device=HOST)
    with pytest.raises(sg.InvalidInputError, match="route"):
        sg.WelchPlan(wp, "psd", device=HOST, route="fused")
    with pytest.raises(TypeError):
        sg.WelchPlan(sg.StftParams(512, 128, sg.WindowType.hanning, False), device=HOST)
    psd, pair = sg.WelchPlan(wp, "psd", device=HOST), sg.WelchPlan(wp, "csd", device=HOST)
    with pytest.raises(sg.DimensionMismatchError, match="expected 512, got 511") as ei:  # N < n_fft: refused, not shrunk
        psd.compute(np.zeros((2, 511)))
    assert "n_samples" in str(ei.value)
    with pytest.raises(sg.DimensionMismatchError, match="y"):
        pair.compute(np.zeros((2, 600)), np.zeros((2, 601)))
    with pytest.raises(sg.InvalidInputError, match="y must be None"):
        psd.compute(np.zeros(600), np.zeros(600))
    with pytest.raises(sg.InvalidInputError, match="y is required"):
        pair.compute(np.zeros(600))
    # the library's own refusals of the two (the Python layer checks first)
    L = _ffi.lib()
    x = np.zeros(600)
    out = np.zeros(2 * 257)
    assert L.sgx_welch_execute(psd._h, x.ctypes.data, x.ctypes.data, 1, 600, 600, out.ctypes.data, 257, _ffi.MEM_HOST, None) == _ffi.SGX_INVALID_INPUT
    assert b"y must be NULL" in L.sgx_welch_last_error(psd._h)
    assert L.sgx_welch_execute(pair._h, x.ctypes.data, None, 1, 600, 600, out.ctypes.data, 514, _ffi.MEM_HOST, None) == _ffi.SGX_INVALID_INPUT
    assert b"y is required" in L.sgx_welch_last_error(pair._h)
    assert L.sgx_welch_execute(pair._h, x.ctypes.data, x.ctypes.data, 1, 600, 600, out.ctypes.data, 257, _ffi.MEM_HOST, None) == _ffi.SGX_DIM_MISMATCH
    with pytest.raises(sg.FFTBackendError, match="no HIP device"):  # shapes are checked first, then the device
        psd.compute(np.zeros(600))
    with pytest.raises(sg.FFTBackendError, match="no HIP device"):
        psd.reserve(2, 600)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _dev_rows(a, pad=13):
    """rows of `a` on the device with sample_stride = N + pad"""
    import torch
    big = torch.zeros((a.shape[0], a.shape[1] + pad), dtype=torch.from_numpy(a[:1, :1]).dtype, device="cuda")
    big[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return big[:, :a.shape[1]]


def _run(plan, x, y=None):
    import torch
    out = plan.compute_torch(_dev_rows(x), None if y is None else _dev_rows(y))
    torch.cuda.synchronize()
    return out.cpu().numpy()


FULL = [(k, d, s) for k in ("psd", "csd", "coherence") for d in (None, "constant", "linear") for s in ("density", "spectrum")]
SHORT = [("psd", "constant", "density"), ("csd", None, "spectrum")]
SIGNALS = {None: ("noise", "dc"), "constant": ("noise", "dc"), "linear": ("ramp", "noise")}
COH_SIGNALS = {None: ("noise",), "constant": ("noise",), "linear": ("smallramp",)}  # (inside the coherence bound's range)


def _parity_cases():
    for dtype in ("float32", "float64"):
        for n in FUSED:
            for hop in ((n, n // 2, n // 4, 97, 1) if n == 256 else (n // 2, n // 4)):
                yield pytest.param(n, hop, dtype, id=f"{n}-{hop}-{dtype}")


@pytest.mark.gpu
@pytest.mark.parametrize("n,hop,dtype", list(_parity_cases()))
def test_fused_parity(n, hop, dtype):
    fs = 16000.0
    combos = FULL if n in (256, 1024) else SHORT
    plans = {c: sg.WelchPlan(sg.WelchParams(n, hop, sg.WindowType.hanning, fs, c[1], c[2]), c[0], dtype) for c in combos}
    first = next(iter(plans.values()))
    assert first.kernel_name == "k_welch"
    t, w = first.tile, first.window()
    worst = {}
    for m in sorted({1, t - 1, t, t + 1, 2 * t + 1} - {0}):
        N = n + (m - 1) * hop + (37 if hop > 37 else hop - 1)
        data = {s: signals(s, 3, N, dtype, seed=1000 * m + i) for i, s in enumerate(("noise", "dc", "ramp", "smallramp"))}
        for (kind, detrend, scaling), plan in plans.items():
            assert plan.tile == t and plan.n_segments(N) == m
            for sname in (COH_SIGNALS if kind == "coherence" else SIGNALS)[detrend]:
                x, y = data[sname]
                got = _run(plan, x, None if kind == "psd" else y)
                ref, bound = reference(kind, x, y, w, n, hop, detrend, scaling, fs, dtype)
                assert got.shape == ref.shape
                r = ratio(got, ref, bound)
                worst[kind] = max(worst.get(kind, 0.0), r)
                assert r <= 1.0, (kind, detrend, scaling, sname, m, r)
    print(f"welch parity n={n} hop={hop} {dtype} tile={t}: worst ratio {worst}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n", [256, 1024])
def test_level_difference_pair(n, dtype):
    """Channels 10^5 apart: each channel's PSD meets its own bound (the channels are separate transforms), the CSD its bound."""
    hop, m = n // 2, 9
    N = n + (m - 1) * hop + 37
    x, y = signals("noise", 3, N, dtype, seed=5)
    x = (x.astype(np.float64) * 1e5).astype(NP[dtype])
    wp = sg.WelchParams(n, hop, sg.WindowType.hanning, 16000.0)
    psd, cs = sg.WelchPlan(wp, "psd", dtype), sg.WelchPlan(wp, "csd", dtype)
    w = psd.window()
    out = {}
    for name, got, (ref, bound) in (("Pxx", _run(psd, x), reference("psd", x, None, w, n, hop, "constant", "density", 16000.0, dtype)),
                                    ("Pyy", _run(psd, y), reference("psd", y, None, w, n, hop, "constant", "density", 16000.0, dtype)),
                                    ("Pxy", _run(cs, x, y), reference("csd", x, y, w, n, hop, "constant", "density", 16000.0, dtype))):
        out[name] = ratio(got, ref, bound)
    print(f"welch level pair n={n} {dtype}: {out}")
    assert max(out.values()) <= 1.0, out


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n", [256, 2048])
def test_identities(n, dtype):
    hop = n // 4
    wp = sg.WelchParams(n, hop, sg.WindowType.hanning, 8000.0)
    psd, cs, co = (sg.WelchPlan(wp, k, dtype) for k in ("psd", "csd", "coherence"))
    m = 2 * psd.tile + 1
    N = n + (m - 1) * hop + 37
    x, y = signals("noise", 3, N, dtype, seed=11)
    pxx, pxy, pyx, cxx, sxx = _run(psd, x), _run(cs, x, y), _run(cs, y, x), _run(co, x, x), _run(cs, x, x)
    assert np.all(pxx > 0)
    assert np.max(np.abs(cxx - 1.0)) <= 8 * U[dtype]
    assert np.all(sxx.imag == 0) and np.array_equal(sxx.real, pxx)
    assert np.array_equal(pyx, np.conj(pxy))
    # one segment: |conj(X) Y|^2 = |X|^2 |Y|^2, coherence 1 within its bound
    x1, y1 = x[:, :n + 5], y[:, :n + 5]
    c1 = _run(co, x1, y1)
    ref, bound = reference("coherence", x1, y1, psd.window(), n, hop, "constant", "density", 8000.0, dtype)
    assert np.max(np.abs(ref - 1.0)) < 1e-12
    r = ratio(c1, ref, bound)
    print(f"welch identities n={n} {dtype}: one-segment coherence ratio {r}")
    assert r <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("n,route", [(512, "auto"), (400, "generic")])
def test_rows_do_not_depend_on_the_batch(n, route):
    import torch
    hop = n // 4
    plan = sg.WelchPlan(sg.WelchParams(n, hop), "coherence", "float32", route=route)
    m = 2 * max(plan.tile, 4) + 3
    N = n + (m - 1) * hop + 11
    x, y = signals("noise", 7, N, "float32", seed=3)
    full = _run(plan, x, y)
    assert np.array_equal(full, _run(plan, x, y))  # a second launch
    for r in (0, 3, 6):
        assert np.array_equal(_run(plan, x[r:r + 1], y[r:r + 1])[0], full[r]), r
    # a NaN in one sample of row 1 (inside a segment) takes row 1's bins, and nothing else
    psd = sg.WelchPlan(sg.WelchParams(n, hop, detrend=None), "psd", "float32", route=route)
    clean = _run(psd, x[:3])
    bad = x[:3].copy()
    bad[1, n + 3] = np.nan
    got = _run(psd, bad)
    assert np.all(np.isnan(got[1])) and np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
    torch.cuda.synchronize()


GENERIC = [(400, 200), (1000, 250), (1023, 511), (8192, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n,hop", GENERIC)
def test_generic_route(n, hop, dtype):
    fs, m = 16000.0, 5
    N = n + (m - 1) * hop + 37
    worst = {}
    for kind, detrend, scaling, sname in (("psd", "constant", "density", "dc"), ("csd", None, "spectrum", "noise"),
                                          ("coherence", "linear", "density", "smallramp")):
        plan = sg.WelchPlan(sg.WelchParams(n, hop, sg.WindowType.hanning, fs, detrend, scaling), kind, dtype)
        assert plan.kernel_name == "welch_generic" and plan.tile == 0
        x, y = signals(sname, 3, N, dtype, seed=n)
        got = _run(plan, x, None if kind == "psd" else y)
        ref, bound = reference(kind, x, y, plan.window(), n, hop, detrend, scaling, fs, dtype)
        worst[kind] = ratio(got, ref, bound)
    print(f"welch generic n={n} {dtype}: worst ratio {worst}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_generic_route_against_fused(dtype):
    n, hop, m, fs = 1024, 256, 11, 16000.0
    N = n + (m - 1) * hop + 37
    x, y = signals("dc", 3, N, dtype, seed=8)
    for kind in ("psd", "csd"):
        wp = sg.WelchParams(n, hop, sg.WindowType.hanning, fs)
        fused, gen = sg.WelchPlan(wp, kind, dtype), sg.WelchPlan(wp, kind, dtype, route="generic")
        assert (fused.kernel_name, gen.kernel_name) == ("k_welch", "welch_generic")
        yy = None if kind == "psd" else y
        a, b = _run(fused, x, yy), _run(gen, x, yy)
        ref, bound = reference(kind, x, y, fused.window(), n, hop, "constant", "density", fs, dtype)
        assert ratio(b, ref, bound) <= 1.0
        assert np.all(np.abs(a - b) <= 2 * bound)


@pytest.mark.gpu
def test_generic_chunk_seam_inside_a_row():
    n, hop, m, dtype = 400, 200, 5, "float64"
    N = n + (m - 1) * hop + 37
    x, _ = signals("dc", 3, N, dtype, seed=21)
    wp = sg.WelchParams(n, hop, sg.WindowType.hanning, 16000.0)
    per = max(n, 2 * (n // 2 + 1)) * 8
    small = sg.WelchPlan(wp, "psd", dtype, max_scratch_bytes=4 * per)  # chunks of 4 segments: 0-3 | 4-7 | 8-11 | ...; row 1 is 5-9
    whole = sg.WelchPlan(wp, "psd", dtype)
    got = _run(small, x)
    ref, bound = reference("psd", x, None, small.window(), n, hop, "constant", "density", 16000.0, dtype)
    r = ratio(got, ref, bound)
    print(f"welch chunk seam: ratio {r}")
    assert r <= 1.0
    assert np.array_equal(got, _run(whole, x))  # segments are added in order: the seams do not change the bits


@pytest.mark.gpu
@pytest.mark.parametrize("n,kind", [(1024, "coherence"), (400, "psd")])
def test_stream_and_memory(n, kind):
    import torch
    hop = n // 4
    plan = sg.WelchPlan(sg.WelchParams(n, hop), kind, "float32")
    N = n + 40 * hop + 5
    x, y = signals("noise", 4, N, "float32", seed=2)
    xd, yd = torch.from_numpy(x).cuda(), (None if kind == "psd" else torch.from_numpy(y).cuda())
    plan.reserve(4, N, host_staging=False)
    before = plan.allocations
    out = torch.empty((4, plan.n_bins), dtype=torch.float32, device="cuda")
    for _ in range(10):
        plan.compute_torch(xd, yd, out=out)
    torch.cuda.synchronize()
    assert plan.allocations == before
    base = out.cpu().numpy().copy()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        o2 = plan.compute_torch(xd, yd)
    side.synchronize()
    assert np.array_equal(o2.cpu().numpy(), base)
    assert np.array_equal(plan.compute(x, None if kind == "psd" else y), base)  # the host-pointer path: the same bits


@pytest.mark.gpu
def test_one_shot_functions():
    n, hop = 512, 128
    wp = sg.WelchParams(n, hop, sample_rate=8000.0)
    x, y = signals("noise", 2, 4000, "float64", seed=4)
    f, pxx = sg.welch(x, wp)
    assert f.shape == (257,) and pxx.shape == (2, 257) and pxx.dtype == np.float64
    w = sg.WelchPlan(wp, device=HOST).window()
    ref, bound = reference("psd", x, None, w, n, hop, "constant", "density", 8000.0, "float64")
    assert ratio(pxx, ref, bound) <= 1.0
    f, pxy = sg.csd(x[0], y[0], wp, dtype="float32")
    assert pxy.shape == (257,) and pxy.dtype == np.complex64
    f, c = sg.coherence(x[0], y[0], wp)
    assert c.shape == (257,) and np.all((c >= 0) & (c <= 1 + 1e-12))
