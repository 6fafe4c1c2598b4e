"""MDCT / IMDCT plans (spectrograms_amd.mdct, sgx_mdct_*) against an independent NumPy restatement of src/mdct.rs.

The restatement is the definition, not the engine's algorithm: for 2N <= 4096 the direct cosine-matrix sums (f64 for f32 plans,
np.longdouble for f64 plans, arguments reduced exactly in integers); above that an f64 np.fft evaluation of the modulated 2N-point DFT,
which a CPU test pins against the direct sums.  Deterministic normwise bounds, u_T = 2^-24 / 2^-53, c = 4:
  forward, per frame   max_k |dC[k,f]| <= c u_T log2(2N) sqrt(N) ||x_f w||_2
  inverse              max_n |dy[n]|   <= c u_T log2(2N) ceil(2N / hop) max|w| max_f 2 ||C_f||_2 / sqrt(N)
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi

HOST = _ffi.DEVICE_HOST_ONLY
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
NP = {"float32": np.float32, "float64": np.float64}
CB = 4.0
WORST = {}


# ---- restatement ---------------------------------------------------------------------------------------------------------------
_PI_LD = np.longdouble("3.14159265358979323846264338327950288")


@functools.lru_cache(maxsize=2)  # (the long-double matrix of N = 2048 takes seconds; callers only read it)
def _cosm(N, dt):
    n = np.arange(2 * N, dtype=np.int64)
    k = np.arange(N, dtype=np.int64)
    r = np.outer(2 * k + 1, 2 * n + 1 + N) % (8 * N)
    pi = _PI_LD if dt is np.longdouble else np.float64(np.pi)
    m = np.cos(r.astype(dt) * pi / dt(4 * N))
    m.setflags(write=False)
    return m


def frames_of(x, two_n, hop):
    nf = (x.shape[-1] - two_n) // hop + 1
    idx = np.arange(nf)[:, None] * hop + np.arange(two_n)[None, :]
    return x[..., idx]  # [..., nf, 2N]


def ref_forward(x, w, two_n, hop, dtype):
    """(batch, n) T-cast samples -> (batch, N, nf) in f64 (the direct sums in f64 / long double, or the f64 FFT form above 4096)."""
    N = two_n // 2
    z = frames_of(np.asarray(x, np.float64), two_n, hop) * np.asarray(w, np.float64)  # [b, nf, 2N]
    if two_n <= 4096:
        dt = np.longdouble if dtype == "float64" else np.float64
        out = np.einsum("kn,bfn->bkf", _cosm(N, dt), z.astype(dt))
        return out.astype(np.float64)
    return fft_forward(z, N)


def fft_forward(z, N):
    n = np.arange(2 * N)
    k = np.arange(N)
    G = np.fft.fft(z * np.exp(-1j * np.pi * n / (2 * N)), axis=-1)[..., :N]
    # (the modulation's integer product reduced mod 8N first: its angle reaches N pi / 2, where f64 keeps ~1e-12 absolute)
    X = (np.exp(-1j * np.pi * (((1 + N) * (2 * k + 1)) % (8 * N)) / (4 * N)) * G).real  # [b, nf, N]
    return np.swapaxes(X, -1, -2)


def ref_frames_inv(c, N, dtype):
    """(batch, N, nf) -> frames y_f[m] (batch, nf, 2N) in f64."""
    c = np.asarray(c, np.float64)
    if 2 * N <= 4096:
        dt = np.longdouble if dtype == "float64" else np.float64
        y = np.einsum("kn,bkf->bfn", _cosm(N, dt), c.astype(dt)) * dt(2.0) / dt(N)
        return y.astype(np.float64)
    return fft_frames_inv(c, N)


def fft_frames_inv(c, N):
    k = np.arange(N)
    m = np.arange(2 * N)
    h = np.swapaxes(c, -1, -2) * np.exp(-1j * np.pi * ((k * (1 + N)) % (4 * N)) / (2 * N))  # [b, nf, N]
    H = np.fft.fft(h, n=2 * N, axis=-1)
    return (2.0 / N) * (np.exp(-1j * np.pi * ((2 * m + 1 + N) % (8 * N)) / (4 * N)) * H).real


def ola(frames, w, hop):
    b, nf, two_n = frames.shape
    out = np.zeros((b, hop * nf + two_n - hop))
    for f in range(nf):
        out[:, f * hop:f * hop + two_n] += frames[:, f] * w
    return out


def fwd_bound(x, w, two_n, hop, dtype):
    N = two_n // 2
    z = frames_of(np.asarray(x, np.float64), two_n, hop) * w
    return CB * U[dtype] * math.log2(two_n) * math.sqrt(N) * np.linalg.norm(z, axis=-1)  # [b, nf]


def inv_bound(c, w, two_n, hop, dtype):
    N = two_n // 2
    cn = np.linalg.norm(np.asarray(c, np.float64), axis=-2)  # [b, nf]
    return CB * U[dtype] * math.log2(two_n) * math.ceil(two_n / hop) * np.max(np.abs(w)) * 2.0 * cn.max() / math.sqrt(N)


def _record(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    print(f"{name}: worst ratio to bound {WORST[name]:.3g}")


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_params_validation_texts():
    with pytest.raises(ValueError, match="^window_size must be > 0$"):
        sg.MdctParams(0, 4, sg.WindowType.hanning)
    with pytest.raises(ValueError, match="^hop_size must be > 0$"):
        sg.MdctParams(8, 0, sg.WindowType.hanning)
    with pytest.raises(ValueError, match="^window_size must be > 0$"):
        sg.MdctParams.sine_window(0)
    with pytest.raises(sg.InvalidInputError, match=r"^Invalid input: window_size must be even, got 7$"):
        sg.MdctParams(7, 2, sg.WindowType.hanning)
    with pytest.raises(sg.InvalidInputError, match=r"^Invalid input: window_size must be >= 4, got 2$"):
        sg.MdctParams(2, 1, sg.WindowType.hanning)
    with pytest.raises(sg.InvalidInputError, match=r"^Invalid input: window_size must be even, got 9$"):
        sg.MdctParams.sine_window(9)
    # a custom window of another length: refused (the reference panics in make_window)
    p = sg.MdctParams(16, 8, sg.WindowType.custom(np.ones(12)))
    with pytest.raises(sg.InvalidInputError, match=r"Custom window size \(12\) must match window_size \(16\)"):
        sg.MdctPlan(p, device=HOST)
    with pytest.raises(sg.FFTBackendError, match="8194"):
        sg.MdctPlan(sg.MdctParams(8194, 4097, sg.WindowType.hanning), device=HOST)
    sg.MdctPlan(sg.MdctParams(16384, 100, sg.WindowType.hanning), device=HOST)


def test_c_abi_validation():
    L = _ffi.lib()
    h = C.c_void_p()
    assert L.sgx_mdct_create(10, 0, _ffi.WIN_HANNING, 0.0, None, 0, _ffi.F32, HOST, C.byref(h)) == _ffi.SGX_INVALID_INPUT
    assert b"hop_size must be > 0" in L.sgx_mdct_last_error(None)
    assert L.sgx_mdct_create(10, 5, _ffi.WIN_HANNING, 0.0, None, 0, _ffi.F32, HOST, C.byref(h)) == _ffi.SGX_OK
    nc, nf = C.c_size_t(), C.c_size_t()
    assert L.sgx_mdct_output_shape(h, 9, C.byref(nc), C.byref(nf)) == _ffi.SGX_INVALID_INPUT
    assert L.sgx_mdct_last_error(h) == b"Invalid input: samples length (9) must be >= window_size (10)"
    out = np.zeros(100, np.float32)
    st = L.sgx_mdct_inverse(h, out.ctypes.data, 1, 4, 3, out.ctypes.data, 100, _ffi.MEM_HOST, None)
    assert st == _ffi.SGX_DIM_MISMATCH and b"coefficients has 4 rows but params.n_coefficients() = 5" in L.sgx_mdct_last_error(h)
    st = L.sgx_mdct_forward(h, out.ctypes.data, 1, 20, out.ctypes.data, 99, _ffi.MEM_HOST, None)  # 5 x 3 expected
    assert st == _ffi.SGX_DIM_MISMATCH and L.sgx_mdct_last_error(h) == b"Dimension mismatch: expected 15, got 99"
    st = L.sgx_mdct_forward(h, out.ctypes.data, 1, 20, out.ctypes.data, 15, _ffi.MEM_HOST, None)
    assert st == _ffi.SGX_BACKEND  # host-only plan
    L.sgx_mdct_destroy(h)


def test_sine_window_values_and_hop():
    for ws in (4, 16, 2048):
        p = sg.MdctParams.sine_window(ws)
        assert p.hop_size == ws // 2 and p.window_size == ws and p.n_coefficients == ws // 2
        w = sg.MdctPlan(p, device=HOST).window()
        np.testing.assert_allclose(w, np.sin(np.pi * (np.arange(ws) + 0.5) / ws), rtol=0, atol=1e-15)
    assert repr(sg.MdctParams.sine_window(16)) == "MdctParams(window_size=16, hop_size=8, n_coefficients=8)"


def test_shapes_and_lengths():
    plan = sg.MdctPlan(sg.MdctParams(16, 6, sg.WindowType.hanning), device=HOST)
    assert plan.output_shape(16) == (8, 1)
    assert plan.output_shape(16 + 6 - 1) == (8, 1)
    assert plan.output_shape(16 + 6) == (8, 2)
    assert plan.inverse_length(0) == 0
    assert plan.inverse_length(3) == 6 * 3 + 16 - 6
    with pytest.raises(sg.InvalidInputError, match=r"samples length \(15\) must be >= window_size \(16\)"):
        plan.output_shape(15)
    with pytest.raises(sg.InvalidInputError, match=r"coefficients has 7 rows but params.n_coefficients\(\) = 8"):
        plan.inverse(np.zeros((7, 3)))
    assert plan.inverse(np.zeros((8, 0))).shape == (0,)
    assert plan.inverse(np.zeros((8, 0)), original_length=100).shape == (0,)


@pytest.mark.parametrize("win", [sg.WindowType.hanning, sg.WindowType.kaiser(5.0), sg.WindowType.blackman,
                                 sg.WindowType.gaussian(3.0)])
def test_window_matches_window_type(win):
    for ws in (6, 64, 1000):
        w = sg.MdctPlan(sg.MdctParams(ws, ws // 2, win), device=HOST).window()
        ref = sg.Plan(sg.SpectrogramParams(sg.StftParams(ws, ws, win, False), 1.0), _ffi.AMP_POWER, None, None, "float64",
                      device=HOST).window()
        np.testing.assert_array_equal(w, ref)


def test_restatement_reproduces_reference_direct_formula_case():
    # python/tests/test_mdct.py "compare with direct formula": 2N = 16, rectangular window, one frame
    N = 8
    np.random.seed(7)
    x = np.random.randn(2 * N)
    ref = np.array([sum(x[n] * np.cos(np.pi * (2 * n + 1 + N) * (2 * k + 1) / (4 * N)) for n in range(2 * N)) for k in range(N)])
    got = ref_forward(x[None], np.ones(2 * N), 2 * N, N, "float64")[0, :, 0]
    np.testing.assert_allclose(got, ref, atol=1e-13)


@pytest.mark.parametrize("N", [8, 9, 512, 2048])
def test_fft_restatement_pinned_to_direct_sums(N):
    rng = np.random.default_rng(N)
    z = rng.standard_normal((1, 3, 2 * N))
    direct = np.einsum("kn,bfn->bkf", _cosm(N, np.float64), z)
    np.testing.assert_allclose(fft_forward(z, N), direct, atol=1e-10 * np.abs(direct).max())
    c = rng.standard_normal((1, N, 3))
    yd = np.einsum("kn,bkf->bfn", _cosm(N, np.float64), c) * 2.0 / N
    np.testing.assert_allclose(fft_frames_inv(c, N), yd, atol=1e-10 * np.abs(yd).max())


_MIXED = [40, 60, 80, 100, 120, 160, 200, 240, 300, 320, 400, 480, 500, 600, 720, 800, 960, 640, 1000, 1080, 1200, 1280]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_kernel_name_selects_fused_route(dtype):
    from tests import test_mdct_readback as RB  # (imports this module: not at the top)
    fused_m = {1 << p for p in range(4, 13)} | set(_MIXED)
    for ws in list(range(4, 700, 2)) + [960, 1000, 1920, 2048, 2560, 4096, 4094, 5120, 8190, 8192, 16384]:
        M = ws // 4 if ws % 4 == 0 else None
        fused = M in fused_m
        p = sg.MdctPlan(sg.MdctParams(ws, ws // 2, sg.WindowType.hanning), dtype, device=HOST)
        assert p.kernel_name() == ("k_mdct_fwd" if fused else "mdct_generic"), ws
        # hop == N: fused iff at least 4 frames of this split fit in the tile's 72 KiB (the table restated in test_mdct_readback)
        inst = RB.instance(ws, dtype)
        assert (inst is not None) == fused, ws
        assert p.kernel_name(inverse=True) == ("k_imdct_ola" if fused and inst[2] >= 4 else "imdct_generic"), (ws, dtype)
        p2 = sg.MdctPlan(sg.MdctParams(ws, ws // 2 + 1, sg.WindowType.hanning), dtype, device=HOST)
        assert p2.kernel_name(inverse=True) == "imdct_generic"
    for ws in (64, 256, 960, 1920, 2048, 4096):
        p = sg.MdctPlan(sg.MdctParams.sine_window(ws), dtype, device=HOST)
        assert p.kernel_name(True) == "k_imdct_ola", ws
    # the 4-frame tile is the smallest the fused inverse takes; 2 frames or 1 run the generic route at hop == N
    generic_at_hop_n = {"float32": {16384}, "float64": {4800, 5120, 8192, 16384}}[dtype]
    for ws in (4320, 4800, 5120, 8192, 16384):
        p = sg.MdctPlan(sg.MdctParams.sine_window(ws), dtype, device=HOST)
        assert p.kernel_name() == "k_mdct_fwd", ws
        assert p.kernel_name(True) == ("imdct_generic" if ws in generic_at_hop_n else "k_imdct_ola"), (ws, dtype)
    assert sg.MdctPlan(sg.MdctParams.sine_window(8192), "float32", device=HOST).kernel_name(True) == "k_imdct_ola"
    for dt, ws in (("float32", 16384), ("float64", 8192), ("float64", 5120), ("float64", 4800)):
        assert sg.MdctPlan(sg.MdctParams.sine_window(ws), dt, device=HOST).kernel_name(True) == "imdct_generic", (dt, ws)


def test_symbols_exported():
    L = _ffi.lib()
    for s in ("sgx_mdct_create", "sgx_mdct_destroy", "sgx_mdct_output_shape", "sgx_mdct_inverse_length", "sgx_mdct_forward",
              "sgx_mdct_inverse", "sgx_mdct_reserve", "sgx_mdct_window", "sgx_mdct_kernel_name", "sgx_mdct_device",
              "sgx_mdct_last_error"):
        assert s in _ffi.SYMBOLS and hasattr(L, s)
    assert {"MdctParams", "MdctPlan", "mdct", "imdct"} <= set(sg.__all__)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def _signal(rng, batch, n, dtype):
    return rng.standard_normal((batch, n)).astype(NP[dtype])


def _check_forward(plan, x, dtype, name):
    p = plan.params
    got = plan.forward(x)
    w = plan.window()
    ref = ref_forward(x, w, p.window_size, p.hop_size, dtype)
    assert got.shape == ref.shape and got.dtype == NP[dtype]
    err = np.abs(got.astype(np.float64) - ref).max(axis=1)  # [b, nf]
    bound = fwd_bound(x, w, p.window_size, p.hop_size, dtype)
    ratio = (err / bound).max()
    _record(f"forward {name} {dtype}", ratio)
    assert ratio <= 1.0, (name, dtype, ratio)
    return got


def _check_inverse(plan, c, dtype, name):
    p = plan.params
    got = plan.inverse(c)
    w = plan.window()
    ref = ola(ref_frames_inv(c, p.n_coefficients, dtype), w, p.hop_size)
    assert got.shape == ref.shape and got.dtype == NP[dtype]
    ratio = np.abs(got.astype(np.float64) - ref).max() / inv_bound(c, w, p.window_size, p.hop_size, dtype)
    _record(f"inverse {name} {dtype}", ratio)
    assert ratio <= 1.0, (name, dtype, ratio)
    return got


_CUSTOM = np.random.default_rng(11).uniform(0.2, 1.0, 256)
CASES = [  # (name, window_size, hop, window)
    *[(f"sine{ws}", ws, ws // 2, None) for ws in (64, 256, 1024, 2048, 4096, 16384, 960, 1920)],
    ("hop2N/4", 256, 64, sg.WindowType.hanning), ("hop3*2N/4", 256, 192, sg.WindowType.kaiser(6.0)),
    ("oddhop", 256, 77, sg.WindowType.hanning), ("hop2N+17", 256, 273, sg.WindowType.hanning),
    ("oddhop-960", 960, 301, sg.WindowType.blackman),
    ("generic4", 4, 2, sg.WindowType.hanning), ("generic6", 6, 3, None), ("generic18", 18, 5, sg.WindowType.kaiser(4.0)),
    ("generic1000", 1000, 500, None), ("generic1000-hop333", 1000, 333, sg.WindowType.hanning), ("generic8190", 8190, 4095, None),
    ("generic8190-hop1000", 8190, 1000, sg.WindowType.hanning), ("custom256", 256, 128, sg.WindowType.custom(_CUSTOM)),
    ("kaiser2048", 2048, 1024, sg.WindowType.kaiser(8.0)),
]


def _params(ws, hop, win):
    return sg.MdctParams.sine_window(ws) if win is None else sg.MdctParams(ws, hop, win)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name,ws,hop,win", CASES, ids=[c[0] for c in CASES])
def test_parity(name, ws, hop, win, dtype):
    rng = np.random.default_rng(ws + hop)
    plan = sg.MdctPlan(_params(ws, hop, win), dtype)
    nf = 6 if ws >= 8192 else 9
    x = _signal(rng, 2, ws + hop * (nf - 1) + hop // 2, dtype)
    _check_forward(plan, x, dtype, name)
    c = rng.standard_normal((2, ws // 2, nf)).astype(NP[dtype])
    _check_inverse(plan, c, dtype, name)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("ws", [256, 2048])
def test_frame_counts_around_tiles(ws, dtype):
    rng = np.random.default_rng(5)
    plan = sg.MdctPlan(sg.MdctParams.sine_window(ws), dtype)
    assert plan.kernel_name() == "k_mdct_fwd" and plan.kernel_name(True) == "k_imdct_ola"
    for nf in (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65):
        x = _signal(rng, 2, ws + (nf - 1) * (ws // 2), dtype)
        _check_forward(plan, x, dtype, f"tiles{ws}")
        c = rng.standard_normal((2, ws // 2, nf)).astype(NP[dtype])
        _check_inverse(plan, c, dtype, f"tiles{ws}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("ws", [18, 256, 1000, 2048, 16384])
def test_round_trip_sine(ws, dtype):
    rng = np.random.default_rng(ws)
    p = sg.MdctParams.sine_window(ws)
    N = ws // 2
    x = _signal(rng, 1, 8 * ws, dtype)[0]
    c = sg.mdct(x, p, dtype=dtype)
    y = sg.imdct(c, p, original_length=x.size, dtype=dtype)
    assert y.shape == x.shape and y.dtype == NP[dtype]
    err = np.abs(y[N:x.size - N].astype(np.float64) - x[N:x.size - N]).max()
    tol = 1e-10 if dtype == "float64" else 3e-6 * math.log2(ws) * np.abs(x).max()
    assert err <= tol, (ws, dtype, err)
    assert sg.imdct(c, p, original_length=10 ** 9, dtype=dtype).shape == (sg.MdctPlan(p, dtype).inverse_length(c.shape[1]),)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("ws,hop", [(2048, 1024), (256, 77), (18, 9)])
def test_batch_invariance_and_repeat(ws, hop, dtype):
    rng = np.random.default_rng(3)
    plan = sg.MdctPlan(sg.MdctParams(ws, hop, sg.WindowType.hanning), dtype)
    x = _signal(rng, 64, ws + 20 * hop + 3, dtype)
    c = plan.forward(x)
    np.testing.assert_array_equal(c, plan.forward(x))
    y = plan.inverse(c)
    np.testing.assert_array_equal(y, plan.inverse(c))
    for b in (0, 1, 31, 63):
        np.testing.assert_array_equal(plan.forward(x[b]), c[b])
        np.testing.assert_array_equal(plan.inverse(c[b]), y[b])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("ws,hop", [(2048, 1024), (256, 77), (1000, 500), (18, 9)])
def test_non_finite_stays_in_its_frames(ws, hop, dtype):
    rng = np.random.default_rng(9)
    p = sg.MdctParams.sine_window(ws) if hop == ws // 2 else sg.MdctParams(ws, hop, sg.WindowType.hanning)
    plan = sg.MdctPlan(p, dtype)
    nf = 12
    x = _signal(rng, 1, ws + (nf - 1) * hop, dtype)
    i = ws + 3 * hop + 1
    x[0, i] = np.nan
    got = plan.forward(x)[0]
    has = [(f * hop <= i < f * hop + ws) for f in range(nf)]
    w = plan.window()
    assert any(has) and not all(has)
    for f in range(nf):
        assert (not np.isfinite(got[:, f]).any()) if has[f] else np.isfinite(got[:, f]).all(), f
    ok = [f for f in range(nf) if not has[f]]
    xs = x.copy()
    xs[0, i] = 0.0
    ref = ref_forward(xs, w, ws, hop, dtype)[0][:, ok]
    bound = fwd_bound(xs, w, ws, hop, dtype)[0][ok]
    assert (np.abs(got[:, ok] - ref).max(axis=0) <= bound).all()
    # inverse: a non-finite coefficient of frame f reaches exactly the output samples [f hop, f hop + 2N)
    c = rng.standard_normal((ws // 2, nf)).astype(NP[dtype])
    f0 = 5
    c[7 % (ws // 2), f0] = np.inf
    y = plan.inverse(c)
    span = np.zeros(y.size, bool)
    span[f0 * hop:f0 * hop + ws] = True
    assert not np.isfinite(y[span]).any() and np.isfinite(y[~span]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("ws,hop", [(2048, 1024), (256, 77), (18, 5)])
def test_torch_and_mem_kinds_agree(ws, hop, dtype):
    import torch
    rng = np.random.default_rng(4)
    plan = sg.MdctPlan(sg.MdctParams(ws, hop, sg.WindowType.hanning), dtype)
    x = _signal(rng, 5, ws + 13 * hop, dtype)
    plan.reserve(5, x.shape[1])
    c_np = plan.forward(x)
    c_t = plan.forward_torch(torch.from_numpy(x).cuda())
    y_t = plan.inverse_torch(c_t)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c_t.cpu().numpy(), c_np)
    np.testing.assert_array_equal(y_t.cpu().numpy(), plan.inverse(c_np))
    # the raw C entry points: host and device memory on the same plan
    L = _ffi.lib()
    out_d = torch.empty(c_np.size, dtype=c_t.dtype, device="cuda")
    xd = torch.from_numpy(x).cuda()
    s = torch.cuda.current_stream().cuda_stream
    assert L.sgx_mdct_forward(plan._h, xd.data_ptr(), 5, x.shape[1], out_d.data_ptr(), c_np.size, _ffi.MEM_DEVICE, C.c_void_p(s)) == 0
    out_h = np.empty(c_np.size, NP[dtype])
    assert L.sgx_mdct_forward(plan._h, x.ctypes.data, 5, x.shape[1], out_h.ctypes.data, c_np.size, _ffi.MEM_HOST, None) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out_d.cpu().numpy(), out_h)


@pytest.mark.gpu
def test_one_shot_functions_and_cache():
    x = np.random.default_rng(2).standard_normal(4096)
    p = sg.MdctParams.sine_window(256)
    c = sg.mdct(x, p)
    assert c.dtype == np.float64 and c.shape == (128, (4096 - 256) // 128 + 1)
    np.testing.assert_array_equal(c, sg.MdctPlan(p).forward(x))
    y = sg.imdct(c, p, original_length=4000)
    assert y.shape == (4000,)
    import importlib
    mdct_mod = importlib.import_module("spectrograms_amd.mdct")
    assert len(mdct_mod._MDCT_CACHE) >= 1
    sg.clear_fft_plan_cache()
    assert len(mdct_mod._MDCT_CACHE) == 0
