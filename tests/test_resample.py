"""Sample-rate conversion plans (sgx_resample_*, spectrograms_amd/resample.py).

The definition (include/spectro_hip.h; torchaudio.functional.resample's semantics without its padding of every phase kernel), with
g = gcd(orig, new), M = orig / g, L = new / g, base = min(L, M) rolloff:
    phi(t) = sinc(t) w(t / lpw) for |t| < lpw, 0 otherwise;   w(u) = cos^2(pi u / 2) (hann) | I0(beta sqrt(1 - u^2)) / I0(beta) (kaiser)
    y[m]   = (base / M) sum_n x[n] phi(base (n / M - m / L)),   0 <= m < ceil(n L / M),   x = 0 outside the row
and its polyphase form y[q L + p] = sum_{k < K} c[p][k] x[q M + j0(p) + k].  `phi_ref` / `table_ref` restate it in NumPy f64; the CPU
tests pin the plan's table to it (host-only plans), everything downstream of that check — here and in
tests/test_resample_readback.py — takes K, j0 and the T-valued table from the plan's accessors.

GPU tests here: the per-sample bound, streaming, locality of a non-finite sample, stream order.  Every case runs a batch of 3 rows of
different data, in both types, on both routes (`route="generic"` forced on the same shapes).
"""
import functools
import math

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi

HOST = _ffi.DEVICE_HOST_ONLY
F32, F64 = "float32", "float64"
NP = {F32: np.float32, F64: np.float64}
U = {F32: 2.0 ** -24, F64: 2.0 ** -53}
LD = np.longdouble
KAISER_BETA = 14.769656459379492
GENERIC_ONLY = (8, 1)  # K = 97 > 64 coefficient registers: outside k_resample_pp's budget
RATIOS = [(3, 1), (1, 3), (2, 1), (3, 2), (7, 5), (44100, 16000), (44100, 48000), GENERIC_ONLY]
# orig -> new: M, L, K, L K, min j0, max j0 at the defaults
TABLE = {(48000, 16000): (3, 1, 37, 37, -18, -18), (44100, 16000): (441, 160, 34, 5440, -16, 422), (16000, 48000): (1, 3, 13, 39, -6, -5),
         (44100, 48000): (147, 160, 13, 2080, -6, 141), (3, 2): (3, 2, 19, 38, -9, -7), (7, 5): (7, 5, 17, 85, -8, -2)}
CASES = [(r, dt, route) for r in RATIOS for dt in (F32, F64) for route in ("auto", "generic") if not (r == GENERIC_ONLY and route == "generic")]
CASE_IDS = [f"{o}to{n}-{dt[5:]}-{route}" for (o, n), dt, route in CASES]


# ---- the definition in NumPy f64 -----------------------------------------------------------------------------------------------------
def phi_ref(t, lpw=6, method="sinc_interp_hann", beta=KAISER_BETA):
    t = np.asarray(t, np.float64)
    u = t / lpw
    if method == "sinc_interp_kaiser":
        w = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / np.i0(beta)
    else:
        w = np.cos(np.pi * u / 2.0) ** 2
    return np.where(np.abs(t) < lpw, np.sinc(t) * w, 0.0)


def reduced(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def tap_times(M, L, base, j0, K):
    """t of tap k of phase p: base ((j0(p) + k) / M - p / L), shape (L, K)."""
    j = j0[:, None] + np.arange(K)[None, :]
    p = np.arange(L)[:, None]
    return base * (j * L - p * M) / float(M * L)


def table_ref(plan, lpw=6, rolloff=0.99, method="sinc_interp_hann", beta=KAISER_BETA):
    M, L, K, j0 = plan.down, plan.up, plan.taps_per_phase, plan.phase_offsets()
    base = min(L, M) * rolloff
    return (base / M) * phi_ref(tap_times(M, L, base, j0, K), lpw, method, beta), base


# ---- shared inputs and references ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_plan(orig, new, dtype=F64, **kw):
    return sg.ResamplePlan(orig, new, dtype=dtype, device=HOST, **dict(kw))


@functools.lru_cache(maxsize=None)
def geometry(orig, new, dtype, **kw):
    """(M, L, K, j0, T-valued table as f64, tile of the tuned route or 1024 where the ratio has none); `kw`: the filter keywords."""
    p = host_plan(orig, new, dtype, **kw)
    return p.down, p.up, p.taps_per_phase, p.phase_offsets(), p.taps(), p.tile or 1024


def noise(n, dtype, seed, batch=3):
    """f32-valued rows of different data in both types."""
    x = np.random.default_rng(seed).standard_normal((batch, n)).astype(np.float32)
    return x.astype(NP[dtype])


def windows(x, M, L, K, j0, n_out=None):
    """The (n_out, K) samples each output of a 1-D row reads, zeros outside the row, and each output's phase."""
    n = x.shape[0]
    n_out = -(-n * L // M) if n_out is None else n_out
    m = np.arange(n_out)
    start = (m // L) * M + j0[m % L]
    left = max(0, -int(start.min())) if n_out else 0
    right = max(0, int(start.max()) + K - n) if n_out else 0
    xp = np.concatenate([np.zeros(left, x.dtype), x, np.zeros(right, x.dtype)])
    return xp[(start + left)[:, None] + np.arange(K)[None, :]], m % L


def exact_rows(x, geo):
    """y and the bound's sum_k |c| |x| per output, in long double (u = 2^-64: exact beside either type's bound)."""
    M, L, K, j0, tab, _ = geo
    ys, mags = [], []
    for row in x:
        X, ph = windows(row, M, L, K, j0)
        C = tab[ph].astype(LD)
        ys.append(np.sum(C * X.astype(LD), axis=1))
        mags.append(np.sum(np.abs(C) * np.abs(X.astype(LD)), axis=1))
    return np.stack(ys), np.stack(mags)


def n_for(outputs, M, L):
    """The smallest row length with at least `outputs` outputs: ceil(n L / M) >= T  <=>  n > (T - 1) M / L."""
    return max(1, (outputs - 1) * M // L + 1)


def lengths(geo):
    """1, K - 1, K, and the rows that end one output before, on and one after a tile seam (the nearest reachable counts when L > M)."""
    M, L, K, _, _, tile = geo
    return sorted({1, max(1, K - 1), K, n_for(tile - 1, M, L), n_for(tile, M, L), n_for(tile + 1, M, L)})


def gpu_plan(ratio, dtype, route):
    plan = sg.ResamplePlan(*ratio, dtype=dtype, route=route)
    want = "resample_generic" if route == "generic" or ratio == GENERIC_ONLY else "k_resample_pp"
    assert plan.kernel_name == want, (plan.kernel_name, want)
    return plan


# ---------------------------------------------------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("kw", [{}, {"resampling_method": "sinc_interp_kaiser"}, {"lowpass_filter_width": 16, "rolloff": 0.9475937167399596,
                                                                                 "resampling_method": "sinc_interp_kaiser", "beta": 14.769656459379492},
                                {"lowpass_filter_width": 3, "rolloff": 1.0}], ids=["hann", "kaiser", "kaiser16", "hann3"])
@pytest.mark.parametrize("ratio", RATIOS + [(48000, 16000), (16000, 48000), (22050, 16000)], ids=lambda r: f"{r[0]}to{r[1]}")
def test_table_matches_the_formula(ratio, kw):
    """|c - formula| <= 2^-40 base / M on the f64 plan (the cap covers two libms' sin / cos / I0); the f32 plan holds the same table
    rounded once."""
    p64 = host_plan(*ratio, F64, **kw)
    ref, base = table_ref(p64, kw.get("lowpass_filter_width", 6), kw.get("rolloff", 0.99), kw.get("resampling_method", "sinc_interp_hann"),
                          kw.get("beta", KAISER_BETA))
    got = p64.taps()
    assert got.shape == ref.shape == (p64.up, p64.taps_per_phase)
    assert np.max(np.abs(got - ref)) <= 2.0 ** -40 * base / p64.down, np.max(np.abs(got - ref))
    p32 = host_plan(*ratio, F32, **kw)
    assert np.array_equal(p32.phase_offsets(), p64.phase_offsets())
    assert np.array_equal(p32.taps(), got.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("ratio", list(TABLE), ids=lambda r: f"{r[0]}to{r[1]}")
def test_table_of_values(ratio):
    M, L, K, LK, jlo, jhi = TABLE[ratio]
    for dt in (F32, F64):
        p = host_plan(*ratio, dt)
        j0 = p.phase_offsets()
        assert (p.down, p.up, p.taps_per_phase, p.up * p.taps_per_phase, int(j0.min()), int(j0.max())) == (M, L, K, LK, jlo, jhi)
        assert p.kernel_name == "k_resample_pp" and p.tile > 0 and p.tile % L == 0 and p.device == HOST


def test_equal_rates_are_the_identity():
    p = host_plan(8000, 8000)
    assert (p.down, p.up, p.taps_per_phase) == (1, 1, 1)
    assert np.array_equal(p.taps(), [[1.0]]) and np.array_equal(p.phase_offsets(), [0])
    assert p.out_len(17) == 17 and p.step(5, 3) == (3, 8) and p.step(5, 0) == (0, 0)


@pytest.mark.parametrize("kw", [{}, {"lowpass_filter_width": 16, "rolloff": 0.9475937167399596, "resampling_method": "sinc_interp_kaiser"}],
                         ids=["default", "kaiser16"])
@pytest.mark.parametrize("ratio", RATIOS + [(48000, 16000), (22050, 16000), (1000, 999)], ids=lambda r: f"{r[0]}to{r[1]}")
def test_support_is_covered_and_K_is_tight(ratio, kw):
    """Every j with |t_j| < lpw - 1e-9 lies in [j0(p), j0(p) + K); K <= floor(2 lpw M / base) + 2; window starts rise with m."""
    p = host_plan(*ratio, F64, **kw)
    M, L, K, j0 = p.down, p.up, p.taps_per_phase, p.phase_offsets()
    lpw, base = kw.get("lowpass_filter_width", 6), min(L, M) * kw.get("rolloff", 0.99)
    assert K <= math.floor(2 * lpw * M / base) + 2
    reach = int(math.ceil(lpw * M / base)) + 2
    ph = np.arange(L)[:, None]
    j = np.floor(ph * M / L).astype(np.int64) + np.arange(-reach, reach + 1)[None, :]
    inside = np.abs(base * (j * L - ph * M) / float(M * L)) < lpw - 1e-9
    assert np.all(~inside | ((j >= j0[:, None]) & (j < j0[:, None] + K)))
    assert np.all(np.diff(j0) >= 0) and j0[-1] <= j0[0] + M


@pytest.mark.parametrize("ratio", RATIOS + [(8000, 8000)], ids=lambda r: f"{r[0]}to{r[1]}")
def test_out_len(ratio):
    p = host_plan(*ratio)
    M, L = reduced(*ratio)
    for n in (1, 2, 3, M - 1, M, M + 1, 2 * M + 1, 1000, 15999, 16000, 441000, 2 ** 40):
        if n >= 1:
            assert p.out_len(n) == -(-n * L // M), n


def brute_emitted(N, M, L, K, j0):
    m = np.arange((N // M + 2) * L + L)
    return int(np.count_nonzero((m // L) * M + j0[m % L] + K - 1 <= N - 1))


@pytest.mark.parametrize("ratio", RATIOS + [(8000, 8000), (22050, 16000)], ids=lambda r: f"{r[0]}to{r[1]}")
def test_step_against_a_brute_force_count(ratio):
    """E(N) = #{m : floor(m / L) M + j0(m mod L) + K - 1 <= N - 1} for every N in 0 .. 2 M + K; a push returns E(N + n) - E(N), a flush
    ceil(N L / M) - E(N)."""
    p = host_plan(*ratio)
    M, L, K, j0 = p.down, p.up, p.taps_per_phase, p.phase_offsets()
    E = [brute_emitted(N, M, L, K, j0) for N in range(2 * M + K + 8)]
    for N in range(1, 2 * M + K + 1):
        assert p.step(0, N) == (E[N], N), N
        assert p.step(N, 7) == (E[N + 7] - E[N], N + 7), N
        assert p.step(N, 0) == (-(-N * L // M) - E[N], 0), N
    assert p.step(0, 0) == (0, 0)
    assert p.consumed == 0 and p.emitted == 0


def test_step_check_values():
    p = host_plan(44100, 16000)
    assert [p.step(0, N)[0] if N else 0 for N in (0, 10, 50, 51, 52, 441, 1000)] == [0, 0, 12, 13, 13, 154, 357]


def test_error_texts():
    bad = [(dict(orig_freq=0, new_freq=16000), "orig_freq and new_freq must be positive integers"),
           (dict(orig_freq=16000, new_freq=-1), "orig_freq and new_freq must be positive integers"),
           (dict(orig_freq=44100.5, new_freq=16000), "orig_freq must be an integer"),
           (dict(orig_freq=2, new_freq=1, rolloff=0.0), r"rolloff must be in \(0, 1\]"),
           (dict(orig_freq=2, new_freq=1, rolloff=1.01), r"rolloff must be in \(0, 1\]"),
           (dict(orig_freq=2, new_freq=1, rolloff=float("nan")), r"rolloff must be in \(0, 1\]"),
           (dict(orig_freq=2, new_freq=1, lowpass_filter_width=0), "lowpass_filter_width must be >= 1"),
           (dict(orig_freq=2, new_freq=1, resampling_method="linear"), "resampling_method must be sinc_interp_hann or sinc_interp_kaiser"),
           (dict(orig_freq=2, new_freq=1, resampling_method="sinc_interp_kaiser", beta=float("inf")), "beta must be finite"),
           (dict(orig_freq=1000003, new_freq=1000000), "the reduced ratio 1000003 : 1000000 needs a table"),
           (dict(orig_freq=2000006, new_freq=2000000), "the reduced ratio 1000003 : 1000000 needs a table")]
    for kw, text in bad:
        with pytest.raises(sg.InvalidInputError, match="Invalid input: .*" + text):
            sg.ResamplePlan(device=HOST, **kw)
    with pytest.raises(ValueError, match="route must be"):
        sg.ResamplePlan(2, 1, route="fast", device=HOST)
    with pytest.raises(ValueError):
        sg.ResamplePlan(2, 1, dtype="float16", device=HOST)
    with pytest.raises(sg.InvalidInputError, match="must not be empty"):
        sg.resample(np.zeros(0), 2, 1)
    with pytest.raises(ValueError):
        sg.resample(np.zeros((2, 2, 2)), 2, 1)


def test_routes_and_the_budget():
    """K <= 64 coefficient registers and L <= 512 work items bound the tuned route; everything else, and any ratio on request, is generic."""
    assert host_plan(*GENERIC_ONLY).taps_per_phase > 64
    for ratio, dt, route in CASES:
        p = sg.ResamplePlan(*ratio, dtype=dt, route=route, device=HOST)
        generic = route == "generic" or ratio == GENERIC_ONLY
        assert p.kernel_name == ("resample_generic" if generic else "k_resample_pp") and (p.tile == 0) == generic
    assert host_plan(1000, 999).kernel_name == "resample_generic"   # L = 999 phases
    assert host_plan(44100, 16000, lowpass_filter_width=64).kernel_name == "resample_generic"
    assert host_plan(22050, 16000).kernel_name == "k_resample_pp"   # L = 320
    assert host_plan(8000, 8000).kernel_name == "k_resample_pp"


def test_host_only_plan_refuses_compute_loudly():
    p = sg.ResamplePlan(3, 2, dtype=F32, device=HOST)
    x = np.zeros((2, 100), np.float32)
    for call in (p.resample, p.process):
        with pytest.raises(sg.FFTBackendError, match="no HIP device"):
            call(x)
    with pytest.raises(sg.FFTBackendError, match="no HIP device"):
        p.reserve(2, 100)
    assert p.flush().shape == (0,) and p.consumed == 0 and p.allocations == 0
    p.reset()
    L = _ffi.lib()
    assert L.sgx_resample_resample(p._h, x.ctypes.data, 2, 100, 100, x.ctypes.data, 5, _ffi.MEM_HOST, None) == _ffi.SGX_DIM_MISMATCH
    assert "expected 134, got 5" in L.sgx_resample_last_error(p._h).decode()
    assert L.sgx_resample_resample(p._h, x.ctypes.data, 2, 100, 99, x.ctypes.data, 134, _ffi.MEM_HOST, None) == _ffi.SGX_INVALID_INPUT
    assert L.sgx_resample_step(None, 0, 1, None, None) == _ffi.SGX_INVALID_INPUT


def test_exports():
    for name in ("ResamplePlan", "resample"):
        assert hasattr(sg, name) and name in sg.__all__
    for sym in ("sgx_resample_create", "sgx_resample_process", "sgx_resample_step", "sgx_resample_phase_offsets", "sgx_resample_tile"):
        assert sym in _ffi.SYMBOLS and hasattr(_ffi.lib(), sym)
    assert _ffi.lib().sgx_abi_version() == 7


# ---------------------------------------------------------------------------------------------------------------------------- GPU tests
def bound_inputs(geo, dtype):
    """3 rows of 1.5 tiles: noise; a 10^6 : 1 level step, loud first, in the middle of the first tile; noise with a silent stretch."""
    M, L, K, _, _, tile = geo
    n = -(-3 * tile * M // (2 * L)) + 3
    x = noise(n, dtype, 11)
    cut = (tile // 2) * M // L
    x[1, cut:] *= NP[dtype](1e-6)
    lo = n // 3
    x[2, lo:lo + 3 * K + 2 * M] = 0
    return x


def check_bound(y, x, geo, dtype):
    """|dy[m]| <= (K + 1) u sum_k |c[p][k]| |x[..]| (gamma_K of the chain; nothing here is measured); exactly 0 over silent windows."""
    ref, mag = exact_rows(x, geo)
    assert y.shape == ref.shape and y.dtype == NP[dtype]
    err = np.abs(y.astype(LD) - ref)
    bound = (geo[2] + 1) * U[dtype] * mag
    worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    assert np.all(err <= bound), worst
    assert np.all(y[mag == 0] == 0)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,dtype,route", CASES, ids=CASE_IDS)
def test_gpu_per_sample_bound(ratio, dtype, route):
    """Every row length of `lengths` on noise, and the level-step / silent-stretch rows: each output within the bound of its own
    window, so the quiet side of a 10^6 : 1 step keeps its own precision."""
    geo = geometry(*ratio, dtype)
    plan = gpu_plan(ratio, dtype, route)
    for n in lengths(geo):
        x = noise(n, dtype, 100 + n)
        y = plan.resample(x)
        assert y.shape == (3, plan.out_len(n))
        check_bound(y, x, geo, dtype)
        assert np.array_equal(plan.resample(x[1]), y[1])  # 1-D in, 1-D out
    x = bound_inputs(geo, dtype)
    y = plan.resample(x)
    check_bound(y, x, geo, dtype)
    assert np.count_nonzero(y[2] == 0) >= 1 and np.all(y[1] != 0)
    assert plan.consumed == 0 and plan.emitted == 0  # the stateless form leaves the stream alone


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
def test_gpu_identity_and_one_shot(dtype):
    x = noise(1000, dtype, 5)
    for route in ("auto", "generic"):
        assert np.array_equal(sg.ResamplePlan(8000, 8000, dtype=dtype, route=route).resample(x), x)
    assert np.array_equal(sg.resample(x, 8000, 8000, dtype=dtype), x)
    y = sg.resample(x.astype(np.float64), 3, 2)
    assert y.dtype == np.float64 and y.shape == (3, 667)
    check_bound(y, x.astype(np.float64), geometry(3, 2, F64), F64)


def chunks_of(n, M):
    """1, 7, M - 1, M, M + 1 and a long remainder."""
    cut = [c for c in (1, 7, M - 1, M, M + 1) if c > 0]
    assert sum(cut) < n
    return cut + [n - sum(cut)]


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,dtype,route", CASES, ids=CASE_IDS)
def test_gpu_streaming_is_bit_equal_to_one_call(ratio, dtype, route):
    geo = geometry(*ratio, dtype)
    M, L, K = geo[:3]
    n = sum(c for c in (1, 7, M - 1, M, M + 1) if c > 0) + -(-3 * geo[5] * M // (2 * L)) + 5
    x = noise(n, dtype, 21)
    plan = gpu_plan(ratio, dtype, route)
    whole = plan.resample(x)
    parts, at = [], 0
    for c in chunks_of(n, M):
        want = plan.step(plan.consumed, c)[0]
        y = plan.process(x[:, at:at + c])
        at += c
        assert y.shape == (3, want) and plan.consumed == at and plan.emitted == sum(p.shape[1] for p in parts) + want
        parts.append(y)
        if len(parts) == 3:  # another batch: refused, and no state moves
            before = (plan.consumed, plan.emitted)
            with pytest.raises(sg.DimensionMismatchError, match="expected 3, got 2"):
                plan.process(x[:2, at:at + 5])
            assert (plan.consumed, plan.emitted) == before
    tail = plan.flush()
    assert tail.shape == (3, plan.out_len(n) - sum(p.shape[1] for p in parts))
    assert np.array_equal(np.concatenate(parts + [tail], axis=1), whole)
    assert plan.consumed == 0 and plan.emitted == 0
    # after the flush (as after reset) the row count is free again, and the history is zeros
    y1 = plan.process(x[0, :K + M])
    assert np.array_equal(np.concatenate([y1, plan.flush()]), plan.resample(x[0, :K + M]))
    plan.process(x[:2, :K])
    plan.reset()
    assert plan.consumed == 0
    y3 = plan.process(x[:, :K + M])
    assert np.array_equal(np.concatenate([y3, plan.flush()], axis=1), plan.resample(x[:, :K + M]))


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,dtype,route", CASES, ids=CASE_IDS)
def test_gpu_non_finite_sample_stays_local(ratio, dtype, route):
    """One NaN in the middle of a tile: every output with a non-zero coefficient on it is NaN, every output whose K-window does not
    cover it is finite and bit-equal to the clean run."""
    geo = geometry(*ratio, dtype)
    M, L, K, j0, tab, tile = geo
    n = -(-3 * tile * M // (2 * L)) + 3
    x = noise(n, dtype, 31)
    at = (tile // 2) * M // L + 1
    plan = gpu_plan(ratio, dtype, route)
    clean = plan.resample(x)
    x[1, at] = np.nan
    y = plan.resample(x)
    m = np.arange(clean.shape[1])
    k = at - ((m // L) * M + j0[m % L])
    covered = (k >= 0) & (k < K)
    hit = np.zeros_like(covered)
    hit[covered] = tab[(m % L)[covered], k[covered]] != 0
    assert hit.sum() >= 1
    assert np.all(np.isnan(y[1][hit]))
    assert np.all(np.isfinite(y[1][~covered])) and np.array_equal(y[1][~covered], clean[1][~covered])
    assert np.array_equal(y[[0, 2]], clean[[0, 2]])


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,dtype,route", [c for c in CASES if c[0] in ((3, 1), (44100, 16000), (1, 3), GENERIC_ONLY)],
                         ids=[i for c, i in zip(CASES, CASE_IDS) if c[0] in ((3, 1), (44100, 16000), (1, 3), GENERIC_ONLY)])
def test_gpu_stream_order(ratio, dtype, route):
    """resample_torch and a cut of process_torch / flush_torch back to back on a side stream, inputs as views into one tensor, one
    synchronise at the end: bit for bit the host-array results; after reserve() `allocations` stands still; a captured resample_torch
    (one stream, a linear chain) replays to the same bits on new data in the same buffers."""
    torch = pytest.importorskip("torch")
    geo = geometry(*ratio, dtype)
    M, L, K = geo[:3]
    n = sum(c for c in (1, 7, M - 1, M, M + 1) if c > 0) + -(-3 * geo[5] * M // (2 * L)) + 5
    xs = [noise(n, dtype, 41 + i) for i in range(3)]
    ref_plan = gpu_plan(ratio, dtype, route)
    refs = [ref_plan.resample(x) for x in xs]
    dev = [torch.from_numpy(x).cuda() for x in xs]
    plan = gpu_plan(ratio, dtype, route)
    cut = chunks_of(n, M)
    plan.reserve(3, max(cut), host_staging=False)
    count = plan.allocations
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        whole = plan.resample_torch(dev[0])
        parts, at = [], 0
        for c in cut:
            parts.append(plan.process_torch(dev[0][:, at:at + c]))
            at += c
        parts.append(plan.flush_torch())
        again = plan.resample_torch(dev[1])
    side.synchronize()
    assert plan.allocations == count
    assert np.array_equal(whole.cpu().numpy(), refs[0]) and np.array_equal(again.cpu().numpy(), refs[1])
    assert np.array_equal(torch.cat(parts, dim=1).cpu().numpy(), refs[0])
    with pytest.raises(sg.DimensionMismatchError):
        plan.resample_torch(dev[0], out=torch.empty((3, 5), dtype=dev[0].dtype, device="cuda"))
    # capture
    xin, out = dev[0].clone(), torch.full_like(whole, -1.0e30)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.resample_torch(xin, out=out)
    for i in (2, 1, 0):
        xin.copy_(dev[i])
        out.fill_(-1.0e30)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), refs[i]), f"replay on input {i} differs from the eager result"
    assert plan.allocations == count
