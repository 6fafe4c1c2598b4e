"""The constant-Q transform plans (sgx_plan_create_cqt_transform; cqt() / CqtResult, src/cqt.rs:517-709): framing, Nyquist
truncation, validation and kernel tables on host-only plans, and on the GPU the complex coefficients of every tile shape and of the
one-frame rows route against a NumPy restatement (the kernels of tests/test_cqt.py with n_fft = klen, the frames taken from sample 0).

Complex tolerance, from the bound of tests/test_cqt.py:5-8: the engine sums the L_g taps of a bin's group as an fma chain in T, so
with u = 2^-24 / 2^-53 and mag = sum_j |x_j| max(|wr_j|, |wi_j|) over the bin's own taps, Re and Im each lie within
e = (L_g + 2) u mag of the sums of the T-cast coefficients times the T samples (summed in f64 for f32 plans, long double for f64).
NaN and Inf positions must match exactly; no value is left out.  Power / magnitude / dB outputs use check_output's bound."""
import ctypes as C
import math

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests.test_cqt import check_output, ref_cqt, ref_kernels, signals

HOST = _ffi.DEVICE_HOST_ONLY
NP = {"float32": np.float32, "float64": np.float64}
CNP = {"float32": np.complex64, "float64": np.complex128}
DTYPES = ["float32", "float64"]
DEFAULT = sg.CqtParams(12, 7, 32.7)


class Kept:
    """The CqtParams with its bins at or above Nyquist dropped (CqtKernel::generate, src/cqt.rs:333-335), for the restatement."""

    def __init__(self, cq, sr):
        self._cq = cq
        self.num_bins = next((k for k in range(cq.num_bins) if cq.bin_frequency(k) >= sr / 2.0), cq.num_bins)

    def __getattr__(self, name):
        return getattr(self._cq, name)

    def frequencies(self):
        return self._cq.frequencies()[:self.num_bins]


def tplan(cq, klen, hop, sr=16000.0, amp=_ffi.AMP_COMPLEX, floor_db=None, dtype="float32", device=HOST):
    return sg.CqtTransformPlan(sr, klen, hop, cq, amp, sg.LogParams(floor_db) if floor_db is not None else None, dtype, device)


def check_complex(got, x, cq, klen, hop, sr, dtype):
    """|Re got - Re ref| <= e and |Im got - Im ref| <= e, e = (L_g + 2) u mag; non-finite positions equal."""
    re, im, mag, lg = ref_cqt(x, Kept(cq, sr), klen, hop, sr, dtype, centre=False)
    u = 2.0 ** -24 if dtype == "float32" else 2.0 ** -53
    got = np.asarray(got)
    assert got.dtype == CNP[dtype] and got.shape == re.shape, (got.dtype, got.shape, re.shape)
    with np.errstate(invalid="ignore"):
        e = (lg[None, :, None] + 2) * u * mag
    worst = 0.0
    for g, r in ((got.real, re), (got.imag, im)):
        assert np.array_equal(np.isnan(g), np.isnan(r)), (np.isnan(g).sum(), np.isnan(r).sum())
        assert np.array_equal(np.isinf(g), np.isinf(r)) and np.array_equal(g[np.isinf(g)] > 0, r[np.isinf(r)] > 0)
        fin = np.isfinite(r)
        d = np.abs(g[fin].astype(r.dtype) - r[fin])
        assert np.all(d <= e[fin]), float(np.max(d / np.maximum(e[fin], 1e-300)))
        if d.size:
            worst = max(worst, float(np.max(d / np.maximum(e[fin], 1e-300))))
    return worst


# ---- CPU: kernel tables, truncation, framing, validation ----------------------------------------------------------------
@pytest.mark.parametrize("klen,sr,cq", [(16384, 44100.0, DEFAULT), (8000, 16000.0, sg.CqtParams(12, 6, 55.0)), (3000, 16000.0, DEFAULT)])
def test_kernel_tables(klen, sr, cq):
    first = min(klen, math.floor(cq.q_factor * sr / cq.f_min + 0.5))
    plan = tplan(cq, klen, 256, sr)
    got, ref = plan.cqt_kernels(), ref_kernels(Kept(cq, sr), sr, klen)
    assert [g.size for g in got] == [r.size for r in ref] and got[0].size == first
    for g, r in zip(got, ref):
        assert np.allclose(g, r, rtol=1e-12, atol=1e-15, equal_nan=True), np.max(np.abs(g - r))
    if klen == 16384:
        assert round(cq.q_factor * sr / cq.f_min) == 22680  # L_0 before the cap
    if klen == 3000:
        assert sum(g.size == 3000 for g in got) > 8  # more than the first group is capped: lpad = 3008 > klen


def test_nyquist_truncation():
    for cq, kept in ((sg.CqtParams(12, 9, 55.0), 87), (sg.CqtParams(12, 9, 32.7), 96), (sg.CqtParams(1, 2, 4000.0), 1)):
        plan = tplan(cq, 8000, 256)
        assert Kept(cq, 16000.0).num_bins == kept
        assert plan.output_shape(8000) == (kept, 1) and len(plan.cqt_kernels()) == kept and plan.n_bands == kept
        f, t = plan.axes(3)
        assert f.shape == (kept,) and np.allclose(f, cq.frequencies()[:kept], rtol=1e-14, atol=0) and f[-1] < 8000.0
        assert np.allclose(t, np.arange(3) * (256 / 16000.0), rtol=1e-15, atol=0)
    f = sg.CqtParams(12, 9, 55.0).frequencies()
    assert 7902 < f[86] < 7904 and 8371 < f[87] < 8373
    with pytest.raises(sg.InvalidInputError, match="no CQT bin lies below the Nyquist frequency"):
        tplan(sg.CqtParams(1, 1, 9000.0), 8000, 256)


def test_output_shape():
    for klen, hop in ((8000, 256), (16384, 512), (16384, 20000), (3000, 7)):
        plan = tplan(DEFAULT, klen, hop)
        for n in (klen, klen + hop - 1, klen + hop, klen + 5 * hop + 3):
            assert plan.output_shape(n) == (84, (n - klen) // hop + 1)
    assert tplan(DEFAULT, 16384, 20000).output_shape(16384 + 2 * 20000) == (84, 3)


def test_validation():
    cq = DEFAULT
    with pytest.raises(sg.InvalidInputError, match="custom window"):
        tplan(cq.with_window(sg.WindowType.custom(np.hanning(64))), 8000, 256)
    with pytest.raises(sg.InvalidInputError, match="16384"):
        tplan(cq, 16385, 256)
    with pytest.raises(sg.InvalidInputError, match="hop_size"):
        tplan(cq, 8000, (1 << 24) + 1)
    with pytest.raises(ValueError):
        tplan(cq, 8000, 0)
    L = _ffi.lib()
    assert L.sgx_abi_version() == 7

    def raw(centre=0, freq=_ffi.FREQ_CQT, amp=_ffi.AMP_COMPLEX):
        p = _ffi.SgxParams()
        p.n_fft, p.hop_size, p.centre, p.window_kind, p.sample_rate_hz = 8000, 256, centre, _ffi.WIN_RECTANGULAR, 16000.0
        p.freq_scale, p.amp_scale, p.dtype, p.device = freq, amp, _ffi.F32, HOST
        return p

    c = _ffi.SgxCqtParams(12, 7, 32.7, 16.8, _ffi.WIN_HANNING, 0.0, 0.01, 1)
    h = C.c_void_p()
    assert L.sgx_plan_create_cqt_transform(C.byref(raw(centre=1)), C.byref(c), C.byref(h)) == _ffi.SGX_INVALID_INPUT and not h.value
    assert b"centre" in L.sgx_last_create_error()
    assert L.sgx_plan_create_cqt_transform(C.byref(raw(freq=_ffi.FREQ_MEL)), C.byref(c), C.byref(h)) == _ffi.SGX_INVALID_INPUT
    bad = _ffi.SgxCqtParams(12, 7, float("nan"), 16.8, _ffi.WIN_HANNING, 0.0, 0.01, 1)
    assert L.sgx_plan_create_cqt_transform(C.byref(raw()), C.byref(bad), C.byref(h)) == _ffi.SGX_INVALID_INPUT
    assert b"f_min must be finite and > 0" in L.sgx_last_create_error()
    for amp in (_ffi.AMP_COMPLEX, _ffi.AMP_POWER, _ffi.AMP_MAGNITUDE, _ffi.AMP_DECIBELS):
        assert L.sgx_plan_create_cqt_transform(C.byref(raw(amp=amp)), C.byref(c), C.byref(h)) == _ffi.SGX_OK and h.value
        L.sgx_plan_destroy(h)
    # sgx_plan_create_cqt keeps its refusals
    spec = sg.SpectrogramParams(sg.StftParams(2048, 512, sg.WindowType.hanning, True), 16000.0)
    with pytest.raises(sg.InvalidInputError, match="complex"):
        sg.Plan(spec, _ffi.AMP_COMPLEX, cq, None, "float32", device=HOST)
    with pytest.raises(sg.InvalidInputError, match="CQT maximum frequency must be below Nyquist frequency"):
        sg.Plan(spec, _ffi.AMP_POWER, sg.CqtParams(12, 9, 32.7), None, "float32", device=HOST)


def test_set_route_only_on_transform_plans():
    L = _ffi.lib()
    spec = sg.SpectrogramParams(sg.StftParams(2048, 512, sg.WindowType.hanning, True), 16000.0)
    mel = sg.Plan(spec, _ffi.AMP_POWER, sg.MelParams(64, 0.0, 8000.0), None, "float32", device=HOST)
    cqs = sg.Plan(spec, _ffi.AMP_POWER, DEFAULT, None, "float32", device=HOST)
    for plan in (mel, cqs):
        assert L.sgx_cqt_set_route(plan._h, 1) == _ffi.SGX_INVALID_INPUT
        assert b"not a CQT transform plan" in L.sgx_last_error(plan._h)
    t = tplan(DEFAULT, 8000, 256)
    for route in (1, 2, 0):
        t.set_route(route)
    for route in (3, -1):
        with pytest.raises(sg.InvalidInputError, match="route"):
            t.set_route(route)


def lds_bytes(m, hop, lpad, elem):  # cqt_lds_bytes (cqt.hip): the tile's span, one skew word per hop when hop % 8 == 0
    span = (16 * m - 1) * hop + lpad
    return (span + (span // hop + 1 if hop % 8 == 0 else 0)) * elem


def lds_m(hop, lpad, elem):  # cqt_lds_m: the largest tile multiple within half the LDS, else within all of it, else 0 (global)
    for cap in (80 * 1024 - 64, 160 * 1024 - 64):
        for m in (4, 2, 1):
            if lds_bytes(m, hop, lpad, elem) <= cap:
                return m
    return 0


TILES = {64: (4, 1), 256: (2, 2), 2048: (1, 0), 4096: (0, 0)}  # hop: (f32 M, f64 M), 0 = global


def test_tile_multiples():
    cq, sr = DEFAULT, 16000.0
    L0 = len(tplan(cq, 16384, 64).cqt_kernels()[0])
    lpad = -(-L0 // 16) * 16
    assert (L0, lpad) == (8229, 8240)
    for hop, (m32, m64) in TILES.items():
        assert (lds_m(hop, lpad, 4), lds_m(hop, lpad, 8)) == (m32, m64), hop
        for dt, m in (("float32", m32), ("float64", m64)):
            assert tplan(cq, 16384, hop, dtype=dt).kernel_name == ("cqt_mfma_lds" if m else "cqt_mfma_global")


def test_cqt_result_arithmetic():
    rng = np.random.default_rng(1)
    for cdt, rdt in ((np.complex64, np.float32), (np.complex128, np.float64)):
        z = (rng.standard_normal((5, 7)) + 1j * rng.standard_normal((5, 7))).astype(cdt)
        r = sg.CqtResult(z, np.arange(5.0), 16000.0, 512)
        re, im = z.real.astype(rdt), z.imag.astype(rdt)
        pw = (re * re).astype(rdt) + (im * im).astype(rdt)
        assert r.to_power().dtype == rdt and np.array_equal(r.to_power(), pw)
        assert r.to_magnitude().dtype == rdt and np.array_equal(r.to_magnitude(), np.sqrt(pw))
        assert (r.n_bins, r.n_frames, r.shape) == (5, 7, (5, 7)) and r.time_resolution == 512 / 16000.0
        assert r.frequencies == [0.0, 1.0, 2.0, 3.0, 4.0] and r.sample_rate == 16000.0 and r.hop_size == 512
        assert np.asarray(r) is z and np.from_dlpack(r).shape == (5, 7)
        assert r.dtype == ("float32" if rdt is np.float32 else "float64")
    with pytest.raises(sg.InvalidInputError, match="samples must be non-empty"):
        sg.cqt(np.zeros(0), 16000.0, DEFAULT, 512)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def gplan(cq, klen, hop, sr=16000.0, amp=_ffi.AMP_COMPLEX, floor_db=None, dtype="float32"):
    return tplan(cq, klen, hop, sr, amp, floor_db, dtype, _ffi.DEVICE_CURRENT)


def run_complex(cq, klen, hop, sr, n, b, dtype, seed=0, route=0):
    x = signals(b, n, sr, seed)
    plan = gplan(cq, klen, hop, sr, dtype=dtype)
    plan.set_route(route)
    got = plan.compute_batch(x.astype(NP[dtype]))
    worst = check_complex(got, x, cq, klen, hop, sr, dtype)
    print(f"cqt transform {dtype} klen {klen} hop {hop} n {n} b {b}: {plan.kernel_name}, worst ratio to bound {worst:.3g}")
    return plan, got


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hop,frames", [(64, 37), (256, 37), (2048, 37), (4096, 37), (256, 38)])
def test_gpu_complex_tile_shapes(hop, frames, dtype):
    """Every tile multiple of both types and the global route; 37 frames: odd (rows only 8-byte aligned in f32), no multiple of 16."""
    n = 16384 + (frames - 1) * hop + 5
    plan, got = run_complex(DEFAULT, 16384, hop, 16000.0, n, 2, dtype)
    assert got.shape == (2, 84, frames)
    m = TILES[hop][DTYPES.index(dtype)]
    assert plan.kernel_name == ("cqt_mfma_lds" if m else "cqt_mfma_global")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_partial_last_group(dtype):
    _, got = run_complex(sg.CqtParams(12, 9, 55.0), 16384, 256, 16000.0, 16384 + 19 * 256, 2, dtype)
    assert got.shape == (2, 87, 20)  # 87 bins: a last group of 7


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_capped_kernels_and_taps_in_front_of_the_signal(dtype):
    # lpad 3008 > klen: 8 zero taps in front of sample 0; on the rows tiles and on the per-signal tiles
    for route in (2, 1):
        plan, got = run_complex(DEFAULT, 3000, 256, 16000.0, 3000, 5, dtype, route=route)
        assert got.shape == (5, 84, 1) and (plan.kernel_name == "cqt_mfma_rows") == (route == 2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_every_low_bin_capped_44k(dtype):
    _, got = run_complex(DEFAULT, 16384, 512, 44100.0, 16384 + 10 * 512, 2, dtype)
    assert got.shape == (2, 84, 11)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_hop_beyond_kernel_length(dtype):
    _, got = run_complex(DEFAULT, 16384, 20000, 16000.0, 16384 + 2 * 20000, 2, dtype)
    assert got.shape == (2, 84, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("amp,floor_db", [(_ffi.AMP_POWER, None), (_ffi.AMP_MAGNITUDE, None), (_ffi.AMP_DECIBELS, -80.0)])
def test_gpu_amplitude_kinds(amp, floor_db, dtype):
    hop, n = 256, 16384 + 36 * 256 + 5
    x = signals(2, n, 16000.0)
    got = gplan(DEFAULT, 16384, hop, amp=amp, floor_db=floor_db, dtype=dtype).compute_batch(x.astype(NP[dtype]))
    assert got.dtype == NP[dtype]
    check_output(got, x, DEFAULT, 16384, hop, 16000.0, dtype, amp, floor_db, centre=False)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["frames", "rows"])
def test_gpu_non_finite_reach(route, dtype):
    """A NaN and an Inf inside the long kernels' reach and outside the short ones' (musical: L_0 = 489 ... L_83 = 4): exactly the
    bins whose own L_k taps hold them go NaN / Inf, in Re and in Im as the reference's sums do; everything else stays in the bound."""
    cq, klen, hop, sr = sg.CqtParams.musical(), 1024, 256, 16000.0
    if route == "frames":
        x = signals(2, 8000, sr, seed=3)
        x[0, 4000] = float("nan")
        x[1, 27 * 256 + 1024 - 50] = float("inf")  # 50 taps from the end of the last frame
    else:
        x = signals(18, klen, sr, seed=3)  # one frame each: two tiles of the rows route
        x[3, klen - 100] = float("nan")
        x[17, klen - 300] = float("inf")
    plan = gplan(cq, klen, hop, sr, dtype=dtype)
    plan.set_route(2 if route == "rows" else 0)
    got = plan.compute_batch(x.astype(NP[dtype]))
    assert plan.kernel_name == ("cqt_mfma_rows" if route == "rows" else "cqt_mfma_lds")
    bad = ~np.isfinite(got)
    assert bad.any() and not bad.all(axis=1).any()  # no frame loses its short bins
    check_complex(got, x, cq, klen, hop, sr, dtype)
    for amp, floor_db in ((_ffi.AMP_POWER, None), (_ffi.AMP_DECIBELS, -80.0)):
        out = gplan(cq, klen, hop, sr, amp, floor_db, dtype).compute_batch(x.astype(NP[dtype]))
        check_output(out, x, cq, klen, hop, sr, dtype, amp, floor_db, centre=False)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_rows_route_equals_per_signal_tiles(dtype):
    """One frame per signal: tiles of 16 signals.  Parity, and the same bits as the per-signal tiles (the same k-ordered fma chain
    over the same taps), for complex and for power output, at batches around the tile."""
    cq, klen, hop, sr = sg.CqtParams(12, 6, 55.0), 8000, 256, 16000.0
    x = signals(70, klen, sr, seed=7)
    xt = x.astype(NP[dtype])
    for amp in (_ffi.AMP_COMPLEX, _ffi.AMP_POWER):
        plan = gplan(cq, klen, hop, sr, amp=amp, dtype=dtype)
        for b in (1, 15, 16, 17, 70):
            plan.set_route(2)
            got = plan.compute_batch(xt[:b])
            assert plan.kernel_name == "cqt_mfma_rows"
            if amp == _ffi.AMP_COMPLEX:
                check_complex(got, x[:b], cq, klen, hop, sr, dtype)
            else:
                check_output(got, x[:b], cq, klen, hop, sr, dtype, amp, None, centre=False)
            plan.set_route(1)
            tiles = plan.compute_batch(xt[:b])
            assert plan.kernel_name in ("cqt_mfma_lds", "cqt_mfma_global")
            assert np.array_equal(got.view(NP[dtype]), tiles.view(NP[dtype])), (amp, b)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_automatic_route_threshold(dtype):
    """Automatic selection keeps the per-signal tiles below ROWS_MIN_BATCH one-frame signals and takes the rows tiles from there on;
    the same bits on both sides of the threshold as with the route forced."""
    from spectrograms_amd.cqt import ROWS_MIN_BATCH
    import torch
    cq, klen, hop, sr = sg.CqtParams.musical(), 1024, 256, 16000.0
    tdt = torch.float32 if dtype == "float32" else torch.float64
    x = torch.from_numpy(signals(1, ROWS_MIN_BATCH * klen, sr, seed=13).reshape(ROWS_MIN_BATCH, klen)).to(tdt).cuda()
    plan = gplan(cq, klen, hop, sr, dtype=dtype)
    below = plan.compute_batch(x[:ROWS_MIN_BATCH - 1]).clone()
    assert plan.kernel_name == "cqt_mfma_lds"
    at = plan.compute_batch(x).clone()
    assert plan.kernel_name == "cqt_mfma_rows"
    plan.set_route(1)
    tiles = plan.compute_batch(x)
    assert plan.kernel_name == "cqt_mfma_lds"
    assert torch.equal(torch.view_as_real(at), torch.view_as_real(tiles))
    assert torch.equal(torch.view_as_real(below), torch.view_as_real(tiles[:ROWS_MIN_BATCH - 1]))
    # one frame more per signal: the frame tiles whatever the route
    plan.set_route(2)
    plan.compute_batch(torch.cat([x[:4], x[:4, :hop]], dim=1))
    assert plan.kernel_name == "cqt_mfma_lds"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_repeat_host_resident_and_reserved_capture(dtype):
    import torch
    cq, klen, hop, sr = DEFAULT, 16384, 256, 16000.0
    x = signals(3, klen + 20 * hop + 1, sr, seed=5).astype(NP[dtype])
    plan = gplan(cq, klen, hop, sr, dtype=dtype)
    xd = torch.from_numpy(x).cuda()
    first = plan.compute_batch(xd).clone()
    for _ in range(2):
        again = plan.compute_batch(xd)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(first), torch.view_as_real(again))
    assert np.array_equal(plan.compute_batch(x).view(NP[dtype]), first.cpu().numpy().view(NP[dtype]))  # host path: the same bits
    res = plan.compute_batch_resident(xd)
    assert res.shape == (3, 84, 21) and np.allclose(res.frequencies, cq.frequencies(), rtol=1e-14, atol=0)
    assert np.allclose(res.times, np.arange(21) * (hop / sr), rtol=1e-15, atol=0)
    # after reserve the device call allocates nothing: captured once on a side stream, replayed on new samples
    fresh = gplan(cq, klen, hop, sr, dtype=dtype)
    fresh.reserve(3, x.shape[1], host_staging=False)
    x2 = torch.from_numpy(signals(3, x.shape[1], sr, seed=6).astype(NP[dtype])).cuda()
    want = plan.compute_batch(x2).clone()
    sin, out = xd.clone(), torch.full((3, 84, 21, 2), -1.0e30, dtype=xd.dtype, device=xd.device)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fresh.compute_batch(sin, out=out)
    for src, ref in ((x2, want), (xd, first)):
        sin.copy_(src)
        out.fill_(-1.0e30)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, torch.view_as_real(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_cqt_function(dtype):
    """cqt() picks klen = min(n, 16384) and equals the plan; a batch equals its rows one by one; the reference's own test shape."""
    import torch
    cq, sr, hop = sg.CqtParams(12, 6, 55.0), 16000.0, 512
    for n in (8000, 16384 + 3 * hop + 7):  # one frame on the rows route; four frames on the frame tiles
        klen = min(n, 16384)
        x = signals(3, n, sr, seed=9).astype(NP[dtype])
        r = sg.cqt(x, sr, cq, hop, dtype)
        assert isinstance(r, sg.CqtResult) and r.data.dtype == CNP[dtype] and r.shape == (3, 72, (n - klen) // hop + 1)
        assert (r.n_bins, r.n_frames, r.sample_rate, r.hop_size) == (72, (n - klen) // hop + 1, sr, hop)
        assert np.allclose(r.frequencies, cq.frequencies(), rtol=1e-14, atol=0)
        assert np.array_equal(r.data.view(NP[dtype]), gplan(cq, klen, hop, sr, dtype=dtype).compute_batch(x).view(NP[dtype]))
        for i in range(3):
            one = sg.cqt(x[i], sr, cq, hop, dtype)
            assert one.shape == r.shape[1:] and np.array_equal(one.data.view(NP[dtype]), r.data[i].view(NP[dtype]))
        check_complex(r.data, x, cq, klen, hop, sr, dtype)
        t = sg.cqt(torch.from_numpy(x).cuda(), sr, cq, hop, dtype)
        assert np.array_equal(t.data.cpu().numpy().view(NP[dtype]), r.data.view(NP[dtype]))
        # to_power / to_magnitude of the result against the restatement, as the plans with those outputs (test_gpu_amplitude_kinds)
        for amp, arr in ((_ffi.AMP_POWER, r.to_power()), (_ffi.AMP_MAGNITUDE, r.to_magnitude())):
            assert arr.dtype == NP[dtype]
            check_output(arr, x, Kept(cq, sr), klen, hop, sr, dtype, amp, None, centre=False)
