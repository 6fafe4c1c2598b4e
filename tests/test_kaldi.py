"""Kaldi fbank / MFCC plans (sgx_kaldi_*, spectrograms_amd.KaldiPlan) against tests/kaldi_ref.py, the NumPy restatement of the
semantics in include/spectro_hip.h.

CPU part (host-only plans): symbols and exports; the tables against the restatement to 4 * 2^-53 relative; the bank's structure; the
frame counts of both edge modes; the restatement itself pinned against the explicit matrix product
F_P pad diag(w) (I - alpha S) (I - 1 1^T / N); two analytic cases; every refused field and validation limit; the routes; the named GPU
cases are exactly the compiled instances of k_kaldi; the bound's range condition r <= 0.1 on the reference of every GPU case.

GPU part: every case asserts |got - ref| / bound <= 1 per output element (the bound: tests/kaldi_ref.py) and prints its worst ratio.
Inputs are rows 0.3 + 0.1 N(0, 1) from a seeded default_rng; the offset exercises the DC removal.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests import kaldi_ref as KR
from tests import test_forward_readback as FR

F32, F64 = "float32", "float64"
DTYPES = (F32, F64)
HOST = _ffi.DEVICE_HOST_ONLY
CSRC = os.path.join(os.path.dirname(os.path.abspath(_ffi.__file__)), "csrc")
TILE = 32  # frames per workgroup tile of k_kaldi (asserted against the plan)
WORST = {}


def KP(**kw):
    return sg.KaldiParams(**kw)


def host(dtype=F32, route="auto", **kw):
    return sg.KaldiPlan(KP(**kw), dtype, device=HOST, route=route)


def record(route, P, dtype, r):
    WORST[(route, P, dtype)] = max(WORST.get((route, P, dtype), 0.0), float(r))


# ---- CPU: symbols, tables, frame counts --------------------------------------------------------------------------------------------------
def test_symbols_and_exports():
    L = C.CDLL(_ffi.LIB_PATH)
    names = [s for s in _ffi.SYMBOLS if s.startswith("sgx_kaldi_")]
    assert {"sgx_kaldi_create", "sgx_kaldi_destroy", "sgx_kaldi_last_error", "sgx_kaldi_device", "sgx_kaldi_kernel_name", "sgx_kaldi_window_size",
            "sgx_kaldi_window_shift", "sgx_kaldi_padded_window_size", "sgx_kaldi_n_out", "sgx_kaldi_tile", "sgx_kaldi_allocations",
            "sgx_kaldi_n_frames", "sgx_kaldi_window", "sgx_kaldi_mel_banks", "sgx_kaldi_dct", "sgx_kaldi_lifter", "sgx_kaldi_execute",
            "sgx_kaldi_reserve"} == set(names)
    for s in names:
        assert hasattr(L, s), s
    for name in ("KaldiParams", "KaldiPlan", "kaldi_fbank", "kaldi_mfcc"):
        assert name in sg.__all__ and hasattr(sg, name)
    assert _ffi.lib().sgx_abi_version() == 7


def test_one_shot_cache_is_cleared_with_the_others():
    from spectrograms_amd import kaldi as K
    K._KALDI_CACHE.get("probe", lambda: 1)
    assert len(K._KALDI_CACHE) >= 1
    sg.clear_fft_plan_cache()
    assert len(K._KALDI_CACHE) == 0


def rel_close(got, ref):
    return np.all(np.abs(got - ref) <= 4 * 2.0 ** -53 * np.abs(ref))


# (fs, frame_length ms) -> N = 400, 200, 1200, 25
TABLE_SIZES = {400: (16000.0, 25.0), 200: (8000.0, 25.0), 1200: (48000.0, 25.0), 25: (1000.0, 25.0)}


@pytest.mark.parametrize("kind", KR.WINDOWS)
@pytest.mark.parametrize("N", list(TABLE_SIZES))
def test_window_tables(N, kind):
    fs, ms = TABLE_SIZES[N]
    for coeff in ((0.42, 0.3) if kind == "blackman" else (0.42,)):
        p = host(F64, sample_frequency=fs, frame_length=ms, window_type=kind, blackman_coeff=coeff, num_mel_bins=5, high_freq=0.0)
        assert p.window_size == N
        got, ref = p.window(), KR.window(kind, N, coeff)
        assert got.shape == ref.shape and rel_close(got, ref), np.max(np.abs(got - ref))


@pytest.mark.parametrize("high", [0.0, -400.0, 7600.0])
@pytest.mark.parametrize("bins", [23, 40, 80])
@pytest.mark.parametrize("N", [400, 1200])
def test_bank_dct_and_lifter_tables(N, bins, high):
    fs, ms = TABLE_SIZES[N]
    for rnd in (True, False):
        p = host(F64, sample_frequency=fs, frame_length=ms, num_mel_bins=bins, high_freq=high, num_ceps=min(13, bins),
                 round_to_power_of_two=rnd, cepstral_lifter=22.0)
        P = p.padded_window_size
        assert P == (1 << (N - 1).bit_length() if rnd else N)
        got, ref = p.mel_banks(), KR.mel_banks(bins, P, fs, 20.0, high)
        assert got.shape == ref.shape == (bins, P // 2 + 1) and rel_close(got, ref)
        assert np.array_equal(got > 0, ref > 0)
        assert rel_close(p.dct(), KR.dct(min(13, bins), bins)) and rel_close(p.lifter(), KR.lifter(min(13, bins), 22.0))
    assert np.array_equal(host(F64, num_ceps=5, cepstral_lifter=0.0).lifter(), np.ones(5))
    small = host(F64, sample_frequency=8000.0, num_mel_bins=bins if bins < 40 else 23, high_freq=min(high, 3600.0))
    assert rel_close(small.mel_banks(), KR.mel_banks(small.params.num_mel_bins, 256, 8000.0, 20.0, min(high, 3600.0)))


def test_dct_is_orthonormal_and_small_tables():
    D = host(F64, num_mel_bins=23, num_ceps=23).dct()
    assert np.max(np.abs(D @ D.T - np.eye(23))) < 1e-14
    p = host(F64, sample_frequency=1000.0, num_mel_bins=5, num_ceps=5)
    assert (p.window_size, p.window_shift, p.padded_window_size) == (25, 10, 32)
    assert rel_close(p.mel_banks(), KR.mel_banks(5, 32, 1000.0, 20.0, 0.0)) and rel_close(p.dct(), KR.dct(5, 5))


def test_bank_structure():
    p = host(F64, num_mel_bins=80)
    bank = p.mel_banks()
    assert p.padded_window_size == 512 and bank.shape == (80, 257)
    assert np.all(bank[:, -1] == 0) and np.all(bank >= 0) and np.all(bank <= 1)
    assert np.all(np.count_nonzero(bank, axis=1) >= 1)
    for row in bank:  # a triangle: one run of positive weights
        nz = np.flatnonzero(row)
        assert np.array_equal(nz, np.arange(nz[0], nz[-1] + 1))


@pytest.mark.parametrize("snip", [True, False])
def test_n_frames(snip):
    for ms_len, ms_shift in ((25.0, 10.0), (25.0625, 10.0625), (25.0, 10.0625), (25.0625, 10.0)):
        p = host(frame_length=ms_len, frame_shift=ms_shift, snip_edges=snip)
        N, shift = p.window_size, p.window_shift
        assert (N, shift) == (400 + (ms_len != 25.0), 160 + (ms_shift != 10.0)) == KR.sizes(p.params)[:2]
        for n in (N, N + shift - 1, N + shift, N + 7 * shift + 3, 5000):
            want = 1 + (n - N) // shift if snip else (n + shift // 2) // shift
            assert p.n_frames(n) == want == KR.n_frames(n, N, shift, snip) == KR.frame_indices(n, N, shift, snip).shape[0]
        assert p.n_frames(N - 1) == 0 and p.n_frames(0) == 0
    assert host(snip_edges=True).n_frames(400) == 1 and host(snip_edges=False).n_frames(400) == 3


def test_n_out():
    assert host(num_mel_bins=80).n_out == 80 and host(num_mel_bins=80, use_energy=True).n_out == 81
    assert host(num_mel_bins=23, num_ceps=13).n_out == 13 and host(num_mel_bins=23, num_ceps=13, use_energy=True).n_out == 13


# ---- CPU: the restatement itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,dc", [(0.97, True), (0.0, True), (0.5, False)])
def test_restatement_against_the_explicit_matrix_product(alpha, dc):
    """One frame as F_P pad diag(w) (I - alpha S) (I - 1 1^T / N), S the shift matrix whose first row repeats the first sample."""
    N, P = 25, 32
    kp = KP(sample_frequency=1000.0, num_mel_bins=5, preemphasis_coefficient=alpha, remove_dc_offset=dc, use_log_fbank=False)
    assert KR.sizes(kp) == (N, 10, P)
    x = np.random.default_rng(5).standard_normal(N) + 2.0
    w = KR.window("povey", N)
    S = np.zeros((N, N))
    S[0, 0] = 1.0
    S[np.arange(1, N), np.arange(N - 1)] = 1.0
    M = np.eye(N) - alpha * S
    if dc:
        M = M @ (np.eye(N) - np.ones((N, N)) / N)
    pad = np.zeros((P, N))
    pad[:N, :N] = np.eye(N)
    k, j = np.arange(P // 2 + 1)[:, None], np.arange(P)[None, :]
    F = np.exp(-2j * np.pi * k * j / P)
    X = F @ pad @ np.diag(w) @ M @ x
    E = (np.abs(X) ** 2) @ KR.mel_banks(5, P, 1000.0, 20.0, 0.0).T
    ref, _, _ = KR.reference(x[None], kp, F64)
    assert ref.shape == (1, 1, 5) and np.allclose(ref[0, 0], E, rtol=1e-12, atol=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_analytic_cases_of_the_restatement(dtype):
    eps = float(np.finfo(KR.NP[dtype]).eps)
    ref, _, _ = KR.reference(np.full((1, 2000), 0.5), KP(num_mel_bins=80), dtype)
    assert ref.shape == (1, 11, 80) and np.all(ref == math.log(eps))
    # an impulse every frame length, frames one frame length apart: every frame holds the same samples
    kp = KP(num_mel_bins=40, frame_shift=25.0)
    x = np.zeros((1, 400 * 6))
    x[0, 7::400] = 1.0
    ref, _, _ = KR.reference(x, kp, dtype)
    assert ref.shape == (1, 6, 40) and np.all(ref == ref[:, :1]) and np.all(np.isfinite(ref)) and np.ptp(ref[0, 0]) > 0


def test_torchaudio_agrees_with_the_restatement():
    torchaudio = pytest.importorskip("torchaudio")
    import torch
    x = (0.3 + 0.1 * np.random.default_rng(1).standard_normal((1, 4000))).astype(np.float32)
    for kw in (dict(num_mel_bins=80), dict(num_mel_bins=23, use_energy=True, snip_edges=False)):
        ref, _, _ = KR.reference(x, KP(**kw), F32)
        got = torchaudio.compliance.kaldi.fbank(torch.from_numpy(x), dither=0.0, **kw).numpy()
        assert np.allclose(got, ref[0], rtol=1e-3, atol=1e-3)
    ref, _, _ = KR.reference(x, KP(num_ceps=13), F32)
    got = torchaudio.compliance.kaldi.mfcc(torch.from_numpy(x), dither=0.0).numpy()
    assert np.allclose(got, ref[0], rtol=1e-3, atol=1e-3)


# ---- CPU: rejections and routes -------------------------------------------------------------------------------------------------------------
REFUSED = [
    (dict(dither=1.0), "dither"), (dict(vtln_warp=1.1), "vtln_warp"), (dict(spectrogram=True), "spectrogram"),
    (dict(min_duration=0.5), "min_duration"), (dict(streaming=True), "streaming"),
    (dict(sample_frequency=1000.0, frame_length=1.5), "frame_length"),            # N = 1
    (dict(frame_shift=0.05), "frame_shift"),                                      # shift = 0
    (dict(sample_frequency=96000.0, frame_length=11000.0), "frame_length"),       # P = 2^21
    (dict(low_freq=-1.0), "low_freq"), (dict(low_freq=8000.0), "low_freq"),
    (dict(high_freq=8001.0), "high_freq"), (dict(high_freq=-8000.0), "high_freq"),
    (dict(low_freq=4000.0, high_freq=4000.0), "low_freq"), (dict(low_freq=4000.0, high_freq=-5000.0), "low_freq"),
    (dict(preemphasis_coefficient=-0.1), "preemphasis_coefficient"), (dict(preemphasis_coefficient=1.01), "preemphasis_coefficient"),
    (dict(num_mel_bins=23, num_ceps=24), "num_ceps"), (dict(num_mel_bins=3), "num_mel_bins"),
]


@pytest.mark.parametrize("kw,field", REFUSED, ids=[f"{f}-{i}" for i, (_, f) in enumerate(REFUSED)])
def test_rejections(kw, field):
    with pytest.raises(sg.InvalidInputError, match=field):
        host(**kw)
    # ... and through the raw ABI: the status and the text of the failed create
    L = _ffi.lib()
    good = host()
    assert good.kernel_name == "k_kaldi"
    p = _ffi.SgxKaldiParams()
    p.sample_frequency, p.frame_length_ms, p.frame_shift_ms, p.vtln_warp, p.num_mel_bins, p.device = 16000.0, 25.0, 10.0, 1.0, 23, HOST
    p.low_freq, p.round_to_power_of_two, p.dither = 20.0, 1, 0.5
    h = C.c_void_p()
    assert L.sgx_kaldi_create(C.byref(p), 0, 0, C.byref(h)) == _ffi.SGX_INVALID_INPUT and not h.value
    assert b"dither" in L.sgx_kaldi_last_error(None)


def test_limits_that_pass_and_python_side_checks():
    assert host(preemphasis_coefficient=1.0).n_out == 23 and host(preemphasis_coefficient=0.0).n_out == 23
    assert host(high_freq=8000.0, low_freq=0.0).n_out == 23 and host(num_mel_bins=4, num_ceps=4).n_out == 4
    assert host(sample_frequency=1000.0, frame_length=2.0, num_mel_bins=4, round_to_power_of_two=False, low_freq=0.0).window_size == 2
    with pytest.raises(sg.InvalidInputError, match="window_type"):
        KP(window_type="hann")
    with pytest.raises(sg.InvalidInputError, match="route"):
        sg.KaldiPlan(KP(), route="fused", device=HOST)
    with pytest.raises(TypeError):
        sg.KaldiPlan(dict())


def test_short_rows_and_host_only_plans():
    p = host()
    for x in (np.zeros(399, np.float32), np.zeros((2, 10), np.float32)):
        with pytest.raises(sg.DimensionMismatchError, match="expected 400"):
            p.compute(x)
    with pytest.raises(sg.DimensionMismatchError):
        p.reserve(1, 399)
    with pytest.raises(sg.FFTBackendError, match="no HIP device"):
        p.compute(np.zeros((2, 4000), np.float32))
    with pytest.raises(sg.FFTBackendError, match="no HIP device"):
        p.reserve(2, 4000)
    assert p.device == -2 and p.allocations == 0
    L = _ffi.lib()
    x, out = np.zeros((1, 4000), np.float32), np.zeros(10, np.float32)
    assert L.sgx_kaldi_execute(p._h, x.ctypes.data, 1, 4000, 4000, out.ctypes.data, 10, _ffi.MEM_HOST, None) == _ffi.SGX_DIM_MISMATCH


# the compiled instances of k_kaldi: P -> the (fs, frame_length ms) that reaches it; num_mel_bins that leaves no band empty there
INSTANCES = {256: (8000.0, 25.0, 23), 512: (16000.0, 25.0, 80), 1024: (32000.0, 25.0, 80), 2048: (48000.0, 25.0, 80)}


@pytest.mark.parametrize("dtype", DTYPES)
def test_routes(dtype):
    for P, (fs, ms, bins) in INSTANCES.items():
        p = host(dtype, sample_frequency=fs, frame_length=ms, num_mel_bins=bins)
        assert (p.kernel_name, p.padded_window_size, p.tile) == ("k_kaldi", P, TILE)
        g = host(dtype, "generic", sample_frequency=fs, frame_length=ms, num_mel_bins=bins)
        assert (g.kernel_name, g.padded_window_size, g.tile) == ("kaldi_generic", P, 0)
    assert host(dtype, sample_frequency=22050.0).padded_window_size == 1024 and host(dtype, sample_frequency=44100.0).kernel_name == "k_kaldi"
    for kw, P in ((dict(round_to_power_of_two=False), 400), (dict(sample_frequency=1000.0, num_mel_bins=5), 32),
                  (dict(sample_frequency=96000.0), 4096), (dict(frame_length=5.0), 128)):
        p = host(dtype, **kw)
        assert (p.kernel_name, p.padded_window_size, p.tile) == ("kaldi_generic", P, 0)
    assert host(dtype, frame_length=16.0, round_to_power_of_two=False).kernel_name == "k_kaldi"  # N = P = 256
    assert host(dtype, num_mel_bins=257, low_freq=0.0).kernel_name == "kaldi_generic"              # more bands than a round keeps in LDS


def parsed_instances(text=None):
    text = text or open(os.path.join(CSRC, "kaldi.hip")).read()
    return {(dt, s) for dt, tag in ((F32, "F32"), (F64, "F64")) for s in FR._xmacro(text, "SGX_KALDI_SPLITS_" + tag)}


def test_the_named_cases_are_the_compiled_instances():
    named = {(dt, FR.reg_split_len(P, dt)) for P in INSTANCES for dt in DTYPES}
    assert len(named) == 8 and parsed_instances() == named
    text = open(os.path.join(CSRC, "kaldi.hip")).read()
    old = "#define SGX_KALDI_SPLITS_F32(X) X(16, 16, 1)"
    assert text.count(old) == 1
    assert parsed_instances(text.replace(old, "#define SGX_KALDI_SPLITS_F32(X) X(16, 16, 16) X(16, 16, 1)")) - named == {(F32, (16, 16, 16))}
    assert named - parsed_instances(text.replace(old, "#define SGX_KALDI_SPLITS_F32(X)")) == {(F32, (16, 16, 1))}


# ---- the GPU cases: (keywords, rows, n, seed, level step) -> (x, ref, bound), the range condition asserted on the reference alone ----------
BASE = {"fbank": dict(num_mel_bins=80), "mfcc": dict(num_mel_bins=23, num_ceps=13)}


def noise_rows(rows, n, dtype, seed, step_at=None):
    x = 0.3 + 0.1 * np.random.default_rng(seed).standard_normal((rows, n))
    if step_at is not None:
        x[:, :step_at] *= 1e6  # a 10^6 : 1 level step: loud before step_at, quiet from it on
    return x.astype(KR.NP[dtype])


@functools.lru_cache(maxsize=None)
def _case(kw_items, dtype, rows, n, seed, step_at):
    x = noise_rows(rows, n, dtype, seed, step_at)
    ref, bound, worst = KR.reference(x, KP(**dict(kw_items)), dtype)
    assert worst <= 0.1, f"input outside the bound's range: r = {worst}"
    for a in (x, ref, bound):
        a.setflags(write=False)
    return x, ref, bound


def case(kw, dtype, rows, n, seed=0, step_at=None):
    return _case(tuple(sorted(kw.items())), dtype, rows, n, seed, step_at)


def seam_lengths(N, shift):
    """(m, n, level step) per seam row: m = 1, tile - 1, tile, tile + 1, 2 tile + 1; the step at the first sample the second tile
    reads; a ragged tail of shift - 1 unused samples."""
    out = []
    for m in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        n = N + (m - 1) * shift + shift - 1
        out.append((m, n, None))
        if m > TILE:
            out.append((m, n, TILE * shift))
    return out


SWITCHES = [dict(remove_dc_offset=False), dict(preemphasis_coefficient=0.0), dict(use_energy=True), dict(use_energy=True, raw_energy=False),
            dict(use_energy=True, htk_compat=True), dict(htk_compat=True), dict(subtract_mean=True), dict(use_energy=True, subtract_mean=True),
            dict(use_energy=True, energy_floor=0.0), dict(use_energy=True, energy_floor=1.0), dict(use_energy=True, energy_floor=100.0),
            dict(remove_dc_offset=False, preemphasis_coefficient=0.0, use_energy=True)]
SWITCHES += [dict(window_type=w) for w in KR.WINDOWS]
FBANK_ONLY = [dict(use_power=False), dict(use_log_fbank=False), dict(use_power=False, use_log_fbank=False, use_energy=True)]
SWITCH_CASES = [("fbank", s) for s in SWITCHES + FBANK_ONLY] + [("mfcc", s) for s in SWITCHES + [dict(cepstral_lifter=0.0)]]
SWITCH_N = 400 + 40 * 160 + 11  # 41 frames: two tiles

ALIGN = [dict(num_mel_bins=80, frame_shift=10.0625), dict(num_mel_bins=80, frame_length=25.0625),
         dict(num_mel_bins=80, frame_length=25.0625, frame_shift=10.0625, snip_edges=False)]
EDGES = [(dict(num_mel_bins=80, snip_edges=False), n) for n in (400, 401, 5000, 400 + 40 * 160 + 7)]
# shift 5: 40 frames read each mirrored end, more than a tile's.  40 bands: over 200 frames the one-bin bands of an 80-band bank meet an
# |X_k|^2 small enough to leave the bound's range (r = 1.7 on the reference alone, f32), whatever the kernel does
EDGES.append((dict(num_mel_bins=40, snip_edges=False, frame_shift=0.32), 1000))
GENERIC = [("P400", dict(num_mel_bins=80, round_to_power_of_two=False), 400, 4000), ("P400-edges", dict(num_mel_bins=80, round_to_power_of_two=False, snip_edges=False), 400, 4000),
           ("P32", dict(sample_frequency=1000.0, num_mel_bins=5), 32, 400), ("P32-mfcc", dict(sample_frequency=1000.0, num_mel_bins=5, num_ceps=4, use_energy=True, snip_edges=False), 32, 400),
           ("P4096", dict(sample_frequency=96000.0, num_mel_bins=80), 4096, 2400 + 12 * 960 + 5),
           ("P4096-mfcc", dict(sample_frequency=96000.0, num_mel_bins=40, num_ceps=13, subtract_mean=True), 4096, 2400 + 12 * 960 + 5)]


def all_gpu_cases():
    """(keywords, dtype, rows, n, seed, step) of every reference a GPU case uses."""
    for dtype in DTYPES:
        for P, (fs, ms, bins) in INSTANCES.items():
            N, shift, _ = KR.sizes(KP(sample_frequency=fs, frame_length=ms))
            yield dict(sample_frequency=fs, frame_length=ms, num_mel_bins=bins), dtype, 3, N + (TILE + 2) * shift + 3, P, None
            yield dict(sample_frequency=fs, frame_length=ms, num_mel_bins=23, num_ceps=13, use_energy=True), dtype, 2, N + (TILE + 2) * shift + 3, P + 1, None
        for m, n, step in seam_lengths(400, 160):
            yield BASE["fbank"], dtype, 2, n, 100 + m, step
        for kw in ALIGN:
            yield kw, dtype, 3, 7000, 7, None
        for kw, n in EDGES:
            yield kw, dtype, 2, n, 9, None
        for kind, sw in SWITCH_CASES:
            yield {**BASE[kind], **sw}, dtype, 2, SWITCH_N, 11, None
        for _, kw, _, n in GENERIC:
            yield kw, dtype, 2, n, 13, None
        yield BASE["fbank"], dtype, 3, 400 + 19 * 160, 15, None  # the chunked generic case


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_gpu_case_is_inside_the_bound_s_range(dtype):
    """r <= 0.1 at every element of every reference (asserted in _case), before any GPU is touched; the shapes are the plan's."""
    count = 0
    for kw, dt, rows, n, seed, step in all_gpu_cases():
        if dt != dtype:
            continue
        x, ref, bound = case(kw, dt, rows, n, seed, step)
        p = host(dt, **kw)
        assert ref.shape == bound.shape == (rows, p.n_frames(n), p.n_out) and np.all(np.isfinite(bound)) and np.all(bound > 0)
        count += 1
    assert count == 68
    assert SWITCH_N > 400 + TILE * 160 and host(dtype, **ALIGN[0]).window_shift == 161 and host(dtype, **ALIGN[1]).window_size == 401
    assert host(dtype, **EDGES[-1][0]).window_shift == 5


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------
def _run(plan, x):
    import torch
    out = plan.compute_torch(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(plan, kw, dtype, rows, n, seed=0, step=None, label=""):
    x, ref, bound = case(kw, dtype, rows, n, seed, step)
    got = _run(plan, x.copy())
    assert got.shape == ref.shape and got.dtype == KR.NP[dtype]
    r = KR.ratio(got, ref, bound)
    print(f"kaldi {plan.kernel_name} P={plan.padded_window_size} {dtype} {label} n={n}: ratio {r:.3g}")
    record(plan.kernel_name, plan.padded_window_size, dtype, r)
    assert r <= 1.0, (label, dtype, n, r)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", list(INSTANCES))
def test_gpu_every_compiled_instance(P, dtype):
    fs, ms, bins = INSTANCES[P]
    N, shift, _ = KR.sizes(KP(sample_frequency=fs, frame_length=ms))
    n = N + (TILE + 2) * shift + 3
    for kw, rows, seed in ((dict(sample_frequency=fs, frame_length=ms, num_mel_bins=bins), 3, P),
                           (dict(sample_frequency=fs, frame_length=ms, num_mel_bins=23, num_ceps=13, use_energy=True), 2, P + 1)):
        plan = sg.KaldiPlan(KP(**kw), dtype)
        assert (plan.kernel_name, plan.padded_window_size, plan.tile) == ("k_kaldi", P, TILE)
        check(plan, kw, dtype, rows, n, seed, label="instance")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_tile_seams(dtype):
    plan = sg.KaldiPlan(KP(**BASE["fbank"]), dtype)
    assert (plan.kernel_name, plan.tile, plan.window_size, plan.window_shift) == ("k_kaldi", TILE, 400, 160)
    for m, n, step in seam_lengths(400, 160):
        assert plan.n_frames(n) == m and plan.n_frames(n + 1) == m + 1
        if step is not None:
            x, _, _ = case(BASE["fbank"], dtype, 2, n, 100 + m, step)
            assert np.abs(x[0, :step]).max() > 1e5 * np.abs(x[0, step:]).max()
        check(plan, BASE["fbank"], dtype, 2, n, 100 + m, step, label=f"seam m={m} step={step}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_alignment(dtype):
    import torch
    for kw in ALIGN:
        plan = sg.KaldiPlan(KP(**kw), dtype)
        assert plan.kernel_name == "k_kaldi" and (plan.window_size % 2 == 1 or plan.window_shift % 2 == 1)
        got = check(plan, kw, dtype, 3, 7000, 7, label="odd")
        # the same rows as a slice of a resident tensor: a row stride larger than n
        x, _, _ = case(kw, dtype, 3, 7000, 7, None)
        X = torch.zeros((3, 7000 + 211), dtype=plan._tdt, device="cuda")
        X[:, 101:7101] = torch.from_numpy(x.copy()).cuda()
        out = plan.compute_torch(X[:, 101:7101])
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), got)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_without_snip_edges(dtype):
    for kw, n in EDGES:
        plan = sg.KaldiPlan(KP(**kw), dtype)
        assert plan.kernel_name == "k_kaldi"
        check(plan, kw, dtype, 2, n, 9, label=f"edges shift={plan.window_shift}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,sw", SWITCH_CASES, ids=[f"{k}-" + "-".join(f"{a}={b}" for a, b in s.items()) for k, s in SWITCH_CASES])
def test_gpu_switches(kind, sw, dtype):
    kw = {**BASE[kind], **sw}
    plan = sg.KaldiPlan(KP(**kw), dtype)
    assert plan.kernel_name == "k_kaldi"
    check(plan, kw, dtype, 2, SWITCH_N, 11, label=f"{kind} {sw}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,kw,P,n", GENERIC, ids=[g[0] for g in GENERIC])
def test_gpu_generic_route(name, kw, P, n, dtype):
    plan = sg.KaldiPlan(KP(**kw), dtype)
    assert (plan.kernel_name, plan.padded_window_size) == ("kaldi_generic", P)
    check(plan, kw, dtype, 2, n, 13, label=name)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_generic_chunks_do_not_change_the_bits(dtype):
    kw, n = BASE["fbank"], 400 + 19 * 160
    whole = sg.KaldiPlan(KP(**kw), dtype, route="generic")
    per_frame = 514 * (8 if dtype == F64 else 4)  # max(P, 2 (P / 2 + 1)) elements per frame and buffer
    split = sg.KaldiPlan(KP(**kw), dtype, route="generic", max_scratch_bytes=25 * per_frame)  # 60 frames: chunks of 25, 25, 10
    assert whole.kernel_name == split.kernel_name == "kaldi_generic" and whole.n_frames(n) == 20
    a = check(whole, kw, dtype, 3, n, 15, label="unchunked")
    b = check(split, kw, dtype, 3, n, 15, label="3 chunks")
    assert np.array_equal(a, b)
    for extra in (dict(num_ceps=13, num_mel_bins=23, use_energy=True, subtract_mean=True),):
        x = noise_rows(3, n, dtype, 16)
        pa = sg.KaldiPlan(KP(**extra), dtype, route="generic")
        pb = sg.KaldiPlan(KP(**extra), dtype, route="generic", max_scratch_bytes=7 * per_frame)
        assert np.array_equal(_run(pa, x), _run(pb, x))


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["auto", "generic"])
@pytest.mark.parametrize("snip", [True, False])
def test_gpu_frame_isolation(snip, route):
    """One NaN sample makes non-finite exactly the frames that contain it, by the index arithmetic of the frames."""
    n = 400 + 50 * 160 + 9
    for at in (3, 3000, n - 2):
        x = noise_rows(1, n, F32, 21)
        x[0, at] = np.nan
        plan = sg.KaldiPlan(KP(num_mel_bins=80, snip_edges=snip, use_energy=True), F32, route=route)
        got = _run(plan, x)[0]
        holds = np.any(KR.frame_indices(n, 400, 160, snip) == at, axis=1)
        # (with snip_edges the last 9 samples are a ragged tail that no frame reads: no frame may change)
        assert got.shape == (holds.size, 81) and holds.sum() <= 4 and holds.any() == (not snip or at < n - 9)
        assert np.array_equal(np.all(~np.isfinite(got), axis=1), holds) and np.array_equal(np.all(np.isfinite(got), axis=1), ~holds)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["auto", "generic"])
def test_gpu_batch_independence_and_reserve(route, dtype):
    kw = dict(num_mel_bins=40, num_ceps=13, use_energy=True, subtract_mean=True)
    n = 400 + 70 * 160
    x = noise_rows(5, n, dtype, 31)
    plan = sg.KaldiPlan(KP(**kw), dtype, route=route)
    plan.reserve(5, n)
    before = plan.allocations
    five = plan.compute(x)
    again = plan.compute(x)
    alone = plan.compute(x[:1])
    last = plan.compute(x[4:])
    assert plan.allocations == before
    assert np.array_equal(five, again) and np.array_equal(five[:1], alone) and np.array_equal(five[4:], last)
    assert np.array_equal(_run(plan, x), five)
    ref, bound, worst = KR.reference(x, KP(**kw), dtype)
    assert worst <= 0.1 and KR.ratio(five, ref, bound) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["auto", "generic"])
def test_gpu_constant_row_is_the_log_of_epsilon(route):
    want = np.float32(math.log(2.0 ** -23))
    got = sg.KaldiPlan(KP(num_mel_bins=80), F32, route=route).compute(np.full((2, 4000), 0.5, np.float32))
    assert got.shape == (2, 23, 80) and np.max(np.abs(got - want)) <= np.spacing(np.abs(want))
    assert sg.kaldi_fbank(np.full(4000, 0.5, np.float32), num_mel_bins=80).shape == (23, 80)
    assert sg.kaldi_mfcc(noise_rows(2, 4000, F64, 1)).shape == (2, 23, 13)


@pytest.mark.gpu
def test_gpu_impulse_train_gives_the_same_features_in_every_frame():
    x = np.zeros((1, 400 * 6), np.float32)
    x[0, 7::400] = 1.0
    got = sg.KaldiPlan(KP(num_mel_bins=40, frame_shift=25.0), F32).compute(x)
    assert got.shape == (1, 6, 40) and np.all(got == got[:, :1]) and np.all(np.isfinite(got))


@pytest.mark.gpu
def test_gpu_worst_ratios_per_route():
    """Prints what the cases above recorded (run the module as a whole): worst ratio to the bound per (route, P, dtype)."""
    print()
    for (route, P, dtype), r in sorted(WORST.items()):
        print(f"| {route} | {P} | {dtype} | {r:.3g} |")
    assert all(r <= 1.0 for r in WORST.values())
