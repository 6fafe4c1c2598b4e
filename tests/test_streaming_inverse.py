"""Streaming inverse STFT plans (sgx_istream_*, StreamingInversePlan): the bookkeeping and the errors on host-only streams, and on the
GPU the carry, indexing, order, normalisation and trim bit for bit on DC-only spectra, every sample of every call against the per-sample
f64 bound of tests/test_istft_precision.py, the analysis -> synthesis chain on device tensors, the state across reserve / reset / flush,
and stream order.

The GPU cases use 3 rows and 23 frames unless stated.  A cut is a list of frame counts per push; `cut_of` is the issue's
[1, 1, 2, K - 1, K, 3 K + 1, rest] with K = ceil(n_fft / hop): entries of 0 frames are left out and the list ends where the frames do
(at 23 frames the 3 K + 1 entry is clipped from K = 4 on).

Exact test: X[0] = n_fft c with integer c = ((5 f + 3 r) mod 13) - 6 per frame f and row r, every other bin zero, power-of-two n_fft:
every twiddle that meets a non-zero value is W^0 and 1 / n_fft is exact, so each inverse row is the constant c.  `restate` is the
stream's arithmetic in NumPy in T: products T(c) w_j rounded once, added in ascending frame order from T(0), the rounded w w summed the
same way, the division where the sum exceeds T(1e-10), the centre trim and the one-frame quirk.

Bounded test: the bound of tests/test_istft_precision.py (its docstring) with its helpers, the f64 reference over all frames of the
signal; on the routes that pair frames 2 p / 2 p + 1 in one complex transform rho is the joint norm over the frames of each call, since
the rows' launcher pairs within a call.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import spectrograms_amd as sg
import tests.test_istft_precision as IP
from spectrograms_amd import _ffi
from tests.test_streaming import rows3

HOST = _ffi.DEVICE_HOST_ONLY
SR = 16000.0
NP = {"float32": np.float32, "float64": np.float64}
CNP = {"float32": np.complex64, "float64": np.complex128}
ROWS, NF = 3, 23


def params_of(n_fft, hop, centre, window="hanning"):
    return sg.SpectrogramParams(sg.StftParams(n_fft, hop, getattr(sg.WindowType, window), centre), SR)


def make_pair(dtype, n_fft, hop, centre, window, device=_ffi.DEVICE_CURRENT):
    plan = sg.Plan(params_of(n_fft, hop, centre, window), _ffi.AMP_COMPLEX, None, None, dtype, device=device)
    return plan, plan.istream()


def cut_of(n_fft, hop, nf):
    k = -(-n_fft // hop)
    cut, left = [], nf
    for f in [1, 1, 2, k - 1, k, 3 * k + 1]:
        f = min(f, left)
        if f > 0:
            cut.append(f)
            left -= f
    return cut + ([left] if left else [])


def hi(n_fft, hop, pad, F):
    return max(pad, min(F * hop, (F - 1) * hop + n_fft - pad)) if F else pad


def run_cut(stream, S, cut, sync=None):
    """Push S[:, :, a:b] per entry of the cut, flush; the per-call outputs (each call's length checked against the semantics)."""
    n_fft, hop, pad = stream._n_fft, stream._hop, stream._pad
    at, outs = 0, []
    for f in cut:
        want = hi(n_fft, hop, pad, at + f) - hi(n_fft, hop, pad, at)
        assert stream.samples(f) == want and stream.frames_taken == at
        blk = S[:, :, at:at + f]
        outs.append(stream.push(blk if hasattr(blk, "data_ptr") else np.ascontiguousarray(blk)))
        assert tuple(outs[-1].shape) == (S.shape[0], want)
        at += f
        assert stream.pending <= n_fft and stream.pending == (at - 1) * hop + n_fft - (0 if at == 1 and pad and n_fft % 2 == 0 else hi(n_fft, hop, pad, at))
        if sync:
            sync()
    outs.append(stream.flush())
    assert stream.frames_taken == 0 and stream.samples_emitted == 0 and stream.pending == 0
    return outs


def istream_of(plan, n_fft, hop, centre):
    s = plan.istream()
    s._n_fft, s._hop, s._pad = n_fft, hop, (n_fft // 2 if centre else 0)  # (for run_cut's own bookkeeping)
    return s


def cat(outs):
    return np.concatenate([np.asarray(o.cpu().numpy() if hasattr(o, "cpu") else o) for o in outs], axis=1)


# ---------------------------------------------------------------------------------------------------------------- CPU
ISTREAM_SYMBOLS = ["sgx_istream_create", "sgx_istream_destroy", "sgx_istream_step", "sgx_istream_frames_taken", "sgx_istream_samples_emitted",
                   "sgx_istream_pending", "sgx_istream_flush_samples", "sgx_istream_push", "sgx_istream_flush", "sgx_istream_reset",
                   "sgx_istream_reserve", "sgx_istream_allocations", "sgx_istream_kernel_name", "sgx_istream_device", "sgx_istream_last_error"]


def test_symbols_are_exported_and_listed():
    L = _ffi.lib()
    for name in ISTREAM_SYMBOLS:
        assert hasattr(L, name), name
        assert name in _ffi.SYMBOLS, name
    assert "StreamingInversePlan" in sg.__all__ and sg.StreamingInversePlan is not None
    assert L.sgx_abi_version() == 7
    plan, stream = make_pair("float32", 64, 16, True, "hanning", HOST)
    assert isinstance(stream, sg.StreamingInversePlan) and stream.kernel_name == "" and stream.device == HOST and stream.dtype == "float32"
    with pytest.raises(ValueError, match="complex STFT plan"):
        sg.Plan(params_of(64, 16, True), _ffi.AMP_POWER, device=HOST).istream()


def test_bookkeeping_matches_istft_length_for_any_cut():
    """2000 seeded cases: sgx_istream_step iterated over a random cut of F frames, plus the flush count (n_frames = 0), gives
    Plan.istft_length(F); each step is hi(F + f) - hi(F); the carry after every step is at most n_fft samples.  The first cases are
    the corners: centre / even n_fft / one frame (the untrimmed frame), its odd neighbour, and hop > n_fft / 2."""
    L = _ffi.lib()
    rng = np.random.default_rng(20240611)
    corners = [(64, 16, True, 1), (64, 64, True, 1), (2, 1, True, 1), (63, 16, True, 1), (64, 40, True, 5), (64, 64, True, 7), (65, 50, True, 3),
               (64, 33, False, 4), (8, 3, True, 23), (700, 700, True, 40)]
    seen = {"quirk": 0, "wide": 0}
    for case in range(2000):
        if case < len(corners):
            n_fft, hop, centre, F = corners[case]
        else:
            n_fft = int(rng.integers(2, 701))
            hop = int(rng.integers(1, n_fft + 1))
            centre = bool(rng.integers(0, 2))
            F = int(rng.integers(1, 41))
        k = int(rng.integers(1, F + 1))
        at = np.sort(rng.choice(np.arange(1, F), k - 1, replace=False)) if k > 1 else np.array([], np.int64)
        cut = np.diff(np.concatenate([[0], at, [F]]))
        assert cut.sum() == F and cut.min() >= 1
        plan = sg.Plan(params_of(n_fft, hop, centre), _ffi.AMP_COMPLEX, device=HOST)
        st = plan.istream()
        pad = n_fft // 2 if centre else 0
        assert (st.frames_taken, st.samples_emitted, st.pending, st.flush_samples()) == (0, 0, 0, 0)
        taken, total, m = 0, 0, C.c_size_t()
        for f in cut:
            assert L.sgx_istream_step(st._h, taken, int(f), C.byref(m)) == _ffi.SGX_OK
            assert m.value == hi(n_fft, hop, pad, taken + int(f)) - hi(n_fft, hop, pad, taken)
            taken, total = taken + int(f), total + m.value
            whole = centre and n_fft % 2 == 0 and taken == 1
            carried = (taken - 1) * hop + n_fft - (0 if whole else hi(n_fft, hop, pad, taken))
            assert 0 <= carried <= n_fft
        assert L.sgx_istream_step(st._h, taken, 0, C.byref(m)) == _ffi.SGX_OK
        assert total + m.value == plan.istft_length(F), (case, n_fft, hop, centre, F, list(cut))
        if centre and n_fft % 2 == 0 and F == 1:
            seen["quirk"] += 1
            assert total == 0 and m.value == n_fft
        if centre and 2 * hop > n_fft and F > 1:
            seen["wide"] += 1
    assert seen["quirk"] >= 3 and seen["wide"] >= 100


def test_errors_on_host_only_streams():
    L = _ffi.lib()
    p = _ffi.SgxParams(n_fft=64, hop_size=16, window_kind=_ffi.WIN_HANNING, sample_rate_hz=SR, dtype=_ffi.F32, device=HOST,
                       freq_scale=_ffi.FREQ_CQT)
    h = C.c_void_p()
    assert L.sgx_istream_create(C.byref(p), C.byref(h)) == _ffi.SGX_INVALID_INPUT and not h.value
    assert L.sgx_istream_last_error(None).decode() == "Invalid input: an inverse stream inverts STFT frames (a CQT plan has no FFT)"
    p = _ffi.SgxParams(n_fft=64, hop_size=65, window_kind=_ffi.WIN_HANNING, sample_rate_hz=SR, dtype=_ffi.F32, device=HOST)
    assert L.sgx_istream_create(C.byref(p), C.byref(h)) == _ffi.SGX_INVALID_INPUT and not h.value  # every check of the offline plan
    assert L.sgx_istream_last_error(None).decode() == "Invalid input: hop_size must be <= n_fft"
    st = sg.StreamingInversePlan(params_of(400, 160, True), dtype="float32", device=HOST)
    assert (st.frames_taken, st.samples_emitted, st.pending, st.n_bins, st.device) == (0, 0, 0, 201, HOST)
    assert (st.samples(1), st.samples(2), st.samples(3), st.flush_samples()) == (0, 120, 280, 0)
    with pytest.raises(sg.InvalidInputError, match="stft matrix must be non-empty"):
        st.push(np.zeros((3, 201, 0), np.complex64))
    x = np.zeros((3, 201, 2), np.complex64)
    out = np.zeros((3, 120), np.float32)
    assert L.sgx_istream_push(st._h, x.ctypes.data, 3, 200, 2, 2, out.ctypes.data, 360, _ffi.MEM_HOST, None) == _ffi.SGX_DIM_MISMATCH
    assert L.sgx_istream_last_error(st._h).decode() == "Dimension mismatch: expected 201, got 200"
    assert L.sgx_istream_push(st._h, x.ctypes.data, 3, 201, 2, 2, out.ctypes.data, 5, _ffi.MEM_HOST, None) == _ffi.SGX_DIM_MISMATCH
    assert L.sgx_istream_last_error(st._h).decode() == "Dimension mismatch: expected 360, got 5"
    assert L.sgx_istream_push(st._h, x.ctypes.data, 3, 201, 2, 2, None, 360, _ffi.MEM_HOST, None) == _ffi.SGX_INVALID_INPUT
    assert L.sgx_istream_last_error(st._h).decode() == "Invalid input: null buffer"
    assert L.sgx_istream_push(st._h, x.ctypes.data, 3, 201, 1, 1, out.ctypes.data, 360, _ffi.MEM_HOST, None) == _ffi.SGX_DIM_MISMATCH
    assert L.sgx_istream_last_error(st._h).decode() == "Dimension mismatch: expected 0, got 360"  # m = 0: out_elems must be 0
    assert L.sgx_istream_push(st._h, x.ctypes.data, 3, 201, 2, 1, out.ctypes.data, 360, _ffi.MEM_HOST, None) == _ffi.SGX_INVALID_INPUT
    assert L.sgx_istream_last_error(st._h).decode() == "Invalid input: bin_stride < n_frames"
    assert L.sgx_istream_push(st._h, None, 3, 201, 2, 2, out.ctypes.data, 360, _ffi.MEM_HOST, None) == _ffi.SGX_INVALID_INPUT
    assert L.sgx_istream_last_error(st._h).decode() == "Invalid input: null buffer"
    with pytest.raises(sg.FFTBackendError) as e:
        st.push(x)
    assert str(e.value) == "hip -- FFT backend error: plan has no HIP device (host-only plan)"
    with pytest.raises(sg.FFTBackendError, match="host-only plan"):
        st.reserve(3, 8)
    with pytest.raises(ValueError, match=r"2-D \(n_bins, f\) or 3-D"):
        st.push(np.zeros(201, np.complex64))
    assert (st.frames_taken, st.samples_emitted, st.pending, st.kernel_name) == (0, 0, 0, "")  # a failed call moves nothing
    # a flush of a stream that has taken no frame emits nothing
    for centre in (True, False):
        fresh = sg.StreamingInversePlan(params_of(400, 160, centre), dtype="float32", device=HOST)
        assert fresh.flush_samples() == 0 and fresh.flush().shape == (0,) and fresh.frames_taken == 0
        assert L.sgx_istream_flush(fresh._h, out.ctypes.data, 360, _ffi.MEM_HOST, None) == _ffi.SGX_DIM_MISMATCH
        assert L.sgx_istream_last_error(fresh._h).decode() == "Dimension mismatch: expected 0, got 360"


# ---------------------------------------------------------------------------------------------------------------- GPU, exact
# (n_fft, hop, centre, window, premise: the output is the rows themselves)
EXACT = [(64, 64, False, "rectangular", True), (512, 512, False, "rectangular", True), (1024, 1024, False, "rectangular", True),
         (64, 16, True, "hanning", False), (64, 16, False, "rectangular", False), (64, 24, True, "hanning", False),
         (64, 40, True, "hanning", False), (64, 64, True, "hanning", False), (8, 3, True, "hanning", False),
         (512, 160, False, "hamming", False), (1024, 256, True, "hanning", False)]


def dc_levels(nf):
    return ((5 * np.arange(nf)[None, :] + 3 * np.arange(ROWS)[:, None]) % 13) - 6  # [row, frame]


def dc_spectra(n_fft, nf, dtype):
    S = np.zeros((ROWS, n_fft // 2 + 1, nf), CNP[dtype])
    S[:, 0, :] = n_fft * dc_levels(nf)
    return S


def restate(c, w, n_fft, hop, centre, T):
    """The stream's arithmetic on rows that are the constants c[row, frame], in T; trimmed like istft."""
    rows, nf = c.shape
    full = (nf - 1) * hop + n_fft
    A, W = np.zeros((rows, full), T), np.zeros(full, T)
    ww = w * w
    assert ww.dtype == T
    for f in range(nf):
        A[:, f * hop:f * hop + n_fft] += c[:, f].astype(T)[:, None] * w[None, :]
        W[f * hop:f * hop + n_fft] += ww
    assert A.dtype == T and W.dtype == T
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.where(W[None, :] > T(1e-10), A / W[None, :], A)
    pad = n_fft // 2 if centre else 0
    return y if full <= 2 * pad else y[:, pad:full - pad]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", EXACT, ids=lambda s: f"{s[0]}-{s[1]}-{'c' if s[2] else 'n'}-{s[3][:4]}")
def test_dc_only_spectra_bit_for_bit(shape, dtype):
    n_fft, hop, centre, window, premise = shape
    T = NP[dtype]
    plan = sg.Plan(params_of(n_fft, hop, centre, window), _ffi.AMP_COMPLEX, None, None, dtype)
    w = np.asarray(plan.window(), np.float64).astype(T)
    stream = istream_of(plan, n_fft, hop, centre)
    for nf in (NF, 1):
        S, c = dc_spectra(n_fft, nf, dtype), dc_levels(nf)
        ref = np.ascontiguousarray(restate(c, w, n_fft, hop, centre, T))
        assert ref.shape == (ROWS, plan.istft_length(nf))
        if premise:  # rectangular window, hop = n_fft: the output is the rows themselves
            assert np.array_equal(ref, np.repeat(c, n_fft, axis=1).astype(T))
        for cut in (cut_of(n_fft, hop, nf), [1] * nf, [nf]):
            got = cat(run_cut(stream, S, cut))
            assert got.dtype == T and got.shape == ref.shape, (nf, cut, got.shape, ref.shape)
            bad = np.flatnonzero((got.view(np.uint32 if T is np.float32 else np.uint64) != ref.view(np.uint32 if T is np.float32 else np.uint64)).ravel())
            assert bad.size == 0, (nf, cut, stream.kernel_name, bad[:4], got.ravel()[bad[:4]], ref.ravel()[bad[:4]])
    assert stream.kernel_name.endswith("+stream_ola")


# ---------------------------------------------------------------------------------------------------------------- GPU, bounded
# (dtype, n_fft, hop, centre, window, the rows' route, frames 2p / 2p + 1 of a call share a transform, frames, cut or None)
BOUNDED = [("float32", 1024, 256, True, "hanning", "c2r_reg", False, NF, None),
           ("float32", 2048, 512, False, "hamming", "c2r_reg", False, NF, None),
           ("float32", 400, 160, True, "blackman", "c2r_reg", False, NF, None),
           ("float32", 251, 62, True, "hanning", "c2r_chirpz", True, NF, None),
           ("float32", 15, 4, False, "hamming", "c2r_rows", False, NF, None),
           ("float32", 13, 13, False, "hanning", "c2r_rows", False, NF, None),
           ("float32", 9001, 2250, True, "hanning", "big", True, 7, [1, 2, 4]),
           ("float64", 512, 160, False, "blackman", "c2r_reg", False, NF, None),
           ("float64", 400, 160, True, "blackman", "c2r_reg", False, NF, None),
           ("float64", 1009, 252, False, "hamming", "c2r_chirpz", True, NF, None)]


def stream_reference(S, cut, n_fft, hop, centre, w, dtype, name, paired):
    """f64 reference + bound of one signal's stream output, all calls end to end (trimmed like istft); rho pairs within a call."""
    r = IP.frames_f64(S, n_fft)
    at = np.cumsum([0] + list(cut))
    rho = np.concatenate([IP.frame_norms(r[a:b], paired) for a, b in zip(at[:-1], at[1:])])
    ref = IP.ola_reference(r, rho, w, hop, dtype, IP.c_of(name, n_fft), IP.g_of(name, n_fft))
    full, pad = ref[0].size, (n_fft // 2 if centre else 0)
    return ref if full <= 2 * pad else tuple(a[pad:full - pad] for a in ref)


def check_bound(got, S, cut, n_fft, hop, centre, w, dtype, name, paired, tag):
    worst = 0.0
    for i in range(S.shape[0]):
        ref = stream_reference(S[i], cut, n_fft, hop, centre, w, dtype, name, paired)
        assert got[i].shape == ref[0].shape, (tag, got[i].shape, ref[0].shape)
        r = IP.ratio(got[i], ref)
        k = int(np.argmax(r))
        worst = max(worst, float(r[k]))
        print(f"{tag}: row {i} worst ratio to bound {float(r[k]):.3g} at sample {k}")
        assert r[k] <= 1.0, f"{tag}: row {i} sample {k}: |dy| {abs(float(got[i][k]) - ref[0][k]):.3g} bound {ref[1][k]:.3g}"
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", BOUNDED, ids=lambda c: f"{c[5]}-{c[0][5:]}-{c[1]}-{c[2]}{'c' if c[3] else ''}-{c[4][:4]}")
def test_every_sample_of_every_call_within_the_f64_bound(case):
    dtype, n_fft, hop, centre, window, name, paired, nf, cut = case
    plan = sg.Plan(params_of(n_fft, hop, centre, window), _ffi.AMP_COMPLEX, None, None, dtype)
    stream = istream_of(plan, n_fft, hop, centre)
    cut = cut or cut_of(n_fft, hop, nf)
    assert sum(cut) == nf
    rng = np.random.default_rng(n_fft)
    e = 4.0 if dtype == "float32" else 8.0
    S = np.stack([IP.rand_spec(rng, n_fft // 2 + 1, nf, n_fft, 10.0 ** (-e * (np.arange(nf) % 3))) for _ in range(ROWS)]).astype(CNP[dtype])
    outs = run_cut(stream, S, cut)  # (every call's length is checked there)
    assert stream.kernel_name == name + "+stream_ola"
    got = cat(outs)
    assert got.shape == (ROWS, plan.istft_length(nf))
    check_bound(got, S, cut, n_fft, hop, centre, IP.plan_window(plan, dtype), dtype, stream.kernel_name.replace("+stream_ola", ""), paired,
                f"{dtype} {name} {n_fft}/{hop}")


# ---------------------------------------------------------------------------------------------------------------- GPU, chain
@pytest.mark.gpu
def test_analysis_to_synthesis_chain_on_device_tensors():
    torch = pytest.importorskip("torch")
    n_fft, hop, centre, dtype, n = 1024, 256, True, "float32", 5003
    plan = sg.Plan(params_of(n_fft, hop, centre), _ffi.AMP_COMPLEX, None, None, dtype)
    fwd, inv = plan.stream(), istream_of(plan, n_fft, hop, centre)
    x = torch.from_numpy(rows3(n, dtype)).cuda()
    blocks = [1, 7, 255, 1, 1023, 256, 773]
    blocks.append(n - sum(blocks))
    at = np.cumsum([0] + blocks)
    spectra, outs, skipped = [], [], 0
    for S in [fwd.push(x[:, a:b]) for a, b in zip(at[:-1], at[1:])] + [fwd.flush()]:
        if S.shape[2] == 0:
            skipped += 1
            continue
        assert S.is_cuda and S.dtype == torch.complex64
        m = inv.samples(S.shape[2])
        outs.append(inv.push(S))
        assert outs[-1].is_cuda and tuple(outs[-1].shape) == (3, m)
        spectra.append(S)
    outs.append(inv.flush())
    assert skipped >= 2 and inv.kernel_name == "c2r_reg+stream_ola"
    Sall = torch.cat(spectra, dim=2).cpu().numpy()
    got = cat(outs)
    assert Sall.shape[2] == plan.output_shape(n)[1] and got.shape == (3, plan.istft_length(Sall.shape[2]))
    check_bound(got, Sall, [s.shape[2] for s in spectra], n_fft, hop, centre, IP.plan_window(plan, dtype), dtype, "c2r_reg", False, "chain")


# ---------------------------------------------------------------------------------------------------------------- GPU, state
@functools.lru_cache(maxsize=None)
def state_spectra(dtype, n_fft, nf=NF, seed=5):
    rng = np.random.default_rng(seed)
    S = np.stack([IP.rand_spec(rng, n_fft // 2 + 1, nf, n_fft, np.ones(nf)) for _ in range(ROWS)]).astype(CNP[dtype])
    S.setflags(write=False)
    return S


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_state_reserve_reset_flush_rows_out_and_slices(dtype):
    torch = pytest.importorskip("torch")
    n_fft, hop, centre = 512, 160, True
    plan = sg.Plan(params_of(n_fft, hop, centre), _ffi.AMP_COMPLEX, None, None, dtype)
    S = state_spectra(dtype, n_fft)
    cut = [1, 3, 8, 2, 8, 1]
    assert sum(cut) == NF
    # reserve: pushes within it, and the flush, allocate nothing; one past it does
    stream = istream_of(plan, n_fft, hop, centre)
    assert stream.allocations == 0
    stream.reserve(3, 8)
    count = stream.allocations
    assert count >= 3
    first = run_cut(stream, S, cut)
    assert stream.allocations == count
    stream.push(np.ascontiguousarray(S[:, :, :9]))
    assert stream.allocations > count
    with pytest.raises(sg.InvalidInputError, match=r"reserve\(\) needs a stream without carried samples"):
        stream.reserve(3, 16)
    # reset drops the carry and frees the row count
    stream.reset()
    assert (stream.frames_taken, stream.samples_emitted, stream.pending) == (0, 0, 0)
    two = stream.push(np.ascontiguousarray(S[:2, :, :4]))  # (what a fresh stream gives: nothing of the nine frames is left)
    assert two.shape == (2, stream_len(n_fft, hop, 4)) and np.array_equal(two, plan.istream().push(np.ascontiguousarray(S[:2, :, :4])))
    # a wrong row count; a failed call moves nothing
    with pytest.raises(sg.DimensionMismatchError, match="expected 2, got 3"):
        stream.push(np.ascontiguousarray(S[:, :, 4:6]))
    assert stream.frames_taken == 4
    # a push after a flush starts a new signal, with the same row count; the second signal equals a first run of the same frames
    stream.flush()
    with pytest.raises(sg.DimensionMismatchError, match="expected 2, got 3"):
        stream.push(np.ascontiguousarray(S[:, :, :1]))
    stream.reset()
    second = run_cut(stream, S, cut)
    assert len(second) == len(first) and all(np.array_equal(a, b) for a, b in zip(first, second))
    again = run_cut(stream, S, cut)  # behind a flush, no reset
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    assert sum(o.shape[1] for o in again) == plan.istft_length(NF)
    # out= is honoured (NumPy and torch), and a 2-D push comes back without the batch axis
    stream = istream_of(plan, n_fft, hop, centre)
    assert stream.push(np.ascontiguousarray(S[:, :, :1])).shape == (3, 0)
    buf = np.full((3, stream.samples(3)), np.nan, NP[dtype])
    assert buf.size and stream.push(np.ascontiguousarray(S[:, :, 1:4]), out=buf) is buf and np.array_equal(buf, first[1])
    with pytest.raises(sg.DimensionMismatchError):
        stream.push(np.ascontiguousarray(S[:, :, 4:12]), out=np.zeros((3, 5), NP[dtype]))
    assert stream.frames_taken == 4
    Sd = torch.from_numpy(np.array(S)).cuda()
    tb = torch.full((3, stream.samples(8)), float("nan"), dtype=torch.float32 if dtype == "float32" else torch.float64, device="cuda")
    assert stream.push(Sd[:, :, 4:12], out=tb) is tb
    assert np.array_equal(tb.cpu().numpy(), first[2])
    one = plan.istream()
    assert one.push(np.ascontiguousarray(S[1, :, :4])).shape == (stream_len(n_fft, hop, 4),) and one.flush().ndim == 1
    # a strided slice of a resident (3, n_bins, 23) tensor gives the bits of its contiguous copy
    a, b = istream_of(plan, n_fft, hop, centre), istream_of(plan, n_fft, hop, centre)
    sliced = run_cut(a, Sd, cut)
    at = np.cumsum([0] + cut)
    copies = [b.push(Sd[:, :, lo:hi_].contiguous()) for lo, hi_ in zip(at[:-1], at[1:])] + [b.flush()]
    assert all(np.array_equal(p.cpu().numpy(), q.cpu().numpy()) for p, q in zip(sliced, copies))
    assert all(np.array_equal(p.cpu().numpy(), q) for p, q in zip(sliced, first))  # and the host path's
    with pytest.raises(ValueError, match="unit inner stride"):
        a.push(Sd.transpose(1, 2)[:, :257, :4])
    # a flush of a stream that has taken no frame emits nothing and launches nothing
    fresh = plan.istream()
    assert fresh.flush_samples() == 0 and fresh.flush().shape == (0,) and fresh.allocations == 0


def stream_len(n_fft, hop, f, pad=None):
    pad = n_fft // 2 if pad is None else pad
    return hi(n_fft, hop, pad, f) - pad


# ---------------------------------------------------------------------------------------------------------------- GPU, stream order
@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype", [((1024, 256, True), "float32"), ((400, 160, False), "float64"), ((251, 62, True), "float32")])
def test_stream_order_on_a_side_stream(shape, dtype):
    """The pushes of one cut and the flush back to back on a side stream, inputs as views into one tensor, one synchronise at the end:
    every output equals, bit for bit, the same cut on the default stream with a synchronise after each call."""
    torch = pytest.importorskip("torch")
    n_fft, hop, centre = shape
    plan = sg.Plan(params_of(n_fft, hop, centre), _ffi.AMP_COMPLEX, None, None, dtype)
    S = state_spectra(dtype, n_fft)
    Sd = torch.from_numpy(np.array(S)).cuda()
    cut = cut_of(n_fft, hop, NF)
    ref = run_cut(istream_of(plan, n_fft, hop, centre), Sd, cut, sync=torch.cuda.synchronize)
    torch.cuda.synchronize()
    stream = istream_of(plan, n_fft, hop, centre)
    stream.reserve(3, max(cut), host_staging=False)
    count = stream.allocations
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        outs = run_cut(stream, Sd, cut)
    side.synchronize()
    assert stream.allocations == count and len(outs) == len(ref)
    for i, (d, h) in enumerate(zip(outs, ref)):
        assert tuple(d.shape) == tuple(h.shape), (i, tuple(d.shape), tuple(h.shape))
        assert np.array_equal(d.cpu().numpy(), h.cpu().numpy()), i
