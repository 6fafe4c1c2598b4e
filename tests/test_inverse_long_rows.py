"""sgx_c2r / sgx_istft at the two lengths whose forward frames run in LDS (the radix-2 kernel in half-length complex form) while no
on-chip tile holds a full-length inverse row: f32 n_fft 32768 and f64 n_fft 16384.  Their inverse rows go through the global-memory
transforms (route "big" / "big+ola"), as a big_four_step plan's do; before, both entry points returned an error there.

Reference: np.fft.irfft in f64 of the T-valued spectrum; frames times the window, overlap-added and divided by the summed squared
window as src/spectrogram.rs:4906-4930 does.  Bounds, u_T = 2^-24 / 2^-53, c = 4 (tests/test_mdct.py's constant): a transform's
error is at most c u log2(n) relative in the 2-norm, and the 2-norm bounds the max, so
  one row            max_t |dy[t]| <= c u log2(n) ||y||_2
  overlap-added      |dy[t]| <= (sum_f |w[t - f hop]| c u log2(n) ||y_f||_2) / norm[t]  +  4 u |y[t]|
(the second term: the window product, the sums and the division, one rounding each).
"""
import math

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi

F32, F64 = "float32", "float64"
NP = {F32: np.float32, F64: np.float64}
CNP = {F32: np.complex64, F64: np.complex128}
U = {F32: 2.0 ** -24, F64: 2.0 ** -53}
CB = 4.0
CASES = [(F32, 32768), (F64, 16384)]
IDS = [f"{d}-{n}" for d, n in CASES]


def make_plan(dtype, n, hop, centre, window, device=_ffi.DEVICE_CURRENT):
    params = sg.SpectrogramParams(sg.StftParams(n, hop, getattr(sg.WindowType, window), centre), 16000.0)
    return sg.Plan(params, _ffi.AMP_COMPLEX, None, None, dtype, device=device)


def rand_spec(rng, shape, dtype):
    """A T-valued half spectrum [..., nb, nf] with real DC and Nyquist rows."""
    s = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(CNP[dtype])
    s[..., 0, :] = s[..., 0, :].real
    s[..., -1, :] = s[..., -1, :].real
    return s


@pytest.mark.parametrize("dtype,n", CASES, ids=IDS)
def test_forward_kind_is_the_lds_kernel(dtype, n):
    assert make_plan(dtype, n, n // 4, True, "hanning", device=_ffi.DEVICE_HOST_ONLY).kernel_name == "lds_radix2"
    assert make_plan(dtype, 2 * n, n // 2, True, "hanning", device=_ffi.DEVICE_HOST_ONLY).kernel_name == "big_four_step"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n", CASES, ids=IDS)
def test_gpu_c2r_single_row(dtype, n):
    rng = np.random.default_rng(n)
    X = rand_spec(rng, (n // 2 + 1, 1), dtype)[:, 0]
    ref = np.fft.irfft(X.astype(np.complex128), n)
    plan = make_plan(dtype, n, n, False, "rectangular")
    for _ in range(2):  # the one-sequence scratch of plan creation, call after call
        got = plan.c2r(X)
        assert got.shape == (n,) and got.dtype == NP[dtype]
        ratio = np.max(np.abs(got.astype(np.float64) - ref)) / (CB * U[dtype] * math.log2(n) * np.linalg.norm(ref))
        print(f"c2r {dtype} {n}: ratio to bound {ratio:.3g}")
        assert ratio <= 1.0
    assert np.array_equal(sg.compute_irfft(X, n, dtype=dtype), got)
    assert plan.istft_kernel_name == "big"


def ref_istft(S, w, n, hop, centre):
    """(y, bound / (c u log2 n)) per batch row, f64."""
    b, _, nf = S.shape
    full = (nf - 1) * hop + n
    y, e, norm = np.zeros((b, full)), np.zeros((b, full)), np.zeros(full)
    for f in range(nf):
        fr = np.fft.irfft(S[:, :, f].astype(np.complex128), n, axis=-1)
        y[:, f * hop:f * hop + n] += fr * w
        e[:, f * hop:f * hop + n] += np.abs(w) * np.linalg.norm(fr, axis=-1, keepdims=True)
        norm[f * hop:f * hop + n] += w * w
    ok = norm > 1e-10
    y[:, ok] /= norm[ok]
    e[:, ok] /= norm[ok]
    pad = n // 2 if centre else 0
    return y[:, pad:full - pad], e[:, pad:full - pad]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n", CASES, ids=IDS)
def test_gpu_istft_several_frames_host_device_and_reserved_capture(dtype, n):
    import torch
    hop, nf, batch = n // 4, 7, 3
    plan = make_plan(dtype, n, hop, True, "hanning")
    rng = np.random.default_rng(n + 1)
    specs = [rand_spec(rng, (batch, n // 2 + 1, nf), dtype) for _ in range(2)]
    w = np.asarray(plan.window(), np.float64)
    host = plan.istft_batch(specs[0])
    assert plan.istft_kernel_name == "big+ola"
    y, e = ref_istft(specs[0], w, n, hop, True)
    assert host.shape == y.shape
    bound = CB * U[dtype] * math.log2(n) * e + 4.0 * U[dtype] * np.abs(y)
    ratio = np.max(np.abs(host.astype(np.float64) - y) / bound)
    print(f"istft {dtype} {n}: worst ratio to bound {ratio:.3g}")
    assert ratio <= 1.0
    # a signal's round trip through the forward LDS kernel and this inverse
    x = rng.standard_normal((batch, 5 * n)).astype(NP[dtype])
    back = plan.istft_batch(plan.compute_batch(x))
    assert back.shape[1] <= x.shape[1] and np.max(np.abs(back - x[:, :back.shape[1]])) < 64 * U[dtype] * math.log2(n) * np.abs(x).max()
    # device tensors: the same bits; after reserve(inverse=True) the call allocates nothing and is captured and replayed
    fresh = make_plan(dtype, n, hop, True, "hanning")
    fresh.reserve(batch, y.shape[1], host_staging=False, inverse=True)
    devs = [torch.from_numpy(s).cuda() for s in specs]
    eager = [plan.istft_batch(d) for d in devs]
    torch.cuda.synchronize()
    assert np.array_equal(eager[0].cpu().numpy(), host)
    sin, out = devs[0].clone(), torch.full_like(eager[0], -1.0e30)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fresh.istft_batch(sin, out=out)
    for k in (1, 0):
        sin.copy_(devs[k])
        out.fill_(-1.0e30)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[k]), f"replay on input {k} differs from the eager result"
