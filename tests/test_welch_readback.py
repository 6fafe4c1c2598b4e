"""The fused Welch kernel read back through signals whose spectra are known in closed form, per bin, for every fused length and both types.

impulse  rectangular window, no detrend, scaling="spectrum", one segment: a unit impulse at offset j has |X[k]| = 1 at every bin, so
         Pxx[k] = g_k / n^2.  At j = 0 and j = n / 2 every transform value is +-1 with no rounding anywhere, |X|^2 is exactly 1 and the
         result is one rounding of the scale product away from g_k / n^2 (none: n is a power of two).  At j = 1 and j = n - 1 the bins
         are W^(+-k), products of rounded table twiddles, so |X|^2 = 1 only to a few u_T; those offsets are held to the PSD bound of
         tests/test_welch.py, which there is (8 log2(n) + 4) u_T relative — still far below what a wrong g_k, scale or bin order costs.
cosine   rectangular window, no detrend, m segments at hop = n: cos(2 pi k0 t / n) puts g (n / 2)^2 scale on bin k0 and nothing
         elsewhere; both are held to the bound.
"""
import numpy as np
import pytest

import spectrograms_amd as sg
from tests.test_welch import FUSED, NP, U, one_sided, ratio, reference

pytestmark = pytest.mark.gpu


def _compute(plan, x):
    import torch
    out = plan.compute_torch(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n", FUSED)
def test_impulse_reads_back_the_scale_at_every_bin(n, dtype):
    plan = sg.WelchPlan(sg.WelchParams(n, n, sg.WindowType.rectangular, 16000.0, None, "spectrum"), "psd", dtype)
    assert plan.kernel_name == "k_welch"
    want = one_sided(n) / float(n) ** 2
    offsets = (0, 1, n // 2, n - 1)
    x = np.zeros((len(offsets), n), NP[dtype])
    for r, j in enumerate(offsets):
        x[r, j] = 1.0
    got = _compute(plan, x).astype(np.float64)
    ref, bound = reference("psd", x, None, np.ones(n), n, n, None, "spectrum", 16000.0, dtype)
    assert np.max(np.abs(ref - want)) <= 1e-12 * want.max()  # (the restatement's own rfft error: the level of its pin to scipy)
    rel = np.abs(got - want) / want
    print(f"welch impulse n={n} {dtype}: worst relative error per offset {dict(zip(offsets, rel.max(axis=1)))} (u_T = {U[dtype]:.2e})")
    for r, j in enumerate(offsets):
        if j in (0, n // 2):
            assert np.all(np.abs(got[r] - want) <= U[dtype] * want), j
        assert ratio(got[r], want, bound[r]) <= 1.0, j


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n", FUSED)
def test_cosine_lands_on_its_bin(n, dtype):
    fs, m = 16000.0, 3
    plan = sg.WelchPlan(sg.WelchParams(n, n, sg.WindowType.rectangular, fs, None, "density"), "psd", dtype)
    bins = (1, n // 4, n // 2 - 1)
    t = np.arange(m * n + 5)
    # the phase reduced in integers first: cos(2 pi k0 t / n) with a large argument is off by t u, which in f64 is above the bound
    two_pi = 8 * np.arctan(np.longdouble(1))
    x = np.stack([np.cos(two_pi * ((k0 * t) % n).astype(np.longdouble) / n) for k0 in bins]).astype(NP[dtype])
    got = _compute(plan, x).astype(np.float64)
    _, bound = reference("psd", x, None, np.ones(n), n, n, None, "density", fs, dtype)
    worst = 0.0
    for r, k0 in enumerate(bins):
        want = np.zeros(n // 2 + 1)
        want[k0] = 2.0 * (n / 2.0) ** 2 * plan.scale
        assert got[r, k0] > 0.5 * want[k0]
        rr = ratio(got[r], want, bound[r])
        worst = max(worst, rr)
        assert rr <= 1.0, (k0, rr)
    print(f"welch cosine n={n} {dtype}: worst ratio {worst}")
