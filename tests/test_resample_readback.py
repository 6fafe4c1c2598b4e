"""k_resample_pp and resample_generic read back tap by tap, and the f32 fma chain.

1. Impulse read-back, `==` on every element.  A row is +0.0 except M impulses at n_i = n_0 + i D, D the smallest integer >= K coprime
   to M, amplitudes (-1)^i 2^((i mod 7) - 3).  No output window holds two impulses (D >= K), the positions run through every residue
   mod M, so every (p, k) of the table is hit, and a window that holds impulse i at tap k must give exactly s_i T(c[p][k]) (a power of
   two times a T value, then exact zeros added), every other output exact zero.  The expectation is built from the positions alone.
2. f32 against its chain on random input.  Each output is acc = 0, acc = fma(c[p][k], x[..], acc), k ascending; the host evaluates
   acc <- float32(longdouble(acc) + longdouble(c) longdouble(x)), the model tests/test_cqt_readback.py pins against
   fractions.Fraction (the 48-bit product is exact in long double, the sum is rounded to 64 bits before the rounding to 24, which
   differs from the single rounding only within 2^-40 ulp of a tie).  Condition, as in that file: at most 1 output in 10^4 may differ,
   none by more than 4 spacings of the largest |sample| in its window.

Table, K and j0 come from the plan's accessors (tests/test_resample.py pins them to the formula).
"""
import math

import numpy as np
import pytest

import spectrograms_amd as sg
from tests import test_resample as TR

F32, F64 = TR.F32, TR.F64
LD = np.longdouble


def impulse_rows(geo, dtype):
    """(x, expected): 3 rows whose impulse trains start at n_0, n_0 + 1, n_0 + 2."""
    M, L, K, j0, tab, _ = geo
    D = K
    while math.gcd(D, M) != 1:
        D += 1
    n0 = K + max(0, -int(j0.min()), int(j0.max()))  # every window that reaches an impulse starts at q >= 0 ..
    n = n0 + 2 + (M - 1) * D + max(0, -int(j0.min())) + M + K  # .. and belongs to an output of the row
    n_out = -(-n * L // M)
    m = np.arange(n_out)
    start = (m // L) * M + j0[m % L]  # rises with m
    x = np.zeros((3, n), TR.NP[dtype])
    exp = np.zeros((3, n_out), TR.NP[dtype])
    hits = np.zeros((L, K), bool)
    for r in range(3):
        taken = np.zeros(n_out, bool)
        for i in range(M):
            at, s = n0 + r + i * D, (-1.0) ** i * 2.0 ** ((i % 7) - 3)
            x[r, at] = s
            lo, hi = np.searchsorted(start, at - K + 1, "left"), np.searchsorted(start, at, "right")
            mm = m[lo:hi]
            assert not taken[mm].any()
            taken[mm] = True
            k = at - start[mm]
            hits[mm % L, k] = True
            exp[r, mm] = (s * tab[mm % L, k]).astype(TR.NP[dtype])  # exact: a power of two times a T value
    assert hits.all(), "an entry of the table is not reached"
    return x, exp


@pytest.mark.parametrize("ratio", TR.RATIOS, ids=lambda r: f"{r[0]}to{r[1]}")
def test_impulse_rows_reach_every_tap(ratio):
    """(No GPU.)  The rows of the read-back hit every (p, k) once per row, within 16 000 samples."""
    for dtype in (F32, F64):
        x, exp = impulse_rows(TR.geometry(*ratio, dtype), dtype)
        assert x.shape[1] <= 16000 and np.count_nonzero(x) == 3 * TR.reduced(*ratio)[0]
        assert np.count_nonzero(exp) <= 3 * np.count_nonzero(TR.geometry(*ratio, dtype)[4])


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,dtype,route", TR.CASES, ids=TR.CASE_IDS)
def test_gpu_impulse_read_back(ratio, dtype, route):
    geo = TR.geometry(*ratio, dtype)
    x, exp = impulse_rows(geo, dtype)
    y = TR.gpu_plan(ratio, dtype, route).resample(x)
    assert y.shape == exp.shape
    bad = np.argwhere(y != exp)
    assert bad.size == 0, (len(bad), bad[:5], y[tuple(bad[0])], exp[tuple(bad[0])])


def chain_f32(x, geo):
    """The f32 chain of every output of a 1-D row on the host, and the largest |sample| of its window."""
    M, L, K, j0, tab, _ = geo
    X, ph = TR.windows(x, M, L, K, j0)
    C = tab[ph].astype(np.float32)
    acc = np.zeros(X.shape[0], np.float32)
    for k in range(K):
        acc = (acc.astype(LD) + C[:, k].astype(LD) * X[:, k].astype(LD)).astype(np.float32)
    return acc, np.max(np.abs(X), axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,route", [(r, route) for r, dt, route in TR.CASES if dt == F32],
                         ids=[i for (r, dt, route), i in zip(TR.CASES, TR.CASE_IDS) if dt == F32])
def test_gpu_f32_matches_its_chain(ratio, route):
    """At most 1 output in 10^4 off the chain, none by more than 4 spacings of the largest |sample| in its window.
    Measured on the MI355X (the test prints each case's count): 0 outputs off the chain in all 15 cases — of 11 523 (3 -> 1), 18 387
    (1 -> 3), 17 286 (2 -> 1), 18 438 (3 -> 2), 18 369 (7 -> 5), 11 526 (44.1 -> 16 kHz), 11 532 (44.1 -> 48 kHz) on both routes and of
    4 611 (8 -> 1, generic only)."""
    geo = TR.geometry(*ratio, F32)
    M, L, _, _, _, tile = geo
    n = -(-3 * tile * M // (2 * L)) + 3
    x = TR.noise(n, F32, 51)
    y = TR.gpu_plan(ratio, F32, route).resample(x)
    off = total = 0
    worst = 0.0
    for r in range(3):
        ref, big = chain_f32(x[r], geo)
        d = np.abs(y[r].astype(np.float64) - ref.astype(np.float64))
        off += int(np.count_nonzero(d))
        total += d.size
        worst = max(worst, float(np.max(d / np.spacing(np.maximum(big, np.float32(1e-30))).astype(np.float64))))
    print(f"resample chain {ratio} {route}: {off} of {total} outputs off the chain, worst {worst:.3g} spacings")
    assert off <= 1e-4 * total and worst <= 4.0, (off, total, worst)
