"""k_cqt tap by tap (cqt.hip, cqt_device_tables of plan.hip): what tests/test_cqt.py and tests/test_cqt_transform.py cannot see in f32.

Their bound e = (L_g + 2) u sum_j |w_j x_j| grows with the group length; in f32 at 2048 taps a table that is off by 1e-3 everywhere,
one tap that reads its neighbour's sample and a lost edge tap all stay below it (test_calibration_* restates the three in NumPy and
asserts exactly that).  Two exact checks close the hole.

1. Impulse read-back, f32 and f64, `==` on every element.  The signal is +0.0 but for impulses p_i = n_fft + i D, i < hop, D the
   smallest integer >= n_fft coprime to hop, amplitude s_i = (-1)^i 2^((i mod 7) - 3): no frame holds two of them, and over the call
   every tap offset 0 .. n_fft - 1 is hit exactly once (p_i mod hop takes every residue).  A frame whose tap t holds impulse i must
   give, for bin k of own length L_k, re = s_i T(Re K_k[j]) and im = s_i T(-Im K_k[j]) with j = t - (n_fft - L_k), 0 where j < 0 and 0
   in every frame without an impulse: fma(x, w, 0) plus exact zeros, on the matrix cores and on the sequential recompute path alike.
   K is the plan's own table (plan.cqt_kernels()); the expectation is built from the impulse positions alone (`expected`).
2. f32 against its fma chain, random input.  v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain, so every output is pinned to that chain
   evaluated on the host: acc <- float32(longdouble(acc) + longdouble(x_t) longdouble(w_t)), taps ascending.  The 48-bit product is
   exact in x86's 64-bit long double mantissa and the sum is rounded once at 64 bits before the cast, which differs from fmaf only
   within 2^-40 ulp of a tie (test_long_double_chain_is_the_exact_chain pins it against fractions.Fraction).  A zero weight leaves
   the accumulator as it is, so walking every tap from the first one any bin weighs is the walk over each group's L_g block rows.
   Condition, as tests/test_mfcc.py: at most 1 output in 10^4 may differ, none by more than 4 spacings of its bin's largest |value|.

Geometry, n_fft (klen) 2048, CqtParams(12, 7, 32.7), 16 kHz: lpad 2048, 84 bins, 25 of them capped at 2048 taps, L_83 = 68.  TABLE
gives the tile multiple per hop and type (0: the global-memory route); hops that are a multiple of 8 take the LDS bank skew.

Measured on an MI355X: every f32 output of part 2 is bit-equal to the host chain (0 of 11 760 per part at hops 64, 512 and 4096, 0 of
2 772 on the rows route, 0 of 11 760 powers; largest difference 0 ulp).  The read-back found two faults in f64, both fixed in
cqt.hip: at hop 441 (M = 1, no skew) frame rows 12 .. 15 came back with the high word of every value zero (the accumulator was read
before the last v_mfma_f64_16x16x4_f64 of a step had written it: mfma_drain), and the f64 power was fma(re, re, im im) instead of two
products and a sum (mul_rn / add_rn were contracted).  test_gpu_f64_bound_without_skew keeps the first one covered on random input."""
import math
from fractions import Fraction

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests.test_cqt import cqt_plan, ref_cqt, signals
from tests.test_cqt_transform import Kept, gplan, lds_bytes, lds_m, run_complex, tplan

HOST = _ffi.DEVICE_HOST_ONLY
NP = {"float32": np.float32, "float64": np.float64}
DTYPES = ["float32", "float64"]
DEFAULT = sg.CqtParams(12, 7, 32.7)
SR = 16000.0
KLEN = 2048
LD = np.longdouble
# hop: (f32 M, f64 M), 0 = global; lpad 2048.  1 and 100 and 441: no skew; M = 1 with more than 64 KiB of dynamic LDS: 441 and 512 and 768
# (f64), 1024 (both) and 2048 (f32).  320 and 768 are there for M = 1 within 64 KiB: f64 needs 263 < hop < 410 for it, f32 594 < hop < 956.
TABLE = {1: (4, 4), 64: (4, 4), 100: (4, 4), 256: (4, 2), 320: (2, 1), 441: (2, 1), 512: (2, 1), 768: (1, 1), 1024: (1, 1), 2048: (1, 0), 4096: (0, 0)}


# ---- geometry and the two host models -----------------------------------------------------------------------------------------
def amp_of(i):
    i = np.asarray(i, np.int64)
    return np.where(i % 2 == 0, 1.0, -1.0) * 2.0 ** ((i % 7) - 3)


def train(n_fft, hop):
    """Impulse positions p_i = n_fft + i D and amplitudes s_i, i < hop."""
    d = n_fft
    while math.gcd(d, hop) != 1:
        d += 1
    i = np.arange(hop, dtype=np.int64)
    return n_fft + i * d, amp_of(i)


def n_frames(n, n_fft, hop, pad):
    return 1 if n + 2 * pad < n_fft else (n + 2 * pad - n_fft) // hop + 1


def hits(pos, n, n_fft, hop, pad=0):
    """(impulse index, frame, tap) of every frame tap that holds one of the impulses at samples `pos` of a signal of n samples."""
    nf = n_frames(n, n_fft, hop, pad)
    q = np.asarray(pos, np.int64) + pad
    out = []
    for r in range(-(-n_fft // hop)):
        f = q // hop - r
        t = q - f * hop
        ok = (f >= 0) & (f < nf) & (t < n_fft)
        out.append(np.stack([np.nonzero(ok)[0], f[ok], t[ok]]))
    return np.concatenate(out, axis=1)


def weights(plan, T, n_fft):
    """The plan's own kernels as the device table holds them: [bins][n_fft], T(Re K) and T(-Im K) right-aligned at the frame's end."""
    Ks = plan.cqt_kernels()
    wr, wi = np.zeros((len(Ks), n_fft), T), np.zeros((len(Ks), n_fft), T)
    for k, K in enumerate(Ks):
        wr[k, n_fft - K.size:] = K.real.astype(T)
        wi[k, n_fft - K.size:] = (-K.imag).astype(T)
    return wr, wi, np.array([K.size for K in Ks])


def first_tap(wr, wi):
    return int(np.argmax(((wr != 0) | (wi != 0)).any(axis=0)))  # the first tap that any bin weighs


def expected(wr, wi, imps, n, n_fft, hop, pad=0):
    """Read-back expectation [b][bins][frames] (re, im) from the impulse positions alone: imps = [(positions, amplitudes)] per signal."""
    T = wr.dtype.type
    nf = n_frames(n, n_fft, hop, pad)
    re, im = np.zeros((len(imps), wr.shape[0], nf), T), np.zeros((len(imps), wr.shape[0], nf), T)
    for b, (pos, s) in enumerate(imps):
        i, f, t = hits(pos, n, n_fft, hop, pad)
        i, f, t = (a[t >= first_tap(wr, wi)] for a in (i, f, t))  # (the taps in front of it weigh nothing in any bin)
        assert f.size == np.unique(f).size, "a frame holds two impulses within the kernels' reach"
        sv = np.asarray(s, np.float64)[i].astype(T)
        re[b][:, f] = wr[:, t] * sv[None, :]  # a power of two times T(w): exact
        im[b][:, f] = wi[:, t] * sv[None, :]
    return re, im


def impulse_signals(n_fft, hop, n=None, extra=((), ())):
    """Two signals: the train, and the train shifted by 3 samples; `extra` adds (position, amplitude) pairs per signal (negative
    positions count from the end)."""
    pos, s = train(n_fft, hop)
    n = int(pos[-1]) + n_fft if n is None else n
    imps = []
    for shift, more in zip((0, 3), extra):
        p = np.concatenate([pos + shift, np.array([q % n for q, _ in more], np.int64)])
        a = np.concatenate([s, np.array([v for _, v in more], np.float64)])
        imps.append((p, a))
    x = np.zeros((2, n), np.float64)
    for b, (p, a) in enumerate(imps):
        x[b, p] = a
    return x, imps, n


def framed(x, n_fft, hop, pad=0):
    """[b][frames][n_fft] of x, zero outside the signal."""
    b, n = x.shape
    nf = n_frames(n, n_fft, hop, pad)
    xp = np.zeros((b, max(n + 2 * pad, (nf - 1) * hop + n_fft)), x.dtype)
    xp[:, pad:pad + n] = x
    return xp[:, np.arange(nf)[:, None] * hop + np.arange(n_fft)[None, :]]


def chain_rows(X, w):
    """The f32 fma chain of one weight row: X [..., taps] f32 samples, w [taps] f32, taps ascending."""
    acc = np.zeros(X.shape[:-1], np.float32)
    for t in range(int(np.argmax(w != 0)), w.size):
        acc = (acc.astype(LD) + X[..., t].astype(LD) * LD(w[t])).astype(np.float32)
    return acc


def fma_chain(x, wr, wi, n_fft, hop, pad=0):
    """(re, im) [b][bins][frames] of the f32 fma chain over the taps in ascending order, every bin at once."""
    X = framed(x.astype(np.float32), n_fft, hop, pad).astype(LD)  # [b][frames][n_fft]
    re = np.zeros((X.shape[0], wr.shape[0], X.shape[1]), np.float32)
    im = np.zeros_like(re)
    wrl, wil = wr.astype(LD), wi.astype(LD)
    for t in range(first_tap(wr, wi), n_fft):
        xt = X[:, None, :, t]
        re = (re.astype(LD) + xt * wrl[None, :, t, None]).astype(np.float32)
        im = (im.astype(LD) + xt * wil[None, :, t, None]).astype(np.float32)
    return re, im


def power_of(re, im):
    return (re * re) + (im * im)  # T(T(re re) + T(im im)), Complex::norm_sqr in T


def tile_rows(m):
    return 16 * m if m else 64  # the global route walks tiles of 64 frames


# ---- CPU: coverage, the constructor, the chain emulation ----------------------------------------------------------------------
def test_hop_list_reaches_every_route_per_type():
    for col, elem in ((0, 4), (1, 8)):
        kinds = set()
        for hop, ms in TABLE.items():
            m = lds_m(hop, KLEN, elem)
            assert m == ms[col], (hop, elem, m)
            big = m == 1 and lds_bytes(m, hop, KLEN, elem) > 64 * 1024  # (launch_t then raises the kernel's dynamic LDS limit)
            kinds.add("global" if not m else "1 big" if big else str(m))
        assert kinds == {"4", "2", "1", "1 big", "global"}, (elem, kinds)
    assert {h for h in TABLE if h % 8 == 0} == {64, 256, 320, 512, 768, 1024, 2048, 4096}  # the hops with the LDS bank skew
    plan = tplan(DEFAULT, KLEN, 256)
    wr, _, lens = weights(plan, np.float32, KLEN)
    assert wr.shape[0] == 84 and int((lens == KLEN).sum()) == 25 and lens[83] == 68 and lens[0] == KLEN


@pytest.mark.parametrize("hop", list(TABLE))
def test_train_hits_every_tap_and_every_tile_row(hop):
    pos, _ = train(KLEN, hop)
    n = int(pos[-1]) + KLEN
    i, f, t = hits(pos, n, KLEN, hop)
    assert np.array_equal(np.sort(t), np.arange(KLEN))  # every tap offset exactly once
    assert f.size == np.unique(f).size  # no frame holds two impulses
    for m in set(TABLE[hop]):
        assert np.array_equal(np.unique(f % tile_rows(m)), np.arange(tile_rows(m))), (hop, m)
    assert np.all(np.diff(pos) >= KLEN) and n_frames(n, KLEN, hop, 0) == (n - KLEN) // hop + 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_expectation_constructor_against_the_restatement(dtype):
    """`expected` against ref_cqt (tests/test_cqt.py) on small cases: a transform framing and a centred spectrogram framing.  ref_cqt
    casts ref_kernels, `expected` the plan's own kernels: 1e-12 apart before the cast, so up to an ulp of T apart after it."""
    T, u = NP[dtype], 2.0 ** -24 if dtype == "float32" else 2.0 ** -53
    cq = sg.CqtParams(12, 3, 400.0)
    for n_fft, hop, pad, plan in ((256, 48, 0, tplan(cq, 256, 48, dtype=dtype)), (256, 64, 0, tplan(cq, 256, 64, dtype=dtype)),
                                  (256, 48, 128, cqt_plan(cq, 256, 48, SR, dtype=dtype))):
        wr, wi, lens = weights(plan, T, n_fft)
        n = None if pad == 0 else int(train(n_fft, hop)[0][-1]) + n_fft + 1
        x, imps, n = impulse_signals(n_fft, hop, n, extra=(((0, 2.0), (-1, 0.5)), ((2, -4.0),)) if pad else ((), ()))
        re, im = expected(wr, wi, imps, n, n_fft, hop, pad)
        rre, rim, _, _ = ref_cqt(x, Kept(cq, SR), n_fft, hop, SR, dtype, centre=pad != 0)
        assert re.shape == rre.shape and np.count_nonzero(re) > 1000
        for got, ref in ((re, rre), (im, rim)):
            ref = ref.astype(np.float64)
            assert np.all(np.abs(got - ref) <= (2 * u + 1e-11) * np.abs(ref) + 1e-14), np.max(np.abs(got - ref))
        # the dense product over the framed signal gives the same values exactly (one non-zero term per sum)
        X = framed(x, n_fft, hop, pad)
        assert np.array_equal(np.einsum("bft,kt->bkf", X, wr.astype(np.float64)).astype(T), re)
        assert np.array_equal(np.einsum("bft,kt->bkf", X, wi.astype(np.float64)).astype(T), im)


def round_f32(v):
    """A Fraction rounded once to the nearest f32, ties to even."""
    if v == 0:
        return np.float32(0.0)
    e = math.floor(math.log2(abs(v)))
    while Fraction(2) ** e > abs(v):
        e -= 1
    while Fraction(2) ** (e + 1) <= abs(v):
        e += 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    q = v / quantum
    k = math.floor(q)
    rem = q - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k % 2 == 1):
        k += 1
    return np.float32(float(k * quantum))


def test_long_double_chain_is_the_exact_chain():
    """One group, 64 taps, 320 outputs: the long double emulation of fmaf equals the exactly rounded chain bit for bit."""
    assert np.finfo(LD).nmant >= 63
    rng = np.random.default_rng(11)
    X = signals(1, 64 + 159 * 3, SR, seed=2).astype(np.float32)
    X = framed(X, 64, 3)[0]  # [160][64]
    X[80:, 32:] *= np.float32(1e-4)
    W = (rng.standard_normal((2, 64)) * np.hanning(64)[None, :] / 8.0).astype(np.float32)
    for w in W:
        got = chain_rows(X, w)
        ref = np.empty(X.shape[0], np.float32)
        for f in range(X.shape[0]):
            acc = Fraction(0)
            for t in range(64):
                acc = Fraction(float(round_f32(acc + Fraction(float(X[f, t])) * Fraction(float(w[t])))))
            ref[f] = np.float32(float(acc))
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # round_f32 itself: ties to even, and the exact values
    one, ulp = Fraction(1), Fraction(2) ** -23
    assert round_f32(one + ulp / 2) == np.float32(1.0) and round_f32(one + 3 * ulp / 2) == np.float32(1.0) + np.float32(2.0 ** -22)
    assert round_f32(Fraction(1, 3)) == np.float32(1.0 / 3.0) and round_f32(-Fraction(5, 4)) == np.float32(-1.25)


# ---- CPU calibration: the hole is real and the two checks close it ------------------------------------------------------------
def mutants(wr, wi, k):
    """(name, wr, wi, src) of bin k: src[t] is the frame tap that the bin's tap t reads."""
    ident = np.arange(wr.shape[1])
    scale = np.float32(1.001)
    yield "table off by 1e-3", wr[k] * scale, wi[k] * scale, ident
    mid = wr.shape[1] // 2
    src = ident.copy()
    src[mid] = mid - 1
    yield "one tap reads its neighbour", wr[k], wi[k], src
    nz = int(np.argmax(wr[k] != 0))
    dr, di = wr[k].copy(), wi[k].copy()
    dr[nz] = di[nz] = 0
    yield "first non-zero tap dropped", dr, di, ident


@pytest.mark.parametrize("k", [0, 24])
def test_calibration_mutants_pass_the_bound_and_fail_the_exact_checks(k):
    """f32, klen 2048, bins 0 and 24 (2048 taps each), in NumPy: three mistakes that check_complex's e accepts on the `signals` input,
    each of which changes the read-back expectation and the fma chain."""
    hop = 64
    wr, wi, _ = weights(tplan(DEFAULT, KLEN, hop), np.float32, KLEN)
    x = signals(1, KLEN, SR)
    re, im, mag, lg = ref_cqt(x, Kept(DEFAULT, SR), KLEN, hop, SR, "float32", centre=False)
    e = (lg[k] + 2) * 2.0 ** -24 * mag[0, k, 0]
    Xs = framed(x.astype(np.float32), KLEN, hop)[0]  # [1][2048]
    xi, imps, n = impulse_signals(KLEN, hop)
    Xi = framed(xi[:1], KLEN, hop)[0]  # [frames][2048], one impulse a frame
    ere, eim = expected(wr, wi, imps[:1], n, KLEN, hop)
    ident = np.arange(KLEN)

    def readback(w, src):
        return (Xi[:, src] @ w.astype(np.float64)).astype(np.float32)

    assert np.array_equal(readback(wr[k], ident), ere[0, k]) and np.array_equal(readback(wi[k], ident), eim[0, k])
    base = chain_rows(Xs, wr[k]), chain_rows(Xs, wi[k])
    clean = max(abs(float(base[0][0]) - re[0, k, 0]), abs(float(base[1][0]) - im[0, k, 0])) / e
    print(f"bin {k}: unmutated chain error / e = {clean:.3g}")
    assert clean < 1.0
    for name, mr, mi, src in mutants(wr, wi, k):
        got = chain_rows(Xs[:, src], mr), chain_rows(Xs[:, src], mi)
        ratio = max(abs(float(got[0][0]) - re[0, k, 0]), abs(float(got[1][0]) - im[0, k, 0])) / e
        print(f"bin {k}: {name}: error / e = {ratio:.3g}")
        assert ratio < 1.0, (name, ratio)  # today's f32 bound accepts it
        changed = np.count_nonzero(readback(mr, src) != ere[0, k]) + np.count_nonzero(readback(mi, src) != eim[0, k])
        assert changed >= 1, name  # the read-back does not
        assert got[0][0] != base[0][0] or got[1][0] != base[1][0], name  # nor does the chain


# ---- GPU: impulse read-back ---------------------------------------------------------------------------------------------------
def assert_route(plan, hop, lpad, dtype, m):
    assert lds_m(hop, lpad, 4 if dtype == "float32" else 8) == m, (hop, lpad, dtype)
    assert plan.kernel_name == ("cqt_mfma_lds" if m else "cqt_mfma_global"), plan.kernel_name


def assert_readback(got, re, im):
    assert got.shape == re.shape and got.real.dtype == re.dtype
    bad = np.count_nonzero(got.real != re) + np.count_nonzero(got.imag != im)
    if bad:
        b, k, f = (a[:8] for a in np.nonzero((got.real != re) | (got.imag != im)))
        raise AssertionError(f"{bad} values differ; first (signal, bin, frame): {list(zip(b.tolist(), k.tolist(), f.tolist()))}")


def transform_readback(cq, klen, hop, dtype, ms):
    m = ms[DTYPES.index(dtype)]
    plan = gplan(cq, klen, hop, SR, dtype=dtype)
    wr, wi, lens = weights(plan, NP[dtype], klen)
    x, imps, n = impulse_signals(klen, hop)
    got = plan.compute_batch(x.astype(NP[dtype]))
    assert_route(plan, hop, -(-int(lens.max()) // 16) * 16, dtype, m)
    re, im = expected(wr, wi, imps, n, klen, hop)
    assert np.count_nonzero(re) >= lens.sum() // 2  # (sparsity and the window's end taps leave some coefficients 0)
    assert_readback(got, re, im)
    return lens


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hop", list(TABLE))
def test_gpu_readback_transform(hop, dtype):
    lens = transform_readback(DEFAULT, KLEN, hop, dtype, TABLE[hop])
    assert lens.size == 84


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_readback_partial_last_group(dtype):
    lens = transform_readback(sg.CqtParams(12, 9, 55.0), 1024, 256, dtype, (4, 2))
    assert lens.size == 87  # a last group of 7


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_readback_taps_in_front_of_the_signal(dtype):
    """klen 1000: lpad 1008, 8 zero taps in front of sample 0 in every frame; several frames per signal (one each: the rows test)."""
    lens = transform_readback(DEFAULT, 1000, 256, dtype, (4, 2))
    assert lens.max() == 1000 and lens.size == 84


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_readback_rows_route(dtype):
    """klen one-frame signals, signal r with its impulse at tap r; device rows klen + 37 apart with NaN in between."""
    import torch
    klen, hop = 1000, 256
    plan = gplan(DEFAULT, klen, hop, SR, dtype=dtype)
    wr, wi, lens = weights(plan, NP[dtype], klen)
    s = amp_of(np.arange(klen)).astype(NP[dtype])
    host = np.full((klen, klen + 37), np.nan, NP[dtype])
    host[:, :klen] = np.diag(s)
    x = torch.from_numpy(host).cuda()
    re, im = (wr * s[None, :]).T[:, :, None], (wi * s[None, :]).T[:, :, None]  # [signal = tap][bin][1]
    for b in (1, 15, 16, 17, klen):
        xs = x[:b, :klen]
        assert xs.stride(0) == klen + 37
        plan.set_route(2)
        got = plan.compute_batch(xs).cpu().numpy()
        assert plan.kernel_name == "cqt_mfma_rows"
        assert_readback(got, re[:b], im[:b])
        plan.set_route(1)
        got = plan.compute_batch(xs).cpu().numpy()
        assert_route(plan, hop, 1008, dtype, (4, 2)[DTYPES.index(dtype)])
        assert_readback(got, re[:b], im[:b])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hop", [256, 100])
def test_gpu_readback_spectrogram_plan(hop, dtype):
    """sgx_plan_create_cqt plans: centred framing, power output.  Impulses at sample 0 and at sample n - 1 besides the train, and
    one at sample 100 of the second signal (frame 0 hangs 512 samples over the start and weighs taps 535 .. 1023 only)."""
    cq, n_fft = sg.CqtParams.musical(), 1024
    plan = cqt_plan(cq, n_fft, hop, SR, _ffi.AMP_POWER, None, dtype, device=_ffi.DEVICE_CURRENT, centre=True)
    wr, wi, lens = weights(plan, NP[dtype], n_fft)
    assert lens[0] == 489 and lens.size == 84
    n = int(train(n_fft, hop)[0][-1]) + n_fft + 1
    x, imps, n = impulse_signals(n_fft, hop, n, extra=(((0, 2.0), (-1, 0.5)), ((100, -4.0),)))
    got = plan.compute_batch(x.astype(NP[dtype]))
    assert_route(plan, hop, 496, dtype, 4 if (dtype == "float32" or hop == 100) else 2)
    re, im = expected(wr, wi, imps, n, n_fft, hop, n_fft // 2)
    want = power_of(re, im)
    nf = n_frames(n, n_fft, hop, n_fft // 2)
    assert np.count_nonzero(want[1, :, 0]) > 0 and np.count_nonzero(want[0, :, nf - 2:]) > 0  # both overhanging ends are read
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_readback_recompute_path(dtype):
    """A NaN 700 taps in front of an impulse: the frames that hold both take the sequential recompute path, their bins whose own
    taps hold the NaN are NaN in both parts and every other bin reads its impulse back exactly."""
    hop = 256
    plan = gplan(DEFAULT, KLEN, hop, SR, dtype=dtype)
    wr, wi, lens = weights(plan, NP[dtype], KLEN)
    x, imps, n = impulse_signals(KLEN, hop)
    zs = (int(imps[0][0][5]) - 700, int(imps[1][0][9]) - 300)
    for b, z in enumerate(zs):
        assert x[b, z] == 0.0
        x[b, z] = np.nan
    got = plan.compute_batch(x.astype(NP[dtype]))
    assert_route(plan, hop, KLEN, dtype, TABLE[hop][DTYPES.index(dtype)])
    re, im = expected(wr, wi, imps, n, KLEN, hop)
    nan = np.zeros(re.shape, bool)
    for b, z in enumerate(zs):
        _, f, t = hits([z], n, KLEN, hop)
        nan[b][:, f] = (KLEN - lens)[:, None] <= t[None, :]
    F = tile_rows(TABLE[hop][DTYPES.index(dtype)])
    for b in range(2):
        fb = nan[b].any(axis=0)
        redo = fb & ~nan[b].all(axis=0) & ((re[b] != 0) & ~nan[b]).any(axis=0)  # NaN in reach, finite bins that read an impulse
        assert redo.any() and not fb.all()
        tiles = np.unique(np.nonzero(redo)[0] // F)
        assert any((~fb[t * F:(t + 1) * F]).any() for t in tiles)  # a frame of the same tile stays on the matrix cores
    for part, want in ((got.real, re), (got.imag, im)):
        assert np.array_equal(np.isnan(part), nan), (np.isnan(part).sum(), nan.sum())
        assert np.all((part == want) | nan), np.argwhere((part != want) & ~nan)[:8].tolist()


# ---- GPU: f32 against its fma chain -------------------------------------------------------------------------------------------
def assert_chain(name, got, ref):
    """At most 1 output in 10^4 off the chain, none by more than 4 spacings of its bin's largest |value|."""
    assert got.shape == ref.shape and got.dtype == np.float32 and np.all(np.isfinite(got))
    share = float(np.mean(got != ref))
    ulp = np.spacing(np.max(np.abs(ref), axis=(0, 2)).astype(np.float32))[None, :, None]
    worst = float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64)) / ulp))
    print(f"cqt f32 chain {name}: {share:.3g} of {got.size} outputs differ, largest difference {worst:.3g} ulp of the bin's maximum")
    assert share <= 1e-4 and worst <= 4.0, (share, worst)


def stepped(b, n, seed):
    x = signals(b, n, SR, seed)
    x[b - 1, n // 2:] *= 1e-4  # a level step inside a tile's shared span
    return x.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("hop", [64, 512, 4096])
def test_gpu_f32_fma_chain_transform(hop):
    plan = gplan(DEFAULT, KLEN, hop, SR, dtype="float32")
    wr, wi, _ = weights(plan, np.float32, KLEN)
    x = stepped(2, KLEN + 69 * hop + 5, seed=21)
    got = plan.compute_batch(x)
    assert_route(plan, hop, KLEN, "float32", TABLE[hop][0])
    assert got.shape == (2, 84, 70)  # more than one tile and a partial one
    re, im = fma_chain(x, wr, wi, KLEN, hop)
    assert_chain(f"transform hop {hop} re", np.ascontiguousarray(got.real), re)
    assert_chain(f"transform hop {hop} im", np.ascontiguousarray(got.imag), im)


@pytest.mark.gpu
def test_gpu_f32_fma_chain_rows_route():
    klen, hop = 1000, 256
    plan = gplan(DEFAULT, klen, hop, SR, dtype="float32")
    wr, wi, _ = weights(plan, np.float32, klen)
    x = stepped(33, klen, seed=22)
    plan.set_route(2)
    got = plan.compute_batch(x)
    assert plan.kernel_name == "cqt_mfma_rows" and got.shape == (33, 84, 1)
    re, im = fma_chain(x, wr, wi, klen, hop)
    assert_chain("rows re", np.ascontiguousarray(got.real), re)
    assert_chain("rows im", np.ascontiguousarray(got.imag), im)


@pytest.mark.gpu
def test_gpu_f32_fma_chain_spectrogram_plan():
    cq, n_fft, hop = sg.CqtParams.musical(), 1024, 256
    plan = cqt_plan(cq, n_fft, hop, SR, _ffi.AMP_POWER, None, "float32", device=_ffi.DEVICE_CURRENT, centre=True)
    wr, wi, _ = weights(plan, np.float32, n_fft)
    x = stepped(2, 69 * hop + 5, seed=23)
    got = plan.compute_batch(x)
    assert_route(plan, hop, 496, "float32", 4)
    assert got.shape == (2, 84, 70)
    re, im = fma_chain(x, wr, wi, n_fft, hop, n_fft // 2)
    assert_chain("spectrogram 1024 / 256 power", got, power_of(re, im))


# ---- GPU: f64, random input, the hops without the LDS skew --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hop", [441, 100])
def test_gpu_f64_bound_without_skew(hop):
    """f64 keeps check_complex's bound (sharp at u = 2^-53) on random input; klen 2048 at the two hops without the LDS skew, M = 1 and
    M = 4, which no complex f64 case had.  At hop 441 the read-back found frame rows 12 .. 15 of the M = 1 instance losing every 4th
    MFMA (the accumulator was read before v_mfma_f64_16x16x4_f64 had written its last register; cqt.hip mfma_drain): on this input the
    error was 7.7e12 times the bound."""
    plan, got = run_complex(DEFAULT, KLEN, hop, SR, KLEN + 36 * hop + 5, 2, "float64")
    assert_route(plan, hop, KLEN, "float64", TABLE[hop][1])
    assert got.shape == (2, 84, 37)
