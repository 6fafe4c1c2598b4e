"""The global-memory transforms (spectrograms_amd/csrc/bigfft.hip) at every sequence length M = 2^14 ... 2^21, in both element types, in both
forms (four-step for powers of two, chirp-z on top of it for every other length), through every entry point that reaches `run_chain`
(forward STFT, C2cPlan, the inverse rows), and across the seams between scratch chunks.

Geometry per M, restated on the CPU from `tile_lanes` / `big_chunk_seqs` (bigfft.hip).  test_geometry_table_restates_tile_lanes checks the table
against this file's own Python copy of those two functions: it pins the test's view of the geometry (which case exercises which tile
and chunk size), not the kernel's — nothing in the C ABI reports them, so a change of bigfft.hip's rule has to be restated here by hand.
l1 = ceil(l / 2), l2 = floor(l / 2); a factor with an odd log2 takes one single radix-2 stage (lds_r2_stage) beside the paired ones
(lds_r4_stage); C sequences per tile within 36 / 72 / 144 KiB of LDS; kBigChunkBytes = 256 MiB of scratch per buffer.

  | M    | l1, l2 | f32: C,KiB in pass A / pass B; sequences per chunk | f64: C,KiB in pass A / pass B; sequences per chunk |
  | 2^14 |  7,  7 | 32,36 / 32,36; 2048                                | 16,36 / 16,36; 1024                                |
  | 2^15 |  8,  7 | 16,36 / 32,36; 1024                                |  8,36 / 16,36;  512                                |
  | 2^16 |  8,  8 | 16,36 / 16,36;  512                                |  8,36 /  8,36;  256                                |
  | 2^17 |  9,  8 |  8,36 / 16,36;  256                                |  8,72 /  8,36;  128                                |
  | 2^18 |  9,  9 |  8,36 /  8,36;  128                                |  8,72 /  8,72;   64                                |
  | 2^19 | 10,  9 |  8,72 /  8,36;   64                                |  8,144 / 8,72;   32                                |
  | 2^20 | 10, 10 |  8,72 /  8,72;   32                                |  8,144 / 8,144;  16                                |
  | 2^21 | 11, 10 |  8,144 / 8,72;   16                                |  2,144 / 8,144;   8                                |

Lengths per M: n = M (four-step), and M/4 + 1, M/2 - 1, M/4 + 2 (chirp-z: the smallest odd, the largest odd and the smallest even
length whose convolution length is M).  n_fft = 2^21 exists only as a power of two; its M is also the chirp-z M of 524 289 ... 2^20 - 1.

References: numpy.fft in f64 of the T-cast input for f32 plans, numpy.fft in np.longdouble of the T-cast input for f64 plans (asserted
at import: numpy's pocketfft keeps long double).  u = 2^-24 / 2^-53.  Constants, those of tests/test_frame_locality.py and
tests/test_istft_precision.py: c = 4 with N_eff = n for the four-step form; c = 12 = 3 x 4 with N_eff = M for chirp-z (three transforms
of the padded length M plus two chirp products).

  forward, per pair of frames (frames 2p and 2p + 1 of a signal ride ONE complex sequence, an odd last frame rides alone; d_a, d_b the
  errors of the two frames over bins 0 ... n/2):
      sqrt(sum_k |d_a[k]|^2 + |d_b[k]|^2) <= c u log2(N_eff) sqrt(N_eff) sqrt(||x_a w||^2 + ||x_b w||^2)
      (test_frame_locality.frame_deltas(joint=True), on the 2-norm over the bins instead of the maximum: the derivation bounds the
      2-norm, the Hermitian split A = (P + conj Q) / 2, B = -i (P - conj Q) / 2 does not enlarge it, and an error spread over many
      bins shows sqrt(n) times earlier.)  Power outputs: |dP[k]| <= delta (2 |X[k]| + delta) with delta that right-hand side.
  impulse, per bin, powers of two: a one-sample frame meets only exact zeros in every butterfly, so each output is the sample times at
      most log2(n) stage twiddles and the one tw_big product (two rounded table entries: two more):
      |X[k] - W_n^(jk)| <= 4 u (log2(n) + 2), the reference exp(-2 pi i ((j k) mod n) / n) in long double.
      (Per product: a rounded table entry, sqrt(2) u / 2, and a complex multiplication, sqrt(5) u: under 3 u; the split's one sum: u.)
  C2cPlan, noise: ||dX||_2 <= c u log2(N_eff) sqrt(N_eff) ||x||_2; the inverse: the same on inverse(X) / n, i.e. with ||X||_2 / n.
  inverse, one row: max_t |dy[t]| <= c u log2(N_eff) ||y||_2; overlap-added (tests/test_inverse_long_rows.py's second formula):
      |dy[t]| <= (sum_f |w[t - f hop]| c u log2(N_eff) ||y_f||_2) / norm[t] + 4 u |y[t]|.
  epilogue kinds against the same plan shape's complex output X^: |P - |X^|^2| <= 4 u |X^|^2 and |A - |X^|| <= 4 u |X^| (one sum of two
      products, FMA or not, and one square root); dB against 10 log10(max(P^, eps)) of the GPU's own power: f64 within db_f64.h's
      4e-15 + 3e-16 |dB| plus one ulp, f32 within 2e-5 dB.

C2cPlan reports no route name.  sgx_c2c_create (fft2d.hip) uploads the bigfft tables, and c2c_run then calls launch_big_c2c, when the
length has no register-tiled split, no LDS chirp-z, more than 2048 points, and either no on-chip tile (fft2d_tile_for: (n + 1) complex
elements within 144 KiB, i.e. f32 up to 2^14 and f64 up to 2^13) or is no power of two: every power of two from 2^15 (f32) / 2^14 (f64)
and 131 073 (M = 2^19) and 524 287 (M = 2^20) are such lengths.

Chunk seams: the scratch holds `big_chunk_seqs` sequences; a larger call is cut at multiples of it, and for the four-step form the
natural-order buffer sits at buf + chunk M.  The seam cases put a seam INSIDE a signal and compare every signal with the same signal
computed alone (one chunk, no seam), bit for bit.

Every case prints its worst ratio to its bound (DESIGN.md 3.6 keeps the table).
"""
import functools
import math

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests import helpers as H

assert np.fft.fft(np.zeros(4, np.longdouble)).dtype == np.complex256, "numpy.fft must keep long double: it is the f64 plans' reference"

F32, F64 = "float32", "float64"
DTYPES = (F32, F64)
NP = {F32: np.float32, F64: np.float64}
CNP = {F32: np.complex64, F64: np.complex128}
REF = {F32: np.float64, F64: np.longdouble}        # the reference's real type
CREF = {F32: np.complex128, F64: np.complex256}
U = {F32: 2.0 ** -24, F64: 2.0 ** -53}
C_FORM = {"four_step": 4.0, "chirpz": 12.0}
HOST = _ffi.DEVICE_HOST_ONLY
LD = np.longdouble
PI_LD = LD(4) * np.arctan(LD(1))
WORST = {}

# ---- geometry ------------------------------------------------------------------------------------------------------------------------
# M -> ((l1, l2), f32 ((C, KiB) pass A, (C, KiB) pass B, sequences per chunk), f64 the same): the docstring's table
GEOMETRY = {
    1 << 14: ((7, 7), ((32, 36), (32, 36), 2048), ((16, 36), (16, 36), 1024)),
    1 << 15: ((8, 7), ((16, 36), (32, 36), 1024), ((8, 36), (16, 36), 512)),
    1 << 16: ((8, 8), ((16, 36), (16, 36), 512), ((8, 36), (8, 36), 256)),
    1 << 17: ((9, 8), ((8, 36), (16, 36), 256), ((8, 72), (8, 36), 128)),
    1 << 18: ((9, 9), ((8, 36), (8, 36), 128), ((8, 72), (8, 72), 64)),
    1 << 19: ((10, 9), ((8, 72), (8, 36), 64), ((8, 144), (8, 72), 32)),
    1 << 20: ((10, 10), ((8, 72), (8, 72), 32), ((8, 144), (8, 144), 16)),
    1 << 21: ((11, 10), ((8, 144), (8, 72), 16), ((2, 144), (8, 144), 8)),
}
MS = sorted(GEOMETRY)


def tile_lanes(L, lanes, dtype):
    """bigfft.hip tile_lanes: (sequences per tile, KiB of the LDS budget that gave them)."""
    cb = 8 if dtype == F32 else 16

    def fit(budget):
        C = 1
        while 2 * C <= lanes and 2 * C * (L + 1) * cb + (L // 2) * cb <= budget and 2 * C <= 64:
            C *= 2
        return C

    seg = 64 // cb
    for kib in (36, 72):
        C = fit(kib << 10)
        if C >= seg or C >= lanes:
            return C, kib
    return fit(144 << 10), 144


def chunk_seqs(M, dtype):
    """bigfft.hip big_chunk_seqs for a call of many sequences."""
    return min(max((256 << 20) // (M * 2 * (4 if dtype == F32 else 8)), 1), 32768)


def log2i(v):
    assert v & (v - 1) == 0
    return v.bit_length() - 1


def big_m(n):
    """Sequence length of frame length n: n itself for a power of two, else the chirp-z convolution length 2^ceil(log2(2n - 1))."""
    if n & (n - 1) == 0:
        return n
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def form_of(n):
    return "chirpz" if n & (n - 1) else "four_step"


def lengths_of(M):
    return (M, M // 4 + 1, M // 2 - 1, M // 4 + 2)


def expected_route(dtype, M, n):
    """sgx_kernel_name of the forward plan, read off plan.hip's cost model and checked on a build of this tree."""
    l, f64 = log2i(M), dtype == F64
    if n == M:
        return "big_four_step" if l >= (15 if f64 else 16) else "lds_radix2"
    if n == M // 4 + 2:
        return "big_chirpz" if l >= (15 if f64 else 16) else "bluestein"
    return "big_chirpz" if l >= (14 if f64 else 15) else "bluestein"


# (dtype, M, n) of every length of the table that runs in bigfft.hip
BIG = [(d, M, n) for d in DTYPES for M in MS for n in lengths_of(M) if expected_route(d, M, n).startswith("big_")]
FOUR = [c for c in BIG if form_of(c[2]) == "four_step"]


def cid(c):
    return f"{c[0][5:]}-2^{log2i(c[1])}-{c[2]}"


def record(entry, dtype, n, ratio, note=""):
    name = f"{entry} {form_of(n)} {dtype} M=2^{log2i(big_m(n))} n={n}{note}"
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    print(f"{name}: worst ratio to bound {WORST[name]:.3g}")


def make_plan(dtype, n, hop, amp=_ffi.AMP_COMPLEX, window=None, centre=False, db=None, device=_ffi.DEVICE_CURRENT):
    window = window or ("hanning" if form_of(n) == "chirpz" else "rectangular")
    params = sg.SpectrogramParams(sg.StftParams(n, hop, getattr(sg.WindowType, window), centre), 16000.0)
    return sg.Plan(params, amp, None, db, dtype, device=device)


def test_geometry_table_restates_tile_lanes():
    for M, ((l1, l2), f32, f64) in GEOMETRY.items():
        l = log2i(M)
        assert (l1, l2) == ((l + 1) // 2, l // 2)
        for dtype, row in ((F32, f32), (F64, f64)):
            got = (tile_lanes(1 << l1, 1 << l2, dtype), tile_lanes(1 << l2, 1 << l1, dtype), chunk_seqs(M, dtype))
            assert got == row, (M, dtype, got, row)
    # the LDS budgets the issue lists as never run by the older files: f64 (A 72, B 36), f64 (A 144, B 72), f32 (A 72, B 36)
    assert GEOMETRY[1 << 17][2][0][1:] + GEOMETRY[1 << 17][2][1][1:] == (72, 36)
    assert GEOMETRY[1 << 19][2][0][1:] + GEOMETRY[1 << 19][2][1][1:] == (144, 72)
    assert GEOMETRY[1 << 19][1][0][1:] + GEOMETRY[1 << 19][1][1][1:] == (72, 36)


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_table(dtype):
    """The kernel every length of the table takes (host-only plans: the decision is the same, no tables are built)."""
    seen = {}
    for M in MS:
        for n in lengths_of(M):
            name = make_plan(dtype, n, n // 3 + 1, device=HOST).kernel_name
            assert name == expected_route(dtype, M, n), (dtype, M, n, name)
            seen[n] = name
    f64 = dtype == F64
    assert seen[4098 if f64 else 8194] == "bluestein" and seen[16384 if f64 else 32768] == "lds_radix2"
    assert seen[32768 if f64 else 65536] == "big_four_step" and seen[4097 if f64 else 8193] == "big_chirpz"
    assert seen[8194 if f64 else 16386] == "big_chirpz"
    assert len([c for c in BIG if c[0] == dtype]) == (30 if f64 else 26)


# ---- inputs, references, bounds --------------------------------------------------------------------------------------------------
def noise_and_tone(seed, nsig, length, dtype):
    rng = np.random.default_rng(seed)
    t = np.arange(length) / 16000.0
    x = 0.5 * np.sin(2 * np.pi * 440.0 * t)[None, :] * np.linspace(1.0, 0.5, nsig)[:, None] + 0.1 * rng.standard_normal((nsig, length))
    return x.astype(NP[dtype])


def windowed_frames(row, w, n, hop, centre, dtype):
    """[n_frames, n] frames of one T-valued signal times the window, in the reference's type (both factors are exact there)."""
    return H.np_frames(np.asarray(row, np.float64), n, hop, centre).astype(REF[dtype]) * w.astype(REF[dtype])[None, :]


def pair_sums(v):
    """[n_frames] -> [pairs]: v[2p] + v[2p + 1], an odd last frame alone."""
    return np.add.reduceat(v, np.arange(0, v.size, 2))


def forward_delta(fr, n, dtype):
    """The right-hand side of the forward bound per pair of frames; fr: the windowed frames [n_frames, n]."""
    Neff = big_m(n)
    nrm2 = pair_sums(np.sum(fr * fr, axis=1).astype(np.float64))
    return C_FORM[form_of(n)] * U[dtype] * math.log2(Neff) * math.sqrt(Neff) * np.sqrt(nrm2)


def forward_ratios(got, fr, n, dtype):
    """got [bins, n_frames] of one signal -> (ratio per pair, the reference spectrum [n_frames, bins])."""
    X = np.fft.rfft(fr, axis=-1)
    assert X.dtype == CREF[dtype]
    d = got.T.astype(CREF[dtype]) - X
    err = np.sqrt(pair_sums(np.sum(d.real ** 2 + d.imag ** 2, axis=1).astype(np.float64)))
    return err / forward_delta(fr, n, dtype), X


def check_forward(plan, x, dtype, n, hop, centre, entry="stft", note=""):
    """Forward bound for every pair of every signal of x, exactly-real DC / Nyquist; returns the output."""
    S = plan.compute_batch(x)
    w = np.asarray(plan.window(), np.float64)
    assert S.dtype == CNP[dtype] and S.shape == (x.shape[0],) + tuple(plan.output_shape(x.shape[1]))
    worst = 0.0
    for b in range(x.shape[0]):
        r, _ = forward_ratios(S[b], windowed_frames(x[b], w, n, hop, centre, dtype), n, dtype)
        assert r.size == (S.shape[2] + 1) // 2
        worst = max(worst, float(np.max(r)))
    record(entry, dtype, n, worst, note)
    assert worst <= 1.0, (dtype, n, worst)
    assert not S[:, 0, :].imag.any() and (n % 2 or not S[:, -1, :].imag.any())
    return S


def three_frames_len(n, hop, centre):
    return (n % 2 + 2 * hop) if centre else n + 2 * hop


def test_bound_calibration_separates_a_single_wrong_bin():
    """Not vacuous, not blind (CPU): a paired complex64 transform sits within a few decades under the forward bound, and one noise bin
    wrong by a hundredth of its own size, which the peak-relative tolerance of tests/test_bigfft.py passes, breaks it."""
    import torch
    n = 1 << 16
    x = noise_and_tone(1, 1, n + n, F32)[0]
    fr = windowed_frames(x, np.ones(n), n, n, False, F32)
    z = torch.fft.fft(torch.complex(torch.from_numpy(fr[0].astype(np.float32)), torch.from_numpy(fr[1].astype(np.float32)))).numpy()
    zc = np.conj(np.roll(z[::-1], 1))
    got = np.stack([((z + zc) / 2)[:n // 2 + 1], (-1j * (z - zc) / 2)[:n // 2 + 1]], axis=1).astype(np.complex64)
    r, X = forward_ratios(got, fr, n, F32)
    print(f"paired complex64 transform, n = 2^16: ratio {r[0]:.3g}")
    assert 1e-4 < r[0] <= 1.0
    k = 4000 + int(np.argmax(np.abs(got[4000:, 0])))  # (the largest noise bin; the tone sits at bin 1802)
    bad = got.copy()
    bad[k, 0] *= np.float32(1.01)
    rb, _ = forward_ratios(bad, fr, n, F32)
    err, peak = abs(complex(bad[k, 0]) - complex(got[k, 0])), float(np.max(np.abs(X)))
    print(f"bin {k} wrong by 1% of its size: ratio {rb[0]:.3g}; the error is {err / peak:.3g} of the peak")
    assert rb[0] > 1.0 and err < 1e-4 * peak


# ---- 2. forward matrix ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", BIG, ids=cid)
def test_gpu_forward_pairs_meet_the_bound(case):
    """Three frames (a pair and a lone frame) per signal, unaligned hop, no centring: kernel name, the forward bound per pair, exactly
    real DC / Nyquist, and signal 1 alone bit-equal to its rows in the batch."""
    dtype, M, n = case
    hop = n // 3 + 1
    nsig = 2 if M < (1 << 20) else 1
    plan = make_plan(dtype, n, hop)
    assert plan.kernel_name == expected_route(dtype, M, n) and big_m(n) == M
    x = noise_and_tone(n, nsig, three_frames_len(n, hop, False), dtype)
    S = check_forward(plan, x, dtype, n, hop, False)
    assert S.shape[2] == 3
    if nsig > 1:
        assert np.array_equal(plan.compute_batch(x[1:2])[0], S[1])


CENTRED = [(F32, 1 << 17), (F64, 1 << 18), (F32, (1 << 18) // 4 + 1), (F64, (1 << 17) // 2 - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n", CENTRED, ids=[f"{d[5:]}-{n}" for d, n in CENTRED])
def test_gpu_forward_centred_frames(dtype, n):
    """One centred case per form and type: the first and last frames read the zero padding (big_frame_elem's out-of-range samples)."""
    hop = n // 3 + 1
    plan = make_plan(dtype, n, hop, centre=True)
    assert plan.kernel_name == ("big_chirpz" if n & (n - 1) else "big_four_step")
    x = noise_and_tone(n + 1, 2, three_frames_len(n, hop, True), dtype)
    S = check_forward(plan, x, dtype, n, hop, True, note=" centred")
    assert S.shape[2] == 3
    assert np.array_equal(plan.compute_batch(x[1:2])[0], S[1])


# ---- 3. impulses ---------------------------------------------------------------------------------------------------------------------
def unit_root(j, k, n):
    """W_n^(j k) for the bins k, in long double."""
    a = (2 * PI_LD) * ((int(j) * k.astype(np.int64)) % n).astype(LD) / LD(n)
    return np.cos(a) - 1j * np.sin(a)


def impulse_positions(n):
    """Sample positions j = n1 M2 + n2 of the unit impulses: 1, M2 - 1, M2, M2 + 1, n / 2, n - 1 and one seeded odd j; then as many more
    as it takes for the set's columns n2 to read EVERY entry of the low twiddle table.  Pass A multiplies output k1 of column n2 by
    tw_big(n2 k1) = thi[p >> 10] tlo[p & 1023]; up to M = 2^18 (M1 <= 512 outputs per column) the first seven positions' three odd
    columns leave entries of tlo unread (at M = 2^16, 2^17 and 2^18 among them entry 777), so a wrong entry there would pass.  The further columns are chosen
    greedily, the one that reads the most unread entries first, until no column reads an unread one."""
    l = log2i(n)
    m1, m2 = 1 << ((l + 1) // 2), 1 << (l // 2)
    pos = [1, m2 - 1, m2, m2 + 1, n // 2, n - 1, int(np.random.default_rng(n).integers(1, n // 2)) * 2 + 1]
    k1 = np.arange(m1)
    reads = lambda n2: (n2 * k1) & 1023
    seen = np.zeros(1024, bool)
    for j in pos:
        seen[reads(j % m2)] = True
    while True:  # (at M = 2^14 some entries are read by no column at all: the loop ends when no column adds one)
        n2 = max(range(1, m2), key=lambda c: np.count_nonzero(~seen[reads(c)]))
        if seen[reads(n2)].all():
            break
        seen[reads(n2)] = True
        pos.append((1 + len(pos) % (m1 - 1)) * m2 + n2)
    return pos


def test_impulse_positions_read_the_whole_low_twiddle_table():
    for l in range(14, 22):
        n = 1 << l
        m1, m2 = 1 << ((l + 1) // 2), 1 << (l // 2)
        pos = impulse_positions(n)
        assert len(pos) == len(set(pos)) and all(0 < j < n for j in pos) and len(pos) <= 40
        assert pos[:6] == [1, m2 - 1, m2, m2 + 1, n // 2, n - 1] and pos[6] % 2 == 1
        read = {(int(j % m2) * k) & 1023 for j in pos for k in range(m1)}
        every = set(((np.arange(m2)[:, None] * np.arange(m1)[None, :]) & 1023).ravel().tolist())
        assert read == every and (l == 14 or len(every) == 1024), (n, len(read), len(every))


def impulse_ratio(row, j, n, dtype):
    """row: bins k = 0 ... len(row) - 1 of the transform of a unit sample at j."""
    ref = unit_root(j, np.arange(row.size), n)
    d = row.astype(np.complex256) - ref
    return float(np.max(np.sqrt(d.real ** 2 + d.imag ** 2))) / (4.0 * U[dtype] * (log2i(n) + 2))


@pytest.mark.gpu
@pytest.mark.parametrize("case", FOUR, ids=cid)
def test_gpu_four_step_impulses_per_bin(case):
    dtype, _, n = case
    pos = impulse_positions(n)
    x = np.zeros((len(pos), n), NP[dtype])
    x[np.arange(len(pos)), pos] = 1.0
    plan = make_plan(dtype, n, n)
    assert plan.kernel_name == "big_four_step"
    S = plan.compute_batch(x)
    assert S.shape == (len(pos), n // 2 + 1, 1)
    worst = max(impulse_ratio(S[i, :, 0], j, n, dtype) for i, j in enumerate(pos))
    record("stft impulse", dtype, n, worst)
    assert worst <= 1.0, (dtype, n, worst)


# ---- 4. epilogue kinds ---------------------------------------------------------------------------------------------------------------
EPILOGUE = [(F32, 1 << 19), (F64, 1 << 19), (F32, (1 << 19) // 4 + 1), (F64, (1 << 19) // 2 - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n", EPILOGUE, ids=[f"{d[5:]}-{n}" for d, n in EPILOGUE])
def test_gpu_power_magnitude_and_db_of_the_same_spectrum(dtype, n):
    """k_big_split's amplitude kinds at M = 2^19 (no older test runs that length): power and magnitude against the complex output of a
    plan of the same shape, dB against the GPU's own power."""
    hop = n // 3 + 1
    u = U[dtype]
    x = noise_and_tone(n + 2, 1, three_frames_len(n, hop, False), dtype)
    name = "big_chirpz" if n & (n - 1) else "big_four_step"
    outs = {}
    for kind, amp, db in (("complex", _ffi.AMP_COMPLEX, None), ("power", _ffi.AMP_POWER, None), ("magnitude", _ffi.AMP_MAGNITUDE, None),
                          ("db", _ffi.AMP_DECIBELS, sg.LogParams(-80.0))):
        plan = make_plan(dtype, n, hop, amp=amp, db=db)
        assert plan.kernel_name == name
        outs[kind] = plan.compute_batch(x)
    Xh = outs["complex"].astype(CREF[dtype])
    p2 = Xh.real ** 2 + Xh.imag ** 2
    P, A, D = (outs[k].astype(REF[dtype]) for k in ("power", "magnitude", "db"))
    assert outs["power"].dtype == NP[dtype] and P.shape == p2.shape == (1, n // 2 + 1, 3)
    live = p2 > 0
    assert live.mean() > 0.99
    rp = float(np.max(np.abs(P - p2)[live] / (4 * u * p2[live])))
    ra = float(np.max(np.abs(A - np.sqrt(p2))[live] / (4 * u * np.sqrt(p2[live]))))
    assert not P[~live].any() and not A[~live].any()
    eps = REF[dtype](NP[dtype](10.0 ** (-80.0 / 10.0)))
    ref = 10 * np.log10(np.maximum(P, eps))
    tol = 2e-5 if dtype == F32 else 4e-15 + 3e-16 * np.abs(ref) + np.spacing(np.abs(ref).astype(np.float64))
    rd = float(np.max(np.abs(D - ref) / tol))
    for kind, r in (("power", rp), ("magnitude", ra), ("db", rd)):
        record(f"stft {kind}", dtype, n, r)
    assert max(rp, ra, rd) <= 1.0, (dtype, n, rp, ra, rd)


# ---- 5. C2cPlan ------------------------------------------------------------------------------------------------------------------------
C2C = [(d, n) for d in DTYPES for n in [1 << l for l in range(15 if d == F32 else 14, 20)] + [131073, 524287]]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n", C2C, ids=[f"{d[5:]}-{n}" for d, n in C2C])
def test_gpu_c2c_forward_inverse_and_impulses(dtype, n):
    """launch_big_c2c (the docstring says why these lengths take it): noise forward and inverse in the 2-norm, impulses per bin."""
    u, form = U[dtype], form_of(n)
    Neff = big_m(n)
    k = C_FORM[form] * u * math.log2(Neff) * math.sqrt(Neff)
    rng = np.random.default_rng(n)
    z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(CNP[dtype])
    plan = sg.C2cPlan(n, dtype)
    zr = z.astype(CREF[dtype])
    ref = np.fft.fft(zr)
    assert ref.dtype == CREF[dtype]
    norm = lambda v: float(np.sqrt(np.sum(v.real ** 2 + v.imag ** 2)))
    rf = norm(plan.forward(z).astype(CREF[dtype]) - ref) / (k * norm(zr))
    record("c2c forward", dtype, n, rf)
    Z = ref.astype(CNP[dtype])
    back = np.fft.ifft(Z.astype(CREF[dtype]))
    ri = norm(plan.inverse(Z).astype(CREF[dtype]) / REF[dtype](n) - back) / (k * norm(Z.astype(CREF[dtype])) / n)
    record("c2c inverse", dtype, n, ri)
    assert rf <= 1.0 and ri <= 1.0, (dtype, n, rf, ri)
    if form == "four_step":
        worst = 0.0
        for j in impulse_positions(n):
            e = np.zeros(n, CNP[dtype])
            e[j] = 1.0
            worst = max(worst, impulse_ratio(plan.forward(e), j, n, dtype))
        record("c2c impulse", dtype, n, worst)
        assert worst <= 1.0, (dtype, n, worst)


# ---- 6. inverse rows -----------------------------------------------------------------------------------------------------------------
def rand_spec(rng, shape, n, dtype):
    """A T-valued half spectrum [..., bins, frames] with real DC and (even n) Nyquist rows."""
    s = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(CNP[dtype])
    s[..., 0, :] = s[..., 0, :].real
    if n % 2 == 0:
        s[..., -1, :] = s[..., -1, :].real
    return s


# one n per (form, type, M): the power of two, and the largest odd length of the M
INVERSE = [c for c in BIG if c[2] in (c[1], c[1] // 2 - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", INVERSE, ids=cid)
def test_gpu_c2r_single_row(case):
    """Plan.c2r / compute_irfft through launch_big_c2r: one row, per sample."""
    dtype, M, n = case
    rng = np.random.default_rng(n + 7)
    X = rand_spec(rng, (n // 2 + 1, 1), n, dtype)[:, 0]
    ref = np.fft.irfft(X.astype(CREF[dtype]), n)
    assert ref.dtype == REF[dtype]
    plan = make_plan(dtype, n, n, window="rectangular")
    got = plan.c2r(X)
    assert plan.istft_kernel_name == "big" and got.shape == (n,) and got.dtype == NP[dtype]
    bound = C_FORM[form_of(n)] * U[dtype] * math.log2(M) * float(np.sqrt(np.sum(ref * ref)))
    ratio = float(np.max(np.abs(got.astype(REF[dtype]) - ref))) / bound
    record("c2r", dtype, n, ratio)
    assert ratio <= 1.0, (dtype, n, ratio)
    assert np.array_equal(sg.compute_irfft(X, n, dtype=dtype), got)
    sg.clear_fft_plan_cache()


def ref_istft(S, w, n, hop, centre, dtype):
    """(y, e) per batch row in the reference's type: the overlap-added reference and sum_f |w| ||y_f||_2 / norm (the bound without
    c u log2 N_eff), as tests/test_inverse_long_rows.py builds them."""
    R = REF[dtype]
    b, _, nf = S.shape
    full = (nf - 1) * hop + n
    w = w.astype(R)
    y, e, norm = np.zeros((b, full), R), np.zeros((b, full), R), np.zeros(full, R)
    for f in range(nf):
        fr = np.fft.irfft(S[:, :, f].astype(CREF[dtype]), n, axis=-1)
        y[:, f * hop:f * hop + n] += fr * w
        e[:, f * hop:f * hop + n] += np.abs(w) * np.sqrt(np.sum(fr * fr, axis=-1, keepdims=True))
        norm[f * hop:f * hop + n] += w * w
    ok = norm > 1e-10
    y[:, ok] /= norm[ok]
    e[:, ok] /= norm[ok]
    pad = n // 2 if centre else 0
    return y[:, pad:full - pad], e[:, pad:full - pad]


def istft_ratio(got, y, e, n, dtype):
    bound = C_FORM[form_of(n)] * U[dtype] * math.log2(big_m(n)) * e + 4.0 * U[dtype] * np.abs(y)
    d = np.abs(got.astype(REF[dtype]) - y)
    return float(np.max(np.where(bound > 0, d / np.where(bound > 0, bound, 1), np.where(d == 0, 0.0, np.inf))))


OLA = [(F32, 1 << 19), (F64, 1 << 19), (F32, (1 << 19) // 4 + 1), (F64, (1 << 19) // 2 - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n", OLA, ids=[f"{d[5:]}-{n}" for d, n in OLA])
def test_gpu_istft_three_frames_at_2_19(dtype, n):
    hop = n // 3 + 1
    plan = make_plan(dtype, n, hop, window="hanning", centre=True)
    S = rand_spec(np.random.default_rng(n + 3), (2, n // 2 + 1, 3), n, dtype)
    got = plan.istft_batch(S)
    assert plan.istft_kernel_name == "big+ola"
    y, e = ref_istft(S, np.asarray(plan.window(), np.float64), n, hop, True, dtype)
    assert got.shape == y.shape and got.dtype == NP[dtype]
    ratio = istft_ratio(got, y, e, n, dtype)
    record("istft", dtype, n, ratio)
    assert ratio <= 1.0, (dtype, n, ratio)


# ---- 7. chunk seams ------------------------------------------------------------------------------------------------------------------
# (n_fft, hop, signals, frames per signal): f64; 1030 sequences against 1024 per chunk (chirp-z, M = 2^14), 519 against 512 (four-step,
# M = 2^15).  The seam falls inside the last signal.
SEAMS = [(4099, 16, 5, 411), (32768, 8, 3, 345)]


@functools.lru_cache(maxsize=2)
def seam_input(n, hop, nsig, nf):
    x = noise_and_tone(n + hop, nsig, n + (nf - 1) * hop, F64)
    x.setflags(write=False)
    return x


def test_seam_shapes_put_a_seam_inside_the_last_signal():
    for n, hop, nsig, nf in SEAMS:
        chunk, pp = chunk_seqs(big_m(n), F64), (nf + 1) // 2
        assert chunk == GEOMETRY[big_m(n)][2][2]
        first, last = (nsig - 1) * pp, nsig * pp - 1
        assert first < chunk <= last and nsig * pp < 2 * chunk and chunk % pp != 0
    assert [((nf + 1) // 2, nsig * ((nf + 1) // 2)) for _, _, nsig, nf in SEAMS] == [(206, 1030), (173, 519)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SEAMS, ids=[f"{s[0]}-{s[1]}" for s in SEAMS])
def test_gpu_forward_power_across_a_chunk_seam(shape):
    """Every signal of a batch that is cut into two chunks is bit-equal to the same signal computed alone; the scratch grows from one
    signal to the batch and serves one signal again with the same bits; a fresh plan reserved for the batch gives the batch's bits;
    the signal the seam cuts meets the forward bound."""
    n, hop, nsig, nf = shape
    x = seam_input(*shape)
    plan = make_plan(F64, n, hop, amp=_ffi.AMP_POWER)
    assert plan.kernel_name == ("big_chirpz" if n & (n - 1) else "big_four_step")
    first = plan.compute_batch(x[0:1])
    full = plan.compute_batch(x)
    assert full.shape == (nsig, n // 2 + 1, nf)
    assert np.array_equal(plan.compute_batch(x[0:1]), first)
    assert np.array_equal(first[0], full[0])
    for s in range(1, nsig):
        assert np.array_equal(plan.compute_batch(x[s:s + 1])[0], full[s]), f"signal {s} depends on its batch"
    fresh = make_plan(F64, n, hop, amp=_ffi.AMP_POWER)
    fresh.reserve(nsig, x.shape[1])
    assert np.array_equal(fresh.compute_batch(x), full)
    del fresh, first
    w = np.asarray(plan.window(), np.float64)
    s, worst = nsig - 1, 0.0
    for f0 in range(0, nf, 64):  # (whole pairs per block)
        f1 = min(nf, f0 + 64)
        fr = windowed_frames(x[s, f0 * hop:(f1 - 1) * hop + n], w, n, hop, False, F64)
        A = np.abs(np.fft.rfft(fr, axis=-1)).T
        D = np.repeat(forward_delta(fr, n, F64), 2)[None, :f1 - f0]
        worst = max(worst, float(np.max(np.abs(full[s][:, f0:f1].astype(LD) - A * A) / (D * (2 * A + D)))))
    record("stft power, seam signal", F64, n, worst)
    assert worst <= 1.0, (n, worst)


@pytest.mark.gpu
def test_gpu_istft_across_a_chunk_seam():
    """istft_batch of the f64 NumPy spectrum of the first seam shape: every signal bit-equal to its own call, the seam signal within the
    overlap-added bound."""
    n, hop, nsig, nf = SEAMS[0]
    x = seam_input(*SEAMS[0])
    plan = make_plan(F64, n, hop)
    w = np.asarray(plan.window(), np.float64)
    S = np.ascontiguousarray(np.stack([np.fft.rfft(H.np_frames(r, n, hop, False) * w[None, :], axis=-1).T for r in x]))
    S[:, 0, :] = S[:, 0, :].real
    assert S.shape == (nsig, n // 2 + 1, nf) and S.dtype == np.complex128
    full = plan.istft_batch(S)
    assert plan.istft_kernel_name == "big+ola" and full.shape == x.shape
    for s in range(nsig):
        assert np.array_equal(plan.istft_batch(S[s:s + 1])[0], full[s]), f"signal {s} depends on its batch"
    y, e = ref_istft(S[nsig - 1:], w, n, hop, False, F64)
    ratio = istft_ratio(full[nsig - 1:], y, e, n, F64)
    record("istft, seam signal", F64, n, ratio)
    assert ratio <= 1.0, ratio
