"""The amplitude step that closes every spectrogram -- p, sqrt(p), 10 log10(max(p, eps)) -- held to ulps of its own power, route by route.

A power plan and a magnitude or dB plan with the same parameters run the same transform and the same bank sums; only the last step
differs.  So the GPU's own power output p (type T) is the exact input of the step under test and the transform's error drops out.
Every case builds AMP_POWER, AMP_MAGNITUDE and AMP_DECIBELS(floor) plans with identical parameters, runs them on one batch, asserts
`execute_kernel_name` (and, with a bank, `bank_stage_name`) equal on all of them and equal to the pinned route, and then checks, on
EVERY element:

  magnitude   mag == sqrt_T(p) bit for bit (numpy's f32 / f64 sqrt is correctly rounded, as sqrtf / sqrt are under hipcc's defaults).
  dB          eps_T = T(10^(floor / 10)) (f64 pow, then the cast: plan.hip `pl->eps = std::pow(10.0, floor_db / 10.0)`, `(T)a.eps` in
              the kernels);  v = p if p > eps_T else eps_T (a NaN p gives eps_T);  ref = 10 log10(v) in np.longdouble;
              |got - ref| <= bound;  v == 0 -> exactly -inf;  v == +inf -> exactly +inf.
  floor       all elements of one output with not (p > eps_T) are bit-identical; the all-zero row holds that one value everywhere.

Bounds (derived, not fitted; the threshold is 1 against them):
  f64         4e-15 + 3e-16 |ref|: db_f64.h's own contract (every f64 route calls it).
  f32         l = log2(v), K = 10 log10 2:  1.5 K spacing32(|l|) + 2^-24 |ref| + 0.5 spacing32(|ref|)
              (v_log_f32's 1 ulp plus the half ulp of the rescaling subtraction on the subnormal path; K rounded to f32; the multiply).
              `big_amp` (bigfft.hip) went through libm log10f and T(10) * before this file; it now runs the same log2 chain as every
              other f32 route (the comments beside the other helpers already said "as the other f32 kernels") and is held to this bound.
  slack_p     0; on a route listed in RELAXED (none) it would be (10 / ln 10) spacing_T(p) / p, and its magnitude within one spacing.

Inputs: one batch per case, rows sigma_b N(0, 1) drawn in T from a seeded default_rng: one all-zero row, sigma = 2^s for s = -70, -60
... +50 (f32) / -520, -510 ... +480 (f64) as far as (n_fft 6 sigma)^2 stays finite in T, one row of expected power 1, and on the
linear f32 routes one row at 2^62 whose re re + im im overflows (p = mag = dB = +inf; asserted to happen from n_fft 64 on, at n_fft
1, 4 and 6 the row's powers stay near 2^125).  That is 16 rows in f32 and 103 in f64.  The power output is asserted finite off that
row and exactly 0 on the zero row.  Frames per signal: two tiles plus one frame of the route (tile: tests/test_forward_readback.py
tile_of; the CQT tile 16 M from tests/test_cqt_transform.py lds_m), which runs interior, tail and partial store sites.  Two
exceptions, both from kernels_r32x16.hip want_pack: 2 tile + 1 frames leave (tile - 1) / (3 tile) >= 1 / 4 of the slots empty, which
is the packing threshold, so the one-signal tiles of k_r32x16 run 2 tile + tile / 2 + 1 frames (41 / 81) and the packed cases 5 (9
with a bank, as tests/test_bank_readback.py).  big_four_step / big_chirpz run 2 frames (their epilogue handles frames in pairs).
Floors: -80 and +30 on every case; on the cases marked extreme (at least one linear and one bank case per helper) also the floors
whose eps_T is subnormal (f32 -440, f64 -3200), zero (f32 -500, f64 -3300: the zero row is -inf) and, in f64, -3050.

Completeness: `grep -n "amp_f32<\\|amp_f64<\\|amp_e<\\|amp_apply(\\|t_db(\\|bs_db(\\|big_amp<\\|amp_t(\\|db2_f32\\|AMP_DB" csrc/*.hip` lists the
store sites; each sits behind one sgx_kernel_name (linear output) or one sgx_bank_stage_name (bank output), and the tables below hold
every name of tests/test_forward_readback.py's route list plus big_* and the three CQT names, and every name of
tests/test_bank_readback.py's NAMES less r32x16_sched_mfcc (its last step is the DCT).  test_gpu_every_route_was_seen asserts it.
Bank cases are that file's own (kernel, bank, stage) rows, imported: per stage name and type the Mel bank with the most bands
(reg_radix_csr and d32x32_sched have only ERB rows there: ERB-64 and ERB-129).  Gammatone, chroma and MFCC end in other steps and
keep their own files.

CPU part: the f32 chain (correctly rounded log2, x K in f32) and libm's f64 10 log10 restated in numpy pass the checker on the same
row recipe (worst ratio printed); seven planted faults each fail it.  `3.0103f`, the constant the issue names as a fault, IS the f32
nearest to 10 log10 2 (asserted), so the planted constant is the next shorter one, 3.010f.

Measured on MI355X (information, not thresholds; DESIGN.md 6.4 keeps the same table): worst |got - ref| / bound in dB and the
elements checked in dB, per route or stage name.  54 cases, 90 415 176 elements; every magnitude is sqrt_T(p) bit for bit, no route
is under the relaxed rule, every floor is one value:
    bank_rows              f32  0.606     76160    f64  0.517   2626500
    big_chirpz             f32  0.627    491640    f64  0.518   2110470
    big_four_step          f32  0.627   3932280    f64  0.518  16876550
    bluestein              f32  0.627    524160    f64  0.518   4217850
    bluestein_rows         f32  0.617    156000    f64
    cqt_mfma_global        f32  0.609    310464    f64   0.52   2855160
    cqt_mfma_lds           f32  0.618    975240    f64   0.52   3936660
    cqt_mfma_rows          f32  0.573     15120    f64  0.517     43260
    d32x16_f64             f32                     f64  0.518   8718435
    d32x16_sched           f32                     f64  0.516   2192355
    d32x32_f64             f32                     f64  0.517   8973875
    d32x32_sched           f32                     f64  0.518   1129395
    d512_f64               f32                     f64  0.518   8603075
    d512_sched             f32                     f64  0.519   4318275
    direct_dft             f32  0.594      1056    f64  0.499      6798
    generic_csr            f32  0.598      7920    f64  0.513     67980
    lds_radix2             f32  0.586      6336    f64  0.507     50985
    r32x16_csr             f32  0.625    492000    f64
    r32x16_f32             f32   0.63   2135456    f64
    r32x16_mfma            f32  0.605     41820    f64
    r32x16_sched           f32  0.622    314880    f64
    r32x16_sched512        f32  0.625    622080    f64
    r32x16_sched_packed    f32  0.628     69120    f64
    r32x32_f32             f32  0.626   2164800    f64
    r32x32_sched           f32   0.62    158400    f64
    r64x32_f32             f32  0.626   2089980    f64
    r64x32_sched           f32  0.613     76160    f64
    reg_radix              f32  0.628    954720    f64  0.518   4883745
    reg_radix_bands        f32  0.628    780000    f64  0.516   1751000
    reg_radix_csr          f32  0.623     65280    f64  0.516    560320
    two_factor_dft         f32  0.607      4224    f64  0.516     27192
On the CPU the restated chains sit at 0.45 (f32) and 0.66 (f64, libm) of the same bounds.
"""
import math

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests import test_bank_readback as BR
from tests import test_bigfft_lengths as BL
from tests import test_forward_readback as FR
from tests.test_cqt_transform import lds_m

F32, F64 = "float32", "float64"
NP = {F32: np.float32, F64: np.float64}
BITS = {F32: np.uint32, F64: np.uint64}
LD = np.longdouble
HOST = _ffi.DEVICE_HOST_ONLY
SR = 16000.0
POWER, MAGNITUDE, DB = _ffi.AMP_POWER, _ffi.AMP_MAGNITUDE, _ffi.AMP_DECIBELS
K_LD = LD(10) * np.log10(LD(2))
K32 = np.float32(3.01029995663981195)
FLOORS = (-80.0, 30.0)
EXTREME = {F32: (-440.0, -500.0), F64: (-3050.0, -3200.0, -3300.0)}
S_STEPS = {F32: range(-70, 51, 10), F64: range(-520, 481, 10)}
OVERFLOW_S = 62
RELAXED = {}  # route or stage name -> the line of code that contracts re re + im im differently per amplitude instance (none found)
WORST = {}
SEEN = set()

assert np.finfo(LD).nmant >= 63, "np.longdouble must be wider than f64: it is the reference"


# ---- restatements: eps_T, the floor rule, the reference and the bounds -----------------------------------------------------------
def eps_t(floor, dtype):
    """eps_T: 10^(floor / 10) in f64 (std::pow), then the cast to T (round to nearest, subnormals kept, 0 below them)."""
    return NP[dtype](math.pow(10.0, floor / 10.0))


def floored(p, eps):
    """max(p, eps) as the kernels take it: p where p > eps, else eps; a NaN p gives eps."""
    return np.where(p > eps, p, eps)


def db_ref(v):
    with np.errstate(divide="ignore"):
        return LD(10) * np.log10(v.astype(LD))


def spacing32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def db_bound(v, ref, dtype):
    """The bound of the docstring for finite v > 0 (type T) and ref = 10 log10 v (long double)."""
    aref = np.abs(ref).astype(np.float64)
    if dtype == F64:
        return 4e-15 + 3e-16 * aref
    return 1.5 * float(K_LD) * spacing32(np.log2(v.astype(LD))) + 2.0 ** -24 * aref + 0.5 * spacing32(aref)


def same_bits(a, b, dtype):
    return (a.view(BITS[dtype]) == b.view(BITS[dtype])) | (np.isnan(a) & np.isnan(b))


def check_magnitude(got, p, dtype, relaxed=False):
    """-> (failures, elements).  mag == sqrt_T(p) bit for bit; `relaxed`: within one spacing of it."""
    T = NP[dtype]
    assert got.dtype == T and p.dtype == T and got.shape == p.shape
    with np.errstate(invalid="ignore"):
        ref = np.sqrt(p)
    ok = same_bits(got, ref, dtype)
    if relaxed:
        with np.errstate(invalid="ignore"):
            ok |= np.abs(got - ref) <= np.spacing(ref)
    bad = np.argwhere(~ok)
    fails = [f"magnitude {tuple(i)}: got {got[tuple(i)]!r}, sqrt_T(p) {ref[tuple(i)]!r}, p {p[tuple(i)]!r}" for i in bad[:3]]
    if len(bad):
        fails.insert(0, f"{len(bad)} of {got.size} magnitudes are not sqrt_T(p)")
    return fails, got.size


def check_db(got, p, floor, dtype, relaxed=False):
    """-> (failures, worst ratio to the bound over the finite elements, elements)."""
    T = NP[dtype]
    assert got.dtype == T and p.dtype == T and got.shape == p.shape
    eps = eps_t(floor, dtype)
    with np.errstate(invalid="ignore"):
        v = floored(p, eps).astype(T)
        at_floor = ~(p > eps)
    fails = []
    zero, inf = v == 0, np.isposinf(v)
    if not np.all(got[zero] == -np.inf):
        fails.append(f"floor {floor}: {int(np.sum(got[zero] != -np.inf))} of {int(zero.sum())} elements with v == 0 are not -inf")
    if not np.all(got[inf] == np.inf):
        fails.append(f"floor {floor}: {int(np.sum(got[inf] != np.inf))} of {int(inf.sum())} elements with v == +inf are not +inf")
    fin = ~(zero | inf)
    vf, gf = v[fin], got[fin]
    ref = db_ref(vf)
    bound = db_bound(vf, ref, dtype)
    if relaxed:
        bound = bound + (10.0 / math.log(10.0)) * (np.spacing(vf).astype(np.float64) / vf.astype(np.float64))
    with np.errstate(invalid="ignore"):
        err = np.abs(gf.astype(LD) - ref).astype(np.float64)
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isfinite(gf), ratio, np.inf)  # (a NaN or an infinity where the reference is finite)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        i = int(np.argmax(ratio))
        fails.append(f"floor {floor}: {int(np.sum(ratio > 1.0))} of {ratio.size} over the bound, worst {worst:.3g} x: v {vf[i]!r} got {gf[i]!r} "
                     f"ref {float(ref[i])!r} bound {bound[i]:.3g}")
    fl = got[at_floor]
    if fl.size and not np.all(same_bits(fl, np.full_like(fl, fl.flat[0]), dtype)):
        fails.append(f"floor {floor}: the {fl.size} elements at the floor hold {np.unique(fl).size} different values")
    return fails, worst, got.size


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def sigma_steps(dtype, n_fft):
    """The s of sigma = 2^s for which (n_fft 6 sigma)^2 stays finite in T."""
    top = 128 if dtype == F32 else 1024
    return [s for s in S_STEPS[dtype] if 2.0 * (math.log2(6.0 * n_fft) + s) < top]


def make_rows(dtype, n_fft, n, unit, overflow=False, reps=1, seed=5):
    """-> (x [rows, n] in T, indices of the zero rows, indices of the overflow rows).  One block is: the zero row, the 2^s rows in
    ascending order (the zero row's only neighbour is the smallest sigma), the unit-power row, the overflow row."""
    T = NP[dtype]
    sig = [0.0] + [2.0 ** s for s in sigma_steps(dtype, n_fft)] + [float(unit)] + ([2.0 ** OVERFLOW_S] if overflow else [])
    sig = np.asarray(sig * reps, T)
    assert np.all(np.isfinite(sig))
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((sig.size, n), dtype=T) * sig[:, None]
    assert x.dtype == T and np.all(np.isfinite(x))
    block = sig.size // reps
    zero = [r * block for r in range(reps)]
    over = [r * block + block - 1 for r in range(reps)] if overflow else []
    return x, zero, over


# ---- cases -------------------------------------------------------------------------------------------------------------------------
class Case:
    """kind: linear | bank | cqt | cqt_transform.  `route` is sgx_execute_kernel_name's text, `stage` sgx_bank_stage_name's."""

    def __init__(self, kind, dtype, n_fft, hop, nf, route, stage="", bank=None, cq=None, extreme=False, overflow=False, set_route=0,
                 tag=""):
        self.kind, self.dtype, self.n_fft, self.hop, self.nf, self.route, self.stage = kind, dtype, n_fft, hop, nf, route, stage
        self.bank, self.cq, self.extreme, self.overflow, self.set_route, self.tag = bank, cq, extreme, overflow, set_route, tag

    @property
    def id(self):
        b = "-" + "-".join(str(int(v) if isinstance(v, float) else v) for v in self.bank) if self.bank else ""
        return f"{self.kind}-{self.stage or self.route}-{self.dtype[5:]}-{self.n_fft}-{self.hop}{b}@{self.nf}{self.tag}"

    @property
    def name(self):
        return self.stage or self.route

    def floors(self):
        return FLOORS + (EXTREME[self.dtype] if self.extreme else ())

    def n_samples(self):
        if self.kind == "cqt_transform":
            return self.n_fft + (self.nf - 1) * self.hop
        # centred: (n + 2 (n_fft // 2) - n_fft) // hop + 1 frames; one sample past the last hop unless the hop is 1
        return (self.nf - 1) * self.hop + self.n_fft % 2 + min(1, self.hop - 1)

    def plan(self, amp, floor=None, device=_ffi.DEVICE_CURRENT):
        db = sg.LogParams(floor) if amp == DB else None
        if self.kind == "cqt_transform":
            p = sg.CqtTransformPlan(SR, self.n_fft, self.hop, self.cq, amp, db, self.dtype, device)
            if self.set_route:
                p.set_route(self.set_route)
            return p
        if self.kind == "bank":
            params = sg.SpectrogramParams(sg.StftParams(self.n_fft, self.hop, sg.WindowType.hanning, True), BR.bank_sr(self.bank))
            return sg.Plan(params, amp, BR.bank_params(self.bank), db, self.dtype, device=device)
        window = sg.WindowType.hanning if self.kind == "cqt" else sg.WindowType.rectangular
        params = sg.SpectrogramParams(sg.StftParams(self.n_fft, self.hop, window, True), SR)
        return sg.Plan(params, amp, self.cq, db, self.dtype, device=device)

    def unit_sigma(self):
        """sigma of the row whose expected power is 1 (the median row or bin for a bank or a CQT)."""
        host = self.plan(POWER, device=HOST)
        if self.kind == "linear":
            return 1.0 / math.sqrt(self.n_fft)  # rectangular window: E |X_k|^2 = n_fft sigma^2
        if self.kind == "bank":
            w2 = float(np.sum(host.window() ** 2))
            rs = BR.table_dense(host, self.n_fft // 2 + 1).sum(axis=1)
            return 1.0 / math.sqrt(w2 * float(np.median(rs[rs > 0])))
        e = [float(np.sum(np.abs(k) ** 2)) for k in host.cqt_kernels()]
        if self.kind == "cqt":  # the STFT window multiplies the frame first
            e = [v * float(np.mean(host.window() ** 2)) for v in e]
        return 1.0 / math.sqrt(float(np.median(e)))

    def batch(self):
        reps = -(-33 // (len(sigma_steps(self.dtype, self.n_fft)) + 2)) if self.set_route == 2 else 1  # rows tiles: 16 signals each
        return make_rows(self.dtype, self.n_fft, self.n_samples(), self.unit_sigma(), self.overflow, reps)


def r32x16_frames(n_fft, packed):
    tile = 16 if n_fft == 1024 else 32
    return 5 if packed else 2 * tile + tile // 2 + 1


def linear_case(dtype, n_fft, hop, route, var="", extreme=False, packed=False, nf=None):
    if nf is None:
        nf = r32x16_frames(n_fft, packed) if route == "r32x16_f32" else 2 * FR.tile_of((dtype, n_fft, hop, var, route)) + 1
    return Case("linear", dtype, n_fft, hop, nf, route, extreme=extreme, overflow=dtype == F32, tag="-packed" if packed else "")


BIG = {("big_four_step", F32): 65536, ("big_four_step", F64): 32768, ("big_chirpz", F32): 8193, ("big_chirpz", F64): 4097}
SMALLEST = {"direct_dft": 1, "lds_radix2": 4, "two_factor_dft": 6}  # the smallest n_fft that selects each, both types

LINEAR = [
    linear_case(F32, 1024, 256, "r32x16_f32", extreme=True),
    linear_case(F32, 512, 128, "r32x16_f32"),
    linear_case(F32, 1024, 256, "r32x16_f32", packed=True),
    linear_case(F32, 512, 128, "r32x16_f32", packed=True),
    linear_case(F32, 2048, 512, "r32x32_f32", extreme=True),
    linear_case(F32, 4096, 1024, "r64x32_f32", extreme=True),
    linear_case(F64, 1024, 256, "d32x16_f64", extreme=True),
    linear_case(F64, 512, 160, "d512_f64", extreme=True),
    linear_case(F64, 2048, 512, "d32x32_f64", extreme=True),
    *[linear_case(d, 256, 64, "reg_radix", extreme=True) for d in (F32, F64)],
    *[linear_case(d, 400, 100, "reg_radix") for d in (F32, F64)],
    *[linear_case(d, n, max(1, n // 4), name, extreme=name == "lds_radix2") for name, n in sorted(SMALLEST.items()) for d in (F32, F64)],
    *[linear_case(d, 251, 62, "bluestein", extreme=True) for d in (F32, F64)],
    *[linear_case(d, n, n // 4, name, extreme=True, nf=2) for (name, d), n in sorted(BIG.items())],
]


def bank_frames(kernel, dtype, n_fft, hop, stage):
    if stage == "r32x16_sched_packed":
        return BR.NFRAMES
    if kernel == "r32x16_f32":
        return r32x16_frames(n_fft, False)
    if kernel.startswith("big_"):
        return 2
    return 2 * FR.tile_of((dtype, n_fft, hop, "", kernel)) + 1


def bank_cases():
    """Per (stage name, type) of tests/test_bank_readback.py's CASES: its Mel row with the most bands (any other bank if it has no Mel)."""
    best = {}
    for dtype, n_fft, hop, bank, out, kernel, stage in BR.CASES:
        base, suffix = BR.split_stage(stage)
        if suffix or base == "r32x16_sched_mfcc" or bank[0] == "chroma" or BR.split_out(out)[0] not in ("power", "magnitude", "db"):
            continue
        if kernel == "d512_f64" and base != "d512_sched":  # (that file's 9-frame step down; here d512 plans run full tiles)
            continue
        rank = (bank[0] == "mel", bank[1])
        if (base, dtype) not in best or rank > best[base, dtype][0]:
            best[base, dtype] = (rank, Case("bank", dtype, n_fft, hop, bank_frames(kernel, dtype, n_fft, hop, base), kernel, base, bank=bank,
                                            extreme=True))
    return [best[k][1] for k in sorted(best)]


BANK = bank_cases()

MUSICAL, DEEP = sg.CqtParams.musical(), sg.CqtParams(12, 7, 32.7)  # L_0 = 489 of 1024 / 4096 of 4096 (capped)


def cqt_tile(case):
    """16 M frames (cqt.hip k_cqt: F = 16 M; M = cqt_lds_m, 1 on the global and rows routes)."""
    L0 = len(case.plan(POWER, device=HOST).cqt_kernels()[0])
    return 16 * max(lds_m(case.hop, -(-L0 // 16) * 16, 4 if case.dtype == F32 else 8), 1)


def cqt_cases():
    out = []
    for d in (F32, F64):
        for kind in ("cqt", "cqt_transform"):
            for cq, n_fft, hop, route in ((MUSICAL, 1024, 256, "cqt_mfma_lds"), (DEEP, 4096, 2500, "cqt_mfma_global")):
                c = Case(kind, d, n_fft, hop, 1, route, cq=cq, extreme=kind == "cqt" or route == "cqt_mfma_global")
                c.nf = 2 * cqt_tile(c) + 1
                out.append(c)
        out.append(Case("cqt_transform", d, 1024, 256, 1, "cqt_mfma_rows", cq=MUSICAL, extreme=True, set_route=2))
    return out


CQT = cqt_cases()
CASES = LINEAR + BANK + CQT


# ---- CPU: the table ------------------------------------------------------------------------------------------------------------
def test_case_ids_are_unique_and_every_name_is_covered():
    assert len({c.id for c in CASES}) == len(CASES)
    assert {c.stage for c in BANK} == BR.NAMES - {"r32x16_sched_mfcc"}
    assert all(c.bank[0] == "mel" for c in BANK if c.stage not in ("reg_radix_csr", "d32x32_sched"))  # (no Mel row on those two there)
    on_chip = {r[4] for r in FR.ROUTES}
    assert {c.route for c in LINEAR} == on_chip | {"big_four_step", "big_chirpz"}
    assert {c.route for c in CQT} == {"cqt_mfma_lds", "cqt_mfma_global", "cqt_mfma_rows"}
    for helper_routes in (("r32x16_f32",), ("r32x32_f32",), ("r64x32_f32",), ("d32x16_f64", "d512_f64"), ("d32x32_f64",),
                          ("reg_radix", "lds_radix2", "two_factor_dft", "direct_dft"), ("bluestein",), ("big_four_step", "big_chirpz")):
        for d in (F32, F64):
            mine = [c for c in LINEAR if c.route in helper_routes and c.dtype == d]
            assert not mine or any(c.extreme for c in mine), (helper_routes, d)  # the extreme floors reach every helper in every type it has
    assert all(c.extreme for c in BANK)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_table_selects_the_named_route(case):
    """Host-only plans, wherever the plan alone determines the route (cqt_mfma_rows is chosen per call; a bank's stage too)."""
    want = "cqt_mfma_lds" if case.route == "cqt_mfma_rows" else case.route
    for amp in (POWER, MAGNITUDE, DB):
        plan = case.plan(amp, -80.0, device=HOST)
        assert plan.kernel_name == want and plan.execute_kernel_name == "" and plan.bank_stage_name == ""
    nb, nf = case.plan(POWER, device=HOST).output_shape(case.n_samples())
    assert nf == case.nf
    if case.kind == "linear":
        assert nb == case.n_fft // 2 + 1
        listed = [r for r in FR.ROUTES if r[:3] == (case.dtype, case.n_fft, case.hop)]
        assert all(r[4] == case.route for r in listed)  # the read-back file's table pins the same name
        if case.route in FR.STEP_DOWN:
            assert case.nf >= FR.STEP_DOWN[case.route]  # (fewer frames per signal would step down to k_reg_radix)
        if case.route.startswith("big_"):
            assert BL.expected_route(case.dtype, BL.big_m(case.n_fft), case.n_fft) == case.route and (case.dtype, BL.big_m(case.n_fft), case.n_fft) in BL.BIG
            assert case.n_fft == min(n for d, _, n in BL.BIG if d == case.dtype and BL.form_of(n) == BL.form_of(case.n_fft))
    if case.kind == "bank":
        assert any(r[0] == case.dtype and r[1:4] == (case.n_fft, case.hop, case.bank) and r[5:] == (case.route, case.stage) for r in BR.CASES)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_smallest_lengths_of_the_generic_routes(dtype):
    first = {}
    for n in range(1, 40):
        params = sg.SpectrogramParams(sg.StftParams(n, max(1, n // 4), sg.WindowType.rectangular, True), SR)
        first.setdefault(sg.Plan(params, POWER, None, None, dtype, device=HOST).kernel_name, n)
    assert {k: first[k] for k in SMALLEST} == SMALLEST


def test_r32x16_frame_counts_sit_on_the_intended_side_of_want_pack():
    """kernels_r32x16.hip want_pack restated: packed when (slots - used) 4 >= slots."""
    def packs(n_fft, nf):
        ft = 16 if n_fft == 1024 else 32
        slots = -(-nf // ft) * ft
        used = 2 * ((nf + 1) // 2) if n_fft == 512 else nf
        return (slots - used) * 4 >= slots
    for n_fft in (1024, 512):
        ft = 16 if n_fft == 1024 else 32
        assert packs(n_fft, 2 * ft + 1) and packs(n_fft, r32x16_frames(n_fft, True)) and not packs(n_fft, r32x16_frames(n_fft, False))
        assert r32x16_frames(n_fft, False) > 2 * ft and r32x16_frames(n_fft, False) % ft  # two whole tiles and a tail
    assert packs(1024, BR.NFRAMES)


def test_restatements_of_eps_and_the_floor_rule():
    assert eps_t(-80.0, F32) == np.float32(1e-8) and eps_t(30.0, F64) == 1000.0
    e = eps_t(-440.0, F32)
    assert e.dtype == np.float32 and 0 < e < np.finfo(np.float32).tiny and e == np.float32(7 * 2.0 ** -149) and float(e) != 1e-44
    assert eps_t(-500.0, F32) == 0 and eps_t(-3300.0, F64) == 0
    assert 0 < eps_t(-3200.0, F64) < np.finfo(np.float64).tiny <= eps_t(-3050.0, F64)
    p = np.array([np.nan, 0.0, 1e-9, 1e-8, 2e-8, np.inf], np.float32)
    with np.errstate(invalid="ignore"):
        v = floored(p, eps_t(-80.0, F32))
    assert v.dtype == np.float32 and np.array_equal(v, np.array([1e-8, 1e-8, 1e-8, 1e-8, 2e-8, np.inf], np.float32))
    assert np.float32(3.0103) == K32  # the "shortened" constant of the issue is the very same f32: see test_planted_faults


# ---- CPU: checker and bounds ---------------------------------------------------------------------------------------------------
def cpu_powers(dtype, n_fft=256, hop=64, nf=9):
    """Powers in T with the GPU cases' distribution: the linear row recipe through numpy's rfft, re re + im im in T."""
    x, zero, over = make_rows(dtype, n_fft, BR.n_samples(hop, nf), 1.0 / math.sqrt(n_fft), overflow=dtype == F32)
    fr = np.stack([BR.H.np_frames(r, n_fft, hop, True) for r in x.astype(np.float64)])
    X = np.fft.rfft(fr, axis=-1)
    T = NP[dtype]
    with np.errstate(over="ignore", under="ignore"):
        re, im = X.real.astype(T), X.imag.astype(T)
        p = re * re + im * im
    assert p.dtype == T and np.all(p[zero] == 0) and (not over or np.isinf(p[over]).any())
    return p


def chain_f32(v, k=K32, ulps=0):
    """The f32 routes: log2 correctly rounded (or moved by `ulps`), times K in f32."""
    with np.errstate(divide="ignore"):
        l = np.log2(v.astype(LD)).astype(np.float32)
    if ulps:
        l = np.where(np.isfinite(l), l + np.float32(ulps) * np.spacing(np.abs(l)), l).astype(np.float32)
    return (l * k).astype(np.float32)


def chain_f64(v):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(v)


def restated(p, floor, dtype):
    with np.errstate(invalid="ignore"):
        v = floored(p, eps_t(floor, dtype))
    return chain_f32(v) if dtype == F32 else chain_f64(v)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_restated_chains_meet_the_bounds(dtype):
    p = cpu_powers(dtype)
    tiny = np.finfo(NP[dtype]).tiny
    assert np.any(p == 0) and np.any((p > 0) & (p < tiny)) and np.any(p > 1) and np.any((p > 0.5) & (p < 2))
    for floor in FLOORS + EXTREME[dtype]:
        got = restated(p, floor, dtype)
        fails, worst, n = check_db(got, p, floor, dtype)
        print(f"restated {dtype} chain, floor {floor}: worst ratio to the bound {worst:.3g} over {n} elements")
        assert not fails and 0.01 < worst <= 1.0, (floor, fails, worst)
        if eps_t(floor, dtype) == 0:
            assert np.all(got[0] == -np.inf)  # the zero row
    fails, _ = check_magnitude(np.sqrt(p), p, dtype)
    assert not fails


def test_planted_faults_fail_the_checker():
    p32, p64 = cpu_powers(F32), cpu_powers(F64)

    def v_of(p, floor, dtype):
        with np.errstate(invalid="ignore"):
            return floored(p, eps_t(floor, dtype))

    def fails(got, p, floor, dtype):
        return bool(check_db(got.astype(NP[dtype]), p, floor, dtype)[0])

    assert not fails(chain_f32(v_of(p32, -80.0, F32)), p32, -80.0, F32)
    # K shortened (3.0103f is K itself: test_restatements_of_eps_and_the_floor_rule)
    assert fails(chain_f32(v_of(p32, -80.0, F32), k=np.float32(3.010)), p32, -80.0, F32)
    # log2 moved by 3 ulp
    assert fails(chain_f32(v_of(p32, -80.0, F32), ulps=3), p32, -80.0, F32)
    # subnormal v flushed to zero before the logarithm
    v = v_of(p32, -440.0, F32)
    assert np.any((v > 0) & (v < np.finfo(np.float32).tiny))
    assert not fails(chain_f32(v), p32, -440.0, F32)
    assert fails(chain_f32(np.where(v < np.finfo(np.float32).tiny, np.float32(0), v)), p32, -440.0, F32)
    # p + eps in place of max
    assert fails(chain_f32(p32 + eps_t(-80.0, F32)), p32, -80.0, F32)
    # eps taken in f64 where T is f32, at floor -440
    with np.errstate(invalid="ignore"):
        v64 = np.where(p32.astype(np.float64) > 1e-44, p32.astype(np.float64), 1e-44)
    with np.errstate(divide="ignore"):
        got = (np.log2(v64.astype(LD)).astype(np.float32) * K32).astype(np.float32)
    assert fails(got, p32, -440.0, F32)
    # f64 output perturbed by 2e-14 dB near 0 dB
    got = chain_f64(v_of(p64, -80.0, F64))
    assert not fails(got, p64, -80.0, F64)
    near = np.argwhere(np.abs(got) < 1.0)
    assert len(near)
    bad = got.copy()
    bad[tuple(near[0])] += 2e-14
    assert fails(bad, p64, -80.0, F64)
    # one element at the floor that differs from the others in its last bit
    bad = got.copy()
    at = np.argwhere(~(p64 > eps_t(-80.0, F64)))
    bad[tuple(at[1])] = np.nextafter(bad[tuple(at[1])], 0.0)
    assert fails(bad, p64, -80.0, F64)
    # magnitude off by one spacing
    for p, d in ((p32, F32), (p64, F64)):
        m = np.sqrt(p)
        assert not check_magnitude(m, p, d)[0]
        i = tuple(np.argwhere(np.isfinite(m) & (m > 0))[0])
        m[i] = np.nextafter(m[i], np.inf)
        assert check_magnitude(m, p, d)[0] and not check_magnitude(m, p, d, relaxed=True)[0]


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def record(case, what, value, count=0):
    w = WORST.setdefault((case.name, case.dtype), {"db": 0.0, "count": 0, "relaxed": case.name in RELAXED})
    w[what] = max(w.get(what, 0.0), value)
    w["count"] += count


def run_plan(case, amp, x, floor=None):
    plan = case.plan(amp, floor)
    got = np.array(plan.compute_batch(x))
    return got, plan.execute_kernel_name, plan.bank_stage_name


def transform_power(case, x):
    """A transform plan's own AMP_COMPLEX output -> re re + im im, each product and the sum rounded in T (cqt.py CqtResult.to_power)."""
    z, route, _ = run_plan(case, _ffi.AMP_COMPLEX, x)
    re, im = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
    assert re.dtype == NP[case.dtype]
    with np.errstate(over="ignore", under="ignore"):
        return re * re + im * im, route


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_gpu_magnitude_and_db_are_ulps_from_the_route_own_power(case):
    x, zero, over = case.batch()
    relaxed = case.name in RELAXED
    p, route, stage = run_plan(case, POWER, x)
    assert (route, stage) == (case.route, case.stage), (route, stage)
    assert p.dtype == NP[case.dtype] and p.shape[0] == x.shape[0] and p.shape[2] == case.nf
    quiet = np.ones(x.shape[0], bool)
    quiet[over] = False
    assert np.all(np.isfinite(p[quiet])) and np.all(p[zero] == 0), "the power output is not finite off the overflow row and 0 on the zero row"
    if over and case.n_fft >= 64:  # E |X_k|^2 = n_fft 2^124 >= 4 x 2^128; at n_fft 1, 4 and 6 the row's powers stay finite (about 2^125)
        assert np.isinf(p[over]).any()
    tiny = np.finfo(NP[case.dtype]).tiny
    print(f"{case.id}: {p.size} powers, {int(np.sum(p == 0))} zero, {int(np.sum((p > 0) & (p < tiny)))} subnormal, {int(np.isinf(p).sum())} inf")
    if case.kind == "cqt_transform":
        pz, zroute = transform_power(case, x)
        assert zroute == route and np.all(same_bits(p, pz, case.dtype)), "power is not re re + im im of the plan's own complex output, rounded in T"
    fails = []
    mag, mroute, mstage = run_plan(case, MAGNITUDE, x)
    assert (mroute, mstage) == (route, stage)
    f, n = check_magnitude(mag, p, case.dtype, relaxed)
    fails += f
    for floor in case.floors():
        db, droute, dstage = run_plan(case, DB, x, floor)
        assert (droute, dstage) == (route, stage)
        f, worst, n = check_db(db, p, floor, case.dtype, relaxed)
        print(f"{case.id} floor {floor}: worst ratio to the bound {worst:.3g} over {n} elements")
        record(case, "db", worst if np.isfinite(worst) else 1e30, n)
        fails += f
        eps = eps_t(floor, case.dtype)
        want = -np.inf if eps == 0 else None
        zr = db[zero]
        assert np.all(same_bits(zr, np.full_like(zr, zr.flat[0]), case.dtype)) and (want is None or zr.flat[0] == want), "the zero row is not one value"
    SEEN.add(case.name)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_gpu_every_route_was_seen():
    """Runs last: prints the worst ratio per route or stage name and type; every name of the tables was met by a passing case."""
    for (name, dtype), w in sorted(WORST.items()):
        print(f"{name:22s} {dtype}: dB worst ratio {w['db']:.3g}, {w['count']} elements{', relaxed magnitude' if w['relaxed'] else ''}")
    assert SEEN >= {c.name for c in CASES}
