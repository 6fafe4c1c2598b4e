"""The forward STFT's matrix M[j, k] = w[j] exp(-2 pi i j k / N), read back entry by entry through every on-chip route.

A frame that holds one unit sample at row j comes out as row j of that matrix: every bin at full scale |w[j]|, and nothing else in
the transform but exact zeros, so each output is the sample times the window and the chain of twiddle products of its path.  The
normwise checks (tests/test_gpu_parity.py: 2e-5 of the batch's peak, 1e-10 in f64; tests/test_frame_locality.py and
tests/test_tile_walks.py: 4 u log2(N) sqrt(N) ||x_f w||_2 per frame) let one entry that is wrong by a relative 1e-3 pass; here every
entry has its own bound of a few ulp.  `big_four_step` and `big_chirpz` stay with tests/test_bigfft_lengths.py (section 3 there reads
their matrix the same way); the CQT names have tests/test_cqt_readback.py.

1. ROUTES: (dtype, n_fft, hop, variant, kernel name), the name asserted on the host-only plan and again on the device plan.
   Variants: "staged" (the tile's samples go through LDS), "direct" (per-lane loads: hop above the staging limit; for k_reg_radix
   see below), "odd" (odd hop), "paired ..." (two frames per complex transform, `paired()` of tests/test_frame_locality.py), "short".
   "short": signals of fewer frames than the tuned kernel's geometry takes (STEP_DOWN below) leave it for k_reg_radix PER CALL
   (plan.hip run_device -> resolve_geometry); `kernel_name` keeps reporting the plan's kernel, so the name column holds the tuned name
   and the case runs k_reg_radix's instance for that length.  That is the only way f32 (16, 8, 8), f32 (16, 16, 8) and f64 (8, 8, 8)
   are reached since every hop at those lengths resolves to a tuned kernel, and the only way the staged f64 variant is (below).
   Nothing observable confirms that a short call ran k_reg_radix: the coverage of those instances rests on reading
   resolve_geometry (n_frames is the count per signal; tuned -> K_REG_RADIX is the first step down) and the geometry lines that
   test_routes_reach_every_on_chip_forward_kernel_name pins.  The same thresholds bound the other way: a case meant for
   d32x16_f64 / d512_f64 / r32x32_f32 needs at least 8 / 16 / 5 frames per signal or it silently measures k_reg_radix instead, so pass
   A runs those routes with that many frames (frames_a), not with 4.
   Every (A, B, C) of SGX_RR_SPLITS_F32 / _F64 / _MIXED (reg_radix.h, parsed on the CPU) is reached per element type or listed in
   UNREACHABLE with its reason; `reg_split_len` is restated here.  For k_reg_radix nothing reports which of the staged / direct
   variants ran, so plan_geometry_reg_radix is restated too (reg_radix_geometry: the budget loop over reg_radix_bytes from
   reg_radix_ft_max down, reg_radix_want_staged, 2 hop <= n_fft, reg_radix_stage_ok at the tile the budget allows) and the CPU route
   test asserts that every "staged" case stages and every "direct" one does not.  f32 stages at most lengths; f32 n_fft 8192 never
   does (one frame with its tables is 81 936 bytes, above kRegBudgetBins: the geometry falls through to one frame, direct).  In f64
   only A >= 16 with C > 1 can stage: (16, 16, 8) never does (one frame of 4096 doubles is already 2048 chunks, the tile the budget
   allows holds 2 frames), (16, 16, 16) is unreachable, and plans of n_fft 2048 keep every hop that could stage for k_d32x32, so
   k_reg_radix<double, 16, 8, 8, staged> is reached only by the short calls of such a plan: the d32x32_f64 "short" case.
   (At n_fft 2048 in f32 an odd hop runs k_r32x32 these days, plan_geometry_r32x32_f32: it is a case of that kernel.)

2. Inputs.  Window: WindowType.custom(w), no normalisation, w[j] = 0.5 + q_j / 2048, q_j seeded integers in [0, 1024) with q_j != q_(j-1)
   and q_j != q_(N-1-j): asymmetric, no zero, neighbours (hence both entries of a pair (2i, 2i+1)) distinct, w and w / 2 exact in f32, so
   x w is exact and the only roundings are the transform's.
   Pass A (centre = False): signal r = 0 ... N - 1 is 1 at every t = r mod N, length N + (F_A - 1) hop; frame f holds one impulse at row
   (r - f hop) mod N, so every frame slot reads every row.  F_A = 4 for N <= 1024, else 2, raised to the tuned kernel's own minimum.
   Residues go in chunks of at most 2^23 output entries.
   Pass B (centre = True): the same trains for 16 residues (0, 1, N/2 - 1, N/2, N - 1, seeded others), 2 x tile + 1 frames per signal
   (tile: the route's frames per tile, TILE / reg_radix_geometry, checked against the geometry functions' own lines on the CPU; the
   largest the kernel can take where its geometry picks by LDS budget), length no multiple of the hop.  A frame whose impulse falls
   into the virtual zero padding is all zero.  r32x16 and bluestein, whose tiles run on into the next signal, also run 5 frames per
   signal.  "short" cases keep below their threshold.

3. Reference and bounds.  ref[j, k] = w[j] exp(-2 pi i ((j k) mod N) / N), the exponent reduced in integers; f64 for f32 plans, long
   double for f64 plans (the import-time assertion of tests/test_bigfft_lengths.py keeps long double honest).  u = 2^-24 / 2^-53 and
   c = 4 are those of tests/test_bigfft_lengths.py and tests/test_frame_locality.py.
     complex, per entry       |X_f[k] - ref[j, k]| <= 4 u (S + 2) W_f
     complex, bluestein       per frame pair  max_k |dX| <= sqrt(sum_k |dX|^2) <= 12 u log2(M) sqrt(M) W_f  (both asserted)
     power                    |P - |ref|^2| <= d (2 |ref| + d), d the complex bound of that entry
   W_f = |w_j|; on the pairing routes |w_a| + |w_b| of the pair's two rows (an absent or all-zero partner counts 0).  A frame whose W_f
   is 0 (all zero, and so is its partner if it has one) has the bound 0: complex and power must be exactly 0 there.  An all-zero frame
   whose partner is live is NOT exactly zero on a pairing route (Z[k] and conj Z[N - k] come from different paths) and gets the pair's bound.
   No entry is masked or skipped.
   S = the largest number of rounded complex products on a path from a sample to a bin, counted from the code; + 2 = the real split's
   table entry and sum.  In an impulse frame every butterfly has one zero input, so a stage is one product or none:
     inreg(P)   Fft<P> (fft_inreg.h:34-65): the combs of 2 and 4 points multiply by 1 and -i only (idx 0, 16); from 8 points on every
                comb has a rounded constant: max(log2 P - 2, 0).  MixFft<N> (fft_inreg.h:171-206), N = P Q, P = 5 or 3: dft5 / dft3
                (one product with rounded constants), cmul_wn<N, k1 n2> unless Q = 1, then MixFft<Q>.
     chain(P)   rr_twiddle (reg_radix.h:25-36): one table entry per set bit of the index, multiplied together and onto the value:
                max popcount(k), k < P factors.
     route              S                          counted from
     r32x16_f32         3 + 2 + 2 = 7              kernels_r32x16.hip:1213-1219 (Fft<16> x 2 + Comb<32>); :242-243 (twb, twa; n_fft 1024:
                                                   :240 and :291-292, row 0 twice); :314-315 / :412-413 (Fft<16>)
     r32x32_f32         3 + 2 + 1 + 2 = 8          kernels_r32x32.hip:255-260; :272-273; :108 (cmul_wn<32>); :113 / :117 (Fft<16>)
     r64x32_f32         3 + 2 + 1 + 3 = 9          kernels_r64x32.hip:183-194; :204-205; :227 / :231 (W_64^n); :239 (Fft<32>)
     d32x16_f64         2 + 2 + 1 + 2 = 7          kernels_d32x16.hip:213-224 (Fft<8> x 2 + Comb<16>); :235-236; :260 (W_32^n); :267 (Fft<16>)
     d512_f64           2 + 2 + 1 + 2 = 7          kernels_d32x16.hip:469-477; :487-488; :509; :516
     d32x32_f64         1 + 2 + 2 + 1 + 2 = 8      kernels_d32x32.hip:194 (W_32^n1); :199 (Fft<16>); :209-210 (twl, twm); :231; :238
     reg_radix A B C    inreg(A) + chain(A) + inreg(B) [+ chain(B) + inreg(C) if C > 1]
                                                   kernels_generic.hip:507 / :530 (MixFft<A>); :479; :550; :560; :577
     lds_radix2         max(log2(n_fft / 2) - 1, 0)  kernels_generic.hip:191 (h = 1: W = 1); :207-218 (every later stage reads the table)
     two_factor_dft     3                          kernels_generic.hip:775-776 (sum); :781 (W_n^(n2 k1)); :792-793 (sum)
     direct_dft         1                          kernels_generic.hip:720-721

4. The checker can fail (CPU): on torch.fft.rfft in the plan's type of the same frames (S = ceil(log2 N)) the clean output passes, and
   each planted fault fails: one entry moved by 64 ulp, the window reversed / shifted by one / pair-swapped, one row's twiddles rounded
   through f32 in an f64 output, frames 2p and 2p + 1 swapped, one bin taken from the neighbouring frame, one denormal in a zero frame.
   The older criteria, restated, let the 64-ulp fault through in both types.  The through-f32 row is about 3e-8 of its sample: the f64
   parity criterion is absolute (1e-10 max(1, max |ref|)), so it catches that row at full scale and lets it through as soon as the
   frame is 2^-10 of full scale (an exact scaling of input and output; asserted), while the entry bound, which scales with the frame,
   fails it by the same factor at either level.  GUARD32 passes it at both.  The f64 per-frame bound of tests/test_frame_locality.py
   scales as well and does catch such a row; the test prints those figures.

5. Every GPU case records its worst ratio to the bound; test_gpu_worst_ratios_per_route prints the table.  Measured on an MI355X
   (information, not thresholds; DESIGN.md 6.2 keeps the same table):
     | kernel                         | f32 complex | f32 power | f64 complex | f64 power |
     | r32x16_f32 (n_fft 1024, 512)   | 0.158       | 0.163     |             |           |
     | r32x32_f32                     | 0.217       | 0.210     |             |           |
     | r64x32_f32                     | 0.208       | 0.204     |             |           |
     | d32x16_f64                     |             |           | 0.365       | 0.259     |
     | d512_f64                       |             |           | 0.288       | 0.168     |
     | d32x32_f64                     |             |           | 0.437       | 0.336     |
     | reg_radix (57 instances)       | 0.250       | 0.158     | 0.394       | 0.202     |
     | reg_radix, short calls         | 0.175       |           | 0.212       |           |
     | lds_radix2                     | 0.114       |           | 0.347       |           |
     | two_factor_dft                 | 0.0975      |           | 0.453       |           |
     | direct_dft                     | 0.104       |           | 0.889       |           |
     | bluestein (its normwise bound) | 0.0161      | 0.0015    | 0.0512      | 0.0030    |
   f64 direct_dft sits at 0.89 of its 12 u bound because of the table, not the kernel: put_twiddle (plan.hip) rounds the angle
   -2 pi p / N to f64 before cos / sin, so an f64 entry is off by up to |angle| x 2.35 u (measured against long double: 10.5 u at N = 13,
   p = 11, which is that case's whole error; 6 to 9 u at N = 1024 ... 8192; far below an f32 entry's own rounding).  The same entries
   feed every other f64 route, whose figures are two to four times the f32 ones.
"""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests import helpers as H
from tests import test_frame_locality as FL
from tests.test_bigfft_lengths import C_FORM, CNP, CREF, F32, F64, LD, NP, PI_LD, REF, U  # (asserts at import that numpy keeps long double)
from tests.test_frame_locality import CB, chirp_m, paired
from tests.test_gpu_parity import GUARD32, TOL64

assert FL.U == U and CB["bluestein"] == C_FORM["chirpz"] == 12.0
C = C_FORM["four_step"]  # 4: the constant of the per-product bound, shared with tests/test_bigfft_lengths.py's impulse line
DTYPES = (F32, F64)
HOST = _ffi.DEVICE_HOST_ONLY
CSRC = os.path.join(os.path.dirname(os.path.abspath(_ffi.__file__)), "csrc")
CHUNK = 1 << 23  # output entries per call
WORST = {}

# ---- 1. routes ---------------------------------------------------------------------------------------------------------------------
TUNED = ("r32x16_f32", "r32x32_f32", "r64x32_f32", "d32x16_f64", "d512_f64", "d32x32_f64")
# frames per signal below which a call leaves the tuned kernel for k_reg_radix (`a.x != nullptr && a.n_frames < ...` in
# plan_geometry_*: kernels_r32x32.hip:386, kernels_r64x32.hip:323, kernels_d32x16.hip:599 and :626, kernels_d32x32.hip:336)
STEP_DOWN = {"r32x32_f32": 5, "r64x32_f32": 4, "d32x16_f64": 8, "d512_f64": 16, "d32x32_f64": 4}
# frames per tile (a.ft of plan_geometry_*; k_bs_fused: up to 16 pairs, bluestein.hip:570; the LDS-budget kernels: at most 16,
# kernels_generic.hip:923); k_reg_radix: reg_radix_ft_max below
TILE = {"r32x32_f32": 16, "r64x32_f32": 8, "d32x16_f64": 16, "d512_f64": 32, "d32x32_f64": 8, "lds_radix2": 16, "two_factor_dft": 16,
        "direct_dft": 16, "bluestein": 32}
S_TUNED = {"r32x16_f32": 7, "r32x32_f32": 8, "r64x32_f32": 9, "d32x16_f64": 7, "d512_f64": 7, "d32x32_f64": 8}  # the docstring's table

# kMixedSplits of reg_radix.h: len -> (A, B)
MIXED = {40: (8, 5), 60: (10, 6), 80: (10, 8), 100: (10, 10), 120: (12, 10), 160: (16, 10), 200: (25, 8), 240: (16, 15), 300: (20, 15),
         320: (20, 16), 400: (25, 16), 480: (24, 20), 500: (25, 20), 600: (25, 24), 720: (30, 24), 800: (32, 25), 960: (32, 30),
         640: (16, 40), 1000: (25, 40), 1080: (30, 36), 1200: (30, 40), 1280: (32, 40)}


def reg_split_len(length, dtype):
    """reg_radix.h reg_split_len: (A, B, C) of a complex transform of `length` points, or None."""
    if length < 16:
        return None
    if length & (length - 1) == 0:
        l2 = length.bit_length() - 1
        if l2 > 12:
            return None
        if l2 <= (6 if dtype == F64 else 8):
            la, lb, lc = (l2 + 1) // 2, l2 // 2, 0
        else:
            la, lb, lc = (l2 + 2) // 3, (l2 + 1) // 3, l2 // 3
        return 1 << la, 1 << lb, 1 << lc
    return MIXED[length] + (1,) if length in MIXED else None


def reg_radix_ft_max(bc):
    """kernels_generic.hip reg_radix_ft_max: the largest tile of k_reg_radix, 256 NI / (B C) frames up to 32."""
    ni = 2 if bc & (bc - 1) == 0 and bc >= 32 else 1
    ft = 1
    while ft < 32 and 2 * ft * bc <= 256 * ni:
        ft *= 2
    return ft


def reg_radix_geometry(dtype, n, hop):
    """kernels_generic.hip plan_geometry_reg_radix for per-bin and complex outputs: (frames per tile, staged)."""
    a, b, c = reg_split_len(n // 2, dtype)
    es, m = (4 if dtype == F32 else 8), a * b * c
    rs = b * c + (0 if c > 1 else 1)   # rr_layout.h rr_swizzle: every three-pass entry has rs = B C; two passes: rows of B + 1
    fs = (a * rs) | 1                  # rr_frame_stride
    tile_bytes = lambda ft: ((ft * fs + m // 2 + 1 + m) * 2 * es + 15) & ~15  # reg_radix_bytes
    budget = 80 << 10                  # kRegBudgetBins
    if dtype == F64 and a >= 16:
        budget = max(budget, (144 - 16) << 10)
    want = dtype == F32 or (a >= 16 and c > 1)  # reg_radix_want_staged (= rr_can_stage)

    def stage_ok(ft):  # reg_radix_stage_ok
        chunks = -(-((ft - 1) * hop + n) // (16 // es))
        rounds = 8 if 2 * m * es >= 16384 else 6  # rr_stage_rounds
        return chunks <= 256 * rounds and chunks * 16 <= ft * fs * 2 * es

    ft = reg_radix_ft_max(b * c)
    while ft >= 1:
        if tile_bytes(ft) <= budget:
            return ft, want and 2 * hop <= n and stage_ok(ft)
        ft >>= 1
    assert tile_bytes(1) <= 144 << 10  # kRegHardLimit
    return 1, False


def _rr(dtype, hops):
    return [(dtype, n, hop, var, "reg_radix") for n, hop, var in hops]


# the mixed sizes: n_fft = 2 len, hop = n_fft / 4
_MIX = [(2 * l, l // 2, "staged") for l in sorted(MIXED)]
ROUTES = [
    (F32, 1024, 64, "staged", "r32x16_f32"), (F32, 1024, 128, "staged", "r32x16_f32"), (F32, 1024, 160, "staged", "r32x16_f32"),
    (F32, 1024, 256, "staged", "r32x16_f32"), (F32, 1024, 400, "direct", "r32x16_f32"), (F32, 1024, 255, "odd", "r32x16_f32"),
    (F32, 512, 64, "paired staged", "r32x16_f32"), (F32, 512, 128, "paired staged", "r32x16_f32"),
    (F32, 512, 160, "paired staged", "r32x16_f32"), (F32, 512, 256, "paired staged", "r32x16_f32"),
    (F32, 512, 150, "paired packed", "r32x16_f32"), (F32, 512, 512, "paired packed", "r32x16_f32"),
    (F32, 2048, 512, "staged", "r32x32_f32"), (F32, 2048, 511, "odd", "r32x32_f32"),
    (F32, 4096, 1024, "staged", "r64x32_f32"),
    (F64, 1024, 256, "staged", "d32x16_f64"), (F64, 1024, 255, "odd", "d32x16_f64"),
    (F64, 512, 160, "paired", "d512_f64"),
    (F64, 2048, 512, "staged", "d32x32_f64"),
    # k_reg_radix through a tuned plan's short calls: f32 (16, 8, 8), f32 (16, 16, 8), f64 (8, 8, 8)
    (F32, 2048, 512, "short", "r32x32_f32"), (F32, 4096, 1024, "short", "r64x32_f32"), (F64, 1024, 256, "short", "d32x16_f64"),
    # ... and the one f64 instance that stages: k_reg_radix<double, 16, 8, 8, staged> (a tile of 4 frames, 1792 chunks of 2048)
    (F64, 2048, 512, "short", "d32x32_f64"),
    # k_reg_radix, powers of two: f32 (4,4,1) (8,4,1) (8,8,1) (16,8,1) (16,16,1: n_fft 512 at an odd hop) (16,16,16)
    *_rr(F32, [(32, 8, "staged"), (64, 16, "staged"), (128, 32, "staged"), (256, 64, "staged"), (512, 129, "odd"), (8192, 2048, "direct"),
               (256, 200, "direct"), (400, 300, "direct"), (400, 161, "odd")]),
    # f64 (4,4,1) (8,4,1) (8,8,1) (8,4,4) (8,8,4: n_fft 512 above hop 260) (16,8,8: 2048 at an odd hop above 1024) (16,16,8: never stages)
    *_rr(F64, [(32, 8, "direct"), (64, 16, "direct"), (128, 32, "direct"), (256, 64, "direct"), (512, 300, "direct"), (2048, 1025, "direct"),
               (4096, 1024, "direct"), (4096, 2500, "direct")]),
    *_rr(F32, _MIX), *_rr(F64, [(n, h, "direct") for n, h, _ in _MIX]),
    *[(d, n, h, "", "lds_radix2") for d in DTYPES for n, h in ((4, 3), (8, 3), (16, 5))], (F64, 8192, 2048, "", "lds_radix2"),
    *[(d, 15, 4, "", "two_factor_dft") for d in DTYPES], *[(d, 13, 4, "", "direct_dft") for d in DTYPES],
    # chirp-z: M = 1024, 2048, 4096
    *[(d, n, h, "paired", "bluestein") for d in DTYPES for n, h in ((401, 160), (1009, 252), (2003, 500))],
]
# (f64 mixed sizes have C = 1, so reg_radix_want_staged is false for them at every hop: "direct")
# "short" cases that stage / do not (reg_radix_geometry, asserted in the route test)
SHORT_STAGED = {(F32, 2048): True, (F32, 4096): True, (F64, 1024): False, (F64, 2048): True}
# reg_radix.h instances no forward STFT call reaches: (dtype, A, B, C) -> why
UNREACHABLE = {
    (F32, 8, 8, 8): "n_fft 1024 in f32 resolves to r32x16_f32 at every hop, and plan_geometry_r32x16_f32 has no frames-per-signal limit",
    (F64, 16, 16, 16): "n_fft 8192 in f64: one frame with its tables is above kRegHardLimit (144 KiB), the plan runs lds_radix2",
}
# power outputs as well: the tuned kernels, bluestein, one k_reg_radix case per type
POWER_TOO = {(F32, 400, 100), (F64, 400, 100)}


def case_id(c):
    return f"{c[4]}-{c[0][5:]}-{c[1]}-{c[2]}" + (f"-{c[3].replace(' ', '_')}" if c[3] else "")


def runs_reg_radix(case):
    return case[4] == "reg_radix" or case[3] == "short"


def kinds_of(case):
    dtype, n, hop, var, name = case
    power = (name in TUNED and var != "short") or name == "bluestein" or (name == "reg_radix" and (dtype, n, hop) in POWER_TOO)
    return ("complex", "power") if power else ("complex",)


def is_paired(case):
    return case[3] != "short" and paired(case[4], case[0], case[1])


def route_S(case):
    """S of the docstring's table; None for the chirp-z bound."""
    dtype, n, _, _, name = case
    if name == "bluestein":
        return None
    if runs_reg_radix(case):
        return S_reg(*reg_split_len(n // 2, dtype))
    if name in S_TUNED:
        return S_TUNED[name]
    return {"lds_radix2": max((n // 2).bit_length() - 2, 0), "two_factor_dft": 3, "direct_dft": 1}[name]


def inreg(p):
    """Rounded products of an impulse through MixFft<p> (the docstring's inreg)."""
    if p & (p - 1) == 0:
        return max(p.bit_length() - 3, 0)
    r = 5 if p % 5 == 0 else 3
    q = p // r
    return 1 + (1 if q > 1 else 0) + inreg(q)


def chain(p):
    return max(bin(k).count("1") for k in range(p))


def S_reg(a, b, c):
    return inreg(a) + chain(a) + inreg(b) + (chain(b) + inreg(c) if c > 1 else 0)


def tile_of(case):
    dtype, n, _, _, name = case
    if runs_reg_radix(case):
        return reg_radix_geometry(dtype, n, case[2])[0]
    if name == "r32x16_f32":
        return 16 if n == 1024 else 32  # kernels_r32x16.hip plan_geometry_r32x16_f32
    return TILE[name]


def frames_a(case):
    """Frames per signal of pass A (the docstring's F_A)."""
    _, n, _, var, name = case
    base = 4 if n <= 1024 else 2
    if var == "short":
        return min(base, STEP_DOWN[name] - 1)
    return max(base, STEP_DOWN.get(name, 0) + (STEP_DOWN.get(name, 0) & 1))  # (an even count: whole pairs)


def frames_b(case):
    """Frames per signal of pass B: two tiles plus one ("short": as many as stay below the threshold)."""
    _, _, _, var, name = case
    full = 2 * tile_of(case) + 1
    return min(full, STEP_DOWN[name] - 1) if var == "short" else full


def make_plan(dtype, n, hop, kind, centre, device=_ffi.DEVICE_CURRENT):
    params = sg.SpectrogramParams(sg.StftParams(n, hop, sg.WindowType.custom(window(n)), centre), 16000.0)
    return sg.Plan(params, _ffi.AMP_COMPLEX if kind == "complex" else _ffi.AMP_POWER, None, None, dtype, device=device)


@pytest.mark.parametrize("case", ROUTES, ids=case_id)
def test_route_table_selects_the_named_kernel(case):
    dtype, n, hop, var, name = case
    for kind in kinds_of(case):
        for centre in (False, True):
            assert make_plan(dtype, n, hop, kind, centre, device=HOST).kernel_name == name
    assert route_S(case) is None or 0 <= route_S(case) <= math.ceil(math.log2(n)) + 4
    fa, fb = frames_a(case), frames_b(case)
    if var == "short":
        assert name in STEP_DOWN and 2 <= fa < STEP_DOWN[name] and fb < STEP_DOWN[name]
    else:
        assert fa >= max(2, STEP_DOWN.get(name, 0)) and fb >= max(3, STEP_DOWN.get(name, 0)) and fb == 2 * tile_of(case) + 1
    if is_paired(case):
        assert fa % 2 == 0
    if runs_reg_radix(case):  # the label against the restated geometry: which variant of the instance the case runs
        ft, staged = reg_radix_geometry(dtype, n, hop)
        assert 1 <= ft <= reg_radix_ft_max(math.prod(reg_split_len(n // 2, dtype)[1:]))
        if var == "short":
            assert staged == SHORT_STAGED[dtype, n]
        elif var in ("staged", "direct"):
            assert staged == (var == "staged"), (case_id(case), ft, staged)


def _xmacro(text, macro):
    body = re.search(r"#define\s+" + macro + r"\(X\)((?:.*\\\n)*.*)\n", text).group(1)
    return [tuple(int(v) for v in m.groups()) for m in re.finditer(r"X\((\d+),\s*(\d+),\s*(\d+)\)", body)]


def header_instances():
    text = open(os.path.join(CSRC, "reg_radix.h")).read()
    f32, f64, mixed = (_xmacro(text, "SGX_RR_SPLITS_" + s) for s in ("F32", "F64", "MIXED"))
    assert len(f32) >= 9 and len(f64) >= 9 and len(mixed) >= 22, (len(f32), len(f64), len(mixed))  # the parser sees the lists
    table = {int(m.group(1)): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"\{(\d+),\s*(\d+),\s*(\d+)\},", text)}
    return f32, f64, mixed, table


def test_reg_split_len_restated_matches_the_header_lists():
    f32, f64, mixed, table = header_instances()
    assert table == MIXED
    pow2 = [1 << l for l in range(4, 13)]
    assert {reg_split_len(l, F32) for l in pow2} == set(f32) and {reg_split_len(l, F64) for l in pow2} == set(f64)
    assert {reg_split_len(l, d) for l in MIXED for d in DTYPES} == set(mixed)
    assert reg_split_len(8, F32) is None and reg_split_len(8192, F32) is None and reg_split_len(24, F64) is None
    for a, b, c in f32 + f64 + mixed:
        assert reg_split_len(a * b * c, F32 if (a, b, c) in f32 + mixed else F64) == (a, b, c)


def test_every_reg_radix_instance_is_reached_or_listed():
    """Fails when a split is added to reg_radix.h and not to ROUTES (or UNREACHABLE)."""
    f32, f64, mixed, _ = header_instances()
    every = {(F32,) + s for s in f32 + mixed} | {(F64,) + s for s in f64 + mixed}
    reached = {(c[0],) + reg_split_len(c[1] // 2, c[0]) for c in ROUTES if runs_reg_radix(c)}
    assert not reached & set(UNREACHABLE), reached & set(UNREACHABLE)
    assert reached | set(UNREACHABLE) == every, (every - reached - set(UNREACHABLE), (reached | set(UNREACHABLE)) - every)
    for key in UNREACHABLE:  # the reasons, checked where a host-only plan can: the length resolves elsewhere at even and odd hops
        dtype, a, b, c = key
        n = 2 * a * b * c
        assert {make_plan(dtype, n, hop, "complex", False, device=HOST).kernel_name for hop in (n // 4, n // 4 + 1, n // 2 + 1, n)} == \
            {"r32x16_f32" if dtype == F32 else "lds_radix2"}
    # one staged and one direct variant per type, by the restated geometry (not by the label)
    for dtype in DTYPES:
        assert {reg_radix_geometry(c[0], c[1], c[2])[1] for c in ROUTES if runs_reg_radix(c) and c[0] == dtype} == {True, False}
    # ... and per instance wherever some call can stage it: every f32 split but (16, 16, 16); in f64 (16, 8, 8) alone
    stages = {(c[0],) + reg_split_len(c[1] // 2, c[0]) for c in ROUTES if runs_reg_radix(c) and reg_radix_geometry(c[0], c[1], c[2])[1]}
    assert stages == {k for k in reached if k[0] == F32 and k[1:] != (16, 16, 16)} | {(F64, 16, 8, 8)}
    assert reg_radix_geometry(F64, 2048, 512) == (4, True) and reg_radix_geometry(F64, 4096, 1024) == (2, False)
    assert reg_radix_geometry(F32, 8192, 2048) == (1, False) and reg_radix_geometry(F32, 400, 100) == (32, True)
    for hop in range(1, 4097):  # f64 (16, 16, 8) and f32 (16, 16, 16) stage at no hop
        assert not reg_radix_geometry(F64, 4096, hop)[1] and not reg_radix_geometry(F32, 8192, min(2 * hop, 8192))[1]
    z = re.findall(r"\{(8|16), (\d+), (\d+), (\d+), \{(\d+),", open(os.path.join(CSRC, "rr_layout.h")).read())
    assert len(z) >= 10 and all(int(rs) == int(b) * int(c) for _, _, b, c, rs in z)  # rr_swizzle's table: rs = B C, as restated
    for dtype in DTYPES:
        assert any(c[4] == "reg_radix" and "power" in kinds_of(c) for c in ROUTES if c[0] == dtype)


def test_routes_reach_every_on_chip_forward_kernel_name():
    """Every name sgx_kernel_name (plan.hip) can return for a forward STFT plan occurs in ROUTES, but for the CQT names and the two
    global-memory routes (tests/test_cqt_readback.py, tests/test_bigfft_lengths.py)."""
    src = open(os.path.join(CSRC, "plan.hip")).read()
    body = re.search(r"const char \*sgx_kernel_name\(const sgx_plan \*plan\) \{(.*?)\n\}", src, re.S).group(1)
    names = set(re.findall(r'"(\w+)"', body))
    tuned = set(re.findall(r'\{K_\w+, "(\w+)", SGX_F(?:32|64),', src))
    assert tuned == set(TUNED) and {"lds_radix2", "reg_radix", "bluestein", "direct_dft", "big_chirpz"} <= names  # the parser sees both
    elsewhere = {n for n in names if n.startswith("cqt_")} | {"big_four_step", "big_chirpz"}
    assert len(elsewhere) == 5
    assert {c[4] for c in ROUTES} == (names | tuned) - elsewhere
    text = "".join(open(os.path.join(CSRC, f"kernels_{k}.hip")).read() for k in ("r32x32", "r64x32", "d32x16", "d32x32"))
    for name in STEP_DOWN:  # the restated thresholds and tiles, against the geometry functions' own lines
        fn = name.split("_f")[0]
        geo = re.search(r"bool plan_geometry_" + fn + r"_f\d+\(StftArgs &a\) \{(.*?)\n\}", text, re.S).group(1)
        assert re.search(r"a\.x != nullptr && a\.n_frames < (\d+)u", geo).group(1) == str(STEP_DOWN[name])
        assert re.search(r"a\.ft = (\d+);", geo).group(1) == str(TILE[name])
    # ... and the other tiles: r32x16 (32 frames at n_fft 512, its three branches; else 16), the LDS-budget kernels' largest tile, the
    # chirp-z tile of up to 2^4 frame pairs
    r16 = open(os.path.join(CSRC, "kernels_r32x16.hip")).read()
    geo = re.search(r"bool plan_geometry_r32x16_f32\(StftArgs &a\) \{(.*?)\n\}", r16, re.S).group(1)
    assert re.findall(r"a\.ft = (\d+);", geo) == ["32", "32", "16"] and geo.index("a.n_fft != 1024") > geo.rindex("a.ft = 32;")
    assert tile_of((F32, 1024, 256, "staged", "r32x16_f32")) == 16 and tile_of((F32, 512, 128, "paired staged", "r32x16_f32")) == 32
    gen = open(os.path.join(CSRC, "kernels_generic.hip")).read()
    pick = re.search(r"static bool pick_frames_per_tile\(.*?\n\}", gen, re.S).group(0)
    assert re.search(r"for \(unsigned ft = (\d+); ft >= 1; ft >>= 1\)", pick).group(1) == "16" == str(TILE["lds_radix2"])
    assert TILE["two_factor_dft"] == TILE["direct_dft"] == 16
    for fn in ("lds_radix2", "direct_dft", "two_factor"):
        assert "pick_frames_per_tile(a, " in re.search(r"bool plan_geometry_" + fn + r"\(StftArgs &a, int dtype\) \{(.*?)\n\}", gen, re.S).group(1)
    bs = open(os.path.join(CSRC, "bluestein.hip")).read()
    geo = re.search(r"bool fused_geometry\(.*?\n\}", bs, re.S).group(0)
    assert 2 << int(re.search(r"ltile = (\d+);", geo).group(1)) == TILE["bluestein"]


# ---- 2. inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def window(n):
    """w[j] = 0.5 + q_j / 2048 (f64, exact in f32 with its half), q_j != q_(j-1), q_j != q_(n-1-j)."""
    rng = np.random.default_rng(n)
    q = rng.integers(0, 1024, n)
    for j in range(n):
        while (j > 0 and q[j] == q[j - 1]) or (n - 1 - j < j and q[j] == q[n - 1 - j]):
            q[j] = rng.integers(0, 1024)
    w = 0.5 + q / 2048.0
    w.setflags(write=False)
    return w


def test_window_is_exact_asymmetric_and_pairwise_distinct():
    for n in sorted({c[1] for c in ROUTES}):
        w = window(n)
        h = (w / 2).astype(np.float32)
        assert np.array_equal(w.astype(np.float32).astype(np.float64), w) and np.array_equal(h.astype(np.float64) * 2, w)
        assert w.min() >= 0.5 and w.max() < 1.0 and np.all(w[1:] != w[:-1])
        j = np.arange(n)
        assert np.all((w != w[::-1]) | (j == n - 1 - j))
        assert np.all(w[0::2][:n // 2] != w[1::2])


def trains(n, hop, frames, residues, centre, dtype):
    """Signals of `frames` frames: signal i is 1 at every t = residues[i] mod n.  Centred: the length is no multiple of the hop."""
    length = n + (frames - 1) * hop if not centre else (frames - 1) * hop + max(1, hop // 3)
    t = np.arange(length)
    return (t[None, :] % n == np.asarray(residues)[:, None]).astype(NP[dtype])


def rows_of(x, n, hop, centre):
    """(row [B, F], live [B, F]) of each frame's impulse, by the independent framing of tests/helpers.py."""
    fr = np.stack([H.np_frames(r, n, hop, centre) for r in x])
    assert np.count_nonzero(fr, axis=-1).max() <= 1
    return fr.argmax(axis=-1), fr.any(axis=-1)


def residues_b(n):
    fixed = list(dict.fromkeys([0, 1, n // 2 - 1, n // 2, n - 1]))
    rng = np.random.default_rng(n + 1)
    rest = [int(r) for r in rng.permutation(n) if r not in fixed]
    return (fixed + rest)[:min(16, n)]


# ---- 3. reference, bounds, the checker ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def roots(n, dtype):
    """exp(-2 pi i m / n), m < n, in the reference's type."""
    R = REF[dtype]
    a = (2 * (PI_LD if R is LD else np.pi)) * np.arange(n).astype(R) / R(n)
    z = np.cos(a) - 1j * np.sin(a)
    assert z.dtype == CREF[dtype]
    z.setflags(write=False)
    return z


def _ratio(err, bound):
    """err / bound; 0 where both are 0, inf where only the bound is."""
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    out = np.zeros(err.shape)
    np.divide(err, bound, out=out, where=bound > 0)
    out[(bound <= 0) & ~(err == 0)] = np.inf
    return out


def complex_bound(rows, live, n, dtype, S, pair, M=None, amp=1.0):
    """(amp w of each frame's row, 0 for an all-zero frame; the complex bound) per [B, F].  amp: the impulses' height, a power of two."""
    wr = np.where(live, amp * window(n)[rows], 0.0)
    Wf = wr.copy()
    if pair:
        F = wr.shape[1]
        f = np.arange(F)
        has = (f ^ 1) < F
        Wf[:, has] += wr[:, (f ^ 1)[has]]
    if M is not None:
        return wr, CB["bluestein"] * U[dtype] * math.log2(M) * math.sqrt(M) * Wf
    return wr, C * U[dtype] * (S + 2) * Wf


def check(got, rows, live, n, dtype, kind, S, pair=False, M=None, amp=1.0):
    """Worst ratio of an output [B, bins, F] to its bounds (section 3 of the docstring).  Both bounds are the same for every bin of a
    frame (|ref[j, k]| = w_j), so the largest error over a frame's bins is compared with them: every entry counts, none is left out."""
    R, CR = REF[dtype], CREF[dtype]
    B, nb, F = got.shape
    assert nb == n // 2 + 1 and rows.shape == live.shape == (B, F)
    wr, delta = complex_bound(rows, live, n, dtype, S, pair, M, amp)
    if kind == "complex":
        idx = (rows[:, :, None].astype(np.int64) * np.arange(nb)[None, None, :]) % n  # [B, F, bins]: the long axis innermost
        d = np.ascontiguousarray(got.transpose(0, 2, 1)).astype(CR) - roots(n, dtype)[idx] * wr[:, :, None].astype(R)
        e2 = d.real ** 2 + d.imag ** 2
        worst = float(np.max(_ratio(np.sqrt(np.max(e2, axis=2)), delta)))
        if M is not None:  # chirp-z: the 2-norm over the bins of a pair's frames, which bounds the largest entry too
            s = np.sqrt(np.add.reduceat(np.sum(e2, axis=2), np.arange(0, F, 2), axis=1))
            worst = max(worst, float(np.max(_ratio(s, delta[:, ::2]))))
        return worst
    assert not np.iscomplexobj(got)
    a2 = (wr.astype(R) * wr.astype(R))[:, None, :]  # |ref[j, k]|^2 = w_j^2 at every bin (exact in R: w has 11 bits)
    err = np.max(np.abs(got.astype(R) - a2), axis=1)
    return float(np.max(_ratio(err, delta * (2 * wr + delta))))


def record(case, kind, pass_, ratio):
    name = "reg_radix (short call of " + case[4] + ")" if case[3] == "short" else case[4]
    key = (name, case[0], kind)
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))
    print(f"{case_id(case)} {kind} pass {pass_}: worst ratio to bound {ratio:.3g}")


# ---- 4. the checker can fail (CPU) -------------------------------------------------------------------------------------------------
def synth(n, dtype, hop, frames, residues, centre, w=None):
    """torch.fft.rfft in the plan's type of the impulse frames times the window: (output [B, bins, F], rows, live)."""
    x = trains(n, hop, frames, residues, centre, dtype)
    fr = np.stack([H.np_frames(r, n, hop, centre) for r in x]) * (window(n) if w is None else w).astype(NP[dtype])[None, None, :]
    got = torch.fft.rfft(torch.from_numpy(fr), dim=-1).numpy().transpose(0, 2, 1)
    rows, live = rows_of(x, n, hop, centre)
    return np.ascontiguousarray(got), rows, live


def log2c(n):
    return math.ceil(math.log2(n))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [80, 400, 512, 1024, 1920, 2048, 4096])
def test_bound_calibration_a_plain_fft_meets_it(n, dtype):
    """Every entry of a plain FFT (S = ceil(log2 N) stages) of pass A's frames, under the window above: 0.09 to 0.20 of the bound, so it
    can be met and is not vacuous.  (N <= 1024: every residue; above: 256 seeded ones.)"""
    res = np.arange(n) if n <= 1024 else np.sort(np.random.default_rng(n).permutation(n)[:256])
    got, rows, live = synth(n, dtype, n // 4, 2, res, False)
    assert live.all() and (n > 1024 or np.array_equal(np.sort(rows[:, 1]), np.arange(n)))
    r = check(got, rows, live, n, dtype, "complex", log2c(n))
    p = check((got.real ** 2 + got.imag ** 2).astype(NP[dtype]), rows, live, n, dtype, "power", log2c(n))
    print(f"N = {n} {dtype}: plain FFT worst entry {r:.3g} of the bound, power {p:.3g}")
    assert 0.02 < r < 0.5 and p < 1.0


def old_criteria(got, rows, live, n, dtype, amp=1.0):
    """(ratio to the parity tolerance of tests/test_gpu_parity.check, worst ratio to the per-frame bound of tests/test_frame_locality.py)."""
    wr = np.where(live, amp * window(n)[rows], 0.0)
    k = np.arange(n // 2 + 1)
    ref = roots(n, F32)[(rows[:, None, :] * k[None, :, None]) % n] * wr[:, None, :]
    err = np.abs(got.astype(np.complex128) - ref)
    scale = float(np.max(np.abs(ref)))
    parity = float(np.max(err)) / (GUARD32 * scale if dtype == F32 else TOL64 * max(1.0, scale))
    per_frame = C * U[dtype] * math.log2(n) * math.sqrt(n) * wr  # ||x_f w||_2 = |w_j|
    return parity, float(np.max(_ratio(np.max(err, axis=1), per_frame)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [512, 1024])
def test_planted_faults_fail_the_checker(n, dtype):
    hop, F, S = n // 4, 9, log2c(n)
    res = residues_b(n)
    got, rows, live = synth(n, dtype, hop, F, res, True)
    run = lambda g, kind="complex": check(g, rows, live, n, dtype, kind, S)
    power = lambda g: (g.real ** 2 + g.imag ** 2).astype(NP[dtype])
    assert (~live).any() and live[:, 1:].any()
    clean = run(got)
    assert 0.02 < clean < 1.0 and run(power(got), "power") < 1.0
    assert not got.transpose(0, 2, 1)[~live].any()
    b, f = [int(v[0]) for v in np.nonzero(live & (rows % 2 == 1) & np.roll(live, -1, axis=1) & (np.arange(F) < F - 1)[None, :])]
    k0 = n // 8 + 3
    # one entry moved by 64 ulp of its own size: caught here, let through by the older criteria
    bad = got.copy()
    bad[b, k0, f] += NP[dtype](64 * np.spacing(NP[dtype](abs(got[b, k0, f]))))
    assert run(bad) > 1.0
    parity, per_frame = old_criteria(bad, rows, live, n, dtype)
    print(f"N = {n} {dtype} 64 ulp: {run(bad):.3g} of the entry bound; {parity:.3g} of the parity tolerance, {per_frame:.3g} of the per-frame bound")
    assert parity < 1.0 and per_frame < 1.0
    # the window reversed, shifted by one, with the entries of each pair (2i, 2i + 1) swapped
    w = window(n)
    swapped = w.reshape(-1, 2)[:, ::-1].reshape(-1)
    for name, wb in (("reversed", w[::-1]), ("shifted", np.roll(w, 1)), ("pair-swapped", swapped)):
        g = synth(n, dtype, hop, F, res, True, w=np.ascontiguousarray(wb))[0]
        assert run(g) > 1.0 and run(power(g), "power") > 1.0, name
    # frames 2p and 2p + 1 swapped; one bin taken from the neighbouring frame
    perm = np.arange(F) ^ 1
    perm[perm >= F] = F - 1
    assert run(np.ascontiguousarray(got[:, :, perm])) > 1.0
    bad = got.copy()
    bad[b, k0, f] = got[b, k0, f + 1]
    assert run(bad) > 1.0
    # a zero frame holding one denormal
    bz, fz = [int(v[0]) for v in np.nonzero(~live)]
    for kind, g in (("complex", got), ("power", power(got))):
        bad = g.copy()
        bad[bz, 5, fz] = np.finfo(NP[dtype]).smallest_subnormal
        assert run(bad, kind) == np.inf
    if dtype == F64:  # one row's twiddles rounded through f32
        j0 = int(rows[b, f])
        k = np.arange(n // 2 + 1)
        a = 2 * np.pi * ((j0 * k) % n) / n
        row32 = w[j0] * (np.cos(a).astype(np.float32).astype(np.float64) - 1j * np.sin(a).astype(np.float32).astype(np.float64))
        bad = got.copy()
        hit = np.nonzero(live & (rows == j0))
        for bb, ff in zip(*hit):
            bad[bb, :, ff] = row32
        assert run(bad) > 1.0
        parity, per_frame = old_criteria(bad, rows, live, n, dtype)
        guard = float(np.max(np.abs(bad - got))) / (GUARD32 * float(np.max(np.abs(got))))
        print(f"N = {n} row {j0} through f32: {run(bad):.3g} of the entry bound; {guard:.3g} of GUARD32, {parity:.3g} of TOL64, "
              f"{per_frame:.3g} of the f64 per-frame bound")
        assert guard < 1.0 and parity > 1.0
        # the same frames at 2^-10 of full scale (input and output scale exactly): the absolute f64 parity criterion lets the row through,
        # the entry bound fails it as before
        amp = 2.0 ** -10
        low = check(bad * amp, rows, live, n, dtype, "complex", S, amp=amp)
        parity_low, per_frame_low = old_criteria(bad * amp, rows, live, n, dtype, amp)
        print(f"    at 2^-10 of full scale: {low:.3g} of the entry bound; {parity_low:.3g} of TOL64, {per_frame_low:.3g} of the f64 per-frame bound")
        assert check(got * amp, rows, live, n, dtype, "complex", S, amp=amp) == clean and low == run(bad) and parity_low < 1.0


# ---- the GPU cases -----------------------------------------------------------------------------------------------------------------
def run_pass(case, plans, kinds, centre, frames, residues, pass_):
    dtype, n, hop, _, name = case
    S, pair = route_S(case), is_paired(case)
    M = chirp_m(n) if name == "bluestein" else None
    nb = n // 2 + 1
    per = max(1, CHUNK // (nb * frames))
    worst = {k: 0.0 for k in kinds}
    for i in range(0, len(residues), per):
        x = trains(n, hop, frames, residues[i:i + per], centre, dtype)
        rows, live = rows_of(x, n, hop, centre)
        assert rows.shape[1] == frames and (centre or live.all())
        for kind in kinds:
            got = np.asarray(plans[kind, centre].compute_batch(x))
            assert got.shape == (x.shape[0], nb, frames) and got.dtype == (CNP[dtype] if kind == "complex" else NP[dtype])
            worst[kind] = max(worst[kind], check(got, rows, live, n, dtype, kind, S, pair, M))
    for kind in kinds:
        record(case, kind, pass_, worst[kind])
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROUTES, ids=case_id)
def test_gpu_every_entry_of_the_forward_matrix(case):
    dtype, n, hop, var, name = case
    kinds = kinds_of(case)
    plans = {(k, c): make_plan(dtype, n, hop, k, c) for k in kinds for c in (False, True)}
    for p in plans.values():
        assert p.kernel_name == name
    # pass A: every row through every frame slot
    fa = frames_a(case)
    a = run_pass(case, plans, kinds, False, fa, np.arange(n), "A")
    # pass B: every tile slot, the zero padding, tiles that run on into the next signal
    res = residues_b(n)
    b = run_pass(case, plans, kinds, True, frames_b(case), res, "B")
    b5 = run_pass(case, plans, kinds, True, 5, res, "B, 5 frames") if name in ("r32x16_f32", "bluestein") else {}
    for p in plans.values():
        assert p.kernel_name == name
    for kind in kinds:
        assert a[kind] <= 1.0 and b[kind] <= 1.0 and b5.get(kind, 0.0) <= 1.0, (case_id(case), kind, a[kind], b[kind], b5.get(kind))


@pytest.mark.gpu
def test_gpu_worst_ratios_per_route():
    """Prints what the cases above recorded (run the module as a whole): worst ratio to the bound per kernel, type and output."""
    print()
    for (name, dtype, kind), r in sorted(WORST.items()):
        print(f"| {name} | {dtype} | {kind} | {r:.3g} |")
    assert all(r <= 1.0 for r in WORST.values())
