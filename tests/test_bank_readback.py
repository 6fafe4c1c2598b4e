"""Filterbank read-back: every weight of every bank route, read back through the kernels one bin at a time.

The filterbank stage (Mel / log-Hz / ERB / chroma rows, MFCC on top) is about a dozen pieces of device code, and the bank's SHAPE picks
one: band schedules per tuned kernel, the matrix-core epilogue, CSR loops, the chirp-z kernel's own rows, the split path.
`Plan.bank_stage_name` (sgx_bank_stage_name) names the stage the last call ran; CASES pins (kernel, stage) for every bank of the sweep.

Probe input: signal b is 0.5 cos(2 pi k_b t / n_fft + phi_b), k_b an integer bin, 9 frames long.  The middle frames hold a three-bin
spectrum, so band m of probe k reads back (almost) the single weight W[m, k]; the first and last two frames see the zero padding and a
broadband spectrum.  One batch holds one signal per probed bin (all n_fft / 2 + 1 up to 1025; the edges and the peak of every band above).

Reference: W64 . P64, P64 = |rfft(frames x window)|^2 in NumPy f64 (magnitudes for the chromagram), W64 an independent f64 bank
(tests/helpers.py).  Bound per signal, band m, frame f -- test_frame_locality.py section 3, its constants imported, not copied:
    delta_f = c u log2(N_eff) sqrt(N_eff) ||x_f w||_2          (c, N_eff, the pair norm: that file's CB / PAIRED per kernel)
    dP_k    = delta_f (2 |X_k| + delta_f)                      (magnitude domain: delta_f)
    d_mf    = sum_k W_mk dP_k + (L_m + 2) u sum_k W_mk P_k + sum_k E_mk P_k
L_m = non-zeros of row m; the 2: the weight's own rounding to T and the amplitude step.  E is the reference's OWN error: W64 and the
plan's table are two f64 evaluations of the same formulas and differ by rounding (w_tol below: the tolerances the existing pins of each
family use, tighter for log-Hz; zero wherever W64 is zero).  The CPU part pins `Plan.mel_weights()` against W64 to exactly that E for every
bank of the sweep -- same columns, values within E -- so a miss on the GPU is the kernel's, not the table's.  In f32 E is 1e-7 of the
bound; in f64 it is what an independent reference can resolve.
    sqrt(M):   max(sqrt(ref) - sqrt(max(ref - d, 0)), sqrt(ref + d) - sqrt(ref)) + 2 u sqrt(ref + d)                     (2 u: the root)
    dB:        (10 / ln 10) ln(1 + d / max(ref, eps)) + the documented dB evaluation error (f32 2e-5 dB, f64 4e-15 + 3e-16 |dB|)
    MFCC:      |lift_c| (sum_i |B_ci| dD_i + (n_mels + 3) u sum_i |B_ci D_i|)           (3: basis, lifter and product roundings)
    chroma:    y = v / s(v):  |dy| <= (|dv| + |y| ds) / (s - ds),  ds <= s(dv),  asserted on frames where s - ds > 0
A row without weights comes back as exactly 0 (the floor in dB).  The threshold is 1: no figure below was turned into one.

CPU calibration (f32 model: scipy rfft of f32 frames, f32 re^2 + im^2, f32 rows summed in ascending-bin order): the model meets the bound
with the worst ratio <= 0.5 per family, and four mutations of one middle band (first weight dropped, 1e-6 max(row) just outside, the row
rolled by a bin, one weight x (1 + 1e-4), 1e-3 for rows of >= 48 non-zeros) each break it.

Surprises met while pinning the table (kept as found, the names queried from the library):
  * The 9 frames of a probe are fewer than k_d512 takes (16): the call steps down to the register-tiled kernel ("reg_radix_bands") while
    sgx_kernel_name keeps naming the plan's kernel, "d512_f64".  One case pins that; the d512 cases run 17 frames per signal ("@17").
  * f32 512 at hop 256: the shorter word budget is overrun by WIDE rows, not by many: Mel 1 and 2 leave the tuned kernel (Mel 2 stays on
    it at hop 128), Mel 3 ... 128 fit, and 129 is the schedule's band limit at every hop.
  * Chroma rows ARE runs of consecutive bins (the Gaussian never rounds to zero inside f_min ... f_max) and dense ERB rows are one run of
    all bins: at 4096 (f32) and 2048 (f64) both take the band schedule of k_r64x32 / k_d32x32, not the split path; at f32 2048 ERB-64
    and log-Hz 300 overflow k_r32x32's schedule and run fused on k_reg_radix (CSR and band table), not split.  The split path behind the
    tuned kernels is reached by a hop past the fused stage's staging (f32 4096 / 2048) and by a schedule that overflows (f64 2048 Mel 300).
  * On a Mel bank over exactly 1000-8000 Hz a single 16-row block always spans bins 64 ... 511 (len4 112, no tail); Mel 17 is the one
    size that is still >= 48 non-zeros per row and has two blocks, both off bin 0 and both with a 3-step tail.  Every ERB block has a
    1-step tail (513 bins).
  * log-Hz with one bin follows the reference's 0 / 0 step: a single weight 1 on bin 0.
  * The "1e-6 max(row) outside" mutant cannot break the bound on the chroma rows (magnitude domain, 265 non-zeros: see the comment
    in the calibration); it is asserted there at 1e-3 max(row) and the 1e-6 figure printed.

Measured on MI355X, worst |got - ref| / d per stage name, linear outputs (power, magnitude, chroma) / dB and MFCC outputs.  The dB figures
near 0.4 are rows far below the floor (ref -120 dB, got -99 dB, bound 60 dB: the bound carries the structural zero, not the decibels):
    bank_rows            f32 0.019 / 0.42       f64 0.11 / 0.11
    bluestein_rows       f32 0.0092 / 0.11
    d32x16_sched                                f64 0.37 / 0.049    (0.37: log-Hz, where E, the reference's own error, is the bound)
    d32x32_sched                                f64 0.0099 / 0.0061
    d512_sched                                  f64 0.049 / 0.032
    generic_csr          f32 0.054 / -          f64 0.026 / -
    r32x16_csr           f32 0.038 / 0.36
    r32x16_mfma          f32 0.027 / 0.35
    r32x16_sched         f32 0.037 / 0.36
    r32x16_sched_packed  f32 0.039 / 0.36
    r32x16_sched512      f32 0.034 / 0.26
    r32x16_sched_mfcc    f32 - / 0.00065
    r32x32_sched         f32 0.034 / -
    r64x32_sched         f32 0.021 / 0.44
    reg_radix_bands      f32 0.047 / 0.0015     f64 0.32 / 0.075    (0.32: log-Hz again)
    reg_radix_csr        f32 0.041 / 0.26       f64 0.0078 / 0.0049
No case of the sweep came back above the bound: the places worth suspecting (the MFMA tail fragments, the schedule's padding steps past
n / 2 and its pad-in-front branch, rows of length 0 and 1, bands 128 and up) read back every weight and every structural zero.
"""
import functools
import math
import os
import re

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests import helpers as H
from tests.test_frame_locality import CB, U, chirp_m, frame_deltas, paired  # the bound's constants live there

HOST = _ffi.DEVICE_HOST_ONLY
SR = 16000.0
NP = {"float32": np.float32, "float64": np.float64}
FLOOR = -120.0
MFCC_FLOOR = -80.0
NFRAMES = 9  # per probe signal, unless the case's output says "@n"
WORST = {}
SEEN = set()

# every name sgx_bank_stage_name can return (plan.hip, beside note_bank_stage) ...
NAMES = {"r32x16_sched", "r32x16_sched_packed", "r32x16_sched512", "r32x16_sched_mfcc", "r32x16_mfma", "r32x16_csr", "r32x32_sched", "r64x32_sched", "d32x16_sched",
         "d512_sched", "d32x32_sched", "reg_radix_bands", "reg_radix_csr", "generic_csr", "bluestein_rows", "bank_rows"}
# ... and the separate MFCC launches appended to one of them
SUFFIXES = {"+mfcc_acc", "+mfcc_rows"}


# ---- banks -----------------------------------------------------------------------------------------------------------------------
# ("mel", n, f_min, f_max, sample rate, norm) | ("loghz", n, f_min, f_max) | ("erb", n, f_min, f_max) | ("chroma", norm)
def mel(n, f_min=0.0, f_max=8000.0, sr=SR, norm="none"):
    return ("mel", n, f_min, f_max, sr, norm)


def loghz(n):
    return ("loghz", n, 30.0, 7900.0)


def erb(n):
    return ("erb", n, 0.0, 8000.0)


MEL48K = mel(80, 0.0, 8000.0, 48000.0)


def bank_sr(bank):
    return bank[4] if bank[0] == "mel" else SR


def bank_params(bank):
    if bank[0] == "mel":
        return sg.MelParams(bank[1], bank[2], bank[3], getattr(sg.MelNorm, bank[5]))
    if bank[0] == "loghz":
        return sg.LogHzParams(bank[1], bank[2], bank[3])
    if bank[0] == "erb":
        return sg.ErbParams(bank[1], bank[2], bank[3])
    return sg.ChromaParams(norm=getattr(sg.ChromaNorm, bank[1]))


def bank_w64(bank, n_fft):
    """The independent f64 bank, dense [rows, n_fft / 2 + 1]."""
    if bank[0] == "mel":
        return H.np_mel_filterbank(bank[4], n_fft, bank[1], bank[2], bank[3], None if bank[5] == "none" else bank[5])
    if bank[0] == "loghz":
        if bank[1] == 1:  # one bin: the reference's step is (ln f_max - ln f_min) / 0, its frequency NaN, `NaN as usize` = 0: weight 1 on bin 0
            W = np.zeros((1, n_fft // 2 + 1))
            W[0, 0] = 1.0
            return W
        return H.np_loghz(SR, n_fft, bank[1], bank[2], bank[3])[0]
    if bank[0] == "erb":
        return H.np_erb(SR, n_fft, bank[1], bank[2], bank[3])[0]
    return H.np_chroma_bank(SR, n_fft)


def w_tol(bank, W, n_fft):
    """E: how far two f64 evaluations of the bank's formulas may differ, elementwise; zero where W64 is zero.  Mel, ERB, chroma: the
    tolerances of the existing pins (test_oracle_golden.py 1e-12 max(1, max W); test_erb.py / test_chroma.py rtol 1e-11, atol 1e-16).
    log-Hz (test_loghz.py pins 1e-9): the weight is the fractional part of f / df <= n_fft / 2 with f = exp(ln f_min + i step), relative
    error (2 ln f_max + 2) u64 per evaluation, two evaluations."""
    nz = W != 0
    if bank[0] == "mel":
        return nz * (1e-12 * max(1.0, float(W.max())))
    if bank[0] == "loghz":
        return nz * (2.0 * (2.0 * math.log(bank[3]) + 2.0) * 2.0 ** -53 * (n_fft / 2))
    if bank[0] == "erb":
        return 1e-11 * np.abs(W)
    return nz * (1e-11 * np.abs(W) + 1e-16)


def split_out(out):
    """'power@17' -> ('power', 17 frames per signal); default NFRAMES."""
    k, _, nf = out.partition("@")
    return k, int(nf) if nf else NFRAMES


def make_plan(dtype, n_fft, hop, bank, out, device=_ffi.DEVICE_CURRENT):
    out = split_out(out)[0]
    params = sg.SpectrogramParams(sg.StftParams(n_fft, hop, sg.WindowType.hanning, True), bank_sr(bank))
    if out == "mfcc":
        return sg.Plan(params, _ffi.AMP_DECIBELS, bank_params(bank), sg.LogParams(MFCC_FLOOR), dtype, device=device, mfcc=sg.MfccParams(13))
    amp = {"power": _ffi.AMP_POWER, "magnitude": _ffi.AMP_MAGNITUDE, "db": _ffi.AMP_DECIBELS, "chroma": _ffi.AMP_MAGNITUDE}[out]
    return sg.Plan(params, amp, bank_params(bank), sg.LogParams(FLOOR) if out == "db" else None, dtype, device=device)


def table_dense(plan, nb):
    ptr, col, val = plan.mel_weights()
    W = np.zeros((ptr.size - 1, nb))
    for m in range(ptr.size - 1):
        W[m, col[ptr[m]:ptr[m + 1]]] = val[ptr[m]:ptr[m + 1]]
    return W


# ---- the sweep -------------------------------------------------------------------------------------------------------------------
# (dtype, n_fft, hop, bank, output, sgx_kernel_name, sgx_bank_stage_name)
F32, F64 = "float32", "float64"
CHROMA = [("chroma", n) for n in ("none", "l1", "l2", "max")]
CASES = [
    # f32 1024: the tuned kernel's stages.  9-frame signals at an even hop ride PACKED tiles (16 slots that run on into the next signals);
    # 41 frames ("@41"), an odd hop and the fused MFCC epilogue keep one-signal tiles
    (F32, 1024, 256, mel(80), "power@41", "r32x16_f32", "r32x16_sched"),
    (F32, 1024, 256, mel(80), "magnitude@41", "r32x16_f32", "r32x16_sched"),
    (F32, 1024, 256, mel(80), "db@41", "r32x16_f32", "r32x16_sched"),
    (F32, 1024, 400, mel(80), "power@41", "r32x16_f32", "r32x16_sched"),
    (F32, 1024, 256, mel(128, 20.0, 7600.0, SR, "slaney"), "power@41", "r32x16_f32", "r32x16_sched"),
    (F32, 1024, 256, mel(128, 20.0, 7600.0, SR, "slaney"), "power", "r32x16_f32", "r32x16_sched_packed"),
    (F32, 1024, 256, mel(80), "power", "r32x16_f32", "r32x16_sched_packed"),
    (F32, 1024, 256, mel(80), "magnitude", "r32x16_f32", "r32x16_sched_packed"),
    (F32, 1024, 256, mel(80), "db", "r32x16_f32", "r32x16_sched_packed"),
    (F32, 1024, 256, mel(128), "power", "r32x16_f32", "r32x16_sched_packed"),
    (F32, 1024, 256, mel(129), "power", "r32x16_f32", "r32x16_csr"),       # past the schedule's 128 bands
    (F32, 1024, 256, mel(200), "power", "r32x16_f32", "r32x16_csr"),
    (F32, 1024, 256, mel(200), "magnitude", "r32x16_f32", "r32x16_csr"),
    (F32, 1024, 256, mel(200), "db", "r32x16_f32", "r32x16_csr"),
    (F32, 1024, 256, mel(1), "power", "r32x16_f32", "r32x16_mfma"),        # one row of one block
    (F32, 1024, 256, mel(2), "power", "r32x16_f32", "r32x16_mfma"),
    (F32, 1024, 256, mel(8), "power", "r32x16_f32", "r32x16_mfma"),
    (F32, 1024, 256, erb(2), "power", "r32x16_f32", "r32x16_mfma"),
    (F32, 1024, 256, erb(17), "power", "r32x16_f32", "r32x16_mfma"),       # a block of one row
    (F32, 1024, 256, erb(40), "power", "r32x16_f32", "r32x16_mfma"),
    (F32, 1024, 256, erb(64), "power", "r32x16_f32", "r32x16_mfma"),
    (F32, 1024, 256, erb(64), "magnitude", "r32x16_f32", "r32x16_mfma"),
    (F32, 1024, 256, erb(64), "db", "r32x16_f32", "r32x16_mfma"),
    (F32, 1024, 256, erb(129), "power", "r32x16_f32", "r32x16_mfma"),      # 9 blocks on 4 waves
    (F32, 1024, 256, mel(23, 300.0, 3400.0), "power", "r32x16_f32", "r32x16_sched_packed"),  # most bins uncovered
    (F32, 1024, 256, MEL48K, "power", "r32x16_f32", "r32x16_sched_packed"),
    # 17 bands, 48.8 non-zeros per row: block 0 covers bins 64 .. 456 (len4 99, tail 3), block 1 one row on bins 404 .. 511 (len4 27, tail 3)
    (F32, 1024, 256, mel(17, 1000.0, 8000.0), "power", "r32x16_f32", "r32x16_mfma"),
    (F32, 1024, 256, loghz(1), "power", "r32x16_f32", "r32x16_sched_packed"),
    (F32, 1024, 256, loghz(96), "power", "r32x16_f32", "r32x16_sched_packed"),
    (F32, 1024, 256, loghz(300), "power", "r32x16_f32", "r32x16_csr"),
    (F32, 1024, 256, CHROMA[0], "chroma", "r32x16_f32", "r32x16_mfma"),    # rows that are not runs
    (F32, 1024, 256, CHROMA[1], "chroma", "r32x16_f32", "r32x16_mfma"),
    (F32, 1024, 256, CHROMA[2], "chroma", "r32x16_f32", "r32x16_mfma"),
    (F32, 1024, 256, CHROMA[3], "chroma", "r32x16_f32", "r32x16_mfma"),
    (F32, 1024, 400, mel(80), "power", "r32x16_f32", "r32x16_sched_packed"),      # per-lane loads
    (F32, 1024, 400, erb(64), "power", "r32x16_f32", "r32x16_mfma"),
    (F32, 1024, 255, mel(80), "power", "r32x16_f32", "r32x16_sched"),      # odd hop: one-signal tiles
    (F32, 1024, 255, mel(200), "power", "r32x16_f32", "r32x16_csr"),
    (F32, 1024, 256, mel(40), "mfcc", "r32x16_f32", "r32x16_sched_mfcc"),
    (F32, 1024, 256, mel(80), "mfcc", "r32x16_f32", "r32x16_sched_mfcc"),
    (F32, 1024, 256, mel(97), "mfcc", "r32x16_f32", "r32x16_sched_packed+mfcc_acc"),  # past the fused epilogue's 96 bands
    # f32 512: two frames per transform
    # hop 256 has the shorter word budget (kMelMaxWordsH256), and WIDE rows overflow it: Mel 2 is the last bank that does not fit
    # (it does at hop 128), Mel 3 the first that does; at the other end 128 bands are the schedule's own limit at every hop
    (F32, 512, 256, mel(2), "power", "reg_radix", "reg_radix_bands"),
    (F32, 512, 256, mel(3), "power", "r32x16_f32", "r32x16_sched512"),
    (F32, 512, 256, mel(128), "power", "r32x16_f32", "r32x16_sched512"),
    (F32, 512, 256, mel(129), "power", "reg_radix", "reg_radix_bands"),
    (F32, 512, 128, mel(2), "power", "r32x16_f32", "r32x16_sched512"),
    (F32, 512, 128, mel(80), "power", "r32x16_f32", "r32x16_sched512"),
    (F32, 512, 128, mel(80), "db", "r32x16_f32", "r32x16_sched512"),
    (F32, 512, 160, mel(80), "power", "r32x16_f32", "r32x16_sched512"),
    (F32, 512, 160, mel(40), "mfcc", "r32x16_f32", "r32x16_sched512+mfcc_acc"),
    (F32, 512, 64, mel(80), "power", "r32x16_f32", "r32x16_sched512"),
    (F32, 512, 150, mel(80), "power", "reg_radix", "reg_radix_bands"),     # an unlisted even hop
    # f32 2048 / 4096
    (F32, 2048, 512, mel(80), "power", "r32x32_f32", "r32x32_sched"),
    (F32, 2048, 512, loghz(96), "power", "r32x32_f32", "r32x32_sched"),
    (F32, 2048, 512, loghz(300), "power", "reg_radix", "reg_radix_bands"), # leaves the tuned kernel (600 two-weight rows of schedule)
    (F32, 2048, 512, erb(64), "power", "reg_radix", "reg_radix_csr"),
    (F32, 2048, 512, CHROMA[2], "chroma", "reg_radix", "reg_radix_bands"),
    (F32, 4096, 1024, mel(80), "power", "r64x32_f32", "r64x32_sched"),
    (F32, 4096, 1024, erb(129), "power", "r64x32_f32", "r64x32_sched"),
    (F32, 4096, 1024, erb(129), "magnitude", "r64x32_f32", "r64x32_sched"),
    (F32, 4096, 1024, erb(129), "db", "r64x32_f32", "r64x32_sched"),
    (F32, 4096, 1024, CHROMA[2], "chroma", "r64x32_f32", "r64x32_sched"),
    (F32, 4096, 2048, mel(80), "power", "r64x32_f32", "bank_rows"),        # hop past the fused stage's staging: per-bin power, then k_bank_rows
    (F32, 4096, 2048, mel(80), "magnitude", "r64x32_f32", "bank_rows"),
    (F32, 4096, 2048, mel(80), "db", "r64x32_f32", "bank_rows"),
    # f64 1024
    (F64, 1024, 256, mel(8), "power", "d32x16_f64", "d32x16_sched"),
    (F64, 1024, 256, mel(9), "power", "reg_radix", "reg_radix_bands"),     # the neighbour on another kernel
    (F64, 1024, 256, mel(128), "power", "d32x16_f64", "d32x16_sched"),
    (F64, 1024, 256, mel(128), "magnitude", "d32x16_f64", "d32x16_sched"),
    (F64, 1024, 256, mel(128), "db", "d32x16_f64", "d32x16_sched"),
    (F64, 1024, 256, mel(129), "power", "d32x16_f64", "d32x16_sched"),
    (F64, 1024, 256, mel(200), "power", "reg_radix", "reg_radix_bands"),
    (F64, 1024, 256, mel(200), "magnitude", "reg_radix", "reg_radix_bands"),
    (F64, 1024, 256, mel(200), "db", "reg_radix", "reg_radix_bands"),
    (F64, 1024, 256, loghz(96), "power", "d32x16_f64", "d32x16_sched"),
    (F64, 1024, 256, loghz(300), "power", "reg_radix", "reg_radix_bands"),
    (F64, 1024, 256, erb(64), "power", "reg_radix", "reg_radix_csr"),
    (F64, 1024, 256, erb(64), "magnitude", "reg_radix", "reg_radix_csr"),
    (F64, 1024, 256, erb(64), "db", "reg_radix", "reg_radix_csr"),
    (F64, 1024, 256, mel(40), "mfcc", "d32x16_f64", "d32x16_sched+mfcc_acc"),
    (F64, 1024, 255, mel(40), "power", "d32x16_f64", "d32x16_sched"),      # odd hop
    # f64 512.  k_d512 takes signals of 16 frames and more; with the 9 frames of a probe the CALL steps down to the register-tiled kernel
    # while sgx_kernel_name still names the plan's kernel (pinned by the first case).  The others run 17 frames ("@17").
    (F64, 512, 128, mel(8), "power", "d512_f64", "reg_radix_bands"),
    (F64, 512, 128, mel(8), "power@17", "d512_f64", "d512_sched"),
    (F64, 512, 128, mel(129), "power@17", "d512_f64", "d512_sched"),       # one-bin rows
    (F64, 512, 128, mel(200), "power", "reg_radix", "reg_radix_bands"),
    (F64, 512, 128, MEL48K, "power@17", "d512_f64", "d512_sched"),         # empty rows on the tuned kernel
    (F64, 512, 256, mel(8), "power@17", "d512_f64", "d512_sched"),
    (F64, 512, 256, mel(129), "power@17", "d512_f64", "d512_sched"),
    (F64, 512, 256, mel(200), "power", "reg_radix", "reg_radix_bands"),
    (F64, 512, 256, MEL48K, "power@17", "d512_f64", "d512_sched"),
    (F64, 512, 128, MEL48K, "db@17", "d512_f64", "d512_sched"),
    # f64 2048
    (F64, 2048, 512, mel(300), "power", "d32x32_f64", "bank_rows"),         # the schedule overflows: split
    (F64, 2048, 512, mel(300), "magnitude", "d32x32_f64", "bank_rows"),
    (F64, 2048, 512, mel(300), "db", "d32x32_f64", "bank_rows"),
    (F64, 2048, 512, erb(129), "power", "d32x32_f64", "d32x32_sched"),
    (F64, 2048, 512, erb(129), "magnitude", "d32x32_f64", "d32x32_sched"),
    (F64, 2048, 512, erb(129), "db", "d32x32_f64", "d32x32_sched"),
    (F64, 2048, 512, CHROMA[2], "chroma", "d32x32_f64", "d32x32_sched"),
    (F64, 2048, 512, mel(400), "mfcc", "d32x32_f64", "bank_rows+mfcc_rows"),  # 400 x 16 f64 basis values: past k_mfcc_acc's LDS
    # generic kernels, chirp-z, global-memory transforms
    (F32, 400, 160, mel(40), "power", "reg_radix", "reg_radix_bands"),     # fused ...
    (F64, 400, 160, mel(40), "power", "reg_radix", "bank_rows"),           # ... against split (f64 composite size)
    (F32, 400, 160, mel(200), "power", "reg_radix", "reg_radix_bands"),    # empty rows
    (F64, 400, 160, mel(200), "power", "reg_radix", "bank_rows"),
    (F32, 400, 160, MEL48K, "power", "reg_radix", "reg_radix_bands"),
    (F64, 400, 160, MEL48K, "power", "reg_radix", "bank_rows"),
    (F32, 400, 160, erb(64), "power", "reg_radix", "reg_radix_csr"),
    (F32, 400, 160, erb(64), "magnitude", "reg_radix", "reg_radix_csr"),
    (F32, 400, 160, erb(64), "db", "reg_radix", "reg_radix_csr"),
    (F32, 400, 160, mel(40), "mfcc", "reg_radix", "reg_radix_bands+mfcc_acc"),
    (F32, 256, 64, mel(40), "power", "reg_radix", "reg_radix_bands"),
    (F64, 256, 64, mel(40), "power", "reg_radix", "reg_radix_bands"),
    (F32, 16, 4, mel(4), "power", "lds_radix2", "generic_csr"),
    (F64, 16, 4, mel(4), "power", "lds_radix2", "generic_csr"),
    (F32, 15, 4, mel(4), "power", "two_factor_dft", "generic_csr"),
    (F64, 13, 4, mel(4), "power", "direct_dft", "generic_csr"),
    (F32, 401, 160, mel(40), "power", "bluestein", "bluestein_rows"),      # in-kernel rows
    (F32, 401, 160, mel(40), "db", "bluestein", "bluestein_rows"),
    (F64, 401, 160, mel(40), "power", "bluestein", "bank_rows"),
    (F32, 2003, 500, mel(80), "power", "bluestein", "bank_rows"),
    (F32, 9001, 2250, mel(80), "power", "big_chirpz", "bank_rows"),        # edge-bin probe list
]


def case_id(c):
    b = c[3]
    tag = "-".join(str(v if not isinstance(v, float) else int(v)) for v in b)
    return f"{c[0][5:]}-{c[1]}-{c[2]}-{tag}-{c[4]}"


BANKS = sorted({(c[1], c[3]) for c in CASES}, key=repr)


# ---- CPU: names, table, weights -------------------------------------------------------------------------------------------------
def test_names_agree_with_the_comment_beside_the_setter():
    src = open(os.path.join(os.path.dirname(_ffi.__file__), "csrc", "plan.hip")).read()
    i = src.index("Every name — keep tests/test_bank_readback.py's NAMES in step")
    block = src[i:src.index("void note_bank_stage", i)]
    found = set(re.findall(r'"([a-z0-9_+]+)"', block))
    assert found == NAMES | SUFFIXES
    # and every name a launcher passes is in that list
    csrc = os.path.join(os.path.dirname(_ffi.__file__), "csrc")
    passed = set()
    for f in os.listdir(csrc):
        for m in re.finditer(r'note_bank_stage\(([^;]*)\);', open(os.path.join(csrc, f)).read()):
            passed |= set(re.findall(r'"([a-z0-9_+]+)"', m.group(1)))
    assert passed == NAMES | SUFFIXES


def split_stage(stage):
    base, plus, suf = stage.partition("+")
    return base, plus + suf


def test_table_names_are_known_names():
    for c in CASES:
        base, suf = split_stage(c[6])
        assert base in NAMES and (suf == "" or suf in SUFFIXES), c
    assert len({case_id(c) for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_table_selects_the_named_kernel(case):
    dtype, n_fft, hop, bank, out, kernel, _ = case
    plan = make_plan(dtype, n_fft, hop, bank, out, device=HOST)
    assert plan.kernel_name == kernel
    assert plan.bank_stage_name == ""  # nothing has run


def test_stage_name_is_empty_without_a_bank():
    params = sg.SpectrogramParams(sg.StftParams(1024, 256, sg.WindowType.hanning, True), SR)
    assert sg.Plan(params, _ffi.AMP_POWER, None, None, F32, device=HOST).bank_stage_name == ""


@pytest.mark.parametrize("n_fft,bank", BANKS, ids=lambda v: str(v).replace(" ", ""))
def test_plan_table_matches_the_independent_bank(n_fft, bank):
    """Same columns; values within E (w_tol) -- the same E the GPU bound grants the reference."""
    T = table_dense(make_plan(F64, n_fft, max(1, n_fft // 4), bank, "chroma" if bank[0] == "chroma" else "power",
                              device=HOST), n_fft // 2 + 1)
    W = bank_w64(bank, n_fft)
    assert T.shape == W.shape
    assert np.array_equal(T != 0, W != 0)
    assert np.all(np.abs(T - W) <= w_tol(bank, W, n_fft))


# ---- probes ----------------------------------------------------------------------------------------------------------------------
def probe_bins(W, n_fft):
    nb = n_fft // 2 + 1
    if nb <= 1025:
        return np.arange(nb)
    four = [0, 1, n_fft // 2 - 1, n_fft // 2]
    L = np.count_nonzero(W, axis=1)
    if np.all(L == nb):  # dense rows have no edges
        return np.unique(np.concatenate([np.round(np.linspace(0, nb - 1, 257)).astype(int), four]))
    bins = list(four)
    for m in range(W.shape[0]):
        nz = np.flatnonzero(W[m])
        if nz.size:
            bins += [nz[0], nz[-1], max(nz[0] - 1, 0), min(nz[-1] + 1, nb - 1), int(np.argmax(W[m]))]
    return np.unique(np.asarray(bins, int))


def n_samples(hop, nf):
    """nf centred frames for even and odd n_fft: n // hop + 1 = (n - 1) // hop + 1 = nf."""
    return (nf - 1) * hop + 1


def probe_batch(n_fft, hop, bins, dtype, nf=NFRAMES, seed=11):
    rng = np.random.default_rng(seed)
    t = np.arange(n_samples(hop, nf))
    phi = rng.uniform(0.0, 2.0 * np.pi, len(bins))
    # (k t mod n_fft keeps the argument exact for the long frames)
    return (0.5 * np.cos(2.0 * np.pi * ((np.asarray(bins)[:, None] * t[None, :]) % n_fft) / n_fft + phi[:, None])).astype(NP[dtype])


@functools.lru_cache(maxsize=1)
def _spectra(dtype, n_fft, hop, bins, window, nf=NFRAMES):
    x = probe_batch(n_fft, hop, np.asarray(bins), dtype, nf)
    x64 = x.astype(np.float64)
    w = np.asarray(window, np.float64)
    X = np.stack([H.np_stft(r, n_fft, hop, w) for r in x64])
    assert X.shape[2] == nf
    return x, x64, np.abs(X)


def rows(W, A):
    """[m, k] x [b, k, f] -> [b, m, f] (W is zero outside a row's non-zeros, so this is the sum over the non-zeros only)."""
    return np.tensordot(W, A, axes=([1], [1])).transpose(1, 0, 2)


def band_ref_and_bound(W, E, A, d, dtype, mag_in):
    """Reference W64 . P64 and d_mf for spectrum magnitudes A [b, k, f] and delta_f d [b, f]."""
    D = d[:, None, :]
    P, dP = (A, np.broadcast_to(D, A.shape)) if mag_in else (A * A, D * (2.0 * A + D))
    L = np.count_nonzero(W, axis=1)[None, :, None]
    ref = rows(W, P)
    return ref, rows(W, dP) + (L + 2) * U[dtype] * ref + rows(E, P)


def db_extra(dtype, ref_db):
    return 2e-5 if dtype == "float32" else 4e-15 + 3e-16 * np.abs(ref_db)


def out_ref_and_bound(bank, out, ref, d, dtype):
    """Carry (ref, d) of the band values to the plan's output."""
    u = U[dtype]
    if out == "power":
        return ref, d
    if out == "magnitude":
        r = np.sqrt(ref)
        return r, np.maximum(r - np.sqrt(np.maximum(ref - d, 0.0)), np.sqrt(ref + d) - r) + 2.0 * u * np.sqrt(ref + d)
    if out == "db":
        eps = 10.0 ** (FLOOR / 10.0)
        r = 10.0 * np.log10(np.maximum(ref, eps))
        return r, (10.0 / math.log(10.0)) * np.log1p(d / np.maximum(ref, eps)) + db_extra(dtype, r)
    if out == "mfcc":
        eps = 10.0 ** (MFCC_FLOOR / 10.0)
        D = 10.0 * np.log10(np.maximum(ref, eps))
        dD = (10.0 / math.log(10.0)) * np.log1p(d / np.maximum(ref, eps)) + db_extra(dtype, D)
        nm = ref.shape[1]
        B = np.cos(np.pi * np.arange(13)[:, None] * (np.arange(nm)[None, :] + 0.5) / nm)
        lift = 1.0 + 11.0 * np.sin(np.pi * np.arange(13) / 22.0)
        r = np.einsum("ci,bif->bcf", B, D) * lift[None, :, None]
        b = (np.einsum("ci,bif->bcf", np.abs(B), dD) + (nm + 3) * u * np.einsum("ci,bif->bcf", np.abs(B), np.abs(D))) * lift[None, :, None]
        return r, b
    assert out == "chroma"
    norm = bank[1]
    if norm == "none":
        return ref, d
    s = {"l1": lambda v: np.sum(np.abs(v), axis=1, keepdims=True), "l2": lambda v: np.sqrt(np.sum(v * v, axis=1, keepdims=True)),
         "max": lambda v: np.max(np.abs(v), axis=1, keepdims=True)}[norm]
    sv, ds = s(ref), s(d)
    ok = sv - ds > 0
    y = ref / np.where(sv > 0, sv, 1.0)
    b = (d + np.abs(y) * ds) / np.where(ok, sv - ds, 1.0)
    return y, np.where(ok, b, np.inf)  # (frames whose norm the bound cannot tell from 0: not asserted)


def ratio(got, ref, bound):
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / bound)  # (bound 0 and an error: inf; bound inf: 0)


def report(name, r):
    WORST[name] = max(WORST.get(name, 0.0), float(r))
    print(f"{name}: worst ratio to bound {WORST[name]:.3g}")


# ---- CPU calibration -------------------------------------------------------------------------------------------------------------
def f32_model(x, w, n_fft, hop, W64, mag_in):
    """The stage in f32 on the CPU: rfft of f32 frames, f32 re^2 + im^2, f32 weights, rows summed un-fused in ascending-bin order."""
    import scipy.fft

    fr = np.stack([H.np_frames(r, n_fft, hop, True) for r in x.astype(np.float32)]) * w.astype(np.float32)[None, None, :]
    assert fr.dtype == np.float32
    X = scipy.fft.rfft(fr, axis=-1)
    assert X.dtype == np.complex64
    P = X.real * X.real + X.imag * X.imag
    if mag_in:
        P = np.sqrt(P)
    P = np.ascontiguousarray(P.transpose(2, 0, 1))  # [k, b, f]
    W32 = W64.astype(np.float32)
    out = np.zeros((W32.shape[0],) + P.shape[1:], np.float32)
    for m in range(W32.shape[0]):
        for k in np.flatnonzero(W32[m]):
            out[m] = out[m] + W32[m, k] * P[k]
    return out.transpose(1, 0, 2).astype(np.float64)


CALIBRATION = [(1024, 256, mel(80)), (1024, 256, loghz(96)), (1024, 256, erb(64)), (1024, 256, ("chroma", "none")), (400, 160, mel(40))]


@pytest.mark.parametrize("n_fft,hop,bank", CALIBRATION, ids=lambda v: str(v).replace(" ", ""))
def test_bound_calibration_f32_model_meets_mutants_break(n_fft, hop, bank):
    nb = n_fft // 2 + 1
    mag_in = bank[0] == "chroma"
    plan = make_plan(F32, n_fft, hop, bank, "chroma" if mag_in else "power", device=HOST)
    w = np.asarray(plan.window(), np.float64)
    W = bank_w64(bank, n_fft)
    E = w_tol(bank, W, n_fft)
    bins = tuple(int(k) for k in probe_bins(W, n_fft))
    x, x64, A = _spectra(F32, n_fft, hop, bins, tuple(w))
    d = frame_deltas(x64, w, n_fft, hop, F32, 4.0, n_fft, False)
    ref, bound = band_ref_and_bound(W, E, A, d, F32, mag_in)
    worst = float(np.max(ratio(f32_model(x, w, n_fft, hop, W, mag_in), ref, bound)))
    report(f"cpu model {case_id((F32, n_fft, hop, bank, 'power'))}", worst)
    assert 1e-4 < worst <= 0.5  # (meets it with room; not vacuous)
    m = W.shape[0] // 2
    nz = np.flatnonzero(W[m])
    dense = nz.size == nb
    step = 1e-3 if np.count_nonzero(W) >= 48 * W.shape[0] else 1e-4
    mutants = {}
    Wm = W.copy(); Wm[m, nz[0]] = 0.0
    mutants["first weight dropped"] = Wm
    if not dense:  # (a dense ERB row has no outside, and rolling it moves every weight: nothing structural to tell apart)
        # Magnitude-domain rows (chroma) cannot show 1e-6 max(row): every bin of the row carries dP = delta_f whether it holds energy or
        # not, so off the tone d = delta_f sum_k W_mk (the rows sum to 1) while the spurious weight adds w |X_k|; delta_f / |X_k| =
        # 4 u 10 sqrt(1024) ||x w|| / |X_k| = 4.2e-6 for a Hann-windowed tone, and max(row) = 0.02: w must pass 2e-4 max(row).  Asserted
        # there at the next decade, 1e-3 max(row); the 1e-6 figure is printed (measured 0.0099 x the bound).
        out_w = 1e-3 if mag_in else 1e-6
        Wm = W.copy(); Wm[m, nz[-1] + 1] = out_w * W[m].max()
        mutants[f"{out_w:g} max(row) outside"] = Wm
        if mag_in:
            Wm = W.copy(); Wm[m, nz[-1] + 1] = 1e-6 * W[m].max()
            mutants["(information) 1e-06 max(row) outside"] = Wm
        Wm = W.copy(); Wm[m] = np.roll(W[m], 1)
        mutants["rolled one bin"] = Wm
    Wm = W.copy(); Wm[m, int(np.argmax(W[m]))] *= 1.0 + step
    mutants[f"one weight x (1 + {step:g})"] = Wm
    for what, Wm in mutants.items():
        sub = np.zeros_like(W)
        sub[m] = Wm[m]  # (only the mutated row is recomputed)
        got = f32_model(x, w, n_fft, hop, sub, mag_in)[:, m, :]
        r = float(np.max(ratio(got, ref[:, m, :], bound[:, m, :])))
        print(f"  {what}: {r:.3g} x the bound")
        assert r > 1.0 or what.startswith("(information)"), (what, r)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def run_case(case):
    """-> (kernel name, stage name, worst ratio, where)."""
    dtype, n_fft, hop, bank, out, _, _ = case
    nb = n_fft // 2 + 1
    mag_in = bank[0] == "chroma"
    plan = make_plan(dtype, n_fft, hop, bank, out)
    out, nf = split_out(out)
    kernel = plan.kernel_name
    assert plan.bank_stage_name == ""
    w = np.asarray(plan.window(), np.float64)
    W = bank_w64(bank, n_fft)
    E = w_tol(bank, W, n_fft)
    bins = tuple(int(k) for k in probe_bins(table_dense(make_plan(F64, n_fft, hop, bank, "chroma" if mag_in else "power", device=HOST), nb), n_fft))
    x, x64, A = _spectra(dtype, n_fft, hop, bins, tuple(w), nf)
    got = np.array(plan.compute_batch(x)).astype(np.float64)
    stage = plan.bank_stage_name
    assert got.shape[0] == len(bins) and got.shape[2] == nf and np.all(np.isfinite(got))
    c = CB.get(kernel, 4.0)
    Neff = chirp_m(n_fft) if kernel in ("bluestein", "big_chirpz") else n_fft
    d = frame_deltas(x64, w, n_fft, hop, dtype, c, Neff, paired(kernel, dtype, n_fft))
    ref, bound = band_ref_and_bound(W, E, A, d, dtype, mag_in)
    empty = np.count_nonzero(W, axis=1) == 0
    oref, obound = out_ref_and_bound(bank, out, ref, bound, dtype)
    if empty.any() and out in ("power", "magnitude", "db"):
        assert np.all(got[:, empty, :] == (FLOOR if out == "db" else 0.0)), "a row without weights is not exactly the oracle's value"
    r = ratio(got, oref, obound)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    where = f"probe bin {bins[i[0]]}, row {i[1]}, frame {i[2]}: got {got[i]:.9g} ref {oref[i]:.9g} bound {obound[i]:.3g}"
    return kernel, stage, float(r[i]), where


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gpu_bank_reads_back_every_weight(case):
    kernel, stage, worst, where = run_case(case)
    print(f"{stage} [{case_id(case)}]: worst ratio to bound {worst:.3g}")
    assert (kernel, stage) == (case[5], case[6])
    SEEN.add(stage)
    key = f"{split_stage(stage)[0]} {case[0]} {'dB / MFCC' if split_out(case[4])[0] in ('db', 'mfcc') else 'linear'}"
    WORST[key] = max(WORST.get(key, 0.0), worst)
    assert worst <= 1.0, (case_id(case), where)


@pytest.mark.gpu
def test_gpu_sweep_reached_every_stage_name():
    """Runs last: every name of NAMES and every MFCC suffix was met by a passing name assertion; prints the worst ratio per stage."""
    for key in sorted(WORST):
        if key.split(" ")[0] in NAMES:
            print(f"{key}: worst |got - ref| / d = {WORST[key]:.2g}")
    assert {split_stage(s)[0] for s in SEEN} >= NAMES
    assert {split_stage(s)[1] for s in SEEN} - {""} >= SUFFIXES
