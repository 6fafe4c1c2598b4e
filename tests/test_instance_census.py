"""Every compiled instance of k_fir_os, k_welch, k_minphase and k_resample_pp is launched by a named GPU case.

1. The census (no GPU).  The instance lists are parsed from the sources: SGX_FIR_SPLITS_F32 / _F64 (fir.hip), SGX_WELCH_SPLITS_F32 /
   _F64 times the three kinds (welch.hip), the SGX_RS_CASE(..) list times the two types (resample.hip), the powers of two
   1 .. kMaxFusedN (minphase.hip).  CENSUS holds the GPU cases of this file per family; each row names the instance it is meant to
   launch and is verified on a host-only plan (kernel name, transform length, the split through tests/test_forward_readback.py's
   restated reg_split_len; for the resampler K, L and the restated choose_route: G, W, work items, LDS bytes).
   test_every_compiled_instance_has_a_case asserts that the instances CENSUS names plus those the owning files' own lists reach
   (tests/test_fir.py FUSED_TAPS, tests/test_welch.py FUSED x its kinds, tests/test_minphase.py FUSED, tests/test_resample.py
   RATIOS) are exactly the parsed ones; an instance no call can reach goes into UNREACHABLE with the line of code that makes it so
   (none today).  The comparison can fail: on a copy of each source with one instance added, and with one removed, it reports that
   instance and nothing else.

2. The GPU cases use the reference, bound and constants of the file that owns the route; no tolerance is set here.
   FIR        tests/test_fir.py (direct sums, the per-segment bound): taps 65, 100, 128 (P = 512), 257, 400, 512 (P = 2048) and the
              first taps of the next splits 129, 513, with 256; ragged lengths, batch 1 and batch 5 with a response per row, both
              forms.  Tile seams: per P = 256 .. 4096, taps = P / 4, a row of 2 tile + 1 and one of tile + 1 segments (tile restated
              from launch_os), a 10^6 : 1 level step right behind the first sample the second tile writes and, in a second pass, at
              the first sample it reads.
   Welch      tests/test_welch.py (extended-precision restatement for f64, the coherence bound inside its range, asserted on the
              reference alone for every m before the GPU is touched): coherence at n = 512 and 4096, hop n / 4,
              m = 1, tile - 1, tile, tile + 1, 2 tile + 1; coherence(x, x) within 8 u of 1 and csd(x, x) bit-equal to welch(x).
   Min. phase tests/test_minphase.py (its restatement and first-order bound, the all-zero criterion): SHORT_FUSED there, n = 4, 8,
              16, 32, 128, 256, 1024, batch 3, every kind, out_len below and above n.
   Resampler  tests/test_resample.py (per-sample bound, streaming bit-equality) and tests/test_resample_readback.py (impulse
              read-back with == on every element, the f32 chain: at most 1 output in 10^4 off it, none by more than 4 spacings):
              RS_ROWS below: KB = 8, 48, 56, 64 (and K = 64 itself), workgroups of 320 and 512 work items, W = 1, tiles between the
              32 KiB aim and the 64 KiB budget, the budget edges K = 65, L = 513 and an f64 tile past 64 KiB on resample_generic, a
              Kaiser table and a width-16 table.

3. Every GPU case records its worst ratio to the owning file's bound; test_gpu_worst_ratios_per_family prints the table.  Measured on
   an MI355X (information, not thresholds; DESIGN.md 6.3 keeps the same table):
     | family            | instance                                             | f32                       | f64                                |
     | k_fir_os          | P = 256 / 512 / 1024                                 | 0.0116 / 0.0110 / 0.0076  | 0.0121 / 0.0135 / 0.0082           |
     |                   | P = 2048 / 4096                                      | 0.0075 / 0.0040           | 0.0064 / 0.0072                    |
     | k_welch coherence | n = 512 / 4096                                       | 0.0051 / 0.0079           | 0.0106 / 0.0082                    |
     | k_minphase        | n = 4 / 8 / 16 / 32                                  | 0.78 / 0.86 / 0.89 / 0.87 | 0.014 / 0.0068 / 0.0057 / 0.0023   |
     |                   | n = 128 / 256 / 1024                                 | 0.97 / 0.93 / 0.99        | 5.7e-4 / 4.9e-4 / 1.7e-4           |
     | k_resample_pp     | KB = 8 (W = 16)                                      | 0.476                     | 0.479                              |
     |                   | KB = 16, 320 / 512 work items                        | 0.247 / 0.289             | 0.246 / 0.339                      |
     |                   | KB = 32, 512 work items, W = 1                       | 0.121                     | 0.105                              |
     |                   | KB = 40, Kaiser / width 16                           | 0.165 / 0.203             | 0.178 / 0.170                      |
     |                   | KB = 48                                              | 0.145                     | 0.109                              |
     |                   | KB = 56, 256 / 512 work items                        | 0.139 / 0.105             | 0.112 / 0.159 (W = 1)              |
     |                   | KB = 64, 256 work items: 5 : 1 and 21 : 4 / 31 : 1   | 0.101 / 0.045             | 0.091 / 0.054                      |
     |                   | KB = 64, 512 work items: 2600 : 509 / 15000 : 511    | 0.082 / 0.065             | 0.114 / generic                    |
     | resample_generic  | K = 65, L = 513, f64 15000 : 511                     | 0.286                     | 0.285                              |
   The f32 chain: 0 outputs off it in all 19 rows (2 313 .. 73 785 outputs per row).  An f32 minimum-phase plan sits just under 1 by
   construction: its bound is the f64 bound plus the one rounding to f32, 2^-24 |y|, and the result is computed in f64 and rounded once.
   Nothing was found wrong in any newly launched instance.  179 GPU cases, 7 s when run alone.
"""
import collections
import functools
import os
import re

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests import test_fir as TF
from tests import test_forward_readback as FR
from tests import test_minphase as TM
from tests import test_resample as TR
from tests import test_resample_readback as RB
from tests import test_welch as TW

F32, F64 = "float32", "float64"
DTYPES = (F32, F64)
ELEM = {F32: 4, F64: 8}
HOST = _ffi.DEVICE_HOST_ONLY
CSRC = os.path.join(os.path.dirname(os.path.abspath(_ffi.__file__)), "csrc")
SOURCES = ("fir.hip", "welch.hip", "minphase.hip", "resample.hip")
WELCH_KINDS = ("psd", "csd", "coherence")
WORST = {}


def record(family, instance, ratio):
    WORST[(family, instance)] = max(WORST.get((family, instance), 0.0), float(ratio))


# ---- 1. the parsed instance lists ------------------------------------------------------------------------------------------------------
def read_sources():
    return {name: open(os.path.join(CSRC, name)).read() for name in SOURCES}


def parse_sources(texts):
    """family -> the set of compiled instances: fir (dtype, (A, B, C)); welch (dtype, (A, B, C), kind); minphase n; resample (dtype, KB)."""
    fir = {(dt, s) for dt, tag in ((F32, "F32"), (F64, "F64")) for s in FR._xmacro(texts["fir.hip"], "SGX_FIR_SPLITS_" + tag)}
    welch = {(dt, s, k) for dt, tag in ((F32, "F32"), (F64, "F64")) for s in FR._xmacro(texts["welch.hip"], "SGX_WELCH_SPLITS_" + tag)
             for k in WELCH_KINDS}
    top = int(re.search(r"constexpr size_t kMaxFusedN = (\d+)\b", texts["minphase.hip"]).group(1))
    minphase = {1 << l for l in range(top.bit_length()) if 1 << l <= top}
    resample = {(dt, int(kb)) for kb in re.findall(r"SGX_RS_CASE\((\d+)\)", texts["resample.hip"]) for dt in DTYPES}
    return {"fir": fir, "welch": welch, "minphase": minphase, "resample": resample}


def test_the_parser_sees_the_sources():
    texts = read_sources()
    parsed = parse_sources(texts)
    for fam in ("fir", "welch"):
        for dt in DTYPES:
            assert len({i[1] for i in parsed[fam] if i[0] == dt}) >= 5, (fam, dt)
    assert len(parsed["welch"]) == 3 * len({i[:2] for i in parsed["welch"]})
    # the kinds are the three the launcher switches over, and the resampler's list is what its switch compiles
    assert all(k in texts["welch.hip"] for k in ("KIND_PSD", "KIND_CSD", "KIND_COH"))
    assert len({kb for _, kb in parsed["resample"]}) >= 8 and all(kb % 8 == 0 for _, kb in parsed["resample"])
    assert max(parsed["minphase"]) == 4096 and len(parsed["minphase"]) == 13
    # the fused routes' splits are reg_split_len's of the powers of two 256 .. 4096, as restated in tests/test_forward_readback.py
    for dt in DTYPES:
        want = {(dt, FR.reg_split_len(P, dt)) for P in FIR_P}
        assert {i for i in parsed["fir"] if i[0] == dt} == want == {i[:2] for i in parsed["welch"] if i[0] == dt}


# ---- CENSUS: FIR ---------------------------------------------------------------------------------------------------------------------------
FIR_P = (256, 512, 1024, 2048, 4096)
# taps -> the P it is meant to launch: 65, 100, 128 and 257, 400, 512 the splits no other file reaches; 129, 256, 513 the other sides of
# the edges 128 | 129, 256 | 257, 512 | 513 (at 64, 128, 256, 512 taps L + 1 is exactly P / 4)
FIR_TAPS = {65: 512, 100: 512, 128: 512, 129: 1024, 256: 1024, 257: 2048, 400: 2048, 512: 2048, 513: 4096}
FIR_TILE = {256: 16, 512: 8, 1024: 4, 2048: 2, 4096: 1}  # sequences per workgroup of k_fir_os, both types (launch_os)


def fir_fused_len(taps):
    """fir.hip fused_len: clamp(next_pow2(4 taps), 256, 4096)."""
    return min(4096, max(256, 1 << (4 * taps - 1).bit_length()))


def fused_seq_bytes(split, dtype):
    """fir.hip / welch.hip fused_seq_bytes: rr_frame_stride(A, rr_swizzle(..).rs) complex elements (rr_layout.h)."""
    a, b, c = split
    text = open(os.path.join(CSRC, "rr_layout.h")).read()
    table = {tuple(int(v) for v in m.groups()[:4]): int(m.group(5)) for m in re.finditer(r"\{(8|16), (\d+), (\d+), (\d+), \{(\d+),", text)}
    assert len(table) >= 10
    rs = table.get((2 * ELEM[dtype], a, b, c), b * c + 1)
    return ((a * rs) | 1) * 2 * ELEM[dtype]


def fir_tile(P, dtype):
    """launch_os for a row of more than 8 sequences: the largest power of two <= 16 whose sequences fit the LDS budget."""
    text = open(os.path.join(CSRC, "fir.hip")).read()
    k32, k64 = re.search(r"kFirLds32 = (\d+) \* 1024, kFirLds64 = (\d+) \* 1024;", text).groups()
    assert (int(k32), int(k64)) == (36, 72)
    budget = (int(k64) if dtype == F64 else int(k32)) * 1024
    per = fused_seq_bytes(FR.reg_split_len(P, dtype), dtype)
    tile = 16
    while tile > 1 and tile * per > budget:
        tile //= 2
    assert tile * per <= budget and (tile == 16 or 2 * tile * per > budget)
    return tile


@pytest.mark.parametrize("dtype", DTYPES)
def test_fir_rows_on_host_only_plans(dtype):
    parsed = parse_sources(read_sources())["fir"]
    for taps, P in list(FIR_TAPS.items()) + [(P // 4, P) for P in FIR_P]:
        p = sg.FirPlan(np.ones(taps), dtype=dtype, device=HOST)
        assert (p.kernel_name, p.fft_size, p.step) == ("k_fir_os", P, P - taps + 1) and fir_fused_len(taps) == P
        assert (dtype, FR.reg_split_len(P, dtype)) in parsed
    for taps in (64, 128, 256, 512):  # the edges: L + 1 = P / 4 exactly, and one more tap is the next split
        assert 4 * taps == fir_fused_len(taps) and fir_fused_len(taps + 1) == 8 * taps
    for P in FIR_P:
        assert fir_tile(P, dtype) == FIR_TILE[P]
        # the seam rows hold more than 8 sequences or more than the tile, so launch_os does not shrink the tile to the row
        assert 2 * FIR_TILE[P] + 1 > FIR_TILE[P] + 1 > FIR_TILE[P]
    assert fused_seq_bytes((16, 16, 1), F32) == 273 * 8 and fused_seq_bytes((16, 16, 16), F64) == 4097 * 16


# ---- CENSUS: Welch -------------------------------------------------------------------------------------------------------------------------
WELCH_N = (512, 4096)  # coherence at these lengths, both types
WELCH_INPUTS = (("constant", "noise"), ("linear", "smallramp"))  # (detrend, tests/test_welch.py signal): inside the coherence bound's range
WELCH_FS = 16000.0


def welch_host(n, dtype, kind="coherence", detrend="constant"):
    return sg.WelchPlan(sg.WelchParams(n, n // 4, sg.WindowType.hanning, WELCH_FS, detrend, "density"), kind, dtype, device=HOST)


def welch_counts(tile):
    return sorted({1, tile - 1, tile, tile + 1, 2 * tile + 1} - {0})


def welch_seed(n, m, detrend):
    return 7000 + 10 * m + n // 512 + (1 if detrend == "linear" else 0)


@functools.lru_cache(maxsize=None)
def welch_case(n, dtype, detrend, sname, m):
    """(x, y, reference, bound) of one coherence case: computed once, shared by the range check and the GPU case, not written to."""
    hop = n // 4
    N = n + (m - 1) * hop + 37
    x, y = TW.signals(sname, 3, N, dtype, seed=welch_seed(n, m, detrend))
    w = welch_host(n, dtype).window()
    ref, bound = TW.reference("coherence", x, y, w, n, hop, detrend, "density", WELCH_FS, dtype)  # (asserts its range condition)
    for a in (x, y, ref, bound):
        a.setflags(write=False)
    return x, y, ref, bound


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", WELCH_N)
def test_welch_rows_on_host_only_plans_and_inside_the_bound_s_range(n, dtype):
    parsed = parse_sources(read_sources())["welch"]
    p = welch_host(n, dtype)
    assert (p.kernel_name, p.n_bins, p.tile) == ("k_welch", n // 2 + 1, 32)
    assert (dtype, FR.reg_split_len(n, dtype), "coherence") in parsed
    for detrend, sname in WELCH_INPUTS:
        for m in welch_counts(p.tile):
            x, _, ref, bound = welch_case(n, dtype, detrend, sname, m)  # cond <= 0.1 holds for this seed, or reference() raises
            assert p.n_segments(x.shape[1]) == m and ref.shape == (3, n // 2 + 1) and np.all(np.isfinite(bound))


# ---- CENSUS: minimum phase -----------------------------------------------------------------------------------------------------------------
MINPHASE_N = {(3, 1): 4, (4, 1): 4, (7, 1): 8, (13, 1): 16, (2, 8): 16, (29, 1): 32, (4, 8): 32, (16, 8): 128, (100, 1): 128, (32, 8): 256,
              (128, 8): 1024, (1000, 1): 1024}
assert list(MINPHASE_N) == TM.SHORT_FUSED


def minphase_out_lens(n):
    return (max(1, n - 1), n + 3)  # below and above n (the plan cuts the second to n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_minphase_rows_on_host_only_plans(dtype):
    for (taps, os_), n in MINPHASE_N.items():
        for out_len in minphase_out_lens(n):
            p = sg.MinPhasePlan(taps, out_len, os_, dtype=dtype, device=HOST)
            assert (p.kernel_name, p.fft_size, p.output_length) == ("k_minphase", n, min(out_len, n)) and TM.fft_len(taps, os_) == n


# ---- CENSUS: resampler ---------------------------------------------------------------------------------------------------------------------
KAISER16 = (("lowpass_filter_width", 16), ("rolloff", 0.9475937167399596), ("resampling_method", "sinc_interp_kaiser"), ("beta", TR.KAISER_BETA))
KAISER = (("resampling_method", "sinc_interp_kaiser"), ("beta", TR.KAISER_BETA))
LPW1, LPW3 = (("lowpass_filter_width", 1),), (("lowpass_filter_width", 3),)
# (orig, new, filter keywords, K, L, work items, (W f32, W f64), (LDS bytes of a whole tile f32, f64), what it reaches); W None: the
# generic route.  Every figure is asserted on a host-only plan against the restated choose_route.
RS = collections.namedtuple("RS", "orig new kw K L items W lds what")
RS_ROWS = [
    RS(1, 2, LPW1, 3, 2, 256, (16, 16), (8224, 16448), "KB = 8: one block of 8 taps, no read-ahead"),
    RS(2, 3, LPW1, 3, 3, 256, (16, 16), (10912, 21824), "KB = 8, L = 3: 255 of 256 work items live"),
    RS(1, 3, LPW3, 7, 3, 256, (16, 16), (5472, 10944), "KB = 8 with 7 live taps"),
    RS(7, 2, (), 43, 2, 256, (9, 4), (32436, 29032), "KB = 48"),
    RS(4, 1, (), 49, 1, 256, (7, 3), (28880, 24992), "KB = 56"),
    RS(9, 2, (), 55, 2, 256, (7, 3), (32464, 28064), "KB = 56, 55 live taps"),
    RS(5, 1, (), 61, 1, 256, (6, 3), (30956, 31192), "KB = 64"),
    RS(21, 4, (), 64, 4, 256, (6, 3), (32488, 32720), "K at the cap: no dead register"),
    RS(16, 3, (), 65, 3, 0, (None, None), (0, 0), "first K past the cap: generic"),
    RS(300, 257, (), 15, 257, 320, (16, 13), (19260, 31320), "first workgroup above 256: work items 257 .. 319 idle"),
    RS(511, 512, (), 13, 512, 512, (16, 7), (32764, 28736), "L at the cap; the f32 tile 4 bytes under the aim"),
    RS(512, 513, (), 13, 513, 0, (None, None), (0, 0), "first L past the cap: generic"),
    RS(2047, 512, (), 49, 512, 512, (3, 1), (24772, 16792), "f64: W = 1, the second chain never runs"),
    RS(2600, 509, (), 62, 509, 512, (3, 1), (31432, 21264), "KB = 64 at 512 work items: the largest register file"),
    RS(31, 1, LPW1, 63, 1, 256, (1, 1), (31876, 63752), "f64 tile above the aim, under the budget"),
    RS(8000, 511, LPW1, 32, 511, 512, (1, 1), (32064, 64128), "f64 tile the last one under 64 KiB"),
    RS(15000, 511, LPW1, 60, 511, 512, (1, None), (60136, 0), "f32 above the aim; f64 over the budget: generic"),
    RS(3, 1, KAISER, 37, 1, 256, (10, 5), (30868, 31016), "a Kaiser table on the device"),
    RS(2, 3, KAISER16, 34, 3, 256, (16, 16), (11036, 22072), "width 16, rolloff 0.9476, Kaiser"),
]
RS_IDS = [f"{r.orig}to{r.new}" + ("-" + "-".join(str(v)[:6] for _, v in r.kw[:3]) if r.kw else "") for r in RS_ROWS]
RS_CASES = [pytest.param(r, dt, id=f"{i}-{dt[5:]}") for r, i in zip(RS_ROWS, RS_IDS) for dt in DTYPES]


def choose_route(M, L, K, jspan, elem):
    """resample.hip choose_route / pp_span / run_dev: (KB, G, W, work items, LDS bytes of a whole tile), or None for the generic route."""
    if K > 64 or L > 512:  # kPpMaxTaps, kPpMaxPhases
        return None
    KB, G = (K + 7) // 8 * 8, max(1, 256 // L)
    span = lambda nq: (nq - 1) * M + jspan + KB  # noqa: E731
    W = 16  # kPpMaxWalk
    while W > 1 and span(G * W) * elem > 32 * 1024:  # kPpLdsAim
        W -= 1
    if span(G * W) * elem > 64 * 1024:  # kPpLds
        return None
    return KB, G, W, (L * G + 63) // 64 * 64, span(G * W) * elem


def rs_geo(row, dtype):
    return TR.geometry(row.orig, row.new, dtype, **dict(row.kw))


def rs_instance(row, dtype):
    """(dtype, KB), or (dtype, "generic")."""
    return (dtype, (row.K + 7) // 8 * 8 if row.W[DTYPES.index(dtype)] else "generic")


def test_resampler_constants_are_the_restated_ones():
    text = read_sources()["resample.hip"]
    assert re.search(r"kPpLds = 64 \* 1024, kPpLdsAim = 32 \* 1024;", text)
    assert re.search(r"kPpMaxTaps = 64, kPpMaxPhases = 512, kPpMaxWalk = 16;", text)
    assert "__launch_bounds__(512) void k_resample_pp" in text


@pytest.mark.parametrize("row,dtype", RS_CASES)
def test_resampler_rows_on_host_only_plans(row, dtype):
    i = DTYPES.index(dtype)
    p = TR.host_plan(row.orig, row.new, dtype, **dict(row.kw))
    M, L, K, j0, _, _ = rs_geo(row, dtype)
    assert (M, L) == TR.reduced(row.orig, row.new) and (K, L) == (row.K, row.L)
    got = choose_route(M, L, K, int(j0.max() - j0.min()), ELEM[dtype])
    if row.W[i] is None:
        assert got is None and (p.kernel_name, p.tile) == ("resample_generic", 0)
        return
    KB, G, W, items, lds = got
    assert (p.kernel_name, p.tile) == ("k_resample_pp", G * W * L)
    assert (W, items, lds) == (row.W[i], row.items, row.lds[i]) and lds <= 64 * 1024 and items <= 512
    assert (dtype, KB) in parse_sources(read_sources())["resample"]


def test_resampler_rows_cover_the_launch_shapes():
    """Workgroups of 256, 320 and 512 work items; W = 1 in both types; a tile between the aim and the budget in both types; every
    budget edge on the generic route."""
    tuned = [(r, dt) for r in RS_ROWS for dt in DTYPES if r.W[DTYPES.index(dt)]]
    assert {r.items for r, _ in tuned} == {256, 320, 512}
    for dt in DTYPES:
        i = DTYPES.index(dt)
        assert any(r.W[i] == 1 for r, d in tuned if d == dt) and any(32 * 1024 < r.lds[i] <= 64 * 1024 for r, d in tuned if d == dt)
        assert {r.what.split(":")[0] for r in RS_ROWS if r.W[i] is None} >= {"first K past the cap", "first L past the cap"}
    assert any(r.W == (1, None) for r in RS_ROWS) and any(r.K == 64 for r, _ in tuned)
    assert max(r.lds[1] for r in RS_ROWS) == 64128  # the next tile of this kind, (15000, 511) in f64, is 120 272 bytes: generic


@functools.lru_cache(maxsize=None)
def rs_impulses(row, dtype):
    x, exp = RB.impulse_rows(rs_geo(row, dtype), dtype)
    x.setflags(write=False)
    exp.setflags(write=False)
    return x, exp


@pytest.mark.parametrize("row,dtype", RS_CASES)
def test_resampler_impulse_rows_reach_every_tap(row, dtype):
    """(No GPU.)  RB.impulse_rows asserts that every (p, k) is hit; M impulses per row.  The rows of the large-M cases are M D samples
    long (10^6 for 15000 : 511), so tests/test_resample_readback.py's 16 000-sample limit is not asserted here."""
    x, exp = rs_impulses(row, dtype)
    geo = rs_geo(row, dtype)
    assert np.count_nonzero(x) == 3 * geo[0] and np.count_nonzero(exp) <= 3 * np.count_nonzero(geo[4])


# ---- the census ------------------------------------------------------------------------------------------------------------------------------
CENSUS = {
    "fir": [(taps, dt, (dt, P)) for taps, P in FIR_TAPS.items() for dt in DTYPES] + [(P // 4, dt, (dt, P)) for P in FIR_P for dt in DTYPES],
    "welch": [(n, dt, (dt, n, "coherence")) for n in WELCH_N for dt in DTYPES],
    "minphase": [(shape, dt, n) for shape, n in MINPHASE_N.items() for dt in DTYPES],
    "resample": [(r, dt, rs_instance(r, dt)) for r in RS_ROWS for dt in DTYPES],
}
UNREACHABLE = {}  # family -> {instance: the line of code that keeps every call from it}


def _params(fn, name):
    return [v for mark in fn.pytestmark if mark.name == "parametrize" and mark.args[0] == name for v in mark.args[1]]


def named_instances():
    """family -> the instances CENSUS names plus those the owning files' own lists reach, in the parser's terms."""
    fir = {(dt, FR.reg_split_len(fir_fused_len(t), dt)) for t in TF.FUSED_TAPS for dt in DTYPES}
    fir |= {(dt, FR.reg_split_len(P, dt)) for _, _, (dt, P) in CENSUS["fir"]}
    # tests/test_welch.py: test_fused_parity runs FULL at n = 256 and 1024 and SHORT elsewhere, test_identities the coherence plan at its n
    welch = {(dt, FR.reg_split_len(n, dt), k) for n in TW.FUSED for dt in DTYPES for k, _, _ in (TW.FULL if n in (256, 1024) else TW.SHORT)}
    welch |= {(dt, FR.reg_split_len(n, dt), "coherence") for n in _params(TW.test_identities, "n") for dt in DTYPES}
    welch |= {(dt, FR.reg_split_len(n, dt), k) for _, _, (dt, n, k) in CENSUS["welch"]}
    minphase = {TM.fft_len(t, o) for t, o in TM.FUSED} | {n for _, _, n in CENSUS["minphase"]}
    resample = {(dt, (TR.geometry(*r, dt)[2] + 7) // 8 * 8) for r in TR.RATIOS if r != TR.GENERIC_ONLY for dt in DTYPES}
    resample |= {inst for _, _, inst in CENSUS["resample"] if inst[1] != "generic"}
    return {"fir": fir, "welch": welch, "minphase": minphase, "resample": resample}


def census_gaps(parsed, named, unreachable):
    """family -> (compiled and neither named nor listed unreachable, named or listed and not compiled)."""
    out = {}
    for fam, have in parsed.items():
        claimed = named[fam] | set(unreachable.get(fam, {}))
        out[fam] = (have - claimed, claimed - have)
    return out


NO_GAPS = {fam: (set(), set()) for fam in ("fir", "welch", "minphase", "resample")}


def test_every_compiled_instance_has_a_case():
    named = named_instances()
    for fam, listed in UNREACHABLE.items():
        assert not named[fam] & set(listed) and all(isinstance(reason, str) and reason for reason in listed.values())
    assert census_gaps(parse_sources(read_sources()), named, UNREACHABLE) == NO_GAPS
    # the rows of the issue's table: each is a case of this file
    assert {i for _, _, i in CENSUS["fir"]} == {(dt, P) for dt in DTYPES for P in FIR_P}
    assert {n for _, _, n in CENSUS["minphase"]} == {4, 8, 16, 32, 128, 256, 1024}
    assert {i[1] for _, _, i in CENSUS["resample"]} >= {8, 48, 56, 64, "generic"}


PLANTED = [
    ("fir", "fir.hip", "#define SGX_FIR_SPLITS_F32(X) X(16, 16, 1)", "#define SGX_FIR_SPLITS_F32(X) X(32, 16, 16) X(16, 16, 1)",
     {(F32, (32, 16, 16))}, set()),
    ("fir", "fir.hip", "#define SGX_FIR_SPLITS_F64(X) X(8, 8, 4) X(8, 8, 8)", "#define SGX_FIR_SPLITS_F64(X) X(8, 8, 4)", set(), {(F64, (8, 8, 8))}),
    ("welch", "welch.hip", "#define SGX_WELCH_SPLITS_F64(X) X(8, 8, 4)", "#define SGX_WELCH_SPLITS_F64(X) X(8, 4, 4) X(8, 8, 4)",
     {(F64, (8, 4, 4), k) for k in WELCH_KINDS}, set()),
    ("welch", "welch.hip", "X(16, 16, 8) X(16, 16, 16)\n#define SGX_WELCH_SPLITS_F64", "X(16, 16, 8)\n#define SGX_WELCH_SPLITS_F64", set(),
     {(F32, (16, 16, 16), k) for k in WELCH_KINDS}),
    ("minphase", "minphase.hip", "kMaxFusedN = 4096", "kMaxFusedN = 8192", {8192}, set()),
    ("minphase", "minphase.hip", "kMaxFusedN = 4096", "kMaxFusedN = 2048", set(), {4096}),
    ("resample", "resample.hip", "SGX_RS_CASE(56) SGX_RS_CASE(64)", "SGX_RS_CASE(56) SGX_RS_CASE(64) SGX_RS_CASE(72)", {(F32, 72), (F64, 72)}, set()),
    ("resample", "resample.hip", "SGX_RS_CASE(40) SGX_RS_CASE(48) SGX_RS_CASE(56)", "SGX_RS_CASE(40) SGX_RS_CASE(56)", set(), {(F32, 48), (F64, 48)}),
]


@pytest.mark.parametrize("fam,name,old,new,missing,extra", PLANTED, ids=[f"{p[0]}-{'added' if p[4] else 'removed'}" for p in PLANTED])
def test_the_census_reports_a_planted_instance(fam, name, old, new, missing, extra):
    """One instance added to a copy of the source is reported as compiled without a case, one removed as a case without an instance,
    and nothing else is reported."""
    texts = read_sources()
    assert texts[name].count(old) == 1
    texts[name] = texts[name].replace(old, new)
    want = dict(NO_GAPS)
    want[fam] = (missing, extra)
    assert census_gaps(parse_sources(texts), named_instances(), UNREACHABLE) == want


# ---- 2. GPU: FIR -----------------------------------------------------------------------------------------------------------------------------
def _fir_plan(h, dtype, P):
    plan = sg.FirPlan(h, dtype=dtype)
    assert (plan.kernel_name, plan.fft_size) == ("k_fir_os", P)
    return plan


def _fir_record(name, dtype, P):
    record("k_fir_os", f"{dtype} P={P}", TF.WORST[name])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("taps", list(FIR_TAPS))
def test_gpu_fir_parity(taps, dtype):
    """tests/test_fir.py test_gpu_parity's batch-1 and batch-5 calls at the tap counts no other file runs."""
    P = FIR_TAPS[taps]
    shared = np.stack([TF.make_ir(taps, 0, dtype)])
    per_row = np.stack([TF.make_ir(taps, 10 + r, dtype) for r in range(5)])
    p1, p5 = _fir_plan(shared[0], dtype, P), _fir_plan(per_row, dtype, P)
    S = p1.step
    name = f"census-k_fir_os-{dtype}-{taps}"
    k = 0
    for n in TF._lengths(taps, S, 1):  # batch 1, one response
        for form in ("process", "convolve"):
            p1.reset()
            TF._check_call(p1, shared, TF.make_signal(TF.KINDS[k % 3], n, k, dtype, step_at=n // 2 + 7)[None], form, dtype, name)
            k += 1
    for n in TF._lengths(taps, S, 5):  # batch 5, a response per row, every kind of input in the batch
        x = np.stack([TF.make_signal(TF.KINDS[r % 3], n, 20 + r, dtype) for r in range(5)])
        for form in ("process", "convolve"):
            p5.reset()
            TF._check_call(p5, per_row, x, form, dtype, name)
    _fir_record(name, dtype, P)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", FIR_P)
def test_gpu_fir_tile_seams(P, dtype):
    """A row of 2 tile + 1 segments and one of tile + 1: whole tiles and a last tile of one segment.  The 10^6 : 1 step sits right
    behind the first sample the second tile writes (its later segments are quiet and held to their own bound), and in a second pass
    at the first sample the second tile reads, L samples earlier, so that its first segment, alone in the tile in the shorter row, is
    quiet as a whole beside a loud first tile."""
    taps, tile = P // 4, FIR_TILE[P]
    h = np.stack([TF.make_ir(taps, 5, dtype)])
    plan = _fir_plan(h[0], dtype, P)
    S = plan.step
    name = f"census-k_fir_os-{dtype}-seam{P}"
    for k, nseg in enumerate((2 * tile + 1, tile + 1)):
        n = (nseg - 1) * S + S // 2 + 1
        assert -(-n // S) == nseg
        for step_at in (tile * S + 1, tile * S - (taps - 1)):
            x = TF.make_signal("step", n, 80 + k, dtype, step_at=step_at)[None]
            assert np.abs(x[0, :step_at]).max() > 1e4 * np.abs(x[0, step_at:]).max()
            plan.reset()
            TF._check_call(plan, h, x, "process", dtype, name)
    _fir_record(name, dtype, P)


# ---- GPU: Welch ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("detrend,sname", WELCH_INPUTS)
@pytest.mark.parametrize("n", WELCH_N)
def test_gpu_welch_coherence(n, detrend, sname, dtype):
    hop = n // 4
    plan = sg.WelchPlan(sg.WelchParams(n, hop, sg.WindowType.hanning, WELCH_FS, detrend, "density"), "coherence", dtype)
    assert plan.kernel_name == "k_welch" and plan.tile == welch_host(n, dtype).tile
    worst = 0.0
    for m in welch_counts(plan.tile):
        x, y, ref, bound = welch_case(n, dtype, detrend, sname, m)
        assert plan.n_segments(x.shape[1]) == m
        got = TW._run(plan, x.copy(), y.copy())  # (the shared rows are read-only)
        assert got.shape == ref.shape
        r = TW.ratio(got, ref, bound)
        print(f"welch coherence n={n} {dtype} {detrend} m={m}: ratio {r:.3g}")
        worst = max(worst, r)
        assert r <= 1.0, (n, dtype, detrend, sname, m, r)
    record("k_welch coherence", f"{dtype} n={n}", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", WELCH_N)
def test_gpu_welch_identities(n, dtype):
    """tests/test_welch.py test_identities' assertions at these lengths: coherence(x, x) within 8 u of 1, csd(x, x) = welch(x) bit for bit."""
    hop = n // 4
    wp = sg.WelchParams(n, hop, sg.WindowType.hanning, 8000.0)
    psd, cs, co = (sg.WelchPlan(wp, k, dtype) for k in WELCH_KINDS)
    assert {p.kernel_name for p in (psd, cs, co)} == {"k_welch"}
    m = 2 * psd.tile + 1
    x, _ = TW.signals("noise", 3, n + (m - 1) * hop + 37, dtype, seed=11)
    pxx, cxx, sxx = TW._run(psd, x), TW._run(co, x, x), TW._run(cs, x, x)
    assert np.all(pxx > 0)
    assert np.max(np.abs(cxx - 1.0)) <= 8 * TW.U[dtype]
    assert np.all(sxx.imag == 0) and np.array_equal(sxx.real, pxx)


# ---- GPU: minimum phase ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("taps,oversample", TM.SHORT_FUSED, ids=[f"{t}-{o}" for t, o in TM.SHORT_FUSED])
def test_gpu_minphase_short_lengths(taps, oversample, dtype):
    n = MINPHASE_N[(taps, oversample)]
    worst = 0.0
    for out_len in minphase_out_lens(n):
        plan = sg.MinPhasePlan(taps, out_len, oversample, dtype=dtype, route="auto")
        assert (plan.kernel_name, plan.fft_size, plan.output_length) == ("k_minphase", n, min(out_len, n))
        for kind in TM.KINDS:
            rows, refs = TM.case(kind, taps, oversample, dtype, out_len=out_len)
            got = plan.execute(rows.astype(TM.NP[dtype]))
            assert got.shape == (3, min(out_len, n))
            worst = max(worst, TM.check_rows(got, refs, dtype, f"census-k_minphase-{dtype}-{kind}"))
    record("k_minphase", f"{dtype} n={n}", worst)


# ---- GPU: resampler ----------------------------------------------------------------------------------------------------------------------------
def _rs_plan(row, dtype):
    plan = sg.ResamplePlan(row.orig, row.new, dtype=dtype, **dict(row.kw))
    tuned = row.W[DTYPES.index(dtype)] is not None
    assert plan.kernel_name == ("k_resample_pp" if tuned else "resample_generic") and (plan.tile > 0) == tuned
    return plan


def _rs_label(row, dtype):
    inst = rs_instance(row, dtype)[1]
    return f"{dtype} " + (f"KB={inst} items={row.items} W={row.W[DTYPES.index(dtype)]}" if inst != "generic" else "generic")


def rs_noise_len(geo):
    """Three tiles of input (a tile is Q q-blocks of M samples, Q L outputs) and a ragged tail."""
    M, L, K, _, _, tile = geo
    return 3 * (tile // L if tile % L == 0 else -(-tile // L)) * M + K + 5


@pytest.mark.gpu
@pytest.mark.parametrize("row,dtype", RS_CASES)
def test_gpu_resampler_impulse_read_back(row, dtype):
    x, exp = rs_impulses(row, dtype)
    y = _rs_plan(row, dtype).resample(x)
    assert y.shape == exp.shape
    bad = np.argwhere(y != exp)
    assert bad.size == 0, (len(bad), bad[:5], y[tuple(bad[0])], exp[tuple(bad[0])])


@pytest.mark.gpu
@pytest.mark.parametrize("row,dtype", RS_CASES)
def test_gpu_resampler_bound_and_chain(row, dtype):
    """Noise over three tiles: every output within tests/test_resample.py's bound of its own window; in f32 also
    tests/test_resample_readback.py's chain condition."""
    geo = rs_geo(row, dtype)
    x = TR.noise(rs_noise_len(geo), dtype, 61)
    y = _rs_plan(row, dtype).resample(x)
    worst = TR.check_bound(y, x, geo, dtype)
    record("k_resample_pp" if row.W[DTYPES.index(dtype)] else "resample_generic", _rs_label(row, dtype), worst)
    if dtype != F32:
        return
    off = total = 0
    spac = 0.0
    for r in range(3):
        ref, big = RB.chain_f32(x[r], geo)
        d = np.abs(y[r].astype(np.float64) - ref.astype(np.float64))
        off += int(np.count_nonzero(d))
        total += d.size
        spac = max(spac, float(np.max(d / np.spacing(np.maximum(big, np.float32(1e-30))).astype(np.float64))))
    print(f"resample chain {row.orig}:{row.new} {row.kw}: {off} of {total} outputs off the chain, worst {spac:.3g} spacings")
    assert off <= 1e-4 * total and spac <= 4.0, (off, total, spac)


def rs_cuts(geo, n):
    """1 sample, K - 2, K - 1 and K samples, a chunk that ends in the middle of the second tile (so it crosses a tile seam of the one
    call and holds one of its own), the rest."""
    M, L, K, _, _, tile = geo
    cut = [c for c in (1, K - 2, K - 1, K) if c > 0]
    cut.append(3 * (-(-tile // L)) * M // 2 - sum(cut))
    assert all(c > 0 for c in cut) and sum(cut) < n
    return cut + [n - sum(cut)]


@pytest.mark.gpu
@pytest.mark.parametrize("row,dtype", RS_CASES)
def test_gpu_resampler_streaming_is_bit_equal_to_one_call(row, dtype):
    geo = rs_geo(row, dtype)
    n = rs_noise_len(geo)
    x = TR.noise(n, dtype, 62)
    plan = _rs_plan(row, dtype)
    whole = plan.resample(x)
    parts, at = [], 0
    for c in rs_cuts(geo, n):
        want = plan.step(plan.consumed, c)[0]
        y = plan.process(x[:, at:at + c])
        at += c
        assert y.shape == (3, want) and plan.consumed == at
        parts.append(y)
    tail = plan.flush()
    assert tail.shape == (3, plan.out_len(n) - sum(p.shape[1] for p in parts))
    assert np.array_equal(np.concatenate(parts + [tail], axis=1), whole)


# ---- 3. the table ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_worst_ratios_per_family():
    """Prints what the cases above recorded (run the module as a whole): worst ratio to the bound per family and instance."""
    print()
    for (family, instance), r in sorted(WORST.items()):
        print(f"| {family} | {instance} | {r:.3g} |")
    assert all(r <= 1.0 for r in WORST.values())
