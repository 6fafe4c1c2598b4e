"""Tile walks of the persistent 1-D kernels: every frame of every row, at batches where a workgroup takes several tiles.

Eleven kernels keep a workgroup per CU (or two) and walk it over a run of tiles, carrying state from tile to tile: the next tile's samples
prefetched into the idle exchange buffer, output stores counted behind the next tile's loads, the fused MFCC of tile t computed at the
top of tile t + 1, the inverse kernels' overlap carried in LDS, two 256-thread halves under one loop control, walks that run on from one
signal into the next.  The sharp tests of the suite (test_frame_locality.py, test_bank_readback.py, test_istft_precision.py) run batches
of 5 rows: no workgroup ever takes a second tile.  The many-tile tests compare against 2e-4 max|ref| of the whole batch.  This file
joins the two.

1. Walk models (CPU).  `walk_halves` (k_r32x16: launch_variant / launch_binaural, the loop control `lead`, the idle half), `walk_slots`
   (k_r32x32, k_r64x32, k_d32x16, k_d512, k_d32x32: one tile per workgroup and round), `carry_runs` + `walk_slots` over runs (the inverse kernels:
   istft_carry_runs of sgx_internal.h restated) say which tiles each walker takes as a function of (tiles, batch, CU count); `regimes`
   names what a walk exercises.  k_reg_radix's resident count depends on registers and LDS: only an upper bound of its grid is modelled,
   4 workgroups per CU (rr_stft_waves never returns more, reg_radix.h) of tiles of at most 32 frames (reg_radix_ft_max), and its batches
   hold three times that many tiles.  Batches are chosen by `choose_batch` from the CU count: the smallest that reaches every regime a
   case lists.
2. GPU: FORWARD / INVERSE tables, kernel and bank stage names asserted after the full-size call.  Per case and batch
     (1) walk independence: row i of the full batch equals bit for bit row i computed in sub-batches in the `one tile` regime (PACK: its
         own B = 1 launch; a long row: its own B = 1 launch — for the inverse a different cut into runs, so a carry rebuilt by a warm-up
         tile must give the bits of the carry that was walked).  EXEMPT lists routes whose two launches legitimately run different
         arithmetic; it is empty.
     (2) the per-frame bound of test_frame_locality.py section 3 / test_bank_readback.py (banks) / the exact fma chain of
         test_mfcc.py (fused MFCC) / d_t of test_istft_precision.py (inverse) / the parity bound of test_binaural.py, on every frame
         (sample) of every row.  No constant is introduced here: every bound and every c is imported.
   Every four rows hold the decades of `level_batch` (f32 1, 1e-4, 1e3, 1e-6; f64 1, 1e-7, 1e5, 1e-10) in an order that moves on with every
   base-4 digit of the row index (walks step by powers of two: a plain cycle of four would give a walker rows of one level only), every
   eighth row switches level inside itself; that a loud tile is followed by a quiet one in some walk is asserted on the model.  The long shape (rows of two walk strides +
   2 tiles, the length a function of the CU count) keeps a walk inside one signal.
3. The checker can fail (CPU): a frame taken from the tile walked before, one f32 rounding of a loud tile's largest bin leaked into the
   quiet tile walked next, a 64-byte run left stale — each fails (1) and (2); the leak passes the 2e-4 max|ref| criterion.

The inverse kernels' carry is zero by itself when a signal ends (its last tile holds the tail), so resetting it between runs matters only
where a run that ends INSIDE a signal is followed by another one: the long inverse batches are searched for exactly that regime.  A build
with that reset removed from k_istft2048 passed every short-signal case and failed assertion 1 on the long hop 512 case (511 samples of the
first tile of a second run); nothing else in this file would have seen it.

Measured on MI355X (256 CUs, 83 GPU cases, 29 s; test_tuned_kernels_many_tiles_per_workgroup in the same visit: 15 s).  Assertion 1 held bit
for bit on every case, EXEMPT stayed empty.  Worst ratio to the bound per kernel, per-bin linear outputs / dB / bank outputs (information,
not thresholds):
    k_r32x16 n_fft 1024    0.011 / 0.068 / 0.010     fused MFCC: every coefficient bit-equal to the fma chain; binaural ILR 0.0034
    k_r32x16 n_fft 512     0.013 / 0.058 / 0.0080    (joint norm)
    k_r32x32               0.0070 / - / 0.0038       k_r64x32     0.0045 / 0.031 / 0.0029
    k_d32x16               0.017 / 0.083 / 0.045     k_d512       0.019 / - / 0.0024 (joint)     k_d32x32   0.010 / - / 0.10 (bank_rows, Mel 300)
    k_reg_radix f32        0.016 / 0.064 / 0.011     k_reg_radix f64   0.026
    inverse, ratio to d_t: istft1024c 0.016, istft2048 0.011, istft_d1024 0.026, istft_d512 0.028 (the same at 41-frame and at 10 s signals)
The figures equal those of the 5-row tests of test_frame_locality.py / test_istft_precision.py to within their scatter: no walk regime costs
precision, and no tile of any walk came back stale, doubled or shifted.
"""
import functools

import numpy as np
import pytest
import torch

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from spectrograms_amd.binaural import BinauralPlan
from tests import helpers as H
from tests import test_bank_readback as BR
from tests import test_binaural as TB
from tests import test_istft_precision as IP
from tests.test_frame_locality import CB, frame_deltas, frames_in, make_plan, n_samples, paired, ratios

HOST = _ffi.DEVICE_HOST_ONLY
SR = 16000.0
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
NP = {"float32": np.float32, "float64": np.float64}
F32, F64 = "float32", "float64"
LEVELS = {F32: [1.0, 1e-4, 1e3, 1e-6], F64: [1.0, 1e-7, 1e5, 1e-10]}  # level_batch's decades
WORST = {}
# routes whose full-size and one-tile launches legitimately run different arithmetic for the same frame: (kernel, kind) -> source lines
EXEMPT = {}

ONE, STEADY, UNEQUAL, CROSS, INSIDE, RAGGED, SHORT_XCD = ("one tile", "3+ tiles", "unequal walks", "walk crosses a signal",
                                                          "walk inside a signal", "ragged last tile", "short last XCD")
LOUD_QUIET = "loud tile before a quiet one"
IDLE = "idle half repeats the first half's tile"  # k_r32x16: `if (next >= hi) next -= half`
WARMUP, SEVERAL = "run starts inside a signal", "several runs per workgroup"
RESET = "a run that ends inside a signal is followed by another"  # the only place where the carry in LDS is not zero when a run starts


# ---- 1. walk models ----------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def walk_halves(total, cus, hs=2):
    """k_r32x16.  -> (walkers, per_xcd, nslots); a walker is (xcd, slot, half, [(tile, own)]): `own` is False where a half repeats the
    first half's tile (an odd run's last round) and for the second half of a binaural workgroup (hs = 1: one tile for both halves)."""
    per_xcd = cdiv(total, 8)
    cu_slots = max(1, cus // 8)
    nslots = min(cdiv(per_xcd, 2), cu_slots) if hs == 2 else min(per_xcd, cu_slots)
    walkers = []
    for x in range(8):
        lo = x * per_xcd
        hi = min(lo + per_xcd, total)
        for s in range(nslots):
            for h in range(2):
                hh = h if hs == 2 else 0
                lead = lo + s * hs
                wid = lead + hh
                if wid >= hi:
                    wid = lead
                seq = []
                while lead < hi:
                    seq.append((wid, wid == lead + hh and (hs == 2 or h == 0)))
                    nxt = lead + nslots * hs + hh
                    if nxt >= hi:
                        nxt -= hh
                    wid = nxt
                    lead += nslots * hs
                walkers.append((x, s, h, seq))
    return walkers, per_xcd, nslots


def walk_slots(total, cus, per_cu=1):
    """One item per workgroup and round (`while (wid < hi)`): the five other tuned forward kernels (per_cu 1) and the runs of the inverse
    kernels (wgs = per_cu x CUs)."""
    per_xcd = cdiv(total, 8)
    nslots = max(1, min(per_xcd, per_cu * cus // 8))
    walkers = []
    for x in range(8):
        lo = x * per_xcd
        hi = min(lo + per_xcd, total)
        for s in range(nslots):
            walkers.append((x, s, 0, [(w, True) for w in range(lo + s, hi, nslots)]))
    return walkers, per_xcd, nslots


def carry_runs(tiles, batch, wgs, ov):
    """istft_carry_runs (sgx_internal.h) -> (R, run_len)."""
    best, R = None, 1
    for r in range(1, tiles + 1):
        ln = cdiv(tiles, r)
        if cdiv(tiles, ln) != r:
            continue
        rounds = cdiv(r * batch, wgs)
        cost = rounds * (ln + (1 if (r > 1 and ov) else 0))
        if best is None or cost < best:
            best, R = cost, r
        if rounds > 1 and ln <= 2:
            break
    return R, cdiv(tiles, R)


def reg_radix_grid_bound(cus):
    """launch_reg_radix_t: grid <= cus x min(by_regs, by_lds), by_regs = rr_stft_waves() <= 4 (reg_radix.h)."""
    return 4 * cus


REG_RADIX_FT_MAX = 32  # reg_radix_ft_max: `while (ft < 32 && ...) ft *= 2`


def regimes(walkers, per_xcd, total, sig_of, ragged, level_of=None):
    own = [(x, [t for t, o in seq if o]) for x, s, h, seq in walkers if any(o for _, o in seq) or h == 0]
    lens = [len(t) for _, t in own]
    out = set()
    if max(lens) == 1:
        out.add(ONE)
    if max(lens) >= 3:
        out.add(STEADY)
    for x in range(8):
        if len({len(t) for xx, t in own if xx == x}) > 1:
            out.add(UNEQUAL)
    for _, t in own:
        for a, b in zip(t, t[1:]):
            out.add(CROSS if sig_of(a) != sig_of(b) else INSIDE)
            if level_of is not None and level_of(a) >= 1e3 * level_of(b):
                out.add(LOUD_QUIET)
    if ragged:
        out.add(RAGGED)
    if 8 * per_xcd > total:
        out.add(SHORT_XCD)
    return out


def locate(walkers, tile, what="tile"):
    """'xcd x slot s half h, tile k of n in its walk, previous tile p' for an assertion message."""
    for x, s, h, seq in walkers:
        for k, (t, o) in enumerate(seq):
            if t == tile and o:
                prev = seq[k - 1][0] if k else None
                return f"{what} {tile}: xcd {x} slot {s} half {h}, {what} {k} of {len(seq)} in its walk, previous {what} {prev}"
    return f"{what} {tile}: in no walk"


def row_level(dtype, r):
    """Level of row r; every eighth row switches between 1 and 1e-4 inside itself (level 1 here).  Every four rows hold the four decades,
    in an order that moves on with every base-4 digit of r: walks step by powers of two (16 tiles = 8 rows of 2 tiles), and a plain r mod 4
    would hand every walker rows of one level only."""
    if r % 8 == 0:
        return 1.0
    q, i = r, 0
    while q:
        i += q % 4
        q //= 4
    return LEVELS[dtype][i % 4]


# forward families: kernel name -> (n_fft -> frames per tile)
FT = {"r32x16_f32": {1024: 16, 512: 32}, "r32x32_f32": {2048: 16}, "r64x32_f32": {4096: 8}, "d32x16_f64": {1024: 16}, "d512_f64": {512: 32},
      "d32x32_f64": {2048: 8}}


def packs(n_fft, hop, nf, batch, mel, sched, mfcc):
    """want_pack (kernels_r32x16.hip) for the shapes of this file (its 32-bit guards are far away)."""
    p512 = n_fft == 512
    unlisted = p512 and hop not in (64, 128, 160, 256)
    if mfcc or (n_fft != 1024 and not p512) or (batch < 2 and not unlisted) or (mel and (not sched or p512)) or hop & 1:
        return False
    ft = 32 if p512 else 16
    slots = cdiv(nf, ft) * ft
    used = 2 * ((nf + 1) // 2) if p512 else nf
    return unlisted or (slots - used) * 4 >= slots


class Geometry:
    """Tiles of one forward launch: which walk model, tiles, and frame -> tile."""

    def __init__(self, case, nf, batch, cus):
        dtype, n_fft, hop, kind, kernel, stage = case[:6]
        self.kernel, self.nf, self.batch, self.cus, self.dtype = kernel, nf, batch, cus, dtype
        self.binaural = kernel == TB.FUSED
        fam = "r32x16_f32" if self.binaural else kernel
        self.reg = kernel == "reg_radix"
        mel = stage is not None
        mfcc = isinstance(kind, tuple) and kind[0] == "mfcc"
        self.pack = fam == "r32x16_f32" and not self.binaural and packs(n_fft, hop, nf, batch, mel, mel and stage.startswith("r32x16_sched"), mfcc)
        self.p512 = fam == "r32x16_f32" and n_fft == 512
        if self.reg:
            self.ft = REG_RADIX_FT_MAX
        else:
            self.ft = FT[fam][n_fft]
        self.tps = cdiv(nf, self.ft)
        if self.pack:
            self.units = (nf + 1) // 2 if self.p512 else nf  # slots (frame pairs) or frames per signal
            self.total = cdiv(batch * self.units, 16)
            self.ragged = self.total * 16 > batch * self.units
        else:
            self.total = self.tps * batch
            self.ragged = nf % self.ft != 0
        if self.reg:
            self.walkers = None
        elif fam == "r32x16_f32":
            self.walkers, self.per_xcd, self.nslots = walk_halves(self.total, cus, 1 if self.binaural else 2)
        else:
            self.walkers, self.per_xcd, self.nslots = walk_slots(self.total, cus)

    def sig_of(self, tile):
        return tile * 16 // self.units if self.pack else tile // self.tps

    def tile_of(self, row, frame):
        if self.pack:
            return (row * self.units + (frame // 2 if self.p512 else frame)) // 16
        return row * self.tps + frame // self.ft

    def regimes(self):
        if self.reg:  # only what the grid bound proves
            r = {STEADY} if self.total >= 3 * reg_radix_grid_bound(self.cus) else set()
            if self.batch * self.nf <= self.cus:  # (at most a tile per frame: total <= CUs <= grid)
                r.add(ONE)
            return r
        r = regimes(self.walkers, self.per_xcd, self.total, self.sig_of, self.ragged, lambda t: row_level(self.dtype, self.sig_of(t)))
        if not self.binaural and any(not o for _, _, _, seq in self.walkers for _, o in seq[1:]):
            r.add(IDLE)
        return r

    def where(self, row, frame):
        t = self.tile_of(row, frame)
        if self.reg:
            return f"row {row} frame {frame} (tile >= {t} of a grid-stride walk)"
        return f"row {row} frame {frame}, {locate(self.walkers, t)}"


SHORT_SET = frozenset({STEADY, UNEQUAL, CROSS, RAGGED, SHORT_XCD, LOUD_QUIET})
LONG_SET = frozenset({STEADY, INSIDE})


def required(case, shape):
    if case[4] == "reg_radix":
        return frozenset({STEADY})
    if shape == "long":
        return LONG_SET
    return SHORT_SET | {IDLE} if case[4] == "r32x16_f32" else SHORT_SET


def frames_of(case, shape, cus):
    """Frames per row: 41 (fewer at the longest hops, as test_frame_locality.py), 5 for the PACK cases, and for the long shape two walk
    strides + 2 tiles so that a walker's consecutive tiles lie in one signal."""
    dtype, n_fft, hop, kind, kernel = case[:5]
    if shape in ("5", "57"):
        return int(shape)
    if shape == "41":
        return frames_in(n_fft, hop, "x")
    fam = "r32x16_f32" if kernel == TB.FUSED else kernel
    stride = max(1, cus // 8) * (2 if fam == "r32x16_f32" and kernel != TB.FUSED else 1)
    return (2 * stride + 2) * FT[fam][n_fft] - 3


def choose_batch(case, shape, cus):
    """The smallest batch whose walk reaches every required regime (searched upwards from two rounds' worth of tiles)."""
    nf = frames_of(case, shape, cus)
    need = required(case, shape)
    if case[4] == "reg_radix":
        return cdiv(3 * reg_radix_grid_bound(cus), cdiv(nf, REG_RADIX_FT_MAX)), nf
    if shape == "long":
        for b in range(2, 64):
            if need <= Geometry(case, nf, b, cus).regimes():
                return b, nf
        raise AssertionError(("no batch", case, shape, cus))
    probe = Geometry(case, nf, 2, cus)
    hs = 1 if probe.binaural else 2 if probe.kernel == "r32x16_f32" else 1
    two_rounds = 2 * 8 * max(1, cus // 8) * hs  # tiles
    per_row = probe.units / 16.0 if Geometry(case, nf, 64, cus).pack else probe.tps
    b0 = max(2, int(two_rounds / per_row))
    for b in range(b0, b0 + 4096):
        if need <= Geometry(case, nf, b, cus).regimes():
            return b, nf
    raise AssertionError(("no batch", case, shape, cus))


def one_tile_rows(case, nf, cus):
    """Rows per comparison launch: the largest sub-batch in the `one tile` regime."""
    if case[4] == "reg_radix":
        return max(1, cus // nf)  # total <= CUs <= grid whatever the tile size
    g2 = Geometry(case, nf, 2, cus)
    hs = 1 if g2.binaural else 2 if g2.kernel == "r32x16_f32" else 1
    s = max(1, 8 * max(1, cus // 8) * hs // g2.tps)
    while s > 1 and ONE not in Geometry(case, nf, s, cus).regimes():
        s -= 1
    return s


# inverse: (dtype, n_fft, hop, centre, window, name, paired, workgroups per CU, blocks per tile)
INVERSE = [
    (F32, 1024, 256, True, "hanning", "istft1024c", False, 2, 16),
    (F32, 1024, 1024, False, "hanning", "istft1024c", False, 2, 16),
    (F32, 2048, 512, True, "hanning", "istft2048", False, 1, 16),
    (F32, 2048, 2048, False, "hanning", "istft2048", False, 1, 16),
    (F64, 1024, 256, True, "hanning", "istft_d1024", False, 1, 16),
    (F64, 1024, 1024, False, "hanning", "istft_d1024", False, 1, 16),
    (F64, 512, 160, False, "blackman", "istft_d512", True, 1, 32),
    (F64, 512, 512, False, "hanning", "istft_d512", True, 1, 32),
]


def inv_tiles(n_fft, hop, nf, blk):
    full = (nf - 1) * hop + n_fft
    return cdiv(cdiv(full, hop), blk)


class InvGeometry:
    def __init__(self, case, nf, batch, cus):
        dtype, n_fft, hop, _, _, _, _, per_cu, blk = case
        self.nf, self.batch, self.dtype = nf, batch, dtype
        self.ov = (n_fft - 1) // hop
        self.tiles = inv_tiles(n_fft, hop, nf, blk)
        self.wgs = per_cu * cus
        self.R, self.run_len = carry_runs(self.tiles, batch, self.wgs, self.ov)
        self.total = self.R * batch
        self.walkers, self.per_xcd, self.nslots = walk_slots(self.total, cus, per_cu)
        self.ragged = cdiv((nf - 1) * hop + n_fft, hop) % blk != 0
        self.hop, self.blk = hop, blk

    def regimes(self):
        r = regimes(self.walkers, self.per_xcd, self.total, lambda rid: rid // self.R, self.ragged,
                    lambda rid: row_level(self.dtype, rid // self.R))
        lens = [len(seq) for _, _, _, seq in self.walkers]
        out = {x for x in r if x in (UNEQUAL, RAGGED, SHORT_XCD, LOUD_QUIET)}
        if max(lens) == 1:
            out.add(ONE)
        if max(lens) >= 3:  # a middle run: the carry is reset before it and after it
            out.add(SEVERAL)
        if max(lens) * self.run_len >= 3:
            out.add(STEADY)
        if CROSS in r:
            out.add(CROSS)
        if self.R > 1 and self.ov:
            out.add(WARMUP)
            if any(a % self.R != self.R - 1 for _, _, _, seq in self.walkers for (a, _), _ in zip(seq, seq[1:])):
                out.add(RESET)
        return out

    def where(self, row, sample):
        t = min(self.tiles - 1, sample // (self.hop * self.blk))
        rid = row * self.R + t // self.run_len
        at = locate(self.walkers, rid, "run")
        return f"row {row} sample {sample}, tile {t} of its signal, {at} (R {self.R}, run_len {self.run_len})"


INV_SHORT = frozenset({SEVERAL, STEADY, UNEQUAL, CROSS, RAGGED, SHORT_XCD, LOUD_QUIET})


def inv_frames(case, shape):
    hop = case[2]
    return 41 if shape == "41" else int(10 * SR) // hop + 1  # 10 s rows


def inv_choose_batch(case, shape, cus):
    nf = inv_frames(case, shape)
    if shape == "41":
        g = InvGeometry(case, nf, 1, cus)
        for b in range(g.wgs + 1, g.wgs + 4096):
            if INV_SHORT <= InvGeometry(case, nf, b, cus).regimes():
                return b, nf
        raise AssertionError(("no batch", case, cus))
    # long rows: R > 1, a cut that differs from the row's own B = 1 launch, and (frames that overlap) workgroups that go on to a second
    # run after one that ended inside a signal
    one = InvGeometry(case, nf, 1, cus)
    for b in range(2, 4096):
        g = InvGeometry(case, nf, b, cus)
        if g.R > 1 and g.run_len != one.run_len and g.run_len >= 2 and (not g.ov or RESET in g.regimes()):
            return b, nf
    raise AssertionError(("no batch", case, cus))


# ---- 2. the tables ------------------------------------------------------------------------------------------------------------------
MEL80, MEL40, MEL200, ERB64, CHROMA = BR.mel(80), BR.mel(40), BR.mel(200), BR.erb(64), ("chroma", "l2")
# (dtype, n_fft, hop, kind, kernel name, bank stage name or None, shapes)
#   kind: "complex" / "power" / "magnitude" / "db_low" (make_plan of test_frame_locality.py), (bank, output) (make_plan of
#   test_bank_readback.py, whose case table says which bank shape reaches which stage), ("mfcc", n_mels, n_mfcc, keep C0), "ilr" (binaural)
FORWARD = [
    # k_r32x16, n_fft 1024
    (F32, 1024, 256, "complex", "r32x16_f32", None, ("41", "long", "5")),  # staged samples, XSPAD
    (F32, 1024, 256, "power", "r32x16_f32", None, ("41", "5")),            # per-bin WIDE stores; 5 frames: PACK tiles of the batch
    (F32, 1024, 256, "magnitude", "r32x16_f32", None, ("41",)),
    (F32, 1024, 256, "db_low", "r32x16_f32", None, ("41",)),
    (F32, 1024, 160, "power", "r32x16_f32", None, ("41",)),                # another staged hop
    (F32, 1024, 400, "complex", "r32x16_f32", None, ("41", "long")),       # per-lane loads (hop > 272)
    (F32, 1024, 400, "db_low", "r32x16_f32", None, ("41",)),
    (F32, 1024, 255, "power", "r32x16_f32", None, ("41",)),                # odd hop
    (F32, 1024, 256, (MEL80, "power"), "r32x16_f32", "r32x16_sched", ("41", "long")),
    (F32, 1024, 256, (MEL80, "db"), "r32x16_f32", "r32x16_sched", ("41",)),
    (F32, 1024, 256, (MEL80, "power"), "r32x16_f32", "r32x16_sched_packed", ("5",)),
    (F32, 1024, 256, (ERB64, "power"), "r32x16_f32", "r32x16_mfma", ("41",)),
    (F32, 1024, 256, (MEL200, "power"), "r32x16_f32", "r32x16_csr", ("41",)),
    (F32, 1024, 255, (BR.loghz(96), "magnitude"), "r32x16_f32", "r32x16_sched", ("41",)),   # odd hop: one-signal tiles
    (F32, 1024, 256, (CHROMA, "chroma"), "r32x16_f32", "r32x16_mfma", ("41",)),
    (F32, 1024, 256, ("mfcc", 40, 13, True), "r32x16_f32", "r32x16_sched_mfcc", ("41", "long")),  # MSTEPS 12
    (F32, 1024, 400, ("mfcc", 80, 20, False), "r32x16_f32", "r32x16_sched_mfcc", ("41",)),  # MSTEPS 20, C0 dropped, per-lane loads
    (F32, 1024, 256, "ilr", TB.FUSED, None, ("41",)),                      # binaural: one tile for both halves (HS = 1)
    # k_r32x16, n_fft 512: two frames per transform
    (F32, 512, 128, "complex", "r32x16_f32", None, ("57", "41", "long")),  # 57 frames: the staged form; 41: 22 of 64 slots empty, PACK
    (F32, 512, 160, "power", "r32x16_f32", None, ("57",)),
    (F32, 512, 256, "magnitude", "r32x16_f32", None, ("57",)),
    (F32, 512, 64, "db_low", "r32x16_f32", None, ("57",)),
    (F32, 512, 128, (MEL80, "power"), "r32x16_f32", "r32x16_sched512", ("41",)),
    (F32, 512, 150, "power", "r32x16_f32", None, ("41", "5")),                # no staged variant: the packed form's per-lane loads
    # k_r32x32
    (F32, 2048, 512, "complex", "r32x32_f32", None, ("41", "long")),
    (F32, 2048, 512, "power", "r32x32_f32", None, ("41",)),
    (F32, 2048, 511, "magnitude", "r32x32_f32", None, ("41",)),
    (F32, 2048, 512, (MEL80, "power"), "r32x32_f32", "r32x32_sched", ("41",)),
    # k_r64x32
    (F32, 4096, 1024, "complex", "r64x32_f32", None, ("41", "long")),
    (F32, 4096, 1024, "power", "r64x32_f32", None, ("41",)),
    (F32, 4096, 1023, "db_low", "r64x32_f32", None, ("41",)),
    (F32, 4096, 1024, (MEL80, "power"), "r64x32_f32", "r64x32_sched", ("41",)),
    (F32, 4096, 2048, (MEL80, "power"), "r64x32_f32", "bank_rows", ("41",)),  # per-bin power, then k_bank_rows
    # k_d32x16
    (F64, 1024, 256, "complex", "d32x16_f64", None, ("41", "long")),
    (F64, 1024, 400, "complex", "d32x16_f64", None, ("41",)),              # the unstaged form DESIGN.md 3.5's bug lived in
    (F64, 1024, 256, "db_low", "d32x16_f64", None, ("41",)),
    (F64, 1024, 255, "power", "d32x16_f64", None, ("41",)),
    (F64, 1024, 256, (BR.mel(128), "power"), "d32x16_f64", "d32x16_sched", ("41",)),
    # k_d512
    (F64, 512, 128, "complex", "d512_f64", None, ("41", "long")),
    (F64, 512, 160, "power", "d512_f64", None, ("41",)),
    (F64, 512, 129, "magnitude", "d512_f64", None, ("41",)),
    (F64, 512, 128, (BR.mel(8), "power"), "d512_f64", "d512_sched", ("41",)),
    # k_d32x32
    (F64, 2048, 512, "complex", "d32x32_f64", None, ("41", "long")),
    (F64, 2048, 511, "power", "d32x32_f64", None, ("41",)),
    (F64, 2048, 512, (BR.erb(129), "power"), "d32x32_f64", "d32x32_sched", ("41",)),
    (F64, 2048, 512, (BR.mel(300), "power"), "d32x32_f64", "bank_rows", ("41",)),
    # k_reg_radix
    (F32, 400, 160, "complex", "reg_radix", None, ("41",)),                # staged
    (F32, 400, 250, "power", "reg_radix", None, ("41",)),                  # 2 hop > n_fft: unstaged
    (F64, 400, 160, "power", "reg_radix", None, ("41",)),
    (F64, 400, 160, "complex", "reg_radix", None, ("41",)),
    (F32, 400, 160, (MEL40, "power"), "reg_radix", "reg_radix_bands", ("41",)),
    (F32, 400, 160, (ERB64, "db"), "reg_radix", "reg_radix_csr", ("41",)),
]
FWD_RUNS = [(c, s) for c in FORWARD for s in c[6]]
INV_RUNS = [(c, s) for c in INVERSE for s in ("41", "long")]
CU_COUNTS = [64, 256, 304]


def kind_tag(kind):
    if isinstance(kind, str):
        return kind
    if kind[0] == "mfcc":
        return f"mfcc{kind[1]}x{kind[2]}{'' if kind[3] else 'nc0'}"
    return f"{kind[0][0]}{kind[0][1]}-{kind[1]}"


def fwd_id(run):
    c, s = run
    return f"{c[4]}-{c[0][5:]}-{c[1]}-{c[2]}-{kind_tag(c[3])}-{c[5] or 'bins'}-{s}"


def inv_id(run):
    c, s = run
    return f"{c[5]}-{c[1]}-{c[2]}-{s}"


def build_plan(case, device=_ffi.DEVICE_CURRENT):
    dtype, n_fft, hop, kind = case[:4]
    if kind == "ilr":
        return BinauralPlan(TB.bparams("ilr", n_fft, hop), dtype, device)
    if isinstance(kind, str):
        return make_plan(dtype, n_fft, hop, kind, device=device)
    if kind[0] == "mfcc":
        mp = sg.MfccParams(kind[2])
        params = sg.SpectrogramParams(sg.StftParams(n_fft, hop, sg.WindowType.hanning, True), SR)
        return sg.Plan(params, _ffi.AMP_DECIBELS, sg.MelParams(kind[1], 0.0, 8000.0), sg.LogParams(BR.MFCC_FLOOR), dtype, device=device,
                       mfcc=mp if kind[3] else mp.with_c0(False))
    return BR.make_plan(dtype, n_fft, hop, kind[0], kind[1], device=device)


# ---- CPU: the models ----------------------------------------------------------------------------------------------------------------
def test_walk_models_reproduce_hand_checked_walks():
    # f32 1024, 512 signals of 3 tiles on 256 CUs: per_xcd 192, 32 slots of two halves, three rounds
    w, per_xcd, nslots = walk_halves(1536, 256)
    assert (per_xcd, nslots, len(w)) == (192, 32, 512)
    assert [t for t, _ in w[0][3]] == [0, 64, 128] and [t for t, _ in w[1][3]] == [1, 65, 129]
    x3 = [q for q in w if q[0] == 3 and q[1] == 31]
    assert [t for t, _ in x3[1][3]] == [3 * 192 + 63, 3 * 192 + 127, 3 * 192 + 191] and all(o for q in w for _, o in q[3])
    # 1025 tiles: per_xcd 129, 32 slots; slot 0 walks a third round in which its second half has a tile (128) but half pairs end there;
    # the last XCD holds 1025 - 903 = 122 tiles
    w, per_xcd, nslots = walk_halves(1025, 256)
    assert (per_xcd, nslots) == (129, 32)
    assert w[0][3] == [(0, True), (64, True), (128, True)] and w[1][3] == [(1, True), (65, True), (128, False)]  # idle half repeats `lead`
    assert w[2][3] == [(2, True), (66, True)]
    last = [q for q in w if q[0] == 7]
    assert last[0][3] == [(903, True), (967, True)] and last[2 * 28 + 1][3] == [(960, True), (1024, True)] and last[2 * 29][3] == [(961, True)]
    owned = sorted(t for q in w for t, o in q[3] if o)
    assert owned == list(range(1025))
    # 5 tiles on 256 CUs: per_xcd 1, one slot; half 1 of every workgroup repeats half 0's tile
    w, per_xcd, nslots = walk_halves(5, 256)
    assert (per_xcd, nslots) == (1, 1) and w[1][3] == [(0, False)] and w[10][3] == [] and w[8][3] == [(4, True)]
    # binaural (HS = 1): 600 tiles, per_xcd 75, 32 slots, both halves on the same tile, three rounds for slots 0 .. 10
    w, per_xcd, nslots = walk_halves(600, 256, hs=1)
    assert (per_xcd, nslots) == (75, 32) and w[0][3] == [(0, True), (32, True), (64, True)] and w[1][3] == [(0, False), (32, False), (64, False)]
    assert [t for t, _ in w[2 * 11][3]] == [11, 43]
    # one tile per workgroup and round: 700 tiles, per_xcd 88, 32 slots: slots 0 .. 23 take three tiles, XCD 7 holds 700 - 616 = 84
    w, per_xcd, nslots = walk_slots(700, 256)
    assert (per_xcd, nslots) == (88, 32) and [t for t, _ in w[0][3]] == [0, 32, 64] and [t for t, _ in w[24][3]] == [24, 56]
    assert [t for t, _ in w[7 * 32 + 20][3]] == [636, 668] and [t for t, _ in w[7 * 32 + 19][3]] == [635, 667, 699]
    for total, cus, hs in [(1, 256, 2), (7, 64, 2), (129, 64, 2), (1537, 304, 2), (333, 256, 1), (99, 304, 1)]:
        w = walk_halves(total, cus, hs)[0]
        assert sorted(t for q in w for t, o in q[3] if o) == list(range(total)), (total, cus, hs)
        for a, b in zip(w[::2], w[1::2]):
            assert len(a[3]) == len(b[3])  # both halves run the same number of rounds and barriers
    for total, cus in [(1, 256), (700, 64), (701, 304)]:
        assert sorted(t for q in walk_slots(total, cus)[0] for t, _ in q[3]) == list(range(total))


def test_carry_runs_match_the_launcher_by_hand():
    """istft_carry_runs, computed by hand from sgx_internal.h: cost = ceil(r batch / wgs) (len + warm-up), smallest cost, smallest r."""
    # 3 tiles, 1100 signals, 512 workgroups, overlap: r 1: 3 rounds x 3 = 9; r 2 (len 2): 5 x 3 = 15 -> stop (rounds > 1, len <= 2)
    assert carry_runs(3, 1100, 512, 3) == (1, 3)
    # 3 tiles, 100 signals, 512 workgroups: r 1: 1 x 3; r 2: 1 x (2 + 1) = 3; r 3: 1 x (1 + 1) = 2 -> R 3
    assert carry_runs(3, 100, 512, 3) == (3, 1)
    # the same without overlap: r 3: 1 x 1
    assert carry_runs(3, 100, 512, 0) == (3, 1)
    # 40 tiles, 1 signal: r 40: 1 x 2 = 2 is the first minimum (r 20: 3, r 14: 4, ...)
    assert carry_runs(40, 1, 512, 3) == (40, 1)
    # 40 tiles, 32 signals, 512 workgroups: r 14 (len 3): 448 runs, 1 x 4 = 4; r 20: 2 x 3 = 6 -> stop
    assert carry_runs(40, 32, 512, 3) == (14, 3)
    # 20 tiles, 64 signals, 256 workgroups, no overlap: r 1: 20; r 2: 10; r 3 (len 7): 7; r 4 (len 5, 256 runs): 1 x 5; r 5 (len 4): 2 x 4;
    # r 7 (len 3): 2 x 3; r 10 (len 2): 3 x 2 -> stop; R 4
    assert carry_runs(20, 64, 256, 0) == (4, 5)
    # one tile: one run
    assert carry_runs(1, 7, 256, 3) == (1, 1)


@pytest.mark.parametrize("run", FWD_RUNS, ids=fwd_id)
def test_table_selects_the_named_kernel(run):
    assert build_plan(run[0], device=HOST).kernel_name == run[0][4]


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_every_case_reaches_every_regime_it_lists(cus):
    for case, shape in FWD_RUNS:
        b, nf = choose_batch(case, shape, cus)
        g = Geometry(case, nf, b, cus)
        assert required(case, shape) <= g.regimes(), (fwd_id((case, shape)), b, g.regimes())
        # PACK: the 5-frame rows, and n_fft 512 per-bin outputs of 41 frames (22 of 64 slots empty) whatever the hop
        assert g.pack == (case[4] == "r32x16_f32" and (shape == "5" or (case[1] == 512 and shape == "41" and case[5] is None))), fwd_id((case, shape))
        if g.pack or shape == "long":
            assert ONE in Geometry(case, nf, 1, cus).regimes(), fwd_id((case, shape))
        else:
            s = one_tile_rows(case, nf, cus)
            assert ONE in Geometry(case, nf, s, cus).regimes() and not Geometry(case, nf, s, cus).pack
    for case, shape in INV_RUNS:
        b, nf = inv_choose_batch(case, shape, cus)
        g = InvGeometry(case, nf, b, cus)
        if shape == "41":
            assert INV_SHORT <= g.regimes(), (inv_id((case, shape)), b, g.regimes())
            assert ONE in InvGeometry(case, nf, max(1, g.wgs // g.tiles), cus).regimes()
        else:
            one = InvGeometry(case, nf, 1, cus)
            assert g.R > 1 and (g.R, g.run_len) != (one.R, one.run_len) and ONE in one.regimes()
            assert (WARMUP in g.regimes()) == (RESET in g.regimes()) == (g.ov > 0)


def test_packed_batches_hold_three_tiles_per_half():
    for case, shape in FWD_RUNS:
        if shape == "5":
            b, nf = choose_batch(case, shape, 256)
            g = Geometry(case, nf, b, 256)
            assert g.pack and g.total > 1024 and max(len([1 for _, o in q[3] if o]) for q in g.walkers) >= 3


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def level_rows(dtype, batch, n, n_fft, hop, seed=7):
    """[batch, n]: row r at row_level (a seed per row); every eighth row switches between 1 and 1e-4 in blocks off the hop grid, as row 0
    of test_frame_locality.py's level_batch."""
    x = np.empty((batch, n), NP[dtype])
    blk = 2 * n_fft + hop // 2 + 7
    step = np.where((np.arange(n) // blk) % 2 == 0, 1.0, 1e-4)
    for r in range(batch):
        v = np.random.default_rng((seed, r)).standard_normal(n)
        x[r] = v * step if r % 8 == 0 else v * row_level(dtype, r)
    return x


def level_spectra(dtype, batch, nb, nf, n_fft, seed=13):
    """[batch, nb, nf] random spectra (test_istft_precision.py's rand_spec): row r at row_level, every eighth row with frame f at
    10^(-4 (f mod 3)) (f64: 10^(-8 (f mod 3)))."""
    S = np.empty((batch, nb, nf), IP.CNP[dtype])
    e = 4.0 if dtype == F32 else 8.0
    for r in range(batch):
        lv = 10.0 ** (-e * (np.arange(nf) % 3)) if r % 8 == 0 else np.full(nf, row_level(dtype, r))
        S[r] = IP.rand_spec(np.random.default_rng((seed, r)), nb, nf, n_fft, lv)
    return S


# ---- the two assertions -------------------------------------------------------------------------------------------------------------
def bits(t):
    if isinstance(t, np.ndarray):
        if np.iscomplexobj(t):
            t = t.view(t.real.dtype).reshape(t.shape + (2,))
        return t.view(np.int32 if t.dtype == np.float32 else np.int64)
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def assert_same_bits(full, part, row0, where, tag):
    """Assertion 1 on rows [row0, row0 + len(part)) of `full`: [rows, bins, frames] (complex: trailing re / im) or [rows, samples]."""
    a, b = bits(full[row0:row0 + part.shape[0]]), bits(part)
    ne = a != b
    if not bool(ne.any()):
        return
    if ne.ndim == 4:
        ne = ne.any(-1)
    idx = ne.nonzero() if isinstance(ne, np.ndarray) else tuple(v.cpu().numpy() for v in ne.nonzero(as_tuple=True))
    r, f = int(idx[0][0]), int(idx[-1][0])
    raise AssertionError(f"{tag}: walk dependence: {len(idx[0])} values differ from the one-tile launch, first at {where(row0 + r, f)}"
                         + (f" bin {int(idx[1][0])}" if len(idx) == 3 else ""))


def bound_ratio(case, name, got, x64, w):
    """Assertion 2's ratio |got - ref| / bound for rows x64 -> array like got."""
    dtype, n_fft, hop, kind = case[:4]
    X = np.stack([H.np_stft(r, n_fft, hop, w) for r in x64])
    d = frame_deltas(x64, w, n_fft, hop, dtype, CB.get(name, 4.0), n_fft, paired(name, dtype, n_fft))
    got = got.astype(np.complex128 if kind == "complex" else np.float64)
    if isinstance(kind, str):
        return ratios(kind, got, X, d, dtype, None, 1e-30)
    bank, out = kind
    W = BR.bank_w64(bank, n_fft)
    ref, bound = BR.band_ref_and_bound(W, BR.w_tol(bank, W, n_fft), np.abs(X), d, dtype, bank[0] == "chroma")
    oref, obound = BR.out_ref_and_bound(bank, out, ref, bound, dtype)
    return BR.ratio(got, oref, obound)


def assert_bound(case, name, got, x64, w, where, tag, chunk=64):
    worst = 0.0
    for i0 in range(0, got.shape[0], chunk):
        g = got[i0:i0 + chunk]
        assert np.all(np.isfinite(g.view(g.real.dtype) if np.iscomplexobj(g) else g)), f"{tag}: non-finite output in rows {i0} .."
        r = bound_ratio(case, name, g, x64[i0:i0 + chunk], w)
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        worst = max(worst, float(r[i]))
        assert r[i] <= 1.0, f"{tag}: ratio to the bound {r[i]:.3g} at {where(i0 + i[0], int(i[-1]))}" + (f" bin / band {i[1]}" if r.ndim == 3 else "")
    return worst


def mfcc_chain(mel_db, kind):
    """test_gpu_fused_mfcc_keeps_the_reference_chain's fold: fmaf in ascending band order from the same launch family's Mel-dB output."""
    _, nm, n_mfcc, c0 = kind
    basis = np.cos(np.pi * np.arange(n_mfcc)[:, None] * (np.arange(nm)[None, :] + 0.5) / nm).astype(np.float32)
    acc = np.zeros((mel_db.shape[0], n_mfcc, mel_db.shape[2]), np.float32)
    for i in range(nm):
        acc = (mel_db[:, i, :][:, None, :].astype(np.float64) * basis[None, :, i, None].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    lifter = sg.MfccParams(n_mfcc).lifter
    if lifter > 0:
        acc = acc * (1.0 + (lifter / 2.0) * np.sin(np.pi * np.arange(n_mfcc) / lifter)).astype(np.float32)[None, :, None]
    return acc if c0 else acc[:, 1:]


def assert_mfcc_chain(got, mel_db, kind, where, tag):
    assert np.all(np.isfinite(got)), f"{tag}: non-finite output"
    ref = mfcc_chain(mel_db, kind)
    assert got.shape == ref.shape
    same = float(np.mean(got == ref))
    err = np.abs(got - ref)
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    lim = 4 * np.spacing(np.max(np.abs(ref)).astype(np.float32))
    assert same > 0.999 and err[i] <= lim, f"{tag}: {same:.5f} bit-equal, |d| {err[i]:.3g} (4 ulp: {lim:.3g}) at {where(int(i[0]), int(i[2]))}"
    return float(err[i] / lim)


def assert_ilr(case, got, L64, R64, w, sb, where, tag):
    """test_binaural.py's parity bound (ILR): |got - t| <= 1.01 (rho_L + rho_R) + 8 u wherever rho <= 1e-2."""
    dtype, n_fft, hop = case[:3]
    assert np.all(np.isfinite(got)), f"{tag}: non-finite output"
    worst = 0.0
    for i0 in range(0, got.shape[0], 64):
        l, r = L64[i0:i0 + 64], R64[i0:i0 + 64]
        XL = np.stack([H.np_stft(v, n_fft, hop, w) for v in l])[:, sb:sb + got.shape[1]]
        XR = np.stack([H.np_stft(v, n_fft, hop, w) for v in r])[:, sb:sb + got.shape[1]]
        dl = TB.frame_deltas(l, w, n_fft, hop, dtype, "r32x16_f32")[:, None, :]
        dr = TB.frame_deltas(r, w, n_fft, hop, dtype, "r32x16_f32")[:, None, :]
        with np.errstate(all="ignore"):
            rl, rr = dl / np.abs(XL), dr / np.abs(XR)
            t = TB.truth("ilr", XL, XR, np.arange(sb, sb + XL.shape[1]), SR / n_fft)
        good = (rl <= 1e-2) & (rr <= 1e-2)
        ratio = np.where(good, np.abs(got[i0:i0 + 64] - t) / (1.01 * (rl + rr) + 8 * U[dtype]), 0.0)
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        worst = max(worst, float(ratio[i]))
        assert ratio[i] <= 1.0, f"{tag}: ratio to the bound {ratio[i]:.3g} at {where(i0 + i[0], int(i[2]))} bin {sb + i[1]}"
    return worst


def report(key, regs, worst):
    WORST[key] = max(WORST.get(key, 0.0), float(worst))
    print(f"{key}: regimes {sorted(regs)}; 100 % of frames compared; worst ratio to bound {worst:.3g}")


# ---- 3. the checker must be able to fail (CPU) --------------------------------------------------------------------------------------
def test_checker_catches_planted_faults():
    """NumPy-made outputs (f32 per-frame rfft of the level rows) on the walk of k_r32x16 at 16 CUs: a stale frame, a leaked rounding and a
    stale 64-byte run each fail both assertions; the leak passes the many-tile tests' 2e-4 max|ref|."""
    case = (F32, 1024, 256, "complex", "r32x16_f32", None)
    pcase = case[:3] + ("power",) + case[4:]
    cus = 16
    b, nf = choose_batch(case, "41", cus)
    g = Geometry(case, nf, b, cus)
    assert SHORT_SET <= g.regimes() and b < 64
    n = n_samples(256, 1024, nf)
    x = level_rows(F32, b, n, 1024, 256)
    x64 = x.astype(np.float64)
    w = np.asarray(make_plan(F32, 1024, 256, "complex", device=HOST).window(), np.float64)
    fr = np.stack([H.np_frames(r, 1024, 256, True) for r in x64]) * w[None, None, :]
    good = np.ascontiguousarray(torch.fft.rfft(torch.from_numpy(fr.astype(np.float32)), dim=-1).numpy().transpose(0, 2, 1))  # [b, 513, nf] c64
    goodp = (good.real ** 2 + good.imag ** 2).astype(np.float32)
    ref = np.fft.rfft(fr, axis=-1).transpose(0, 2, 1)
    assert 1e-4 < assert_bound(case, "r32x16_f32", good, x64, w, g.where, "good") <= 1.0
    assert assert_bound(pcase, "r32x16_f32", goodp, x64, w, g.where, "good") <= 1.0
    assert_same_bits(good, good.copy(), 0, g.where, "good")
    assert_same_bits(torch.from_numpy(good), torch.from_numpy(good[5:9].copy()), 5, g.where, "good")

    def fails(c, bad, base):
        with pytest.raises(AssertionError, match="ratio to the bound .* previous tile"):
            assert_bound(c, "r32x16_f32", bad, x64, w, g.where, "planted")
        with pytest.raises(AssertionError, match="walk dependence: .* previous tile"):
            assert_same_bits(bad, base, 0, g.where, "planted")
        with pytest.raises(AssertionError, match="walk dependence: .* previous tile"):  # (the device tensors' path)
            assert_same_bits(torch.from_numpy(bad), torch.from_numpy(base), 0, g.where, "planted")

    # a walker whose consecutive tiles are a loud one (>= 1e3 above) and then a quiet one, and a middle tile of a walk
    pairs = [(a, c) for _, _, _, seq in g.walkers for (a, oa), (c, oc) in zip(seq, seq[1:])
             if oa and oc and row_level(F32, g.sig_of(a)) >= 1e3 * row_level(F32, g.sig_of(c)) and g.sig_of(a) % 8 and g.sig_of(c) % 8]
    assert pairs
    loud, quiet = pairs[0]
    rl, rq = g.sig_of(loud), g.sig_of(quiet)
    fl, fq = (loud % g.tps) * 16, (quiet % g.tps) * 16
    # (a) one frame of the quiet row replaced by the same frame index of the tile walked before it
    bad = good.copy()
    bad[rq, :, fq + 3] = good[rl, :, fl + 3]
    fails(case, bad, good)
    # (b) one f32 rounding of the loud tile's largest bin added to one bin of the quiet tile walked next
    leak = 2.0 ** -24 * float(np.max(np.abs(good[rl, :, fl:fl + 16])))
    bad = good.copy()
    bad[rq, 100, fq + 5] += np.float32(leak)
    fails(case, bad, good)
    # ... which the whole-batch criterion of the many-tile tests cannot see
    assert np.max(np.abs(bad - ref)) <= 2e-4 * max(1.0, float(np.max(np.abs(ref))))
    assert float(np.max(bound_ratio(case, "r32x16_f32", bad[rq:rq + 1], x64[rq:rq + 1], w))) > 1.0
    # (c) a 64-byte run (16 frames of one bin of f32 power) of a middle tile left at its previous-launch value
    mids = [seq[1][0] for _, _, _, seq in g.walkers if len(seq) >= 3 and all(o for _, o in seq) and g.sig_of(seq[1][0]) % 4 == 1
            and g.sig_of(seq[1][0]) % 8 and (seq[1][0] % g.tps + 1) * 16 <= nf]
    assert mids
    rm, fm = g.sig_of(mids[0]), (mids[0] % g.tps) * 16
    prev = level_rows(F32, b, n, 1024, 256, seed=8).astype(np.float64)
    frp = H.np_frames(prev[rm], 1024, 256, True) * w[None, :]
    stale = (np.abs(np.fft.rfft(frp, axis=-1)) ** 2).astype(np.float32).T
    bad = goodp.copy()
    bad[rm, 200, fm:fm + 16] = stale[200, fm:fm + 16]
    fails(pcase, bad, goodp)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=1)
def _inputs(dtype, batch, n, n_fft, hop):
    x = level_rows(dtype, batch, n, n_fft, hop)
    return x, torch.from_numpy(x).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("run", FWD_RUNS, ids=fwd_id)
def test_gpu_forward_walks_every_frame(run):
    case, shape = run
    dtype, n_fft, hop, kind, kernel, stage = case[:6]
    cus = cu_count()
    batch, nf = choose_batch(case, shape, cus)
    g = Geometry(case, nf, batch, cus)
    regs = g.regimes()
    assert required(case, shape) <= regs
    n = n_samples(hop, n_fft, nf)
    x, xd = _inputs(dtype, batch, n, n_fft, hop)
    plan = build_plan(case)
    w = np.asarray((make_plan(dtype, n_fft, hop, "complex", device=HOST) if kind == "ilr" else plan).window(), np.float64)
    if kind == "ilr":  # the right channel: the left one delayed by 3 samples at half the level, plus noise of the row's level
        rt = 0.5 * np.roll(x, 3, axis=1) + 0.2 * level_rows(dtype, batch, n, n_fft, hop, seed=9)
        rd = torch.from_numpy(rt.astype(NP[dtype])).cuda()
        launch = lambda a, b: plan.compute_torch(xd[a:b], rd[a:b])  # noqa: E731
    else:
        launch = lambda a, b: plan.compute_batch(xd[a:b])  # noqa: E731
    full = launch(0, batch)
    torch.cuda.synchronize()
    tag = fwd_id(run)
    assert plan.kernel_name == kernel, (tag, plan.kernel_name)
    if stage is not None:
        assert plan.bank_stage_name == stage, (tag, plan.bank_stage_name)
    assert full.shape[0] == batch and full.shape[2] == nf
    # (1) walk independence
    if (kernel, kind_tag(kind)) not in EXEMPT:
        sub = 1 if (g.pack or shape == "long") else one_tile_rows(case, nf, cus)
        assert ONE in Geometry(case, nf, sub, cus).regimes()
        for r0 in range(0, batch, sub):
            assert_same_bits(full, launch(r0, min(batch, r0 + sub)), r0, g.where, tag)
    # (2) the per-frame bound at full size
    got = full.cpu().numpy()
    x64 = x.astype(np.float64)
    if kind == "ilr":
        worst = assert_ilr(case, got.astype(np.float64), x64, rt.astype(NP[dtype]).astype(np.float64), w, plan.output_shape(n)[0], g.where, tag)
    elif isinstance(kind, tuple) and kind[0] == "mfcc":
        params = sg.SpectrogramParams(sg.StftParams(n_fft, hop, sg.WindowType.hanning, True), SR)
        mel = sg.Plan(params, _ffi.AMP_DECIBELS, sg.MelParams(kind[1], 0.0, 8000.0), sg.LogParams(BR.MFCC_FLOOR), dtype)
        worst = assert_mfcc_chain(got, mel.compute_batch(xd).cpu().numpy(), kind, g.where, tag)
    else:
        worst = assert_bound(case, kernel, got, x64, w, g.where, tag)
    report(f"{kernel} {dtype} {n_fft}/{hop} {kind_tag(kind)} {stage or ''} [{shape}] batch {batch} x {nf} frames, {g.total} tiles", regs, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("run", INV_RUNS, ids=inv_id)
def test_gpu_inverse_walks_every_sample(run):
    case, shape = run
    dtype, n_fft, hop, centre, window, name, pair, per_cu, blk = case
    cus = cu_count()
    batch, nf = inv_choose_batch(case, shape, cus)
    g = InvGeometry(case, nf, batch, cus)
    regs = g.regimes()
    plan = IP.make_plan(dtype, n_fft, hop, centre, window)
    S = level_spectra(dtype, batch, n_fft // 2 + 1, nf, n_fft)
    Sd = torch.from_numpy(S).cuda()
    full = plan.istft_batch(Sd)
    torch.cuda.synchronize()
    tag = inv_id(run)
    assert plan.istft_kernel_name == name, (tag, plan.istft_kernel_name)
    if shape == "41":
        assert INV_SHORT <= regs
        sub = max(1, g.wgs // g.tiles)
    else:
        one = InvGeometry(case, nf, 1, cus)
        assert g.R > 1 and g.run_len != one.run_len and (WARMUP in regs) == (RESET in regs) == (g.ov > 0)
        sub = 1
    assert ONE in InvGeometry(case, nf, sub, cus).regimes()
    off = n_fft // 2 if centre else 0
    where = lambda r, t: g.where(r, t + off)  # noqa: E731
    if (name, "istft") not in EXEMPT:
        for r0 in range(0, batch, sub):
            part = plan.istft_batch(Sd[r0:r0 + sub].contiguous())
            assert plan.istft_kernel_name == name
            assert_same_bits(full, part, r0, where, tag)
    got = full.cpu().numpy()
    assert np.all(np.isfinite(got)), f"{tag}: non-finite output"
    w = IP.plan_window(plan, dtype)
    worst = 0.0
    for i in range(batch):
        r = IP.ratio(got[i], IP.signal_reference(S[i], n_fft, hop, w, dtype, name, pair, got.shape[1]))
        k = int(np.argmax(r))
        worst = max(worst, float(r[k]))
        assert r[k] <= 1.0, f"{tag}: ratio to d_t {r[k]:.3g} at {where(i, k)}"
    report(f"{name} {dtype} {n_fft}/{hop} [{shape}] batch {batch} x {nf} frames, R {g.R} x {g.run_len} tiles", regs, worst)


@pytest.mark.gpu
def test_gpu_worst_ratios_per_family():
    """Runs last: the worst ratio per (kernel, kind, regime set) met by a passing case."""
    for key in sorted(WORST):
        print(f"{key}: {WORST[key]:.3g}")
    assert not EXEMPT or all(isinstance(v, str) and v for v in EXEMPT.values())
