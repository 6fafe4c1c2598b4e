"""The forward STFT kernels on both sides of their 32-bit guards: frame counts, row and output bases past 2^31 and 2^32 bytes, row lengths.

Every tuned forward kernel (k_r32x16 at n_fft 1024 and 512, k_r32x32, k_r64x32, k_d32x16, k_d512, k_d32x32) addresses a sample row and one
signal's output with 32-bit byte offsets, and its plan_geometry_* function declines the calls whose offsets would not fit; the call then runs
down the chain of resolve_geometry (plan.hip): k_reg_radix, and past that kernel's own row guard lds_radix2 / two_factor_dft / direct_dft,
which index with size_t.  Until this file no forward test allocated 2^31 bytes: a guard off by one element size, a row base formed in 32
bits or a route past the guard that misaddresses a large output would all have left the suite green.

`Plan.kernel_name` names the kernel the PLAN starts the chain on, not the one a call ran; `Plan.execute_kernel_name`
(sgx_execute_kernel_name, added with this file) names the kernel of the last successful call after its steps down the chain, as
`istft_kernel_name` does for the inverse.  Every case asserts it.

The plans are made here (`fwd_plan`, centre = False) and not by test_frame_locality.py's make_plan, which is centred: only without the
padding is frame f of a row the transform of x[f hop : f hop + n_fft], so that a slice of x is a call of its own.  The bound is that
file's: delta_f = c u_T log2(N) sqrt(N) ||x_f w|| (c = CB.get(name, 4), the pair's joint norm on the pairing routes), `deltas` restates it on
squared frame norms for NumPy and for the device and is pinned against frame_deltas on the CPU; `ratios` is imported.  No tolerance
constant is introduced.

1. The limits (CPU): the largest admitted n_frames of every guard from its formula, pinned; the kernels the plans start on.
2. Each frame-count guard, at and one frame past (GPU), complex output (8 / 16 bytes per bin: the size the guards assume), one signal made
   on the device.  At: the tuned kernel ran; EVERY element equals (torch.equal) the same plan's call on the slice of x that holds its piece of
   4096 frames; three windows of 32 frames (start, middle, end) meet the f64 bound on the host.  Past: k_reg_radix ran; the same windows;
   every element lies within twice the tuned kernel's bound of the tuned 4096-frame pieces (both are within one bound of the truth), the
   bound computed on the device from the pieces' own frame norms.  Besides the issue's seven shapes, n_fft 512 at hop 100: the "unlisted hop"
   branch of plan_geometry_r32x16_f32 runs the packed form for one signal too, so ITS third guard, 33 x 257 x 8 bytes per frame, is
   reachable (31651 frames) and has a case of its own.  Every case is repeated with linear power: half the bytes, declined at the same
   frame count (the guards count 8 / 16 bytes per bin for every output, which errs on the safe side), the kernels' other store path.
   Two signals at the limit (n_fft 1024, f32 and f64): k_r32x16 stores through one descriptor per pair of signals, 2^32 - 8176 bytes.
3. Bases (GPU).  Output: 17 (f32) / 9 (f64) signals of 65536 frames, rows beginning past 2^31 and 2^32 bytes equal their own B = 1 launches.
   Input: 5 rows of 8192 samples at sample_stride 2^28 (f32) / 2^27 (f64), NaN everywhere else, on k_r32x16, k_d32x16 and k_reg_radix
   (n_fft 400).  Packed tiles: 64 rows of 17 frames at the largest stride with 64 stride 4 < 0xfffffff0 (2^24 - 1) and at 2^24 + 1.
   Per-bin outputs do not show whether a call was packed (neither name does); a Mel-80 plan does ("r32x16_sched_packed" against
   "r32x16_sched"), so the same two strides are also run on one and the stage name asserted on each side of the guard.  At n_fft 512 /
   hop 100 the whole kernel declines past the guard and the call runs on k_reg_radix: its rows cannot equal the bits of a contiguous B = 1
   launch (which runs k_r32x16), so they are held to the B = 1 launch on the same route — the contiguous copy of the row presented with a
   row stride of 2^30, which a one-row call never uses — and, like every small case here, to the f64 bound on every frame.
   Not run: `batch x n_frames >= 0x7fffffff` needs 2^31 frames of output (at least 4 TB).
4. Row lengths.  The tuned kernels' `n_samples >= 2^29` (f32) / `2^28` (f64) cannot be reached: hop <= n_fft (validate, plan.hip) and
   the frame guard admits L frames with L (n_fft / 2 + 1) 8 < 2^31, so a row has fewer than L n_fft + n_fft < 2^29 samples; shown for every
   hop, centred or not, on the CPU.  Likewise the packed form's third guard at n_fft 1024: from 30781 frames on a row leaves at most 15 of
   its >= 30784 slots empty and is never packed.  k_reg_radix's `n_samples x es >= 2^31` (GPU): one f32 row at n_fft 256, hop 256, linear
   power, 2^29 - 1 samples (k_reg_radix) and 32 frames more (lds_radix2 accepts, so no error text is involved), windows and pieces as in 2.
5. The checker can fail (CPU): a frame shifted by one, row 16 holding row 0's data (a base wrapped modulo 2^32) and a stale 64-byte run
   each fail the assertion that would meet them.

Measured on MI355X (256 CUs; 45 GPU cases, 7.3 s for this file alone, the slowest case 0.7 s: the process's first call).  Every guard sat
where its formula says: each `at` case ran on the tuned kernel and equalled its 4096-frame pieces bit for bit, each `past` case ran on
the route the chain names, every row past 2^31 and 2^32 bytes (output and input) equalled its own launch, no NaN was read.  No library
fix was needed.  Worst ratios (information, not thresholds): windows at the guard / windows one past it (k_reg_radix) / every element
against the tuned pieces in units of twice the bound, complex | linear power:
    k_r32x16 1024/256       0.0075 / 0.0064 / 0.0062 | 0.0077 / 0.0070 / 0.0072     two signals at the limit 0.0075
    k_r32x16 512/128 (joint) 0.0069 / 0.013 / 0.0071 | 0.0071 / 0.014 / 0.0069      512/100 (packed form) 0.0070 / 0.0098 / 0.0061 | 0.0076 / 0.0099 / 0.0060
    k_r32x32 2048/512       0.0049 / 0.0048 / 0.0045 | 0.0051 / 0.0049 / 0.0046     k_r64x32 4096/1024  0.0035 / 0.0049 / 0.0033 | 0.0036 / 0.0049 / 0.0030
    k_d512 512/128 (joint)  0.011 / 0.014 / 0.0087 | 0.011 / 0.016 / 0.0088         k_d32x16 1024/256   0.013 / 0.010 / 0.0080 | 0.013 / 0.012 / 0.0085
    k_d32x32 2048/512       0.0086 / 0.0068 / 0.0047 | 0.0090 / 0.0066 / 0.0049     two f64 signals at the limit 0.011
    output bases 0.0069 (f32 x 17) / 0.013 (f64 x 9); row bases 0.0072 (k_r32x16) / 0.011 (k_d32x16) / 0.010 (k_reg_radix); packed tiles
    0.0087 at both strides (the same bits), 512/100 0.011 packed and 0.013 on k_reg_radix; k_reg_radix's row guard 0.019 at, lds_radix2
    past it 0.015, every element 0.018 of twice the bound from the k_reg_radix pieces.
The figures equal those of the 41-frame rows of test_frame_locality.py to within their scatter: a 2 GiB signal costs no precision.
"""
import math

import numpy as np
import pytest
import torch

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests import helpers as H
from tests import test_frame_locality as FL
from tests.test_frame_locality import CB, U, paired, ratios

HOST = _ffi.DEVICE_HOST_ONLY
SR = 16000.0
F32, F64 = "float32", "float64"
ES = {F32: 4, F64: 8}
TDT = {F32: torch.float32, F64: torch.float64}
PIECE = 4096  # frames per comparison launch
WIN = 32      # frames per host window
GIB = 1 << 30
WORST = {}


def _small_device():
    return torch.cuda.is_available() and torch.cuda.get_device_properties(0).total_memory < 16 * GIB


big_memory = pytest.mark.skipif(_small_device(), reason="needs a device of at least 16 GiB (the cases hold up to 6 GiB at a time)")


def need(nbytes):
    """A shortage of device memory is reported, not skipped."""
    free = torch.cuda.mem_get_info()[0]
    assert free >= nbytes + GIB // 4, f"{free / GIB:.2f} GiB free on the device, the case needs {nbytes / GIB:.2f}"


def fwd_plan(dtype, n_fft, hop, kind="complex", device=_ffi.DEVICE_CURRENT, mel=None):
    params = sg.SpectrogramParams(sg.StftParams(n_fft, hop, sg.WindowType.hanning, False), SR)
    amp = {"complex": _ffi.AMP_COMPLEX, "power": _ffi.AMP_POWER}[kind]
    return sg.Plan(params, amp, mel, None, dtype, device=device)


def n_of(nf, n_fft, hop):
    return (nf - 1) * hop + n_fft


# ---- 1. the limits -----------------------------------------------------------------------------------------------------------------
# (dtype, n_fft, hop, tuned kernel, bytes per frame in its guard); one frame past every one of them the chain names k_reg_radix
GUARDS = [
    (F32, 512, 128, "r32x16_f32", 257 * 8),         # kernels_r32x16.hip, plan_geometry_r32x16_f32: the listed hops of n_fft 512
    (F32, 1024, 256, "r32x16_f32", 513 * 8),        # the same function, n_fft 1024
    (F32, 2048, 512, "r32x32_f32", 1025 * 8),       # kernels_r32x32.hip
    (F32, 4096, 1024, "r64x32_f32", 2049 * 8),      # kernels_r64x32.hip
    (F64, 512, 128, "d512_f64", 257 * 16),          # kernels_d32x16.hip, plan_geometry_d512_f64
    (F64, 1024, 256, "d32x16_f64", 513 * 16),       # kernels_d32x16.hip
    (F64, 2048, 512, "d32x32_f64", 1025 * 16),      # kernels_d32x32.hip
    (F32, 512, 100, "r32x16_f32", 33 * 257 * 8),    # the unlisted hops of n_fft 512: the packed form's (ft + 1) bins n_frames 8
]
PAST = "reg_radix"
PACK3_1024 = 17 * 513 * 8  # want_pack's third guard at n_fft 1024 (ft 16): never the one that decides (section 4)


def guard_limit(per_frame):
    """Largest n_frames with n_frames * per_frame < 0x7fffffff."""
    return (0x7fffffff - 1) // per_frame


def _gid(c):
    return f"{c[3]}-{c[1]}-{c[2]}"


def test_guard_limits_match_the_code():
    assert [guard_limit(g[4]) for g in GUARDS] == [1044495, 523265, 261888, 131008, 522247, 261632, 130944, 31651]
    assert guard_limit(GUARDS[1][4]) == 523265  # istft1024c's (test_istft_precision.py)
    for g in GUARDS:
        L = guard_limit(g[4])
        assert L * g[4] < 0x7fffffff <= (L + 1) * g[4]
    # the packed form's guard on the batch's span: 64 rows
    s_at = packed_stride_limit(64)
    assert s_at == 2 ** 24 - 1 and 64 * s_at * 4 < 0xfffffff0 <= 64 * (s_at + 1) * 4
    # k_reg_radix's rows
    assert (2 ** 29 - 1) * 4 < 2 ** 31 <= 2 ** 29 * 4


@pytest.mark.parametrize("case", GUARDS, ids=_gid)
def test_guard_table_starts_on_the_named_kernel(case):
    dtype, n_fft, hop, kernel, _ = case
    plan = fwd_plan(dtype, n_fft, hop, device=HOST)
    assert plan.kernel_name == kernel and plan.execute_kernel_name == ""
    L = guard_limit(case[4])
    assert plan.output_shape(n_of(L, n_fft, hop)) == (n_fft // 2 + 1, L) and plan.output_shape(n_of(L + 1, n_fft, hop))[1] == L + 1


def test_generic_cases_start_on_reg_radix():
    assert fwd_plan(F32, 256, 256, "power", device=HOST).kernel_name == "reg_radix"
    assert fwd_plan(F32, 400, 160, device=HOST).kernel_name == "reg_radix"


def packed_stride_limit(batch):
    """Largest sample_stride with batch * stride * 4 < 0xfffffff0 (want_pack / plan_geometry_r32x16_f32)."""
    return (0xfffffff0 - 1) // (batch * 4)


# ---- the bound ---------------------------------------------------------------------------------------------------------------------
def deltas(nrm2, dtype, name, n_fft):
    """test_frame_locality.py's frame_deltas from the squared norms ||x_f w||^2 [..., frames] (NumPy or torch), the frames counted from
    an even one: c u_T log2(N) sqrt(N) ||x_f w||, on the pairing routes the joint norm of frames f and f ^ 1 (an odd last frame alone)."""
    if paired(name, dtype, n_fft):
        nf = nrm2.shape[-1]
        idx = np.arange(nf) ^ 1
        idx[idx >= nf] = nf - 1  # (only the last frame of an odd count: its own index)
        alone = idx == np.arange(nf)
        if torch.is_tensor(nrm2):
            partner = nrm2[..., torch.from_numpy(idx).to(nrm2.device)]
            nrm2 = nrm2 + torch.where(torch.from_numpy(alone).to(nrm2.device), torch.zeros_like(partner), partner)
        else:
            nrm2 = nrm2 + np.where(alone, 0.0, nrm2[..., idx])
    return CB.get(name, 4.0) * U[dtype] * math.log2(n_fft) * math.sqrt(n_fft) * nrm2 ** 0.5


def test_deltas_restate_frame_deltas():
    rng = np.random.default_rng(3)
    for name, dtype, n_fft, hop, nf in [("r32x16_f32", F32, 512, 128, 41), ("r32x16_f32", F32, 1024, 256, 41), ("d512_f64", F64, 512, 160, 8),
                                        ("reg_radix", F64, 400, 160, 7)]:
        x = rng.standard_normal((2, FL.n_samples(hop, n_fft, nf)))
        w = np.asarray(fwd_plan(dtype, n_fft, hop, device=HOST).window(), np.float64)
        want = FL.frame_deltas(x, w, n_fft, hop, dtype, CB.get(name, 4.0), n_fft, paired(name, dtype, n_fft))
        nrm2 = np.stack([np.sum((H.np_frames(r, n_fft, hop, True) * w) ** 2, axis=-1) for r in x])
        assert nrm2.shape == want.shape
        assert np.allclose(deltas(nrm2, dtype, name, n_fft), want, rtol=1e-15, atol=0.0)
        assert np.allclose(deltas(torch.from_numpy(nrm2), dtype, name, n_fft).numpy(), want, rtol=1e-15, atol=0.0)


def host_ratio(xw, got, kind, name, dtype, n_fft, hop, w):
    """Ratio to the bound of `got` [bins, frames] for the f64 samples xw of exactly those frames (the first one even in its row)."""
    fr = H.np_frames(np.asarray(xw, np.float64), n_fft, hop, False) * w[None, :]
    assert fr.shape[0] == got.shape[1], (fr.shape, got.shape)
    X = np.fft.rfft(fr, axis=-1).T[None]
    d = deltas(np.sum(fr ** 2, axis=-1), dtype, name, n_fft)[None]
    g = got.astype(np.complex128 if kind == "complex" else np.float64)[None]
    assert np.all(np.isfinite(g.view(np.float64))), "non-finite output"
    return ratios(kind, g, X, d, dtype)[0]


def x_of(x, f0, f1, n_fft, hop):
    """The samples of frames [f0, f1) of every row: a view."""
    return x[:, f0 * hop:n_of(f1, n_fft, hop)]


def window_starts(nf):
    return sorted({0, (nf // 2) & ~1, max(0, nf - WIN) & ~1})


def assert_windows(x, out, row, kind, name, dtype, n_fft, hop, w, tag):
    """Three windows of 32 frames (the last one up to the row's end) of out[row] against the f64 bound; the only host copies."""
    nf = out.shape[2]
    worst = 0.0
    for f0 in window_starts(nf):
        f1 = nf if f0 + WIN + 1 >= nf else f0 + WIN
        xw = x_of(x[row:row + 1], f0, f1, n_fft, hop)[0].cpu().numpy()
        r = host_ratio(xw, out[row, :, f0:f1].cpu().numpy(), kind, name, dtype, n_fft, hop, w)
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        worst = max(worst, float(r[i]))
        assert r[i] <= 1.0, f"{tag}: ratio to the f64 bound {r[i]:.3g} at row {row} frame {f0 + int(i[-1])}" + (f" bin {i[0]}" if r.ndim == 2 else "")
    return worst


def pieces(nf, piece=PIECE):
    return [(f0, min(nf, f0 + piece)) for f0 in range(0, nf, piece)]


def first_difference(a, b):
    ne = (a != b) | (a != a) | (b != b)
    idx = ne.nonzero()
    return int(idx.shape[0]), tuple(int(v) for v in idx[0])


def assert_pieces_equal(compute, x, out, n_fft, hop, tag, piece=PIECE):
    """Every element of out [rows, bins, frames] equals the call on the slice of x that holds its piece of `piece` frames."""
    for f0, f1 in pieces(out.shape[2], piece):
        part = compute(x_of(x, f0, f1, n_fft, hop))
        assert part.shape == out[:, :, f0:f1].shape, (tag, part.shape, f0, f1)
        if not torch.equal(part, out[:, :, f0:f1]):
            count, (r, k, f) = first_difference(part, out[:, :, f0:f1])
            raise AssertionError(f"{tag}: {count} values of frames {f0} .. {f1} differ from the piece's own launch, first at row {r} bin {k} frame {f0 + f}")


def assert_rows_equal(compute, x, out, rows, tag):
    """out[r] equals the B = 1 launch on row r's own samples, bit for bit."""
    for r in rows:
        part = compute(x[r:r + 1])
        if not torch.equal(part[0], out[r]):
            count, (k, f) = first_difference(part[0], out[r])
            raise AssertionError(f"{tag}: row {r}: {count} values differ from the row's own B = 1 launch, first at bin {k} frame {f}")


def pieces_ratio(compute, x, out, kind, name, dtype, n_fft, hop, w, piece=PIECE):
    """max over every element of |out - piece| / (2 x the bound of `name`, the pieces' kernel), the bound from the pieces' own frame norms,
    all on the device.  Power: both values lie within D (2 A + D) of A^2; A <= sqrt(piece) + D.  -> (worst, first frame of its piece)"""
    wd = torch.as_tensor(w, dtype=torch.float64, device=x.device)
    per = []
    for f0, f1 in pieces(out.shape[2], piece):
        xp = x_of(x, f0, f1, n_fft, hop)
        part = compute(xp)
        nrm2 = ((xp.unfold(1, n_fft, hop).to(torch.float64) * wd) ** 2).sum(-1)
        d = deltas(nrm2, dtype, name, n_fft)[:, None, :]
        diff = (out[:, :, f0:f1] - part).abs().to(torch.float64)
        if kind == "complex":
            r = diff / (2.0 * d)
        else:
            a = part.to(torch.float64).clamp_min(0.0).sqrt() + d
            r = diff / (2.0 * d * (2.0 * a + d))
        per.append(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max())
    per = torch.stack(per).cpu().numpy()
    i = int(np.argmax(per))
    return float(per[i]), pieces(out.shape[2], piece)[i][0]


def report(tag, **worst):
    WORST[tag] = worst
    print(f"{tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def randn(shape, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, dtype=TDT[dtype], device="cuda", generator=gen)


def run(plan, route):
    """compute_batch that asserts the kernel the call ran."""
    def go(xs):
        y = plan.compute_batch(xs)
        assert plan.execute_kernel_name == route, (plan.execute_kernel_name, route, tuple(xs.shape), xs.stride(0))
        return y
    return go


def no_nan(t):
    return not bool(torch.isnan(torch.view_as_real(t) if t.is_complex() else t).any())


# ---- 2. each frame-count guard, at and one past ------------------------------------------------------------------------------------
@big_memory
@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1], ids=["at", "past"])
@pytest.mark.parametrize("kind", ["complex", "power"])
@pytest.mark.parametrize("case", GUARDS, ids=_gid)
def test_gpu_frame_count_guard(case, kind, side):
    """Complex output is the size the guards assume; linear power (half of it: the guards decline it at the same frame count, which
    errs on the safe side) takes the kernels' other store path."""
    dtype, n_fft, hop, kernel, per = case
    nf = guard_limit(per) + side
    n, bins = n_of(nf, n_fft, hop), n_fft // 2 + 1
    need(n * ES[dtype] + nf * bins * 2 * ES[dtype] + GIB // 2)
    plan = fwd_plan(dtype, n_fft, hop, kind)
    assert plan.kernel_name == kernel
    route = PAST if side else kernel
    x = randn((1, n), dtype, nf)
    out = run(plan, route)(x)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, bins, nf)
    w = np.asarray(plan.window(), np.float64)
    tag = f"{dtype} {kernel} {n_fft}/{hop} {kind} {'past' if side else 'at'} {nf} frames ({route})"
    ww = assert_windows(x, out, 0, kind, route, dtype, n_fft, hop, w, tag)
    if side == 0:
        assert_pieces_equal(run(plan, kernel), x, out, n_fft, hop, tag)
        report(tag, windows=ww)
    else:
        wp, f0 = pieces_ratio(run(plan, kernel), x, out, kind, kernel, dtype, n_fft, hop, w)
        report(tag, windows=ww, pieces=wp)
        assert wp <= 1.0, f"{tag}: {wp:.3g} x twice the bound away from the tuned pieces, in frames {f0} .. {f0 + PIECE}"
    del x, out
    torch.cuda.empty_cache()


@big_memory
@pytest.mark.gpu
@pytest.mark.parametrize("case", [GUARDS[1], GUARDS[5]], ids=_gid)
def test_gpu_frame_count_guard_batch_of_two(case):
    """Two signals at the limit: the second begins less than one frame's bytes short of 2^31.  k_r32x16 stores through one descriptor per
    PAIR of signals (4 294 959 120 bytes here: unsigned offsets up to 2^32), and a signal of 32705 tiles hands its neighbour's first tile to
    the other half of the same workgroup."""
    dtype, n_fft, hop, kernel, per = case
    nf = guard_limit(per)
    n, bins = n_of(nf, n_fft, hop), n_fft // 2 + 1
    need(2 * (n * ES[dtype] + nf * bins * 2 * ES[dtype]) + GIB // 2)
    plan = fwd_plan(dtype, n_fft, hop)
    x = randn((2, n), dtype, nf + 2)
    out = run(plan, kernel)(x)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, bins, nf) and nf * per < 0x7fffffff <= (nf + 1) * per
    w = np.asarray(plan.window(), np.float64)
    tag = f"{dtype} {kernel} {n_fft}/{hop} 2 x {nf} frames"
    worst = max(assert_windows(x, out, r, "complex", kernel, dtype, n_fft, hop, w, tag) for r in (0, 1))
    assert_pieces_equal(run(plan, kernel), x, out, n_fft, hop, tag)
    report(tag, windows=worst)
    del x, out
    torch.cuda.empty_cache()


# ---- 3. row and output bases past 2^31 and 2^32 bytes --------------------------------------------------------------------------------
OUT_BASES = [(F32, 1024, 256, "r32x16_f32", 17, (0, 7, 8, 15, 16)), (F64, 1024, 256, "d32x16_f64", 9, (0, 3, 4, 7, 8))]


@big_memory
@pytest.mark.gpu
@pytest.mark.parametrize("case", OUT_BASES, ids=_gid)
def test_gpu_output_bases_past_2_31_and_2_32_bytes(case):
    dtype, n_fft, hop, kernel, batch, rows = case
    nf, bins = 65536, n_fft // 2 + 1
    n = n_of(nf, n_fft, hop)
    row_bytes = bins * nf * 2 * ES[dtype]
    assert rows[1] * row_bytes < 2 ** 31 <= rows[2] * row_bytes and rows[3] * row_bytes < 2 ** 32 <= rows[4] * row_bytes and rows[4] == batch - 1
    need(batch * (n * ES[dtype] + row_bytes) + row_bytes + GIB // 2)
    plan = fwd_plan(dtype, n_fft, hop)
    x = randn((batch, n), dtype, batch)
    out = run(plan, kernel)(x)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (batch, bins, nf)
    tag = f"{dtype} {kernel} {n_fft}/{hop} {batch} x {nf} frames"
    assert_rows_equal(run(plan, kernel), x, out, range(batch), tag)  # (every row, the named ones among them)
    w = np.asarray(plan.window(), np.float64)
    worst = max(assert_windows(x, out, r, "complex", kernel, dtype, n_fft, hop, w, tag) for r in rows[2:])
    report(tag, windows=worst)
    del x, out
    torch.cuda.empty_cache()


def assert_all_frames(rows, out, kind, name, dtype, n_fft, hop, w, tag):
    """The f64 bound on every frame of a small batch (host copies of a few hundred kilobytes)."""
    xs, got = rows.cpu().numpy(), out.cpu().numpy()
    worst = 0.0
    for r in range(xs.shape[0]):
        q = host_ratio(xs[r], got[r], kind, name, dtype, n_fft, hop, w)
        worst = max(worst, float(np.max(q)))
        assert np.max(q) <= 1.0, f"{tag}: row {r}: ratio to the f64 bound {np.max(q):.3g}"
    return worst


IN_BASES = [(F32, 1024, 256, "r32x16_f32", 28), (F64, 1024, 256, "d32x16_f64", 27), (F32, 400, 160, "reg_radix", 28)]


@big_memory
@pytest.mark.gpu
@pytest.mark.parametrize("case", IN_BASES, ids=_gid)
def test_gpu_row_bases_past_2_31_and_2_32_bytes(case):
    dtype, n_fft, hop, kernel, lg = case
    batch, n, stride = 5, 8192, 1 << lg
    assert 2 * stride * ES[dtype] == 2 ** 31 and 4 * stride * ES[dtype] == 2 ** 32  # rows 2 and 4 begin there
    need(batch * stride * ES[dtype] + GIB // 4)
    plan = fwd_plan(dtype, n_fft, hop)
    rows = randn((batch, n), dtype, lg)
    big = torch.full((batch, stride), float("nan"), dtype=TDT[dtype], device="cuda")
    big[:, :n] = rows
    xs = big[:, :n]
    assert xs.stride(0) == stride and bool(torch.isnan(big[:, n:n + 4096]).all())
    out = run(plan, kernel)(xs)
    torch.cuda.synchronize()
    tag = f"{dtype} {kernel} {n_fft}/{hop} 5 rows at sample_stride 2^{lg}"
    assert no_nan(out), f"{tag}: NaN in the output: a sample was read outside its row"
    assert_rows_equal(run(plan, kernel), rows, out, range(batch), tag)
    report(tag, frames=assert_all_frames(rows, out, "complex", kernel, dtype, n_fft, hop, np.asarray(plan.window(), np.float64), tag))
    del big, xs, out
    torch.cuda.empty_cache()


def one_row_at_stride(row, stride):
    """A [1, n] view of a contiguous row with sample_stride `stride`: a one-row call never adds the stride to an address, but the
    guards on batch x sample_stride see it."""
    return torch.as_strided(row, (1, row.shape[-1]), (stride, 1))


MEL80 = sg.MelParams(80, 0.0, 8000.0)
# (n_fft, hop, output kind or the bank, kernel at the guard, kernel past it, bank stage at / past or None)
PACKED = [(1024, 256, "power", "r32x16_f32", "r32x16_f32", None), (1024, 256, MEL80, "r32x16_f32", "r32x16_f32", ("r32x16_sched_packed", "r32x16_sched")),
          (512, 100, "power", "r32x16_f32", "reg_radix", None)]


@big_memory
@pytest.mark.gpu
@pytest.mark.parametrize("case", PACKED, ids=lambda c: f"{c[0]}-{c[1]}-{c[2] if isinstance(c[2], str) else 'mel80'}")
def test_gpu_packed_tiles_guard_on_the_batch_span(case):
    """64 rows of 17 frames: packed while 64 x sample_stride x 4 < 0xfffffff0.  The bank stage name shows the packing of a Mel plan; for
    per-bin outputs at n_fft 1024 nothing does (both sides are "r32x16_f32"), at n_fft 512 / hop 100 the kernel itself declines."""
    n_fft, hop, kind, k_at, k_past, stages = case
    dtype, batch, nf = F32, 64, 17
    n = n_of(nf, n_fft, hop)
    mel = None if isinstance(kind, str) else kind
    plan = fwd_plan(dtype, n_fft, hop, "power", mel=mel)
    assert plan.kernel_name == k_at
    rows = randn((batch, n), dtype, n_fft + hop)
    w = np.asarray(plan.window(), np.float64)
    single = torch.cat([run(plan, k_at)(rows[r:r + 1]) for r in range(batch)])  # contiguous B = 1 launches
    if stages:
        assert plan.bank_stage_name == "r32x16_sched"  # (a one-row call is never packed at n_fft 1024)
    s_at = packed_stride_limit(batch)
    for side, stride in enumerate((s_at, 2 ** 24 + 1)):
        assert (batch * stride * 4 >= 0xfffffff0) == bool(side)
        need(batch * stride * 4)
        flat = torch.full((batch * stride,), float("nan"), dtype=torch.float32, device="cuda")
        big = flat.view(batch, stride)
        big[:, :n] = rows
        route = k_past if side else k_at
        out = run(plan, route)(big[:, :n])
        torch.cuda.synchronize()
        tag = f"{dtype} {n_fft}/{hop} {'mel80' if mel else kind} 64 x 17 frames at sample_stride {stride} ({route})"
        if stages:
            assert plan.bank_stage_name == stages[side], (tag, plan.bank_stage_name)
        assert no_nan(out), f"{tag}: NaN in the output: a sample was read outside its row"
        if route == k_at:
            ref = single
        else:  # another kernel: its own B = 1 launches
            ref = torch.cat([run(plan, route)(one_row_at_stride(rows[r], 2 ** 30)) for r in range(batch)])
        if not torch.equal(out, ref):
            count, (r, k, f) = first_difference(out, ref)
            raise AssertionError(f"{tag}: {count} values differ from the rows' B = 1 launches, first at row {r} bin {k} frame {f}")
        if mel is None:
            report(tag, frames=assert_all_frames(rows, out, "power", route, dtype, n_fft, hop, w, tag))
        del flat, big, out
        torch.cuda.empty_cache()


# ---- 4. the row-length guards --------------------------------------------------------------------------------------------------------
def test_tuned_row_length_guards_lie_behind_the_frame_guards():
    """n_samples >= 2^29 (f32) / 2^28 (f64): at every hop the plan admits (1 .. n_fft) the longest row the frame guard lets through is
    shorter, centred (n_frames = n / hop + 1) or not (n_frames = (n - n_fft) / hop + 1)."""
    for dtype, n_fft, _, kernel, per in GUARDS[:7]:
        L = guard_limit(per)
        hop = np.arange(1, n_fft + 1, dtype=np.int64)
        plain, centred = L * hop + n_fft - 1, L * hop - 1  # the longest rows of L frames
        assert np.all((plain - n_fft) // hop + 1 == L) and np.all((plain + 1 - n_fft) // hop + 1 == L + 1)
        assert np.all(centred // hop + 1 == L) and np.all((centred + 1) // hop + 1 == L + 1)
        assert int(max(plain.max(), centred.max())) == L * n_fft + n_fft - 1 < (2 ** 29 if dtype == F32 else 2 ** 28), (kernel, n_fft)
        for centre in (False, True):  # the plan counts frames that way
            p = sg.Plan(sg.SpectrogramParams(sg.StftParams(n_fft, n_fft, sg.WindowType.hanning, centre), SR), _ffi.AMP_COMPLEX, None, None, dtype, device=HOST)
            n = int(centred[-1] if centre else plain[-1])
            assert p.output_shape(n)[1] == L and p.output_shape(n + 1)[1] == L + 1
    # the stricter guards of the packed form (n_fft 512, unlisted hops <= 512) only shorten the rows
    assert guard_limit(GUARDS[7][4]) * 512 + 511 < 2 ** 29
    plan = fwd_plan(F32, 1024, 1024, device=HOST)  # the longest admitted row of k_r32x16: 523265 frames at hop = n_fft
    assert plan.output_shape(523265 * 1024 + 1023)[1] == 523265 and 523265 * 1024 + 1023 < 2 ** 29


def test_packed_third_guard_is_unreachable_at_n_fft_1024():
    """(ft + 1) bins n_frames 8 >= 0x7fffffff needs 30781 frames; a row is packed only if a quarter of its 16-frame tiles' slots are empty
    (want_pack: (slots - used) 4 >= slots), and a row of nf frames leaves at most 15 empty."""
    nf0 = guard_limit(PACK3_1024) + 1
    assert nf0 == 30781
    for nf in (nf0, nf0 + 1, nf0 + 3, nf0 + 15):
        slots = -(-nf // 16) * 16
        assert (slots - nf) * 4 < slots
    assert 15 * 4 < nf0


@big_memory
@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1], ids=["at", "past"])
def test_gpu_reg_radix_row_length_guard(side):
    """One f32 row of 2^29 - 1 samples (the last k_reg_radix addresses with signed 32-bit byte offsets) and 32 frames more (lds_radix2)."""
    dtype, n_fft, hop, kind = F32, 256, 256, "power"
    n = 2 ** 29 - 1 + side * 32 * hop
    nf, bins = (n - n_fft) // hop + 1, n_fft // 2 + 1
    assert (n * 4 >= 2 ** 31) == bool(side)
    need(n * 4 + nf * bins * 4 + GIB // 2)
    plan = fwd_plan(dtype, n_fft, hop, kind)
    assert plan.kernel_name == "reg_radix"
    route = "lds_radix2" if side else "reg_radix"
    x = randn((1, n), dtype, n)
    out = run(plan, route)(x)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, bins, nf)
    w = np.asarray(plan.window(), np.float64)
    tag = f"{dtype} reg_radix {n_fft}/{hop} {kind} {'past' if side else 'at'} {n} samples ({route})"
    ww = assert_windows(x, out, 0, kind, route, dtype, n_fft, hop, w, tag)
    if side == 0:
        assert_pieces_equal(run(plan, "reg_radix"), x, out, n_fft, hop, tag)
        report(tag, windows=ww)
    else:
        wp, f0 = pieces_ratio(run(plan, "reg_radix"), x, out, kind, "reg_radix", dtype, n_fft, hop, w)
        report(tag, windows=ww, pieces=wp)
        assert wp <= 1.0, f"{tag}: {wp:.3g} x twice the bound away from the k_reg_radix pieces, in frames {f0} .. {f0 + PIECE}"
    del x, out
    torch.cuda.empty_cache()


# ---- 5. the checker can fail (CPU) -----------------------------------------------------------------------------------------------------
def test_checker_catches_planted_faults():
    """A NumPy-free stand-in for a plan (torch's f32 rfft of the windowed frames, complex [rows, 513, frames]) on 17 rows of 200 frames,
    pieces of 64 frames: the checks pass on its own output and each planted fault fails the one that would meet it on the device."""
    dtype, n_fft, hop, name, piece = F32, 1024, 256, "r32x16_f32", 64
    nf, batch = 200, 17
    n = n_of(nf, n_fft, hop)
    w = np.asarray(fwd_plan(dtype, n_fft, hop, device=HOST).window(), np.float64)
    wt = torch.from_numpy(w.astype(np.float32))

    def compute(xs):
        return torch.fft.rfft(xs.unfold(1, n_fft, hop) * wt, dim=-1).transpose(1, 2).contiguous()

    x = torch.from_numpy(np.random.default_rng(9).standard_normal((batch, n)).astype(np.float32))
    good = compute(x)
    assert tuple(good.shape) == (batch, 513, nf)
    assert_pieces_equal(compute, x, good, n_fft, hop, "good", piece)
    assert_rows_equal(compute, x, good, range(batch), "good")
    wr, _ = pieces_ratio(compute, x, good, "complex", name, dtype, n_fft, hop, w, piece)
    assert wr == 0.0
    assert 1e-4 < assert_windows(x, good, 16, "complex", name, dtype, n_fft, hop, w, "good") <= 1.0

    # (a) from frame 100 on every frame of row 0 is its successor: a tile walked one frame off
    bad = good.clone()
    bad[0, :, 100:nf - 1] = good[0, :, 101:nf]
    with pytest.raises(AssertionError, match=r"frames 64 \.\. 128 differ .* first at row 0 bin 0 frame 100"):
        assert_pieces_equal(compute, x, bad, n_fft, hop, "shifted", piece)
    assert pieces_ratio(compute, x, bad, "complex", name, dtype, n_fft, hop, w, piece)[0] > 1e3
    with pytest.raises(AssertionError, match=r"ratio to the f64 bound .* at row 0 frame 1[0-3]\d"):
        assert_windows(x, bad, 0, "complex", name, dtype, n_fft, hop, w, "shifted")
    # (b) row 16 holds row 0's data: its base wrapped modulo 2^32 bytes
    bad = good.clone()
    bad[16] = good[0]
    with pytest.raises(AssertionError, match="row 16: .* differ from the row's own B = 1 launch, first at bin 0 frame 0"):
        assert_rows_equal(compute, x, bad, (0, 7, 8, 15, 16), "wrapped")
    with pytest.raises(AssertionError, match="ratio to the f64 bound .* at row 16"):
        assert_windows(x, bad, 16, "complex", name, dtype, n_fft, hop, w, "wrapped")
    # (c) a 64-byte run (8 frames of one complex f32 bin) left at the value of an earlier call
    stale = compute(torch.from_numpy(np.random.default_rng(10).standard_normal((1, n)).astype(np.float32)))
    bad = good.clone()
    bad[0, 300, 136:144] = stale[0, 300, 136:144]
    with pytest.raises(AssertionError, match=r"8 values of frames 128 \.\. 192 differ .* first at row 0 bin 300 frame 136"):
        assert_pieces_equal(compute, x, bad, n_fft, hop, "stale", piece)
    wr, f0 = pieces_ratio(compute, x, bad, "complex", name, dtype, n_fft, hop, w, piece)
    assert wr > 1e3 and f0 == 128
    with pytest.raises(AssertionError, match="row 0: 8 values differ"):
        assert_rows_equal(compute, x, bad, (0,), "stale")
    # a NaN cannot hide in the comparison of a value with itself
    bad = good.clone()
    bad[0, 5, 7] = float("nan")
    assert pieces_ratio(compute, x, bad, "complex", name, dtype, n_fft, hop, w, piece) == (float("inf"), 0)
    with pytest.raises(AssertionError, match="first at row 0 bin 5 frame 7"):
        assert_pieces_equal(compute, x, bad, n_fft, hop, "nan", piece)
    assert not no_nan(bad) and no_nan(good)


@big_memory
@pytest.mark.gpu
def test_gpu_worst_ratios():
    """Runs last: what the passing cases measured (information, not thresholds)."""
    for tag in sorted(WORST):
        print(f"{tag}: {WORST[tag]}")
