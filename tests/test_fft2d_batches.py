"""Batched 2-D convolve, filter and FFT: every element of every image against a float64 reference, at batch sizes chosen from the
tile arithmetic of the persistent column kernel (k_colconv1024, kernels_c2c1024.hip; launch_colconv1024).

launch_colconv1024 runs `total = tiles_per_image * B` tiles on `slots = min(CUs / 8, ceil(total / 8))` workgroups per XCD; workgroup
`slot` of XCD `x` walks `lo + slot, lo + slot + slots, ...` below `hi` of the XCD's contiguous run `[x per_xcd, (x + 1) per_xcd)` and
prefetches each next tile while the current one finishes.  The batch size therefore decides whether a workgroup runs one tile or many,
whether walks have equal length, and whether a walk crosses from one image into the next.  `launches` / `regimes` below restate that
arithmetic; every GPU case asserts that its batch list covers the regimes, computed from the device's CU count.

Reference: every operator here is linear and circular (convolve_fft with pad_kernel_for_fft's centring; the radial masks with their
half-spectrum quirk S14), so for an operator L at (R, C) the impulse response h = L(delta) is taken once from the oracle and
ref(x) = irfft2(rfft2(x) * rfft2(h)) in float64 (torch.fft on the CPU).  `test_restatement_equals_the_oracle` pins this to the oracle.

Inputs: N = 300 distinct f32 images (smooth structure plus noise), image i scaled by 10^((i mod 7) - 3), so one batch spans 1e-3 ... 1e3;
batches are slices x[o : o + B] at non-zero offsets, so an image sits at different tile positions in different batches.

Bounds, per image and without a max(1, .) floor (f32; the f64 route: 1e-12 relative), m_i = max(max|x_i|, max|ref_i|) and
r_i = max(rms(x_i), rms(ref_i)):
  convolve / filter / inverse   max|got_i - ref_i| <= 2e-6 m_i,          rms(got_i - ref_i) <= 4e-7 r_i
  forward                       max|got_i - ref_i| <= 2e-6 max|ref_i|,   ||got_i - ref_i||_2 <= 1e-6 ||ref_i||_2
  and, for real outputs, the largest error of an image's 32-row x 16-column blocks (the last ones partial) at most 20 x the median's.
Where the output is no larger than the input (the Gaussian, the masks) m_i, r_i are the input's, the caps as first set.  The larger of
the two is there for the 7 x 5 random kernel: its spectrum reaches 14.8 and its output 12 x max|x|, and f32 pocketfft itself is then
at 4.9e-6 max|x| (2.3e-6 rms(x)), but at 3.9e-7 max|ref| (1.7e-7 rms(ref)).  The 4 x 6 outer product has max|ref| ~ 1.2 max|x|.
So wherever m_i is the output's, the max cap is 2e-6 max|ref_i|, 10 x tighter than the suite's earlier 2e-5 max(1, max|ref|).
The 1024 x 100 routes (generic row kernels, 100 = 4 x 25) have the rms cap 8e-7 r_i (25 x under 2e-5): their error is a uniform
4.1e-7 rms(x) with the Gaussian over every image of every scale (f32 pocketfft 1.8e-7), and their block spread is that of rounding.
`test_checker_catches_planted_faults` shows that a misplaced tile, a tile from the previous position and a 1e-4 error in the quietest
image all fail these checks, and that the reference rounded to f32 passes them.

Worst per-image ratios measured on an MI355X (max / rms or norm, over the scales above; block spread):
  gauss separable 5.2e-7 / 2.6e-7; 3.0     outer46 separable 7.3e-7 / 3.0e-7; 2.4    gauss outer 6.2e-7 / 3.5e-7; 2.5
  outer46 outer 7.3e-7 / 3.7e-7; 2.8       rand75 spectrum 6.5e-7 / 3.3e-7; 2.6      lowpass 4.9e-7 / 2.4e-7; 2.6
  highpass 3.9e-7 / 1.5e-7; 2.7            bandpass 2.3e-7 / 7.2e-8; 3.5             1024 x 100 gauss 7.9e-7 / 4.1e-7; 3.7
  1024 x 100 rand75 9.8e-7 / 5.2e-7; 3.3   1024 x 7 gauss5 4.8e-7 / 2.0e-7; 3.3     1024 x 7 rand75 5.1e-7 / 2.3e-7; 2.9
  forward 2.1e-7 / 2.1e-7                  inverse 4.4e-7 / 1.7e-7; 2.5              f64 unfused 1.4e-15 / 9.1e-16; 2.3
"""
import math

import numpy as np
import pytest
import torch

import spectrograms_amd as sg
from oracle import oracle as orc

N = 300
SEED = 20260
CONV_CAPS = (2e-6, 4e-7)   # (max, rms) relative to the larger of the input and the reference image
NARROW100_CAPS = (2e-6, 8e-7)  # the 1024 x 100 routes (generic row kernels, 100 = 4 x 25): measured, see the module docstring
BLOCK_SPREAD = 20.0        # largest / median error of an image's 32-row x 16-column blocks (f32 rounding on the CPU: <= 2.7)
FWD_CAPS = (2e-6, 1e-6)    # (max, 2-norm) relative to the reference spectrum
F64_CAPS = (1e-12, 1e-12)
SEP_TILES = 32             # separable passes: 512 row pairs / 16 per tile, each pass
CHUNK = 64                 # fft2d.hip kConvChunk: two-stream chunks from 2 * CHUNK images on (1024 x 1024 only)

# ---- inputs ------------------------------------------------------------------------------------------------------------------------


def image_scale(i):
    return 10.0 ** ((i % 7) - 3)


def master_images(idx, R, C):
    """f32 images [len(idx), R, C] on the CPU; image i depends on (i, R, C) only."""
    r = torch.arange(R, dtype=torch.float64)[:, None]
    c = torch.arange(C, dtype=torch.float64)[None, :]
    out = torch.empty((len(idx), R, C), dtype=torch.float32)
    for n, i in enumerate(idx):
        g = torch.Generator().manual_seed(SEED * 1000 + i)
        f = 0.002 + 0.05 * torch.rand(6, generator=g, dtype=torch.float64)
        p = 2 * math.pi * torch.rand(3, generator=g, dtype=torch.float64)
        smooth = torch.sin(f[0] * r + p[0]) + torch.cos(f[1] * c + p[1]) + 0.5 * torch.sin(f[2] * r + f[3] * c + p[2])
        noise = 0.1 * torch.randn((R, C), generator=g, dtype=torch.float64)
        out[n] = (image_scale(i) * (smooth + noise)).float()
    return out


def offset(B, n=N):
    """A non-zero start for a batch of B of the n master images (0 only when B == n)."""
    return 0 if B == n else 1 + (37 * B) % (n - B)


# ---- reference ---------------------------------------------------------------------------------------------------------------------

RNG = np.random.default_rng(7)
KERNELS = {
    "gauss": sg.gaussian_kernel_2d(9, 2.0, dtype="float32"),
    "gauss5": sg.gaussian_kernel_2d(5, 2.0, dtype="float32"),
    "outer46": np.outer(RNG.standard_normal(4), RNG.standard_normal(6)).astype(np.float32),  # rank 1, even sizes
    "rand75": RNG.standard_normal((7, 5)).astype(np.float32),                               # not rank 1
    "box15": np.ones((1, 5), np.float32) / 5,
    "col91": np.linspace(1.0, 2.0, 9, dtype=np.float32)[:, None],
}
FILTERS = {"low": (0, 0.3, 0.0), "high": (1, 0.2, 0.0), "band": (2, 0.1, 0.6)}
_H = {}


def impulse_response(op, R, C, dtype="float32"):
    """h = L(delta) through the oracle, float64 [R, C]."""
    d = np.zeros((R, C))
    d[0, 0] = 1.0
    if op in FILTERS:
        return orc.filter2d(d, *FILTERS[op])
    k = KERNELS[op] if dtype == "float32" else sg.gaussian_kernel_2d(9, 2.0, dtype="float64")
    return orc.convolve_fft(d, k.astype(np.float64))


def transfer(op, R, C, dtype="float32"):
    """rfft2 of the operator's impulse response, complex128 [R, C // 2 + 1] (cached)."""
    key = (op, R, C, dtype)
    if key not in _H:
        _H[key] = torch.fft.rfft2(torch.from_numpy(impulse_response(op, R, C, dtype)))
    return _H[key]


def reference(x, H):
    """ref(x) = irfft2(rfft2(x) * H) in float64, x [B, R, C] (any real dtype)."""
    R, C = x.shape[-2:]
    return torch.fft.irfft2(torch.fft.rfft2(x.double()) * H, s=(R, C))


# ---- the per-image checker ---------------------------------------------------------------------------------------------------------


def image_ratios(got, ref, x=None):
    """Per image: (max|got - ref|, ||got - ref||_2) over the larger of (max|x|, max|ref|) and of (||x||_2, ||ref||_2), or over those of
    `ref` alone when x is None.  Real or complex (a trailing (re, im) axis is not expected: pass complex tensors).  A non-finite
    difference gives inf."""
    d = (got.to(ref.dtype) - ref).abs().flatten(1)
    d = torch.nan_to_num(d, nan=math.inf, posinf=math.inf)
    r = ref.abs().flatten(1)
    smax, snorm = r.amax(1), r.pow(2).sum(1).sqrt()
    if x is not None:
        s = x.double().abs().flatten(1)
        smax, snorm = torch.maximum(smax, s.amax(1)), torch.maximum(snorm, s.pow(2).sum(1).sqrt())
    return (d.amax(1) / smax).numpy(), (d.pow(2).sum(1).sqrt() / snorm).numpy()


def block_spread(got, ref):
    """Per real image [B, R, C]: the largest over the median of the max errors of its 32-row x 16-column blocks, the last row and column
    blocks partial where R, C are not multiples (1024 x 100: six blocks of 16 columns and one of 4).  Rounding spreads over the whole
    image (2 ... 2.7 for f32 on the CPU); a misplaced tile stands out by orders of magnitude even where a cap would let it by."""
    B, R, C = got.shape
    d = torch.nan_to_num((got.to(ref.dtype) - ref).abs(), nan=math.inf)
    d = torch.nn.functional.pad(d, (0, -C % 16, 0, -R % 32))  # zeros: a partial block's max is that of its own elements
    b = d.reshape(B, -(-R // 32), 32, -(-C // 16), 16).amax(dim=(2, 4)).flatten(1)
    return (b.amax(1) / b.median(1).values.clamp_min(1e-300)).numpy()


def locate(got, ref, i):
    """Where image i's largest error sits: row, column, 32-row block, 16-column block."""
    d = torch.nan_to_num((got[i].to(ref.dtype) - ref[i]).abs(), nan=math.inf)
    r, c = divmod(int(d.argmax()), d.shape[1])
    return f"row {r} col {c} (row block {r // 32}, col block {c // 16})"


class Checker:
    """Accumulates per-image ratios over chunks of a batch, then asserts every image within its caps."""

    def __init__(self, caps):
        self.caps = caps
        self.emax, self.enorm, self.spread, self.where = [], [], [], {}

    def add(self, got, ref, x=None, first=0):
        a, b = image_ratios(got, ref, x)
        ok = (a <= self.caps[0]) & (b <= self.caps[1])
        if x is not None:  # real images: the error must also be spread over the image
            sp = block_spread(got, ref)
            ok &= sp <= BLOCK_SPREAD
            self.spread.append(sp)
        for j in np.flatnonzero(~ok):
            self.where[first + int(j)] = locate(got, ref, int(j))
        self.emax.append(a)
        self.enorm.append(b)

    def result(self, what=""):
        a, b = np.concatenate(self.emax), np.concatenate(self.enorm)
        sp = np.concatenate(self.spread) if self.spread else np.zeros_like(a)
        bad = sorted(self.where)
        assert not bad, (f"{what}: {len(bad)} of {len(a)} images out of bounds (caps {self.caps}, block spread "
                         f"{BLOCK_SPREAD}); first: " + "; ".join(f"image {i}: max {a[i]:.3g}, norm {b[i]:.3g}, spread {sp[i]:.3g} at "
                                                                  f"{self.where[i]}" for i in bad[:8]))
        return float(a.max()), float(b.max()), float(sp.max())


def check_images(got, ref, x=None, caps=CONV_CAPS, what=""):
    ck = Checker(caps)
    ck.add(got, ref, x)
    return ck.result(what)


# ---- tile regimes of launch_colconv1024 --------------------------------------------------------------------------------------------


def colconv_tiles(C):
    return (C // 2 + 1 + 15) // 16


def launches(route, B, C=1024, sep_group=512):
    """(tiles per image, images) of every k_colconv1024 launch a convolve / filter call of B images makes (fft2d.hip)."""
    if route == "separable":
        return [(SEP_TILES, min(sep_group, B - b0)) for b0 in range(0, B, sep_group) for _ in range(2)]
    t = colconv_tiles(C)
    if C == 1024 and B >= 2 * CHUNK:
        return [(t, min(CHUNK, B - b0)) for b0 in range(0, B, CHUNK)]
    return [(t, B)]


def walks(tiles, batch, cus):
    """The tile indices each workgroup walks in one launch."""
    total = tiles * batch
    per_xcd = (total + 7) // 8
    slots = max(1, min(cus // 8, per_xcd))
    return [list(range(x * per_xcd + s, min(x * per_xcd + per_xcd, total), slots)) for x in range(8) for s in range(slots)]


def regimes(route, B, cus, C=1024, sep_group=512):
    out = set()
    for tiles, nb in launches(route, B, C, sep_group):
        w = [t for t in walks(tiles, nb, cus) if t]
        n = [len(t) for t in w]
        if max(n) == 1:
            out.add("one tile")
        if len(set(n)) > 1:
            out.add("unequal walks")
        if any(len({t // tiles for t in wk}) > 1 for wk in w):
            out.add("walk crosses an image")
        if max(n) >= 8:
            out.add("8+ tiles")
    if route != "separable" and C == 1024 and B >= 2 * CHUNK and B % CHUNK:
        out.add("ragged last chunk")
    return out


FOUR = {"one tile", "unequal walks", "walk crosses an image", "8+ tiles"}


def covered(route, batches, cus, C=1024):
    return set().union(*(regimes(route, B, cus, C) for B in batches))


# ---- CPU: the reference, the checker, the regime arithmetic ------------------------------------------------------------------------

RESTATE_CASES = [((64, 48), ["gauss", "outer46", "rand75", "box15", "col91"]), ((37, 50), ["gauss", "outer46", "rand75", "box15", "col91"]),
                 ((33, 20), ["gauss", "outer46", "rand75", "box15", "col91"]), ((1024, 100), ["gauss", "outer46", "rand75", "box15"]),
                 ((1024, 7), ["gauss5", "rand75", "box15", "col91"]), ((1024, 1024), ["gauss", "outer46", "rand75", "col91"])]


@pytest.mark.parametrize("shape,ops", RESTATE_CASES, ids=[f"{s[0]}x{s[1]}" for s, _ in RESTATE_CASES])
def test_restatement_equals_the_oracle(shape, ops):
    """irfft2(rfft2(x) * rfft2(L(delta))) is the oracle's convolve_fft / filter2d to 1e-12: kernels of odd and even sizes, 1 x n and
    n x 1 (pad_kernel_for_fft's centring), rank 1 or not, and the three radial masks (built on the half spectrum's dims, S14)."""
    R, C = shape
    x = master_images([3, 11], R, C).double()
    for op in ops + list(FILTERS):
        ref = reference(x, transfer(op, R, C))
        for i in range(2):
            xi = x[i].numpy()
            o = orc.filter2d(xi, *FILTERS[op]) if op in FILTERS else orc.convolve_fft(xi, KERNELS[op].astype(np.float64))
            assert np.max(np.abs(ref[i].numpy() - o)) <= 1e-12 * np.max(np.abs(o)), (op, shape)
    # the forward transform of the f32 / f64 routes is torch's rfft2: pinned to the oracle's fft2d here too
    assert np.max(np.abs(torch.fft.rfft2(x[0]).numpy() - orc.fft2d(x[0].numpy()))) <= 1e-12 * np.max(np.abs(orc.fft2d(x[0].numpy())))


def test_master_images_span_six_decades_and_differ():
    x = master_images(range(8), 64, 48)
    peak = x.abs().flatten(1).amax(1)
    assert float(peak.max() / peak.min()) > 1e5
    assert torch.equal(master_images([5], 64, 48)[0], x[5])  # an image does not depend on the others
    assert not torch.equal(x[0], x[7])                       # same scale, other image
    assert all(offset(B) > 0 and offset(B) + B <= N for B in range(1, N))


def test_checker_catches_planted_faults():
    """A correct f32 output passes; each planted fault fails the per-image check, among them one that the suite's earlier whole-batch
    bound 2e-5 max(1, max|ref|) misses."""
    R = C = 1024
    x = master_images(range(8), R, C)          # scales 1e-3 ... 1e3, and image 7 again at 1e-3
    ref = reference(x, transfer("gauss", R, C))
    good = ref.float()
    assert check_images(good, ref, x)[0] < 0.1 * CONV_CAPS[0]

    def fails(bad):
        with pytest.raises(AssertionError, match="out of bounds"):
            check_images(bad, ref, x)

    bad = good.clone()
    bad[0, :, 512:528] = good[7, :, 512:528]         # a 16-column tile from another image of the same scale
    fails(bad)
    bad = good.clone()
    bad[7, 256:288, :] = good[0, 256:288, :]         # a 32-row block from another image of the same scale
    fails(bad)
    bad = good.clone()
    bad[3, 288:320, :] = good[3, 256:288, :]         # a tile replaced by the previous tile of the same image
    fails(bad)
    with pytest.raises(AssertionError, match="spread"):  # ... which the block spread flags even with no cap at all
        check_images(bad, ref, x, caps=(1.0, 1.0))
    bad = good.clone()
    bad[0, :, 528:544] = good[0, :, 512:528]         # ... and a column tile
    fails(bad)
    q = int(x.abs().flatten(1).amax(1).argmin())     # the quietest image
    bad = good.clone()
    bad[q, 700, 300] += 1e-4 * float(ref[q].abs().max())
    fails(bad)
    whole = float((bad.double() - ref).abs().max())
    assert whole <= 2e-5 * max(1.0, float(ref.abs().max()))  # the whole-batch bound does not see it
    # an output larger than the input: f32 pocketfft with the 7 x 5 random kernel (max|H| 14.8) is within 0.5 x the caps of the
    # output's scale, and above the max cap when measured against max|x| alone; its output is ~ 12 x max|x|
    H = transfer("rand75", R, C)
    ref = reference(x, H)
    y32 = torch.fft.irfft2(torch.fft.rfft2(x) * H.to(torch.complex64), s=(R, C))
    a, b, _ = check_images(y32, ref, x)
    assert a < 0.5 * CONV_CAPS[0] and b < 0.5 * CONV_CAPS[1]
    d = (y32.double() - ref).abs().flatten(1).amax(1)
    assert float((d / x.abs().flatten(1).amax(1)).max()) > CONV_CAPS[0]
    assert float((ref.abs().flatten(1).amax(1) / x.abs().flatten(1).amax(1)).min()) > 8
    # the forward checker: a spectrum tile from another image, and a per-image 1e-4 relative error
    S = torch.fft.rfft2(x[:2].double())
    Sg = S.to(torch.complex64)
    assert check_images(Sg, S, caps=FWD_CAPS)[0] < 0.1 * FWD_CAPS[0]
    bad = Sg.clone()
    bad[1, 32:64, 16:32] = Sg[0, 32:64, 16:32]
    with pytest.raises(AssertionError, match="out of bounds"):
        check_images(bad, S, caps=FWD_CAPS)
    bad = Sg.clone()
    bad[0, 5, 5] += 1e-4 * float(S[0].abs().max())
    with pytest.raises(AssertionError, match="out of bounds"):
        check_images(bad, S, caps=FWD_CAPS)


def test_kernel_name_is_empty_before_any_call():
    plan = sg.Fft2dPlan(1024, 1024, "float32", device=-2)
    assert plan.kernel_name == ""
    with pytest.raises(Exception, match="no HIP device"):  # a failed call names no route
        plan.convolve(np.zeros((1, 1024, 1024), np.float32), KERNELS["gauss"])
    assert plan.kernel_name == ""


def test_regime_arithmetic_matches_the_launch_formula():
    """The tile regimes quoted for 256 CUs (32 workgroups per XCD) and the coverage of the GPU batch lists."""
    cus = 256
    assert regimes("separable", 8, cus) == {"one tile"}
    w = [len(t) for t in walks(SEP_TILES, 9, cus)]
    assert w.count(2) == 4 * 8 and w.count(1) == 28 * 8  # B = 9: per_xcd 36, four of the 32 slots of each XCD walk 2 tiles
    assert "walk crosses an image" in regimes("separable", 9, cus)
    assert {len(t) for t in walks(SEP_TILES, 40, cus)} == {5}
    assert max(len(t) for t in walks(SEP_TILES, 512, cus)) == 64
    assert colconv_tiles(1024) == 33 and colconv_tiles(100) == 4 and colconv_tiles(7) == 1
    assert launches("colconv", 129) == [(33, 64), (33, 64), (33, 1)]
    assert launches("separable", 40, sep_group=9) == [(32, 9)] * 8 + [(32, 4)] * 2
    for route, batches in BATCHES.items():
        assert covered(ROUTE_OF[route], batches, cus) >= NEED[route], route


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

BATCHES = {
    "separable": [1, 8, 9, 17, 40, 65, 127, 129, 300],
    "outer": [1, 9, 63, 64, 65, 127, 128, 129, 193, 300],
    "spectrum": [1, 9, 63, 64, 65, 127, 128, 129, 193, 300],
    "mask": [9, 65, 129, 300],
}
ROUTE_OF = {"separable": "separable", "outer": "colconv", "spectrum": "colconv", "mask": "colconv"}
NEED = {"separable": FOUR, "outer": FOUR | {"ragged last chunk"}, "spectrum": FOUR | {"ragged last chunk"},
        "mask": {"unequal walks", "walk crosses an image", "8+ tiles", "ragged last chunk"}}
NARROW_BATCHES = [1, 9, 65, 129, 300]
FFT_BATCHES = [9, 65, 129, 300]
WORST = {}


def report(name, worst):
    WORST[name] = worst
    print(f"\n[fft2d batches] {name}: worst per-image max ratio {worst[0]:.3g}, norm ratio {worst[1]:.3g}, block spread {worst[2]:.3g}")


@pytest.fixture
def clean_env(monkeypatch):
    for v in ("SGX_CONV_RANK1", "SGX_CONV_SEPARABLE", "SGX_SEP_GROUP"):
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def masters():
    """masters(R, C): the N master images at (R, C) on cuda:0, built once per shape and freed after this module's tests."""
    dev = {}

    def get(R, C):
        if (R, C) not in dev:
            x = torch.empty((N, R, C), dtype=torch.float32, device="cuda")
            for i0 in range(0, N, 20):
                x[i0:i0 + 20].copy_(master_images(range(i0, min(N, i0 + 20)), R, C))
            dev[(R, C)] = x
        return dev[(R, C)]

    yield get
    dev.clear()
    torch.cuda.empty_cache()


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def expected_route(route, B, C=1024):
    name = {"separable": "separable", "outer": "colconv_outer", "spectrum": "colconv_spectrum", "mask": "colconv_mask"}[route]
    return name + "/chunked" if route != "separable" and C == 1024 and B >= 2 * CHUNK else name


def op_call(op):
    if op in FILTERS:
        return lambda plan, x: plan.filter_torch(x, *FILTERS[op])
    return lambda plan, x: plan.convolve_torch(x, KERNELS[op])


def compare_chunks(y, x, H, caps, what, chunk=16):
    """Every image of y [B, R, C] (device) against reference(x) with H, in chunks on the CPU."""
    ck = Checker(caps)
    for i0 in range(0, x.shape[0], chunk):
        xc = x[i0:i0 + chunk].cpu()
        ck.add(y[i0:i0 + chunk].cpu(), reference(xc, H), xc, first=i0)
    return ck.result(what)


def batch_consistency(call, plan, x, full, batches, route_of_b):
    """Each B < N: its slice of the master set at a non-zero offset gives the bits of the full run, and so does a repeat."""
    for B in batches:
        if B == x.shape[0]:
            continue
        o = offset(B, x.shape[0])
        xs = x[o:o + B]
        y = call(plan, xs)
        if route_of_b:
            assert plan.kernel_name == route_of_b(B), (B, plan.kernel_name)
        y2 = call(plan, xs)
        torch.cuda.synchronize()
        assert torch.equal(y, y2), f"B={B}: a repeated launch differs"
        if not torch.equal(y, full[o:o + B]):
            d = (y - full[o:o + B]).abs().flatten(1).amax(1)
            bad = torch.nonzero(d).flatten().tolist()
            raise AssertionError(f"B={B} at offset {o}: images {[o + b for b in bad[:10]]} differ from the N={x.shape[0]} run "
                                 f"(max {float(d.max()):.3g})")


CONV_CASES = [("gauss", "separable"), ("outer46", "separable"), ("gauss", "outer"), ("outer46", "outer"), ("rand75", "spectrum"),
              ("low", "mask"), ("high", "mask"), ("band", "mask")]


@pytest.mark.gpu
@pytest.mark.parametrize("op,route", CONV_CASES, ids=[f"{o}-{r}" for o, r in CONV_CASES])
def test_gpu_conv_1024_every_image_every_batch(op, route, clean_env, masters):
    """1024 x 1024 f32 convolve / filter on the fused routes: the N = 300 run against the f64 reference, every image; every other batch
    of the list bit-identical to its slice of that run; every launch repeated on the same plan.  (separable: also groups of 9, 9, 9, 9, 4
    by SGX_SEP_GROUP=9 at B = 40.)"""
    cus = cu_count()
    assert covered(ROUTE_OF[route], BATCHES[route], cus) >= NEED[route], covered(ROUTE_OF[route], BATCHES[route], cus)
    if route == "outer":
        clean_env.setenv("SGX_CONV_SEPARABLE", "0")
    x = masters(1024, 1024)
    call = op_call(op)
    plan = sg.Fft2dPlan(1024, 1024, "float32")
    full = call(plan, x)
    assert plan.kernel_name == expected_route(route, N)
    torch.cuda.synchronize()
    assert torch.equal(call(plan, x), full), "a repeated N-image launch differs"
    report(f"{op}/{route}", compare_chunks(full, x, transfer(op, 1024, 1024), CONV_CAPS, f"{op}/{route}"))
    batch_consistency(call, plan, x, full, BATCHES[route], lambda B: expected_route(route, B))
    if route == "separable":
        clean_env.setenv("SGX_SEP_GROUP", "9")
        batch_consistency(call, plan, x, full, [40], lambda B: "separable")


NARROW_CASES = [((1024, 100), "gauss", "outer"), ((1024, 100), "rand75", "spectrum"), ((1024, 7), "gauss5", "outer"),
                ((1024, 7), "rand75", "spectrum")]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,op,route", NARROW_CASES, ids=[f"{s[1]}-{o}" for s, o, _ in NARROW_CASES])
def test_gpu_conv_narrow_every_image_every_batch(shape, op, route, clean_env, masters):
    """The fused column stage on narrow images (4 and 1 tiles per image; never chunked): the N = 300 run against the f64 reference,
    every other batch bit-identical to its slice, every launch repeated."""
    R, C = shape
    cus = cu_count()
    assert covered("colconv", NARROW_BATCHES, cus, C) >= {"one tile", "unequal walks", "walk crosses an image"}
    x = masters(R, C)
    call = op_call(op)
    plan = sg.Fft2dPlan(R, C, "float32")
    full = call(plan, x)
    assert plan.kernel_name == expected_route(route, N, C)
    torch.cuda.synchronize()
    assert torch.equal(call(plan, x), full)
    caps = NARROW100_CAPS if C == 100 else CONV_CAPS
    report(f"{op}/{route} {R}x{C}", compare_chunks(full, x, transfer(op, R, C), caps, f"{op} {shape}", chunk=64))
    batch_consistency(call, plan, x, full, NARROW_BATCHES, lambda B: expected_route(route, B, C))


@pytest.mark.gpu
def test_gpu_forward_inverse_every_image_every_batch(masters):
    """forward_torch (row plan + k_c2c1024) against rfft2 in f64, then inverse_torch (k_c2c1024 + k_c2r1024) of the reference spectra
    rounded to f32 against irfft2 of those spectra in f64; every batch bit-identical to its slice of the N run, every launch repeated."""
    x = masters(1024, 1024)
    plan = sg.Fft2dPlan(1024, 1024, "float32")
    fwd = lambda p, a: p.forward_torch(a)
    S = fwd(plan, x)
    torch.cuda.synchronize()
    assert torch.equal(fwd(plan, x), S)
    ck = Checker(FWD_CAPS)
    spec = torch.empty_like(S)  # the reference spectra, f32, on the device
    for i0 in range(0, N, 16):
        ref = torch.fft.rfft2(x[i0:i0 + 16].cpu().double())
        ck.add(torch.view_as_complex(S[i0:i0 + 16].cpu()), ref, first=i0)
        spec[i0:i0 + 16].copy_(torch.view_as_real(ref.to(torch.complex64)))
    report("forward", ck.result("forward"))
    batch_consistency(fwd, plan, x, S, FFT_BATCHES, None)
    del S
    inv = lambda p, a: p.inverse_torch(a)
    y = inv(plan, spec)
    torch.cuda.synchronize()
    assert torch.equal(inv(plan, spec), y)
    ck = Checker(CONV_CAPS)
    for i0 in range(0, N, 16):
        sc = torch.view_as_complex(spec[i0:i0 + 16].cpu()).to(torch.complex128)
        ck.add(y[i0:i0 + 16].cpu(), torch.fft.irfft2(sc, s=(1024, 1024)), x[i0:i0 + 16].cpu(), first=i0)
    report("inverse", ck.result("inverse"))
    batch_consistency(inv, plan, spec, y, FFT_BATCHES, None)


@pytest.mark.gpu
def test_gpu_f64_unfused_gaussian(clean_env, masters):
    """float64 1024 x 1024 (no fused f64 route): 40 images against the reference to 1e-12, B = 9 bit-identical to its slice."""
    x = masters(1024, 1024)[:40].double()
    k = sg.gaussian_kernel_2d(9, 2.0, dtype="float64")
    call = lambda p, a: p.convolve_torch(a, k)
    plan = sg.Fft2dPlan(1024, 1024, "float64")
    full = call(plan, x)
    assert plan.kernel_name == "unfused"
    torch.cuda.synchronize()
    assert torch.equal(call(plan, x), full)
    report("gauss/unfused f64", compare_chunks(full, x, transfer("gauss", 1024, 1024, "float64"), F64_CAPS, "f64"))
    batch_consistency(call, plan, x, full, [9, 40], lambda B: "unfused")


def boundary_images(route, B, cus):
    """The two images on either side of the first XCD run boundary of the (first) launch."""
    tiles, nb = launches(ROUTE_OF[route], B)[0]
    per_xcd = (tiles * nb + 7) // 8
    return (per_xcd - 1) // tiles, per_xcd // tiles


NONFINITE_CASES = [(r, v) for r in ("separable", "outer", "spectrum", "mask") for v in ("nan", "inf")]


@pytest.mark.gpu
@pytest.mark.parametrize("route,value", NONFINITE_CASES, ids=[f"{r}-{v}" for r, v in NONFINITE_CASES])
def test_gpu_non_finite_pixel_stays_in_its_image(route, value, clean_env, masters):
    """One NaN / +Inf pixel at (0, 0) or (R - 1, C - 1) of image j: image j is non-finite exactly where the f64 reference is, every
    other image is bit-identical to the clean run.  j on either side of an XCD run boundary at B = 40 (each XCD covers 5 images), and
    the 1-image last chunk at B = 129."""
    cus = cu_count()
    if route == "outer":
        clean_env.setenv("SGX_CONV_SEPARABLE", "0")
    op = {"separable": "gauss", "outer": "gauss", "spectrum": "rand75", "mask": "band"}[route]
    call = op_call(op)
    x = masters(1024, 1024)
    plan = sg.Fft2dPlan(1024, 1024, "float32")
    H = transfer(op, 1024, 1024)
    v = math.nan if value == "nan" else math.inf
    b40 = boundary_images(route, 40, cus)
    if cus == 256:
        assert b40 == (4, 5)
    for B, js in ((40, b40), (129, (128,))):
        o = offset(B)
        clean = call(plan, x[o:o + B])
        assert plan.kernel_name == expected_route(route, B)
        for j in js:
            for (r, c) in ((0, 0), (1023, 1023)):
                xb = x[o:o + B].clone()
                xb[j, r, c] = v
                y = call(plan, xb)
                torch.cuda.synchronize()
                assert torch.equal(y[:j], clean[:j]) and torch.equal(y[j + 1:], clean[j + 1:]), \
                    f"B={B}: a non-finite pixel in image {j} reached another image"
                ref = reference(xb[j:j + 1].cpu(), H)[0]
                got = y[j].cpu()
                assert torch.equal(torch.isfinite(got), torch.isfinite(ref)), \
                    f"B={B} image {j} pixel ({r}, {c}): {int(torch.isfinite(got).sum())} finite outputs, reference {int(torch.isfinite(ref).sum())}"


@pytest.mark.gpu
def test_gpu_plan_state_across_routes(clean_env, masters):
    """One plan: Gaussian -> 7 x 5 -> Gaussian three-pass -> lowpass -> Gaussian again; each result bit-identical to a fresh plan's
    (the kernel-spectrum / factor cache across routes, fft2d.hip sgx_fft2d_convolve)."""
    x = masters(1024, 1024)
    o = offset(9)
    xs = x[o:o + 9]
    plan = sg.Fft2dPlan(1024, 1024, "float32")
    steps = [("gauss", None, "separable"), ("rand75", None, "colconv_spectrum"), ("gauss", "0", "colconv_outer"),
             ("low", None, "colconv_mask"), ("gauss", None, "separable")]
    for op, sep, name in steps:
        if sep is None:
            clean_env.delenv("SGX_CONV_SEPARABLE", raising=False)
        else:
            clean_env.setenv("SGX_CONV_SEPARABLE", sep)
        call = op_call(op)
        got = call(plan, xs)
        assert plan.kernel_name == name, (op, plan.kernel_name)
        fresh = sg.Fft2dPlan(1024, 1024, "float32")
        want = call(fresh, xs)
        assert fresh.kernel_name == name
        torch.cuda.synchronize()
        assert torch.equal(got, want), (op, sep)
    with pytest.raises(sg.InvalidInputError, match="must not exceed"):  # a failed call leaves the last route named
        plan.convolve_torch(xs, np.ones((1025, 1), np.float32))
    assert plan.kernel_name == "separable"
    assert sg.Fft2dPlan(1024, 1024, "float32").kernel_name == ""
