"""Every fused MDCT instance run on the device, and its cosine matrix read back entry by entry.

k_mdct_fwd / k_imdct_ola exist once per (A, B, C) pass split and element type: 31 lengths M = window_size / 4 per dtype.  Each has
its own LDS layout, rows per round, frames per tile and register target, so each is run here.

0. `instance` restates the host arithmetic that sizes a tile (split, strides, bytes per frame, frames per tile, fused inverse or not);
   a CPU test pins it to the figures worked out by hand and to the routes the library reports.
1. Forward read-back.  One row, hop 1, a unit impulse at sample 2N - 1 of 4N - 1 samples: frame f sees it at n = 2N - 1 - f, so the
   [N, 2N] output is the operator itself, C[k, f] = w_T[n] cos(pi (2n + 1 + N)(2k + 1) / (4N)).  Above window 4096 a sampled set:
   8 rows, an odd hop, >= 512 distinct n, the fold's branch edges among them.  Per entry
       |got - ref| <= 4 u_T log2(2N) |w_T[n]|:
   with an impulse every addition is with an exact zero, the error is that of the chain of complex multiplications on one path.
2. Inverse read-back.  hop = N, identity coefficients (one-hot frames above N = 2048): block b is frame b's first half plus frame
   b - 1's second half.  Per sample |got - ref| <= 4 u_T mult (2/N) sum |w_T| + u_T sum |partial sums| (the additions of the
   overlap-add, ascending frames; one addition at hop = N, where it is u_T |ref|), mult = log2(2N), plus 2 log2(P) on chirp-z.
3. Dense parity (tests/test_mdct.py's normwise bounds) at frame counts around each instance's tile, and frame isolation with `==`:
   a frame scaled by a power of two must scale its own outputs exactly and touch no other.
4. The generic route across a 256 MiB chunk seam, bit for bit against the same plan row by row.
5. Hops past the fused forward's 32-bit sample index take the generic route (host-only).
"""
import math

import numpy as np
import pytest

import spectrograms_amd as sg
from tests import test_mdct as TM

LD = np.longdouble
U, NP, CB, HOST = TM.U, TM.NP, TM.CB, TM.HOST
DTYPES = ["float32", "float64"]

# ---- 0. the instances ----------------------------------------------------------------------------------------------------------
MIXED = {40: (8, 5), 60: (10, 6), 80: (10, 8), 100: (10, 10), 120: (12, 10), 160: (16, 10), 200: (25, 8), 240: (16, 15),
         300: (20, 15), 320: (20, 16), 400: (25, 16), 480: (24, 20), 500: (25, 20), 600: (25, 24), 720: (30, 24), 800: (32, 25),
         960: (32, 30), 640: (16, 40), 1000: (25, 40), 1080: (30, 36), 1200: (30, 40), 1280: (32, 40)}  # kMixedSplits
LENGTHS = sorted([1 << p for p in range(4, 13)] + list(MIXED))
WINDOWS = [4 * m for m in LENGTHS]
LDS_BUDGET = 72 * 1024  # kMdctLds


def split(M, dtype):
    """(A, B, C) of reg_split_len, None where M has no pass split."""
    if M >= 16 and M & (M - 1) == 0 and M <= 4096:
        l2 = M.bit_length() - 1
        if l2 <= (6 if dtype == "float64" else 8):
            return 1 << ((l2 + 1) // 2), 1 << (l2 // 2), 1
        return 1 << ((l2 + 2) // 3), 1 << ((l2 + 1) // 3), 1 << (l2 // 3)
    return (*MIXED[M], 1) if M in MIXED else None


def instance(ws, dtype):
    """(split, bytes per frame, frames per tile, inverse fused at hop == N) of window size ws, None where the forward is not fused."""
    if ws % 4 or split(ws // 4, dtype) is None:
        return None
    a, b, c = split(ws // 4, dtype)
    rs = b * c + 1 if c == 1 else b * c  # rr_swizzle: every three-pass entry of its table has rs = B C
    per = ((a * rs) | 1) * (16 if dtype == "float64" else 8)  # rr_frame_stride, complex elements
    if per > LDS_BUDGET:
        return None
    tile = 32
    while tile > 1 and tile * per > LDS_BUDGET:
        tile //= 2
    return (a, b, c), per, tile, tile >= 4


def stated_tile(ws, dtype):
    """The frames per tile worked out by hand from the 72 KiB budget."""
    steps = {"float32": [(1024, 32), (2048, 16), (4320, 8), (8192, 4), (16384, 2)],
             "float64": [(512, 32), (1024, 16), (2048, 8), (4320, 4), (8192, 2), (16384, 1)]}[dtype]
    return next(t for top, t in steps if ws <= top)


def test_instance_table():
    assert len(WINDOWS) == 31 and len(set(WINDOWS)) == 31
    for dtype in DTYPES:
        splits = set()
        for ws in WINDOWS:
            (a, b, c), per, tile, inv = instance(ws, dtype)
            assert a * b * c == ws // 4
            splits.add((a, b, c))
            assert tile == stated_tile(ws, dtype), (ws, dtype, per, tile)
            assert tile * per <= LDS_BUDGET and (tile == 32 or 2 * tile * per > LDS_BUDGET)
            p = sg.MdctPlan(sg.MdctParams.sine_window(ws), dtype, device=HOST)
            assert p.kernel_name() == "k_mdct_fwd", (ws, dtype)
            assert p.kernel_name(True) == ("k_imdct_ola" if inv else "imdct_generic"), (ws, dtype)
        assert len(splits) == 31
    assert instance(512, "float64")[0] == (8, 4, 4) and instance(512, "float32")[0] == (16, 8, 1)
    # the tile shapes no other test runs: a 4-frame inverse tile, a 2-frame f64 forward tile
    assert [ws for ws in WINDOWS if instance(ws, "float32")[2] == 4] == [4800, 5120, 8192]
    assert [ws for ws in WINDOWS if instance(ws, "float64")[2] == 4] == [2400, 2560, 2880, 3200, 3840, 4000, 4096, 4320]
    assert [ws for ws in WINDOWS if instance(ws, "float64")[2] == 2] == [4800, 5120, 8192]
    assert [ws for ws in WINDOWS if not instance(ws, "float32")[3]] == [16384]
    assert [ws for ws in WINDOWS if not instance(ws, "float64")[3]] == [4800, 5120, 8192, 16384]
    assert instance(1000, "float32") is None and instance(66, "float64") is None


# ---- 5. hops past the 32-bit sample index ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_large_hop_takes_generic_forward(dtype):
    """k_mdct_fwd reads xt[s hop + i] with s <= 31, i < 2N in 32 bits: fused only while 31 hop + 2N <= 2^32."""
    ws = 256
    hop = (2 ** 32 - ws) // 31
    assert 31 * hop + ws <= 2 ** 32 < 31 * (hop + 1) + ws and hop + 1 < 2 ** 31
    assert sg.MdctPlan(sg.MdctParams(ws, hop, sg.WindowType.hanning), dtype, device=HOST).kernel_name() == "k_mdct_fwd"
    assert sg.MdctPlan(sg.MdctParams(ws, hop + 1, sg.WindowType.hanning), dtype, device=HOST).kernel_name() == "mdct_generic"
    assert sg.MdctPlan(sg.MdctParams(ws, 2 ** 31 - 1, sg.WindowType.hanning), dtype, device=HOST).kernel_name() == "mdct_generic"


# ---- the restatement on index subsets -------------------------------------------------------------------------------------------
def cos_sub(N, ks, ns, dt):
    """TM._cosm(N, dt)[ks][:, ns] without the whole matrix: the same integer reduction, the same expression."""
    r = np.outer(2 * np.asarray(ks, np.int64) + 1, 2 * np.asarray(ns, np.int64) + 1 + N) % (8 * N)
    pi = TM._PI_LD if dt is LD else np.float64(np.pi)
    return np.cos(r.astype(dt) * pi / dt(4 * N))


def ref_dt(dtype):
    return LD if dtype == "float64" else np.float64


def test_cos_sub_is_cosm():
    for N, dt in ((16, LD), (30, np.float64), (100, LD)):
        ks, ns = np.array([0, 1, N // 2, N - 1]), np.array([0, N - 1, N, 2 * N - 1, 7])
        np.testing.assert_array_equal(cos_sub(N, ks, ns, dt), TM._cosm(N, dt)[ks][:, ns])


def window_t(plan, dtype):
    """plan.window() as the kernels hold it: cast to the plan's type."""
    return plan.window().astype(NP[dtype]).astype(np.float64)


def _sine(ws):
    return sg.WindowType.custom(np.sin(np.pi * (np.arange(ws, dtype=np.float64) + 0.5) / ws))


def _entries(got, ref, bnd, name, where):
    """Per entry |got - ref| <= bnd; the worst ratio recorded as tests/test_mdct.py records its own."""
    err = got.astype(ref.dtype)
    err -= ref
    np.abs(err, out=err)
    bnd = np.broadcast_to(bnd, err.shape)
    ok = err <= bnd
    pos = bnd > 0
    TM._record(name, (err[pos] / bnd[pos]).max() if pos.any() else 0.0)
    if not ok.all():
        bad = np.argwhere(~ok)
        worst = tuple(bad[np.argmax([float(err[tuple(i)] - bnd[tuple(i)]) for i in bad[:4096]])])
        raise AssertionError(f"{name}: {len(bad)} of {ok.size} entries past the bound; first {[where(*i) for i in bad[:6]]}; worst "
                             f"{where(*worst)} got {got[worst]!r} ref {float(ref[worst])!r} bound {float(bnd[worst]):.3g}")


# ---- 1. forward read-back --------------------------------------------------------------------------------------------------------
def sampled_forward_design(N):
    """(hop, n_frames, impulse position per row): 8 rows, row r's impulse seen at n = e_r (mod hop) by every frame that holds it,
    e_r the first and last sample of each quarter of the frame; the residues differ, so the rows hit >= 8 floor(2N / hop) >= 512 n."""
    two_n, h = 2 * N, N // 2
    edges = [0, h - 1, h, 2 * h - 1, 2 * h, 3 * h - 1, 3 * h, 4 * h - 1]
    hop = (two_n // 64 - 1) | 1
    while len({e % hop for e in edges}) < 8:
        hop -= 2
    nf = -(-two_n // hop) + 2
    pos = [e + -(-(two_n - 1 - e) // hop) * hop for e in edges]  # in [2N - 1, 2N - 1 + hop): every frame that holds it exists
    return hop, nf, pos, edges


def sampled_forward_positions(N):
    hop, nf, pos, edges = sampled_forward_design(N)
    n = np.asarray(pos)[:, None] - np.arange(nf)[None, :] * hop  # [row, frame]
    return hop, nf, pos, edges, n, (n >= 0) & (n < 2 * N)


@pytest.mark.parametrize("ws", [w for w in WINDOWS if w > 4096])
def test_sampled_forward_design(ws):
    N = ws // 2
    hop, nf, pos, edges, n, valid = sampled_forward_positions(N)
    hit = set(n[valid].tolist())
    assert hop % 2 == 1 and hop >= 3 and len(hit) >= 512 and len(hit) == valid.sum() and set(edges) <= hit
    assert max(pos) < ws + (nf - 1) * hop


def _forward_readback(ws, dtype, win, label):
    N, dt, u = ws // 2, ref_dt(dtype), U[dtype]
    tol = CB * u * math.log2(ws)
    name = f"readback forward {label} {dtype} {instance(ws, dtype)[0]}"
    if ws <= 4096:
        plan = sg.MdctPlan(sg.MdctParams(ws, 1, win), dtype)
        assert plan.kernel_name() == "k_mdct_fwd"
        w = window_t(plan, dtype)
        x = np.zeros(4 * N - 1, NP[dtype])
        x[2 * N - 1] = 1
        got = plan.forward(x)
        assert got.shape == (N, 2 * N) and got.dtype == NP[dtype]
        ref = (TM._cosm(N, dt) * w.astype(dt))[:, ::-1]  # frame f holds the impulse at n = 2N - 1 - f
        wn = np.abs(w[::-1])[None, :]
        _entries(got, ref, tol * wn, name, lambda k, f: (int(k), 2 * N - 1 - int(f)))
        zero = np.broadcast_to(wn == 0, got.shape)
        assert (got[zero] == 0).all()
        return w
    hop, nf, pos, _, n, valid = sampled_forward_positions(N)
    plan = sg.MdctPlan(sg.MdctParams(ws, hop, win), dtype)
    assert plan.kernel_name() == "k_mdct_fwd"
    w = window_t(plan, dtype)
    x = np.zeros((len(pos), ws + (nf - 1) * hop), NP[dtype])
    x[np.arange(len(pos)), pos] = 1
    got = plan.forward(x)
    assert got.shape == (len(pos), N, nf)
    rr, ff = np.nonzero(valid)
    ref = np.zeros(got.shape, dt)
    ref[rr, :, ff] = (cos_sub(N, np.arange(N), n[rr, ff], dt) * w[n[rr, ff]].astype(dt)).T
    bnd = np.zeros((len(pos), 1, nf))
    bnd[rr, 0, ff] = tol * np.abs(w[n[rr, ff]])
    _entries(got, ref, bnd, name, lambda r, k, f: (int(k), int(n[r, f])))  # a frame without the impulse: exact zeros
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws", WINDOWS)
def test_forward_readback(ws, dtype):
    _forward_readback(ws, dtype, _sine(ws), "sine")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws", [512, 960, 4096])
def test_forward_readback_hann(ws, dtype):
    w = _forward_readback(ws, dtype, sg.WindowType.hanning, "hann")
    assert w[0] == 0 and (w[1:ws // 2] > 0).all()  # (the zero columns were compared with == 0 above)


# ---- 2. inverse read-back --------------------------------------------------------------------------------------------------------
def one_hot_ks(N):
    """The unit's k per frame: all of 0 .. N - 1 for N <= 2048, else 512 distinct k, the ends and the middle among them, shuffled."""
    if N <= 2048:
        return np.arange(N)
    rng = np.random.default_rng(N)
    special = [0, 1, N // 2 - 1, N // 2, N - 2, N - 1]
    rest = [k for k in rng.permutation(N).tolist() if k not in special][:512 - len(special)]
    return rng.permutation(np.array(special + rest))


def inverse_expected(N, hop, ks, w, dt, mult, u):
    """(ref, bound) of the overlap-added inverse of one-hot frames, frame f a unit at k = ks[f]; additions in ascending frame order."""
    nf, two_n = len(ks), 2 * N
    cosr = TM._cosm(N, dt) if np.array_equal(ks, np.arange(N)) else cos_sub(N, ks, np.arange(two_n), dt)
    terms = cosr * (dt(2.0) / dt(N)) * w.astype(dt)  # [nf, 2N]
    chain = CB * u * mult * (2.0 / N) * np.abs(w)
    n_out = hop * nf + two_n - hop
    ref, bnd, seen = np.zeros(n_out, dt), np.zeros(n_out), np.zeros(n_out, bool)
    for f in range(nf):
        s = slice(f * hop, f * hop + two_n)
        ref[s] += terms[f]
        bnd[s] += chain + np.where(seen[s], u * np.abs(ref[s]).astype(np.float64), 0.0)
        seen[s] = True
    return ref, bnd


def _inverse_readback(ws, hop, dtype, route, mult, label):
    N, dt = ws // 2, ref_dt(dtype)
    plan = sg.MdctPlan(sg.MdctParams(ws, hop, _sine(ws)), dtype)
    assert plan.kernel_name(True) == route, (ws, hop, dtype)
    w = window_t(plan, dtype)
    ks = one_hot_ks(N)
    c = np.zeros((N, len(ks)), NP[dtype])
    c[ks, np.arange(len(ks))] = 1
    got = plan.inverse(c)
    ref, bnd = inverse_expected(N, hop, ks, w, dt, mult, U[dtype])
    assert got.shape == ref.shape and got.dtype == NP[dtype]
    _entries(got, ref, bnd, f"readback inverse {label} {dtype}", lambda p: (int(p), "frames", int(max(0, (p - ws) // hop + 1)), int(p // hop)))


_INV_AT_HOP_N = [(ws, dt) for dt in DTYPES for ws in WINDOWS]


@pytest.mark.gpu
@pytest.mark.parametrize("ws,dtype", [c for c in _INV_AT_HOP_N if instance(*c)[3]], ids=lambda v: str(v))
def test_inverse_readback_fused(ws, dtype):
    split_, _, tile, _ = instance(ws, dtype)
    # ceil((n_frames + 1) / nbk) tiles, the halo frame of each recomputed
    assert -(-(len(one_hot_ks(ws // 2)) + 1) // (tile - 1)) >= 2
    _inverse_readback(ws, ws // 2, dtype, "k_imdct_ola", math.log2(ws), f"fused {split_}")


@pytest.mark.gpu
@pytest.mark.parametrize("ws,dtype", [c for c in _INV_AT_HOP_N if not instance(*c)[3]], ids=lambda v: str(v))
def test_inverse_readback_hop_n_not_fused(ws, dtype):
    """The lengths whose tile is below 4 frames: the route they do take at hop == N (launch_c2c_reg on M, the same stage count)."""
    _inverse_readback(ws, ws // 2, dtype, "imdct_generic", math.log2(ws), f"generic at hop N {instance(ws, dtype)[0]}")


def chirpz_length(L):
    """bluestein_host_tables: the convolution length is the smallest power of two >= 2 L - 1, L the transform length."""
    P = 1
    while P < 2 * L - 1:
        P *= 2
    return P


# (window, hop, multiplier of the bound): 256 and 960 run launch_c2c_reg on M = 64 / 240 (the stages of the fused kernels); 1000 is a
# chirp-z of L = M = 250 in P = 512; 18 sums its L = N = 9 points directly; 8190 is a chirp-z of L = N = 4095 in P = 8192
GENERIC_INV = [(256, 64, math.log2(256)), (960, 301, math.log2(960)),
               (1000, 500, math.log2(1000) + 2 * math.log2(chirpz_length(250))), (18, 9, math.log2(18)),
               (8190, 4095, math.log2(8190) + 2 * math.log2(chirpz_length(4095)))]


def test_chirpz_lengths():
    assert chirpz_length(250) == 512 and chirpz_length(4095) == 8192 and chirpz_length(4096) == 8192 and chirpz_length(4097) == 16384


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws,hop,mult", GENERIC_INV, ids=[f"{g[0]}-hop{g[1]}" for g in GENERIC_INV])
def test_inverse_readback_generic(ws, hop, mult, dtype):
    _inverse_readback(ws, hop, dtype, "imdct_generic", mult, f"generic {ws}/{hop}")


# ---- 3. dense parity and frame isolation -----------------------------------------------------------------------------------------
def forward_counts(tile):
    return sorted({n for n in (tile - 1, tile, tile + 1, 2 * tile + 1) if n > 0})


def inverse_counts(tile, fused):
    nbk = tile - 1
    return sorted({n for n in (nbk - 1, nbk, nbk + 1, 2 * nbk, 2 * nbk + 1) if n > 0}) if fused else [1, 2, 3, 5]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws", WINDOWS)
def test_dense_forward(ws, dtype):
    split_, _, tile, _ = instance(ws, dtype)
    rng = np.random.default_rng(ws)
    plan = sg.MdctPlan(sg.MdctParams.sine_window(ws), dtype)
    assert plan.kernel_name() == "k_mdct_fwd"
    for nf in forward_counts(tile):
        TM._check_forward(plan, TM._signal(rng, 3, ws + (nf - 1) * (ws // 2), dtype), dtype, f"dense {split_}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws", WINDOWS)
def test_dense_inverse(ws, dtype):
    split_, _, tile, fused = instance(ws, dtype)
    rng = np.random.default_rng(ws + 1)
    plan = sg.MdctPlan(sg.MdctParams.sine_window(ws), dtype)
    assert plan.kernel_name(True) == ("k_imdct_ola" if fused else "imdct_generic")
    for nf in inverse_counts(tile, fused):
        TM._check_inverse(plan, rng.standard_normal((3, ws // 2, nf)).astype(NP[dtype]), dtype, f"dense {split_}")


EXPS = (0, 20, -20, 7)


def _no_underflow(one, dtype):
    nz = np.abs(one[one != 0])
    assert nz.size and 2.0 ** -20 * float(nz.min()) >= float(np.finfo(NP[dtype]).tiny)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws", WINDOWS)
def test_forward_frame_isolation(ws, dtype):
    """Disjoint frames (hop = 2N), frame f = base * 2^e_f: column f == 2^e_f times the one-frame result, exactly."""
    tile = instance(ws, dtype)[2]
    nf = 2 * tile + 1
    base = np.random.default_rng(ws).uniform(0.5, 2.0, ws).astype(NP[dtype])
    plan = sg.MdctPlan(sg.MdctParams(ws, ws, _sine(ws)), dtype)
    assert plan.kernel_name() == "k_mdct_fwd"
    one = plan.forward(base)[:, 0]
    _no_underflow(one, dtype)
    e = np.array([EXPS[f % 4] for f in range(nf)])
    got = plan.forward(np.concatenate([np.ldexp(base, k) for k in e]))
    exp = np.ldexp(one[:, None], e[None, :])
    assert got.shape == exp.shape and got.dtype == exp.dtype
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (len(bad), bad[:6].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws", WINDOWS)
def test_inverse_frame_isolation(ws, dtype):
    """hop = N, even frames base * 2^e, odd frames zero: blocks 2j and 2j + 1 == 2^e times the halves of the one-frame inverse."""
    N = ws // 2
    _, _, tile, fused = instance(ws, dtype)
    nf = 2 * (tile - 1) + 1 if fused else 5
    base = np.random.default_rng(ws + 2).uniform(0.5, 2.0, N).astype(NP[dtype])
    plan = sg.MdctPlan(sg.MdctParams(ws, N, _sine(ws)), dtype)
    assert plan.kernel_name(True) == ("k_imdct_ola" if fused else "imdct_generic")
    one = plan.inverse(base[:, None])
    assert one.shape == (ws,)
    _no_underflow(one, dtype)
    c = np.zeros((N, nf), NP[dtype])
    exp = np.zeros((nf + 1) * N, NP[dtype])
    for j in range((nf + 1) // 2):
        c[:, 2 * j] = np.ldexp(base, EXPS[j % 4])
        exp[2 * j * N:(2 * j + 2) * N] = np.ldexp(one, EXPS[j % 4])
    got = plan.inverse(c)
    assert got.shape == exp.shape and got.dtype == exp.dtype
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (len(bad), [(int(p // N), int(p % N)) for p in bad[:6]])


# ---- 4. the generic route across a chunk seam ------------------------------------------------------------------------------------
SEAM_WS, SEAM_HOP = 8190, 3
CHUNK_BYTES = 256 << 20  # kChunkBytes


def seam_frames_per_chunk():
    """gen_sizes for window 8190 in f64: N = 4095 is odd, so a frame is two sequences of L = N complex f64 (131040 B; the inverse's
    windowed frame, 2N f64, is smaller), and a chunk is floor(256 MiB / 131040) frames, forward and inverse alike."""
    N = SEAM_WS // 2
    per_seq, per_frame = 2 * N * 2 * 8, SEAM_WS * 8
    return CHUNK_BYTES // max(per_seq, per_frame)


def test_seam_arithmetic():
    assert seam_frames_per_chunk() == 2048
    assert 3 * 700 > 2048 and divmod(2048, 700) == (2, 648) and 4 * 1024 == 2 * 2048


@pytest.mark.gpu
@pytest.mark.parametrize("rows,nf", [(3, 700), (4, 1024)], ids=["seam-in-row", "seam-on-row-boundary"])
def test_generic_chunk_seam(rows, nf):
    dtype, ws, hop, N = "float64", SEAM_WS, SEAM_HOP, SEAM_WS // 2
    gc = seam_frames_per_chunk()
    assert rows * nf > gc and nf <= gc  # the batch needs more than one chunk, a row alone does not
    seams = list(range(gc, rows * nf, gc))
    rng = np.random.default_rng(rows)
    plan = sg.MdctPlan(sg.MdctParams(ws, hop, sg.WindowType.hanning), dtype)
    assert plan.kernel_name() == "mdct_generic" and plan.kernel_name(True) == "imdct_generic"
    w = plan.window()
    x = TM._signal(rng, rows, ws + (nf - 1) * hop, dtype)
    got = plan.forward(x)
    assert got.shape == (rows, N, nf)
    for r in range(rows):
        np.testing.assert_array_equal(got[r], plan.forward(x[r]), err_msg=f"forward row {r}")
    near = sorted({0, rows * nf - 1} | {g for s in seams for g in range(s - 16, s + 16)})
    for g in near:
        r, f = divmod(g, nf)
        xs = x[r:r + 1, f * hop:f * hop + ws]
        ref = TM.fft_forward(TM.frames_of(xs.astype(np.float64), ws, hop) * w, N)[0, :, 0]
        assert np.abs(got[r, :, f] - ref).max() <= TM.fwd_bound(xs, w, ws, hop, dtype)[0, 0], (r, f)
    del got
    c = rng.standard_normal((rows, N, nf))
    y = plan.inverse(c)
    for r in range(rows):
        np.testing.assert_array_equal(y[r], plan.inverse(c[r]), err_msg=f"inverse row {r}")
    bound = TM.inv_bound(c, w, ws, hop, dtype)
    for r in range(rows):  # whole rows: every sample a seam frame reaches, and the first and last frame
        ref = np.zeros(y.shape[1])
        for f0 in range(0, nf, 256):
            part = TM.ola(TM.fft_frames_inv(c[r:r + 1, :, f0:f0 + 256], N), w, hop)[0]
            ref[f0 * hop:f0 * hop + part.size] += part
        ratio = np.abs(y[r] - ref).max() / bound
        TM._record(f"inverse seam {rows}x{nf} {dtype}", ratio)
        assert ratio <= 1.0, (r, ratio)
