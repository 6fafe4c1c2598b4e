"""The reference of tests/test_iir.py and tests/test_iir_readback.py: the cascade of second-order sections of include/spectro_hip_iir.h
in numpy, once in np.longdouble (`ref`) and once in f64 (`seq`, operation for operation what scipy.signal.sosfilt and the kernel's
work items do), the two-pass zero-phase form built on them, sosfilt_zi, the test filters and the bound.

Bound.  For a row, E = max(max |seq - ref|, 2^-53 max |ref|): how far the plain sequential f64 recurrence sits from the long-double
evaluation, and never less than half an ulp of the row's largest value.  An f64 output y must satisfy max |y - ref| <= 8 E: the factor
is a margin over the reference's own scatter, not a measurement of the kernel (the blocked form with one matrix product between blocks
came out at 0.4 .. 2.2 E on the CPU; the log-step scan stacks up to eight).  An f32 output must lie within one f32 ulp of ref, element
by element.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2.0 ** -60, "np.longdouble is no wider than f64 here: the reference would be the thing under test"

BOUND_FACTOR = 8.0


def cascade(sos, x, zi=None, dtype=np.float64, lengths=None, trajectory=False):
    """(y, zf) through the sections in order, Direct Form II transposed, every value of `dtype`.  `x` is one row (n,) or rows (R, n)
    run side by side (the loop over samples is Python's); `sos` is (S, 6) or (R, S, 6), `zi` (S, 2) or (R, S, 2).  With `lengths` (R,)
    row r ends after lengths[r] samples: zf[r] is its state there (what lies behind in y is to be ignored).  With `trajectory` a third
    result holds the state after every sample, (R, n, S, 2) (or (n, S, 2) for one row)."""
    x = np.asarray(x)
    one = x.ndim == 1
    x2 = np.atleast_2d(x).astype(dtype)
    R, n = x2.shape
    c = np.asarray(sos, dtype=np.float64).astype(dtype)
    S = c.shape[-2]
    co = [[c[..., i, k] for k in (0, 1, 2, 4, 5)] for i in range(S)]
    z = np.zeros((R, S, 2), dtype)
    if zi is not None:
        z[:] = np.asarray(zi).astype(dtype)
    z0, z1 = [z[:, i, 0].copy() for i in range(S)], [z[:, i, 1].copy() for i in range(S)]
    ends = {}
    if lengths is not None:
        for r, m in enumerate(lengths):
            ends.setdefault(int(m), []).append(r)
    zf = np.zeros((R, S, 2), dtype)
    y = np.empty((R, n), dtype)
    zt = np.empty((R, n, S, 2), dtype) if trajectory else None
    for t in range(n):
        v = x2[:, t]
        for i in range(S):
            b0, b1, b2, a1, a2 = co[i]
            w = b0 * v + z0[i]
            z0[i] = b1 * v - a1 * w + z1[i]
            z1[i] = b2 * v - a2 * w
            v = w
            if trajectory:
                zt[:, t, i, 0], zt[:, t, i, 1] = z0[i], z1[i]
        y[:, t] = v
        if t + 1 in ends:
            for i in range(S):
                zf[ends[t + 1], i, 0], zf[ends[t + 1], i, 1] = z0[i][ends[t + 1]], z1[i][ends[t + 1]]
    if lengths is None:
        for i in range(S):
            zf[:, i, 0], zf[:, i, 1] = z0[i], z1[i]
    if trajectory:
        return (y[0], zf[0], zt[0]) if one else (y, zf, zt)
    return (y[0], zf[0]) if one else (y, zf)


def ref(sos, x, zi=None, lengths=None, trajectory=False):
    return cascade(sos, x, zi, LD, lengths, trajectory)


def seq(sos, x, zi=None, lengths=None, trajectory=False):
    return cascade(sos, x, zi, np.float64, lengths, trajectory)


def state_ratio(zf, zt_seq, zt_ref):
    """A final state (S, 2) against the reference's, by the row's rule applied to the states: per section, E = max over the row of
    |state_seq - state_ref|, and never less than 2^-53 of the largest value the section's state takes in the row (one instant's
    state can be small where its terms cancel; its error is that of the terms); zf passes at max |zf - state_ref[-1]| <= 8 E."""
    zs, zr = np.asarray(zt_seq, LD), np.asarray(zt_ref, LD)
    worst = 0.0
    for i in range(zr.shape[1]):
        e = float(max(np.max(np.abs(zs[:, i] - zr[:, i])), 2.0 ** -53 * np.max(np.abs(zr[:, i]))))
        d = float(np.max(np.abs(np.asarray(zf, LD)[i] - zr[-1, i])))
        worst = max(worst, d / (BOUND_FACTOR * e) if e > 0 else (0.0 if d == 0 else np.inf))
    return worst


def sosfilt_zi(sos, dtype=LD):
    """scipy.signal.sosfilt_zi: per section the solution of (I - A^T) zi = B, scaled by the gain at DC of the sections before it."""
    sos = np.asarray(sos, dtype=np.float64).astype(dtype)
    zi = np.empty((sos.shape[0], 2), dtype)
    scale = dtype(1.0)
    for i, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        det = 1 + a1 + a2
        B0, B1 = b1 - a1 * b0, b2 - a2 * b0
        z0 = (B0 + B1) / det
        zi[i] = scale * z0, scale * (B1 - a2 * z0)
        scale = scale * ((b0 + b1 + b2) / det)
    return zi


def default_padlen(sos):
    sos = np.asarray(sos, dtype=np.float64)
    return 3 * (2 * sos.shape[0] + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum())))


def odd_ext(x, pad):
    if pad == 0:
        return x
    return np.concatenate([2 * x[0] - x[pad:0:-1], x, 2 * x[-1] - x[-2:-(pad + 2):-1]])


def filtfilt(sos, x, padlen=None, dtype=np.float64):
    """scipy.signal.sosfiltfilt(sos, x, padtype="odd", padlen=padlen) of one row, every value of `dtype`."""
    return filtfilt_rows(sos, [x], padlen, dtype)[0]


def filtfilt_rows(sos, rows, padlen=None, dtype=np.float64):
    """`filtfilt` of rows of different lengths, run side by side: a list of results."""
    pad = default_padlen(sos) if padlen is None else padlen
    ext = [odd_ext(np.asarray(x).astype(dtype), pad) for x in rows]
    assert all(np.shape(x)[0] > pad for x in rows)
    lens = [e.shape[0] for e in ext]
    zi = sosfilt_zi(sos, LD).astype(dtype)

    def run(seqs):
        X = np.zeros((len(seqs), max(lens)), dtype)
        for r, e in enumerate(seqs):
            X[r, :lens[r]] = e
        y, _ = cascade(sos, X, zi[None] * X[:, :1, None], dtype)
        return [y[r, :lens[r]] for r in range(len(seqs))]

    fwd = run(ext)
    bwd = [y[::-1] for y in run([y[::-1] for y in fwd])]
    return [y[pad:y.shape[0] - pad] if pad else y for y in bwd]


def bound(s, r):
    """E of a row (or of a state) from its `seq` and `ref` values."""
    s, r = np.asarray(s, LD), np.asarray(r, LD)
    return float(max(np.max(np.abs(s - r)), 2.0 ** -53 * np.max(np.abs(r))))


def ratio64(y, s, r):
    """max |y - ref| / (8 E): an f64 output passes at <= 1."""
    e = bound(s, r)
    d = float(np.max(np.abs(np.asarray(y, LD) - np.asarray(r, LD))))
    return d / (BOUND_FACTOR * e) if e > 0 else (0.0 if d == 0 else np.inf)


def check32(y, r):
    """(worst |y - f32(ref)| in ulps of ref, share of elements that differ from f32(ref) at all); passes at <= 1 ulp."""
    r = np.asarray(r, LD)
    r32 = r.astype(np.float32)
    ulp = np.spacing(np.abs(r32)).astype(LD)
    worst = float(np.max(np.abs(np.asarray(y, np.float32).astype(LD) - r32.astype(LD)) / ulp))
    return worst, float(np.mean(np.asarray(y, np.float32) != r32))


# ---- the test filters -------------------------------------------------------------------------------------------------------------
# The designs are scipy.signal's (output="sos"), kept as numbers so that no GPU test needs scipy: butter(8, 0.01), butter(4, 0.001,
# "highpass"), ellip(3, 1, 40, [0.2, 0.3], "bandpass"), butter(16, 0.3).
BUTTER8_LP = np.array([
    [3.4219614165936484e-15, 6.843922833187297e-15, 3.4219614165936484e-15, 1.0, -1.939269633591658, 0.9402270185020654],
    [1.0, 2.0, 1.0, 1.0, -1.9481335385151675, 0.9490952993868512],
    [1.0, 2.0, 1.0, 1.0, -1.9647269019487286, 0.9656968546857874],
    [1.0, 2.0, 1.0, 1.0, -1.9868379069766875, 0.987818775546285],
])
BUTTER4_HP = np.array([
    [0.9959037221384247, -1.9918074442768494, 0.9959037221384247, 1.0, -1.9942020618642575, 0.9942119028974503],
    [1.0, -2.0, 1.0, 1.0, -1.997588562550215, 0.9975984202951876],
])
ELLIP6_BP = np.array([
    [0.010984809455851343, 0.0, -0.010984809455851343, 1.0, -1.3221689714525553, 0.846808589798882],
    [1.0, -0.5980651817738911, 1.0, 1.0, -1.1358641759478654, 0.9219661441839279],
    [1.0, -1.8066479532856774, 1.0000000000000002, 1.0, -1.5680529172134967, 0.9423103160469926],
])
BUTTER16_LP = np.array([
    [1.310504512325866e-07, 2.621009024651732e-07, 1.310504512325866e-07, 1.0, -0.6512418128586466, 0.1079587490817111],
    [1.0, 2.0, 1.0, 1.0, -0.662598972946529, 0.1272807039003924],
    [1.0, 2.0, 1.0, 1.0, -0.6860681949181047, 0.1672089291834213],
    [1.0, 2.0, 1.0, 1.0, -0.7232594973342533, 0.2304825521113455],
    [1.0, 2.0, 1.0, 1.0, -0.776859208898273, 0.32167182805008426],
    [1.0, 2.0, 1.0, 1.0, -0.8510190833340232, 0.4478401423221979],
    [1.0, 2.0, 1.0, 1.0, -0.9519982498701609, 0.6196361616035594],
    [1.0, 2.0, 1.0, 1.0, -1.089199659445263, 0.8530571415277588],
])
_R, _TH = 0.9999, 0.1 * np.pi
FILTERS = {
    "butter8_lp_0.01": BUTTER8_LP,
    "butter4_hp_0.001": BUTTER4_HP,
    "ellip6_bp": ELLIP6_BP,
    "resonator_0.9999": np.array([[1.0 - _R, 0.0, 0.0, 1.0, -2.0 * _R * np.cos(_TH), _R * _R]]),
    "dc_blocker": np.array([[1.0, -1.0, 0.0, 1.0, -0.995, 0.0]]),
    "butter16_lp_0.3": BUTTER16_LP,
    "integrator": np.array([[1.0, 0.0, 0.0, 1.0, -1.0, 0.0]]),
    "fir_only": np.array([[0.25, 0.5, 0.25, 1.0, 0.0, 0.0]]),
}


def signals(batch, n, np_dtype, seed):
    """Gaussian rows drawn in the plan's type (and widened by the caller)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((batch, n)).astype(np_dtype)
