"""IIR filtering plans (sgx_iir_*, spectrograms_amd/iir.py) against tests/iir_ref.py.

The reference is the recurrence of include/spectro_hip_iir.h in numpy, in np.longdouble (`ref`) and in f64 (`seq`).  For a row,
E = max(max |seq - ref|, 2^-53 max |ref|); an f64 output must satisfy max |y - ref| <= 8 E, an f32 output |y - f32(ref)| <= one f32
ulp of ref per element (tests/iir_ref.py says where the factor comes from).  Inputs are drawn in the plan's type and widened.  Every
case prints its worst ratio to the bound; profiles/time_iir.txt keeps the table of an MI355X run.

CPU: the family's ctypes table against include/spectro_hip_iir.h (the parser rules of tests/test_abi.py), the header as C99, the
rejections, sosfilt_zi / padlen / the coefficient helpers against their formulas, `seq` against scipy where scipy imports, and the
census: every (T, S, direction) the X-macro compiles has a GPU case.

GPU: every instance in both types and directions at the lengths 1, 2, L - 1, L, L + 1, tile - 1, tile, tile + 1, 2 tiles + 37; the
eight filters with entry and exit states; streaming pushes; per-row banks; batch independence; the split and chain routes; filtfilt;
a NaN inside a row; the stream contract on every route.  The impulse read-back and the transition tables are in
tests/test_iir_readback.py.
"""
import ctypes as C
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests import iir_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spectro_hip_iir.h")
HOST = _ffi.DEVICE_HOST_ONLY
F32, F64 = "float32", "float64"
DTYPES = (F32, F64)
NP = {F32: np.float32, F64: np.float64}
L, TILE, SEG = 16, 4096, 8 * 4096  # asserted against the plan where they are used
# The backward cases run filtfilt with padlen 0 down to one sample, where the steady-state entry state cancels a high- or band-pass
# filter's output to the rounding of its terms; an element that is nothing but cancelled rounding has no f32 ulp to be held to (the
# f64 recurrence itself is not within it), so the instance cases take low-pass sections (and the DC blocker, whose entry state cancels
# exactly).  The high-pass and the band-pass run in the filter, impulse, NaN, batch and stream cases.
INSTANCE_FILTER = {1: "dc_blocker", 2: "butter16_lp_0.3", 4: "butter8_lp_0.01", 8: "butter16_lp_0.3"}
WORST = {}  # case -> worst ratio to the bound (f64) or worst distance in f32 ulps, printed per case


def lengths(plan):
    l, t = plan.block, plan.tile
    assert (l, t) == (L, TILE)
    return [1, 2, l - 1, l, l + 1, t - 1, t, t + 1, 2 * t + 37]


def sos_of(S):
    """The filter an instance's cases run: the first `S` sections of a design."""
    return R.FILTERS[INSTANCE_FILTER[S]][:S]


def check(case, y, s, r, dtype):
    """One row (or state) `y` against its `seq` and `ref` values; records and returns the case's figure."""
    if dtype == F64:
        fig = R.ratio64(y, s, r)
        share = None
    else:
        fig, share = R.check32(y, r)
    WORST[case] = max(WORST.get(case, 0.0), fig)
    assert fig <= 1.0, (case, fig, share)
    return fig, share


def check_state(case, zf, zt_seq, zt_ref):
    """A final state against the reference's state trajectories (tests/iir_ref.py `state_ratio`): the bound scaled by the state's size."""
    fig = R.state_ratio(zf, zt_seq, zt_ref)
    WORST[case] = max(WORST.get(case, 0.0), fig)
    assert fig <= 1.0, (case, fig)


def report(case, shares=()):
    unit = "f32 ulp" if "float32" in case and not case.endswith(("-zf", "-state")) else "of 8 E"
    extra = f", {100.0 * max(shares):.2f} % of the elements differ from f32(ref)" if shares else ""
    print(f"\n{case}: worst {WORST.get(case, 0.0):.3f} {unit}{extra}")


# ---- CPU: the ABI ------------------------------------------------------------------------------------------------------------------------
_C_SCALARS = {"size_t": C.c_size_t, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "double": C.c_double,
              "float": C.c_float}
_C_RETURNS = {"sgx_status": C.c_int, "void": None, "const char *": C.c_char_p, "size_t": C.c_size_t, "int32_t": C.c_int32,
              "double": C.c_double}


def header_declarations():
    """{name: (return type, [parameter types])} of every function the header declares (tests/test_abi.py `_header_declarations`)."""
    hdr = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^(sgx_status|void|size_t|int32_t|double|const char \*)\s*(sgx_\w+)\s*\(([^;{}()]*)\)\s*;", hdr, re.M):
        types = []
        for prm in (q.strip() for q in params.split(",")):
            if prm == "void" and "," not in params:
                continue
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s+(\**)\s*(?:const\s+)?\w+", prm)
            assert m, (name, prm)
            types.append("*" if m.group(2) else m.group(1))
        assert name not in out, name
        out[name] = (ret, types)
    return out


def test_second_signature_table_matches_the_iir_header():
    decl = header_declarations()
    assert set(decl) == set(_ffi.IIR_SIGNATURES), set(decl) ^ set(_ffi.IIR_SIGNATURES)
    assert not set(_ffi.IIR_SIGNATURES) & set(_ffi.SIGNATURES)
    L_ = _ffi.lib()
    for name, (ret, types) in decl.items():
        restype, argtypes = _ffi.IIR_SIGNATURES[name]
        assert restype is _C_RETURNS[ret], (name, ret, restype)
        assert len(argtypes) == len(types), (name, types, argtypes)
        for i, (ctype, arg) in enumerate(zip(types, argtypes)):
            if ctype == "*":
                assert arg in (C.c_void_p, C.c_char_p) or issubclass(arg, C._Pointer), (name, i, arg)
            else:
                assert arg is _C_SCALARS[ctype], (name, i, ctype, arg)
        f = getattr(L_, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    # every call that enqueues work takes `void *stream` last
    hdr = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name in ("filter", "process", "filtfilt", "reset", "state", "set_state"):
        assert re.search(r"sgx_iir_%s\s*\([^;]*void \*stream\)\s*;" % name, hdr), name
    # the main header stays as it was: it neither includes this one nor declares the family, and the version is 7
    main = open(os.path.join(ROOT, "include", "spectro_hip.h")).read()
    assert "sgx_iir" not in main and "spectro_hip_iir.h" not in main and _ffi.lib().sgx_abi_version() == 7
    assert '#include "spectro_hip.h"' in open(HEADER).read()


def test_header_compiles_as_c99():
    src = '#include "spectro_hip_iir.h"\nint main(void) { sgx_iir *p = 0; return sgx_iir_n_sections(p) == 0 && SGX_IIR_ROUTE_CHAIN == 2 ? 0 : 1; }\n'
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    cmd = [cc] if cc else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-D__HIP_PLATFORM_AMD__"]
    r = subprocess.run(cmd + ["-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-"],
                       input=src, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_exports():
    for name in ("IirPlan", "sosfilt", "sosfiltfilt", "sosfilt_zi", "biquad", "lowpass_biquad", "highpass_biquad", "bandpass_biquad",
                 "bandreject_biquad", "allpass_biquad", "equalizer_biquad", "preemphasis_sos", "deemphasis_sos"):
        assert hasattr(sg, name) and name in sg.__all__


# ---- CPU: rejections ---------------------------------------------------------------------------------------------------------------------
def test_create_rejections_name_the_section():
    ok = [1.0, 0.0, 0.0, 1.0, -0.5, 0.0]
    with pytest.raises(sg.InvalidInputError, match="section 1 has a pole outside the unit circle"):
        sg.IirPlan([ok, [1.0, 0.0, 0.0, 1.0, 0.0, 1.0000001]], device=HOST)
    with pytest.raises(sg.InvalidInputError, match="section 0 has a pole outside the unit circle"):
        sg.IirPlan([[1.0, 0.0, 0.0, 1.0, -2.0000001, 1.0]], device=HOST)
    with pytest.raises(sg.InvalidInputError, match="section 2 of filter 1 has a pole outside"):
        sg.IirPlan([[ok, ok, ok], [ok, ok, [1.0, 0.0, 0.0, 1.0, 1.6, 0.5]]], device=HOST)
    # on the circle: allowed (an integrator, a double integrator, an undamped resonator)
    for a1, a2 in ((-1.0, 0.0), (-2.0, 1.0), (2.0, 1.0), (-2.0 * math.cos(0.3), 1.0), (0.0, -1.0)):
        sg.IirPlan([[1.0, 0.0, 0.0, 1.0, a1, a2]], device=HOST)
    with pytest.raises(sg.InvalidInputError, match="section 0 has a0 = 2"):
        sg.IirPlan([[1.0, 0.0, 0.0, 2.0, -0.5, 0.0]], device=HOST)
    for bad in (float("nan"), float("inf")):
        for k in (0, 4):
            s = list(ok)
            s[k] = bad
            with pytest.raises(sg.InvalidInputError, match="section 1 has a non-finite coefficient"):
                sg.IirPlan([ok, s], device=HOST)
    with pytest.raises(sg.InvalidInputError, match="at least one section"):
        sg.IirPlan(np.zeros((0, 6)), device=HOST)
    # the raw ABI likewise, without aborting
    lib, h = _ffi.lib(), C.c_void_p()
    assert lib.sgx_iir_create(None, 0, 1, 0, _ffi.F64, HOST, C.byref(h)) == _ffi.SGX_INVALID_INPUT and not h.value
    assert b"at least one section" in lib.sgx_iir_last_error(None)
    one = (C.c_double * 6)(*ok)
    assert lib.sgx_iir_create(one, 1, 1, 7, _ffi.F64, HOST, C.byref(h)) == _ffi.SGX_INVALID_INPUT
    assert lib.sgx_iir_create(one, 1, 1, 0, 5, HOST, C.byref(h)) == _ffi.SGX_INVALID_INPUT


def test_python_shape_dtype_and_route_errors():
    with pytest.raises(ValueError, match="sos must be"):
        sg.IirPlan([1.0, 0.0, 0.0, 1.0, 0.0, 0.0], device=HOST)
    with pytest.raises(ValueError, match="sos must be"):
        sg.IirPlan(np.zeros((2, 5)), device=HOST)
    with pytest.raises(ValueError, match="route must be"):
        sg.IirPlan(R.FILTERS["dc_blocker"], device=HOST, route="generic")
    with pytest.raises(ValueError):
        sg.IirPlan(R.FILTERS["dc_blocker"], dtype="float16", device=HOST)
    with pytest.raises(sg.InvalidInputError, match="split route takes up to 8"):
        sg.IirPlan(np.tile(R.FILTERS["dc_blocker"], (9, 1)), device=HOST, route="split")
    p = sg.IirPlan(R.FILTERS["butter8_lp_0.01"], device=HOST)
    with pytest.raises(ValueError, match="samples must be 1-D"):
        p.filter(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="batch must be > 0"):
        p.filter(np.zeros((0, 8)))
    with pytest.raises(sg.DimensionMismatchError):
        p.filter(np.zeros((2, 8)), zi=np.zeros((2, 3, 2)))
    with pytest.raises(ValueError, match="state must be"):
        p.set_state(np.zeros((2, 3, 2)))
    with pytest.raises(ValueError, match="padlen"):
        p.filtfilt(np.zeros(100), padlen=-1)
    # n <= padlen, as scipy; checked before the device is
    assert p.padlen == 27
    with pytest.raises(sg.InvalidInputError, match=r"length of the input \(27\) must be greater than padlen \(27\)"):
        p.filtfilt(np.zeros(27))
    with pytest.raises(sg.InvalidInputError, match=r"greater than padlen \(40\)"):
        p.filtfilt(np.zeros(40), padlen=40)
    with pytest.raises(sg.InvalidInputError, match="samples must be non-empty"):
        p.filter(np.zeros(0))
    # a host-only plan refuses compute loudly
    with pytest.raises(sg.FFTBackendError, match="no HIP device"):
        p.filter(np.zeros(8))
    with pytest.raises(sg.FFTBackendError, match="no HIP device"):
        p.filtfilt(np.zeros(100))
    with pytest.raises(sg.FFTBackendError, match="no HIP device"):
        p.process(np.zeros(8))
    bank = sg.IirPlan(np.stack([R.FILTERS["dc_blocker"], R.FILTERS["integrator"]]), device=HOST)
    with pytest.raises(sg.DimensionMismatchError, match="one filter per row"):
        bank.filter(np.zeros((3, 8)))
    with pytest.raises(sg.InvalidInputError, match="section 0 has a pole at z = 1"):
        bank.zi()
    with pytest.raises(sg.InvalidInputError, match="pole at z = 1"):
        bank.filtfilt(np.zeros((2, 100)))
    with pytest.raises(sg.InvalidInputError, match="a0 must not be 0"):
        sg.biquad(np.zeros(4), 1, 0, 0, 0, 0, 0)


# ---- CPU: formulas -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in R.FILTERS if k != "integrator"])
def test_sosfilt_zi_and_padlen_against_their_formulas(name):
    sos = R.FILTERS[name]
    plan = sg.IirPlan(sos, device=HOST)
    assert plan.n_sections == len(sos) and plan.padlen == R.default_padlen(sos)
    zi, want = sg.sosfilt_zi(sos), R.sosfilt_zi(sos)
    assert zi.shape == (len(sos), 2) and np.array_equal(zi, plan.zi())
    assert np.array_equal(zi, want.astype(np.float64))  # the same solve in long double, rounded once
    # the defining property: a constant input of 1 from state zi leaves the state where it is and gives the DC gain
    y, zf = R.ref(sos, np.ones(64), want)
    gain = np.prod(sos[:, :3].sum(1).astype(R.LD) / sos[:, 3:].sum(1).astype(R.LD))
    scale = max(1.0, float(np.max(np.abs(want))))
    assert float(np.max(np.abs(zf - want))) <= 64 * len(sos) * 2.0 ** -60 * scale / float(np.min(1 + sos[:, 4] + sos[:, 5]))
    assert float(np.max(np.abs(y - gain))) <= 64 * len(sos) * 2.0 ** -60 * scale / float(np.min(1 + sos[:, 4] + sos[:, 5]))


def test_padlen_counts_the_sections_without_b2_or_a2():
    assert sg.IirPlan([[1, 0, 0, 1, 0, 0]], device=HOST).padlen == 3 * (2 + 1 - 1)
    assert sg.IirPlan([[1, 0, 0, 1, -0.5, 0.25]], device=HOST).padlen == 9          # b2 == 0 only: min(1, 0)
    assert sg.IirPlan([[1, 0, 0, 1, 0, 0], [1, 1, 1, 1, 0, 0.5]], device=HOST).padlen == 12         # min(1, 1)
    assert sg.IirPlan([[1, 0, 0, 1, -0.5, 0.25], [1, 1, 0, 1, 0.2, 0.1]], device=HOST).padlen == 15  # min(2, 0)
    assert sg.IirPlan([[[1, 0, 0, 1, 0, 0]], [[1, 1, 1, 1, 0, 0.5]]], device=HOST).padlen == 9  # a bank: the largest over the filters
    assert sg.IirPlan(np.tile(R.FILTERS["dc_blocker"], (12, 1)), device=HOST).kernel_name == "iir_chain"
    assert sg.IirPlan(np.tile(R.FILTERS["dc_blocker"], (12, 1)), device=HOST).tile == 0
    p = sg.IirPlan(R.FILTERS["dc_blocker"], device=HOST)
    assert (p.kernel_name, p.tile, p.block, p.device, p.dtype) == ("k_iir_sos", TILE, L, HOST, F64)
    assert sg.IirPlan(R.FILTERS["dc_blocker"], device=HOST, route="split").kernel_name == "k_iir_sos+split"
    assert sg.IirPlan(R.FILTERS["dc_blocker"], device=HOST, route="chain", dtype=F32).kernel_name == "iir_chain"


def test_biquad_helpers_against_the_cookbook_formulas():
    sr, f, q, gain = 48000.0, 1234.5, 1.3, -4.5
    w0 = 2 * math.pi * f / sr
    c, s = math.cos(w0), math.sin(w0)
    al = s / (2 * q)
    A = 10.0 ** (gain / 40.0)
    want = {
        "lowpass": ((1 - c) / 2, 1 - c, (1 - c) / 2, 1 + al, -2 * c, 1 - al),
        "highpass": ((1 + c) / 2, -(1 + c), (1 + c) / 2, 1 + al, -2 * c, 1 - al),
        "bandpass": (al, 0.0, -al, 1 + al, -2 * c, 1 - al),
        "bandreject": (1.0, -2 * c, 1.0, 1 + al, -2 * c, 1 - al),
        "allpass": (1 - al, -2 * c, 1 + al, 1 + al, -2 * c, 1 - al),
    }
    for name, co in want.items():
        got = getattr(sg, name + "_biquad")(sr, f, q)
        assert got.shape == (6,) and got[3] == 1.0
        assert np.allclose(got, np.array(co) / co[3], rtol=4e-16, atol=0), name
    got = sg.bandpass_biquad(sr, f, q, const_skirt_gain=True)
    assert np.allclose(got, np.array([s / 2, 0.0, -s / 2, 1 + al, -2 * c, 1 - al]) / (1 + al), rtol=4e-16, atol=0)
    got = sg.equalizer_biquad(sr, f, gain, q)
    assert np.allclose(got, np.array([1 + al * A, -2 * c, 1 - al * A, 1 + al / A, -2 * c, 1 - al / A]) / (1 + al / A), rtol=1e-15, atol=0)
    assert np.array_equal(sg.preemphasis_sos(0.97), [1.0, -0.97, 0.0, 1.0, 0.0, 0.0])
    assert np.array_equal(sg.deemphasis_sos(0.97), [1.0, 0.0, 0.0, 1.0, -0.97, 0.0])
    # every helper's section passes the pole check, and pre- and de-emphasis undo each other
    for row in (sg.lowpass_biquad(sr, 20.0), sg.highpass_biquad(sr, 23990.0, 10.0), sg.equalizer_biquad(sr, f, 12.0)):
        sg.IirPlan(row[None], device=HOST)
    x = np.random.default_rng(0).standard_normal(200)
    y, _ = R.seq(np.stack([sg.preemphasis_sos(0.5), sg.deemphasis_sos(0.5)]), x)
    assert np.max(np.abs(y - x)) <= 64 * 2.0 ** -53 * np.max(np.abs(x))
    with pytest.raises(sg.InvalidInputError):
        sg.lowpass_biquad(sr, 24000.0)


def test_seq_is_scipys_sosfilt_where_scipy_imports():
    ss = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(5)
    for name, sos in R.FILTERS.items():
        x = rng.standard_normal(700)
        zi = 0.1 * rng.standard_normal((len(sos), 2))
        y, zf = R.seq(sos, x, zi)
        ys, zs = ss.sosfilt(sos, x, zi=zi)
        assert np.array_equal(y, ys) and np.array_equal(zf, zs), name
        if name == "integrator":
            continue
        # scipy solves zi in f64 by a 2 x 2 system whose determinant is 1 + a1 + a2: its relative error is about 2^-52 / that determinant
        det = float(np.min(1 + sos[:, 4] + sos[:, 5]))
        tol = 64 * len(sos) * 2.0 ** -52 / det
        zs = ss.sosfilt_zi(sos)
        assert np.max(np.abs(R.sosfilt_zi(sos).astype(np.float64) - zs)) <= tol * np.max(np.abs(zs)), name
        for pad in (None, 0, 5):
            f, fs = R.filtfilt(sos, x, pad), ss.sosfiltfilt(sos, x, padtype="odd", padlen=pad)
            assert f.shape == fs.shape and np.max(np.abs(f - fs)) <= max(tol, 1e-13) * max(np.max(np.abs(fs)), np.max(np.abs(x))) * 1e3, (name, pad)


# ---- CPU: the census ------------------------------------------------------------------------------------------------------------------------
def compiled_instances():
    text = open(os.path.join(os.path.dirname(os.path.abspath(_ffi.__file__)), "csrc", "iir.hip")).read()
    m = re.search(r"#define SGX_IIR_SECTIONS\(X\)((?: X\(\d+\))+)", text)
    sections = [int(v) for v in re.findall(r"X\((\d+)\)", m.group(1))]
    # the one launcher expands the list into both types and both directions
    assert re.search(r"launch_t<double, S_, true>.*launch_t<double, S_, false>", text) and re.search(r"launch_t<float, S_, true>.*launch_t<float, S_, false>", text)
    assert text.count("SGX_IIR_SECTIONS(") == 3  # the definition, instance_for and launch_sos
    return {(dt, s, d) for dt in DTYPES for s in sections for d in ("forward", "backward")}


INSTANCE_CASES = [(dt, s, d) for dt in DTYPES for s in (1, 2, 4, 8) for d in ("forward", "backward")]


def test_census_every_compiled_instance_has_a_gpu_case():
    assert compiled_instances() == set(INSTANCE_CASES)
    assert set(INSTANCE_FILTER) == {s for _, s, _ in INSTANCE_CASES}
    for s, name in INSTANCE_FILTER.items():
        assert len(sos_of(s)) == s and sg.IirPlan(sos_of(s), device=HOST).kernel_name == "k_iir_sos"
    # a cascade between two instances runs on the next one, padded with identity sections
    assert len(R.FILTERS["ellip6_bp"]) == 3


# ---- GPU helpers ---------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def forward_reference(name, S, dtype, batch, n, seed):
    """(x, ref, seq) of `batch` Gaussian rows of n samples through the first S sections of a filter, from zero state."""
    x = R.signals(batch, n, NP[dtype], seed)
    sos = R.FILTERS[name][:S]
    return x, R.ref(sos, x)[0], R.seq(sos, x)[0]


# ---- GPU: every instance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,S,direction", INSTANCE_CASES, ids=[f"{d[5:]}-S{s}-{w}" for d, s, w in INSTANCE_CASES])
def test_gpu_every_instance_at_every_seam_length(dtype, S, direction):
    import torch
    sos = sos_of(S)
    plan = sg.IirPlan(sos, dtype=dtype)
    ns = lengths(plan)
    case = f"instance-{dtype}-S{S}-{direction}"
    shares = []
    if direction == "forward":
        x, r, s = forward_reference(INSTANCE_FILTER[S], S, dtype, 3, ns[-1], 11)
        xd = dev(x)
        for n in ns:  # a prefix of a row filters to the prefix of its output
            y = plan.filter_torch(xd[:, :n].contiguous()).cpu().numpy()
            assert plan.kernel_name == "k_iir_sos"
            for b in range(3):
                shares.append(check(case, y[b], s[b, :n], r[b, :n], dtype)[1])
            if dtype == F64:  # the first block of a call runs from its true state in one work item: the sequential recurrence's bits
                assert np.array_equal(y[:, :min(n, L)], s[:, :min(n, L)]), n
    else:  # the backward instance runs the second half of filtfilt; padlen 0 lets it run at every length
        x = R.signals(3, ns[-1], NP[dtype], 12)
        rows = [x[b, :n] for n in ns for b in range(3)]
        r = R.filtfilt_rows(sos, rows, 0, R.LD)
        s = R.filtfilt_rows(sos, rows, 0, np.float64)
        xd = dev(x)
        for i, n in enumerate(ns):
            y = plan.filtfilt_torch(xd[:, :n].contiguous(), padlen=0).cpu().numpy()
            for b in range(3):
                shares.append(check(case, y[b], s[3 * i + b], r[3 * i + b], dtype)[1])
    torch.cuda.synchronize()
    report(case, [v for v in shares if v is not None])


# ---- GPU: the filters, with entry and exit states --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(R.FILTERS))
def test_gpu_filters_with_entry_and_exit_states(name, dtype):
    import torch
    sos = R.FILTERS[name]
    S, n, batch = len(sos), TILE + 37, 3
    plan = sg.IirPlan(sos, dtype=dtype)
    x = R.signals(batch, n, NP[dtype], 21)
    zi = 0.25 * np.random.default_rng(22).standard_normal((batch, S, 2))
    case = f"filter-{name}-{dtype}"
    shares = []
    for z in (None, zi):
        r, _, rt = R.ref(sos, x, z, trajectory=True)
        s, _, st = R.seq(sos, x, z, trajectory=True)
        zf = torch.full((batch, S, 2), float("nan"), dtype=torch.float64, device="cuda")
        y = plan.filter_torch(dev(x), zi=None if z is None else dev(z), zf=zf).cpu().numpy()
        assert plan.kernel_name == ("iir_chain" if S > 8 else "k_iir_sos")
        for b in range(batch):
            shares.append(check(case, y[b], s[b], r[b], dtype)[1])
            check_state(case + "-zf", zf[b].cpu().numpy(), st[b], rt[b])  # (the state is f64 in both types)
        # the host path: the same bits, and scipy's return convention
        yh = plan.filter(x, z, return_zf=True)
        assert np.array_equal(yh[0], y, equal_nan=True) and np.array_equal(yh[1], zf.cpu().numpy())
    report(case, [v for v in shares if v is not None])
    report(case + "-zf")


@pytest.mark.gpu
def test_gpu_one_shot_functions():
    x = R.signals(2, 1000, np.float64, 31)
    sos = R.FILTERS["ellip6_bp"]
    r, s = R.ref(sos, x)[0], R.seq(sos, x)[0]
    y = sg.sosfilt(sos, x)
    assert y.dtype == np.float64 and y.shape == x.shape
    for b in range(2):
        check("one-shot-f64", y[b], s[b], r[b], F64)
    y1, zf = sg.sosfilt(sos, x[0], zi=np.zeros((3, 2)))
    assert np.array_equal(y1, y[0]) and zf.shape == (3, 2)
    f = sg.sosfiltfilt(sos, x[0].astype(np.float32), dtype=F32)
    assert f.dtype == np.float32 and check("one-shot-f32", f, None, R.filtfilt(sos, x[0].astype(np.float32), None, R.LD), F32)[0] <= 1.0
    yb = sg.biquad(x[0], 2.0, 0.0, -2.0, 2.0, -1.0, 0.5)
    rb, sb = R.ref([[1.0, 0.0, -1.0, 1.0, -0.5, 0.25]], x[0])[0], R.seq([[1.0, 0.0, -1.0, 1.0, -0.5, 0.25]], x[0])[0]
    check("one-shot-f64", yb, sb, rb, F64)


# ---- GPU: streaming ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_streaming_pushes_against_one_call(dtype):
    import torch
    name, S = "butter8_lp_0.01", 4
    sos = R.FILTERS[name]
    plan = sg.IirPlan(sos, dtype=dtype)
    pushes = [1, 7, 0, plan.tile + 3, 2 * plan.block]
    n, batch = sum(pushes), 3
    x, r, s = forward_reference(name, S, dtype, batch, n, 41)
    xd = dev(x)

    def run():
        out, at = [], 0
        for m in pushes:
            out.append(plan.process_torch(xd[:, at:at + m].contiguous()))
            at += m
        return torch.cat(out, dim=1)

    first = run()
    y = first.cpu().numpy()
    case = f"streaming-{dtype}"
    shares = [check(case, y[b], s[b], r[b], dtype)[1] for b in range(batch)]
    # the state: against the reference's, round trip bit for bit, and reset returns to the first call's bits
    rt, qt = R.ref(sos, x, trajectory=True)[2], R.seq(sos, x, trajectory=True)[2]
    st = plan.state(batch)
    for b in range(batch):
        check_state(case + "-state", st[b], qt[b], rt[b])
    plan.set_state(st)
    assert np.array_equal(plan.state(batch), st)
    with pytest.raises(sg.DimensionMismatchError, match="rows of the state"):
        plan.process_torch(xd[:2, :8].contiguous())
    plan.reset()
    assert same(run(), first)
    plan.reset()
    plan.process_torch(xd[:2, :8].contiguous())  # reset frees the row count
    # the host path carries the same state
    plan.reset()
    yh = np.concatenate([plan.process(x[:, :100]), plan.process(x[:, 100:100]), plan.process(x[:, 100:300])], axis=1)
    for b in range(batch):
        check(case, yh[b], s[b, :300], r[b, :300], dtype)
    # set_state on a fresh plan continues a row where another plan left it
    a, b2 = sg.IirPlan(sos, dtype=dtype), sg.IirPlan(sos, dtype=dtype)
    ya = a.process_torch(xd[:, :500].contiguous())
    b2.set_state(a.state(batch))
    yb = torch.cat([ya, b2.process_torch(xd[:, 500:].contiguous())], dim=1).cpu().numpy()
    for b in range(batch):
        shares.append(check(case, yb[b], s[b], r[b], dtype)[1])
    report(case, [v for v in shares if v is not None])


# ---- GPU: per-row banks and batch independence -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_per_row_bank_equals_single_filter_plans_bit_for_bit(dtype):
    import torch
    names = ("dc_blocker", "resonator_0.9999", "integrator")
    bank = np.stack([R.FILTERS[k] for k in names])
    n = TILE + 37
    x = dev(R.signals(3, n, NP[dtype], 51))
    plan = sg.IirPlan(bank, dtype=dtype)
    zf = torch.zeros((3, 1, 2), dtype=torch.float64, device="cuda")
    y = plan.filter_torch(x, zf=zf)
    for b, k in enumerate(names):
        z1 = torch.zeros((1, 1, 2), dtype=torch.float64, device="cuda")
        y1 = sg.IirPlan(R.FILTERS[k], dtype=dtype).filter_torch(x[b:b + 1].contiguous(), zf=z1)
        assert same(y[b:b + 1], y1) and same(zf[b:b + 1], z1), k
    xs = x[:2].cpu().numpy()  # filtfilt over a bank, where sosfilt_zi exists
    bank2 = np.stack([R.FILTERS["dc_blocker"], R.FILTERS["resonator_0.9999"]])
    f = sg.IirPlan(bank2, dtype=dtype).filtfilt_torch(x[:2].contiguous())
    for b in range(2):
        f1 = sg.IirPlan(bank2[b], dtype=dtype).filtfilt_torch(dev(xs[b:b + 1]), padlen=9)
        assert same(f[b:b + 1], f1), b


@pytest.mark.gpu
@pytest.mark.parametrize("route,n", [("auto", 2 * TILE + 37), ("split", 3 * SEG + 37)], ids=["k_iir_sos", "split"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_a_row_alone_and_as_row_2_of_5(dtype, route, n):
    sos = R.FILTERS["butter4_hp_0.001"]
    x = dev(R.signals(5, n, NP[dtype], 61))
    plan = sg.IirPlan(sos, dtype=dtype, route=route)
    five = plan.filter_torch(x)
    name = plan.kernel_name
    assert name == ("k_iir_sos+split" if route == "split" else "k_iir_sos")
    alone = sg.IirPlan(sos, dtype=dtype, route=route).filter_torch(x[2:3].contiguous())
    assert same(five[2:3], alone)
    assert same(plan.filtfilt_torch(x)[2:3], plan.filtfilt_torch(x[2:3].contiguous()))
    assert plan.kernel_name == name


# ---- GPU: routes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_split_route_against_the_bound(dtype):
    import torch
    name = "resonator_0.9999"  # a memory of tens of thousands of samples: every segment's entry state matters
    sos = R.FILTERS[name]
    n = 3 * SEG + 37
    x, r, s = forward_reference(name, 1, dtype, 2, n, 71)
    plan = sg.IirPlan(sos, dtype=dtype, route="split")
    zf = torch.zeros((2, 1, 2), dtype=torch.float64, device="cuda")
    y = plan.filter_torch(dev(x), zf=zf).cpu().numpy()
    assert plan.kernel_name == "k_iir_sos+split" and plan.tile == TILE
    case = f"split-{dtype}"
    shares = [check(case, y[b], s[b], r[b], dtype)[1] for b in range(2)]
    rt, qt = R.ref(sos, x, trajectory=True)[2], R.seq(sos, x, trajectory=True)[2]
    for b in range(2):
        check_state(case + "-zf", zf[b].cpu().numpy(), qt[b], rt[b])
    # streaming on the split route: the state passes through launch 2
    h = n // 2
    yp = torch.cat([plan.process_torch(dev(x[:, :h])), plan.process_torch(dev(x[:, h:]))], dim=1).cpu().numpy()
    for b in range(2):
        shares.append(check(case, yp[b], s[b], r[b], dtype)[1])
    # "auto" takes the split route for few long rows, and the one-launch route for short ones
    auto = sg.IirPlan(sos, dtype=dtype)
    ya = auto.filter_torch(dev(x))
    assert auto.kernel_name == "k_iir_sos+split" and np.array_equal(ya.cpu().numpy(), y)
    auto.filter_torch(dev(x[:, :SEG]))
    assert auto.kernel_name == "k_iir_sos"
    report(case, [v for v in shares if v is not None])


@pytest.mark.gpu
def test_gpu_chain_of_12_sections_equals_plans_of_8_and_4_bit_for_bit():
    sos = np.concatenate([R.FILTERS["butter16_lp_0.3"], R.FILTERS["ellip6_bp"], R.FILTERS["dc_blocker"]])
    assert len(sos) == 12
    x = dev(R.signals(3, TILE + 37, np.float64, 81))
    chain = sg.IirPlan(sos, dtype=F64)
    y = chain.filter_torch(x)
    assert chain.kernel_name == "iir_chain" and chain.tile == 0
    y8 = sg.IirPlan(sos[:8], dtype=F64).filter_torch(x)
    y4 = sg.IirPlan(sos[8:], dtype=F64).filter_torch(y8)
    assert same(y, y4)
    # a forced chain of few sections is the one-launch route's arithmetic
    forced = sg.IirPlan(sos[:4], dtype=F64, route="chain")
    assert same(forced.filter_torch(x), sg.IirPlan(sos[:4], dtype=F64).filter_torch(x)) and forced.kernel_name == "iir_chain"
    # 12 sections in f32 against the bound, forward and zero-phase
    x32 = R.signals(2, TILE + 37, np.float32, 82)
    p32 = sg.IirPlan(sos, dtype=F32)
    y32 = p32.filter_torch(dev(x32)).cpu().numpy()
    r = R.ref(sos, x32)[0]
    f32 = p32.filtfilt_torch(dev(x32)).cpu().numpy()
    rf = R.filtfilt_rows(sos, list(x32), None, R.LD)
    for b in range(2):
        check("chain-float32", y32[b], None, r[b], F32)
        check("chain-filtfilt-float32", f32[b], None, rf[b], F32)
    report("chain-float32")
    report("chain-filtfilt-float32")


# ---- GPU: filtfilt ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_filtfilt_at_its_seams_without_allocating(dtype):
    sos = R.FILTERS["butter8_lp_0.01"]
    plan = sg.IirPlan(sos, dtype=dtype)
    pad = plan.padlen
    ns = [pad + 1, TILE, TILE + 1]
    x = R.signals(3, ns[-1], NP[dtype], 91)
    rows = [x[b, :n] for n in ns for b in range(3)]
    r, s = R.filtfilt_rows(sos, rows, None, R.LD), R.filtfilt_rows(sos, rows, None, np.float64)
    plan.reserve(3, ns[-1], host_staging=False)
    count = plan.allocations
    case = f"filtfilt-{dtype}"
    shares = []
    for i, n in enumerate(ns):
        y = plan.filtfilt_torch(dev(x[:, :n])).cpu().numpy()
        for b in range(3):
            shares.append(check(case, y[b], s[3 * i + b], r[3 * i + b], dtype)[1])
    assert plan.allocations == count, "filtfilt allocated after reserve: there is no flipped or extended copy to make"
    # an explicit padlen, and the split route walks backward over segments
    y = plan.filtfilt_torch(dev(x[:1, :500]), padlen=100).cpu().numpy()
    check(case, y[0], R.filtfilt(sos, x[0, :500], 100), R.filtfilt(sos, x[0, :500], 100, R.LD), dtype)
    report(case, [v for v in shares if v is not None])


@pytest.mark.gpu
def test_gpu_filtfilt_on_the_split_route():
    sos = R.FILTERS["dc_blocker"]
    n = 2 * SEG + 37
    x = R.signals(1, n, np.float64, 92)
    plan = sg.IirPlan(sos, dtype=F64, route="split")
    y = plan.filtfilt_torch(dev(x)).cpu().numpy()
    assert plan.kernel_name == "k_iir_sos+split"
    check("filtfilt-split-float64", y[0], R.filtfilt(sos, x[0]), R.filtfilt(sos, x[0], None, R.LD), F64)
    report("filtfilt-split-float64")


# ---- GPU: a NaN inside a row -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_nan_in_one_row(dtype):
    name, S = "butter4_hp_0.001", 2
    n, at = 2 * TILE, TILE + 5
    x, r, s = forward_reference(name, S, dtype, 3, n, 101)
    plan = sg.IirPlan(R.FILTERS[name], dtype=dtype)
    clean = plan.filter_torch(dev(x))
    bad = x.copy()
    bad[1, at] = np.nan
    y = plan.filter_torch(dev(bad))
    assert same(y[0], clean[0]) and same(y[2], clean[2])
    y1 = y[1].cpu().numpy()
    check(f"nan-{dtype}", y1[:at], s[1, :at], r[1, :at], dtype)
    assert np.all(np.isnan(y1[at:]))  # as the reference: a recursive filter never recovers
    assert np.all(np.isnan(R.seq(R.FILTERS[name], bad[1].astype(np.float64))[0][at:]))


# ---- GPU: the stream contract on every route -------------------------------------------------------------------------------------------------
SENTINEL = -1.2345678e30
_PRODUCER = {}


def producer():
    """(buffer, operations): in-place additions on a 1 GiB buffer that take about 25 ms on this device."""
    import torch
    if not _PRODUCER:
        big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
        for _ in range(4):
            big.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(16):
            big.add_(1.0)
        e1.record()
        torch.cuda.synchronize()
        _PRODUCER["big"], _PRODUCER["ops"] = big, max(8, int(math.ceil(25.0 * 16.0 / e0.elapsed_time(e1))))
    return _PRODUCER["big"], _PRODUCER["ops"]


CHAIN12 = np.concatenate([R.BUTTER16_LP, R.ELLIP6_BP, R.FILTERS["dc_blocker"]])
# id -> (sos, route, rows, n, call, route name)
STREAM_CASES = {
    "k_iir_sos-filter": (R.BUTTER4_HP, "auto", 4, TILE + 37, "filter", "k_iir_sos"),
    "k_iir_sos-filtfilt": (R.BUTTER8_LP, "auto", 4, TILE + 37, "filtfilt", "k_iir_sos"),
    "k_iir_sos-process": (R.BUTTER4_HP, "auto", 4, TILE + 37, "process", "k_iir_sos"),
    "split-filter": (R.BUTTER4_HP, "split", 2, 2 * SEG + 37, "filter", "k_iir_sos+split"),
    "split-filtfilt": (R.BUTTER4_HP, "split", 2, 2 * SEG + 37, "filtfilt", "k_iir_sos+split"),
    "chain-filter": (CHAIN12, "auto", 4, TILE + 37, "filter", "iir_chain"),
    "chain-filtfilt": (CHAIN12, "auto", 4, TILE + 37, "filtfilt", "iir_chain"),
}


def stream_call(plan, kind, x, out):
    if kind == "filter":
        plan.filter_torch(x, out=out)
    elif kind == "filtfilt":
        plan.filtfilt_torch(x, out=out)
    else:  # a schedule that starts from and returns to the state after reset: reset, two pushes
        h = x.shape[1] // 2
        plan.reset()
        out[:, :h] = plan.process_torch(x[:, :h].contiguous())
        out[:, h:] = plan.process_torch(x[:, h:].contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", list(STREAM_CASES))
def test_gpu_stream_contract(cid, dtype):
    import torch
    sos, route, rows, n, kind, name = STREAM_CASES[cid]
    inputs = [dev(R.signals(rows, n, NP[dtype], seed)) for seed in (111, 112, 113)]

    def fresh():
        return sg.IirPlan(sos, dtype=dtype, route=route)

    def eager(x):
        p, out = fresh(), torch.empty_like(x)
        stream_call(p, kind, x, out)
        torch.cuda.synchronize()
        assert p.kernel_name == name
        return out

    refs = [eager(x) for x in inputs]
    # A: one operation of the caller's stream, behind a long-running producer whose last operation writes the samples
    big, ops = producer()
    plan = fresh()
    side = torch.cuda.Stream()
    xin, out = torch.empty_like(inputs[0]), torch.empty_like(inputs[0])
    sentinel = torch.full_like(out, SENTINEL)
    with torch.cuda.stream(side):  # warm on other data: scratch and state hold stale values
        xin.copy_(inputs[1])
        stream_call(plan, kind, xin, out)
    torch.cuda.synchronize()
    xin.fill_(float("nan"))
    out.copy_(sentinel)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record()
        for _ in range(ops):
            big.add_(1.0)
        xin.copy_(inputs[0])
        e1.record()
        stream_call(plan, kind, xin, out)
        snap = out.clone()
        out.copy_(sentinel)
    producer_done = e1.query()
    torch.cuda.synchronize()
    assert same(snap, refs[0]), "the result queued behind the producer differs from the call on the default stream"
    assert same(out, sentinel), "something wrote the output after the work queued behind the call"
    assert e0.elapsed_time(e1) >= 10.0 and producer_done is False, "no hazard window was shown"
    # B: after reserve the call is captured into a graph and replayed; the allocation counter stands still
    plan = fresh()
    plan.reserve(rows, n, host_staging=False)
    count = plan.allocations
    xin = inputs[0].clone()
    out.copy_(sentinel)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        stream_call(plan, kind, xin, out)
    for k in (1, 2):
        xin.copy_(inputs[k])
        out.copy_(sentinel)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, refs[k]), f"replay {k} differs from the eager result"
    assert plan.allocations == count and plan.kernel_name == name
    # C: three calls with other shapes in between do not change a repeated call's bits
    plan = fresh()
    stream_call(plan, kind, inputs[0], out)
    assert same(out, refs[0])
    for b, m in ((1, 100), (rows, n + 4096), (rows - 1, 2 * TILE)):
        if kind == "process":
            plan.reset()
        small = inputs[2][:b, :m].contiguous() if m <= n else torch.cat([inputs[2], inputs[1][:, :m - n]], dim=1)[:b].contiguous()
        stream_call(plan, kind, small, torch.empty_like(small))
    stream_call(plan, kind, inputs[0], out)
    torch.cuda.synchronize()
    assert same(out, refs[0]) and plan.kernel_name == name
