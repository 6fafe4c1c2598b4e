"""Where the nine plan types of the C ABI keep their error texts (CPU only: every plan here is host-only, device -2).

A failed create leaves its text in a per-thread string of that plan type (sgx_fft2d and sgx_c2c share one), read with
<prefix>_last_error(NULL) — sgx_last_create_error() for sgx_plan; a failed call leaves its text on the plan and nowhere else.
"""
import ctypes as C
import threading

import numpy as np
import pytest

from spectrograms_amd import _ffi

HOST = _ffi.DEVICE_HOST_ONLY
NO_DEVICE = b"hip -- FFT backend error: plan has no HIP device (host-only plan)"
L = _ffi.lib()
X = np.zeros(8192, np.float64)  # input and output of every refused call (nothing reads or writes it)
PX = X.ctypes.data


def _stft(n_fft=1024):
    return _ffi.SgxParams(n_fft=n_fft, hop_size=256, centre=1, window_kind=_ffi.WIN_HANNING, sample_rate_hz=16000.0,
                          freq_scale=_ffi.FREQ_LINEAR, amp_scale=_ffi.AMP_POWER, dtype=_ffi.F32, device=HOST)


def _itd(power=1):
    return _ffi.SgxBinauralParams(_ffi.BINAURAL_ITD, 100.0, 500.0, power, 0)


ONES = (C.c_double * 5)(1, 1, 1, 1, 1)


class Family:
    """create(out, variant): variant None is a valid host-only plan, "a" and "b" two invalid inputs with different texts.
    call(h, out_elems): a compute call with out_elems (the wrong one where `expected` is given, else ignored); expected(h): the
    right out_elems of that call, None where the call has no such argument."""

    def __init__(self, name, create, call, expected=None, create_error=None):
        self.name, self.create, self.call, self.expected = name, create, call, expected
        self.destroy = getattr(L, name + "_destroy")
        self.last_error = getattr(L, "sgx_last_error" if name == "sgx_plan" else name + "_last_error")
        self.create_error = create_error or (lambda: self.last_error(None))

    def open(self):
        h = C.c_void_p()
        assert self.create(C.byref(h), None) == _ffi.SGX_OK and h.value
        return h

    def fail_create(self, variant):
        h = C.c_void_p()
        assert self.create(C.byref(h), variant) == _ffi.SGX_INVALID_INPUT and not h.value
        assert self.create_error().startswith(b"Invalid input:")


def _binaural_shape(h):
    sb, nb, nf = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert L.sgx_binaural_output_shape(h, 4096, C.byref(sb), C.byref(nb), C.byref(nf)) == _ffi.SGX_OK
    assert (sb.value, nb.value, nf.value) == (6, 26, 17)  # bins round(100 / 15.625) .. round(500 / 15.625), 1 + 4096 / 256 frames
    return nb.value * nf.value


FAMILIES = [
    Family("sgx_plan",
           lambda out, v: L.sgx_plan_create(None if v == "a" else C.byref(_stft(0 if v == "b" else 1024)), out),
           lambda h, n: L.sgx_execute(h, PX, 1, 4096, 4096, PX, n, _ffi.MEM_HOST, None),
           lambda h: 513 * 17, create_error=L.sgx_last_create_error),
    Family("sgx_fft2d",
           lambda out, v: L.sgx_fft2d_create(0 if v == "a" else 8, 8, 5 if v == "b" else _ffi.F32, HOST, out),
           lambda h, n: L.sgx_fft2d_forward(h, PX, 1, PX, _ffi.MEM_HOST, None)),
    Family("sgx_c2c",
           lambda out, v: L.sgx_c2c_create(0 if v == "a" else 8, 5 if v == "b" else _ffi.F32, HOST, out),
           lambda h, n: L.sgx_c2c_forward(h, PX, n),
           lambda h: 8),
    Family("sgx_mdct",
           lambda out, v: L.sgx_mdct_create(9 if v == "b" else 10, 0 if v == "a" else 5, _ffi.WIN_HANNING, 0.0, None, 0, _ffi.F32, HOST, out),
           lambda h, n: L.sgx_mdct_forward(h, PX, 1, 20, PX, n, _ffi.MEM_HOST, None),
           lambda h: 15),  # 5 coefficients x 3 frames (tests/test_mdct.py)
    Family("sgx_binaural",
           lambda out, v: L.sgx_binaural_create(None if v == "a" else C.byref(_stft()), C.byref(_itd(0 if v == "b" else 1)), out),
           lambda h, n: L.sgx_binaural_execute(h, PX, PX, 1, 4096, 4096, PX, n, _ffi.MEM_HOST, None),
           _binaural_shape),
    Family("sgx_gammatone",
           lambda out, v: L.sgx_gammatone_create(8000.0, 64, 0 if v == "a" else 16, 1 if v == "b" else 8, 100.0, 3000.0, 0, 0, 0.0,
                                                 _ffi.F64, HOST, out),
           lambda h, n: L.sgx_gammatone_execute(h, PX, 1, 128, 128, PX, n, _ffi.MEM_HOST, None),
           lambda h: 8 * 5),  # 8 bands x (1 + (128 - 64) / 16) frames
    Family("sgx_fir",
           lambda out, v: L.sgx_fir_create(ONES, 0 if v == "a" else 5, 1, 0, 0, 5 if v == "b" else _ffi.F32, HOST, out),
           lambda h, n: L.sgx_fir_process(h, PX, 1, 16, 16, PX, n, _ffi.MEM_HOST, None),
           lambda h: 16),  # (tests/test_fir.py)
    Family("sgx_deconv",
           lambda out, v: L.sgx_deconv_create(0 if v == "a" else 8, 4, 0.0, 5 if v == "b" else _ffi.F32, HOST, out),
           lambda h, n: L.sgx_deconv_execute(h, PX, PX, 1, 1, PX, n, _ffi.MEM_HOST, None),
           lambda h: 5),  # 8 - 4 + 1
    Family("sgx_minphase",
           lambda out, v: L.sgx_minphase_create(0 if v == "a" else 5, 0 if v == "b" else 5, 8, 0, _ffi.F32, HOST, out),
           lambda h, n: L.sgx_minphase_execute(h, PX, 1, PX, n, _ffi.MEM_HOST, None),
           lambda h: 5),
]
IDS = [f.name for f in FAMILIES]
SHARED = {"sgx_fft2d": "sgx_c2c", "sgx_c2c": "sgx_fft2d"}


def create_errors():
    return {f.name: f.create_error() for f in FAMILIES}


def in_thread(fn):
    """Run fn on a newly started thread; its assertion failures are re-raised here."""
    box = []

    def run():
        try:
            fn()
        except BaseException as e:  # noqa: BLE001 (handed to the caller)
            box.append(e)
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if box:
        raise box[0]


def test_create_errors_are_per_family():
    def body():
        assert create_errors() == dict.fromkeys(IDS, b"")  # a fresh thread has no create error
        assert L.sgx_last_error(None) == b""
        for f in FAMILIES:
            before = create_errors()
            f.fail_create("a")
            after = create_errors()
            assert after[f.name] != before[f.name]
            for other in IDS:
                if other == f.name:
                    continue
                if SHARED.get(f.name) == other:
                    assert after[other] == after[f.name]  # sgx_fft2d and sgx_c2c: one string
                else:
                    assert after[other] == before[other], (f.name, other)
        assert L.sgx_last_error(None) == L.sgx_last_create_error()  # sgx_last_error(NULL) reads the create error too
    in_thread(body)


def test_create_errors_are_per_thread():
    for f in FAMILIES:
        f.fail_create("a")
    mine = create_errors()
    assert all(mine.values())
    theirs = {}

    def body():
        assert create_errors() == dict.fromkeys(IDS, b"")
        for f in FAMILIES:
            f.fail_create("b")
        theirs.update(create_errors())
    in_thread(body)
    assert create_errors() == mine
    for f in FAMILIES:
        if f.name != "sgx_fft2d":  # (its text is the one sgx_c2c left in the shared string, the same in both threads' runs)
            assert theirs[f.name] != mine[f.name], f.name
    assert theirs["sgx_fft2d"] == theirs["sgx_c2c"] and mine["sgx_fft2d"] == mine["sgx_c2c"]


@pytest.mark.parametrize("f", FAMILIES, ids=IDS)
def test_call_errors_go_to_the_plan(f):
    f.fail_create("a")
    h = f.open()
    try:
        before = create_errors()
        assert f.last_error(h) == b""
        assert f.call(h, f.expected(h) if f.expected else 0) == _ffi.SGX_BACKEND
        assert f.last_error(h) == NO_DEVICE
        assert create_errors() == before and before[f.name]
    finally:
        f.destroy(h)


@pytest.mark.parametrize("f", [f for f in FAMILIES if f.expected], ids=[f.name for f in FAMILIES if f.expected])
def test_dimension_mismatch_text(f):
    h = f.open()
    try:
        n = f.expected(h)
        before = create_errors()
        for got in (n - 1, n + 3):
            assert f.call(h, got) == _ffi.SGX_DIM_MISMATCH  # (checked before the host-only refusal)
            assert f.last_error(h) == b"Dimension mismatch: expected %d, got %d" % (n, got)
        assert create_errors() == before
        if f.name == "sgx_plan":
            e, g = C.c_size_t(), C.c_size_t()
            assert L.sgx_last_dim_mismatch(h, C.byref(e), C.byref(g)) == _ffi.SGX_OK and (e.value, g.value) == (n, n + 3)
    finally:
        f.destroy(h)
