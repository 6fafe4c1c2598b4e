"""ctypes binding of include/spectro_hip.h — the same symbols a Rust `fft_backend::hip_backend` would bind.

The library is REQUIRED: importing this module without a built libspectro_hip.so raises; there is no
CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# SGX_LIB_PATH lets kernel A/B experiments (tools/ablate.sh) load an alternative build of the same ABI
LIB_PATH = os.environ.get("SGX_LIB_PATH") or os.path.join(_PKG, "libspectro_hip.so")

SGX_OK, SGX_INVALID_INPUT, SGX_DIM_MISMATCH, SGX_BACKEND, SGX_INTERNAL = range(5)
WIN_RECTANGULAR, WIN_HANNING, WIN_HAMMING, WIN_BLACKMAN, WIN_KAISER, WIN_GAUSSIAN, WIN_CUSTOM = range(7)
FREQ_LINEAR, FREQ_MEL, FREQ_LOGHZ, FREQ_ERB, FREQ_CHROMA, FREQ_CQT = 0, 1, 2, 3, 4, 5
MELNORM_NONE, MELNORM_SLANEY, MELNORM_L1, MELNORM_L2 = range(4)
AMP_POWER, AMP_MAGNITUDE, AMP_DECIBELS, AMP_COMPLEX = range(4)
F32, F64 = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1
DEVICE_CURRENT, DEVICE_HOST_ONLY = -1, -2
FIR_ROUTE_AUTO, FIR_ROUTE_GENERIC = 0, 1
MINPHASE_ROUTE_AUTO, MINPHASE_ROUTE_GENERIC = 0, 1
RESAMPLE_ROUTE_AUTO, RESAMPLE_ROUTE_GENERIC = 0, 1
RESAMPLE_SINC_HANN, RESAMPLE_SINC_KAISER = 0, 1
WELCH_PSD, WELCH_CSD, WELCH_COHERENCE = 0, 1, 2
WELCH_DETREND_NONE, WELCH_DETREND_CONSTANT, WELCH_DETREND_LINEAR = 0, 1, 2
WELCH_DENSITY, WELCH_SPECTRUM = 0, 1
WELCH_ROUTE_AUTO, WELCH_ROUTE_GENERIC = 0, 1
KALDI_WIN_HANNING, KALDI_WIN_HAMMING, KALDI_WIN_POVEY, KALDI_WIN_RECTANGULAR, KALDI_WIN_BLACKMAN = range(5)
KALDI_ROUTE_AUTO, KALDI_ROUTE_GENERIC = 0, 1
IIR_ROUTE_AUTO, IIR_ROUTE_SPLIT, IIR_ROUTE_CHAIN = 0, 1, 2

class SgxParams(C.Structure):
    _fields_ = [
        ("n_fft", C.c_uint32), ("hop_size", C.c_uint32), ("centre", C.c_int32), ("window_kind", C.c_int32),
        ("window_param", C.c_double), ("custom_window", C.POINTER(C.c_double)), ("custom_window_len", C.c_uint32),
        ("sample_rate_hz", C.c_double), ("freq_scale", C.c_int32), ("n_mels", C.c_uint32), ("f_min", C.c_double),
        ("f_max", C.c_double), ("mel_norm", C.c_int32), ("amp_scale", C.c_int32), ("has_log_params", C.c_int32),
        ("floor_db", C.c_double), ("dtype", C.c_int32), ("device", C.c_int32),
        ("n_mfcc", C.c_uint32), ("mfcc_include_c0", C.c_int32), ("mfcc_lifter", C.c_uint32), ("erb_spacing", C.c_int32),
        ("chroma_tuning", C.c_double), ("chroma_norm", C.c_int32),
    ]


class SgxCqtParams(C.Structure):
    _fields_ = [
        ("bins_per_octave", C.c_uint32), ("n_octaves", C.c_uint32), ("f_min", C.c_double), ("q_factor", C.c_double),
        ("window_kind", C.c_int32), ("window_param", C.c_double), ("sparsity_threshold", C.c_double), ("normalize", C.c_int32),
    ]


BINAURAL_ITD, BINAURAL_IPD, BINAURAL_ILD, BINAURAL_ILR = range(4)


class SgxBinauralParams(C.Structure):
    _fields_ = [("kind", C.c_int32), ("start_freq", C.c_double), ("end_freq", C.c_double), ("magphase_power", C.c_uint32),
                ("wrapped", C.c_int32)]


class SgxKaldiParams(C.Structure):
    _fields_ = [
        ("sample_frequency", C.c_double), ("frame_length_ms", C.c_double), ("frame_shift_ms", C.c_double),
        ("blackman_coeff", C.c_double), ("preemphasis_coefficient", C.c_double), ("energy_floor", C.c_double), ("low_freq", C.c_double),
        ("high_freq", C.c_double), ("dither", C.c_double), ("vtln_warp", C.c_double), ("min_duration", C.c_double),
        ("cepstral_lifter", C.c_double),
        ("window_type", C.c_int32), ("remove_dc_offset", C.c_int32), ("raw_energy", C.c_int32), ("round_to_power_of_two", C.c_int32),
        ("snip_edges", C.c_int32), ("use_energy", C.c_int32), ("use_power", C.c_int32), ("use_log_fbank", C.c_int32),
        ("htk_compat", C.c_int32), ("subtract_mean", C.c_int32), ("spectrogram", C.c_int32), ("streaming", C.c_int32),
        ("num_mel_bins", C.c_uint32), ("num_ceps", C.c_uint32), ("dtype", C.c_int32), ("device", C.c_int32),
    ]


# ---- the C ABI, once: name -> (restype, argtypes), grouped by family as include/spectro_hip.h is.  lib() applies it; tests/test_abi.py
# checks it against the header's declarations, parameter by parameter.  A new family adds its block here and nowhere else.
_vp, _sz, _i32, _u32, _i64, _f64, _str = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32, C.c_int64, C.c_double, C.c_char_p
_P = C.POINTER
_ST = C.c_int  # sgx_status
_EXEC = [_vp, _vp, _sz, _sz, _sz, _vp, _sz, _i32, _vp]  # plan, in, batch, n, stride, out, out_elems, mem_kind, stream
_FLUSH = [_vp, _vp, _sz, _i32, _vp]                     # plan, out, out_elems, mem_kind, stream
_RESERVE = [_vp, _sz, _sz, _i32]                        # plan, batch, n, host_staging


def _family(prefix, sizes=(), kernel_name=True, device=True):
    """What every family declares alike: <prefix>_destroy, _last_error, _device, _kernel_name and its size_t getters."""
    d = {f"{prefix}_destroy": (None, [_vp]), f"{prefix}_last_error": (_str, [_vp])}
    if device:
        d[f"{prefix}_device"] = (_i32, [_vp])
    if kernel_name:
        d[f"{prefix}_kernel_name"] = (_str, [_vp])
    d.update({f"{prefix}_{g}": (_sz, [_vp]) for g in sizes})
    return d


SIGNATURES = {
    # spectrogram plans (sgx_plan)
    "sgx_plan_create": (_ST, [_P(SgxParams), _P(_vp)]),
    "sgx_plan_destroy": (None, [_vp]),
    "sgx_plan_create_cqt": (_ST, [_P(SgxParams), _P(SgxCqtParams), _P(_vp)]),
    "sgx_plan_create_cqt_transform": (_ST, [_P(SgxParams), _P(SgxCqtParams), _P(_vp)]),
    "sgx_cqt_set_route": (_ST, [_vp, _i32]),
    "sgx_cqt_kernels": (_ST, [_vp, _P(_sz), _P(_u32), _P(_f64), _P(_f64)]),
    "sgx_output_shape": (_ST, [_vp, _sz, _P(_sz), _P(_sz)]),
    "sgx_execute": (_ST, _EXEC),
    "sgx_execute_timed": (_ST, [_vp, _vp, _sz, _sz, _sz, _vp, _sz, _vp, _i32, _P(C.c_float)]),
    "sgx_axes": (_ST, [_vp, _sz, _P(_f64), _P(_f64)]),
    "sgx_r2c": (_ST, [_vp, _vp, _sz, _vp, _sz]),
    "sgx_c2r": (_ST, [_vp, _vp, _sz, _vp, _sz]),
    "sgx_istft_length": (_ST, [_vp, _sz, _P(_sz)]),
    "sgx_istft": (_ST, _EXEC),
    "sgx_window": (_ST, [_vp, _P(_f64)]),
    "sgx_mel_weights": (_ST, [_vp, _P(_sz), _P(_u32), _P(_u32), _P(_f64)]),
    "sgx_reserve": (_ST, [_vp, _sz, _sz, _i32, _i32]),
    "sgx_plan_device": (_i32, [_vp]),
    "sgx_last_dim_mismatch": (_ST, [_vp, _P(_sz), _P(_sz)]),
    "sgx_last_error": (_str, [_vp]),
    "sgx_last_create_error": (_str, []),
    "sgx_kernel_name": (_str, [_vp]),
    "sgx_execute_kernel_name": (_str, [_vp]),
    "sgx_istft_kernel_name": (_str, [_vp]),
    "sgx_bank_stage_name": (_str, [_vp]),
    "sgx_abi_version": (_i32, []),
    "sgx_device_count": (_i32, []),
    "sgx_membench": (_ST, [_i32, _sz, _i32, _i32, _P(_f64)]),
    "sgx_clock_probe": (_ST, [_i32, _vp, _P(_f64)]),
    # sharding (sgx_comm)
    "sgx_shard_range": (_ST, [_sz, _i32, _i32, _P(_sz), _P(_sz)]),
    "sgx_comm_unique_id": (_ST, [_vp]),
    "sgx_comm_create": (_ST, [_vp, _i32, _i32, _i32, _P(_vp)]),
    "sgx_comm_adopt": (_ST, [_vp, _i32, _i32, _i32, _P(_vp)]),
    **_family("sgx_comm", kernel_name=False, device=False),
    "sgx_gather": (_ST, [_vp, _vp, _vp, _sz, _sz, _i32, _vp]),
    "sgx_shard_execute": (_ST, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp, _vp]),
    "sgx_shard_execute_chunked": (_ST, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp, _i32, _vp]),
    # 2-D FFT (sgx_fft2d) and 1-D complex (sgx_c2c)
    "sgx_fft2d_create": (_ST, [_sz, _sz, _i32, _i32, _P(_vp)]),
    **_family("sgx_fft2d"),
    "sgx_fft2d_forward": (_ST, [_vp, _vp, _sz, _vp, _i32, _vp]),
    "sgx_fft2d_inverse": (_ST, [_vp, _vp, _sz, _vp, _i32, _vp]),
    "sgx_fft2d_convolve": (_ST, [_vp, _vp, _sz, _vp, _sz, _sz, _vp, _i32, _vp]),
    "sgx_fft2d_filter": (_ST, [_vp, _vp, _sz, _i32, _f64, _f64, _vp, _i32, _vp]),
    "sgx_fft2d_reserve": (_ST, [_vp, _sz, _i32]),
    "sgx_c2c_create": (_ST, [_sz, _i32, _i32, _P(_vp)]),
    **_family("sgx_c2c", kernel_name=False, device=False),
    "sgx_c2c_forward": (_ST, [_vp, _vp, _sz]),
    "sgx_c2c_inverse": (_ST, [_vp, _vp, _sz]),
    # MDCT (sgx_mdct)
    "sgx_mdct_create": (_ST, [_sz, _sz, _i32, _f64, _P(_f64), _u32, _i32, _i32, _P(_vp)]),
    **_family("sgx_mdct", kernel_name=False),
    "sgx_mdct_kernel_name": (_str, [_vp, _i32]),
    "sgx_mdct_output_shape": (_ST, [_vp, _sz, _P(_sz), _P(_sz)]),
    "sgx_mdct_inverse_length": (_ST, [_vp, _sz, _P(_sz)]),
    "sgx_mdct_forward": (_ST, [_vp, _vp, _sz, _sz, _vp, _sz, _i32, _vp]),
    "sgx_mdct_inverse": (_ST, _EXEC),
    "sgx_mdct_reserve": (_ST, _RESERVE),
    "sgx_mdct_window": (_ST, [_vp, _P(_f64)]),
    # binaural (sgx_binaural)
    "sgx_binaural_create": (_ST, [_P(SgxParams), _P(SgxBinauralParams), _P(_vp)]),
    **_family("sgx_binaural"),
    "sgx_binaural_output_shape": (_ST, [_vp, _sz, _P(_sz), _P(_sz), _P(_sz)]),
    "sgx_binaural_axes": (_ST, [_vp, _sz, _P(_f64), _P(_f64)]),
    "sgx_binaural_execute": (_ST, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _sz, _i32, _vp]),
    "sgx_binaural_histogram": (_ST, [_vp, _vp, _sz, _sz, _sz, _f64, _f64, _i32, _i32, _vp, _sz, _i32, _vp]),
    "sgx_binaural_reserve": (_ST, _RESERVE),
    # gammatone (sgx_gammatone)
    "sgx_gammatone_create": (_ST, [_f64, _sz, _sz, _u32, _f64, _f64, _i32, _i32, _f64, _i32, _i32, _P(_vp)]),
    **_family("sgx_gammatone"),
    "sgx_gammatone_output_shape": (_ST, [_vp, _sz, _P(_sz), _P(_sz)]),
    "sgx_gammatone_execute": (_ST, _EXEC),
    "sgx_gammatone_center_frequencies": (_ST, [_vp, _P(_f64)]),
    "sgx_gammatone_coefficients": (_ST, [_vp, _P(_f64)]),
    "sgx_gammatone_reserve": (_ST, _RESERVE),
    # FIR and deconvolution (sgx_fir, sgx_deconv)
    "sgx_fir_create": (_ST, [_P(_f64), _sz, _sz, _sz, _i32, _i32, _i32, _P(_vp)]),
    **_family("sgx_fir", sizes=("fft_size", "step", "taps")),
    "sgx_fir_process": (_ST, _EXEC),
    "sgx_fir_convolve": (_ST, _EXEC),
    "sgx_fir_reset": (_ST, [_vp, _vp]),
    "sgx_fir_reserve": (_ST, _RESERVE),
    "sgx_deconv_create": (_ST, [_sz, _sz, _f64, _i32, _i32, _P(_vp)]),
    **_family("sgx_deconv", sizes=("output_length",), kernel_name=False),
    "sgx_deconv_execute": (_ST, [_vp, _vp, _vp, _sz, _sz, _vp, _sz, _i32, _vp]),
    "sgx_deconv_reserve": (_ST, _RESERVE),
    # minimum phase (sgx_minphase)
    "sgx_minphase_create": (_ST, [_sz, _sz, _sz, _i32, _i32, _i32, _P(_vp)]),
    **_family("sgx_minphase", sizes=("fft_size", "output_length", "taps")),
    "sgx_minphase_execute": (_ST, [_vp, _vp, _sz, _vp, _sz, _i32, _vp]),
    "sgx_minphase_reserve": (_ST, [_vp, _sz, _i32]),
    # streaming forward and inverse (sgx_stream, sgx_istream)
    "sgx_stream_create": (_ST, [_P(SgxParams), _P(_vp)]),
    **_family("sgx_stream", sizes=("pending", "frames_emitted", "n_bins", "allocations")),
    "sgx_stream_step": (_ST, [_vp, _sz, _sz, _P(_sz), _P(_sz)]),
    "sgx_stream_flush_frames": (_ST, [_vp, _P(_sz)]),
    "sgx_stream_push": (_ST, _EXEC),
    "sgx_stream_flush": (_ST, _FLUSH),
    "sgx_stream_reset": (_ST, [_vp, _vp]),
    "sgx_stream_reserve": (_ST, _RESERVE),
    "sgx_istream_create": (_ST, [_P(SgxParams), _P(_vp)]),
    **_family("sgx_istream", sizes=("frames_taken", "samples_emitted", "pending", "allocations")),
    "sgx_istream_step": (_ST, [_vp, _sz, _sz, _P(_sz)]),
    "sgx_istream_flush_samples": (_ST, [_vp, _P(_sz)]),
    "sgx_istream_push": (_ST, [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _i32, _vp]),
    "sgx_istream_flush": (_ST, _FLUSH),
    "sgx_istream_reset": (_ST, [_vp, _vp]),
    "sgx_istream_reserve": (_ST, _RESERVE),
    # sample-rate conversion (sgx_resample)
    "sgx_resample_create": (_ST, [_i64, _i64, _i32, _f64, _i32, _f64, _i32, _i32, _i32, _P(_vp)]),
    **_family("sgx_resample", sizes=("up", "down", "taps_per_phase", "tile", "consumed", "emitted", "allocations")),
    "sgx_resample_resample": (_ST, _EXEC),
    "sgx_resample_process": (_ST, _EXEC),
    "sgx_resample_flush": (_ST, _FLUSH),
    "sgx_resample_reset": (_ST, [_vp, _vp]),
    "sgx_resample_reserve": (_ST, _RESERVE),
    "sgx_resample_step": (_ST, [_vp, _sz, _sz, _P(_sz), _P(_sz)]),
    "sgx_resample_out_len": (_sz, [_vp, _sz]),
    "sgx_resample_taps": (_ST, [_vp, _P(_f64)]),
    "sgx_resample_phase_offsets": (_ST, [_vp, _P(_i64)]),
    # Welch estimates (sgx_welch)
    "sgx_welch_create": (_ST, [_P(SgxParams), _i32, _i32, _i32, _i32, _sz, _P(_vp)]),
    **_family("sgx_welch", sizes=("n_bins", "allocations", "tile")),
    "sgx_welch_n_segments": (_sz, [_vp, _sz]),
    "sgx_welch_frequencies": (_ST, [_vp, _P(_f64)]),
    "sgx_welch_window": (_ST, [_vp, _P(_f64)]),
    "sgx_welch_scale": (_f64, [_vp]),
    "sgx_welch_execute": (_ST, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _sz, _i32, _vp]),
    "sgx_welch_reserve": (_ST, _RESERVE),
    # Kaldi fbank / MFCC features (sgx_kaldi)
    "sgx_kaldi_create": (_ST, [_P(SgxKaldiParams), _i32, _sz, _P(_vp)]),
    **_family("sgx_kaldi", sizes=("window_size", "window_shift", "padded_window_size", "n_out", "tile", "allocations")),
    "sgx_kaldi_n_frames": (_sz, [_vp, _sz]),
    "sgx_kaldi_window": (_ST, [_vp, _P(_f64)]),
    "sgx_kaldi_mel_banks": (_ST, [_vp, _P(_f64)]),
    "sgx_kaldi_dct": (_ST, [_vp, _P(_f64)]),
    "sgx_kaldi_lifter": (_ST, [_vp, _P(_f64)]),
    "sgx_kaldi_execute": (_ST, _EXEC),
    "sgx_kaldi_reserve": (_ST, _RESERVE),
}
SYMBOLS = list(SIGNATURES)  # every symbol include/spectro_hip.h declares

# the IIR family's block, a table of its own because its declarations live in include/spectro_hip_iir.h; lib() applies it after SIGNATURES
# and tests/test_iir.py checks it against that header by the rules of tests/test_abi.py
IIR_SIGNATURES = {
    "sgx_iir_create": (_ST, [_P(_f64), _sz, _sz, _i32, _i32, _i32, _P(_vp)]),
    **_family("sgx_iir", sizes=("n_sections", "padlen", "tile", "block", "allocations")),
    "sgx_iir_filter": (_ST, [_vp, _vp, _sz, _sz, _sz, _vp, _sz, _vp, _vp, _i32, _vp]),
    "sgx_iir_process": (_ST, _EXEC),
    "sgx_iir_filtfilt": (_ST, [_vp, _vp, _sz, _sz, _sz, _vp, _sz, _i64, _i32, _vp]),
    "sgx_iir_reset": (_ST, [_vp, _vp]),
    "sgx_iir_state": (_ST, [_vp, _P(_f64), _sz, _vp]),
    "sgx_iir_set_state": (_ST, [_vp, _P(_f64), _sz, _vp]),
    "sgx_iir_reserve": (_ST, _RESERVE),
    "sgx_iir_transition": (_ST, [_vp, _i32, _P(_f64)]),
    "sgx_iir_zi": (_ST, [_vp, _P(_f64)]),
}


class SpectrogramError(Exception):
    """Base error (src/python/error.rs:10-66)."""


class InvalidInputError(SpectrogramError):
    pass


class DimensionMismatchError(SpectrogramError):
    """DimensionMismatch { expected, got } (src/error.rs:19-21): the two numbers are attributes when the library reported them."""

    def __init__(self, msg="", expected=None, got=None):
        super().__init__(msg)
        self.expected, self.got = expected, got


class FFTBackendError(SpectrogramError):
    pass


class InternalError(SpectrogramError):
    pass


_ERR = {SGX_INVALID_INPUT: InvalidInputError, SGX_DIM_MISMATCH: DimensionMismatchError,
        SGX_BACKEND: FFTBackendError, SGX_INTERNAL: InternalError}

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FFTBackendError(
            f"hip -- FFT backend error: {LIB_PATH} is not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `python -m spectrograms_amd.build`); this package has no CPU fallback")
    try:
        # torch wheels bundle their own HIP/HSA runtime.  Load it first so libspectro_hip.so binds to that same
        # copy (same SONAME) instead of pulling /opt/rocm's: two HIP runtimes in one process cannot both see the GPU.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**SIGNATURES, **IIR_SIGNATURES}.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def np_dtype(code: int):
    """numpy type of a dtype code (F32 / F64)."""
    return np.float32 if code == F32 else np.float64


def raise_status(status: int, plan=None) -> None:
    if status == SGX_OK:
        return
    L = lib()
    msg = (L.sgx_last_error(plan) if plan else L.sgx_last_create_error()) or b""
    text = msg.decode() or f"status {status}"
    if status == SGX_DIM_MISMATCH and plan:
        e, g = C.c_size_t(), C.c_size_t()
        if L.sgx_last_dim_mismatch(plan, C.byref(e), C.byref(g)) == SGX_OK:
            raise DimensionMismatchError(text, e.value, g.value)
    raise _ERR.get(status, InternalError)(text)


# the base of the satellite plan families and the plan cache live in _handle.py, which reads the names above at call time
from ._handle import NativeHandle, PlanCache, clear_plan_caches, current_device_key, custom_window, dtype_name  # noqa: E402,F401
