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

# every symbol include/spectro_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "sgx_plan_create", "sgx_plan_destroy", "sgx_output_shape", "sgx_execute", "sgx_execute_timed", "sgx_axes",
    "sgx_r2c", "sgx_c2r", "sgx_istft", "sgx_istft_length", "sgx_window", "sgx_mel_weights", "sgx_shard_range", "sgx_last_error", "sgx_last_create_error",
    "sgx_kernel_name", "sgx_istft_kernel_name", "sgx_bank_stage_name", "sgx_abi_version", "sgx_device_count",
    "sgx_fft2d_create", "sgx_fft2d_destroy", "sgx_fft2d_forward", "sgx_fft2d_inverse", "sgx_fft2d_convolve",
    "sgx_fft2d_filter", "sgx_fft2d_last_error", "sgx_fft2d_reserve", "sgx_fft2d_device", "sgx_fft2d_kernel_name",
    "sgx_reserve", "sgx_plan_device", "sgx_last_dim_mismatch",
    "sgx_c2c_create", "sgx_c2c_destroy", "sgx_c2c_forward", "sgx_c2c_inverse", "sgx_c2c_last_error",
    "sgx_comm_unique_id", "sgx_comm_create", "sgx_comm_adopt", "sgx_comm_destroy", "sgx_comm_last_error", "sgx_gather", "sgx_shard_execute", "sgx_shard_execute_chunked",
    "sgx_membench", "sgx_clock_probe", "sgx_plan_create_cqt", "sgx_cqt_kernels", "sgx_plan_create_cqt_transform", "sgx_cqt_set_route",
    "sgx_mdct_create", "sgx_mdct_destroy", "sgx_mdct_output_shape", "sgx_mdct_inverse_length", "sgx_mdct_forward", "sgx_mdct_inverse",
    "sgx_mdct_reserve", "sgx_mdct_window", "sgx_mdct_kernel_name", "sgx_mdct_device", "sgx_mdct_last_error",
    "sgx_binaural_create", "sgx_binaural_destroy", "sgx_binaural_output_shape", "sgx_binaural_axes", "sgx_binaural_execute",
    "sgx_binaural_histogram", "sgx_binaural_reserve", "sgx_binaural_kernel_name", "sgx_binaural_device", "sgx_binaural_last_error",
    "sgx_gammatone_create", "sgx_gammatone_destroy", "sgx_gammatone_output_shape", "sgx_gammatone_execute", "sgx_gammatone_center_frequencies",
    "sgx_gammatone_coefficients", "sgx_gammatone_reserve", "sgx_gammatone_kernel_name", "sgx_gammatone_device", "sgx_gammatone_last_error",
    "sgx_fir_create", "sgx_fir_destroy", "sgx_fir_process", "sgx_fir_convolve", "sgx_fir_reset", "sgx_fir_reserve", "sgx_fir_fft_size",
    "sgx_fir_step", "sgx_fir_taps", "sgx_fir_kernel_name", "sgx_fir_device", "sgx_fir_last_error",
    "sgx_deconv_create", "sgx_deconv_destroy", "sgx_deconv_output_length", "sgx_deconv_execute", "sgx_deconv_reserve",
    "sgx_deconv_device", "sgx_deconv_last_error",
    "sgx_minphase_create", "sgx_minphase_destroy", "sgx_minphase_execute", "sgx_minphase_reserve", "sgx_minphase_fft_size",
    "sgx_minphase_output_length", "sgx_minphase_taps", "sgx_minphase_kernel_name", "sgx_minphase_device", "sgx_minphase_last_error",
    "sgx_stream_create", "sgx_stream_destroy", "sgx_stream_step", "sgx_stream_pending", "sgx_stream_frames_emitted", "sgx_stream_flush_frames",
    "sgx_stream_n_bins", "sgx_stream_push", "sgx_stream_flush", "sgx_stream_reset", "sgx_stream_reserve", "sgx_stream_allocations",
    "sgx_stream_kernel_name", "sgx_stream_device", "sgx_stream_last_error",
    "sgx_istream_create", "sgx_istream_destroy", "sgx_istream_step", "sgx_istream_frames_taken", "sgx_istream_samples_emitted",
    "sgx_istream_pending", "sgx_istream_flush_samples", "sgx_istream_push", "sgx_istream_flush", "sgx_istream_reset",
    "sgx_istream_reserve", "sgx_istream_allocations", "sgx_istream_kernel_name", "sgx_istream_device", "sgx_istream_last_error",
    "sgx_resample_create", "sgx_resample_destroy", "sgx_resample_resample", "sgx_resample_process", "sgx_resample_flush", "sgx_resample_reset",
    "sgx_resample_reserve", "sgx_resample_step", "sgx_resample_out_len", "sgx_resample_up", "sgx_resample_down", "sgx_resample_taps_per_phase",
    "sgx_resample_taps", "sgx_resample_phase_offsets", "sgx_resample_tile", "sgx_resample_consumed", "sgx_resample_emitted",
    "sgx_resample_allocations", "sgx_resample_kernel_name", "sgx_resample_device", "sgx_resample_last_error",
    "sgx_welch_create", "sgx_welch_destroy", "sgx_welch_n_bins", "sgx_welch_n_segments", "sgx_welch_frequencies", "sgx_welch_window",
    "sgx_welch_scale", "sgx_welch_execute", "sgx_welch_reserve", "sgx_welch_allocations", "sgx_welch_tile", "sgx_welch_kernel_name",
    "sgx_welch_device", "sgx_welch_last_error",
]


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
    vp, sz = C.c_void_p, C.c_size_t
    L.sgx_plan_create.argtypes = [C.POINTER(SgxParams), C.POINTER(vp)]
    L.sgx_plan_destroy.argtypes = [vp]
    L.sgx_plan_destroy.restype = None
    L.sgx_output_shape.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(sz)]
    L.sgx_execute.argtypes = [vp, vp, sz, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_execute_timed.argtypes = [vp, vp, sz, sz, sz, vp, sz, vp, C.c_int32, C.POINTER(C.c_float)]
    L.sgx_axes.argtypes = [vp, sz, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.sgx_r2c.argtypes = [vp, vp, sz, vp, sz]
    L.sgx_c2r.argtypes = [vp, vp, sz, vp, sz]
    L.sgx_istft_length.argtypes = [vp, sz, C.POINTER(sz)]
    L.sgx_istft.argtypes = [vp, vp, sz, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_window.argtypes = [vp, C.POINTER(C.c_double)]
    L.sgx_mel_weights.argtypes = [vp, C.POINTER(sz), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    L.sgx_shard_range.argtypes = [sz, C.c_int32, C.c_int32, C.POINTER(sz), C.POINTER(sz)]
    L.sgx_last_error.argtypes = [vp]
    L.sgx_last_error.restype = C.c_char_p
    L.sgx_last_create_error.restype = C.c_char_p
    L.sgx_kernel_name.argtypes = [vp]
    L.sgx_kernel_name.restype = C.c_char_p
    L.sgx_istft_kernel_name.argtypes = [vp]
    L.sgx_istft_kernel_name.restype = C.c_char_p
    L.sgx_bank_stage_name.argtypes = [vp]
    L.sgx_bank_stage_name.restype = C.c_char_p
    L.sgx_abi_version.restype = C.c_int32
    L.sgx_device_count.restype = C.c_int32
    L.sgx_fft2d_create.argtypes = [sz, sz, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.sgx_fft2d_destroy.argtypes = [vp]
    L.sgx_fft2d_destroy.restype = None
    L.sgx_fft2d_forward.argtypes = [vp, vp, sz, vp, C.c_int32, vp]
    L.sgx_fft2d_inverse.argtypes = [vp, vp, sz, vp, C.c_int32, vp]
    L.sgx_fft2d_convolve.argtypes = [vp, vp, sz, vp, sz, sz, vp, C.c_int32, vp]
    L.sgx_fft2d_filter.argtypes = [vp, vp, sz, C.c_int32, C.c_double, C.c_double, vp, C.c_int32, vp]
    L.sgx_fft2d_last_error.argtypes = [vp]
    L.sgx_fft2d_last_error.restype = C.c_char_p
    L.sgx_fft2d_reserve.argtypes = [vp, sz, C.c_int32]
    L.sgx_fft2d_device.argtypes = [vp]
    L.sgx_fft2d_device.restype = C.c_int32
    L.sgx_fft2d_kernel_name.argtypes = [vp]
    L.sgx_fft2d_kernel_name.restype = C.c_char_p
    L.sgx_reserve.argtypes = [vp, sz, sz, C.c_int32, C.c_int32]
    L.sgx_plan_device.argtypes = [vp]
    L.sgx_plan_device.restype = C.c_int32
    L.sgx_last_dim_mismatch.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    L.sgx_c2c_create.argtypes = [sz, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.sgx_c2c_destroy.argtypes = [vp]
    L.sgx_c2c_destroy.restype = None
    L.sgx_c2c_forward.argtypes = [vp, vp, sz]
    L.sgx_c2c_inverse.argtypes = [vp, vp, sz]
    L.sgx_c2c_last_error.argtypes = [vp]
    L.sgx_c2c_last_error.restype = C.c_char_p
    L.sgx_comm_unique_id.argtypes = [vp]
    L.sgx_comm_create.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.sgx_comm_adopt.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.sgx_comm_destroy.argtypes = [vp]
    L.sgx_comm_destroy.restype = None
    L.sgx_comm_last_error.argtypes = [vp]
    L.sgx_comm_last_error.restype = C.c_char_p
    L.sgx_gather.argtypes = [vp, vp, vp, sz, sz, C.c_int32, vp]
    L.sgx_shard_execute.argtypes = [vp, vp, vp, sz, sz, sz, vp, vp, vp]
    L.sgx_shard_execute_chunked.argtypes = [vp, vp, vp, sz, sz, sz, vp, vp, C.c_int32, vp]
    L.sgx_membench.argtypes = [C.c_int32, sz, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    L.sgx_clock_probe.argtypes = [C.c_int32, C.c_void_p, C.POINTER(C.c_double)]
    L.sgx_clock_probe.restype = C.c_int32
    L.sgx_plan_create_cqt.argtypes = [C.POINTER(SgxParams), C.POINTER(SgxCqtParams), C.POINTER(vp)]
    L.sgx_plan_create_cqt_transform.argtypes = [C.POINTER(SgxParams), C.POINTER(SgxCqtParams), C.POINTER(vp)]
    L.sgx_cqt_set_route.argtypes = [vp, C.c_int32]
    L.sgx_cqt_kernels.argtypes = [vp, C.POINTER(sz), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.sgx_mdct_create.argtypes = [sz, sz, C.c_int32, C.c_double, C.POINTER(C.c_double), C.c_uint32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.sgx_mdct_destroy.argtypes = [vp]
    L.sgx_mdct_destroy.restype = None
    L.sgx_mdct_output_shape.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(sz)]
    L.sgx_mdct_inverse_length.argtypes = [vp, sz, C.POINTER(sz)]
    L.sgx_mdct_forward.argtypes = [vp, vp, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_mdct_inverse.argtypes = [vp, vp, sz, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_mdct_reserve.argtypes = [vp, sz, sz, C.c_int32]
    L.sgx_mdct_window.argtypes = [vp, C.POINTER(C.c_double)]
    L.sgx_mdct_kernel_name.argtypes = [vp, C.c_int32]
    L.sgx_mdct_kernel_name.restype = C.c_char_p
    L.sgx_mdct_device.argtypes = [vp]
    L.sgx_mdct_device.restype = C.c_int32
    L.sgx_mdct_last_error.argtypes = [vp]
    L.sgx_mdct_last_error.restype = C.c_char_p
    L.sgx_binaural_create.argtypes = [C.POINTER(SgxParams), C.POINTER(SgxBinauralParams), C.POINTER(vp)]
    L.sgx_binaural_destroy.argtypes = [vp]
    L.sgx_binaural_destroy.restype = None
    L.sgx_binaural_output_shape.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.sgx_binaural_axes.argtypes = [vp, sz, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.sgx_binaural_execute.argtypes = [vp, vp, vp, sz, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_binaural_histogram.argtypes = [vp, vp, sz, sz, sz, C.c_double, C.c_double, C.c_int32, C.c_int32, vp, sz, C.c_int32, vp]
    L.sgx_binaural_reserve.argtypes = [vp, sz, sz, C.c_int32]
    L.sgx_binaural_kernel_name.argtypes = [vp]
    L.sgx_binaural_kernel_name.restype = C.c_char_p
    L.sgx_binaural_device.argtypes = [vp]
    L.sgx_binaural_device.restype = C.c_int32
    L.sgx_binaural_last_error.argtypes = [vp]
    L.sgx_binaural_last_error.restype = C.c_char_p
    L.sgx_gammatone_create.argtypes = [C.c_double, sz, sz, C.c_uint32, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                       C.c_int32, C.POINTER(vp)]
    L.sgx_gammatone_destroy.argtypes = [vp]
    L.sgx_gammatone_destroy.restype = None
    L.sgx_gammatone_output_shape.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(sz)]
    L.sgx_gammatone_execute.argtypes = [vp, vp, sz, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_gammatone_center_frequencies.argtypes = [vp, C.POINTER(C.c_double)]
    L.sgx_gammatone_coefficients.argtypes = [vp, C.POINTER(C.c_double)]
    L.sgx_gammatone_reserve.argtypes = [vp, sz, sz, C.c_int32]
    L.sgx_gammatone_kernel_name.argtypes = [vp]
    L.sgx_gammatone_kernel_name.restype = C.c_char_p
    L.sgx_gammatone_device.argtypes = [vp]
    L.sgx_gammatone_device.restype = C.c_int32
    L.sgx_gammatone_last_error.argtypes = [vp]
    L.sgx_gammatone_last_error.restype = C.c_char_p
    L.sgx_fir_create.argtypes = [C.POINTER(C.c_double), sz, sz, sz, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.sgx_fir_destroy.argtypes = [vp]
    L.sgx_fir_destroy.restype = None
    L.sgx_fir_process.argtypes = [vp, vp, sz, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_fir_convolve.argtypes = [vp, vp, sz, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_fir_reset.argtypes = [vp, vp]
    L.sgx_fir_reserve.argtypes = [vp, sz, sz, C.c_int32]
    for f in (L.sgx_fir_fft_size, L.sgx_fir_step, L.sgx_fir_taps, L.sgx_deconv_output_length):
        f.argtypes = [vp]
        f.restype = sz
    L.sgx_fir_kernel_name.argtypes = [vp]
    L.sgx_fir_kernel_name.restype = C.c_char_p
    L.sgx_fir_device.argtypes = [vp]
    L.sgx_fir_device.restype = C.c_int32
    L.sgx_fir_last_error.argtypes = [vp]
    L.sgx_fir_last_error.restype = C.c_char_p
    L.sgx_deconv_create.argtypes = [sz, sz, C.c_double, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.sgx_deconv_destroy.argtypes = [vp]
    L.sgx_deconv_destroy.restype = None
    L.sgx_deconv_execute.argtypes = [vp, vp, vp, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_deconv_reserve.argtypes = [vp, sz, sz, C.c_int32]
    L.sgx_deconv_device.argtypes = [vp]
    L.sgx_deconv_device.restype = C.c_int32
    L.sgx_deconv_last_error.argtypes = [vp]
    L.sgx_deconv_last_error.restype = C.c_char_p
    L.sgx_minphase_create.argtypes = [sz, sz, sz, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.sgx_minphase_destroy.argtypes = [vp]
    L.sgx_minphase_destroy.restype = None
    L.sgx_minphase_execute.argtypes = [vp, vp, sz, vp, sz, C.c_int32, vp]
    L.sgx_minphase_reserve.argtypes = [vp, sz, C.c_int32]
    for f in (L.sgx_minphase_fft_size, L.sgx_minphase_output_length, L.sgx_minphase_taps):
        f.argtypes = [vp]
        f.restype = sz
    L.sgx_minphase_kernel_name.argtypes = [vp]
    L.sgx_minphase_kernel_name.restype = C.c_char_p
    L.sgx_minphase_device.argtypes = [vp]
    L.sgx_minphase_device.restype = C.c_int32
    L.sgx_minphase_last_error.argtypes = [vp]
    L.sgx_minphase_last_error.restype = C.c_char_p
    L.sgx_stream_create.argtypes = [C.POINTER(SgxParams), C.POINTER(vp)]
    L.sgx_stream_destroy.argtypes = [vp]
    L.sgx_stream_destroy.restype = None
    L.sgx_stream_step.argtypes = [vp, sz, sz, C.POINTER(sz), C.POINTER(sz)]
    L.sgx_stream_flush_frames.argtypes = [vp, C.POINTER(sz)]
    for f in (L.sgx_stream_pending, L.sgx_stream_frames_emitted, L.sgx_stream_n_bins, L.sgx_stream_allocations):
        f.argtypes = [vp]
        f.restype = sz
    L.sgx_stream_push.argtypes = [vp, vp, sz, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_stream_flush.argtypes = [vp, vp, sz, C.c_int32, vp]
    L.sgx_stream_reset.argtypes = [vp, vp]
    L.sgx_stream_reserve.argtypes = [vp, sz, sz, C.c_int32]
    L.sgx_stream_kernel_name.argtypes = [vp]
    L.sgx_stream_kernel_name.restype = C.c_char_p
    L.sgx_stream_device.argtypes = [vp]
    L.sgx_stream_device.restype = C.c_int32
    L.sgx_stream_last_error.argtypes = [vp]
    L.sgx_stream_last_error.restype = C.c_char_p
    L.sgx_istream_create.argtypes = [C.POINTER(SgxParams), C.POINTER(vp)]
    L.sgx_istream_destroy.argtypes = [vp]
    L.sgx_istream_destroy.restype = None
    L.sgx_istream_step.argtypes = [vp, sz, sz, C.POINTER(sz)]
    L.sgx_istream_flush_samples.argtypes = [vp, C.POINTER(sz)]
    for f in (L.sgx_istream_frames_taken, L.sgx_istream_samples_emitted, L.sgx_istream_pending, L.sgx_istream_allocations):
        f.argtypes = [vp]
        f.restype = sz
    L.sgx_istream_push.argtypes = [vp, vp, sz, sz, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_istream_flush.argtypes = [vp, vp, sz, C.c_int32, vp]
    L.sgx_istream_reset.argtypes = [vp, vp]
    L.sgx_istream_reserve.argtypes = [vp, sz, sz, C.c_int32]
    L.sgx_istream_kernel_name.argtypes = [vp]
    L.sgx_istream_kernel_name.restype = C.c_char_p
    L.sgx_istream_device.argtypes = [vp]
    L.sgx_istream_device.restype = C.c_int32
    L.sgx_istream_last_error.argtypes = [vp]
    L.sgx_istream_last_error.restype = C.c_char_p
    L.sgx_resample_create.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(vp)]
    L.sgx_resample_destroy.argtypes = [vp]
    L.sgx_resample_destroy.restype = None
    L.sgx_resample_resample.argtypes = [vp, vp, sz, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_resample_process.argtypes = [vp, vp, sz, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_resample_flush.argtypes = [vp, vp, sz, C.c_int32, vp]
    L.sgx_resample_reset.argtypes = [vp, vp]
    L.sgx_resample_reserve.argtypes = [vp, sz, sz, C.c_int32]
    L.sgx_resample_step.argtypes = [vp, sz, sz, C.POINTER(sz), C.POINTER(sz)]
    L.sgx_resample_out_len.argtypes = [vp, sz]
    L.sgx_resample_out_len.restype = sz
    for f in (L.sgx_resample_up, L.sgx_resample_down, L.sgx_resample_taps_per_phase, L.sgx_resample_tile, L.sgx_resample_consumed,
              L.sgx_resample_emitted, L.sgx_resample_allocations):
        f.argtypes = [vp]
        f.restype = sz
    L.sgx_resample_taps.argtypes = [vp, C.POINTER(C.c_double)]
    L.sgx_resample_phase_offsets.argtypes = [vp, C.POINTER(C.c_int64)]
    L.sgx_resample_kernel_name.argtypes = [vp]
    L.sgx_resample_kernel_name.restype = C.c_char_p
    L.sgx_resample_device.argtypes = [vp]
    L.sgx_resample_device.restype = C.c_int32
    L.sgx_resample_last_error.argtypes = [vp]
    L.sgx_resample_last_error.restype = C.c_char_p
    L.sgx_welch_create.argtypes = [C.POINTER(SgxParams), C.c_int32, C.c_int32, C.c_int32, C.c_int32, sz, C.POINTER(vp)]
    L.sgx_welch_destroy.argtypes = [vp]
    L.sgx_welch_destroy.restype = None
    for f in (L.sgx_welch_n_bins, L.sgx_welch_allocations, L.sgx_welch_tile):
        f.argtypes = [vp]
        f.restype = sz
    L.sgx_welch_n_segments.argtypes = [vp, sz]
    L.sgx_welch_n_segments.restype = sz
    L.sgx_welch_frequencies.argtypes = [vp, C.POINTER(C.c_double)]
    L.sgx_welch_window.argtypes = [vp, C.POINTER(C.c_double)]
    L.sgx_welch_scale.argtypes = [vp]
    L.sgx_welch_scale.restype = C.c_double
    L.sgx_welch_execute.argtypes = [vp, vp, vp, sz, sz, sz, vp, sz, C.c_int32, vp]
    L.sgx_welch_reserve.argtypes = [vp, sz, sz, C.c_int32]
    L.sgx_welch_kernel_name.argtypes = [vp]
    L.sgx_welch_kernel_name.restype = C.c_char_p
    L.sgx_welch_device.argtypes = [vp]
    L.sgx_welch_device.restype = C.c_int32
    L.sgx_welch_last_error.argtypes = [vp]
    L.sgx_welch_last_error.restype = C.c_char_p
    _lib = L
    return L


def np_dtype(code: int):
    """numpy type of a dtype code (F32 / F64)."""
    return np.float32 if code == F32 else np.float64


class NativeHandle:
    """One opaque plan of a satellite family of the C ABI.  A subclass names the family's symbol prefix (`_prefix`, e.g. "sgx_mdct"),
    sets `_lib` and `_dt` (the plan's dtype code) and passes its create call's status and handle to `_create`; every later status
    goes through `_check`.  Creation errors are read from <prefix>_last_error(NULL), call errors from the plan."""

    _prefix = ""
    _h = None

    def _last_error(self, handle) -> str:
        return (getattr(self._lib, self._prefix + "_last_error")(handle) or b"").decode()

    def _create(self, status: int, handle) -> None:
        if status:
            raise _ERR.get(status, InternalError)(self._last_error(None))
        self._h = handle

    def _check(self, status: int) -> None:
        if status:
            raise _ERR.get(status, InternalError)(self._last_error(self._h))

    def __del__(self):
        if self._h:
            getattr(self._lib, self._prefix + "_destroy")(self._h)
            self._h = None

    @property
    def _np(self):
        return np_dtype(self._dt)

    @property
    def _tdt(self):
        import torch
        return torch.float32 if self._dt == F32 else torch.float64


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
