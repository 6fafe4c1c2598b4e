"""spectrograms_amd — MI355X (gfx950) engine for the batched STFT / Mel-spectrogram hot path of the
`spectrograms` crate, behind the reference's own parameter / plan / function names.

The compute path is hand-written HIP in libspectro_hip.so reached through the C ABI of
include/spectro_hip.h.  There is no CPU fallback: if the library is not built, or no HIP device is present,
compute calls raise FFTBackendError.
"""
from ._ffi import DimensionMismatchError, FFTBackendError, InternalError, InvalidInputError, SpectrogramError
from .binaural import (BinauralPlan, ILDSpectrogramParams, ILRSpectrogramParams, IPDSpectrogramParams, ITDSpectrogramParams,
                       IldSpectrogram, IlrSpectrogram, IpdSpectrogram, ItdSpectrogram, compute_ild_spectrogram, compute_ilr_spectrogram,
                       compute_ilr_spectrogram_diff, compute_ipd_spectrogram, compute_itd_spectrogram, compute_itd_spectrogram_diff)
from .cqt import CqtResult, CqtTransformPlan, cqt
from .fft2d import (C2cPlan, Fft2dPlan, Fft2dPlanner, bandpass_filter, convolve_fft, detect_edges_fft, fft2d, fftfreq, fftshift,
                    fftshift_1d, gaussian_kernel_2d, highpass_filter, ifft2d, ifftshift, ifftshift_1d, lowpass_filter,
                    magnitude_spectrum_2d, power_spectrum_2d, rfftfreq, sharpen_fft)
from .functions import (clear_fft_plan_cache, compute_chromagram, compute_cqt_db_spectrogram,
                        compute_cqt_magnitude_spectrogram, compute_cqt_power_spectrogram, compute_erb_db_spectrogram,
                        compute_erb_magnitude_spectrogram, compute_erb_power_spectrogram, compute_fft, compute_irfft,
                        compute_istft, compute_linear_db_spectrogram, compute_linear_magnitude_spectrogram,
                        compute_linear_power_spectrogram, compute_loghz_db_spectrogram,
                        compute_loghz_magnitude_spectrogram, compute_loghz_power_spectrogram,
                        compute_magnitude_spectrum, compute_mel_db_spectrogram, compute_mel_magnitude_spectrogram,
                        compute_mel_power_spectrogram, compute_mfcc, compute_power_spectrum, compute_rfft, compute_stft,
                        fft_plan_cache_info)
from .gammatone import GammatonePlan, gammatone_center_frequencies, gammatone_iir_spectrogram
from .fir import DeconvPlan, FirPlan, OverlapSaveConvolver, fft_convolve, fft_deconvolve
from .iir import (IirPlan, allpass_biquad, bandpass_biquad, bandreject_biquad, biquad, deemphasis_sos, equalizer_biquad, highpass_biquad,
                  lowpass_biquad, preemphasis_sos, sosfilt, sosfilt_zi, sosfiltfilt)
from .kaldi import KaldiParams, KaldiPlan, kaldi_fbank, kaldi_mfcc
from .mdct import MdctParams, MdctPlan, imdct, mdct
from .minphase import MinPhasePlan, minimum_phase, minimum_phase_with
from .params import (ChromaNorm, ChromaParams, CqtParams, ErbParams, GammatoneParams, LogHzParams, LogParams, MelNorm, MelParams,
                     MfccParams, SpectrogramParams, StftParams, WindowType)
from .resample import ResamplePlan, resample
from .source import ChromaSource, CqtSource, GammatoneSource, MfccSource
from .planner import Chromagram, Mfcc, Plan, Spectrogram, SpectrogramBatch, SpectrogramPlanner, StftResult
from .streaming import StreamingInversePlan, StreamingPlan
from .welch import WelchParams, WelchPlan, coherence, csd, welch

# The reference exposes one plan class per (frequency scale, amplitude scale) (python/spectrograms/__init__.pyi:1087-1245);
# here they are one class parameterised at construction, exported under the same names.
LinearPowerPlan = LinearMagnitudePlan = LinearDbPlan = Plan
MelPowerPlan = MelMagnitudePlan = MelDbPlan = Plan
ErbPowerPlan = ErbMagnitudePlan = ErbDbPlan = Plan
LogHzPowerPlan = LogHzMagnitudePlan = LogHzDbPlan = Plan
CqtPowerPlan = CqtMagnitudePlan = CqtDbPlan = Plan

__all__ = [
    "SpectrogramError", "InvalidInputError", "DimensionMismatchError", "FFTBackendError", "InternalError",
    "WindowType", "StftParams", "SpectrogramParams", "MelParams", "MelNorm", "LogParams", "SpectrogramPlanner",
    "Plan", "Spectrogram", "StftResult", "compute_linear_power_spectrogram", "compute_linear_magnitude_spectrogram",
    "compute_linear_db_spectrogram", "compute_mel_power_spectrogram", "compute_mel_magnitude_spectrogram",
    "compute_mel_db_spectrogram", "compute_stft", "compute_mfcc", "MfccParams", "Mfcc", "clear_fft_plan_cache",
    "fft_plan_cache_info", "compute_fft", "compute_rfft", "compute_power_spectrum", "compute_magnitude_spectrum",
    "compute_chromagram", "ChromaParams", "ChromaNorm", "Chromagram", "SpectrogramBatch", "compute_irfft",
    "compute_istft", "ErbParams", "GammatoneParams", "compute_erb_power_spectrogram",
    "compute_erb_magnitude_spectrogram", "compute_erb_db_spectrogram", "LogHzParams",
    "compute_loghz_power_spectrogram", "compute_loghz_magnitude_spectrogram", "compute_loghz_db_spectrogram",
    "fft2d", "ifft2d", "C2cPlan", "Fft2dPlan", "Fft2dPlanner", "convolve_fft", "gaussian_kernel_2d", "lowpass_filter",
    "highpass_filter", "bandpass_filter", "detect_edges_fft", "sharpen_fft", "power_spectrum_2d",
    "magnitude_spectrum_2d", "fftshift", "ifftshift", "fftfreq", "rfftfreq", "fftshift_1d", "ifftshift_1d",
    "LinearPowerPlan", "LinearMagnitudePlan", "LinearDbPlan", "MelPowerPlan", "MelMagnitudePlan", "MelDbPlan",
    "ErbPowerPlan", "ErbMagnitudePlan", "ErbDbPlan", "LogHzPowerPlan", "LogHzMagnitudePlan", "LogHzDbPlan",
    "CqtParams", "compute_cqt_power_spectrogram", "compute_cqt_magnitude_spectrogram", "compute_cqt_db_spectrogram",
    "CqtPowerPlan", "CqtMagnitudePlan", "CqtDbPlan", "MdctParams", "MdctPlan", "mdct", "imdct",
    "ITDSpectrogramParams", "IPDSpectrogramParams", "ILDSpectrogramParams", "ILRSpectrogramParams", "ItdSpectrogram", "IpdSpectrogram",
    "IldSpectrogram", "IlrSpectrogram", "BinauralPlan", "compute_itd_spectrogram", "compute_ipd_spectrogram", "compute_ild_spectrogram",
    "compute_ilr_spectrogram", "compute_itd_spectrogram_diff", "compute_ilr_spectrogram_diff",
    "GammatonePlan", "gammatone_iir_spectrogram", "gammatone_center_frequencies",
    "FirPlan", "OverlapSaveConvolver", "DeconvPlan", "fft_convolve", "fft_deconvolve",
    "MinPhasePlan", "minimum_phase", "minimum_phase_with",
    "cqt", "CqtResult", "CqtTransformPlan", "GammatoneSource", "CqtSource", "ChromaSource", "MfccSource",
    "StreamingPlan", "StreamingInversePlan", "ResamplePlan", "resample",
    "WelchParams", "WelchPlan", "welch", "csd", "coherence",
    "KaldiParams", "KaldiPlan", "kaldi_fbank", "kaldi_mfcc",
    "IirPlan", "sosfilt", "sosfiltfilt", "sosfilt_zi", "biquad", "lowpass_biquad", "highpass_biquad", "bandpass_biquad",
    "bandreject_biquad", "allpass_biquad", "equalizer_biquad", "preemphasis_sos", "deemphasis_sos",
]
