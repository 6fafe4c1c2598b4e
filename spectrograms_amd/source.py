"""Representation-agnostic feature sources: the SpectrogramSource trait of the reference (src/source.rs:39-350), "a thing that
turns a mono signal into an [n_bands x n_frames] matrix".

Every source has `compute_matrix(samples)`, `n_bands`, `center_frequencies()`, `sample_rate` and `hop_seconds`.  Every spectrogram
`Plan` is one (planner.py); the four classes here are the reference's other implementors.  Each runs exactly the launches of the
one-shot function it names (on that function's cached plan), so its matrix is that function's `data` bit for bit.  Beyond the
reference, `compute_matrix` also takes a (batch, n) array and returns a leading batch axis, and a `dtype` ("float32" / "float64",
default float64) chooses T as for the one-shot functions.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _ffi
from .cqt import MAX_KERNEL_LENGTH, transform_plan
from .planner import signal_length
from .params import ChromaParams, CqtParams, ErbParams, LogParams, MelParams, MfccParams, SpectrogramParams, StftParams

N_CHROMA = 12


def _matrix(plan, samples):
    """`samples` (n,) or (batch, n) through a Plan's batched call."""
    x = np.asarray(samples)
    return plan.compute_batch(x[None])[0] if x.ndim == 1 else plan.compute_batch(x)


class _Source:
    def __init__(self, sample_rate: float, hop_size: int, dtype: Optional[str]):
        if int(hop_size) <= 0:
            raise ValueError("hop_size must be > 0")  # NonZeroUsize
        self.sample_rate, self._hop, self._dtype = float(sample_rate), int(hop_size), dtype

    @property
    def hop_seconds(self) -> float:
        return self._hop / self.sample_rate


class GammatoneSource(_Source):
    """GammatoneSource (src/source.rs:95-166): the time-domain IIR gammatone bank, `gammatone_iir_spectrogram`.  A dB floor on the
    ErbParams gives decibel output."""

    def __init__(self, sample_rate: float, frame_size: int, hop_size: int, erb_params: ErbParams, dtype: Optional[str] = None):
        if not isinstance(erb_params, ErbParams):
            raise TypeError("erb_params must be an ErbParams")
        if int(frame_size) <= 0:
            raise ValueError("frame_size must be > 0")
        super().__init__(sample_rate, hop_size, dtype)
        self.frame_size, self.params = int(frame_size), erb_params

    @property
    def n_bands(self) -> int:
        return self.params.n_filters

    def center_frequencies(self) -> list:
        from .gammatone import gammatone_center_frequencies
        return gammatone_center_frequencies(self.params).tolist()

    def compute_matrix(self, samples):
        from .gammatone import _plan
        signal_length(samples)
        return _plan(self.sample_rate, self.frame_size, self._hop, self.params, self._dtype).compute(samples)


class CqtSource(_Source):
    """CqtSource (src/source.rs:168-228): cqt(...).to_magnitude().  The magnitude is formed in the kernel's epilogue (a transform
    plan with magnitude output): the complex tensor is never written."""

    def __init__(self, sample_rate: float, hop_size: int, cqt_params: CqtParams, dtype: Optional[str] = None):
        if not isinstance(cqt_params, CqtParams):
            raise TypeError("cqt_params must be a CqtParams")
        super().__init__(sample_rate, hop_size, dtype)
        self.params = cqt_params

    def center_frequencies(self) -> list:
        """The bins below Nyquist (:213-219)."""
        nyquist = self.sample_rate / 2.0
        return [f for f in self.params.frequencies() if f < nyquist]

    @property
    def n_bands(self) -> int:
        return len(self.center_frequencies())

    def compute_matrix(self, samples):
        n = signal_length(samples)
        plan = transform_plan(self.sample_rate, min(n, MAX_KERNEL_LENGTH), self._hop, self.params, _ffi.AMP_MAGNITUDE, None, self._dtype)
        return _matrix(plan, samples)


class ChromaSource(_Source):
    """ChromaSource (src/source.rs:230-287): `compute_chromagram`, 12 pitch classes; the centre frequencies are those of the lowest
    octave, f_min 2^(i / 12)."""

    def __init__(self, sample_rate: float, stft_params: StftParams, chroma_params: ChromaParams, dtype: Optional[str] = None):
        super().__init__(sample_rate, stft_params.hop_size, dtype)
        self.stft_params, self.params = stft_params, chroma_params

    n_bands = property(lambda s: N_CHROMA)

    def center_frequencies(self) -> list:
        return [self.params.f_min * 2.0 ** (i / N_CHROMA) for i in range(N_CHROMA)]

    def compute_matrix(self, samples):
        from .functions import Plan
        signal_length(samples)
        return _matrix(Plan(SpectrogramParams(self.stft_params, self.sample_rate), _ffi.AMP_MAGNITUDE, self.params, None, self._dtype), samples)


class MfccSource(_Source):
    """MfccSource (src/source.rs:289-350): `compute_mfcc`; n_mfcc bands whose "centre frequencies" are the indices 0.0, 1.0, ..."""

    def __init__(self, sample_rate: float, stft_params: StftParams, n_mels: int, mfcc_params: MfccParams, dtype: Optional[str] = None):
        if int(n_mels) <= 0:
            raise ValueError("n_mels must be > 0")
        super().__init__(sample_rate, stft_params.hop_size, dtype)
        self.stft_params, self.n_mels, self.params = stft_params, int(n_mels), mfcc_params

    @property
    def n_bands(self) -> int:
        return self.params.n_mfcc

    def center_frequencies(self) -> list:
        return [float(i) for i in range(self.params.n_mfcc)]

    def compute_matrix(self, samples):
        from .functions import Plan
        signal_length(samples)
        params = SpectrogramParams(self.stft_params, self.sample_rate)
        return _matrix(Plan(params, _ffi.AMP_DECIBELS, MelParams(self.n_mels, 0.0, self.sample_rate / 2.0), LogParams(-80.0), self._dtype,
                            mfcc=self.params), samples)


__all__ = ["GammatoneSource", "CqtSource", "ChromaSource", "MfccSource"]
