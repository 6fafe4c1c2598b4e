"""The feature sources (SpectrogramSource, src/source.rs:39-350): metadata against the trait's formulas on the CPU; on the GPU each
source's matrix against the one-shot function it stands for — the same launches on the same cached plan, so the same bits — and
CqtSource against the restatement of tests/test_cqt_transform.py within the magnitude bound of tests/test_cqt.py."""
import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests.test_cqt import check_output, signals

HOST = _ffi.DEVICE_HOST_ONLY
NP = {"float32": np.float32, "float64": np.float64}
SR = 16000.0
STFT = sg.StftParams(1024, 256, sg.WindowType.hanning, True)


def sources():
    return [sg.GammatoneSource(SR, 400, 160, sg.ErbParams(32, 50.0, 7000.0)), sg.CqtSource(SR, 512, sg.CqtParams(12, 9, 55.0)),
            sg.ChromaSource(SR, STFT, sg.ChromaParams()), sg.MfccSource(SR, STFT, 40, sg.MfccParams(13))]


def test_metadata():
    gt, cq, ch, mf = sources()
    assert (gt.n_bands, gt.sample_rate, gt.hop_seconds) == (32, SR, 160 / SR)
    assert np.array_equal(gt.center_frequencies(), sg.gammatone_center_frequencies(sg.ErbParams(32, 50.0, 7000.0)))
    f = sg.CqtParams(12, 9, 55.0).frequencies()
    assert cq.n_bands == 87 and cq.center_frequencies() == f[:87] and f[87] >= SR / 2 and cq.hop_seconds == 512 / SR
    assert sg.CqtSource(SR, 512, sg.CqtParams(1, 2, 4000.0)).n_bands == 1  # f_1 = 8000 = Nyquist is dropped (>=)
    assert sg.CqtSource(SR, 512, sg.CqtParams(12, 7, 32.7)).n_bands == 84
    assert ch.n_bands == 12 and ch.center_frequencies() == [sg.ChromaParams().f_min * 2.0 ** (i / 12) for i in range(12)]
    assert ch.hop_seconds == 256 / SR and ch.sample_rate == SR
    assert mf.n_bands == 13 and mf.center_frequencies() == [float(i) for i in range(13)] and mf.hop_seconds == 256 / SR
    # every spectrogram plan is a source
    params = sg.SpectrogramParams(STFT, SR)
    mel = sg.Plan(params, _ffi.AMP_POWER, sg.MelParams(64, 0.0, 8000.0), None, "float32", device=HOST)
    assert mel.n_bands == 64 and mel.sample_rate == SR and mel.hop_seconds == 256 / SR
    assert mel.center_frequencies() == mel.axes(1)[0].tolist() and len(mel.center_frequencies()) == 64
    lin = sg.Plan(params, _ffi.AMP_MAGNITUDE, None, None, "float64", device=HOST)
    assert lin.n_bands == 513 and lin.center_frequencies()[1] == SR / 1024
    cqp = sg.Plan(params, _ffi.AMP_POWER, sg.CqtParams(12, 7, 32.7), None, "float32", device=HOST)
    assert cqp.n_bands == 84 and np.allclose(cqp.center_frequencies(), sg.CqtParams(12, 7, 32.7).frequencies(), rtol=1e-14, atol=0)
    tp = sg.CqtTransformPlan(SR, 8000, 20000, sg.CqtParams(12, 9, 55.0), device=HOST)
    assert tp.n_bands == 87 and tp.sample_rate == SR and tp.hop_seconds == 20000 / SR


def test_empty_input_text():
    params = sg.SpectrogramParams(STFT, SR)
    plan = sg.Plan(params, _ffi.AMP_POWER, None, None, "float32", device=HOST)
    for src in sources() + [plan]:
        for empty in (np.zeros(0), np.zeros((0, 16)), np.zeros((2, 0))):
            with pytest.raises(sg.InvalidInputError, match="samples must be non-empty"):
                src.compute_matrix(empty)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_gpu_sources_equal_their_functions(dtype):
    x = signals(3, 6000, SR, seed=11).astype(NP[dtype])
    erb = sg.ErbParams(32, 50.0, 7000.0)
    cases = [
        (sg.GammatoneSource(SR, 400, 160, erb, dtype), lambda s: sg.gammatone_iir_spectrogram(s, SR, 400, 160, erb, dtype)[0]),
        (sg.ChromaSource(SR, STFT, sg.ChromaParams(), dtype), lambda s: sg.compute_chromagram(s, STFT, SR, sg.ChromaParams(), dtype).data),
        (sg.MfccSource(SR, STFT, 40, sg.MfccParams(13), dtype), lambda s: sg.compute_mfcc(s, STFT, SR, 40, sg.MfccParams(13), dtype).data),
    ]
    params = sg.SpectrogramParams(STFT, SR)
    for amp, mapping, db in ((_ffi.AMP_DECIBELS, sg.MelParams(64, 0.0, 8000.0), sg.LogParams(-80.0)), (_ffi.AMP_POWER, None, None),
                             (_ffi.AMP_MAGNITUDE, sg.CqtParams(12, 7, 32.7), None)):
        plan = sg.Plan(params, amp, mapping, db, dtype)
        cases.append((plan, lambda s, plan=plan: plan.compute(s).data))
    for src, fn in cases:
        one = src.compute_matrix(x[0])
        assert one.shape[0] == src.n_bands == len(src.center_frequencies()) and one.dtype == NP[dtype]
        assert np.array_equal(one, fn(x[0]), equal_nan=True), type(src).__name__
        many = src.compute_matrix(x)
        assert many.shape == (3,) + one.shape
        for i in range(3):
            assert np.array_equal(many[i], fn(x[i]), equal_nan=True), (type(src).__name__, i)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n", [6000, 16384 + 2 * 512 + 3])
def test_gpu_cqt_source(n, dtype):
    from tests.test_cqt_transform import Kept
    cq, hop = sg.CqtParams(12, 9, 55.0), 512
    src = sg.CqtSource(SR, hop, cq, dtype)
    x = signals(2, n, SR, seed=12)
    klen = min(n, 16384)
    got = src.compute_matrix(x.astype(NP[dtype]))
    assert got.shape == (2, 87, (n - klen) // hop + 1) and got.dtype == NP[dtype] and src.n_bands == 87
    check_output(got, x, Kept(cq, SR), klen, hop, SR, dtype, _ffi.AMP_MAGNITUDE, None, centre=False)
    one = src.compute_matrix(x[1].astype(NP[dtype]))
    assert np.array_equal(one, got[1])
