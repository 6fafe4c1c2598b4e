"""GPU tests of the checks that stand between a caller's tensor and a kernel that trusts its pointer (spectrograms_amd/_handle.py),
through every stateless torch entry of the plan families.

Per entry: one valid call; every rejected input and `out` raises its class and launches nothing; the valid call repeated on the same
plan gives the same bits; and the families that take a row stride give, on a slice `big[:, 3:3 + n]` at batch 2 and at batch 1, the
bits of the call on the contiguous copy (the one stride rule at its b == 1 corner).  The shapes are the smallest each tuned kernel
accepts: these are rejections and tiny valid calls.
"""
import numpy as np
import pytest
import torch

import spectrograms_amd as sg

pytestmark = pytest.mark.gpu

B = 2
SPEC = sg.SpectrogramParams(sg.StftParams(256, 64, sg.WindowType.hanning, True), 16000.0)


def noise(*shape, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).cuda()


class Entry:
    """One torch entry: `make()` the plan, `inputs()` its valid device tensors (the first is the one the cases vary), `call(plan, ins,
    out)`; `strided`: the C entry takes a row stride; `shape_error`: the class a wrong rank or an empty batch of the input raises."""

    def __init__(self, name, make, inputs, call, kernel, strided=False, shape_error=ValueError):
        self.name, self.make, self.inputs, self.call, self.kernel = name, make, inputs, call, kernel
        self.strided, self.shape_error = strided, shape_error


ENTRIES = [
    Entry("fir.convolve", lambda: sg.FirPlan(np.hanning(8), dtype="float32"), lambda: [noise(B, 300)],
          lambda p, ins, out: p.convolve_torch(ins[0], out), "k_fir_os"),
    Entry("mdct.forward", lambda: sg.MdctPlan(sg.MdctParams.sine_window(64), "float32"), lambda: [noise(B, 320)],
          lambda p, ins, out: p.forward_torch(ins[0], out), "k_mdct_fwd"),
    Entry("minphase.execute", lambda: sg.MinPhasePlan(16, dtype="float32"), lambda: [noise(B, 16)],
          lambda p, ins, out: p.execute_torch(ins[0], out), "k_minphase"),
    Entry("deconv.execute", lambda: sg.DeconvPlan(300, 8, 1e-3, "float32"), lambda: [noise(B, 300), noise(1, 8, seed=1)],
          lambda p, ins, out: p.execute_torch(ins[0], ins[1], out), None),
    Entry("gammatone.compute", lambda: sg.GammatonePlan(16000.0, 64, 16, sg.ErbParams(8, 50.0, 4000.0), "float32"), lambda: [noise(B, 400)],
          lambda p, ins, out: p.compute_torch(ins[0], out), "k_gammatone_iir", strided=True),
    Entry("binaural.compute", lambda: sg.BinauralPlan(sg.ILDSpectrogramParams(SPEC), "float32"), lambda: [noise(B, 512), noise(B, 512, seed=1)],
          lambda p, ins, out: p.compute_torch(ins[0], ins[1], out), None),
    Entry("resample.resample", lambda: sg.ResamplePlan(3, 2, dtype="float32"), lambda: [noise(B, 300)],
          lambda p, ins, out: p.resample_torch(ins[0], out), "k_resample_pp", strided=True),
    Entry("welch.compute", lambda: sg.WelchPlan(sg.WelchParams(256, 128), "psd", "float32"), lambda: [noise(B, 512)],
          lambda p, ins, out: p.compute_torch(ins[0], None, out), "k_welch", strided=True),
    Entry("fft2d.forward", lambda: sg.Fft2dPlan(64, 64, "float32"), lambda: [noise(B, 64, 64)],
          lambda p, ins, out: p.forward_torch(ins[0], out), None, shape_error=sg.DimensionMismatchError),
]


def bits(t) -> bytes:
    return t.cpu().numpy().tobytes()


def widened(x):
    """`x` as a slice `big[..., 3:3 + n]` of a wider tensor: the same values, unit inner stride, a row stride of n + 13."""
    big = torch.zeros(tuple(x.shape[:-1]) + (x.shape[-1] + 13,), dtype=x.dtype, device=x.device)
    big[..., 3:3 + x.shape[-1]] = x
    return big[..., 3:3 + x.shape[-1]]


@pytest.mark.parametrize("e", ENTRIES, ids=[e.name for e in ENTRIES])
def test_gpu_rejected_inputs_raise_and_leave_the_plan_as_it_was(e):
    plan, ins = e.make(), e.inputs()
    if e.kernel is not None:
        name = plan.kernel_name
        assert (name() if callable(name) else name) == e.kernel  # the tuned route at its smallest shape
    x = ins[0]
    first = e.call(plan, ins, None)
    want = bits(first)

    def with_x(t):
        return [t] + ins[1:]

    # ---- the input: dtype, layout, rank, batch
    bad_inputs = [("wrong dtype", x.double(), ValueError),
                  ("transposed", x.transpose(-1, -2).contiguous().transpose(-1, -2), ValueError),
                  ("wrong rank", x[0], e.shape_error),
                  ("zero batch", x[:0], e.shape_error)]
    if not e.strided:
        bad_inputs.append(("strided rows", widened(x), ValueError))
    for what, t, err in bad_inputs:
        assert what in ("wrong dtype", "wrong rank", "zero batch") or (tuple(t.shape) == tuple(x.shape) and not t.is_contiguous()), what
        with pytest.raises(err):
            e.call(plan, with_x(t), None)
    # ---- out: shape, dtype, layout
    shape = tuple(first.shape)
    longer = shape[:-1] + (shape[-1] + 1,)
    bad_outs = [("wrong shape", torch.empty(longer, dtype=first.dtype, device="cuda"), sg.DimensionMismatchError),
                ("wrong rank", torch.empty(shape + (1,), dtype=first.dtype, device="cuda"), sg.DimensionMismatchError),
                ("wrong dtype", torch.empty(shape, dtype=torch.float64, device="cuda"), ValueError),
                ("non-contiguous", torch.empty(shape[:-1] + (2 * shape[-1],), dtype=first.dtype, device="cuda")[..., ::2], ValueError)]
    for what, out, err in bad_outs:
        assert what != "non-contiguous" or (tuple(out.shape) == shape and not out.is_contiguous())
        with pytest.raises(err) as ei:
            e.call(plan, ins, out)
        if what == "wrong shape":
            assert ei.value.expected == shape and ei.value.got == longer
    # ---- the same plan, the same input, the same path: the same bits, into a new tensor and into `out`
    assert bits(e.call(plan, ins, None)) == want
    out = torch.full(shape, float("nan"), dtype=first.dtype, device="cuda")
    assert e.call(plan, ins, out) is out and bits(out) == want


STRIDED = [e for e in ENTRIES if e.strided]


@pytest.mark.parametrize("batch", [2, 1])
@pytest.mark.parametrize("e", STRIDED, ids=[e.name for e in STRIDED])
def test_gpu_strided_rows_give_the_bits_of_the_contiguous_copy(e, batch):
    """`big[:, 3:3 + n]`: at batch 2 the row stride is the tensor's, at batch 1 torch calls the slice contiguous and the stride handed to
    the kernel is n."""
    plan = e.make()
    x = e.inputs()[0][:batch].contiguous()
    sliced = widened(x)
    assert sliced.data_ptr() != x.data_ptr() and sliced.stride(0) == x.shape[1] + 13 and sliced.is_contiguous() == (batch == 1)
    want = bits(e.call(plan, [x], None))
    assert bits(e.call(plan, [sliced], None)) == want
    assert bits(e.call(plan, [x], None)) == want
