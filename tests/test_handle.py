"""CPU tests of what the plan families share (spectrograms_amd/_handle.py): the plan cache behind the one-shot functions and the
device check that every torch entry runs before anything else."""
import numpy as np
import pytest
import torch

import spectrograms_amd as sg
from spectrograms_amd import _ffi, _handle

HOST = _ffi.DEVICE_HOST_ONLY


class Counting:
    """A factory that counts its calls and returns a new object each time."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


def test_plan_cache_evicts_the_least_recently_used_of_sixteen():
    cache, make = _ffi.PlanCache(), Counting()
    first = [cache.get(k, make) for k in range(16)]
    assert len(cache) == 16 and make.calls == 16 and list(cache) == list(range(16))
    assert all(cache.get(k, make) is first[k] for k in range(16)) and make.calls == 16  # hits build nothing
    cache.get(16, make)  # the 17th key evicts the first
    assert len(cache) == 16 and make.calls == 17 and 0 not in cache and list(cache) == list(range(1, 17))
    assert cache.get(0, make) is not first[0] and make.calls == 18 and 1 not in cache  # key 0 is built again, key 1 goes


def test_plan_cache_hit_moves_its_key_to_the_back():
    cache, make = _ffi.PlanCache(), Counting()
    first = [cache.get(k, make) for k in range(16)]
    assert cache.get(0, make) is first[0] and list(cache)[-1] == 0  # a hit: most recently used last
    cache.get(16, make)
    assert 0 in cache and 1 not in cache and len(cache) == 16  # so it survives the next eviction; key 1 was the oldest
    assert cache.get(0, make) is first[0] and make.calls == 17
    cache.clear()
    assert len(cache) == 0 and list(cache) == []
    assert cache.get(0, make) is not first[0] and make.calls == 18


def test_clear_fft_plan_cache_reaches_a_cache_made_after_import():
    """The registry, not a list of names: a cache nobody has told clear_fft_plan_cache about is emptied by it."""
    cache, make = _ffi.PlanCache(), Counting()
    other = _ffi.PlanCache(4)
    for k in range(3):
        cache.get(k, make)
        other.get(("x", k), make)
    assert len(cache) == 3 and len(other) == 3
    sg.clear_fft_plan_cache()
    assert len(cache) == 0 and len(other) == 0
    cache.get(0, make)
    assert make.calls == 7


def test_every_family_builds_its_cache_from_the_shared_class():
    import importlib
    held = (("functions", "_PLAN_CACHE"), ("cqt", "_CQT_CACHE"), ("gammatone", "_GT_CACHE"), ("mdct", "_MDCT_CACHE"),
            ("welch", "_WELCH_CACHE"), ("binaural", "_BIN_CACHE"))  # (by module path: the package exports functions named cqt, mdct, welch)
    caches = [getattr(importlib.import_module("spectrograms_amd." + m), name) for m, name in held] + [sg.Fft2dPlanner()._plans]
    assert all(isinstance(c, _ffi.PlanCache) for c in caches)
    assert all(c in _handle._CACHES for c in caches)


class NoCalls:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        def refuse(*args):
            raise AssertionError(f"{name} was called before the tensor was refused")
        return refuse


def _spec(n_fft=64, hop=16):
    return sg.SpectrogramParams(sg.StftParams(n_fft, hop, sg.WindowType.hanning, True), 16000.0)


def _cpu(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


# (family, make the host-only plan, call its torch entry with CPU tensors)
TORCH_ENTRIES = [
    ("fir.convolve", lambda: sg.FirPlan(np.ones(4), dtype="float32", device=HOST), lambda p: p.convolve_torch(_cpu(2, 32))),
    ("fir.process", lambda: sg.FirPlan(np.ones(4), dtype="float32", device=HOST), lambda p: p.process_torch(_cpu(2, 32))),
    ("deconv", lambda: sg.DeconvPlan(32, 4, 0.0, "float32", device=HOST), lambda p: p.execute_torch(_cpu(2, 32), _cpu(1, 4))),
    ("mdct.forward", lambda: sg.MdctPlan(sg.MdctParams.sine_window(16), "float32", device=HOST), lambda p: p.forward_torch(_cpu(2, 64))),
    ("mdct.inverse", lambda: sg.MdctPlan(sg.MdctParams.sine_window(16), "float32", device=HOST), lambda p: p.inverse_torch(_cpu(2, 8, 7))),
    ("minphase", lambda: sg.MinPhasePlan(8, dtype="float32", device=HOST), lambda p: p.execute_torch(_cpu(2, 8))),
    ("gammatone", lambda: sg.GammatonePlan(16000.0, 64, 16, sg.ErbParams(8, 50.0, 4000.0), "float32", device=HOST),
     lambda p: p.compute_torch(_cpu(2, 256))),
    ("binaural", lambda: sg.BinauralPlan(sg.ILDSpectrogramParams(_spec(256, 64)), "float32", device=HOST),
     lambda p: p.compute_torch(_cpu(2, 512), _cpu(2, 512))),
    ("resample.resample", lambda: sg.ResamplePlan(3, 2, dtype="float32", device=HOST), lambda p: p.resample_torch(_cpu(2, 64))),
    ("resample.process", lambda: sg.ResamplePlan(3, 2, dtype="float32", device=HOST), lambda p: p.process_torch(_cpu(2, 64))),
    ("welch", lambda: sg.WelchPlan(sg.WelchParams(64, 32), "psd", "float32", device=HOST), lambda p: p.compute_torch(_cpu(2, 256))),
    ("welch.csd", lambda: sg.WelchPlan(sg.WelchParams(64, 32), "csd", "float32", device=HOST),
     lambda p: p.compute_torch(_cpu(2, 256), _cpu(2, 256))),
    ("stream", lambda: sg.StreamingPlan(_spec(), _ffi.AMP_POWER, dtype="float32", device=HOST), lambda p: p.push(_cpu(2, 100))),
    ("stream.1d", lambda: sg.StreamingPlan(_spec(), _ffi.AMP_POWER, dtype="float32", device=HOST), lambda p: p.push(_cpu(100))),
    ("istream", lambda: sg.StreamingInversePlan(_spec(), "float32", device=HOST), lambda p: p.push(_cpu(2, 33, 4, dtype=torch.complex64))),
    ("fft2d.forward", lambda: sg.Fft2dPlan(8, 8, "float32", device=HOST), lambda p: p.forward_torch(_cpu(2, 8, 8))),
    ("fft2d.inverse", lambda: sg.Fft2dPlan(8, 8, "float32", device=HOST), lambda p: p.inverse_torch(_cpu(2, 8, 5, 2))),
    ("fft2d.convolve", lambda: sg.Fft2dPlan(8, 8, "float32", device=HOST), lambda p: p.convolve_torch(_cpu(2, 8, 8), np.ones((3, 3)))),
    ("fft2d.filter", lambda: sg.Fft2dPlan(8, 8, "float32", device=HOST), lambda p: p.filter_torch(_cpu(2, 8, 8), 0, 0.5)),
]


@pytest.mark.parametrize("name,make,call", TORCH_ENTRIES, ids=[e[0] for e in TORCH_ENTRIES])
def test_torch_entry_refuses_a_cpu_tensor_before_any_library_call(name, make, call):
    """The first check of every torch entry: the tensor lives on the plan's device.  A CPU tensor handed to a host-only plan is a
    ValueError that names the plan's device, raised before the library is called."""
    plan = make()
    assert plan.device == HOST
    lib, plan._lib = plan._lib, NoCalls()
    try:
        with pytest.raises(ValueError, match=r"is on cpu, the plan is bound to cuda:-2"):
            call(plan)
    finally:
        plan._lib = lib  # (the plan is destroyed through it)


def test_cpu_out_tensor_is_refused_like_a_cpu_input():
    """The out-tensor helper runs the same device check (no GPU needed to see it: the input check is what a CPU run reaches first, so
    the helper is called directly)."""
    plan = sg.DeconvPlan(32, 4, 0.0, "float32", device=HOST)
    with pytest.raises(ValueError, match=r"out is on cpu, the plan is bound to cuda:-2"):
        plan._out_tensor(_cpu(2, 32), (2, 32), "cpu")
    assert tuple(plan._out_tensor(None, (2, 32), "cpu").shape) == (2, 32)
