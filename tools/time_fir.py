"""Times the streaming FIR plans (fir.hip) on the device: one JSON line per (taps, route, dtype) with the kernel, us per call, samples
per second, S / P, and the fraction of 8 TB/s that the algorithmic bytes imply (x read once, y written once).

Shape: 256 rows x 10 s at 48 kHz, one impulse response for all rows, device-resident, f32 and f64, the streaming form (process):
taps 128, 512, 2048 on the fused route (k_fir_os) and 8192 on the generic one; with --generic also 128 / 512 / 2048 on the generic
route.  Each case is timed with device events around back-to-back calls on one stream, after a warm-up, over at least 1 s of calls.

    python tools/time_fir.py [--generic]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES = 8.0e12


def time_call(fn, torch):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        fn()
    e1.record()
    e1.synchronize()
    per = e0.elapsed_time(e1) / 3 * 1e-3
    iters = max(10, int(1.0 / max(per, 1e-6)) + 1)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3, iters


def main():
    import numpy as np
    import torch

    import spectrograms_amd as sg
    torch.cuda.set_device(0)
    batch, n = 256, 480000
    cases = [(128, "auto"), (512, "auto"), (2048, "auto"), (8192, "auto")]
    if "--generic" in sys.argv:
        cases += [(128, "generic"), (512, "generic"), (2048, "generic")]
    rng = np.random.default_rng(0)
    for dtype in ("float32", "float64"):
        tdt = torch.float32 if dtype == "float32" else torch.float64
        x = torch.randn(batch, n, dtype=tdt, device="cuda")
        out = torch.empty_like(x)
        for taps, route in cases:
            ir = rng.standard_normal(taps) * np.exp(-np.arange(taps) / (taps / 4.0))
            plan = sg.FirPlan(ir, dtype=dtype, route=route)
            plan.reserve(batch, n, host_staging=False)
            s, iters = time_call(lambda: plan.process_torch(x, out), torch)
            nbytes = 2 * batch * n * x.element_size()
            print(json.dumps({"taps": taps, "route": route, "dtype": dtype, "batch": batch, "n_samples": n, "kernel": plan.kernel_name,
                              "fft_size": plan.fft_size, "step": plan.step, "s_over_p": round(plan.step / plan.fft_size, 3),
                              "us": round(s * 1e6, 1), "iters": iters, "samples_per_s": round(batch * n / s, 1),
                              "algorithmic_bytes": nbytes, "frac_8tbs": round(nbytes / s / PEAK_BYTES, 4)}), flush=True)
            del plan
        del x, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
