"""Times the IIR plans (iir.hip) on the device against what a caller has without them: one JSON line per case with the route, us per
call, the fraction of 8 TB/s that the algorithmic bytes imply (x read once, y written once), the fraction of the f64 vector rate that
the two passes' operations imply (9 operations per section and sample, twice), and beside it FirPlan on the filter's impulse response
truncated where its tail falls below 2^-24 of its l1 norm (the truncation length is stated).

Cases, device-resident:
    256 rows x 10 s at 48 kHz, f32 and f64, one section (a DC blocker) and four (Butterworth-8 low-pass at 0.01), sosfilt;
    the same rows, four sections, sosfiltfilt;
    4096 streams x 1600-sample pushes, four sections, the streaming form;
    8 rows x 10 min at 48 kHz, four sections, on the split route.
Each case is timed with device events around back-to-back calls on one stream, after a warm-up, over at least 0.25 s of calls.

    python tools/time_iir.py [--no-baseline]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES = 8.0e12
PEAK_F64_VECTOR = 78.6e12  # MI355X vector f64, operations per second
OPS_PER_SECTION = 9        # 5 products, 4 sums

DC_BLOCKER = np.array([[1.0, -1.0, 0.0, 1.0, -0.995, 0.0]])
BUTTER8_LP = np.array([  # scipy.signal.butter(8, 0.01, output="sos")
    [3.4219614165936484e-15, 6.843922833187297e-15, 3.4219614165936484e-15, 1.0, -1.939269633591658, 0.9402270185020654],
    [1.0, 2.0, 1.0, 1.0, -1.9481335385151675, 0.9490952993868512],
    [1.0, 2.0, 1.0, 1.0, -1.9647269019487286, 0.9656968546857874],
    [1.0, 2.0, 1.0, 1.0, -1.9868379069766875, 0.987818775546285],
])


def time_call(fn, torch, min_s=0.25):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        fn()
    e1.record()
    e1.synchronize()
    per = e0.elapsed_time(e1) / 3 * 1e-3
    iters = max(5, int(min_s / max(per, 1e-6)) + 1)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3, iters


def truncated_impulse_response(sos, limit=1 << 19):
    """The impulse response cut where the l1 norm of what follows falls below 2^-24 of the whole (f64 recurrence on the host)."""
    n = 1 << 12
    while True:
        x = np.zeros(n)
        x[0] = 1.0
        z = np.zeros((len(sos), 2))
        h = np.empty(n)
        for t in range(n):
            v = x[t]
            for i, (b0, b1, b2, _, a1, a2) in enumerate(sos):
                w = b0 * v + z[i, 0]
                z[i, 0] = b1 * v - a1 * w + z[i, 1]
                z[i, 1] = b2 * v - a2 * w
                v = w
            h[t] = v
        tail = np.cumsum(np.abs(h)[::-1])[::-1]  # tail[k] = sum |h[k:]|
        keep = int(np.argmax(tail < 2.0 ** -24 * tail[0])) if np.any(tail < 2.0 ** -24 * tail[0]) else 0
        if keep and keep < n // 2:
            return h[:keep]
        if 2 * n > limit:
            return h
        n *= 2


def main():
    import torch

    import spectrograms_amd as sg
    torch.cuda.set_device(0)
    cases = [("sosfilt", DC_BLOCKER, "auto", 256, 480000), ("sosfilt", BUTTER8_LP, "auto", 256, 480000),
             ("sosfiltfilt", BUTTER8_LP, "auto", 256, 480000), ("stream", BUTTER8_LP, "auto", 4096, 1600),
             ("sosfilt", BUTTER8_LP, "split", 8, 28800000)]
    irs = {}
    for dtype in ("float32", "float64"):
        tdt = torch.float32 if dtype == "float32" else torch.float64
        for form, sos, route, batch, n in cases:
            x = torch.randn(batch, n, dtype=tdt, device="cuda")
            out = torch.empty_like(x)
            plan = sg.IirPlan(sos, dtype=dtype, route=route)
            plan.reserve(batch, n, host_staging=False)
            call = {"sosfilt": lambda: plan.filter_torch(x, out=out), "sosfiltfilt": lambda: plan.filtfilt_torch(x, out=out),
                    "stream": lambda: plan.process_torch(x, out=out)}[form]
            s, iters = time_call(call, torch)
            passes = 2 if form == "sosfiltfilt" else 1
            n_run = n + (2 * plan.padlen if passes == 2 else 0)
            nbytes = 2 * batch * n * x.element_size()
            ops = 2 * passes * OPS_PER_SECTION * len(sos) * batch * n_run
            row = {"form": form, "sections": len(sos), "route": plan.kernel_name, "dtype": dtype, "batch": batch, "n_samples": n,
                   "tile": plan.tile, "block": plan.block, "us": round(s * 1e6, 1), "iters": iters,
                   "samples_per_s": round(batch * n / s, 1), "algorithmic_bytes": int(nbytes), "frac_8tbs": round(nbytes / s / PEAK_BYTES, 4),
                   "frac_f64_vector": round(ops / s / PEAK_F64_VECTOR, 4), "fir_taps": None, "fir_us": None, "fir_kernel": None}
            if "--no-baseline" not in sys.argv and form != "sosfiltfilt":
                try:
                    key = len(sos)
                    if key not in irs:
                        irs[key] = truncated_impulse_response(sos)
                    fir = sg.FirPlan(irs[key], dtype=dtype)
                    fir.reserve(batch, n, host_staging=False)
                    sf, _ = time_call(lambda: fir.process_torch(x, out=out), torch)
                    row["fir_taps"], row["fir_us"], row["fir_kernel"] = int(len(irs[key])), round(sf * 1e6, 1), fir.kernel_name
                    row["fir_over_iir"] = round(sf / s, 2)
                    del fir
                except Exception as e:  # noqa: BLE001 (reported, not hidden)
                    row["fir_error"] = f"{type(e).__name__}: {str(e)[:200]}"
            print(json.dumps(row), flush=True)
            del plan, x, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
