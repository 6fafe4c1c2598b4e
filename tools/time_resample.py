"""Times the sample-rate conversion plans (resample.hip) on the device against what a caller writes without them: one JSON line per
(shape, dtype) with the kernel, us per call, input samples per second, the fraction of 8 TB/s that the algorithmic bytes imply
(x read once, y written once), and the ratio to the baseline.

Shapes, device-resident, f32 and f64:
    256 rows x 10 s at 44.1 -> 16 kHz, 48 -> 16 kHz and 16 -> 48 kHz, the stateless form (resample_torch);
    4096 streams x 1600-sample pushes at 48 -> 16 kHz, the streaming form (process_torch).
Baseline: torchaudio's construction on this tree's own dependencies — torch.nn.functional.conv1d of the padded rows with the dense
[new, 1, 2 width + orig] kernel at stride orig (reduced rates), transposed and trimmed, on the same device and dtype.  A baseline that
the installed torch cannot run (no f64 convolution, out of memory) is reported as null with the error text, not replaced.
Each case is timed with device events around back-to-back calls on one stream, after a warm-up, over at least 1 s of calls.

    python tools/time_resample.py [--no-baseline]
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES = 8.0e12


def time_call(fn, torch, min_s=1.0):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        fn()
    e1.record()
    e1.synchronize()
    per = e0.elapsed_time(e1) / 3 * 1e-3
    iters = max(10, int(min_s / max(per, 1e-6)) + 1)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3, iters


def dense_kernel(orig, new, torch, tdt, lpw=6, rolloff=0.99):
    """torchaudio's _get_sinc_resample_kernel (sinc_interp_hann) on the reduced rates, built in f64: ([new, 1, 2 width + orig], width)."""
    g = math.gcd(orig, new)
    orig, new = orig // g, new // g
    base = min(orig, new) * rolloff
    width = math.ceil(lpw * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
    t = (t * base).clamp_(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    k = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / orig)
    return k.to(tdt).cuda(), width, orig, new


def baseline(x, kernel, width, orig, new, torch):
    n = x.shape[-1]
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (width, width + orig))[:, None], kernel, stride=orig)
    y = y.transpose(1, 2).reshape(x.shape[0], -1)
    return y[:, :-(-n * new // orig)]


def main():
    import torch

    import spectrograms_amd as sg
    torch.cuda.set_device(0)
    shapes = [("whole", 44100, 16000, 256, 441000), ("whole", 48000, 16000, 256, 480000), ("whole", 16000, 48000, 256, 160000),
              ("stream", 48000, 16000, 4096, 1600)]
    for dtype in ("float32", "float64"):
        tdt = torch.float32 if dtype == "float32" else torch.float64
        for form, orig, new, batch, n in shapes:
            x = torch.randn(batch, n, dtype=tdt, device="cuda")
            plan = sg.ResamplePlan(orig, new, dtype=dtype)
            plan.reserve(batch, n, host_staging=False)
            if form == "whole":
                out = torch.empty((batch, plan.out_len(n)), dtype=tdt, device="cuda")
                s, iters = time_call(lambda: plan.resample_torch(x, out), torch)
                n_out = plan.out_len(n)
            else:  # pushes of one block after another: the output count alternates with the phase of the stream
                s, iters = time_call(lambda: plan.process_torch(x), torch)
                n_out = n * plan.up / plan.down
            nbytes = batch * (n + n_out) * x.element_size()
            row = {"form": form, "orig": orig, "new": new, "dtype": dtype, "batch": batch, "n_samples": n, "kernel": plan.kernel_name,
                   "down": plan.down, "up": plan.up, "taps_per_phase": plan.taps_per_phase, "tile": plan.tile, "us": round(s * 1e6, 1),
                   "iters": iters, "samples_per_s": round(batch * n / s, 1), "algorithmic_bytes": int(nbytes),
                   "frac_8tbs": round(nbytes / s / PEAK_BYTES, 4), "baseline_us": None, "speedup": None}
            if "--no-baseline" not in sys.argv:
                try:
                    k, width, ro, rn = dense_kernel(orig, new, torch, tdt)
                    ref = baseline(x, k, width, ro, rn, torch)
                    if form == "whole":  # the two must agree before their times are compared
                        err = float((ref - plan.resample_torch(x)).abs().max())
                        row["max_abs_diff_to_baseline"] = err
                    sb, _ = time_call(lambda: baseline(x, k, width, ro, rn, torch), torch)
                    row["baseline_us"], row["speedup"] = round(sb * 1e6, 1), round(sb / s, 2)
                    del k, ref
                except Exception as e:  # noqa: BLE001 (reported, not hidden)
                    row["baseline_error"] = f"{type(e).__name__}: {str(e)[:200]}"
            print(json.dumps(row), flush=True)
            del plan, x
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
