"""Times the Kaldi fbank / MFCC plans (kaldi.hip) on the device against the composition a caller writes today with torch alone: one JSON
line per (shape, dtype) with the kernel, the tile, us per call, input samples per second, the algorithmic bytes (the samples read once,
the features written once), the time those bytes take at 8 TB/s, the fraction of 8 TB/s reached, and the ratio to the baseline.

Shapes, device-resident:
    256 rows x 10 s at 16 kHz: fbank-80 and MFCC-13 of 23 bins; 64 rows x 10 s at 48 kHz (N 1200 -> P 2048): fbank-80;
    4096 rows x 1 s at 16 kHz: fbank-80; each in f32 and f64.
Baseline, torch alone: `unfold` into frames, the frame mean, the pre-emphasis difference, the window product, `torch.fft.rfft` at P
points, |X|^2, `matmul` with the plan's bank, `log` of the floored energies (MFCC: one more `matmul` with the plan's DCT and the lifter).
The two must agree (max absolute difference of the log features printed) before their times are compared.  Each case is timed with
device events around back-to-back calls on one stream, after a warm-up, over at least 0.5 s of calls.

    python tools/time_kaldi.py [--no-baseline]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES = 8.0e12


def time_call(fn, torch, min_s=0.5):
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


def main():
    import torch

    import spectrograms_amd as sg
    torch.cuda.set_device(0)
    cases = [("fbank80", 256, 160000, dict(num_mel_bins=80)), ("mfcc13of23", 256, 160000, dict(num_mel_bins=23, num_ceps=13)),
             ("fbank80-48k", 64, 480000, dict(num_mel_bins=80, sample_frequency=48000.0)), ("fbank80-1s", 4096, 16000, dict(num_mel_bins=80))]
    for dtype in ("float32", "float64"):
        tdt = torch.float32 if dtype == "float32" else torch.float64
        eps = torch.finfo(tdt).eps
        for name, batch, n, kw in cases:
            x = 0.3 + 0.1 * torch.randn(batch, n, dtype=tdt, device="cuda")
            kp = sg.KaldiParams(**kw)
            plan = sg.KaldiPlan(kp, dtype)
            plan.reserve(batch, n, host_staging=False)
            m, N, shift, P = plan.n_frames(n), plan.window_size, plan.window_shift, plan.padded_window_size
            out = torch.empty((batch, m, plan.n_out), dtype=tdt, device="cuda")
            s, iters = time_call(lambda: plan.compute_torch(x, out=out), torch)
            es = x.element_size()
            in_bytes, out_bytes = batch * n * es, batch * m * plan.n_out * es
            row = {"case": name, "dtype": dtype, "batch": batch, "n_samples": n, "window_size": N, "window_shift": shift, "padded": P,
                   "frames": m, "n_out": plan.n_out, "kernel": plan.kernel_name, "tile": plan.tile, "us": round(s * 1e6, 1), "iters": iters,
                   "samples_per_s": round(batch * n / s, 1), "input_bytes": int(in_bytes), "output_bytes": int(out_bytes),
                   "us_at_8tbs": round((in_bytes + out_bytes) / PEAK_BYTES * 1e6, 1),
                   "frac_8tbs": round((in_bytes + out_bytes) / s / PEAK_BYTES, 4), "baseline_us": None, "speedup": None}
            if "--no-baseline" not in sys.argv:
                try:
                    w = torch.from_numpy(plan.window()).to(device="cuda", dtype=tdt)
                    bank_t = torch.from_numpy(plan.mel_banks()).to(device="cuda", dtype=tdt).T.contiguous()
                    alpha = kp.preemphasis_coefficient
                    dl = None
                    if kp.num_ceps:
                        dl = (torch.from_numpy(plan.dct()).to(device="cuda", dtype=tdt).T * torch.from_numpy(plan.lifter()).to(device="cuda", dtype=tdt)).contiguous()

                    def base():
                        f = x.unfold(-1, N, shift)
                        f = f - f.mean(dim=-1, keepdim=True)
                        g = f - alpha * torch.cat([f[..., :1], f[..., :-1]], dim=-1)
                        X = torch.fft.rfft(g * w, n=P, dim=-1)
                        L = torch.log(torch.clamp_min(torch.matmul(X.real ** 2 + X.imag ** 2, bank_t), eps))
                        return L if dl is None else torch.matmul(L, dl)
                    ref = base()
                    row["max_abs_diff_to_baseline"] = float((ref - plan.compute_torch(x)).abs().max())
                    del ref
                    sb, _ = time_call(base, torch)
                    row["baseline_us"], row["speedup"] = round(sb * 1e6, 1), round(sb / s, 2)
                except Exception as e:  # noqa: BLE001 (reported, not hidden)
                    row["baseline_error"] = f"{type(e).__name__}: {str(e)[:200]}"
            print(json.dumps(row), flush=True)
            del plan, x, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
