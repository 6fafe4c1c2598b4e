"""Times the Welch plans (welch.hip) on the device against the composition a caller writes without them: one JSON line per
(shape, kind, dtype) with the kernel, the tile, us per call, input samples per second, the algorithmic bytes (the samples read once,
the spectrum written once; the fused route adds its partials, reported as scratch_bytes), the fraction of 8 TB/s on the input bytes,
and the ratio to the baseline.

Shapes, device-resident, 16 kHz:
    256 rows x 10 s at n_fft 1024 / hop 512 and 1024 / 256, 64 rows x 10 s at 4096 / 2048: PSD in f32 and f64;
    256 rows x 10 s at 1024 / 512: coherence in f32 and f64.
Baseline, on the same tree, in code the Welch plans do not touch:
    PSD        a no-centre linear power plan (Plan.compute_batch on the device tensor, the [batch][bins][frames] spectrogram), torch.mean over the frames, times
               the one-sided weights and the scale; detrend "constant" has no counterpart there, so both sides run WITHOUT detrend;
    coherence  two no-centre complex STFT plans, then torch arithmetic: mean |X|^2, mean |Y|^2, mean conj(X) Y, the quotient.
The two must agree (max relative difference printed) before their times are compared.  Each case is timed with device events around
back-to-back calls on one stream, after a warm-up, over at least 1 s of calls.

    python tools/time_welch.py [--no-baseline]
"""
import json
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


def main():
    import torch

    import spectrograms_amd as sg
    from spectrograms_amd import _ffi
    torch.cuda.set_device(0)
    fs = 16000.0
    cases = [("psd", 256, 160000, 1024, 512), ("psd", 256, 160000, 1024, 256), ("psd", 64, 160000, 4096, 2048),
             ("coherence", 256, 160000, 1024, 512)]
    for dtype in ("float32", "float64"):
        tdt = torch.float32 if dtype == "float32" else torch.float64
        for kind, batch, n, n_fft, hop in cases:
            x = torch.randn(batch, n, dtype=tdt, device="cuda")
            y = (0.5 * x + torch.randn(batch, n, dtype=tdt, device="cuda")) if kind != "psd" else None
            plan = sg.WelchPlan(sg.WelchParams(n_fft, hop, sg.WindowType.hanning, fs, None, "density"), kind, dtype)
            plan.reserve(batch, n, host_staging=False)
            out = torch.empty((batch, plan.n_bins), dtype=tdt, device="cuda")
            s, iters = time_call(lambda: plan.compute_torch(x, y, out=out), torch)
            m, nb, es = plan.n_segments(n), plan.n_bins, x.element_size()
            in_bytes = batch * n * es * (1 if kind == "psd" else 2)
            tiles = -(-m // plan.tile) if plan.tile else 1
            row = {"kind": kind, "dtype": dtype, "batch": batch, "n_samples": n, "n_fft": n_fft, "hop": hop, "segments": m,
                   "kernel": plan.kernel_name, "tile": plan.tile, "us": round(s * 1e6, 1), "iters": iters,
                   "samples_per_s": round(batch * n / s, 1), "input_bytes": int(in_bytes), "output_bytes": int(batch * nb * es),
                   "scratch_bytes": int(2 * batch * tiles * nb * es * (1 if kind == "psd" else 4)),
                   "frac_8tbs_input": round(in_bytes / s / PEAK_BYTES, 4), "baseline_us": None, "speedup": None}
            if "--no-baseline" not in sys.argv:
                try:
                    sp = sg.SpectrogramParams(sg.StftParams(n_fft, hop, sg.WindowType.hanning, False), fs)
                    g = torch.full((nb,), 2.0, dtype=tdt, device="cuda")
                    g[0] = g[-1] = 1.0
                    if kind == "psd":
                        pw = sg.Plan(sp, _ffi.AMP_POWER, None, None, dtype)
                        gs = g * plan.scale

                        def base():
                            return pw.compute_batch(x).mean(dim=-1) * gs
                        row["baseline_bytes"] = int(in_bytes + 2 * batch * nb * m * es)
                    else:
                        cx, cy = sg.Plan(sp, _ffi.AMP_COMPLEX, None, None, dtype), sg.Plan(sp, _ffi.AMP_COMPLEX, None, None, dtype)

                        def base():
                            X, Y = cx.compute_batch(x), cy.compute_batch(y)
                            X = torch.view_as_complex(X) if not X.is_complex() else X
                            Y = torch.view_as_complex(Y) if not Y.is_complex() else Y
                            pxy = (X.conj() * Y).mean(dim=-1)
                            return (pxy.real ** 2 + pxy.imag ** 2) / ((X.real ** 2 + X.imag ** 2).mean(dim=-1) * (Y.real ** 2 + Y.imag ** 2).mean(dim=-1))
                        row["baseline_bytes"] = int(in_bytes + 2 * 2 * batch * nb * m * 2 * es)
                    ref = base()
                    row["max_rel_diff_to_baseline"] = float(((ref - plan.compute_torch(x, y)).abs() / ref.abs().clamp_min(1e-30)).max())
                    sb, _ = time_call(base, torch)
                    row["baseline_us"], row["speedup"] = round(sb * 1e6, 1), round(sb / s, 2)
                    del ref
                except Exception as e:  # noqa: BLE001 (reported, not hidden)
                    row["baseline_error"] = f"{type(e).__name__}: {str(e)[:200]}"
            print(json.dumps(row), flush=True)
            del plan, x, y, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
