"""Times the minimum-phase plans (minphase.hip) on the device against the four f64 real transforms they contain.

Shape: 1024 rows x 512 taps at oversample 8 (n = 4096), device-resident, f32 and f64 rows, the fused route (k_minphase) and the
generic route (minphase_generic, forced).  The yardstick is what the library could already do for these rows before the plans existed:
the four f64 real transforms of length 4096 as existing plans — two complex-STFT executes and two sgx_istft calls with n_fft = hop =
4096, a rectangular window, not centred, 1024 one-frame rows — back to back on one stream, without any of the steps between them.

Every case is warmed up, then the cases take turns for --rounds rounds (default 5); a turn is timed with device events around
back-to-back calls over at least 0.25 s.  One JSON line per case with the median, the fastest and the slowest turn, and a last line
with the ratios fused / yardstick.

    python tools/time_minphase.py [--rounds N] [--batch B] [--taps T]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def turn(fn, torch, min_s=0.25):
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
    return e0.elapsed_time(e1) / iters * 1e-3


def main():
    import numpy as np
    import torch

    import spectrograms_amd as sg
    from spectrograms_amd import _ffi
    torch.cuda.set_device(0)
    batch, taps, rounds = arg("--batch", 1024), arg("--taps", 512), arg("--rounds", 5)
    rng = np.random.default_rng(0)
    k = np.arange(taps)
    ir = rng.standard_normal((batch, taps)) * np.exp(-k / (taps / 6.0))
    cases = {}
    keep = []
    for dtype in ("float32", "float64"):
        tdt = torch.float32 if dtype == "float32" else torch.float64
        x = torch.from_numpy(ir).to(tdt).cuda()
        for route in ("auto", "generic"):
            plan = sg.MinPhasePlan(taps, dtype=dtype, route=route)
            plan.reserve(batch, host_staging=False)
            out = torch.empty((batch, plan.output_length), dtype=tdt, device="cuda")
            keep.append((plan, x, out))
            cases[f"{plan.kernel_name}-{dtype}"] = (lambda p=plan, a=x, o=out: p.execute_torch(a, o))
    n = keep[0][0].fft_size
    # the yardstick: the four f64 real transforms of length n over `batch` one-frame rows, as plans the library already had
    stft = sg.Plan(sg.SpectrogramParams(sg.StftParams(n, n, sg.WindowType.rectangular, False), 1.0), _ffi.AMP_COMPLEX, None, None, "float64")
    stft.reserve(batch, n, host_staging=False)
    stft.reserve(batch, n, host_staging=False, inverse=True)
    rows = torch.randn(batch, n, dtype=torch.float64, device="cuda")
    spec = torch.empty((batch, n // 2 + 1, 1, 2), dtype=torch.float64, device="cuda")
    back = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    stft.compute_batch(rows, spec)
    cspec = torch.view_as_complex(spec)

    def four():
        stft.compute_batch(rows, spec)
        stft.istft_batch(cspec, back)
        stft.compute_batch(rows, spec)
        stft.istft_batch(cspec, back)

    cases["four_f64_transforms"] = four
    cases["r2c_f64"] = lambda: stft.compute_batch(rows, spec)
    cases["c2r_f64"] = lambda: stft.istft_batch(cspec, back)
    for fn in cases.values():  # every shape of the timed window, warm
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    for _ in range(rounds):
        for name, fn in cases.items():
            times[name].append(turn(fn, torch))
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        print(json.dumps({"case": name, "batch": batch, "taps": taps, "n": n, "rounds": rounds, "us_median": round(med[name] * 1e6, 1),
                          "us_min": round(min(ts) * 1e6, 1), "us_max": round(max(ts) * 1e6, 1),
                          "forward_kernel": stft.kernel_name if "f64" in name and "minphase" not in name else None,
                          "inverse_kernel": stft.istft_kernel_name if "f64" in name and "minphase" not in name else None}), flush=True)
    print(json.dumps({"fused_f64_over_four_transforms": round(med["k_minphase-float64"] / med["four_f64_transforms"], 3),
                      "fused_f32_over_four_transforms": round(med["k_minphase-float32"] / med["four_f64_transforms"], 3),
                      "generic_f64_over_four_transforms": round(med["minphase_generic-float64"] / med["four_f64_transforms"], 3)}), flush=True)


if __name__ == "__main__":
    main()
