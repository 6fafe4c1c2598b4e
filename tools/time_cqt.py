"""Times the constant-Q plans (cqt.hip) on the device and prints one line per case: device us per launch, frames/s, the useful and
issued FLOPs (4 per tap per frame: a multiply-add each for Re and Im; useful = the bins' own L_k taps, issued = the groups' L_g taps
x 8 bins, both counted from the plan's tables) and the issued rate as a fraction of the f32 matrix-core peak (155 TF).

Cases: the reference's Criterion `cqt` shape (n_fft 2048, hop 512, 16 kHz, CqtParams(12, 7, 32.7)) at 64 x 10 s and 256 x 10 s, and
CqtParams.musical() (q = 1: L_0 = 489, bound by memory) at 256 x 10 s; f32 and f64.  f64: the fraction is against 78.6 TF, the
nominal f64 matrix rate of the part (not measured here).

The transform plans (sgx_plan_create_cqt_transform, cqt()'s framing) follow: 256 x 10 s at 16 kHz, CqtParams(12, 7, 32.7), frames of
16384 samples every 512, complex against power output (the same GEMM, different stores); and the one-frame shape of the reference's
own callers, signals of 8000 samples with CqtParams(12, 6, 55.0), complex, on the rows route (route 2) against the per-signal tiles
(route 1) at batches 1 .. 4096.  `existing` / `transform` as a second argument runs one half only.

    python tools/time_cqt.py [iters] [existing|transform]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import spectrograms_amd as sg  # noqa: E402

PEAK = {"float32": 155e12, "float64": 78.6e12}


def case(name, cq, batch, dtype, iters):
    sr, n_fft, hop = 16000.0, 2048, 512
    params = sg.SpectrogramParams(sg.StftParams(n_fft, hop, sg.WindowType.hanning, True), sr)
    plan = sg.SpectrogramPlanner().cqt_power_plan(params, cq, dtype)
    tdt = torch.float32 if dtype == "float32" else torch.float64
    n = int(10 * sr)
    x = torch.randn(batch, n, dtype=tdt, device="cuda")
    nb, nf = plan.output_shape(n)
    out = torch.empty(batch, nb, nf, dtype=tdt, device="cuda")
    plan.compute_batch(x, out)
    plan.time_batch_torch(x, out, 3)  # warm-up
    ms = plan.time_batch_torch(x, out, iters)
    lens = [k.size for k in plan.cqt_kernels()]
    lg = [-(-max(lens[g:g + 8]) // 16) * 16 for g in range(0, len(lens), 8)]
    frames = batch * nf
    useful = 4.0 * sum(lens) * frames
    issued = 4.0 * 8 * sum(lg) * frames
    s = ms * 1e-3
    return {"case": name, "dtype": dtype, "batch": batch, "frames": frames, "kernel": plan.kernel_name, "us": round(ms * 1e3, 1),
            "frames_per_s": round(frames / s), "useful_gflop": round(useful / 1e9, 2), "issued_gflop": round(issued / 1e9, 2),
            "issued_tflops": round(issued / s / 1e12, 1), "frac_peak": round(issued / s / PEAK[dtype], 3)}


def transform_case(name, cq, klen, hop, n, batch, amp, route, dtype, iters):
    from spectrograms_amd import _ffi
    sr = 16000.0
    plan = sg.CqtTransformPlan(sr, klen, hop, cq, amp, None, dtype)
    plan.set_route(route)
    tdt = torch.float32 if dtype == "float32" else torch.float64
    x = torch.randn(batch, n, dtype=tdt, device="cuda")
    nb, nf = plan.output_shape(n)
    out = torch.empty((batch, nb, nf, 2) if amp == _ffi.AMP_COMPLEX else (batch, nb, nf), dtype=tdt, device="cuda")
    plan.compute_batch(x, out)
    plan.time_batch_torch(x, out, 3)  # warm-up
    ms = plan.time_batch_torch(x, out, iters)
    lens = [k.size for k in plan.cqt_kernels()]
    lg = [-(-max(lens[g:g + 8]) // 16) * 16 for g in range(0, len(lens), 8)]
    frames = batch * nf
    issued = 4.0 * 8 * sum(lg) * frames
    s = ms * 1e-3
    return {"case": name, "dtype": dtype, "batch": batch, "frames": frames, "out": "complex" if amp == _ffi.AMP_COMPLEX else "power",
            "route": route, "kernel": plan.kernel_name, "us": round(ms * 1e3, 1), "frames_per_s": round(frames / s),
            "useful_gflop": round(4.0 * sum(lens) * frames / 1e9, 2), "issued_gflop": round(issued / 1e9, 2),
            "issued_tflops": round(issued / s / 1e12, 2), "frac_peak": round(issued / s / PEAK[dtype], 4)}


def main():
    from spectrograms_amd import _ffi
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    which = sys.argv[2] if len(sys.argv) > 2 else "all"
    torch.cuda.set_device(0)
    for dtype in ("float32", "float64"):
        if which == "transform":
            break
        for name, cq, batch in (("bench_12x7", sg.CqtParams(12, 7, 32.7), 64), ("bench_12x7", sg.CqtParams(12, 7, 32.7), 256),
                                ("musical", sg.CqtParams.musical(), 256)):
            print(json.dumps(case(name, cq, batch, dtype, iters)), flush=True)
    for dtype in ("float32", "float64"):
        if which == "existing":
            break
        for amp in (_ffi.AMP_COMPLEX, _ffi.AMP_POWER, _ffi.AMP_COMPLEX, _ffi.AMP_POWER):  # alternating: the two differ by the stores only
            print(json.dumps(transform_case("transform_12x7", sg.CqtParams(12, 7, 32.7), 16384, 512, 160000, 256, amp, 0, dtype, iters)),
                  flush=True)
        for batch in (1, 16, 64, 256, 4096):
            for route in (2, 1, 2, 1):
                print(json.dumps(transform_case("one_frame_12x6", sg.CqtParams(12, 6, 55.0), 8000, 256, 8000, batch, _ffi.AMP_COMPLEX,
                                                route, dtype, max(2, iters // 4) if route == 1 and batch >= 256 else iters)), flush=True)


if __name__ == "__main__":
    main()
