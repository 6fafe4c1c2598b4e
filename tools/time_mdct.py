"""Times the MDCT / IMDCT plans (mdct.hip) on the device: one JSON line per (direction, dtype, window) with the route, device us per
call, the algorithmic bytes (forward: samples read + coefficients written; inverse: coefficients read + samples written) and their rate
as a fraction of 8 TB/s.

Shape: 256 signals x 10 s of 16 kHz audio, sine windows 256 / 512 / 1024 / 2048 / 4096 at hop N (the reference's Criterion list,
benches/mdct_benchmarks.rs), f32 and f64.  Each case is timed with device events around back-to-back launches on one stream, after a
warm-up, over at least 1 s of launches.

With --ab the same cases also run on the generic route (fold, batched complex transform, post-twiddle, overlap-add) of a variant build
of mdct.hip with -DSGX_MDCT_NO_FUSED (build/libsgx_mdct_generic.so, loaded through SGX_LIB_PATH in a child process); the product library
reads no switch.

    python tools/time_mdct.py [--ab]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12
WINDOWS = (256, 512, 1024, 2048, 4096)


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


def run(route):
    import torch

    import spectrograms_amd as sg
    torch.cuda.set_device(0)
    batch, n = 256, 160000
    for dtype in ("float32", "float64"):
        tdt = torch.float32 if dtype == "float32" else torch.float64
        es = 4 if dtype == "float32" else 8
        x = torch.randn(batch, n, dtype=tdt, device="cuda")
        for ws in WINDOWS:
            plan = sg.MdctPlan(sg.MdctParams.sine_window(ws), dtype)
            plan.reserve(batch, n, host_staging=False)
            c = plan.forward_torch(x)
            y = plan.inverse_torch(c)
            for inverse in (False, True):
                fn = (lambda: plan.inverse_torch(c, y)) if inverse else (lambda: plan.forward_torch(x, c))
                s, iters = time_call(fn, torch)
                nbytes = (c.numel() + y.numel()) * es if inverse else (x.numel() + c.numel()) * es
                print(json.dumps({"route": route, "direction": "inverse" if inverse else "forward", "dtype": dtype, "window": ws,
                                  "hop": ws // 2, "batch": batch, "n_samples": n, "kernel": plan.kernel_name(inverse),
                                  "us": round(s * 1e6, 1), "iters": iters, "mb": round(nbytes / 1e6, 1),
                                  "tb_per_s": round(nbytes / s / 1e12, 3), "frac_8tbs": round(nbytes / s / PEAK, 3)}), flush=True)
            del c, y, plan
        del x
        torch.cuda.empty_cache()


def main():
    if os.environ.get("SGX_MDCT_ROUTE"):
        run(os.environ["SGX_MDCT_ROUTE"])
        return
    run("fused")
    if "--ab" in sys.argv:
        from spectrograms_amd import build
        lib = os.path.join(ROOT, "build", "libsgx_mdct_generic.so")
        if not os.path.exists(lib):
            lib = build.variant("mdct_generic", ["-DSGX_MDCT_NO_FUSED"], ("mdct.hip",))
        env = dict(os.environ, SGX_LIB_PATH=lib, SGX_MDCT_ROUTE="generic")
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env)
        sys.exit(r.returncode)


if __name__ == "__main__":
    main()
