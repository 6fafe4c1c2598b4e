"""Times the binaural plans (binaural.hip) on the device against mono plans over the same samples: one JSON line per case with the route,
device us per call and the ratio to the mono plan the issue names as its yardstick.

Shape: 256 stereo pairs x 10 s of 16 kHz audio, f32, n_fft 1024, hop 256.  The mono plans run on the same 512 rows (left rows, then right
rows) in one call.  Each case is timed with device events around back-to-back launches on one stream, after a warm-up, over at least 1 s
of launches.
  itd_default  ITD, band 50-620 Hz       vs  Mel-80 power (same reads and transforms, small output)
  ild_full     ILD, bins 1..511          vs  linear power (per-bin output of about the same size)
  ipd / ilr    their default bands       (for reference)
  complex      the complex STFT alone of the 512 rows (the generic route's first stage)

With --ab the binaural cases also run on the generic route (complex STFT of each channel into scratch, then the epilogue kernel) of a
variant build of binaural.hip with -DSGX_BIN_NO_FUSED (build/libsgx_bin_generic.so, loaded through SGX_LIB_PATH in a child process), and
a last line gives fused / generic per case; the product library reads no switch.

    python tools/time_binaural.py [--ab]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def run():
    import torch

    import spectrograms_amd as sg
    from spectrograms_amd import _ffi
    torch.cuda.set_device(0)
    pairs, n, sr = 256, 160000, 16000.0
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(2 * pairs, n, dtype=torch.float32, device="cuda", generator=g)
    left, right = x[:pairs], x[pairs:]
    sp = sg.SpectrogramParams(sg.StftParams(1024, 256, sg.WindowType.hanning, True), sr)

    def mono(name, plan):
        out = plan.compute_batch(x) if not plan.is_complex else None  # (the complex output is a view of a real buffer: allocated per call)
        s, it = time_call((lambda: plan.compute_batch(x)) if out is None else (lambda: plan.compute_batch(x, out)), torch)
        return {"case": name, "kernel": plan.kernel_name, "us": round(s * 1e6, 1), "iters": it}

    ref = {"mel80_power": mono("mel80_power_512_rows", sg.Plan(sp, _ffi.AMP_POWER, sg.MelParams(80, 0.0, 8000.0), dtype="float32")),
           "linear_power": mono("linear_power_512_rows", sg.Plan(sp, _ffi.AMP_POWER, dtype="float32")),
           "complex": mono("complex_512_rows", sg.Plan(sp, _ffi.AMP_COMPLEX, dtype="float32"))}
    for r in ref.values():
        print(json.dumps(r), flush=True)
    bw = sr / 1024
    cases = [("itd_default", sg.ITDSpectrogramParams(sp), "mel80_power"), ("ild_full", sg.ILDSpectrogramParams(sp, bw, sr / 2), "linear_power"),
             ("ipd_default", sg.IPDSpectrogramParams(sp), None), ("ilr_default", sg.ILRSpectrogramParams(sp), None),
             ("itd_full", sg.ITDSpectrogramParams(sp, bw, sr / 2), "linear_power")]
    for name, params, against in cases:
        plan = sg.BinauralPlan(params, "float32")
        plan.reserve(pairs, n, host_staging=False)
        out = plan.compute_torch(left.contiguous(), right.contiguous())
        lc, rc = left.contiguous(), right.contiguous()
        s, it = time_call(lambda: plan.compute_torch(lc, rc, out), torch)
        rec = {"route": os.environ.get("SGX_BIN_ROUTE", "product"), "case": name, "kernel": plan.kernel_name, "n_bins": out.shape[1], "us": round(s * 1e6, 1), "iters": it}
        if against:
            rec["vs"] = ref[against]["case"]
            rec["ratio"] = round(s * 1e6 / ref[against]["us"], 3)
        print(json.dumps(rec), flush=True)
        del out, plan
        torch.cuda.empty_cache()


def main():
    if os.environ.get("SGX_BIN_ROUTE"):
        run()
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, SGX_BIN_ROUTE="product"), stdout=subprocess.PIPE,
                       text=True)
    sys.stdout.write(r.stdout)
    if r.returncode or "--ab" not in sys.argv:
        sys.exit(r.returncode)
    from spectrograms_amd import build
    lib = build.variant("bin_generic", ["-DSGX_BIN_NO_FUSED"], ("binaural.hip",))
    g = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, SGX_LIB_PATH=lib, SGX_BIN_ROUTE="generic"),
                       stdout=subprocess.PIPE, text=True)
    sys.stdout.write(g.stdout)
    us = lambda out: {d["case"]: d["us"] for d in map(json.loads, out.splitlines()) if d.get("route")}
    a, b = us(r.stdout), us(g.stdout)
    print(json.dumps({"generic_over_fused": {k: round(b[k] / a[k], 2) for k in a if k in b}}), flush=True)
    sys.exit(g.returncode)


if __name__ == "__main__":
    main()
