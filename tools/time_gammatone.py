"""Times the gammatone IIR plans (gammatone.hip) on the device: one JSON line per (shape, dtype) with the kernel, device ms per batch,
(frame, band) pairs per second, and the fraction of the f64 vector peak that the operation count implies.

Operation count: per sample of every (signal, frame, band) the four sections take 16 f64 operations (per section y = a0 x + z0,
a1 x + z1, that minus b1 y, -b2 y: three fused multiply-adds and a multiply) and the energy sum one: 17 lane-operations, each one
issue slot of the f64 vector unit.  Peak: 256 CUs x 4 SIMDs x 16 f64 lanes per clock x 2.4 GHz = 3.93e13 lane-operations per second
(the 78.6 TFLOP/s f64 vector figure counts a fused multiply-add as two).

Shapes: 64 signals x 10 s, device-resident, f32 and f64:
  48 kHz, frame 3840, hop 960, 64 bands Apple TR35 50 Hz - 16 kHz (the reference's documented audio mode)
  16 kHz, frame 1280, hop 320, 40 bands linear 0 - 8 kHz (speech_standard)
Each case is timed with device events around back-to-back launches on one stream, after a warm-up, over at least 1 s of launches.

    python tools/time_gammatone.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_LANE_OPS = 256 * 4 * 16 * 2.4e9
OPS_PER_SAMPLE = 17


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
    import torch

    import spectrograms_amd as sg
    torch.cuda.set_device(0)
    batch = 64
    shapes = (("48k_3840_960_tr35_64", 48000.0, 3840, 960, sg.ErbParams(64, 50.0, 16000.0, "apple_tr35")),
              ("16k_1280_320_speech_40", 16000.0, 1280, 320, sg.ErbParams.speech_standard()))
    for name, sr, frame, hop, erb in shapes:
        n = int(10 * sr)
        for dtype in ("float32", "float64"):
            tdt = torch.float32 if dtype == "float32" else torch.float64
            x = torch.randn(batch, n, dtype=tdt, device="cuda")
            for floor in (None, -80.0):
                plan = sg.GammatonePlan(sr, frame, hop, erb if floor is None else erb.with_db_floor(floor), dtype)
                out = plan.compute_torch(x)
                s, iters = time_call(lambda: plan.compute_torch(x, out), torch)
                nb, nf = plan.output_shape(n)
                pairs = batch * nb * nf
                ops = pairs * frame * OPS_PER_SAMPLE
                print(json.dumps({"shape": name, "dtype": dtype, "db_floor": floor, "batch": batch, "n_samples": n, "n_frames": nf,
                                  "kernel": plan.kernel_name, "ms": round(s * 1e3, 3), "iters": iters,
                                  "pairs_per_s": round(pairs / s, 1), "lane_ops": ops, "ms_at_peak": round(ops / PEAK_LANE_OPS * 1e3, 3),
                                  "frac_f64_vector_peak": round(ops / s / PEAK_LANE_OPS, 3)}), flush=True)
                del plan, out
            del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
