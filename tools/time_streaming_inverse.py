"""Times the streaming inverse STFT plans (istream.hip) on the device next to the loop a caller writes by hand today: one JSON line per
case with the device time per push of both, median / min / max over all timed pushes, and the ratio of the medians.

Cases (device-resident random spectra, steady state, f frames per push):
    4096 streams x 10 frames, 512 / 160, f32
      64 streams x 31 frames, 2048 / 512, f32 and f64
     256 streams x 16 frames, 1024 / 256, f32
"stream" is StreamingInversePlan.push(frames).  "by_hand" keeps the last K - 1 = ceil(n_fft / hop) - 1 frames: S = torch.cat([tail,
frames], 2); y = no-centre Plan.istft_batch(S); out = y[:, (K - 1) hop : (K - 1) hop + f hop]; tail = S[:, :, f:]: every frame is
inverted about n_fft / (f hop) + 1 times.  Both allocate their outputs through torch, as a caller would.  Each push is timed
with its own pair of torch.cuda.Event on the current stream; after a warm-up the two forms take turns for --rounds rounds of --pushes
pushes each.  "_us_back_to_back" is a round's first event to its last over its pushes (the median over the rounds): what a caller who
pushes without waiting pays per push, launch gaps included.

    python tools/time_streaming_inverse.py [--rounds 7] [--pushes 200]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    import spectrograms_amd as sg
    from spectrograms_amd import _ffi

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pushes", type=int, default=200)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    cases = [(512, 160, "float32", 4096, 10), (2048, 512, "float32", 64, 31), (2048, 512, "float64", 64, 31), (1024, 256, "float32", 256, 16)]
    for n_fft, hop, dtype, batch, f in cases:
        cdt = torch.complex64 if dtype == "float32" else torch.complex128
        nb, keep = n_fft // 2 + 1, -(-n_fft // hop) - 1

        def params(centre):
            return sg.SpectrogramParams(sg.StftParams(n_fft, hop, sg.WindowType.hanning, centre), 16000.0)

        stream = sg.StreamingInversePlan(params(True), dtype)
        stream.reserve(batch, f, host_staging=False)
        flat = sg.Plan(params(False), _ffi.AMP_COMPLEX, None, None, dtype)
        flat.reserve(batch, (keep + f - 1) * hop + n_fft, host_staging=False, inverse=True)
        blocks = []
        for _ in range(4):
            S = torch.randn(batch, nb, f, dtype=cdt, device="cuda")
            S[:, 0] = S[:, 0].real.to(cdt)
            S[:, -1] = S[:, -1].real.to(cdt)
            blocks.append(S)
        hand = {"tail": torch.zeros(batch, nb, keep, dtype=cdt, device="cuda")}

        def push_stream(S):
            return stream.push(S)

        def push_hand(S):
            rows = torch.cat([hand["tail"], S], 2)
            y = flat.istft_batch(rows)
            hand["tail"] = rows[:, :, f:]
            return y[:, keep * hop:(keep + f) * hop]

        def timed(fn, count):
            evs = []
            for i in range(count):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(blocks[i % len(blocks)])
                e1.record()
                evs.append((e0, e1))
            torch.cuda.synchronize()
            return [a.elapsed_time(b) * 1e3 for a, b in evs], evs[0][0].elapsed_time(evs[-1][1]) * 1e3 / count  # us

        for fn in (push_stream, push_hand):  # warm-up: code objects, the allocator's blocks, a full carry
            timed(fn, 10)
        us, run = {"stream": [], "by_hand": []}, {"stream": [], "by_hand": []}
        for _ in range(args.rounds):
            for k, fn in (("stream", push_stream), ("by_hand", push_hand)):
                each, mean = timed(fn, args.pushes)
                us[k] += each
                run[k].append(mean)
        row = {"dtype": dtype, "batch": batch, "frames_per_push": f, "n_fft": n_fft, "hop": hop, "samples_per_push": f * hop,
               "kernel": stream.kernel_name, "by_hand_kernel": flat.istft_kernel_name, "by_hand_frames_per_call": keep + f,
               "pushes": args.rounds * args.pushes}
        for k, v in us.items():
            row[k + "_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
            row[k + "_us_back_to_back"] = round(statistics.median(run[k]), 1)
        row["stream_over_by_hand"] = round(statistics.median(us["stream"]) / statistics.median(us["by_hand"]), 3)
        print(json.dumps(row), flush=True)
        del stream, flat, blocks, hand
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
