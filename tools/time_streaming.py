"""Times the streaming spectrogram plans (stream.hip) on the device next to what a caller writes by hand with the same plan: one JSON
line per case with the device time per push of both, median / min / max over all timed pushes, and the ratio of the medians.  A push
emits block / hop frames on average (16000 / 512 = 31.25: the pushes cycle through 31, 31, 31, 32); both forms see the same cycle.

Cases (device-resident blocks of noise, steady state):
    4096 streams x 1600-sample blocks, speech_default (512 / 160) Mel-80 dB, f32
      64 streams x 16000-sample blocks, music_default (2048 / 512) linear power, f32 and f64
"stream" is StreamingPlan.push(block).  "by_hand" is the carry a caller keeps today: rows = torch.cat([tail, block], 1); frames =
no-centre Plan.compute_batch(rows); tail = rows[:, consumed:].clone().  Both allocate their outputs through torch, as a caller would.
Each push is timed with its own pair of torch.cuda.Event on the current stream; after a warm-up the two forms take turns for
--rounds rounds of --pushes pushes each.  "_us_back_to_back" is a round's first event to its last over its pushes (the median over
the rounds): what a caller who pushes without waiting pays per push, launch gaps included.

    python tools/time_streaming.py [--rounds 7] [--pushes 200]
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
    speech, music = sg.SpectrogramParams.speech_default(16000.0), sg.SpectrogramParams.music_default(44100.0)
    cases = [("speech_mel80_db", speech, (_ffi.AMP_DECIBELS, sg.MelParams(80, 0.0, 8000.0), sg.LogParams(-80.0)), "float32", 4096, 1600),
             ("music_linear_power", music, (_ffi.AMP_POWER, None, None), "float32", 64, 16000),
             ("music_linear_power", music, (_ffi.AMP_POWER, None, None), "float64", 64, 16000)]
    for name, params, (amp, mel, db), dtype, batch, block in cases:
        tdt = torch.float32 if dtype == "float32" else torch.float64
        st = params.stft
        stream = sg.StreamingPlan(params, amp, mel, db, dtype)
        stream.reserve(batch, block, host_staging=False)
        flat = sg.Plan(sg.SpectrogramParams(type(st)(st.n_fft, st.hop_size, st.window, False), params.sample_rate), amp, mel, db, dtype)
        flat.reserve(batch, st.n_fft - 1 + block, host_staging=False)
        blocks = [torch.randn(batch, block, dtype=tdt, device="cuda") for _ in range(4)]
        hand = {"tail": torch.zeros(batch, st.n_fft // 2 if st.centre else 0, dtype=tdt, device="cuda")}

        def push_stream(x):
            return stream.push(x)

        def push_hand(x):
            rows = torch.cat([hand["tail"], x], 1)
            p = rows.shape[1]
            f = (p - st.n_fft) // st.hop_size + 1 if p >= st.n_fft else 0
            out = flat.compute_batch(rows) if f else None
            hand["tail"] = rows[:, f * st.hop_size:].clone()
            return out

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

        for fn in (push_stream, push_hand):  # warm-up: code objects, the allocator's blocks, the steady pending length
            timed(fn, 10)
        us, run = {"stream": [], "by_hand": []}, {"stream": [], "by_hand": []}
        for _ in range(args.rounds):
            for k, fn in (("stream", push_stream), ("by_hand", push_hand)):
                each, mean = timed(fn, args.pushes)
                us[k] += each
                run[k].append(mean)
        row = {"case": name, "dtype": dtype, "batch": batch, "block": block, "n_fft": st.n_fft, "hop": st.hop_size,
               "kernel": stream.kernel_name, "mean_frames_per_push": round(block / st.hop_size, 2), "pushes": args.rounds * args.pushes}
        for k, v in us.items():
            row[k + "_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
            row[k + "_us_back_to_back"] = round(statistics.median(run[k]), 1)
        row["stream_over_by_hand"] = round(statistics.median(us["stream"]) / statistics.median(us["by_hand"]), 3)
        print(json.dumps(row), flush=True)
        del stream, flat, blocks, hand
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
