"""Audio through the host route (io/wave.py lps_from_wave, float64 NumPy) against the device route (csrc/wave.hip k_feat_wave), at the
recipes' framing (400 / 160 / 512, Hamming): 64 utterances of rounded Gaussian noise per batch.  Record only, no threshold, no promise of a
speed-up.

  host     lps_from_wave of every utterance on a pool of 16 threads, best and median of the repeats; the bytes a caller then uploads per
           frame (257 float32)
  device   rsrgan_feat_wave alone between two device events, resident samples and tables, median / min / max over the rounds; the bytes
           that travel per frame (int16 samples of the overlapping spans and the two tables); the largest difference to the host route
  live     what StreamBank.push_audio ships per frame for pushes of `--push` frames' worth of samples, against push (1028 bytes)

Usage: python tools/wave_bench.py [--out profiles/feat_wave.txt] [--frames 100 500]"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, nargs="+", default=[100, 500])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--push", type=int, default=10)
    a = ap.parse_args(argv)
    import torch
    from rsrgan_amd.io import wave as W
    from rsrgan_amd.frontend import FrontEnd
    ops = FrontEnd()
    dev, spec = ops.device, W.DEFAULT
    lines = []
    for frames in a.frames:
        rng = np.random.default_rng(frames)
        n = spec.frame_length + (frames - 1) * spec.frame_shift
        utts = [np.clip(np.rint(rng.standard_normal(n) * 3000), -32768, 32767).astype(np.int16) for _ in range(a.batch)]
        total = frames * a.batch
        times = []
        with ThreadPoolExecutor(16) as pool:
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                host = list(pool.map(W.lps_from_wave, utts))
                times.append(time.perf_counter() - t0)
        lines.append({"measurement": "host", "frames": frames, "B": a.batch, "threads": 16, "s_per_batch_best": round(min(times), 5),
                      "s_per_batch_median": round(statistics.median(times), 5), "bytes_up_per_frame": spec.bins * 4})
        wb = W.pack_wave(utts)
        win = torch.from_numpy(W.window_table(spec.window, spec.frame_length).astype(np.float32)).to(dev)
        tw = torch.from_numpy(W.twiddle_table(spec.padded)).to(dev)
        pcm, seg, off = (torch.from_numpy(v).to(dev) for v in (wb.samples, wb.seg, wb.offsets))
        out = torch.empty(total, spec.bins, dtype=torch.float32, device=dev)
        launch = lambda: ops.op_feat_wave(pcm, seg, off, a.batch, win, tw, out)
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); launch(); e1.record()
            e1.synchronize()
            us.append(1e3 * e0.elapsed_time(e1))
        diff = float(np.abs(out.cpu().numpy() - np.concatenate(host, 0)).max())
        lines.append({"measurement": "device", "frames": frames, "B": a.batch, "launch": "k_feat_wave, int16 samples",
                      "us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2), "rounds": a.rounds,
                      "frames_per_s_median": round(total / (statistics.median(us) * 1e-6)), "bytes_up_per_frame": round(wb.nbytes() / total, 1),
                      "max_abs_difference_to_the_host_route": diff})
    span = spec.frame_length + (a.push - 1) * spec.frame_shift
    lines.append({"measurement": "live", "push_frames": a.push, "bytes_up_per_frame_push_audio": round((span * 2 + 16 + 8) / a.push, 1),
                  "bytes_up_per_frame_push": spec.bins * 4, "note": "one row per push; the round's own table (24 bytes per bank row) travels on both routes"})
    text = "".join(json.dumps(o) + "\n" for o in lines)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/wave_bench.py on an MI355X (gfx950): audio through the host route (lps_from_wave, 16 threads) against the device route\n"
                    "(csrc/wave.hip k_feat_wave); see the tool's docstring for what each line measures.  One JSON object per line; host times are of\n"
                    "the GPU machine's CPU.\n" + text)


if __name__ == "__main__":
    main()
