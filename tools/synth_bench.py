"""Audio out on the device (csrc/synth.hip, rsrgan_wave_synth: four launches) against the float64 host route (io/wave.py
wave_from_lps), at the shape a decode of the sequence recipes would feed: B utterances of --seconds, every utterance's own LPS plus
N(0, 1) per bin as the enhanced rows.

  host     wave_from_lps on every utterance over 16 threads, wall clock, best and median of --repeats
  device   the entry alone between two device events, resident samples, rows and tables, median / min / max over the rounds; the largest
           e = max |out - host| / rms(host) over the batch beside it
  --bench  additionally `bench.py --gpus 1 --steps 30 --warmup 5` in a child process, twice: the training step beside which the call runs

Usage: python tools/synth_bench.py [--out profiles/wave_synth.txt] [--bench]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bench", default=False, action="store_true")
    a = ap.parse_args(argv)
    import torch
    from rsrgan_amd.frontend import FrontEnd
    from rsrgan_amd.io import wave as W
    ops = FrontEnd()
    dev = ops.device
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    rng = np.random.default_rng(1)
    n, B, spec = int(a.seconds * 16000), a.batch, W.DEFAULT
    utts = [np.clip(np.rint(rng.standard_normal(n) * 3000), -32768, 32767).astype(np.int16) for _ in range(B)]
    rows = [(W.lps_from_wave(u) + rng.standard_normal((W.num_frames(n), spec.bins))).astype(np.float32) for u in utts]
    lines, times = [], []
    one = lambda i: W.wave_from_lps(rows[i], utts[i], spec)
    with ThreadPoolExecutor(16) as pool:
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            host = list(pool.map(one, range(B)))
            times.append(time.perf_counter() - t0)
    lines.append({"measurement": "host", "route": "wave_from_lps (float64, np.fft, sequential de-emphasis)", "B": B, "samples": n,
                  "frames": int(rows[0].shape[0]), "threads": 16, "s_per_batch_best": round(min(times), 5),
                  "s_per_batch_median": round(statistics.median(times), 5)})
    wb = W.pack_wave(utts)
    lps = up(np.concatenate(rows, 0))
    pcm, seg, off = up(wb.samples), up(wb.seg), up(wb.offsets)
    us = ops.upload_stream()
    win, tw = ops.wave_tables(spec, us)
    us.synchronize()
    out = torch.empty(B * n, dtype=torch.float32, device=dev)
    work = torch.empty(ops.wave_synth_work(B, int(lps.shape[0]), B * n, spec.frame_length), dtype=torch.uint8, device=dev)
    launch = lambda: ops.op_wave_synth(pcm, seg, off, lps, B, win, tw, out, seg, work, spec.frame_length, spec.frame_shift, spec.padded,
                                       spec.preemph)
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    t = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); launch(); e1.record()
        e1.synchronize()
        t.append(1e3 * e0.elapsed_time(e1))
    got = out.cpu().numpy().reshape(B, n).astype(np.float64)
    e = max(float(np.abs(got[b] - host[b]).max() / np.sqrt((host[b] * host[b]).mean())) for b in range(B))
    lines.append({"measurement": "device", "entry": "rsrgan_wave_synth, int16 samples, four launches", "B": B, "samples": n,
                  "frames": int(rows[0].shape[0]), "us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2),
                  "us_max": round(max(t), 2), "rounds": a.rounds, "work_bytes": int(work.numel()), "largest_e_against_the_host_route": e})
    if a.bench:
        for run in range(2):
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5"], cwd=ROOT,
                               capture_output=True, text=True, timeout=600)
            last = [l for l in r.stdout.splitlines() if l.startswith("{")]
            lines.append({"measurement": "bench.py --gpus 1 --steps 30 --warmup 5", "run": run,
                          "result": {k: v for k, v in json.loads(last[-1]).items() if k in ("value", "unit", "ms_per_step", "ms_per_step_median", "steps")}
                          if last else r.stderr[-400:]})
    text = "".join(json.dumps(o) + "\n" for o in lines)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/synth_bench.py on an MI355X (gfx950): rsrgan_wave_synth (csrc/synth.hip) against the float64 host route; see the tool's\n"
                    "docstring for what each line measures.  One JSON object per line; host times are of the GPU machine's CPU.\n" + text)


if __name__ == "__main__":
    main()
