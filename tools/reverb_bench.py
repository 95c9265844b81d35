"""Reverberation on the device (csrc/reverb.hip, rsrgan_wave_reverb: four launches) against the float64 host route (io/reverb.py
reverberate), at the shape the sequence recipes would feed: B utterances of --seconds against an RIR of --rir_seconds, a noise on every
utterance, shift and normalize on, for C in --fft.

  host     reverberate on every utterance over 16 threads, wall clock, best and median of --repeats
  device   the entry alone between two device events, resident samples and tables, median / min / max over the rounds; the largest
           e = max |out - host| / rms(host) over the batch beside it
  --bench  additionally `bench.py --gpus 1 --steps 30 --warmup 5` in a child process, twice: the training step this entry would feed

Usage: python tools/reverb_bench.py [--out profiles/reverb.txt] [--fft 512 1024 2048] [--bench]"""
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
    ap.add_argument("--fft", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--rir_seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bench", default=False, action="store_true")
    a = ap.parse_args(argv)
    import torch
    from rsrgan_amd.frontend import FrontEnd
    from rsrgan_amd.io import reverb as RV
    from rsrgan_amd.io import wave as W
    ops = FrontEnd()
    dev = ops.device
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    rng = np.random.default_rng(1)
    n, L, B = int(a.seconds * 16000), int(a.rir_seconds * 16000), a.batch
    utts = [np.clip(np.rint(rng.standard_normal(n) * 3000), -32768, 32767).astype(np.int16) for _ in range(B)]
    rirs = []
    for r in range(4):
        h = (rng.standard_normal(L) * 0.1 * np.exp(-np.arange(L) / (0.12 * L))).astype(np.float32)
        h[30 + r] = 1.0
        rirs.append(h)
    noises = [(rng.standard_normal(3 * 16000) * 500).astype(np.float32)]
    draws = [(b % 4, 0, 100 * b, n + L - 1 - 100 * b, 5.0 + 0.4 * b) for b in range(B)]
    lines = []
    times = []
    one = lambda i: RV.reverberate(utts[i], rirs[draws[i][0]], noises[0], None, draws[i][2], draws[i][3], draws[i][4])
    with ThreadPoolExecutor(16) as pool:
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            host = list(pool.map(one, range(B)))
            times.append(time.perf_counter() - t0)
    lines.append({"measurement": "host", "route": "reverberate (float64, np.fft)", "B": B, "samples": n, "taps": L, "threads": 16,
                  "s_per_batch_best": round(min(times), 5), "s_per_batch_median": round(statistics.median(times), 5)})
    wb = W.pack_wave(utts)
    rir, rseg = RV.rir_table(rirs)
    noise, nseg, npow = RV.noise_table(noises)
    pcm, seg = up(wb.samples), up(wb.seg)
    tabs = [up(v) for v in (rir, rseg, noise, nseg, npow, np.array([d[:4] for d in draws], np.int32), np.array([d[4] for d in draws], np.float32))]
    out = torch.empty(B * n, dtype=torch.float32, device=dev)
    for C in a.fft:
        tw = up(W.twiddle_table(2 * C))
        work = torch.empty(ops.wave_reverb_work(B, n, L, C), dtype=torch.uint8, device=dev)
        launch = lambda: ops.op_wave_reverb(pcm, seg, tabs[0], tabs[1], tabs[2], tabs[3], tabs[4], tabs[5], tabs[6], B, C, tw, out, seg, work)
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); launch(); e1.record()
            e1.synchronize()
            us.append(1e3 * e0.elapsed_time(e1))
        got = out.cpu().numpy().reshape(B, n).astype(np.float64)
        e = max(float(np.abs(got[b] - host[b]).max() / np.sqrt((host[b] * host[b]).mean())) for b in range(B))
        lines.append({"measurement": "device", "entry": "rsrgan_wave_reverb, int16 samples, four launches", "C": C, "B": B, "samples": n, "taps": L,
                      "us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2), "rounds": a.rounds,
                      "work_bytes": int(work.numel()), "largest_e_against_the_host_route": e})
        del work
    if a.bench:
        for run in range(2):
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5"], cwd=ROOT,
                               capture_output=True, text=True, timeout=600)
            last = [l for l in r.stdout.splitlines() if l.startswith("{")]
            lines.append({"measurement": "bench.py --gpus 1 --steps 30 --warmup 5", "run": run, "result": {k: v for k, v in json.loads(last[-1]).items() if k in ("value", "unit", "ms_per_step", "ms_per_step_median", "steps")}
                          if last else r.stderr[-400:]})
    text = "".join(json.dumps(o) + "\n" for o in lines)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/reverb_bench.py on an MI355X (gfx950): rsrgan_wave_reverb (csrc/reverb.hip) against the float64 host route; see the tool's\n"
                    "docstring for what each line measures.  One JSON object per line; host times are of the GPU machine's CPU.\n" + text)


if __name__ == "__main__":
    main()
