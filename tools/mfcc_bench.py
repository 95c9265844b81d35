"""The labels' front end (csrc/wave.hip k_feat_mfcc: PCM -> 40-dim MFCC, compute-mfcc-feats with mfcc_hires.conf) beside the inputs' front
end (k_feat_wave: PCM -> 257-dim LPS) on the SAME samples in the same process, and the float64 host route (io/wave.py mfcc_from_wave), at
tools/wave_bench.py's batch shapes: 64 utterances of rounded Gaussian noise of 100 and of 500 frames, int16.  Record only, no threshold:
the LPS launch is the yardstick -- the MFCC launch writes 40 floats per frame instead of 257 and adds about 2 k multiply-adds per frame.

  host     mfcc_from_wave of every utterance on a pool of 16 threads, best and median of the repeats
  device   rsrgan_feat_mfcc and rsrgan_feat_wave alone between two device events, resident samples and tables, median / min / max over the
           rounds, interleaved round by round; the largest difference of the MFCC rows to the host route
  --banks  the LDS bank conflicts of the mel sums for the recipe's table, ENUMERATED from the table (ds_read_b32: 32-lane halves, bank =
           dword index mod 32), no device needed

Usage: python tools/mfcc_bench.py [--out profiles/feat_mfcc.txt] [--frames 100 500] [--banks]"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bank_cycles(first, count):
    """lane j reads index first[j] + t at step t < count[j]: (LDS cycles, half-wave reads, the worst step's ways) over the wavefronts"""
    cycles = reads = worst = 0
    for w0 in range(0, len(first), 64):
        for half in range(w0, min(w0 + 64, len(first)), 32):
            lanes = list(zip(first[half:half + 32], count[half:half + 32]))
            for t in range(max(n for _, n in lanes)):
                banks = {}
                for a, n in lanes:
                    if t < n:
                        banks.setdefault((a + t) % 32, set()).add(a + t)
                if banks:
                    ways = max(len(v) for v in banks.values())
                    cycles, reads, worst = cycles + ways, reads + 1, max(worst, ways)
    return cycles, reads, worst


def banks_line(spec):
    from rsrgan_amd.io import wave as W
    seg, _ = W.mel_table(spec)
    p, w = bank_cycles(seg[:, 0].tolist(), seg[:, 1].tolist()), bank_cycles(seg[:, 2].tolist(), seg[:, 1].tolist())
    return {"measurement": "lds banks of the mel sums, enumerated", "filters": int(seg.shape[0]), "weights": int(seg[:, 1].sum()),
            "p_reads": {"cycles": p[0], "half_wave_reads": p[1], "worst_ways": p[2]},
            "w_reads": {"cycles": w[0], "half_wave_reads": w[1], "worst_ways": w[2]}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, nargs="+", default=[100, 500])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--banks", default=False, action="store_true")
    a = ap.parse_args(argv)
    from rsrgan_amd.io import wave as W
    lspec, mspec = W.DEFAULT, W.MFCC_DEFAULT
    if a.banks:
        sys.stdout.write(json.dumps(banks_line(mspec)) + "\n")
        return
    import torch
    from rsrgan_amd.frontend import FrontEnd
    ops = FrontEnd()
    dev = ops.device
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    tw = up(W.twiddle_table(512))
    lwin, mwin = (up(W.window_table(s.window, 400).astype(np.float32)) for s in (lspec, mspec))
    mseg, mw = (up(t) for t in W.mel_table(mspec))
    dct = up(W.dct_table(mspec))
    lines = [banks_line(mspec)]
    for frames in a.frames:
        rng = np.random.default_rng(frames)
        n = 400 + (frames - 1) * 160
        utts = [np.clip(np.rint(rng.standard_normal(n) * 3000), -32768, 32767).astype(np.int16) for _ in range(a.batch)]
        total = frames * a.batch
        times = []
        with ThreadPoolExecutor(16) as pool:
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                host = list(pool.map(W.mfcc_from_wave, utts))
                times.append(time.perf_counter() - t0)
        lines.append({"measurement": "host", "route": "mfcc_from_wave", "frames": frames, "B": a.batch, "threads": 16,
                      "s_per_batch_best": round(min(times), 5), "s_per_batch_median": round(statistics.median(times), 5)})
        wb = W.pack_wave(utts)
        pcm, seg, off = (up(v) for v in (wb.samples, wb.seg, wb.offsets))
        lout = torch.empty(total, 257, dtype=torch.float32, device=dev)
        mout = torch.empty(total, 40, dtype=torch.float32, device=dev)
        launches = {"k_feat_mfcc": lambda: ops.op_feat_mfcc(pcm, seg, off, a.batch, mwin, tw, mseg, mw, dct, mout),
                    "k_feat_wave": lambda: ops.op_feat_wave(pcm, seg, off, a.batch, lwin, tw, lout)}
        for _ in range(3):
            for f in launches.values():
                f()
        torch.cuda.synchronize()
        us = {k: [] for k in launches}
        for _ in range(a.rounds):
            for k, f in launches.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); f(); e1.record()
                e1.synchronize()
                us[k].append(1e3 * e0.elapsed_time(e1))
        diff = float(np.abs(mout.cpu().numpy() - np.concatenate(host, 0)).max())
        for k, v in us.items():
            line = {"measurement": "device", "frames": frames, "B": a.batch, "launch": k + ", int16 samples", "us_median": round(statistics.median(v), 2),
                    "us_min": round(min(v), 2), "us_max": round(max(v), 2), "rounds": a.rounds,
                    "frames_per_s_median": round(total / (statistics.median(v) * 1e-6))}
            if k == "k_feat_mfcc":
                line["max_abs_difference_to_the_host_route"] = diff
            lines.append(line)
    text = "".join(json.dumps(o) + "\n" for o in lines)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/mfcc_bench.py on an MI355X (gfx950): the MFCC launch (csrc/wave.hip k_feat_mfcc) beside the LPS launch (k_feat_wave) on the\n"
                    "same samples, and the float64 host route (mfcc_from_wave, 16 threads); see the tool's docstring for what each line measures.\n"
                    "One JSON object per line; host times are of the GPU machine's CPU.\n" + text)


if __name__ == "__main__":
    main()
