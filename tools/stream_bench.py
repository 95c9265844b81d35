"""The live multi-stream decode (rsrgan_amd/stream.py StreamBank): the host path (CMVN and the splice in NumPy, the expanded batch uploaded,
the whole output copied back and de-normalised in NumPy) against the device path (device_features=True: the packed raw frames and a
table uploaded, csrc/feat.hip k_feat_stream on a device-resident ring, k_feat_denorm, only each row's frames copied back).

  One inference handle at the reference's size (lstm 3 x 760 / 280, as --decode_lean builds it), D = 257, context 5 / 5, output 40, S = 32
  streams.  Every round pushes 10 new frames to each of the 32 rows (chunk = 10: one forward_stream call of 10 frames per round once the
  right context is filled), 200 rounds per pass after a warm-up pass of 20.  A pass is timed per round (bank.push returns host arrays, so
  a round ends with its device-to-host copy).  The two paths ALTERNATE (--repeats passes each) on the same handle and the same frames; the
  report gives every pass's median and mean, the median over passes and their spread, the bytes each path moved over PCIe per round
  (StreamBank.counters: what was handed to the copies, both directions), the ratio, and whether the two paths returned the same bytes.

Usage: python tools/stream_bench.py [--out profiles/feat_stream.txt] [--rounds 200] [--repeats 3]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--streams", type=int, default=32)
ap.add_argument("--push", type=int, default=10)
ap.add_argument("--rounds", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--dim", type=int, default=257)
ap.add_argument("--out_dim", type=int, default=40)
ap.add_argument("--context", type=int, default=5)
a = ap.parse_args()


def one_pass(bank, frames, rounds):
    """`rounds` pushes of a.push frames to every row, then a flush (not timed); ms per round and a digest of everything returned"""
    S, n = a.streams, a.push
    bank.reset()
    for k in bank.counters:
        bank.counters[k] = 0
    ms, digest = [], 0.0
    for i in range(rounds):
        t0 = time.perf_counter()
        outs = bank.push({r: frames[r, i * n:(i + 1) * n] for r in range(S)})
        ms.append((time.perf_counter() - t0) * 1e3)
        digest += float(sum(np.abs(o).sum() for o in outs.values()))
    counters = dict(bank.counters)
    digest += float(sum(np.abs(o).sum() for o in bank.flush().values()))
    return ms, counters, digest


def main():
    import torch
    sys.path.insert(0, HERE)
    from rsrgan_amd import GAN_RNN
    from rsrgan_amd.stream import StreamBank
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    S, ctx = a.streams, a.context
    args = SimpleNamespace(batch_size=S, input_dim=a.dim, output_dim=a.out_dim, left_context=ctx, right_context=ctx, g_type="lstm", keep_prob=1.0,
                           batch_norm=False, num_gpu=1, save_dir=None, l2_scale=1e-5, g_learning_rate=8e-5, d_learning_rate=1e-3,
                           init_mse_weight=10.0, init_disc_noise_std=0.0, disc_updates=1, gen_updates=2)
    model = GAN_RNN(None, args, ["gpu:0"], cross_validation=True, infer=True, max_frames=a.push, inference_only=True)
    rng = np.random.default_rng(0)
    cmvn = dict(mean_inputs=rng.standard_normal(a.dim), stddev_inputs=rng.uniform(0.5, 2.0, a.dim),
                mean_labels=rng.standard_normal(a.out_dim), stddev_labels=rng.uniform(0.5, 2.0, a.out_dim))
    frames = rng.standard_normal((S, a.rounds * a.push, a.dim), dtype=np.float32) * 2 + 1
    banks = {"host": StreamBank(model, cmvn, ctx, ctx, chunk=a.push, streams=S, device_features=False),
             "device": StreamBank(model, cmvn, ctx, ctx, chunk=a.push, streams=S, device_features=True)}
    lines, runs = [], {k: [] for k in banks}

    def emit(o):
        lines.append(json.dumps(o))
        print(lines[-1], flush=True)
    for name, bank in banks.items():
        one_pass(bank, frames, a.warmup)
    for rep in range(a.repeats):
        for name, bank in banks.items():
            ms, c, digest = one_pass(bank, frames, a.rounds)
            o = {"measurement": "pass", "path": name, "repeat": rep, "streams": S, "push": a.push, "rounds": a.rounds, "D": a.dim, "context": ctx,
                 "ring_frames": bank.ring_frames, "ms_per_round_median": round(float(np.median(ms)), 4), "ms_per_round_mean": round(float(np.mean(ms)), 4),
                 "ms_per_round_p90": round(float(np.percentile(ms, 90)), 4), "forward_calls": c["calls"],
                 "bytes_up_per_round": round(c["bytes_up"] / a.rounds, 1), "bytes_down_per_round": round(c["bytes_down"] / a.rounds, 1), "digest": digest}
            emit(o)
            runs[name].append(o)
    summary = {"measurement": "summary", "repeats": a.repeats}
    for name, rs in runs.items():
        v = sorted(r["ms_per_round_median"] for r in rs)
        summary[name] = {"ms_per_round_passes": [r["ms_per_round_median"] for r in rs], "median": v[len(v) // 2], "spread": round(v[-1] - v[0], 4),
                         "bytes_per_round": rs[0]["bytes_up_per_round"] + rs[0]["bytes_down_per_round"]}
    h, d = summary["host"], summary["device"]
    summary["host_over_device_time"] = round(h["median"] / d["median"], 3)
    summary["host_over_device_bytes"] = round(h["bytes_per_round"] / d["bytes_per_round"], 3)
    summary["device_faster_by_more_than_the_spread"] = bool(h["median"] - d["median"] > max(h["spread"], d["spread"]))
    summary["same_bytes_returned"] = len({r["digest"] for rs in runs.values() for r in rs}) == 1
    summary["device_status"] = model.engine.device_status()
    emit(summary)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/stream_bench.py on an MI355X (gfx950): StreamBank's host path against its device path (csrc/feat.hip k_feat_stream,\n"
                    "k_feat_denorm); see the tool's docstring for what each line measures.  One JSON object per line: every pass in the order it ran,\n"
                    "then the summary.\n")
            f.write("\n".join(lines) + "\n")
    model.engine.close()


main()
