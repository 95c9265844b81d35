"""ms per (1 D + 1 G) step of GAN_RNN with g_type lstm, --batch_norm on against off in the same build and session: the runs alternate
(off, on, off, on, ...), each on a fresh handle, the launch sequence replayed as hipGraphs (flags 3, what bench.py times).  Per
setting: the median over the runs of each run's median step time, and the recurrence-kernel launches of one eagerly profiled step
(profile_launches(); the input layer's own launches are not recurrence kernels and not in that counter).  One JSON line per setting.

Every kernel of a step, the input layer's included, is counted from outside: `--trace on|off --steps K` runs K steps of ONE setting and
nothing else, to be run under a kernel trace (rocprofv3 --kernel-trace, a run of its own); the difference of two such runs' dispatch
counts divided by the difference of their K is the kernels per step.  `--root DIR` imports rsrgan_amd from another tree, so the same
count can be taken on a build of another commit; profiles/seq_bn_step.txt names the tree of every count it holds.

Usage: python tools/seq_bn_step.py [--batch 64] [--frames 100] [--steps 50] [--warmup 10] [--runs 3] [--trace on|off [--root DIR]]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--trace", choices=("on", "off"), default=None, help="run --steps steps of this batch_norm setting only (for a kernel trace)")
ap.add_argument("--root", type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree to import rsrgan_amd from")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--dim", type=int, default=257)
ap.add_argument("--out_dim", type=int, default=40)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--runs", type=int, default=3)
a = ap.parse_args()
sys.path.insert(0, a.root)
from rsrgan_amd import GAN_RNN      # noqa: E402

B, T = a.batch, a.frames
rng = np.random.default_rng(0)
xh = rng.standard_normal((B, T, a.dim)).astype(np.float32)
labh = rng.standard_normal((B, T, a.out_dim)).astype(np.float32)
lnh = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
lnh[0] = T


def build(batch_norm):
    """the model of one setting on a fresh handle, and the batch on its device"""
    args = SimpleNamespace(batch_size=B, input_dim=a.dim, output_dim=a.out_dim, left_context=0, right_context=0, g_type="lstm",
                           keep_prob=1.0, batch_norm=batch_norm, num_gpu=1, save_dir=None, l2_scale=1e-5, g_learning_rate=8e-5,
                           d_learning_rate=1e-3, init_mse_weight=10.0, init_disc_noise_std=0.0, disc_updates=1, gen_updates=1)
    m = GAN_RNN(None, args, ["gpu:0"], max_frames=T, net_overrides=dict(flags=1 | 2))
    dev = m.engine.device
    return m, torch.tensor(xh, device=dev), torch.tensor(labh, device=dev), torch.tensor(lnh, device=dev)


def one_run(batch_norm):
    m, x, lab, ln = build(batch_norm)
    times = []
    with m.on_stream():
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.d_step(x, lab, ln, sync=False)
            out = m.g_step(x, lab, ln, reuse_g_forward=True, sync=False)
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        m.engine.profile_begin()                 # (one more step, outside the timing: which launches it took)
        m.d_step(x, lab, ln, sync=False)
        m.g_step(x, lab, ln, reuse_g_forward=True, sync=False)
        torch.cuda.synchronize()
    launches = int(m.engine.profile_launches())
    m.engine.profile_read()
    status = m.engine.device_status()
    losses = [float(v) for v in out.reshape(-1).cpu().numpy()]
    m.engine.close()
    return float(np.median(times)), launches, status, losses


if a.trace is not None:
    m, x, lab, ln = build(a.trace == "on")
    with m.on_stream():
        for _ in range(a.steps):
            m.d_step(x, lab, ln, sync=False)
            m.g_step(x, lab, ln, reuse_g_forward=True, sync=False)
        torch.cuda.synchronize()
    print(json.dumps({"trace": a.trace, "steps": a.steps, "batch_size": B, "frames": T, "device_status": m.engine.device_status()}))
    m.engine.close()
    sys.exit(0)

res = {False: [], True: []}
info = {}
for _ in range(a.runs):
    for bn in (False, True):
        ms, launches, status, losses = one_run(bn)
        res[bn].append(round(ms, 3))
        info[bn] = (launches, status, losses)
for bn in (False, True):
    v = sorted(res[bn])
    print(json.dumps({"workload": "GAN_RNN lstm 1 D + 1 G step", "batch_norm": bn, "batch_size": B, "frames": T, "input_dim": a.dim,
                      "output_dim": a.out_dim, "steps": a.steps, "warmup": a.warmup, "ms_per_step_runs": res[bn],
                      "ms_per_step_median": v[len(v) // 2], "spread_ms": round(v[-1] - v[0], 3),
                      "recurrence_launches_per_step": info[bn][0], "device_status": info[bn][1], "g_losses_last_step": info[bn][2]}))
