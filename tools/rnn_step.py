"""ms per supervised step of RNNTrainer for one or more sequence generators at one shape, measured side by side: the runs of the listed
g_types alternate (a, b, a, b, ...), each run on a fresh handle, launch sequence replayed as a hipGraph (as tools/bnlstm_step.py).
Prints one JSON line per g_type: every run's ms_per_step, their median and spread (max - min).

Usage: python tools/rnn_step.py [--g_types res_lstm_i,res_lstm_base] [--layers 2] [--cells 760] [--proj 257] [--dim 257]
                                [--batch 8] [--frames 100] [--steps 30] [--warmup 5] [--runs 3]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rsrgan_amd.trainer import RNNTrainer      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--g_types", type=str, default="res_lstm_i,res_lstm_base")
ap.add_argument("--layers", type=int, default=2)
ap.add_argument("--cells", type=int, default=760)
ap.add_argument("--proj", type=int, default=257)
ap.add_argument("--dim", type=int, default=257, help="input_dim (res_lstm_i / res_lstm_l need it equal to --proj)")
ap.add_argument("--out_dim", type=int, default=40)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
a = ap.parse_args()
B, T = a.batch, a.frames
rng = np.random.default_rng(0)
xh = rng.standard_normal((B, T, a.dim)).astype(np.float32)
labh = rng.standard_normal((B, T, a.out_dim)).astype(np.float32)
lnh = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
lnh[0] = T


def one_run(g_type):
    args = SimpleNamespace(batch_size=B, input_dim=a.dim, output_dim=a.out_dim, left_context=0, right_context=0, g_type=g_type,
                           keep_prob=1.0, batch_norm=False, num_gpu=1, save_dir=None, l2_scale=1e-5, g_learning_rate=2e-4)
    m = RNNTrainer(None, args, ["gpu:0"], max_frames=T,
                   net_overrides=dict(flags=1 | 2, g_layers=a.layers, g_cells=a.cells, g_proj=a.proj))
    dev = m.engine.device
    x, lab, ln = torch.tensor(xh, device=dev), torch.tensor(labh, device=dev), torch.tensor(lnh, device=dev)
    with m.on_stream():
        for _ in range(a.warmup):
            m.step(x, lab, ln, sync=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            out = m.step(x, lab, ln, sync=False)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        m.engine.profile_begin()                 # (one more step, outside the timing: which launches it took)
        m.step(x, lab, ln, sync=False)
        torch.cuda.synchronize()
    kinds = {str(k): m.engine.profile_read_kind(k)[0] for k in (1, 2)}
    m.engine.profile_read()
    status = m.engine.device_status()
    losses = [float(v) for v in out.reshape(-1).cpu().numpy()]
    m.engine.close()
    return dt * 1e3, kinds, status, losses


types = a.g_types.split(",")
res = {t: [] for t in types}
info = {}
for _ in range(a.runs):
    for t in types:
        ms, kinds, status, losses = one_run(t)
        res[t].append(round(ms, 3))
        info[t] = (kinds, status, losses)
for t in types:
    v = sorted(res[t])
    print(json.dumps({"workload": "RNNTrainer %s supervised step" % t, "g_layers": a.layers, "g_cells": a.cells, "g_proj": a.proj,
                      "input_dim": a.dim, "output_dim": a.out_dim, "batch_size": B, "frames": T, "steps": a.steps, "warmup": a.warmup,
                      "ms_per_step_runs": res[t], "ms_per_step_median": v[len(v) // 2], "spread_ms": round(v[-1] - v[0], 3),
                      "persistent_launches_last_run": info[t][0], "device_status": info[t][1], "losses_last_step": info[t][2]}))
