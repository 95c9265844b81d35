"""ms per supervised step of RNNTrainer(g_type='bnlstm') at the shape run_rnn.sh trains with (--g_type bnlstm in place of lstm):
batch_size 8 per GPU, input_dim = output_dim = 40, T = 100, 3 x BNLSTMCell(760, num_proj=280); launch sequence replayed as a
hipGraph.  Prints one JSON line.  Usage: python tools/bnlstm_step.py [--steps N] [--warmup W] [--batch B] [--frames T]"""
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
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--frames", type=int, default=100)
a = ap.parse_args()
B, T, D = a.batch, a.frames, 40
args = SimpleNamespace(batch_size=B, input_dim=D, output_dim=D, left_context=0, right_context=0, g_type="bnlstm", keep_prob=1.0,
                       batch_norm=False, num_gpu=1, save_dir=None, l2_scale=1e-5, g_learning_rate=2e-4)
m = RNNTrainer(None, args, ["gpu:0"], max_frames=T, net_overrides=dict(flags=1 | 2))
rng = np.random.default_rng(0)
dev = m.engine.device
x = torch.tensor(rng.standard_normal((B, T, D)).astype(np.float32), device=dev)
lab = torch.tensor(rng.standard_normal((B, T, D)).astype(np.float32), device=dev)
ln = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
ln[0] = T
ln = torch.tensor(ln, device=dev)
with m.on_stream():
    for _ in range(a.warmup):
        m.step(x, lab, ln, sync=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = m.step(x, lab, ln, sync=False)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
print(json.dumps({"workload": "RNNTrainer bnlstm supervised step", "batch_size": B, "frames": T, "input_dim": D, "output_dim": D,
                  "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt * 1e3, 3),
                  "losses_last_step": [float(v) for v in out.reshape(-1).cpu().numpy()]}))
