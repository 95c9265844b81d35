"""Kaldi-compressed archives through the host reader against the device decode (csrc/feat.hip k_feat_decode, --device_decode), at the
recipe's sizes: D = 257 inputs and 40 labels, context 5 / 5, B = 64, utterances of --frames frames (default: 100 and 500).  The archives
are written from a seed into a temporary directory with the format-1 encoder of tests/feat_decode_ref.py.  Record only, no threshold.

  host     PaddedBatchReader.materialize with device_features=False -- the only route the parent commit has for such archives: read,
           decode to float64, CMVN, splice, pad.  Seconds per batch on one host thread (best and median of --host_repeats) and the bytes
           of the expanded batch it uploads.
  coded    the same reader with device_decode=True: seconds per batch (file reads and one copy of the bytes) and the bytes it ships
           (blob + tables, inputs and labels).
  device   rsrgan_feat_decode + rsrgan_feat_batch(mean = NULL) for the inputs and for the labels, the four launches between two device
           events, on resident tensors: median of --rounds rounds after a warm-up; and the same for the decode launches alone.
  step     one training step (1 D-run + 2 G-runs of GAN_RNN on the reference's nets, a resident batch), wall time between device
           synchronisations, median: what the device time is a share of.  --step 0 leaves it out.

Usage: python tools/feat_decode_bench.py [--out profiles/feat_decode.txt] [--frames 100 500]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--frames", type=int, nargs="+", default=[100, 500])
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--dim", type=int, default=257)
ap.add_argument("--out_dim", type=int, default=40)
ap.add_argument("--context", type=int, default=5)
ap.add_argument("--host_repeats", type=int, default=5)
ap.add_argument("--rounds", type=int, default=40, help="timed rounds of the device launches (at least 20)")
ap.add_argument("--step", type=int, default=1, help="also time a training step on the reference's nets")
a = ap.parse_args()


def write_data(d, frames):
    from tests import feat_decode_ref as R
    rng = np.random.default_rng(frames)
    xs = [("utt%04d" % i, rng.standard_normal((frames, a.dim)) * 2 + 1, "C") for i in range(a.batch)]
    ys = [("utt%04d" % i, rng.standard_normal((frames, a.out_dim)) - 1, "C") for i in range(a.batch)]
    R.write_archive(os.path.join(d, "in.ark"), os.path.join(d, "in.scp"), xs)
    R.write_archive(os.path.join(d, "lab.ark"), os.path.join(d, "lab.scp"), ys)
    return {"mean_inputs": rng.standard_normal(a.dim), "stddev_inputs": rng.uniform(0.5, 2.0, a.dim),
            "mean_labels": rng.standard_normal(a.out_dim), "stddev_labels": rng.uniform(0.5, 2.0, a.out_dim)}


def timed(f, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        r = f()
        out.append(time.perf_counter() - t0)
    return r, out


def measure(frames, emit):
    import torch
    from rsrgan_amd import _lib
    from rsrgan_amd.io import PaddedBatchReader
    B, ctx = a.batch, a.context
    with tempfile.TemporaryDirectory() as d:
        cmvn = write_data(d, frames)
        mk = lambda **k: PaddedBatchReader(os.path.join(d, "in.scp"), os.path.join(d, "lab.scp"), B, ctx, ctx, cmvn=cmvn, num_buckets=1,
                                           shuffle=False, **k)
        host, coded = mk(), mk(device_decode=True)
        plan = next(iter(host.plan()))
        assert len(plan) == B
        host.materialize(plan); coded.materialize(plan)                     # (the page cache of the archives)
        hi, ht = timed(lambda: host.materialize(plan), a.host_repeats)
        ci, ct = timed(lambda: coded.materialize(plan), a.host_repeats)
    emit({"measurement": "host", "frames": frames, "B": B, "s_per_batch_best": round(min(ht), 5), "s_per_batch_median": round(float(np.median(ht)), 5),
          "s_per_utterance_best": round(min(ht) / B, 6), "bytes_uploaded": int(hi[1].nbytes + hi[2].nbytes + hi[3].nbytes)})
    emit({"measurement": "coded", "frames": frames, "B": B, "s_per_batch_best": round(min(ct), 5), "s_per_batch_median": round(float(np.median(ct)), 5),
          "bytes_shipped": int(ci[1].nbytes() + ci[2].nbytes()), "raw_float32_bytes": int(4 * B * frames * (a.dim + a.out_dim))})
    assert torch.cuda.is_available(), "the device measurement needs the GPU"
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    sides = []
    for cb, c in ((ci[1], ctx), (ci[2], 0)):
        t = SimpleNamespace(D=cb.dim, ctx=c, rows=int(cb.offsets[-1]), T=cb.shape[1])
        t.blob, t.seg, t.scale, t.off = (torch.from_numpy(v).to(dev) for v in (cb.blob, cb.seg, cb.scale, cb.offsets))
        t.mean, t.std = torch.from_numpy(cb.mean).to(dev), torch.from_numpy(cb.stddev).to(dev)
        t.raw = torch.empty(t.rows, t.D, dtype=torch.float32, device=dev)
        t.out = torch.empty(B, t.T, t.D * (2 * c + 1), dtype=torch.float32, device=dev)
        t.ln = torch.empty(B, dtype=torch.int32, device=dev)
        sides.append(t)

    def go(splice):
        for t in sides:
            rc = lib.rsrgan_feat_decode(p(t.blob), t.blob.numel(), p(t.seg), p(t.scale), p(t.off), B, t.D, p(t.mean), p(t.std), p(t.raw), t.rows,
                                        C.c_void_p(s.cuda_stream))
            assert rc == 0, lib.rsrgan_last_error()
            if splice:
                rc = lib.rsrgan_feat_batch(p(t.raw), t.rows, p(t.off), B, t.T, t.D, t.ctx, t.ctx, None, None, p(t.out), p(t.ln), C.c_void_p(s.cuda_stream))
                assert rc == 0, lib.rsrgan_last_error()
    res = {}
    for name, splice in (("decode+splice", True), ("decode", False)):
        for _ in range(10):
            go(splice)
        torch.cuda.synchronize()
        us = []
        for _ in range(max(a.rounds, 20)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s); go(splice); e1.record(s)
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        v = sorted(us)
        res[name] = {"us_median": round(v[len(v) // 2], 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2), "rounds": len(v)}
    # the device result is the host's: the measured launches computed the batch the host reader made
    same = all(np.array_equal(t.out.cpu().numpy().view(np.int32), np.ascontiguousarray(w).view(np.int32)) for t, w in zip(sides, (hi[1], hi[2])))
    o = {"measurement": "device", "frames": frames, "B": B, "launches": "k_feat_decode + k_feat_batch, inputs (D %d, context %d/%d) and labels (D %d)" % (
        a.dim, ctx, ctx, a.out_dim), "equal_to_the_host_batch": bool(same)}
    o.update(res)
    if a.step:
        from rsrgan_amd import GAN_RNN
        args = SimpleNamespace(batch_size=B, input_dim=a.dim, output_dim=a.out_dim, left_context=ctx, right_context=ctx, g_type="lstm",
                               keep_prob=1.0, batch_norm=False, num_gpu=1, save_dir=None, l2_scale=1e-5, g_learning_rate=8e-5,
                               d_learning_rate=1e-3, init_mse_weight=10.0, init_disc_noise_std=0.0, disc_updates=1, gen_updates=2)
        m = GAN_RNN(None, args, ["gpu:0"], max_frames=frames)
        x, lab, ln = sides[0].out, sides[1].out, sides[0].ln
        step = []
        with m.on_stream():
            for i in range(20):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.d_step(x, lab, ln, sync=False, gather=False)
                m.g_step(x, lab, ln, reuse_g_forward=True, sync=False, gather=False)
                m.g_step(x, lab, ln, sync=False, gather=False)
                torch.cuda.synchronize()
                if i >= 8:
                    step.append((time.perf_counter() - t0) * 1e3)
        o["training_step_ms_median"] = round(float(np.median(step)), 3)
        o["device_status"] = m.engine.device_status()
        o["share_of_a_training_step"] = round(res["decode+splice"]["us_median"] / 1e3 / o["training_step_ms_median"], 4)
        m.engine.close()
    emit(o)


def main():
    lines = []

    def emit(o):
        lines.append(json.dumps(o))
        print(lines[-1], flush=True)
    for frames in a.frames:
        measure(frames, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/feat_decode_bench.py on an MI355X (gfx950): Kaldi-compressed archives through the host reader against the device decode\n"
                    "(see the tool's docstring for what each line measures).  One JSON object per line; host times are of the GPU machine's CPU.\n")
            f.write("\n".join(lines) + "\n")


main()
