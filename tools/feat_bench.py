"""The feature front end (CMVN, context splice, padding) on the host against on the device (csrc/feat.hip, --device_features).  Two
measurements, both on the GPU; arks and statistics are written from a seed with ArkWriter into a temporary directory.

  kernel   rsrgan_feat_batch alone: windows of back-to-back launches between two device events (--launches per window, --windows
           windows, after a warm-up), at D = 257, context 5 / 5, B = 64, T = 100 and at D = 40, context 0 / 0, same B and T, with
           CMVN.  Achieved bytes/s = the ALGORITHMIC bytes (out written once, raw, offsets and statistics read once) over the time, next
           to the HBM peak (8.0 TB/s spec, 6.29 TB/s measured with a float4 copy) and the 4.9 TB/s of this project's own elementwise
           kernels.  The 11-fold re-read of raw is served by the caches and is not counted.
  loop     train_one_iteration of GAN_RNN on the reference's nets (lstm 3 x 760 / 280, discriminator 2 x 256 / 40, 1 D + 2 G updates)
           at B = 64, T about 100 (utterances of 90 .. 99 frames), context 5 / 5, fed by prefetch(PaddedBatchReader) as
           run_gan_rnn.train feeds it: wall time of whole iterations (they end in a device-to-host copy of the losses) after one
           warm-up iteration, per batch.  Variants: the host path of the tree under --parent_root (a build of the parent commit; without
           it: this tree's own host path) and this tree with device_features.  Every variant runs in a fresh child process, the variants
           ALTERNATE (--repeats rounds), and the report gives every run, the median and the spread.  Each child also reports what
           bounds its loop: the reader alone (no device) and the GPU step alone (a resident batch), and the 7 averages of its last
           iteration -- the variants must agree on them bit for bit.

Usage: python tools/feat_bench.py [--parent_root DIR] [--out profiles/feat_frontend.txt] [--batches 12] [--repeats 3]
       python tools/feat_bench.py --mode kernel | --mode loop --root DIR --device_features 0|1 --data DIR   (what the driver runs)"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("driver", "kernel", "loop"), default="driver")
ap.add_argument("--root", type=str, default=HERE, help="tree to import rsrgan_amd from (loop mode)")
ap.add_argument("--parent_root", type=str, default=None, help="a built tree of the parent commit: its host path is the baseline")
ap.add_argument("--device_features", type=int, default=0)
ap.add_argument("--data", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--dim", type=int, default=257)
ap.add_argument("--out_dim", type=int, default=40)
ap.add_argument("--context", type=int, default=5)
ap.add_argument("--batches", type=int, default=12, help="batches per iteration (loop)")
ap.add_argument("--iters", type=int, default=3, help="timed iterations per child (loop)")
ap.add_argument("--repeats", type=int, default=3, help="rounds of alternating children (loop)")
ap.add_argument("--launches", type=int, default=400, help="launches per timed window (kernel), at least 200")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
a = ap.parse_args()
HBM_SPEC, HBM_COPY, OWN_ELEMENTWISE = 8.0e12, 6.29e12, 4.9e12


def write_data(d):
    """B x batches utterances of frames - 10 .. frames - 1 frames, inputs [n, dim] and labels [n, out_dim], and train_cmvn.npz"""
    sys.path.insert(0, HERE)
    from rsrgan_amd.io import ArkWriter
    rng = np.random.default_rng(0)
    wi, wl = ArkWriter(os.path.join(d, "in.scp")), ArkWriter(os.path.join(d, "lab.scp"))
    for i in range(a.batch * a.batches):
        n = int(rng.integers(a.frames - 10, a.frames))                 # (one length bucket of the reader: (n - 200) // 50 is the same for all)
        wi.write_next_utt(os.path.join(d, "in.ark"), "utt%05d" % i, rng.standard_normal((n, a.dim), dtype=np.float32) * 2 + 1)
        wl.write_next_utt(os.path.join(d, "lab.ark"), "utt%05d" % i, rng.standard_normal((n, a.out_dim), dtype=np.float32) - 1)
    wi.close(); wl.close()
    np.savez(os.path.join(d, "train_cmvn.npz"), mean_inputs=rng.standard_normal(a.dim), stddev_inputs=rng.uniform(0.5, 2.0, a.dim),
             mean_labels=rng.standard_normal(a.out_dim), stddev_labels=rng.uniform(0.5, 2.0, a.out_dim))


def kernel_mode():
    import ctypes as C
    import torch
    sys.path.insert(0, a.root)
    from rsrgan_amd import _lib
    assert torch.cuda.is_available(), "the kernel measurement needs the GPU"
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    assert a.launches >= 200
    for D, ctx in ((a.dim, a.context), (a.out_dim, 0)):
        B, T = a.batch, a.frames
        rng = np.random.default_rng(1)
        n = rng.integers(T - 10, T + 1, size=B); n[0] = T
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(n)]).astype(np.int32)).to(dev)
        rows = int(n.sum())
        raw = torch.from_numpy(rng.standard_normal((rows, D), dtype=np.float32)).to(dev)
        mean = torch.from_numpy(rng.standard_normal(D)).to(dev); std = torch.from_numpy(rng.uniform(0.5, 2.0, D)).to(dev)
        Dout = D * (2 * ctx + 1)
        # eight output buffers in rotation: 8 x 72 MB is more than the 256 MB last-level cache holds, so the stores of the large shape go
        # to HBM (the small shape's 8 x 1 MB stay cached: that shape measures the launch, not the memory)
        outs = [torch.empty(B, T, Dout, dtype=torch.float32, device=dev) for _ in range(8)]
        out, ln = outs[0], torch.empty(B, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream()
        p = lambda t: C.c_void_p(t.data_ptr())

        def go(k):
            for i in range(k):
                rc = lib.rsrgan_feat_batch(p(raw), rows, p(off), B, T, D, ctx, ctx, p(mean), p(std), p(outs[i & 7]), p(ln), C.c_void_p(s.cuda_stream))
                assert rc == 0, lib.rsrgan_last_error()
        go(50)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s); go(a.launches); e1.record(s)
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.launches)
        nbytes = out.numel() * 4 + raw.numel() * 4 + off.numel() * 4 + 2 * D * 8 + B * 4
        v = sorted(us)
        med = v[len(v) // 2]
        print(json.dumps({"measurement": "kernel", "kernel": "k_feat_batch<cmvn>", "D": D, "left": ctx, "right": ctx, "B": B, "T": T, "Dout": Dout,
                          "launches_per_window": a.launches, "us_per_launch_windows": [round(x, 3) for x in us], "us_per_launch_median": round(med, 3),
                          "spread_us": round(v[-1] - v[0], 3), "algorithmic_bytes": nbytes, "achieved_TBps": round(nbytes / med / 1e6, 3),
                          "share_of_hbm_spec_8.0": round(nbytes / med / 1e6 / 8.0, 3), "share_of_float4_copy_6.29": round(nbytes / med / 1e6 / 6.29, 3),
                          "vs_own_elementwise_4.9": round(nbytes / med / 1e6 / 4.9, 3), "checksum": float(out.double().sum().item())}), flush=True)


def loop_mode():
    import torch
    sys.path.insert(0, a.root)
    from rsrgan_amd import GAN_RNN, train_one_iteration
    from rsrgan_amd.io import PaddedBatchReader, prefetch
    assert torch.cuda.is_available(), "the loop measurement needs the GPU"
    B, T, ctx = a.batch, a.frames, a.context
    args = SimpleNamespace(batch_size=B, input_dim=a.dim, output_dim=a.out_dim, left_context=ctx, right_context=ctx, g_type="lstm",
                           keep_prob=1.0, batch_norm=False, num_gpu=1, save_dir=None, l2_scale=1e-5, g_learning_rate=8e-5,
                           d_learning_rate=1e-3, init_mse_weight=10.0, init_disc_noise_std=0.0, disc_updates=1, gen_updates=2)
    m = GAN_RNN(None, args, ["gpu:0"], max_frames=T)
    cmvn = np.load(os.path.join(a.data, "train_cmvn.npz"))
    kw = dict(device_features=True) if a.device_features else {}
    mk = lambda: PaddedBatchReader(os.path.join(a.data, "in.scp"), os.path.join(a.data, "lab.scp"), B, ctx, ctx, cmvn=cmvn, shuffle=True,
                                   seed=1234, **kw)
    reader = mk()
    plan = list(mk().plan())
    nb, full = len(plan), sum(1 for w in plan if len(w) == B)         # (the loop skips partial windows: the time is per TRAINED batch)
    train_one_iteration(None, m, nb, 0, prefetch(reader))             # warm-up: code objects, graph capture, the page cache of the arks
    torch.cuda.synchronize()
    ms, res = [], None
    for it in range(a.iters):
        t0 = time.perf_counter()
        res = train_one_iteration(None, m, nb, it + 1, prefetch(reader))          # (returns the losses: a device-to-host copy ends it)
        ms.append((time.perf_counter() - t0) * 1e3 / full)
    # what bounds the loop: the reader alone ...
    t0 = time.perf_counter()
    items = list(mk())
    reader_ms = (time.perf_counter() - t0) * 1e3 / len(items)
    # ... and the GPU step alone, on a resident expanded batch
    item = items[0]
    if a.device_features:
        from rsrgan_amd.train import device_batch
        x, lab, ln = device_batch(m, item[1], item[2], item[3])
    else:
        dev = m.engine.device
        x, lab, ln = torch.from_numpy(item[1]).to(dev), torch.from_numpy(item[2]).to(dev), torch.from_numpy(item[3]).to(dev)
    step = []
    with m.on_stream():
        for i in range(30):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.d_step(x, lab, ln, sync=False, gather=False)
            m.g_step(x, lab, ln, reuse_g_forward=True, sync=False, gather=False)
            m.g_step(x, lab, ln, sync=False, gather=False)
            torch.cuda.synchronize()
            if i >= 10:
                step.append((time.perf_counter() - t0) * 1e3)
    status = m.engine.device_status()
    v = sorted(ms)
    print(json.dumps({"measurement": "loop", "root": os.path.relpath(a.root, HERE), "device_features": bool(a.device_features), "B": B, "T": T,
                      "context": ctx, "windows_per_iteration": nb, "batches_per_iteration": full, "ms_per_batch_iterations": [round(x, 3) for x in ms],
                      "ms_per_batch_median": round(v[len(v) // 2], 3), "reader_alone_ms_per_batch": round(reader_ms, 3),
                      "gpu_step_alone_ms_per_batch": round(float(np.median(step)), 3), "device_status": status,
                      "averages_last_iteration": [float(r) for r in res]}), flush=True)
    m.engine.close()


def child(extra):
    """one measurement in a fresh process; its JSON lines"""
    cmd = [sys.executable, os.path.abspath(__file__)] + extra
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("child %s ended with status %d: stopping, nothing more is started on the device" % (" ".join(extra), r.returncode))
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def driver():
    common = ["--batch", str(a.batch), "--frames", str(a.frames), "--dim", str(a.dim), "--out_dim", str(a.out_dim), "--context", str(a.context),
              "--batches", str(a.batches), "--iters", str(a.iters), "--launches", str(a.launches), "--windows", str(a.windows)]
    lines = []

    def emit(o):
        lines.append(json.dumps(o))
        print(lines[-1], flush=True)
    for o in child(["--mode", "kernel"] + common):
        emit(o)
    base_root = a.parent_root or HERE
    variants = [("host path, parent commit" if a.parent_root else "host path, this tree", base_root, 0), ("device_features, this tree", HERE, 1)]
    runs = {name: [] for name, _, _ in variants}
    with tempfile.TemporaryDirectory() as d:
        write_data(d)
        for _ in range(a.repeats):
            for name, root, dev in variants:
                o = child(["--mode", "loop", "--root", root, "--device_features", str(dev), "--data", d] + common)[-1]
                o["variant"] = name
                emit(o)
                runs[name].append(o)
    summary = {"measurement": "loop summary", "repeats": a.repeats}
    for name, rs in runs.items():
        v = sorted(r["ms_per_batch_median"] for r in rs)
        summary[name] = {"ms_per_batch_runs": [r["ms_per_batch_median"] for r in rs], "median": v[len(v) // 2], "spread": round(v[-1] - v[0], 3),
                         "reader_alone_ms_per_batch": sorted(r["reader_alone_ms_per_batch"] for r in rs)[len(rs) // 2],
                         "gpu_step_alone_ms_per_batch": sorted(r["gpu_step_alone_ms_per_batch"] for r in rs)[len(rs) // 2]}
    (h, hs), (dv, ds) = [(summary[n]["median"], summary[n]["spread"]) for n, _, _ in variants]
    summary["host_over_device"] = round(h / dv, 3)
    summary["faster_by_more_than_the_spread"] = bool(h - dv > max(hs, ds))
    avgs = [r["averages_last_iteration"] for rs in runs.values() for r in rs]
    summary["every_run_gave_the_same_averages"] = all(v == avgs[0] for v in avgs)
    emit(summary)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/feat_bench.py on an MI355X (gfx950): the feature front end on the host against csrc/feat.hip (see the tool's docstring for what\n"
                    "each line measures).  One JSON object per line: the kernel at both shapes, every loop run in the order it ran, the summary.\n")
            f.write("\n".join(lines) + "\n")


{"driver": driver, "kernel": kernel_mode, "loop": loop_mode}[a.mode]()
