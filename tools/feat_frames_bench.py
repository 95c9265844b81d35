"""The frame-level recipes' feature front end on the host (io.FrameBatchReader: a shuffle queue of spliced frames) against on the device
(--device_features: FrameBatchReader(device_features=True) + HipEngine.featurize_frames, csrc/feat.hip k_feat_frames).  Two measurements,
both on the GPU; arks and statistics are written from a seed with ArkWriter into a temporary directory.

  kernel   rsrgan_feat_frames alone at D = 257, context 5 / 5, N = 256 (the shipped batch) and N = 6400 (the benched batch): windows of
           back-to-back launches between two device events (--launches per window, --windows windows, after a warm-up), eight output
           buffers in rotation.  Four variants per N: the gather from a NORMALISED pool (mean = NULL, the product path), the gather from a
           raw pool with statistics (eleven double divisions per raw element), and rsrgan_feat_batch on the same number of output bytes
           (B x T = N) without and with statistics.  Achieved bytes/s = the ALGORITHMIC bytes (out written once; every source row that
           is read at all, the table and the statistics read once) over the time, next to the 6.29 TB/s a float4 copy reaches.  At
           N = 256 the output is 2.9 MB and eight buffers stay in the last-level cache: that shape measures the LAUNCH, not the memory.
  loop     run_gan_dnn._one_epoch (training) with the reference DNN generator and discriminator_dnn at the shipped configuration
           (run_gan_dnn.sh: batch 256, context 5 / 5, num_threads 32, batch norm, 1 D-run + 1 G-run, a fresh batch per run) on
           --utts utterances of 400 .. 899 frames: wall time of one pass per batch, after a warm-up.  Variants: the host reader of the tree
           under --parent_root (a build of the parent commit; without it: this tree's own host path) and this tree with device_features.
           Every variant runs in a fresh child process, the variants ALTERNATE (--repeats rounds); the report gives every run, the median
           and the spread.  Each child also reports what bounds its loop -- the reader alone (no device) and the GPU steps alone (a
           resident batch) --, the pool's high-water pool_rows and bytes, and the 7 averages of the pass: the variants must agree on them
           bit for bit.

Usage: python tools/feat_frames_bench.py [--parent_root DIR] [--out profiles/feat_frames.txt] [--repeats 3]
       python tools/feat_frames_bench.py --mode kernel | --mode loop --root DIR --device_features 0|1 --data DIR   (what the driver runs)"""
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
ap.add_argument("--parent_root", type=str, default=None, help="a built tree of the parent commit: its host reader is the baseline")
ap.add_argument("--device_features", type=int, default=0)
ap.add_argument("--data", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--dim", type=int, default=257)
ap.add_argument("--out_dim", type=int, default=40)
ap.add_argument("--context", type=int, default=5)
ap.add_argument("--num_threads", type=int, default=32)
ap.add_argument("--utts", type=int, default=60)
ap.add_argument("--repeats", type=int, default=3, help="rounds of alternating children (loop)")
ap.add_argument("--launches", type=int, default=400, help="launches per timed window (kernel), at least 200")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--timeout", type=int, default=280, help="seconds a child may take")
a = ap.parse_args()
HBM_COPY = 6.29e12


def write_data(d):
    sys.path.insert(0, HERE)
    from rsrgan_amd.io import ArkWriter
    rng = np.random.default_rng(0)
    wi, wl = ArkWriter(os.path.join(d, "in.scp")), ArkWriter(os.path.join(d, "lab.scp"))
    for i in range(a.utts):
        n = int(rng.integers(400, 900))
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
    D, ctx = a.dim, a.context
    Dout = D * (2 * ctx + 1)
    s = torch.cuda.current_stream()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rng = np.random.default_rng(1)
    mean = torch.from_numpy(rng.standard_normal(D)).to(dev); std = torch.from_numpy(rng.uniform(0.5, 2.0, D)).to(dev)
    # the pool: 64 utterances of 400 .. 899 frames in slots of 4-row units, as the reader lays them out
    lens = rng.integers(400, 900, 64)
    firsts = np.concatenate([[0], np.cumsum((lens + 3) // 4 * 4)])
    pool_rows = int(firsts[-1])
    pool = torch.from_numpy(rng.standard_normal((pool_rows, D), dtype=np.float32)).to(dev)
    for N, (B, T) in ((256, (4, 64)), (6400, (64, 100))):
        u = rng.integers(0, 64, N)
        picks_h = np.stack([firsts[u] + (rng.random(N) * lens[u]).astype(np.int64), firsts[u], firsts[u] + lens[u]], 1).astype(np.int32)
        picks = torch.from_numpy(picks_h).to(dev)
        idx = np.clip(picks_h[:, :1] + np.arange(-ctx, ctx + 1)[None, :], picks_h[:, 1:2], picks_h[:, 2:3] - 1)
        src_rows = int(np.unique(idx).size)                              # source rows that are read at all
        n = rng.integers(T - 10, T + 1, size=B); n[0] = T
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(n)]).astype(np.int32)).to(dev)
        raw_rows = int(n.sum())
        raw = torch.from_numpy(rng.standard_normal((raw_rows, D), dtype=np.float32)).to(dev)
        outs = [torch.empty(N, Dout, dtype=torch.float32, device=dev) for _ in range(8)]        # 8 x 72 MB at N = 6400: past the 256 MB cache
        out_bytes = outs[0].numel() * 4

        def frames(m, sd):
            return lambda o: lib.rsrgan_feat_frames(p(pool), pool_rows, p(picks), N, D, ctx, ctx, p(m), p(sd), p(o), C.c_void_p(s.cuda_stream))

        def batch(m, sd):
            return lambda o: lib.rsrgan_feat_batch(p(raw), raw_rows, p(off), B, T, D, ctx, ctx, p(m), p(sd), p(o), None, C.c_void_p(s.cuda_stream))
        stat_bytes = 2 * D * 8
        variants = [("k_feat_frames<null>", frames(None, None), out_bytes + src_rows * D * 4 + N * 12),
                    ("k_feat_frames<norm>", frames(mean, std), out_bytes + src_rows * D * 4 + N * 12 + stat_bytes),
                    ("k_feat_batch<null>", batch(None, None), out_bytes + raw.numel() * 4 + off.numel() * 4),
                    ("k_feat_batch<norm>", batch(mean, std), out_bytes + raw.numel() * 4 + off.numel() * 4 + stat_bytes)]
        for name, call, nbytes in variants:
            def go(k):
                for i in range(k):
                    rc = call(outs[i & 7])
                    assert rc == 0, lib.rsrgan_last_error()
            go(50)
            torch.cuda.synchronize()
            us = []
            for _ in range(a.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s); go(a.launches); e1.record(s)
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / a.launches)
            v = sorted(us)
            med = v[len(v) // 2]
            print(json.dumps({"measurement": "kernel", "kernel": name, "N": N, "B_x_T": [B, T] if "batch" in name else None, "D": D, "left": ctx,
                              "right": ctx, "Dout": Dout, "pool_rows": pool_rows if "frames" in name else raw_rows,
                              "source_rows_read": src_rows if "frames" in name else raw_rows, "launches_per_window": a.launches,
                              "us_per_launch_windows": [round(x, 3) for x in us], "us_per_launch_median": round(med, 3),
                              "spread_us": round(v[-1] - v[0], 3), "algorithmic_bytes": nbytes, "achieved_TBps": round(nbytes / med / 1e6, 3),
                              "share_of_float4_copy_6.29": round(nbytes / med / 1e6 / 6.29, 3),
                              "launch_bound_shape": N == 256, "checksum": float(outs[0].double().sum().item())}), flush=True)


def loop_mode():
    import torch
    sys.path.insert(0, a.root)
    from rsrgan_amd import GAN
    from rsrgan_amd import run_gan_dnn as RD
    from rsrgan_amd.io import FrameBatchReader
    assert torch.cuda.is_available(), "the loop measurement needs the GPU"
    N, ctx = a.batch, a.context
    FLAGS = SimpleNamespace(batch_size=N, input_dim=a.dim, output_dim=a.out_dim, left_context=ctx, right_context=ctx, g_type="dnn", keep_prob=1.0,
                            batch_norm=True, num_gpu=1, save_dir=None, l2_scale=1e-5, g_learning_rate=1e-4, d_learning_rate=1e-4,
                            init_mse_weight=1.0, init_disc_noise_std=0.0, disc_updates=1, gen_updates=1, num_threads=a.num_threads)
    m = GAN(None, FLAGS, ["gpu:0"])
    cmvn = np.load(os.path.join(a.data, "train_cmvn.npz"))
    kw = dict(device_features=True) if a.device_features else {}
    mk = lambda: FrameBatchReader(os.path.join(a.data, "in.scp"), os.path.join(a.data, "lab.scp"), N, ctx, ctx, cmvn=cmvn, num_threads=a.num_threads,
                                  shuffle=True, seed=1234, **kw)
    if a.device_features:
        from rsrgan_amd.train import device_frames
        feed = lambda r: device_frames(m, r)
    else:
        feed = lambda r: r
    quiet = lambda *_: None
    RD._one_epoch(m, feed(mk()), 8, 0, FLAGS, True, quiet)              # warm-up: code objects, the page cache of the arks
    torch.cuda.synchronize()
    reader = mk()
    nb = reader.num_batches()
    t0 = time.perf_counter()
    res = RD._one_epoch(m, feed(reader), nb, 1, FLAGS, True, quiet)      # (every run ends in a device-to-host copy of its losses)
    torch.cuda.synchronize()
    ran = 2 * int(nb / 2)
    loop_ms = (time.perf_counter() - t0) * 1e3 / ran
    pool = m.engine.frame_pool_stats(reader.reader_id) if a.device_features else None
    # what bounds the loop: the reader alone (no device) ...
    t0 = time.perf_counter()
    k = 0
    for item in mk():
        k += 1
        if k == ran:
            break
    reader_ms = (time.perf_counter() - t0) * 1e3 / k
    # ... and the GPU steps alone, on a resident batch (per batch: a D-run and a G-run take one each)
    it = iter(feed(mk()))
    x, lab = next(it)
    if not isinstance(x, torch.Tensor):
        x, lab = torch.from_numpy(x).to(m.engine.device), torch.from_numpy(lab).to(m.engine.device)
    step = []
    for i in range(60):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.d_step(x, lab, train=True)
        m.g_step(x, lab, train=True)
        if i >= 20:
            step.append((time.perf_counter() - t0) * 1e3 / 2)
    print(json.dumps({"measurement": "loop", "root": os.path.relpath(a.root, HERE), "device_features": bool(a.device_features), "N": N,
                      "context": ctx, "num_threads": a.num_threads, "queue_capacity": reader.capacity, "batches": ran,
                      "ms_per_batch": round(loop_ms, 3), "reader_alone_ms_per_batch": round(reader_ms, 3),
                      "gpu_steps_alone_ms_per_batch": round(float(np.median(step)), 3), "pool": pool,
                      "averages_of_the_pass": [float(r) for r in res]}), flush=True)
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
    common = ["--batch", str(a.batch), "--dim", str(a.dim), "--out_dim", str(a.out_dim), "--context", str(a.context), "--num_threads",
              str(a.num_threads), "--utts", str(a.utts), "--launches", str(a.launches), "--windows", str(a.windows)]
    lines = []

    def emit(o):
        lines.append(json.dumps(o))
        print(lines[-1], flush=True)
    for o in child(["--mode", "kernel"] + common):
        emit(o)
    base_root = a.parent_root or HERE
    variants = [("host reader, parent commit" if a.parent_root else "host reader, this tree", base_root, 0), ("device_features, this tree", HERE, 1)]
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
    med = lambda v: sorted(v)[len(v) // 2]
    for name, rs in runs.items():
        v = [r["ms_per_batch"] for r in rs]
        summary[name] = {"ms_per_batch_runs": v, "median": med(v), "spread": round(max(v) - min(v), 3),
                         "reader_alone_ms_per_batch": med([r["reader_alone_ms_per_batch"] for r in rs]),
                         "gpu_steps_alone_ms_per_batch": med([r["gpu_steps_alone_ms_per_batch"] for r in rs])}
    (h, hs), (dv, ds) = [(summary[n]["median"], summary[n]["spread"]) for n, _, _ in variants]
    summary["host_over_device"] = round(h / dv, 3)
    summary["faster_by_more_than_the_spreads"] = bool(h - dv > max(hs, ds))
    summary["device_loop_over_gpu_steps_alone"] = round(dv / summary[variants[1][0]]["gpu_steps_alone_ms_per_batch"], 3)
    summary["pool_high_water"] = runs[variants[1][0]][-1]["pool"]
    avgs = [r["averages_of_the_pass"] for rs in runs.values() for r in rs]
    summary["every_run_gave_the_same_averages"] = all(v == avgs[0] for v in avgs)
    emit(summary)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/feat_frames_bench.py on an MI355X (gfx950): the frame-level feature front end on the host against csrc/feat.hip\n"
                    "k_feat_frames (see the tool's docstring for what each line measures).  One JSON object per line: the kernels at both\n"
                    "sizes, every loop run in the order it ran, the summary.\n")
            f.write("\n".join(lines) + "\n")


{"driver": driver, "kernel": kernel_mode, "loop": loop_mode}[a.mode]()
