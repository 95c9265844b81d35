"""Model.run_summaries with its histograms on the host (the route of every commit before --device_summaries: three tensors copied to
the host, np.searchsorted over the 1551 limits) against on the device (csrc/hist.hip, five histograms).  All on the GPU, one process:

  summary  wall time of whole run_summaries calls (each ends in a device-to-host copy) on GAN_RNN with the reference's nets, 257-dim
           inputs, context 0, T = 100: the headline shape (lstm, B = 64) and the shipped recipe's (res_lstm_l, batch_size = 8).  The
           two routes ALTERNATE call by call on one model after --warmup calls of each; the median and the spread of --calls calls of
           each are reported, for a batch that is resident on the device (what --device_features feeds) and for a host batch.
  kernel   rsrgan_hist alone on the three tensors of the headline summary (x, labels and a G(x)-sized tensor): windows of back-to-back
           calls between two device events.  Achieved bytes/s = the bytes of the tensors, read once, over the time, next to the HBM
           rate (8.0 TB/s spec, 6.29 TB/s measured with a float4 copy).  Then 2^22 standard-normal values against 2^22 copies of 1.0
           (every lane of every wave in ONE bucket): time per element of each.

Usage: python tools/summary_bench.py [--out profiles/summary_hist.txt] [--calls 30] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--calls", type=int, default=30, help="timed calls of each route (at least 20)")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--launches", type=int, default=100, help="rsrgan_hist calls per timed window")
ap.add_argument("--windows", type=int, default=5)
a = ap.parse_args()
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
lines = []


def emit(**kw):
    lines.append(json.dumps(kw))
    print(lines[-1], flush=True)


def summary_times(net, B):
    import torch
    from rsrgan_amd import GAN_RNN
    T = a.frames
    args = SimpleNamespace(batch_size=B, input_dim=257, output_dim=40, left_context=0, right_context=0, g_type=net, keep_prob=1.0,
                           batch_norm=False, num_gpu=1, save_dir=None, l2_scale=0.0, disc_updates=1, gen_updates=1, init_mse_weight=10.0,
                           init_disc_noise_std=0.0, d_learning_rate=1e-3, g_learning_rate=8e-5)
    model = GAN_RNN(None, args, ["gpu:0"], max_frames=T, seed=4321, net_overrides=dict(flags=3))
    rng = np.random.default_rng(1234)
    host = (rng.standard_normal((B, T, 257)).astype(np.float32), rng.standard_normal((B, T, 40)).astype(np.float32),
            rng.integers(T // 2, T + 1, size=B).astype(np.int32))
    dev = tuple(torch.from_numpy(v).to(model.engine.device) for v in host)
    for feed, batch in (("device-resident batch", dev), ("host batch", host)):
        ms = {False: [], True: []}
        for i in range(a.warmup + max(a.calls, 20)):
            for flag in (False, True):
                model.device_summaries = flag
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                blob = model.run_summaries(*batch)
                dt = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    ms[flag].append(dt)
        off, on = statistics.median(ms[False]), statistics.median(ms[True])
        emit(measurement="summary", net=net, B=B, T=T, feed=feed, calls=len(ms[True]), bytes_of_summary=len(blob),
             host_route_ms_median=round(off, 3), host_route_ms_min_max=[round(min(ms[False]), 3), round(max(ms[False]), 3)],
             device_route_ms_median=round(on, 3), device_route_ms_min_max=[round(min(ms[True]), 3), round(max(ms[True]), 3)],
             host_over_device=round(off / on, 2), device_not_slower=bool(on <= off), device_status=model.engine.device_status())
    model.engine.close()


def window_us(ops, tensors):
    """us per rsrgan_hist call of windows of back-to-back calls.  The host needs longer to make a call than the device to run it, so each
    window is queued behind a plug (a matrix product of some ten milliseconds): the device meets the first event with the whole
    window already in its queue, and the time between the events is the kernels' own."""
    import torch
    out = []
    plug = torch.randn(8192, 8192, device=ops.device)
    for w in range(a.windows + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.mm(plug, plug)
        e0.record()
        for _ in range(a.launches):
            ops.hist(tensors)
        e1.record(); e1.synchronize()
        if w:                                                    # (window 0 warms up)
            out.append(e0.elapsed_time(e1) * 1e3 / a.launches)
    return out


def kernel_times():
    import torch
    from rsrgan_amd.ops import OpEntries
    ops = OpEntries()
    g = torch.Generator(device=ops.device); g.manual_seed(7)
    B, T = 64, a.frames
    ts = [torch.randn(B, T, 257, device=ops.device, generator=g), torch.randn(B, T, 40, device=ops.device, generator=g),
          torch.randn(B, T, 40, device=ops.device, generator=g)]
    us = window_us(ops, ts)
    nbytes = sum(t.numel() for t in ts) * 4
    med = statistics.median(us)
    emit(measurement="kernel", what="rsrgan_hist of x [64,100,257], labels and G(x) [64,100,40]: k_hist + k_hist_finish per call",
         launches_per_window=a.launches, us_per_call_windows=[round(v, 3) for v in us], us_per_call_median=round(med, 3), bytes_read=nbytes,
         achieved_TBps=round(nbytes / med * 1e-6, 3), share_of_hbm_spec_8_0=round(nbytes / med * 1e6 / HBM_SPEC, 3),
         share_of_float4_copy_6_29=round(nbytes / med * 1e6 / HBM_COPY, 3))
    n = 1 << 22
    normal, ones = torch.randn(n, device=ops.device, generator=g), torch.ones(n, device=ops.device)
    un, uo = statistics.median(window_us(ops, [normal])), statistics.median(window_us(ops, [ones]))
    emit(measurement="contention", elements=n, normal_sample_us_per_call=round(un, 3), one_bucket_us_per_call=round(uo, 3),
         normal_ps_per_element=round(un / n * 1e6, 3), one_bucket_ps_per_element=round(uo / n * 1e6, 3), one_bucket_over_normal=round(uo / un, 2))


if __name__ == "__main__":
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/summary_bench.py measures on the GPU: no device visible")
    emit(measurement="box", device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=str(torch.version.hip))
    kernel_times()
    summary_times("lstm", 64)
    summary_times("res_lstm_l", 8)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/summary_bench.py: Model.run_summaries with its histograms on the host against on the device (csrc/hist.hip), and the\n"
                    "bare rsrgan_hist call (see the tool's docstring for what each line measures).  One JSON object per line.\n")
            f.write("\n".join(lines) + "\n")
