#!/usr/bin/env python
"""Decode throughput and streaming latency of the sequence generators, one JSON line per configuration.

    python tools/decode_bench.py [--g_type res_lstm_l] [--utts 256] [--min_frames 200] [--max_frames 1500] [--repeats 3]
                                 [--configs a,b,c,d,live,bnlstm] [--lib path/to/librsrgan_hip.so] [--lean]

A seeded synthetic test set (utterance lengths uniform in [min_frames, max_frames], N(0,1) features, the handle's initial
variables) goes through

    a     whole utterances, batch_size 1: run_gan_rnn.decode's loop (model.forward per utterance, handle of max_frames frames)
    b     --decode_chunk 200 --decode_streams 1   (rsrgan_amd.stream.decode_streams)
    c     --decode_chunk 200 --decode_streams 32
    d     --decode_chunk 200 --decode_streams 64
    live  one stream on a batch_size-1 handle: ms per StreamEnhancer.push of 10 / 50 / 100 frames (median and p90 of the pushes
          of one long utterance; the host waits for every push's output, as a recogniser behind it would)

    bnlstm  (not in the default list) 3 x BNLSTMCell(760, num_proj=280), Din 257, Dout 40, the initial variables, one utterance
          of --bn_frames (1000) frames: whole, in --chunk-frame chunks and as 32 streams on the inference-only model
          (RNNTrainer(inference_only=True): the persistent forward on the folded variables), and whole on the full model's forward
          (two launches per step and layer) -- --repeats alternating passes over the four, median us per frame of each

and reports utterances/s and frames/s of every repeat (host wall clock around the whole set, device drained at the end: the
copies of the inputs and outputs are part of decoding).  `--lib`: time another build of the library (configuration a only
makes sense for a build without the stateful forward).  `--lean`: every configuration on an inference-only model
(GAN_RNN(inference_only=True): the generator alone, no BPTT stash); the records carry "lean": true."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build(g_type, batch, frames, din, dout, lean=False):
    from rsrgan_amd import GAN_RNN
    args = SimpleNamespace(batch_size=batch, input_dim=din, output_dim=dout, left_context=0, right_context=0, g_type=g_type,
                           keep_prob=1.0, batch_norm=False, num_gpu=1, save_dir=None, l2_scale=0.0)
    return GAN_RNN(None, args, ["gpu:0"], cross_validation=True, infer=True, max_frames=frames, **({"inference_only": True} if lean else {}))


def bnlstm_config(a, base):
    """one utterance through the bnlstm inference model (whole, chunked, 32 streams) and through the full model's forward"""
    import torch
    from rsrgan_amd.stream import decode_streams
    from rsrgan_amd.trainer import RNNTrainer
    T, chunk = a.bn_frames, a.chunk
    args = SimpleNamespace(batch_size=1, input_dim=a.input_dim, output_dim=a.output_dim, left_context=0, right_context=0, g_type="bnlstm",
                           keep_prob=1.0, batch_norm=False, num_gpu=1, save_dir=None, l2_scale=0.0)

    def mk(batch, frames, lean):
        return RNNTrainer(None, SimpleNamespace(**dict(vars(args), batch_size=batch)), ["gpu:0"], cross_validation=True, max_frames=frames,
                          inference_only=lean)
    utt = np.random.default_rng(a.seed).standard_normal((T, a.input_dim)).astype(np.float32)
    ln = np.array([T], np.int32)
    whole, chunked, many, full = mk(1, T, True), mk(1, chunk, True), mk(32, chunk, True), mk(1, T, False)
    g = whole.get_vars()[0]
    for m in (chunked, many):
        m.set_vars(g)
    full.set_vars(g, None)
    runs = {
        "whole": (T, lambda: whole.forward(utt[None], ln)),
        "chunked": (T, lambda: sum(1 for _ in decode_streams(chunked, iter([utt]), chunk, 1))),
        "streams32": (32 * T, lambda: sum(1 for _ in decode_streams(many, iter([utt] * 32), chunk, 32))),
        "full_forward": (T, lambda: full.forward(utt[None], ln)),
    }
    y_lean, y_full = np.asarray(whole.forward(utt[None], ln), np.float64), np.asarray(full.forward(utt[None], ln), np.float64)
    secs = {k: [] for k in runs}
    for rep_ in range(a.repeats + 1):                     # (pass 0 warms every shape up)
        for k, (_, fn) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep_:
                secs[k].append(time.perf_counter() - t0)
    rec = dict(base, config="bnlstm", g_type="bnlstm", utterances=1, frames=T, chunk=chunk,
               lean_vs_full_rel=float(np.linalg.norm(y_lean - y_full) / np.linalg.norm(y_full)),
               device_bytes=dict(inference=whole.engine.device_bytes(), full=full.engine.device_bytes()))
    for k, (frames, _) in runs.items():
        rec[k] = dict(seconds=[round(s, 5) for s in secs[k]], us_per_frame_median=round(1e6 * float(np.median(secs[k])) / frames, 3))
    print(json.dumps(rec), flush=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--g_type", default="res_lstm_l")
    p.add_argument("--utts", type=int, default=256)
    p.add_argument("--min_frames", type=int, default=200)
    p.add_argument("--max_frames", type=int, default=1500)
    p.add_argument("--chunk", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--configs", default="a,b,c,d,live")
    p.add_argument("--input_dim", type=int, default=257)
    p.add_argument("--output_dim", type=int, default=40)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--lib", default=None)
    p.add_argument("--lean", default=False, action="store_true", help="run the configurations on an inference-only model")
    p.add_argument("--bn_frames", type=int, default=1000, help="configuration bnlstm: frames of its utterance")
    a = p.parse_args(argv)
    if a.lib:
        from rsrgan_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
        import ctypes

        class OlderBuild(ctypes.CDLL):
            """a build from before the stateful forward (or before rsrgan_device_bytes) lacks those entry points: the binding may still set
            their argtypes (on a stand-in that nothing calls: configuration a uses rsrgan_forward_g only)"""
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if name.startswith("rsrgan_g_state_") or name in ("rsrgan_forward_g_stream", "rsrgan_device_bytes"):
                        return SimpleNamespace()
                    raise
        _lib.C.CDLL = OlderBuild
    import torch
    rng = np.random.default_rng(a.seed)
    lens = rng.integers(a.min_frames, a.max_frames + 1, size=a.utts)
    utts = [rng.standard_normal((int(n), a.input_dim)).astype(np.float32) for n in lens]
    frames = int(lens.sum())
    base = dict(g_type=a.g_type, utterances=a.utts, frames=frames, min_frames=a.min_frames, max_frames=a.max_frames,
                device=torch.cuda.get_device_name(0), lib=a.lib or "built", lean=bool(a.lean))

    def report(name, extra, secs):
        rec = dict(base, config=name, **extra)
        rec["seconds"] = [round(s, 4) for s in secs]
        rec["utts_per_s"] = [round(a.utts / s, 2) for s in secs]
        rec["frames_per_s"] = [round(frames / s, 1) for s in secs]
        rec["utts_per_s_median"] = round(a.utts / float(np.median(secs)), 2)
        print(json.dumps(rec), flush=True)

    def timed(fn):
        fn()                                              # warm-up: allocations, the library's lazy copies, first launches
        secs = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return secs

    for name in [c.strip() for c in a.configs.split(",") if c.strip()]:
        if name == "a":
            model = build(a.g_type, 1, a.max_frames, a.input_dim, a.output_dim, a.lean)

            def whole():
                for u in utts:
                    model.forward(u[None], np.array([len(u)], np.int32))
            report("a", dict(batch_size=1, chunk=0, streams=1), timed(whole))
        elif name in ("b", "c", "d"):
            from rsrgan_amd.stream import decode_streams
            streams = {"b": 1, "c": 32, "d": 64}[name]
            model = build(a.g_type, streams, a.chunk, a.input_dim, a.output_dim, a.lean)

            def chunked():
                n = sum(1 for _ in decode_streams(model, iter(utts), a.chunk, streams))
                assert n == len(utts)
            report(name, dict(batch_size=streams, chunk=a.chunk, streams=streams), timed(chunked))
        elif name == "live":
            from rsrgan_amd.stream import StreamEnhancer
            model = build(a.g_type, 1, 100, a.input_dim, a.output_dim, a.lean)
            enh = StreamEnhancer(model, None, 0, 0, chunk=100)
            long_utt = rng.standard_normal((3000, a.input_dim)).astype(np.float32)
            out = {}
            for n in (10, 50, 100):
                ms = []
                for rep in range(2):                      # (the first pass warms up)
                    ms = []
                    for pos in range(0, len(long_utt), n):
                        t0 = time.perf_counter()
                        enh.push(long_utt[pos:pos + n])   # returns host arrays: the device has finished
                        ms.append(1e3 * (time.perf_counter() - t0))
                    enh.flush()
                out["push_%d" % n] = dict(pushes=len(ms), ms_median=round(float(np.median(ms)), 4), ms_p90=round(float(np.percentile(ms, 90)), 4),
                                          ms_per_frame=round(float(np.median(ms)) / n, 5))
            print(json.dumps(dict(base, config="live", batch_size=1, **out)), flush=True)
        elif name == "bnlstm":
            bnlstm_config(a, base)
            continue
        else:
            raise SystemExit("unknown configuration %r" % name)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
