#!/usr/bin/env python
"""The kernels every D-run / G-run call issues, for comparing two builds of the library (the launch-order invariant of DESIGN.md 3b).

Driver (run under the profiler, once per build and flags value; reference lstm size, B = 32, T = 5):

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o r -- python tools/step_trace.py --flags 1 [--lib other.so]

covers the defaults (D-run, G-run on its forward, G-run with a fresh forward), RSRGAN_DPIPE=1 and the bucketed data-parallel
sequence (backward, wait on every bucket, apply), each twice.  A marker kernel (a cumulative sum, which nothing else here launches)
follows every call.

Comparison:

    python tools/step_trace.py --compare <dir A> <dir B> [--counts]

prints per call whether the ordered kernel-name lists (by dispatch id; --counts: the kernel counts, for graph replays whose nodes are
dispatched in no fixed order) are identical, and exits non-zero if any differ."""
import argparse
import collections
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MARK = "scan"          # substring of the marker's kernel names (torch.cumsum)


def drive(flags, lib):
    import ctypes as C
    import torch
    if lib:
        from rsrgan_amd import _lib
        _lib.LIB_PATH = os.path.abspath(lib)
    from oracle import rsrgan_oracle as O
    from tests.helpers import NET_D, NET_G, build_hip_pair, rand_batch
    cfg, B, T = O.NetCfg(), 32, 5
    x, lab, ln = rand_batch(cfg, B, T, seed=6, ragged=True)
    tick = torch.arange(64, device="cuda", dtype=torch.float32)

    def mark():
        torch.cuda.synchronize()
        tick.cumsum(0)
        torch.cuda.synchronize()

    def handle(dpipe):
        os.environ["RSRGAN_DPIPE"] = dpipe
        m = build_hip_pair(cfg, B, T, seed=5, flags=flags)[0]
        os.environ["RSRGAN_DPIPE"] = "0"
        return m
    for dpipe in ("0", "1"):
        m = handle(dpipe)
        with m.on_stream():
            mark()
            for _ in range(3 if flags & 2 else 2):          # (graphs: eager, captured, replayed)
                for call in (lambda: m.engine.d_backward(x, lab, ln, train=True, apply=True),
                             lambda: m.engine.g_backward(x, lab, ln, train=True, reuse=True, apply=True),
                             lambda: m.engine.g_backward(x, lab, ln, train=True, reuse=False, apply=True)):
                    call(); mark()
        m.engine.close()
    m = handle("0")
    e = m.engine
    other = torch.cuda.Stream()
    with m.on_stream():
        mark()
        for _ in range(3 if flags & 2 else 2):
            for net, call in ((NET_D, lambda: e.d_backward(x, lab, ln, train=True, apply=False)),
                              (NET_G, lambda: e.g_backward(x, lab, ln, train=True, reuse=True, apply=False))):
                call()
                from rsrgan_amd import _lib
                for i in range(len(e.grad_buckets(net))):
                    _lib.check(e.lib.rsrgan_grad_bucket_wait(e.h, net, i, C.c_void_p(other.cuda_stream)))
                other.synchronize()
                mark()
                e.apply(net); mark()
    assert e.device_status() == 0
    e.close()


def calls_of(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, (d, files)
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    calls, cur = [], []
    for r in rows:
        name = r["Kernel_Name"].split("(")[0]
        if MARK in name.lower():
            if cur:
                calls.append(cur)
            cur = []
        else:
            cur.append(name)
    return calls[1:]          # (what precedes the first marker pair: handle construction, uploads)


def compare(a, b, counts):
    ca, cb = calls_of(a), calls_of(b)
    bad = len(ca) != len(cb)
    print("%d calls in %s, %d in %s" % (len(ca), a, len(cb), b))
    for i, (x, y) in enumerate(zip(ca, cb)):
        same = collections.Counter(x) == collections.Counter(y) if counts else x == y
        print("call %2d: %3d kernels  %s" % (i, len(x), "identical" if same else "DIFFERENT (%d kernels in the other build)" % len(y)))
        if not same:
            bad = True
            for j, (u, v) in enumerate(zip(x, y)):
                if u != v:
                    print("   first difference at kernel %d: %s | %s" % (j, u[-60:], v[-60:]))
                    break
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--flags", type=int, default=1)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--counts", action="store_true")
    a = ap.parse_args()
    sys.exit(compare(a.compare[0], a.compare[1], a.counts) if a.compare else drive(a.flags, a.lib))
