"""csrc/conv.hip kernel by kernel: the implicit-GEMM forward convolution (k_conv_fwd, k_conv_fwd4), the data gradient (the same kernels on the
flipped filter) and the weight gradient (k_conv_wgrad, k_conv_wgrad4, k_conv_wgrad_red), each through the host launch function the
model calls (rsrgan_op_conv_fwd / rsrgan_op_conv_wgrad) against torch.nn.functional.conv2d in fp64 on the CPU, from the same
fp32-rounded inputs; both gradients are fp64 autograd of that forward.  Every case asserts its numbers first and the plan that ran
(rsrgan_op_conv_last_plan) second, so a plan failure says the arithmetic was right.

Case construction: the filter carries a ramp over (dh, dw, ci, co) and the input one over (h, w, c) on top of noise; operand columns up
to pad4(C) are zero (the kernels' contract), the columns beyond and guard rows before and behind every operand are NaN; out, dW and db
are pre-filled with a sentinel: guard rows, rows behind the extent and every column from N on (the epilogues write co < N only: columns
[N, pad4(N)) stay unchanged) must come back bit-identical; the workspace is NaN up to its size (a partial the reducer reads but no
workgroup wrote poisons dW) with a sentinel band behind it; every launch runs twice and must be bit-identical.

Bound: max |err| / max(|ref|_max, 1) < 2e-5, what tests/test_gpu_wgrad_ops.py holds fp32-MFMA products to at K = 20000; every
reduction here is shorter.  test_mutations_exceed_the_bound shows on the CPU that a tap dropped at a strip edge, a one-column shift
and a wrong flip are at least 100 x that bound at the longest reductions of the table.

The process-scope switches (RSRGAN_CONV4, _CONV4_KS, _WGRAD4, _WGRAD_DH, _CONV_ROWS) each run the whole table once in a fresh child
process.  COVERED collects (family, template arguments, planner branch, FB > 1, fpg > 1) of every launch of a passing case;
test_zz_ledger compares it with LEDGER, derived by reading the planners."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 7.0
GUARD = 3                      # guard rows before and behind every buffer
WS_GUARD = 4096                # sentinel floats behind the workspace
TOL = 2e-5
COVERED = set()                # (family, template arguments, branch, FB > 1, fpg > 1)
WAVES = set()                  # (waves, PS, nkg) of every weight-gradient launch
ERRORS = []                    # (setting, kind, case, error)
_REF = {}                      # fp64 references, computed once per case and left unchanged
_FAULTED = []                  # a launch that raised (a HIP error, not a failed assertion): nothing more is started on the GPU


def make_engine():
    from rsrgan_amd.ops import OpEntries
    return OpEntries()


@pytest.fixture(scope="module")
def eng():
    return make_engine()


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    if _FAULTED:
        pytest.fail("not run: %s raised a HIP error earlier in this module" % _FAULTED[0])


def stops_the_module(fn):
    """anything but a failed assertion out of a launch (a HIP error) keeps every later test and child process from starting"""
    def wrapped(*a, **kw):
        try:
            return fn(*a, **kw)
        except AssertionError:
            raise
        except Exception:
            _FAULTED.append(fn.__name__)
            raise
    return wrapped


def pad4(n):
    return (n + 3) // 4 * 4


def gen(*seed):
    s = 0
    for v in seed:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator(device="cpu").manual_seed(s)


def relerr(got, ref):
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1.0)


def image(R, S, W, C, seed):
    """[R][S][W][C] fp32: noise + a ramp over (h, w, c)"""
    h = torch.arange(S, dtype=torch.float32)[:, None, None]
    w = torch.arange(W, dtype=torch.float32)[None, :, None]
    c = torch.arange(C, dtype=torch.float32)[None, None, :]
    ramp = 0.03 * (((5 * h + 3 * w + 7 * c) % 11) - 5)
    return torch.randn(R, S, W, C, generator=gen(R, S, W, C, seed), dtype=torch.float32) + ramp[None]


def filt(S, fw, Cin, Cout, seed):
    """[S][fw][Cin][Cout] fp32 as the model stores a layer's filter: noise + a ramp over (dh, dw, ci, co)"""
    dh = torch.arange(S, dtype=torch.float32)[:, None, None, None]
    dw = torch.arange(fw, dtype=torch.float32)[None, :, None, None]
    ci = torch.arange(Cin, dtype=torch.float32)[None, None, :, None]
    co = torch.arange(Cout, dtype=torch.float32)[None, None, None, :]
    ramp = 0.03 * (((3 * dh + 5 * dw + 7 * ci + 11 * co) % 13) - 6)
    return torch.randn(S, fw, Cin, Cout, generator=gen(S, fw, Cin, Cout, seed), dtype=torch.float32) + ramp


def conv_ref(x, f):
    """NHWC conv2d, kernel [S, fw] over the whole height, stride 1, SAME: x [R][S][W][C], f [S][fw][C][N] -> [R][S][W][N]"""
    S, fw = f.shape[0], f.shape[1]
    y = F.conv2d(x.permute(0, 3, 1, 2).contiguous(), f.permute(3, 2, 0, 1).contiguous(), padding=((S - 1) // 2, (fw - 1) // 2))
    return y.permute(0, 2, 3, 1)


def operand(mat, dev, extra=4):
    """mat [rows][cols] -> device view [rows][pad4(cols) + extra]: zeros up to pad4(cols), NaN beyond and in GUARD rows on both sides"""
    rows, cols = mat.shape
    whole = torch.full((rows + 2 * GUARD, pad4(cols) + extra), float("nan"), dtype=torch.float32)
    whole[GUARD:GUARD + rows, :pad4(cols)] = 0.0
    whole[GUARD:GUARD + rows, :cols] = mat
    whole = whole.to(dev)
    return whole, whole[GUARD:GUARD + rows]


def filter_operand(f, dev):
    """[S*fw*Cin][pad4(Cout) + 4]: NaN from column Cout on (k_conv_prep reads n < Cout only)"""
    S, fw, Cin, Cout = f.shape
    whole = torch.full((S * fw * Cin + 2 * GUARD, pad4(Cout) + 4), float("nan"), dtype=torch.float32)
    whole[GUARD:GUARD + S * fw * Cin, :Cout] = f.reshape(S * fw * Cin, Cout)
    whole = whole.to(dev)
    return whole, whole[GUARD:GUARD + S * fw * Cin]


def sentinel(rows, cols, dev, extra=4):
    whole = torch.full((rows + 2 * GUARD, pad4(cols) + extra), SENT, dtype=torch.float32, device=dev)
    return whole, whole[GUARD:GUARD + rows]


def untouched(whole, rows, cols):
    """everything of a sentinel buffer but [rows][cols] of its body is bit-unchanged"""
    chk = whole.clone()
    chk[GUARD:GUARD + rows, :cols] = SENT
    return bool(torch.all(chk.view(torch.int32) == torch.tensor(SENT).view(torch.int32).item()))


def key_of(p):
    args = (p["a0"], p["a1"]) if p["family"] == "fwd" else (p["a0"], p["a1"], p["a2"])
    return (p["family"], args, p["branch"], p["FB"] > 1, p["fpg"] > 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# forward and data gradient
# ---------------------------------------------------------------------------------------------------------------------------------
MASK_VALUES = torch.tensor([1.5, -2.0, 0.0, -0.0, 1e-30, -1e-30], dtype=torch.float32)


def fwd_reference(C, N, S, W, fw, R, flip, bias, relu, mask):
    k = ("fwd", C, N, S, W, fw, R, flip, bias, relu, mask)
    if k in _REF:
        return _REF[k]
    x = image(R, S, W, C, 1)
    f = filt(S, fw, N, C, 2) if flip else filt(S, fw, C, N, 2)      # flip: the layer is N -> C and x the gradient of its output
    b = torch.randn(N, generator=gen(N, 3), dtype=torch.float32) if bias else None
    if flip:
        x0 = torch.zeros(R, S, W, N, dtype=torch.float64, requires_grad=True)
        ref, = torch.autograd.grad(conv_ref(x0, f.double()), x0, x.double())
    else:
        ref = conv_ref(x.double(), f.double())
    if bias:
        ref = ref + b.double()
    if relu:
        ref = torch.clamp(ref, min=0.0)
    m = None
    if mask:
        m = MASK_VALUES[torch.randint(0, len(MASK_VALUES), (R, S, W, N), generator=gen(R, S, W, N, 4))]
        ref = torch.where(m.double() > 0, ref, torch.zeros_like(ref))
    _REF[k] = (x, f, b, m, ref.detach())
    return _REF[k]


@stops_the_module
def run_fwd(eng, shape, R, flip=False, bias=False, relu=False, mask=False, setting="default"):
    """two launches (bit-identical) against the fp64 reference; returns the plan records"""
    C, N, S, W, fw = shape
    dev = eng.device
    x, f, b, m, ref = fwd_reference(C, N, S, W, fw, R, flip, bias, relu, mask)
    M = R * S * W
    xw, xd = operand(x.reshape(M, C), dev)
    fwhole, fd = filter_operand(f, dev)
    bd = None
    if b is not None:                                          # [4 NaN | N values | 8 NaN]: 16-byte aligned, a read past either end poisons out
        bw = torch.full((4 + N + 8,), float("nan"), dtype=torch.float32)
        bw[4:4 + N] = b
        bw = bw.to(dev)
        bd = bw[4:4 + N]
    mw, md = operand(m.reshape(M, N), dev) if m is not None else (None, None)
    o1w, o1 = sentinel(M, N, dev)
    o2w, o2 = sentinel(M, N, dev)
    assert xd.stride(0) > pad4(C) and o1.stride(0) > pad4(N)
    assert eng.op_conv_fwd(xd, C, fd, o1, N, R, S, W, fw, flip=flip, bias=bd, relu=relu, mask=md)
    plans = eng.op_conv_last_plan()
    assert eng.op_conv_fwd(xd, C, fd, o2, N, R, S, W, fw, flip=flip, bias=bd, relu=relu, mask=md)
    torch.cuda.synchronize()
    got = o1[:, :N].cpu().double().reshape(R, S, W, N)
    err = relerr(got, ref)
    print("conv_ops %-14s %-5s C=%-2d N=%-2d S=%-2d W=%-3d fw=%-2d R=%-3d bias=%d relu=%d mask=%d err %.2e  %s" % (
        setting, "dgrad" if flip else "fwd", C, N, S, W, fw, R, bias, relu, mask, err,
        " + ".join("%s<%d,%d,%d> %s TW=%d FB=%d" % (p["family"], p["a0"], p["a1"], p["a2"], p["branch"], p["TW"], p["FB"]) for p in plans)))
    assert err < TOL, err
    if mask:
        zero = (m.reshape(M, N) > 0).logical_not()
        assert bool(torch.all(o1[:, :N].cpu().view(torch.int32)[zero] == 0)), "a masked output is not +0.0"
    assert untouched(o1w, M, N), "out written outside [positions][N]: guard rows, rows behind the extent or columns from N on"
    assert torch.equal(o1w.view(torch.int32), o2w.view(torch.int32)), "two launches of one convolution differ"
    ERRORS.append((setting, "dgrad" if flip else "fwd", (C, N, S, W, fw, R), err))
    return plans


# shape (C, N, S, W, fw), the launches under the default switches (family, template arguments, branch, TW, FB), options.
# Single strip / row-aligned main + remainder; W in {1, 5, 63, 64, 65, 72, 129, 200, 257}; S in {1, 3, 5, 7, 11}; fw in {1, 3, 7, 13}
# with fw > W; N in {1, 3, 4, 5, 12, 16, 17, 20, 31, 32}; C in {1, 4, 8, 12, 16, 24, 32}.
FWD = [
    ((4, 12, 1, 65, 1), [("fwd4", (3, 3, 2), "main", 64, 1), ("fwd4", (2, 3, 2), "rem", 1, 16)], dict(bias=True, relu=True)),
    ((12, 20, 3, 257, 7), [("fwd4", (3, 5, 2), "main", 64, 1), ("fwd4", (2, 5, 2), "rem", 1, 16)], dict(flip=True, mask=True)),
    ((16, 32, 11, 257, 13), [("fwd4", (3, 8, 2), "main", 64, 1), ("fwd4", (2, 8, 2), "rem", 1, 7)], dict(bias=True, relu=True)),
    ((8, 5, 3, 5, 13), [("fwd", (4, 1), "whole", 5, 1)], dict(flip=True, mask=True)),                    # filter wider than the frame
    ((1, 12, 11, 64, 13), [("fwd4", (3, 3, 2), "whole", 64, 1)], dict(bias=True)),                       # W = 64 exactly: no split
    ((24, 17, 7, 129, 3), [("fwd", (6, 2), "main", 64, 1), ("fwd", (4, 2), "rem", 1, 16)], dict(bias=True, relu=True, mask=True)),
    ((32, 31, 5, 72, 7), [("fwd", (6, 2), "main", 64, 1), ("fwd", (4, 2), "rem", 8, 9)], dict(flip=True)),
    ((12, 3, 3, 200, 3), [("fwd", (6, 1), "main", 64, 1), ("fwd", (4, 1), "rem", 8, 16)], dict(relu=True)),
    ((16, 1, 11, 63, 1), [("fwd", (6, 1), "whole", 63, 1)], dict(bias=True)),
    ((4, 4, 5, 1, 3), [("fwd4", (2, 1, 2), "whole", 1, 1)], dict(mask=True)),                            # W = 1: only halo columns
    ((24, 16, 3, 63, 3), [("fwd", (4, 1), "whole", 63, 1)], dict(flip=True, mask=True)),                 # N = 16: 16x16x4 by default
    ((1, 4, 3, 200, 1), [("fwd4", (3, 1, 2), "main", 64, 1), ("fwd4", (2, 1, 2), "rem", 8, 16)], dict(bias=True, relu=True)),
    ((1, 16, 1, 65, 1), [("fwd", (6, 1), "main", 64, 1), ("fwd", (4, 1), "rem", 1, 16)], dict()),
    ((1, 20, 11, 63, 1), [("fwd4", (3, 5, 2), "whole", 63, 1)], dict(relu=True)),
    ((1, 12, 1, 1, 1), [("fwd4", (2, 3, 2), "whole", 1, 1)], dict(bias=True)),                           # one position per frame
    ((1, 20, 1, 1, 1), [("fwd4", (2, 5, 2), "whole", 1, 1)], dict()),
    ((1, 32, 1, 1, 1), [("fwd4", (2, 8, 2), "whole", 1, 1)], dict(bias=True, relu=True)),
    ((1, 32, 3, 200, 1), [("fwd4", (3, 8, 2), "main", 64, 1), ("fwd4", (2, 8, 2), "rem", 8, 16)], dict(mask=True)),
    ((1, 16, 11, 63, 1), [("fwd", (6, 1), "whole", 63, 1)], dict(bias=True, relu=True)),
    ((32, 12, 7, 5, 7), [("fwd4", (2, 3, 2), "whole", 5, 1)], dict(flip=True)),                          # C' = 36, filter wider than the frame
]


def check_fwd_plans(plans, want):
    assert len(plans) == len(want), plans
    for p, (family, args, branch, TW, FB) in zip(plans, want):
        got = (p["family"], (p["a0"], p["a1"]) if family == "fwd" else (p["a0"], p["a1"], p["a2"]), p["branch"], p["TW"], p["FB"])
        assert got == (family, args, branch, TW, FB), (got, want)
        assert p["lds"] <= 160 * 1024 and p["gx"] >= 1 and p["gy"] >= 1


def cover(plans):
    for p in plans:
        COVERED.add(key_of(p))
        if p["family"] in ("wgrad", "wgrad4"):
            WAVES.add((p["waves"], p["PS"], p["nkg"]))


@pytest.mark.parametrize("shape,want,opts", FWD, ids=["C%d-N%d-S%d-W%d-fw%d" % c[0] for c in FWD])
def test_forward(eng, shape, want, opts):
    plans = run_fwd(eng, shape, 3, **opts)
    check_fwd_plans(plans, want)
    cover(plans)


@pytest.mark.parametrize("shape,FB", [((4, 12, 1, 65, 1), 16), ((16, 32, 11, 257, 13), 7), ((24, 17, 7, 129, 3), 16)])
def test_forward_frames_per_workgroup(eng, shape, FB):
    """the one-strip remainder launch takes FB frames per workgroup: R below, at and above FB, and a ragged last frame group"""
    for R in (1, FB - 1, FB, FB + 1, 2 * FB + 3):
        plans = run_fwd(eng, shape, R, bias=True, relu=True)
        assert plans[1]["branch"] == "rem" and plans[1]["FB"] == FB and plans[1]["gy"] == (R + FB - 1) // FB, plans
        cover(plans)


def test_forward_refusals(eng):
    """shapes conv_fwd_supported rejects: nothing launched, the sentinels intact, an empty plan record"""
    dev = eng.device
    for C, N, S, W, fw in [(24, 12, 3, 9, 13), (32, 12, 3, 9, 13), (4, 4, 4, 9, 3), (4, 4, 3, 9, 4), (4, 33, 3, 9, 3), (6, 4, 3, 9, 3)]:
        assert eng.op_conv_supported(C, N, S, W, fw) == (False, False), (C, N, S, W, fw)
        _, xd = operand(torch.zeros(S * W, C), dev)
        _, fd = filter_operand(torch.zeros(S, fw, C, N), dev)
        ow, o = sentinel(S * W, N, dev)
        assert eng.op_conv_fwd(xd, C, fd, o, N, 1, S, W, fw) is False
        assert eng.op_conv_last_plan() == []
        torch.cuda.synchronize()
        assert untouched(ow, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def wgrad_reference(C, N, S, W, fw, R):
    k = ("wgrad", C, N, S, W, fw, R)
    if k in _REF:
        return _REF[k]
    x = image(R, S, W, C, 5)
    d = image(R, S, W, N, 6)
    f0 = torch.zeros(S, fw, C, N, dtype=torch.float64, requires_grad=True)
    dW, = torch.autograd.grad(conv_ref(x.double(), f0), f0, d.double())
    _REF[k] = (x, d, dW.detach(), d.double().sum(dim=(0, 1, 2)))
    return _REF[k]


@stops_the_module
def run_wgrad(eng, shape, with_db=True, R_max=None, ws=None, setting="default"):
    C, N, S, W, fw, R = shape
    dev = eng.device
    R_max = R if R_max is None else R_max
    x, d, ref, ref_db = wgrad_reference(C, N, S, W, fw, R)
    M, K = R * S * W, S * fw * C
    _, xd = operand(x.reshape(M, C), dev)
    _, dd = operand(d.reshape(M, N), dev)
    need = eng.op_conv_ws_floats(C, R_max, S, W, fw)
    if ws is None:
        ws = torch.empty(need + WS_GUARD, dtype=torch.float32, device=dev)
    assert ws.numel() == need + WS_GUARD
    outs = []
    for _ in range(2):
        ws[:need] = float("nan")
        ws[need:] = SENT
        gw, g = sentinel(K, N, dev)
        dbw = torch.full((4 + 40,), SENT, dtype=torch.float32, device=dev) if with_db else None
        db = dbw[4:] if with_db else None                      # sentinels in front of db[0] and from db[N] on
        assert eng.op_conv_wgrad(xd, C, dd, N, g, ws, R_max, R, S, W, fw, db=db, ws_floats=need)
        outs.append((gw, g, dbw))
    plans = eng.op_conv_last_plan()
    torch.cuda.synchronize()
    (gw, g, dbw), (gw2, _, dbw2) = outs
    db = dbw[4:] if with_db else None
    err = relerr(g[:, :N].cpu().double().reshape(S, fw, C, N), ref)
    err_db = relerr(db[:N].cpu().double(), ref_db) if with_db else 0.0
    p = plans[0]
    print("conv_ops %-14s wgrad C=%-2d N=%-2d S=%-2d W=%-3d fw=%-2d R=%-3d db=%d err %.2e db %.2e  %s<%d,%d,%d> %s DH=%d fpg=%d groups=%d strips=%d nkg=%d PS=%d waves=%d gmax=%d" % (
        setting, C, N, S, W, fw, R, with_db, err, err_db, p["family"], p["a0"], p["a1"], p["a2"], p["branch"], p["DH"], p["fpg"],
        p["groups"], p["nstrips"], p["nkg"], p["PS"], p["waves"], p["gmax"]))
    assert err < TOL and err_db < TOL, (err, err_db)
    assert untouched(gw, K, N), "dW written outside [S*fw*C][N]"
    if with_db:
        assert bool(torch.all(db[N:] == SENT)) and bool(torch.all(dbw[:4] == SENT)), "db written in front of db[0] or from db[N] on"
        assert torch.equal(dbw.view(torch.int32), dbw2.view(torch.int32)), "two launches differ in db"
    assert bool(torch.all(ws[need:] == SENT)), "the workspace guard band was written"
    assert torch.equal(gw.view(torch.int32), gw2.view(torch.int32)), "two launches of one weight gradient differ: the order is not fixed"
    ERRORS.append((setting, "wgrad", shape, max(err, err_db)))
    return plans


# shape (C, N, S, W, fw, R) and under the default switches (family, template arguments, branch, DH, fpg, groups, nstrips, nkg, PS, waves, gmax)
WGRAD = [
    # fpg > 1: R = 130 at gmax = 85 and R = 40 at gmax = 36 divide evenly (65 x 2, 20 x 2); the RAGGED last group -- the r >= R early
    # exit -- is R = 131 (66 groups, the last of one frame), R = 41, the R = 35 cases (18 groups at fpg = 2) and the odd R of the sweep
    ((1, 12, 3, 5, 3, 130), ("wgrad4", (3, 3, 12), "search", 1, 2, 65, 1, 1, 12, 12, 85)),              # R > gmax: fpg = 2
    ((1, 12, 3, 5, 3, 131), ("wgrad4", (3, 3, 12), "search", 1, 2, 66, 1, 1, 12, 12, 85)),              # ragged: the last group holds one frame
    ((4, 5, 3, 200, 3, 41), ("wgrad", (1, 1, 6), "rows", 6, 2, 21, 7, 0, 1, 16, 36)),                   # ragged, multi-strip
    ((16, 17, 3, 200, 13, 40), ("wgrad", (2, 2, 3), "k2", 3, 2, 20, 7, 0, 1, 16, 36)),                  # K' = 272 > 256, multi-strip
    ((24, 12, 3, 200, 3, 2), ("wgrad4", (3, 3, 12), "rows", 6, 1, 2, 7, 2, 3, 12, 36)),
    ((24, 20, 5, 63, 7, 3), ("wgrad4", (5, 3, 12), "search", 1, 1, 3, 1, 3, 4, 12, 51)),                # PS 4
    ((32, 32, 11, 257, 7, 2), ("wgrad4", (8, 3, 8), "rows", 6, 1, 2, 9, 4, 1, 8, 14)),
    ((16, 32, 7, 129, 13, 2), ("wgrad4", (8, 3, 8), "rows", 4, 1, 2, 5, 4, 1, 8, 25)),                  # S = 7: DH = 4, 8 waves x PS 1
    ((20, 12, 3, 200, 13, 3), ("wgrad4", (3, 3, 10), "k2", 3, 1, 3, 7, 5, 2, 10, 36)),                  # fw * C = 260: nkg = 5, 10 waves
    ((4, 5, 3, 200, 3, 2), ("wgrad", (1, 1, 6), "rows", 6, 1, 2, 7, 0, 1, 16, 36)),                     # N % 4 != 0: 16x16x4
    ((8, 31, 7, 129, 1, 2), ("wgrad", (1, 2, 4), "rows", 4, 1, 2, 5, 0, 1, 16, 25)),
    ((8, 31, 7, 129, 1, 35), ("wgrad", (1, 2, 4), "rows", 4, 2, 18, 5, 0, 1, 16, 25)),
    ((1, 1, 7, 129, 1, 35), ("wgrad", (1, 1, 4), "rows", 4, 2, 18, 5, 0, 1, 16, 25)),
    ((12, 4, 1, 1, 1, 1), ("wgrad4", (1, 3, 12), "search", 1, 1, 1, 1, 1, 12, 12, 256)),                # one position
    ((1, 1, 11, 64, 13, 1), ("wgrad", (1, 1, 6), "rows", 6, 1, 1, 2, 0, 1, 16, 64)),
    ((4, 3, 1, 65, 7, 3), ("wgrad", (1, 1, 1), "search", 1, 1, 3, 1, 0, 1, 16, 256)),                   # S = 1
    ((12, 16, 5, 72, 3, 2), ("wgrad4", (4, 3, 12), "search", 1, 1, 2, 1, 1, 12, 12, 51)),
    ((1, 4, 3, 200, 1, 40), ("wgrad4", (1, 3, 12), "rows", 6, 2, 20, 7, 1, 6, 12, 36)),                 # R = 40 > gmax = 36: fpg = 2, 20 even groups
    ((12, 20, 3, 200, 13, 40), ("wgrad4", (5, 3, 12), "rows", 6, 2, 20, 7, 3, 2, 12, 36)),
    ((16, 32, 1, 1, 13, 1), ("wgrad4", (8, 3, 12), "search", 1, 1, 1, 1, 4, 3, 12, 256)),               # PS 3
    ((1, 16, 7, 129, 1, 15), ("wgrad4", (4, 3, 12), "rows", 4, 1, 15, 5, 1, 6, 12, 25)),
    ((20, 12, 1, 1, 13, 1), ("wgrad4", (3, 3, 10), "search", 1, 1, 1, 1, 5, 2, 10, 256)),
    ((1, 32, 3, 1, 1, 130), ("wgrad4", (8, 3, 12), "search", 1, 2, 65, 1, 1, 12, 12, 85)),
    ((1, 32, 3, 200, 1, 15), ("wgrad4", (8, 3, 12), "rows", 6, 1, 15, 7, 1, 6, 12, 36)),
    ((1, 16, 3, 200, 1, 40), ("wgrad4", (4, 3, 12), "rows", 6, 2, 20, 7, 1, 6, 12, 36)),
    ((1, 32, 3, 200, 1, 40), ("wgrad4", (8, 3, 12), "rows", 6, 2, 20, 7, 1, 6, 12, 36)),
    ((20, 12, 3, 1, 13, 130), ("wgrad4", (3, 3, 10), "search", 1, 2, 65, 1, 5, 2, 10, 85)),
    ((16, 4, 3, 200, 13, 40), ("wgrad4", (1, 3, 8), "rows", 6, 2, 20, 7, 4, 1, 8, 36)),
    ((32, 16, 3, 200, 7, 15), ("wgrad4", (4, 3, 8), "rows", 6, 1, 15, 7, 4, 1, 8, 36)),
    ((1, 4, 3, 200, 1, 1), ("wgrad4", (1, 3, 12), "rows", 6, 1, 1, 7, 1, 6, 12, 36)),
    ((1, 16, 3, 1, 1, 130), ("wgrad4", (4, 3, 12), "search", 1, 2, 65, 1, 1, 12, 12, 85)),
    ((1, 20, 3, 200, 1, 1), ("wgrad4", (5, 3, 12), "rows", 6, 1, 1, 7, 1, 6, 12, 36)),
    ((1, 1, 5, 257, 1, 15), ("wgrad", (1, 1, 6), "rows", 6, 1, 15, 9, 0, 1, 16, 28)),
    ((1, 17, 3, 257, 1, 15), ("wgrad", (1, 2, 6), "rows", 6, 1, 15, 9, 0, 1, 16, 28)),
    ((1, 12, 3, 200, 1, 40), ("wgrad4", (3, 3, 12), "rows", 6, 2, 20, 7, 1, 6, 12, 36)),
    ((16, 4, 3, 200, 13, 1), ("wgrad4", (1, 3, 8), "rows", 6, 1, 1, 7, 4, 1, 8, 36)),
    ((1, 17, 5, 257, 1, 15), ("wgrad", (1, 2, 6), "rows", 6, 1, 15, 9, 0, 1, 16, 28)),
    ((16, 17, 3, 1, 13, 130), ("wgrad", (2, 2, 1), "search", 1, 2, 65, 1, 0, 1, 16, 85)),
    ((16, 12, 3, 200, 13, 1), ("wgrad4", (3, 3, 8), "rows", 6, 1, 1, 7, 4, 1, 8, 36)),
    ((16, 20, 3, 200, 13, 1), ("wgrad4", (5, 3, 8), "rows", 6, 1, 1, 7, 4, 1, 8, 36)),
    ((16, 12, 3, 200, 13, 40), ("wgrad4", (3, 3, 8), "rows", 6, 2, 20, 7, 4, 1, 8, 36)),
    ((20, 12, 3, 200, 13, 40), ("wgrad4", (3, 3, 10), "k2", 3, 2, 20, 7, 5, 2, 10, 36)),
    ((16, 16, 3, 200, 13, 40), ("wgrad4", (4, 3, 8), "rows", 6, 2, 20, 7, 4, 1, 8, 36)),
    ((16, 20, 3, 200, 13, 40), ("wgrad4", (5, 3, 8), "rows", 6, 2, 20, 7, 4, 1, 8, 36)),
    ((16, 32, 3, 200, 13, 40), ("wgrad4", (8, 3, 8), "rows", 6, 2, 20, 7, 4, 1, 8, 36)),
    ((8, 12, 3, 200, 13, 2), ("wgrad4", (3, 3, 12), "rows", 6, 1, 2, 7, 2, 3, 12, 36)),                 # nkg 2 x two row sets: PS 3
    ((12, 12, 3, 200, 13, 2), ("wgrad4", (3, 3, 12), "rows", 6, 1, 2, 7, 3, 2, 12, 36)),                # nkg 3 x two row sets: PS 2
    ((8, 3, 3, 5, 13, 130), ("wgrad", (1, 1, 1), "search", 1, 2, 65, 1, 0, 1, 16, 85)),                 # filter wider than the frame; 65 even groups
    ((16, 1, 3, 200, 13, 2), ("wgrad", (2, 1, 3), "k2", 3, 1, 2, 7, 0, 1, 16, 36)),
    ((16, 3, 3, 200, 13, 40), ("wgrad", (2, 1, 3), "k2", 3, 2, 20, 7, 0, 1, 16, 36)),
    ((16, 17, 3, 200, 13, 2), ("wgrad", (2, 2, 3), "k2", 3, 1, 2, 7, 0, 1, 16, 36)),
    ((16, 5, 5, 9, 13, 2), ("wgrad", (2, 1, 1), "search", 1, 1, 2, 1, 0, 1, 16, 51)),
    ((16, 5, 3, 1, 13, 130), ("wgrad", (2, 1, 1), "search", 1, 2, 65, 1, 0, 1, 16, 85)),
    ((16, 31, 5, 9, 13, 2), ("wgrad", (2, 2, 1), "search", 1, 1, 2, 1, 0, 1, 16, 51)),
    ((4, 17, 3, 9, 3, 2), ("wgrad", (1, 2, 1), "search", 1, 1, 2, 1, 0, 1, 16, 85)),
    ((4, 17, 3, 1, 3, 130), ("wgrad", (1, 2, 1), "search", 1, 2, 65, 1, 0, 1, 16, 85)),
    ((4, 5, 3, 200, 3, 40), ("wgrad", (1, 1, 6), "rows", 6, 2, 20, 7, 0, 1, 16, 36)),
    ((4, 17, 3, 200, 3, 40), ("wgrad", (1, 2, 6), "rows", 6, 2, 20, 7, 0, 1, 16, 36)),
]
WFIELDS = ("DH", "fpg", "groups", "nstrips", "nkg", "PS", "waves", "gmax")


@pytest.mark.parametrize("shape,want", WGRAD, ids=["C%d-N%d-S%d-W%d-fw%d-R%d" % c[0] for c in WGRAD])
def test_weight_gradient(eng, shape, want):
    i = [c[0] for c in WGRAD].index(shape)
    plans = run_wgrad(eng, shape, with_db=i % 3 != 1)
    assert len(plans) == 1
    p = plans[0]
    got = (p["family"], (p["a0"], p["a1"], p["a2"]), p["branch"]) + tuple(p[k] for k in WFIELDS)
    assert got == want, (got, want)
    C, N, S, W, fw, R = shape
    assert p["groups"] == (R + p["fpg"] - 1) // p["fpg"] and (p["gx"], p["gy"], p["gz"]) == ((S + p["DH"] - 1) // p["DH"], p["groups"], p["nstrips"])
    cover(plans)


@pytest.mark.parametrize("C,N,S,W,fw", [(4, 12, 5, 257, 3), (4, 5, 3, 200, 3)])
def test_weight_gradient_workspace_sweep(eng, C, N, S, W, fw):
    """every R <= R_max = 60 on ONE workspace of rsrgan_op_conv_ws_floats(R_max) floats with the guard band behind it: the group count
    is not monotonic in R (groups = ceil(R / ceil(R / gmax))), so the workspace is sized for the worst R' <= R_max"""
    R_max = 60
    need = eng.op_conv_ws_floats(C, R_max, S, W, fw)
    ws = torch.empty(need + WS_GUARD, dtype=torch.float32, device=eng.device)
    groups = {}
    for R in range(1, R_max + 1):
        p = run_wgrad(eng, (C, N, S, W, fw, R), R_max=R_max, ws=ws)[0]
        groups[R] = p["groups"]
        gmax = p["gmax"]
        assert p["groups"] == (R + p["fpg"] - 1) // p["fpg"] and p["fpg"] == (R + gmax - 1) // gmax
    assert gmax < R_max and groups[gmax] == gmax and groups[gmax + 1] < gmax, (gmax, groups)      # both sides of the step
    assert max(groups.values()) > groups[R_max], "R_max itself is not the worst frame count"
    # and the size is what the worst R' needs, not more than any R' <= R_max asks for
    assert need == eng.op_conv_ws_floats(C, gmax, S, W, fw) > eng.op_conv_ws_floats(C, gmax - 1, S, W, fw)


def test_weight_gradient_refusals(eng):
    dev = eng.device
    for C, N, S, W, fw in [(24, 12, 3, 9, 13), (4, 4, 4, 9, 3), (4, 4, 3, 9, 4), (4, 33, 3, 9, 3)]:
        assert eng.op_conv_supported(C, N, S, W, fw)[1] is False
        _, xd = operand(torch.zeros(S * W, C), dev)
        _, dd = operand(torch.zeros(S * W, N), dev)
        gw, g = sentinel(S * fw * C, N, dev)
        db = torch.full((40,), SENT, dtype=torch.float32, device=dev)
        ws = torch.full((1024,), SENT, dtype=torch.float32, device=dev)
        assert eng.op_conv_wgrad(xd, C, dd, N, g, ws, 1, 1, S, W, fw, db=db) is False
        assert eng.op_conv_last_plan() == []
        torch.cuda.synchronize()
        assert untouched(gw, 0, 0) and bool(torch.all(db == SENT)) and bool(torch.all(ws == SENT))


# ---------------------------------------------------------------------------------------------------------------------------------
# the bound separates the mistakes that matter (CPU only: mutated fp64 references)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mutations_exceed_the_bound():
    """at the longest reductions of the tables (forward / data gradient: S*fw*C = 11*13*16 = 2288 and 11*7*32 = 2464; weight gradient:
    R*S*W = 40*3*200 positions) one tap dropped at a strip edge, a one-column shift and a wrong flip are each >= 100 x TOL"""
    for C, N, S, W, fw, TW in [(16, 32, 11, 257, 13, 64), (32, 12, 11, 63, 7, 63)]:
        x, f = image(1, S, W, C, 1).double(), filt(S, fw, C, N, 2).double()
        ref = conv_ref(x, f)
        pt, pl = (S - 1) // 2, (fw - 1) // 2
        edge = min(TW, W) - 1                                  # the last column of the first strip, its rightmost tap of the middle row
        drop = ref.clone()
        src = edge + (fw - 1) - pl
        if src < W:
            drop[:, :, edge, :] -= torch.einsum("rhc,cn->rhn", x[:, :, src, :], f[pt, fw - 1])
        else:                                                   # (the tap reads the right halo there: take the leftmost tap instead)
            drop[:, :, edge, :] -= torch.einsum("rhc,cn->rhn", x[:, :, edge - pl, :], f[pt, 0])
        shift = torch.roll(ref, 1, dims=2)
        flip = conv_ref(x, torch.flip(f, dims=(0, 1)))
        for name, mut in (("tap", drop), ("shift", shift), ("flip", flip)):
            e = relerr(mut, ref)
            print("conv_ops mutation fwd %s C=%d N=%d S=%d W=%d fw=%d: %.2e" % (name, C, N, S, W, fw, e))
            assert e >= 100 * TOL, (name, e)
        # data gradient of the layer N -> C: the same three mistakes in the transposed convolution
        g = image(1, S, W, C, 1).double()
        fl = filt(S, fw, N, C, 2).double()
        x0 = torch.zeros(1, S, W, N, dtype=torch.float64, requires_grad=True)
        dref, = torch.autograd.grad(conv_ref(x0, fl), x0, g)
        unflipped = conv_ref(g, fl.permute(0, 1, 3, 2))        # the forward kernel on the filter with the channels swapped but NOT flipped
        ddrop = dref.clone()
        ddrop[:, :, edge, :] -= torch.einsum("rhc,nc->rhn", g[:, :, edge - pl, :], fl[pt, fw - 1]) if edge - pl >= 0 else 0
        for name, mut in (("tap", ddrop), ("shift", torch.roll(dref, 1, dims=2)), ("flip", unflipped)):
            e = relerr(mut, dref)
            print("conv_ops mutation dgrad %s C=%d N=%d S=%d W=%d fw=%d: %.2e" % (name, C, N, S, W, fw, e))
            assert e >= 100 * TOL, (name, e)
    C, N, S, W, fw, R = 16, 32, 3, 200, 13, 40
    x, d, ref, _ = wgrad_reference(C, N, S, W, fw, R)
    pt, pl = (S - 1) // 2, (fw - 1) // 2
    edge = 28                                                  # TW = 29: the last column of the first strip, the tap (pt, fw - 1)
    drop = ref.clone()
    drop[pt, fw - 1] -= torch.einsum("rhc,rhn->cn", x.double()[:, :, edge + fw - 1 - pl, :], d.double()[:, :, edge, :])
    for name, mut in (("tap", drop), ("shift", torch.roll(ref, 1, dims=1)), ("flip", torch.flip(ref, dims=(0, 1)))):
        e = relerr(mut, ref)
        print("conv_ops mutation wgrad %s: %.2e" % (name, e))
        assert e >= 100 * TOL, (name, e)


# ---------------------------------------------------------------------------------------------------------------------------------
# the process-scope switches: the whole table once per setting in a fresh child process
# ---------------------------------------------------------------------------------------------------------------------------------
SETTINGS = [
    ("CONV4=0", {"RSRGAN_CONV4": "0"}),
    ("CONV4=2", {"RSRGAN_CONV4": "2"}),
    ("CONV4=2 KS=4", {"RSRGAN_CONV4": "2", "RSRGAN_CONV4_KS": "4"}),
    ("WGRAD4=1 DH=3", {"RSRGAN_WGRAD4": "1", "RSRGAN_WGRAD_DH": "3"}),
    ("CONV_ROWS=0", {"RSRGAN_CONV_ROWS": "0"}),
    ("WGRAD4=0", {"RSRGAN_WGRAD4": "0"}),
]
_CHILD_DEAD = []               # a child that faulted, aborted or timed out: no further child is started


def setting_rules(name, kind, shape, plans):
    """what each setting promises about the plan, from the comments at the switches' uses in conv.hip"""
    N = shape[1]
    fams = [p["family"] for p in plans]
    if kind == "wgrad":
        p = plans[0]
        if name in ("CONV4=0", "WGRAD4=0"):
            assert fams == ["wgrad"], (name, shape, plans)
        elif name == "WGRAD4=1 DH=3":
            assert (fams == ["wgrad4"]) == (N % 4 == 0 and N % 16 != 0) and p["DH"] <= 3 and p["branch"] != "rows", (name, shape, plans)
        else:
            assert (fams == ["wgrad4"]) == (N % 4 == 0), (name, shape, plans)
        return
    if name == "CONV4=0":
        assert set(fams) == {"fwd"}, (name, shape, plans)
    elif name.startswith("CONV4=2"):
        assert set(fams) == ({"fwd4"} if N % 4 == 0 else {"fwd"}), (name, shape, plans)
        for p in plans:
            if p["family"] == "fwd4":
                assert p["a2"] == (4 if p["a0"] == 4 else 2) and p["a0"] in ((3, 4) if name.endswith("KS=4") else (2, 3)), (name, shape, plans)
    elif name == "CONV_ROWS=0":
        assert len(plans) == 1 and plans[0]["branch"] == "whole" and plans[0]["FB"] == 1, (name, shape, plans)
    else:
        assert set(fams) == ({"fwd4"} if N % 4 == 0 and N != 16 else {"fwd"}), (name, shape, plans)


CHILD_CHECK_FAILED = 2         # exit status of a child whose launches all returned but a check failed; anything else nonzero: no further child


def worker_main(name):
    """exit status 0: passed; CHILD_CHECK_FAILED: an assertion failed (the card is fine); any other exception -- a HIP error out of an
    entry or of the synchronize is one -- leaves with the interpreter's status 1, which the parent treats like an abort or a time-out"""
    import traceback
    try:
        worker_body(name)
    except AssertionError:
        traceback.print_exc()
        sys.stdout.flush()
        sys.exit(CHILD_CHECK_FAILED)


def worker_body(name):
    eng = make_engine()
    for shape, _, opts in FWD:
        if name != "WGRAD4=0":
            plans = run_fwd(eng, shape, 3, setting=name, **opts)
            setting_rules(name, "fwd", shape, plans)
            cover(plans)
    if name == "CONV4=2 KS=4":
        for R in (1, 6, 7, 8, 17):                              # FB = 7 in the 512-position form with k' quarters
            plans = run_fwd(eng, (16, 32, 11, 257, 13), R, setting=name, bias=True)
            assert plans[1]["FB"] == 7
    for i, (shape, _) in enumerate(WGRAD):
        plans = run_wgrad(eng, shape, with_db=i % 3 != 1, setting=name)
        setting_rules(name, "wgrad", shape, plans)
        cover(plans)
    if name == "WGRAD4=1 DH=3":                                 # the searched branch on multi-strip frames: DH = 2 and DH = 3 by frame count
        for shape, DH, fpg in [((4, 5, 3, 200, 3, 15), 2, 1), ((4, 17, 3, 200, 3, 15), 2, 1), ((4, 5, 3, 200, 3, 20), 3, 1),
                               ((4, 17, 3, 200, 3, 20), 3, 1), ((4, 5, 5, 200, 3, 20), 2, 2), ((4, 17, 5, 200, 3, 20), 2, 2)]:
            plans = run_wgrad(eng, shape, setting=name)
            assert (plans[0]["DH"], plans[0]["fpg"], plans[0]["branch"]) == (DH, fpg, "search"), plans
            cover(plans)
    print("RESULT " + json.dumps({"covered": sorted(COVERED), "waves": sorted(WAVES), "errors": ERRORS}))


@pytest.mark.parametrize("name,env", SETTINGS, ids=[s[0].replace(" ", "_") for s in SETTINGS])
def test_switch_settings(name, env):
    if _CHILD_DEAD:                                            # (and, through the autouse fixture, after a HIP error in this process)
        pytest.fail("not started: the child for %s faulted, aborted, timed out or raised something that was no failed check" % _CHILD_DEAD[0])
    e = dict(os.environ)
    e.update(env)
    src = "import sys; sys.path.insert(0, %r); from tests import test_gpu_conv_ops as t; t.worker_main(%r)" % (ROOT, name)
    try:
        p = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, env=e, timeout=240)
    except subprocess.TimeoutExpired:
        _CHILD_DEAD.append(name)
        raise
    for line in p.stdout.splitlines():
        if line.startswith("conv_ops "):
            print(line)
    if p.returncode not in (0, CHILD_CHECK_FAILED):            # a signal, an abort, or an exception that was no failed check (a HIP error)
        _CHILD_DEAD.append(name)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    for fam, args, branch, fb, fpg in out["covered"]:
        COVERED.add((fam, tuple(args), branch, fb, fpg))
    for w in out["waves"]:
        WAVES.add(tuple(w))
    assert len(out["errors"]) >= len(WGRAD)


# ---------------------------------------------------------------------------------------------------------------------------------
# The ledger, from reading launch_conv_fwd / conv_fwd_range / launch_conv_wgrad / wgrad_plan / wgrad4_plan / wgrad4_waves, for the
# shapes of the issue's lists (W in {1..257}, S in {1, 3, 5, 7, 11}, fw in {1, 3, 7, 13}, N in {1, 3, 4, 5, 12, 16, 17, 20, 31, 32},
# C in {1, 4, 8, 12, 16, 24, 32}) plus C = 20 / fw = 13 / N = 12 (the one supported shape family with fw * C > 256).
#
# Forward.  RT = 4 or 6 by conv_fwd_plan, NT = 2 above 16 output channels.  The row-aligned main launch is always RT = 6 (G = 3 in the
# 4x4x1 form); the remainder of these widths (W % 64 in {1, 8}) is one strip of RT = 4, and one strip always takes FB > 1 (cap =
# 512 / (S * TWr) >= 5, the LDS fits >= 7 frames), so "rem" comes with FB > 1 and only with RT = 4 (G = 2, or 4 under CONV4_KS=4);
# "whole" (W <= 64, or CONV_ROWS=0) takes either RT.  ncg = N / 4 in {1, 3, 5, 8} by default (N = 16 stays on 16x16x4), plus 4
# under CONV4=2.  KS=4 only changes the RT = 4 form (G = 4, KS = 4).
LEDGER_FWD = (
    [("fwd", (rt, nt), "whole", False, False) for rt in (4, 6) for nt in (1, 2)] +
    [("fwd", (6, nt), "main", False, False) for nt in (1, 2)] +
    [("fwd", (4, nt), "rem", True, False) for nt in (1, 2)] +
    [("fwd4", (g, ncg, 2), "whole", False, False) for g in (2, 3) for ncg in (1, 3, 4, 5, 8)] +
    [("fwd4", (3, ncg, 2), "main", False, False) for ncg in (1, 3, 4, 5, 8)] +
    [("fwd4", (2, ncg, 2), "rem", True, False) for ncg in (1, 3, 4, 5, 8)] +
    [("fwd4", (4, ncg, 4), br, br == "rem", False) for ncg in (1, 3, 4, 5, 8) for br in ("whole", "rem")])
# Weight gradient, 16x16x4 (N % 4 != 0, or the 4x4x1 form switched off): KT = 2 iff K' > 256, NT = 2 above 16 channels.  One strip:
# searched, DH = 1.  Multi-strip: K' > 256 -> "k2" with DH = 3 (KT = 2 only); K' <= 256 -> "rows" with DH = 6 (S in {3, 5, 11}) or
# 4 (S = 7; S = 1 has one strip at these widths); under WGRAD_DH=3 the K' <= 256 shapes are searched over DH = 1..3 (the fewest
# frames per group wins, the smaller DH on a tie: 1, 2 and 3 all occur).  Every plan with and without fpg > 1 (R above gmax).
LEDGER_WGRAD = (
    [("wgrad", (kt, nt, 1), "search", False, f) for kt in (1, 2) for nt in (1, 2) for f in (False, True)] +
    [("wgrad", (2, nt, 3), "k2", False, f) for nt in (1, 2) for f in (False, True)] +
    [("wgrad", (1, nt, dh), "rows", False, f) for nt in (1, 2) for dh in (4, 6) for f in (False, True)] +
    [("wgrad", (1, nt, dh), "search", False, f) for nt in (1, 2) for dh in (2, 3) for f in (False, True)])
# 4x4x1 (N % 4 == 0): template arguments (N / 4, 3, waves).  wgrad4_plan passes min(K', 256) for nkg <= 4, so "k2" needs nkg = 5
# (fw * C in 257..320: C = 20, fw = 13 only, since 32 * ldf / 4 <= 2560 bounds K').  wgrad4_waves: roles = nkg * ceil(DH / 3):
# 1, 2, 3, 4, 6 -> 12 waves (PS 12, 6, 4, 3, 2), 5 -> 10 waves (PS 2), 8 -> 8 waves (PS 1).  One strip is searched (DH = 1, 12 or
# 10 waves); multi-strip is "rows" (12 waves up to nkg = 3, 8 waves at nkg = 4) or "k2" (10 waves).
LEDGER_WGRAD4 = (
    [("wgrad4", (ncg, 3, 12), br, False, f) for ncg in (1, 3, 4, 5, 8) for br in ("search", "rows") for f in (False, True)] +
    [("wgrad4", (ncg, 3, 8), "rows", False, f) for ncg in (1, 3, 4, 5, 8) for f in (False, True)] +
    [("wgrad4", (3, 3, 10), br, False, f) for br in ("search", "k2") for f in (False, True)])
LEDGER = set(LEDGER_FWD + LEDGER_WGRAD + LEDGER_WGRAD4)
LEDGER_WAVES = {(16, 1, 0), (12, 12, 1), (12, 6, 1), (12, 6, 2), (12, 3, 2), (12, 4, 3), (12, 2, 3), (12, 3, 4), (8, 1, 4), (10, 2, 5)}


N_TESTS = len(FWD) + 3 + 1 + len(WGRAD) + 2 + 1 + 1 + len(SETTINGS) + 1      # every test item of this module, the ledger included


def test_zz_ledger(request):
    """prints every combination a passing case asserted and compares them with the hand-written ledger.  Only a run that deselected
    tests of this module (-k, a node id) is excused: then nothing can be required"""
    print("conv_ops combinations asserted by passing cases: %d of %d" % (len(COVERED & LEDGER), len(LEDGER)))
    for c in sorted(COVERED):
        print("  conv_ops covered %s" % (c,))
    print("conv_ops achieved errors: max %.2e over %d launches" % (max([e[3] for e in ERRORS] + [0.0]), len(ERRORS)))
    mine = [i for i in request.session.items if i.nodeid.split("::")[0].endswith("test_gpu_conv_ops.py")]
    if len(mine) != N_TESTS:
        print("conv_ops partial run (%d of %d tests selected): the ledger is not compared" % (len(mine), N_TESTS))
        return
    assert LEDGER - COVERED == set(), ("combinations no passing case reached", sorted(LEDGER - COVERED))
    assert COVERED - LEDGER == set(), ("combinations missing from the hand-written ledger", sorted(COVERED - LEDGER))
    assert WAVES == LEDGER_WAVES, (sorted(WAVES - LEDGER_WAVES), sorted(LEDGER_WAVES - WAVES))
