"""csrc/segan.hip launcher by launcher, and the window-GEMM primitives of csrc/segan.cpp (conv2_fwd, conv2_wgrad, tconv2), each through the
host function SeganModel calls (rsrgan_op_segan_*) on caller-owned buffers, against fp64 references on the CPU from the same
fp32-rounded inputs.  Every case asserts its numbers first and, for the column reductions, the kernel form that ran
(rsrgan_op_segan_last_plan) second, so a plan failure says the arithmetic was right.

References.  Strided convolution: torch conv1d at stride 2 over an input zero-padded by hand with TensorFlow's SAME rule
(oracle/segan_oracle.py:downconv); every transposed convolution and every weight gradient is fp64 autograd of that forward (no parity
class and no flip is re-derived here).  VBN: vbn_stats / vbn_apply / leaky of the oracle and their autograd.  Head: conv1d_same + the
FC and their autograd.  Layout kernels: the index formula in numpy.  RMSProp, LSGAN, L1: the formulas in fp64.

Guards.  Operands are noise plus an index ramp, with NaN guard rows on both sides and NaN columns beyond their row; every output
buffer is sentinel-filled and must come back bit-unchanged outside its valid extent; scratch is NaN up to its stated size with a
sentinel band behind it; pad, t0, t1 of the window-GEMM entries hold 1e30 up to the model's size for that layer and NaN beyond it (a
view that leaves the rows launch_pad_rows wrote shows up as 1e30-sized garbage or NaN; a read multiplied by a zero K-padding column
does not); every launch runs twice, from fresh buffers, and must be bit-identical.

Bounds.  Pure moves: bit-equal.  Elementwise kernels: within 1 ulp of the fp64 value rounded to fp32; where the kernel adds terms
(accumulate, extra, k1 + k2 h) the ulp is that of the largest term, since each rounding is half an ulp of what it rounds.  GEMM-backed
results and the conv1 / head products: max |err| / max(|ref|_max, 1) < 2e-5.  Reductions (colred, sum_all, the losses, the
conv1 weight gradient, dwfc / dbfc, dgamma / dbeta, and the VBN backward chain that hangs on them): 6l's rule, the kernel's error
against fp64 is at most 4 x the error of the same sums accumulated in fp32 in plain row order on the CPU, both maxima over at least 16
independent sums (narrow shapes run 16 / C windows with fresh data); both figures are printed per case.  The VBN coefficients
(launch_vbn_coef) get a per-column bound from the number formats, derived at vbn_coef_tolerance.

test_mutations_exceed_the_bound (CPU) applies eight mistakes to the references and requires each to break its bound.
RSRGAN_COLRED_VEC=0 and =15 each run the whole column-reduction table in one fresh child process.  COVERED collects (mode, form,
chunk doubled, P > 1) of every passing column reduction; test_zz_ledger compares it with LEDGER, written by hand."""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from oracle import segan_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 7.0
BIG = 1e30
GUARD = 3                      # guard rows before and behind every matrix
BAND = 1024                    # sentinel / NaN floats behind scratch buffers
TOL = 2e-5                     # max |err| / max(|ref|_max, 1)
F32, F64 = np.float32, np.float64
NAN = float("nan")
COVERED = set()                # (mode, vec, chunk doubled, P > 1) of every passing column reduction
LINES = []                     # one report line per case
WORST = {}                     # output -> largest error on the project's scale (or in ulp)
_FAULTED = []                  # a launch that raised (a HIP error, not a failed assertion): nothing more is started on the GPU
_CHILD_DEAD = []
CHILD_CHECK_FAILED = 3


def make_engine():
    from rsrgan_amd.ops import OpEntries
    return OpEntries()


@pytest.fixture(scope="module")
def eng():
    return make_engine()


@pytest.fixture(autouse=True)
def _stop_after_a_fault(request):
    if _FAULTED and not request.node.name.startswith("test_mutations"):
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
    wrapped.__name__ = fn.__name__
    return wrapped


def pad4(n):
    return (n + 3) // 4 * 4


def rng(*seed):
    return np.random.default_rng([17] + [int(v) for v in seed])


def noise(g, *shape):
    """fp32 noise plus a ramp over the last two indices"""
    x = g.standard_normal(shape).astype(F32)
    idx = np.indices(shape[-2:]) if len(shape) >= 2 else np.indices((1, shape[-1]))
    ramp = 0.03 * (((5 * idx[0] + 3 * idx[1]) % 11) - 5)
    return (x + ramp.reshape(shape[-2:] if len(shape) >= 2 else shape).astype(F32)).astype(F32)


def report(line):
    LINES.append(line)
    print("segan_ops " + line)


def note(name, err):
    WORST[name] = max(WORST.get(name, 0.0), float(err))


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return bool(torch.equal(bits(a), bits(b)))


# ---------------------------------------------------------------------------------------------------------------------------------
# device buffers with guards
# ---------------------------------------------------------------------------------------------------------------------------------
class Dev:
    """buffers of one case on the engine's device; run(fn) calls fn(i) for i = 0, 1 on two fresh sets and compares every output"""

    def __init__(self, eng):
        self.dev = eng.device
        self.outs, self.scr = [], []

    def inp(self, mat, ld=None, fill=NAN):
        """operand [rows][cols] -> device view inside [GUARD + rows + GUARD][ld], everything else NaN; 1-D: a row vector"""
        m = torch.as_tensor(np.ascontiguousarray(mat, dtype=F32))
        one = m.ndim == 1
        m = m.reshape(1, -1) if one else m.reshape(-1, m.shape[-1])
        rows, cols = m.shape
        ld = cols if ld is None else ld
        whole = torch.full((rows + 2 * GUARD, ld), fill, dtype=torch.float32)
        whole[GUARD:GUARD + rows, :cols] = m
        whole = whole.to(self.dev)
        v = whole[GUARD:GUARD + rows]
        return v[0] if one else v

    def out(self, rows, cols, ld=None, col0=0, init=None):
        """two sentinel-filled outputs [GUARD + rows + GUARD][ld]; the valid extent is rows x [col0, col0 + cols) (init: its start values)"""
        ld = col0 + cols if ld is None else ld
        cpu0 = torch.full((rows + 2 * GUARD, ld), SENT, dtype=torch.float32)
        if init is not None:
            cpu0[GUARD:GUARD + rows, col0:col0 + cols] = torch.as_tensor(np.ascontiguousarray(init, dtype=F32)).reshape(rows, cols)
        o = dict(cpu0=cpu0, bufs=[cpu0.to(self.dev), cpu0.to(self.dev)], rows=rows, cols=cols, col0=col0)
        self.outs.append(o)
        return o

    @staticmethod
    def view(o, i):
        return o["bufs"][i][GUARD:GUARD + o["rows"]]

    def scratch(self, floats, fill=NAN, behind=SENT):
        """two buffers of `floats` floats (NaN: never read before written) with a band behind them that must not change"""
        cpu0 = torch.cat([torch.full((floats,), fill, dtype=torch.float32), torch.full((BAND,), behind, dtype=torch.float32)])
        s = dict(cpu0=cpu0, bufs=[cpu0.to(self.dev), cpu0.to(self.dev)], floats=floats)
        self.scr.append(s)
        return s

    def run(self, fn):
        for i in range(2):
            fn(i)
        torch.cuda.synchronize()
        res = []
        for s in self.scr:
            for b in s["bufs"]:
                assert same_bits(b.cpu()[s["floats"]:], s["cpu0"][s["floats"]:]), "the band behind a scratch buffer was written"
        for o in self.outs:
            a, b = o["bufs"][0].cpu(), o["bufs"][1].cpu()
            assert same_bits(a, b), "two runs of one launch differ"
            r0, r1, c0, c1 = GUARD, GUARD + o["rows"], o["col0"], o["col0"] + o["cols"]
            exp = o["cpu0"].clone()
            exp[r0:r1, c0:c1] = a[r0:r1, c0:c1]
            assert same_bits(a, exp), "written outside the valid extent"
            res.append(a[r0:r1, c0:c1].numpy().astype(F64))
        return res


def relerr(got, ref):
    ref = np.asarray(ref, F64)
    assert np.isfinite(got).all(), "non-finite output (a guard was read)"
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1.0))


def ulp32(x):
    return np.spacing(np.maximum(np.abs(np.asarray(x, F64)).astype(F32), np.finfo(F32).tiny)).astype(F64)


def ulps(got, ref, scale=None):
    """largest |got - fl32(ref)| in ulp32 of max(|ref|, scale)"""
    assert np.isfinite(got).all(), "non-finite output (a guard was read)"
    r32 = np.asarray(ref, F64).astype(F32).astype(F64)
    mag = np.abs(r32) if scale is None else np.maximum(np.abs(r32), np.abs(scale))
    return float((np.abs(got - r32) / ulp32(mag)).max())


def seqsum(terms):
    """fp32 sums in plain row order over axis 0"""
    t = np.ascontiguousarray(terms, dtype=F32)
    if t.shape[0] == 0:
        return np.zeros(t.shape[1:], F32)
    return np.cumsum(t.reshape(t.shape[0], -1), axis=0, dtype=F32)[-1].reshape(t.shape[1:])


def reduction_rule(name, case, kernel_err, plain_err, nsums):
    assert nsums >= 16, (name, nsums)
    report("%s %s kernel %.3e plain %.3e sums %d" % (name, case, kernel_err, plain_err, nsums))
    note(name, kernel_err)
    assert kernel_err <= 4.0 * plain_err, (name, case, kernel_err, plain_err)


# ---------------------------------------------------------------------------------------------------------------------------------
# strided convolution as a window GEMM: conv2_fwd, conv2_wgrad, tconv2
# ---------------------------------------------------------------------------------------------------------------------------------
LS, KS, CS, BNS = [1, 2, 3, 4, 5, 37, 64, 65], [2, 3, 5, 6, 20, 31], [16, 48, 80], [1, 3, 7]
CONV2 = [(L, k, CS[(i + j) % 3], CS[(i + 2 * j + 1) % 3], BNS[(i + j) % 3], (i + j) % 2 == 0) for i, L in enumerate(LS) for j, k in enumerate(KS)]
_REF = {}                      # fp64 references, computed once per case and left unchanged


def conv2_data(L, k, Cin, Cout, Bn):
    key = ("conv2", L, k, Cin, Cout, Bn)
    if key not in _REF:
        g = rng(1, L, k, Cin, Cout, Bn)
        Lo = (L + 1) // 2
        x, W = noise(g, Bn, L, Cin), noise(g, k * Cin, Cout).reshape(k, 1, Cin, Cout)
        bz, bt = noise(g, Cout), noise(g, Cin)
        dz = noise(g, Bn, Lo, Cout)
        x64 = torch.tensor(x.astype(F64), requires_grad=True)
        W64 = torch.tensor(W.astype(F64), requires_grad=True)
        z = O.downconv(x64, W64, None)
        (z * torch.tensor(dz.astype(F64))).sum().backward()
        _REF[key] = dict(x=x, W=W, bz=bz, bt=bt, dz=dz, z=z.detach().numpy(), dW=W64.grad.numpy().reshape(k * Cin, Cout), dx=x64.grad.numpy())
    return _REF[key]


@stops_the_module
def run_conv2(eng, L, k, Cin, Cout, Bn, bias):
    d = conv2_data(L, k, Cin, Cout, Bn)
    Lo = (L + 1) // 2
    case = "L=%d k=%d Cin=%d Cout=%d Bn=%d bias=%d" % (L, k, Cin, Cout, Bn, bias)
    pad_n = eng.op_segan_sizes(0, [Bn, L, Cin, k])[0]
    # forward
    D = Dev(eng)
    X, Wd = D.inp(d["x"]), D.inp(d["W"].reshape(k * Cin, Cout), ld=Cout + 4)
    bd = D.inp(d["bz"]) if bias else None
    Z, pad = D.out(Bn * Lo, Cout), D.scratch(pad_n, fill=BIG, behind=NAN)
    (z,) = D.run(lambda i: eng.op_segan("conv2", "conv2_fwd", [X, Wd, bd, D.view(Z, i), pad["bufs"][i]], [Bn, L, Cin, k, Cout, Cout + 4, pad_n]))
    e_f = relerr(z, d["z"].reshape(Bn * Lo, Cout) + (d["bz"].astype(F64) if bias else 0.0))
    # weight gradient
    D = Dev(eng)
    X, dZ = D.inp(d["x"]), D.inp(d["dz"], ld=Cout + 8)
    dW, pad = D.out(k * Cin, Cout, ld=Cout + 4), D.scratch(pad_n, fill=BIG, behind=NAN)
    (dw,) = D.run(lambda i: eng.op_segan("conv2", "conv2_wgrad", [X, dZ, D.view(dW, i), pad["bufs"][i]], [Bn, L, Cin, k, Cout, Cout + 8, Cout + 4, pad_n]))
    e_w = relerr(dw, d["dW"])
    # the data gradient: the transposed convolution Lo -> L (L even: Lt = 2 Ls; odd: Lt = 2 Ls - 1) of Cout -> Cin channels
    s = eng.op_segan_sizes(1, [Bn, Lo, Cout, L, Cin, k])
    D = Dev(eng)
    S, Wd = D.inp(d["dz"]), D.inp(d["W"].reshape(k * Cin, Cout), ld=Cout + 4)
    bd = D.inp(d["bt"]) if bias else None
    T = D.out(Bn * L, Cin)
    pad, t0, t1 = (D.scratch(n, fill=BIG, behind=NAN) for n in (s[0], s[1], s[1]))
    w0, w1 = D.scratch(s[2]), D.scratch(s[3])
    (t,) = D.run(lambda i: eng.op_segan("conv2", "tconv2", [S, Wd, bd, D.view(T, i), pad["bufs"][i], t0["bufs"][i], t1["bufs"][i], w0["bufs"][i], w1["bufs"][i]],
                                        [Bn, Lo, Cout, L, k, Cin, Cout + 4, s[0], s[1], s[2], s[3]]))
    e_t = relerr(t, d["dx"].reshape(Bn * L, Cin) + (d["bt"].astype(F64) if bias else 0.0))
    report("conv2 %s fwd %.2e wgrad %.2e tconv2 %.2e Q=(%d,%d) pf=%d pb=%d" % (case, e_f, e_w, e_t, s[7], s[8], s[9], s[10]))
    for n_, e in (("conv2_fwd", e_f), ("conv2_wgrad", e_w), ("tconv2", e_t)):
        note(n_, e)
        assert e < TOL, (n_, case, e)
    if L == 1:
        assert 0 in (s[7], s[8])                           # Ls = Lt = 1: one empty parity class (the `continue`, max(Q, 1))


@pytest.mark.parametrize("L,k,Cin,Cout,Bn,bias", CONV2, ids=["L%d_k%d_%dto%d_B%d" % c[:5] for c in CONV2])
def test_conv2(eng, L, k, Cin, Cout, Bn, bias):
    run_conv2(eng, L, k, Cin, Cout, Bn, bias)


# ---------------------------------------------------------------------------------------------------------------------------------
# the single-channel ends: conv1_fwd, conv1_wgrad, tconv1
# ---------------------------------------------------------------------------------------------------------------------------------
L1S = [1, 2, 5, 37, 1023, 1024, 1025, 2047, 2051]       # Lo on both sides of C1_SUB = 512 and of the 1024-position chunk
KC1 = [(2, 16), (16, 16), (21, 48), (32, 32)]            # k * C = 32, 256, 1008, 1024 exactly
CONV1 = [(L, k, C, 1 + 2 * ((i + j) % 2), 0) for i, L in enumerate(L1S) for j, (k, C) in enumerate(KC1)]
CONV1 += [(4100, 2, 16, 3, 1), (2051, 21, 48, 1, 1)]     # scratch of B * k * C floats: the chunk doubles twice (Lo = 2050) / once


def conv1_data(L, k, C, B):
    key = ("conv1", L, k, C, B)
    if key not in _REF:
        g = rng(2, L, k, C, B)
        Lo = (L + 1) // 2
        x, W, b, bt, dz = noise(g, B, L), noise(g, k, C), noise(g, C), noise(g, 1), noise(g, B, Lo, C)
        x64 = torch.tensor(x.astype(F64), requires_grad=True)
        W64 = torch.tensor(W.astype(F64).reshape(k, 1, 1, C), requires_grad=True)
        z = O.downconv(x64[..., None], W64, None)
        (z * torch.tensor(dz.astype(F64))).sum().backward()
        _REF[key] = dict(x=x, W=W, b=b, bt=bt, dz=dz, z=z.detach().numpy(), dW=W64.grad.numpy().reshape(k, C), dx=x64.grad.numpy())
    return _REF[key]


def conv1_wgrad_plain(x, dz, k, drop_last_row_of_chunk=0):
    """dW[dk][c] = sum over (b, o) in plain order of x[b, 2o + dk - pl] dz[b, o, c], products and sums in fp32"""
    B, L = x.shape
    Lo, C = dz.shape[1], dz.shape[2]
    pl = max((Lo - 1) * 2 + k - L, 0) // 2
    xp = np.zeros((B, 2 * Lo + k + 2), F32)
    xp[:, pl:pl + L] = x
    out = np.zeros((k, C), F32)
    keep = np.ones(Lo, bool)
    if drop_last_row_of_chunk:
        keep[drop_last_row_of_chunk - 1::drop_last_row_of_chunk] = False
    for dk in range(k):
        win = xp[:, dk:dk + 2 * Lo:2][:, keep]                                # [B][Lo]
        out[dk] = seqsum((win[:, :, None] * dz[:, keep]).reshape(-1, C))
    return out


@stops_the_module
def run_conv1(eng, L, k, C, B, small):
    d = conv1_data(L, k, C, B)
    Lo, ldx = (L + 1) // 2, L + 5
    case = "L=%d k=%d C=%d B=%d small=%d" % (L, k, C, B, small)
    D = Dev(eng)
    X, Wd, bd = D.inp(d["x"], ld=ldx), D.inp(d["W"], ld=C + 4), D.inp(d["b"])
    Z = D.out(B * Lo, C, ld=C + 4)
    (z,) = D.run(lambda i: eng.op_segan("conv1", "conv1_fwd", [X, Wd, bd, D.view(Z, i)], [B, L, k, C, ldx, C + 4, C + 4]))
    e_f = relerr(z, d["z"].reshape(B * Lo, C) + d["b"].astype(F64))
    # weight gradient: default scratch = one partial per 1024-position chunk and batch row; small: B * k * C floats
    nch = (Lo + 1023) // 1024
    sf = B * k * C if small else B * nch * k * C
    D = Dev(eng)
    X, dZ = D.inp(d["x"], ld=ldx), D.inp(d["dz"], ld=C + 4)
    dW, scr = D.out(k, C, ld=C + 4), D.scratch(sf)
    (dw,) = D.run(lambda i: eng.op_segan("conv1", "conv1_wgrad", [X, dZ, D.view(dW, i), scr["bufs"][i]], [B, L, k, C, ldx, C + 4, C + 4, sf]))
    plain = conv1_wgrad_plain(d["x"], d["dz"], k)
    # transposed: t[b, i] = the data gradient of the same layer (+ bias)
    D = Dev(eng)
    S, Wd, bd = D.inp(d["dz"], ld=C + 4), D.inp(d["W"], ld=C + 4), D.inp(d["bt"])
    T = D.out(B, L, ld=ldx)
    (t,) = D.run(lambda i: eng.op_segan("conv1", "tconv1", [S, Wd, bd, D.view(T, i)], [B, Lo, C, L, k, C + 4, C + 4, ldx]))
    e_t = relerr(t, d["dx"] + float(d["bt"][0]))
    report("conv1 %s fwd %.2e tconv1 %.2e" % (case, e_f, e_t))
    for n_, e in (("conv1_fwd", e_f), ("tconv1", e_t)):
        note(n_, e)
        assert e < TOL, (n_, case, e)
    reduction_rule("conv1_wgrad", case, np.abs(dw - d["dW"]).max(), np.abs(plain.astype(F64) - d["dW"]).max(), k * C)


@pytest.mark.parametrize("L,k,C,B,small", CONV1, ids=["L%d_k%d_C%d_B%d_s%d" % c for c in CONV1])
def test_conv1(eng, L, k, C, B, small):
    run_conv1(eng, L, k, C, B, small)


# ---------------------------------------------------------------------------------------------------------------------------------
# launch_colred: four modes, two forms
# ---------------------------------------------------------------------------------------------------------------------------------
CRED_C = [1, 5, 12, 16, 48, 255, 256, 257, 300, 1024, 1028]
CRED_R = [1, 7, 63, 64, 65, 1000, 20000]
# (C, rows_per, P, coff (lda = 2 C), accumulate, scratch: "default" | "min" (P x 2 x C: the chunk doubles to one per pass) | "exact" | "below")
COLRED = [(C, CRED_R[(2 * i + j) % 7], 1 + (i + j) % 3, 0, (i + j) % 4 == 0, "default") for i, C in enumerate(CRED_C) for j in range(3)
          if not (C >= 256 and CRED_R[(2 * i + j) % 7] == 20000)]              # (20000 rows: at C = 12, 16, 257 below)
COLRED += [(12, 20000, 2, 0, False, "default"), (257, 20000, 1, 0, False, "default"), (1028, 1000, 3, 0, False, "default"),
           (48, 65, 2, 48, False, "default"), (5, 63, 1, 5, True, "default"), (256, 64, 3, 256, False, "default"),
           (5, 1000, 1, 0, False, "min"), (5, 1000, 3, 0, False, "min"), (16, 1000, 1, 0, False, "min"), (16, 1000, 2, 0, True, "min"),
           (48, 1000, 2, 0, False, "exact"), (48, 1000, 2, 0, False, "below"), (255, 1000, 1, 0, False, "exact"), (255, 1000, 3, 0, False, "below")]
LEAK = 0.3


def colred_vec_expected(mode, C, mask):
    """launch_colred takes the 16-byte form when the mode's bit is set and C, lda = C + 8 (or 2 C), coff, ldb = C + 4, ldcoef = C + 4 are multiples of 4"""
    return bool((mask >> mode) & 1) and C % 4 == 0


def colred_refs(C, rows, P, w):
    key = ("colred", C, rows, P, w)
    if key not in _REF:
        g = rng(3, C, rows, P, w)
        a = noise(g, P * rows, C) + F32(0.25)
        b = noise(g, P * rows, C)
        coef = np.zeros((P * 8, C), F32)
        for p in range(P):
            coef[p * 8 + 0] = noise(g, C) * F32(0.1) + F32(0.25)             # mu
            coef[p * 8 + 3] = g.uniform(0.5, 1.5, C).astype(F32) * np.where(g.random(C) < 0.5, -1, 1).astype(F32)    # sc, signed
            coef[p * 8 + 4] = noise(g, C) * F32(0.5)                          # sh
        a3, b3 = a.reshape(P, rows, C), b.reshape(P, rows, C)
        a64, b64 = a3.astype(F64), b3.astype(F64)
        mu, sc, sh = (coef[k_::8].astype(F64)[:, None, :] for k_ in (0, 3, 4))
        side = a64 * sc + sh >= 0                                             # exact sign: the product of two floats is exact in fp64
        g64 = b64 * np.where(side, 1.0, F64(F32(LEAK)))
        g32 = (b3 * np.where(side, F32(1), F32(LEAK)).astype(F32)).astype(F32)
        ref = {0: (a64.sum(1), None), 1: ((a64 * np.minimum(b64, 0)).sum(1), None), 2: (a64.sum(1), (a64 * a64).sum(1)),
               3: (g64.sum(1), (g64 * (a64 - mu)).sum(1))}
        pl = lambda t: np.stack([seqsum(t[p]) for p in range(P)]).astype(F64)
        plain = {0: (pl(a3), None), 1: (pl(a3 * np.minimum(b3, F32(0))), None), 2: (pl(a3), pl(a3 * a3)),
                 3: (pl(g32), pl(g32 * (a3 - coef[0::8][:, None, :])))}
        _REF[key] = dict(a=a, b=b, coef=coef, ref=ref, plain=plain)
    return _REF[key]


@stops_the_module
def run_colred(eng, C, rows, P, coff, acc, scratch, mask, setting="default"):
    windows = max(1, -(-16 // C))
    lda = 2 * C if coff else C + 8
    for mode in range(4):
        vec = colred_vec_expected(mode, C, mask)
        base = 64 if vec else 256
        nout, two = (2 if mode >= 2 else 1), mode in (1, 3)
        need_default = -(-rows // base) * P * 2 * C
        sf = {"default": max(need_default, 4096), "min": P * 2 * C, "exact": need_default, "below": need_default - 1}[scratch]
        kerr = perr = 0.0
        for w in range(windows):
            r = colred_refs(C, rows, P, w)
            init = noise(rng(4, C, P, mode, w), P * nout, C)
            D = Dev(eng)
            A = D.inp(np.concatenate([np.full((P * rows, coff), NAN, F32), r["a"]], 1) if coff else r["a"], ld=lda)
            Bm = D.inp(r["b"], ld=C + 4) if two else None
            Cf = D.inp(r["coef"], ld=C + 4) if mode == 3 else None
            out, scr = D.out(P * nout, C, ld=C + 4, init=init if acc else None), D.scratch(sf)
            plans = []

            def launch(i):
                eng.op_segan("colred", ("sum", "dalpha", "moments", "vbn_bwd")[mode], [A, Bm, Cf, D.view(out, i), scr["bufs"][i]],
                             [lda, coff, C + 4, C, rows, P, C + 4, C + 4, 1 if acc else 0, sf], [LEAK])
                plans.append(eng.op_segan_last_plan())
            (got,) = D.run(launch)
            ref = np.stack([r["ref"][mode][j][p] for p in range(P) for j in range(nout)])
            plain = np.stack([r["plain"][mode][j][p] for p in range(P) for j in range(nout)])
            if acc:
                ref = ref + init.astype(F64)
                plain = (init + plain.astype(F32)).astype(F64)
            kerr, perr = max(kerr, np.abs(got - ref).max()), max(perr, np.abs(plain - ref).max())
        case = "%s C=%d rows=%d P=%d coff=%d acc=%d scratch=%s mode=%d" % (setting, C, rows, P, coff, acc, scratch, mode)
        reduction_rule("colred", case, kerr, perr, windows * C * P * nout)
        # the plan second: the form, and whether the chunk doubled, from reading launch_colred
        p = plans[-1]
        chunks_default = -(-rows // base)
        doubled = scratch in ("min", "below") and chunks_default > 1 or chunks_default > (256 if vec else 128) or (vec and chunks_default * P > 4096)
        report("colred-plan %s vec=%d chunk=%d chunks_per=%d grid=%d" % (case, p["vec"], p["chunk"], p["chunks_per"], p["grid"]))
        assert (p["vec"], p["mode"]) == (int(vec), mode), (case, p)
        assert (p["chunk"] > base) == bool(doubled) and p["chunks_per"] == -(-rows // p["chunk"]) and p["grid"] == P * p["chunks_per"], (case, p)
        assert p["chunks_per"] * P * 2 * C <= sf and (p["chunk"] == base or (p["chunk"] // 2) & (p["chunk"] // 2 - 1) == 0), (case, p)
        if scratch == "min":
            assert p["chunks_per"] == 1, (case, p)
        COVERED.add((mode, int(vec), bool(doubled), P > 1))


@pytest.mark.parametrize("C,rows,P,coff,acc,scratch", COLRED, ids=["C%d_r%d_P%d_o%d_a%d_%s" % c for c in COLRED])
def test_colred(eng, C, rows, P, coff, acc, scratch):
    run_colred(eng, C, rows, P, coff, acc, scratch, mask=11)


def test_colred_short_scratch_is_refused(eng):
    """one float below one chunk per pass: refused before anything runs, not a loop that never ends"""
    from rsrgan_amd._lib import RsrganError
    a = torch.zeros(64, 16, device=eng.device)
    out, scr = torch.zeros(4, 16, device=eng.device), torch.zeros(256, device=eng.device)
    t0 = time.time()
    with pytest.raises(RsrganError, match="scratch of 63 floats below"):
        eng.op_segan("colred", "sum", [a, None, None, out, scr], [16, 0, 16, 16, 64, 2, 16, 16, 0, 63], [LEAK])
    assert time.time() - t0 < 1.0


def worker_main(name):
    try:
        eng = make_engine()
        mask = int(os.environ["RSRGAN_COLRED_VEC"])
        for c in COLRED:
            run_colred(eng, *c, mask=mask, setting=name)
        print("RESULT " + json.dumps({"covered": sorted(COVERED), "lines": len(LINES)}))
    except AssertionError:
        import traceback
        traceback.print_exc()
        sys.exit(CHILD_CHECK_FAILED)


@pytest.mark.parametrize("mask", [0, 15])
def test_colred_switch_settings(mask):
    name = "RSRGAN_COLRED_VEC=%d" % mask
    if _CHILD_DEAD:
        pytest.fail("not started: the child for %s faulted, aborted, timed out or raised something that was no failed check" % _CHILD_DEAD[0])
    e = dict(os.environ)
    e["RSRGAN_COLRED_VEC"] = str(mask)
    src = "import sys; sys.path.insert(0, %r); from tests import test_gpu_segan_ops as t; t.worker_main(%r)" % (ROOT, name)
    try:
        p = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, env=e, timeout=240)
    except subprocess.TimeoutExpired:
        _CHILD_DEAD.append(name)
        raise
    for line in p.stdout.splitlines():
        if line.startswith("segan_ops "):
            print(line)
    if p.returncode not in (0, CHILD_CHECK_FAILED):
        _CHILD_DEAD.append(name)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    for mode, vec, doubled, pgt in out["covered"]:
        COVERED.add((mode, vec, bool(doubled), bool(pgt)))
    assert out["lines"] >= 8 * len(COLRED)


# ---------------------------------------------------------------------------------------------------------------------------------
# virtual batch norm
# ---------------------------------------------------------------------------------------------------------------------------------
EPS = float(F32(1e-5))
VBN = [(C, rows, 1 + 2 * ((i + j) % 2)) for i, C in enumerate([16, 48, 257]) for j, rows in enumerate([1, 9, 1000])]
SCEN = {"D": dict(P=3, ref=False, p0=0), "G": dict(P=2, ref=False, p0=1), "R": dict(P=2, ref=True, p0=0)}
U = 2.0 ** -24


def vbn_case(C, rows, B, scen):
    """h [P][rows][C] with a column of |mean| >> sigma and a constant column; gamma signed, beta nonzero; the fp64 forward and backward of
    the oracle's VBN (pass 0 is the reference pass unless ref statistics are given; passes >= p0 carry a gradient)"""
    key = ("vbn", C, rows, B, scen)
    if key in _REF:
        return _REF[key]
    sc_ = SCEN[scen]
    P, p0 = sc_["P"], sc_["p0"]
    g = rng(5, C, rows, B, P, p0, sc_["ref"])
    h = (noise(g, P * rows, C) * g.uniform(0.5, 2.0, C).astype(F32) + g.normal(0, 1.0, C).astype(F32)).reshape(P, rows, C)
    h[:, :, 1] = F32(30.0 if rows > 1 else 3.0) + g.standard_normal((P, rows)).astype(F32)           # |mean| >> sigma: E[h^2] - E[h]^2 loses 3 digits in fp32
    h[:, :, 2] = F32(0.5)                                                        # constant: the variance is eps and rounding residue
    gamma = (g.uniform(0.5, 2.0, C) * np.where(g.random(C) < 0.5, -1, 1)).astype(F32)
    beta = g.normal(0, 1, C).astype(F32)
    dy = noise(g, P * rows, C).reshape(P, rows, C)
    mr_ = g.uniform(-1, 1, C)
    ref_mq = np.stack([mr_, mr_ * mr_ + g.uniform(0.5, 2, C)]).astype(F32) if sc_["ref"] else None
    c = 1.0 / (B + 1.0)
    h64 = torch.tensor(h.astype(F64), requires_grad=True)
    g64, b64 = torch.tensor(gamma.astype(F64), requires_grad=True), torch.tensor(beta.astype(F64), requires_grad=True)
    stats, ys = [], []
    for p in range(P):
        m, q = O.vbn_stats(h64[p][None])
        if ref_mq is not None:
            mr, qr = torch.tensor(ref_mq[0].astype(F64)), torch.tensor(ref_mq[1].astype(F64))
            m, q = c * m + (1 - c) * mr, c * q + (1 - c) * qr
        elif p > 0:
            mr, qr = stats[0]
            if p0 > 0:                                     # the G-run's backward treats the reference pass as a constant
                mr, qr = mr.detach(), qr.detach()
            m, q = c * m + (1 - c) * mr, c * q + (1 - c) * qr
        stats.append((m, q))
        ys.append(O.leaky(O.vbn_apply(h64[p], m, q, g64, b64, EPS), float(F32(LEAK))))
    loss = sum((ys[p] * torch.tensor(dy[p].astype(F64))).sum() for p in range(p0, P))
    loss.backward()
    coef = np.zeros((P * 8, C), F64)
    for p, (m, q) in enumerate(stats):
        m, q = m.detach().numpy(), q.detach().numpy()
        sd = 1.0 / np.sqrt(EPS + q - m * m)
        coef[p * 8:p * 8 + 5] = [m, q, sd, gamma * sd, beta - m * gamma * sd]
    _REF[key] = dict(h=h, gamma=gamma, beta=beta, dy=dy, ref_mq=ref_mq, coef=coef, y=np.stack([y.detach().numpy() for y in ys]),
                     dh=h64.grad.numpy(), dgamma=g64.grad.numpy(), dbeta=b64.grad.numpy(), c=c)
    return _REF[key]


def vbn_coef_tolerance(r, rows, B, P, ref):
    """Per-column bounds for the five coefficient rows, from the formats (u = 2^-24, one rounding = u relative).  The sums arrive
    rounded (1 u); m = sum * fl(1 / rows) is 2 more; the mix c m + (1 - c) m_ref is 4 roundings of terms bounded by
    M = |c m_batch| + |(1 - c) m_ref|: E_m = 8 u M (8: the count above with one to spare), likewise E_q.  var = eps + q - m^2 is computed
    from those: E_var = E_q + 2 |m| E_m + 3 u (eps + q + m^2).  sd = var^-1/2 turns a relative error of var into half of it, plus sqrt
    and the division: E_sd = sd (E_var / (2 var) + 3 u) -- to first order, so the bound is doubled where var is mostly cancellation.
    sc = gamma sd: E_sc = |gamma| E_sd + u |sc|.  sh = beta - m sc: E_sh = |m| E_sc + |sc| E_m + 2 u (|beta| + |m sc|)."""
    coef, c = r["coef"], r["c"]
    h64 = r["h"].astype(F64)
    out = []
    for p in range(P):
        m, q, sd, sc, sh = coef[p * 8:p * 8 + 5]
        mb, qb = np.abs(h64[p].mean(0)), (h64[p] ** 2).mean(0)
        live = ref or p > 0
        if live:
            mr, qr = (np.abs(r["ref_mq"][0]), r["ref_mq"][1]) if ref else (np.abs(h64[0].mean(0)), (h64[0] ** 2).mean(0))
            M, Q = c * mb + (1 - c) * mr, c * qb + (1 - c) * qr
        else:
            M, Q = mb, qb
        Em, Eq = 8 * U * M, 8 * U * Q
        var = 1.0 / (sd * sd)
        Evar = Eq + 2 * np.abs(m) * Em + 3 * U * (EPS + Q + m * m)
        Esd = 2 * sd * (Evar / (2 * var) + 3 * U)
        Esc = np.abs(r["gamma"]) * Esd + U * np.abs(sc)
        Esh = np.abs(m) * Esc + np.abs(sc) * Em + 2 * U * (np.abs(r["beta"]) + np.abs(m * sc))
        out += [Em, Eq, Esd, Esc, Esh]
    return np.stack(out)


def vbn_bwd_plain(r, P, p0, first_live, rows, coef32, mut=None):
    """the backward chain restated in plain fp32: S1, S2 in row order, k_vbn_bwd_coef's formulas, dh = g sc + k1 + k2 h"""
    c = F32(r["c"])
    if mut == "one_minus_c":
        c = F32(1) - c
    h, dy, gamma = r["h"][p0:], r["dy"][p0:], r["gamma"]
    np_ = P - p0
    cf = coef32.reshape(P, 8, -1)[p0:]
    side = h.astype(F64) * cf[:, 3].astype(F64)[:, None] + cf[:, 4].astype(F64)[:, None] >= 0
    g = (dy * np.where(side, F32(1), F32(LEAK)).astype(F32)).astype(F32)
    S1 = np.stack([seqsum(g[p]) for p in range(np_)])
    S2 = np.stack([seqsum(g[p] * (h[p] - cf[p, 0])) for p in range(np_)])
    k1, k2 = np.zeros_like(S1), np.zeros_like(S1)
    dg, db = np.zeros_like(S1[0]), np.zeros_like(S1[0])
    dmref, dqref = np.zeros_like(dg), np.zeros_like(dg)
    inv = F32(1.0) / F32(rows)
    for p in range(np_ - 1, -1, -1):
        mu, sd, sc = cf[p, 0], cf[p, 2], cf[p, 3]
        s3 = sd * sd * sd
        dmu, dq = -sc * S1[p] + mu * s3 * gamma * S2[p], F32(-0.5) * s3 * gamma * S2[p]
        dg, db = dg + sd * S2[p], db + S1[p]
        if p >= first_live:
            dmb, dqb = c * dmu, c * dq
            dmref, dqref = dmref + (F32(1) - c) * dmu, dqref + (F32(1) - c) * dq
        else:
            dmb, dqb = dmu + dmref, dq + dqref
        k1[p], k2[p] = dmb * inv, (F32(1) if mut == "k2" else F32(2)) * dqb * inv
    dh = g * cf[:, 3][:, None] + k1[:, None] + k2[:, None] * h
    return dh.astype(F32), dg.astype(F32), db.astype(F32)


@stops_the_module
def run_vbn(eng, C, rows, B, scen):
    sc_ = SCEN[scen]
    P, p0, ref = sc_["P"], sc_["p0"], sc_["ref"]
    r = vbn_case(C, rows, B, scen)
    case = "%s C=%d rows=%d B=%d" % (scen, C, rows, B)
    ldc = C + 4
    h64 = r["h"].astype(F64)
    # ---- coefficients from the fp64 sums rounded to fp32 (the same bits on both sides)
    sums = np.stack([v for p in range(P) for v in (h64[p].sum(0), (h64[p] ** 2).sum(0))]).astype(F32)
    D = Dev(eng)
    Sd, Gd, Bd = D.inp(sums, ld=C + 8), D.inp(r["gamma"]), D.inp(r["beta"])
    Rd = D.inp(r["ref_mq"], ld=ldc) if ref else None
    Co = D.out(P * 8, C, ld=ldc)
    (coef,) = D.run(lambda i: eng.op_segan("vbn", "coef", [Sd, Gd, Bd, Rd, D.view(Co, i)], [C, rows, P, ldc, C + 8, B], [EPS]))
    tol = vbn_coef_tolerance(r, rows, B, P, ref)
    worst = 0.0
    for p in range(P):
        got, want = coef[p * 8:p * 8 + 5], r["coef"][p * 8:p * 8 + 5]
        assert np.isfinite(got).all(), case
        ratio = np.abs(got - want) / tol[p * 5:p * 5 + 5]
        worst = max(worst, ratio.max())
        assert (coef[p * 8 + 5:p * 8 + 8] == SENT).all(), "rows 5-7 are the backward pass's"
    report("vbn_coef %s worst |err| / bound %.3f (ill-conditioned columns: bound / |sd| = %.1e, %.1e)" % (case, worst, tol[2][1] / r["coef"][2][1], tol[2][2] / r["coef"][2][2]))
    note("vbn_coef (|err| / bound)", worst)
    assert worst <= 1.0, (case, worst)
    # ---- apply from the reference's coefficients rounded to fp32; planted kinks: sh = -fl(h sc), so that h sc + sh is the rounding residue
    coef32 = np.zeros((P * 8, C), F32)
    coef32[:] = r["coef"].astype(F32)
    hk = r["h"].copy()
    nk = min(rows, 8)
    for p in range(P):
        coef32[p * 8 + 3, 3], coef32[p * 8 + 4, 3] = F32(0.5), F32(-1.0)            # column 3: exactly 0 at h = 2, one ulp on both sides
        hk[p, :nk, 3] = np.array([2.0, np.nextafter(F32(2), F32(3)), np.nextafter(F32(2), F32(1)), 2.0, 1.0, 3.0, 2.0, 2.0], F32)[:nk]
        hk[p, 0, 4] = F32(1.7)                                                      # column 4: sh = -fl(h sc): the residue decides the side
        coef32[p * 8 + 4, 4] = -(hk[p, 0, 4] * coef32[p * 8 + 3, 4])
    c64 = coef32.astype(F64).reshape(P, 8, C)
    v = hk.astype(F64) * c64[:, 3][:, None] + c64[:, 4][:, None]
    yref = np.where(v >= 0, v, F64(F32(LEAK)) * v)
    D = Dev(eng)
    Hd, Cd = D.inp(hk.reshape(P * rows, C)), D.inp(coef32, ld=ldc)
    Y = D.out(P * rows, C)
    (y,) = D.run(lambda i: eng.op_segan("vbn", "apply", [Hd, Cd, D.view(Y, i)], [C, rows, P, ldc], [LEAK]))
    e_y = ulps(y, yref.reshape(P * rows, C))
    prod = hk[:, 0, 4].astype(F64) * c64[:, 3, 4]
    assert (np.abs(v[:, 0, 4]) <= ulp32(prod)).all() and (v[:, 0, 3] == 0).all()      # the residue of one rounding; exactly 0
    # ---- backward chain on passes [p0, P): colred mode 3 -> bwd_coef -> bwd_apply, fed the same fp32 coefficients
    np_ = P - p0
    first_live = 1 if (p0 == 0 and not ref) else 0
    with_grads = scen != "G"
    acc = scen == "R"
    ginit = noise(rng(6, C), 2, C)
    dyk = r["dy"].copy()
    D = Dev(eng)
    Hd, DYd = D.inp(hk[p0:].reshape(np_ * rows, C)), D.inp(dyk[p0:].reshape(np_ * rows, C))
    Gd = D.inp(r["gamma"])
    S, scr = D.out(np_ * 2, C, ld=C + 8), D.scratch(max(4096, -(-rows // 64) * np_ * 2 * C))
    CF = D.out(np_ * 8, C, ld=ldc, init=coef32[p0 * 8:])
    DG, DB = D.out(1, C, init=ginit[0] if acc else None), D.out(1, C, init=ginit[1] if acc else None)
    DH = D.out(np_ * rows, C)

    def chain(i):
        cf = D.view(CF, i)
        eng.op_segan("colred", "vbn_bwd", [Hd, DYd, cf, D.view(S, i), scr["bufs"][i]], [C, 0, C, C, rows, np_, ldc, C + 8, 0, scr["floats"]], [LEAK])
        eng.op_segan("vbn", "bwd_coef", [D.view(S, i), Gd, cf, D.view(DG, i)[0] if with_grads else None, D.view(DB, i)[0] if with_grads else None],
                     [C, rows, np_, ldc, C + 8, B, first_live, 1 if acc else 0], [0.0])
        eng.op_segan("vbn", "bwd_apply", [Hd, DYd, cf, D.view(DH, i)], [C, rows, np_, ldc], [LEAK])
    _, cf_out, dg, db, dh = D.run(chain)
    keep = [0, 1, 2, 3, 4, 7]                              # the backward writes rows 5 and 6 only
    assert (cf_out.astype(F32).reshape(np_, 8, C)[:, keep] == coef32[p0 * 8:].reshape(np_, 8, C)[:, keep]).all(), case
    if not with_grads:
        assert (dg == SENT).all() and (db == SENT).all()
    # the fp64 reference of the chain on the planted inputs: the oracle's autograd needs the oracle's own coefficients, so the planted
    # columns 3 and 4 are compared through the formula with the reference's k1, k2 (fp64 from the fp32 coefficients) instead
    k64 = vbn_bwd_ref(hk[p0:], dyk[p0:], c64[p0:], r["gamma"], r["c"], first_live, rows)
    plain_dh, plain_dg, plain_db = vbn_bwd_plain(dict(r, h=hk, dy=dyk), P, p0, first_live, rows, coef32)
    ref_dh = k64["dh"].reshape(np_ * rows, C)
    plain_e = np.abs(plain_dh.reshape(np_ * rows, C).astype(F64) - ref_dh).max()
    reduction_rule("vbn_bwd dh", case, np.abs(dh - ref_dh).max(), plain_e, np_ * C)
    vbn_algebra_is_the_oracles(r, P, p0, first_live, rows, case)
    if with_grads:
        rg, rb = k64["dgamma"] + (ginit[0].astype(F64) if acc else 0), k64["dbeta"] + (ginit[1].astype(F64) if acc else 0)
        pg, pb = ((ginit[0] + plain_dg) if acc else plain_dg).astype(F64), ((ginit[1] + plain_db) if acc else plain_db).astype(F64)
        reduction_rule("vbn dgamma", case, np.abs(dg[0] - rg).max(), np.abs(pg - rg).max(), C)
        reduction_rule("vbn dbeta", case, np.abs(db[0] - rb).max(), np.abs(pb - rb).max(), C)
    # ---- bwd_apply alone from the reference's k1, k2 rounded to fp32: the side of the kink is k_vbn_apply's
    cfk = coef32[p0 * 8:].copy().reshape(np_, 8, C)
    cfk[:, 5], cfk[:, 6] = k64["k1"].astype(F32), k64["k2"].astype(F32)
    k = cfk.astype(F64)
    side = hk[p0:].astype(F64) * k[:, 3][:, None] + k[:, 4][:, None] >= 0
    gg = dyk[p0:].astype(F64) * np.where(side, 1.0, F64(F32(LEAK)))
    t1, t2, t3 = gg * k[:, 3][:, None], np.broadcast_to(k[:, 5][:, None], gg.shape), k[:, 6][:, None] * hk[p0:].astype(F64)
    D = Dev(eng)
    Hd, DYd, Cd = D.inp(hk[p0:].reshape(np_ * rows, C)), D.inp(dyk[p0:].reshape(np_ * rows, C)), D.inp(cfk.reshape(np_ * 8, C), ld=ldc)
    DH = D.out(np_ * rows, C)
    (dh1,) = D.run(lambda i: eng.op_segan("vbn", "bwd_apply", [Hd, DYd, Cd, D.view(DH, i)], [C, rows, np_, ldc], [LEAK]))
    scale = (np.abs(t1) + np.abs(t2) + np.abs(t3)).reshape(np_ * rows, C)
    e_dh = ulps(dh1, (t1 + t2 + t3).reshape(np_ * rows, C), scale=scale)
    # the kink: where v is the rounding residue or exactly 0, y's side (from k_vbn_apply) and the backward's must agree
    yk = y.reshape(P, rows, C)[p0:]
    for col in (3, 4):
        gk = dh1.reshape(np_, rows, C)[:, :nk, col] - (t2 + t3)[:, :nk, col]
        want = dyk[p0:, :nk, col].astype(F64) * np.where(v[p0:, :nk, col] >= 0, 1.0, LEAK) * k[:, 3, col][:, None]
        # (k1 + k2 h can dwarf g sc -- a single row has sd = eps^-1/2 -- so the comparison allows the rounding of the whole sum)
        slack = 2 * ulp32(scale.reshape(np_, rows, C)[:, :nk, col]) + 1e-6 * np.abs(want)
        assert (np.abs(gk - want) <= slack).all(), ("the backward took the other side of the kink", case, col)
        assert ((yk[:, :nk, col] >= 0) == (v[p0:, :nk, col] >= 0)).all(), ("k_vbn_apply took the other side of the kink", case, col)
    report("vbn %s apply %.2f ulp bwd_apply %.2f ulp (of the largest term)" % (case, e_y, e_dh))
    note("vbn_apply (ulp)", e_y)
    note("vbn_bwd_apply (ulp)", e_dh)
    assert e_y <= 1.0, (case, e_y)
    assert e_dh <= 1.0, (case, e_dh)


def vbn_bwd_ref(h, dy, c64, gamma, c, first_live, rows, mut=None):
    """k_vbn_bwd_coef's algebra in fp64 from fp32 inputs: the exact value the chain approximates"""
    np_, C = h.shape[0], h.shape[2]
    h, dy, gamma = h.astype(F64), dy.astype(F64), gamma.astype(F64)
    side = h * c64[:, 3][:, None] + c64[:, 4][:, None] >= 0
    g = dy * np.where(side, 1.0, F64(F32(LEAK)))
    S1, S2 = g.sum(1), (g * (h - c64[:, 0][:, None])).sum(1)
    k1, k2 = np.zeros((np_, C)), np.zeros((np_, C))
    dg = db = dmref = dqref = np.zeros(C)
    for p in range(np_ - 1, -1, -1):
        mu, sd, sc = c64[p, 0], c64[p, 2], c64[p, 3]
        dmu, dq = -sc * S1[p] + mu * sd ** 3 * gamma * S2[p], -0.5 * sd ** 3 * gamma * S2[p]
        dg, db = dg + sd * S2[p], db + S1[p]
        if p >= first_live:
            dmb, dqb, dmref, dqref = c * dmu, c * dq, dmref + (1 - c) * dmu, dqref + (1 - c) * dq
        else:
            dmb, dqb = dmu + dmref, dq + dqref
        k1[p], k2[p] = dmb / rows, 2 * dqb / rows
    return dict(dh=g * c64[:, 3][:, None] + k1[:, None] + k2[:, None] * h, k1=k1, k2=k2, dgamma=dg, dbeta=db)


def vbn_algebra_is_the_oracles(r, P, p0, first_live, rows, case):
    """k_vbn_bwd_coef's formulas (vbn_bwd_ref) from the oracle's own fp64 coefficients against the oracle's autograd: CPU against CPU, both
    in fp64, so only the algebra is compared (1e-8 on the scale max(|ref|_max, 1): fp64 rounding through the same cancellation)"""
    c64 = r["coef"].reshape(P, 8, -1)[p0:]
    k = vbn_bwd_ref(r["h"][p0:], r["dy"][p0:], c64, r["gamma"], r["c"], first_live, rows)
    for name, got, want in (("dh", k["dh"], r["dh"][p0:]), ("dgamma", k["dgamma"], r["dgamma"]), ("dbeta", k["dbeta"], r["dbeta"])):
        e = np.abs(got - want).max() / max(np.abs(want).max(), 1.0)
        assert e < 1e-8, ("the fp64 restatement of the chain disagrees with the oracle's autograd", name, case, e)


VBN_CASES = [(C, rows, B, s) for (C, rows, B) in VBN for s in ("D", "G", "R")]


@pytest.mark.parametrize("C,rows,B,scen", VBN_CASES, ids=["C%d_r%d_B%d_%s" % c for c in VBN_CASES])
def test_vbn(eng, C, rows, B, scen):
    run_vbn(eng, C, rows, B, scen)


# ---------------------------------------------------------------------------------------------------------------------------------
# the discriminator's head
# ---------------------------------------------------------------------------------------------------------------------------------
HEAD_KCR = [(5, 16, 1), (31, 48, 6), (31, 16, 6), (5, 48, 1)]
HEAD = [(Ld,) + HEAD_KCR[(i + j) % 4] for i, Ld in enumerate([1, 9, 255, 256, 257, 300]) for j in (0, 1)]


@stops_the_module
def run_head(eng, Ld, k, C, R):
    case = "Ld=%d k=%d C=%d R=%d" % (Ld, k, C, R)
    kw = pw = kb = pb_ = 0.0
    for w in range(16):                                    # 16 windows: dbfc is one sum per launch
        g = rng(7, Ld, k, C, R, w)
        h, W, wfc, bfc, dl = noise(g, R, Ld, C), noise(g, k, C), noise(g, Ld, 1), noise(g, 1), noise(g, R)
        h64 = torch.tensor(h.astype(F64), requires_grad=True)
        W64 = torch.tensor(W.astype(F64), requires_grad=True)
        f64, b64 = torch.tensor(wfc.astype(F64), requires_grad=True), torch.tensor(bfc.astype(F64), requires_grad=True)
        conv = O.conv1d_same(h64, W64[:, :, None])[..., 0]
        logits = (conv @ f64)[:, 0] + b64
        co32 = conv.detach().numpy().astype(F32)            # the backward kernels read the forward's conv_out: the same bits on both sides
        (logits * torch.tensor(dl.astype(F64))).sum().backward()
        D = Dev(eng)
        Hd, Wd, Fd, Bd = D.inp(h.reshape(R * Ld, C)), D.inp(W.reshape(k * C)), D.inp(wfc, ld=4), D.inp(bfc)
        CO, LG = D.out(R, Ld), D.out(1, R)
        co, lg = D.run(lambda i: eng.op_segan("dhead", "fwd", [Hd, Wd, Fd, Bd, D.view(CO, i), D.view(LG, i)[0]], [R, Ld, C, k, 4]))
        e_c, e_l = relerr(co, conv.detach().numpy()), relerr(lg[0], logits.detach().numpy())
        D = Dev(eng)
        DL, Hd, COd, Wd, Fd = D.inp(dl), D.inp(h.reshape(R * Ld, C)), D.inp(co32), D.inp(W.reshape(k * C)), D.inp(wfc, ld=4)
        dW, dF, dB, dH = D.out(1, k * C), D.out(Ld, 1, ld=4), D.out(1, 1), D.out(R * Ld, C)
        gw, gf, gb, gh = D.run(lambda i: eng.op_segan("dhead", "bwd", [DL, Hd, COd, Wd, Fd, D.view(dW, i)[0], D.view(dF, i), D.view(dB, i)[0], D.view(dH, i)],
                                                      [R, Ld, C, k, 4]))
        D = Dev(eng)
        DL, Hd, COd, Wd, Fd = D.inp(dl), D.inp(h.reshape(R * Ld, C)), D.inp(co32), D.inp(W.reshape(k * C)), D.inp(wfc, ld=4)
        dH2 = D.out(R * Ld, C)
        (gh2,) = D.run(lambda i: eng.op_segan("dhead", "bwd", [DL, Hd, COd, Wd, Fd, None, None, None, D.view(dH2, i)], [R, Ld, C, k, 4]))
        assert (gh2 == gh).all(), "dh with and without the parameter gradients"
        e_w, e_h = relerr(gw[0], W64.grad.numpy().reshape(k * C)), relerr(gh, h64.grad.numpy().reshape(R * Ld, C))
        for n_, e in (("dhead conv_out", e_c), ("dhead logits", e_l), ("dhead dW", e_w), ("dhead dh", e_h)):
            note(n_, e)
            assert e < TOL, (n_, case, w, e)
        # dwfc[p] = sum_r dlogit[r] conv_out[r][p] and dbfc = sum_r dlogit[r], compared in full
        rf = (dl.astype(F64)[:, None] * co32.astype(F64)).sum(0)
        assert np.abs(rf - f64.grad.numpy()[:, 0]).max() <= 1e-5 * max(np.abs(rf).max(), 1.0)
        kw, pw = max(kw, np.abs(gf[:, 0] - rf).max()), max(pw, np.abs(seqsum(dl[:, None] * co32).astype(F64) - rf).max())
        kb, pb_ = max(kb, abs(gb[0, 0] - dl.astype(F64).sum())), max(pb_, abs(float(seqsum(dl[:, None])[0]) - dl.astype(F64).sum()))
    report("dhead %s conv_out %.2e logits %.2e dW %.2e dh %.2e" % (case, e_c, e_l, e_w, e_h))
    reduction_rule("dhead dwfc", case, kw, pw, 16 * Ld)
    reduction_rule("dhead dbfc", case, kb, pb_, 16)


@pytest.mark.parametrize("Ld,k,C,R", HEAD, ids=["Ld%d_k%d_C%d_R%d" % c for c in HEAD])
def test_dhead(eng, Ld, k, C, R):
    run_head(eng, Ld, k, C, R)


# ---------------------------------------------------------------------------------------------------------------------------------
# layout and elementwise kernels, losses, optimizer
# ---------------------------------------------------------------------------------------------------------------------------------
@stops_the_module
def _pad_rows(eng, B, L, C, pf, pb):
    x = noise(rng(8, B, L, C, pf, pb), B * L, C)
    D = Dev(eng)
    X, Y = D.inp(x), D.out(B * (pf + L + pb), C)
    (y,) = D.run(lambda i: eng.op_segan("elem", "pad_rows", [X, D.view(Y, i)], [B, L, C, pf, pb]))
    ref = np.zeros((B, pf + L + pb, C), F32)
    ref[:, pf:pf + L] = x.reshape(B, L, C)
    assert (y.astype(F32) == ref.reshape(-1, C)).all()


@pytest.mark.parametrize("B,L,C,pf,pb", [(1, 1, 16, 0, 0), (3, 5, 48, 3, 0), (2, 37, 80, 0, 15), (7, 2, 16, 9, 9)])
def test_pad_rows(eng, B, L, C, pf, pb):
    _pad_rows(eng, B, L, C, pf, pb)


NAB = [1, 31, 32, 33, 80]


def prep_jobs(n):
    return [(NAB[j % 5], NAB[(j // 5 + j) % 5], j % 2, 1 + j % 3) for j in range(n)]       # (na, nb, e, ne)


@stops_the_module
def _prep(eng, njobs):
    """njobs through launch_prep_tconv_many (44 to a launch), each also through launch_prep_tconv: bit-equal to each other and to the formula"""
    jobs = prep_jobs(njobs)
    D = Dev(eng)
    Ws, outs, singles, refs, ptr_dims = [], [], [], [], [njobs]
    for j, (na, nb, e, ne) in enumerate(jobs):
        taps = 2 * (ne - 1) + e + 1
        W = noise(rng(9, j, na, nb), taps * nb, na)
        Ws.append(D.inp(W, ld=na + 3))
        outs.append(D.out(ne * na, nb, ld=nb + 5))
        singles.append(D.out(ne * na, nb, ld=nb + 5))
        ref = np.zeros((ne, na, nb), F32)
        for rr in range(ne):
            ref[rr] = W.reshape(taps, nb, na)[2 * (ne - 1 - rr) + e].T
        refs.append(ref.reshape(ne * na, nb))
        ptr_dims += [na + 3, nb, na, e, ne, nb + 5]

    def launch(i):
        eng.op_segan("elem", "prep_tconv_many", [t for j in range(njobs) for t in (Ws[j], D.view(outs[j], i))], ptr_dims)
        for j, (na, nb, e, ne) in enumerate(jobs):
            eng.op_segan("elem", "prep_tconv", [Ws[j], D.view(singles[j], i)], [1, na + 3, nb, na, e, ne, nb + 5])
    res = D.run(launch)
    for j in range(njobs):
        assert (res[2 * j].astype(F32) == refs[j]).all() and (res[2 * j + 1].astype(F32) == refs[j]).all(), (j, jobs[j])


@pytest.mark.parametrize("njobs", [44, 45])
def test_prep_tconv(eng, njobs):
    _prep(eng, njobs)


@stops_the_module
def _interleave(eng, pl, Lt, bias):
    B, C = 3, 16
    i0 = [(e - pl) % 2 for e in (0, 1)]
    Q = [max((Lt - i0[e] + 1) // 2, 0) if Lt > i0[e] else 0 for e in (0, 1)]
    g = rng(10, pl, Lt, bias)
    Ts = [noise(g, B * max(Q[e], 1), C) for e in (0, 1)]
    bv = noise(g, C)
    D = Dev(eng)
    T0, T1, Bd = D.inp(Ts[0]), D.inp(Ts[1]), (D.inp(bv) if bias else None)
    T = D.out(B * Lt, C)
    (t,) = D.run(lambda i: eng.op_segan("elem", "interleave", [T0, T1, Bd, D.view(T, i)], [max(Q[0], 1), max(Q[1], 1), i0[0], i0[1], pl, B, Lt, C]))
    ref = np.zeros((B, Lt, C), F64)
    for p in range(Lt):
        e = (p + pl) & 1
        ref[:, p] = Ts[e].reshape(B, max(Q[e], 1), C)[:, (p - i0[e]) >> 1].astype(F64) + (bv.astype(F64) if bias else 0.0)
    if bias:
        assert ulps(t, ref.reshape(B * Lt, C)) <= 1.0
    else:
        assert (t == ref.reshape(B * Lt, C)).all()


@pytest.mark.parametrize("pl,Lt,bias", [(pl, Lt, b) for pl in (4, 9) for Lt in (1, 6, 7) for b in (False, True)])
def test_interleave(eng, pl, Lt, bias):
    _interleave(eng, pl, Lt, bias)


def act_ref(z, alpha, leak):
    z = z.astype(F64)
    if alpha is not None:
        return np.maximum(z, 0) + alpha.astype(F64) * (z - np.abs(z)) * 0.5
    return np.maximum(z, F64(F32(leak)) * z)


def act_grad(z, alpha, leak, prelu_at_zero=0.5):
    """1 above 0, the slope below; exactly at 0 (either sign): PReLU a / 2 (d|x|/dx = 0 in TensorFlow), leaky 1 (tf.maximum's tie)"""
    z = z.astype(F64)
    a = np.broadcast_to(alpha.astype(F64), z.shape) if alpha is not None else np.full(z.shape, F64(F32(leak)))
    at0 = prelu_at_zero * a if alpha is not None else np.ones(z.shape)
    return np.where(z > 0, 1.0, np.where(z < 0, a, at0))


@stops_the_module
def _act(eng, rows, C, prelu):
    g = rng(11, rows, C, prelu)
    z = noise(g, rows, C)
    z[0, :8] = np.array([0.0, -0.0, 1e-30, -1e-30, 0.0, -0.0, 1e-30, -1e-30], F32)
    z[rows - 1, C - 4:] = np.array([0.0, -0.0, 1e-30, -1e-30], F32)
    alpha = (g.uniform(0.1, 0.9, C) * np.where(g.random(C) < 0.3, -1, 1)).astype(F32) if prelu else None
    dy, extra = noise(g, rows, C) + F32(0.5), noise(g, rows, C)
    ldo, coff = 2 * C + 4, C
    D = Dev(eng)
    Z, A = D.inp(z), (D.inp(alpha) if prelu else None)
    Y = D.out(rows, C, ld=ldo, col0=coff)
    (y,) = D.run(lambda i: eng.op_segan("elem", "act_fwd", [Z, A, D.view(Y, i)], [C, ldo, coff, rows], [LEAK]))
    e_f = ulps(y, act_ref(z, alpha, LEAK))
    res = []
    for ex in (None, extra):
        D = Dev(eng)
        DY = D.inp(np.concatenate([np.full((rows, coff), NAN, F32), dy], 1), ld=ldo)
        Z, A, E = D.inp(z), (D.inp(alpha) if prelu else None), (D.inp(ex) if ex is not None else None)
        DZ = D.out(rows, C)
        (dz,) = D.run(lambda i: eng.op_segan("elem", "act_bwd", [DY, Z, A, E, D.view(DZ, i)], [ldo, coff, C, rows], [LEAK]))
        t = dy.astype(F64) * act_grad(z, alpha, LEAK)
        res.append(ulps(dz, t + (ex.astype(F64) if ex is not None else 0.0), scale=np.abs(t)))
        zero = z == 0
        want0 = (dy.astype(F64) * (0.5 * alpha.astype(F64) if prelu else 1.0))[zero] + (ex.astype(F64)[zero] if ex is not None else 0.0)
        assert np.abs(dz[zero] - want0).max() <= 1e-6 * max(np.abs(want0).max(), 1.0), "the slope exactly at 0"
    report("act rows=%d C=%d prelu=%d fwd %.2f ulp bwd %.2f / %.2f ulp" % (rows, C, prelu, e_f, res[0], res[1]))
    note("act_fwd (ulp)", e_f)
    note("act_bwd (ulp)", max(res))
    assert e_f <= 1.0 and max(res) <= 1.0


@pytest.mark.parametrize("rows,C,prelu", [(3, 16, True), (3, 16, False), (700, 48, True), (257, 80, False)])
def test_activations(eng, rows, C, prelu):
    _act(eng, rows, C, prelu)


@stops_the_module
def _copy_cols(eng, rows, C, acc):
    g = rng(12, rows, C, acc)
    src, init = noise(g, rows, C), noise(g, rows, C)
    lds, soff, ldd, doff = 2 * C + 3, C + 1, 3 * C, C
    D = Dev(eng)
    S = D.inp(np.concatenate([np.full((rows, soff), NAN, F32), src], 1), ld=lds)
    O_ = D.out(rows, C, ld=ldd, col0=doff, init=init if acc else None)
    (o,) = D.run(lambda i: eng.op_segan("elem", "copy_cols", [S, D.view(O_, i)], [lds, soff, ldd, doff, C, rows, 1 if acc else 0]))
    if acc:
        assert ulps(o, init.astype(F64) + src.astype(F64), scale=np.maximum(np.abs(init), np.abs(src))) <= 1.0
    else:
        assert (o.astype(F32) == src).all()


@pytest.mark.parametrize("rows,C,acc", [(1, 1, False), (37, 5, True), (700, 48, False), (700, 48, True)])
def test_copy_cols(eng, rows, C, acc):
    _copy_cols(eng, rows, C, acc)


@stops_the_module
def _joint(eng, B, Lx, U_, with_noise):
    g = rng(13, B, Lx, U_)
    x, tail, nz = noise(g, B, Lx), noise(g, B, U_), noise(g, B, Lx + U_)
    D = Dev(eng)
    X, T, N = D.inp(x), D.inp(tail), (D.inp(nz) if with_noise else None)
    J = D.out(B, Lx + U_)
    (j,) = D.run(lambda i: eng.op_segan("elem", "build_joint1", [X, T, N, D.view(J, i)], [Lx, U_, B]))
    cat = np.concatenate([x, tail], 1)
    if with_noise:
        assert ulps(j, cat.astype(F64) + nz.astype(F64), scale=np.maximum(np.abs(cat), np.abs(nz))) <= 1.0
    else:
        assert (j.astype(F32) == cat).all()


@pytest.mark.parametrize("B,Lx,U_,with_noise", [(1, 1, 1, False), (3, 37, 5, True), (2, 2827, 40, False), (2, 300, 40, True)])
def test_build_joint1(eng, B, Lx, U_, with_noise):
    _joint(eng, B, Lx, U_, with_noise)


@stops_the_module
def _sum_all(eng, rows, cols):
    ke = pe = 0.0
    for w in range(16):
        x = noise(rng(14, rows, cols, w), rows, cols) + F32(0.1)
        D = Dev(eng)
        X, Out, scr = D.inp(x, ld=cols + 3), D.out(1, 1), D.scratch(256)
        (o,) = D.run(lambda i: eng.op_segan("elem", "sum_all", [X, D.view(Out, i)[0], scr["bufs"][i]], [rows, cols, cols + 3]))
        ref = x.astype(F64).sum()
        ke, pe = max(ke, abs(o[0, 0] - ref)), max(pe, abs(float(seqsum(x.reshape(-1, 1))[0]) - ref))
    reduction_rule("sum_all", "rows=%d cols=%d" % (rows, cols), ke, pe, 16)


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 37), (32, 2827)])
def test_sum_all(eng, rows, cols):
    _sum_all(eng, rows, cols)


@stops_the_module
def _lsgan(eng, mode, P, B):
    fake = P - 1
    ke = pe = ud = 0.0
    for w in range(16):
        lg = noise(rng(15, mode, P, B, w), P, B) + F32(0.5)
        D = Dev(eng)
        L_ = D.inp(lg.reshape(P * B))
        DL, L3 = D.out(1, P * B), D.out(1, 3 if mode == 0 else 1, ld=3)
        dl, l3 = D.run(lambda i: eng.op_segan("elem", "lsgan", [L_, D.view(DL, i)[0], D.view(L3, i)[0]], [B, mode, fake, P]))
        l64, l32 = lg.astype(F64), lg
        dref = np.zeros((P, B))
        if mode == 0:
            rl = ((l64[1] - 1) ** 2).mean() if P > 1 else 0.0
            fk = (l64[2] ** 2).mean() if P > 2 else 0.0
            ref = np.array([rl, fk, rl + fk])
            e1 = (l32[1] - F32(1)) if P > 1 else np.zeros(1, F32)
            e2 = l32[2] if P > 2 else np.zeros(1, F32)
            p1, p2 = seqsum((e1 * e1)[:, None])[0] / F32(B), seqsum((e2 * e2)[:, None])[0] / F32(B)
            plain = np.array([p1, p2, F32(p1 + p2)], F64)
            if P > 1:
                dref[1] = 2 * (l64[1] - 1) / B
            if P > 2:
                dref[2] = 2 * l64[2] / B
        else:
            ref = np.array([((l64[fake] - 1) ** 2).mean()])
            e1 = l32[fake] - F32(1)
            plain = np.array([seqsum((e1 * e1)[:, None])[0] / F32(B)], F64)
            dref[fake] = 2 * (l64[fake] - 1) / B
        ke, pe = max(ke, np.abs(l3[0] - ref).max()), max(pe, np.abs(plain - ref).max())
        ud = max(ud, ulps(dl[0], dref.reshape(P * B)))
    note("lsgan dlogits (ulp)", ud)
    assert ud <= 1.0, ud
    reduction_rule("lsgan loss", "mode=%d P=%d B=%d" % (mode, P, B), ke, pe, 16)


@pytest.mark.parametrize("mode,P,B", [(m, P, B) for m in (0, 1) for (P, B) in ((2, 1), (2, 128), (3, 100))])
def test_lsgan(eng, mode, P, B):
    _lsgan(eng, mode, P, B)


@stops_the_module
def _l1(eng, n, acc):
    ke = pe = ud = 0.0
    for w in range(16):
        g = rng(16, n, acc, w)
        G, lab, init = noise(g, n), noise(g, n), noise(g, n)
        lab[::3] = G[::3]                                   # G == labels: sign 0
        lam, adv = F32(100.0), F32(0.37)
        D = Dev(eng)
        Gd, Ld_, Lm = D.inp(G), D.inp(lab), D.inp(np.array([lam], F32))
        dG, L3 = D.out(1, n, init=init if acc else None), D.out(1, 2, ld=3, col0=1, init=None)
        L3["cpu0"][GUARD, 0] = float(adv)
        L3["bufs"] = [L3["cpu0"].to(eng.device), L3["cpu0"].to(eng.device)]
        dg, l3 = D.run(lambda i: eng.op_segan("elem", "l1", [Gd, Ld_, Lm, D.view(dG, i)[0], D.view(L3, i)[0]], [n, 1 if acc else 0]))
        e64 = G.astype(F64) - lab.astype(F64)
        l1 = 100.0 * np.abs(e64).mean()
        ref = np.array([l1, float(adv) + l1])
        p1 = F32(lam * seqsum(np.abs(G - lab)[:, None])[0]) / F32(n)
        plain = np.array([p1, F32(adv + p1)], F64)
        ke, pe = max(ke, np.abs(l3[0] - ref).max()), max(pe, np.abs(plain - ref).max())
        d = 100.0 * np.sign(e64) / n
        ud = max(ud, ulps(dg[0], d + (init.astype(F64) if acc else 0.0), scale=np.maximum(np.abs(d), np.abs(init) if acc else 0.0)))
        assert (dg[0][::3] == (init[::3] if acc else 0.0)).all(), "sign(0) = 0"
    note("l1 dG (ulp)", ud)
    assert ud <= 1.0, ud
    reduction_rule("l1 loss", "n=%d acc=%d" % (n, acc), ke, pe, 32)


@pytest.mark.parametrize("n,acc", [(1, False), (255, True), (257, False), (5000, True)])
def test_l1(eng, n, acc):
    _l1(eng, n, acc)


@stops_the_module
def _rmsprop(eng, n):
    g = rng(17, n)
    w, gr, ms = noise(g, n), noise(g, n) * F32(0.1), g.uniform(0.5, 2.0, n).astype(F32)
    gr[:4] = 0
    lr, decay, eps = F32(1e-3), F32(0.9), F32(1e-10)
    D = Dev(eng)
    Gd, Lr = D.inp(gr), D.inp(np.array([lr], F32))
    Wd, Md = D.out(1, n, init=w), D.out(1, n, init=ms)
    wn, mn = D.run(lambda i: eng.op_segan("elem", "rmsprop", [D.view(Wd, i)[0], Gd, D.view(Md, i)[0], Lr], [n], [decay, eps]))
    d64, om = F64(decay), F64(F32(1) - decay)
    m = d64 * ms.astype(F64) + om * gr.astype(F64) ** 2
    # w from the fp64 ms, not from the kernel's: the step lr g / sqrt(ms + eps) carries ms's ulp halved by the root, the root, the quotient
    # and the product (4 u of the step, u = 2^-24), and the difference is rounded once (1 ulp of the larger of |w| and the step)
    step = F64(lr) * gr.astype(F64) / np.sqrt(m + F64(eps))
    wref = w.astype(F64) - step
    e_m = ulps(mn[0], m)
    slack = ulp32(np.maximum(np.abs(w), np.abs(step))) + 4 * U * np.abs(step)
    e_w = float((np.abs(wn[0] - wref.astype(F32).astype(F64)) / slack).max())
    report("rmsprop n=%d ms %.2f ulp w %.2f of its bound" % (n, e_m, e_w))
    note("rmsprop ms (ulp)", e_m)
    note("rmsprop w (|err| / bound)", e_w)
    assert e_m <= 1.0 and e_w <= 1.0, (e_m, e_w)


@pytest.mark.parametrize("n", [1, 257, 70000])
def test_rmsprop(eng, n):
    _rmsprop(eng, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# mutations (CPU): each mistake must break the bound its output is held to
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mutations_exceed_the_bound():
    ratios, misses = {}, {}

    def rec(name, shape, err, bound):
        r = err / bound if bound > 0 else (math.inf if err > 0 else 0.0)
        ratios[name] = min(ratios.get(name, math.inf), r) if r > 1 else ratios.get(name, math.inf)
        if r <= 1:
            misses.setdefault(name, []).append(shape)

    for (L, k, Cin, Cout, Bn, bias) in CONV2:
        d = conv2_data(L, k, Cin, Cout, Bn)
        Lo, pl = (L + 1) // 2, max(((L + 1) // 2 - 1) * 2 + k - L, 0) // 2
        z, dx = d["z"], d["dx"]
        scale_z, scale_x = max(np.abs(z).max(), 1.0), max(np.abs(dx).max(), 1.0)
        W = d["W"].astype(F64)[:, 0]
        x = d["x"].astype(F64)
        shape = (L, k)
        # a tap dropped at the first / last output position: the first tap that falls inside the input there
        for name, o in (("tap dropped at the first output", 0), ("tap dropped at the last output", Lo - 1)):
            taps = [dk for dk in range(k) if 0 <= 2 * o + dk - pl < L]
            contrib = x[:, 2 * o + taps[0] - pl] @ W[taps[0]]
            rec(name, shape, np.abs(contrib).max() / scale_z, TOL)
        # pl off by one: the forward of the input moved by one position
        xs = np.zeros_like(x)
        xs[:, 1:] = x[:, :-1]
        zs = O.downconv(torch.tensor(xs), torch.tensor(d["W"].astype(F64)), None).numpy()
        rec("pl off by one", shape, np.abs(zs - z).max() / scale_z, TOL)
        # the transposed convolution: classes swapped = neighbours exchanged; i0 off by two = a class moved by one of its own positions
        sw = dx.copy()
        n2 = L // 2 * 2
        sw[:, 0:n2:2], sw[:, 1:n2:2] = dx[:, 1:n2:2], dx[:, 0:n2:2]
        rec("parity classes swapped", shape, np.abs(sw - dx).max() / scale_x, TOL)
        sh = dx.copy()
        if L > 2:
            sh[:, 0:L - 2:2] = dx[:, 2:L:2]
        rec("i0 off by two", shape, np.abs(sh - dx).max() / scale_x, TOL)
    # the last row of a chunk lost, in the reductions: the bound is 4 x the plain error
    for (L, k, C, B, small) in CONV1:
        if L > 2100:
            continue
        d = conv1_data(L, k, C, B)
        plain = conv1_wgrad_plain(d["x"], d["dz"], k).astype(F64)
        lost = conv1_wgrad_plain(d["x"], d["dz"], k, drop_last_row_of_chunk=min(512, (L + 1) // 2)).astype(F64)
        rec("last row of a chunk lost (conv1 wgrad)", (L, k, C), np.abs(lost - d["dW"]).max(), 4 * np.abs(plain - d["dW"]).max())
    for (C, rows, P, coff, acc, scratch) in COLRED[:33]:
        r = colred_refs(C, rows, P, 0)
        a3 = r["a"].reshape(P, rows, C)
        lost = np.stack([seqsum(a3[p][:-1]) if rows > 1 else np.zeros(C, F32) for p in range(P)]).astype(F64)
        rec("last row of a chunk lost (colred)", (C, rows, P), np.abs(lost - r["ref"][0][0]).max(), 4 * np.abs(r["plain"][0][0] - r["ref"][0][0]).max())
    # VBN: (1 - c) for c in the mix, k2 without its factor 2 (the backward chain; B = 1 has c = 1 - c)
    for (C, rows, B) in VBN:
        for scen in ("D", "R"):
            sc_ = SCEN[scen]
            r = vbn_case(C, rows, B, scen)
            coef32 = r["coef"].astype(F32)
            first_live = 0 if sc_["ref"] else 1
            c64 = coef32.astype(F64).reshape(sc_["P"], 8, C)
            ref = vbn_bwd_ref(r["h"], r["dy"], c64, r["gamma"], r["c"], first_live, rows)["dh"]
            plain = vbn_bwd_plain(r, sc_["P"], 0, first_live, rows, coef32)[0].astype(F64)
            for mut, name in (("one_minus_c", "(1 - c) for c"), ("k2", "k2 without its factor 2")):
                m = vbn_bwd_plain(r, sc_["P"], 0, first_live, rows, coef32, mut=mut)[0].astype(F64)
                if mut == "one_minus_c" and B == 1:
                    assert (m == plain).all()
                    continue
                rec(name, (C, rows, B, scen), np.abs(m - ref).max(), 4 * np.abs(plain - ref).max())
    # PReLU's slope at 0 taken as a: the planted zeros of the activation cases
    z = np.array([[0.0, -0.0, 1.0, -1.0]], F32)
    alpha, dy = np.array([0.25, 0.5, 0.25, 0.5], F32), np.ones((1, 4), F32)
    good, bad = dy * act_grad(z, alpha, LEAK), dy * act_grad(z, alpha, LEAK, prelu_at_zero=1.0)
    rec("PReLU's slope at 0 taken as a", "planted zeros", float((np.abs(bad - good) / ulp32(good)).max()), 1.0)
    for name in sorted(set(ratios) | set(misses)):
        print("segan_ops mutation %-42s smallest separating ratio %.3g; not separated at %s" % (name, ratios.get(name, math.nan), misses.get(name, "no shape")))
    # every mistake separates at every shape where it changes the result at all, except the ones listed (and explained) here
    allowed = {
        # one input position, one output position: moving the input by one leaves only zeros in reach of some taps, and with k = 2 or 3
        # at L <= 2 the moved forward can coincide; a class of a one- or two-position output has nothing to exchange or move
        "pl off by one": lambda s: s[0] == 1,
        "parity classes swapped": lambda s: s[0] == 1,
        "i0 off by two": lambda s: s[0] <= 2,
        # a single row per pass: nothing is left to lose but the whole sum, which still separates unless the plain error is 0 too
        "last row of a chunk lost (colred)": lambda s: False,
        "last row of a chunk lost (conv1 wgrad)": lambda s: False,
    }
    for name, shapes in misses.items():
        bad_ = [s for s in shapes if not allowed.get(name, lambda s: False)(s)]
        assert not bad_, (name, "does not separate at", bad_)
    assert all(math.isfinite(v) and v > 1 for v in ratios.values()), ratios


# ---------------------------------------------------------------------------------------------------------------------------------
# The ledger, from reading launch_colred: the form is the mode's bit of RSRGAN_COLRED_VEC where C, lda, coff, ldb, ldcoef are multiples of
# 4 (the table has such C and others), so both forms of every mode occur across the default (bits 0, 1, 3) and the two children (none,
# all).  The chunk doubles (a) on the 16-byte form at rows_per = 20000 (313 chunks of 64 > 256), (b) on either form when the scratch is
# below the default chunk's need ("min", "below": C = 5, 16, 48, 255 with P = 1 and P > 1); never on the scalar form by size alone
# (20000 / 256 = 79 <= 128).  P = 1 and P > 1 occur with every one of these.
# ---------------------------------------------------------------------------------------------------------------------------------
LEDGER = {(mode, vec, doubled, pgt) for mode in range(4) for vec in (0, 1) for doubled in (False, True) for pgt in (False, True)}


def test_zz_ledger(request):
    """prints what the passing cases asserted and compares the column-reduction combinations with the hand-written ledger; only a run
    that names its tests (-k, --deselect, a node id) is excused, so a case added or dropped later cannot switch the comparison off"""
    for k_, v in sorted(WORST.items()):
        print("segan_ops worst %-28s %.3e" % (k_, v))
    for c in sorted(COVERED):
        print("segan_ops covered %s" % (c,))
    opt = request.config.option
    if opt.keyword or getattr(opt, "deselect", None) or any("::" in a for a in request.config.args):
        print("segan_ops partial run (-k, --deselect or a node id): the ledger is not compared")
        return
    assert LEDGER - COVERED == set(), ("combinations no passing case reached", sorted(LEDGER - COVERED))
    assert COVERED - LEDGER == set(), sorted(COVERED - LEDGER)
