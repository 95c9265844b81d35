"""csrc/bn.hip kernel by kernel: the three forward / backward routes of batch_norm(renorm=True) (small: k_bn_fwd_small / k_bn_bwd_small;
sliced: k_bn_stats1/2 + k_bn_apply, k_bn_bwd1/2/3; narrow: k_bn_part_narrow + k_bn_elem_narrow), k_bn_infer_coef and the state update
(k_bn_commit_many, k_bn_commit), each through the host launch function the model calls (rsrgan_op_bn_forward / _backward / _commit)
against oracle/bn_renorm.py in fp64 on the CPU, from the same fp32-rounded inputs.  Every case asserts its numbers first and the
route that ran (rsrgan_op_bn_last_plan) second, so a plan failure says the arithmetic was right.

Case construction.  The layer starts from a random NON-initial state (renorm_mean / renorm_stddev random, the two weights in
(0.2, 0.9), gamma signed and non-unit, beta nonzero, moving_* random): r is far from 1 and d far from 0 (each case prints their
ranges), so the d.sum(dy') term of dgamma, the factor r of a, the d.gamma part of b and the mixed mean / stddev all carry weight.
dy has mean 0.5.  The backward pass is tested on its own: its y and stat inputs are the fp64 reference rounded to fp32, so the
ReLU mask [y > 0] is the same bits for the kernel, the restatement and the reference (dy' = dy.[y_ref > 0]); +0.0 and -0.0 are
planted into y at places where dy != 0.  With relu = false, y is a NaN-filled buffer: it must not be read.

Guards.  Operand columns [cols, pad4(cols)) are zero (the kernels' contract; the same columns of stat are zero and never written),
the columns beyond and GUARD rows on both sides of every operand are NaN; y, stat (one statistics slot more than the calls),
dbeta / dgamma are sentinel-filled and everything outside the valid extent must come back bit-unchanged (for training = false: stat
rows 0-3 too); scratch is NaN up to its size with a sentinel band behind it; sums holds a FINITE sentinel (its padding columns are
never written and are multiplied by a = 0: 0 x NaN would be NaN -- the contract of include/rsrgan.h); padding columns of y and dz
on the sliced and narrow routes must be 0; every launch runs twice and must be bit-identical.

Bound (DESIGN 6l's rule for reductions).  For every output (y, the six stat rows, dz, dbeta, dgamma):
    max over the output of (|kernel - ref| - 4 ulp32(max |ref| of the column))  <=  4 x max |plain - ref|
where `plain` is a plain fp32 restatement of the same algorithm on the CPU: the first-row shift, sums in fp32 in plain row order,
the moments and corrections finished in fp64, a and b rounded once to fp32, z.a + b in fp32 (multiply, then add).  The 4 ulp cover
the one multiply-add whose contraction the compiler decides (0.5 ulp of the product, which is up to the column's magnitude) and the
single roundings of a and b (0.5 ulp each, times |z| and 1) -- three half-ulps of quantities bounded by the column's max, rounded up.
Both sides are maxima over at least 16 columns (narrower shapes run 16 / cols windows with fresh data).  On the outlier columns the
restatement loses accuracy too: both figures are printed and only "worse than 4 x plain fp32" fails.  The project's scale
max |err| / max(|ref|_max, 1) is printed with them.  State update: the kernel computes in double and rounds once, |err| <= 2^-23 |ref|.

test_mutations_exceed_the_bound (CPU) applies six mistakes to the restatement and requires each to break that bound.

One fresh child process runs RSRGAN_BN_NARROW=1 RSRGAN_BN_SMALL_ROWS=0 (the narrow form at few rows, the sliced route at small-route
shapes).  COVERED collects (route, direction, calls > 1, training, relu) of every passing launch; test_zz_ledger compares it with
LEDGER, written by hand from the tables below."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import bn_renorm as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 7.0
GUARD = 3                      # guard rows before and behind every matrix
BAND = 4096                    # sentinel floats behind scratch
F32, F64 = np.float32, np.float64
EPS32 = float(F32(1e-3))       # BN_EPS of bn.hip is a float constant
SCOPE = "t"
PRE = SCOPE + "/BatchNorm/"
VARS = ("beta", "gamma", "moving_mean", "moving_variance", "renorm_mean", "renorm_mean_weight", "renorm_stddev", "renorm_stddev_weight")
COVERED = set()                # (route, "fwd" | "bwd", calls > 1, training, relu)
LINES = []                     # one report line per launch pair
WORST = {}                     # output -> (largest kernel error on the project's scale, largest excess / bound)
_FAULTED = []                  # a launch that raised (a HIP error, not a failed assertion): nothing more is started on the GPU


def pad4(n):
    return (n + 3) // 4 * 4


def model_scratch(cols):
    """Model::scratch_floats for a batch-norm layer"""
    return max(4 * 64 * cols, 16384)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs, the fp64 reference and the plain fp32 restatement (all CPU, numpy)
# ---------------------------------------------------------------------------------------------------------------------------------
def make_state(cols, seed):
    g = np.random.default_rng([11, cols, seed])
    sign = np.where(g.random(cols) < 0.5, -1.0, 1.0)
    st = dict(beta=g.normal(0, 1, cols), gamma=sign * g.uniform(0.5, 2.0, cols), moving_mean=g.normal(0, 1, cols),
              moving_variance=g.uniform(0.2, 2.0, cols), renorm_mean=g.normal(0, 0.5, cols), renorm_mean_weight=g.uniform(0.2, 0.9, 1),
              renorm_stddev=g.uniform(0.3, 1.5, cols), renorm_stddev_weight=g.uniform(0.2, 0.9, 1))
    return {k: v.astype(F32) for k, v in st.items()}


def oracle_params(st):
    return {PRE + k: (F64(v[0]) if k.endswith("weight") else v.astype(F64)) for k, v in st.items()}


EDGE_COLS = 6                  # columns 0..5 of an `edges` case: constant, 1000 + 1e-2 noise, 6-sigma and 50-sigma first row, all y < 0, plain


def make_inputs(rows, cols, calls, seed, edges=False):
    g = np.random.default_rng([13, rows, cols, calls, seed])
    scale, shift = g.uniform(0.5, 2.0, cols), g.normal(0, 2.0, cols)
    z = g.standard_normal((calls, rows, cols), dtype=F32) * scale.astype(F32) + shift.astype(F32)
    z += (0.3 * np.arange(calls)).astype(F32)[:, None, None]
    if edges:
        assert cols >= 16 and rows >= 16
        z[:, :, 0] = 3.25
        z[:, :, 1] = 1000.0 + 1e-2 * g.normal(0, 1, (calls, rows))
        z[:, 0, 2] = shift[2] + 6.0 * scale[2]
        z[:, 0, 3] = shift[3] + 50.0 * scale[3]
    dy = g.standard_normal((calls, rows, cols), dtype=F32) + F32(0.5)
    return z, dy


SEQSUM_REDUCE_FROM = 1 << 22


def seqsum(x, force_cumsum=False):
    """fp32 column sums in plain row order.  From 4 Mi elements on, numpy's reduction over axis 0 of a C-ordered [rows][cols >= 64] matrix,
    which adds row after row into the accumulator row (pairwise summation is used along a contiguous axis only): the same order at a
    tenth of the time.  test_mutations_exceed_the_bound compares the two bit for bit, so a numpy that sums differently fails there."""
    assert x.dtype == F32 and x.ndim == 2
    if x.size >= SEQSUM_REDUCE_FROM and x.shape[1] >= 64 and x.flags.c_contiguous and not force_cumsum:
        return np.add.reduce(x, axis=0, dtype=F32)
    return np.cumsum(x, axis=0, dtype=F32)[-1]


def finish_forward(z0, s1, s2, n, st, swap=False):
    """the moments, corrections and the affine from the shifted fp32 sums, in fp64 (k_bn_stats2); rows mean, stddev, r, d, a, b"""
    m0 = s1.astype(F64) / n
    var = np.maximum(s2.astype(F64) / n - m0 * m0, 0.0)
    mean = z0.astype(F64) + m0
    sd = np.sqrt(var + EPS32)
    wm, ws = F64(st["renorm_mean_weight"][0]), F64(st["renorm_stddev_weight"][0])
    if swap:
        wm, ws = ws, wm
    mixed_mean = st["renorm_mean"].astype(F64) + (1.0 - wm) * mean
    mixed_sd = st["renorm_stddev"].astype(F64) + (1.0 - ws) * sd
    r, d = sd / mixed_sd, (mean - mixed_mean) / mixed_sd
    gam = st["gamma"].astype(F64)
    a = r * gam / sd
    return np.stack([mean, sd, r, d, a, d * gam + st["beta"].astype(F64) - mean * a])


def plain_forward(z, st, training=True, relu=True, mut=None):
    """z [rows][cols] fp32 -> (stat [6][cols] fp32, y fp32).  mut: a mistake of test_mutations_exceed_the_bound"""
    n = z.shape[0]
    if training:
        zz = z[:-1] if mut == "lastrow" else z
        if mut == "unshifted":
            z0 = np.zeros_like(z[0])
        else:
            z0 = z[0]
        v = zz - z0
        stat = finish_forward(z0, seqsum(v), seqsum(v * v), n - 1 if mut == "nm1" else n, st, swap=mut == "swap").astype(F32)
    else:
        a = st["gamma"].astype(F64) / np.sqrt(st["moving_variance"].astype(F64) + EPS32)
        stat = np.zeros((6, z.shape[1]), F32)
        stat[4], stat[5] = a.astype(F32), (st["beta"].astype(F64) - st["moving_mean"].astype(F64) * a).astype(F32)
    y = z * stat[4] + stat[5]
    return stat, (np.maximum(y, F32(0)) if relu else y)


def plain_backward(dy, yin, z, stat, relu=True, mut=None):
    """-> (dz fp32, dbeta fp64, dgamma fp64) of one call, from the fp32 stat rows as the kernels read them"""
    n = z.shape[0]
    mean, isd, a = stat[0], F32(1) / stat[1], stat[4]
    g = np.where(yin > 0, dy, F32(0)) if relu else dy
    gs = dy if mut == "nomask" else g                     # (the mask left out of the partial sums only)
    xh = (z - mean) * isd
    cut = slice(0, n - 1) if mut == "lastrow" else slice(0, n)
    s1, s2 = seqsum(gs[cut]).astype(F64), seqsum(gs[cut] * xh[cut]).astype(F64)
    gb = s1
    gg = stat[2].astype(F64) * s2 + (0.0 if mut == "dterm" else stat[3].astype(F64) * s1)
    m1, m2 = (s1 / n).astype(F32), (s2 / n).astype(F32)
    return a * (g - m1 - xh * m2), gb, gg


def reference(rows, cols, calls, seed, training, relu, edges, acc_init):
    """everything one window of a case needs: the inputs, the fp64 reference and the restatement.  Nothing here is modified later."""
    st = make_state(cols, seed)
    if edges:
        st["beta"][4] = F32(-100.0)                       # column 4: every pre-activation negative
    z, dy = make_inputs(rows, cols, calls, seed, edges)
    P = oracle_params(st)
    out = dict(st=st, z=z, dy=dy, calls=[])
    gb_ref = np.zeros(cols) + (acc_init[0].astype(F64) if acc_init else 0.0)
    gg_ref = np.zeros(cols) + (acc_init[1].astype(F64) if acc_init else 0.0)
    gb_pl, gg_pl = gb_ref.copy(), gg_ref.copy()
    g = np.random.default_rng([17, rows, cols, seed])
    for k in range(calls):
        zk = z[k].astype(F64)
        c = dict()
        if training:
            y, cache = O.forward_train(P, SCOPE, zk)
            a = cache["r"] * P[PRE + "gamma"] / cache["std"]
            c["stat"] = np.stack([cache["mean"], cache["std"], cache["r"], cache["d"], a,
                                  cache["d"] * P[PRE + "gamma"] + P[PRE + "beta"] - cache["mean"] * a])
            c["r"], c["d"] = cache["r"], cache["d"]
        else:
            y = O.forward_infer(P, SCOPE, zk)
            a = P[PRE + "gamma"] / np.sqrt(P[PRE + "moving_variance"] + O.EPS)
            c["stat"] = np.stack([a, P[PRE + "beta"] - P[PRE + "moving_mean"] * a])      # rows 4, 5
        c["y"] = np.maximum(y, 0.0) if relu else y
        c["stat_pl"], c["y_pl"] = plain_forward(z[k], st, training, relu)
        if training:
            if edges and relu:
                assert (y[:, 4] < 0).all()
            yin = c["y"].astype(F32)                      # the backward pass reads the reference's y, rounded
            if relu:                                       # +0.0 and -0.0 where dy != 0
                rr, cc = g.integers(0, rows, 24), g.integers(min(EDGE_COLS, cols - 1), cols, 24)
                yin[rr[:12], cc[:12]] = F32(0.0)
                yin[rr[12:], cc[12:]] = F32(-0.0)
                assert (dy[k][rr, cc] != 0).all()
            c["yin"] = yin
            mask = (yin > 0) if relu else np.ones_like(yin, bool)
            dz, grads = O.backward_train(P, cache, dy[k].astype(F64) * mask)
            c["dz"] = dz
            gb_ref += grads[PRE + "beta"]
            gg_ref += grads[PRE + "gamma"]
            c["stat_in"] = c["stat"].astype(F32)
            c["dz_pl"], gb, gg = plain_backward(dy[k], yin, z[k], c["stat_in"], relu)
            gb_pl += gb
            gg_pl += gg
        out["calls"].append(c)
    out.update(dbeta=gb_ref, dgamma=gg_ref, dbeta_pl=gb_pl.astype(F32), dgamma_pl=gg_pl.astype(F32))
    return out


def ulp4(colmax):
    return 4.0 * np.spacing(np.asarray(colmax, F64).astype(F32)).astype(F64)


class Errors:
    """per output: the kernel's excess over the 4-ulp allowance, the restatement's error and the project-scale figure, as maxima"""

    def __init__(self):
        self.d = {}

    def add(self, name, got, plain, ref):
        """got, plain, ref: [rows][cols] or [cols]; the allowance is per column"""
        got, plain, ref = (np.asarray(v).reshape(-1, np.shape(ref)[-1]) for v in (got, plain, ref))
        assert ref.dtype == F64
        allow = ulp4(np.abs(ref).max(0))
        with np.errstate(invalid="ignore"):
            ek = np.abs(got - ref)
            excess, kern, pl = (ek - allow).max(), ek.max(), np.abs(plain - ref).max()
        if not np.isfinite(excess):
            excess = kern = float("inf")                  # a NaN or inf in the kernel's output fails whatever the restatement did
        scale = kern / max(np.abs(ref).max(), 1.0)
        e = self.d.setdefault(name, [-np.inf, 0.0, 0.0, 0.0])
        e[0], e[1], e[2], e[3] = max(e[0], excess), max(e[1], pl), max(e[2], kern), max(e[3], scale)

    def check(self):
        bad = []
        for name, (excess, pl, kern, scale) in self.d.items():
            w = WORST.setdefault(name, [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], kern), max(w[1], scale), max(w[2], excess / (4 * pl) if pl > 0 else (0.0 if excess <= 0 else np.inf))
            if not excess <= 4.0 * pl:
                bad.append((name, "kernel %.3e (after the 4-ulp allowance %.3e) > 4 x plain fp32 %.3e" % (kern, excess, pl)))
        return bad

    def text(self):
        return " ".join("%s k=%.1e p=%.1e s=%.1e" % (n, e[2], e[1], e[3]) for n, e in self.d.items())


# ---------------------------------------------------------------------------------------------------------------------------------
# the expected plan, from reading launch_bn_forward / launch_bn_backward / bn_slices / bn_narrow_grid
# ---------------------------------------------------------------------------------------------------------------------------------
def want_plan(route, backward, rows, cols, calls, training, scratch_floats):
    p = dict(route=route, backward=1 if backward else 0, calls=calls, q=0, R=0)
    if route == "small":
        p.update(launches=1, slices=0, per=0, pgx=(cols + 15) // 16, pgy=1, egrid=0)
        return p
    slices = per = 0
    if training:
        slices = min(512, scratch_floats // (2 * cols))
        slices = max(1, min(slices, (rows + 63) // 64))
        per = (rows + slices - 1) // slices
        slices = (rows + per - 1) // per
    p.update(launches=calls * (3 if training else 2), slices=slices, per=per)
    if route == "sliced":
        p.update(pgx=(cols + 63) // 64 if training else 0, pgy=slices, egrid=min((rows * (pad4(cols) // 4) + 255) // 256, 4096))
    else:
        q = pad4(cols) // 4
        R = 256 // q
        p.update(pgx=slices, pgy=1 if training else 0, egrid=max(1, min(8192, (rows + 4 * R - 1) // (4 * R))), q=q, R=R)
    return p


# ---------------------------------------------------------------------------------------------------------------------------------
# device buffers
# ---------------------------------------------------------------------------------------------------------------------------------
def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def dev_matrix(mat, ld, dev):
    """mat [calls][rows][cols] -> whole [GUARD + calls*rows + GUARD][ld] on the device and its body: zeros up to pad4(cols), NaN beyond"""
    import torch
    calls, rows, cols = mat.shape
    whole = torch.full((calls * rows + 2 * GUARD, ld), float("nan"), dtype=torch.float32)
    body = whole[GUARD:GUARD + calls * rows]
    body[:, :pad4(cols)] = 0.0
    body[:, :cols] = torch.from_numpy(np.ascontiguousarray(mat.reshape(calls * rows, cols)))
    whole = whole.to(dev)
    return whole, whole[GUARD:GUARD + calls * rows]


def dev_fill(nrows, ld, dev, value=SENT):
    import torch
    whole = torch.full((nrows + 2 * GUARD, ld), value, dtype=torch.float32, device=dev)
    return whole, whole[GUARD:GUARD + nrows]


def dev_vector(vals, dev, value=SENT):
    """[4 sentinels | values | 8 sentinels]; returns (whole, view)"""
    import torch
    n = len(vals)
    whole = torch.full((4 + n + 8,), value, dtype=torch.float32)
    whole[4:4 + n] = torch.from_numpy(np.ascontiguousarray(vals, F32))
    whole = whole.to(dev)
    return whole, whole[4:4 + n]


def dev_stat(slots, cols, ldc, dev, rows_data=None):
    """[GUARD + slots*6 + GUARD][ldc] of sentinels with the padding columns [cols, pad4(cols)) of the body zero (the contract)"""
    import torch
    whole = torch.full((slots * 6 + 2 * GUARD, ldc), SENT, dtype=torch.float32)
    whole[GUARD:GUARD + slots * 6, cols:pad4(cols)] = 0.0
    if rows_data is not None:
        whole[GUARD:GUARD + rows_data.shape[0], :cols] = torch.from_numpy(np.ascontiguousarray(rows_data, F32))
    whole = whole.to(dev)
    return whole, whole[GUARD:GUARD + slots * 6]


def dev_scratch(floats, dev):
    import torch
    whole = torch.full((floats + BAND,), float("nan"), dtype=torch.float32)
    whole[floats:] = SENT
    return whole.to(dev)


def same_outside(after, before, written):
    """after, before: whole buffers on the CPU; written: bool mask of what the launch may write.  Everything else bit-unchanged."""
    return bool((bits(after) == bits(before))[~written].all())


def band_intact(scratch, floats):
    import torch
    return bool((bits(scratch[floats:].cpu()) == torch.tensor(SENT).view(torch.int32).item()).all())


def stops_the_module(fn):
    """anything but a failed assertion out of a launch (a HIP error) keeps every later test and the child process from starting"""
    def wrapped(*a, **kw):
        try:
            return fn(*a, **kw)
        except AssertionError:
            raise
        except Exception:
            _FAULTED.append(fn.__name__)
            raise
    return wrapped


# ---------------------------------------------------------------------------------------------------------------------------------
# one case: forward, then (training) backward, over 16 / cols windows
# ---------------------------------------------------------------------------------------------------------------------------------
def case(rows, cols, route, calls=1, training=True, relu=True, ex=(4, 8, 12), scratch="model", bwd_route=None, accumulate=False,
         no_dbeta=False, edges=False, want=None):
    """ex: columns of (z, y, dy) beyond pad4(cols) (all 0: the narrow form's layout); scratch: "model" or a float count;
    want: literal plan fields checked on top of the transcription"""
    return dict(rows=rows, cols=cols, route=route, calls=calls, training=training, relu=relu, ex=ex, scratch=scratch,
                bwd_route=bwd_route or route, accumulate=accumulate, no_dbeta=no_dbeta, edges=edges, want=want or {})


def case_id(c):
    s = "%s-%dx%d" % (c["route"], c["rows"], c["cols"])
    if c["calls"] > 1:
        s += "-calls%d" % c["calls"]
    for k in ("accumulate", "no_dbeta", "edges"):
        if c[k]:
            s += "-" + k
    if not c["training"]:
        s += "-infer"
    if not c["relu"]:
        s += "-norelu"
    if c["scratch"] != "model":
        s += "-scr%d" % c["scratch"]
    if c["ex"] != (4, 8, 12):
        s += "-ex%d.%d.%d" % c["ex"]
    return s


def check_plan(plan, c, route, backward, sf):
    w = want_plan(route, backward, c["rows"], c["cols"], c["calls"], c["training"], sf)
    assert plan == w, ("plan", plan, "expected", w)
    for k, v in c["want"].items():
        if k.startswith("bwd_") == bool(backward) or not k.startswith(("bwd_", "fwd_")):
            kk = k.split("_", 1)[1] if k.startswith(("bwd_", "fwd_")) else k
            assert plan[kk] == v, (kk, plan[kk], v)


@stops_the_module
def run_case(eng, c, setting="default"):
    import torch
    dev = eng.device
    rows, cols, calls, training, relu = c["rows"], c["cols"], c["calls"], c["training"], c["relu"]
    cp = pad4(cols)
    ldz, ldy, ldd, ldc = cp + c["ex"][0], cp + c["ex"][1], cp + c["ex"][2], cp + (0 if c["ex"] == (0, 0, 0) else 4)
    sf = model_scratch(cols) if c["scratch"] == "model" else c["scratch"]
    windows = (16 + cols - 1) // cols
    M = calls * rows
    ef, eb = Errors(), Errors()
    plans = {}
    failures = []
    t0 = time.time()
    for w in range(windows):
        acc_init = None
        if c["accumulate"]:
            gi = np.random.default_rng([19, cols, w])
            acc_init = (gi.normal(0, 3, cols).astype(F32), gi.normal(0, 3, cols).astype(F32))
        ref = reference(rows, cols, calls, w, training, relu, c["edges"], acc_init)
        st = ref["st"]
        if w == 0 and training:
            rr, dd = np.stack([k["r"] for k in ref["calls"]]), np.stack([k["d"] for k in ref["calls"]])
            rng_text = "r in [%.2f, %.2f] d in [%.2f, %.2f]" % (rr.min(), rr.max(), dd.min(), dd.max())
            assert cols < 16 or (np.abs(rr - 1).max() > 0.2 and np.abs(dd).max() > 0.2), "the state is too close to the initial one"
        elif w == 0:
            rng_text = "inference"
        # ---- forward: two launches on fresh outputs
        zw, zd = dev_matrix(ref["z"], ldz, dev)
        z_before = zw.clone()
        var_bufs = [dev_vector(st[n], dev) for n in VARS]
        var_before = [b[0].cpu() for b in var_bufs]
        outs = []
        for rep in range(2):
            yw, yd = dev_fill(M, ldy, dev)
            sw, sd = dev_stat(calls + 1, cols, ldc, dev)
            scr = dev_scratch(sf, dev)
            y0, s0 = yw.cpu(), sw.cpu()
            eng.op_bn_forward(zd, yd, rows, cols, [b[1] for b in var_bufs], sd, scr, calls=calls, training=training, relu=relu,
                              scratch_floats=sf)
            if rep == 0:
                plans["fwd"] = eng.op_bn_last_plan()
            torch.cuda.synchronize()
            outs.append((yw, sw, scr))
        if not all(torch.equal(bits(a), bits(b)) for a, b in zip(outs[0][:2], outs[1][:2])):
            failures.append("two forward launches differ")
        ya, sa, scra = (t.cpu() for t in outs[0])
        del outs
        froute = plans["fwd"]["route"]
        ycols = cols if froute == "small" else cp                     # the small route writes c < cols only
        for k in range(calls):
            ck = ref["calls"][k]
            got_y = ya[GUARD + k * rows:GUARD + (k + 1) * rows, :cols].numpy()
            ef.add("y", got_y, ck["y_pl"], ck["y"])
            got_s = sa[GUARD + 6 * k:GUARD + 6 * k + 6, :cols].numpy()
            names = ("mean", "sd", "r", "d", "a", "b")
            for i in (range(6) if training else (4, 5)):
                ef.add(names[i], got_s[i], ck["stat_pl"][i], ck["stat"][i if training else i - 4])
            if c["edges"] and training:                               # a constant column: var = 0 exactly, stddev = sqrt(eps)
                assert got_s[1][0] == F32(np.sqrt(EPS32)) and got_s[0][0] == F32(3.25), ("constant column", got_s[0][0], got_s[1][0])
            if c["edges"] and training and relu:
                assert not got_y[:, 4].any(), "an all-negative pre-activation column gave y != 0"
        wy = torch.zeros_like(y0, dtype=torch.bool)
        wy[GUARD:GUARD + M, :ycols] = True
        ws_ = torch.zeros_like(s0, dtype=torch.bool)
        for k in range(calls):
            ws_[GUARD + 6 * k + (0 if training else 4):GUARD + 6 * k + 6, :cols] = True
        if froute != "small" and not bool((bits(ya[GUARD:GUARD + M, cols:cp]) == 0).all()):
            failures.append("padding columns of y are not +0.0")
        if not same_outside(ya, y0, wy):
            failures.append("y written outside [rows][%d]" % ycols)
        if not same_outside(sa, s0, ws_):
            failures.append("stat written outside the rows of the calls that ran (or in its padding columns)")
        if not band_intact(scra, sf):
            failures.append("forward wrote behind scratch")
        if not all(torch.equal(bits(b[0].cpu()), bits(v0)) for b, v0 in zip(var_bufs, var_before)):
            failures.append("the forward pass changed a variable")
        if not training:
            continue
        # ---- backward: y and stat from the reference (fp32), two launches on fresh copies (dz is written over dy)
        yin = np.stack([k["yin"] for k in ref["calls"]])
        if relu:
            yinw, yind = dev_matrix(yin, ldy, dev)
        else:
            yinw, yind = dev_fill(M, ldy, dev, float("nan"))          # not read without the ReLU
        stat_in = np.concatenate([k["stat_in"] for k in ref["calls"]])
        stw, std_ = dev_stat(calls + 1, cols, ldc, dev, stat_in)
        st_before = stw.cpu()
        outs = []
        for rep in range(2):
            dw, dd_ = dev_matrix(ref["dy"], ldd, dev)
            if c["no_dbeta"]:
                gbw = ggw = gbd = ggd = None
            else:
                gbw, gbd = dev_vector(acc_init[0] if acc_init else np.full(cols, SENT, F32), dev)
                ggw, ggd = dev_vector(acc_init[1] if acc_init else np.full(cols, SENT, F32), dev)
            sums = torch.full((2 * ldc + 64,), SENT, dtype=torch.float32, device=dev)
            scr = dev_scratch(sf, dev)
            d0 = dw.cpu()
            eng.op_bn_backward(dd_, yind, zd, rows, cols, std_, sums, scr, dbeta=gbd, dgamma=ggd, calls=calls, accumulate=c["accumulate"],
                               relu=relu, scratch_floats=sf)
            if rep == 0:
                plans["bwd"] = eng.op_bn_last_plan()
            torch.cuda.synchronize()
            outs.append((dw, gbw, ggw, sums, scr))
        for a, b in zip(outs[0][:3], outs[1][:3]):
            if a is not None and not torch.equal(bits(a), bits(b)):
                failures.append("two backward launches differ")
        da, gba, gga, suma, scra = (None if t is None else t.cpu() for t in outs[0])
        del outs
        broute = plans["bwd"]["route"]
        dcols = cols if broute == "small" else cp
        for k in range(calls):
            ck = ref["calls"][k]
            got = da[GUARD + k * rows:GUARD + (k + 1) * rows, :cols].numpy()
            eb.add("dz", got, ck["dz_pl"], ck["dz"])
            if c["edges"] and relu:
                assert not got[:, 4].any(), "dz != 0 in a column whose every y is 0"
        if not c["no_dbeta"]:
            eb.add("dbeta", gba[4:4 + cols].numpy(), ref["dbeta_pl"], ref["dbeta"])
            eb.add("dgamma", gga[4:4 + cols].numpy(), ref["dgamma_pl"], ref["dgamma"])
            if c["edges"] and relu and not c["accumulate"]:
                assert gba[4 + 4] == 0 and gga[4 + 4] == 0, "dbeta / dgamma != 0 in a column whose every y is 0"
            for gv in (gba, gga):
                if not bool((bits(gv[:4]) == bits(torch.tensor([SENT] * 4))).all() and (bits(gv[4 + cols:]) == bits(torch.tensor([SENT] * 8))).all()):
                    failures.append("dbeta / dgamma written outside [cols]")
        wd = torch.zeros_like(d0, dtype=torch.bool)
        wd[GUARD:GUARD + M, :dcols] = True
        if not same_outside(da, d0, wd):
            failures.append("dz written outside [rows][%d]" % dcols)
        if broute != "small" and not bool((da[GUARD:GUARD + M, cols:cp] == 0).all()):
            failures.append("padding columns of dz are not 0")
        if broute != "small":
            sm = torch.ones_like(suma, dtype=torch.bool)
            sm[:cols] = False
            sm[ldc:ldc + cols] = False
            if not bool((bits(suma[sm]) == torch.tensor(SENT).view(torch.int32).item()).all()):
                failures.append("sums written outside [2][cols]")
        if not band_intact(scra, sf):
            failures.append("backward wrote behind scratch")
        if not (torch.equal(bits(stw.cpu()), bits(st_before)) and torch.equal(bits(zw), bits(z_before))):
            failures.append("the backward pass changed stat or z")
    host = time.time() - t0
    line = "bn_ops %-8s %-40s fwd %s %s | %s" % (setting, case_id(c), fmt_plan(plans["fwd"]), ef.text(), rng_text)
    print(line)
    LINES.append(line)
    if training:
        line = "bn_ops %-8s %-40s bwd %s %s" % (setting, case_id(c), fmt_plan(plans["bwd"]), eb.text())
        print(line)
        LINES.append(line)
    print("bn_ops host time %.2f s (%d windows)" % (host, windows))
    bad = ef.check() + eb.check()
    assert not bad, bad
    assert not failures, sorted(set(failures))
    # numbers first, the plan second
    assert plans["fwd"]["route"] == c["route"], plans["fwd"]
    check_plan(plans["fwd"], c, c["route"], False, sf)
    COVERED.add((c["route"], "fwd", calls > 1, training, relu))
    if training:
        assert plans["bwd"]["route"] == c["bwd_route"], plans["bwd"]
        check_plan(plans["bwd"], c, c["bwd_route"], True, sf)
        COVERED.add((c["bwd_route"], "bwd", calls > 1, True, relu))
    return host


def fmt_plan(p):
    s = "%s launches=%d" % (p["route"], p["launches"])
    if p["route"] != "small":
        s += " slices=%d per=%d part=%dx%d elem=%d" % (p["slices"], p["per"], p["pgx"], p["pgy"], p["egrid"])
    if p["route"] == "narrow":
        s += " q=%d R=%d" % (p["q"], p["R"])
    return s


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------------------
# small route: rows <= 384 and cols >= 64.  rows x cols crossed; calls, the infer / no-ReLU / no-dbeta forms rotate over the cross.
SMALL = []
for i, rows in enumerate((1, 15, 16, 17, 256, 384)):
    for j, cols in enumerate((64, 65, 79, 80, 257)):
        SMALL.append(case(rows, cols, "small", calls=1 + (i + j) % 2, want=dict(pgx=(cols + 15) // 16, launches=1)))
SMALL += [
    case(17, 65, "small", calls=2, training=False),
    case(256, 80, "small", calls=2, training=False),
    case(16, 79, "small", relu=False),
    case(384, 257, "small", no_dbeta=True),
    case(256, 80, "small", edges=True),
]
# route boundaries: rows 384 -> 385, cols 63 -> 64, accumulate on a small shape
BOUNDARY = [
    case(384, 64, "small"),
    case(385, 64, "sliced", want=dict(slices=7, per=55)),
    case(384, 63, "sliced", want=dict(slices=6, per=64)),
    case(256, 80, "small", bwd_route="sliced", accumulate=True, want=dict(bwd_slices=4, bwd_per=64, bwd_launches=3)),
]
# sliced route.  32769 rows with at most 16 columns: 16384 / (2 cols) >= 512 slices allowed, (rows + 63) / 64 = 513 -> 512, per = 65,
# 505 slices, the last of 9 rows.  4200 x 1024: 4200 workgroups of elementwise work, capped at 4096.
SLICED = [
    case(1, 1, "sliced", want=dict(slices=1, per=1)), case(1, 63, "sliced"), case(63, 3, "sliced"), case(63, 63, "sliced"),
    case(64, 5, "sliced", want=dict(slices=1, per=64)), case(64, 1, "sliced"), case(65, 63, "sliced", want=dict(slices=2, per=33)),
    case(65, 3, "sliced"), case(385, 5, "sliced"), case(385, 130, "sliced", relu=False), case(385, 64, "sliced", calls=2),
    case(1000, 65, "sliced", want=dict(slices=16, per=63)), case(1000, 1, "sliced"), case(1000, 130, "sliced"),
    case(1000, 5, "sliced", calls=2, want=dict(launches=6)),
    case(1000, 65, "sliced", scratch=2 * 65, want=dict(slices=1, per=1000, pgy=1)),
    case(1000, 65, "sliced", scratch=6 * 65 + 1, want=dict(slices=3, per=334, pgy=3)),
    case(1000, 65, "sliced", no_dbeta=True), case(1000, 65, "sliced", calls=2, training=False), case(65, 3, "sliced", training=False),
    case(1000, 65, "sliced", edges=True),
    case(32769, 5, "sliced", want=dict(slices=505, per=65)), case(32769, 3, "sliced", want=dict(slices=505, per=65)),
    case(32769, 64, "sliced", scratch=2 * 64 * 600, want=dict(slices=505, per=65)),
    case(32769, 130, "sliced", want=dict(slices=128, per=257)),
    case(4200, 1024, "sliced", want=dict(egrid=4096)),
]
# narrow route at the default switch: rows >= 4096, every leading dimension = pad4(cols) <= 64.  Every ld in {4 .. 64} with cols = ld,
# ld - 1 and ld - 3, the four row counts rotating; ld / 4 = 3, 5, 6, 7, 9 .. 15 do not divide 256 (R = 256 / q leaves idle threads).
NARROW = []
for i, ld in enumerate(range(4, 68, 4)):
    for j, cols in enumerate((ld, ld - 1, ld - 3)):
        NARROW.append(case((4096, 4097, 4099, 5000)[(i + j) % 4], cols, "narrow", ex=(0, 0, 0), want=dict(q=ld // 4, R=256 // (ld // 4))))
NARROW += [
    case(5000, 12, "narrow", ex=(0, 0, 0), want=dict(q=3, R=85)), case(4097, 57, "narrow", ex=(0, 0, 0), want=dict(q=15, R=17)),
    case(4097, 64, "narrow", ex=(0, 0, 0), calls=2),
    case(4099, 24, "narrow", ex=(0, 0, 0), calls=2, want=dict(launches=6)), case(4096, 28, "narrow", ex=(0, 0, 0), training=False),
    case(4097, 33, "narrow", ex=(0, 0, 0), relu=False), case(5000, 44, "narrow", ex=(0, 0, 0), no_dbeta=True),
    case(4099, 30, "narrow", ex=(0, 0, 0), edges=True),
    case(4096, 12, "sliced", ex=(0, 4, 0)),                            # unequal leading dimensions: the same shape is sliced
    case(4095, 12, "sliced", ex=(0, 0, 0)),                            # one row below the switch
]
# past the 8192-workgroup cap of k_bn_elem_narrow (ld = 64: R = 16, 64 rows per workgroup and pass): 134 MB per matrix, the only large case
BIG = case(8192 * 64 + 53, 64, "narrow", ex=(0, 0, 0), want=dict(egrid=8192, slices=128, per=4097))


@pytest.fixture(scope="module")
def eng():
    from rsrgan_amd.ops import OpEntries
    return OpEntries()


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    if _FAULTED:
        pytest.fail("not run: %s raised a HIP error earlier in this module" % _FAULTED[0])


@pytest.mark.gpu
@pytest.mark.parametrize("c", SMALL, ids=[case_id(c) + "-%d" % i for i, c in enumerate(SMALL)])
def test_small_route(eng, c):
    run_case(eng, c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", BOUNDARY, ids=[case_id(c) + "-%d" % i for i, c in enumerate(BOUNDARY)])
def test_route_boundaries(eng, c):
    run_case(eng, c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", SLICED, ids=[case_id(c) + "-%d" % i for i, c in enumerate(SLICED)])
def test_sliced_route(eng, c):
    run_case(eng, c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", NARROW, ids=[case_id(c) + "-%d" % i for i, c in enumerate(NARROW)])
def test_narrow_route(eng, c):
    run_case(eng, c)


@pytest.mark.gpu
def test_narrow_past_the_elementwise_grid_cap(eng):
    """rows = 8192 x 64 + 53 at ld = 64: the threads of k_bn_elem_narrow take a second pass.  The host side (inputs, the fp64 reference, the
    restatement, the copies) dominates this test; its time is printed."""
    host = run_case(eng, BIG)
    print("bn_ops the 134 MB narrow case: %.1f s of host time" % host)


# ---------------------------------------------------------------------------------------------------------------------------------
# the state update
# ---------------------------------------------------------------------------------------------------------------------------------
COMMIT_COLS = (1, 256, 257, 1000)


def commit_inputs(cols, seed):
    st = make_state(cols, 100 + seed)
    g = np.random.default_rng([23, cols, seed])
    stat = np.zeros((12, cols), F32)
    for u in range(2):
        stat[6 * u] = g.normal(0, 2, cols)
        stat[6 * u + 1] = g.uniform(0.1, 3.0, cols)
        stat[6 * u + 2:6 * u + 6] = g.normal(0, 1, (4, cols))
    return st, stat


def commit_reference(st, stat, t0, t1):
    P = oracle_params(st)
    for u, t in ((0, t0), (1, t1)):
        for _ in range(t):
            O.commit(P, dict(scope=SCOPE, mean=stat[6 * u].astype(F64), std=stat[6 * u + 1].astype(F64)))
    return P


@stops_the_module
def run_commit(eng, t0, t1, single=False):
    """the four layers in one launch (single: one launch each); returns the whole variable buffers of every layer"""
    import torch
    dev = eng.device
    entries, keep = [], []
    for i, cols in enumerate(COMMIT_COLS):
        st, stat = commit_inputs(cols, i)
        bufs = [dev_vector(st[n], dev) for n in VARS]
        sw, sd = dev_stat(2, cols, pad4(cols) + 4, dev, stat)
        keep.append((st, stat, bufs, sw, sw.cpu()))
        entries.append(([b[1] for b in bufs], sd, cols, t0, t1))
    if single:
        for e in entries:
            eng.op_bn_commit([e], single=True)
    else:
        eng.op_bn_commit(entries)
    torch.cuda.synchronize()
    return keep


@pytest.mark.gpu
@pytest.mark.parametrize("t0,t1", [(1, 0), (2, 1), (3, 3), (0, 2)])
def test_commit_many_matches_the_oracle(eng, t0, t1):
    import torch
    keep = run_commit(eng, t0, t1)
    worst = {}
    for cols, (st, stat, bufs, sw, s0) in zip(COMMIT_COLS, keep):
        P = commit_reference(st, stat, t0, t1)
        assert torch.equal(bits(sw.cpu()), bits(s0)), "the update wrote into stat"
        for name, (whole, view) in zip(VARS, bufs):
            got = whole.cpu()
            assert bool((got[:4] == SENT).all() and (got[4 + len(st[name]):] == SENT).all()), (name, "written outside its extent")
            g = got[4:4 + len(st[name])].numpy().astype(F64)
            if name in ("beta", "gamma"):
                assert np.array_equal(g, st[name].astype(F64)), name
                continue
            ref = np.atleast_1d(P[PRE + name])
            rel = (np.abs(g - ref) / np.abs(ref)).max()
            worst[name] = max(worst.get(name, 0.0), rel)
            assert rel <= 2.0 ** -23, (cols, name, rel)                   # computed in double, rounded once (the two weights are separate buffers)
            assert not np.array_equal(g, st[name].astype(F64)), (name, "unchanged")
    line = "bn_ops commit_many times (%d, %d) cols %s: rel " % (t0, t1, COMMIT_COLS) + " ".join("%s %.1e" % kv for kv in worst.items())
    print(line)
    LINES.append(line)


@pytest.mark.gpu
@pytest.mark.parametrize("times", [1, 2, 3])
def test_commit_single_equals_commit_many(eng, times):
    import torch
    many, one = run_commit(eng, times, 0), run_commit(eng, times, 0, single=True)
    for a, b in zip(many, one):
        for name, (wa, _), (wb, _) in zip(VARS, a[2], b[2]):
            assert torch.equal(bits(wa.cpu()), bits(wb.cpu())), (name, "k_bn_commit and k_bn_commit_many differ")


# ---------------------------------------------------------------------------------------------------------------------------------
# the mistakes the bound must catch (CPU only)
# ---------------------------------------------------------------------------------------------------------------------------------
# shapes of the tables, one or two per route, up to the 32769 rows of the slice cap.  Not the 524341-row shape (20 s of restatements on
# the CPU): there 1 / n = 2e-6 is below the error of a plain fp32 sum of n terms, so the bound cannot separate n - 1 or a lost row, and the
# plain errors of dbeta / dgamma are 4.2 / 8.9 absolute (1e-5 of the sums' terms' total): that case guards the second elementwise pass and
# the slice arithmetic, the shorter shapes guard the formulas.
MUT_SHAPES = [(17, 80), (256, 80), (384, 64), (65, 63), (1000, 65), (4099, 30), (32769, 64)]
MUTATIONS = ("dterm", "swap", "nm1", "lastrow", "nomask", "unshifted")


def test_mutations_exceed_the_bound():
    """each mistake, applied to the restatement, must break  excess <= 4 x plain  on at least one output, by the printed margin"""
    g = np.random.default_rng(29)
    for shape in ((70000, 64), (4200, 1024)):                    # the two summation routines of seqsum agree bit for bit
        x = g.standard_normal(shape, dtype=F32) + F32(0.5)
        assert x.size >= SEQSUM_REDUCE_FROM and np.array_equal(seqsum(x), seqsum(x, force_cumsum=True)), shape
        assert not np.array_equal(seqsum(x), x.sum(0, dtype=F64).astype(F32))        # (and are not simply exact)
    for rows, cols in MUT_SHAPES:
        ref = reference(rows, cols, 1, 0, True, True, True, None)
        ck, st = ref["calls"][0], ref["st"]
        for mut in MUTATIONS:
            e = Errors()
            if mut in ("swap", "nm1", "unshifted") or mut == "lastrow":
                stat, y = plain_forward(ref["z"][0], st, mut=mut)
                e.add("y", y, ck["y_pl"], ck["y"])
                for i, n in enumerate(("mean", "sd", "r", "d", "a", "b")):
                    e.add(n, stat[i], ck["stat_pl"][i], ck["stat"][i])
            if mut in ("dterm", "lastrow", "nomask"):
                dz, gb, gg = plain_backward(ref["dy"][0], ck["yin"], ref["z"][0], ck["stat_in"], mut=mut)
                e.add("dz", dz, ck["dz_pl"], ck["dz"])
                e.add("dbeta", gb.astype(F32), ref["dbeta_pl"], ref["dbeta"])
                e.add("dgamma", gg.astype(F32), ref["dgamma_pl"], ref["dgamma"])
            name, margin = max(((n, v[0] / (4 * v[1]) if v[1] > 0 else np.inf) for n, v in e.d.items()), key=lambda t: t[1])
            print("bn_ops mutation %-9s %5d x %-3d: worst output %-6s exceeds the bound %.1f x" % (mut, rows, cols, name, margin))
            if mut == "unshifted":                                   # the claim is about the 1000 + 1e-2 noise column
                ex = np.abs(stat[1].astype(F64)[1] - ck["stat"][1][1]) - ulp4(ck["stat"][1][1])
                assert ex > 4 * np.abs(F64(ck["stat_pl"][1][1]) - ck["stat"][1][1]), (rows, cols, ex)      # (against that column's own plain error)
            assert margin > 1.0, (mut, rows, cols, name, margin)


# ---------------------------------------------------------------------------------------------------------------------------------
# RSRGAN_BN_NARROW=1 RSRGAN_BN_SMALL_ROWS=0 in one fresh child process
# ---------------------------------------------------------------------------------------------------------------------------------
CHILD_ENV = {"RSRGAN_BN_NARROW": "1", "RSRGAN_BN_SMALL_ROWS": "0"}
CHILD_CHECK_FAILED = 2         # exit status of a child whose launches all returned but a check failed; anything else nonzero: the card may be gone
CHILD = []
for ld, cols in ((4, 3), (12, 11), (64, 64)):
    R = 256 // (ld // 4)
    for rows in (1, 2, R - 1, R, 4 * R, 4 * R + 1, 70):
        CHILD.append(case(rows, cols, "narrow", ex=(0, 0, 0)))
CHILD += [case(256, 80, "sliced"), case(17, 64, "sliced", calls=2), case(384, 257, "sliced")]


def worker_main():
    """exit status 0: passed; CHILD_CHECK_FAILED: an assertion failed (the card is fine); any other exception -- a HIP error out of an
    entry or of the synchronize is one -- leaves with the interpreter's status 1, which the parent treats like an abort or a time-out"""
    import traceback
    from rsrgan_amd.ops import OpEntries
    try:
        e = OpEntries()
        for c in CHILD:
            run_case(e, c, setting="narrow=1")
    except AssertionError:
        traceback.print_exc()
        sys.stdout.flush()
        sys.exit(CHILD_CHECK_FAILED)
    print("RESULT " + json.dumps({"covered": sorted(COVERED), "worst": WORST}))


@pytest.mark.gpu
def test_narrow_at_few_rows_and_sliced_at_small_shapes_in_a_child_process():
    e = dict(os.environ)
    e.update(CHILD_ENV)
    src = "import sys; sys.path.insert(0, %r); from tests import test_gpu_bn_ops as t; t.worker_main()" % ROOT
    try:
        p = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, env=e, timeout=240)
    except subprocess.TimeoutExpired:
        _FAULTED.append("the child process (timed out)")
        raise
    for line in p.stdout.splitlines():
        if line.startswith("bn_ops "):
            print(line)
            if not line.startswith("bn_ops host"):
                LINES.append(line)
    if p.returncode not in (0, CHILD_CHECK_FAILED):            # a signal, an abort, or an exception that was no failed check (a HIP error)
        _FAULTED.append("the child process (status %d)" % p.returncode)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert len(out["covered"]) >= 4
    for route, direction, multi, training, relu in out["covered"]:
        COVERED.add((route, direction, multi, training, relu))
    for name, w in out["worst"].items():
        mine = WORST.setdefault(name, [0.0, 0.0, 0.0])
        WORST[name] = [max(a, b) for a, b in zip(mine, w)]


# ---------------------------------------------------------------------------------------------------------------------------------
# The ledger (route, direction, calls > 1, training, relu), by hand from the tables above: every route runs forward and backward with
# one call and with two, without the ReLU (one call), and forward with training = false -- on the small and sliced routes with two calls
# (SMALL, SLICED: 17 x 65 / 256 x 80 / 1000 x 65 with calls = 2), on the sliced and narrow routes with one (65 x 3, 4096 x 28).
# ---------------------------------------------------------------------------------------------------------------------------------
LEDGER = set(
    [(route, d, multi, True, True) for route in ("small", "sliced", "narrow") for d in ("fwd", "bwd") for multi in (False, True)] +
    [(route, d, False, True, False) for route in ("small", "sliced", "narrow") for d in ("fwd", "bwd")] +
    [("small", "fwd", True, False, True), ("sliced", "fwd", True, False, True), ("sliced", "fwd", False, False, True),
     ("narrow", "fwd", False, False, True)])
N_GPU_TESTS = len(SMALL) + len(BOUNDARY) + len(SLICED) + len(NARROW) + 1 + 4 + 3 + 1 + 1      # every gpu-marked test of this module, the ledger included


@pytest.mark.gpu
def test_zz_ledger(request):
    """prints every combination a passing case asserted and the largest errors, and compares with the hand-written ledger.  Only a run
    that deselected tests of this module (-k, a node id) is excused: then nothing can be required"""
    print("bn_ops combinations asserted by passing cases: %d of %d" % (len(COVERED & LEDGER), len(LEDGER)))
    for cmb in sorted(COVERED):
        print("  bn_ops covered %s" % (cmb,))
    for name, (kern, scale, ratio) in WORST.items():
        print("bn_ops worst %-6s max |err| %.2e, on the scale max(|ref|, 1) %.2e, excess / bound %.2f" % (name, kern, scale, ratio))
    mine = [i for i in request.session.items if i.nodeid.split("::")[0].endswith("test_gpu_bn_ops.py") and i.get_closest_marker("gpu")]
    if len(mine) != N_GPU_TESTS:                                  # (-m gpu deselects only the CPU mutation test: the ledger is compared)
        print("bn_ops partial run (%d of %d gpu tests selected): the ledger is not compared" % (len(mine), N_GPU_TESTS))
        return
    assert LEDGER - COVERED == set(), ("combinations no passing case reached", sorted(LEDGER - COVERED))
    assert COVERED - LEDGER == set(), ("combinations missing from the hand-written ledger", sorted(COVERED - LEDGER))
