"""csrc/bn_seq.hip: batch_norm(renorm=True) + leaky-ReLU under the row rule (Bp, Bt) of a padded time-major batch, through
rsrgan_op_bn_seq_forward / _backward, against oracle/bn_renorm.py in fp64 evaluated on the COUNTED rows only (row r counts iff
Bp == 0 or r % Bp < Bt); the leaky step is applied here.  Inputs, guards, the two error figures and their bounds are those of
tests/test_gpu_bn_ops.py for the sliced route, imported from it unchanged:
    max over the output of (|kernel - ref| - 4 ulp32(max |ref| of the column))  <=  4 x max |plain - ref|
with `plain` the plain fp32 restatement (first-row shift, sums in fp32 in row order over the counted rows, moments finished in fp64),
and the project's scale max |err| / max(|ref|_max, 1) printed beside it.  Shapes narrower than 16 columns run 16 / cols windows.

Every training case runs its launches three times: padding rows of z and dy filled with 1e6, again with 1e6 (two runs of the same
call must be bit-identical) and with 0 (statistics, y and dz on the counted rows, dbeta, dgamma bit-identical between the fills;
the padding rows of y and dz exactly 0).  The single counted row (32, 1, 1) must give variance 0: stddev = sqrt(eps), mean = z0.

test_wrong_n_misses_the_bound (CPU): the restatement with n = T.Bp in place of T.Bt must exceed the bound by at least 10 x on every
shape with padding rows -- otherwise the shapes would prove nothing about the mask."""
import os

import numpy as np
import pytest

from oracle import bn_renorm as O
from tests import test_gpu_bn_ops as B

F32, F64 = np.float32, np.float64
COLS = (7, 280, 1024)
SHAPES = ((0, 0, 5), (32, 8, 12), (32, 1, 1), (64, 33, 5), (32, 32, 100))        # (Bp, Bt, T); Bp = 0: rows = T, all counted
ALPHAS = (0.3, 0.0)
MODES = ("initial", "random", "infer")
LINES = []
_FAULTED = []


def n_rows(Bp, T):
    return T if Bp == 0 else T * Bp


def counted(Bp, Bt, T):
    r = np.arange(n_rows(Bp, T))
    return np.ones(len(r), bool) if Bp == 0 else (r % Bp) < Bt


def leaky(x, alpha):
    return np.where(x > 0, x, x * x.dtype.type(alpha))


def initial_state(cols):
    st = {k.rsplit("/", 1)[-1]: np.atleast_1d(v).astype(F32) for k, v in O.init_vars(B.SCOPE, cols).items()}
    return st


def build(cols, Bp, Bt, T, alpha, mode, w, n_wrong=False):
    """one window: inputs, the fp64 reference on the counted rows, the plain restatement.  n_wrong: the restatement with n = all rows"""
    rows, cnt = n_rows(Bp, T), counted(Bp, Bt, T)
    st = initial_state(cols) if mode == "initial" else B.make_state(cols, 40 + w)
    z, dy = B.make_inputs(rows, cols, 1, 7 + w)
    z, dy = z[0], dy[0]
    P = B.oracle_params(st)
    zc, dc = z[cnt], dy[cnt]
    n = rows if n_wrong else int(cnt.sum())
    out = dict(st=st, z=z, dy=dy, cnt=cnt)
    al = F32(alpha)
    if mode == "infer":
        out["y"] = leaky(O.forward_infer(P, B.SCOPE, zc.astype(F64)), alpha)
        a = P[B.PRE + "gamma"] / np.sqrt(P[B.PRE + "moving_variance"] + O.EPS)
        out["stat"] = np.stack([a, P[B.PRE + "beta"] - P[B.PRE + "moving_mean"] * a])
        stat_pl, y_pl = B.plain_forward(zc, st, False, False)
        out["stat_pl"], out["y_pl"] = stat_pl, leaky(y_pl, al)
        return out
    y, cache = O.forward_train(P, B.SCOPE, zc.astype(F64))
    a = cache["r"] * P[B.PRE + "gamma"] / cache["std"]
    out["stat"] = np.stack([cache["mean"], cache["std"], cache["r"], cache["d"], a,
                            cache["d"] * P[B.PRE + "gamma"] + P[B.PRE + "beta"] - cache["mean"] * a])
    out["y"] = leaky(y, alpha)
    v = zc - zc[0]
    stat_pl = B.finish_forward(zc[0], B.seqsum(v), B.seqsum(v * v), n, st).astype(F32)
    out["stat_pl"], out["y_pl"] = stat_pl, leaky(zc * stat_pl[4] + stat_pl[5], al)
    # backward: y and stat from the reference, rounded; +0.0 and -0.0 planted where dy != 0 (the slope there is alpha)
    yin = out["y"].astype(F32)
    g = np.random.default_rng([31, cols, Bp, Bt, T, w])
    k = min(24, yin.size)
    rr, cc = g.integers(0, yin.shape[0], k), g.integers(0, cols, k)
    yin[rr[:k // 2], cc[:k // 2]] = F32(0.0)
    yin[rr[k // 2:], cc[k // 2:]] = F32(-0.0)
    out["yin"] = yin
    slope = np.where(yin > 0, 1.0, alpha)
    dz, grads = O.backward_train(P, cache, dc.astype(F64) * slope)
    out.update(dz=dz, dbeta=grads[B.PRE + "beta"], dgamma=grads[B.PRE + "gamma"], stat_in=out["stat"].astype(F32))
    gp = np.where(yin > 0, dc, dc * al)
    si = out["stat_in"]
    xh = (zc - si[0]) * (F32(1) / si[1])
    s1, s2 = B.seqsum(gp).astype(F64), B.seqsum(gp * xh).astype(F64)
    out["dbeta_pl"], out["dgamma_pl"] = s1.astype(F32), (si[2].astype(F64) * s2 + si[3].astype(F64) * s1).astype(F32)
    out["dz_pl"] = si[4] * (gp - (s1 / n).astype(F32) - xh * (s2 / n).astype(F32))
    return out


def add_forward(e, ref, y, stat, training):
    e.add("y", y, ref["y_pl"], ref["y"])
    for i in (range(6) if training else (4, 5)):
        e.add(("mean", "sd", "r", "d", "a", "b")[i], stat[i], ref["stat_pl"][i], ref["stat"][i if training else i - 4])


def add_backward(e, ref, dz, gb, gg):
    e.add("dz", dz, ref["dz_pl"], ref["dz"])
    e.add("dbeta", gb, ref["dbeta_pl"], ref["dbeta"])
    e.add("dgamma", gg, ref["dgamma_pl"], ref["dgamma"])


def over_bound(e):
    """[(output, excess / (4 x plain))] of the outputs beyond the bound"""
    bad = []
    for name, (excess, pl, kern, scale) in e.d.items():
        if not excess <= 4.0 * pl:
            bad.append((name, float("inf") if pl == 0 else excess / (4.0 * pl), kern, pl))
    return bad


def with_padding(mat, cnt, fill, cols):
    """[rows][cols] with the counted rows of `mat` and the other rows = fill"""
    full = np.full((len(cnt), cols), fill, F32)
    full[cnt] = mat[cnt] if mat.shape[0] == len(cnt) else mat
    return full


def run_case(eng, cols, Bp, Bt, T, alpha, mode):
    import torch
    dev = eng.device
    rows, cp = n_rows(Bp, T), B.pad4(cols)
    ld = ldc = cp
    sf = 64 * cols                                     # what every model scratch holds for a column reduction
    training = mode != "infer"
    windows = (16 + cols - 1) // cols
    ef, eb = B.Errors(), B.Errors()
    failures = []
    G = B.GUARD
    for w in range(windows):
        ref = build(cols, Bp, Bt, T, alpha, mode, w)
        cnt, st = ref["cnt"], ref["st"]
        pad = ~cnt
        var_bufs = [B.dev_vector(st[n], dev) for n in B.VARS]
        var_before = [b[0].cpu() for b in var_bufs]
        fwd, bwd = [], []
        for fill in (1e6, 1e6, 0.0):
            zw, zd = B.dev_matrix(with_padding(ref["z"], cnt, fill, cols)[None], ld, dev)
            yw, yd = B.dev_fill(rows, ld, dev)
            sw, sd = B.dev_stat(2, cols, ldc, dev)
            scr = B.dev_scratch(sf, dev)
            y0, s0 = yw.cpu(), sw.cpu()
            eng.op_bn_seq_forward(zd, yd, rows, cols, [b[1] for b in var_bufs], sd, scr, alpha=alpha, Bp=Bp, Bt=Bt, training=training,
                                  scratch_floats=sf)
            torch.cuda.synchronize()
            ya, sa = yw.cpu(), sw.cpu()
            fwd.append((ya, sa))
            wy = torch.zeros_like(y0, dtype=torch.bool)
            wy[G:G + rows, :cp] = True
            ws_ = torch.zeros_like(s0, dtype=torch.bool)
            ws_[G + (0 if training else 4):G + 6, :cols] = True
            if not B.same_outside(ya, y0, wy):
                failures.append("y written outside [rows][%d]" % cp)
            if not B.same_outside(sa, s0, ws_):
                failures.append("stat written outside its rows (or in its padding columns)")
            if not B.band_intact(scr.cpu(), sf):
                failures.append("forward wrote behind scratch")
            if not bool((B.bits(ya[G:G + rows][torch.from_numpy(pad)]) == 0).all()):
                failures.append("padding rows of y are not +0.0")
            if not bool((B.bits(ya[G:G + rows, cols:cp]) == 0).all()):
                failures.append("padding columns of y are not +0.0")
            if not training:
                continue
            yin = with_padding(ref["yin"], cnt, fill, cols)
            yinw, yind = B.dev_matrix(yin[None], ld, dev)
            stw, std_ = B.dev_stat(2, cols, ldc, dev, ref["stat_in"])
            st_before, z_before = stw.cpu(), zw.cpu()
            dw, dd_ = B.dev_matrix(with_padding(ref["dy"], cnt, fill, cols)[None], ld, dev)
            gbw, gbd = B.dev_vector(np.full(cols, B.SENT, F32), dev)
            ggw, ggd = B.dev_vector(np.full(cols, B.SENT, F32), dev)
            sums = torch.full((2 * ldc + 64,), B.SENT, dtype=torch.float32, device=dev)
            scr = B.dev_scratch(sf, dev)
            d0 = dw.cpu()
            eng.op_bn_seq_backward(dd_, yind, zd, rows, cols, std_, sums, scr, alpha=alpha, Bp=Bp, Bt=Bt, dbeta=gbd, dgamma=ggd,
                                   scratch_floats=sf)
            torch.cuda.synchronize()
            da, gba, gga, suma = dw.cpu(), gbw.cpu(), ggw.cpu(), sums.cpu()
            bwd.append((da, gba, gga))
            wd = torch.zeros_like(d0, dtype=torch.bool)
            wd[G:G + rows, :cp] = True
            if not B.same_outside(da, d0, wd):
                failures.append("dz written outside [rows][%d]" % cp)
            if not bool((B.bits(da[G:G + rows][torch.from_numpy(pad)]) == 0).all()):
                failures.append("padding rows of dz are not +0.0")
            if not bool((da[G:G + rows, cols:cp] == 0).all()):
                failures.append("padding columns of dz are not 0")
            for gv in (gba, gga):
                if not bool((gv[:4] == B.SENT).all() and (gv[4 + cols:] == B.SENT).all()):
                    failures.append("dbeta / dgamma written outside [cols]")
            sm = torch.ones_like(suma, dtype=torch.bool)
            sm[:cols] = False
            sm[ldc:ldc + cols] = False
            if not bool((suma[sm] == B.SENT).all()):
                failures.append("sums written outside [2][cols]")
            if not B.band_intact(scr.cpu(), sf):
                failures.append("backward wrote behind scratch")
            if not (torch.equal(B.bits(stw.cpu()), B.bits(st_before)) and torch.equal(B.bits(zw.cpu()), B.bits(z_before))):
                failures.append("the backward pass changed stat or z")
        if not all(torch.equal(B.bits(b[0].cpu()), B.bits(v0)) for b, v0 in zip(var_bufs, var_before)):
            failures.append("the forward pass changed a variable")
        cm = torch.from_numpy(cnt)
        body = lambda t: t[G:G + rows]
        if not (torch.equal(B.bits(fwd[0][0]), B.bits(fwd[1][0])) and torch.equal(B.bits(fwd[0][1]), B.bits(fwd[1][1]))):
            failures.append("two forward launches differ")
        if not (torch.equal(B.bits(body(fwd[0][0])[cm]), B.bits(body(fwd[2][0])[cm])) and torch.equal(B.bits(fwd[0][1]), B.bits(fwd[2][1]))):
            failures.append("forward: the padding rows' contents reached the statistics or y")
        ya, sa = fwd[0]
        stat = sa[G:G + 6, :cols].numpy()
        add_forward(ef, ref, ya[G:G + rows, :cols].numpy()[cnt], stat, training)
        if training and int(cnt.sum()) == 1:
            assert (stat[1] == F32(np.sqrt(B.EPS32))).all() and np.array_equal(stat[0], ref["z"][0]), ("single row", stat[0][:4], stat[1][:4])
        if training:
            if not all(torch.equal(B.bits(a), B.bits(b)) for a, b in zip(bwd[0], bwd[1])):
                failures.append("two backward launches differ")
            if not (torch.equal(B.bits(body(bwd[0][0])[cm]), B.bits(body(bwd[2][0])[cm])) and torch.equal(B.bits(bwd[0][1]), B.bits(bwd[2][1]))
                    and torch.equal(B.bits(bwd[0][2]), B.bits(bwd[2][2]))):
                failures.append("backward: the padding rows' contents reached dz, dbeta or dgamma")
            da, gba, gga = bwd[0]
            add_backward(eb, ref, da[G:G + rows, :cols].numpy()[cnt], gba[4:4 + cols].numpy(), gga[4:4 + cols].numpy())
    line = "bn_seq_ops %4d cols (Bp %2d, Bt %2d, T %3d) alpha %.1f %-7s fwd %s" % (cols, Bp, Bt, T, alpha, mode, ef.text())
    if training:
        line += " | bwd " + eb.text()
    print(line)
    bad = over_bound(ef) + over_bound(eb)
    assert not bad, bad
    assert not failures, sorted(set(failures))
    LINES.append(line)                                 # (passing cases only: test_zz_write_profile)


CASES = [(c, s, a, m) for c in COLS for s in SHAPES for a in ALPHAS for m in MODES]


@pytest.fixture(scope="module")
def eng():
    from rsrgan_amd.ops import OpEntries
    return OpEntries()


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    if _FAULTED:
        pytest.fail("not run: %s raised a HIP error earlier in this module" % _FAULTED[0])


@pytest.mark.gpu
@pytest.mark.parametrize("cols,shape,alpha,mode", CASES, ids=["%d-Bp%d.Bt%d.T%d-a%.1f-%s" % ((c,) + s + (a, m)) for c, s, a, m in CASES])
def test_bn_seq_ops(eng, cols, shape, alpha, mode):
    try:
        run_case(eng, cols, *shape, alpha, mode)
    except AssertionError:
        raise
    except Exception:                                    # a HIP error: nothing more is started on the GPU from this module
        _FAULTED.append("%d cols %s" % (cols, shape))
        raise


PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bn_seq_ops_errors.txt")
PROFILE_HEADER = """tests/test_gpu_bn_seq_ops.py on an MI355X (gfx950): rsrgan_op_bn_seq_forward / _backward (csrc/bn_seq.hip) against oracle/bn_renorm.py in
fp64 on the counted rows.  Per output: k = max |kernel - ref|, p = max |plain fp32 restatement - ref|, s = k / max(|ref|_max, 1).
Bound (unchanged from the sliced route of tests/test_gpu_bn_ops.py): max(|kernel - ref| - 4 ulp32(column max)) <= 4 x p.
Written by test_zz_write_profile at the end of a run in which all %d cases passed (`python -m pytest tests/test_gpu_bn_seq_ops.py -m gpu`).
"""


@pytest.mark.gpu
def test_zz_write_profile():
    """the achieved figures of a complete passing run go to profiles/bn_seq_ops_errors.txt; a partial run (-k, a node id, a failure)
    writes nothing"""
    if len(LINES) != len(CASES):
        print("bn_seq_ops partial run (%d of %d cases passed): profiles/bn_seq_ops_errors.txt is not written" % (len(LINES), len(CASES)))
        return
    with open(PROFILE, "w") as f:
        f.write(PROFILE_HEADER % len(CASES) + "\n".join(LINES) + "\n")


@pytest.mark.gpu
def test_padding_columns_come_out_zero_whatever_they_hold(eng):
    """y and dz in the columns [cols, pad4(cols)) are literal zeros, also where z and dy hold NaN there (beyond the operands' contract)"""
    import torch
    cols, Bp, Bt, T, alpha = 7, 32, 8, 2, 0.3
    rows, dev = n_rows(Bp, T), eng.device
    ref = build(cols, Bp, Bt, T, alpha, "random", 0)
    var_bufs = [B.dev_vector(ref["st"][n], dev) for n in B.VARS]
    _, zd = B.dev_matrix(ref["z"][None], 8, dev)
    _, yd = B.dev_fill(rows, 8, dev)
    _, sd = B.dev_stat(2, cols, 8, dev)
    clean = zd.clone()
    zd[:, cols:] = float("nan")
    eng.op_bn_seq_forward(zd, yd, rows, cols, [b[1] for b in var_bufs], sd, B.dev_scratch(64 * cols, dev), alpha=alpha, Bp=Bp, Bt=Bt)
    _, y2 = B.dev_fill(rows, 8, dev)
    _, s2 = B.dev_stat(2, cols, 8, dev)
    eng.op_bn_seq_forward(clean, y2, rows, cols, [b[1] for b in var_bufs], s2, B.dev_scratch(64 * cols, dev), alpha=alpha, Bp=Bp, Bt=Bt)
    torch.cuda.synchronize()
    assert torch.equal(B.bits(yd.cpu()), B.bits(y2.cpu())) and torch.equal(B.bits(sd.cpu()), B.bits(s2.cpu()))
    assert bool((B.bits(yd[:, cols:].cpu()) == 0).all())
    _, dd_ = B.dev_matrix(ref["dy"][None], 8, dev)
    dd_[:, cols:] = float("nan")
    sums = torch.full((2 * 8 + 64,), B.SENT, dtype=torch.float32, device=dev)
    eng.op_bn_seq_backward(dd_, yd, zd, rows, cols, sd, sums, B.dev_scratch(64 * cols, dev), alpha=alpha, Bp=Bp, Bt=Bt)
    torch.cuda.synchronize()
    out = dd_.cpu()
    assert bool((B.bits(out[:, cols:]) == 0).all()) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("cols", COLS)
def test_wrong_n_misses_the_bound(cols):
    """host only: the expected values recomputed with n = T.Bp instead of T.Bt, held against the reference as a kernel's output would be"""
    for Bp, Bt, T in SHAPES:
        if Bp == 0 or Bt == Bp:
            continue
        worst = 0.0
        for alpha in ALPHAS:
            e = B.Errors()
            for w in range((16 + cols - 1) // cols):
                ref, wrong = build(cols, Bp, Bt, T, alpha, "random", w), build(cols, Bp, Bt, T, alpha, "random", w, n_wrong=True)
                add_forward(e, ref, wrong["y_pl"], wrong["stat_pl"], True)
                add_backward(e, ref, wrong["dz_pl"], wrong["dbeta_pl"], wrong["dgamma_pl"])
            margin = max([m for _, m, _, _ in over_bound(e)] or [0.0])
            print("bn_seq_ops wrong-n %4d cols (Bp %d, Bt %d, T %d) alpha %.1f: misses the bound %.1f x" % (cols, Bp, Bt, T, alpha, margin))
            worst = max(worst, margin)
            assert margin >= 10.0, (cols, Bp, Bt, T, alpha, margin)
