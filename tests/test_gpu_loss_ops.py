"""The loss kernels and the element-wise kernels at the end of a step (csrc/kernels.hip: k_lsgan, k_dhead1 / k_dhead2, k_mse1 / k_mse2,
k_g_total, k_dropout_fwd / _bwd, k_lrelu_bwd), each through the launch_* function the model calls (rsrgan_op_step_elem) against fp64
numpy computed from the same fp32-rounded inputs.  The references restate the reference project's graph:
models/gan_rnn_placeholder.py:244-260 (d_rl_loss = mean((D(real) - d_real)^2), d_fk_loss = mean((D(fake) - d_fake)^2), g_mse_loss =
0.5 * mean((g - labels)^2) * output_dim, g_loss = adv + lambda * mse + l2), models/discriminator_lstm.py:93-104 (one fully connected
logit per frame), models/discriminator_dnn.py:93 (tf.clip_by_value(y, -0.5, 1.5): the gradient passes where lo <= y <= hi),
models/dnn.py:116-121 (tf.nn.dropout: x / keep * mask) and tf.nn.leaky_relu's derivative (alpha where the activation is not positive).

The (Bp, Bt) rule of a row-padded model: every Bp rows of a frame's half are Bt utterances and Bp - Bt padding rows, which count in no
mean and get a zero gradient.  The padding rows here hold finite junk of magnitude 1e3 that would move any mean that counted them.

Output buffers are pre-filled with a sentinel: padding columns [cols, ld), columns 1 .. 3 of the ld = 4 logit and weight buffers and guard
rows behind the last row must come back bit-unchanged; input padding columns hold NaN where the kernel must not read them.  Every launch
runs twice from fresh buffers and must give bit-identical results.  Bounds: tests/update_ref.py (4 x the plain-order fp32 error, floored at
2 ulp); per-element outputs (dlogits, dout, dy, gw) on the scale max(|ref|, scale x 2^-20) with scale = max |ref| of that output, scalars
(losses, gb, logits' figure: see there) relative.  Each case prints both errors ("loss_ops" lines)."""
import numpy as np
import pytest

from tests.helpers import mask_of_key
from tests.update_ref import SENT, bits_equal, dev, elem_err, f32, f64, host, rel_err, rng, seqsum32, twice
from tests.update_ref import bounded as _bounded

pytestmark = pytest.mark.gpu

GUARD = 3                              # sentinel rows behind the last row
T_REAL, T_FAKE = f32(0.9), f32(-0.7)   # the two targets differ
# k_dhead forms its logits itself, as a dot product whose rounding error does not shrink with the result.  Where logit - target nearly
# cancels, the per-element figure of dlogits / dout is that one element's rounding luck, in the kernel's FMA order as much as in the
# CPU's plain one, and says nothing about either.  So the head's inputs are positive (logits in about [0.3, 1.4]) and both targets lie
# above the logits' range: no difference cancels, dlogits has one sign so that the sums gw and gb do not cancel either, and the figures
# measure the arithmetic.
DH_T_REAL, DH_T_FAKE = f32(2.0), f32(3.0)


@pytest.fixture(scope="module")
def eng():
    from rsrgan_amd.ops import OpEntries
    return OpEntries()


def bounded(case, name, k, p):
    _bounded("loss_ops", case, name, k, p)


def matrix(vals, ld, fill, guard=GUARD):
    """[rows + guard][ld] fp32: vals in the leading columns, `fill` in the padding columns and the guard rows"""
    rows, cols = vals.shape
    buf = np.full((rows + guard, ld), fill, dtype=f32)
    buf[:rows, :cols] = vals
    return buf


def frame_unchanged(got, before, rows, cols):
    """everything outside [0, rows) x [0, cols) is bit-unchanged"""
    a, b = got.copy(), before.copy()
    a[:rows, :cols] = 0.0
    b[:rows, :cols] = 0.0
    return bits_equal(a, b)


def row_rule(T, Nd, n_real, Bp, Bt):
    """real[r], valid[r] and the two counts of the T * Nd rows: row r is entry r % Nd of frame r // Nd"""
    j = np.arange(T * Nd) % Nd
    real = j < n_real
    valid = np.ones(T * Nd, dtype=bool) if Bp == 0 else (j % Bp) < Bt
    return real, valid, int((real & valid).sum()), int((~real & valid).sum())


def lsgan_ref(logit, real, valid, cr, cf, T, lo=None, hi=None, t_real=T_REAL, t_fake=T_FAKE):
    """T = f64: the reference; T = f32: the same formulas in fp32, sums in row order.  -> loss3, dlogits"""
    raw = logit.astype(T)
    val = raw if lo is None else np.minimum(np.maximum(raw, T(lo)), T(hi))
    tgt = np.where(real, T(t_real), T(t_fake)).astype(T)
    d = np.where(valid, val - tgt, T(0.0)).astype(T)
    cnt = np.where(real, T(max(cr, 1)), T(max(cf, 1))).astype(T)
    dl = (T(2.0) * d / cnt).astype(T)
    if lo is not None:
        dl = np.where((raw < T(lo)) | (raw > T(hi)), T(0.0), dl).astype(T)
    sq = (d * d).astype(T)
    if T is f64:
        sr, sf = sq[real].sum(), sq[~real].sum()
    else:
        sr, sf = seqsum32(sq[real]), seqsum32(sq[~real])
    lr = sr / T(cr) if cr > 0 else T(0.0)
    lf = sf / T(cf) if cf > 0 else T(0.0)
    return np.array([lr, lf, lr + lf], dtype=T), dl


# ---------------------------------------------------------------------------------------------------------------------- k_lsgan
LSGAN_SHAPES = {5: (1, 5, 5, 3), 1000: (125, 8, 4, 3), 2500: (125, 20, 10, 7)}         # rows: T, Nd, Bp, Bt


@pytest.mark.parametrize("mode", ["plain", "pad", "clip", "pad_clip", "no_grad"])
@pytest.mark.parametrize("rows", sorted(LSGAN_SHAPES))
def test_lsgan(eng, rows, mode):
    T, Nd, Bp, Bt = LSGAN_SHAPES[rows]
    pad, clip = "pad" in mode, "clip" in mode
    if not pad:
        Bp = Bt = 0
    lo, hi = (f32(-0.5), f32(1.5)) if clip else (None, None)
    for n_real in (0, Nd, Nd // 2):
        if pad and n_real % Bp:
            continue                                         # (a half is whole blocks of Bp rows: the entry refuses anything else)
        real, valid, cr, cf = row_rule(T, Nd, n_real, Bp, Bt)
        logit = (rng(50, rows, n_real).standard_normal(rows) * 1.5 + 0.5).astype(f32)
        logit[~valid] = (rng(51, rows).choice([-1.0, 1.0], rows) * rng(52, rows).uniform(1e3, 2e3, rows)).astype(f32)[~valid]
        v = np.flatnonzero(valid)
        if clip:                                             # exactly lo, exactly hi, below lo, above hi -- on rows that count
            edge = [lo, hi, f32(-0.75), f32(2.25)]
            for k, r in enumerate(v[:4] if rows == 5 else np.concatenate([v[:4], v[-4:]])):
                logit[r] = edge[k % 4]
        l64, d64 = lsgan_ref(logit, real, valid, cr, cf, f64, lo, hi)
        l32, d32 = lsgan_ref(logit, real, valid, cr, cf, f32, lo, hi)
        lg0 = matrix(logit[:, None], 4, np.nan)
        dl0 = matrix(np.full((rows, 1), SENT, dtype=f32), 4, SENT)
        tg = np.array([T_REAL, T_FAKE], dtype=f32)

        def run():
            ld_, dd, td, od = dev(lg0, eng), dev(dl0, eng), dev(tg, eng), dev(np.full(8, SENT, dtype=f32), eng)
            eng.op_step_elem("lsgan", [ld_, None if mode == "no_grad" else dd, td[0:], td[1:], od],
                             [T, Nd, n_real, 4, 1 if clip else 0, Bp, Bt], [lo if clip else 0.0, hi if clip else 0.0])
            return {"dl": host(dd), "loss": host(od), "logits": host(ld_)}
        out = twice(run)
        case = "lsgan rows=%d n_real=%d %s" % (rows, n_real, mode)
        assert bits_equal(out["logits"], lg0) and np.all(out["loss"][3:] == SENT)
        bounded(case, "loss3", rel_err(out["loss"][:3], l64), rel_err(l32, l64))
        if mode == "no_grad":
            assert bits_equal(out["dl"], dl0)
            continue
        assert frame_unchanged(out["dl"], dl0, rows, 1)
        got = out["dl"][:rows, 0]
        assert not np.any(got[~valid]) and not np.any(np.signbit(got[~valid])), "a padding row's gradient is not +0"
        if clip:
            outside = (logit < lo) | (logit > hi)
            at_edge = valid & ((logit == lo) | (logit == hi))
            assert outside[valid].any() and at_edge.sum() >= 2
            assert not np.any(got[outside]), "gradient outside the clip bounds"
            assert np.all(got[at_edge] != 0.0), "no gradient where the logit equals a bound"
        bounded(case, "dlogits", elem_err([got], [d64]), elem_err([d32], [d64]))


# ---------------------------------------------------------------------------------------------------------------------- k_dhead1 / k_dhead2
DHEAD_SHAPES = {5: (1, 5, 2, (5, 3, 0)), 64: (8, 8, 4, (4, 3, 4)), 64 * 17 + 5: (1, 64 * 17 + 5, 546, (64 * 17 + 5, 700, 64 * 17 + 5))}
#               rows: T, Nd, n_real, (Bp, Bt, n_real of the padded case)


def dhead_ref(top, w, b, real, valid, cr, cf, T):
    """-> logits, loss3, dlogits, dout, gw, gb; T = f32: every sum in plain order (columns, then rows)"""
    x, wv = top.astype(T), w.astype(T)
    if T is f64:
        logit = x @ wv + T(b)
    else:
        logit = np.full(x.shape[0], T(b), dtype=T)
        for c in range(x.shape[1]):
            logit = logit + x[:, c] * wv[c]
    l3, dl = lsgan_ref(logit, real, valid, cr, cf, T, t_real=DH_T_REAL, t_fake=DH_T_FAKE)
    dout = (dl[:, None] * wv[None, :]).astype(T)
    prod = (x * dl[:, None]).astype(T)
    if T is f64:
        gw, gb = prod.sum(0), dl.sum()
    else:
        gw, gb = np.cumsum(prod, axis=0, dtype=T)[-1], seqsum32(dl)
    return logit, l3, dl, dout, gw, gb


@pytest.mark.parametrize("rows", sorted(DHEAD_SHAPES))
@pytest.mark.parametrize("dR", [4, 40, 60])
def test_dhead(eng, dR, rows):
    """rows = 64 x 17 + 5: 18 blocks of partials, not a multiple of the 16 lanes k_dhead2 strides over"""
    T, Nd, n_real0, padded = DHEAD_SHAPES[rows]
    ldt, ldo = dR + 4, dR + 8
    for pad in (False, True):
        Bp, Bt, n_real = padded if pad else (0, 0, n_real0)
        real, valid, cr, cf = row_rule(T, Nd, n_real, Bp, Bt)
        top = rng(60, dR, rows, pad).uniform(0.25, 1.25, (rows, dR)).astype(f32)
        top[~valid] *= f32(1e3)                              # junk on the padding rows
        w = (rng(61, dR, rows).uniform(0.5, 1.5, dR) / dR).astype(f32)
        b = f32(0.05)
        r64, r32 = dhead_ref(top, w, b, real, valid, cr, cf, f64), dhead_ref(top, w, b, real, valid, cr, cf, f32)
        top0, w0 = matrix(top, ldt, np.nan), matrix(w[:, None], 4, np.nan, guard=0)
        lg0 = matrix(np.full((rows, 1), SENT, dtype=f32), 4, SENT)
        do0 = matrix(np.full((rows, dR), SENT, dtype=f32), ldo, SENT)
        gw0 = matrix(np.full((dR, 1), SENT, dtype=f32), 4, SENT)
        nblk = (rows + 63) // 64
        for want_g in (0, 1):
            for want_w in (0, 1):
                def run():
                    bufs = {"top": dev(top0, eng), "w": dev(w0, eng), "b": dev(np.array([b, np.nan], dtype=f32), eng), "logits": dev(lg0, eng),
                            "dl": dev(lg0, eng), "dout": dev(do0, eng), "gw": dev(gw0, eng), "gb": dev(np.full(4, SENT, dtype=f32), eng),
                            "tg": dev(np.array([DH_T_REAL, DH_T_FAKE], dtype=f32), eng), "loss": dev(np.full(8, SENT, dtype=f32), eng),
                            "part": dev(np.full(nblk * 67, np.nan, dtype=f32), eng)}
                    # every output buffer is handed over whatever the flags say, as Model::d_head does (its G-run passes the
                    # discriminator's live gradient buffers with want_wgrads = 0): the flags alone keep a switched-off output untouched
                    eng.op_step_elem("dhead", [bufs["top"], bufs["w"], bufs["b"], bufs["logits"], bufs["dl"], bufs["dout"], bufs["gw"], bufs["gb"],
                                               bufs["tg"][0:], bufs["tg"][1:], bufs["loss"], bufs["part"]],
                                     [T, Nd, n_real, dR, ldt, 4, 4, ldo, want_g, want_w, Bp, Bt, nblk * 67])
                    return {k: host(v) for k, v in bufs.items() if k != "part"}
                out = twice(run)
                case = "dhead dR=%d rows=%d pad=%d g=%d w=%d" % (dR, rows, pad, want_g, want_w)
                assert bits_equal(out["top"], top0) and bits_equal(out["w"], w0)
                assert frame_unchanged(out["logits"], lg0, rows, 1) and np.all(out["loss"][3:] == SENT)
                bounded(case, "logits", elem_err([out["logits"][:rows, 0]], [r64[0]]), elem_err([r32[0]], [r64[0]]))
                bounded(case, "loss3", rel_err(out["loss"][:3], r64[1]), rel_err(r32[1], r64[1]))
                if want_g:
                    assert frame_unchanged(out["dl"], lg0, rows, 1) and frame_unchanged(out["dout"], do0, rows, dR)
                    gdl, gdo = out["dl"][:rows, 0], out["dout"][:rows, :dR]
                    assert not np.any(gdl[~valid]) and not np.any(gdo[~valid]), "a padding row's gradient is not 0"
                    bounded(case, "dlogits", elem_err([gdl], [r64[2]]), elem_err([r32[2]], [r64[2]]))
                    bounded(case, "dout", elem_err([gdo], [r64[3]]), elem_err([r32[3]], [r64[3]]))
                else:                                        # switched off: untouched
                    assert bits_equal(out["dl"], lg0) and bits_equal(out["dout"], do0)
                if want_w:
                    assert frame_unchanged(out["gw"], gw0, dR, 1) and np.all(out["gb"][1:] == SENT)
                    bounded(case, "gw", elem_err([out["gw"][:dR, 0]], [r64[4]]), elem_err([r32[4]], [r64[4]]))
                    bounded(case, "gb", rel_err(out["gb"][:1], [r64[5]]), rel_err([r32[5]], [r64[5]]))
                else:
                    assert bits_equal(out["gw"], gw0) and np.all(out["gb"] == SENT)


# ---------------------------------------------------------------------------------------------------------------------- k_mse1 / k_mse2 / k_g_total
def mse_ref(y, lab, dy0, valid, n_eff, lam, acc, T):
    d = np.where(valid[:, None], y.astype(T) - lab.astype(T), T(0.0)).astype(T)
    sq = (d * d).astype(T)
    s = sq.sum() if T is f64 else seqsum32(sq)
    loss = T(0.5) * s / T(n_eff)
    scale = T(lam) / T(n_eff)
    dy = ((dy0.astype(T) if acc else T(0.0)) + scale * d).astype(T)
    return loss, dy


@pytest.mark.parametrize("mode", ["plain", "accumulate", "pad", "pad_accumulate", "no_dy"])
@pytest.mark.parametrize("shape", [(3, 5, 8, 3, 2), (264, 257, 260, 8, 5)], ids=["3x5", "264x257"])
def test_mse_and_g_total(eng, shape, mode):
    """264 x 257 = 67848 elements: more than the 256 x 256 threads of the launch, so the grid strides; lambda is read from device memory"""
    rows, D, ld, Bp, Bt = shape
    acc, pad = "accumulate" in mode, "pad" in mode
    if not pad:
        Bp = Bt = 0
    valid = np.ones(rows, dtype=bool) if not pad else (np.arange(rows) % Bp) < Bt
    n_eff = int(valid.sum())
    lam = f32(0.37)
    y = rng(70, rows).standard_normal((rows, D)).astype(f32)
    lab = rng(71, rows).standard_normal((rows, D)).astype(f32)
    y[~valid] = f32(1e3)
    lab[~valid] = f32(-1e3)
    dy_prev = rng(72, rows).standard_normal((rows, D)).astype(f32)
    (l64, d64), (l32, d32) = mse_ref(y, lab, dy_prev, valid, n_eff, lam, acc, f64), mse_ref(y, lab, dy_prev, valid, n_eff, lam, acc, f32)
    y0, lab0, dy0 = matrix(y, ld, np.nan), matrix(lab, ld, np.nan), matrix(dy_prev, ld, SENT)
    adv, l2 = f32(0.8125), f32(0.046875)
    l4_0 = np.array([adv, SENT, l2, SENT, SENT], dtype=f32)

    def run():
        yd, ld_, dd, lamd = dev(y0, eng), dev(lab0, eng), dev(dy0, eng), dev(np.array([lam], dtype=f32), eng)
        l4, sc = dev(l4_0, eng), dev(np.full(1024, np.nan, dtype=f32), eng)
        eng.op_step_elem("mse", [yd, ld_, None if mode == "no_dy" else dd, lamd, l4[1:], sc], [rows, D, ld, 1 if acc else 0, Bp, Bt, 1024])
        eng.op_step_elem("g_total", [l4, lamd])
        return {"y": host(yd), "lab": host(ld_), "dy": host(dd), "l4": host(l4)}
    out = twice(run)
    case = "mse %dx%d %s" % (rows, D, mode)
    assert bits_equal(out["y"], y0) and bits_equal(out["lab"], lab0)
    l4 = out["l4"]
    assert l4[0] == adv and l4[2] == l2 and l4[4] == SENT
    bounded(case, "mse", rel_err([l4[1]], [l64]), rel_err([l32], [l64]))
    # losses[3] = adv + lambda * mse + l2, from the mse the launch left in l4[1]
    tot64 = f64(adv) + f64(lam) * f64(l4[1]) + f64(l2)
    bounded(case, "total", rel_err([l4[3]], [tot64]), rel_err([adv + lam * l4[1] + l2], [tot64]))
    if mode == "no_dy":
        assert bits_equal(out["dy"], dy0)
        return
    assert frame_unchanged(out["dy"], dy0, rows, D)
    got = out["dy"][:rows, :D]
    if pad:
        assert bits_equal(got[~valid], dy_prev[~valid] if acc else np.zeros_like(got[~valid])), "a padding row's gradient is not 0"
    bounded(case, "dy", elem_err([got], [d64]), elem_err([d32], [d64]))


# ---------------------------------------------------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("keep", [0.8, 1.0, 0.01])
@pytest.mark.parametrize("shape", [(3, 5, 8), (2100, 1000, 1004)], ids=["3x5", "2100x1000"])
def test_dropout(eng, shape, keep):
    """2100 x 1000 elements: more than the 8192 x 256 threads of the capped grid.  The mask is the host mirror's (tests/helpers.py) for the
    key the test passes; kept values are bit-equal to fp32 x / keep, dropped ones are +0; the backward reads the mask back from y > 0"""
    rows, cols, ld = shape
    key = 0xC0FFEE1234567890 ^ (rows * 0x9E3779B97F4A7C15 & 0xFFFFFFFFFFFFFFFF)
    k32 = f32(keep)
    thr = int(float(k32) * 16777216.0)
    mask = mask_of_key(key, rows, cols, keep) > 0
    assert keep == 1.0 and mask.all() or keep < 1.0 and abs(mask.mean() - keep) < 0.02 + 1.0 / np.sqrt(mask.size)
    x = np.abs(rng(80, rows).standard_normal((rows, cols))).astype(f32) + f32(0.01)       # non-negative: a ReLU's output
    d = rng(81, rows).standard_normal((rows, cols)).astype(f32)
    x0, d0 = matrix(x, ld, SENT), matrix(d, ld, SENT)

    def run():
        yd, dd = dev(x0, eng), dev(d0, eng)
        eng.op_step_elem("dropout_fwd", [yd], [rows, cols, ld, key, thr], [k32])
        out = {"y": host(yd).copy()}
        eng.op_step_elem("dropout_bwd", [yd, dd], [rows, cols, ld], [k32])
        out["d"], out["y2"] = host(dd), host(yd)
        return out
    out = twice(run)
    assert frame_unchanged(out["y"], x0, rows, cols) and frame_unchanged(out["d"], d0, rows, cols) and bits_equal(out["y"], out["y2"])
    y, dg = out["y"][:rows, :cols], out["d"][:rows, :cols]
    assert np.array_equal(y != 0.0, mask), "the mask is not the host mirror's"
    assert bits_equal(y, np.where(mask, x / k32, f32(0.0)))
    assert bits_equal(dg, np.where(mask, d / k32, f32(0.0)))
    print("loss_ops dropout %dx%d keep=%.2f: %d of %d kept, forward and backward bit-equal" % (rows, cols, keep, int(mask.sum()), mask.size))


# ---------------------------------------------------------------------------------------------------------------------- k_lrelu_bwd
@pytest.mark.parametrize("alpha", [0.3, 0.0])
@pytest.mark.parametrize("shape", [(3, 5, 8), (700, 760, 764)], ids=["3x5", "700x760"])
def test_lrelu_bwd(eng, shape, alpha):
    """d *= alpha where h is not positive (h == 0 included), one fp32 multiply; 700 x 760 elements: more than the 2048 x 256 threads"""
    rows, cols, ld = shape
    h = rng(90, rows).standard_normal((rows, cols)).astype(f32)
    h[rng(91, rows).random((rows, cols)) < 0.2] = 0.0
    h[0, 0], h[-1, -1] = 0.0, -0.0
    d = rng(92, rows).standard_normal((rows, cols)).astype(f32)
    h0, d0 = matrix(h, ld, np.nan), matrix(d, ld, SENT)

    def run():
        hd, dd = dev(h0, eng), dev(d0, eng)
        eng.op_step_elem("lrelu_bwd", [hd, dd], [rows, cols, ld], [alpha])
        return {"h": host(hd), "d": host(dd)}
    out = twice(run)
    assert bits_equal(out["h"], h0) and frame_unchanged(out["d"], d0, rows, cols)
    want = np.where(h > 0, d, d * f32(alpha))
    assert bits_equal(out["d"][:rows, :cols], want)
    assert bits_equal(out["d"][0, 0], d[0, 0] * f32(alpha))
    print("loss_ops lrelu_bwd %dx%d alpha=%.1f: bit-equal, %d entries with h == 0" % (rows, cols, alpha, int((h == 0).sum())))
