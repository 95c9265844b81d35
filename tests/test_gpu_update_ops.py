"""The end of every training step, kernel by kernel: the chunked kernels of csrc/kernels.hip (k_sumsq, k_dw_reduce, k_l2, k_l2_total,
the per-tensor clip_by_norm inside k_apply_sgd / k_apply_adam, k_adam_tick), each through the launch_* function the model calls
(rsrgan_op_update, rsrgan_op_step_elem) and with the chunk table the model's own host code builds (rsrgan_op_chunks), against fp64
numpy computed from the same fp32-rounded inputs.  The references restate models/gan_rnn_placeholder.py:144-186 (GradientDescent, Adam
in TensorFlow's form -- lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), w -= lr_t m / (sqrt(v) + eps) --, tf.clip_by_norm = g clip / max(|g|, clip),
ExponentialMovingAverage) and :252-256 (tf.nn.l2_loss = sum(v^2) / 2 over the variables without "bias" in their name).

One tensor table serves all of them: 4, 4092, 4096, 4100, 3 x 4096 + 8, 257 x 4096 + 12 and 40 floats (1, 1, 1, 2, 4, 258, 1 chunks: short tail
chunks, several chunks per tensor, and more chunks than the 256 threads that sum a tensor's partials), every tensor at a multiple of 64
floats as ParamSet::add places them, l2 flags alternating.  The gaps between tensors and a guard band behind the last one hold a sentinel
in every output buffer and NaN in every input buffer; outputs must come back bit-unchanged there.  Every sequence of launches runs twice
from fresh buffers and must give bit-identical results.

Bounds (the rule of tests/test_gpu_wgrad_ops.py's column sums): 4 x the error of the same quantity evaluated in fp32 on the CPU in plain
order with the same formula, both against fp64 in the same metric -- the factor covers summation order and FMA contraction only --,
floored at 2 ulp (2^-22 relative) where the CPU's fp32 happens to be exact.  Per-element outputs (w, m, v, ema, g): max over elements of
|got - ref| / max(|ref|, scale x 2^-20), scale = max |ref| over the table tensor the element belongs to; every tensor is held to its own
bound.  Sums (partial, the L2 total): |got - ref| / |ref|.  Each case prints both errors ("update_ops" lines)."""
import numpy as np
import pytest

from rsrgan_amd._lib import DYN_COUNT, DYN_SLOTS
from tests.update_ref import SENT, ULP2, bits_equal, dev, elem_err, f32, f64, host, rel_err, rng, twice
from tests.update_ref import bounded as _bounded

pytestmark = pytest.mark.gpu

PRE = "update_ops"
CH = 4096
SIZES = [4, 4092, 4096, 4100, 3 * 4096 + 8, 257 * 4096 + 12, 40]
GUARD = 64


@pytest.fixture(scope="module")
def eng():
    from rsrgan_amd.ops import OpEntries
    return OpEntries()


def make_table(sizes):
    tensors, off = [], 0
    for i, n in enumerate(sizes):
        tensors.append((off, n, (i + 1) % 2))
        off += (n + 63) // 64 * 64
    return tensors, off + GUARD


TENSORS, TOTAL = make_table(SIZES)


def own_chunks(tensors):
    """(tensor, offset, length) of every chunk, written out here: tensor order, 4096 floats, a short tail"""
    return [(i, o + c, min(CH, n - c)) for i, (o, n, _) in enumerate(tensors) for c in range(0, n, CH)]


CHUNKS = own_chunks(TENSORS)
NC = len(CHUNKS)


def flat(parts, fill, tensors=TENSORS, total=TOTAL):
    """the flat buffer: tensor i = parts[i], `fill` everywhere else"""
    buf = np.full(total, fill, dtype=f32)
    for (o, n, _), p in zip(tensors, parts):
        buf[o:o + n] = p
    return buf


def parts_of(buf, tensors=TENSORS):
    return [buf[o:o + n] for o, n, _ in tensors]


def gaps_unchanged(got, before, tensors=TENSORS):
    mask = np.ones(got.shape[0], dtype=bool)
    for o, n, _ in tensors:
        mask[o:o + n] = False
    return np.array_equal(got[mask].view(np.uint32), before[mask].view(np.uint32))


def bounded(case, name, k, p):
    _bounded(PRE, case, name, k, p)


def bounded_each(case, name, got, r32, r64):
    """a per-element output, tensor by tensor of the table: each against its own plain-order fp32 error"""
    figs = [(elem_err([a], [c]), elem_err([b], [c])) for a, b, c in zip(got, r32, r64)]
    if len(figs) > 16:                  # a long table: every tensor is held to its bound, the one nearest its bound is printed
        for t, (k, p) in enumerate(figs):
            assert k <= max(4.0 * p, ULP2), (case, "%s[%d]" % (name, t), k, p)
        t = max(range(len(figs)), key=lambda i: figs[i][0] / max(4.0 * figs[i][1], ULP2))
        figs = {t: figs[t]}
    else:
        figs = dict(enumerate(figs))
    for t, (k, p) in figs.items():
        _bounded(PRE, case, "%s[%d]" % (name, t), k, p)


def sumsq_refs(parts, chunks=CHUNKS, tensors=TENSORS):
    """per chunk: fp64 sum of squares, and the same sum accumulated in fp32 in plain order"""
    r64, r32 = [], []
    for t, o, n in chunks:
        x = parts[t][o - tensors[t][0]:o - tensors[t][0] + n]
        r64.append(float((x.astype(f64) ** 2).sum()))
        r32.append(float(np.cumsum(x * x, dtype=f32)[-1]))
    return np.array(r64), np.array(r32)


# ---------------------------------------------------------------------------------------------------------------------- the table
def test_table_is_the_models(eng):
    t = eng.op_chunks(TENSORS)
    assert NC == 268 and [c for c in t["t_count"]] == [1, 1, 1, 2, 4, 258, 1]
    assert list(zip(t["tensor"], t["off"], t["len"])) == CHUNKS                 # the number of chunks and their order
    assert t["t_l2"] == [l2 for _, _, l2 in TENSORS]
    assert t["t_first"] == [min(i for i, c in enumerate(CHUNKS) if c[0] == k) for k in range(len(TENSORS))]


# ---------------------------------------------------------------------------------------------------------------------- k_sumsq
def test_sumsq(eng):
    parts = [rng(1, i).standard_normal(n).astype(f32) * f32(0.5 + i) for i, n in enumerate(SIZES)]
    g = flat(parts, np.nan)
    r64, r32 = sumsq_refs(parts)

    def run():
        gd, pd = dev(g, eng), dev(np.full(NC + 8, SENT, dtype=f32), eng)
        eng.op_update("sumsq", TENSORS, [gd, pd], TOTAL, NC + 8)
        return {"partial": host(pd), "g": host(gd)}
    out = twice(run)
    assert bits_equal(out["g"], g)
    assert np.all(out["partial"][NC:] == SENT), "partial written beyond the chunks"
    bounded("sumsq", "partial", rel_err(out["partial"][:NC], r64), rel_err(r32, r64))


# ---------------------------------------------------------------------------------------------------------------------- k_dw_reduce
@pytest.mark.parametrize("ntiles", [1, 2, 5])
def test_dw_reduce(eng, ntiles):
    """records in an order of their own (tensors 6, 4, 3, 2, 1; 4 NaN floats between them), a stride 100 floats beyond the record; tensors 0
    and 5 (258 chunks) were not computed by the launch: src = -1"""
    src, at = [-1] * len(SIZES), 0
    for t in (6, 4, 3, 2, 1):
        src[t] = at
        at += SIZES[t] + 4
    stride = at + 100
    ws = np.full(ntiles * stride, np.nan, dtype=f32)
    for t in (6, 4, 3, 2, 1):
        for r in range(ntiles):
            ws[r * stride + src[t]:r * stride + src[t] + SIZES[t]] = rng(2, ntiles, t, r).standard_normal(SIZES[t]).astype(f32)
    old = [rng(3, i).standard_normal(n).astype(f32) for i, n in enumerate(SIZES)]
    g0 = flat(old, SENT)
    want = []
    for t, n in enumerate(SIZES):
        if src[t] < 0:
            want.append(old[t])
            continue
        acc = ws[src[t]:src[t] + n].copy()                       # fp32 additions in tile order: nothing can contract
        for r in range(1, ntiles):
            acc += ws[r * stride + src[t]:r * stride + src[t] + n]
        want.append(acc)
    r64, r32 = sumsq_refs(want)

    def run():
        wd, gd, pd = dev(ws, eng), dev(g0, eng), dev(np.full(NC + 8, SENT, dtype=f32), eng)
        eng.op_update("dw_reduce", TENSORS, [wd, gd, pd], TOTAL, NC + 8, extra=(stride, ntiles, ws.shape[0]), src=src)
        return {"g": host(gd), "partial": host(pd), "ws": host(wd)}
    out = twice(run)
    assert bits_equal(out["ws"], ws)
    assert gaps_unchanged(out["g"], g0)
    for t, (got, w) in enumerate(zip(parts_of(out["g"]), want)):
        assert bits_equal(got, w), "tensor %d (src %d)" % (t, src[t])
    assert np.all(out["partial"][NC:] == SENT)
    bounded("dw_reduce ntiles=%d" % ntiles, "partial", rel_err(out["partial"][:NC], r64), rel_err(r32, r64))


# ---------------------------------------------------------------------------------------------------------------------- k_l2, k_l2_total
def l2_case(eng, case, tensors, total, seed):
    sizes = [n for _, n, _ in tensors]
    chunks = own_chunks(tensors)
    nc = len(chunks)
    w = [rng(seed, i).standard_normal(n).astype(f32) for i, n in enumerate(sizes)]
    g = [rng(seed + 1, i).standard_normal(n).astype(f32) for i, n in enumerate(sizes)]
    scale = f32(1.0e-3)
    w0, g0 = flat(w, np.nan, tensors, total), flat(g, SENT, tensors, total)

    def run():
        wd, gd, sd = dev(w0, eng), dev(g0, eng), dev(np.array([scale], dtype=f32), eng)
        pd, od = dev(np.full(nc + 8, SENT, dtype=f32), eng), dev(np.full(4, SENT, dtype=f32), eng)
        eng.op_update("l2", tensors, [wd, gd, sd, pd], total, nc + 8)
        eng.op_step_elem("l2_total", [pd, sd, od], [nc])
        return {"g": host(gd), "partial": host(pd), "out": host(od), "w": host(wd)}
    out = twice(run)
    assert bits_equal(out["w"], w0) and gaps_unchanged(out["g"], g0, tensors)
    assert np.all(out["partial"][nc:] == SENT) and np.all(out["out"][1:] == SENT)
    got = parts_of(out["g"], tensors)
    on = [i for i, (_, _, l2) in enumerate(tensors) if l2]
    for i, (_, _, l2) in enumerate(tensors):
        if not l2:
            assert bits_equal(got[i], g[i]), "unflagged tensor %d changed" % i
    for c, (t, _, _) in enumerate(chunks):
        if not tensors[t][2]:
            assert out["partial"][c] == 0.0 and not np.signbit(out["partial"][c])
    ref_g = [g[i].astype(f64) + f64(scale) * w[i].astype(f64) for i in on]
    bounded_each(case, "g", [got[i] for i in on], [g[i] + scale * w[i] for i in on], ref_g)
    r64, r32 = sumsq_refs(w, chunks, tensors)
    flagged = np.array([tensors[t][2] == 1 for t, _, _ in chunks])
    bounded(case, "partial", rel_err(out["partial"][:nc][flagged], r64[flagged]), rel_err(r32[flagged], r64[flagged]))
    allw = np.concatenate([w[i] for i in on])
    ref_total = 0.5 * f64(scale) * float((allw.astype(f64) ** 2).sum())
    total32 = f32(0.5) * scale * np.cumsum(allw * allw, dtype=f32)[-1]
    bounded(case, "total", rel_err(out["out"][:1], [ref_total]), rel_err([total32], [ref_total]))


def test_l2_main_table(eng):
    l2_case(eng, "l2 main table", TENSORS, TOTAL, 10)


def test_l2_total_1100_chunks(eng):
    """k_l2_total's single block of 1024 threads over more than 1024 partials: 1100 one-chunk tensors of 4 .. 64 floats"""
    tensors, total = make_table([4 * (1 + i % 16) for i in range(1100)])
    l2_case(eng, "l2 1100 chunks", tensors, total, 20)


# ---------------------------------------------------------------------------------------------------------------------- clip + updates
FACTORS = [[2.0, 0.5, 0.0, 100.0, 0.5, 2.0, 100.0],      # |g| / clip of every tensor, round by round; tensor 5 (258 chunks) always clipped
           [0.5, 0.5, 100.0, 0.0, 2.0, 100.0, 2.0],
           [0.0, 0.5, 0.5, 2.0, 100.0, 2.0, 0.0]]
BIG = 5                                                   # the 258-chunk tensor
BIG_SHARES = ((0, 256 * CH, 0.01), (256 * CH, 257 * CH, 0.66), (257 * CH, SIZES[5], 0.33))      # of |g|^2: chunks 0 .. 255, chunk 256, the 12-float chunk 257
TINY = 1                                                  # the tensor whose gradients lie in [1e-9, 1e-7] in the `tiny` cases (factor 0.5 in every round)


def norm64(x):
    return float(np.sqrt((x.astype(f64) ** 2).sum()))


def grads(seed, rnd, clip, tiny):
    """gradients of one round with |g| = FACTORS[rnd] x clip (clip = 0: the norms clip = 15 would give); asserted on the fp64 norms.
    An element keeps its sign from round to round: Adam's m then adds terms of one sign.  Where m cancels, its per-element figure is one
    element's rounding luck (the clip factor's last bit, magnified), in the kernel's summation order as much as in the plain one.
    The 258-chunk tensor carries 99 % of its squared norm in chunks 256 and 257, the two that the 256 threads summing a tensor's partials
    reach only on their second pass: a sum that stops at 256 chunks, or loses either of the two, is off by a factor and not by a per cent
    (and the plain-order fp32 sum, which meets the large terms last, stays accurate, so the tensor's bound stays tight)."""
    c = clip if clip > 0 else 15.0
    out = []
    for i, n in enumerate(SIZES):
        fac = FACTORS[rnd][i]
        sign = np.where(rng(seed, 1000, i).random(n) < 0.5, -1.0, 1.0)
        if tiny and i == TINY:
            x = np.exp(rng(seed, rnd, i).uniform(np.log(2e-9), np.log(5e-8), n)) * sign
        else:
            x = np.abs(rng(seed, rnd, i).standard_normal(n)) * sign
        if i == BIG:
            for lo, hi, share in BIG_SHARES:
                x[lo:hi] *= np.sqrt(share) / norm64(x[lo:hi])
        if clip > 0 or not (tiny and i == TINY):
            x = x * (fac * c / norm64(x))
        x = x.astype(f32)
        if clip > 0:
            ratio = norm64(x) / clip
            assert abs(ratio - fac) <= 1e-6 * fac and abs(ratio - 1.0) > 0.01, (i, ratio)      # the four norms; none within 1 % of the clip
        if tiny and i == TINY:
            assert 1e-9 <= np.abs(x).min() and np.abs(x).max() <= 1e-7
        out.append(x)
    return out


def clip_scales(g, clip):
    """per tensor: tf.clip_by_norm's factor in fp64, and launch's formula clip * min(1 / sqrt(sum), 1 / clip) in plain-order fp32"""
    s64, s32 = [], []
    for x in g:
        if not clip > 0:
            s64.append(1.0); s32.append(f32(1.0))
            continue
        n = norm64(x)
        s64.append(f64(clip) / max(n, f64(clip)))
        s = np.cumsum(x * x, dtype=f32)[-1]
        inv = f32(1.0) / np.sqrt(s) if s > 0 else f32(np.inf)
        s32.append(f32(clip) * min(inv, f32(1.0) / f32(clip)))
    return s64, s32


def dyn_of(**kw):
    d = np.zeros(DYN_COUNT, dtype=f32)
    for k, v in kw.items():
        d[DYN_SLOTS[k]] = v
    return d


def sgd_step(w, g, ema, sc, lr, dec, T):
    """T = f32: the launch's formula in fp32; T = f64: the reference"""
    one = T(1.0)
    nw = [x.astype(T) - T(lr) * (y.astype(T) * T(s)) for x, y, s in zip(w, g, sc)]
    ne = [T(dec) * e.astype(T) + (one - T(dec)) * x for e, x in zip(ema, nw)]
    return nw, ne


@pytest.mark.parametrize("clip", [15.0, 0.0], ids=["clip15", "clip_off"])
@pytest.mark.parametrize("with_ema", [False, True], ids=["no_ema", "ema"])
def test_clip_sgd(eng, with_ema, clip):
    lr, dec = f32(0.05), f32(0.9999)
    w = [rng(30, i).standard_normal(n).astype(f32) for i, n in enumerate(SIZES)]
    ema = [rng(31, i).standard_normal(n).astype(f32) for i, n in enumerate(SIZES)]
    g = grads(32, 0, clip, False)
    s64, s32 = clip_scales(g, clip)
    if clip > 0:
        assert s64[5] < 1.0 and s64[1] == 1.0 and s64[2] == 1.0                 # the 258-chunk tensor is clipped; |g| = 0.5 x clip and 0 are not
    else:
        assert norm64(g[5]) > 15.0 and s64[5] == 1.0                            # clipping off: applied unscaled
    w64, e64 = sgd_step(w, g, ema, s64, lr, dec, f64)
    w32, e32 = sgd_step(w, g, ema, s32, lr, dec, f32)
    w0, g0, e0 = flat(w, SENT), flat(g, np.nan), flat(ema, SENT)
    dyn = dyn_of(d_lr=lr, clip=clip, ema=dec, g_lr=123.0)                          # (SGD is the discriminator's: it reads d_lr)

    def run():
        wd, gd, ed, dd = dev(w0, eng), dev(g0, eng), dev(e0, eng), dev(dyn, eng)
        pd = dev(np.full(NC + 8, SENT, dtype=f32), eng)
        eng.op_update("sumsq", TENSORS, [gd, pd], TOTAL, NC + 8)
        eng.op_update("apply_sgd", TENSORS, [wd, gd, ed if with_ema else None, pd, dd], TOTAL, NC + 8)
        return {"w": host(wd), "ema": host(ed), "dyn": host(dd)}
    out = twice(run)
    assert bits_equal(out["dyn"], dyn) and gaps_unchanged(out["w"], w0)
    case = "sgd %s %s" % ("clip=15" if clip > 0 else "clip=0", "ema" if with_ema else "no-ema")
    bounded_each(case, "w", parts_of(out["w"]), w32, w64)
    if with_ema:
        assert gaps_unchanged(out["ema"], e0)
        bounded_each(case, "ema", parts_of(out["ema"]), e32, e64)
    else:
        assert bits_equal(out["ema"], e0)
    assert not np.any(g[2]) and bits_equal(parts_of(out["w"])[2], w[2])         # clip_by_norm at a zero gradient: no NaN, nothing moves


def lr_t64(lr, b1, b2, t):
    return f64(lr) * np.sqrt(1.0 - f64(b2) ** t) / (1.0 - f64(b1) ** t)


def adam_step(w, g, m, v, ema, sc, lrt, b1, b2, eps, dec, T, eps_inside=False):
    one = T(1.0)
    gg = [y.astype(T) * T(s) for y, s in zip(g, sc)]
    nm = [T(b1) * a.astype(T) + (one - T(b1)) * x for a, x in zip(m, gg)]
    nv = [T(b2) * a.astype(T) + (one - T(b2)) * x * x for a, x in zip(v, gg)]
    if eps_inside:
        nw = [x.astype(T) - T(lrt) * a / np.sqrt(b + T(eps)) for x, a, b in zip(w, nm, nv)]
    else:
        nw = [x.astype(T) - T(lrt) * a / (np.sqrt(b) + T(eps)) for x, a, b in zip(w, nm, nv)]
    ne = [T(dec) * e.astype(T) + (one - T(dec)) * x for e, x in zip(ema, nw)]
    return nw, nm, nv, ne


@pytest.mark.parametrize("case", ["G clip=15", "D tiny clip", "G tiny clip=0"], ids=["G-clip15", "D-tiny-clip", "G-tiny-clip0"])
def test_clip_adam_three_rounds(eng, case):
    """three tick-and-apply rounds, m / v / ema / t carried over.  "tiny": tensor 1's gradients lie in [1e-9, 1e-7], so sqrt(v) is of the
    order of eps = 1e-8; with a clip, the clip is twice that tensor's norm (it passes unclipped) and the other norms are 0, 2 and 100 clips"""
    net_d, tiny = case.startswith("D"), "tiny" in case
    lr_slot, lrt_slot = ("d_lr", "adam_lrt_d") if net_d else ("g_lr", "adam_lrt")
    lr, b1, b2, eps, dec = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(0.9999)
    if case == "G clip=15":
        clip = 15.0
    elif case == "D tiny clip":
        clip = float(f32(2.0 * norm64(grads(40, 0, 0.0, True)[TINY])))
    else:
        clip = 0.0
    gs = [grads(40, r, clip, tiny) for r in range(3)]
    w = [rng(41, i).standard_normal(n).astype(f32) * f32(0.1) for i, n in enumerate(SIZES)]
    ema = [rng(42, i).standard_normal(n).astype(f32) * f32(0.1) for i, n in enumerate(SIZES)]
    zeros = [np.zeros(n, dtype=f32) for n in SIZES]
    st64, st32, refs = (w, zeros, zeros, ema), (w, zeros, zeros, ema), []
    for r in range(3):
        s64, s32 = clip_scales(gs[r], clip)
        if clip > 0:
            assert s64[5] < 1.0 and (not tiny or s64[TINY] == 1.0)
        lrt = lr_t64(lr, b1, b2, r + 1)
        n64 = adam_step(st64[0], gs[r], st64[1], st64[2], st64[3], s64, lrt, b1, b2, eps, dec, f64)
        n32 = adam_step(st32[0], gs[r], st32[1], st32[2], st32[3], s32, f32(lrt), b1, b2, eps, dec, f32)
        if tiny and r == 0:                  # on the CPU: eps inside the root is far outside any bound this test can come to
            wrong = adam_step(st64[0], gs[r], st64[1], st64[2], st64[3], s64, lrt, b1, b2, eps, dec, f64, eps_inside=True)
            e_wrong, e_cpu = elem_err([wrong[0][TINY]], [n64[0][TINY]]), elem_err([n32[0][TINY]], [n64[0][TINY]])
            print("update_ops %-34s eps-inside w err %.2e against the bound %.2e" % ("adam " + case, e_wrong, max(4 * e_cpu, ULP2)))
            assert e_wrong > 1000.0 * max(4.0 * e_cpu, ULP2)
        st64, st32 = n64, n32
        refs.append((n64, n32))
    dyn0 = dyn_of(clip=clip, beta1=b1, beta2=b2, eps=eps, ema=dec, g_lr=7.0, d_lr=9.0)
    dyn0[DYN_SLOTS[lr_slot]] = lr
    bufs0 = [flat(w, SENT), flat(zeros, SENT), flat(zeros, SENT), flat(ema, SENT)]

    def run():
        wd, md, vd, ed = [dev(b, eng) for b in bufs0]
        dd, td = dev(dyn0, eng), dev(np.zeros(4, dtype=np.int32), eng)
        out = {}
        for r in range(3):
            gd, pd = dev(flat(gs[r], np.nan), eng), dev(np.full(NC + 8, SENT, dtype=f32), eng)
            eng.op_update("sumsq", TENSORS, [gd, pd], TOTAL, NC + 8)
            eng.op_step_elem("adam_tick", [dd, td], [DYN_SLOTS[lr_slot], DYN_SLOTS[lrt_slot]], [b1, b2])
            eng.op_update("apply_adam", TENSORS, [wd, gd, md, vd, ed, pd, dd], TOTAL, NC + 8, extra=(DYN_SLOTS[lrt_slot],))
            for k, t in (("w", wd), ("m", md), ("v", vd), ("ema", ed), ("dyn", dd), ("t", td)):
                out["%s%d" % (k, r)] = host(t).copy()
        return out
    out = twice(run)
    other = DYN_SLOTS["adam_lrt" if net_d else "adam_lrt_d"]
    for r in range(3):
        assert out["t%d" % r].tolist() == [r + 1, 0, 0, 0]
        d = out["dyn%d" % r]
        keep = [i for i in range(DYN_COUNT) if i != DYN_SLOTS[lrt_slot]]
        assert bits_equal(d[keep], dyn0[keep]) and d[other] == 0.0              # the tick writes its own lr_t slot only
        n64, n32 = refs[r]
        for k, name in enumerate(("w", "m", "v", "ema")):
            got = out["%s%d" % (name, r)]
            assert gaps_unchanged(got, bufs0[k]), name
            bounded_each("adam %s round %d" % (case, r + 1), name, parts_of(got), n32[k], n64[k])


# ---------------------------------------------------------------------------------------------------------------------- k_adam_tick
@pytest.mark.parametrize("pair", [("g_lr", "adam_lrt"), ("d_lr", "adam_lrt_d")], ids=["G", "D"])
def test_adam_tick(eng, pair):
    lr, b1, b2 = f32(2e-4), f32(0.9), f32(0.999)
    dyn0 = dyn_of(**{pair[0]: lr, "g_lr" if pair[0] == "d_lr" else "d_lr": 55.0})
    for t0, ticks in ((0, 3), (999, 1)):
        def run():
            dd, td = dev(dyn0, eng), dev(np.array([t0, 77], dtype=np.int32), eng)
            out = {}
            for i in range(ticks):
                eng.op_step_elem("adam_tick", [dd, td], [DYN_SLOTS[pair[0]], DYN_SLOTS[pair[1]]], [b1, b2])
                out["dyn%d" % i], out["t%d" % i] = host(dd).copy(), host(td).copy()
            return out
        out = twice(run)
        for i in range(ticks):
            t = t0 + i + 1
            assert out["t%d" % i].tolist() == [t, 77]
            want = f32(lr_t64(lr, b1, b2, t))
            got = out["dyn%d" % i][DYN_SLOTS[pair[1]]]
            print("update_ops %-34s t=%-4d lr_t got %.9e want %.9e" % ("adam_tick " + pair[0], t, got, want))
            assert abs(f64(got) - f64(want)) <= f64(np.spacing(want)), (t, got, want)        # within 1 fp32 ulp of the fp64 formula
            keep = [k for k in range(DYN_COUNT) if k != DYN_SLOTS[pair[1]]]
            assert bits_equal(out["dyn%d" % i][keep], dyn0[keep])
