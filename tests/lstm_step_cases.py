"""The jobs of tests/test_gpu_lstm_step_ops.py as host-side descriptions (numpy only): the logical inputs, the padded buffer images a launch
starts from, the pointer group and dims record of rsrgan_op_lstm_step, which region of which buffer the phase is documented to write,
and the references (tests/lstm_step_ref.py, computed once per job and dtype).  tests/test_lstm_step_ref.py uses the same jobs on the
CPU to show that the plain-order fp32 error `p` of the small-K jobs stays above the 2-ulp floor of the bound rule.

Buffer images: inputs carry finite junk of magnitude 1e3 in the padding columns that meet only zero weights (x in [I, ldI), m in
[P, ldP), h in [H, ldH)), zeros in the padding a kernel copies into an output (dmst / dout of phase A), NaN in the GUARD rows at and
beyond N; outputs are SENT everywhere, guard rows included.

Values.  elem_err is a per-element RELATIVE error, and the bound of an output is 4 x the plain-order fp32 error of one evaluation.  With
operands of random sign every dot product and every sum of the cell formula cancels somewhere, 1 / |value| is heavy-tailed, and both
k and p become the rounding error of the ONE most-cancelled element of the tensor -- two independent draws whose ratio says nothing
about the kernel (and a bound of 1e-3 where arithmetic is good to 1e-6).  So the jobs are built without cancellation: every sum the
phases form has terms of one sign.  Activations are positive, a weight column (a kernel row in phase B) carries ONE sign, and the
operands that meet it in a sum carry the same one: bias and zx the sign of their gate column; c_prev the sign of its cell's j column;
w_i, w_f, w_o the sign that makes w . c agree with the gate's pre-activation (the forget column is positive, so forget_bias adds);
in phase A w_o follows c_t, w_i follows tanh(j), w_f follows c_prev, and dout, dmst, Wp are positive; in phase B the old dx / dmst carry
their column's sign.  What keeps the plain-order p of the short products above the rule's 2 ulp (tests/test_lstm_step_ref.py checks it)
is arithmetic error under a BOUNDED condition number, the same in every element, and never an amplified error of exp or tanh itself:
forward, the i, f and o pre-activations have magnitudes 4 .. 11, negative in three cells of four, and sigma's relative error at a negative argument is the
absolute error of that argument (forget_bias against a negative f column cancels at most 5 : 3); backward, the carried dc opposes the
step's own contribution at a fixed 72 .. 80 % (BwdAJob), so the new dc -- and the three gate gradients proportional to it -- carry a
condition number of ~7; |c_t| <= 1.5 and |tanh(j)| <= 0.9 keep 1 - tanh^2 away from amplifying the library's own error."""
import numpy as np

from tests import lstm_step_ref as R
from tests.helpers import _mask_of_tag
from tests.update_ref import SENT

f32, f64 = np.float32, np.float64
GUARD = 3                                      # rows behind row N - 1 of every [N][ld] buffer
pad4 = R.pad4


def image(a, ld, pad="junk", guard=np.nan, rng=None):
    """[N][C] -> float32 [N + GUARD][ld]: padding columns `pad` ("junk": finite, magnitude 1e3), guard rows `guard`"""
    a = np.asarray(a, dtype=f32)
    N, C = a.shape
    out = np.empty((N + GUARD, ld), f32)
    out[:N, :C] = a
    if ld > C:
        out[:N, C:] = (1e3 * np.sign(rng.standard_normal((N, ld - C)) + 1e-9)).astype(f32) if isinstance(pad, str) else f32(pad)
    out[N:] = f32(guard)
    return out


def blank(N, ld):
    return np.full((N + GUARD, ld), SENT, f32)


def signs(rng, n, p_neg=0.5):
    return np.where(rng.random(n) < p_neg, -1.0, 1.0)


def lengths(rng, N, t):
    """0, t, t + 1 and a value above t + 1 are always present: both branches at the boundary"""
    ln = rng.integers(0, t + 4, N)
    ln[:4] = [0, t, t + 1, t + 3]
    return rng.permutation(ln).astype(np.int32)


class Job:
    op = None
    keep = 1.0                                 # (of a job without dropout: the entry does not read it)

    def _drop_values(self, N, P, on, seed):
        self.dropmask, self.keep, self.ddims, self.run = None, 1.0, [0, 0, 0], 5
        if on:
            self.keep, dseed, tag = 0.75, 0x1234ABCD + seed, (1 << 40) | (2 << 20) | 3
            self.dropmask = _mask_of_tag(dseed, self.run, tag, N, P, self.keep)
            self.ddims = [dseed, tag, int(float(f32(self.keep)) * 16777216.0)]

    def _drop(self, N, P, on, seed):
        self._drop_values(N, P, on, seed)
        if on:
            self.bufs["ctr"] = np.array([self.run], np.int64)   # (the device reads it as unsigned)

    def ref(self, dt):
        key = "_ref_%s" % np.dtype(dt).name
        if not hasattr(self, key):
            setattr(self, key, self._ref(dt))
        return getattr(self, key)


class GatesJob(Job):
    """k_fwd_gates: (N, I, P, H); zx: the x-part precomputed, gates aliases it (I is unused); noproj: m = h (P = H), the np_* outputs"""
    op = "fwd_gates"

    def __init__(self, N, I, P, H, zx=False, noproj=False, res=False, t=2, seed=0):
        rng = np.random.default_rng([101, seed, N, P, H])
        I = 0 if zx else I
        P = H if noproj else P
        self.N, self.I, self.P, self.H, self.zx, self.noproj, self.res, self.t = N, I, P, H, zx, noproj, res, t
        ldI, ldP, ldH, H4 = pad4(I), pad4(P), pad4(H), 4 * H
        # per cell: the sign of the j column (and of c_prev), of the i, f and o columns (three in four negative: see above)
        u, si, sf, so = signs(rng, H), signs(rng, H, 0.75), signs(rng, H, 0.75), signs(rng, H, 0.75)
        sc = np.concatenate([si, u, sf, so])
        self.K = (sc[None, :] * rng.uniform(0.2, 1.0, (I + P, H4)) * (1.5 / (I + P))).astype(f32)
        self.x = rng.uniform(0.1, 1.0, (N, I)).astype(f32)
        self.m = rng.uniform(0.1, 1.0, (N, P)).astype(f32)
        lo, hi = np.repeat([4.0, 0.5, 4.0, 4.0], H), np.repeat([10.0, 2.0, 10.0, 10.0], H)       # magnitudes: i, f, o 4 .. 10, j 0.5 .. 2
        self.zxv = (sc[None, :] * rng.uniform(lo, hi, (N, H4))).astype(f32)
        self.bias = (sc * rng.uniform(lo, hi)).astype(f32)
        self.wi, self.wf, self.wo = ((sg * rng.uniform(0.2, 0.6, H)).astype(f32) for sg in (si * u, sf * u, so * u))
        self.c_prev = (u[None, :] * rng.uniform(0.3, 1.0, (N, H))).astype(f32)
        self.len = lengths(rng, N, t)
        self.forget_bias = 1.0
        # the residual input: 5 .. 50 % of the output it is added to and of its sign (any value on the masked rows, where the output is 0),
        # so the sum keeps the relative error of h in every element
        self.noproj = self.res = False
        h64 = self._ref(f64)["h"]
        self.noproj, self.res = noproj, res
        self.res_in = np.where(h64 != 0.0, h64 * rng.uniform(0.05, 0.5, (N, H)), rng.uniform(0.3, 1.0, (N, H)))[:, :P].astype(f32) if noproj else None
        self.bufs = {"K": self.K, "m": image(self.m, ldP, rng=rng), "wf": self.wf, "wi": self.wi, "wo": self.wo,
                     "c_prev": image(self.c_prev, H), "c_out": blank(N, H), "h": blank(N, ldH), "len": self.len}
        if zx:
            self.bufs["gates"] = image(self.zxv, H4, guard=SENT)
        else:
            self.bufs.update(x=image(self.x, ldI, rng=rng), bias=self.bias, gates=blank(N, H4))
        self.outs = {"gates": ("gates", 0, H4, None), "c_out": ("c_out", 0, H, None), "h": ("h", 0, H, None)}
        if noproj:
            self.bufs.update(m_out=blank(N, ldP), out=blank(N, ldP))
            self.outs.update(m_out=("m_out", 0, H, None), out=("out", 0, H, None))
            if res:
                self.bufs.update(res_in=image(self.res_in, ldP, rng=rng), res_out=blank(N, ldP))
                self.outs["res_out"] = ("res_out", 0, H, None)
        self.images = {"Wsw": "Wg_h" if zx else "Wg_full"}
        np_ = ["m_out", "out", "res_in" if res else None, "res_out" if res else None] if noproj else [None] * 4
        self.ptrs = [None if zx else "x", None, "m", None, "Wsw", "gates" if zx else None, None if zx else "bias", "wf", "wi", "wo", "c_prev",
                     "c_out", "gates", "h", "len"] + np_
        self.dims = [N, H, ldI, ldP, ldH, t]

    def _ref(self, dt):
        kw = dict(zx=self.zxv) if self.zx else dict(x=self.x, Kx=self.K[:self.I], bias=self.bias)
        return R.fwd_gates(dt, m=self.m, Kh=self.K[self.I:], wi=self.wi, wf=self.wf, wo=self.wo, c_prev=self.c_prev, length=self.len, t=self.t,
                           forget_bias=self.forget_bias, noproj=self.noproj, res_in=self.res_in if self.res else None, **kw)


class ProjJob(Job):
    """k_fwd_proj: (N, P, H); fc: the fully_connected form (no len, no m_prev, the row-major WpT alone, bias and noise, ldo != ldm)"""
    op = "fwd_proj"

    def __init__(self, N, P, H, fc=False, res=False, drop=False, t=2, seed=0):
        rng = np.random.default_rng([102, seed, N, P, H])
        self.N, self.P, self.H, self.fc, self.res, self.t = N, P, H, fc, res, t
        ldP, ldH = pad4(P), pad4(H)
        ldo = ldP + 4 if fc else ldP
        sp = signs(rng, P)                                            # the sign of an output column
        self.Wp = (sp[None, :] * rng.uniform(0.2, 1.0, (H, P)) * (1.5 / H)).astype(f32)
        self.h = rng.uniform(0.1, 1.0, (N, H)).astype(f32)
        self.m_prev = rng.standard_normal((N, P)).astype(f32)
        self.bias = (sp * rng.uniform(0.5, 1.5, P)).astype(f32)
        self.noise = (sp[None, :] * rng.uniform(0.1, 1.0, (N, P))).astype(f32)
        self.res_in = (sp[None, :] * rng.uniform(0.1, 1.0, (N, P))).astype(f32)
        self.len = None if fc else lengths(rng, N, t)
        self.bufs = {"Wp": image(self.Wp, ldP, pad=0.0)[:H], "h": image(self.h, ldH, rng=rng), "m_out": blank(N, ldP), "out": blank(N, ldo)}
        self.outs = {"m_out": ("m_out", 0, P, None), "out": ("out", 0, P, None)}
        if fc:
            self.bufs.update(bias=self.bias, noise=np.concatenate([self.noise.ravel(), np.full(8, np.nan, f32)]))
        else:
            self.bufs.update(m_prev=image(self.m_prev, ldP, rng=rng), len=self.len)
        if res:
            self.bufs.update(res_in=image(self.res_in, ldP, rng=rng), res_out=blank(N, ldP))
            self.outs["res_out"] = ("res_out", 0, P, None)
        self._drop(N, P, drop, seed)
        self.images = {"WpT": "transpose"} if fc else {"WpT": "transpose", "WpT_sw": "WpT_sw"}
        self.ptrs = ["h", "WpT", None if fc else "WpT_sw", None if fc else "m_prev", "m_out", "out", "res_in" if res else None,
                     "res_out" if res else None, None if fc else "len", "bias" if fc else None, "noise" if fc else None, "ctr" if drop else None]
        self.dims = [N, P, ldH, ldP, ldo, t] + self.ddims

    def _ref(self, dt):
        return R.fwd_proj(dt, h=self.h, Wp=self.Wp, t=self.t, m_prev=None if self.fc else self.m_prev, length=self.len,
                          bias=self.bias if self.fc else None, noise=self.noise if self.fc else None, res_in=self.res_in if self.res else None,
                          dropmask=self.dropmask, keep=self.keep)


class BwdAJob(Job):
    """k_bwd_a2: (N, P, H); noproj: no Wp (P = H), dmt must stay untouched"""
    op = "bwd_a"

    def __init__(self, N, P, H, noproj=False, dout=True, drop=False, t=2, seed=0):
        rng = np.random.default_rng([103, seed, N, P, H])
        P = H if noproj else P
        self.N, self.P, self.H, self.noproj, self.has_dout, self.t = N, P, H, noproj, dout, t
        ldP, H4 = pad4(P), 4 * H
        tj, up, sn = signs(rng, H), signs(rng, H), signs(rng, H)      # per cell: the sign of tanh(j), of c_prev, of c_t
        self.Wp = (rng.uniform(0.2, 1.0, (H, P)) * (1.5 / P)).astype(f32)
        self.dout = rng.uniform(0.1, 1.0, (N, P)).astype(f32)
        self.dmst = rng.uniform(0.1, 1.0, (N, P)).astype(f32)
        g = rng.uniform(0.1, 0.9, (N, H4))
        g[:, H:2 * H] = tj[None, :] * rng.uniform(0.2, 0.9, (N, H))
        self.gates = g.astype(f32)
        self.c_prev = (up[None, :] * rng.uniform(0.3, 1.5, (N, H))).astype(f32)
        self.c_cur = (sn[None, :] * rng.uniform(0.3, 1.5, (N, H))).astype(f32)
        self.dc = rng.uniform(0.1, 1.0, (N, H)).astype(f32)
        self.wi, self.wf, self.wo = ((sg * rng.uniform(0.2, 0.6, H)).astype(f32) for sg in (tj, up, sn))
        self.len = lengths(rng, N, t)
        self.has_dout, self.noproj, self.N, self.P, self.H, self.t, self.dropmask, self.keep = dout, noproj, N, P, H, t, None, 1.0
        self._drop_values(N, P, drop, seed)
        # the carried dc of the live rows opposes the step's own contribution R = dh go (1 - tc^2) + dao w_o (positive by construction) at
        # 72 .. 80 % of it: the new dc is 20 .. 28 % of R everywhere, a cancellation of one bounded ratio (condition ~7) in every element
        zero = self._ref(f64, dc=np.zeros((N, H)))
        tc = np.tanh(self.c_cur.astype(f64))
        go = self.gates[:, 3 * H:].astype(f64)
        dao = zero["dz"][:, 3 * H:]
        rest = dao / (tc * go * (1.0 - go)) * go * (1.0 - tc * tc) + dao * self.wo.astype(f64)
        live_rows = (self.len > t)[:, None]
        assert np.all(rest[live_rows[:, 0]] > 0.0)
        self.dc = np.where(live_rows, -rest * rng.uniform(0.72, 0.8, (N, H)), self.dc).astype(f32)
        live = self.len > t
        self.bufs = {"dmst": image(self.dmst, ldP, pad=0.0), "dmt": blank(N, ldP), "gates": image(self.gates, H4, guard=SENT),
                     "c_prev": image(self.c_prev, H), "c_cur": image(self.c_cur, H), "wf": self.wf, "wi": self.wi, "wo": self.wo,
                     "dc": image(self.dc, H, guard=SENT), "len": self.len}
        if dout:
            self.bufs["dout"] = image(self.dout, ldP, pad=0.0)
        self.outs = {"dz": ("gates", 0, H4, None), "dc": ("dc", 0, H, live)}
        if not noproj:
            self.bufs["Wp"] = image(self.Wp, ldP, pad=0.0)[:H]
            self.outs["dmt"] = ("dmt", 0, ldP, None)             # whole float4s up to ldm: the padding comes out as the zeros that went in
        self.images = {} if noproj else {"Wp_sw": "Wp_sw"}
        self._drop(N, P, drop, seed)
        self.ptrs = ["dout" if dout else None, "dmst", None if noproj else "Wp", None if noproj else "Wp_sw", "dmt", "gates", "c_prev", "c_cur",
                     "wf", "wi", "wo", "dc", "len", "ctr" if drop else None]
        self.dims = [N, P, H, ldP, t] + self.ddims

    def _ref(self, dt, dc=None):
        r = R.bwd_a(dt, dout=self.dout if self.has_dout else None, dmst=self.dmst, Wp=None if self.noproj else self.Wp, gates=self.gates,
                    c_prev=self.c_prev, c_cur=self.c_cur, wi=self.wi, wf=self.wf, wo=self.wo, dc=self.dc if dc is None else dc, length=self.len,
                    t=self.t, dropmask=self.dropmask, keep=self.keep)
        ldP = pad4(self.P)
        r["dmt"] = np.concatenate([r["dmt"], np.zeros((self.N, ldP - self.P), r["dmt"].dtype)], axis=1)
        return r


class BwdBJob(Job):
    """k_bwd_b and the split-K pair: (N, I, P, H); with_dx False: rows [I, I + P) alone, dx NULL (or, dx_given, a buffer that must stay
    untouched); tiled False: the row-major K; fc: y (+)= in . W^T of a fully_connected stage (I = D columns, K = H4 = ld_in, no len, no dmst)"""
    op = "bwd_b"

    def __init__(self, N, I, P, H, with_dx=True, accumulate=False, tiled=True, fc=False, dx_given=False, t=2, seed=0, H4=None):
        rng = np.random.default_rng([104, seed, N, I, P, H])
        P = 0 if fc else P
        H4 = H4 if fc else 4 * H
        self.N, self.I, self.P, self.H4, self.fc, self.t, self.acc = N, I, P, H4, fc, t, accumulate
        self.n_begin, self.n_end = (0 if with_dx else I), I + P
        ldI, ldP = pad4(I), pad4(P)
        sr = signs(rng, I + P)                                        # the sign of a kernel row = of an output column
        self.K = (sr[:, None] * rng.uniform(0.2, 1.0, (I + P, H4)) * (1.5 / H4)).astype(f32)
        self.dz = rng.uniform(0.1, 1.0, (N, H4)).astype(f32)
        self.dx0 = (sr[None, :I] * rng.uniform(0.1, 1.0, (N, I))).astype(f32)
        self.dm0 = (sr[None, I:] * rng.uniform(0.1, 1.0, (N, P))).astype(f32)
        self.len = None if fc else lengths(rng, N, t)
        self.bufs = {"dz": image(self.dz, H4), "K": self.K}
        self.outs = {}
        if with_dx or dx_given:
            self.bufs["dx"] = image(self.dx0, ldI, pad=SENT, guard=SENT)
        if with_dx:
            self.outs["dx"] = ("dx", 0, I, None)
        if not fc:
            self.bufs.update(dmst=image(self.dm0, ldP, pad=SENT, guard=SENT), len=self.len)
            self.outs["dmst"] = ("dmst", 0, P, None)
        self.images = {"Ksw": "Kb_full" if with_dx else "Kb_rec"} if tiled else {}
        self.ptrs = ["dz", "K", "Ksw" if tiled else None, "dx" if "dx" in self.bufs else None, None if fc else "dmst", None if fc else "len"]
        self.dims = [N, I, self.n_begin, self.n_end, ldI, ldP, t, H4, 1 if accumulate else 0]
        self.H = H4 // 4

    def _ref(self, dt):
        return R.bwd_b(dt, dz=self.dz, K=self.K, I=self.I, n_begin=self.n_begin, n_end=self.n_end, t=self.t, length=self.len, dx_old=self.dx0,
                       dmst_old=self.dm0, accumulate=self.acc)


# the outputs that pass through the device's expf / tanhf: their bound needs p above the 2-ulp floor (see the GPU test's docstring)
TRANSCENDENTAL = ("gates", "c_out", "h", "m_out", "out", "res_out", "dz", "dc")


def gates_fb0():
    job = GatesJob(5, 9, 7, 12, seed=3)
    job.forget_bias = 0.0
    return job


def three(op):
    """two heavy jobs of different shapes and one light one: plan_groups gives each heavy job a group of XCD slots"""
    return {"fwd_gates": lambda: [GatesJob(33, 24, 24, 40, seed=1), GatesJob(30, 20, 28, 44, seed=2), GatesJob(5, 9, 7, 12, seed=3)],
            "fwd_proj": lambda: [ProjJob(33, 40, 48, seed=1), ProjJob(40, 36, 40, res=True, seed=2), ProjJob(5, 7, 12, seed=3)],
            "bwd_a": lambda: [BwdAJob(33, 40, 80, seed=1), BwdAJob(40, 36, 70, seed=2), BwdAJob(5, 7, 12, seed=3)],
            "bwd_b": lambda: [BwdBJob(33, 24, 24, 40, seed=1), BwdBJob(30, 20, 28, 44, with_dx=False, seed=2), BwdBJob(5, 9, 7, 12, seed=3)],
            "bwd_b_splitk": lambda: [BwdBJob(33, 24, 24, 40, seed=1), BwdBJob(30, 20, 28, 44, seed=2), BwdBJob(5, 9, 7, 12, seed=3)]}[op]()


def eight(op):
    """MAXJ small jobs of different shapes and forms"""
    if op == "fwd_gates":
        return [GatesJob(5 + j, 9, 7 + j % 3, 12 + j, zx=j % 2 == 1, seed=10 + j) for j in range(8)]
    if op == "fwd_proj":
        return [ProjJob(5 + j, 7 + j, 12 + j, res=j % 2 == 1, seed=10 + j) for j in range(8)]
    if op == "bwd_a":
        return [BwdAJob(5 + j, 7 + j, 12 + j, noproj=j == 5, dout=j != 2, seed=10 + j) for j in range(8)]
    return [BwdBJob(5 + j, 9, 7 + j, 12 + j, with_dx=j % 3 != 1, accumulate=j % 2 == 1, seed=10 + j) for j in range(8)]


def small_k_jobs():
    """the jobs of the GPU test whose products are short (K <= 80): where the plain-order p could fall to the floor"""
    jobs = {"gates (5,9,7,12)": GatesJob(5, 9, 7, 12), "gates forget_bias 0": gates_fb0(), "gates zx (17,-,16,20)": GatesJob(17, 0, 16, 20, zx=True),
            "gates noproj (19,24,24,24)": GatesJob(19, 24, 24, 24, noproj=True, res=True), "bwd_a (5,-,7,12)": BwdAJob(5, 7, 12),
            "bwd_a (33,-,64,40)": BwdAJob(33, 64, 40), "bwd_a (33,-,65,40)": BwdAJob(33, 65, 40), "bwd_a drop (33,-,65,40)": BwdAJob(33, 65, 40, drop=True),
            "bwd_a no dout (5,-,7,12)": BwdAJob(5, 7, 12, dout=False, seed=1), "bwd_a noproj (19,-,24,24)": BwdAJob(19, 24, 24, noproj=True)}
    for op in ("fwd_gates", "bwd_a"):
        jobs.update({"%s three %d" % (op, j): job for j, job in enumerate(three(op))})
        jobs.update({"%s eight %d" % (op, j): job for j, job in enumerate(eight(op))})
    return jobs
