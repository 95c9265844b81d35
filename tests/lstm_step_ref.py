"""Plain references of ONE LSTMP step, phase by phase as the launch-per-phase kernels of csrc/kernels.hip split it (k_fwd_gates,
k_fwd_proj, k_bwd_a2, k_bwd_b / k_bwd_bp + k_bwd_b_red), for tests/test_gpu_lstm_step_ops.py.  The formulas are the reference project's
cell (tf.contrib.rnn.LSTMCell as models/BNLSTMCell.py:176-217 restates it, under tf.nn.dynamic_rnn's masking; oracle/rsrgan_oracle.py
lstmp_fwd / lstmp_bwd): gate order i, j, f, o; peepholes on c_prev for i and f and on the new c for o; the forget bias added at run time.

Every function works on the LOGICAL arrays (no padding columns) and takes a dtype:
  float64 -- the reference;
  float32 -- the same formula in plain order: every dot product accumulates one term at a time in fp32 (np.cumsum), exp and tanh are
             numpy's fp32 ones.  Its error against float64 is the `p` of the bound rule (tests/update_ref.py).
With torch.float64 tensors in place of arrays the forward functions are differentiable (tests/test_lstm_step_ref.py checks the two
backward phases against torch.autograd through them)."""
import numpy as np

try:
    import torch
except ImportError:                                       # (the references themselves need numpy alone)
    torch = None

f32, f64 = np.float32, np.float64


def _is_t(a):
    return torch is not None and isinstance(a, torch.Tensor)


def _exp(a):
    return torch.exp(a) if _is_t(a) else np.exp(a)


def _tanh(a):
    return torch.tanh(a) if _is_t(a) else np.tanh(a)


def _where(c, a, b):
    if _is_t(a) or _is_t(b):
        c = torch.as_tensor(np.asarray(c))
        a = a if _is_t(a) else torch.as_tensor(np.asarray(a, dtype=f64))
        b = b if _is_t(b) else torch.as_tensor(np.asarray(b, dtype=f64))
        return torch.where(c, a, b)
    return np.where(c, a, b)


def _cat(parts):
    return torch.cat(parts, dim=1) if _is_t(parts[0]) else np.concatenate(parts, axis=1)


def _cast(a, dt):
    if a is None or _is_t(a):
        return a
    return np.asarray(a, dtype=dt)


def dot(a, b, dt):
    """a [N][K] . b [K][M].  float32: one product and one add per term, both rounded to fp32, k ascending"""
    if _is_t(a) or _is_t(b):
        return a @ b
    a, b = np.asarray(a, dtype=dt), np.asarray(b, dtype=dt)
    if dt == f64:
        return a @ b
    N, K = a.shape
    M = b.shape[1]
    out = np.zeros((N, M), f32)
    if K == 0:
        return out
    step = max(1, (1 << 23) // max(N * K, 1))                 # <= 32 MB of products at a time
    for m0 in range(0, M, step):
        prod = a[:, :, None] * b[None, :, m0:m0 + step]
        out[:, m0:m0 + step] = np.cumsum(prod, axis=1, dtype=f32)[:, -1, :]
    return out


def sigmoid(x):
    return 1.0 / (1.0 + _exp(-x)) if _is_t(x) else (x.dtype.type(1.0) / (x.dtype.type(1.0) + np.exp(-x)))


def live_rows(length, t, N):
    """dynamic_rnn: row r takes the step iff t < length[r]; length None (fully_connected stages): every row"""
    if length is None:
        return np.ones((N, 1), bool)
    return (t < np.asarray(length))[:, None]


def fwd_gates(dt, *, m, Kh, wi, wf, wo, c_prev, length, t, forget_bias, x=None, Kx=None, bias=None, zx=None, noproj=False, res_in=None):
    """forward phase 1.  z = zx | bias (+ x . Kx) + m . Kh; Kx [I][4H], Kh [P][4H].  Returns gates [N][4H] = sigma(i), tanh(j),
    sigma(f), sigma(o), c_out, h; with noproj also m_out, out and (res_in given) res_out.  Masked rows: c passes through, gates and h zero."""
    m, Kh, wi, wf, wo, c_prev = (_cast(v, dt) for v in (m, Kh, wi, wf, wo, c_prev))
    N, H = c_prev.shape
    live = live_rows(length, t, N)
    if zx is not None:
        z = _cast(zx, dt)
    else:
        z = _cast(bias, dt)[None, :] + dot(_cast(x, dt), _cast(Kx, dt), dt)
    z = z + dot(m, Kh, dt)
    fb = forget_bias if _is_t(z) else z.dtype.type(forget_bias)
    gi = sigmoid(z[:, :H] + wi * c_prev)
    gf = sigmoid(z[:, 2 * H:3 * H] + fb + wf * c_prev)
    gj = _tanh(z[:, H:2 * H])
    cn = gf * c_prev + gi * gj
    go = sigmoid(z[:, 3 * H:] + wo * cn)
    h = go * _tanh(cn)
    zero = 0.0 if _is_t(z) else np.zeros((), z.dtype)
    out = {"gates": _where(live, _cat([gi, gj, gf, go]), zero), "c_out": _where(live, cn, c_prev), "h": _where(live, h, zero)}
    if noproj:
        out["m_out"] = _where(live, h, m)
        out["out"] = _where(live, h, zero)
        if res_in is not None:
            out["res_out"] = out["out"] + _cast(res_in, dt)
    return out


def fwd_proj(dt, *, h, Wp, t, m_prev=None, length=None, bias=None, noise=None, res_in=None, dropmask=None, keep=1.0):
    """forward phase 2.  v = h . Wp (+ bias), Wp [H][P]; m_out keeps m_prev on masked rows, out is zero there; dropout (dropmask [N][P] of
    0 / 1, out / keep where kept) and noise touch `out` only; res_out = the dropped output + res_in"""
    h, Wp = _cast(h, dt), _cast(Wp, dt)
    N = h.shape[0]
    live = live_rows(length, t, N)
    v = dot(h, Wp, dt)
    if bias is not None:
        v = v + _cast(bias, dt)[None, :]
    zero = 0.0 if _is_t(v) else np.zeros((), v.dtype)
    res = {"m_out": v if m_prev is None else _where(live, v, _cast(m_prev, dt))}
    o = _where(live, v, zero)
    if dropmask is not None:
        kp = float(f32(keep)) if _is_t(o) else o.dtype.type(f32(keep))
        o = _where(np.asarray(dropmask) > 0, o / kp, zero)
    res["out"] = o if noise is None else o + _cast(noise, dt)
    if res_in is not None:
        res["res_out"] = o + _cast(res_in, dt)
    return res


def bwd_a(dt, *, dmst, gates, c_prev, c_cur, wi, wf, wo, dc, length, t, dout=None, Wp=None, dropmask=None, keep=1.0):
    """backward phase A.  dm = mask (dout dropmask / keep + dmst); dh = dm . Wp^T (dm itself without a projection); the gate gradients
    dz = (dai, dj, daf, dao) and the carried dc (csrc/kernels.hip k_bwd_a2).  Masked rows: dz zero, dc unchanged.  Returns dmt, dz, dc."""
    dmst, gates, c_prev, c_cur, wi, wf, wo, dc = (np.asarray(v, dtype=dt) for v in (dmst, gates, c_prev, c_cur, wi, wf, wo, dc))
    N, H = c_prev.shape
    one = dt(1.0)
    live = live_rows(length, t, N)
    d = np.zeros_like(dmst) if dout is None else np.asarray(dout, dtype=dt)
    if dropmask is not None and dout is not None:
        d = np.where(np.asarray(dropmask) > 0, d * (one / dt(f32(keep))), dt(0.0))
    dm = np.where(live, dmst + d, dt(0.0))
    dh = dm if Wp is None else dot(dm, np.asarray(Wp, dtype=dt).T, dt)
    gi, gj, gf, go = gates[:, :H], gates[:, H:2 * H], gates[:, 2 * H:3 * H], gates[:, 3 * H:]
    tc = np.tanh(c_cur)
    dao = dh * tc * go * (one - go)
    dcn = dc + dh * go * (one - tc * tc) + dao * wo
    daf = dcn * c_prev * gf * (one - gf)
    dai = dcn * gj * gi * (one - gi)
    dj = dcn * gi * (one - gj * gj)
    dcp = dcn * gf + dai * wi + daf * wf
    dz = np.where(live, np.concatenate([dai, dj, daf, dao], axis=1), dt(0.0))
    return {"dmt": dm, "dz": dz, "dc": np.where(live, dcp, dc)}


def bwd_b(dt, *, dz, K, I, n_begin, n_end, t, length=None, dx_old=None, dmst_old=None, accumulate=False):
    """backward phase B.  [dx | dmst] = dz . K^T over the kernel rows [n_begin, n_end), K [(I + R)][4H]: columns n < I are dx (assigned, or
    added to dx_old), the others dmst = (live ? 0 : dmst_old) + value -- without lengths every row is live.  Returns dx [N][I] (columns
    < n_begin as dx_old) and dmst [N][n_end - I], whichever exist."""
    dz, K = np.asarray(dz, dtype=dt), np.asarray(K, dtype=dt)
    N = dz.shape[0]
    live = live_rows(length, t, N)
    val = dot(dz, K[n_begin:n_end].T, dt)
    res = {}
    if n_begin < I:
        old = np.asarray(dx_old, dtype=dt)
        dx = old.copy()
        hi = min(I, n_end)
        dx[:, n_begin:hi] = (old[:, n_begin:hi] if accumulate else dt(0.0)) + val[:, :hi - n_begin]
        res["dx"] = dx
    if n_end > I:
        old = np.asarray(dmst_old, dtype=dt)
        lo = max(n_begin, I)
        dm = old.copy()
        dm[:, lo - I:n_end - I] = np.where(live, dt(0.0), old[:, lo - I:n_end - I]) + val[:, lo - n_begin:]
        res["dmst"] = dm
    return res


# ---- the weight images the step kernels read, as Model::refresh_swizzles (csrc/model.cpp) asks launch_swizzle_many for them: one row of
# rsrgan_op_layout("swizzle_many") dims per image -- ld, gates, H, C, c0, K1, I, P, kx, nct, nkb -- and the floats of the image
def pad4(n):
    return (n + 3) & ~3


def swizzle_rows(I, P, H, has_proj=True):
    """K [(I + P)][4H] dense, Wp [H][ldP].  name -> (source, dims row, floats)"""
    ldI, ldP, ldH, H4 = pad4(I), pad4(P), pad4(H), 4 * H
    ncb, kbI, kbP, kbH, kb4 = (H + 15) // 16, (ldI + ldP + 15) // 16, (ldP + 15) // 16, (ldH + 15) // 16, (H4 + 15) // 16
    rows = {"Wg_full": ("K", [H4, 4, H, 0, 0, 0, I, P, ldI, 4 * ncb, kbI]),
            "Wg_h": ("K", [H4, 4, H, 0, 0, 0, I, P, 0, 4 * ncb, kbP]),
            "Kb_full": ("K", [H4, 0, 0, I + P, 0, H4, 0, 0, 0, (I + P + 15) // 16, kb4]),
            "Kb_rec": ("K", [H4, 0, 0, P, I, H4, 0, 0, 0, (P + 15) // 16, kb4])}
    if has_proj:
        rows["WpT_sw"] = ("Wp", [ldP, 1, P, 0, 0, 0, H, 0, 16 * kbH, (P + 15) // 16, kbH])        # M[p][k] = Wp[k][p]
        rows["Wp_sw"] = ("Wp", [ldP, 0, 0, H, 0, P, 0, 0, 0, ncb, kbP])                          # M[cell][k] = Wp[cell][k]
    return {k: (src, r, r[9] * r[10] * 256) for k, (src, r) in rows.items()}
