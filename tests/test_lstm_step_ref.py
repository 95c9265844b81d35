"""tests/lstm_step_ref.py pinned to something other than itself (no device): its forward phases, chained, are the oracle's cell; its two
backward phases, chained, are torch.autograd through its forward phases.  Both in float64, to 1e-12."""
import numpy as np
import pytest
import torch

from oracle import rsrgan_oracle as O
from tests import lstm_step_cases as Cs
from tests import lstm_step_ref as R
from tests.update_ref import ULP2, elem_err

f64 = np.float64
TOL = 1e-12


def layer_params(rng, I, P, H, proj):
    r = P if proj else H
    return {"K": rng.uniform(-0.4, 0.4, (I + r, 4 * H)), "b": rng.uniform(-0.3, 0.3, 4 * H), "wf": rng.uniform(-0.5, 0.5, H),
            "wi": rng.uniform(-0.5, 0.5, H), "wo": rng.uniform(-0.5, 0.5, H), "Wp": rng.uniform(-0.4, 0.4, (H, P)) if proj else None}


def step_fwd(p, I, x, m, c, lengths, t, forget_bias, wrap=lambda a: a):
    """one step of one layer through the phase functions: (out, m_next, c_next, gates)"""
    g = R.fwd_gates(f64, x=x, Kx=wrap(p["K"][:I]), bias=wrap(p["b"]), m=m, Kh=wrap(p["K"][I:]), wi=wrap(p["wi"]), wf=wrap(p["wf"]),
                    wo=wrap(p["wo"]), c_prev=c, length=lengths, t=t, forget_bias=forget_bias, noproj=p["Wp"] is None)
    if p["Wp"] is None:
        return g["out"], g["m_out"], g["c_out"], g
    q = R.fwd_proj(f64, h=g["h"], Wp=wrap(p["Wp"]), m_prev=m, length=lengths, t=t)
    return q["out"], q["m_out"], g["c_out"], g


@pytest.mark.parametrize("proj", [True, False])
@pytest.mark.parametrize("forget_bias", [1.0, 0.0])
def test_forward_phases_chain_to_the_oracle_cell(proj, forget_bias):
    rng = np.random.default_rng([11, int(proj)])
    B, T, I, P, H = 5, 3, 9, 7, 12
    r = P if proj else H
    lengths = np.array([0, 1, 2, 3, 3])
    x = rng.standard_normal((B, T, I))
    layers = [layer_params(rng, I, P, H, proj), layer_params(rng, r, P, H, proj)]
    # the oracle: two stacked dynamic_rnn layers
    ref_in, ref_caches = x, []
    for p in layers:
        ref_in, cache = O.lstmp_fwd(ref_in, lengths, (p["K"], p["b"], p["wf"], p["wi"], p["wo"], p["Wp"]), forget_bias=forget_bias)
        ref_caches.append(cache)
    # the phase functions, step by step
    inp = x
    for l, p in enumerate(layers):
        Il = inp.shape[2]
        m, c = np.zeros((B, r)), np.zeros((B, H))
        outs = np.zeros((B, T, r))
        for t in range(T):
            outs[:, t], m, c, g = step_fwd(p, Il, inp[:, t], m, c, lengths, t, forget_bias)
            mask, _, _, gi, gj, gf, go, cn, _, h = ref_caches[l][0][t]
            live = mask[:, 0]
            for got, want in ((g["gates"], np.concatenate([gi, gj, gf, go], axis=1)), (g["c_out"], cn), (g["h"], h)):
                assert np.abs(got[live] - want[live]).max(initial=0.0) <= TOL
                assert not np.any(got[~live]) or got is g["c_out"]
        ref_out = O.lstmp_fwd(inp, lengths, (p["K"], p["b"], p["wf"], p["wi"], p["wo"], p["Wp"]), forget_bias=forget_bias)[0]
        assert np.abs(outs - ref_out).max() <= TOL
        assert not np.any(outs[lengths[:, None] <= np.arange(T)[None, :]])
        inp = outs
    assert np.abs(inp - ref_in).max() <= TOL


@pytest.mark.parametrize("proj", [True, False])
def test_backward_phases_chain_to_autograd(proj):
    rng = np.random.default_rng([12, int(proj)])
    B, T, I, P, H = 5, 3, 9, 7, 12
    r = P if proj else H
    lengths = np.array([0, 1, 2, 3, 3])
    p = layer_params(rng, I, P, H, proj)
    x = rng.standard_normal((B, T, I))
    m0, c0 = rng.standard_normal((B, r)), rng.standard_normal((B, H))
    G = rng.standard_normal((B, T, r))                       # d loss / d out
    Gm, Gc = rng.standard_normal((B, r)), rng.standard_normal((B, H))       # ... / d final state
    tt = lambda a: torch.tensor(a, dtype=torch.float64)
    xt, m0t, c0t = tt(x).requires_grad_(), tt(m0).requires_grad_(), tt(c0).requires_grad_()
    m, c, loss = m0t, c0t, 0.0
    for t in range(T):
        out, m, c, _ = step_fwd(p, I, xt[:, t], m, c, lengths, t, 1.0, wrap=tt)
        loss = loss + (out * tt(G[:, t])).sum()
    loss = loss + (m * tt(Gm)).sum() + (c * tt(Gc)).sum()
    loss.backward()
    # the same forward in numpy for the stash, then phase A / phase B from t = T - 1 down
    m, c, stash = m0, c0, []
    for t in range(T):
        _, mn, cn, g = step_fwd(p, I, x[:, t], m, c, lengths, t, 1.0)
        stash.append((g["gates"], c, cn))
        m, c = mn, cn
    dmst, dc = Gm.copy(), Gc.copy()
    dx = np.zeros((B, T, I))
    for t in range(T - 1, -1, -1):
        gates, cp, cn = stash[t]
        a = R.bwd_a(f64, dout=G[:, t], dmst=dmst, Wp=p["Wp"], gates=gates, c_prev=cp, c_cur=cn, wi=p["wi"], wf=p["wf"], wo=p["wo"], dc=dc,
                    length=lengths, t=t)
        live = lengths > t
        assert not np.any(a["dz"][~live]) and not np.any(a["dmt"][~live]) and np.array_equal(a["dc"][~live], dc[~live])
        b = R.bwd_b(f64, dz=a["dz"], K=p["K"], I=I, n_begin=0, n_end=I + r, t=t, length=lengths, dx_old=np.full((B, I), 7.0), dmst_old=dmst)
        # the recurrent half alone (rows [I, I + r), no dx) carries the same state gradient
        b1 = R.bwd_b(f64, dz=a["dz"], K=p["K"], I=I, n_begin=I, n_end=I + r, t=t, length=lengths, dmst_old=dmst)
        assert "dx" not in b1 and np.abs(b1["dmst"] - b["dmst"]).max() <= TOL
        dx[:, t], dmst, dc = b["dx"], b["dmst"], a["dc"]
    assert np.abs(dx - xt.grad.numpy()).max() <= TOL
    assert np.abs(dmst - m0t.grad.numpy()).max() <= TOL
    assert np.abs(dc - c0t.grad.numpy()).max() <= TOL


def test_fp32_plain_order_is_sequential():
    """dot(float32) adds one rounded product at a time, k ascending: the value of an explicit loop"""
    rng = np.random.default_rng(13)
    a, b = rng.standard_normal((3, 37)).astype(np.float32), rng.standard_normal((37, 5)).astype(np.float32)
    want = np.zeros((3, 5), np.float32)
    for k in range(37):
        want = (want + a[:, k:k + 1] * b[k:k + 1, :]).astype(np.float32)
    assert np.array_equal(R.dot(a, b, np.float32), want)
    assert np.abs(R.dot(a, b, np.float64) - a.astype(np.float64) @ b.astype(np.float64)).max() < 1e-13


def test_swizzle_rows_describe_whole_images():
    rows = R.swizzle_rows(9, 7, 12)
    assert set(rows) == {"Wg_full", "Wg_h", "Kb_full", "Kb_rec", "WpT_sw", "Wp_sw"}
    assert rows["Wg_full"][1][8:] == [12, 4, 2] and rows["Kb_rec"][1][3:6] == [7, 9, 48] and rows["WpT_sw"][2] == 256
    assert set(R.swizzle_rows(24, 24, 24, has_proj=False)) == {"Wg_full", "Wg_h", "Kb_full", "Kb_rec"}


def test_small_k_jobs_keep_p_above_the_floor():
    """tests/test_gpu_lstm_step_ops.py bounds the outputs that pass through expf / tanhf by 4 p alone, so no floor for the device's math
    library has to be assumed: that needs p above the rule's 2 ulp on the jobs with short products, which the references alone decide"""
    for name, job in Cs.small_k_jobs().items():
        r64, r32 = job.ref(np.float64), job.ref(np.float32)
        for k in r64:
            assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64, (name, k)
            if k in Cs.TRANSCENDENTAL:
                p = elem_err([r32[k]], [r64[k]])
                assert p > ULP2, (name, k, p)
