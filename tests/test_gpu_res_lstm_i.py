"""g_type 'res_lstm_i' (models/res_lstm_i.py under models/rnn_trainer.py) on the device against tests/res_lstm_i_ref.py, the fp64
reference tests/test_res_lstm_i_ref.py pins on the CPU.  Truth is always that reference, never another configuration of the library.

Bounds: the small nets are held to tests/test_gpu_parity.py's for the same quantities (losses 1e-4, gradients 2e-3 relative L2 per
tensor, variables and EMA after the steps 1e-4, outputs 1e-4), the reference widths to tests/test_gpu_fullsize.py's (losses and
enhanced-MFCC L1 1e-3, every gradient tensor 2e-3), the stateful forward to tests/test_gpu_stream.py's (1e-4 small, 1e-3 reference
width).  Which plan ran is asserted through the launch counters (rsrgan_profile_read_kind): kind 1 the persistent forward launch
(k_glstm_fwd<..., RESX> here), kind 2 the persistent BPTT.

RES_LSTM_I_MARGIN_OUT=<file>: the reference-width cases append their achieved errors to that JSON file (the way
profiles/r7_stream_margin.json was written; DESIGN.md 6k says what has been recorded so far)."""
import json
import os

import numpy as np
import pytest

from oracle import rsrgan_oracle as O
from tests import res_lstm_i_ref as R
from tests.helpers import NET_G, args_for, overrides, rand_batch, rand_params, rel_err, seq_dropout_mask, split_flat

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_RTOL = 1e-4, 2e-3     # tests/test_gpu_parity.py
RTOL = 1e-3                           # tests/test_gpu_fullsize.py
K_GFWD, K_GBWD = 1, 2                 # rsrgan_profile_read_kind (include/rsrgan.h)
LR = float(np.float32(1e-3))


def small(L=2):
    return R.make_cfg(input_dim=9, output_dim=5, g_layers=L, g_cells=12, g_proj=9, d_layers=2, d_cells=8, d_proj=5)


def ragged(cfg, B, T, seed):
    x, lab, ln = rand_batch(cfg, B, T, seed=seed, ragged=True)
    if B > 1:
        ln[-1] = 1
    if B > 2:
        ln[1] = T // 2 + 1
    return x, lab, ln


def pair(cfg, B, T, flags, seed=0, keep=1.0, l2=1e-3, g_type=None, g=None):
    """(RNNTrainer on the HIP engine, fp64 reference) with identical fp32-rounded variables"""
    from rsrgan_amd.trainer import RNNTrainer
    g = R.rand_g(cfg, seed) if g is None else g
    _, d = rand_params(R.table_cfg(cfg), seed)
    args = args_for(cfg, B, l2_scale=l2, g_learning_rate=1e-3, keep_prob=keep)
    if g_type is not None:
        args.g_type = g_type
    m = RNNTrainer(None, args, ["gpu:0"], max_frames=T, net_overrides=dict(overrides(cfg), flags=flags))
    assert [(n, tuple(s)) for n, s, _ in m.engine.tensor_table(NET_G)] == [(n, tuple(s)) for n, s in R.g_param_specs(cfg)]
    m.set_vars(g, d)
    drop = {} if keep >= 1.0 else dict(keep_prob=float(np.float32(keep)),
                                       mask_fn=lambda run, tower, layer, b, t, p: seq_dropout_mask(4321, run, layer, b, t, p, keep))
    o = R.ResLstmIOracle(cfg, g, batch_size=B, l2_scale=l2, g_learning_rate=LR, **drop)
    return m, o


def grads_of(m):
    return split_flat(m.engine.get_grads(NET_G).cpu().numpy(), m.engine.tensor_table(NET_G))


def check_grads(got, want, tol=GRAD_RTOL):
    errs = {}
    for k in want:
        e = rel_err(got[k], want[k])
        errs[k] = e
        scale = float(np.abs(want[k]).max())
        assert e < tol or np.abs(got[k] - want[k]).max() < 1e-6 * max(scale, 1.0), (k, e)
    return errs


def l1(y, want):
    return float(np.abs(y - want).mean() / np.abs(want).mean())


def kinds_of(eng):
    k = {i: eng.profile_read_kind(i)[0] for i in range(1, 9)}
    eng.profile_read()
    return k


def _margin(name, rec):
    path = os.environ.get("RES_LSTM_I_MARGIN_OUT")
    print("res_lstm_i margin", name, json.dumps(rec, sort_keys=True))
    if not path:
        return
    data = json.load(open(path)) if os.path.exists(path) else {"bounds": {"losses": RTOL, "mfcc": RTOL, "gradients": GRAD_RTOL}, "cases": {}}
    data["cases"][name] = rec
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


# ---- small net: 9 -> L x LSTMP(12, p9) -> 5; L = 3 is where "always x" and "running sum" differ in a middle layer --------------------

@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("B", [1, 4, 40])
@pytest.mark.parametrize("L", [2, 3])
def test_small_matches_reference(L, B, flags):
    cfg = small(L)
    T = 7
    m, o = pair(cfg, B, T, flags, seed=11 + L)
    x, lab, ln = ragged(cfg, B, T, 5)
    got = m.engine.g_backward(x, lab, ln, None, train=True, apply=False).cpu().numpy()
    want, wg, y_ref = o.g_tower(x.astype(np.float64), lab.astype(np.float64), ln)
    print("small", L, B, flags, "losses", got, want)
    assert got[0] == 0.0 and np.allclose(got[1:], want[1:], rtol=LOSS_RTOL, atol=1e-7), (got, want)
    print("gradients", check_grads(grads_of(m), wg))
    y = m.forward(x, ln)
    assert np.abs(y - y_ref).max() < 1e-4 and l1(y, y_ref) < LOSS_RTOL
    # padded frames: y = x . W + b
    pad = np.arange(T)[None, :] >= ln[:, None]
    if pad.any():
        g32 = {k: v.astype(np.float64) for k, v in o.g.items()}
        assert np.abs(y - (x.astype(np.float64) @ g32[R.FC_W] + g32[R.FC_B]))[pad].max() < 1e-5
    for i in range(3):
        xs, ls, lns = ragged(cfg, B, T, 20 + i)
        a = np.ravel(m.step(xs, ls, lns)); b = np.ravel(o.g_step(xs, ls, lns))[1:]
        assert np.allclose(a, b, rtol=LOSS_RTOL, atol=1e-7), (i, a, b)
    gv, _ = m.get_vars()
    ema = split_flat(m.engine.get_params(NET_G, "ema").cpu().numpy(), m.engine.tensor_table(NET_G))
    for k in o.g:
        assert rel_err(gv[k], o.g[k]) < 1e-4, k
        assert rel_err(ema[k], o.g_ema[k]) < 1e-4, k
    assert m.engine.get_scalar("adam_step") == 3 and m.engine.device_status() == 0


@pytest.mark.parametrize("flags", [0, 1])
def test_dropout_wrapper_small(flags):
    """DropoutWrapper(output_keep_prob) wraps the cell: out_l is dropped before the add; res_lstm_l's per-layer mask tags"""
    cfg = small(3)
    B, T, keep = 5, 7, 0.75
    m, o = pair(cfg, B, T, flags, seed=17, keep=keep)
    _, plain = pair(cfg, B, T, flags, seed=17)
    for i in range(3):
        xs, ls, lns = ragged(cfg, B, T, 30 + i)
        a = np.ravel(m.step(xs, ls, lns)); b = np.ravel(o.g_step(xs, ls, lns))[1:]
        assert np.allclose(a, b, rtol=LOSS_RTOL, atol=1e-7), (i, a, b)
        if i == 0:
            assert not np.allclose(b[0], np.ravel(plain.g_step(xs, ls, lns))[1], rtol=1e-3)      # the masks do act
    gv, _ = m.get_vars()
    for k in o.g:
        assert rel_err(gv[k], o.g[k]) < 2e-4, k         # (tests/test_gpu_parity.py::test_dropout_wrapper_on_the_generator_layers' bound)
    xs, ls, lns = ragged(cfg, B, T, 5)
    ev = np.ravel(m.step(xs, ls, lns, train=False)); w = np.ravel(o.g_step(xs, ls, lns, train=False))
    assert np.allclose(ev[0], w[1], rtol=LOSS_RTOL)                                             # the evaluation fetch is undropped
    assert m.engine.device_status() == 0


# ---- reference widths: 2 x LSTMP(760, p257), the persistent launches and the launch path --------------------------------------------

def _wide_case(name, B, persistent):
    cfg = R.make_cfg()
    T = 12
    m, o = pair(cfg, B, T, 1, seed=400 + B, l2=0.0)
    x, lab, ln = ragged(cfg, B, T, 500 + B)
    x64, lab64 = x.astype(np.float64), lab.astype(np.float64)
    eng = m.engine
    eng.profile_begin()
    got = eng.g_backward(x, lab, ln, None, train=True, apply=False).cpu().numpy()
    y = m.forward(x, ln)
    k = kinds_of(eng)
    want, wg, y_ref = o.g_tower(x64, lab64, ln)
    gerr = {n: rel_err(v, wg[n]) for n, v in grads_of(m).items()}
    lerr = float(np.abs(got[1:] - np.asarray(want[1:])).max() / abs(want[3]))
    _margin(name, dict(B=B, T=T, persistent=persistent, loss_rel=lerr, mfcc_l1=l1(y, y_ref), grad_rel_max=max(gerr.values()),
                       grad_rel=gerr, kinds={str(i): v for i, v in k.items()}))
    assert got[0] == 0.0 and np.allclose(got[1:], want[1:], rtol=RTOL), (got, want)
    for n, e in gerr.items():
        assert e < GRAD_RTOL, (n, e)
    assert l1(y, y_ref) < RTOL
    assert eng.device_status() == 0
    if persistent:
        assert k[K_GFWD] == 2 and k[K_GBWD] == 1, k       # (g_backward: forward + BPTT; forward)
    else:
        assert k[K_GFWD] == 0 and k[K_GBWD] == 0, k
    return m, o


@pytest.mark.parametrize("B", [32, 8, 64])
def test_reference_width_persistent(B):
    """a full 32-row group; 8 rows padded to 32 (one tile lane); two row groups"""
    _wide_case("B%d_persistent" % B, B, True)


@pytest.mark.parametrize("B", [32, 8, 64])
def test_reference_width_launch_path(B, monkeypatch):
    monkeypatch.setenv("RSRGAN_GPERSIST", "0")            # (handle scope: read at rsrgan_create)
    _wide_case("B%d_launch_path" % B, B, False)


def _two_steps(g_type, B=32, T=6):
    cfg = R.make_cfg() if g_type == "res_lstm_i" else O.NetCfg(g_type=g_type, g_layers=2, g_cells=760, g_proj=257)
    tc = R.table_cfg(cfg) if g_type == "res_lstm_i" else cfg
    from rsrgan_amd.trainer import RNNTrainer
    g, d = rand_params(tc, 77)
    m = RNNTrainer(None, args_for(cfg, B, g_learning_rate=1e-3), ["gpu:0"], max_frames=T, net_overrides=dict(overrides(cfg), flags=1))
    m.set_vars(g, d)
    for i in range(2):
        xs, ls, lns = ragged(cfg, B, T, 60 + i)
        m.step(xs, ls, lns)
    gv, _ = m.get_vars()
    assert m.engine.device_status() == 0
    m.engine.close()
    return {k: v.copy() for k, v in gv.items()}


def test_run_to_run_identical_and_other_generators_undisturbed():
    before = {t: _two_steps(t) for t in ("res_lstm_l", "res_lstm_base")}
    a, b = _two_steps("res_lstm_i"), _two_steps("res_lstm_i")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    for t in before:
        after = _two_steps(t)
        assert all(np.array_equal(before[t][k], after[k]) for k in after), t
    assert not np.array_equal(a[R.FC_W], before["res_lstm_l"][R.FC_W]) and not np.array_equal(a[R.FC_W], before["res_lstm_base"][R.FC_W])


# ---- the stateful forward -----------------------------------------------------------------------------------------------------------

def run_chunks(model, x, ln, cuts):
    outs, pos = [], 0
    for i, n in enumerate(cuts):
        lc = np.clip(ln - pos, 0, n).astype(np.int32)
        outs.append(model.forward_stream(np.ascontiguousarray(x[:, pos:pos + n]), lc, reset=True if i == 0 else None))
        pos += n
    assert pos == x.shape[1]
    return np.concatenate(outs, 1)


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("B", [1, 4])
def test_chunked_small(B, flags):
    cfg = small(3)
    m, o = pair(cfg, B, 16, flags, seed=21)
    x, _, ln = ragged(cfg, B, 37, 22)
    want = o.forward(x, ln)
    y = run_chunks(m, x, ln, (5, 1, 16, 15))
    assert l1(y, want) < LOSS_RTOL and np.abs(y - want).max() < 1e-4
    assert m.engine.device_status() == 0


def test_chunked_reference_width_persistent():
    cfg = R.make_cfg()
    B = 32
    m, o = pair(cfg, B, 12, 1, seed=31)
    x, _, ln = ragged(cfg, B, 36, 32)
    want = o.forward(x, ln)
    m.engine.profile_begin()
    y = run_chunks(m, x, ln, (12, 12, 12))
    k = kinds_of(m.engine)
    err = l1(y, want)
    _margin("B32_chunked_3x12", dict(B=B, T=36, mfcc_l1_chunked=err, kinds={str(i): v for i, v in k.items()}))
    assert err < RTOL and m.engine.device_status() == 0
    assert k[K_GFWD] == 3, k


def test_state_get_reset_set_roundtrip():
    cfg = small(2)
    B = 4
    m, _ = pair(cfg, B, 8, 1, seed=41)
    eng = m.engine
    assert eng.g_state_floats() == 2 * (12 + 9)          # (c, m) per layer; the sums are per frame and carry nothing
    x, _, _ = rand_batch(cfg, B, 16, seed=42)
    a, b_ = np.ascontiguousarray(x[:, :8]), np.ascontiguousarray(x[:, 8:])
    la, lb = np.array([8, 8, 3, 8], np.int32), np.array([8, 5, 0, 1], np.int32)
    m.forward_stream(a, la, reset=True)
    y2 = m.forward_stream(b_, lb)
    m.forward_stream(a, la, reset=True)
    st = eng.g_state_get().clone()
    eng.g_state_reset()
    assert float(eng.g_state_get().abs().sum()) == 0.0
    eng.g_state_set(st)
    z2 = m.forward_stream(b_, lb)
    assert np.array_equal(y2, z2)


# ---- what is refused; checkpoints ---------------------------------------------------------------------------------------------------

def test_rejections():
    from rsrgan_amd import GAN_RNN
    from rsrgan_amd._lib import RsrganError
    from rsrgan_amd.engine_hip import HipEngine
    cfg = small(2)
    kw = dict(batch_size=4, max_frames=5, input_dim=9, output_dim=5, g_type="res_lstm_i", **overrides(cfg))
    with pytest.raises(RsrganError, match="res_lstm_i"):
        HipEngine(flags=1, **kw)                          # no RSRGAN_FLAG_SUPERVISED
    with pytest.raises(RsrganError, match="res_lstm_i"):
        HipEngine(flags=1 | 16, **dict(kw, g_proj=7))     # g_proj != input_dim
    HipEngine(flags=1 | 16, **kw).close()
    with pytest.raises(ValueError, match="Unrecognized G type"):
        GAN_RNN(None, args_for(cfg, 4), ["gpu:0"], max_frames=5, net_overrides=overrides(cfg))


def test_checkpoints(tmp_path):
    cfg = small(2)
    B, T = 4, 5
    m, _ = pair(cfg, B, T, 1, seed=51)
    x, lab, ln = ragged(cfg, B, T, 52)
    m.step(x, lab, ln)
    m.save(str(tmp_path / "i"), 3)
    g0, _ = m.get_vars()
    ref = m.step(x, lab, ln, train=False)
    m2, _ = pair(cfg, B, T, 1, seed=99)
    assert m2.load(str(tmp_path / "i"))
    g1, _ = m2.get_vars()
    assert all(np.array_equal(g0[k], g1[k]) for k in g0) and m2.engine.get_scalar("adam_step") == 1
    assert np.allclose(np.ravel(m2.step(x, lab, ln, train=False)), np.ravel(ref), rtol=1e-6)
    # the variable table is res_lstm_l's: a two-layer res_lstm_l checkpoint loads, and computes this generator on those variables
    lcfg = R.table_cfg(cfg)
    ml, _ = pair(lcfg, B, T, 1, seed=61, g_type="res_lstm_l", g=rand_params(lcfg, 61)[0])
    ml.step(x, lab, ln)
    ml.save(str(tmp_path / "l"), 1)
    gl, _ = ml.get_vars()
    assert m2.load(str(tmp_path / "l"))
    g2, _ = m2.get_vars()
    assert all(np.array_equal(gl[k], g2[k]) for k in gl)
    want = R.generator_fwd(cfg, {k: v.astype(np.float64) for k, v in gl.items()}, x.astype(np.float64), ln)[0]
    assert np.abs(m2.forward(x, ln) - want).max() < 1e-4
