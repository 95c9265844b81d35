"""RNNTrainer(g_type='bnlstm') -- the recurrent batch-norm LSTMP generator of models/bnlstm.py -- on the HIP path against the
fp64 torch oracle of tests/bnlstm_ref.py: losses, every gradient, Adam steps with the moving statistics and the EMA shadows,
the evaluation twin and decode, the full-size model, the variable table and its initial values, a checkpoint round trip,
run-to-run reproducibility and the rejected configurations."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import bnlstm_ref as R
from tests.helpers import NET_G, rel_err, split_flat

pytestmark = pytest.mark.gpu

FLAG_WAVEFRONT, FLAG_GRAPH, FLAG_SUPERVISED = 1, 2, 16


def _args(B, din, dout, **kw):
    a = SimpleNamespace(batch_size=B, input_dim=din, output_dim=dout, left_context=0, right_context=0, g_type="bnlstm",
                        keep_prob=1.0, batch_norm=False, num_gpu=1, save_dir=None, l2_scale=0.0, g_learning_rate=1e-3)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _batch(B, T, din, dout, seed, tmax=None):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, din)).astype(np.float32)
    lab = rng.standard_normal((B, T, dout)).astype(np.float32)
    hi = T if tmax is None else tmax
    ln = rng.integers(max(hi // 2, 1), hi + 1, size=B).astype(np.int32)
    ln[0] = hi
    if B > 2:
        ln[-1] = 1                                       # a row that is padding from its second step on
    return x, lab, ln


def _trainer(B, T, L, H, P, din, dout, flags=FLAG_WAVEFRONT, seed=4321, **kw):
    from rsrgan_amd.trainer import RNNTrainer
    return RNNTrainer(None, _args(B, din, dout, **kw), ["gpu:0"], max_frames=T, seed=seed,
                      net_overrides=dict(g_layers=L, g_cells=H, g_proj=P, flags=flags))


def _g(m):
    return split_flat(m.engine.get_params(NET_G, "variables").cpu().numpy(), m.engine.tensor_table(NET_G))


def _err(a, b):
    """relative error with a floor: with one row every batch-norm site passes no gradient below it (exactly 0 in fp64, fp32
    contraction leftovers of ~1e-17 here)"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-6))


def _check_vars(got, want, tol, names):
    for k in names:
        assert _err(got[k], want[k]) < tol, (k, _err(got[k], want[k]))


# (B, flags, longest length): B=5 replays hipGraphs and ends before T; the kernels run ceil(B / 16) row tiles: 1 .. 4 (B = 64, the
# largest batch the C ABI takes)
SMALL = [(1, 1, None), (5, 3, 5), (40, 1, None), (24, 1, None), (64, 3, None)]


@pytest.mark.parametrize("B,flags,tmax", SMALL)
def test_small_against_oracle(B, flags, tmax):
    _small_case(B, flags, tmax, 2, 12, 7, 6, 5, 7)


def test_wide_cell_partial_tiles_against_oracle():
    """K > 128 (layer 1's input and every state kernel read P = 150 columns) and partial 16-column tiles (H = 100, P = 150), three
    row tiles with a one-row last tile (B = 33)"""
    _small_case(33, 1, None, 2, 100, 150, 24, 20, 6)


def _small_case(B, flags, tmax, L, H, P, din, dout, T):
    specs = R.param_specs(din, dout, L, H, P)
    p0 = R.rand_params(specs, 11)
    m = _trainer(B, T, L, H, P, din, dout, flags, l2_scale=1e-3)
    assert [n for n, _, _ in m.engine.tensor_table(NET_G)] == [n for n, _ in specs]
    m.set_vars(p0, None)
    o = R.BnlstmOracle(p0, L, output_dim=dout, l2_scale=1e-3, g_learning_rate=float(np.float32(1e-3)))
    x, lab, ln = _batch(B, T, din, dout, 5, tmax)
    got = m.engine.g_backward(x, lab, ln, None, train=True, apply=False).cpu().numpy()
    want, wg, mom = o.tower(x, lab, ln, train=True)
    assert got[0] == 0.0 and np.allclose(got[1:], want[1:], rtol=1e-4), (got, want)
    gr = split_flat(m.engine.get_grads(NET_G).cpu().numpy(), m.engine.tensor_table(NET_G))
    _check_vars(gr, wg, 2e-3, wg)
    for k in o.moving:
        assert not np.any(gr[k]), k                      # no gradient for the moving statistics
    m.engine.apply(NET_G)
    o.update_moving(mom)
    from oracle import rsrgan_oracle as O
    O.GanRnnOracle.apply_g(o, wg)
    for i in range(2):
        xs, ls, lns = _batch(B, T, din, dout, 20 + i, tmax)
        got = np.ravel(m.step(xs, ls, lns))
        w = o.step(xs, ls, lns)
        assert np.allclose(got, np.ravel(w)[1:], rtol=2e-4), (i, got, w)
    gv = _g(m)
    _check_vars(gv, o.params(), 1e-3, o.g)
    _check_vars(gv, o.params(), 1e-4, o.moving)
    ema = split_flat(m.engine.get_params(NET_G, "ema").cpu().numpy(), m.engine.tensor_table(NET_G))
    _check_vars(ema, o.params(ema=True), 1e-3, o.g)
    # the cross_validation twin's fetch and decode normalise with the moving statistics and leave them as they are
    from rsrgan_amd.trainer import RNNTrainer
    tw = RNNTrainer(None, _args(B, din, dout, l2_scale=1e-3), ["gpu:0"], cross_validation=True, share_engine_from=m)
    before = m.engine.get_params(NET_G, "variables").cpu().numpy()
    ev = np.ravel(tw.step(x, lab, ln))
    w, _, _ = o.tower(x, lab, ln, train=False)
    assert np.allclose(ev, np.ravel(w)[1:], rtol=2e-4, atol=1e-7) and ev[1] == 0.0, (ev, w)
    y = m.forward(x, ln)
    assert rel_err(y, o.forward(x, ln)) < 2e-4
    assert np.array_equal(before, m.engine.get_params(NET_G, "variables").cpu().numpy())


def test_full_size_against_oracle():
    """3 x BNLSTMCell(760, num_proj=280) at run_rnn.sh's shape (Din = Dout = 40, batch_size 8), T = 100, ragged"""
    L, H, P, din, dout, B, T = 3, 760, 280, 40, 40, 8, 100
    specs = R.param_specs(din, dout, L, H, P)
    p0 = R.rand_params(specs, 3)
    m = _trainer(B, T, L, H, P, din, dout, FLAG_WAVEFRONT | FLAG_GRAPH)
    m.set_vars(p0, None)
    o = R.BnlstmOracle(p0, L, output_dim=dout)
    x, lab, ln = _batch(B, T, din, dout, 9)
    got = m.engine.g_backward(x, lab, ln, None, train=True, apply=False).cpu().numpy()
    want, wg, mom = o.tower(x, lab, ln, train=True)
    assert np.allclose(got[1:], want[1:], rtol=1e-4), (got, want)
    gr = split_flat(m.engine.get_grads(NET_G).cpu().numpy(), m.engine.tensor_table(NET_G))
    _check_vars(gr, wg, 2e-3, wg)
    o.update_moving(mom)
    _check_vars(_g(m), o.params(), 1e-4, o.moving)


def test_full_size_four_row_tiles_against_oracle():
    """the full-width cell (3 x BNLSTMCell(760, num_proj=280)) at B = 64 (four 16-row tiles), T = 12, ragged: gradients and moving statistics"""
    L, H, P, din, dout, B, T = 3, 760, 280, 40, 40, 64, 12
    specs = R.param_specs(din, dout, L, H, P)
    p0 = R.rand_params(specs, 5)
    m = _trainer(B, T, L, H, P, din, dout, FLAG_WAVEFRONT | FLAG_GRAPH)
    m.set_vars(p0, None)
    o = R.BnlstmOracle(p0, L, output_dim=dout)
    x, lab, ln = _batch(B, T, din, dout, 13)
    got = m.engine.g_backward(x, lab, ln, None, train=True, apply=False).cpu().numpy()
    want, wg, mom = o.tower(x, lab, ln, train=True)
    assert np.allclose(got[1:], want[1:], rtol=1e-4), (got, want)
    gr = split_flat(m.engine.get_grads(NET_G).cpu().numpy(), m.engine.tensor_table(NET_G))
    _check_vars(gr, wg, 2e-3, wg)
    o.update_moving(mom)
    _check_vars(_g(m), o.params(), 1e-4, o.moving)


def test_table_and_initial_values():
    from rsrgan_amd.trainer import RNNTrainer
    din, dout, H, P = 40, 40, 760, 280
    m = RNNTrainer(None, _args(8, din, dout), ["gpu:0"], max_frames=4)
    table = [(n, tuple(s)) for n, s, _ in m.engine.tensor_table(NET_G)]
    assert table == [(n, tuple(s)) for n, s in R.param_specs(din, dout, 3, H, P)]
    g = _g(m)
    sd = np.sqrt(2.0 / P)
    w = g["g_model/fully_connected/weights"]
    assert np.abs(w).max() <= 2 * sd * (1 + 1e-6) and abs(w.std() - 0.88 * sd) < 0.05 * sd      # truncated at 2 sigma
    for k in ("g_model/fully_connected/biases", "g_model/fully_connected_1/biases"):
        assert not np.any(g[k]), k
    for l in range(3):
        pre = R.cell_prefix(l)
        for site in ("input", "state", "cell"):
            assert np.all(g[pre + site + "/scale"] == np.float32(0.1)) and not np.any(g[pre + site + "/offset"])
            assert not np.any(g[pre + site + "/moving_mean"]) and np.all(g[pre + site + "/moving_var"] == 1.0)
        b = g[pre + "bias"]
        assert np.all(b != 0) and np.abs(b).max() <= np.sqrt(3.0 / (4 * H)) * (1 + 1e-6)
        for d in ("W_F_diag", "W_I_diag", "W_O_diag"):
            assert np.abs(g[pre + d]).max() <= np.sqrt(3.0 / H) * (1 + 1e-6) and np.any(g[pre + d])
        lim = np.sqrt(6.0 / (P + 4 * H))
        assert np.abs(g[pre + "input_kernel"]).max() <= lim * (1 + 1e-6) and np.abs(g[pre + "state_kernel"]).max() <= lim * (1 + 1e-6)


def test_checkpoint_decode_uses_ema_weights_and_raw_statistics(tmp_path):
    L, H, P, din, dout, B, T = 2, 12, 7, 6, 5, 5, 6
    specs = R.param_specs(din, dout, L, H, P)
    p0 = R.rand_params(specs, 21)
    m = _trainer(B, T, L, H, P, din, dout)
    m.set_vars(p0, None)
    o = R.BnlstmOracle(p0, L, output_dim=dout, g_learning_rate=float(np.float32(1e-3)))
    for i in range(2):
        xs, ls, lns = _batch(B, T, din, dout, 40 + i)
        m.step(xs, ls, lns)
        o.step(xs, ls, lns)
    m.save(str(tmp_path), 2)
    m2 = _trainer(B, T, L, H, P, din, dout, seed=99)
    assert m2.load(str(tmp_path), moving_average=True)
    x, _, ln = _batch(B, T, din, dout, 50)
    assert rel_err(m2.forward(x, ln), o.forward(x, ln, ema=True)) < 2e-4


def test_reproducible():
    L, H, P, din, dout, B, T = 2, 40, 24, 6, 5, 16, 9
    outs = []
    for _ in range(2):
        m = _trainer(B, T, L, H, P, din, dout, FLAG_WAVEFRONT | FLAG_GRAPH, seed=7, l2_scale=1e-3)
        for i in range(2):
            xs, ls, lns = _batch(B, T, din, dout, 60 + i)
            m.step(xs, ls, lns)
        outs.append(m.engine.get_params(NET_G, "variables").cpu().numpy().tobytes())
        m.engine.close()
    assert outs[0] == outs[1]


def test_rejections():
    from rsrgan_amd import _lib
    from rsrgan_amd.gan_rnn import GAN_RNN
    with pytest.raises(ValueError):
        GAN_RNN(None, _args(4, 6, 5), ["gpu:0"], max_frames=4)
    with pytest.raises(NotImplementedError):
        _trainer(4, 4, 2, 12, 7, 6, 5, keep_prob=0.75)
    with pytest.raises(NotImplementedError):
        _trainer(4, 4, 2, 12, 7, 6, 5, batch_norm=True)
    lib = _lib.load()
    for B, flags in ((8, FLAG_WAVEFRONT), (65, FLAG_WAVEFRONT | FLAG_SUPERVISED), (8, FLAG_WAVEFRONT | FLAG_SUPERVISED | _lib.FLAG_BATCH_NORM)):
        cfg = _lib.RsrganCfg()
        assert lib.rsrgan_default_cfg(5, C.byref(cfg)) == 0
        cfg.batch_size, cfg.max_frames, cfg.input_dim, cfg.output_dim, cfg.flags = B, 4, 6, 5, flags
        h = C.c_void_p()
        assert lib.rsrgan_create(C.byref(cfg), C.c_uint64(1), C.byref(h)) == -1, (B, flags)
        assert b"bnlstm" in lib.rsrgan_last_error()
    m = _trainer(4, 4, 2, 12, 7, 6, 5)
    assert lib.rsrgan_set_dropout(m.engine.h, C.c_float(0.5), C.c_uint64(1)) == -1
