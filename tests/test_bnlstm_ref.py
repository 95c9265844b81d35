"""The fp64 bnlstm oracle (tests/bnlstm_ref.py) on CPU: its batch norm, its autograd gradients against central finite
differences (rows past their length included), the moving statistics of a training step, and the C ABI's defaults for the
bnlstm generator type."""
import ctypes as C

import numpy as np
import torch

from tests import bnlstm_ref as R

DIN, DOUT, L, H, P = 4, 3, 2, 5, 3


def _tiny(seed=3):
    specs = R.param_specs(DIN, DOUT, L, H, P)
    p = R.rand_params(specs, seed)
    rng = np.random.default_rng(seed + 1)
    x = rng.standard_normal((3, 4, DIN))
    lab = rng.standard_normal((3, 4, DOUT))
    ln = np.array([4, 2, 1], np.int32)                     # ragged, one row of length 1
    return specs, p, x, lab, ln


def test_step_batch_norm_equals_formula():
    specs, p, x, lab, ln = _tiny()
    pt = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in p.items()}
    _, mom = R.forward(pt, x, ln, L, train=True)
    pre = R.cell_prefix(0)
    h0 = np.maximum(x @ p["g_model/fully_connected/weights"].astype(np.float64) + p["g_model/fully_connected/biases"], 0.0)
    for t in range(x.shape[1]):
        xh = h0[:, t] @ p[pre + "input_kernel"].astype(np.float64)
        assert np.allclose(mom[pre + "input/moving_mean"][t], xh.mean(0), rtol=0, atol=1e-13)
        assert np.allclose(mom[pre + "input/moving_var"][t], xh.var(0), rtol=0, atol=1e-13)      # biased
    # the formula against torch's own training-mode batch norm (biased variance in the normalisation)
    v = np.random.default_rng(0).standard_normal((6, 7))
    sc, of = np.linspace(0.2, 1.4, 7), np.linspace(-0.3, 0.3, 7)
    ref = torch.nn.functional.batch_norm(torch.tensor(v), None, None, torch.tensor(sc), torch.tensor(of), training=True,
                                         eps=R.EPS).numpy()
    assert np.allclose(R.bn_formula(v, sc, of), ref, rtol=0, atol=1e-12)


def test_autograd_matches_finite_differences():
    specs, p, x, lab, ln = _tiny()
    o = R.BnlstmOracle(p, L, output_dim=DOUT)
    _, grads, _ = o.tower(x, lab, ln, train=True)

    def loss(params, xx):
        pt = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in params.items()}
        y, _ = R.forward(pt, xx, ln, L, train=True)
        return float(0.5 * DOUT * torch.mean((y - torch.tensor(lab)) ** 2))

    eps = 1e-6
    base = {k: np.asarray(v, np.float64) for k, v in p.items()}
    for name, _ in specs:
        if R.is_moving(name):
            continue
        fd = np.zeros_like(base[name])
        for idx in np.ndindex(fd.shape):
            old = base[name][idx]
            base[name][idx] = old + eps; lp = loss(base, x)
            base[name][idx] = old - eps; lm = loss(base, x)
            base[name][idx] = old
            fd[idx] = (lp - lm) / (2 * eps)
        err = np.linalg.norm(grads[name] - fd) / max(np.linalg.norm(fd), 1e-12)
        assert err < 1e-6, (name, err)
    # the padded frames of the length-1 row (fed like a parameter) reach the loss only through the batch statistics of the
    # steps past its length: their gradient is not zero, and autograd has it right
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    pt = {k: torch.tensor(v) for k, v in base.items()}
    y, _ = R.forward(pt, xt, ln, L, train=True)
    (0.5 * DOUT * torch.mean((y - torch.tensor(lab)) ** 2)).backward()
    g_pad = xt.grad.numpy()[2, 1:]
    assert np.abs(g_pad).max() > 1e-6
    for idx in np.ndindex(g_pad.shape):
        xx = np.array(x, np.float64)
        xx[(2, 1 + idx[0], idx[1])] += eps; lp = loss(base, xx)
        xx[(2, 1 + idx[0], idx[1])] -= 2 * eps; lm = loss(base, xx)
        assert abs((lp - lm) / (2 * eps) - g_pad[idx]) < 1e-6 * max(1.0, abs(g_pad[idx])), idx


def test_moving_statistics_are_the_sequential_ema():
    specs, p, x, lab, ln = _tiny(7)
    o = R.BnlstmOracle(p, L, output_dim=DOUT, g_learning_rate=1e-3)
    start = {k: v.copy() for k, v in o.moving.items()}
    _, _, mom = o.tower(x, lab, ln, train=True)
    o.step(x, lab, ln)
    T = x.shape[1]
    for k, v in o.moving.items():
        mu = mom[k]
        closed = R.DECAY ** T * start[k] + sum((1 - R.DECAY) * R.DECAY ** (T - 1 - t) * mu[t] for t in range(T))
        assert np.allclose(v, closed, rtol=1e-12, atol=1e-14), k
        assert not np.allclose(v, start[k])
    # an evaluation fetch leaves them alone
    before = {k: v.copy() for k, v in o.moving.items()}
    o.step(x, lab, ln, train=False)
    for k in before:
        assert np.array_equal(before[k], o.moving[k])


def test_default_cfg_of_bnlstm_through_ctypes():
    from rsrgan_amd import _lib
    lib = _lib.load()
    cfg = _lib.RsrganCfg()
    assert _lib.G_TYPES["bnlstm"] == 5
    assert lib.rsrgan_default_cfg(5, C.byref(cfg)) == 0
    assert (cfg.g_type, cfg.g_layers, cfg.g_cells, cfg.g_proj) == (5, 3, 760, 280)        # models/bnlstm.py:41-43
    assert cfg.lrelu_alpha == 0.0 and cfg.forget_bias == 1.0 and cfg.clip_norm == 15.0


def test_checkpoint_loader_reads_bnlstm_statistics_raw():
    from rsrgan_amd.gan_rnn import _bn_statistic
    pre = R.cell_prefix(1)
    assert _bn_statistic(pre + "cell/moving_mean") and _bn_statistic(pre + "state/moving_var")
    assert not _bn_statistic(pre + "cell/scale") and not _bn_statistic(pre + "bias") and not _bn_statistic(pre + "input_kernel")
    assert _bn_statistic("g_model/fully_connected/BatchNorm/moving_mean")
