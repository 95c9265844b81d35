"""tests/res_lstm_i_ref.py pinned on the CPU: its gradients against central differences, its forward against the oracle's res_lstm_l
where the two generators must agree or differ by a known term, and the padded frames (models/res_lstm_i.py:101-199)."""
import dataclasses

import numpy as np

from oracle import rsrgan_oracle as O
from tests import res_lstm_i_ref as R


def _tiny(L=2):
    cfg = R.make_cfg(input_dim=3, output_dim=2, g_layers=L, g_cells=4, g_proj=3)
    rng = np.random.default_rng(7)
    g = {k: v.astype(np.float64) for k, v in R.rand_g(cfg, 3).items()}
    B, T = 3, 4
    x = rng.standard_normal((B, T, 3))
    lab = rng.standard_normal((B, T, 2))
    ln = np.array([4, 1, 2], np.int32)              # a length-1 row, a padded tail
    return cfg, g, x, lab, ln


def _loss(cfg, g, x, lab, ln, l2=1e-2, drop=None):
    y, _ = R.generator_fwd(cfg, g, x, ln, drop)
    return O.g_mse(y, lab, cfg.output_dim)[0] + O.l2_term(g, l2)[0]


def test_variable_table_is_res_lstm_l():
    cfg = R.make_cfg()
    specs = R.g_param_specs(cfg)
    assert specs == O.g_param_specs(O.NetCfg.res_lstm_l(g_layers=2))
    assert [n for n, _ in specs][:6] == [R.cell(0) + s for s in ("/kernel", "/bias", "/w_f_diag", "/w_i_diag", "/w_o_diag", "/projection/kernel")]
    assert dict(specs)[R.cell(1) + "/kernel"] == (257 + 257, 4 * 760) and [n for n, _ in specs][-2:] == [R.FC_W, R.FC_B]


def test_gradients_match_central_differences():
    for L, masks in ((2, False), (3, False), (2, True)):
        cfg, g, x, lab, ln = _tiny(L)
        drop = None
        if masks:
            mk = [np.random.default_rng(50 + l).integers(0, 2, (3, 4, 3)).astype(np.float64) for l in range(L)]
            drop = (0.75, lambda l: mk[l])
        o = R.ResLstmIOracle(cfg, g, batch_size=3, l2_scale=1e-2, keep_prob=0.75 if masks else 1.0, mask_fn=(lambda run, tw, l, b, t, p: mk[l]) if masks else None)
        _, grads, _ = o.g_tower(x, lab, ln)
        eps = 1e-6
        for k in g:
            num = np.zeros_like(g[k])
            it = np.nditer(g[k], flags=["multi_index"])
            for _ in it:
                i = it.multi_index
                keep = g[k][i]
                g[k][i] = keep + eps; up = _loss(cfg, g, x, lab, ln, drop=drop)
                g[k][i] = keep - eps; dn = _loss(cfg, g, x, lab, ln, drop=drop)
                g[k][i] = keep
                num[i] = (up - dn) / (2 * eps)
            assert np.abs(num - grads[k]).max() < 1e-7 * max(1.0, np.abs(num).max()), (L, masks, k)


def test_one_layer_is_res_lstm_l():
    cfg, g, x, lab, ln = _tiny(1)
    y, _ = R.generator_fwd(cfg, g, x, ln)
    want, _ = O.generator_fwd(R.table_cfg(cfg), g, x, ln)
    assert np.abs(y - want).max() < 1e-12


def test_two_layers_differ_from_res_lstm_l_by_out1_through_the_fc():
    """res_lstm_l's FC reads out_2 + out_1 + x, this one out_2 + x, and both feed layer 2 the same out_1 + x"""
    cfg, g, x, lab, ln = _tiny(2)
    y, c = R.generator_fwd(cfg, g, x, ln)
    want, _ = O.generator_fwd(R.table_cfg(cfg), g, x, ln)
    live = (np.arange(4)[None, :] < ln[:, None])[:, :, None]
    diff = np.where(live, c["outs"][0] @ g[R.FC_W], 0.0)
    assert np.abs((want - y) - diff).max() < 1e-12 and np.abs(diff).max() > 1e-3
    assert np.abs(np.where(live, 0.0, want - y)).max() == 0.0


def test_three_layers_middle_input_is_out_plus_x_not_the_running_sum():
    cfg, g, x, lab, ln = _tiny(3)
    _, c = R.generator_fwd(cfg, g, x, ln)
    assert np.array_equal(c["ins"][2], c["outs"][1] + x)
    _, cl = O.generator_fwd(R.table_cfg(cfg), g, x, ln)
    assert np.abs(cl["ins"][2] - c["ins"][2]).max() > 1e-3


def test_padded_frames_are_the_fc_of_the_input():
    cfg, g, x, lab, ln = _tiny(2)
    y, c = R.generator_fwd(cfg, g, x, ln)
    pad = np.arange(4)[None, :] >= ln[:, None]
    assert pad.sum() == 5
    assert np.abs(y - (x @ g[R.FC_W] + g[R.FC_B]))[pad].max() < 1e-15
    for l in range(1, 3):
        assert np.array_equal(c["ins"][l][pad], x[pad])


def test_supervised_step_is_clip_adam_ema():
    cfg, g, x, lab, ln = _tiny(2)
    o = R.ResLstmIOracle(cfg, g, batch_size=3, l2_scale=1e-2, g_learning_rate=1e-2, clip_norm=0.05)
    _, grads, _ = o.g_tower(x, lab, ln)
    adv, mse, l2, tot = (v[0] for v in o.g_step(x, lab, ln))
    assert adv == 0.0 and abs(tot - (mse + l2)) < 1e-15 and l2 > 0
    k = R.cell(1) + "/kernel"
    gc = O.clip_by_norm(grads[k], 0.05)
    assert np.linalg.norm(grads[k]) > 0.05 and abs(np.linalg.norm(gc) - 0.05) < 1e-12
    lr_t = 1e-2 * np.sqrt(1 - 0.999) / (1 - 0.9)
    want = g[k] - lr_t * (0.1 * gc) / (np.sqrt(0.001 * gc * gc) + 1e-8)
    assert np.abs(o.g[k] - want).max() < 1e-12
    assert np.abs(o.g_ema[k] - (0.9999 * g[k] + 0.0001 * o.g[k])).max() < 1e-15
    o.cross_validation = True
    ev = o.g_step(x, lab, ln, train=False)
    assert ev[2][0] == 0.0 and o.adam_t == 1
    assert dataclasses.asdict(cfg)["g_type"] == "res_lstm_i"
