"""Pins tests/seq_bn_ref.py (the fp64 reference of batch norm on the sequence path) on the CPU: central differences for every
trainable tensor from a NON-initial statistics state (at the initial state r = 1 and d = 0 for any batch: the corrections would go
untested), the L2 term over beta and gamma, the update-op counts of a D-run and a G-run, the evaluation path."""
import numpy as np
import pytest

from oracle import bn_renorm as BN
from oracle import rsrgan_oracle as O
from tests import seq_bn_ref as R
from tests.helpers import rand_batch, small_cfg

B, T = 3, 5


def make(supervised=False, l2_scale=1e-3, seed=3, **kw):
    cfg = small_cfg()
    g, d = R.rand_params(cfg, seed)
    g = {k: np.asarray(v, np.float64) for k, v in g.items()}
    d = {k: np.asarray(v, np.float64) for k, v in d.items()}
    o = R.SeqBnOracle(cfg, g, d, batch_size=B, l2_scale=l2_scale, supervised=supervised, g_learning_rate=1e-3, **kw)
    x, lab, ln = rand_batch(cfg, B, T, seed=9, ragged=True)
    return cfg, o, x.astype(np.float64), lab.astype(np.float64), ln


def test_specs_have_no_biases_and_eight_batch_norm_variables():
    cfg = small_cfg()
    names = [n for n, _ in R.g_param_specs(cfg)]
    assert names[0] == "g_model/fully_connected/weights"
    assert names[1:9] == [R.PRE + k for k in ("beta", "gamma", "moving_mean", "moving_variance", "renorm_mean", "renorm_mean_weight",
                                             "renorm_stddev", "renorm_stddev_weight")]
    assert "g_model/fully_connected/biases" not in names and names[9].startswith("g_model/rnn/")


@pytest.mark.parametrize("supervised", [False, True])
def test_gradients_match_central_differences_from_a_non_initial_state(supervised):
    cfg, o, x, lab, ln = make(supervised)
    # the state is far from the initial one: the corrections r, d carry weight
    _, cache = R.generator_fwd(cfg, o.params(), x, ln, True)
    assert np.abs(cache["bn"]["r"] - 1).max() > 0.2 and np.abs(cache["bn"]["d"]).max() > 0.2
    _, grads, _ = o.g_tower(x, lab, ln, want_grads=True)
    assert set(grads) == set(o.g)
    o.frozen = (cache["bn"]["r"], cache["bn"]["d"])        # stop_gradient: the differences below hold the corrections fixed
    rng = np.random.default_rng(5)
    h = 1e-6
    for name in o.g:
        flat = o.g[name].reshape(-1)
        for i in rng.choice(flat.size, min(3, flat.size), replace=False):
            keep = flat[i]
            flat[i] = keep + h; lp = o.g_tower(x, lab, ln, want_grads=True)[0][3]
            flat[i] = keep - h; lm = o.g_tower(x, lab, ln, want_grads=True)[0][3]
            flat[i] = keep
            num, ana = (lp - lm) / (2 * h), grads[name].reshape(-1)[i]
            assert abs(num - ana) <= 1e-6 * max(1.0, abs(ana)), (name, i, num, ana)


def test_l2_term_includes_beta_and_gamma():
    cfg, o, x, lab, ln = make()
    (_, _, l2, _), grads, _ = o.g_tower(x, lab, ln, want_grads=True)
    want = 1e-3 * sum(0.5 * float(np.sum(v * v)) for k, v in o.g.items() if "bias" not in k)
    assert np.isclose(l2, want, rtol=1e-12)
    o0 = make(l2_scale=0.0)[1]
    _, g0, _ = o0.g_tower(x, lab, ln, want_grads=True)
    for k in (R.PRE + "beta", R.PRE + "gamma"):
        assert np.allclose(grads[k] - g0[k], 1e-3 * o.g[k], rtol=1e-9, atol=1e-15), k
        without = want - 1e-3 * 0.5 * float(np.sum(o.g[k] ** 2))
        assert not np.isclose(l2, without, rtol=1e-6)
    assert all(not BN.is_state(k) for k in grads)


def test_d_run_leaves_the_state_alone_and_g_run_commits_twice():
    cfg, o, x, lab, ln = make()
    before = {k: np.array(v) for k, v in o.state.items()}
    o.d_step(x, lab, ln)
    assert o.commits == 0 and all(np.array_equal(before[k], o.state[k]) for k in before)
    _, cache = R.generator_fwd(cfg, o.params(), x, ln, True)
    o.g_step(x, lab, ln)
    assert o.commits == 2
    want = dict(before)
    BN.commit(want, cache["bn"]); BN.commit(want, cache["bn"])
    for k in before:
        assert np.allclose(o.state[k], want[k], rtol=1e-14), k
        assert not np.array_equal(o.state[k], before[k]), k
    # evaluation fetches commit nothing
    o.g_step(x, lab, ln, train=False); o.d_step(x, lab, ln, train=False)
    assert o.commits == 2


def test_eval_path_is_forward_infer():
    cfg, o, x, lab, ln = make()
    p = o.params()
    y_eval = o.forward_infer(x, ln)
    # by hand: forward_infer on x.W, then the layers of the project oracle on the activated input
    z = (x @ p[R.SCOPE + "/weights"]).reshape(B * T, -1)
    h = O.leakyrelu(BN.forward_infer(p, R.SCOPE, z), cfg.lrelu_alpha).reshape(B, T, -1)
    ins = h
    for l in range(cfg.g_layers):
        ins, _ = O.lstmp_fwd(ins, ln, O._layer_params(p, "g_model/rnn/multi_rnn_cell/cell_%d/lstm_cell" % l, True), cfg.forget_bias)
    y = O.fc_fwd(ins, p["g_model/fully_connected_1/weights"], p["g_model/fully_connected_1/biases"])
    assert np.allclose(y_eval, y, rtol=1e-13, atol=1e-15)
    assert not np.allclose(y_eval, o.forward(x, ln), rtol=1e-3)            # (the training forward normalises with the batch moments)
    ev = o.g_step(x, lab, ln, train=False)
    assert ev[2] == [0.0]                                                   # no L2 on the evaluation fetch
    ocv = make(cross_validation=True)[1]
    assert np.allclose(ocv.forward(x, ln), y_eval, rtol=1e-13)
