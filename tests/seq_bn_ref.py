"""fp64 reference of args.batch_norm on the sequence path: g_type lstm with the input layer
leakyrelu_0.3(batch_norm(x.W, is_training, scale=True, renorm=True)), no bias (models/lstm.py:61-87), under GAN_RNN
(models/gan_rnn_placeholder.py) and RNNTrainer (models/rnn_trainer.py).  Composed from oracle.rsrgan_oracle (lstmp_fwd / lstmp_bwd,
fc_fwd / fc_bwd, the losses, l2_term, clip_by_norm, the Adam + EMA form of GanRnnOracle) and oracle.bn_renorm (forward_train,
backward_train, commit, forward_infer); it modifies neither.

The moments run over all B.T frames of the batch, the t >= len frames included (x = 0 there, so z = 0).  Update ops, by scope
(gan_rnn_placeholder.py:164-175): the discriminator has none -- a D-run commits nothing and only reads the state; a G-run (and an
RNNTrainer step) commits the generator's update TWICE with the same batch (tower 0 builds G with reuse=False and again with
reuse=True, :196,204; rnn_trainer.py:131-132,148-150).  Corrections read the state from the start of the run, commits happen at its
end.  beta and gamma are trainable g_ variables without "bias" in their names: they take the L2 term (:254), are clipped per tensor,
get Adam and an EMA shadow; the six statistics take nothing."""
from __future__ import annotations

import numpy as np

from oracle import bn_renorm as BN
from oracle import rsrgan_oracle as O

SCOPE = "g_model/fully_connected"
PRE = SCOPE + "/BatchNorm/"


def g_param_specs(cfg):
    """the variables in creation order: weights, the eight BatchNorm variables (no biases), the cells, the output FC"""
    base = O.g_param_specs(cfg)
    assert base[0][0] == SCOPE + "/weights" and base[1][0] == SCOPE + "/biases"
    P = base[0][1][1]
    return [base[0]] + [(n, tuple(s)) for n, s in BN.var_specs(SCOPE, P)] + list(base[2:])


def rand_params(cfg, seed=0, initial_state=False):
    """fp32-rounded: the project's xavier weights and small random biases; gamma signed-free in (0.5, 1.5), beta ~ N(0, 0.3); the statistics
    away from their initial values (r far from 1, d far from 0) unless initial_state"""
    from tests.helpers import rand_params as base_params
    g0, d = base_params(cfg, seed)
    rng = np.random.default_rng([seed, 77])
    g = {}
    for name, shape in g_param_specs(cfg):
        if name in g0:
            g[name] = g0[name]
            continue
        leaf = name.rsplit("/", 1)[-1]
        if initial_state and BN.is_state(name):
            v = BN.init_vars(SCOPE, shape[0] if shape else 1)[name]
        elif leaf == "gamma":
            v = rng.uniform(0.5, 1.5, shape)
        elif leaf == "beta":
            v = rng.normal(0, 0.3, shape)
        elif leaf == "moving_mean":
            v = rng.normal(0, 0.5, shape)
        elif leaf == "moving_variance":
            v = rng.uniform(0.3, 2.0, shape)
        elif leaf == "renorm_mean":
            v = rng.normal(0, 0.3, shape)
        elif leaf == "renorm_stddev":
            v = rng.uniform(0.2, 0.9, shape)
        else:                                              # the two scalar weights
            v = rng.uniform(0.3, 0.8, shape)
        g[name] = np.asarray(v, np.float32).reshape(shape)
    return g, d


def generator_fwd(cfg, params, x, lengths, train, frozen=None):
    """x [B, T, Din] -> (y [B, T, Dout], cache).  train: batch moments and the renorm corrections; else the moving statistics.
    frozen = (r, d): the corrections held at these values instead of the batch's own (they are stop_gradient in the reference, so a
    finite difference of the loss must not move them)"""
    hp = cfg.g_proj > 0
    W = params[SCOPE + "/weights"]
    B, T, _ = x.shape
    z = O.fc_fwd(x, W, np.zeros(W.shape[1], x.dtype)).reshape(B * T, -1)
    cache = {"x": x}
    if train:
        a, cache["bn"] = BN.forward_train(params, SCOPE, z)
        if frozen is not None:
            r, d = frozen
            a = cache["bn"]["xhat"] * (r * params[PRE + "gamma"]) + (d * params[PRE + "gamma"] + params[PRE + "beta"])
    else:
        a = BN.forward_infer(params, SCOPE, z)
    cache["a"] = a
    ins = [O.leakyrelu(a, cfg.lrelu_alpha).reshape(B, T, -1)]
    for l in range(cfg.g_layers):
        pre = "g_model/rnn/multi_rnn_cell/cell_%d/lstm_cell" % l
        out, c = O.lstmp_fwd(ins[-1], lengths, O._layer_params(params, pre, hp), cfg.forget_bias)
        cache[pre] = c
        ins.append(out)
    cache["ins"] = ins
    y = O.fc_fwd(ins[-1], params["g_model/fully_connected_1/weights"], params["g_model/fully_connected_1/biases"])
    return y, cache


def generator_bwd(cfg, params, cache, dy):
    """gradients of the trainables (the statistics have none); a training forward's cache"""
    hp = cfg.g_proj > 0
    grads = {}
    ins = cache["ins"]
    d, dw, db = O.fc_bwd(ins[-1], params["g_model/fully_connected_1/weights"], dy)
    grads["g_model/fully_connected_1/weights"], grads["g_model/fully_connected_1/biases"] = dw, db
    for l in range(cfg.g_layers - 1, -1, -1):
        pre = "g_model/rnn/multi_rnn_cell/cell_%d/lstm_cell" % l
        d, g = O.lstmp_bwd(d, cache[pre], O._layer_params(params, pre, hp))
        O._put_layer_grads(grads, pre, g)
    B, T, P = d.shape
    da = d.reshape(B * T, P) * np.where(cache["a"] > 0, 1.0, cfg.lrelu_alpha)
    dz, bn_grads = BN.backward_train(params, cache["bn"], da)
    grads.update(bn_grads)
    _, dw, _ = O.fc_bwd(cache["x"], params[SCOPE + "/weights"], dz.reshape(B, T, P))
    grads[SCOPE + "/weights"] = dw
    return grads


class SeqBnOracle(O.GanRnnOracle):
    """GanRnnOracle with the batch-normalised input layer: self.g holds the trainables (Adam, EMA, L2, clip), self.state the six
    statistics.  supervised=True: RNNTrainer's graph (no discriminator)."""

    def __init__(self, cfg, g_params, d_params, *, supervised=False, **kw):
        self.order = [n for n, _ in g_param_specs(cfg)]
        assert list(g_params) == self.order, "variables out of creation order"
        train = {k: v for k, v in g_params.items() if not BN.is_state(k)}
        super().__init__(cfg, train, d_params, **kw)
        self.state = {k: np.array(v, np.float64).reshape(() if k.endswith("_weight") else np.shape(v))
                      for k, v in g_params.items() if BN.is_state(k)}
        self.supervised = supervised
        self.commits = 0
        self.frozen = None                         # (r, d) for finite differences, see generator_fwd

    def params(self, ema=False):
        src = dict(self.g_ema if ema else self.g)
        src.update(self.state)
        return {k: src[k] for k in self.order}

    def _training(self, want_grads):
        return want_grads and not self.cross_validation

    def forward(self, inputs, lengths, train=True):
        """model.g_outputs of the training model is built with is_training (batch moments); train=False: the cross_validation twin"""
        x = np.asarray(inputs, self.dtype)
        return generator_fwd(self.cfg, self.params(), x, np.asarray(lengths).astype(np.int32), train and not self.cross_validation)[0]

    def forward_infer(self, inputs, lengths, ema=False):
        return generator_fwd(self.cfg, self.params(ema), np.asarray(inputs, self.dtype), np.asarray(lengths).astype(np.int32), False)[0]

    def d_tower(self, x, lab, ln, noise_real=None, noise_fake=None, want_grads=True, tower=0):
        cfg = self.cfg
        y, _ = generator_fwd(cfg, self.params(), x, ln, self._training(want_grads))
        lr_, cr = O.discriminator_fwd(cfg, self.d, lab, ln, noise_real)
        lf_, cf = O.discriminator_fwd(cfg, self.d, y, ln, noise_fake)
        d_rl, dlr = O.lsgan_mean_sq(lr_, self.d_real)
        d_fk, dlf = O.lsgan_mean_sq(lf_, self.d_fake)
        grads = None
        if want_grads:
            _, gr = O.discriminator_bwd(cfg, self.d, cr, dlr)
            _, gf = O.discriminator_bwd(cfg, self.d, cf, dlf)
            grads = {k: gr[k] + gf[k] for k in gr}
        return (d_rl, d_fk, d_rl + d_fk), grads

    def g_tower(self, x, lab, ln, noise_fake=None, want_grads=True, tower=0):
        cfg = self.cfg
        params = self.params()
        training = self._training(want_grads)
        y, cg = generator_fwd(cfg, params, x, ln, training, self.frozen)
        self.last_bn = cg.get("bn")
        mse, dy_mse = O.g_mse(y, lab, cfg.output_dim)
        if training and self.l2_scale > 0.0:
            g_l2, l2g = O.l2_term(self.g, self.l2_scale)          # (self.g: the trainables -- beta and gamma among them)
        else:
            g_l2, l2g = 0.0, {}
        g_adv, dy = 0.0, self.mse_lambda * dy_mse
        if not self.supervised:
            lf_, cf = O.discriminator_fwd(cfg, self.d, y, ln, noise_fake)
            g_adv, dlf = O.lsgan_mean_sq(lf_, self.d_real)
            if want_grads:
                dy = dy + O.discriminator_bwd(cfg, self.d, cf, dlf, want_param_grads=False)[0]
        grads = None
        if want_grads:
            grads = generator_bwd(cfg, params, cg, dy)
            for k, v in l2g.items():
                grads[k] = grads[k] + v
        return (g_adv, mse, g_l2, g_adv + self.mse_lambda * mse + g_l2), grads, y

    def commit_run(self):
        """the G-run's update ops: the generator's, twice with the run's batch"""
        for _ in range(2):
            BN.commit(self.state, self.last_bn)
            self.commits += 1

    def g_step(self, inputs, labels, lengths, noise_fake=None, train=True):
        assert self.num_towers == 1
        x = np.asarray(inputs, self.dtype); lab = np.asarray(labels, self.dtype)
        ls, g, _ = self.g_tower(x, lab, np.asarray(lengths).astype(np.int32), noise_fake, want_grads=train)
        if train:
            self.commit_run()
            self.apply_g(g)
        return [ls[0]], [ls[1]], [ls[2]], [ls[3]]
