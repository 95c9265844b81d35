"""fp64 reference of the res_lstm_i generator (models/res_lstm_i.py:41-199) and of its supervised step (models/rnn_trainer.py:131-156),
composed from the public pieces of oracle.rsrgan_oracle: lstmp_fwd / lstmp_bwd, fc_fwd / fc_bwd, g_mse, l2_term, clip_by_norm (inside
GanRnnOracle.apply_g).  TEST ONLY.

res_lstm_i is res_lstm_l's stack of LSTMCell(g_cells, num_proj=g_proj, peepholes) -- the same variable table, name by name -- with the
residual ALWAYS taken from the stack's input, never from a running sum:

    in_0 = x,   in_l = drop(out_{l-1}) + x,   y = (drop(out_{L-1}) + x) . W + b

dynamic_rnn zeroes out_l past a row's length, so a padded frame has in_l = x and y = x . W + b; those frames enter the MSE mean.  x is
data: nothing flows into the residual branch, d(out_{l-1}) = d(in_l) (through K_x only) and d(out_{L-1}) = dy . W^T -- the plain
stack's BPTT, with the weight-gradient products reading the summed inputs in_l.

tests/test_res_lstm_i_ref.py pins this file: central differences on every tensor, L = 1 against oracle.generator_fwd of res_lstm_l,
L = 2 against res_lstm_l by exactly out_1 . W_fc, the padded frames."""
import dataclasses

import numpy as np

from oracle import rsrgan_oracle as O

FC_W = "g_model/forward_out/fully_connected/weights"
FC_B = "g_model/forward_out/fully_connected/biases"


def cell(l):
    return "g_model/lstm_cell_%d/rnn/lstm_cell" % (l + 1)


def make_cfg(**kw):
    """NetCfg of a res_lstm_i generator (the reference builds 2 x LSTMCell(760, num_proj=257): res_lstm_i.py:43-44,101-118)"""
    c = O.NetCfg(g_type="res_lstm_i", g_layers=2, g_cells=760, g_proj=257)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def table_cfg(cfg):
    """the cfg whose oracle.g_param_specs IS res_lstm_i's variable table: res_lstm_l's, names and order"""
    return dataclasses.replace(cfg, g_type="res_lstm_l")


def g_param_specs(cfg):
    assert cfg.g_proj == cfg.input_dim, "residual adds need proj == input_dim (res_lstm_i.py:111)"
    return O.g_param_specs(table_cfg(cfg))


def generator_fwd(cfg, params, x, lengths, drop=None):
    """x [B,T,Din] -> (y [B,T,Dout], cache); drop as oracle.generator_fwd's: (keep_prob, mask_of_layer)"""
    cache = {"outs": []}
    ins = [x]
    for l in range(cfg.g_layers):
        out, c = O.lstmp_fwd(ins[-1], lengths, O._layer_params(params, cell(l), True), cfg.forget_bias)
        cache[cell(l)] = c
        if drop is not None:                      # DropoutWrapper(output_keep_prob) wraps the cell: out_l is dropped before the add
            keep, mask_of = drop
            m = np.asarray(mask_of(l), out.dtype)
            cache["drop%d" % l] = (m, keep)
            out = out / keep * m
        cache["outs"].append(out)
        ins.append(out + x)                       # res_lstm_i.py:111,190: always the stack's input
    cache["ins"] = ins
    return O.fc_fwd(ins[-1], params[FC_W], params[FC_B]), cache


def generator_bwd(cfg, params, cache, dy):
    grads = {}
    d, grads[FC_W], grads[FC_B] = O.fc_bwd(cache["ins"][-1], params[FC_W], dy)
    for l in range(cfg.g_layers - 1, -1, -1):
        dr = cache.get("drop%d" % l)
        if dr is not None:
            d = d * dr[0] / dr[1]
        d, g = O.lstmp_bwd(d, cache[cell(l)], O._layer_params(params, cell(l), True))      # d(in_l) = d(out_{l-1}): x is data
        O._put_layer_grads(grads, cell(l), g)
    return grads


class ResLstmIOracle(O.GanRnnOracle):
    """RNNTrainer(g_type='res_lstm_i'): GanRnnOracle's state, masks, clip + Adam + EMA (apply_g) and g_step around this file's tower"""
    supervised = True

    def __init__(self, cfg, g_params, **kw):
        kw.setdefault("mse_lambda", 1.0)
        super(ResLstmIOracle, self).__init__(cfg, g_params, {}, **kw)

    def forward(self, inputs, lengths):
        x = np.asarray(inputs, self.dtype)
        return generator_fwd(self.cfg, self.g, x, np.asarray(lengths).astype(np.int32))[0]

    def g_tower(self, x, lab, ln, noise_fake=None, want_grads=True, tower=0):
        cfg = self.cfg
        y, cg = generator_fwd(cfg, self.g, x, ln, self._drop(x.shape, want_grads, tower))
        mse, dy = O.g_mse(y, lab, cfg.output_dim)
        g_l2, l2g = O.l2_term(self.g, self.l2_scale) if (not self.cross_validation and self.l2_scale > 0.0) else (0.0, {})
        grads = None
        if want_grads:
            grads = generator_bwd(cfg, self.g, cg, self.mse_lambda * dy)
            for k, v in l2g.items():
                grads[k] = grads[k] + v
        return (0.0, mse, g_l2, self.mse_lambda * mse + g_l2), grads, y


def rand_g(cfg, seed=0, bias_std=0.1):
    """tests.helpers.rand_params for this generator: xavier weights, small random biases, rounded to fp32"""
    rng = np.random.default_rng(seed)
    g = O.xavier_init(g_param_specs(cfg), rng)
    for k in g:
        if "bias" in k:
            g[k] = rng.normal(0, bias_std, g[k].shape)
        g[k] = g[k].astype(np.float32)
    return g
