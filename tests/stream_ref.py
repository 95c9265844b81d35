"""fp64 restatement of the sequence generators' forward that TAKES and RETURNS the recurrent state (c, m) of every layer -- the
reference the stateful forward (rsrgan_forward_g_stream, rsrgan_amd/stream.py) is checked against on the host.  TEST ONLY.

It is pinned to the oracle, not the other way round (tests/test_stream_host.py): with zero state it must equal
oracle.rsrgan_oracle.generator_fwd on whole ragged batches to 1e-12 -- it is the same arithmetic in the same operation order
(lstmp_fwd's cell, dynamic_rnn's masking: a row past its length outputs zeros and copies its state through) -- so what it
adds is only where the state comes from and where it goes.

RefStreamModel is the stand-in for GAN_RNN in the host-logic tests of StreamEnhancer / decode_streams / run_gan_rnn.decode
(the way tests/helpers.OracleEngine stands in for the engine): forward() = the oracle on the whole utterance,
forward_stream() = this file with a per-row carried state.  It returns float64, so the host logic can be held to 1e-12."""
from types import SimpleNamespace

import numpy as np

from oracle import rsrgan_oracle as O


def zero_state(cfg, B, dtype=np.float64):
    R = cfg.g_proj if cfg.g_proj > 0 else cfg.g_cells
    return [(np.zeros((B, cfg.g_cells), dtype), np.zeros((B, R), dtype)) for _ in range(cfg.g_layers)]


def lstmp_fwd_state(x, lengths, p, c, m, forget_bias=1.0):
    """oracle lstmp_fwd from (c, m) instead of zeros; returns (out, c, m) -- the state of row b after its lengths[b] frames"""
    K, b, wf, wi, wo, Wp = p
    B, T, _ = x.shape
    H = wf.shape[0]
    out = np.zeros((B, T, m.shape[1]), x.dtype)
    for t in range(T):
        mask = (t < lengths)[:, None]
        xm = np.concatenate([x[:, t], m], axis=1)
        z = xm @ K + b
        i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        gi = O.sigmoid(i + wi * c)
        gf = O.sigmoid(f + forget_bias + wf * c)
        gj = np.tanh(j)
        cn = gf * c + gi * gj
        go = O.sigmoid(o + wo * cn)
        h = go * np.tanh(cn)
        mn = h @ Wp if Wp is not None else h
        out[:, t] = np.where(mask, mn, 0.0)
        c = np.where(mask, cn, c)
        m = np.where(mask, mn, m)
    return out, c, m


def generator_fwd_state(cfg, params, x, lengths, state):
    """oracle generator_fwd (no dropout) from `state` = [(c_l, m_l)]; returns (y, new state)"""
    hp = cfg.g_proj > 0
    lengths = np.asarray(lengths)
    new = []
    if cfg.g_type == "lstm":
        a = O.fc_fwd(x, params["g_model/fully_connected/weights"], params["g_model/fully_connected/biases"])
        cur = O.leakyrelu(a, cfg.lrelu_alpha)
        for l in range(cfg.g_layers):
            pre = "g_model/rnn/multi_rnn_cell/cell_%d/lstm_cell" % l
            cur, c, m = lstmp_fwd_state(cur, lengths, O._layer_params(params, pre, hp), state[l][0], state[l][1], cfg.forget_bias)
            new.append((c, m))
        y = O.fc_fwd(cur, params["g_model/fully_connected_1/weights"], params["g_model/fully_connected_1/biases"])
    else:
        res = cfg.g_type == "res_lstm_l"
        cur = x
        for l in range(cfg.g_layers):
            pre = "g_model/lstm_cell_%d/rnn/lstm_cell" % (l + 1)
            out, c, m = lstmp_fwd_state(cur, lengths, O._layer_params(params, pre, hp), state[l][0], state[l][1], cfg.forget_bias)
            new.append((c, m))
            cur = out + cur if res else out
        y = O.fc_fwd(cur, params["g_model/forward_out/fully_connected/weights"],
                     params["g_model/forward_out/fully_connected/biases"])
    return y, new


class RefStreamModel(object):
    """GAN_RNN's decode-side interface on the CPU: forward, forward_stream, load, save_dir.

    `tag_column`: when set, column `tag_column` of the inputs is taken as an utterance tag (constant over an utterance, different
    between utterances: the tests build their data that way) and forward_stream ASSERTS the rows' discipline: the frames a row is
    fed in one call belong to one utterance, and a row whose utterance changes is reset with that call."""

    def __init__(self, cfg, g_params, batch_size, max_frames, tag_column=None, save_dir=None):
        self.cfg = cfg
        self.g = {k: np.asarray(v, np.float64) for k, v in g_params.items()}
        self.batch_size, self.output_dim, self.save_dir = batch_size, cfg.output_dim, save_dir
        self.engine = SimpleNamespace(batch_size=batch_size, max_frames=max_frames, output_dim=cfg.output_dim)
        self.state = zero_state(cfg, batch_size)
        self.tag_column = tag_column
        self.row_tag = [None] * batch_size
        self.calls = []                       # (T, lengths, reset rows) of every forward_stream call

    def load(self, save_dir, moving_average=False):
        return True

    def _check(self, x, ln):
        x = np.asarray(x)
        ln = np.asarray(ln, np.int32)
        assert x.ndim == 3 and x.shape[0] == self.batch_size and x.shape[2] == self.cfg.input_dim, x.shape
        assert 0 < x.shape[1] <= self.engine.max_frames, (x.shape, self.engine.max_frames)
        assert ln.shape == (self.batch_size,) and (ln >= 0).all() and (ln <= x.shape[1]).all(), ln
        return x.astype(np.float64), ln

    def forward(self, inputs, lengths):
        x, ln = self._check(inputs, lengths)
        return O.generator_fwd(self.cfg, self.g, x, ln)[0]

    def forward_stream(self, inputs, lengths, reset=None):
        x, ln = self._check(inputs, lengths)
        rows = list(range(self.batch_size)) if reset is True else [int(r) for r in (reset or [])]
        for r in rows:
            for c, m in self.state:
                c[r] = 0.0
                m[r] = 0.0
            self.row_tag[r] = None
        if self.tag_column is not None:
            for r in range(self.batch_size):
                if ln[r] == 0:
                    continue
                tags = np.unique(x[r, :ln[r], self.tag_column])
                assert tags.size == 1, "row %d was fed frames of %d utterances in one call" % (r, tags.size)
                assert self.row_tag[r] is None or self.row_tag[r] == tags[0], "row %d changed utterance without a reset" % r
                self.row_tag[r] = tags[0]
        self.calls.append((x.shape[1], ln.copy(), tuple(rows)))
        y, self.state = generator_fwd_state(self.cfg, self.g, x, ln, self.state)
        return y
