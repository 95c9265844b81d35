"""fp64 oracle of the reference's bnlstm generator on the supervised trainer (models/bnlstm.py:38-127, models/BNLSTMCell.py,
models/rnn_trainer.py:66-205), written line by line from BNLSTMCell.call in torch float64.

TF 1.4's dynamic_rnn runs the cell on ALL rows at every step t < T (the fed time axis); a row past its length gets output 0
and keeps its (c, m): a `where` here.  Such rows therefore enter every step's batch statistics and receive gradient through
them.  Gradients come from torch.autograd, independent of the hand-derived HIP backward.  The moving statistics of a training
run follow the sequential EMA over t = 0..T-1 (the definition DESIGN.md adopts).  The optimizer step reuses the project
oracle's l2_term / clip_by_norm and its Adam + EMA update (oracle.rsrgan_oracle.GanRnnOracle.apply_g)."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from oracle import rsrgan_oracle as O

EPS, DECAY = 1e-3, 0.999
BN_LEAVES = ("scale", "offset", "moving_mean", "moving_var")


def cell_prefix(l: int) -> str:
    return "g_model/rnn/multi_rnn_cell/cell_%d/bnlstm_cell/" % l


def param_specs(din: int, dout: int, layers: int, cells: int, proj: int) -> List[Tuple[str, Tuple[int, ...]]]:
    """the variables in the reference's creation order (TF 1.4 layer scoping: _to_snake_case('BNLSTMCell') = bnlstm_cell)"""
    H4 = 4 * cells
    s = [("g_model/fully_connected/weights", (din, proj)), ("g_model/fully_connected/biases", (proj,))]
    for l in range(layers):
        p = cell_prefix(l)
        s += [(p + "input_kernel", (proj, H4)), (p + "state_kernel", (proj, H4))]
        s += [(p + "input/" + k, (H4,)) for k in BN_LEAVES]
        s += [(p + "state/" + k, (H4,)) for k in BN_LEAVES]
        s += [(p + "bias", (H4,)), (p + "W_F_diag", (cells,)), (p + "W_I_diag", (cells,)), (p + "W_O_diag", (cells,))]
        s += [(p + "cell/" + k, (cells,)) for k in BN_LEAVES]
        s += [(p + "projection/kernel", (cells, proj))]
    s += [("g_model/fully_connected_1/weights", (proj, dout)), ("g_model/fully_connected_1/biases", (dout,))]
    return s


def is_moving(name: str) -> bool:
    return name.rsplit("/", 1)[-1] in ("moving_mean", "moving_var")


def rand_params(specs, seed: int) -> Dict[str, np.ndarray]:
    """random fp32 values that exercise every path: xavier-scaled matrices, scale ~ U(0.3, 1.3), small offsets / biases /
    diagonals, moving statistics away from their initial values (variances positive)"""
    rng = np.random.default_rng(seed)
    p = {}
    for name, shape in specs:
        leaf = name.rsplit("/", 1)[-1]
        if len(shape) == 2:
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            v = rng.uniform(-lim, lim, shape)
        elif leaf == "scale":
            v = rng.uniform(0.3, 1.3, shape)
        elif leaf == "moving_var":
            v = rng.uniform(0.5, 2.0, shape)
        else:
            v = rng.normal(0.0, 0.2, shape)
        p[name] = v.astype(np.float32)
    return p


def _sites(p, l):
    return {s: [p[cell_prefix(l) + s + "/" + k] for k in BN_LEAVES] for s in ("input", "state", "cell")}


def forward(p: Dict[str, torch.Tensor], x, lengths, layers: int, train: bool, forget_bias: float = 1.0):
    """y [B,T,Dout] and, for a training run, the batch moments {moving-statistic name: [T, n]} of every site"""
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=torch.float64)
    B, T, _ = x.shape
    ln = torch.as_tensor(np.asarray(lengths, np.int64))
    mask = torch.arange(T)[None, :] < ln[:, None]                       # [B, T]
    inp = torch.relu(x @ p["g_model/fully_connected/weights"] + p["g_model/fully_connected/biases"])
    moments: Dict[str, List[torch.Tensor]] = {}

    def batch_norm(v, l, site):                                         # BNLSTMCell.py:20-47
        scale, offset, mm, mv = _sites(p, l)[site]
        if train:
            mean = v.mean(0)
            var = ((v - mean) ** 2).mean(0)                             # tf.nn.moments: biased
            moments.setdefault(cell_prefix(l) + site + "/moving_mean", []).append(mean)
            moments.setdefault(cell_prefix(l) + site + "/moving_var", []).append(var)
        else:
            mean, var = mm, mv
        return (v - mean) / torch.sqrt(var + EPS) * scale + offset

    for l in range(layers):
        pre = cell_prefix(l)
        W_xh, W_hh, W_p = p[pre + "input_kernel"], p[pre + "state_kernel"], p[pre + "projection/kernel"]
        H, P = W_p.shape
        c = torch.zeros(B, H, dtype=torch.float64)
        m = torch.zeros(B, P, dtype=torch.float64)
        outs = []
        for t in range(T):
            xh = inp[:, t] @ W_xh
            hh = m @ W_hh
            bn_xh = batch_norm(xh, l, "input")
            bn_hh = batch_norm(hh, l, "state")
            lstm_matrix = bn_xh + bn_hh + p[pre + "bias"]
            i, j, f, o = torch.split(lstm_matrix, H, dim=1)
            c_new = (c * torch.sigmoid(f + forget_bias + p[pre + "W_F_diag"] * c) +
                     torch.sigmoid(i + p[pre + "W_I_diag"] * c) * torch.tanh(j))
            bn_c = batch_norm(c_new, l, "cell")
            h = torch.sigmoid(o + p[pre + "W_O_diag"] * c_new) * torch.tanh(bn_c)
            m_new = h @ W_p
            mk = mask[:, t:t + 1]
            outs.append(torch.where(mk, m_new, torch.zeros_like(m_new)))
            c = torch.where(mk, c_new, c)
            m = torch.where(mk, m_new, m)
        inp = torch.stack(outs, 1)
    y = inp @ p["g_model/fully_connected_1/weights"] + p["g_model/fully_connected_1/biases"]
    return y, {k: torch.stack(v, 0) for k, v in moments.items()}


def bn_formula(v, scale, offset, eps=EPS):
    """BN of one step in plain numpy fp64: per column over the batch axis, biased variance"""
    v = np.asarray(v, np.float64)
    mean = v.mean(0)
    var = ((v - mean) ** 2).mean(0)
    return scale * (v - mean) / np.sqrt(var + eps) + offset


def sequential_ema(start, per_step, decay=DECAY):
    out = np.array(start, np.float64)
    for row in np.asarray(per_step, np.float64):
        out = out * decay + row * (1.0 - decay)
    return out


class BnlstmOracle:
    """RNNTrainer(g_type='bnlstm') in fp64: tower losses / gradients, the Adam step with per-tensor clip and EMA of the
    trainables, the moving statistics of training runs."""

    def __init__(self, params: Dict[str, np.ndarray], layers: int, *, output_dim: int, l2_scale=0.0, g_learning_rate=1e-3,
                 clip_norm=15.0, mse_lambda=1.0):
        self.layers, self.output_dim = layers, output_dim
        self.g = {k: np.array(v, np.float64) for k, v in params.items() if not is_moving(k)}   # trainables (Adam, EMA)
        self.moving = {k: np.array(v, np.float64) for k, v in params.items() if is_moving(k)}
        self.order = list(params)
        self.l2_scale, self.g_learning_rate, self.clip_norm, self.mse_lambda = l2_scale, g_learning_rate, clip_norm, mse_lambda
        self.beta1, self.beta2, self.eps = 0.9, 0.999, 1e-8
        self.adam_m = {k: np.zeros_like(v) for k, v in self.g.items()}
        self.adam_v = {k: np.zeros_like(v) for k, v in self.g.items()}
        self.adam_t = 0
        self.ema_decay = 0.9999
        self.g_ema = {k: v.copy() for k, v in self.g.items()}

    def params(self, ema=False):
        src = self.g_ema if ema else self.g
        out = dict(src)
        out.update(self.moving)
        return {k: out[k] for k in self.order}

    def _torch(self, p, grad):
        return {k: torch.tensor(v, dtype=torch.float64, requires_grad=grad and not is_moving(k)) for k, v in p.items()}

    def tower(self, x, lab, ln, train=True):
        """(g_adv=0, g_mse, g_l2, g_loss), gradients of the trainables (train only), the batch moments (train only)"""
        p = self._torch(self.params(), train)
        y, moments = forward(p, x, ln, self.layers, train)
        lab_t = torch.as_tensor(np.asarray(lab), dtype=torch.float64)
        mse = 0.5 * self.output_dim * torch.mean((y - lab_t) ** 2)        # rnn_trainer.py:146-148
        l2, l2g = O.l2_term(self.g, self.l2_scale) if (train and self.l2_scale > 0) else (0.0, {})
        grads = None
        if train:
            (self.mse_lambda * mse).backward()
            grads = {k: p[k].grad.numpy().copy() for k in self.g}
            for k, v in l2g.items():
                grads[k] = grads[k] + v
        m = float(mse.detach())
        return (0.0, m, l2, self.mse_lambda * m + l2), grads, {k: v.detach().numpy() for k, v in moments.items()}

    def update_moving(self, moments):
        for k, v in moments.items():
            self.moving[k] = sequential_ema(self.moving[k], v)

    def step(self, x, lab, ln, train=True):
        losses, grads, moments = self.tower(x, lab, ln, train)
        if train:
            self.update_moving(moments)
            O.GanRnnOracle.apply_g(self, grads)             # clip_by_norm per tensor, Adam, EMA of the trainables
        return losses

    def forward(self, x, ln, ema=False):
        p = {k: torch.tensor(v, dtype=torch.float64) for k, v in self.params(ema).items()}
        return forward(p, x, ln, self.layers, False)[0].numpy()
