"""The decode-time algebra of the bnlstm inference handle, without a GPU.

Outside training every batch-norm site of BNLSTMCell normalises with the moving statistics, constants of the handle, so the cell is a
plain peephole LSTMP whose input / state kernels are scaled column by column, whose bias absorbs the two sites' shifts, and whose cell
site is one affine map in front of the output tanh.  fold64() is that fold in numpy fp64 and lstmp_forward64() the plain cell with the
extra affine: together they must reproduce tests/bnlstm_ref.forward(train=False).  Both are the references of tests/test_gpu_bnl_infer.py.
Also here: the operator's symbol and binding, RNNTrainer(bnlstm, inference_only=True) on a stub engine, run_rnn's choice of the model."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import bnlstm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3                                   # BNLSTMCell.py:20 batch_norm(epsilon=1e-3)
SITES = ("input", "state", "cell")


def draw_params(specs, seed, zero_cell_scale=()):
    """bnlstm_ref.rand_params with the batch-norm leaves redrawn so that every term of the fold matters: means ~ N(0, 0.3), variances in
    [0.5, 2], scales in +-[0.05, 0.3], offsets ~ N(0, 0.1) (with the initial 0 / 1 / 0.1 / 0 a dropped mean or offset would not show).
    zero_cell_scale: units of every layer's cell site whose scale is 0 (h then depends on the offset alone)"""
    p = R.rand_params(specs, seed)
    rng = np.random.default_rng(seed + 1000)
    for name, shape in specs:
        leaf = name.rsplit("/", 1)[-1]
        if "/bnlstm_cell/" not in name or leaf not in R.BN_LEAVES:
            continue
        if leaf == "moving_mean":
            v = rng.normal(0.0, 0.3, shape)
        elif leaf == "moving_var":
            v = rng.uniform(0.5, 2.0, shape)
        elif leaf == "scale":
            v = rng.uniform(0.05, 0.3, shape) * rng.choice([-1.0, 1.0], shape)
            if "/cell/" in name:
                v[list(zero_cell_scale)] = 0.0
        else:
            v = rng.normal(0.0, 0.1, shape)
        p[name] = v.astype(np.float32)
    return p


def site64(p, l, site):
    return [np.asarray(p[R.cell_prefix(l) + site + "/" + k], np.float64) for k in R.BN_LEAVES]      # scale offset moving_mean moving_var


def fold64(p, l):
    """KxT [4H][P], KhT [4H][P], bias [4H], ca [H], cb [H] of layer l in fp64, and the five terms of the bias / two of cb (for the bounds)"""
    pre = R.cell_prefix(l)
    g, shift = {}, {}
    for s in SITES:
        scale, offset, mean, var = site64(p, l, s)
        g[s] = scale / np.sqrt(var + EPS)
        shift[s] = (offset, -g[s] * mean)
    Wx, Wh = np.asarray(p[pre + "input_kernel"], np.float64), np.asarray(p[pre + "state_kernel"], np.float64)
    bias_terms = [np.asarray(p[pre + "bias"], np.float64), shift["input"][0], shift["input"][1], shift["state"][0], shift["state"][1]]
    return dict(KxT=(Wx * g["input"][None, :]).T, KhT=(Wh * g["state"][None, :]).T, bias=sum(bias_terms), ca=g["cell"],
                cb=shift["cell"][0] + shift["cell"][1], bias_terms=bias_terms, cb_terms=list(shift["cell"]))


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def lstmp_forward64(p, x, lengths, layers, forget_bias=1.0, state=None):
    """input FC + ReLU, `layers` plain peephole LSTMP cells on the folded variables with h = sigmoid(o + w_o c) tanh(ca c + cb), output FC.
    fp64 numpy; dynamic_rnn's masking.  state: [(c, m)] per layer to start from (None: zeros); returns y [B, T, Dout] and the final state"""
    P64 = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    B, T, _ = x.shape
    ln = np.asarray(lengths)
    inp = np.maximum(x @ P64["g_model/fully_connected/weights"] + P64["g_model/fully_connected/biases"], 0.0)
    final = []
    for l in range(layers):
        pre = R.cell_prefix(l)
        f = fold64(p, l)
        Wp = P64[pre + "projection/kernel"]
        H, Pw = Wp.shape
        wi, wf, wo = P64[pre + "W_I_diag"], P64[pre + "W_F_diag"], P64[pre + "W_O_diag"]
        c, m = (np.zeros((B, H)), np.zeros((B, Pw))) if state is None else (np.array(state[l][0], np.float64), np.array(state[l][1], np.float64))
        outs = np.zeros((B, T, Pw))
        for t in range(T):
            z = inp[:, t] @ f["KxT"].T + m @ f["KhT"].T + f["bias"]
            i, j, fg, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
            cn = c * _sig(fg + forget_bias + wf * c) + _sig(i + wi * c) * np.tanh(j)
            h = _sig(o + wo * cn) * np.tanh(f["ca"] * cn + f["cb"])
            mn = h @ Wp
            live = (t < ln)[:, None]
            outs[:, t] = np.where(live, mn, 0.0)
            c, m = np.where(live, cn, c), np.where(live, mn, m)
        final.append((c, m))
        inp = outs
    return inp @ P64["g_model/fully_connected_1/weights"] + P64["g_model/fully_connected_1/biases"], final


def oracle_forward(p, x, lengths, layers):
    p64 = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in p.items()}
    return R.forward(p64, np.asarray(x, np.float64), lengths, layers, False)[0].numpy()


# ---- the algebra ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("zero", [(), (0, 5)])
def test_folded_lstmp_equals_the_batch_norm_cell(zero):
    L, H, P, din, dout, B, T = 2, 12, 7, 6, 5, 3, 9
    specs = R.param_specs(din, dout, L, H, P)
    p = draw_params(specs, 31, zero)
    rng = np.random.default_rng(32)
    x = rng.standard_normal((B, T, din))
    ln = np.array([T, 5, 1], np.int32)
    want = oracle_forward(p, x, ln, L)
    got, _ = lstmp_forward64(p, x, ln, L)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("folded LSTMP against bnlstm_ref.forward(train=False): rel", err)
    assert err < 1e-10
    # every term of the fold matters at these statistics: dropping one moves the output far beyond the GPU tests' 2e-4
    for leaf in ("moving_mean", "offset"):
        for site in SITES:
            q = dict(p)
            for l in range(L):
                k = R.cell_prefix(l) + site + "/" + leaf
                q[k] = np.zeros_like(p[k])
            moved = np.linalg.norm(lstmp_forward64(q, x, ln, L)[0] - want) / np.linalg.norm(want)
            assert moved > 1e-3, (site, leaf, moved)


def test_carried_state_is_the_raw_cell_state():
    """two chunks that hand (c, m) on = the whole utterance: the carried c is the cell state BEFORE the cell site's affine map"""
    L, H, P, din, dout, B, T = 2, 12, 7, 6, 5, 3, 9
    p = draw_params(R.param_specs(din, dout, L, H, P), 33)
    x = np.random.default_rng(34).standard_normal((B, T, din))
    ln = np.array([T, 5, 1], np.int32)
    whole, _ = lstmp_forward64(p, x, ln, L)
    y1, st = lstmp_forward64(p, x[:, :4], np.clip(ln, 0, 4), L)
    y2, _ = lstmp_forward64(p, x[:, 4:], np.clip(ln - 4, 0, 5), L, state=st)
    assert np.allclose(np.concatenate([y1, y2], 1), whole, rtol=0, atol=1e-13)


# ---- flag, symbol, binding ---------------------------------------------------------------------------------------------------------

def test_fold_operator_declared_bound_and_exported():
    from rsrgan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rsrgan.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+rsrgan_op_bnl_fold\s*\(", code)
    assert re.search(r"RSRGAN_FLAG_INFER\s*=\s*64", code) and _lib.FLAG_INFER == 64
    assert "rsrgan_op_bnl_fold" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "rsrgan_op_bnl_fold") and len(lib.rsrgan_op_bnl_fold.argtypes) == 14
    # a null pointer is refused before any HIP call (no GPU needed)
    assert lib.rsrgan_op_bnl_fold(None, None, None, None, 7, 12, None, 8, None, 8, None, None, None, None) == -1
    assert b"op_bnl_fold" in lib.rsrgan_last_error()


# ---- RNNTrainer(bnlstm, inference_only=True) on a stub engine ----------------------------------------------------------------------------

class StubEngine(object):
    """what an inference-only model touches of an engine: the generator's table and variables"""
    inference = True
    ema_enabled = False

    def __init__(self, specs):
        self.table, off = [], 0
        for name, shape in specs:
            self.table.append((name, tuple(shape), off))
            off += int(np.prod(shape))
        self.n, self.calls, self.flat = off, [], None

    def tensor_table(self, net):
        assert net == 0, "an inference-only model has no discriminator"
        return self.table

    def param_count(self, net):
        assert net == 0
        return self.n

    def set_params(self, net, flat, what="variables"):
        self.calls.append((net, what))
        self.flat = np.array(flat, np.float32)

    def set_scalar(self, k, v):
        pass


def _bnl_args(B=2, din=6, dout=5):
    return SimpleNamespace(batch_size=B, input_dim=din, output_dim=dout, left_context=0, right_context=0, g_type="bnlstm", keep_prob=1.0,
                           batch_norm=False, num_gpu=1, save_dir=None, l2_scale=0.0, g_learning_rate=1e-3)


@pytest.mark.parametrize("moving_average", [False, True])
def test_inference_only_trainer_loads_the_generator_alone(tmp_path, moving_average):
    from rsrgan_amd.trainer import RNNTrainer
    L, H, P, din, dout = 2, 12, 7, 6, 5
    specs = R.param_specs(din, dout, L, H, P)
    p = draw_params(specs, 41)
    payload = {}
    for name, v in p.items():
        payload[name] = v
        if not R.is_moving(name):
            payload[name + "/ExponentialMovingAverage"] = v + np.float32(1.0)      # the shadows differ from the variables
            payload[name + "/Adam"] = np.zeros_like(v)
    payload["d_model/fully_connected/weights"] = np.zeros((5, 1), np.float32)
    os.makedirs(str(tmp_path), exist_ok=True)
    np.savez(str(tmp_path / "RNNTrainer-3.npz"), **payload)
    with open(str(tmp_path / "checkpoint"), "w") as f:
        f.write('model_checkpoint_path: "RNNTrainer-3"\n')
    eng = StubEngine(specs)
    m = RNNTrainer(None, _bnl_args(din=din, dout=dout), ["gpu:0"], engine=eng, inference_only=True)
    assert m.inference_only and m.cross_validation
    assert m.load(str(tmp_path), moving_average=moving_average)
    assert eng.calls == [(0, "variables")]
    for name, shape, off in eng.table:
        got = eng.flat[off:off + int(np.prod(shape))].reshape(shape)
        shadow = moving_average and not R.is_moving(name)       # the trainables under their shadow names, the moving statistics raw
        assert np.array_equal(got, p[name] + np.float32(1.0) if shadow else p[name]), name
    for call in (lambda: m.g_step(None, None, None), lambda: m.save(str(tmp_path), 4), lambda: m.d_step(None, None, None)):
        with pytest.raises(RuntimeError):
            call()


# ---- run_rnn: which model decode builds ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("argv,lean,logged", [
    (["--g_type", "bnlstm"], False, False),
    (["--g_type", "bnlstm", "--decode_lean"], True, False),
    (["--g_type", "bnlstm", "--decode_chunk", "16"], True, True),
    (["--g_type", "bnlstm", "--decode_chunk", "16", "--decode_streams", "3", "--decode_lean"], True, False),
    (["--g_type", "lstm", "--decode_chunk", "16"], False, False),
])
def test_run_rnn_builds_the_inference_model_for_chunked_bnlstm_decode(monkeypatch, argv, lean, logged):
    from rsrgan_amd import run_rnn as RR
    FLAGS, _ = RR.build_parser().parse_known_args(["--decode"] + argv)
    logs = []
    assert RR.decode_lean(FLAGS, logs.append) is lean
    assert len(logs) == (1 if logged else 0)
    if logged:
        assert "bnlstm" in logs[0] and "inference-only" in logs[0]
    # ... and decode() hands exactly that to the model it builds
    made = {}

    def fake_model(flags, cv, share, net_overrides, **kw):
        made.update(kw, batch_size=flags.batch_size)
        return "model"
    monkeypatch.setattr(RR, "_model", fake_model)
    monkeypatch.setattr(RR.gan_loop, "decode", lambda F, model_factory, log: model_factory())
    assert RR.decode(FLAGS, log=lambda s: None) == "model"
    assert made.get("inference_only", False) is lean
    chunk = FLAGS.decode_chunk
    assert made["max_frames"] == (chunk if chunk > 0 else FLAGS.max_frames) and made["batch_size"] == (FLAGS.decode_streams if chunk > 0 else 1)
