"""rsrgan_amd/run_rnn.py -- the outer loop of scripts/train_rnn.py:270-430 -- on the CPU, on a stand-in model whose cross-validation
losses are scripted: the learning-rate sequence, accept / reject and which iterations save, the stop rule, the last-model rule, resume,
decode; and the C ABI's new enumerator on the loaded library (no GPU needed for rsrgan_default_cfg)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import rsrgan_oracle as O
from rsrgan_amd import run_gan_rnn as G
from rsrgan_amd import run_rnn as R
from rsrgan_amd.io import ArkReader, ArkWriter


def _data(tmp, n, tag, rng, din, dout):
    wi, wl = ArkWriter(str(tmp / (tag + "_in.scp"))), ArkWriter(str(tmp / (tag + "_lab.scp")))
    for i in range(n):
        T = int(rng.integers(6, 10))
        wi.write_next_utt(str(tmp / (tag + "_in.ark")), "%s%02d" % (tag, i), rng.standard_normal((T, din)) * 2 + 1)
        wl.write_next_utt(str(tmp / (tag + "_lab.ark")), "%s%02d" % (tag, i), rng.standard_normal((T, dout)) - 1)
    wi.close(); wl.close()
    return str(tmp / (tag + "_in.scp")), str(tmp / (tag + "_lab.scp"))


class Shared(object):
    def __init__(self, cv_losses, have_checkpoint=False):
        self.cv_losses, self.have_checkpoint = list(cv_losses), have_checkpoint
        self.lr_set, self.saves, self.loads, self.train_calls, self.eval_calls, self.lr_at_step = [], [], [], 0, 0, []
        self.iteration = 0


class StandIn(object):
    """what run_rnn.train touches of an RNNTrainer: batch_size, num_gpu, save_dir, g_learning_rate, engine.device, g_step, load, save"""

    def __init__(self, sh, FLAGS, cv):
        self.sh, self.cv = sh, cv
        self.batch_size, self.num_gpu, self.save_dir = FLAGS.batch_size, FLAGS.num_gpu, FLAGS.save_dir
        self.engine = SimpleNamespace(device=torch.device("cpu"))

    g_learning_rate = property(lambda s: s.sh.lr_set[-1], lambda s, v: s.sh.lr_set.append(float(v)))

    def g_step(self, x, lab, ln, train=True, sync=True, gather=True):
        sh = self.sh
        assert not sync and not gather and train == (not self.cv)
        assert x.shape[0] == self.batch_size and lab.shape[:2] == x.shape[:2] and len(ln) == self.batch_size
        if train:
            if sh.train_calls % 2 == 0:
                sh.iteration += 1
            sh.train_calls += 1
            sh.lr_at_step.append(sh.lr_set[-1])
            return torch.tensor([[0.0, 2.0, 0.5, 2.5]])
        sh.eval_calls += 1
        v = sh.cv_losses[sh.iteration - 1]
        return torch.tensor([[0.0, v - 0.25, 0.25, v]], dtype=torch.float64)

    def load(self, save_dir, model_file=None, moving_average=False):
        self.sh.loads.append(save_dir)
        return self.sh.have_checkpoint

    def save(self, save_dir, step):
        assert not self.cv and save_dir == self.save_dir
        self.sh.saves.append(step)


def _flags(tmp_path, extra=()):
    rng = np.random.default_rng(0)
    din, dout = 5, 3
    tr = _data(tmp_path, 4, "tr", rng, din, dout)
    cv = _data(tmp_path, 2, "cv", rng, din, dout)
    FLAGS, _ = R.build_parser().parse_known_args([
        "--data_dir", str(tmp_path), "--tr_inputs_scp", tr[0], "--tr_labels_scp", tr[1], "--cv_inputs_scp", cv[0], "--cv_labels_scp", cv[1],
        "--input_dim", str(din), "--output_dim", str(dout), "--left_context", "1", "--right_context", "1", "--batch_size", "2",
        "--apply_cmvn", "false", "--save_dir", str(tmp_path / "exp"), "--g_learning_rate", "0.003", "--g_type", "res_lstm_i",
        "--tr_list_file", "ignored"] + list(extra))                       # unknown flag ignored like the reference
    return FLAGS


def _run(tmp_path, cv_losses, extra=(), have_checkpoint=False):
    FLAGS = _flags(tmp_path, extra)
    sh = Shared(cv_losses, have_checkpoint)
    made = []

    def factory(cv, share):
        assert (share is None) == (not cv) and (share is None or share is made[0])
        made.append(StandIn(sh, FLAGS, cv))
        return made[-1]
    logs = []
    hist = R.train(FLAGS, model_factory=factory, log=logs.append)
    return FLAGS, sh, hist, "\n".join(logs)


def test_parser_has_the_recipes_flags():
    FLAGS = R.build_parser().parse_args([])
    assert (FLAGS.batch_size, FLAGS.g_learning_rate, FLAGS.min_epochs, FLAGS.max_epochs, FLAGS.end_improve) == (256, 0.0001, 15, 20, 0.001)
    assert (FLAGS.save_dir, FLAGS.keep_prob, FLAGS.l2_scale, FLAGS.num_gpu, FLAGS.decode) == ("exp/rnn", 1.0, 0.00001, 1, False)
    for t in ("lstm", "res_lstm_l", "res_lstm_base", "bnlstm", "res_lstm_i"):
        assert t in R.RNNTrainer.G_TYPES


def test_learning_rate_accept_reject_and_stop(tmp_path):
    #            accept accept reject accept  accept(tiny: stops, 4 > min_iters = 3 is the first iteration allowed to)
    cv = [5.0, 4.0, 4.5, 3.99, 3.9899, 1.0, 1.0]
    FLAGS, sh, hist, text = _run(tmp_path, cv, ["--min_epochs", "3", "--max_epochs", "7", "--num_gpu", "1"])
    assert hist == cv[:5]
    assert sh.saves == [1, 2, 4, 5]                                        # iteration 3 rejected: nothing saved, nothing reloaded
    assert sh.loads == [FLAGS.save_dir] and "[!] Begin a new model." in text
    # the learning rate: num_gpu * lr first, then exponential_decay(iteration, num_gpu, min_iters, lr) after each iteration
    want = [1 * 0.003] + [O.exponential_decay(k, 1, 3, 0.003) for k in range(1, 6)]
    assert np.allclose(sh.lr_set, want, rtol=1e-12) and len(sh.lr_set) == 6
    assert np.allclose(sh.lr_at_step, np.repeat(want[:5], 2), rtol=1e-12)  # two batches per iteration, each at that iteration's rate
    assert sh.train_calls == 10 and sh.eval_calls == 5
    assert "Iteration 3: Nnet Rejected. g_loss_prev = 4.00000, g_loss_new = 4.50000" in text
    assert "Iteration 4: Nnet Accepted. Save model SUCCESS. g_loss_prev = 4.00000, g_loss_new = 3.99000" in text
    assert "Iteration 5: Finished, too small relative G improvement" in text and "Iteration 4: Finished" not in text
    assert "1/7 (TRAIN AVG.LOSS): g_mse_loss = 2.00000, g_l2_loss = 0.50000, g_loss = 2.50000, learning_rate= 3.000e-03" in text
    assert "1/7 (CROSS AVG.LOSS): g_mse_loss = 4.75000, g_l2_loss = 0.25000, g_loss = 5.00000, time = " in text
    assert text.rstrip().endswith("Training Done.")


def test_small_improvement_before_min_iters_does_not_stop(tmp_path):
    cv = [5.0, 4.9999, 4.9998, 4.9997]
    _, sh, hist, text = _run(tmp_path, cv, ["--min_epochs", "3", "--max_epochs", "4"])
    assert len(hist) == 4 and "Iteration 4: Finished" in text and "Iteration 3: Finished" not in text
    assert sh.saves == [1, 2, 3, 4]


def test_runs_to_max_iters_and_last_model_rule_saves_nothing_twice(tmp_path):
    """check_interval = 1 (train_rnn.py:342): the window is empty when the loop ends, so the last-model rule adds no save"""
    cv = [5.0, 6.0, 4.0]
    _, sh, hist, text = _run(tmp_path, cv, ["--min_epochs", "3", "--max_epochs", "3"])
    assert hist == cv and sh.saves == [1, 3] and "Finished" not in text
    assert text.count("Nnet Accepted") == 2 and text.count("Nnet Rejected") == 1


def test_multi_gpu_learning_rate(tmp_path):
    # (the stand-in is one rank; batches of batch_size * num_gpu rows would be sharded by the real model: here num_gpu only scales)
    FLAGS = _flags(tmp_path, ["--min_epochs", "2", "--max_epochs", "2", "--batch_size", "1", "--num_gpu", "2"])
    sh = Shared([5.0, 4.0])
    m = []

    class Two(StandIn):
        def g_step(self, x, lab, ln, **kw):
            return StandIn.g_step(self, x[:1], lab[:1], ln[:1], **kw)
    hist = R.train(FLAGS, model_factory=lambda cv, share: (m.append(Two(sh, FLAGS, cv)), m[-1])[1], log=lambda s: None)
    assert len(hist) == 2
    assert np.allclose(sh.lr_set, [2 * 0.003, O.exponential_decay(1, 2, 2, 0.003), O.exponential_decay(2, 2, 2, 0.003)], rtol=1e-12)


def test_resume_from_a_checkpoint(tmp_path):
    FLAGS, sh, hist, text = _run(tmp_path, [5.0], ["--min_epochs", "1", "--max_epochs", "1"], have_checkpoint=True)
    assert "[*] Load SUCCESS" in text and "[!] Begin a new model." not in text and sh.loads == [FLAGS.save_dir]


class Decoder(object):
    def __init__(self, FLAGS, dout):
        self.save_dir, self.dout, self.calls = FLAGS.save_dir, dout, []

    def load(self, save_dir, moving_average=False):
        self.calls.append(("load", save_dir, moving_average))
        return True

    def forward(self, x, ln):
        self.calls.append(("forward", x.shape, x.dtype, float(x.sum()), ln.tolist()))
        return np.cumsum(x[:, :, :self.dout], axis=1)


def test_decode_with_defaults_is_run_gan_rnn_decode(tmp_path):
    rng = np.random.default_rng(3)
    din, dout = 5, 3
    te = _data(tmp_path, 3, "te", rng, din, dout)
    np.savez(tmp_path / "train_cmvn.npz", mean_inputs=np.full(din, 1.0), stddev_inputs=np.full(din, 2.0),
             mean_labels=np.full(dout, -1.0), stddev_labels=np.full(dout, 1.5))
    outs, calls = [], []
    for mod, sub in ((R, "a"), (G, "b")):
        FLAGS, _ = mod.build_parser().parse_known_args(["--decode", "--data_dir", str(tmp_path), "--test_inputs_scp", te[0], "--input_dim", str(din),
                                                        "--output_dim", str(dout), "--left_context", "1", "--right_context", "1",
                                                        "--save_dir", str(tmp_path / sub)])
        assert FLAGS.decode_chunk == 0 and FLAGS.decode_streams == 1
        dec = Decoder(FLAGS, dout)
        scp = mod.decode(FLAGS, model_factory=lambda: dec, log=lambda s: None)
        assert scp == os.path.join(str(tmp_path / sub), "test", "feats.scp")
        r = ArkReader(); r(scp)
        outs.append([(u, r.read_utt_data_from_index(i)) for i, u in enumerate(r.utt_ids)])
        calls.append([c if c[0] != "load" else ("load", os.path.basename(c[1]), c[2]) for c in dec.calls])
    assert calls[0][1:] == calls[1][1:] and calls[0][0] == ("load", "a", False) and len(calls[0]) == 4
    for (ua, a), (ub, b) in zip(*outs):
        assert ua == ub and np.array_equal(a, b)


def test_enumerator_and_default_cfg_on_the_loaded_library():
    from rsrgan_amd import _lib
    assert _lib.G_TYPES["res_lstm_i"] == 6
    lib = _lib.load()
    cfg = _lib.RsrganCfg()
    assert lib.rsrgan_default_cfg(6, C.byref(cfg)) == 0
    assert (cfg.g_type, cfg.g_layers, cfg.g_cells, cfg.g_proj) == (6, 2, 760, 257)
    assert lib.rsrgan_default_cfg(9, C.byref(cfg)) != 0 and b"Unrecognized G type" in lib.rsrgan_last_error()


def test_gan_rnn_still_refuses_it():
    from rsrgan_amd import GAN_RNN
    from tests.helpers import args_for
    with pytest.raises(ValueError, match="Unrecognized G type"):
        GAN_RNN(None, args_for(O.NetCfg(g_type="res_lstm_i"), 2), ["cpu:0"], engine=object())
