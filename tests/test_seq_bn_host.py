"""Host logic of args.batch_norm on the sequence path (no GPU: a recording engine): which g_types pass the flag to the engine, and
what sync_batch_norm_state exchanges."""
import numpy as np
import pytest
import torch

from rsrgan_amd import GAN_RNN, dist as rdist
from rsrgan_amd.trainer import RNNTrainer
from tests import seq_bn_ref as R
from tests.helpers import NET_G, args_for, small_cfg


class RecordingEngine:
    """stands in for HipEngine: keeps the keyword arguments it was built with and one flat vector per net"""
    ema_enabled = True
    built = []

    def __init__(self, **kw):
        self.kw = kw
        self.device = torch.device("cpu")
        self.scalars = {}
        RecordingEngine.built.append(self)

    def set_scalar(self, k, v):
        self.scalars[k] = v

    def set_dropout(self, keep, seed):
        pass


@pytest.fixture
def recording(monkeypatch):
    import rsrgan_amd.engine_hip as eh
    RecordingEngine.built = []
    monkeypatch.setattr(eh, "HipEngine", RecordingEngine)
    return RecordingEngine


@pytest.mark.parametrize("cls", [GAN_RNN, RNNTrainer])
def test_only_g_type_lstm_passes_the_flag(recording, cls, capsys):
    m = cls(None, args_for(small_cfg(), 2, batch_norm=True), ["gpu:0"], max_frames=4)
    assert m.engine.kw.get("batch_norm") is True and m.engine_batch_norm
    m = cls(None, args_for(small_cfg(), 2), ["gpu:0"], max_frames=4)
    assert "batch_norm" not in m.engine.kw
    capsys.readouterr()
    for g_type in ("res_lstm_l", "res_lstm_base") + (("res_lstm_i",) if cls is RNNTrainer else ()):
        cfg = small_cfg(g_type)
        with_flag = cls(None, args_for(cfg, 2, batch_norm=True), ["gpu:0"], max_frames=4)
        out = capsys.readouterr().out
        without = cls(None, args_for(cfg, 2), ["gpu:0"], max_frames=4)
        assert with_flag.engine.kw == without.engine.kw and "batch_norm" not in with_flag.engine.kw        # the same handle
        assert out.count("\n") == 1 and "ignores" in out and g_type in out                                  # one line of log
        assert not with_flag.engine_batch_norm and with_flag.sync_batch_norm_state() == 0


def test_bnlstm_still_refuses_batch_norm(recording):
    with pytest.raises(NotImplementedError, match="bnlstm"):
        RNNTrainer(None, args_for(small_cfg(), 2, g_type="bnlstm", batch_norm=True), ["gpu:0"], max_frames=4)
    assert not recording.built


class TableEngine:
    """the engine protocol sync_batch_norm_state touches, over the variable table of the batch-normalised generator"""
    ema_enabled = True

    def __init__(self, cfg, value):
        self.device = torch.device("cpu")
        self.table, off = [], 0
        for name, shape in R.g_param_specs(cfg):
            shape = (1,) if tuple(shape) == () else tuple(shape)
            self.table.append((name, shape, off))
            off += int(np.prod(shape))
        self.flat = torch.full((off,), float(value))
        self.sets = 0

    def tensor_table(self, net):
        assert net == NET_G
        return self.table

    def get_params(self, net, what="variables"):
        assert net == NET_G and what == "variables"
        return self.flat.clone()

    def set_params(self, net, flat, what="variables"):
        assert net == NET_G and what == "variables"
        self.flat = flat.clone()
        self.sets += 1

    def set_scalar(self, k, v):
        pass


@pytest.mark.parametrize("cls", [GAN_RNN, RNNTrainer])
def test_sync_averages_the_six_statistics_and_nothing_else(monkeypatch, cls):
    cfg = small_cfg()
    eng = TableEngine(cfg, 1.0)
    m = cls(None, args_for(cfg, 2, batch_norm=True), ["cpu:0"], engine=eng)
    assert m.sync_batch_norm_state() == 0 and eng.sets == 0                 # one process: nothing to exchange
    sent = []

    def fake_mean(t, group=None):                                            # the other rank holds 3.0 everywhere
        sent.append(t.numel())
        t.mul_(0.5).add_(1.5)
    monkeypatch.setattr(rdist, "world_size", lambda group=None: 2)
    monkeypatch.setattr(rdist, "all_reduce_mean_", fake_mean)
    P = cfg.g_proj
    n = m.sync_batch_norm_state()
    assert n == 4 * P + 2 and sent == [n] and eng.sets == 1
    for name, shape, off in eng.table:
        got = eng.flat[off:off + int(np.prod(shape))]
        leaf = name.rsplit("/", 1)[-1]
        is_stat = "/BatchNorm/" in name and leaf not in ("beta", "gamma")
        assert bool((got == (2.0 if is_stat else 1.0)).all()), name
    assert sum(1 for name, _, _ in eng.table if "/BatchNorm/" in name) == 8
    # without the flag: no exchange, whatever the table holds
    m0 = cls(None, args_for(cfg, 2), ["cpu:0"], engine=TableEngine(cfg, 1.0))
    assert m0.sync_batch_norm_state() == 0
