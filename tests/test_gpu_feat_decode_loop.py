"""The device decode through its call sites, over small archives that hold Kaldi-compressed, double and float utterances (6 input and 3
label dimensions, ragged lengths, several shorter than the context): HipEngine.featurize on the items of
PaddedBatchReader(device_decode=True) and HipEngine.featurize_frames on those of FrameBatchReader(device_decode=True) give the default
readers' batches bit for bit, labels and lengths included; one train_one_iteration fed by the device_decode reader ends on the losses
and variables of one fed by the default reader; --decode --device_decode writes the archive --decode writes."""
import numpy as np
import pytest
import torch

from rsrgan_amd.io import FrameBatchReader, PaddedBatchReader
from tests import feat_decode_ref as R
from tests.feat_ref import cmvn_for
from tests.helpers import args_for, overrides, small_cfg

pytestmark = pytest.mark.gpu

LEFT, RIGHT, B = 5, 5, 4
DIN, DOUT = 6, 3
LENGTHS = [7, 3, 9, 5, 6, 2, 9, 4, 8, 1]           # two full windows of 4 and a partial one the loops skip


def _cfg():
    return small_cfg("lstm", input_dim=DIN, output_dim=DOUT)


def _bits_equal(t, want):
    return torch.equal(t.cpu().view(torch.int32), torch.from_numpy(np.ascontiguousarray(want, np.float32)).view(torch.int32))


def _reader(scp, cmvn, dev):
    return PaddedBatchReader(scp[0], scp[1], B, LEFT, RIGHT, cmvn=cmvn, num_buckets=1, shuffle=True, seed=5, device_decode=dev)


@pytest.fixture()
def counted(monkeypatch):
    """how often the device decode was launched"""
    from rsrgan_amd.engine_hip import HipEngine
    calls = []
    real = HipEngine.op_feat_decode

    def op_feat_decode(self, *a, **k):
        calls.append(a[4])
        return real(self, *a, **k)
    monkeypatch.setattr(HipEngine, "op_feat_decode", op_feat_decode)
    return calls


@pytest.mark.parametrize("kinds", ["C", "CDF"], ids=["compressed", "mixed"])
def test_featurize_equals_the_default_readers_items(tmp_path, counted, kinds):
    from rsrgan_amd import GAN_RNN
    cfg = _cfg()
    rng = np.random.default_rng(21)
    scp = R.write_arks(tmp_path, "tr", LENGTHS, DIN, DOUT, rng, kinds=kinds)
    cmvn = cmvn_for(rng, DIN, DOUT)
    m = GAN_RNN(None, args_for(cfg, B, left_context=LEFT, right_context=RIGHT), ["gpu:0"], max_frames=max(LENGTHS), net_overrides=overrides(cfg))
    want, got = list(_reader(scp, cmvn, False)), list(_reader(scp, cmvn, True))
    assert len(want) == len(got) == 3
    for k, (w, g) in enumerate(zip(want, got)):
        assert g[0] == w[0]
        x, ln = m.engine.featurize(g[1], ready=bool(k % 2))
        lab, ln2 = m.engine.featurize(g[2], ready=True)
        torch.cuda.synchronize()
        assert x.shape == w[1].shape and lab.shape == w[2].shape
        assert _bits_equal(x, w[1]) and _bits_equal(lab, w[2]), k
        assert ln.cpu().tolist() == ln2.cpu().tolist() == w[3].tolist() == g[3].tolist()
    assert counted == [len(w[0]) for w in want for _ in range(2)]          # one decode launch per side, B utterances each
    m.engine.max_frames = 8                                                # (the limit is checked before any device work)
    with pytest.raises(ValueError, match="longer than max_frames = 8"):
        m.engine.featurize(next(g for g in got if max(g[3]) == 9)[1])
    assert len(counted) == 6
    m.engine.close()


@pytest.mark.parametrize("with_cmvn,shuffle", [(True, True), (False, False)], ids=["cmvn-shuffled", "raw-in-order"])
def test_featurize_frames_equals_the_default_readers_batches(tmp_path, counted, with_cmvn, shuffle):
    from types import SimpleNamespace
    from rsrgan_amd import GAN
    args = SimpleNamespace(batch_size=32, input_dim=DIN, output_dim=DOUT, left_context=2, right_context=1, g_type="dnn", save_dir=None)
    engine = GAN(None, args, ["gpu:0"], net_overrides=dict(g_layers=2, g_cells=32, d_layers=2, d_cells=16)).engine
    rng = np.random.default_rng(31)
    lengths = rng.integers(80, 90, 25) if shuffle else rng.integers(40, 90, 25)
    scp = R.write_arks(tmp_path, "fr", lengths, DIN, DOUT, rng, kinds="CCD")
    cmvn = cmvn_for(rng, DIN, DOUT) if with_cmvn else None
    mk = lambda **k: FrameBatchReader(scp[0], scp[1], 32, 2, 1, cmvn=cmvn, num_threads=0, shuffle=shuffle, seed=3, **k)
    want, dev = list(mk()), mk(device_decode=True, initial_pool_rows=64)
    got = 0
    for k, item in enumerate(dev):
        x, lab = engine.featurize_frames(item, ready=bool(k % 2))
        torch.cuda.synchronize()
        assert _bits_equal(x, want[k][0]) and _bits_equal(lab, want[k][1]), k
        got += 1
    assert got == len(want) == int(lengths.sum()) // 32
    st = engine.frame_pool_stats(dev.reader_id)
    assert st["uploads"] == 25 and st["pool_rows"] == dev.allocator.pool_rows > 64
    assert len(counted) == 2 * 25 and set(counted) == {1}                  # every admission decoded straight into its slot, inputs and labels
    engine.close()


def test_one_training_iteration_is_equal(tmp_path, counted):
    from rsrgan_amd import GAN_RNN, train_one_iteration
    cfg = _cfg()
    rng = np.random.default_rng(22)
    scp = R.write_arks(tmp_path, "tr", LENGTHS, DIN, DOUT, rng, kinds="C")
    cmvn = cmvn_for(rng, DIN, DOUT)
    args = args_for(cfg, B, left_context=LEFT, right_context=RIGHT, disc_updates=1, gen_updates=2, l2_scale=1e-4)
    res, models = [], []
    for dev in (False, True):
        m = GAN_RNN(None, args, ["gpu:0"], max_frames=max(LENGTHS), net_overrides=overrides(cfg))
        n0 = len(counted)
        res.append(train_one_iteration(None, m, 3, 0, _reader(scp, cmvn, dev)))
        assert len(counted) - n0 == (4 if dev else 0)                      # 2 full batches x (labels, inputs)
        models.append(m)
    assert np.all(np.isfinite(res[0])) and res[0] == res[1], (res[0], res[1])
    (ga, da), (gb, db) = models[0].get_vars(), models[1].get_vars()
    assert set(ga) == set(gb) and set(da) == set(db) and len(ga) > 0 and len(da) > 0
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    for k in da:
        assert np.array_equal(da[k], db[k]), k


def test_frame_level_decode_writes_the_same_archive(tmp_path, counted):
    """run_gan_dnn --decode --device_decode: B = 1, T = the longest utterance, zero rows behind the shorter ones"""
    from rsrgan_amd import GAN
    from rsrgan_amd import run_gan_dnn as RD
    rng = np.random.default_rng(44)
    lengths = [7, 1, 12, 3]
    items = [("te%02d" % i, rng.standard_normal((n, DIN)) * 2 + 1, "CCDF"[i]) for i, n in enumerate(lengths)]
    R.write_archive(str(tmp_path / "te_in.ark"), str(tmp_path / "te_in.scp"), items)
    np.savez(tmp_path / "train_cmvn.npz", **cmvn_for(rng, DIN, DOUT))
    ov = dict(g_layers=2, g_cells=32, d_layers=2, d_cells=16)
    base = ["--decode", "--data_dir", str(tmp_path), "--test_inputs_scp", str(tmp_path / "te_in.scp"), "--input_dim", str(DIN), "--output_dim",
            str(DOUT), "--left_context", "2", "--right_context", "1", "--batch_size", "16", "--save_dir", str(tmp_path / "exp")]
    FLAGS = RD.build_parser().parse_args(base)
    GAN(None, FLAGS, ["gpu:0"], net_overrides=ov).save(FLAGS.save_dir, 1)
    written = []
    for flag in ([], ["--device_decode"]):
        FLAGS = RD.build_parser().parse_args(base + flag)
        n0 = len(counted)
        scp = RD.decode(FLAGS, log=lambda s: None, net_overrides=ov)
        assert len(counted) - n0 == (4 if flag else 0)
        written.append((open(scp, "rb").read(), open(scp[:-4] + ".ark", "rb").read()))
    assert len(written[0][1]) > sum(lengths) * 4 * DOUT and written[0][0].count(b"\n") == 4
    assert written[0][0] == written[1][0] and written[0][1] == written[1][1]


def test_decode_writes_the_same_archive(tmp_path, counted):
    from rsrgan_amd import GAN_RNN
    from rsrgan_amd import run_gan_rnn as G
    cfg = _cfg()
    rng = np.random.default_rng(33)
    lengths = [7, 4, 10, 1, 6]
    items = [("te%03d" % i, rng.standard_normal((n, DIN)) * 2 + 1, "CDCFC"[i]) for i, n in enumerate(lengths)]
    R.write_archive(str(tmp_path / "te_in.ark"), str(tmp_path / "te_in.scp"), items)
    np.savez(tmp_path / "train_cmvn.npz", **cmvn_for(rng, DIN, DOUT))
    base = ["--decode", "--data_dir", str(tmp_path), "--test_inputs_scp", str(tmp_path / "te_in.scp"), "--input_dim", str(DIN), "--output_dim",
            str(DOUT), "--left_context", str(LEFT), "--right_context", str(RIGHT), "--save_dir", str(tmp_path / "exp"), "--max_frames", "16",
            "--g_type", "lstm"]
    ov = overrides(cfg)
    FLAGS = G.build_parser().parse_args(base)
    GAN_RNN(None, FLAGS, ["gpu:0"], max_frames=16, net_overrides=ov).save(FLAGS.save_dir, 1)
    written = []
    for flag in ([], ["--device_decode"]):
        FLAGS = G.build_parser().parse_args(base + flag)
        assert FLAGS.device_decode is bool(flag) and not FLAGS.device_features
        n0 = len(counted)
        scp = G.decode(FLAGS, log=lambda s: None, net_overrides=ov)
        assert len(counted) - n0 == (5 if flag else 0)
        written.append((open(scp, "rb").read(), open(scp[:-4] + ".ark", "rb").read()))
    assert len(written[0][1]) > sum(lengths) * 4 * DOUT and written[0][0].count(b"\n") == 5
    assert written[0][0] == written[1][0] and written[0][1] == written[1][1]
