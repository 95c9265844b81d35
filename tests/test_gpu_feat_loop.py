"""The device-side feature front end through the call sites: the same archives, the same seeds, once through the default reader (CMVN,
splice and padding on the host, the expanded batch uploaded) and once through PaddedBatchReader(device_features=True) (packed raw frames
uploaded, HipEngine.featurize expands them with csrc/feat.hip).  The front end gives the host path's bits and the library has no
atomics, so everything downstream is EQUAL: the 7 averages of train_one_iteration, every generator and discriminator variable after two
iterations, the same for the supervised loop on RNNTrainer, and the bytes of feats.ark / feats.scp that --decode writes, whole-utterance
and with --decode_chunk 3 --decode_streams 2."""
import os

import numpy as np
import pytest

from rsrgan_amd.io import PaddedBatchReader
from tests import feat_ref
from tests.helpers import args_for, overrides, small_cfg

pytestmark = pytest.mark.gpu

LEFT, RIGHT, B = 2, 1, 4
LENGTHS = [7, 3, 9, 5, 6, 2, 9, 4, 8, 1]           # shuffled into two full windows of 4 and a partial one the loops skip


@pytest.fixture()
def counted(monkeypatch):
    """how often HipEngine.featurize ran"""
    from rsrgan_amd.engine_hip import HipEngine
    calls = []
    real = HipEngine.featurize

    def featurize(self, packed, *a, **k):
        calls.append((packed.shape, k.get("ready", False)))
        return real(self, packed, *a, **k)
    monkeypatch.setattr(HipEngine, "featurize", featurize)
    return calls


def _data(tmp_path):
    cfg = small_cfg("lstm")
    rng = np.random.default_rng(21)
    scp = feat_ref.write_arks(tmp_path, "tr", LENGTHS, cfg.input_dim, cfg.output_dim, rng)
    return cfg, scp, feat_ref.cmvn_for(rng, cfg.input_dim, cfg.output_dim)


def _reader(scp, cmvn, dev):
    return PaddedBatchReader(scp[0], scp[1], B, LEFT, RIGHT, cmvn=cmvn, num_buckets=1, shuffle=True, seed=5, device_features=dev)


def _same_vars(a, b):
    ga, da = a.get_vars(); gb, db = b.get_vars()
    assert set(ga) == set(gb) and set(da) == set(db) and len(ga) > 0
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    for k in da:
        assert np.array_equal(da[k], db[k]), k


def test_gan_iterations_are_equal(tmp_path, counted):
    from rsrgan_amd import GAN_RNN, train_one_iteration
    cfg, scp, cmvn = _data(tmp_path)
    args = args_for(cfg, B, left_context=LEFT, right_context=RIGHT, disc_updates=1, gen_updates=2, l2_scale=1e-4)
    res, models = [], []
    for dev in (False, True):
        m = GAN_RNN(None, args, ["gpu:0"], max_frames=max(LENGTHS), net_overrides=overrides(cfg))
        rd = _reader(scp, cmvn, dev)
        n0 = len(counted)
        res.append([train_one_iteration(None, m, 3, it, rd) for it in range(2)])
        assert len(counted) - n0 == (8 if dev else 0)            # 2 iterations x 2 full batches x (labels, inputs)
        models.append(m)
    assert all(np.all(np.isfinite(r)) for r in res[0]) and res[0][0] != res[0][1]
    assert res[0] == res[1], (res[0], res[1])
    _same_vars(*models)
    # labels (and lengths) complete on return under the pipelined D-run, the inputs in stream order
    assert [r for _, r in counted[-2:]] == [os.environ.get("RSRGAN_DPIPE", "0") not in ("", "0"), False]
    # cross-validation on the trained pair: the twin's averages are equal too
    from rsrgan_amd import eval_one_iteration
    cv = [eval_one_iteration(None, GAN_RNN(None, args, ["gpu:0"], cross_validation=True, share_engine_from=m), 3, 0,
                             [b for b in _reader(scp, cmvn, dev) if len(b[0]) == B]) for m, dev in zip(models, (False, True))]
    assert cv[0] == cv[1] and np.all(np.isfinite(cv[0]))


def test_supervised_iterations_are_equal(tmp_path, counted):
    from rsrgan_amd import run_rnn as R
    from rsrgan_amd.trainer import RNNTrainer
    cfg, scp, cmvn = _data(tmp_path)
    args = args_for(cfg, B, left_context=LEFT, right_context=RIGHT, g_learning_rate=1e-3, l2_scale=1e-4)
    res, models = [], []
    for dev in (False, True):
        m = RNNTrainer(None, args, ["gpu:0"], max_frames=max(LENGTHS), net_overrides=overrides(cfg))
        n0 = len(counted)
        res.append([R.train_one_iteration(m, 3, it, _reader(scp, cmvn, dev)) for it in range(2)])
        assert len(counted) - n0 == (8 if dev else 0)
        res[-1].append(R.eval_one_iteration(RNNTrainer(None, args, ["gpu:0"], cross_validation=True, share_engine_from=m), 3, 0,
                                            _reader(scp, cmvn, dev)))
        models.append(m)
    assert np.all(np.isfinite(res[0])) and res[0][0] != res[0][1]
    assert res[0] == res[1], (res[0], res[1])
    ga, gb = models[0].get_vars()[0], models[1].get_vars()[0]
    assert len(ga) > 0 and all(np.array_equal(ga[k], gb[k]) for k in ga)


def test_an_utterance_longer_than_max_frames_is_refused_before_device_work(tmp_path):
    from rsrgan_amd import GAN_RNN
    cfg, scp, cmvn = _data(tmp_path)
    m = GAN_RNN(None, args_for(cfg, B, left_context=LEFT, right_context=RIGHT), ["gpu:0"], max_frames=8, net_overrides=overrides(cfg))
    item = next(b for b in _reader(scp, cmvn, True) if max(b[3]) == 9)
    with pytest.raises(ValueError, match="longer than max_frames = 8"):
        m.engine.featurize(item[1])
    fits = feat_ref.random_packed(np.random.default_rng(1), [8, 3, 5, 1], cfg.input_dim, LEFT, RIGHT)
    x, ln = m.engine.featurize(fits, ready=True)                      # (complete on return: no synchronize before the copies below)
    want, want_len = feat_ref.expand(fits, None, LEFT, RIGHT, 8)
    assert np.array_equal(x.cpu().numpy(), want) and ln.cpu().tolist() == want_len.tolist() == [8, 3, 5, 1]


@pytest.mark.parametrize("extra", [[], ["--decode_chunk", "3", "--decode_streams", "2"]], ids=["whole", "chunked"])
def test_decode_writes_the_same_bytes(tmp_path, counted, extra):
    from rsrgan_amd import GAN_RNN
    from rsrgan_amd import run_gan_rnn as G
    cfg = small_cfg("lstm")
    rng = np.random.default_rng(33)
    te = feat_ref.write_arks(tmp_path, "te", [7, 4, 10, 1, 6], cfg.input_dim, cfg.output_dim, rng)
    np.savez(tmp_path / "train_cmvn.npz", **feat_ref.cmvn_for(rng, cfg.input_dim, cfg.output_dim))
    base = ["--decode", "--data_dir", str(tmp_path), "--test_inputs_scp", te[0], "--input_dim", str(cfg.input_dim), "--output_dim",
            str(cfg.output_dim), "--left_context", str(LEFT), "--right_context", str(RIGHT), "--save_dir", str(tmp_path / "exp"),
            "--max_frames", "16", "--g_type", "lstm"] + extra
    ov = overrides(cfg)
    FLAGS = G.build_parser().parse_args(base)
    GAN_RNN(None, FLAGS, ["gpu:0"], max_frames=16, net_overrides=ov).save(FLAGS.save_dir, 1)
    written = []
    for flag in ([], ["--device_features"]):
        FLAGS = G.build_parser().parse_args(base + flag)
        n0 = len(counted)
        scp = G.decode(FLAGS, log=lambda s: None, net_overrides=ov)
        assert len(counted) - n0 == (5 if flag else 0)
        written.append((open(scp, "rb").read(), open(scp[:-4] + ".ark", "rb").read()))
    assert len(written[0][1]) > 5 * 4 * cfg.output_dim and written[0][0].count(b"\n") == 5
    assert written[0][0] == written[1][0] and written[0][1] == written[1][1]
