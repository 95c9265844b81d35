"""The frame-level device-side front end through its call sites.

(a) A whole pass of FrameBatchReader(device_features=True) through HipEngine.featurize_frames -- pool growth, normalise-once uploads and
    the k_feat_frames gathers on the device -- gives the default reader's batches with the same seed, bit for bit.  The initial pool is
    small enough that it grows on the device, and rows an utterance has left are handed out again: within the pass for the in-order
    reader, and by the second pass for the shuffled one (a shuffled queue of 1000 frames lets go of an utterance's last frame only after
    all 25 utterances were enqueued).
(b) run_gan_dnn.train for one epoch on a small net, once on the host path and once with --device_features: the front end gives the host
    path's bits and the library has no atomics, so every generator and discriminator variable is EQUAL, the summaries' losses are, and
    --decode writes byte-equal feats.ark / feats.scp.
(c) A counter shows HipEngine.featurize_frames (training) and HipEngine.featurize (decode) ran on the flagged path and only there."""
import glob
import os

import numpy as np
import pytest
import torch

from rsrgan_amd.io import ArkWriter, FrameBatchReader
from tests import feat_frames_ref as R
from tests.feat_ref import cmvn_for

pytestmark = pytest.mark.gpu

OV = dict(g_layers=2, g_cells=32, d_layers=2, d_cells=16)


@pytest.fixture(scope="module")
def engine():
    """any engine will do: the front end does not depend on the nets"""
    from types import SimpleNamespace
    from rsrgan_amd import GAN
    args = SimpleNamespace(batch_size=32, input_dim=3, output_dim=2, left_context=1, right_context=1, g_type="dnn", save_dir=None)
    m = GAN(None, args, ["gpu:0"], net_overrides=OV)
    yield m.engine
    m.engine.close()


def _bits_equal(t, want):
    return torch.equal(t.cpu().view(torch.int32), torch.from_numpy(np.ascontiguousarray(want, np.float32)).view(torch.int32))


@pytest.mark.parametrize("din,dout,ctx,with_cmvn,shuffle", [(3, 2, 1, True, True), (3, 2, 1, False, False), (257, 40, 5, True, True)],
                         ids=["cmvn-shuffled", "raw-in-order", "257x11-cmvn-shuffled"])
def test_a_whole_pass_equals_the_default_reader(tmp_path, engine, din, dout, ctx, with_cmvn, shuffle):
    rng = np.random.default_rng(100 + din)
    # 25 utterances of 40 .. 89 frames.  The shuffled cases draw them from 80 .. 89: nothing leaves a shuffled queue before everything
    # is in it, so the pool must hold all 25 slots, more than the 2048 rows it has when the first batch is drawn -- it grows ON THE DEVICE,
    # with live rows to carry over.  The in-order reader frees slots as it goes and reuses them within the pass.
    lengths = rng.integers(80, 90, 25) if shuffle else None
    xs, ls, total = R.frame_data(tmp_path, 25, rng, din=din, dout=dout, lengths=lengths, random_values=True)
    cmvn = cmvn_for(rng, din, dout) if with_cmvn else None
    mk = lambda dev, **k: FrameBatchReader(xs, ls, 32, ctx, ctx, cmvn=cmvn, num_threads=0, shuffle=shuffle, seed=3, device_features=dev, **k)
    host, dev = mk(False), mk(True, initial_pool_rows=64)
    mirror = R.HostPool(dev.reader_id)                    # the stand-in runs beside the engine: it counts reuses and checks the allocator
    assert engine.frame_pool_stats(dev.reader_id) is None
    batches = 0
    for _pass in range(2):
        want = list(host)
        got = 0
        mirror.new_pass()
        for k, item in enumerate(dev):
            mirror.feed(item)
            x, lab = engine.featurize_frames(item, ready=bool(k % 2))        # (ready: complete on return; else in stream order, by event)
            assert x.shape == (32, din * (2 * ctx + 1)) and lab.shape == (32, dout) and x.dtype == lab.dtype == torch.float32
            assert _bits_equal(x, want[k][0]), "inputs of batch %d, pass %d" % (k, _pass)
            assert _bits_equal(lab, want[k][1]), "labels of batch %d, pass %d" % (k, _pass)
            got += 1
        assert got == len(want) == total // 32
        batches += got
        if _pass == 0 and not shuffle:
            assert mirror.reuses >= 1, "no freed slot was handed out again within the pass"
    st = engine.frame_pool_stats(dev.reader_id)
    assert st["items"] == batches and st["uploads"] == 50 and mirror.reuses >= 1
    if shuffle:
        assert st["growths"] >= 1 and mirror.growths >= 1 and st["pool_rows"] == 4096, "the pool did not grow on the device"
    assert st["pool_rows"] == dev.allocator.pool_rows > 64 and st["bytes"] == st["pool_rows"] * (din + dout) * 4
    # an item that is not the next one of its pool is refused before any device work: the pool's counters stay
    stale = next(iter(mk(True, initial_pool_rows=64)))
    stale.reader_id = dev.reader_id
    with pytest.raises(ValueError, match="out of order"):
        engine.featurize_frames(stale)
    assert engine.frame_pool_stats(dev.reader_id)["items"] == batches
    engine.drop_frame_pool(dev.reader_id)
    assert engine.frame_pool_stats(dev.reader_id) is None


@pytest.fixture()
def counted(monkeypatch):
    """how often the two front ends ran"""
    from rsrgan_amd.engine_hip import HipEngine
    calls = {"frames": 0, "batch": 0}
    real_f, real_b = HipEngine.featurize_frames, HipEngine.featurize

    def featurize_frames(self, item, *a, **k):
        calls["frames"] += 1
        return real_f(self, item, *a, **k)

    def featurize(self, packed, *a, **k):
        calls["batch"] += 1
        return real_b(self, packed, *a, **k)
    monkeypatch.setattr(HipEngine, "featurize_frames", featurize_frames)
    monkeypatch.setattr(HipEngine, "featurize", featurize)
    return calls


def test_training_and_decode_are_equal_on_both_paths(tmp_path, counted):
    from rsrgan_amd import GAN
    from rsrgan_amd import run_gan_dnn as RD
    from rsrgan_amd import summary as S
    rng = np.random.default_rng(0)
    din, dout = 6, 4

    def data(tag, lengths):
        wi, wl = ArkWriter(str(tmp_path / (tag + "_in.scp"))), ArkWriter(str(tmp_path / (tag + "_lab.scp")))
        for i, T in enumerate(lengths):
            wi.write_next_utt(str(tmp_path / (tag + "_in.ark")), "%s%02d" % (tag, i), (rng.standard_normal((T, din)) * 2 + 1).astype(np.float32))
            wl.write_next_utt(str(tmp_path / (tag + "_lab.ark")), "%s%02d" % (tag, i), (rng.standard_normal((T, dout)) - 1).astype(np.float32))
        wi.close(); wl.close()
        return str(tmp_path / (tag + "_in.scp")), str(tmp_path / (tag + "_lab.scp"))
    tr, cv = data("tr", rng.integers(60, 100, 30)), data("cv", rng.integers(60, 100, 8))
    te = data("te", [7, 1, 12, 3])                              # decode: utterances shorter than the context, padded to the longest
    np.savez(tmp_path / "train_cmvn.npz", **cmvn_for(rng, din, dout))
    res = []
    for flag in ([], ["--device_features"]):
        save = str(tmp_path / ("exp_dev" if flag else "exp_host"))
        FLAGS = RD.build_parser().parse_args([
            "--data_dir", str(tmp_path), "--tr_inputs_scp", tr[0], "--tr_labels_scp", tr[1], "--cv_inputs_scp", cv[0], "--cv_labels_scp", cv[1],
            "--test_inputs_scp", te[0], "--input_dim", str(din), "--output_dim", str(dout), "--left_context", "2", "--right_context", "1",
            "--batch_size", "64", "--min_epoches", "1", "--max_epoches", "1", "--save_dir", save, "--g_learning_rate", "0.003",
            "--d_learning_rate", "0.001", "--batch_norm", "true", "--init_mse_weight", "10", "--num_threads", "2", "--gen_updates", "2"] + flag)
        assert FLAGS.device_features is bool(flag)
        made = []

        def factory():
            made.append(GAN(None, FLAGS, ["gpu:0"], net_overrides=OV))
            return made[-1]
        n0 = dict(counted)
        hist = RD.train(FLAGS, model_factory=factory, log=lambda s: None)
        model = made[0]
        used = counted["frames"] - n0["frames"]
        # (c) two cross-validation passes and one training pass, a fresh batch per run: int(batches / 3) rounds of 3
        tr_b, cv_b = (int(v) for v in open(tmp_path / "batch_num.txt").read().split()[1::-1])
        assert used == (3 * (tr_b // 3) + 2 * 3 * (cv_b // 3) if flag else 0) and tr_b >= 6 and cv_b >= 3
        if flag:
            pools = [model.engine.frame_pool_stats(r) for r in model.engine.frame_pool_readers()]
            assert len(pools) == 2 and all(p["items"] > 0 for p in pools)                   # training and cross-validation reader: two pools
        model.save(save, 7)                                      # (whatever the accept / reject rule did: decode needs a checkpoint)
        g, d = model.get_vars()
        events = {sub: S.read_events(glob.glob(os.path.join(save, sub, "events.out.tfevents.*"))[0]) for sub in ("train", "eval")}
        FLAGS.decode = True
        n1 = counted["batch"]
        scp = RD.decode(FLAGS, log=lambda s: None, net_overrides=OV)
        assert counted["batch"] - n1 == (4 if flag else 0)
        res.append((hist, g, d, events, open(scp, "rb").read().replace(save.encode(), b"SAVE"), open(scp[:-4] + ".ark", "rb").read()))
        model.engine.close()
    (h0, g0, d0, e0, s0, a0), (h1, g1, d1, e1, s1, a1) = res
    assert np.all(np.isfinite(h0)) and h0 == h1
    assert set(g0) == set(g1) and set(d0) == set(d1) and len(g0) > 0 and len(d0) > 0
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
    for k in d0:
        assert np.array_equal(d0[k], d1[k]), k
    for sub in ("train", "eval"):                                # the summary fetch on the last batch took device tensors: the same scalars
        assert len(e0[sub]) == len(e1[sub]) >= 2
        for a, b in zip(e0[sub][1:], e1[sub][1:]):
            assert a[2]["g_loss"] == b[2]["g_loss"] and a[2]["d_loss"] == b[2]["d_loss"] and np.isfinite(a[2]["g_loss"])
            assert a[2]["g_clean"]["num"] == b[2]["g_clean"]["num"] == 64 * dout
    assert len(a0) > 23 * 4 * dout and s0.count(b"\n") == 4
    assert s0 == s1 and a0 == a1
