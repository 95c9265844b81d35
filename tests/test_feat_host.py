"""The host side of the device-side feature front end: PaddedBatchReader(device_features=True) ships packed raw frames, and their host
expansion (tests/feat_ref.py: apply_cmvn, splice_feats, the padding rule) is the default reader's batch bit for bit -- same ids, same
order, same lengths; PackedBatch.rows shards as GAN_RNN._shard shards an expanded batch; a float64 archive is refused; the call sites
pass other items through and refuse packed ones on an engine without a device front end (no host fallback)."""
from types import SimpleNamespace

import numpy as np
import pytest

from rsrgan_amd import run_gan_rnn as G
from rsrgan_amd import run_rnn as R
from rsrgan_amd.gan_rnn import GAN_RNN
from rsrgan_amd.io import PackedBatch, PaddedBatchReader, pack_utterances, prefetch
from rsrgan_amd.train import device_batch, is_packed
from tests import feat_ref

DIN, DOUT = 6, 3
LENGTHS = [7, 1, 12, 4, 9, 2, 5, 12, 3, 8, 6]           # ragged, shorter than either context, 11 = 2 full windows of 4 + a partial one


def _readers(tmp_path, cmvn, left, right, seed, shuffle=True, **kw):
    rng = np.random.default_rng(11)
    scp = feat_ref.write_arks(tmp_path, "tr", LENGTHS, DIN, DOUT, rng)
    mk = lambda dev: PaddedBatchReader(scp[0], scp[1], 4, left, right, cmvn=cmvn, num_buckets=1, shuffle=shuffle, seed=seed,
                                       device_features=dev, **kw)
    return mk(False), mk(True)


@pytest.mark.parametrize("with_cmvn", [True, False])
@pytest.mark.parametrize("left,right", [(5, 5), (2, 1), (0, 0)])
def test_packed_reader_expands_to_the_default_readers_items(tmp_path, with_cmvn, left, right):
    cmvn = feat_ref.cmvn_for(np.random.default_rng(5), DIN, DOUT) if with_cmvn else None
    host, dev = _readers(tmp_path, cmvn, left, right, seed=77)
    assert list(host.plan()) == list(dev.plan())                      # (fresh rngs of one seed: the same draw)
    host, dev = _readers(tmp_path, cmvn, left, right, seed=77)
    a, b = list(host), list(dev)
    assert len(a) == len(b) == 3 and [len(i[0]) for i in a] == [4, 4, 3]          # the partial last window is there
    for want, item in zip(a, b):
        assert is_packed(item[1]) and is_packed(item[2]) and isinstance(item[1], PackedBatch)
        assert item[1].data.dtype == np.float32 and item[1].offsets.dtype == np.int32 and item[1].data.shape[1] == DIN
        assert item[1].shape == want[1].shape and item[2].shape == want[2].shape
        got = feat_ref.expand_item(item)
        assert got[0] == want[0]
        for g, w in zip(got[1:], want[1:]):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        assert np.array_equal(item[3], want[3]) and item[3].dtype == np.int32
        assert np.array_equal(item[1].lengths(), want[3])


def test_prefetch_keeps_packed_items_and_their_order(tmp_path):
    host, dev = _readers(tmp_path, None, 1, 1, seed=3)
    want = [i[0] for i in host]
    assert [i[0] for i in prefetch(dev, threads=2)] == want


def test_rows_shards_as_shard_does(tmp_path):
    cmvn = feat_ref.cmvn_for(np.random.default_rng(6), DIN, DOUT)
    _, dev = _readers(tmp_path, cmvn, 2, 1, seed=1, shuffle=False)
    item = next(iter(dev))
    full = feat_ref.expand_item(item)
    for lo, hi in ((0, 2), (2, 4), (1, 2), (0, 4), (3, 3)):
        part = item[1].rows(lo, hi)
        assert part.shape == (hi - lo,) + item[1].shape[1:] and part.offsets[0] == 0 and part.offsets.dtype == np.int32
        assert part.data.shape[0] == part.offsets[-1]                  # only this shard's frames travel
        if hi > lo:
            X, L = feat_ref.expand(part, (part.mean, part.stddev), part.left, part.right, part.shape[1])
            assert np.array_equal(X, full[1][lo:hi]) and np.array_equal(L, full[3][lo:hi])
    with pytest.raises(ValueError):
        item[1].rows(2, 5)
    # GAN_RNN._shard itself: a batch of batch_size rows passes, any other row count is refused as for arrays (one rank here)
    model = SimpleNamespace(batch_size=4, process_group=None)
    assert GAN_RNN._shard(model, item[1]) is item[1]
    model.batch_size = 3
    with pytest.raises(ValueError, match="batch has 4 rows"):
        GAN_RNN._shard(model, item[1])


def test_shard_of_a_two_rank_batch(monkeypatch):
    from rsrgan_amd import dist as rdist
    rng = np.random.default_rng(2)
    packed = feat_ref.random_packed(rng, [3, 5, 2, 4], DIN, 1, 1)
    want, _ = feat_ref.expand(packed, None, 1, 1, 5)
    monkeypatch.setattr(rdist, "world_size", lambda g=None: 2)
    for r in (0, 1):
        monkeypatch.setattr(rdist, "rank", lambda g=None, r=r: r)
        part = GAN_RNN._shard(SimpleNamespace(batch_size=2, process_group=None), packed)
        got, _ = feat_ref.expand(part, None, 1, 1, 5)
        assert np.array_equal(got, want[2 * r:2 * r + 2])
        assert np.array_equal(GAN_RNN._shard(SimpleNamespace(batch_size=2, process_group=None), want), want[2 * r:2 * r + 2])


def test_a_float64_archive_is_refused(tmp_path):
    rng = np.random.default_rng(4)
    scp = feat_ref.write_arks(tmp_path, "dbl", [5, 6, 7, 8], DIN, DOUT, rng, double_at=2)
    list(PaddedBatchReader(scp[0], scp[1], 4, 1, 1, num_buckets=1, shuffle=False))                # the host path converts
    with pytest.raises(ValueError, match="dbl002.*float32"):
        list(PaddedBatchReader(scp[0], scp[1], 4, 1, 1, num_buckets=1, shuffle=False, device_features=True))
    with pytest.raises(ValueError, match="float32"):
        pack_utterances([np.zeros((3, 2), np.float64)])


def test_call_sites_pass_other_items_through_and_never_fall_back():
    x, lab, ln = np.zeros((2, 3, 4), np.float32), np.zeros((2, 3, 1), np.float32), np.array([3, 2], np.int32)
    out = device_batch(None, x, lab, ln)
    assert out[0] is x and out[1] is lab and out[2] is ln
    packed = feat_ref.random_packed(np.random.default_rng(0), [3, 2], 4)
    model = SimpleNamespace(engine=SimpleNamespace(), batch_size=2, _shard=lambda a: a)
    with pytest.raises(RuntimeError, match="device-side front end"):
        device_batch(model, packed, packed, ln)


def test_flag_defaults_off_and_reaches_the_reader(tmp_path):
    for mod in (G, R):
        assert mod.build_parser().parse_args([]).device_features is False
        assert mod.build_parser().parse_args(["--device_features"]).device_features is True
        assert mod.build_parser().parse_args(["--device_features", "false"]).device_features is False
    rng = np.random.default_rng(9)
    scp = feat_ref.write_arks(tmp_path, "fl", [4, 5], DIN, DOUT, rng)
    FLAGS = G.build_parser().parse_args(["--batch_size", "2", "--left_context", "1", "--right_context", "2", "--device_features"])
    rd = G._reader(FLAGS, scp[0], scp[1], None, False, None)
    item = next(iter(rd))
    assert rd.device_features and is_packed(item[1]) and (item[1].left, item[1].right) == (1, 2) and item[1].shape == (2, 5, DIN * 4)
    FLAGS.device_features = False
    assert isinstance(next(iter(G._reader(FLAGS, scp[0], scp[1], None, False, None)))[1], np.ndarray)
