"""The host side of the frame-level device-side front end: FrameBatchReader(device_features=True) keeps the shuffle queue as bookkeeping
and yields io.FrameDraw items; tests/feat_frames_ref.HostPool replays them with apply_cmvn and indexing alone (a NumPy stand-in for the
pool the engine keeps on the device).  The replayed batches must be the default reader's with the same seed, bit for bit (np.array_equal
on the int32 views), and the row allocator must keep its promises over a whole pass.  No device anywhere."""
import numpy as np
import pytest

from rsrgan_amd.io import FrameBatchReader, FrameDraw, RowAllocator
from tests import feat_frames_ref as R
from tests.feat_ref import cmvn_for, write_arks


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _pair(scp, batch, left, right, cmvn, shuffle, seed, num_threads=2, **kw):
    mk = lambda dev, **k: FrameBatchReader(scp[0], scp[1], batch, left, right, cmvn=cmvn, num_threads=num_threads, shuffle=shuffle, seed=seed,
                                           device_features=dev, **k)
    return mk(False), mk(True, **kw)


def _assert_same_pass(host, dev, limit=None):
    """one pass of both readers; returns (batches, the HostPool that replayed the device reader's items)"""
    pool = R.HostPool(dev.reader_id)
    want = list(host)
    it, n = iter(dev), 0
    for k in range(len(want) + 2 if limit is None else limit):          # bounded: a stalled iterator fails instead of hanging the suite
        item = next(it, None)
        if item is None:
            break
        assert isinstance(item, FrameDraw) and item.serial == k and item.picks.dtype == np.int32 and item.picks.shape == (dev.batch_size, 3)
        x, y = pool.feed(item)
        assert n < len(want), "the device reader yields more batches than the default reader"
        assert x.dtype == np.float32 and x.shape == want[n][0].shape and y.shape == want[n][1].shape
        assert np.array_equal(_bits(x), _bits(want[n][0])), "inputs of batch %d" % n
        assert np.array_equal(_bits(y), _bits(want[n][1])), "labels of batch %d" % n
        n += 1
    assert n == len(want) and n > 0
    return n, pool


@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffled", "in-order"])
@pytest.mark.parametrize("with_cmvn", [True, False], ids=["cmvn", "raw"])
def test_replayed_batches_equal_the_default_readers(tmp_path, with_cmvn, shuffle):
    rng = np.random.default_rng(0)
    xs, ls, total = R.frame_data(tmp_path, 25, rng, random_values=with_cmvn)
    cmvn = cmvn_for(rng, 3, 2) if with_cmvn else None
    host, dev = _pair((xs, ls), 32, 1, 1, cmvn, shuffle, seed=3)
    assert dev.capacity == host.capacity == 1000 + 3 * 32 and dev.num_batches() == host.num_batches() == total // 32
    assert dev.num_frames() == host.num_frames() == total
    n, pool = _assert_same_pass(host, dev)
    assert n == total // 32
    # a second pass goes on with the same generator state on both sides, with the next serial numbers and in the same pool: what the
    # first pass left in the queue is dropped, its rows are handed out again
    want = list(host)
    pool.new_pass()
    got = [pool.feed(item) for item in dev]
    assert len(got) == len(want) == n and pool.ledger.next_serial == 2 * n and pool.reuses >= 1
    assert all(np.array_equal(_bits(g[0]), _bits(w[0])) and np.array_equal(_bits(g[1]), _bits(w[1])) for g, w in zip(got, want))


def test_context_5_5_with_utterances_of_one_and_three_frames(tmp_path):
    rng = np.random.default_rng(5)
    lengths = [40, 1, 55, 3, 70, 48, 1, 66, 3, 52]
    xs, ls, total = R.frame_data(tmp_path, None, rng, din=4, dout=2, lengths=lengths, random_values=True)
    cmvn = cmvn_for(rng, 4, 2)
    for shuffle in (True, False):
        host, dev = _pair((xs, ls), 16, 5, 5, cmvn, shuffle, seed=11, num_threads=1)
        n, pool = _assert_same_pass(host, dev)
        assert n == total // 16
        sizes = [r for _, ups, _ in pool.history for _, r in ups]
        assert 1 in sizes and 3 in sizes                        # utterances shorter than either context were drawn from


def test_an_utterance_longer_than_the_queue_is_admitted(tmp_path):
    """tests/test_frame_level_loop.py's case: lengths [300, 1400, 200] at batch 32, capacity 1064 < 1400"""
    rng = np.random.default_rng(1)
    lens = [300, 1400, 200]
    xs, ls, total = R.frame_data(tmp_path, None, rng, din=2, dout=1, lengths=lens)
    for shuffle in (False, True):
        host, dev = _pair((xs, ls), 32, 0, 0, None, shuffle, seed=1, num_threads=1)
        assert dev.capacity == 1000 + 2 * 32 < 1400
        n, pool = _assert_same_pass(host, dev, limit=sum(lens) // 32 + 2)
        assert n == sum(lens) // 32
        assert pool.ledger.pool_rows >= 1400 and pool.growths >= 1            # the over-long utterance made the pool grow


@pytest.mark.parametrize("shuffle,utts", [(False, 25), (True, 150)], ids=["in-order", "shuffled"])
def test_allocator_invariants_over_a_whole_pass(tmp_path, shuffle, utts):
    """HostPool.feed asserts per item: every slot starts on a multiple of 4, live slots never overlap (a slot is live until its
    utterance's last frame was drawn, so it is reused only after that), every pick names a live utterance.  Here: pool_rows is monotone,
    and a deliberately small initial pool makes the pool grow AND reuse freed rows.  (A shuffled queue of 1000 frames lets go of an
    utterance's last frame late: that case takes more data than the queue holds several times over.)"""
    rng = np.random.default_rng(0)
    xs, ls, total = R.frame_data(tmp_path, utts, rng)
    host, dev = _pair((xs, ls), 32, 1, 1, None, shuffle, seed=3, num_threads=0, initial_pool_rows=64)
    assert dev.allocator.pool_rows == 64 and host.capacity == 1032
    n, pool = _assert_same_pass(host, dev)
    rows = [h[0] for h in pool.history]
    assert all(a <= b for a, b in zip(rows, rows[1:])) and rows[0] > 64 and all(r % 4 == 0 for r in rows)
    assert pool.growths + (rows[0] > 64) >= 1 and dev.allocator.growths >= 1
    assert pool.reuses >= 1, "no freed slot was handed out again"
    assert sum(len(h[2]) for h in pool.history) >= 1
    firsts = [f for _, ups, _ in pool.history for f, _ in ups]
    assert len(firsts) == utts and all(f % 4 == 0 for f in firsts)


def test_row_allocator_first_fit_coalescing_and_growth():
    a = RowAllocator(30)
    assert a.pool_rows == 32
    s = [a.alloc(n) for n in (5, 8, 3, 9)]                      # 8 + 8 + 4 + 12 rows
    assert s == [0, 8, 16, 20] and a.blocks == []
    a.free(8); a.free(16)
    assert a.blocks == [[8, 12]]                                # neighbours coalesce
    assert a.alloc(4) == 8 and a.alloc(6) == 12                 # first fit
    assert a.alloc(2) == 32 and a.pool_rows == 64 and a.growths == 1            # nothing fits: doubled, rows handed out keep their numbers
    a.free(0); a.free(20)
    assert a.blocks == [[0, 8], [20, 12], [36, 28]]
    assert a.alloc(40) == 36 and a.pool_rows == 128             # the free block that ended at the old capacity joins the new rows
    assert a.blocks == [[0, 8], [20, 12], [76, 52]]
    a.free(36)
    assert a.blocks == [[0, 8], [20, 12], [36, 92]]
    assert a.alloc(90) == 36 and a.alloc(9) == 20
    assert sorted(a.live) == [8, 12, 20, 32, 36]


def test_the_flag_parses_as_in_run_gan_rnn():
    from rsrgan_amd import run_gan_dnn, run_gan_dnn_iter
    for mod in (run_gan_dnn, run_gan_dnn_iter):
        assert mod.build_parser().parse_args([]).device_features is False
        assert mod.build_parser().parse_args(["--device_features"]).device_features is True
        assert mod.build_parser().parse_args(["--device_features", "false"]).device_features is False
    FLAGS = run_gan_dnn.build_parser().parse_args(["--batch_size", "8", "--num_threads", "1", "--device_features"])
    assert FLAGS.left_context == FLAGS.right_context == 5


def test_reader_from_the_flag_and_device_frames_without_an_engine(tmp_path):
    from types import SimpleNamespace
    from rsrgan_amd import run_gan_dnn as G
    from rsrgan_amd.train import device_frames
    rng = np.random.default_rng(2)
    xs, ls, _ = R.frame_data(tmp_path, 4, rng)
    FLAGS = G.build_parser().parse_args(["--batch_size", "8", "--left_context", "1", "--right_context", "2", "--num_threads", "1", "--device_features"])
    rd = G._reader(FLAGS, xs, ls, None, True, 7)
    item = next(iter(rd))
    assert rd.device_features and isinstance(item, FrameDraw) and (item.left, item.right) == (1, 2) and item.shape == (8, 3 * 4)
    FLAGS.device_features = False
    host = G._reader(FLAGS, xs, ls, None, True, 7)
    assert not host.device_features
    batch = next(iter(host))
    model = SimpleNamespace(disc_updates=1, gen_updates=1)                       # no engine: host batches pass through, frame draws raise
    assert next(device_frames(model, [batch])) is batch
    with pytest.raises(RuntimeError, match="featurize_frames"):
        next(device_frames(model, [item]))


def test_an_out_of_order_item_raises(tmp_path):
    rng = np.random.default_rng(4)
    xs, ls, _ = R.frame_data(tmp_path, 25, rng)
    _, dev = _pair((xs, ls), 32, 1, 1, None, True, seed=3)
    it = iter(dev)
    first, second = next(it), next(it)
    pool = R.HostPool(dev.reader_id)
    with pytest.raises(ValueError, match="out of order"):
        pool.feed(second)
    pool.feed(first)
    with pytest.raises(ValueError, match="out of order"):
        pool.feed(first)                                        # consumed once
    pool.feed(second)
    _, other = _pair((xs, ls), 32, 1, 1, None, True, seed=3)
    with pytest.raises(ValueError, match="reader"):
        pool.feed(next(iter(other)))                            # another reader's item: another pool


def test_a_float64_matrix_is_refused_by_name(tmp_path):
    rng = np.random.default_rng(6)
    scp = write_arks(tmp_path, "dbl", [5, 4, 6], 3, 2, rng, double_at=1)
    rd = FrameBatchReader(scp[0], scp[1], 4, 1, 1, shuffle=False, device_features=True)
    with pytest.raises(ValueError, match="dbl001"):
        list(rd)
    assert len(list(FrameBatchReader(scp[0], scp[1], 4, 1, 1, shuffle=False))) == 3           # the default reader takes it
