"""Host side of the live multi-stream decode (no GPU): StreamBank(device_features=False) on the fp64 stand-in model of
tests/stream_ref.py -- every row against a StreamEnhancer of its own (bitwise) and against the whole-utterance arithmetic
(tests/test_stream_host._whole, that file's TOL) --, the NumPy reference of rsrgan_feat_stream (tests/feat_stream_ref.py: the ring, slot
by slot) against the host splice over a schedule that overwrites every slot at least three times at the smallest admissible ring, the
same schedule refused at one frame less, and run_gan_rnn --decode_push against --decode_chunk."""
import os

import numpy as np
import pytest

from rsrgan_amd import run_gan_rnn as R
from rsrgan_amd.io import ArkReader, ArkWriter
from rsrgan_amd.stream import StreamBank, StreamEnhancer
from tests import feat_stream_ref as FR
from tests import stream_ref as SR
from tests.helpers import small_cfg
from tests.test_stream_host import TOL, _cmvn, _g64, _whole

CHUNK, MAX_FRAMES, RAW_DIM = 5, 8, 3


class RowwiseModel(SR.RefStreamModel):
    """RefStreamModel whose forward_stream evaluates every row on its own and frame by frame, as calls of one row and one frame: every
    matrix product has the same shape whichever row it is, whatever the other rows do and however the utterance was cut into calls (a
    bank and an enhancer cut the same pushes differently), so what a frame gets back depends on the row's frames and state alone, bit
    for bit.  That is what lets a row of a bank be compared with a one-row enhancer by equality."""

    def forward_stream(self, inputs, lengths, reset=None):
        x, ln = self._check(inputs, lengths)
        rows = list(range(self.batch_size)) if reset is True else [int(r) for r in (reset or [])]
        for r in rows:
            for c, m in self.state:
                c[r] = 0.0
                m[r] = 0.0
        self.calls.append((x.shape[1], ln.copy(), tuple(rows)))
        y = np.zeros((self.batch_size, x.shape[1], self.cfg.output_dim))
        for r in range(self.batch_size):
            n = int(ln[r])
            if n == 0:
                continue
            new = [(c[r:r + 1].copy(), m[r:r + 1].copy()) for c, m in self.state]
            for t in range(n):
                yt, new = SR.generator_fwd_state(self.cfg, self.g, x[r:r + 1, t:t + 1], np.array([1], np.int32), new)
                y[r, t] = yt[0, 0]
            for (c, m), (cn, mn) in zip(self.state, new):
                c[r], m[r] = cn[0], mn[0]
        return y


def _model(left, right, batch):
    cfg = small_cfg("lstm", input_dim=RAW_DIM * (left + 1 + right), output_dim=4)
    return RowwiseModel(cfg, _g64(cfg, 11), batch, MAX_FRAMES)


def _lengths(left, right):
    return [T for T in (1, 2, left + right, left + right + 1, 23, 40) if T > 0]


@pytest.mark.parametrize("with_cmvn", [True, False], ids=["cmvn", "raw"])
@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("ctx", [(0, 0), (2, 3), (5, 5)])
def test_every_row_equals_an_enhancer_of_its_own(ctx, streams, with_cmvn):
    left, right = ctx
    rng = np.random.default_rng(1000 * left + 10 * right + streams)
    cmvn = _cmvn(RAW_DIM, 4, rng) if with_cmvn else None
    model = _model(left, right, streams + 1)                     # one row beyond `streams`: it must rest in every call
    bank = StreamBank(model, cmvn, left, right, chunk=CHUNK, streams=streams)
    assert bank.ring_frames == left + CHUNK + right and bank.dim == RAW_DIM
    lens = _lengths(left, right)
    # row r goes through the utterance lengths rotated by r, so the rows are out of phase; its frames and push sizes are its own
    todo = {r: [rng.standard_normal((T, RAW_DIM)) * 2 + 1 for T in lens[r:] + lens[:r]] for r in range(streams)}
    cur = {r: dict(x=todo[r].pop(0), pos=0, pushes=[], outs=[]) for r in range(streams)}
    finished = {r: [] for r in range(streams)}                   # (frames, pushes, bank output) per utterance
    while cur:
        sizes = {r: int(rng.integers(0, 12)) for r in cur}
        n0 = len(model.calls)
        got = bank.push({r: c["x"][c["pos"]:c["pos"] + sizes[r]] for r, c in cur.items()})
        assert set(got) == set(cur)
        for r, c in cur.items():
            c["pushes"].append(sizes[r]); c["outs"].append(got[r]); c["pos"] += sizes[r]
        for _, ln, _ in model.calls[n0:]:                        # rows without work rest
            assert all(ln[r] == 0 for r in range(streams + 1) if r not in cur)
        ended = [r for r, c in cur.items() if c["pos"] >= c["x"].shape[0]]
        for r in ended:                                          # exactly the last right_context frames are held back
            assert sum(o.shape[0] for o in cur[r]["outs"]) == max(0, cur[r]["x"].shape[0] - right)
        if ended:
            n0 = len(model.calls)
            tail = bank.flush(ended)                             # a subset: the other rows' utterances go on
            assert set(tail) == set(ended)
            for _, ln, _ in model.calls[n0:]:
                assert all(ln[r] == 0 for r in range(streams + 1) if r not in ended)
        for r in ended:
            c = cur.pop(r)
            finished[r].append((c["x"], c["pushes"], np.concatenate(c["outs"] + [tail[r]], 0)))
            if todo[r]:
                cur[r] = dict(x=todo[r].pop(0), pos=0, pushes=[], outs=[])
    assert model.calls and all(T <= CHUNK for T, _, _ in model.calls)           # never more than `chunk` frames per call
    assert all((ln[streams:] == 0).all() for _, ln, _ in model.calls)
    if streams > 1:
        assert any((ln > 0).sum() > 1 for _, ln, _ in model.calls)             # rows did advance in the same call
    for r in range(streams):
        assert len(finished[r]) == len(lens)
        enh = StreamEnhancer(_model(left, right, 1), cmvn, left, right, chunk=CHUNK)
        for frames, pushes, got in finished[r]:
            outs, pos = [], 0
            for n in pushes:
                outs.append(enh.push(frames[pos:pos + n]))
                pos += n
            want = np.concatenate(outs + [enh.flush()], 0)
            assert got.shape == want.shape == (frames.shape[0], 4) and got.dtype == want.dtype
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), (r, frames.shape[0])
            whole = _whole(model, frames, cmvn, left, right)
            assert np.abs(got - whole).max() <= TOL, (r, frames.shape[0], np.abs(got - whole).max())


def test_reset_and_flush_of_a_subset_leave_the_other_rows_alone():
    left, right = 2, 3
    rng = np.random.default_rng(5)
    cmvn = _cmvn(RAW_DIM, 4, rng)
    model = _model(left, right, 3)
    bank = StreamBank(model, cmvn, left, right, chunk=CHUNK)
    assert bank.streams == 3 and bank.chunk == CHUNK
    a, b, c, d = (rng.standard_normal((T, RAW_DIM)) for T in (31, 17, 12, 9))
    outs = [bank.push({0: a[:13], 1: b[:9], 2: c[:7]})[0]]
    bank.reset([1])                                              # row 1's utterance is abandoned
    assert bank.flush([2])[2].shape[0] == right                  # row 2's ends after 7 frames: the held-back ones come out
    second = bank.push({0: a[13:20], 1: d[:4]})                  # row 1 begins another
    outs.append(second[0])
    tail = bank.flush()                                          # every busy row: 0 and 1
    assert set(tail) == {0, 1}
    got_d = np.concatenate([second[1], tail[1]], 0)
    outs.append(tail[0])
    got_a = np.concatenate(outs, 0)
    assert np.abs(got_a - _whole(model, a[:20], cmvn, left, right)).max() <= TOL
    assert np.abs(got_d - _whole(model, d[:4], cmvn, left, right)).max() <= TOL
    assert bank.flush() == {} and bank.push({1: np.zeros((0, RAW_DIM))})[1].shape == (0, 4)
    got_c = np.concatenate([bank.push({2: c})[2], bank.flush([2])[2]], 0)       # after its flush, row 2 starts fresh
    assert np.abs(got_c - _whole(model, c, cmvn, left, right)).max() <= TOL


def test_rejections_come_before_any_work():
    model = _model(1, 1, 2)
    for kw in (dict(chunk=MAX_FRAMES + 1), dict(streams=3), dict(streams=0), dict(left_context=-1), dict(device_features=True)):
        with pytest.raises(ValueError):
            StreamBank(model, None, **dict(dict(left_context=1, right_context=1), **kw))
    with pytest.raises(ValueError, match="op_feat_stream"):
        StreamEnhancer(model, None, 1, 1, device_features=True)
    bank = StreamBank(model, None, 1, 1, streams=1)
    assert bank.chunk == MAX_FRAMES
    good = np.zeros((4, RAW_DIM))
    for bad in ({1: good}, {-1: good}, {0: np.zeros(RAW_DIM)}, {0: np.zeros((4, RAW_DIM + 1))}, {0: good, 2: good}):
        with pytest.raises(ValueError):
            bank.push(bad)
    with pytest.raises(ValueError):
        bank.flush([1])
    with pytest.raises(ValueError):
        bank.reset([7])
    assert model.calls == []


# ---- the reference of rsrgan_feat_stream on the bank's own tables, at the smallest ring ----------------------------------------

def _ring_schedule(bank, rng, streams, frames):
    """pushes of [0, 12) frames per row until every row's utterance is in, one flush, then a second utterance on the used ring"""
    for utt in range(2):
        pos = {r: 0 for r in range(streams)}
        while any(pos[r] < frames[utt][r].shape[0] for r in pos):
            sizes = {r: int(rng.integers(0, 12)) for r in pos}
            bank.push({r: frames[utt][r][pos[r]:pos[r] + sizes[r]] for r in pos})
            for r in pos:
                pos[r] += sizes[r]
        bank.flush()


@pytest.mark.parametrize("with_cmvn", [True, False], ids=["cmvn", "raw"])
@pytest.mark.parametrize("ctx", [(0, 0), (2, 3)])
def test_ring_reference_equals_the_host_splice_at_the_smallest_ring(ctx, with_cmvn):
    left, right = ctx
    streams, batch = 3, 4
    H = left + CHUNK + right
    seed = 77 + left
    rng = np.random.default_rng(seed)
    cmvn = _cmvn(RAW_DIM, 4, rng) if with_cmvn else None
    stats = (None, None) if cmvn is None else (cmvn["mean_inputs"], cmvn["stddev_inputs"])
    # (float32 values, so that the float32 frames the device path would ship are the frames the host path normalises)
    frames = [[rng.standard_normal((T, RAW_DIM)).astype(np.float32) * 2 + 1 for T in Ts] for Ts in ((4 * H + 3, 5 * H, 4 * H + 1), (7, 2 * H, 1))]

    def run(ring_frames):
        bank = StreamBank(_model(left, right, batch), cmvn, left, right, chunk=CHUNK, streams=streams)
        assert bank.ring_frames == H
        bank.ring_frames = ring_frames
        ring = np.full((batch, ring_frames, RAW_DIM), np.nan, np.float32)
        writes = np.zeros((batch, ring_frames), np.int64)
        host_featurize, rounds = bank._featurize_host, []

        def featurize(table, fresh, T):
            x, ln = host_featurize(table, fresh, T)
            for r in range(batch):
                for i in range(table[r, 2]):
                    writes[r, FR.mod(table[r, 1] + i, ring_frames)] += 1
            want, want_ln = FR.feat_stream(fresh.astype(np.float32) if fresh.shape[0] else None, table, ring, T, left, right, *stats)
            assert np.array_equal(want.view(np.int32), x.view(np.int32)) and np.array_equal(want_ln, ln)
            rounds.append(table.copy())
            return x, ln
        bank._featurize_host = featurize
        _ring_schedule(bank, np.random.default_rng(seed + 1), streams, frames)
        return writes, rounds

    writes, rounds = run(H)
    assert writes[:streams].min() >= 3, writes                   # every slot of every live row was overwritten at least three times
    assert not writes[streams:].any()
    # the window reaches H: a row holding `right` frames took in `chunk` more
    assert max(int(t[r, 5]) - (int(t[r, 3]) - left) + 1 for t in rounds for r in range(streams) if t[r, 2] or t[r, 4]) == H
    with pytest.raises(AssertionError, match="do not fit a ring of %d" % (H - 1)):
        run(H - 1)                                               # one frame less: the same schedule breaks the invariant and is refused


# ---- run_gan_rnn --decode_push ------------------------------------------------------------------------------------------------

def test_decode_push_equals_decode_chunk(tmp_path):
    rng = np.random.default_rng(9)
    din, dout, left, right = 3, 4, 2, 1
    w = ArkWriter(str(tmp_path / "te.scp"))
    lens = [5, 37, 1, 16, 90, 17, 33]
    for i, T in enumerate(lens):
        w.write_next_utt(str(tmp_path / "te.ark"), "utt%02d" % i, rng.standard_normal((T, din)) * 2 + 1)
    w.close()
    np.savez(tmp_path / "train_cmvn.npz", **_cmvn(din, dout, rng))
    cfg = small_cfg("lstm", input_dim=din * (left + 1 + right), output_dim=dout)
    g = _g64(cfg, 13)
    base = ["--decode", "--data_dir", str(tmp_path), "--test_inputs_scp", str(tmp_path / "te.scp"), "--input_dim", str(din),
            "--output_dim", str(dout), "--left_context", str(left), "--right_context", str(right), "--decode_chunk", "16",
            "--decode_streams", "4"]
    scps, models = [], []
    for tag, extra in (("chunk", []), ("push", ["--decode_push", "7"])):
        F, _ = R.build_parser().parse_known_args(base + ["--save_dir", str(tmp_path / tag)] + extra)
        assert F.decode_push == (7 if extra else 0)
        m = SR.RefStreamModel(cfg, g, 4, 16, save_dir=F.save_dir)
        scps.append(R.decode(F, model_factory=lambda: m, log=lambda s: None))
        models.append(m)
    r0, r1 = ArkReader(), ArkReader()
    r0(scps[0]); r1(scps[1])
    assert r1.utt_ids == r0.utt_ids == ["utt%02d" % i for i in range(len(lens))]
    for i, T in enumerate(lens):
        a, b = r0.read_utt_data_from_index(i), r1.read_utt_data_from_index(i)
        assert a.shape == b.shape == (T, dout)
        assert np.abs(a.astype(np.float64) - b).max() <= 1e-6 * max(1.0, np.abs(a).max())
    assert models[1].calls and all(T <= 16 for T, _, _ in models[1].calls)
    assert any((ln > 0).sum() > 1 for _, ln, _ in models[1].calls)             # the pushes of several rows shared calls
    F, _ = R.build_parser().parse_known_args([a for a in base if a not in ("--decode_chunk", "16")] + ["--save_dir", str(tmp_path / "x"),
                                                                                                 "--decode_push", "7"])
    with pytest.raises(SystemExit):
        R.decode(F, model_factory=lambda: SR.RefStreamModel(cfg, g, 4, 16, save_dir=F.save_dir), log=lambda s: None)
    from rsrgan_amd import run_rnn
    assert run_rnn.build_parser().parse_args(["--decode_push", "3"]).decode_push == 3
