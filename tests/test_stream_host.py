"""Host side of the stateful generator forward (no GPU): the fp64 reference with carried state (tests/stream_ref.py) pinned to the
oracle, StreamEnhancer / decode_streams / run_gan_rnn.decode against the whole-utterance result on a stand-in model built on that
reference, and the new C-ABI symbols in the header, the binding and the cross-compiled library."""
import os
import re

import numpy as np
import pytest

from oracle import rsrgan_oracle as O
from rsrgan_amd import run_gan_rnn as R
from rsrgan_amd.io import ArkReader, ArkWriter, splice_feats
from tests import stream_ref as SR
from tests.helpers import rand_params, small_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
G_TYPES = ["lstm", "res_lstm_l", "res_lstm_base"]
NEW_SYMBOLS = ["rsrgan_g_state_floats", "rsrgan_g_state_reset", "rsrgan_g_state_get", "rsrgan_g_state_set", "rsrgan_forward_g_stream"]


def _g64(cfg, seed):
    return {k: np.asarray(v, np.float64) for k, v in rand_params(cfg, seed)[0].items()}


def _ragged(cfg, B, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, cfg.input_dim))
    ln = rng.integers(2, T + 1, size=B).astype(np.int32)
    ln[0], ln[1], ln[2] = T, 1, 7                      # a full row, a row of length 1, a row that ends inside the second chunk
    return x, ln


# ---- the reference with state is the oracle -------------------------------------------------------------------------------------

@pytest.mark.parametrize("g_type", G_TYPES)
@pytest.mark.parametrize("proj", [True, False])
def test_zero_state_equals_oracle(g_type, proj):
    cfg = small_cfg(g_type)
    if not proj:
        if g_type == "res_lstm_l":
            cfg.g_cells = cfg.input_dim                # the residual sum needs equal widths
        cfg.g_proj = 0
    g = _g64(cfg, 3)
    x, ln = _ragged(cfg, 6, 13, 4)
    want = O.generator_fwd(cfg, g, x, ln)[0]
    got, _ = SR.generator_fwd_state(cfg, g, x, ln, SR.zero_state(cfg, 6))
    assert np.abs(got - want).max() <= TOL


@pytest.mark.parametrize("g_type", G_TYPES)
@pytest.mark.parametrize("cuts", [(5, 1, 4, 3), (1,) * 13, (13,), (6, 7)])
def test_chunked_with_carry_equals_whole(g_type, cuts):
    cfg = small_cfg(g_type)
    g = _g64(cfg, 5)
    B, T = 6, 13
    x, ln = _ragged(cfg, B, T, 6)
    want = O.generator_fwd(cfg, g, x, ln)[0]
    state, pos, outs = SR.zero_state(cfg, B), 0, []
    for n in cuts:
        lc = np.clip(ln - pos, 0, n).astype(np.int32)   # rows that end inside the chunk, rows already ended -> 0
        y, state = SR.generator_fwd_state(cfg, g, x[:, pos:pos + n], lc, state)
        outs.append(y)
        pos += n
    assert pos == T
    assert np.abs(np.concatenate(outs, 1) - want).max() <= TOL
    # the state after the last chunk is the state of a whole call (every row at its own length)
    _, whole = SR.generator_fwd_state(cfg, g, x, ln, SR.zero_state(cfg, B))
    for (c0, m0), (c1, m1) in zip(state, whole):
        assert np.abs(c0 - c1).max() <= TOL and np.abs(m0 - m1).max() <= TOL


def test_rows_with_length_zero_keep_their_state():
    cfg = small_cfg("lstm")
    g = _g64(cfg, 7)
    x, ln = _ragged(cfg, 4, 9, 8)
    _, st = SR.generator_fwd_state(cfg, g, x, ln, SR.zero_state(cfg, 4))
    rest = np.array([3, 0, 0, 2], np.int32)
    _, st2 = SR.generator_fwd_state(cfg, g, x[:, :3], rest, st)
    for (c0, m0), (c1, m1) in zip(st, st2):
        assert np.array_equal(c0[1:3], c1[1:3]) and np.array_equal(m0[1:3], m1[1:3])
        assert not np.array_equal(c0[0], c1[0])


# ---- StreamEnhancer -------------------------------------------------------------------------------------------------------------

def _cmvn(din, dout, rng):
    return dict(mean_inputs=rng.standard_normal(din), stddev_inputs=rng.uniform(0.5, 2.0, din),
                mean_labels=rng.standard_normal(dout), stddev_labels=rng.uniform(0.5, 2.0, dout))


def _whole(model, frames, cmvn, left, right):
    """run_gan_rnn.decode's arithmetic for one utterance on a batch-1 view of the model"""
    x = np.asarray(frames, np.float64)
    if cmvn is not None:
        x = (x - cmvn["mean_inputs"]) / cmvn["stddev_inputs"]
    x = splice_feats(x, left, right).astype(np.float32)
    y = O.generator_fwd(model.cfg, model.g, x[None].astype(np.float64), np.array([x.shape[0]], np.int32))[0][0]
    return y * cmvn["stddev_labels"] + cmvn["mean_labels"] if cmvn is not None else y


def _stream_model(left, right, batch=1, max_frames=8, g_type="lstm", tag_column=None, raw_dim=3):
    cfg = small_cfg(g_type, input_dim=raw_dim * (left + 1 + right), output_dim=4)
    if g_type == "res_lstm_l":
        cfg.g_proj = cfg.input_dim
    return SR.RefStreamModel(cfg, _g64(cfg, 11), batch, max_frames, tag_column=tag_column), raw_dim


@pytest.mark.parametrize("ctx", [(0, 0), (2, 3), (5, 5)])
@pytest.mark.parametrize("pushes", ["1", "7", "random"])
@pytest.mark.parametrize("with_cmvn", [True, False])
def test_stream_enhancer_equals_whole_utterance(ctx, pushes, with_cmvn):
    from rsrgan_amd.stream import StreamEnhancer
    left, right = ctx
    model, din = _stream_model(left, right, batch=2, max_frames=8)
    rng = np.random.default_rng(100 * left + right)
    cmvn = _cmvn(din, 4, rng) if with_cmvn else None
    enh = StreamEnhancer(model, cmvn, left, right, chunk=5)
    # utterances of 1 .. 40 frames, some shorter than left + right + 1, back to back through one enhancer
    for T in (1, 2, left + right, left + right + 1, 23, 40):
        if T == 0:
            continue
        frames = rng.standard_normal((T, din)) * 2 + 1
        outs, pos = [], 0
        while pos < T:
            n = 1 if pushes == "1" else 7 if pushes == "7" else int(rng.integers(0, 12))
            outs.append(enh.push(frames[pos:pos + n]))
            pos += n
        held = sum(o.shape[0] for o in outs)
        assert held == max(0, T - right)                # exactly the last right_context frames are held back
        outs.append(enh.flush())
        got = np.concatenate(outs, 0)
        want = _whole(model, frames, cmvn, left, right)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= TOL, (T, np.abs(got - want).max())
    assert all(T <= 5 for T, _, _ in model.calls)       # never more than `chunk` frames per call
    assert all((ln[1:] == 0).all() for _, ln, _ in model.calls)      # one live stream: row 0 only


def test_stream_enhancer_reset_and_bounds():
    from rsrgan_amd.stream import StreamEnhancer
    model, din = _stream_model(1, 1, max_frames=8)
    with pytest.raises(ValueError):
        StreamEnhancer(model, None, 1, 1, chunk=9)       # beyond the handle's max_frames
    enh = StreamEnhancer(model, None, 1, 1)
    assert enh.chunk == 8
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal((11, din)), rng.standard_normal((6, din))
    enh.push(a)                                          # abandoned mid-utterance
    enh.reset()
    got = np.concatenate([enh.push(b[:2]), enh.push(b[2:]), enh.flush()], 0)
    assert np.abs(got - _whole(model, b, None, 1, 1)).max() <= TOL
    assert enh.push(np.zeros((0, din))).shape == (0, 4) and enh.flush().shape == (0, 4)


# ---- decode_streams -------------------------------------------------------------------------------------------------------------

def _tagged_utterances(rng, n, din, lo, hi):
    """utterance i carries the tag i + 1 in column 0 of every frame (RefStreamModel.tag_column)"""
    utts = []
    for i in range(n):
        x = rng.standard_normal((int(rng.integers(lo, hi + 1)), din)).astype(np.float32)
        x[:, 0] = i + 1
        utts.append(x)
    return utts


@pytest.mark.parametrize("streams", [1, 3, 8])
@pytest.mark.parametrize("g_type", ["lstm", "res_lstm_l"])
def test_decode_streams_equals_whole_in_order(streams, g_type):
    from rsrgan_amd.stream import decode_streams
    chunk = 6
    model, din = _stream_model(0, 0, batch=8, max_frames=chunk, g_type=g_type, tag_column=0, raw_dim=5)
    rng = np.random.default_rng(streams)
    utts = _tagged_utterances(rng, 20, din, 1, 40)       # some shorter than a chunk, some many chunks
    utts[3], utts[4] = utts[3][:2], utts[4][:chunk]
    consumed = []

    def source():
        for i, u in enumerate(utts):
            consumed.append(i)
            yield u
    outs = list(decode_streams(model, source(), chunk, streams))          # (an iterator is enough: utterances are taken one by one)
    assert len(outs) == len(utts) == len(consumed)
    for i, (u, y) in enumerate(zip(utts, outs)):         # in input order, each equal to its whole-utterance result
        want = O.generator_fwd(model.cfg, model.g, u[None].astype(np.float64), np.array([len(u)], np.int32))[0][0]
        assert y.shape == want.shape, i
        assert np.abs(y - want).max() <= TOL, (i, np.abs(y - want).max())
    assert all((ln[streams:] == 0).all() for _, ln, _ in model.calls)
    if streams > 1:
        assert any((ln > 0).sum() > 1 for _, ln, _ in model.calls)      # rows did run side by side
    with pytest.raises(ValueError):
        list(decode_streams(model, utts, chunk + 1, streams))
    with pytest.raises(ValueError):
        list(decode_streams(model, utts, chunk, 9))


# ---- run_gan_rnn.decode ---------------------------------------------------------------------------------------------------------

def _decode_parent_loop(FLAGS, model, cmvn, out_dir):
    """the decode loop as it was before the streaming flags existed, restated: what the default flags must still write"""
    os.makedirs(out_dir, exist_ok=True)
    scp, ark = os.path.join(out_dir, "feats.scp"), os.path.join(out_dir, "feats.ark")
    writer, reader = ArkWriter(scp), ArkReader()
    reader(FLAGS.test_inputs_scp)
    for i, utt in enumerate(reader.utt_ids):
        x = reader.read_utt_data_from_index(i).astype(np.float64)
        x = (x - cmvn["mean_inputs"]) / cmvn["stddev_inputs"]
        x = splice_feats(x, FLAGS.left_context, FLAGS.right_context).astype(np.float32)[None]
        activations = np.asarray(model.forward(x, np.array([x.shape[1]], np.int32)))
        writer.write_next_utt(ark, utt, np.vstack(activations * cmvn["stddev_labels"] + cmvn["mean_labels"]))
    writer.close()
    return scp, ark


def test_decode_default_is_unchanged_and_chunked_matches(tmp_path):
    rng = np.random.default_rng(9)
    din, dout, left, right = 3, 4, 2, 1
    w = ArkWriter(str(tmp_path / "te.scp"))
    lens = [5, 37, 1, 16, 90, 17, 33]                    # 90 > any max_frames the chunked handle has
    for i, T in enumerate(lens):
        w.write_next_utt(str(tmp_path / "te.ark"), "utt%02d" % i, rng.standard_normal((T, din)) * 2 + 1)
    w.close()
    cm = _cmvn(din, dout, rng)
    np.savez(tmp_path / "train_cmvn.npz", **cm)
    cmvn = np.load(tmp_path / "train_cmvn.npz")
    cfg = small_cfg("lstm", input_dim=din * (left + 1 + right), output_dim=dout)
    g = _g64(cfg, 13)
    base = ["--decode", "--data_dir", str(tmp_path), "--test_inputs_scp", str(tmp_path / "te.scp"), "--input_dim", str(din),
            "--output_dim", str(dout), "--left_context", str(left), "--right_context", str(right)]
    # the parent's loop
    F0, _ = R.build_parser().parse_known_args(base + ["--save_dir", str(tmp_path / "exp0")])
    _, ark0 = _decode_parent_loop(F0, SR.RefStreamModel(cfg, g, 1, 3000), cmvn, str(tmp_path / "exp0" / "test"))
    # default flags: the same bytes, through forward() only
    F1, _ = R.build_parser().parse_known_args(base + ["--save_dir", str(tmp_path / "exp1")])
    assert (F1.decode_chunk, F1.decode_streams) == (0, 1)
    m1 = SR.RefStreamModel(cfg, g, 1, 3000, save_dir=F1.save_dir)
    scp1 = R.decode(F1, model_factory=lambda: m1, log=lambda s: None)
    ark1 = os.path.join(os.path.dirname(scp1), "feats.ark")
    assert open(ark1, "rb").read() == open(ark0, "rb").read()
    strip = lambda p: [re.sub(r" .*/(exp\d)/", " ", l) for l in open(p)]
    assert strip(scp1) == strip(os.path.join(os.path.dirname(ark0), "feats.scp"))
    assert m1.calls == []
    # chunked, four streams: the same matrices in the same order
    F2, _ = R.build_parser().parse_known_args(base + ["--save_dir", str(tmp_path / "exp2"), "--decode_chunk", "16", "--decode_streams", "4"])
    m2 = SR.RefStreamModel(cfg, g, 4, 16, save_dir=F2.save_dir)
    scp2 = R.decode(F2, model_factory=lambda: m2, log=lambda s: None)
    r0, r2 = ArkReader(), ArkReader()
    r0(os.path.join(os.path.dirname(ark0), "feats.scp")); r2(scp2)
    assert r2.utt_ids == r0.utt_ids == ["utt%02d" % i for i in range(len(lens))]
    for i, T in enumerate(lens):
        a, b = r0.read_utt_data_from_index(i), r2.read_utt_data_from_index(i)
        assert a.shape == b.shape == (T, dout)
        assert np.abs(a.astype(np.float64) - b).max() <= 1e-6 * max(1.0, np.abs(a).max())
    assert m2.calls and all(T <= 16 for T, _, _ in m2.calls)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

def test_new_symbols_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsrgan.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rsrgan_[a-z_0-9]+)\s*\(", src))
    from rsrgan_amd import _lib
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in _lib.SYMBOLS, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes, s
    # nothing to run without a device, but a null handle is refused before anything is touched
    assert lib.rsrgan_forward_g_stream(None, None, None, 1, None, None) < 0
    assert b"null handle" in lib.rsrgan_last_error()
