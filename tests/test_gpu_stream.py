"""The stateful generator forward on the device (rsrgan_forward_g_stream, rsrgan_g_state_*): chunked, streaming and multi-stream
decode.  Truth is always the fp64 oracle on the WHOLE utterance (oracle.forward), never another configuration of the library.
Bounds: the small nets are held to tests/test_gpu_parity.py's bound for the same quantity (enhanced-MFCC L1, relative, 1e-4), the
reference-size nets to tests/test_gpu_plan_edges.py's (1e-3), and which forward plan ran is asserted through the launch counters
(rsrgan_profile_read_kind) -- oracle first, path second.

STREAM_MARGIN_OUT=<file>: the reference-size cases append their achieved errors (chunked and whole call, same inputs) to
that JSON file (profiles/r7_stream_margin.json was written this way)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import rsrgan_oracle as O
from tests.helpers import NET_G, args_for, build_hip_pair, overrides, rand_batch, rand_params, small_cfg

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-4                      # tests/test_gpu_parity.py
RTOL = 1e-3                           # tests/test_gpu_plan_edges.py
K_GFWD, K_NPFWD = 1, 7                # rsrgan_profile_read_kind (include/rsrgan.h)
G_TYPES = ["lstm", "res_lstm_l", "res_lstm_base"]


def l1(y, want):
    return float(np.abs(y - want).mean() / np.abs(want).mean())


def ragged(cfg, B, T, seed):
    x, _, ln = rand_batch(cfg, B, T, seed=seed, ragged=True)
    if B > 1:
        ln[-1] = 1
    if B > 2:
        ln[1] = T // 2 + 1
    return x, ln


def run_chunks(model, x, ln, cuts, reset=True):
    """x [B, T, D] cut along time into `cuts`; each row's per-chunk length from its total length (rows that end inside a chunk, rows
    already ended -> 0)"""
    outs, pos = [], 0
    for i, n in enumerate(cuts):
        lc = np.clip(ln - pos, 0, n).astype(np.int32)
        outs.append(model.forward_stream(np.ascontiguousarray(x[:, pos:pos + n]), lc, reset=True if (reset and i == 0) else None))
        pos += n
    assert pos == x.shape[1]
    return np.concatenate(outs, 1)


def kinds_of(eng):
    k = {i: eng.profile_read_kind(i)[0] for i in range(1, 9)}
    eng.profile_read()
    return k


def _margin(name, rec):
    path = os.environ.get("STREAM_MARGIN_OUT")
    print("stream margin", name, json.dumps(rec, sort_keys=True))
    if not path:
        return
    data = json.load(open(path)) if os.path.exists(path) else {"bounds": {"mfcc": RTOL}, "cases": {}}
    data["cases"][name] = rec
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


# ---- small nets: every generator type, padded and unpadded batches, all three schedules -----------------------------------------

@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("B", [1, 4, 40])
@pytest.mark.parametrize("g_type", G_TYPES)
def test_chunked_equals_oracle_small(g_type, B, flags):
    cfg = small_cfg(g_type)
    T, cuts = 37, (5, 1, 16, 15)
    model, oracle = build_hip_pair(cfg, B, 16, seed=21, flags=flags)
    x, ln = ragged(cfg, B, T, 22)
    want = oracle.forward(x, ln)
    y = run_chunks(model, x, ln, cuts)
    err = l1(y, want)
    print("small", g_type, B, flags, "chunked mfcc L1", err)
    assert err < LOSS_RTOL
    # rows past their length: the output FC's bias, as in forward_g (the oracle's rows)
    assert np.abs(y - want).max() < 1e-4
    assert model.engine.device_status() == 0


# ---- reference-size nets: each forward plan ------------------------------------------------------------------------------------

def _plan_case(name, cfg, B, flags, kind, seed, env=None):
    T, cuts = 300, (100, 100, 100)
    model, oracle = build_hip_pair(cfg, B, 100, seed=seed, flags=flags)
    x, ln = ragged(cfg, B, T, seed + 1)
    want = oracle.forward(x.astype(np.float64), ln)
    eng = model.engine
    eng.profile_begin()
    y = run_chunks(model, x, ln, cuts)
    k = kinds_of(eng)
    err = l1(y, want)
    # the whole-call error of the same inputs, chunk by chunk from zero state where the handle cannot hold them at once: a handle of
    # 300 frames on the same variables
    whole_model, _ = build_hip_pair(cfg, B, T, seed=seed, flags=flags)
    err_whole = l1(whole_model.forward(x, ln), want)
    _margin(name, dict(B=B, T=T, cuts=list(cuts), flags=flags, mfcc_l1_chunked=err, mfcc_l1_whole=err_whole, kinds={str(i): v for i, v in k.items()}))
    assert err < RTOL, (err, err_whole)
    assert eng.device_status() == 0
    if kind is None:
        assert k[K_GFWD] == 0 and k[K_NPFWD] == 0, k
    else:
        assert k[kind] == len(cuts), k
    return model


@pytest.mark.parametrize("B", [32, 8])
@pytest.mark.parametrize("g_type", ["lstm", "res_lstm_l"])
def test_chunked_reference_size_persistent(g_type, B):
    """3 x 760 / p280 and 4 x 760 / p257 (running residual sums) on k_glstm_fwd: a full 32-row group, and 8 rows (one tile lane, padded)"""
    cfg = O.NetCfg() if g_type == "lstm" else O.NetCfg.res_lstm_l()
    _plan_case("%s_B%d_persistent" % (g_type, B), cfg, B, 1, K_GFWD, 300 + B)


def test_chunked_unprojected_persistent():
    """num_proj=None (2 x 512): k_glstm_np_fwd; the state is h"""
    cfg = O.NetCfg(g_type="lstm", g_layers=2, g_cells=512, g_proj=0, d_type="dnn", d_layers=4, d_cells=1024)
    _plan_case("noproj_B64_persistent", cfg, 64, 1, K_NPFWD, 340)


def test_chunked_reference_size_launch_path():
    """RSRGAN_FLAG_WAVEFRONT off: the launch-per-phase path (rnn_forward) carries the state through slot 0 of the stash as well"""
    _plan_case("lstm_B32_launch_path", O.NetCfg(), 32, 0, None, 350)


# ---- longer than the handle ----------------------------------------------------------------------------------------------------

def test_utterance_longer_than_max_frames():
    cfg = small_cfg("lstm")
    model, oracle = build_hip_pair(cfg, 1, 64, seed=31, flags=1)
    T = 1000
    x, _, ln = rand_batch(cfg, 1, T, seed=32)
    want = oracle.forward(x, ln)
    cuts = (64,) * 15 + (40,)
    assert len(cuts) == 16 and sum(cuts) == T
    y = run_chunks(model, x, ln, cuts)
    err = l1(y, want)
    print("T=1000 in 16 calls: mfcc L1", err)
    assert err < LOSS_RTOL
    with pytest.raises(ValueError):
        model.forward(x, ln)                              # forward_g on the same handle still refuses T = 1000
    from rsrgan_amd import _lib
    import torch
    eng = model.engine
    xt = torch.zeros(1, T, cfg.input_dim, device=eng.device)
    yt = torch.zeros(1, T, cfg.output_dim, device=eng.device)
    lt = torch.tensor([T], dtype=torch.int32, device=eng.device)
    for fn in (eng.lib.rsrgan_forward_g, eng.lib.rsrgan_forward_g_stream):
        assert fn(eng.h, xt.data_ptr(), lt.data_ptr(), T, yt.data_ptr(), None) == -1      # RSRGAN_ERR_INVALID
        assert b"max_frames" in eng.lib.rsrgan_last_error()


# ---- the state API ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g_type,flags", [("lstm", 1), ("res_lstm_l", 0)])
def test_state_get_reset_set_roundtrip(g_type, flags):
    cfg = small_cfg(g_type)
    B = 4
    model, oracle = build_hip_pair(cfg, B, 16, seed=41, flags=flags)
    eng = model.engine
    x, ln = ragged(cfg, B, 24, 42)
    ln[:] = [24, 13, 24, 1]
    sf = eng.g_state_floats()
    assert sf == cfg.g_layers * (cfg.g_cells + cfg.g_proj)
    a, b_ = np.ascontiguousarray(x[:, :12]), np.ascontiguousarray(x[:, 12:])
    la, lb = np.clip(ln, 0, 12).astype(np.int32), np.clip(ln - 12, 0, 12).astype(np.int32)
    # uninterrupted
    y1 = model.forward_stream(a, la, reset=True)
    y2 = model.forward_stream(b_, lb)
    # get after a chunk, reset, set, next chunk: bitwise the same
    z1 = model.forward_stream(a, la, reset=True)
    st = eng.g_state_get().clone()
    assert st.shape == (B, sf) and float(st.abs().sum()) > 0
    eng.g_state_reset()
    assert float(eng.g_state_get().abs().sum()) == 0.0
    eng.g_state_set(st)
    z2 = model.forward_stream(b_, lb)
    assert np.array_equal(y1, z1) and np.array_equal(y2, z2)
    # rows whose length is 0 keep their state bitwise: row 3 ended in the first chunk, row 1 after one frame of the second
    after = eng.g_state_get().cpu().numpy()
    assert np.array_equal(after[3], st.cpu().numpy()[3])
    rest = model.forward_stream(b_, np.array([0, 0, 5, 0], np.int32))
    after2 = eng.g_state_get().cpu().numpy()
    assert np.array_equal(after2[[0, 1, 3]], after[[0, 1, 3]]) and not np.array_equal(after2[2], after[2])
    assert rest.shape == (B, 12, cfg.output_dim)
    # reset(rows=[1]) zeroes row 1 only
    eng.g_state_reset([1])
    after3 = eng.g_state_get().cpu().numpy()
    assert not after3[1].any() and np.array_equal(after3[[0, 2, 3]], after2[[0, 2, 3]])
    # the whole thing is the oracle's
    want = oracle.forward(x, ln)
    assert l1(np.concatenate([y1, y2], 1), want) < LOSS_RTOL
    assert eng.device_status() == 0


def test_state_parked_and_resumed_on_another_handle():
    cfg = small_cfg("lstm")
    B = 4
    m1, oracle = build_hip_pair(cfg, B, 16, seed=51, flags=1)
    m2, _ = build_hip_pair(cfg, B, 16, seed=51, flags=1)
    x, _, ln = rand_batch(cfg, B, 30, seed=52)
    want = oracle.forward(x, ln)
    y1 = m1.forward_stream(np.ascontiguousarray(x[:, :14]), np.full(B, 14, np.int32), reset=True)
    st = m1.engine.g_state_get().cpu()
    # row 2 of the first handle continues on row 0 of the second
    st2 = np.zeros_like(st.numpy())
    st2[0] = st.numpy()[2]
    m2.engine.g_state_set(st2)
    x2 = np.zeros((B, 16, cfg.input_dim), np.float32)
    x2[0] = x[2, 14:30]
    y2 = m2.forward_stream(x2, np.array([16, 0, 0, 0], np.int32))
    got = np.concatenate([y1[2], y2[0]], 0)
    assert l1(got, want[2]) < LOSS_RTOL


# ---- isolation: training calls and forward_g neither see nor disturb the carried state -----------------------------------------

@pytest.mark.parametrize("big", [False, True])
def test_stream_and_training_calls_do_not_interact(big):
    cfg = O.NetCfg() if big else small_cfg("lstm")
    B, T = (32, 12) if big else (4, 12)
    flags = 1
    plain, _ = build_hip_pair(cfg, B, T, seed=61, flags=flags)       # never streams
    mixed, oracle = build_hip_pair(cfg, B, T, seed=61, flags=flags)
    x, lab, ln = rand_batch(cfg, B, T, seed=62, ragged=True)
    xs, _, _ = rand_batch(cfg, B, 2 * T, seed=63)
    lns = np.full(B, 2 * T, np.int32)
    lns[-1] = T + 3
    # the stream alone, for reference
    alone, _ = build_hip_pair(cfg, B, T, seed=61, flags=flags)
    s_ref = run_chunks(alone, xs, lns, (T, T))
    # plain handle: forward, d_step, g_step
    p_y = plain.forward(x, ln)
    p_d = np.ravel(plain.d_step(x, lab, ln))
    p_g = np.ravel(plain.g_step(x, lab, ln, reuse_g_forward=True))
    p_y2 = plain.forward(x, ln)
    # the same calls with stream chunks in between
    s1 = mixed.forward_stream(np.ascontiguousarray(xs[:, :T]), np.clip(lns, 0, T).astype(np.int32), reset=True)
    m_y = mixed.forward(x, ln)
    m_d = np.ravel(mixed.d_step(x, lab, ln))
    m_g = np.ravel(mixed.g_step(x, lab, ln, reuse_g_forward=True))
    m_y2 = mixed.forward(x, ln)
    s2 = mixed.forward_stream(np.ascontiguousarray(xs[:, T:]), np.clip(lns - T, 0, T).astype(np.int32))
    assert np.array_equal(p_y, m_y) and np.array_equal(p_d, m_d) and np.array_equal(p_g, m_g) and np.array_equal(p_y2, m_y2)
    # the first chunk ran before any update; the second runs on updated weights on `mixed` only, so compare chunk 1 bitwise and check
    # that the state survived the training calls: a handle that streams chunk 1, takes the same updates, then streams chunk 2
    assert np.array_equal(s1, s_ref[:, :T])
    alone.forward_stream(np.ascontiguousarray(xs[:, :T]), np.clip(lns, 0, T).astype(np.int32), reset=True)
    st = alone.engine.g_state_get().clone()
    alone.forward(x, ln); alone.d_step(x, lab, ln); alone.g_step(x, lab, ln, reuse_g_forward=True); alone.forward(x, ln)
    assert np.array_equal(alone.engine.g_state_get().cpu().numpy(), st.cpu().numpy())      # untouched by forward_g / d_step / g_step
    a2 = alone.forward_stream(np.ascontiguousarray(xs[:, T:]), np.clip(lns - T, 0, T).astype(np.int32))
    assert np.array_equal(s2, a2)
    assert mixed.engine.device_status() == 0


# ---- rejections ----------------------------------------------------------------------------------------------------------------

def test_rejections():
    from rsrgan_amd import _lib
    cfg = small_cfg("lstm")
    model, _ = build_hip_pair(cfg, 2, 8, seed=71)
    eng = model.engine
    x, _, ln = rand_batch(cfg, 2, 9, seed=72)
    with pytest.raises(ValueError):
        eng.forward_g_stream(x, ln)                                           # T > max_frames
    with pytest.raises(ValueError):
        eng.forward_g_stream(x[:1, :4], ln[:1])                               # wrong batch
    with pytest.raises(ValueError):
        eng.forward_g_stream(x[:, :4, :3], ln)                                # wrong width
    with pytest.raises(ValueError):
        eng.forward_g_stream(x[:, :4], None)
    with pytest.raises(ValueError):
        eng.g_state_set(np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError):
        eng.g_state_reset([2])
    assert eng.lib.rsrgan_g_state_get(eng.h, None, None) == -1 and b"null" in eng.lib.rsrgan_last_error()
    # generators without a carried state
    from types import SimpleNamespace
    from rsrgan_amd.trainer import DNNTrainer
    from tests.test_gpu_bnlstm import _trainer as bnl_trainer

    def frame_level(g_type, din, ov):
        args = SimpleNamespace(batch_size=4, input_dim=din, output_dim=5, left_context=1, right_context=1, g_type=g_type, keep_prob=1.0,
                               batch_norm=False, num_gpu=1, save_dir=None, l2_scale=0.0, g_learning_rate=1e-3, d_learning_rate=1e-3,
                               init_mse_weight=1.0, disc_updates=1, gen_updates=1)
        return DNNTrainer(None, args, ["gpu:0"], net_overrides=ov).engine
    cases = [(frame_level("dnn", 9, dict(g_layers=2, g_cells=16, d_layers=2, d_cells=16)), "no recurrent state"),
             (frame_level("rced", 16, dict(g_layers=9, g_cells=4, d_layers=2, d_cells=16)), "no recurrent state"),
             (bnl_trainer(4, 8, 2, 12, 7, 9, 5).engine, "not built")]
    for e, word in cases:
        with pytest.raises(_lib.RsrganError) as ei:
            e.g_state_floats()
        assert word in str(ei.value), ei.value
        n = C.c_int32()
        assert e.lib.rsrgan_g_state_floats(e.h, C.byref(n)) == -1            # RSRGAN_ERR_INVALID
        xx = np.zeros((e.batch_size, 1, e.input_dim), np.float32)
        with pytest.raises(_lib.RsrganError):
            e.forward_g_stream(xx, np.ones(e.batch_size, np.int32))
        with pytest.raises(_lib.RsrganError):
            e.g_state_reset()


# ---- decode_streams end to end ---------------------------------------------------------------------------------------------------

def test_decode_streams_on_the_device():
    from rsrgan_amd.stream import StreamEnhancer, decode_streams
    cfg = small_cfg("res_lstm_l")
    model, _ = build_hip_pair(cfg, 4, 64, seed=81, flags=1)
    g, d = rand_params(cfg, 81)
    oracle = O.GanRnnOracle(cfg, g, d, batch_size=1)
    rng = np.random.default_rng(82)
    utts = [rng.standard_normal((int(rng.integers(30, 401)), cfg.input_dim)).astype(np.float32) for _ in range(12)]
    outs = list(decode_streams(model, iter(utts), 64, 4))
    assert len(outs) == 12
    for i, (u, y) in enumerate(zip(utts, outs)):
        want = oracle.forward(u[None].astype(np.float64), np.array([len(u)], np.int32))[0]
        assert y.shape == want.shape
        err = l1(y, want)
        assert err < LOSS_RTOL, (i, len(u), err)
    # one live stream on row 0 of the same handle, pushes of 10 frames, no context
    enh = StreamEnhancer(model, None, 0, 0, chunk=64)
    u = utts[0]
    got = np.concatenate([enh.push(u[p:p + 10]) for p in range(0, len(u), 10)] + [enh.flush()], 0)
    want = oracle.forward(u[None].astype(np.float64), np.array([len(u)], np.int32))[0]
    assert l1(got, want) < LOSS_RTOL
    assert model.engine.device_status() == 0
