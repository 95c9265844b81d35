"""The inference-only generator handle on the device (RSRGAN_FLAG_INFER; GAN_RNN / RNNTrainer(inference_only=True)).

Two references.  (a) A full handle with the same variables: the persistent forward of an inference handle is the full handle's with the
stash stores taken out (csrc/gpersist.hip LEAN), so outputs and carried states must be BITWISE equal.  (b) The fp64 oracle on the whole
utterance, within the bounds tests/test_gpu_stream.py holds the stateful forward to: enhanced-MFCC L1 1e-3 where a persistent plan runs
(its "each forward plan" cases; tests/test_gpu_plan_edges.py holds the 2 x 64 / p32 shapes to the same 1e-3), 1e-4 for the
helpers.small_cfg() nets on the launch-per-phase path (its small-net cases).  Which plan ran is asserted through the launch counters
(rsrgan_profile_read_kind: 1 = k_glstm_fwd, 7 = k_glstm_np_fwd) -- numbers first, path second."""
import argparse
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import rsrgan_oracle as O
from tests import res_lstm_i_ref as RI
from tests.helpers import NET_D, NET_G, args_for, build_hip_pair, overrides, rand_batch, rand_params, small_cfg

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-4                      # tests/test_gpu_stream.py: the small nets
RTOL = 1e-3                           # tests/test_gpu_stream.py: each (persistent) forward plan; tests/test_gpu_plan_edges.py
K_GFWD, K_NPFWD = 1, 7                # rsrgan_profile_read_kind (include/rsrgan.h)
GP_TMAX = 2046                        # csrc/kernels.h: the longest persistent generator launch
INFER_WINDOW = 64                     # csrc/model.h Model::INFER_WINDOW
ERR_INVALID, ERR_STATE = -1, -4


def l1(y, want):
    return float(np.abs(y - want).mean() / np.abs(want).mean())


def kinds_of(eng):
    k = {i: eng.profile_read_kind(i)[0] for i in range(1, 9)}
    eng.profile_read()
    return k


# ---- the generators: the smallest shapes the persistent plans take (tests/test_gpu_plan_edges.py) ----------------------------------

def gen_cfg(name):
    """2 x LSTMP(64, p32): NC = 4 = 2 * ceil(P / 16) workgroups per layer; Din = 32 for the residual stacks.  unprojected: that file's
    2 x 512 without projection (with the LSTM discriminator: a batch is padded to the 32-row group only beside that one)"""
    if name == "lstm":
        return O.NetCfg(g_layers=2, g_cells=64, g_proj=32)
    if name in ("res_lstm_l", "res_lstm_base"):
        return O.NetCfg(g_type=name, input_dim=32, g_layers=2, g_cells=64, g_proj=32)
    if name == "res_lstm_i":
        return RI.make_cfg(input_dim=32, g_layers=2, g_cells=64, g_proj=32)
    if name == "unprojected":
        return O.NetCfg(g_type="lstm", g_layers=2, g_cells=512, g_proj=0)
    raise KeyError(name)


GENERATORS = ["lstm", "res_lstm_l", "res_lstm_base", "res_lstm_i", "unprojected"]


def full_pair(cfg, B, Tmax, seed, flags=1):
    """(full model, oracle, the generator's variables)"""
    if cfg.g_type == "res_lstm_i":
        from tests.test_gpu_res_lstm_i import pair
        g = RI.rand_g(cfg, seed)
        m, o = pair(cfg, B, Tmax, flags, seed=seed, g=g)
        return m, o, g
    m, o = build_hip_pair(cfg, B, Tmax, seed=seed, flags=flags)
    return m, o, rand_params(cfg, seed)[0]


def infer_model(cfg, B, Tmax, g, flags=1, like=None):
    from rsrgan_amd import GAN_RNN
    from rsrgan_amd.trainer import RNNTrainer
    cls = RNNTrainer if cfg.g_type == "res_lstm_i" else GAN_RNN
    m = cls(None, args_for(cfg, B), ["gpu:0"], max_frames=Tmax, net_overrides=dict(overrides(cfg), flags=flags), inference_only=True)
    eng = m.engine
    assert eng.inference and eng.tensor_table(NET_D) == [] and eng.param_count(NET_D) == 0
    if like is not None:                                # names, order and offsets of the training handle's table: a checkpoint loads
        assert eng.tensor_table(NET_G) == like.engine.tensor_table(NET_G)
    m.set_vars(g)
    return m


def ragged(cfg, B, T, seed):
    x, _, ln = rand_batch(cfg, B, T, seed=seed, ragged=True)
    if B > 1:
        ln[-1] = 1
    if B > 2:
        ln[1] = T // 2 + 1
    return x, ln


def forward_counted(model, x, ln):
    eng = model.engine
    eng.profile_begin()
    y = model.forward(x, ln)
    return y, kinds_of(eng)


# ---- 1. the persistent path ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 4, 40])
@pytest.mark.parametrize("gen", GENERATORS)
def test_persistent_forward_bitwise_and_oracle(gen, B):
    cfg = gen_cfg(gen)
    T = 37
    full, oracle, g = full_pair(cfg, B, T, seed=11)
    lean = infer_model(cfg, B, T, g, like=full)
    x, ln = ragged(cfg, B, T, 12)
    want = oracle.forward(x.astype(np.float64), ln)
    y_full, k_full = forward_counted(full, x, ln)
    y_lean, k_lean = forward_counted(lean, x, ln)
    y_again = lean.forward(x, ln)
    e_full, e_lean = l1(y_full, want), l1(y_lean, want)
    print("persistent", gen, B, "mfcc L1 full", e_full, "inference", e_lean, "kinds", k_full, k_lean)
    assert np.array_equal(y_lean, y_full)
    assert np.array_equal(y_again, y_lean)
    assert e_full < RTOL and e_lean < RTOL
    kind, other = (K_NPFWD, K_GFWD) if gen == "unprojected" else (K_GFWD, K_NPFWD)
    assert k_full[kind] == 1 and k_lean[kind] == 1 and k_full[other] == 0 and k_lean[other] == 0, (k_full, k_lean)
    assert k_lean[2] == 0 and k_lean[3] == 0                # no BPTT, no fused launch
    assert full.engine.device_status() == 0 and lean.engine.device_status() == 0


# ---- 2. streaming ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gen", ["lstm", "res_lstm_l", "res_lstm_i", "unprojected"])
def test_streaming_states_bitwise_and_oracle(gen):
    cfg = gen_cfg(gen)
    B, T, cuts = 4, 37, (5, 1, 16, 15)
    full, oracle, g = full_pair(cfg, B, 16, seed=21)
    lean = infer_model(cfg, B, 16, g, like=full)
    x, ln = ragged(cfg, B, T, 22)
    want = oracle.forward(x.astype(np.float64), ln)
    assert lean.engine.g_state_floats() == full.engine.g_state_floats()
    outs, pos, states = [], 0, []
    lean.engine.profile_begin()
    for i, n in enumerate(cuts):
        lc = np.clip(ln - pos, 0, n).astype(np.int32)
        xc = np.ascontiguousarray(x[:, pos:pos + n])
        y_f = full.forward_stream(xc, lc, reset=True if i == 0 else None)
        y_l = lean.forward_stream(xc, lc, reset=True if i == 0 else None)
        s_f, s_l = full.engine.g_state_get().cpu().numpy(), lean.engine.g_state_get().cpu().numpy()
        assert np.array_equal(y_l, y_f), (i, n)
        assert np.array_equal(s_l, s_f), (i, n)
        outs.append(y_l); states.append(s_l)
        pos += n
    k = kinds_of(lean.engine)
    err = l1(np.concatenate(outs, 1), want)
    print("streaming", gen, "mfcc L1", err, "kinds", k)
    assert err < RTOL
    assert k[K_NPFWD if gen == "unprojected" else K_GFWD] == len(cuts), k
    # rows 1 and 3 ended before the last chunk (lengths 19 and 1): their state did not move in it, bitwise
    assert np.array_equal(states[3][[1, 3]], states[2][[1, 3]]) and not np.array_equal(states[3][0], states[2][0])
    # a call in which some rows rest (length 0): they keep their state bitwise, the others move
    eng = lean.engine
    xr = np.ascontiguousarray(x[:, :12])
    eng.forward_g_stream(xr, np.array([0, 0, 5, 0], np.int32))
    after = eng.g_state_get().cpu().numpy()
    assert np.array_equal(after[[0, 1, 3]], states[3][[0, 1, 3]]) and not np.array_equal(after[2], states[3][2])
    # get -> reset -> set -> the next chunk reproduces the uninterrupted run
    a, b_ = np.ascontiguousarray(x[:, :12]), np.ascontiguousarray(x[:, 12:28])
    la, lb = np.clip(ln, 0, 12).astype(np.int32), np.clip(ln - 12, 0, 16).astype(np.int32)
    y1 = lean.forward_stream(a, la, reset=True)
    y2 = lean.forward_stream(b_, lb)
    z1 = lean.forward_stream(a, la, reset=True)
    st = eng.g_state_get().clone()
    assert float(st.abs().sum()) > 0
    eng.g_state_reset()
    assert float(eng.g_state_get().abs().sum()) == 0.0
    eng.g_state_set(st)
    z2 = lean.forward_stream(b_, lb)
    assert np.array_equal(y1, z1) and np.array_equal(y2, z2)
    assert eng.device_status() == 0 and full.engine.device_status() == 0


# ---- 3. the windowed launch-per-phase fallback -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fallback_case(g_type):
    cfg = small_cfg(g_type)                              # H = 12, P = 7 (9): no persistent plan takes it
    B, T = 4, 150                                        # three windows: 64 + 64 + 22
    g, d = rand_params(cfg, 31)
    x, _, _ = rand_batch(cfg, B, T, seed=32)
    ln = np.array([T, 30, INFER_WINDOW, 1], np.int32)    # rows that end inside the first window, at its last frame, after one frame
    want = O.GanRnnOracle(cfg, g, d, batch_size=B).forward(x.astype(np.float64), ln)
    want.setflags(write=False)
    return cfg, g, x, ln, want


@pytest.mark.parametrize("flags", [1, 0])
@pytest.mark.parametrize("g_type", ["lstm", "res_lstm_l"])
def test_windowed_fallback_against_oracle(g_type, flags):
    cfg, g, x, ln, want = _fallback_case(g_type)
    B, T = x.shape[:2]
    lean = infer_model(cfg, B, T, g, flags=flags)
    bytes0 = lean.engine.device_bytes()
    y, k = forward_counted(lean, x, ln)
    err = l1(y, want)
    print("fallback", g_type, flags, "whole call mfcc L1", err, "max abs", float(np.abs(y - want).max()))
    assert err < LOSS_RTOL and np.abs(y - want).max() < 1e-4
    assert k[K_GFWD] == 0 and k[K_NPFWD] == 0, k
    assert lean.engine.device_bytes() > bytes0           # the launch path's gates / h of one window came with its first use
    bytes1 = lean.engine.device_bytes()
    # the same through the stateful forward in chunks of 70 + 80 (two windows each)
    outs, pos = [], 0
    lean.engine.profile_begin()
    for i, n in enumerate((70, 80)):
        lc = np.clip(ln - pos, 0, n).astype(np.int32)
        outs.append(lean.forward_stream(np.ascontiguousarray(x[:, pos:pos + n]), lc, reset=True if i == 0 else None))
        pos += n
    k = kinds_of(lean.engine)
    ys = np.concatenate(outs, 1)
    err = l1(ys, want)
    print("fallback", g_type, flags, "70 + 80 mfcc L1", err)
    assert err < LOSS_RTOL and np.abs(ys - want).max() < 1e-4
    assert k[K_GFWD] == 0 and k[K_NPFWD] == 0, k
    assert lean.engine.device_bytes() == bytes1
    assert lean.engine.device_status() == 0


# ---- 4. beyond GP_TMAX: consecutive persistent launches ----------------------------------------------------------------------------

def test_beyond_gp_tmax_two_persistent_launches():
    cfg = gen_cfg("lstm")
    B, T = 4, 2100
    g, d = rand_params(cfg, 41)
    lean = infer_model(cfg, B, T, g)
    x, ln = ragged(cfg, B, T, 42)
    ln[2] = GP_TMAX + 7                                  # ends inside the second launch
    want = O.GanRnnOracle(cfg, g, d, batch_size=B).forward(x.astype(np.float64), ln)
    y, k = forward_counted(lean, x, ln)
    err, tail = l1(y, want), l1(y[:, GP_TMAX:], want[:, GP_TMAX:])
    print("T = 2100 mfcc L1", err, "frames past GP_TMAX alone", tail, "kinds", k)
    assert err < RTOL and tail < RTOL
    assert k[K_GFWD] == 2, k
    assert lean.engine.device_status() == 0


# ---- 5. reference size -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g_type,B", [("lstm", 32), ("res_lstm_l", 8)])
def test_reference_size_bitwise_and_oracle(g_type, B):
    """3 x 760 / p280 on a full 32-row group; 4 x 760 / p257 with 8 rows (padded, one tile lane)"""
    cfg = O.NetCfg() if g_type == "lstm" else O.NetCfg.res_lstm_l()
    T = 300
    full, oracle, g = full_pair(cfg, B, T, seed=51)
    lean = infer_model(cfg, B, T, g, like=full)
    x, ln = ragged(cfg, B, T, 52)
    want = oracle.forward(x.astype(np.float64), ln)
    y_full, k_full = forward_counted(full, x, ln)
    y_lean, k_lean = forward_counted(lean, x, ln)
    e = l1(y_lean, want)
    print("reference size", g_type, B, "mfcc L1", e, "bytes full", full.engine.device_bytes(), "inference", lean.engine.device_bytes())
    assert np.array_equal(y_lean, y_full)
    assert e < RTOL
    assert k_full[K_GFWD] == 1 and k_lean[K_GFWD] == 1, (k_full, k_lean)
    assert lean.engine.device_status() == 0 and full.engine.device_status() == 0


# ---- 6. footprint ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g_type", ["lstm", "res_lstm_l"])
def test_footprint_below_the_gates_stash_alone(g_type):
    from rsrgan_amd.engine_hip import HipEngine
    B, max_frames = 32, 1000
    layers, H = (3, 760) if g_type == "lstm" else (4, 760)
    gates_stashes = 4 * max_frames * B * 4 * H * layers          # bytes of the [T][N][4H] fp32 gate stashes of this configuration alone
    sizes = {}
    for inference in (True, False):
        eng = HipEngine(batch_size=B, max_frames=max_frames, g_type=g_type, flags=1, inference=inference)
        sizes[inference] = eng.device_bytes()
        eng.close()
    print("footprint", g_type, "gates stashes alone", gates_stashes, "inference handle", sizes[True], "full handle", sizes[False])
    assert 0 < sizes[True] < gates_stashes
    assert sizes[False] >= gates_stashes                          # the counter counts stashes


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals():
    import torch
    from rsrgan_amd import _lib
    cfg = small_cfg("lstm")
    B, T = 2, 6
    g, d = rand_params(cfg, 71)
    lean = infer_model(cfg, B, T, g)
    eng, lib = lean.engine, lean.engine.lib
    dev = eng.device
    x = torch.zeros(B, T, cfg.input_dim, device=dev); lab = torch.zeros(B, T, cfg.output_dim, device=dev)
    ln = torch.full((B,), T, dtype=torch.int32, device=dev); out = torch.zeros(8, device=dev)
    flat = torch.zeros(eng.param_count(NET_G), device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    ptr, cnt, off = C.c_void_p(), C.c_int64(), C.c_int64()
    state_calls = {
        "rsrgan_d_step": lambda: lib.rsrgan_d_step(eng.h, p(x), p(lab), p(ln), T, None, None, p(out), 1, None),
        "rsrgan_d_step(train=0)": lambda: lib.rsrgan_d_step(eng.h, p(x), p(lab), p(ln), T, None, None, p(out), 0, None),
        "rsrgan_g_step": lambda: lib.rsrgan_g_step(eng.h, p(x), p(lab), p(ln), T, None, p(out), 1, 0, None),
        "rsrgan_d_backward": lambda: lib.rsrgan_d_backward(eng.h, p(x), p(lab), p(ln), T, None, None, p(out), None),
        "rsrgan_g_backward": lambda: lib.rsrgan_g_backward(eng.h, p(x), p(lab), p(ln), T, None, p(out), 0, None),
        "rsrgan_apply(G)": lambda: lib.rsrgan_apply(eng.h, NET_G, None),
        "rsrgan_apply(D)": lambda: lib.rsrgan_apply(eng.h, NET_D, None),
        "rsrgan_grad_buffer": lambda: lib.rsrgan_grad_buffer(eng.h, NET_G, C.byref(ptr), C.byref(cnt)),
        "rsrgan_grad_bucket_count": lambda: lib.rsrgan_grad_bucket_count(eng.h, NET_G),
        "rsrgan_grad_bucket_info": lambda: lib.rsrgan_grad_bucket_info(eng.h, NET_G, 0, C.byref(off), C.byref(cnt)),
        "rsrgan_grad_bucket_wait": lambda: lib.rsrgan_grad_bucket_wait(eng.h, NET_G, 0, None),
        "rsrgan_get_grads": lambda: lib.rsrgan_get_grads(eng.h, NET_G, p(flat), None),
        "rsrgan_set_dropout": lambda: lib.rsrgan_set_dropout(eng.h, 0.5, 1),
    }
    for name, call in state_calls.items():
        assert call() == ERR_STATE, name
        assert b"inference" in lib.rsrgan_last_error(), (name, lib.rsrgan_last_error())
    for what in (1, 2, 3):
        for fn in (lib.rsrgan_get_params, lib.rsrgan_set_params):
            assert fn(eng.h, NET_G, what, p(flat), None) == ERR_INVALID, what
            assert b"inference" in lib.rsrgan_last_error()
    # ... and through the Python layers
    for call in (lambda: eng.d_backward(x, lab, ln), lambda: eng.g_backward(x, lab, ln), lambda: eng.apply(NET_G), lambda: eng.get_grads(NET_G),
                 lambda: eng.grad_view(NET_G), lambda: eng.grad_buckets(NET_G), lambda: eng.set_dropout(0.5)):
        with pytest.raises(_lib.RsrganError) as ei:
            call()
        assert "inference-only" in str(ei.value)
    for call in (lambda: lean.d_step(x, lab, ln), lambda: lean.g_step(x, lab, ln), lambda: lean.save("/nonexistent", 1)):
        with pytest.raises(RuntimeError):
            call()
    # what works: the variables, the table, the status, the footprint
    got = eng.get_params(NET_G).cpu().numpy()
    eng.set_params(NET_G, got)
    assert np.array_equal(eng.get_params(NET_G).cpu().numpy(), got)
    assert eng.device_status() == 0 and eng.device_bytes() > 0
    # generators without an inference handle
    for g_type, flags in (("dnn", 64), ("rced", 64), ("bnlstm", 64 | 16)):
        c = _lib.RsrganCfg()
        assert lib.rsrgan_default_cfg(_lib.G_TYPES[g_type], C.byref(c)) == 0
        c.batch_size, c.flags = 4, flags
        h = C.c_void_p()
        assert lib.rsrgan_create(C.byref(c), 1, C.byref(h)) == ERR_INVALID, g_type
        assert b"not built" in lib.rsrgan_last_error(), (g_type, lib.rsrgan_last_error())
        assert not h.value
    # a full handle still accepts everything
    full, oracle = build_hip_pair(cfg, B, T, seed=71)
    xn, labn, lnn = rand_batch(cfg, B, T, seed=72)
    assert np.allclose(np.ravel(full.d_step(xn, labn, lnn)), np.ravel(oracle.d_step(xn, labn, lnn)), rtol=1e-3)
    assert np.allclose(np.ravel(full.g_step(xn, labn, lnn, reuse_g_forward=True)), np.ravel(oracle.g_step(xn, labn, lnn)), rtol=1e-3)
    fe = full.engine
    fe.d_backward(xn, labn, lnn, train=True, apply=False); fe.apply(NET_D)
    assert fe.get_grads(NET_G).numel() == fe.param_count(NET_G) and len(fe.grad_buckets(NET_G)) >= 1 and fe.grad_view(NET_G).numel() > 0
    for what in ("adam_m", "adam_v", "ema"):
        fe.set_params(NET_G, fe.get_params(NET_G, what), what)
    fe.set_dropout(1.0)
    assert fe.device_bytes() > eng.device_bytes() and not fe.inference


# ---- 8. end to end: run_gan_rnn.decode --decode_lean --------------------------------------------------------------------------------

def test_decode_lean_writes_the_same_ark(tmp_path):
    from rsrgan_amd import GAN_RNN, run_gan_rnn as R
    from rsrgan_amd.io import ArkWriter
    rng = np.random.default_rng(81)
    cfg = gen_cfg("lstm")
    din, dout, left, right = 3, cfg.output_dim, 1, 1
    cfg.input_dim = din * (left + 1 + right)
    w = ArkWriter(str(tmp_path / "te.scp"))
    for i, T in enumerate([5, 37, 1, 16, 90, 17]):
        w.write_next_utt(str(tmp_path / "te.ark"), "utt%02d" % i, rng.standard_normal((T, din)) * 2 + 1)
    w.close()
    np.savez(tmp_path / "train_cmvn.npz", mean_inputs=rng.standard_normal(din), stddev_inputs=rng.uniform(0.5, 2, din),
             mean_labels=rng.standard_normal(dout), stddev_labels=rng.uniform(0.5, 2, dout))
    ov = dict(overrides(cfg), flags=1)
    base = ["--decode", "--data_dir", str(tmp_path), "--test_inputs_scp", str(tmp_path / "te.scp"), "--input_dim", str(din),
            "--output_dim", str(dout), "--left_context", str(left), "--right_context", str(right), "--max_frames", "128"]
    arks = {}
    for name, extra in (("whole", []), ("whole_lean", ["--decode_lean"]), ("chunk", ["--decode_chunk", "16", "--decode_streams", "4"]),
                        ("chunk_lean", ["--decode_chunk", "16", "--decode_streams", "4", "--decode_lean"])):
        F, _ = R.build_parser().parse_known_args(base + extra + ["--save_dir", str(tmp_path / name)])
        if not arks:                                     # the checkpoint of a full model, copied to every run's save_dir below
            g, d = rand_params(cfg, 82)
            full = GAN_RNN(None, argparse.Namespace(**dict(vars(F), batch_size=2)), ["gpu:0"], max_frames=8, net_overrides=ov)
            full.set_vars(g, d)
            full.save(str(tmp_path / "ckpt"), 3)
            ckpt = {f: open(str(tmp_path / "ckpt" / f), "rb").read() for f in os.listdir(str(tmp_path / "ckpt"))}
        os.makedirs(F.save_dir, exist_ok=True)
        for f, data in ckpt.items():
            with open(os.path.join(F.save_dir, f), "wb") as fh:
                fh.write(data)
        logs = []
        scp = R.decode(F, log=logs.append, net_overrides=ov)
        assert any("Load SUCCESS" in s for s in logs)
        arks[name] = open(os.path.join(os.path.dirname(scp), "feats.ark"), "rb").read()
    assert len(arks["whole"]) > 0
    assert arks["whole_lean"] == arks["whole"]
    assert arks["chunk_lean"] == arks["chunk"]
