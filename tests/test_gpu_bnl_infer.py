"""The bnlstm inference handle on the device (RSRGAN_FLAG_INFER with g_type bnlstm): the fold operator against the numpy
fp64 fold, the persistent forward with the cell-norm variant (csrc/gpersist.hip CN) against tests/bnlstm_ref.forward(train=False) -- the
2e-4 the project holds bnlstm decode to (tests/test_gpu_bnlstm.py) --, streaming, long and full-size runs, the handle's refusals and
run_rnn's decode.  The variables are drawn by tests/test_bnlstm_fold_host.draw_params, so every term of the fold matters.  Which plan
ran is asserted through the launch counters (rsrgan_profile_read_kind: 1 = k_glstm_fwd, 7 = k_glstm_np_fwd)."""
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests import bnlstm_ref as R
from tests.helpers import NET_D, NET_G, rel_err
from tests.test_bnlstm_fold_host import draw_params, fold64, oracle_forward

pytestmark = pytest.mark.gpu

TOL = 2e-4                                 # tests/test_gpu_bnlstm.py:114,194
U = 2.0 ** -24                             # unit roundoff of fp32
K_GFWD, K_NPFWD = 1, 7
FLAG_WAVEFRONT, FLAG_SUPERVISED, FLAG_INFER = 1, 16, 64
ERR_INVALID, ERR_STATE = -1, -4
SMALL = dict(L=2, H=64, P=32, din=9, dout=5)       # NC = 4 = 2 * ceil(P / 16) workgroups per layer: the smallest shape the plan takes
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(B, din, dout, **kw):
    a = SimpleNamespace(batch_size=B, input_dim=din, output_dim=dout, left_context=0, right_context=0, g_type="bnlstm", keep_prob=1.0,
                        batch_norm=False, num_gpu=1, save_dir=None, l2_scale=0.0, g_learning_rate=1e-3)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _model(B, T, inference, L, H, P, din, dout, flags=FLAG_WAVEFRONT):
    from rsrgan_amd.trainer import RNNTrainer
    return RNNTrainer(None, _args(B, din, dout), ["gpu:0"], max_frames=T, net_overrides=dict(g_layers=L, g_cells=H, g_proj=P, flags=flags),
                      inference_only=inference)


def _specs(L, H, P, din, dout):
    return R.param_specs(din, dout, L, H, P)


def _lengths(B, T, seed):
    rng = np.random.default_rng(seed)
    ln = rng.integers(max(T // 2, 1), T + 1, size=B).astype(np.int32)
    ln[0] = T
    if B > 1:
        ln[-1] = 1
    return ln


def kinds_of(eng):
    k = {i: eng.profile_read_kind(i)[0] for i in range(1, 9)}
    eng.profile_read()
    return k


# ---- 1. the fold operator ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,H", [(32, 64), (7, 12), (280, 760)])
def test_fold_operator_against_fp64(P, H):
    import torch
    from rsrgan_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    p = draw_params(_specs(1, H, P, 3, 3), 51)
    pre = R.cell_prefix(0)
    want = fold64(p, 0)
    ldI, ldP = ((P + 3) & ~3) + 4, ((P + 3) & ~3) + 8
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    Wx, Wh, bias = t(p[pre + "input_kernel"]), t(p[pre + "state_kernel"]), t(p[pre + "bias"])
    bn = [t(p[pre + s + "/" + k]) for s in ("input", "state", "cell") for k in R.BN_LEAVES]
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    KxT, KhT, bf, ca, cb = nan(4 * H, ldI), nan(4 * H, ldP), nan(4 * H), nan(H), nan(H)
    ptr = lambda x: C.c_void_p(x.data_ptr())
    table = (C.c_void_p * 12)(*[x.data_ptr() for x in bn])
    rc = lib.rsrgan_op_bnl_fold(ptr(Wx), ptr(Wh), table, ptr(bias), P, H, ptr(KxT), ldI, ptr(KhT), ldP, ptr(bf), ptr(ca), ptr(cb), None)
    assert rc == 0, lib.rsrgan_last_error()
    torch.cuda.synchronize()
    KxT, KhT, bf, ca, cb = (x.cpu().numpy().astype(np.float64) for x in (KxT, KhT, bf, ca, cb))
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    e = dict(KxT=rel(KxT[:, :P], want["KxT"]), KhT=rel(KhT[:, :P], want["KhT"]), ca=rel(ca, want["ca"]))
    bias_room = 8 * U * sum(np.abs(v) for v in want["bias_terms"])
    cb_room = 8 * U * sum(np.abs(v) for v in want["cb_terms"])
    e_bias, e_cb = np.abs(bf - want["bias"]), np.abs(cb - want["cb"])
    print("fold", (P, H), "rel", e, "bias worst |err| / room", float((e_bias / bias_room).max()), "cb", float((e_cb / cb_room).max()))
    assert not np.any(KxT[:, P:]) and not np.any(KhT[:, P:])          # padding columns: written, and zero
    for k, v in e.items():
        assert v < 4 * U, (k, v)                                       # two roundings of fp32
    assert np.all(e_bias <= bias_room) and np.all(e_cb <= cb_room)


# ---- 2. the persistent path against the oracle ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,zero", [(1, ()), (4, (0, 5, 63)), (40, ()), (70, ())])
def test_persistent_forward_against_oracle(B, zero):
    T = 37
    p = draw_params(_specs(**SMALL), 61, zero)
    rng = np.random.default_rng(62 + B)
    x = rng.standard_normal((B, T, SMALL["din"])).astype(np.float32)
    ln = _lengths(B, T, 63)
    want = oracle_forward(p, x, ln, SMALL["L"])
    lean = _model(B, T, True, **SMALL)
    eng = lean.engine
    assert eng.inference and eng.tensor_table(NET_D) == []
    lean.set_vars(p)
    eng.profile_begin()
    y = lean.forward(x, ln)
    k = kinds_of(eng)
    e_lean = rel_err(y, want)
    assert np.array_equal(lean.forward(x, ln), y)
    msg = "persistent bnlstm B=%d rel err inference %.3g" % (B, e_lean)
    if B <= 64:                                       # the training handle's decode (two launches per step and layer) on the same variables
        full = _model(B, T, False, **SMALL)
        assert eng.tensor_table(NET_G) == full.engine.tensor_table(NET_G)      # names, order, offsets: a checkpoint loads
        full.set_vars(p, None)
        full.engine.profile_begin()
        y_full = full.forward(x, ln)
        k_full = kinds_of(full.engine)
        e_full = rel_err(y_full, want)
        msg += " full %.3g mutual %.3g" % (e_full, rel_err(y, y_full))
        assert e_full < TOL
        assert k_full[K_GFWD] == 0 and k_full[K_NPFWD] == 0          # (the counter tells the two paths apart)
    print(msg, "kinds", k)
    assert e_lean < TOL
    assert k[K_GFWD] == 1 and k[K_NPFWD] == 0 and k[2] == 0 and k[3] == 0, k      # one persistent launch; nothing else recurrent exists on this handle
    if zero:                                          # scale = 0 at a cell unit: tanh sees the offset alone -- the units still matter
        q = dict(p)
        for l in range(SMALL["L"]):
            name = R.cell_prefix(l) + "cell/offset"
            q[name] = p[name].copy(); q[name][list(zero)] += np.float32(0.5)
        lean.set_vars(q)
        assert rel_err(lean.forward(x, ln), oracle_forward(q, x, ln, SMALL["L"])) < TOL
        assert rel_err(lean.forward(x, ln), want) > 10 * TOL
    assert eng.device_status() == 0


# ---- 3. streaming ------------------------------------------------------------------------------------------------------------------

def test_streaming_rows_are_independent_utterances():
    L, H, P, din, dout = (SMALL[k] for k in ("L", "H", "P", "din", "dout"))
    B, T, cuts = 4, 37, (5, 1, 16, 15)
    p = draw_params(_specs(**SMALL), 71)
    rng = np.random.default_rng(72)
    x = rng.standard_normal((B, T, din)).astype(np.float32)
    lean = _model(B, T, True, **SMALL)
    eng = lean.engine
    lean.set_vars(p)
    assert eng.g_state_floats() == L * (H + P)                      # per row: (c, m) of every layer, DESIGN.md 6j
    # per chunk and row: frames fed.  row 0: one utterance of 37 frames; row 1: 19 frames, ends inside the third chunk; row 2 rests for the
    # second chunk and goes on (36 frames); row 3: 4 frames (ends inside the first chunk), reset in front of the third chunk, a second
    # utterance of 16 + 9 frames
    fed = np.array([[5, 1, 16, 15], [5, 1, 13, 0], [5, 0, 16, 15], [4, 0, 16, 9]], np.int32)
    outs, pos = [], 0
    eng.profile_begin()
    for i, n in enumerate(cuts):
        xc = np.ascontiguousarray(x[:, pos:pos + n])
        outs.append(lean.forward_stream(xc, fed[:, i], reset=True if i == 0 else ([3] if i == 2 else None)))
        pos += n
    k = kinds_of(eng)
    got = np.concatenate(outs, 1)
    assert k[K_GFWD] == len(cuts) and k[K_NPFWD] == 0, k
    bias = np.asarray(p["g_model/fully_connected_1/biases"], np.float64)

    def alone(frames):
        return oracle_forward(p, frames[None], np.array([len(frames)], np.int32), L)[0]
    want = np.broadcast_to(bias, (B, T, dout)).copy()                # (frames past a row's length: the output FC's bias)
    want[0] = alone(x[0])
    want[1, :19] = alone(x[1, :19])
    w2 = alone(np.concatenate([x[2, :5], x[2, 6:]]))
    want[2, :5], want[2, 6:] = w2[:5], w2[5:]
    want[3, :4] = alone(x[3, :4])
    want[3, 6:31] = alone(x[3, 6:31])
    errs = [rel_err(got[b], want[b]) for b in range(B)]
    print("streaming bnlstm rel err per row", errs)
    assert max(errs) < TOL
    # CARRY changes where the initial state comes from, not the arithmetic: rows that were never reset or rested, bitwise
    whole = lean.forward(x, np.array([37, 19, 1, 1], np.int32))
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    # get -> reset -> set -> continue reproduces the uninterrupted run
    a, b_ = np.ascontiguousarray(x[:, :12]), np.ascontiguousarray(x[:, 12:28])
    la, lb = np.array([12, 12, 7, 1], np.int32), np.array([16, 3, 0, 0], np.int32)
    y1 = lean.forward_stream(a, la, reset=True)
    y2 = lean.forward_stream(b_, lb)
    s2 = eng.g_state_get().cpu().numpy()
    z1 = lean.forward_stream(a, la, reset=True)
    st = eng.g_state_get().clone()
    assert float(st.abs().sum()) > 0
    eng.g_state_reset()
    assert float(eng.g_state_get().abs().sum()) == 0.0
    eng.g_state_set(st)
    z2 = lean.forward_stream(b_, lb)
    assert np.array_equal(y1, z1) and np.array_equal(y2, z2) and np.array_equal(eng.g_state_get().cpu().numpy(), s2)
    assert np.array_equal(s2[2:], st.cpu().numpy()[2:]) and not np.array_equal(s2[0], st.cpu().numpy()[0])      # resting rows keep their state
    assert eng.device_status() == 0


# ---- 4. long and full size -----------------------------------------------------------------------------------------------------------

def test_beyond_one_launch_two_persistent_launches():
    B, T = 3, 2100                                   # GP_TMAX = 2046 frames per launch
    p = draw_params(_specs(**SMALL), 81)
    x = np.random.default_rng(82).standard_normal((B, T, SMALL["din"])).astype(np.float32)
    ln = np.array([T, 2047, 1], np.int32)
    lean = _model(B, T, True, **SMALL)
    lean.set_vars(p)
    lean.engine.profile_begin()
    y = lean.forward(x, ln)
    k = kinds_of(lean.engine)
    err = rel_err(y, oracle_forward(p, x, ln, SMALL["L"]))
    print("T = 2100 bnlstm rel err", err, "kinds", k)
    assert err < TOL and k[K_GFWD] == 2 and k[K_NPFWD] == 0
    assert lean.engine.device_status() == 0


def test_full_size_against_oracle():
    cfg = dict(L=3, H=760, P=280, din=40, dout=40)
    B, T = 8, 50
    p = draw_params(_specs(**cfg), 91)
    x = np.random.default_rng(92).standard_normal((B, T, cfg["din"])).astype(np.float32)
    ln = _lengths(B, T, 93)
    lean = _model(B, T, True, **cfg)
    lean.set_vars(p)
    lean.engine.profile_begin()
    y = lean.forward(x, ln)
    k = kinds_of(lean.engine)
    err = rel_err(y, oracle_forward(p, x, ln, cfg["L"]))
    print("3 x 760 / p280 bnlstm rel err", err, "kinds", k)
    assert err < TOL and k[K_GFWD] == 1
    assert lean.engine.device_status() == 0


# ---- 5. the handle -------------------------------------------------------------------------------------------------------------------

def test_handle_footprint_refusals_and_refresh():
    import torch
    from rsrgan_amd import _lib
    B, T = 4, 37
    p = draw_params(_specs(**SMALL), 101)
    lean, full = _model(B, T, True, **SMALL), _model(B, T, False, **SMALL)
    eng, lib = lean.engine, lean.engine.lib
    print("device bytes 2 x 64 / p32, B = 4, T = 37: inference", eng.device_bytes(), "full", full.engine.device_bytes())
    assert 0 < eng.device_bytes() < full.engine.device_bytes()
    # every training call is refused
    dev = eng.device
    x = torch.zeros(B, T, SMALL["din"], device=dev); lab = torch.zeros(B, T, SMALL["dout"], device=dev)
    ln = torch.full((B,), T, dtype=torch.int32, device=dev); out = torch.zeros(8, device=dev)
    flat = torch.zeros(eng.param_count(NET_G), device=dev)
    q = lambda t: C.c_void_p(t.data_ptr())
    ptr, cnt, off = C.c_void_p(), C.c_int64(), C.c_int64()
    calls = {
        "rsrgan_d_step": lambda: lib.rsrgan_d_step(eng.h, q(x), q(lab), q(ln), T, None, None, q(out), 1, None),
        "rsrgan_g_step": lambda: lib.rsrgan_g_step(eng.h, q(x), q(lab), q(ln), T, None, q(out), 1, 0, None),
        "rsrgan_d_backward": lambda: lib.rsrgan_d_backward(eng.h, q(x), q(lab), q(ln), T, None, None, q(out), None),
        "rsrgan_g_backward": lambda: lib.rsrgan_g_backward(eng.h, q(x), q(lab), q(ln), T, None, q(out), 0, None),
        "rsrgan_apply": lambda: lib.rsrgan_apply(eng.h, NET_G, None),
        "rsrgan_grad_buffer": lambda: lib.rsrgan_grad_buffer(eng.h, NET_G, C.byref(ptr), C.byref(cnt)),
        "rsrgan_grad_bucket_count": lambda: lib.rsrgan_grad_bucket_count(eng.h, NET_G),
        "rsrgan_grad_bucket_info": lambda: lib.rsrgan_grad_bucket_info(eng.h, NET_G, 0, C.byref(off), C.byref(cnt)),
        "rsrgan_grad_bucket_wait": lambda: lib.rsrgan_grad_bucket_wait(eng.h, NET_G, 0, None),
        "rsrgan_get_grads": lambda: lib.rsrgan_get_grads(eng.h, NET_G, q(flat), None),
        "rsrgan_set_dropout": lambda: lib.rsrgan_set_dropout(eng.h, 0.5, 1),
    }
    for name, call in calls.items():
        assert call() == ERR_STATE, name
        assert b"inference" in lib.rsrgan_last_error(), (name, lib.rsrgan_last_error())
    for what in (1, 2, 3):
        assert lib.rsrgan_set_params(eng.h, NET_G, what, q(flat), None) == ERR_INVALID and b"inference" in lib.rsrgan_last_error()
    for call in (lambda: lean.g_step(x, lab, ln), lambda: lean.save("/nonexistent", 1)):
        with pytest.raises(RuntimeError):
            call()

    def create(flags, **kw):
        c = _lib.RsrganCfg()
        assert lib.rsrgan_default_cfg(_lib.G_TYPES["bnlstm"], C.byref(c)) == 0
        c.batch_size, c.max_frames, c.input_dim, c.output_dim, c.flags = 4, 8, 9, 5, flags
        c.g_layers, c.g_cells, c.g_proj = 2, 64, 32
        for k_, v in kw.items():
            setattr(c, k_, v)
        h = C.c_void_p()
        rc = lib.rsrgan_create(C.byref(c), 1, C.byref(h))
        msg = lib.rsrgan_last_error()
        if rc == 0:
            lib.rsrgan_destroy(h)
        return rc, msg
    rc, msg = create(FLAG_INFER | FLAG_SUPERVISED)                    # no RSRGAN_FLAG_WAVEFRONT: the only forward is the persistent one
    assert rc == ERR_INVALID and b"not built" in msg, msg
    rc, msg = create(FLAG_INFER | FLAG_SUPERVISED | FLAG_WAVEFRONT, g_proj=0)
    assert rc == ERR_INVALID and b"bnlstm" in msg, msg
    rc, msg = create(FLAG_INFER | FLAG_SUPERVISED | FLAG_WAVEFRONT, g_cells=16)      # 4 cells per layer: fewer workgroups than P = 32 needs reducers
    assert rc == ERR_INVALID and b"no persistent forward plan" in msg, msg
    rc, msg = create(FLAG_INFER | FLAG_WAVEFRONT)
    assert rc == ERR_INVALID and b"SUPERVISED" in msg, msg
    rc, msg = create(FLAG_INFER | FLAG_SUPERVISED | FLAG_WAVEFRONT)
    assert rc == 0, msg
    # a training handle keeps refusing the stateful calls
    n = C.c_int32()
    assert lib.rsrgan_g_state_floats(full.engine.h, C.byref(n)) == ERR_INVALID and b"not built" in lib.rsrgan_last_error()
    # RSRGAN_GP_TAGS=0: refused at create (the switch is read once per process: a child)
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); from rsrgan_amd import _lib; lib = _lib.load(); c = _lib.RsrganCfg();\n"
            "assert lib.rsrgan_default_cfg(5, C.byref(c)) == 0\n"
            "c.batch_size, c.max_frames, c.input_dim, c.output_dim, c.flags = 4, 8, 9, 5, 64 | 16 | 1\n"
            "c.g_layers, c.g_cells, c.g_proj = 2, 64, 32\n"
            "h = C.c_void_p(); rc = lib.rsrgan_create(C.byref(c), 1, C.byref(h)); print(rc, lib.rsrgan_last_error().decode())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RSRGAN_GP_TAGS="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("-1 ") and "RSRGAN_GP_TAGS" in r.stdout, r.stdout
    # set_params refreshes the fold: new moving statistics change the next forward accordingly
    rng = np.random.default_rng(102)
    xs = rng.standard_normal((B, T, SMALL["din"])).astype(np.float32)
    lns = _lengths(B, T, 103)
    lean.set_vars(p)
    y0 = lean.forward(xs, lns)
    assert rel_err(y0, oracle_forward(p, xs, lns, SMALL["L"])) < TOL
    p2 = dict(p)
    for name in p:
        if R.is_moving(name):
            p2[name] = (p[name] * np.float32(1.5) + np.float32(0.1)).astype(np.float32)
    lean.set_vars(p2)
    y1 = lean.forward(xs, lns)
    assert rel_err(y1, oracle_forward(p2, xs, lns, SMALL["L"])) < TOL
    assert rel_err(y1, y0) > 10 * TOL
    got = eng.get_params(NET_G).cpu().numpy()
    eng.set_params(NET_G, got)
    assert np.array_equal(eng.get_params(NET_G).cpu().numpy(), got)
    assert eng.device_status() == 0


# ---- 6. end to end: run_rnn.decode ---------------------------------------------------------------------------------------------------

def test_run_rnn_decode_lean_and_chunked(tmp_path):
    from rsrgan_amd import run_rnn as RR
    from rsrgan_amd.io import ArkReader, ArkWriter
    from rsrgan_amd.trainer import RNNTrainer
    rng = np.random.default_rng(111)
    L, H, P, dout = SMALL["L"], SMALL["H"], SMALL["P"], SMALL["dout"]
    din, left, right = 3, 1, 1
    w = ArkWriter(str(tmp_path / "te.scp"))
    for i, T in enumerate([5, 37, 1, 16, 60, 17]):
        w.write_next_utt(str(tmp_path / "te.ark"), "utt%02d" % i, rng.standard_normal((T, din)) * 2 + 1)
    w.close()
    np.savez(tmp_path / "train_cmvn.npz", mean_inputs=rng.standard_normal(din), stddev_inputs=rng.uniform(0.5, 2, din),
             mean_labels=rng.standard_normal(dout), stddev_labels=rng.uniform(0.5, 2, dout))
    ov = dict(g_layers=L, g_cells=H, g_proj=P, flags=FLAG_WAVEFRONT)
    base = ["--decode", "--g_type", "bnlstm", "--data_dir", str(tmp_path), "--test_inputs_scp", str(tmp_path / "te.scp"), "--input_dim", str(din),
            "--output_dim", str(dout), "--left_context", str(left), "--right_context", str(right), "--max_frames", "64"]
    mats, ckpt = {}, None
    for name, extra in (("whole", []), ("whole_lean", ["--decode_lean"]), ("chunk_lean", ["--decode_chunk", "16", "--decode_streams", "3", "--decode_lean"]),
                        ("chunk_auto", ["--decode_chunk", "16", "--decode_streams", "3"])):
        F, _ = RR.build_parser().parse_known_args(base + extra + ["--save_dir", str(tmp_path / name)])
        if ckpt is None:                                 # the checkpoint of a training model, copied to every run's save_dir
            full = RNNTrainer(None, SimpleNamespace(**dict(vars(F), batch_size=2)), ["gpu:0"], max_frames=8, net_overrides=ov)
            full.set_vars(draw_params(_specs(L, H, P, din * (left + 1 + right), dout), 112), None)
            full.save(str(tmp_path / "ckpt"), 3)
            ckpt = {f: open(str(tmp_path / "ckpt" / f), "rb").read() for f in os.listdir(str(tmp_path / "ckpt"))}
        os.makedirs(F.save_dir, exist_ok=True)
        for f, data in ckpt.items():
            with open(os.path.join(F.save_dir, f), "wb") as fh:
                fh.write(data)
        logs = []
        scp = RR.decode(F, log=logs.append, net_overrides=ov)
        assert any("Load SUCCESS" in s for s in logs)
        assert any("inference-only" in s for s in logs) == (name == "chunk_auto")
        r = ArkReader(); r(scp)
        mats[name] = [(u, np.asarray(r.read_utt_data_from_index(i))) for i, u in enumerate(r.utt_ids)]
    assert len(mats["whole"]) == 6
    for name in ("whole_lean", "chunk_lean", "chunk_auto"):
        for (ua, a), (ub, b) in zip(mats["whole"], mats[name]):
            assert ua == ub and a.shape == b.shape
            assert rel_err(b, a) < TOL, (name, ua, rel_err(b, a))
