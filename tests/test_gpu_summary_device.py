"""The device route of the TensorBoard summaries: the discriminator's logits handed out by the C ABI (rsrgan_d_logits) against the fp64
oracle, their histograms straight from the handle's buffer (rsrgan_d_logits_hist) against rsrgan_hist of the dense tensors, and
Model.run_summaries with device_summaries=True against the same model with it off."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dnn_gan_oracle as DO
from oracle import rsrgan_oracle as O
from rsrgan_amd import summary as S
from tests import hist_ref as R
from tests.helpers import args_for, build_hip_pair, overrides, rand_batch, small_cfg

pytestmark = pytest.mark.gpu

ATOL = 1e-4                    # the bound tests/test_gpu_parity.py puts on forward outputs


def _hist_pair_agrees(engine, real, fake):
    """d_logits_hist() against rsrgan_hist of the dense tensors: every field but the two sums equal, the sums within the bound"""
    direct = engine.d_logits_hist().cpu().numpy()
    dense = engine.hist([real, fake]).cpu().numpy()
    assert direct.shape == dense.shape == (2, 5 + R.NL)
    for k, t in enumerate((real, fake)):
        assert R.same(direct[k][:3], dense[k][:3]) and np.array_equal(direct[k][5:], dense[k][5:])
        R.check(direct[k], t.cpu().numpy())
        R.check(dense[k], t.cpu().numpy())


def _sequence_case(cfg, B, T, flags, seed):
    model, oracle = build_hip_pair(cfg, B, T, seed=seed, flags=flags, init_disc_noise_std=0.0)
    x, lab, ln = rand_batch(cfg, B, T, seed=seed + 1, ragged=True)
    e = model.engine
    with pytest.raises(Exception, match="no D-run"):
        e.d_logits()
    e.d_backward(x, lab, ln, None, None, train=False, apply=False)
    real, fake = e.d_logits()
    assert tuple(real.shape) == tuple(fake.shape) == (B, T)
    x64, lab64 = x.astype(np.float64), lab.astype(np.float64)
    y, _ = O.generator_fwd(cfg, oracle.g, x64, ln)
    want_real = np.asarray(O.discriminator_fwd(cfg, oracle.d, lab64, ln, None)[0]).reshape(B, T)
    want_fake = np.asarray(O.discriminator_fwd(cfg, oracle.d, y, ln, None)[0]).reshape(B, T)
    err = max(np.abs(real.cpu().numpy() - want_real).max(), np.abs(fake.cpu().numpy() - want_fake).max())
    print("d_logits vs oracle: max abs error %.3e" % err)
    assert err < ATOL
    _hist_pair_agrees(e, real, fake)
    # a G-run writes D(G(x)) over them: nothing to hand out until the next D-run
    e.g_backward(x, lab, ln, None, train=False, reuse=False, apply=False)
    with pytest.raises(Exception, match="no D-run"):
        e.d_logits_hist()
    assert e.device_status() == 0
    return model, (x, lab, ln)


def test_sequence_logits_lstm():
    """B = 4: where the batch is padded to a 32-row group, 28 of its rows are padding and none of them may be handed out"""
    _sequence_case(small_cfg(), 4, 7, 3, seed=21)


def test_sequence_logits_res_lstm_l():
    _sequence_case(small_cfg("res_lstm_l"), 4, 7, 3, seed=23)


def test_sequence_logits_of_a_padded_full_size_batch():
    """the reference's sizes at the shipped recipe's batch_size = 8: the persistent launches pad the batch to 32 rows (tests/test_gpu_padrows.py)"""
    _sequence_case(O.NetCfg(), 8, 9, 3, seed=25)


def test_frame_level_logits_are_the_clipped_ones():
    from tests.test_gpu_dnn_gan import _dnn_pair
    cfg = DO.DnnCfg(input_dim=6, output_dim=5, left_context=2, right_context=1, g_units=20, g_hidden=3, d_units=18, d_hidden=2)
    N = 7
    m, o = _dnn_pair(cfg, N, seed=31)
    d = {k: (np.asarray(v) * (3.0 if k.endswith("weights") else 1.0)).astype(np.float32) for k, v in o.d.items()}     # logits well outside [-0.5, 1.5]
    m.set_vars(None, d)
    o.d = {k: v.astype(np.float64) for k, v in d.items()}
    rng = np.random.default_rng(32)
    x = rng.standard_normal((N, cfg.fed_dim)).astype(np.float32); lab = rng.standard_normal((N, cfg.output_dim)).astype(np.float32)
    m.engine.d_backward(x[:, None], lab[:, None], None, train=False, apply=False)
    real, fake = m.engine.d_logits()
    assert tuple(real.shape) == tuple(fake.shape) == (N, 1)
    x64, lab64 = x.astype(np.float64), lab.astype(np.float64)
    di = o._d_inputs(x64)
    want, raws = [], []
    for tail in (lab64, o.forward(x64)):
        out, raw, _ = DO.d_forward(cfg, o.d, np.concatenate([di, tail], 1), False)
        want.append(out.reshape(N, 1)); raws.append(raw)
    raws = np.concatenate(raws)
    assert (raws < cfg.clip_lo).any() or (raws > cfg.clip_hi).any(), "the case does not reach the clip"
    got = np.stack([real.cpu().numpy(), fake.cpu().numpy()])
    assert got.min() >= cfg.clip_lo and got.max() <= cfg.clip_hi
    err = np.abs(got - np.stack(want)).max()
    print("frame-level d_logits vs clipped oracle: max abs error %.3e" % err)
    assert err < ATOL
    _hist_pair_agrees(m.engine, real, fake)


def _events(tmp_path, name, blob):
    w = S.FileWriter(str(tmp_path / name))
    w.add_summary(blob, 5); w.close()
    ev = S.read_events(w.path)[1]
    assert ev[1] == 5
    return ev[2]


def _same_histogram(a, b, values, scale):
    """two parsed histograms of `values`: min, max, num, bucket_limit and bucket equal; the sums within scale x the derived bound"""
    assert R.same([a[k] for k in ("min", "max", "num")], [b[k] for k in ("min", "max", "num")]), (a, b)
    assert np.array_equal(a["bucket_limit"], b["bucket_limit"]) and np.array_equal(a["bucket"], b["bucket"])
    _, (b_sum, b_sq) = R.record(values)
    print("sum: |a - b| = %.3e (bound %.3e); sum_squares: |a - b| = %.3e (bound %.3e)"
          % (abs(a["sum"] - b["sum"]), scale * b_sum, abs(a["sum_squares"] - b["sum_squares"]), scale * b_sq))
    assert abs(a["sum"] - b["sum"]) <= scale * b_sum and abs(a["sum_squares"] - b["sum_squares"]) <= scale * b_sq


def test_run_summaries_on_the_device_against_the_host_route(tmp_path):
    cfg, B, T = small_cfg(), 4, 7
    model, _ = build_hip_pair(cfg, B, T, seed=41, flags=3, init_disc_noise_std=0.0)
    x, lab, ln = rand_batch(cfg, B, T, seed=42, ragged=True)
    assert model.device_summaries is False
    off = _events(tmp_path, "off", model.run_summaries(x, lab, ln))
    model.device_summaries = True
    on = _events(tmp_path, "on", model.run_summaries(x, lab, ln))
    assert list(off) == list(S.LOSS_TAGS) + ["real_clean", "real_noise", "g_clean"]
    assert list(on) == list(S.LOSS_TAGS) + list(S.HIST_TAGS) and len(on) == 12
    for t in S.LOSS_TAGS:
        assert on[t] == off[t], t
    y = model.forward(x, ln)
    for tag, values in (("real_clean", x), ("real_noise", lab), ("g_clean", y)):
        assert on[tag]["num"] == values.size
        _same_histogram(on[tag], off[tag], values, 2.0)              # each side within the bound of the exact sum
    # the logits this fetch saw: the same D-run again (train=False changes nothing)
    model.engine.d_backward(x, lab, ln, None, None, train=False, apply=False)
    real, fake = (t.cpu().numpy() for t in model.engine.d_logits())
    ref = _events(tmp_path, "ref", S.model_summaries([on[t] for t in S.LOSS_TAGS], d_real=real, d_fake=fake))
    for tag, values in (("d_real", real), ("d_fake", fake)):
        assert on[tag]["num"] == B * T
        _same_histogram(on[tag], ref[tag], values, 2.0)
    # device tensors in, the same summary out
    dev = model.engine.device
    again = _events(tmp_path, "dev", model.run_summaries(torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(ln).to(dev)))
    assert list(again) == list(on)
    for tag in S.HIST_TAGS:
        assert again[tag]["num"] == on[tag]["num"] and np.array_equal(again[tag]["bucket"], on[tag]["bucket"])


def test_trainer_without_a_discriminator_writes_three_histograms(tmp_path):
    from rsrgan_amd.trainer import RNNTrainer
    cfg, B, T = small_cfg(), 4, 6
    m = RNNTrainer(None, args_for(cfg, B, device_summaries=True), ["gpu:0"], max_frames=T, net_overrides=overrides(cfg))
    x, lab, ln = rand_batch(cfg, B, T, seed=52, ragged=True)
    on = _events(tmp_path, "on", m.run_summaries(x, lab, ln))
    m.device_summaries = False
    off = _events(tmp_path, "off", m.run_summaries(x, lab, ln))
    assert list(on) == list(off) == list(S.LOSS_TAGS) + ["real_clean", "real_noise", "g_clean"]
    for tag, values in (("real_clean", x), ("real_noise", lab), ("g_clean", m.forward(x, ln))):
        _same_histogram(on[tag], off[tag], values, 2.0)
    lib, t = m.engine.lib, C.c_int32()
    assert lib.rsrgan_d_logits(m.engine.h, None, None, C.byref(t), None) == -1 and b"no discriminator" in lib.rsrgan_last_error()


def test_inference_handle_refuses_d_logits():
    from rsrgan_amd import GAN_RNN
    cfg = small_cfg()
    m = GAN_RNN(None, args_for(cfg, 2), ["gpu:0"], max_frames=5, net_overrides=overrides(cfg), inference_only=True)
    lib, t = m.engine.lib, C.c_int32()
    assert lib.rsrgan_d_logits(m.engine.h, None, None, C.byref(t), None) == -1
    assert b"inference-only" in lib.rsrgan_last_error()
    out = torch.zeros(2, 5 + R.NL, dtype=torch.float64, device=m.engine.device)
    assert lib.rsrgan_d_logits_hist(m.engine.h, C.c_void_p(out.data_ptr()), None) == -1
    assert b"inference-only" in lib.rsrgan_last_error()
