"""Training from audio through the call sites, on a small generator (input_dim = 33, output_dim = 5, no context) with small framings
(inputs WaveSpec(64, 32, 64): 33 LPS bins; labels MfccSpec(64, 32, 64, 5 filters, 5 cepstra)) and four wav pairs of 5 to 20 frames:

  * device_batch on WaveBatchReader(device_features=True)'s item equals rsrgan_feat_wave / rsrgan_feat_mfcc followed by rsrgan_feat_batch,
    bit for bit, for inputs, labels and lengths; sharding through rows() gives the same rows;
  * one GAN iteration (train_one_iteration) fed by that reader gives the losses and variable bits of an identically initialised model fed
    the tensors device_batch returned, with and without RSRGAN_DPIPE=1; the same for one supervised iteration on RNNTrainer;
  * wave_cmvn on the device agrees with its host route: per dimension |mean - mean_host| and |stddev - stddev_host| are at most 4 x the
    per-value error figure of tests/test_gpu_mfcc_ops.py (the larger of the float32 CPU baseline's error against float64 on the same
    audio and the float32 spacing at the largest value); a mean moves by at most the largest per-value difference, and so does a standard
    deviation (centring is a projection).  The assertion is stated relative to each dimension's stddev, difference / stddev at most
    4 x figure / stddev: the tolerance is a per-value error and scales with nothing else, so this is the absolute inequality divided
    through.  -s prints the achieved relative values."""
import numpy as np
import pytest
import torch

from rsrgan_amd.io import wave as W
from rsrgan_amd.io.wave_cmvn import wave_cmvn, wave_ops
from rsrgan_amd.io.wave_reader import WaveBatchReader
from rsrgan_amd.train import device_batch
from tests import feat_ref
from tests import mfcc_ref as MR
from tests import wave_ref as R
from tests.helpers import args_for, overrides, small_cfg
from tests.test_mfcc_host import SMALL_IN, SMALL_LAB, kw_of, write_wavs

pytestmark = pytest.mark.gpu

B, FRAMES = 4, [5, 20, 11, 8]


def _setup(tmp_path):
    cfg = small_cfg("lstm", input_dim=33, output_dim=5)
    rng = np.random.default_rng(41)
    a, b, data = write_wavs(tmp_path, "tr", FRAMES, rng)
    cmvn = feat_ref.cmvn_for(rng, 33, 5)
    cmvn["mean_inputs"] = cmvn["mean_inputs"] + 15.0                   # (LPS values of this audio lie near 15)
    return cfg, a, b, data, cmvn


def _reader(a, b, cmvn):
    return WaveBatchReader(a, b, B, 0, 0, cmvn=cmvn, num_buckets=1, shuffle=True, seed=5, device_features=True, input_spec=SMALL_IN,
                           label_spec=SMALL_LAB)


def _raw(eng, wb):
    """the kernel's raw rows of a WaveBatch through the op entries, and its device offset table"""
    dev = eng.device
    us = eng.upload_stream()
    tabs = eng.wave_tables(wb.spec, us)
    us.synchronize()
    pcm, seg, off = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (wb.samples, wb.seg, wb.offsets))
    s = wb.spec
    raw = torch.empty(int(wb.offsets[-1]), s.bins, dtype=torch.float32, device=dev)
    if hasattr(s, "num_mel_bins"):
        eng.op_feat_mfcc(pcm, seg, off, len(wb), tabs[0], tabs[1], tabs[2], tabs[3], tabs[4], raw, s.frame_length, s.frame_shift, s.padded, s.preemph)
    else:
        eng.op_feat_wave(pcm, seg, off, len(wb), tabs[0], tabs[1], raw, s.frame_length, s.frame_shift, s.padded, s.preemph)
    return raw, off


def _expand(eng, wb):
    raw, off = _raw(eng, wb)
    Bn, T, D = wb.shape[0], wb.shape[1], wb.dim
    dm, ds = (torch.from_numpy(np.ascontiguousarray(v)).to(eng.device) for v in (wb.mean, wb.stddev))
    out = torch.empty(Bn, T, D * (wb.left + 1 + wb.right), dtype=torch.float32, device=eng.device)
    ln = torch.empty(Bn, dtype=torch.int32, device=eng.device)
    eng.op_feat_batch(raw, off, Bn, T, D, wb.left, wb.right, dm, ds, out, ln)
    torch.cuda.synchronize()
    return out, ln


def test_device_batch_is_the_two_kernels_then_the_splice(tmp_path):
    from rsrgan_amd import GAN_RNN
    cfg, a, b, data, cmvn = _setup(tmp_path)
    m = GAN_RNN(None, args_for(cfg, B), ["gpu:0"], max_frames=max(FRAMES), net_overrides=overrides(cfg))
    ids, xb, yb, lengths = next(iter(_reader(a, b, cmvn)))
    assert sorted(lengths.tolist()) == sorted(FRAMES) and xb.shape == (B, 20, 33) and yb.shape == (B, 20, 5)
    x, lab, ln = device_batch(m, xb, yb, lengths)
    torch.cuda.synchronize()
    wx, wl = _expand(m.engine, xb)
    wy, wl2 = _expand(m.engine, yb)
    assert torch.equal(x.view(torch.int32), wx.view(torch.int32)) and torch.equal(lab.view(torch.int32), wy.view(torch.int32))
    assert ln.cpu().tolist() == wl.cpu().tolist() == wl2.cpu().tolist() == lengths.tolist()
    # the labels are the definition's frames, normalised: to float32 accuracy (the figures themselves: tests/test_gpu_mfcc_ops.py)
    u = ids[0]
    host = (W.mfcc_from_wave(data[u][1], SMALL_LAB).astype(np.float64) - cmvn["mean_labels"]) / cmvn["stddev_labels"]
    assert np.abs(lab[0, :host.shape[0]].cpu().numpy() - host).max() < 1e-3
    # shards of the batch: the same rows
    for lo, hi in ((0, 1), (1, 4), (2, 3)):
        px, _ = m.engine.featurize(xb.rows(lo, hi), ready=True)
        py, pl = m.engine.featurize(yb.rows(lo, hi), ready=True)
        assert torch.equal(px.view(torch.int32), x[lo:hi].view(torch.int32)) and torch.equal(py.view(torch.int32), lab[lo:hi].view(torch.int32))
        assert pl.cpu().tolist() == lengths[lo:hi].tolist()
    assert m.engine.device_status() == 0


def _twin_items(model, reader):
    """the reader's full batches as host copies of what device_batch makes of them"""
    items = []
    for ids, xb, yb, ln in reader:
        if len(ids) != B:
            continue
        x, lab, n = device_batch(model, xb, yb, ln)
        torch.cuda.synchronize()
        items.append([ids, x.cpu().numpy(), lab.cpu().numpy(), n.cpu().numpy()])
    return items


@pytest.mark.parametrize("dpipe", ["0", "1"])
def test_one_gan_iteration_from_audio(tmp_path, monkeypatch, dpipe):
    monkeypatch.setenv("RSRGAN_DPIPE", dpipe)
    from rsrgan_amd import GAN_RNN, train_one_iteration
    cfg, a, b, data, cmvn = _setup(tmp_path)
    args = args_for(cfg, B, disc_updates=1, gen_updates=2, l2_scale=1e-4)
    mk = lambda: GAN_RNN(None, args, ["gpu:0"], max_frames=max(FRAMES), net_overrides=overrides(cfg))
    m1, m2 = mk(), mk()
    items = _twin_items(m2, _reader(a, b, cmvn))
    assert len(items) == 1
    r1 = train_one_iteration(None, m1, 1, 0, _reader(a, b, cmvn))
    r2 = train_one_iteration(None, m2, 1, 0, items)
    assert np.all(np.isfinite(r1)) and r1 == r2, (r1, r2)
    (g1, d1), (g2, d2) = m1.get_vars(), m2.get_vars()
    assert len(g1) > 0 and all(np.array_equal(g1[k], g2[k]) for k in g1) and all(np.array_equal(d1[k], d2[k]) for k in d1)
    assert m1.engine.device_status() == 0


def test_one_supervised_iteration_from_audio(tmp_path):
    from rsrgan_amd import run_rnn as RR
    from rsrgan_amd.trainer import RNNTrainer
    cfg, a, b, data, cmvn = _setup(tmp_path)
    args = args_for(cfg, B, g_learning_rate=1e-3, l2_scale=1e-4)
    mk = lambda: RNNTrainer(None, args, ["gpu:0"], max_frames=max(FRAMES), net_overrides=overrides(cfg))
    m1, m2 = mk(), mk()
    items = _twin_items(m2, _reader(a, b, cmvn))
    r1 = RR.train_one_iteration(m1, 1, 0, _reader(a, b, cmvn))
    r2 = RR.train_one_iteration(m2, 1, 0, items)
    assert np.all(np.isfinite(r1)) and r1 == r2 and r1[0] > 0, (r1, r2)
    g1, g2 = m1.get_vars()[0], m2.get_vars()[0]
    assert len(g1) > 0 and all(np.array_equal(g1[k], g2[k]) for k in g1)


def test_wave_cmvn_on_the_device(tmp_path, capsys):
    cfg, a, b, data, _ = _setup(tmp_path)
    host = wave_cmvn(a, b, None, SMALL_IN, SMALL_LAB)
    dev = wave_cmvn(a, b, wave_ops(), SMALL_IN, SMALL_LAB)
    # the per-value figures, from float64 and the float32 CPU baselines on the same audio
    fig_in = fig_lab = 0.0
    kw = dict(N=64, S=32, P=64)
    for x, y in data.values():
        want = R.lps(x, "hamming", **kw)
        fig_in = max(fig_in, np.abs(R.lps_fp32_baseline(x, "hamming", **kw) - want).max(), R.ulp32(np.abs(want).max()))
        c = MR.stages(y, **kw_of(SMALL_LAB))[2]
        fig_lab = max(fig_lab, np.abs(MR.mfcc_fp32_baseline(y, **kw_of(SMALL_LAB))[1] - c).max(), R.ulp32(np.abs(c).max()))
    lines = []
    for key, fig in (("inputs", fig_in), ("labels", fig_lab)):
        for name in ("mean_", "stddev_"):
            diff = np.abs(dev[name + key] - host[name + key])
            lines.append("%s%s: largest difference %.3e (%.3e of the dimension's stddev), bound 4 x %.3e" % (
                name, key, diff.max(), (diff / host["stddev_" + key]).max(), fig))
            assert (diff / host["stddev_" + key] <= 4 * fig / host["stddev_" + key]).all(), lines[-1]
    with capsys.disabled():
        print("\n" + "\n".join(lines))
