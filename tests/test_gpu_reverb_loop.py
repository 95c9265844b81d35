"""The simulation through the call sites, on four wav files of 0.2 .. 0.4 s, three 103-tap RIRs and two noises, with the recipes' framings
(257 LPS bins, 40 MFCC) and a small generator:

  * HipEngine.featurize of a WaveBatch with a plan equals, bit for bit, op_wave_reverb, then op_feat_wave(kind = 1), then op_feat_batch
    called one by one; shards through rows() give the same rows;
  * HipEngine.simulate agrees with the host route's PCM (io.reverb.reverberate, float64) within the bound of tests/test_gpu_reverb_ops.py:
    e = max |out - host| / rms(host) at most 4 x the largest e of reverb_ref.reverb_fp32_yardstick over the same utterances, evaluated here;
  * run_rnn with --tr_rir_scp --cv_rir_scp --device_features trains, cross-validates and saves; the second epoch draws other rooms for the
    training split and the same (epoch 0's) for cross-validation."""
import os
import wave

import numpy as np
import pytest
import torch

from rsrgan_amd.io import reverb as RV
from rsrgan_amd.io import wave as W
from rsrgan_amd.io.wave_reader import WaveBatchReader
from tests import reverb_ref as RR
from tests.helpers import build_hip_pair, small_cfg

pytestmark = pytest.mark.gpu

B, COUNTS = 4, (3300, 4100, 6400, 4800)


def _corpus(d, tag="tr"):
    rng = np.random.default_rng(3)
    lab, rir, noi = [], [], []

    def wav(path, x):
        with wave.open(str(path), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
            f.writeframes(np.asarray(x, "<i2").tobytes())
    for i, n in enumerate(COUNTS):
        wav(d / ("%s%d.wav" % (tag, i)), np.clip(np.rint(rng.standard_normal(n) * 2500), -32768, 32767))
        lab.append("%s%d %s" % (tag, i, d / ("%s%d.wav" % (tag, i))))
    for i, q in enumerate((0, 40, 102)):
        h = rng.standard_normal(103) * 0.2 * np.exp(-np.arange(103) / 30.0)
        h[q] = 1.5
        np.save(d / ("r%d.npy" % i), h.astype(np.float32))
        rir.append("rir%d %s" % (i, d / ("r%d.npy" % i)))
    for i, n in enumerate((900, 2500)):
        wav(d / ("n%d.wav" % i), np.rint(rng.standard_normal(n) * 700))
        noi.append("noise%d %s" % (i, d / ("n%d.wav" % i)))
    out = []
    for name, lines in ((tag + "_labels.scp", lab), ("rir.scp", rir), ("noise.scp", noi)):
        (d / name).write_text("\n".join(lines) + "\n")
        out.append(str(d / name))
    return out


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("reverb_loop")
    lab, rir, noi = _corpus(d)
    model, _ = build_hip_pair(small_cfg("lstm", input_dim=257 * 3, output_dim=40), B, 64, seed=1)
    rng = np.random.default_rng(4)
    cmvn = dict(mean_inputs=rng.standard_normal(257) + 15.0, stddev_inputs=rng.uniform(0.5, 2.0, 257), mean_labels=rng.standard_normal(40),
                stddev_labels=rng.uniform(0.5, 2.0, 40))
    sim = RV.ReverbSim(rir, noi, RV.ReverbSpec(fft=256), seed=3)
    reader = WaveBatchReader(None, lab, B, 1, 1, cmvn=cmvn, num_buckets=1, shuffle=False, device_features=True, simulate=sim)
    return model.engine, reader, sim


def test_featurize_is_the_three_entries_one_by_one(setup):
    eng, reader, sim = setup
    ids, X, Y, lengths = next(iter(reader))
    assert X.plan is not None and len(ids) == B
    x, ln = eng.featurize(X, ready=True)
    torch.cuda.synchronize()
    dev = eng.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rir, rseg = RV.rir_table(sim.rirs)
    noise, nseg, npow = RV.noise_table(sim.noises)
    C = sim.spec.fft
    counts = X.seg[:, 1]
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    oseg = np.stack([first, counts], 1).astype(np.int64)
    pcm = torch.full((int(counts.sum()),), -7.0, dtype=torch.float32, device=dev)
    work = torch.zeros(eng.wave_reverb_work(B, int(counts.max()), 103, C), dtype=torch.uint8, device=dev)
    eng.op_wave_reverb(t(X.samples), t(X.seg), t(rir), t(rseg), t(noise), t(nseg), t(npow), t(X.plan.sel), t(X.plan.snr), B, C,
                       t(W.twiddle_table(2 * C)), pcm, t(oseg), work, None, True, True)
    s = X.spec
    off = t(X.offsets)
    raw = torch.empty(int(X.offsets[-1]), s.bins, dtype=torch.float32, device=dev)
    eng.op_feat_wave(pcm, t(oseg), off, B, t(W.window_table(s.window, s.frame_length).astype(np.float32)), t(W.twiddle_table(s.padded)), raw,
                     s.frame_length, s.frame_shift, s.padded, s.preemph)
    T = X.shape[1]
    want = torch.empty(B, T, s.bins * 3, dtype=torch.float32, device=dev)
    wl = torch.empty(B, dtype=torch.int32, device=dev)
    eng.op_feat_batch(raw, off, B, T, s.bins, 1, 1, t(X.mean), t(X.stddev), want, wl)
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int32), want.view(torch.int32)) and ln.cpu().tolist() == wl.cpu().tolist() == lengths.tolist()
    assert torch.isfinite(x).all()
    for lo, hi in ((0, 1), (1, 4)):
        px, pl = eng.featurize(X.rows(lo, hi), ready=True)
        assert torch.equal(px.view(torch.int32), x[lo:hi].view(torch.int32)) and pl.cpu().tolist() == lengths[lo:hi].tolist()
    assert eng.device_status() == 0


def test_simulate_agrees_with_the_host_route(setup, capsys):
    eng, reader, sim = setup
    ids, X, Y, lengths = next(iter(reader))
    gains = torch.zeros(B, 2, dtype=torch.float32, device=eng.device)
    pcm, dseg, oseg = eng.simulate(X, gains=gains)
    eng.upload_stream().synchronize()
    pcm, gains = pcm.cpu().numpy(), gains.cpu().numpy()
    assert np.array_equal(oseg, dseg.cpu().numpy()) and np.array_equal(oseg[:, 1], X.seg[:, 1])
    yard, worst, lines = 0.0, 0.0, []
    for k in range(B):
        x = X.samples[int(X.seg[k, 0]):int(X.seg[k, 0] + X.seg[k, 1])]
        r, v, s, m = (int(a) for a in X.plan.sel[k])
        snr = float(X.plan.snr[k])
        host, (c, g) = RV.reverberate(x, sim.rirs[r], sim.noises[v] if v >= 0 else None, float(sim.noise_pow[v]) if v >= 0 else None, s, m, snr,
                                      gains=True)
        args = dict(x=x, h=sim.rirs[r], cols=RR.rir_columns(sim.rirs[r]), noise=sim.noises[v] if v >= 0 else None,
                    p_v=float(sim.noise_pow[v]) if v >= 0 else None, s=s, m=m, snr=snr)
        yard = max(yard, RR.figure(RR.reverb_fp32_yardstick(**args)[0], RR.reverb_ref(**args)[0]))
        got = pcm[int(oseg[k, 0]):int(oseg[k, 0] + oseg[k, 1])]
        e = RR.figure(got, host)
        worst = max(worst, e)
        lines.append("utt %d n %d rir %d noise %d: e %.3e  c %.6f (host %.6f)  g %.6f (host %.6f)" % (k, x.shape[0], r, v, e, gains[k, 0], c, gains[k, 1], g))
        assert abs(gains[k, 0] - c) <= 1e-5 * c and abs(gains[k, 1] - g) <= 1e-5 * g
    with capsys.disabled():
        print("\n" + "\n".join(lines) + "\nyardstick %.3e, bound 4 x" % yard)
    assert worst <= 4.0 * yard, (worst, yard)


def test_run_rnn_from_clean_audio(tmp_path, monkeypatch):
    from rsrgan_amd import run_rnn as R
    lab, rir, noi = _corpus(tmp_path)
    cv_lab = _corpus(tmp_path, "cv")[0]
    np.savez(tmp_path / "train_cmvn.npz", mean_inputs=np.full(257, 15.0), stddev_inputs=np.full(257, 3.0), mean_labels=np.zeros(40),
             stddev_labels=np.full(40, 10.0))
    drawn = []
    plan0 = RV.ReverbSim.plan

    def spy(self, utt_indices, counts, epoch=None):
        p = plan0(self, utt_indices, counts, epoch)
        drawn.append((self.epoch, tuple(utt_indices), p.sel.copy()))
        return p
    monkeypatch.setattr(RV.ReverbSim, "plan", spy)
    FLAGS, _ = R.build_parser().parse_known_args([
        "--data_dir", str(tmp_path), "--tr_rir_scp", rir, "--tr_labels_wav_scp", lab, "--cv_rir_scp", rir, "--cv_labels_wav_scp", cv_lab,
        "--noise_scp", noi, "--sim_seed", "9", "--device_features", "--batch_size", "4", "--min_epochs", "2", "--max_epochs", "2",
        "--left_context", "1", "--right_context", "1", "--save_dir", str(tmp_path / "exp"), "--max_frames", "64", "--g_learning_rate", "0.001"])
    logs = []
    hist = R.train(FLAGS, log=logs.append, net_overrides=dict(g_layers=1, g_cells=8, g_proj=4))
    text = "\n".join(logs)
    assert len(hist) == 2 and np.all(np.isfinite(hist)) and "#train_batch = 1, #valid_batch = 1" in text
    assert os.path.exists(tmp_path / "exp" / "checkpoint")
    epochs = sorted({e for e, _, _ in drawn})
    assert epochs == [0, 1]
    e0 = [sel for e, _, sel in drawn if e == 0]
    e1 = [sel for e, _, sel in drawn if e == 1]
    # the training split draws once per epoch, cross-validation once per epoch with epoch 0 (its own ReverbSim): 2 + 1 plans at epoch 0, 1 at epoch 1
    assert len(e1) == 1 and len(e0) == 3
    assert any(np.array_equal(a, b) for a in e0 for b in e0 if a is not b)                   # cross-validation: the same draws both times
    assert all(not np.array_equal(e1[0], a) for a in e0)                                     # the second epoch: other rooms
