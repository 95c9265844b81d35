"""Audio out in the loop, on a small supervised model (RNNTrainer, lstm, input_dim = 257 x (1 + 1 + 1), output_dim = 257, random weights
saved as a checkpoint) and three short wavs:

  * run_rnn --decode --wav_scp .. --wav_out DIR on the host route and with --device_features, once plain and once with --decode_chunk 10
    --decode_streams 2: every run writes one wav per utterance with the input's sample count and a wav.scp; no sample of a device-route
    file differs from the host-route file by more than 1 (the quantisation step); feats.ark equals the one written without --wav_out;
  * HipEngine.synthesize on the matrices of feats.ark meets the bound of tests/test_gpu_wave_synth_ops.py against float64;
  * one training iteration of run_rnn from --tr_labels_wav_scp .. --label_kind lps --device_features feeds label batches equal, bit for
    bit, to op_feat_wave of the label audio pushed through rsrgan_feat_batch (as tests/test_gpu_mfcc_loop.py checks the MFCC labels),
    and gives the losses and variable bits of a twin fed those tensors."""
import os

import numpy as np
import pytest
import torch

from rsrgan_amd.io import ArkReader
from rsrgan_amd.io import wave as W
from rsrgan_amd.train import device_batch
from tests import wave_synth_ref as Y
from tests.helpers import overrides, small_cfg
from tests.test_gpu_mfcc_loop import _expand, _twin_items
from tests.test_mfcc_host import write_wavs

pytestmark = pytest.mark.gpu

LEFT, RIGHT, NB = 1, 1, 257
FRAMES = [6, 23, 3]


def _cmvn(tmp_path):
    rng = np.random.default_rng(8)
    np.savez(tmp_path / "train_cmvn.npz", mean_inputs=20.0 + rng.standard_normal(NB), stddev_inputs=rng.uniform(2.0, 4.0, NB),
             mean_labels=18.0 + rng.standard_normal(NB), stddev_labels=rng.uniform(1.0, 3.0, NB))


def _matrices(scp):
    rd = ArkReader()
    rd(scp)
    return {u: np.asarray(rd.read_utt_data_from_index(i)) for i, u in enumerate(rd.utt_ids)}


def test_decode_writes_audio(tmp_path, capsys):
    from rsrgan_amd import run_rnn as RR
    from rsrgan_amd.io.wave_cmvn import wave_ops
    from rsrgan_amd.trainer import RNNTrainer
    cfg = small_cfg("lstm", input_dim=NB * (LEFT + 1 + RIGHT), output_dim=NB)
    ov = overrides(cfg)
    a, _, data = write_wavs(tmp_path, "te", FRAMES, np.random.default_rng(31), spec=W.DEFAULT)
    _cmvn(tmp_path)
    base = ["--decode", "--data_dir", str(tmp_path), "--wav_scp", a, "--input_dim", str(NB), "--output_dim", str(NB), "--left_context",
            str(LEFT), "--right_context", str(RIGHT), "--save_dir", str(tmp_path / "exp"), "--max_frames", "32", "--g_type", "lstm", "--batch_size", "1"]
    FLAGS = RR.build_parser().parse_args(base)
    RNNTrainer(None, FLAGS, ["gpu:0"], cross_validation=True, max_frames=32, net_overrides=ov).save(FLAGS.save_dir, 1)

    def run(tag, extra):
        out = tmp_path / ("wav_" + tag)
        F = RR.build_parser().parse_args(base + extra + (["--wav_out", str(out)] if tag != "none" else []))
        scp = RR.decode(F, log=lambda s: None, net_overrides=ov)
        ark = open(scp[:-4] + ".ark", "rb").read()
        if tag == "none":
            return ark, _matrices(scp), None
        lines = [l.split() for l in open(out / "wav.scp")]
        assert [l[0] for l in lines] == sorted(data) and sorted(os.listdir(out)) == sorted([u + ".wav" for u in data] + ["wav.scp"])
        wavs = {u: W.read_wav(p) for u, p in lines}
        for u in data:
            assert wavs[u].shape == data[u][0].shape and wavs[u].dtype == np.int16 and wavs[u].any()
        return ark, _matrices(scp), wavs

    chunked = ["--decode_chunk", "10", "--decode_streams", "2"]
    runs = {k: run(k, e) for k, e in (("none", ["--device_features"]), ("host", []), ("dev", ["--device_features"]),
                                      ("hostc", chunked), ("devc", ["--device_features"] + chunked))}
    assert runs["dev"][0] == runs["none"][0], "--wav_out changed feats.ark"
    for h, d in (("host", "dev"), ("hostc", "devc")):
        for u in data:
            diff = np.abs(runs[h][2][u].astype(np.int32) - runs[d][2][u].astype(np.int32)).max()
            assert diff <= 1, (h, d, u, diff)
    # the float outputs, through HipEngine.synthesize on the matrices that were written: the operator test's bound against float64
    eng = wave_ops()
    mats = runs["dev"][1]
    utts = sorted(data)
    wb = W.pack_wave([data[u][0] for u in utts])
    lps = np.concatenate([mats[u] for u in utts], 0).astype(np.float32)
    out, seg = eng.synthesize(wb, lps)
    eng.upload_stream().synchronize()
    out = out.cpu().numpy()
    # a device tensor of the rows gives the same bits
    out2, _ = eng.synthesize(wb, torch.from_numpy(lps).to(eng.device))
    eng.upload_stream().synchronize()
    assert out2.cpu().numpy().tobytes() == out.tobytes()
    lines = []
    for i, u in enumerate(utts):
        m = lps[wb.offsets[i]:wb.offsets[i + 1]]
        ref, base32 = Y.synth(m, data[u][0]), Y.synth_fp32_baseline(m, data[u][0])
        got = out[seg[i, 0]:seg[i, 0] + seg[i, 1]]
        e, b = Y.figure(got, ref), Y.bound(base32, ref)
        lines.append("%s n %d  e %.3e  bound %.3e  rms %.1f" % (u, ref.shape[0], e, b, np.sqrt((ref * ref).mean())))
        assert e <= b, lines[-1]
        # and the file is that output, quantised
        assert np.abs(W.quantize_pcm(ref).astype(np.int32) - runs["dev"][2][u].astype(np.int32)).max() <= 1
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    with pytest.raises(ValueError, match="MFCC"):
        eng.synthesize(W.pack_wave([data[utts[0]][0]], spec=W.MFCC_DEFAULT), np.zeros((1, 40), np.float32))


def test_one_iteration_with_lps_labels(tmp_path):
    from rsrgan_amd import run_rnn as RR
    from rsrgan_amd.run_gan_rnn import _cmvn as load_cmvn, check_wav_flags, split_reader
    from rsrgan_amd.trainer import RNNTrainer
    cfg = small_cfg("lstm", input_dim=NB * (LEFT + 1 + RIGHT), output_dim=NB)
    ov = overrides(cfg)
    a, b, data = write_wavs(tmp_path, "tr", [5, 9, 4, 7], np.random.default_rng(32), spec=W.DEFAULT)
    _cmvn(tmp_path)
    FLAGS = RR.build_parser().parse_args(["--data_dir", str(tmp_path), "--tr_inputs_wav_scp", a, "--tr_labels_wav_scp", b, "--label_kind", "lps",
                                          "--device_features", "--input_dim", str(NB), "--output_dim", str(NB), "--left_context", str(LEFT),
                                          "--right_context", str(RIGHT), "--batch_size", "4", "--save_dir", str(tmp_path / "exp"),
                                          "--max_frames", "16", "--g_learning_rate", "0.001"])
    check_wav_flags(FLAGS)
    cmvn = load_cmvn(FLAGS)
    mk = lambda: RNNTrainer(None, FLAGS, ["gpu:0"], max_frames=16, net_overrides=ov)
    m1, m2 = mk(), mk()
    reader = lambda: split_reader(FLAGS, "tr", cmvn, False, None)
    ids, xb, yb, lengths = next(iter(reader()))
    assert yb.spec is W.DEFAULT and yb.shape == (4, 9, NB) and xb.shape == (4, 9, NB * 3)
    x, lab, ln = device_batch(m1, xb, yb, lengths)
    torch.cuda.synchronize()
    wy, wl = _expand(m1.engine, yb)                                      # op_feat_wave of the label audio, then rsrgan_feat_batch
    wx, _ = _expand(m1.engine, xb)
    assert torch.equal(lab.view(torch.int32), wy.view(torch.int32)) and torch.equal(x.view(torch.int32), wx.view(torch.int32))
    assert ln.cpu().tolist() == wl.cpu().tolist() == lengths.tolist()
    u = ids[0]
    host = (W.lps_from_wave(data[u][1]).astype(np.float64) - cmvn["mean_labels"]) / cmvn["stddev_labels"]
    assert np.abs(lab[0, :host.shape[0]].cpu().numpy() - host).max() < 1e-3
    # one supervised iteration from that reader: the losses and variable bits of a twin fed the tensors
    items = _twin_items(m2, reader())
    assert len(items) == 1
    r1 = RR.train_one_iteration(m1, 1, 0, reader())
    r2 = RR.train_one_iteration(m2, 1, 0, items)
    assert np.all(np.isfinite(r1)) and r1 == r2 and r1[0] > 0, (r1, r2)
    g1, g2 = m1.get_vars()[0], m2.get_vars()[0]
    assert len(g1) > 0 and all(np.array_equal(g1[k], g2[k]) for k in g1)
    assert m1.engine.device_status() == 0
