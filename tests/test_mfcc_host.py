"""The host side of training from audio: io.wave.MfccSpec, its tables and the host route mfcc_from_wave against the independent float64
definition of tests/mfcc_ref.py; WaveBatch / pack_wave with an MfccSpec; io.wave_reader.WaveBatchReader against PaddedBatchReader's plan
and against the host route's frames; io.wave_cmvn's host route against direct NumPy statistics.  No device."""
import wave as stdwave

import numpy as np
import pytest

from rsrgan_amd.io import PaddedBatchReader, prefetch
from rsrgan_amd.io import wave as W
from rsrgan_amd.io.features import apply_cmvn, splice_feats
from rsrgan_amd.io.wave_cmvn import main as cmvn_main
from rsrgan_amd.io.wave_cmvn import wave_cmvn
from rsrgan_amd.io.wave_reader import WaveBatchReader
from rsrgan_amd.train import is_packed
from tests import feat_ref
from tests import mfcc_ref as MR
from tests import wave_ref as R

SMALL_IN = W.WaveSpec(64, 32, 64)
SMALL_LAB = W.MfccSpec(64, 32, 64, num_mel_bins=5, num_ceps=5, sample_rate=16000, low_freq=20, high_freq=0)


def noise(rng, n, sigma=3000):
    return np.clip(np.rint(rng.standard_normal(n) * sigma), -32768, 32767).astype(np.int16)


def kw_of(spec):
    return dict(win=spec.window, N=spec.frame_length, S=spec.frame_shift, P=spec.padded, coef=spec.preemph, M=spec.num_mel_bins,
                C=spec.num_ceps, rate=spec.sample_rate, low=spec.low_freq, high=spec.high_freq, Q=spec.cepstral_lifter)


@pytest.mark.parametrize("spec", [W.MFCC_DEFAULT, W.MfccSpec(num_ceps=0), W.MfccSpec(200, 80, 256, sample_rate=8000, num_mel_bins=23, num_ceps=13),
                                  SMALL_LAB], ids=["mfcc", "fbank", "8k", "small"])
def test_host_route_agrees_with_the_definition(spec):
    rng = np.random.default_rng(3)
    N, S = spec.frame_length, spec.frame_shift
    x = noise(rng, N + 4 * S + 11)
    x[N:N + S] = 0                                                  # (a stretch of digital silence inside)
    m, l, c = MR.stages(x, **kw_of(spec))
    want = c if spec.num_ceps else l
    got = W.mfcc_from_wave(x, spec)
    assert got.dtype == np.float32 and got.shape == want.shape == (5, spec.bins)
    assert (np.abs(got.astype(np.float64) - want) <= R.ulp32(want)).all()
    assert W.mfcc_from_wave(x[:N - 1], spec).shape == (0, spec.bins)
    # float samples on the int16 scale: the same frames
    assert np.array_equal(W.mfcc_from_wave(x.astype(np.float32), spec), got)


def test_default_mel_table():
    seg, w = W.mel_table(W.MFCC_DEFAULT)
    assert seg.dtype == np.int32 and seg.shape == (40, 3) and w.dtype == np.float32
    assert w.shape[0] == 468 == W.MFCC_DEFAULT.nnz and seg[:, 1].min() >= 1 and seg[:, 1].max() == 30
    assert np.array_equal(seg[:, 2], np.concatenate([[0], np.cumsum(seg[:, 1])[:-1]]))          # contiguous, in filter order
    assert (seg[:, 0] >= 0).all() and (seg[:, 0] + seg[:, 1] <= 256).all()                        # the Nyquist bin never enters
    cover = np.zeros(256, int)
    total = np.zeros(256)
    for (a, n, at), (ra, rw) in zip(seg, MR.filters()):
        cover[a:a + n] += 1
        assert a == ra and n == len(rw)
        assert (np.abs(w[at:at + n] - np.asarray(rw)) <= R.ulp32(rw)).all() and (w[at:at + n] > 0).all()
    assert cover.max() == 2
    # between the first and the last centre the two weights of a bin sum to 1
    for a, w64 in W._mel_filters(W.MFCC_DEFAULT):
        total[a:a + w64.shape[0]] += w64
    mel = W._mel(np.arange(256) * 16000 / 512)
    delta = (W._mel(7600.0) - W._mel(20.0)) / 41
    inner = (mel >= W._mel(20.0) + delta) & (mel <= W._mel(20.0) + 40 * delta)
    assert inner.sum() > 200 and np.abs(total[inner] - 1.0).max() <= 1e-12


def test_an_empty_filter_is_kept():
    spec = W.MfccSpec(100, 30, 128, window="hamming", num_mel_bins=40, num_ceps=13, low_freq=20, high_freq=8000)
    seg, w = W.mel_table(spec)
    assert (seg[:, 1] == 0).sum() == 1 and sum(1 for _, f in MR.filters(128, 40, 16000, 20.0, 8000.0) if not f) == 1
    x = noise(np.random.default_rng(4), 100 + 30 * 2)
    fb = W.mfcc_from_wave(x, W.MfccSpec(100, 30, 128, window="hamming", num_mel_bins=40, num_ceps=0, low_freq=20, high_freq=8000))
    j = int(np.flatnonzero(seg[:, 1] == 0)[0])
    assert (fb[:, j] == np.float32(np.log(W.EPS))).all()


def test_dct_table():
    d = W.dct_table(W.MfccSpec(cepstral_lifter=0)).astype(np.float64)
    assert d.shape == (40, 40) and np.abs(d @ d.T - np.eye(40)).max() <= 40 * 2.0 ** -23
    d64 = W._dct64(W.MfccSpec(cepstral_lifter=0))
    assert np.abs(d64 @ d64.T - np.eye(40)).max() <= 1e-13
    lift = W._dct64(W.MFCC_DEFAULT) / d64
    assert np.array_equal(lift[0], np.ones(40))                                                   # row 0 of the lifter is 1
    assert np.abs(lift[11] - 12.0).max() <= 1e-12                                                 # 1 + 11 sin(pi / 2)
    assert (np.abs(W.dct_table(W.MFCC_DEFAULT) - MR.dct()) <= R.ulp32(MR.dct())).all()
    assert W.dct_table(W.MfccSpec(num_ceps=13)).shape == (13, 40) and W.dct_table(W.MfccSpec(num_ceps=0)).shape == (0, 40)


@pytest.mark.parametrize("kw,word", [(dict(num_mel_bins=0), "num_mel_bins"), (dict(num_mel_bins=129), "num_mel_bins"),
                                     (dict(num_ceps=41), "num_ceps"), (dict(num_ceps=-1), "num_ceps"),
                                     (dict(low_freq=-1.0), "low_freq"), (dict(low_freq=8000.0), "low_freq"), (dict(high_freq=8001.0), "high_freq"),
                                     (dict(high_freq=-8000.0), "high_freq"), (dict(cepstral_lifter=-1.0), "cepstral_lifter"),
                                     (dict(window="hann"), "window"), (dict(padded=500), "padded"), (dict(frame_shift=0), "frame_shift"),
                                     (dict(padded=64, frame_length=64, frame_shift=32, low_freq=7000.0, high_freq=7100.0, num_mel_bins=2, num_ceps=2),
                                      "weights"),
                                     (dict(frame_length=2048, frame_shift=700, padded=2048, num_mel_bins=128), "bytes of LDS")])
def test_spec_refusals(kw, word):
    with pytest.raises(ValueError, match=word):
        W.MfccSpec(**kw)


def test_spec_fields():
    s = W.MFCC_DEFAULT
    assert (s.frame_length, s.frame_shift, s.padded, s.preemph, s.window, s.sample_rate) == (400, 160, 512, 0.97, "povey", 16000)
    assert (s.num_mel_bins, s.num_ceps, s.low_freq, s.high_freq, s.cepstral_lifter) == (40, 40, 20.0, -400.0, 22.0)
    assert s.bins == 40 and W.MfccSpec(num_ceps=13).bins == 13 and W.MfccSpec(num_ceps=0).bins == 40 and s.band() == (20.0, 7600.0)
    assert s.lds_bytes() == 31408
    keys = {W.DEFAULT.key(), W.WaveSpec(window="povey").key(), s.key(), W.MfccSpec(num_ceps=13).key(), W.MfccSpec(num_mel_bins=41).key(),
            W.MfccSpec(low_freq=30).key(), W.MfccSpec(high_freq=-300).key(), W.MfccSpec(cepstral_lifter=0).key()}
    assert len(keys) == 8 and s.key() == W.MfccSpec().key()


def test_wave_batch_with_an_mfcc_spec():
    rng = np.random.default_rng(8)
    utts = [noise(rng, 400 + 160 * k + 17) for k in (3, 0, 5)]
    wb = W.pack_wave(utts, None, 0, 0, spec=W.MFCC_DEFAULT)
    assert wb.shape == (3, 6, 40) and wb.dim == 40 and list(np.diff(wb.offsets)) == [4, 1, 6] and is_packed(wb)
    part = wb.rows(1, 3)
    assert part.shape == (2, 6, 40) and part.spec is W.MFCC_DEFAULT and np.array_equal(part.samples, np.concatenate(utts[1:]))
    with pytest.raises(ValueError):
        W.WaveBatch(wb.samples, wb.seg, wb.offsets, (3, 6, 257), spec=W.MFCC_DEFAULT)


FRAMES = [210, 260, 205, 255, 320, 7, 251, 212, 262]            # buckets 0, 1, 0, 1, 2, below, 1, 0, 1


def write_wavs(tmp, tag, frames, rng, spec=SMALL_IN, extra=None, rate=16000):
    """one pair of wav files per utterance (reverberant = clean + noise), `extra[i]` more samples in utterance i's LABEL file; returns
    (inputs wav.scp, labels wav.scp, {utt: (input samples, label samples)})"""
    scp, data = [tmp / (tag + "_in_wav.scp"), tmp / (tag + "_lab_wav.scp")], {}
    lines = [[], []]
    for i, f in enumerate(frames):
        utt = "%s%03d" % (tag, i)
        n = spec.frame_length + (f - 1) * spec.frame_shift + (i * 7) % spec.frame_shift if f else spec.frame_length - 1
        clean = noise(rng, n + (extra or {}).get(i, 0), 2000)
        pair = (np.clip(clean[:n].astype(np.int64) + noise(rng, n, 500), -32768, 32767).astype(np.int16), clean)
        for k, x in enumerate(pair):
            path = tmp / ("%s_%d.wav" % (utt, k))
            with stdwave.open(str(path), "wb") as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
                w.writeframes(x.astype("<i2").tobytes())
            lines[k].append("%s %s\n" % (utt, path))
        data[utt] = pair
    for p, l in zip(scp, lines):
        p.write_text("".join(l))
    return str(scp[0]), str(scp[1]), data


def test_reader_plans_as_the_padded_reader_does(tmp_path):
    rng = np.random.default_rng(12)
    a, b, _ = write_wavs(tmp_path, "tr", FRAMES, rng)
    ark = feat_ref.write_arks(tmp_path, "tr", FRAMES, 3, 2, rng)
    for shuffle, seed in ((True, 5), (True, 99), (False, None)):
        mk = lambda dev: WaveBatchReader(a, b, 2, 1, 1, num_buckets=20, shuffle=shuffle, seed=seed, device_features=dev, input_spec=SMALL_IN,
                                         label_spec=SMALL_LAB)
        want = list(PaddedBatchReader(ark[0], ark[1], 2, 1, 1, num_buckets=20, shuffle=shuffle, seed=seed).plan())
        assert list(mk(False).plan()) == want == list(mk(True).plan())
        assert sum(len(w) for w in want) == len(FRAMES) and any(len(w) == 1 for w in want)           # partial windows at the end


@pytest.mark.parametrize("with_cmvn", [True, False])
def test_reader_items(tmp_path, with_cmvn):
    rng = np.random.default_rng(13)
    frames = [7, 1, 12, 4, 9]
    a, b, data = write_wavs(tmp_path, "cv", frames, rng)
    cmvn = feat_ref.cmvn_for(np.random.default_rng(5), SMALL_IN.bins, SMALL_LAB.bins) if with_cmvn else None
    mk = lambda dev: WaveBatchReader(a, b, 2, 2, 1, cmvn=cmvn, num_buckets=1, shuffle=True, seed=3, device_features=dev, input_spec=SMALL_IN,
                                     label_spec=SMALL_LAB)
    host, dev = list(mk(False)), list(prefetch(mk(True), threads=2))
    assert [len(i[0]) for i in host] == [2, 2, 1] and [i[0] for i in host] == [i[0] for i in dev]
    for item, ditem in zip(host, dev):
        ids, X, Y, L = item
        T = max(frames[int(u[2:])] for u in ids)
        assert X.shape == (len(ids), T, SMALL_IN.bins * 4) and Y.shape == (len(ids), T, SMALL_LAB.bins) and X.dtype == Y.dtype == np.float32
        for r, u in enumerate(ids):
            x = W.lps_from_wave(data[u][0], spec=SMALL_IN).astype(np.float64)
            y = W.mfcc_from_wave(data[u][1], SMALL_LAB).astype(np.float64)
            if cmvn is not None:
                x, y = apply_cmvn(x, y, cmvn)
            n = frames[int(u[2:])]
            assert L[r] == n == x.shape[0] == y.shape[0]
            assert np.array_equal(X[r, :n], splice_feats(x, 2, 1).astype(np.float32)) and not X[r, n:].any()
            assert np.array_equal(Y[r, :n], y.astype(np.float32)) and not Y[r, n:].any()
        # the device route's item: the samples, the same shapes, lengths and statistics
        _, xb, yb, ln = ditem
        assert is_packed(xb) and is_packed(yb) and xb.shape == X.shape and yb.shape == Y.shape and np.array_equal(ln, L) and ln.dtype == np.int32
        assert xb.spec is SMALL_IN and yb.spec is SMALL_LAB and (xb.left, xb.right, yb.left, yb.right) == (2, 1, 0, 0)
        assert np.array_equal(xb.samples, np.concatenate([data[u][0] for u in ids]))
        assert np.array_equal(yb.samples, np.concatenate([data[u][1] for u in ids]))
        if cmvn is not None:
            assert np.array_equal(xb.mean, cmvn["mean_inputs"]) and np.array_equal(yb.stddev, cmvn["stddev_labels"])
        else:
            assert xb.mean is None and yb.stddev is None


def test_reader_refusals(tmp_path):
    rng = np.random.default_rng(14)
    a, b, _ = write_wavs(tmp_path, "mm", [5, 6, 4], rng, extra={1: 32})
    with pytest.raises(ValueError, match="mm001.*6 input frames.*7 label frames"):
        WaveBatchReader(a, b, 2, input_spec=SMALL_IN, label_spec=SMALL_LAB)
    a, b, _ = write_wavs(tmp_path, "nf", [5, 0, 4], rng)
    with pytest.raises(ValueError, match="nf001.*makes no frame"):
        WaveBatchReader(a, b, 2, input_spec=SMALL_IN, label_spec=SMALL_LAB)
    a, b, _ = write_wavs(tmp_path, "ok", [5, 3], rng)
    other = tmp_path / "other.scp"
    other.write_text("".join(reversed(open(b).readlines())))
    with pytest.raises(ValueError, match="same utterance ids"):
        WaveBatchReader(a, str(other), 2, input_spec=SMALL_IN, label_spec=SMALL_LAB)


@pytest.mark.parametrize("mod", ["run_gan_rnn", "run_rnn"])
def test_wav_scp_flags(tmp_path, mod):
    import importlib
    M = importlib.import_module("rsrgan_amd." + mod)
    from rsrgan_amd.run_gan_rnn import check_wav_flags, split_reader
    a, b, _ = write_wavs(tmp_path, "fl", [3, 2], np.random.default_rng(16), spec=W.DEFAULT)
    tr = ["--tr_inputs_wav_scp", a, "--tr_labels_wav_scp", b]
    parse = lambda extra: M.build_parser().parse_args(["--batch_size", "2"] + extra)
    check_wav_flags(parse([]))                                                        # no audio: nothing to check
    FLAGS = parse(tr + ["--cv_inputs_scp", "x.scp", "--cv_labels_scp", "y.scp", "--device_features"])
    check_wav_flags(FLAGS)                                                            # one split from audio, the other from archives
    rd = split_reader(FLAGS, "tr", None, False, None)
    assert isinstance(rd, WaveBatchReader) and rd.device_features and rd.label_spec is W.MFCC_DEFAULT and len(rd) == 2
    assert not split_reader(parse(tr), "tr", None, False, None).device_features
    for extra, word in ((tr[:2], "given together"), (["--cv_labels_wav_scp", b], "given together"),
                        (tr + ["--tr_inputs_scp", "x.scp"], "one kind per split"), (tr + ["--device_decode"], "--device_decode"),
                        (tr + ["--input_dim", "33"], "--input_dim is 33"), (tr + ["--output_dim", "13"], "--output_dim is 13")):
        with pytest.raises(SystemExit, match=word):
            check_wav_flags(parse(extra))
    with pytest.raises(SystemExit, match="makes no frame"):
        a0, b0, _ = write_wavs(tmp_path, "f0", [0], np.random.default_rng(17), spec=W.DEFAULT)
        split_reader(parse(["--tr_inputs_wav_scp", a0, "--tr_labels_wav_scp", b0]), "tr", None, False, None)


def test_wave_cmvn_host_route(tmp_path):
    rng = np.random.default_rng(15)
    a, b, data = write_wavs(tmp_path, "st", [3, 2, 4], rng, spec=W.DEFAULT)
    out = tmp_path / "cmvn.npz"
    stats = cmvn_main(["--inputs_wav_scp", a, "--labels_wav_scp", b, "--out", str(out)])
    x = np.concatenate([W.lps_from_wave(p[0]) for p in data.values()]).astype(np.float64)
    y = np.concatenate([W.mfcc_from_wave(p[1]) for p in data.values()]).astype(np.float64)
    assert x.shape == (9, 257) and y.shape == (9, 40)
    saved = np.load(str(out))
    for key, f in (("inputs", x), ("labels", y)):
        mean = f.sum(0) / f.shape[0]
        std = np.sqrt((f * f).sum(0) / f.shape[0] - mean * mean)
        for name, want in (("mean_", mean), ("stddev_", std)):
            assert saved[name + key].dtype == np.float64 and np.array_equal(saved[name + key], stats[name + key])
            assert np.allclose(saved[name + key], want, rtol=1e-9, atol=1e-12)
        assert np.allclose(saved["stddev_" + key], f.std(0), rtol=1e-6)
    # a dimension without variance is an error here
    flat = tmp_path / "flat.scp"
    path = tmp_path / "flat.wav"
    with stdwave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.full(400 + 160, 1000, "<i2").tobytes())
    flat.write_text("flat %s\n" % path)
    with pytest.raises(ValueError, match="no variance"):
        wave_cmvn(str(flat), str(flat))
