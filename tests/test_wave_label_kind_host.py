"""LPS targets from audio on the host: io.wave_reader.WaveBatchReader with an LPS label spec yields lps_from_wave of the label audio
(the device route already dispatches on the spec); --label_kind on the two sequence recipes and on io.wave_cmvn; the refusals of
--wav_out.  No device is needed."""
import importlib

import numpy as np
import pytest

from rsrgan_amd.io import wave as W
from rsrgan_amd.io.features import apply_cmvn, splice_feats
from rsrgan_amd.io.wave_cmvn import main as cmvn_main
from rsrgan_amd.io.wave_reader import WaveBatchReader
from tests import feat_ref
from tests.test_mfcc_host import SMALL_IN, write_wavs

SMALL_LPS = W.WaveSpec(SMALL_IN.frame_length, SMALL_IN.frame_shift, SMALL_IN.padded, 0.9, "povey")      # (another framing than the inputs')


@pytest.mark.parametrize("with_cmvn", [True, False])
def test_reader_yields_lps_labels(tmp_path, with_cmvn):
    rng = np.random.default_rng(21)
    frames = [6, 2, 9]
    a, b, data = write_wavs(tmp_path, "lk", frames, rng)
    cmvn = feat_ref.cmvn_for(np.random.default_rng(6), SMALL_IN.bins, SMALL_LPS.bins) if with_cmvn else None
    mk = lambda dev: WaveBatchReader(a, b, 2, 1, 1, cmvn=cmvn, num_buckets=1, shuffle=False, device_features=dev, input_spec=SMALL_IN,
                                     label_spec=SMALL_LPS)
    items = list(mk(False))
    assert [len(i[0]) for i in items] == [2, 1]
    for ids, X, Y, L in items:
        assert Y.shape[2] == SMALL_LPS.bins and Y.dtype == np.float32
        for r, u in enumerate(ids):
            x = W.lps_from_wave(data[u][0], spec=SMALL_IN).astype(np.float64)
            y = W.lps_from_wave(data[u][1], spec=SMALL_LPS).astype(np.float64)
            if cmvn is not None:
                x, y = apply_cmvn(x, y, cmvn)
            n = int(L[r])
            assert n == y.shape[0]
            assert np.array_equal(Y[r, :n], y.astype(np.float32)) and not Y[r, n:].any()
            assert np.array_equal(X[r, :n], splice_feats(x, 1, 1).astype(np.float32))
    # the device route's item carries the label samples under the LPS spec
    _, xb, yb, _ = next(iter(mk(True)))
    assert yb.spec is SMALL_LPS and yb.dim == SMALL_LPS.bins and not hasattr(yb.spec, "num_mel_bins")


@pytest.mark.parametrize("mod", ["run_gan_rnn", "run_rnn"])
def test_label_kind_flags(tmp_path, mod):
    M = importlib.import_module("rsrgan_amd." + mod)
    from rsrgan_amd.run_gan_rnn import check_wav_flags, label_spec, split_reader
    a, b, data = write_wavs(tmp_path, "fk", [3, 2], np.random.default_rng(22), spec=W.DEFAULT)
    tr = ["--tr_inputs_wav_scp", a, "--tr_labels_wav_scp", b]
    parse = lambda extra: M.build_parser().parse_args(["--batch_size", "2"] + extra)
    assert parse([]).label_kind == "mfcc" and parse([]).wav_out is None
    with pytest.raises(SystemExit):
        parse(["--label_kind", "fbank"])
    # lps: 257 / 257 passes, the default --output_dim 40 does not
    FLAGS = parse(tr + ["--label_kind", "lps", "--output_dim", "257"])
    check_wav_flags(FLAGS)
    assert label_spec(FLAGS) is W.DEFAULT
    with pytest.raises(SystemExit, match="label frames of 257; --input_dim is 257, --output_dim is 40"):
        check_wav_flags(parse(tr + ["--label_kind", "lps"]))
    rd = split_reader(FLAGS, "tr", None, False, None)
    assert rd.label_spec is W.DEFAULT
    ids, X, Y, L = next(iter(rd))
    assert Y.shape == (2, 3, 257)
    assert np.array_equal(Y[0], W.lps_from_wave(data[ids[0]][1]))
    # mfcc: the present verdicts, word for word
    check_wav_flags(parse(tr))
    check_wav_flags(parse(tr + ["--label_kind", "mfcc"]))
    assert split_reader(parse(tr), "tr", None, False, None).label_spec is W.MFCC_DEFAULT
    with pytest.raises(SystemExit) as e:
        check_wav_flags(parse(tr + ["--output_dim", "257"]))
    assert str(e.value) == "--*_wav_scp makes input frames of 257 bins and label frames of 40; --input_dim is 257, --output_dim is 257"
    with pytest.raises(SystemExit, match="--output_dim is 13"):
        check_wav_flags(parse(tr + ["--output_dim", "13"]))


@pytest.mark.parametrize("mod", ["run_gan_rnn", "run_rnn"])
def test_wav_out_refusals(tmp_path, mod):
    """the refusals come before a model is built: a factory that must not be called"""
    M = importlib.import_module("rsrgan_amd." + mod)
    a, _, _ = write_wavs(tmp_path, "wo", [3], np.random.default_rng(23), spec=W.DEFAULT)

    def never():
        raise AssertionError("a model was built")

    base = ["--decode", "--save_dir", str(tmp_path / "exp"), "--wav_out", str(tmp_path / "wavs")]
    parse = lambda extra: M.build_parser().parse_args(base + extra)
    for extra in (["--test_inputs_scp", "x.scp", "--output_dim", "257"], ["--wav_scp", a, "--output_dim", "40"], ["--wav_scp", a]):
        with pytest.raises(SystemExit) as e:
            M.decode(parse(extra), model_factory=never)
        assert "--wav_out" in str(e.value) and "--wav_scp" in str(e.value) and "--output_dim" in str(e.value)
    with pytest.raises(SystemExit, match="--wav_out does not go with --decode_push"):
        M.decode(parse(["--wav_scp", a, "--output_dim", "257", "--decode_chunk", "10", "--decode_push", "5"]), model_factory=never)
    assert not (tmp_path / "wavs").exists()


def test_wave_cmvn_label_kind(tmp_path):
    a, b, data = write_wavs(tmp_path, "ck", [3, 2, 4], np.random.default_rng(24), spec=W.DEFAULT)
    stats = cmvn_main(["--inputs_wav_scp", a, "--labels_wav_scp", b, "--out", str(tmp_path / "c.npz"), "--label_kind", "lps"])
    f = np.concatenate([W.lps_from_wave(data[u][1]).astype(np.float64) for u in sorted(data)], 0)
    assert stats["mean_labels"].shape == (257,) and np.allclose(stats["mean_labels"], f.mean(0), rtol=1e-12, atol=0)
    assert np.allclose(stats["stddev_labels"], f.std(0), rtol=1e-9, atol=0)
    assert cmvn_main(["--inputs_wav_scp", a, "--labels_wav_scp", b, "--out", str(tmp_path / "d.npz")])["mean_labels"].shape == (40,)
