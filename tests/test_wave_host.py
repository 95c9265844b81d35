"""Host side of the waveform front end (no GPU): rsrgan_amd/io/wave.py's host route against the frame-by-frame float64 definition of
tests/wave_ref.py and against known answers, the frame count at its edges, pack_wave's tables, the wav and scp readers through files,
and push_audio on the host route: audio cut into pushes of any size yields exactly what push yields for the frames of the whole
utterance."""
import math
import wave

import numpy as np
import pytest

from rsrgan_amd.io import wave as W
from tests import wave_ref as R
from tests.helpers import rand_params, small_cfg

LOG_EPS = math.log(R.EPS)


def _noise(n, seed=0, sigma=3000.0):
    return np.clip(np.rint(np.random.default_rng(seed).standard_normal(n) * sigma), -32768, 32767).astype(np.int16)


# ---- the host route is the definition ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", ["hamming", "povey"])
@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_host_route_equals_the_definition_to_one_ulp(window, dtype):
    x = _noise(400 + 160 * 6 + 37, seed=3).astype(dtype)
    got = W.lps_from_wave(x, window=window)
    want = R.lps(x, window)
    assert got.dtype == np.float32 and got.shape == want.shape == (7, 257)
    assert (np.abs(got.astype(np.float64) - want) <= R.ulp32(want)).all(), float(np.abs(got - want).max())


def test_other_framings():
    x = _noise(3000, seed=4)
    spec = W.WaveSpec(frame_length=200, frame_shift=80, padded=256, preemph=0.5, window="povey")
    got = W.lps_from_wave(x, spec=spec)
    want = R.lps(x, "povey", N=200, S=80, P=256, coef=0.5)
    assert got.shape == want.shape == (1 + (3000 - 200) // 80, 129)
    assert (np.abs(got.astype(np.float64) - want) <= R.ulp32(want)).all()
    for bad in (dict(padded=500), dict(padded=32), dict(padded=4096), dict(frame_length=600), dict(frame_shift=0), dict(frame_shift=401),
                dict(preemph=1.5), dict(preemph=-0.1), dict(window="hann")):
        with pytest.raises(ValueError):
            W.WaveSpec(**bad)


def test_tables():
    w = W.window_table("hamming", 400)
    assert w.dtype == np.float64 and np.abs(w - R.window("hamming")).max() < 1e-15 and abs(w[0] - 0.08) < 1e-15
    assert np.abs(W.window_table("povey", 400) - R.window("povey")).max() < 1e-15
    t = W.twiddle_table(512)
    assert t.dtype == np.float32 and t.shape == (256, 2) and t.flags.c_contiguous
    assert t[0].tolist() == [1.0, 0.0] and t[128, 1] == -1.0 and abs(t[128, 0]) < 1e-7
    j = np.arange(256)
    assert np.abs(t[:, 0] - np.cos(2 * np.pi * j / 512)).max() < 6e-8 and np.abs(t[:, 1] + np.sin(2 * np.pi * j / 512)).max() < 6e-8


# ---- known answers ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [0, 1000, -32768])
def test_silence_and_a_constant_give_log_eps_in_every_bin(value):
    out = W.lps_from_wave(np.full(560, value, np.int16))
    assert out.shape == (2, 257)
    assert (out == np.float32(LOG_EPS)).all()


def test_an_impulse_gives_the_closed_form():
    """x = A at sample i0: after the mean is removed v = A (delta - 1 / N); pre-emphasis makes the pair A (delta[i0] - c delta[i0 + 1]) on a
    constant -(A / N)(1 - c); windowed, X_k = A (w[i0] z^i0 - c w[i0 + 1] z^(i0 + 1)) - (A / N)(1 - c) sum_i w[i] z^i, z = exp(-2 pi i k / P)"""
    A, i0, c, N, P = 12000.0, 137, 0.97, 400, 512
    x = np.zeros(400, np.int16)
    x[i0] = int(A)
    out = W.lps_from_wave(x).astype(np.float64)[0]
    w = R.window("hamming")
    k = np.arange(257)
    z = lambda i: np.exp(-2j * np.pi * ((k * i) % P) / P)
    X = A * (w[i0] * z(i0) - c * w[i0 + 1] * z(i0 + 1)) - (A / N) * (1 - c) * sum(w[i] * z(i) for i in range(N))
    want = np.log(np.maximum(np.abs(X) ** 2, R.EPS))
    want[0] = math.log(A * A * (1 - 1 / N) ** 2 + (N - 1) * (A / N) ** 2)
    assert np.abs(out - want).max() <= 2 * R.ulp32(want).max(), float(np.abs(out - want).max())


@pytest.mark.parametrize("k0", [3, 40, 200])
def test_a_bin_centred_sine_peaks_in_its_bin(k0):
    i = np.arange(400 + 160)
    x = np.rint(20000 * np.sin(2 * np.pi * k0 * i / 512)).astype(np.int16)
    out = W.lps_from_wave(x)
    assert (out[:, 1:].argmax(1) + 1 == k0).all()
    far = np.abs(np.arange(257) - k0) > 8
    far[0] = False
    assert (out[:, k0:k0 + 1] - out[:, far] > math.log(1e4)).all()      # the Hamming side lobes are 43 dB and more below


@pytest.mark.parametrize("n,frames", [(0, 0), (399, 0), (400, 1), (559, 1), (560, 2), (16000, 98)])
def test_frame_counts(n, frames):
    assert W.num_frames(n) == R.frame_count(n) == frames
    assert W.lps_from_wave(np.zeros(n, np.int16)).shape == (frames, 257)


# ---- pack_wave ----------------------------------------------------------------------------------------------------------------------------

def test_pack_wave_tables():
    utts = [_noise(n, seed=n) for n in (1000, 399, 400, 2000)]
    wb = W.pack_wave(utts, left=2, right=1)
    assert wb.samples.dtype == np.int16 and wb.kind == W.KIND_INT16 and wb.samples.shape == (3799,)
    assert wb.seg.dtype == np.int64 and wb.seg.tolist() == [[0, 1000], [1000, 399], [1399, 400], [1799, 2000]]
    assert wb.offsets.dtype == np.int32 and wb.offsets.tolist() == [0, 4, 4, 5, 16]
    assert wb.shape == (4, 11, 257 * 4) and wb.dim == 257 and len(wb) == 4
    assert wb.lengths().tolist() == [4, 0, 1, 11]
    assert wb.nbytes() == 3799 * 2 + 4 * 16 + 5 * 4
    for b, u in enumerate(utts):
        a, n = wb.seg[b]
        assert np.array_equal(wb.samples[a:a + n], u)
    assert W.pack_wave(utts, T=7).shape == (4, 7, 257) and W.pack_wave(utts, T=7).lengths().tolist() == [4, 0, 1, 7]
    # one float utterance makes the blob float32, on the same scale
    wf = W.pack_wave([utts[0], utts[3].astype(np.float64)])
    assert wf.samples.dtype == np.float32 and wf.kind == W.KIND_FLOAT32 and np.array_equal(wf.samples[:1000], utts[0].astype(np.float32))
    # a shard: its own samples, tables rebased
    sh = wb.rows(2, 4)
    assert sh.seg.tolist() == [[0, 400], [400, 2000]] and sh.offsets.tolist() == [0, 1, 12] and sh.shape == (2, 11, 257 * 4)
    assert np.array_equal(sh.samples, np.concatenate(utts[2:]))
    assert (sh.left, sh.right) == (2, 1)


def test_wave_batch_refuses_what_the_device_cannot_check():
    wb = W.pack_wave([_noise(1000), _noise(600)])
    good = dict(samples=wb.samples, seg=wb.seg, offsets=wb.offsets, shape=wb.shape)
    W.WaveBatch(**good)
    seg = wb.seg.copy(); seg[1, 1] = 601
    off = wb.offsets.copy(); off[2] += 1
    for bad in (dict(seg=seg), dict(offsets=off), dict(samples=wb.samples.astype(np.float64)), dict(offsets=wb.offsets.astype(np.int64)),
                dict(seg=wb.seg.astype(np.int32)), dict(shape=(2, 4, 256)), dict(shape=(3, 4, 257))):
        with pytest.raises(ValueError):
            W.WaveBatch(**dict(good, **bad))
    with pytest.raises(ValueError):
        W.pack_wave([np.zeros((10, 2), np.int16)])
    with pytest.raises(ValueError):
        W.pack_wave([])


# ---- files --------------------------------------------------------------------------------------------------------------------------------

def _write_wav(path, data, rate=16000, width=2):
    data = np.asarray(data)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1 if data.ndim == 1 else data.shape[1])
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(data.astype("<i2" if width == 2 else np.uint8).tobytes())


def test_wav_round_trip(tmp_path):
    x = _noise(1234, seed=9)
    _write_wav(tmp_path / "a.wav", x)
    got = W.read_wav(tmp_path / "a.wav")
    assert got.dtype == np.int16 and np.array_equal(got, x)
    st = np.stack([x, -x // 2], 1).astype(np.int16)
    _write_wav(tmp_path / "st.wav", st)
    assert np.array_equal(W.read_wav(tmp_path / "st.wav"), st[:, 0]) and np.array_equal(W.read_wav(tmp_path / "st.wav", channel=1), st[:, 1])
    with pytest.raises(ValueError, match="channel 2"):
        W.read_wav(tmp_path / "st.wav", channel=2)
    _write_wav(tmp_path / "r8.wav", x, rate=8000)
    with pytest.raises(ValueError, match="8000 Hz, expected 16000"):
        W.read_wav(tmp_path / "r8.wav")
    assert np.array_equal(W.read_wav(tmp_path / "r8.wav", sample_rate=8000), x)
    _write_wav(tmp_path / "w1.wav", np.abs(x) % 255, width=1)
    with pytest.raises(ValueError, match="8-bit"):
        W.read_wav(tmp_path / "w1.wav")


def test_scp_round_trip(tmp_path):
    (tmp_path / "wav.scp").write_text("utt1 %s/a.wav\n\nutt2\t%s/b c.wav  \n" % (tmp_path, tmp_path))
    assert W.read_wav_scp(tmp_path / "wav.scp") == [("utt1", "%s/a.wav" % tmp_path), ("utt2", "%s/b c.wav" % tmp_path)]
    (tmp_path / "piped.scp").write_text("utt1 %s/a.wav\nutt2 sox x.flac -t wav - |\n" % tmp_path)
    with pytest.raises(ValueError, match="piped entry"):
        W.read_wav_scp(tmp_path / "piped.scp")
    (tmp_path / "short.scp").write_text("utt1\n")
    with pytest.raises(ValueError, match="expected `utt path`"):
        W.read_wav_scp(tmp_path / "short.scp")


# ---- --decode --wav_scp, host route ------------------------------------------------------------------------------------------------------

def test_decode_wav_scp_writes_what_the_frames_archive_gives(tmp_path):
    """run_gan_rnn --decode --wav_scp on a stand-in model: the matrices of the same command on an archive of lps_from_wave's frames; with
    --decode_push the live path is driven by pushes of samples"""
    from rsrgan_amd import run_gan_rnn as G
    from rsrgan_amd.io import ArkReader, ArkWriter
    from tests import stream_ref as SR
    left, right = 1, 1
    utts = [_noise(n, seed=n) for n in (400 + 160 * 5, 400, 400 + 160 * 12 + 80)]
    w = ArkWriter(str(tmp_path / "te.scp"))
    lines = []
    for i, u in enumerate(utts):
        _write_wav(tmp_path / ("u%d.wav" % i), u)
        lines.append("utt%d %s/u%d.wav\n" % (i, tmp_path, i))
        w.write_next_utt(str(tmp_path / "te.ark"), "utt%d" % i, W.lps_from_wave(u))
    w.close()
    (tmp_path / "wav.scp").write_text("".join(lines))
    rng = np.random.default_rng(2)
    np.savez(tmp_path / "train_cmvn.npz", mean_inputs=rng.standard_normal(257) + 20, stddev_inputs=rng.uniform(2, 4, 257),
             mean_labels=rng.standard_normal(4), stddev_labels=rng.uniform(0.5, 2, 4))
    cfg = small_cfg("lstm", input_dim=257 * (left + 1 + right), output_dim=4)
    g = {k: np.asarray(v, np.float64) for k, v in rand_params(cfg, 13)[0].items()}
    base = ["--decode", "--data_dir", str(tmp_path), "--input_dim", "257", "--output_dim", "4", "--left_context", str(left),
            "--right_context", str(right)]

    def decode(name, extra, batch=1, cap=3000):
        F, _ = G.build_parser().parse_known_args(base + ["--save_dir", str(tmp_path / name)] + extra)
        m = SR.RefStreamModel(cfg, g, batch, cap, save_dir=F.save_dir)
        rd = ArkReader()
        rd(G.decode(F, model_factory=lambda: m, log=lambda s: None))
        return rd.utt_ids, [rd.read_utt_data_from_index(i) for i in range(len(rd.utt_ids))]

    ids0, ark = decode("a", ["--test_inputs_scp", str(tmp_path / "te.scp")])
    ids1, wav = decode("b", ["--wav_scp", str(tmp_path / "wav.scp")])
    ids2, live = decode("c", ["--wav_scp", str(tmp_path / "wav.scp"), "--decode_chunk", "4", "--decode_streams", "2", "--decode_push", "3"], 2, 4)
    assert ids0 == ids1 == ids2 == ["utt0", "utt1", "utt2"]
    for u, a, b, c in zip(utts, ark, wav, live):
        assert a.shape == b.shape == c.shape == (W.num_frames(u.shape[0]), 4)
        assert np.array_equal(a, b)
        assert np.abs(a.astype(np.float64) - c).max() <= 1e-6 * max(1.0, np.abs(a).max())
    for extra, word in ((["--wav_scp", str(tmp_path / "wav.scp"), "--input_dim", "40"], "257 bins"),
                        (["--wav_scp", str(tmp_path / "wav.scp"), "--device_decode"], "--device_decode")):
        with pytest.raises(SystemExit, match=word):
            decode("d", extra)
    (tmp_path / "short.scp").write_text(lines[0])
    _write_wav(tmp_path / "u0.wav", utts[0][:399])
    with pytest.raises(SystemExit, match="make no frame"):
        decode("e", ["--wav_scp", str(tmp_path / "short.scp")])


# ---- push_audio, host route --------------------------------------------------------------------------------------------------------------

def _bank(left, right, streams=2, chunk=4):
    from rsrgan_amd.stream import StreamBank
    from tests import stream_ref as SR
    cfg = small_cfg("lstm", input_dim=257 * (left + 1 + right), output_dim=4)
    g = {k: np.asarray(v, np.float64) for k, v in rand_params(cfg, 11)[0].items()}
    model = SR.RefStreamModel(cfg, g, streams, 8)
    rng = np.random.default_rng(5)
    cmvn = dict(mean_inputs=rng.standard_normal(257) + 10, stddev_inputs=rng.uniform(0.5, 2.0, 257),
                mean_labels=rng.standard_normal(4), stddev_labels=rng.uniform(0.5, 2.0, 4))
    return StreamBank(model, cmvn, left, right, chunk=chunk, streams=streams)


@pytest.mark.parametrize("push", [1, 159, 160, 161, 1000])
def test_push_audio_yields_what_push_yields_for_the_whole_utterance(push):
    """the same frames arrive in the same pushes on both banks -- on one as audio, on the other as slices of lps_from_wave of the WHOLE
    utterance -- so the forward calls are the same and the outputs equal bit for bit: cutting the audio changes no frame"""
    n = 400 + 160 * 9 + 77 if push > 1 else 400 + 160 * 2 + 5
    x = _noise(n, seed=push)
    whole = W.lps_from_wave(x)
    F = whole.shape[0]
    a, b = _bank(2, 1), _bank(2, 1)
    got, want, seen = [], [], 0
    for lo in range(0, n, push):
        got.append(a.push_audio({1: x[lo:lo + push]})[1])
        have = W.num_frames(min(lo + push, n))
        want.append(b.push({1: whole[seen:have]})[1])
        seen = have
        assert a._pcm[1].shape[0] < 400 and a._pcm[1].shape[0] == min(lo + push, n) - (have * 160 if have else 0)
    got.append(a.flush([1])[1]); want.append(b.flush([1])[1])
    assert a._pcm[1] is None                                             # flush drops the samples of no complete frame
    got, want = np.concatenate(got, 0), np.concatenate(want, 0)
    assert got.shape == want.shape == (F, 4) and got.dtype == np.float64
    assert got.tobytes() == want.tobytes()
    assert len(a.model.calls) == len(b.model.calls) > 0 and a.counters == b.counters


def test_push_audio_rows_side_by_side_and_reset():
    from rsrgan_amd.stream import StreamBank, StreamEnhancer, decode_live, decode_live_audio
    utts = [_noise(n, seed=n) for n in (2000, 399, 1500, 0, 900)]
    ref = list(decode_live(_bank(1, 1), [W.lps_from_wave(u) for u in utts], 3))
    got = list(decode_live_audio(_bank(1, 1), utts, 3 * 160))
    assert [g.shape for g in got] == [r.shape for r in ref] == [(W.num_frames(u.shape[0]), 4) for u in utts]
    for g, r in zip(got, ref):
        assert np.abs(g - r).max() <= 1e-12 if g.size else True
    bank = _bank(0, 0)
    bank.push_audio({0: utts[0][:300]})
    assert bank._pcm[0].shape[0] == 300
    bank.reset([0])
    assert bank._pcm[0] is None
    with pytest.raises(ValueError):
        bank.push_audio({0: np.zeros((4, 2), np.int16)})
    with pytest.raises(ValueError):
        bank.push_audio({5: utts[0]})
    with pytest.raises(ValueError):
        list(decode_live_audio(bank, utts, 0))
    # int16 and float samples of one row meet: the row goes on in float32, the same frames
    a, b = _bank(0, 0), _bank(0, 0)
    ya = np.concatenate([a.push_audio({0: utts[0][:700]})[0], a.push_audio({0: utts[0][700:].astype(np.float64)})[0], a.flush([0])[0]], 0)
    yb = np.concatenate([b.push_audio({0: utts[0]})[0], b.flush([0])[0]], 0)
    assert ya.shape == yb.shape and np.abs(ya - yb).max() <= 1e-12
    # the enhancer's host path
    enh = StreamEnhancer(a.model, a.cmvn, 0, 0, chunk=4)
    ye = np.concatenate([enh.push_audio(utts[0][:333]), enh.push_audio(utts[0][333:]), enh.flush()], 0)
    assert ye.shape == yb.shape and np.abs(ye - yb).max() <= 1e-12 and enh._pcm is None
