"""The host side of the simulation (rsrgan_amd/io/reverb.py): the float64 route against tests/reverb_ref.py, the table columns against a loop,
the draws, WaveBatchReader(simulate=...) and the refusals of the command lines.  No device is needed."""
import threading
import wave

import numpy as np
import pytest

from rsrgan_amd import run_gan_rnn, run_rnn
from rsrgan_amd.io import reverb as RV
from rsrgan_amd.io import wave_cmvn
from rsrgan_amd.io.wave_reader import WaveBatchReader
from tests import reverb_ref as RR


def write_wav(path, x, rate=16000):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(rate)
        f.writeframes(np.asarray(x, "<i2").tobytes())


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """six clean utterances of 0.2 .. 0.4 s, three 103-tap RIRs (.npy), two noises"""
    d = tmp_path_factory.mktemp("reverb")
    rng = np.random.default_rng(3)
    lab, rir, noi = [], [], []
    for i, n in enumerate((3300, 4100, 5000, 6400, 3700, 4800)):
        write_wav(d / ("u%d.wav" % i), np.clip(np.rint(rng.standard_normal(n) * 2500), -32768, 32767))
        lab.append("utt%d %s" % (i, d / ("u%d.wav" % i)))
    for i, q in enumerate((0, 40, 102)):
        h = rng.standard_normal(103) * 0.2 * np.exp(-np.arange(103) / 30.0)
        h[q] = 1.5
        np.save(d / ("r%d.npy" % i), h.astype(np.float32))
        rir.append("rir%d %s" % (i, d / ("r%d.npy" % i)))
    for i, n in enumerate((900, 2500)):
        write_wav(d / ("n%d.wav" % i), np.rint(rng.standard_normal(n) * 700))
        noi.append("noise%d %s" % (i, d / ("n%d.wav" % i)))
    for name, lines in (("labels.scp", lab), ("rir.scp", rir), ("noise.scp", noi)):
        (d / name).write_text("\n".join(lines) + "\n")
    return d


CONFIGS = [dict(n=227, L=103, q=40, noise=50, s=3, m=200), dict(n=69, L=33, q=0, noise=None, s=0, m=0), dict(n=500, L=1, q=0, noise=300, s=100, m=400),
           dict(n=64, L=None, q=0, noise=50, s=0, m=64), dict(n=1000, L=400, q=399, noise=120, s=5000, m=10), dict(n=31, L=103, q=60, noise=40, s=0, m=0)]


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("shift,normalize", [(True, True), (False, False), (True, False), (False, True)])
def test_reverberate_against_the_reference(cfg, shift, normalize):
    rng = np.random.default_rng(cfg["n"])
    x = np.rint(rng.standard_normal(cfg["n"]) * 3000).astype(np.int16)
    h = None
    if cfg["L"]:
        h = (rng.standard_normal(cfg["L"]) * 0.3).astype(np.float32)
        h[cfg["q"]] = 2.0
    v = (rng.standard_normal(cfg["noise"]) * 500).astype(np.float32) if cfg["noise"] else None
    rate = 1000
    want, (c, g) = RR.reverb_ref(x, h, RR.rir_columns(h, rate) if h is not None else None, v, RR.noise_power(v) if v is not None else None,
                                 cfg["s"], cfg["m"], 7.0, shift, normalize)
    got, (c2, g2) = RV.reverberate(x, h, v, None, cfg["s"], cfg["m"], 7.0, shift, normalize, sample_rate=rate, gains=True)
    assert got.shape == want.shape and got.dtype == np.float64
    assert RR.figure(got, want) <= 1e-9
    assert abs(c2 - c) <= 1e-12 * c and abs(g2 - g) <= 1e-12 * max(g, 1e-300)


def test_table_columns_against_a_loop():
    rng = np.random.default_rng(5)
    rirs = [rng.standard_normal(L).astype(np.float32) for L in (1, 17, 900, 103)]
    rirs[1][[3, 9]] = 5.0                                              # a tie: the FIRST maximum
    rirs[2][850] = 9.0                                                 # e1 is cut at L
    taps, seg = RV.rir_table(rirs, 16000)
    assert taps.dtype == np.float32 and seg.dtype == np.int64 and seg.shape == (4, 5)
    at = 0
    for r, h in enumerate(rirs):
        q, e0, e1 = RR.rir_columns(h, 16000)
        assert tuple(seg[r]) == (at, h.shape[0], q, e0, e1)
        assert np.array_equal(taps[at:at + h.shape[0]], h)
        at += h.shape[0]
    assert seg[1, 2] == 3 and tuple(seg[2, 2:]) == (850, 834, 900)
    noises = [rng.standard_normal(n).astype(np.float32) * 100 for n in (40, 1000)] + [np.zeros(8, np.float32)]
    flat, nseg, pw = RV.noise_table(noises)
    assert nseg.dtype == np.int64 and pw.dtype == np.float32 and nseg.tolist() == [[0, 40], [40, 1000], [1040, 8]]
    for i, v in enumerate(noises):
        acc = 0.0
        for t in v:
            acc += float(t) * float(t)
        assert pw[i] == np.float32(acc / v.shape[0]) or abs(float(pw[i]) - acc / v.shape[0]) <= 1e-7 * acc / v.shape[0]
    assert pw[2] == 0.0 and np.array_equal(flat[40:1040], noises[1])


def test_draw_is_a_function_of_seed_epoch_and_index(corpus):
    sim = RV.ReverbSim(str(corpus / "rir.scp"), str(corpus / "noise.scp"), RV.ReverbSpec(snr=(5, 20)), seed=11)
    first = {(e, i): sim.draw(i, 4000 + i, epoch=e) for e in range(3) for i in range(50)}
    # any order, any thread, a second object: the same draws
    other = RV.ReverbSim(str(corpus / "rir.scp"), str(corpus / "noise.scp"), RV.ReverbSpec(snr=(5, 20)), seed=11)
    got = {}

    def work(keys):
        for e, i in keys:
            got[e, i] = other.draw(i, 4000 + i, epoch=e)
    keys = sorted(first, reverse=True)
    ts = [threading.Thread(target=work, args=(keys[k::4],)) for k in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got == first
    sim.set_epoch(2)
    assert all(sim.draw(i, 4000 + i) == first[2, i] for i in range(50))
    # epochs, indices and seeds give other draws; everything lies in range
    assert len({first[0, i][:2] for i in range(50)}) > 3
    assert sum(first[0, i] != first[1, i] for i in range(50)) > 40
    assert sum(RV.draw(12, 0, i, 4000 + i, 3, [103] * 3, 2, sim.spec) != first[0, i] for i in range(50)) > 40
    for (e, i), (r, v, s, m, snr) in first.items():
        assert 0 <= r < 3 and 0 <= v < 2 and 0 <= s < 4000 + i and s + m == 4000 + i + 103 - 1 and 5.0 <= snr <= 20.0
    none = RV.draw(11, 0, 7, 4000, 3, [103] * 3, 0, sim.spec)
    assert none[1] == -1 and none[3] == 0
    assert none[0] == RV.draw(11, 0, 7, 4000, 3, [103] * 3, 2, sim.spec)[0]            # (the RIR does not depend on whether noises exist)


def test_reader_with_simulate(corpus):
    lab, rir, noi = (str(corpus / k) for k in ("labels.scp", "rir.scp", "noise.scp"))
    mk = lambda **kw: WaveBatchReader(None, lab, 2, 1, 1, shuffle=True, seed=5, simulate=RV.ReverbSim(rir, noi, RV.ReverbSpec(), seed=3), **kw)
    plain = WaveBatchReader(lab, lab, 2, 1, 1, shuffle=True, seed=5)
    host, dev = mk(), mk(device_features=True)
    plan = list(plain.plan())
    assert list(host.plan()) == plan == list(dev.plan()) and host._nframes == plain._nframes
    # host route: the items are padded batches of the reverberated audio; any materialize order gives the same items
    fwd = [host.materialize(b) for b in plan]
    bwd = [host.materialize(b) for b in reversed(plan)][::-1]
    clean = [plain.materialize(b) for b in plan]
    for a, b, c in zip(fwd, bwd, clean):
        assert a[0] == b[0] == c[0]
        for k in (1, 2, 3):
            assert np.array_equal(a[k], b[k])
        assert a[1].shape == c[1].shape and np.array_equal(a[2], c[2]) and np.array_equal(a[3], c[3])       # equal frame counts, the same labels
        assert not np.array_equal(a[1], c[1])                                                                 # (the inputs are reverberant)
    # the input frames are lps_from_wave of io.reverb.reverberate with the utterance's draw
    from rsrgan_amd.io.wave import lps_from_wave, read_wav
    i = plan[0][0]
    x = read_wav(host.labels[i][1])
    want = lps_from_wave(host.simulate.apply(x, host.simulate.draw(i, x.shape[0])))
    assert np.array_equal(fwd[0][1][0, :want.shape[0], 257:514], want)
    # another epoch: other rooms, the same labels
    host.set_epoch(1)
    again = host.materialize(plan[0])
    assert not np.array_equal(again[1], fwd[0][1]) and np.array_equal(again[2], fwd[0][2])
    # device route: clean samples + the plan
    item = dev.materialize(plan[0])
    X, Y = item[1], item[2]
    assert X.plan is not None and Y.plan is None and len(X.plan) == 2 and X.samples.dtype == np.int16
    assert np.array_equal(X.samples, Y.samples) and np.array_equal(X.offsets, Y.offsets)
    for k, i in enumerate(plan[0]):
        r, v, s, m, snr = dev.simulate.draw(i, int(X.seg[k, 1]))
        assert tuple(X.plan.sel[k]) == (r, v, s, m) and X.plan.snr[k] == np.float32(snr)
    half = X.rows(1, 2)
    assert len(half.plan) == 1 and np.array_equal(half.plan.sel[0], X.plan.sel[1])
    item2 = [dev.materialize(b) for b in reversed(plan)][-1]
    assert np.array_equal(item2[1].plan.sel, X.plan.sel) and np.array_equal(item2[1].plan.snr, X.plan.snr)


def test_reader_refusals(corpus):
    lab, rir = str(corpus / "labels.scp"), str(corpus / "rir.scp")
    sim = RV.ReverbSim(rir)
    with pytest.raises(ValueError, match="exactly one"):
        WaveBatchReader(lab, lab, 2, simulate=sim)
    with pytest.raises(ValueError, match="exactly one"):
        WaveBatchReader(None, lab, 2)
    with pytest.raises(ValueError, match="must shift"):
        WaveBatchReader(None, lab, 2, simulate=RV.ReverbSim(rir, spec=RV.ReverbSpec(shift=False)))
    for kw in (dict(fft=100), dict(fft=4096), dict(snr=(20, 5)), dict(noise_prob=1.5), dict(sample_rate=0)):
        with pytest.raises(ValueError):
            RV.ReverbSpec(**kw)
    (corpus / "empty.scp").write_text("")
    with pytest.raises(ValueError, match="lists no files"):
        RV.ReverbSim(str(corpus / "empty.scp"))


def _flags(parser, corpus, *extra):
    lab = str(corpus / "labels.scp")
    return parser.parse_args(["--input_dim", "257", "--output_dim", "40"] + [a.replace("LAB", lab).replace("RIR", str(corpus / "rir.scp"))
                                                                            .replace("NOI", str(corpus / "noise.scp")) for a in extra])


@pytest.mark.parametrize("mod", [run_gan_rnn, run_rnn])
def test_cli_refusals(mod, corpus):
    p = mod.build_parser()
    ok = _flags(p, corpus, "--tr_rir_scp", "RIR", "--tr_labels_wav_scp", "LAB", "--cv_rir_scp", "RIR", "--cv_labels_wav_scp", "LAB", "--noise_scp", "NOI")
    run_gan_rnn.check_wav_flags(ok)
    r = run_gan_rnn.split_reader(ok, "tr", None, True, 1)
    assert r.simulate is not None and len(r.simulate.rirs) == 3 and len(r.simulate.noises) == 2 and r.simulate.spec.snr == (5.0, 20.0)
    for extra, word in ((("--tr_rir_scp", "RIR", "--tr_inputs_wav_scp", "LAB", "--tr_labels_wav_scp", "LAB"), "give one of them"),
                        (("--tr_rir_scp", "RIR"), "needs --tr_labels_wav_scp"),
                        (("--cv_rir_scp", "RIR", "--cv_labels_wav_scp", "LAB", "--cv_inputs_scp", "x.scp"), "give one kind per split"),
                        (("--noise_scp", "NOI", "--tr_inputs_wav_scp", "LAB", "--tr_labels_wav_scp", "LAB"), "--noise_scp adds noise to simulated inputs"),
                        (("--tr_rir_scp", "RIR", "--tr_labels_wav_scp", "LAB", "--snr_lower", "30", "--snr_upper", "10"), "is above --snr_upper"),
                        (("--tr_rir_scp", "RIR", "--tr_labels_wav_scp", "LAB", "--device_decode"), "--device_decode decodes archives")):
        with pytest.raises(SystemExit) as e:
            run_gan_rnn.check_wav_flags(_flags(p, corpus, *extra))
        assert word in str(e.value), (word, str(e.value))


def test_wave_cmvn_with_simulate(corpus, tmp_path):
    lab, rir = str(corpus / "labels.scp"), str(corpus / "rir.scp")
    stats = wave_cmvn.main(["--rir_scp", rir, "--labels_wav_scp", lab, "--out", str(tmp_path / "cmvn.npz"), "--sim_seed", "3"])
    plain = wave_cmvn.wave_cmvn(lab, lab)
    assert stats["mean_inputs"].shape == (257,) and np.array_equal(stats["mean_labels"], plain["mean_labels"])
    assert not np.array_equal(stats["mean_inputs"], plain["mean_inputs"])
    for argv, word in ((["--labels_wav_scp", lab, "--out", "x"], "not both and not neither"),
                       (["--inputs_wav_scp", lab, "--rir_scp", rir, "--labels_wav_scp", lab, "--out", "x"], "not both and not neither"),
                       (["--inputs_wav_scp", lab, "--noise_scp", lab, "--labels_wav_scp", lab, "--out", "x"], "--noise_scp goes with --rir_scp")):
        with pytest.raises(SystemExit) as e:
            wave_cmvn.main(argv)
        assert word in str(e.value)
