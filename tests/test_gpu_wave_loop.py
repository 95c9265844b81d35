"""The waveform front end in the loop, on a small generator with input_dim = 257 x (2 + 1 + 2), B = 4:

  * HipEngine.featurize(WaveBatch) equals rsrgan_feat_batch applied to the rows rsrgan_feat_wave gave, bit for bit;
  * StreamBank(device_features=True).push_audio, the audio cut into ragged pushes of 1, 159, 161 and 4000 samples over three rows with a
    flush in between, gives the outputs of push fed with the DEVICE's log-power-spectrum rows of the whole utterances (the same frames
    in the same pushes), bit for bit: chunking the audio changes nothing;
  * those outputs agree with the host route's (lps_from_wave in float64, then push) within the bound tests/test_gpu_feat_stream_loop.py
    holds a host path and a device path that cut their forward calls alike or not to: 2 x LOSS_RTOL on G(x);
  * counters["bytes_up"] per frame is below the push route's."""
import numpy as np
import pytest
import torch

from rsrgan_amd.io import wave as W
from rsrgan_amd.stream import StreamBank
from tests.helpers import build_hip_pair, small_cfg
from tests.test_gpu_stream import LOSS_RTOL, l1

pytestmark = pytest.mark.gpu

LEFT, RIGHT, CHUNK, NB = 2, 2, 5, 257


@pytest.fixture(scope="module")
def model():
    cfg = small_cfg("lstm", input_dim=NB * (LEFT + 1 + RIGHT), output_dim=4)
    m, _ = build_hip_pair(cfg, 4, 8, seed=77, flags=1)
    return m


def _cmvn(rng):
    return dict(mean_inputs=20.0 + rng.standard_normal(NB), stddev_inputs=rng.uniform(2.0, 4.0, NB),
                mean_labels=rng.standard_normal(4), stddev_labels=rng.uniform(0.5, 2.0, 4))


def _noise(rng, n):
    return np.clip(np.rint(rng.standard_normal(n) * 3000), -32768, 32767).astype(np.int16)


def _device_lps(eng, utts):
    """the device's raw LPS rows of whole utterances, on the host: [frames_i, 257] float32 each"""
    wb = W.pack_wave(utts)
    us = eng.upload_stream()
    with torch.cuda.stream(us):
        raw, _ = eng.wave_features(wb.samples, wb.seg, wb.offsets, int(wb.offsets[-1]), wb.spec, us)
    us.synchronize()
    raw = raw.cpu().numpy()
    return [raw[a:b] for a, b in zip(wb.offsets[:-1], wb.offsets[1:])], wb


def test_featurize_wave_batch_equals_wave_then_batch(model):
    eng = model.engine
    rng = np.random.default_rng(5)
    cm = _cmvn(rng)
    utts = [_noise(rng, n) for n in (400 + 160 * 7 + 3, 399, 400, 400 + 160 * 4 + 159)]
    mean, std = np.ascontiguousarray(cm["mean_inputs"]), np.ascontiguousarray(cm["stddev_inputs"])
    wb = W.pack_wave(utts, None, LEFT, RIGHT, mean, std)
    assert wb.shape == (4, 8, NB * 5) and wb.lengths().tolist() == [8, 0, 1, 5]
    x, ln = eng.featurize(wb)
    torch.cuda.synchronize()
    assert ln.cpu().tolist() == [8, 0, 1, 5]
    lps, _ = _device_lps(eng, utts)
    raw = torch.from_numpy(np.concatenate(lps, 0)).to(eng.device)
    off = torch.from_numpy(wb.offsets).to(eng.device)
    dm, ds = torch.from_numpy(mean).to(eng.device), torch.from_numpy(std).to(eng.device)
    want = torch.empty_like(x)
    eng.op_feat_batch(raw, off, 4, 8, NB, LEFT, RIGHT, dm, ds, want)
    torch.cuda.synchronize()
    assert x.shape == (4, 8, NB * 5) and torch.equal(x.view(torch.int32), want.view(torch.int32))
    # and the rows are the definition's, to float32 accuracy of a log near 20 (the figures themselves: tests/test_gpu_wave_ops.py)
    host = W.lps_from_wave(utts[0])
    assert np.abs(lps[0] - host).max() < 1e-3
    # a float32 batch on the same scale: the same bits
    xf, _ = eng.featurize(W.pack_wave([u.astype(np.float32) for u in utts], None, LEFT, RIGHT, mean, std))
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int32), xf.view(torch.int32))
    with pytest.raises(ValueError):
        eng.featurize(W.pack_wave([_noise(rng, 400 + 160 * 8)], None, LEFT, RIGHT, mean, std))      # 9 frames, max_frames = 8
    assert eng.device_status() == 0


def _schedule(utts):
    """steps of ({row: (lo, hi)} sample ranges pushed, rows flushed afterwards): ragged pushes of 1, 159, 161 and 4000 samples, every row at
    its own phase of that cycle; row 2 carries two utterances, the flush between them drops the first one's samples of no frame"""
    sizes = [1, 159, 161, 4000]
    pos, which, phase, steps = {r: 0 for r in utts}, {r: 0 for r in utts}, {r: r for r in utts}, []
    while which:
        push, ended = {}, []
        for r in list(which):
            n = utts[r][which[r]].shape[0]
            k = sizes[phase[r] % 4]
            phase[r] += 1
            push[r] = (which[r], pos[r], min(pos[r] + k, n))
            pos[r] += k
            if pos[r] >= n:
                ended.append(r)
                pos[r] = 0
                which[r] += 1
                if which[r] == len(utts[r]):
                    del which[r]
        steps.append((push, ended))
    return steps


def test_push_audio_on_the_device_equals_push_of_the_devices_frames(model):
    eng = model.engine
    rng = np.random.default_rng(6)
    cm = _cmvn(rng)
    utts = {0: [_noise(rng, 5000)], 1: [_noise(rng, 4700)], 2: [_noise(rng, 700), _noise(rng, 4500)]}
    flat = [u for r in sorted(utts) for u in utts[r]]
    lps, _ = _device_lps(eng, flat)
    whole = {}
    for r in sorted(utts):
        whole[r] = [lps.pop(0) for _ in utts[r]]
    steps = _schedule(utts)
    assert sum(len(e) for _, e in steps) == 4 and len(steps) > 6

    def drive(bank, as_audio):
        done, cur = {r: [] for r in utts}, {r: [] for r in utts}
        for push, ended in steps:
            if as_audio:
                outs = bank.push_audio({r: utts[r][u][lo:hi] for r, (u, lo, hi) in push.items()})
            else:
                outs = bank.push({r: whole[r][u][W.num_frames(lo):W.num_frames(hi)] for r, (u, lo, hi) in push.items()})
            for r, y in outs.items():
                cur[r].append(y)
            for r, y in (bank.flush(ended) if ended else {}).items():
                done[r].append(np.concatenate(cur[r] + [y], 0))
                cur[r] = []
        return done

    audio = StreamBank(model, cm, LEFT, RIGHT, chunk=CHUNK, streams=3, device_features=True)
    got = drive(audio, True)
    frames_ = StreamBank(model, cm, LEFT, RIGHT, chunk=CHUNK, streams=3, device_features=True)
    want = drive(frames_, False)
    host = StreamBank(model, cm, LEFT, RIGHT, chunk=CHUNK, streams=3, device_features=False)
    ref = drive(host, True)
    total = 0
    for r in utts:
        assert len(got[r]) == len(want[r]) == len(ref[r]) == len(utts[r])
        for u, a, b, c in zip(utts[r], got[r], want[r], ref[r]):
            F = W.num_frames(u.shape[0])
            total += F
            assert a.shape == b.shape == c.shape == (F, 4) and a.dtype == np.float64
            assert a.tobytes() == b.tobytes(), (r, F, int((a != b).sum()))                  # chunking the audio changes nothing
            g = [(o - cm["mean_labels"]) / cm["stddev_labels"] for o in (a, c)]
            assert l1(g[0], g[1]) < 2 * LOSS_RTOL, (r, F, l1(g[0], g[1]))                     # the host route's frames, float64
    assert audio.counters["rounds"] == frames_.counters["rounds"] and audio.counters["calls"] == frames_.counters["calls"]
    # what went up: the samples of the completed frames and three small tables per push with frames, against 1028 bytes per frame
    up_audio, up_frames = audio.counters["bytes_up"] / total, frames_.counters["bytes_up"] / total
    assert up_audio < up_frames and up_frames > NB * 4, (up_audio, up_frames)
    assert all(p is None for p in audio._pcm)
    assert eng.device_status() == 0
