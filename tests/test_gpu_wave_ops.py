"""rsrgan_feat_wave (csrc/wave.hip k_feat_wave) through HipEngine.op_feat_wave against the float64 definition of tests/wave_ref.py.

One batch of seven utterances -- rounded Gaussian noise (sigma 3000), a bin-centred tone (amplitude 20000), a +-full-scale square wave,
one impulse, a clipped random walk, digital silence, a constant 1000 -- whose frame counts lie around the kernel's frames per workgroup
F: F + 1, F, F - 1, 2, 1, 0 and 3 (the silence makes no frame: the constant, mean-free zero as well, is the utterance that exercises the
clamp).  One utterance starts at an odd sample; both sample kinds run; one run truncates an utterance through `offsets`.

Two error figures per utterance, both against float64, no bin left out of the first:
  power   max |exp(out_k) - max(p_k, eps)| / max(max_k p_k, eps)              over all bins k >= 1 of all frames
  log     max |out_k - log max(p_k, eps)| over the bins with p_k >= 1e-6 max_k p_k, and |out_0 - E|
The bound of each is 4 x the larger of (a) the figure tests/wave_ref.py lps_fp32_baseline -- the same steps in float32 on the CPU with
torch.fft.rfft -- reaches on the same utterance, computed here, and (b) the float32 spacing at the frame's largest |log| value (a relative
power error d and a log error d are the same thing to first order, so (b) serves both).  Why 4: another butterfly order and radix changes
the number of roundings per output by a small factor; a wrong twiddle, a dropped stage or a lost pre-emphasis is wrong by orders of
magnitude.  The log figure must cover at least 95 % of the noise utterance's bins.

Further: the bits are equal across two runs, across the two sample kinds and across two batch compositions of the same utterances; rows
outside every utterance keep a canary; nothing is written in front of `out` or past out_rows.  -s prints the achieved figures
(profiles/feat_wave.txt holds them)."""
import numpy as np
import pytest
import torch

from rsrgan_amd.io import wave as W
from tests import wave_ref as R
from tests.helpers import build_hip_pair, small_cfg

pytestmark = pytest.mark.gpu

BAND = 64                                     # floats in front of and behind `out` (a multiple of 4: out stays 16-byte aligned)
CANARY = -12345.5
NAMES = ["noise", "tone", "square", "impulse", "walk", "silence", "constant"]


@pytest.fixture(scope="module")
def eng():
    model, _ = build_hip_pair(small_cfg("lstm"), 1, 4, seed=1)
    return model.engine


def _samples(frames):
    return 0 if frames <= 0 else R.N + (frames - 1) * R.S


def signals(F):
    """the seven utterances (int16) by name; the sample counts leave up to S - 1 samples of no frame behind the last frame"""
    rng = np.random.default_rng(2024)
    count = dict(noise=F + 1, tone=F, square=F - 1, impulse=2, walk=1, silence=0, constant=3)
    n = {k: _samples(v) + (37 if v else 399) for k, v in count.items()}
    i = {k: np.arange(v) for k, v in n.items()}
    s = {
        "noise": np.clip(np.rint(rng.standard_normal(n["noise"]) * 3000), -32768, 32767),
        "tone": np.rint(20000 * np.sin(2 * np.pi * 37 * i["tone"] / R.P + 0.3)),
        "square": np.where((i["square"] // 23) % 2 == 0, 32767, -32768),
        "impulse": np.where(i["impulse"] == 300, 25000, 0),
        "walk": np.clip(np.cumsum(rng.integers(-400, 401, n["walk"])), -32768, 32767),
        "silence": np.zeros(n["silence"]),
        "constant": np.full(n["constant"], 1000),
    }
    return {k: v.astype(np.int16) for k, v in s.items()}, count


@pytest.fixture(scope="module")
def case(eng):
    F = eng.wave_frames_per_workgroup(R.P)
    assert F >= 3
    sig, count = signals(F)
    ref = {k: R.frames(v) for k, v in sig.items()}                      # (E, p) in float64, computed once and left unchanged
    base = {k: R.lps_fp32_baseline(v) for k, v in sig.items()}
    for k in NAMES:
        assert ref[k][1].shape == base[k].shape == (count[k], R.NB)
    return F, sig, count, ref, base


def figures(out, E, p):
    """(power figure, log figure, share of bins the log figure covers, the float32 spacing at the largest |log| value) of one utterance"""
    out = np.asarray(out, np.float64)
    if out.shape[0] == 0:
        return 0.0, 0.0, 1.0, 0.0
    pk, ok = np.maximum(p[:, 1:], R.EPS), out[:, 1:]
    top = np.maximum(p[:, 1:].max(1, keepdims=True), R.EPS)
    power = float((np.abs(np.exp(ok) - pk) / top).max())
    line = p[:, 1:] >= 1e-6 * p[:, 1:].max(1, keepdims=True)
    err = np.abs(ok - np.log(pk))
    e0 = np.abs(out[:, 0] - np.log(np.maximum(E, R.EPS)))
    log = float(max(err[line].max() if line.any() else 0.0, e0.max()))
    want = np.concatenate([np.log(np.maximum(E, R.EPS))[:, None], np.log(pk)], 1)
    return power, log, float(line.mean()), float(R.ulp32(np.abs(want).max()))


def layout(sig, order, pads, slack, kind):
    """the batch as the entry takes it: utterance k of `order` after pads[k] samples of filler, its frame 0 at a row that leaves
    slack[k] canary rows behind its last frame"""
    parts, seg, rows, at, row = [], [], [], 0, 0
    for k in order:
        parts.append(np.full(pads[k], 77, np.int16)); at += pads[k]
        parts.append(sig[k]); seg.append((at, sig[k].shape[0])); at += sig[k].shape[0]
        rows.append(row); row += R.frame_count(sig[k].shape[0]) + slack[k]
    parts.append(np.full(5, -77, np.int16))
    blob = np.concatenate(parts)
    return blob.astype(np.float32) if kind else blob, np.array(seg, np.int64), np.array(rows + [row], np.int32)


def run(eng, blob, seg, offsets, out_rows, spec=W.DEFAULT, extra=0):
    """one launch into a banded canary buffer -> (the whole buffer's bits, out [out_rows + extra, bins] on the host)"""
    dev = eng.device
    us = eng.upload_stream()
    win, tw = eng.wave_tables(spec, us)
    us.synchronize()
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (blob, seg, offsets)]
    keep = [a.clone() for a in t]
    NB = spec.bins
    buf = torch.full((BAND + (out_rows + extra) * NB + BAND,), CANARY, dtype=torch.float32, device=dev)
    out = buf[BAND:BAND + (out_rows + extra) * NB].view(out_rows + extra, NB)
    assert out.data_ptr() % 16 == 0
    eng.op_feat_wave(t[0], t[1], t[2], seg.shape[0], win, tw, out, spec.frame_length, spec.frame_shift, spec.padded, spec.preemph,
                     out_rows=out_rows)
    torch.cuda.synchronize()
    for a, b in zip(t, keep):
        assert torch.equal(a, b), "an input was written"
    host = buf.cpu().numpy()
    assert (host[:BAND] == CANARY).all() and (host[-BAND:] == CANARY).all(), "written outside out"
    return host.view(np.int32).copy(), host[BAND:-BAND].reshape(out_rows + extra, NB).copy()


PADS = dict(noise=0, tone=4, square=3, impulse=0, walk=8, silence=2, constant=1)       # (3: the square wave starts at an odd sample)
SLACK = dict(noise=0, tone=2, square=0, impulse=1, walk=0, silence=3, constant=0)


def split(out, order, sig, offsets, slack):
    """{name: its rows}, after checking that every row of no utterance kept the canary"""
    rows, used = {}, np.zeros(out.shape[0], bool)
    for i, k in enumerate(order):
        n = R.frame_count(sig[k].shape[0])
        rows[k] = out[offsets[i]:offsets[i] + n]
        used[offsets[i]:offsets[i] + n] = True
    assert (out[~used] == CANARY).all(), "a row of no utterance was written"
    assert not (out[used] == CANARY).any() and np.isfinite(out[used]).all()
    return rows


def test_error_figures_bits_and_canaries(eng, case, capsys):
    F, sig, count, ref, base = case
    blob, seg, offsets = layout(sig, NAMES, PADS, SLACK, 0)
    assert seg[2, 0] % 2 == 1                                            # the odd start
    out_rows = int(offsets[-1]) + 2
    bits, out = run(eng, blob, seg, offsets, out_rows, extra=3)          # (3 rows past out_rows: nothing is written there)
    rows = split(out, NAMES, sig, offsets, SLACK)
    lines = []
    fails = []
    for k in NAMES:
        E, p = ref[k]
        got = figures(rows[k], E, p)
        want = figures(base[k], E, p)
        bound_p, bound_l = 4 * max(want[0], got[3]), 4 * max(want[1], got[3])
        lines.append("%-8s frames %2d  power %.3e (baseline %.3e, bound %.3e)  log %.3e (baseline %.3e, bound %.3e)  bins above the line %.3f"
                     % (k, count[k], got[0], want[0], bound_p, got[1], want[1], bound_l, got[2]))
        if not (got[0] <= bound_p and got[1] <= bound_l):
            fails.append(k)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert figures(rows["noise"], *ref["noise"])[2] >= 0.95, "the log figure covers too few of the noise utterance's bins"
    assert not fails, (fails, lines)
    # the clamp: a constant is mean-free zero, so every bin, bin 0 included, holds ONE value: the device's logf(eps), within a float32
    # spacing of log(eps)
    c = rows["constant"]
    assert (c == c[0, 0]).all() and abs(float(c[0, 0]) - np.log(R.EPS)) <= float(R.ulp32(np.log(R.EPS)))
    # run to run
    bits2, _ = run(eng, blob, seg, offsets, out_rows, extra=3)
    assert np.array_equal(bits, bits2)
    # float32 samples on the same scale: the same bits
    fb, fseg, foff = layout(sig, NAMES, PADS, SLACK, 1)
    assert fb.dtype == np.float32
    bits3, _ = run(eng, fb, fseg, foff, out_rows, extra=3)
    assert np.array_equal(bits, bits3)
    # another composition of the same utterances: other order, other sample offsets, other rows, other neighbours in the workgroups' walk
    order = NAMES[::-1]
    pads = dict(noise=5, tone=0, square=0, impulse=7, walk=1, silence=0, constant=2)
    slack = dict(noise=1, tone=0, square=4, impulse=0, walk=0, silence=0, constant=1)
    b2, s2, o2 = layout(sig, order, pads, slack, 0)
    _, out2 = run(eng, b2, s2, o2, int(o2[-1]))
    rows2 = split(out2, order, sig, o2, slack)
    for k in NAMES:
        assert rows[k].tobytes() == rows2[k].tobytes(), k


def test_offsets_truncate_an_utterance(eng, case):
    F, sig, count, ref, base = case
    blob, seg, offsets = layout(sig, NAMES, PADS, SLACK, 0)
    _, full = run(eng, blob, seg, offsets, int(offsets[-1]))
    # the noise utterance (F + 1 frames) gets 3 rows, the tone (F frames) none: later utterances move up
    n = np.diff(offsets)
    n[0], n[1] = 3, 0
    cut = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    _, out = run(eng, blob, seg, cut, int(cut[-1]))
    want = np.full_like(out, CANARY)
    for i, k in enumerate(NAMES):
        m = min(R.frame_count(sig[k].shape[0]), int(n[i]))
        want[cut[i]:cut[i] + m] = full[offsets[i]:offsets[i] + m]
    assert out.tobytes() == want.tobytes()
    # out_rows below the table's rows: nothing is written past it (rows the table places there are clamped onto the last row, which is
    # therefore not compared)
    short = int(offsets[1]) - 2
    _, out = run(eng, blob, seg, offsets, short, extra=4)
    assert out[:short - 1].tobytes() == full[:short - 1].tobytes() and (out[short:] == CANARY).all()


@pytest.mark.parametrize("N,S,P,window", [(200, 80, 256, "povey"), (100, 30, 128, "hamming"), (64, 64, 64, "hamming"), (1000, 333, 1024, "hamming"),
                                          (2048, 700, 2048, "hamming")])
def test_other_framings(eng, N, S, P, window):
    """the general path (P is an argument; an odd log2(P / 2) ends in a radix-2 stage; P above 1024 takes fewer frames per workgroup):
    noise, 2 F + 1 frames, the same two figures and bounds"""
    spec = W.WaveSpec(N, S, P, 0.5, window)
    F = eng.wave_frames_per_workgroup(P)
    frames = 2 * F + 1
    x = np.clip(np.rint(np.random.default_rng(P).standard_normal(N + (frames - 1) * S + 1) * 3000), -32768, 32767).astype(np.int16)
    E, p = R.frames(x, window, N=N, S=S, P=P, coef=0.5)
    base = R.lps_fp32_baseline(x, window, N=N, S=S, P=P, coef=0.5)
    _, out = run(eng, x, np.array([[0, x.shape[0]]], np.int64), np.array([0, frames], np.int32), frames, spec=spec, extra=1)
    assert (out[frames:] == CANARY).all()
    got, want = figures(out[:frames], E, p), figures(base, E, p)
    assert got[2] >= 0.95
    assert got[0] <= 4 * max(want[0], got[3]) and got[1] <= 4 * max(want[1], got[3]), (got, want)
