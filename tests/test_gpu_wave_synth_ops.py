"""rsrgan_wave_synth (csrc/synth.hip) through HipEngine.op_wave_synth against the float64 definition of tests/wave_synth_ref.py.

One batch of the seven utterances of tests/test_gpu_wave_ops.py -- noise, tone, square, impulse, walk, silence, constant -- whose frame
counts lie around the frames per workgroup Fw: Fw + 1, Fw, Fw - 1, 2, 1, 0 and 3; the square wave starts at an odd sample.  A second batch
of noise with sample counts around the scan chunk CH: CH - 1, CH, CH + 1, 2 CH + 1.  Three LPS inputs per utterance: its own LPS, its own
LPS plus N(0, 1) per bin, and the LPS of a different signal of the same length.

Figure: e = max_t |out - ref| / rms(ref) over EVERY sample of the utterance.  Bound: 4 x the larger of (a) what synth_fp32_baseline -- the
same steps in float32 on the CPU, torch.fft, a sequential recurrence -- reaches on the same utterance and LPS, computed here, and (b) the
float32 spacing at max |ref| over rms(ref).  Why 4: another butterfly or scan order changes the number of roundings by a small factor; a
wrong twiddle, a lost carry or a missed mean term is wrong by orders of magnitude.  A reference that is identically zero demands exact
zeros.

Further: equal bits across two runs, across int16 / float32 samples, across a permuted batch and across B = 1 against the full batch;
canaries in front of and behind `out`, between the utterances and behind a capacity shorter than n; rows truncated through `offsets`.
-s prints the achieved figures (profiles/wave_synth.txt holds them)."""
import numpy as np
import pytest
import torch

from rsrgan_amd.io import wave as W
from tests import wave_ref as R
from tests import wave_synth_ref as Y
from tests.helpers import build_hip_pair, small_cfg
from tests.test_gpu_wave_ops import NAMES, signals

pytestmark = pytest.mark.gpu

BAND = 64
CANARY = -12345.5
KINDS = ("own", "noisy", "other")


@pytest.fixture(scope="module")
def eng():
    model, _ = build_hip_pair(small_cfg("lstm"), 1, 4, seed=1)
    return model.engine


def lps_inputs(x, seed, spec=W.DEFAULT):
    """the three LPS inputs of an utterance, float32 [F, bins] each"""
    rng = np.random.default_rng(seed)
    own = W.lps_from_wave(x, spec=spec)
    noisy = (own + rng.standard_normal(own.shape)).astype(np.float32)
    y = np.clip(np.rint(rng.standard_normal(x.shape[0]) * 2000), -32768, 32767).astype(np.int16)
    return dict(own=own, noisy=noisy, other=W.lps_from_wave(y, spec=spec))


def references(sig, names, spec=W.DEFAULT):
    """{(name, kind): (lps, float64 reference, fp32 baseline)}: computed once per module and left unchanged"""
    kw = dict(win=spec.window, N=spec.frame_length, S=spec.frame_shift, P=spec.padded, coef=spec.preemph)
    out = {}
    for i, k in enumerate(names):
        for kind, lps in lps_inputs(sig[k], 100 + i, spec).items():
            out[k, kind] = (lps, Y.synth(lps, sig[k], **kw), Y.synth_fp32_baseline(lps, sig[k], **kw))
    return out


def layout(sig, lps, order, pads, gaps, caps, kind):
    """the batch as the entry takes it: utterance k after pads[k] samples of filler; its rows after one canary row; its output after
    gaps[k] canary samples, with capacity caps.get(k, n)"""
    parts, seg, rows, off, oseg, at, row, o = [], [], [], [], [], 0, 0, 0
    nb = next(iter(lps.values())).shape[1]
    for k in order:
        parts.append(np.full(pads.get(k, 0), 77, np.int16)); at += pads.get(k, 0)
        parts.append(sig[k]); seg.append((at, sig[k].shape[0])); at += sig[k].shape[0]
        rows.append(lps[k]); off.append(row); row += lps[k].shape[0]
        o += gaps.get(k, 0)
        oseg.append((o, caps.get(k, sig[k].shape[0]))); o += caps.get(k, sig[k].shape[0])
    parts.append(np.full(5, -77, np.int16))
    blob = np.concatenate(parts)
    rows.append(np.full((1, nb), 3.0, np.float32))                      # (one row of no utterance: lps_rows is never 0)
    return (blob.astype(np.float32) if kind else blob, np.array(seg, np.int64), np.array(off + [row], np.int32), np.concatenate(rows, 0),
            np.array(oseg, np.int64), o + 3)


def run(eng, blob, seg, offsets, lps, oseg, out_len, spec=W.DEFAULT):
    """one call into a banded canary buffer -> out [out_len] on the host"""
    dev = eng.device
    us = eng.upload_stream()
    win, tw = eng.wave_tables(spec, us)
    us.synchronize()
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (blob, seg, offsets, lps, oseg)]
    keep = [a.clone() for a in t]
    B = seg.shape[0]
    buf = torch.full((BAND + out_len + BAND,), CANARY, dtype=torch.float32, device=dev)
    out = buf[BAND:BAND + out_len]
    work = torch.empty(eng.wave_synth_work(B, lps.shape[0], out_len, spec.frame_length), dtype=torch.uint8, device=dev)
    eng.op_wave_synth(t[0], t[1], t[2], t[3], B, win, tw, out, t[4], work, spec.frame_length, spec.frame_shift, spec.padded, spec.preemph)
    torch.cuda.synchronize()
    for a, b in zip(t, keep):
        assert torch.equal(a, b), "an input was written"
    host = buf.cpu().numpy()
    assert (host[:BAND] == CANARY).all() and (host[-BAND:] == CANARY).all(), "written outside out"
    return host[BAND:-BAND].copy()


def split(out, order, sig, oseg):
    """{name: its samples}, after checking that every sample of no utterance kept the canary"""
    got, used = {}, np.zeros(out.shape[0], bool)
    for i, k in enumerate(order):
        n = min(sig[k].shape[0], int(oseg[i, 1]))
        got[k] = out[oseg[i, 0]:oseg[i, 0] + n]
        used[oseg[i, 0]:oseg[i, 0] + n] = True
    assert (out[~used] == CANARY).all(), "a sample of no utterance was written"
    assert not (out[used] == CANARY).any() and np.isfinite(out[used]).all()
    return got


def check(got, refs, names, kind, label, lines):
    fails = []
    for k in names:
        _, ref, base = refs[k, kind]
        e, b = Y.figure(got[k], ref[:got[k].shape[0]]), Y.bound(base, ref)
        lines.append("%-8s %-9s %-6s n %5d  e %.3e  baseline %.3e  bound %.3e" % (label, k, kind, ref.shape[0], e, Y.figure(base, ref), b))
        if not e <= b:
            fails.append((k, kind))
        if not ref.any():
            assert not got[k].any(), (k, kind)
    return fails


PADS = dict(noise=0, tone=4, square=3, impulse=0, walk=8, silence=2, constant=1)       # (3: the square wave starts at an odd sample)
GAPS = dict(noise=0, tone=2, square=0, impulse=1, walk=0, silence=3, constant=5)


@pytest.fixture(scope="module")
def case(eng):
    Fw = eng.wave_frames_per_workgroup(R.P)
    assert Fw >= 3
    sig, count = signals(Fw)
    refs = references(sig, NAMES)
    for k in NAMES:
        assert refs[k, "own"][0].shape == (count[k], R.NB)
    return sig, count, refs


def test_error_figures_bits_and_canaries(eng, case, capsys):
    sig, count, refs = case
    lines, fails, first = [], [], {}
    for kind in KINDS:
        lps = {k: refs[k, kind][0] for k in NAMES}
        blob, seg, off, rows, oseg, n_out = layout(sig, lps, NAMES, PADS, GAPS, {}, 0)
        assert seg[2, 0] % 2 == 1
        out = run(eng, blob, seg, off, rows, oseg, n_out)
        got = split(out, NAMES, sig, oseg)
        fails += check(got, refs, NAMES, kind, "frames", lines)
        first[kind] = (out, got)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not fails, (fails, lines)
    # the constant has no spectrum: all of its output is the restored mean, x[t] - a^t x[0] wherever a frame covers
    c, cov = first["own"][1]["constant"], R.N + 2 * R.S
    want = 1000.0 * (1.0 - R.COEF ** np.arange(cov))
    assert np.abs(c[:cov] - want).max() <= 0.05 and not c[cov:].any() and not first["own"][1]["silence"].any()
    kind = "noisy"
    lps = {k: refs[k, kind][0] for k in NAMES}
    out0, got0 = first[kind]
    args = layout(sig, lps, NAMES, PADS, GAPS, {}, 0)
    # run to run
    assert run(eng, *args).tobytes() == out0.tobytes()
    # float32 samples on the same scale: the same bits
    fargs = layout(sig, lps, NAMES, PADS, GAPS, {}, 1)
    assert fargs[0].dtype == np.float32
    assert run(eng, *fargs).tobytes() == out0.tobytes()
    # another composition of the same utterances: other order, other sample offsets, other rows, other places in out
    order = NAMES[::-1]
    pads = dict(noise=5, impulse=7, walk=1, constant=2)
    gaps = dict(noise=1, square=4, constant=1)
    a2 = layout(sig, lps, order, pads, gaps, {}, 0)
    got2 = split(run(eng, *a2), order, sig, a2[4])
    for k in NAMES:
        assert got0[k].tobytes() == got2[k].tobytes(), k
    # B = 1 against the full batch
    for k in ("noise", "walk"):
        a1 = layout(sig, lps, [k], {k: 1}, {k: 2}, {}, 0)
        assert split(run(eng, *a1), [k], sig, a1[4])[k].tobytes() == got0[k].tobytes(), k
    # a capacity shorter than n: the samples that fit are the same, nothing behind them is written
    caps = dict(noise=sig["noise"].shape[0] - 100, tone=1, square=0)
    a3 = layout(sig, lps, NAMES, PADS, GAPS, caps, 0)
    got3 = split(run(eng, *a3), NAMES, sig, a3[4])
    for k in NAMES:
        assert got3[k].tobytes() == got0[k][:got3[k].shape[0]].tobytes(), k
    assert got3["noise"].shape[0] == caps["noise"] and got3["tone"].shape[0] == 1 and got3["square"].shape[0] == 0


def test_offsets_truncate_an_utterance(eng, case):
    sig, count, refs = case
    lps = {k: refs[k, "noisy"][0] for k in NAMES}
    blob, seg, off, rows, oseg, n_out = layout(sig, lps, NAMES, PADS, GAPS, {}, 0)
    full = split(run(eng, blob, seg, off, rows, oseg, n_out), NAMES, sig, oseg)
    # the noise utterance (Fw + 1 frames) gets 3 rows, the tone (Fw frames) none: later utterances' rows move up
    keep = dict(noise=3, tone=0)
    rows2, off2 = [], [0]
    for k in NAMES:
        m = keep.get(k, lps[k].shape[0])
        rows2.append(lps[k][:m]); off2.append(off2[-1] + m)
    rows2.append(np.full((1, R.NB), 3.0, np.float32))
    out = split(run(eng, blob, seg, np.array(off2, np.int32), np.concatenate(rows2, 0), oseg, n_out), NAMES, sig, oseg)
    for k in NAMES:
        if k not in keep:
            assert out[k].tobytes() == full[k].tobytes(), k
    assert not out["tone"].any()
    cov = R.N + 2 * R.S
    ref = Y.synth(lps["noise"][:3], sig["noise"])
    base = Y.synth_fp32_baseline(lps["noise"][:3], sig["noise"])
    assert not out["noise"][cov:].any() and out["noise"][cov - 1] != 0.0
    assert Y.figure(out["noise"], ref) <= Y.bound(base, ref)
    # the samples only the first two frames reach have the full run's bits
    assert out["noise"][:2 * R.S + 1].tobytes() == full["noise"][:2 * R.S + 1].tobytes()
    # lps_rows below the table's rows: the utterance whose rows end there is cut, nothing is read past it
    short = int(off[1]) - 2
    o2 = split(run(eng, blob, seg, off, rows[:short], oseg, n_out), NAMES, sig, oseg)
    c2 = R.N + (short - 1) * R.S
    assert o2["noise"][:c2 - R.N + 1].tobytes() == full["noise"][:c2 - R.N + 1].tobytes() and not o2["noise"][c2:].any()
    for k in NAMES[1:]:
        assert not o2[k].any(), k


def test_chunk_boundaries(eng, capsys):
    CH = eng.wave_synth_chunk()
    rng = np.random.default_rng(9)
    names = ["ch-1", "ch", "ch+1", "2ch+1"]
    sig = {k: np.clip(np.rint(rng.standard_normal(n) * 3000), -32768, 32767).astype(np.int16)
           for k, n in zip(names, (CH - 1, CH, CH + 1, 2 * CH + 1))}
    refs = references(sig, names)
    lines, fails = [], []
    for kind in KINDS:
        lps = {k: refs[k, kind][0] for k in names}
        a = layout(sig, lps, names, {"ch": 1}, {"ch+1": 3}, {}, 0)
        got = split(run(eng, *a), names, sig, a[4])
        fails += check(got, refs, names, kind, "chunks", lines)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not fails, (fails, lines)


@pytest.mark.parametrize("N,S,P,window,coef", [(200, 80, 256, "povey", 0.97), (100, 30, 128, "hamming", 0.97), (64, 64, 64, "hamming", 0.97),
                                               (1000, 333, 1024, "hamming", 0.97), (400, 160, 512, "hamming", 0.0)])
def test_other_framings(eng, N, S, P, window, coef, capsys):
    """the general path (P is an argument; an odd log2(P / 2) ends in a radix-2 stage; no overlap; more terms per sample; no pre-emphasis):
    noise, 2 Fw + 1 frames, the same figure and bound"""
    spec = W.WaveSpec(N, S, P, coef, window)
    frames = 2 * eng.wave_frames_per_workgroup(P) + 1
    x = np.clip(np.rint(np.random.default_rng(P).standard_normal(N + (frames - 1) * S + 1) * 3000), -32768, 32767).astype(np.int16)
    sig = {"x": x}
    refs = references(sig, ["x"], spec)
    lines, fails = [], []
    for kind in KINDS:
        a = layout(sig, {"x": refs["x", kind][0]}, ["x"], {}, {"x": 1}, {}, 0)
        got = split(run(eng, *a, spec=spec), ["x"], sig, a[4])
        fails += check(got, refs, ["x"], kind, "%d/%d/%d" % (N, S, P), lines)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not fails, (fails, lines)
