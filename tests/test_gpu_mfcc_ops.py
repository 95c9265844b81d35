"""rsrgan_feat_mfcc (csrc/wave.hip k_feat_mfcc) through HipEngine.op_feat_mfcc against the float64 definition of tests/mfcc_ref.py.

The seven utterances of tests/test_gpu_wave_ops.py (signals(F), imported) in the same banded canary buffer and the same two layouts, with
the default MfccSpec, launched twice: as log-mel (C = 0) and as MFCC (C = 40).  Each stage is checked on its own, so a failure names it.

  mel     against float64, per utterance: power = max |exp(out_j) - max(m_j, eps)| / max(max_j m_j, eps) over all filters; log =
          max |out_j - log max(m_j, eps)| over the filters with m_j >= 1e-6 max_j m_j.  Each at most 4 x the larger of (a) the figure
          tests/mfcc_ref.py mfcc_fp32_baseline reaches on the same utterance, computed here, and (b) the float32 spacing at the largest
          |log| value.  Why 4 (as tests/test_gpu_wave_ops.py): another summation order changes the number of roundings by a small factor; a
          wrong weight, a shifted bin or a lost filter is wrong by orders of magnitude.  The line leaves no filter of the noise, square,
          impulse, walk and constant utterances out (a fact of the float64 reference, asserted).
  dct     a derived bound, no baseline: c^ = dct32 . l_device in float64, from the float32 table and the device's own log-mel bits;
          |c_i - c^_i| <= (M + 1) 2^-24 sum_j |dct_ij l_j|, the standard bound of an M-term fp32 dot product in any order, FMA or not.
  end     max |c_i - c_i(float64)| at most 4 x max(the baseline's figure, the float32 spacing at the largest |c|) for the five utterances
          above; printed, not bounded, for the tone: its far filters sit 1e-10 below the peak, where the float32 baseline itself is off by
          1e-2.
Further: the constant utterance's log-mel row is one value within a float32 spacing of log(eps); the bits are equal run to run, between
the two sample kinds and between two batch compositions; canaries hold in rows of no utterance, in front of `out` and past out_rows;
inputs and tables are unwritten; `offsets` truncates; five other shapes reach the other code paths; a hostile mel_seg is clamped.
-s prints the achieved figures (profiles/feat_mfcc.txt holds them)."""
import numpy as np
import pytest
import torch

from rsrgan_amd import _lib
from rsrgan_amd.io import wave as W
from tests import mfcc_ref as MR
from tests import wave_ref as R
from tests.helpers import build_hip_pair, small_cfg
from tests.test_gpu_wave_ops import BAND, CANARY, NAMES, PADS, SLACK, layout, signals, split

pytestmark = pytest.mark.gpu

MFCC, FBANK = W.MFCC_DEFAULT, W.MfccSpec(num_ceps=0)
FULL = ["noise", "square", "impulse", "walk", "constant"]          # the utterances whose filters all lie above the line


@pytest.fixture(scope="module")
def eng():
    model, _ = build_hip_pair(small_cfg("lstm"), 1, 4, seed=1)
    return model.engine


def ref_kw(spec):
    return dict(win=spec.window, N=spec.frame_length, S=spec.frame_shift, P=spec.padded, coef=spec.preemph, M=spec.num_mel_bins,
                C=spec.num_ceps, rate=spec.sample_rate, low=spec.low_freq, high=spec.high_freq, Q=spec.cepstral_lifter)


@pytest.fixture(scope="module")
def case(eng):
    F = eng.wave_frames_per_workgroup(R.P)
    assert F >= 3
    sig, count = signals(F)
    ref = {k: MR.stages(v, **ref_kw(MFCC)) for k, v in sig.items()}             # (m, l, c) in float64, computed once, left unchanged
    base = {k: MR.mfcc_fp32_baseline(v, **ref_kw(MFCC)) for k, v in sig.items()}
    for k in NAMES:
        assert ref[k][0].shape == base[k][0].shape == (count[k], 40) and ref[k][2].shape == base[k][1].shape == (count[k], 40)
    return F, sig, count, ref, base


def run(eng, blob, seg, offsets, out_rows, spec, extra=0, mel_seg=None):
    """one launch into a banded canary buffer -> (the whole buffer's bits, out [out_rows + extra, spec.bins] on the host)"""
    dev = eng.device
    us = eng.upload_stream()
    tabs = list(eng.wave_tables(spec, us))
    us.synchronize()
    if mel_seg is not None:
        tabs[2] = torch.from_numpy(np.ascontiguousarray(mel_seg, np.int32)).to(dev)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (blob, seg, offsets)]
    watch = t + [a for a in tabs if a is not None]
    keep = [a.clone() for a in watch]
    NB = spec.bins
    pad = -(out_rows + extra) * NB % 4                                           # (the band behind stays a multiple of 4 floats)
    buf = torch.full((BAND + (out_rows + extra) * NB + pad + BAND,), CANARY, dtype=torch.float32, device=dev)
    out = buf[BAND:BAND + (out_rows + extra) * NB].view(out_rows + extra, NB)
    assert out.data_ptr() % 16 == 0
    eng.op_feat_mfcc(t[0], t[1], t[2], seg.shape[0], tabs[0], tabs[1], tabs[2], tabs[3], tabs[4], out, spec.frame_length, spec.frame_shift,
                     spec.padded, spec.preemph, out_rows=out_rows)
    torch.cuda.synchronize()
    for a, b in zip(watch, keep):
        assert torch.equal(a, b), "an input or a table was written"
    host = buf.cpu().numpy()
    body = host[BAND:BAND + (out_rows + extra) * NB]
    assert (host[:BAND] == CANARY).all() and (host[BAND + body.shape[0]:] == CANARY).all(), "written outside out"
    return host.view(np.int32).copy(), body.reshape(out_rows + extra, NB).copy()


def mel_figures(out, m):
    """(power figure, log figure, share of filters the log figure covers, the float32 spacing at the largest |log| value) of one utterance"""
    out = np.asarray(out, np.float64)
    if out.shape[0] == 0:
        return 0.0, 0.0, 1.0, 0.0
    mk = np.maximum(m, R.EPS)
    top = np.maximum(m.max(1, keepdims=True), R.EPS)
    power = float((np.abs(np.exp(out) - mk) / top).max())
    line = m >= 1e-6 * m.max(1, keepdims=True)
    err = np.abs(out - np.log(mk))
    return power, float(err[line].max()), float(line.mean()), float(R.ulp32(np.abs(np.log(mk)).max()))


def check_dct(c_dev, l_dev, dct32):
    """the derived bound of the DCT stage; returns the largest |c - c^| / bound"""
    d, l = dct32.astype(np.float64), np.asarray(l_dev, np.float64)
    if c_dev.shape[0] == 0:
        return 0.0
    want = l @ d.T
    bound = (d.shape[1] + 1) * 2.0 ** -24 * (np.abs(l)[:, None, :] * np.abs(d)[None, :, :]).sum(2)
    ratio = np.abs(np.asarray(c_dev, np.float64) - want) / bound
    assert (ratio <= 1.0).all(), ("dct stage", float(ratio.max()))
    return float(ratio.max())


def end_figures(c_out, c):
    """(max |c_i - c_i(float64)|, the float32 spacing at the largest |c|)"""
    if c.shape[0] == 0:
        return 0.0, 0.0
    return float(np.abs(np.asarray(c_out, np.float64) - c).max()), float(R.ulp32(np.abs(c).max()))


def test_stages_bits_and_canaries(eng, case, capsys):
    F, sig, count, ref, base = case
    blob, seg, offsets = layout(sig, NAMES, PADS, SLACK, 0)
    assert seg[2, 0] % 2 == 1                                            # the odd start
    out_rows = int(offsets[-1]) + 2
    lbits, lout = run(eng, blob, seg, offsets, out_rows, FBANK, extra=3)  # (3 rows past out_rows: nothing is written there)
    cbits, cout = run(eng, blob, seg, offsets, out_rows, MFCC, extra=3)
    lrows, crows = split(lout, NAMES, sig, offsets, SLACK), split(cout, NAMES, sig, offsets, SLACK)
    dct32 = W.dct_table(MFCC)
    lines, fails = [], []
    for k in NAMES:
        m, l, c = ref[k]
        got, want = mel_figures(lrows[k], m), mel_figures(base[k][0], m)
        bound_p, bound_l = 4 * max(want[0], got[3]), 4 * max(want[1], got[3])
        lines.append("%-8s frames %2d  mel: power %.3e (baseline %.3e, bound %.3e)  log %.3e (baseline %.3e, bound %.3e)  filters above the line %.3f"
                     % (k, count[k], got[0], want[0], bound_p, got[1], want[1], bound_l, got[2]))
        if not (got[0] <= bound_p and got[1] <= bound_l):
            fails.append(("mel", k))
        if k in FULL:
            assert got[2] == 1.0, (k, got[2])
        ratio = check_dct(crows[k], lrows[k], dct32)
        e, eb = end_figures(crows[k], c), end_figures(base[k][1], c)
        bound_e = 4 * max(eb[0], e[1])
        lines.append("%-8s            dct: |c - dct32 . l_device| at most %.3f of the bound  end: %.3e (baseline %.3e, bound %.3e%s)"
                     % (k, ratio, e[0], eb[0], bound_e, "" if k in FULL or not count[k] else ", not asserted"))
        if k in FULL and not e[0] <= bound_e:
            fails.append(("end", k))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    # the tone: 6 of the 40 filters of every frame lie above the line in the float64 reference (15 %)
    tone = ref["tone"][0]
    assert ((tone >= 1e-6 * tone.max(1, keepdims=True)).sum(1) == 6).all() and abs(mel_figures(lrows["tone"], tone)[2] - 0.15) < 1e-12
    assert not fails, (fails, lines)
    # the clamp: a constant is mean-free zero, every filter sums zeros: ONE value, the device's logf(eps), within a spacing of log(eps)
    c = lrows["constant"]
    assert (c == c[0, 0]).all() and abs(float(c[0, 0]) - np.log(R.EPS)) <= float(R.ulp32(np.log(R.EPS)))
    # run to run; float32 samples on the same scale; both for both launches
    fb, fseg, foff = layout(sig, NAMES, PADS, SLACK, 1)
    assert fb.dtype == np.float32
    for spec, bits in ((FBANK, lbits), (MFCC, cbits)):
        assert np.array_equal(bits, run(eng, blob, seg, offsets, out_rows, spec, extra=3)[0])
        assert np.array_equal(bits, run(eng, fb, fseg, foff, out_rows, spec, extra=3)[0])
    # another composition of the same utterances: other order, other sample offsets, other rows, other neighbours in the workgroups' walk
    order = NAMES[::-1]
    pads = dict(noise=5, tone=0, square=0, impulse=7, walk=1, silence=0, constant=2)
    slack = dict(noise=1, tone=0, square=4, impulse=0, walk=0, silence=0, constant=1)
    b2, s2, o2 = layout(sig, order, pads, slack, 0)
    for spec, rows in ((FBANK, lrows), (MFCC, crows)):
        rows2 = split(run(eng, b2, s2, o2, int(o2[-1]), spec)[1], order, sig, o2, slack)
        for k in NAMES:
            assert rows[k].tobytes() == rows2[k].tobytes(), k


def test_offsets_truncate_an_utterance(eng, case):
    F, sig, count, ref, base = case
    blob, seg, offsets = layout(sig, NAMES, PADS, SLACK, 0)
    _, full = run(eng, blob, seg, offsets, int(offsets[-1]), MFCC)
    # the noise utterance (F + 1 frames) gets 3 rows, the tone (F frames) none: later utterances move up
    n = np.diff(offsets)
    n[0], n[1] = 3, 0
    cut = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    _, out = run(eng, blob, seg, cut, int(cut[-1]), MFCC)
    want = np.full_like(out, CANARY)
    for i, k in enumerate(NAMES):
        m = min(R.frame_count(sig[k].shape[0]), int(n[i]))
        want[cut[i]:cut[i] + m] = full[offsets[i]:offsets[i] + m]
    assert out.tobytes() == want.tobytes()
    # out_rows below the table's rows: nothing is written past it (rows the table places there are clamped onto the last row, which is
    # therefore not compared)
    short = int(offsets[1]) - 2
    _, out = run(eng, blob, seg, offsets, short, MFCC, extra=4)
    assert out[:short - 1].tobytes() == full[:short - 1].tobytes() and (out[short:] == CANARY).all()


SHAPES = [(200, 80, 256, 23, 13, "povey", 8000, -400.0),           # 8 kHz, the general path, C < M
          (100, 30, 128, 40, 13, "hamming", 16000, 8000.0),       # 20 .. 8000 Hz: one empty filter; the last stage is radix 2
          (64, 64, 64, 5, 5, "hamming", 16000, -400.0),
          (1000, 333, 1024, 80, 0, "hamming", 16000, -400.0),     # M > 64: the lane loop; fbank only
          (2048, 700, 2048, 128, 40, "hamming", 16000, -400.0),   # fewer frames per workgroup; the LDS need is checked against 64 KB
          (2048, 700, 2048, 40, 13, "hamming", 16000, -400.0)]    # fewer frames per workgroup, a table that fits


@pytest.mark.parametrize("N,S,P,M,C,window,rate,high", SHAPES)
def test_other_shapes(eng, N, S, P, M, C, window, rate, high):
    """noise, 2 F + 1 frames, the same stage checks.  A shape whose LDS need (the formula of include/rsrgan.h) is above 64 KB must be
    refused by the spec and by the entry, with the byte count; every other shape runs."""
    F = eng.wave_frames_per_workgroup(P)
    filt = MR.filters(P, M, rate, 20.0, high)
    nnz, nz, H = sum(len(w) for _, w in filt), min(4, F), P // 2
    need = 8 * (H + nz * H) + 4 * (2 * N + (F - 1) * S) + 4 * (nz * H + nz * M + M * C + 3 * M + nnz)
    kw = dict(frame_length=N, frame_shift=S, padded=P, window=window, sample_rate=rate, num_mel_bins=M, num_ceps=C, high_freq=high)
    if need > 65536:
        with pytest.raises(ValueError, match="%d bytes of LDS" % need):
            W.MfccSpec(**kw)
        dev = eng.device
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
        with pytest.raises(_lib.RsrganError, match="%d bytes of LDS" % need):
            eng.op_feat_mfcc(z(N, dt=torch.int16), torch.tensor([[0, N]], device=dev), torch.tensor([0, 1], dtype=torch.int32, device=dev), 1,
                             z(N), z(H, 2), z(M, 3, dt=torch.int32), z(nnz), z(C, M), z(4, C), N, S, P)
        return
    spec, fb = W.MfccSpec(**kw), W.MfccSpec(**dict(kw, num_ceps=0))
    assert spec.lds_bytes() == need and spec.nnz == nnz
    if (N, P) == (100, 128):
        assert sum(1 for _, w in filt if not w) == 1
    frames = 2 * F + 1
    x = np.clip(np.rint(np.random.default_rng(P).standard_normal(N + (frames - 1) * S + 1) * 3000), -32768, 32767).astype(np.int16)
    m, l, c = MR.stages(x, **ref_kw(spec))
    bl, bc = MR.mfcc_fp32_baseline(x, **ref_kw(spec))
    one = (x, np.array([[0, x.shape[0]]], np.int64), np.array([0, frames], np.int32), frames)
    _, lout = run(eng, *one, fb, extra=1)
    assert (lout[frames:] == CANARY).all() and np.isfinite(lout[:frames]).all()
    got, want = mel_figures(lout[:frames], m), mel_figures(bl, m)
    assert got[2] >= 0.95
    assert got[0] <= 4 * max(want[0], got[3]) and got[1] <= 4 * max(want[1], got[3]), (got, want)
    if C:
        _, cout = run(eng, *one, spec, extra=1)
        assert (cout[frames:] == CANARY).all()
        check_dct(cout[:frames], lout[:frames], W.dct_table(spec))
        e, eb = end_figures(cout[:frames], c), end_figures(bc, c)
        assert e[0] <= 4 * max(eb[0], e[1]), (e, eb)


def test_hostile_tables(eng, case):
    """a mel_seg whose entries point outside the spectrum and past nnz: the launch completes, the output is finite, the canaries hold
    (run checks them), and the filters left alone keep their bits.  Nothing is provoked: the clamps of the kernel are what is checked."""
    F, sig, count, ref, base = case
    blob, seg, offsets = layout(sig, NAMES, PADS, SLACK, 0)
    out_rows = int(offsets[-1])
    mseg, mw = W.mel_table(MFCC)
    bad = mseg.copy()
    big = 2 ** 31 - 1
    bad[0] = (-5, 7, -3)
    bad[1] = (big, big, big)
    bad[2] = (255, big, 467)
    bad[3] = (10, -4, 10)
    bad[4] = (100, 200, 460)
    bad[5] = (-big - 1, -big - 1, -big - 1)
    _, good = run(eng, blob, seg, offsets, out_rows, FBANK)
    _, out = run(eng, blob, seg, offsets, out_rows, FBANK, mel_seg=bad)
    used = good != CANARY
    assert ((out != CANARY) == used).all() and np.isfinite(out[used]).all()
    assert out[:, 6:].tobytes() == good[:, 6:].tobytes()
    _, cout = run(eng, blob, seg, offsets, out_rows, MFCC, mel_seg=bad)
    assert np.isfinite(cout[cout != CANARY]).all()
