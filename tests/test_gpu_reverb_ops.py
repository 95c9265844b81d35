"""rsrgan_wave_reverb (csrc/reverb.hip) through HipEngine.op_wave_reverb against the float64 definition of tests/reverb_ref.py.

C = 64 (blocks of 32 samples) unless a case says otherwise; all utterances of a launch lie in ONE batch, their outputs in a banded canary
buffer with a gap of canaries behind each.  The batch: every n in {1, 31, 32, 33, 69, 227} against every L in {1, 32, 33, 103} (peak at
tap 0, in the middle, at the last tap), and the special cases of CASES below (noise: none, shorter than the utterance and wrapping,
starting late, starting past the end, m = 0, a zero noise; no RIR with and without noise; an all-zero utterance; a capacity below
n_out); utterances start at odd and even samples; both kinds of PCM; shift and normalize each on and off.  One case at C = 1024 and one
at C = 2048 with n = 16000, L = 4000.  No case feeds tables that point outside their buffers.

Checks: per utterance e = max |out - ref| / rms(ref); an utterance whose reference is all zero must be exactly zero.  The bound is NOT a
constant: it is 4 x the largest e that reverb_ref.reverb_fp32_yardstick (the same definition, its convolutions done as one float32
torch.fft.rfft / irfft on the CPU) reaches over this file's cases, evaluated here at run time.  Why 4: the kernel sums up to ceil(L / 32)
spectral products per block and uses table twiddles; a float32 emulation of the partitioned route stays below 1 x, so a kernel above 4 x
has an error in it, not rounding.  Both figures are printed with -s (profiles/reverb.txt holds them).  Further: the canaries and
everything past each capacity are untouched; the bits are equal across two runs, between the two sample kinds, across a permuted batch
and across B = 1 against B = 9; gains agree with the reference to 1e-5 relative; device_status() == 0."""
import numpy as np
import pytest
import torch

from rsrgan_amd.io import reverb as RV
from rsrgan_amd.io.wave import twiddle_table
from tests import reverb_ref as RR
from tests.helpers import build_hip_pair, small_cfg

pytestmark = pytest.mark.gpu

BAND, GAP, CANARY = 64, 5, -12345.5
RATE = 1000                                    # of the RIR columns: [e0, e1) = [q - 1, q + 50), so the early part is a true sub-range at L = 103
NS, LS = (1, 31, 32, 33, 69, 227), (1, 32, 33, 103)
FLAGS = [(True, True), (False, False), (True, False), (False, True)]


def _rirs():
    rng = np.random.default_rng(7)
    out = []
    for L, q in ((1, 0), (32, 0), (33, 16), (103, 102), (103, 40)):
        h = (rng.standard_normal(L) * 0.2 * np.exp(-np.arange(L) / 30.0)).astype(np.float32)
        h[q] = 1.5                                                   # the peak: tap 0, the middle, the last tap
        out.append(h)
    return out


def _noises():
    rng = np.random.default_rng(8)
    return [(rng.standard_normal(50) * 900).astype(np.float32), (rng.standard_normal(300) * 400).astype(np.float32), np.zeros(40, np.float32)]


RIR_OF_L = {1: 0, 32: 1, 33: 2, 103: 3}
# (n, rir index, noise index, s, m, snr, capacity or None, all-zero)
CASES = [(32, 1, 0, 0, 63, 10.0, None, False),          # a noise shorter than the utterance, wrapping, over all of y
         (69, 3, 1, 50, 121, 5.0, None, False),         # starting late
         (227, 4, 0, 3, 200, 20.0, None, False),        # wrapping four times, ending early
         (227, 3, 1, 10000, 50, 10.0, None, False),     # starting past the end
         (69, 4, 0, 0, 0, 10.0, None, False),           # m = 0
         (227, 2, 2, 0, 259, 10.0, None, False),        # a zero noise: P_v = 0
         (69, 4, 0, 0, 171, 10.0, None, True),          # an all-zero utterance
         (227, -1, 0, 5, 100, 15.0, None, False),       # no RIR, a noise: E = P_in
         (227, -1, -1, 0, 0, 0.0, None, False),         # no RIR, no noise
         (33, 1, -1, 0, 0, 0.0, 20, False),             # a capacity below n_out
         (32, 3, 1, 7, 100, 8.0, None, False),          # n < L
         (227, 4, 1, 0, 329, 12.0, 100, False)]         # noise and a short capacity


def _utts():
    rng = np.random.default_rng(9)
    utts = [(n, RIR_OF_L[L] if (L != 103 or i % 2) else 4, -1, 0, 0, 0.0, None, False) for i, n in enumerate(NS) for L in LS] + CASES
    sig = []
    for n, *_rest, zero in utts:
        sig.append(np.zeros(n, np.int16) if zero else np.clip(np.rint(rng.standard_normal(n) * 3000), -32768, 32767).astype(np.int16))
    return utts, sig


def _args(u, x, rirs, noises, shift, normalize, rate=RATE):
    n, r, v, s, m, snr = u[:6]
    return dict(x=x, h=rirs[r] if r >= 0 else None, cols=RR.rir_columns(rirs[r], rate) if r >= 0 else None,
                noise=noises[v] if v >= 0 else None, p_v=RR.noise_power(noises[v]) if v >= 0 else None, s=s, m=m, snr=snr, shift=shift,
                normalize=normalize)


def _big():
    rng = np.random.default_rng(11)
    x = np.clip(np.rint(rng.standard_normal(16000) * 3000), -32768, 32767).astype(np.int16)
    h = (rng.standard_normal(4000) * 0.1 * np.exp(-np.arange(4000) / 900.0)).astype(np.float32)
    h[37] = 1.0
    v = (rng.standard_normal(5000) * 500).astype(np.float32)
    return x, h, v


@pytest.fixture(scope="module")
def eng():
    model, _ = build_hip_pair(small_cfg("lstm"), 1, 4, seed=1)
    return model.engine


@pytest.fixture(scope="module")
def case():
    """the utterances, their float64 references per flag pair, and the yardstick's largest figure over ALL cases of the file (computed once)"""
    rirs, noises = _rirs(), _noises()
    utts, sig = _utts()
    ref, yard = {}, 0.0
    for fl in FLAGS:
        ref[fl] = [RR.reverb_ref(**_args(u, x, rirs, noises, *fl)) for u, x in zip(utts, sig)]
        for (u, x), (want, _) in zip(zip(utts, sig), ref[fl]):
            yard = max(yard, RR.figure(RR.reverb_fp32_yardstick(**_args(u, x, rirs, noises, *fl))[0], want))
    bx, bh, bv = _big()
    bargs = dict(x=bx, h=bh, cols=RR.rir_columns(bh, 16000), noise=bv, p_v=RR.noise_power(bv), s=1000, m=12000, snr=10.0, shift=True, normalize=True)
    bref = RR.reverb_ref(**bargs)
    yard_big = RR.figure(RR.reverb_fp32_yardstick(**bargs)[0], bref[0])
    return dict(rirs=rirs, noises=noises, utts=utts, sig=sig, ref=ref, big=(bx, bh, bv, bargs, bref), yard=max(yard, yard_big), yard_small=yard,
                yard_big=yard_big)


def run(eng, utts, sig, rirs, noises, shift, normalize, C=64, kind=0, rate=RATE, order=None):
    """one launch -> ([out of utterance i: the samples written], gains [B, 2], the whole buffer's bits).  Checks every canary."""
    dev = eng.device
    order = list(range(len(utts))) if order is None else order
    rir, rseg = RV.rir_table(rirs, rate)
    noise, nseg, npow = RV.noise_table(noises)
    parts, seg, at = [], [], 0
    for j, i in enumerate(order):
        pad = 1 + (j % 3)                                           # utterances start at odd and at even samples
        parts.append(np.full(pad, 77, np.int16)); at += pad
        seg.append((at, sig[i].shape[0])); parts.append(sig[i]); at += sig[i].shape[0]
    blob = np.concatenate(parts)
    if kind:
        blob = blob.astype(np.float32)
    assert len(seg) < 3 or (any(a % 2 for a, _ in seg) and any(a % 2 == 0 for a, _ in seg))
    sel = np.array([utts[i][1:5] for i in order], np.int32).reshape(-1, 4)
    snr = np.array([utts[i][5] for i in order], np.float32)
    oseg, writes, o = [], [], BAND
    for i in order:
        n, r = utts[i][0], utts[i][1]
        n_out = n if shift else n + (rirs[r].shape[0] if r >= 0 else 1) - 1
        cap = n_out if utts[i][6] is None else utts[i][6]
        oseg.append((o, cap)); writes.append(min(n_out, cap))
        o += max(cap, n_out) + GAP                                   # (a short capacity is followed by canaries where the rest would lie)
    buf = torch.full((o + BAND,), CANARY, dtype=torch.float32, device=dev)
    B = len(order)
    n_max, L_max = max(utts[i][0] for i in order), max(h.shape[0] for h in rirs)
    work = torch.zeros(eng.wave_reverb_work(B, n_max, L_max, C) + 32, dtype=torch.uint8, device=dev)
    work[-32:] = 0x5A
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tabs = [t(a) for a in (blob, np.array(seg, np.int64), rir, rseg, noise, nseg, npow, sel, snr, twiddle_table(2 * C), np.array(oseg, np.int64))]
    keep = [a.clone() for a in tabs]
    gains = torch.full((B + 1, 2), CANARY, dtype=torch.float32, device=dev)
    eng.op_wave_reverb(tabs[0], tabs[1], tabs[2], tabs[3], tabs[4], tabs[5], tabs[6], tabs[7], tabs[8], B, C, tabs[9], buf, tabs[10], work[:-32],
                       gains, shift, normalize)
    torch.cuda.synchronize()
    for a, b in zip(tabs, keep):
        assert torch.equal(a, b), "an input or a table was written"
    assert (work[-32:] == 0x5A).all(), "written past work"
    host, g = buf.cpu().numpy(), gains.cpu().numpy()
    assert (g[B] == CANARY).all()
    used = np.zeros(host.shape[0], bool)
    outs = [None] * len(utts)
    for j, i in enumerate(order):
        outs[i] = host[oseg[j][0]:oseg[j][0] + writes[j]].copy()
        used[oseg[j][0]:oseg[j][0] + writes[j]] = True
    assert (host[~used] == CANARY).all(), "written outside an utterance's min(n_out, capacity) samples"
    assert not (host[used] == CANARY).any(), "an utterance's samples were not all written"
    gg = np.zeros((len(utts), 2), np.float32)
    gg[order] = g[:B]
    return outs, gg, host.view(np.int32).copy()


def check(outs, gains, utts, refs, bound, lines, tag):
    """-> (the failures, the largest e)"""
    fails, worst = [], 0.0
    for i, (u, (want, (c, g))) in enumerate(zip(utts, refs)):
        got = outs[i]
        rms = float(np.sqrt((want * want).mean()))
        if rms == 0.0:
            e = 0.0 if not got.any() else float("inf")               # an all-zero reference: exactly zero
        else:
            e = float(np.abs(got - want[:got.shape[0]]).max() / rms)
        worst = max(worst, e)
        lines.append("%s utt %2d n %3d rir %2d noise %2d  e %.3e  (bound %.3e)  c %.6f g %.6f" % (tag, i, u[0], u[1], u[2], e, bound, gains[i, 0], gains[i, 1]))
        if not e <= bound:
            fails.append((tag, i, e))
        for got_g, want_g in ((gains[i, 0], c), (gains[i, 1], g)):
            if not abs(float(got_g) - want_g) <= 1e-5 * abs(want_g):
                fails.append((tag, i, "gain", float(got_g), want_g))
    return fails, worst


def test_against_float64_with_canaries(eng, case, capsys):
    utts, sig, rirs, noises = case["utts"], case["sig"], case["rirs"], case["noises"]
    bound = 4.0 * case["yard"]
    lines = ["yardstick (float32 rfft / irfft on this CPU): largest e %.3e over the C = 64 cases, %.3e for n = 16000, L = 4000; bound 4 x %.3e"
             % (case["yard_small"], case["yard_big"], case["yard"])]
    fails, worst = [], 0.0
    for fl in FLAGS:
        outs, gains, bits = run(eng, utts, sig, rirs, noises, *fl)
        f, w = check(outs, gains, utts, case["ref"][fl], bound, lines, "shift %d normalize %d" % fl)
        fails, worst = fails + f, max(worst, w)
        # run to run, and float32 samples on the same scale
        assert np.array_equal(bits, run(eng, utts, sig, rirs, noises, *fl)[2])
        assert np.array_equal(bits, run(eng, utts, sig, rirs, noises, *fl, kind=1)[2])
    lines.append("largest kernel e %.3e = %.2f x the yardstick" % (worst, worst / case["yard"]))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not fails, fails
    assert eng.device_status() == 0


def test_bits_do_not_depend_on_the_batch(eng, case):
    utts, sig, rirs, noises = case["utts"], case["sig"], case["rirs"], case["noises"]
    pick = [len(utts) - len(CASES) + k for k in (0, 1, 2, 5, 7, 9, 10)] + [3, 23]           # nine utterances: B = 9
    sub, ssig = [utts[i] for i in pick], [sig[i] for i in pick]
    outs, gains, _ = run(eng, sub, ssig, rirs, noises, True, True)
    perm = [4, 8, 0, 6, 2, 7, 1, 5, 3]
    outs2, gains2, _ = run(eng, sub, ssig, rirs, noises, True, True, order=perm)
    for a, b in zip(outs, outs2):
        assert a.tobytes() == b.tobytes()
    assert gains.tobytes() == gains2.tobytes()
    full, gfull, _ = run(eng, utts, sig, rirs, noises, True, True)
    for k, i in enumerate(pick):
        one, g1, _ = run(eng, [sub[k]], [ssig[k]], rirs, noises, True, True)                 # B = 1
        assert one[0].tobytes() == outs[k].tobytes() == full[i].tobytes(), k
        assert g1[0].tobytes() == gains[k].tobytes() == gfull[i].tobytes(), k
    assert eng.device_status() == 0


@pytest.mark.parametrize("C", [1024, 2048])
def test_long_utterance(eng, case, C, capsys):
    bx, bh, bv, bargs, (want, (c, g)) = case["big"]
    u = [(16000, 0, 0, bargs["s"], bargs["m"], bargs["snr"], None, False)]
    outs, gains, bits = run(eng, u, [bx], [bh], [bv], True, True, C=C, rate=16000)
    e = RR.figure(outs[0], want)
    with capsys.disabled():
        print("\nC = %d, n = 16000, L = 4000: e %.3e, yardstick %.3e (this case), bound 4 x %.3e; c %.6f g %.6f" % (C, e, case["yard_big"], case["yard"],
                                                                                                              gains[0, 0], gains[0, 1]))
    assert e <= 4.0 * case["yard"], (e, case["yard"])
    assert abs(float(gains[0, 0]) - c) <= 1e-5 * c and abs(float(gains[0, 1]) - g) <= 1e-5 * g
    assert np.array_equal(bits, run(eng, u, [bx], [bh], [bv], True, True, C=C, rate=16000)[2])
    assert eng.device_status() == 0
