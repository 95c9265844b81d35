"""Data simulation for the dereverberation recipes: reverberant inputs made from the clean labels' audio and a list of room impulse
responses (RIRs), optionally with an additive noise at a random SNR, drawn afresh every epoch -- what the reference prepares offline with
Kaldi's wav-reverberate (reverberate/run.sh, steps/data/reverberate_bash.py).  The definition is the one stated at rsrgan_wave_reverb in
include/rsrgan.h:

    P_in = mean x^2;  y = x * h (full length n + L - 1);  E = mean (x * h[e0:e1])^2 with [e0, e1) the early part around the peak q;
    y[s + i] += g v[i mod nv], i < m, g = sqrt(10^(-snr / 10) E / P_v);  c = sqrt(P_in / mean y^2) (normalize);  out[i] = c y[i + q] (shift)

`reverberate` is the HOST route (float64, np.fft); the device route is HipEngine.op_wave_reverb / simulate / featurize(WaveBatch with a
plan) (csrc/reverb.hip).  The draws stay on the host: `draw` is a function of (seed, epoch, utterance index) alone, so io.prefetch may
materialize batches on several threads in any order."""
from __future__ import annotations

import random

import numpy as np

from .wave import read_wav, read_wav_scp

FFT_SIZES = (64, 128, 256, 512, 1024, 2048)
_M64 = (1 << 64) - 1


class ReverbSpec(object):
    """sample_rate; shift (drop the q samples before the RIR's peak: the output is as long as the input); normalize (the output keeps the
    input's power); fft, the complex FFT length C of the device route (a block is C / 2 samples; a power of two in [64, 2048]); snr =
    (lower, upper) dB, drawn uniformly; noise_prob, the probability that an utterance gets a noise when noises are given.
    The default fft is 1024, the fastest measured: 191 us for 32 utterances of 5 s against 0.5 s RIRs on an MI355X, against 259 us at 512
    and 249 us at 2048 (profiles/reverb.txt)."""

    def __init__(self, sample_rate=16000, shift=True, normalize=True, fft=1024, snr=(5.0, 20.0), noise_prob=1.0):
        self.sample_rate, self.shift, self.normalize, self.fft = int(sample_rate), bool(shift), bool(normalize), int(fft)
        self.snr, self.noise_prob = (float(snr[0]), float(snr[1])), float(noise_prob)
        if self.fft not in FFT_SIZES:
            raise ValueError("fft = %d is no power of two in [64, 2048]" % self.fft)
        if self.sample_rate < 1:
            raise ValueError("sample_rate = %d must be positive" % self.sample_rate)
        if not self.snr[0] <= self.snr[1]:
            raise ValueError("snr = (%g, %g): the lower bound is above the upper" % self.snr)
        if not 0.0 <= self.noise_prob <= 1.0:
            raise ValueError("noise_prob = %r outside [0, 1]" % noise_prob)


DEFAULT = ReverbSpec()


def read_rir_scp(path, sample_rate=16000):
    """lines `name path` -> [(name, float32 taps)]: 16-bit PCM wav files (the raw sample values, as wav-reverberate reads them) or .npy
    arrays of floats.  ValueError for an empty list or an RIR without taps."""
    out = []
    for name, p in read_wav_scp(path):
        h = np.load(p) if p.endswith(".npy") else read_wav(p, sample_rate=sample_rate)
        h = np.ascontiguousarray(h, np.float32).reshape(-1)
        if h.shape[0] < 1:
            raise ValueError("%s: %s holds no taps" % (path, name))
        out.append((name, h))
    if not out:
        raise ValueError("%s lists no files" % path)
    return out


def rir_columns(h, sample_rate=16000):
    """(q, e0, e1): q the index of the first maximum of h (Kaldi's Vector::Max), [e0, e1) = [max(q - floor(0.001 fs), 0),
    min(q + floor(0.05 fs), L)) the early part"""
    h = np.asarray(h, np.float64)
    q = int(np.argmax(h))
    return q, max(q - int(0.001 * sample_rate), 0), min(q + int(0.05 * sample_rate), h.shape[0])


def rir_table(rirs, sample_rate=16000):
    """arrays of taps -> (rir float32 [sum L], rir_seg int64 [R, 5] = (first tap, L, q, e0, e1)) as rsrgan_wave_reverb takes them"""
    rirs = [np.ascontiguousarray(h, np.float32).reshape(-1) for h in rirs]
    seg, at = np.zeros((len(rirs), 5), np.int64), 0
    for r, h in enumerate(rirs):
        if h.shape[0] < 1:
            raise ValueError("RIR %d holds no taps" % r)
        seg[r] = (at, h.shape[0]) + rir_columns(h, sample_rate)
        at += h.shape[0]
    return (np.concatenate(rirs) if rirs else np.zeros(0, np.float32)), seg


def noise_table(noises):
    """arrays of samples -> (noise float32 [sum nv], noise_seg int64 [V, 2] = (first, nv), noise_pow float32 [V]: the power in fp64, rounded
    once)"""
    noises = [np.ascontiguousarray(v, np.float32).reshape(-1) for v in noises]
    seg, pw, at = np.zeros((len(noises), 2), np.int64), np.zeros(len(noises), np.float32), 0
    for i, v in enumerate(noises):
        seg[i] = (at, v.shape[0])
        d = v.astype(np.float64)
        pw[i] = (d * d).sum() / v.shape[0] if v.shape[0] else 0.0
        at += v.shape[0]
    return (np.concatenate(noises) if noises else np.zeros(0, np.float32)), seg, pw


def _fftconv(x, h):
    n = x.shape[0] + h.shape[0] - 1
    size = 1 << max(int(n - 1).bit_length(), 1)
    return np.fft.irfft(np.fft.rfft(x, size) * np.fft.rfft(h, size), size)[:n]


def reverberate(x, h=None, noise=None, noise_pow=None, s=0, m=0, snr=0.0, shift=True, normalize=True, sample_rate=16000, gains=False):
    """the host route, float64: samples x [n] (int16 or floats on that scale), taps h (None: no RIR), noise samples (None: none) with
    their power (default: computed here), added from y[s] over a span of m samples, wrapping, at `snr` dB -> out float64 [n] with shift,
    [n + L - 1] without; gains=True: (out, (c, g))"""
    x = np.asarray(x).astype(np.float64).reshape(-1)
    n = x.shape[0]
    if n < 1:
        raise ValueError("reverberate: no samples")
    p_in = float((x * x).sum() / n)
    q, E = 0, p_in
    if h is None:
        y = x.copy()
    else:
        h = np.asarray(h).astype(np.float64).reshape(-1)
        q, e0, e1 = rir_columns(h, sample_rate)
        y = _fftconv(x, h)
        E = 0.0
        if noise is not None and e1 > e0:
            ye = _fftconv(x, h[e0:e1])
            E = float((ye * ye).sum() / (n + (e1 - e0) - 1))
    g = 0.0
    if noise is not None and len(noise):
        v = np.asarray(noise).astype(np.float64).reshape(-1)
        p_v = float((v * v).sum() / v.shape[0]) if noise_pow is None else float(noise_pow)
        if E > 0.0 and p_v > 0.0:
            g = float(np.sqrt(10.0 ** (-float(snr) / 10.0) * E / p_v))
        s = min(max(int(s), 0), y.shape[0])
        m = min(max(int(m), 0), y.shape[0] - s)
        if m and g:
            y[s:s + m] += g * v[np.arange(m) % v.shape[0]]
    c = 1.0
    if normalize:
        p_out = float((y * y).sum() / y.shape[0])
        if p_out > 0.0:
            c = float(np.sqrt(p_in / p_out))
    out = c * (y[q:q + n] if shift else y)
    return (out, (c, g)) if gains else out


def _rng(seed, epoch, utt_index):
    """random.Random from an explicit integer mix of (seed, epoch, utterance index): splitmix64's finaliser over their weighted sum"""
    z = (int(seed) * 0x9E3779B97F4A7C15 + int(epoch) * 0xBF58476D1CE4E5B9 + int(utt_index) * 0x94D049BB133111EB + 0x2545F4914F6CDD1D) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return random.Random(z ^ (z >> 31))


def draw(seed, epoch, utt_index, n, num_rirs, rir_lengths=None, num_noises=0, spec=DEFAULT):
    """the draw of one utterance of n samples: (rir index, noise index or -1, s, m, snr).  A function of its arguments alone: the same four
    variates are taken whatever the outcome.  The noise starts at a random sample of the utterance and runs to the end of y."""
    rng = _rng(seed, epoch, utt_index)
    u = [rng.random() for _ in range(4)]
    r = min(int(u[0] * num_rirs), num_rirs - 1) if num_rirs > 0 else -1
    L = int(rir_lengths[r]) if (r >= 0 and rir_lengths is not None) else 1
    v = -1
    if num_noises > 0 and u[1] < spec.noise_prob:
        v = min(int(u[1] / max(spec.noise_prob, 1e-300) * num_noises), num_noises - 1)
    s = min(int(u[2] * n), max(n - 1, 0)) if v >= 0 else 0
    m = n + L - 1 - s if v >= 0 else 0
    snr = spec.snr[0] + (spec.snr[1] - spec.snr[0]) * u[3]
    return r, v, s, m, float(snr)


class ReverbSim(object):
    """The simulation a WaveBatchReader runs on its labels' audio: the RIRs of `rir_scp`, the noises of `noise_scp` (None: none), a
    ReverbSpec and a seed.  `epoch` (set_epoch) selects the draws; cross-validation keeps epoch 0.  The packed tables (`bank`) are built
    once; HipEngine.reverb_bank uploads them once."""

    def __init__(self, rir_scp, noise_scp=None, spec=DEFAULT, seed=0):
        self.spec, self.seed, self.epoch = spec, int(seed), 0
        self.rirs = [h for _, h in read_rir_scp(rir_scp, spec.sample_rate)]
        self.noises = []
        if noise_scp:
            self.noises = [np.ascontiguousarray(read_wav(p, sample_rate=spec.sample_rate), np.float32) for _, p in read_wav_scp(noise_scp)]
            if not self.noises:
                raise ValueError("%s lists no files" % noise_scp)
        self.rir, self.rir_seg = rir_table(self.rirs, spec.sample_rate)
        self.noise, self.noise_seg, self.noise_pow = noise_table(self.noises)
        self.max_taps = int(self.rir_seg[:, 1].max())

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def draw(self, utt_index, n, epoch=None):
        return draw(self.seed, self.epoch if epoch is None else epoch, utt_index, n, len(self.rirs), self.rir_seg[:, 1], len(self.noises), self.spec)

    def plan(self, utt_indices, counts, epoch=None):
        """the ReverbPlan of a batch: the draws of its utterances (their indices in the reader, their sample counts)"""
        d = [self.draw(i, n, epoch) for i, n in zip(utt_indices, counts)]
        return ReverbPlan(self, np.array([t[:4] for t in d], np.int32).reshape(-1, 4), np.array([t[4] for t in d], np.float32))

    def apply(self, x, drawn):
        """the host route on one utterance with its draw"""
        r, v, s, m, snr = drawn
        return reverberate(x, self.rirs[r] if r >= 0 else None, self.noises[v] if v >= 0 else None, float(self.noise_pow[v]) if v >= 0 else None,
                           s, m, snr, self.spec.shift, self.spec.normalize, self.spec.sample_rate)


class ReverbPlan(object):
    """what a WaveBatch carries for the device route: the bank (a ReverbSim, or anything with its rir / rir_seg / noise / noise_seg /
    noise_pow / spec / max_taps members), sel int32 [B, 4] = (rir index, noise index, s, m) and snr float32 [B]"""

    def __init__(self, bank, sel, snr):
        self.bank, self.sel, self.snr = bank, np.ascontiguousarray(sel, np.int32), np.ascontiguousarray(snr, np.float32)
        if self.sel.ndim != 2 or self.sel.shape[1] != 4 or self.snr.shape != (self.sel.shape[0],):
            raise ValueError("sel must be int32 [B, 4] and snr float32 [B], got %s and %s" % (self.sel.shape, self.snr.shape))

    @property
    def spec(self):
        return self.bank.spec

    def __len__(self):
        return self.sel.shape[0]

    def rows(self, lo, hi):
        return ReverbPlan(self.bank, self.sel[lo:hi], self.snr[lo:hi])

    def nbytes(self):
        return int(self.sel.nbytes + self.snr.nbytes)


def sim_from_flags(FLAGS, split):
    """the ReverbSim of a split ("tr" / "cv") from --{split}_rir_scp, --noise_scp, --snr_lower, --snr_upper, --sim_seed; None without the flag"""
    rir = getattr(FLAGS, split + "_rir_scp", None)
    if not rir:
        return None
    spec = ReverbSpec(snr=(float(getattr(FLAGS, "snr_lower", 5.0)), float(getattr(FLAGS, "snr_upper", 20.0))))
    return ReverbSim(rir, getattr(FLAGS, "noise_scp", None) or None, spec, int(getattr(FLAGS, "sim_seed", 0)))


def add_sim_flags(p):
    """the simulation's flags of run_gan_rnn / run_rnn / io.wave_cmvn"""
    for split in ("tr", "cv"):
        p.add_argument("--%s_rir_scp" % split, type=str, default=None, help="train from CLEAN audio: a list `name path` of room impulse "
                       "responses (16-bit wav or .npy) in place of --%s_inputs_wav_scp; the inputs are the labels' audio reverberated with an "
                       "RIR drawn per utterance and epoch (io/reverb.py; with --device_features on the device, csrc/reverb.hip)" % split)
    p.add_argument("--noise_scp", type=str, default=None, help="with --*_rir_scp: a wav.scp of noises, one added per utterance at a random SNR")
    p.add_argument("--snr_lower", type=float, default=5.0, help="with --noise_scp: the lower end of the SNR range, dB")
    p.add_argument("--snr_upper", type=float, default=20.0, help="with --noise_scp: the upper end of the SNR range, dB")
    p.add_argument("--sim_seed", type=int, default=0, help="with --*_rir_scp: the seed of the draws (RIR, noise, SNR, start)")

