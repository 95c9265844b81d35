"""The waveform side of the data path: 16-bit PCM -> the 257-dim log-power-spectrum (LPS) frames the recipes take as inputs (the
reference's README names Kaldi's compute-spectrogram-feats with a Hamming window as their source).  The definition -- the one stated at
rsrgan_feat_wave in include/rsrgan.h -- is compute-spectrogram-feats --dither=0 --window-type=hamming with Kaldi's other defaults:

    samples   int16 PCM widened to float without scaling; float input is taken as already on that scale
    frames    F = 0 if n < N else 1 + (n - N) // S (snip-edges); frame f is samples [f * S, f * S + N)
    per frame v -= sum(v) / N;  E = log(max(sum(v ** 2), eps));  v'[i] = v[i] - 0.97 * v[i - 1] (v'[0] = v[0] - 0.97 * v[0]);
              v' *= window;  zero-pad to P;  p = |DFT_P(v')| ** 2;  out[k] = log(max(p[k], eps)) for k >= 1, out[0] = E

with N = 400, S = 160, P = 512, eps = FLT_EPSILON (WaveSpec holds them).  lps_from_wave is the HOST route (float64 NumPy, one rounding
to float32); the device route is HipEngine.op_feat_wave / featurize(WaveBatch) / StreamBank.push_audio (csrc/wave.hip), which take the
window and the twiddles as tables built here in float64 and rounded once.

The labels of the recipes are another feature of the same audio: 40-dim MFCC (Kaldi's compute-mfcc-feats with the WSJ mfcc_hires.conf),
stated at rsrgan_feat_mfcc in include/rsrgan.h.  MfccSpec holds its parameters, mel_table / dct_table build the filterbank and the
liftered DCT the kernel takes as tables, mfcc_from_wave is the host route; the device route is HipEngine.op_feat_mfcc /
featurize(WaveBatch with an MfccSpec) (csrc/wave.hip k_feat_mfcc).  io/wave_reader.py reads training batches from two wav.scp files.

The way back is wave_from_lps: enhanced LPS rows and the samples they came from -> samples (the row's magnitude, the samples' phase,
weighted overlap-add, de-emphasis), stated at rsrgan_wave_synth in include/rsrgan.h; the device route is HipEngine.op_wave_synth /
synthesize (csrc/synth.hip).  quantize_pcm and write_wav take the result to a 16-bit RIFF file, read_wav's inverse."""
from __future__ import annotations

import wave as _wave

import numpy as np

EPS = float(np.finfo(np.float32).eps)
KIND_INT16, KIND_FLOAT32 = 0, 1                # the `kind` of include/rsrgan.h rsrgan_feat_wave
WINDOWS = ("hamming", "povey")


class WaveSpec(object):
    """the framing of the front end: frame_length N, frame_shift S, padded P (a power of two in [64, 2048], 1 <= S <= N <= P), preemph
    in [0, 1], window 'hamming' | 'povey', the sample rate read_wav expects"""

    def __init__(self, frame_length=400, frame_shift=160, padded=512, preemph=0.97, window="hamming", sample_rate=16000):
        self.frame_length, self.frame_shift, self.padded = int(frame_length), int(frame_shift), int(padded)
        self.preemph, self.window, self.sample_rate = float(preemph), str(window), int(sample_rate)
        P = self.padded
        if P < 64 or P > 2048 or P & (P - 1):
            raise ValueError("padded = %d is no power of two in [64, 2048]" % P)
        if not 1 <= self.frame_shift <= self.frame_length <= P:
            raise ValueError("frame_length = %d, frame_shift = %d, padded = %d outside 1 <= shift <= length <= padded" % (
                self.frame_length, self.frame_shift, P))
        if not 0.0 <= self.preemph <= 1.0:
            raise ValueError("preemph = %r outside [0, 1]" % preemph)
        if self.window not in WINDOWS:
            raise ValueError("window %r is none of %s" % (window, WINDOWS))

    @property
    def bins(self):
        return self.padded // 2 + 1

    def key(self):
        return (self.frame_length, self.frame_shift, self.padded, self.preemph, self.window)


DEFAULT = WaveSpec()


def _frames_per_workgroup(P):
    """csrc/wave.hip wave_frames: the frames a workgroup takes"""
    return 8 if P <= 1024 else 2


class MfccSpec(WaveSpec):
    """the labels' front end (include/rsrgan.h rsrgan_feat_mfcc): WaveSpec's framing, Povey window by default, then num_mel_bins M
    triangular mel filters between low_freq and high_freq (a high_freq <= 0 is an offset from Nyquist), the log, and num_ceps C rows of
    the DCT with the cepstral lifter Q multiplied in (Q = 0: none).  num_ceps = 0 means log-mel output (Kaldi's fbank features).  The
    defaults are compute-mfcc-feats with the WSJ conf/mfcc_hires.conf.  Refused: M outside [1, 128], C outside [0, M], not
    0 <= low < high <= Nyquist, a negative lifter, a table of no or more than 8192 weights, a launch above 64 KB of LDS."""

    def __init__(self, frame_length=400, frame_shift=160, padded=512, preemph=0.97, window="povey", sample_rate=16000, num_mel_bins=40,
                 num_ceps=40, low_freq=20.0, high_freq=-400.0, cepstral_lifter=22.0):
        WaveSpec.__init__(self, frame_length, frame_shift, padded, preemph, window, sample_rate)
        self.num_mel_bins, self.num_ceps = int(num_mel_bins), int(num_ceps)
        self.low_freq, self.high_freq, self.cepstral_lifter = float(low_freq), float(high_freq), float(cepstral_lifter)
        M, C = self.num_mel_bins, self.num_ceps
        if not 1 <= M <= 128:
            raise ValueError("num_mel_bins = %d outside [1, 128]" % M)
        if not 0 <= C <= M:
            raise ValueError("num_ceps = %d outside [0, num_mel_bins = %d]" % (C, M))
        if self.sample_rate < 1:
            raise ValueError("sample_rate = %d must be positive" % self.sample_rate)
        lo, hi = self.band()
        if not 0.0 <= lo < hi <= 0.5 * self.sample_rate:
            raise ValueError("low_freq = %r, high_freq = %r: the band [%g, %g] Hz is not inside 0 <= low < high <= Nyquist = %g" % (
                low_freq, high_freq, lo, hi, 0.5 * self.sample_rate))
        if not self.cepstral_lifter >= 0.0:
            raise ValueError("cepstral_lifter = %r must be 0 (none) or positive" % cepstral_lifter)
        nnz = sum(w.shape[0] for _, w in _mel_filters(self))
        if not 1 <= nnz <= 8192:
            raise ValueError("the mel table holds %d weights, outside [1, 8192]" % nnz)
        self.nnz = nnz
        if self.lds_bytes() > 65536:
            raise ValueError("frame_length = %d, frame_shift = %d, padded = %d, num_mel_bins = %d, num_ceps = %d, %d weights need %d bytes of "
                             "LDS, above the kernel's 65536" % (self.frame_length, self.frame_shift, self.padded, M, C, nnz, self.lds_bytes()))

    def band(self):
        """(low, high) in Hz after the offset rule"""
        return self.low_freq, self.high_freq if self.high_freq > 0.0 else 0.5 * self.sample_rate + self.high_freq

    def lds_bytes(self):
        """the dynamic LDS of the launch (include/rsrgan.h rsrgan_feat_mfcc states the formula)"""
        N, S, P, M, C = self.frame_length, self.frame_shift, self.padded, self.num_mel_bins, self.num_ceps
        F, H = _frames_per_workgroup(P), P // 2
        nz = min(4, F)
        return 8 * (H + nz * H) + 4 * (2 * N + (F - 1) * S) + 4 * (nz * H + nz * M + M * C + 3 * M + self.nnz)

    @property
    def bins(self):
        return self.num_ceps if self.num_ceps else self.num_mel_bins

    def key(self):
        return WaveSpec.key(self) + ("mfcc", self.sample_rate, self.num_mel_bins, self.num_ceps, self.low_freq, self.high_freq,
                                     self.cepstral_lifter)


_FILTERS, _DCTS = {}, {}          # the float64 tables of the host route, kept per (the fields they depend on): built once, read-only


def _mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)


def _mel_filters(spec):
    """[(first bin a_j, float64 weights [n_j])] of the M filters over the bins [0, P / 2) (Kaldi's MelBanks: the Nyquist bin never enters)"""
    M, P = spec.num_mel_bins, spec.padded
    lo, hi = spec.band()
    ck = (P, spec.sample_rate, M, lo, hi)
    if ck in _FILTERS:
        return _FILTERS[ck]
    mlo, mhi = float(_mel(lo)), float(_mel(hi))
    delta = (mhi - mlo) / (M + 1)
    mel = _mel(np.arange(P // 2, dtype=np.float64) * spec.sample_rate / P)
    out = []
    for j in range(M):
        left, centre, right = mlo + j * delta, mlo + (j + 1) * delta, mlo + (j + 2) * delta
        idx = np.flatnonzero((mel > left) & (mel < right))
        if idx.shape[0] == 0:
            out.append((0, np.zeros(0, np.float64)))
            continue
        a, n = int(idx[0]), int(idx.shape[0])
        assert int(idx[-1]) == a + n - 1                              # (mel ascends with the bin: a filter is contiguous)
        m = mel[a:a + n]
        out.append((a, np.where(m <= centre, (m - left) / (centre - left), (right - m) / (right - centre))))
    for _, w in out:
        w.setflags(write=False)
    if len(_FILTERS) > 16:
        _FILTERS.clear()
    _FILTERS[ck] = out
    return out


def mel_table(spec):
    """(mel_seg int32 [M, 3] = (first bin, bins, index of the first weight in mel_w), mel_w float32 [nnz]): built in float64, rounded once"""
    filt = _mel_filters(spec)
    seg, at = np.zeros((len(filt), 3), np.int32), 0
    for j, (a, w) in enumerate(filt):
        seg[j] = (a, w.shape[0], at)
        at += w.shape[0]
    return seg, np.ascontiguousarray(np.concatenate([w for _, w in filt]).astype(np.float32))


def _dct64(spec):
    """float64 [C, M]: Kaldi's ComputeDctMatrix (row 0 sqrt(1 / M), row k sqrt(2 / M) cos(pi / M (n + 1/2) k)), row i times the lifter
    1 + (Q / 2) sin(pi i / Q)"""
    M, C, Q = spec.num_mel_bins, spec.num_ceps, spec.cepstral_lifter
    if (M, C, Q) in _DCTS:
        return _DCTS[M, C, Q]
    k, n = np.arange(C, dtype=np.float64)[:, None], np.arange(M, dtype=np.float64)[None, :]
    d = np.sqrt(2.0 / M) * np.cos(np.pi / M * (n + 0.5) * k)
    d[:1] = np.sqrt(1.0 / M)
    if Q > 0.0:
        d *= 1.0 + 0.5 * Q * np.sin(np.pi * k / Q)
    d.setflags(write=False)
    if len(_DCTS) > 16:
        _DCTS.clear()
    _DCTS[M, C, Q] = d
    return d


def dct_table(spec):
    """float32 [C, M] row-major, the lifter multiplied in: built in float64, rounded once ([0, M] for log-mel output)"""
    return np.ascontiguousarray(_dct64(spec).astype(np.float32))


MFCC_DEFAULT = MfccSpec()


def mfcc_from_wave(x, spec=MFCC_DEFAULT):
    """the host route of the labels: samples [n] -> MFCC [F, C] (or log-mel [F, M] with num_ceps = 0) float32, the definition of
    rsrgan_feat_mfcc in float64 (np.fft.rfft, float64 tables), rounded once"""
    N, S, P = spec.frame_length, spec.frame_shift, spec.padded
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("samples must be a 1-D array, got shape %s" % (x.shape,))
    F = num_frames(x.shape[0], spec)
    if F == 0:
        return np.zeros((0, spec.bins), np.float32)
    v = x[np.arange(F)[:, None] * S + np.arange(N)[None, :]].astype(np.float64)
    v -= v.sum(1, keepdims=True) / N
    v = v - spec.preemph * np.concatenate([v[:, :1], v[:, :-1]], 1)
    v *= window_table(spec.window, N)
    X = np.fft.rfft(v, n=P, axis=1)
    p = X.real ** 2 + X.imag ** 2
    m = np.stack([p[:, a:a + w.shape[0]] @ w for a, w in _mel_filters(spec)], 1)
    out = np.log(np.maximum(m, EPS))
    if spec.num_ceps:
        out = out @ _dct64(spec).T
    return out.astype(np.float32)


def window_table(name="hamming", N=400):
    """float64 [N]: hamming 0.54 - 0.46 cos(2 pi i / (N - 1)); povey (0.5 - 0.5 cos(2 pi i / (N - 1))) ** 0.85"""
    if name not in WINDOWS:
        raise ValueError("window %r is none of %s" % (name, WINDOWS))
    c = np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / max(N - 1, 1))
    return 0.54 - 0.46 * c if name == "hamming" else (0.5 - 0.5 * c) ** 0.85


def twiddle_table(P=512):
    """float32 [P / 2, 2] = (cos, -sin)(2 pi j / P): exp(-2 pi i j / P) for the first half circle, float64 rounded once"""
    a = 2.0 * np.pi * np.arange(P // 2, dtype=np.float64) / P
    return np.ascontiguousarray(np.stack([np.cos(a), -np.sin(a)], 1).astype(np.float32))


def num_frames(n, spec=DEFAULT):
    """frames of an utterance of n samples (snip-edges)"""
    n = int(n)
    return 0 if n < spec.frame_length else 1 + (n - spec.frame_length) // spec.frame_shift


def as_pcm(x, what="samples"):
    """a 1-D sample array as the front end ships it: int16 stays int16, everything else becomes float32 (on the int16 scale)"""
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("%s must be a 1-D array of samples, got shape %s" % (what, x.shape))
    if x.dtype == np.int16:
        return np.ascontiguousarray(x)
    if x.dtype.kind not in "iuf":
        raise ValueError("%s must be int16 or floating-point samples, got %s" % (what, x.dtype))
    return np.ascontiguousarray(x, np.float32)


def lps_from_wave(x, window="hamming", spec=None):
    """the host route: samples [n] -> LPS [F, P / 2 + 1] float32, the definition above in float64 (np.fft.rfft), rounded once"""
    spec = WaveSpec(window=window) if spec is None else spec
    N, S, P = spec.frame_length, spec.frame_shift, spec.padded
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("samples must be a 1-D array, got shape %s" % (x.shape,))
    F = num_frames(x.shape[0], spec)
    if F == 0:
        return np.zeros((0, spec.bins), np.float32)
    v = x[np.arange(F)[:, None] * S + np.arange(N)[None, :]].astype(np.float64)
    v -= v.sum(1, keepdims=True) / N
    energy = np.log(np.maximum((v * v).sum(1), EPS))
    v = v - spec.preemph * np.concatenate([v[:, :1], v[:, :-1]], 1)
    v *= window_table(spec.window, N)
    X = np.fft.rfft(v, n=P, axis=1)
    out = np.log(np.maximum(X.real ** 2 + X.imag ** 2, EPS))
    out[:, 0] = energy
    return out.astype(np.float32)


def wave_from_lps(lps, samples, spec=DEFAULT):
    """the host route of audio out: LPS rows [rows, P / 2 + 1] (de-normalised, what lps_from_wave gives) and the samples [n] the frames
    came from -> float64 samples [n] on the int16 scale, the definition of rsrgan_wave_synth in float64 (np.fft, sequential de-emphasis).
    F = min(num_frames(n), rows); samples no frame covers are 0."""
    N, S, P, a = spec.frame_length, spec.frame_shift, spec.padded, spec.preemph
    x, lps = np.asarray(samples), np.asarray(lps)
    if x.ndim != 1:
        raise ValueError("samples must be a 1-D array, got shape %s" % (x.shape,))
    if lps.ndim != 2 or lps.shape[1] != P // 2 + 1:
        raise ValueError("lps must be [rows, %d], got shape %s" % (P // 2 + 1, lps.shape))
    n = x.shape[0]
    F = min(num_frames(n, spec), lps.shape[0])
    out = np.zeros(n, np.float64)
    if F == 0:
        return out
    w = window_table(spec.window, N)
    v = x[np.arange(F)[:, None] * S + np.arange(N)[None, :]].astype(np.float64)
    m = v.sum(1, keepdims=True) / N
    v -= m
    v = (v - a * np.concatenate([v[:, :1], v[:, :-1]], 1)) * w
    X = np.fft.rfft(v, n=P, axis=1)
    L = lps[:F].astype(np.float64)
    L = np.clip(np.where(np.isnan(L), -80.0, L), -80.0, 80.0)
    g = np.exp(0.5 * (L - np.log(np.maximum(X.real ** 2 + X.imag ** 2, EPS))))
    g[:, 0] = g[:, 1]
    y = np.fft.irfft(g * X, n=P, axis=1)[:, :N] + w * (1.0 - a) * m * g[:, 1:2]
    cov = (F - 1) * S + N
    num, den = np.zeros(cov, np.float64), np.zeros(cov, np.float64)
    w2 = w * w
    for f in range(F):                                                # (f ascending; sample 0 of a frame enters neither sum)
        num[f * S + 1:f * S + N] += w[1:] * y[f, 1:]
        den[f * S + 1:f * S + N] += w2[1:]
    z = np.where(den > 0.0, num / np.maximum(den, 1e-3), 0.0)
    prev = 0.0
    for t in range(cov):
        prev = out[t] = z[t] + a * prev
    return out


def quantize_pcm(y):
    """float samples on the int16 scale -> int16: rint, saturated to [-32768, 32767]"""
    return np.clip(np.rint(np.asarray(y, np.float64)), -32768.0, 32767.0).astype(np.int16)


def write_wav(path, samples, sample_rate=16000):
    """int16 samples [n] (anything else goes through quantize_pcm) -> a mono RIFF file of 16-bit PCM (stdlib `wave`): read_wav's inverse"""
    samples = np.asarray(samples)
    if samples.ndim != 1:
        raise ValueError("samples must be a 1-D array, got shape %s" % (samples.shape,))
    if samples.dtype != np.int16:
        samples = quantize_pcm(samples)
    with _wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sample_rate))
        f.writeframes(samples.astype("<i2").tobytes())


def read_wav(path, channel=0, sample_rate=16000):
    """a RIFF file of 16-bit PCM -> int16 [n] (stdlib `wave`): mono, or `channel` of an interleaved file.  ValueError for another sample
    width, another sample rate than `sample_rate` (None: any) or a channel the file does not have."""
    with _wave.open(str(path), "rb") as f:
        nch, width, rate, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        if width != 2:
            raise ValueError("%s: %d-bit samples; only 16-bit PCM is read" % (path, 8 * width))
        if sample_rate is not None and rate != int(sample_rate):
            raise ValueError("%s: sample rate %d Hz, expected %d Hz (the frames are 25 ms / 10 ms at that rate)" % (path, rate, int(sample_rate)))
        if not 0 <= int(channel) < nch:
            raise ValueError("%s: channel %d of a file with %d" % (path, int(channel), nch))
        data = np.frombuffer(f.readframes(n), "<i2")
    return np.ascontiguousarray(data.reshape(-1, nch)[:, int(channel)]).astype(np.int16)


def read_wav_scp(path):
    """lines `utt path` -> [(utt, path)].  A piped entry (`utt command |`, Kaldi's way to run sox per utterance) is refused: this reader
    starts no processes."""
    items = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            parts = line.split(None, 1)
            if len(parts) != 2:
                raise ValueError("%s:%d: expected `utt path`, got %r" % (path, no, line))
            if parts[1].rstrip().endswith("|") or parts[1].lstrip().startswith("|"):
                raise ValueError("%s:%d: %s is a piped entry (%r); only plain file paths are read -- write the audio to files first" % (
                    path, no, parts[0], parts[1]))
            items.append((parts[0], parts[1].strip()))
    return items


class WaveBatch(object):
    """CodedBatch's sibling for audio: the utterances' SAMPLES, to become LPS frames, then normalised, spliced and padded on the device
    (HipEngine.featurize, csrc/wave.hip k_feat_wave).  `samples` int16 or float32 [n]: the utterances one after the other; `seg` int64
    [B, 2] = (first sample, sample count); `offsets` int32 [B + 1]: utterance b has offsets[b + 1] - offsets[b] = num_frames(count)
    frames; `shape` = (B, T, bins * (left + 1 + right)); `left`, `right`, `mean`, `stddev` as in PackedBatch; `spec` the framing.  The
    constructor checks what the device cannot: every segment inside the samples and the offsets the frame counts.  `plan` (an
    io.reverb.ReverbPlan of B draws, or None): the samples are CLEAN audio, to be reverberated on the device before the frames are made
    (HipEngine.simulate, csrc/reverb.hip); the plan's spec shifts, so the frame counts are those of the clean samples."""

    def __init__(self, samples, seg, offsets, shape, left=0, right=0, mean=None, stddev=None, spec=DEFAULT, plan=None):
        self.samples, self.seg, self.offsets, self.spec, self.plan = samples, seg, offsets, spec, plan
        self.shape = tuple(int(v) for v in shape)
        self.left, self.right, self.mean, self.stddev = int(left), int(right), mean, stddev
        B, C = self.shape[0], self.left + 1 + self.right
        if self.shape[2] != spec.bins * C:
            raise ValueError("shape[2] = %d is not bins * (left + 1 + right) = %d * %d" % (self.shape[2], spec.bins, C))
        self.dim = spec.bins
        if plan is not None and (len(plan) != B or not plan.spec.shift):
            raise ValueError("the plan holds %d draws for %d utterances, or does not shift (the frame counts would differ)" % (len(plan), B))
        if samples.ndim != 1 or samples.dtype not in (np.int16, np.float32):
            raise ValueError("samples must be a flat int16 or float32 array, got %s %s" % (samples.dtype, samples.shape))
        if offsets.shape != (B + 1,) or offsets.dtype != np.int32:
            raise ValueError("offsets must hold B + 1 = %d int32 entries, got %s %s" % (B + 1, offsets.dtype, offsets.shape))
        if seg.shape != (B, 2) or seg.dtype != np.int64:
            raise ValueError("seg must be int64 [%d, 2], got %s %s" % (B, seg.dtype, seg.shape))
        if offsets[0] != 0:
            raise ValueError("offsets must start at 0")
        for b in range(B):
            first, count = int(seg[b, 0]), int(seg[b, 1])
            if first < 0 or count < 0 or first + count > samples.shape[0]:
                raise ValueError("utterance %d: samples [%d, %d) do not lie in the %d packed samples" % (b, first, first + count, samples.shape[0]))
            if int(offsets[b + 1]) - int(offsets[b]) != num_frames(count, spec):
                raise ValueError("utterance %d: offsets give it %d frames, its %d samples make %d" % (
                    b, int(offsets[b + 1]) - int(offsets[b]), count, num_frames(count, spec)))

    @property
    def kind(self):
        return KIND_INT16 if self.samples.dtype == np.int16 else KIND_FLOAT32

    def __len__(self):
        return self.shape[0]

    def lengths(self):
        """frames of every utterance after truncation at T (int32 [B]): what the splice kernel writes as `lengths`"""
        return np.minimum(np.diff(self.offsets), self.shape[1]).astype(np.int32)

    def nbytes(self):
        """what travels to the device: the samples and the two tables"""
        return int(self.samples.nbytes + self.seg.nbytes + self.offsets.nbytes) + (self.plan.nbytes() if self.plan is not None else 0)

    def rows(self, lo, hi):
        """utterances [lo, hi) as a batch of their own (GAN_RNN._shard): only their samples, both tables rebased to 0, the same T"""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= self.shape[0]:
            raise ValueError("rows [%d, %d) outside the batch of %d" % (lo, hi, self.shape[0]))
        utts = [self.samples[int(a):int(a) + int(n)] for a, n in self.seg[lo:hi]]
        plan = self.plan.rows(lo, hi) if self.plan is not None else None
        return pack_wave(utts, self.shape[1], self.left, self.right, self.mean, self.stddev, self.spec, plan=plan) if utts else \
            WaveBatch(self.samples[:0], self.seg[:0], np.zeros(1, np.int32), (0,) + self.shape[1:], self.left, self.right, self.mean,
                      self.stddev, self.spec, plan)


def pack_wave(utts, T=None, left=0, right=0, mean=None, stddev=None, spec=DEFAULT, names=None, plan=None):
    """sample arrays [n_i] (int16, or floats on the int16 scale) -> WaveBatch padded to T frames (default: the longest).  The samples are
    copied once, int16 if every utterance is, float32 otherwise; nothing is computed."""
    pcm = [as_pcm(u, "utterance %s" % (names[i] if names is not None else i)) for i, u in enumerate(utts)]
    if not pcm:
        raise ValueError("pack_wave: no utterances")
    dtype = np.int16 if all(u.dtype == np.int16 for u in pcm) else np.float32
    counts = np.array([u.shape[0] for u in pcm], np.int64)
    first = np.zeros(len(pcm), np.int64)
    np.cumsum(counts[:-1], out=first[1:])
    frames = [num_frames(n, spec) for n in counts]
    offsets = np.zeros(len(pcm) + 1, np.int64)
    np.cumsum(frames, out=offsets[1:])
    if offsets[-1] >= 2 ** 31:
        raise ValueError("a batch of %d frames does not fit the int32 offset table" % offsets[-1])
    samples = np.concatenate([u.astype(dtype, copy=False) for u in pcm], 0)
    return WaveBatch(samples, np.stack([first, counts], 1), offsets.astype(np.int32),
                     (len(pcm), max(frames) if T is None else int(T), spec.bins * (left + 1 + right)), left, right, mean, stddev, spec, plan)
