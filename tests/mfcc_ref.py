"""The MFCC / log-mel front end (include/rsrgan.h rsrgan_feat_mfcc) written out in float64, independent of rsrgan_amd/io/wave.py: explicit
loops over filters, bins and coefficients, math.log / math.cos / math.sin, the power spectrum from tests/wave_ref.frames (a product with
the DFT matrix, no FFT).  stages() returns the mel energies unclamped and unlogged, their logs and the cepstra, which is what the error
figures of the GPU tests are stated in.  mfcc_fp32_baseline: the same steps in float32 on the CPU with torch.fft.rfft and float32
tables -- what an ordinary fp32 implementation reaches, the yardstick of those figures."""
import functools
import math

import numpy as np

from tests import wave_ref as R

EPS = R.EPS


def mel(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


@functools.lru_cache(maxsize=None)
def filters(P=512, M=40, rate=16000, low=20.0, high=-400.0):
    """[(first bin, [weights])] of the M filters over the bins 0 .. P / 2 - 1; an empty filter is (0, [])"""
    hi = high if high > 0 else 0.5 * rate + high
    mlo, mhi = mel(low), mel(hi)
    delta = (mhi - mlo) / (M + 1)
    out = []
    for j in range(M):
        left, centre, right = mlo + j * delta, mlo + (j + 1) * delta, mlo + (j + 2) * delta
        first, w = 0, []
        for i in range(P // 2):
            m = mel(i * rate / P)
            if left < m < right:
                if not w:
                    first = i
                assert i == first + len(w), "a filter with a hole"
                w.append((m - left) / (centre - left) if m <= centre else (right - m) / (right - centre))
        out.append((first, w))
    return out


@functools.lru_cache(maxsize=None)
def dct(M=40, C=40, Q=22.0):
    """[C][M] float64: Kaldi's ComputeDctMatrix, row i times the lifter 1 + (Q / 2) sin(pi i / Q) (Q = 0: none)"""
    d = np.zeros((C, M))
    for i in range(C):
        lift = 1.0 + 0.5 * Q * math.sin(math.pi * i / Q) if Q > 0 else 1.0
        for n in range(M):
            d[i, n] = lift * (math.sqrt(1.0 / M) if i == 0 else math.sqrt(2.0 / M) * math.cos(math.pi / M * (n + 0.5) * i))
    return d


def stages(x, win="povey", N=R.N, S=R.S, P=R.P, coef=R.COEF, M=40, C=40, rate=16000, low=20.0, high=-400.0, Q=22.0):
    """samples [n] -> (m [F, M] mel energies, l [F, M] = log max(m, eps), c [F, C] cepstra), float64, nothing rounded"""
    _, p = R.frames(x, win, N=N, S=S, P=P, coef=coef)
    filt, F = filters(P, M, rate, low, high), p.shape[0]
    m, l = np.zeros((F, M)), np.zeros((F, M))
    for f in range(F):
        for j, (a, w) in enumerate(filt):
            s = 0.0
            for t, wt in enumerate(w):
                s += wt * p[f, a + t]
            m[f, j] = s
            l[f, j] = math.log(max(s, EPS))
    d = dct(M, C, Q)
    c = np.zeros((F, C))
    for f in range(F):
        for i in range(C):
            s = 0.0
            for j in range(M):
                s += d[i, j] * l[f, j]
            c[f, i] = s
    return m, l, c


def mfcc_fp32_baseline(x, win="povey", N=R.N, S=R.S, P=R.P, coef=R.COEF, M=40, C=40, rate=16000, low=20.0, high=-400.0, Q=22.0):
    """the same steps in float32 on the CPU (torch.fft.rfft, float32 tables, torch.matmul for the two sums): (l [F, M], c [F, C]) float32"""
    import torch
    x = torch.from_numpy(np.asarray(x).astype(np.float32))
    F = R.frame_count(x.shape[0], N, S)
    if F == 0:
        return np.zeros((0, M), np.float32), np.zeros((0, C), np.float32)
    v = x.unfold(0, N, S)[:F].clone()
    v = v - v.sum(1, keepdim=True) / np.float32(N)
    v = v - np.float32(coef) * torch.cat([v[:, :1], v[:, :-1]], 1)
    v = v * torch.from_numpy(R.window(win, N).astype(np.float32))
    X = torch.fft.rfft(v, n=P, dim=1)
    p = (X.real ** 2 + X.imag ** 2)[:, :P // 2]
    bank = np.zeros((M, P // 2), np.float32)
    for j, (a, w) in enumerate(filters(P, M, rate, low, high)):
        bank[j, a:a + len(w)] = np.asarray(w, np.float64).astype(np.float32)
    l = torch.log(torch.clamp(p @ torch.from_numpy(bank).T, min=EPS))
    c = l @ torch.from_numpy(dct(M, C, Q).astype(np.float32)).T if C else l[:, :0]
    return l.numpy().astype(np.float32), c.numpy().astype(np.float32)
