"""The log-power-spectrum front end (include/rsrgan.h rsrgan_feat_wave) written out frame by frame in float64, independent of
rsrgan_amd/io/wave.py: explicit loops over frames, the window from math.cos, the transform as a product with the DFT matrix (whose
angles are reduced in integers first), no FFT.  frames() returns the energy and the POWER spectrum unclamped and unlogged, which is what
the error figures of the GPU tests are stated in.  lps_fp32_baseline: the same steps in float32 on the CPU with torch.fft.rfft -- what
an ordinary fp32 implementation reaches, the yardstick of those figures."""
import functools
import math

import numpy as np

N, S, P, COEF = 400, 160, 512, 0.97
NB = P // 2 + 1
EPS = float(np.finfo(np.float32).eps)


def frame_count(n, N=N, S=S):
    return 0 if n < N else 1 + (n - N) // S


@functools.lru_cache(maxsize=None)
def window(name="hamming", N=N):
    a = [math.cos(2.0 * math.pi * i / (N - 1)) for i in range(N)]
    if name == "hamming":
        return np.array([0.54 - 0.46 * c for c in a], np.float64)
    if name == "povey":
        return np.array([(0.5 - 0.5 * c) ** 0.85 for c in a], np.float64)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def dft_matrix(N=N, P=P):
    """[N, P / 2 + 1] complex128: exp(-2 pi i (j k mod P) / P); rows N .. P - 1 multiply the zero padding and are left out"""
    jk = (np.arange(N, dtype=np.int64)[:, None] * np.arange(P // 2 + 1, dtype=np.int64)[None, :]) % P
    ang = 2.0 * np.pi * jk.astype(np.float64) / P
    return np.cos(ang) - 1j * np.sin(ang)


def frames(x, win="hamming", N=N, S=S, P=P, coef=COEF):
    """samples [n] -> (E [F] float64 = the sum of squares of the mean-free frame, p [F, P / 2 + 1] float64 = |X_k|^2), nothing clamped"""
    x = np.asarray(x, np.float64)
    F = frame_count(x.shape[0], N, S)
    w, M = window(win, N), dft_matrix(N, P)
    E, p = np.zeros(F), np.zeros((F, P // 2 + 1))
    for f in range(F):
        v = x[f * S:f * S + N].copy()
        v -= v.sum() / N
        E[f] = float((v * v).sum())
        old = v.copy()
        v[1:] = old[1:] - coef * old[:-1]
        v[0] = old[0] - coef * old[0]
        v *= w
        X = v @ M
        p[f] = X.real ** 2 + X.imag ** 2
    return E, p


def lps(x, win="hamming", **kw):
    """the definition's output in float64 [F, P / 2 + 1] (not rounded)"""
    E, p = frames(x, win, **kw)
    out = np.log(np.maximum(p, EPS))
    out[:, 0] = np.log(np.maximum(E, EPS))
    return out


def lps_fp32_baseline(x, win="hamming", N=N, S=S, P=P, coef=COEF):
    """the same steps in float32 on the CPU, torch.fft.rfft for the transform: [F, P / 2 + 1] float32"""
    import torch
    x = torch.from_numpy(np.asarray(x).astype(np.float32))
    F = frame_count(x.shape[0], N, S)
    if F == 0:
        return np.zeros((0, P // 2 + 1), np.float32)
    v = x.unfold(0, N, S)[:F].clone()
    v = v - v.sum(1, keepdim=True) / np.float32(N)
    energy = torch.log(torch.clamp((v * v).sum(1), min=EPS))
    v = v - np.float32(coef) * torch.cat([v[:, :1], v[:, :-1]], 1)
    v = v * torch.from_numpy(window(win, N).astype(np.float32))
    X = torch.fft.rfft(v, n=P, dim=1)
    out = torch.log(torch.clamp(X.real ** 2 + X.imag ** 2, min=EPS))
    out[:, 0] = energy
    return out.numpy().astype(np.float32)


def ulp32(a):
    """the float32 spacing at |a|"""
    return np.spacing(np.abs(np.asarray(a, np.float32))).astype(np.float64)
