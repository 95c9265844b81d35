"""Audio out (include/rsrgan.h rsrgan_wave_synth) written out frame by frame in float64, independent of rsrgan_amd/io/wave.py: explicit
loops over frames and samples, the window and the DFT matrix of tests/wave_ref.py (no FFT), the inverse transform as the real part of the
product with the conjugate matrix, a sequential de-emphasis.  synth_fp32_baseline: the same steps in float32 on the CPU with
torch.fft.rfft / irfft and a sequential float32 recurrence -- what an ordinary fp32 implementation reaches, the yardstick of the GPU
tests' figures."""
import numpy as np

from tests import wave_ref as R

N, S, P, COEF, EPS = R.N, R.S, R.P, R.COEF, R.EPS
LCLAMP, FLOOR = 80.0, 1e-3


def clamp_lps(L):
    L = np.asarray(L, np.float64)
    return np.clip(np.where(np.isnan(L), -LCLAMP, L), -LCLAMP, LCLAMP)


def synth(lps, x, win="hamming", N=N, S=S, P=P, coef=COEF):
    """LPS rows [rows, P / 2 + 1] and the samples [n] the frames came from -> float64 samples [n]"""
    x = np.asarray(x, np.float64)
    lps = np.asarray(lps)
    n, H = x.shape[0], P // 2
    F = min(R.frame_count(n, N, S), lps.shape[0])
    out = np.zeros(n, np.float64)
    if F == 0:
        return out
    w, M = R.window(win, N), R.dft_matrix(N, P)
    cov = (F - 1) * S + N
    num, den = np.zeros(cov), np.zeros(cov)
    weight = np.full(H + 1, 2.0)
    weight[0] = weight[H] = 1.0
    for f in range(F):
        v = x[f * S:f * S + N].copy()
        m = v.sum() / N
        v -= m
        old = v.copy()
        v[1:] = old[1:] - coef * old[:-1]
        v[0] = old[0] - coef * old[0]
        v *= w
        X = v @ M
        p = X.real ** 2 + X.imag ** 2
        g = np.exp((clamp_lps(lps[f]) - np.log(np.maximum(p, EPS))) / 2.0)
        g[0] = g[1]
        Y = g * X
        y = ((np.conj(M) * (weight * Y)[None, :]).real.sum(1)) / P
        y += w * (1.0 - coef) * m * g[1]
        for i in range(1, N):
            num[f * S + i] += w[i] * y[i]
            den[f * S + i] += w[i] * w[i]
    prev = 0.0
    for t in range(cov):
        z = num[t] / max(den[t], FLOOR) if den[t] > 0.0 else 0.0
        prev = z + coef * prev
        out[t] = prev
    return out


def synth_fp32_baseline(lps, x, win="hamming", N=N, S=S, P=P, coef=COEF):
    """the same steps in float32 on the CPU: torch.fft.rfft / irfft, a sequential float32 de-emphasis -> float32 [n]"""
    import torch
    x = torch.from_numpy(np.asarray(x).astype(np.float32))
    lps = np.asarray(lps)
    n = x.shape[0]
    F = min(R.frame_count(n, N, S), lps.shape[0])
    out = np.zeros(n, np.float32)
    if F == 0:
        return out
    f32 = np.float32
    w = torch.from_numpy(R.window(win, N).astype(np.float32))
    v = x.unfold(0, N, S)[:F].clone()
    m = v.sum(1, keepdim=True) / f32(N)
    v = v - m
    v = (v - f32(coef) * torch.cat([v[:, :1], v[:, :-1]], 1)) * w
    X = torch.fft.rfft(v, n=P, dim=1)
    L = torch.from_numpy(clamp_lps(lps[:F]).astype(np.float32))
    g = torch.exp((L - torch.log(torch.clamp(X.real ** 2 + X.imag ** 2, min=EPS))) * f32(0.5))
    g[:, 0] = g[:, 1]
    y = torch.fft.irfft(g * X, n=P, dim=1)[:, :N] + w * (f32(1.0) - f32(coef)) * m * g[:, 1:2]
    wy, w2 = (w * y).numpy(), (w * w).numpy()
    cov = (F - 1) * S + N
    num, den = np.zeros(cov, np.float32), np.zeros(cov, np.float32)
    for f in range(F):
        num[f * S + 1:f * S + N] += wy[f, 1:]
        den[f * S + 1:f * S + N] += w2[1:]
    z = np.where(den > 0, num / np.maximum(den, f32(FLOOR)), f32(0)).astype(np.float32)
    prev, c = f32(0), f32(coef)
    for t in range(cov):
        prev = f32(z[t] + c * prev)
        out[t] = prev
    return out


def figure(got, ref):
    """max |got - ref| / rms(ref) over every sample; a reference that is identically zero demands exact zeros (the figure is then 0 or inf)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.shape[0] == 0:
        return 0.0
    rms = float(np.sqrt((ref * ref).mean()))
    err = float(np.abs(got - ref).max())
    if rms == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / rms


def bound(base, ref):
    """4 x the larger of the fp32 baseline's figure and the float32 spacing at max |ref| over rms(ref)"""
    ref = np.asarray(ref, np.float64)
    if ref.shape[0] == 0 or not np.any(ref):
        return 0.0
    rms = float(np.sqrt((ref * ref).mean()))
    return 4.0 * max(figure(base, ref), float(R.ulp32(np.abs(ref).max())) / rms)
