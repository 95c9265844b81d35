"""The reverberation of include/rsrgan.h rsrgan_wave_reverb written out in float64 with np.convolve and plain sums, independent of
rsrgan_amd/io/reverb.py; and the yardstick of tests/test_gpu_reverb_ops.py: the same definition with its convolutions done as ONE
float32 torch.fft.rfft / irfft on the CPU (what a single-precision FFT convolution costs, measured where the test runs)."""
import numpy as np
import torch


def rir_columns(h, rate=16000):
    """(q, e0, e1) of an RIR by a loop: q the index of the FIRST maximum, [e0, e1) = [max(q - floor(0.001 rate), 0), min(q + floor(0.05 rate), L))"""
    q, best = 0, None
    for i, v in enumerate(np.asarray(h, np.float64)):
        if best is None or v > best:
            q, best = i, v
    return q, max(q - int(0.001 * rate), 0), min(q + int(0.05 * rate), len(h))


def noise_power(v):
    v = np.asarray(v, np.float64)
    return float((v * v).sum() / v.shape[0]) if v.shape[0] else 0.0


def _conv64(x, h):
    return np.convolve(x, h)


def _conv32(x, h):
    n = x.shape[0] + h.shape[0] - 1
    size = 1 << max(int(n - 1).bit_length(), 1)
    X = torch.fft.rfft(torch.from_numpy(x.astype(np.float32)), n=size)
    H = torch.fft.rfft(torch.from_numpy(h.astype(np.float32)), n=size)
    return torch.fft.irfft(X * H, n=size)[:n].numpy().astype(np.float64)


def _reverb(conv, x, h=None, cols=None, noise=None, p_v=None, s=0, m=0, snr=0.0, shift=True, normalize=True):
    x = np.asarray(x).astype(np.float64)
    n = x.shape[0]
    p_in = float((x * x).sum() / n)
    if h is None:
        y, q, E = x.copy(), 0, p_in
    else:
        h = np.asarray(h).astype(np.float64)
        q, e0, e1 = cols
        y = conv(x, h)
        E = 0.0
        if noise is not None and e1 > e0:
            ye = conv(x, h[e0:e1])
            E = float((ye * ye).sum() / (n + (e1 - e0) - 1))
    g = 0.0
    if noise is not None and len(noise):
        v = np.asarray(noise).astype(np.float64)
        if E > 0.0 and p_v > 0.0:
            g = float(np.sqrt(10.0 ** (-snr / 10.0) * E / p_v))
        for i in range(m):
            if s + i >= y.shape[0]:
                break
            y[s + i] += g * v[i % v.shape[0]]
    c = 1.0
    if normalize:
        p_out = float((y * y).sum() / y.shape[0])
        if p_out > 0.0:
            c = float(np.sqrt(p_in / p_out))
    out = c * (y[q:q + n] if shift else y)
    return out, (c, g)


def reverb_ref(x, h=None, cols=None, noise=None, p_v=None, s=0, m=0, snr=0.0, shift=True, normalize=True):
    """float64: (out, (c, g)).  h None: no RIR; cols = (q, e0, e1); noise None: none, else float samples with their power p_v, start s, span m"""
    return _reverb(_conv64, x, h, cols, noise, p_v, s, m, snr, shift, normalize)


def reverb_fp32_yardstick(x, h=None, cols=None, noise=None, p_v=None, s=0, m=0, snr=0.0, shift=True, normalize=True):
    """the same with float32 FFT convolutions"""
    return _reverb(_conv32, x, h, cols, noise, p_v, s, m, snr, shift, normalize)


def figure(out, ref):
    """e = max |out - ref| / rms(ref); an all-zero reference asks for exact zeros (figure 0, else inf)"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    if ref.shape[0] == 0:
        return 0.0
    rms = float(np.sqrt((ref * ref).mean()))
    if rms == 0.0:
        return 0.0 if not out.any() else float("inf")
    return float(np.abs(out - ref).max() / rms)
