"""NumPy reference of rsrgan_feat_stream and rsrgan_feat_denorm (include/rsrgan.h, csrc/feat.hip k_feat_stream / k_feat_denorm): the two
formulas of the header spelled out element by element -- the ring, its slots and `mod` included, not only the final splice.  TEST ONLY.

feat_stream works on the ring in place, as the kernel does.  Its append runs i upwards, so where napp > H the last write to a slot stands
(what the header states); its emit then reads the ring as it stands after the append."""
import numpy as np


def mod(j, H):
    """the non-negative remainder"""
    return int(j) - (int(j) // int(H)) * int(H)              # (Python's floor division: the remainder has H's sign)


def feat_stream(fresh, table, hist, T, left, right, mean=None, stddev=None):
    """fresh [rows, D] float32 or None, table [B, 6] = (src, app0, napp, emit0, nemit, last), hist [B, H, D] float32 (UPDATED IN PLACE).
    Returns (out [B, T, D * (left + 1 + right)] float32, lengths [B] int32)."""
    B, H, D = hist.shape
    C = left + 1 + right
    rows = 0 if fresh is None else fresh.shape[0]
    out = np.empty((B, T, D * C), np.float32)
    lengths = np.empty(B, np.int32)
    for r in range(B):
        src, app0, napp, emit0, nemit, last = (int(v) for v in table[r])
        for i in range(max(napp, 0) if rows > 0 else 0):
            row = min(max(src + i, 0), rows - 1)
            slot = mod(app0 + i, H)
            if mean is None:
                hist[r, slot] = fresh[row]
            else:
                hist[r, slot] = ((fresh[row].astype(np.float64) - mean) / stddev).astype(np.float32)
    for r in range(B):
        src, app0, napp, emit0, nemit, last = (int(v) for v in table[r])
        lengths[r] = min(max(nemit, 0), T)
        for t in range(T):
            if t >= min(nemit, T) or last < 0:
                out[r, t] = 0.0                                   # +0.0
                continue
            for c in range(C):
                j = min(max(emit0 + t + c - left, 0), last)
                out[r, t, c * D:(c + 1) * D] = hist[r, mod(j, H)]
    return out, lengths


def feat_denorm(y, lengths, mean, stddev):
    """y [B, T, D] float32 -> float64: NumPy's `y * stddev + mean` (two roundings) on the rows below each length, +0.0 from there on"""
    y = np.asarray(y)
    assert y.dtype == np.float32 and mean.dtype == np.float64 and stddev.dtype == np.float64
    B, T, D = y.shape
    out = np.zeros((B, T, D), np.float64)
    for b in range(B):
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        out[b, :n] = y[b, :n] * stddev + mean
    return out
