"""Reference of the device histogram (csrc/hist.hip, include/rsrgan.h rsrgan_hist): the bucket search of rsrgan_amd/summary.py
histogram() (np.searchsorted(side="right"), clamped to the last bucket) and math.fsum -- the correctly rounded sum -- for sum and
sum_squares.  Shared by tests/test_gpu_hist_ops.py and tests/test_gpu_summary_device.py."""
import math

import numpy as np

from rsrgan_amd import summary as S

NL = len(S._LIMITS)
EPS = 2.0 ** -52


def _fsum(v):
    """math.fsum, with NumPy's answer where fsum has none: a NaN term, or infinities of both signs, give NaN; one sign gives it"""
    v = np.asarray(v, np.float64)
    if np.isnan(v).any() or (np.isposinf(v).any() and np.isneginf(v).any()):
        return float("nan")
    if np.isinf(v).any():
        return float("inf") if np.isposinf(v).any() else float("-inf")
    return math.fsum(v.tolist())


def record(values):
    """[min, max, num, sum, sum_squares, counts...] of a tensor's float32 values, and the bound on |sum - fsum| and |sum_squares - fsum|:
    n * 2^-52 * sum |term|, the worst case of ANY order of n fp64 additions (n - 1 roundings of at most 2^-53 relative to a partial sum
    that never exceeds sum |term| * (1 + tiny)) with a factor 2 of slack.  The squares of float32 values are exact in float64, so only
    the order of the additions contributes."""
    x = np.asarray(values, np.float32).astype(np.float64).ravel()
    if x.size == 0:
        x = np.zeros(1)
    idx = np.minimum(np.searchsorted(S._LIMITS, x, side="right"), NL - 1)
    counts = np.bincount(idx, minlength=NL).astype(np.float64)
    sq = x * x
    with np.errstate(invalid="ignore"):
        rec = np.concatenate([[x.min(), x.max(), float(x.size), _fsum(x), _fsum(sq)], counts])
    n = x.size
    finite = np.isfinite(x).all()
    bounds = (n * EPS * math.fsum(np.abs(x).tolist()), n * EPS * math.fsum(sq.tolist())) if finite else (0.0, 0.0)
    return rec, bounds


def same(a, b):
    """equal as numbers, NaN equal to NaN (+0.0 and -0.0 are the same minimum)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check(got, values, scale=1.0):
    """a device record against the reference of `values`: min, max, num and every count exactly, the two sums within scale x the bound
    (non-finite sums: the same infinity, or NaN for NaN)"""
    got = np.asarray(got, np.float64).ravel()
    want, (b_sum, b_sq) = record(values)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert same(got[:3], want[:3]), (got[:5], want[:5])
    bad = np.nonzero(got[5:] != want[5:])[0]
    assert bad.size == 0, [(int(i), S._LIMITS[i], got[5 + i], want[5 + i]) for i in bad[:8]]
    for k, bound in ((3, b_sum), (4, b_sq)):
        if np.isfinite(want[k]):
            print("hist field %d: |got - fsum| = %.3e, bound %.3e" % (k, abs(got[k] - want[k]), scale * bound))
            assert abs(got[k] - want[k]) <= scale * bound, (k, got[k], want[k], bound)
        else:
            assert same(got[k], want[k]), (k, got[k], want[k])
