"""rsrgan_feat_stream and rsrgan_feat_denorm (csrc/feat.hip k_feat_stream / k_feat_denorm) through ctypes on caller-owned tensors against
the NumPy reference tests/feat_stream_ref.py, by EQUALITY of the raw bytes (the sign of zero counts).  No tolerance anywhere.

Front end: B = 4 rows, T = 8, the ring at StreamBank's minimum for chunk = 5 (H = left + 5 + right), six consecutive calls on one ring and
a seventh without fresh frames.  The rows rotate through four roles, so every call has a resting row (napp = nemit = 0), a row that
begins an utterance and appends without emitting, a row that emits from its utterance's first frame (emit0 = 0: the left clamp) and a
row that takes in its last frames and is flushed (the right clamp at `last`); by its flush an utterance has more than H frames, so the
ring wraps.  Every table is checked against the window invariant before it is used.  `out` is NaN before every call, `hist` is compared
after every call, and hist, out and fresh lie between guard bands that must come back untouched -- also after a call whose table is
hostile, which must return RSRGAN_OK (memory safety by construction: every index is clamped or a remainder)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from rsrgan_amd import _lib
from tests import feat_stream_ref as FR
from tests.feat_ref import seeded_stats

pytestmark = pytest.mark.gpu

BAND, GUARD = 64, 12345.0                      # floats around hist, out and fresh, and what they hold
CHUNK = 5


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Banded(object):
    """a device array of `n` elements between two guard bands"""

    def __init__(self, n, dtype=torch.float32, fill=None, band=BAND):
        self.buf = torch.full((band + n + band,), GUARD, dtype=dtype, device="cuda")
        self.mid = self.buf[band:band + n]
        self.band = band
        if fill is not None:
            self.mid.copy_(torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)))

    def intact(self):
        return bool((self.buf[:self.band] == GUARD).all()) and bool((self.buf[self.band + self.mid.numel():] == GUARD).all())


def _call(lib, fresh, table, hist, B, H, T, D, left, right, stats, out, lengths):
    rc = lib.rsrgan_feat_stream(_ptr(fresh), 0 if fresh is None else fresh.numel() // D, _ptr(table), _ptr(hist), B, H, T, D, left, right,
                                _ptr(stats[0]), _ptr(stats[1]), _ptr(out), _ptr(lengths), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.rsrgan_last_error().decode()
    torch.cuda.synchronize()


def _schedule(B, H, T, left, right, calls):
    """the tables of `calls` consecutive calls and the fresh rows each needs: row r has role (c - r) mod 4 in call c"""
    n, nxt = [0] * B, [0] * B
    tables = []
    for c in range(calls):
        table, src = np.zeros((B, 6), np.int32), 1                      # (fresh row 0 belongs to nobody)
        for r in range(B):
            role = (c - r) % 4
            if role == 1:                                               # a new utterance: two frames, none emitted yet
                n[r] = nxt[r] = 0
                a, k = 2, 0
            elif role == 2:                                             # emits from frame 0
                assert nxt[r] == 0
                a = 3 + right
                k = min(T, n[r] + a)
            elif role == 3:                                             # the last frames come in and everything left is emitted
                a = min(T, CHUNK + right) - (n[r] - nxt[r])
                k = n[r] + a - nxt[r]
            else:
                a = k = 0
            table[r] = (src, n[r], a, nxt[r], k, n[r] + a - 1)
            # the window invariant (include/rsrgan.h): a table the reference and the kernel must agree on
            assert a >= 0 and 0 <= k <= T and (a == 0 and k == 0 or (n[r] + a - 1) - (nxt[r] - left) + 1 <= H)
            src += a; n[r] += a; nxt[r] += k
        tables.append((table, src))
    return tables, n, nxt


def _run_front_end(lib, B, T, D, left, right, with_cmvn, calls=6):
    H = left + CHUNK + right
    rng = np.random.default_rng(1000 * D + 10 * left + right + (1 if with_cmvn else 0))
    stats_h = seeded_stats(rng, D) if with_cmvn else (None, None)
    stats_d = tuple(None if s is None else torch.from_numpy(s).cuda() for s in stats_h)
    Dout = D * (left + 1 + right)
    tables, n, nxt = _schedule(B, H, T, left, right, calls)
    ring_h = (rng.standard_normal((B, H, D)) * 3).astype(np.float32)     # (what the ring held before: slots never written must survive)
    ring_d = Banded(B * H * D, fill=ring_h)
    assert ring_d.mid.data_ptr() % 16 == 0
    seen = dict(rest=0, hold=0, first=0, flush=0, wrapped=False, clamped_right=False)
    # a seventh call without fresh frames: whoever still holds frames is flushed; its napp must count as 0
    last_table = np.array([(0, n[r], 3, nxt[r], n[r] - nxt[r], n[r] - 1) for r in range(B)], np.int32)
    assert (last_table[:, 4] > 0).any()
    for table, rows in tables + [(last_table, 0)]:
        fresh_h = (rng.standard_normal((rows, D)) * 2.0 + 0.5).astype(np.float32) if rows else None
        fresh_d = Banded(rows * D, fill=fresh_h) if rows else None
        out_d = Banded(B * T * Dout)
        out_d.mid.fill_(float("nan"))
        len_d = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        table_d = torch.from_numpy(table).cuda()
        _call(lib, None if fresh_d is None else fresh_d.mid, table_d, ring_d.mid, B, H, T, D, left, right, stats_d, out_d.mid, len_d)
        want, want_len = FR.feat_stream(fresh_h, table, ring_h, T, left, right, *stats_h)
        got = out_d.mid.cpu().numpy().reshape(B, T, Dout)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), int((got.view(np.int32) != want.view(np.int32)).sum())
        assert np.array_equal(len_d.cpu().numpy(), want_len)
        assert np.array_equal(ring_d.mid.cpu().numpy().view(np.int32), ring_h.reshape(-1).view(np.int32)), "the ring differs"
        assert ring_d.intact() and out_d.intact() and (fresh_d is None or fresh_d.intact()), "a guard band was written"
        assert torch.equal(table_d.cpu(), torch.from_numpy(table)) and (fresh_d is None or np.array_equal(fresh_d.mid.cpu().numpy(), fresh_h.reshape(-1)))
        if rows:
            for r in range(B):
                _, app0, napp, emit0, nemit, last = (int(v) for v in table[r])
                seen["rest"] += napp == 0 and nemit == 0
                seen["hold"] += napp > 0 and nemit == 0
                seen["first"] += nemit > 0 and emit0 == 0 and left > 0
                seen["flush"] += nemit > 0 and emit0 + nemit - 1 == last
                seen["wrapped"] |= napp > 0 and app0 + napp - 1 >= H
                seen["clamped_right"] |= nemit > 0 and emit0 + nemit - 1 + right > last
        # rows that rest or only append are written as +0.0
        for r in range(B):
            if table[r, 4] <= 0:
                assert not got[r].view(np.int32).any()
    return seen


@pytest.mark.parametrize("with_cmvn", [True, False], ids=["cmvn", "raw"])
@pytest.mark.parametrize("left,right", [(0, 0), (2, 3), (5, 5)])
@pytest.mark.parametrize("D", [3, 257])
def test_feat_stream_equals_the_reference_call_after_call(lib, D, left, right, with_cmvn):
    seen = _run_front_end(lib, 4, 8, D, left, right, with_cmvn)
    assert seen["rest"] >= 6 and seen["hold"] >= 6 and seen["flush"] >= 6 and seen["wrapped"], seen
    assert seen["first"] >= (6 if left else 0) and seen["clamped_right"] == (right > 0), seen


def test_feat_stream_scalar_tail(lib):
    """B * T * Dout = 3 * 5 * 18 = 270 is no multiple of 4: the last two elements leave one by one"""
    _run_front_end(lib, 3, 5, 3, 2, 3, True)


def test_feat_stream_second_grid_stride_pass(lib):
    """8 x 100 x 2827 elements are more than 2048 x 256 lanes of four: lanes take a second pass (one call, H = 128 holds the window)"""
    B, T, D, left, right, H = 8, 100, 257, 5, 5, 128
    assert B * T * D * 11 > 2048 * 256 * 4
    rng = np.random.default_rng(3)
    stats_h = seeded_stats(rng, D)
    stats_d = tuple(torch.from_numpy(s).cuda() for s in stats_h)
    fresh_h = (rng.standard_normal((B * T, D)) * 2.0 + 0.5).astype(np.float32)
    table = np.array([(r * T, 0, T, 0, T - (r % 3), T - 1) for r in range(B)], np.int32)
    ring_h = np.zeros((B, H, D), np.float32)
    ring_d, fresh_d, out_d = Banded(B * H * D, fill=ring_h), Banded(B * T * D, fill=fresh_h), Banded(B * T * D * 11)
    out_d.mid.fill_(float("nan"))
    len_d = torch.empty(B, dtype=torch.int32, device="cuda")
    _call(lib, fresh_d.mid, torch.from_numpy(table).cuda(), ring_d.mid, B, H, T, D, left, right, stats_d, out_d.mid, len_d)
    want, want_len = FR.feat_stream(fresh_h, table, ring_h, T, left, right, *stats_h)
    assert np.array_equal(out_d.mid.cpu().numpy().view(np.int32), want.reshape(-1).view(np.int32))
    assert np.array_equal(ring_d.mid.cpu().numpy().view(np.int32), ring_h.reshape(-1).view(np.int32))
    assert np.array_equal(len_d.cpu().numpy(), want_len) and ring_d.intact() and out_d.intact() and fresh_d.intact()


@pytest.mark.parametrize("with_cmvn", [True, False], ids=["cmvn", "raw"])
def test_feat_stream_is_memory_safe_whatever_the_table_holds(lib, with_cmvn):
    """negative counts, src beyond fresh_rows, frames and `last` far beyond H, an append longer than the ring: RSRGAN_OK, the lengths of
    the formula, and nothing outside hist, out and fresh is touched.  (The VALUES of such a call are not the utterance's and are not
    compared: a slot may be read while it is rewritten.)"""
    B, T, D, left, right = 4, 8, 257, 2, 3
    H, rows = left + CHUNK + right, 6
    big = 2 ** 31 - 1
    table = np.array([(10 ** 6, -7, 3, -5, 4, big),
                      (-50, big - 10, -4, big - 20, -3, -9),
                      (0, 5, 100, 3, big, 10 ** 9),
                      (rows + 5, -big, 2, -big, 9, 7)], np.int32)
    rng = np.random.default_rng(4)
    stats_d = tuple(torch.from_numpy(s).cuda() for s in seeded_stats(rng, D)) if with_cmvn else (None, None)
    ring_d = Banded(B * H * D, fill=np.zeros((B, H, D), np.float32))
    fresh_d = Banded(rows * D, fill=rng.standard_normal((rows, D)).astype(np.float32))
    out_d = Banded(B * T * D * (left + 1 + right))
    out_d.mid.fill_(float("nan"))
    len_d = torch.empty(B, dtype=torch.int32, device="cuda")
    _call(lib, fresh_d.mid, torch.from_numpy(table).cuda(), ring_d.mid, B, H, T, D, left, right, stats_d, out_d.mid, len_d)
    assert ring_d.intact() and out_d.intact() and fresh_d.intact(), "a guard band was written"
    assert len_d.cpu().tolist() == [4, 0, 8, 8]
    got = out_d.mid.cpu().numpy().reshape(B, T, -1)
    assert not np.isnan(got).any(), "every element of out is written"
    assert not got[1].view(np.int32).any() and not got[0, 4:].view(np.int32).any()      # nemit < 0 / t >= nemit: +0.0


# ---- rsrgan_feat_denorm ---------------------------------------------------------------------------------------------------------

def _denorm_inputs(B, T, D):
    rng = np.random.default_rng(7)
    y = rng.standard_normal((B, T, D)).astype(np.float32)
    return y, rng.uniform(0.5, 2.0, D), rng.standard_normal(D)


@pytest.mark.parametrize("shift", [0, 1], ids=["out16", "out8"])
@pytest.mark.parametrize("lengths", [[7, 0, 3, 7], None], ids=["lengths", "null"])
@pytest.mark.parametrize("B,T,D", [(4, 7, 3), (4, 7, 40), (3, 7, 3)])
def test_feat_denorm_equals_numpy(lib, B, T, D, lengths, shift):
    """(3, 7, 3): 63 elements, so the last three leave through the scalar tail.  shift: `out` 8-byte but not 16-byte aligned."""
    y, stddev, mean = _denorm_inputs(B, T, D)
    ln = None if lengths is None else np.asarray(lengths[:B], np.int32)
    want = FR.feat_denorm(y, ln, mean, stddev)
    # the case is a real check of contract(off): rounding y * s + m ONCE (exactly, with rationals) gives other bits somewhere
    once = np.array([[float(Fraction(float(v)) * Fraction(float(s)) + Fraction(float(m))) for v, s, m in zip(row, stddev, mean)] for row in y[0]])
    assert np.array_equal(want[0], y[0] * stddev + mean)
    differ = int((once.view(np.int64) != want[0].view(np.int64)).sum())
    print("singly rounded differs in", differ, "of", once.size)
    assert differ >= 1
    out_d = Banded(B * T * D + shift, dtype=torch.float64, band=BAND)
    out = out_d.mid[shift:]
    assert out.data_ptr() % 16 == 8 * shift
    out_d.mid.fill_(float("nan"))
    y_d, ln_d = torch.from_numpy(y).cuda(), None if ln is None else torch.from_numpy(ln).cuda()
    mean_d, stddev_d = torch.from_numpy(mean).cuda(), torch.from_numpy(stddev).cuda()
    rc = lib.rsrgan_feat_denorm(_ptr(y_d), _ptr(ln_d), B, T, D, _ptr(mean_d), _ptr(stddev_d), _ptr(out),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.rsrgan_last_error().decode()
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(B, T, D)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), int((got.view(np.int64) != want.view(np.int64)).sum())
    assert out_d.intact() and (shift == 0 or bool(torch.isnan(out_d.mid[:shift]).all()))
    assert torch.equal(y_d.cpu(), torch.from_numpy(y))
