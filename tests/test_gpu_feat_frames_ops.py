"""rsrgan_feat_frames (csrc/feat.hip k_feat_frames) on caller-owned tensors against the host expansion -- io.features.apply_cmvn and
splice_feats on the utterance a pick names (tests/feat_frames_ref.expand_picks) -- by EQUALITY of the bits (torch.equal on the int32
view).  No tolerance anywhere.

The pool holds utterances of [9, 1, 2, 6] frames behind 3 lead rows, so none starts at row 0.  The picks: every frame of every
utterance, so both clamps at an utterance's first and last frame are taken and utterances are shorter than either context; repeated and
out-of-order rows; one pick with hi <= lo, whose output row must be +0.0; an N whose N * Dout is no multiple of 4 (the scalar tail)
wherever Dout admits one (Dout = 40 admits none); at D = 257 with context 5 / 5, N = 800: more than 2048 x 256 x 4 elements, so lanes take
a second grid-stride pass.  `out` sits between NaN bands that must come back untouched; pool and picks must be unchanged; two launches
must give the same bits.  pool_rows below what the table asks for is compared against the clamped formula."""
import ctypes as C

import numpy as np
import pytest
import torch

from rsrgan_amd import _lib
from tests import feat_frames_ref as R
from tests.feat_ref import seeded_stats

pytestmark = pytest.mark.gpu

CONFIGS = [(257, 5, 5), (5, 2, 3), (40, 0, 0), (7, 0, 4)]
LENGTHS, LEAD = [9, 1, 2, 6], 3
BAND = 64                                     # floats in front of and behind `out` (a multiple of 4: out stays 16-byte aligned)


def make_pool(rng, D):
    rows = LEAD + sum(LENGTHS)
    pool = (rng.standard_normal((rows, D)) * 2.0 + 0.5).astype(np.float32)
    bounds, lo = [], LEAD
    for n in LENGTHS:
        bounds.append((lo, lo + n)); lo += n
    return pool, bounds


def make_picks(rng, bounds, N, zero_at):
    """every frame of every utterance in a shuffled order, then random repeats up to N; pick `zero_at` names an empty utterance"""
    every = [(r, lo, hi) for lo, hi in bounds for r in range(lo, hi)]
    assert N > len(every)
    order = rng.permutation(len(every))
    picks = [every[i] for i in order] + [every[int(i)] for i in rng.integers(0, len(every), N - len(every))]
    picks[zero_at] = (bounds[0][0] + 2, bounds[0][0] + 4, bounds[0][0] + 4 - (zero_at % 2))          # hi == lo or hi < lo
    return np.asarray(picks, np.int32)


def launch(lib, pool, pool_rows, picks, N, D, left, right, mean, stddev, out):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = lib.rsrgan_feat_frames(p(pool), pool_rows, p(picks), N, D, left, right, p(mean), p(stddev), p(out),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.rsrgan_last_error().decode()


def run_case(lib, pool_h, picks_h, stats, left, right, pool_rows=None):
    """two launches into banded buffers; returns out [N, Dout] of the first after every invariant held"""
    dev = torch.device("cuda", 0)
    N, D = picks_h.shape[0], pool_h.shape[1]
    total = N * D * (left + 1 + right)
    pool, picks = torch.from_numpy(pool_h).to(dev), torch.from_numpy(picks_h).to(dev)
    pool0, picks0 = pool.clone(), picks.clone()
    mean, stddev = (None, None) if stats is None else (torch.from_numpy(stats[0]).to(dev), torch.from_numpy(stats[1]).to(dev))
    assert mean is None or (mean.dtype == torch.float64 and stddev.dtype == torch.float64)
    outs = []
    for _ in range(2):
        buf = torch.full((BAND + total + BAND,), float("nan"), dtype=torch.float32, device=dev)
        nan_bits = buf[:1].view(torch.int32).item()
        out = buf[BAND:BAND + total]
        assert out.data_ptr() % 16 == 0 and pool.data_ptr() % 16 == 0
        launch(lib, pool, pool_h.shape[0] if pool_rows is None else pool_rows, picks, N, D, left, right, mean, stddev, out)
        torch.cuda.synchronize()
        bits = buf.view(torch.int32)
        assert bool((bits[:BAND] == nan_bits).all()) and bool((bits[BAND + total:] == nan_bits).all()), "a band around out was written"
        outs.append(out.clone())
    assert torch.equal(pool.view(torch.int32), pool0.view(torch.int32)) and torch.equal(picks, picks0), "an input was written"
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two launches differ"
    return outs[0].reshape(N, -1)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _equal(got, want):
    w = torch.from_numpy(np.ascontiguousarray(want, np.float32)).to(got.device)
    return torch.equal(got.view(torch.int32), w.view(torch.int32))


@pytest.mark.parametrize("with_cmvn", [True, False], ids=["cmvn", "raw"])
@pytest.mark.parametrize("D,left,right", CONFIGS)
def test_feat_frames_equals_the_host_expansion(lib, D, left, right, with_cmvn):
    rng = np.random.default_rng(2000 * D + 10 * left + right + (1 if with_cmvn else 0))
    stats = seeded_stats(rng, D) if with_cmvn else None
    pool, bounds = make_pool(rng, D)
    assert bounds[0][0] == LEAD > 0 and max(LENGTHS) > left and min(LENGTHS) <= min(left, right) + 1
    Dout = D * (left + 1 + right)
    sizes = [24]                                                 # 18 frames + repeats; one workgroup at the small shapes
    tail = next((n for n in (23, 25, 26, 27) if (n * Dout) % 4), None)
    assert (tail is None) == (Dout % 4 == 0)
    if tail is not None:
        sizes.append(tail)
    if D == 257:
        sizes.append(800)
        assert 800 * Dout > 2048 * 256 * 4                       # a second grid-stride pass
    for N in sizes:
        Z = N - 3                                                # (among the repeats: every frame stays covered)
        picks = make_picks(rng, bounds, N, zero_at=Z)
        covered = {(int(r), int(lo)) for r, lo, hi in picks if hi > lo}
        assert len(covered) == sum(LENGTHS) and len(picks) > len(covered)            # every frame, and repeats
        assert np.any(np.diff(picks[:, 0]) < 0)                                       # out of order
        want = R.expand_picks(pool, picks, left, right, stats)
        assert np.array_equal(want.view(np.int32), R.gather(pool, picks, left, right, stats).view(np.int32))      # the two references agree
        got = run_case(lib, pool, picks, stats, left, right)
        assert _equal(got, want), (N, int((got.cpu().view(torch.int32) != torch.from_numpy(want).view(torch.int32)).sum()))
        assert not bool(got[Z].view(torch.int32).any()), "the row of a pick with hi <= lo is +0.0"
        assert bool(got[Z - 1].view(torch.int32).any())


@pytest.mark.parametrize("with_cmvn", [True, False], ids=["cmvn", "raw"])
def test_source_rows_are_clamped_into_the_pool(lib, with_cmvn):
    """pool_rows below what the table asks for (the tensor itself is larger, so nothing here depends on the clamp for its safety): rows past
    pool_rows - 1 read row pool_rows - 1"""
    rng = np.random.default_rng(9)
    D, left, right = 5, 2, 3
    stats = seeded_stats(rng, D) if with_cmvn else None
    pool, bounds = make_pool(rng, D)
    picks = make_picks(rng, bounds, 27, zero_at=5)
    pool_rows = 14                                               # the third utterance ends at row 15, the fourth lies wholly beyond
    assert bounds[2][1] == 15 and bounds[3][0] >= pool_rows
    want = R.gather(pool, picks, left, right, stats, pool_rows=pool_rows)
    assert not np.array_equal(want, R.gather(pool, picks, left, right, stats))
    got = run_case(lib, pool, picks, stats, left, right, pool_rows=pool_rows)
    assert _equal(got, want)
