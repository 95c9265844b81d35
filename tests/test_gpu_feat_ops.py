"""rsrgan_feat_batch (csrc/feat.hip) against the host expansion of tests/feat_ref.py -- io.features.apply_cmvn and splice_feats, the
functions the default reader runs -- by EQUALITY of the bits (torch.equal on the int32 view): the kernel computes (x - mean) / stddev in
IEEE double and rounds once, as the host does.  No tolerance anywhere.

Batches of every (D, left, right): utterances shorter than either context at T = longest; the same at a larger T (zero rows past the
longest utterance); the same at a smaller T (truncation: the context is clamped at the utterance's own last frame, lengths = min(n, T));
a batch with an empty utterance (an all-zero row); an offset table that does not start at 0; a batch whose B * T * Dout is no multiple
of 4 (the scalar tail; Dout = 40 admits none: every product is a multiple of 4); and, at D = 257 with context 5 / 5, a batch of more
than 2048 x 256 x 4 elements, so that lanes take a second grid-stride pass.  The smallest batch is one workgroup, the largest of the
common ones 100.  `out` and `lengths` sit between NaN / marker bands that must come back untouched; raw and offsets must be unchanged;
two launches must give the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from rsrgan_amd import _lib
from tests import feat_ref

pytestmark = pytest.mark.gpu

CONFIGS = [(257, 5, 5), (5, 2, 3), (40, 0, 0), (7, 0, 4)]
BAND = 64                                     # floats in front of and behind `out` (a multiple of 4: out stays 16-byte aligned)
MARK = -123456789


def batches(D, left, right):
    """(name, lengths, T, lead rows in front of the first utterance)"""
    out = [("short", [9, 1, 2, 6], 9, 0), ("padded", [9, 1, 2, 6], 12, 0), ("truncated", [9, 1, 2, 6], 4, 0),
           ("empty-row", [3, 0, 5, 2], 5, 0), ("offset0", [4, 7, 1], 7, 3)]
    if (3 * 5 * D * (left + 1 + right)) % 4:
        out.append(("tail", [3, 2, 5], 5, 0))
    if D == 257:
        out.append(("two-passes", [100, 57, 83, 100, 1, 64, 99, 31], 100, 0))
    return out


def launch(lib, raw, raw_rows, off, B, T, D, left, right, mean, stddev, out, lengths):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = lib.rsrgan_feat_batch(p(raw), raw_rows, p(off), B, T, D, left, right, p(mean), p(stddev), p(out), p(lengths),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.rsrgan_last_error().decode()


def run_case(lib, packed, stats, left, right, T, raw_rows=None, with_lengths=True):
    """two launches into banded buffers; returns (out [B, T, Dout], lengths [B]) of the first after every invariant held"""
    dev = torch.device("cuda", 0)
    B, D = packed.shape[0], packed.data.shape[1]
    total = B * T * D * (left + 1 + right)
    raw, off = torch.from_numpy(packed.data).to(dev), torch.from_numpy(packed.offsets).to(dev)
    raw0, off0 = raw.clone(), off.clone()
    mean, stddev = (None, None) if stats is None else (torch.from_numpy(stats[0]).to(dev), torch.from_numpy(stats[1]).to(dev))
    assert mean is None or (mean.dtype == torch.float64 and stddev.dtype == torch.float64)
    outs = []
    for _ in range(2):
        buf = torch.full((BAND + total + BAND,), float("nan"), dtype=torch.float32, device=dev)
        lbuf = torch.full((4 + B + 4,), MARK, dtype=torch.int32, device=dev)
        nan_bits = buf[:1].view(torch.int32).item()
        out, ln = buf[BAND:BAND + total], lbuf[4:4 + B]
        assert out.data_ptr() % 16 == 0
        launch(lib, raw, packed.data.shape[0] if raw_rows is None else raw_rows, off, B, T, D, left, right, mean, stddev, out,
               ln if with_lengths else None)
        torch.cuda.synchronize()
        bits = buf.view(torch.int32)
        assert bool((bits[:BAND] == nan_bits).all()) and bool((bits[BAND + total:] == nan_bits).all()), "a band around out was written"
        assert bool((lbuf[:4] == MARK).all()) and bool((lbuf[4 + B:] == MARK).all()), "a band around lengths was written"
        if not with_lengths:
            assert bool((ln == MARK).all())
        outs.append((out.clone(), ln.clone()))
    assert torch.equal(raw.view(torch.int32), raw0.view(torch.int32)) and torch.equal(off, off0), "an input was written"
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1], outs[1][1])
    return outs[0][0].reshape(B, T, -1), outs[0][1]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("with_cmvn", [True, False], ids=["cmvn", "raw"])
@pytest.mark.parametrize("D,left,right", CONFIGS)
def test_feat_batch_equals_the_host_expansion(lib, D, left, right, with_cmvn):
    rng = np.random.default_rng(1000 * D + 10 * left + right + (1 if with_cmvn else 0))
    stats = feat_ref.seeded_stats(rng, D) if with_cmvn else None
    names = []
    for name, lengths, T, lead in batches(D, left, right):
        packed = feat_ref.random_packed(rng, lengths, D, left, right, T, lead, stats)
        want, want_len = feat_ref.expand(packed, stats, left, right, T)
        got, got_len = run_case(lib, packed, stats, left, right, T)
        total = want.size
        if name == "tail":
            assert total % 4 != 0
        if name == "two-passes":
            assert total > 2048 * 256 * 4
        if name == "offset0":
            assert packed.offsets[0] != 0
        w = torch.from_numpy(want).to(got.device)
        assert torch.equal(got.view(torch.int32), w.view(torch.int32)), (name, int((got.view(torch.int32) != w.view(torch.int32)).sum()))
        assert got_len.cpu().tolist() == want_len.tolist() == [min(n, T) for n in lengths], name
        if name == "empty-row":
            assert not bool(got[1].view(torch.int32).any())                    # +0.0 everywhere
        if name == "padded":
            assert not bool(got[:, 9:].view(torch.int32).any())
        names.append(name)
    assert len(names) >= 5


def test_lengths_may_be_null_and_source_rows_are_clamped_into_raw(lib):
    """lengths = NULL: nothing but `out` is written.  raw_rows below what the offset table asks for (the tensor itself is larger, so
    nothing here depends on the clamp for its safety): rows past raw_rows - 1 read row raw_rows - 1."""
    rng = np.random.default_rng(8)
    D, left, right, T = 5, 2, 3, 6
    packed = feat_ref.random_packed(rng, [6, 4, 5], D, left, right, T)
    want, _ = feat_ref.expand(packed, None, left, right, T)
    got, _ = run_case(lib, packed, None, left, right, T, with_lengths=False)
    assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32))
    raw_rows = 8
    assert packed.offsets.tolist() == [0, 6, 10, 15] and packed.data.shape[0] == 15
    got, got_len = run_case(lib, packed, None, left, right, T, raw_rows=raw_rows)
    want = np.zeros_like(want)
    for b in range(3):
        o, n = int(packed.offsets[b]), int(packed.offsets[b + 1] - packed.offsets[b])
        for t in range(min(n, T)):
            for c in range(left + 1 + right):
                row = min(max(o + min(max(t + c - left, 0), n - 1), 0), raw_rows - 1)
                want[b, t, c * D:(c + 1) * D] = packed.data[row]
    assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32))
    assert got_len.cpu().tolist() == [6, 4, 5]
