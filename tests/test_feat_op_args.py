"""rsrgan_feat_batch (csrc/feat.hip) refuses every argument error before its first HIP call, as the operator entries of
tests/test_op_args.py do, naming the argument in rsrgan_last_error().  The pointers are made-up addresses: a refused call never reads
them, and no device is needed."""
import pytest

from rsrgan_amd import _lib
from tests.test_op_args import P, refused


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def feat(lib, **kw):
    a = dict(raw=P, raw_rows=100, offsets=P + 4096, B=4, T=9, D=7, left=2, right=3, mean=P + 8192, stddev=P + 12288, out=P + 16384,
             lengths=P + 20480)
    a.update(kw)
    return lib.rsrgan_feat_batch(a["raw"], a["raw_rows"], a["offsets"], a["B"], a["T"], a["D"], a["left"], a["right"], a["mean"], a["stddev"],
                                 a["out"], a["lengths"], None)


def test_symbol_is_bound(lib):
    assert "rsrgan_feat_batch" in _lib.SYMBOLS and hasattr(lib, "rsrgan_feat_batch")
    assert len(lib.rsrgan_feat_batch.argtypes) == 13


@pytest.mark.parametrize("which", ["raw", "offsets", "out"])
def test_null_required_pointer(lib, which):
    refused(lib, feat(lib, **{which: None}), "feat_batch", "null pointer")


@pytest.mark.parametrize("which", ["mean", "stddev"])
def test_only_one_of_mean_and_stddev(lib, which):
    refused(lib, feat(lib, **{which: None}), "feat_batch", "mean and stddev must both be given or both be null")


def test_alignment(lib):
    for which in ("raw", "out"):
        for off in (4, 8):
            refused(lib, feat(lib, **{which: P + off}), "feat_batch", "raw or out not 16-byte aligned")
    for which in ("offsets", "lengths"):
        refused(lib, feat(lib, **{which: P + 4096 + 2}), "feat_batch", "offsets or lengths not 4-byte aligned")
    for which in ("mean", "stddev"):
        refused(lib, feat(lib, **{which: P + 8192 + 4}), "feat_batch", "mean or stddev not 8-byte aligned")


@pytest.mark.parametrize("which", ["B", "T", "D", "raw_rows"])
def test_sizes_below_one(lib, which):
    for v in (0, -1):
        refused(lib, feat(lib, **{which: v}), "feat_batch", "must be positive")


def test_negative_context(lib):
    refused(lib, feat(lib, left=-1), "feat_batch", "negative context (left -1, right 3)")
    refused(lib, feat(lib, right=-2), "feat_batch", "negative context (left 2, right -2)")


def test_limits(lib):
    """the limits include/rsrgan.h states: a context of at most 1024 frames on either side, at most 2^32 - 1 output elements,
    at most 2^40 raw floats"""
    refused(lib, feat(lib, left=1025), "feat_batch", "context above the entry's 1024")
    refused(lib, feat(lib, right=1025), "feat_batch", "context above the entry's 1024")
    # 2^16 x 2^16 x 1 x 1 = 2^32: one element too many; so is every way of reaching it
    refused(lib, feat(lib, B=1 << 16, T=1 << 16, D=1, left=0, right=0), "feat_batch", "above the entry's 2^32 - 1 elements")
    refused(lib, feat(lib, B=1 << 15, T=1 << 15, D=4, left=0, right=0), "above the entry's 2^32 - 1 elements")
    refused(lib, feat(lib, B=1 << 15, T=1 << 15, D=1, left=1, right=2), "above the entry's 2^32 - 1 elements")
    refused(lib, feat(lib, B=(1 << 31) - 1, T=(1 << 31) - 1, D=(1 << 31) - 1, left=1024, right=1024), "above the entry's 2^32 - 1 elements")
    refused(lib, feat(lib, raw_rows=(1 << 40) // 7 + 1), "feat_batch", "raw_rows x D", "above the entry's 2^40")
