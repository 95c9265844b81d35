"""rsrgan_feat_frames (csrc/feat.hip) refuses every argument error before its first HIP call, as rsrgan_feat_batch does
(tests/test_feat_op_args.py), naming the argument in rsrgan_last_error().  The pointers are made-up addresses: a refused call never reads
them, and no device is needed."""
import pytest

from rsrgan_amd import _lib
from tests.test_op_args import P, refused


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def frames(lib, **kw):
    a = dict(pool=P, pool_rows=100, picks=P + 4096, N=8, D=7, left=2, right=3, mean=P + 8192, stddev=P + 12288, out=P + 16384)
    a.update(kw)
    return lib.rsrgan_feat_frames(a["pool"], a["pool_rows"], a["picks"], a["N"], a["D"], a["left"], a["right"], a["mean"], a["stddev"], a["out"],
                                  None)


def test_symbol_is_bound(lib):
    assert "rsrgan_feat_frames" in _lib.SYMBOLS and hasattr(lib, "rsrgan_feat_frames")
    assert len(lib.rsrgan_feat_frames.argtypes) == 11


@pytest.mark.parametrize("which", ["pool", "picks", "out"])
def test_null_required_pointer(lib, which):
    refused(lib, frames(lib, **{which: None}), "feat_frames", "null pointer")


@pytest.mark.parametrize("which", ["mean", "stddev"])
def test_only_one_of_mean_and_stddev(lib, which):
    refused(lib, frames(lib, **{which: None}), "feat_frames", "mean and stddev must both be given or both be null")


def test_alignment(lib):
    for which in ("pool", "out"):
        for off in (4, 8):
            refused(lib, frames(lib, **{which: P + off}), "feat_frames", "pool or out not 16-byte aligned")
    refused(lib, frames(lib, picks=P + 4096 + 2), "feat_frames", "picks not 4-byte aligned")
    for which in ("mean", "stddev"):
        refused(lib, frames(lib, **{which: P + 8192 + 4}), "feat_frames", "mean or stddev not 8-byte aligned")


@pytest.mark.parametrize("which", ["N", "D", "pool_rows"])
def test_sizes_below_one(lib, which):
    for v in (0, -1):
        refused(lib, frames(lib, **{which: v}), "feat_frames", "must be positive")


def test_negative_context(lib):
    refused(lib, frames(lib, left=-1), "feat_frames", "negative context (left -1, right 3)")
    refused(lib, frames(lib, right=-2), "feat_frames", "negative context (left 2, right -2)")


def test_limits(lib):
    """the limits include/rsrgan.h states: a context of at most 1024 frames on either side, at most 2^32 - 1 output elements, at most
    2^40 pool floats"""
    refused(lib, frames(lib, left=1025), "feat_frames", "context above the entry's 1024")
    refused(lib, frames(lib, right=1025), "feat_frames", "context above the entry's 1024")
    # 2^16 x 2^16 x 1 = 2^32: one element too many; so is every way of reaching it
    refused(lib, frames(lib, N=1 << 16, D=1 << 16, left=0, right=0), "feat_frames", "above the entry's 2^32 - 1 elements")
    refused(lib, frames(lib, N=1 << 30, D=1, left=1, right=2), "above the entry's 2^32 - 1 elements")
    refused(lib, frames(lib, N=(1 << 31) - 1, D=(1 << 31) - 1, left=1024, right=1024), "above the entry's 2^32 - 1 elements")
    refused(lib, frames(lib, pool_rows=(1 << 40) // 7 + 1), "feat_frames", "pool_rows x D", "above the entry's 2^40")


def test_statistics_may_both_be_null_only_together(lib):
    """both NULL is the product path's form (the pool already normalised): with every other argument in order such a call is NOT refused
    for its statistics -- shown here by the next refusal in line naming something else"""
    refused(lib, frames(lib, mean=None, stddev=None, N=0), "feat_frames", "must be positive")
