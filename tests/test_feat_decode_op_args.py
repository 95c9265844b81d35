"""rsrgan_feat_decode (csrc/feat.hip k_feat_decode) refuses every argument error before its first HIP call, as rsrgan_feat_batch does
(tests/test_feat_op_args.py), naming the argument in rsrgan_last_error().  The pointers are made-up addresses: a refused call never
reads them, and no device is needed."""
import pytest

from rsrgan_amd import _lib
from tests.test_op_args import P, refused


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def dec(lib, **kw):
    a = dict(blob=P, blob_bytes=4096, seg=P + 4096, scale=P + 8192, offsets=P + 12288, B=4, D=7, mean=P + 16384, stddev=P + 20480,
             out=P + 24576, out_rows=100)
    a.update(kw)
    return lib.rsrgan_feat_decode(a["blob"], a["blob_bytes"], a["seg"], a["scale"], a["offsets"], a["B"], a["D"], a["mean"], a["stddev"],
                                  a["out"], a["out_rows"], None)


def test_symbol_is_bound(lib):
    assert "rsrgan_feat_decode" in _lib.SYMBOLS and hasattr(lib, "rsrgan_feat_decode")
    assert len(lib.rsrgan_feat_decode.argtypes) == 12


@pytest.mark.parametrize("which", ["blob", "seg", "offsets", "out"])
def test_null_required_pointer(lib, which):
    refused(lib, dec(lib, **{which: None}), "feat_decode", "null pointer")


def test_scale_is_always_required(lib):
    refused(lib, dec(lib, scale=None), "feat_decode", "null pointer (scale)")
    refused(lib, dec(lib, scale=None, mean=None, stddev=None), "feat_decode", "null pointer (scale)")


@pytest.mark.parametrize("which", ["mean", "stddev"])
def test_only_one_of_mean_and_stddev(lib, which):
    refused(lib, dec(lib, **{which: None}), "feat_decode", "mean and stddev must both be given or both be null")


def test_alignment(lib):
    for which in ("blob", "out"):
        for off in (1, 4, 8):
            refused(lib, dec(lib, **{which: P + off}), "feat_decode", "blob or out not 16-byte aligned")
    for which in ("seg", "mean", "stddev"):
        for off in (2, 4):
            refused(lib, dec(lib, **{which: P + 4096 + off}), "feat_decode", "seg, mean or stddev not 8-byte aligned")
    for which in ("scale", "offsets"):
        for off in (1, 2):
            refused(lib, dec(lib, **{which: P + 8192 + off}), "feat_decode", "scale or offsets not 4-byte aligned")


@pytest.mark.parametrize("which", ["B", "D", "blob_bytes", "out_rows"])
def test_sizes_below_one(lib, which):
    for v in (0, -1):
        refused(lib, dec(lib, **{which: v}), "feat_decode", "must be positive")


def test_limit(lib):
    """the limit include/rsrgan.h states: at most 2^40 output floats"""
    refused(lib, dec(lib, out_rows=(1 << 40) // 7 + 1), "feat_decode", "out_rows x D", "above the entry's 2^40")
    refused(lib, dec(lib, out_rows=(1 << 40) + 1, D=1), "feat_decode", "above the entry's 2^40")
    refused(lib, dec(lib, out_rows=(1 << 62), D=(1 << 31) - 1), "feat_decode", "above the entry's 2^40")
