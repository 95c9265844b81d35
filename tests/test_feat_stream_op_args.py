"""rsrgan_feat_stream and rsrgan_feat_denorm (csrc/feat.hip) refuse every argument error before their first HIP call, as rsrgan_feat_batch
and rsrgan_feat_frames do, naming the argument in rsrgan_last_error().  The pointers are made-up addresses: a refused call never reads
them, and no device is needed.  The header, the binding and the cross-compiled library agree on the two symbols."""
import os
import re

import pytest

from rsrgan_amd import _lib
from tests.test_op_args import P, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rsrgan_feat_stream", "rsrgan_feat_denorm"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def stream(lib, **kw):
    a = dict(fresh=P, fresh_rows=40, table=P + 4096, hist=P + 8192, B=4, H=15, T=8, D=7, left=2, right=3, mean=P + 12288, stddev=P + 16384,
             out=P + 20480, lengths=P + 24576)
    a.update(kw)
    return lib.rsrgan_feat_stream(a["fresh"], a["fresh_rows"], a["table"], a["hist"], a["B"], a["H"], a["T"], a["D"], a["left"], a["right"],
                                  a["mean"], a["stddev"], a["out"], a["lengths"], None)


def denorm(lib, **kw):
    a = dict(y=P, lengths=P + 4096, B=4, T=7, D=5, mean=P + 8192, stddev=P + 12288, out=P + 16384)
    a.update(kw)
    return lib.rsrgan_feat_denorm(a["y"], a["lengths"], a["B"], a["T"], a["D"], a["mean"], a["stddev"], a["out"], None)


def test_symbols_declared_bound_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsrgan.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rsrgan_[a-z_0-9]+)\s*\(", src))
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SYMBOLS and hasattr(lib, s), s
    assert len(lib.rsrgan_feat_stream.argtypes) == 15 and len(lib.rsrgan_feat_denorm.argtypes) == 9
    assert sorted(_lib.SYMBOLS) == sorted(declared)


# ---- rsrgan_feat_stream ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["table", "hist", "out"])
def test_stream_null_required_pointer(lib, which):
    refused(lib, stream(lib, **{which: None}), "feat_stream", "null pointer (table, hist or out)")


def test_stream_fresh_may_be_null_exactly_when_there_are_no_fresh_rows(lib):
    refused(lib, stream(lib, fresh=None), "feat_stream", "null pointer (fresh)", "fresh_rows = 40")
    # a flush-only call (fresh NULL, fresh_rows 0) is NOT refused for its fresh: the next refusal in line names something else
    refused(lib, stream(lib, fresh=None, fresh_rows=0, B=0), "feat_stream", "must be positive")
    refused(lib, stream(lib, fresh_rows=-1), "feat_stream", "fresh_rows = -1 is negative")


@pytest.mark.parametrize("which", ["mean", "stddev"])
def test_stream_only_one_of_mean_and_stddev(lib, which):
    refused(lib, stream(lib, **{which: None}), "feat_stream", "mean and stddev must both be given or both be null")
    refused(lib, stream(lib, mean=None, stddev=None, T=0), "feat_stream", "must be positive")         # both NULL: not refused for that


def test_stream_alignment(lib):
    for which, base in (("fresh", P), ("hist", P + 8192), ("out", P + 20480)):
        for off in (4, 8):
            refused(lib, stream(lib, **{which: base + off}), "feat_stream", "fresh, hist or out not 16-byte aligned")
    refused(lib, stream(lib, table=P + 4096 + 2), "feat_stream", "table or lengths not 4-byte aligned")
    refused(lib, stream(lib, lengths=P + 24576 + 1), "feat_stream", "table or lengths not 4-byte aligned")
    for which, base in (("mean", P + 12288), ("stddev", P + 16384)):
        refused(lib, stream(lib, **{which: base + 4}), "feat_stream", "mean or stddev not 8-byte aligned")
    refused(lib, stream(lib, lengths=None, D=0), "feat_stream", "must be positive")                    # lengths may be NULL


@pytest.mark.parametrize("which", ["B", "H", "T", "D"])
def test_stream_sizes_below_one(lib, which):
    for v in (0, -1):
        refused(lib, stream(lib, **{which: v}), "feat_stream", "B, H, T, D must be positive")


def test_stream_contexts(lib):
    refused(lib, stream(lib, left=-1), "feat_stream", "negative context (left -1, right 3)")
    refused(lib, stream(lib, right=-2), "feat_stream", "negative context (left 2, right -2)")
    refused(lib, stream(lib, left=1025), "feat_stream", "context above the entry's 1024")
    refused(lib, stream(lib, right=1025), "feat_stream", "context above the entry's 1024")


def test_stream_limits(lib):
    """at most 2^32 - 1 elements of out and of the ring, at most 2^40 fresh floats"""
    refused(lib, stream(lib, B=1 << 16, T=1 << 16, D=1, left=0, right=0), "feat_stream", "B x T x D x (left + 1 + right)",
            "above the entry's 2^32 - 1 elements")
    refused(lib, stream(lib, B=1 << 10, T=1 << 10, D=1 << 10, left=1, right=2), "B x T x D x (left + 1 + right)", "above the entry's 2^32 - 1 elements")
    refused(lib, stream(lib, B=(1 << 31) - 1, T=(1 << 31) - 1, D=(1 << 31) - 1, left=1024, right=1024), "above the entry's 2^32 - 1 elements")
    refused(lib, stream(lib, B=1 << 16, H=1 << 16, T=1, D=1), "feat_stream", "B x H x D = 65536 x 65536 x 1", "above the entry's 2^32 - 1 elements")
    refused(lib, stream(lib, B=(1 << 31) - 1, H=(1 << 31) - 1, T=1, D=1, left=0, right=0), "B x H x D", "above the entry's 2^32 - 1 elements")
    refused(lib, stream(lib, B=1, H=1 << 20, T=1, D=1 << 12), "B x H x D", "above the entry's 2^32 - 1 elements")
    refused(lib, stream(lib, fresh_rows=(1 << 40) // 7 + 1), "feat_stream", "fresh_rows x D", "above the entry's 2^40")


# ---- rsrgan_feat_denorm ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["y", "out"])
def test_denorm_null_required_pointer(lib, which):
    refused(lib, denorm(lib, **{which: None}), "feat_denorm", "null pointer (y or out)")


@pytest.mark.parametrize("null", [("mean",), ("stddev",), ("mean", "stddev")])
def test_denorm_needs_both_statistics(lib, null):
    refused(lib, denorm(lib, **{k: None for k in null}), "feat_denorm", "null pointer (mean or stddev): both are needed")


def test_denorm_alignment(lib):
    for off in (4, 8):
        refused(lib, denorm(lib, y=P + off), "feat_denorm", "y not 16-byte aligned")
    refused(lib, denorm(lib, lengths=P + 4096 + 2), "feat_denorm", "lengths not 4-byte aligned")
    for which, base in (("mean", P + 8192), ("stddev", P + 12288), ("out", P + 16384)):
        refused(lib, denorm(lib, **{which: base + 4}), "feat_denorm", "mean, stddev or out not 8-byte aligned")
    refused(lib, denorm(lib, out=P + 16384 + 8, lengths=None, B=0), "feat_denorm", "must be positive")  # 8 bytes do for out; lengths may be NULL


@pytest.mark.parametrize("which", ["B", "T", "D"])
def test_denorm_sizes_below_one(lib, which):
    for v in (0, -1):
        refused(lib, denorm(lib, **{which: v}), "feat_denorm", "B, T, D must be positive")


def test_denorm_limit(lib):
    refused(lib, denorm(lib, B=1 << 16, T=1 << 16, D=1), "feat_denorm", "B x T x D = 65536 x 65536 x 1", "above the entry's 2^32 - 1 elements")
    refused(lib, denorm(lib, B=(1 << 31) - 1, T=(1 << 31) - 1, D=(1 << 31) - 1), "above the entry's 2^32 - 1 elements")
    refused(lib, denorm(lib, B=1, T=1 << 20, D=1 << 12), "above the entry's 2^32 - 1 elements")
