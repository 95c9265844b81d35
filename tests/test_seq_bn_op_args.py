"""rsrgan_op_bn_seq_forward / _backward refuse every argument error before their first HIP call, as the entries of
tests/test_op_args.py do: the refusals of rsrgan_op_bn_forward / _backward, plus alpha, the row rule (Bp, Bt) and rows % Bp.
The pointers are made-up addresses: a refused call never reads them."""
import pytest

from rsrgan_amd import _lib
from tests.test_op_args import P, bn_vars, refused


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def fwd(lib, **kw):
    a = dict(z=P, ldz=68, y=P, ldy=72, rows=64, cols=65, vars=bn_vars(), stat=P, ldc=68, training=1, relu=1, alpha=0.3, Bp=32, Bt=8,
             scratch=P, scratch_floats=130)
    a.update(kw)
    return lib.rsrgan_op_bn_seq_forward(a["z"], a["ldz"], a["y"], a["ldy"], a["rows"], a["cols"], a["vars"], a["stat"], a["ldc"], a["training"],
                                        a["relu"], a["alpha"], a["Bp"], a["Bt"], a["scratch"], a["scratch_floats"], None)


def bwd(lib, **kw):
    a = dict(dy=P, ldd=76, y=P, ldy=72, z=P, ldz=68, rows=64, cols=65, stat=P, ldc=68, dbeta=P, dgamma=P, acc=0, relu=1, alpha=0.3, Bp=32,
             Bt=8, sums=P, scratch=P, scratch_floats=130)
    a.update(kw)
    return lib.rsrgan_op_bn_seq_backward(a["dy"], a["ldd"], a["y"], a["ldy"], a["z"], a["ldz"], a["rows"], a["cols"], a["stat"], a["ldc"],
                                         a["dbeta"], a["dgamma"], a["acc"], a["relu"], a["alpha"], a["Bp"], a["Bt"], a["sums"], a["scratch"],
                                         a["scratch_floats"], None)


def test_symbols_are_bound():
    assert "rsrgan_op_bn_seq_forward" in _lib.SYMBOLS and "rsrgan_op_bn_seq_backward" in _lib.SYMBOLS


@pytest.mark.parametrize("which", ["z", "y", "vars", "stat", "scratch"])
def test_forward_null_pointer(lib, which):
    refused(lib, fwd(lib, **{which: None}), "op_bn_seq_forward", "null pointer")


@pytest.mark.parametrize("which", ["dy", "y", "z", "stat", "sums", "scratch"])
def test_backward_null_pointer(lib, which):
    refused(lib, bwd(lib, **{which: None}), "op_bn_seq_backward", "null pointer")


@pytest.mark.parametrize("call,who", [(fwd, "op_bn_seq_forward"), (bwd, "op_bn_seq_backward")])
def test_shape_alignment_and_rule_refusals(lib, call, who):
    lds = ("ldz", "ldy", "ldc") + (("ldd",) if call is bwd else ())
    for which in lds:
        refused(lib, call(lib, **{which: 70}), who, "leading dimension", "multiple of 4")
        refused(lib, call(lib, **{which: 64}), "leading dimension below its padded row of 68")
    for which in ("rows", "cols"):
        refused(lib, call(lib, **{which: 0}), "positive")
    refused(lib, call(lib, scratch_floats=129), "scratch of 129 floats", "2 x cols = 130")
    for which in (("z", "y", "stat") if call is fwd else ("dy", "y", "z", "stat", "sums")):
        refused(lib, call(lib, **{which: P + 4}), "not 16-byte aligned")
    refused(lib, call(lib, scratch=P + 2), "not 4-byte aligned")
    for a in (-0.1, 1.5, float("nan"), float("inf")):
        refused(lib, call(lib, alpha=a), who, "alpha", "outside [0, 1]")
    for Bp, Bt in ((-1, 0), (0, 3), (32, 0), (32, 33), (32, -1)):
        refused(lib, call(lib, Bp=Bp, Bt=Bt), who, "row rule (Bp %d, Bt %d)" % (Bp, Bt))
    refused(lib, call(lib, rows=65), who, "rows = 65 is no multiple of Bp = 32")
    if call is bwd:
        refused(lib, bwd(lib, dbeta=None), "dbeta and dgamma must both be given or both be null")
        refused(lib, bwd(lib, dgamma=P + 2), "not 4-byte aligned")
    for i in range(8) if call is fwd else ():
        refused(lib, fwd(lib, vars=bn_vars(null_at=i)), "eight variables")
