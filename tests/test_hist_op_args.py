"""rsrgan_hist (csrc/hist.hip) refuses every argument error before any device work, as rsrgan_feat_batch does (tests/test_feat_op_args.py),
naming the argument in rsrgan_last_error(); rsrgan_hist_limits is built on the host and equals summary._LIMITS bit for bit.  The
pointers are made-up addresses: a refused call never reads them, and no device is needed."""
import ctypes as C

import numpy as np
import pytest

from rsrgan_amd import _lib
from rsrgan_amd import summary as S
from tests.test_op_args import P, refused


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def hist(lib, n=2, x="t", dims="t", out=P + 65536, shapes=((3, 5, 5), (7, 1, 4)), null_at=None, ptr_off=0):
    xs = _lib.ptr_table([None if i == null_at else P + 4096 * i + ptr_off for i in range(max(n, 1))]) if x == "t" else x
    flat = [v for s in shapes for v in s] or [0]
    dm = (C.c_int64 * len(flat))(*flat) if dims == "t" else dims
    return lib.rsrgan_hist(n, xs, dm, out, None)


def test_symbols_are_bound(lib):
    for name, nargs in (("rsrgan_hist", 5), ("rsrgan_hist_limits", 2), ("rsrgan_d_logits", 5), ("rsrgan_d_logits_hist", 3)):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs


def test_count_below_one_or_above_the_entry_s_sixteen(lib):
    for n in (0, -1):
        refused(lib, hist(lib, n=n), "hist", "at least one tensor")
    refused(lib, hist(lib, n=17, shapes=((1, 1, 1),) * 17), "hist", "above the entry's 16 tensors")


@pytest.mark.parametrize("which", ["x", "dims", "out"])
def test_null_table_or_output(lib, which):
    refused(lib, hist(lib, **{which: None}), "hist", "null pointer (x, dims or out)")


def test_null_tensor_with_elements(lib):
    refused(lib, hist(lib, null_at=1), "hist", "tensor 1", "null pointer (x[1])", "7 x 1 elements")


def test_alignment(lib):
    refused(lib, hist(lib, out=P + 65536 + 4), "hist", "out not 8-byte aligned")
    refused(lib, hist(lib, ptr_off=2), "hist", "tensor 0", "not 4-byte aligned")


def test_leading_dimension_below_the_row(lib):
    refused(lib, hist(lib, shapes=((3, 5, 5), (7, 4, 3))), "hist", "tensor 1", "ld = 3 below its row of 4")


@pytest.mark.parametrize("shape", [(-1, 5, 5), (3, -5, 5), (3, 0, -1)])
def test_negative_sizes(lib, shape):
    refused(lib, hist(lib, shapes=(shape, (7, 1, 4))), "hist", "tensor 0", "negative size")


def test_more_than_2_31_minus_1_elements(lib):
    refused(lib, hist(lib, shapes=((1 << 16, 1 << 15, 1 << 15), (7, 1, 4))), "hist", "tensor 0", "above the entry's 2^31 - 1 elements")
    refused(lib, hist(lib, shapes=((3, 5, 5), (1, 1 << 31, 1 << 31))), "hist", "tensor 1", "above the entry's 2^31 - 1 elements")
    refused(lib, hist(lib, shapes=(((1 << 62), (1 << 62), (1 << 62)), (7, 1, 4))), "hist", "above the entry's 2^31 - 1 elements")
    refused(lib, hist(lib, shapes=((3, 5, (1 << 40) + 1), (7, 1, 4))), "hist", "ld = 1099511627777 above the entry's 2^40")


def test_handle_entries_refuse_a_null_handle(lib):
    t = C.c_int32()
    assert lib.rsrgan_d_logits(None, None, None, C.byref(t), None) == -1 and b"null handle" in lib.rsrgan_last_error()
    assert lib.rsrgan_d_logits_hist(None, P, None) == -1 and b"null handle" in lib.rsrgan_last_error()


def test_limits_equal_the_python_table_bit_for_bit(lib):
    n = C.c_int32()
    assert lib.rsrgan_hist_limits(None, C.byref(n)) == 0 and n.value == len(S._LIMITS)
    buf = (C.c_double * n.value)()
    assert lib.rsrgan_hist_limits(buf, C.byref(n)) == 0
    got = np.frombuffer(buf, np.float64)
    assert np.array_equal(got.view(np.uint64), S._LIMITS.view(np.uint64))
    assert np.array_equal(_lib.hist_limits().view(np.uint64), S._LIMITS.view(np.uint64))
    refused(lib, lib.rsrgan_hist_limits(buf, None), "hist_limits", "null pointer (n)")
