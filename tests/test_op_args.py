"""The operator test entries (rsrgan_op_gemm2, _gemm_batch, _gemm16_batch, _lstm_colsums, _colsum, _gemm_last_plan) refuse every
argument error BEFORE their first HIP call, naming it in rsrgan_last_error(): so the refusals run here, without a device.  The
pointers are made-up addresses: a refused call never reads them."""
import ctypes as C

import pytest

from rsrgan_amd import _lib

ERR_INVALID = -1
P = 0x10000                                    # a non-null, 16-byte aligned "device pointer" nobody dereferences


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def refused(lib, rc, *words):
    assert rc == ERR_INVALID, rc
    msg = lib.rsrgan_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)
    return msg


def gemm2(lib, **kw):
    a = dict(A=P, lda=64, a_kc=0, A2=None, lda2=0, M1=0, B=P, ldb=64, b_kc=0, C=P, ldc=64, M=64, N=64, K=64, bias=None, act=0,
             alpha=0.3, acc=0, rows_per=0, outer=0, inner=0, workers=0, force=-1)
    a.update(kw)
    return lib.rsrgan_op_gemm2(a["A"], a["lda"], a["a_kc"], a["A2"], a["lda2"], a["M1"], a["B"], a["ldb"], a["b_kc"], a["C"], a["ldc"],
                               a["M"], a["N"], a["K"], a["bias"], a["act"], a["alpha"], a["acc"], a["rows_per"], a["outer"], a["inner"],
                               a["workers"], a["force"], None)


def tab(n, null_at=None):
    return _lib.ptr_table([None if i == null_at else P + 4096 * i for i in range(n)])


def gemm_batch(lib, nb=2, A="t", A2="t", B="t", C_="t", lda=64, lda2=64, M1=32, ldb=64, ldc=64, M=64, N=64, K=64, workers=0):
    t = lambda v: tab(nb) if isinstance(v, str) else v
    return lib.rsrgan_op_gemm_batch(nb, t(A), lda, t(A2), lda2, M1, t(B), ldb, t(C_), ldc, M, N, K, 0, workers, None)


def gemm16_batch(lib, n=2, A="t", A2="t", B="t", C_="t", lda=64, lda2=64, M1=32, ldb=64, ldc=64, M=64, N=64, K=64):
    t = lambda v: tab(max(n, 1)) if isinstance(v, str) else v
    return lib.rsrgan_op_gemm16_batch(n, t(A), lda, t(A2), lda2, M1, t(B), ldb, t(C_), ldc, M, N, K, 0, None)


def colsums(lib, nb=2, rows=8, H=8, null_table=None, null_entry=None):
    ts = [None if i == null_table else tab(max(nb, 1), null_at=0 if i == null_entry else None) for i in range(7)]
    return lib.rsrgan_op_lstm_colsums(nb, *ts, rows, H, None)


@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_gemm2_null_pointer(lib, which):
    refused(lib, gemm2(lib, **{which: None}), "op_gemm2", "null pointer")


@pytest.mark.parametrize("which", ["lda", "ldb", "ldc"])
def test_gemm2_leading_dimension(lib, which):
    refused(lib, gemm2(lib, **{which: 66}), "op_gemm2", "leading dimension", "multiple of 4")
    refused(lib, gemm2(lib, A2=P, M1=32, lda2=30), "leading dimension", "multiple of 4")


def test_gemm2_a2_with_a_kcontig(lib):
    refused(lib, gemm2(lib, A2=P, lda2=64, M1=32, a_kc=1), "A2 together with a_kcontig")


@pytest.mark.parametrize("M1", [1, 2, 3, 5, 30, 33, 62, 63])
def test_gemm2_m1_not_a_multiple_of_4(lib, M1):
    """every kernel -- k_gemm / k_gemm_s by 16-byte DMA chunk, k_gemm16 by float4 -- takes a chunk whole from A or whole from A2"""
    refused(lib, gemm2(lib, A2=P, lda2=64, M1=M1), "M1 = %d" % M1, "multiple of 4")
    refused(lib, gemm2(lib, A2=P, lda2=64, M1=M1, M=4100, N=4100, K=256), "M1 = %d" % M1, "multiple of 4")     # (the stream-K route)


def test_gemm2_m1_range_sizes_workers_force_and_map(lib):
    refused(lib, gemm2(lib, A2=P, lda2=64, M1=0), "M1 = 0")
    refused(lib, gemm2(lib, A2=P, lda2=64, M1=64), "M1 = 64")
    refused(lib, gemm2(lib, M=0), "positive")
    refused(lib, gemm2(lib, K=-1), "positive")
    refused(lib, gemm2(lib, workers=257), "workers = 257")
    refused(lib, gemm2(lib, workers=-8), "workers = -8")
    refused(lib, gemm2(lib, force=8), "force_cfg = 8")
    refused(lib, gemm2(lib, rows_per=-1), "rows_per = -1")
    refused(lib, gemm2(lib, rows_per=5, outer=64, inner=4, A2=P, lda2=64, M1=32), "A2 together with a row map")
    refused(lib, gemm2(lib, rows_per=5, outer=64, inner=4, b_kc=1), "row map together with b_kcontig")
    refused(lib, gemm2(lib, rows_per=5, outer=66, inner=4), "row map strides")
    refused(lib, gemm2(lib, rows_per=5, outer=64, inner=3), "row map strides")


def test_gemm_batch_refusals(lib):
    refused(lib, gemm_batch(lib, nb=0), "nb = 0")
    refused(lib, gemm_batch(lib, nb=-1), "nb = -1")
    for which in ("A", "B", "C_"):
        refused(lib, gemm_batch(lib, **{which: None}), "op_gemm_batch", "null pointer table")
        refused(lib, gemm_batch(lib, nb=3, **{which: tab(3, null_at=2)}), "null pointer in problem 2")
    refused(lib, gemm_batch(lib, A2=tab(2, null_at=1)), "null pointer in problem 1")
    for which in ("lda", "lda2", "ldb", "ldc"):
        refused(lib, gemm_batch(lib, **{which: 62}), "leading dimension", "multiple of 4")
    for M1 in (31, 33, 34):
        refused(lib, gemm_batch(lib, M1=M1), "M1 = %d" % M1, "multiple of 4")
    refused(lib, gemm_batch(lib, M1=64), "M1 = 64")
    refused(lib, gemm_batch(lib, N=0), "positive")
    refused(lib, gemm_batch(lib, workers=300), "workers = 300")


def test_gemm16_batch_refusals(lib):
    for n in (0, 5, -3):
        refused(lib, gemm16_batch(lib, n=n), "n = %d" % n, "outside the table")
    for which in ("A", "B", "C_"):
        refused(lib, gemm16_batch(lib, **{which: None}), "op_gemm16_batch", "null pointer table")
        refused(lib, gemm16_batch(lib, n=4, **{which: tab(4, null_at=3)}), "null pointer in problem 3")
    for which in ("lda", "lda2", "ldb", "ldc"):
        refused(lib, gemm16_batch(lib, **{which: 63}), "leading dimension", "multiple of 4")
    for M1 in (1, 30, 35):
        refused(lib, gemm16_batch(lib, M1=M1), "M1 = %d" % M1, "multiple of 4", "float4")
    refused(lib, gemm16_batch(lib, K=0), "positive")


def test_lstm_colsums_refusals(lib):
    for nb in (0, 5, -1):
        refused(lib, colsums(lib, nb=nb), "nb = %d" % nb, "outside the table")
    for i in range(7):
        refused(lib, colsums(lib, null_table=i), "op_lstm_colsums", "null pointer table")
        refused(lib, colsums(lib, null_entry=i), "null pointer in layer 0")
    refused(lib, colsums(lib, rows=0), "positive")
    refused(lib, colsums(lib, H=0), "positive")
    refused(lib, colsums(lib, nb=4, H=4096), "scratch")


def test_colsum_refusals(lib):
    f = lib.rsrgan_op_colsum
    refused(lib, f(None, 8, None, 0, P, 4, 8, 0, None), "op_colsum", "null pointer")
    refused(lib, f(P, 8, None, 0, None, 4, 8, 0, None), "op_colsum", "null pointer")
    refused(lib, f(P, 8, None, 0, P, 0, 8, 0, None), "positive")
    refused(lib, f(P, 8, None, 0, P, 4, 0, 0, None), "positive")
    refused(lib, f(P, 7, None, 0, P, 4, 8, 0, None), "leading dimension")
    refused(lib, f(P, 8, P, 4, P, 4, 8, 0, None), "leading dimension")
    refused(lib, f(P, 8, P, 8, P, 4, 8, 1, None), "tall form has no multiplier")


def test_last_plan_null_and_initial_record(lib):
    refused(lib, lib.rsrgan_op_gemm_last_plan(None), "op_gemm_last_plan", "null pointer")
    out = (C.c_int32 * 8)(*([-7] * 8))
    assert lib.rsrgan_op_gemm_last_plan(out) == 0
    assert all(v >= 0 for v in out) and out[0] in _lib.GEMM_CLASSES


def test_existing_gemm_entry_still_refuses(lib):
    rc = lib.rsrgan_op_gemm(None, 64, 0, P, 64, 0, P, 64, 8, 8, 8, None, 0, 0.3, 0, None)
    refused(lib, rc, "op_gemm")
    rc = lib.rsrgan_op_gemm(P, 62, 0, P, 64, 0, P, 64, 8, 8, 8, None, 0, 0.3, 0, None)
    refused(lib, rc, "multiple of 4")
