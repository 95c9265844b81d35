"""The operator test entries (rsrgan_op_gemm2, _gemm_batch, _gemm16_batch, _lstm_colsums, _colsum, _gemm_last_plan, _conv_*, _bn_*, _segan_*) refuse every
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


# ---- the convolution entries (csrc/conv.hip through launch_conv_prep / launch_conv_fwd / launch_conv_wgrad)
def conv_fwd(lib, **kw):
    a = dict(x=P, ldc_in=8, C=8, F=P, ldf=12, flip=0, bias=None, relu=0, mask=None, out=P, ldc_out=12, N=12, R=2, S=3, W=9, fw=3)
    a.update(kw)
    return lib.rsrgan_op_conv_fwd(a["x"], a["ldc_in"], a["C"], a["F"], a["ldf"], a["flip"], a["bias"], a["relu"], a["mask"], a["out"],
                                  a["ldc_out"], a["N"], a["R"], a["S"], a["W"], a["fw"], None)


def conv_wgrad(lib, **kw):
    a = dict(x=P, ldc_in=8, C=8, d=P, ldc_d=12, N=12, dW=P, ldw=12, db=None, ws=P, ws_floats=1 << 30, R_max=4, R=2, S=3, W=9, fw=3)
    a.update(kw)
    return lib.rsrgan_op_conv_wgrad(a["x"], a["ldc_in"], a["C"], a["d"], a["ldc_d"], a["N"], a["dW"], a["ldw"], a["db"], a["ws"],
                                    a["ws_floats"], a["R_max"], a["R"], a["S"], a["W"], a["fw"], None)


@pytest.mark.parametrize("which", ["x", "F", "out"])
def test_conv_fwd_null_pointer(lib, which):
    refused(lib, conv_fwd(lib, **{which: None}), "op_conv_fwd", "null pointer")


def test_conv_fwd_refusals(lib):
    for which in ("ldc_in", "ldc_out", "ldf"):
        refused(lib, conv_fwd(lib, **{which: 14}), "op_conv_fwd", "leading dimension", "multiple of 4")
    refused(lib, conv_fwd(lib, ldc_in=4), "leading dimension below its row")
    refused(lib, conv_fwd(lib, ldc_out=8), "leading dimension below its row")
    refused(lib, conv_fwd(lib, ldf=8), "leading dimension below its row")
    refused(lib, conv_fwd(lib, flip=1, C=12, N=8, ldc_in=12, ldc_out=8, ldf=8), "leading dimension below its row")     # flip: F has C columns
    refused(lib, conv_fwd(lib, bias=P + 4), "bias not 16-byte aligned")
    refused(lib, conv_fwd(lib, mask=P + 8), "not 16-byte aligned")
    refused(lib, conv_fwd(lib, x=P + 4), "not 16-byte aligned")
    refused(lib, conv_fwd(lib, R=0), "R = 0")
    refused(lib, conv_fwd(lib, R=1 << 20, S=3, W=9), "positions exceed the entry's 2^24")
    refused(lib, conv_fwd(lib, R=-2), "R = -2")
    for which in ("C", "N", "S", "W", "fw"):
        refused(lib, conv_fwd(lib, **{which: 0}), "positive")


def test_conv_fwd_unsupported_shape_is_not_applicable_without_a_device(lib):
    """the model's rule for the patch-matrix path: nothing is launched (no HIP call: this passes without a device)"""
    assert conv_fwd(lib, S=4) == _lib.OP_NOT_APPLICABLE
    assert conv_fwd(lib, fw=4) == _lib.OP_NOT_APPLICABLE
    assert conv_fwd(lib, N=33, ldc_out=36, ldf=36) == _lib.OP_NOT_APPLICABLE
    assert conv_fwd(lib, C=24, ldc_in=24, fw=13) == _lib.OP_NOT_APPLICABLE
    out = (C.c_int32 * 40)(*([-7] * 40))
    assert lib.rsrgan_op_conv_last_plan(out) == 0 and list(out) == [0] * 40


@pytest.mark.parametrize("which", ["x", "d", "dW", "ws"])
def test_conv_wgrad_null_pointer(lib, which):
    refused(lib, conv_wgrad(lib, **{which: None}), "op_conv_wgrad", "null pointer")


def test_conv_wgrad_refusals(lib):
    for which in ("ldc_in", "ldc_d", "ldw"):
        refused(lib, conv_wgrad(lib, **{which: 18}), "op_conv_wgrad", "leading dimension", "multiple of 4")
    refused(lib, conv_wgrad(lib, ldc_in=4), "leading dimension below its row")
    refused(lib, conv_wgrad(lib, ldc_d=8), "leading dimension below its row")
    refused(lib, conv_wgrad(lib, ldw=8), "leading dimension below its row")
    refused(lib, conv_wgrad(lib, R=0), "R = 0")
    refused(lib, conv_wgrad(lib, R=5), "R = 5", "R_max = 4")
    refused(lib, conv_wgrad(lib, ws=P + 4), "not 16-byte aligned")
    refused(lib, conv_wgrad(lib, dW=P + 2), "dW or db not 4-byte aligned")
    refused(lib, conv_wgrad(lib, db=P + 1), "dW or db not 4-byte aligned")
    refused(lib, conv_wgrad(lib, R=4, R_max=4, S=11, W=257 * 2048), "positions exceed")
    need = lib.rsrgan_op_conv_ws_floats(8, 4, 3, 9, 3)
    assert need > 0
    refused(lib, conv_wgrad(lib, ws_floats=need - 1), "workspace of %d floats" % (need - 1), "R_max = 4")
    refused(lib, conv_wgrad(lib, ws_floats=-1), "workspace")
    refused(lib, conv_wgrad(lib, ws_floats=lib.rsrgan_op_conv_ws_floats(8, 2, 3, 9, 3) - 1, R_max=4, R=2), "workspace")
    assert conv_wgrad(lib, S=4) == _lib.OP_NOT_APPLICABLE
    assert conv_wgrad(lib, N=33, ldc_d=36, ldw=36) == _lib.OP_NOT_APPLICABLE


def test_conv_supported_and_ws_floats_answer_without_a_device(lib):
    assert lib.rsrgan_op_conv_supported(12, 16, 11, 257, 13) == 3
    assert lib.rsrgan_op_conv_supported(1, 12, 11, 257, 13) == 3
    assert lib.rsrgan_op_conv_supported(24, 12, 3, 9, 13) == 0          # the filter slice exceeds 5 float4 per thread
    assert lib.rsrgan_op_conv_supported(4, 4, 4, 9, 3) == 0 and lib.rsrgan_op_conv_supported(4, 4, 3, 9, 4) == 0
    assert lib.rsrgan_op_conv_supported(4, 33, 3, 9, 3) == 0 and lib.rsrgan_op_conv_supported(6, 4, 3, 9, 3) == 0
    refused(lib, lib.rsrgan_op_conv_supported(4, 4, 0, 9, 3), "op_conv_supported", "positive")
    refused(lib, int(lib.rsrgan_op_conv_ws_floats(4, 0, 3, 9, 3)), "op_conv_ws_floats", "positive")
    # the group count is not monotonic in the frame count (S = 5, W = 257: 9 strips, gmax = 28): the size covers the worst R' <= R
    ws = [lib.rsrgan_op_conv_ws_floats(4, R, 5, 257, 3) for R in range(1, 61)]
    assert all(b >= a for a, b in zip(ws, ws[1:])) and ws[27] > ws[26] and ws[59] == ws[27]
    refused(lib, lib.rsrgan_op_conv_last_plan(None), "op_conv_last_plan", "null pointer")


# ---- the batch-renorm entries (csrc/bn.hip through launch_bn_forward / launch_bn_backward / launch_bn_commit_many / launch_bn_commit)
def bn_vars(null_at=None, odd_at=None, n=1):
    return _lib.ptr_table([None if i == null_at else P + 4096 * i + (2 if i == odd_at else 0) for i in range(8 * n)])


def bn_fwd(lib, **kw):
    a = dict(z=P, ldz=68, y=P, ldy=72, rows=16, cols=65, calls=1, vars=bn_vars(), stat=P, ldc=68, training=1, relu=1, scratch=P,
             scratch_floats=130)
    a.update(kw)
    return lib.rsrgan_op_bn_forward(a["z"], a["ldz"], a["y"], a["ldy"], a["rows"], a["cols"], a["calls"], a["vars"], a["stat"], a["ldc"],
                                    a["training"], a["relu"], a["scratch"], a["scratch_floats"], None)


def bn_bwd(lib, **kw):
    a = dict(dy=P, ldd=76, y=P, ldy=72, z=P, ldz=68, rows=16, cols=65, calls=1, stat=P, ldc=68, dbeta=P, dgamma=P, acc=0, relu=1, sums=P,
             scratch=P, scratch_floats=130)
    a.update(kw)
    return lib.rsrgan_op_bn_backward(a["dy"], a["ldd"], a["y"], a["ldy"], a["z"], a["ldz"], a["rows"], a["cols"], a["calls"], a["stat"],
                                     a["ldc"], a["dbeta"], a["dgamma"], a["acc"], a["relu"], a["sums"], a["scratch"], a["scratch_floats"], None)


def bn_commit(lib, n=1, vars="t", stat="t", dims=None, single=0):
    m = max(n, 1)
    d = [65, 68, 1, 0] * m if dims is None else dims
    return lib.rsrgan_op_bn_commit(n, bn_vars(n=m) if isinstance(vars, str) else vars, tab(m) if isinstance(stat, str) else stat,
                                   (C.c_int32 * len(d))(*d), single, None)


@pytest.mark.parametrize("which", ["z", "y", "vars", "stat", "scratch"])
def test_bn_forward_null_pointer(lib, which):
    refused(lib, bn_fwd(lib, **{which: None}), "op_bn_forward", "null pointer")


def test_bn_forward_refusals(lib):
    for which in ("ldz", "ldy", "ldc"):
        refused(lib, bn_fwd(lib, **{which: 70}), "op_bn_forward", "leading dimension", "multiple of 4")
        refused(lib, bn_fwd(lib, **{which: 64}), "leading dimension below its padded row of 68")
    for which in ("rows", "cols", "calls"):
        refused(lib, bn_fwd(lib, **{which: 0}), "positive")
        refused(lib, bn_fwd(lib, **{which: -3}), "positive")
    refused(lib, bn_fwd(lib, rows=1 << 20, calls=1 << 11), "above the entry's 2^30")
    # one slice of partial sums is 2 x cols floats: bn_slices answers 1 slice for anything less and the kernels would write past it
    refused(lib, bn_fwd(lib, scratch_floats=129), "scratch of 129 floats", "2 x cols = 130")
    refused(lib, bn_fwd(lib, scratch_floats=0), "scratch of 0 floats")
    refused(lib, bn_fwd(lib, scratch_floats=-1), "scratch")
    refused(lib, bn_fwd(lib, training=0, scratch_floats=129), "scratch")            # (the same rule without partial sums: one contract)
    for which in ("z", "y", "stat"):
        refused(lib, bn_fwd(lib, **{which: P + 4}), "not 16-byte aligned")
    refused(lib, bn_fwd(lib, scratch=P + 2), "scratch not 4-byte aligned")
    for i in range(8):
        refused(lib, bn_fwd(lib, vars=bn_vars(null_at=i)), "op_bn_forward", "eight variables")
        refused(lib, bn_fwd(lib, vars=bn_vars(odd_at=i)), "eight variables")


@pytest.mark.parametrize("which", ["dy", "y", "z", "stat", "sums", "scratch"])
def test_bn_backward_null_pointer(lib, which):
    refused(lib, bn_bwd(lib, **{which: None}), "op_bn_backward", "null pointer")


def test_bn_backward_refusals(lib):
    refused(lib, bn_bwd(lib, dbeta=None), "dbeta and dgamma")
    refused(lib, bn_bwd(lib, dgamma=None), "dbeta and dgamma")
    for which in ("ldd", "ldy", "ldz", "ldc"):
        refused(lib, bn_bwd(lib, **{which: 74}), "op_bn_backward", "leading dimension", "multiple of 4")
        refused(lib, bn_bwd(lib, **{which: 64}), "leading dimension below its padded row of 68")
    for which in ("rows", "cols", "calls"):
        refused(lib, bn_bwd(lib, **{which: 0}), "positive")
    refused(lib, bn_bwd(lib, scratch_floats=129), "scratch of 129 floats", "2 x cols = 130")
    refused(lib, bn_bwd(lib, acc=1, scratch_floats=64), "scratch of 64 floats")
    for which in ("dy", "y", "z", "stat", "sums"):
        refused(lib, bn_bwd(lib, **{which: P + 8}), "not 16-byte aligned")
    for which in ("scratch", "dbeta", "dgamma"):
        refused(lib, bn_bwd(lib, **{which: P + 1}), "not 4-byte aligned")


def test_bn_commit_refusals(lib):
    for n in (0, 25, -1):
        refused(lib, bn_commit(lib, n=n), "op_bn_commit", "n = %d" % n, "1 .. 24")
    refused(lib, bn_commit(lib, vars=None), "null pointer table")
    refused(lib, bn_commit(lib, stat=None), "null pointer table")
    refused(lib, lib.rsrgan_op_bn_commit(1, bn_vars(), tab(1), None, 0, None), "null pointer table")
    refused(lib, bn_commit(lib, n=3, vars=bn_vars(null_at=8 * 2 + 5, n=3)), "variables of entry 2")
    refused(lib, bn_commit(lib, n=2, stat=tab(2, null_at=1)), "stat of entry 1")
    refused(lib, bn_commit(lib, dims=[65, 68, -1, 0]), "negative times (-1, 0) in entry 0")
    refused(lib, bn_commit(lib, n=2, dims=[65, 68, 1, 0, 65, 68, 2, -2]), "negative times (2, -2) in entry 1")
    refused(lib, bn_commit(lib, dims=[0, 68, 1, 0]), "cols = 0")
    refused(lib, bn_commit(lib, dims=[65, 64, 1, 0]), "ldc = 64")
    refused(lib, bn_commit(lib, dims=[65, 70, 1, 0]), "ldc = 70")
    refused(lib, bn_commit(lib, n=2, single=1), "single-entry form")
    refused(lib, bn_commit(lib, dims=[65, 68, 1, 1], single=1), "single-entry form")


def test_bn_last_plan_null_and_initial_record(lib):
    refused(lib, lib.rsrgan_op_bn_last_plan(None), "op_bn_last_plan", "null pointer")
    out = (C.c_int32 * 16)(*([-7] * 16))
    assert lib.rsrgan_op_bn_last_plan(out) == 0
    # (the record is per thread and outlives a test: all zero in a fresh process, the last launch's plan after tests/test_gpu_bn_ops.py)
    assert out[0] in _lib.BN_ROUTES and all(v >= 0 for v in out) and list(out[11:]) == [0] * 5
    refused(lib, bn_fwd(lib, rows=0), "positive")
    again = (C.c_int32 * 16)(*([-7] * 16))
    assert lib.rsrgan_op_bn_last_plan(again) == 0 and list(again) == list(out)   # a refused call launches nothing and records nothing


# ---- rsrgan_op_segan_*: (family, op) -> (number of pointers, optional pointer slots, a valid dims table, floats)
SEGAN_VALID = {
    ("conv2", 0): (5, {2}, [2, 9, 16, 5, 48, 48, None], []),                     # pad_floats filled from rsrgan_op_segan_sizes
    ("conv2", 1): (4, set(), [2, 9, 16, 5, 48, 48, 48, None], []),
    ("conv2", 2): (9, {2}, [2, 5, 16, 9, 5, 48, 16, None, None, None, None], []),
    ("conv1", 0): (4, {2}, [2, 37, 31, 16, 40, 16, 16], []),
    ("conv1", 1): (4, set(), [2, 37, 31, 16, 40, 16, 16, 2 * 31 * 16], []),
    ("conv1", 2): (4, {2}, [2, 19, 16, 37, 31, 16, 16, 40], []),
    ("colred", 3): (5, set(), [16, 0, 16, 16, 100, 2, 16, 16, 0, 64], [0.3]),
    ("vbn", 0): (5, {3}, [16, 9, 3, 16, 16, 2], [1e-5]),
    ("vbn", 1): (3, set(), [16, 9, 3, 16], [0.3]),
    ("vbn", 2): (5, {3, 4}, [16, 9, 3, 16, 16, 2, 1, 0], [0.0]),
    ("vbn", 3): (4, set(), [16, 9, 3, 16], [0.3]),
    ("elem", 0): (2, set(), [2, 9, 16, 3, 4], [0.0]),
    ("elem", 1): (2, set(), [1, 16, 16, 16, 0, 3, 16], [0.0]),
    ("elem", 2): (4, set(), [2, 16, 16, 16, 0, 3, 16, 16, 16, 16, 1, 2, 16], [0.0]),
    ("elem", 3): (4, {2}, [5, 4, 0, 1, 2, 2, 9, 16], [0.0]),
    ("elem", 4): (3, {1}, [16, 40, 8, 9], [0.3]),
    ("elem", 5): (5, {2, 3}, [40, 8, 16, 9], [0.3]),
    ("elem", 6): (2, set(), [40, 8, 32, 4, 16, 9, 0], [0.0]),
    ("elem", 7): (4, {2}, [37, 5, 2], [0.0]),
    ("elem", 8): (3, set(), [9, 37, 40], [0.0]),
    ("elem", 9): (3, {1}, [4, 0, 2, 3], [0.0]),
    ("elem", 10): (5, {3}, [300, 1], [0.0]),
    ("elem", 11): (4, set(), [300], [0.9, 1e-10]),
    ("dhead", 0): (6, set(), [3, 9, 16, 5, 1], []),
    ("dhead", 1): (9, {5, 6, 7}, [3, 9, 16, 5, 1], []),
}


def segan_sizes(lib, kind, dims):
    out = (C.c_int64 * 12)()
    rc = lib.rsrgan_op_segan_sizes(kind, (C.c_int64 * len(dims))(*dims), out)
    return rc, list(out)


def segan_call(lib, family, op, null_at=None, misalign_at=None, dims=None, **patch):
    n, _, valid, fl = SEGAN_VALID[(family, op)]
    d = list(valid if dims is None else dims)
    if family == "conv2":                                       # the model's sizes for the valid layer
        if op == 2:
            s = segan_sizes(lib, 1, [2, 5, 16, 9, 48, 5])[1]
            for i, v in zip((7, 8, 9, 10), s[:4]):
                d[i] = v if d[i] is None else d[i]
        else:
            i = 6 if op == 0 else 7
            d[i] = segan_sizes(lib, 0, [2, 9, 16, 5])[1][0] if d[i] is None else d[i]
    for i, v in patch.get("set", {}).items():
        d[i] = v
    ptrs = [None if i == null_at else P + 4096 * i + (4 if i == misalign_at else 0) for i in range(n)]
    return getattr(lib, "rsrgan_op_segan_" + family)(op, (C.c_void_p * n)(*ptrs), (C.c_int64 * len(d))(*d), (C.c_float * max(len(fl), 1))(*fl), None)


@pytest.mark.parametrize("family,op", sorted(SEGAN_VALID))
def test_segan_null_pointers_and_tables(lib, family, op):
    n, optional, valid, fl = SEGAN_VALID[(family, op)]
    fn = getattr(lib, "rsrgan_op_segan_" + family)
    refused(lib, fn(op, None, (C.c_int64 * 16)(), (C.c_float * 2)(), None), "op_segan_" + family, "null table")
    refused(lib, fn(99, (C.c_void_p * 16)(), (C.c_int64 * 16)(), (C.c_float * 2)(), None), "op_segan_" + family, "outside")
    for i in range(n):
        if i not in optional:
            refused(lib, segan_call(lib, family, op, null_at=i), "op_segan_" + family, "null pointer")
    if optional & {5, 6, 7} and family == "dhead":
        refused(lib, segan_call(lib, family, op, null_at=6), "all be given or all be null")
    if family == "vbn" and op == 2:
        refused(lib, segan_call(lib, family, op, null_at=3), "both be given or both be null")


@pytest.mark.parametrize("family,op", sorted(SEGAN_VALID))
def test_segan_sizes_below_one(lib, family, op):
    """every slot of every dims table at -1 (sizes, offsets, flags and scratch sizes alike), and a size beyond the entry's limit"""
    valid = SEGAN_VALID[(family, op)][2]
    for i in range(len(valid)):
        refused(lib, segan_call(lib, family, op, set={i: -1}), "op_segan_" + family)
    refused(lib, segan_call(lib, family, op, set={0: 1 << 40}), "op_segan_" + family)


def test_segan_conv2_refusals(lib):
    refused(lib, segan_call(lib, "conv2", 0, set={2: 18}), "Cin", "multiple of 4")
    refused(lib, segan_call(lib, "conv2", 0, set={4: 50, 5: 52}), "Cout", "multiple of 4")
    refused(lib, segan_call(lib, "conv2", 0, set={5: 44}), "leading dimension ldw")
    refused(lib, segan_call(lib, "conv2", 0, set={5: 50}), "ldw", "multiple of 4")
    refused(lib, segan_call(lib, "conv2", 0, misalign_at=4), "pad not 16-byte aligned")
    need = segan_sizes(lib, 0, [2, 9, 16, 5])[1][0]
    assert need == 2 * (9 + 4) * 16 + 64                        # same_pad(9, 5): out 5, total (5 - 1) * 2 + 5 - 9 = 4
    refused(lib, segan_call(lib, "conv2", 0, set={6: need - 1}), "pad of", "the model gives")
    refused(lib, segan_call(lib, "conv2", 1, set={7: need - 1}), "pad of", "the model gives")
    refused(lib, segan_call(lib, "conv2", 1, set={5: 44}), "leading dimension ldz")
    s = segan_sizes(lib, 1, [2, 5, 16, 9, 48, 5])[1]
    # tgeom(5, 9, 5): pl = 2, ne = {3, 2}, i0 = {0, 1}, Q = {5, 4}, q0 = {1, 1}: pf = 1, pb = 1
    assert s[:11] == [2 * 7 * 16 + 64, 2 * 5 * 48 + 64, 3 * 16 * 48, 2 * 16 * 48, 2, 0, 1, 5, 4, 1, 1], s
    for i, word in ((7, "pad of"), (8, "t0 / t1 of"), (9, "Wt0 of"), (10, "Wt1 of")):
        refused(lib, segan_call(lib, "conv2", 2, set={i: s[i - 7] - 1}), word)
    refused(lib, segan_call(lib, "conv2", 2, set={3: 8, 1: 5}), "not ceil(Lt / 2)")
    refused(lib, segan_call(lib, "conv2", 2, set={4: 1}), "k = 1")
    refused(lib, segan_call(lib, "conv2", 2, misalign_at=7), "Wt0 not 16-byte aligned")
    assert segan_sizes(lib, 1, [2, 1, 16, 1, 48, 5])[1][7:9] == [1, 0]            # Ls = Lt = 1: one empty parity class
    refused(lib, segan_sizes(lib, 1, [2, 5, 16, 8, 48, 5])[0], "op_segan_sizes", "not ceil(Lt / 2)")
    refused(lib, segan_sizes(lib, 7, [1])[0], "kind = 7")
    refused(lib, lib.rsrgan_op_segan_sizes(0, None, None), "null pointer")


def test_segan_conv1_refusals(lib):
    refused(lib, segan_call(lib, "conv1", 0, set={3: 20, 5: 20, 6: 20}), "C = 20", "multiple of 16")
    refused(lib, segan_call(lib, "conv1", 0, set={4: 36}), "leading dimension ldx")
    refused(lib, segan_call(lib, "conv1", 0, set={6: 18}), "ldz")
    refused(lib, segan_call(lib, "conv1", 0, misalign_at=3), "z not 16-byte aligned")
    # launch_conv1_wgrad would abort() on these: refused, never launched
    refused(lib, segan_call(lib, "conv1", 1, set={2: 33, 3: 32, 5: 32, 6: 32, 7: 1 << 20}), "k x C = 1056 above 1024")
    refused(lib, segan_call(lib, "conv1", 1, set={2: 17, 3: 64, 5: 64, 6: 64, 7: 1 << 20}), "k x C = 1088 above 1024")
    refused(lib, segan_call(lib, "conv1", 1, set={3: 18, 5: 20, 6: 20}), "no multiple of 4")
    refused(lib, segan_call(lib, "conv1", 1, set={5: 18}), "ldz", "multiple of 4")
    refused(lib, segan_call(lib, "conv1", 1, set={7: 2 * 31 * 16 - 1}), "scratch of", "B x k x C")
    refused(lib, segan_call(lib, "conv1", 1, set={0: 70000, 7: 1 << 30}), "65535")
    assert segan_sizes(lib, 2, [32, 32])[1][:2] == [1, (512 * 32 + 1024 + 32) * 4]
    assert segan_sizes(lib, 2, [31, 32])[1][1] == 69756                          # the reference's first D block: 69.7 KB
    assert segan_sizes(lib, 2, [33, 32])[1][0] == 0 and segan_sizes(lib, 2, [21, 48])[1][0] == 1 and segan_sizes(lib, 2, [8, 6])[1][0] == 0
    refused(lib, segan_call(lib, "conv1", 2, set={2: 18, 5: 20, 6: 20}), "C = 18", "multiple of 4")
    refused(lib, segan_call(lib, "conv1", 2, set={1: 18}), "not ceil(Lt / 2)")
    refused(lib, segan_call(lib, "conv1", 2, set={7: 36}), "leading dimension ldt")


def test_segan_colred_refusals(lib):
    before = (C.c_int32 * 8)()
    assert lib.rsrgan_op_segan_last_plan(before) == 0
    for mode in (-1, 4):
        refused(lib, lib.rsrgan_op_segan_colred(mode, (C.c_void_p * 5)(), (C.c_int64 * 10)(), (C.c_float * 1)(), None), "mode = %d" % mode)
    n, _, valid, fl = SEGAN_VALID[("colred", 3)]

    def colred(mode, null_at=None, **set_):
        d = list(valid)
        for i, v in set_.items():
            d[int(i[1:])] = v
        ptrs = [None if i == null_at else P + 4096 * i for i in range(5)]
        return lib.rsrgan_op_segan_colred(mode, (C.c_void_p * 5)(*ptrs), (C.c_int64 * 10)(*d), (C.c_float * 1)(0.3), None)
    assert segan_sizes(lib, 3, [16, 2])[1][0] == 64
    for mode in range(4):
        refused(lib, colred(mode, d9=63), "scratch of 63 floats below the P x 2 x C = 64")     # one float short: refused, the doubling never starts
        refused(lib, colred(mode, d0=12), "leading dimension lda")
        refused(lib, colred(mode, d1=4), "leading dimension lda")                # coff + C beyond the row
        refused(lib, colred(mode, d7=12), "leading dimension ldo")
        refused(lib, colred(mode, null_at=0), "null pointer (a)")
    for mode in (1, 3):
        refused(lib, colred(mode, null_at=1), "null pointer (b)")
        refused(lib, colred(mode, d2=12), "leading dimension ldb")
    refused(lib, colred(3, null_at=2), "null pointer (coef)")
    refused(lib, colred(3, d6=12), "leading dimension ldcoef")
    refused(lib, colred(0, d5=65), "P above 64")
    refused(lib, lib.rsrgan_op_segan_last_plan(None), "op_segan_last_plan", "null pointer")
    out = (C.c_int32 * 8)()
    assert lib.rsrgan_op_segan_last_plan(out) == 0 and list(out) == list(before)      # a refused call launches nothing and records nothing


def test_segan_elem_vbn_dhead_refusals(lib):
    refused(lib, segan_call(lib, "elem", 0, set={2: 18}), "C = 18", "multiple of 4")
    refused(lib, segan_call(lib, "elem", 0, misalign_at=1), "dst not 16-byte aligned")
    refused(lib, segan_call(lib, "elem", 1, set={0: 2}), "launch_prep_tconv: 1")
    refused(lib, segan_call(lib, "elem", 2, set={0: 133}), "1 .. 132")
    refused(lib, segan_call(lib, "elem", 2, set={10: 2}), "e = 2 of job 1")
    refused(lib, segan_call(lib, "elem", 2, set={12: 12}), "leading dimension ldd")
    refused(lib, segan_call(lib, "elem", 3, set={2: 1}), "i00 = 1 is not the first position of parity class 0 under pl = 2")
    refused(lib, segan_call(lib, "elem", 3, set={1: 3}), "Q1 = 3 below the 4 positions")
    refused(lib, segan_call(lib, "elem", 3, set={7: 18}), "multiple of 4")
    refused(lib, segan_call(lib, "elem", 4, set={1: 20}), "leading dimension ldo")
    refused(lib, segan_call(lib, "elem", 5, set={0: 20}), "leading dimension ldy")
    refused(lib, segan_call(lib, "elem", 6, set={0: 20}), "leading dimension lds")
    refused(lib, segan_call(lib, "elem", 6, set={2: 16}), "leading dimension ldd")
    refused(lib, segan_call(lib, "elem", 8, set={2: 36}), "leading dimension ld")
    refused(lib, segan_call(lib, "elem", 9, set={1: 2}), "mode = 2")
    refused(lib, segan_call(lib, "elem", 9, set={1: 1, 2: 3}), "fake_pass")
    refused(lib, segan_call(lib, "elem", 6, set={6: 2}), "accumulate = 2 is neither 0 nor 1")
    refused(lib, segan_call(lib, "vbn", 0, set={3: 12}), "leading dimension ldc")
    refused(lib, segan_call(lib, "vbn", 0, set={4: 12}), "leading dimension lds")
    refused(lib, segan_call(lib, "vbn", 2, set={6: 2}), "first_live = 2")
    refused(lib, segan_call(lib, "vbn", 1, set={2: 65}), "P above 64")
    refused(lib, segan_call(lib, "dhead", 1, set={0: 1 << 20, 1: 1 << 10}), "2^28")


def test_segan_null_float_table(lib):
    """fl may be NULL exactly where include/rsrgan.h lists no float: ops that take one refuse NULL; the others get past it to their own checks"""
    def call(family, op, **kw):
        n, _, valid, _ = SEGAN_VALID[(family, op)]
        d = list(valid)
        for i, v in kw.items():
            d[int(i[1:])] = v
        ptrs = [P + 4096 * i for i in range(n)]
        return getattr(lib, "rsrgan_op_segan_" + family)(op, (C.c_void_p * n)(*ptrs), (C.c_int64 * len(d))(*d), None, None)
    for family, op in (("vbn", 0), ("vbn", 1), ("vbn", 3), ("elem", 4), ("elem", 5), ("elem", 11), ("colred", 3)):
        refused(lib, call(family, op), "null table", "fl")
    refused(lib, call("elem", 0, d2=18), "C = 18")                 # pad_rows, copy_cols, bwd_coef: NULL fl is fine, the next check speaks
    refused(lib, call("elem", 6, d6=2), "accumulate = 2")
    refused(lib, call("vbn", 2, d6=2), "first_live = 2")


def test_segan_create_refuses_what_would_abort_in_a_step(lib):
    """configs whose single-channel weight gradient has no kernel (k * C > 1024) or whose depths exceed the column-sum buffer are refused
    at create time, before the device is asked for"""
    def create(**kw):
        cfg = _lib.SeganCfg()
        assert lib.rsrgan_segan_default_cfg(C.byref(cfg)) == 0
        cfg.n_layers, cfg.input_len, cfg.batch_size = 2, 64, 2
        for k, v in kw.items():
            if k.endswith("depths"):
                for i, x in enumerate(v):
                    getattr(cfg, k)[i] = x
            else:
                setattr(cfg, k, v)
        h = C.c_void_p()
        return lib.rsrgan_segan_create(C.byref(cfg), 1, C.byref(h))
    refused(lib, create(g_depths=[32, 32], g_kwidth=31), "g_kwidth * 2 * g_depths[0] = 1984", "1024")
    refused(lib, create(d_depths=[48, 48], d_kwidth=31), "d_kwidth * d_depths[0] = 1488", "1024")
    refused(lib, create(d_depths=[16, 2064], d_kwidth=5), "d_depths above 2048")
    assert segan_sizes(lib, 2, [20, 2 * 16])[1][0] == 1 and segan_sizes(lib, 2, [31, 16])[1][0] == 1      # the reference's own shapes pass
