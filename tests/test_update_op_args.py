"""rsrgan_op_chunks, rsrgan_op_update and rsrgan_op_step_elem refuse every argument error BEFORE their first HIP call, naming it in
rsrgan_last_error(): so the refusals run here, without a device.  The pointers are made-up addresses: a refused call never reads them.
The chunk table itself is host code: it is checked here against a chunking written out in this file."""
import ctypes as C

import pytest

from rsrgan_amd import _lib

ERR_INVALID = -1
P = 0x10000                                    # a non-null, 16-byte aligned "device pointer" nobody dereferences
TENSORS = [(0, 4, 1), (64, 4100, 0), (4224, 40, 1)]                # (float offset, floats, l2 flag): 1 + 2 + 1 chunks
BUF = 4288

# valid arguments of every op: (number of pointers, pointers that may be NULL, dims, fl)
UPDATE = {"sumsq": (2, (), ()), "dw_reduce": (3, (), (4288, 2, 2 * 4288)), "l2": (4, (), ()), "apply_sgd": (5, (2,), ()),
          "apply_adam": (7, (4,), (11,))}
ELEM = {"lsgan": (5, (1,), [3, 8, 4, 4, 1, 4, 2], [-0.5, 1.5]),
        "dhead": (12, (), [3, 8, 4, 40, 40, 4, 4, 40, 1, 1, 4, 2, 67], []),
        "mse": (6, (2,), [28, 5, 8, 1, 4, 2, 1024], []),
        "g_total": (2, (), [], []),
        "l2_total": (3, (), [7], []),
        "adam_tick": (2, (), [0, 11], [0.9, 0.999]),
        "dropout_fwd": (1, (), [3, 5, 8, 1234, 1 << 23], [0.5]),
        "dropout_bwd": (2, (), [3, 5, 8], [0.5]),
        "lrelu_bwd": (2, (), [3, 5, 8], [0.3])}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def refused(lib, rc, *words):
    assert rc == ERR_INVALID, rc
    msg = lib.rsrgan_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)
    return msg


def ptrs_of(n, null_at=None, misalign_at=None):
    return (C.c_void_p * n)(*[None if i == null_at else P + 4096 * i + (4 if i == misalign_at else 0) for i in range(n)])


def update(lib, op, tensors=TENSORS, buf=BUF, partial=4, extra=None, src=(0, 64, 4224), null_at=None, misalign_at=None):
    n, _, ex = UPDATE[op]
    ex = list(ex if extra is None else extra)
    dims = [len(tensors), buf, partial] + (ex + [0, 0, 0])[:3] + [v for t in tensors for v in t] + (list(src) if op == "dw_reduce" else [])
    return lib.rsrgan_op_update(_lib.UPDATE_OPS.index(op), ptrs_of(n, null_at, misalign_at), (C.c_int64 * len(dims))(*dims), None, None)


def elem(lib, op, set=None, fl=None, null_at=None, misalign_at=None, null_fl=False, null_dims=False):
    n, _, dims, f = ELEM[op]
    dims = list(dims)
    for i, v in (set or {}).items():
        dims[i] = v
    f = list(f if fl is None else fl)
    return lib.rsrgan_op_step_elem(_lib.STEP_ELEM_OPS.index(op), ptrs_of(n, null_at, misalign_at),
                                   None if null_dims else (C.c_int64 * max(len(dims), 1))(*dims),
                                   None if null_fl else (C.c_float * max(len(f), 1))(*f), None)


def chunks(lib, tensors, out_ints=None):
    flat = [v for t in tensors for v in t]
    tt = (C.c_int64 * max(len(flat), 1))(*flat)
    nc = C.c_int32(-1)
    rc = lib.rsrgan_op_chunks(tt, len(tensors), None, 0, C.byref(nc))
    if rc != 0:
        return rc, None
    n = 3 * nc.value + 3 * len(tensors) if out_ints is None else out_ints
    out = (C.c_int32 * max(n, 1))()
    rc = lib.rsrgan_op_chunks(tt, len(tensors), out, n, C.byref(nc))
    return rc, (nc.value, list(out)[:n])


# ---------------------------------------------------------------------------------------------------------------- the chunk table
def test_chunk_table_against_own_chunking(lib):
    """tensor order, 4096-float chunks, a short tail chunk per tensor; the sizes of tests/test_gpu_update_ops.py"""
    sizes = [4, 4092, 4096, 4100, 3 * 4096 + 8, 257 * 4096 + 12, 40]
    tensors, off = [], 0
    for i, n in enumerate(sizes):
        tensors.append((off, n, i % 2))
        off += (n + 63) // 64 * 64
    rc, (nc, out) = chunks(lib, tensors)
    assert rc == 0
    want = {k: [] for k in ("tensor", "off", "len", "t_first", "t_count", "t_l2")}
    for i, (o, n, l2) in enumerate(tensors):
        want["t_first"].append(len(want["tensor"]))
        for c in range(0, n, 4096):
            want["tensor"].append(i); want["off"].append(o + c); want["len"].append(min(4096, n - c))
        want["t_count"].append(len(want["tensor"]) - want["t_first"][-1])
        want["t_l2"].append(l2)
    assert want["t_count"] == [1, 1, 1, 2, 4, 258, 1] and nc == 268
    assert out == sum((want[k] for k in ("tensor", "off", "len", "t_first", "t_count", "t_l2")), [])


def test_chunks_refusals(lib):
    refused(lib, lib.rsrgan_op_chunks(None, 1, None, 0, C.byref(C.c_int32())), "op_chunks", "null pointer (tensors)")
    refused(lib, lib.rsrgan_op_chunks((C.c_int64 * 3)(0, 4, 0), 1, None, 0, None), "null pointer (n_chunks)")
    refused(lib, chunks(lib, [])[0], "n_tensors = 0")
    refused(lib, chunks(lib, [(0, 4, 0)] * 4097)[0], "n_tensors = 4097")
    refused(lib, chunks(lib, [(2, 4, 0)])[0], "offset 2 of tensor 0", "multiple of 4")
    refused(lib, chunks(lib, [(0, 4, 0), (-4, 4, 0)])[0], "offset -4 of tensor 1")
    refused(lib, chunks(lib, [(0, 6, 0)])[0], "length 6 of tensor 0", "multiple of 4")
    refused(lib, chunks(lib, [(0, 0, 0)])[0], "length 0 of tensor 0")
    refused(lib, chunks(lib, [(0, 4, 2)])[0], "l2 flag 2")
    refused(lib, chunks(lib, TENSORS, out_ints=20)[0], "out of 20 ints below the table's 21")


# ---------------------------------------------------------------------------------------------------------------- rsrgan_op_update
@pytest.mark.parametrize("op", list(UPDATE))
def test_update_refusals_common(lib, op):
    n, opt, _ = UPDATE[op]
    names = {"sumsq": ["g", "partial"], "dw_reduce": ["ws", "g", "partial"], "l2": ["w", "g", "l2_scale", "partial"],
             "apply_sgd": ["w", "g", "ema", "partial", "dyn"], "apply_adam": ["w", "g", "m", "v", "ema", "partial", "dyn"]}[op]
    for i in range(n):
        if i not in opt:
            refused(lib, update(lib, op, null_at=i), "op_update", "null pointer (%s)" % names[i])
        if names[i] in ("w", "g", "m", "v", "ema", "ws"):
            refused(lib, update(lib, op, misalign_at=i), "%s not 16-byte aligned" % names[i])
    refused(lib, update(lib, op, tensors=[(0, 4, 1), (66, 40, 0)]), "offset 66 of tensor 1", "multiple of 4")
    refused(lib, update(lib, op, tensors=[(0, 4, 1), (64, 42, 0)]), "length 42 of tensor 1", "multiple of 4")
    refused(lib, update(lib, op, tensors=[(0, -4, 1)]), "length -4 of tensor 0")
    refused(lib, update(lib, op, tensors=[]), "n_tensors = 0")
    refused(lib, update(lib, op, buf=4260), "tensor 2 ends at 4264", "4260 floats")
    refused(lib, update(lib, op, buf=0), "buf_floats = 0")
    refused(lib, update(lib, op, partial=3), "partial of 3 floats below the table's 4 chunks")     # scratch too small
    assert lib.rsrgan_op_update(_lib.UPDATE_OPS.index(op), None, None, None, None) == ERR_INVALID
    assert "null table" in lib.rsrgan_last_error().decode()


def test_update_refusals_own(lib):
    for op in (-1, 5):
        refused(lib, lib.rsrgan_op_update(op, ptrs_of(2), (C.c_int64 * 9)(1, 4, 1, 0, 0, 0, 0, 4, 0), None, None), "op = %d" % op)
    refused(lib, update(lib, "dw_reduce", extra=(4286, 2, 2 * 4288)), "stride", "multiple of 4")
    refused(lib, update(lib, "dw_reduce", extra=(0, 2, 2 * 4288)), "stride = 0")
    refused(lib, update(lib, "dw_reduce", extra=(4288, 0, 2 * 4288)), "ntiles = 0")
    refused(lib, update(lib, "dw_reduce", extra=(4288, 65, 65 * 4288)), "ntiles = 65")
    refused(lib, update(lib, "dw_reduce", extra=(4288, 2, 2 * 4288 - 28)), "ws of 8548 floats below tensor 2's last record")
    refused(lib, update(lib, "dw_reduce", src=(0, 66, 4224)), "src 66 of tensor 1")
    refused(lib, update(lib, "dw_reduce", src=(0, -2, 4224)), "src -2 of tensor 1")
    refused(lib, update(lib, "dw_reduce", src=(0, 64, 4252)), "tensor 2 at src 4252 does not fit a record of stride 4288")
    refused(lib, update(lib, "apply_adam", extra=(10,)), "lrt_slot = 10")


# ---------------------------------------------------------------------------------------------------------------- rsrgan_op_step_elem
PTR_NAMES = {"lsgan": ["logits", "dlogits", "t_real", "t_fake", "loss3"],
             "dhead": ["top", "w", "b", "logits", "dlogits", "dout", "gw", "gb", "t_real", "t_fake", "loss3", "part"],
             "mse": ["y", "lab", "dy", "lambda", "loss", "scratch"], "g_total": ["l4", "lambda"], "l2_total": ["partial", "l2_scale", "out"],
             "adam_tick": ["dyn", "t"], "dropout_fwd": ["y"], "dropout_bwd": ["y", "d"], "lrelu_bwd": ["h", "d"]}


@pytest.mark.parametrize("op", list(ELEM))
def test_step_elem_null_pointers_and_tables(lib, op):
    n, opt, dims, fl = ELEM[op]
    for i in range(n):
        if i not in opt:
            refused(lib, elem(lib, op, null_at=i), "op_step_elem", "null pointer (%s)" % PTR_NAMES[op][i])
    if dims:
        refused(lib, elem(lib, op, null_dims=True), "null table (dims)")
    if fl:
        refused(lib, elem(lib, op, null_fl=True), "null table (fl")
    refused(lib, lib.rsrgan_op_step_elem(_lib.STEP_ELEM_OPS.index(op), None, None, None, None), "null table (ptrs)")


def test_step_elem_op_range(lib):
    for op in (-1, 9):
        refused(lib, lib.rsrgan_op_step_elem(op, ptrs_of(2), (C.c_int64 * 4)(), (C.c_float * 2)(), None), "op = %d" % op)


def bp_refusals(lib, op, i_rows, i_bp, i_bt, rows_name):
    """Bp > 0 with Bt > Bp (or < 1), and a row count Bp does not divide"""
    _, _, dims, _ = ELEM[op]
    refused(lib, elem(lib, op, set={i_bt: dims[i_bp] + 1}), "Bt = %d outside 1 .. Bp = %d" % (dims[i_bp] + 1, dims[i_bp]))
    refused(lib, elem(lib, op, set={i_bt: 0}), "Bt = 0 outside")
    refused(lib, elem(lib, op, set={i_bp: -1}), "Bp = -1")
    refused(lib, elem(lib, op, set={i_bp: 3, i_bt: 2}), "%s = %d is not divisible by Bp = 3" % (rows_name, dims[i_rows]))


def test_lsgan_refusals(lib):
    refused(lib, elem(lib, "lsgan", set={0: 0}), "T = 0")
    refused(lib, elem(lib, "lsgan", set={1: -8}), "Nd = -8")
    refused(lib, elem(lib, "lsgan", set={2: 9}), "n_real = 9 outside 0 .. Nd = 8")
    refused(lib, elem(lib, "lsgan", set={3: 0}), "leading dimension ldl")
    refused(lib, elem(lib, "lsgan", set={4: 2}), "clip_on = 2")
    bp_refusals(lib, "lsgan", 1, 5, 6, "Nd")
    refused(lib, elem(lib, "lsgan", set={2: 2}), "n_real = 2 is not divisible by Bp = 4")


def test_dhead_refusals(lib):
    refused(lib, elem(lib, "dhead", set={3: 38, 4: 40}), "dR = 38 is not a multiple of 4")
    refused(lib, elem(lib, "dhead", set={3: 64, 4: 64, 7: 64}), "dR = 64 above 60")
    refused(lib, elem(lib, "dhead", set={3: 0}), "dR = 0")
    refused(lib, elem(lib, "dhead", set={4: 36}), "leading dimension ldt = 36 below its row of 40")
    refused(lib, elem(lib, "dhead", set={4: 42}), "ldt = 42 is not a multiple of 4")
    refused(lib, elem(lib, "dhead", set={7: 36}), "leading dimension ldo")
    refused(lib, elem(lib, "dhead", set={7: 42}), "ldo = 42 is not a multiple of 4")
    refused(lib, elem(lib, "dhead", set={5: 0}), "leading dimension ldw")
    refused(lib, elem(lib, "dhead", set={6: 0}), "leading dimension ldl")
    refused(lib, elem(lib, "dhead", set={0: 0}), "T = 0")
    refused(lib, elem(lib, "dhead", set={2: 12}), "n_real = 12")
    refused(lib, elem(lib, "dhead", set={8: 2}), "want_grads = 2")
    refused(lib, elem(lib, "dhead", set={12: 66}), "part of 66 floats below")
    refused(lib, elem(lib, "dhead", set={0: 17, 12: 2 * 67}), "part of 134 floats below ceil(T x Nd / 64) x 67 = 201")
    refused(lib, elem(lib, "dhead", misalign_at=0), "top not 16-byte aligned")
    refused(lib, elem(lib, "dhead", misalign_at=5), "dout not 16-byte aligned")
    bp_refusals(lib, "dhead", 1, 10, 11, "Nd")
    # outputs that are switched off may be NULL; the ones switched on may not
    for i, flag in ((4, 8), (5, 8), (6, 9), (7, 9)):
        refused(lib, elem(lib, "dhead", null_at=i), "null pointer (%s)" % PTR_NAMES["dhead"][i])
        refused(lib, elem(lib, "dhead", null_at=i, set={flag: 0, 12: 0}), "part of 0 floats")       # past the pointer check


def test_mse_refusals(lib):
    refused(lib, elem(lib, "mse", set={0: 0}), "rows = 0")
    refused(lib, elem(lib, "mse", set={1: 0}), "D = 0")
    refused(lib, elem(lib, "mse", set={2: 4}), "leading dimension ld = 4 below its row of 5")
    refused(lib, elem(lib, "mse", set={3: 2}), "accumulate = 2")
    refused(lib, elem(lib, "mse", set={6: 1023}), "scratch of 1023 floats below launch_mse's 1024")
    bp_refusals(lib, "mse", 0, 4, 5, "rows")
    refused(lib, elem(lib, "mse", set={0: 26}), "rows = 26 is not divisible by Bp = 4")


def test_small_op_refusals(lib):
    refused(lib, elem(lib, "l2_total", set={0: 0}), "n = 0")
    refused(lib, elem(lib, "adam_tick", set={1: 12}), "slots (0, 12)")
    refused(lib, elem(lib, "adam_tick", set={0: 1}), "slots (1, 11)")
    refused(lib, elem(lib, "adam_tick", fl=[1.0, 0.999]), "beta1 = 1")
    for op in ("dropout_fwd", "dropout_bwd", "lrelu_bwd"):
        refused(lib, elem(lib, op, set={0: 0}), "rows = 0")
        refused(lib, elem(lib, op, set={1: 0}), "cols = 0")
        refused(lib, elem(lib, op, set={2: 4}), "leading dimension ld = 4 below its row of 5")
    for op in ("dropout_fwd", "dropout_bwd"):
        refused(lib, elem(lib, op, fl=[0.0]), "keep = 0 outside (0, 1]")
        refused(lib, elem(lib, op, fl=[1.5]), "keep = 1.5")
    refused(lib, elem(lib, "dropout_fwd", set={4: (1 << 24) + 1}), "thr = 16777217")
    refused(lib, elem(lib, "dropout_fwd", set={4: -1}), "thr = -1")
