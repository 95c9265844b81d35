"""rsrgan_op_layout refuses every argument error BEFORE its first HIP call, naming it in rsrgan_last_error(): so the refusals run here,
without a device.  The pointers are made-up addresses: a refused call never reads them.  That a valid argument set of every op gets past
the checks is shown in a child process that sees no device: there the launch itself fails (RSRGAN_ERR_HIP), not the checks
(RSRGAN_ERR_INVALID)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from rsrgan_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_HIP = -1, -2
P = 0x10000                                    # a non-null, 16-byte aligned "device pointer" nobody dereferences

SW_GATES = [80, 4, 20, 0, 0, 0, 7, 12, 8, 8, 2]          # ld, gates, H, C, c0, K1, I, P, kx, nct, nkb
SW_ROWS = [80, 0, 0, 19, 0, 80, 0, 0, 0, 2, 5]
# valid arguments of every op: (number of pointers, pointers that may be NULL, dims, fl)
VALID = {"pack_tm": (2, (), [3, 5, 257, 260], []),
         "unpack_bm": (2, (), [4, 5, 257, 260, 2], []),
         "stage_inputs": (12, tuple(range(12)), [4, 5, 3, 257, 260, 40, 48, 1, 3, 300, 7], []),
         "build_d_input": (5, (2, 3), [3, 4, 40, 48, 1], []),
         "add_noise_rows": (3, (1,), [3, 4, 40, 48, 8, 5], []),
         "transpose": (2, (), [68, 38, 33, 65], []),
         "transpose_many": (4, (), [2, 68, 38, 33, 65, 4, 6, 1, 1], []),
         "swizzle_many": (4, (), [2] + SW_GATES + SW_ROWS, []),
         "im2col": (2, (), [80, 4, 4, 4, 5, 4, 3, 52, 40], []),
         "col2im": (2, (), [52, 4, 4, 5, 4, 3, 8, 40], []),
         "expand_c4": (2, (), [23, 20, 3], []),
         "gstate": (6, (1, 5), [2, 57, 3, 0, 2, 20, 12, 16, 0, 20, 0, 0, 32], []),
         "window_len": (2, (), [5, 3, 1000], []),
         "zero_many": (2, (), [2, 255, 8193], []),
         "fill": (1, (), [257], [1.5]),
         "build_joint": (3, (), [52, 3, 44, 40, 40, 88, 5, 5], []),
         "slice_cols": (2, (), [88, 44, 48, 5, 40], []),
         "pad_copy": (2, (), [5, 7, 8, 1], []),
         "copy_f": (2, (), [300], [])}
PTR_NAMES = {"pack_tm": ["src", "dst"], "unpack_bm": ["src", "dst"], "build_d_input": ["lab", "y", "nr", "nf", "xd"],
             "add_noise_rows": ["src", "noise", "dst"], "transpose": ["src", "dst"],
             "transpose_many": ["src of job 0", "dst of job 0", "src of job 1", "dst of job 1"],
             "swizzle_many": ["src of job 0", "dst of job 0", "src of job 1", "dst of job 1"], "im2col": ["src", "col"], "col2im": ["dcol", "dst"],
             "expand_c4": ["src", "dst"], "gstate": ["state", "mask", "c of job 0", "mst of job 0", "c of job 1", "mst of job 1"],
             "window_len": ["len", "dst"], "zero_many": ["p of job 0", "p of job 1"], "fill": ["p"], "build_joint": ["x", "tail", "joint"],
             "slice_cols": ["src", "dst"], "pad_copy": ["dense", "padded"], "copy_f": ["src", "dst"]}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def refused(lib, rc, *words):
    assert rc == ERR_INVALID, rc
    msg = lib.rsrgan_last_error().decode()
    assert "op_layout" in msg, msg
    for w in words:
        assert w in msg, (w, msg)
    return msg


def ptrs_of(n, null_at=None, misalign_at=None):
    """null_at: an index or a tuple of them"""
    nulls = null_at if isinstance(null_at, tuple) else (null_at,)
    return (C.c_void_p * n)(*[None if i in nulls else P + 4096 * i + (4 if i == misalign_at else 0) for i in range(n)])


def call(lib, op, set=None, dims=None, fl=None, null_at=None, misalign_at=None, null_fl=False, null_dims=False, null_ptrs=False):
    n, _, dm, f = VALID[op]
    dm = list(dm if dims is None else dims)
    for i, v in (set or {}).items():
        dm[i] = v
    f = list(f if fl is None else fl)
    return lib.rsrgan_op_layout(_lib.LAYOUT_OPS.index(op), None if null_ptrs else ptrs_of(n, null_at, misalign_at),
                                None if null_dims else (C.c_int64 * max(len(dm), 1))(*dm),
                                None if null_fl else (C.c_float * max(len(f), 1))(*f), None)


def test_op_names_cover_the_entry(lib):
    assert list(VALID) == list(_lib.LAYOUT_OPS) and len(_lib.LAYOUT_OPS) == 19
    for op in (-1, 19):
        refused(lib, lib.rsrgan_op_layout(op, ptrs_of(2), (C.c_int64 * 4)(), (C.c_float * 1)(), None), "op = %d" % op)


@pytest.mark.parametrize("op", list(VALID))
def test_null_tables_and_required_pointers(lib, op):
    n, opt, _, fl = VALID[op]
    refused(lib, call(lib, op, null_ptrs=True), "null table")
    refused(lib, call(lib, op, null_dims=True), "null table")
    if fl:
        refused(lib, call(lib, op, null_fl=True), "null table (fl")
    for i in range(n):
        if i not in opt:
            refused(lib, call(lib, op, null_at=i), "null pointer (%s)" % PTR_NAMES[op][i])


def test_a_valid_call_of_every_op_gets_past_the_checks():
    """in a child that sees no device (and says so before it calls anything): every op returns RSRGAN_ERR_HIP from its failed launch"""
    code = ("import ctypes as C, json, sys\n"
            "sys.path.insert(0, %r)\n"
            "from rsrgan_amd import _lib\n"
            "import tests.test_layout_op_args as A\n"
            "lib = _lib.load()\n"
            "hip = C.CDLL('libamdhip64.so')\n"
            "n = C.c_int(-1)\n"
            "rc = hip.hipGetDeviceCount(C.byref(n))\n"
            "if rc == 0 and n.value > 0:\n"
            "    print(json.dumps({'devices': n.value})); sys.exit(0)\n"
            "print(json.dumps({'devices': 0, 'rc': {op: A.call(lib, op) for op in A.VALID}}))\n") % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["devices"] == 0, "the child still sees %d device(s)" % res["devices"]
    assert res["rc"] == {op: ERR_HIP for op in VALID}


def test_extents_below_one(lib):
    for op, i, name in (("pack_tm", 0, "B"), ("pack_tm", 1, "T"), ("pack_tm", 2, "D"), ("unpack_bm", 1, "T"), ("stage_inputs", 0, "B"),
                        ("stage_inputs", 3, "D of job 0"), ("stage_inputs", 9, "n of job 2"), ("build_d_input", 2, "D"), ("add_noise_rows", 4, "Ns"),
                        ("transpose", 2, "R"), ("transpose", 3, "C"), ("transpose_many", 7, "R of job 1"), ("swizzle_many", 10, "nct of job 0"),
                        ("swizzle_many", 22, "nkb of job 1"), ("swizzle_many", 3, "H of job 0"), ("swizzle_many", 15, "C of job 1"),
                        ("swizzle_many", 17, "K1 of job 1"), ("im2col", 2, "C"), ("im2col", 5, "kh"), ("im2col", 8, "M"), ("col2im", 2, "S"),
                        ("col2im", 5, "kw"), ("expand_c4", 1, "n"), ("expand_c4", 2, "rows"), ("gstate", 1, "SF"), ("gstate", 5, "H of job 0"),
                        ("zero_many", 2, "len of job 1"), ("fill", 0, "n"), ("build_joint", 4, "Dt"), ("build_joint", 7, "R"), ("slice_cols", 3, "R"),
                        ("slice_cols", 4, "C"), ("pad_copy", 0, "rows"), ("pad_copy", 1, "cols"), ("copy_f", 0, "n")):
        refused(lib, call(lib, op, set={i: 0}), "%s = 0 outside 1" % name)
    for op, i, name in (("add_noise_rows", 5, "row0"), ("gstate", 2, "rows"), ("gstate", 4, "slot"), ("window_len", 0, "n"), ("window_len", 1, "t0"),
                        ("window_len", 2, "Tw"), ("build_joint", 1, "off"), ("build_joint", 2, "dim"), ("build_joint", 6, "row0"), ("slice_cols", 1, "off"),
                        ("swizzle_many", 9, "kx of job 0"), ("swizzle_many", 7, "I of job 0"), ("swizzle_many", 16, "c0 of job 1")):
        refused(lib, call(lib, op, set={i: -1}), "%s = -1 outside 0" % name)
    refused(lib, call(lib, "swizzle_many", set={7: 0, 8: 0}), "I + P = 0 source rows of job 0")


def test_leading_dimensions_below_the_width(lib):
    for op, i, name, ld, need in (("pack_tm", 3, "ld", 256, 257), ("unpack_bm", 3, "ld", 256, 257), ("stage_inputs", 4, "ld of job 0", 256, 257),
                                  ("stage_inputs", 6, "ld of job 1", 39, 40), ("build_d_input", 3, "ld", 39, 40), ("add_noise_rows", 3, "ld", 39, 40),
                                  ("transpose", 0, "lds", 64, 65), ("transpose", 1, "ldd", 32, 33), ("transpose_many", 1, "lds of job 0", 64, 65),
                                  ("transpose_many", 6, "ldd of job 1", 0, 1), ("swizzle_many", 1, "ld of job 0", 79, 80),
                                  ("swizzle_many", 12, "ld of job 1", 79, 80), ("im2col", 1, "ldc", 3, 4), ("im2col", 7, "ldk", 47, 48),
                                  ("im2col", 0, "row_stride", 76, 80), ("col2im", 0, "ldk", 44, 48), ("col2im", 6, "ldc", 0, 4),
                                  ("expand_c4", 0, "ld_src", 19, 20), ("gstate", 7, "ldP of job 0", 11, 12), ("build_joint", 0, "ldx", 46, 47),
                                  ("build_joint", 3, "ldt", 39, 40), ("build_joint", 5, "ldj", 83, 84), ("slice_cols", 0, "lds", 83, 84),
                                  ("slice_cols", 2, "ldd", 39, 40), ("pad_copy", 2, "ld", 6, 7)):
        refused(lib, call(lib, op, set={i: ld}), "leading dimension %s = %d below its row of %d" % (name, ld, need))


def test_row_windows(lib):
    refused(lib, call(lib, "unpack_bm", set={4: 5}), "Bt = 5 outside 0 (all rows) .. B = 4")
    refused(lib, call(lib, "unpack_bm", set={4: -1}), "Bt = -1")
    refused(lib, call(lib, "stage_inputs", set={2: 5}), "Bt = 5 outside 0 (all rows) .. B = 4")
    refused(lib, call(lib, "add_noise_rows", set={5: 6}), "rows [row0 = 6, row0 + B = 9) outside Ns = 8")
    refused(lib, call(lib, "build_d_input", set={4: 2}), "with_real = 2")
    refused(lib, call(lib, "pad_copy", set={3: 2}), "to_padded = 2")
    # lab belongs to with_real alone; x to dim > 0 alone
    refused(lib, call(lib, "build_d_input", null_at=0), "null pointer (lab)")
    refused(lib, call(lib, "build_d_input", null_at=(0, 1), set={4: 0}), "null pointer (y)")          # (lab itself was accepted)
    refused(lib, call(lib, "build_joint", null_at=0), "null pointer (x)")
    refused(lib, call(lib, "build_joint", null_at=(0, 1), set={2: 0}), "null pointer (tail)")


def test_list_lengths(lib):
    refused(lib, call(lib, "transpose_many", set={0: 0}), "n = 0 jobs outside the list (1 .. 16)")
    refused(lib, call(lib, "transpose_many", set={0: 17}), "n = 17 jobs outside the list (1 .. 16)")
    refused(lib, call(lib, "swizzle_many", set={0: 0}), "n = 0 jobs outside the list (1 .. 24)")
    refused(lib, call(lib, "swizzle_many", set={0: 25}), "n = 25 jobs outside the list (1 .. 24)")
    refused(lib, call(lib, "zero_many", set={0: 0}), "n = 0 buffers outside the list (1 .. 32)")
    refused(lib, call(lib, "zero_many", set={0: 33}), "n = 33 buffers outside the list (1 .. 32)")
    refused(lib, call(lib, "gstate", set={0: 0}), "nl = 0 layers outside 1 .. 4")
    refused(lib, call(lib, "gstate", set={0: 5}), "nl = 5 layers outside 1 .. 4")


def test_float4_conditions(lib):
    # col2im: ldc, ldk and C multiples of 4, 16-byte pointers
    refused(lib, call(lib, "col2im", set={6: 6}), "ldc = 6 is not a multiple of 4")
    refused(lib, call(lib, "col2im", set={0: 50}), "ldk = 50 is not a multiple of 4")
    refused(lib, call(lib, "col2im", set={1: 3}), "C = 3 is not a multiple of 4")
    refused(lib, call(lib, "col2im", misalign_at=0), "dcol not 16-byte aligned")
    refused(lib, call(lib, "col2im", misalign_at=1), "dst not 16-byte aligned")
    # im2col: the float4 form whenever C % 4 == 0 and ldc % 4 == 0
    refused(lib, call(lib, "im2col", misalign_at=0), "src not 16-byte aligned")
    refused(lib, call(lib, "im2col", misalign_at=1), "col not 16-byte aligned")
    refused(lib, call(lib, "im2col", set={0: 82}), "row_stride = 82 is not a multiple of 4")
    refused(lib, call(lib, "im2col", set={7: 50}), "ldk = 50 is not a multiple of 4")
    refused(lib, call(lib, "im2col", set={7: 44}), "leading dimension ldk = 44 below its row of 48")
    refused(lib, call(lib, "im2col", set={8: 41}), "M = 41 positions are no whole frames of S x W = 20")
    refused(lib, call(lib, "col2im", set={7: 39}), "M = 39 positions are no whole frames")
    # swizzle_many and expand_c4 store float4
    refused(lib, call(lib, "swizzle_many", misalign_at=1), "dst of job 0 not 16-byte aligned")
    refused(lib, call(lib, "swizzle_many", misalign_at=3), "dst of job 1 not 16-byte aligned")
    refused(lib, call(lib, "expand_c4", misalign_at=1), "dst not 16-byte aligned")


def test_scalar_im2col_takes_any_alignment():
    """C = 3, ldc = 3: launch_im2col's scalar form; a 4-byte aligned pointer, an odd row_stride and ldk are no errors (the call gets as
    far as its size checks)"""
    lib = _lib.load()
    dims = [63, 3, 3, 4, 5, 4, 3, 37, 0]
    rc = lib.rsrgan_op_layout(_lib.LAYOUT_OPS.index("im2col"), ptrs_of(2, misalign_at=0), (C.c_int64 * 9)(*dims), None, None)
    refused(lib, rc, "M = 0")


def test_gstate_and_swizzle_rules(lib):
    refused(lib, call(lib, "gstate", set={3: 3}), "dir = 3 outside 0")
    refused(lib, call(lib, "gstate", set={3: -1}), "dir = -1 outside 0")
    refused(lib, call(lib, "gstate", set={12: 38}), "layer 1 at offset 38 with H + P = 20 does not fit SF = 57")
    refused(lib, call(lib, "gstate", set={8: -4}), "layer 0 at offset -4")
    refused(lib, call(lib, "gstate", null_at=3), "null pointer (mst of job 0)")
    refused(lib, call(lib, "gstate", null_at=(2, 3, 4), set={3: 2, 1: 1 << 30, 2: 65535}), "rows x SF above")      # dir 2 needs no layer buffers
    refused(lib, call(lib, "swizzle_many", set={2: 5}), "gates = 5 of job 0 outside 0")
    refused(lib, call(lib, "swizzle_many", set={10: 7}), "nct = 7 of job 0 below gates x ceil(H / 16) = 8", "must cover the source")
    refused(lib, call(lib, "swizzle_many", set={2: 1, 1: 20, 10: 1}), "nct = 1 of job 0 below gates x ceil(H / 16) = 2")
