"""rsrgan_op_lstm_step refuses every argument error BEFORE its first HIP call, naming it in rsrgan_last_error(): so the refusals run here,
without a device, on made-up pointers nobody dereferences (the pattern of tests/test_layout_op_args.py).  That a valid argument set of
every op gets past the checks is shown in a child process that sees no device: there the launch itself fails (RSRGAN_ERR_HIP)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from rsrgan_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_HIP = -1, -2
P0 = 0x10000
THR = 12582912                                  # floor(0.75 x 2^24)

# per op: pointer names of a job, the pointers a valid job leaves NULL, the dims record of a job, fl
NAMES = {"fwd_gates": ["x", "KxT", "m", "KhT", "Wsw", "zx", "bias", "wf", "wi", "wo", "c_prev", "c_out", "gates", "h", "len", "np_m_out", "np_out",
                       "np_res_in", "np_res_out"],
         "fwd_proj": ["h", "WpT", "WpT_sw", "m_prev", "m_out", "out", "res_in", "res_out", "len", "bias", "noise", "drop_ctr"],
         "bwd_a": ["dout", "dmst", "Wp", "Wp_sw", "dmt", "gates", "c_prev", "c_cur", "wf", "wi", "wo", "dc", "len", "drop_ctr"],
         "bwd_b": ["dz", "K", "Ksw", "dx", "dmst", "len"],
         "bwd_b_splitk": ["dz", "K", "Ksw", "dx", "dmst", "len"]}
VALID = {"fwd_gates": ((5, 15, 16, 17, 18), [5, 12, 12, 8, 12, 1], [1.0]),            # N, H, ldx, ldm, ldh, t
         "fwd_proj": ((), [5, 7, 12, 8, 8, 1, 3, 4, THR], [0.75]),                   # N, P, ldh, ldm, ldo, t, seed, tag, thr
         "bwd_a": ((), [5, 7, 12, 8, 1, 3, 4, THR], [0.75]),                         # N, P, H, ldm, t, seed, tag, thr
         "bwd_b": ((), [5, 9, 0, 16, 12, 8, 1, 48, 0], []),                          # N, I, n_begin, n_end, lddx, ldm, t, H4, dx_accumulate
         "bwd_b_splitk": ((), [5, 9, 0, 16, 12, 8, 1, 48, 0], [])}
REQUIRED = {"fwd_gates": ["m", "Wsw", "bias", "wf", "wi", "wo", "c_prev", "c_out", "gates", "h", "len"],
            "fwd_proj": ["h", "WpT", "m_out", "out"],
            "bwd_a": ["dmst", "dmt", "gates", "c_prev", "c_cur", "wf", "wi", "wo", "dc", "len"],
            "bwd_b": ["dz", "dx", "dmst"], "bwd_b_splitk": ["dz", "dx", "dmst", "ws"]}
ALIGN16 = {"fwd_gates": ["x", "m", "Wsw"], "fwd_proj": ["h", "WpT", "WpT_sw"], "bwd_a": ["dout", "dmst", "Wp_sw", "dmt"], "bwd_b": ["dz", "K", "Ksw"],
           "bwd_b_splitk": ["dz", "K", "Ksw"]}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def refused(lib, rc, *words):
    assert rc == ERR_INVALID, rc
    msg = lib.rsrgan_last_error().decode()
    assert "op_lstm_step" in msg, msg
    for w in words:
        assert w in msg, (w, msg)
    return msg


def call(lib, op, set=None, null=(), give=(), misalign=None, n=1, fl="valid", ws_floats=80, null_ptrs=False, null_dims=False, job=0):
    """n copies of the valid job; `set` (dims index -> value), `null` / `give` / `misalign` (pointer names) act on job `job`"""
    names, nulls, rec, f = NAMES[op], VALID[op][0], VALID[op][1], VALID[op][2]
    ptrs, dims = [], [n]
    for j in range(max(n, 1)):
        r = list(rec)
        for i, v in ((set or {}).items() if j == job else ()):
            r[i] = v
        dims += r
        for i, nm in enumerate(names):
            off = j == job
            isnull = (i in nulls and not (off and nm in give)) or (off and nm in null)
            ptrs.append(None if isnull else P0 + 4096 * (len(names) * j + i) + (4 if off and nm == misalign else 0))
    if op == "bwd_b_splitk":
        ptrs.append(None if "ws" in null else P0 + 4096 * 1000)
        dims.append(ws_floats)
    fv = (f * max(n, 1)) if fl == "valid" else fl
    return lib.rsrgan_op_lstm_step(_lib.LSTM_STEP_OPS.index(op), None if null_ptrs else (C.c_void_p * len(ptrs))(*ptrs),
                                   None if null_dims else (C.c_int64 * len(dims))(*dims),
                                   None if fv is None else (C.c_float * max(len(fv), 1))(*fv), None)


def test_op_names_cover_the_entry(lib):
    assert list(VALID) == list(_lib.LSTM_STEP_OPS) and len(_lib.LSTM_STEP_OPS) == 5
    assert len(_lib.LSTM_STEP_FORMS) == 17 and len(_lib.LSTM_STEP_PLAN_FIELDS) == 10
    for op in (-1, 5):
        refused(lib, lib.rsrgan_op_lstm_step(op, (C.c_void_p * 19)(), (C.c_int64 * 8)(1), (C.c_float * 1)(), None), "op = %d" % op)
    assert lib.rsrgan_op_lstm_step_last_plan(None) == ERR_INVALID


@pytest.mark.parametrize("op", list(VALID))
def test_tables_job_count_and_required_pointers(lib, op):
    refused(lib, call(lib, op, null_ptrs=True), "null table")
    refused(lib, call(lib, op, null_dims=True), "null table")
    refused(lib, call(lib, op, n=0), "n = 0 jobs outside 1 .. 8")
    refused(lib, call(lib, op, n=9), "n = 9 jobs outside 1 .. 8")
    for nm in REQUIRED[op]:
        refused(lib, call(lib, op, null=(nm,)), "null pointer (%s" % nm)
    for nm in REQUIRED[op]:                                   # ... of the job that has the fault, named
        if nm != "ws":
            refused(lib, call(lib, op, null=(nm,), n=3, job=2), "null pointer (%s of job 2" % nm)
    for nm in ALIGN16[op]:
        refused(lib, call(lib, op, misalign=nm), "%s of job 0 not 16-byte aligned" % nm)
    for i, nm in ((0, "N"), (1, {"fwd_gates": "H", "fwd_proj": "P", "bwd_a": "P"}.get(op))):
        if nm:
            refused(lib, call(lib, op, set={i: 0}), "%s of job 0 = 0 outside 1" % nm)
    ti = {"fwd_gates": 5, "fwd_proj": 5, "bwd_a": 4}.get(op, 6)
    refused(lib, call(lib, op, set={ti: -1}), "t of job 0 = -1 outside 0")


def test_a_valid_call_of_every_op_gets_past_the_checks():
    """in a child that sees no device: every op, with one job and with MAXJ jobs, returns RSRGAN_ERR_HIP from its failed launch"""
    code = ("import ctypes as C, json, sys\n"
            "sys.path.insert(0, %r)\n"
            "from rsrgan_amd import _lib\n"
            "import tests.test_lstm_step_op_args as A\n"
            "lib = _lib.load()\n"
            "hip = C.CDLL('libamdhip64.so')\n"
            "n = C.c_int(-1)\n"
            "rc = hip.hipGetDeviceCount(C.byref(n))\n"
            "if rc == 0 and n.value > 0:\n"
            "    print(json.dumps({'devices': n.value})); sys.exit(0)\n"
            "print(json.dumps({'devices': 0, 'rc': {op: [A.call(lib, op), A.call(lib, op, n=8, ws_floats=640)] for op in A.VALID}}))\n") % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["devices"] == 0, "the child still sees %d device(s)" % res["devices"]
    assert res["rc"] == {op: [ERR_HIP, ERR_HIP] for op in VALID}


def test_fwd_gates_rules(lib):
    op = "fwd_gates"
    refused(lib, call(lib, op, fl=None), "null table (fl: forget_bias)")
    refused(lib, call(lib, op, null=("x",)), "null pointer (x and zx of job 0)")
    refused(lib, call(lib, op, give=("zx",)), "x and zx of job 0 both given")
    refused(lib, call(lib, op, set={2: 10}), "ldx of job 0 = 10 is not a multiple of 4")
    refused(lib, call(lib, op, set={2: 0}), "leading dimension ldx of job 0 = 0 below its row of 4")
    refused(lib, call(lib, op, set={3: 6}), "ldm of job 0 = 6 is not a multiple of 4")
    refused(lib, call(lib, op, set={4: 11}), "leading dimension ldh of job 0 = 11 below its row of 12")
    refused(lib, call(lib, op, set={2: 516, 3: 512}), "ldx + ldm of job 0 = 1028 above 1024")
    refused(lib, call(lib, op, null=("x",), give=("zx",), set={3: 1028}), "ldx + ldm of job 0 = 1028 above 1024")      # (zx: ldm alone)
    refused(lib, call(lib, op, give=("np_out",)), "np_out, np_res_in or np_res_out of job 0 given without np_m_out")
    refused(lib, call(lib, op, give=("np_m_out",)), "leading dimension ldm of job 0 = 8 below its row of 12 (m = h without a projection)")
    refused(lib, call(lib, op, give=("np_m_out", "np_res_out"), set={3: 12}), "null pointer (np_res_in of job 0)")


def test_fwd_proj_rules(lib):
    op = "fwd_proj"
    refused(lib, call(lib, op, set={2: 14}), "ldh of job 0 = 14 is not a multiple of 4")
    refused(lib, call(lib, op, set={3: 6}), "leading dimension ldm of job 0 = 6 below its row of 7")
    refused(lib, call(lib, op, set={4: 6}), "leading dimension ldo of job 0 = 6 below its row of 7")
    refused(lib, call(lib, op, null=("m_prev",)), "null pointer (m_prev of job 0): masked rows keep m_prev")
    refused(lib, call(lib, op, null=("res_in",)), "null pointer (res_in of job 0)")
    refused(lib, call(lib, op, null=("len", "m_prev"), set={0: 85}), "N of job 0 = 85 above P x ldh = 84 without len")
    refused(lib, call(lib, op, fl=None), "null table (fl: keep")
    refused(lib, call(lib, op, fl=[0.0]), "keep of job 0 = 0 outside (0, 1]")
    refused(lib, call(lib, op, fl=[1.5]), "keep of job 0 = 1.5 outside (0, 1]")
    refused(lib, call(lib, op, set={8: (1 << 24) + 1}), "thr of job 0 = 16777217 outside 0 .. 2^24")
    refused(lib, call(lib, op, set={8: -1}), "thr of job 0 = -1")


def test_bwd_a_rules(lib):
    op = "bwd_a"
    refused(lib, call(lib, op, set={3: 10}), "ldm of job 0 = 10 is not a multiple of 4")
    refused(lib, call(lib, op, set={3: 4}), "leading dimension ldm of job 0 = 4 below its row of 7")
    refused(lib, call(lib, op, null=("Wp_sw",)), "null pointer (Wp_sw of job 0)")
    refused(lib, call(lib, op, null=("Wp",)), "null pointer (Wp of job 0)")
    refused(lib, call(lib, op, set={1: 385, 3: 388}), "ldm of job 0 = 388 above 384 with a projection")
    refused(lib, call(lib, op, null=("Wp", "Wp_sw")), "P of job 0 = 7 is not H = 12 without a projection")
    refused(lib, call(lib, op, null=("Wp", "Wp_sw", "dmt", "dmst"), set={1: 512, 2: 512, 3: 512}), "null pointer (dmst of job 0)")      # (no 384 limit, no dmt)
    refused(lib, call(lib, op, fl=[-0.5]), "keep of job 0 = -0.5 outside (0, 1]")
    refused(lib, call(lib, op, set={7: 1 << 25}), "thr of job 0")


@pytest.mark.parametrize("op", ["bwd_b", "bwd_b_splitk"])
def test_bwd_b_rules(lib, op):
    refused(lib, call(lib, op, set={7: 50}), "H4 of job 0 = 50 is not a multiple of 4")
    refused(lib, call(lib, op, set={7: 0}), "leading dimension H4 of job 0 = 0 below its row of 4")
    refused(lib, call(lib, op, set={3: 0}), "n_end of job 0 = 0 not above n_begin = 0")
    refused(lib, call(lib, op, set={2: -1}), "n_begin of job 0 = -1 outside 0")
    refused(lib, call(lib, op, set={1: -1}), "I of job 0 = -1 outside 0")
    refused(lib, call(lib, op, null=("K", "Ksw")), "null pointer (K and Ksw of job 0)")
    refused(lib, call(lib, op, set={4: 8}), "leading dimension lddx of job 0 = 8 below its row of 9")
    refused(lib, call(lib, op, set={5: 4}), "leading dimension ldm of job 0 = 4 below its row of 7")
    refused(lib, call(lib, op, set={8: 2}), "dx_accumulate of job 0 = 2 is neither 0 nor 1")
    # dx belongs to n_begin < I alone, dmst to n_end > I alone
    refused(lib, call(lib, op, null=("dx", "dz"), set={2: 9}), "null pointer (dz of job 0)")
    refused(lib, call(lib, op, null=("dmst", "dz"), set={3: 9}), "null pointer (dz of job 0)")


def test_splitk_rules(lib):
    op = "bwd_b_splitk"
    refused(lib, call(lib, op, ws_floats=79), "ws of 79 floats below the plan's need of 80")
    refused(lib, call(lib, op, ws_floats=-1), "ws of -1 floats")
    # three equal jobs own XCD groups of 3, 3 and 2 slots, and KG follows the slots: (3 + 3 + 2) x 5 x 16 floats
    refused(lib, call(lib, op, n=3, ws_floats=639), "below the plan's need of 640")
    # 385 k-blocks: KG is held to the 16 partials of k_bwd_b_red, so kpg = 25 and a wave's half of it is 13 k-blocks
    refused(lib, call(lib, op, set={7: 6160}, ws_floats=1 << 30), "kpg of job 0 = 25", "at most 12 k-blocks")
    refused(lib, call(lib, op, set={7: 6160}, ws_floats=1 << 30, n=2, job=1), "kpg of job 1 = 25")
