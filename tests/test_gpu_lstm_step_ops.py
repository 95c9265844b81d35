"""The launch-per-phase LSTM step kernels (csrc/kernels.hip k_fwd_gates, k_fwd_proj, k_bwd_a2, k_bwd_b, k_bwd_bp + k_bwd_b_red), each
through the launcher the model calls (rsrgan_op_lstm_step), against the fp64 step references of tests/lstm_step_ref.py (pinned to the
oracle's cell and to torch.autograd in tests/test_lstm_step_ref.py).  The jobs -- inputs, padded buffer images, pointer groups -- are
tests/lstm_step_cases.py's.  Every case

  * asserts through rsrgan_op_lstm_step_last_plan WHICH instantiation ran and the grid it ran on (the launchers choose by shape);
  * runs twice from fresh buffers, bit-identical;
  * reads back EVERY buffer of every job: outside the region the phase is documented to write -- rows >= N, the padding columns of m_out /
    out / res_out / h / dx / dmst, dc of masked rows, dmt without a projection, a dx that n_begin >= I leaves alone, every input -- the bits
    are the ones the launch started from (outputs start as SENT, guard rows included; input rows >= N hold NaN, the input padding that
    meets only zero weights holds +-1e3).  k_bwd_a2 stores dmt as whole float4s up to ldm: that padding is compared with the zeros
    that went in with dmst / dout;
  * bounds every output by the project's rule (tests/update_ref.py): the kernel's error k <= max(4 p, 2 ulp), p = the error of the same
    formula in plain-order fp32, both against fp64 in elem_err's metric.

The floor of the outputs that pass through the device's expf / tanhf (gates, c_out, h and what the unprojected epilogue copies from h;
dz, dc): the ROCm installation was searched for a stated maximum ulp error of expf and tanhf -- the HIP headers, the device-library
headers, the installed documentation -- and none is stated there, so NO floor for the math library is assumed: those outputs are held
to 4 p, and tests/test_lstm_step_ref.py::test_small_k_jobs_keep_p_above_the_floor shows on the CPU that p of every short-product job
here stays above the rule's 2 ulp (the smallest: 3.4e-7 = 1.4 x 2^-22, c_out of (5, 9, 7, 12) at forget_bias 0), i.e. that the floor
is never what bounds them.  tests/lstm_step_cases.py says how the inputs keep p there without cancellation.  The sums and products alone (m_out, out, res_out of the projection, dmt, dx, dmst, the split-K results) keep the rule's
2-ulp floor.

Shapes are (N, I, P, H) with every leading dimension the next multiple of 4."""
import numpy as np
import pytest
import torch

from rsrgan_amd.ops import OpEntries
from tests import lstm_step_ref as R
from tests.lstm_step_cases import BwdAJob, BwdBJob, GatesJob, ProjJob, eight, gates_fb0, three
from tests.update_ref import bounded, dev, elem_err, host, twice

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
PREFIX = "lstm_step_ops"
JOBMAP_MAX = 768                               # csrc/kernels.h


@pytest.fixture(scope="module")
def eng():
    return OpEntries()


def r8(n):
    return (n + 7) & ~7


def weight_images(eng, job, d):
    """the fragment-tiled and transposed weight copies of a job, built once on the device by the (bit-tested) layout entry from the rows of
    Model::refresh_swizzles (tests/lstm_step_ref.py swizzle_rows)"""
    if not hasattr(job, "_img"):
        img = {}
        rows = R.swizzle_rows(getattr(job, "I", 0), job.P, job.H, has_proj="Wp" in job.bufs)
        for name, kind in job.images.items():
            if kind == "transpose":                     # WpT [P][ldH] = Wp [H][ldP] transposed, zero padding
                ldP, ldH = R.pad4(job.P), R.pad4(job.H)
                img[name] = torch.zeros(job.P * ldH, dtype=torch.float32, device=eng.device)
                eng.op_layout("transpose", [d["Wp"], img[name]], [ldP, ldH, job.H, job.P])
            else:
                src, row, floats = rows[kind]
                img[name] = torch.full((floats,), float("nan"), dtype=torch.float32, device=eng.device)
                eng.op_layout("swizzle_many", [d[src], img[name]], [1] + row)
        assert eng.device_status() == 0
        job._img = img
    return job._img


def check_job(case, j, job, res):
    N = job.N
    r64, r32 = job.ref(f64), job.ref(f32)
    written = {}
    for name, (buf, c0, c1, rows) in job.outs.items():
        init = job.bufs[buf]
        got = res["%d.%s" % (j, buf)].reshape(init.shape)
        mask = np.zeros(init.shape, bool)
        mask[:N, c0:c1] = True if rows is None else rows[:, None]
        written[buf] = written.get(buf, False) | mask
        sel = slice(None) if rows is None else rows
        g, w64, w32 = got[:N, c0:c1][sel], np.asarray(r64[name])[:, c0:c1][sel], np.asarray(r32[name])[:, c0:c1][sel]
        assert w64.dtype == f64 and w32.dtype == f32 and g.shape == w64.shape and g.size > 0, (case, name)
        assert np.all(np.isfinite(g)), (case, name, "a written element is not finite")
        bounded(PREFIX, case, name, elem_err([g], [w64]), elem_err([w32], [w64]))
    for buf, init in job.bufs.items():                   # everything else: the bits the launch started from
        got = res["%d.%s" % (j, buf)]
        a, b = np.ascontiguousarray(got).reshape(-1).view(np.uint8), np.ascontiguousarray(init).reshape(-1).view(np.uint8)
        assert a.shape == b.shape, (case, buf)
        diff = (a != b).reshape(-1, init.dtype.itemsize).any(axis=1).reshape(init.shape)
        if buf in written:
            diff &= ~written[buf]
        assert not diff.any(), "%s: %s changed outside its documented region at %s (%d elements)" % (case, buf, np.argwhere(diff)[0], diff.sum())


def launch(eng, op, jobs, case):
    plan = {}

    def once():
        ptrs, dims, devs = [], [len(jobs)], []
        for job in jobs:
            d = {k: dev(v, eng) for k, v in job.bufs.items()}
            named = dict(d, **weight_images(eng, job, d))
            ptrs += [None if n is None else named[n] for n in job.ptrs]
            dims += job.dims
            devs.append(d)
        fl = [jobs[0].forget_bias] if op == "fwd_gates" else [job.keep for job in jobs]
        if op == "bwd_b_splitk":                         # the partial tiles: NaN wherever the first kernel does not write
            n_ws = sum(16 * job.N * R.pad4(job.n_end - job.n_begin) for job in jobs)
            ws = torch.full((n_ws,), float("nan"), dtype=torch.float32, device=eng.device)
            ptrs.append(ws)
            dims.append(n_ws)
        eng.op_lstm_step(op, ptrs, dims, fl)
        plan.update(eng.op_lstm_step_last_plan())
        assert eng.device_status() == 0
        return {"%d.%s" % (j, k): host(t) for j, d in enumerate(devs) for k, t in d.items()}

    res = twice(once)
    for j, job in enumerate(jobs):
        check_job(case if len(jobs) == 1 else "%s job %d" % (case, j), j, job, res)
    print("%s %-40s plan %s" % (PREFIX, case, " ".join("%s=%s" % kv for kv in plan.items())))
    return plan


def tiles(job, form):
    """(column blocks, row blocks) of a job under the form that ran"""
    if job.op == "fwd_gates":
        return (job.H + 15) // 16, -(-job.N // (16 if form == "gates<18,1>" else 32))
    if job.op == "fwd_proj":
        return (job.P + 15) // 16, -(-job.N // 32)
    if job.op == "bwd_a":
        return (job.H + 31) // 32, -(-job.N // 32)
    return (job.n_end - job.n_begin + 15) // 16, -(-job.N // (16 if form == "bwd_b<8,8,8,1>" else 32))


def ungrouped_grid(jobs, form):
    return sum(r8(c) * r for c, r in (tiles(job, form) for job in jobs))


# ------------------------------------------------------------------------------------------------ single jobs: every form, its edges
SINGLE = [
    # forward phase 1
    ("fwd_gates", "x (5,9,7,12)", lambda: GatesJob(5, 9, 7, 12), "gates<18,1>"),
    ("fwd_gates", "x (5,9,7,12) forget_bias 0", gates_fb0, "gates<18,1>"),
    ("fwd_gates", "zx (17,-,16,20) nkb 1", lambda: GatesJob(17, 0, 16, 20, zx=True), "gates<18,1>"),                # the second K half is empty
    ("fwd_gates", "x (33,256,320,40) Ktot 576", lambda: GatesJob(33, 256, 320, 40), "gates<18,1>"),                 # 18 k-blocks per wave: the slice is full
    ("fwd_gates", "x (32,257,320,40) Ktot 580", lambda: GatesJob(32, 257, 320, 40), "gates<32,2>"),
    ("fwd_gates", "x (16,512,512,24) Ktot 1024", lambda: GatesJob(16, 512, 512, 24), "gates<32,2>"),                # 32 k-blocks per wave: the limit
    ("fwd_gates", "x (257,9,7,272) 153 blocks", lambda: GatesJob(257, 9, 7, 272), "gates<18,2>"),                   # ragged last row and cell block
    ("fwd_gates", "noproj (19,24,24,24) res", lambda: GatesJob(19, 24, 24, 24, noproj=True, res=True), "gates<18,1>"),
    ("fwd_gates", "noproj zx (16,-,512,512)", lambda: GatesJob(16, 0, 512, 512, zx=True, noproj=True), "gates<18,1>"),
    # forward phase 2
    ("fwd_proj", "(5,-,7,12)", lambda: ProjJob(5, 7, 12), "proj<4>"),
    ("fwd_proj", "(33,-,280,384) kb 24", lambda: ProjJob(33, 280, 384), "proj<4>"),
    ("fwd_proj", "(33,-,280,400) kb 25", lambda: ProjJob(33, 280, 400), "proj<8>"),
    ("fwd_proj", "(20,-,257,760) res", lambda: ProjJob(20, 257, 760, res=True), "proj<8>"),
    ("fwd_proj", "fc (37,-,40,280)", lambda: ProjJob(37, 40, 280, fc=True), "proj<4>"),
    ("fwd_proj", "fc (37,-,1,40)", lambda: ProjJob(37, 1, 40, fc=True), "proj<4>"),
    ("fwd_proj", "drop (5,-,7,12)", lambda: ProjJob(5, 7, 12, drop=True, res=True), "proj<4,drop>"),
    ("fwd_proj", "drop (33,-,40,400)", lambda: ProjJob(33, 40, 400, drop=True), "proj<8,drop>"),
    # backward phase A
    ("bwd_a", "(5,-,7,12)", lambda: BwdAJob(5, 7, 12), "bwd_a<4>"),
    ("bwd_a", "(33,-,64,40) nkb 4", lambda: BwdAJob(33, 64, 40), "bwd_a<4>"),
    ("bwd_a", "(33,-,65,40) nkb 5", lambda: BwdAJob(33, 65, 40), "bwd_a<18>"),
    ("bwd_a", "(33,-,288,48) nkb 18", lambda: BwdAJob(33, 288, 48), "bwd_a<18>"),
    ("bwd_a", "(33,-,289,48) nkb 19", lambda: BwdAJob(33, 289, 48), "bwd_a<24>"),
    ("bwd_a", "(16,-,384,760) nkb 24", lambda: BwdAJob(16, 384, 760), "bwd_a<24>"),                                  # the limit; H leaves a ragged 32-cell block
    ("bwd_a", "no dout (5,-,7,12)", lambda: BwdAJob(5, 7, 12, dout=False, seed=1), "bwd_a<4>"),
    ("bwd_a", "noproj (19,-,24,24)", lambda: BwdAJob(19, 24, 24, noproj=True), "bwd_a<4>"),
    ("bwd_a", "noproj (16,-,512,512)", lambda: BwdAJob(16, 512, 512, noproj=True), "bwd_a<24>"),
    ("bwd_a", "drop (33,-,65,40)", lambda: BwdAJob(33, 65, 40, drop=True), "bwd_a<18,drop>"),
    # backward phase B, one launch of tiles
    ("bwd_b", "dx (5,9,7,12)", lambda: BwdBJob(5, 9, 7, 12), "bwd_b<8,8,8,1>"),                                        # the first tile holds dx and dmst columns
    ("bwd_b", "dx += (5,9,7,12)", lambda: BwdBJob(5, 9, 7, 12, accumulate=True), "bwd_b<8,8,8,1>"),
    ("bwd_b", "rec (5,9,7,12) dx NULL", lambda: BwdBJob(5, 9, 7, 12, with_dx=False), "bwd_b<8,8,8,1>"),
    ("bwd_b", "rec (5,9,7,12) dx untouched", lambda: BwdBJob(5, 9, 7, 12, with_dx=False, dx_given=True, accumulate=True), "bwd_b<8,8,8,1>"),
    ("bwd_b", "dx (17,40,40,256) kb 64", lambda: BwdBJob(17, 40, 40, 256), "bwd_b<8,8,8,1>"),
    ("bwd_b", "dx (33,40,40,260) kb 65", lambda: BwdBJob(33, 40, 40, 260), "bwd_b<8,0,6>"),
    ("bwd_b", "row-major dx (19,9,7,12)", lambda: BwdBJob(19, 9, 7, 12, tiled=False), "bwd_b<8,8,8,1>"),
    ("bwd_b", "fc += (37,40,-,K 280)", lambda: BwdBJob(37, 40, 0, 0, fc=True, tiled=False, accumulate=True, H4=280), "bwd_b<8,8,8,1>"),
    ("bwd_b", "fc = (37,40,-,K 1044)", lambda: BwdBJob(37, 40, 0, 0, fc=True, tiled=False, H4=1044), "bwd_b<8,0,6>"),
]


@pytest.mark.parametrize("op,case,make,form", SINGLE, ids=["%s %s" % (c[0], c[1]) for c in SINGLE])
def test_single_job(eng, op, case, make, form):
    job = make()
    plan = launch(eng, op, [job], "%s %s" % (op, case))
    assert plan["form"] == form, plan
    assert plan["threads"] == (256 if form.startswith(("proj<4", "bwd_a")) else 512), plan
    assert plan["map_valid"] == 1 and plan["groups"] == 0 and plan["grid"] == ungrouped_grid([job], form), plan


# ------------------------------------------------------------------------------------------------ split-K phase B
SPLITK = [
    # case, job, KG, kpg: nkb = ceil(H4 / 16) k-blocks in KG slices of kpg; a workgroup's two K halves take ceil(kpg / 2) and the rest
    ("dx (5,9,7,12)", lambda: BwdBJob(5, 9, 7, 12), 1, 3),                              # nkb 3: one slice, halves of 2 and 1
    ("dx (17,9,7,32) kpg 1", lambda: BwdBJob(17, 9, 7, 32), 8, 1),                      # nkb 8: the second half of every workgroup is empty
    ("dx (17,9,7,80) short slice", lambda: BwdBJob(17, 9, 7, 80), 7, 3),                # nkb 20: six slices of 3 and one of 2
    ("dx += (65,25,40,12) ragged", lambda: BwdBJob(65, 25, 40, 12, accumulate=True), 1, 3),       # 65 rows, 65 columns, ldw 68
    ("rec (17,9,7,32)", lambda: BwdBJob(17, 9, 7, 32, with_dx=False), 8, 1),
    ("dx (64,257,280,760) generator", lambda: BwdBJob(64, 257, 280, 760), 8, 24),       # nkb 190: 24 per slice, 12 per wave -- the register limit; last slice 22
    ("row-major dx (17,9,7,80)", lambda: BwdBJob(17, 9, 7, 80, tiled=False), 7, 3),
    ("fc += (37,40,-,K 280)", lambda: BwdBJob(37, 40, 0, 0, fc=True, tiled=False, accumulate=True, H4=280), 6, 3),
]


@pytest.mark.parametrize("case,make,KG,kpg", SPLITK, ids=[c[0] for c in SPLITK])
def test_splitk(eng, case, make, KG, kpg):
    job = make()
    plan = launch(eng, "bwd_b_splitk", [job], "bwd_b_splitk %s" % case)
    assert plan["form"] == "splitk" and plan["threads"] == 512 and plan["map_valid"] == 1, plan
    assert (plan["KG"], plan["kpg"]) == (KG, kpg), plan
    ncols = job.n_end - job.n_begin
    assert plan["grid"] == r8(KG * -(-ncols // 64) * -(-job.N // 64)) and plan["grid2"] == r8(-(-job.N * ncols // 256)), plan
    assert plan["tiled"] == (1 if job.ptrs[2] else 0), plan


# ------------------------------------------------------------------------------------------------ several jobs in one launch
THREE_FORMS = {"fwd_gates": "gates<18,1>", "fwd_proj": "proj<4>", "bwd_a": "bwd_a<4>", "bwd_b": "bwd_b<8,8,8,1>"}


@pytest.mark.parametrize("op", list(THREE_FORMS))
def test_three_jobs_two_xcd_groups(eng, op):
    jobs = three(op)
    plan = launch(eng, op, jobs, "%s three jobs" % op)
    assert plan["form"] == THREE_FORMS[op] and plan["map_valid"] == 1, plan
    # the two heavy jobs run side by side on their own XCD slots from round 0, the light one after them on all eight: fewer rounds than
    # the contiguous layout, where every job spans all eight slots in turn
    assert plan["groups"] == 2 and plan["grid"] % 8 == 0 and plan["grid"] < ungrouped_grid(jobs, plan["form"]), plan


def test_three_jobs_splitk(eng):
    jobs = three("bwd_b_splitk")
    plan = launch(eng, "bwd_b_splitk", jobs, "bwd_b_splitk three jobs")
    assert plan["form"] == "splitk" and plan["map_valid"] == 1 and plan["groups"] == 2, plan


@pytest.mark.parametrize("op", ["fwd_gates", "fwd_proj", "bwd_a", "bwd_b", "bwd_b_splitk"])
def test_eight_jobs(eng, op):
    plan = launch(eng, op, eight(op), "%s eight jobs" % op)
    assert plan["map_valid"] == 1 and plan["grid"] % 8 == 0, plan


def test_gates_without_a_job_map(eng):
    """16 x 49 = 784 blocks > JOBMAP_MAX: the kernels find their job by walking the places"""
    job = GatesJob(1568, 0, 16, 256, zx=True)
    plan = launch(eng, "fwd_gates", [job], "fwd_gates zx (1568,-,16,256) no map")
    assert plan["form"] == "gates<18,2>" and plan["grid"] == 784 and plan["grid"] > JOBMAP_MAX and plan["map_valid"] == 0, plan


def test_two_jobs_without_a_job_map(eng):
    """... and picks the right one of two: a second, small job behind the 784 blocks"""
    jobs = [GatesJob(1568, 0, 16, 256, zx=True), GatesJob(33, 24, 24, 40, seed=4)]
    plan = launch(eng, "fwd_gates", jobs, "fwd_gates two jobs no map")
    assert plan["form"] == "gates<18,2>" and plan["grid"] == 784 + 8 * 2 and plan["map_valid"] == 0 and plan["groups"] == 0, plan
