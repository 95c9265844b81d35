"""The weight-gradient tail, kernel by kernel: the stream-K GEMMs (k_gemm, k_gemm_s, k_gemm_fixup) in every tile form and plan, the
batched launches (launch_gemm_batch, launch_gemm16_batch), the window-view row maps and the column-sum kernels, each through the host
launch function the model calls (the rsrgan_op_* test entries) against torch fp64 on the CPU computed from the same fp32-rounded
inputs.  Every case asserts its numbers first and the plan that ran (rsrgan_op_gemm_last_plan) second, so a plan failure says the
arithmetic was right.

GEMM cases: B carries a column ramp (a transposed write cannot pass); C is pre-filled with a sentinel and its padding columns
[N, ldc) and a guard band of rows behind M must come back bit-unchanged; the operands' columns beyond their zero padding are NaN (a read
past the operand poisons the result); the launch runs twice and must give bit-identical output (gemm.hip promises a fixed summation
order); the accumulate pass runs after the plain one.  Bounds: max |err| / max(|ref|_max, 1) < 2e-5, and < 4e-5 after accumulate --
what tests/test_gpu_gemm.py holds K = 20000 to; a dropped 32-deep k-tile at K = 2048 is ~3e-2 on that scale.

Column sums: the bound is 4 x the error of the same sums accumulated in fp32 in plain row order on the CPU (both against fp64, same
metric); the factor covers summation-order differences only.  Each case prints both errors."""
import pytest
import torch

from rsrgan_amd._lib import GEMM_FORMS

pytestmark = pytest.mark.gpu

SENT = 7.0
GUARD = 3                      # sentinel rows behind M
TOL, TOL_ACC = 2e-5, 4e-5
COVERED = set()                # (kernel class, BM, BN, kind of plan) of every plan a passing case asserted
LAYOUTS = [(True, False), (True, True), (False, False), (False, True)]


@pytest.fixture(scope="module")
def eng():
    from rsrgan_amd.ops import OpEntries
    return OpEntries()


def pad4(n):
    return (n + 3) // 4 * 4


def gen(*seed):
    s = 0
    for v in seed:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator(device="cpu").manual_seed(s)


def relerr(got, ref, scale=None):
    return (got - ref).abs().max().item() / max((ref if scale is None else scale).abs().max().item(), 1.0)


def operand(mat, dev, extra=4):
    """[rows][pad4(cols) + extra] device buffer holding the fp32 matrix: zeros up to pad4(cols) (the kernels' contract), NaN beyond"""
    rows, cols = mat.shape
    buf = torch.full((rows, pad4(cols) + extra), float("nan"), dtype=torch.float32)
    buf[:, :pad4(cols)] = 0.0
    buf[:, :cols] = mat
    return buf.to(dev)


def make_problem(M, N, K, seed, with_bias):
    g = gen(M, N, K, seed)
    A = torch.randn(M, K, generator=g, dtype=torch.float32)
    B = (torch.randn(K, N, generator=g, dtype=torch.float32) + torch.arange(N, dtype=torch.float32)[None, :] * 0.01)
    bias = torch.randn(N, generator=g, dtype=torch.float32) if with_bias else None
    prod = A.double() @ B.double()
    ref = prod
    if with_bias:
        ref = prod + bias.double()
        ref = torch.maximum(ref, 0.3 * ref)
    return A, B, bias, prod, ref


def new_c(M, N, dev):
    return torch.full((M + GUARD, pad4(N) + 4), SENT, dtype=torch.float32, device=dev)


def check_c(C, M, N, ref, tol, scale=None):
    torch.cuda.synchronize()
    err = relerr(C[:M, :N].cpu().double(), ref, scale)
    assert err < tol, err
    assert bool(torch.all(C[:M, N:] == SENT)), "padding columns [N, ldc) written"
    assert bool(torch.all(C[M:] == SENT)), "rows behind M written"
    return err


def device_operands(A, B, akc, bkc, M1, dev):
    """A: [M][K] if akc else [K][M] (split at row M1 of A = column M1 of the stored matrix into two buffers of different ld)"""
    Ad = A2d = None
    if akc:
        Ad = operand(A, dev)
    elif M1:
        Ad = operand(A[:M1].t(), dev, extra=4)
        A2d = operand(A[M1:].t(), dev, extra=12)                       # lda2 != lda
        assert Ad.stride(0) != A2d.stride(0)
    else:
        Ad = operand(A.t(), dev)
    Bd = operand(B.t(), dev) if bkc else operand(B, dev)
    return Ad, A2d, Bd


def run_gemm(eng, M, N, K, akc, bkc, M1=0, workers=0, force=-1, seed=0, with_bias=True, problem=None):
    """plain launch twice (bit-identical), then accumulate; returns the plan of the plain launch"""
    dev = eng.device
    A, B, bias, prod, ref = problem if problem is not None else make_problem(M, N, K, seed, with_bias)
    Ad, A2d, Bd = device_operands(A, B, akc, bkc, M1, dev)
    bd = bias.to(dev) if bias is not None else None
    kw = dict(A2=A2d, M1=M1, workers=workers, force_cfg=force)
    C1, C2 = new_c(M, N, dev), new_c(M, N, dev)
    eng.op_gemm2(Ad, akc, Bd, bkc, C1, M, N, K, bias=bd, act=1 if bias is not None else 0, alpha=0.3, **kw)
    plan = eng.op_gemm_last_plan()
    eng.op_gemm2(Ad, akc, Bd, bkc, C2, M, N, K, bias=bd, act=1 if bias is not None else 0, alpha=0.3, **kw)
    err = check_c(C1, M, N, ref, TOL)
    assert torch.equal(C1, C2), "two launches of one product differ: the summation order is not fixed"
    eng.op_gemm2(Ad, akc, Bd, bkc, C1, M, N, K, accumulate=True, **kw)
    err2 = check_c(C1, M, N, ref + prod, TOL_ACC, scale=ref)
    print("gemm %dx%dx%d akc=%d bkc=%d M1=%d w=%d force=%d: err %.2e acc %.2e plan %s" % (M, N, K, akc, bkc, M1, workers, force, err, err2, plan))
    return plan


def cover(plan, kind):
    COVERED.add((plan["cls"], plan["bm"], plan["bn"], kind))


# ---------------------------------------------------------------------------------------------------------------------------------
# plans the planner picks by itself (launch_gemm_mapped -> launch_layout -> plan_cfg), one case per plan
# ---------------------------------------------------------------------------------------------------------------------------------
PLANNER = [
    # name, (M, N, K), (akc, bkc), M1, expected plan fields, Ur == 0 ?
    ("128x128 cut Ur=0", (560, 3040, 2048), (False, False), 0, dict(cls="k_gemm", bm=128, bn=128, n_dp=0, fixup=1, W=256), True),
    ("128x128 cut Ur=0 [A|A2]", (560, 3040, 2048), (False, False), 280, dict(cls="k_gemm", bm=128, bn=128, n_dp=0, fixup=1, W=256), True),
    ("128x128 cut Ur!=0", (516, 3000, 2080), (False, True), 0, dict(cls="k_gemm", bm=128, bn=128, n_dp=0, fixup=1, W=256), False),
    ("128x128 cut Ur!=0 [A|A2]", (516, 3000, 2080), (False, False), 260, dict(cls="k_gemm", bm=128, bn=128, n_dp=0, fixup=1, W=256), False),
    ("128x96 cut (d(h0))", (6400, 280, 3040), (True, True), 0, dict(cls="k_gemm", bm=128, bn=96, n_dp=0, fixup=1, W=256), False),
    ("128x128 whole rounds", (6400, 3040, 280), (True, False), 0, dict(cls="k_gemm", bm=128, bn=128, n_dp=1200, fixup=0, W=256), True),
    ("128x128 rounds + cut remainder", (2700, 4500, 512), (False, False), 0, dict(cls="k_gemm", bm=128, bn=128, n_dp=512, fixup=1, W=256), False),
    ("k_gemm_s 128x256 rounds + cut remainder", (8900, 2700, 512), (True, False), 0, dict(cls="k_gemm_s", bm=128, bn=256, n_dp=512, fixup=1, W=256), False),
    ("96x128 whole", (1600, 3040, 280), (False, False), 0, dict(cls="k_gemm", bm=96, bn=128, n_dp=408, fixup=0), True),
    ("k_gemm_s 128x256", (2048, 8192, 256), (True, False), 0, dict(cls="k_gemm_s", bm=128, bn=256, fixup=0, W=256), True),
    ("k_gemm_s 256x256", (2048, 16384, 256), (False, False), 0, dict(cls="k_gemm_s", bm=256, bn=256, fixup=0, W=256), True),
    ("k_gemm_s 256x128", (14080, 1664, 256), (True, True), 0, dict(cls="k_gemm_s", bm=256, bn=128, fixup=0, W=256), True),
    ("256x64 cut", (30000, 64, 2050), (True, True), 0, dict(cls="k_gemm", bm=256, bn=64, n_dp=0, fixup=1, W=256), False),
    ("256x32 whole", (126000, 32, 256), (True, True), 0, dict(cls="k_gemm", bm=256, bn=32, fixup=0, W=256), True),
    ("gemm16 (below the routing threshold)", (130, 200, 2049), (False, False), 0, dict(cls="gemm16", bm=128, bn=128), True),
    ("gemm16 [A|A2]", (300, 257, 40), (False, False), 128, dict(cls="gemm16", splits=1), True),
    ("n32", (2500, 24, 2000), (True, False), 0, dict(cls="n32", bm=256, bn=32), True),
]


@pytest.mark.parametrize("name,shape,layout,M1,want,ur0", PLANNER, ids=[p[0] for p in PLANNER])
def test_planner_plans(eng, name, shape, layout, M1, want, ur0):
    M, N, K = shape
    plan = run_gemm(eng, M, N, K, layout[0], layout[1], M1=M1, seed=1)
    for k, v in want.items():
        assert plan[k] == v, (k, plan)
    assert (plan["Ur"] == 0) == ur0, plan
    if plan["cls"] == "gemm16" and K >= 2048:
        assert plan["splits"] > 1, plan
    cover(plan, "cut" if plan["fixup"] else "whole")
    if plan["fixup"]:
        cover(plan, "Ur=0" if plan["Ur"] == 0 else "Ur!=0")
    if plan["n_dp"] > plan["W"] > 0:
        cover(plan, "several rounds")
    if plan["n_dp"] > 0 and plan["fixup"]:
        cover(plan, "rounds + cut remainder")
    if M1:
        cover(plan, "[A|A2]")


# ---------------------------------------------------------------------------------------------------------------------------------
# every tile form at its edges, small: forced past the routing rule and the cost comparison (force_cfg of the test entry)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("akc,bkc", LAYOUTS)
@pytest.mark.parametrize("form", range(8), ids=["%s_%dx%d" % f for f in GEMM_FORMS])
def test_forced_form_edges(eng, form, akc, bkc):
    cls, bm, bn = GEMM_FORMS[form]
    # M, N one below / at / one above the tile edge (N % 4 != 0 among them), K around the k-tile and just past 64 k-tiles
    shapes = [(bm - 1, bn + 1, 31), (bm, bn, 32), (bm + 1, bn - 1, 33), (bm - 1, bn, 2049), (bm + 1, bn + 1, 2049), (bm, bn + 2, 2049)]
    for i, (M, N, K) in enumerate(shapes):
        plan = run_gemm(eng, M, N, K, akc, bkc, force=form, seed=10 + i)
        assert (plan["cls"], plan["bm"], plan["bn"]) == (cls, bm, bn), plan
        if K == 2049 and (M > bm or N > bn):
            assert plan["fixup"] == 1 and plan["n_dp"] == 0, plan              # 4 tiles x 65 k-tiles over 32 workers: cut
            cover(plan, "forced cut")
        else:
            cover(plan, "forced")
    if not akc:
        # the stacked operand: M1 a multiple of 4 that is no multiple of the tile, inside the first tile and inside the second
        for M, M1 in ((bm + 1, bm - 28), (2 * bm + 1, bm + 36)):
            plan = run_gemm(eng, M, bn + 1, 2049, akc, bkc, M1=M1, force=form, seed=20)
            assert (plan["cls"], plan["bm"], plan["bn"]) == (cls, bm, bn) and plan["fixup"] == 1, plan
            cover(plan, "forced [A|A2]")
    # worker slots: 9 tiles x 229 k-tiles = 2061 units, enough for 256 workers; one problem, one reference
    M, N, K = 2 * bm + 1, 2 * bn + 1, 7297
    problem = make_problem(M, N, K, 30, True)
    ws = []
    for workers in (8, 64, 224, 256):
        plan = run_gemm(eng, M, N, K, akc, bkc, workers=workers, force=form, problem=problem)
        assert (plan["cls"], plan["bm"], plan["bn"]) == (cls, bm, bn), plan
        assert plan["W"] == workers and plan["fixup"] == 1 and plan["Ur"] != 0, plan
        ws.append(plan["W"])
    cover(plan, "forced workers 8..256")


# ---------------------------------------------------------------------------------------------------------------------------------
# row maps: a window view [samples][positions][channels] of a channels-last activation, both orientations of the SEGAN code
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", [-1, 0, 5], ids=["planner", "128x128", "s256x256"])
@pytest.mark.parametrize("akc", [True, False], ids=["rows_mapped", "k_mapped"])
@pytest.mark.parametrize("rows_per,samples", [(5, 60), (37, 9), (1000, 2)])
def test_row_map_window_views(eng, rows_per, samples, akc, force):
    dev = eng.device
    cin, kw, stride, N = 4, 31, 2, 24
    RL = kw * cin                                         # one window: kw positions x cin channels, contiguous
    inner = stride * cin                                  # < RL: the windows overlap
    Lp = (rows_per - 1) * stride + kw + 5
    outer = Lp * cin
    assert inner < RL and outer > rows_per * inner
    g = gen(rows_per, samples, 77)
    X = torch.randn(samples * outer, generator=g, dtype=torch.float32)
    view = X.double().as_strided((samples, rows_per, RL), (outer, inner, 1)).reshape(samples * rows_per, RL)     # [R][RL]
    R = samples * rows_per
    Xd = torch.cat([X, torch.full((64,), float("nan"))]).to(dev)
    if akc:            # forward: mapped index = output row; C[R][N] = view . W + bias, leaky-relu
        M, K = R, RL
        Bm = torch.randn(K, N, generator=g, dtype=torch.float32) + torch.arange(N, dtype=torch.float32)[None, :] * 0.01
        bias = torch.randn(N, generator=g, dtype=torch.float32)
        prod = view @ Bm.double()
        ref = prod + bias.double()
        ref = torch.maximum(ref, 0.3 * ref)
    else:              # filter gradient: mapped index = k; C[RL][N] = view^T . dY
        M, K = RL, R
        Bm = torch.randn(K, N, generator=g, dtype=torch.float32) + torch.arange(N, dtype=torch.float32)[None, :] * 0.01
        bias = None
        prod = view.t() @ Bm.double()
        ref = prod
    Bd = operand(Bm, dev)
    bd = bias.to(dev) if bias is not None else None
    kwargs = dict(lda=pad4(RL), row_map=(rows_per, outer, inner), force_cfg=force)
    C1, C2 = new_c(M, N, dev), new_c(M, N, dev)
    eng.op_gemm2(Xd, akc, Bd, False, C1, M, N, K, bias=bd, act=1 if akc else 0, alpha=0.3, **kwargs)
    plan = eng.op_gemm_last_plan()
    eng.op_gemm2(Xd, akc, Bd, False, C2, M, N, K, bias=bd, act=1 if akc else 0, alpha=0.3, **kwargs)
    err = check_c(C1, M, N, ref, TOL)
    assert torch.equal(C1, C2)
    eng.op_gemm2(Xd, akc, Bd, False, C1, M, N, K, accumulate=True, **kwargs)
    err2 = check_c(C1, M, N, ref + prod, TOL_ACC, scale=ref)
    print("row map rows_per=%d akc=%d force=%d: err %.2e acc %.2e plan %s" % (rows_per, akc, force, err, err2, plan))
    assert plan["cls"] in ("k_gemm", "k_gemm_s"), plan                 # a window view never takes the split-K kernels
    if force >= 0:
        assert (plan["cls"], plan["bm"], plan["bn"]) == GEMM_FORMS[force], plan
    cover(plan, "row map, rows mapped" if akc else "row map, k mapped")


# ---------------------------------------------------------------------------------------------------------------------------------
# launch_gemm_batch: nb products [A_b | A2_b]^T B_b in one stream-K launch
# ---------------------------------------------------------------------------------------------------------------------------------
def batch_problems(nb, M, N, K, M1, dev, seed):
    """different data per problem (a swapped operand table cannot pass); A and A2 of different leading dimensions"""
    ps = []
    for b in range(nb):
        A, B, _, prod, _ = make_problem(M, N, K, seed + 17 * b, False)
        Ad, A2d, Bd = device_operands(A, B, False, False, M1, dev)
        ps.append((Ad, A2d, Bd, prod))
    return ps


def run_batch(eng, entry, nb, M, N, K, M1, seed, **kw):
    dev = eng.device
    ps = batch_problems(nb, M, N, K, M1, dev, seed)
    As, A2s, Bs = [p[0] for p in ps], ([p[1] for p in ps] if M1 else None), [p[2] for p in ps]
    C1 = [new_c(M, N, dev) for _ in ps]
    C2 = [new_c(M, N, dev) for _ in ps]
    r1 = entry(As, A2s, Bs, C1, M, N, K, M1=M1, **kw)
    plan = eng.op_gemm_last_plan()
    entry(As, A2s, Bs, C2, M, N, K, M1=M1, **kw)
    errs = [check_c(C1[b], M, N, ps[b][3], TOL) for b in range(nb)]
    for b in range(nb):
        assert torch.equal(C1[b], C2[b]), "problem %d: two launches differ" % b
    entry(As, A2s, Bs, C1, M, N, K, M1=M1, accumulate=True, **kw)
    errs2 = [check_c(C1[b], M, N, 2.0 * ps[b][3], TOL_ACC, scale=ps[b][3]) for b in range(nb)]
    print("batch nb=%d %dx%dx%d M1=%d %s: err %.2e acc %.2e plan %s" % (nb, M, N, K, M1, kw, max(errs), max(errs2), plan))
    return r1, plan


@pytest.mark.parametrize("nb,workers", [(2, 0), (3, 0), (4, 0), (3, 224)])
def test_gemm_batch_192x256(eng, nb, workers):
    """the form the training step runs: 192 x 256 tiles on k_gemm_s, cut, one fix-up launch for all problems"""
    ran, plan = run_batch(eng, eng.op_gemm_batch, nb, 560, 3040, 2048, 280, seed=40 + nb, workers=workers)
    assert ran is True
    assert (plan["cls"], plan["bm"], plan["bn"], plan["fixup"], plan["n_dp"]) == ("k_gemm_s_batch", 192, 256, 1, 0), plan
    assert plan["W"] == (workers or 256), plan
    assert (plan["Ur"] == 0) == (workers == 0), plan                  # nb x 36 tiles x 64 k-tiles: a multiple of 256, not of 224
    cover(plan, "workers=%d" % (workers or 256))


@pytest.mark.parametrize("workers", [0, 224])
def test_gemm_batch_128x128(eng, workers):
    """M = 700: 192-row tiles pad as much as 128-row tiles (768), so the batch runs on k_gemm at 128 x 128"""
    ran, plan = run_batch(eng, eng.op_gemm_batch, 2, 700, 3040, 2048, 348, seed=50, workers=workers)
    assert ran is True
    assert (plan["cls"], plan["bm"], plan["bn"], plan["fixup"]) == ("k_gemm_batch", 128, 128, 1), plan
    assert plan["W"] == (workers or 256), plan
    cover(plan, "workers=%d" % (workers or 256))


@pytest.mark.parametrize("nb,shape", [(1, (560, 3040, 2048)), (5, (560, 3040, 2048)), (2, (128, 128, 64)), (3, (560, 3040, 200))])
def test_gemm_batch_not_applicable(eng, nb, shape):
    """one product, more than the table holds, or a product of the split-K kernels: nothing is launched, the caller's C is untouched"""
    dev = eng.device
    M, N, K = shape
    A = torch.zeros(K, pad4(M), dtype=torch.float32, device=dev)
    B = torch.zeros(K, pad4(N), dtype=torch.float32, device=dev)
    Cs = [new_c(M, N, dev) for _ in range(nb)]
    assert eng.op_gemm_batch([A] * nb, None, [B] * nb, Cs, M, N, K) is False
    torch.cuda.synchronize()
    for C_ in Cs:
        assert bool(torch.all(C_ == SENT))


# ---------------------------------------------------------------------------------------------------------------------------------
# launch_gemm16_batch: up to 4 products on the split-K kernel, one reduce launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("shape,M1,split", [((80, 1024, 6400), 40, True),          # the discriminator's dK = [x | m]^T dZ
                                            ((256, 40, 6400), 0, True),            # dWp = h^T dm
                                            ((83, 130, 100), 40, False)],          # short K: no split, no reduce launch
                         ids=["dK", "dWp", "shortK"])
def test_gemm16_batch(eng, n, shape, M1, split):
    M, N, K = shape
    _, plan = run_batch(eng, eng.op_gemm16_batch, n, M, N, K, M1, seed=60 + n)         # (the accumulate pass is part of run_batch)
    assert plan["cls"] == "gemm16_batch", plan
    assert (plan["splits"] > 1) == split, plan
    cover(plan, "split-K" if split else "no split")


# ---------------------------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------------------------
def rowsum32(x):
    """fp32 accumulation in plain row order"""
    acc = torch.zeros(x.shape[1], dtype=torch.float32)
    for r in range(x.shape[0]):
        acc += x[r]
    return acc


NB_OF = {1: 1, 63: 7, 64: 8, 257: 1, 6400: 32}         # rows = T x Nb: c_{t-1} and c_t are the stash at offsets 0 and Nb rows
CS_ROWS, CS_H = [1, 63, 64, 257, 6400], [1, 63, 64, 65, 256, 760]


@pytest.mark.parametrize("H", CS_H)
@pytest.mark.parametrize("rows", CS_ROWS)
def test_lstm_colsums(eng, rows, H):
    dev = eng.device
    nbatch = 2 + (CS_ROWS.index(rows) + CS_H.index(H)) % 3            # the batched launch at 2, 3 or 4 layers; the single launch always
    Nb = NB_OF[rows]
    layers = []
    worst_r = 0.0
    for p in range(nbatch):                                            # distinct data per layer; its references computed once
        g = gen(rows, H, p, 5)
        dz = torch.randn(rows, 4 * H, generator=g, dtype=torch.float32)
        c = torch.randn(rows + Nb, H, generator=g, dtype=torch.float32)
        cp, cc = c[:rows], c[Nb:Nb + rows]
        refs = []
        for x32 in (dz, dz[:, :H] * cp, dz[:, 2 * H:3 * H] * cp, dz[:, 3 * H:] * cc):
            ref = x32.double().sum(0)
            refs.append(ref)
            worst_r = max(worst_r, relerr(rowsum32(x32).double(), ref))
        layers.append((dz.to(dev), c.to(dev), refs))
    worst_k = 0.0
    for nb in (1, nbatch):
        use = layers[-nb:]                                             # (nb = 1 runs the last layer's data)
        dzd, cd = [u[0] for u in use], [u[1] for u in use]
        db = [torch.empty(4 * H + 8, dtype=torch.float32, device=dev) for _ in use]
        dw = [[torch.empty(H + 8, dtype=torch.float32, device=dev) for _ in use] for _ in range(3)]
        out = []
        for rep in range(2):
            for t in db + dw[0] + dw[1] + dw[2]:
                t.fill_(SENT)
            eng.op_lstm_colsums(dzd, [c[:rows] for c in cd], [c[Nb:Nb + rows] for c in cd], db, dw[0], dw[1], dw[2], rows, H)
            torch.cuda.synchronize()
            out.append([t.cpu().clone() for t in db + dw[0] + dw[1] + dw[2]])
        for a, b in zip(out[0], out[1]):
            assert torch.equal(a, b), "two launches differ"
        for p, u in enumerate(use):
            for got, n, ref in zip((db[p], dw[0][p], dw[1][p], dw[2][p]), (4 * H, H, H, H), u[2]):
                gc = got.cpu()
                assert bool(torch.all(gc[n:] == SENT)), "outputs beyond 4H / H written"
                worst_k = max(worst_k, relerr(gc[:n].double(), ref))
    print("lstm_colsums rows=%d H=%d nb=1,%d: kernel err %.3e, fp32 row-order err %.3e" % (rows, H, nbatch, worst_k, worst_r))
    assert worst_k <= 4.0 * worst_r, (worst_k, worst_r)


def run_colsum(eng, rows, cols, mult, tall, seed):
    """cols < 16: the launch runs on 16 // cols column windows of one wide matrix (independent data), so that the two errors of a
    shape are maxima over at least 16 sums and not one rounding each"""
    dev = eng.device
    nwin = max(1, 16 // cols)
    g = gen(rows, cols, seed)
    a = torch.randn(rows, cols * nwin + 3, generator=g, dtype=torch.float32)       # lda != cols
    b = torch.randn(rows, cols * nwin + 8, generator=g, dtype=torch.float32)
    ad, bd = a.to(dev), b.to(dev)
    x32 = a[:, :cols * nwin] * b[:, :cols * nwin] if mult else a[:, :cols * nwin]
    ref = x32.double().sum(0)
    er = relerr(rowsum32(x32).double(), ref)
    got = []
    for w in range(nwin):
        outs = []
        for rep in range(2):
            out = torch.full((cols + 8,), SENT, dtype=torch.float32, device=dev)
            eng.op_colsum(ad[:, w * cols:], out, rows, cols, b=bd[:, w * cols:] if mult else None, tall=tall)
            torch.cuda.synchronize()
            outs.append(out.cpu())
        assert torch.equal(outs[0], outs[1]), "two launches differ"
        assert bool(torch.all(outs[0][cols:] == SENT)), "outputs beyond cols written"
        got.append(outs[0][:cols])
    ek = relerr(torch.cat(got).double(), ref)
    print("colsum%s rows=%d cols=%d b=%d: kernel err %.3e, fp32 row-order err %.3e" % ("_tall" if tall else "", rows, cols, mult, ek, er))
    assert ek <= 4.0 * er, (ek, er)


@pytest.mark.parametrize("mult", [False, True], ids=["plain", "times_b"])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 760])
@pytest.mark.parametrize("rows", CS_ROWS)
def test_colsum(eng, rows, cols, mult):
    run_colsum(eng, rows, cols, mult, False, 9)


@pytest.mark.parametrize("cols", [1, 24, 32])
@pytest.mark.parametrize("rows", [100, 100000])
def test_colsum_tall(eng, rows, cols):
    run_colsum(eng, rows, cols, False, True, 11)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_zz_covered_plans_listed():
    """prints, once, every (kernel class, tile, plan kind) a passing case above asserted; when the whole module ran, every kernel class
    and every tile form of the stream-K kernels must be among them"""
    print("plans asserted by passing cases:")
    for c in sorted(COVERED):
        print("  %-15s %3dx%-3d %s" % c)
    classes = {c[0] for c in COVERED}
    if len(COVERED) < 40:                                  # a partial run (-k): nothing to require
        return
    assert classes == {"gemm16", "n32", "k_gemm", "k_gemm_s", "gemm16_batch", "k_gemm_batch", "k_gemm_s_batch"}, classes
    planner = {(c[0], c[1], c[2]) for c in COVERED if not c[3].startswith("forced") and not c[3].startswith("row map")}
    for f in GEMM_FORMS:
        assert f in planner, ("tile form never picked by the planner in a passing case", f)
    kinds = {c[3] for c in COVERED}
    for k in ("cut", "whole", "Ur=0", "Ur!=0", "several rounds", "rounds + cut remainder", "[A|A2]", "row map, rows mapped", "row map, k mapped", "split-K", "no split"):
        assert k in kinds, k
    assert ("k_gemm_s_batch", 192, 256, "workers=224") in COVERED and ("k_gemm_batch", 128, 128, "workers=256") in COVERED
