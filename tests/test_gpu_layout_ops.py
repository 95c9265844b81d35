"""The layout, staging and weight-copy kernels (csrc/kernels.hip: k_pack_tm, k_unpack_bm, k_stage_inputs, k_build_d_input, k_add_noise_rows,
k_build_joint, k_slice_cols, k_transpose, k_transpose_many, k_swizzle_many, k_im2col<4> / <1>, k_col2im, k_expand_c4, k_gstate, k_window_len,
k_zero_many, k_fill, k_copy_f, k_pad_copy), each through the launch_* function the model calls (rsrgan_op_layout), against the references of
tests/layout_ref.py (checked on their own in tests/test_layout_ref.py).  Every kernel here is a copy, one fp32 add or one fixed-order fp32
sum, so every comparison is of bits: there is no tolerance in this file.

Every destination sits between two guard bands and starts, guards included, as a NaN of the payload 0x7fc0dead -- a long-lived buffer that
holds an earlier call's data, not the zeros of a fresh allocation.  The reference starts from the same contents, so a promised zero that is
not written and a write where none is promised both show.  The guard is 64 floats; the transposes take 4096, which holds every store a
tile kernel without its edge test would make.  Sources hold random normals and a few special values (-0.0, a denormal, +inf), so a kernel
that computes where it should copy shows.  The whole buffer is compared; a mismatch prints its first index and the count."""
import numpy as np
import pytest
import torch

from rsrgan_amd.ops import OpEntries
from tests import layout_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32
POISON = 0x7fc0dead
GUARD = 64                                     # floats on each side of every destination
WIDE = 4096                                    # ... of the transposes' (see above)


@pytest.fixture(scope="module")
def eng():
    return OpEntries()


def poison(n):
    return np.full(n, POISON, dtype=np.uint32).view(f32)


def source(n, seed):
    """n random normals with -0.0, a denormal and +inf among them"""
    x = np.random.default_rng(seed).standard_normal(n).astype(f32)
    for at, v in ((0, -0.0), (n // 3, 1e-40), (n // 2, np.inf), (n - 1, -0.0)):
        x[at] = f32(v)
    return x


def dev(host):
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


class Dst:
    """a destination of n floats (or int32 words) between two guards, all of it poisoned, or holding `body` between poisoned guards"""

    def __init__(self, n, guard=GUARD, body=None):
        self.n, self.guard = n, guard
        self.before = poison(n) if body is None else np.ascontiguousarray(body, dtype=f32).reshape(-1).copy()
        self.t = dev(np.concatenate([poison(guard), self.before, poison(guard)]))
        self.view = self.t[guard:guard + n]
        assert self.view.data_ptr() % 16 == 0

    def check(self, want, what):
        got = self.t.cpu().numpy().view(np.uint32)
        exp = np.concatenate([poison(self.guard), np.ascontiguousarray(want).reshape(-1).view(f32), poison(self.guard)]).view(np.uint32)
        assert got.shape == exp.shape, (what, got.shape, exp.shape)
        bad = np.flatnonzero(got != exp)
        if bad.size:
            i = int(bad[0])
            print("layout_ops %s: %d of %d words differ, the first at %d (body starts at %d): got 0x%08x, want 0x%08x"
                  % (what, bad.size, got.size, i, self.guard, got[i], exp[i]))
        assert bad.size == 0, "%s: %d words differ, the first at index %d of the guarded buffer" % (what, bad.size, int(bad[0]))


def done(eng):
    assert eng.device_status() == 0


# ------------------------------------------------------------------------------------------------ batch-major <-> time-major
PACK_SHAPES = [(3, 5, 257, 260), (3, 5, 40, 48), (1, 1, 1, 4)]       # 128-thread blocks and 3 strides / 64-thread blocks / the smallest


@pytest.mark.parametrize("B,T,D,ld", PACK_SHAPES)
def test_pack_tm(eng, B, T, D, ld):
    src = source(B * T * D, 1)
    dst = Dst(T * B * ld)
    eng.op_layout("pack_tm", [dev(src), dst.view], [B, T, D, ld])
    done(eng)
    dst.check(R.pack_tm_ref(src, B, T, D, ld, dst.before), "pack_tm")


@pytest.mark.parametrize("B,T,D,ld,Bt", [s + (0,) for s in PACK_SHAPES] + [(4, 5, 257, 260, 2), (4, 5, 40, 48, 2)])
def test_unpack_bm(eng, B, T, D, ld, Bt):
    src = source(T * B * ld, 2)
    dst = Dst(B * T * D)                       # (Bt of B rows: the rows behind them keep the poison)
    eng.op_layout("unpack_bm", [dev(src), dst.view], [B, T, D, ld, Bt])
    done(eng)
    dst.check(R.unpack_bm_ref(src, ld, B, T, D, Bt, dst.before), "unpack_bm")


@pytest.mark.parametrize("have", [(1, 1), (1, 0), (0, 1)])
def test_stage_inputs(eng, have):
    """both packs with different D, each absent in turn; copies of 1, 3 and 300 words (one float, two int32) and one NULL slot.  The sources
    of the packs are B rows tall although Bt rows are the caller's: rows [Bt, B) of every destination frame must keep the poison"""
    B, T, Bt = 4, 5, 3
    packs, ptrs, dims = [], [], [B, T, Bt]
    for k, (D, ld) in enumerate(((257, 260), (40, 48))):
        src = source(B * T * D, 3 + k) if have[k] else None
        dst = Dst(T * B * ld)
        packs.append((src, D, ld, dst))
        ptrs += [None if src is None else dev(src), dst.view]
        dims += [D, ld]
    copies = []
    for k, n in enumerate((1, 3, None, 300)):
        if n is None:
            src = None
        elif k == 3:
            src = source(n + 8, 9)
        else:
            src = np.arange(100, 100 + n + 8, dtype=np.int32).view(f32)
        dst = Dst((n or 4) + 8)
        copies.append((src, n or 4, dst))
        ptrs += [None if src is None else dev(src), dst.view]
        dims.append(n or 4)
    eng.op_layout("stage_inputs", ptrs, dims)
    done(eng)
    po, co = R.stage_inputs_ref([(s, D, ld, d.before) for s, D, ld, d in packs], [(s, n, d.before) for s, n, d in copies], B, T, Bt)
    for k in range(2):
        packs[k][3].check(po[k], "stage_inputs pack %d" % k)
    for k in range(4):
        copies[k][2].check(co[k], "stage_inputs copy %d" % k)


def test_stage_inputs_all_rows(eng):
    """Bt = 0: every one of the B rows"""
    B, T, D, ld = 3, 2, 40, 44
    src, dst = source(B * T * D, 5), Dst(T * B * ld)
    eng.op_layout("stage_inputs", [dev(src), dst.view] + [None] * 10, [B, T, 0, D, ld, 1, 1, 1, 1, 1, 1])
    done(eng)
    po, _ = R.stage_inputs_ref([(src, D, ld, dst.before)], [], B, T, 0)
    dst.check(po[0], "stage_inputs Bt = 0")


# ------------------------------------------------------------------------------------------------ the discriminator's input
D_INPUT = [(3, 4, 40, 48, wr, nr, nf) for wr in (0, 1) for nr in (0, 1) for nf in (0, 1)] + [(64, 17, 257, 260, 1, 1, 1)]


@pytest.mark.parametrize("B,T,D,ld,with_real,has_nr,has_nf", D_INPUT)
def test_build_d_input(eng, B, T, D, ld, with_real, has_nr, has_nf):
    """(64, 17, 257, 260): 559,232 elements, above the 2048 x 256 one pass of the capped grid covers"""
    lab, y = source(T * B * ld, 11), source(T * B * ld, 12)
    nr = source(B * D, 13) if has_nr else None
    nf = source(B * D, 14) if has_nf else None
    dst = Dst(T * (2 * B if with_real else B) * ld)
    eng.op_layout("build_d_input", [dev(lab) if with_real else None, dev(y), None if nr is None else dev(nr), None if nf is None else dev(nf), dst.view],
                  [B, T, D, ld, with_real])
    done(eng)
    dst.check(R.build_d_input_ref(lab, y, nr, nf, B, T, D, ld, with_real, dst.before), "build_d_input")


@pytest.mark.parametrize("B,T,D,ld,Ns,row0", [(3, 4, 40, 48, 8, 5), (3, 4, 40, 48, 3, 0), (64, 33, 257, 260, 70, 3)])
@pytest.mark.parametrize("has_noise", [0, 1])
def test_add_noise_rows(eng, B, T, D, ld, Ns, row0, has_noise):
    """(64, 33, 257): 542,784 elements, above one pass of the capped grid; rows outside [row0, row0 + B) keep the poison"""
    src = source(T * B * ld, 15)
    noise = source(B * D, 16) if has_noise else None
    dst = Dst(T * Ns * ld)
    eng.op_layout("add_noise_rows", [dev(src), None if noise is None else dev(noise), dst.view], [B, T, D, ld, Ns, row0])
    done(eng)
    dst.check(R.add_noise_rows_ref(src, noise, B, T, D, ld, Ns, row0, dst.before), "add_noise_rows")


@pytest.mark.parametrize("ldx,off,dim,ldt,Dt,ldj,row0,Rn", [(52, 3, 44, 40, 40, 88, 5, 5), (52, 3, 0, 40, 40, 88, 5, 5), (52, 3, 44, 40, 40, 88, 5, 6300)])
def test_build_joint(eng, ldx, off, dim, ldt, Dt, ldj, row0, Rn):
    """R = 6300: 529,200 elements, above one pass of the capped grid; rows outside [row0, row0 + R) keep the poison"""
    x, tail = source(Rn * ldx, 17), source(Rn * ldt, 18)
    dst = Dst((row0 + Rn + 3) * ldj)
    eng.op_layout("build_joint", [dev(x) if dim else None, dev(tail), dst.view], [ldx, off, dim, ldt, Dt, ldj, row0, Rn])
    done(eng)
    dst.check(R.build_joint_ref(x, ldx, off, dim, tail, ldt, Dt, ldj, row0, Rn, dst.before), "build_joint")


@pytest.mark.parametrize("lds,off,ldd,Rn,C", [(88, 44, 48, 5, 40), (88, 44, 48, 13200, 40)])
def test_slice_cols(eng, lds, off, ldd, Rn, C):
    """R = 13200: 528,000 elements, above one pass of the capped grid"""
    src = source(Rn * lds, 19)
    dst = Dst(Rn * ldd)
    eng.op_layout("slice_cols", [dev(src), dst.view], [lds, off, ldd, Rn, C])
    done(eng)
    dst.check(R.slice_cols_ref(src, lds, off, ldd, Rn, C, dst.before), "slice_cols")


# ------------------------------------------------------------------------------------------------ weight copies
TR_SHAPES = [(1, 1), (32, 32), (33, 65), (7, 100)]                   # (R, C); lds = C + 3, ldd = R + 5


@pytest.mark.parametrize("Rn,C", TR_SHAPES)
def test_transpose(eng, Rn, C):
    lds, ldd = C + 3, Rn + 5
    src = source(Rn * lds, 21)
    dst = Dst(C * ldd, guard=WIDE)
    eng.op_layout("transpose", [dev(src), dst.view], [lds, ldd, Rn, C])
    done(eng)
    dst.check(R.transpose_ref(src, lds, ldd, Rn, C, dst.before), "transpose")


@pytest.mark.parametrize("order", ["forward", "reverse", "sixteen"])
def test_transpose_many(eng, order):
    """the four shapes in one launch, in both orders (unequal block counts under the block-to-job search), and a full list of 16 jobs"""
    shapes = {"forward": TR_SHAPES, "reverse": TR_SHAPES[::-1], "sixteen": TR_SHAPES * 4}[order]
    jobs, ptrs, dims = [], [], [len(shapes)]
    for j, (Rn, C) in enumerate(shapes):
        lds, ldd = C + 3, Rn + 5
        src, dst = source(Rn * lds, 30 + j), Dst(C * ldd, guard=WIDE)
        jobs.append((src, lds, ldd, Rn, C, dst))
        ptrs += [dev(src), dst.view]
        dims += [lds, ldd, Rn, C]
    eng.op_layout("transpose_many", ptrs, dims)
    done(eng)
    for j, (src, lds, ldd, Rn, C, dst) in enumerate(jobs):
        dst.check(R.transpose_ref(src, lds, ldd, Rn, C, dst.before), "transpose_many job %d" % j)


SW_H, SW_I, SW_P, SW_LDI, SW_LDP = 20, 7, 12, 8, 16


def swizzle_jobs():
    """(name, source, job): the forms Model::refresh_swizzles builds at H = 20 (ncb = 2), I = 7, P = 12, ldI = 8 -- the gates image with kx = ldI
    and kx = 0, the kernel's rows from c0 = 0 and c0 = I, the projection transposed (gates = 1) and plain -- and a job of 3 tiles = 192
    float4: the tail threads of its one block must write nothing"""
    g = np.random.default_rng(41)
    H, I, P, ldI, ldP = SW_H, SW_I, SW_P, SW_LDI, SW_LDP
    K = source((I + P) * 4 * H, 42)
    Wp = source(H * ldP, 43)
    odd = g.standard_normal(40 * 12).astype(f32)
    ncb, kb4, kbH = (H + 15) // 16, (4 * H + 15) // 16, ((H + 3) // 4 * 4 + 15) // 16

    def job(**kw):
        j = dict(ld=0, gates=0, H=0, C=0, c0=0, K1=0, I=0, P=0, kx=0, nct=1, nkb=1)
        j.update(kw)
        return j
    return [("Wg_full", K, job(ld=4 * H, gates=4, H=H, I=I, P=P, kx=ldI, nct=4 * ncb, nkb=(ldI + P + 15) // 16)),
            ("Wg_h", K, job(ld=4 * H, gates=4, H=H, I=I, P=P, kx=0, nct=4 * ncb, nkb=(P + 15) // 16)),
            ("Kb_full", K, job(ld=4 * H, C=I + P, c0=0, K1=4 * H, nct=(I + P + 15) // 16, nkb=kb4)),
            ("Kb_rec", K, job(ld=4 * H, C=P, c0=I, K1=4 * H, nct=(P + 15) // 16, nkb=kb4)),
            ("WpT_sw", Wp, job(ld=ldP, gates=1, H=P, I=H, P=0, kx=16 * kbH, nct=(P + 15) // 16, nkb=kbH)),
            ("Wp_sw", Wp, job(ld=ldP, C=H, c0=0, K1=P, nct=ncb, nkb=(P + 15) // 16)),
            ("three_tiles", odd, job(ld=12, C=40, c0=0, K1=10, nct=3, nkb=1))]


SW_FIELDS = ("ld", "gates", "H", "C", "c0", "K1", "I", "P", "kx", "nct", "nkb")


def run_swizzles(eng, jobs):
    ptrs, dims, dsts = [], [len(jobs)], []
    for _, src, j in jobs:
        dst = Dst(j["nct"] * j["nkb"] * 256)                          # exactly swizzle_floats(nct, nkb) between the guards
        dsts.append(dst)
        ptrs += [dev(src), dst.view]
        dims += [j[f] for f in SW_FIELDS]
    eng.op_layout("swizzle_many", ptrs, dims)
    done(eng)
    for (name, src, j), dst in zip(jobs, dsts):
        dst.check(R.swizzle_ref(src, j, dst.before), "swizzle_many %s" % name)


@pytest.mark.parametrize("which", ["all", "Wg_full", "Wg_h", "Kb_full", "Kb_rec", "WpT_sw", "Wp_sw", "three_tiles", "reverse", "twentyfour"])
def test_swizzle_many(eng, which):
    jobs = swizzle_jobs()
    assert [j["nct"] * j["nkb"] for name, _, j in jobs if name == "three_tiles"] == [3]
    if which == "reverse":
        jobs = jobs[::-1]
    elif which == "twentyfour":
        jobs = (jobs * 4)[:24]
    elif which != "all":
        jobs = [j for j in jobs if j[0] == which]
    run_swizzles(eng, jobs)


# ------------------------------------------------------------------------------------------------ R-CED's patch matrix
GEOMS = [(5, 4, 3), (6, 4, 4)]                 # (W, kh, kw) at S = 4, R = 2: kh = S and even is what the R-CED layers pass


@pytest.mark.parametrize("W,kh,kw", GEOMS)
@pytest.mark.parametrize("C,ldc,slack", [(4, 4, 0), (4, 4, 8), (4, 8, 4), (3, 3, 0), (3, 3, 5), (1, 1, 0), (1, 1, 3)])
def test_im2col(eng, W, kh, kw, C, ldc, slack):
    """C = 4 on ldc = 4 / 8: the float4 form (ldk = K + 4); C = 3 and C = 1: the scalar form (ldk = K + 1); slack: row_stride above S W ldc"""
    S, Rn = 4, 2
    K, M, row_stride = kh * kw * C, Rn * S * W, S * W * ldc + slack
    ldk = K + 4 if C % 4 == 0 else K + 1
    src = source(Rn * row_stride, 51)
    dst = Dst(M * ldk)
    eng.op_layout("im2col", [dev(src), dst.view], [row_stride, ldc, C, S, W, kh, kw, ldk, M])
    done(eng)
    dst.check(R.im2col_ref(src, row_stride, ldc, C, S, W, kh, kw, ldk, M, dst.before), "im2col")


@pytest.mark.parametrize("W,kh,kw", GEOMS)
@pytest.mark.parametrize("C,ldc", [(4, 8), (8, 8)])
def test_col2im(eng, W, kh, kw, C, ldc):
    """C = 4 on ldc = 8: the pad columns come back as +0.0; the sums are fp32, dh outer and dw inner"""
    S, Rn = 4, 2
    K, M = kh * kw * C, Rn * S * W
    ldk = K + 4
    dcol = source(M * ldk, 52)
    dst = Dst(M * ldc)
    eng.op_layout("col2im", [dev(dcol), dst.view], [ldk, C, S, W, kh, kw, ldc, M])
    done(eng)
    dst.check(R.col2im_ref(dcol, ldk, C, S, W, kh, kw, ldc, M, dst.before), "col2im")


def test_expand_c4(eng):
    rows, n, ld_src = 3, 20, 23
    src = source(rows * ld_src, 53)
    dst = Dst(rows * n * 4)
    eng.op_layout("expand_c4", [dev(src), dst.view], [ld_src, n, rows])
    done(eng)
    dst.check(R.expand_c4_ref(src, ld_src, n, rows, dst.before), "expand_c4")


# ------------------------------------------------------------------------------------------------ carried state, windows
GS_LAYERS = [(20, 12, 16), (20, 0, 0)]         # (H, P, ldP): a projected layer and an unprojected one
GS_SPARE, GS_ROWS, GS_SLOT = 5, 3, 2


def gstate_case(direction):
    """state [rows][SF] with SF = the layers' H + P and 5 spare floats; c / mst stashes of slot + rows rows.  The side a direction reads
    holds data, the side it writes the poison"""
    SF = sum(H + P for H, P, _ in GS_LAYERS) + GS_SPARE
    state = Dst(GS_ROWS * SF, body=source(GS_ROWS * SF, 61) if direction == 0 else None)
    layers, off, n = [], 0, GS_SLOT + GS_ROWS
    for l, (H, P, ldP) in enumerate(GS_LAYERS):
        c = Dst(n * H, body=source(n * H, 62 + l) if direction == 1 else None)
        m = None if ldP == 0 else Dst(n * ldP, body=source(n * ldP, 64 + l) if direction == 1 else None)
        layers.append((c, m, H, P, ldP, off))
        off += H + P
    return SF, state, layers


def run_gstate(eng, direction, rows, mask):
    SF, state, layers = gstate_case(direction)
    ptrs = [state.view, None if mask is None else dev(np.asarray(mask, dtype=np.int32))]
    dims = [len(layers), SF, rows, direction, GS_SLOT]
    for c, m, H, P, ldP, off in layers:
        ptrs += [c.view, None if m is None else m.view]
        dims += [H, P, ldP, off]
    eng.op_layout("gstate", ptrs, dims)
    done(eng)
    st, cs, ms = R.gstate_ref(state.before, [(c.before, None if m is None else m.before, H, P, ldP, off) for c, m, H, P, ldP, off in layers],
                              SF, rows, direction, GS_SLOT, mask)
    state.check(st, "gstate dir %d state" % direction)
    for l, (c, m, *_) in enumerate(layers):
        c.check(cs[l], "gstate dir %d c of layer %d" % (direction, l))
        if m is not None:
            m.check(ms[l], "gstate dir %d mst of layer %d" % (direction, l))


def test_gstate_load(eng):
    """dir 0: the slot's c and mst rows from the state, mst's columns [P, ldP) +0.0 over the poison; rows below the slot, the state and its
    spare floats untouched"""
    run_gstate(eng, 0, GS_ROWS, None)


def test_gstate_store_and_round_trip(eng):
    """dir 1: the state's valid part from the slot, its spare floats untouched; and a load followed by a store gives the state back"""
    run_gstate(eng, 1, GS_ROWS, None)
    SF, state, layers = gstate_case(0)
    back = Dst(GS_ROWS * SF)
    for direction, st in ((0, state), (1, back)):
        ptrs, dims = [st.view, None], [len(layers), SF, GS_ROWS, direction, GS_SLOT]
        for c, m, H, P, ldP, off in layers:
            ptrs += [c.view, None if m is None else m.view]
            dims += [H, P, ldP, off]
        eng.op_layout("gstate", ptrs, dims)
    done(eng)
    want = back.before.copy()
    for row in range(GS_ROWS):
        for _, _, H, P, _, off in layers:
            want[row * SF + off:row * SF + off + H + P] = state.before[row * SF + off:row * SF + off + H + P]
    back.check(want, "gstate round trip")


@pytest.mark.parametrize("mask", [None, (1, 0, 1)])
def test_gstate_reset(eng, mask):
    """dir 2: whole state rows +0.0, the masked-out row keeps its contents (here: the poison)"""
    SF, _, layers = gstate_case(0)
    state = Dst(GS_ROWS * SF)
    ptrs, dims = [state.view, None if mask is None else dev(np.asarray(mask, dtype=np.int32))], [len(layers), SF, GS_ROWS, 2, GS_SLOT]
    for c, m, H, P, ldP, off in layers:
        ptrs += [None, None]
        dims += [H, P, ldP, off]
    eng.op_layout("gstate", ptrs, dims)
    done(eng)
    st, _, _ = R.gstate_ref(state.before, [(c.before, None, H, P, ldP, off) for c, m, H, P, ldP, off in layers], SF, GS_ROWS, 2, GS_SLOT, mask)
    assert (st.view(np.uint32) == POISON).sum() == (SF if mask else 0)
    state.check(st, "gstate dir 2")


@pytest.mark.parametrize("direction", [0, 1, 2])
def test_gstate_no_rows(eng, direction):
    """rows = 0: no launch, nothing changes"""
    run_gstate(eng, direction, 0, None)


class IntDst(Dst):
    def check(self, want, what):
        super().check(np.ascontiguousarray(want, dtype=np.int32).view(f32), what)


@pytest.mark.parametrize("t0,Tw", [(0, 5), (5, 5), (3, 1000)])
def test_window_len(eng, t0, Tw):
    length = np.array([0, 1, 5, 6, 100], dtype=np.int32)
    dst = IntDst(8)
    eng.op_layout("window_len", [dev(length), dst.view], [5, t0, Tw])
    done(eng)
    want = R.window_len_ref(length, 5, t0, Tw, dst.before.view(np.int32))
    assert list(want[:5]) == [min(max(int(v) - t0, 0), Tw) for v in length]
    dst.check(want, "window_len")
    none = IntDst(8)
    eng.op_layout("window_len", [dev(length), none.view], [0, t0, Tw])      # n = 0: a no-op
    done(eng)
    none.check(none.before.view(np.int32), "window_len n = 0")


# ------------------------------------------------------------------------------------------------ buffers
def test_zero_many(eng):
    """one launch, 32 blocks of 256 threads per buffer: one element, less than a block, exactly one pass (8192), one more, several passes.
    Each buffer has its own guards; the zeros are +0.0"""
    lens = (1, 255, 8192, 8193, 20000)
    dsts = [Dst(n) for n in lens]
    eng.op_layout("zero_many", [d.view for d in dsts], [len(lens)] + list(lens))
    done(eng)
    for n, d, want in zip(lens, dsts, R.zero_many_ref(lens, [d.before for d in dsts])):
        assert not want[:n].view(np.uint32).any()
        d.check(want, "zero_many %d" % n)


def test_zero_many_full_list(eng):
    lens = [1 + 37 * j for j in range(32)]
    dsts = [Dst(n + 3) for n in lens]
    eng.op_layout("zero_many", [d.view for d in dsts], [32] + lens)
    done(eng)
    for n, d, want in zip(lens, dsts, R.zero_many_ref(lens, [d.before for d in dsts])):
        d.check(want, "zero_many of 32, %d" % n)


@pytest.mark.parametrize("n", [1, 257, 600000])
@pytest.mark.parametrize("v", [-0.0, 1.5])
def test_fill(eng, n, v):
    """600000: above the 2048 x 256 one pass of the capped grid covers; -0.0 keeps its sign"""
    dst = Dst(n + 5)
    eng.op_layout("fill", [dst.view], [n], [v])
    done(eng)
    dst.check(R.fill_ref(n, v, dst.before), "fill")


@pytest.mark.parametrize("n", [1, 3, 4, 300])
def test_copy_f(eng, n):
    src = source(n + 4, 71)
    dst = Dst(n + 4)
    eng.op_layout("copy_f", [dev(src), dst.view], [n])
    done(eng)
    dst.check(R.copy_f_ref(src, n, dst.before), "copy_f")


@pytest.mark.parametrize("rows,cols,ld", [(5, 7, 8), (1, 1, 4), (520, 513, 516)])
@pytest.mark.parametrize("to_padded", [1, 0])
def test_pad_copy(eng, rows, cols, ld, to_padded):
    """(520, 513, 516): 266,760 elements, above the 1024 x 256 one pass of the capped grid covers.  The side that is read is unchanged"""
    dense = Dst(rows * cols, body=source(rows * cols, 72) if to_padded else None)
    padded = Dst(rows * ld, body=None if to_padded else source(rows * ld, 73))
    eng.op_layout("pad_copy", [dense.view, padded.view], [rows, cols, ld, to_padded])
    done(eng)
    dn, pd = R.pad_copy_ref(dense.before, padded.before, rows, cols, ld, to_padded)
    dense.check(dn, "pad_copy dense")
    padded.check(pd, "pad_copy padded")
