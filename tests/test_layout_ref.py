"""tests/layout_ref.py -- the references tests/test_gpu_layout_ops.py compares the layout kernels with -- against independent
formulations (no GPU): the patch matrix against torch's conv2d on an explicitly TF-SAME-padded input, col2im as its adjoint, the tiled
weight image read back lane by lane against the logical matrices built by slicing, the row builders against np.concatenate."""
import numpy as np
import pytest
import torch

from tests import layout_ref as R

f32, f64 = np.float32, np.float64


def rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------------ im2col / col2im
GEOMS = [(4, 5, 4, 3), (4, 6, 4, 4), (5, 4, 3, 2), (3, 3, 1, 1), (4, 5, 2, 5)]       # (S, W, kh, kw): odd and even extents


@pytest.mark.parametrize("S,W,kh,kw", GEOMS)
@pytest.mark.parametrize("C,ldc", [(4, 4), (3, 5), (1, 1)])
def test_im2col_is_conv2d_on_the_same_padded_input(S, W, kh, kw, C, ldc):
    """im2col_ref(x) @ F.reshape(K, Cout) = conv2d(pad_TF_SAME(x), F): (k - 1) // 2 leading and k // 2 trailing zeros per axis"""
    g = rng(S * 100 + W * 10 + kh + kw + C)
    Rn, Cout, K = 2, 3, kh * kw * C
    ldk, row_stride, M = K + 2, S * W * ldc + 3, Rn * S * W
    src = g.standard_normal(Rn * row_stride).astype(f32)
    F = g.standard_normal((kh, kw, C, Cout))
    col = R.im2col_ref(src, row_stride, ldc, C, S, W, kh, kw, ldk, M, np.full(M * ldk, 7.0, f32)).reshape(M, ldk)
    assert np.all(col[:, K:] == 0.0)
    got = col[:, :K].astype(f64) @ F.reshape(K, Cout)
    x = np.stack([src[r * row_stride:r * row_stride + S * W * ldc].reshape(S, W, ldc)[:, :, :C] for r in range(Rn)]).astype(f64)
    xp = np.pad(x, ((0, 0), ((kh - 1) // 2, kh // 2), ((kw - 1) // 2, kw // 2), (0, 0)))
    want = torch.nn.functional.conv2d(torch.from_numpy(xp).permute(0, 3, 1, 2), torch.from_numpy(F).permute(3, 2, 0, 1))
    want = want.permute(0, 2, 3, 1).reshape(M, Cout).numpy()
    assert want.shape == got.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("S,W,kh,kw", GEOMS)
@pytest.mark.parametrize("C,ldc", [(4, 8), (8, 8)])
def test_col2im_is_the_adjoint_of_im2col(S, W, kh, kw, C, ldc):
    """<im2col(x), d> == <x, col2im(d)> in fp64 (the fp32 sums of col2im_ref are exact on these small-integer values)"""
    g = rng(S * 100 + W * 10 + kh + kw + C)
    Rn, K = 2, kh * kw * C
    ldk, M = K + 4, Rn * S * W
    x = g.integers(-8, 9, size=(M, ldc)).astype(f32)
    d = g.integers(-8, 9, size=(M, ldk)).astype(f32)
    col = R.im2col_ref(x, S * W * ldc, ldc, C, S, W, kh, kw, ldk, M, np.zeros(M * ldk, f32)).reshape(M, ldk)
    back = R.col2im_ref(d, ldk, C, S, W, kh, kw, ldc, M, np.full(M * ldc, 7.0, f32)).reshape(M, ldc)
    assert np.all(back[:, C:] == 0.0) and not np.signbit(back[:, C:]).any()
    lhs = float((col[:, :K].astype(f64) * d[:, :K].astype(f64)).sum())
    rhs = float((x[:, :C].astype(f64) * back[:, :C].astype(f64)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


def test_col2im_sums_in_fp32_dh_outer_dw_inner():
    """one interior position of a 3 x 3 filter: nine terms whose fp32 sum depends on the order"""
    S = W = kh = kw = 3
    C, ldc, K = 4, 4, 36
    d = np.zeros((9, K), f32)
    vals = [f32(2.0 ** 24), f32(1.0), f32(1.0), f32(-2.0 ** 24), f32(1.0), f32(0.5), f32(3.0), f32(2.0 ** -10), f32(7.0)]
    for dh in range(3):
        for dw in range(3):
            ho, wo = 1 - dh + 1, 1 - dw + 1        # the output position whose patch element (dh, dw) is the centre (1, 1)
            d[ho * W + wo, (dh * kw + dw) * C] = vals[dh * 3 + dw]
    acc = f32(0.0)
    for v in vals:
        acc = f32(acc + v)
    got = R.col2im_ref(d, K, C, S, W, kh, kw, ldc, 9, np.zeros(36, f32)).reshape(9, 4)
    assert got[4, 0] == acc and acc != f32(sum(float(v) for v in vals))


# ------------------------------------------------------------------------------------------------ the fragment-tiled weight copies
H, I, P, LDI, LDP = 20, 7, 12, 8, 16


def read_back(img, nct, nkb):
    """lane by lane: the float4 at tile * 256 + 16 q * 4 + lr * 4, i.e. lane l = 16 q + lr, holds M[16 ct + lr][16 kb + 4 q .. + 3]"""
    M = np.full((16 * nct, 16 * nkb), np.nan, f32)
    for ct in range(nct):
        for kb in range(nkb):
            tile = ct * nkb + kb
            for l in range(64):
                q, lr = l >> 4, l & 15
                at = tile * 256 + 16 * q * 4 + lr * 4
                M[16 * ct + lr, 16 * kb + 4 * q:16 * kb + 4 * q + 4] = img[at:at + 4]
    return M


def gates_matrix(K, kx, nkb):
    """the [x | m] concatenation of the gates product over a TF-layout kernel K [(I + P)][4H]: per gate a block of 16 ceil(H / 16) rows,
    row = cell, columns = x padded to kx, then m"""
    ncb = (H + 15) // 16
    M = np.zeros((4 * 16 * ncb, 16 * nkb), f32)
    for g in range(4):
        blk = K[:, g * H:(g + 1) * H].T                                   # [cell][row of K]
        if kx:
            M[g * 16 * ncb:g * 16 * ncb + H, :I] = blk[:, :I]
        M[g * 16 * ncb:g * 16 * ncb + H, kx:kx + P] = blk[:, I:I + P]
    return M


def swizzle_forms():
    """(name, source, job, logical matrix by slicing) of the four forms Model::refresh_swizzles builds"""
    g = rng(11)
    K = g.standard_normal((I + P, 4 * H)).astype(f32)
    Wp = g.standard_normal((H, LDP)).astype(f32)
    ncb, kb4, kbH = (H + 15) // 16, (4 * H + 15) // 16, ((H + 3) // 4 * 4 + 15) // 16
    forms = []
    nkb = (LDI + P + 15) // 16
    forms.append(("Wg_full", K, dict(ld=4 * H, gates=4, H=H, C=0, c0=0, K1=0, I=I, P=P, kx=LDI, nct=4 * ncb, nkb=nkb), gates_matrix(K, LDI, nkb)))
    nkb = (P + 15) // 16
    forms.append(("Wg_h", K, dict(ld=4 * H, gates=4, H=H, C=0, c0=0, K1=0, I=I, P=P, kx=0, nct=4 * ncb, nkb=nkb), gates_matrix(K, 0, nkb)))
    for name, C, c0 in (("Kb_full", I + P, 0), ("Kb_rec", P, I)):
        nct = (C + 15) // 16
        M = np.zeros((16 * nct, 16 * kb4), f32)
        M[:C, :4 * H] = K[c0:c0 + C]
        forms.append((name, K, dict(ld=4 * H, gates=0, H=0, C=C, c0=c0, K1=4 * H, I=0, P=0, kx=0, nct=nct, nkb=kb4), M))
    nct = (P + 15) // 16
    M = np.zeros((16 * nct, 16 * kbH), f32)
    M[:P, :H] = Wp[:, :P].T                                               # M[p][k] = Wp[k][p]
    forms.append(("WpT_sw", Wp, dict(ld=LDP, gates=1, H=P, C=0, c0=0, K1=0, I=H, P=0, kx=16 * kbH, nct=nct, nkb=kbH), M))
    return forms


@pytest.mark.parametrize("name", ["Wg_full", "Wg_h", "Kb_full", "Kb_rec", "WpT_sw"])
def test_swizzle_ref_read_back_lane_by_lane(name):
    (_, src, job, M), = [f for f in swizzle_forms() if f[0] == name]
    n = job["nct"] * job["nkb"] * 256
    img = R.swizzle_ref(src, job, np.full(n + 8, 7.0, f32))
    assert np.all(img[n:] == 7.0)
    got = read_back(img, job["nct"], job["nkb"])
    assert got.shape == M.shape and np.count_nonzero(M) > 0
    assert np.array_equal(got.view(np.uint32), M.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the row builders
@pytest.mark.parametrize("with_real", [0, 1])
@pytest.mark.parametrize("noise", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_build_d_input_against_concatenate(with_real, noise):
    B, T, D, ld = 3, 4, 5, 8
    g = rng(5)
    lab, y = g.standard_normal((T, B, ld)).astype(f32), g.standard_normal((T, B, ld)).astype(f32)
    nr = g.standard_normal((B, D)).astype(f32) if noise[0] else None
    nf = g.standard_normal((B, D)).astype(f32) if noise[1] else None
    Nd = 2 * B if with_real else B
    out = R.build_d_input_ref(lab, y, nr, nf, B, T, D, ld, with_real, np.full(T * Nd * ld + 4, 7.0, f32))
    zero = np.zeros((B, D), f32)
    fake = y[:, :, :D] + (zero if nf is None else nf)[None]
    want = np.concatenate([lab[:, :, :D] + (zero if nr is None else nr)[None], fake], axis=1) if with_real else fake
    got = out[:T * Nd * ld].reshape(T, Nd, ld)
    assert np.array_equal(got[:, :, :D], want.astype(f32))
    assert np.all(got[:, :, D:] == 7.0) and np.all(out[T * Nd * ld:] == 7.0)


def test_add_noise_rows_and_null_noise_sign():
    B, T, D, ld, Ns, row0 = 2, 3, 5, 8, 6, 3
    g = rng(6)
    src, noise = g.standard_normal((T, B, ld)).astype(f32), g.standard_normal((B, D)).astype(f32)
    src[0, 0, 0] = -0.0
    out = R.add_noise_rows_ref(src, noise, B, T, D, ld, Ns, row0, np.full(T * Ns * ld, 7.0, f32)).reshape(T, Ns, ld)
    assert np.array_equal(out[:, row0:row0 + B, :D], src[:, :, :D] + noise[None])
    out[:, row0:row0 + B, :D] = 7.0
    assert np.all(out == 7.0)
    out = R.add_noise_rows_ref(src, None, B, T, D, ld, Ns, row0, np.full(T * Ns * ld, 7.0, f32)).reshape(T, Ns, ld)
    assert out[0, row0, 0] == 0.0 and not np.signbit(out[0, row0, 0])             # -0.0 + +0.f
    assert np.array_equal(out[:, row0:row0 + B, 1:D], src[:, :, 1:D])


@pytest.mark.parametrize("dim", [0, 44])
def test_build_joint_against_concatenate(dim):
    ldx, off, ldt, Dt, ldj, row0, Rn = 52, 3, 40, 40, 88, 5, 5
    g = rng(7)
    x, tail = g.standard_normal((Rn, ldx)).astype(f32), g.standard_normal((Rn, ldt)).astype(f32)
    out = R.build_joint_ref(x if dim else None, ldx, off, dim, tail, ldt, Dt, ldj, row0, Rn, np.full((row0 + Rn + 2) * ldj, 7.0, f32))
    out = out.reshape(-1, ldj)
    assert np.array_equal(out[row0:row0 + Rn, :dim + Dt], np.concatenate([x[:, off:off + dim], tail[:, :Dt]], axis=1))
    out[row0:row0 + Rn, :dim + Dt] = 7.0
    assert np.all(out == 7.0)


def test_pack_unpack_and_transpose_against_numpy():
    B, T, D, ld = 3, 5, 7, 8
    g = rng(8)
    x = g.standard_normal((B, T, D)).astype(f32)
    tm = R.pack_tm_ref(x, B, T, D, ld, np.full(T * B * ld, 7.0, f32)).reshape(T, B, ld)
    assert np.array_equal(tm[:, :, :D], x.transpose(1, 0, 2)) and np.all(tm[:, :, D:] == 7.0)
    back = R.unpack_bm_ref(tm, ld, B, T, D, 2, np.full(B * T * D, 7.0, f32)).reshape(B, T, D)
    assert np.array_equal(back[:2], x[:2]) and np.all(back[2] == 7.0)
    a = g.standard_normal((7, 13)).astype(f32)
    t = R.transpose_ref(a, 13, 9, 7, 10, np.full(10 * 9, 7.0, f32)).reshape(10, 9)
    assert np.array_equal(t[:, :7], a[:, :10].T) and np.all(t[:, 7:] == 7.0)
