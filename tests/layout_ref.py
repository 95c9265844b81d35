"""NumPy references of the layout, staging and weight-copy kernels behind rsrgan_op_layout (csrc/kernels.hip), one function per op, written
from the launchers' comments in csrc/kernels.h and the reference project's semantics -- plain indexed loops and slicing.  Each takes the
op's arguments plus the PREVIOUS contents of every destination (flat fp32 arrays, as the kernels see them) and returns the whole expected
destination, so that "left untouched" is part of the expectation.  Every op is a copy, one fp32 add, or (col2im) one fp32 sum in a fixed
order: the results are meant to be compared bit for bit.  tests/test_layout_ref.py checks these functions against independent
formulations; tests/test_gpu_layout_ops.py checks the kernels against them."""
import numpy as np

f32 = np.float32
ZERO = f32(0.0)


def _flat(a):
    return np.ascontiguousarray(a, dtype=f32).reshape(-1)


# ------------------------------------------------------------------------------------------------ batch-major <-> time-major
def pack_tm_ref(src, B, T, D, ld, dst):
    """[B][T][D] -> [T][B][ld]; columns [D, ld) are not written"""
    out = _flat(dst).copy()
    s = _flat(src)
    for b in range(B):
        for t in range(T):
            o = (t * B + b) * ld
            out[o:o + D] = s[(b * T + t) * D:(b * T + t + 1) * D]
    return out


def unpack_bm_ref(src, ld, B, T, D, Bt, dst):
    """[T][B][ld] -> [Bt or B][T][D]: the source's row stride stays B"""
    out = _flat(dst).copy()
    s = _flat(src)
    for b in range(Bt if Bt > 0 else B):
        for t in range(T):
            o = (t * B + b) * ld
            out[(b * T + t) * D:(b * T + t + 1) * D] = s[o:o + D]
    return out


def stage_inputs_ref(packs, copies, B, T, Bt):
    """packs: up to two (src [Bt or B][T][D] or None, D, ld, dst [T][B][ld]); copies: up to four (src or None, n words, dst), any 32-bit
    type.  -> (the packs' expected destinations, the copies'); a slot without a source keeps its destination"""
    rows = Bt if Bt > 0 else B
    po, co = [], []
    for src, D, ld, dst in packs:
        out = _flat(dst).copy()
        if src is not None:
            s = _flat(src)
            for b in range(rows):                 # rows [Bt, B) of every frame are not written
                for t in range(T):
                    o = (t * B + b) * ld
                    out[o:o + D] = s[(b * T + t) * D:(b * T + t + 1) * D]
        po.append(out)
    for src, n, dst in copies:
        out = np.array(dst).reshape(-1).copy()
        if src is not None:
            out.view(np.uint32)[:n] = np.ascontiguousarray(src).reshape(-1).view(np.uint32)[:n]
        co.append(out)
    return po, co


# ------------------------------------------------------------------------------------------------ the discriminator's input
def _noise(n, B, D):
    """[B][D] broadcast over time; a null noise adds +0.f (csrc/kernels.h)"""
    return np.zeros((B, D), dtype=f32) if n is None else _flat(n)[:B * D].reshape(B, D)


def build_d_input_ref(lab, y, nr, nf, B, T, D, ld, with_real, dst):
    """rows [0, B) of every frame = labels + noise_r (with_real only), the next B rows = y + noise_f; xd [T][Nd][ld], Nd = 2B or B"""
    Nd = 2 * B if with_real else B
    out = _flat(dst).copy()
    o = out[:T * Nd * ld].reshape(T, Nd, ld)
    yy = _flat(y)[:T * B * ld].reshape(T, B, ld)
    r0 = 0
    if with_real:
        ll = _flat(lab)[:T * B * ld].reshape(T, B, ld)
        o[:, :B, :D] = (ll[:, :, :D] + _noise(nr, B, D)[None]).astype(f32)
        r0 = B
    o[:, r0:r0 + B, :D] = (yy[:, :, :D] + _noise(nf, B, D)[None]).astype(f32)
    return out


def add_noise_rows_ref(src, noise, B, T, D, ld, Ns, row0, dst):
    """dst[t][row0 + b] = src[t][b] + noise[b]; dst has Ns rows per frame, the others are not written"""
    out = _flat(dst).copy()
    o = out[:T * Ns * ld].reshape(T, Ns, ld)
    s = _flat(src)[:T * B * ld].reshape(T, B, ld)
    o[:, row0:row0 + B, :D] = (s[:, :, :D] + _noise(noise, B, D)[None]).astype(f32)
    return out


def build_joint_ref(x, ldx, off, dim, tail, ldt, Dt, ldj, row0, R, dst):
    """joint[row0 + r] = concat(x[r][off : off + dim], tail[r][0 : Dt])"""
    out = _flat(dst).copy()
    t = _flat(tail)
    for r in range(R):
        o = (row0 + r) * ldj
        if dim > 0:
            out[o:o + dim] = _flat(x)[r * ldx + off:r * ldx + off + dim]
        out[o + dim:o + dim + Dt] = t[r * ldt:r * ldt + Dt]
    return out


def slice_cols_ref(src, lds, off, ldd, R, C, dst):
    """dst[r][0 : C] = src[r][off : off + C]"""
    out = _flat(dst).copy()
    s = _flat(src)
    for r in range(R):
        out[r * ldd:r * ldd + C] = s[r * lds + off:r * lds + off + C]
    return out


# ------------------------------------------------------------------------------------------------ weight copies
def transpose_ref(src, lds, ldd, R, C, dst):
    """dst[c][r] = src[r][c]"""
    out = _flat(dst).copy()
    s = _flat(src)
    for c in range(C):
        for r in range(R):
            out[c * ldd + r] = s[r * lds + c]
    return out


def swizzle_logical(src, job):
    """the logical matrix M [16 nct][16 nkb] of csrc/kernels.h's SwizzleJob comment, zero outside the source.  job: dict of the struct's
    fields (ld, gates, H, C, c0, K1, I, P, kx, nct, nkb)"""
    j = job
    s = _flat(src)
    M = np.zeros((16 * j["nct"], 16 * j["nkb"]), dtype=f32)
    for c in range(M.shape[0]):
        for k in range(M.shape[1]):
            if j["gates"] == 0:                   # rows of a k-contiguous matrix
                if c < j["C"] and k < j["K1"]:
                    M[c, k] = s[(j["c0"] + c) * j["ld"] + k]
                continue
            ncb = (j["H"] + 15) // 16              # c = g * 16 ncb + cell; the source column is g * H + cell
            g, cell = divmod(c, 16 * ncb)
            if g >= j["gates"] or cell >= j["H"]:
                continue
            if k < j["kx"]:
                row = k if k < j["I"] else None
            else:
                row = j["I"] + (k - j["kx"]) if k - j["kx"] < j["P"] else None
            if row is not None:
                M[c, k] = s[row * j["ld"] + g * j["H"] + cell]
    return M


def swizzle_ref(src, job, dst):
    """the tiled image of M: tile (ct, kb) = the 16 columns x 16 k of one MFMA k-block as [q][lr][4], tiles of one column block
    contiguous along k; the float4 of lane l = 16 q + lr holds M[16 ct + lr][16 kb + 4 q .. + 3].  Exactly nct * nkb * 256 floats"""
    nct, nkb = job["nct"], job["nkb"]
    M = swizzle_logical(src, job)
    out = _flat(dst).copy()
    out[:nct * nkb * 256] = M.reshape(nct, 16, nkb, 4, 4).transpose(0, 2, 3, 1, 4).reshape(-1)       # (ct, lr, kb, q, u) -> (ct, kb, q, lr, u)
    return out


# ------------------------------------------------------------------------------------------------ R-CED's patch matrix
def _frames(src, row_stride, ldc, C, S, W, R):
    """x[r][h][w][c] = src[r * row_stride + (h * W + w) * ldc + c]"""
    s = _flat(src)
    x = np.empty((R, S, W, C), dtype=f32)
    for r in range(R):
        for h in range(S):
            for w in range(W):
                o = r * row_stride + (h * W + w) * ldc
                x[r, h, w] = s[o:o + C]
    return x


def im2col_ref(src, row_stride, ldc, C, S, W, kh, kw, ldk, M, dst):
    """col[p][(dh * kw + dw) * C + c] = x[r][h + dh - pt][w + dw - pl][c] (0 outside the frame), p = (r * S + h) * W + w; TF SAME: pt =
    (kh - 1) // 2, pl = (kw - 1) // 2 leading zeros, the extra element of an even extent trails.  Columns [K, ldk) are written as 0"""
    R = M // (S * W)
    pt, pl = (kh - 1) // 2, (kw - 1) // 2
    x = _frames(src, row_stride, ldc, C, S, W, R)
    out = _flat(dst).copy()
    col = out[:M * ldk].reshape(R, S, W, ldk)
    col[...] = ZERO
    for dh in range(kh):
        for dw in range(kw):
            k = (dh * kw + dw) * C
            for h in range(S):
                for w in range(W):
                    hh, ww = h + dh - pt, w + dw - pl
                    if 0 <= hh < S and 0 <= ww < W:
                        col[:, h, w, k:k + C] = x[:, hh, ww]
    return out


def col2im_ref(dcol, ldk, C, S, W, kh, kw, ldc, M, dst):
    """the adjoint of im2col_ref as a gather: dst[p][c] = the fp32 sum, dh outer and dw inner from +0.0, of dcol[p'][(dh * kw + dw) * C + c]
    over the positions p' whose patch element (dh, dw) is p.  dst [M][ldc], columns [C, ldc) written as +0.0"""
    R = M // (S * W)
    pt, pl = (kh - 1) // 2, (kw - 1) // 2
    d = _flat(dcol)[:M * ldk].reshape(R, S, W, ldk)
    acc = np.zeros((R, S, W, ldc), dtype=f32)
    for dh in range(kh):
        for dw in range(kw):
            k = (dh * kw + dw) * C
            for h in range(S):
                for w in range(W):
                    ho, wo = h - dh + pt, w - dw + pl          # the output position whose patch element (dh, dw) is (h, w)
                    if 0 <= ho < S and 0 <= wo < W:
                        acc[:, h, w, :C] = (acc[:, h, w, :C] + d[:, ho, wo, k:k + C]).astype(f32)
    out = _flat(dst).copy()
    out[:M * ldc] = acc.reshape(-1)
    return out


def expand_c4_ref(src, ld_src, n, rows, dst):
    """[rows][ld_src] rows of n scalars -> [rows * n][4] = (value, 0, 0, 0)"""
    out = _flat(dst).copy()
    s = _flat(src)
    o = out[:rows * n * 4].reshape(rows, n, 4)
    for r in range(rows):
        o[r, :, 0] = s[r * ld_src:r * ld_src + n]
        o[r, :, 1:] = ZERO
    return out


# ------------------------------------------------------------------------------------------------ carried state, windows
def gstate_ref(state, layers, SF, rows, direction, slot, mask):
    """state [rows][SF]: a row = layer 0's c [H], layer 0's m [P], layer 1's c, ... at the layers' offsets.  layers: (c, mst, H, P, ldP, off)
    with c [..][H] and mst [..][ldP] (None where ldP == 0); `slot` is a row offset into both.  0: state -> slot (mst's columns [P, ldP)
    zero); 1: slot -> state (the valid columns only); 2: zero the whole state row where mask is non-zero (mask None: every row).
    -> (state, [c], [mst]) as expected afterwards"""
    st = _flat(state).copy()
    cs = [_flat(L[0]).copy() for L in layers]
    ms = [None if L[1] is None else _flat(L[1]).copy() for L in layers]
    for row in range(rows):
        if direction == 2:
            if mask is None or mask[row] != 0:
                st[row * SF:(row + 1) * SF] = ZERO
            continue
        for l, (_, _, H, P, ldP, off) in enumerate(layers):
            sc = row * SF + off
            co, mo = (slot + row) * H, (slot + row) * ldP
            if direction == 0:
                cs[l][co:co + H] = st[sc:sc + H]
                if ldP > 0:
                    ms[l][mo:mo + P] = st[sc + H:sc + H + P]
                    ms[l][mo + P:mo + ldP] = ZERO
            else:
                st[sc:sc + H] = cs[l][co:co + H]
                if P > 0:
                    st[sc + H:sc + H + P] = ms[l][mo:mo + P]
    return st, cs, ms


def window_len_ref(length, n, t0, Tw, dst):
    """dst[b] = clamp(len[b] - t0, 0, Tw), int32"""
    out = np.array(dst, dtype=np.int32).reshape(-1).copy()
    for b in range(n):
        out[b] = min(max(int(length[b]) - t0, 0), Tw)
    return out


# ------------------------------------------------------------------------------------------------ buffers
def zero_many_ref(lens, dsts):
    outs = []
    for n, dst in zip(lens, dsts):
        out = _flat(dst).copy()
        out[:n] = ZERO                             # +0.0
        outs.append(out)
    return outs


def fill_ref(n, v, dst):
    out = _flat(dst).copy()
    out[:n] = f32(v)
    return out


def copy_f_ref(src, n, dst):
    out = _flat(dst).copy()
    out[:n] = _flat(src)[:n]
    return out


def pad_copy_ref(dense, padded, rows, cols, ld, to_padded):
    """dense [rows][cols] <-> padded [rows][ld]; -> (dense, padded) as expected afterwards: the source unchanged, the destination's
    padding columns untouched"""
    dn, pd = _flat(dense).copy(), _flat(padded).copy()
    for r in range(rows):
        if to_padded:
            pd[r * ld:r * ld + cols] = dn[r * cols:(r + 1) * cols]
        else:
            dn[r * cols:(r + 1) * cols] = pd[r * ld:r * ld + cols]
    return dn, pd
