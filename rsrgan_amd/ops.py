"""OpEntries -- the unit-test operator entries of the C ABI (include/rsrgan.h rsrgan_op_*, csrc/capi_ops.cpp): the library's own host
launch code on caller-owned device tensors.  No handle: a loaded library, a device and the current stream are all they need, so the
operator tests and tools/gemm_bench.py build an OpEntries() and no model.  FrontEnd (frontend.py), and through it HipEngine, derives from it."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import (BN_PLAN_FIELDS, BN_ROUTES, CONV_FAMILIES, CONV_FWD_BRANCHES, CONV_PLAN_FIELDS, CONV_WGRAD_BRANCHES, GEMM_CLASSES,
                   GEMM_PLAN_FIELDS, LAYOUT_OPS, LSTM_STEP_FORMS, LSTM_STEP_OPS, LSTM_STEP_PLAN_FIELDS, SEGAN_OPS, SEGAN_PLAN_FIELDS, STEP_ELEM_OPS,
                   UPDATE_OPS, check, ptr_table)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class OpEntries:
    def __init__(self, device: Optional[torch.device] = None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.RsrganError("no GPU visible: rsrgan_amd runs only on MI355X (gfx950); there is no CPU fallback")
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(self.device)

    def _stream(self, stream=None):
        """the entries' stream argument: `stream`, or the current one"""
        return C.c_void_p((torch.cuda.current_stream(self.device) if stream is None else stream).cuda_stream)

    @staticmethod
    def _table(ts):
        return None if ts is None else ptr_table([None if t is None else t.data_ptr() for t in ts])

    @staticmethod
    def _tables(ptrs, dims, fl=()):
        """the (ptrs, dims, fl) host tables of a table-form entry: tensors or None, ints (any 64-bit value wraps to int64), floats"""
        pt = (C.c_void_p * max(len(ptrs), 1))(*[None if t is None else t.data_ptr() for t in ptrs])
        dm = (C.c_int64 * max(len(dims), 1))(*[(int(v) + 2 ** 63) % 2 ** 64 - 2 ** 63 for v in dims])
        ff = (C.c_float * max(len(fl), 1))(*[float(v) for v in fl])
        return pt, dm, ff

    def launch_floor(self, n=400, mode=1):
        """us per dependent launch of a replayed graph of n launches (mode 0: empty kernels, 1: one dependent operand round trip)"""
        us = C.c_double()
        check(self.lib.rsrgan_op_launch_floor(n, mode, C.byref(us), self._stream()))
        return us.value

    # -- TensorBoard histograms on the device (include/rsrgan.h rsrgan_hist, csrc/hist.hip): a product entry that needs no handle ------
    HIST_MAX_TENSORS = 16          # csrc/kernels.h: tensors per call of the entry

    def hist_limits(self):
        """the bucket limits the kernel uses (rsrgan_hist_limits) as a float64 array: summary._LIMITS bit for bit"""
        return _lib.hist_limits()

    def hist(self, tensors) -> torch.Tensor:
        """[len(tensors), 5 + NL] float64 device tensor: one histogram record (summary.histogram_stats) per float32 device tensor, on
        the current stream.  A tensor is read where it lies if it is contiguous, or 2-D with unit column stride (a view with a leading
        dimension: logits[:, :1] of a [rows, 4] buffer); anything else is made contiguous first."""
        views, keep = [], []
        for t in tensors:
            if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.float32:
                raise ValueError("hist: float32 tensors on %s are needed" % (self.device,))
            if t.numel() == 0:
                views.append((None, 0, 0, 0))
            elif t.is_contiguous():
                views.append((t, 1, t.numel(), t.numel()))
            elif t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
                views.append((t, t.shape[0], t.shape[1], t.stride(0)))
            else:
                c = t.contiguous()
                keep.append(c)
                views.append((c, 1, c.numel(), c.numel()))
        nl = len(self.hist_limits())
        out = torch.empty(len(views), 5 + nl, dtype=torch.float64, device=self.device)
        for i in range(0, len(views), self.HIST_MAX_TENSORS):
            part = views[i:i + self.HIST_MAX_TENSORS]
            dims = (C.c_int64 * (3 * len(part)))(*[int(v) for _, r, c, ld in part for v in (r, c, ld)])
            check(self.lib.rsrgan_hist(len(part), self._table([v[0] for v in part]), dims, _ptr(out[i:]), self._stream()))
        self._keep_hist = (tensors, keep)          # borrowed until the stream has consumed them
        return out

    def op_gemm(self, A, a_kc, B, b_kc, C_, M, N, K, bias=None, act=0, alpha=0.3, accumulate=False):
        check(self.lib.rsrgan_op_gemm(_ptr(A), A.stride(0), 1 if a_kc else 0, _ptr(B), B.stride(0), 1 if b_kc else 0,
                                      _ptr(C_), C_.stride(0), M, N, K, _ptr(bias), act, alpha, 1 if accumulate else 0,
                                      self._stream()))

    def op_gemm2(self, A, a_kc, B, b_kc, C_, M, N, K, A2=None, M1=0, lda=None, lda2=None, bias=None, act=0, alpha=0.3,
                 accumulate=False, row_map=None, workers=0, force_cfg=-1):
        """row_map = (rows_per, outer, inner) in floats: a window view of A (then lda is unused)"""
        rp, outer, inner = row_map if row_map else (0, 0, 0)
        check(self.lib.rsrgan_op_gemm2(_ptr(A), A.stride(0) if lda is None else lda, 1 if a_kc else 0, _ptr(A2),
                                       0 if A2 is None else (A2.stride(0) if lda2 is None else lda2), M1, _ptr(B), B.stride(0),
                                       1 if b_kc else 0, _ptr(C_), C_.stride(0), M, N, K, _ptr(bias), act, alpha,
                                       1 if accumulate else 0, rp, outer, inner, workers, force_cfg, self._stream()))

    def op_gemm_batch(self, As, A2s, Bs, Cs, M, N, K, M1=0, accumulate=False, workers=0) -> bool:
        """True: launched; False: not applicable (nothing ran, the caller launches the products one by one)"""
        rc = self.lib.rsrgan_op_gemm_batch(len(As), self._table(As), As[0].stride(0), self._table(A2s),
                                           A2s[0].stride(0) if A2s else 0, M1, self._table(Bs), Bs[0].stride(0), self._table(Cs),
                                           Cs[0].stride(0), M, N, K, 1 if accumulate else 0, workers, self._stream())
        if rc == 1:
            return False
        check(rc)
        return True

    def op_gemm16_batch(self, As, A2s, Bs, Cs, M, N, K, M1=0, accumulate=False):
        check(self.lib.rsrgan_op_gemm16_batch(len(As), self._table(As), As[0].stride(0), self._table(A2s),
                                              A2s[0].stride(0) if A2s else 0, M1, self._table(Bs), Bs[0].stride(0), self._table(Cs),
                                              Cs[0].stride(0), M, N, K, 1 if accumulate else 0, self._stream()))

    def op_gemm_last_plan(self) -> dict:
        out = (C.c_int32 * 8)()
        check(self.lib.rsrgan_op_gemm_last_plan(out))
        d = dict(zip(GEMM_PLAN_FIELDS, list(out)))
        d["cls"] = GEMM_CLASSES[d["cls"]]
        return d

    def op_conv_supported(self, C_, N, S, W, fw):
        """(conv_fwd_supported, conv_wgrad_supported) of csrc/conv.hip"""
        rc = self.lib.rsrgan_op_conv_supported(C_, N, S, W, fw)
        if rc < 0:
            check(rc)
        return bool(rc & 1), bool(rc & 2)

    def op_conv_ws_floats(self, C_, R_max, S, W, fw) -> int:
        n = self.lib.rsrgan_op_conv_ws_floats(C_, R_max, S, W, fw)
        if n < 0:
            check(int(n))
        return int(n)

    def op_conv_fwd(self, x, C_, F, out, N, R, S, W, fw, flip=False, bias=None, relu=False, mask=None) -> bool:
        """x [R*S*W][ldc_in], F as the model stores the layer's filter, out [R*S*W][ldc_out]; False: not applicable (nothing ran)"""
        rc = self.lib.rsrgan_op_conv_fwd(_ptr(x), x.stride(0), C_, _ptr(F), F.stride(0), 1 if flip else 0, _ptr(bias), 1 if relu else 0,
                                         _ptr(mask), _ptr(out), out.stride(0), N, R, S, W, fw, self._stream())
        if rc == 1:
            return False
        check(rc)
        return True

    def op_conv_wgrad(self, x, C_, d, N, dW, ws, R_max, R, S, W, fw, db=None, ws_floats=None) -> bool:
        rc = self.lib.rsrgan_op_conv_wgrad(_ptr(x), x.stride(0), C_, _ptr(d), d.stride(0), N, _ptr(dW), dW.stride(0), _ptr(db), _ptr(ws),
                                           ws.numel() if ws_floats is None else ws_floats, R_max, R, S, W, fw, self._stream())
        if rc == 1:
            return False
        check(rc)
        return True

    def op_conv_last_plan(self) -> list:
        """one dict per launch of the calling thread's last op_conv_fwd / op_conv_wgrad (empty: not applicable)"""
        out = (C.c_int32 * 40)()
        check(self.lib.rsrgan_op_conv_last_plan(out))
        plans = []
        for i in range(out[0]):
            d = dict(zip(CONV_PLAN_FIELDS, out[1 + 19 * i:1 + 19 * (i + 1)]))
            d["family"] = CONV_FAMILIES[d["family"]]
            d["branch"] = (CONV_FWD_BRANCHES if d["family"] in ("fwd", "fwd4") else CONV_WGRAD_BRANCHES)[d["branch"]]
            plans.append(d)
        return plans

    def op_bn_forward(self, z, y, rows, cols, bn_vars, stat, scratch, calls=1, training=True, relu=True, scratch_floats=None):
        """z, y [calls * rows][ld]; bn_vars: the eight tensors in _lib.BN_VARS order; stat [calls * 6][ldc]"""
        check(self.lib.rsrgan_op_bn_forward(_ptr(z), z.stride(0), _ptr(y), y.stride(0), rows, cols, calls, self._table(bn_vars), _ptr(stat),
                                            stat.stride(0), 1 if training else 0, 1 if relu else 0, _ptr(scratch),
                                            scratch.numel() if scratch_floats is None else scratch_floats, self._stream()))

    def op_bn_backward(self, dy, y, z, rows, cols, stat, sums, scratch, dbeta=None, dgamma=None, calls=1, accumulate=False, relu=True,
                       scratch_floats=None):
        """dy [calls * rows][ldd] is overwritten by dz; sums [2][ldc]"""
        check(self.lib.rsrgan_op_bn_backward(_ptr(dy), dy.stride(0), _ptr(y), y.stride(0), _ptr(z), z.stride(0), rows, cols, calls, _ptr(stat),
                                             stat.stride(0), _ptr(dbeta), _ptr(dgamma), 1 if accumulate else 0, 1 if relu else 0, _ptr(sums),
                                             _ptr(scratch), scratch.numel() if scratch_floats is None else scratch_floats, self._stream()))

    def op_bn_seq_forward(self, z, y, rows, cols, bn_vars, stat, scratch, alpha=0.3, Bp=0, Bt=0, training=True, relu=True, scratch_floats=None):
        """the sequence form: leaky-ReLU of slope alpha; row r counts iff Bp == 0 or r % Bp < Bt (include/rsrgan.h)"""
        check(self.lib.rsrgan_op_bn_seq_forward(_ptr(z), z.stride(0), _ptr(y), y.stride(0), rows, cols, self._table(bn_vars), _ptr(stat),
                                                stat.stride(0), 1 if training else 0, 1 if relu else 0, alpha, Bp, Bt, _ptr(scratch),
                                                scratch.numel() if scratch_floats is None else scratch_floats, self._stream()))

    def op_bn_seq_backward(self, dy, y, z, rows, cols, stat, sums, scratch, alpha=0.3, Bp=0, Bt=0, dbeta=None, dgamma=None, accumulate=False,
                           relu=True, scratch_floats=None):
        """dy [rows][ldd] is overwritten by dz (exact zeros on the rows that do not count); sums [2][ldc]"""
        check(self.lib.rsrgan_op_bn_seq_backward(_ptr(dy), dy.stride(0), _ptr(y), y.stride(0), _ptr(z), z.stride(0), rows, cols, _ptr(stat),
                                                 stat.stride(0), _ptr(dbeta), _ptr(dgamma), 1 if accumulate else 0, 1 if relu else 0, alpha,
                                                 Bp, Bt, _ptr(sums), _ptr(scratch),
                                                 scratch.numel() if scratch_floats is None else scratch_floats, self._stream()))

    def op_bn_commit(self, entries, single=False):
        """entries: (bn_vars, stat, cols, times0, times1) per layer; single: k_bn_commit instead of k_bn_commit_many"""
        dims = []
        for _, st, cols, t0, t1 in entries:
            dims += [cols, st.stride(0), t0, t1]
        check(self.lib.rsrgan_op_bn_commit(len(entries), self._table([t for e in entries for t in e[0]]), self._table([e[1] for e in entries]),
                                           (C.c_int32 * len(dims))(*dims), 1 if single else 0, self._stream()))

    def op_bn_last_plan(self) -> dict:
        out = (C.c_int32 * 16)()
        check(self.lib.rsrgan_op_bn_last_plan(out))
        d = dict(zip(BN_PLAN_FIELDS, list(out)))
        d["route"] = BN_ROUTES[d["route"]]
        return d

    def op_segan(self, family, op, ptrs, dims, fl=()):
        """rsrgan_op_segan_<family>, op by name (_lib.SEGAN_OPS); ptrs: tensors or None, dims: ints, fl: floats (include/rsrgan.h)"""
        check(getattr(self.lib, "rsrgan_op_segan_" + family)(SEGAN_OPS[family].index(op), *self._tables(ptrs, dims, fl), self._stream()))

    def op_segan_sizes(self, kind, dims) -> list:
        out = (C.c_int64 * 12)()
        check(self.lib.rsrgan_op_segan_sizes(kind, (C.c_int64 * len(dims))(*[int(v) for v in dims]), out))
        return list(out)

    def op_segan_last_plan(self) -> dict:
        out = (C.c_int32 * 8)()
        check(self.lib.rsrgan_op_segan_last_plan(out))
        return dict(zip(SEGAN_PLAN_FIELDS, list(out)))

    def op_chunks(self, tensors) -> dict:
        """the model's chunk table of tensors [(float offset, floats, l2 flag)] (no device)"""
        flat = [int(v) for t in tensors for v in t]
        tt = (C.c_int64 * len(flat))(*flat)
        nc = C.c_int32()
        check(self.lib.rsrgan_op_chunks(tt, len(tensors), None, 0, C.byref(nc)))
        n = 3 * nc.value + 3 * len(tensors)
        out = (C.c_int32 * n)()
        check(self.lib.rsrgan_op_chunks(tt, len(tensors), out, n, C.byref(nc)))
        o, res, at = list(out), {}, 0
        for name, cnt in (("tensor", nc.value), ("off", nc.value), ("len", nc.value), ("t_first", len(tensors)), ("t_count", len(tensors)),
                          ("t_l2", len(tensors))):
            res[name] = o[at:at + cnt]
            at += cnt
        return res

    def op_update(self, op, tensors, ptrs, buf_floats, partial_floats, extra=(), src=()):
        """rsrgan_op_update, op by name (_lib.UPDATE_OPS); tensors [(offset, floats, l2)], extra: the op's own dims, src: dw_reduce's offsets"""
        dims = [len(tensors), buf_floats, partial_floats] + (list(extra) + [0, 0, 0])[:3] + [v for t in tensors for v in t] + list(src)
        pt, dm, _ = self._tables(ptrs, dims)
        check(self.lib.rsrgan_op_update(UPDATE_OPS.index(op), pt, dm, None, self._stream()))

    def op_step_elem(self, op, ptrs, dims=(), fl=()):
        """rsrgan_op_step_elem, op by name (_lib.STEP_ELEM_OPS); ptrs: tensors or None, dims: ints (a dropout key: any 64-bit value), fl: floats"""
        check(self.lib.rsrgan_op_step_elem(STEP_ELEM_OPS.index(op), *self._tables(ptrs, dims, fl), self._stream()))

    def op_layout(self, op, ptrs, dims=(), fl=()):
        """rsrgan_op_layout, op by name (_lib.LAYOUT_OPS); ptrs: tensors or None, dims: ints, fl: floats (include/rsrgan.h)"""
        check(self.lib.rsrgan_op_layout(LAYOUT_OPS.index(op), *self._tables(ptrs, dims, fl), self._stream()))

    def op_lstm_step(self, op, ptrs, dims, fl=()):
        """rsrgan_op_lstm_step, op by name (_lib.LSTM_STEP_OPS): one launch of n jobs; ptrs: one group of tensors or None per job, dims: n, then
        one record per job (split-K: then ws and its floats), fl: forget_bias, or keep per job (include/rsrgan.h)"""
        check(self.lib.rsrgan_op_lstm_step(LSTM_STEP_OPS.index(op), *self._tables(ptrs, dims, fl), self._stream()))

    def op_lstm_step_last_plan(self) -> dict:
        out = (C.c_int32 * 16)()
        check(self.lib.rsrgan_op_lstm_step_last_plan(out))
        d = dict(zip(LSTM_STEP_PLAN_FIELDS, list(out)))
        d["form"] = LSTM_STEP_FORMS[d["form"]]
        return d

    def device_status(self) -> int:
        """the handle-free form of HipEngine.device_status: waits for the current stream; 0, or -2 (RSRGAN_ERR_HIP) where a launch or a
        kernel of it failed"""
        try:
            torch.cuda.current_stream(self.device).synchronize()
        except RuntimeError:
            return -2
        return 0

    def op_lstm_colsums(self, dz, cprev, ccur, db, dwi, dwf, dwo, rows, H):
        """lists of nb tensors each: dz [rows][4H], cprev / ccur [rows][H], db [>= 4H], dwi / dwf / dwo [>= H]"""
        check(self.lib.rsrgan_op_lstm_colsums(len(dz), self._table(dz), self._table(cprev), self._table(ccur), self._table(db),
                                              self._table(dwi), self._table(dwf), self._table(dwo), rows, H, self._stream()))

    def op_colsum(self, a, out, rows, cols, b=None, tall=False):
        check(self.lib.rsrgan_op_colsum(_ptr(a), a.stride(0), _ptr(b), 0 if b is None else b.stride(0), _ptr(out), rows, cols,
                                        1 if tall else 0, self._stream()))
