"""HipEngine -- thin Python wrapper over the C ABI (include/rsrgan.h).

PyTorch is only plumbing here: it owns the device buffers that are passed to the library as raw
pointers (Tensor.data_ptr()) and the HIP stream the library enqueues on.  No arithmetic of the
GAN step happens in torch."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import NET_D, NET_G, RsrganCfg, SCALARS, WHAT, check
from .ops import OpEntries, _ptr


class _RawDeviceBuffer:
    """Exposes a device pointer owned by librsrgan_hip through __cuda_array_interface__ so that
    torch can alias it (zero copy) -- needed to all-reduce the gradient buffer with RCCL."""

    def __init__(self, ptr: int, count: int):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f4", "data": (ptr, False),
                                         "version": 2, "strides": None}


class WaveFrontEnd(OpEntries):
    """The waveform front end on the handle-free entries (rsrgan_feat_wave, rsrgan_feat_mfcc): the op wrappers, the per-spec table cache
    and wave_features, on the upload stream.  HipEngine is one; so is a bare WaveFrontEnd(), for callers without a model (io.wave_cmvn,
    tools/mfcc_bench.py)."""

    def upload_stream(self):
        """the stream the feature front end uploads and runs on (featurize, featurize_frames, StreamBank)"""
        us = getattr(self, "_upload_stream", None)
        if us is None:
            us = self._upload_stream = torch.cuda.Stream(self.device)
        return us

    # -- the waveform side (include/rsrgan.h rsrgan_feat_wave, csrc/wave.hip k_feat_wave) -------------------------------------------
    def wave_frames_per_workgroup(self, P=512):
        """the consecutive frames of one utterance a workgroup of k_feat_wave takes (rsrgan_feat_wave_frames)"""
        return int(self.lib.rsrgan_feat_wave_frames(P))

    def op_feat_wave(self, pcm, seg, offsets, B, window, twiddle, out, N=400, S=160, P=512, preemph=0.97, kind=None, n_samples=None,
                     out_rows=None, stream=None):
        """rsrgan_feat_wave on caller-owned device tensors (pcm int16 or float32 [n], seg [B, 2] i64 = (first sample, count), offsets
        [B + 1] i32, window [N] f32, twiddle [P / 2, 2] f32, out [rows, P / 2 + 1] f32), on `stream` (default: the current one).  kind
        defaults to what pcm's dtype says."""
        if kind is None:
            if pcm.dtype not in (torch.int16, torch.float32):
                raise ValueError("op_feat_wave: pcm must be int16 or float32, got %s" % pcm.dtype)
            kind = 0 if pcm.dtype == torch.int16 else 1
        check(self.lib.rsrgan_feat_wave(_ptr(pcm), kind, pcm.numel() if n_samples is None else n_samples, _ptr(seg), _ptr(offsets), B, N, S, P,
                                        preemph, _ptr(window), _ptr(twiddle), _ptr(out), out.shape[0] if out_rows is None else out_rows,
                                        self._stream() if stream is None else C.c_void_p(stream.cuda_stream)))

    def op_feat_mfcc(self, pcm, seg, offsets, B, window, twiddle, mel_seg, mel_w, dct, out, N=400, S=160, P=512, preemph=0.97, M=None, ceps=None,
                     nnz=None, kind=None, n_samples=None, out_rows=None, stream=None):
        """rsrgan_feat_mfcc on caller-owned device tensors (pcm, seg, offsets, window, twiddle as op_feat_wave takes them; mel_seg [M, 3]
        i32, mel_w [nnz] f32, dct [C, M] f32 or None for log-mel output; out [rows, C or M] f32), on `stream` (default: the current one).
        M, ceps (the entry's C) and nnz default to what the tables' shapes say."""
        if kind is None:
            if pcm.dtype not in (torch.int16, torch.float32):
                raise ValueError("op_feat_mfcc: pcm must be int16 or float32, got %s" % pcm.dtype)
            kind = 0 if pcm.dtype == torch.int16 else 1
        M = int(mel_seg.shape[0]) if M is None else M
        ceps = (0 if dct is None else int(dct.shape[0])) if ceps is None else ceps
        check(self.lib.rsrgan_feat_mfcc(_ptr(pcm), kind, pcm.numel() if n_samples is None else n_samples, _ptr(seg), _ptr(offsets), B, N, S, P,
                                        preemph, _ptr(window), _ptr(twiddle), _ptr(mel_seg), _ptr(mel_w), mel_w.numel() if nnz is None else nnz,
                                        M, _ptr(dct), ceps, _ptr(out), out.shape[0] if out_rows is None else out_rows,
                                        self._stream() if stream is None else C.c_void_p(stream.cuda_stream)))

    # -- reverberation (include/rsrgan.h rsrgan_wave_reverb, csrc/reverb.hip) -------------------------------------------------------
    def wave_reverb_work(self, B, n_max, L_max, fft):
        """the bytes of `work` for B utterances of at most n_max samples against at most L_max taps (rsrgan_wave_reverb_work)"""
        need = int(self.lib.rsrgan_wave_reverb_work(B, n_max, L_max, fft))
        if need <= 0:
            raise ValueError("wave_reverb_work: B = %d, n_max = %d, L_max = %d, fft = %d outside the entry's limits" % (B, n_max, L_max, fft))
        return need

    def op_wave_reverb(self, pcm, seg, rir, rir_seg, noise, noise_seg, noise_pow, sel, snr, B, fft, twiddle, out, out_seg, work, gains=None,
                       shift=True, normalize=True, kind=None, stream=None):
        """rsrgan_wave_reverb on caller-owned device tensors: pcm int16 or float32 [n], seg [B, 2] i64; rir f32 [taps], rir_seg [R, 5] i64 =
        (first tap, L, q, e0, e1) (both None: no RIRs); noise f32, noise_seg [V, 2] i64, noise_pow [V] f32 (all None: no noises); sel
        [B, 4] i32 = (rir index, noise index, s, m); snr [B] f32; twiddle [fft, 2] f32 = io.wave.twiddle_table(2 * fft); out f32, out_seg
        [B, 2] i64 = (first, capacity); work uint8 (wave_reverb_work bytes); gains [B, 2] f32 or None.  On `stream` (default: the current
        one); nothing is allocated and nothing waits for the device."""
        if kind is None:
            if pcm.dtype not in (torch.int16, torch.float32):
                raise ValueError("op_wave_reverb: pcm must be int16 or float32, got %s" % pcm.dtype)
            kind = 0 if pcm.dtype == torch.int16 else 1
        R = 0 if rir_seg is None else int(rir_seg.shape[0])
        V = 0 if noise_seg is None else int(noise_seg.shape[0])
        check(self.lib.rsrgan_wave_reverb(_ptr(pcm), kind, pcm.numel(), _ptr(seg), _ptr(rir), 0 if rir is None else rir.numel(), _ptr(rir_seg),
                                          _ptr(noise), 0 if noise is None else noise.numel(), _ptr(noise_seg), _ptr(noise_pow), _ptr(sel),
                                          _ptr(snr), B, R, V, fft, _ptr(twiddle), (1 if shift else 0) | (2 if normalize else 0), _ptr(out),
                                          out.numel(), _ptr(out_seg), _ptr(gains), _ptr(work), work.numel() * work.element_size(),
                                          self._stream() if stream is None else C.c_void_p(stream.cuda_stream)))

    def reverb_bank(self, bank, us=None):
        """the packed tables of an io.reverb.ReverbSim (or anything with its rir / rir_seg / noise / noise_seg / noise_pow members) as
        device tensors (rir, rir_seg, noise, noise_seg, noise_pow; the noise triple None without noises): uploaded once on the upload
        stream and kept with the bank"""
        ent = getattr(bank, "_device_tables", None)
        if ent is None or ent[0] != self.device:
            us = self.upload_stream() if us is None else us
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            with torch.cuda.stream(us):
                tabs = (up(bank.rir), up(bank.rir_seg)) if bank.rir_seg.shape[0] else (None, None)
                tabs += (up(bank.noise), up(bank.noise_seg), up(bank.noise_pow)) if bank.noise_seg.shape[0] else (None, None, None)
            us.synchronize()                                          # (once per bank: later calls may come on other streams)
            ent = bank._device_tables = (self.device, tabs)
        return ent[1]

    def _reverb_twiddle(self, fft, us):
        from .io.wave import twiddle_table
        cache = self.__dict__.setdefault("_reverb_tw", {})
        if fft not in cache:
            with torch.cuda.stream(us):
                cache[fft] = torch.from_numpy(twiddle_table(2 * fft)).to(self.device)
        return cache[fft]

    def simulate(self, wb, plan=None, stream=None, gains=None):
        """io.WaveBatch of clean samples + an io.reverb.ReverbPlan (default: the batch's own) -> (pcm float32 [sum n_out] on the device, its
        segment table int64 [B, 2] on the device, the same table on the host): rsrgan_wave_reverb on `stream` (default: the upload
        stream), the uploads queued there too.  n_out is the utterance's count with the plan's shift, count + L - 1 without.  The
        reverberant audio never exists on the host."""
        plan = wb.plan if plan is None else plan
        if plan is None or len(plan) != len(wb):
            raise ValueError("simulate: the batch of %d utterances needs a plan of as many draws" % len(wb))
        us = self.upload_stream() if stream is None else stream
        bank, spec = plan.bank, plan.spec
        B, counts = len(wb), wb.seg[:, 1].astype(np.int64)
        ri = plan.sel[:, 0].astype(np.int64)
        taps = np.where((ri >= 0) & (ri < bank.rir_seg.shape[0]), bank.rir_seg[np.clip(ri, 0, max(bank.rir_seg.shape[0] - 1, 0)), 1], 1) \
            if bank.rir_seg.shape[0] else np.ones(B, np.int64)
        n_out = counts if spec.shift else np.where(counts > 0, counts + taps - 1, 0)
        first = np.zeros(B, np.int64)
        np.cumsum(n_out[:-1], out=first[1:])
        out_seg = np.stack([first, n_out], 1)
        need = self.wave_reverb_work(B, max(int(counts.max()), 1), int(taps.max()), spec.fft)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device, non_blocking=True)
        with torch.cuda.stream(us):
            rir, rseg, noise, nseg, npow = self.reverb_bank(bank, us)
            tw = self._reverb_twiddle(spec.fft, us)
            pcm, dseg, sel, snr, oseg = up(wb.samples), up(wb.seg), up(plan.sel), up(plan.snr), up(out_seg)
            out = torch.empty(max(int(n_out.sum()), 1), dtype=torch.float32, device=self.device)
            work = torch.empty(need, dtype=torch.uint8, device=self.device)
            self.op_wave_reverb(pcm, dseg, rir, rseg, noise, nseg, npow, sel, snr, B, spec.fft, tw, out, oseg, work, gains, spec.shift,
                                spec.normalize, stream=us)
        return out, oseg, out_seg

    # -- audio out (include/rsrgan.h rsrgan_wave_synth, csrc/synth.hip) ---------------------------------------------------------------
    def wave_synth_chunk(self):
        """the samples of a scan chunk of the synthesis kernels (rsrgan_wave_synth_chunk)"""
        return int(self.lib.rsrgan_wave_synth_chunk())

    def wave_synth_work(self, B, lps_rows, out_samples, N=400):
        """the bytes of `work` for B utterances, lps_rows LPS rows and out_samples output samples (rsrgan_wave_synth_work)"""
        need = int(self.lib.rsrgan_wave_synth_work(B, lps_rows, out_samples, N))
        if need <= 0:
            raise ValueError("wave_synth_work: B = %d, lps_rows = %d, out_samples = %d, N = %d outside the entry's limits" % (
                B, lps_rows, out_samples, N))
        return need

    def op_wave_synth(self, pcm, seg, offsets, lps, B, window, twiddle, out, out_seg, work, N=400, S=160, P=512, preemph=0.97, kind=None,
                      lps_rows=None, stream=None):
        """rsrgan_wave_synth on caller-owned device tensors (pcm, seg, offsets, window, twiddle as op_feat_wave takes them; lps [rows,
        P / 2 + 1] f32; out f32 [samples], out_seg [B, 2] i64 = (first, capacity); work uint8 (wave_synth_work bytes)), on `stream`
        (default: the current one); nothing is allocated and nothing waits for the device."""
        if kind is None:
            if pcm.dtype not in (torch.int16, torch.float32):
                raise ValueError("op_wave_synth: pcm must be int16 or float32, got %s" % pcm.dtype)
            kind = 0 if pcm.dtype == torch.int16 else 1
        check(self.lib.rsrgan_wave_synth(_ptr(pcm), kind, pcm.numel(), _ptr(seg), _ptr(offsets), _ptr(lps),
                                         lps.shape[0] if lps_rows is None else lps_rows, B, N, S, P, preemph, _ptr(window), _ptr(twiddle),
                                         _ptr(out), out.numel(), _ptr(out_seg), _ptr(work), work.numel() * work.element_size(),
                                         self._stream() if stream is None else C.c_void_p(stream.cuda_stream)))

    def synthesize(self, wb, lps, stream=None):
        """io.WaveBatch (the samples the frames came from) + LPS rows [rows, bins] (a device or host tensor, or an array; de-normalised,
        utterance b at rows wb.offsets[b] .. wb.offsets[b + 1]) -> (samples float32 [sum n] on the device, their segment table int64
        [B, 2] on the host): rsrgan_wave_synth on `stream` (default: the upload stream), the uploads queued there too.  The window and
        twiddle tables are the engine's cached ones; `work` is kept and grown."""
        spec = wb.spec
        if hasattr(spec, "num_mel_bins"):
            raise ValueError("synthesize: the batch's spec makes MFCC / log-mel frames; only an LPS framing (io.wave.WaveSpec) can be inverted")
        us = self.upload_stream() if stream is None else stream
        if not torch.is_tensor(lps):
            lps = torch.from_numpy(np.ascontiguousarray(lps, np.float32))
        if lps.dim() != 2 or lps.shape[1] != spec.bins or lps.shape[0] < 1:
            raise ValueError("synthesize: lps must be [rows >= 1, %d], got %s" % (spec.bins, tuple(lps.shape)))
        B, total = len(wb), max(int(wb.samples.shape[0]), 1)
        need = self.wave_synth_work(B, int(lps.shape[0]), total, spec.frame_length)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device, non_blocking=True)
        if lps.is_cuda:
            us.wait_stream(torch.cuda.current_stream(self.device))           # (the rows were made on the caller's stream)
            lps.record_stream(us)
        with torch.cuda.stream(us):
            win, tw = self._wave_tables(spec, us)
            work = self.__dict__.get("_synth_work")
            if work is None or work.numel() < need:
                work = self._synth_work = torch.empty(need, dtype=torch.uint8, device=self.device)
            lps = lps.to(self.device, torch.float32, non_blocking=True).contiguous()
            out = torch.empty(total, dtype=torch.float32, device=self.device)
            self.op_wave_synth(up(wb.samples), up(wb.seg), up(wb.offsets), lps, B, win, tw, out, up(wb.seg), work, spec.frame_length,
                               spec.frame_shift, spec.padded, spec.preemph, stream=us)
        return out, wb.seg

    def _wave_tables(self, spec, us):
        """the window and the twiddles of a framing as fp32 device tensors: built on the host in float64, rounded once, uploaded at first use
        and kept per engine (as _cmvn_device keeps the statistics).  For an io.wave.MfccSpec three more follow: mel_seg, mel_w and the DCT
        (None for log-mel output)."""
        from .io.wave import dct_table, mel_table, twiddle_table, window_table
        cache = self.__dict__.setdefault("_wave_cache", {})
        ent = cache.get(spec.key())
        if ent is None:
            win = np.ascontiguousarray(window_table(spec.window, spec.frame_length).astype(np.float32))
            with torch.cuda.stream(us):
                ent = (torch.from_numpy(win).to(self.device), torch.from_numpy(twiddle_table(spec.padded)).to(self.device))
                if hasattr(spec, "num_mel_bins"):
                    mseg, mw = mel_table(spec)
                    ent += (torch.from_numpy(mseg).to(self.device), torch.from_numpy(mw).to(self.device),
                            torch.from_numpy(dct_table(spec)).to(self.device) if spec.num_ceps else None)
            if len(cache) > 16:
                cache.clear()
            cache[spec.key()] = ent
        return ent

    def wave_features(self, samples, seg, offsets, rows, spec, us):
        """host samples and tables -> (raw feature rows [rows, spec.bins], the offset table) on the device: LPS for a WaveSpec
        (rsrgan_feat_wave), MFCC or log-mel for an MfccSpec (rsrgan_feat_mfcc).  The uploads and the launch are queued on `us` (the caller is
        inside `with torch.cuda.stream(us)`)"""
        pcm = torch.from_numpy(np.ascontiguousarray(samples)).to(self.device, non_blocking=True)
        dseg = torch.from_numpy(np.ascontiguousarray(seg)).to(self.device, non_blocking=True)
        return self._wave_rows(pcm, dseg, int(seg.shape[0]), offsets, rows, spec, us)

    def _wave_rows(self, pcm, dseg, B, offsets, rows, spec, us):
        """wave_features on samples and segments that are on the device already"""
        tabs = self._wave_tables(spec, us)
        off = torch.from_numpy(np.ascontiguousarray(offsets)).to(self.device, non_blocking=True)
        raw = torch.empty(rows, spec.bins, dtype=torch.float32, device=self.device)
        if hasattr(spec, "num_mel_bins"):
            win, tw, mseg, mw, dct = tabs
            self.op_feat_mfcc(pcm, dseg, off, B, win, tw, mseg, mw, dct, raw, spec.frame_length, spec.frame_shift, spec.padded,
                              spec.preemph, stream=us)
        else:
            win, tw = tabs
            self.op_feat_wave(pcm, dseg, off, B, win, tw, raw, spec.frame_length, spec.frame_shift, spec.padded, spec.preemph,
                              stream=us)
        return raw, off

    def wave_lps(self, samples, seg, offsets, rows, spec, us):
        """wave_features under its first name: the spec's type says which features come out"""
        return self.wave_features(samples, seg, offsets, rows, spec, us)


class HipEngine(WaveFrontEnd):      # (the handle-free rsrgan_op_* wrappers and launch_floor: ops.py)
    def __init__(self, *, batch_size: int, max_frames: int, input_dim: int = 257, output_dim: int = 40,
                 g_type: str = "lstm", g_layers: Optional[int] = None, g_cells: Optional[int] = None,
                 g_proj: Optional[int] = None, d_layers: Optional[int] = None, d_cells: Optional[int] = None,
                 d_proj: Optional[int] = None, d_type: Optional[str] = None, d_joint_off: Optional[int] = None,
                 d_joint_dim: Optional[int] = None, clip_norm: Optional[float] = None, g_splice: Optional[int] = None,
                 l2_scale: float = 0.0, cross_validation: bool = False, batch_norm: bool = False,
                 ema_decay: float = 0.9999, seed: int = 4321, device: Optional[torch.device] = None, flags: int = 3,
                 inference: bool = False):
        if g_type not in _lib.G_TYPES:
            raise ValueError("Unrecognized G type {}".format(g_type))      # gan_rnn_placeholder.py:131-132
        OpEntries.__init__(self, device)
        cfg = RsrganCfg()
        check(self.lib.rsrgan_default_cfg(_lib.G_TYPES[g_type], C.byref(cfg)))
        cfg.batch_size, cfg.max_frames, cfg.input_dim, cfg.output_dim = batch_size, max_frames, input_dim, output_dim
        for k, v in dict(g_layers=g_layers, g_cells=g_cells, g_proj=g_proj, d_layers=d_layers, d_cells=d_cells,
                         d_proj=d_proj).items():
            if v is not None:
                setattr(cfg, k, int(v))
        if d_type is not None:
            if d_type not in _lib.D_TYPES:
                raise ValueError("Unrecognized D type {}".format(d_type))
            cfg.d_type = _lib.D_TYPES[d_type]
            if d_type == "dnn" and g_type not in ("dnn", "rced"):          # discriminator_dnn on the 40-dim target only
                cfg.d_layers = d_layers or 4
                cfg.d_cells = d_cells or 1024
                cfg.d_joint_off, cfg.d_joint_dim = 0, 0
        if d_joint_off is not None:
            cfg.d_joint_off = int(d_joint_off)
        if d_joint_dim is not None:
            cfg.d_joint_dim = int(d_joint_dim)
        if clip_norm is not None:
            cfg.clip_norm = float(clip_norm)
        if g_splice is not None:
            cfg.g_splice = int(g_splice)
        cfg.l2_scale = l2_scale
        cfg.cross_validation = 1 if cross_validation else 0
        cfg.ema_decay = ema_decay
        # inference: a generator-only, forward-only handle (include/rsrgan.h RSRGAN_FLAG_INFER): no discriminator, no optimizer
        # state, no BPTT stash; forward_g, forward_g_stream, the g_state_* calls and the generator's variables only
        self.inference = bool(inference)
        cfg.flags = flags | (_lib.FLAG_BATCH_NORM if batch_norm else 0) | (_lib.FLAG_INFER if inference else 0)
        self.cfg = cfg
        self.batch_size, self.max_frames = batch_size, max_frames
        self.input_dim, self.output_dim = input_dim, output_dim
        self.h = C.c_void_p()
        # RSRGAN_DPIPE (include/rsrgan.h rsrgan_d_step): the library may read a D-run's labels and lengths ahead of the stream if the
        # caller vouches that they are complete when the call is made.  THIS layer can always vouch: d_backward hands every labels /
        # lengths tensor through upload_ready (copied or converted on the upload stream, host-waited), so the pipelined D-run is the
        # default of the Python mirror -- and what bench.py times.  The C ABI's own default stays off: a raw caller has to opt in.
        os.environ.setdefault("RSRGAN_DPIPE", "1")
        check(self.lib.rsrgan_create(C.byref(cfg), C.c_uint64(seed), C.byref(self.h)))
        self._grad_views = {}
        self._comm_stream = None
        # hipGraph capture needs a real stream: the library moves work handed to the legacy null stream onto its own stream
        # with an event hop on both sides of EVERY call (measured ~0.2 ms per call); loops that run under on_stream() hand it
        # this stream instead and pay nothing
        self.stream = torch.cuda.Stream(device=self.device)
        self.d_has_adam = g_type in ("dnn", "rced")
        self.ema_enabled = ema_decay > 0 and not inference      # no EMA shadow buffers in the library otherwise (WHAT['ema'] is absent)

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.rsrgan_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _training_only(self, what: str):
        if self.inference:
            raise _lib.RsrganError("%s: this engine is inference-only (HipEngine(inference=True)): it has no discriminator, "
                                   "gradients or optimizer state" % what)

    def device_bytes(self) -> int:
        """bytes of device memory the library's handle owns (rsrgan_device_bytes); torch's own tensors are not in it"""
        n = C.c_int64()
        check(self.lib.rsrgan_device_bytes(self.h, C.byref(n)))
        return n.value

    # -- plumbing ----------------------------------------------------------------------
    @contextlib.contextmanager
    def on_stream(self):
        """Make the engine's stream the current torch stream for the block (ordered after the previous current stream on
        entry, and the previous stream after it on exit).  Nested use is free."""
        prev = torch.cuda.current_stream(self.device)
        if prev == self.stream:
            yield
            return
        self.stream.wait_stream(prev)
        try:
            with torch.cuda.stream(self.stream):
                yield
        finally:                       # also when the block raises: later work on `prev` must still see what was queued here
            prev.wait_stream(self.stream)

    def _f32(self, a, shape=None) -> torch.Tensor:
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        t = t.to(self.device, torch.float32, non_blocking=True).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError("expected shape %s, got %s" % (tuple(shape), tuple(t.shape)))
        return t

    def upload_ready(self, a, int32=False) -> torch.Tensor:
        """Host array -> device tensor that is COMPLETE when this returns (copied on an upload stream of its own, which the host
        waits for -- not for the compute stream): what RSRGAN_DPIPE=1 asks of the labels and lengths of a D-run (include/rsrgan.h
        rsrgan_d_step), so that D(real) of the next step can run beside the previous step's tail.  Device tensors are converted on the
        upload stream if they need it, and waited for once per tensor object otherwise (see below)."""
        us = getattr(self, "_upload_stream", None)
        if us is None:
            us = self._upload_stream = torch.cuda.Stream(self.device)
        if isinstance(a, torch.Tensor) and a.device == self.device:
            want = torch.int32 if int32 else torch.float32
            if a.dtype == want and a.is_contiguous():
                # A device tensor nobody has vouched for may still be being written by a kernel queued on some stream.  The first time
                # this very tensor object (at this version: in-place writes through torch bump it) comes by, the host waits for the
                # device once; from then on it passes through untouched -- a resident batch fed again and again (bench.py, a cached
                # validation set) costs nothing, a freshly computed tensor per step costs a device wait per step (or RSRGAN_DPIPE=0).
                seen = self.__dict__.setdefault("_vouched", {})
                ent = seen.get(id(a))
                if ent is None or ent[0]() is not a or ent[1] != a._version:
                    torch.cuda.synchronize(self.device)
                    self._vouch(a)
                return a
            # an int64 `lengths`, a float64 or strided label: the conversion is a KERNEL.  Queued on the current stream it would sit
            # behind that stream's backlog while D(real) on the library's side stream reads its output ahead of it -- so it runs on
            # the upload stream (the caller vouches for `a` itself being complete) and the host waits for it, as for a host array.
            with torch.cuda.stream(us):
                t = a.to(want).contiguous()
            us.synchronize()
            t.record_stream(torch.cuda.current_stream(self.device))
            self._vouch(t)
            return t
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a) if int32 else np.ascontiguousarray(a, dtype=np.float32))
        with torch.cuda.stream(us):
            t = t.to(self.device, non_blocking=True)
            t = (t.to(torch.int32) if int32 else t.to(torch.float32)).contiguous()
        us.synchronize()
        t.record_stream(torch.cuda.current_stream(self.device))
        self._vouch(t)
        return t

    def _vouch(self, t):
        """remember that device tensor `t` (this object, at this version) is complete: upload_ready lets it pass without a wait"""
        import weakref
        seen = self.__dict__.setdefault("_vouched", {})
        if len(seen) > 256:
            for k in [k for k, (r, _) in seen.items() if r() is None]:
                del seen[k]
            if len(seen) > 256:
                seen.clear()
        seen[id(t)] = (weakref.ref(t), t._version)

    def upload_async(self, a, int32=False) -> torch.Tensor:
        """Host array -> device tensor on the upload stream, consumed in STREAM order: the current stream waits for the copy (an event,
        no host wait), so the copy runs beside whatever the compute stream still has queued instead of in front of the next step's
        first launch (a 6.6 MB pageable copy of the input frames is ~0.6 ms of a 4.8 ms step).  What the inputs of every run, and the
        labels / lengths of a stream-ordered D-run (RSRGAN_DPIPE=0), need; device tensors pass through."""
        if isinstance(a, torch.Tensor) and a.device == self.device:
            return a
        us = getattr(self, "_upload_stream", None)
        if us is None:
            us = self._upload_stream = torch.cuda.Stream(self.device)
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a) if int32 else np.ascontiguousarray(a, dtype=np.float32))
        with torch.cuda.stream(us):
            t = t.to(self.device, non_blocking=True)
            t = (t.to(torch.int32) if int32 else t.to(torch.float32)).contiguous()
            ev = torch.cuda.Event()
            ev.record(us)
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        t.record_stream(cur)
        return t

    # -- the feature front end on the device (include/rsrgan.h rsrgan_feat_batch, csrc/feat.hip) ---------------------------
    def op_feat_batch(self, raw, offsets, B, T, D, left, right, mean, stddev, out, lengths=None, raw_rows=None, stream=None):
        """rsrgan_feat_batch on caller-owned device tensors (raw [rows, D] f32, offsets [B + 1] i32, mean / stddev [D] f64 or None,
        out B * T * D * (left + 1 + right) f32, lengths [B] i32 or None), on `stream` (default: the current one)"""
        check(self.lib.rsrgan_feat_batch(_ptr(raw), raw.shape[0] if raw_rows is None else raw_rows, _ptr(offsets), B, T, D, left, right,
                                         _ptr(mean), _ptr(stddev), _ptr(out), _ptr(lengths),
                                         self._stream() if stream is None else C.c_void_p(stream.cuda_stream)))

    def _cmvn_device(self, mean, stddev, us):
        """the two CMVN vectors as fp64 device tensors, uploaded once per pair of host arrays (the cache holds the host arrays, so
        their ids stay theirs)"""
        cache = self.__dict__.setdefault("_cmvn_cache", {})
        ent = cache.get((id(mean), id(stddev)))
        if ent is None:
            host = [np.ascontiguousarray(v, np.float64).reshape(-1) for v in (mean, stddev)]
            with torch.cuda.stream(us):
                dev = [torch.from_numpy(h).to(self.device) for h in host]
            if len(cache) > 16:
                cache.clear()
            ent = cache[(id(mean), id(stddev))] = (mean, stddev, dev[0], dev[1])
        return ent[2], ent[3]

    def featurize(self, packed, left=None, right=None, mean=None, stddev=None, ready=False, limit=True):
        """io.PackedBatch (raw frames + offsets) -> (x [B, T, D * (left + 1 + right)] f32, lengths [B] i32) on the device: CMVN, splice
        and padding in one kernel (csrc/feat.hip), bit for bit what io.features computes on the host.  left / right / mean / stddev
        default to what the batch carries.  The packed frames and the offset table travel on the engine's upload stream and the kernel
        runs there: ready=True waits for THAT stream only and vouches for the results (what upload_ready gives the labels and lengths of
        a D-run under RSRGAN_DPIPE=1); ready=False hands them over by event, as upload_async does.  ValueError before any device work
        if an utterance is longer than max_frames (limit=False: the caller cuts the result into chunks itself, as the chunked decode
        does).  An io.CodedBatch (the archive's bytes: float, double or Kaldi-compressed matrices) is decoded on the device first
        (_featurize_coded), an io.WaveBatch (audio samples) becomes log-power-spectrum frames there first (_featurize_wave); everything
        else is the same."""
        left = packed.left if left is None else int(left)
        right = packed.right if right is None else int(right)
        if mean is None and stddev is None:
            mean, stddev = packed.mean, packed.stddev
        if (mean is None) != (stddev is None):
            raise ValueError("featurize: mean and stddev must both be given or both be None")
        if hasattr(packed, "blob"):
            return self._featurize_coded(packed, left, right, mean, stddev, ready, limit)
        if hasattr(packed, "samples"):
            return self._featurize_wave(packed, left, right, mean, stddev, ready, limit)
        data, offsets = packed.data, packed.offsets
        if not isinstance(data, np.ndarray) or data.dtype != np.float32 or data.ndim != 2:
            raise ValueError("featurize: packed.data must be a float32 [rows, D] array")
        B, T = int(packed.shape[0]), int(packed.shape[1])
        D = data.shape[1]
        offsets = np.ascontiguousarray(offsets, np.int32)
        if offsets.shape != (B + 1,) or B < 1 or T < 1 or data.shape[0] < 1:
            raise ValueError("featurize: B = %d, T = %d, %d rows, %d offsets" % (B, T, data.shape[0], offsets.shape[0]))
        n = np.diff(offsets.astype(np.int64))
        if n.min() < 0 or offsets[0] < 0 or offsets[-1] > data.shape[0]:
            raise ValueError("featurize: the offset table does not describe utterances inside the %d packed rows" % data.shape[0])
        if limit and max(int(n.max()), T) > self.max_frames:
            raise ValueError("featurize: an utterance of %d frames (T = %d) is longer than max_frames = %d" % (int(n.max()), T, self.max_frames))
        if mean is not None and (np.size(mean) != D or np.size(stddev) != D):
            raise ValueError("featurize: mean / stddev must hold D = %d entries, got %d / %d" % (D, np.size(mean), np.size(stddev)))
        us = getattr(self, "_upload_stream", None)
        if us is None:
            us = self._upload_stream = torch.cuda.Stream(self.device)
        dm, ds = self._cmvn_device(mean, stddev, us) if mean is not None else (None, None)
        with torch.cuda.stream(us):
            raw = torch.from_numpy(np.ascontiguousarray(data)).to(self.device, non_blocking=True)
            off = torch.from_numpy(offsets).to(self.device, non_blocking=True)
            out = torch.empty(B, T, D * (left + 1 + right), dtype=torch.float32, device=self.device)
            ln = torch.empty(B, dtype=torch.int32, device=self.device)
            self.op_feat_batch(raw, off, B, T, D, left, right, dm, ds, out, ln, stream=us)
            if not ready:
                ev = torch.cuda.Event()
                ev.record(us)
        cur = torch.cuda.current_stream(self.device)
        if ready:
            us.synchronize()
            self._vouch(out); self._vouch(ln)
        else:
            cur.wait_event(ev)
        out.record_stream(cur); ln.record_stream(cur)
        return out, ln

    # -- the archive side (include/rsrgan.h rsrgan_feat_decode, csrc/feat.hip k_feat_decode) -----------------------------------
    def op_feat_decode(self, blob, seg, scale, offsets, B, D, mean, stddev, out, blob_bytes=None, out_rows=None, stream=None):
        """rsrgan_feat_decode on caller-owned device tensors (blob uint8, seg [B, 2] i64 = (byte offset, kind), scale [B, 2] f32 = (min,
        range), offsets [B + 1] i32, mean / stddev [D] f64 or None, out [rows, D] f32), on `stream` (default: the current one)"""
        check(self.lib.rsrgan_feat_decode(_ptr(blob), blob.numel() if blob_bytes is None else blob_bytes, _ptr(seg), _ptr(scale), _ptr(offsets),
                                          B, D, _ptr(mean), _ptr(stddev), _ptr(out), out.shape[0] if out_rows is None else out_rows,
                                          self._stream() if stream is None else C.c_void_p(stream.cuda_stream)))

    def _featurize_coded(self, coded, left, right, mean, stddev, ready, limit):
        """featurize for an io.CodedBatch: the blob and the three tables travel on the upload stream, rsrgan_feat_decode turns them into
        normalised float32 rows [frames, D] and rsrgan_feat_batch (mean = NULL) splices and pads those -- the decode normalises, because the
        host path never rounds the decoded value to float32 before it does."""
        blob, seg, scale, offsets = coded.blob, coded.seg, coded.scale, coded.offsets
        B, T, D = int(coded.shape[0]), int(coded.shape[1]), int(coded.dim)
        rows = int(offsets[-1]) if offsets.shape[0] else 0
        if B < 1 or T < 1 or rows < 1 or offsets.shape != (B + 1,):
            raise ValueError("featurize: B = %d, T = %d, %d rows, %d offsets" % (B, T, rows, offsets.shape[0]))
        n = np.diff(offsets.astype(np.int64))
        if limit and max(int(n.max()), T) > self.max_frames:
            raise ValueError("featurize: an utterance of %d frames (T = %d) is longer than max_frames = %d" % (int(n.max()), T, self.max_frames))
        if mean is not None and (np.size(mean) != D or np.size(stddev) != D):
            raise ValueError("featurize: mean / stddev must hold D = %d entries, got %d / %d" % (D, np.size(mean), np.size(stddev)))
        us = self.upload_stream()
        dm, ds = self._cmvn_device(mean, stddev, us) if mean is not None else (None, None)
        with torch.cuda.stream(us):
            dblob = torch.from_numpy(np.ascontiguousarray(blob)).to(self.device, non_blocking=True)
            dseg = torch.from_numpy(np.ascontiguousarray(seg)).to(self.device, non_blocking=True)
            dscale = torch.from_numpy(np.ascontiguousarray(scale)).to(self.device, non_blocking=True)
            off = torch.from_numpy(np.ascontiguousarray(offsets)).to(self.device, non_blocking=True)
            raw = torch.empty(rows, D, dtype=torch.float32, device=self.device)
            out = torch.empty(B, T, D * (left + 1 + right), dtype=torch.float32, device=self.device)
            ln = torch.empty(B, dtype=torch.int32, device=self.device)
            self.op_feat_decode(dblob, dseg, dscale, off, B, D, dm, ds, raw, stream=us)
            self.op_feat_batch(raw, off, B, T, D, left, right, None, None, out, ln, stream=us)
            if not ready:
                ev = torch.cuda.Event()
                ev.record(us)
        cur = torch.cuda.current_stream(self.device)
        if ready:
            us.synchronize()
            self._vouch(out); self._vouch(ln)
        else:
            cur.wait_event(ev)
        out.record_stream(cur); ln.record_stream(cur)
        return out, ln

    def _featurize_wave(self, wb, left, right, mean, stddev, ready, limit):
        """featurize for an io.WaveBatch: the samples and the two tables travel on the upload stream, wave_features writes the raw rows
        [frames, bins] the batch's spec asks for (rsrgan_feat_wave: LPS; rsrgan_feat_mfcc: MFCC or log-mel) and rsrgan_feat_batch
        normalises, splices and pads those; the hand-off is _featurize_coded's."""
        offsets, spec = wb.offsets, wb.spec
        B, T, D = int(wb.shape[0]), int(wb.shape[1]), int(wb.dim)
        rows = int(offsets[-1]) if offsets.shape[0] else 0
        if B < 1 or T < 1 or rows < 1 or offsets.shape != (B + 1,):
            raise ValueError("featurize: B = %d, T = %d, %d rows, %d offsets" % (B, T, rows, offsets.shape[0]))
        n = np.diff(offsets.astype(np.int64))
        if limit and max(int(n.max()), T) > self.max_frames:
            raise ValueError("featurize: an utterance of %d frames (T = %d) is longer than max_frames = %d" % (int(n.max()), T, self.max_frames))
        if mean is not None and (np.size(mean) != D or np.size(stddev) != D):
            raise ValueError("featurize: mean / stddev must hold D = %d entries, got %d / %d" % (D, np.size(mean), np.size(stddev)))
        us = self.upload_stream()
        dm, ds = self._cmvn_device(mean, stddev, us) if mean is not None else (None, None)
        with torch.cuda.stream(us):
            if getattr(wb, "plan", None) is not None:
                # clean samples with a plan: reverberated on the device first (csrc/reverb.hip), float32 on the int16 scale
                pcm, dseg, _ = self.simulate(wb, stream=us)
                raw, off = self._wave_rows(pcm, dseg, B, offsets, rows, spec, us)
            else:
                raw, off = self.wave_features(wb.samples, wb.seg, offsets, rows, spec, us)
            out = torch.empty(B, T, D * (left + 1 + right), dtype=torch.float32, device=self.device)
            ln = torch.empty(B, dtype=torch.int32, device=self.device)
            self.op_feat_batch(raw, off, B, T, D, left, right, dm, ds, out, ln, stream=us)
            if not ready:
                ev = torch.cuda.Event()
                ev.record(us)
        cur = torch.cuda.current_stream(self.device)
        if ready:
            us.synchronize()
            self._vouch(out); self._vouch(ln)
        else:
            cur.wait_event(ev)
        out.record_stream(cur); ln.record_stream(cur)
        return out, ln

    # -- the frame-level recipes' front end (include/rsrgan.h rsrgan_feat_frames, csrc/feat.hip k_feat_frames) ------------------
    def op_feat_frames(self, pool, picks, N, D, left, right, mean, stddev, out, pool_rows=None, stream=None):
        """rsrgan_feat_frames on caller-owned device tensors (pool [rows, D] f32, picks [N, 3] i32 = (row, lo, hi), mean / stddev [D] f64 or
        None, out N * D * (left + 1 + right) f32), on `stream` (default: the current one)"""
        check(self.lib.rsrgan_feat_frames(_ptr(pool), pool.shape[0] if pool_rows is None else pool_rows, _ptr(picks), N, D, left, right,
                                          _ptr(mean), _ptr(stddev), _ptr(out),
                                          self._stream() if stream is None else C.c_void_p(stream.cuda_stream)))

    def featurize_frames(self, item, ready=False):
        """io.FrameDraw (FrameBatchReader(device_features=True)) -> (x [N, D * (left + 1 + right)] f32, labels [N, Dl] f32) on the device, bit
        for bit the default reader's batch.  The engine keeps one pool per reader: inputs [pool_rows, D] and labels [pool_rows, Dl], holding
        the queue's utterances NORMALISED (float64 arithmetic, one rounding: rsrgan_feat_batch with B = 1, context 0 / 0, writing straight
        into the slot).  Per item: grow the pools if the reader's allocator did (old rows keep their numbers), normalise the new utterances
        once, then gather the drawn frames with two rsrgan_feat_frames launches (inputs with the recipe's context, labels with none; mean =
        NULL).  Gathering rows commutes with the elementwise cast to float32, which is why normalise -> cast -> gather gives the bits of the
        host's normalise -> splice -> cast.  Coded admissions (FrameBatchReader(device_decode=True): the archive's bytes) are decoded and
        normalised into the slot by rsrgan_feat_decode instead.  ready as in featurize.  ValueError before any device work for an item that is not the next one
        of its reader."""
        from .io.features import pack_coded
        from .io.frame_pool import PoolLedger, is_coded
        pools =self.__dict__.setdefault("_frame_pools", {})
        st = pools.get(item.reader_id)
        if st is None:
            st = pools[item.reader_id] = {"ledger": PoolLedger(item.reader_id), "x": None, "y": None, "items": 0, "uploads": 0, "growths": 0}
        st["ledger"].admit(item)                                   # (raises before anything is queued)
        N, D, Dl, left, right = item.picks.shape[0], item.input_dim, item.label_dim, item.left, item.right
        us = getattr(self, "_upload_stream", None)
        if us is None:
            us = self._upload_stream = torch.cuda.Stream(self.device)
        mi = si = ml = sl = None
        if item.stats is not None:
            if any(np.size(v) != d for v, d in zip(item.stats, (D, D, Dl, Dl))):
                raise ValueError("featurize_frames: the statistics must hold %d / %d entries" % (D, Dl))
            mi, si = self._cmvn_device(item.stats[0], item.stats[1], us)
            ml, sl = self._cmvn_device(item.stats[2], item.stats[3], us)
        # EVERYTHING below is queued on the upload stream, item after item: pool growth, uploads, normalisation and the gathers.  Slot reuse
        # rests on that order alone: the reader hands a slot out again once its utterance's last frame was drawn, so an upload into a freed
        # slot belongs to a LATER item than the last gather that read the slot, and runs behind it on this stream.  The same order keeps a
        # grown pool's copy of the old rows behind every write to them and in front of every later read.
        with torch.cuda.stream(us):
            if st["x"] is None or item.pool_rows > st["x"].shape[0]:
                nx = torch.empty(item.pool_rows, D, dtype=torch.float32, device=self.device)
                ny = torch.empty(item.pool_rows, Dl, dtype=torch.float32, device=self.device)
                if st["x"] is not None:
                    old = st["x"].shape[0]
                    nx[:old].copy_(st["x"]); ny[:old].copy_(st["y"])
                    st["growths"] += 1
                st["x"], st["y"] = nx, ny
            px, py = st["x"], st["y"]
            coded = [u for u in item.uploads if is_coded(u[1])]
            if coded:
                # coded admissions (FrameBatchReader(device_decode=True)): the item's bytes travel as ONE blob per side with one set of
                # tables, and every utterance is decoded and normalised straight into its pool rows by a launch of its own (B = 1, the
                # table pointers advanced to its entry, offsets = (first, first + n), out = the whole pool): slots are not adjacent
                # rows, and rows between them belong to other utterances
                offs = torch.tensor([[f, f + u.rows] for f, u, _ in coded], dtype=torch.int32).to(self.device, non_blocking=True)
                for side, pool, Dp, m, s in ((1, px, D, mi, si), (2, py, Dl, ml, sl)):
                    cb = pack_coded([u[side] for u in coded])
                    dblob = torch.from_numpy(cb.blob).to(self.device, non_blocking=True)
                    dseg = torch.from_numpy(cb.seg).to(self.device, non_blocking=True)
                    dscale = torch.from_numpy(cb.scale).to(self.device, non_blocking=True)
                    for b in range(len(coded)):
                        self.op_feat_decode(dblob, dseg[b], dscale[b], offs[b], 1, Dp, m, s, pool, stream=us)
            for first, rx, ry in item.uploads:
                if is_coded(rx):
                    continue
                n = rx.shape[0]
                if mi is None:
                    px[first:first + n].copy_(torch.from_numpy(rx), non_blocking=True)
                    py[first:first + n].copy_(torch.from_numpy(ry), non_blocking=True)
                    continue
                off = torch.tensor([0, n], dtype=torch.int32).to(self.device, non_blocking=True)
                sx = torch.from_numpy(rx).to(self.device, non_blocking=True)
                sy = torch.from_numpy(ry).to(self.device, non_blocking=True)
                # (a slot starts on a multiple of 4 rows: its address is 16-byte aligned at any D, as the entry asks of `out`)
                self.op_feat_batch(sx, off, 1, n, D, 0, 0, mi, si, px[first:first + n], None, stream=us)
                self.op_feat_batch(sy, off, 1, n, Dl, 0, 0, ml, sl, py[first:first + n], None, stream=us)
            picks = torch.from_numpy(item.picks).to(self.device, non_blocking=True)
            x = torch.empty(N, D * (left + 1 + right), dtype=torch.float32, device=self.device)
            lab = torch.empty(N, Dl, dtype=torch.float32, device=self.device)
            self.op_feat_frames(px, picks, N, D, left, right, None, None, x, stream=us)
            self.op_feat_frames(py, picks, N, Dl, 0, 0, None, None, lab, stream=us)
            if not ready:
                ev = torch.cuda.Event()
                ev.record(us)
        st["items"] += 1; st["uploads"] += len(item.uploads)
        cur = torch.cuda.current_stream(self.device)
        if ready:
            us.synchronize()
            self._vouch(x); self._vouch(lab)
        else:
            cur.wait_event(ev)
        x.record_stream(cur); lab.record_stream(cur)
        return x, lab

    def frame_pool_stats(self, reader_id):
        """{'pool_rows', 'bytes', 'items', 'uploads', 'growths'} of one reader's pool (None before its first item)"""
        st = self.__dict__.get("_frame_pools", {}).get(reader_id)
        if st is None or st["x"] is None:
            return None
        return {"pool_rows": st["x"].shape[0], "bytes": (st["x"].numel() + st["y"].numel()) * 4, "items": st["items"], "uploads": st["uploads"],
                "growths": st["growths"]}

    def drop_frame_pool(self, reader_id):
        """forget a reader's pool (its device memory goes back to torch once the last batch gathered from it is consumed)"""
        self.__dict__.get("_frame_pools", {}).pop(reader_id, None)

    # -- the live path's front end and the output side (include/rsrgan.h rsrgan_feat_stream / rsrgan_feat_denorm, csrc/feat.hip) ------
    def op_feat_stream(self, fresh, table, hist, B, H, T, D, left, right, mean, stddev, out, lengths=None, fresh_rows=None, stream=None):
        """rsrgan_feat_stream on caller-owned device tensors (fresh [rows, D] f32 or None, table [B, 6] i32 = (src, app0, napp, emit0, nemit,
        last), hist [B, H, D] f32, mean / stddev [D] f64 or None, out B * T * D * (left + 1 + right) f32, lengths [B] i32 or None), on
        `stream` (default: the current one)"""
        rows = (0 if fresh is None else fresh.shape[0]) if fresh_rows is None else fresh_rows
        check(self.lib.rsrgan_feat_stream(_ptr(fresh), rows, _ptr(table), _ptr(hist), B, H, T, D, left, right, _ptr(mean), _ptr(stddev),
                                          _ptr(out), _ptr(lengths), self._stream() if stream is None else C.c_void_p(stream.cuda_stream)))

    def op_feat_denorm(self, y, lengths, B, T, D, mean, stddev, out, stream=None):
        """rsrgan_feat_denorm on caller-owned device tensors (y B * T * D f32, lengths [B] i32 or None, mean / stddev [D] f64, out B * T * D
        f64), on `stream` (default: the current one)"""
        check(self.lib.rsrgan_feat_denorm(_ptr(y), _ptr(lengths), B, T, D, _ptr(mean), _ptr(stddev), _ptr(out),
                                          self._stream() if stream is None else C.c_void_p(stream.cuda_stream)))

    def denormalize(self, y, mean, stddev, lengths=None):
        """G(x) y [B, T, D] f32 on the device -> y * stddev + mean as [B, T, D] f64 on the device (rows from lengths[b] on are zero), on the
        current stream: bit for bit NumPy's result on the host copy.  mean / stddev: host arrays of D entries (uploaded once per pair)."""
        y = y.contiguous()
        B, T, D = y.shape
        if np.size(mean) != D or np.size(stddev) != D:
            raise ValueError("denormalize: mean / stddev must hold D = %d entries, got %d / %d" % (D, np.size(mean), np.size(stddev)))
        us = self.upload_stream()
        dm, ds = self._cmvn_device(mean, stddev, us)
        cur = torch.cuda.current_stream(self.device)
        cur.wait_stream(us)                                        # (the statistics' upload, the first time)
        out = torch.empty(B, T, D, dtype=torch.float64, device=self.device)
        self.op_feat_denorm(y, lengths, B, T, D, dm, ds, out)
        return out

    def _i32(self, a) -> torch.Tensor:
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(self.device).to(torch.int32).contiguous()       # placeholder is float32, cast like dynamic_rnn

    def _noise(self, n):
        if n is None:
            return None
        return self._f32(n).reshape(self.batch_size, self.output_dim)

    # -- scalars -----------------------------------------------------------------------
    def set_scalar(self, name: str, v: float):
        check(self.lib.rsrgan_set_scalar(self.h, SCALARS[name], float(v)))

    def get_scalar(self, name: str) -> float:
        out = C.c_double()
        check(self.lib.rsrgan_get_scalar(self.h, SCALARS[name], C.byref(out)))
        return out.value

    # -- variables ---------------------------------------------------------------------
    def tensor_table(self, net: int) -> List[Tuple[str, Tuple[int, ...], int]]:
        n = self.lib.rsrgan_num_tensors(self.h, net)
        out = []
        buf = C.create_string_buffer(256)
        for i in range(n):
            r, c, off = C.c_int32(), C.c_int32(), C.c_int64()
            check(self.lib.rsrgan_tensor_info(self.h, net, i, buf, 256, C.byref(r), C.byref(c), C.byref(off)))
            shape = (r.value,) if c.value == 0 else (r.value, c.value)
            out.append((buf.value.decode(), shape, off.value))
        return out

    def param_count(self, net: int) -> int:
        return int(self.lib.rsrgan_param_count(self.h, net))

    def get_params(self, net: int, what: str = "variables") -> torch.Tensor:
        out = torch.empty(self.param_count(net), dtype=torch.float32, device=self.device)
        check(self.lib.rsrgan_get_params(self.h, net, WHAT[what], _ptr(out), self._stream()))
        return out

    def set_params(self, net: int, flat, what: str = "variables"):
        t = self._f32(flat).reshape(-1)
        if t.numel() != self.param_count(net):
            raise ValueError("expected %d floats, got %d" % (self.param_count(net), t.numel()))
        check(self.lib.rsrgan_set_params(self.h, net, WHAT[what], _ptr(t), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()        # `t` may be a temporary

    def get_grads(self, net: int) -> torch.Tensor:
        self._training_only('get_grads')
        out = torch.empty(self.param_count(net), dtype=torch.float32, device=self.device)
        check(self.lib.rsrgan_get_grads(self.h, net, _ptr(out), self._stream()))
        return out

    def grad_view(self, net: int) -> torch.Tensor:
        """Zero-copy torch view of the library's (padded, flat) gradient buffer."""
        self._training_only('grad_view')
        if net not in self._grad_views:
            p, n = C.c_void_p(), C.c_int64()
            check(self.lib.rsrgan_grad_buffer(self.h, net, C.byref(p), C.byref(n)))
            self._grad_views[net] = torch.as_tensor(_RawDeviceBuffer(p.value, n.value), device=self.device)
        return self._grad_views[net]

    def grad_buckets(self, net: int) -> List[Tuple[int, int]]:
        """(offset, count) float ranges of the gradient buffer in the order the backward completes them."""
        self._training_only('grad_buckets')
        out = []
        for i in range(self.lib.rsrgan_grad_bucket_count(self.h, net)):
            off, cnt = C.c_int64(), C.c_int64()
            check(self.lib.rsrgan_grad_bucket_info(self.h, net, i, C.byref(off), C.byref(cnt)))
            out.append((off.value, cnt.value))
        return out

    def all_reduce_grads(self, net: int, group=None, force: bool = False):
        """average_gradients (utils/ops.py:343-376) over ranks: one all-reduce per gradient bucket, issued on a
        communication stream that waits only for that bucket's completion event, so RCCL moves the first buckets over
        xGMI while the weight-gradient GEMMs of the later ones still run.  RSRGAN_BUCKETED_ALLREDUCE=0 (or a single
        bucket) falls back to one all-reduce of the whole buffer on the compute stream."""
        from . import dist as rdist
        ws = rdist.world_size(group)
        if ws == 1 and not force:
            return
        view = self.grad_view(net)
        buckets = self.grad_buckets(net)
        if len(buckets) <= 1 or os.environ.get("RSRGAN_BUCKETED_ALLREDUCE", "1") == "0":
            rdist.all_reduce_mean_(view, group)
            return
        if self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(device=self.device)

        def wait_bucket(i, stream):
            check(self.lib.rsrgan_grad_bucket_wait(self.h, net, i, C.c_void_p(stream.cuda_stream)))

        timing = {"buckets": []} if getattr(self, "bucket_timing", False) else None
        rdist.all_reduce_mean_buckets_(view, buckets, group, wait_bucket, self._comm_stream, timing)   # joins before rsrgan_apply
        if timing is not None:
            self._last_timing = timing

    def bucket_report(self):
        """Diagnostic of the last bucketed all-reduce run with `engine.bucket_timing = True` (synchronises): per bucket its bytes,
        the milliseconds its all-reduce took on the communication stream and when it started / ended relative to the moment the
        compute stream had finished every gradient; `exposed_ms` = how long the compute stream then waited for the communication
        stream (everything before that moment was hidden behind the weight-gradient GEMMs of the later buckets)."""
        t = getattr(self, "_last_timing", None)
        if not t:
            return None
        torch.cuda.synchronize(self.device)
        rows = []
        for i, nbytes, e0, e1 in t["buckets"]:
            rows.append({"bucket": i, "bytes": int(nbytes), "allreduce_ms": round(e0.elapsed_time(e1), 4),
                         "start_vs_compute_done_ms": round(t["ready"].elapsed_time(e0), 4),
                         "end_vs_compute_done_ms": round(t["ready"].elapsed_time(e1), 4)})
        return {"buckets": rows, "exposed_ms": round(t["ready"].elapsed_time(t["joined"]), 4)}

    # -- the path ----------------------------------------------------------------------
    def _check_batch(self, x, lab=None, ln=None):
        """The library reads and writes exactly batch_size x T x input_dim / output_dim elements behind the raw pointers:
        refuse anything else here (the reference's placeholders have these static shapes, gan_rnn_placeholder.py:94-104)."""
        if x.dim() != 3 or x.shape[0] != self.batch_size or x.shape[2] != self.input_dim:
            raise ValueError("inputs must be [batch_size=%d, T, input_dim=%d], got %s" % (self.batch_size, self.input_dim, tuple(x.shape)))
        T = x.shape[1]
        if not 0 < T <= self.max_frames:
            raise ValueError("T=%d outside (0, max_frames=%d]" % (T, self.max_frames))
        if lab is not None and tuple(lab.shape) != (self.batch_size, T, self.output_dim):
            raise ValueError("labels must be [%d, %d, %d], got %s" % (self.batch_size, T, self.output_dim, tuple(lab.shape)))
        if ln is not None and ln.numel() != self.batch_size:
            raise ValueError("lengths must hold batch_size=%d entries, got %d" % (self.batch_size, ln.numel()))
        return T

    def forward_g(self, x, lengths) -> torch.Tensor:
        x = self._f32(x)
        ln = self._i32(lengths) if lengths is not None else None
        T = self._check_batch(x, None, ln)
        B = self.batch_size
        y = torch.empty(B, T, self.output_dim, dtype=torch.float32, device=self.device)
        check(self.lib.rsrgan_forward_g(self.h, _ptr(x), _ptr(ln), T, _ptr(y), self._stream()))
        return y

    # -- the stateful forward (include/rsrgan.h: the carried generator state) -------------
    def g_state_floats(self) -> int:
        """floats of one row's state blob: layer 0's c, layer 0's m, layer 1's c, ... unpadded"""
        n = C.c_int32()
        check(self.lib.rsrgan_g_state_floats(self.h, C.byref(n)))
        return n.value

    def g_state_reset(self, rows=None):
        """zero the carried state of the rows in `rows` (an iterable of row indices); None = every row"""
        mask = None
        if rows is not None:
            m = np.zeros(self.batch_size, dtype=np.int32)
            for r in rows:
                if not 0 <= int(r) < self.batch_size:
                    raise ValueError("row %d outside [0, batch_size=%d)" % (int(r), self.batch_size))
                m[int(r)] = 1
            mask = self._i32(m)
        check(self.lib.rsrgan_g_state_reset(self.h, _ptr(mask), self._stream()))
        self._keep_mask = mask

    def g_state_get(self) -> torch.Tensor:
        out = torch.empty(self.batch_size, self.g_state_floats(), dtype=torch.float32, device=self.device)
        check(self.lib.rsrgan_g_state_get(self.h, _ptr(out), self._stream()))
        return out

    def g_state_set(self, t):
        t = self._f32(t, (self.batch_size, self.g_state_floats()))
        check(self.lib.rsrgan_g_state_set(self.h, _ptr(t), self._stream()))
        self._keep_state = t

    def forward_g_stream(self, x, lengths) -> torch.Tensor:
        """forward_g from and into the carried state: row b continues where its previous call ended and advances by lengths[b]"""
        x = self._f32(x)
        if lengths is None:
            raise ValueError("forward_g_stream needs lengths")
        ln = self._i32(lengths)
        T = self._check_batch(x, None, ln)
        y = torch.empty(self.batch_size, T, self.output_dim, dtype=torch.float32, device=self.device)
        check(self.lib.rsrgan_forward_g_stream(self.h, _ptr(x), _ptr(ln), T, _ptr(y), self._stream()))
        self._keep3 = (x, ln)
        return y

    def d_backward(self, x, lab, lengths, noise_real=None, noise_fake=None, train=True, apply=False) -> torch.Tensor:
        self._training_only("d_backward")
        if os.environ.get("RSRGAN_DPIPE", "0") not in ("", "0"):      # the library reads labels / lengths ahead of the stream: hand it complete ones
            lab = self.upload_ready(lab)
            lengths = self.upload_ready(lengths, int32=True) if lengths is not None else None
        x, lab = self._f32(x), self._f32(lab)
        ln = self._i32(lengths) if lengths is not None else None
        nr, nf = self._noise(noise_real), self._noise(noise_fake)
        out = torch.empty(3, dtype=torch.float32, device=self.device)
        T = self._check_batch(x, lab, ln)
        if apply or not train:
            check(self.lib.rsrgan_d_step(self.h, _ptr(x), _ptr(lab), _ptr(ln), T, _ptr(nr), _ptr(nf), _ptr(out),
                                         1 if train else 0, self._stream()))
        else:
            check(self.lib.rsrgan_d_backward(self.h, _ptr(x), _ptr(lab), _ptr(ln), T, _ptr(nr), _ptr(nf), _ptr(out),
                                             self._stream()))
        self._keep = (x, lab, ln, nr, nf)       # borrowed until the stream has consumed them
        return out

    def g_backward(self, x, lab, lengths, noise_fake=None, train=True, reuse=False, apply=False) -> torch.Tensor:
        self._training_only("g_backward")
        x, lab = self._f32(x), self._f32(lab)
        ln = self._i32(lengths) if lengths is not None else None
        nf = self._noise(noise_fake)
        out = torch.empty(4, dtype=torch.float32, device=self.device)
        T = self._check_batch(x, lab, ln)
        if apply or not train:
            check(self.lib.rsrgan_g_step(self.h, _ptr(x), _ptr(lab), _ptr(ln), T, _ptr(nf), _ptr(out),
                                         1 if train else 0, 1 if reuse else 0, self._stream()))
        else:
            check(self.lib.rsrgan_g_backward(self.h, _ptr(x), _ptr(lab), _ptr(ln), T, _ptr(nf), _ptr(out),
                                             1 if reuse else 0, self._stream()))
        self._keep2 = (x, lab, ln, nf)
        return out

    # -- the D-run's logits and their histograms (include/rsrgan.h rsrgan_d_logits, rsrgan_d_logits_hist; csrc/hist.hip) -----
    def d_logits(self):
        """(real, fake): the discriminator's logits of the most recent d_backward as two [batch_size, T] float32 device tensors (the
        reference's d_rl_logits / d_fk_logits [B, T, 1]; with d_type dnn the clipped values).  Call before the next g_backward: it
        writes D(G(x)) over them."""
        T = C.c_int32()
        check(self.lib.rsrgan_d_logits(self.h, None, None, C.byref(T), self._stream()))
        real = torch.empty(self.batch_size, T.value, dtype=torch.float32, device=self.device)
        fake = torch.empty_like(real)
        check(self.lib.rsrgan_d_logits(self.h, _ptr(real), _ptr(fake), C.byref(T), self._stream()))
        return real, fake

    def d_logits_hist(self) -> torch.Tensor:
        """[2, 5 + NL] float64 device tensor: the histogram records (summary.histogram_stats) of d_logits()' two tensors, read straight
        from the library's buffer"""
        out = torch.empty(2, 5 + len(_lib.hist_limits()), dtype=torch.float64, device=self.device)
        check(self.lib.rsrgan_d_logits_hist(self.h, _ptr(out), self._stream()))
        return out

    def apply(self, net: int):
        self._training_only('apply')
        check(self.lib.rsrgan_apply(self.h, net, self._stream()))

    def profile_begin(self):
        check(self.lib.rsrgan_profile_begin(self.h))

    def profile_read_kind(self, kind):
        """(launches, total_us, algorithmic_flops) of kernel class `kind` since profile_begin; call before profile_read.
        1 = k_glstm_fwd, 2 = k_glstm_bwd (timed); count only (total_us = alg_flops = 0): 3 = k_glstm_fwd_dt, 4 = stand-alone discriminator
        forward launches (k_dlstm_fwd, k_dlstm_fwd_t, D(real) under RSRGAN_DPIPE), 5 = stand-alone k_dlstm_bwd, 6 = those of 5 with the
        weight gradients inside the launch, 7 = k_glstm_np_fwd, 8 = k_glstm_np_bwd"""
        n, us, fl = C.c_int32(), C.c_double(), C.c_double()
        check(self.lib.rsrgan_profile_read_kind(self.h, kind, C.byref(n), C.byref(us), C.byref(fl)))
        return n.value, us.value, fl.value

    def profile_read(self):
        """(launches, total_us, algorithmic_flops) of k_fwd_gates since profile_begin (synchronises)."""
        n, us, fl = C.c_int32(), C.c_double(), C.c_double()
        check(self.lib.rsrgan_profile_read(self.h, C.byref(n), C.byref(us), C.byref(fl)))
        return n.value, us.value, fl.value

    def device_status(self):
        """0, or 1 + the first workgroup of a persistent recurrence launch whose bounded wait expired (synchronises; clears the word)"""
        code = C.c_int32()
        check(self.lib.rsrgan_device_status(self.h, C.byref(code)))
        return code.value

    def set_dropout(self, keep_prob, seed=0):
        """tf.nn.dropout(h, keep_prob) after every hidden ReLU of the frame-level nets (dnn.py:116-121); `seed` = mask stream"""
        self._training_only("set_dropout")
        check(self.lib.rsrgan_set_dropout(self.h, float(keep_prob), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def profile_launches(self):
        """launches of the recurrence kernels the host issued since profile_begin (the profiled step runs eagerly)"""
        n = C.c_int64()
        check(self.lib.rsrgan_profile_launches(self.h, C.byref(n)))
        return n.value
