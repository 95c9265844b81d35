"""FrontEnd -- the device front end on the handle-free entries of the C ABI (include/rsrgan.h rsrgan_feat_*, rsrgan_wave_*; csrc/capi_front.cpp):
the op wrappers, the caches, the upload stream with its two hand-offs, and featurize / featurize_frames / denormalize / simulate /
synthesize on top of them.  No handle: HipEngine is one; so is a bare FrontEnd(), for callers without a model (io.wave_cmvn, the tools)."""
from __future__ import annotations

import contextlib
import weakref

import numpy as np
import torch

from ._lib import check
from .ops import OpEntries, _ptr


def _pcm_kind(who, pcm, kind):
    """the entries' `kind` of a PCM tensor: what the caller said, else what the dtype says (0 int16, 1 float32)"""
    if kind is not None:
        return kind
    if pcm.dtype not in (torch.int16, torch.float32):
        raise ValueError("%s: pcm must be int16 or float32, got %s" % (who, pcm.dtype))
    return 0 if pcm.dtype == torch.int16 else 1


class FrontEnd(OpEntries):
    def __init__(self, device=None, max_frames=None):
        """max_frames: the longest utterance featurize accepts (a model's handle has one; None: no limit)"""
        OpEntries.__init__(self, device)
        self.max_frames = max_frames
        self._upload_stream = None      # (lazy, upload_stream(): a process that never uses the front end opens no extra stream)
        self._vouched = {}              # id(tensor) -> (weak reference, version): the device tensors upload_ready lets pass
        self._cmvn_cache = {}           # (id(mean), id(stddev)) -> the host arrays and their fp64 device copies
        self._frame_pools = {}          # reader id -> the frame-level recipes' pool (featurize_frames)
        self._wave_cache = {}           # spec key -> window, twiddles (and the mel / DCT tables)
        self._reverb_tw = {}            # fft -> the reverberation's twiddles
        self._synth_work = None         # synthesize's `work`, kept and grown

    # -- the upload stream and its hand-offs ------------------------------------------------------------------------------------------
    def upload_stream(self):
        """the stream the feature front end uploads and runs on (featurize, featurize_frames, StreamBank)"""
        if self._upload_stream is None:
            self._upload_stream = torch.cuda.Stream(self.device)
        return self._upload_stream

    @contextlib.contextmanager
    def handoff(self, ready):
        """`with self.handoff(ready) as res:` -- the block runs with the upload stream current and puts the device tensors it made into the
        list `res`; on the way out they are handed to the current stream.  ready=False: by an event recorded on the upload stream, which
        the current stream waits for (no host wait).  ready=True: the host waits for the upload stream -- for THAT stream only -- and
        vouches for every result, so upload_ready lets it pass.  Either way the results' memory is held until the current stream is done
        with it (record_stream)."""
        us, res = self.upload_stream(), []
        with torch.cuda.stream(us):
            yield res
            if not ready:
                ev = torch.cuda.Event()
                ev.record(us)
        cur = torch.cuda.current_stream(self.device)
        if ready:
            us.synchronize()
            for t in res:
                self.vouch(t)
        else:
            cur.wait_event(ev)
        for t in res:
            t.record_stream(cur)

    def _put(self, a):
        """host array -> device tensor of the same dtype, queued on the current stream"""
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device, non_blocking=True)

    def _upload(self, a, int32):
        """host array (or a tensor elsewhere) -> contiguous int32 / float32 device tensor, queued on the current stream"""
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a) if int32 else np.ascontiguousarray(a, dtype=np.float32))
        t = t.to(self.device, non_blocking=True)
        return (t.to(torch.int32) if int32 else t.to(torch.float32)).contiguous()

    def upload_ready(self, a, int32=False) -> torch.Tensor:
        """Host array -> device tensor that is COMPLETE when this returns (copied on an upload stream of its own, which the host
        waits for -- not for the compute stream): what RSRGAN_DPIPE=1 asks of the labels and lengths of a D-run (include/rsrgan.h
        rsrgan_d_step), so that D(real) of the next step can run beside the previous step's tail.  Device tensors are converted on the
        upload stream if they need it, and waited for once per tensor object otherwise (see below)."""
        self.upload_stream()
        if isinstance(a, torch.Tensor) and a.device == self.device:
            want = torch.int32 if int32 else torch.float32
            if a.dtype == want and a.is_contiguous():
                # A device tensor nobody has vouched for may still be being written by a kernel queued on some stream.  The first time
                # this very tensor object (at this version: in-place writes through torch bump it) comes by, the host waits for the
                # device once; from then on it passes through untouched -- a resident batch fed again and again (bench.py, a cached
                # validation set) costs nothing, a freshly computed tensor per step costs a device wait per step (or RSRGAN_DPIPE=0).
                ent = self._vouched.get(id(a))
                if ent is None or ent[0]() is not a or ent[1] != a._version:
                    torch.cuda.synchronize(self.device)
                    self.vouch(a)
                return a
            # an int64 `lengths`, a float64 or strided label: the conversion is a KERNEL.  Queued on the current stream it would sit
            # behind that stream's backlog while D(real) on the library's side stream reads its output ahead of it -- so it runs on
            # the upload stream (the caller vouches for `a` itself being complete) and the host waits for it, as for a host array.
            with self.handoff(True) as res:
                res.append(a.to(want).contiguous())
            return res[0]
        with self.handoff(True) as res:
            res.append(self._upload(a, int32))
        return res[0]

    def vouch(self, t):
        """remember that device tensor `t` (this object, at this version) is complete: upload_ready lets it pass without a wait"""
        seen = self._vouched
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
        with self.handoff(False) as res:
            res.append(self._upload(a, int32))
        return res[0]

    # -- the feature front end on the device (include/rsrgan.h rsrgan_feat_batch, csrc/feat.hip) ---------------------------
    def op_feat_batch(self, raw, offsets, B, T, D, left, right, mean, stddev, out, lengths=None, raw_rows=None, stream=None):
        """rsrgan_feat_batch on caller-owned device tensors (raw [rows, D] f32, offsets [B + 1] i32, mean / stddev [D] f64 or None,
        out B * T * D * (left + 1 + right) f32, lengths [B] i32 or None), on `stream` (default: the current one)"""
        check(self.lib.rsrgan_feat_batch(_ptr(raw), raw.shape[0] if raw_rows is None else raw_rows, _ptr(offsets), B, T, D, left, right,
                                         _ptr(mean), _ptr(stddev), _ptr(out), _ptr(lengths), self._stream(stream)))

    def cmvn_device(self, mean, stddev, us):
        """the two CMVN vectors as fp64 device tensors, uploaded once per pair of host arrays (the cache holds the host arrays, so
        their ids stay theirs); (None, None) for no statistics"""
        if mean is None:
            return None, None
        cache = self._cmvn_cache
        ent = cache.get((id(mean), id(stddev)))
        if ent is None:
            host = [np.ascontiguousarray(v, np.float64).reshape(-1) for v in (mean, stddev)]
            with torch.cuda.stream(us):
                dev = [torch.from_numpy(h).to(self.device) for h in host]
            if len(cache) > 16:
                cache.clear()
            ent = cache[(id(mean), id(stddev))] = (mean, stddev, dev[0], dev[1])
        return ent[2], ent[3]

    def _check_tables(self, B, T, D, rows, offsets, mean, stddev, limit, packed=False):
        """what featurize refuses before any device work, for every kind of batch.  `packed`: the rows are an array of their own (not
        made from the offset table's last entry), so the table must also lie inside it.  Without max_frames there is no length limit."""
        if offsets.shape != (B + 1,) or B < 1 or T < 1 or rows < 1:
            raise ValueError("featurize: B = %d, T = %d, %d rows, %d offsets" % (B, T, rows, offsets.shape[0]))
        n = np.diff(offsets.astype(np.int64))
        if packed and (n.min() < 0 or offsets[0] < 0 or offsets[-1] > rows):
            raise ValueError("featurize: the offset table does not describe utterances inside the %d packed rows" % rows)
        if limit and self.max_frames is not None and max(int(n.max()), T) > self.max_frames:
            raise ValueError("featurize: an utterance of %d frames (T = %d) is longer than max_frames = %d" % (int(n.max()), T, self.max_frames))
        if mean is not None and (np.size(mean) != D or np.size(stddev) != D):
            raise ValueError("featurize: mean / stddev must hold D = %d entries, got %d / %d" % (D, np.size(mean), np.size(stddev)))

    def _splice(self, raw, off, B, T, D, left, right, dm, ds, us):
        """raw rows on the device -> [x [B, T, D * (left + 1 + right)] f32, lengths [B] i32]: rsrgan_feat_batch on `us`"""
        out = torch.empty(B, T, D * (left + 1 + right), dtype=torch.float32, device=self.device)
        ln = torch.empty(B, dtype=torch.int32, device=self.device)
        self.op_feat_batch(raw, off, B, T, D, left, right, dm, ds, out, ln, stream=us)
        return [out, ln]

    def featurize(self, packed, left=None, right=None, mean=None, stddev=None, ready=False, limit=True):
        """io.PackedBatch (raw frames + offsets) -> (x [B, T, D * (left + 1 + right)] f32, lengths [B] i32) on the device: CMVN, splice
        and padding in one kernel (csrc/feat.hip), bit for bit what io.features computes on the host.  left / right / mean / stddev
        default to what the batch carries.  The packed frames and the offset table travel on the engine's upload stream and the kernel
        runs there: ready=True waits for THAT stream only and vouches for the results (what upload_ready gives the labels and lengths of
        a D-run under RSRGAN_DPIPE=1); ready=False hands them over by event, as upload_async does (handoff).  ValueError before any device
        work if an utterance is longer than max_frames (limit=False: the caller cuts the result into chunks itself, as the chunked decode
        does; a bare FrontEnd() has no max_frames and no limit).  An io.CodedBatch (the archive's bytes: float, double or Kaldi-compressed
        matrices) is decoded on the device first (_featurize_coded), an io.WaveBatch (audio samples) becomes log-power-spectrum frames
        there first (_featurize_wave); everything else is the same."""
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
        data = packed.data
        if not isinstance(data, np.ndarray) or data.dtype != np.float32 or data.ndim != 2:
            raise ValueError("featurize: packed.data must be a float32 [rows, D] array")
        B, T, D = int(packed.shape[0]), int(packed.shape[1]), data.shape[1]
        offsets = np.ascontiguousarray(packed.offsets, np.int32)
        self._check_tables(B, T, D, data.shape[0], offsets, mean, stddev, limit, packed=True)
        us = self.upload_stream()
        dm, ds = self.cmvn_device(mean, stddev, us)
        with self.handoff(ready) as res:
            res += self._splice(self._put(data), self._put(offsets), B, T, D, left, right, dm, ds, us)
        return tuple(res)

    # -- the archive side (include/rsrgan.h rsrgan_feat_decode, csrc/feat.hip k_feat_decode) -----------------------------------
    def op_feat_decode(self, blob, seg, scale, offsets, B, D, mean, stddev, out, blob_bytes=None, out_rows=None, stream=None):
        """rsrgan_feat_decode on caller-owned device tensors (blob uint8, seg [B, 2] i64 = (byte offset, kind), scale [B, 2] f32 = (min,
        range), offsets [B + 1] i32, mean / stddev [D] f64 or None, out [rows, D] f32), on `stream` (default: the current one)"""
        check(self.lib.rsrgan_feat_decode(_ptr(blob), blob.numel() if blob_bytes is None else blob_bytes, _ptr(seg), _ptr(scale), _ptr(offsets),
                                          B, D, _ptr(mean), _ptr(stddev), _ptr(out), out.shape[0] if out_rows is None else out_rows,
                                          self._stream(stream)))

    def _featurize_coded(self, coded, left, right, mean, stddev, ready, limit):
        """featurize for an io.CodedBatch: the blob and the three tables travel on the upload stream, rsrgan_feat_decode turns them into
        normalised float32 rows [frames, D] and rsrgan_feat_batch (mean = NULL) splices and pads those -- the decode normalises, because the
        host path never rounds the decoded value to float32 before it does."""
        offsets = coded.offsets
        B, T, D = int(coded.shape[0]), int(coded.shape[1]), int(coded.dim)
        rows = int(offsets[-1]) if offsets.shape[0] else 0
        self._check_tables(B, T, D, rows, offsets, mean, stddev, limit)
        us = self.upload_stream()
        dm, ds = self.cmvn_device(mean, stddev, us)
        with self.handoff(ready) as res:
            dblob, dseg, dscale, off = self._put(coded.blob), self._put(coded.seg), self._put(coded.scale), self._put(offsets)
            raw = torch.empty(rows, D, dtype=torch.float32, device=self.device)
            self.op_feat_decode(dblob, dseg, dscale, off, B, D, dm, ds, raw, stream=us)
            res += self._splice(raw, off, B, T, D, left, right, None, None, us)
        return tuple(res)

    def _featurize_wave(self, wb, left, right, mean, stddev, ready, limit):
        """featurize for an io.WaveBatch: the samples and the two tables travel on the upload stream, wave_features writes the raw rows
        [frames, bins] the batch's spec asks for (rsrgan_feat_wave: LPS; rsrgan_feat_mfcc: MFCC or log-mel) and rsrgan_feat_batch
        normalises, splices and pads those."""
        offsets, spec = wb.offsets, wb.spec
        B, T, D = int(wb.shape[0]), int(wb.shape[1]), int(wb.dim)
        rows = int(offsets[-1]) if offsets.shape[0] else 0
        self._check_tables(B, T, D, rows, offsets, mean, stddev, limit)
        us = self.upload_stream()
        dm, ds = self.cmvn_device(mean, stddev, us)
        with self.handoff(ready) as res:
            if getattr(wb, "plan", None) is not None:
                # clean samples with a plan: reverberated on the device first (csrc/reverb.hip), float32 on the int16 scale
                pcm, dseg, _ = self.simulate(wb, stream=us)
                raw, off = self.wave_rows(pcm, dseg, B, offsets, rows, spec, us)
            else:
                raw, off = self.wave_features(wb.samples, wb.seg, offsets, rows, spec, us)
            res += self._splice(raw, off, B, T, D, left, right, dm, ds, us)
        return tuple(res)

    # -- the frame-level recipes' front end (include/rsrgan.h rsrgan_feat_frames, csrc/feat.hip k_feat_frames) ------------------
    def op_feat_frames(self, pool, picks, N, D, left, right, mean, stddev, out, pool_rows=None, stream=None):
        """rsrgan_feat_frames on caller-owned device tensors (pool [rows, D] f32, picks [N, 3] i32 = (row, lo, hi), mean / stddev [D] f64 or
        None, out N * D * (left + 1 + right) f32), on `stream` (default: the current one)"""
        check(self.lib.rsrgan_feat_frames(_ptr(pool), pool.shape[0] if pool_rows is None else pool_rows, _ptr(picks), N, D, left, right,
                                          _ptr(mean), _ptr(stddev), _ptr(out), self._stream(stream)))

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
        st = self._frame_pools.get(item.reader_id)
        if st is None:
            st = self._frame_pools[item.reader_id] = {"ledger": PoolLedger(item.reader_id), "x": None, "y": None, "items": 0, "uploads": 0,
                                                      "growths": 0}
        st["ledger"].admit(item)                                   # (raises before anything is queued)
        N, D, Dl, left, right = item.picks.shape[0], item.input_dim, item.label_dim, item.left, item.right
        us = self.upload_stream()
        mi = si = ml = sl = None
        if item.stats is not None:
            if any(np.size(v) != d for v, d in zip(item.stats, (D, D, Dl, Dl))):
                raise ValueError("featurize_frames: the statistics must hold %d / %d entries" % (D, Dl))
            mi, si = self.cmvn_device(item.stats[0], item.stats[1], us)
            ml, sl = self.cmvn_device(item.stats[2], item.stats[3], us)
        # EVERYTHING below is queued on the upload stream, item after item: pool growth, uploads, normalisation and the gathers.  Slot reuse
        # rests on that order alone: the reader hands a slot out again once its utterance's last frame was drawn, so an upload into a freed
        # slot belongs to a LATER item than the last gather that read the slot, and runs behind it on this stream.  The same order keeps a
        # grown pool's copy of the old rows behind every write to them and in front of every later read.
        with self.handoff(ready) as res:
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
            res += [x, lab]
        st["items"] += 1; st["uploads"] += len(item.uploads)
        return x, lab

    def frame_pool_readers(self):
        """the reader ids that have a pool here"""
        return list(self._frame_pools)

    def frame_pool_stats(self, reader_id):
        """{'pool_rows', 'bytes', 'items', 'uploads', 'growths'} of one reader's pool (None before its first item)"""
        st = self._frame_pools.get(reader_id)
        if st is None or st["x"] is None:
            return None
        return {"pool_rows": st["x"].shape[0], "bytes": (st["x"].numel() + st["y"].numel()) * 4, "items": st["items"], "uploads": st["uploads"],
                "growths": st["growths"]}

    def drop_frame_pool(self, reader_id):
        """forget a reader's pool (its device memory goes back to torch once the last batch gathered from it is consumed)"""
        self._frame_pools.pop(reader_id, None)

    # -- the live path's front end and the output side (include/rsrgan.h rsrgan_feat_stream / rsrgan_feat_denorm, csrc/feat.hip) ------
    def op_feat_stream(self, fresh, table, hist, B, H, T, D, left, right, mean, stddev, out, lengths=None, fresh_rows=None, stream=None):
        """rsrgan_feat_stream on caller-owned device tensors (fresh [rows, D] f32 or None, table [B, 6] i32 = (src, app0, napp, emit0, nemit,
        last), hist [B, H, D] f32, mean / stddev [D] f64 or None, out B * T * D * (left + 1 + right) f32, lengths [B] i32 or None), on
        `stream` (default: the current one)"""
        rows = (0 if fresh is None else fresh.shape[0]) if fresh_rows is None else fresh_rows
        check(self.lib.rsrgan_feat_stream(_ptr(fresh), rows, _ptr(table), _ptr(hist), B, H, T, D, left, right, _ptr(mean), _ptr(stddev),
                                          _ptr(out), _ptr(lengths), self._stream(stream)))

    def op_feat_denorm(self, y, lengths, B, T, D, mean, stddev, out, stream=None):
        """rsrgan_feat_denorm on caller-owned device tensors (y B * T * D f32, lengths [B] i32 or None, mean / stddev [D] f64, out B * T * D
        f64), on `stream` (default: the current one)"""
        check(self.lib.rsrgan_feat_denorm(_ptr(y), _ptr(lengths), B, T, D, _ptr(mean), _ptr(stddev), _ptr(out), self._stream(stream)))

    def denormalize(self, y, mean, stddev, lengths=None):
        """G(x) y [B, T, D] f32 on the device -> y * stddev + mean as [B, T, D] f64 on the device (rows from lengths[b] on are zero), on the
        current stream: bit for bit NumPy's result on the host copy.  mean / stddev: host arrays of D entries (uploaded once per pair)."""
        y = y.contiguous()
        B, T, D = y.shape
        if np.size(mean) != D or np.size(stddev) != D:
            raise ValueError("denormalize: mean / stddev must hold D = %d entries, got %d / %d" % (D, np.size(mean), np.size(stddev)))
        us = self.upload_stream()
        dm, ds = self.cmvn_device(mean, stddev, us)
        cur = torch.cuda.current_stream(self.device)
        cur.wait_stream(us)                                        # (the statistics' upload, the first time)
        out = torch.empty(B, T, D, dtype=torch.float64, device=self.device)
        self.op_feat_denorm(y, lengths, B, T, D, dm, ds, out)
        return out

    # -- the waveform side (include/rsrgan.h rsrgan_feat_wave, csrc/wave.hip k_feat_wave) -------------------------------------------
    def wave_frames_per_workgroup(self, P=512):
        """the consecutive frames of one utterance a workgroup of k_feat_wave takes (rsrgan_feat_wave_frames)"""
        return int(self.lib.rsrgan_feat_wave_frames(P))

    def op_feat_wave(self, pcm, seg, offsets, B, window, twiddle, out, N=400, S=160, P=512, preemph=0.97, kind=None, n_samples=None,
                     out_rows=None, stream=None):
        """rsrgan_feat_wave on caller-owned device tensors (pcm int16 or float32 [n], seg [B, 2] i64 = (first sample, count), offsets
        [B + 1] i32, window [N] f32, twiddle [P / 2, 2] f32, out [rows, P / 2 + 1] f32), on `stream` (default: the current one).  kind
        defaults to what pcm's dtype says."""
        kind = _pcm_kind("op_feat_wave", pcm, kind)
        check(self.lib.rsrgan_feat_wave(_ptr(pcm), kind, pcm.numel() if n_samples is None else n_samples, _ptr(seg), _ptr(offsets), B, N, S, P,
                                        preemph, _ptr(window), _ptr(twiddle), _ptr(out), out.shape[0] if out_rows is None else out_rows,
                                        self._stream(stream)))

    def op_feat_mfcc(self, pcm, seg, offsets, B, window, twiddle, mel_seg, mel_w, dct, out, N=400, S=160, P=512, preemph=0.97, M=None, ceps=None,
                     nnz=None, kind=None, n_samples=None, out_rows=None, stream=None):
        """rsrgan_feat_mfcc on caller-owned device tensors (pcm, seg, offsets, window, twiddle as op_feat_wave takes them; mel_seg [M, 3]
        i32, mel_w [nnz] f32, dct [C, M] f32 or None for log-mel output; out [rows, C or M] f32), on `stream` (default: the current one).
        M, ceps (the entry's C) and nnz default to what the tables' shapes say."""
        kind = _pcm_kind("op_feat_mfcc", pcm, kind)
        M = int(mel_seg.shape[0]) if M is None else M
        ceps = (0 if dct is None else int(dct.shape[0])) if ceps is None else ceps
        check(self.lib.rsrgan_feat_mfcc(_ptr(pcm), kind, pcm.numel() if n_samples is None else n_samples, _ptr(seg), _ptr(offsets), B, N, S, P,
                                        preemph, _ptr(window), _ptr(twiddle), _ptr(mel_seg), _ptr(mel_w), mel_w.numel() if nnz is None else nnz,
                                        M, _ptr(dct), ceps, _ptr(out), out.shape[0] if out_rows is None else out_rows, self._stream(stream)))

    def wave_tables(self, spec, us):
        """the window and the twiddles of a framing as fp32 device tensors: built on the host in float64, rounded once, uploaded at first use
        and kept per engine (as cmvn_device keeps the statistics).  For an io.wave.MfccSpec three more follow: mel_seg, mel_w and the DCT
        (None for log-mel output)."""
        from .io.wave import dct_table, mel_table, twiddle_table, window_table
        cache = self._wave_cache
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

    _wave_tables = wave_tables      # (the name it had while it was private: callers written against it keep working)

    def wave_features(self, samples, seg, offsets, rows, spec, us):
        """host samples and tables -> (raw feature rows [rows, spec.bins], the offset table) on the device: LPS for a WaveSpec
        (rsrgan_feat_wave), MFCC or log-mel for an MfccSpec (rsrgan_feat_mfcc): the spec's type says which features come out.  The
        uploads and the launch are queued on `us` (the caller is inside `with torch.cuda.stream(us)`)"""
        return self.wave_rows(self._put(samples), self._put(seg), int(seg.shape[0]), offsets, rows, spec, us)

    def wave_rows(self, pcm, dseg, B, offsets, rows, spec, us):
        """wave_features on samples and segments that are on the device already"""
        tabs = self.wave_tables(spec, us)
        off = self._put(offsets)
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
        kind = _pcm_kind("op_wave_reverb", pcm, kind)
        R = 0 if rir_seg is None else int(rir_seg.shape[0])
        V = 0 if noise_seg is None else int(noise_seg.shape[0])
        check(self.lib.rsrgan_wave_reverb(_ptr(pcm), kind, pcm.numel(), _ptr(seg), _ptr(rir), 0 if rir is None else rir.numel(), _ptr(rir_seg),
                                          _ptr(noise), 0 if noise is None else noise.numel(), _ptr(noise_seg), _ptr(noise_pow), _ptr(sel),
                                          _ptr(snr), B, R, V, fft, _ptr(twiddle), (1 if shift else 0) | (2 if normalize else 0), _ptr(out),
                                          out.numel(), _ptr(out_seg), _ptr(gains), _ptr(work), work.numel() * work.element_size(),
                                          self._stream(stream)))

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
        if fft not in self._reverb_tw:
            with torch.cuda.stream(us):
                self._reverb_tw[fft] = torch.from_numpy(twiddle_table(2 * fft)).to(self.device)
        return self._reverb_tw[fft]

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
        with torch.cuda.stream(us):
            rir, rseg, noise, nseg, npow = self.reverb_bank(bank, us)
            tw = self._reverb_twiddle(spec.fft, us)
            pcm, dseg, sel, snr, oseg = self._put(wb.samples), self._put(wb.seg), self._put(plan.sel), self._put(plan.snr), self._put(out_seg)
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
        kind = _pcm_kind("op_wave_synth", pcm, kind)
        check(self.lib.rsrgan_wave_synth(_ptr(pcm), kind, pcm.numel(), _ptr(seg), _ptr(offsets), _ptr(lps),
                                         lps.shape[0] if lps_rows is None else lps_rows, B, N, S, P, preemph, _ptr(window), _ptr(twiddle),
                                         _ptr(out), out.numel(), _ptr(out_seg), _ptr(work), work.numel() * work.element_size(),
                                         self._stream(stream)))

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
        if lps.is_cuda:
            us.wait_stream(torch.cuda.current_stream(self.device))           # (the rows were made on the caller's stream)
            lps.record_stream(us)
        with torch.cuda.stream(us):
            win, tw = self.wave_tables(spec, us)
            work = self._synth_work
            if work is None or work.numel() < need:
                work = self._synth_work = torch.empty(need, dtype=torch.uint8, device=self.device)
            lps = lps.to(self.device, torch.float32, non_blocking=True).contiguous()
            out = torch.empty(total, dtype=torch.float32, device=self.device)
            self.op_wave_synth(self._put(wb.samples), self._put(wb.seg), self._put(wb.offsets), lps, B, win, tw, out, self._put(wb.seg), work,
                               spec.frame_length, spec.frame_shift, spec.padded, spec.preemph, stream=us)
        return out, wb.seg
