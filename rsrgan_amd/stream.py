"""Decoding with the generator's carried state (GAN_RNN.forward_stream): one live stream enhanced while it arrives
(StreamEnhancer), many utterances decoded side by side in the rows of one handle (decode_streams), and many live streams enhanced side
by side, with the splice and the de-normalising on the device if asked (StreamBank, decode_live).  The live classes take audio as well
(push_audio, decode_live_audio): samples become log-power-spectrum frames on the host (io/wave.py) or on the device (csrc/wave.hip).

All are host logic around `model.forward_stream(inputs, lengths, reset)`: the model keeps, per batch row, the recurrent
state of every generator layer between calls, so an utterance is a sequence of chunks of at most the handle's max_frames
frames.  Everything per frame (CMVN, the splice, the input and output FC, de-normalising) does not depend on how the
utterance was cut, and the recurrence hands its fp32 state over unchanged: what comes out equals the whole-utterance
decode of run_gan_rnn.decode."""
from __future__ import annotations

from typing import Iterable, Iterator, Optional

import numpy as np


def _model_dims(model):
    eng = getattr(model, "engine", None)
    batch = int(getattr(model, "batch_size", None) or getattr(eng, "batch_size"))
    cap = getattr(eng, "max_frames", None) or getattr(model, "max_frames", None)
    return batch, (int(cap) if cap else None)


def _on_device(a):
    """a torch tensor (an utterance the device-side front end produced) rather than a host array"""
    return hasattr(a, "new_zeros") and hasattr(a, "detach")


def _wave_spec(wave):
    from .io.wave import DEFAULT
    return DEFAULT if wave is None else wave


def _take_frames(pending, samples, spec):
    """(buf, keep): `pending` followed by the new `samples`, and the tail of it that belongs to no complete frame yet -- what stays on the
    host for the next push, at most frame_length - 1 samples.  int16 stays int16; anything else makes the row float32."""
    from .io.wave import as_pcm, num_frames
    x = as_pcm(samples)
    if pending is not None and pending.shape[0]:
        x = np.concatenate([pending, x]) if pending.dtype == x.dtype else np.concatenate([pending.astype(np.float32), x.astype(np.float32)])
    F = num_frames(x.shape[0], spec)
    return x, (x[F * spec.frame_shift:] if F else x)


class _DeviceRows(object):
    """`count` consecutive rows, from `start`, of a frame tensor that is already on the device (StreamBank.push_audio): what a round
    appends for a row in place of host frames"""

    def __init__(self, start, count):
        self.start, self.shape = int(start), (int(count),)


class StreamEnhancer(object):
    """One live stream on batch row 0 of `model`.

        enh = StreamEnhancer(model, cmvn, left_context=5, right_context=5, chunk=100)
        for frames in microphone:                 # [n, input_dim], any n >= 0
            out = enh.push(frames)                # [k, output_dim]: the frames that are final now
        out = enh.flush()                         # the rest; the enhancer is ready for the next utterance

    It owns what run_gan_rnn.decode does around the forward call: CMVN of the inputs (float64, make_tfrecords.py:84-87), the
    splice (io.features.splice_feats: frame i needs frames i - left .. i + right, so the last `right_context` frames are held
    back until their right context exists; before the first and after the last frame of the utterance that frame is repeated)
    and de-normalising with the label CMVN.  The concatenation of everything push() and flush() return for an utterance equals
    decode()'s matrix for it, however the input was cut into pushes.  `chunk`: frames per forward call (at most the handle's
    max_frames, the default).  `device_features=True`: the splice and the de-normalising run on the device; the enhancer is then a
    one-row StreamBank (raw frames are shipped as float32)."""

    def __init__(self, model, cmvn=None, left_context=0, right_context=0, chunk=None, device_features=False, wave=None):
        # device_features: the splice and the de-normalising run on the device -- a one-row StreamBank serves push, flush and reset
        self._bank = StreamBank(model, cmvn, left_context, right_context, chunk, streams=1, device_features=True, wave=wave) if device_features else None
        self.wave = _wave_spec(wave)                # the framing push_audio turns samples into frames with
        self.model, self.cmvn = model, cmvn
        self.left, self.right = int(left_context), int(right_context)
        if self.left < 0 or self.right < 0:
            raise ValueError("contexts must be >= 0")
        self.batch, cap = _model_dims(model)
        self.chunk = int(chunk) if chunk else (cap or 100)
        if self.chunk <= 0 or (cap is not None and self.chunk > cap):
            raise ValueError("chunk=%d outside (0, max_frames=%s]" % (self.chunk, cap))
        self.reset()

    def reset(self):
        """forget the utterance in flight: the next push starts a new one from the zero state"""
        if self._bank is not None:
            self._bank.reset()
        self._hist = None           # normalised frames [base, n) of the utterance (float64)
        self._base = 0               # utterance index of _hist[0]
        self._n = 0                  # frames received
        self._next = 0               # next frame to enhance
        self._fresh = True           # the carried state of row 0 is zeroed with the next forward call
        self._pcm = None             # push_audio: the samples that belong to no complete frame yet

    # -- pieces -------------------------------------------------------------------------
    def _normalise(self, frames):
        x = np.array(frames, np.float64)
        if x.ndim != 2:
            raise ValueError("frames must be [n, input_dim], got %s" % (x.shape,))
        if self.cmvn is not None:
            x = (x - self.cmvn["mean_inputs"]) / self.cmvn["stddev_inputs"]
        return x

    def _spliced(self, start, stop):
        """splice_feats rows [start, stop) of the utterance as far as it is known (the last known frame stands in beyond it:
        only flush() asks for such rows, when that frame is the utterance's last)"""
        idx = np.arange(start, stop)
        last = self._n - 1
        take = lambda j: self._hist[np.clip(j, 0, last) - self._base]
        parts = [take(idx - i) for i in range(self.left, 0, -1)]
        parts.append(take(idx))
        parts += [take(idx + i) for i in range(1, self.right + 1)]
        return np.concatenate(parts, 1).astype(np.float32)

    def _enhance(self, stop):
        """frames [_next, stop) through the generator, `chunk` at a time"""
        outs = []
        while self._next < stop:
            n = min(self.chunk, stop - self._next)
            x1 = self._spliced(self._next, self._next + n)
            x = np.zeros((self.batch, n, x1.shape[1]), np.float32)
            x[0] = x1
            ln = np.zeros(self.batch, np.int32)
            ln[0] = n
            y = np.asarray(self.model.forward_stream(x, ln, reset=[0] if self._fresh else None))[0, :n]
            self._fresh = False
            if self.cmvn is not None:
                y = y * self.cmvn["stddev_labels"] + self.cmvn["mean_labels"]
            outs.append(y)
            self._next += n
        # frames below _next - left are never read again
        keep = max(self._base, min(self._next - self.left, self._n - 1))
        if self._hist is not None and keep > self._base:
            self._hist = self._hist[keep - self._base:]
            self._base = keep
        return outs

    def _empty(self):
        d = getattr(self.model, "output_dim", None) or getattr(getattr(self.model, "engine", None), "output_dim", 0)
        return np.zeros((0, int(d)), np.float64 if self.cmvn is not None else np.float32)

    # -- the interface --------------------------------------------------------------------
    def push(self, frames):
        if self._bank is not None:
            return self._bank.push({0: frames})[0]
        x = self._normalise(frames)
        if x.shape[0]:
            self._hist = x if self._hist is None else np.concatenate([self._hist, x], 0)
            self._n += x.shape[0]
        outs = self._enhance(self._n - self.right) if self._n - self.right > self._next else []
        return np.concatenate(outs, 0) if outs else self._empty()

    def push_audio(self, samples):
        """push for audio: `samples` [n] (int16 PCM, or floats on that scale) of the utterance, any n >= 0.  The frames the samples
        received so far complete (io.wave: 400 samples every 160) are pushed; the samples that belong to no complete frame yet -- at most
        frame_length - 1 -- wait for the next call.  flush() and reset() drop them: a frame is never made of fewer samples."""
        if self._bank is not None:
            return self._bank.push_audio({0: samples})[0]
        from .io.wave import lps_from_wave
        buf, keep = _take_frames(self._pcm, samples, self.wave)
        self._pcm = keep
        return self.push(lps_from_wave(buf, spec=self.wave))

    def flush(self):
        """the end of the utterance: the held-back frames, their right context filled with the last frame"""
        if self._bank is not None:
            return self._bank.flush([0])[0]
        outs = self._enhance(self._n) if self._n > self._next else []
        out = np.concatenate(outs, 0) if outs else self._empty()
        self.reset()
        return out


def _raw_dim(model, C):
    """the width of a raw frame: the generator's input width over the number of spliced frames (None if the model does not say)"""
    eng = getattr(model, "engine", None)
    d = getattr(eng, "input_dim", None) or getattr(model, "input_dim", None) or getattr(getattr(model, "cfg", None), "input_dim", None)
    return int(d) // C if d and int(d) % C == 0 else None


class StreamBank(object):
    """Many live streams, one per batch row of `model`: the live form of decode_streams.

        bank = StreamBank(model, cmvn, left_context=5, right_context=5, chunk=10, streams=32, device_features=True)
        outs = bank.push({row: frames, ...})      # {row: [k, output_dim]}: the frames of each pushed row that are final now
        outs = bank.flush(rows)                   # ends those rows' utterances (default: all busy rows); their next push starts a new one
        bank.reset(rows)                          # forgets utterances in flight

    Per row it is StreamEnhancer: CMVN of the inputs, the splice with the last `right_context` frames held back until their right
    context exists, de-normalising with the label CMVN.  One push or flush advances every row that has work in the SAME forward_stream
    calls: the work is cut into rounds; in a round a row takes in at most `chunk` of its new frames and enhances at most `chunk` frames;
    rows without work rest with length 0; a row that begins an utterance is named in `reset=` of its first call.

    The ring.  Per row, n frames have arrived and frames [0, next) are enhanced.  Outside a round n - next <= right_context (a push
    enhances everything whose right context exists; shown below for every round).  A round appends a <= chunk frames, n' = n + a, and
    enhances frames [next, next + k), k = min(chunk, n' - right - next) on a push (k = min(chunk, n' - next) on a flush, where a = 0).
    n' - next <= right + chunk, so on a push k = n' - right - next whenever that is positive and n' - (next + k) <= right again.  The
    round reads frames next - left .. min(next + k - 1 + right, n' - 1): all of them lie in [next - left, n' - 1], a window of
    (n' - next) + left <= left + chunk + right frames; frames below next - left are dead.  Hence the ring holds

        H = left_context + chunk + right_context

    frames per row, utterance frame j in slot j mod H, and H is the least such size: a row that holds `right` frames and takes in
    `chunk` more reads a window of exactly H.  Before each round the window invariant of rsrgan_feat_stream is ASSERTED for every row
    from its table entry (last - (emit0 - left) + 1 <= H, emit0 - left <= app0, app0 + napp - 1 <= last), on both paths.

    device_features=False: the host arithmetic of StreamEnhancer for every row (float64 CMVN, the splice, one rounding to float32; the
    [batch, T, D * C] batch is uploaded and the whole output copied back).  device_features=True: one ring [batch, H, D] per bank on the
    device; per round the packed new raw frames and the table travel on the engine's upload stream, rsrgan_feat_stream runs there and
    hands the spliced batch to forward_stream by event (as HipEngine.featurize does), rsrgan_feat_denorm runs on the result and only each
    row's k x output_dim doubles are copied back.  The two paths make the same forward_stream calls on the same bits.  Without CMVN
    nothing is normalised or de-normalised and the output is float32.  ValueError before any device work: a row outside [0, streams),
    frames that are not [n, input_dim], device_features=True on a model whose engine has no op_feat_stream."""

    def __init__(self, model, cmvn=None, left_context=0, right_context=0, chunk=None, streams=None, device_features=False, wave=None):
        self.model, self.cmvn = model, cmvn
        self.wave = _wave_spec(wave)                                       # the framing push_audio turns samples into frames with
        self.left, self.right = int(left_context), int(right_context)
        if self.left < 0 or self.right < 0:
            raise ValueError("contexts must be >= 0")
        self.batch, cap = _model_dims(model)
        self.chunk = int(chunk) if chunk else (cap or 100)
        if self.chunk <= 0 or (cap is not None and self.chunk > cap):
            raise ValueError("chunk=%d outside (0, max_frames=%s]" % (self.chunk, cap))
        self.streams = self.batch if streams is None else int(streams)
        if not 0 < self.streams <= self.batch:
            raise ValueError("streams=%d outside (0, batch_size=%d]" % (self.streams, self.batch))
        self.device_features = bool(device_features)
        if self.device_features and not hasattr(getattr(model, "engine", None), "op_feat_stream"):
            raise ValueError("device_features=True needs an engine with a device-side streaming front end (HipEngine.op_feat_stream)")
        self.ring_frames = self.left + self.chunk + self.right             # H (the class docstring derives it)
        self.dim = _raw_dim(model, self.left + 1 + self.right)             # (None: the first push fixes it)
        self._stats = None if cmvn is None else {k: np.ascontiguousarray(cmvn[k], np.float64).reshape(-1) for k in
                                                 ("mean_inputs", "stddev_inputs", "mean_labels", "stddev_labels")}
        self._n = np.zeros(self.streams, np.int64)                         # frames received
        self._next = np.zeros(self.streams, np.int64)                      # next frame to enhance
        self._fresh = np.ones(self.streams, bool)                          # the row's carried state is zeroed with its next forward call
        self._hist = [None] * self.streams                                 # host path: normalised frames [base, n) (float64)
        self._base = np.zeros(self.streams, np.int64)
        self._ring, self._pinned = None, {}                                # device path
        self._pcm = [None] * self.streams                                  # push_audio: the samples that belong to no complete frame yet
        self.counters = {"rounds": 0, "calls": 0, "bytes_up": 0, "bytes_down": 0}      # bytes: host <-> device, both paths

    # -- the interface --------------------------------------------------------------------
    def reset(self, rows=None):
        """forget the utterances in flight on `rows` (default: all): their next push starts a new one from the zero state"""
        for r in (range(self.streams) if rows is None else self._rows(rows)):
            self._n[r] = self._next[r] = self._base[r] = 0
            self._fresh[r] = True
            self._hist[r] = None
            self._pcm[r] = None

    def push(self, frames_by_row):
        work = {}
        for r, frames in frames_by_row.items():
            r = self._rows([r])[0]
            x = np.asarray(frames)
            if x.ndim != 2 or (self.dim is not None and x.shape[1] != self.dim) or x.shape[1] < 1:
                raise ValueError("frames of row %d must be [n, input_dim%s], got %s" % (r, "" if self.dim is None else "=%d" % self.dim, x.shape))
            work[r] = x
        if self.dim is None and work:
            dims = {x.shape[1] for x in work.values()}
            if len(dims) != 1:
                raise ValueError("frames of different widths in one push: %s" % sorted(dims))
            self.dim = dims.pop()
        # (the device path ships raw float32 frames; the host path normalises in float64 whatever arrives, as StreamEnhancer does)
        work = {r: np.ascontiguousarray(x, np.float32 if self.device_features else np.float64) for r, x in work.items()}
        return self._rounds({r: x.shape[0] for r, x in work.items()}, lambda r, lo, n: work[r][lo:lo + n])

    def _rounds(self, count, piece, dev=None):
        """a push cut into rounds: row r has count[r] new frames, piece(r, lo, n) are frames [lo, lo + n) of them as a round appends
        them -- host frames, or _DeviceRows of the frame tensor `dev`"""
        outs, pos = {r: [] for r in count}, {r: 0 for r in count}
        while True:
            app, emit = {}, {}
            for r, total in count.items():
                a = min(self.chunk, total - pos[r])
                k = min(self.chunk, int(self._n[r]) + a - self.right - int(self._next[r]))
                if a > 0:
                    app[r] = piece(r, pos[r], a)
                    pos[r] += a
                if k > 0:
                    emit[r] = k
            if not app and not emit:
                break
            for r, y in self._round(app, emit, dev).items():
                outs[r].append(y)
        return {r: np.concatenate(o, 0) if o else self._empty() for r, o in outs.items()}

    def push_audio(self, samples_by_row):
        """push for audio: {row: samples [n]} (int16 PCM, or floats on that scale), any n >= 0.  Per row the host keeps only the samples
        that belong to no complete frame yet (at most frame_length - 1); the frames this call completes are enhanced as push enhances
        them.  device_features=False: io.wave.lps_from_wave on the host, then push.  device_features=True: the samples of the completed
        frames go up once, ONE rsrgan_feat_wave launch writes every row's new log-power-spectrum frames into one device tensor, and the
        rounds' table entries (`src`) point into it: no frame visits the host.  flush() and reset() drop a row's pending samples."""
        from .io.wave import lps_from_wave, num_frames
        spec = self.wave
        if self.dim is not None and self.dim != spec.bins:
            raise ValueError("push_audio makes frames of %d bins, the bank's frames have %d" % (spec.bins, self.dim))
        if self.device_features and not hasattr(self.model.engine, "wave_features"):
            raise ValueError("push_audio with device_features=True needs an engine with a device-side waveform front end (HipEngine.op_feat_wave)")
        taken = {}
        for r, x in samples_by_row.items():
            r = self._rows([r])[0]
            taken[r] = _take_frames(self._pcm[r], x, spec)                 # (raises before any row's state changes)
        for r, (_, keep) in taken.items():
            self._pcm[r] = keep
        if not self.device_features:
            return self.push({r: lps_from_wave(buf, spec=spec) for r, (buf, _) in taken.items()})
        if self.dim is None and taken:
            self.dim = spec.bins
        N, S = spec.frame_length, spec.frame_shift
        count = {r: num_frames(buf.shape[0], spec) for r, (buf, _) in taken.items()}
        rows = [r for r in sorted(count) if count[r] > 0]
        if not rows:
            return self._rounds(count, None)
        # one blob, one launch: row r's frames are rows base[r] .. base[r] + count[r] - 1 of `lps`
        spans = [taken[r][0][:(count[r] - 1) * S + N] for r in rows]
        if len({s.dtype for s in spans}) > 1:
            spans = [s.astype(np.float32) for s in spans]
        seg = np.zeros((len(rows), 2), np.int64)
        seg[:, 1] = [s.shape[0] for s in spans]
        seg[1:, 0] = np.cumsum(seg[:-1, 1])
        offsets = np.zeros(len(rows) + 1, np.int32)
        offsets[1:] = np.cumsum([count[r] for r in rows])
        base = {r: int(offsets[i]) for i, r in enumerate(rows)}
        blob = np.concatenate(spans)
        import torch
        eng = self.model.engine
        us = eng.upload_stream()
        with torch.cuda.stream(us):                                        # (the rounds read `lps` on this stream too: no other order is needed)
            lps, _ = eng.wave_features(blob, seg, offsets, int(offsets[-1]), spec, us)
        self.counters["bytes_up"] += blob.nbytes + seg.nbytes + offsets.nbytes
        return self._rounds(count, lambda r, lo, n: _DeviceRows(base[r] + lo, n), dev=lps)

    def flush(self, rows=None):
        """the end of the utterances on `rows` (default: every row with an utterance in flight): the held-back frames, their right
        context filled with the last frame"""
        rows = [r for r in range(self.streams) if self._n[r] > 0] if rows is None else self._rows(rows)
        outs = {r: [] for r in rows}
        while True:
            emit = {r: min(self.chunk, int(self._n[r] - self._next[r])) for r in rows if self._n[r] > self._next[r]}
            if not emit:
                break
            for r, y in self._round({}, emit).items():
                outs[r].append(y)
        self.reset(rows)
        return {r: np.concatenate(o, 0) if o else self._empty() for r, o in outs.items()}

    # -- pieces -------------------------------------------------------------------------
    def _rows(self, rows):
        rows = [int(r) for r in rows]
        for r in rows:
            if not 0 <= r < self.streams:
                raise ValueError("row %d outside [0, streams=%d)" % (r, self.streams))
        return rows

    def _empty(self):
        d = getattr(self.model, "output_dim", None) or getattr(getattr(self.model, "engine", None), "output_dim", 0)
        return np.zeros((0, int(d)), np.float64 if self.cmvn is not None else np.float32)

    def _on_stream(self):
        import contextlib
        on = getattr(getattr(self.model, "engine", None), "on_stream", None)
        return on() if on is not None else contextlib.nullcontext()

    def _round(self, app, emit, dev=None):
        """one round: `app` {row: new frames (at most chunk)} are taken in, `emit` {row: k} frames [next, next + k) are enhanced in one
        forward_stream call.  Returns {row: [k, output_dim]}.  `dev` (push_audio's device path): the new frames are rows of this device
        tensor, `app` {row: _DeviceRows}, and the table's `src` entries point into it instead of into a packed upload."""
        table = np.zeros((self.batch, 6), np.int32)                        # (src, app0, napp, emit0, nemit, last) of rsrgan_feat_stream
        table[:, 5] = -1
        src, H = 0, self.ring_frames
        for r in range(self.streams):
            a = app[r].shape[0] if r in app else 0
            table[r] = (app[r].start if dev is not None and r in app else src, self._n[r], a, self._next[r], emit.get(r, 0), self._n[r] + a - 1)
            src += a
        for r in set(app) | set(emit):
            _, app0, napp, emit0, nemit, last = (int(v) for v in table[r])
            if last - (emit0 - self.left) + 1 > H or emit0 - self.left > app0 or app0 + napp - 1 > last or emit0 + nemit - 1 > last:
                raise AssertionError("row %d: frames %d .. %d do not fit a ring of %d (the window invariant of rsrgan_feat_stream)"
                                     % (r, emit0 - self.left, last, H))
        if dev is not None:
            fresh = dev if app else dev[:0]
        else:
            fresh = np.concatenate([app[r] for r in sorted(app)], 0) if app else np.zeros((0, self.dim), np.float32 if self.device_features else np.float64)
        T = max(1, max(emit.values()) if emit else 0)
        outs = {}
        with self._on_stream():
            x, ln = (self._featurize_device if self.device_features else self._featurize_host)(table, fresh, T)
            for r in app:
                self._n[r] += app[r].shape[0]
            self.counters["rounds"] += 1
            if emit:
                begin = [r for r in sorted(emit) if self._fresh[r]]
                y = self.model.forward_stream(x, ln, reset=begin or None)
                self.counters["calls"] += 1
                for r in emit:
                    self._fresh[r] = False
                    self._next[r] += emit[r]
                outs = (self._collect_device if self.device_features else self._collect_host)(y, ln, emit)
        return outs

    # host path: StreamEnhancer's arithmetic per row
    def _featurize_host(self, table, fresh, T):
        x = np.zeros((self.batch, T, self.dim * (self.left + 1 + self.right)), np.float32)
        for r in range(self.streams):
            src, app0, napp, emit0, nemit, last = (int(v) for v in table[r])
            if napp > 0:
                new = fresh[src:src + napp]
                if self.cmvn is not None:
                    new = (new - self.cmvn["mean_inputs"]) / self.cmvn["stddev_inputs"]
                self._hist[r] = new if self._hist[r] is None else np.concatenate([self._hist[r], new], 0)
            if nemit > 0:
                idx = np.arange(emit0, emit0 + nemit)
                take = lambda j: self._hist[r][np.clip(j, 0, last) - self._base[r]]
                parts = [take(idx - i) for i in range(self.left, 0, -1)]
                parts.append(take(idx))
                parts += [take(idx + i) for i in range(1, self.right + 1)]
                x[r, :nemit] = np.concatenate(parts, 1).astype(np.float32)
                # frames below next - left are never read again
                keep = max(int(self._base[r]), min(emit0 + nemit - self.left, last))
                if keep > self._base[r]:
                    self._hist[r] = self._hist[r][keep - int(self._base[r]):]
                    self._base[r] = keep
        ln = np.clip(table[:, 4], 0, T).astype(np.int32)
        self.counters["bytes_up"] += x.nbytes + ln.nbytes
        return x, ln

    def _collect_host(self, y, ln, emit):
        y = np.asarray(y)
        self.counters["bytes_down"] += y.shape[0] * y.shape[1] * y.shape[2] * 4          # (the handle's output is float32; all of it comes back)
        outs = {}
        for r, k in emit.items():
            o = y[r, :k]
            outs[r] = o * self.cmvn["stddev_labels"] + self.cmvn["mean_labels"] if self.cmvn is not None else np.array(o)
        return outs

    # device path: the ring, rsrgan_feat_stream and rsrgan_feat_denorm
    def _featurize_device(self, table, fresh, T):
        import torch
        eng = self.model.engine
        B, H, D = self.batch, self.ring_frames, self.dim
        us = eng.upload_stream()
        st = self._stats
        dm, ds = eng.cmvn_device(st["mean_inputs"], st["stddev_inputs"], us) if st is not None else (None, None)
        # everything that touches the ring is queued on the upload stream, round after round: that order alone is what lets a round overwrite
        # the slots of frames the round before still read
        with eng.handoff(False) as res:
            if self._ring is None:
                self._ring = torch.zeros(B, H, D, dtype=torch.float32, device=eng.device)
            if _on_device(fresh):                                          # (push_audio: the frames were made on the device, on this stream)
                fr, up = (fresh if fresh.shape[0] else None), 0
            else:
                fr, up = (torch.from_numpy(fresh).to(eng.device, non_blocking=True) if fresh.shape[0] else None), fresh.nbytes
            tb = torch.from_numpy(table).to(eng.device, non_blocking=True)
            out = torch.empty(B, T, D * (self.left + 1 + self.right), dtype=torch.float32, device=eng.device)
            ln = torch.empty(B, dtype=torch.int32, device=eng.device)
            eng.op_feat_stream(fr, tb, self._ring, B, H, T, D, self.left, self.right, dm, ds, out, ln, stream=us)
            res += [out, ln]
        self.counters["bytes_up"] += up + table.nbytes
        return out, ln

    def _collect_device(self, y, ln, emit):
        import torch
        eng = self.model.engine
        st = self._stats
        z = eng.denormalize(y, st["mean_labels"], st["stddev_labels"], lengths=ln) if st is not None else y.contiguous()
        host = self._pinned.get(z.dtype)
        if host is None:
            host = self._pinned[z.dtype] = torch.empty(self.batch, self.chunk, z.shape[2], dtype=z.dtype, pin_memory=True)
        for r, k in emit.items():
            host[r, :k].copy_(z[r, :k], non_blocking=True)
            self.counters["bytes_down"] += k * z.shape[2] * z.element_size()
        torch.cuda.current_stream(eng.device).synchronize()
        return {r: host[r, :k].numpy().copy() for r, k in emit.items()}


def decode_live(bank: StreamBank, utterances: Iterable[np.ndarray], push: int) -> Iterator[np.ndarray]:
    """decode_streams through the live path: every utterance (RAW frames [T_i, input_dim]) arrives as pushes of `push` frames on one row
    of `bank` and ends with a flush; a row whose utterance has ended takes the next one.  Yields the enhanced utterances
    [T_i, output_dim] (de-normalised if the bank has CMVN) in input order."""
    push = int(push)
    if push <= 0:
        raise ValueError("push=%d must be positive" % push)
    source = enumerate(utterances)
    rows = [None] * bank.streams                 # per row: [index, frames, position, outputs]
    done, next_out, exhausted = {}, 0, False
    while True:
        for r in range(bank.streams):
            while rows[r] is None and not exhausted:
                try:
                    i, x = next(source)
                except StopIteration:
                    exhausted = True
                    break
                x = np.asarray(x)
                if x.ndim != 2:
                    raise ValueError("utterance %d must be [T, D], got %s" % (i, x.shape))
                if x.shape[0] == 0:
                    done[i] = bank._empty()
                    continue
                rows[r] = [i, x, 0, []]
        busy = [r for r in range(bank.streams) if rows[r] is not None]
        if busy:
            for r, y in bank.push({r: rows[r][1][rows[r][2]:rows[r][2] + push] for r in busy}).items():
                rows[r][3].append(y)
                rows[r][2] += push
            ended = [r for r in busy if rows[r][2] >= rows[r][1].shape[0]]
            for r, y in (bank.flush(ended) if ended else {}).items():
                done[rows[r][0]] = np.concatenate(rows[r][3] + [y], 0)
                rows[r] = None
        while next_out in done:
            yield done.pop(next_out)
            next_out += 1
        if not busy and exhausted:
            return


def decode_live_audio(bank: StreamBank, utterances: Iterable[np.ndarray], push_samples: int) -> Iterator[np.ndarray]:
    """decode_live from audio: every utterance (SAMPLES [n_i], int16 PCM or floats on that scale) arrives as pushes of `push_samples`
    samples on one row of `bank` (StreamBank.push_audio) and ends with a flush.  Yields the enhanced utterances [F_i, output_dim], F_i the
    frames the samples make (io.wave.num_frames), in input order."""
    push = int(push_samples)
    if push <= 0:
        raise ValueError("push_samples=%d must be positive" % push)
    source = enumerate(utterances)
    rows = [None] * bank.streams                 # per row: [index, samples, position, outputs]
    done, next_out, exhausted = {}, 0, False
    while True:
        for r in range(bank.streams):
            while rows[r] is None and not exhausted:
                try:
                    i, x = next(source)
                except StopIteration:
                    exhausted = True
                    break
                x = np.asarray(x)
                if x.ndim != 1:
                    raise ValueError("utterance %d must be a 1-D array of samples, got %s" % (i, x.shape))
                if x.shape[0] == 0:
                    done[i] = bank._empty()
                    continue
                rows[r] = [i, x, 0, []]
        busy = [r for r in range(bank.streams) if rows[r] is not None]
        if busy:
            for r, y in bank.push_audio({r: rows[r][1][rows[r][2]:rows[r][2] + push] for r in busy}).items():
                rows[r][3].append(y)
                rows[r][2] += push
            ended = [r for r in busy if rows[r][2] >= rows[r][1].shape[0]]
            for r, y in (bank.flush(ended) if ended else {}).items():
                done[rows[r][0]] = np.concatenate(rows[r][3] + [y], 0)
                rows[r] = None
        while next_out in done:
            yield done.pop(next_out)
            next_out += 1
        if not busy and exhausted:
            return


def decode_streams(model, utterances: Iterable[np.ndarray], chunk: int, streams: Optional[int] = None, finish=None) -> Iterator[np.ndarray]:
    """Decode many utterances side by side: rows [0, streams) of `model` each hold one utterance at its own position; every
    call advances every busy row by up to `chunk` frames; a row whose utterance ends takes the next one (its state is reset
    with that call), rows without work rest (lengths 0).  `utterances`: the generator's input matrices [T_i, D] (normalised
    and spliced, what GAN_RNN.forward takes), consumed lazily.  Yields G(x_i) [T_i, output_dim] in input order.  `finish`: applied to
    the output of every call that is a device tensor, before it is copied back (run_gan_rnn --device_features de-normalises there)."""
    batch, cap = _model_dims(model)
    streams = batch if streams is None else int(streams)
    chunk = int(chunk)
    if not 0 < streams <= batch:
        raise ValueError("streams=%d outside (0, batch_size=%d]" % (streams, batch))
    if chunk <= 0 or (cap is not None and chunk > cap):
        raise ValueError("chunk=%d outside (0, max_frames=%s]" % (chunk, cap))
    source = enumerate(utterances)
    rows = [None] * streams                  # per row: [index, x, position, outputs]
    done, next_out, exhausted = {}, 0, False
    while True:
        fresh = []
        for r in range(streams):
            while rows[r] is None and not exhausted:
                try:
                    i, x = next(source)
                except StopIteration:
                    exhausted = True
                    break
                if not _on_device(x):        # (a device tensor -- run_gan_rnn --device_features -- stays where it is)
                    x = np.asarray(x, np.float32)
                if x.ndim != 2:
                    raise ValueError("utterance %d must be [T, D], got %s" % (i, x.shape))
                if x.shape[0] == 0:
                    done[i] = np.zeros((0, int(getattr(model, "output_dim", 0) or 0)), np.float32)
                    continue
                rows[r] = [i, x, 0, []]
                fresh.append(r)
        busy = [r for r in range(streams) if rows[r] is not None]
        if busy:
            take = {r: min(chunk, rows[r][1].shape[0] - rows[r][2]) for r in busy}
            T = max(take.values())
            x0 = rows[busy[0]][1]
            xb = x0.new_zeros((batch, T, x0.shape[1])) if _on_device(x0) else np.zeros((batch, T, x0.shape[1]), np.float32)
            ln = np.zeros(batch, np.int32)
            for r in busy:
                _, x, pos, _ = rows[r]
                xb[r, :take[r]] = x[pos:pos + take[r]]
                ln[r] = take[r]
            y = model.forward_stream(xb, ln, reset=fresh or None)
            if finish is not None and _on_device(y):
                y = finish(y)
            y = y.detach().cpu().numpy() if _on_device(y) else np.asarray(y)
            for r in busy:
                rows[r][3].append(np.array(y[r, :take[r]]))
                rows[r][2] += take[r]
                if rows[r][2] == rows[r][1].shape[0]:
                    done[rows[r][0]] = np.concatenate(rows[r][3], 0)
                    rows[r] = None
        while next_out in done:
            yield done.pop(next_out)
            next_out += 1
        if not busy and exhausted:
            return
