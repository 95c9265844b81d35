"""Decoding with the generator's carried state (GAN_RNN.forward_stream): one live stream enhanced while it arrives
(StreamEnhancer), and many utterances decoded side by side in the rows of one handle (decode_streams).

Both are host logic around `model.forward_stream(inputs, lengths, reset)`: the model keeps, per batch row, the recurrent
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
    max_frames, the default)."""

    def __init__(self, model, cmvn=None, left_context=0, right_context=0, chunk=None):
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
        self._hist = None            # normalised frames [base, n) of the utterance (float64)
        self._base = 0               # utterance index of _hist[0]
        self._n = 0                  # frames received
        self._next = 0               # next frame to enhance
        self._fresh = True           # the carried state of row 0 is zeroed with the next forward call

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
        x = self._normalise(frames)
        if x.shape[0]:
            self._hist = x if self._hist is None else np.concatenate([self._hist, x], 0)
            self._n += x.shape[0]
        outs = self._enhance(self._n - self.right) if self._n - self.right > self._next else []
        return np.concatenate(outs, 0) if outs else self._empty()

    def flush(self):
        """the end of the utterance: the held-back frames, their right context filled with the last frame"""
        outs = self._enhance(self._n) if self._n > self._next else []
        out = np.concatenate(outs, 0) if outs else self._empty()
        self.reset()
        return out


def decode_streams(model, utterances: Iterable[np.ndarray], chunk: int, streams: Optional[int] = None) -> Iterator[np.ndarray]:
    """Decode many utterances side by side: rows [0, streams) of `model` each hold one utterance at its own position; every
    call advances every busy row by up to `chunk` frames; a row whose utterance ends takes the next one (its state is reset
    with that call), rows without work rest (lengths 0).  `utterances`: the generator's input matrices [T_i, D] (normalised
    and spliced, what GAN_RNN.forward takes), consumed lazily.  Yields G(x_i) [T_i, output_dim] in input order."""
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
