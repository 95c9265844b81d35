"""Feature pipeline between the ark reader and GAN_RNN.d_step/g_step: global CMVN
(io_funcs/make_tfrecords.py:84-87), Kaldi-style splicing (io_funcs/tfrecords_io.py:177-203) and
length-bucketed, zero-padded batches (io_funcs/tfrecords_dataset.py:139-175)."""
from __future__ import annotations

import random
from typing import Iterator, List, Optional

import numpy as np

from .kaldi_ark import ArkReader, coded_bytes


def apply_cmvn(inputs, labels, cmvn):
    """make_tfrecords.py:84-87: float64 arithmetic, (x - mean) / stddev."""
    inputs = np.array(inputs, np.float64)                 # private float64 copy, then in place (no temporaries)
    inputs -= cmvn["mean_inputs"]; inputs /= cmvn["stddev_inputs"]
    if labels is not None:
        labels = np.array(labels, np.float64)
        labels -= cmvn["mean_labels"]; labels /= cmvn["stddev_labels"]
    return inputs, labels


def splice_feats(feats, left, right):
    """tfrecords_io.py:177-203: [row, col] -> [row, col*(left+1+right)].  The i-th left context is
    feats shifted down by i with the first row repeated (tf.pad SYMMETRIC one row at a time), the
    i-th right context is feats shifted up by i with the last row repeated; order: left far..near,
    centre, right near..far."""
    feats = np.asarray(feats)
    row = feats.shape[0]
    idx = np.arange(row)
    parts = [feats[np.maximum(idx - i, 0)] for i in range(left, 0, -1)]
    parts.append(feats)
    parts += [feats[np.minimum(idx + i, row - 1)] for i in range(1, right + 1)]
    return np.concatenate(parts, 1)


class PackedBatch(object):
    """A batch as the device-side front end takes it (HipEngine.featurize, csrc/feat.hip): the utterances' RAW frames one after the
    other and where each begins -- no CMVN, no splice, no padding.  `data` float32 [rows, D]; `offsets` int32 [B + 1] (utterance b
    is data[offsets[b]:offsets[b + 1]]); `shape` = the (B, T, D * (left + 1 + right)) the expanded batch has, so that what reads
    `.shape[0]` of a fed batch (train_one_iteration's row check, GAN_RNN._shard) works on either kind.  `left`, `right`, `mean`,
    `stddev` say how the reader that made the batch would have expanded it (mean / stddev: float64 [D], or None for no CMVN)."""

    def __init__(self, data, offsets, shape, left=0, right=0, mean=None, stddev=None):
        self.data, self.offsets, self.shape = data, offsets, tuple(int(v) for v in shape)
        self.left, self.right, self.mean, self.stddev = int(left), int(right), mean, stddev
        if self.offsets.shape[0] != self.shape[0] + 1:
            raise ValueError("offsets must hold B + 1 = %d entries, got %d" % (self.shape[0] + 1, self.offsets.shape[0]))

    def __len__(self):
        return self.shape[0]

    def lengths(self):
        """frames of every utterance after truncation at T (int32 [B]): what the kernel writes as `lengths`"""
        return np.minimum(np.diff(self.offsets), self.shape[1]).astype(np.int32)

    def rows(self, lo, hi):
        """utterances [lo, hi) as a batch of their own -- this rank's shard of a fed batch (GAN_RNN._shard): only their frames, offsets
        rebased to 0, the same T"""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= self.shape[0]:
            raise ValueError("rows [%d, %d) outside the batch of %d" % (lo, hi, self.shape[0]))
        a, b = int(self.offsets[lo]), int(self.offsets[hi])
        return PackedBatch(self.data[a:b], (self.offsets[lo:hi + 1] - self.offsets[lo]).astype(np.int32), (hi - lo,) + self.shape[1:],
                           self.left, self.right, self.mean, self.stddev)


def pack_utterances(mats, left=0, right=0, mean=None, stddev=None, T=None, names=None):
    """float32 [n_i, D] matrices -> PackedBatch padded to T (default: the longest).  A matrix that is not float32 raises ValueError
    naming it: the device entry takes fp32 raw frames only."""
    for i, m in enumerate(mats):
        if not isinstance(m, np.ndarray) or m.dtype != np.float32 or m.ndim != 2:
            raise ValueError("utterance %s: the device-side front end takes float32 [frames, dim] matrices only, got %s %s" % (
                names[i] if names is not None else i, getattr(m, "dtype", type(m).__name__), getattr(m, "shape", "")))
    n = [m.shape[0] for m in mats]
    offsets = np.zeros(len(mats) + 1, np.int64)
    np.cumsum(n, out=offsets[1:])
    if offsets[-1] >= 2 ** 31:
        raise ValueError("a packed batch of %d frames does not fit the int32 offset table" % offsets[-1])
    D = mats[0].shape[1]
    data = np.concatenate(mats, 0)                           # (a private, writable copy also of a single read-only matrix)
    return PackedBatch(data, offsets.astype(np.int32), (len(mats), max(n) if T is None else int(T), D * (left + 1 + right)), left, right,
                       mean, stddev)


ALIGN = 16                                 # every utterance's segment starts at a multiple of this in a CodedBatch's blob


class CodedBatch(object):
    """PackedBatch's sibling for archives that are not float32: the utterances in their ARCHIVE encoding, to be decoded, normalised,
    spliced and padded on the device (HipEngine.featurize, csrc/feat.hip k_feat_decode).  `blob` uint8: the matrices' bytes as the files
    hold them, every utterance's segment starting at a multiple of 16; `seg` int64 [B, 2] = (byte offset of the segment, kind:
    kaldi_ark.KIND_*); `scale` float32 [B, 2] = (min, range) of a compressed matrix's header; `offsets` int32 [B + 1]: utterance b has
    offsets[b + 1] - offsets[b] frames.  `shape`, `left`, `right`, `mean`, `stddev` as in PackedBatch; `dim` = the matrices' columns.
    The constructor checks what the device cannot: known kinds, monotone offsets, every segment aligned and inside the blob with the
    size its kind, frames and dim imply."""

    def __init__(self, blob, seg, scale, offsets, shape, left=0, right=0, mean=None, stddev=None):
        self.blob, self.seg, self.scale, self.offsets = blob, seg, scale, offsets
        self.shape = tuple(int(v) for v in shape)
        self.left, self.right, self.mean, self.stddev = int(left), int(right), mean, stddev
        B, C = self.shape[0], self.left + 1 + self.right
        if self.shape[2] < C or self.shape[2] % C:
            raise ValueError("shape[2] = %d is no multiple of left + 1 + right = %d" % (self.shape[2], C))
        self.dim = self.shape[2] // C
        if blob.dtype != np.uint8 or blob.ndim != 1:
            raise ValueError("blob must be a flat uint8 array, got %s %s" % (blob.dtype, blob.shape))
        if offsets.shape != (B + 1,) or offsets.dtype != np.int32:
            raise ValueError("offsets must hold B + 1 = %d int32 entries, got %s %s" % (B + 1, offsets.dtype, offsets.shape))
        if seg.shape != (B, 2) or seg.dtype != np.int64 or scale.shape != (B, 2) or scale.dtype != np.float32:
            raise ValueError("seg must be int64 [%d, 2] and scale float32 [%d, 2], got %s %s and %s %s" % (
                B, B, seg.dtype, seg.shape, scale.dtype, scale.shape))
        n = np.diff(offsets.astype(np.int64))
        if (B and n.min() < 0) or offsets[0] < 0:
            raise ValueError("offsets must start at 0 or above and never decrease")
        for b in range(B):
            size = coded_bytes(int(seg[b, 1]), int(n[b]), self.dim)
            if size is None:
                raise ValueError("utterance %d: unknown kind %d" % (b, seg[b, 1]))
            if seg[b, 0] < 0 or seg[b, 0] % ALIGN or seg[b, 0] + size > blob.shape[0]:
                raise ValueError("utterance %d: a segment of %d bytes at byte %d does not lie in the blob of %d (segments start at multiples "
                                 "of %d)" % (b, size, seg[b, 0], blob.shape[0], ALIGN))

    def __len__(self):
        return self.shape[0]

    def lengths(self):
        """frames of every utterance after truncation at T (int32 [B]): what the splice kernel writes as `lengths`"""
        return np.minimum(np.diff(self.offsets), self.shape[1]).astype(np.int32)

    def nbytes(self):
        """what travels to the device: the blob and the three tables"""
        return int(self.blob.nbytes + self.seg.nbytes + self.scale.nbytes + self.offsets.nbytes)

    def rows(self, lo, hi):
        """utterances [lo, hi) as a batch of their own -- this rank's shard of a fed batch (GAN_RNN._shard): only their bytes, segment
        offsets and frame offsets rebased to 0, the same T"""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= self.shape[0]:
            raise ValueError("rows [%d, %d) outside the batch of %d" % (lo, hi, self.shape[0]))
        n = np.diff(self.offsets[lo:hi + 1].astype(np.int64))
        sizes = [coded_bytes(int(self.seg[b, 1]), int(n[b - lo]), self.dim) for b in range(lo, hi)]
        parts = [self.blob[int(self.seg[b, 0]):int(self.seg[b, 0]) + s] for b, s in zip(range(lo, hi), sizes)]
        blob, starts = _join_aligned(parts)
        seg = np.stack([starts, self.seg[lo:hi, 1]], 1).astype(np.int64).reshape(hi - lo, 2)
        return CodedBatch(blob, seg, np.ascontiguousarray(self.scale[lo:hi]), (self.offsets[lo:hi + 1] - self.offsets[lo]).astype(np.int32),
                          (hi - lo,) + self.shape[1:], self.left, self.right, self.mean, self.stddev)


def _join_aligned(parts):
    """byte strings / uint8 arrays -> (one uint8 array in which part i starts at starts[i], a multiple of ALIGN; the gaps are zero)"""
    starts = np.zeros(len(parts), np.int64)
    at = 0
    for i, p in enumerate(parts):
        starts[i] = at
        at += (len(p) + ALIGN - 1) // ALIGN * ALIGN
    blob = np.zeros(max(at, ALIGN), np.uint8)
    for s, p in zip(starts.tolist(), parts):
        blob[s:s + len(p)] = np.frombuffer(p, np.uint8) if isinstance(p, (bytes, bytearray)) else p
    return blob, starts


def pack_coded(mats, left=0, right=0, mean=None, stddev=None, T=None, names=None):
    """kaldi_ark.CodedMatrix items (ArkReader.read_coded) -> CodedBatch padded to T (default: the longest): the bytes are copied once,
    nothing is decoded."""
    D = mats[0].cols
    for i, m in enumerate(mats):
        if m.cols != D:
            raise ValueError("utterance %s: %d columns, the batch has %d" % (names[i] if names is not None else i, m.cols, D))
    n = [m.rows for m in mats]
    offsets = np.zeros(len(mats) + 1, np.int64)
    np.cumsum(n, out=offsets[1:])
    if offsets[-1] >= 2 ** 31:
        raise ValueError("a coded batch of %d frames does not fit the int32 offset table" % offsets[-1])
    blob, starts = _join_aligned([m.data for m in mats])
    seg = np.stack([starts, np.array([m.kind for m in mats], np.int64)], 1)
    scale = np.array([[m.min, m.range] for m in mats], np.float32).reshape(len(mats), 2)
    return CodedBatch(blob, seg, scale, offsets.astype(np.int32), (len(mats), max(n) if T is None else int(T), D * (left + 1 + right)), left,
                      right, mean, stddev)


def plan_batches(nframes, batch_size, num_buckets, shuffle, rng) -> Iterator[List[int]]:
    """The batching rule of get_padded_batch (tfrecords_dataset.py:139-175) on frame counts alone: the utterance indices of every batch,
    in order -- windows of batch_size per length bucket (start 200 frames, width 50, ids clipped at num_buckets), partial windows at
    the end.  Shared by PaddedBatchReader and io.wave_reader.WaveBatchReader."""
    order = list(range(len(nframes)))
    if shuffle:
        rng.shuffle(order)
    windows = {}
    for i in order:
        if num_buckets > 1:
            key = min(num_buckets, (nframes[i] - 200) // 50)      # :157-165
        else:
            key = 0
        w = windows.setdefault(key, [])
        w.append(i)
        if len(w) == batch_size:
            yield w
            windows[key] = []
    for key in sorted(windows):
        if windows[key]:
            yield windows[key]


def pad_items(items):
    """(utt, x [n, D], y [n, Dl]) triples -> [ids, X [B, T, D], Y [B, T, Dl], lengths]: zero padding to the longest utterance"""
    T = max(x.shape[0] for _, x, _ in items)
    ids = [u for u, _, _ in items]
    X = np.empty((len(items), T, items[0][1].shape[1]), np.float32)       # every element is written exactly once below
    Y = np.empty((len(items), T, items[0][2].shape[1]), np.float32)
    L = np.zeros(len(items), np.int32)
    for b, (_, x, y) in enumerate(items):
        n = x.shape[0]
        X[b, :n] = x; X[b, n:] = 0.0
        Y[b, :n] = y; Y[b, n:] = 0.0
        L[b] = n
    return [ids, X, Y, L]


class PaddedBatchReader(object):
    """get_padded_batch (tfrecords_dataset.py:53-180) without TFRecords: reads (inputs, labels)
    utterance pairs from two scp files, applies CMVN and splicing, groups utterances into windows of
    `batch_size` by length bucket (start 200 frames, width 50, ids clipped at num_buckets, :157-171),
    pads each batch with zeros to its longest utterance and yields
    [utt_ids, inputs [B,T,D*(L+1+R)] f32, labels [B,T,Dout] f32, lengths [B] i32] -- the items
    train_one_iteration pops from its queue (train_gan_rnn_placeholder.py:67).  Partial windows are
    emitted at the end of the data, like tf.contrib.data.group_by_window; the training loop skips them.

    device_features=True: CMVN, splicing and padding are left to the device (HipEngine.featurize).  materialize only reads and
    concatenates the raw utterances and yields [utt_ids, PackedBatch(inputs), PackedBatch(labels), lengths]; plan() is the same, so
    the same seed draws the same batches in the same order, and the expanded items are bit for bit the default reader's.

    device_decode=True (implies device_features): the archives' bytes travel UNDECODED -- float, double and Kaldi-compressed matrices
    alike -- and the device decodes them too (csrc/feat.hip k_feat_decode).  materialize reads each matrix's bytes (ArkReader.read_coded,
    no NumPy decode) and yields [utt_ids, CodedBatch(inputs), CodedBatch(labels), lengths]; plan() is the same again."""

    def __init__(self, inputs_scp, labels_scp, batch_size, left_context=0, right_context=0, cmvn=None,
                 num_buckets=20, shuffle=True, seed=None, device_features=False, device_decode=False):
        self.device_decode = bool(device_decode)
        self.device_features = bool(device_features) or self.device_decode
        self._stats = None
        if self.device_features and cmvn is not None:
            self._stats = tuple(np.ascontiguousarray(cmvn[k], np.float64).reshape(-1)
                                for k in ("mean_inputs", "stddev_inputs", "mean_labels", "stddev_labels"))
        self.inputs, self.labels = ArkReader(), ArkReader()
        self.inputs(inputs_scp)
        self.labels(labels_scp)
        assert self.inputs.utt_ids == self.labels.utt_ids, "inputs_utt_id == labels_utt_id (make_tfrecords.py:35)"
        self.batch_size, self.left, self.right = batch_size, left_context, right_context
        self.cmvn, self.num_buckets, self.shuffle = cmvn, num_buckets, shuffle
        self.rng = random.Random(seed)
        self._nframes = None

    def __len__(self):
        return len(self.inputs.utt_ids)

    def _utt(self, i):
        x = self.inputs.read_utt_data_from_index(i).astype(np.float64)
        y = self.labels.read_utt_data_from_index(i).astype(np.float64)
        if self.cmvn is not None:
            x, y = apply_cmvn(x, y, self.cmvn)
        return self.inputs.utt_ids[i], splice_feats(x, self.left, self.right).astype(np.float32), y.astype(np.float32)

    def _pad(self, items):
        return pad_items(items)

    def plan(self) -> Iterator[List[int]]:
        """The utterance indices of every batch, in the order __iter__ yields them -- from the matrix headers alone, so the
        expensive part (materialize) can run on several threads (io.prefetch)."""
        if self._nframes is None:
            self._nframes = [self.inputs.utt_shape_from_index(i)[0] for i in range(len(self))]
        return plan_batches(self._nframes, self.batch_size, self.num_buckets, self.shuffle, self.rng)

    def _packed(self, indices):
        ids = [self.inputs.utt_ids[i] for i in indices]
        xs = [self.inputs.read_utt_data_from_index(i) for i in indices]
        ys = [self.labels.read_utt_data_from_index(i) for i in indices]
        for u, x, y in zip(ids, xs, ys):
            if x.shape[0] != y.shape[0]:
                raise ValueError("utterance %s: %d input frames, %d label frames" % (u, x.shape[0], y.shape[0]))
        mi, si, ml, sl = self._stats if self._stats is not None else (None,) * 4
        X = pack_utterances(xs, self.left, self.right, mi, si, names=ids)
        Y = pack_utterances(ys, 0, 0, ml, sl, names=ids)
        return [ids, X, Y, X.lengths()]

    def _coded(self, indices):
        ids = [self.inputs.utt_ids[i] for i in indices]
        xs = [self.inputs.read_coded_from_index(i) for i in indices]
        ys = [self.labels.read_coded_from_index(i) for i in indices]
        for u, x, y in zip(ids, xs, ys):
            if x.rows != y.rows:
                raise ValueError("utterance %s: %d input frames, %d label frames" % (u, x.rows, y.rows))
        mi, si, ml, sl = self._stats if self._stats is not None else (None,) * 4
        X = pack_coded(xs, self.left, self.right, mi, si, names=ids)
        Y = pack_coded(ys, 0, 0, ml, sl, names=ids)
        return [ids, X, Y, X.lengths()]

    def materialize(self, indices: List[int]) -> List:
        if self.device_decode:
            return self._coded(indices)
        if self.device_features:
            return self._packed(indices)
        return self._pad([self._utt(i) for i in indices])

    def __iter__(self) -> Iterator[List]:
        for indices in self.plan():
            yield self.materialize(indices)


class FrameBatchReader(object):
    """get_batch of the frame-level recipes (io_funcs/tfrecords_io.py:206-255) without TFRecords: every utterance is normalised,
    spliced and its frames `enqueue_many`-ed into a tf.RandomShuffleQueue(capacity = 1000 + (num_threads + 1) * batch_size,
    min_after_dequeue = 1000); `dequeue_many(batch_size)` draws that many frames uniformly at random from the queue.  Yields
    [inputs [N, D*(L+1+R)] f32, labels [N, Dout] f32].  Utterances are visited in shuffled order once per pass
    (string_input_producer(shuffle=True, num_epochs)); the frames left over at the end of the data that do not fill a batch are
    dropped, as dequeue_many does when the queue closes.

    device_features=True: the queue is bookkeeping only.  The utterances live in a pool of rows on the device (HipEngine.featurize_frames
    normalises each ONCE into the slot the reader's RowAllocator gave it) and every batch is an io.frame_pool.FrameDraw: the raw utterances
    enqueued since the previous batch and a table of the drawn frames (pool row, the utterance's row range) from which one kernel gathers the
    spliced batch.  Enqueuing follows the rules of __iter__ and drawing makes the same calls on self.rng, so the same seed draws the same
    frames in the same order as the default reader, and the expanded batches are its batches bit for bit.  `initial_pool_rows`: the
    pool's first capacity (default: the queue's capacity; it doubles when an utterance does not fit).

    device_decode=True (implies device_features): an admission carries the matrices' bytes as the archive holds them
    (kaldi_ark.CodedMatrix: float, double or Kaldi-compressed) and the device decodes and normalises them into the pool rows in one
    launch (csrc/feat.hip k_feat_decode); the queue's bookkeeping and the draws are the same."""

    def __init__(self, inputs_scp, labels_scp, batch_size, left_context=0, right_context=0, cmvn=None, num_threads=4,
                 shuffle=True, seed=None, device_features=False, initial_pool_rows=None, device_decode=False):
        self.device_decode = bool(device_decode)
        self.device_features = bool(device_features) or self.device_decode
        self.inputs, self.labels = ArkReader(), ArkReader()
        self.inputs(inputs_scp)
        self.labels(labels_scp)
        assert self.inputs.utt_ids == self.labels.utt_ids, "inputs_utt_id == labels_utt_id (make_tfrecords.py:35)"
        self.batch_size, self.left, self.right, self.cmvn, self.shuffle = batch_size, left_context, right_context, cmvn, shuffle
        self.capacity = 1000 + (num_threads + 1) * batch_size
        self.min_after_dequeue = 1000 if shuffle else 0
        self.rng = np.random.default_rng(seed)
        if self.device_features:
            from . import frame_pool
            self.reader_id, self._serial = frame_pool.new_reader_id(), 0
            self.allocator = frame_pool.RowAllocator(self.capacity if initial_pool_rows is None else initial_pool_rows)
            self._stats = None
            if cmvn is not None:
                self._stats = tuple(np.ascontiguousarray(cmvn[k], np.float64).reshape(-1)
                                    for k in ("mean_inputs", "stddev_inputs", "mean_labels", "stddev_labels"))

    def num_frames(self):
        return sum(self.inputs.utt_shape_from_index(i)[0] for i in range(len(self.inputs.utt_ids)))

    def num_batches(self):
        """get_num_batch (train_gan_dnn.py:346-370) counts dequeued batches of one pass: floor(frames / batch_size)."""
        return self.num_frames() // self.batch_size

    def _utt(self, i):
        x = self.inputs.read_utt_data_from_index(i).astype(np.float64)
        y = self.labels.read_utt_data_from_index(i).astype(np.float64)
        if self.cmvn is not None:
            x, y = apply_cmvn(x, y, self.cmvn)
        return splice_feats(x, self.left, self.right).astype(np.float32), y.astype(np.float32)

    def _raw(self, i):
        if self.device_decode:
            x, y = self.inputs.read_coded_from_index(i), self.labels.read_coded_from_index(i)
            if x.rows != y.rows:
                raise ValueError("utterance %s: %d input frames, %d label frames" % (self.inputs.utt_ids[i], x.rows, y.rows))
            return x, y
        x, y = self.inputs.read_utt_data_from_index(i), self.labels.read_utt_data_from_index(i)
        for m, what in ((x, "inputs"), (y, "labels")):
            if not isinstance(m, np.ndarray) or m.dtype != np.float32 or m.ndim != 2:
                raise ValueError("utterance %s: the device-side front end takes float32 [frames, dim] matrices only, got %s %s %s" % (
                    self.inputs.utt_ids[i], what, getattr(m, "dtype", type(m).__name__), getattr(m, "shape", "")))
        if x.shape[0] != y.shape[0]:
            raise ValueError("utterance %s: %d input frames, %d label frames" % (self.inputs.utt_ids[i], x.shape[0], y.shape[0]))
        return np.array(x, order="C"), np.array(y, order="C")          # (private, writable copies: the ark reader's views are read-only)

    def _iter_draws(self):
        """__iter__ with the queue as a table: one row (pool row, lo, hi, slot) per held frame, in the order the default reader's
        concatenated queue holds them.  A new pass drops what the previous one left in the queue, slots included."""
        from .frame_pool import FrameDraw
        order = np.arange(len(self.inputs.utt_ids))
        if self.shuffle:
            self.rng.shuffle(order)
        alloc = self.allocator
        alloc.free_all()
        table, held = np.zeros((0, 4), np.int32), 0
        left_in = {}                               # slot -> frames of it still in the queue
        uploads, dims = [], None
        todo = list(order)
        N = self.batch_size

        def draw():
            nonlocal table, held, uploads
            pick = self.rng.choice(held, N, replace=False) if self.shuffle else np.arange(N)
            keep = np.ones(held, bool); keep[pick] = False
            drawn = table[pick]
            table, held = table[keep], held - N
            slots, counts = np.unique(drawn[:, 3], return_counts=True)
            for s, c in zip(slots.tolist(), counts.tolist()):
                left_in[s] -= c
                if left_in[s] == 0:                # the utterance's last held frame was drawn: its rows may be handed out again.  The
                    del left_in[s]                 # consumer writes them no sooner than a LATER item's uploads, behind this item's gather
                    alloc.free(s)
            item = FrameDraw(self._serial, self.reader_id, uploads, alloc.pool_rows, np.ascontiguousarray(drawn[:, :3]), self.left, self.right,
                             self._stats, dims[0], dims[1])
            self._serial += 1
            uploads = []
            return item
        while todo or held >= N:
            while todo and (held < N or held + self.inputs.utt_shape_from_index(int(todo[0]))[0] <= self.capacity):
                x, y = self._raw(int(todo.pop(0)))
                n = x.shape[0]
                dims = (x.shape[1], y.shape[1])
                if n == 0:
                    continue
                first = alloc.alloc(n)
                if alloc.pool_rows >= 2 ** 31:
                    raise ValueError("a frame pool of %d rows does not fit the int32 pick table" % alloc.pool_rows)
                block = np.empty((n, 4), np.int32)
                block[:, 0] = np.arange(first, first + n); block[:, 1] = first; block[:, 2] = first + n; block[:, 3] = first
                table = np.concatenate([table, block]); held += n
                left_in[first] = n
                uploads.append((first, x, y))
            if held >= N and (held - N >= self.min_after_dequeue or not todo):
                yield draw()
            elif not todo:
                break
            elif held >= N:
                yield draw()

    def __iter__(self):
        if self.device_features:
            yield from self._iter_draws()
            return
        order = np.arange(len(self.inputs.utt_ids))
        if self.shuffle:
            self.rng.shuffle(order)
        qx, qy, held = [], [], 0                   # the queue as a list of per-utterance blocks + how many frames it holds
        todo = list(order)
        N = self.batch_size

        def draw():
            nonlocal qx, qy, held
            X, Y = np.concatenate(qx), np.concatenate(qy)
            pick = self.rng.choice(held, N, replace=False) if self.shuffle else np.arange(N)
            keep = np.ones(held, bool); keep[pick] = False
            bx, by = X[pick], Y[pick]
            qx, qy, held = [X[keep]], [Y[keep]], held - N
            return [bx, by]
        while todo or held >= N:
            # the enqueuing threads keep the queue as full as its capacity allows: an utterance is enqueued when it fits, and
            # whenever no batch can be drawn (held < N) -- tf's enqueue_many admits an over-long utterance piecewise as room
            # frees up, so it never blocks the dequeue side for good (an utterance longer than the capacity must not hang)
            while todo and (held < N or held + self.inputs.utt_shape_from_index(int(todo[0]))[0] <= self.capacity):
                x, y = self._utt(int(todo.pop(0)))
                qx.append(x); qy.append(y); held += x.shape[0]
            if held >= N and (held - N >= self.min_after_dequeue or not todo):
                yield draw()
            elif not todo:
                break
            elif held >= N:                        # an utterance longer than the room left: dequeue first, as a blocked enqueue would wait
                yield draw()
