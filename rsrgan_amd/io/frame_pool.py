"""Host bookkeeping of the frame-level recipes' device-side front end (FrameBatchReader(device_features=True), HipEngine.featurize_frames,
csrc/feat.hip k_feat_frames).  No device in here: the shuffle queue of io_funcs/tfrecords_io.py:206-255 kept as a table of WHICH frames it
holds, the utterances themselves resident in a pool of rows on the device.

  RowAllocator   where an utterance's frames live in the pool: first fit over a free list with coalescing, slots in units of 4 rows (a
                 slot's byte offset is a multiple of 16 at any D), growth by doubling, no compaction -- deterministic, so that the same
                 seed gives the same pool rows.
  FrameDraw      one batch: the utterances enqueued since the previous batch (raw frames and the pool row each goes to), the capacity
                 the pool must have by now, and the table of drawn frames.
  PoolLedger     the consumer's side of the contract: items of one reader are consumed once, in the order they were made."""
from __future__ import annotations

import itertools

import numpy as np

UNIT = 4                                  # rows per allocation unit: 4 rows x D floats x 4 bytes is a multiple of 16 at any D
_ids = itertools.count(1)


def new_reader_id():
    """what tells one reader's pool from another's on the engine (the training and the cross-validation reader are two pools)"""
    return next(_ids)


def _up(n):
    return (int(n) + UNIT - 1) // UNIT * UNIT


class RowAllocator(object):
    """Rows [0, pool_rows) as slots.  alloc(n) -> first row of a slot of _up(n) rows: the first free block that holds it; when none does,
    pool_rows doubles (the new rows join the free list, coalesced with a free block that ended at the old capacity) until one does.  Rows
    handed out keep their numbers for as long as they are held.  free(first) returns a slot; neighbours coalesce."""

    def __init__(self, pool_rows):
        self.pool_rows = max(_up(pool_rows), UNIT)
        self.blocks = [[0, self.pool_rows]]             # free blocks [first, rows], sorted by first, never adjacent
        self.live = {}                                  # first row -> rows of every slot handed out
        self.growths = 0

    def alloc(self, n):
        need = max(_up(n), UNIT)
        while True:
            for k, (first, rows) in enumerate(self.blocks):
                if rows >= need:
                    if rows == need:
                        del self.blocks[k]
                    else:
                        self.blocks[k] = [first + need, rows - need]
                    self.live[first] = need
                    return first
            old = self.pool_rows
            self.pool_rows = old * 2
            self.growths += 1
            if self.blocks and self.blocks[-1][0] + self.blocks[-1][1] == old:
                self.blocks[-1][1] += old
            else:
                self.blocks.append([old, old])

    def free(self, first):
        rows = self.live.pop(first)
        lo, hi = 0, len(self.blocks)
        while lo < hi:                                  # where the block goes in the sorted list
            mid = (lo + hi) // 2
            if self.blocks[mid][0] < first:
                lo = mid + 1
            else:
                hi = mid
        self.blocks.insert(lo, [first, rows])
        if lo + 1 < len(self.blocks) and first + rows == self.blocks[lo + 1][0]:
            self.blocks[lo][1] += self.blocks[lo + 1][1]
            del self.blocks[lo + 1]
        if lo > 0 and self.blocks[lo - 1][0] + self.blocks[lo - 1][1] == first:
            self.blocks[lo - 1][1] += self.blocks[lo][1]
            del self.blocks[lo]

    def free_all(self):
        self.live.clear()
        self.blocks = [[0, self.pool_rows]]


class FrameDraw(object):
    """One batch of the frame-level reader as the device-side front end takes it.  `serial`: 0, 1, 2 ... per reader; `reader_id`: whose pool;
    `uploads`: [(first_row, raw_inputs float32 [n, D], raw_labels float32 [n, Dl])] of the utterances enqueued since the previous item, to be
    normalised once into rows first_row .. first_row + n - 1; `pool_rows`: the capacity the pool must have by now (monotone); `picks` int32
    [N, 3] = (row, lo, hi): the drawn frames, each with its utterance's row range; `left`, `right`; `stats`: (mean_inputs, stddev_inputs,
    mean_labels, stddev_labels) in float64, or None for no CMVN.  Under FrameBatchReader(device_decode=True) an upload's two matrices are
    kaldi_ark.CodedMatrix items instead (the archive's bytes, decoded on the device).  Stateful: consumed once, in order (PoolLedger)."""

    def __init__(self, serial, reader_id, uploads, pool_rows, picks, left, right, stats, input_dim, label_dim):
        self.serial, self.reader_id, self.uploads, self.pool_rows, self.picks = int(serial), reader_id, uploads, int(pool_rows), picks
        self.left, self.right, self.stats = int(left), int(right), stats
        self.input_dim, self.label_dim = int(input_dim), int(label_dim)
        self.shape = (picks.shape[0], self.input_dim * (self.left + 1 + self.right))

    def __len__(self):
        return self.shape[0]


def is_frame_draw(a):
    """a FrameDraw (by its fields, as train.is_packed tells a PackedBatch)"""
    return hasattr(a, "picks") and hasattr(a, "uploads") and hasattr(a, "serial")


def is_coded(m):
    """a kaldi_ark.CodedMatrix (by its fields): an admission whose bytes the device decodes"""
    return hasattr(m, "kind") and hasattr(m, "data") and hasattr(m, "rows")


class PoolLedger(object):
    """What a consumer of FrameDraw items (HipEngine.featurize_frames; the NumPy stand-in of the tests) checks BEFORE it touches its pool:
    the item is the next one of its reader, its pool never shrinks, and every upload and pick lies inside it."""

    def __init__(self, reader_id):
        self.reader_id, self.next_serial, self.pool_rows = reader_id, 0, 0

    def admit(self, item):
        if item.reader_id != self.reader_id:
            raise ValueError("frame draw of reader %r handed to the pool of reader %r" % (item.reader_id, self.reader_id))
        if item.serial != self.next_serial:
            raise ValueError("frame draw %d of reader %r is out of order: the pool expects draw %d (items are consumed once, in the order "
                             "the reader made them)" % (item.serial, self.reader_id, self.next_serial))
        if item.pool_rows < self.pool_rows or item.pool_rows < 1 or item.pool_rows % UNIT:
            raise ValueError("frame draw %d: pool_rows = %d (the pool holds %d rows and never shrinks; units of %d)" % (
                item.serial, item.pool_rows, self.pool_rows, UNIT))
        for first, x, y in item.uploads:
            if is_coded(x) or is_coded(y):
                # a coded admission (FrameBatchReader(device_decode=True)): kaldi_ark.CodedMatrix pairs, whose constructor has checked the
                # byte count against kind, rows and cols
                if not (is_coded(x) and is_coded(y)) or x.rows != y.rows or x.cols != item.input_dim or y.cols != item.label_dim:
                    raise ValueError("frame draw %d: an upload is not a pair of coded [n, %d] / [n, %d] matrices" % (
                        item.serial, item.input_dim, item.label_dim))
            elif (x.dtype != np.float32 or y.dtype != np.float32 or x.ndim != 2 or y.ndim != 2 or x.shape[0] != y.shape[0]
                    or x.shape[1] != item.input_dim or y.shape[1] != item.label_dim):
                raise ValueError("frame draw %d: an upload is not a pair of float32 [n, %d] / [n, %d] matrices" % (
                    item.serial, item.input_dim, item.label_dim))
            if first < 0 or first % UNIT or first + x.shape[0] > item.pool_rows:
                raise ValueError("frame draw %d: an upload of %d rows at row %d does not lie in the pool of %d" % (
                    item.serial, x.shape[0], first, item.pool_rows))
        p = item.picks
        if p.dtype != np.int32 or p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
            raise ValueError("frame draw %d: picks must be int32 [N, 3]" % item.serial)
        if p.min() < 0 or p.max() > item.pool_rows or np.any(p[:, 0] < p[:, 1]) or np.any(p[:, 0] >= p[:, 2]):
            raise ValueError("frame draw %d: a pick does not lie inside its utterance, or its utterance not inside the pool" % item.serial)
        self.next_serial += 1
        self.pool_rows = item.pool_rows
