"""Host stand-ins for the frame-level device-side front end (csrc/feat.hip k_feat_frames, HipEngine.featurize_frames), built only from
io.features.apply_cmvn / splice_feats and indexing.

  HostPool        replays the FrameDraw items of FrameBatchReader(device_features=True) the way the engine does: a pool of normalised
                  float32 rows per reader, grown by copying, every upload normalised once (float64, one rounding) into its slot, the
                  batch gathered by index.  It also records what the allocator invariants are checked on.
  gather          the formula of include/rsrgan.h for rsrgan_feat_frames on a raw pool, clamps included.
  expand_picks    the same for picks that lie inside their utterances, through splice_feats on the utterance itself."""
import numpy as np

from rsrgan_amd.io import ArkWriter, PoolLedger, apply_cmvn, splice_feats


def gather(pool, picks, left, right, stats=None, pool_rows=None):
    """out [N, D * (left + 1 + right)] float32 by the entry's formula: context clamped into [lo, hi), then into [0, pool_rows); a pick with
    hi <= lo gives +0.0; stats = (mean, stddev) float64 or None"""
    pool, picks = np.asarray(pool), np.asarray(picks).astype(np.int64)
    rows = pool.shape[0] if pool_rows is None else int(pool_rows)
    src = pool
    if stats is not None:
        src = apply_cmvn(pool, None, {"mean_inputs": stats[0], "stddev_inputs": stats[1]})[0].astype(np.float32)
    c = np.arange(-left, right + 1)[None, :]
    idx = np.minimum(np.maximum(picks[:, :1] + c, picks[:, 1:2]), picks[:, 2:3] - 1)
    idx = np.minimum(np.maximum(idx, 0), rows - 1)
    out = src[idx].reshape(picks.shape[0], -1)
    out[picks[:, 2] <= picks[:, 1]] = 0.0
    return np.ascontiguousarray(out, np.float32)


def expand_picks(pool, picks, left, right, stats=None):
    """the host path on the utterance a pick names: normalise in float64, splice_feats, one cast, the drawn row"""
    out = np.zeros((len(picks), pool.shape[1] * (left + 1 + right)), np.float32)
    for i, (row, lo, hi) in enumerate(np.asarray(picks).tolist()):
        if hi <= lo:
            continue
        x = pool[lo:hi].astype(np.float64)
        if stats is not None:
            x = apply_cmvn(x, None, {"mean_inputs": stats[0], "stddev_inputs": stats[1]})[0]
        out[i] = splice_feats(x, left, right).astype(np.float32)[row - lo]
    return out


class HostPool(object):
    def __init__(self, reader_id):
        self.ledger = PoolLedger(reader_id)
        self.x = self.y = None
        self.live = {}                   # first row -> [rows, frames not yet drawn] of every utterance in the pool
        self.history = []                # per item: (pool_rows, [(first, rows) uploaded], [first freed after this item's draw])
        self.reuses = self.growths = 0
        self._freed_rows = np.zeros(0, bool)

    def new_pass(self):
        """the reader starts a new pass over the data: what the previous pass left in the queue is dropped, its rows are free"""
        for lo, (rows, _) in self.live.items():
            self._freed_rows[lo:lo + rows] = True
        self.live.clear()

    def feed(self, item):
        """one item -> (inputs [N, Dout] float32, labels [N, Dl] float32); asserts the allocator invariants on the way"""
        self.ledger.admit(item)
        if self.x is None or item.pool_rows > self.x.shape[0]:
            self.growths += self.x is not None
            nx, ny = np.full((item.pool_rows, item.input_dim), np.nan, np.float32), np.full((item.pool_rows, item.label_dim), np.nan, np.float32)
            if self.x is not None:
                nx[:self.x.shape[0]] = self.x; ny[:self.y.shape[0]] = self.y
            self.x, self.y = nx, ny
            fr = np.zeros(item.pool_rows, bool); fr[:self._freed_rows.shape[0]] = self._freed_rows
            self._freed_rows = fr
        ups = []
        for first, rx, ry in item.uploads:
            n = rx.shape[0]
            assert first % 4 == 0, "a slot starts on a multiple of 4"
            for f, (rows, _) in self.live.items():
                assert first + n <= f or f + rows <= first, "live slots overlap: [%d, %d) and [%d, %d)" % (first, first + n, f, f + rows)
            if self._freed_rows[first:first + n].any():
                self.reuses += 1
            self._freed_rows[first:first + n] = False
            if item.stats is not None:
                mi, si, ml, sl = item.stats
                nxt, nyt = apply_cmvn(rx, ry, {"mean_inputs": mi, "stddev_inputs": si, "mean_labels": ml, "stddev_labels": sl})
            else:
                nxt, nyt = rx, ry
            self.x[first:first + n] = nxt.astype(np.float32); self.y[first:first + n] = nyt.astype(np.float32)
            self.live[first] = [n, n]
            ups.append((first, n))
        freed = []
        for row, lo, hi in item.picks.tolist():
            ent = self.live.get(lo)
            assert ent is not None and lo + ent[0] == hi and lo <= row < hi, "a pick names rows no live utterance holds"
            ent[1] -= 1
            assert ent[1] >= 0, "more frames drawn from an utterance than it has"
        for lo in sorted({int(v) for v in item.picks[:, 1]}):
            if self.live[lo][1] == 0:                   # the last frame was drawn: only now may the rows be handed out again
                self._freed_rows[lo:lo + self.live[lo][0]] = True
                del self.live[lo]
                freed.append(lo)
        self.history.append((item.pool_rows, ups, freed))
        return gather(self.x, item.picks, item.left, item.right), gather(self.y, item.picks, 0, 0)


def frame_data(tmp, n, rng, din=3, dout=2, tag="tr", lengths=None, random_values=False):
    """the archives of tests/test_frame_level_loop.py (_data): n utterances of 40 .. 89 frames (or `lengths`), input column 0 the
    utterance, column 1 the frame, labels 2 x the first dout input columns; random_values: Gaussian frames instead"""
    wi, wl = ArkWriter(str(tmp / (tag + "_in.scp"))), ArkWriter(str(tmp / (tag + "_lab.scp")))
    total = 0
    for i in range(n if lengths is None else len(lengths)):
        T = int(rng.integers(40, 90)) if lengths is None else int(lengths[i])
        total += T
        if random_values:
            x = (rng.standard_normal((T, din)) * 2 + 1).astype(np.float32)
            y = (rng.standard_normal((T, dout)) - 1).astype(np.float32)
        else:
            x = np.zeros((T, din), np.float32); x[:, 0] = i; x[:, 1] = np.arange(T)
            y = 2.0 * x[:, :dout]
        wi.write_next_utt(str(tmp / (tag + "_in.ark")), "%s%02d" % (tag, i), x)
        wl.write_next_utt(str(tmp / (tag + "_lab.ark")), "%s%02d" % (tag, i), y)
    wi.close(); wl.close()
    return str(tmp / (tag + "_in.scp")), str(tmp / (tag + "_lab.scp")), total
