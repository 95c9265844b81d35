"""The host side of the device decode: ArkReader.read_coded, io.CodedBatch and the readers' device_decode=True.  The coded items carry
the archives' bytes undecoded; expanded on the host (tests/feat_decode_ref.py: read_compress, apply_cmvn, splice_feats, the padding rule)
they are the default readers' items bit for bit -- same ids, order and lengths -- over archives that mix float, double and compressed
utterances.  No device in here."""
import numpy as np
import pytest

from rsrgan_amd.io import ArkReader, CodedBatch, FrameBatchReader, FrameDraw, PaddedBatchReader, PoolLedger, pack_coded, prefetch
from rsrgan_amd.io.kaldi_ark import KIND_COMPRESSED, KIND_DOUBLE, KIND_FLOAT
from tests import feat_decode_ref as R
from tests import feat_frames_ref
from tests.feat_ref import cmvn_for

DIN, DOUT, B = 6, 3, 4
LENGTHS = [7, 3, 9, 5, 6, 2, 9, 4, 8, 1, 12, 2]      # ragged, several shorter than the context


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _data(tmp_path, seed=3):
    rng = np.random.default_rng(seed)
    scp = R.write_arks(tmp_path, "tr", LENGTHS, DIN, DOUT, rng)
    return scp, cmvn_for(rng, DIN, DOUT)


@pytest.mark.parametrize("with_cmvn", [True, False], ids=["cmvn", "raw"])
@pytest.mark.parametrize("left,right", [(5, 5), (2, 1), (0, 0)])
def test_padded_reader_items_expand_to_the_default_readers(tmp_path, left, right, with_cmvn):
    scp, cmvn = _data(tmp_path)
    cmvn = cmvn if with_cmvn else None
    mk = lambda **k: PaddedBatchReader(scp[0], scp[1], B, left, right, cmvn=cmvn, num_buckets=1, shuffle=True, seed=5, **k)
    want, got = list(mk()), list(mk(device_decode=True))
    assert len(want) == len(got) == 3
    kinds = set()
    for w, g in zip(want, got):
        assert isinstance(g[1], CodedBatch) and isinstance(g[2], CodedBatch)
        assert g[1].shape == w[1].shape and g[2].shape == w[2].shape and len(g[1]) == len(w[0])
        kinds |= set(g[1].seg[:, 1].tolist())
        e = R.expand_item(g)
        assert e[0] == w[0]
        assert _same(e[1], w[1]) and _same(e[2], w[2]) and _same(e[3], w[3]) and _same(g[3], w[3])
    assert kinds == {KIND_FLOAT, KIND_DOUBLE, KIND_COMPRESSED}


def test_device_decode_implies_device_features_and_leaves_the_plan_alone(tmp_path):
    scp, cmvn = _data(tmp_path)
    mk = lambda **k: PaddedBatchReader(scp[0], scp[1], B, 2, 1, cmvn=cmvn, shuffle=True, seed=9, **k)
    r = mk(device_decode=True)
    assert r.device_decode and r.device_features and not mk(device_features=True).device_decode
    assert list(r.plan()) == list(mk().plan())


@pytest.mark.parametrize("with_cmvn,ctx", [(True, 5), (False, 0), (True, (2, 1))], ids=["cmvn-5", "raw-0", "cmvn-2-1"])
def test_frame_reader_items_expand_to_the_default_readers(tmp_path, with_cmvn, ctx):
    left, right = ctx if isinstance(ctx, tuple) else (ctx, ctx)
    rng = np.random.default_rng(11)
    lengths = rng.integers(40, 90, 25)
    scp = R.write_arks(tmp_path, "fr", lengths, DIN, DOUT, rng)
    cmvn = cmvn_for(rng, DIN, DOUT) if with_cmvn else None
    mk = lambda **k: FrameBatchReader(scp[0], scp[1], 32, left, right, cmvn=cmvn, num_threads=0, shuffle=True, seed=3, **k)
    want, dev = list(mk()), mk(device_decode=True, initial_pool_rows=64)
    assert dev.device_features
    pool, ledger = feat_frames_ref.HostPool(dev.reader_id), PoolLedger(dev.reader_id)
    got, kinds = 0, set()
    for k, item in enumerate(dev):
        ledger.admit(item)                                             # the consumer's checks take the coded form
        # the stand-in's pool takes final float32 rows: decode each coded admission with the host reader's own functions and normalise
        # from the DECODED float64, as the default reader does
        ups = []
        for first, cx, cy in item.uploads:
            assert isinstance(cx.data, bytes) and isinstance(cy.data, bytes)
            kinds.add(cx.kind)
            x, y = (R.decode_segment(c.kind, c.rows, c.cols, c.min, c.range, c.data).astype(np.float64) for c in (cx, cy))
            if cmvn is not None:
                x, y = R.apply_cmvn(x, y, cmvn)
            ups.append((first, x.astype(np.float32), y.astype(np.float32)))
        x, lab = pool.feed(FrameDraw(item.serial, item.reader_id, ups, item.pool_rows, item.picks, item.left, item.right, None,
                                     item.input_dim, item.label_dim))
        assert _same(x, want[k][0]) and _same(lab, want[k][1]), k
        got += 1
    assert got == len(want) == int(lengths.sum()) // 32 and kinds == {0, 1, 2}


def test_read_coded_returns_the_files_bytes(tmp_path):
    rng = np.random.default_rng(2)
    mats = [("a", rng.standard_normal((13, 5)), "F"), ("b", rng.standard_normal((9, 7)), "D"), ("c", rng.standard_normal((37, 4)) * 3, "C"),
            ("d", rng.standard_normal((1, 5)), "C")]
    ark, scp = str(tmp_path / "m.ark"), str(tmp_path / "m.scp")
    R.write_archive(ark, scp, mats)
    whole = open(ark, "rb").read()
    rd = ArkReader()
    rd(scp)
    for i, (utt, m, kind) in enumerate(mats):
        c = rd.read_coded_from_index(i)
        n, D = m.shape
        assert (c.kind, c.rows, c.cols, c.shape) == (R.KINDS[kind], n, D, (n, D))
        rec = R.record(m, kind)
        head = 21 if kind == "C" else 15
        at = int(rd.scp_data[i][1])
        assert bytes(c.data) == rec[head:] == whole[at + head:at + len(rec)]
        assert len(c.data) == {"F": 4 * n * D, "D": 8 * n * D, "C": 8 * D + n * D}[kind]
        if kind == "C":
            assert (c.min, c.range) == tuple(float(v) for v in np.frombuffer(rec[5:13], "<f4"))
        # and decoding those bytes is what read_ark returns
        assert _same(np.asarray(R.decode_segment(c.kind, n, D, c.min, c.range, c.data)), np.asarray(rd.read_utt_data_from_index(i)))


def test_read_coded_raises_what_read_ark_raises(tmp_path):
    bad = {"text": b"x [ 1 2 ]", "cm2": b"\0BCM2" + bytes(16), "empty": b"\0BCM " + bytes(16), "type": b"\0BXM \4\1\0\0\0\4\1\0\0\0" + bytes(8)}
    rd = ArkReader()
    for tag, data in bad.items():
        p = str(tmp_path / tag)
        open(p, "wb").write(data)
        with pytest.raises(ValueError) as a:
            rd.read_ark(p, 0)
        with pytest.raises(ValueError) as b:
            rd.read_coded(p, 0)
        assert str(a.value) == str(b.value), tag


def test_the_blob_holds_the_archives_bytes_and_little_else(tmp_path):
    scp, cmvn = _data(tmp_path)
    for item in PaddedBatchReader(scp[0], scp[1], B, 2, 1, cmvn=cmvn, num_buckets=1, shuffle=False, device_decode=True):
        for cb, D in ((item[1], DIN), (item[2], DOUT)):
            n = np.diff(cb.offsets)
            sizes = [{0: 4 * k * D, 1: 8 * k * D, 2: 8 * D + k * D}[int(kind)] for k, kind in zip(n, cb.seg[:, 1])]
            assert sum(sizes) <= cb.blob.nbytes <= sum(sizes) + 15 * len(n)
            assert np.all(cb.seg[:, 0] % 16 == 0) and cb.blob.dtype == np.uint8
            assert cb.seg.dtype == np.int64 and cb.scale.dtype == np.float32 and cb.offsets.dtype == np.int32
            assert cb.nbytes() == cb.blob.nbytes + cb.seg.nbytes + cb.scale.nbytes + cb.offsets.nbytes


def test_rows_shards_as_packed_batch_rows_does(tmp_path):
    rng = np.random.default_rng(8)
    mats = [rng.standard_normal((n, 5)) * 2 for n in (4, 9, 1, 6, 3, 7)]
    stats = (rng.standard_normal(5), rng.uniform(0.5, 2, 5))
    cb = R.coded_batch(mats, "CFDCCD", 2, 1, stats)
    X, L = R.expand_coded(cb)
    for lo, hi in ((0, 6), (0, 3), (3, 6), (2, 3), (4, 4)):
        s = cb.rows(lo, hi)
        assert s.shape == (hi - lo,) + cb.shape[1:] and (s.left, s.right) == (2, 1) and s.mean is cb.mean and s.stddev is cb.stddev
        assert s.offsets[0] == 0 and s.offsets.tolist() == (cb.offsets[lo:hi + 1] - cb.offsets[lo]).tolist()
        assert (hi == lo or s.seg[0, 0] == 0) and np.all(s.seg[:, 0] % 16 == 0)
        sizes = sum(R.coded_bytes(int(k), int(n), 5) for k, n in zip(s.seg[:, 1], np.diff(s.offsets)))
        assert s.blob.nbytes <= max(sizes + 15 * (hi - lo), 16)                        # only the shard's bytes travel
        x, ln = R.expand_coded(s)
        assert _same(x, X[lo:hi]) and _same(ln, L[lo:hi]) and _same(s.lengths(), cb.lengths()[lo:hi])
    with pytest.raises(ValueError, match="outside the batch"):
        cb.rows(2, 7)


def test_the_constructor_refuses_what_the_device_cannot_check():
    rng = np.random.default_rng(1)
    cb = R.coded_batch([rng.standard_normal((5, 3)), rng.standard_normal((4, 3))], "CF")
    mk = lambda **k: CodedBatch(**dict(dict(blob=cb.blob, seg=cb.seg, scale=cb.scale, offsets=cb.offsets, shape=cb.shape), **k))
    mk()
    with pytest.raises(ValueError, match="does not lie in the blob"):
        mk(blob=cb.blob[:-16])                                         # the last segment leaves the blob
    seg = cb.seg.copy(); seg[1, 0] += 16
    with pytest.raises(ValueError, match="does not lie in the blob"):
        mk(seg=seg)
    seg = cb.seg.copy(); seg[0, 0] = 8
    with pytest.raises(ValueError, match="multiples of 16"):
        mk(seg=seg)
    seg = cb.seg.copy(); seg[1, 1] = 3
    with pytest.raises(ValueError, match="unknown kind 3"):
        mk(seg=seg)
    with pytest.raises(ValueError, match="never decrease"):
        mk(offsets=np.array([0, 5, 4], np.int32))
    with pytest.raises(ValueError, match="B \\+ 1"):
        mk(offsets=np.array([0, 5], np.int32))


def test_prefetch_keeps_the_order(tmp_path):
    scp, cmvn = _data(tmp_path)
    mk = lambda: PaddedBatchReader(scp[0], scp[1], B, 2, 1, cmvn=cmvn, num_buckets=1, shuffle=True, seed=4, device_decode=True)
    want = list(mk())
    for threads in (1, 3):
        got = list(prefetch(mk(), capacity=2, threads=threads))
        assert [g[0] for g in got] == [w[0] for w in want]
        for g, w in zip(got, want):
            assert _same(g[1].blob, w[1].blob) and _same(g[2].blob, w[2].blob) and _same(g[3], w[3])


def test_device_features_alone_still_refuses_other_encodings(tmp_path):
    scp, cmvn = _data(tmp_path)
    with pytest.raises(ValueError, match="float32"):
        list(PaddedBatchReader(scp[0], scp[1], B, 2, 1, cmvn=cmvn, num_buckets=1, shuffle=False, device_features=True))


def test_pack_coded_refuses_mixed_widths():
    rng = np.random.default_rng(0)
    rd_items = [R.coded_batch([rng.standard_normal((3, d))], "F") for d in (4, 5)]
    from rsrgan_amd.io import CodedMatrix
    mats = [CodedMatrix(0, 3, c.dim, 0.0, 0.0, bytes(c.blob[:4 * 3 * c.dim])) for c in rd_items]
    with pytest.raises(ValueError, match="columns"):
        pack_coded(mats)
