"""frontend.FrontEnd without a model: a bare FrontEnd() featurizes packed, coded and waveform batches to the bits the engine's loop tests
hold HipEngine.featurize to (tests/feat_ref.expand, tests/feat_decode_ref.expand_coded, rsrgan_feat_wave then rsrgan_feat_batch), has no
length limit where a HipEngine of max_frames = 8 refuses, and hands its results over as handoff() says: ready=True results pass
upload_ready without a device wait, ready=False results are ordered behind the upload stream by an event alone."""
import numpy as np
import pytest
import torch

from rsrgan_amd.io import wave as W
from tests import feat_decode_ref, feat_ref

pytestmark = pytest.mark.gpu

LEFT, RIGHT, D = 2, 1, 7
LENGTHS = [5, 1, 3]


@pytest.fixture(scope="module")
def fe():
    from rsrgan_amd.frontend import FrontEnd
    return FrontEnd()


@pytest.fixture(scope="module")
def engine8():
    from rsrgan_amd.engine_hip import HipEngine
    eng = HipEngine(batch_size=3, max_frames=8, input_dim=D * (LEFT + 1 + RIGHT), output_dim=5, g_layers=2, g_cells=12, g_proj=7, d_layers=2,
                    d_cells=8, d_proj=5)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def packed():
    """(the batch, its reference expansion): three utterances of 5, 1 and 3 frames, D = 7, context 2 / 1, statistics"""
    rng = np.random.default_rng(11)
    p = feat_ref.random_packed(rng, LENGTHS, D, LEFT, RIGHT, stats=feat_ref.seeded_stats(rng, D))
    return p, feat_ref.expand(p, (p.mean, p.stddev), LEFT, RIGHT, max(LENGTHS))


def _bits_equal(t, want):
    return torch.equal(t.cpu().view(torch.int32), torch.from_numpy(np.ascontiguousarray(want, np.float32)).view(torch.int32))


@pytest.fixture()
def syncs(monkeypatch):
    """how often torch.cuda.synchronize ran"""
    calls, real = [], torch.cuda.synchronize

    def synchronize(*a, **k):
        calls.append(a)
        return real(*a, **k)
    monkeypatch.setattr(torch.cuda, "synchronize", synchronize)
    return calls


def test_packed_batch_equals_the_reference(fe, packed):
    p, (want, want_len) = packed
    x, ln = fe.featurize(p, ready=True)                              # (complete on return: no synchronize before the copies)
    assert x.shape == want.shape == (3, 5, D * 4) and _bits_equal(x, want) and ln.cpu().tolist() == want_len.tolist() == LENGTHS


def test_coded_batch_equals_the_reference(fe):
    rng = np.random.default_rng(12)
    mats = [rng.standard_normal((n, D)) * 2 + 1 for n in LENGTHS]
    cb = feat_decode_ref.coded_batch(mats, "CDF", LEFT, RIGHT, stats=feat_ref.seeded_stats(rng, D))
    want, want_len = feat_decode_ref.expand_coded(cb)
    x, ln = fe.featurize(cb, ready=True)
    assert x.shape == want.shape == (3, 5, D * 4) and _bits_equal(x, want) and ln.cpu().tolist() == want_len.tolist() == LENGTHS


def test_no_max_frames_no_limit(fe, engine8):
    rng = np.random.default_rng(13)
    p = feat_ref.random_packed(rng, [11, 1, 3], D, LEFT, RIGHT, stats=feat_ref.seeded_stats(rng, D))
    assert fe.max_frames is None
    x, ln = fe.featurize(p, ready=True)
    want, want_len = feat_ref.expand(p, (p.mean, p.stddev), LEFT, RIGHT, 11)
    assert _bits_equal(x, want) and ln.cpu().tolist() == want_len.tolist() == [11, 1, 3]
    with pytest.raises(ValueError, match="longer than max_frames = 8"):
        engine8.featurize(p)
    x8, _ = engine8.featurize(p, ready=True, limit=False)            # (the engine's own front end, limit waived: the same bits)
    assert torch.equal(x8.view(torch.int32), x.view(torch.int32))


def test_wave_batch_equals_wave_then_batch(fe):
    rng = np.random.default_rng(14)
    utts = [np.clip(np.rint(rng.standard_normal(n) * 3000), -32768, 32767).astype(np.int16) for n in (400, 560, 1040)]
    mean, std = 20.0 + rng.standard_normal(257), rng.uniform(2.0, 4.0, 257)
    wb = W.pack_wave(utts, None, LEFT, RIGHT, mean, std)
    assert wb.lengths().tolist() == [1, 2, 5] and wb.shape == (3, 5, 257 * 4)
    x, ln = fe.featurize(wb, ready=True)
    assert ln.cpu().tolist() == [1, 2, 5]
    us = fe.upload_stream()
    with torch.cuda.stream(us):
        raw, off = fe.wave_features(wb.samples, wb.seg, wb.offsets, int(wb.offsets[-1]), wb.spec, us)
        dm, ds = torch.from_numpy(mean).to(fe.device), torch.from_numpy(std).to(fe.device)
        want = torch.empty_like(x)
        fe.op_feat_batch(raw, off, 3, 5, 257, LEFT, RIGHT, dm, ds, want, stream=us)
    us.synchronize()
    assert raw.shape == (8, 257) and torch.equal(x.view(torch.int32), want.view(torch.int32))


def test_ready_results_pass_upload_ready_without_a_wait(fe, packed, syncs, tmp_path):
    from rsrgan_amd.io import FrameBatchReader
    from tests.feat_frames_ref import frame_data
    p, (want, _) = packed
    x, ln = fe.featurize(p, ready=True)
    assert fe.upload_ready(x) is x and fe.upload_ready(ln, int32=True) is ln and syncs == []
    xs, ls, _ = frame_data(tmp_path, 3, np.random.default_rng(15), lengths=[6, 4, 5])
    default = next(iter(FrameBatchReader(xs, ls, 8, LEFT, RIGHT, num_threads=0, shuffle=False)))
    item = next(iter(FrameBatchReader(xs, ls, 8, LEFT, RIGHT, num_threads=0, shuffle=False, device_features=True)))
    fx, flab = fe.featurize_frames(item, ready=True)
    assert fe.upload_ready(fx) is fx and fe.upload_ready(flab) is flab and syncs == []
    assert _bits_equal(fx, default[0]) and _bits_equal(flab, default[1])
    # a result handed over by event is nobody's word that it is complete: one device wait, once per tensor object
    y, _ = fe.featurize(p)
    assert fe.upload_ready(y) is y and len(syncs) == 1
    assert fe.upload_ready(y) is y and len(syncs) == 1
    assert _bits_equal(x, want) and _bits_equal(y, want)


def test_event_handoff_orders_the_current_stream_behind_the_upload_stream(fe, packed):
    p, (want, want_len) = packed
    torch.cuda.synchronize()
    with torch.cuda.stream(fe.upload_stream()):
        torch.cuda._sleep(20_000_000)                                # (milliseconds of device time in front of the uploads and the kernel)
    x, ln = fe.featurize(p)
    cur = torch.cuda.current_stream(fe.device)
    xc, lc = x.clone(), ln.clone()                                   # read on the current stream, behind nothing but the event
    cur.synchronize()                                                # (the host waits for the CURRENT stream only)
    assert _bits_equal(xc, want) and lc.cpu().tolist() == want_len.tolist()
