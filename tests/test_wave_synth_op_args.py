"""rsrgan_wave_synth (csrc/synth.hip) refuses every argument error before its first HIP call, as rsrgan_feat_wave does
(tests/test_wave_op_args.py), naming the argument in rsrgan_last_error(); rsrgan_wave_synth_work and rsrgan_wave_synth_chunk answer on
the host.  The pointers are made-up addresses: a refused call never reads them, and no device is needed."""
import pytest

from rsrgan_amd import _lib
from tests.test_op_args import P, refused

WORK = 1 << 30


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def syn(lib, **kw):
    a = dict(pcm=P, kind=0, n_samples=16000, seg=P + 65536, offsets=P + 69632, lps=P + 131072, lps_rows=100, B=4, N=400, S=160, P=512,
             preemph=0.97, window=P + 73728, twiddle=P + 77824, out=P + 81920, out_samples=16000, out_seg=P + 196608, work=P + 262144,
             work_bytes=WORK)
    a.update(kw)
    return lib.rsrgan_wave_synth(a["pcm"], a["kind"], a["n_samples"], a["seg"], a["offsets"], a["lps"], a["lps_rows"], a["B"], a["N"], a["S"],
                                 a["P"], a["preemph"], a["window"], a["twiddle"], a["out"], a["out_samples"], a["out_seg"], a["work"],
                                 a["work_bytes"], None)


def test_symbols_are_bound(lib):
    for s in ("rsrgan_wave_synth", "rsrgan_wave_synth_work", "rsrgan_wave_synth_chunk"):
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert len(lib.rsrgan_wave_synth.argtypes) == 20


def test_chunk_and_work(lib):
    ch = lib.rsrgan_wave_synth_chunk()
    assert ch >= 64 and ch & (ch - 1) == 0
    # lps_rows * N floats and ceil(out_samples / CH) + B carries
    assert lib.rsrgan_wave_synth_work(4, 100, 16000, 400) == 4 * (100 * 400 + -(-16000 // ch) + 4)
    assert lib.rsrgan_wave_synth_work(1, 1, 1, 1) == 4 * (1 + 1 + 1)
    assert lib.rsrgan_wave_synth_work(65535, 1 << 40, 1 << 40, 2048) == 4 * ((2048 << 40) + ((1 << 40) // ch) + 65535)
    for bad in ((0, 100, 16000, 400), (-1, 100, 16000, 400), (65536, 100, 16000, 400), (4, 0, 16000, 400), (4, (1 << 40) + 1, 16000, 400),
                (4, 100, 0, 400), (4, 100, -5, 400), (4, 100, (1 << 40) + 1, 400), (4, 100, 16000, 0), (4, 100, 16000, 2049)):
        assert lib.rsrgan_wave_synth_work(*bad) == 0, bad


@pytest.mark.parametrize("which", ["pcm", "seg", "offsets", "out"])
def test_null_required_pointer(lib, which):
    refused(lib, syn(lib, **{which: None}), "wave_synth", "null pointer (pcm, seg, offsets or out)")


@pytest.mark.parametrize("which", ["window", "twiddle"])
def test_null_table(lib, which):
    refused(lib, syn(lib, **{which: None}), "wave_synth", "null pointer (window or twiddle)")


@pytest.mark.parametrize("which", ["lps", "out_seg", "work"])
def test_null_new_pointer(lib, which):
    refused(lib, syn(lib, **{which: None}), "wave_synth", "null pointer (lps, out_seg or work)")


@pytest.mark.parametrize("kind", [-1, 2, 7])
def test_unknown_kind(lib, kind):
    refused(lib, syn(lib, kind=kind), "wave_synth", "kind = %d" % kind)


def test_alignment(lib):
    refused(lib, syn(lib, pcm=P + 1), "wave_synth", "pcm not aligned to its 2-byte samples")
    for off in (1, 2, 3):
        refused(lib, syn(lib, kind=1, pcm=P + off), "wave_synth", "pcm not aligned to its 4-byte samples")
    for which in ("lps", "work"):
        for off in (1, 2, 4, 8):
            refused(lib, syn(lib, **{which: P + 131072 + off}), "wave_synth", "lps or work not 16-byte aligned")
    for which in ("seg", "out_seg"):
        for off in (1, 2, 4):
            refused(lib, syn(lib, **{which: P + 65536 + off}), "wave_synth", "seg or out_seg not 8-byte aligned")
    for which in ("offsets", "window", "twiddle", "out"):
        for off in (1, 2):
            refused(lib, syn(lib, **{which: P + 69632 + off}), "wave_synth", "offsets, window, twiddle or out not 4-byte aligned")


@pytest.mark.parametrize("b", [0, -1, 65536])
def test_batch(lib, b):
    refused(lib, syn(lib, B=b), "wave_synth", "B = %d outside [1, 65535]" % b)


def test_counts(lib):
    for v in (0, -1):
        refused(lib, syn(lib, n_samples=v), "wave_synth", "n_samples must be positive")
        refused(lib, syn(lib, lps_rows=v), "wave_synth", "lps_rows = %d outside [1, 2^40]" % v)
        refused(lib, syn(lib, out_samples=v), "wave_synth", "out_samples = %d outside [1, 2^40]" % v)
    big = (1 << 40) + 1
    refused(lib, syn(lib, n_samples=big), "wave_synth", "n_samples", "above the entry's 2^40")
    refused(lib, syn(lib, lps_rows=big), "wave_synth", "lps_rows = %d outside [1, 2^40]" % big)
    refused(lib, syn(lib, out_samples=big), "wave_synth", "out_samples = %d outside [1, 2^40]" % big)


@pytest.mark.parametrize("p", [0, 32, 63, 500, 513, 4096, -512])
def test_padded_length(lib, p):
    refused(lib, syn(lib, P=p, N=min(400, max(p, 1)), S=1), "wave_synth", "P = %d is no power of two in [64, 2048]" % p)


@pytest.mark.parametrize("n,s,p", [(400, 0, 512), (400, -160, 512), (400, 401, 512), (513, 160, 512), (0, 0, 512), (65, 1, 64)])
def test_frame_sizes(lib, n, s, p):
    refused(lib, syn(lib, N=n, S=s, P=p), "wave_synth", "outside 1 <= S <= N <= P")


@pytest.mark.parametrize("c", [-0.01, 1.01, float("nan"), float("inf")])
def test_preemph(lib, c):
    refused(lib, syn(lib, preemph=c), "wave_synth", "preemph", "outside [0, 1]")


def test_short_work(lib):
    need = lib.rsrgan_wave_synth_work(4, 100, 16000, 400)
    for wb in (need - 1, need - 4, 0, -1):
        refused(lib, syn(lib, work_bytes=wb), "wave_synth", "work_bytes = %d below the %d bytes" % (wb, need))
    # more rows or more output samples need more
    refused(lib, syn(lib, work_bytes=need, lps_rows=101), "wave_synth", "work_bytes")
    refused(lib, syn(lib, work_bytes=need, out_samples=16000 + lib.rsrgan_wave_synth_chunk()), "wave_synth", "work_bytes")
