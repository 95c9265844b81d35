"""rsrgan_feat_wave (csrc/wave.hip k_feat_wave) refuses every argument error before its first HIP call, as rsrgan_feat_decode does
(tests/test_feat_decode_op_args.py), naming the argument in rsrgan_last_error().  The pointers are made-up addresses: a refused call
never reads them, and no device is needed."""
import pytest

from rsrgan_amd import _lib
from tests.test_op_args import P, refused


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def wav(lib, **kw):
    a = dict(pcm=P, kind=0, n_samples=16000, seg=P + 65536, offsets=P + 69632, B=4, N=400, S=160, P=512, preemph=0.97, window=P + 73728,
             twiddle=P + 77824, out=P + 81920, out_rows=100)
    a.update(kw)
    return lib.rsrgan_feat_wave(a["pcm"], a["kind"], a["n_samples"], a["seg"], a["offsets"], a["B"], a["N"], a["S"], a["P"], a["preemph"],
                                a["window"], a["twiddle"], a["out"], a["out_rows"], None)


def test_symbols_are_bound(lib):
    for s in ("rsrgan_feat_wave", "rsrgan_feat_wave_frames"):
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert len(lib.rsrgan_feat_wave.argtypes) == 15


def test_frames_per_workgroup(lib):
    assert lib.rsrgan_feat_wave_frames(512) >= 1
    for p in (64, 128, 256, 1024, 2048):
        assert lib.rsrgan_feat_wave_frames(p) >= 1
    for p in (0, 32, 500, 4096, -512):
        assert lib.rsrgan_feat_wave_frames(p) == 0


@pytest.mark.parametrize("which", ["pcm", "seg", "offsets", "out"])
def test_null_required_pointer(lib, which):
    refused(lib, wav(lib, **{which: None}), "feat_wave", "null pointer (pcm, seg, offsets or out)")


@pytest.mark.parametrize("which", ["window", "twiddle"])
def test_null_table(lib, which):
    refused(lib, wav(lib, **{which: None}), "feat_wave", "null pointer (window or twiddle)")


@pytest.mark.parametrize("kind", [-1, 2, 7])
def test_unknown_kind(lib, kind):
    refused(lib, wav(lib, kind=kind), "feat_wave", "kind = %d" % kind)


def test_alignment(lib):
    refused(lib, wav(lib, pcm=P + 1), "feat_wave", "pcm not aligned to its 2-byte samples")
    for off in (1, 2, 3):
        refused(lib, wav(lib, kind=1, pcm=P + off), "feat_wave", "pcm not aligned to its 4-byte samples")
    for off in (1, 2, 4, 8):
        refused(lib, wav(lib, out=P + 81920 + off), "feat_wave", "out not 16-byte aligned")
    for off in (1, 2, 4):
        refused(lib, wav(lib, seg=P + 65536 + off), "feat_wave", "seg not 8-byte aligned")
    for which in ("offsets", "window", "twiddle"):
        for off in (1, 2):
            refused(lib, wav(lib, **{which: P + 69632 + off}), "feat_wave", "offsets, window or twiddle not 4-byte aligned")


@pytest.mark.parametrize("which", ["B", "n_samples", "out_rows"])
def test_sizes_below_one(lib, which):
    for v in (0, -1):
        refused(lib, wav(lib, **{which: v}), "feat_wave", "must be positive")


@pytest.mark.parametrize("p", [0, 32, 63, 500, 513, 4096, -512])
def test_padded_length(lib, p):
    refused(lib, wav(lib, P=p, N=min(400, max(p, 1)), S=1), "feat_wave", "P = %d is no power of two in [64, 2048]" % p)


@pytest.mark.parametrize("n,s,p", [(400, 0, 512), (400, -160, 512), (400, 401, 512), (513, 160, 512), (0, 0, 512), (65, 1, 64)])
def test_frame_sizes(lib, n, s, p):
    refused(lib, wav(lib, N=n, S=s, P=p), "feat_wave", "outside 1 <= S <= N <= P")


@pytest.mark.parametrize("c", [-0.01, 1.01, float("nan"), float("inf")])
def test_preemph(lib, c):
    refused(lib, wav(lib, preemph=c), "feat_wave", "preemph", "outside [0, 1]")


def test_limit(lib):
    """the limit include/rsrgan.h states: at most 2^40 output floats"""
    refused(lib, wav(lib, out_rows=(1 << 40) // 257 + 1), "feat_wave", "out_rows x (P / 2 + 1)", "above the entry's 2^40")
    refused(lib, wav(lib, out_rows=(1 << 40) // 33 + 1, P=64, N=64, S=64), "feat_wave", "above the entry's 2^40")
    refused(lib, wav(lib, out_rows=(1 << 62)), "feat_wave", "above the entry's 2^40")
