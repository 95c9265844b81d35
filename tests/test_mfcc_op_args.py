"""rsrgan_feat_mfcc (csrc/wave.hip k_feat_mfcc) refuses every argument error before its first HIP call, as rsrgan_feat_wave does
(tests/test_wave_op_args.py), naming the argument in rsrgan_last_error().  The pointers are made-up addresses: a refused call never reads
them, and no device is needed."""
import pytest

from rsrgan_amd import _lib
from tests.test_op_args import P, refused

PTRS = dict(pcm=P, seg=P + 65536, offsets=P + 69632, window=P + 73728, twiddle=P + 77824, out=P + 81920, mel_seg=P + 2 * 65536,
            mel_w=P + 3 * 65536, dct=P + 4 * 65536)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def mfcc(lib, **kw):
    a = dict(PTRS, kind=0, n_samples=16000, B=4, N=400, S=160, P=512, preemph=0.97, nnz=468, M=40, C=40, out_rows=100)
    a.update(kw)
    return lib.rsrgan_feat_mfcc(a["pcm"], a["kind"], a["n_samples"], a["seg"], a["offsets"], a["B"], a["N"], a["S"], a["P"], a["preemph"],
                                a["window"], a["twiddle"], a["mel_seg"], a["mel_w"], a["nnz"], a["M"], a["dct"], a["C"], a["out"],
                                a["out_rows"], None)


def test_symbol_is_bound(lib):
    assert "rsrgan_feat_mfcc" in _lib.SYMBOLS and hasattr(lib, "rsrgan_feat_mfcc")
    assert len(lib.rsrgan_feat_mfcc.argtypes) == 21


@pytest.mark.parametrize("which", ["pcm", "seg", "offsets", "out"])
def test_null_required_pointer(lib, which):
    refused(lib, mfcc(lib, **{which: None}), "feat_mfcc", "null pointer (pcm, seg, offsets or out)")


@pytest.mark.parametrize("which", ["window", "twiddle"])
def test_null_table(lib, which):
    refused(lib, mfcc(lib, **{which: None}), "feat_mfcc", "null pointer (window or twiddle)")


@pytest.mark.parametrize("which", ["mel_seg", "mel_w"])
def test_null_mel_table(lib, which):
    refused(lib, mfcc(lib, **{which: None}), "feat_mfcc", "null pointer (mel_seg or mel_w)")


def test_dct_and_c_go_together(lib):
    refused(lib, mfcc(lib, dct=None), "feat_mfcc", "null pointer (dct)", "C = 40")
    refused(lib, mfcc(lib, C=0), "feat_mfcc", "dct given with C = 0")


@pytest.mark.parametrize("kind", [-1, 2, 7])
def test_unknown_kind(lib, kind):
    refused(lib, mfcc(lib, kind=kind), "feat_mfcc", "kind = %d" % kind)


def test_alignment(lib):
    refused(lib, mfcc(lib, pcm=P + 1), "feat_mfcc", "pcm not aligned to its 2-byte samples")
    for off in (1, 2, 3):
        refused(lib, mfcc(lib, kind=1, pcm=P + off), "feat_mfcc", "pcm not aligned to its 4-byte samples")
    for off in (1, 2, 4, 8):
        refused(lib, mfcc(lib, out=PTRS["out"] + off), "feat_mfcc", "out not 16-byte aligned")
    for off in (1, 2, 4):
        refused(lib, mfcc(lib, seg=PTRS["seg"] + off), "feat_mfcc", "seg not 8-byte aligned")
    for which in ("offsets", "window", "twiddle"):
        for off in (1, 2):
            refused(lib, mfcc(lib, **{which: PTRS[which] + off}), "feat_mfcc", "offsets, window or twiddle not 4-byte aligned")
    for which in ("mel_seg", "mel_w", "dct"):
        for off in (1, 2, 3):
            refused(lib, mfcc(lib, **{which: PTRS[which] + off}), "feat_mfcc", "mel_seg, mel_w or dct not 4-byte aligned")


@pytest.mark.parametrize("which", ["B", "n_samples", "out_rows"])
def test_sizes_below_one(lib, which):
    for v in (0, -1):
        refused(lib, mfcc(lib, **{which: v}), "feat_mfcc", "must be positive")


@pytest.mark.parametrize("p", [0, 32, 63, 500, 513, 4096, -512])
def test_padded_length(lib, p):
    refused(lib, mfcc(lib, P=p, N=min(400, max(p, 1)), S=1), "feat_mfcc", "P = %d is no power of two in [64, 2048]" % p)


@pytest.mark.parametrize("n,s,p", [(400, 0, 512), (400, -160, 512), (400, 401, 512), (513, 160, 512), (0, 0, 512), (65, 1, 64)])
def test_frame_sizes(lib, n, s, p):
    refused(lib, mfcc(lib, N=n, S=s, P=p), "feat_mfcc", "outside 1 <= S <= N <= P")


@pytest.mark.parametrize("c", [-0.01, 1.01, float("nan"), float("inf")])
def test_preemph(lib, c):
    refused(lib, mfcc(lib, preemph=c), "feat_mfcc", "preemph", "outside [0, 1]")


@pytest.mark.parametrize("m", [0, -1, 129, 1 << 20])
def test_mel_bins(lib, m):
    refused(lib, mfcc(lib, M=m, C=0, dct=None), "feat_mfcc", "M = %d outside [1, 128]" % m)


@pytest.mark.parametrize("c", [-1, 41, 128])
def test_ceps(lib, c):
    refused(lib, mfcc(lib, C=c), "feat_mfcc", "C = %d outside [0, M = 40]" % c)


@pytest.mark.parametrize("nnz", [0, -5, 8193, 1 << 30])
def test_weights(lib, nnz):
    refused(lib, mfcc(lib, nnz=nnz), "feat_mfcc", "nnz = %d outside [1, 8192]" % nnz)


def test_lds_need(lib):
    """the need include/rsrgan.h states: 8 (H + nz H) + 4 (2 N + (F - 1) S) + 4 (nz H + nz M + M C + 3 M + nnz) bytes, refused above 65536
    with the count in the message"""
    F = lib.rsrgan_feat_wave_frames(2048)
    nz, H, N, S, M, C, nnz = min(4, F), 1024, 2048, 700, 128, 40, 1918
    need = 8 * (H + nz * H) + 4 * (2 * N + (F - 1) * S) + 4 * (nz * H + nz * M + M * C + 3 * M + nnz)
    assert need > 65536
    refused(lib, mfcc(lib, N=N, S=S, P=2048, M=M, C=C, nnz=nnz), "feat_mfcc", "%d bytes of LDS" % need, "above the entry's 65536")
    refused(lib, mfcc(lib, N=1024, S=1024, P=1024, M=128, C=128, nnz=8192), "feat_mfcc", "bytes of LDS")


def test_limit(lib):
    """the limit include/rsrgan.h states: at most 2^40 output floats, the width being C, or M with C = 0"""
    refused(lib, mfcc(lib, out_rows=(1 << 40) // 40 + 1), "feat_mfcc", "out_rows x width", "above the entry's 2^40")
    refused(lib, mfcc(lib, out_rows=(1 << 40) // 13 + 1, C=13), "feat_mfcc", "above the entry's 2^40")
    refused(lib, mfcc(lib, out_rows=(1 << 40) // 40 + 1, C=0, dct=None), "feat_mfcc", "above the entry's 2^40")
    refused(lib, mfcc(lib, out_rows=(1 << 62)), "feat_mfcc", "above the entry's 2^40")
