"""rsrgan_wave_reverb (csrc/reverb.hip) refuses every argument error before its first HIP call, as rsrgan_feat_mfcc does
(tests/test_mfcc_op_args.py), naming the argument in rsrgan_last_error(); and the figures of rsrgan_wave_reverb_work.  The pointers are
made-up addresses: a refused call never reads them, and no device is needed."""
import pytest

from rsrgan_amd import _lib
from tests.test_op_args import P, refused

NAMES = ["pcm", "seg", "rir", "rir_seg", "noise", "noise_seg", "noise_pow", "sel", "snr", "twiddle", "out", "out_seg", "gains", "work"]
PTRS = {k: P + 65536 * i for i, k in enumerate(NAMES)}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def rev(lib, **kw):
    a = dict(PTRS, kind=0, n_samples=16000, n_taps=800, n_noise=500, B=4, R=2, V=1, C=64, flags=3, out_samples=16000, work_bytes=1 << 20)
    a.update(kw)
    return lib.rsrgan_wave_reverb(a["pcm"], a["kind"], a["n_samples"], a["seg"], a["rir"], a["n_taps"], a["rir_seg"], a["noise"], a["n_noise"],
                                  a["noise_seg"], a["noise_pow"], a["sel"], a["snr"], a["B"], a["R"], a["V"], a["C"], a["twiddle"], a["flags"],
                                  a["out"], a["out_samples"], a["out_seg"], a["gains"], a["work"], a["work_bytes"], None)


def need(n, L, Le, C):
    """the slot include/rsrgan.h describes (csrc/reverb.hip rev_layout), written out again"""
    Bk = C // 2
    cd = lambda a: -(-a // Bk)
    NI, PH, PE = cd(n), cd(L), cd(Le)
    NO = cd(n + L - 1) if L > 0 else NI
    NOE = cd(n + Le - 1) if Le > 0 else 0
    spectra = 2 * ((NI + 2) // 2) + 2 * ((PH + 1) // 2) + 2 * ((PE + 1) // 2)
    floats = 4 + NI + 3 * NO + NOE
    return spectra * C * 8 + (floats + 3) // 4 * 16


def test_symbols_are_bound(lib):
    for s in ("rsrgan_wave_reverb", "rsrgan_wave_reverb_work"):
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert len(lib.rsrgan_wave_reverb.argtypes) == 26


@pytest.mark.parametrize("B,n,L,C", [(1, 1, 1, 64), (9, 227, 103, 64), (32, 80000, 8000, 512), (32, 80000, 8000, 1024), (64, 80000, 8000, 2048),
                                     (3, 16000, 0, 128)])
def test_work_figures(lib, B, n, L, C):
    assert lib.rsrgan_wave_reverb_work(B, n, L, C) == B * need(n, L, L, C)
    assert lib.rsrgan_wave_reverb_work(B, n, L, C) % 16 == 0


@pytest.mark.parametrize("B,n,L,C", [(0, 1, 1, 64), (65536, 1, 1, 64), (1, 0, 1, 64), (1, (1 << 28) + 1, 1, 64), (1, 1, -1, 64), (1, 1, (1 << 24) + 1, 64),
                                     (1, 1, 1, 32), (1, 1, 1, 96), (1, 1, 1, 4096)])
def test_work_refusals(lib, B, n, L, C):
    assert lib.rsrgan_wave_reverb_work(B, n, L, C) == 0


@pytest.mark.parametrize("which", ["pcm", "seg", "sel", "snr"])
def test_null_inputs(lib, which):
    refused(lib, rev(lib, **{which: None}), "wave_reverb", "null pointer (pcm, seg, sel or snr)")


@pytest.mark.parametrize("which", ["out", "out_seg"])
def test_null_outputs(lib, which):
    refused(lib, rev(lib, **{which: None}), "wave_reverb", "null pointer (out or out_seg)")


@pytest.mark.parametrize("which", ["twiddle", "work"])
def test_null_twiddle_or_work(lib, which):
    refused(lib, rev(lib, **{which: None}), "wave_reverb", "null pointer (twiddle or work)")


def test_banks_go_with_their_counts(lib):
    for which in ("rir", "rir_seg"):
        refused(lib, rev(lib, **{which: None}), "wave_reverb", "null pointer (rir or rir_seg)", "R = 2")
    for which in ("noise", "noise_seg", "noise_pow"):
        refused(lib, rev(lib, **{which: None}), "wave_reverb", "null pointer (noise, noise_seg or noise_pow)", "V = 1")
    refused(lib, rev(lib, n_taps=0), "wave_reverb", "n_taps = 0", "R = 2")
    refused(lib, rev(lib, n_noise=0), "wave_reverb", "n_noise = 0", "V = 1")
    refused(lib, rev(lib, n_taps=-1, R=0, rir=None, rir_seg=None), "wave_reverb", "n_taps = -1")


@pytest.mark.parametrize("b", [0, -1, 65536, 1 << 30])
def test_batch(lib, b):
    refused(lib, rev(lib, B=b), "wave_reverb", "B = %d outside [1, 65535]" % b)


@pytest.mark.parametrize("which", ["R", "V"])
def test_counts(lib, which):
    for v in (-1, (1 << 20) + 1):
        refused(lib, rev(lib, **{which: v}), "wave_reverb", "%s = %d outside [0, 2^20]" % (which, v))


@pytest.mark.parametrize("kind", [-1, 2, 7])
def test_unknown_kind(lib, kind):
    refused(lib, rev(lib, kind=kind), "wave_reverb", "kind = %d" % kind)


def test_alignment(lib):
    refused(lib, rev(lib, pcm=P + 1), "wave_reverb", "pcm not aligned to its 2-byte samples")
    for off in (1, 2, 3):
        refused(lib, rev(lib, kind=1, pcm=P + off), "wave_reverb", "pcm not aligned to its 4-byte samples")
    for off in (1, 2, 4, 8):
        refused(lib, rev(lib, work=PTRS["work"] + off), "wave_reverb", "work not 16-byte aligned")
    for which in ("seg", "rir_seg", "noise_seg", "out_seg"):
        for off in (1, 2, 4):
            refused(lib, rev(lib, **{which: PTRS[which] + off}), "wave_reverb", "seg, rir_seg, noise_seg or out_seg not 8-byte aligned")
    for which in ("rir", "noise", "noise_pow"):
        for off in (1, 2, 3):
            refused(lib, rev(lib, **{which: PTRS[which] + off}), "wave_reverb", "rir, noise or noise_pow not 4-byte aligned")
    for which in ("sel", "snr", "twiddle"):
        for off in (1, 2, 3):
            refused(lib, rev(lib, **{which: PTRS[which] + off}), "wave_reverb", "sel, snr or twiddle not 4-byte aligned")
    for which in ("out", "gains"):
        for off in (1, 2, 3):
            refused(lib, rev(lib, **{which: PTRS[which] + off}), "wave_reverb", "out or gains not 4-byte aligned")


@pytest.mark.parametrize("which", ["n_samples", "out_samples"])
def test_sizes(lib, which):
    for v in (0, -1):
        refused(lib, rev(lib, **{which: v}), "wave_reverb", "must be positive")
    refused(lib, rev(lib, **{which: (1 << 40) + 1}), "wave_reverb", "above the entry's 2^40")


@pytest.mark.parametrize("c", [0, 32, 63, 500, 1025, 4096, -64])
def test_fft_length(lib, c):
    refused(lib, rev(lib, C=c), "wave_reverb", "C = %d is no power of two in [64, 2048]" % c)


@pytest.mark.parametrize("f", [-1, 4, 7, 256])
def test_flags(lib, f):
    refused(lib, rev(lib, flags=f), "wave_reverb", "flags = %d" % f)


def test_work_too_small(lib):
    for B, C in ((4, 64), (32, 2048)):
        least = lib.rsrgan_wave_reverb_work(B, 1, 1, C)
        refused(lib, rev(lib, B=B, C=C, work_bytes=least - 1), "wave_reverb", "work_bytes = %d below the %d bytes" % (least - 1, least))
    refused(lib, rev(lib, work_bytes=0), "wave_reverb", "work_bytes = 0")
    refused(lib, rev(lib, work_bytes=-5), "wave_reverb", "work_bytes = -5")


def test_gains_may_be_null(lib):
    """gains = NULL is no error of its own: a call with it and an error elsewhere is refused for that error"""
    refused(lib, rev(lib, gains=None, C=3), "wave_reverb", "C = 3")
