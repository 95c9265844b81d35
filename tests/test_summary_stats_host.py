"""rsrgan_amd/summary.py: histogram_from_stats encodes a record (what csrc/hist.hip computes on the device, here built with NumPy) into
the bytes histogram() writes; model_summaries without the new arguments writes the parent's bytes, with them five histogram tags in the
reference's order.  No device."""
import numpy as np
import pytest

from rsrgan_amd import summary as S

L = S._LIMITS
F32 = np.float32


def _at_limits():
    """float32(limit) and its two float32 neighbours, for a handful of limits of both signs"""
    out = []
    for i in (5, 300, 700, len(L) // 2 - 1, len(L) // 2, len(L) // 2 + 1, 900, 1200, 1500):
        v = F32(L[i])
        out += [v, np.nextafter(v, F32(np.inf)), np.nextafter(v, F32(-np.inf))]
    return np.array(out, F32)


CASES = {
    "normal": np.random.default_rng(0).standard_normal(1000).astype(F32),
    "zeros": np.zeros(33, F32),
    "one": np.array([3.25], F32),
    "empty": np.zeros(0, F32),
    "limits": _at_limits(),
    "inf": np.array([np.inf, -np.inf, 1.0], F32),
}


def numpy_record(values):
    """the record, written out again here (not summary.histogram_stats): [min, max, num, sum, sum_squares, counts]"""
    x = np.asarray(values, np.float64).ravel()
    if x.size == 0:
        x = np.zeros(1)
    counts = np.zeros(len(L))
    for v in x:
        k = 0
        while k < len(L) - 1 and not v < L[k]:               # the first limit greater than v, clamped to the last bucket
            k += 1
        counts[k] += 1
    with np.errstate(invalid="ignore"):
        return np.concatenate([[x.min(), x.max(), x.size, x.sum(), np.square(x).sum()], counts])


@pytest.mark.parametrize("name", sorted(CASES))
def test_histogram_from_stats_writes_histogram_s_bytes(name):
    v = CASES[name]
    with np.errstate(invalid="ignore"):
        want = S.histogram("tag/" + name, v)
    rec = numpy_record(v)
    assert rec.shape == (S.STATS_HEAD + len(L),) and rec[S.STATS_HEAD:].sum() == max(v.size, 1)
    assert S.histogram_from_stats("tag/" + name, rec) == want
    with np.errstate(invalid="ignore"):
        got = S.histogram_stats(v)
    assert np.array_equal(got, rec, equal_nan=True)


def test_histogram_from_stats_refuses_a_record_of_another_length():
    with pytest.raises(ValueError):
        S.histogram_from_stats("t", np.zeros(len(L)))


# model_summaries([1 .. 7], inputs [[0.5, -1.0]], labels [2.0], g [0.0, 1e-13]) as the commit before the device route wrote it
PARENT = bytes.fromhex(
    "0a100a09645f726c5f6c6f7373150000803f0a100a09645f666b5f6c6f737315000000400a0d0a06645f6c6f737315000040400a110a0a675f6164765f6c6f7373"
    "15000080400a110a0a675f6d73655f6c6f7373150000a0400a100a09675f6c325f6c6f7373150000c0400a0d0a06675f6c6f7373150000e0400a90010a0a726561"
    "6c5f636c65616e2a810109000000000000f0bf11000000000000e03f19000000000000004021000000000000e0bf29000000000000f43f32282b14facdbe24f0bf"
    "08996919155aedbffae55a25d31fde3fb03125ee8091e03fffffffffffffef7f3a280000000000000000000000000000f03f0000000000000000000000000000f0"
    "3f00000000000000000a6f0a0a7265616c5f6e6f6973652a6109000000000000004011000000000000004019000000000000f03f21000000000000004029000000"
    "00000010403218dc94cd2e8d75ff3fe011f10c744d0140ffffffffffffef7f3a180000000000000000000000000000f03f00000000000000000a6c0a07675f636c"
    "65616e2a610900000000000000001100000060c2253c3d1900000000000000402100000060c2253c3d2920ad1ab640c2883a3218000000000000000011ea2d8199"
    "97713dffffffffffffef7f3a18000000000000000000000000000000400000000000000000")

SMALL = (np.array([[0.5, -1.0]], F32), np.array([2.0], F32), np.array([0.0, 1e-13], F32))


def test_model_summaries_without_the_new_arguments_is_the_parent_s():
    assert len(PARENT) == 492
    assert S.model_summaries([1, 2, 3, 4, 5, 6, 7], *SMALL) == PARENT


def test_model_summaries_with_logits_writes_five_tags_in_the_reference_s_order(tmp_path):
    d_real, d_fake = np.array([[0.9, 1.1], [1.0, 0.7]], F32), np.array([[0.1, -0.2], [0.0, 0.3]], F32)
    blob = S.model_summaries([1, 2, 3, 4, 5, 6, 7], *SMALL, d_real=d_real, d_fake=d_fake)
    # the scalars, then d_real, d_fake, then the parent's three (gan_rnn_placeholder.py:285-296)
    scalars = S.merge(S.scalar(t, v) for t, v in zip(S.LOSS_TAGS, [1, 2, 3, 4, 5, 6, 7]))
    assert blob == scalars + S.histogram("d_real", d_real) + S.histogram("d_fake", d_fake) + PARENT[len(scalars):]
    # the records in place of the tensors: the same bytes
    stats = {t: S.histogram_stats(a) for t, a in zip(S.HIST_TAGS, (d_real, d_fake) + SMALL)}
    assert S.model_summaries([1, 2, 3, 4, 5, 6, 7], stats=stats) == blob
    w = S.FileWriter(str(tmp_path))
    w.add_summary(blob, 3); w.close()
    ev = S.read_events(w.path)[1]
    assert ev[1] == 3 and list(ev[2]) == list(S.LOSS_TAGS) + list(S.HIST_TAGS)
    assert ev[2]["d_real"]["num"] == 4 and ev[2]["d_real"]["max"] == float(F32(1.1)) and ev[2]["d_fake"]["min"] == float(F32(-0.2))
    assert ev[2]["d_fake"]["bucket"].sum() == 4 and ev[2]["g_clean"]["num"] == 2
