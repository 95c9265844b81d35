"""k_hist / k_hist_finish (csrc/hist.hip) through rsrgan_hist against tests/hist_ref.py: min, max, num and every bucket count exactly, sum
and sum_squares within n * 2^-52 * sum |term| of math.fsum (derived in hist_ref.record, not measured).  The sizes are the smallest at
which the kernel takes another path: below, at and above a wave; the 16-byte path with and without a tail; a view with a leading
dimension; several workgroups per tensor (more than 8192 elements) and the one-bucket wave aggregation."""
import numpy as np
import pytest
import torch

from tests import hist_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
FMAX = np.finfo(F32).max
DENORM = np.nextafter(F32(0), F32(1))


@pytest.fixture(scope="module")
def ops():
    from rsrgan_amd.ops import OpEntries
    return OpEntries()


def run(ops, arrays):
    """records of host float32 arrays (each uploaded as it is shaped)"""
    ts = [torch.from_numpy(np.ascontiguousarray(a, F32)).to(ops.device) for a in arrays]
    out = ops.hist(ts)
    assert tuple(out.shape) == (len(arrays), 5 + R.NL) and out.dtype == torch.float64
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 257 * 7])
def test_element_counts(ops, n):
    v = (np.random.default_rng(n).standard_normal(n) * 3).astype(F32)
    R.check(run(ops, [v])[0], v)


def test_strided_view_does_not_read_the_other_columns(ops):
    """cols = 1, ld = 4: the discriminator's logits buffer, 4 x 7 x 2 rows; the other three columns hold NaN"""
    rows = 4 * 7 * 2
    buf = np.full((rows, 4), np.nan, F32)
    buf[:, 0] = np.random.default_rng(5).standard_normal(rows).astype(F32)
    t = torch.from_numpy(buf).to(ops.device)
    got = ops.hist([t[:, :1]]).cpu().numpy()[0]
    assert not np.isnan(got).any()
    R.check(got, buf[:, 0])
    # two columns of a padded leading dimension
    buf[:, 1] = 2.0
    t = torch.from_numpy(buf).to(ops.device)
    R.check(ops.hist([t[:, :2]]).cpu().numpy()[0], buf[:, :2])


def test_three_tensors_of_different_sizes_in_one_call(ops):
    rng = np.random.default_rng(9)
    vs = [rng.standard_normal((3, 5, 7)).astype(F32), (rng.standard_normal(20001) * 1e-3).astype(F32), np.array([[-2.5]], F32)]
    got = run(ops, vs)
    for g, v in zip(got, vs):
        R.check(g, v)


def test_empty_tensor_is_the_single_value_zero(ops):
    got = run(ops, [np.zeros((0, 3), F32), np.array([1.5], F32)])
    R.check(got[0], np.zeros(0, F32))
    assert got[0][2] == 1.0 and got[0][5:].sum() == 1.0
    R.check(got[1], [1.5])


def test_one_bucket(ops):
    """2^20 copies of 1.0: every lane of every wave hits one LDS counter"""
    n = 1 << 20
    got = ops.hist([torch.ones(n, dtype=torch.float32, device=ops.device)]).cpu().numpy()[0]
    k = int(np.searchsorted(R.S._LIMITS, 1.0, side="right"))
    assert got[5 + k] == float(n) and got[5:].sum() == float(n)
    assert list(got[:5]) == [1.0, 1.0, float(n), float(n), float(n)]


def _around_limits():
    L = R.S._LIMITS
    zero = len(L) // 2
    idx = [1, 90, 250, 400, 555, 700, 760, zero - 1, zero + 1, zero + 15, 800, 950, 1100, 1300, 1480, len(L) - 2]      # 16 limits, both signs
    out = []
    for i in idx + [zero]:
        v = F32(L[i])                                           # the float32 nearest the limit
        out += [v, np.nextafter(v, F32(np.inf)), np.nextafter(v, F32(-np.inf))]
    return np.array(out, F32)


def test_values_around_limits(ops):
    v = _around_limits()
    assert v.size == 51 and np.isfinite(v).all()
    R.check(run(ops, [v])[0], v)


def test_zeros_denormals_and_extremes(ops):
    v = np.array([0.0, -0.0, DENORM, -DENORM, 1e-13, -1e-13, FMAX, -FMAX], F32)
    got = run(ops, [v, np.array([np.inf, 1.0, -2.0], F32), np.array([-np.inf, 1.0, -2.0], F32), np.array([np.inf, -np.inf, 0.5], F32)])
    R.check(got[0], v)
    R.check(got[1], [np.inf, 1.0, -2.0]); R.check(got[2], [-np.inf, 1.0, -2.0]); R.check(got[3], [np.inf, -np.inf, 0.5])
    assert got[1][5 + R.NL - 1] == 1.0 and got[2][5] == 1.0                 # +inf: the last bucket, -inf: the first
    assert got[3][5] == 1.0 and got[3][5 + R.NL - 1] == 1.0 and np.isnan(got[3][3]) and got[3][4] == np.inf


def test_one_nan_among_normals(ops):
    v = np.random.default_rng(11).standard_normal(300).astype(F32)
    v[123] = np.nan
    got = run(ops, [v])[0]
    assert np.isnan(got[[0, 1, 3, 4]]).all() and got[2] == 300.0
    assert got[5 + R.NL - 1] == 1.0                                          # the NaN counts into the last bucket
    R.check(got, v)


def test_two_calls_return_the_same_bytes(ops):
    rng = np.random.default_rng(13)
    ts = [torch.from_numpy(rng.standard_normal(50000).astype(F32)).to(ops.device), torch.from_numpy(rng.standard_normal((64, 33)).astype(F32)).to(ops.device)]
    a = ops.hist(ts).cpu().numpy()
    b = ops.hist(ts).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    R.check(a[0], ts[0].cpu().numpy()); R.check(a[1], ts[1].cpu().numpy())
