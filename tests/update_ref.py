"""Shared by tests/test_gpu_update_ops.py and tests/test_gpu_loss_ops.py: the error metrics, the bound rule and the run-twice harness.

Bound rule (tests/test_gpu_wgrad_ops.py's, for column sums): a kernel's error may be 4 x the error of the same quantity evaluated in
fp32 on the CPU in plain order with the same formula, both measured against fp64 in the same metric; the factor covers summation order
and FMA contraction only.  Where the CPU's fp32 error falls below 2 ulp of the result (2^-22 relative: the final rounding and one
division), the bound is 2 ulp."""
import numpy as np
import torch

f32, f64 = np.float32, np.float64
SENT = 7.0
ULP2 = 2.0 ** -22                      # 2 ulp of a result, relative: one fp32 ulp is at most 2^-23 of the value


def rng(*seed):
    return np.random.default_rng(list(seed))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def elem_err(got, ref):
    """per-element outputs, a list of tensors: the worst tensor's max |got - ref| / max(|ref|, scale 2^-20), scale = that tensor's max |ref|
    (an all-zero reference asks for exact zeros)"""
    worst = 0.0
    for g, r in zip(got, ref):
        scale = np.abs(r).max()
        if scale == 0.0:
            worst = max(worst, 0.0 if not np.any(g) else float("inf"))
            continue
        worst = max(worst, float((np.abs(np.asarray(g).astype(f64) - r) / np.maximum(np.abs(r), scale * 2.0 ** -20)).max()))
    return worst


def rel_err(got, ref):
    """sums and scalars: max |got - ref| / |ref| (a reference of 0 asks for 0)"""
    got, ref = np.asarray(got, dtype=f64).ravel(), np.asarray(ref, dtype=f64).ravel()
    z = ref == 0.0
    assert not np.any(got[z]), "a quantity whose reference is 0 is not 0"
    return float((np.abs(got[~z] - ref[~z]) / np.abs(ref[~z])).max()) if np.any(~z) else 0.0


def bounded(prefix, case, name, k, p):
    bound = max(4.0 * p, ULP2)
    print("%s %-40s %-8s k=%.2e p=%.2e bound=%.2e" % (prefix, case, name, k, p, bound))
    assert k <= bound, (case, name, k, p, bound)


def dev(a, eng):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def twice(run):
    """run() -> dict of arrays, each time from fresh buffers: both runs bit-identical (the kernels promise a fixed summation order)"""
    a, b = run(), run()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "two runs differ in %s" % k
    return a


def seqsum32(x):
    """fp32 accumulation in plain order"""
    x = np.ascontiguousarray(x, dtype=f32).ravel()
    return np.cumsum(x, dtype=f32)[-1] if x.size else f32(0.0)
