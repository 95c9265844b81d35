"""Parity at BASELINE.json's full sizes (configs[1]: B=32,T=50; configs[2] per GPU: B=64,T=100; reference-true networks):
the HIP path against the fp64 oracle (losses, every gradient tensor, enhanced-MFCC L1; tolerance 1e-3 relative as the
north_star states), plus oracle-free properties of the domain at the same size: the tower mean (the N-rank result equals
the 1-rank result on the concatenated batch), schedule equivalence, frames beyond `lengths`."""
import numpy as np
import pytest

from oracle import rsrgan_oracle as O
from tests.helpers import NET_D, NET_G, build_hip_pair, rand_batch, rel_err, split_flat

pytestmark = pytest.mark.gpu
RTOL = 1e-3           # BASELINE.json north_star: <= 1e-3 relative on losses and enhanced-MFCC L1


def _grads(model, net):
    return split_flat(model.engine.get_grads(net).cpu().numpy(), model.engine.tensor_table(net))


def _step_against_oracle(cfg, B, T, flags, seed):
    model, oracle = build_hip_pair(cfg, B, T, seed=seed, flags=flags)
    x, lab, ln = rand_batch(cfg, B, T, seed=seed + 100, ragged=True)
    x64, lab64 = x.astype(np.float64), lab.astype(np.float64)
    for _ in range(2 if flags & 2 else 0):
        model.engine.d_backward(x, lab, ln, None, None, train=True, apply=False)
        model.engine.g_backward(x, lab, ln, None, train=True, reuse=True, apply=False)
    got = model.engine.d_backward(x, lab, ln, None, None, train=True, apply=False).cpu().numpy()
    want, wg = oracle.d_tower(x64, lab64, ln)
    assert np.allclose(got, want, rtol=RTOL), (got, want)
    gd = _grads(model, NET_D)
    for k in wg:
        assert rel_err(gd[k], wg[k]) < 2e-3, ("D", k, rel_err(gd[k], wg[k]))
    got = model.engine.g_backward(x, lab, ln, None, train=True, reuse=True, apply=False).cpu().numpy()
    want, wg, y_ref = oracle.g_tower(x64, lab64, ln)
    assert np.allclose(got, want, rtol=RTOL), (got, want)
    gg = _grads(model, NET_G)
    for k in wg:
        assert rel_err(gg[k], wg[k]) < 2e-3, ("G", k, rel_err(gg[k], wg[k]))
    y = model.forward(x, ln)
    assert np.abs(y - y_ref).mean() / np.abs(y_ref).mean() < RTOL          # enhanced-MFCC L1
    # one full iteration (1 D + 1 G update), then the losses of the updated networks
    a = model.d_step(x, lab, ln); b = oracle.d_step(x64, lab64, ln)
    assert np.allclose(np.ravel(a), np.ravel(b), rtol=RTOL)
    a = model.g_step(x, lab, ln, reuse_g_forward=True); b = oracle.g_step(x64, lab64, ln)
    assert np.allclose(np.ravel(a), np.ravel(b), rtol=RTOL)
    a = model.g_step(x, lab, ln, train=False); b = oracle.g_step(x64, lab64, ln, train=False)
    assert np.allclose(np.ravel(a), np.ravel(b), rtol=RTOL), (a, b)
    assert model.engine.device_status() == 0


@pytest.mark.parametrize("flags", [1, 3])
@pytest.mark.parametrize("B,T", [(32, 50), (64, 100)])
def test_full_size_step_against_oracle(B, T, flags):
    """flags=3 is what bench.py times: the wavefront schedule replayed as hipGraphs.  A segment runs eagerly on its first use,
    is captured on its second and replayed from the third on, so the graph case repeats each backward three times (the
    gradients do not depend on the repetition: apply=False) and compares what the REPLAY produced.  At these sizes the generator's
    forward recurrence is the persistent launch of csrc/gpersist.hip (B % 32 == 0) and both discriminator-only recurrences are
    the persistent launches of csrc/dpersist.hip."""
    _step_against_oracle(O.NetCfg(), B, T, flags, seed=100 + B)


OTHER_NETS = {
    # the network the shipped run_gan_rnn_placeholder.sh:124,149 selects: 4 x LSTMP(760, p257) with the running residual sum
    # (models/res_lstm_l.py:101-194); at B = 64 its four layers and P = 257 take other XCD-group / split-K plans than at B = 4
    "res_lstm_l": lambda: O.NetCfg.res_lstm_l(),
    # BASELINE.json configs[1] as worded: 2-layer 512-unit LSTM generator (num_proj=None) + DNN discriminator (4 x 1024)
    "baseline_named": lambda: O.NetCfg(g_type="lstm", g_layers=2, g_cells=512, g_proj=0, d_type="dnn", d_layers=4, d_cells=1024),
}


@pytest.mark.parametrize("flags", [1, 3])
@pytest.mark.parametrize("net,B,T", [("res_lstm_l", 64, 100), ("res_lstm_l", 32, 50), ("baseline_named", 32, 50)])
def test_full_size_other_networks_against_oracle(net, B, T, flags):
    _step_against_oracle(OTHER_NETS[net](), B, T, flags, seed=300 + B)


def test_full_size_tower_mean_property():
    """average_gradients: losses and gradients of the [64]-row batch are the means of those of its two [32]-row halves."""
    cfg = O.NetCfg()
    B, T = 64, 100
    full, _ = build_hip_pair(cfg, B, T, seed=7, flags=1)
    half, _ = build_hip_pair(cfg, B // 2, T, seed=7, flags=1)          # same seed -> identical variables
    x, lab, ln = rand_batch(cfg, B, T, seed=8, ragged=True)
    lf = full.engine.d_backward(x, lab, ln, None, None, train=True, apply=False).cpu().numpy()
    gf = _grads(full, NET_D)
    lg = full.engine.g_backward(x, lab, ln, None, train=True, reuse=True, apply=False).cpu().numpy()
    gg = _grads(full, NET_G)
    acc_l, acc_lg, acc_d, acc_g = 0.0, 0.0, None, None
    for s in (slice(0, B // 2), slice(B // 2, B)):
        l = half.engine.d_backward(x[s], lab[s], ln[s], None, None, train=True, apply=False).cpu().numpy()
        gd = _grads(half, NET_D)
        l2 = half.engine.g_backward(x[s], lab[s], ln[s], None, train=True, reuse=True, apply=False).cpu().numpy()
        g2 = _grads(half, NET_G)
        acc_l = acc_l + 0.5 * l; acc_lg = acc_lg + 0.5 * l2
        acc_d = {k: 0.5 * v for k, v in gd.items()} if acc_d is None else {k: acc_d[k] + 0.5 * gd[k] for k in gd}
        acc_g = {k: 0.5 * v for k, v in g2.items()} if acc_g is None else {k: acc_g[k] + 0.5 * g2[k] for k in g2}
    assert np.allclose(lf, acc_l, rtol=1e-5) and np.allclose(lg, acc_lg, rtol=1e-5)
    for k in gf:
        assert rel_err(gf[k], acc_d[k]) < 1e-4, k
    for k in gg:
        assert rel_err(gg[k], acc_g[k]) < 1e-4, k


def test_full_size_schedules_agree_and_padding_is_inert():
    cfg = O.NetCfg()
    B, T = 64, 100
    a, _ = build_hip_pair(cfg, B, T, seed=9, flags=1)
    b, _ = build_hip_pair(cfg, B, T, seed=9, flags=0)
    x, lab, ln = rand_batch(cfg, B, T, seed=10, ragged=True)
    for m in (a, b):
        m.engine.d_backward(x, lab, ln, None, None, train=True, apply=False)
    for k, v in _grads(a, NET_D).items():
        assert rel_err(v, _grads(b, NET_D)[k]) < 1e-5, k
    la = a.engine.g_backward(x, lab, ln, None, train=True, reuse=True, apply=False).cpu().numpy()
    lb = b.engine.g_backward(x, lab, ln, None, train=True, reuse=True, apply=False).cpu().numpy()
    assert np.allclose(la, lb, rtol=1e-6)
    gb = _grads(b, NET_G)
    for k, v in _grads(a, NET_G).items():
        assert rel_err(v, gb[k]) < 1e-5, k
    # frames at t >= length: G(x) = output-FC bias there, and garbage in the padded input frames changes nothing
    y = a.forward(x, ln)
    gv, _ = a.get_vars()
    bias = gv["g_model/fully_connected_1/biases"]
    x2 = x.copy()
    for i in range(B):
        assert np.allclose(y[i, ln[i]:], bias[None, :], atol=1e-6)
        x2[i, ln[i]:] = 1e3
    y2 = a.forward(x2, ln)
    assert np.array_equal(y, y2)
    l2 = a.engine.g_backward(x2, lab, ln, None, train=True, reuse=False, apply=False).cpu().numpy()
    assert np.allclose(la, l2, rtol=1e-6)


# ---- the configuration bench.py TIMES, against the fp64 oracle (round 6) ---------------------------------------------------------
# bench.py enqueues steps without a host wait on one stream, device-resident batches, hipGraph replay (flags = 3), and gives the
# library the guarantee RSRGAN_DPIPE=1 asks for (D(real) of the next D-run on the side stream beside the previous G-run's
# weight-gradient GEMMs, the D-run itself = k_glstm_fwd_dt with D(G(x)) trailing over rows [B, 2B)); the ring hand-offs of the
# persistent generator launches carry a pass-parity tag in the lowest mantissa bit of every partial sum (RSRGAN_GP_TAGS=1: a 22-bit
# mantissa on those partials).  Each case below runs in a process of its own (the switches are read once per process) and compares
# with the oracle -- NOT with another configuration of the library: losses 1e-3, every gradient tensor 2e-3, enhanced-MFCC L1 1e-3
# (gan_rnn_placeholder.py:207-213,244-260; train_gan_rnn_placeholder.py:72-101).  The ACHIEVED errors are written to
# gpurun_out/parity_margin/<case>.json; tools/mk_parity_margin.py folds them into profiles/r6_parity_margin.json, which bench.py
# quotes in its JSON line ("parity_margin").
import hashlib
import json
import os
import subprocess
import sys
import tempfile

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_AS_BENCHED = r"""
import json, os, sys, hashlib
import numpy as np, torch
sys.path.insert(0, %r)
from oracle import rsrgan_oracle as O
from tests.helpers import NET_D, NET_G, build_hip_pair, rand_batch, rel_err, split_flat
net, B, T, seed = os.environ["RSRGAN_TEST_NET"], int(os.environ["RSRGAN_TEST_B"]), int(os.environ["RSRGAN_TEST_T"]), int(os.environ["RSRGAN_TEST_SEED"])
cfg = O.NetCfg.res_lstm_l() if net == "res_lstm_l" else O.NetCfg()
model, oracle = build_hip_pair(cfg, B, T, seed=seed, flags=3)
host = [rand_batch(cfg, B, T, seed=seed + 100 + i, ragged=True) for i in range(3)]
dev = [tuple(torch.from_numpy(v).cuda() for v in b) for b in host]
torch.cuda.synchronize()
eng = model.engine
grads = lambda n: split_flat(eng.get_grads(n).cpu().numpy(), eng.tensor_table(n))

# the oracle's side of the case depends on (net, B, T, seed) only: computed once, shared by the DPIPE / tag variants of the case
cache = os.environ["RSRGAN_TEST_ORACLE_CACHE"]
if os.path.exists(cache):
    want = dict(np.load(cache))
else:
    want = {}
    for i, (x, lab, ln) in enumerate(host):
        if i != 2: continue          # (gradients and losses at the injected variables: the LAST batch of the turn -- what a mixed-up or stale batch would break; all three batches are compared after the updates below)
        x64, lab64 = x.astype(np.float64), lab.astype(np.float64)
        l, gd = oracle.d_tower(x64, lab64, ln)
        want["p1_d%%d" %% i] = np.asarray(l, np.float64)
        l2, gg, y = oracle.g_tower(x64, lab64, ln)
        want["p1_g%%d" %% i] = np.asarray(l2, np.float64)
        for k, v in gd.items(): want["gd/" + k] = v
        for k, v in gg.items(): want["gg/" + k] = v
        want["y"] = y
    for i, (x, lab, ln) in enumerate(host):        # three full iterations (1 D + 1 G update each), one per batch
        x64, lab64 = x.astype(np.float64), lab.astype(np.float64)
        want["p2_d%%d" %% i] = np.ravel(np.asarray(oracle.d_step(x64, lab64, ln), np.float64))
        want["p2_g%%d" %% i] = np.ravel(np.asarray(oracle.g_step(x64, lab64, ln), np.float64))
    x, lab, ln = host[0]
    want["p2_eval"] = np.ravel(np.asarray(oracle.g_step(x.astype(np.float64), lab.astype(np.float64), ln, train=False), np.float64))
    tmp = cache + ".%%d.tmp.npz" %% os.getpid()
    np.savez(tmp, **want); os.replace(tmp, cache)

got = {}
# phase 1: gradients at the injected variables.  D-run + G-run of the three batches in turn, nine pairs enqueued WITHOUT a host wait
# (a segment runs eagerly on its first use, is captured on its second, replayed from the third on); nothing is applied
outs = []
with eng.on_stream():
    for it in range(9):
        x, lab, ln = dev[it %% 3]
        d = eng.d_backward(x, lab, ln, None, None, train=True, apply=False)
        g = eng.g_backward(x, lab, ln, None, train=True, reuse=True, apply=False)
        outs.append((d, g))
torch.cuda.synchronize()
for i in (2,):
    got["p1_d%%d" %% i] = outs[6 + i][0].cpu().numpy().astype(np.float64)
    got["p1_g%%d" %% i] = outs[6 + i][1].cpu().numpy().astype(np.float64)
gd, gg = grads(NET_D), grads(NET_G)           # of the last pair: batch 2
y = model.forward(host[2][0], host[2][2])
# phase 2: three full iterations as train_one_iteration / bench.py issue them (updates inside rsrgan_d_step / rsrgan_g_step)
outs = []
with eng.on_stream():
    for i in range(3):
        x, lab, ln = dev[i]
        d = model.d_step(x, lab, ln, sync=False, gather=False)
        g = model.g_step(x, lab, ln, reuse_g_forward=True, sync=False, gather=False)
        outs.append((d, g))
torch.cuda.synchronize()
for i in range(3):
    got["p2_d%%d" %% i] = np.ravel(outs[i][0].cpu().numpy()).astype(np.float64)
    got["p2_g%%d" %% i] = np.ravel(outs[i][1].cpu().numpy()).astype(np.float64)
got["p2_eval"] = np.ravel(np.asarray(model.g_step(host[0][0], host[0][1], host[0][2], train=False), np.float64))

relmax = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-30)))
res = {"loss": 0.0, "loss_after_updates": 0.0, "grad_d": 0.0, "grad_g": 0.0, "worst": {}}
for k in got:
    # (g_l2 is exactly 0 with l2_scale = 0 on both sides: skipped by the mask)
    m = np.abs(want[k]) > 0
    e = relmax(got[k][m], want[k][m])
    key = "loss" if k.startswith("p1_") else "loss_after_updates"
    if e > res[key]:
        res[key] = e; res["worst"][key] = k
for k, v in gd.items():
    e = rel_err(v, want["gd/" + k])
    if e > res["grad_d"]: res["grad_d"] = e; res["worst"]["grad_d"] = k
for k, v in gg.items():
    e = rel_err(v, want["gg/" + k])
    if e > res["grad_g"]: res["grad_g"] = e; res["worst"]["grad_g"] = k
res["mfcc_l1"] = float(np.abs(y - want["y"]).mean() / np.abs(want["y"]).mean())
res["device_status"] = int(eng.device_status())
eng.profile_begin()
x, lab, ln = dev[0]
with eng.on_stream():
    eng.d_backward(x, lab, ln, None, None, train=True, apply=False)
res["standalone_g_forward_launches"] = int(eng.profile_read_kind(1)[0])      # 0 under RSRGAN_DPIPE=1: the D-run is k_glstm_fwd_dt
eng.profile_read()
res["case"] = {"net": net, "B": B, "T": T, "RSRGAN_DPIPE": os.environ.get("RSRGAN_DPIPE", "0"), "RSRGAN_GP_TAGS": os.environ.get("RSRGAN_GP_TAGS", "1"),
               "flags": 3, "lengths": "ragged", "batches": 3, "enqueued_without_host_wait": True}
print("RESULT " + json.dumps(res))
""" % _ROOT


def _oracle_cache_key(net, B, T, seed):
    """the cached oracle results are those of this oracle: keyed on its source (and the helpers that feed it), the case and the seed"""
    h = hashlib.sha256()
    for rel in ("oracle/rsrgan_oracle.py", "tests/helpers.py"):
        with open(os.path.join(_ROOT, rel), "rb") as f:
            h.update(f.read())
    h.update(("%s %d %d %d" % (net, B, T, seed)).encode())
    return h.hexdigest()[:24]


def _as_benched(net, B, T, dpipe, tags):
    seed = 500 + B
    cache = os.path.join(tempfile.gettempdir(), "rsrgan_oracle_asbenched_%s_%d_%d_%s.npz" % (net, B, T, _oracle_cache_key(net, B, T, seed)))
    env = dict(os.environ, RSRGAN_TEST_NET=net, RSRGAN_TEST_B=str(B), RSRGAN_TEST_T=str(T), RSRGAN_TEST_SEED=str(seed),
               RSRGAN_DPIPE=str(dpipe), RSRGAN_GP_TAGS=str(tags), RSRGAN_TEST_ORACLE_CACHE=cache)
    p = subprocess.run([sys.executable, "-c", _AS_BENCHED], capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    out = os.path.join(_ROOT, "gpurun_out", "parity_margin")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "%s_B%d_T%d_dpipe%d_tags%d.json" % (net, B, T, dpipe, tags)), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    return res


@pytest.mark.parametrize("tags", [1, 0])
@pytest.mark.parametrize("dpipe", [1, 0])
@pytest.mark.parametrize("net,B,T", [("lstm", 64, 100), ("lstm", 32, 50), ("res_lstm_l", 32, 50)])
def test_full_size_step_as_benched_against_oracle(net, B, T, dpipe, tags):
    """What bench.py times (RSRGAN_DPIPE=1, tagged ring hand-offs, graph replay, steps enqueued without a host wait over three
    ragged batches in turn) and its three neighbours (DPIPE off, tags off) against the fp64 oracle."""
    if tags == 0 and (net, B) != ("lstm", 64):
        pytest.skip("the untagged hand-offs are compared at the headline size only")
    r = _as_benched(net, B, T, dpipe, tags)
    assert r["device_status"] == 0
    assert r["standalone_g_forward_launches"] == (0 if dpipe else 1), r      # proves which D-run ran
    assert r["loss"] < RTOL and r["loss_after_updates"] < RTOL, r
    assert r["grad_d"] < 2e-3 and r["grad_g"] < 2e-3, r
    assert r["mfcc_l1"] < RTOL, r


def test_shipped_recipe_host_fed_iteration_against_oracle():
    """The loop a user runs at the recipe the reference ships (run_gan_rnn_placeholder.sh:124,126,129-130: res_lstm_l, batch_size 8, 1 D-run +
    2 G-runs per batch; scripts/train_gan_rnn_placeholder.py:48-133): train_one_iteration over HOST batches of different padded lengths,
    ragged rows, through io.prefetch -- labels / lengths through upload_ready (the Python layer's RSRGAN_DPIPE=1 default), the inputs on
    the upload stream in stream order, the second G-run recomputing the generator's forward (k_glstm_fwd_dt) -- against the oracle's
    train_one_iteration on the same batches: the 7 averages within 1e-3, the updated variables of both nets after 5 x (1 + 2) updates."""
    from rsrgan_amd import train_one_iteration
    from rsrgan_amd.io import prefetch
    cfg = O.NetCfg.res_lstm_l()
    B = 8
    model, oracle = build_hip_pair(cfg, B, 100, seed=810, flags=3, disc_updates=1, gen_updates=2)
    batches = [rand_batch(cfg, B, T, seed=820 + i, ragged=True) for i, T in enumerate((60, 50, 60, 60, 40))]      # (T = 60: eager, captured, replayed)
    batches.insert(2, rand_batch(cfg, 5, 60, seed=830))          # a partial window: skipped (train...py:69-70)
    got = train_one_iteration(None, model, len(batches), 0, prefetch([[None, x, lab, ln] for x, lab, ln in batches], capacity=4))
    want = O.train_one_iteration(oracle, [(x.astype(np.float64), lab.astype(np.float64), ln) for x, lab, ln in batches], 1, 2)
    assert np.allclose(got, want, rtol=RTOL), (got, want)
    gv, dv = model.get_vars()
    for k, v in oracle.g.items():
        assert rel_err(gv[k], v) < 1e-4, ("G", k, rel_err(gv[k], v))
    for k, v in oracle.d.items():
        assert rel_err(dv[k], v) < 1e-4, ("D", k, rel_err(dv[k], v))
    assert model.engine.device_status() == 0
