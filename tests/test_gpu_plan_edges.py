"""The recurrences are planned per handle (and some per call) from the shapes and from what the device can hold: one persistent launch,
one per row group, the 8- or 16-cell unprojected form, the launch-per-phase path beyond GP_TMAX, the discriminator's persistent launches
with or without the weight gradients inside, the one-lane form of a padded batch.  Each case here runs one of those plans against the
fp64 oracle (losses 1e-3, every gradient tensor 2e-3, enhanced-MFCC L1 1e-3, ragged lengths with a row of length 1, non-zero biases)
and asserts through the launch counters (rsrgan_profile_read_kind) which plan ran -- oracle first, path second, so a path failure
says the numbers were right."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import rsrgan_oracle as O
from tests.helpers import NET_D, NET_G, args_for, build_hip_pair, rand_batch, rand_params, rel_err, split_flat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-3
GP_TMAX = 2046                        # csrc/kernels.h: the longest persistent generator launch

# kinds of rsrgan_profile_read_kind (include/rsrgan.h)
K_GFWD, K_GBWD, K_GFWD_DT, K_DFWD, K_DBWD, K_DBWD_DW, K_NPFWD, K_NPBWD = 1, 2, 3, 4, 5, 6, 7, 8


def narrow_g(**kw):
    """2 x LSTMP(64, p32): still planned as one persistent generator launch (gpersist_plan), cheap for the oracle at T = 2047"""
    c = O.NetCfg(g_layers=2, g_cells=64, g_proj=32)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def batch(cfg, B, T, seed):
    x, lab, ln = rand_batch(cfg, B, T, seed=seed, ragged=True)
    if B > 1:
        ln[-1] = 1
    return x, lab, ln


def make_oracle(cfg, B, seed):
    """the oracle build_hip_pair pairs with a model of these variables (default arguments), without a model"""
    g, d = rand_params(cfg, seed)
    a = args_for(cfg, B)
    return O.GanRnnOracle(cfg, g, d, batch_size=B, l2_scale=a.l2_scale, g_learning_rate=float(np.float32(a.g_learning_rate)),
                          d_learning_rate=float(np.float32(a.d_learning_rate)), mse_lambda=float(np.float32(a.init_mse_weight)))


def oracle_towers(oracle, x, lab, ln):
    x64, lab64 = x.astype(np.float64), lab.astype(np.float64)
    ld, gd = oracle.d_tower(x64, lab64, ln)
    lg, gg, y = oracle.g_tower(x64, lab64, ln)
    return dict(ld=np.asarray(ld), gd=gd, lg=np.asarray(lg), gg=gg, y=y)


def _grads(model, net):
    return split_flat(model.engine.get_grads(net).cpu().numpy(), model.engine.tensor_table(net))


def kinds_of(eng):
    k = {i: eng.profile_read_kind(i)[0] for i in range(1, 9)}
    eng.profile_read()
    return k


def run_against(model, want, x, lab, ln, reps=1):
    """One D-run and one G-run (reuse of the D-run's generator forward, nothing applied) per repetition, each against the oracle; the
    first inside a profile window.  reps > 1 (flags 3): the later ones run eagerly, are captured, then replayed.  Returns the kinds."""
    eng = model.engine
    kinds = None
    for r in range(reps):
        if r == 0:
            eng.profile_begin()
        ld = eng.d_backward(x, lab, ln, None, None, train=True, apply=False).cpu().numpy()
        gd = _grads(model, NET_D)
        lg = eng.g_backward(x, lab, ln, None, train=True, reuse=True, apply=False).cpu().numpy()
        gg = _grads(model, NET_G)
        if r == 0:
            kinds = kinds_of(eng)
        assert np.allclose(ld, want["ld"], rtol=RTOL), (r, ld, want["ld"])
        assert np.allclose(lg, want["lg"], rtol=RTOL), (r, lg, want["lg"])
        bad = {("D", k): rel_err(gd[k], v) for k, v in want["gd"].items() if not rel_err(gd[k], v) < 2e-3}
        bad.update({("G", k): rel_err(gg[k], v) for k, v in want["gg"].items() if not rel_err(gg[k], v) < 2e-3})
        assert not bad, (r, bad)
    y = model.forward(x, ln)
    assert np.abs(y - want["y"]).mean() / np.abs(want["y"]).mean() < RTOL          # enhanced-MFCC L1
    assert eng.device_status() == 0
    return kinds


# ---- A. BASELINE.json configs[2] as worded: 2 x 512 generator without projection + DNN discriminator, B = 64, T = 100 ----------------
# (bench.py --full times it as variants[0].)  The unprojected forward is k_glstm_np_fwd.  Its BPTT (k_glstm_np_bwd) produces no input
# gradient for layer 0, which the lstm generator's input FC needs: configs[2]'s BPTT is the launch path at every NT.  The unprojected
# BPTT serves a stack fed the input frames directly (res_lstm_base without projection), for 8 cells per workgroup only (NT = 2, 256
# workgroups at 64 rows: the whole MI355X, which the residency probe grants there); with 16 cells (NT = 4) it takes the launch path (B).

def baseline_named(g_type="lstm"):
    return O.NetCfg(g_type=g_type, g_layers=2, g_cells=512, g_proj=0, d_type="dnn", d_layers=4, d_cells=1024)


@functools.lru_cache(maxsize=None)
def _baseline_oracle(g_type, B, T, seed):
    return oracle_towers(make_oracle(baseline_named(g_type), B, seed), *batch(baseline_named(g_type), B, T, seed + 1))


def _np_case(B, T, flags, seed, want_np_bwd, g_type="lstm"):
    cfg = baseline_named(g_type)
    want = _baseline_oracle(g_type, B, T, seed)
    model, _ = build_hip_pair(cfg, B, T, seed=seed, flags=flags)
    k = run_against(model, want, *batch(cfg, B, T, seed + 1), reps=4 if flags & 2 else 1)
    assert k[K_NPFWD] >= 1 and k[K_NPBWD] == want_np_bwd, k
    assert k[K_GFWD] == k[K_GBWD] == k[K_GFWD_DT] == k[K_DFWD] == k[K_DBWD] == 0, k
    return k


@pytest.mark.parametrize("flags", [1, 3])
def test_baseline_named_configs2_against_oracle(flags):
    _np_case(64, 100, flags, 910, 0)


@pytest.mark.parametrize("flags", [1, 3])
def test_unprojected_bptt_launch_against_oracle(flags):
    import torch
    # 8 cells per workgroup needs 2 layers x 64 chunks x 2 row groups = 256 resident workgroups
    np_bwd = 1 if torch.cuda.get_device_properties(0).multi_processor_count >= 256 else 0
    _np_case(64, 100, flags, 915, np_bwd, g_type="res_lstm_base")


# ---- B. the 16-cell unprojected form (RSRGAN_GP_NP_NT=4, a process-scope row of csrc/switches.h: read once per process): forward persistent, BPTT on the launch path ---------

def np16_case():
    assert os.environ.get("RSRGAN_GP_NP_NT") == "4"
    _np_case(64, 20, 1, 920, 0, g_type="res_lstm_base")


def test_unprojected_16_cell_form_against_oracle():
    env = dict(os.environ, RSRGAN_GP_NP_NT="4")
    code = "import sys; sys.path.insert(0, %r); from tests.test_gpu_plan_edges import np16_case; np16_case(); print('NP16 OK')" % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "NP16 OK" in p.stdout, p.stderr[-3000:]


# ---- C. res_lstm_base (the stack of projected cells fed the input frames, no sums) on the persistent generator launches ---------------

def test_res_lstm_base_persistent_against_oracle():
    cfg = O.NetCfg.res_lstm_l(g_type="res_lstm_base")
    B, T = 32, 20
    model, oracle = build_hip_pair(cfg, B, T, seed=930, flags=3)
    x, lab, ln = batch(cfg, B, T, 931)
    k = run_against(model, oracle_towers(oracle, x, lab, ln), x, lab, ln, reps=4)
    assert k[K_GFWD] + k[K_GFWD_DT] >= 1 and k[K_GBWD] >= 1, k


def test_single_block_projection_bptt_takes_launch_path_against_oracle():
    """P = 16 (one 16-column block): the persistent BPTT's hand-offs time out at this width, so the handle plans its BPTT on the launch
    path and keeps the persistent forward"""
    cfg = narrow_g(g_proj=16)
    B, T = 32, 20
    model, oracle = build_hip_pair(cfg, B, T, seed=935, flags=3)
    x, lab, ln = batch(cfg, B, T, 936)
    k = run_against(model, oracle_towers(oracle, x, lab, ln), x, lab, ln, reps=4)
    assert k[K_GFWD] + k[K_GFWD_DT] >= 1 and k[K_GBWD] == 0, k


# ---- D. across GP_TMAX: T = 2047 takes the launch-per-phase generator path, T <= 2046 the persistent launch ---------------------------

def test_decode_across_gp_tmax_against_oracle():
    """decode's single utterance (B = 1, padded to one 32-row group) on one handle at T = 2046, 2047, 2046: prefixes of one input, so
    one oracle forward at 2047 checks all three (the recurrence is causal)"""
    cfg = O.NetCfg()
    model, oracle = build_hip_pair(cfg, 1, 2100, seed=940, flags=1)
    x, _, _ = rand_batch(cfg, 1, GP_TMAX + 1, seed=941)
    y_ref = oracle.forward(x.astype(np.float64), np.array([GP_TMAX + 1], np.int32))
    eng = model.engine
    for T, persistent in ((GP_TMAX, True), (GP_TMAX + 1, False), (GP_TMAX, True)):
        eng.profile_begin()
        y = model.forward(np.ascontiguousarray(x[:, :T]), np.array([T], np.int32))
        k = kinds_of(eng)
        want = y_ref[:, :T]
        l1 = np.abs(y - want).mean() / np.abs(want).mean()
        assert l1 < RTOL, (T, l1)
        assert k[K_GFWD] == (1 if persistent else 0), (T, k)
    assert eng.device_status() == 0


@pytest.mark.parametrize("B", [32, 8])
def test_training_beyond_gp_tmax_against_oracle(B):
    """T = 2047: the generator's recurrences on the launch path, the discriminator's still persistent (its rings are sized by Tmax)"""
    cfg = narrow_g()
    T = GP_TMAX + 1
    model, oracle = build_hip_pair(cfg, B, 2100, seed=950 + B, flags=1)
    x, lab, ln = batch(cfg, B, T, 951 + B)
    k = run_against(model, oracle_towers(oracle, x, lab, ln), x, lab, ln)
    assert k[K_GFWD] == k[K_GBWD] == k[K_GFWD_DT] == 0, k
    assert k[K_DFWD] >= 1 and k[K_DBWD] >= 1, k


# ---- E. a padded batch (B = 8: one 16-row tile of real rows in a 32-row group) after a forward-only pass beyond GP_TMAX ---------------
# The one-lane form of the persistent launches (GPersistArgs::nrt, DPersistArgs::nrt) never touches the padding tile, while the
# weight-gradient products and column sums read every row of the stash: anything a launch-path pass (T > GP_TMAX) left in the padding
# rows would be summed into the gradients of the next one-lane G-run.  Control: the same G-run without the long pass.

@functools.lru_cache(maxsize=None)
def _padded_oracle(seed):
    cfg = narrow_g()
    return oracle_towers(make_oracle(cfg, 8, seed), *batch(cfg, 8, 60, seed + 2))


@pytest.mark.parametrize("long_call", ["none", "eval", "forward"])
@pytest.mark.parametrize("flags", [1, 3])
def test_padded_one_lane_after_long_forward_against_oracle(flags, long_call):
    cfg = narrow_g()
    B, T = 8, 60
    model, _ = build_hip_pair(cfg, B, 2100, seed=960, flags=flags)
    xl, labl, lnl = batch(cfg, B, GP_TMAX + 1, 961)
    if long_call == "eval":            # the cross-validation twin's fetch (share_engine_from: the same handle)
        model.g_step(xl, labl, lnl, train=False)
    elif long_call == "forward":
        model.forward(xl, lnl)
    k = run_against(model, _padded_oracle(960), *batch(cfg, B, T, 962), reps=4 if flags & 2 else 1)
    assert k[K_GFWD] + k[K_GFWD_DT] >= 1 and k[K_GBWD] >= 1, k          # the one-lane persistent launches ran


# ---- F. the discriminator's shapes at the dpersist predicates (narrow generator, B = 32, T = 20) ------------------------------------
# persistent D: every layer I % 4 == 0, P <= 48, at most DP_MAXL = 3 layers; weight gradients inside k_dlstm_bwd: every layer I == I0,
# P == P0, I <= 48, P <= 47

D_SHAPES = {
    # name: (output_dim, d_proj, d_layers, persistent, dW inside the launch)
    "io44_p44": (44, 44, 2, True, True),
    "io48_p48": (48, 48, 2, True, False),             # P > 47
    "io40_p44": (40, 44, 2, True, False),             # layer 1's I = 44 != I0 = 40
    "one_layer_io40_p44": (40, 44, 1, True, True),
    "three_layers": (40, 40, 3, True, True),          # DP_MAXL
    "p52": (40, 52, 2, False, False),                 # P > 48: launch path
    "io42": (42, 40, 2, False, False),                # I % 4 != 0: launch path; the G-run's y_tm hand-off with padding columns
}


@pytest.mark.parametrize("shape", list(D_SHAPES))
def test_discriminator_shapes_against_oracle(shape):
    out, proj, layers, persistent, dw = D_SHAPES[shape]
    cfg = narrow_g(output_dim=out, d_proj=proj, d_layers=layers)
    B, T = 32, 20
    model, oracle = build_hip_pair(cfg, B, T, seed=970, flags=3)
    x, lab, ln = batch(cfg, B, T, 971)
    k = run_against(model, oracle_towers(oracle, x, lab, ln), x, lab, ln, reps=4)
    if persistent:
        assert k[K_DFWD] >= 1 and k[K_DBWD] >= 1, k
        assert (k[K_DBWD_DW] >= 1) if dw else (k[K_DBWD_DW] == 0), k
    else:
        assert k[K_DFWD] == k[K_DBWD] == k[K_DBWD_DW] == 0, k
