"""The configurations whose handle construction is pinned (tests/test_gpu_init_tables.py against tests/golden/init_tables.json,
recorded by tools/record_init_tables.py): together they take every branch of Model::init at least once, at the smallest shapes at
which the branch exists (max_frames <= 6).  One list, shared by the recorder and the test, so the two cannot drift apart."""
import hashlib

from oracle import rsrgan_oracle as O
from tests.helpers import NET_D, NET_G, small_cfg

SEED = 4321
WAVEFRONT, GRAPH, SUPERVISED = 1, 2, 16          # the flag bits of include/rsrgan.h


def _kw(cfg, B, T, flags=3, **extra):
    """HipEngine's keyword arguments for a NetCfg"""
    kw = dict(batch_size=B, max_frames=T, input_dim=cfg.input_dim, output_dim=cfg.output_dim, g_type=cfg.g_type, g_layers=cfg.g_layers,
              g_cells=cfg.g_cells, g_proj=cfg.g_proj, d_layers=cfg.d_layers, d_cells=cfg.d_cells, d_proj=cfg.d_proj, flags=flags)
    if cfg.d_type != "lstm":
        kw["d_type"] = cfg.d_type
    kw.update(extra)
    return kw


def _frame(g_type, fed, splice, joint, **extra):
    """a frame-level generator with discriminator_dnn, as rsrgan_amd.GAN words it (max_frames = 1)"""
    kw = dict(batch_size=7, max_frames=1, input_dim=fed, output_dim=5, g_type=g_type, d_type="dnn", d_joint_off=joint * (splice // 2),
              d_joint_dim=joint, g_splice=splice, d_layers=2, d_cells=18)
    kw.update(extra)
    return kw


_DPERSIST = small_cfg("lstm", output_dim=40, d_cells=256, d_proj=40)
_BNL = dict(input_dim=9, output_dim=5, g_type="bnlstm", g_layers=2, g_cells=64, g_proj=32, max_frames=6)
# tests/test_gpu_plan_edges.py baseline_named(): the single-hop (unprojected) persistent forward, B = 64
_UNPROJECTED = O.NetCfg(g_layers=2, g_cells=512, g_proj=0, d_type="dnn", d_layers=4, d_cells=1024)
# tests/test_gpu_dnn_gan.py: 6-dim frames, context (2, 1), 3 x 20 generator, 2 x 18 discriminator
_DNN = dict(g_layers=3, g_cells=20)
# tests/test_gpu_trainers.py test_rced_generator_matches_oracle: 9-dim frames, the filter table scaled to 4 channels
_RCED = dict(g_layers=9, g_cells=4)

CASES = [
    ("lstm_small", _kw(small_cfg("lstm"), 3, 5)),
    ("lstm_small_cross_validation", _kw(small_cfg("lstm"), 3, 5, cross_validation=True)),
    ("lstm_small_no_ema", _kw(small_cfg("lstm"), 3, 5, ema_decay=0.0)),
    ("lstm_d256_b16", _kw(_DPERSIST, 16, 5)),                        # the discriminator's persistent rings, in-kernel weight gradients
    ("reference_b32", _kw(O.NetCfg(), 32, 4)),                       # the generator's rings, trail_fits, DPIPE
    ("reference_b8", _kw(O.NetCfg(), 8, 4)),                         # row padding to 32
    ("unprojected_b64", _kw(_UNPROJECTED, 64, 6)),
    ("res_lstm_l_small", _kw(small_cfg("res_lstm_l"), 3, 5)),
    ("res_lstm_base_small", _kw(small_cfg("res_lstm_base"), 3, 5)),
    ("res_lstm_i_supervised", _kw(small_cfg("res_lstm_i", g_proj=9), 3, 5, flags=3 | SUPERVISED)),
    ("lstm_batch_norm", _kw(small_cfg("lstm"), 3, 5, batch_norm=True)),
    ("lstm_batch_norm_inference", _kw(small_cfg("lstm"), 3, 5, batch_norm=True, inference=True)),
    ("lstm_d_dnn", _kw(small_cfg("lstm", d_type="dnn", d_layers=2, d_cells=11), 3, 5)),
    ("lstm_inference", _kw(small_cfg("lstm"), 3, 5, inference=True)),
    ("res_lstm_l_inference", _kw(small_cfg("res_lstm_l"), 3, 5, inference=True)),
    ("bnlstm_supervised_b4", dict(_BNL, batch_size=4, flags=3 | SUPERVISED)),
    ("bnlstm_inference", dict(_BNL, batch_size=4, flags=WAVEFRONT | SUPERVISED, inference=True)),
    ("dnn", _frame("dnn", 24, 4, 6, **_DNN)),
    ("dnn_batch_norm", _frame("dnn", 24, 4, 6, batch_norm=True, **_DNN)),
    ("rced_splice4", _frame("rced", 36, 4, 9, **_RCED)),             # even splice: patch-matrix GEMMs
    ("rced_splice4_batch_norm", _frame("rced", 36, 4, 9, batch_norm=True, **_RCED)),
    ("rced_splice3", _frame("rced", 27, 3, 9, **_RCED)),             # odd splice: the implicit-GEMM convolution's buffers
]


def describe(kw):
    """everything of a handle that init decides, as JSON-able values: tables, byte count, initial bits, bucket ranges, state width"""
    from rsrgan_amd import _lib
    from rsrgan_amd.engine_hip import HipEngine
    e = HipEngine(seed=SEED, **kw)
    try:
        nets = (NET_G,) if e.inference else (NET_G, NET_D)
        out = {"device_bytes": e.device_bytes(), "tables": {}, "param_count": {}, "variables_sha256": {}, "grad_buckets": {}}
        for net in nets:
            k = "g" if net == NET_G else "d"
            out["tables"][k] = [[name, list(shape), off] for name, shape, off in e.tensor_table(net)]
            out["param_count"][k] = e.param_count(net)
            out["variables_sha256"][k] = hashlib.sha256(e.get_params(net, "variables").cpu().numpy().tobytes()).hexdigest()
            if not e.inference:
                out["grad_buckets"][k] = [list(b) for b in e.grad_buckets(net)]
        try:
            out["g_state_floats"] = e.g_state_floats()
        except _lib.RsrganError:
            out["g_state_floats"] = None
        return out
    finally:
        e.close()
