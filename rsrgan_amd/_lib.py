"""ctypes binding of include/rsrgan.h (librsrgan_hip.so).  Fails loudly when the library is missing."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librsrgan_hip.so")

G_TYPES = {"lstm": 0, "res_lstm_l": 1, "res_lstm_base": 2, "dnn": 3, "rced": 4, "bnlstm": 5, "res_lstm_i": 6}
FLAG_BATCH_NORM = 32          # include/rsrgan.h RSRGAN_FLAG_BATCH_NORM
FLAG_INFER = 64               # include/rsrgan.h RSRGAN_FLAG_INFER: a generator-only, forward-only handle
D_TYPES = {"lstm": 0, "dnn": 1}
NET_G, NET_D = 0, 1
SCALARS = {"g_learning_rate": 0, "d_learning_rate": 1, "mse_lambda": 2, "d_real": 3, "d_fake": 4,
           "l2_scale": 5, "clip_norm": 6, "adam_step": 7, "adam_step_d": 8}
WHAT = {"variables": 0, "adam_m": 1, "adam_v": 2, "ema": 3}

# every symbol include/rsrgan.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = ["rsrgan_default_cfg", "rsrgan_create", "rsrgan_destroy", "rsrgan_last_error", "rsrgan_set_scalar",
           "rsrgan_get_scalar", "rsrgan_num_tensors", "rsrgan_tensor_info", "rsrgan_param_count",
           "rsrgan_get_params", "rsrgan_set_params", "rsrgan_get_grads", "rsrgan_forward_g",
           "rsrgan_g_state_floats", "rsrgan_g_state_reset", "rsrgan_g_state_get", "rsrgan_g_state_set", "rsrgan_forward_g_stream",
           "rsrgan_d_step",
           "rsrgan_g_step", "rsrgan_d_backward", "rsrgan_g_backward", "rsrgan_apply", "rsrgan_grad_buffer",
           "rsrgan_grad_bucket_count", "rsrgan_grad_bucket_info", "rsrgan_grad_bucket_wait",
           "rsrgan_profile_begin", "rsrgan_profile_read", "rsrgan_profile_read_kind", "rsrgan_profile_launches", "rsrgan_op_launch_floor", "rsrgan_device_status", "rsrgan_device_bytes", "rsrgan_set_dropout",
           "rsrgan_op_gemm", "rsrgan_op_gemm2", "rsrgan_op_gemm_batch", "rsrgan_op_gemm16_batch", "rsrgan_op_gemm_last_plan",
           "rsrgan_op_lstm_colsums", "rsrgan_op_colsum", "rsrgan_op_bnl_fold", "rsrgan_version",
           "rsrgan_op_conv_fwd", "rsrgan_op_conv_wgrad", "rsrgan_op_conv_ws_floats", "rsrgan_op_conv_supported", "rsrgan_op_conv_last_plan",
           "rsrgan_op_bn_forward", "rsrgan_op_bn_backward", "rsrgan_op_bn_commit", "rsrgan_op_bn_last_plan",
           "rsrgan_op_bn_seq_forward", "rsrgan_op_bn_seq_backward", "rsrgan_feat_batch", "rsrgan_feat_frames",
           "rsrgan_feat_stream", "rsrgan_feat_denorm", "rsrgan_feat_decode", "rsrgan_feat_wave", "rsrgan_feat_mfcc", "rsrgan_feat_wave_frames",
           "rsrgan_wave_reverb", "rsrgan_wave_reverb_work", "rsrgan_wave_synth", "rsrgan_wave_synth_work", "rsrgan_wave_synth_chunk",
           "rsrgan_hist", "rsrgan_hist_limits", "rsrgan_d_logits", "rsrgan_d_logits_hist",
           "rsrgan_op_segan_sizes", "rsrgan_op_segan_conv2", "rsrgan_op_segan_conv1", "rsrgan_op_segan_colred", "rsrgan_op_segan_last_plan",
           "rsrgan_op_segan_vbn", "rsrgan_op_segan_elem", "rsrgan_op_segan_dhead",
           "rsrgan_op_chunks", "rsrgan_op_update", "rsrgan_op_step_elem", "rsrgan_op_layout", "rsrgan_op_lstm_step", "rsrgan_op_lstm_step_last_plan",
           "rsrgan_segan_default_cfg", "rsrgan_segan_create", "rsrgan_segan_destroy", "rsrgan_segan_set_scalar",
           "rsrgan_segan_num_tensors", "rsrgan_segan_tensor_info", "rsrgan_segan_param_count", "rsrgan_segan_get_params",
           "rsrgan_segan_set_params", "rsrgan_segan_forward_g", "rsrgan_segan_d_backward", "rsrgan_segan_g_backward",
           "rsrgan_segan_grad_buffer", "rsrgan_segan_apply"]


class RsrganCfg(C.Structure):
    _fields_ = [("batch_size", C.c_int32), ("max_frames", C.c_int32), ("input_dim", C.c_int32),
                ("output_dim", C.c_int32), ("g_type", C.c_int32), ("g_layers", C.c_int32), ("g_cells", C.c_int32),
                ("g_proj", C.c_int32), ("d_type", C.c_int32), ("d_layers", C.c_int32), ("d_cells", C.c_int32),
                ("d_proj", C.c_int32), ("l2_scale", C.c_float), ("clip_norm", C.c_float), ("adam_beta1", C.c_float),
                ("adam_beta2", C.c_float), ("adam_eps", C.c_float), ("ema_decay", C.c_float),
                ("lrelu_alpha", C.c_float), ("forget_bias", C.c_float), ("cross_validation", C.c_int32),
                ("flags", C.c_int32), ("d_joint_off", C.c_int32), ("d_joint_dim", C.c_int32), ("g_splice", C.c_int32)]


class SeganCfg(C.Structure):
    """include/rsrgan.h rsrgan_segan_cfg"""
    _fields_ = [("batch_size", C.c_int32), ("input_len", C.c_int32), ("output_dim", C.c_int32), ("n_layers", C.c_int32),
                ("g_depths", C.c_int32 * 16), ("d_depths", C.c_int32 * 16), ("g_kwidth", C.c_int32), ("d_kwidth", C.c_int32),
                ("g_prelu", C.c_int32), ("lrelu_alpha", C.c_float), ("vbn_eps", C.c_float), ("rms_decay", C.c_float),
                ("rms_eps", C.c_float)]


class RsrganError(RuntimeError):
    pass


_lib = None


def load():
    """dlopen librsrgan_hip.so; raise (never fall back) if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); rsrgan_amd has no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    p, i32, i64, f32, vp = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_void_p
    lib.rsrgan_last_error.restype = C.c_char_p
    lib.rsrgan_default_cfg.argtypes = [i32, C.POINTER(RsrganCfg)]
    lib.rsrgan_create.argtypes = [C.POINTER(RsrganCfg), C.c_uint64, C.POINTER(vp)]
    lib.rsrgan_destroy.argtypes = [vp]
    lib.rsrgan_set_scalar.argtypes = [vp, i32, C.c_double]
    lib.rsrgan_get_scalar.argtypes = [vp, i32, C.POINTER(C.c_double)]
    lib.rsrgan_num_tensors.argtypes = [vp, i32]
    lib.rsrgan_tensor_info.argtypes = [vp, i32, i32, C.c_char_p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    lib.rsrgan_param_count.argtypes = [vp, i32]
    lib.rsrgan_param_count.restype = i64
    lib.rsrgan_get_params.argtypes = [vp, i32, i32, p, vp]
    lib.rsrgan_set_params.argtypes = [vp, i32, i32, p, vp]
    lib.rsrgan_get_grads.argtypes = [vp, i32, p, vp]
    lib.rsrgan_forward_g.argtypes = [vp, p, p, i32, p, vp]
    lib.rsrgan_g_state_floats.argtypes = [vp, C.POINTER(i32)]
    lib.rsrgan_g_state_reset.argtypes = [vp, p, vp]
    lib.rsrgan_g_state_get.argtypes = [vp, p, vp]
    lib.rsrgan_g_state_set.argtypes = [vp, p, vp]
    lib.rsrgan_forward_g_stream.argtypes = [vp, p, p, i32, p, vp]
    lib.rsrgan_d_step.argtypes = [vp, p, p, p, i32, p, p, p, i32, vp]
    lib.rsrgan_g_step.argtypes = [vp, p, p, p, i32, p, p, i32, i32, vp]
    lib.rsrgan_d_backward.argtypes = [vp, p, p, p, i32, p, p, p, vp]
    lib.rsrgan_g_backward.argtypes = [vp, p, p, p, i32, p, p, i32, vp]
    lib.rsrgan_apply.argtypes = [vp, i32, vp]
    lib.rsrgan_grad_buffer.argtypes = [vp, i32, C.POINTER(p), C.POINTER(i64)]
    lib.rsrgan_grad_bucket_count.argtypes = [vp, i32]
    lib.rsrgan_grad_bucket_info.argtypes = [vp, i32, i32, C.POINTER(i64), C.POINTER(i64)]
    lib.rsrgan_grad_bucket_wait.argtypes = [vp, i32, i32, vp]
    lib.rsrgan_profile_begin.argtypes = [vp]
    lib.rsrgan_profile_read.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.rsrgan_profile_read_kind.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.rsrgan_device_status.argtypes = [vp, C.POINTER(i32)]
    lib.rsrgan_device_bytes.argtypes = [vp, C.POINTER(i64)]
    lib.rsrgan_set_dropout.argtypes = [vp, f32, C.c_uint64]
    lib.rsrgan_profile_launches.argtypes = [vp, C.POINTER(i64)]
    lib.rsrgan_op_launch_floor.argtypes = [i32, i32, C.POINTER(C.c_double), vp]
    lib.rsrgan_op_gemm.argtypes = [p, i32, i32, p, i32, i32, p, i32, i32, i32, i32, p, i32, f32, i32, vp]
    pp = C.POINTER(C.c_void_p)
    lib.rsrgan_op_gemm2.argtypes = [p, i32, i32, p, i32, i32, p, i32, i32, p, i32, i32, i32, i32, p, i32, f32, i32, i32, i64, i64, i32, i32, vp]
    lib.rsrgan_op_gemm_batch.argtypes = [i32, pp, i32, pp, i32, i32, pp, i32, pp, i32, i32, i32, i32, i32, i32, vp]
    lib.rsrgan_op_gemm16_batch.argtypes = [i32, pp, i32, pp, i32, i32, pp, i32, pp, i32, i32, i32, i32, i32, vp]
    lib.rsrgan_op_gemm_last_plan.argtypes = [C.POINTER(i32)]
    lib.rsrgan_op_lstm_colsums.argtypes = [i32, pp, pp, pp, pp, pp, pp, pp, i32, i32, vp]
    lib.rsrgan_op_colsum.argtypes = [p, i32, p, i32, p, i32, i32, i32, vp]
    lib.rsrgan_op_bnl_fold.argtypes = [p, p, pp, p, i32, i32, p, i32, p, i32, p, p, p, vp]
    lib.rsrgan_op_conv_fwd.argtypes = [p, i32, i32, p, i32, i32, p, i32, p, p, i32, i32, i32, i32, i32, i32, vp]
    lib.rsrgan_op_conv_wgrad.argtypes = [p, i32, i32, p, i32, i32, p, i32, p, p, i64, i32, i32, i32, i32, i32, vp]
    lib.rsrgan_op_conv_ws_floats.argtypes = [i32, i32, i32, i32, i32]
    lib.rsrgan_op_conv_ws_floats.restype = i64
    lib.rsrgan_op_conv_supported.argtypes = [i32, i32, i32, i32, i32]
    lib.rsrgan_op_conv_last_plan.argtypes = [C.POINTER(i32)]
    lib.rsrgan_op_bn_forward.argtypes = [p, i32, p, i32, i32, i32, i32, pp, p, i32, i32, i32, p, i64, vp]
    lib.rsrgan_op_bn_backward.argtypes = [p, i32, p, i32, p, i32, i32, i32, i32, p, i32, p, p, i32, i32, p, p, i64, vp]
    lib.rsrgan_op_bn_seq_forward.argtypes = [p, i32, p, i32, i32, i32, pp, p, i32, i32, i32, f32, i32, i32, p, i64, vp]
    lib.rsrgan_op_bn_seq_backward.argtypes = [p, i32, p, i32, p, i32, i32, i32, p, i32, p, p, i32, i32, f32, i32, i32, p, p, i64, vp]
    lib.rsrgan_feat_batch.argtypes = [p, i64, p, i32, i32, i32, i32, i32, p, p, p, p, vp]
    lib.rsrgan_feat_frames.argtypes = [p, i64, p, i32, i32, i32, i32, p, p, p, vp]
    lib.rsrgan_feat_stream.argtypes = [p, i64, p, p, i32, i32, i32, i32, i32, i32, p, p, p, p, vp]
    lib.rsrgan_feat_denorm.argtypes = [p, p, i32, i32, i32, p, p, p, vp]
    lib.rsrgan_feat_decode.argtypes = [p, i64, p, p, p, i32, i32, p, p, p, i64, vp]
    lib.rsrgan_feat_wave.argtypes = [p, i32, i64, p, p, i32, i32, i32, i32, f32, p, p, p, i64, vp]
    lib.rsrgan_feat_mfcc.argtypes = [p, i32, i64, p, p, i32, i32, i32, i32, f32, p, p, p, p, i32, i32, p, i32, p, i64, vp]
    lib.rsrgan_feat_wave_frames.argtypes = [i32]
    lib.rsrgan_wave_reverb.argtypes = [p, i32, i64, p, p, i64, p, p, i64, p, p, p, p, i32, i32, i32, i32, p, i32, p, i64, p, p, p, i64, vp]
    lib.rsrgan_wave_reverb_work.argtypes = [i32, i64, i64, i32]
    lib.rsrgan_wave_reverb_work.restype = i64
    lib.rsrgan_wave_synth.argtypes = [p, i32, i64, p, p, p, i64, i32, i32, i32, i32, f32, p, p, p, i64, p, p, i64, vp]
    lib.rsrgan_wave_synth_work.argtypes = [i32, i64, i64, i32]
    lib.rsrgan_wave_synth_work.restype = i64
    lib.rsrgan_wave_synth_chunk.argtypes = []
    lib.rsrgan_hist.argtypes = [i32, pp, C.POINTER(i64), p, vp]
    lib.rsrgan_hist_limits.argtypes = [C.POINTER(C.c_double), C.POINTER(i32)]
    lib.rsrgan_d_logits.argtypes = [vp, p, p, C.POINTER(i32), vp]
    lib.rsrgan_d_logits_hist.argtypes = [vp, p, vp]
    lib.rsrgan_op_bn_commit.argtypes =[i32, pp, pp, C.POINTER(i32), i32, vp]
    lib.rsrgan_op_bn_last_plan.argtypes = [C.POINTER(i32)]
    lib.rsrgan_op_segan_sizes.argtypes = [i32, C.POINTER(i64), C.POINTER(i64)]
    for f in (lib.rsrgan_op_segan_conv2, lib.rsrgan_op_segan_conv1, lib.rsrgan_op_segan_colred, lib.rsrgan_op_segan_vbn, lib.rsrgan_op_segan_elem,
              lib.rsrgan_op_segan_dhead, lib.rsrgan_op_update, lib.rsrgan_op_step_elem, lib.rsrgan_op_layout, lib.rsrgan_op_lstm_step):
        f.argtypes = [i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(C.c_float), vp]
    lib.rsrgan_op_segan_last_plan.argtypes = [C.POINTER(i32)]
    lib.rsrgan_op_lstm_step_last_plan.argtypes = [C.POINTER(i32)]
    lib.rsrgan_op_chunks.argtypes = [C.POINTER(i64), i32, C.POINTER(i32), i64, C.POINTER(i32)]
    lib.rsrgan_segan_default_cfg.argtypes = [C.POINTER(SeganCfg)]
    lib.rsrgan_segan_create.argtypes = [C.POINTER(SeganCfg), C.c_uint64, C.POINTER(vp)]
    lib.rsrgan_segan_destroy.argtypes = [vp]
    lib.rsrgan_segan_set_scalar.argtypes = [vp, i32, C.c_double]
    lib.rsrgan_segan_num_tensors.argtypes = [vp, i32]
    lib.rsrgan_segan_tensor_info.argtypes = [vp, i32, i32, C.c_char_p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    lib.rsrgan_segan_param_count.argtypes = [vp, i32]
    lib.rsrgan_segan_param_count.restype = i64
    lib.rsrgan_segan_get_params.argtypes = [vp, i32, i32, p, vp]
    lib.rsrgan_segan_set_params.argtypes = [vp, i32, i32, p, vp]
    lib.rsrgan_segan_forward_g.argtypes = [vp, p, p, p, vp]
    lib.rsrgan_segan_d_backward.argtypes = [vp, p, p, p, p, p, p, p, i32, vp]
    lib.rsrgan_segan_g_backward.argtypes = [vp, p, p, p, p, p, p, i32, vp]
    lib.rsrgan_segan_grad_buffer.argtypes = [vp, i32, C.POINTER(p), C.POINTER(i64)]
    lib.rsrgan_segan_apply.argtypes = [vp, i32, vp]
    _lib = lib
    return lib


OP_NOT_APPLICABLE = 1         # include/rsrgan.h RSRGAN_OP_NOT_APPLICABLE
# rsrgan_op_gemm_last_plan: kernel classes and the fields of the record
GEMM_CLASSES = {0: "none", 1: "gemm16", 2: "n32", 3: "k_gemm", 4: "k_gemm_s", 5: "gemm16_batch", 6: "k_gemm_batch", 7: "k_gemm_s_batch"}
GEMM_PLAN_FIELDS = ("cls", "bm", "bn", "W", "n_dp", "fixup", "splits", "Ur")
# force_cfg of rsrgan_op_gemm2: (kernel class, BM, BN) of each tile form
GEMM_FORMS = [("k_gemm", 128, 128), ("k_gemm", 96, 128), ("k_gemm", 128, 96), ("k_gemm", 256, 64), ("k_gemm", 256, 32),
              ("k_gemm_s", 256, 256), ("k_gemm_s", 128, 256), ("k_gemm_s", 256, 128)]
# rsrgan_op_conv_last_plan: kernel families, branches and the 19 fields of each launch of the record
CONV_FAMILIES = {0: "none", 1: "fwd", 2: "fwd4", 3: "wgrad", 4: "wgrad4"}
CONV_FWD_BRANCHES = {1: "whole", 2: "main", 3: "rem"}
CONV_WGRAD_BRANCHES = {1: "k2", 2: "rows", 3: "search"}
CONV_PLAN_FIELDS = ("family", "a0", "a1", "a2", "branch", "TW", "FB", "gx", "gy", "gz", "lds", "DH", "fpg", "groups", "nstrips", "nkg",
                    "PS", "waves", "gmax")
# rsrgan_op_bn_last_plan: routes and the fields of the record; the order of the eight variables of a layer
BN_ROUTES = {0: "none", 1: "small", 2: "sliced", 3: "narrow"}
BN_PLAN_FIELDS = ("route", "backward", "calls", "launches", "slices", "per", "pgx", "pgy", "egrid", "q", "R")
# rsrgan_op_segan_*: the op codes of each family and the fields of the column-reduction record
SEGAN_OPS = {"conv2": ("conv2_fwd", "conv2_wgrad", "tconv2"), "conv1": ("conv1_fwd", "conv1_wgrad", "tconv1"),
             "colred": ("sum", "dalpha", "moments", "vbn_bwd"), "vbn": ("coef", "apply", "bwd_coef", "bwd_apply"),
             "elem": ("pad_rows", "prep_tconv", "prep_tconv_many", "interleave", "act_fwd", "act_bwd", "copy_cols", "build_joint1", "sum_all",
                      "lsgan", "l1", "rmsprop"),
             "dhead": ("fwd", "bwd")}
# rsrgan_op_update / rsrgan_op_step_elem: the op codes, and the slots of the device scalars `dyn` (csrc/kernels.h DYN_*)
UPDATE_OPS = ("sumsq", "dw_reduce", "l2", "apply_sgd", "apply_adam")
STEP_ELEM_OPS = ("lsgan", "dhead", "mse", "g_total", "l2_total", "adam_tick", "dropout_fwd", "dropout_bwd", "lrelu_bwd")
# rsrgan_op_layout: the op codes (one per launch_* function of the layout, staging and weight-copy kernels)
LAYOUT_OPS = ("pack_tm", "unpack_bm", "stage_inputs", "build_d_input", "add_noise_rows", "transpose", "transpose_many", "swizzle_many", "im2col",
              "col2im", "expand_c4", "gstate", "window_len", "zero_many", "fill", "build_joint", "slice_cols", "pad_copy", "copy_f")
# rsrgan_op_lstm_step: the op codes (one per step launcher), the forms of rsrgan_op_lstm_step_last_plan and the fields of its record
LSTM_STEP_OPS = ("fwd_gates", "fwd_proj", "bwd_a", "bwd_b", "bwd_b_splitk")
LSTM_STEP_FORMS = {0: "none", 1: "gates<18,1>", 2: "gates<18,2>", 3: "gates<32,2>", 4: "proj<4>", 5: "proj<8>", 6: "proj<4,drop>", 7: "proj<8,drop>",
                   8: "bwd_a<4>", 9: "bwd_a<18>", 10: "bwd_a<24>", 11: "bwd_a<4,drop>", 12: "bwd_a<18,drop>", 13: "bwd_a<24,drop>",
                   14: "bwd_b<8,8,8,1>", 15: "bwd_b<8,0,6>", 16: "splitk"}
LSTM_STEP_PLAN_FIELDS = ("form", "threads", "grid", "map_valid", "KG", "kpg", "grid2", "lds", "groups", "tiled")
DYN_SLOTS = {"g_lr": 0, "d_lr": 1, "lambda": 2, "d_real": 3, "d_fake": 4, "l2": 5, "clip": 6, "beta1": 7, "beta2": 8, "eps": 9, "ema": 10,
             "adam_lrt": 11, "adam_lrt_d": 12}
DYN_COUNT = 16
SEGAN_PLAN_FIELDS = ("vec", "mode", "chunk", "chunks_per", "grid")
BN_VARS = ("beta", "gamma", "moving_mean", "moving_variance", "renorm_mean", "renorm_mean_weight", "renorm_stddev", "renorm_stddev_weight")


def ptr_table(ptrs):
    """a C array of device pointers (None stays NULL) for the batched operator entries"""
    return (C.c_void_p * max(len(ptrs), 1))(*[None if q is None else q for q in ptrs])


_hist_limits = None


def hist_limits():
    """the bucket limits of rsrgan_hist (rsrgan_hist_limits: built in C++, on the host) as a float64 array; no device is needed"""
    global _hist_limits
    if _hist_limits is None:
        import numpy as np
        lib = load()
        n = C.c_int32()
        check(lib.rsrgan_hist_limits(None, C.byref(n)))
        buf = (C.c_double * n.value)()
        check(lib.rsrgan_hist_limits(buf, C.byref(n)))
        _hist_limits = np.frombuffer(buf, np.float64).copy()
        _hist_limits.setflags(write=False)
    return _hist_limits


def check(rc):
    if rc != 0:
        raise RsrganError("librsrgan_hip error %d: %s" % (rc, load().rsrgan_last_error().decode()))
