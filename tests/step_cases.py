"""The training step's call sequences whose results are pinned (tests/test_gpu_step_fixture.py against tests/golden/step_fixture.json,
recorded by tools/record_step_fixture.py): together they enter every branch of Model::d_backward, Model::g_backward and their helpers
(csrc/model_step.cpp) at least once, at the smallest shapes at which the branch exists.  One list and one runner, shared by the recorder
and the test, so the two cannot drift apart.

A case builds a model with fixed seeds, runs its call sequence three times over -- every graph segment runs eagerly, is captured, is
replayed -- and records per call the returned losses as fp32 bit patterns, at the end the SHA-256 of every variable (Adam moments and
EMA where the handle has them; both gradient buffers where the sequence stops before `apply`), after one more profiled D + G pass the
recurrence launch counts, and the device status word.  Bits are reproducible across processes (tests/test_gpu_placement.py relies on
the same), so everything is compared exactly.

Switches of process scope are read once per process: the cases are grouped, one worker subprocess per group and environment."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPERVISED, OVERLAP = 16, 4          # flag bits of include/rsrgan.h (1 = wavefront, 2 = graphs)
NOISE_STD = 0.3


# ---- call sequences: (op, options).  op "d" / "g": engine.d_backward / g_backward with train, apply, reuse, noise_real ("nr"), noise_fake
# ("nf": True = a tensor is passed); "apply": engine.apply(net); "wait": every gradient bucket's event awaited on another stream ----
def D(**kw):
    return ("d", dict(dict(train=True, apply=True, nr=False, nf=False), **kw))


def G(**kw):
    return ("g", dict(dict(train=True, apply=True, reuse=False, nf=False), **kw))


STEP = [D(), G(reuse=True)]                               # rsrgan_d_step + rsrgan_g_step on the D-run's forward
STEP_FRESH = [D(), G()]                                   # the G-run recomputes the generator's forward
STEP_TWICE = [D(), G(reuse=True), G()]                    # gen_updates = 2: one G-run of each kind
GRADS_ONLY = [D(apply=False), G(apply=False, reuse=True)]  # stops before apply: the gradient buffers are hashed
DATA_PARALLEL = [D(apply=False), ("wait", 1), ("apply", 1), G(apply=False, reuse=True), ("wait", 0), ("apply", 0)]
EVAL = [D(train=False), G(train=False)]
SUP = [G()]
REFUSE = "refuse"


def _case(name, note, net, B, T, flags, seq, env=None, henv=None, group=None, **build):
    """env: the worker process's environment (switches of process scope); henv: set around the handle's construction (handle scope)"""
    return dict(name=name, note=note, net=net, B=B, T=T, flags=flags, seq=seq, env=dict(env or {}), henv=dict(henv or {}), group=group,
                build=build)


HANDLE_SCOPE = ("TRAIL", "GPERSIST", "DPERSIST", "DPIPE")          # csrc/switches.h: read when the handle is created
HANDLE_GROUP = "ref_handle_switches"


def _ref_switch(var, val, note, seq=STEP_TWICE, net="ref:lstm"):
    name = "ref_lstm_%s_%s" % (var.lower(), val)
    if var in HANDLE_SCOPE:
        return _case(name, note, net, 32, 5, 3, seq, henv={"RSRGAN_" + var: val}, group=HANDLE_GROUP)
    return _case(name, note, net, 32, 5, 3, seq, env={"RSRGAN_" + var: val}, group="%s=%s" % (var, val))


CASES = [
    # -- the supervised trainer's step (the `if (supervised())` block of g_backward)
    _case("sup_lstm_train", "supervised: gradients, no L2 (memset of the L2 loss)", "small:lstm", 6, 5, 1 | SUPERVISED, SUP, group="small"),
    _case("sup_lstm_train_l2", "supervised: launch_l2 + launch_l2_total", "small:lstm", 6, 5, 1 | SUPERVISED, SUP, group="small", l2_scale=1e-3),
    _case("sup_lstm_eval", "supervised: eval fetch (launch_mse without dy)", "small:lstm", 6, 5, 1 | SUPERVISED, [G(train=False)], group="small",
          l2_scale=1e-3),
    _case("sup_lstm_batch_norm", "supervised + sequence batch norm: seq_bn_commit(2) between L2 and g_total", "small:lstm", 6, 5,
          3 | SUPERVISED, SUP, group="small", l2_scale=1e-3, batch_norm=True),
    _case("sup_res_lstm_i_ref", "reference-size res_lstm_i: persistent launches without the fused ones (a.res == 2)", "ref:res_lstm_i", 32, 5,
          3 | SUPERVISED, SUP, group="ref_res", l2_scale=1e-3),
    # -- flags 0: layer by layer (d_backward_pass, the three wirings of g_backward_pass, g_forward, add_noise_rows)
    _case("f0_lstm", "flags 0 lstm: g_backward_pass lstm wiring, reuse, direct D input", "small:lstm", 6, 5, 0, STEP, group="small"),
    _case("f0_lstm_fresh_noise", "flags 0: fresh forward, noise_real + noise_fake (not `direct`)", "small:lstm", 6, 5, 0,
          [D(nr=True, nf=True), G(nf=True)], group="small"),
    _case("f0_res_lstm_l", "flags 0 res_lstm_l: accumulate-in-place wiring", "small:res_lstm_l", 6, 5, 0, STEP_FRESH, group="small"),
    _case("f0_res_lstm_base", "flags 0 res_lstm_base: no d(h0)", "small:res_lstm_base", 6, 5, 0, STEP, group="small"),
    _case("f0_eval", "flags 0: eval fetch of each run", "small:lstm", 6, 5, 0, EVAL, group="small"),
    _case("f0_grads_l2", "flags 0: stop before apply (gradient buffers), L2 on", "small:lstm", 6, 5, 0, GRADS_ONLY, group="small", l2_scale=1e-3),
    # -- discriminator_dnn with a sequence generator (fc_backward, the "no noise" rule)
    _case("ddnn_f0", "d_type dnn, flags 0: fc_backward in both runs; the noise given is ignored", "small:lstm:ddnn", 6, 5, 0,
          [D(nr=True, nf=True), G(nf=True)], group="small"),
    _case("ddnn_f1", "d_type dnn, flags 1: one-chain waves, want_grads && d_dnn() backward", "small:lstm:ddnn", 6, 5, 1, STEP_TWICE, group="small"),
    _case("ddnn_f1_eval", "d_type dnn: eval fetches", "small:lstm:ddnn", 6, 5, 1, EVAL, group="small"),
    # -- flags 1 and 3 on small nets: no persistent plan applies (waves with FcStage, three-chain D-run wave, SEG_G_FCIN)
    _case("f1_lstm", "flags 1 lstm: forward / backward waves with FcStage, eager", "small:lstm", 6, 5, 1, STEP_TWICE, group="small"),
    _case("f1_lstm_noise", "flags 1: noise through the FcStage", "small:lstm", 6, 5, 1, [D(nr=True, nf=True), G(reuse=True, nf=True), G(nf=True)],
          group="small"),
    _case("f3_lstm", "flags 3 lstm: SEG_D, SEG_G_MAIN, SEG_G_FCIN, SEG_G_TAIL, SEG_APPLY_G captured and replayed", "small:lstm", 6, 5, 3,
          STEP_TWICE, group="small"),
    _case("f3_lstm_l2_bn", "flags 3 lstm + batch norm + L2: tail_body's L2 and seq_bn_commit", "small:lstm", 6, 5, 3, STEP_TWICE, group="small",
          l2_scale=1e-3, batch_norm=True),
    _case("f3_res_lstm_l", "flags 3 res_lstm_l: wave backward, update inlined (no FCIN segment)", "small:res_lstm_l", 6, 5, 3, STEP_TWICE,
          group="small"),
    _case("f3_res_lstm_base", "flags 3 res_lstm_base", "small:res_lstm_base", 6, 5, 3, STEP, group="small"),
    _case("f3_eval", "flags 3: eval fetches (want_grads = false keys)", "small:lstm", 6, 5, 3, EVAL + STEP, group="small"),
    _case("f3_data_parallel", "flags 3 small: bucketed segments on the launch wave (rnn_backward with defer_wgrads), layer_wgrads per layer",
          "small:lstm", 6, 5, 3, DATA_PARALLEL, group="small"),
    _case("f5_overlap", "flags 1|4: weight gradients on the side stream in chunks (overlap(): not bucketed, no graphs)", "small:lstm", 6, 5,
          1 | OVERLAP, STEP + [D(apply=False), ("apply", 1), G(apply=False), ("apply", 0)], group="small"),
    # -- reference sizes, flags 3, defaults
    _case("ref_lstm", "reference lstm: fused forward / backward launches, fcs_inside, inlined update, one graph per run", "ref:lstm", 32, 5, 3,
          STEP_TWICE, group="ref_lstm"),
    _case("ref_lstm_t1", "reference lstm at T = 1", "ref:lstm", 32, 1, 3, STEP_TWICE, group="ref_lstm"),
    _case("ref_lstm_padded", "reference lstm, 8 rows padded to 32 (trail_nrt)", "ref:lstm", 8, 5, 3, STEP_TWICE, group="ref_lstm"),
    _case("ref_lstm_noise_eval", "reference lstm: noise tensors, then eval fetches", "ref:lstm", 32, 5, 3,
          [D(nr=True, nf=True), G(reuse=True, nf=True), G(nf=True)] + EVAL, group="ref_lstm"),
    _case("ref_lstm_grads", "reference lstm: rsrgan_d_backward / rsrgan_g_backward only (gradient buffers)", "ref:lstm", 32, 5, 3,
          [D(apply=False), G(apply=False, reuse=True), G(apply=False)], group="ref_lstm"),
    _case("ref_res_lstm_l", "reference res_lstm_l: fused launches with the residual sums, dk_tmp", "ref:res_lstm_l", 32, 5, 3, STEP_TWICE,
          group="ref_res"),
    # -- one switch at a time
    _ref_switch("TRAIL", "0", "two BPTT launches and the two GEMMs between them (!trailed)"),
    _ref_switch("TRAIL_FWD", "0", "persist_forward_g + tail + persist_forward in the fresh G-run"),
    _ref_switch("FC_SIDE", "0", "!fcs_inside: output-FC gradients behind the launch, SEG_G_FCIN, no inlined update"),
    _ref_switch("FUSED_SEG", "0", "updates in segments of their own; bucketed stays off"),
    _ref_switch("DHEAD", "0", "d_logits + launch_lsgan + the head's GEMMs"),
    _ref_switch("GPERSIST", "1", "persistent forward only: launch wave backward behind it"),
    _ref_switch("GPERSIST", "2", "persistent BPTT only: forward wave with FcStage in front of it"),
    _ref_switch("DPERSIST", "0", "fold_forward / rnn_forward, rnn_backward for the discriminator alone"),
    _ref_switch("DW_INKERNEL", "0", "persist_backward's batch_wgrads branch"),
    _ref_switch("DPIPE", "1", "dsplit, gsplit, bwd_rest, ev_dfree", seq=STEP_TWICE + STEP),
    _case("ref_res_lstm_l_dpipe_1", "DPIPE with res_lstm_l: bwd_rest without fcs_inside", "ref:res_lstm_l", 32, 5, 3, STEP_TWICE,
          henv={"RSRGAN_DPIPE": "1"}, group=HANDLE_GROUP),
    _ref_switch("DPIPE", "2", "a noise_real tensor under the pipelined D-run", seq=[D(nr=True), G(reuse=True), D(nr=True, nf=True), G(nf=True)]),
    _case("ref_lstm_dpipe_1_noise_real", "DPIPE=1 with a noise_real tensor: the stream-ordered D-run", "ref:lstm", 32, 5, 3,
          [D(nr=True), G(reuse=True)], henv={"RSRGAN_DPIPE": "1"}, group=HANDLE_GROUP),
    # -- the data-parallel sequence at reference lstm size
    _case("ref_dp", "bucketed segments, batch_wgrads applicable (SEG_G_BATCH + dK per layer)", "ref:lstm", 32, 5, 3, DATA_PARALLEL, group="ref_dp"),
    _case("ref_dp_l2", "the same with L2: bucket marks reset before finish_buckets", "ref:lstm", 32, 5, 3, DATA_PARALLEL, group="ref_dp",
          l2_scale=1e-3),
    _case("ref_dp_wgrad_batch_0", "bucketed, layer_wgrads per layer", "ref:lstm", 32, 5, 3, DATA_PARALLEL, env={"RSRGAN_WGRAD_BATCH": "0"},
          group="WGRAD_BATCH=0"),
    _case("ref_dp_l2_wgrad_batch_0", "the same with L2", "ref:lstm", 32, 5, 3, DATA_PARALLEL, env={"RSRGAN_WGRAD_BATCH": "0"},
          group="WGRAD_BATCH=0", l2_scale=1e-3),
    # -- DropoutWrapper on a reference-size lstm
    _case("ref_lstm_dropout", "seq_drop_on: a fresh forward every run, persistent generator paths off", "ref:lstm", 32, 5, 3,
          STEP_TWICE + [G(train=False)], group="ref_dp", keep_prob=0.8),
    # -- refusals: status code and message, no launch
    _case("refuse_d_on_supervised", "d_backward on a supervised handle", "small:lstm", 6, 5, 1 | SUPERVISED, REFUSE, group="small", refusal="d"),
    _case("refuse_reuse_without_forward", "reuse_g_forward on a fresh handle", "small:lstm", 6, 5, 3, REFUSE, group="small", refusal="reuse"),
    _case("refuse_cv_batch_norm_grads", "gradients of a cross-validation batch-norm model", "small:lstm", 6, 5, 3, REFUSE, group="small",
          refusal="cv_bn", batch_norm=True, cross_validation=True),
    _case("refuse_null_labels", "null labels in both runs", "small:lstm", 6, 5, 3, REFUSE, group="small", refusal="labels"),
]

GROUPS = []
for _c in CASES:
    if _c["group"] not in GROUPS:
        GROUPS.append(_c["group"])


def group_cases(group):
    cs = [c for c in CASES if c["group"] == group]
    assert cs and all(c["env"] == cs[0]["env"] for c in cs), group          # one environment per worker
    return cs


# ---- building and running a case (in the worker process) ----
def _net_cfg(net):
    from oracle import rsrgan_oracle as O
    from tests.helpers import small_cfg
    size, g_type = net.split(":")[:2]
    if size == "small":
        kw = dict(d_type="dnn", d_layers=2, d_cells=11) if net.endswith(":ddnn") else {}
        return small_cfg(g_type, **kw)
    if g_type == "res_lstm_i":
        from tests import res_lstm_i_ref as R
        return R.make_cfg()
    return O.NetCfg() if g_type == "lstm" else O.NetCfg.res_lstm_l(g_type=g_type)


def _build(case):
    from tests.helpers import args_for, build_hip_pair, overrides, rand_params
    cfg = _net_cfg(case["net"])
    B, T, flags = case["B"], case["T"], case["flags"]
    kw = {k: v for k, v in case["build"].items() if k not in ("refusal", "cross_validation")}
    if cfg.g_type == "res_lstm_i":                    # RNNTrainer only (GAN_RNN refuses the type, as the reference GAN does)
        from rsrgan_amd.trainer import RNNTrainer
        from tests import res_lstm_i_ref as R
        m = RNNTrainer(None, args_for(cfg, B, **kw), ["gpu:0"], max_frames=T, net_overrides=dict(overrides(cfg), flags=flags))
        m.set_vars(R.rand_g(cfg, 5), rand_params(R.table_cfg(cfg), 5)[1])
        return cfg, m
    if case["build"].get("batch_norm") or case["build"].get("cross_validation"):
        # (the batch-norm table is not build_hip_pair's: the library's own seeded initial values, which tests/test_gpu_init_tables.py pins)
        from rsrgan_amd import GAN_RNN
        m = GAN_RNN(None, args_for(cfg, B, **kw), ["gpu:0"], cross_validation=bool(case["build"].get("cross_validation")), max_frames=T,
                    net_overrides=dict(overrides(cfg), flags=flags))
        return cfg, m
    return cfg, build_hip_pair(cfg, B, T, seed=5, flags=flags, **kw)[0]


def _bits(t):
    import numpy as np
    return [int(v) for v in np.ravel(t.cpu().numpy()).view(np.uint32)]


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _refusal(case, e, x, lab, ln):
    import ctypes as C
    import torch
    from rsrgan_amd import _lib
    kind = case["build"]["refusal"]
    out = []

    def attempt(f):
        try:
            f()
            out.append("accepted")
        except _lib.RsrganError as err:
            out.append(str(err))
    if kind == "d":
        attempt(lambda: e.d_backward(x, lab, ln))
    elif kind == "reuse":
        attempt(lambda: e.g_backward(x, lab, ln, reuse=True, apply=True))
    elif kind == "cv_bn":
        attempt(lambda: e.g_backward(x, lab, ln, train=True, apply=False))
    else:
        xs, lens = e._f32(x), e._i32(ln)
        o = torch.empty(4, dtype=torch.float32, device=e.device)
        p = lambda t: C.c_void_p(t.data_ptr())
        attempt(lambda: _lib.check(e.lib.rsrgan_d_step(e.h, p(xs), None, p(lens), case["T"], None, None, p(o), 1, e._stream())))
        attempt(lambda: _lib.check(e.lib.rsrgan_g_step(e.h, p(xs), None, p(lens), case["T"], None, p(o), 1, 0, e._stream())))
    return out


def run_case(case):
    import ctypes as C
    import numpy as np
    import torch
    from rsrgan_amd import _lib
    from tests.helpers import NET_D, NET_G, rand_batch
    saved = {k: os.environ.get(k) for k in case["henv"]}
    os.environ.update(case["henv"])
    try:
        cfg, model = _build(case)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    e = model.engine
    B, T = case["B"], case["T"]
    x, lab, ln = rand_batch(cfg, B, T, seed=6, ragged=True)
    rng = np.random.default_rng(7)
    noise = {k: (NOISE_STD * rng.standard_normal((B, 1, cfg.output_dim))).astype(np.float32) for k in ("nr", "nf")}
    out = {}
    try:
        with model.on_stream():
            if case["seq"] == REFUSE:
                out["refusals"] = _refusal(case, e, x, lab, ln)
                out["device_status"] = int(e.device_status())
                return out
            other = torch.cuda.Stream(device=e.device)

            def call(op, o):
                if op == "d":
                    return e.d_backward(x, lab, ln, noise["nr"] if o["nr"] else None, noise["nf"] if o["nf"] else None, train=o["train"],
                                        apply=o["apply"] and o["train"])
                return e.g_backward(x, lab, ln, noise["nf"] if o["nf"] else None, train=o["train"], reuse=o["reuse"],
                                    apply=o["apply"] and o["train"])
            calls = []
            for _ in range(3):                       # eager, captured, replayed
                for op, o in case["seq"]:
                    if op in ("d", "g"):
                        calls.append(_bits(call(op, o)))
                    elif op == "wait":
                        for i in range(len(e.grad_buckets(o))):
                            _lib.check(e.lib.rsrgan_grad_bucket_wait(e.h, o, i, C.c_void_p(other.cuda_stream)))
                        other.synchronize()
                    else:
                        e.apply(o)
            out["calls"] = calls
            nets = (NET_G,) if case["flags"] & SUPERVISED else (NET_G, NET_D)
            state = {}
            for net in nets:
                for what in ("variables", "adam_m", "adam_v", "ema"):
                    try:
                        state["%s_%s" % ("g" if net == NET_G else "d", what)] = _sha(e.get_params(net, what))
                    except _lib.RsrganError:
                        pass
            out["state_sha256"] = state
            if case["seq"][-1][0] in ("d", "g") and not case["seq"][-1][1]["apply"]:
                out["grads_sha256"] = {"g" if net == NET_G else "d": _sha(e.get_grads(net)) for net in nets}
            # one more pass of the first D-run and the first G-run of the sequence, profiled (eager): which recurrence launches ran
            e.profile_begin()
            for want in ("d", "g"):
                first = [o for op, o in case["seq"] if op == want][:1]
                if first:
                    call(want, first[0])
            kinds = [int(e.profile_read_kind(k)[0]) for k in range(1, 9)]
            out["profile_flops"] = [float(e.profile_read_kind(k)[2]) for k in (1, 2)]
            k0 = e.profile_read_kind(0)
            out["profile_kinds"] = [int(k0[0])] + kinds
            out["profile_flops"].insert(0, float(k0[2]))
            out["profile_launches"] = int(e.profile_launches())
            out["device_status"] = int(e.device_status())
        return out
    finally:
        e.close()


def worker_main(group):
    out = {}
    for case in group_cases(group):
        try:
            out[case["name"]] = run_case(case)
        except Exception:                             # (reported per case: the test and the recorder refuse a record with an error)
            import traceback
            out[case["name"]] = {"error": traceback.format_exc()}
            err = sys.exc_info()[1]
            host_only = isinstance(err, (AssertionError, TypeError, ValueError, KeyError, AttributeError, IndexError)) or \
                str(err).startswith(("librsrgan_hip error -1:", "librsrgan_hip error -4:"))      # (a refused call: nothing was launched)
            if not host_only:
                break                                 # (possibly the device: nothing more is started on it from this process)
    print("RESULT " + json.dumps(out))


def run_group(group, timeout=600):
    """the cases of `group` in a fresh process under the group's environment -> {case name: record}"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSRGAN_")}
    env["RSRGAN_DPIPE"] = "0"          # (the Python layer's default is the pipelined D-run: the DPIPE groups set it themselves)
    env.update(group_cases(group)[0]["env"])
    src = "import sys; sys.path.insert(0, %r); from tests.step_cases import worker_main; worker_main(%r)" % (ROOT, group)
    p = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, env=env, cwd=ROOT, timeout=timeout)
    assert p.returncode == 0, (group, p.stdout[-1000:], p.stderr[-3000:])
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
