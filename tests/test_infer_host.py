"""Host side of the inference-only generator handle (no GPU): RSRGAN_FLAG_INFER and rsrgan_device_bytes in the header, the binding and
the cross-compiled library; GAN_RNN / RNNTrainer(inference_only=True) on a stand-in engine -- the training methods raise, load() reads
the generator's variables alone (their shadow names with moving_average) from a checkpoint a full model wrote; --decode_lean parses
and leaves decode() with a model_factory as it is."""
import os
import re

import numpy as np
import pytest

from rsrgan_amd import GAN_RNN, run_gan_rnn as R, run_rnn as RR
from rsrgan_amd.io import ArkWriter
from rsrgan_amd.trainer import RNNTrainer
from tests import stream_ref as SR
from tests.helpers import NET_D, NET_G, OracleEngine, args_for, rand_params, small_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_and_symbol_in_header_binding_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsrgan.h")).read(), flags=re.S)
    m = re.search(r"\bRSRGAN_FLAG_INFER\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == 64
    from rsrgan_amd import _lib
    assert _lib.FLAG_INFER == 64
    flags = [int(v) for n, v in re.findall(r"\b(RSRGAN_[A-Z_]+)\s*=\s*(\d+)", src) if n.split("_")[1] == "FLAG"]
    assert len(flags) >= 7 and len(flags) == len(set(flags)) and all(v & (v - 1) == 0 for v in flags)      # one bit each, none shared
    assert "rsrgan_device_bytes" in re.findall(r"\b(rsrgan_[a-z_0-9]+)\s*\(", src)
    assert "rsrgan_device_bytes" in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.rsrgan_device_bytes.argtypes
    assert lib.rsrgan_device_bytes(None, None) < 0 and b"null handle" in lib.rsrgan_last_error()


class RecordingEngine(OracleEngine):
    """the stand-in engine, noting every variable buffer a model writes or reads"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.sets, self.gets = [], []

    def set_params(self, net, flat, what="variables"):
        self.sets.append((net, what))
        return super().set_params(net, flat, what)

    def get_params(self, net, what="variables"):
        self.gets.append((net, what))
        return super().get_params(net, what)


def _models(tmp_path, cls=GAN_RNN, g_type="lstm"):
    cfg = small_cfg(g_type)
    B = 2
    g, d = rand_params(cfg, 3)
    args = args_for(cfg, B, save_dir=str(tmp_path / "exp"))
    full = cls(None, args, ["cpu:0"], engine=OracleEngine(cfg, g, d, B))
    # shadows and moments that differ from the variables, so that what load() read is visible
    for what, f in (("ema", 0.5), ("adam_m", 0.25), ("adam_v", 0.125)):
        full.engine.set_params(NET_G, full.engine.get_params(NET_G).numpy() * f, what)
    full.save(args.save_dir, 7)
    g0, d0 = rand_params(cfg, 4)                        # other values: load() has to bring the checkpoint's
    eng = RecordingEngine(cfg, g0, d0, B)
    lean = cls(None, args, ["cpu:0"], engine=eng, inference_only=True)
    return cfg, full, lean, eng


@pytest.mark.parametrize("cls", [GAN_RNN, RNNTrainer])
def test_training_methods_raise(tmp_path, cls):
    cfg, full, lean, eng = _models(tmp_path, cls)
    assert lean.inference_only and lean.cross_validation and not full.inference_only
    x = np.zeros((2, 3, cfg.input_dim), np.float32); lab = np.zeros((2, 3, cfg.output_dim), np.float32); ln = np.full(2, 3, np.int32)
    for call in (lambda: lean.d_step(x, lab, ln), lambda: lean.g_step(x, lab, ln), lambda: lean.g_step(x, lab, ln, train=False),
                 lambda: lean.save(str(tmp_path / "exp2"), 1)):
        with pytest.raises(RuntimeError) as ei:
            call()
        assert "inference-only" in str(ei.value) or "no discriminator" in str(ei.value), ei.value
    assert not os.path.exists(str(tmp_path / "exp2"))
    # forward is the engine's
    y = lean.forward(x, ln)
    assert y.shape == (2, 3, cfg.output_dim)
    with pytest.raises(ValueError):
        cls(None, args_for(cfg, 2), ["cpu:0"], share_engine_from=full, inference_only=True)


@pytest.mark.parametrize("moving_average", [False, True])
def test_load_reads_the_generator_variables_only(tmp_path, moving_average):
    cfg, full, lean, eng = _models(tmp_path)
    before_d = eng.get_params(NET_D).numpy().copy()
    before_m = eng.get_params(NET_G, "adam_m").numpy().copy()
    eng.sets.clear(); eng.gets.clear()
    assert lean.load(str(tmp_path / "exp"), moving_average=moving_average)
    assert eng.sets == [(NET_G, "variables")], eng.sets
    want = full.engine.get_params(NET_G, "ema" if moving_average else "variables").numpy()
    assert np.array_equal(eng.get_params(NET_G).numpy(), want)
    assert np.array_equal(eng.get_params(NET_D).numpy(), before_d)
    assert np.array_equal(eng.get_params(NET_G, "adam_m").numpy(), before_m)
    # a checkpoint without shadows: moving_average fails as it does on a full model, the plain load works
    data = dict(np.load(str(tmp_path / "exp" / "GAN_RNN-7.npz")))
    os.makedirs(str(tmp_path / "plain"))
    np.savez(str(tmp_path / "plain" / "GAN_RNN-7.npz"), **{k: v for k, v in data.items() if k.startswith("g_model") and "/Exponential" not in k and "/Adam" not in k})
    with open(str(tmp_path / "plain" / "checkpoint"), "w") as f:
        f.write('model_checkpoint_path: "GAN_RNN-7"\n')
    assert lean.load(str(tmp_path / "plain"), moving_average=moving_average) == (not moving_average)
    assert not full.load(str(tmp_path / "plain"), moving_average=True)


def test_decode_lean_parses_and_model_factory_decode_is_unaffected(tmp_path):
    for mod in (R, RR):
        F, _ = mod.build_parser().parse_known_args(["--decode"])
        assert F.decode_lean is False
        F, _ = mod.build_parser().parse_known_args(["--decode", "--decode_lean"])
        assert F.decode_lean is True
    rng = np.random.default_rng(9)
    din, dout = 3, 4
    w = ArkWriter(str(tmp_path / "te.scp"))
    for i, T in enumerate([5, 37, 1]):
        w.write_next_utt(str(tmp_path / "te.ark"), "utt%02d" % i, rng.standard_normal((T, din)) * 2 + 1)
    w.close()
    cfg = small_cfg("lstm", input_dim=din, output_dim=dout)
    g = {k: np.asarray(v, np.float64) for k, v in rand_params(cfg, 13)[0].items()}
    base = ["--decode", "--test_inputs_scp", str(tmp_path / "te.scp"), "--input_dim", str(din), "--output_dim", str(dout),
            "--left_context", "0", "--right_context", "0", "--apply_cmvn", "false"]
    arks, calls = [], []
    for name, extra in (("a", []), ("b", ["--decode_lean"])):
        F, _ = R.build_parser().parse_known_args(base + extra + ["--save_dir", str(tmp_path / name)])
        m = SR.RefStreamModel(cfg, g, 1, 3000, save_dir=F.save_dir)
        scp = R.decode(F, model_factory=lambda: m, log=lambda s: None)
        arks.append(open(os.path.join(os.path.dirname(scp), "feats.ark"), "rb").read())
        calls.append(list(m.calls))
    assert arks[0] == arks[1] and calls[0] == calls[1]
