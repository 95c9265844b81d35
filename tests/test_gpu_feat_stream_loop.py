"""The live multi-stream decode on the device: StreamBank(device_features=True) -- the ring, rsrgan_feat_stream, the stateful forward,
rsrgan_feat_denorm -- against StreamBank(device_features=False) on the SAME handle with the same schedule.  The front end gives the host
path's bits, the forward is deterministic and the de-normalising gives NumPy's bits, so the two make the same forward_stream calls and
return EQUAL bytes per row, with and without CMVN.  Truth is the fp64 oracle on the whole utterance (tests/test_gpu_stream.py's bound for
the small nets).  Then StreamEnhancer(device_features=True) against its host path, and run_gan_rnn --decode --device_features against
the same command with the de-normalising done on the host (the arithmetic before rsrgan_feat_denorm existed): the same bytes."""
import numpy as np
import pytest

from oracle import rsrgan_oracle as O
from rsrgan_amd.io import splice_feats
from rsrgan_amd.stream import StreamBank, StreamEnhancer
from tests import feat_ref
from tests.helpers import build_hip_pair, overrides, rand_params, small_cfg
from tests.test_gpu_stream import LOSS_RTOL, l1

pytestmark = pytest.mark.gpu

RAW_DIM, CHUNK, SEED = 3, 5, 91


def _pair(left, right):
    cfg = small_cfg("lstm", input_dim=RAW_DIM * (left + 1 + right), output_dim=4)
    model, _ = build_hip_pair(cfg, 4, 8, seed=SEED, flags=1)
    g, d = rand_params(cfg, SEED)
    return cfg, model, O.GanRnnOracle(cfg, g, d, batch_size=1)


def _schedule(rng, streams=3):
    """two utterances per row, cut into pushes of [0, 12) frames: a list of steps {row: frames}, with the rows whose utterance ends there"""
    utts = {r: [(rng.standard_normal((int(T), RAW_DIM)) * 2 + 1).astype(np.float32) for T in rng.integers(9, 41, 2)] for r in range(streams)}
    pos, which, steps = {r: 0 for r in utts}, {r: 0 for r in utts}, []
    while which:
        push, ended = {}, []
        for r in list(which):
            x = utts[r][which[r]]
            n = int(rng.integers(0, 12))
            push[r] = x[pos[r]:pos[r] + n]
            pos[r] += n
            if pos[r] >= x.shape[0]:
                ended.append(r)
                pos[r] = 0
                which[r] += 1
                if which[r] == len(utts[r]):
                    del which[r]
        steps.append((push, ended))
    return utts, steps


def _run(bank, steps, streams=3):
    """every utterance's output per row, the concatenation of what push and flush returned for it"""
    done, cur = {r: [] for r in range(streams)}, {r: [] for r in range(streams)}
    for push, ended in steps:
        for r, y in bank.push(push).items():
            cur[r].append(y)
        for r, y in (bank.flush(ended) if ended else {}).items():
            done[r].append(np.concatenate(cur[r] + [y], 0))
            cur[r] = []
    return done


def _recorded(model):
    calls, real = [], model.forward_stream

    def forward_stream(inputs, lengths, reset=None):
        ln = lengths.cpu().numpy() if hasattr(lengths, "cpu") else np.asarray(lengths)
        calls.append((int(inputs.shape[1]), tuple(int(v) for v in ln), tuple(reset or ())))
        return real(inputs, lengths, reset=reset)
    model.forward_stream = forward_stream
    return calls


@pytest.mark.parametrize("with_cmvn", [True, False], ids=["cmvn", "raw"])
@pytest.mark.parametrize("left,right", [(2, 3), (0, 0)])
def test_device_bank_equals_host_bank_and_the_oracle(left, right, with_cmvn):
    cfg, model, oracle = _pair(left, right)
    rng = np.random.default_rng(10 * left + right + (100 if with_cmvn else 0))
    cmvn = feat_ref.cmvn_for(rng, RAW_DIM, 4) if with_cmvn else None
    utts, steps = _schedule(rng)
    calls = _recorded(model)
    results = []
    for dev in (False, True):
        bank = StreamBank(model, cmvn, left, right, chunk=CHUNK, streams=3, device_features=dev)
        assert bank.ring_frames == left + CHUNK + right
        n0 = len(calls)
        results.append((_run(bank, steps), calls[n0:], dict(bank.counters)))
    (host, host_calls, host_n), (devc, dev_calls, dev_n) = results
    assert host_calls == dev_calls and len(dev_calls) > 6                 # the same forward_stream calls ...
    assert all(T <= CHUNK and ln[3] == 0 for T, ln, _ in dev_calls)
    assert any(sum(v > 0 for v in ln) > 1 for _, ln, _ in dev_calls)      # ... in which rows advance side by side
    for r in range(3):
        assert len(host[r]) == len(devc[r]) == 2
        for u, a, b in zip(utts[r], host[r], devc[r]):                    # ... and the same bytes
            assert a.shape == b.shape == (u.shape[0], 4) and a.dtype == b.dtype == (np.float64 if with_cmvn else np.float32)
            assert a.tobytes() == b.tobytes(), (r, u.shape[0], int((a != b).sum()))
            x = u.astype(np.float64)
            if cmvn is not None:
                x = (x - cmvn["mean_inputs"]) / cmvn["stddev_inputs"]
            x = splice_feats(x, left, right).astype(np.float32)
            want = oracle.forward(x[None].astype(np.float64), np.array([x.shape[0]], np.int32))[0]
            # (the bound is stated for G(x) itself: the de-normalising, one product and one sum in fp64, is undone in fp64)
            y = (b - cmvn["mean_labels"]) / cmvn["stddev_labels"] if cmvn is not None else b
            err = l1(y, want)
            assert err < LOSS_RTOL, (r, u.shape[0], err)
    # the device path moved the packed raw frames and the tables up, and exactly each row's k x output_dim values down
    frames = sum(u.shape[0] for r in utts for u in utts[r])
    assert dev_n["rounds"] == host_n["rounds"] and dev_n["calls"] == host_n["calls"] == len(dev_calls)
    assert dev_n["bytes_down"] == frames * 4 * (8 if with_cmvn else 4)
    assert dev_n["bytes_up"] == frames * RAW_DIM * 4 + dev_n["rounds"] * 4 * 6 * 4
    if left + right > 0:
        assert dev_n["bytes_up"] < host_n["bytes_up"]
    assert model.engine.device_status() == 0


def test_stream_enhancer_device_features_equals_its_host_path():
    left, right = 2, 3
    cfg, model, _ = _pair(left, right)
    rng = np.random.default_rng(17)
    cmvn = feat_ref.cmvn_for(rng, RAW_DIM, 4)
    u = (rng.standard_normal((37, RAW_DIM)) * 2 + 1).astype(np.float32)
    cuts = [0, 4, 4, 15, 16, 30, 37]
    outs = []
    for dev in (False, True):
        enh = StreamEnhancer(model, cmvn, left, right, chunk=CHUNK, device_features=dev)
        got = [enh.push(u[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        assert sum(o.shape[0] for o in got) == 37 - right
        outs.append(np.concatenate(got + [enh.flush()], 0))
        assert enh.flush().shape == (0, 4)
    assert outs[0].shape == outs[1].shape == (37, 4) and outs[0].dtype == outs[1].dtype == np.float64
    # with the switch the enhancer is a one-row bank: the bytes of the one-row bank's host path, which makes the same calls
    bank = StreamBank(model, cmvn, left, right, chunk=CHUNK, streams=1)
    ref = np.concatenate([bank.push({0: u[a:b]})[0] for a, b in zip(cuts[:-1], cuts[1:])] + [bank.flush()[0]], 0)
    assert outs[1].tobytes() == ref.tobytes(), int((outs[1] != ref).sum())
    # the enhancer's own host path cuts the same pushes into OTHER forward calls (it takes a push in at once, a bank in rounds), and the
    # fp32 forward may round differently under another cut.  Each cut is within LOSS_RTOL of the fp64 whole-utterance result
    # (tests/test_gpu_stream.py), so the two are within twice that of each other, in the same measure on G(x) itself
    g = [(o - cmvn["mean_labels"]) / cmvn["stddev_labels"] for o in outs]
    assert l1(g[1], g[0]) < 2 * LOSS_RTOL, l1(g[1], g[0])
    assert model.engine.device_status() == 0


@pytest.mark.parametrize("extra", [[], ["--decode_chunk", "3", "--decode_streams", "2"], ["--decode_chunk", "3", "--decode_streams", "2", "--decode_push", "4"]],
                         ids=["whole", "chunked", "push"])
def test_decode_device_features_writes_the_bytes_of_the_host_denormalise(tmp_path, monkeypatch, extra):
    import torch
    from rsrgan_amd import GAN_RNN
    from rsrgan_amd import run_gan_rnn as G
    from rsrgan_amd.engine_hip import HipEngine
    left, right = 2, 1
    cfg = small_cfg("lstm")
    rng = np.random.default_rng(33)
    te = feat_ref.write_arks(tmp_path, "te", [7, 4, 10, 1, 6], cfg.input_dim, cfg.output_dim, rng)
    np.savez(tmp_path / "train_cmvn.npz", **feat_ref.cmvn_for(rng, cfg.input_dim, cfg.output_dim))
    base = ["--decode", "--data_dir", str(tmp_path), "--test_inputs_scp", te[0], "--input_dim", str(cfg.input_dim), "--output_dim",
            str(cfg.output_dim), "--left_context", str(left), "--right_context", str(right), "--save_dir", str(tmp_path / "exp"),
            "--max_frames", "16", "--g_type", "lstm", "--device_features"] + extra
    ov = overrides(cfg)
    FLAGS = G.build_parser().parse_args(base)
    GAN_RNN(None, FLAGS, ["gpu:0"], max_frames=16, net_overrides=ov).save(FLAGS.save_dir, 1)
    launches, real = [], HipEngine.op_feat_denorm

    def counted(self, *a, **k):
        launches.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(HipEngine, "op_feat_denorm", counted)
    scp = G.decode(FLAGS, log=lambda s: None, net_overrides=ov)
    device = (open(scp, "rb").read(), open(scp[:-4] + ".ark", "rb").read())
    assert len(launches) >= 5                                             # the kernel did run

    def host_denormalize(self, y, mean, stddev, lengths=None):           # NumPy on the float32 copy: what decode computed before
        out = y.detach().cpu().numpy() * stddev + mean
        if lengths is not None:
            for b, n in enumerate(lengths.cpu().tolist()):
                out[b, n:] = 0.0
        return torch.from_numpy(out)
    monkeypatch.setattr(HipEngine, "denormalize", host_denormalize)
    n0 = len(launches)
    scp = G.decode(FLAGS, log=lambda s: None, net_overrides=ov)
    assert len(launches) == n0
    host = (open(scp, "rb").read(), open(scp[:-4] + ".ark", "rb").read())
    assert len(host[1]) > 5 * 4 * cfg.output_dim and host[0].count(b"\n") == 5
    assert device == host
