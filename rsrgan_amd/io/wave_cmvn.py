"""The global CMVN statistics of a training set given as AUDIO: the train_cmvn.npz the recipes load, from two wav.scp files.

    python -m rsrgan_amd.io.wave_cmvn --inputs_wav_scp tr/inputs_wav.scp --labels_wav_scp tr/labels_wav.scp --out data/train/train_cmvn.npz [--device]

Inputs become log-power-spectrum frames (io.wave.DEFAULT), labels MFCC frames (io.wave.MFCC_DEFAULT) or, with --label_kind lps, LPS
frames too.  Per dimension, sum x and sum x^2
over all frames are accumulated in float64; mean = sum x / n, stddev = sqrt(sum x^2 / n - mean^2), as the reference's
convert_cmvn_to_numpy.py computes them from Kaldi's statistics.  --device: the frames come from the two kernels of csrc/wave.hip and are
summed with float64 torch reductions on the device.  A dimension with zero variance is an error here, not a division by zero later.
--rir_scp (with --noise_scp, --snr_lower, --snr_upper, --sim_seed, as run_gan_rnn takes them) in place of --inputs_wav_scp: the inputs are
the labels' audio reverberated with epoch 0's draws (io/reverb.py; with --device on the device, csrc/reverb.hip)."""
from __future__ import annotations

import argparse

import numpy as np

from . import wave as W


def _finish(name, sx, sxx, n):
    if n < 1:
        raise ValueError("%s: no frames" % name)
    mean = sx / n
    var = sxx / n - mean * mean
    bad = np.flatnonzero(~(var > 0.0))
    if bad.shape[0]:
        raise ValueError("%s: dimension %d has no variance over the %d frames (sum x^2 / n - mean^2 = %g)" % (name, int(bad[0]), n, var[bad[0]]))
    return mean, np.sqrt(var)


def _host_sums(items, spec, featurize, simulate=None):
    sx, sxx, n = np.zeros(spec.bins), np.zeros(spec.bins), 0
    for i, (_, path) in enumerate(items):
        x = W.read_wav(path, sample_rate=spec.sample_rate)
        if simulate is not None:
            x = simulate.apply(x, simulate.draw(i, x.shape[0], epoch=0))
        f = featurize(x).astype(np.float64)
        sx += f.sum(0); sxx += (f * f).sum(0); n += f.shape[0]
    return sx, sxx, n


def _device_sums(items, spec, engine, batch=64, simulate=None):
    import torch
    sx = sxx = None
    n = 0
    us = engine.upload_stream()
    for lo in range(0, len(items), batch):
        utts = [W.read_wav(p, sample_rate=spec.sample_rate) for _, p in items[lo:lo + batch]]
        plan = simulate.plan(range(lo, lo + len(utts)), [u.shape[0] for u in utts], epoch=0) if simulate is not None else None
        wb = W.pack_wave(utts, spec=spec, plan=plan)
        rows = int(wb.offsets[-1])
        if rows < 1:
            continue
        with torch.cuda.stream(us):
            if plan is not None:
                pcm, dseg, _ = engine.simulate(wb, stream=us)
                f = engine.wave_rows(pcm, dseg, len(wb), wb.offsets, rows, spec, us)[0].double()
            else:
                f = engine.wave_features(wb.samples, wb.seg, wb.offsets, rows, spec, us)[0].double()
            a, b = f.sum(0), (f * f).sum(0)
            sx, sxx = (a, b) if sx is None else (sx + a, sxx + b)
        n += rows
    if sx is None:
        return np.zeros(spec.bins), np.zeros(spec.bins), 0
    us.synchronize()
    return sx.cpu().numpy(), sxx.cpu().numpy(), n


def wave_ops():
    """the waveform front end without a model: the handle-free entries on the current device (HipEngine's base class)"""
    from ..frontend import FrontEnd
    return FrontEnd()


def wave_cmvn(inputs_wav_scp, labels_wav_scp, engine=None, input_spec=W.DEFAULT, label_spec=W.MFCC_DEFAULT, simulate=None):
    """{mean_inputs, stddev_inputs, mean_labels, stddev_labels} (float64) over all frames of the two wav.scp files; engine: a HipEngine for
    the device route, None for the host route.  simulate (an io.reverb.ReverbSim, with inputs_wav_scp None): the inputs are the labels'
    audio reverberated with epoch 0's draws"""
    if (simulate is None) == (inputs_wav_scp is None):
        raise ValueError("the inputs come from inputs_wav_scp or from simulate on the labels' audio: give exactly one")
    ys = W.read_wav_scp(labels_wav_scp)
    xs = ys if simulate is not None else W.read_wav_scp(inputs_wav_scp)
    if engine is None:
        si = _host_sums(xs, input_spec, lambda s: W.lps_from_wave(s, spec=input_spec), simulate)
        label = (lambda s: W.mfcc_from_wave(s, label_spec)) if isinstance(label_spec, W.MfccSpec) else \
            (lambda s: W.lps_from_wave(s, spec=label_spec))
        sl = _host_sums(ys, label_spec, label)
    else:
        si, sl = _device_sums(xs, input_spec, engine, simulate=simulate), _device_sums(ys, label_spec, engine)
    mi, di = _finish("inputs", *si)
    ml, dl = _finish("labels", *sl)
    return {"mean_inputs": mi, "stddev_inputs": di, "mean_labels": ml, "stddev_labels": dl}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--inputs_wav_scp", default=None)
    p.add_argument("--rir_scp", default=None, help="in place of --inputs_wav_scp: simulate the inputs from the labels' audio (io/reverb.py)")
    p.add_argument("--noise_scp", default=None)
    p.add_argument("--snr_lower", type=float, default=5.0)
    p.add_argument("--snr_upper", type=float, default=20.0)
    p.add_argument("--sim_seed", type=int, default=0)
    p.add_argument("--labels_wav_scp", required=True)
    p.add_argument("--out", required=True, help="the .npz to write (the recipes read <data_dir>/train_cmvn.npz)")
    p.add_argument("--label_kind", default="mfcc", choices=("mfcc", "lps"), help="the labels' features: MFCC (default) or LPS (audio out)")
    p.add_argument("--device", default=False, action="store_true", help="make and sum the frames on the device")
    a = p.parse_args(argv)
    if bool(a.inputs_wav_scp) == bool(a.rir_scp):
        raise SystemExit("wave_cmvn: give --inputs_wav_scp or --rir_scp (the inputs simulated from the labels' audio), not both and not neither")
    if a.noise_scp and not a.rir_scp:
        raise SystemExit("wave_cmvn: --noise_scp goes with --rir_scp")
    engine = wave_ops() if a.device else None
    try:
        sim = None
        if a.rir_scp:
            from .reverb import ReverbSim, ReverbSpec
            sim = ReverbSim(a.rir_scp, a.noise_scp, ReverbSpec(snr=(a.snr_lower, a.snr_upper)), a.sim_seed)
        stats = wave_cmvn(a.inputs_wav_scp, a.labels_wav_scp, engine, label_spec=W.MFCC_DEFAULT if a.label_kind == "mfcc" else W.DEFAULT,
                          simulate=sim)
    except (OSError, EOFError, ValueError) as e:
        raise SystemExit("wave_cmvn: %s" % e)
    np.savez(a.out, **stats)
    return stats


if __name__ == "__main__":
    main()
