#!/usr/bin/env python
"""Outer loop of the sequence-level GAN recipe: scripts/train_gan_rnn_placeholder.py:204-584 (decode, train,
main) and stage 2-3 of run_gan_rnn_placeholder.sh, with Kaldi scp/ark files instead of TFRecords.

    python -m rsrgan_amd.run_gan_rnn --data_dir data/train --tr_inputs_scp tr/inputs.scp --tr_labels_scp tr/labels.scp \\
        --cv_inputs_scp cv/inputs.scp --cv_labels_scp cv/labels.scp --g_type res_lstm_l --batch_size 8 --save_dir exp/x
    python -m rsrgan_amd.run_gan_rnn --decode --test_inputs_scp test/inputs.scp --data_dir data/train --save_dir exp/x

Multi-GPU: launch with `python -m torch.distributed.run --nproc-per-node N -m rsrgan_amd.run_gan_rnn ...`; each batch of
batch_size*num_gpu utterances is sliced per rank (models/gan_rnn_placeholder.py:157-159), LR x num_gpu (:458-459).
Flag names and defaults are the reference's (train_gan_rnn_placeholder.py:587-747); the *_list_file flags (lists of
TFRecord files) are replaced by *_inputs_scp / *_labels_scp."""
from __future__ import annotations

import argparse
import datetime
import os
import sys

import numpy as np

from . import dist as rdist
from .gan_rnn import GAN_RNN
from .io import ArkReader, ArkWriter, PaddedBatchReader, pack_coded, pack_utterances, pack_wave, prefetch, splice_feats
from .train import eval_one_iteration, exponential_decay, train_one_iteration


def str2bool(v):
    return str(v).lower() in ("yes", "true", "t", "1")


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--decode", default=False, action="store_true", help="Flag indicating decoding or training.")
    p.add_argument("--data_dir", type=str, default=None, help="Data directory (holds train_cmvn.npz).")
    for n in ("tr_inputs_scp", "tr_labels_scp", "cv_inputs_scp", "cv_labels_scp", "test_inputs_scp"):
        p.add_argument("--" + n, type=str, default=None)
    p.add_argument("--input_dim", type=int, default=257)
    p.add_argument("--output_dim", type=int, default=40)
    p.add_argument("--left_context", type=int, default=5)
    p.add_argument("--right_context", type=int, default=5)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--g_learning_rate", type=float, default=0.0003)
    p.add_argument("--d_learning_rate", type=float, default=0.001)
    p.add_argument("--min_epoches", type=int, default=25)
    p.add_argument("--max_epoches", type=int, default=30)
    p.add_argument("--end_improve", type=float, default=0.001)
    p.add_argument("--num_threads", type=int, default=24)
    p.add_argument("--save_dir", type=str, default="exp/gan_rnn")
    p.add_argument("--init_mse_weight", type=float, default=1.0)
    p.add_argument("--g_type", type=str, default="lstm")
    p.add_argument("--disc_updates", type=int, default=1)
    p.add_argument("--gen_updates", type=int, default=2)
    p.add_argument("--batch_norm", type=str2bool, nargs="?", default="false")
    p.add_argument("--keep_prob", type=float, default=1.0)
    p.add_argument("--init_disc_noise_std", type=float, default=0.0)
    p.add_argument("--l2_scale", type=float, default=0.00001)
    p.add_argument("--num_gpu", type=int, default=1)
    p.add_argument("--apply_cmvn", type=str2bool, nargs="?", default="true", help="normalise with data_dir/train_cmvn.npz "
                   "(make_tfrecords.py:84-87 did this when writing TFRecords)")
    p.add_argument("--max_frames", type=int, default=3000, help="capacity of the padded time axis")
    p.add_argument("--decode_chunk", type=int, default=0, help="decode: frames per forward call; > 0 decodes utterances of any length "
                   "in chunks that carry the generator's state (0: one whole utterance per call, at most max_frames)")
    p.add_argument("--decode_streams", type=int, default=1, help="decode with --decode_chunk: utterances decoded side by side, one per "
                   "batch row")
    p.add_argument("--decode_lean", default=False, action="store_true", help="decode on an inference-only model (inference_only=True: "
                   "the generator alone, no BPTT stash)")
    p.add_argument("--decode_push", type=int, default=0, help="decode with --decode_chunk: the live path -- every utterance arrives as pushes "
                   "of this many raw frames through a StreamBank of --decode_streams rows (0: off)")
    p.add_argument("--device_features", type=str2bool, nargs="?", const=True, default=False, help="CMVN, context splice and padding on the "
                   "device (csrc/feat.hip): the reader ships packed raw frames and an offset table instead of the expanded batch; "
                   "training, cross-validation and --decode; the same numbers bit for bit")
    p.add_argument("--device_summaries", type=str2bool, nargs="?", const=True, default=False, help="the TensorBoard histograms of the "
                   "training and cross-validation summaries are computed on the device (csrc/hist.hip) and the discriminator's logits get "
                   "theirs (d_real, d_fake); off: three histograms computed on the host")
    p.add_argument("--device_decode", type=str2bool, nargs="?", const=True, default=False, help="implies --device_features, and the archive "
                   "is decoded on the device as well (csrc/feat.hip k_feat_decode): the reader ships each matrix's bytes as the file holds "
                   "them -- float, double or Kaldi-compressed -- with no host decode; training, cross-validation and --decode; the same "
                   "numbers bit for bit")
    p.add_argument("--wav_scp", type=str, default=None, help="decode: read AUDIO instead of --test_inputs_scp -- lines `utt path` naming "
                   "16-bit PCM wav files at 16 kHz; the log-power-spectrum frames (io/wave.py: 400 samples every 160, Hamming, 257 bins) are "
                   "computed on the host, or with --device_features on the device (csrc/wave.hip); with --decode_push K the live path is "
                   "driven by pushes of K x 160 samples")
    for n in ("tr_inputs_wav_scp", "tr_labels_wav_scp", "cv_inputs_wav_scp", "cv_labels_wav_scp"):
        p.add_argument("--" + n, type=str, default=None, help="train from AUDIO: a wav.scp (lines `utt path`, 16-bit PCM at 16 kHz) in place "
                       "of the split's *_scp archive; inputs become 257-bin log-power-spectrum frames, labels 40-dim MFCC frames "
                       "(io/wave.py MfccSpec: compute-mfcc-feats with mfcc_hires.conf), on the host, or with --device_features on the "
                       "device (csrc/wave.hip); given in pairs")
    add_audio_out_flags(p)
    from .io.reverb import add_sim_flags
    add_sim_flags(p)
    return p


def add_audio_out_flags(p):
    """--label_kind and --wav_out, shared by the two sequence recipes"""
    p.add_argument("--label_kind", type=str, default="mfcc", choices=("mfcc", "lps"), help="train from AUDIO: the labels' features -- mfcc "
                   "(40-dim MFCC, io/wave.py MfccSpec) or lps (the inputs' 257-bin log-power-spectrum framing: the targets a model needs "
                   "for --wav_out); --output_dim must be the kind's bins")
    p.add_argument("--wav_out", type=str, default=None, help="decode with --wav_scp and --output_dim 257: besides feats.ark, every utterance's "
                   "de-normalised output goes back to samples against its own input audio (the enhanced magnitude, the input's phase, "
                   "overlap-add, de-emphasis: io/wave.py wave_from_lps; with --device_features on the device, csrc/synth.hip) and is "
                   "written as DIR/<utt>.wav, listed in DIR/wav.scp")


def label_spec(FLAGS):
    """the framing of the labels made from audio: --label_kind"""
    from .io import wave as W
    return W.DEFAULT if getattr(FLAGS, "label_kind", "mfcc") == "lps" else W.MFCC_DEFAULT


class _WavSink(object):
    """--wav_out: every utterance's de-normalised output matrix -> DIR/<utt>.wav and a line of DIR/wav.scp.  engine: a HipEngine for
    the device route (HipEngine.synthesize), None for the host route (io.wave.wave_from_lps)."""

    def __init__(self, out_dir, source, engine=None):
        self.dir, self.source, self.engine = out_dir, source, engine
        os.makedirs(out_dir, exist_ok=True)
        self.scp = open(os.path.join(out_dir, "wav.scp"), "w")

    def write(self, i, lps):
        """lps: utterance i's [T, bins] matrix, a host array or a device tensor"""
        W, utt = self.source.W, self.source.utt_ids[i]
        x = self.source.read_samples(i)
        if self.engine is not None:
            out, _ = self.engine.synthesize(W.pack_wave([x], spec=self.source.spec, names=[utt]), lps)
            self.engine.upload_stream().synchronize()
            y = out.cpu().numpy()
        else:
            y = W.wave_from_lps(lps.detach().cpu().numpy() if hasattr(lps, "detach") else np.asarray(lps), x, self.source.spec)
        path = os.path.join(self.dir, utt + ".wav")
        W.write_wav(path, W.quantize_pcm(y), self.source.spec.sample_rate)
        self.scp.write("%s %s\n" % (utt, path))

    def close(self):
        self.scp.close()


class _WavSource(object):
    """--wav_scp: the utterances of a wav.scp behind the two members decode uses of an ArkReader (utt_ids, read_utt_data_from_index: here
    the host route's frames), and the samples themselves for the device route and the live path"""

    def __init__(self, path, input_dim):
        from .io import wave as W
        self.W, self.spec = W, W.DEFAULT
        if int(input_dim) != self.spec.bins:
            raise SystemExit("--wav_scp makes frames of %d bins; --input_dim is %d" % (self.spec.bins, int(input_dim)))
        try:
            self.items = W.read_wav_scp(path)
        except (OSError, ValueError) as e:
            raise SystemExit("--wav_scp: %s" % e)
        self.utt_ids = [u for u, _ in self.items]

    def read_samples(self, i):
        utt, path = self.items[i]
        try:
            x = self.W.read_wav(path, sample_rate=self.spec.sample_rate)
        except (OSError, EOFError, ValueError, self.W._wave.Error) as e:
            raise SystemExit("--wav_scp: %s: %s" % (utt, e))
        if self.W.num_frames(x.shape[0], self.spec) < 1:
            raise SystemExit("--wav_scp: %s: %d samples make no frame of %d" % (utt, x.shape[0], self.spec.frame_length))
        return x

    def read_utt_data_from_index(self, i):
        return self.W.lps_from_wave(self.read_samples(i), spec=self.spec)


def _device_decode(FLAGS):
    return bool(getattr(FLAGS, "device_decode", False))


def _device_features(FLAGS):
    return bool(getattr(FLAGS, "device_features", False)) or _device_decode(FLAGS)


def _cmvn(FLAGS):
    if not str2bool(FLAGS.apply_cmvn):
        return None
    path = os.path.join(FLAGS.data_dir or ".", "train_cmvn.npz")
    if not os.path.isfile(path):
        raise SystemExit("%s not exist, exit now." % path)                 # train_gan_rnn_placeholder.py:256-260
    return np.load(path)


def check_wav_flags(FLAGS):
    """the *_wav_scp flags come in pairs, replace the split's archive flags and do not go with --device_decode; the two dims are the
    specs' bins.  --{tr,cv}_rir_scp takes the place of the split's --*_inputs_wav_scp (the inputs are simulated from the labels' audio);
    --noise_scp goes with it only.  SystemExit with a message otherwise."""
    from .io import wave as W
    any_wav = any_rir = False
    for split in ("tr", "cv"):
        a, b = (getattr(FLAGS, "%s_%s_wav_scp" % (split, k), None) for k in ("inputs", "labels"))
        rir = getattr(FLAGS, split + "_rir_scp", None)
        if rir and a:
            raise SystemExit("--%s_rir_scp simulates the inputs from the labels' audio in place of --%s_inputs_wav_scp: give one of them" % (split, split))
        if rir and not b:
            raise SystemExit("--%s_rir_scp needs --%s_labels_wav_scp: the clean audio it reverberates" % (split, split))
        any_rir = any_rir or bool(rir)
        a = a or rir
        if bool(a) != bool(b):
            raise SystemExit("--%s_inputs_wav_scp and --%s_labels_wav_scp are given together or not at all" % (split, split))
        if a and (getattr(FLAGS, split + "_inputs_scp", None) or getattr(FLAGS, split + "_labels_scp", None)):
            raise SystemExit("--%s_*_wav_scp reads audio in place of --%s_inputs_scp / --%s_labels_scp: give one kind per split" % (
                split, split, split))
        any_wav = any_wav or bool(a)
    if getattr(FLAGS, "noise_scp", None) and not any_rir:
        raise SystemExit("--noise_scp adds noise to simulated inputs: it goes with --tr_rir_scp / --cv_rir_scp")
    if any_rir and not float(getattr(FLAGS, "snr_lower", 5.0)) <= float(getattr(FLAGS, "snr_upper", 20.0)):
        raise SystemExit("--snr_lower %g is above --snr_upper %g" % (FLAGS.snr_lower, FLAGS.snr_upper))
    if any_wav and _device_decode(FLAGS):
        raise SystemExit("--*_wav_scp reads audio, --device_decode decodes archives: use --device_features for the device route")
    labels = label_spec(FLAGS)                                              # (--label_kind: MFCC_DEFAULT unless it says lps)
    if any_wav and (int(FLAGS.input_dim) != W.DEFAULT.bins or int(FLAGS.output_dim) != labels.bins):
        raise SystemExit("--*_wav_scp makes input frames of %d bins and label frames of %d; --input_dim is %d, --output_dim is %d" % (
            W.DEFAULT.bins, labels.bins, int(FLAGS.input_dim), int(FLAGS.output_dim)))


def split_reader(FLAGS, split, cmvn, shuffle, seed):
    """the reader of a split ("tr" / "cv"): over its two wav.scp files if they are given, over its two archives otherwise"""
    wav, rir = getattr(FLAGS, split + "_inputs_wav_scp", None), getattr(FLAGS, split + "_rir_scp", None)
    if wav or rir:
        from .io.reverb import sim_from_flags
        from .io.wave_reader import WaveBatchReader
        try:
            return WaveBatchReader(wav or None, getattr(FLAGS, split + "_labels_wav_scp"), FLAGS.batch_size * FLAGS.num_gpu, FLAGS.left_context,
                                   FLAGS.right_context, cmvn=cmvn, shuffle=shuffle, seed=seed, device_features=_device_features(FLAGS),
                                   label_spec=label_spec(FLAGS), simulate=sim_from_flags(FLAGS, split) if rir else None)
        except (OSError, EOFError, ValueError) as e:
            raise SystemExit("--%s_*_wav_scp: %s" % (split, e))
    return _reader(FLAGS, getattr(FLAGS, split + "_inputs_scp"), getattr(FLAGS, split + "_labels_scp"), cmvn, shuffle, seed)


def _reader(FLAGS, inputs_scp, labels_scp, cmvn, shuffle, seed):
    return PaddedBatchReader(inputs_scp, labels_scp, FLAGS.batch_size * FLAGS.num_gpu, FLAGS.left_context, FLAGS.right_context,
                             cmvn=cmvn, shuffle=shuffle, seed=seed, device_features=_device_features(FLAGS), device_decode=_device_decode(FLAGS))


def get_num_batch(reader, full):
    """get_num_batch (:346-385) counts the batches of a full pass; the reader's plan() gives the same count from the archive
    headers alone (no utterance is read, normalised, spliced or padded just to be counted)."""
    return sum(1 for _ in reader.plan())


def train(FLAGS, model_factory=None, log=print, net_overrides=None):
    """train (:388-584) + the batch counting of main (:305-343).  Returns the list of per-iteration CV g_loss."""
    check_wav_flags(FLAGS)
    cmvn = _cmvn(FLAGS)
    mk = model_factory or (lambda cv, share: GAN_RNN(None, FLAGS, ["gpu:%d" % rdist.rank()], cross_validation=cv,
                                                      max_frames=FLAGS.max_frames, share_engine_from=share,
                                                      net_overrides=net_overrides))
    tr_model = mk(False, None)
    cv_model = mk(True, tr_model)                                          # shares variables (:436-437)
    if tr_model.load(tr_model.save_dir, moving_average=False):
        log("[*] Load SUCCESS")
    else:
        log("[!] Begin a new model.")
    full = FLAGS.batch_size * FLAGS.num_gpu
    tr_reader = split_reader(FLAGS, "tr", cmvn, True, 1234)
    cv_reader = split_reader(FLAGS, "cv", cmvn, False, None)
    tr_num_batch = get_num_batch(split_reader(FLAGS, "tr", None, False, None), full)
    cv_num_batch = get_num_batch(split_reader(FLAGS, "cv", None, False, None), full)
    train_batch_per_iter, valdi_batch_per_iter = tr_num_batch, cv_num_batch
    min_iters = int(FLAGS.min_epoches * tr_num_batch / train_batch_per_iter)
    max_iters = int(FLAGS.max_epoches * tr_num_batch / train_batch_per_iter)
    log("LOG: #train_batch = {}, #valid_batch = {}, #min_iters = {}, #max_iters = {}".format(tr_num_batch, cv_num_batch, min_iters, max_iters))

    g_loss_prev, g_rel_impr, check_interval, windows_g_loss = 10000.0, 1.0, 1, []           # :452-456
    tr_model.g_learning_rate = FLAGS.num_gpu * FLAGS.g_learning_rate                         # :458-461
    tr_model.d_learning_rate = FLAGS.num_gpu * FLAGS.d_learning_rate
    history = []
    iteration = -1
    for iteration in range(max_iters):
        start = datetime.datetime.now()
        # reader thread + Queue(32) as :463-478: reading, CMVN, splicing and padding overlap the GPU steps
        if hasattr(tr_reader, "set_epoch"):
            tr_reader.set_epoch(iteration)                # (--tr_rir_scp: other rooms every epoch; cross-validation keeps epoch 0's)
        tr = train_one_iteration(None, tr_model, train_batch_per_iter * FLAGS.num_gpu, iteration + 1, prefetch(tr_reader), FLAGS.num_gpu)
        if hasattr(tr_model, "sync_batch_norm_state"):
            tr_model.sync_batch_norm_state()           # one copy of the batch-norm statistics over the ranks, before cross-validation and the checkpoint
        cv = eval_one_iteration(None, cv_model, valdi_batch_per_iter * FLAGS.num_gpu, iteration + 1,
                                prefetch(b for b in cv_reader if len(b[0]) == full), FLAGS.num_gpu)
        end = datetime.datetime.now()
        log("{}/{} (INFO): d_learning_rate = {:.5e}, g_learning_rate = {:.5e}, time = {:.3f} h\n"
            "{}/{} (TRAIN AVG.LOSS): d_rl_loss = {:.5f}, d_fk_loss = {:.5f}, d_loss = {:.5f}, g_adv_loss = {:.5f}, "
            "g_mse_loss = {:.5f}, g_l2_loss = {:.3e}, g_loss = {:.5f}\n"
            "{}/{} (CROSS AVG.LOSS): d_rl_loss = {:.5f}, d_fk_loss = {:.5f}, d_loss = {:.5f}, g_adv_loss = {:.5f}, "
            "g_mse_loss = {:.5f}, g_l2_loss = {:.3e}, g_loss = {:.5f}".format(
                iteration + 1, max_iters, tr_model.d_learning_rate, tr_model.g_learning_rate, (end - start).total_seconds() / 3600.0,
                iteration + 1, max_iters, *tr, iteration + 1, max_iters, *cv))
        cv_g_loss = cv[6]
        history.append(cv_g_loss)
        # Start decay learning rate (:525-533)
        tr_model.g_learning_rate = exponential_decay(iteration + 1, FLAGS.num_gpu, min_iters, FLAGS.g_learning_rate)
        tr_model.d_learning_rate = exponential_decay(iteration + 1, FLAGS.num_gpu, min_iters, FLAGS.d_learning_rate)
        tr_model.disc_noise_std = exponential_decay(iteration + 1, FLAGS.num_gpu, min_iters, FLAGS.init_disc_noise_std,
                                                    multiply_jobs=False)
        windows_g_loss.append(cv_g_loss)
        # Accept or reject new parameters (:537-554)
        if (iteration + 1) % check_interval == 0:
            g_loss_new = float(np.mean(windows_g_loss))
            g_rel_impr = (g_loss_prev - g_loss_new) / g_loss_prev
            if g_rel_impr > 0.0:
                tr_model.save(tr_model.save_dir, iteration + 1)
                log("Iteration {}: Nnet Accepted. Save model SUCCESS. g_loss_prev = {:.5f}, g_loss_new = {:.5f}".format(
                    iteration + 1, g_loss_prev, g_loss_new))
                g_loss_prev = g_loss_new
            else:
                log("Iteration {}: Nnet Rejected. g_loss_prev = {:.5f}, g_loss_new = {:.5f}".format(iteration + 1, g_loss_prev, g_loss_new))
            windows_g_loss = []
        # Stopping criterion (:557-562)
        if iteration + 1 > min_iters and (iteration + 1) % check_interval == 0 and g_rel_impr < FLAGS.end_improve:
            log("Iteration %d: Finished, too small relative G improvement %g" % (iteration + 1, g_rel_impr))
            break
    if windows_g_loss:                                                     # :570-581
        g_loss_new = float(np.mean(windows_g_loss))
        if (g_loss_prev - g_loss_new) / g_loss_prev > 0.0:
            tr_model.save(tr_model.save_dir, iteration + 1)
    log("Training Done.")
    return history


def decode(FLAGS, model_factory=None, log=print, net_overrides=None):
    """decode (:204-302): batch 1, G(x), de-normalise with the label CMVN, write feats.ark / feats.scp."""
    chunk, streams = int(getattr(FLAGS, "decode_chunk", 0) or 0), max(1, int(getattr(FLAGS, "decode_streams", 1) or 1))
    push = int(getattr(FLAGS, "decode_push", 0) or 0)
    if push < 0 or (push > 0 and chunk <= 0):
        raise SystemExit("--decode_push needs a positive value and --decode_chunk")
    # (--decode_chunk N: the handle holds N frames of `streams` rows; an utterance is a sequence of calls that carry the state)
    mk = model_factory or (lambda: GAN_RNN(None, argparse.Namespace(**dict(vars(FLAGS), batch_size=streams if chunk > 0 else 1)),
                                           ["gpu:%d" % rdist.rank()], cross_validation=True, infer=True,
                                           max_frames=chunk if chunk > 0 else FLAGS.max_frames, net_overrides=net_overrides,
                                           **({"inference_only": True} if getattr(FLAGS, "decode_lean", False) else {})))
    wav, wav_out = getattr(FLAGS, "wav_scp", None), getattr(FLAGS, "wav_out", None)
    if wav_out:
        from .io import wave as W
        if not wav or int(FLAGS.output_dim) != W.DEFAULT.bins:
            raise SystemExit("--wav_out needs --wav_scp (the audio whose phase it keeps) and --output_dim %d (LPS rows to synthesise from); "
                             "--wav_scp is %s, --output_dim is %d" % (W.DEFAULT.bins, wav or "not given", int(FLAGS.output_dim)))
        if push > 0:
            raise SystemExit("--wav_out does not go with --decode_push: the live path has no synthesis")
    model = mk()
    if model.load(model.save_dir, moving_average=False):
        log("[*] Load SUCCESS")
    else:
        raise SystemExit("[!] Load failed. Checkpoint not found. Exit now.")
    cmvn = _cmvn(FLAGS)
    out_dir = os.path.join(FLAGS.save_dir, "test")
    os.makedirs(out_dir, exist_ok=True)
    write_scp_path, write_ark_path = os.path.join(out_dir, "feats.scp"), os.path.join(out_dir, "feats.ark")
    if os.path.exists(write_ark_path):
        os.remove(write_ark_path)
    writer = ArkWriter(write_scp_path)
    if wav:
        # --wav_scp: audio instead of an archive of frames (training from audio: the --tr_*_wav_scp / --cv_*_wav_scp flags)
        if _device_decode(FLAGS):
            raise SystemExit("--wav_scp reads audio, --device_decode decodes archives: use --device_features for the device route")
        reader = _WavSource(wav, FLAGS.input_dim)
    else:
        reader = ArkReader()
        reader(FLAGS.test_inputs_scp)
    start = datetime.datetime.now()
    denorm = lambda a: a * cmvn["stddev_labels"] + cmvn["mean_labels"] if cmvn is not None else a
    sink = None
    if wav_out:
        engine = getattr(model, "engine", None) if _device_features(FLAGS) else None
        if _device_features(FLAGS) and getattr(engine, "synthesize", None) is None:
            raise SystemExit("--wav_out with --device_features needs an engine with device-side synthesis (HipEngine.synthesize)")
        sink = _WavSink(wav_out, reader, engine)

    def write_all(outs, post):
        """one matrix per utterance, in scp order"""
        for i, (utt, activations) in enumerate(zip(reader.utt_ids, outs)):
            matrix = post(np.asarray(activations))
            writer.write_next_utt(write_ark_path, utt, matrix)
            if sink is not None:
                sink.write(i, matrix)
            log("[{}/{}] Write inferred {} to {}".format(i + 1, len(reader.utt_ids), utt, write_ark_path))
        writer.close()
        if sink is not None:
            sink.close()
        log("Decoding time is {}s".format((datetime.datetime.now() - start).total_seconds()))
        return write_scp_path

    if push > 0:
        # --decode_push N: the live path.  The raw utterance arrives N frames at a time on one row of a StreamBank, which owns CMVN, the
        # splice and the de-normalising (on the device with --device_features)
        from .stream import StreamBank, decode_live
        try:
            bank = StreamBank(model, cmvn, FLAGS.left_context, FLAGS.right_context, chunk, streams,
                              device_features=bool(getattr(FLAGS, "device_features", False)))
        except ValueError as e:
            raise SystemExit("--decode_push: %s" % e)
        if wav:                                                              # pushes of N frames' worth of new samples
            from .stream import decode_live_audio
            return write_all(decode_live_audio(bank, (reader.read_samples(i) for i in range(len(reader.utt_ids))),
                                               push * reader.spec.frame_shift), lambda a: a)
        return write_all(decode_live(bank, (reader.read_utt_data_from_index(i) for i in range(len(reader.utt_ids))), push), lambda a: a)

    def features(i):
        x = reader.read_utt_data_from_index(i).astype(np.float64)
        if cmvn is not None:
            x = (x - cmvn["mean_inputs"]) / cmvn["stddev_inputs"]
        return splice_feats(x, FLAGS.left_context, FLAGS.right_context).astype(np.float32)

    host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    finish = None
    if _device_features(FLAGS):
        # --device_features: the raw utterance travels (--device_decode: its bytes as the archive holds them, decoded on the device), CMVN and the splice run on the device (HipEngine.featurize) and the generator reads
        # the device tensor; the same bits as features() above.  The output is de-normalised on the device as well (HipEngine.denormalize,
        # rsrgan_feat_denorm: the product and the sum rounded separately, NumPy's bits) and comes back as the float64 matrix that is written.
        featurize = getattr(getattr(model, "engine", None), "featurize", None)
        denormalize = getattr(getattr(model, "engine", None), "denormalize", None)
        if featurize is None or denormalize is None:
            raise SystemExit("--device_features needs an engine with a device-side front end (HipEngine.featurize, HipEngine.denormalize)")
        if cmvn is not None:
            label_stats = tuple(np.ascontiguousarray(cmvn[k], np.float64).reshape(-1) for k in ("mean_labels", "stddev_labels"))
            finish = lambda y: denormalize(y, *label_stats)
            denorm = lambda a: a                                             # (done where the activations were)
        stats = (None, None) if cmvn is None else tuple(np.ascontiguousarray(cmvn[k], np.float64).reshape(-1)
                                                        for k in ("mean_inputs", "stddev_inputs"))

        def features(i):                                                     # noqa: F811 -- [n, D * (L + 1 + R)] on the device
            if wav:                                                          # the samples travel; the frames are made on the device
                return featurize(pack_wave([reader.read_samples(i)], None, FLAGS.left_context, FLAGS.right_context, *stats,
                                           spec=reader.spec, names=[reader.utt_ids[i]]), limit=chunk <= 0)[0][0]
            if _device_decode(FLAGS):
                coded = pack_coded([reader.read_coded_from_index(i)], FLAGS.left_context, FLAGS.right_context, *stats, names=[reader.utt_ids[i]])
                return featurize(coded, limit=chunk <= 0)[0][0]
            packed = pack_utterances([reader.read_utt_data_from_index(i)], FLAGS.left_context, FLAGS.right_context, *stats,
                                     names=[reader.utt_ids[i]])
            return featurize(packed, limit=chunk <= 0)[0][0]                 # (chunked decode cuts the utterance itself)

    if chunk > 0:
        from .stream import decode_streams
        outs = decode_streams(model, (features(i) for i in range(len(reader.utt_ids))), chunk, streams, finish=finish)
        return write_all(outs, denorm)                                             # (in scp order, as the loop below writes them)
    for i, utt in enumerate(reader.utt_ids):
        x = features(i)[None]
        activations = model.forward(x, np.array([x.shape[1]], np.int32))
        activations = finish(activations) if finish is not None else activations
        on_device = sink is not None and sink.engine is not None and hasattr(activations, "detach")
        if on_device:
            sink.write(i, activations[0])                                    # (the de-normalised device tensor, before it comes back)
        sequence = denorm(host(activations))
        if sink is not None and not on_device:
            sink.write(i, np.vstack(sequence))
        writer.write_next_utt(write_ark_path, utt, np.vstack(sequence))
        log("[{}/{}] Write inferred {} to {}".format(i + 1, len(reader.utt_ids), utt, write_ark_path))
    writer.close()
    if sink is not None:
        sink.close()
    log("Decoding time is {}s".format((datetime.datetime.now() - start).total_seconds()))
    return write_scp_path


def main(argv=None):
    FLAGS, unparsed = build_parser().parse_known_args(argv)                # unknown flags are ignored, as in the reference (:748)
    rank, local, world = rdist.init_from_env()
    if world > 1:
        FLAGS.num_gpu = world
    if FLAGS.decode:
        rdist.run_on_rank0(lambda: decode(FLAGS))                          # one writer for <save_dir>/test/feats.{ark,scp}; a failure releases the others
    else:
        train(FLAGS)


if __name__ == "__main__":
    main()
