#!/usr/bin/env python
"""Outer loop of the supervised sequence recipe: scripts/train_rnn.py:26-88,270-430 (train_one_iteration, eval_one_iteration, train,
main's batch counting) and stage 2-3 of run_rnn.sh, around RNNTrainer (models/rnn_trainer.py), with Kaldi scp/ark files instead of
TFRecords.  Generator-only MSE training: used on its own, and to pre-train the generator the GAN recipe then loads.

    python -m rsrgan_amd.run_rnn --data_dir data/train --tr_inputs_scp tr/inputs.scp --tr_labels_scp tr/labels.scp \\
        --cv_inputs_scp cv/inputs.scp --cv_labels_scp cv/labels.scp --g_type res_lstm_i --batch_size 8 --save_dir exp/rnn
    python -m rsrgan_amd.run_rnn --decode --test_inputs_scp test/inputs.scp --data_dir data/train --g_type res_lstm_i --save_dir exp/rnn

--g_type: lstm, res_lstm_l, res_lstm_base, bnlstm, res_lstm_i (rnn_trainer.py:97-108).  Multi-GPU as run_gan_rnn: launch with
`python -m torch.distributed.run --nproc-per-node N -m rsrgan_amd.run_rnn ...`.  Flag names and defaults are the reference's
(train_rnn.py:432-570); the *_list_file flags are replaced by *_inputs_scp / *_labels_scp.  Decode -- reader, CMVN, chunked and
multi-stream decode, the archive writer -- is run_gan_rnn's, on an RNNTrainer."""
from __future__ import annotations

import argparse
import datetime

import numpy as np

from . import dist as rdist
from . import run_gan_rnn as gan_loop
from .io import prefetch
from .run_gan_rnn import _cmvn, check_wav_flags, get_num_batch, split_reader, str2bool
from .train import _batches, _check_device, _on_stream, device_batch, exponential_decay
from .trainer import RNNTrainer


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
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--g_learning_rate", type=float, default=0.0001)
    p.add_argument("--min_epochs", type=int, default=15)
    p.add_argument("--max_epochs", type=int, default=20)
    p.add_argument("--end_improve", type=float, default=0.001)
    p.add_argument("--num_threads", type=int, default=24)
    p.add_argument("--save_dir", type=str, default="exp/rnn")
    p.add_argument("--g_type", type=str, default="lstm")
    p.add_argument("--batch_norm", type=str2bool, nargs="?", default="false")
    p.add_argument("--keep_prob", type=float, default=1.0)
    p.add_argument("--l2_scale", type=float, default=0.00001)
    p.add_argument("--num_gpu", type=int, default=1)
    p.add_argument("--apply_cmvn", type=str2bool, nargs="?", default="true")
    p.add_argument("--max_frames", type=int, default=3000, help="capacity of the padded time axis")
    p.add_argument("--decode_chunk", type=int, default=0, help="decode: frames per forward call (run_gan_rnn --decode_chunk)")
    p.add_argument("--decode_streams", type=int, default=1, help="decode with --decode_chunk: utterances decoded side by side")
    p.add_argument("--decode_lean", default=False, action="store_true", help="decode on an inference-only model (inference_only=True: "
                   "the generator alone, no BPTT stash; --g_type bnlstm with --decode_chunk always decodes on it)")
    p.add_argument("--decode_push", type=int, default=0, help="decode with --decode_chunk: the live path, pushes of this many raw frames "
                   "(run_gan_rnn --decode_push)")
    p.add_argument("--device_features", type=str2bool, nargs="?", const=True, default=False, help="CMVN, context splice and padding on the "
                   "device (run_gan_rnn --device_features)")
    p.add_argument("--device_summaries", type=str2bool, nargs="?", const=True, default=False, help="the TensorBoard histograms of the "
                   "training and cross-validation summaries are computed on the device (csrc/hist.hip) and the discriminator's logits get "
                   "theirs (d_real, d_fake); off: three histograms computed on the host")
    p.add_argument("--device_decode", type=str2bool, nargs="?", const=True, default=False, help="implies --device_features; the archive's "
                   "bytes travel undecoded and the device decodes them (run_gan_rnn --device_decode)")
    p.add_argument("--wav_scp", type=str, default=None, help="decode: read audio (lines `utt path`, 16-bit PCM wav at 16 kHz) instead of "
                   "--test_inputs_scp (run_gan_rnn --wav_scp)")
    for n in ("tr_inputs_wav_scp", "tr_labels_wav_scp", "cv_inputs_wav_scp", "cv_labels_wav_scp"):
        p.add_argument("--" + n, type=str, default=None, help="train from audio: a wav.scp in place of the split's *_scp archive "
                       "(run_gan_rnn --%s)" % n)
    gan_loop.add_audio_out_flags(p)
    from .io.reverb import add_sim_flags
    add_sim_flags(p)
    return p


def _run_batches(model, num_batch, iteration, queue, num_gpu, train):
    """the batch loop of train_one_iteration / eval_one_iteration (train_rnn.py:26-57,60-86): the three averages (mse, l2, total) over
    the batches, towers averaged; one summary of the last fed batch at the end (:50-51,79-80).  Losses stay on the device until the
    end of the iteration."""
    full = model.batch_size * num_gpu
    acc, n, last = None, 0, None
    it = _batches(queue)
    for _ in range(int(num_batch / num_gpu)):
        try:
            _, x, lab, ln = next(it)
        except StopIteration:
            break
        if x.shape[0] != full:
            continue
        x, lab, ln = device_batch(model, x, lab, ln, d_run=False)      # (--device_features: packed raw frames, expanded on the device)
        tw =model.g_step(x, lab, ln, train=train, sync=False, gather=False).mean(0)      # this tower's (adv = 0, mse, l2, total)
        acc = tw if acc is None else acc + tw
        n += 1
        last = (x, lab, ln)
    w = model.writer_for(train) if n and hasattr(model, "writer_for") else None
    if w is not None:
        w.add_summary(model.run_summaries(*last), iteration * num_batch)
    if acc is None:
        return 0.0, 0.0, 0.0
    g = (rdist.all_reduce_mean_(acc.clone(), getattr(model, "process_group", None)) / n).cpu().numpy()
    _check_device(model, np.zeros(3), g)
    return float(g[1]), float(g[2]), float(g[3])


def train_one_iteration(model, tr_num_batch, iteration, train_queue, num_gpu=None):
    with _on_stream(model):
        return _run_batches(model, tr_num_batch, iteration, train_queue, num_gpu or model.num_gpu, True)


def eval_one_iteration(model, cv_num_batch, iteration, valid_queue, num_gpu=None):
    with _on_stream(model):
        return _run_batches(model, cv_num_batch, iteration, valid_queue, num_gpu or model.num_gpu, False)


def _model(FLAGS, cv, share, net_overrides, **kw):
    return RNNTrainer(None, FLAGS, ["gpu:%d" % rdist.rank()], cross_validation=cv, share_engine_from=share,
                      net_overrides=net_overrides, **kw)


def train(FLAGS, model_factory=None, log=print, net_overrides=None):
    """train (:270-430) + the batch counting of main (:196-221).  Returns the list of per-iteration CV g_loss."""
    check_wav_flags(FLAGS)
    cmvn = _cmvn(FLAGS)
    mk = model_factory or (lambda cv, share: _model(FLAGS, cv, share, net_overrides, max_frames=FLAGS.max_frames))
    tr_model = mk(False, None)
    cv_model = mk(True, tr_model)                                          # shares variables (:319-325)
    if tr_model.load(tr_model.save_dir):
        log("[*] Load SUCCESS")
    else:
        log("[!] Begin a new model.")
    full = FLAGS.batch_size * FLAGS.num_gpu
    tr_reader = split_reader(FLAGS, "tr", cmvn, True, 1234)
    cv_reader = split_reader(FLAGS, "cv", cmvn, False, None)
    tr_num_batch = get_num_batch(split_reader(FLAGS, "tr", None, False, None), full)
    cv_num_batch = get_num_batch(split_reader(FLAGS, "cv", None, False, None), full)
    train_batch_per_iter, valdi_batch_per_iter = tr_num_batch, cv_num_batch                  # :204-205
    min_iters = int(FLAGS.min_epochs * tr_num_batch / train_batch_per_iter)
    max_iters = int(FLAGS.max_epochs * tr_num_batch / train_batch_per_iter)
    log("LOG: #train_batch = {}, #valid_batch = {}, #min_iters = {}, #max_iters = {}".format(tr_num_batch, cv_num_batch, min_iters, max_iters))

    g_loss_prev, g_rel_impr, check_interval, windows_g_loss = 10000.0, 1.0, 1, []           # :340-343
    tr_model.g_learning_rate = FLAGS.num_gpu * FLAGS.g_learning_rate                         # :345-347
    history = []
    iteration = -1
    for iteration in range(max_iters):
        start = datetime.datetime.now()
        if hasattr(tr_reader, "set_epoch"):
            tr_reader.set_epoch(iteration)                # (--tr_rir_scp: other rooms every epoch; cross-validation keeps epoch 0's)
        tr = train_one_iteration(tr_model, train_batch_per_iter * FLAGS.num_gpu, iteration + 1, prefetch(tr_reader), FLAGS.num_gpu)
        if hasattr(tr_model, "sync_batch_norm_state"):
            tr_model.sync_batch_norm_state()           # one copy of the batch-norm statistics over the ranks, before cross-validation and the checkpoint
        cv = eval_one_iteration(cv_model, valdi_batch_per_iter * FLAGS.num_gpu, iteration + 1,
                                prefetch(b for b in cv_reader if len(b[0]) == full), FLAGS.num_gpu)
        end = datetime.datetime.now()
        log("{}/{} (TRAIN AVG.LOSS): g_mse_loss = {:.5f}, g_l2_loss = {:.5f}, g_loss = {:.5f}, learning_rate= {:.3e}\n"
            "{}/{} (CROSS AVG.LOSS): g_mse_loss = {:.5f}, g_l2_loss = {:.5f}, g_loss = {:.5f}, time = {:.2f} h".format(
                iteration + 1, max_iters, tr[0], tr[1], tr[2], tr_model.g_learning_rate,
                iteration + 1, max_iters, cv[0], cv[1], cv[2], (end - start).total_seconds() / 3600.0))
        cv_g_loss = cv[2]
        history.append(cv_g_loss)
        # Start decay learning rate (:374-378)
        tr_model.g_learning_rate = exponential_decay(iteration + 1, FLAGS.num_gpu, min_iters, FLAGS.g_learning_rate)
        windows_g_loss.append(cv_g_loss)
        # Accept or reject new parameters (:382-399; the reload of a rejected iteration is commented out there: nothing else happens)
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
        # Stopping criterion (:401-407)
        if iteration + 1 > min_iters and (iteration + 1) % check_interval == 0 and g_rel_impr < FLAGS.end_improve:
            log("Iteration %d: Finished, too small relative G improvement %g" % (iteration + 1, g_rel_impr))
            break
    if windows_g_loss:                                                     # Whether save the last model (:414-426)
        g_loss_new = float(np.mean(windows_g_loss))
        if (g_loss_prev - g_loss_new) / g_loss_prev > 0.0:
            tr_model.save(tr_model.save_dir, iteration + 1)
            log("Iteration {}: Nnet Accepted. Save model SUCCESS. g_loss_prev = {:.5f}, g_loss_new = {:.5f}".format(
                iteration + 1, g_loss_prev, g_loss_new))
    log("Training Done.")
    return history


def decode_lean(FLAGS, log=print):
    """whether decode builds the inference-only model: --decode_lean, and -- with one logged line -- a chunked bnlstm decode without it: the
    stateful forward of a bnlstm model exists on the inference handle only (a training handle answers 'not built')"""
    if getattr(FLAGS, "decode_lean", False):
        return True
    if int(getattr(FLAGS, "decode_chunk", 0) or 0) > 0 and getattr(FLAGS, "g_type", None) == "bnlstm":
        log("--decode_chunk with --g_type bnlstm: decoding on the inference-only model (as --decode_lean), the only stateful forward bnlstm has")
        return True
    return False


def decode(FLAGS, model_factory=None, log=print, net_overrides=None):
    """decode (:89-176) = run_gan_rnn.decode on an RNNTrainer: batch 1 (or --decode_streams rows of --decode_chunk frames)"""
    chunk, streams = int(getattr(FLAGS, "decode_chunk", 0) or 0), max(1, int(getattr(FLAGS, "decode_streams", 1) or 1))
    lean = decode_lean(FLAGS, log) if model_factory is None else False
    mk = model_factory or (lambda: _model(argparse.Namespace(**dict(vars(FLAGS), batch_size=streams if chunk > 0 else 1)), True, None,
                                          net_overrides, max_frames=chunk if chunk > 0 else FLAGS.max_frames,
                                          **({"inference_only": True} if lean else {})))
    return gan_loop.decode(FLAGS, model_factory=mk, log=log)


def main(argv=None):
    FLAGS, unparsed = build_parser().parse_known_args(argv)                # unknown flags are ignored, as in the reference
    rank, local, world = rdist.init_from_env()
    if world > 1:
        FLAGS.num_gpu = world
    if FLAGS.decode:
        rdist.run_on_rank0(lambda: decode(FLAGS))
    else:
        train(FLAGS)


if __name__ == "__main__":
    main()
