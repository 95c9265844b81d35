"""Training batches from audio: PaddedBatchReader's sibling over two wav.scp files (reverberant inputs, clean labels) instead of two feature
archives.  Inputs become log-power-spectrum frames (io.wave.WaveSpec), labels MFCC frames (io.wave.MfccSpec: compute-mfcc-feats with
mfcc_hires.conf) or, with a plain WaveSpec as label_spec, LPS frames, on the host or on the device."""
from __future__ import annotations

import random
import wave as _wave
from typing import Iterator, List

import numpy as np

from .features import apply_cmvn, pad_items, plan_batches, splice_feats
from .wave import DEFAULT, MFCC_DEFAULT, MfccSpec, lps_from_wave, mfcc_from_wave, num_frames, pack_wave, read_wav, read_wav_scp


class WaveBatchReader(object):
    """Reads (inputs, labels) utterance pairs from two wav.scp files (lines `utt path`, 16-bit PCM; the utterance ids of the two files
    equal and in the same order) and yields PaddedBatchReader's items with its plan() rules: windows of `batch_size` by length bucket
    (start 200 frames, width 50, ids clipped at num_buckets), partial windows at the end.  The frame counts come from the wav headers
    alone (no sample is read before materialize), so io.prefetch can run materialize on several threads.

    Default route: lps_from_wave / mfcc_from_wave (lps_from_wave for an LPS label_spec) on the host (float64, one rounding), then PaddedBatchReader's float64 CMVN, splice and
    zero padding: the items are ordinary padded batches [utt_ids, inputs [B, T, bins * (L + 1 + R)] f32, labels [B, T, label bins] f32,
    lengths [B] i32].
    device_features=True: the samples travel; the items are [utt_ids, WaveBatch(inputs), WaveBatch(labels), lengths] and the device makes
    the frames (csrc/wave.hip k_feat_wave / k_feat_mfcc), normalises, splices and pads them (HipEngine.featurize).

    simulate=io.reverb.ReverbSim(rir_scp, noise_scp, spec, seed) with inputs_wav_scp=None: there is no second corpus; the inputs are the
    LABELS' audio reverberated with the RIR (and noise) drawn for (seed, epoch, utterance index) -- set_epoch selects the epoch, the draw
    of an utterance depends on nothing else, so materialize may run on several threads in any order.  The spec must shift, so that the
    reverberant utterance is as long as the clean one and the frame counts agree.  Host route: io.reverb.reverberate (float64), then
    lps_from_wave.  device_features=True: the items are [utt_ids, WaveBatch(CLEAN samples + the batch's ReverbPlan), WaveBatch(labels),
    lengths] and the device reverberates (csrc/reverb.hip) before it makes the frames.  Without `simulate` nothing changes.

    ValueError at construction, naming the utterance: a pair whose two files make different frame counts, an utterance that makes no
    frame, ids that differ between the two files."""

    def __init__(self, inputs_wav_scp, labels_wav_scp, batch_size, left_context=0, right_context=0, cmvn=None, num_buckets=20, shuffle=True,
                 seed=None, device_features=False, input_spec=DEFAULT, label_spec=MFCC_DEFAULT, simulate=None):
        self.device_features = bool(device_features)
        self.simulate = simulate
        if (simulate is None) == (inputs_wav_scp is None):
            raise ValueError("the inputs come from inputs_wav_scp or from simulate=ReverbSim(...) on the labels' audio: give exactly one")
        if simulate is not None:
            if not simulate.spec.shift:
                raise ValueError("simulate: the ReverbSpec must shift (shift=True), so that the frame counts of inputs and labels agree")
            if simulate.spec.sample_rate != input_spec.sample_rate or input_spec.sample_rate != label_spec.sample_rate:
                raise ValueError("simulate: the sample rates of the ReverbSpec (%d), the inputs (%d) and the labels (%d) differ" % (
                    simulate.spec.sample_rate, input_spec.sample_rate, label_spec.sample_rate))
            inputs_wav_scp = labels_wav_scp
        self.input_spec, self.label_spec = input_spec, label_spec
        self._stats = None
        if self.device_features and cmvn is not None:
            self._stats = tuple(np.ascontiguousarray(cmvn[k], np.float64).reshape(-1)
                                for k in ("mean_inputs", "stddev_inputs", "mean_labels", "stddev_labels"))
        self.inputs, self.labels = read_wav_scp(inputs_wav_scp), read_wav_scp(labels_wav_scp)
        self.utt_ids = [u for u, _ in self.inputs]
        if self.utt_ids != [u for u, _ in self.labels]:
            raise ValueError("%s and %s do not list the same utterance ids in the same order" % (inputs_wav_scp, labels_wav_scp))
        self.batch_size, self.left, self.right = batch_size, left_context, right_context
        self.cmvn, self.num_buckets, self.shuffle = cmvn, num_buckets, shuffle
        self.rng = random.Random(seed)
        self._nframes = []
        for (u, px), (_, py) in zip(self.inputs, self.labels):
            fx, fy = num_frames(_header_samples(px), input_spec), num_frames(_header_samples(py), label_spec)
            if fx != fy:
                raise ValueError("utterance %s: %d input frames (%s), %d label frames (%s)" % (u, fx, px, fy, py))
            if fx == 0:
                raise ValueError("utterance %s: %s makes no frame (fewer than %d samples)" % (u, px, input_spec.frame_length))
            self._nframes.append(fx)

    def __len__(self):
        return len(self.utt_ids)

    def plan(self) -> Iterator[List[int]]:
        """the utterance indices of every batch, in the order __iter__ yields them: PaddedBatchReader's rule on the headers' frame counts"""
        return plan_batches(self._nframes, self.batch_size, self.num_buckets, self.shuffle, self.rng)

    def __iter__(self) -> Iterator[List]:
        for indices in self.plan():
            yield self.materialize(indices)

    def set_epoch(self, epoch):
        """simulate: the epoch of the draws from here on (cross-validation never calls it: epoch 0 every time)"""
        if self.simulate is not None:
            self.simulate.set_epoch(epoch)

    def _samples(self, i):
        if self.simulate is not None:
            # host route: the labels' audio through the RIR and noise drawn for (seed, epoch, i); float64, not quantised
            sy = read_wav(self.labels[i][1], sample_rate=self.label_spec.sample_rate)
            return self.simulate.apply(sy, self.simulate.draw(i, sy.shape[0])), sy
        return (read_wav(self.inputs[i][1], sample_rate=self.input_spec.sample_rate),
                read_wav(self.labels[i][1], sample_rate=self.label_spec.sample_rate))

    def _utt(self, i):
        sx, sy = self._samples(i)
        x = lps_from_wave(sx, spec=self.input_spec).astype(np.float64)
        y = _label_frames(sy, self.label_spec).astype(np.float64)
        if self.cmvn is not None:
            x, y = apply_cmvn(x, y, self.cmvn)
        return self.utt_ids[i], splice_feats(x, self.left, self.right).astype(np.float32), y.astype(np.float32)

    def _waves(self, indices):
        ids = [self.utt_ids[i] for i in indices]
        mi, si, ml, sl = self._stats if self._stats is not None else (None,) * 4
        if self.simulate is not None:
            clean = [read_wav(self.labels[i][1], sample_rate=self.label_spec.sample_rate) for i in indices]
            pairs = [(c, c) for c in clean]
            plan = self.simulate.plan(indices, [c.shape[0] for c in clean])
        else:
            pairs, plan = [self._samples(i) for i in indices], None
        X = pack_wave([p[0] for p in pairs], None, self.left, self.right, mi, si, self.input_spec, names=ids, plan=plan)
        Y = pack_wave([p[1] for p in pairs], None, 0, 0, ml, sl, self.label_spec, names=ids)
        return [ids, X, Y, X.lengths()]

    def materialize(self, indices: List[int]) -> List:
        if self.device_features:
            return self._waves(indices)
        return pad_items([self._utt(i) for i in indices])


def _label_frames(samples, spec):
    """the host route of the labels dispatches on the spec, as the device route does (HipEngine.wave_features): MFCC / log-mel for an
    MfccSpec, LPS for a plain WaveSpec (the targets a model must have for audio out)"""
    return mfcc_from_wave(samples, spec) if isinstance(spec, MfccSpec) else lps_from_wave(samples, spec=spec)


def _header_samples(path):
    """samples per channel of a RIFF file, from its header alone"""
    with _wave.open(str(path), "rb") as f:
        return f.getnframes()
