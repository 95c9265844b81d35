"""Host reference of the device-side feature front end (csrc/feat.hip, HipEngine.featurize): the expansion of a packed batch built only
from io.features.apply_cmvn, io.features.splice_feats and the padding rule of PaddedBatchReader._pad -- the very functions the default
reader runs per utterance.  An utterance longer than T is spliced WHOLE and then cut: its context is clamped at its own last frame,
never at T."""
import struct

import numpy as np

from rsrgan_amd.io import ArkWriter, PackedBatch, apply_cmvn, splice_feats


def expand(packed, cmvn, left, right, T):
    """packed: anything with .data [rows, D] float32 and .offsets [B + 1]; cmvn: None or (mean [D], stddev [D]) in float64.
    Returns (out [B, T, D * (left + 1 + right)] float32, lengths [B] int32)."""
    data, offsets = np.asarray(packed.data), np.asarray(packed.offsets).astype(np.int64)
    B, D = len(offsets) - 1, data.shape[1]
    out = np.empty((B, T, D * (left + 1 + right)), np.float32)
    lengths = np.zeros(B, np.int32)
    for b in range(B):
        x = data[offsets[b]:max(offsets[b + 1], offsets[b])].astype(np.float64)
        if cmvn is not None:
            x, _ = apply_cmvn(x, None, {"mean_inputs": cmvn[0], "stddev_inputs": cmvn[1]})
        x = splice_feats(x, left, right).astype(np.float32) if x.shape[0] else np.zeros((0, out.shape[2]), np.float32)
        n = min(x.shape[0], T)
        out[b, :n] = x[:n]; out[b, n:] = 0.0
        lengths[b] = n
    return out, lengths


def expand_item(item, T=None):
    """a packed reader item [ids, PackedBatch, PackedBatch, lengths] -> the default reader's [ids, X, Y, L]"""
    ids, xp, yp, _ = item
    T = xp.shape[1] if T is None else T
    stats = lambda p: None if p.mean is None else (p.mean, p.stddev)
    X, L = expand(xp, stats(xp), xp.left, xp.right, T)
    Y, L2 = expand(yp, stats(yp), yp.left, yp.right, T)
    assert np.array_equal(L, L2)
    return [ids, X, Y, L]


def seeded_stats(rng, D):
    """fp64 statistics: any mean, stddev in [0.5, 2]"""
    return rng.standard_normal(D) * 3.0, rng.uniform(0.5, 2.0, D)


def random_packed(rng, lengths, D, left=0, right=0, T=None, lead=0, stats=None):
    """utterances of the given lengths packed behind `lead` unused rows (offsets[0] = lead)"""
    rows = lead + int(sum(lengths))
    data = (rng.standard_normal((max(rows, 1), D)) * 2.0 + 0.5).astype(np.float32)
    offsets = (lead + np.concatenate([[0], np.cumsum(lengths)])).astype(np.int32)
    T = max(max(lengths), 1) if T is None else T
    mean, stddev = stats if stats is not None else (None, None)
    return PackedBatch(data, offsets, (len(lengths), T, D * (left + 1 + right)), left, right, mean, stddev)


def write_arks(tmp, tag, lengths, din, dout, rng, double_at=None):
    """input / label arks of float32 utterances with the given lengths (utterance `double_at` of the inputs as a float64 'BDM ' matrix);
    returns (inputs.scp, labels.scp)"""
    wi, wl = ArkWriter(str(tmp / (tag + "_in.scp"))), ArkWriter(str(tmp / (tag + "_lab.scp")))
    for i, T in enumerate(lengths):
        utt = "%s%03d" % (tag, i)
        x = rng.standard_normal((T, din)) * 2 + 1
        if i == double_at:
            ark = str(tmp / (tag + "_in.ark"))
            with open(ark, "ab") as f:
                f.write(utt.encode())
                pos = f.tell()
                f.write(struct.pack("<xcccc", b"B", b"D", b"M", b" "))
                f.write(struct.pack("<bi", 4, T)); f.write(struct.pack("<bi", 4, din))
                f.write(np.ascontiguousarray(x, np.float64).tobytes())
            wi.scp_file_write.write("%s %s:%s\n" % (utt, ark, pos))
        else:
            wi.write_next_utt(str(tmp / (tag + "_in.ark")), utt, x)
        wl.write_next_utt(str(tmp / (tag + "_lab.ark")), utt, rng.standard_normal((T, dout)) - 1)
    wi.close(); wl.close()
    return str(tmp / (tag + "_in.scp")), str(tmp / (tag + "_lab.scp"))


def cmvn_for(rng, din, dout):
    mi, si = seeded_stats(rng, din)
    ml, sl = seeded_stats(rng, dout)
    return {"mean_inputs": mi, "stddev_inputs": si, "mean_labels": ml, "stddev_labels": sl}
