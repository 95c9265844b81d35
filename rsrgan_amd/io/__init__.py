"""NumPy / Kaldi-ark data path replacing the reference's io_funcs (TFRecords + tf.data):
ark/scp reader and writer, global CMVN, Kaldi-style splicing, length-bucketed padded batches."""
from .kaldi_ark import ArkReader, ArkWriter, CodedMatrix, read_binary_file, convert_cmvn_to_numpy     # noqa: F401
from .features import apply_cmvn, splice_feats, PaddedBatchReader, FrameBatchReader                          # noqa: F401
from .features import PackedBatch, pack_utterances, CodedBatch, pack_coded                # noqa: F401
from .wave import MfccSpec, WaveBatch, WaveSpec, lps_from_wave, mfcc_from_wave, num_frames, pack_wave, read_wav, read_wav_scp        # noqa: F401
from .wave import quantize_pcm, wave_from_lps, write_wav     # noqa: F401
from .wave_reader import WaveBatchReader                    # noqa: F401
from .reverb import ReverbPlan, ReverbSim, ReverbSpec, reverberate                          # noqa: F401
from .frame_pool import FrameDraw, PoolLedger, RowAllocator                                 # noqa: F401
from .prefetch import prefetch                                                             # noqa: F401
