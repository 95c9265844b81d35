/* rsrgan.h -- C ABI of librsrgan_hip.so: RSRGAN's sequence-level GAN training step
 * (LSTMP generator + LSTMP discriminator, LSGAN losses, SGD(D)/Adam(G)) as
 * hand-written HIP kernels for MI355X (gfx950).
 *
 * The reference (wangkenpu/rsrgan, Python 2.7 + TensorFlow 1.4) has no FFI; the
 * de-facto boundary is the object surface that
 *   scripts/train_gan_rnn_placeholder.py:train_one_iteration (:48-133),
 *   eval_one_iteration (:136-201) and decode (:204-302)
 * touch on models/gan_rnn_placeholder.py:GAN_RNN (:62-298).  Every entry point
 * below names the reference interface it replaces.  The reference-side binding
 * (a ctypes stub a maintainer would drop into models/gan_rnn_placeholder.py) is
 * shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no torch types.  Every `const float*` / `float*` data pointer is a
 *     DEVICE pointer owned by the caller (e.g. torch.Tensor.data_ptr()) and is
 *     only borrowed for the duration of the call's stream work, exactly like a
 *     TF feed_dict entry (gan_rnn_placeholder.py:94-104).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 *     work is enqueued asynchronously on it; nothing synchronises the device.
 *   - every function returns 0 on success or a negative rsrgan_status; nothing
 *     throws across the ABI; rsrgan_last_error() returns a thread-local string.
 *   - one handle per process/GPU, single caller thread
 *     (train_gan_rnn_placeholder.py:463-478: all sess.run calls come from the
 *     main thread).
 *   - all arithmetic is IEEE fp32 (tf.float32 placeholders, :94-104).
 */
#ifndef RSRGAN_H_
#define RSRGAN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rsrgan_status {
  RSRGAN_OK = 0,
  RSRGAN_ERR_INVALID = -1,     /* bad argument / unsupported configuration (ValueError in the reference, :131-132) */
  RSRGAN_ERR_HIP = -2,         /* a HIP runtime call failed */
  RSRGAN_ERR_NO_DEVICE = -3,   /* no gfx950 device visible */
  RSRGAN_ERR_STATE = -4        /* call sequence error (e.g. apply without backward) */
} rsrgan_status;

/* args.g_type (gan_rnn_placeholder.py:125-132) */
enum { RSRGAN_G_LSTM = 0, RSRGAN_G_RES_LSTM_L = 1, RSRGAN_G_RES_LSTM_BASE = 2,
       RSRGAN_G_DNN = 3, /* models/gan.py:109-110 + models/dnn.py: frame-level FC generator */
       RSRGAN_G_RCED = 4, /* models/rced.py: frame-level 9 x conv2d + FC generator (dnn_trainer.py:98-99), batch_norm=False */
       RSRGAN_G_BNLSTM = 5 /* models/bnlstm.py: input FC + ReLU, BNLSTMCell(g_cells, num_proj=g_proj, peepholes) x g_layers with batch
                              normalisation inside the recurrence, output FC; RSRGAN_FLAG_SUPERVISED only (models/rnn_trainer.py),
                              batch_size <= 64 (training handles; an inference handle pads to the persistent launch's row groups), no
                              RSRGAN_FLAG_BATCH_NORM, no dropout */,
       RSRGAN_G_RES_LSTM_I = 6 /* models/res_lstm_i.py: res_lstm_l's cells and variable table, but the residual is always the stack's
                                  input: inputs_{l+1} = outputs_l + x, the output FC reads outputs_L + x (never a running sum);
                                  needs g_proj == input_dim; RSRGAN_FLAG_SUPERVISED only (models/rnn_trainer.py:97-108: the
                                  reference GAN has no such generator) */ };
/* self.discriminator (gan_rnn_placeholder.py:117; models/gan.py:104) */
enum { RSRGAN_D_LSTM = 0, RSRGAN_D_DNN = 1 /* models/discriminator_dnn.py */ };
/* which network a call addresses */
enum { RSRGAN_NET_G = 0, RSRGAN_NET_D = 1 };

/* Mutable scalars that the reference changes with sess.run(tf.assign(...))
 * between steps (train_gan_rnn_placeholder.py:63-64,460-461,531-533;
 * gan_rnn_placeholder.py:112-123). */
typedef enum rsrgan_scalar {
  RSRGAN_G_LEARNING_RATE = 0,
  RSRGAN_D_LEARNING_RATE = 1,
  RSRGAN_MSE_LAMBDA = 2,
  RSRGAN_D_REAL = 3,
  RSRGAN_D_FAKE = 4,
  RSRGAN_L2_SCALE = 5,
  RSRGAN_CLIP_NORM = 6,
  RSRGAN_ADAM_STEP = 7,       /* Adam's t (beta powers) of the generator, for checkpoint/resume */
  RSRGAN_ADAM_STEP_D = 8,     /* Adam's t of the discriminator (frame-level GAN only: models/gan.py:125) */
  RSRGAN_SCALAR_COUNT_
} rsrgan_scalar;

/* Construction arguments: the fields GAN_RNN.__init__ reads from `args`
 * (gan_rnn_placeholder.py:65-137) plus the layer sizes the reference
 * hard-codes (models/lstm.py:43-45, models/res_lstm_l.py:43-45,
 * models/discriminator_lstm.py:26-28) made runtime parameters. */
typedef struct rsrgan_cfg {
  int32_t batch_size;      /* per-GPU B (:96) */
  int32_t max_frames;      /* capacity for the padded time axis T */
  int32_t input_dim;       /* input_dim*(left_context+1+right_context) (:96-98) */
  int32_t output_dim;      /* 40 */
  int32_t g_type;          /* RSRGAN_G_* */
  int32_t g_layers;        /* 3 (lstm) / 4 (res_lstm_l, res_lstm_base) / 2 (res_lstm_i) */
  int32_t g_cells;         /* 760 */
  int32_t g_proj;          /* 280 (lstm) / 257 (res_lstm_*) */
  int32_t d_type;          /* RSRGAN_D_LSTM */
  int32_t d_layers;        /* 2 */
  int32_t d_cells;         /* 256 */
  int32_t d_proj;          /* 40 */
  float   l2_scale;        /* args.l2_scale (:91) */
  float   clip_norm;       /* self.max_grad_norm = 15 (:71) */
  float   adam_beta1;      /* 0.9   (tf.train.AdamOptimizer defaults, :147) */
  float   adam_beta2;      /* 0.999 */
  float   adam_eps;        /* 1e-8  */
  float   ema_decay;       /* MOVING_AVERAGE_DECAY 0.9999 (:70); 0 disables the shadow copy */
  float   lrelu_alpha;     /* utils/ops.py:120 (0.3) */
  float   forget_bias;     /* LSTMCell(forget_bias=1.0) (models/lstm.py:94) */
  int32_t cross_validation;/* 1 = the cross_validation=True twin: no L2 term (:253) */
  int32_t flags;           /* RSRGAN_FLAG_* */
  /* frame-level GAN (models/gan.py:158-175): D sees concat(inputs[:, d_joint_off : +d_joint_dim], labels|G(x));
   * d_joint_dim = 0 feeds D the 40-dim target only, as gan_rnn_placeholder.py:207-208 does */
  int32_t d_joint_off;
  int32_t d_joint_dim;
  /* R-CED generator (models/rced.py:36-52): the fed frame is reshaped to [g_splice, input_dim / g_splice, 1]
   * (g_splice = left_context + 1 + right_context); 9 conv2d layers 12,16,20,24,32,24,20,16,12 x [g_splice, 13..7..13] */
  int32_t g_splice;
} rsrgan_cfg;

enum {
  RSRGAN_FLAG_WAVEFRONT = 1,   /* run the stacked LSTMs as one (layer,t) wavefront (default schedule when set) */
  RSRGAN_FLAG_GRAPH = 2,       /* replay the (static, per T) launch sequences of the wavefront schedule as hipGraphs: 1.6 us per
                                  dependent kernel on the GPU vs 3.1-4.6 us host-bound per eager launch (measured, round 2) */
  RSRGAN_FLAG_NO_SPLITK_B = 8, /* backward phase B as one launch of 32x16 tiles (round-1 first form) instead of split-K + reduce */
  RSRGAN_FLAG_SUPERVISED = 16, /* generator-only trainer (models/rnn_trainer.py:66-156, models/dnn_trainer.py:64-148):
                                  g_loss = mse_lambda*g_mse + g_l2, no discriminator pass; rsrgan_d_step is an error */
  RSRGAN_FLAG_OVERLAP = 4,     /* weight-gradient GEMMs on a side stream, chunked over time, concurrent with the backward
                                  wave (measured SLOWER on MI355X: 12.77 vs 12.20 ms/step; off by default) */
  RSRGAN_FLAG_INFER = 64,      /* GAN_RNN(..., infer=True) (models/gan_rnn_placeholder.py:133-135): a generator-only, forward-only handle.  No
                                  discriminator (RSRGAN_NET_D's tensor table is empty), no gradients, optimizer moments or EMA shadows, no
                                  BPTT stash: the recurrent state buffers hold min(max_frames, 64) + 1 steps and the persistent forward
                                  launches run without their stash stores (csrc/gpersist.hip LEAN), a batch longer than one launch as
                                  consecutive launches that carry the state.  RSRGAN_NET_G's tensor table is the training handle's (names,
                                  order, offsets), so a checkpoint loads.  For the sequence generators lstm, res_lstm_l, res_lstm_base,
                                  res_lstm_i (with RSRGAN_FLAG_SUPERVISED, as always), the unprojected stack and bnlstm; dnn and rced:
                                  RSRGAN_ERR_INVALID ("not built").  bnlstm (with RSRGAN_FLAG_SUPERVISED | RSRGAN_FLAG_WAVEFRONT):
                                  the three batch-norm sites are folded into the kernels, the bias and a per-unit affine pair with the moving
                                  statistics at create and at every rsrgan_set_params(what = 0); the persistent launch is the only forward
                                  it has, so create returns RSRGAN_ERR_INVALID without RSRGAN_FLAG_WAVEFRONT ("not built"), for a shape
                                  without a persistent plan and under RSRGAN_GP_TAGS=0, and after a reported device failure
                                  (rsrgan_device_status) the forward calls return RSRGAN_ERR_HIP.  batch_size is padded to 1, 2, 4 or 8
                                  groups of 32 rows (at most 256).  Work: rsrgan_forward_g, rsrgan_forward_g_stream, rsrgan_g_state_*,
                                  rsrgan_set_params / rsrgan_get_params with what = 0 on RSRGAN_NET_G, the tensor-table calls,
                                  rsrgan_device_status, rsrgan_device_bytes, the profile counters, rsrgan_destroy.  Refused before the first
                                  HIP call, rsrgan_last_error() naming the inference-only handle: rsrgan_d_step, rsrgan_g_step,
                                  rsrgan_*_backward, rsrgan_apply, rsrgan_grad_buffer, rsrgan_grad_bucket_*, rsrgan_get_grads and
                                  rsrgan_set_dropout with RSRGAN_ERR_STATE, get / set_params with what = 1, 2, 3 with RSRGAN_ERR_INVALID. */
  RSRGAN_FLAG_BATCH_NORM = 32  /* args.batch_norm (run_gan_dnn.sh:134, run_dnn.sh:134): the hidden fully_connected layers of the
                                  frame-level generator (models/dnn.py:56-61) and of discriminator_dnn (:36-41) are
                                  relu(batch_norm(x.W, is_training = !cross_validation, scale=True, renorm=True)) without biases;
                                  the variable table gains <scope>/BatchNorm/{beta,gamma,moving_mean,moving_variance,renorm_mean,
                                  renorm_mean_weight,renorm_stddev,renorm_stddev_weight}.  Frame-level nets only. */
};

typedef struct rsrgan_handle_s* rsrgan_handle;

/* fills *cfg with the reference's hard-coded sizes for `g_type`. */
int rsrgan_default_cfg(int32_t g_type, rsrgan_cfg* cfg);

/* GAN_RNN(sess, args, devices, cross_validation, infer) (gan_rnn_placeholder.py:65-137).
 * Allocates parameters (xavier-uniform / zero biases from `seed`, as
 * xavier_initializer()/zeros_initializer(), models/lstm.py:86-87), optimizer
 * state and all activation stashes for (batch_size, max_frames). */
int rsrgan_create(const rsrgan_cfg* cfg, uint64_t seed, rsrgan_handle* out);
int rsrgan_destroy(rsrgan_handle h);
const char* rsrgan_last_error(void);

/* sess.run(tf.assign(model.<scalar>, v)) (train_gan_rnn_placeholder.py:63-64,460-461,531-533) */
int rsrgan_set_scalar(rsrgan_handle h, int32_t which, double v);
int rsrgan_get_scalar(rsrgan_handle h, int32_t which, double* v);

/* Variable table == tf.trainable_variables() split by the g_/d_ prefix
 * (gan_rnn_placeholder.py:301-317), in graph-construction order. */
int rsrgan_num_tensors(rsrgan_handle h, int32_t net);
int rsrgan_tensor_info(rsrgan_handle h, int32_t net, int32_t idx,
                       char* name, int32_t name_cap,
                       int32_t* rows, int32_t* cols, int64_t* dense_offset);
/* number of floats of the DENSE (TF-shaped, unpadded) flat parameter vector */
int64_t rsrgan_param_count(rsrgan_handle h, int32_t net);

/* tf.train.Saver save/restore payload (gan_rnn_placeholder.py:26-60) and parity
 * injection: dense flat vectors in variable-table order, DEVICE pointers.
 * `what`: 0 = variables, 1 = Adam m, 2 = Adam v (G only), 3 = EMA shadow. */
int rsrgan_get_params(rsrgan_handle h, int32_t net, int32_t what, float* dense, void* stream);
int rsrgan_set_params(rsrgan_handle h, int32_t net, int32_t what, const float* dense, void* stream);
/* last computed (tower-local or all-reduced) gradients, dense, for tests */
int rsrgan_get_grads(rsrgan_handle h, int32_t net, float* dense, void* stream);

/* sess.run(model.g_outputs, {inputs, lengths}) (train_gan_rnn_placeholder.py:282-285)
 *   x [B,T,Din] batch-major, lengths int32 [B], y [B,T,Dout]. */
int rsrgan_forward_g(rsrgan_handle h, const float* x, const int32_t* lengths, int32_t T,
                     float* y, void* stream);

/* ---- stateful generator forward: chunked, streaming and multi-stream decode ----
 * The handle keeps a CARRIED generator state: per layer l the cell state c_l [batch_size, H] and the projected state m_l
 * [batch_size, P] (P = H without num_proj: the state is h), fp32, zero after rsrgan_create.  Only the five calls below read or
 * write it; rsrgan_forward_g and every training call start from cell.zero_state as before.  Sequence generators only:
 * RSRGAN_ERR_INVALID for the frame-level ones (dnn, rced: no state) and for a bnlstm training handle (not built; a bnlstm
 * inference handle, RSRGAN_FLAG_INFER, carries (c, m) per layer like the others: c is the raw cell state, before the cell site's norm).
 *
 * floats of one row's state blob: sum over layers of (H + P); a row is layer 0's c, layer 0's m, layer 1's c, ... unpadded. */
int rsrgan_g_state_floats(rsrgan_handle h, int32_t* n);
/* zero the carried state of the rows whose entry of row_mask (DEVICE int32 [batch_size]) is non-zero; NULL = all rows. */
int rsrgan_g_state_reset(rsrgan_handle h, const int32_t* row_mask, void* stream);
/* copy the carried state out / in: DEVICE [batch_size, floats] buffers (park a stream, resume it on another row or handle). */
int rsrgan_g_state_get(rsrgan_handle h, float* dst, void* stream);
int rsrgan_g_state_set(rsrgan_handle h, const float* src, void* stream);
/* rsrgan_forward_g, but every row b starts from its carried state, and afterwards the carried state is the row's state after
 * its lengths[b] frames (dynamic_rnn copies the state of a finished row through; lengths[b] = 0: the row is inert and keeps
 * its state).  y rows past lengths[b] are the output FC's bias, as in rsrgan_forward_g.  T in (0, max_frames]. */
int rsrgan_forward_g_stream(rsrgan_handle h, const float* x, const int32_t* lengths, int32_t T,
                            float* y, void* stream);

/* sess.run([model.d_opt, model.d_rl_losses, model.d_fk_losses, model.d_losses], feed)
 * (train_gan_rnn_placeholder.py:77-82).  labels [B,T,Dout].  noise_real/noise_fake
 * are the two gaussian_noise_layer draws ([B,Dout], broadcast over T,
 * utils/ops.py:19-30) or NULL for disc_noise_std == 0.  out_losses: DEVICE
 * float[3] = {d_rl, d_fk, d_loss}.  For the frame-level GAN (g_type RSRGAN_G_DNN: models/gan.py,
 * scripts/train_gan_dnn.py) the same entry points are used with T = 1, x [N,1,Din*(L+1+R)], labels
 * [N,1,Dout]; lengths may be NULL there.  train=0 gives the eval fetch
 * (train_gan_rnn_placeholder.py:154-160): losses only, no update.
 * Every buffer is read in `stream` order -- unless the process runs with RSRGAN_DPIPE=1, by which the CALLER guarantees that
 * `labels` and `lengths` (=2: `noise_real` too) are complete when the call is made: they are then read on a side stream, possibly
 * before earlier work on `stream` has finished, so that D(real) of this call can run beside the previous call's tail
 * (DESIGN.md 6-R5 (13)).  Results do not depend on it. */
int rsrgan_d_step(rsrgan_handle h, const float* x, const float* labels, const int32_t* lengths,
                  int32_t T, const float* noise_real, const float* noise_fake,
                  float* out_losses, int32_t train, void* stream);

/* sess.run([model.g_opt, model.g_adv_losses, model.g_mse_losses, model.g_l2_losses,
 *           model.g_losses], feed) (train_gan_rnn_placeholder.py:94-101).
 * out_losses: DEVICE float[4] = {g_adv, g_mse, g_l2, g_loss}.
 * reuse_g_forward=1: the generator forward of the immediately preceding
 * rsrgan_d_step / rsrgan_d_backward on the SAME batch is still valid (G did not
 * change in between) and is not recomputed. */
int rsrgan_g_step(rsrgan_handle h, const float* x, const float* labels, const int32_t* lengths,
                  int32_t T, const float* noise_fake, float* out_losses,
                  int32_t train, int32_t reuse_g_forward, void* stream);

/* Data-parallel split of the two steps (gan_rnn_placeholder.py:164-184):
 *   *_backward  = per-tower compute_gradients (:169,:173) into the gradient
 *                 buffer, losses as above;
 *   caller      = average_gradients over towers (utils/ops.py:343-376) as an
 *                 RCCL all-reduce(avg) of rsrgan_grad_buffer();
 *   *_apply     = clip_by_norm per tensor (:178-182) then apply_gradients
 *                 (:183-184) and the EMA (:185-186). */
int rsrgan_d_backward(rsrgan_handle h, const float* x, const float* labels, const int32_t* lengths,
                      int32_t T, const float* noise_real, const float* noise_fake,
                      float* out_losses, void* stream);
int rsrgan_g_backward(rsrgan_handle h, const float* x, const float* labels, const int32_t* lengths,
                      int32_t T, const float* noise_fake, float* out_losses,
                      int32_t reuse_g_forward, void* stream);
int rsrgan_apply(rsrgan_handle h, int32_t net, void* stream);
/* device pointer + float count of the (padded) flat gradient buffer of `net`;
 * padding entries are always zero, so it can be all-reduced as one message. */
int rsrgan_grad_buffer(rsrgan_handle h, int32_t net, float** ptr, int64_t* count);
/* Gradient buckets (average_gradients iterates per variable, utils/ops.py:356-375): the flat buffer as
 * contiguous float ranges [offset, offset+count) listed in the order the backward pass completes them (generator, merged
 * wavefront backward: output FC, input FC, LSTM layer 0..L-1; otherwise one bucket = the whole buffer).  The ranges tile
 * the buffer exactly.  rsrgan_grad_bucket_wait makes `stream` wait (hipStreamWaitEvent) until bucket i of the most recent
 * *_backward on this handle is final, so the caller can all-reduce bucket i on a communication stream while the weight
 * gradients of the later buckets are still being computed. */
int rsrgan_grad_bucket_count(rsrgan_handle h, int32_t net);
int rsrgan_grad_bucket_info(rsrgan_handle h, int32_t net, int32_t i, int64_t* offset, int64_t* count);
int rsrgan_grad_bucket_wait(rsrgan_handle h, int32_t net, int32_t i, void* stream);

/* Live timing of the dominant kernel (k_fwd_gates: LSTMCell gates + cell update of every (layer, t) job of a wavefront
 * diagonal) for bench.py's roofline object: between rsrgan_profile_begin and rsrgan_profile_read every launch of that
 * kernel is bracketed by HIP events on the stream it runs on; read returns the launch count, the summed event time and
 * the summed algorithmic FLOPs (2*N*(I+P)*4H per job; the layer-0 x-part is excluded when it was batched into a GEMM). */
int rsrgan_profile_begin(rsrgan_handle h);
int rsrgan_profile_read(rsrgan_handle h, int32_t* launches, double* total_us, double* alg_flops);
/* the same window for another kernel class: kind 0 = k_fwd_gates (as above), kind 1 = k_glstm_fwd, the persistent launch that runs the
 * generator's whole forward recurrence (csrc/gpersist.hip; algorithmic FLOP = every layer's input product -- layer 0's included: it runs
 * inside the launch since round 4 --, recurrent product and projection, over the CALLER's rows: padding rows of a row-padded model do
 * not count), kind 2 = k_glstm_bwd, its BPTT (state-gradient product, dh = dm . W_p^T, the input-gradient product
 * above layer 0; in the G-run the launch is k_glstm_bwd_dt, which also carries the discriminator's BPTT in its trailing form,
 * csrc/dpersist_dev.h: that half's state- and input-gradient products, dh = dm . W_p^T and dy . W_out^T are counted too), kind 3 =
 * k_glstm_fwd_dt, the forward launch with D(G(x)) trailing inside it (the D-run under RSRGAN_DPIPE, every G-run that recomputes the
 * forward): the NUMBER of launches only (total_us and alg_flops come back 0).  Kinds 4..8 are counts only as well (counted on the host
 * where the launch is enqueued): 4 = the stand-alone discriminator forward launches (k_dlstm_fwd, k_dlstm_fwd_t, D(real) under
 * RSRGAN_DPIPE), 5 = the stand-alone discriminator BPTT launches (k_dlstm_bwd), 6 = those of kind 5 that carry the weight-gradient
 * workgroups inside the launch, 7 = k_glstm_np_fwd and 8 = k_glstm_np_bwd (the unprojected generator's forward and BPTT launches).
 * Call before rsrgan_profile_read (which closes the window). */
int rsrgan_profile_read_kind(rsrgan_handle h, int32_t kind, int32_t* launches, double* total_us, double* alg_flops);

/* Health of the persistent recurrence kernels (csrc/dpersist.hip, csrc/gpersist.hip): synchronises the handle's stream and returns in
 * *code 0, or 1 + the first workgroup whose bounded wait for another workgroup's partials expired -- of a discriminator launch as is,
 * of a generator launch (k_glstm_fwd / k_glstm_bwd; in k_glstm_bwd_dt each half reports as its own kind) with 0x10000 added -- and clears the (sticky) device word.  A failed launch has
 * already poisoned its step's losses with NaN.  A failure means the launch's workgroups were not all resident at once (CUs taken
 * away after rsrgan_create, which asks the device how many it can hold: csrc/gpersist.hip resident_probe): the handle re-arms its
 * hand-off rings and takes the launch-per-phase path for that recurrence from then on.  Nothing in the reference corresponds to this. */
int rsrgan_device_status(rsrgan_handle h, int32_t* code);

/* The device memory this handle owns, in bytes: the sum of its device allocations (parameters, activations and stashes, workspaces,
 * hand-off rings, control blocks, chunk tables).  Works on every handle; hipMemGetInfo is device-wide and says nothing about one
 * handle on a shared device. */
int rsrgan_device_bytes(rsrgan_handle h, int64_t* bytes);

/* tf.nn.dropout(h, keep_prob) after every hidden ReLU of the frame-level nets (models/dnn.py:86,99,116-121 and
 * models/discriminator_dnn.py:68,81,100-105; `--keep_prob` of scripts/train_gan_dnn.py).  0 < keep_prob <= 1.  As in the
 * reference it only acts in training runs with l2_scale > 0 (dnn.py:67-71 resets keep_prob to 1.0 otherwise).  `seed` selects
 * the mask stream (give every rank its own); masks change with every training run.
 * On the sequence model it is tf.contrib.rnn.DropoutWrapper(cell, output_keep_prob=keep_prob) around every generator layer
 * (models/lstm.py:99-102, models/res_lstm_l.py:96-99; the discriminator has none): the output of (layer, t) that feeds the layer
 * above / the output FC / the residual sum is dropped, the carried state is not; is_training only, no l2_scale condition
 * (lstm.py:71-72).  RSRGAN_ERR_INVALID for generator layers without a projection. */
int rsrgan_set_dropout(rsrgan_handle h, float keep_prob, uint64_t seed);

/* launches of the recurrence kernels (gates / projection / backward A, B, B-reduce) the host issued since rsrgan_profile_begin: with the
 * floor of a dependent launch (rsrgan_op_launch_floor) this is the serial-recurrence latency bound SURVEY 8d asks bench.py to report */
int rsrgan_profile_launches(rsrgan_handle h, int64_t* n);
/* microseconds per launch of a replayed hipGraph of n dependent 256-workgroup launches: mode 0 = empty kernels (the kernel boundary),
 * mode 1 = each reads 1 KB per wave of what its predecessor wrote and stores it back (one dependent operand round trip) */
int rsrgan_op_launch_floor(int32_t n, int32_t mode, double* us_per_launch, void* stream);

/* ---- low-level operator entry points (unit parity tests + micro-benchmarks) ----
 * Every rsrgan_op_* entry of this header is csrc/capi_ops.cpp's, apart from the product's ABI in csrc/capi.cpp; none takes a handle.
 * Python reaches them through rsrgan_amd.ops.OpEntries.
 * C[M,N] = op(A)*op(B) (+bias) with fp32 MFMA.  a_kcontig: A is [M,K] row-major
 * (else stored [K,M]); b_kcontig: B is stored [N,K] (else [K,N] row-major).
 * All leading dimensions must be multiples of 4 floats, pointers 16-byte aligned.
 * act: 0 none, 1 leaky-relu(alpha).  accumulate: C += result. */
int rsrgan_op_gemm(const float* A, int32_t lda, int32_t a_kcontig,
                   const float* B, int32_t ldb, int32_t b_kcontig,
                   float* C, int32_t ldc, int32_t M, int32_t N, int32_t K,
                   const float* bias, int32_t act, float alpha, int32_t accumulate, void* stream);

/* The entries below exist for the unit parity tests only (tests/test_gpu_wgrad_ops.py, tests/test_op_args.py); no trainer calls them.
 * Each goes through the host launch function the model calls, with a private workspace of the model's size (32 Mi floats).  Every
 * argument error -- a null pointer, a leading dimension that is no multiple of 4, a table size outside the table, A2 together with
 * a_kcontig, M1 % 4 != 0 -- returns RSRGAN_ERR_INVALID before the first HIP call, rsrgan_last_error() naming it.
 *
 * rsrgan_op_gemm2: rsrgan_op_gemm over the stacked operand [A | A2] (A stored [K][M1], A2 [K][M - M1]; A2 NULL: none) and / or a
 * row map of A (map_rows_per > 0: row r of A is at A + (r / rows_per) * outer + (r % rows_per) * inner -- a window view of a
 * [samples][positions][channels] activation; with a_kcontig the mapped index is the row m, without it the reduction index k).
 * workers: worker slots of the stream-K launch for this call (0: the default, 256).  force_cfg: -1 = the planner's choice; 0..7 =
 * that tile form (k_gemm 128x128, 96x128, 128x96, 256x64, 256x32; k_gemm_s 256x256, 128x256, 256x128) whatever the routing rule and
 * the cost model say. */
int rsrgan_op_gemm2(const float* A, int32_t lda, int32_t a_kcontig, const float* A2, int32_t lda2, int32_t M1,
                    const float* B, int32_t ldb, int32_t b_kcontig, float* C, int32_t ldc, int32_t M, int32_t N, int32_t K,
                    const float* bias, int32_t act, float alpha, int32_t accumulate,
                    int32_t map_rows_per, int64_t map_outer, int64_t map_inner, int32_t workers, int32_t force_cfg, void* stream);
/* nb same-shaped products C[b] (+)= [A[b] | A2[b]]^T-style (operands [K][M1 | M - M1], [K][N]) as ONE stream-K launch.  Returns
 * RSRGAN_OP_NOT_APPLICABLE (nothing launched, C untouched: the caller runs them one by one) for nb < 2, nb > 4 and products below the
 * routing threshold of the stream-K kernels; RSRGAN_OK when it launched. */
#define RSRGAN_OP_NOT_APPLICABLE 1
int rsrgan_op_gemm_batch(int32_t nb, const float* const* A, int32_t lda, const float* const* A2, int32_t lda2, int32_t M1,
                         const float* const* B, int32_t ldb, float* const* C, int32_t ldc, int32_t M, int32_t N, int32_t K,
                         int32_t accumulate, int32_t workers, void* stream);
/* n = 1..4 same-shaped products on the split-K kernel in one launch (+ one reduce launch) */
int rsrgan_op_gemm16_batch(int32_t n, const float* const* A, int32_t lda, const float* const* A2, int32_t lda2, int32_t M1,
                           const float* const* B, int32_t ldb, float* const* C, int32_t ldc, int32_t M, int32_t N, int32_t K,
                           int32_t accumulate, void* stream);
/* what the calling thread's last GEMM launch was: out = { kernel class (1 gemm16, 2 n32, 3 k_gemm, 4 k_gemm_s, 5 gemm16 batch,
 * 6 k_gemm batch, 7 k_gemm_s batch; 0: none yet), BM, BN, W, n_dp, 1 if a fix-up launch followed, split-K factor, Ur } */
int rsrgan_op_gemm_last_plan(int32_t out[8]);
/* LSTM bias / peephole column sums of nb = 1..4 layers: db[4H] = colsum(dz [rows][4H]); dwi = colsum(dz_i * cprev), dwf =
 * colsum(dz_f * cprev), dwo = colsum(dz_o * ccur) (cprev, ccur [rows][H]).  nb = 1: the single-layer launch; nb > 1: the batch. */
int rsrgan_op_lstm_colsums(int32_t nb, const float* const* dz, const float* const* cprev, const float* const* ccur, float* const* db,
                           float* const* dwi, float* const* dwf, float* const* dwo, int32_t rows, int32_t H, void* stream);
/* out[c] = sum_r a[r * lda + c] * (b ? b[r * ldb + c] : 1); tall != 0: the tall-and-narrow form (b must be NULL) */
int rsrgan_op_colsum(const float* a, int32_t lda, const float* b, int32_t ldb, float* out, int32_t rows, int32_t cols, int32_t tall,
                     void* stream);
/* the decode-time fold of one BNLSTMCell (csrc/bnlstm.hip k_bnl_fold).  Wx = input_kernel, Wh = state_kernel [P][4H];
 * bn = {scale, offset, moving_mean, moving_var} x {input [4H], state [4H], cell [H]}; bias [4H].  With g = scale / sqrt(moving_var + 1e-3):
 * KxT [4H][ldI] row col = g_in[col] * Wx[:, col] and KhT [4H][ldP] likewise with g_st (columns [P, ld) zero), bias_f [4H] = bias +
 * (offset_in - g_in mean_in) + (offset_st - g_st mean_st), ca [H] = g_cell, cb [H] = offset_cell - g_cell mean_cell.  DEVICE pointers. */
int rsrgan_op_bnl_fold(const float* Wx, const float* Wh, const float* const bn[12], const float* bias, int32_t P, int32_t H, float* KxT,
                       int32_t ldI, float* KhT, int32_t ldP, float* bias_f, float* ca, float* cb, void* stream);

/* ---- the implicit-GEMM convolution of the R-CED generator (csrc/conv.hip).  Unit parity tests only (tests/test_gpu_conv_ops.py,
 * tests/test_op_args.py); no trainer calls them.  Each goes through the host launch function Model::rced_forward / rced_backward
 * call and never launches a kernel directly.  Layout: NHWC, `in` [R*S*W][ldc_in] (R frames of S rows x W columns, C channels; C = 1:
 * ldc_in = 4 as the model's expanded input), kernel [S, fw] over the whole height, stride 1, SAME.  A null pointer, a leading dimension
 * that is no multiple of 4 or shorter than its padded row, a misaligned pointer or bias (16 bytes for in, out, mask, bias, d and ws --
 * the kernels move them as float4 --, 4 bytes for dW and db, which the reducer stores as scalars), R < 1, R > R_max, more than 2^24
 * positions R*S*W (the entries' own limit: far above any test, far below the 32-bit offsets of the kernels) or a short workspace returns
 * RSRGAN_ERR_INVALID before the first HIP call, rsrgan_last_error() naming it.  rsrgan_op_conv_fwd keeps one prepared-filter buffer per
 * calling thread, grown on demand and never freed.  A shape the implicit kernels do not cover returns
 * RSRGAN_OP_NOT_APPLICABLE with nothing launched and the outputs untouched (the model then takes the patch-matrix path).
 *
 * rsrgan_op_conv_fwd: launch_conv_prep into a private buffer, then launch_conv_fwd.  flip = 0: out[.., N] = conv(in[.., C], F) (+ bias)
 * (relu), F [S*fw*C][ldf] with N columns as the model stores a layer C -> N.  flip = 1: the data gradient of a layer N -> C: `in` is the
 * gradient of its output (C channels), F its filter [S*fw*N][ldf] with C columns, out the gradient of its input (N channels).
 * mask (may be NULL) [R*S*W][ldc_out]: out = 0 where mask <= 0.  Columns [N, ldc_out) of out are never written. */
int rsrgan_op_conv_fwd(const float* in, int32_t ldc_in, int32_t C, const float* F, int32_t ldf, int32_t flip, const float* bias, int32_t relu,
                       const float* mask, float* out, int32_t ldc_out, int32_t N, int32_t R, int32_t S, int32_t W, int32_t fw, void* stream);
/* dW [S*fw*C][ldw] = the weight gradient of a layer C -> N from its input `in` and output gradient d [R*S*W][ldc_d]; db (may be NULL)
 * [N] = the column sums of d.  ws: a caller-owned workspace of ws_floats >= rsrgan_op_conv_ws_floats(C, R_max, S, W, fw) floats. */
int rsrgan_op_conv_wgrad(const float* in, int32_t ldc_in, int32_t C, const float* d, int32_t ldc_d, int32_t N, float* dW, int32_t ldw, float* db,
                         float* ws, int64_t ws_floats, int32_t R_max, int32_t R, int32_t S, int32_t W, int32_t fw, void* stream);
/* conv_wgrad_ws_floats: the workspace for any frame count 1 .. R_max (negative: an argument error).  No device needed. */
int64_t rsrgan_op_conv_ws_floats(int32_t C, int32_t R_max, int32_t S, int32_t W, int32_t fw);
/* bit 0: conv_fwd_supported(C, N, S, W, fw), bit 1: conv_wgrad_supported (negative: an argument error).  No device needed. */
int rsrgan_op_conv_supported(int32_t C, int32_t N, int32_t S, int32_t W, int32_t fw);
/* what the calling thread's last rsrgan_op_conv_fwd / _wgrad launched: out[0] = launches (0: not applicable; forward: 1 or 2 = the
 * row-aligned main launch and its remainder; weight gradient: 1), then 19 values per launch: kernel family (1 k_conv_fwd<RT, NT>,
 * 2 k_conv_fwd4<G, NCG, KS>, 3 k_conv_wgrad<KT, NT, 16, DH>, 4 k_conv_wgrad4<NCG, 3, NWV>), its three template arguments in that order,
 * branch (forward: 1 whole width, 2 row-aligned main, 3 remainder; weight gradient, the rule of wgrad_plan that set DH: 1 two k'-tile
 * rounds, 2 six or four rows, 3 searched over 1..3), TW, FB, grid x, y, z, LDS bytes, DH, fpg, groups, nstrips, nkg, PS, waves, gmax
 * (the last eight: weight gradient only) */
int rsrgan_op_conv_last_plan(int32_t out[40]);

/* ---- batch_norm(renorm=True) of the frame-level nets (csrc/bn.hip).  Unit parity tests only (tests/test_gpu_bn_ops.py,
 * tests/test_op_args.py); no trainer calls them.  Each goes through the host launch function the model calls (launch_bn_forward,
 * launch_bn_backward, launch_bn_commit_many, launch_bn_commit) on caller-owned buffers.  vars: the layer's eight device pointers in
 * the order beta, gamma, moving_mean, moving_variance, renorm_mean, renorm_mean_weight [1], renorm_stddev, renorm_stddev_weight [1].
 * z, y, dy: [calls * rows][ld] (the calls are consecutive row blocks); stat: [calls][6][ldc] (mean, stddev, r, d, a, b per call;
 * training = 0 writes rows 4 and 5 only); sums: [2][ldc]; scratch: scratch_floats floats of partial sums.  Contract of the padding
 * columns [cols, pad4(cols)): the caller keeps them 0 in z, dy and stat (the kernels never write them in stat or sums), sums may hold
 * any FINITE value there (it is multiplied by a = 0), y and dz come out 0 there on the sliced and narrow routes and are not written
 * on the small route.  RSRGAN_ERR_INVALID before the first HIP call, rsrgan_last_error() naming it, for: a null required pointer (dbeta
 * and dgamma may both be NULL, not one of them); z, y, dy, stat or sums not 16-byte aligned (moved as float4) or any other pointer not
 * 4-byte aligned; a leading dimension that is no multiple of 4 or below pad4(cols); rows, cols or calls < 1; calls * rows above
 * 2^30; scratch_floats < 2 * cols (one slice of partial sums: with less the kernels would write past the buffer). */
int rsrgan_op_bn_forward(const float* z, int32_t ldz, float* y, int32_t ldy, int32_t rows, int32_t cols, int32_t calls,
                         float* const* vars, float* stat, int32_t ldc, int32_t training, int32_t relu, float* scratch,
                         int64_t scratch_floats, void* stream);
/* dy: the gradient of y (after its ReLU when relu), overwritten by the gradient of z.  accumulate: add to dbeta / dgamma. */
int rsrgan_op_bn_backward(float* dy, int32_t ldd, const float* y, int32_t ldy, const float* z, int32_t ldz, int32_t rows, int32_t cols,
                          int32_t calls, const float* stat, int32_t ldc, float* dbeta, float* dgamma, int32_t accumulate, int32_t relu,
                          float* sums, float* scratch, int64_t scratch_floats, void* stream);
/* The sequence form (csrc/bn_seq.hip; tests/test_gpu_bn_seq_ops.py): one call of the same layer followed by a leaky-ReLU of slope
 * alpha (relu = 0: no activation, y is not read by the backward pass), under the row rule of a padded time-major batch: row r counts
 * iff Bp == 0 || r % Bp < Bt.  The moments and the backward sums run over the counted rows (n of them); y and dz are written as exact
 * zeros on the other rows whatever z and dy hold there.  Arguments, layouts, padding-column contract and refusals are those of
 * rsrgan_op_bn_forward / _backward (y and dz come out 0 in the padding columns); refused in addition: alpha outside [0, 1], a row
 * rule other than Bp = Bt = 0 or 1 <= Bt <= Bp, rows no multiple of Bp.  The backward pass also writes sums = [s1 / n, s2 / n]. */
int rsrgan_op_bn_seq_forward(const float* z, int32_t ldz, float* y, int32_t ldy, int32_t rows, int32_t cols, float* const* vars,
                             float* stat, int32_t ldc, int32_t training, int32_t relu, float alpha, int32_t Bp, int32_t Bt,
                             float* scratch, int64_t scratch_floats, void* stream);
int rsrgan_op_bn_seq_backward(float* dy, int32_t ldd, const float* y, int32_t ldy, const float* z, int32_t ldz, int32_t rows,
                              int32_t cols, const float* stat, int32_t ldc, float* dbeta, float* dgamma, int32_t accumulate,
                              int32_t relu, float alpha, int32_t Bp, int32_t Bt, float* sums, float* scratch, int64_t scratch_floats,
                              void* stream);
/* the update ops of n = 1..24 layers in one launch (launch_bn_commit_many): entry i has vars[8 * i .. 8 * i + 7], stat[i] and
 * dims[4 * i ..] = cols, ldc, times0, times1 (statistics slot 0 applied times0 times, then slot 1 times1 times).  single != 0: n = 1
 * and times1 = 0 through launch_bn_commit.  Refused: n outside 1..24, a null pointer, negative times, cols < 1, ldc % 4 or
 * ldc < pad4(cols), single with n != 1 or times1 != 0. */
int rsrgan_op_bn_commit(int32_t n, float* const* vars, const float* const* stat, const int32_t* dims, int32_t single, void* stream);
/* what the calling thread's last rsrgan_op_bn_forward / _backward launched: out = { route (1 small: k_bn_fwd_small / k_bn_bwd_small,
 * 2 sliced: k_bn_stats1/2 + k_bn_apply, k_bn_bwd1/2/3, 3 narrow: k_bn_part_narrow + k_bn_elem_narrow; 0: none yet), 1 if backward,
 * calls, kernel launches of all calls, slices, rows per slice, partial-sum grid x, y, elementwise grid, q = ld / 4 and R = 256 / q
 * (narrow only), 0.. }; with calls > 1 launched call by call the fields are those of the call launched last (forward: call 0, launched
 * after calls 1 .. n-1; backward: call n-1) */
int rsrgan_op_bn_last_plan(int32_t out[16]);

/* ---- the feature front end of the sequence recipes on the device (csrc/feat.hip): global CMVN (io_funcs/make_tfrecords.py:84-87),
 * Kaldi-style splicing (io_funcs/tfrecords_io.py:177-203), zero padding to T (io_funcs/tfrecords_dataset.py:139-175).  One launch; no
 * handle.  raw [raw_rows][D]: the utterances' raw frames, packed; offsets [B + 1]: utterance b is rows offsets[b] .. offsets[b + 1] - 1,
 * n_b = offsets[b + 1] - offsets[b].  With Dout = D * (left + 1 + right):
 *   out[b, t, c * D + d] = norm(raw[offsets[b] + clamp(t + c - left, 0, n_b - 1), d])   for t < min(n_b, T), c = 0 .. left + right
 *   out[b, t, :]         = 0                                                            for t >= min(n_b, T), every t when n_b <= 0
 *   lengths[b]           = min(max(n_b, 0), T)
 *   norm(v)              = mean ? (float)(((double)v - mean[d]) / stddev[d]) : v
 * Columns: left contexts far to near, the centre, right contexts near to far (io.features.splice_feats).  The context is clamped at the
 * utterance's own first and last frame, not at T: truncation never invents a repeated frame.  The arithmetic is IEEE double
 * subtraction and division and one rounding to float, which is what the host path computes (io.features.apply_cmvn): the results are
 * equal bit for bit.  Source rows are additionally clamped into [0, raw_rows): the kernel is memory-safe whatever the device-resident
 * offset table holds.  All pointers are DEVICE pointers; mean and stddev ([D] double) are both given or both NULL; lengths may be NULL.
 * RSRGAN_ERR_INVALID before the first HIP call, rsrgan_last_error() naming the argument, for: a null raw, offsets or out; only one of
 * mean / stddev; raw or out not 16-byte aligned; offsets or lengths not 4-byte, mean or stddev not 8-byte aligned; B, T, D or raw_rows
 * below 1; left or right negative.  Limits, refused alike: left or right above 1024; B * T * D * (left + 1 + right) above 2^32 - 1
 * elements (a 16 GiB batch: the kernel divides flat indices in 32 bits); raw_rows * D above 2^40. */
int rsrgan_feat_batch(const float* raw, int64_t raw_rows, const int32_t* offsets, int32_t B, int32_t T, int32_t D, int32_t left,
                      int32_t right, const double* mean, const double* stddev, float* out, int32_t* lengths, void* stream);
/* The frame-level recipes' form (io_funcs/tfrecords_io.py:206-255: batches of single spliced frames drawn from a shuffle queue): the
 * queue's utterances stay resident in pool [pool_rows][D] and one launch gathers the N drawn frames.  picks [N][3] = (row, lo, hi): the
 * pool row of the frame and the pool row range [lo, hi) of the utterance it belongs to.  With Dout = D * (left + 1 + right):
 *   out[i, c * D + d] = norm(pool[clamp(clamp(row + c - left, lo, hi - 1), 0, pool_rows - 1), d])   if hi > lo
 *   out[i, :]         = +0.0                                                                        if hi <= lo
 *   norm(v)           = mean ? (float)(((double)v - mean[d]) / stddev[d]) : v
 * Columns as above; the context is clamped at the utterance's own first and last frame; the outer clamp makes the kernel memory-safe
 * whatever the device-resident table holds.  The same row may appear in any number of picks, in any order.  mean = stddev = NULL reads
 * a pool that already holds normalised frames (what HipEngine.featurize_frames keeps); with statistics the arithmetic is that of
 * rsrgan_feat_batch.  All pointers are DEVICE pointers.  RSRGAN_ERR_INVALID before the first HIP call, rsrgan_last_error() naming the
 * argument, for: a null pool, picks or out; only one of mean / stddev; pool or out not 16-byte aligned; picks not 4-byte, mean or
 * stddev not 8-byte aligned; N, D or pool_rows below 1; left or right negative or above 1024; N * D * (left + 1 + right) above
 * 2^32 - 1 elements; pool_rows * D above 2^40. */
int rsrgan_feat_frames(const float* pool, int64_t pool_rows, const int32_t* picks, int32_t N, int32_t D, int32_t left, int32_t right,
                       const double* mean, const double* stddev, float* out, void* stream);
/* The live path's form (rsrgan_amd/stream.py StreamBank): streaming append and splice on a device-resident ring, one launch, no handle.
 * hist [B][H][D] holds each row's NORMALISED frames, utterance frame j of row r in slot j mod H (mod: the non-negative remainder);
 * fresh [fresh_rows][D] holds the raw frames that arrived with this call, packed over all rows; table [B][6] =
 * (src, app0, napp, emit0, nemit, last) per row.  With Dout = D * (left + 1 + right):
 *   append:  hist[r][(app0 + i) mod H][d] = norm(fresh[clamp(src + i, 0, fresh_rows - 1)][d])      i in [0, napp)
 *   emit:    out[r, t, c * D + d] = hist'[r][clamp(emit0 + t + c - left, 0, last) mod H][d]         t < min(nemit, T)
 *            out[r, t, :]         = +0.0                                             otherwise (every t when nemit <= 0 or last < 0)
 *            lengths[r]           = clamp(nemit, 0, T)
 *   norm(v)  = mean ? (float)(((double)v - mean[d]) / stddev[d]) : v
 * hist' is the ring after this call's append: the emit behaves as if the append had happened first.  Columns as above.  The clamp at 0
 * and at `last` is the utterance's own edge (a caller that never asks for a frame whose right context is incomplete makes the clamp at
 * `last` inert until the utterance ends, where it repeats the last frame).  Negative napp or nemit count as 0; with fresh_rows == 0
 * every napp counts as 0 (a flush-only call); where napp > H the last write to a slot stands.  Normalising once on append and gathering
 * fp32 afterwards gives the host path's bits.  With these rules and the clamp on `fresh`, the kernel reads and writes nothing outside
 * its buffers, whatever the table holds.  The values are the utterance's only while the window fits the ring,
 * last - (emit0 - left) + 1 <= H with emit0 - left <= app0 and app0 + napp - 1 <= last: that is the caller's to keep.  All pointers are
 * DEVICE pointers; lengths may be NULL; mean and stddev ([D] double) are both given or both NULL.  RSRGAN_ERR_INVALID before the first
 * HIP call, rsrgan_last_error() naming the argument, for: a null table, hist or out; a null fresh unless fresh_rows == 0; only one of
 * mean / stddev; fresh, hist or out not 16-byte aligned; table or lengths not 4-byte, mean or stddev not 8-byte aligned; B, H, T or D
 * below 1; fresh_rows negative; left or right negative or above 1024; B * T * D * (left + 1 + right) or B * H * D above 2^32 - 1
 * elements; fresh_rows * D above 2^40. */
int rsrgan_feat_stream(const float* fresh, int64_t fresh_rows, const int32_t* table, float* hist, int32_t B, int32_t H, int32_t T, int32_t D,
                       int32_t left, int32_t right, const double* mean, const double* stddev, float* out, int32_t* lengths, void* stream);
/* The output side: de-normalise G(x) y [B][T][D] (fp32) with the label statistics into out [B][T][D] (fp64), one launch, no handle:
 *   out[b, t, d] = t < len_b ? fl64(fl64((double)y[b, t, d] * stddev[d]) + mean[d]) : 0.0     len_b = lengths ? clamp(lengths[b], 0, T) : T
 * The product and the sum are rounded separately, which is what NumPy's `y * stddev + mean` computes on a float32 array and float64
 * statistics: the results are equal bit for bit (a fused multiply-add would give other bits).  All pointers are DEVICE pointers;
 * lengths may be NULL.  RSRGAN_ERR_INVALID before the first HIP call, rsrgan_last_error() naming the argument, for: a null y, out, mean or
 * stddev; y not 16-byte aligned; lengths not 4-byte aligned; mean, stddev or out not 8-byte aligned; B, T or D below 1; B * T * D above
 * 2^32 - 1 elements. */
int rsrgan_feat_denorm(const float* y, const int32_t* lengths, int32_t B, int32_t T, int32_t D, const double* mean, const double* stddev,
                       double* out, void* stream);
/* The archive side: decode a batch of utterances from their Kaldi archive encoding into NORMALISED float32 rows out [out_rows][D], one
 * launch, no handle.  blob: the matrices' bytes as they lie in the file; seg [B][2] = (byte offset of utterance b's segment in blob, kind);
 * scale [B][2] = (min, range), read for kind 2 only; offsets [B + 1]: utterance b has n_b = offsets[b + 1] - offsets[b] frames and goes
 * to rows offsets[b] .. offsets[b + 1] - 1 of out.  Element (j, d), j < n_b, in IEEE double, no multiply-add:
 *   kind 0 ('BFM ', float  [n][D] row-major):  x = (double)f32[j * D + d]
 *   kind 1 ('BDM ', double [n][D] row-major):  x = f64[j * D + d]
 *   kind 2 ('BCM ', Kaldi compressed format 1: 4 * D little-endian uint16 percentiles, then D * n bytes, column-major):
 *            p_k = min + ((range * 1.52590218966964e-05) * (double)u16[4 * d + k])          k = 0 .. 3; min, range widened to double
 *            v   = (double)byte[d * n + j]
 *            x   = v <  64  ? p_0 + ((p_1 - p_0) *  v       ) * (1 / 64.0)
 *                : v <= 192 ? p_1 + ((p_2 - p_1) * (v -  64)) * (1 / 128.0)
 *                :            p_2 + ((p_3 - p_2) * (v - 192)) * (1 / 63.0)              (1 / 63.0: the rounded constant, multiplied)
 *   out[offsets[b] + j][d] = mean ? (float)((x - mean[d]) / stddev[d]) : (float)x
 * These are io.kaldi_ark's uint16_to_float and char_to_float, io.features.apply_cmvn and the reader's cast to float32: the results are
 * equal to the host path's bit for bit; the decoded value is never rounded to float before it is normalised.  out is then an ordinary
 * `raw` / `pool` for rsrgan_feat_batch / rsrgan_feat_frames with mean = stddev = NULL.  Rows of out that belong to no utterance are not
 * written; n_b <= 0 writes nothing; an unknown kind writes +0.0.  Every byte index is clamped into [0, blob_bytes) and every destination
 * row into [0, out_rows): the kernel reads and writes nothing outside its buffers, whatever the device-resident tables hold.  All
 * pointers are DEVICE pointers; mean and stddev ([D] double) are both given or both NULL.  RSRGAN_ERR_INVALID before the first HIP call,
 * rsrgan_last_error() naming the argument, for: a null blob, seg, offsets or out; a null scale (always required: the kinds are not
 * visible to the host); only one of mean / stddev; blob or out not 16-byte aligned; seg, mean or stddev not 8-byte, scale or offsets not
 * 4-byte aligned; B, D, blob_bytes or out_rows below 1; out_rows * D above 2^40. */
int rsrgan_feat_decode(const uint8_t* blob, int64_t blob_bytes, const int64_t* seg, const float* scale, const int32_t* offsets, int32_t B,
                       int32_t D, const double* mean, const double* stddev, float* out, int64_t out_rows, void* stream);
/* The waveform side (csrc/wave.hip): PCM samples -> the RAW log-power-spectrum (LPS) rows every other entry starts from,
 * out [out_rows][P / 2 + 1] float32, one launch, no handle.  The definition is Kaldi's compute-spectrogram-feats --dither=0
 * --window-type=hamming with its other defaults, stated here in full.  Constants of the recipes: N = 400 samples per frame (25 ms at
 * 16 kHz), shift S = 160, padded length P = 512, NB = P / 2 + 1 = 257 bins, eps = FLT_EPSILON.
 *   samples      pcm, kind 0: int16, widened to float without scaling (as Kaldi's wave reader does); kind 1: float32, taken as already
 *                on that scale.  Utterance b is samples seg[b] = (first sample, sample count), n = the count.
 *   frame count  F_b = n < N ? 0 : 1 + (n - N) / S  (snip-edges); frame f is samples [f * S, f * S + N) of the utterance.
 *   per frame, on v[0 .. N):
 *     1. v -= (sum v) / N
 *     2. E = log(max(sum v^2, eps))                       the raw energy: before pre-emphasis and before the window
 *     3. v'[i] = v[i] - preemph * v[i - 1] for i >= 1,  v'[0] = v[0] - preemph * v[0]         (the old values on the right)
 *     4. v'[i] *= window[i]
 *     5. zero-pad to P;  X = DFT_P(v');  p_k = |X_k|^2                                         k = 0 .. P / 2
 *     6. out[k] = log(max(p_k, eps)) for k = 1 .. P / 2,  out[0] = E
 *   rows         frame f of utterance b goes to row offsets[b] + f, for f < min(F_b, offsets[b + 1] - offsets[b]); rows that belong to no
 *                utterance are not written.
 * window [N] float32 is the caller's table, so the kernel is window-agnostic (rsrgan_amd/io/wave.py builds Hamming,
 * 0.54 - 0.46 cos(2 pi i / (N - 1)), and Povey, (0.5 - 0.5 cos)^0.85, in fp64 and rounds once).  twiddle [P / 2][2] float32 =
 * (cos, -sin)(2 pi j / P), j < P / 2, built the same way: the kernel calls no sincosf and sums in a fixed order, so a frame has the same
 * bits run to run, whatever its utterance's place in the batch.  Arithmetic: fp32 throughout; the real FFT is a P / 2-point complex FFT
 * (radix 4) and a split pass.  out is then an ordinary `raw` for rsrgan_feat_batch, or `fresh` for rsrgan_feat_stream.  The segment is
 * clamped into [0, n_samples), every sample index too, and every destination row into [0, out_rows): the kernel reads and writes nothing
 * outside its buffers, whatever the device-resident tables hold.  An utterance starts at any sample: pcm is only asked to be aligned
 * to its element.  All pointers are DEVICE pointers.  RSRGAN_ERR_INVALID before the first HIP call, rsrgan_last_error() naming the
 * argument, for: a null pcm, seg, offsets, out, window or twiddle; a kind other than 0 or 1; pcm not aligned to its element size (2 or
 * 4 bytes); out not 16-byte, seg not 8-byte, offsets, window or twiddle not 4-byte aligned; B, n_samples or out_rows below 1; P no
 * power of two in [64, 2048]; not 1 <= S <= N <= P; preemph outside [0, 1] (or NaN); out_rows * (P / 2 + 1) above 2^40. */
int rsrgan_feat_wave(const void* pcm, int32_t kind, int64_t n_samples, const int64_t* seg, const int32_t* offsets, int32_t B, int32_t N,
                     int32_t S, int32_t P, float preemph, const float* window, const float* twiddle, float* out, int64_t out_rows,
                     void* stream);
/* The labels' side of the waveform front end (csrc/wave.hip k_feat_mfcc): PCM samples -> RAW MFCC or log-mel rows,
 * out [out_rows][C ? C : M] float32, one launch, no handle.  The definition is Kaldi's compute-mfcc-feats --dither=0 with the WSJ
 * conf/mfcc_hires.conf (--use-energy=false --num-mel-bins=40 --num-ceps=40 --low-freq=20 --high-freq=-400) and its other defaults: Povey
 * window, pre-emphasis 0.97, DC removal, snip-edges, 25 ms / 10 ms frames, padding to a power of two, cepstral lifter 22.  Samples,
 * frame count and rows are rsrgan_feat_wave's.  Per frame, steps 1, 3, 4 and 5 of rsrgan_feat_wave run unchanged (mean removal,
 * pre-emphasis with the old values, the caller's window, zero padding to P, p_k = |X_k|^2 for k = 0 .. P / 2); the raw energy of step 2 is
 * no part of the output.  Then, with eps = FLT_EPSILON:
 *     6'. m_j = sum_t w_j[t] * p[a_j + t], t = 0 .. n_j - 1 ascending, j < M         the mel energies; filter j covers the contiguous bins
 *                                                                                   [a_j, a_j + n_j) inside [0, P / 2): the Nyquist bin
 *                                                                                   never enters (Kaldi's MelBanks); n_j = 0 gives m_j = 0
 *     7'. l_j = log(max(m_j, eps))
 *     8'. c_i = sum_j dct[i][j] * l_j, j ascending, i < C                            the cepstra.  C = 0 (dct == NULL): the row is l itself,
 *                                                                                   the M log-mel energies (compute-fbank-feats)
 * The filterbank and the DCT are the caller's device tables, as the window and the twiddles are, so the kernel is filterbank-agnostic:
 *   mel_seg [M][3] int32 = (a_j, n_j, the index of w_j[0] in mel_w);  mel_w [nnz] float32;  dct [C][M] float32 row-major, the lifter
 *   multiplied in.
 * rsrgan_amd/io/wave.py builds them in fp64 and rounds once: Mel(f) = 1127 ln(1 + f / 700); M + 2 points equally spaced in mel between
 * Mel(low) and Mel(high) (a high <= 0 is an offset from Nyquist); bin i has frequency i * rate / P and belongs to filter j where
 * left_j < Mel < right_j strictly, with weight (Mel - left) / (centre - left) up to the centre and (right - Mel) / (right - centre) after
 * it; dct row 0 = sqrt(1 / M), row k = sqrt(2 / M) cos(pi / M (n + 1/2) k) (Kaldi's ComputeDctMatrix), row i scaled by the lifter
 * 1 + (Q / 2) sin(pi i / Q), Q = 22 (Q = 0: none).  Kaldi computes its tables in float32 and sums in another order: bit parity with a
 * Kaldi binary is NOT pinned (none was available to compare against); the tests pin the definition above against float64.
 * Arithmetic: fp32 throughout, fixed summation orders, so a frame's bits depend on nothing but its samples and the tables.  Every a_j is
 * clamped into [0, P / 2), n_j into [0, P / 2 - a_j], every weight index into [0, nnz), besides the clamps of rsrgan_feat_wave: the kernel
 * reads and writes nothing outside its buffers, whatever the device-resident tables hold.  Limits: 1 <= M <= 128, 0 <= C <= M,
 * 1 <= nnz <= 8192, and the launch's dynamic LDS -- 4 (P / 2 + nz P / 2) x 2 + 4 (2 N + (F - 1) S) + 4 (nz P / 2 + nz M + M C + 3 M + nnz)
 * bytes with F = rsrgan_feat_wave_frames(P), nz = min(4, F) -- at most 65536 (30.7 KB for 400 / 160 / 512 / 40 / 40 / 468).  All pointers
 * are DEVICE pointers.  RSRGAN_ERR_INVALID before the first HIP call, rsrgan_last_error() naming the argument, for everything
 * rsrgan_feat_wave refuses, and: a null mel_seg or mel_w; dct null with C != 0 or given with C = 0; mel_seg, mel_w or dct not 4-byte
 * aligned; M, C or nnz outside the limits; an LDS need above 65536 bytes (the message holds the count); out_rows * (C ? C : M) above 2^40. */
int rsrgan_feat_mfcc(const void* pcm, int32_t kind, int64_t n_samples, const int64_t* seg, const int32_t* offsets, int32_t B, int32_t N,
                     int32_t S, int32_t P, float preemph, const float* window, const float* twiddle, const int32_t* mel_seg,
                     const float* mel_w, int32_t nnz, int32_t M, const float* dct, int32_t C, float* out, int64_t out_rows, void* stream);
/* The frames one workgroup of rsrgan_feat_wave or rsrgan_feat_mfcc takes (consecutive frames of one utterance, whose overlapping samples
 * it reads once); 0 for a P the entries refuse.  Tests place their utterance lengths around it. */
int rsrgan_feat_wave_frames(int32_t P);
/* Reverberate clean audio on the device (csrc/reverb.hip): what Kaldi's wav-reverberate --impulse-response=..
 * --shift-output --normalize-output [--additive-signals .. --snrs .. --start-times ..] does, as its documentation and the reference's
 * reverberate/ scripts describe it, stated here in full.  No Kaldi source or binary was available to compare against: bit parity with
 * Kaldi is NOT pinned; the tests pin the definition below against float64.
 * Per utterance b: x[0 .. n) its samples seg[b] = (first sample, count) of pcm (kind 0: int16 widened without scaling, kind 1: float32 on
 * that scale); sel[b] = (rir index, noise index, s, m).  RIR r is taps rir_seg[r] = (first tap, L, q, e0, e1) of rir (float32): q the index
 * of the FIRST maximum of h (Kaldi's Vector::Max), [e0, e1) = [max(q - floor(0.001 fs), 0), min(q + floor(0.05 fs), L)) the early part;
 * the host fills them (rsrgan_amd/io/reverb.py rir_table), the kernels take them as given and clamp them.  Noise v is samples
 * noise_seg[v] = (first, nv) of noise (float32) with its power P_v = noise_pow[v] (computed on the host in fp64).
 *   1. P_in = (1 / n) sum x^2
 *   2. y = x * h, full length len = n + L - 1.  rir index -1 (or outside [0, R)): y = x, len = n, q = 0
 *   3. E = (1 / (n + (e1 - e0) - 1)) sum (x * h[e0 .. e1))^2, the early-reverberation energy (e1 = e0: E = 0); without an RIR E = P_in.
 *      It is formed only when a noise is selected
 *   4. noise index -1 (or outside [0, V), or nv = 0): none, g = 0.  Else y[s + i] += g v[i mod nv] for 0 <= i < m, s + i < len, with
 *      g = sqrt(10^(-snr[b] / 10) E / P_v); g = 0 if E = 0 or P_v = 0 (or P_v, g not finite)
 *   5. flags & 2 (normalize): c = sqrt(P_in / P_out), P_out = (1 / len) sum y^2 after the noise; c = 1 if P_out = 0.  Else c = 1
 *   6. out[first_b + i] = c y[i + (flags & 1 ? q : 0)] for i < min(n_out, capacity_b), out_seg[b] = (first, capacity); n_out = n with
 *      flags & 1 (shift), else len.  float32 on the int16 scale, not quantised.  gains[b] = (c, g) if gains is given.
 * Arithmetic: uniformly partitioned overlap-save in fp32.  C is the complex FFT length, a block C / 2 samples; the RIR is cut into
 * ceil(L / (C / 2)) partitions whose spectra are formed per call, per utterance, in `work`; output block k is the inverse transform of
 * sum_p X[k - p] H[p], p ascending; two real blocks ride one complex transform.  twiddle [C][2] float32 = (cos, -sin)(2 pi j / 2 C), j < C
 * (rsrgan_amd/io/wave.py twiddle_table(2 C)): no sincosf.  The sums of squares and the cross term sum y v are fp32 per block in a fixed
 * order and are finished per utterance in fp64 in block order, P_out as sum y^2 + 2 g sum y v + g^2 sum v^2; no atomics: an utterance's
 * output bits depend on its samples, its tables and C only, not on its place in the batch or on B.
 * Clamps: every segment into its buffer, n to 2^28, L to 2^24, q into [0, L), e0 <= e1 into [0, L], s into [0, len], m into
 * [0, len - s], the capacity into out: the kernels read and write nothing outside their buffers, whatever the device-resident tables
 * hold, and utterance b writes min(n_out, capacity_b) samples of out and nothing else there.  work: utterance b owns
 * work + b * (work_bytes / B rounded down to 16); an utterance that needs more than its slot (longer than the n_max, L_max the caller
 * sized for) writes nothing and has gains (1, 0); so does an empty one.  rsrgan_wave_reverb_work(B, n_max, L_max, C): the bytes for B
 * utterances of at most n_max samples against at most L_max taps; 0 for B outside [1, 65535], n_max outside [1, 2^28], L_max outside
 * [0, 2^24] or a C the entry refuses.  No handle, no allocation, nothing synchronises with the host; four launches on `stream`.  All
 * pointers are DEVICE pointers.  RSRGAN_ERR_INVALID before the first HIP call, rsrgan_last_error() naming the argument, for: a null pcm,
 * seg, sel, snr, out, out_seg, twiddle or work; a null rir or rir_seg with R > 0; a null noise, noise_seg or noise_pow with V > 0; B
 * outside [1, 65535]; R or V outside [0, 2^20]; a kind other than 0 or 1; pcm not aligned to its element; work not 16-byte, seg,
 * rir_seg, noise_seg or out_seg not 8-byte, any other pointer not 4-byte aligned; n_samples or out_samples outside [1, 2^40]; n_taps
 * (n_noise) outside [R > 0, 2^40] ([V > 0, 2^40]); C no power of two in [64, 2048]; flags outside [0, 3]; work_bytes below
 * rsrgan_wave_reverb_work(B, 1, 1, C). */
int rsrgan_wave_reverb(const void* pcm, int32_t kind, int64_t n_samples, const int64_t* seg, const float* rir, int64_t n_taps,
                       const int64_t* rir_seg, const float* noise, int64_t n_noise, const int64_t* noise_seg, const float* noise_pow,
                       const int32_t* sel, const float* snr, int32_t B, int32_t R, int32_t V, int32_t C, const float* twiddle, int32_t flags,
                       float* out, int64_t out_samples, const int64_t* out_seg, float* gains, void* work, int64_t work_bytes, void* stream);
int64_t rsrgan_wave_reverb_work(int32_t B, int64_t n_max, int64_t L_max, int32_t C);
/* Audio out (csrc/synth.hip): enhanced LPS rows back to samples -- the magnitude of every frame is replaced by the row's, the
 * phase of the utterance's own (reverberant) samples is kept, the frames are overlap-added with the analysis window and the pre-emphasis
 * is undone.  Kaldi has no such tool: nothing is pinned against a Kaldi binary; the tests pin the definition below against float64.
 * All constants and symbols are rsrgan_feat_wave's: N, S, P, H = P / 2, NB = H + 1, eps = FLT_EPSILON, a = preemph, the caller's window
 * table w [N] and twiddle table [P / 2][2], samples of kind 0 / 1.  Utterance b is the n samples x[0 .. n) of seg[b]; its LPS rows are rows
 * offsets[b] .. offsets[b + 1] of lps [lps_rows][NB] float32: de-normalised natural-log power on the int16 scale, what rsrgan_feat_wave
 * itself would write.  F = min(F_b, offsets[b + 1] - offsets[b], lps_rows - offsets[b]) with rsrgan_feat_wave's frame count F_b.
 *   per frame f < F, on v[i] = x[f S + i], row = offsets[b] + f:
 *     1. m_f = (sum v) / N; v -= m_f; then steps 3, 4, 5 of rsrgan_feat_wave unchanged: X_k (complex) and p_k = |X_k|^2, k = 0 .. H
 *     2. L_k = lps[row][k] clamped into [-80, 80]; a NaN counts as -80
 *     3. g_k = exp((L_k - log max(p_k, eps)) / 2) for k = 1 .. H (not sqrt(exp(L) / p), which overflows fp32); g_0 = g_1: bin 0 of an
 *        LPS row carries the raw energy, not a DC power, so DC follows the lowest bin
 *     4. Y_k = g_k X_k;  y_f[i] = IDFT_P(Y)[i] for i < N (Y is Hermitian by construction: y_f is real)
 *     5. y_f[i] += w[i] (1 - a) m_f g_1: the mean step 1 removed, restored in the pre-emphasised domain with the lowest bin's gain
 *        (preemph(v - m) = preemph(v) - (1 - a) m at every i, the i = 0 rule included)
 *   overlap-add; sample i = 0 of a frame enters neither sum (v'[0] = v[0] - a v[0] disagrees with every other frame on that sample):
 *     num[t] = sum_f w[i] y_f[i],  den[t] = sum_f w[i]^2,  i = t - f S, 1 <= i < N, f ascending (at most ceil(N / S) terms)
 *     z[t] = den[t] > 0 ? num[t] / max(den[t], 1e-3) : 0          the floor: a short fade where a window reaches zero at the utterance's
 *                                                                ends (Povey); Hamming's smallest den is 0.0064
 *   de-emphasis over the utterance: out[t] = z[t] + a out[t - 1], out[-1] = 0, for t < (F - 1) S + N.
 * Samples t >= (F - 1) S + N (no frame covers them) and every sample of an utterance with F = 0 are written as +0.0.  Utterance b writes
 * min(n, capacity_b) samples at out_seg[b] = (first, capacity): float32 on the int16 scale, not quantised; nothing else is written.  So
 * out is linear in exp(L / 2), and with L the utterance's own LPS g = 1 and the chain gives x[t] - a^t x[0] wherever den is above the floor.
 * Arithmetic: fp32 throughout; the inverse transform is the merge pass and the forward FFT on the conjugate; the recurrence runs in chunks
 * of rsrgan_wave_synth_chunk() samples from a zero state (strips per lane, a scan over the lanes, the wavefronts in order), the chunks'
 * end values are carried utterance by utterance (c_{j+1} = e_j + a^CH c_j) and added as a^(i + 1) c_j; powers of a are repeated products
 * in a fixed order.  No sincosf, no atomics: an utterance's bits depend on its samples, its LPS rows, the tables and N, S, P, a only, not
 * on B, its place in the batch or the sample kind.  Every segment, offset, row, sample index and capacity is clamped: the kernels read
 * and write nothing outside their buffers, whatever the device-resident tables hold (out segments that overlap give unspecified values
 * inside out).  work: rsrgan_wave_synth_work(B, lps_rows, out_samples, N) bytes -- lps_rows * N floats (the windowed frames) and
 * ceil(out_samples / CH) + B carries; 0 for B outside [1, 65535], lps_rows or out_samples outside [1, 2^40], N outside [1, 2048].  No
 * handle, no allocation, nothing synchronises with the host; four launches on `stream`.  All pointers are DEVICE pointers.
 * RSRGAN_ERR_INVALID before the first HIP call, rsrgan_last_error() naming the argument, for: a null pcm, seg, offsets, lps, window,
 * twiddle, out, out_seg or work; a kind other than 0 or 1; pcm not aligned to its element; lps or work not 16-byte, seg or out_seg not
 * 8-byte, offsets, window, twiddle or out not 4-byte aligned; B outside [1, 65535]; n_samples, lps_rows or out_samples outside
 * [1, 2^40]; P no power of two in [64, 2048]; not 1 <= S <= N <= P; preemph outside [0, 1] (or NaN); work_bytes below
 * rsrgan_wave_synth_work(B, lps_rows, out_samples, N). */
int rsrgan_wave_synth(const void* pcm, int32_t kind, int64_t n_samples, const int64_t* seg, const int32_t* offsets, const float* lps,
                      int64_t lps_rows, int32_t B, int32_t N, int32_t S, int32_t P, float preemph, const float* window,
                      const float* twiddle, float* out, int64_t out_samples, const int64_t* out_seg, void* work, int64_t work_bytes,
                      void* stream);
int64_t rsrgan_wave_synth_work(int32_t B, int64_t lps_rows, int64_t out_samples, int32_t N);
/* The samples of a scan chunk of rsrgan_wave_synth (CH).  Tests place their utterance lengths around it. */
int rsrgan_wave_synth_chunk(void);

/* ---- TensorBoard histogram summaries on the device (csrc/hist.hip): what tf.summary.histogram's HistogramProto holds,
 * computed where the tensors are.  No handle.  x: a HOST table of n DEVICE pointers to float32 tensors; dims: a HOST table of n x
 * (rows, cols, ld), tensor i being the strided 2-D view x[i][r * ld + c] (ld >= cols; ld = cols: dense).  out (DEVICE): n records of
 * 5 + NL doubles, NL the length of the table rsrgan_hist_limits gives:
 *   [0] min  [1] max  [2] num  [3] sum  [4] sum_squares  [5 + k] the count of bucket k
 * Bucket of a value v, widened to double: the first limit greater than v, clamped to the last bucket (rsrgan_amd/summary.py histogram());
 * -inf counts into the first bucket, +inf and NaN into the last; a NaN makes min, max, sum and sum_squares NaN.  A tensor without
 * elements (rows or cols 0; its pointer may be NULL) yields the record of the single value 0.0.  min, max, num and the counts are exact;
 * sum and sum_squares are fp64 sums in a fixed order: the record has the same bits run to run.  Two launches on `stream`; calls on
 * different streams are ordered against each other by the entry (they share the launches' device memory), so it cannot be captured into
 * a graph.  RSRGAN_ERR_INVALID before any device work, rsrgan_last_error() naming the argument, for: n below 1 or above 16; a null x,
 * dims or out; out not 8-byte aligned; for a tensor: a negative rows, cols or ld; ld below cols; rows x cols above 2^31 - 1; ld above
 * 2^40; a null or not 4-byte aligned pointer where there are elements. */
int rsrgan_hist(int32_t n, const float* const* x, const int64_t* dims, double* out, void* stream);
/* The bucket limits the kernel uses (TensorFlow's defaults: +-1e-12 * 1.1^k by repeated multiplication in double, +-DBL_MAX, 0.0),
 * built once on the host: *n receives their count, out (HOST, may be NULL to ask for the count alone) the limits. */
int rsrgan_hist_limits(double* out, int32_t* n);
/* The discriminator logits of the most recent D-run (rsrgan_d_backward / rsrgan_d_step, training or not) as two dense DEVICE tensors
 * [batch_size][T] float32, batch-major -- the reference's d_rl_logits / d_fk_logits [B, T, 1] (gan_rnn_placeholder.py:219-220): the
 * caller's batch_size rows only (none of the rows that pad a batch to the kernels' row group), every frame including those past a row's
 * length, as the reference's histograms see them.  With d_type dnn the values are the clipped ones discriminator_dnn returns
 * (discriminator_dnn.py:93); a frame-level handle (g_type dnn / rced) has T = 1.  *T receives the frame count; real and fake may both be
 * NULL to ask for it alone.  A G-run overwrites the logits with D(G(x)): call between the D-run and the G-run, in stream order.
 * RSRGAN_ERR_INVALID on an inference handle, on a handle without a discriminator (RSRGAN_FLAG_SUPERVISED) and when no D-run's logits
 * are at hand. */
int rsrgan_d_logits(rsrgan_handle h, float* real, float* fake, int32_t* T, void* stream);
/* rsrgan_hist of those two tensors (record 0: real, record 1: fake) straight from the handle's buffer, without the dense copies.
 * out: DEVICE, 2 x (5 + NL) doubles.  The same refusals. */
int rsrgan_d_logits_hist(rsrgan_handle h, double* out, void* stream);

/* ---- the SEGAN operators (csrc/segan.hip and the window-GEMM primitives of csrc/segan.cpp).  Unit parity tests only
 * (tests/test_gpu_segan_ops.py, tests/test_op_args.py); no trainer calls them.  Each goes through the host function SeganModel calls
 * and never launches a kernel directly.  One entry per family: op selects the launcher; ptrs is a HOST table of device pointers,
 * dims a HOST table of sizes and fl of float parameters, in the order listed ("?" = may be NULL; fl may be NULL where none is listed).
 * Tensors are channels-last [rows = batch x position][channels] fp32.  A null table or required pointer, a misaligned pointer
 * (16 bytes where a kernel moves float4: X, W, Z, dZ, dW, pad, t0, t1, Wt of conv2; z, dz of conv1; S of tconv1; a, b, coef, scratch of
 * colred; pad_rows and interleave operands; 4 bytes elsewhere), a size below 1 (or below 0 for offsets and pads) or above the entry's
 * limit, a leading dimension below its row, a channel count the kernel cannot take, or a scratch below the launcher's need returns
 * RSRGAN_ERR_INVALID before the first HIP call, rsrgan_last_error() naming it: a shape a launcher would abort on is never launched.
 *
 * rsrgan_op_segan_sizes (no device): kind 0, dims Bn, L, C, k: out[0] = the pad floats SeganModel::init gives a conv2_fwd / conv2_wgrad
 * of that layer (its + 64 included).  kind 1, dims Bn, Ls, Cs, Lt, Ct, k (tconv2): out = pad floats, t0 / t1 floats, Wt[0] floats,
 * Wt[1] floats, pl, i0[0], i0[1], Q[0], Q[1], pf, pb.  kind 2, dims k, C: out[0] = 1 if launch_conv1_wgrad's kernel takes the shape
 * (k * C <= 1024, C % 4 == 0), out[1] = its dynamic LDS in bytes.  kind 3, dims C, P: the least scratch of launch_colred. */
int rsrgan_op_segan_sizes(int32_t kind, const int64_t* dims, int64_t out[12]);
/* a bare SeganModel holding exactly pad, t0, t1 and the GEMM workspace (16 Mi floats, the model's), then the method itself.
 * op 0 conv2_fwd:   ptrs X, W, bias?, Z, pad;  dims Bn, L, Cin, k, Cout, ldw, pad_floats.  Z [Bn * ceil(L/2)][Cout] = stride-2 SAME conv.
 * op 1 conv2_wgrad: ptrs X, dZ, dW, pad;  dims Bn, L, Cin, k, Cout, ldz, ldw, pad_floats.  dW [k * Cin][ldw].
 * op 2 tconv2:      ptrs S, W, bias?, T, pad, t0, t1, Wt0, Wt1;  dims Bn, Ls, Cs, Lt, k, Ct, ldw, pad_floats, t_floats, wt0_floats,
 *                   wt1_floats.  W [k * Ct][ldw] with Cs columns is the filter of the downconv Ct -> Cs whose data gradient (= the
 *                   deconv Cs -> Ct) T [Bn * Lt][Ct] is; Wt0 / Wt1 are prepared from it by launch_prep_tconv_many as refresh_weights
 *                   does.  Lt is 2 Ls or 2 Ls - 1.  pad_floats, t_floats, wt*_floats at least rsrgan_op_segan_sizes'. */
int rsrgan_op_segan_conv2(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream);
/* the single-channel ends.
 * op 0 launch_conv1_fwd:   ptrs x, W, bias?, z;  dims B, L, k, C, ldx, ldw, ldz (C % 16 == 0).
 * op 1 launch_conv1_wgrad: ptrs x, dz, dW, scratch;  dims B, L, k, C, ldx, ldz, ldw, scratch_floats (>= B * k * C; k * C <= 1024;
 *                          refused too when the kernel's LDS exceeds the device's, asked once after the argument checks).
 * op 2 launch_tconv1:      ptrs S, W, bias?, t;  dims B, Ls, C, Lt, k, lds, ldw, ldt. */
int rsrgan_op_segan_conv1(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream);
/* launch_colred, mode 0..3: ptrs a, b?, coef?, out, scratch;  dims lda, coff, ldb, C, rows_per, P, ldcoef, ldo, accumulate,
 * scratch_floats (>= P * 2 * C: refused below, the chunk doubles above);  fl leak.  b: modes 1, 3; coef [P * 8][ldcoef]: mode 3. */
int rsrgan_op_segan_colred(int32_t mode, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream);
/* what the calling thread's last launch_colred launched: out = { 1 if the 16-byte form k_colred_part4 (0: k_colred_part), mode, rows per
 * chunk, chunks per pass, grid of the partial kernel, 0.. } */
int rsrgan_op_segan_last_plan(int32_t out[8]);
/* virtual batch norm; every op: dims C, rows_per, P, ldc, then its own.
 * op 0 launch_vbn_coef:      ptrs sums, gamma, beta, ref_coef?, coef;  dims .., lds, B;  fl eps
 * op 1 launch_vbn_apply:     ptrs h, coef, y;  fl leak
 * op 2 launch_vbn_bwd_coef:  ptrs sums, gamma, coef, dgamma?, dbeta? (both or none);  dims .., lds, B, first_live, accumulate
 * op 3 launch_vbn_bwd_apply: ptrs h, dy, coef, dh;  fl leak */
int rsrgan_op_segan_vbn(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream);
/* layout, elementwise, losses, optimizer.
 * op 0 launch_pad_rows:     ptrs src, dst;  dims B, L, C, pf, pb
 * op 1 launch_prep_tconv:   ptrs W, dst;  dims 1, ldw, nb, na, e, ne, ldd
 * op 2 launch_prep_tconv_many, 44 jobs to a launch as refresh_weights: ptrs (W, dst) per job;  dims n, then ldw, nb, na, e, ne, ldd per job
 * op 3 launch_interleave:   ptrs T0, T1, bias?, T;  dims Q0, Q1, i00, i01, pl, B, Lt, C (i0 and Q must agree with pl and Lt)
 * op 4 launch_act_fwd:      ptrs z, alpha? (NULL: leaky), out;  dims C, ldo, coff, rows;  fl leak
 * op 5 launch_act_bwd:      ptrs dy, z, alpha?, extra?, dz;  dims ldy, coff, C, rows;  fl leak
 * op 6 launch_copy_cols:    ptrs src, dst;  dims lds, soff, ldd, doff, C, rows, accumulate
 * op 7 launch_build_joint1: ptrs x, tail, noise?, joint;  dims Lx, U, B
 * op 8 launch_sum_all:      ptrs src, out, scratch (256 floats);  dims rows, cols, ld
 * op 9 launch_segan_lsgan:  ptrs logits, dlogits?, loss3;  dims B, mode, fake_pass, P
 * op 10 launch_segan_l1:    ptrs G, labels, lambda, dG?, loss3;  dims n, accumulate
 * op 11 launch_rmsprop:     ptrs w, g, ms, lr;  dims n;  fl decay, eps */
int rsrgan_op_segan_elem(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream);
/* the discriminator's head; dims R, Ld, C, k, ldfc.
 * op 0 launch_dhead_fwd: ptrs h, W, wfc, bfc, conv_out, logits
 * op 1 launch_dhead_bwd: ptrs dlogit, h, conv_out, W, wfc, dW?, dwfc?, dbfc? (all three or none), dh */
int rsrgan_op_segan_dhead(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream);

/* ---- the step's small kernels (csrc/kernels.hip: the LSGAN and MSE terms, discriminator_lstm's fused head, L2, the per-tensor
 * clip_by_norm, SGD / Adam / EMA, frame-level dropout, lrelu').  Unit parity tests only (tests/test_gpu_update_ops.py,
 * tests/test_gpu_loss_ops.py, tests/test_update_op_args.py); no trainer calls them.  Each goes through the launch_* function the
 * model calls and never launches a kernel directly.  ptrs / dims / fl as in the SEGAN entries above ("?" = may be NULL).  A null
 * table or required pointer, a misaligned pointer (16 bytes for the flat buffers w, g, m, v, ema, ws and for the head's top / dout;
 * 4 bytes elsewhere), a size below 1, a leading dimension below its row (or no multiple of 4 where a kernel moves float4: ldt, ldo),
 * a tensor offset or length that is no multiple of 4, dR % 4 != 0 or dR > 60, Bp > 0 with Bt outside 1 .. Bp or a row count that Bp
 * does not divide, or a scratch below the launcher's need returns RSRGAN_ERR_INVALID before the first HIP call, rsrgan_last_error()
 * naming it.
 *
 * Device scalars `dyn` [16 floats], by slot: 0 g_lr, 1 d_lr, 2 lambda, 3 d_real, 4 d_fake, 5 l2_scale, 6 clip, 7 beta1, 8 beta2,
 * 9 eps, 10 ema_decay, 11 Adam's lr_t of G, 12 of D.
 *
 * rsrgan_op_chunks (no device): the chunk table the model builds for its flat parameter buffer, from tensors [n_tensors][3] =
 * (float offset, floats, l2 flag), 1 .. 4096 of them: *n_chunks, and, where out is not NULL (out_ints >= 3 * n_chunks + 3 *
 * n_tensors), out = tensor[n_chunks], off[n_chunks], len[n_chunks], t_first[n_tensors], t_count[n_tensors], t_l2[n_tensors]. */
int rsrgan_op_chunks(const int64_t* tensors, int32_t n_tensors, int32_t* out, int64_t out_ints, int32_t* n_chunks);
/* the chunked kernels; the entry builds the table of rsrgan_op_chunks, uploads it for the call and synchronises the stream.
 * Every op: dims n_tensors, buf_floats (of each flat buffer), partial_floats (>= n_chunks), three op-specific values (0 where none),
 * then the n_tensors triples.  partial [n_chunks] is an output of ops 0 - 2 and the input of ops 3 - 4.
 * op 0 launch_sumsq:      ptrs g, partial
 * op 1 launch_dw_reduce:  ptrs ws, g, partial;  dims .., stride, ntiles (1 .. 64), ws_floats, triples, then src[n_tensors]: the tensor's
 *                         float offset inside a record (a multiple of 4, the tensor inside the stride) or -1
 * op 2 launch_l2:         ptrs w, g, l2_scale, partial
 * op 3 launch_apply_sgd:  ptrs w, g, ema?, partial, dyn
 * op 4 launch_apply_adam: ptrs w, g, m, v, ema?, partial, dyn;  dims .., lrt_slot (11 or 12) */
int rsrgan_op_update(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream);
/* the losses and the element-wise kernels.
 * op 0 launch_lsgan:       ptrs logits, dlogits?, t_real, t_fake, loss3;  dims T, Nd, n_real, ldl, clip_on, Bp, Bt;  fl clip_lo, clip_hi
 * op 1 launch_dhead:       ptrs top, w, b, logits, dlogits?, dout?, gw?, gb?, t_real, t_fake, loss3, part;  dims T, Nd, n_real, dR, ldt,
 *                          ldw, ldl, ldo, want_grads (dlogits, dout), want_wgrads (gw, gb), Bp, Bt, part_floats (>= ceil(T Nd / 64) x 67)
 * op 2 launch_mse:         ptrs y, lab, dy?, lambda, loss, scratch;  dims rows, D, ld, accumulate, Bp, Bt, scratch_floats (>= 1024)
 * op 3 launch_g_total:     ptrs l4, lambda  (dims may be NULL)
 * op 4 launch_l2_total:    ptrs partial, l2_scale, out;  dims n
 * op 5 launch_adam_tick:   ptrs dyn, t (int32);  dims lr_slot, lrt_slot ((0, 11) or (1, 12));  fl beta1, beta2
 * op 6 launch_dropout_fwd: ptrs y;  dims rows, cols, ld, key (the 64 bits of the unsigned key), thr (0 .. 2^24);  fl keep
 * op 7 launch_dropout_bwd: ptrs y, d;  dims rows, cols, ld;  fl keep
 * op 8 launch_lrelu_bwd:   ptrs h, d;  dims rows, cols, ld;  fl alpha */
int rsrgan_op_step_elem(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream);
/* the layout, staging and weight-copy kernels (csrc/kernels.hip; tests/test_gpu_layout_ops.py, tests/test_layout_op_args.py): every one
 * a copy, a single fp32 add or one fixed-order fp32 sum, so the tests ask for equal bits.  The list ops (2, 6, 7, 11, 13) build the
 * launcher's job struct from dims and ptrs and name an argument "<name> of job <j>".  RSRGAN_ERR_INVALID before the first HIP call,
 * rsrgan_last_error() naming it, for: a null table or required pointer; a size below 1 (below 0 where 0 is a no-op: rows of op 11, n of
 * op 12; an offset, row0, slot, t0, Tw, dim, I, P, kx, c0); a leading dimension below its row; Bt outside 0 .. B; rows [row0, row0 + B)
 * outside Ns; a list longer than the launcher's struct (16 transposes, 24 swizzles, 32 buffers, 4 layers); op 7: a dst that is not 16-byte
 * aligned, gates outside 0 .. 4, with gates >= 1 nct below gates x ceil(H / 16) (the logical matrix must cover the source); ops 8, 9: M
 * no multiple of S x W, ldk below kh x kw x C; op 8 where C % 4 == 0 and ldc % 4 == 0 (the float4 form): src or col not 16-byte aligned,
 * row_stride or ldk no multiple of 4; op 9: dcol or dst not 16-byte aligned, C, ldc or ldk no multiple of 4; op 10: a dst that is not
 * 16-byte aligned; op 11: dir outside 0 .. 2, a layer whose off + H + P exceeds SF.
 * op 0 launch_pack_tm:         ptrs src, dst;  dims B, T, D, ld
 * op 1 launch_unpack_bm:       ptrs src, dst;  dims B, T, D, ld, Bt (0: all B rows)
 * op 2 launch_stage_inputs:    ptrs (src, dst) of pack 0, pack 1, copy 0 .. 3 (a NULL src skips the slot);  dims B, T, Bt, D0, ld0, D1, ld1,
 *                              n0 .. n3 (32-bit words of each copy)
 * op 3 launch_build_d_input:   ptrs lab (NULL without with_real), y, nr?, nf?, xd;  dims B, T, D, ld, with_real
 * op 4 launch_add_noise_rows:  ptrs src, noise?, dst;  dims B, T, D, ld, Ns, row0
 * op 5 launch_transpose:       ptrs src, dst;  dims lds, ldd, R, C
 * op 6 launch_transpose_many:  ptrs (src, dst) per job;  dims n (1 .. 16), then lds, ldd, R, C per job
 * op 7 launch_swizzle_many:    ptrs (src, dst) per job;  dims n (1 .. 24), then ld, gates, H, C, c0, K1, I, P, kx, nct, nkb per job (csrc/kernels.h
 *                              SwizzleJob; dst [nct * nkb * 256])
 * op 8 launch_im2col:          ptrs src, col;  dims row_stride, ldc, C, S, W, kh, kw, ldk, M
 * op 9 launch_col2im:          ptrs dcol, dst;  dims ldk, C, S, W, kh, kw, ldc, M
 * op 10 launch_expand_c4:      ptrs src, dst;  dims ld_src, n, rows
 * op 11 launch_gstate:         ptrs state, mask? (int32), then (c, mst) per layer (unused by dir 2; mst NULL where ldP = 0);  dims nl (1 .. 4), SF,
 *                              rows, dir, slot, then H, P, ldP, off per layer
 * op 12 launch_window_len:     ptrs len, dst (int32);  dims n, t0, Tw
 * op 13 launch_zero_many:      ptrs p per buffer;  dims n (1 .. 32), then the floats of each
 * op 14 launch_fill:           ptrs p;  dims n;  fl v
 * op 15 launch_build_joint:    ptrs x (NULL with dim = 0), tail, joint;  dims ldx, off, dim, ldt, Dt, ldj, row0, R
 * op 16 launch_slice_cols:     ptrs src, dst;  dims lds, off, ldd, R, C
 * op 17 launch_pad_copy:       ptrs dense, padded;  dims rows, cols, ld, to_padded
 * op 18 launch_copy_f:         ptrs src, dst;  dims n */
int rsrgan_op_layout(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream);
/* the launch-per-phase LSTM step kernels (csrc/kernels.hip k_fwd_gates, k_fwd_proj, k_bwd_a2, k_bwd_b, k_bwd_bp + k_bwd_b_red) through
 * their five launchers, without a handle (tests/test_gpu_lstm_step_ops.py, tests/test_lstm_step_op_args.py; DESIGN.md "The step-kernel
 * entry").  A call describes n jobs of ONE launch: dims[0] = n (1 .. 8, csrc/kernels.h MAXJ), then one record per job; ptrs holds one group
 * per job, in the order below; an argument is named "<name> of job <j>".  A pointer marked ? may be NULL and selects the optional form
 * exactly as the job structs of csrc/kernels.h document it.  The entry fills the job struct field by field, computes nblk_c and kb_max as
 * csrc/model.cpp does, and calls the launcher; the fragment-tiled (Wsw, WpT_sw, Wp_sw, Ksw) and transposed (WpT) weight images are the
 * caller's (rsrgan_op_layout ops 7 and 5, with the SwizzleJob rows of Model::refresh_swizzles).  RSRGAN_ERR_INVALID before the first HIP
 * call, rsrgan_last_error() naming the argument, for: a null table or required pointer; n outside 1 .. 8; a size below 1 (t, I, n_begin
 * below 0); a leading dimension below its row; a pointer the kernels move float4 through that is not 16-byte aligned; and the kernels' limits:
 * op 0: ldx, ldm multiples of 4, ldx + ldm <= 1024 (ldm alone with zx), exactly one of x and zx, bias with x, ldm >= H and np_res_in
 *       with np_res_out where np_m_out is given, no np_* pointer without np_m_out;
 * op 1: ldh a multiple of 4, m_prev with len, res_in with res_out, without len N <= P x ldh (the kernel reads its stand-in for len from
 *       WpT), with drop_ctr 0 < keep <= 1 and thr in 0 .. 2^24;
 * op 2: ldm a multiple of 4, Wp and Wp_sw both or neither, with them ldm <= 384 and dmt, without them P == H; drop as op 1;
 * ops 3, 4: H4 a multiple of 4 (dz rows and the row-major K move as float4), n_end above n_begin, K or Ksw, dx where n_begin < I, dmst
 *       where n_end > I, dx_accumulate 0 or 1; op 4: ws below bwd_b_plan's need, and (kpg + 1) / 2 > 12 for any job (the register slice
 *       of k_bwd_bp, what Model::bwd_b_splitk_ok refuses for the kernel's sake).
 * op 0 launch_fwd_gates:  ptrs x?, KxT? (unread), m, KhT? (unread), Wsw, zx?, bias?, wf, wi, wo, c_prev, c_out, gates, h, len (int32),
 *                         np_m_out?, np_out?, np_res_in?, np_res_out?;  dims N, H, ldx, ldm, ldh, t;  fl forget_bias
 * op 1 launch_fwd_proj:   ptrs h, WpT, WpT_sw?, m_prev?, m_out, out, res_in?, res_out?, len?, bias?, noise?, drop_ctr? (uint64);
 *                         dims N, P, ldh, ldm, ldo, t, drop seed, drop tag, drop thr;  fl keep of job 0, of job 1, ... (read with drop_ctr)
 * op 2 launch_bwd_a:      ptrs dout?, dmst, Wp?, Wp_sw?, dmt (? without a projection), gates, c_prev, c_cur, wf, wi, wo, dc, len, drop_ctr?;
 *                         dims N, P, H, ldm, t, drop seed, drop tag, drop thr;  fl keep per job
 * op 3 launch_bwd_b:      ptrs dz, K?, Ksw?, dx?, dmst?, len?;  dims N, I, n_begin, n_end, lddx, ldm, t, H4, dx_accumulate
 * op 4 bwd_b_plan + launch_bwd_b_splitk:  as op 3, then ptrs[6 n] = ws and dims[1 + 9 n] = the floats of ws */
int rsrgan_op_lstm_step(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream);
/* what the calling thread's last step launch chose (host stores only): out[0] form -- 1 k_fwd_gates<18,1> (16-row blocks), 2 <18,2>,
 * 3 <32,2>; 4 k_fwd_proj<4>, 5 <8>, 6 <4,drop>, 7 <8,drop>; 8 k_bwd_a2<4>, 9 <18>, 10 <24>, 11 .. 13 the same with dropout; 14 k_bwd_b
 * <8,8,8,1> (16-row tiles), 15 the pipelined <8,0,6>; 16 split-K -- out[1] threads per block, out[2] grid, out[3] 1 where the job map was
 * filled (grid <= 768), out[4], out[5] KG and kpg of job 0 (split-K), out[6] the grid of k_bwd_b_red, out[7] dynamic LDS bytes, out[8] jobs
 * that own a group of XCD slots, out[9] 1 where job 0 of a split-K launch reads the fragment-tiled K; the rest 0 */
int rsrgan_op_lstm_step_last_plan(int32_t out[16]);

/* ---- SEGAN-style conv G/D (models/segan.py:SEGAN with generator.py:AEGenerator, discriminator.py:discriminator, utils/bnorm.py:VBN;
 * BASELINE.json configs[4]).  The reference's trainer cannot run as shipped (segan.py:136 calls an undefined variables_on_gpu0(),
 * scripts/train_segan.py:20 imports a missing module); the graph it would build is fully specified and is what these entry
 * points compute.  One run = sess.run([model.d_opt, model.d_losses[0]]) / sess.run([model.g_opt, model.g_losses[0]])
 * (scripts/train_segan.py:32-52).  x [B, input_len], labels [B, output_dim]; the random draws of a run are INPUTS: z
 * [B, len(code), depth_last] (generator.py:201-205) and one gaussian_noise_layer draw [B, input_len + output_dim] per
 * discriminator call -- reference ("dummy") pass, real, fake (discriminator.py:74; NULL = std 0). */
typedef struct rsrgan_segan_cfg {
  int32_t batch_size;      /* args.batch_size (also the VBN mixing weight 1 / (B + 1), bnorm.py:37) */
  int32_t input_len;       /* input_dim * (left_context + 1 + right_context) (segan.py:96-100) */
  int32_t output_dim;      /* units of the generator's last dense layer (generator.py:283-287) */
  int32_t n_layers;        /* len(g_enc_depths) = len(d_num_fmaps) = 11 (segan.py:89-91) */
  int32_t g_depths[16];    /* 16,32,32,64,64,128,128,256,256,512,1024; multiples of 16 */
  int32_t d_depths[16];
  int32_t g_kwidth;        /* 20 (generator.py:151) */
  int32_t d_kwidth;        /* 31 (discriminator.py:79,88) */
  int32_t g_prelu;         /* args.g_nl == 'prelu' (run_segan.sh:120); 0 = leakyrelu */
  float   lrelu_alpha;     /* utils/ops.py:120 (0.3) */
  float   vbn_eps;         /* bnorm.py:17 (1e-5) */
  float   rms_decay;       /* tf.train.RMSPropOptimizer defaults (segan.py:123-124): 0.9 */
  float   rms_eps;         /* 1e-10 */
} rsrgan_segan_cfg;
typedef struct rsrgan_segan_handle_s* rsrgan_segan_handle;
enum { RSRGAN_SEGAN_G_LR = 0, RSRGAN_SEGAN_D_LR = 1, RSRGAN_SEGAN_L1_LAMBDA = 2 };   /* segan.py:110-111,106 */
int rsrgan_segan_default_cfg(rsrgan_segan_cfg* cfg);
int rsrgan_segan_create(const rsrgan_segan_cfg* cfg, uint64_t seed, rsrgan_segan_handle* out);
int rsrgan_segan_destroy(rsrgan_segan_handle h);
int rsrgan_segan_set_scalar(rsrgan_segan_handle h, int32_t which, double v);
/* variable table = tf.trainable_variables() split by the g_/d_ prefix (segan.py:269-283), graph-construction order */
int rsrgan_segan_num_tensors(rsrgan_segan_handle h, int32_t net);
int rsrgan_segan_tensor_info(rsrgan_segan_handle h, int32_t net, int32_t idx, char* name, int32_t name_cap, int32_t* rows, int32_t* cols,
                             int64_t* dense_offset);
int64_t rsrgan_segan_param_count(rsrgan_segan_handle h, int32_t net);
/* what: 0 = variables, 1 = the RMSProp "rms" slots, 2 = last gradients (tower-local or all-reduced); dense flat DEVICE vectors */
int rsrgan_segan_get_params(rsrgan_segan_handle h, int32_t net, int32_t what, float* dense, void* stream);
int rsrgan_segan_set_params(rsrgan_segan_handle h, int32_t net, int32_t what, const float* dense, void* stream);
/* G(x) [B, output_dim] (model.Gs, segan.py:194-197) */
int rsrgan_segan_forward_g(rsrgan_segan_handle h, const float* x, const float* z, float* y, void* stream);
/* per-tower compute_gradients (segan.py:139-146): losses DEVICE float[3] = {d_rl, d_fk, d_loss} / {g_adv, g_l1, g_loss}; train = 0: losses only */
int rsrgan_segan_d_backward(rsrgan_segan_handle h, const float* x, const float* labels, const float* z, const float* noise_ref,
                            const float* noise_real, const float* noise_fake, float* out_losses, int32_t train, void* stream);
int rsrgan_segan_g_backward(rsrgan_segan_handle h, const float* x, const float* labels, const float* z, const float* noise_ref,
                            const float* noise_fake, float* out_losses, int32_t train, void* stream);
/* average_gradients (segan.py:148-149) = the caller's RCCL all-reduce(avg) of this buffer; then apply_gradients (:150-151) */
int rsrgan_segan_grad_buffer(rsrgan_segan_handle h, int32_t net, float** ptr, int64_t* count);
int rsrgan_segan_apply(rsrgan_segan_handle h, int32_t net, void* stream);

int rsrgan_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RSRGAN_H_ */
