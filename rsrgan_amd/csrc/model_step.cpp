// model_step.cpp -- the training step's drivers: graph segments, the D-run and the G-run with their plans and stages, the supervised
// trainers' steps, the generator's forward and its inference windows, the updates.  The recurrences they launch
// (rnn_forward / rnn_backward, the persistent launches, the weight gradients) are in model.cpp; what a handle is built from in
// model_init.cpp.
#include "model.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace rsr {

// ------------------------------------------------------------------------------------------ hipGraph segments
static inline uint64_t seg_key(int seg, int T, unsigned bits) { return ((uint64_t)seg << 48) | ((uint64_t)(unsigned)T << 16) | (bits & 0xffffu); }
enum { SEG_D = 1, SEG_G_MAIN = 2, SEG_G_FCIN = 3, SEG_G_LAYER0 = 4 /* .. + MAXJ */, SEG_G_L2 = 20, SEG_G_TAIL = 21, SEG_APPLY_D = 22, SEG_APPLY_G = 23, SEG_G_BATCH = 24, SEG_BNL = 25 };

template <class F>
void Model::run_seg(uint64_t key, hipStream_t s, F&& body) {
  if (!graphs_on() || s == nullptr) { body(); return; }
  if (graphs.size() > 96) drop_graphs();                   // many distinct T (length-bucketed training): start over
  GraphSlot& g = graphs[key];
  if (g.exec) { if (hipGraphLaunch(g.exec, s) != hipSuccess) { (void)hipGetLastError(); g.exec = nullptr; g.uses = -1; body(); } return; }
  if (g.uses < 0) { body(); return; }                       // capture failed once: eager from then on
  if (g.uses++ == 0) { body(); return; }                    // first use: eager (also runs every lazy one-time setup)
  if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); g.uses = -1; body(); return; }
  body();
  hipGraph_t gr = nullptr;
  if (hipStreamEndCapture(s, &gr) != hipSuccess || !gr) {
    (void)hipGetLastError(); g.uses = -1;
    if (switch_now_graph_debug()) fprintf(stderr, "rsrgan: capture of segment %llx failed, eager from here on\n", (unsigned long long)key);
    body(); return;
  }
  hipGraphExec_t ex = nullptr;
  if (hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0) != hipSuccess || !ex) { (void)hipGetLastError(); (void)hipGraphDestroy(gr); g.uses = -1; body(); return; }
  (void)hipGraphDestroy(gr);
  g.exec = ex;
  if (hipGraphLaunch(g.exec, s) != hipSuccess) { (void)hipGetLastError(); (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; g.uses = -1; body(); }
}
void Model::drop_graphs() {
  for (auto& kv : graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  graphs.clear();
}
hipStream_t Model::enter(hipStream_t caller) {
  if (caller != nullptr || !main_s) return caller;
  (void)hipEventRecord(ev_in, caller);
  (void)hipStreamWaitEvent(main_s, ev_in, 0);
  return main_s;
}
void Model::leave(hipStream_t caller, hipStream_t work) {
  if (work == caller) return;
  (void)hipEventRecord(ev_out, work);
  (void)hipStreamWaitEvent(caller, ev_out, 0);
}
const float* Model::stage_noise(const float* src, float* buf, hipStream_t s) {
  if (!src) return nullptr;
  (void)hipMemcpyAsync(buf, src, (size_t)Bt * Dout * sizeof(float), hipMemcpyDeviceToDevice, s);
  return buf;
}

void Model::mark_bucket(int net, int i, hipStream_t s) {
  GradBucket& b = gbk[net][i];
  (void)hipEventRecord(b.ev, s);
  b.marked = true;
}
void Model::finish_buckets(int net, hipStream_t s) {
  for (auto& b : gbk[net]) {
    if (!b.marked) (void)hipEventRecord(b.ev, s);
    b.marked = false;
  }
}
// ------------------------------------------------------------------------------------------
int Model::prepare_batch(const float* x, const float* labels, const int32_t* lengths, int T, hipStream_t s, const float** nr,
                         const float** nf, hipStream_t early) {
  if (T <= 0 || T > Tmax) { set_error("T=%d outside (0, max_frames=%d]", T, Tmax); return RSRGAN_ERR_INVALID; }
  if (!x || (!lengths && !g_dnn())) { set_error("null input pointer"); return RSRGAN_ERR_INVALID; }
  // one launch: both packs, the lengths (twice: the stacked discriminator batch reads rows [B, 2B) as well) and the callers' noise
  // (a padded model, Bt < B: the caller's Bt rows land in rows [0, Bt) of every frame; rows [Bt, B) of the packs, their lengths and
  // their noise stay at the zeros of the allocation)
  StageJobs j{}; j.B = B; j.T = T; j.Bt = Bt;
  j.pack[0] = StagePack{x, x_tm, Din, ldDin};
  if (labels) j.pack[1] = StagePack{labels, lab_tm, Dout, ldDout};
  if (lengths) { j.copy[0] = StageCopy{lengths, len_dev, Bt}; j.copy[1] = StageCopy{lengths, len_dev + B, Bt}; }
  if (nr && *nr) { j.copy[2] = StageCopy{*nr, noise_r_buf, Bt * Dout}; *nr = noise_r_buf; }
  if (nf && *nf) { j.copy[3] = StageCopy{*nf, noise_f_buf, Bt * Dout}; *nf = noise_f_buf; }
  if (early) {
    // (RSRGAN_DPIPE) what D(real) needs -- the labels, the lengths, its noise -- goes ahead on the side stream, behind the last use of
    // the buffers it overwrites (ev_dfree); the input frames and D(G(x))'s noise stay in stream order
    StageJobs e{}; e.B = B; e.T = T; e.Bt = Bt;
    e.pack[1] = j.pack[1]; e.copy[0] = j.copy[0]; e.copy[1] = j.copy[1]; e.copy[2] = j.copy[2];
    j.pack[1] = StagePack{}; j.copy[0] = StageCopy{}; j.copy[1] = StageCopy{}; j.copy[2] = StageCopy{};
    (void)hipStreamWaitEvent(early, ev_dfree, 0);
    launch_stage_inputs(e, early);
  }
  launch_stage_inputs(j, s);
  cur_T = T;
  g_fwd_valid = false;
  return RSRGAN_OK;
}

Chain Model::g_chain(int T) {
  (void)T;
  Chain ch;
  const bool res = cfg.g_type == RSRGAN_G_RES_LSTM_L;
  for (size_t l = 0; l < gl.size(); ++l) {
    LayerRun R;
    R.ps = &G; R.L = &gl[l]; R.S = &g_st[l]; R.in = g_ins[l];
    R.N = B; R.Ns = B; R.row0 = 0; R.len = len_dev;
    R.zx_batched = (l == 0);                 // layer 0's input exists for all t before the wave starts
    R.carry = g_carry;
    if (res) { R.res_in = g_ins[l]; R.res_out = g_res[l]; }   // inputs_{l+1} = outputs_l + inputs_l (res_lstm_l.py:111,121,131,190)
    if (g_resi()) { R.res_in = g_ins[0]; R.res_out = g_res[l]; }      // inputs_{l+1} = outputs_l + x (res_lstm_i.py:111,190)
    if (seq_drop_on()) R.drop = DropSpec{drop_ctr, drop_seed, (1ull << 40) | ((unsigned long long)l << 20), drop_thr(), keep_prob};
    ch.push_back(R);
  }
  return ch;
}

Chain Model::d_chain(int N, int Ns, int row0) {
  Chain ch;
  for (size_t l = 0; l < dl.size(); ++l) {
    LayerRun R;
    R.ps = &D; R.L = &dl[l]; R.S = &d_st[l]; R.in = l == 0 ? xd : d_st[l - 1].out;
    R.N = N; R.Ns = Ns; R.row0 = row0; R.len = len_dev + row0;
    R.zx_batched = false;
    ch.push_back(R);
  }
  return ch;
}

void Model::gstate_xfer(int dir, int T, int rows, const int* mask, hipStream_t s) {
  GStateArgs a{};
  a.nl = (int)gl.size(); a.SF = g_state_sf; a.rows = rows; a.dir = dir; a.state = g_state; a.slot = (size_t)T * B; a.mask = mask;      // (T: the slot of c / mst that holds the final state)
  int off = 0;
  for (size_t l = 0; l < gl.size(); ++l) {
    a.L[l] = GStateLayer{g_st[l].c, g_st[l].mst, gl[l].H, gl[l].P, gl[l].ldP, off};
    off += gl[l].H + gl[l].P;
  }
  launch_gstate(a, s);
}

void Model::g_forward_head(int T, hipStream_t s) {
  if (cfg.g_type == RSRGAN_G_LSTM || g_bnl()) {   // h = leakyrelu(x.W + b)  (models/lstm.py:82-87; bnlstm.py:103-108: relu, as bnl_forward)
    const int P = gR, ldP = pad4(P);
    if (seq_bn_infer()) {      // the folded layer: h = leakyrelu(x.W' + b)
      gemm(x_tm, ldDin, true, G.W(g_fc_in_w), ldP, false, g_h0, ldP, T * B, P, Din, g_bn_fold_b, 1, cfg.lrelu_alpha, false, s);
      return;
    }
    if (seq_bn()) {      // h = leakyrelu(batch_norm(x.W)): batch moments over the caller's rows in a training fetch, else the moving statistics
      gemm(x_tm, ldDin, true, G.W(g_fc_in_w), ldP, false, g_z0, ldP, T * B, P, Din, nullptr, 0, 0.f, false, s);
      g_fwd_bn_train = bn_training();
      launch_bn_seq_forward(g_z0, ldP, g_h0, ldP, T * B, P, bn_vars(G, g_bn_t), g_bn_stat, ldP, g_fwd_bn_train, true, cfg.lrelu_alpha, pad_Bp(), Bt,
                            g_bn_scr, (size_t)64 * ldP, s);
      return;
    }
    gemm(x_tm, ldDin, true, G.W(g_fc_in_w), ldP, false, g_h0, ldP, T * B, P, Din, G.W(g_fc_in_b), 1, g_bnl() ? 0.f : cfg.lrelu_alpha, false, s);
  }
}
// d = d(h0) [R][ldP] -> the input layer's parameter gradients (models/lstm.py:82-87).  Without batch norm: through the leaky-ReLU, dW and
// the bias column sum.  With it: the normaliser's backward (dbeta, dgamma, dz in place, exact zeros on the padding rows), then dW = x^T.dz.
void Model::g_fc_in_backward(float* d, int R, float* colsum_scratch, hipStream_t q) {
  const int P = gR, ldP = pad4(P);
  if (seq_bn()) {
    launch_bn_seq_backward(d, ldP, g_h0, ldP, g_z0, ldP, R, P, g_bn_stat, ldP, G.Gd(g_bn_t[0]), G.Gd(g_bn_t[1]), false, true, cfg.lrelu_alpha,
                           pad_Bp(), Bt, g_bn_sums, g_bn_scr, (size_t)64 * ldP, q);
    gemm(x_tm, ldDin, false, d, ldP, false, G.Gd(g_fc_in_w), ldP, Din, P, R, nullptr, 0, 0.f, false, q);
    return;
  }
  launch_lrelu_bwd(g_h0, d, (size_t)R, P, ldP, cfg.lrelu_alpha, q);
  gemm(x_tm, ldDin, false, d, ldP, false, G.Gd(g_fc_in_w), ldP, Din, P, R, nullptr, 0, 0.f, false, q);
  launch_colsum(d, ldP, nullptr, 0, G.Gd(g_fc_in_b), R, P, colsum_scratch, q);
}
// An inference handle's input FC: keep the weights as they were set on the host, then fold the moving statistics into the device copy
// in place.  Only a writer of the variables (Model::init, rsrgan_set_params) raises g_fc_in_unfolded; without it the device copy is
// already the folded one and a second fold would scale it again and lose the host copy, so the call does nothing.
void Model::seq_bn_fold(hipStream_t s) {
  if (!g_fc_in_unfolded) return;
  const TensorDesc& t = G.t[g_fc_in_w];
  g_w0_host.resize((size_t)t.rows * t.ld);
  if (hipMemcpyAsync(g_w0_host.data(), G.W(g_fc_in_w), g_w0_host.size() * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    set_error("RSRGAN_FLAG_BATCH_NORM | RSRGAN_FLAG_INFER: copying the input FC's weights to the host failed");
    inf_failed = true;
    return;
  }
  launch_bn_seq_fold(G.W(g_fc_in_w), t.ld, t.rows, gR, bn_vars(G, g_bn_t), g_bn_fold_b, s);
  g_fc_in_unfolded = false;
}
// the generator's UPDATE_OPS of one run (gan_rnn_placeholder.py:164-175 filters them by scope; tower 0 builds G twice, :196,204): the
// statistics of the run's forward, `times` times.  The discriminator has no batch norm: a D-run commits nothing.
void Model::seq_bn_commit(int times, hipStream_t s) {
  launch_bn_commit(gR, bn_vars(G, g_bn_t), g_bn_stat, pad4(gR), times, s);
}
void Model::g_forward_tail(int T, hipStream_t s) {   // y = outputs.W + b (models/lstm.py:121-124)
  const int P = gR, ldP = pad4(P);
  gemm(g_ins[gl.size()], ldP, true, G.W(g_fc_out_w), ldDout, false, y_tm, ldDout, T * B, Dout, P, G.W(g_fc_out_b), 0, 0.f, false, s);
  g_fwd_valid = true;
}
void Model::g_forward(int T, hipStream_t s, Chain* extra) {
  if (g_dnn()) { bn_eval_call = false; g_frame_forward(T * B, s); g_fwd_valid = true; return; }
  if (g_bnl() && !infer()) { bnl_forward(T, false, s); return; }      // (rsrgan_forward_g: decode normalises with the moving statistics)
  g_forward_head(T, s);
  if (infer()) { infer_forward(T, s); g_forward_tail(T, s); return; }
  if (!extra && persist_forward_g(T, s)) { g_forward_tail(T, s); return; }
  std::vector<Chain> chains;
  chains.push_back(g_chain(T));
  if (extra) chains.push_back(*extra);
  rnn_forward(chains, T, s);
  g_forward_tail(T, s);
}

// The recurrence of an inference handle (RSRGAN_FLAG_INFER) over T frames, in windows that hand the state on: one persistent launch of the
// stash-free variants per <= GP_TMAX frames (normally one), or -- shapes the persistent plans do not take, RSRGAN_FLAG_WAVEFRONT off,
// persist_disable -- the launch-per-phase path in windows of <= INFER_WINDOW frames, which is all the stashes hold.  A window reads its
// initial state in slot 0 of c / mst (the first one: zeros, or the caller's carried state under g_carry) and leaves its final state in
// slot inf_slot (1 behind a persistent launch, the window's length behind the launch path): copied to slot 0 for the next window, read by
// gstate_xfer behind the last.  Rows get the window's own lengths clamp(len - t0, 0, Tw): a row that ended earlier copies its state
// through and outputs zeros, as dynamic_rnn does.  Only the top layer's outputs go to the full-length buffer.
bool Model::infer_fallback_stash() {
  for (size_t l = 0; l < gl.size(); ++l) {
    LstmStash& S = g_st[l];
    if (!S.gates) S.gates = alloc_opt<float>((size_t)inf_W * B * 4 * gl[l].H);
    if (!S.h) S.h = alloc_opt<float>((size_t)inf_W * B * gl[l].ldH);
    if (!S.gates || !S.h) return false;
  }
  return true;
}
// one window on the launch-per-phase path: every layer sees stashes and inputs one window long, the top layer's outputs land in place in
// the full-length buffer
void Model::infer_window_launches(int t0, int Tw, hipStream_t s) {
  const bool res_l = cfg.g_type == RSRGAN_G_RES_LSTM_L, res_any = res_l || g_resi();
  const size_t top = gl.size() - 1;
  const float* x0 = g_ins[0] + (size_t)t0 * B * gl[0].ldI;
  std::vector<LstmStash> st(g_st);
  Chain ch;
  for (size_t l = 0; l < gl.size(); ++l) {
    const size_t o = l == top ? (size_t)t0 * B * gl[l].ldP : 0;
    if (!res_any) st[l].out += o;
    LayerRun R;
    R.ps = &G; R.L = &gl[l]; R.S = &st[l]; R.in = l == 0 ? x0 : g_ins[l];
    R.N = B; R.Ns = B; R.row0 = 0; R.len = len_win;
    R.zx_batched = (l == 0);
    R.carry = g_carry;
    if (res_l) { R.res_in = R.in; R.res_out = g_res[l] + o; }       // inputs_{l+1} = outputs_l + inputs_l
    if (g_resi()) { R.res_in = x0; R.res_out = g_res[l] + o; }       // inputs_{l+1} = outputs_l + x
    ch.push_back(R);
  }
  std::vector<Chain> chains{ch};
  rnn_forward(chains, Tw, s);
}
void Model::infer_forward(int T, hipStream_t s) {
  const bool carry_in = g_carry;
  bool persist = gp_fwd_on() && wavefront();
  for (int t0 = 0; t0 < T;) {
    const int Tw = std::min(T - t0, persist ? gp_Tcap : inf_W);
    g_carry = carry_in || t0 > 0;
    inf_t0 = t0;
    launch_window_len(len_dev, len_win, B, t0, Tw, s);
    if (persist && persist_forward_g(Tw, s)) {
      inf_slot = 1;
    } else if (bnl_infer()) {
      // (a bnlstm handle: the launch path does not know the fold.  Reached only after persist_disable, whose failure the caller has already
      // been told by rsrgan_device_status: every later forward reports it again)
      set_error("g_type bnlstm inference handle: the persistent forward is off after a reported device failure, and no other forward is built");
      inf_failed = true; break;
    } else if (persist) {
      persist = false;                                   // (no persistent plan takes this shape: the same frames again, in the launch path's windows)
      continue;
    } else {
      if (!infer_fallback_stash()) { set_error("hipMalloc failed (the launch path's stash of an inference handle)"); inf_failed = true; break; }
      infer_window_launches(t0, Tw, s);
      inf_slot = Tw;
    }
    t0 += Tw;
    if (t0 < T) infer_state_to_slot0(s);
  }
  g_carry = carry_in;
  inf_t0 = 0;
}
void Model::infer_state_to_slot0(hipStream_t s) {
  for (size_t l = 0; l < gl.size(); ++l) {
    const size_t nc = (size_t)B * gl[l].H, nm = (size_t)B * gl[l].ldP;
    (void)hipMemcpyAsync(g_st[l].c, g_st[l].c + (size_t)inf_slot * nc, nc * sizeof(float), hipMemcpyDeviceToDevice, s);
    (void)hipMemcpyAsync(g_st[l].mst, g_st[l].mst + (size_t)inf_slot * nm, nm * sizeof(float), hipMemcpyDeviceToDevice, s);
  }
}

void Model::d_logits(int N, int T, hipStream_t s) {
  const int ldPd = pad4(dR);
  gemm(d_st[dl.size() - 1].out, ldPd, true, D.W(d_fc_w), 4, false, logits, 4, T * N, 1, dR, D.W(d_fc_b), 0, 0.f, false, s);
}

// discriminator_lstm's head in one pass (kernels.hip k_dhead1 / 2): logits and the LSGAN terms of N rows per frame (the first n_real
// of them against *t_real), and with want_grads dlogits and d(outputs) in d_dB, with want_wgrads the output FC's gradients too.
// False: not applicable (the caller runs d_logits + launch_lsgan + the GEMMs of d_backward_pass).
bool Model::d_head(int N, int T, int n_real, const float* t_real, const float* t_fake, float* loss3, bool want_grads, bool want_wgrads,
                   hipStream_t s) {
  const int ldPd = pad4(dR), nb = (T * N + 63) / 64;
  if (!switches().dhead || d_dnn() || dl.empty() || dR % 4 != 0 || dR + 3 > 64 ||       // (k_dhead2 sums 64 quantities: 3 + dR)
      (size_t)nb * (DH_MAXR + 3) > scratch_floats) return false;
  DHeadArgs a{};
  a.top = d_st[dl.size() - 1].out; a.ldt = ldPd; a.w = D.W(d_fc_w); a.ldw = 4; a.b = D.W(d_fc_b);
  a.logits = logits; a.ldl = 4; a.dlogits = dlogits; a.dout = d_dB; a.ldo = ldPd; a.gw = D.Gd(d_fc_w); a.gb = D.Gd(d_fc_b);
  a.T = T; a.Nd = N; a.n_real = n_real; a.dR = dR; a.t_real = t_real; a.t_fake = t_fake; a.loss3 = loss3; a.part = scratch;
  a.want_grads = want_grads ? 1 : 0; a.want_wgrads = want_wgrads ? 1 : 0;
  a.Bp = pad_Bp(); a.Bt = Bt;
  launch_dhead(a, s);
  return true;
}

// ------------------------------------------------------------------------------------------ pieces the drivers share
// discriminator_lstm's head and the LSGAN terms of N rows per frame (the first n_real against d_real, the rest against *t_fake): d_head,
// else d_logits + launch_lsgan.  Returns whether the fused head ran (d(outputs) lies in d_dB then, the output FC's gradients are done).
bool Model::d_head_or_logits(int N, int T, int n_real, const float* t_fake, float* loss3, bool want_grads, bool want_wgrads, hipStream_t s) {
  if (d_head(N, T, n_real, dyn + DYN_D_REAL, t_fake, loss3, want_grads, want_wgrads, s)) return true;
  d_logits(N, T, s);
  launch_lsgan(logits, 4, want_grads ? dlogits : nullptr, T, N, n_real, dyn + DYN_D_REAL, t_fake, loss3, s, false, 0.f, 0.f, pad_Bp(), Bt);
  return false;
}

// The discriminator's BPTT wiring over the ping-pong d_dB, d_dA: the top layer reads d(outputs) in d_dB, every layer writes its input
// gradient where the layer below reads it; layer 0's goes to din0 (nullptr: not needed).  Returns the ping-pong buffer layer 0 leaves free.
float* Model::wire_d_bptt(Chain& ch, bool want_wgrads, float* din0, bool accumulate0) {
  float* cur = d_dB;
  float* other = d_dA;
  for (int l = (int)ch.size() - 1; l >= 0; --l) {
    ch[l].dout = cur; ch[l].want_wgrads = want_wgrads;
    if (l == 0) { ch[l].din = din0; ch[l].din_accumulate = accumulate0; }
    else { ch[l].din = other; ch[l].din_accumulate = false; std::swap(cur, other); }
  }
  return other;
}

// The generator's over the ping-pong a, b (a holds the top layer's d(outputs)); every layer wants its weight gradients.  Returns the buffer
// that holds d(h0) behind the pass (lstm: it feeds the input FC).
float* Model::wire_g_bptt(Chain& ch, float* a, float* b) {
  for (int l = (int)ch.size() - 1; l >= 0; --l) {
    ch[l].want_wgrads = true;
    if (cfg.g_type == RSRGAN_G_RES_LSTM_L) {      // d(inputs_l) = dx_l + d(inputs_{l+1}): one buffer, accumulated in place
      ch[l].dout = a; ch[l].din = l > 0 ? a : nullptr; ch[l].din_accumulate = true;
    } else {
      const bool need = cfg.g_type == RSRGAN_G_LSTM || l > 0;      // lstm: d(h0) feeds the input FC
      ch[l].dout = a; ch[l].din = need ? b : nullptr; ch[l].din_accumulate = false;
      std::swap(a, b);
    }
  }
  return a;
}

// output FC: dW = in^T . dy ; db = colsum(dy)  (batched over time)
void Model::g_fc_out_wgrads(const float* dy, int R, hipStream_t q) {
  const int P = gR, ldP = pad4(P);
  gemm(g_ins[gl.size()], ldP, false, dy, ldDout, false, G.Gd(g_fc_out_w), ldDout, P, Dout, R, nullptr, 0, 0.f, false, q);
  launch_colsum(dy, ldDout, nullptr, 0, G.Gd(g_fc_out_b), R, Dout, (side && q == side) ? scratch2 : scratch, q);
}

// the per-step output FC of a forward wave: y_t and rows [row02, row02 + B) of the discriminator's input (Ns2 rows per frame), noise added
FcStage Model::g_out_fc_stage(const float* nf, int Ns2, int row02) {
  FcStage F;
  F.offset = (int)gl.size(); F.N = B; F.K = gR; F.D = Dout;
  F.in = g_ins[gl.size()]; F.ld_in = pad4(gR); F.WT = g_fc_out_wT; F.bias = G.W(g_fc_out_b); F.noise = nf;
  F.y = y_tm; F.ldy = ldDout; F.out2 = xd; F.ld2 = ldDout; F.Ns2 = Ns2; F.row02 = row02;
  return F;
}

void Model::g_loss_tail(bool l2, hipStream_t s) {
  if (l2) {
    launch_l2(G.w, G.g, G.ct, dyn + DYN_L2, G.partial, s);
    launch_l2_total(G.partial, G.ct.n_chunks, dyn + DYN_L2, losses + 5, s);
  } else {
    (void)hipMemsetAsync(losses + 5, 0, sizeof(float), s);
  }
  launch_g_total(losses + 3, dyn + DYN_LAMBDA, s);
}

// the generator's forward as ONE persistent launch and the output FC behind it (the caller has run g_forward_head); false: not applicable
bool Model::g_forward_persist(int T, hipStream_t s) {
  if (!persist_forward_g(T, s)) return false;
  g_forward_tail(T, s);
  return true;
}

// leaves in last_dx0 (d_dA or d_dB) the gradient w.r.t. the discriminator input when need_dx0
void Model::d_backward_pass(int N, int T, bool want_wgrads, bool need_dx0, const float* dlog, hipStream_t s, bool head_done) {
  const int R = T * N;
  const int ldPd = pad4(dR);
  const float* top = d_st[dl.size() - 1].out;
  if (want_wgrads && !head_done) {
    gemm(top, ldPd, false, dlog, 4, false, D.Gd(d_fc_w), 4, dR, 1, R, nullptr, 0, 0.f, false, s);
    launch_colsum(dlog, 4, nullptr, 0, D.Gd(d_fc_b), R, 1, scratch, s);
  }
  // d(outputs) = dlogits . W^T  (d_head has left it in d_dB)
  if (!head_done) gemm(dlog, 4, true, D.W(d_fc_w), 4, true, d_dB, ldPd, R, dR, 1, nullptr, 0, 0.f, false, s);
  std::vector<Chain> chains(1, d_chain(N, N, 0));
  Chain& ch = chains[0];
  last_dx0 = wire_d_bptt(ch, want_wgrads, nullptr, false);
  if (need_dx0) ch[0].din = last_dx0;
  if (!persist_backward(ch, T, s)) rnn_backward(chains, T, s);
}

void Model::g_backward_pass(int T, float* dy, hipStream_t s) {
  const int R = T * B;
  const int P = gR, ldP = pad4(P);
  // output FC: dW = in^T . dy ; db = colsum(dy) ; d(in) = dy . W^T
  g_fc_out_wgrads(dy, R, s);
  gemm(dy, ldDout, true, G.W(g_fc_out_w), ldDout, true, g_dA, ldP, R, P, Dout, nullptr, 0, 0.f, false, s);
  std::vector<Chain> chains(1, g_chain(T));
  float* dh0 = wire_g_bptt(chains[0], g_dA, g_dB);
  if (!persist_backward_g(chains[0], T, s)) rnn_backward(chains, T, s);
  // through leakyrelu and the input FC (models/lstm.py:82-87)
  if (cfg.g_type == RSRGAN_G_LSTM) g_fc_in_backward(dh0, R, scratch, s);
}

// ------------------------------------------------------------------------------------------ the D-run
DRunPlan Model::plan_d_run(int T, const float* nr, const float* nf, bool want_grads, hipStream_t s) {
  DRunPlan p;
  p.T = T; p.want_grads = want_grads; p.nr = nr; p.nf = nf;
  // RSRGAN_DPIPE: D(real) on the side stream, ahead of this call's place in the stream; the run itself is k_glstm_fwd_dt (D(G(x)) trailing)
  // (RSRGAN_DPIPE=1 covers labels and lengths; a noise_real tensor drawn on the caller's stream right before the call is covered by =2 only)
  if (dpipe && (!nr || sw.dpipe >= 2) && wavefront() && gp_fwd_on() && !d_dnn() && !seq_drop_on() && T > 0 && T <= Tmax) {
    Chain dchk = d_chain(B, 2 * B, B);
    p.dsplit = persist_forward_real(T, side, true) && persist_forward_g_trail(dchk, T, s, nf, true);
  }
  // rsrgan_d_step: the update follows in the same call -- its launches close this segment (one graph: no launch boundary in front
  // of the clip / SGD / weight-copy kernels); RSRGAN_FUSED_SEG=0 keeps them in a segment of their own
  p.inl = fused_apply && switches().fused_seg && want_grads && !d_dnn() && graphs_on();
  return p;
}

// x -> G(x) -> the discriminator's input rows [B, 2B) (+ noise_fake) -> D over both halves of the stacked batch, in the best form that applies
void Model::d_run_forward(const DRunPlan& p, hipStream_t s) {
  const int T = p.T;
  if (p.dsplit) {
    g_forward_head(T, s);
    Chain dch = d_chain(B, 2 * B, B);
    if (persist_forward_g_trail(dch, T, s, p.nf)) return;
  }
  if (wavefront() && gp_fwd_on()) {
    // the generator as ONE persistent launch, then both discriminator calls stacked (N = 2B) as another
    g_forward_head(T, s);
    if (g_forward_persist(T, s)) {
      launch_add_noise_rows(y_tm, p.nf, xd, B, T, Dout, ldDout, 2 * B, B, s);
      if (!d_dnn()) {
        std::vector<Chain> chains(1, d_chain(2 * B, 2 * B, 0));
        if (!persist_forward(chains[0], T, s)) rnn_forward(chains, T, s);
      }
      return;
    }
  }
  if (wavefront()) {
    // ONE wave: G's layers | D(real) (independent of G) | per-step output FC -> y_t, xd fake rows |
    // D(fake) two diagonals behind G's top layer
    if (!gp_fwd_on()) g_forward_head(T, s);
    const int Lg = (int)gl.size();
    std::vector<Chain> chains{g_chain(T)};
    std::vector<int> offs{0};
    if (!d_dnn()) {
      chains.push_back(d_chain(B, 2 * B, 0)); offs.push_back(0);
      chains.push_back(d_chain(B, 2 * B, B)); offs.push_back(Lg + 1);
    }
    std::vector<FcStage> fcs{g_out_fc_stage(p.nf, 2 * B, B)};
    rnn_forward(chains, T, s, &offs, &fcs);
    return;
  }
  g_forward(T, s);
  launch_add_noise_rows(y_tm, p.nf, xd, B, T, Dout, ldDout, 2 * B, B, s);
  if (!d_dnn()) {
    std::vector<Chain> chains(1, d_chain(2 * B, 2 * B, 0));
    rnn_forward(chains, T, s);
  }
}

// the three LSGAN losses over the stacked batch and, with gradients, the discriminator's backward pass with its weight gradients
void Model::d_run_head_backward(const DRunPlan& p, hipStream_t s) {
  const int T = p.T;
  if (d_dnn()) {
    d_dnn_forward_loss(T, 2 * B, B, p.want_grads, losses, s);
    if (p.want_grads) fc_backward(D, dfc, d_act, T * 2 * B, dlogits, true, false, s);
    return;
  }
  const bool head = d_head_or_logits(2 * B, T, B, dyn + DYN_D_FAKE, losses, p.want_grads, p.want_grads, s);
  if (p.want_grads) d_backward_pass(2 * B, T, true, false, dlogits, s, head);
}

int Model::d_backward(const float* x, const float* labels, const int32_t* lengths, int T, const float* nr, const float* nf,
                      float* out_losses, bool want_grads, hipStream_t s) {
  if (!labels) { set_error("labels required"); return RSRGAN_ERR_INVALID; }
  if (supervised()) { set_error("RSRGAN_FLAG_SUPERVISED: the trainer graph has no discriminator step"); return RSRGAN_ERR_STATE; }
  if (g_dnn()) return dnn_d_backward(x, labels, T, out_losses, want_grads, s);
  if (d_dnn()) { nr = nullptr; nf = nullptr; }    // discriminator_dnn.py:58: the noise layer is commented out
  bn_eval_call = !want_grads;                      // (is_training of this fetch: the DropoutWrapper masks; read by seq_drop_on() below)
  if (seq_bn()) g_fwd_bn_train = bn_training();    // (on the host: a replayed segment does not run g_forward_head's body)
  dfree_current = false;                           // this run writes the discriminator's stash and input rows
  DRunPlan p = plan_d_run(T, nr, nf, want_grads, s);
  int rc = prepare_batch(x, labels, lengths, T, s, &p.nr, &p.nf, p.dsplit ? side : nullptr);      // (stages the noise too: caller pointers never enter a graph)
  if (rc) return rc;
  p.kbits = (want_grads ? 1u : 0u) | (p.nr ? 2u : 0u) | (p.nf ? 4u : 0u) | (p.inl ? 8u : 0u) | (p.dsplit ? 16u : 0u);
  if (p.dsplit) {
    // discriminator input rows [0,B) = labels + noise_real, D(real) over them; this stream waits for it in front of its own launches
    // (the fused forward launch and the D(real) launch do not fit the device together)
    launch_add_noise_rows(lab_tm, p.nr, xd, B, T, Dout, ldDout, 2 * B, 0, side);
    (void)persist_forward_real(T, side);
    (void)hipEventRecord(ev_real, side);
    (void)hipStreamWaitEvent(s, ev_real, 0);
  }
  if (seq_drop_on()) launch_drop_tick(drop_ctr, s);     // a new training run: new masks (read from device memory: graph-safe)
  run_seg(seg_key(SEG_D, T, p.kbits), s, [&]() {
    // discriminator input rows [0,B) = labels + noise_real (gan_rnn_placeholder.py:207,212; utils/ops.py:19-30)
    if (!p.dsplit) launch_add_noise_rows(lab_tm, p.nr, xd, B, T, Dout, ldDout, 2 * B, 0, s);
    d_run_forward(p, s);
    d_run_head_backward(p, s);
    if (p.inl) apply_body(RSRGAN_NET_D, s);
  });
  dlog_T = T; dlog_rows = 2 * B; dlog_fake0 = (size_t)B;      // logits row t * 2B + n: n < B real, the rest fake
  d_partial_fresh = false;        // (a later rsrgan_apply -- after the caller's all-reduce -- squares the gradients it finds)
  g_fwd_valid = true;
  if (p.inl) apply_inlined |= 2;
  if (want_grads) { finish_buckets(RSRGAN_NET_D, s); d_grads_ready = true; }
  if (out_losses) launch_copy_f(losses, out_losses, 3, s);
  HIPC(hipGetLastError());
  return RSRGAN_OK;
}

// ------------------------------------------------------------------------------------------ the G-run
// Makes no launch.  Every decision here is one a replayed segment could not make: its body does not run.
GRunPlan Model::plan_g_run(int T, const float* nf, bool want_grads, bool reuse, hipStream_t s) {
  GRunPlan p;
  p.T = T; p.R = T * B; p.want_grads = want_grads; p.reuse = reuse; p.nf = nf;
  p.l2_on = !cfg.cross_validation && scal[RSRGAN_L2_SCALE] > 0.0;
  p.wave_bwd = want_grads && !d_dnn() && wavefront();
  const bool fused_seg = switches().fused_seg;
  p.bucketed = p.wave_bwd && gbk[RSRGAN_NET_G].size() > 1 && !overlap() && !(fused_apply && fused_seg);
  p.dy = g_dB;                                    // (the G-side ping-pong of the wavefront backward is g_dA / g_dC)
  if (p.wave_bwd) {
    p.dch = d_chain(B, B, 0);
    wire_d_bptt(p.dch, false, p.dy, true);        // layer 0's input gradient lands on top of the mse term in dy
    p.gch = g_chain(T);
    p.dh0 = wire_g_bptt(p.gch, g_dA, g_dC);
    // (res_lstm_i inside the check reads gp_trail_next: false here, as at every call site this answer replaced)
    p.g_bptt_persist = dl[0].ldI == ldDout && persist_backward_g(p.gch, T, s, true);
  }
  const bool fc_side_env = switches().wgrad_streams >= 2 && switches().fc_side;
  p.fcs_inside = p.wave_bwd && !p.bucketed && side && fc_side_env && cfg.g_type == RSRGAN_G_LSTM && p.g_bptt_persist;
  p.inl = fused_apply && fused_seg && p.wave_bwd && !p.bucketed && graphs_on() && !(cfg.g_type == RSRGAN_G_LSTM && !p.fcs_inside);
  p.kbits = (want_grads ? 1u : 0u) | (nf ? 2u : 0u) | (reuse ? 4u : 0u) | (p.l2_on ? 8u : 0u) | (p.bucketed ? 16u : 0u) | (p.inl ? 32u : 0u);
  if (p.g_bptt_persist) {
    Chain dc0 = p.dch;
    dc0[0].din = nullptr;
    p.trail_plan = persist_backward_trail(dc0, T, s, p.dy, ldDout, g_dA, pad4(gR), true);
  }
  p.gsplit = dpipe && p.trail_plan;
  return p;
}

// the two FCs' parameter gradients as the riders chain_wgrads puts on the side stream (fcs_inside): the output FC's need dy, complete in
// front of the generator's BPTT; the input FC's need the d(h0) GEMM behind it
void Model::g_fc_side_pair(const GRunPlan& p, StreamFn& pre, StreamFn& post) {
  if (!p.fcs_inside) return;
  const float* dy = p.dy; float* dh0 = p.dh0; const int R = p.R;
  pre = [this, dy, R](hipStream_t q) { g_fc_out_wgrads(dy, R, q); };
  // through leakyrelu and the input FC (models/lstm.py:82-87)
  post = [this, dh0, R](hipStream_t q) { g_fc_in_backward(dh0, R, (side && q == side) ? scratch2 : scratch, q); };
}

// The generator's forward of a run that does not reuse one, in the best form that applies: with D(G(x)) trailing in the same launch
// (k_glstm_fwd_dt), as one persistent launch + the output FC, as ONE wave with the discriminator, layer by layer.  True: D(G(x)) ran with
// it -- y, the discriminator's input rows and its stash are there.
bool Model::g_run_forward(const GRunPlan& p, hipStream_t s) {
  const int T = p.T;
  if (p.reuse) return false;
  if (!wavefront()) { g_forward(T, s); return false; }
  if (gp_fwd_on()) {
    g_forward_head(T, s);
    if (!d_dnn()) {
      Chain dch = d_chain(B, B, 0);
      if (persist_forward_g_trail(dch, T, s, p.nf)) return true;
    }
    if (g_forward_persist(T, s)) return false;
  }
  // ONE forward wave: G's layers | per-step output FC (-> y_t and D's input rows, noise added) | D's layers
  if (!gp_fwd_on()) g_forward_head(T, s);
  std::vector<Chain> chains{g_chain(T)};
  std::vector<int> offs{0};
  if (!d_dnn()) { chains.push_back(d_chain(B, B, 0)); offs.push_back((int)gl.size() + 1); }
  std::vector<FcStage> fcs{g_out_fc_stage(p.nf, B, 0)};
  rnn_forward(chains, T, s, &offs, &fcs);
  return true;
}

// D(G(x)) on y + noise (utils/ops.py:19-30) behind a generator forward that did not carry it
void Model::g_run_d_forward(const GRunPlan& p, hipStream_t s) {
  const int T = p.T;
  // Without a noise draw (init_disc_noise_std = 0, the shipped recipe) the discriminator reads y where it lies -- the same [T][B][ld]
  // layout as its input rows --: one launch less in front of the recurrence
  const bool direct = !p.nf && !d_dnn() && dl[0].ldI == ldDout;
  if (!direct) launch_add_noise_rows(y_tm, p.nf, xd, B, T, Dout, ldDout, B, 0, s);
  if (d_dnn()) return;
  std::vector<Chain> chains(1, d_chain(B, B, 0));
  if (direct) chains[0][0].in = y_tm;
  if (!persist_forward(chains[0], T, s) && !fold_forward(chains[0], T, s)) rnn_forward(chains, T, s);
}

// g_adv = mean((D(G(x)) - d_real)^2)  (gan_rnn_placeholder.py:246): all rows "fake", target d_real.  Returns whether the fused head ran.
bool Model::g_run_loss_head(const GRunPlan& p, hipStream_t s) {
  bool g_head = false;
  if (d_dnn()) d_dnn_forward_loss(p.T, B, 0, p.want_grads, tmp3, s);
  else g_head = d_head_or_logits(B, p.T, 0, dyn + DYN_D_REAL, tmp3, p.want_grads, false, s);
  launch_copy_f(tmp3 + 1, losses + 3, 1, s);
  return g_head;
}

// The mse term and the backward pass through D into G.  False: the run is split behind the fused BPTT launch (gsplit) -- nothing more
// belongs to this segment, g_run_bwd_rest is the next one.
bool Model::g_run_backward(const GRunPlan& p, bool g_head, hipStream_t s) {
  const int T = p.T, R = p.R;
  if (!p.want_grads) {
    launch_mse(y_tm, lab_tm, ldDout, nullptr, R, Dout, dyn + DYN_LAMBDA, false, losses + 4, scratch, s, pad_Bp(), Bt);
    return true;
  }
  if (d_dnn()) {
    // discriminator_dnn: data gradient through the FC stack (time-batched GEMMs), then the generator's BPTT wave
    float* dyd = fc_backward(D, dfc, d_act, R, dlogits, false, true, s);      // [T*B][ldDout] (d_joint_dim == 0)
    launch_mse(y_tm, lab_tm, ldDout, dyd, R, Dout, dyn + DYN_LAMBDA, true, losses + 4, scratch, s, pad_Bp(), Bt);
    g_backward_pass(T, dyd, s);
    return true;
  }
  if (!p.wave_bwd) {
    d_backward_pass(B, T, false, true, dlogits, s, g_head);
    float* dyd = last_dx0;                        // d g_adv / d y
    launch_mse(y_tm, lab_tm, ldDout, dyd, R, Dout, dyn + DYN_LAMBDA, true, losses + 4, scratch, s, pad_Bp(), Bt);
    g_backward_pass(T, dyd, s);
    return true;
  }
  // ONE backward wave: D's layers (data gradient only) | per-step output-FC backward | G's layers.
  // dy[t] = lambda*(y-lab)/(B*T) (written first) + d g_adv/d y[t] (accumulated by D layer 0's phase B)
  const int Ld = (int)dl.size(), ldPd = pad4(dR);
  if (!g_head) gemm(dlogits, 4, true, D.W(d_fc_w), 4, true, d_dB, ldPd, R, dR, 1, nullptr, 0, 0.f, false, s);      // d(D outputs) = dlogits . W^T
  launch_mse(y_tm, lab_tm, ldDout, p.dy, R, Dout, dyn + DYN_LAMBDA, false, losses + 4, scratch, s, pad_Bp(), Bt);
  if (p.g_bptt_persist) {
    if (!g_run_bptt_fused(p, s)) return false;
  } else {
    FcStage F;                                     // d(ins[L])[t] = dy[t] . W_out^T
    F.offset = Ld; F.N = B; F.K = Dout; F.D = gR;
    F.in = p.dy; F.ld_in = ldDout; F.WT = G.W(g_fc_out_w); F.y = g_dA; F.ldy = pad4(gR); F.accumulate = false;
    std::vector<int> offs{0, Ld + 1};
    std::vector<FcStage> fcs{F};
    std::vector<Chain> chains{p.dch, p.gch};
    ScopedSet<bool> defer(defer_wgrads, p.bucketed);
    rnn_backward(chains, T, s, &offs, &fcs);
  }
  // output FC parameter gradients (batched over time, dy is complete now)
  if (!p.fcs_inside) g_fc_out_wgrads(p.dy, R, s);
  return true;
}

// The generator's BPTT as ONE persistent launch: the discriminator's data gradient in its trailing form INSIDE that launch
// (k_glstm_bwd_dt; the generator's top layer polls its gradient step by step: dy and g_dA are completed there), or first and alone (its
// own persistent launch, layer 0's input gradient as a GEMM on top of the mse term in dy, then the output FC's data gradient as one GEMM).
// False: gsplit -- the launch only, ev_dfree is recorded behind it and what follows is a segment of its own (g_run_bwd_rest).
bool Model::g_run_bptt_fused(const GRunPlan& p, hipStream_t s) {
  const int T = p.T, R = p.R, ldP = pad4(gR);
  ScopedSet<bool> defer(defer_wgrads, p.bucketed);
  std::vector<Chain> dc1(1, p.dch);
  dc1[0][0].din = nullptr;
  const bool trailed = p.trail_plan && persist_backward_trail(dc1[0], T, s, p.dy, ldDout, g_dA, ldP);
  if (!trailed) {
    if (!persist_backward(dc1[0], T, s)) rnn_backward(dc1, T, s);
    const int H4d = 4 * dl[0].H;
    gemm(d_st[0].gates, H4d, true, D.W(dl[0].tK), H4d, true, p.dy, ldDout, R, dl[0].I, H4d, nullptr, 0, 0.f, true, s);
    gemm(p.dy, ldDout, true, G.W(g_fc_out_w), ldDout, true, g_dA, ldP, R, gR, Dout, nullptr, 0, 0.f, false, s);
  }
  ScopedSet<bool> trail(gp_trail_next, trailed);
  StreamFn pre, post;
  g_fc_side_pair(p, pre, post);
  ScopedSet<int> phase(gp_phase, p.gsplit ? 1 : 0);
  persist_backward_g(p.gch, T, s, false, pre, post);
  return !p.gsplit;
}

// what follows the fused launch of a split run: layer 0's input gradient, the weight gradients, the FCs' (and the inlined update)
void Model::g_run_bwd_rest(const GRunPlan& p, hipStream_t s) {
  StreamFn pre, post;
  g_fc_side_pair(p, pre, post);
  {
    // the next D-run's D(real) (32 workgroups that own their CUs) runs beside these launches when the host is ahead: the chip-filling
    // GEMMs leave it room (a persistent stream-K launch on all 256 CUs would wait for it with 32 of its workers, and it for them)
    ScopedSet<int> workers(g_gemm_workers, std::min(g_gemm_workers, switches().dpipe_w));
    {
      ScopedSet<bool> defer(defer_wgrads, p.bucketed);
      ScopedSet<int> phase(gp_phase, 2);
      persist_backward_g(p.gch, p.T, s, false, pre, post);
    }
    if (!p.fcs_inside) g_fc_out_wgrads(p.dy, p.R, s);
  }
  if (p.inl) { g_run_tail(p, s); apply_body(RSRGAN_NET_G, s); }
}

void Model::g_run_tail(const GRunPlan& p, hipStream_t s) {
  g_loss_tail(p.want_grads && p.l2_on, s);
  // the G-run's update ops, at the end of the run and inside its captured segment: the generator's, twice with the same batch
  if (seq_bn() && p.want_grads && bn_training()) seq_bn_commit(2, s);
}

int Model::g_backward(const float* x, const float* labels, const int32_t* lengths, int T, const float* nf,
                      float* out_losses, bool want_grads, bool reuse, hipStream_t s) {
  if (!labels) { set_error("labels required"); return RSRGAN_ERR_INVALID; }
  dlog_T = 0;                                      // the run's discriminator head writes D(G(x)) over the D-run's logits
  if (g_dnn()) return dnn_g_backward(x, labels, T, out_losses, want_grads, reuse, s);
  if (g_bnl()) return bnl_step(x, labels, lengths, T, out_losses, want_grads, s);
  bn_eval_call = !want_grads;                      // (is_training of this fetch)
  if (seq_bn() && want_grads && cfg.cross_validation) {
    set_error("RSRGAN_FLAG_BATCH_NORM: gradients of the cross_validation model (moving-statistics batch norm) are not built");
    return RSRGAN_ERR_INVALID;
  }
  if (seq_bn() && reuse && g_fwd_bn_train != bn_training()) reuse = false;      // the forward at hand normalised the other way
  if (seq_bn() && !reuse) g_fwd_bn_train = bn_training();
  dfree_current = false;                           // this run reads and writes the discriminator's stash
  if (seq_drop_on()) { reuse = false; launch_drop_tick(drop_ctr, s); }     // a new sess.run: new DropoutWrapper masks, a new forward
  if (supervised()) return g_supervised_step(x, labels, lengths, T, out_losses, want_grads, s);
  if (d_dnn()) nf = nullptr;
  if (reuse) {
    if (!g_fwd_valid || T != cur_T) { set_error("reuse_g_forward without a valid generator forward"); return RSRGAN_ERR_STATE; }
  } else {
    int rc = prepare_batch(x, labels, lengths, T, s);
    if (rc) return rc;
  }
  nf = stage_noise(nf, noise_f_buf, s);
  const GRunPlan p = plan_g_run(T, nf, want_grads, reuse, s);

  run_seg(seg_key(SEG_G_MAIN, T, p.kbits | (p.trail_plan ? 64u : 0u) | (p.gsplit ? 128u : 0u)), s, [&]() {
    // (trailing form) the top layer's gradient buffer armed with the all-ones pattern HERE, at the head of the run: k_glstm_bwd polls it,
    // and a fill in front of the fork would be the node both launches depend on (a fill node as the fork point serialized them)
    if (p.trail_plan) gpersist_arm_bytes(g_dA, (size_t)T * B * pad4(gR) * sizeof(float), s);
    if (!g_run_forward(p, s)) g_run_d_forward(p, s);
    const bool g_head = g_run_loss_head(p, s);
    if (!g_run_backward(p, g_head, s)) return;
    if (p.inl) { g_run_tail(p, s); apply_body(RSRGAN_NET_G, s); }
  });
  if (p.gsplit) {
    (void)hipEventRecord(ev_dfree, s);
    dfree_inside = true; dfree_current = true;
    run_seg(seg_key(SEG_G_MAIN, T, p.kbits | 64u | 256u), s, [&]() { g_run_bwd_rest(p, s); });
  }
  if (p.inl) apply_inlined |= 1;
  if (!reuse) g_fwd_valid = true;
  if (p.wave_bwd) {
    int bi = 0;
    if (p.bucketed) mark_bucket(RSRGAN_NET_G, bi++, s);
    if (cfg.g_type == RSRGAN_G_LSTM && !p.fcs_inside) {
      // through leakyrelu and the input FC (models/lstm.py:82-87)
      run_seg(seg_key(SEG_G_FCIN, T, p.kbits), s, [&]() { g_fc_in_backward(p.dh0, p.R, scratch, s); });
      if (p.bucketed) mark_bucket(RSRGAN_NET_G, bi++, s);
    }
    if (p.bucketed) {        // LSTM weight gradients layer by layer: each completes one bucket (all-reduced while the next runs)
      // (same-shaped layers: every layer's dWp and column sums first, as one launch per kind -- decided on the host, a replayed
      //  segment does not run its body -- then a layer's bucket is complete behind its dK GEMM)
      bool dkd = false;
      const bool gb = batch_wgrads(p.gch, T, s, false, &dkd, true);
      if (gb) run_seg(seg_key(SEG_G_BATCH, T, p.kbits), s, [&]() { bool d_ = false; (void)batch_wgrads(p.gch, T, s, false, &d_); });
      int li = 0;
      for (auto& Rr : p.gch) {
        run_seg(seg_key(SEG_G_LAYER0 + li, T, p.kbits), s, [&]() { if (gb) layer_wgrads_gemms(Rr, 0, T, false, s, true, false); else layer_wgrads(Rr, T, s); });
        mark_bucket(RSRGAN_NET_G, bi++, s);
        ++li;
      }
    }
  }
  if (!p.inl) run_seg(seg_key(SEG_G_TAIL, T, p.kbits), s, [&]() { g_run_tail(p, s); });
  if (want_grads) {
    if (p.l2_on) for (auto& bk : gbk[RSRGAN_NET_G]) bk.marked = false;      // the L2 term touches every tensor: all buckets final only now
    finish_buckets(RSRGAN_NET_G, s);
    g_grads_ready = true;
  }
  if (out_losses) launch_copy_f(losses + 3, out_losses, 4, s);
  HIPC(hipGetLastError());
  return RSRGAN_OK;
}

// RNNTrainer's step (models/rnn_trainer.py:131-156): g_loss = 0.5*Dout*mse(G(x), labels) + l2; no discriminator in the graph
int Model::g_supervised_step(const float* x, const float* labels, const int32_t* lengths, int T, float* out_losses, bool want_grads, hipStream_t s) {
  int rc = prepare_batch(x, labels, lengths, T, s);
  if (rc) return rc;
  g_forward(T, s);
  const bool l2s = !cfg.cross_validation && scal[RSRGAN_L2_SCALE] > 0.0;
  HIPC(hipMemsetAsync(losses + 3, 0, sizeof(float), s));
  if (want_grads) {
    float* dy = g_dC;                            // g_backward_pass ping-pongs g_dA / g_dB
    launch_mse(y_tm, lab_tm, ldDout, dy, T * B, Dout, dyn + DYN_LAMBDA, false, losses + 4, scratch, s, pad_Bp(), Bt);
    g_backward_pass(T, dy, s);
    // (not g_loss_tail: the update ops and the bucket events lie between the L2 launches and the total here)
    if (l2s) {
      launch_l2(G.w, G.g, G.ct, dyn + DYN_L2, G.partial, s);
      launch_l2_total(G.partial, G.ct.n_chunks, dyn + DYN_L2, losses + 5, s);
    }
    if (seq_bn() && bn_training()) seq_bn_commit(2, s);      // rnn_trainer.py:131-132,148-150: the generator is built twice
    { finish_buckets(RSRGAN_NET_G, s); g_grads_ready = true; }
  } else {
    launch_mse(y_tm, lab_tm, ldDout, nullptr, T * B, Dout, dyn + DYN_LAMBDA, false, losses + 4, scratch, s, pad_Bp(), Bt);
  }
  if (!(want_grads && l2s)) HIPC(hipMemsetAsync(losses + 5, 0, sizeof(float), s));
  launch_g_total(losses + 3, dyn + DYN_LAMBDA, s);
  if (out_losses) launch_copy_f(losses + 3, out_losses, 4, s);
  HIPC(hipGetLastError());
  return RSRGAN_OK;
}

// the bnlstm trainer's step (models/rnn_trainer.py:131-156 on models/bnlstm.py): g_loss = 0.5*Dout*mse + l2.  A training fetch
// (gradients on a cross_validation=0 handle) normalises with each step's batch statistics and advances the moving statistics;
// an evaluation fetch normalises with the moving statistics.  One graph segment per (T, kind of fetch).
int Model::bnl_step(const float* x, const float* labels, const int32_t* lengths, int T, float* out_losses, bool want_grads, hipStream_t s) {
  if (want_grads && cfg.cross_validation) {
    set_error("g_type bnlstm: gradients of the cross_validation model (moving-statistics batch norm) are not built");
    return RSRGAN_ERR_INVALID;
  }
  int rc = prepare_batch(x, labels, lengths, T, s);
  if (rc) return rc;
  const bool l2s = want_grads && scal[RSRGAN_L2_SCALE] > 0.0;
  run_seg(seg_key(SEG_BNL, T, (want_grads ? 1u : 0u) | (l2s ? 2u : 0u)), s, [&]() {
    bnl_forward(T, want_grads, s);
    (void)hipMemsetAsync(losses + 3, 0, sizeof(float), s);
    float* dy = want_grads ? g_dC : nullptr;
    launch_mse(y_tm, lab_tm, ldDout, dy, T * B, Dout, dyn + DYN_LAMBDA, false, losses + 4, scratch, s, pad_Bp(), Bt);
    if (want_grads) bnl_backward(T, dy, s);
    g_loss_tail(l2s, s);
  });
  if (want_grads) { finish_buckets(RSRGAN_NET_G, s); g_grads_ready = true; }
  g_fwd_valid = false;
  if (out_losses) launch_copy_f(losses + 3, out_losses, 4, s);
  HIPC(hipGetLastError());
  return RSRGAN_OK;
}

// per-tensor clip_by_norm + the optimizer + EMA + the weight copies (gan_rnn_placeholder.py:177-189): the launches of one update
void Model::apply_body(int net, hipStream_t s) {
  if (net == RSRGAN_NET_D) {
    if (!d_partial_fresh) launch_sumsq(D.g, D.ct, D.partial, s);      // (k_dw_reduce of the same segment has left the sums of squares)
    d_partial_fresh = false;
    if (d_adam()) {                              // models/gan.py:125: d_opt = AdamOptimizer(d_learning_rate)
      launch_adam_tick(dyn, adam_t_dev_d, (double)cfg.adam_beta1, (double)cfg.adam_beta2, s, DYN_D_LR, DYN_ADAM_LRT_D);
      launch_apply_adam(D.w, D.g, D.m, D.v, D.ema, D.ct, D.partial, dyn, s, DYN_ADAM_LRT_D);
    } else {
      launch_apply_sgd(D.w, D.g, D.ema, D.ct, D.partial, dyn, s);
    }
    refresh_transposes(RSRGAN_NET_D, s);
  } else {
    launch_sumsq(G.g, G.ct, G.partial, s);
    launch_adam_tick(dyn, adam_t_dev, (double)cfg.adam_beta1, (double)cfg.adam_beta2, s);
    launch_apply_adam(G.w, G.g, G.m, G.v, G.ema, G.ct, G.partial, dyn, s);
    refresh_transposes(RSRGAN_NET_G, s);
  }
}

int Model::apply(int net, hipStream_t s) {
  if (net == RSRGAN_NET_D) {
    if (!d_grads_ready) { set_error("apply(D) without gradients"); return RSRGAN_ERR_STATE; }
    // (apply_inlined: rsrgan_d_step's backward segment already ran / replayed these launches at its end -- one graph, no boundary)
    if (!(apply_inlined & 2)) run_seg(seg_key(SEG_APPLY_D, 0, 0), s, [&]() { apply_body(RSRGAN_NET_D, s); });
    apply_inlined &= ~2;
    if (d_adam()) scal[RSRGAN_ADAM_STEP_D] += 1;
    d_grads_ready = false;
  } else if (net == RSRGAN_NET_G) {
    if (!g_grads_ready) { set_error("apply(G) without gradients"); return RSRGAN_ERR_STATE; }
    if (!(apply_inlined & 1)) run_seg(seg_key(SEG_APPLY_G, 0, 0), s, [&]() { apply_body(RSRGAN_NET_G, s); });
    // (RSRGAN_DPIPE: the generator's update touches nothing the next D(real) reads or writes, so the event stays where the G-run's
    // backward launch -- or the previous call's end -- recorded it; a run that has used the discriminator's stash since and has NOT
    // recorded it leaves the record to the end of this call)
    if (dfree_current) dfree_inside = true;
    apply_inlined &= ~1;
    scal[RSRGAN_ADAM_STEP] += 1;
    g_grads_ready = false;
    g_fwd_valid = false;
  } else {
    set_error("bad net %d", net);
    return RSRGAN_ERR_INVALID;
  }
  HIPC(hipGetLastError());
  return RSRGAN_OK;
}

}  // namespace rsr
