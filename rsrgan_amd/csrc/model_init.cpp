// model_init.cpp -- construction and destruction of a handle: Model::init as a sequence of named stages (DESIGN.md "handle
// construction"), the allocator and its failure rule, the gradient buckets.  Nothing here is on a step's path.
// Reference graph: models/gan_rnn_placeholder.py:139-298 (build_model / build_model_single_gpu), generator models/lstm.py:41-129 |
// models/res_lstm_l.py:41-199, discriminator models/discriminator_lstm.py:24-110.
#include "model.h"

#include <algorithm>
#include <cmath>
#include <random>

namespace rsr {

int ParamSet::add(const std::string& name, int rows, int cols, bool is_vector) {
  TensorDesc d;
  d.name = name;
  d.rows = rows; d.cols = cols; d.ld = pad4(cols);
  d.off = padded; d.dense_off = dense;
  d.l2 = name.find("bias") == std::string::npos;
  d.is_vector = is_vector;
  padded += ((int64_t)rows * d.ld + 63) / 64 * 64;
  dense += (int64_t)rows * cols;
  t.push_back(d);
  return (int)t.size() - 1;
}

// ------------------------------------------------------------------------------------------ device memory
// alloc: a REQUIRED buffer -- a failure is recorded on the handle and the running stage refuses the handle at its next alloc_status().
// alloc_opt: a buffer whose absence the caller handles (a path switched off, a size shrunk): nullptr, nothing recorded.
void* Model::alloc_raw(size_t bytes, bool required) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    if (required && !alloc_fail) { alloc_fail = true; alloc_fail_bytes = bytes; }
    return nullptr;
  }
  (void)hipMemset(p, 0, bytes);
  allocs.push_back(p);
  alloc_bytes += bytes;
  return p;
}
template <typename T> T* Model::alloc(size_t n) { return reinterpret_cast<T*>(alloc_raw((n ? n : 1) * sizeof(T), true)); }
template <typename T> T* Model::alloc_opt(size_t n) { return reinterpret_cast<T*>(alloc_raw((n ? n : 1) * sizeof(T), false)); }
template float* Model::alloc<float>(size_t);          // (bnlstm.cpp and model.cpp use these)
template int* Model::alloc<int>(size_t);
template float* Model::alloc_opt<float>(size_t);

int Model::alloc_status(const char* stage) const {
  if (!alloc_fail) return RSRGAN_OK;
  set_error("hipMalloc failed (%s: %zu bytes)", stage, alloc_fail_bytes);
  return RSRGAN_ERR_HIP;
}

static void add_lstm(ParamSet& ps, std::vector<LstmLayer>& out, const std::string& prefix, int I, int H, int proj) {
  LstmLayer L;
  const int P = proj > 0 ? proj : H;
  L.has_proj = proj > 0;
  L.I = I; L.H = H; L.P = P; L.ldI = pad4(I); L.ldP = pad4(P); L.ldH = pad4(H);
  L.tK = ps.add(prefix + "/kernel", I + P, 4 * H, false);
  L.tb = ps.add(prefix + "/bias", 1, 4 * H, true);
  L.twf = ps.add(prefix + "/w_f_diag", 1, H, true);
  L.twi = ps.add(prefix + "/w_i_diag", 1, H, true);
  L.two = ps.add(prefix + "/w_o_diag", 1, H, true);
  L.tWp = L.has_proj ? ps.add(prefix + "/projection/kernel", H, P, false) : -1;
  out.push_back(L);
}

// the host half of a ChunkTable (no HIP call): tensor i is floats[i] floats at float offset off[i] of the flat buffer, cut into
// 4096-float chunks in tensor order, the last chunk of a tensor short.  build_chunks below and the rsrgan_op_update test entry call it.
void chunk_table_host(const int64_t* toff, const int64_t* floats, const int* l2, int n, ChunkTableHost& out) {
  constexpr int CH = 4096;
  out = ChunkTableHost();
  for (int i = 0; i < n; ++i) {
    out.t_first.push_back((int)out.tensor.size());
    int cnt = 0;
    for (int64_t o = 0; o < floats[i]; o += CH) {
      out.tensor.push_back(i);
      out.off.push_back((int)(toff[i] + o));
      out.len.push_back((int)std::min<int64_t>(CH, floats[i] - o));
      ++cnt;
    }
    out.t_count.push_back(cnt);
    out.t_l2.push_back(l2[i] ? 1 : 0);
  }
}

static int build_chunks(Model& M, ParamSet& ps) {
  std::vector<int64_t> toff, floats;
  std::vector<int> l2;
  for (const TensorDesc& d : ps.t) {
    toff.push_back(d.off);
    floats.push_back((int64_t)d.rows * d.ld);
    l2.push_back(d.l2 ? 1 : 0);
  }
  ChunkTableHost h;
  chunk_table_host(toff.data(), floats.data(), l2.data(), (int)ps.t.size(), h);
  auto up = [&](const std::vector<int>& v, const int*& dst) -> hipError_t {      // (a failed allocation is the stage's to report)
    int* d = M.alloc<int>(v.size());
    dst = d;
    return d ? hipMemcpy(d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice) : hipSuccess;
  };
  HIPC(up(h.tensor, ps.ct.tensor)); HIPC(up(h.off, ps.ct.off)); HIPC(up(h.len, ps.ct.len));
  HIPC(up(h.t_first, ps.ct.t_first)); HIPC(up(h.t_count, ps.ct.t_count)); HIPC(up(h.t_l2, ps.ct.t_l2));
  ps.ct.n_chunks = (int)h.tensor.size();
  ps.ct.n_tensors = (int)ps.t.size();
  ps.partial = M.alloc<float>(h.tensor.size());
  return RSRGAN_OK;
}

static void alloc_stash(Model& M, LstmStash& S, const LstmLayer& L, int N, int T) {
  S.gates = M.alloc<float>((size_t)T * N * 4 * L.H);
  S.c = M.alloc<float>((size_t)(T + 1) * N * L.H);
  S.h = M.alloc<float>((size_t)T * N * L.ldH);
  S.mst = M.alloc<float>((size_t)(T + 1) * N * L.ldP);
  S.out = M.alloc<float>((size_t)T * N * L.ldP);
  S.dmt = M.alloc<float>((size_t)T * N * L.ldP);
  S.dc = M.alloc<float>((size_t)N * L.H);
  S.dmst = M.alloc<float>((size_t)N * L.ldP);
}

// An inference handle's stash (RSRGAN_FLAG_INFER): the carried states of W + 1 steps and the layer's outputs -- of W steps, or of all T
// where the output FC reads them (out_T).  gates / h, which only the launch-per-phase path touches, come with its first use
// (Model::infer_fallback_stash); nothing of the backward pass exists.
static void alloc_stash_infer(Model& M, LstmStash& S, const LstmLayer& L, int N, int W, int out_T) {
  S.c = M.alloc<float>((size_t)(W + 1) * N * L.H);
  S.mst = M.alloc<float>((size_t)(W + 1) * N * L.ldP);
  S.out = M.alloc<float>((size_t)out_T * N * L.ldP);
}

// the control block of a persistent launch (kernels.h DP_CTL_*) in its initial state: generation 1, no workgroup finished, no error
static hipError_t ctl_reset(unsigned* ctl) {
  const unsigned ctl0[DP_CTL_WORDS] = {1u, 0u, 0u, 0u};
  return hipMemcpy(ctl, ctl0, sizeof(ctl0), hipMemcpyHostToDevice);
}

int Model::init(const rsrgan_cfg& c, uint64_t seed) {
  cfg = c;
  B = Bt = c.batch_size; Tmax = c.max_frames; Din = c.input_dim; Dout = c.output_dim;
  ldDin = pad4(Din); ldDout = pad4(Dout);
  gR = c.g_proj > 0 ? c.g_proj : c.g_cells;
  dR = c.d_proj > 0 ? c.d_proj : c.d_cells;
  if (int rc = check_cfg()) return rc;
  build_tables();
  plan_rows();
  if (int rc = alloc_params()) return rc;
  if (int rc = alloc_generator()) return rc;
  if (int rc = alloc_discriminator()) return rc;
  if (int rc = alloc_shared()) return rc;          // (in front of plan_persistent: the DPIPE ring needs the side stream)
  if (int rc = plan_persistent()) return rc;
  return init_values(seed);
}

// ------------------------------------------------------------------------------------------ stage 1: refusals
// Every refusal that depends on cfg and switches() alone, in the order a configuration with two faults has always been reported.
int Model::check_cfg() const {
  const rsrgan_cfg& c = cfg;
  if (B <= 0 || Tmax <= 0 || Din <= 0 || Dout <= 0 || c.g_layers <= 0 || c.d_layers <= 0 || c.g_cells <= 0 ||
      c.d_cells <= 0 || (c.g_layers > MAXJ && !g_dnn()) || c.d_layers > MAXJ) {
    set_error("invalid sizes in rsrgan_cfg");
    return RSRGAN_ERR_INVALID;
  }
  if (infer() && g_dnn()) {
    set_error("RSRGAN_FLAG_INFER: an inference-only handle for g_type %d is not built (the sequence generators lstm, res_lstm_l, res_lstm_base, res_lstm_i, bnlstm only)", c.g_type);
    return RSRGAN_ERR_INVALID;
  }
  if (c.d_type != RSRGAN_D_LSTM && c.d_type != RSRGAN_D_DNN) { set_error("Unrecognized D type %d", c.d_type); return RSRGAN_ERR_INVALID; }
  if (g_dnn() && !d_dnn()) { set_error("the frame-level generator (dnn) needs discriminator_dnn (models/gan.py:104)"); return RSRGAN_ERR_INVALID; }
  if (!g_dnn() && (c.g_proj < 0 || c.g_proj > 384)) { set_error("generator num_proj must be in [0, 384] (0 = num_proj=None)"); return RSRGAN_ERR_INVALID; }
  if (!d_dnn() && (c.d_proj < 0 || c.d_proj > 384)) { set_error("discriminator num_proj must be in [0, 384] (0 = num_proj=None)"); return RSRGAN_ERR_INVALID; }
  if (!g_dnn() && d_dnn() && c.d_joint_dim != 0) { set_error("discriminator_dnn on the sequence model is fed the target only (d_joint_dim must be 0)"); return RSRGAN_ERR_INVALID; }
  if (!g_dnn() && 2 * pad4(gR) > 1024) { set_error("generator layer input+state wider than 1024 floats is not supported by k_fwd_gates"); return RSRGAN_ERR_INVALID; }
  if (!d_dnn() && pad4(dR) + std::max(pad4(dR), pad4(c.output_dim)) > 1024) { set_error("discriminator layer too wide for k_fwd_gates"); return RSRGAN_ERR_INVALID; }
  if (d_dnn() && (c.d_joint_dim < 0 || c.d_joint_off < 0 || c.d_joint_off + c.d_joint_dim > Din)) { set_error("bad d_joint slice"); return RSRGAN_ERR_INVALID; }
  if (g_bnl()) { const int rc = bnl_check(c); if (rc) return rc; }
  if (bn_on() && !g_dnn()) {
    // the sequence path: the flag acts in models/lstm.py:61-87 alone (res_lstm_*'s input FC is commented out, discriminator_lstm's too)
    if (c.g_type != RSRGAN_G_LSTM) {
      set_error("RSRGAN_FLAG_BATCH_NORM on the sequence path is built for g_type lstm only (the reference's res_lstm_* generators ignore "
                "batch_norm: build them without the flag; bnlstm's input-FC batch norm is not built), got g_type %d", c.g_type);
      return RSRGAN_ERR_INVALID;
    }
    if (c.d_type != RSRGAN_D_LSTM) {
      set_error("RSRGAN_FLAG_BATCH_NORM with a sequence generator needs discriminator_lstm (discriminator_dnn's batch norm is built for the frame-level generators only)");
      return RSRGAN_ERR_INVALID;
    }
  }
  if (bn_on() && g_dnn()) {      // the update ops of a run are ONE launch over a fixed table (kernels.h BnCommitList): refuse what it cannot hold
    const int nbn = (c.g_type == RSRGAN_G_RCED ? 9 : c.g_layers) + (c.d_type == RSRGAN_D_DNN ? c.d_layers : 0);
    if (nbn > 24) { set_error("batch norm: %d normalised layers, at most 24 are supported", nbn); return RSRGAN_ERR_INVALID; }
  }
  switch (c.g_type) {
    case RSRGAN_G_RCED:
      if (c.g_splice <= 0 || Din % c.g_splice) { set_error("R-CED: input_dim must be g_splice x frame width"); return RSRGAN_ERR_INVALID; }
      if (c.g_layers < 1 || c.g_layers > 9) { set_error("R-CED: g_layers must be in [1, 9]"); return RSRGAN_ERR_INVALID; }
      break;
    case RSRGAN_G_RES_LSTM_L:
      if (gR != Din) { set_error("res_lstm_l needs g_proj == input_dim (models/res_lstm_l.py:111)"); return RSRGAN_ERR_INVALID; }
      break;
    case RSRGAN_G_RES_LSTM_I:
      // models/res_lstm_i.py:101-190: the same cells and variable names; the sums are outputs_l + the stack's input
      if (!supervised()) {
        set_error("g_type res_lstm_i is built for the supervised trainer only (RSRGAN_FLAG_SUPERVISED; the reference GAN has no res_lstm_i generator)");
        return RSRGAN_ERR_INVALID;
      }
      if (gR != Din) { set_error("res_lstm_i needs g_proj == input_dim (models/res_lstm_i.py:111)"); return RSRGAN_ERR_INVALID; }
      break;
    case RSRGAN_G_DNN: case RSRGAN_G_LSTM: case RSRGAN_G_RES_LSTM_BASE: case RSRGAN_G_BNLSTM:
      break;
    default:
      set_error("Unrecognized G type %d", c.g_type);                       // gan_rnn_placeholder.py:131-132
      return RSRGAN_ERR_INVALID;
  }
  return RSRGAN_OK;
}

// ------------------------------------------------------------------------------------------ stage 2: variable tables
// in graph-construction order (gan_rnn_placeholder.py:301-317): the sequence of ParamSet::add calls defines every offset
void Model::build_tables() {
  const rsrgan_cfg& c = cfg;
  const int P = gR, H = c.g_cells;
  auto fc_name = [](const char* net, int i) { return std::string(net) + "/fully_connected" + (i == 0 ? "" : "_" + std::to_string(i)); };
  // <scope>/BatchNorm/* in normalization.py's build order (contrib layers create no biases under a normalizer_fn)
  auto add_bn = [&](ParamSet& ps, const std::string& nm, int o, int (&tbn)[8]) {
    static const char* kBn[8] = {"beta", "gamma", "moving_mean", "moving_variance", "renorm_mean", "renorm_mean_weight", "renorm_stddev",
                                 "renorm_stddev_weight"};
    for (int k = 0; k < 8; ++k) {
      const bool scalar = k == 5 || k == 7;
      tbn[k] = ps.add(nm + "/BatchNorm/" + kBn[k], 1, scalar ? 1 : o, true);
      ps.t[tbn[k]].l2 = false;                                     // constant-initialised, never regularised
      ps.t[tbn[k]].bias_init = (k == 1 || k == 3) ? 1.f : 0.f;     // gamma = 1, moving_variance = 1
      ps.t[tbn[k]].trainable = k < 2;
    }
  };
  auto add_fc = [&](ParamSet& ps, std::vector<FcLayer>& out, const std::string& nm, int in, int o, bool bn = false) {
    FcLayer F; F.in = in; F.out = o; F.ld_in = pad4(in); F.ld_out = pad4(o);
    F.tW = ps.add(nm + "/weights", in, o, false);
    if (bn) {
      F.bn = true; F.tb = -1;
      add_bn(ps, nm, o, F.tbn);
    } else {
      F.tb = ps.add(nm + "/biases", 1, o, true);
    }
    out.push_back(F);
  };
  if (c.g_type == RSRGAN_G_RCED) {                                       // models/rced.py:90-116
    static const int kNum[9] = {12, 16, 20, 24, 32, 24, 20, 16, 12}, kWidth[9] = {13, 11, 9, 7, 7, 7, 9, 11, 13};
    rcS = c.g_splice; rcW = Din / c.g_splice;
    int cin = 1;
    for (int l = 0; l < c.g_layers; ++l) {
      // the reference's table; g_cells < 32 scales it down for tests (every width stays a multiple of 4, col2im needs that)
      const int co = c.g_cells >= 32 ? kNum[l] : std::max(4, kNum[l] * c.g_cells / 32 / 4 * 4);
      ConvLayer L; L.fw = kWidth[l]; L.Cin = cin; L.Cout = co; L.K = rcS * L.fw * cin; L.ldK = pad4(L.K);
      L.ldCin = l == 0 ? 1 : pad4(cin); L.ldCout = pad4(co);
      const std::string nm = std::string("g_model/Conv") + (l == 0 ? "" : "_" + std::to_string(l));
      L.tW = G.add(nm + "/weights", L.K, co, false);
      if (bn_on()) { L.bn = true; L.tb = -1; add_bn(G, nm, co, L.tbn); }
      else L.tb = G.add(nm + "/biases", 1, co, true);
      G.t[L.tW].xavier_fan_out = rcS * L.fw * co;           // xavier for conv: receptive field x channels on both sides
      gconv.push_back(L);
      cin = co;
    }
    const int flat = rcS * rcW * cin;
    rc_fc.in = flat; rc_fc.out = Dout; rc_fc.ld_in = flat; rc_fc.ld_out = ldDout;
    rc_fc.tW = G.add("g_model/fully_connected/weights", flat, Dout, false);
    rc_fc.tb = G.add("g_model/fully_connected/biases", 1, Dout, true);
    G.t[rc_fc.tb].bias_init = 0.1f;
  } else if (c.g_type == RSRGAN_G_DNN) {                                 // models/dnn.py:79-110: (1+3) x [FC units, ReLU], FC -> Dout
    int in = Din;
    for (int l = 0; l < c.g_layers; ++l) { add_fc(G, gfc, fc_name("g_model", l), in, c.g_cells, bn_on()); in = c.g_cells; }
    add_fc(G, gfc, fc_name("g_model", c.g_layers), in, Dout);
  } else if (c.g_type == RSRGAN_G_LSTM) {                                // models/lstm.py:82-124
    g_fc_in_w = G.add("g_model/fully_connected/weights", Din, P, false);
    if (bn_on()) {
      // normalizer_fn=batch_norm: no biases.  gan_rnn_placeholder.py:254 / rnn_trainer.py:164 sum l2_loss over every trainable g_ variable
      // without "bias" in its name: beta and gamma TAKE the L2 term here (the frame-level nets regularise weights only)
      add_bn(G, "g_model/fully_connected", P, g_bn_t);
      for (int k = 0; k < 2; ++k) { G.t[g_bn_t[k]].l2 = true; G.t[g_bn_t[k]].const_init = true; }
    } else {
      g_fc_in_b = G.add("g_model/fully_connected/biases", 1, P, true);
    }
    for (int l = 0; l < c.g_layers; ++l)
      add_lstm(G, gl, "g_model/rnn/multi_rnn_cell/cell_" + std::to_string(l) + "/lstm_cell", P, H, c.g_proj);
    g_fc_out_w = G.add("g_model/fully_connected_1/weights", P, Dout, false);
    g_fc_out_b = G.add("g_model/fully_connected_1/biases", 1, Dout, true);
  } else if (g_bnl()) {                                                  // models/bnlstm.py:101-123
    bnl_params();
    if (infer()) bnl_infer_layers();                                     // (the same table; gl = the folded views)
  } else {                                                               // res_lstm_l | res_lstm_base | res_lstm_i: models/res_lstm_l.py:101-194
    int in = Din;
    for (int l = 0; l < c.g_layers; ++l) {
      add_lstm(G, gl, "g_model/lstm_cell_" + std::to_string(l + 1) + "/rnn/lstm_cell", in, H, c.g_proj);
      in = P;
    }
    g_fc_out_w = G.add("g_model/forward_out/fully_connected/weights", P, Dout, false);
    g_fc_out_b = G.add("g_model/forward_out/fully_connected/biases", 1, Dout, true);
  }
  if (infer()) {
    // gan_rnn_placeholder.py:133-135: the generator alone -- RSRGAN_NET_D's table stays empty
  } else if (d_dnn()) {                                                  // models/discriminator_dnn.py:61-92
    int in = c.d_joint_dim + Dout;
    for (int l = 0; l < c.d_layers; ++l) { add_fc(D, dfc, fc_name("d_model", l), in, c.d_cells, bn_on()); in = c.d_cells; }
    add_fc(D, dfc, fc_name("d_model", c.d_layers), in, 1);
  } else {                                                               // models/discriminator_lstm.py:70-104
    int in = Dout;
    for (int l = 0; l < c.d_layers; ++l) {
      add_lstm(D, dl, "d_model/rnn/multi_rnn_cell/cell_" + std::to_string(l) + "/lstm_cell", in, c.d_cells, c.d_proj);
      in = dR;
    }
    d_fc_w = D.add("d_model/fully_connected/weights", dR, 1, false);
    d_fc_b = D.add("d_model/fully_connected/biases", 1, 1, true);
  }
}

// ------------------------------------------------------------------------------------------ stage 3: row padding
// for the persistent generator recurrences (model.h Bt)
void Model::plan_rows() {
  int Bp = (Bt + GP_ROWS - 1) / GP_ROWS * GP_ROWS;
  // (a bnlstm inference handle has no other forward than the persistent one: up to the next count of row groups its plans take -- 1, 2, 4, 8)
  if (bnl_infer()) for (int g : {1, 2, 4, 8}) if (Bp <= g * GP_ROWS) { Bp = g * GP_ROWS; break; }
  if (switches().pad_rows && gp_live && Bp != Bt && !g_dnn() && (!g_bnl() || infer()) && !d_dnn() && wavefront()) {
    B = Bp;
    GPersistArgs ga{};
    if (!gpersist_shape(ga, std::min(Tmax, (int)GP_TMAX))) B = Bt;     // (only where the padded batch does take the persistent path)
  }
}

// ------------------------------------------------------------------------------------------ stage 4: variables and their copies
int Model::alloc_params() {
  const bool inf = infer();                                 // (the variables and their copies only: no gradients, moments, shadows, no discriminator)
  G.w = alloc<float>(G.padded);
  if (!inf) {
    G.g = alloc<float>(G.padded); G.m = alloc<float>(G.padded); G.v = alloc<float>(G.padded);
    G.ema = ema_on() ? alloc<float>(G.padded) : nullptr;
    D.w = alloc<float>(D.padded); D.g = alloc<float>(D.padded);
    if (d_adam()) { D.m = alloc<float>(D.padded); D.v = alloc<float>(D.padded); }
    D.ema = ema_on() ? alloc<float>(D.padded) : nullptr;
  }
  if (int rc = alloc_status("parameters")) return rc;
  if (!inf) {
    if (int rc = build_chunks(*this, G)) return rc;
    if (int rc = build_chunks(*this, D)) return rc;
  }
  if (int rc = alloc_status("chunk tables")) return rc;
  for (auto* layers : {&gl, &dl})
    for (auto& L : *layers) {
      L.KxT = alloc<float>((size_t)4 * L.H * L.ldI);
      L.KhT = alloc<float>((size_t)4 * L.H * L.ldP);
      if (bnl_infer()) {                                    // (the folded bias and cell pair; no launch-per-phase path, so none of its copies)
        L.bias_f = alloc<float>((size_t)4 * L.H); L.ca = alloc<float>(L.H); L.cb = alloc<float>(L.H);
        continue;
      }
      L.WpT = L.has_proj ? alloc<float>((size_t)L.P * L.ldH) : nullptr;
      const int ncb = (L.H + 15) / 16, kbI = (L.ldI + L.ldP + 15) / 16, kbP = (L.ldP + 15) / 16, kbH = (L.ldH + 15) / 16, kb4 = (4 * L.H + 15) / 16;
      L.Wg_full = alloc<float>(swizzle_floats(4 * ncb, kbI));
      L.Wg_h = alloc<float>(swizzle_floats(4 * ncb, kbP));
      L.WpT_sw = L.has_proj ? alloc<float>(swizzle_floats((L.P + 15) / 16, kbH)) : nullptr;
      if (inf) continue;                                    // (the backward phases' copies)
      L.Wp_sw = L.has_proj ? alloc<float>(swizzle_floats(ncb, kbP)) : nullptr;
      L.Kb_full = alloc<float>(swizzle_floats((L.I + L.P + 15) / 16, kb4));
      L.Kb_rec = alloc<float>(swizzle_floats((L.P + 15) / 16, kb4));
    }
  return alloc_status(bnl_infer() ? "bnlstm folded copies" : "weight copies");
}

// ------------------------------------------------------------------------------------------ stage 5: the generator's buffers
int Model::alloc_generator() {
  const bool inf = infer();
  const size_t TB = frame_rows();
  const int ldP = g_ldP();
  x_tm = alloc<float>(TB * ldDin); lab_tm = inf ? nullptr : alloc<float>(TB * ldDout); y_tm = alloc<float>(TB * ldDout);
  g_st.resize(gl.size());
  inf_W = std::min(Tmax, (int)INFER_WINDOW);
  for (size_t l = 0; l < gl.size(); ++l) {
    if (bnl_infer()) alloc_stash_infer(*this, g_st[l], gl[l], B, 1, l + 1 == gl.size() ? Tmax : 0);      // (slots 0 and 1; the top layer's outputs)
    else if (inf) alloc_stash_infer(*this, g_st[l], gl[l], B, inf_W, l + 1 == gl.size() && !res_sums() ? Tmax : inf_W);
    else alloc_stash(*this, g_st[l], gl[l], B, Tmax);
  }
  if (!g_dnn() && (!g_bnl() || inf) && !gl.empty() && gl.size() <= (size_t)GP_MAXL) {      // the carried state of the stateful forward
    for (auto& L : gl) g_state_sf += L.H + L.P;
    g_state = alloc<float>((size_t)B * g_state_sf);
    if (int rc = alloc_status("carried generator state")) return rc;
  }
  g_ins.resize(gl.size() + 1);
  if (g_rced()) {
    alloc_rced();
    if (int rc = alloc_status("R-CED buffers")) return rc;
  } else if (g_dnn()) {
    g_act.push_back(x_tm);
    for (size_t l = 0; l + 1 < gfc.size(); ++l) g_act.push_back(alloc<float>(TB * gfc[l].ld_out));
    g_act.push_back(y_tm);
  } else if (g_bnl() && !inf) {
    bnl_alloc();
    if (int rc = alloc_status("bnlstm buffers")) return rc;
  } else if (cfg.g_type == RSRGAN_G_LSTM || g_bnl()) {
    g_h0 = alloc<float>(TB * ldP);
    g_ins[0] = g_h0;
    for (size_t l = 0; l < gl.size(); ++l) g_ins[l + 1] = g_st[l].out;
    if (seq_bn_infer()) {
      g_bn_fold_b = alloc<float>(ldP);
    } else if (seq_bn()) {
      g_z0 = alloc<float>(TB * ldP); g_bn_stat = alloc<float>((size_t)BN_STAT_ROWS * ldP); g_bn_sums = alloc<float>((size_t)2 * ldP);
      g_bn_scr = alloc<float>((size_t)64 * ldP);
    }
    if (int rc = alloc_status(seq_bn() ? "sequence batch norm" : "activations")) return rc;
  } else {
    g_ins[0] = x_tm;
    for (size_t l = 0; l < gl.size(); ++l) {
      if (res_sums()) {                                     // (res_lstm_i: g_res[l] = out_l + x)
        g_res.push_back(alloc<float>((inf && l + 1 < gl.size() ? (size_t)inf_W * B : TB) * ldP));      // (an inference handle: one window below the top layer)
        g_ins[l + 1] = g_res.back();
      } else {
        g_ins[l + 1] = g_st[l].out;
      }
    }
  }
  const int gmaxld = std::max(std::max(ldP, ldDin), ldDout);      // (g_dB / g_dC also carry dy [T*B][ldDout]: an output wider than the generator's
                                                                  //  layers overflowed them -- found by __graft_entry__.smoke()'s second configuration)
  if (!inf) { g_dA = alloc<float>(TB * gmaxld); g_dB = alloc<float>(TB * gmaxld); g_dC = alloc<float>(TB * gmaxld); }
  return alloc_status("activations");
}

// R-CED (dnn.cpp): activations, the implicit-GEMM convolution's prepared filters and work space, the patch matrices
void Model::alloc_rced() {
  const size_t TB = frame_rows(), M = TB * rcS * rcW;
  int maxC = 4;
  rc_act.push_back(x_tm);
  for (auto& L : gconv) {
    rc_act.push_back(alloc<float>(M * L.ldCout));
    if (L.bn) { L.pre = alloc<float>(M * L.ldCout); L.stat = alloc<float>((size_t)BN_STAT_ROWS * L.ldCout); }
    maxC = std::max(maxC, L.ldCout);
  }
  // implicit-GEMM convolution (conv.hip) for every layer it covers: forward and data gradient never build a patch matrix
  rc_ft_fwd.assign(gconv.size(), nullptr); rc_ft_bwd.assign(gconv.size(), nullptr);
  rc_wgrad_implicit.assign(gconv.size(), 0);
  bool any_implicit = false;
  size_t wg_ws = 0;
  for (size_t l = 0; l < gconv.size() && sw.rced_implicit; ++l) {
    const ConvLayer& L = gconv[l];
    if (conv_fwd_supported(L.Cin, L.Cout, rcS, rcW, L.fw)) { rc_ft_fwd[l] = alloc<float>(conv_prep_floats(rcS, L.fw, L.Cin)); any_implicit = true; }
    if (l > 0 && conv_fwd_supported(L.Cout, L.Cin, rcS, rcW, L.fw)) rc_ft_bwd[l] = alloc<float>(conv_prep_floats(rcS, L.fw, L.Cout));
    if (conv_wgrad_supported(L.Cin, L.Cout, rcS, rcW, L.fw)) {
      rc_wgrad_implicit[l] = 1;
      wg_ws = std::max(wg_ws, conv_wgrad_ws_floats(L.Cin, (int)TB, rcS, rcW, L.fw));
    }
  }
  if (wg_ws) rc_wg_ws = alloc<float>(wg_ws);
  if (rc_ft_fwd[0] && rc_wgrad_implicit[0]) rc_x4 = alloc<float>(M * 4);
  else { rc_ft_fwd[0] = nullptr; rc_wgrad_implicit[0] = 0; }          // layer 0 is implicit only as a whole
  // patch matrices: kept per layer from the forward pass when they fit a 96 GB budget (288 GB HBM3E), else one shared
  // buffer that the backward pass refills
  size_t keep = 0;
  for (auto& L : gconv) keep += M * L.ldK;
  rc_keep_cols = !any_implicit && keep * sizeof(float) <= ((size_t)96 << 30) && !cfg.cross_validation;
  if (rc_keep_cols) {
    for (auto& L : gconv) { rc_cols.push_back(alloc_opt<float>(M * L.ldK)); if (!rc_cols.back()) rc_keep_cols = false; }
    if (!rc_keep_cols) rc_cols.clear();
  }
  // shared patch-matrix buffers only as wide as the layers that still take the patch-matrix path need them
  int colK = 4, dcolK = 4;
  for (size_t l = 0; l < gconv.size(); ++l) {
    if (!rc_ft_fwd[l] || !rc_wgrad_implicit[l]) colK = std::max(colK, gconv[l].ldK);
    if (l > 0 && !rc_ft_bwd[l]) dcolK = std::max(dcolK, gconv[l].ldK);
  }
  rc_col = rc_keep_cols ? rc_cols[0] : alloc<float>(M * colK);
  rc_dcol = alloc<float>(M * dcolK);
  rc_dA = alloc<float>(M * maxC); rc_dB = alloc<float>(M * maxC);
}

// ------------------------------------------------------------------------------------------ stage 6: the discriminator's buffers
int Model::alloc_discriminator() {
  const rsrgan_cfg& c = cfg;
  const bool inf = infer();
  const size_t TB = frame_rows(), TB2 = TB * 2;
  if (!inf) { xd = alloc<float>(TB2 * ldDout); logits = alloc<float>(TB2 * 4); dlogits = alloc<float>(TB2 * 4); }
  if (d_dnn() && !inf) {
    ldJ = pad4(c.d_joint_dim + Dout);
    if (c.d_joint_dim > 0) joint = alloc<float>(TB2 * ldJ);
    d_act.push_back(c.d_joint_dim > 0 ? joint : xd);
    for (size_t l = 0; l + 1 < dfc.size(); ++l) d_act.push_back(alloc<float>(TB2 * dfc[l].ld_out));
    d_act.push_back(logits);
    dy_buf = alloc<float>(TB * ldDout);
  }
  if ((g_dnn() || d_dnn()) && !inf) {
    int mx = std::max(ldJ, ldDin);
    for (auto& F : gfc) mx = std::max(mx, std::max(F.ld_in, F.ld_out));
    for (auto& F : dfc) mx = std::max(mx, std::max(F.ld_in, F.ld_out));
    fc_dA = alloc<float>(TB2 * mx); fc_dB = alloc<float>(TB2 * mx);
    if (bn_on()) {
      bn_sums = alloc<float>((size_t)2 * mx);
      for (auto& F : gfc) if (F.bn) { F.pre = alloc<float>(TB * F.ld_out); F.stat = alloc<float>((size_t)2 * BN_STAT_ROWS * F.ld_out); }
      for (auto& F : dfc) if (F.bn) { F.pre = alloc<float>(TB2 * F.ld_out); F.stat = alloc<float>((size_t)2 * BN_STAT_ROWS * F.ld_out); }
    }
  }
  adam_t_dev_d = alloc<int>(1);
  d_st.resize(dl.size());
  for (size_t l = 0; l < dl.size(); ++l) alloc_stash(*this, d_st[l], dl[l], 2 * B, Tmax);
  // folded views of the discriminator's cells (model.h): only for stacks of projected cells
  bool fold = sw.dfold && !dl.empty();
  for (auto& L : dl) fold = fold && L.has_proj && L.H <= 288 && (L.ldH & 3) == 0;
  if (fold) {
    dl_fold.resize(dl.size()); dl_fold_K.resize(dl.size()); d_fold_st.resize(dl.size());
    for (size_t l = 0; l < dl.size(); ++l) {
      LstmLayer F = dl[l];
      F.has_proj = false; F.tWp = -1;
      F.I = l == 0 ? dl[0].I : dl[l - 1].H; F.ldI = l == 0 ? dl[0].ldI : dl[l - 1].ldH;
      F.P = dl[l].H; F.ldP = dl[l].ldH;
      F.KxT = F.KhT = F.WpT = nullptr; F.WpT_sw = F.Wp_sw = F.Kb_full = F.Kb_rec = nullptr;
      const int ncb = (F.H + 15) / 16;
      F.Wg_full = alloc<float>(swizzle_floats(4 * ncb, (F.ldI + F.ldP + 15) / 16));
      F.Wg_h = alloc<float>(swizzle_floats(4 * ncb, (F.ldP + 15) / 16));
      dl_fold_K[l] = alloc<float>((size_t)(F.I + F.H) * 4 * F.H);
      dl_fold[l] = F;
      LstmStash S = d_st[l];
      S.mst = alloc<float>((size_t)(Tmax + 1) * 2 * B * F.ldP);
      S.out = nullptr; S.dmt = nullptr; S.dmst = nullptr;
      d_fold_st[l] = S;
    }
  }
  const int dmaxld = std::max(d_ldP(), ldDout);
  if (!inf) { d_dA = alloc<float>(TB2 * dmaxld); d_dB = alloc<float>(TB2 * dmaxld); }
  return alloc_status("discriminator buffers");
}

// ------------------------------------------------------------------------------------------ stage 7: what both nets share
// streams and events, device scalars, scratch and the GEMM work spaces
int Model::alloc_shared() {
  const rsrgan_cfg& c = cfg;
  const bool inf = infer();
  drop_ctr = (unsigned long long*)alloc<float>(4);
  len_dev = alloc<int>(2 * B);
  if (inf) len_win = alloc<int>(B);                         // a window's row lengths (infer_forward)
  zeros = alloc<float>(64);
  if (!inf) { noise_r_buf = alloc<float>((size_t)B * Dout); noise_f_buf = alloc<float>((size_t)B * Dout); }
  if (hipStreamCreateWithFlags(&main_s, hipStreamNonBlocking) != hipSuccess) main_s = nullptr;
  if (main_s && (hipEventCreateWithFlags(&ev_in, hipEventDisableTiming) != hipSuccess ||
                 hipEventCreateWithFlags(&ev_out, hipEventDisableTiming) != hipSuccess)) { (void)hipStreamDestroy(main_s); main_s = nullptr; }
  dyn = alloc<float>(DYN_COUNT); adam_t_dev = alloc<int>(1);
  losses = alloc<float>(8); tmp3 = alloc<float>(4);
  size_t maxcols = 7 * (size_t)std::max(c.g_cells, c.d_cells);
  maxcols = std::max(maxcols, (size_t)Din + 4);
  maxcols = std::max(maxcols, (size_t)std::max(g_ldP(), ldDin));
  scratch_floats = std::max<size_t>(4 * 64 * maxcols, 16384);            // (x 4: the column sums of up to four layers in one launch)
  if (!inf) {                                               // (column sums and loss partials; the per-step FC stage of the fused training launches)
    scratch = alloc<float>(scratch_floats);
    scratch2 = alloc<float>(std::max<size_t>(4 * 64 * maxcols, 1024));
    // (at least B floats: k_fwd_proj reads the stand-in of a stage's missing `len` -- one word per row, unused -- from WpT, which a narrow
    //  output under a large batch, Dout x ldP < B, would otherwise end before; rsrgan_op_lstm_step refuses that shape)
    g_fc_out_wT = g_dnn() ? nullptr : alloc<float>(std::max((size_t)Dout * g_ldP(), (size_t)B));
  }
  if (inf || hipStreamCreateWithFlags(&side, hipStreamNonBlocking) != hipSuccess) side = nullptr;
  if (hipEventCreateWithFlags(&ev_last, hipEventDisableTiming) != hipSuccess) ev_last = nullptr;
  if (side) {
    for (auto& e : ev_pool)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { side = nullptr; break; }
  }
  // the work spaces are optional: without one, the path that needs it is off
  gemm_ws_floats = (size_t)32 << 20;          // 128 MiB of split-K partial tiles / stream-K pieces (two 192 x 256 pieces per worker: 100 MB)
  gemm_ws = alloc_opt<float>(gemm_ws_floats);
  if (!gemm_ws) gemm_ws_floats = 0;
  bwdb_ws_floats = inf ? 0 : (size_t)8 << 20;
  if (!inf) {
    bwdb_ws = alloc_opt<float>(bwdb_ws_floats);             // (bwd_b_splitk_ok: the one-launch form of backward phase B)
    gemm_ws2 = alloc_opt<float>(gemm_ws_floats ? gemm_ws_floats : 1);
  }
  if (!inf && switches().dk_pad && !gl.empty() && gl[0].has_proj && gl[0].I % 4 != 0 && gl[0].ldI % 4 == 0 && gl.size() <= (size_t)GEMM_MAXB) {
    dk_tmp_per = (size_t)(gl[0].ldI + gl[0].P) * 4 * gl[0].H;
    dk_tmp = alloc_opt<float>(dk_tmp_per * gl.size());
    if (!dk_tmp) dk_tmp_per = 0;
  }
  if (!gemm_ws2) side = nullptr;                            // (the side stream's GEMMs need a work space of their own)
  if (int rc = alloc_status("shared work space")) return rc;
  HIPC(hipMemset(drop_ctr, 0, 16));
  return RSRGAN_OK;
}

// ------------------------------------------------------------------------------------------ stage 8: the persistent launches
// Residency probes, rings and control blocks of the persistent recurrences.  A ring that cannot be allocated switches its path off
// (alloc_opt); only the probed discriminator ring itself is required.
int Model::plan_persistent() {
  if (int rc = plan_dpersist()) return rc;
  if (int rc = plan_gpersist()) return rc;
  if (bnl_infer() && !gp_fwd_on()) {
    // the persistent forward is the only one this handle has (no launch-per-phase path knows the fold): no plan, no handle
    set_error("g_type bnlstm with RSRGAN_FLAG_INFER: no persistent forward plan for this configuration (batch_size=%d padded to %d rows, %d x %d / p%d; "
              "gpersist_plan's shapes, every workgroup of a row group resident at once, RSRGAN_GPERSIST / RSRGAN_PAD_ROWS not switched off), "
              "and a launch-per-phase forward of the folded cell is not built", Bt, B, cfg.g_layers, cfg.g_cells, cfg.g_proj);
    return RSRGAN_ERR_INVALID;
  }
  // the trailing discriminator BPTT beside k_glstm_bwd (the G-run): both launches' workgroups resident at once -- ask the device
  GPersistArgs ga{};
  if (sw.trail && dp_gran && (dp_live & 2) && gp_gran1 && gp_gran3 && !gp_noproj && (gp_live & 2) && B % 32 == 0 && gpersist_args(ga, gp_Tcap))
    trail_fits = resident_probe(gpersist_grid(ga) + ((dpersist_trail_grid((int)dl.size(), B) + 7) & ~7), GP_THREADS,
                                std::max(gpersist_lds_bytes(), dpersist_trail_lds_bytes()));
  lazy_sw = switches().lazy_swizzle && wavefront() && gp_gran1 && gp_gran3 && (gp_live & 3) == 3 && dp_gran && (dp_live & 3) == 3;
  // RSRGAN_DPIPE: the ring, control block and events of the D(real) launch on the side stream
  if (sw.dpipe > 0 && trail_fits && side && !d_dnn() && dp_max_grid >= dpersist_grid((int)dl.size(), B)) {
    const size_t gb = dpersist_granule_bytes((int)dl.size(), B, Tmax) / 2;      // (a forward launch: one edge per layer)
    dp_gran2 = (unsigned long long*)alloc_opt<float>(gb / sizeof(float));
    dp_ctl2 = (unsigned*)alloc_opt<float>(16);
    if (dp_gran2 && dp_ctl2 && hipEventCreateWithFlags(&ev_dfree, hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&ev_real, hipEventDisableTiming) == hipSuccess) {
      HIPC(ctl_reset(dp_ctl2));
      dpipe = true;
    }
  }
  return RSRGAN_OK;
}

int Model::plan_dpersist() {
  if (dp_live && !dl.empty() && dl.size() <= (size_t)DP_MAXL && B % 16 == 0) {
    // every workgroup of a launch waits for the others: ask the device whether the stacked (2B rows) or at least the single (B rows)
    // launch is resident at once -- a CU mask, a partition or a neighbour can take CUs away without multiProcessorCount knowing
    const int nl_ = (int)dl.size();
    for (int rows : {2 * B, B}) {
      const int g_ = dpersist_grid(nl_, rows);
      if (g_ <= 128 && resident_probe(g_, 512, dpersist_lds_bytes())) { dp_max_grid = g_; break; }
    }
  }
  if (dp_max_grid <= 0) return RSRGAN_OK;
  dp_gran_bytes = dpersist_granule_bytes((int)dl.size(), 2 * B, Tmax);
  dp_gran = (unsigned long long*)alloc<float>(dp_gran_bytes / sizeof(float));
  dp_ctl = (unsigned*)alloc<float>(16);
  if (int rc = alloc_status("persistent discriminator rings")) return rc;
  HIPC(ctl_reset(dp_ctl));
  // the weight gradients inside the D-run's BPTT launch (the stacked call over 2B rows): shapes only here, pointers per call
  DPersistArgs pa{};
  pa.nl = (int)dl.size(); pa.N = 2 * B; pa.H = dl[0].H;
  for (size_t l = 0; l < dl.size(); ++l) { pa.L[l].I = dl[l].I; pa.L[l].P = dl[l].P; pa.L[l].ldP = dl[l].ldP; pa.L[l].ldI = dl[l].ldI; }
  bool shapes = switches().dw_inkernel && (dp_live & 2) && dpersist_dw_supported(pa) && !d_adam();
  for (auto& L : dl) shapes = shapes && L.has_proj && L.H == dl[0].H && L.ldH == dl[0].ldH;
  if (shapes && dpersist_grid(pa.nl, pa.N) == dp_max_grid) {
    const int nt = pa.N / 16;
    dw_stride = dpersist_dw_stride(pa);
    dw_ws = alloc_opt<float>((size_t)pa.nl * nt * dw_stride);
    dw_flag = (unsigned*)alloc_opt<float>(dpersist_dw_flag_bytes(pa.nl, pa.N, Tmax) / sizeof(float));
    std::vector<long long> src(D.t.size(), -1);
    const int IP = dl[0].I + dl[0].P, H4 = 4 * dl[0].H, H_ = dl[0].H;
    for (size_t l = 0; l < dl.size(); ++l) {
      const long long base = (long long)l * nt * (long long)dw_stride;
      src[dl[l].tK] = base; src[dl[l].tb] = base + (long long)IP * H4;
      const long long pp = base + (long long)(IP + 1) * H4;
      src[dl[l].twi] = pp; src[dl[l].twf] = pp + H_; src[dl[l].two] = pp + 2 * H_; src[dl[l].tWp] = pp + 3 * H_;
    }
    dw_src = (long long*)alloc_opt<float>(src.size() * 2);
    if (dw_ws && dw_flag && dw_src) HIPC(hipMemcpy(dw_src, src.data(), src.size() * sizeof(long long), hipMemcpyHostToDevice));
    else dw_ws = nullptr;                                   // (the weight-gradient launches behind the BPTT)
  }
  return RSRGAN_OK;
}

int Model::plan_gpersist() {
  const bool inf = infer();
  if (!gp_live || g_dnn() || (g_bnl() && !inf)) return RSRGAN_OK;
  auto ring = [&](size_t bytes) { return (unsigned long long*)alloc_opt<float>(bytes / sizeof(float)); };
  GPersistArgs ga{};
  gp_Tcap = std::min(Tmax, (int)GP_TMAX);
  gp_noproj = !gl.empty() && !gl[0].has_proj;
  if (gp_noproj) {
    // 8 cells per workgroup (all weights in registers) needs twice the workgroups of 16: B = 64 with two layers is the whole
    // device -- ask it; if it cannot hold them, try the 16-cell form
    bool fits = false;
    for (int nt : {2, 4}) {
      gp_np_nt = nt;
      if (gpersist_shape(ga, gp_Tcap) && resident_probe(gpersist_grid(ga), GP_THREADS, gpersist_np_lds_bytes())) { fits = true; break; }
    }
    if (!fits) { gp_np_nt = 0; return RSRGAN_OK; }
    gp_gran2_bytes = gpersist_np_gran2_bytes(ga);
    gp_gran2 = ring(gp_gran2_bytes);
    gp_ctl = (unsigned*)alloc_opt<float>(16);
    // the BPTT form exists for 8 cells per workgroup only: its two rings (state gradient, input gradient between layers)
    if (gp_np_nt == 2 && (gp_live & 2) && switches().gp_np_bwd && !inf) {
      gp_gran1 = ring(gpersist_np_gran1_bytes(ga));
      gp_gran3 = ring(gpersist_np_gran3_bytes(ga));
      if (!gp_gran1 || !gp_gran3) { gp_gran1 = gp_gran3 = nullptr; }
    }
    if (!gp_gran1) gp_gran1 = gp_gran2;                       // (forward only: the pointer just says "the forward path is on")
    if (gp_gran2 && gp_ctl) {
      HIPC(ctl_reset(gp_ctl));
      gpersist_rearm();
    } else { gp_gran1 = gp_gran2 = gp_gran3 = nullptr; gp_ctl = nullptr; }
  } else if (gpersist_args(ga, gp_Tcap) && resident_probe(gpersist_grid(ga), GP_THREADS, gpersist_lds_bytes())) {
    gp_gran1 = ring(gpersist_gran1_bytes(ga));
    gp_gran2_bytes = gpersist_gran2_bytes(ga);
    gp_gran2 = ring(gp_gran2_bytes);
    gp_ctl = (unsigned*)alloc_opt<float>(16);
    // the BPTT launch's hand-offs time out when a layer's recurrent width is a single 16-column block (P <= 16: seen at H = 64 and
    // 128, the bounded waits expire and the step is poisoned): such a stack keeps the persistent forward, its BPTT takes the launch path
    bool bwd_ok = (gp_live & 2) != 0 && !inf;
    for (auto& L : gl) bwd_ok = bwd_ok && L.P > 16;
    if (bwd_ok) gp_gran3 = ring(gpersist_gran3_bytes(ga));
    if (gp_gran1 && gp_gran2 && gp_ctl) {
      HIPC(ctl_reset(gp_ctl));
      gpersist_rearm();
    } else { gp_gran1 = gp_gran2 = nullptr; gp_ctl = nullptr; }
  }
  return RSRGAN_OK;
}

// ------------------------------------------------------------------------------------------ stage 9: initial values
// xavier_initializer() uniform / zeros (models/lstm.py:86-87,93); the scalars; the weight copies; the gradient buckets
int Model::init_values(uint64_t seed) {
  const rsrgan_cfg& c = cfg;
  const bool inf = infer();
  std::mt19937_64 rng(seed);
  for (ParamSet* ps : {&G, &D}) {
    if (ps == &D && inf) continue;
    std::vector<float> host((size_t)ps->padded, 0.f);
    if (ps == &G && g_bnl()) bnl_init(host, seed);
    else for (auto& t : ps->t) {
      if (!t.l2 || t.const_init) {                           // biases: zero, except R-CED's output FC (rced.py:116: 0.1)
        if (t.bias_init != 0.f)
          for (int cc = 0; cc < t.cols; ++cc) host[(size_t)t.off + cc] = t.bias_init;
        continue;
      }
      const double fan_in = t.is_vector ? t.cols : t.rows, fan_out = t.xavier_fan_out > 0 ? t.xavier_fan_out : t.cols;
      const double lim = std::sqrt(6.0 / (fan_in + fan_out));
      std::uniform_real_distribution<double> u(-lim, lim);
      for (int r = 0; r < t.rows; ++r)
        for (int cc = 0; cc < t.cols; ++cc) host[(size_t)t.off + (size_t)r * t.ld + cc] = (float)u(rng);
    }
    HIPC(hipMemcpy(ps->w, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    if (ps->ema) HIPC(hipMemcpy(ps->ema, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  scal[RSRGAN_G_LEARNING_RATE] = 8e-5; scal[RSRGAN_D_LEARNING_RATE] = 1e-3; scal[RSRGAN_MSE_LAMBDA] = 10.0;
  scal[RSRGAN_D_REAL] = 1.0; scal[RSRGAN_D_FAKE] = 0.0; scal[RSRGAN_L2_SCALE] = c.l2_scale;
  scal[RSRGAN_CLIP_NORM] = c.clip_norm; scal[RSRGAN_ADAM_STEP] = 0;
  float hdyn[DYN_COUNT] = {0};
  hdyn[DYN_G_LR] = 8e-5f; hdyn[DYN_D_LR] = 1e-3f; hdyn[DYN_LAMBDA] = 10.f; hdyn[DYN_D_REAL] = 1.f; hdyn[DYN_D_FAKE] = 0.f;
  hdyn[DYN_L2] = c.l2_scale; hdyn[DYN_CLIP] = c.clip_norm; hdyn[DYN_B1] = c.adam_beta1; hdyn[DYN_B2] = c.adam_beta2;
  hdyn[DYN_EPS] = c.adam_eps; hdyn[DYN_EMA] = c.ema_decay;
  HIPC(hipMemcpy(dyn, hdyn, sizeof(hdyn), hipMemcpyHostToDevice));
  g_fc_in_unfolded = true;                         // (the initial values were just uploaded)
  refresh_transposes(RSRGAN_NET_G, nullptr);
  if (!inf) {
    refresh_transposes(RSRGAN_NET_D, nullptr);
    int rc = build_buckets(); if (rc) return rc;
  }
  HIPC(hipDeviceSynchronize());
  HIPC(hipGetLastError());
  return RSRGAN_OK;
}

void Model::destroy() {
  drop_graphs();
  if (main_s) {
    (void)hipStreamSynchronize(main_s);
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_out) (void)hipEventDestroy(ev_out);
    (void)hipStreamDestroy(main_s);
    main_s = nullptr;
  }
  if (side) {
    (void)hipStreamSynchronize(side);
    for (auto& e : ev_pool) if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(side);
    side = nullptr;
  }
  if (ev_last) { (void)hipEventDestroy(ev_last); ev_last = nullptr; ev_last_set = false; }
  if (ev_dfree) { (void)hipEventDestroy(ev_dfree); ev_dfree = nullptr; }
  if (ev_real) { (void)hipEventDestroy(ev_real); ev_real = nullptr; }
  dpipe = false;
  for (auto& v : gbk) { for (auto& b : v) if (b.ev) (void)hipEventDestroy(b.ev); v.clear(); }
  for (auto& e : prof_ev) if (e) (void)hipEventDestroy(e);
  prof_ev.clear();
  for (auto& e : prof_gp_ev) if (e) (void)hipEventDestroy(e);
  prof_gp_ev.clear();
  for (auto& e : prof_gb_ev) if (e) (void)hipEventDestroy(e);
  prof_gb_ev.clear();
  for (void* p : allocs) (void)hipFree(p);
  allocs.clear();
}

int Model::build_buckets() {
  auto range = [](const ParamSet& ps, int lo, int hi, GradBucket& b) {      // tensors lo..hi inclusive
    b.off = ps.t[lo].off;
    b.count = (hi + 1 < (int)ps.t.size() ? ps.t[hi + 1].off : ps.padded) - b.off;
  };
  auto whole = [](const ParamSet& ps, std::vector<GradBucket>& v) { GradBucket b; b.off = 0; b.count = ps.padded; v.assign(1, b); };
  whole(D, gbk[RSRGAN_NET_D]);
  whole(G, gbk[RSRGAN_NET_G]);
  if (!g_dnn() && wavefront()) {
    // completion order of the merged generator backward: output FC, input FC (g_type lstm), then the LSTM layers
    std::vector<GradBucket> v;
    bool ok = true;
    GradBucket b;
    range(G, g_fc_out_w, g_fc_out_b, b); ok = ok && g_fc_out_b == g_fc_out_w + 1; v.push_back(b);
    if (cfg.g_type == RSRGAN_G_LSTM) {
      const int hi = seq_bn() ? g_bn_t[7] : g_fc_in_b;                 // (batch norm: weights, then the eight BatchNorm variables)
      range(G, g_fc_in_w, hi, b); ok = ok && hi == g_fc_in_w + (seq_bn() ? 8 : 1); v.push_back(b);
    }
    for (auto& L : gl) {
      const int lo = L.tK, hi = L.has_proj ? L.tWp : L.two;
      ok = ok && L.tb > lo && L.tb < hi && L.twf > lo && L.twi > lo && L.two <= hi && hi - lo == (L.has_proj ? 5 : 4);
      range(G, lo, hi, b); v.push_back(b);
    }
    int64_t covered = 0;
    for (auto& x : v) covered += x.count;
    if (ok && covered == G.padded) gbk[RSRGAN_NET_G] = v;      // else: keep the single whole-buffer bucket
  }
  for (auto& v : gbk)
    for (auto& b : v)
      if (hipEventCreateWithFlags(&b.ev, hipEventDisableTiming) != hipSuccess) { set_error("hipEventCreate failed"); return RSRGAN_ERR_HIP; }
  return RSRGAN_OK;
}

}  // namespace rsr
