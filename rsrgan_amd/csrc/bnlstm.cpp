// bnlstm.cpp -- the recurrent batch-norm LSTMP generator of models/bnlstm.py:38-127 on the supervised trainer path
// (models/rnn_trainer.py:66-205): variable table and initial values, buffers, and the launch schedule of a step.
//
// Schedule (layer-major): input FC + ReLU as one time-batched GEMM; per layer the x-part x.W_xh for all T*B rows as one GEMM and
// BN_input for all steps (k_bnl_bn_in), then two launches per step (k_bnl_cell_fwd: m_{t-1}.W_hh, BN_state, gates, c, BN_cell, h;
// k_bnl_proj: m = h.W_proj with dynamic_rnn's masking), then the moving statistics (k_bnl_ema, training runs only); output FC.
// The BPTT mirrors it: two launches per step (k_bnl_cell_bwd, k_bnl_dm), BN_input's backward for all steps, then the data and
// weight gradients as GEMMs over the T*B rows and the vector gradients as column sums.  See DESIGN.md "bnlstm".
#include <cmath>
#include <random>

#include "model.h"

namespace rsr {

namespace {
constexpr float kBnlEps = 1e-3f, kBnlDecay = 0.999f;      // BNLSTMCell.py:20 batch_norm(epsilon=1e-3, decay=0.999)
}

int Model::bnl_check(const rsrgan_cfg& c) const {
  if (!(c.flags & RSRGAN_FLAG_SUPERVISED)) {
    set_error("g_type bnlstm is built for the supervised trainer only (RSRGAN_FLAG_SUPERVISED; the reference GAN has no bnlstm generator)");
    return RSRGAN_ERR_INVALID;
  }
  if (c.flags & RSRGAN_FLAG_BATCH_NORM) { set_error("g_type bnlstm: the input FC's batch_norm (RSRGAN_FLAG_BATCH_NORM) is not built"); return RSRGAN_ERR_INVALID; }
  if (c.flags & RSRGAN_FLAG_INFER) {
    // decode normalises with the moving statistics, so rows do not interact (no 64-row limit: the batch is padded to the
    // persistent launch's row groups) -- and the persistent launch is the only forward such a handle has
    if (!(c.flags & RSRGAN_FLAG_WAVEFRONT)) {
      set_error("g_type bnlstm with RSRGAN_FLAG_INFER needs RSRGAN_FLAG_WAVEFRONT: its forward is the persistent launch, a launch-per-phase forward of the folded cell is not built");
      return RSRGAN_ERR_INVALID;
    }
    if (!switches().gp_tags) {
      set_error("g_type bnlstm with RSRGAN_FLAG_INFER: RSRGAN_GP_TAGS=0 is set, and the folded cell's persistent forward is built for tagged rings only");
      return RSRGAN_ERR_INVALID;
    }
  } else if (!bnl_supported(c.batch_size)) {
    set_error("g_type bnlstm: batch_size=%d, at most 64 rows per GPU are supported (one workgroup holds a step's batch statistics)", c.batch_size);
    return RSRGAN_ERR_INVALID;
  }
  if (c.g_proj <= 0) { set_error("g_type bnlstm needs num_proj (g_proj > 0)"); return RSRGAN_ERR_INVALID; }
  return RSRGAN_OK;
}

// g_model/fully_connected, g_model/rnn/multi_rnn_cell/cell_<l>/bnlstm_cell/* in BNLSTMCell.call's creation order, g_model/fully_connected_1
void Model::bnl_params() {
  const int P = cfg.g_proj, H = cfg.g_cells;
  g_fc_in_w = G.add("g_model/fully_connected/weights", Din, P, false);
  g_fc_in_b = G.add("g_model/fully_connected/biases", 1, P, true);
  static const char* kBn[4] = {"scale", "offset", "moving_mean", "moving_var"};
  for (int l = 0; l < cfg.g_layers; ++l) {
    const std::string pre = "g_model/rnn/multi_rnn_cell/cell_" + std::to_string(l) + "/bnlstm_cell/";
    BnlCell C;
    C.tWx = G.add(pre + "input_kernel", P, 4 * H, false);
    C.tWh = G.add(pre + "state_kernel", P, 4 * H, false);
    auto site = [&](const char* nm, int n, int (&idx)[4]) {
      for (int k = 0; k < 4; ++k) {
        idx[k] = G.add(pre + nm + "/" + kBn[k], 1, n, true);
        if (k >= 2) { G.t[idx[k]].trainable = false; G.t[idx[k]].l2 = false; }     // moving statistics: no gradient, no L2
      }
    };
    site("input", 4 * H, C.tin);
    site("state", 4 * H, C.tst);
    C.tb = G.add(pre + "bias", 1, 4 * H, true);
    C.twf = G.add(pre + "W_F_diag", 1, H, true);
    C.twi = G.add(pre + "W_I_diag", 1, H, true);
    C.two = G.add(pre + "W_O_diag", 1, H, true);
    site("cell", H, C.tce);
    C.tWp = G.add(pre + "projection/kernel", H, P, false);
    bnl.push_back(C);
  }
  g_fc_out_w = G.add("g_model/fully_connected_1/weights", P, Dout, false);
  g_fc_out_b = G.add("g_model/fully_connected_1/biases", 1, Dout, true);
}

// An inference handle's layers (RSRGAN_FLAG_INFER): one LstmLayer view per BNLSTMCell for the persistent forward -- input and
// recurrent width P, the cell's own bias / peephole / projection tensors, no stacked kernel (tK = -1: input_kernel and state_kernel stay two
// tensors; KxT / KhT receive their folded, transposed copies from bnl_refresh_fold)
void Model::bnl_infer_layers() {
  for (const BnlCell& C : bnl) {
    LstmLayer L;
    L.has_proj = true;
    L.I = L.P = cfg.g_proj; L.H = cfg.g_cells; L.ldI = L.ldP = pad4(L.P); L.ldH = pad4(L.H);
    L.tK = -1; L.tb = C.tb; L.twf = C.twf; L.twi = C.twi; L.two = C.two; L.tWp = C.tWp;
    gl.push_back(L);
  }
}

void Model::bnl_refresh_fold(hipStream_t s) {
  for (size_t l = 0; l < bnl.size(); ++l) {
    const BnlCell& C = bnl[l]; const LstmLayer& L = gl[l];
    BnlFold f{};
    f.Wx = G.W(C.tWx); f.Wh = G.W(C.tWh); f.bias = G.W(C.tb);
    for (int k = 0; k < 4; ++k) { f.bn[k] = G.W(C.tin[k]); f.bn[4 + k] = G.W(C.tst[k]); f.bn[8 + k] = G.W(C.tce[k]); }
    f.P = L.P; f.H = L.H; f.ldI = L.ldI; f.ldP = L.ldP; f.eps = kBnlEps;
    f.KxT = L.KxT; f.KhT = L.KhT; f.bias_f = L.bias_f; f.ca = L.ca; f.cb = L.cb;
    launch_bnl_fold(f, s);
  }
}

// (all required: alloc_generator tests the handle's allocation status behind this)
void Model::bnl_alloc() {
  const size_t TB = (size_t)Tmax * B, TB1 = (size_t)(Tmax + 1) * B;
  const int H = cfg.g_cells, H4 = 4 * H, ldP = pad4(cfg.g_proj), ldH = pad4(H);
  g_h0 = alloc<float>(TB * ldP);
  for (BnlCell& C : bnl) {
    C.zx = alloc<float>(TB * H4); C.xh_in = alloc<float>(TB * H4); C.yin = alloc<float>(TB * H4);
    C.xh_s = alloc<float>(TB * H4); C.act = alloc<float>(TB * H4); C.dz = alloc<float>(TB * H4);
    C.cnew = alloc<float>(TB * ldH); C.chat = alloc<float>(TB * ldH); C.h = alloc<float>(TB * ldH); C.dyc = alloc<float>(TB * ldH);
    C.ccar = alloc<float>(TB1 * ldH); C.mst = alloc<float>(TB1 * ldP);     // ([0] = the zero initial state: never written)
    C.out = alloc<float>(TB * ldP); C.dmn = alloc<float>(TB * ldP);
    C.mu = alloc<float>((size_t)Tmax * 9 * H); C.var = alloc<float>((size_t)Tmax * 9 * H);
    C.dcc = alloc<float>((size_t)B * ldH); C.dmc = alloc<float>((size_t)B * ldP);
  }
}

// initial values (bnlstm.py:47-52,103-123, BNLSTMCell.py:20-47,176-215): input FC truncated_normal(0, sqrt(2 / num_proj)) redrawn
// outside 2 sigma, zero biases; input / state kernels and the output FC xavier; bias, diagonals and projection/kernel without an
// initializer = glorot_uniform (1-D: U(+-sqrt(3 / n))); scale 0.1, offset 0, moving_mean 0, moving_var 1
void Model::bnl_init(std::vector<float>& host, uint64_t seed) const {
  std::mt19937_64 rng(seed ^ 0xb417e5ull);
  auto fill = [&](int ti, const std::function<double()>& f) {
    const TensorDesc& t = G.t[ti];
    for (int r = 0; r < t.rows; ++r)
      for (int c = 0; c < t.cols; ++c) host[(size_t)t.off + (size_t)r * t.ld + c] = (float)f();
  };
  auto uni = [&](int ti, double lim) { std::uniform_real_distribution<double> u(-lim, lim); fill(ti, [&] { return u(rng); }); };
  auto glorot = [&](int ti) {
    const TensorDesc& t = G.t[ti];
    const double fi = t.is_vector ? t.cols : t.rows, fo = t.cols;
    uni(ti, std::sqrt(6.0 / (fi + fo)));
  };
  auto constant = [&](int ti, float v) { fill(ti, [&] { return (double)v; }); };
  {
    const double sd = std::sqrt(2.0 / cfg.g_proj);
    std::normal_distribution<double> n(0.0, sd);
    fill(g_fc_in_w, [&] { double v; do { v = n(rng); } while (std::fabs(v) > 2.0 * sd); return v; });
    constant(g_fc_in_b, 0.f);
  }
  for (const BnlCell& C : bnl) {
    glorot(C.tWx); glorot(C.tWh);
    for (const int* s : {C.tin, C.tst, C.tce}) { constant(s[0], 0.1f); constant(s[1], 0.f); constant(s[2], 0.f); constant(s[3], 1.f); }
    glorot(C.tb); glorot(C.twf); glorot(C.twi); glorot(C.two); glorot(C.tWp);
  }
  glorot(g_fc_out_w);
  constant(g_fc_out_b, 0.f);
}

BnlLayer Model::bnl_args(int l, bool train) const {
  const BnlCell& C = bnl[l];
  float* w = G.w;
  auto W = [&](int ti) { return w + G.t[ti].off; };
  BnlLayer a{};
  a.B = B; a.H = cfg.g_cells; a.P = cfg.g_proj; a.ldP = pad4(a.P); a.ldH = pad4(a.H); a.nst = 9 * a.H;
  a.train = train ? 1 : 0; a.eps = kBnlEps; a.fb = cfg.forget_bias;
  a.len = len_dev;
  a.Whh = W(C.tWh); a.Wp = W(C.tWp); a.bias = W(C.tb); a.wf = W(C.twf); a.wi = W(C.twi); a.wo = W(C.two);
  a.sc_in = W(C.tin[0]); a.of_in = W(C.tin[1]); a.mm_in = W(C.tin[2]); a.mv_in = W(C.tin[3]);
  a.sc_s = W(C.tst[0]); a.of_s = W(C.tst[1]); a.mm_s = W(C.tst[2]); a.mv_s = W(C.tst[3]);
  a.sc_c = W(C.tce[0]); a.of_c = W(C.tce[1]); a.mm_c = W(C.tce[2]); a.mv_c = W(C.tce[3]);
  a.xh_in = C.xh_in; a.yin = C.yin; a.xh_s = C.xh_s; a.act = C.act; a.cnew = C.cnew; a.chat = C.chat; a.ccar = C.ccar; a.h = C.h;
  a.mst = C.mst; a.out = C.out; a.mu = C.mu; a.var = C.var;
  a.dz = C.dz; a.dhh = C.yin; a.dyc = C.dyc; a.dmn = C.dmn; a.dcc = C.dcc; a.dmc = C.dmc;      // (d(hh) reuses BN_input's output)
  return a;
}

void Model::bnl_forward(int T, bool train, hipStream_t s) {
  const int P = cfg.g_proj, ldP = pad4(P), H4 = 4 * cfg.g_cells, R = T * B;
  // h = relu(x.W + b) (bnlstm.py:103-108; act 1 with alpha 0)
  gemm(x_tm, ldDin, true, G.W(g_fc_in_w), ldP, false, g_h0, ldP, R, P, Din, G.W(g_fc_in_b), 1, 0.f, false, s);
  for (size_t l = 0; l < bnl.size(); ++l) {
    const BnlCell& C = bnl[l];
    const BnlLayer a = bnl_args((int)l, train);
    const float* xin = l == 0 ? g_h0 : bnl[l - 1].out;
    gemm(xin, ldP, true, G.W(C.tWx), H4, false, C.zx, H4, R, H4, P, nullptr, 0, 0.f, false, s);
    launch_bnl_bn_in(a, C.zx, T, s);
    for (int t = 0; t < T; ++t) {
      launch_bnl_cell_fwd(a, t, s);
      launch_bnl_proj(a, t, s);
    }
    if (train) launch_bnl_ema(a, T, kBnlDecay, s);
  }
  // y = outputs.W + b (bnlstm.py:120-123)
  gemm(bnl.back().out, ldP, true, G.W(g_fc_out_w), ldDout, false, y_tm, ldDout, R, Dout, P, G.W(g_fc_out_b), 0, 0.f, false, s);
}

void Model::bnl_backward(int T, float* dy, hipStream_t s) {
  const int P = cfg.g_proj, ldP = pad4(P), H = cfg.g_cells, H4 = 4 * H, ldH = pad4(H), R = T * B;
  // output FC: dW = out^T dy, db = colsum(dy), d(out) = dy W^T
  gemm(bnl.back().out, ldP, false, dy, ldDout, false, G.Gd(g_fc_out_w), ldDout, P, Dout, R, nullptr, 0, 0.f, false, s);
  launch_colsum(dy, ldDout, nullptr, 0, G.Gd(g_fc_out_b), R, Dout, scratch, s);
  float* cur = g_dA;
  float* other = g_dB;
  gemm(dy, ldDout, true, G.W(g_fc_out_w), ldDout, true, cur, ldP, R, P, Dout, nullptr, 0, 0.f, false, s);
  for (int l = (int)bnl.size() - 1; l >= 0; --l) {
    const BnlCell& C = bnl[l];
    BnlLayer a = bnl_args(l, true);
    a.dout = cur;
    (void)hipMemsetAsync(C.dcc, 0, (size_t)B * ldH * sizeof(float), s);
    (void)hipMemsetAsync(C.dmc, 0, (size_t)B * ldP * sizeof(float), s);
    for (int t = T - 1; t >= 0; --t) {
      launch_bnl_cell_bwd(a, t, s);
      launch_bnl_dm(a, t, s);
    }
    launch_bnl_bn_in_bwd(a, C.zx, T, s);                 // d(x.W_xh) -> zx
    const float* xin = l == 0 ? g_h0 : bnl[l - 1].out;
    gemm(C.zx, H4, true, G.W(C.tWx), H4, true, other, ldP, R, P, H4, nullptr, 0, 0.f, false, s);           // d(input)
    gemm(xin, ldP, false, C.zx, H4, false, G.Gd(C.tWx), H4, P, H4, R, nullptr, 0, 0.f, false, s);          // input_kernel
    gemm(C.mst, ldP, false, C.yin, H4, false, G.Gd(C.tWh), H4, P, H4, R, nullptr, 0, 0.f, false, s);       // state_kernel: m_{t-1}^T d(hh)
    gemm(C.h, ldH, false, C.dmn, ldP, false, G.Gd(C.tWp), ldP, H, P, R, nullptr, 0, 0.f, false, s);        // projection/kernel
    launch_colsum(C.dz, H4, nullptr, 0, G.Gd(C.tb), R, H4, scratch, s);                                    // bias
    launch_colsum(C.dz, H4, nullptr, 0, G.Gd(C.tst[1]), R, H4, scratch, s);                                // state/offset
    launch_colsum(C.dz, H4, C.xh_s, H4, G.Gd(C.tst[0]), R, H4, scratch, s);                                // state/scale
    launch_colsum(C.dz, H4, nullptr, 0, G.Gd(C.tin[1]), R, H4, scratch, s);                                // input/offset
    launch_colsum(C.dz, H4, C.xh_in, H4, G.Gd(C.tin[0]), R, H4, scratch, s);                               // input/scale
    launch_colsum(C.dyc, ldH, nullptr, 0, G.Gd(C.tce[1]), R, H, scratch, s);                               // cell/offset
    launch_colsum(C.dyc, ldH, C.chat, ldH, G.Gd(C.tce[0]), R, H, scratch, s);                              // cell/scale
    launch_colsum(C.dz, H4, C.ccar, ldH, G.Gd(C.twi), R, H, scratch, s);                                   // W_I_diag: d(i) c_prev
    launch_colsum(C.dz + 2 * H, H4, C.ccar, ldH, G.Gd(C.twf), R, H, scratch, s);                           // W_F_diag: d(f) c_prev
    launch_colsum(C.dz + 3 * H, H4, C.cnew, ldH, G.Gd(C.two), R, H, scratch, s);                           // W_O_diag: d(o) c
    std::swap(cur, other);
  }
  // through the ReLU and the input FC
  launch_lrelu_bwd(g_h0, cur, (size_t)R, P, ldP, 0.f, s);
  gemm(x_tm, ldDin, false, cur, ldP, false, G.Gd(g_fc_in_w), ldP, Din, P, R, nullptr, 0, 0.f, false, s);
  launch_colsum(cur, ldP, nullptr, 0, G.Gd(g_fc_in_b), R, P, scratch, s);
}

}  // namespace rsr
