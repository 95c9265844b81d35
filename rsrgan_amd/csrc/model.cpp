// model.cpp -- the recurrences of the GAN step and what they need: weight-copy refreshes, the launch-per-phase and wavefront drivers
// (rnn_forward / rnn_backward), the persistent launches, the weight gradients.  The step's drivers (the D-run, the G-run, the updates):
// model_step.cpp.  Tables, buffers and everything else a handle is built from: model_init.cpp.
// Reference graph: models/gan_rnn_placeholder.py:139-298 (build_model / build_model_single_gpu),
// generator models/lstm.py:41-129 | models/res_lstm_l.py:41-199, discriminator
// models/discriminator_lstm.py:24-110.
#include "model.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace rsr {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* get_error() { return g_err; }

void Model::refresh_transposes(int net, hipStream_t s) {
  const ParamSet& ps = net == RSRGAN_NET_G ? G : D;
  auto& layers = net == RSRGAN_NET_G ? gl : dl;
  TransposeList tl{};
  auto add = [&](const float* src, int lds_, float* dst, int ldd, int R, int C) {
    if (tl.n == 16) { launch_transpose_many(tl, s); tl.n = 0; }
    tl.j[tl.n++] = TransposeJob{src, dst, lds_, ldd, R, C, 0};
  };
  if (net == RSRGAN_NET_G && bnl_infer()) { bnl_refresh_fold(s); return; }      // (its forward copies are the folded ones, nothing else)
  if (net == RSRGAN_NET_G && seq_bn_infer()) seq_bn_fold(s);                     // (folds only behind a writer of the variables: g_fc_in_unfolded)
  for (auto& L : layers) {
    const float* K = ps.W(L.tK);
    const int H4 = 4 * L.H;
    add(K, H4, L.KxT, L.ldI, L.I, H4);                       // [I][4H] -> [4H][ldI]
    add(K + (size_t)L.I * H4, H4, L.KhT, L.ldP, L.P, H4);    // [P][4H] -> [4H][ldP]
    if (L.has_proj) add(ps.W(L.tWp), L.ldP, L.WpT, L.ldH, L.H, L.P);         // [H][ldP] -> [P][ldH]
  }
  if (net == RSRGAN_NET_G && g_fc_out_wT && g_fc_out_w >= 0)
    add(G.W(g_fc_out_w), ldDout, g_fc_out_wT, pad4(gR), gR, Dout);   // [P][ldDout] -> [Dout][ldP]
  launch_transpose_many(tl, s);
  if (!lazy_sw) refresh_swizzles(net, s);
  // (the folded discriminator kernels are derived where they are used, fold_forward: with the persistent discriminator launch on,
  //  that is never -- three GEMMs, a copy and a swizzle launch, 60 us per step, used to follow every discriminator update)
  if (net == RSRGAN_NET_G)
    for (size_t l = 0; l < gconv.size(); ++l) {                       // R-CED: re-arranged filters of the implicit-GEMM conv
      const ConvLayer& L = gconv[l];
      if (rc_ft_fwd[l]) launch_conv_prep(G.W(L.tW), L.ldCout, rcS, L.fw, L.Cin, L.Cout, false, rc_ft_fwd[l], s);
      if (rc_ft_bwd[l]) launch_conv_prep(G.W(L.tW), L.ldCout, rcS, L.fw, L.Cin, L.Cout, true, rc_ft_bwd[l], s);
    }
}

// The fragment-tiled weight copies of the launch-per-phase recurrence kernels (k_fwd_gates, k_fwd_proj, k_bwd_a2, k_bwd_bp).  With
// both generator and discriminator recurrences on their persistent launches (lazy_sw) nothing reads them in a training step: they are
// then rebuilt at the top of rnn_forward / rnn_backward -- the only readers -- instead of after every optimizer step (46 us for the
// generator's 23 MB, 11 us for the discriminator).
void Model::refresh_swizzles(int net, hipStream_t s) {
  if (net == RSRGAN_NET_G && bnl_infer()) return;          // (no launch-per-phase path, none of its copies)
  const ParamSet& ps = net == RSRGAN_NET_G ? G : D;
  auto& layers = net == RSRGAN_NET_G ? gl : dl;
  {
    SwizzleList sl{};
    auto addz = [&](const SwizzleJob& j) {
      if (!j.dst) return;
      if (sl.n == 24) { launch_swizzle_many(sl, s); sl.n = 0; }
      sl.j[sl.n++] = j;
    };
    for (auto& L : layers) {
      const float* K = ps.W(L.tK);
      const int H4 = 4 * L.H, ncb = (L.H + 15) / 16, kbI = (L.ldI + L.ldP + 15) / 16, kbP = (L.ldP + 15) / 16, kbH = (L.ldH + 15) / 16, kb4 = (H4 + 15) / 16;
      //            src  dst        ld     gates H    C          c0   K1  I    P    kx     nct                 nkb
      addz(SwizzleJob{K, L.Wg_full, H4,    4,    L.H, 0,         0,   0,  L.I, L.P, L.ldI, 4 * ncb,            kbI, 0});
      addz(SwizzleJob{K, L.Wg_h,    H4,    4,    L.H, 0,         0,   0,  L.I, L.P, 0,     4 * ncb,            kbP, 0});
      addz(SwizzleJob{K, L.Kb_full, H4,    0,    0,   L.I + L.P, 0,   H4, 0,   0,   0,     (L.I + L.P + 15) / 16, kb4, 0});
      addz(SwizzleJob{K, L.Kb_rec,  H4,    0,    0,   L.P,       L.I, H4, 0,   0,   0,     (L.P + 15) / 16,    kb4, 0});
      if (L.has_proj) {
        const float* Wp = ps.W(L.tWp);                   // [H][ldP]
        addz(SwizzleJob{Wp, L.WpT_sw, L.ldP, 1,  L.P, 0,         0,   0,  L.H, 0,   16 * kbH, (L.P + 15) / 16, kbH, 0});     // M[p][k] = Wp[k][p]
        addz(SwizzleJob{Wp, L.Wp_sw,  L.ldP, 0,  0,   L.H,       0,   L.P, 0,  0,   0,     ncb,                kbP, 0});     // M[cell][k] = Wp[cell][k]
      }
    }
    launch_swizzle_many(sl, s);
  }
}

// ------------------------------------------------------------------------------------------
// stacks of dynamic_rnn(LSTMCell) layers.  Two schedules over the same kernels:
//   layer-sequential: per layer one time-batched GEMM for the x-part, then 2 launches per step;
//   wavefront (RSRGAN_FLAG_WAVEFRONT): launch d carries every (layer l, t = d - l) job of every
//   co-scheduled chain, so a 3-layer stack over T steps costs 2*(T+2) launches instead of 6*T.
// ------------------------------------------------------------------------------------------
static inline int kb16(int ld) { return (ld + 15) >> 4; }

bool Model::bwd_b_splitk_ok(const BwdBJobs& jobs) const {
  if (!bwdb_ws || (cfg.flags & RSRGAN_FLAG_NO_SPLITK_B)) return false;
  BwdBJobs tmp = jobs;
  const size_t need = bwd_b_plan(tmp, nullptr);
  if (need > bwdb_ws_floats) return false;
  int blocks = 0;
  for (int i = 0; i < tmp.n; ++i) {
    if ((tmp.j[i].kpg + 1) / 2 > 12) return false;       // k_bwd_bp holds <= 12 k-blocks of weights per wave
    blocks += tmp.j[i].KG * tmp.j[i].ncg * tmp.j[i].nrg;
  }
  return blocks >= 96;          // small launches (the discriminator alone): one 32x16-tile launch is faster (9.3 vs 10.4 us)
}

void Model::gemm(const float* A, int lda, bool a_kc, const float* B_, int ldb, bool b_kc, float* C, int ldc, int M, int N,
                 int K, const float* bias, int act, float alpha, bool accumulate, hipStream_t s) {
  launch_gemm(A, lda, a_kc, B_, ldb, b_kc, C, ldc, M, N, K, bias, act, alpha, accumulate, s,
              (side && s == side) ? gemm_ws2 : gemm_ws, gemm_ws_floats);
}

static void fill_gate(FwdGateJob& a, const LayerRun& R, int t, bool zx) {
  const LstmLayer& L = *R.L; const LstmStash& S = *R.S; const ParamSet& ps = *R.ps;
  const int H = L.H, H4 = 4 * H;
  const size_t r = (size_t)t * R.Ns + R.row0, rn = (size_t)(t + 1) * R.Ns + R.row0;
  a.x = zx ? nullptr : R.in + r * L.ldI;
  a.KxT = L.KxT; a.ldx = L.ldI; a.Wsw = zx ? L.Wg_h : L.Wg_full;
  a.m = S.mst + r * L.ldP; a.KhT = L.KhT; a.ldm = L.ldP;
  a.zx = zx ? S.gates + r * H4 : nullptr; a.bias = ps.W(L.tb);
  a.wf = ps.W(L.twf); a.wi = ps.W(L.twi); a.wo = ps.W(L.two);
  a.c_prev = S.c + r * H; a.c_out = S.c + rn * H;
  a.gates = S.gates + r * H4;
  a.h = S.h + r * L.ldH; a.ldh = L.ldH;
  a.len = R.len; a.t = t; a.N = R.N; a.H = H;
  a.nblk_c = (H + 15) / 16;
  if (L.has_proj) { a.np_m_out = nullptr; a.np_out = nullptr; a.np_res_in = nullptr; a.np_res_out = nullptr; }
  else {     // num_proj=None: m = h; the gates epilogue also does the dynamic_rnn masking and the residual add
    a.np_m_out = S.mst + rn * L.ldP; a.np_out = S.out ? S.out + r * L.ldP : nullptr;
    a.np_res_in = R.res_in ? R.res_in + r * L.ldP : nullptr;
    a.np_res_out = R.res_out ? R.res_out + r * L.ldP : nullptr;
  }
}
static void fill_proj(FwdProjJob& p, const LayerRun& R, int t) {
  const LstmLayer& L = *R.L; const LstmStash& S = *R.S;
  const size_t r = (size_t)t * R.Ns + R.row0, rn = (size_t)(t + 1) * R.Ns + R.row0;
  p.h = S.h + r * L.ldH; p.WpT = L.WpT; p.WpT_sw = L.WpT_sw; p.ldh = L.ldH;
  p.m_prev = S.mst + r * L.ldP; p.m_out = S.mst + rn * L.ldP; p.out = S.out + r * L.ldP;
  p.res_in = R.res_in ? R.res_in + r * L.ldP : nullptr;
  p.res_out = R.res_out ? R.res_out + r * L.ldP : nullptr;
  p.len = R.len; p.bias = nullptr; p.noise = nullptr;
  p.ldm = L.ldP; p.ldo = L.ldP; p.P = L.P; p.t = t; p.N = R.N;
  p.nblk_c = (L.P + 15) / 16;
  p.drop = R.drop; p.drop.tag += (unsigned long long)t;
}
static void fill_fc_fwd(FwdProjJob& p, const FcStage& F, int t) {
  p.h = F.in + (size_t)t * F.N * F.ld_in; p.WpT = F.WT; p.WpT_sw = nullptr; p.ldh = F.ld_in;
  p.m_prev = nullptr; p.m_out = F.y + (size_t)t * F.N * F.ldy; p.ldm = F.ldy;
  p.out = F.out2 + ((size_t)t * F.Ns2 + F.row02) * F.ld2; p.ldo = F.ld2;
  p.res_in = nullptr; p.res_out = nullptr; p.len = nullptr; p.bias = F.bias; p.noise = F.noise;
  p.P = F.D; p.t = t; p.N = F.N;
  p.nblk_c = (F.D + 15) / 16;
  p.drop = DropSpec{};
}
static void fill_fc_bwd(BwdBJob& b, const FcStage& F, int t) {   // y[t] (=|+=) in[t] . W^T, W = [D rows][ld_in]
  b.dz = F.in + (size_t)t * F.N * F.ld_in; b.K = F.WT; b.Ksw = nullptr; b.H4 = F.ld_in;
  b.dx = F.y + (size_t)t * F.N * F.ldy; b.lddx = F.ldy; b.dmst = nullptr; b.len = nullptr;
  b.I = F.D; b.n_begin = 0; b.n_end = F.D; b.ldm = 0; b.t = t; b.N = F.N;
  b.dx_accumulate = F.accumulate ? 1 : 0;
  b.nblk_c = (F.D + 15) / 16;
}
static void fill_bwd_a(BwdAJob& a, const LayerRun& R, int t) {
  const LstmLayer& L = *R.L; const LstmStash& S = *R.S; const ParamSet& ps = *R.ps;
  const int H = L.H, H4 = 4 * H;
  const size_t r = (size_t)t * R.Ns + R.row0, rn = (size_t)(t + 1) * R.Ns + R.row0;
  a.dout = R.dout ? R.dout + r * L.ldP : nullptr;
  a.dmst = S.dmst + (size_t)R.row0 * L.ldP; a.Wp = L.has_proj ? ps.W(L.tWp) : nullptr; a.Wp_sw = L.has_proj ? L.Wp_sw : nullptr;
  a.dmt = S.dmt + r * L.ldP;
  a.gates = S.gates + r * H4;
  a.c_prev = S.c + r * H; a.c_cur = S.c + rn * H;
  a.wf = ps.W(L.twf); a.wi = ps.W(L.twi); a.wo = ps.W(L.two);
  a.dc = S.dc + (size_t)R.row0 * H; a.len = R.len; a.ldm = L.ldP; a.P = L.P; a.t = t; a.N = R.N; a.H = H;
  a.nblk_c = (H + bwd_a_cells() - 1) / bwd_a_cells();
  a.drop = R.drop; a.drop.tag += (unsigned long long)t;
}
static void fill_bwd_b(BwdBJob& b, const LayerRun& R, int t, bool with_dx) {
  const LstmLayer& L = *R.L; const LstmStash& S = *R.S; const ParamSet& ps = *R.ps;
  const int H4 = 4 * L.H;
  const size_t r = (size_t)t * R.Ns + R.row0;
  b.dz = S.gates + r * H4; b.K = ps.W(L.tK); b.Ksw = with_dx ? L.Kb_full : L.Kb_rec;
  b.dx = with_dx ? R.din + r * L.ldI : nullptr;
  b.dmst = S.dmst + (size_t)R.row0 * L.ldP; b.len = R.len;
  b.I = L.I; b.n_begin = with_dx ? 0 : L.I; b.n_end = L.I + L.P; b.lddx = L.ldI; b.ldm = L.ldP; b.t = t; b.N = R.N; b.H4 = H4;
  b.dx_accumulate = R.din_accumulate ? 1 : 0;
  b.nblk_c = (b.n_end - b.n_begin + 15) / 16;
}

int Model::gates_blocks(int H, int N) const { return job_blocks((H + 15) / 16, N, fwd_gates_rows()); }
int Model::proj_blocks(int P, int N) const { return job_blocks((P + 15) / 16, N); }
int Model::bwd_a_blocks(int H, int N) const { return job_blocks((H + bwd_a_cells() - 1) / bwd_a_cells(), N); }
static void run_gates(const FwdGateJobs& gj, int blocks, int kb, hipStream_t s) { launch_fwd_gates(gj, blocks, kb, s); }
static void run_proj(const FwdProjJobs& pj, int blocks, int kb, hipStream_t s) { launch_fwd_proj(pj, blocks, kb, s); }
static void run_bwd_a(const BwdAJobs& aj, int blocks, int kb, hipStream_t s) { launch_bwd_a(aj, blocks, kb, s); }
void Model::run_bwd_b_splitk(BwdBJobs& bj, hipStream_t s) { bwd_b_plan(bj, bwdb_ws); launch_bwd_b_splitk(bj, s); }

// the event ring of a bracketed launch kind (rsrgan_profile_read_kind): room for bracket number n
static void prof_ring_room(std::vector<hipEvent_t>& ev, int n, size_t step) {
  if ((size_t)(2 * n + 2) <= ev.size()) return;
  const size_t old = ev.size();
  ev.resize(old + step, nullptr);
  for (size_t i = old; i < ev.size(); ++i) (void)hipEventCreate(&ev[i]);
}
void Model::gates_launch(const FwdGateJobs& gj, int blocks, int kb, hipStream_t s) {
  if (!prof_on) { run_gates(gj, blocks, kb, s); return; }
  prof_ring_room(prof_ev, prof_n, 128);
  for (int i = 0; i < gj.n; ++i) {
    const FwdGateJob& J = gj.j[i];
    prof_flops += 2.0 * J.N * ((J.x ? J.ldx : 0) + J.ldm) * 4.0 * J.H;
  }
  (void)hipEventRecord(prof_ev[2 * prof_n], s);
  run_gates(gj, blocks, kb, s);
  (void)hipEventRecord(prof_ev[2 * prof_n + 1], s);
  ++prof_n;
}

void Model::rnn_forward(std::vector<Chain>& chains, int T, hipStream_t s, const std::vector<int>* offsets,
                        const std::vector<FcStage>* fcs) {
  if (lazy_sw) { refresh_swizzles(RSRGAN_NET_G, s); refresh_swizzles(RSRGAN_NET_D, s); }      // (from the current variables, every time)
  // zero initial state (cell.zero_state, models/lstm.py:107): slot 0 of c / m for the rows of each run
  {
    ZeroList zl{};
    for (auto& ch : chains)
      for (auto& R : ch) {
        if (R.carry) continue;                       // (the stateful forward: slot 0 holds the carried state)
        if (zl.n + 2 > 32) { launch_zero_many(zl, s); zl.n = 0; }
        zl.p[zl.n] = R.S->c + (size_t)R.row0 * R.L->H; zl.len[zl.n++] = (unsigned)((size_t)R.N * R.L->H);
        zl.p[zl.n] = R.S->mst + (size_t)R.row0 * R.L->ldP; zl.len[zl.n++] = (unsigned)((size_t)R.N * R.L->ldP);
      }
    launch_zero_many(zl, s);
  }
  auto zx_gemm = [&](const LayerRun& R) {     // x-part of every step: zx = in . K[0:I] + bias, batched over T*N frames
    const int H4 = 4 * R.L->H;
    gemm(R.in, R.L->ldI, true, R.ps->W(R.L->tK), H4, false, R.S->gates, H4, T * R.N, H4, R.L->I, R.ps->W(R.L->tb), 0, 0.f, false, s);
  };
  if (!wavefront()) {
    for (auto& ch : chains)
      for (auto& R : ch) {
        const bool zx = R.Ns == R.N && R.row0 == 0;          // rows contiguous over time -> batch the x-part
        if (zx) zx_gemm(R);
        for (int t = 0; t < T; ++t) {
          FwdGateJobs gj{}; gj.n = 1; gj.forget_bias = cfg.forget_bias;
          fill_gate(gj.j[0], R, t, zx);
          gates_launch(gj, gates_blocks(R.L->H, R.N), (zx ? 0 : kb16(R.L->ldI)) + kb16(R.L->ldP), s);
          if (R.L->has_proj) {
            FwdProjJobs pj{}; pj.n = 1;
            fill_proj(pj.j[0], R, t);
            run_proj(pj, proj_blocks(R.L->P, R.N), kb16(R.L->ldH), s);
          }
        }
      }
    return;
  }
  int last = 0;      // last diagonal with work
  for (size_t c = 0; c < chains.size(); ++c) {
    const int off = offsets ? (*offsets)[c] : 0;
    last = std::max(last, off + (int)chains[c].size() - 1 + T - 1);
    for (auto& R : chains[c])
      if (R.zx_batched) zx_gemm(R);
  }
  if (fcs)
    for (auto& F : *fcs) last = std::max(last, F.offset + T - 1);
  for (int d = 0; d <= last; ++d) {
    FwdGateJobs gj{}; gj.forget_bias = cfg.forget_bias;
    FwdProjJobs pj{};
    int gb = 0, pb = 0, gk = 0, pk = 0;
    // a diagonal's jobs only depend on earlier diagonals, so they may be split over several launches
    auto flush_g = [&]() { if (gj.n) gates_launch(gj, gb, gk, s); gj.n = 0; gb = gk = 0; };
    auto flush_p = [&]() { if (pj.n) run_proj(pj, pb, pk, s); pj.n = 0; pb = pk = 0; };
    for (size_t c = 0; c < chains.size(); ++c) {
      Chain& ch = chains[c];
      const int off = offsets ? (*offsets)[c] : 0;
      for (int l = (int)ch.size() - 1; l >= 0; --l) {     // upper layers first: their K is twice layer 0's (heavy blocks dispatch first)
        const int t = d - off - l;
        if (t < 0 || t >= T) continue;
        const LayerRun& R = ch[l];
        if (gj.n == MAXJ) flush_g();
        FwdGateJob& a = gj.j[gj.n++]; fill_gate(a, R, t, R.zx_batched); gb += gates_blocks(R.L->H, R.N);
        gk = std::max(gk, (R.zx_batched ? 0 : kb16(R.L->ldI)) + kb16(R.L->ldP));
      }
    }
    flush_g();
    for (size_t c = 0; c < chains.size(); ++c) {
      Chain& ch = chains[c];
      const int off = offsets ? (*offsets)[c] : 0;
      for (int l = (int)ch.size() - 1; l >= 0; --l) {
        const int t = d - off - l;
        if (t < 0 || t >= T) continue;
        const LayerRun& R = ch[l];
        if (!R.L->has_proj) continue;
        if (pj.n == MAXJ) flush_p();
        FwdProjJob& p = pj.j[pj.n++]; fill_proj(p, R, t); pb += proj_blocks(R.L->P, R.N);
        pk = std::max(pk, kb16(R.L->ldH));
      }
    }
    if (fcs)
      for (auto& F : *fcs) {
        const int t = d - F.offset;
        if (t < 0 || t >= T) continue;
        if (pj.n == MAXJ) flush_p();
        FwdProjJob& p = pj.j[pj.n++]; fill_fc_fwd(p, F, t); pb += proj_blocks(F.D, F.N);
        pk = std::max(pk, kb16(F.ld_in));
      }
    flush_p();
  }
}

// Kf_l = [ Kx' ; Wp_l . Kh_l ] with Kx' = K_0[0:I] (layer 0) or Wp_{l-1} . K_l[0:I_l] (I_l = P_{l-1}), then its fragment-tiled copies
void Model::refresh_fold(hipStream_t s) {
  SwizzleList sl{};
  for (size_t l = 0; l < dl.size(); ++l) {
    const LstmLayer& L = dl[l]; const LstmLayer& F = dl_fold[l];
    const int H4 = 4 * L.H;
    const float* K = D.W(L.tK);
    float* Kf = dl_fold_K[l];
    if (l == 0) (void)hipMemcpyAsync(Kf, K, (size_t)L.I * H4 * sizeof(float), hipMemcpyDeviceToDevice, s);
    else gemm(D.W(dl[l - 1].tWp), dl[l - 1].ldP, true, K, H4, false, Kf, H4, dl[l - 1].H, H4, L.I, nullptr, 0, 0.f, false, s);
    gemm(D.W(L.tWp), L.ldP, true, K + (size_t)L.I * H4, H4, false, Kf + (size_t)F.I * H4, H4, L.H, H4, L.P, nullptr, 0, 0.f, false, s);
    const int ncb = (F.H + 15) / 16;
    sl.j[sl.n++] = SwizzleJob{Kf, F.Wg_full, H4, 4, F.H, 0, 0, 0, F.I, F.P, F.ldI, 4 * ncb, (F.ldI + F.ldP + 15) / 16, 0};
    sl.j[sl.n++] = SwizzleJob{Kf, F.Wg_h, H4, 4, F.H, 0, 0, 0, F.I, F.P, 0, 4 * ncb, (F.ldP + 15) / 16, 0};
  }
  launch_swizzle_many(sl, s);
}

// The forward recurrence of a discriminator chain running alone, one launch per time step (folded cells, model.h), then the
// masked outputs of every layer as time-batched GEMMs.  The carried projection state mst is NOT produced (only the weight
// gradients read it, and this path serves the runs that do not train the discriminator).
bool Model::fold_forward(Chain& ch, int T, hipStream_t s) {
  if (dl_fold.empty() || !wavefront() || ch.size() != dl_fold.size()) return false;
  Chain fch;
  for (size_t l = 0; l < ch.size(); ++l) {
    const LayerRun& R = ch[l];
    if (R.L != &dl[l] || R.S != &d_st[l] || R.res_in || R.res_out || R.zx_batched || R.want_wgrads || R.row0 != 0 || R.Ns != R.N) return false;
    LayerRun Rf = R;
    Rf.L = &dl_fold[l]; Rf.S = &d_fold_st[l];
    if (l > 0) Rf.in = d_st[l - 1].h;                  // the masked h of the layer below (0 where t >= len)
    fch.push_back(Rf);
  }
  refresh_fold(s);                                   // from the current variables, every time: nothing can go stale, capture or not
  std::vector<Chain> chains{fch};
  const bool prof_was = prof_on;
  prof_on = false;                                   // bench.py's dominant-kernel timing covers the merged forward wave's launches only
  rnn_forward(chains, T, s);                         // (these launches execute re-associated products: K is not the algorithmic K)
  prof_on = prof_was;
  for (size_t l = 0; l < ch.size(); ++l) {           // out_t = h_t . Wp  (h_t = 0 on masked rows: dynamic_rnn's zero output)
    const LstmLayer& L = dl[l];
    gemm(d_st[l].h, L.ldH, true, D.W(L.tWp), L.ldP, false, d_st[l].out, L.ldP, T * ch[l].N, L.P, L.H, nullptr, 0, 0.f, false, s);
  }
  return true;
}

// The launch arguments of a persistent discriminator recurrence from a chain: false unless the chain is the discriminator's own stack
// over its own stash, projected cells of one width, every layer reading the one below.  flags: DPA_BWD the backward launches (dmt);
// DPA_IN0 / DPA_IN_ALL which layers get their input (layer 0's input product inside the launch / the in-kernel weight gradients);
// DPA_ROWS the chain may cover rows [row0, row0 + N) of a stash Ns rows tall (else: the whole stash, Ns and row0 stay 0).
enum { DPA_BWD = 1, DPA_IN0 = 2, DPA_IN_ALL = 4, DPA_ROWS = 8 };
bool Model::dpersist_fill(DPersistArgs& a, const Chain& ch, int T, unsigned flags, unsigned long long* gran, unsigned* ctl) const {
  a = DPersistArgs{};
  a.nl = (int)ch.size(); a.N = ch[0].N; a.T = T; a.H = dl[0].H; a.len = ch[0].len;
  a.gran = gran; a.ctl = ctl; a.forget_bias = cfg.forget_bias;
  if (flags & DPA_ROWS) { a.Ns = ch[0].Ns; a.row0 = ch[0].row0; }
  for (size_t l = 0; l < ch.size(); ++l) {
    const LayerRun& R = ch[l]; const LstmLayer& L = dl[l]; const LstmStash& S = d_st[l];
    if (R.L != &L || R.S != &S || R.res_in || R.res_out || R.N != a.N || !L.has_proj || L.H != a.H) return false;
    if (flags & DPA_ROWS ? (R.Ns != ch[0].Ns || R.row0 != ch[0].row0) : (R.row0 != 0 || R.Ns != R.N)) return false;
    if (l > 0 && R.in != d_st[l - 1].out) return false;
    DPersistLayer& D_ = a.L[l];
    D_.K = D.W(L.tK); D_.bias = D.W(L.tb); D_.wi = D.W(L.twi); D_.wf = D.W(L.twf); D_.wo = D.W(L.two); D_.Wp = D.W(L.tWp);
    D_.gates = S.gates; D_.c = S.c; D_.h = S.h; D_.mst = S.mst; D_.out = S.out;
    if (flags & DPA_BWD) D_.dmt = S.dmt;
    D_.I = L.I; D_.P = L.P; D_.ldP = L.ldP; D_.ldH = L.ldH; D_.ldI = L.ldI;
    D_.in = (flags & DPA_IN_ALL) || ((flags & DPA_IN0) && l == 0) ? R.in : nullptr;
  }
  return true;
}

// The same chain as ONE persistent launch (dpersist.hip): layer 0's x-part batched over time first, everything else in the kernel.
// Produces the complete stash (gates, c, h, mst, out), unlike fold_forward.
bool Model::persist_forward(Chain& ch, int T, hipStream_t s) {
  if (!dp_gran || !(dp_live & 1) || !wavefront() || ch.size() != dl.size()) return false;
  DPersistArgs a{};
  if (!dpersist_fill(a, ch, T, DPA_IN0, dp_gran, dp_ctl)) return false;      // (layer 0's input product runs inside the launch as well)
  if (!dpersist_supported(a) || dpersist_grid(a.nl, a.N) > dp_max_grid || dpersist_granule_bytes(a.nl, a.N, a.T) > dp_gran_bytes) return false;
  if (switches().dfwd_t && a.N % 32 == 0) launch_dlstm_fwd_t(a, s); else launch_dlstm_fwd(a, s);
  if (prof_on) ++prof_cnt[4];
  return true;
}

// The generator's stack as ONE persistent launch (gpersist.hip).  Same stash as the wavefront launches leave (gates, c, h, mst, out of
// every layer), so the backward pass does not know which forward ran.
// the discriminator's halves of the fused launches: the second tile of the (only) tile pair is padding (DPersistArgs::nrt; RSRGAN_DP_NRT=0: it runs)
int Model::trail_nrt() const {
  const bool on = switches().dp_nrt && switches().gp_nrt;             // (only beside a generator that drops the tile as well)
  // (and only when every recurrence of both nets runs persistent: see gpersist_shape's note on the padding rows of the stash)
  return on && B == 32 && Bt <= 16 && (gp_live & 3) == 3 && (dp_live & 3) == 3 ? 1 : 0;
}
bool Model::gpersist_shape(GPersistArgs& a, int T) const {              // (sizes only: usable before any buffer exists)
  const bool res = (cfg.g_type == RSRGAN_G_RES_LSTM_L || g_resi()) && switches().gp_res;      // the running residual sum rides the hand-offs (gpersist.hip RES)
  // (res_lstm_base, models/res_lstm_base.py:101-139: the same stack of projected cells fed the input frames directly, no sums)
  if (!gp_live || gl.empty() || gl.size() > (size_t)GP_MAXL || (cfg.g_type != RSRGAN_G_LSTM && cfg.g_type != RSRGAN_G_RES_LSTM_BASE && !res && !bnl_infer())) return false;
  a = GPersistArgs{};
  a.nl = (int)gl.size(); a.N = B; a.T = T; a.H = gl[0].H; a.res = res ? (g_resi() ? 2 : 1) : 0;      // (2: res_lstm_i, the sums are out_l + x -- gpersist.hip RESX, the forward launch only)
  bool noproj = !gl[0].has_proj;
  // ring slots tagged with the parity of the ring pass instead of re-armed with sentinels (gpersist.hip gp_store_t); RSRGAN_GP_TAGS=0: the sentinel form
  a.tags = switches().gp_tags && !noproj ? 1 : 0;
  if (bnl_infer()) { if (!a.tags) return false; a.cnorm = 1; }      // (gpersist.hip CN: instantiated for tagged rings only; bnl_check refuses the handle)
  for (size_t l = 0; l < gl.size(); ++l) {
    const LstmLayer& L = gl[l];
    if (L.has_proj == noproj || L.H != a.H) return false;
    GPersistLayer& G_ = a.L[l];
    G_.I = L.I; G_.P = L.P; G_.ldI = L.ldI; G_.ldP = L.ldP; G_.ldH = L.ldH;
  }
  // num_proj=None (BASELINE.json's 2 x 512 generator): the single-hop form, forward only (gpersist.hip np_fwd_body)
  if (noproj) return switches().gp_noproj && !res && (gp_live & 1) && gpersist_np_plan(a, gp_np_nt);
  if (!gpersist_plan(a)) return false;
  // a padded model whose real rows fit one 16-row tile (the shipped batch_size = 8, decode's single utterance): the other tile of the
  // row group holds padding rows only -- length 0 in every batch, zeros in every stash since the allocation -- and does not run
  // (GPersistArgs::nrt).  RSRGAN_GP_NRT=0: both tiles run.
  // (only when BOTH recurrences run persistent: a launch-path forward writes gate activations into the padding rows of the stash,
  // which a one-lane BPTT would never turn into dz = 0 -- the weight-gradient products would read them as dZ)
  if (switches().gp_nrt && B == 32 && Bt <= 16 && (gp_live & 3) == 3) a.nrt = 1;
  // the forward launch's off-chain work (the X waves' products, the stash stores) behind the lane's publication instead of beside it
  // (GPersistArgs::sched; pays with two row groups on the fabric: 13.5 -> 13.0 us per step at 64 rows, nothing at 32).  RSRGAN_GP_SCHED=0..3
  const int sched_env = switches().gp_sched;
  a.sched = sched_env >= 0 ? sched_env : (B >= 64 ? 3 : 0);
  return true;
}
bool Model::gpersist_args(GPersistArgs& a, int T) const {
  if (!gpersist_shape(a, T)) return false;
  a.len = len_dev;
  a.gran1 = gp_gran1; a.gran2 = gp_gran2; a.gran3 = gp_gran3; a.ctl = gp_ctl; a.forget_bias = cfg.forget_bias;
  for (size_t l = 0; l < gl.size(); ++l) {
    const LstmLayer& L = gl[l]; const LstmStash& S = g_st[l];
    GPersistLayer& G_ = a.L[l];
    G_.KxT = L.KxT; G_.KhT = L.KhT; G_.bias = L.bias_f ? L.bias_f : G.W(L.tb); G_.ca = L.ca; G_.cb = L.cb; G_.wi = G.W(L.twi); G_.wf = G.W(L.twf); G_.wo = G.W(L.two); G_.Wp = L.has_proj ? G.W(L.tWp) : nullptr;
    G_.gates = S.gates; G_.c = S.c; G_.h = S.h; G_.mst = S.mst; G_.out = S.out; G_.dmt = S.dmt;
    G_.res_out = a.res ? g_res[l] : nullptr;
  }
  return true;
}

// A persistent launch reported a failed bounded wait (rsrgan_device_status): its workgroups were not all resident -- somebody else's
// work on the device, CUs taken away after rsrgan_create.  Another attempt would spin into the same time-out on every step: this
// handle takes the launch-per-phase path from now on (the captured graphs hold the persistent launches: dropped).
void Model::persist_disable(int which) {
  if (which == 1) gp_live = 0; else dp_live = 0;
  lazy_sw = false;
  trail_fits = false;
  dpipe = false;
  drop_graphs();
  refresh_swizzles(RSRGAN_NET_G, nullptr);
  refresh_swizzles(RSRGAN_NET_D, nullptr);
  // (on the null stream, which orders nothing against the non-blocking streams the next call works on: rsrgan_device_status, the only
  // caller, is a synchronising call anyway)
  (void)hipStreamSynchronize(nullptr);
}

void Model::gpersist_rearm() {
  GPersistArgs a{};
  if (!gp_gran1 || !gpersist_args(a, gp_Tcap)) return;
  if (gp_noproj) {                                                       // (the unprojected form: only its BPTT has rings)
    if (gp_gran3) { gpersist_np_arm(a, 0); (void)hipDeviceSynchronize(); }
    return;
  }
  gpersist_arm(a, 0);
  (void)hipDeviceSynchronize();
}

// A stack planned as one launch per row group (GPersistArgs::ngl: res_lstm_l at 64 rows does not fit the device at once): the launches
// one after the other; `fused` (k_glstm_fwd_dt / k_glstm_bwd_dt with the discriminator's half over ALL rows) rides the launch of group
// `fused_at` -- the LAST forward launch (the FC workgroups read the earlier groups' chunks, which stay in their slots), the FIRST
// backward launch (the later groups' launches find d(outputs) complete and do not poll).
static void glstm_fwd_groups(GPersistArgs a, const DPersistArgs* d, hipStream_t s) {
  const int ngr = a.N / GP_ROWS;
  if (!a.ngl) { if (d) launch_glstm_fwd_dt(a, *d, s); else launch_glstm_fwd(a, s); return; }
  for (int g = 0; g < ngr; ++g) {
    a.grp0 = g;
    if (d && g == ngr - 1) launch_glstm_fwd_dt(a, *d, s); else launch_glstm_fwd(a, s);
  }
}
static void glstm_bwd_groups(GPersistArgs a, const DPersistArgs* d, hipStream_t s) {
  const int ngr = a.N / GP_ROWS;
  if (!a.ngl) { if (d) launch_glstm_bwd_dt(a, *d, s); else launch_glstm_bwd(a, s); return; }
  for (int g = 0; g < ngr; ++g) {
    a.grp0 = g;
    if (d && g == 0) { a.dout_trail = 1; launch_glstm_bwd_dt(a, *d, s); } else { a.dout_trail = 0; launch_glstm_bwd(a, s); }
  }
}

bool Model::persist_forward_g(int T, hipStream_t s) {
  if (!gp_fwd_on() || !wavefront() || seq_drop_on()) return false;
  GPersistArgs a{};
  if (!gpersist_args(a, T) || (gp_noproj ? gpersist_np_gran2_bytes(a) : gpersist_gran2_bytes(a)) > gp_gran2_bytes) return false;
  a.L[0].in = g_ins[0];                                // (layer 0's input product runs inside the launch as well)
  a.carry = g_carry ? 1 : 0;                           // (the stateful forward: the CARRY variants of the same launches, counted alike)
  if (infer()) {
    // the stash-free variants (gpersist.hip LEAN) on window [inf_t0, inf_t0 + T): this window's lengths, its rows of the stack's input and of
    // the top layer's outputs; below the top layer nothing is written (the layers publish through gran2)
    a.lean = 1; a.len = len_win;
    a.L[0].in = g_ins[0] + (size_t)inf_t0 * B * gl[0].ldI;
    const size_t top = gl.size() - 1;
    for (size_t l = 0; l < gl.size(); ++l) {
      GPersistLayer& G_ = a.L[l];
      G_.gates = G_.h = G_.dmt = nullptr;
      const size_t o = (size_t)inf_t0 * B * gl[l].ldP;
      G_.out = l == top && !a.res ? g_st[l].out + o : nullptr;
      G_.res_out = l == top && a.res ? g_res[l] + o : nullptr;
    }
  }
  if (gp_noproj) {                                     // num_proj=None: the single-hop form (no event bracket: bench.py's dominant-kernel timing is the projected form's)
    for (size_t l = 0; l < gl.size(); ++l) a.L[l].Wp = nullptr;
    launch_glstm_np_fwd(a, s);
    if (prof_on) ++prof_cnt[7];
    return true;
  }
  if (prof_on) {
    prof_ring_room(prof_gp_ev, prof_gp_n, 8);
    // algorithmic FLOP of the launch: every layer's input and recurrent product and its projection
    for (size_t l = 0; l < gl.size(); ++l)
      prof_gp_flops += 2.0 * Bt * T * ((double)(gl[l].I + gl[l].P) * 4.0 * gl[l].H + (double)gl[l].H * gl[l].P);
    (void)hipEventRecord(prof_gp_ev[2 * prof_gp_n], s);
    glstm_fwd_groups(a, nullptr, s);
    (void)hipEventRecord(prof_gp_ev[2 * prof_gp_n + 1], s);
    ++prof_gp_n;
    return true;
  }
  glstm_fwd_groups(a, nullptr, s);
  return true;
}

// The generator's forward recurrence with D(G(x)) a few steps behind it as ONE launch (gpersist.hip k_glstm_fwd_dt): the G-run of a
// schedule that recomputes the generator's forward (gen_updates > 1: run_gan_rnn_placeholder.sh:130): y, the discriminator's input rows
// (y + noise) and both stashes are complete behind it.  False: not applicable (the caller runs the launches one after the other).
// D(real) of the D-run as a launch of its own over rows [0, B) of the stacked stash (RSRGAN_DPIPE), with granules and control block of its own
bool Model::persist_forward_real(int T, hipStream_t q, bool check_only) {
  if (!dpipe || !dp_gran2 || !(dp_live & 1) || !wavefront()) return false;
  Chain ch = d_chain(B, 2 * B, 0);
  DPersistArgs a{};
  if (!dpersist_fill(a, ch, T, DPA_IN0 | DPA_ROWS, dp_gran2, dp_ctl2)) return false;
  if (!dpersist_supported(a) || dpersist_grid(a.nl, a.N) > dp_max_grid || T > Tmax) return false;
  if (check_only) return true;
  launch_dlstm_fwd(a, q);
  if (prof_on) ++prof_cnt[4];
  return true;
}

bool Model::persist_forward_g_trail(Chain& ch, int T, hipStream_t s, const float* nf, bool check_only) {
  if (!switches().trail_fwd || !trail_fits || !gp_fwd_on() || gp_noproj || !wavefront() || seq_drop_on() || !dp_gran || !(dp_live & 1) || ch.size() != dl.size()) return false;
  GPersistArgs a{};
  if (!gpersist_args(a, T) || a.res == 2 || gpersist_gran2_bytes(a) > gp_gran2_bytes) return false;      // (res_lstm_i: no fused launches)
  a.L[0].in = g_ins[0];
  a.fwd_trail = 1;
  DPersistArgs d{};
  // (rows [row0, row0 + N) of a stash Ns rows tall: the D-run's D(G(x)) writes the second half of the stacked stash)
  if (!dpersist_fill(d, ch, T, DPA_IN0 | DPA_ROWS, dp_gran, dp_ctl)) return false;
  if (ch[0].in != xd || d.N != B || B % 32 != 0 || dl[0].I != Dout || Dout % 4 != 0 || !dpersist_supported(d)) return false;
  if (dpersist_granule_bytes(d.nl + 1, d.N, d.T) / 2 > dp_gran_bytes) return false;      // (one edge per layer and one for layer 0's input)
  d.dy = y_tm; d.ld_dy = ldDout; d.fc_w = G.W(g_fc_out_w); d.ld_fcw = ldDout; d.fc_P = gR; d.fc_b = G.W(g_fc_out_b);
  d.noise = nf; d.dtop = xd; d.ld_dtop = ldDout; d.xd_Ns = ch[0].Ns; d.xd_row0 = ch[0].row0;
  d.nrt = trail_nrt();
  if (check_only) return true;
  if (prof_on) ++prof_fdt_n;
  glstm_fwd_groups(a, &d, s);
  g_fwd_valid = true;
  return true;
}

// BPTT through the generator's stack as ONE persistent launch (gpersist.hip k_glstm_bwd): dz over the gate activations of every
// layer's stash, dm per step in dmt.  Layer 0's input gradient (the input FC's d(h0)) is one GEMM over the dz stash afterwards.
bool Model::persist_backward_g(const Chain& ch, int T, hipStream_t s, bool check_only, const StreamFn& pre, const StreamFn& post) {
  if (!gp_gran1 || !gp_gran3 || !(gp_live & 2) || !wavefront() || seq_drop_on() || ch.size() != gl.size()) return false;
  GPersistArgs a{};
  if (!gpersist_args(a, T) || (gp_noproj ? gpersist_np_gran2_bytes(a) : gpersist_gran2_bytes(a)) > gp_gran2_bytes) return false;
  if (gp_noproj) {
    // num_proj=None (gpersist.hip k_glstm_np_bwd): dz over the gate activations of every layer's stash; no input gradient for layer 0
    if (a.NT != 2 || a.res) return false;
    for (size_t l = 0; l < ch.size(); ++l) {
      const LayerRun& R = ch[l];
      if (R.L != &gl[l] || R.S != &g_st[l] || R.res_in || R.res_out || R.row0 != 0 || R.Ns != R.N || R.N != a.N || R.len != a.len) return false;
      if (l > 0 && (R.din_accumulate || ch[l].din != ch[l - 1].dout)) return false;
    }
    if (ch[0].din) return false;
    a.dout_top = ch.back().dout; a.ld_dout = gl.back().ldP;
    if (!a.dout_top) return false;
    if (check_only) return true;
    launch_glstm_np_bwd(a, s);
    if (prof_on) ++prof_cnt[8];
    if (!defer_wgrads) chain_wgrads(ch, T, s, nullptr, pre, post);
    else { if (pre) pre(s); if (post) post(s); }
    return true;
  }
  // res_lstm_i: x is data, nothing flows into the residual branch -- d(out_{l-1}) = d(in_l) through K_x only, the plain stack's BPTT
  // (the RES = false launches); the forward sums of the chain are the stack's input + out_l
  const bool resi = a.res == 2;
  if (resi) { a.res = 0; if (gp_trail_next) return false; }
  for (size_t l = 0; l < ch.size(); ++l) {
    const LayerRun& R = ch[l];
    if (R.L != &gl[l] || R.S != &g_st[l] || R.row0 != 0 || R.Ns != R.N || R.N != a.N || R.len != a.len) return false;
    if (!a.res) {
      if (resi ? (R.res_in != g_ins[0] || R.res_out != g_res[l]) : (R.res_in || R.res_out)) return false;
      if (l > 0 && (R.din_accumulate || ch[l].din != ch[l - 1].dout)) return false;
    } else {
      // res_lstm_l: the callers keep d(inputs_l) = dx_l + d(inputs_{l+1}) accumulated in ONE buffer (dout == din, accumulate); inside the
      // launch that sum travels from reducer to reducer, the buffer is only read as the top layer's d(outputs)
      if (R.res_in != g_ins[l] || R.res_out != g_res[l] || R.dout != ch.back().dout) return false;
      if (l > 0 ? (!R.din_accumulate || R.din != R.dout) : R.din != nullptr) return false;
    }
  }
  if (!a.res && ch[0].din && ch[0].din_accumulate) return false;
  a.dout_top = ch.back().dout; a.ld_dout = gl.back().ldP;
  if (!a.dout_top) return false;
  if (check_only) return true;
  // d(inputs of layer 0) = dZ_0 . K_x^T: a time-batched GEMM behind the launch (126 us).  RSRGAN_GP_DIN0=1 runs it inside the launch
  // (layer 0's X waves publish partials to ring 0 of gran3, its reducers sum them a step late): built, bit-stable, parity-green --
  // and 0.2 ms per step SLOWER (k_glstm_bwd 16.7 -> 19.4 us per step: a third more hand-off traffic and MFMA bursts on the layer
  // every other layer waits for), so it stays off.
  const bool din_inside = ch[0].din && switches().gp_din0 && (gl[0].I + 15) / 16 <= (gl[0].P + 15) / 16 && gl[0].ldI % 4 == 0;
  if (din_inside) { a.din0 = ch[0].din; a.ld_din0 = gl[0].ldI; }
  a.dout_trail = gp_trail_next ? switch_now_trail_dbg() : 0;
  if (gp_phase == 2) {
  } else if (prof_on) {
    prof_ring_room(prof_gb_ev, prof_gb_n, 8);
    // algorithmic FLOP of the launch: every layer's state-gradient product and dh = dm . W_p^T, the input-gradient product (layer 0's
    // only when it runs inside the launch)
    for (size_t l = 0; l < gl.size(); ++l)
      prof_gb_flops += 2.0 * Bt * T * ((double)((l || din_inside ? gl[l].I : 0) + gl[l].P) * 4.0 * gl[l].H + (double)gl[l].H * gl[l].P);
    if (gp_trail_next) {      // k_glstm_bwd_dt: + the discriminator's data gradient (every layer's state- and input-gradient product, dh = dm . W_p^T) and dy . W_out^T
      for (size_t l = 0; l < dl.size(); ++l)
        prof_gb_flops += 2.0 * Bt * T * ((double)(dl[l].I + dl[l].P) * 4.0 * dl[l].H + (double)dl[l].H * dl[l].P);
      prof_gb_flops += 2.0 * Bt * T * (double)Dout * gR;
    }
    (void)hipEventRecord(prof_gb_ev[2 * prof_gb_n], s);
    glstm_bwd_groups(a, gp_trail_next ? &dt_args : nullptr, s);
    (void)hipEventRecord(prof_gb_ev[2 * prof_gb_n + 1], s);
    ++prof_gb_n;
  } else
    glstm_bwd_groups(a, gp_trail_next ? &dt_args : nullptr, s);
  if (gp_phase == 1) return true;
  auto din0 = [&](hipStream_t q) {
    if (ch[0].din && !din_inside) {
      const LayerRun& R = ch[0];
      const int H4 = 4 * R.L->H;
      gemm(R.S->gates, H4, true, R.ps->W(R.L->tK), H4, true, R.din, R.L->ldI, T * R.N, R.L->I, H4, nullptr, 0, 0.f, false, q);
    }
  };
  if (!defer_wgrads) chain_wgrads(ch, T, s, din0, pre, post);
  else { if (pre) pre(s); din0(s); if (post) post(s); }
  return true;
}

// BPTT through a discriminator chain running alone as ONE persistent launch (dpersist.hip k_dlstm_bwd), then the weight-gradient
// GEMMs over the dz it leaves in the stash.  No input gradient for layer 0 (the D-run does not need one).
bool Model::persist_backward(Chain& ch, int T, hipStream_t s) {
  if (!dp_gran || !(dp_live & 2) || !wavefront() || ch.size() != dl.size() || ch[0].din) return false;
  DPersistArgs a{};
  if (!dpersist_fill(a, ch, T, DPA_BWD | DPA_IN_ALL, dp_gran, dp_ctl)) return false;
  a.dout_top = ch.back().dout; a.ld_dout = dl.back().ldP;
  if (!a.dout_top || !dpersist_supported(a) || dpersist_grid(a.nl, a.N) > dp_max_grid || dpersist_granule_bytes(a.nl, a.N, a.T) > dp_gran_bytes) return false;
  // the weight gradients ride the launch (dp_dw_body) when every layer wants them, for the stacked call the records were sized for
  bool dw = dw_ws && !defer_wgrads && a.N == 2 * B && T <= Tmax;
  for (auto& R : ch) dw = dw && R.want_wgrads && R.in && R.ps == &D;
  if (dw) { a.dw_ws = dw_ws; a.dw_flag = dw_flag; a.dw_stride = dw_stride; }
  launch_dlstm_bwd(a, s);
  if (prof_on) { ++prof_cnt[5]; if (dw) ++prof_cnt[6]; }
  if (dw) {
    launch_dw_reduce(dw_ws, dw_stride, a.N / 16, dw_src, D.g, D.ct, D.partial, s);
    d_partial_fresh = true;
    return true;
  }
  if (!defer_wgrads) {           // (on one stream: the discriminator's sequences are short launches, two streams cost them 0.04 ms)
    bool dK_done = false;
    const bool rest = batch_wgrads(ch, T, s, true, &dK_done);
    for (auto& R : ch)
      if (R.want_wgrads) {
        if (!dK_done || !rest) layer_wgrads_gemms(R, 0, T, false, s, !dK_done, !rest);
        if (!rest) layer_wgrads_colsums(R, T, s, (side && s == side) ? scratch2 : scratch);
      }
  }
  return true;
}

bool Model::persist_backward_trail(Chain& ch, int T, hipStream_t s, float* dy, int ld_dy, float* dtop, int ld_dtop, bool check_only) {
  if (!trail_fits || !dp_gran || !(dp_live & 2) || !wavefront() || ch.size() != dl.size() || ch[0].din) return false;
  DPersistArgs a{};
  for (auto& R : ch) if (R.want_wgrads) return false;
  if (!dpersist_fill(a, ch, T, DPA_BWD, dp_gran, dp_ctl)) return false;
  a.dout_top = ch.back().dout; a.ld_dout = dl.back().ldP;
  a.dy = dy; a.ld_dy = ld_dy; a.fc_w = G.W(g_fc_out_w); a.ld_fcw = ldDout; a.fc_P = gR; a.dtop = dtop; a.ld_dtop = ld_dtop;
  if (!a.dout_top || a.N != B || dl[0].I != Dout || !dpersist_trail_supported(a) || dpersist_granule_bytes(a.nl, a.N, a.T) > dp_gran_bytes) return false;
  if (check_only) return true;
  a.nrt = trail_nrt();
  dt_args = a;                                           // (persist_backward_g launches k_glstm_bwd_dt with it)
  return true;
}

void Model::layer_wgrads_gemms(const LayerRun& R, int t0, int t1, bool accumulate, hipStream_t s, bool do_dK, bool do_dWp) {
  const LstmLayer& L = *R.L; const LstmStash& S = *R.S; const ParamSet& ps = *R.ps;
  const int H = L.H, H4 = 4 * H, Rws = (t1 - t0) * R.N;      // needs Ns == N (rows contiguous over time)
  const size_t r0 = (size_t)t0 * R.N;
  float* dK = ps.Gd(L.tK);
  // dK[0:I] (+)= in^T . dZ ; dK[I:I+P] (+)= m_{t-1}^T . dZ ; dWp (+)= h^T . dm   over frames [t0, t1)
  if (!do_dK) {
  } else if (L.I % 4 == 0) {        // one GEMM over the stacked operand [x_t | m_{t-1}] (two source stashes, one output tensor)
    launch_gemm2(R.in + r0 * L.ldI, L.ldI, S.mst + r0 * L.ldP, L.ldP, L.I, false, S.gates + r0 * H4, H4, false, dK, H4,
                 L.I + L.P, H4, Rws, nullptr, 0, 0.f, accumulate, s, (side && s == side) ? gemm_ws2 : gemm_ws, gemm_ws_floats);
  } else {
    gemm(R.in + r0 * L.ldI, L.ldI, false, S.gates + r0 * H4, H4, false, dK, H4, L.I, H4, Rws, nullptr, 0, 0.f, accumulate, s);
    gemm(S.mst + r0 * L.ldP, L.ldP, false, S.gates + r0 * H4, H4, false, dK + (size_t)L.I * H4, H4, L.P, H4, Rws, nullptr, 0, 0.f, accumulate, s);
  }
  if (L.has_proj && do_dWp)
    gemm(S.h + r0 * L.ldH, L.ldH, false, S.dmt + r0 * L.ldP, L.ldP, false, ps.Gd(L.tWp), L.ldP, H, L.P, Rws, nullptr, 0, 0.f, accumulate, s);
}

// The layers of a stack have ONE shape more often than not (generator: 3 x (280 + 280 -> 760 / p280), discriminator: 2 x (40 + 40 -> 256 /
// p40)): their projection gradients h^T dm, their bias / peephole column sums and -- where the product is small enough for k_gemm16 --
// their kernel gradients [x | m]^T dZ run as one launch per kind for all layers (blockIdx.z = layer) instead of one per layer: these
// launches are latency-bound (the discriminator's six per layer left the chip idle for 0.26 ms per D-run).  Returns whether dWp and
// the column sums are done (*dK_done: the kernel gradients as well); the caller runs per layer what is not.
bool Model::batch_wgrads(const Chain& ch, int T, hipStream_t s, bool dK_too, bool* dK_done, bool check_only) {
  *dK_done = false;
  std::vector<const LayerRun*> rs;
  for (auto& R : ch) if (R.want_wgrads) rs.push_back(&R);
  if (!switches().wgrad_batch || rs.size() < 2 || rs.size() > (size_t)GEMM16_MAXB) return false;
  const LstmLayer& L0 = *rs[0]->L;
  for (auto* R : rs) {
    const LstmLayer& L = *R->L;
    if (L.I != L0.I || L.P != L0.P || L.H != L0.H || L.ldI != L0.ldI || L.ldP != L0.ldP || L.ldH != L0.ldH || !L.has_proj ||
        R->N != rs[0]->N || R->Ns != R->N || R->row0 != 0)
      return false;
    // (an input width that is no multiple of 4 -- res_lstm_l's 257: the kernel gradient is the caller's, over the zero-padded ld columns
    //  into dk_tmp; the projection gradients and the column sums below do not care)
    if (L.I % 4 != 0 && (dK_too || !dk_tmp || R->ps != &G)) return false;
  }
  const int H = L0.H, H4 = 4 * H, Rws = T * rs[0]->N;
  if ((size_t)rs.size() * 64 * 7 * H > scratch_floats) return false;
  float* ws = (side && s == side) ? gemm_ws2 : gemm_ws;
  float* scr = (side && s == side) ? scratch2 : scratch;
  // (the rule of launch_gemm_mapped: only products with little work per tile run on k_gemm16)
  auto small = [&](int M, int N, int K) { const double outs = (double)M * N; return !(K >= 256 && outs >= 4.0e6) && !(K >= 2048 && outs >= 1.5e6); };
  if (check_only) { *dK_done = dK_too && small(L0.I + L0.P, H4, Rws); return small(H, L0.P, Rws); }      // (host-only: what a call would do)
  if (dK_too && small(L0.I + L0.P, H4, Rws)) {
    Gemm16Batch bt{}; bt.n = (int)rs.size();
    for (int p = 0; p < bt.n; ++p) { bt.A[p] = rs[p]->in; bt.A2[p] = rs[p]->S->mst; bt.B[p] = rs[p]->S->gates; bt.C[p] = rs[p]->ps->Gd(rs[p]->L->tK); }
    launch_gemm16_batch(bt, L0.ldI, L0.ldP, L0.I, H4, H4, L0.I + L0.P, H4, Rws, false, s, ws, gemm_ws_floats);
    *dK_done = true;
  }
  if (!small(H, L0.P, Rws)) return false;                     // (never for the nets of this repository: the caller runs the rest per layer)
  {
    Gemm16Batch bt{}; bt.n = (int)rs.size();
    for (int p = 0; p < bt.n; ++p) { bt.A[p] = rs[p]->S->h; bt.A2[p] = nullptr; bt.B[p] = rs[p]->S->dmt; bt.C[p] = rs[p]->ps->Gd(rs[p]->L->tWp); }
    launch_gemm16_batch(bt, L0.ldH, 0, 0, L0.ldP, L0.ldP, H, L0.P, Rws, false, s, ws, gemm_ws_floats);
  }
  {
    ColsumsBatch cb{}; cb.n = (int)rs.size();
    for (int p = 0; p < cb.n; ++p) {
      const LayerRun& R = *rs[p]; const LstmLayer& L = *R.L; const ParamSet& ps = *R.ps;
      cb.dz[p] = R.S->gates; cb.cprev[p] = R.S->c; cb.ccur[p] = R.S->c + (size_t)R.N * H;
      cb.db[p] = ps.Gd(L.tb); cb.dwi[p] = ps.Gd(L.twi); cb.dwf[p] = ps.Gd(L.twf); cb.dwo[p] = ps.Gd(L.two);
    }
    launch_lstm_colsums_batch(cb, Rws, H, scr, s);
  }
  return true;
}
void Model::layer_wgrads_colsums(const LayerRun& R, int T, hipStream_t s, float* scr) {
  const LstmLayer& L = *R.L; const LstmStash& S = *R.S; const ParamSet& ps = *R.ps;
  const int H = L.H, H4 = 4 * H, Rws = T * R.N;
  // bias: colsum(dZ); peepholes: dw_i = sum dai*c_{t-1}; dw_f = sum daf*c_{t-1}; dw_o = sum dao*c_t -- one pass over dZ
  (void)H4;
  launch_lstm_colsums(S.gates, S.c, S.c + (size_t)R.N * H, ps.Gd(L.tb), ps.Gd(L.twi), ps.Gd(L.twf), ps.Gd(L.two), Rws, H, scr, s);
}
void Model::layer_wgrads(const LayerRun& R, int T, hipStream_t s) {
  layer_wgrads_gemms(R, 0, T, false, s);
  layer_wgrads_colsums(R, T, s, (side && s == side) ? scratch2 : scratch);
}
// The weight gradients of a chain whose BPTT is complete (the persistent launches leave every layer's dz at once): the layers'
// launch sequences (dK GEMM + fix-up, dWp GEMM + reduce, the two column-sum kernels) do not depend on each other, and only the dK
// GEMM fills the chip -- the upper layers' sequences ride the side stream beside the lowest layer's (and `between`, the caller's
// launches that only need the BPTT), joined before returning.  RSRGAN_WGRAD_STREAMS=1: everything on s.
// `pre` / `post` (optional): launches of the caller that only need the BPTT's inputs / only `between`'s result (the output and input
// FCs' parameter gradients: short launches that used to follow the dK GEMMs): they ride the side stream too, `post` behind an event
// recorded on s right after `between`.
void Model::chain_wgrads(const Chain& ch, int T, hipStream_t s, const StreamFn& between, const StreamFn& pre, const StreamFn& post) {
  int nw = 0;
  for (auto& R : ch) nw += R.want_wgrads ? 1 : 0;
  if (!side || switches().wgrad_streams < 2 || nw < 2) {
    if (pre) pre(s);
    if (between) between(s);
    if (post) post(s);
    for (auto& R : ch)
      if (R.want_wgrads) layer_wgrads(R, T, s);
    return;
  }
  // RSRGAN_DIN0_SIDE=1: `between` (the input gradient of layer 0 and what hangs on it) rides the side stream as well, the chip-filling
  // kernel-gradient GEMMs start at once on s
  const bool between_side = switches().din0_side;
  hipEvent_t ev = ev_pool[ev_next++ & 15];
  (void)hipEventRecord(ev, s);
  (void)hipStreamWaitEvent(side, ev, 0);
  if (pre) pre(side);
  auto after_between = [&]() {
    if (!post) return;
    hipEvent_t e2 = ev_pool[ev_next++ & 15];
    (void)hipEventRecord(e2, s);
    (void)hipStreamWaitEvent(side, e2, 0);
    post(side);
  };
  bool dK_done = false;
  if (between_side && between && post) {
    between(side); post(side);                                  // (first on the side stream: what hangs on it is the longest chain there)
    const bool rest = batch_wgrads(ch, T, side, false, &dK_done);
    std::vector<const LayerRun*> rs;
    for (auto& R : ch) if (R.want_wgrads) rs.push_back(&R);
    bool batched = false;
    if (rest && rs.size() >= 2 && rs.size() <= (size_t)GEMM_MAXB) {
      const float *A_[GEMM_MAXB], *A2_[GEMM_MAXB], *B_[GEMM_MAXB]; float* C_[GEMM_MAXB];
      const LstmLayer& L0 = *rs[0]->L;
      const bool padI = L0.I % 4 != 0;                     // (x over its ld columns into dk_tmp, rows copied behind: see model.h dk_tmp)
      const int Ie = padI ? L0.ldI : L0.I;
      for (size_t i = 0; i < rs.size(); ++i) { A_[i] = rs[i]->in; A2_[i] = rs[i]->S->mst; B_[i] = rs[i]->S->gates; C_[i] = padI ? dk_tmp + i * dk_tmp_per : rs[i]->ps->Gd(rs[i]->L->tK); }
      batched = launch_gemm_batch((int)rs.size(), A_, L0.ldI, A2_, L0.ldP, Ie, B_, 4 * L0.H, C_, 4 * L0.H, Ie + L0.P, 4 * L0.H, T * rs[0]->N, false, s, gemm_ws, gemm_ws_floats);
      if (batched && padI)
        for (size_t i = 0; i < rs.size(); ++i) {
          float* dK_ = rs[i]->ps->Gd(rs[i]->L->tK);
          launch_copy_f(C_[i], dK_, L0.I * 4 * L0.H, s);
          launch_copy_f(C_[i] + (size_t)Ie * 4 * L0.H, dK_ + (size_t)L0.I * 4 * L0.H, L0.P * 4 * L0.H, s);
        }
    }
    for (auto& R : ch)
      if (R.want_wgrads) {
        if (!batched || !rest) layer_wgrads_gemms(R, 0, T, false, s, !batched, !rest);
        if (!rest) layer_wgrads_colsums(R, T, s, scratch);
      }
  } else if (batch_wgrads(ch, T, side, false, &dK_done)) {
    // every layer's dWp + column sums as three launches beside the chip-filling dK GEMMs, which stay on s one after the other
    if (between) between(s);
    after_between();
    // the layers' kernel gradients [x | m]^T dZ: same shapes (batch_wgrads checked that) -> one stream-K launch over all of them
    std::vector<const LayerRun*> rs;
    for (auto& R : ch) if (R.want_wgrads) rs.push_back(&R);
    bool batched = false;
    if (rs.size() >= 2 && rs.size() <= (size_t)GEMM_MAXB) {
      const float *A_[GEMM_MAXB], *A2_[GEMM_MAXB], *B_[GEMM_MAXB]; float* C_[GEMM_MAXB];
      const LstmLayer& L0 = *rs[0]->L;
      const bool padI = L0.I % 4 != 0;                     // (x over its ld columns into dk_tmp, rows copied behind: see model.h dk_tmp)
      const int Ie = padI ? L0.ldI : L0.I;
      for (size_t i = 0; i < rs.size(); ++i) { A_[i] = rs[i]->in; A2_[i] = rs[i]->S->mst; B_[i] = rs[i]->S->gates; C_[i] = padI ? dk_tmp + i * dk_tmp_per : rs[i]->ps->Gd(rs[i]->L->tK); }
      batched = launch_gemm_batch((int)rs.size(), A_, L0.ldI, A2_, L0.ldP, Ie, B_, 4 * L0.H, C_, 4 * L0.H, Ie + L0.P, 4 * L0.H, T * rs[0]->N, false, s,
                                  (side && s == side) ? gemm_ws2 : gemm_ws, gemm_ws_floats);
      if (batched && padI)
        for (size_t i = 0; i < rs.size(); ++i) {
          float* dK_ = rs[i]->ps->Gd(rs[i]->L->tK);
          launch_copy_f(C_[i], dK_, L0.I * 4 * L0.H, s);
          launch_copy_f(C_[i] + (size_t)Ie * 4 * L0.H, dK_ + (size_t)L0.I * 4 * L0.H, L0.P * 4 * L0.H, s);
        }
    }
    if (!batched)
      for (auto& R : ch)
        if (R.want_wgrads) layer_wgrads_gemms(R, 0, T, false, s, true, false);
  } else {
    bool first = true;
    for (auto& R : ch) {
      if (!R.want_wgrads) continue;
      if (first) { first = false; continue; }                  // (the lowest layer with weight gradients stays on s)
      layer_wgrads(R, T, side);
    }
    if (between) between(s);
    after_between();
    for (auto& R : ch)
      if (R.want_wgrads) { layer_wgrads(R, T, s); break; }
  }
  ev = ev_pool[ev_next++ & 15];
  (void)hipEventRecord(ev, side);
  (void)hipStreamWaitEvent(s, ev, 0);                       // join: the optimizer needs every gradient
}

void Model::rnn_backward(std::vector<Chain>& chains, int T, hipStream_t s, const std::vector<int>* offsets,
                         const std::vector<FcStage>* fcs) {
  if (lazy_sw) { refresh_swizzles(RSRGAN_NET_G, s); refresh_swizzles(RSRGAN_NET_D, s); }
  {
    ZeroList zl{};
    for (auto& ch : chains)
      for (auto& R : ch) {
        if (zl.n + 2 > 32) { launch_zero_many(zl, s); zl.n = 0; }
        zl.p[zl.n] = R.S->dc + (size_t)R.row0 * R.L->H; zl.len[zl.n++] = (unsigned)((size_t)R.N * R.L->H);
        zl.p[zl.n] = R.S->dmst + (size_t)R.row0 * R.L->ldP; zl.len[zl.n++] = (unsigned)((size_t)R.N * R.L->ldP);
      }
    launch_zero_many(zl, s);
  }
  if (!wavefront()) {
    for (auto& ch : chains)
      for (int l = (int)ch.size() - 1; l >= 0; --l) {
        const LayerRun& R = ch[l];
        for (int t = T - 1; t >= 0; --t) {
          BwdAJobs aj{}; aj.n = 1; fill_bwd_a(aj.j[0], R, t);
          run_bwd_a(aj, bwd_a_blocks(R.L->H, R.N), kb16(R.L->ldP), s);
          BwdBJobs bj{}; bj.n = 1; fill_bwd_b(bj.j[0], R, t, false);
          if (bwd_b_splitk_ok(bj)) run_bwd_b_splitk(bj, s);
          else launch_bwd_b(bj, job_blocks(bj.j[0].nblk_c, R.N, kb16(4 * R.L->H) <= 64 ? 16 : 32), kb16(4 * R.L->H), s);
        }
        if (R.want_wgrads) layer_wgrads(R, T, s);
        if (R.din) {   // din (+)= dZ . K[0:I]^T, batched over time
          const int H4 = 4 * R.L->H;
          gemm(R.S->gates, H4, true, R.ps->W(R.L->tK), H4, true, R.din, R.L->ldI, T * R.N, R.L->I, H4, nullptr, 0, 0.f,
               R.din_accumulate, s);
        }
      }
    return;
  }
  int last = 0;
  for (size_t c = 0; c < chains.size(); ++c)
    last = std::max(last, (offsets ? (*offsets)[c] : 0) + (int)chains[c].size() - 1 + T - 1);
  if (fcs)
    for (auto& F : *fcs) last = std::max(last, F.offset + T - 1);
  // Weight-gradient GEMMs ride a side stream in time chunks: a chunk [tb, te) of a chain is final once
  // its bottom layer has passed time tb, i.e. after diagonal (T-1-tb) + off + Lc - 1.
  const int nchunk = (overlap() && T >= 16) ? 4 : 1;
  bool any_w = false;
  for (auto& ch : chains) for (auto& R : ch) any_w |= R.want_wgrads;
  const bool ovl = overlap() && any_w;
  std::vector<int> chunk_done(chains.size(), 0);            // chunks already handed to the side stream
  auto chunk_lo = [&](int c) { return T - ((c + 1) * T) / nchunk; };   // chunk c (c=0 = latest frames): [lo, hi)
  auto chunk_hi = [&](int c) { return T - (c * T) / nchunk; };
  for (int d = 0; d <= last; ++d) {
    BwdAJobs aj{}; BwdBJobs bj{};
   
    int ab = 0, bb = 0, ak = 0, bk = 0;
    auto flush_a = [&]() { if (aj.n) run_bwd_a(aj, ab, ak, s); aj.n = 0; ab = ak = 0; };
    auto flush_b = [&]() {
      if (bj.n) {
        if (bwd_b_splitk_ok(bj)) run_bwd_b_splitk(bj, s);
        else {
          launch_bwd_b(bj, bb, bk, s);                 // (small-K launches use 16-row tiles; the launcher places the jobs)
        }
      }
      bj.n = 0; bb = bk = 0;
    };
    for (size_t c = 0; c < chains.size(); ++c) {
      Chain& ch = chains[c];
      const int Lc = (int)ch.size(), off = offsets ? (*offsets)[c] : 0;
      for (int l = Lc - 1; l >= 0; --l) {
        const int t = T - 1 - (d - off - (Lc - 1 - l));
        if (t < 0 || t >= T) continue;
        if (aj.n == MAXJ) flush_a();
        BwdAJob& a = aj.j[aj.n++]; fill_bwd_a(a, ch[l], t); ab += bwd_a_blocks(ch[l].L->H, ch[l].N);
        ak = std::max(ak, kb16(ch[l].L->ldP));
      }
    }
    flush_a();
    for (size_t c = 0; c < chains.size(); ++c) {
      Chain& ch = chains[c];
      const int Lc = (int)ch.size(), off = offsets ? (*offsets)[c] : 0;
      for (int l = Lc - 1; l >= 0; --l) {
        const int t = T - 1 - (d - off - (Lc - 1 - l));
        if (t < 0 || t >= T) continue;
        const LayerRun& R = ch[l];
        if (bj.n == MAXJ) flush_b();
        BwdBJob& b = bj.j[bj.n++]; fill_bwd_b(b, R, t, R.din != nullptr); bb += job_blocks(b.nblk_c, R.N);
        bk = std::max(bk, kb16(4 * R.L->H));
      }
    }
    if (fcs)
      for (auto& F : *fcs) {
        const int t = T - 1 - (d - F.offset);
        if (t < 0 || t >= T) continue;
        if (bj.n == MAXJ) flush_b();
        BwdBJob& b = bj.j[bj.n++]; fill_fc_bwd(b, F, t); bb += job_blocks(b.nblk_c, F.N);
        bk = std::max(bk, kb16(F.ld_in));
      }
    flush_b();
    if (ovl) {
      for (size_t c = 0; c < chains.size(); ++c) {
        Chain& ch = chains[c];
        if (!ch[0].want_wgrads) continue;
        const int off = offsets ? (*offsets)[c] : 0, Lc = (int)ch.size();
        while (chunk_done[c] < nchunk && d >= (T - 1 - chunk_lo(chunk_done[c])) + off + Lc - 1) {
          const int cc = chunk_done[c]++;
          hipEvent_t ev = ev_pool[ev_next++ & 15];
          (void)hipEventRecord(ev, s);
          (void)hipStreamWaitEvent(side, ev, 0);
          for (auto& R : ch)
            if (R.want_wgrads) layer_wgrads_gemms(R, chunk_lo(cc), chunk_hi(cc), cc > 0, side);
        }
      }
    }
  }
  if (ovl) {
    for (auto& ch : chains)
      for (auto& R : ch)
        if (R.want_wgrads) layer_wgrads_colsums(R, T, side, scratch2);
    hipEvent_t ev = ev_pool[ev_next++ & 15];
    (void)hipEventRecord(ev, side);
    (void)hipStreamWaitEvent(s, ev, 0);                     // join: the optimizer needs every gradient
  } else if (!defer_wgrads) {
    for (auto& ch : chains)
      for (auto& R : ch)
        if (R.want_wgrads) layer_wgrads(R, T, s);
  }
}

}  // namespace rsr
