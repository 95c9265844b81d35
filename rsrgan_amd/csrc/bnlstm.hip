// bnlstm.hip -- kernels of the recurrent batch-norm LSTMP generator (models/bnlstm.py:38-127, models/BNLSTMCell.py): one
// BNLSTMCell layer runs two launches per time step in each direction; everything batched over time is a GEMM or a column sum
// of the existing launchers (bnlstm.cpp).
//
// The statistics of every batch-norm site are per column over the batch rows of ONE step (tf.nn.moments(x, [0])), so a workgroup
// that owns a few cell units owns their columns for ALL B <= 64 rows and every reduction is local: no cross-workgroup coupling,
// fixed summation orders, bit-reproducible.  Products with a step's weights run on v_mfma_f32_16x16x4_f32: each wave takes every
// NW-th k-step of all tiles and the waves' partial tiles are added in wave order through LDS.
#include "model.h"

namespace rsr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int BNL_U = 8;                 // cell units per workgroup of the cell kernels (4 gates x 8 units = 32 gate columns)
constexpr int BNL_MAXB = 64;             // rows of a step (one workgroup holds all of them)
constexpr int BNL_PC = 16;               // output columns per workgroup of the projection / state-gradient kernels

__device__ __forceinline__ float sig(float x) { return 1.0f / (1.0f + expf(-x)); }

// C[RT*16][NCT*16] = A[rows][K] . B[K][cols] into red[0..): every wave accumulates the k-steps ks = w, w + NW, ... of all
// tiles, the NW partial tiles are then summed in wave order (deterministic).  fa(r, k) / fb(k, c) return 0 outside the operands.
// red: NW * (BNL_MAXB * NCT * 16) floats; the result is left as red[r * NCT * 16 + c].
template <int NW, int NCT, class FA, class FB>
__device__ void wg_mma(int RT, int K, FA fa, FB fb, float* red) {
  constexpr int LDC = NCT * 16, PART = BNL_MAXB * LDC;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  f32x4 acc[4][NCT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NCT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int r16 = lane & 15, kq = lane >> 4;
  // UNR k-steps per round: all their operand loads are issued before the first MFMA (a step's operands come from L2 / HBM; one
  // load-then-MFMA per k-step left every launch bound by memory latency)
  constexpr int UNR = 8;
  for (int k0 = 4 * w; k0 < K; k0 += 4 * NW * UNR) {
    float bv[UNR][NCT], av[UNR][4];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int k = k0 + 4 * NW * u + kq;
#pragma unroll
      for (int j = 0; j < NCT; ++j) bv[u][j] = fb(k, j * 16 + r16);
#pragma unroll
      for (int i = 0; i < 4; ++i) av[u][i] = i < RT ? fa(i * 16 + r16, k) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < RT)                                            // (wave-uniform)
#pragma unroll
          for (int j = 0; j < NCT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][i], bv[u][j], acc[i][j], 0, 0, 0);
  }
  float* mine = red + w * PART;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < RT)
#pragma unroll
      for (int j = 0; j < NCT; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) mine[(i * 16 + 4 * kq + q) * LDC + j * 16 + r16] = acc[i][j][q];
  __syncthreads();
  const int n = RT * 16 * LDC;
  for (int e = threadIdx.x; e < n; e += NW * 64) {
    float s = red[e];
    for (int v = 1; v < NW; ++v) s += red[v * PART + e];
    red[e] = s;
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------- forward
// BN_input for all t at once: zx [T*B][4H] -> xh_in (x-hat) and yin = scale * x-hat + offset; training: the step's moments
// (biased variance) -> mu / var [t][0, 4H), else the moving statistics.
__global__ __launch_bounds__(64) void k_bnl_bn_in(BnlLayer a, const float* __restrict__ zx, int T) {
  const int t = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x, H4 = 4 * a.H, B = a.B;
  if (j >= H4 || t >= T) return;
  const float* z = zx + (size_t)t * B * H4 + j;
  float mean, var;
  if (a.train) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += z[(size_t)b * H4];
    mean = s / B;
    float q = 0.f;
    for (int b = 0; b < B; ++b) { const float d = z[(size_t)b * H4] - mean; q += d * d; }
    var = q / B;
    a.mu[(size_t)t * a.nst + j] = mean; a.var[(size_t)t * a.nst + j] = var;
  } else {
    mean = a.mm_in[j]; var = a.mv_in[j];
  }
  const float rs = 1.0f / sqrtf(var + a.eps), sc = a.sc_in[j], of = a.of_in[j];
  for (int b = 0; b < B; ++b) {
    const size_t o = ((size_t)t * B + b) * H4 + j;
    const float xh = (z[(size_t)b * H4] - mean) * rs;
    a.xh_in[o] = xh;
    a.yin[o] = sc * xh + of;
  }
}

// one step of BNLSTMCell.call (BNLSTMCell.py:176-217) for BNL_U units x all B rows; dynamic_rnn's copy-through of (c, m) for rows
// past their length.  grid = ceil(H / BNL_U), 256 threads.
__global__ __launch_bounds__(256) void k_bnl_cell_fwd(BnlLayer a, int t) {
  __shared__ float red[4 * BNL_MAXB * 32];
  __shared__ float s_mean[32], s_rs[32], s_cn[BNL_MAXB * BNL_U], s_zo[BNL_MAXB * BNL_U], s_cm[BNL_U], s_cr[BNL_U];
  const int H = a.H, H4 = 4 * H, B = a.B, P = a.P, u0 = blockIdx.x * BNL_U, RT = (B + 15) >> 4;
  const float* mprev = a.mst + (size_t)t * B * a.ldP;
  auto col = [&](int c) { return (c >> 3) * H + u0 + (c & 7); };            // gate column of local column c (gate-major: i j f o)
  auto ok = [&](int c) { return u0 + (c & 7) < H; };
  wg_mma<4, 2>(RT, P,
               [&](int r, int k) { return (r < B && k < P) ? mprev[(size_t)r * a.ldP + k] : 0.f; },
               [&](int k, int c) { return (k < P && ok(c)) ? a.Whh[(size_t)k * H4 + col(c)] : 0.f; }, red);
  // state site: hh = m_{t-1} . W_hh
  if (threadIdx.x < 32 && ok(threadIdx.x)) {
    const int c = threadIdx.x, j = col(c);
    float mean, var;
    if (a.train) {
      float s = 0.f;
      for (int b = 0; b < B; ++b) s += red[b * 32 + c];
      mean = s / B;
      float q = 0.f;
      for (int b = 0; b < B; ++b) { const float d = red[b * 32 + c] - mean; q += d * d; }
      var = q / B;
      a.mu[(size_t)t * a.nst + H4 + j] = mean; a.var[(size_t)t * a.nst + H4 + j] = var;
    } else {
      mean = a.mm_s[j]; var = a.mv_s[j];
    }
    s_mean[c] = mean; s_rs[c] = 1.0f / sqrtf(var + a.eps);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < B * BNL_U; e += 256) {
    const int b = e >> 3, uu = e & 7, u = u0 + uu;
    if (u >= H) continue;
    const size_t rz = ((size_t)t * B + b) * H4;
    float z[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = g * 8 + uu, j = g * H + u;
      const float xh = (red[b * 32 + c] - s_mean[c]) * s_rs[c];
      a.xh_s[rz + j] = xh;
      z[g] = a.yin[rz + j] + (a.sc_s[j] * xh + a.of_s[j]) + a.bias[j];
    }
    const float cp = a.ccar[((size_t)t * B + b) * a.ldH + u];
    const float ai = sig(z[0] + a.wi[u] * cp), gj = tanhf(z[1]), af = sig(z[2] + a.fb + a.wf[u] * cp);
    const float cn = cp * af + ai * gj;
    a.act[rz + u] = ai; a.act[rz + H + u] = gj; a.act[rz + 2 * H + u] = af;
    a.cnew[((size_t)t * B + b) * a.ldH + u] = cn;
    s_cn[e] = cn; s_zo[e] = z[3];
  }
  __syncthreads();
  // cell site: BN(c) over the B rows (rows past their length included: dynamic_rnn runs the cell on all of them)
  if (threadIdx.x < BNL_U && u0 + threadIdx.x < H) {
    const int uu = threadIdx.x, u = u0 + uu;
    float mean, var;
    if (a.train) {
      float s = 0.f;
      for (int b = 0; b < B; ++b) s += s_cn[b * BNL_U + uu];
      mean = s / B;
      float q = 0.f;
      for (int b = 0; b < B; ++b) { const float d = s_cn[b * BNL_U + uu] - mean; q += d * d; }
      var = q / B;
      a.mu[(size_t)t * a.nst + 2 * H4 + u] = mean; a.var[(size_t)t * a.nst + 2 * H4 + u] = var;
    } else {
      mean = a.mm_c[u]; var = a.mv_c[u];
    }
    s_cm[uu] = mean; s_cr[uu] = 1.0f / sqrtf(var + a.eps);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < B * BNL_U; e += 256) {
    const int b = e >> 3, uu = e & 7, u = u0 + uu;
    if (u >= H) continue;
    const size_t rz = ((size_t)t * B + b) * H4, rh = ((size_t)t * B + b) * a.ldH;
    const float cn = s_cn[e], ch = (cn - s_cm[uu]) * s_cr[uu];
    const float ao = sig(s_zo[e] + a.wo[u] * cn);
    a.act[rz + 3 * H + u] = ao;
    a.chat[rh + u] = ch;
    a.h[rh + u] = ao * tanhf(a.sc_c[u] * ch + a.of_c[u]);
    const float cp = a.ccar[rh + u];
    a.ccar[rh + (size_t)B * a.ldH + u] = t < a.len[b] ? cn : cp;
  }
}

// m_t = h_t . W_proj; rows past their length: output 0, m carried.  grid = ceil(P / BNL_PC), 256 threads.
__global__ __launch_bounds__(256) void k_bnl_proj(BnlLayer a, int t) {
  __shared__ float red[4 * BNL_MAXB * BNL_PC];
  const int B = a.B, H = a.H, P = a.P, p0 = blockIdx.x * BNL_PC, RT = (B + 15) >> 4;
  const float* h = a.h + (size_t)t * B * a.ldH;
  wg_mma<4, 1>(RT, H,
               [&](int r, int k) { return (r < B && k < H) ? h[(size_t)r * a.ldH + k] : 0.f; },
               [&](int k, int c) { return (k < H && p0 + c < P) ? a.Wp[(size_t)k * a.ldP + p0 + c] : 0.f; }, red);
  for (int e = threadIdx.x; e < B * BNL_PC; e += 256) {
    const int b = e / BNL_PC, c = e % BNL_PC, p = p0 + c;
    if (p >= P) continue;
    const size_t o = ((size_t)t * B + b) * a.ldP + p;
    const bool v = t < a.len[b];
    const float m = red[b * BNL_PC + c];
    a.mst[o + (size_t)B * a.ldP] = v ? m : a.mst[o];
    a.out[o] = v ? m : 0.f;
  }
}

// moving statistics of a training run: the sequential EMA over t = 0..T-1, all three sites of one layer
__global__ __launch_bounds__(256) void k_bnl_ema(BnlLayer a, int T, float decay) {
  const int j = blockIdx.x * 256 + threadIdx.x, H4 = 4 * a.H;
  if (j >= a.nst) return;
  float *mm, *mv;
  int c;
  if (j < H4) { mm = a.mm_in; mv = a.mv_in; c = j; }
  else if (j < 2 * H4) { mm = a.mm_s; mv = a.mv_s; c = j - H4; }
  else { mm = a.mm_c; mv = a.mv_c; c = j - 2 * H4; }
  float m = mm[c], v = mv[c];
  const float one_m = 1.0f - decay;
  for (int t = 0; t < T; ++t) {
    m = m * decay + a.mu[(size_t)t * a.nst + j] * one_m;
    v = v * decay + a.var[(size_t)t * a.nst + j] * one_m;
  }
  mm[c] = m; mv[c] = v;
}

// --------------------------------------------------------------------------------------------------------------- backward
// Step t of the BPTT for BNL_U units x all B rows: dm_new = (dout_t + dm_carry) on live rows (0 past the length; stashed by
// workgroup 0 for dW_proj), dh = dm_new . W_proj^T, back through h = sigma(o + w_o c) tanh(BN_cell(c)), the cell-site batch norm
// (all rows), the peepholes and the gates -> dz; the state-site batch norm -> d(hh); the carried dc.  grid = ceil(H / BNL_U).
__global__ __launch_bounds__(256) void k_bnl_cell_bwd(BnlLayer a, int t) {
  __shared__ float red[4 * BNL_MAXB * 16];
  __shared__ float s_g1[BNL_MAXB * BNL_U], s_g2[BNL_MAXB * BNL_U], s_dz[BNL_MAXB * 32], s_m1[32], s_m2[32];
  const int H = a.H, H4 = 4 * H, B = a.B, P = a.P, u0 = blockIdx.x * BNL_U, RT = (B + 15) >> 4;
  const float* dout = a.dout + (size_t)t * B * a.ldP;
  auto dmn = [&](int r, int k) { return (r < B && k < P && t < a.len[r]) ? dout[(size_t)r * a.ldP + k] + a.dmc[(size_t)r * a.ldP + k] : 0.f; };
  if (blockIdx.x == 0)
    for (int e = threadIdx.x; e < B * P; e += 256) {
      const int b = e / P, p = e % P;
      a.dmn[((size_t)t * B + b) * a.ldP + p] = dmn(b, p);
    }
  wg_mma<4, 1>(RT, P, dmn,
               [&](int k, int c) { return (k < P && c < BNL_U && u0 + c < H) ? a.Wp[(size_t)(u0 + c) * a.ldP + k] : 0.f; }, red);
  const size_t nst = a.nst;
  for (int e = threadIdx.x; e < B * BNL_U; e += 256) {
    const int b = e >> 3, uu = e & 7, u = u0 + uu;
    if (u >= H) continue;
    const size_t rz = ((size_t)t * B + b) * H4, rh = ((size_t)t * B + b) * a.ldH;
    const float ch = a.chat[rh + u], ao = a.act[rz + 3 * H + u];
    const float ty = tanhf(a.sc_c[u] * ch + a.of_c[u]), dh = red[b * 16 + uu];
    const float dyc = dh * ao * (1.f - ty * ty);
    a.dyc[rh + u] = dyc;
    s_dz[b * 32 + 24 + uu] = dh * ty * ao * (1.f - ao);                // d(o + w_o c)
    s_g1[e] = dyc * a.sc_c[u];
    s_g2[e] = dyc * a.sc_c[u] * ch;
  }
  __syncthreads();
  if (threadIdx.x < BNL_U) {
    const int uu = threadIdx.x;
    float s1 = 0.f, s2 = 0.f;
    for (int b = 0; b < B; ++b) { s1 += s_g1[b * BNL_U + uu]; s2 += s_g2[b * BNL_U + uu]; }
    s_m1[uu] = s1 / B; s_m2[uu] = s2 / B;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < B * BNL_U; e += 256) {
    const int b = e >> 3, uu = e & 7, u = u0 + uu;
    if (u >= H) continue;
    const size_t rz = ((size_t)t * B + b) * H4, rh = ((size_t)t * B + b) * a.ldH;
    const bool live = t < a.len[b];
    const float rs = 1.0f / sqrtf(a.var[(size_t)t * nst + 2 * H4 + u] + a.eps);
    const float cp = a.ccar[rh + u], ch = a.chat[rh + u];
    const float ai = a.act[rz + u], gj = a.act[rz + H + u], af = a.act[rz + 2 * H + u];
    const float dzo = s_dz[b * 32 + 24 + uu];
    const float dcar = a.dcc[(size_t)b * a.ldH + u];
    float dc = live ? dcar : 0.f;
    dc += dzo * a.wo[u] + rs * (s_g1[e] - s_m1[uu] - ch * s_m2[uu]);
    const float dzf = dc * cp * af * (1.f - af), dzi = dc * gj * ai * (1.f - ai), dzj = dc * ai * (1.f - gj * gj);
    const float dcp = dc * af + dzf * a.wf[u] + dzi * a.wi[u];
    a.dcc[(size_t)b * a.ldH + u] = dcp + (live ? 0.f : dcar);
    a.dz[rz + u] = dzi; a.dz[rz + H + u] = dzj; a.dz[rz + 2 * H + u] = dzf; a.dz[rz + 3 * H + u] = dzo;
    s_dz[b * 32 + uu] = dzi; s_dz[b * 32 + 8 + uu] = dzj; s_dz[b * 32 + 16 + uu] = dzf;
  }
  __syncthreads();
  // state site: BN backward over the B rows of the step
  if (threadIdx.x < 32 && u0 + (threadIdx.x & 7) < H) {
    const int c = threadIdx.x, j = (c >> 3) * H + u0 + (c & 7);
    const float sc = a.sc_s[j];
    float s1 = 0.f, s2 = 0.f;
    for (int b = 0; b < B; ++b) {
      const float g = s_dz[b * 32 + c] * sc;
      s1 += g; s2 += g * a.xh_s[((size_t)t * B + b) * H4 + j];
    }
    s_m1[c] = s1 / B; s_m2[c] = s2 / B;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < B * 32; e += 256) {
    const int b = e >> 5, c = e & 31;
    if (u0 + (c & 7) >= H) continue;
    const int j = (c >> 3) * H + u0 + (c & 7);
    const size_t o = ((size_t)t * B + b) * H4 + j;
    const float rs = 1.0f / sqrtf(a.var[(size_t)t * nst + H4 + j] + a.eps);
    a.dhh[o] = rs * (s_dz[b * 32 + c] * a.sc_s[j] - s_m1[c] - a.xh_s[o] * s_m2[c]);
  }
}

// dm_carry = d(hh)_t . W_hh^T (+ the carried dm on rows past their length: m_t = m_{t-1} there).  grid = ceil(P / BNL_PC),
// 1024 threads (16 waves share the 4H-deep product).
__global__ __launch_bounds__(1024) void k_bnl_dm(BnlLayer a, int t) {
  __shared__ float red[16 * BNL_MAXB * BNL_PC];
  const int B = a.B, H4 = 4 * a.H, P = a.P, p0 = blockIdx.x * BNL_PC, RT = (B + 15) >> 4;
  const float* dhh = a.dhh + (size_t)t * B * H4;
  wg_mma<16, 1>(RT, H4,
                [&](int r, int k) { return (r < B && k < H4) ? dhh[(size_t)r * H4 + k] : 0.f; },
                [&](int k, int c) { return (k < H4 && p0 + c < P) ? a.Whh[(size_t)(p0 + c) * H4 + k] : 0.f; }, red);
  for (int e = threadIdx.x; e < B * BNL_PC; e += 1024) {
    const int b = e / BNL_PC, c = e % BNL_PC, p = p0 + c;
    if (p >= P) continue;
    const size_t o = (size_t)b * a.ldP + p;
    a.dmc[o] = red[b * BNL_PC + c] + (t < a.len[b] ? 0.f : a.dmc[o]);
  }
}

// BN_input backward for all t at once: dz -> d(zx) (into dzx [T*B][4H])
__global__ __launch_bounds__(64) void k_bnl_bn_in_bwd(BnlLayer a, float* __restrict__ dzx, int T) {
  const int t = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x, H4 = 4 * a.H, B = a.B;
  if (j >= H4 || t >= T) return;
  const float sc = a.sc_in[j], rs = 1.0f / sqrtf(a.var[(size_t)t * a.nst + j] + a.eps);
  float s1 = 0.f, s2 = 0.f;
  for (int b = 0; b < B; ++b) {
    const size_t o = ((size_t)t * B + b) * H4 + j;
    const float g = a.dz[o] * sc;
    s1 += g; s2 += g * a.xh_in[o];
  }
  s1 /= B; s2 /= B;
  for (int b = 0; b < B; ++b) {
    const size_t o = ((size_t)t * B + b) * H4 + j;
    dzx[o] = rs * (a.dz[o] * sc - s1 - a.xh_in[o] * s2);
  }
}

// ------------------------------------------------------------------------------------------------------------------ decode
// Outside training every batch-norm site normalises with the moving statistics (BNLSTMCell.py:43-49): constants of the handle, so each
// site is a per-column affine map and the cell a peephole LSTMP with scaled kernels.  With g = scale / sqrt(moving_var + eps)
// -- computed as scale * (1.0f / sqrtf(moving_var + eps)), the expression of the step kernels above --:
//   KxT[col][k] = g_in[col] W_xh[k][col],  KhT[col][k] = g_st[col] W_hh[k][col]        (k-contiguous, rows zero-padded to their ld)
//   bias_f[col] = (bias + (offset_in - g_in mean_in)) + (offset_st - g_st mean_st)
//   ca[u] = g_cell[u],  cb[u] = offset_cell - g_cell mean_cell
// grid (ceil(4H / 32), ceil(max(ldI, ldP) / 32), 2 = input | state), 256 threads: a 32 x 32 tile through LDS, coalesced on both sides;
// the first tile row of the input half also writes the bias, that of the state half the cell pair.
__global__ __launch_bounds__(256) void k_bnl_fold(BnlFold a) {
  __shared__ float tile[32][33];
  const int H4 = 4 * a.H, P = a.P, st = blockIdx.z;
  const float* W = st ? a.Wh : a.Wx;
  float* out = st ? a.KhT : a.KxT;
  const int ld = st ? a.ldP : a.ldI;
  const float *sc = a.bn[4 * st], *mv = a.bn[4 * st + 3];
  const int c0 = blockIdx.x * 32, k0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int k = k0 + i, c = c0 + tx;
    tile[i][tx] = (k < P && c < H4) ? W[(size_t)k * H4 + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, k = k0 + tx;
    if (c < H4 && k < ld) {
      const float g = sc[c] * (1.0f / sqrtf(mv[c] + a.eps));
      out[(size_t)c * ld + k] = k < P ? tile[tx][i] * g : 0.f;
    }
  }
  if (blockIdx.y != 0 || ty != 0) return;
  const int c = c0 + tx;
  if (st == 0 && c < H4) {
    const float gi = a.bn[0][c] * (1.0f / sqrtf(a.bn[3][c] + a.eps)), gs = a.bn[4][c] * (1.0f / sqrtf(a.bn[7][c] + a.eps));
    a.bias_f[c] = (a.bias[c] + fmaf(-gi, a.bn[2][c], a.bn[1][c])) + fmaf(-gs, a.bn[6][c], a.bn[5][c]);
  }
  if (st == 1 && c < a.H) {
    const float gc = a.bn[8][c] * (1.0f / sqrtf(a.bn[11][c] + a.eps));
    a.ca[c] = gc;
    a.cb[c] = fmaf(-gc, a.bn[10][c], a.bn[9][c]);
  }
}

}  // namespace

bool bnl_supported(int B) { return B >= 1 && B <= BNL_MAXB; }

void launch_bnl_bn_in(const BnlLayer& a, const float* zx, int T, hipStream_t s) {
  hipLaunchKernelGGL(k_bnl_bn_in, dim3((4 * a.H + 63) / 64, T), dim3(64), 0, s, a, zx, T);
}
void launch_bnl_cell_fwd(const BnlLayer& a, int t, hipStream_t s) {
  hipLaunchKernelGGL(k_bnl_cell_fwd, dim3((a.H + BNL_U - 1) / BNL_U), dim3(256), 0, s, a, t);
}
void launch_bnl_proj(const BnlLayer& a, int t, hipStream_t s) {
  hipLaunchKernelGGL(k_bnl_proj, dim3((a.P + BNL_PC - 1) / BNL_PC), dim3(256), 0, s, a, t);
}
void launch_bnl_ema(const BnlLayer& a, int T, float decay, hipStream_t s) {
  hipLaunchKernelGGL(k_bnl_ema, dim3((a.nst + 255) / 256), dim3(256), 0, s, a, T, decay);
}
void launch_bnl_cell_bwd(const BnlLayer& a, int t, hipStream_t s) {
  hipLaunchKernelGGL(k_bnl_cell_bwd, dim3((a.H + BNL_U - 1) / BNL_U), dim3(256), 0, s, a, t);
}
void launch_bnl_dm(const BnlLayer& a, int t, hipStream_t s) {
  hipLaunchKernelGGL(k_bnl_dm, dim3((a.P + BNL_PC - 1) / BNL_PC), dim3(1024), 0, s, a, t);
}
void launch_bnl_fold(const BnlFold& a, hipStream_t s) {
  const int ld = a.ldI > a.ldP ? a.ldI : a.ldP;
  hipLaunchKernelGGL(k_bnl_fold, dim3((4 * a.H + 31) / 32, (ld + 31) / 32, 2), dim3(256), 0, s, a);
}
void launch_bnl_bn_in_bwd(const BnlLayer& a, float* dzx, int T, hipStream_t s) {
  hipLaunchKernelGGL(k_bnl_bn_in_bwd, dim3((4 * a.H + 63) / 64, T), dim3(64), 0, s, a, dzx, T);
}
}  // namespace rsr
