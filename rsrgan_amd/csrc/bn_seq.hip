// bn_seq.hip -- batch_norm(is_training, scale=True, renorm=True) + leaky-ReLU on the sequence path: the generator's input layer
// leakyrelu(batch_norm(x.W)) of models/lstm.py:61-87.  The algorithm is bn.hip's (oracle/bn_renorm.py); two things differ:
//   * the activation has a negative slope alpha (bn.hip knows ReLU only);
//   * the operand is the time-major [T*Bp][ld] tensor of a padded batch: every group of Bp rows is Bt caller rows and Bp - Bt padding
//     rows of the library's own.  Row r counts iff Bp == 0 || r % Bp < Bt; n = the number of counted rows.  The moments and the
//     backward sums run over the counted rows, y and dz come out as exact zeros on the others whatever z / dy hold there.
// Two launches per direction (the chain they sit on is launch-latency-bound):
//   forward   k_bnq_part<false> (row-slice partial sums of z - z0, z0 = row 0, the first counted row) -> k_bnq_fwd: every workgroup
//             finishes the moments of ITS 64 columns from the slice partials (double, fixed order: the arithmetic of k_bn_stats2), then
//             applies y = leaky(z*a + b) to its rows.  All workgroups of a column block compute the same bits; the first row
//             block writes stat.  training = false: k_bnq_fwd alone, a and b from the moving statistics.
//   backward  k_bnq_part<true> (partials of sum dy', sum dy'.xhat, dy' = dy.(y > 0 ? 1 : alpha)) -> k_bnq_bwd (finishes the sums,
//             the first row block writes dbeta / dgamma / sums, then dz in place over dy).
// No atomics; every sum has a fixed order given (rows, cols, scratch_floats), so results are bit-reproducible.  16-byte loads and
// stores throughout: a thread owns one quad column, 16 quad lanes x 16 row lanes per workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace rsr {

constexpr float BNQ_EPS = 1e-3f;            // contrib.layers.batch_norm epsilon (bn.hip BN_EPS)
constexpr int BNQ_MAX_SLICES = 32;          // 2 x 32 x cols floats of partials: within the 64 x cols floats every model scratch holds

__device__ __forceinline__ float4 bnq_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ bool bnq_counted(int r, int Bp, int Bt) { return Bp == 0 || r % Bp < Bt; }
__device__ __forceinline__ float bnq_affine(float z, float a, float b) {      // z*a + b with the product rounded (see k_bnq_fwd)
#pragma clang fp contract(off)
  const float p = z * a;
  return p + b;
}
__device__ __forceinline__ float bnq_slope(float g, float y, float alpha) { return y > 0.f ? g : g * alpha; }

// partial sums of one row slice over the counted rows: scratch[slice][2][cols]
//   forward : sum (z - z0), sum (z - z0)^2 ; backward: sum dy', sum dy'.xhat
template <bool BWD>
__global__ __launch_bounds__(256) void k_bnq_part(const float* __restrict__ z, int ldz, const float* __restrict__ dy, int ldd,
                                                  const float* __restrict__ y, int ldy, const float* __restrict__ stat, int ldc, int rows,
                                                  int cols, int per, int Bp, int Bt, int act, float alpha, float* __restrict__ scratch) {
  __shared__ float red[2][16][64];
  const int ql = threadIdx.x & 15, rl = threadIdx.x >> 4, c = blockIdx.x * 64 + ql * 4;
  const int cp = (cols + 3) & ~3;
  const int rbeg = blockIdx.y * per, rend = min(rows, rbeg + per);
  float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
  if (c < cp) {
    float4 m, k;                              // forward: m = row 0 (the shift); backward: m = mean, k = 1 / stddev (0 in padding columns)
    if (BWD) {
      m = bnq_ld4(stat + c);
      const float4 sd = bnq_ld4(stat + ldc + c);
      k = make_float4(sd.x > 0.f ? 1.f / sd.x : 0.f, sd.y > 0.f ? 1.f / sd.y : 0.f, sd.z > 0.f ? 1.f / sd.z : 0.f, sd.w > 0.f ? 1.f / sd.w : 0.f);
    } else {
      m = bnq_ld4(z + c); k = m;
    }
#pragma unroll 4
    for (int r = rbeg + rl; r < rend; r += 16) {
      if (!bnq_counted(r, Bp, Bt)) continue;
      const float4 zv = bnq_ld4(z + (size_t)r * ldz + c);
      if (BWD) {
        float4 g = bnq_ld4(dy + (size_t)r * ldd + c);
        if (act) {
          const float4 yv = bnq_ld4(y + (size_t)r * ldy + c);
          g = make_float4(bnq_slope(g.x, yv.x, alpha), bnq_slope(g.y, yv.y, alpha), bnq_slope(g.z, yv.z, alpha), bnq_slope(g.w, yv.w, alpha));
        }
        s1.x += g.x; s1.y += g.y; s1.z += g.z; s1.w += g.w;
        s2.x += g.x * ((zv.x - m.x) * k.x); s2.y += g.y * ((zv.y - m.y) * k.y);
        s2.z += g.z * ((zv.z - m.z) * k.z); s2.w += g.w * ((zv.w - m.w) * k.w);
      } else {
        const float vx = zv.x - m.x, vy = zv.y - m.y, vz = zv.z - m.z, vw = zv.w - m.w;
        s1.x += vx; s1.y += vy; s1.z += vz; s1.w += vw;
        s2.x += vx * vx; s2.y += vy * vy; s2.z += vz * vz; s2.w += vw * vw;
      }
    }
  }
  *reinterpret_cast<float4*>(&red[0][rl][ql * 4]) = s1; *reinterpret_cast<float4*>(&red[1][rl][ql * 4]) = s2;
  __syncthreads();
  if (threadIdx.x < 128) {
    const int which = threadIdx.x >> 6, l = threadIdx.x & 63, cc = blockIdx.x * 64 + l;
    if (cc < cols) {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) t += red[which][i][l];
      scratch[((size_t)blockIdx.y * 2 + which) * cols + cc] = t;
    }
  }
}

// the slice partials of this workgroup's 64 columns, summed in double by four threads per column and combined in a fixed order
// (k_bn_stats2's order).  Every thread calls it; the result is valid in threads 0 .. 63 (column blockIdx.x * 64 + threadIdx.x).
__device__ __forceinline__ void bnq_finish(const float* __restrict__ scratch, int slices, int cols, double (*red2)[4][64], double& s1, double& s2) {
  const int l = threadIdx.x & 63, sl = threadIdx.x >> 6, c = blockIdx.x * 64 + l;
  double p1 = 0.0, p2 = 0.0;
  if (c < cols) {
#pragma unroll 8
    for (int i = sl; i < slices; i += 4) { p1 += scratch[((size_t)i * 2) * cols + c]; p2 += scratch[((size_t)i * 2 + 1) * cols + c]; }
  }
  red2[0][sl][l] = p1; red2[1][sl][l] = p2;
  __syncthreads();
  s1 = ((red2[0][0][l] + red2[0][1][l]) + red2[0][2][l]) + red2[0][3][l];
  s2 = ((red2[1][0][l] + red2[1][1][l]) + red2[1][2][l]) + red2[1][3][l];
}

// stat rows: 0 mean, 1 stddev, 2 r, 3 d, 4 a, 5 b (y = z*a + b); training = 0 writes rows 4 and 5 only, from the moving statistics
__global__ __launch_bounds__(256) void k_bnq_fwd(const float* __restrict__ scratch, int slices, const float* __restrict__ z, int ldz,
                                                 float* __restrict__ y, int ldy, int rows, int cols, int n, int per, BnVars v,
                                                 float* __restrict__ stat, int ldc, int training, int act, float alpha, int Bp, int Bt) {
  __shared__ double red2[2][4][64];
  __shared__ float ab[2][64];
  double s1 = 0.0, s2 = 0.0;
  if (training) bnq_finish(scratch, slices, cols, red2, s1, s2);
  if (threadIdx.x < 64) {
    const int l = threadIdx.x, c = blockIdx.x * 64 + l;
    float af = 0.f, bf = 0.f;                  // (padding columns: zeros are written, whatever z holds there)
    if (c < cols) {
      if (training) {
        const double m0 = s1 / n;
        const double var = fmax(s2 / n - m0 * m0, 0.0);
        const double mean = (double)z[c] + m0;
        const double sd = sqrt(var + (double)BNQ_EPS);
        const double mixed_mean = (double)v.rm[c] + (1.0 - (double)v.rmw[0]) * mean;
        const double mixed_sd = (double)v.rs[c] + (1.0 - (double)v.rsw[0]) * sd;
        const double r = sd / mixed_sd, d = (mean - mixed_mean) / mixed_sd;
        const double g = v.gamma[c];
        const double a = r * g / sd;
        af = (float)a; bf = (float)(d * g + (double)v.beta[c] - mean * a);
        if (blockIdx.y == 0) { stat[c] = (float)mean; stat[ldc + c] = (float)sd; stat[2 * ldc + c] = (float)r; stat[3 * ldc + c] = (float)d; }
      } else {
        const double a = (double)v.gamma[c] / sqrt((double)v.mv[c] + (double)BNQ_EPS);
        af = (float)a; bf = (float)((double)v.beta[c] - (double)v.mm[c] * a);
      }
      if (blockIdx.y == 0) { stat[4 * ldc + c] = af; stat[5 * ldc + c] = bf; }
    }
    ab[0][l] = af; ab[1][l] = bf;
  }
  __syncthreads();
  const int ql = threadIdx.x & 15, rl = threadIdx.x >> 4, c = blockIdx.x * 64 + ql * 4;
  if (c >= ((cols + 3) & ~3)) return;
  const float4 a = *reinterpret_cast<const float4*>(&ab[0][ql * 4]), b = *reinterpret_cast<const float4*>(&ab[1][ql * 4]);
  const int rbeg = blockIdx.y * per, rend = min(rows, rbeg + per);
#pragma unroll 4
  for (int r = rbeg + rl; r < rend; r += 16) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bnq_counted(r, Bp, Bt)) {
      const float4 zv = bnq_ld4(z + (size_t)r * ldz + c);
      // the product is rounded before the add (no contraction): where the batch has ONE counted row, z = mean and b = fl(-mean.a) (+ d.gamma + beta),
      // so fl(z.a) cancels against b exactly and y = d.gamma + beta as in the reference; a fused multiply-add leaves the product's rounding
      // residual there, 1e-6 of |z.a| beside an exact 0
      o = make_float4(bnq_affine(zv.x, a.x, b.x), bnq_affine(zv.y, a.y, b.y), bnq_affine(zv.z, a.z, b.z), bnq_affine(zv.w, a.w, b.w));
      if (act) o = make_float4(o.x > 0.f ? o.x : o.x * alpha, o.y > 0.f ? o.y : o.y * alpha, o.z > 0.f ? o.z : o.z * alpha, o.w > 0.f ? o.w : o.w * alpha);
      if (c + 3 >= cols) { if (c + 1 >= cols) o.y = 0.f; if (c + 2 >= cols) o.z = 0.f; o.w = 0.f; }      // padding columns: literal zeros
    }
    *reinterpret_cast<float4*>(y + (size_t)r * ldy + c) = o;
  }
}

// dbeta = sum dy', dgamma = r.sum dy'.xhat + d.sum dy' (assigned or accumulated), sums = [s1/n, s2/n], then
// dz = gamma*r/stddev * (dy' - s1/n - xhat*s2/n) in place over dy on the counted rows, 0 on the others.  stat[4] = a = gamma*r/stddev.
__global__ __launch_bounds__(256) void k_bnq_bwd(const float* __restrict__ scratch, int slices, float* __restrict__ dy, int ldd,
                                                 const float* __restrict__ y, int ldy, const float* __restrict__ z, int ldz,
                                                 const float* __restrict__ stat, int ldc, int rows, int cols, int n, int per,
                                                 float* __restrict__ dbeta, float* __restrict__ dgamma, int accumulate, float* __restrict__ sums,
                                                 int act, float alpha, int Bp, int Bt) {
  __shared__ double red2[2][4][64];
  __shared__ float cst[5][64];                 // mean, 1 / stddev, a, s1 / n, s2 / n
  double s1, s2;
  bnq_finish(scratch, slices, cols, red2, s1, s2);
  if (threadIdx.x < 64) {
    const int l = threadIdx.x, c = blockIdx.x * 64 + l;
    float mean = 0.f, isd = 0.f, a = 0.f, m1 = 0.f, m2 = 0.f;      // (padding columns: zeros are written, whatever dy holds there)
    if (c < cols) {
      mean = stat[c]; isd = 1.f / stat[ldc + c]; a = stat[4 * ldc + c];
      m1 = (float)(s1 / n); m2 = (float)(s2 / n);
      if (blockIdx.y == 0) {
        if (dbeta) {
          const double gb = s1, gg = (double)stat[2 * ldc + c] * s2 + (double)stat[3 * ldc + c] * s1;
          dbeta[c] = (float)(accumulate ? (double)dbeta[c] + gb : gb);
          dgamma[c] = (float)(accumulate ? (double)dgamma[c] + gg : gg);
        }
        sums[c] = m1; sums[ldc + c] = m2;
      }
    }
    cst[0][l] = mean; cst[1][l] = isd; cst[2][l] = a; cst[3][l] = m1; cst[4][l] = m2;
  }
  __syncthreads();
  const int ql = threadIdx.x & 15, rl = threadIdx.x >> 4, c = blockIdx.x * 64 + ql * 4;
  if (c >= ((cols + 3) & ~3)) return;
  const float4 mean = *reinterpret_cast<const float4*>(&cst[0][ql * 4]), isd = *reinterpret_cast<const float4*>(&cst[1][ql * 4]);
  const float4 a = *reinterpret_cast<const float4*>(&cst[2][ql * 4]);
  const float4 m1 = *reinterpret_cast<const float4*>(&cst[3][ql * 4]), m2 = *reinterpret_cast<const float4*>(&cst[4][ql * 4]);
  const int rbeg = blockIdx.y * per, rend = min(rows, rbeg + per);
#pragma unroll 4
  for (int r = rbeg + rl; r < rend; r += 16) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bnq_counted(r, Bp, Bt)) {
      float4 g = bnq_ld4(dy + (size_t)r * ldd + c);
      if (act) {
        const float4 yv = bnq_ld4(y + (size_t)r * ldy + c);
        g = make_float4(bnq_slope(g.x, yv.x, alpha), bnq_slope(g.y, yv.y, alpha), bnq_slope(g.z, yv.z, alpha), bnq_slope(g.w, yv.w, alpha));
      }
      const float4 zv = bnq_ld4(z + (size_t)r * ldz + c);
      o.x = a.x * (g.x - m1.x - (zv.x - mean.x) * isd.x * m2.x);
      o.y = a.y * (g.y - m1.y - (zv.y - mean.y) * isd.y * m2.y);
      o.z = a.z * (g.z - m1.z - (zv.z - mean.z) * isd.z * m2.z);
      o.w = a.w * (g.w - m1.w - (zv.w - mean.w) * isd.w * m2.w);
      if (c + 3 >= cols) { if (c + 1 >= cols) o.y = 0.f; if (c + 2 >= cols) o.z = 0.f; o.w = 0.f; }      // padding columns: literal zeros
    }
    *reinterpret_cast<float4*>(dy + (size_t)r * ldd + c) = o;
  }
}

int bn_seq_count(int rows, int Bp, int Bt) { return Bp == 0 ? rows : rows / Bp * Bt + std::min(rows % Bp, Bt); }

static int bnq_slices(int rows, int cols, size_t scratch_floats, int* per) {
  int slices = (int)std::min<size_t>(BNQ_MAX_SLICES, scratch_floats / ((size_t)2 * std::max(cols, 1)));
  slices = std::max(1, std::min(slices, (rows + 63) / 64));
  *per = (rows + slices - 1) / slices;
  return (rows + *per - 1) / *per;
}
static int bnq_row_blocks(int rows, int* per) {          // the elementwise pass: 64 rows per workgroup, at most 512 row blocks
  const int blocks = std::max(1, std::min(512, (rows + 63) / 64));
  *per = (rows + blocks - 1) / blocks;
  return (rows + *per - 1) / *per;
}

void launch_bn_seq_forward(const float* z, int ldz, float* y, int ldy, int rows, int cols, const BnVars& v, float* stat, int ldc, bool training,
                           bool act, float alpha, int Bp, int Bt, float* scratch, size_t scratch_floats, hipStream_t s) {
  const int cb = (cols + 63) / 64, n = bn_seq_count(rows, Bp, Bt);
  int per = 0, slices = 0;
  if (training) {
    slices = bnq_slices(rows, cols, scratch_floats, &per);
    hipLaunchKernelGGL(k_bnq_part<false>, dim3(cb, slices), dim3(256), 0, s, z, ldz, nullptr, 0, nullptr, 0, nullptr, 0, rows, cols, per, Bp, Bt, 0,
                       0.f, scratch);
  }
  int eper;
  const int eb = bnq_row_blocks(rows, &eper);
  hipLaunchKernelGGL(k_bnq_fwd, dim3(cb, eb), dim3(256), 0, s, scratch, slices, z, ldz, y, ldy, rows, cols, n, eper, v, stat, ldc, training ? 1 : 0,
                     act ? 1 : 0, alpha, Bp, Bt);
}

void launch_bn_seq_backward(float* dy, int ldd, const float* y, int ldy, const float* z, int ldz, int rows, int cols, const float* stat, int ldc,
                            float* dbeta, float* dgamma, bool accumulate, bool act, float alpha, int Bp, int Bt, float* sums, float* scratch,
                            size_t scratch_floats, hipStream_t s) {
  const int cb = (cols + 63) / 64, n = bn_seq_count(rows, Bp, Bt);
  int per, eper;
  const int slices = bnq_slices(rows, cols, scratch_floats, &per);
  hipLaunchKernelGGL(k_bnq_part<true>, dim3(cb, slices), dim3(256), 0, s, z, ldz, dy, ldd, y, ldy, stat, ldc, rows, cols, per, Bp, Bt, act ? 1 : 0,
                     alpha, scratch);
  const int eb = bnq_row_blocks(rows, &eper);
  hipLaunchKernelGGL(k_bnq_bwd, dim3(cb, eb), dim3(256), 0, s, scratch, slices, dy, ldd, y, ldy, z, ldz, stat, ldc, rows, cols, n, eper, dbeta, dgamma,
                     accumulate ? 1 : 0, sums, act ? 1 : 0, alpha, Bp, Bt);
}

// RSRGAN_FLAG_INFER: the moving statistics folded into the input FC in place, once per rsrgan_set_params (in the manner of k_bnl_fold):
// W[k][c] *= a[c], bias[c] = b[c] with a = gamma / sqrt(moving_variance + eps), b = beta - moving_mean * a.  One thread per column.
__global__ __launch_bounds__(256) void k_bnq_fold(float* __restrict__ W, int ldw, int K, int cols, BnVars v, float* __restrict__ bias) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  const double a = (double)v.gamma[c] / sqrt((double)v.mv[c] + (double)BNQ_EPS);
  const float af = (float)a;
  bias[c] = (float)((double)v.beta[c] - (double)v.mm[c] * a);
  for (int k = 0; k < K; ++k) W[(size_t)k * ldw + c] *= af;
}
void launch_bn_seq_fold(float* W, int ldw, int K, int cols, const BnVars& v, float* bias, hipStream_t s) {
  hipLaunchKernelGGL(k_bnq_fold, dim3((cols + 255) / 256), dim3(256), 0, s, W, ldw, K, cols, v, bias);
}

}  // namespace rsr
