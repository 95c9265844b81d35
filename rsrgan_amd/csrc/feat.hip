// feat.hip -- the feature front end of the sequence recipes on the device: global CMVN (io_funcs/make_tfrecords.py:84-87), Kaldi-style
// splicing (io_funcs/tfrecords_io.py:177-203) and zero padding to T (io_funcs/tfrecords_dataset.py:139-175) in ONE launch, from packed
// raw utterances.  With C = left + 1 + right, Dout = D * C and n_b = offsets[b + 1] - offsets[b]:
//   out[b, t, c * D + d] = norm(raw[offsets[b] + clamp(t + c - left, 0, n_b - 1), d])     t < min(n_b, T)
//   out[b, t, :]         = 0                                                              t >= min(n_b, T) (every t when n_b <= 0)
//   lengths[b]           = min(max(n_b, 0), T)
//   norm(v)              = mean ? (float)(((double)v - mean[d]) / stddev[d]) : v
// The arithmetic is the host path's (io/features.py apply_cmvn: float64 subtraction and division, ONE rounding to float32), so the
// result has the host path's bits: plain IEEE operations on double, nothing to contract, no reciprocal.  This file is never compiled with
// -ffast-math.
// Layout: Dout (2827 in the recipes) is no multiple of 4, so rows of `out` are not 16-byte aligned; `out` is treated as ONE flat, 16-byte
// aligned array of B * T * Dout floats.  A lane owns four consecutive flat elements, derives (b, t, c, d) of the first by division and of
// the next three by carrying, and issues one 16-byte store; the last (B * T * Dout) % 4 elements are stored one by one.  Grid-stride, at
// most 2048 workgroups of 256.  The flat index is 64 bits wide where it is an address or a loop counter; it is below 2^32 (the entry's
// limit), so the divisions are 32-bit.  Source rows are clamped into [0, raw_rows): whatever the offset table holds, no lane reads
// outside raw.  No atomics, no LDS, no scratch memory.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace rsr {

struct FeatPos { uint32_t b, t, c, d; };

__device__ __forceinline__ FeatPos feat_pos(uint32_t e, uint32_t T, uint32_t D, uint32_t Dout) {
  const uint32_t r = e / Dout, col = e - r * Dout;
  FeatPos p;
  p.b = r / T; p.t = r - p.b * T; p.c = col / D; p.d = col - p.c * D;
  return p;
}

// the source row of (b, t, c): a pointer to its D floats, or null where the output row is zero (t >= n; every t when n <= 0).  Worked out once per
// (b, t, c), not once per element: a quad changes it only where it crosses a context boundary.
__device__ __forceinline__ const float* feat_row(const float* __restrict__ raw, long long raw_rows, long long off, long long n, const FeatPos& p,
                                                 int left, uint32_t D) {
  if ((long long)p.t >= n) return nullptr;
  const long long j = min(max((long long)p.t + (long long)p.c - left, 0ll), n - 1);      // clamped at the utterance's own first and last frame
  const long long row = min(max(off + j, 0ll), raw_rows - 1);         // memory safety, whatever offsets holds
  return raw + (size_t)row * D;
}

template <bool NORM>
__device__ __forceinline__ float feat_value(const float* __restrict__ src, uint32_t d, const double* __restrict__ mean,
                                            const double* __restrict__ stddev) {
#pragma clang fp contract(off)
  if (!src) return 0.f;
  const float v = src[d];
  if (!NORM) return v;
  const double c = (double)v - mean[d];
  return (float)(c / stddev[d]);
}

template <bool NORM>
__global__ __launch_bounds__(256) void k_feat_batch(const float* __restrict__ raw, long long raw_rows, const int* __restrict__ offsets, int B,
                                                    uint32_t T, uint32_t D, int left, uint32_t C, const double* __restrict__ mean,
                                                    const double* __restrict__ stddev, float* __restrict__ out, int* __restrict__ lengths,
                                                    unsigned long long total) {
  const uint32_t Dout = D * C;
  const unsigned long long gid = (unsigned long long)blockIdx.x * 256 + threadIdx.x, stride = (unsigned long long)gridDim.x * 256;
  if (lengths) {
    for (unsigned long long b = gid; b < (unsigned long long)B; b += stride)
      lengths[b] = (int)min(max((long long)offsets[b + 1] - (long long)offsets[b], 0ll), (long long)T);
  }
  const unsigned long long quads = total >> 2;
  for (unsigned long long q = gid; q < quads; q += stride) {
    FeatPos p = feat_pos((uint32_t)(q << 2), T, D, Dout);             // (total < 2^32)
    long long off = offsets[p.b];
    long long n = (long long)offsets[p.b + 1] - off;
    const float* src = feat_row(raw, raw_rows, off, n, p, left, D);
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = feat_value<NORM>(src, p.d, mean, stddev);
      if (i == 3) break;
      if (++p.d == D) {
        p.d = 0;
        if (++p.c == C) {
          p.c = 0;
          if (++p.t == T) {                                           // (a quad never runs past the last row: 4 q + 3 < total)
            p.t = 0; ++p.b;
            off = offsets[p.b]; n = (long long)offsets[p.b + 1] - off;
          }
        }
        src = feat_row(raw, raw_rows, off, n, p, left, D);
      }
    }
    *reinterpret_cast<float4*>(out + (q << 2)) = make_float4(v[0], v[1], v[2], v[3]);
  }
  const uint32_t tail = (uint32_t)(total & 3);
  if (gid < tail) {
    const unsigned long long e = (quads << 2) + gid;
    const FeatPos p = feat_pos((uint32_t)e, T, D, Dout);
    const long long off = offsets[p.b];
    out[e] = feat_value<NORM>(feat_row(raw, raw_rows, off, (long long)offsets[p.b + 1] - off, p, left, D), p.d, mean, stddev);
  }
}

void launch_feat_batch(const float* raw, long long raw_rows, const int* offsets, int B, int T, int D, int left, int right, const double* mean,
                       const double* stddev, float* out, int* lengths, hipStream_t s) {
  const int C = left + 1 + right;
  const unsigned long long total = (unsigned long long)B * T * D * C;
  // (one workgroup at least: the tail and the lengths are written by the first lanes of the grid, grid-stride over B)
  const int grid = (int)std::min<unsigned long long>(2048, std::max<unsigned long long>(1, ((total >> 2) + 255) / 256));
  if (mean)
    hipLaunchKernelGGL(k_feat_batch<true>, dim3(grid), dim3(256), 0, s, raw, raw_rows, offsets, B, (uint32_t)T, (uint32_t)D, left, (uint32_t)C, mean,
                       stddev, out, lengths, total);
  else
    hipLaunchKernelGGL(k_feat_batch<false>, dim3(grid), dim3(256), 0, s, raw, raw_rows, offsets, B, (uint32_t)T, (uint32_t)D, left, (uint32_t)C, mean,
                       stddev, out, lengths, total);
}

// ---- the frame-level recipes' front end: gather spliced frames from a device-resident pool of utterances.  picks [N][3] = (row, lo, hi): pool
// row of the drawn frame and the pool row range [lo, hi) of its utterance.  With C = left + 1 + right, Dout = D * C:
//   out[i, c * D + d] = norm(pool[clamp(clamp(row + c - left, lo, hi - 1), 0, pool_rows - 1), d])     hi > lo
//   out[i, :]         = +0.0                                                                          hi <= lo
// The same layout as k_feat_batch: `out` is one flat 16-byte aligned array of N * Dout floats, a lane owns four consecutive elements and
// issues one 16-byte store, the last (N * Dout) % 4 elements are stored one by one, grid-stride, at most 2048 workgroups of 256.  The pick
// triple is read where a quad starts and where it crosses into the next pick; the source row is worked out once per (i, c).  The outer clamp
// is memory safety: whatever the table holds, no lane reads outside pool.  No atomics, no LDS, no scratch memory.
struct FramePos { uint32_t i, c, d; };

__device__ __forceinline__ FramePos frame_pos(uint32_t e, uint32_t D, uint32_t Dout) {
  FramePos p;
  p.i = e / Dout;
  const uint32_t col = e - p.i * Dout;
  p.c = col / D; p.d = col - p.c * D;
  return p;
}

struct FramePick { int row, lo, hi; };

__device__ __forceinline__ FramePick frame_pick(const int* __restrict__ picks, uint32_t i) {
  const int* t = picks + (size_t)i * 3;
  FramePick k;
  k.row = t[0]; k.lo = t[1]; k.hi = t[2];
  return k;
}

// the source row of (pick, c): a pointer to its D floats, or null where the output row is zero (hi <= lo)
__device__ __forceinline__ const float* frame_row(const float* __restrict__ pool, long long pool_rows, const FramePick& k, uint32_t c, int left,
                                                  uint32_t D) {
  if (k.hi <= k.lo) return nullptr;
  const long long j = min(max((long long)k.row + (long long)c - left, (long long)k.lo), (long long)k.hi - 1);      // the utterance's own first and last frame
  const long long row = min(max(j, 0ll), pool_rows - 1);              // memory safety, whatever picks holds
  return pool + (size_t)row * D;
}

template <bool NORM>
__global__ __launch_bounds__(256) void k_feat_frames(const float* __restrict__ pool, long long pool_rows, const int* __restrict__ picks, uint32_t D,
                                                     int left, uint32_t C, const double* __restrict__ mean, const double* __restrict__ stddev,
                                                     float* __restrict__ out, unsigned long long total) {
  const uint32_t Dout = D * C;
  const unsigned long long gid = (unsigned long long)blockIdx.x * 256 + threadIdx.x, stride = (unsigned long long)gridDim.x * 256;
  const unsigned long long quads = total >> 2;
  for (unsigned long long q = gid; q < quads; q += stride) {
    FramePos p = frame_pos((uint32_t)(q << 2), D, Dout);              // (total < 2^32)
    FramePick k = frame_pick(picks, p.i);
    const float* src = frame_row(pool, pool_rows, k, p.c, left, D);
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = feat_value<NORM>(src, p.d, mean, stddev);
      if (i == 3) break;
      if (++p.d == D) {
        p.d = 0;
        if (++p.c == C) {                                             // (a quad never runs past the last pick: 4 q + 3 < total)
          p.c = 0; ++p.i;
          k = frame_pick(picks, p.i);
        }
        src = frame_row(pool, pool_rows, k, p.c, left, D);
      }
    }
    *reinterpret_cast<float4*>(out + (q << 2)) = make_float4(v[0], v[1], v[2], v[3]);
  }
  const uint32_t tail = (uint32_t)(total & 3);
  if (gid < tail) {
    const unsigned long long e = (quads << 2) + gid;
    const FramePos p = frame_pos((uint32_t)e, D, Dout);
    out[e] = feat_value<NORM>(frame_row(pool, pool_rows, frame_pick(picks, p.i), p.c, left, D), p.d, mean, stddev);
  }
}

void launch_feat_frames(const float* pool, long long pool_rows, const int* picks, int N, int D, int left, int right, const double* mean,
                        const double* stddev, float* out, hipStream_t s) {
  const int C = left + 1 + right;
  const unsigned long long total = (unsigned long long)N * D * C;
  // (one workgroup at least: the tail is written by the first lanes of the grid)
  const int grid = (int)std::min<unsigned long long>(2048, std::max<unsigned long long>(1, ((total >> 2) + 255) / 256));
  if (mean)
    hipLaunchKernelGGL(k_feat_frames<true>, dim3(grid), dim3(256), 0, s, pool, pool_rows, picks, (uint32_t)D, left, (uint32_t)C, mean, stddev, out,
                       total);
  else
    hipLaunchKernelGGL(k_feat_frames<false>, dim3(grid), dim3(256), 0, s, pool, pool_rows, picks, (uint32_t)D, left, (uint32_t)C, mean, stddev, out,
                       total);
}

}  // namespace rsr
