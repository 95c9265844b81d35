// wave_fft.h -- the LDS complex FFT of the waveform kernels (wave.hip k_feat_wave / k_feat_mfcc, reverb.hip): the swizzle, the digit-reversed
// position, the table twiddles and the in-place transform.  The bank reasoning is at the head of wave.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rsr {

__device__ __forceinline__ uint32_t fft_sw(uint32_t e) { return e ^ (((e >> 5) & 1u) * 5u) ^ (((e >> 6) & 1u) * 26u); }

// where frequency f of the H-point transform lies after the in-place stages (digits of f, least significant first, are the stages' outputs)
__device__ __forceinline__ uint32_t fft_pos(uint32_t f, uint32_t H) {
  uint32_t pos = 0, L = H;
  while (L >= 4) { L >>= 2; pos += (f & 3u) * L; f >>= 2; }
  if (L == 2) pos += f & 1u;
  return pos;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// exp(-2 pi i idx / P) for idx < P = 2 H from the table of the first half circle
__device__ __forceinline__ float2 tw_at(const float2* tw, uint32_t idx, uint32_t H) {
  const float2 t = tw[idx & (H - 1)];
  return (idx & H) ? make_float2(-t.x, -t.y) : t;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the H-point complex FFT in place (digit-reversed result); a workgroup barrier after every stage
__device__ __forceinline__ void wave_fft(float2* z, const float2* tw, uint32_t P, uint32_t H, uint32_t lane, bool live) {
  uint32_t L = H;
  for (; L >= 4; L >>= 2) {
    const uint32_t q = L >> 2, step = P / L;
    if (live) {
      for (uint32_t t = lane; t < (H >> 2); t += 64) {
        const uint32_t k = t & (q - 1), base = (t - k) * 4 + k;       // block * L + k
        const float2 a0 = z[fft_sw(base)], a1 = z[fft_sw(base + q)], a2 = z[fft_sw(base + 2 * q)], a3 = z[fft_sw(base + 3 * q)];
        const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y), t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
        const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y), t3 = make_float2(a1.x - a3.x, a1.y - a3.y);
        float2 y0 = make_float2(t0.x + t2.x, t0.y + t2.y), y2 = make_float2(t0.x - t2.x, t0.y - t2.y);
        float2 y1 = make_float2(t1.x + t3.y, t1.y - t3.x), y3 = make_float2(t1.x - t3.y, t1.y + t3.x);
        if (q > 1) {
          y1 = cmul(y1, tw_at(tw, k * step, H));
          y2 = cmul(y2, tw_at(tw, 2 * k * step, H));
          y3 = cmul(y3, tw_at(tw, 3 * k * step, H));
        }
        z[fft_sw(base)] = y0; z[fft_sw(base + q)] = y1; z[fft_sw(base + 2 * q)] = y2; z[fft_sw(base + 3 * q)] = y3;
      }
    }
    __syncthreads();
  }
  if (L == 2) {
    if (live) {
      for (uint32_t t = lane; t < (H >> 1); t += 64) {
        const float2 a0 = z[fft_sw(2 * t)], a1 = z[fft_sw(2 * t + 1)];
        z[fft_sw(2 * t)] = make_float2(a0.x + a1.x, a0.y + a1.y);
        z[fft_sw(2 * t + 1)] = make_float2(a0.x - a1.x, a0.y - a1.y);
      }
    }
    __syncthreads();
  }
}

}  // namespace rsr
