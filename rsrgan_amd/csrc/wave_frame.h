// wave_frame.h -- the frame helpers of the waveform kernels (wave.hip k_feat_wave / k_feat_mfcc, synth.hip k_synth_frames): finding a
// workgroup's run of frames, staging its samples, the mean, and pre-emphasis + window + padding into the FFT buffer.  The reasoning is
// at the head of wave.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wave_fft.h"

namespace rsr {

constexpr int WAVE_WAVES = 4;

template <bool F32>
__device__ __forceinline__ float wave_sample(const void* __restrict__ pcm, long long i) {
  return F32 ? reinterpret_cast<const float*>(pcm)[i] : (float)reinterpret_cast<const short*>(pcm)[i];
}

// run w of the launch: which utterance it belongs to, where its samples and rows start (uniform over the workgroup)
struct WaveRun {
  long long s0, off, f0;       // the utterance's first sample (clamped), its first row, the run's first frame
  uint32_t nf;                 // frames of the run, 1 .. F
};

// false: run w does not exist (w grows: no later run of this workgroup exists either)
__device__ __forceinline__ bool wave_find_run(unsigned long long w, const long long* __restrict__ seg, const int* __restrict__ offsets, int B,
                                              long long n_samples, uint32_t N, uint32_t S, long long out_rows, uint32_t F, WaveRun& r) {
  int b = 0;
  unsigned long long first = 0;
  long long rows = 0, s0 = 0, cnt = 0;
  for (; b < B; ++b) {
    s0 = min(max(seg[2 * (size_t)b], 0ll), n_samples);
    cnt = min(max(seg[2 * (size_t)b + 1], 0ll), n_samples - s0);
    const long long frames = cnt < (long long)N ? 0ll : 1 + (cnt - (long long)N) / (long long)S;
    rows = min(min(frames, max((long long)offsets[b + 1] - (long long)offsets[b], 0ll)), out_rows);
    const unsigned long long t = ((unsigned long long)rows + F - 1) / F;
    if (w < first + t) break;
    first += t;
  }
  if (b == B) return false;
  r.s0 = s0;
  r.f0 = (long long)(w - first) * F;
  r.off = offsets[b];
  r.nf = (uint32_t)min((long long)F, rows - r.f0);
  return true;
}

// the samples of a run, widened to float, into smp; a workgroup barrier on either side
template <bool F32>
__device__ __forceinline__ void wave_stage_run(float* smp, const void* __restrict__ pcm, long long n_samples, const WaveRun& r, uint32_t N,
                                               uint32_t S, uint32_t tid) {
  __syncthreads();                                                    // (the run before is done with smp; the staged tables are complete)
  const long long g0 = r.s0 + r.f0 * (long long)S;
  const uint32_t span = (r.nf - 1) * S + N;
  for (uint32_t i = tid; i < span; i += 256) smp[i] = wave_sample<F32>(pcm, min(max(g0 + (long long)i, 0ll), n_samples - 1));
  __syncthreads();
}

// 1: the mean of a frame
__device__ __forceinline__ float wave_mean(const float* x, uint32_t N, uint32_t lane) {
  float s = 0.f;
  for (uint32_t i = lane; i < N; i += 64) s += x[i];
  return wave_sum(s) / (float)N;
}

// 3, 4, 5: pre-emphasis, window, zero padding; two real samples are one complex element.  Ends in a workgroup barrier.
__device__ __forceinline__ void wave_load_frame(float2* z, const float* x, float mean, float preemph, const float* win, uint32_t N, uint32_t H,
                                                uint32_t lane, bool live) {
  for (uint32_t j = lane; j < H; j += 64) {
    float v[2];
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      const uint32_t i = 2 * j + h;
      v[h] = 0.f;
      if (i < N) {
        const float cur = x[i] - mean, prev = x[i ? i - 1 : 0u] - mean;
        v[h] = (cur - preemph * prev) * win[i];
      }
    }
    if (live) z[fft_sw(j)] = make_float2(v[0], v[1]);
  }
  __syncthreads();
}

}  // namespace rsr
