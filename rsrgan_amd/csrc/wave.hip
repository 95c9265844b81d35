// wave.hip -- the waveform front end on the device: PCM samples -> log-power-spectrum frames (the 257-dim LPS every entry point of the
// library starts from; the reference's README names Kaldi's compute-spectrogram-feats with a Hamming window as their source).  The
// definition is the one stated at rsrgan_feat_wave in include/rsrgan.h: snip-edges framing (N samples every S), per frame the mean is
// removed, E = log(max(sum v^2, eps)) is taken, then pre-emphasis, the caller's window table, zero padding to P, |DFT_P|^2, log; bin 0
// carries E.  fp32 throughout.
// Work: a workgroup (256 threads, four wavefronts) takes a run of F consecutive frames of ONE utterance (F = wave_frames(P): 8 up to
// P = 1024, 2 above), so the overlapping span of (F - 1) * S + N samples is read from global memory once, widened to float, into LDS.
// Workgroups find their (utterance, run) by walking the two tables, as k_feat_decode does: the host knows no frame count, only that the
// runs of utterances that lie in `out` without overlap number at most ceil(out_rows / F) + B.
// A wavefront owns one frame at a time.  The real FFT of length P is a complex FFT of length H = P / 2 on z[j] = v[2j] + i v[2j + 1]
// followed by the split pass X_k = E_k + W_P^k O_k.  The complex FFT is decimation in frequency, in place in LDS, radix 4 while the
// sub-length is at least 4 and one radix-2 stage when log2(H) is odd: H = 256 is four radix-4 stages of 64 butterflies, one per lane.
// The result lies digit-reversed; the split pass reads it through fft_pos.  Twiddles come from the caller's table
// tw[j] = exp(-2 pi i j / P), j < H (fp64 on the host, rounded once; staged in LDS), the second half of the circle by negation: no sincosf,
// so a frame has the same bits whatever the launch shape.  The two sums (mean, energy) run in a fixed order: lane l adds samples
// l, l + 64, ... ascending, then a xor-butterfly over the lanes.
// LDS banks (MI355X: an 8-byte read is served per 32-lane half, 64 dword banks, so the 32 float2 indices of a half must differ mod 32).
// The butterflies of stage s touch float2 indices of stride H / 4^s: unswizzled, stage 2 is a 2-way and stages 3 and 4 (strides 4 and 1
// with four elements per lane: the lanes of a half then agree in index bits 2-3 / 0-1) are 4-way conflicts.  fft_sw folds index bit 5 into
// bits 0 and 2 and bit 6 into bits 1, 3 and 4; for H = 256 every stage's reads are then conflict-free (stage by stage: the 32 lanes of a half
// vary bits {0-4}, {0-3, 6}, {0, 1, 4-6}, {2-6}, and the swizzled low five bits are a bijection of each set).  The 8-byte stores are served
// per 16 lanes on 32 banks and stay 2-way conflicted in the last stage; they are bound by the register transfer, not by the array.
// Memory safety: the segment start is clamped into [0, n_samples], its count into what is left, every sample index into [0, n_samples),
// every output row into [0, out_rows); an utterance writes min(F_b, offsets[b + 1] - offsets[b], out_rows) rows and rows of no utterance
// are not written.  The int16 samples are read one by one (an utterance starts at any sample).  No atomics, no traffic between
// workgroups, no scratch memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "kernels.h"

namespace rsr {

constexpr int WAVE_WAVES = 4;

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

template <bool F32>
__device__ __forceinline__ float wave_sample(const void* __restrict__ pcm, long long i) {
  return F32 ? reinterpret_cast<const float*>(pcm)[i] : (float)reinterpret_cast<const short*>(pcm)[i];
}

// PT: the padded length at compile time (the fast path, 512), or 0: P is the argument
template <int PT, bool F32>
__global__ __launch_bounds__(256) void k_feat_wave(const void* __restrict__ pcm, long long n_samples, const long long* __restrict__ seg,
                                                    const int* __restrict__ offsets, int B, uint32_t N, uint32_t S, uint32_t Prt, float preemph,
                                                    const float* __restrict__ window, const float* __restrict__ twiddle, float* __restrict__ out,
                                                    long long out_rows, unsigned long long runs, uint32_t F) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const uint32_t P = PT ? (uint32_t)PT : Prt, H = P >> 1, NB = H + 1;
  const uint32_t nz = min((uint32_t)WAVE_WAVES, F);                  // frames in flight: one buffer per working wavefront
  float2* tw = reinterpret_cast<float2*>(lds_raw);                   // [H]
  float2* zall = tw + H;                                             // [nz][H]
  float* win = reinterpret_cast<float*>(zall + (size_t)nz * H);      // [N]
  float* smp = win + N;                                              // [(F - 1) * S + N]
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t i = tid; i < H; i += 256) tw[i] = make_float2(twiddle[2 * i], twiddle[2 * i + 1]);      // (the table is 4-byte aligned)
  for (uint32_t i = tid; i < N; i += 256) win[i] = window[i];
  float2* z = zall + (size_t)min(wave, nz - 1) * H;
  for (unsigned long long w = blockIdx.x; w < runs; w += gridDim.x) {
    // which utterance run w belongs to (uniform over the workgroup)
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
    if (b == B) break;                                                // (w grows: no later run of this workgroup exists either)
    const long long f0 = (long long)(w - first) * F, off = offsets[b];
    const uint32_t nf = (uint32_t)min((long long)F, rows - f0);
    __syncthreads();                                                  // (the run before is done with smp; tw and win are complete)
    {
      const long long g0 = s0 + f0 * (long long)S;
      const uint32_t span = (nf - 1) * S + N;
      for (uint32_t i = tid; i < span; i += 256) smp[i] = wave_sample<F32>(pcm, min(max(g0 + (long long)i, 0ll), n_samples - 1));
    }
    __syncthreads();
    for (uint32_t it = 0; it < F; it += nz) {
      const uint32_t fl = it + wave;
      const bool live = wave < nz && fl < nf;
      const float* x = smp + (live ? fl * S : 0u);
      // 1, 2: the mean and the raw energy
      float s = 0.f;
      for (uint32_t i = lane; i < N; i += 64) s += x[i];
      const float mean = wave_sum(s) / (float)N;
      float e = 0.f;
      for (uint32_t i = lane; i < N; i += 64) { const float v = x[i] - mean; e += v * v; }
      const float energy = logf(fmaxf(wave_sum(e), FLT_EPSILON));
      // 3, 4, 5: pre-emphasis, window, zero padding; two real samples are one complex element
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
      uint32_t L = H;
      for (; L >= 4; L >>= 2) {
        const uint32_t q = L >> 2, step = P / L;
        if (live) {
          for (uint32_t t = lane; t < (H >> 2); t += 64) {
            const uint32_t k = t & (q - 1), base = (t - k) * 4 + k;   // block * L + k
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
      // the split pass, |X_k|^2 and the log; consecutive lanes write consecutive bins of the row
      if (live) {
        const long long row = min(max(off + f0 + (long long)fl, 0ll), out_rows - 1);
        float* o = out + (size_t)row * NB;
        for (uint32_t k = lane; k <= H; k += 64) {
          const float2 a = z[fft_sw(fft_pos(k & (H - 1), H))], c = z[fft_sw(fft_pos((H - k) & (H - 1), H))];
          const float2 ev = make_float2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y));         // (Z_k + conj Z_{H-k}) / 2
          const float2 od = make_float2(0.5f * (a.y + c.y), -0.5f * (a.x - c.x));        // -i (Z_k - conj Z_{H-k}) / 2
          const float2 r = cmul(od, tw_at(tw, k, H));
          const float re = ev.x + r.x, im = ev.y + r.y;
          o[k] = k == 0 ? energy : logf(fmaxf(re * re + im * im, FLT_EPSILON));
        }
      }
      __syncthreads();                                                // (z is rewritten by this wavefront's next frame)
    }
  }
}

int wave_frames(int P) { return P <= 1024 ? 8 : 2; }

void launch_feat_wave(const void* pcm, int kind, long long n_samples, const long long* seg, const int* offsets, int B, int N, int S, int P,
                      float preemph, const float* window, const float* twiddle, float* out, long long out_rows, hipStream_t s) {
  const int F = wave_frames(P), H = P / 2, nz = std::min(WAVE_WAVES, F);
  const unsigned long long runs = ((unsigned long long)out_rows + F - 1) / F + (unsigned long long)B;
  const int grid = (int)std::min<unsigned long long>(16384, runs);
  // twiddles, the wavefronts' buffers, the window, the samples of a run: 16.4 KB for 400 / 160 / 512, at most 56 KB (P = 1024, N = S = P)
  const size_t lds = (size_t)(H + nz * H) * sizeof(float2) + (size_t)(N + (F - 1) * S + N) * sizeof(float);
#define RSR_WAVE_LAUNCH(PT, F32) \
  hipLaunchKernelGGL((k_feat_wave<PT, F32>), dim3(grid), dim3(256), lds, s, pcm, n_samples, seg, offsets, B, (uint32_t)N, (uint32_t)S, (uint32_t)P, \
                     preemph, window, twiddle, out, out_rows, runs, (uint32_t)F)
  if (P == 512) { if (kind) RSR_WAVE_LAUNCH(512, true); else RSR_WAVE_LAUNCH(512, false); }
  else { if (kind) RSR_WAVE_LAUNCH(0, true); else RSR_WAVE_LAUNCH(0, false); }
#undef RSR_WAVE_LAUNCH
}

}  // namespace rsr
