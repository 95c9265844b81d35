// wave.hip -- the waveform front end on the device: PCM samples -> log-power-spectrum frames (the 257-dim LPS every entry point of the
// library starts from; the reference's README names Kaldi's compute-spectrogram-feats with a Hamming window as their source), and
// PCM samples -> MFCC / log-mel frames (the 40-dim labels: compute-mfcc-feats with mfcc_hires.conf).  The definitions are the ones stated
// at rsrgan_feat_wave and rsrgan_feat_mfcc in include/rsrgan.h: snip-edges framing (N samples every S), per frame the mean is
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
// The two kernels share the frame pipeline as __device__ functions (wave_find_run, wave_stage_run, wave_mean, wave_load_frame, wave_fft,
// wave_power); k_feat_wave adds the raw energy and the log, k_feat_mfcc the mel / cepstral epilogue described in front of it.
// The swizzle, fft_pos, the twiddle lookup and wave_fft itself live in wave_fft.h, which reverb.hip shares; the frame helpers (wave_find_run,
// wave_stage_run, wave_mean, wave_load_frame) in wave_frame.h, which synth.hip shares.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "kernels.h"
#include "wave_fft.h"
#include "wave_frame.h"

namespace rsr {

// the split pass for bin k <= H: p_k = |X_k|^2
__device__ __forceinline__ float wave_power(const float2* z, const float2* tw, uint32_t k, uint32_t H) {
  const float2 a = z[fft_sw(fft_pos(k & (H - 1), H))], c = z[fft_sw(fft_pos((H - k) & (H - 1), H))];
  const float2 ev = make_float2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y));         // (Z_k + conj Z_{H-k}) / 2
  const float2 od = make_float2(0.5f * (a.y + c.y), -0.5f * (a.x - c.x));        // -i (Z_k - conj Z_{H-k}) / 2
  const float2 r = cmul(od, tw_at(tw, k, H));
  const float re = ev.x + r.x, im = ev.y + r.y;
  return re * re + im * im;
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
    WaveRun r;
    if (!wave_find_run(w, seg, offsets, B, n_samples, N, S, out_rows, F, r)) break;
    wave_stage_run<F32>(smp, pcm, n_samples, r, N, S, tid);
    for (uint32_t it = 0; it < F; it += nz) {
      const uint32_t fl = it + wave;
      const bool live = wave < nz && fl < r.nf;
      const float* x = smp + (live ? fl * S : 0u);
      // 1, 2: the mean and the raw energy
      const float mean = wave_mean(x, N, lane);
      float e = 0.f;
      for (uint32_t i = lane; i < N; i += 64) { const float v = x[i] - mean; e += v * v; }
      const float energy = logf(fmaxf(wave_sum(e), FLT_EPSILON));
      wave_load_frame(z, x, mean, preemph, win, N, H, lane, live);
      wave_fft(z, tw, P, H, lane, live);
      // the split pass, |X_k|^2 and the log; consecutive lanes write consecutive bins of the row
      if (live) {
        const long long row = min(max(r.off + r.f0 + (long long)fl, 0ll), out_rows - 1);
        float* o = out + (size_t)row * NB;
        for (uint32_t k = lane; k <= H; k += 64) o[k] = k == 0 ? energy : logf(fmaxf(wave_power(z, tw, k, H), FLT_EPSILON));
      }
      __syncthreads();                                                // (z is rewritten by this wavefront's next frame)
    }
  }
}

// ---- MFCC / log-mel (include/rsrgan.h rsrgan_feat_mfcc): the same pipeline up to p_k, then per frame, by the wavefront that owns it,
//   p     the split pass writes p_k, k < H, into the wavefront's OWN row prow [H] (not over z: the pass reads z[k] and z[H - k], which other
//         lanes of the wavefront still need); the Nyquist bin is not formed
//   mel   lane j (stride 64 for M > 64) sums filter j, t ascending: m_j = sum_t w[w0_j + t] * p[a_j + t]; l_j = log(max(m_j, eps)) -> lrow [M]
//   dct   lane i (stride 64) forms c_i = sum_j dct[i][j] * l_j, j ascending, from dctT [M][C], the table staged TRANSPOSED once per
//         workgroup: lanes i, i + 1, .. read consecutive dwords (no conflict) and l_j is one address for all lanes (a broadcast)
// A workgroup barrier separates the three steps (the loop is uniform over the workgroup, as the FFT stages' barriers already demand).
// LDS banks of the mel sums (ds_read_b32: per 32-lane half, bank = dword index mod 32): at step t lane j reads p[a_j + t].  The filters'
// first bins a_j ascend with j but not evenly, so two lanes of a half can meet on a bank with different bins.  ENUMERATED for the
// recipe's table (400 / 160 / 512, 40 filters of 3 .. 30 bins; tools/mfcc_bench.py --banks prints the count), not measured: lanes 0 - 31
// are active for 19 steps, lanes 32 - 39 for 30, no step is worse than 2-way, and the 49 half-wave reads take 78 LDS cycles where 49 would
// be conflict-free -- 29 cycles per frame beside the 128 of the four FFT stages' 8-byte reads and stores (4 x (4 x 2 + 4 x 6)), so the row is left unpadded.  The weights
// w[w0_j + t] take 77 cycles for the same 49 reads (worst step 4-way: the short low filters' w0_j lie close together).
// Memory safety: a_j is clamped into [0, H), n_j into [0, H - a_j], every weight index into [0, nnz): the tables are device-resident, the
// host cannot see them, and the kernel reads and writes nothing outside its buffers whatever they hold.
template <int PT, bool F32>
__global__ __launch_bounds__(256) void k_feat_mfcc(const void* __restrict__ pcm, long long n_samples, const long long* __restrict__ seg,
                                                    const int* __restrict__ offsets, int B, uint32_t N, uint32_t S, uint32_t Prt, float preemph,
                                                    const float* __restrict__ window, const float* __restrict__ twiddle,
                                                    const int* __restrict__ mel_seg, const float* __restrict__ mel_w, uint32_t nnz, uint32_t M,
                                                    const float* __restrict__ dct, uint32_t C, float* __restrict__ out, long long out_rows,
                                                    unsigned long long runs, uint32_t F) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const uint32_t P = PT ? (uint32_t)PT : Prt, H = P >> 1, NC = C ? C : M;
  const uint32_t nz = min((uint32_t)WAVE_WAVES, F);
  float2* tw = reinterpret_cast<float2*>(lds_raw);                   // [H]
  float2* zall = tw + H;                                             // [nz][H]
  float* win = reinterpret_cast<float*>(zall + (size_t)nz * H);      // [N]
  float* smp = win + N;                                              // [(F - 1) * S + N]
  float* pall = smp + (F - 1) * S + N;                               // [nz][H]
  float* lall = pall + (size_t)nz * H;                               // [nz][M]
  float* dctT = lall + (size_t)nz * M;                               // [M][C]
  int* mseg = reinterpret_cast<int*>(dctT + (size_t)M * C);          // [M][3]
  float* mw = reinterpret_cast<float*>(mseg + 3 * M);                // [nnz]
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t i = tid; i < H; i += 256) tw[i] = make_float2(twiddle[2 * i], twiddle[2 * i + 1]);
  for (uint32_t i = tid; i < N; i += 256) win[i] = window[i];
  for (uint32_t i = tid; i < M * C; i += 256) { const uint32_t c = i / M, j = i - c * M; dctT[j * C + c] = dct[i]; }
  for (uint32_t i = tid; i < 3 * M; i += 256) mseg[i] = mel_seg[i];
  for (uint32_t i = tid; i < nnz; i += 256) mw[i] = mel_w[i];
  float2* z = zall + (size_t)min(wave, nz - 1) * H;
  float* prow = pall + (size_t)min(wave, nz - 1) * H;
  float* lrow = lall + (size_t)min(wave, nz - 1) * M;
  for (unsigned long long w = blockIdx.x; w < runs; w += gridDim.x) {
    WaveRun r;
    if (!wave_find_run(w, seg, offsets, B, n_samples, N, S, out_rows, F, r)) break;
    wave_stage_run<F32>(smp, pcm, n_samples, r, N, S, tid);
    for (uint32_t it = 0; it < F; it += nz) {
      const uint32_t fl = it + wave;
      const bool live = wave < nz && fl < r.nf;
      const float* x = smp + (live ? fl * S : 0u);
      const float mean = wave_mean(x, N, lane);
      wave_load_frame(z, x, mean, preemph, win, N, H, lane, live);
      wave_fft(z, tw, P, H, lane, live);
      if (live)
        for (uint32_t k = lane; k < H; k += 64) prow[k] = wave_power(z, tw, k, H);
      __syncthreads();
      const long long row = min(max(r.off + r.f0 + (long long)fl, 0ll), out_rows - 1);
      float* o = out + (size_t)row * NC;
      if (live) {
        for (uint32_t j = lane; j < M; j += 64) {
          const uint32_t a = (uint32_t)min(max(mseg[3 * j], 0), (int)H - 1);
          const uint32_t n = (uint32_t)min(max(mseg[3 * j + 1], 0), (int)(H - a));
          const uint32_t w0 = (uint32_t)min(max(mseg[3 * j + 2], 0), (int)nnz - 1);
          float m = 0.f;
          for (uint32_t t = 0; t < n; ++t) m += mw[min(w0 + t, nnz - 1)] * prow[a + t];
          const float l = logf(fmaxf(m, FLT_EPSILON));
          if (C) lrow[j] = l; else o[j] = l;
        }
      }
      if (C) {
        __syncthreads();
        if (live) {
          for (uint32_t i = lane; i < C; i += 64) {
            float c = 0.f;
            for (uint32_t j = 0; j < M; ++j) c += dctT[j * C + i] * lrow[j];
            o[i] = c;
          }
        }
      }
      __syncthreads();                                                // (z, prow and lrow are rewritten by this wavefront's next frame)
    }
  }
}

int wave_frames(int P) { return P <= 1024 ? 8 : 2; }

// twiddles, the wavefronts' buffers, the window, the samples of a run: 16.4 KB for 400 / 160 / 512, at most 56 KB (P = 1024, N = S = P)
static size_t wave_lds(int N, int S, int P) {
  const int F = wave_frames(P), H = P / 2, nz = std::min(WAVE_WAVES, F);
  return (size_t)(H + nz * H) * sizeof(float2) + (size_t)(N + (F - 1) * S + N) * sizeof(float);
}

void launch_feat_wave(const void* pcm, int kind, long long n_samples, const long long* seg, const int* offsets, int B, int N, int S, int P,
                      float preemph, const float* window, const float* twiddle, float* out, long long out_rows, hipStream_t s) {
  const int F = wave_frames(P);
  const unsigned long long runs = ((unsigned long long)out_rows + F - 1) / F + (unsigned long long)B;
  const int grid = (int)std::min<unsigned long long>(16384, runs);
  const size_t lds = wave_lds(N, S, P);
#define RSR_WAVE_LAUNCH(PT, F32) \
  hipLaunchKernelGGL((k_feat_wave<PT, F32>), dim3(grid), dim3(256), lds, s, pcm, n_samples, seg, offsets, B, (uint32_t)N, (uint32_t)S, (uint32_t)P, \
                     preemph, window, twiddle, out, out_rows, runs, (uint32_t)F)
  if (P == 512) { if (kind) RSR_WAVE_LAUNCH(512, true); else RSR_WAVE_LAUNCH(512, false); }
  else { if (kind) RSR_WAVE_LAUNCH(0, true); else RSR_WAVE_LAUNCH(0, false); }
#undef RSR_WAVE_LAUNCH
}

// k_feat_wave's need plus the power rows, the log-mel rows, the transposed DCT and the two mel tables: 30.7 KB for 400 / 160 / 512 with
// 40 filters, 40 cepstra and the recipe's 468 weights
size_t mfcc_lds_bytes(int N, int S, int P, int M, int C, int nnz) {
  const int F = wave_frames(P), H = P / 2, nz = std::min(WAVE_WAVES, F);
  return wave_lds(N, S, P) + ((size_t)nz * H + (size_t)nz * M + (size_t)M * C + 3 * (size_t)M + (size_t)nnz) * sizeof(float);
}

void launch_feat_mfcc(const void* pcm, int kind, long long n_samples, const long long* seg, const int* offsets, int B, int N, int S, int P,
                      float preemph, const float* window, const float* twiddle, const int* mel_seg, const float* mel_w, int nnz, int M,
                      const float* dct, int C, float* out, long long out_rows, hipStream_t s) {
  const int F = wave_frames(P);
  const unsigned long long runs = ((unsigned long long)out_rows + F - 1) / F + (unsigned long long)B;
  const int grid = (int)std::min<unsigned long long>(16384, runs);
  const size_t lds = mfcc_lds_bytes(N, S, P, M, C, nnz);
#define RSR_MFCC_LAUNCH(PT, F32) \
  hipLaunchKernelGGL((k_feat_mfcc<PT, F32>), dim3(grid), dim3(256), lds, s, pcm, n_samples, seg, offsets, B, (uint32_t)N, (uint32_t)S, (uint32_t)P, \
                     preemph, window, twiddle, mel_seg, mel_w, (uint32_t)nnz, (uint32_t)M, dct, (uint32_t)C, out, out_rows, runs, (uint32_t)F)
  if (P == 512) { if (kind) RSR_MFCC_LAUNCH(512, true); else RSR_MFCC_LAUNCH(512, false); }
  else { if (kind) RSR_MFCC_LAUNCH(0, true); else RSR_MFCC_LAUNCH(0, false); }
#undef RSR_MFCC_LAUNCH
}

}  // namespace rsr
