// synth.hip -- audio out on the device (include/rsrgan.h rsrgan_wave_synth): enhanced log-power-spectrum rows back to
// samples.  Per frame the magnitude is replaced by the row's, the phase of the utterance's own samples is kept; the frames are
// overlap-added with the analysis window as synthesis window and the pre-emphasis is undone by its recurrence.  The definition is the
// one stated at the entry.  fp32 throughout, no atomics, no traffic between workgroups inside a launch, no scratch memory.
// Four launches, grid (items, B): blockIdx.y is the utterance, so nothing an utterance computes depends on its place in the batch.
//   k_synth_frames  wave.hip's sibling: a workgroup takes runs of F consecutive frames of its utterance, stages their samples once, a
//                   wavefront owns a frame: mean, pre-emphasis, window, the H = P / 2 point complex FFT (wave_frame.h, wave_fft.h).  Lane t
//                   takes the bin pairs (k, H - k), k = t, t + 64, .. <= H / 2: the split pass gives X_k and X_{H-k} (bit for bit the
//                   power k_feat_wave takes the log of), the gains g = exp((L - log max(p, eps)) / 2), and the merge pass
//                   Z'_k = E_k + i O_k, E_k = (Y_k + conj Y_{H-k}) / 2, O_k = conj(W^k) (Y_k - conj Y_{H-k}) / 2, whose conjugate goes
//                   to the wavefront's SECOND buffer in natural order (the split pass of other lanes still reads the first).  The
//                   forward wave_fft of the conjugate is the inverse transform: sample 2 j + h is read through fft_pos(j), conjugated
//                   and scaled by 1 / H -- the trick of k_rev_conv.  w[i] (y[i] + w[i] (1 - a) m g_1) goes to work [row][N].
//   k_synth_ola     a workgroup takes chunks of CH = 2048 output samples: sample t gathers its <= ceil(N / S) frame terms, f ascending,
//                   with sum w^2 beside them, divides, and lands in LDS (coalesced reads of `work`).  Then the recurrence
//                   r[t] = z[t] + a r[t - 1] from a zero state at the chunk's start: thread i runs the strip [8 i, 8 i + 8) in order; the
//                   strips' end values are combined by a Hillis-Steele scan over the lanes with the powers a^8, a^16, .. (repeated
//                   squares), the four wavefronts in order with a^512; a strip then adds a^(q + 1) times the state in front of it.
//                   Everything runs in a fixed order.  The chunk goes to `out` (coalesced), its end value to the carries.
//   k_synth_carry   one wavefront per utterance: c_0 = 0, c_{j+1} = e_j + a^CH c_j over its chunks in order; c_j replaces e_j.
//   k_synth_out     out[t] += a^(i + 1) c_j for sample i of chunk j >= 1; a^(i + 1) = a^(i mod 256 + 1) (binary powers, bits ascending)
//                   times (a^256)^(i / 256) (repeated products): a fixed order per sample.
// LDS banks of the strips (ds_read_b32 / ds_write_b32: per 32-lane half, bank = dword index mod 32): thread i reads dwords 8 i + q; with
// one pad dword per 32 (index e -> e + e / 32) lane l of a half lands on bank (8 l + l / 4 + q) mod 32, a bijection of the 32 lanes.
// The inverse transform's epilogue reads float2 index fft_sw(fft_pos(i / 2)): two lanes share an address (a broadcast) and the 16 addresses
// of a half differ in the digits fft_pos moves to the top, of which the swizzle keeps all but index bit 7 for H = 256: a 2-way conflict.
// Memory safety: syn_utt clamps every segment, offset, row count and capacity, and all four kernels call it: s0 into [0, n_samples], n
// into what is left, the first row into [0, lps_rows], F into the rows left there, the first output sample into [0, out_samples], the
// capacity into what is left.  A frame reads row off + f < lps_rows of lps and writes that row of work; a sample index is below n; an
// output index below first + min(n, capacity).  The carries of utterance b start at the sum of ceil(min(n, capacity) / CH) over the
// utterances in front of it, which for segments that do not overlap ends below ceil(out_samples / CH) + B; the index is clamped below
// that count whatever the tables hold.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "kernels.h"
#include "wave_fft.h"
#include "wave_frame.h"

namespace rsr {

constexpr int SYN_CH = 2048, SYN_STRIP = SYN_CH / 256;

struct SynUtt {
  long long s0, n, off, F, o0, nw, cov;      // first sample, samples, first row, frames, first output sample, samples written, samples a frame covers
};

__device__ __forceinline__ long long syn_clamp(long long v, long long lo, long long hi) { return min(max(v, lo), hi); }

// utterance b with everything clamped (uniform over the workgroup)
__device__ __forceinline__ void syn_utt(const SynArgs& a, int b, SynUtt& u) {
  u.s0 = syn_clamp(a.seg[2 * (size_t)b], 0, a.n_samples);
  u.n = syn_clamp(a.seg[2 * (size_t)b + 1], 0, a.n_samples - u.s0);
  const long long frames = u.n < (long long)a.N ? 0ll : 1 + (u.n - (long long)a.N) / (long long)a.S;
  u.off = syn_clamp(a.offsets[b], 0, a.lps_rows);
  u.F = min(min(frames, max((long long)a.offsets[b + 1] - (long long)a.offsets[b], 0ll)), a.lps_rows - u.off);
  u.o0 = syn_clamp(a.out_seg[2 * (size_t)b], 0, a.out_samples);
  u.nw = min(u.n, syn_clamp(a.out_seg[2 * (size_t)b + 1], 0, a.out_samples - u.o0));
  u.cov = u.F > 0 ? (u.F - 1) * (long long)a.S + (long long)a.N : 0ll;
}

__device__ __forceinline__ long long syn_chunks(const SynUtt& u) { return (u.nw + SYN_CH - 1) / SYN_CH; }

// the first carry of utterance b: the chunks of the utterances in front of it
__device__ __forceinline__ long long syn_slot0(const SynArgs& a, int b) {
  long long s = 0;
  for (int i = 0; i < b; ++i) { SynUtt v; syn_utt(a, i, v); s += syn_chunks(v); }
  return s;
}

__device__ __forceinline__ float* syn_carry(const SynArgs& a, long long slot0, long long j) {
  return a.work + (size_t)a.lps_rows * a.N + (size_t)min(slot0 + j, a.slots - 1);
}

// the split pass for bin k <= H: X_k (wave.hip wave_power takes its squared modulus, operation for operation)
__device__ __forceinline__ float2 syn_bin(const float2* z, const float2* tw, uint32_t k, uint32_t H) {
  const float2 a = z[fft_sw(fft_pos(k & (H - 1), H))], c = z[fft_sw(fft_pos((H - k) & (H - 1), H))];
  const float2 ev = make_float2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y));         // (Z_k + conj Z_{H-k}) / 2
  const float2 od = make_float2(0.5f * (a.y + c.y), -0.5f * (a.x - c.x));        // -i (Z_k - conj Z_{H-k}) / 2
  const float2 r = cmul(od, tw_at(tw, k, H));
  return make_float2(ev.x + r.x, ev.y + r.y);
}

// 2, 3: the gain of a bin from its LPS value and its power; a NaN counts as -80
__device__ __forceinline__ float syn_gain(float L, float2 X) {
  const float Lc = fminf(fmaxf(L, -80.f), 80.f);
  return expf(0.5f * (Lc - logf(fmaxf(X.x * X.x + X.y * X.y, FLT_EPSILON))));
}

// the merge pass for index k < H from Y_k and Y_{H-k}: conj(E_k + i O_k)
__device__ __forceinline__ float2 syn_merge(float2 y, float2 c, float2 w) {
  const float2 e = make_float2(0.5f * (y.x + c.x), 0.5f * (y.y - c.y));
  const float2 o = cmul(make_float2(0.5f * (y.x - c.x), 0.5f * (y.y + c.y)), make_float2(w.x, -w.y));
  return make_float2(e.x - o.y, -(e.y + o.x));
}

// a^e, the bits of e ascending
__device__ __forceinline__ float syn_pow(float a, uint32_t e) {
  float r = 1.f, s = a;
  for (; e; e >>= 1) { if (e & 1u) r *= s; s *= s; }
  return r;
}

// PT: the padded length at compile time (the fast path, 512), or 0: P is the argument
template <int PT, bool F32>
__global__ __launch_bounds__(256) void k_synth_frames(SynArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const uint32_t P = PT ? (uint32_t)PT : a.P, H = P >> 1, NB = H + 1, N = a.N, S = a.S, F = a.F;
  const uint32_t nz = min((uint32_t)WAVE_WAVES, F);
  float2* tw = reinterpret_cast<float2*>(lds_raw);                   // [H]
  float2* zall = tw + H;                                             // [nz][H]: the forward transform
  float2* yall = zall + (size_t)nz * H;                              // [nz][H]: the inverse transform
  float* win = reinterpret_cast<float*>(yall + (size_t)nz * H);      // [N]
  float* smp = win + N;                                              // [(F - 1) * S + N]
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  SynUtt u;
  syn_utt(a, blockIdx.y, u);
  const unsigned long long runs = ((unsigned long long)u.F + F - 1) / F;
  if (blockIdx.x >= runs) return;
  for (uint32_t i = tid; i < H; i += 256) tw[i] = make_float2(a.twiddle[2 * i], a.twiddle[2 * i + 1]);
  for (uint32_t i = tid; i < N; i += 256) win[i] = a.window[i];
  float2* z = zall + (size_t)min(wave, nz - 1) * H;
  float2* y = yall + (size_t)min(wave, nz - 1) * H;
  const float inv = 1.f / (float)H, dc = 1.f - a.preemph;
  for (unsigned long long w = blockIdx.x; w < runs; w += gridDim.x) {
    WaveRun r;
    r.s0 = u.s0; r.off = u.off; r.f0 = (long long)w * F;
    r.nf = (uint32_t)min((long long)F, u.F - r.f0);
    wave_stage_run<F32>(smp, a.pcm, a.n_samples, r, N, S, tid);
    for (uint32_t it = 0; it < F; it += nz) {
      const uint32_t fl = it + wave;
      const bool live = wave < nz && fl < r.nf;
      const float* x = smp + (live ? fl * S : 0u);
      const float mean = wave_mean(x, N, lane);
      wave_load_frame(z, x, mean, a.preemph, win, N, H, lane, live);
      wave_fft(z, tw, P, H, lane, live);
      const long long row = live ? r.off + r.f0 + (long long)fl : 0ll;        // (live: below off + F <= lps_rows)
      float g1 = 0.f;
      if (live) {
        const float* __restrict__ L = a.lps + (size_t)row * NB;
        g1 = syn_gain(L[1], syn_bin(z, tw, 1, H));
        for (uint32_t k = lane; k <= (H >> 1); k += 64) {
          const uint32_t k2 = H - k;
          const float2 xa = syn_bin(z, tw, k, H), xb = syn_bin(z, tw, k2, H);
          const float ga = k ? syn_gain(L[k], xa) : g1, gb = syn_gain(L[k2], xb);
          const float2 ya = make_float2(ga * xa.x, ga * xa.y), yb = make_float2(gb * xb.x, gb * xb.y);
          y[fft_sw(k)] = syn_merge(ya, yb, tw_at(tw, k, H));
          if (k && k2 != k) y[fft_sw(k2)] = syn_merge(yb, ya, tw_at(tw, k2, H));
        }
      }
      __syncthreads();
      wave_fft(y, tw, P, H, lane, live);
      if (live) {
        float* o = a.work + (size_t)row * N;
        const float m = dc * mean * g1;
        for (uint32_t i = lane; i < N; i += 64) {
          const float2 v = y[fft_sw(fft_pos(i >> 1, H))];
          const float wi = win[i];
          o[i] = wi * (((i & 1u) ? -v.y : v.x) * inv + wi * m);
        }
      }
      __syncthreads();                                                // (z and y are rewritten by this wavefront's next frame)
    }
  }
}

__device__ __forceinline__ uint32_t syn_pad(uint32_t e) { return e + (e >> 5); }

__global__ __launch_bounds__(256) void k_synth_ola(SynArgs a) {
  __shared__ float zb[SYN_CH + SYN_CH / 32];
  __shared__ float wtot[4];
  SynUtt u;
  syn_utt(a, blockIdx.y, u);
  const long long nc = syn_chunks(u);
  if ((long long)blockIdx.x >= nc) return;
  const long long slot0 = syn_slot0(a, blockIdx.y);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, N = a.N, S = a.S;
  const float pre = a.preemph;
  float pw[SYN_STRIP];                                                // a^(q + 1): repeated products
  pw[0] = pre;
#pragma unroll
  for (int q = 1; q < SYN_STRIP; ++q) pw[q] = pw[q - 1] * pre;
  const float* __restrict__ win = a.window;
  const float* __restrict__ fr = a.work;
  for (long long j = blockIdx.x; j < nc; j += gridDim.x) {
    const long long base = j * SYN_CH;
    for (uint32_t i = tid; i < (uint32_t)SYN_CH; i += 256) {
      const long long t = base + i;
      float zv = 0.f;
      if (t >= 1 && t < u.nw && t < u.cov) {
        const long long lo = t >= (long long)N ? (t - N) / S + 1 : 0ll, hi = min(u.F - 1, (t - 1) / S);
        float num = 0.f, den = 0.f;
        for (long long f = lo; f <= hi; ++f) {
          const uint32_t k = (uint32_t)(t - f * S);                    // 1 <= k < N
          const float wk = win[k];
          num += fr[(size_t)(u.off + f) * N + k];
          den += wk * wk;
        }
        zv = den > 0.f ? num / fmaxf(den, 1e-3f) : 0.f;
      }
      zb[syn_pad(i)] = zv;
    }
    __syncthreads();
    float r[SYN_STRIP], prev = 0.f;
#pragma unroll
    for (int q = 0; q < SYN_STRIP; ++q) { prev = zb[syn_pad(SYN_STRIP * tid + q)] + pre * prev; r[q] = prev; }
    // the state at the end of every strip of the wavefront, from zero at the wavefront's first sample; pl = a^(8 (lane + 1))
    float e = prev, mult = pw[SYN_STRIP - 1], pl = 1.f;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const float v = __shfl_up(e, d, 64);
      if (lane >= d) e += mult * v;
      if ((lane + 1) & d) pl *= mult;
      mult *= mult;
    }
    if (lane == 63) { pl = mult; wtot[wave] = e; }
    __syncthreads();
    float cw = 0.f;                                                   // the state in front of the wavefront: the wavefronts before it, in order
    for (uint32_t v = 0; v < wave; ++v) cw = wtot[v] + mult * cw;
    e += pl * cw;
    float c = __shfl_up(e, 1, 64);                                    // the state in front of the strip
    if (lane == 0) c = cw;
#pragma unroll
    for (int q = 0; q < SYN_STRIP; ++q) zb[syn_pad(SYN_STRIP * tid + q)] = r[q] + pw[q] * c;
    if (tid == 255) *syn_carry(a, slot0, j) = e;
    __syncthreads();
    for (uint32_t i = tid; i < (uint32_t)SYN_CH; i += 256) {
      const long long t = base + i;
      if (t < u.nw) a.out[u.o0 + t] = t < u.cov ? zb[syn_pad(i)] : 0.f;
    }
    __syncthreads();                                                  // (zb and wtot are rewritten by the next chunk)
  }
}

__global__ __launch_bounds__(64) void k_synth_carry(SynArgs a) {
  SynUtt u;
  syn_utt(a, blockIdx.x, u);
  const long long nc = syn_chunks(u), slot0 = syn_slot0(a, blockIdx.x);
  const uint32_t lane = threadIdx.x;
  float pch = a.preemph;                                              // a^CH: repeated squares
  for (int s = 1; s < SYN_CH; s <<= 1) pch *= pch;
  float c = 0.f;
  for (long long j0 = 0; j0 < nc; j0 += 64) {
    const bool have = j0 + lane < nc;
    const float ev = have ? *syn_carry(a, slot0, j0 + lane) : 0.f;
    float mine = 0.f;
    for (uint32_t l = 0; l < 64; ++l) {
      const float e = __shfl(ev, l, 64);
      if (lane == l) mine = c;
      c = e + pch * c;
    }
    if (have) *syn_carry(a, slot0, j0 + lane) = mine;
  }
}

__global__ __launch_bounds__(256) void k_synth_out(SynArgs a) {
  SynUtt u;
  syn_utt(a, blockIdx.y, u);
  const long long nc = syn_chunks(u), lim = min(u.nw, u.cov);
  if ((long long)blockIdx.x + 1 >= nc) return;
  const long long slot0 = syn_slot0(a, blockIdx.y);
  const uint32_t tid = threadIdx.x;
  const float p0 = syn_pow(a.preemph, tid + 1), p256 = syn_pow(a.preemph, 256);
  for (long long j = (long long)blockIdx.x + 1; j < nc; j += gridDim.x) {
    const float c = *syn_carry(a, slot0, j);
    float p = p0;
    for (uint32_t i = tid; i < (uint32_t)SYN_CH; i += 256) {
      const long long t = j * SYN_CH + i;
      if (t < lim) a.out[u.o0 + t] += p * c;
      p *= p256;
    }
  }
}

int synth_chunk() { return SYN_CH; }

// twiddles, two buffers per working wavefront, the window, the samples of a run
static size_t synth_lds(int N, int S, int P, int F) {
  const int H = P / 2, nz = std::min(WAVE_WAVES, F);
  return (size_t)(H + 2 * nz * H) * sizeof(float2) + (size_t)(N + (F - 1) * S + N) * sizeof(float);
}

// the frames of a run: wave_frames(P) where that fits 64 KB of LDS (25.5 KB for 400 / 160 / 512), else 2 (at most 64 KB: P = N = S = 2048)
static int synth_frames(int N, int S, int P) {
  const int F = wave_frames(P);
  return synth_lds(N, S, P, F) <= 65536 ? F : 2;
}

long long synth_work_floats(int B, long long lps_rows, long long out_samples, int N) {
  return lps_rows * (long long)N + (out_samples + SYN_CH - 1) / SYN_CH + (long long)B;
}

void launch_wave_synth(const SynArgs& args, hipStream_t s) {
  SynArgs a = args;
  const int N = (int)a.N, S = (int)a.S, P = (int)a.P, F = synth_frames(N, S, P);
  a.F = (uint32_t)F;
  a.slots = (a.out_samples + SYN_CH - 1) / SYN_CH + (long long)a.B;
  const size_t lds = synth_lds(N, S, P, F);
  // an utterance has at most as many frames as lps has rows and as n_samples make
  const long long fmax = std::min(a.lps_rows, a.n_samples < N ? 0ll : 1 + (a.n_samples - N) / S);
  const unsigned gf = (unsigned)std::min<long long>(std::max<long long>((fmax + F - 1) / F, 1), 16384);
  const unsigned gc = (unsigned)std::min<long long>((std::min(a.out_samples, a.n_samples) + SYN_CH - 1) / SYN_CH, 65536);
#define RSR_SYNTH_LAUNCH(PT, F32) hipLaunchKernelGGL((k_synth_frames<PT, F32>), dim3(gf, a.B), dim3(256), lds, s, a)
  if (P == 512) { if (a.kind) RSR_SYNTH_LAUNCH(512, true); else RSR_SYNTH_LAUNCH(512, false); }
  else { if (a.kind) RSR_SYNTH_LAUNCH(0, true); else RSR_SYNTH_LAUNCH(0, false); }
#undef RSR_SYNTH_LAUNCH
  hipLaunchKernelGGL(k_synth_ola, dim3(gc, a.B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_synth_carry, dim3(a.B), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_synth_out, dim3(gc, a.B), dim3(256), 0, s, a);
}

}  // namespace rsr
