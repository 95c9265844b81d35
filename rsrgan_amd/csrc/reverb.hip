// reverb.hip -- reverberate clean audio on the device (include/rsrgan.h rsrgan_wave_reverb): y = x * h by uniformly
// partitioned overlap-save on the LDS FFT of wave_fft.h, the early-reverberation energy, an additive noise at an SNR, power
// normalisation and the shift by the RIR's peak.  The definition is the one stated at the entry.  fp32 throughout; the per-utterance
// sums are finished in fp64.
// Blocks: C is the complex FFT length, a block is Bk = C / 2 samples.  W_j = x[(j - 1) Bk, (j + 1) Bk) (zero outside the utterance) is the
// window of input block j, H_p the spectrum of taps [p Bk, (p + 1) Bk) padded with Bk zeros.  Output block k, y[k Bk, (k + 1) Bk), is the
// second half of IDFT_C(sum_p DFT(W_{k - p}) . H_p), p ascending.  Four launches, grid (items, B): blockIdx.y is the utterance, so
// nothing an utterance computes depends on its place in the batch.
//   k_rev_spectra  a wavefront takes a PAIR of real chunks as real and imaginary part of one transform and splits the result
//                  (A_f = (Z_f + conj Z_{C - f}) / 2, B_f = (Z_f - conj Z_{C - f}) / 2i): the windows W_2a, W_2a+1, the RIR's partitions
//                  2a, 2a + 1, and those of the early taps [e0, e1).  Spectra go to the utterance's slot of `work` in natural order.  The
//                  input power of each block (sum of its squares) is taken on the way.
//   k_rev_conv     a wavefront takes output blocks k, k + 1 (k even): since h is real, sum_p (W_{k - p} + i W_{k + 1 - p}) . H_p inverts to
//                  y_k + i y_{k + 1}.  Lane l forms the sum for bins l, l + 64, .. with p ascending (W_{k + 1 - p} is the value read one step
//                  earlier), writes the conjugate into LDS, runs the forward wave_fft and reads sample Bk + t through fft_pos, conjugated
//                  and scaled by 1 / C.  y goes to `out` unscaled and without noise; per block, sum y^2, sum y v and sum v^2 (v the noise
//                  where its span covers the block) go to the slot.  The early convolution is the same code on the early partitions,
//                  keeping only the sum of squares.  Without an RIR the block is the samples themselves, exactly.
//   k_rev_gains    one wavefront per utterance: lanes 0 - 4 add the five arrays of block sums in block order in fp64; lane 0 forms P_in,
//                  E, g, P_out = (sum y^2 + 2 g sum y v + g^2 sum v^2) / len and c.
//   k_rev_out      out[i] = c (y[i + shift] + g v), in place.
// Sums: lane l adds its elements l, l + 64, .. ascending, then the xor-butterfly of wave_sum; no atomics.
// Memory safety: every segment, index, q, e0, e1, s, m and capacity is clamped by rev_utt, which all four kernels call; the slot of an
// utterance is work + b * (work_bytes / B rounded down to 16) and an utterance whose need (rev_layout) is above the slot is skipped by
// all four kernels: it writes nothing.  LDS: twiddles [C] and nz buffers [C] of float2, nz = 4 up to C = 1024, 2 above: at most 48 KB.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.h"
#include "wave_fft.h"

namespace rsr {

constexpr long long REV_MAX_N = 1ll << 28, REV_MAX_L = 1ll << 24;     // samples of an utterance, taps of an RIR (clamps)

struct RevLayout {
  long long NI, NO, NOE, PH, PE;       // input blocks, output blocks, output blocks of the early convolution, partitions (full, early)
  unsigned long long xs, hs, he, fl, bytes;      // byte offsets of the window spectra, the partition spectra (full, early), the floats; the need
};

// the slot of an utterance of n samples with L taps (0: no RIR), Le early taps (0: the early energy is not needed)
__host__ __device__ inline RevLayout rev_layout(long long n, long long L, long long Le, long long C) {
  const long long Bk = C / 2;
  RevLayout r;
  r.NI = (n + Bk - 1) / Bk;
  r.PH = (L + Bk - 1) / Bk;
  r.PE = (Le + Bk - 1) / Bk;
  r.NO = L > 0 ? (n + L - 1 + Bk - 1) / Bk : r.NI;
  r.NOE = Le > 0 ? (n + Le - 1 + Bk - 1) / Bk : 0;
  const unsigned long long spec = (unsigned long long)C * sizeof(float2);
  r.xs = 0;
  r.hs = r.xs + 2 * (unsigned long long)((r.NI + 2) / 2) * spec;
  r.he = r.hs + 2 * (unsigned long long)((r.PH + 1) / 2) * spec;
  r.fl = r.he + 2 * (unsigned long long)((r.PE + 1) / 2) * spec;
  const unsigned long long nf = 4 + (unsigned long long)(r.NI + 3 * r.NO + r.NOE);      // (c, g, -, -), Sxx, Syy, Syv, Svv, See
  r.bytes = r.fl + ((nf + 3) & ~3ull) * sizeof(float);
  return r;
}

size_t reverb_work_bytes(int B, long long n_max, long long L_max, int C) {
  return (size_t)B * rev_layout(n_max, L_max, L_max, C).bytes;
}

struct RevUtt {
  long long x0, h0, v0, o0, s, m;      // first sample, first tap, first noise sample, first output sample; the noise's start and span in y
  int n, L, q, e0, Le, nv, len, lenE, sh, nw;      // samples, taps (0: none), peak, first early tap, early taps, noise samples, len(y), len of the
                                                   // early convolution, the shift, the samples written
  bool noisy;                          // a noise is selected (g is formed, the early energy is needed)
  float pv, snr;
  RevLayout lay;
  float2 *Xs, *Hs, *He;
  float *cg, *Sxx, *Syy, *Syv, *Svv, *See;
};

__device__ __forceinline__ long long rev_clamp(long long v, long long lo, long long hi) { return min(max(v, lo), hi); }

// utterance b with everything clamped; false: it is empty or its slot is too small (uniform over the workgroup)
__device__ __forceinline__ bool rev_utt(const RevArgs& a, int b, RevUtt& u) {
  u.x0 = rev_clamp(a.seg[2 * (size_t)b], 0, a.n_samples);
  u.n = (int)rev_clamp(a.seg[2 * (size_t)b + 1], 0, min(a.n_samples - u.x0, REV_MAX_N));
  const int ri = a.sel[4 * (size_t)b], ni = a.sel[4 * (size_t)b + 1];
  u.h0 = 0; u.L = 0; u.q = 0; u.e0 = 0; u.Le = 0;
  if (ri >= 0 && ri < a.R && a.rir) {
    const long long* rs = a.rir_seg + 5 * (size_t)ri;
    u.h0 = rev_clamp(rs[0], 0, a.n_taps);
    u.L = (int)rev_clamp(rs[1], 0, min(a.n_taps - u.h0, REV_MAX_L));
    if (u.L > 0) {
      u.q = (int)rev_clamp(rs[2], 0, u.L - 1);
      u.e0 = (int)rev_clamp(rs[3], 0, u.L);
      u.Le = (int)rev_clamp(rs[4], u.e0, u.L) - u.e0;
    }
  }
  u.v0 = 0; u.nv = 0; u.pv = 0.f;
  if (ni >= 0 && ni < a.V && a.noise) {
    u.v0 = rev_clamp(a.noise_seg[2 * (size_t)ni], 0, a.n_noise);
    u.nv = (int)rev_clamp(a.noise_seg[2 * (size_t)ni + 1], 0, min(a.n_noise - u.v0, 1ll << 30));
    u.pv = a.noise_pow[ni];
  }
  u.noisy = u.nv > 0;
  u.snr = a.snr[b];
  u.len = u.n ? u.n + max(u.L, 1) - 1 : 0;
  u.s = rev_clamp(a.sel[4 * (size_t)b + 2], 0, u.len);
  u.m = u.noisy ? rev_clamp(a.sel[4 * (size_t)b + 3], 0, u.len - u.s) : 0;
  if (!u.noisy || u.L == 0) u.Le = 0;
  u.lenE = u.Le > 0 ? u.n + u.Le - 1 : 0;
  u.sh = (a.flags & 1) ? u.q : 0;
  u.o0 = rev_clamp(a.out_seg[2 * (size_t)b], 0, a.out_samples);
  const long long cap = rev_clamp(a.out_seg[2 * (size_t)b + 1], 0, a.out_samples - u.o0);
  u.nw = (int)min((long long)((a.flags & 1) ? u.n : u.len), cap);
  u.lay = rev_layout(u.n, u.L, u.Le, a.C);
  unsigned char* slot = a.work + (size_t)b * a.slot;
  u.Xs = reinterpret_cast<float2*>(slot + u.lay.xs);
  u.Hs = reinterpret_cast<float2*>(slot + u.lay.hs);
  u.He = reinterpret_cast<float2*>(slot + u.lay.he);
  u.cg = reinterpret_cast<float*>(slot + u.lay.fl);
  u.Sxx = u.cg + 4;
  u.Syy = u.Sxx + u.lay.NI;
  u.Syv = u.Syy + u.lay.NO;
  u.Svv = u.Syv + u.lay.NO;
  u.See = u.Svv + u.lay.NO;
  return u.n > 0 && u.lay.bytes <= a.slot;
}

__device__ __forceinline__ float rev_sample(const RevArgs& a, long long i) {
  return a.kind ? reinterpret_cast<const float*>(a.pcm)[i] : (float)reinterpret_cast<const short*>(a.pcm)[i];
}

__device__ __forceinline__ float2* rev_lds(unsigned char* raw, const RevArgs& a, uint32_t nz, uint32_t tid, float2*& tw) {
  const uint32_t C = a.C;
  tw = reinterpret_cast<float2*>(raw);                               // [C]: exp(-2 pi i j / 2 C)
  for (uint32_t i = tid; i < C; i += 256) tw[i] = make_float2(a.twiddle[2 * i], a.twiddle[2 * i + 1]);
  return tw + C + (size_t)min(tid >> 6, nz - 1) * C;                  // the wavefront's buffer [C]
}

__global__ __launch_bounds__(256) void k_rev_spectra(RevArgs a, uint32_t nz) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const uint32_t C = a.C, Bk = C >> 1, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  RevUtt u;
  if (!rev_utt(a, blockIdx.y, u)) return;
  const uint32_t nX = (uint32_t)((u.lay.NI + 2) / 2), nH = (uint32_t)((u.lay.PH + 1) / 2), nE = (uint32_t)((u.lay.PE + 1) / 2);
  if ((unsigned long long)blockIdx.x * nz >= (unsigned long long)nX + nH + nE) return;
  float2* tw;
  float2* z = rev_lds(lds_raw, a, nz, tid, tw);
  const uint32_t it = blockIdx.x * nz + wave;
  const bool live = wave < nz && it < nX + nH + nE, isx = it < nX, early = it >= nX + nH;
  const uint32_t pr = isx ? it : early ? it - nX - nH : it - nX;      // the pair: chunks 2 pr, 2 pr + 1
  const long long hb = u.h0 + (early ? u.e0 : 0), Lr = early ? u.Le : u.L;
  float sa = 0.f, sb = 0.f;
  for (uint32_t j = lane; j < C; j += 64) {
    float re = 0.f, im = 0.f;
    if (live && isx) {
      const long long ta = ((long long)2 * pr - 1) * Bk + j, tb = ta + Bk;
      if (ta >= 0 && ta < u.n) re = rev_sample(a, u.x0 + ta);
      if (tb < u.n) im = rev_sample(a, u.x0 + tb);
      if (j >= Bk) { sa += re * re; sb += im * im; }
    } else if (live && j < Bk) {
      const long long ta = (long long)2 * pr * Bk + j, tb = ta + Bk;
      if (ta < Lr) re = a.rir[hb + ta];
      if (tb < Lr) im = a.rir[hb + tb];
    }
    if (live) z[fft_sw(j)] = make_float2(re, im);
  }
  if (live && isx) {
    sa = wave_sum(sa); sb = wave_sum(sb);
    if (lane == 0) {
      if (2 * (long long)pr < u.lay.NI) u.Sxx[2 * pr] = sa;
      if (2 * (long long)pr + 1 < u.lay.NI) u.Sxx[2 * pr + 1] = sb;
    }
  }
  if (u.L == 0) return;                                                // (uniform: without an RIR only the input power is needed)
  __syncthreads();
  wave_fft(z, tw, 2 * C, C, lane, live);
  if (live) {
    float2* d0 = (isx ? u.Xs : early ? u.He : u.Hs) + (size_t)2 * pr * C;
    float2* d1 = d0 + C;
    for (uint32_t f = lane; f < C; f += 64) {
      const float2 p = z[fft_sw(fft_pos(f, C))], c = z[fft_sw(fft_pos((C - f) & (C - 1), C))];
      d0[f] = make_float2(0.5f * (p.x + c.x), 0.5f * (p.y - c.y));
      d1[f] = make_float2(0.5f * (p.y + c.y), -0.5f * (p.x - c.x));
    }
  }
}

__global__ __launch_bounds__(256) void k_rev_conv(RevArgs a, uint32_t nz) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const uint32_t C = a.C, Bk = C >> 1, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  RevUtt u;
  if (!rev_utt(a, blockIdx.y, u)) return;
  const uint32_t nF = (uint32_t)((u.lay.NO + 1) / 2), nE = (uint32_t)((u.lay.NOE + 1) / 2);
  if ((unsigned long long)blockIdx.x * nz >= (unsigned long long)nF + nE) return;
  float2* tw;
  float2* z = rev_lds(lds_raw, a, nz, tid, tw);
  const uint32_t it = blockIdx.x * nz + wave;
  const bool live = wave < nz && it < nF + nE, early = it >= nF;
  const long long k = 2 * (long long)(early ? it - nF : it);          // output blocks k, k + 1
  const long long NI = u.lay.NI, NOx = early ? u.lay.NOE : u.lay.NO, lenx = early ? u.lenE : u.len;
  float inv = 1.f;
  if (u.L == 0) {
    // no RIR: the blocks are the samples, laid where the epilogue reads them
    if (live)
      for (uint32_t t = lane; t < Bk; t += 64) {
        const long long ta = k * Bk + t, tb = ta + Bk;
        z[fft_sw(fft_pos(Bk + t, C))] = make_float2(ta < u.n ? rev_sample(a, u.x0 + ta) : 0.f, tb < u.n ? -rev_sample(a, u.x0 + tb) : 0.f);
      }
    __syncthreads();
  } else {
    if (live) {
      const float2* __restrict__ Hs = early ? u.He : u.Hs;
      const float2* __restrict__ Xs = u.Xs;
      const long long PH = early ? u.lay.PE : u.lay.PH;
      const long long plo = max(0ll, k - NI), phi = min(PH - 1, k + 1);
      for (uint32_t f = lane; f < C; f += 64) {
        float2 acc = make_float2(0.f, 0.f);
        float2 prev = (k + 1 - plo <= NI) ? Xs[(size_t)(k + 1 - plo) * C + f] : make_float2(0.f, 0.f);
#pragma unroll 4
        for (long long p = plo; p <= phi; ++p) {
          const float2 cur = (k - p >= 0) ? Xs[(size_t)(k - p) * C + f] : make_float2(0.f, 0.f);
          const float2 r = cmul(make_float2(cur.x - prev.y, cur.y + prev.x), Hs[(size_t)p * C + f]);
          acc.x += r.x; acc.y += r.y;
          prev = cur;
        }
        z[fft_sw(f)] = make_float2(acc.x, -acc.y);
      }
    }
    __syncthreads();
    wave_fft(z, tw, 2 * C, C, lane, live);
    inv = 1.f / (float)C;
  }
  if (!live) return;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const long long kb = k + half;
    if (kb >= NOx) break;
    float yy = 0.f, yv = 0.f, vv = 0.f;
    for (uint32_t t = lane; t < Bk; t += 64) {
      const float2 r = z[fft_sw(fft_pos(Bk + t, C))];
      const float y = half ? -r.y * inv : r.x * inv;
      const long long ty = kb * Bk + t;
      if (ty < lenx) {
        yy += y * y;
        if (!early) {
          if (ty >= u.s && ty < u.s + u.m) {
            const float v = a.noise[u.v0 + (ty - u.s) % u.nv];
            yv += y * v; vv += v * v;
          }
          const long long i = ty - u.sh;
          if (i >= 0 && i < u.nw) a.out[u.o0 + i] = y;
        }
      }
    }
    yy = wave_sum(yy); yv = wave_sum(yv); vv = wave_sum(vv);
    if (lane == 0) {
      if (early) u.See[kb] = yy;
      else { u.Syy[kb] = yy; u.Syv[kb] = yv; u.Svv[kb] = vv; }
    }
  }
}

__global__ __launch_bounds__(64) void k_rev_gains(RevArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  RevUtt u;
  if (!rev_utt(a, b, u)) {
    if (a.gains && lane == 0) { a.gains[2 * (size_t)b] = 1.f; a.gains[2 * (size_t)b + 1] = 0.f; }
    return;
  }
  const float* arr = lane == 0 ? u.Sxx : lane == 1 ? u.Syy : lane == 2 ? u.Syv : lane == 3 ? u.Svv : u.See;
  const long long cnt = lane == 0 ? u.lay.NI : lane < 4 ? u.lay.NO : lane == 4 ? u.lay.NOE : 0;
  double sum = 0.0;
  for (long long i = 0; i < cnt; i += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = i + j < cnt ? arr[i + j] : 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) sum += (double)v[j];                 // block order
  }
  const double sxx = __shfl(sum, 0, 64), syy = __shfl(sum, 1, 64), syv = __shfl(sum, 2, 64), svv = __shfl(sum, 3, 64), see = __shfl(sum, 4, 64);
  if (lane) return;
  const double pin = sxx / (double)u.n;
  const double E = u.L == 0 ? pin : u.lenE > 0 ? see / (double)u.lenE : 0.0;
  float g = 0.f;
  if (u.noisy && E > 0.0 && u.pv > 0.f) {
    const double gd = sqrt(pow(10.0, -(double)u.snr / 10.0) * E / (double)u.pv);
    if (gd == gd && gd <= 3.0e38) g = (float)gd;
  }
  const double pout = (syy + 2.0 * (double)g * syv + (double)g * (double)g * svv) / (double)u.len;
  float c = 1.f;
  if ((a.flags & 2) && pout > 0.0) c = (float)sqrt(pin / pout);
  u.cg[0] = c; u.cg[1] = g;
  if (a.gains) { a.gains[2 * (size_t)b] = c; a.gains[2 * (size_t)b + 1] = g; }
}

__global__ __launch_bounds__(256) void k_rev_out(RevArgs a) {
  RevUtt u;
  if (!rev_utt(a, blockIdx.y, u)) return;
  const float c = u.cg[0], g = u.cg[1];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < u.nw; i += (long long)gridDim.x * 256) {
    const long long ty = i + u.sh;
    float y = a.out[u.o0 + i];
    if (ty >= u.s && ty < u.s + u.m) y += g * a.noise[u.v0 + (ty - u.s) % u.nv];
    a.out[u.o0 + i] = c * y;
  }
}

void launch_wave_reverb(const RevArgs& a, size_t work_bytes, hipStream_t s) {
  RevArgs r = a;
  r.slot = ((unsigned long long)work_bytes / (unsigned long long)a.B) & ~15ull;
  const uint32_t C = a.C, nz = C <= 1024 ? 4u : 2u;
  const size_t lds = (size_t)(1 + nz) * C * sizeof(float2);
  // the items of an utterance are bounded by the spectra its slot can hold: window and partition pairs; output block pairs
  const unsigned long long spectra = r.slot / ((unsigned long long)C * sizeof(float2));
  const unsigned gs = (unsigned)std::min<unsigned long long>((spectra / 2 + nz) / nz, 1u << 30);
  const unsigned gc = (unsigned)std::min<unsigned long long>((spectra + 2 + nz) / nz, 1u << 30);
  const unsigned go = (unsigned)std::min<unsigned long long>(std::max<unsigned long long>((unsigned long long)a.out_samples / (2048ull * a.B), 1), 1024);
  hipLaunchKernelGGL(k_rev_spectra, dim3(gs, a.B), dim3(256), lds, s, r, nz);
  hipLaunchKernelGGL(k_rev_conv, dim3(gc, a.B), dim3(256), lds, s, r, nz);
  hipLaunchKernelGGL(k_rev_gains, dim3(a.B), dim3(64), 0, s, r);
  hipLaunchKernelGGL(k_rev_out, dim3(go, a.B), dim3(256), 0, s, r);
}

}  // namespace rsr
