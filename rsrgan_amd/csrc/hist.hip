// hist.hip -- what a TensorBoard histogram summary holds (TensorFlow's HistogramProto with the default bucket limits of
// core/lib/histogram/histogram.cc), computed where the tensors are.  For each of n float32 tensors, given as strided 2-D views
// (element (r, c) at x[r * ld + c * cs]), one record of HIST_REC doubles:
//   [0] min  [1] max  [2] num  [3] sum  [4] sum_squares  [5 + i] the count of bucket i, i < HIST_NL
// The bucket of a value v, widened to double, is upper_bound(limits, v): the first limit GREATER than v, clamped to the last bucket --
// rsrgan_amd/summary.py histogram() (np.searchsorted(side="right")).  -inf lands in bucket 0; +inf and NaN compare greater than / unordered
// with every limit and land in the last; a NaN makes min, max, sum and sum_squares NaN, as NumPy's reductions do.  A view without
// elements yields the record of the single value 0.0 (summary.py substitutes it).
// The limit table (+-1e-12 * 1.1^k by repeated multiplication in double, +-DBL_MAX, 0.0) is built ONCE, on the host, by the loop of
// single multiplications summary._default_limits() runs -- a lone IEEE multiply has nothing to contract; this file is never compiled
// with -ffast-math -- and kept on the device.
// Two launches:
//   k_hist         one launch for all n views, a share of at most HIST_BLOCKS workgroups each (by element count, at least one),
//                  grid-stride over the view's elements.  The table and a row of 32-bit counts live in LDS (12.4 KB + 6.2 KB); the bucket
//                  is found by a branch-free binary search over the LDS table (11 probes; a lane's four searches interleave).  A wave
//                  whose active lanes all hit ONE bucket -- the contention case: normalised features, constants -- adds the lane count
//                  once instead of 64 times.  At its end a workgroup adds its non-empty buckets to the view's global counts with 32-bit
//                  integer vector atomics (exact, order-free) and stores its fp64 partials (sum, sum_squares, min, max, NaN seen) as a
//                  row of its own.
//   k_hist_finish  one workgroup per view: the partial rows added in a fixed tree over the workgroup index -- the same bits run to run;
//                  no floating-point atomics anywhere -- the counts widened to double (exact) and the global counts zeroed again for
//                  the next call.
// Squares of float32 values are exact in double, so sum_squares differs from any other summation order by the additions alone.
// Indices: rows * cols <= 2^31 - 1 (the entry's limit), so element indices and their grid-stride successors fit 32 unsigned bits; the
// address r * ld + c * cs is 64 bits wide.  Plain C++ and vector memory operations only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <map>
#include <mutex>
#include <vector>

#include "kernels.h"

namespace rsr {

static constexpr int HIST_THREADS = 512;             // 8 waves
static constexpr int HIST_BLOCKS = 1024;             // four per CU: the shares of all views of a launch add up to at most this (+ one each)
static constexpr unsigned HIST_MIN_PER_BLOCK = 4096; // a workgroup loads the 12.4 KB table first: no more workgroups than this many elements each
static constexpr int HIST_PART = 5;                  // doubles per partial row: sum, sum_squares, min, max, NaN seen

struct HistArgs {
  HistView v[HIST_MAX_TENSORS];
  int blk0[HIST_MAX_TENSORS + 1];                    // view t owns workgroups [blk0[t], blk0[t + 1])
  int n;
  float clip_lo, clip_hi;
};

const std::vector<double>& hist_limits() {
  static const std::vector<double> table = [] {
#pragma clang fp contract(off)
    std::vector<double> pos;
    for (double v = 1e-12; v < 1e20; v *= 1.1) pos.push_back(v);
    pos.push_back(DBL_MAX);
    std::vector<double> t;
    for (size_t i = pos.size(); i-- > 0;) t.push_back(-pos[i]);
    t.push_back(0.0);
    t.insert(t.end(), pos.begin(), pos.end());
    return t;
  }();
  return table;
}

// first limit greater than v (clamped to the last bucket) = how many limits are not greater than v; NaN: no comparison holds, all are
// counted.  Eleven probes whatever the value (HIST_NL < 2048): no branch depends on the data, so the searches of a lane's four values
// interleave and hide each other's LDS latency.
__device__ __forceinline__ int hist_bucket(const double* __restrict__ lim, double v) {
  static_assert(HIST_NL < 2048, "hist_bucket probes 11 times");
  int pos = 0;
#pragma unroll
  for (int step = 1024; step > 0; step >>= 1) {
    const int to = pos + step;
    const double l = lim[min(to, HIST_NL) - 1];
    pos = (to <= HIST_NL && !(v < l)) ? to : pos;
  }
  return min(pos, HIST_NL - 1);
}

struct HistAcc { double sum, sq; float mn, mx; int nan; };

__device__ __forceinline__ float hist_clip(float v, int clip, float lo, float hi) {
  return clip ? fminf(fmaxf(v, lo), hi) : v;                  // tf.clip_by_value, in the form k_lsgan applies it
}

// one element per lane (act: the lane holds one; b: its bucket).  Called by every lane of the wave together: the loops around it are
// wave-uniform.
__device__ __forceinline__ void hist_add(HistAcc& a, unsigned* __restrict__ cnt, float v, int b, bool act) {
  const unsigned long long m = __ballot(act);
  if (m) {
    const int first = __ffsll((long long)m) - 1;
    const int b0 = __shfl(b, first);
    if (__ballot(act && b == b0) == m) {
      if ((int)(threadIdx.x & 63) == first) atomicAdd(&cnt[b0], (unsigned)__popcll(m));
    } else if (act) {
      atomicAdd(&cnt[b], 1u);
    }
  }
  if (act) {
    const double d = (double)v;
    a.sum += d; a.sq += d * d;
    a.mn = fminf(a.mn, v); a.mx = fmaxf(a.mx, v);             // (fminf / fmaxf drop a NaN operand: the flag carries it)
    a.nan |= (v != v) ? 1 : 0;
  }
}

__device__ __forceinline__ void hist_merge(HistAcc& a, const HistAcc& o) {
  a.sum += o.sum; a.sq += o.sq; a.mn = fminf(a.mn, o.mn); a.mx = fmaxf(a.mx, o.mx); a.nan |= o.nan;
}

// the same tree every time: lanes by shuffle, then the waves in order
__device__ __forceinline__ HistAcc hist_block_reduce(HistAcc a, HistAcc* red) {
  for (int off = 32; off > 0; off >>= 1) {
    HistAcc o;
    o.sum = __shfl_down(a.sum, off); o.sq = __shfl_down(a.sq, off); o.mn = __shfl_down(a.mn, off); o.mx = __shfl_down(a.mx, off);
    o.nan = __shfl_down(a.nan, off);
    hist_merge(a, o);
  }
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = a;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 1; i < nw; ++i) hist_merge(a, red[i]);
  return a;                                                   // (thread 0's is the workgroup's)
}

__global__ __launch_bounds__(HIST_THREADS) void k_hist(const HistArgs a, const double* __restrict__ limits, unsigned* __restrict__ counts,
                                                       double* __restrict__ part) {
  __shared__ double lim[HIST_NL];
  __shared__ unsigned cnt[HIST_NL];
  __shared__ HistAcc red[HIST_THREADS / 64];
  // this workgroup's view, picked with constant indices (the argument block stays in scalar registers)
  int t = 0;
  HistView v = a.v[0];
  int blk0 = 0, nblk = a.blk0[1];
#pragma unroll
  for (int i = 1; i < HIST_MAX_TENSORS; ++i)
    if (i < a.n && (int)blockIdx.x >= a.blk0[i]) { t = i; v = a.v[i]; blk0 = a.blk0[i]; nblk = a.blk0[i + 1] - a.blk0[i]; }
  for (int i = threadIdx.x; i < HIST_NL; i += HIST_THREADS) { lim[i] = limits[i]; cnt[i] = 0u; }
  __syncthreads();

  HistAcc acc{0.0, 0.0, __builtin_inff(), -__builtin_inff(), 0};
  const unsigned total = v.rows * v.cols;                     // <= 2^31 - 1
  const unsigned start = (unsigned)((int)blockIdx.x - blk0) * HIST_THREADS, stride = (unsigned)nblk * HIST_THREADS;
  if (total == 0u) {
    // no elements: the record of the single value 0.0
    if (start == 0u && threadIdx.x < 64) hist_add(acc, cnt, 0.f, hist_bucket(lim, 0.0), threadIdx.x == 0);
  } else if (v.cs == 1 && (v.ld == (long long)v.cols || v.rows == 1u) && ((size_t)v.x & 15) == 0) {
    // dense and 16-byte aligned: four elements per lane and load, the last total % 4 one by one
    const unsigned quads = total >> 2;
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(v.x);
    for (unsigned q0 = start; q0 < quads; q0 += stride) {     // (q0 is uniform over the workgroup)
      const unsigned q = q0 + threadIdx.x;
      const bool act = q < quads;
      const float4 f = act ? x4[q] : float4{0.f, 0.f, 0.f, 0.f};
      const float e0 = hist_clip(f.x, v.clip, a.clip_lo, a.clip_hi), e1 = hist_clip(f.y, v.clip, a.clip_lo, a.clip_hi);
      const float e2 = hist_clip(f.z, v.clip, a.clip_lo, a.clip_hi), e3 = hist_clip(f.w, v.clip, a.clip_lo, a.clip_hi);
      const int b0 = hist_bucket(lim, (double)e0), b1 = hist_bucket(lim, (double)e1);      // four independent searches first
      const int b2 = hist_bucket(lim, (double)e2), b3 = hist_bucket(lim, (double)e3);
      hist_add(acc, cnt, e0, b0, act);
      hist_add(acc, cnt, e1, b1, act);
      hist_add(acc, cnt, e2, b2, act);
      hist_add(acc, cnt, e3, b3, act);
    }
    if (start == 0u && threadIdx.x < 64) {
      const unsigned e = (quads << 2) + threadIdx.x;
      const bool act = threadIdx.x < (total & 3u);
      const float f = hist_clip(act ? v.x[e] : 0.f, v.clip, a.clip_lo, a.clip_hi);
      hist_add(acc, cnt, f, hist_bucket(lim, (double)f), act);
    }
  } else {
    for (unsigned e0 = start; e0 < total; e0 += stride) {
      const unsigned e = e0 + threadIdx.x;
      const bool act = e < total;
      float f = 0.f;
      if (act) {
        const unsigned r = e / v.cols, c = e - r * v.cols;
        f = hist_clip(v.x[(long long)r * v.ld + (long long)c * v.cs], v.clip, a.clip_lo, a.clip_hi);
      }
      hist_add(acc, cnt, f, hist_bucket(lim, (double)f), act);
    }
  }
  __syncthreads();
  unsigned* __restrict__ gc = counts + (size_t)t * HIST_NL;
  for (int i = threadIdx.x; i < HIST_NL; i += HIST_THREADS)
    if (cnt[i]) atomicAdd(&gc[i], cnt[i]);
  acc = hist_block_reduce(acc, red);
  if (threadIdx.x == 0) {
    double* p = part + (size_t)blockIdx.x * HIST_PART;
    p[0] = acc.sum; p[1] = acc.sq; p[2] = (double)acc.mn; p[3] = (double)acc.mx; p[4] = (double)acc.nan;
  }
}

__global__ __launch_bounds__(256) void k_hist_finish(const HistArgs a, unsigned* __restrict__ counts, const double* __restrict__ part,
                                                     double* __restrict__ out) {
  __shared__ HistAcc red[4];
  const int t = blockIdx.x;
  int blk0 = 0, nblk = a.blk0[1];
  unsigned total = a.v[0].rows * a.v[0].cols;
#pragma unroll
  for (int i = 1; i < HIST_MAX_TENSORS; ++i)
    if (i == t) { blk0 = a.blk0[i]; nblk = a.blk0[i + 1] - a.blk0[i]; total = a.v[i].rows * a.v[i].cols; }
  HistAcc acc{0.0, 0.0, __builtin_inff(), -__builtin_inff(), 0};
  for (int b = threadIdx.x; b < nblk; b += 256) {
    const double* p = part + (size_t)(blk0 + b) * HIST_PART;
    HistAcc o{p[0], p[1], (float)p[2], (float)p[3], (int)p[4]};
    hist_merge(acc, o);
  }
  acc = hist_block_reduce(acc, red);
  double* rec = out + (size_t)t * HIST_REC;
  if (threadIdx.x == 0) {
    const double qnan = __builtin_nan("");
    rec[0] = acc.nan ? qnan : (double)acc.mn;
    rec[1] = acc.nan ? qnan : (double)acc.mx;
    rec[2] = total ? (double)total : 1.0;
    rec[3] = acc.sum; rec[4] = acc.sq;
  }
  unsigned* gc = counts + (size_t)t * HIST_NL;
  for (int i = threadIdx.x; i < HIST_NL; i += 256) {
    rec[5 + i] = (double)gc[i];
    gc[i] = 0u;
  }
}

// ---- the launches' own device memory: the table, the global counts (zero between calls) and the partial rows -- one set per device,
// made at the first call.  Calls on different streams share it, so each call waits for the one before it by event.
namespace {
struct HistSpace {
  double* limits = nullptr;
  unsigned* counts = nullptr;
  double* part = nullptr;
  hipEvent_t done = nullptr;
  bool recorded = false;
};
std::mutex hist_mu;
std::map<int, HistSpace> hist_spaces;

HistSpace* hist_space() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  HistSpace& w = hist_spaces[dev];
  if (w.done) return &w;
  const std::vector<double>& table = hist_limits();
  const size_t cbytes = (size_t)HIST_MAX_TENSORS * HIST_NL * sizeof(unsigned);
  HistSpace nw;
  bool ok = (int)table.size() == HIST_NL &&
            hipMalloc((void**)&nw.limits, HIST_NL * sizeof(double)) == hipSuccess &&
            hipMalloc((void**)&nw.counts, cbytes) == hipSuccess &&
            hipMalloc((void**)&nw.part, (size_t)(HIST_BLOCKS + HIST_MAX_TENSORS) * HIST_PART * sizeof(double)) == hipSuccess &&
            hipMemcpy(nw.limits, table.data(), HIST_NL * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemset(nw.counts, 0, cbytes) == hipSuccess &&
            hipEventCreateWithFlags(&nw.done, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    if (nw.limits) (void)hipFree(nw.limits);
    if (nw.counts) (void)hipFree(nw.counts);
    if (nw.part) (void)hipFree(nw.part);
    return nullptr;
  }
  w = nw;
  return &w;
}
}  // namespace

bool launch_hist(int n, const HistView* views, float clip_lo, float clip_hi, double* out, hipStream_t s) {
  if (n < 1 || n > HIST_MAX_TENSORS) return false;
  HistArgs a{};
  a.n = n; a.clip_lo = clip_lo; a.clip_hi = clip_hi;
  unsigned long long sum = 0;
  for (int t = 0; t < n; ++t) sum += (unsigned long long)views[t].rows * views[t].cols;
  int at = 0;
  for (int t = 0; t < n; ++t) {
    a.v[t] = views[t];
    const unsigned long long total = (unsigned long long)views[t].rows * views[t].cols;
    const unsigned long long want = (total + HIST_MIN_PER_BLOCK - 1) / HIST_MIN_PER_BLOCK;
    const unsigned long long share = sum ? (unsigned long long)HIST_BLOCKS * total / sum : 0;
    a.blk0[t] = at;
    at += (int)std::max(1ull, std::min(want, share));
  }
  for (int t = n; t <= HIST_MAX_TENSORS; ++t) a.blk0[t] = at;
  std::lock_guard<std::mutex> lock(hist_mu);
  HistSpace* w = hist_space();
  if (!w) return false;
  if (w->recorded && hipStreamWaitEvent(s, w->done, 0) != hipSuccess) return false;
  hipLaunchKernelGGL(k_hist, dim3(at), dim3(HIST_THREADS), 0, s, a, w->limits, w->counts, w->part);
  hipLaunchKernelGGL(k_hist_finish, dim3(n), dim3(256), 0, s, a, w->counts, w->part, out);
  w->recorded = hipEventRecord(w->done, s) == hipSuccess;
  return w->recorded;
}

// the discriminator's logits ([rows][4], column 0; frame t's rows at (t * frame_rows + b)) as a dense batch-major [B][T] tensor
__global__ __launch_bounds__(256) void k_logits_dense(const float* __restrict__ logits, int frame_rows, int B, int T, float* __restrict__ out,
                                                      int clip, float clip_lo, float clip_hi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * T) return;
  const int b = i / T, t = i - b * T;
  float v = logits[((size_t)t * frame_rows + b) * 4];
  if (clip) v = fminf(fmaxf(v, clip_lo), clip_hi);
  out[i] = v;
}
void launch_logits_dense(const float* logits, int frame_rows, int B, int T, float* out, bool clip, float clip_lo, float clip_hi, hipStream_t s) {
  hipLaunchKernelGGL(k_logits_dense, dim3((B * T + 255) / 256), dim3(256), 0, s, logits, frame_rows, B, T, out, clip ? 1 : 0, clip_lo, clip_hi);
}

}  // namespace rsr
