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
// Further down, in the same layout: k_feat_frames (the frame-level recipes: a gather from a resident pool), k_feat_stream (the live path:
// append to a per-row ring of normalised frames and emit the spliced rows) and k_feat_denorm (the output side, float64).  k_feat_stream is
// ONE launch, not an append launch and an emit launch: a live round is a few hundred rows, so a launch costs more than the work in it, and
// the emit needs no order against the append because it takes this call's frames from `fresh` (normalising them with the append's own
// expression) and only older frames from the ring, which the window invariant stated at the kernel keeps in other slots.
// Last: k_feat_decode, the archive side (float, double and Kaldi-compressed matrices -> normalised float32 rows, tiled through LDS).
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

// ---- the live path's front end: streaming append and splice on a device-resident ring.  hist [B][H][D] holds each row's NORMALISED frames,
// utterance frame j of row r in slot j mod H (the non-negative remainder); fresh [fresh_rows][D] holds the raw frames that arrived with this
// call, packed over all rows; table [B][6] = (src, app0, napp, emit0, nemit, last) per row.  With C = left + 1 + right, Dout = D * C:
//   append:  hist[r][(app0 + i) mod H][d] = norm(fresh[clamp(src + i, 0, fresh_rows - 1)][d])      i in [0, napp)
//   emit:    out[r, t, c * D + d] = hist'[r][clamp(emit0 + t + c - left, 0, last) mod H][d]         t < min(nemit, T)
//            out[r, t, :]         = +0.0                                                           otherwise (every t when nemit <= 0 or last < 0)
//            lengths[r]           = clamp(nemit, 0, T)
// hist' is the ring after this call's append; negative napp / nemit count as 0, and every napp counts as 0 when fresh_rows == 0.  Where
// napp > H the formula writes a slot more than once and the last write stands: the kernel writes only i in [max(0, napp - H), napp), which
// is that result, each slot written by one lane, and bounds the work per row at H * D whatever the table holds.
//
// ONE launch, not an append launch followed by an emit launch.  A live round is tiny (32 rows x 10 frames in the record of
// profiles/feat_stream.txt): a second launch would cost more than everything the first one computes.  The emit therefore does not read
// this call's frames from the ring, where another lane of the same launch may not have stored them yet: a frame j in
// [app0 + max(0, napp - H), app0 + napp) is taken from `fresh` and normalised on the spot -- the same expression on the same operands as
// the append evaluates, so the same bits as the slot will hold -- and every other frame is read from `hist`.
// The window invariant (the caller's; StreamBank asserts it before each call): last - (emit0 - left) + 1 <= H, with
// emit0 - left <= app0 and app0 + napp - 1 <= last.  The frames the emit reads, j in [max(emit0 - left, 0), last], and the frames the append
// stores, j in [app0, app0 + napp), then lie in ONE run of at most H consecutive frame numbers, which occupy pairwise different slots.  An
// old frame (j < app0) and an appended one (j >= app0) are different numbers of that run, hence different slots: no slot the append writes
// is a slot this call still reads as an old frame, and the launch has no read-after-write order to keep.  Outside the invariant the values
// are not the utterance's (a slot may be read while it is rewritten) but nothing else happens: every slot index is a remainder below H,
// every row of `fresh` is clamped into [0, fresh_rows), and the output row is decided by t and nemit alone.
// Layout: the emit is k_feat_batch's (out as one flat 16-byte aligned array, a lane owns four consecutive elements, the last total % 4 are
// stored one by one).  The append stores single floats: the slots it writes are scattered through the ring (D is no multiple of 4, and a
// quad would cover elements of frames that are not rewritten).  Grid-stride, at most 2048 workgroups of 256; no atomics, no LDS, no
// scratch memory.
struct StreamRow { long long src, app0, napp, lo, emit0, nemit, last; };      // lo: first i the append writes (max(0, napp - H))

__device__ __forceinline__ StreamRow stream_row(const int* __restrict__ table, uint32_t r, long long fresh_rows, uint32_t H) {
  const int* t = table + (size_t)r * 6;
  StreamRow k;
  k.src = t[0]; k.app0 = t[1]; k.napp = fresh_rows > 0 ? max((long long)t[2], 0ll) : 0ll;
  k.lo = max(k.napp - (long long)H, 0ll);
  k.emit0 = t[3]; k.nemit = t[4]; k.last = t[5];
  return k;
}

__device__ __forceinline__ uint32_t stream_slot(long long j, uint32_t H) {
  const long long m = j % (long long)H;
  return (uint32_t)(m < 0 ? m + (long long)H : m);
}

// the raw frame the append stores as utterance frame app0 + i
__device__ __forceinline__ const float* stream_fresh(const float* __restrict__ fresh, long long fresh_rows, const StreamRow& k, long long i, uint32_t D) {
  return fresh + (size_t)min(max(k.src + i, 0ll), fresh_rows - 1) * D;
}

struct StreamSrc { const float* p; bool raw; };      // D floats (null: a zero row); raw: from `fresh`, still to be normalised

__device__ __forceinline__ StreamSrc stream_src(const float* __restrict__ fresh, long long fresh_rows, const float* hist, const StreamRow& k,
                                                const FeatPos& p, int left, uint32_t H, uint32_t D) {
  StreamSrc s;
  s.p = nullptr; s.raw = false;
  if ((long long)p.t >= k.nemit || k.last < 0) return s;
  const long long j = min(max(k.emit0 + (long long)p.t + (long long)p.c - left, 0ll), k.last);      // clamped at the utterance's own first and last frame
  const long long i = j - k.app0;
  if (i >= k.lo && i < k.napp) { s.p = stream_fresh(fresh, fresh_rows, k, i, D); s.raw = true; }
  else s.p = hist + ((size_t)p.b * H + stream_slot(j, H)) * D;
  return s;
}

template <bool NORM>
__device__ __forceinline__ float stream_value(const StreamSrc& s, uint32_t d, const double* __restrict__ mean, const double* __restrict__ stddev) {
  if (!s.p) return 0.f;
  return s.raw ? feat_value<NORM>(s.p, d, mean, stddev) : s.p[d];
}

template <bool NORM>
__global__ __launch_bounds__(256) void k_feat_stream(const float* __restrict__ fresh, long long fresh_rows, const int* __restrict__ table, float* hist,
                                                     int B, uint32_t H, uint32_t T, uint32_t D, int left, uint32_t C,
                                                     const double* __restrict__ mean, const double* __restrict__ stddev, float* __restrict__ out,
                                                     int* __restrict__ lengths, unsigned long long total, unsigned long long ring) {
  const uint32_t Dout = D * C;
  const unsigned long long gid = (unsigned long long)blockIdx.x * 256 + threadIdx.x, stride = (unsigned long long)gridDim.x * 256;
  if (lengths) {
    for (unsigned long long b = gid; b < (unsigned long long)B; b += stride)
      lengths[b] = (int)min(max((long long)table[b * 6 + 4], 0ll), (long long)T);
  }
  // the append: element e of the ring is (r, slot, d); the one i in [lo, lo + H) whose frame app0 + i lives in that slot is stored if i < napp
  if (fresh_rows > 0) {
    for (unsigned long long e = gid; e < ring; e += stride) {       // (ring = B * H * D < 2^32)
      const uint32_t fr = (uint32_t)e / D, d = (uint32_t)e - fr * D, r = fr / H, slot = fr - r * H;
      const StreamRow k = stream_row(table, r, fresh_rows, H);
      if (k.napp <= 0) continue;
      const long long i = k.lo + (long long)stream_slot((long long)slot - k.app0 - k.lo, H);
      if (i < k.napp) hist[e] = feat_value<NORM>(stream_fresh(fresh, fresh_rows, k, i, D), d, mean, stddev);
    }
  }
  // the emit
  const unsigned long long quads = total >> 2;
  for (unsigned long long q = gid; q < quads; q += stride) {
    FeatPos p = feat_pos((uint32_t)(q << 2), T, D, Dout);             // (total < 2^32)
    StreamRow k = stream_row(table, p.b, fresh_rows, H);
    StreamSrc src = stream_src(fresh, fresh_rows, hist, k, p, left, H, D);
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = stream_value<NORM>(src, p.d, mean, stddev);
      if (i == 3) break;
      if (++p.d == D) {
        p.d = 0;
        if (++p.c == C) {
          p.c = 0;
          if (++p.t == T) {                                           // (a quad never runs past the last row: 4 q + 3 < total)
            p.t = 0; ++p.b;
            k = stream_row(table, p.b, fresh_rows, H);
          }
        }
        src = stream_src(fresh, fresh_rows, hist, k, p, left, H, D);
      }
    }
    *reinterpret_cast<float4*>(out + (q << 2)) = make_float4(v[0], v[1], v[2], v[3]);
  }
  const uint32_t tail = (uint32_t)(total & 3);
  if (gid < tail) {
    const unsigned long long e = (quads << 2) + gid;
    const FeatPos p = feat_pos((uint32_t)e, T, D, Dout);
    out[e] = stream_value<NORM>(stream_src(fresh, fresh_rows, hist, stream_row(table, p.b, fresh_rows, H), p, left, H, D), p.d, mean, stddev);
  }
}

void launch_feat_stream(const float* fresh, long long fresh_rows, const int* table, float* hist, int B, int H, int T, int D, int left, int right,
                        const double* mean, const double* stddev, float* out, int* lengths, hipStream_t s) {
  const int C = left + 1 + right;
  const unsigned long long total = (unsigned long long)B * T * D * C, ring = (unsigned long long)B * H * D;
  if (!fresh) fresh_rows = 0;
  // (sized by the emit's quads or the ring's elements, whichever asks for more lanes; one workgroup at least, as in launch_feat_batch)
  const unsigned long long lanes = std::max<unsigned long long>(total >> 2, fresh_rows > 0 ? ring : 0);
  const int grid = (int)std::min<unsigned long long>(2048, std::max<unsigned long long>(1, (lanes + 255) / 256));
  if (mean)
    hipLaunchKernelGGL(k_feat_stream<true>, dim3(grid), dim3(256), 0, s, fresh, fresh_rows, table, hist, B, (uint32_t)H, (uint32_t)T, (uint32_t)D, left,
                       (uint32_t)C, mean, stddev, out, lengths, total, ring);
  else
    hipLaunchKernelGGL(k_feat_stream<false>, dim3(grid), dim3(256), 0, s, fresh, fresh_rows, table, hist, B, (uint32_t)H, (uint32_t)T, (uint32_t)D, left,
                       (uint32_t)C, mean, stddev, out, lengths, total, ring);
}

// ---- the output side: de-normalise G(x) with the label statistics, into the float64 the host path produces.
//   out[b, t, d] = t < len_b ? fl64(fl64((double)y[b, t, d] * stddev[d]) + mean[d]) : 0.0        len_b = lengths ? clamp(lengths[b], 0, T) : T
// The product and the sum are rounded SEPARATELY, as NumPy's `y * stddev + mean` rounds them on a float32 array and float64 statistics:
// contract(off) keeps the compiler from fusing them into one multiply-add, whose single rounding gives other bits.  y is one flat 16-byte
// aligned array of B * T * D floats: a lane owns four consecutive elements, reads them with one 16-byte load and derives (b, t, d) of the
// first by division and of the next three by carrying; the last (B * T * D) % 4 elements are handled one by one.  The entry asks only
// 8-byte alignment of the float64 `out` (a caller may hand in any row of a larger matrix), so the four results leave as 8-byte stores.
// Grid-stride, at most 2048 workgroups of 256; no atomics, no LDS, no scratch memory.
__device__ __forceinline__ double denorm_value(float y, uint32_t d, const double* __restrict__ mean, const double* __restrict__ stddev) {
#pragma clang fp contract(off)
  const double p = (double)y * stddev[d];
  return p + mean[d];
}

__device__ __forceinline__ long long denorm_len(const int* __restrict__ lengths, uint32_t b, uint32_t T) {
  return lengths ? min(max((long long)lengths[b], 0ll), (long long)T) : (long long)T;
}

__global__ __launch_bounds__(256) void k_feat_denorm(const float* __restrict__ y, const int* __restrict__ lengths, uint32_t T, uint32_t D,
                                                     const double* __restrict__ mean, const double* __restrict__ stddev, double* __restrict__ out,
                                                     unsigned long long total) {
  const unsigned long long gid = (unsigned long long)blockIdx.x * 256 + threadIdx.x, stride = (unsigned long long)gridDim.x * 256;
  const unsigned long long quads = total >> 2;
  for (unsigned long long q = gid; q < quads; q += stride) {
    const uint32_t e = (uint32_t)(q << 2), row = e / D;              // (total < 2^32)
    uint32_t d = e - row * D, b = row / T, t = row - b * T;
    long long n = denorm_len(lengths, b, T);
    const float4 in = *reinterpret_cast<const float4*>(y + (q << 2));
    const float v[4] = {in.x, in.y, in.z, in.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      out[(q << 2) + i] = (long long)t < n ? denorm_value(v[i], d, mean, stddev) : 0.0;
      if (i == 3) break;
      if (++d == D) {
        d = 0;
        if (++t == T) {                                               // (a quad never runs past the last row: 4 q + 3 < total)
          t = 0; ++b;
          n = denorm_len(lengths, b, T);
        }
      }
    }
  }
  const uint32_t tail = (uint32_t)(total & 3);
  if (gid < tail) {
    const unsigned long long e = (quads << 2) + gid;
    const uint32_t row = (uint32_t)e / D, d = (uint32_t)e - row * D, b = row / T, t = row - b * T;
    out[e] = (long long)t < denorm_len(lengths, b, T) ? denorm_value(y[e], d, mean, stddev) : 0.0;
  }
}

void launch_feat_denorm(const float* y, const int* lengths, int B, int T, int D, const double* mean, const double* stddev, double* out,
                        hipStream_t s) {
  const unsigned long long total = (unsigned long long)B * T * D;
  const int grid = (int)std::min<unsigned long long>(2048, std::max<unsigned long long>(1, ((total >> 2) + 255) / 256));
  hipLaunchKernelGGL(k_feat_denorm, dim3(grid), dim3(256), 0, s, y, lengths, (uint32_t)T, (uint32_t)D, mean, stddev, out, total);
}

// ---- the archive side: decode a batch of utterances from their Kaldi archive encoding into normalised float32 rows, one launch.
// blob: the matrices' bytes as they lie in the file; seg [B][2] = (byte offset of utterance b's segment in blob, kind); scale [B][2] = (min,
// range) of a compressed matrix's header; n_b = offsets[b + 1] - offsets[b].  Element (j, d) of utterance b, j < n_b:
//   kind 0 (float  [n][D] row-major):  x = (double)f32[j * D + d]
//   kind 1 (double [n][D] row-major):  x = f64[j * D + d]
//   kind 2 (compressed, format 1: 4 * D little-endian uint16 percentiles, then D * n bytes, column-major):
//            p_k = min + ((range * 1.52590218966964e-05) * (double)u16[4 * d + k])                 k = 0 .. 3
//            v   = (double)byte[d * n + j]
//            x   = v < 64 ? p_0 + ((p_1 - p_0) * v) * (1 / 64.0) : v <= 192 ? p_1 + ((p_2 - p_1) * (v - 64)) * (1 / 128.0)
//                                                                            : p_2 + ((p_3 - p_2) * (v - 192)) * (1 / 63.0)
//   out[offsets[b] + j][d] = mean ? (float)((x - mean[d]) / stddev[d]) : (float)x
// which is io/kaldi_ark.py's uint16_to_float and char_to_float, io/features.py's apply_cmvn and the reader's cast, operation by operation
// in IEEE double (contract(off): no multiply-add is formed; 1 / 63.0 is the rounded constant, multiplied): the host path's bits.  The
// decoded value is never rounded to float before it is normalised, which is why decode and CMVN are one kernel.
// Work: a tile is 64 frames x 64 dimensions of one utterance.  Tiles are numbered utterance by utterance, frames-major, and a workgroup
// finds its (utterance, tile) by walking the offset table (B scalar loads): the host knows no n_b, only that sum ceil(n_b / 64) is at most
// ceil(out_rows / 64) + B for utterances that lie in `out` without overlap, which is what the grid-stride loop runs to.
// Layout: a compressed column is contiguous along FRAMES, a row of `out` along DIMENSIONS.  Load phase: a wave owns one column and its 64
// lanes read 64 consecutive bytes (byte loads: a column starts at any byte address), decode, normalise and store the float into the LDS
// tile [frame][dimension], rows padded to 65 floats (the 64 lanes of a store hit 64 different banks).  Store phase: a wave owns one frame
// and its lanes write 64 consecutive floats of the output row.  The four percentiles of a column become doubles once per workgroup and
// column (256 threads = 64 columns x 4), in LDS.  Kinds 0 and 1 are row-major like `out` and go straight through, no LDS.
// Memory safety: the segment offset is clamped into [0, blob_bytes], every byte index into [0, blob_bytes) (the 4- and 8-byte loads into
// [0, blob_bytes - size], aligned down; a blob shorter than the load gives +0.0), every destination row into [0, out_rows); an unknown kind
// writes +0.0; n_b <= 0 writes nothing.  No atomics, no traffic between workgroups, no scratch memory.
constexpr int DEC_TF = 64, DEC_TD = 64;

template <bool NORM>
__device__ __forceinline__ float decode_norm(double x, uint32_t d, const double* __restrict__ mean, const double* __restrict__ stddev) {
#pragma clang fp contract(off)
  if (!NORM) return (float)x;
  const double c = x - mean[d];
  return (float)(c / stddev[d]);
}

__device__ __forceinline__ double decode_byte(const double* __restrict__ p, uint32_t byte) {
#pragma clang fp contract(off)
  const double v = (double)byte;
  if (byte < 64) return p[0] + ((p[1] - p[0]) * v) * (1 / 64.0);
  if (byte <= 192) return p[1] + ((p[2] - p[1]) * (v - 64)) * (1 / 128.0);
  return p[2] + ((p[3] - p[2]) * (v - 192)) * (1 / 63.0);
}

// a byte index clamped into the blob (both ends: sums of garbage table entries may wrap)
__device__ __forceinline__ long long decode_at(long long i, long long blob_bytes) { return min(max(i, 0ll), blob_bytes - 1); }

template <bool NORM>
__global__ __launch_bounds__(256) void k_feat_decode(const uint8_t* __restrict__ blob, long long blob_bytes, const long long* __restrict__ seg,
                                                      const float* __restrict__ scale, const int* __restrict__ offsets, int B, uint32_t D,
                                                      const double* __restrict__ mean, const double* __restrict__ stddev, float* __restrict__ out,
                                                      long long out_rows, unsigned long long row_tiles, uint32_t d_tiles) {
#pragma clang fp contract(off)
  __shared__ float tile[DEC_TF][DEC_TD + 1];
  __shared__ double pc[DEC_TD][4];
  const uint32_t tid = threadIdx.x;
  const unsigned long long total = row_tiles * d_tiles;
  for (unsigned long long w = blockIdx.x; w < total; w += gridDim.x) {
    const unsigned long long rt = w / d_tiles;
    const uint32_t d0 = (uint32_t)(w - rt * d_tiles) * DEC_TD;
    // which utterance row tile rt belongs to (uniform over the workgroup)
    int b = 0;
    unsigned long long first = 0;
    long long n = 0, rows = 0;
    for (; b < B; ++b) {
      n = max((long long)offsets[b + 1] - (long long)offsets[b], 0ll);
      rows = min(n, out_rows);
      const unsigned long long t = ((unsigned long long)rows + DEC_TF - 1) / DEC_TF;
      if (rt < first + t) break;
      first += t;
    }
    if (b == B) break;                                                // (rt grows with w: no later tile of this workgroup exists either)
    const long long j0 = (long long)(rt - first) * DEC_TF, off = offsets[b];
    const long long s = min(max(seg[2 * (size_t)b], 0ll), blob_bytes), kind = seg[2 * (size_t)b + 1];
    const uint32_t nf = (uint32_t)min((long long)DEC_TF, rows - j0), nd = min((uint32_t)DEC_TD, D - d0);
    if (kind == 2) {
      {
        const uint32_t col = tid >> 2, k = tid & 3;
        if (col < nd) {
          const long long i = s + 8ll * (d0 + col) + 2 * k;
          const uint32_t u = (uint32_t)blob[decode_at(i, blob_bytes)] | ((uint32_t)blob[decode_at(i + 1, blob_bytes)] << 8);
          pc[col][k] = (double)scale[2 * (size_t)b] + (((double)scale[2 * (size_t)b + 1] * 1.52590218966964e-05) * (double)u);
        }
      }
      __syncthreads();
      const long long payload = s + 8ll * D;
      for (uint32_t e = tid; e < DEC_TF * DEC_TD; e += 256) {       // a wave: 64 frames of one column
        const uint32_t jj = e & (DEC_TF - 1), dd = e / DEC_TF;
        if (jj < nf && dd < nd) {
          const long long i = payload + (long long)(d0 + dd) * n + j0 + jj;
          tile[jj][dd] = decode_norm<NORM>(decode_byte(pc[dd], blob[decode_at(i, blob_bytes)]), d0 + dd, mean, stddev);
        }
      }
      __syncthreads();
      for (uint32_t e = tid; e < DEC_TF * DEC_TD; e += 256) {       // a wave: 64 dimensions of one frame
        const uint32_t dd = e & (DEC_TD - 1), jj = e / DEC_TD;
        if (jj < nf && dd < nd) {
          const long long row = min(max(off + j0 + jj, 0ll), out_rows - 1);
          out[(size_t)row * D + d0 + dd] = tile[jj][dd];
        }
      }
      __syncthreads();                                                // (tile and pc are rewritten by the next tile of this workgroup)
      continue;
    }
    const long long size = kind == 0 ? 4 : 8;
    const bool known = (kind == 0 || kind == 1) && blob_bytes >= size;
    for (uint32_t e = tid; e < DEC_TF * DEC_TD; e += 256) {
      const uint32_t dd = e & (DEC_TD - 1), jj = e / DEC_TD;
      if (jj < nf && dd < nd) {
        float v = 0.f;
        if (known) {
          const long long i = min(max(s + size * ((j0 + jj) * (long long)D + d0 + dd), 0ll), blob_bytes - size) & ~(size - 1);
          const double x = kind == 0 ? (double)*reinterpret_cast<const float*>(blob + i) : *reinterpret_cast<const double*>(blob + i);
          v = decode_norm<NORM>(x, d0 + dd, mean, stddev);
        }
        const long long row = min(max(off + j0 + jj, 0ll), out_rows - 1);
        out[(size_t)row * D + d0 + dd] = v;
      }
    }
  }
}

void launch_feat_decode(const uint8_t* blob, long long blob_bytes, const long long* seg, const float* scale, const int* offsets, int B, int D,
                        const double* mean, const double* stddev, float* out, long long out_rows, hipStream_t s) {
  const unsigned long long row_tiles = ((unsigned long long)out_rows + DEC_TF - 1) / DEC_TF + (unsigned long long)B;
  const uint32_t d_tiles = ((uint32_t)D + DEC_TD - 1) / DEC_TD;
  const int grid = (int)std::min<unsigned long long>(16384, row_tiles * d_tiles);
  if (mean)
    hipLaunchKernelGGL(k_feat_decode<true>, dim3(grid), dim3(256), 0, s, blob, blob_bytes, seg, scale, offsets, B, (uint32_t)D, mean, stddev, out,
                       out_rows, row_tiles, d_tiles);
  else
    hipLaunchKernelGGL(k_feat_decode<false>, dim3(grid), dim3(256), 0, s, blob, blob_bytes, seg, scale, offsets, B, (uint32_t)D, mean, stddev, out,
                       out_rows, row_tiles, d_tiles);
}

}  // namespace rsr
