// capi_front.cpp -- the product's handle-free entries of include/rsrgan.h: the device front end (rsrgan_feat_*, rsrgan_wave_*) and the
// histograms (rsrgan_hist*).  Every refusal returns before the first HIP call and names its entry and argument in rsrgan_last_error().
#include "capi_common.h"

typedef unsigned long long ull;
// flat indices are divided in 32 bits (feat.hip): a product of positive 31-bit factors above 2^32 - 1, no partial product overflowing before it is found
static bool over32(ull a, ull b, ull c = 1, ull d = 1) { const ull lim = 0xFFFFFFFFull; return a * b > lim || a * b * c > lim || a * b * c * d > lim; }

// refusal groups that several entries word alike, as capi_ops.cpp's OP_CONV_SHAPE: `who` names the entry, the arguments keep their names
#define FE_STATS_PAIR(who) OP_REFUSE((mean == nullptr) != (stddev == nullptr), who ": mean and stddev must both be given or both be null")
#define FE_CONTEXT(who) \
  OP_REFUSE(left < 0 || right < 0, who ": negative context (left %d, right %d)", left, right); \
  OP_REFUSE(left > 1024 || right > 1024, who ": context above the entry's 1024 (left %d, right %d)", left, right)
#define FE_PCM(who) \
  OP_REFUSE(kind != 0 && kind != 1, who ": kind = %d is neither 0 (int16) nor 1 (float32)", kind); \
  OP_REFUSE((size_t)pcm & (kind ? 3 : 1), who ": pcm not aligned to its %d-byte samples", kind ? 4 : 2)
#define FE_FRAMING(who) \
  OP_REFUSE(P < 64 || P > 2048 || (P & (P - 1)), who ": P = %d is no power of two in [64, 2048]", P); \
  OP_REFUSE(S < 1 || N < S || P < N, who ": N = %d, S = %d, P = %d outside 1 <= S <= N <= P", N, S, P); \
  OP_REFUSE(!(preemph >= 0.f && preemph <= 1.f), who ": preemph = %g outside [0, 1]", (double)preemph)
#define FE_INDEX_BTD(who) \
  OP_REFUSE(over32(B, T, D, left + 1 + right), who ": B x T x D x (left + 1 + right) = %d x %d x %d x %d above the entry's 2^32 - 1 elements", \
            B, T, D, left + 1 + right)
#define FE_ROWS_D(who, rows) OP_REFUSE((ull)rows > ((1ull << 40) / (ull)D), who ": " #rows " x D = %lld x %d above the entry's 2^40", (long long)rows, D)

extern "C" {

// ---- the feature front end (feat.hip): no handle, one launch on the caller's stream
int rsrgan_feat_batch(const float* raw, int64_t raw_rows, const int32_t* offsets, int32_t B, int32_t T, int32_t D, int32_t left, int32_t right,
                      const double* mean, const double* stddev, float* out, int32_t* lengths, void* stream) {
  OP_REFUSE(!raw || !offsets || !out, "feat_batch: null pointer (raw, offsets or out)");
  FE_STATS_PAIR("feat_batch");
  OP_REFUSE(((size_t)raw & 15) || ((size_t)out & 15), "feat_batch: raw or out not 16-byte aligned");
  OP_REFUSE(((size_t)offsets & 3) || ((size_t)lengths & 3), "feat_batch: offsets or lengths not 4-byte aligned");
  OP_REFUSE(((size_t)mean & 7) || ((size_t)stddev & 7), "feat_batch: mean or stddev not 8-byte aligned");
  OP_REFUSE(B < 1 || T < 1 || D < 1 || raw_rows < 1, "feat_batch: B, T, D, raw_rows must be positive (got %d, %d, %d, %lld)", B, T, D,
            (long long)raw_rows);
  FE_CONTEXT("feat_batch");
  FE_INDEX_BTD("feat_batch");
  FE_ROWS_D("feat_batch", raw_rows);
  launch_feat_batch(raw, (long long)raw_rows, offsets, B, T, D, left, right, mean, stddev, out, lengths, (hipStream_t)stream);
  OP_LAUNCHED("feat_batch");
}

int rsrgan_feat_frames(const float* pool, int64_t pool_rows, const int32_t* picks, int32_t N, int32_t D, int32_t left, int32_t right,
                       const double* mean, const double* stddev, float* out, void* stream) {
  OP_REFUSE(!pool || !picks || !out, "feat_frames: null pointer (pool, picks or out)");
  FE_STATS_PAIR("feat_frames");
  OP_REFUSE(((size_t)pool & 15) || ((size_t)out & 15), "feat_frames: pool or out not 16-byte aligned");
  OP_REFUSE((size_t)picks & 3, "feat_frames: picks not 4-byte aligned");
  OP_REFUSE(((size_t)mean & 7) || ((size_t)stddev & 7), "feat_frames: mean or stddev not 8-byte aligned");
  OP_REFUSE(N < 1 || D < 1 || pool_rows < 1, "feat_frames: N, D, pool_rows must be positive (got %d, %d, %lld)", N, D, (long long)pool_rows);
  FE_CONTEXT("feat_frames");
  OP_REFUSE(over32(N, D, left + 1 + right), "feat_frames: N x D x (left + 1 + right) = %d x %d x %d above the entry's 2^32 - 1 elements", N, D, left + 1 + right);
  FE_ROWS_D("feat_frames", pool_rows);
  launch_feat_frames(pool, (long long)pool_rows, picks, N, D, left, right, mean, stddev, out, (hipStream_t)stream);
  OP_LAUNCHED("feat_frames");
}

int rsrgan_feat_stream(const float* fresh, int64_t fresh_rows, const int32_t* table, float* hist, int32_t B, int32_t H, int32_t T, int32_t D,
                       int32_t left, int32_t right, const double* mean, const double* stddev, float* out, int32_t* lengths, void* stream) {
  OP_REFUSE(!table || !hist || !out, "feat_stream: null pointer (table, hist or out)");
  OP_REFUSE(fresh_rows < 0, "feat_stream: fresh_rows = %lld is negative", (long long)fresh_rows);
  OP_REFUSE(!fresh && fresh_rows != 0, "feat_stream: null pointer (fresh) with fresh_rows = %lld: fresh may be null only when fresh_rows is 0",
            (long long)fresh_rows);
  FE_STATS_PAIR("feat_stream");
  OP_REFUSE(((size_t)fresh & 15) || ((size_t)hist & 15) || ((size_t)out & 15), "feat_stream: fresh, hist or out not 16-byte aligned");
  OP_REFUSE(((size_t)table & 3) || ((size_t)lengths & 3), "feat_stream: table or lengths not 4-byte aligned");
  OP_REFUSE(((size_t)mean & 7) || ((size_t)stddev & 7), "feat_stream: mean or stddev not 8-byte aligned");
  OP_REFUSE(B < 1 || H < 1 || T < 1 || D < 1, "feat_stream: B, H, T, D must be positive (got %d, %d, %d, %d)", B, H, T, D);
  FE_CONTEXT("feat_stream");
  FE_INDEX_BTD("feat_stream");
  OP_REFUSE(over32(B, H, D), "feat_stream: B x H x D = %d x %d x %d above the entry's 2^32 - 1 elements", B, H, D);
  FE_ROWS_D("feat_stream", fresh_rows);
  launch_feat_stream(fresh, (long long)fresh_rows, table, hist, B, H, T, D, left, right, mean, stddev, out, lengths, (hipStream_t)stream);
  OP_LAUNCHED("feat_stream");
}

int rsrgan_feat_denorm(const float* y, const int32_t* lengths, int32_t B, int32_t T, int32_t D, const double* mean, const double* stddev,
                       double* out, void* stream) {
  OP_REFUSE(!y || !out, "feat_denorm: null pointer (y or out)");
  OP_REFUSE(!mean || !stddev, "feat_denorm: null pointer (mean or stddev): both are needed");
  OP_REFUSE((size_t)y & 15, "feat_denorm: y not 16-byte aligned");
  OP_REFUSE((size_t)lengths & 3, "feat_denorm: lengths not 4-byte aligned");
  OP_REFUSE(((size_t)mean & 7) || ((size_t)stddev & 7) || ((size_t)out & 7), "feat_denorm: mean, stddev or out not 8-byte aligned");
  OP_REFUSE(B < 1 || T < 1 || D < 1, "feat_denorm: B, T, D must be positive (got %d, %d, %d)", B, T, D);
  OP_REFUSE(over32(B, T, D), "feat_denorm: B x T x D = %d x %d x %d above the entry's 2^32 - 1 elements", B, T, D);
  launch_feat_denorm(y, lengths, B, T, D, mean, stddev, out, (hipStream_t)stream);
  OP_LAUNCHED("feat_denorm");
}

int rsrgan_feat_decode(const uint8_t* blob, int64_t blob_bytes, const int64_t* seg, const float* scale, const int32_t* offsets, int32_t B, int32_t D,
                       const double* mean, const double* stddev, float* out, int64_t out_rows, void* stream) {
  OP_REFUSE(!blob || !seg || !offsets || !out, "feat_decode: null pointer (blob, seg, offsets or out)");
  OP_REFUSE(!scale, "feat_decode: null pointer (scale): it is always needed, the kinds are not visible to the host");
  FE_STATS_PAIR("feat_decode");
  OP_REFUSE(((size_t)blob & 15) || ((size_t)out & 15), "feat_decode: blob or out not 16-byte aligned");
  OP_REFUSE(((size_t)seg & 7) || ((size_t)mean & 7) || ((size_t)stddev & 7), "feat_decode: seg, mean or stddev not 8-byte aligned");
  OP_REFUSE(((size_t)scale & 3) || ((size_t)offsets & 3), "feat_decode: scale or offsets not 4-byte aligned");
  OP_REFUSE(B < 1 || D < 1 || blob_bytes < 1 || out_rows < 1, "feat_decode: B, D, blob_bytes, out_rows must be positive (got %d, %d, %lld, %lld)", B,
            D, (long long)blob_bytes, (long long)out_rows);
  FE_ROWS_D("feat_decode", out_rows);
  launch_feat_decode(blob, (long long)blob_bytes, reinterpret_cast<const long long*>(seg), scale, offsets, B, D, mean, stddev, out,
                     (long long)out_rows, (hipStream_t)stream);
  OP_LAUNCHED("feat_decode");
}

// ---- the waveform front end (wave.hip): no handle, one launch on the caller's stream
int rsrgan_feat_wave(const void* pcm, int32_t kind, int64_t n_samples, const int64_t* seg, const int32_t* offsets, int32_t B, int32_t N, int32_t S,
                     int32_t P, float preemph, const float* window, const float* twiddle, float* out, int64_t out_rows, void* stream) {
  OP_REFUSE(!pcm || !seg || !offsets || !out, "feat_wave: null pointer (pcm, seg, offsets or out)");
  OP_REFUSE(!window || !twiddle, "feat_wave: null pointer (window or twiddle)");
  FE_PCM("feat_wave");
  OP_REFUSE((size_t)out & 15, "feat_wave: out not 16-byte aligned");
  OP_REFUSE((size_t)seg & 7, "feat_wave: seg not 8-byte aligned");
  OP_REFUSE(((size_t)offsets & 3) || ((size_t)window & 3) || ((size_t)twiddle & 3), "feat_wave: offsets, window or twiddle not 4-byte aligned");
  OP_REFUSE(B < 1 || n_samples < 1 || out_rows < 1, "feat_wave: B, n_samples, out_rows must be positive (got %d, %lld, %lld)", B,
            (long long)n_samples, (long long)out_rows);
  FE_FRAMING("feat_wave");
  OP_REFUSE((ull)out_rows > ((1ull << 40) / (ull)(P / 2 + 1)), "feat_wave: out_rows x (P / 2 + 1) = %lld x %d above the entry's 2^40", (long long)out_rows, P / 2 + 1);
  launch_feat_wave(pcm, kind, (long long)n_samples, reinterpret_cast<const long long*>(seg), offsets, B, N, S, P, preemph, window, twiddle, out,
                   (long long)out_rows, (hipStream_t)stream);
  OP_LAUNCHED("feat_wave");
}

int rsrgan_feat_mfcc(const void* pcm, int32_t kind, int64_t n_samples, const int64_t* seg, const int32_t* offsets, int32_t B, int32_t N, int32_t S,
                     int32_t P, float preemph, const float* window, const float* twiddle, const int32_t* mel_seg, const float* mel_w, int32_t nnz,
                     int32_t M, const float* dct, int32_t C, float* out, int64_t out_rows, void* stream) {
  OP_REFUSE(!pcm || !seg || !offsets || !out, "feat_mfcc: null pointer (pcm, seg, offsets or out)");
  OP_REFUSE(!window || !twiddle, "feat_mfcc: null pointer (window or twiddle)");
  OP_REFUSE(!mel_seg || !mel_w, "feat_mfcc: null pointer (mel_seg or mel_w)");
  FE_PCM("feat_mfcc");
  OP_REFUSE((size_t)out & 15, "feat_mfcc: out not 16-byte aligned");
  OP_REFUSE((size_t)seg & 7, "feat_mfcc: seg not 8-byte aligned");
  OP_REFUSE(((size_t)offsets & 3) || ((size_t)window & 3) || ((size_t)twiddle & 3), "feat_mfcc: offsets, window or twiddle not 4-byte aligned");
  OP_REFUSE(((size_t)mel_seg & 3) || ((size_t)mel_w & 3) || ((size_t)dct & 3), "feat_mfcc: mel_seg, mel_w or dct not 4-byte aligned");
  OP_REFUSE(B < 1 || n_samples < 1 || out_rows < 1, "feat_mfcc: B, n_samples, out_rows must be positive (got %d, %lld, %lld)", B,
            (long long)n_samples, (long long)out_rows);
  FE_FRAMING("feat_mfcc");
  OP_REFUSE(M < 1 || M > 128, "feat_mfcc: M = %d outside [1, 128]", M);
  OP_REFUSE(C < 0 || C > M, "feat_mfcc: C = %d outside [0, M = %d]", C, M);
  OP_REFUSE(nnz < 1 || nnz > 8192, "feat_mfcc: nnz = %d outside [1, 8192]", nnz);
  OP_REFUSE(C != 0 && !dct, "feat_mfcc: null pointer (dct) with C = %d: only C = 0 (log-mel output) takes none", C);
  OP_REFUSE(C == 0 && dct, "feat_mfcc: dct given with C = 0: the log-mel output takes no DCT table");
  const size_t lds = mfcc_lds_bytes(N, S, P, M, C, nnz);
  OP_REFUSE(lds > 65536, "feat_mfcc: N = %d, S = %d, P = %d, M = %d, C = %d, nnz = %d need %zu bytes of LDS, above the entry's 65536", N, S, P, M, C,
            nnz, lds);
  OP_REFUSE((ull)out_rows > ((1ull << 40) / (ull)(C ? C : M)), "feat_mfcc: out_rows x width = %lld x %d above the entry's 2^40", (long long)out_rows, C ? C : M);
  launch_feat_mfcc(pcm, kind, (long long)n_samples, reinterpret_cast<const long long*>(seg), offsets, B, N, S, P, preemph, window, twiddle, mel_seg,
                   mel_w, nnz, M, dct, C, out, (long long)out_rows, (hipStream_t)stream);
  OP_LAUNCHED("feat_mfcc");
}

int rsrgan_feat_wave_frames(int32_t P) { return (P >= 64 && P <= 2048 && !(P & (P - 1))) ? wave_frames(P) : 0; }

// ---- reverberation on the device (reverb.hip): no handle, no allocation; four launches on the caller's stream
static bool reverb_sizes_ok(int32_t B, int64_t n_max, int64_t L_max, int32_t C) {
  return B >= 1 && B <= 65535 && n_max >= 1 && n_max <= ((int64_t)1 << 28) && L_max >= 0 && L_max <= ((int64_t)1 << 24) && C >= 64 && C <= 2048 &&
         !(C & (C - 1));
}

int64_t rsrgan_wave_reverb_work(int32_t B, int64_t n_max, int64_t L_max, int32_t C) {
  return reverb_sizes_ok(B, n_max, L_max, C) ? (int64_t)reverb_work_bytes(B, (long long)n_max, (long long)L_max, C) : 0;
}

int rsrgan_wave_reverb(const void* pcm, int32_t kind, int64_t n_samples, const int64_t* seg, const float* rir, int64_t n_taps, const int64_t* rir_seg,
                       const float* noise, int64_t n_noise, const int64_t* noise_seg, const float* noise_pow, const int32_t* sel, const float* snr,
                       int32_t B, int32_t R, int32_t V, int32_t C, const float* twiddle, int32_t flags, float* out, int64_t out_samples,
                       const int64_t* out_seg, float* gains, void* work, int64_t work_bytes, void* stream) {
  OP_REFUSE(!pcm || !seg || !sel || !snr, "wave_reverb: null pointer (pcm, seg, sel or snr)");
  OP_REFUSE(!out || !out_seg, "wave_reverb: null pointer (out or out_seg)");
  OP_REFUSE(!twiddle || !work, "wave_reverb: null pointer (twiddle or work)");
  OP_REFUSE(B < 1 || B > 65535, "wave_reverb: B = %d outside [1, 65535]", B);
  OP_REFUSE(R < 0 || R > (1 << 20), "wave_reverb: R = %d outside [0, 2^20]", R);
  OP_REFUSE(V < 0 || V > (1 << 20), "wave_reverb: V = %d outside [0, 2^20]", V);
  OP_REFUSE(R > 0 && (!rir || !rir_seg), "wave_reverb: null pointer (rir or rir_seg) with R = %d: only R = 0 takes none", R);
  OP_REFUSE(V > 0 && (!noise || !noise_seg || !noise_pow), "wave_reverb: null pointer (noise, noise_seg or noise_pow) with V = %d: only V = 0 takes none", V);
  FE_PCM("wave_reverb");
  OP_REFUSE((size_t)work & 15, "wave_reverb: work not 16-byte aligned");
  OP_REFUSE(((size_t)seg & 7) || ((size_t)rir_seg & 7) || ((size_t)noise_seg & 7) || ((size_t)out_seg & 7),
            "wave_reverb: seg, rir_seg, noise_seg or out_seg not 8-byte aligned");
  OP_REFUSE(((size_t)rir & 3) || ((size_t)noise & 3) || ((size_t)noise_pow & 3), "wave_reverb: rir, noise or noise_pow not 4-byte aligned");
  OP_REFUSE(((size_t)sel & 3) || ((size_t)snr & 3) || ((size_t)twiddle & 3), "wave_reverb: sel, snr or twiddle not 4-byte aligned");
  OP_REFUSE(((size_t)out & 3) || ((size_t)gains & 3), "wave_reverb: out or gains not 4-byte aligned");
  OP_REFUSE(n_samples < 1 || out_samples < 1, "wave_reverb: n_samples, out_samples must be positive (got %lld, %lld)", (long long)n_samples,
            (long long)out_samples);
  OP_REFUSE(n_samples > ((int64_t)1 << 40) || out_samples > ((int64_t)1 << 40), "wave_reverb: n_samples or out_samples above the entry's 2^40 (got %lld, %lld)",
            (long long)n_samples, (long long)out_samples);
  OP_REFUSE(n_taps < (R > 0) || n_taps > ((int64_t)1 << 40), "wave_reverb: n_taps = %lld outside [%d, 2^40] with R = %d", (long long)n_taps, R > 0, R);
  OP_REFUSE(n_noise < (V > 0) || n_noise > ((int64_t)1 << 40), "wave_reverb: n_noise = %lld outside [%d, 2^40] with V = %d", (long long)n_noise, V > 0, V);
  OP_REFUSE(C < 64 || C > 2048 || (C & (C - 1)), "wave_reverb: C = %d is no power of two in [64, 2048]", C);
  OP_REFUSE(flags < 0 || flags > 3, "wave_reverb: flags = %d holds bits other than 1 (shift) and 2 (normalize)", flags);
  const int64_t least = (int64_t)reverb_work_bytes(B, 1, 1, C);
  OP_REFUSE(work_bytes < least, "wave_reverb: work_bytes = %lld below the %lld bytes B = %d utterances of one sample need at C = %d", (long long)work_bytes,
            (long long)least, B, C);
  RevArgs a{pcm, kind, (long long)n_samples, reinterpret_cast<const long long*>(seg), rir, (long long)n_taps, reinterpret_cast<const long long*>(rir_seg),
            noise, (long long)n_noise, reinterpret_cast<const long long*>(noise_seg), noise_pow, sel, snr, B, R, V, (uint32_t)C, twiddle, flags, out,
            (long long)out_samples, reinterpret_cast<const long long*>(out_seg), gains, static_cast<unsigned char*>(work), 0ull};
  launch_wave_reverb(a, (size_t)work_bytes, (hipStream_t)stream);
  OP_LAUNCHED("wave_reverb");
}

// ---- audio out on the device (synth.hip): no handle, no allocation; four launches on the caller's stream
int rsrgan_wave_synth_chunk(void) { return synth_chunk(); }

int64_t rsrgan_wave_synth_work(int32_t B, int64_t lps_rows, int64_t out_samples, int32_t N) {
  const int64_t lim = (int64_t)1 << 40;
  if (B < 1 || B > 65535 || lps_rows < 1 || lps_rows > lim || out_samples < 1 || out_samples > lim || N < 1 || N > 2048) return 0;
  return (int64_t)sizeof(float) * (int64_t)synth_work_floats(B, (long long)lps_rows, (long long)out_samples, N);
}

int rsrgan_wave_synth(const void* pcm, int32_t kind, int64_t n_samples, const int64_t* seg, const int32_t* offsets, const float* lps,
                      int64_t lps_rows, int32_t B, int32_t N, int32_t S, int32_t P, float preemph, const float* window, const float* twiddle,
                      float* out, int64_t out_samples, const int64_t* out_seg, void* work, int64_t work_bytes, void* stream) {
  OP_REFUSE(!pcm || !seg || !offsets || !out, "wave_synth: null pointer (pcm, seg, offsets or out)");
  OP_REFUSE(!window || !twiddle, "wave_synth: null pointer (window or twiddle)");
  OP_REFUSE(!lps || !out_seg || !work, "wave_synth: null pointer (lps, out_seg or work)");
  FE_PCM("wave_synth");
  OP_REFUSE(((size_t)lps & 15) || ((size_t)work & 15), "wave_synth: lps or work not 16-byte aligned");
  OP_REFUSE(((size_t)seg & 7) || ((size_t)out_seg & 7), "wave_synth: seg or out_seg not 8-byte aligned");
  OP_REFUSE(((size_t)offsets & 3) || ((size_t)window & 3) || ((size_t)twiddle & 3) || ((size_t)out & 3),
            "wave_synth: offsets, window, twiddle or out not 4-byte aligned");
  OP_REFUSE(B < 1 || B > 65535, "wave_synth: B = %d outside [1, 65535]", B);
  OP_REFUSE(n_samples < 1, "wave_synth: n_samples must be positive (got %lld)", (long long)n_samples);
  OP_REFUSE(n_samples > ((int64_t)1 << 40), "wave_synth: n_samples = %lld above the entry's 2^40", (long long)n_samples);
  OP_REFUSE(lps_rows < 1 || lps_rows > ((int64_t)1 << 40), "wave_synth: lps_rows = %lld outside [1, 2^40]", (long long)lps_rows);
  OP_REFUSE(out_samples < 1 || out_samples > ((int64_t)1 << 40), "wave_synth: out_samples = %lld outside [1, 2^40]", (long long)out_samples);
  FE_FRAMING("wave_synth");
  const int64_t need = rsrgan_wave_synth_work(B, lps_rows, out_samples, N);
  OP_REFUSE(work_bytes < need, "wave_synth: work_bytes = %lld below the %lld bytes rsrgan_wave_synth_work(%d, %lld, %lld, %d) gives",
            (long long)work_bytes, (long long)need, B, (long long)lps_rows, (long long)out_samples, N);
  SynArgs a{pcm, kind, (long long)n_samples, reinterpret_cast<const long long*>(seg), offsets, lps, (long long)lps_rows, B, (uint32_t)N, (uint32_t)S,
            (uint32_t)P, preemph, window, twiddle, out, (long long)out_samples, reinterpret_cast<const long long*>(out_seg),
            static_cast<float*>(work), 0ll, 0u};
  launch_wave_synth(a, (hipStream_t)stream);
  OP_LAUNCHED("wave_synth");
}

// ---- TensorBoard histograms on the device (hist.hip): no handle; two launches on the caller's stream
int rsrgan_hist_limits(double* out, int32_t* n) {
  OP_REFUSE(!n, "hist_limits: null pointer (n)");
  return guard("rsrgan_hist_limits", [&]() -> int {
    const std::vector<double>& t = hist_limits();
    *n = (int32_t)t.size();
    if (out) std::memcpy(out, t.data(), t.size() * sizeof(double));
    return RSRGAN_OK;
  });
}

int rsrgan_hist(int32_t n, const float* const* x, const int64_t* dims, double* out, void* stream) {
  OP_REFUSE(n < 1, "hist: n = %d: at least one tensor is needed", n);
  OP_REFUSE(n > HIST_MAX_TENSORS, "hist: n = %d above the entry's %d tensors per call", n, HIST_MAX_TENSORS);
  OP_REFUSE(!x || !dims || !out, "hist: null pointer (x, dims or out)");
  OP_REFUSE((size_t)out & 7, "hist: out not 8-byte aligned");
  HistView v[HIST_MAX_TENSORS];
  for (int i = 0; i < n; ++i) {
    const int64_t rows = dims[3 * i], cols = dims[3 * i + 1], ld = dims[3 * i + 2];
    OP_REFUSE(rows < 0 || cols < 0 || ld < 0, "hist: tensor %d: negative size (rows %lld, cols %lld, ld %lld)", i, (long long)rows, (long long)cols,
              (long long)ld);
    OP_REFUSE(ld < cols, "hist: tensor %d: leading dimension ld = %lld below its row of %lld", i, (long long)ld, (long long)cols);
    const int64_t lim = 0x7FFFFFFF;                        // element indices are 32 bits wide (hist.hip)
    OP_REFUSE(rows > lim || cols > lim || (rows && cols > lim / rows), "hist: tensor %d: rows x cols = %lld x %lld above the entry's 2^31 - 1 elements",
              i, (long long)rows, (long long)cols);
    OP_REFUSE(ld > ((int64_t)1 << 40), "hist: tensor %d: ld = %lld above the entry's 2^40", i, (long long)ld);
    const bool empty = rows == 0 || cols == 0;
    OP_REFUSE(!x[i] && !empty, "hist: tensor %d: null pointer (x[%d]) with %lld x %lld elements: only a tensor without elements may be null", i, i,
              (long long)rows, (long long)cols);
    OP_REFUSE((size_t)x[i] & 3, "hist: tensor %d: x[%d] not 4-byte aligned", i, i);
    v[i] = HistView{empty ? nullptr : x[i], (long long)ld, 1, empty ? 0u : (unsigned)rows, empty ? 0u : (unsigned)cols, 0};
  }
  if (!launch_hist(n, v, 0.f, 0.f, out, (hipStream_t)stream)) { set_error("hist: the launches' device memory or stream order could not be set up"); return RSRGAN_ERR_HIP; }
  OP_LAUNCHED("hist");
}

}  // extern "C"
