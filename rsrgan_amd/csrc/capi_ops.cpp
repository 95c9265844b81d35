// capi_ops.cpp -- the unit-test operator entries of include/rsrgan.h (rsrgan_op_*): the model's own host launch functions on
// caller-owned buffers, no handle.  First the positional-argument entries (launch floor, gemm, column sums, bnl_fold, conv, bn), then
// the table-form ones (op, ptrs, dims, fl: segan, chunks, update, step_elem, layout).  The product's entries are capi.cpp's and capi_front.cpp's.
#include "capi_common.h"

extern "C" {

int rsrgan_op_launch_floor(int32_t n, int32_t mode, double* us_per_launch, void* stream) {
  if (n <= 0 || !us_per_launch) { set_error("op_launch_floor: bad argument"); return RSRGAN_ERR_INVALID; }
  // captured once and replayed, like the step's segments (an eager chain is host-bound at 3-5 us per launch)
  static float* buf = nullptr;
  if (!buf && hipMalloc((void**)&buf, 2 * 65536 * 4 * sizeof(float)) != hipSuccess) { set_error("hipMalloc failed"); return RSRGAN_ERR_HIP; }
  hipStream_t s = nullptr;
  hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = RSRGAN_ERR_HIP;
  do {
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) break;
    if (hipMemsetAsync(buf, 0, 2 * 65536 * 4 * sizeof(float), s) != hipSuccess) break;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) break;
    launch_floor_chain(buf, buf + 65536 * 4, n, mode, s);
    if (hipStreamEndCapture(s, &g) != hipSuccess) break;
    if (hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) break;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) break;
    if (hipGraphLaunch(ge, s) != hipSuccess) break;                 // warm-up replay
    if (hipEventRecord(e0, s) != hipSuccess || hipGraphLaunch(ge, s) != hipSuccess || hipEventRecord(e1, s) != hipSuccess) break;
    if (hipEventSynchronize(e1) != hipSuccess) break;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) break;
    *us_per_launch = 1e3 * ms / n;
    rc = RSRGAN_OK;
  } while (0);
  if (rc != RSRGAN_OK) set_error("op_launch_floor: HIP call failed");
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (ge) (void)hipGraphExecDestroy(ge);
  if (g) (void)hipGraphDestroy(g);
  if (s) (void)hipStreamDestroy(s);
  (void)stream;
  return rc;
}

// ---- unit-test entries of the operators (tests/test_gpu_gemm.py, test_gpu_wgrad_ops.py, test_op_args.py).  Each goes through the host
// launch function the model calls, with a private workspace of the model's size (Model::gemm_ws_floats: 32 Mi floats -- with less,
// launch_gemm_batch's 192 x 256 form, the one the training step runs, is never taken).  Every argument error returns before the
// first HIP call, so the refusals are testable without a device.
static const size_t g_op_ws_floats = (size_t)32 << 20;
static const size_t g_op_scratch_floats = (size_t)2 << 20;       // column-sum partials (4 layers x 64 slices x 7 x 760 = 1.4 M)
static float* op_ws() {
  static float* ws = nullptr;
  if (!ws && hipMalloc((void**)&ws, g_op_ws_floats * sizeof(float)) != hipSuccess) ws = nullptr;
  return ws;
}
static float* op_scratch() {
  static float* sc = nullptr;
  if (!sc && hipMalloc((void**)&sc, g_op_scratch_floats * sizeof(float)) != hipSuccess) sc = nullptr;
  return sc;
}
struct WorkersScope {            // narrows g_gemm_workers for one call (the step: 224 under DPIPE, 256 otherwise)
  int saved;
  explicit WorkersScope(int w) : saved(g_gemm_workers) { if (w > 0) g_gemm_workers = w; }
  ~WorkersScope() { g_gemm_workers = saved; }
};

int rsrgan_op_gemm(const float* A, int32_t lda, int32_t a_kc, const float* B, int32_t ldb, int32_t b_kc, float* C, int32_t ldc,
                   int32_t M, int32_t N, int32_t K, const float* bias, int32_t act, float alpha, int32_t accumulate, void* stream) {
  if (!A || !B || !C || (lda & 3) || (ldb & 3)) { set_error("op_gemm: null pointer or leading dimension not a multiple of 4"); return RSRGAN_ERR_INVALID; }
  float* ws = op_ws();
  launch_gemm(A, lda, a_kc != 0, B, ldb, b_kc != 0, C, ldc, M, N, K, bias, act, alpha, accumulate != 0, (hipStream_t)stream,
              ws, ws ? g_op_ws_floats : 0);
  OP_LAUNCHED("op_gemm");
}

int rsrgan_op_gemm2(const float* A, int32_t lda, int32_t a_kc, const float* A2, int32_t lda2, int32_t M1, const float* B, int32_t ldb,
                    int32_t b_kc, float* C, int32_t ldc, int32_t M, int32_t N, int32_t K, const float* bias, int32_t act, float alpha,
                    int32_t accumulate, int32_t map_rows_per, int64_t map_outer, int64_t map_inner, int32_t workers, int32_t force_cfg,
                    void* stream) {
  OP_REFUSE(!A || !B || !C, "op_gemm2: null pointer (A, B or C)");
  OP_REFUSE(M <= 0 || N <= 0 || K <= 0, "op_gemm2: M, N, K must be positive (got %d, %d, %d)", M, N, K);
  OP_REFUSE((lda & 3) || (ldb & 3) || (ldc & 3) || (A2 && (lda2 & 3)), "op_gemm2: leading dimension not a multiple of 4 (lda %d, lda2 %d, ldb %d, ldc %d)", lda, lda2, ldb, ldc);
  OP_REFUSE(workers < 0 || workers > 256, "op_gemm2: workers = %d outside 0 (default) .. 256", workers);
  OP_REFUSE(force_cfg < -1 || force_cfg > 7, "op_gemm2: force_cfg = %d outside -1 (planner) .. 7", force_cfg);
  OP_REFUSE(map_rows_per < 0, "op_gemm2: row map with rows_per = %d", map_rows_per);
  if (map_rows_per > 0) {
    OP_REFUSE(A2 != nullptr, "op_gemm2: A2 together with a row map");
    OP_REFUSE(b_kc != 0, "op_gemm2: a row map together with b_kcontig");
    OP_REFUSE((map_outer & 3) || (map_inner & 3), "op_gemm2: row map strides not multiples of 4 (outer %lld, inner %lld)", (long long)map_outer, (long long)map_inner);
  }
  if (A2) {
    OP_REFUSE(a_kc != 0, "op_gemm2: A2 together with a_kcontig (the stacked operand is m-contiguous)");
    OP_REFUSE(M1 <= 0 || M1 >= M, "op_gemm2: M1 = %d outside (0, M = %d)", M1, M);
    OP_REFUSE(M1 & 3, "op_gemm2: M1 = %d is not a multiple of 4: every kernel moves the stacked operand in 16-byte chunks", M1);
  }
  float* ws = op_ws();
  {
    WorkersScope wsc(workers);
    const GemmRowMap ma{map_rows_per, (long long)map_outer, (long long)map_inner};
    launch_gemm_mapped(A, lda, ma, A2, lda2, M1, a_kc != 0, B, ldb, b_kc != 0, C, ldc, M, N, K, bias, act, alpha, accumulate != 0,
                       (hipStream_t)stream, ws, ws ? g_op_ws_floats : 0, force_cfg);
  }
  OP_LAUNCHED("op_gemm2");
}

int rsrgan_op_gemm_batch(int32_t nb, const float* const* A, int32_t lda, const float* const* A2, int32_t lda2, int32_t M1,
                         const float* const* B, int32_t ldb, float* const* C, int32_t ldc, int32_t M, int32_t N, int32_t K,
                         int32_t accumulate, int32_t workers, void* stream) {
  OP_REFUSE(nb < 1 || nb > 64, "op_gemm_batch: nb = %d outside 1 .. 64 (more than %d: not applicable)", nb, GEMM_MAXB);
  OP_REFUSE(!A || !B || !C, "op_gemm_batch: null pointer table (A, B or C)");
  for (int b = 0; b < nb; ++b) OP_REFUSE(!A[b] || !B[b] || !C[b] || (A2 && !A2[b]), "op_gemm_batch: null pointer in problem %d", b);
  OP_REFUSE(M <= 0 || N <= 0 || K <= 0, "op_gemm_batch: M, N, K must be positive (got %d, %d, %d)", M, N, K);
  OP_REFUSE((lda & 3) || (ldb & 3) || (ldc & 3) || (A2 && (lda2 & 3)), "op_gemm_batch: leading dimension not a multiple of 4 (lda %d, lda2 %d, ldb %d, ldc %d)", lda, lda2, ldb, ldc);
  OP_REFUSE(workers < 0 || workers > 256, "op_gemm_batch: workers = %d outside 0 (default) .. 256", workers);
  if (A2) {
    OP_REFUSE(M1 <= 0 || M1 >= M, "op_gemm_batch: M1 = %d outside (0, M = %d)", M1, M);
    OP_REFUSE(M1 & 3, "op_gemm_batch: M1 = %d is not a multiple of 4: the kernels move the stacked operand in 16-byte chunks", M1);
  }
  float* ws = op_ws();
  bool ran;
  {
    WorkersScope wsc(workers);
    ran = launch_gemm_batch(nb, A, lda, A2, lda2, M1, B, ldb, C, ldc, M, N, K, accumulate != 0, (hipStream_t)stream, ws, ws ? g_op_ws_floats : 0);
  }
  OP_LAUNCH_OK("op_gemm_batch");
  return ran ? RSRGAN_OK : RSRGAN_OP_NOT_APPLICABLE;
}

int rsrgan_op_gemm16_batch(int32_t n, const float* const* A, int32_t lda, const float* const* A2, int32_t lda2, int32_t M1,
                           const float* const* B, int32_t ldb, float* const* C, int32_t ldc, int32_t M, int32_t N, int32_t K,
                           int32_t accumulate, void* stream) {
  OP_REFUSE(n < 1 || n > GEMM16_MAXB, "op_gemm16_batch: n = %d outside the table (1 .. %d)", n, GEMM16_MAXB);
  OP_REFUSE(!A || !B || !C, "op_gemm16_batch: null pointer table (A, B or C)");
  for (int p = 0; p < n; ++p) OP_REFUSE(!A[p] || !B[p] || !C[p] || (A2 && !A2[p]), "op_gemm16_batch: null pointer in problem %d", p);
  OP_REFUSE(M <= 0 || N <= 0 || K <= 0, "op_gemm16_batch: M, N, K must be positive (got %d, %d, %d)", M, N, K);
  OP_REFUSE((lda & 3) || (ldb & 3) || (ldc & 3) || (A2 && (lda2 & 3)), "op_gemm16_batch: leading dimension not a multiple of 4 (lda %d, lda2 %d, ldb %d, ldc %d)", lda, lda2, ldb, ldc);
  if (A2) {
    OP_REFUSE(M1 <= 0 || M1 >= M, "op_gemm16_batch: M1 = %d outside (0, M = %d)", M1, M);
    OP_REFUSE(M1 & 3, "op_gemm16_batch: M1 = %d is not a multiple of 4: k_gemm16 loads the stacked operand as float4", M1);
  }
  Gemm16Batch bt{};
  bt.n = n;
  for (int p = 0; p < n; ++p) { bt.A[p] = A[p]; bt.A2[p] = A2 ? A2[p] : nullptr; bt.B[p] = B[p]; bt.C[p] = C[p]; }
  float* ws = op_ws();
  launch_gemm16_batch(bt, lda, lda2, M1, ldb, ldc, M, N, K, accumulate != 0, (hipStream_t)stream, ws, ws ? g_op_ws_floats : 0);
  OP_LAUNCHED("op_gemm16_batch");
}

int rsrgan_op_gemm_last_plan(int32_t out[8]) {
  OP_REFUSE(!out, "op_gemm_last_plan: null pointer");
  const GemmPlanRecord& r = g_gemm_last_plan;
  out[0] = r.cls; out[1] = r.bm; out[2] = r.bn; out[3] = r.W; out[4] = r.n_dp; out[5] = r.fixup; out[6] = r.splits; out[7] = r.Ur;
  return RSRGAN_OK;
}

int rsrgan_op_lstm_colsums(int32_t nb, const float* const* dz, const float* const* cprev, const float* const* ccur, float* const* db,
                           float* const* dwi, float* const* dwf, float* const* dwo, int32_t rows, int32_t H, void* stream) {
  OP_REFUSE(nb < 1 || nb > 4, "op_lstm_colsums: nb = %d outside the table (1 .. 4)", nb);
  OP_REFUSE(!dz || !cprev || !ccur || !db || !dwi || !dwf || !dwo, "op_lstm_colsums: null pointer table");
  for (int p = 0; p < nb; ++p)
    OP_REFUSE(!dz[p] || !cprev[p] || !ccur[p] || !db[p] || !dwi[p] || !dwf[p] || !dwo[p], "op_lstm_colsums: null pointer in layer %d", p);
  OP_REFUSE(rows <= 0 || H <= 0, "op_lstm_colsums: rows and H must be positive (got %d, %d)", rows, H);
  OP_REFUSE((size_t)nb * 64 * 7 * (size_t)H > g_op_scratch_floats, "op_lstm_colsums: nb x 64 x 7 x H = %zu floats of partials exceed the entry's scratch", (size_t)nb * 64 * 7 * (size_t)H);
  float* sc = op_scratch();
  if (!sc) { set_error("op_lstm_colsums: hipMalloc failed"); return RSRGAN_ERR_HIP; }
  if (nb == 1) launch_lstm_colsums(dz[0], cprev[0], ccur[0], db[0], dwi[0], dwf[0], dwo[0], rows, H, sc, (hipStream_t)stream);
  else {
    ColsumsBatch cb{};
    cb.n = nb;
    for (int p = 0; p < nb; ++p) { cb.dz[p] = dz[p]; cb.cprev[p] = cprev[p]; cb.ccur[p] = ccur[p]; cb.db[p] = db[p]; cb.dwi[p] = dwi[p]; cb.dwf[p] = dwf[p]; cb.dwo[p] = dwo[p]; }
    launch_lstm_colsums_batch(cb, rows, H, sc, (hipStream_t)stream);
  }
  OP_LAUNCHED("op_lstm_colsums");
}

int rsrgan_op_colsum(const float* a, int32_t lda, const float* b, int32_t ldb, float* out, int32_t rows, int32_t cols, int32_t tall,
                     void* stream) {
  OP_REFUSE(!a || !out, "op_colsum: null pointer (a or out)");
  OP_REFUSE(rows <= 0 || cols <= 0, "op_colsum: rows and cols must be positive (got %d, %d)", rows, cols);
  OP_REFUSE(lda < cols || (b && ldb < cols), "op_colsum: leading dimension below cols = %d (lda %d, ldb %d)", cols, lda, ldb);
  OP_REFUSE(tall && b, "op_colsum: the tall form has no multiplier b");
  OP_REFUSE((size_t)(tall ? 512 : 64) * (size_t)cols > g_op_scratch_floats, "op_colsum: cols = %d exceeds the entry's scratch", cols);
  float* sc = op_scratch();
  if (!sc) { set_error("op_colsum: hipMalloc failed"); return RSRGAN_ERR_HIP; }
  if (tall) launch_colsum_tall(a, lda, out, rows, cols, sc, g_op_scratch_floats, (hipStream_t)stream);
  else launch_colsum(a, lda, b, ldb, out, rows, cols, sc, (hipStream_t)stream);
  OP_LAUNCHED("op_colsum");
}

int rsrgan_op_bnl_fold(const float* Wx, const float* Wh, const float* const bn[12], const float* bias, int32_t P, int32_t H, float* KxT,
                       int32_t ldI, float* KhT, int32_t ldP, float* bias_f, float* ca, float* cb, void* stream) {
  OP_REFUSE(!Wx || !Wh || !bn || !bias || !KxT || !KhT || !bias_f || !ca || !cb, "op_bnl_fold: null pointer");
  for (int k = 0; k < 12; ++k) OP_REFUSE(!bn[k], "op_bnl_fold: null pointer in bn[%d]", k);
  OP_REFUSE(P <= 0 || H <= 0, "op_bnl_fold: P and H must be positive (got %d, %d)", P, H);
  OP_REFUSE(ldI < P || ldP < P, "op_bnl_fold: leading dimension below P = %d (ldI %d, ldP %d)", P, ldI, ldP);
  OP_REFUSE((long long)H * 4 * (long long)(ldI > ldP ? ldI : ldP) > (1ll << 28), "op_bnl_fold: 4H x ld exceeds the entry's 2^28 floats");
  BnlFold f{};
  f.Wx = Wx; f.Wh = Wh; f.bias = bias;
  for (int k = 0; k < 12; ++k) f.bn[k] = bn[k];
  f.P = P; f.H = H; f.ldI = ldI; f.ldP = ldP; f.eps = 1e-3f;          // (BNLSTMCell.py:20 batch_norm(epsilon=1e-3))
  f.KxT = KxT; f.KhT = KhT; f.bias_f = bias_f; f.ca = ca; f.cb = cb;
  launch_bnl_fold(f, (hipStream_t)stream);
  OP_LAUNCHED("op_bnl_fold");
}

// ---- the implicit-GEMM convolution (conv.hip) through the launch functions Model::rced_forward / rced_backward call
// the prepared filter Ft of one call: grow-only and kept for the life of the thread like op_ws() for the process (a test entry has no
// handle to hang it on); per thread, as the plan record beside it, so two threads never share one
static float* op_conv_ft(size_t floats) {
  static thread_local float* ft = nullptr;
  static thread_local size_t cap = 0;
  if (floats > cap) {
    if (ft) { (void)hipDeviceSynchronize(); (void)hipFree(ft); ft = nullptr; cap = 0; }
    if (hipMalloc((void**)&ft, floats * sizeof(float)) != hipSuccess) { ft = nullptr; return nullptr; }
    cap = floats;
  }
  return ft;
}
static inline int op_pad4(int n) { return (n + 3) & ~3; }
#define OP_CONV_SHAPE(who) \
  OP_REFUSE(C < 1 || N < 1 || S < 1 || W < 1 || fw < 1, who ": C, N, S, W, fw must be positive (got %d, %d, %d, %d, %d)", C, N, S, W, fw); \
  OP_REFUSE(R < 1, who ": R = %d frames", R); \
  OP_REFUSE((long long)R * S * W > (1 << 24), who ": R x S x W = %lld positions exceed the entry's 2^24", (long long)R * S * W)

int rsrgan_op_conv_supported(int32_t C, int32_t N, int32_t S, int32_t W, int32_t fw) {
  OP_REFUSE(C < 1 || N < 1 || S < 1 || W < 1 || fw < 1, "op_conv_supported: C, N, S, W, fw must be positive (got %d, %d, %d, %d, %d)", C, N, S, W, fw);
  return (conv_fwd_supported(C, N, S, W, fw) ? 1 : 0) | (conv_wgrad_supported(C, N, S, W, fw) ? 2 : 0);
}

int64_t rsrgan_op_conv_ws_floats(int32_t C, int32_t R_max, int32_t S, int32_t W, int32_t fw) {
  OP_REFUSE(C < 1 || R_max < 1 || S < 1 || W < 1 || fw < 1, "op_conv_ws_floats: C, R_max, S, W, fw must be positive (got %d, %d, %d, %d, %d)", C, R_max, S, W, fw);
  return (int64_t)conv_wgrad_ws_floats(C, R_max, S, W, fw);
}

int rsrgan_op_conv_fwd(const float* in, int32_t ldc_in, int32_t C, const float* F, int32_t ldf, int32_t flip, const float* bias, int32_t relu,
                       const float* mask, float* out, int32_t ldc_out, int32_t N, int32_t R, int32_t S, int32_t W, int32_t fw, void* stream) {
  OP_REFUSE(!in || !F || !out, "op_conv_fwd: null pointer (in, F or out)");
  OP_CONV_SHAPE("op_conv_fwd");
  OP_REFUSE((ldc_in & 3) || (ldc_out & 3) || (ldf & 3), "op_conv_fwd: leading dimension not a multiple of 4 (ldc_in %d, ldc_out %d, ldf %d)", ldc_in, ldc_out, ldf);
  OP_REFUSE(ldc_in < op_pad4(C) || ldc_out < op_pad4(N) || ldf < (flip ? C : N),
            "op_conv_fwd: leading dimension below its row (ldc_in %d for C = %d, ldc_out %d for N = %d, ldf %d for %d filter columns)", ldc_in, C, ldc_out, N, ldf, flip ? C : N);
  OP_REFUSE(((size_t)in & 15) || ((size_t)out & 15) || ((size_t)mask & 15), "op_conv_fwd: in, out or mask not 16-byte aligned");
  OP_REFUSE((size_t)bias & 15, "op_conv_fwd: bias not 16-byte aligned (k_conv_fwd4 adds it as float4)");
  g_conv_last_plan.n = 0;
  if (!conv_fwd_supported(C, N, S, W, fw)) return RSRGAN_OP_NOT_APPLICABLE;      // (the model: the patch-matrix path)
  float* Ft = op_conv_ft(conv_prep_floats(S, fw, C));
  if (!Ft) { set_error("op_conv_fwd: hipMalloc failed"); return RSRGAN_ERR_HIP; }
  // forward: the layer is C -> N; data gradient (flip): the layer is N -> C, F is its filter and `in` its output gradient
  launch_conv_prep(F, ldf, S, fw, flip ? N : C, flip ? C : N, flip != 0, Ft, (hipStream_t)stream);
  launch_conv_fwd(in, ldc_in, C, Ft, bias, relu != 0, out, ldc_out, N, R, S, W, fw, (hipStream_t)stream, mask);
  OP_LAUNCHED("op_conv_fwd");
}

int rsrgan_op_conv_wgrad(const float* in, int32_t ldc_in, int32_t C, const float* d, int32_t ldc_d, int32_t N, float* dW, int32_t ldw, float* db,
                         float* ws, int64_t ws_floats, int32_t R_max, int32_t R, int32_t S, int32_t W, int32_t fw, void* stream) {
  OP_REFUSE(!in || !d || !dW || !ws, "op_conv_wgrad: null pointer (in, d, dW or ws)");
  OP_CONV_SHAPE("op_conv_wgrad");
  OP_REFUSE(R > R_max, "op_conv_wgrad: R = %d frames above R_max = %d the workspace is sized for", R, R_max);
  OP_REFUSE((ldc_in & 3) || (ldc_d & 3) || (ldw & 3), "op_conv_wgrad: leading dimension not a multiple of 4 (ldc_in %d, ldc_d %d, ldw %d)", ldc_in, ldc_d, ldw);
  OP_REFUSE(ldc_in < op_pad4(C) || ldc_d < op_pad4(N) || ldw < N,
            "op_conv_wgrad: leading dimension below its row (ldc_in %d for C = %d, ldc_d %d and ldw %d for N = %d)", ldc_in, C, ldc_d, ldw, N);
  OP_REFUSE(((size_t)in & 15) || ((size_t)d & 15) || ((size_t)ws & 15), "op_conv_wgrad: in, d or ws not 16-byte aligned");
  OP_REFUSE(((size_t)dW & 3) || ((size_t)db & 3), "op_conv_wgrad: dW or db not 4-byte aligned");      // (k_conv_wgrad_red stores scalars)
  g_conv_last_plan.n = 0;
  if (!conv_wgrad_supported(C, N, S, W, fw)) return RSRGAN_OP_NOT_APPLICABLE;    // (the model: the patch matrix and a GEMM)
  const size_t need = conv_wgrad_ws_floats(C, R_max, S, W, fw);
  OP_REFUSE(ws_floats < 0 || (size_t)ws_floats < need, "op_conv_wgrad: workspace of %lld floats below the %zu that R_max = %d frames need", (long long)ws_floats, need, R_max);
  launch_conv_wgrad(in, ldc_in, C, d, ldc_d, N, dW, ldw, ws, R, S, W, fw, (hipStream_t)stream, db);
  OP_LAUNCHED("op_conv_wgrad");
}

int rsrgan_op_conv_last_plan(int32_t out[40]) {
  OP_REFUSE(!out, "op_conv_last_plan: null pointer");
  const ConvPlanRecord& p = g_conv_last_plan;
  for (int i = 0; i < 40; ++i) out[i] = 0;
  out[0] = p.n;
  for (int i = 0; i < p.n && i < 2; ++i) {
    const ConvLaunchRecord& r = p.l[i];
    const int v[19] = {r.family, r.a0, r.a1, r.a2, r.branch, r.TW, r.FB, r.gx, r.gy, r.gz, r.lds, r.DH, r.fpg, r.groups, r.nstrips, r.nkg, r.PS, r.waves, r.gmax};
    for (int j = 0; j < 19; ++j) out[1 + 19 * i + j] = v[j];
  }
  return RSRGAN_OK;
}

// ---- batch_norm(renorm=True) (bn.hip) through the launch functions Model::dnn_forward / rced_forward and their backward passes call
static bool op_bn_vars(float* const* vars, BnVars& v) {
  for (int i = 0; i < 8; ++i) if (!vars[i] || ((size_t)vars[i] & 3)) return false;
  v = BnVars{vars[0], vars[1], vars[2], vars[3], vars[4], vars[5], vars[6], vars[7]};
  return true;
}
#define OP_BN_SHAPE(who, l0, l1, l2) \
  OP_REFUSE(rows < 1 || cols < 1 || calls < 1, who ": rows, cols, calls must be positive (got %d, %d, %d)", rows, cols, calls); \
  OP_REFUSE((long long)rows * calls > (1 << 30), who ": calls x rows = %lld above the entry's 2^30", (long long)rows * calls); \
  OP_REFUSE((l0 & 3) || (l1 & 3) || (l2 & 3) || (ldc & 3), who ": leading dimension not a multiple of 4 (%d, %d, %d, ldc %d)", l0, l1, l2, ldc); \
  OP_REFUSE(l0 < op_pad4(cols) || l1 < op_pad4(cols) || l2 < op_pad4(cols) || ldc < op_pad4(cols), \
            who ": leading dimension below its padded row of %d (%d, %d, %d, ldc %d)", op_pad4(cols), l0, l1, l2, ldc); \
  OP_REFUSE(scratch_floats < 2 * (int64_t)cols, who ": scratch of %lld floats below the 2 x cols = %d of one slice of partial sums", \
            (long long)scratch_floats, 2 * cols)

// the sequence form (bn_seq.hip): one call, a leaky-ReLU of slope alpha and the row rule (Bp, Bt) of a padded batch
#define OP_BN_SEQ_RULE(who) \
  OP_REFUSE(!(alpha >= 0.f && alpha <= 1.f), who ": alpha = %g outside [0, 1]", (double)alpha); \
  OP_REFUSE(Bp < 0 || Bt < 0 || (Bp == 0 && Bt != 0) || (Bp > 0 && (Bt < 1 || Bt > Bp)), \
            who ": row rule (Bp %d, Bt %d): Bp = Bt = 0 counts every row, else 1 <= Bt <= Bp", Bp, Bt); \
  OP_REFUSE(Bp > 0 && rows % Bp, who ": rows = %d is no multiple of Bp = %d", rows, Bp)
#define OP_BN_NO_RULE(who) (void)0
// the refusals of the two forward and of the two backward entries, in their order; `rule`: OP_BN_SEQ_RULE or OP_BN_NO_RULE
#define OP_BN_FWD_ARGS(who, rule) \
  OP_REFUSE(!z || !y || !vars || !stat || !scratch, who ": null pointer (z, y, vars, stat or scratch)"); \
  OP_BN_SHAPE(who, ldz, ldy, ldz); \
  rule(who); \
  OP_REFUSE(((size_t)z & 15) || ((size_t)y & 15) || ((size_t)stat & 15), who ": z, y or stat not 16-byte aligned"); \
  OP_REFUSE((size_t)scratch & 3, who ": scratch not 4-byte aligned"); \
  BnVars v; \
  OP_REFUSE(!op_bn_vars(vars, v), who ": a null or misaligned pointer among the eight variables")
#define OP_BN_BWD_ARGS(who, rule) \
  OP_REFUSE(!dy || !y || !z || !stat || !sums || !scratch, who ": null pointer (dy, y, z, stat, sums or scratch)"); \
  OP_REFUSE((dbeta == nullptr) != (dgamma == nullptr), who ": dbeta and dgamma must both be given or both be null"); \
  OP_BN_SHAPE(who, ldd, ldy, ldz); \
  rule(who); \
  OP_REFUSE(((size_t)dy & 15) || ((size_t)y & 15) || ((size_t)z & 15) || ((size_t)stat & 15) || ((size_t)sums & 15), \
            who ": dy, y, z, stat or sums not 16-byte aligned"); \
  OP_REFUSE(((size_t)scratch & 3) || ((size_t)dbeta & 3) || ((size_t)dgamma & 3), who ": scratch, dbeta or dgamma not 4-byte aligned")

int rsrgan_op_bn_forward(const float* z, int32_t ldz, float* y, int32_t ldy, int32_t rows, int32_t cols, int32_t calls, float* const* vars,
                         float* stat, int32_t ldc, int32_t training, int32_t relu, float* scratch, int64_t scratch_floats, void* stream) {
  OP_BN_FWD_ARGS("op_bn_forward", OP_BN_NO_RULE);
  launch_bn_forward(z, ldz, y, ldy, rows, cols, v, stat, ldc, training != 0, relu != 0, scratch, (size_t)scratch_floats, (hipStream_t)stream, calls);
  OP_LAUNCHED("op_bn_forward");
}

int rsrgan_op_bn_backward(float* dy, int32_t ldd, const float* y, int32_t ldy, const float* z, int32_t ldz, int32_t rows, int32_t cols,
                          int32_t calls, const float* stat, int32_t ldc, float* dbeta, float* dgamma, int32_t accumulate, int32_t relu,
                          float* sums, float* scratch, int64_t scratch_floats, void* stream) {
  OP_BN_BWD_ARGS("op_bn_backward", OP_BN_NO_RULE);
  launch_bn_backward(dy, ldd, y, ldy, z, ldz, rows, cols, stat, ldc, dbeta, dgamma, accumulate != 0, relu != 0, sums, scratch,
                     (size_t)scratch_floats, (hipStream_t)stream, calls);
  OP_LAUNCHED("op_bn_backward");
}

int rsrgan_op_bn_seq_forward(const float* z, int32_t ldz, float* y, int32_t ldy, int32_t rows, int32_t cols, float* const* vars, float* stat,
                             int32_t ldc, int32_t training, int32_t relu, float alpha, int32_t Bp, int32_t Bt, float* scratch,
                             int64_t scratch_floats, void* stream) {
  const int calls = 1;
  OP_BN_FWD_ARGS("op_bn_seq_forward", OP_BN_SEQ_RULE);
  launch_bn_seq_forward(z, ldz, y, ldy, rows, cols, v, stat, ldc, training != 0, relu != 0, alpha, Bp, Bt, scratch, (size_t)scratch_floats,
                        (hipStream_t)stream);
  OP_LAUNCHED("op_bn_seq_forward");
}

int rsrgan_op_bn_seq_backward(float* dy, int32_t ldd, const float* y, int32_t ldy, const float* z, int32_t ldz, int32_t rows, int32_t cols,
                              const float* stat, int32_t ldc, float* dbeta, float* dgamma, int32_t accumulate, int32_t relu, float alpha,
                              int32_t Bp, int32_t Bt, float* sums, float* scratch, int64_t scratch_floats, void* stream) {
  const int calls = 1;
  OP_BN_BWD_ARGS("op_bn_seq_backward", OP_BN_SEQ_RULE);
  launch_bn_seq_backward(dy, ldd, y, ldy, z, ldz, rows, cols, stat, ldc, dbeta, dgamma, accumulate != 0, relu != 0, alpha, Bp, Bt, sums, scratch,
                         (size_t)scratch_floats, (hipStream_t)stream);
  OP_LAUNCHED("op_bn_seq_backward");
}

int rsrgan_op_bn_commit(int32_t n, float* const* vars, const float* const* stat, const int32_t* dims, int32_t single, void* stream) {
  OP_REFUSE(n < 1 || n > 24, "op_bn_commit: n = %d outside the list (1 .. 24)", n);
  OP_REFUSE(!vars || !stat || !dims, "op_bn_commit: null pointer table (vars, stat or dims)");
  BnCommitList cl;
  cl.n = n;
  for (int i = 0; i < n; ++i) {
    const int cols = dims[4 * i], ldc = dims[4 * i + 1], t0 = dims[4 * i + 2], t1 = dims[4 * i + 3];
    BnCommit& e = cl.e[i];
    OP_REFUSE(!op_bn_vars(vars + 8 * i, e.v), "op_bn_commit: a null or misaligned pointer among the variables of entry %d", i);
    OP_REFUSE(!stat[i] || ((size_t)stat[i] & 3), "op_bn_commit: null or misaligned stat of entry %d", i);
    OP_REFUSE(cols < 1, "op_bn_commit: cols = %d in entry %d", cols, i);
    OP_REFUSE((ldc & 3) || ldc < op_pad4(cols), "op_bn_commit: ldc = %d of entry %d is no multiple of 4 or below its padded row of %d", ldc, i, op_pad4(cols));
    OP_REFUSE(t0 < 0 || t1 < 0, "op_bn_commit: negative times (%d, %d) in entry %d", t0, t1, i);
    e.stat = stat[i]; e.cols = cols; e.ldc = ldc; e.times0 = t0; e.times1 = t1;
  }
  OP_REFUSE(single && (n != 1 || cl.e[0].times1 != 0), "op_bn_commit: the single-entry form takes n = 1 and times1 = 0");
  if (single) launch_bn_commit(cl.e[0].cols, cl.e[0].v, cl.e[0].stat, cl.e[0].ldc, cl.e[0].times0, (hipStream_t)stream);
  else launch_bn_commit_many(cl, (hipStream_t)stream);
  OP_LAUNCHED("op_bn_commit");
}

int rsrgan_op_bn_last_plan(int32_t out[16]) {
  OP_REFUSE(!out, "op_bn_last_plan: null pointer");
  const BnPlanRecord& p = g_bn_last_plan;
  const int v[11] = {p.route, p.backward, p.calls, p.launches, p.slices, p.per, p.pgx, p.pgy, p.egrid, p.q, p.R};
  for (int i = 0; i < 16; ++i) out[i] = i < 11 ? v[i] : 0;
  return RSRGAN_OK;
}

// ---- the SEGAN operators (segan.hip, and the window-GEMM primitives of segan.cpp) through the host functions SeganModel calls, on
// caller-owned buffers (tests/test_gpu_segan_ops.py).  One entry per family: op selects the launcher, ptrs is a HOST table of device
// pointers, dims a host table of sizes, fl of float parameters, each in the order include/rsrgan.h lists.  From here on every entry
// is of this table form and defines WHO for capi_common.h's OP_DIM / OP_PTR / OP_LD / ... checks.
#define FP(i) ((float*)ptrs[i])
static const size_t g_segan_ws_floats = (size_t)16 << 20;        // SeganModel::gemm_ws_floats

#define WHO "op_segan_sizes"
int rsrgan_op_segan_sizes(int32_t kind, const int64_t* dims, int64_t out[12]) {
  OP_REFUSE(!dims || !out, WHO ": null pointer");
  OP_REFUSE(kind < 0 || kind > 3, WHO ": kind = %d outside 0 .. 3", kind);
  for (int i = 0; i < 12; ++i) out[i] = 0;
  const int64_t* d = dims;
  if (kind == 0) {                                       // conv2_fwd / conv2_wgrad: Bn, L, C, k
    for (int i = 0; i < 4; ++i) OP_DIM("a size", d[i], 1);
    out[0] = (int64_t)(conv2_pad_floats((int)d[0], (int)d[1], (int)d[2], (int)d[3]) + SEGAN_SCRATCH_SLACK);
  } else if (kind == 1) {                                // tconv2: Bn, Ls, Cs, Lt, Ct, k
    for (int i = 0; i < 6; ++i) OP_DIM("a size", d[i], 1);
    OP_DIM("k", d[5], 2);
    const int Bn = (int)d[0], Ls = (int)d[1], Cs = (int)d[2], Lt = (int)d[3], Ct = (int)d[4], k = (int)d[5];
    OP_REFUSE(Ls != (Lt + 1) / 2, WHO ": Ls = %d is not ceil(Lt / 2) of Lt = %d", Ls, Lt);
    const TGeom g = tgeom(Ls, Lt, k);
    out[0] = (int64_t)(tconv2_pad_floats(Bn, Ls, Cs, Lt, k) + SEGAN_SCRATCH_SLACK);
    out[1] = (int64_t)(tconv2_t_floats(Bn, Ls, Lt, Ct, k) + SEGAN_SCRATCH_SLACK);
    out[2] = (int64_t)g.ne[0] * Cs * pad4(Ct); out[3] = (int64_t)g.ne[1] * Cs * pad4(Ct);
    out[4] = g.pl; out[5] = g.i0[0]; out[6] = g.i0[1]; out[7] = g.Q[0]; out[8] = g.Q[1]; out[9] = g.pf; out[10] = g.pb;
  } else if (kind == 2) {                                // launch_conv1_wgrad: k, C -> shape accepted, LDS bytes (no device)
    OP_DIM("k", d[0], 1); OP_DIM("C", d[1], 1);
    out[0] = conv1_wgrad_shape_ok((int)d[0], (int)d[1]) ? 1 : 0;
    out[1] = (int64_t)conv1_wgrad_lds_bytes((int)d[0], (int)d[1]);
  } else {                                               // launch_colred: C, P -> the least scratch
    OP_DIM("C", d[0], 1); OP_DIM("P", d[1], 1);
    out[0] = (int64_t)colred_min_scratch((int)d[0], (int)d[1]);
  }
  return RSRGAN_OK;
}
#undef WHO

#define WHO "op_segan_conv2"
int rsrgan_op_segan_conv2(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream) {
  (void)fl;
  OP_TABLES(0);
  OP_REFUSE(op < 0 || op > 2, WHO ": op = %d outside 0 (conv2_fwd), 1 (conv2_wgrad), 2 (tconv2)", op);
  const int64_t* d = dims;
  hipStream_t s = (hipStream_t)stream;
  if (op == 0 || op == 1) {
    // 0: ptrs X, W, bias (may be NULL), Z, pad;  dims Bn, L, Cin, k, Cout, ldw, pad_floats
    // 1: ptrs X, dZ, dW, pad;                    dims Bn, L, Cin, k, Cout, ldz, ldw, pad_floats
    OP_DIM("Bn", d[0], 1); OP_DIM("L", d[1], 1); OP_DIM("Cin", d[2], 1); OP_DIM("k", d[3], 1); OP_DIM("Cout", d[4], 1);
    const int Bn = (int)d[0], L = (int)d[1], Cin = (int)d[2], k = (int)d[3], Cout = (int)d[4];
    OP_MUL4("Cin", Cin); OP_MUL4("Cout", Cout);
    OP_REFUSE((int64_t)Bn * (L + 2 * k) * Cin > (1 << 28) || (int64_t)k * Cin > (1 << 20), WHO ": Bn x (L + 2 k) x Cin above the entry's 2^28");
    const int64_t pad_floats = op == 0 ? d[6] : d[7];
    const size_t need = conv2_pad_floats(Bn, L, Cin, k) + SEGAN_SCRATCH_SLACK;
    OP_REFUSE(pad_floats < 0 || (size_t)pad_floats < need, WHO ": pad of %lld floats below the %zu the model gives this layer", (long long)pad_floats, need);
    if (op == 0) {
      OP_PTR("X", ptrs[0], 16); OP_PTR("W", ptrs[1], 16); OP_OPT("bias", ptrs[2], 16); OP_PTR("Z", ptrs[3], 16); OP_PTR("pad", ptrs[4], 16);
      OP_MUL4("ldw", d[5]); OP_LD("ldw", d[5], Cout);
    } else {
      OP_PTR("X", ptrs[0], 16); OP_PTR("dZ", ptrs[1], 16); OP_PTR("dW", ptrs[2], 16); OP_PTR("pad", ptrs[3], 16);
      OP_MUL4("ldz", d[5]); OP_LD("ldz", d[5], Cout); OP_MUL4("ldw", d[6]); OP_LD("ldw", d[6], Cout);
    }
    float* ws = op_ws();
    if (!ws) { set_error(WHO ": hipMalloc failed"); return RSRGAN_ERR_HIP; }
    SeganModel m;                                          // bare: the primitives use pad, t0, t1 and the GEMM workspace only
    m.gemm_ws = ws; m.gemm_ws_floats = g_segan_ws_floats;
    m.pad = FP(op == 0 ? 4 : 3); m.pad_floats = (size_t)pad_floats;
    if (op == 0) m.conv2_fwd(FP(0), Bn, L, Cin, k, FP(1), (int)d[5], FP(2), Cout, FP(3), s);
    else m.conv2_wgrad(FP(0), Bn, L, Cin, k, FP(1), (int)d[5], Cout, FP(2), (int)d[6], s);
    OP_LAUNCHED(WHO);
  }
  // 2: ptrs S, W, bias (may be NULL), T, pad, t0, t1, Wt0, Wt1;  dims Bn, Ls, Cs, Lt, k, Ct, ldw, pad_floats, t_floats, wt0_floats, wt1_floats
  //    W [k * Ct][ldw] with Cs columns: the filter of the downconv Ct -> Cs whose data gradient this is (= a deconv Cs -> Ct)
  OP_DIM("Bn", d[0], 1); OP_DIM("Ls", d[1], 1); OP_DIM("Cs", d[2], 1); OP_DIM("Lt", d[3], 1); OP_DIM("k", d[4], 2); OP_DIM("Ct", d[5], 1);
  const int Bn = (int)d[0], Ls = (int)d[1], Cs = (int)d[2], Lt = (int)d[3], k = (int)d[4], Ct = (int)d[5];
  OP_MUL4("Cs", Cs); OP_MUL4("Ct", Ct);
  OP_REFUSE(Ls != (Lt + 1) / 2, WHO ": Ls = %d is not ceil(Lt / 2) of Lt = %d", Ls, Lt);
  OP_REFUSE((int64_t)Bn * (Ls + 2 * k) * std::max(Cs, Ct) > (1 << 28) || (int64_t)k * Cs * Ct > (1 << 28), WHO ": Bn x (Ls + 2 k) x C above the entry's 2^28");
  OP_MUL4("ldw", d[6]); OP_LD("ldw", d[6], Cs);
  const char* names[9] = {"S", "W", "bias", "T", "pad", "t0", "t1", "Wt0", "Wt1"};
  for (int i = 0; i < 9; ++i) { if (i == 2) OP_OPT(names[i], ptrs[i], 16); else OP_PTR(names[i], ptrs[i], 16); }
  const TGeom g = tgeom(Ls, Lt, k);
  const size_t need_pad = tconv2_pad_floats(Bn, Ls, Cs, Lt, k) + SEGAN_SCRATCH_SLACK, need_t = tconv2_t_floats(Bn, Ls, Lt, Ct, k) + SEGAN_SCRATCH_SLACK;
  OP_REFUSE(d[7] < 0 || (size_t)d[7] < need_pad, WHO ": pad of %lld floats below the %zu the model gives this layer", (long long)d[7], need_pad);
  OP_REFUSE(d[8] < 0 || (size_t)d[8] < need_t, WHO ": t0 / t1 of %lld floats below the %zu the model gives this layer", (long long)d[8], need_t);
  for (int e = 0; e < 2; ++e)
    OP_REFUSE(d[9 + e] < (int64_t)g.ne[e] * Cs * pad4(Ct), WHO ": Wt%d of %lld floats below ne x Cs x Ct = %lld", e, (long long)d[9 + e], (long long)g.ne[e] * Cs * pad4(Ct));
  float* ws = op_ws();
  if (!ws) { set_error(WHO ": hipMalloc failed"); return RSRGAN_ERR_HIP; }
  SeganModel m;
  m.gemm_ws = ws; m.gemm_ws_floats = g_segan_ws_floats;
  m.pad = FP(4); m.pad_floats = (size_t)d[7]; m.t0 = FP(5); m.t1 = FP(6); m.t_floats = (size_t)d[8];
  float* Wt[2] = {FP(7), FP(8)};
  PrepTconvBatch pb(s);                                   // as SeganModel::refresh_weights prepares a downconv's data gradient
  for (int e = 0; e < 2; ++e) pb.add(FP(1), (int)d[6], Ct, Cs, e, g.ne[e], Wt[e], pad4(Ct));
  pb.flush();
  m.tconv2(FP(0), Bn, Ls, Cs, Lt, k, Wt, g.ne, Ct, FP(2), FP(3), s);
  OP_LAUNCHED(WHO);
}
#undef WHO

#define WHO "op_segan_conv1"
int rsrgan_op_segan_conv1(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream) {
  (void)fl;
  OP_TABLES(0);
  OP_REFUSE(op < 0 || op > 2, WHO ": op = %d outside 0 (conv1_fwd), 1 (conv1_wgrad), 2 (tconv1)", op);
  const int64_t* d = dims;
  hipStream_t s = (hipStream_t)stream;
  if (op == 0) {                                         // ptrs x, W, bias (may be NULL), z;  dims B, L, k, C, ldx, ldw, ldz
    OP_DIM("B", d[0], 1); OP_DIM("L", d[1], 1); OP_DIM("k", d[2], 1); OP_DIM("C", d[3], 1);
    OP_REFUSE(d[3] & 15, WHO ": C = %lld is not a multiple of 16 (k_conv1_fwd writes 16 channels at a time)", (long long)d[3]);
    OP_REFUSE((d[2] + 1) * d[3] * 4 > (64 << 10), WHO ": (k + 1) x C floats of filter exceed 64 KB of LDS");
    OP_PTR("x", ptrs[0], 4); OP_PTR("W", ptrs[1], 4); OP_OPT("bias", ptrs[2], 4); OP_PTR("z", ptrs[3], 16);
    OP_LD("ldx", d[4], d[1]); OP_LD("ldw", d[5], d[3]); OP_LD("ldz", d[6], d[3]); OP_MUL4("ldz", d[6]);
    launch_conv1_fwd(FP(0), (int)d[4], (int)d[0], (int)d[1], (int)d[2], FP(1), (int)d[5], FP(2), (int)d[3], FP(3), (int)d[6], s);
    OP_LAUNCHED(WHO);
  }
  if (op == 1) {                                         // ptrs x, dz, dW, scratch;  dims B, L, k, C, ldx, ldz, ldw, scratch_floats
    OP_DIM("B", d[0], 1); OP_DIM("L", d[1], 1); OP_DIM("k", d[2], 1); OP_DIM("C", d[3], 1);
    OP_REFUSE(d[0] > 65535, WHO ": B = %lld above the grid's 65535", (long long)d[0]);
    OP_REFUSE(!conv1_wgrad_shape_ok((int)d[2], (int)d[3]), WHO ": k x C = %lld above 1024 or C = %lld no multiple of 4: launch_conv1_wgrad has no kernel for it",
              (long long)(d[2] * d[3]), (long long)d[3]);
    OP_PTR("x", ptrs[0], 4); OP_PTR("dz", ptrs[1], 16); OP_PTR("dW", ptrs[2], 4); OP_PTR("scratch", ptrs[3], 4);
    OP_LD("ldx", d[4], d[1]); OP_LD("ldz", d[5], d[3]); OP_MUL4("ldz", d[5]); OP_LD("ldw", d[6], d[3]);
    OP_REFUSE(d[7] < d[0] * d[2] * d[3], WHO ": scratch of %lld floats below B x k x C = %lld (one partial per batch row)", (long long)d[7], (long long)(d[0] * d[2] * d[3]));
    OP_REFUSE(!conv1_wgrad_supported((int)d[2], (int)d[3]), WHO ": %zu bytes of LDS above the device's %zu", conv1_wgrad_lds_bytes((int)d[2], (int)d[3]), device_lds_limit());
    launch_conv1_wgrad(FP(0), (int)d[4], (int)d[0], (int)d[1], (int)d[2], FP(1), (int)d[5], (int)d[3], FP(2), (int)d[6], FP(3), (size_t)d[7], s);
    OP_LAUNCHED(WHO);
  }
  // 2: ptrs S, W, bias (may be NULL), t;  dims B, Ls, C, Lt, k, lds, ldw, ldt
  OP_DIM("B", d[0], 1); OP_DIM("Ls", d[1], 1); OP_DIM("C", d[2], 1); OP_DIM("Lt", d[3], 1); OP_DIM("k", d[4], 1);
  OP_MUL4("C", d[2]);
  OP_REFUSE(d[1] != (d[3] + 1) / 2, WHO ": Ls = %lld is not ceil(Lt / 2) of Lt = %lld", (long long)d[1], (long long)d[3]);
  OP_REFUSE(d[4] * d[2] * 4 > (64 << 10), WHO ": k x C floats of filter exceed 64 KB of LDS");
  OP_PTR("S", ptrs[0], 16); OP_PTR("W", ptrs[1], 4); OP_OPT("bias", ptrs[2], 4); OP_PTR("t", ptrs[3], 4);
  OP_LD("lds", d[5], d[2]); OP_MUL4("lds", d[5]); OP_LD("ldw", d[6], d[2]); OP_LD("ldt", d[7], d[3]);
  launch_tconv1(FP(0), (int)d[5], (int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4], FP(1), (int)d[6], FP(2), FP(3), (int)d[7], s);
  OP_LAUNCHED(WHO);
}
#undef WHO

#define WHO "op_segan_colred"
int rsrgan_op_segan_colred(int32_t mode, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream) {
  // ptrs a, b, coef, out, scratch;  dims lda, coff, ldb, C, rows_per, P, ldcoef, ldo, accumulate, scratch_floats;  fl leak
  OP_TABLES(1);
  OP_REFUSE(mode < 0 || mode > 3, WHO ": mode = %d outside 0 .. 3", mode);
  const int64_t* d = dims;
  const bool two = mode == 1 || mode == 3;
  OP_DIM("C", d[3], 1); OP_DIM("rows_per", d[4], 1); OP_DIM("P", d[5], 1); OP_DIM("coff", d[1], 0); OP_FLAG("accumulate", d[8]);
  OP_REFUSE(d[4] * d[5] > ((int64_t)1 << 30) || d[5] > 64, WHO ": P x rows_per above the entry's 2^30, or P above 64");
  // 16 bytes wherever the sizes let launch_colred take the 16-byte form (it looks at the sizes, not at the pointers)
  const int al = (d[3] % 4 == 0 && d[0] % 4 == 0 && d[1] % 4 == 0) ? 16 : 4;
  OP_PTR("a", ptrs[0], al); OP_PTR("out", ptrs[3], 4); OP_PTR("scratch", ptrs[4], 16);
  OP_LD("lda", d[0], d[1] + d[3]); OP_LD("ldo", d[7], d[3]);
  if (two) { OP_PTR("b", ptrs[1], d[2] % 4 == 0 ? al : 4); OP_LD("ldb", d[2], d[3]); }
  if (mode == 3) { OP_PTR("coef", ptrs[2], d[6] % 4 == 0 ? al : 4); OP_LD("ldcoef", d[6], d[3]); }
  const size_t need = colred_min_scratch((int)d[3], (int)d[5]);
  OP_REFUSE(d[9] < 0 || (size_t)d[9] < need, WHO ": scratch of %lld floats below the P x 2 x C = %zu of one chunk per pass", (long long)d[9], need);
  launch_colred(mode, FP(0), (int)d[0], (int)d[1], FP(1), (int)d[2], (int)d[3], (size_t)d[4], (int)d[5], FP(2), (int)d[6], fl[0], FP(3), (int)d[7], d[8] != 0,
                FP(4), (size_t)d[9], (hipStream_t)stream);
  OP_LAUNCHED(WHO);
}
#undef WHO

#define WHO "op_segan_last_plan"
int rsrgan_op_segan_last_plan(int32_t out[8]) {
  OP_REFUSE(!out, WHO ": null pointer");
  const ColredPlanRecord& p = g_colred_last_plan;
  const int v[5] = {p.vec, p.mode, p.chunk, p.chunks_per, p.grid};
  for (int i = 0; i < 8; ++i) out[i] = i < 5 ? v[i] : 0;
  return RSRGAN_OK;
}
#undef WHO

#define WHO "op_segan_vbn"
int rsrgan_op_segan_vbn(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream) {
  OP_TABLES(0);
  OP_REFUSE(op < 0 || op > 3, WHO ": op = %d outside 0 (vbn_coef), 1 (vbn_apply), 2 (vbn_bwd_coef), 3 (vbn_bwd_apply)", op);
  const int64_t* d = dims;
  OP_REFUSE(op != 2 && !fl, WHO ": null table (fl: eps or leak)");
  hipStream_t s = (hipStream_t)stream;
  // every op: dims C, rows_per, P, ldc, then its own
  OP_DIM("C", d[0], 1); OP_DIM("rows_per", d[1], 1); OP_DIM("P", d[2], 1); OP_LD("ldc", d[3], d[0]);
  OP_REFUSE(d[1] * d[2] * d[0] > ((int64_t)1 << 30) || d[2] > 64, WHO ": P x rows_per x C above the entry's 2^30, or P above 64");
  const int C = (int)d[0], P = (int)d[2], ldc = (int)d[3];
  const size_t rows_per = (size_t)d[1];
  if (op == 0) {                                         // ptrs sums, gamma, beta, ref_coef (may be NULL), coef;  dims .., lds, B;  fl eps
    OP_PTR("sums", ptrs[0], 4); OP_PTR("gamma", ptrs[1], 4); OP_PTR("beta", ptrs[2], 4); OP_OPT("ref_coef", ptrs[3], 4); OP_PTR("coef", ptrs[4], 4);
    OP_LD("lds", d[4], C); OP_DIM("B", d[5], 1);
    launch_vbn_coef(FP(0), (int)d[4], P, C, rows_per, (int)d[5], fl[0], FP(1), FP(2), FP(3), FP(4), ldc, s);
  } else if (op == 1) {                                  // ptrs h, coef, y;  fl leak
    OP_PTR("h", ptrs[0], 4); OP_PTR("coef", ptrs[1], 4); OP_PTR("y", ptrs[2], 4);
    launch_vbn_apply(FP(0), C, rows_per, P, FP(1), ldc, fl[0], FP(2), s);
  } else if (op == 2) {                                  // ptrs sums, gamma, coef, dgamma, dbeta (both may be NULL);  dims .., lds, B, first_live, accumulate
    OP_PTR("sums", ptrs[0], 4); OP_PTR("gamma", ptrs[1], 4); OP_PTR("coef", ptrs[2], 4); OP_OPT("dgamma", ptrs[3], 4); OP_OPT("dbeta", ptrs[4], 4);
    OP_REFUSE((ptrs[3] == nullptr) != (ptrs[4] == nullptr), WHO ": dgamma and dbeta must both be given or both be null");
    OP_LD("lds", d[4], C); OP_DIM("B", d[5], 1);
    OP_REFUSE(d[6] < 0 || d[6] > 1, WHO ": first_live = %lld outside 0 (all live) .. 1 (pass 0 is the reference)", (long long)d[6]);
    OP_FLAG("accumulate", d[7]);
    launch_vbn_bwd_coef(FP(0), (int)d[4], P, (int)d[6], C, rows_per, (int)d[5], FP(1), FP(2), ldc, FP(3), FP(4), d[7] != 0, s);
  } else {                                               // ptrs h, dy, coef, dh;  fl leak
    OP_PTR("h", ptrs[0], 4); OP_PTR("dy", ptrs[1], 4); OP_PTR("coef", ptrs[2], 4); OP_PTR("dh", ptrs[3], 4);
    launch_vbn_bwd_apply(FP(0), FP(1), C, rows_per, P, FP(2), ldc, fl[0], FP(3), s);
  }
  OP_LAUNCHED(WHO);
}
#undef WHO

#define WHO "op_segan_elem"
int rsrgan_op_segan_elem(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream) {
  OP_TABLES(0);
  OP_REFUSE(op < 0 || op > 11, WHO ": op = %d outside 0 .. 11", op);
  const int64_t* d = dims;
  OP_REFUSE((op == 4 || op == 5 || op == 11) && !fl, WHO ": null table (fl: leak, or decay and eps)");
  hipStream_t s = (hipStream_t)stream;
  switch (op) {
    case 0: {                                            // pad_rows: ptrs src, dst;  dims B, L, C, pf, pb
      OP_DIM("B", d[0], 1); OP_DIM("L", d[1], 1); OP_DIM("C", d[2], 1); OP_DIM("pf", d[3], 0); OP_DIM("pb", d[4], 0); OP_MUL4("C", d[2]);
      OP_REFUSE(d[0] * (d[1] + d[3] + d[4]) * d[2] > ((int64_t)1 << 30), WHO ": B x (pf + L + pb) x C above the entry's 2^30");
      OP_PTR("src", ptrs[0], 16); OP_PTR("dst", ptrs[1], 16);
      launch_pad_rows(FP(0), FP(1), (int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4], s);
      break;
    }
    case 1: case 2: {                                    // prep_tconv (one job) / prep_tconv_many: ptrs (W, dst) per job;  dims n, then ldw, nb, na, e, ne, ldd per job
      OP_DIM("n", d[0], 1);
      OP_REFUSE(d[0] > 132 || (op == 1 && d[0] != 1), WHO ": n = %lld jobs outside 1 .. 132 (launch_prep_tconv: 1)", (long long)d[0]);
      const int n = (int)d[0];
      for (int j = 0; j < n; ++j) {
        const int64_t* q = d + 1 + 6 * j;
        OP_PTR("W", ptrs[2 * j], 4); OP_PTR("dst", ptrs[2 * j + 1], 4);
        OP_DIM("nb", q[1], 1); OP_DIM("na", q[2], 1); OP_DIM("ne", q[4], 1); OP_LD("ldw", q[0], q[2]); OP_LD("ldd", q[5], q[1]);
        OP_REFUSE(q[3] < 0 || q[3] > 1, WHO ": e = %lld of job %d outside 0 .. 1", (long long)q[3], j);
        OP_REFUSE(q[4] * q[1] * q[2] > (1 << 28), WHO ": ne x nb x na of job %d above the entry's 2^28", j);
      }
      if (op == 1) launch_prep_tconv(FP(0), (int)d[1], (int)d[2], (int)d[3], (int)d[4], (int)d[5], FP(1), (int)d[6], s);
      else {
        PrepTconvBatch pb(s);
        for (int j = 0; j < n; ++j) { const int64_t* q = d + 1 + 6 * j; pb.add(FP(2 * j), (int)q[0], (int)q[1], (int)q[2], (int)q[3], (int)q[4], FP(2 * j + 1), (int)q[5]); }
        pb.flush();
      }
      break;
    }
    case 3: {                                            // interleave: ptrs T0, T1, bias (may be NULL), T;  dims Q0, Q1, i00, i01, pl, B, Lt, C
      OP_DIM("Q0", d[0], 1); OP_DIM("Q1", d[1], 1); OP_DIM("pl", d[4], 0); OP_DIM("B", d[5], 1); OP_DIM("Lt", d[6], 1); OP_DIM("C", d[7], 1); OP_MUL4("C", d[7]);
      for (int e = 0; e < 2; ++e) {
        const int64_t i0 = (((e - d[4]) % 2) + 2) % 2, cnt = d[6] > i0 ? (d[6] - i0 + 1) / 2 : 0;
        OP_REFUSE(d[2 + e] != i0, WHO ": i0%d = %lld is not the first position of parity class %d under pl = %lld", e, (long long)d[2 + e], e, (long long)d[4]);
        OP_REFUSE(d[e] < cnt, WHO ": Q%d = %lld below the %lld positions of its class", e, (long long)d[e], (long long)cnt);
      }
      OP_REFUSE(d[5] * d[6] * d[7] > ((int64_t)1 << 30), WHO ": B x Lt x C above the entry's 2^30");
      OP_PTR("T0", ptrs[0], 16); OP_PTR("T1", ptrs[1], 16); OP_OPT("bias", ptrs[2], 16); OP_PTR("T", ptrs[3], 16);
      launch_interleave(FP(0), FP(1), (int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4], FP(2), FP(3), (int)d[5], (int)d[6], (int)d[7], s);
      break;
    }
    case 4: {                                            // act_fwd: ptrs z, alpha (NULL: leaky), out;  dims C, ldo, coff, rows;  fl leak
      OP_DIM("C", d[0], 1); OP_DIM("coff", d[2], 0); OP_DIM("rows", d[3], 1); OP_LD("ldo", d[1], d[2] + d[0]);
      OP_REFUSE(d[3] * d[1] > ((int64_t)1 << 30), WHO ": rows x ldo above the entry's 2^30");
      OP_PTR("z", ptrs[0], 4); OP_OPT("alpha", ptrs[1], 4); OP_PTR("out", ptrs[2], 4);
      launch_act_fwd(FP(0), (int)d[0], FP(1), fl[0], FP(2), (int)d[1], (int)d[2], (size_t)d[3], s);
      break;
    }
    case 5: {                                            // act_bwd: ptrs dy, z, alpha, extra (may be NULL), dz;  dims ldy, coff, C, rows;  fl leak
      OP_DIM("C", d[2], 1); OP_DIM("coff", d[1], 0); OP_DIM("rows", d[3], 1); OP_LD("ldy", d[0], d[1] + d[2]);
      OP_REFUSE(d[3] * d[0] > ((int64_t)1 << 30), WHO ": rows x ldy above the entry's 2^30");
      OP_PTR("dy", ptrs[0], 4); OP_PTR("z", ptrs[1], 4); OP_OPT("alpha", ptrs[2], 4); OP_OPT("extra", ptrs[3], 4); OP_PTR("dz", ptrs[4], 4);
      launch_act_bwd(FP(0), (int)d[0], (int)d[1], FP(1), (int)d[2], FP(2), fl[0], FP(3), FP(4), (size_t)d[3], s);
      break;
    }
    case 6: {                                            // copy_cols: ptrs src, dst;  dims lds, soff, ldd, doff, C, rows, accumulate
      OP_DIM("C", d[4], 1); OP_DIM("rows", d[5], 1); OP_DIM("soff", d[1], 0); OP_DIM("doff", d[3], 0); OP_FLAG("accumulate", d[6]);
      OP_LD("lds", d[0], d[1] + d[4]); OP_LD("ldd", d[2], d[3] + d[4]);
      OP_REFUSE(d[5] * std::max(d[0], d[2]) > ((int64_t)1 << 30), WHO ": rows x ld above the entry's 2^30");
      OP_PTR("src", ptrs[0], 4); OP_PTR("dst", ptrs[1], 4);
      launch_copy_cols(FP(0), (int)d[0], (int)d[1], FP(1), (int)d[2], (int)d[3], (int)d[4], (size_t)d[5], d[6] != 0, s);
      break;
    }
    case 7: {                                            // build_joint1: ptrs x, tail, noise (may be NULL), joint;  dims Lx, U, B
      OP_DIM("Lx", d[0], 1); OP_DIM("U", d[1], 1); OP_DIM("B", d[2], 1);
      OP_REFUSE(d[2] * (d[0] + d[1]) > ((int64_t)1 << 30), WHO ": B x (Lx + U) above the entry's 2^30");
      OP_PTR("x", ptrs[0], 4); OP_PTR("tail", ptrs[1], 4); OP_OPT("noise", ptrs[2], 4); OP_PTR("joint", ptrs[3], 4);
      launch_build_joint1(FP(0), (int)d[0], FP(1), (int)d[1], FP(2), FP(3), (int)d[2], s);
      break;
    }
    case 8: {                                            // sum_all: ptrs src, out, scratch (256 floats);  dims rows, cols, ld
      OP_DIM("rows", d[0], 1); OP_DIM("cols", d[1], 1); OP_LD("ld", d[2], d[1]);
      OP_REFUSE(d[0] * d[2] > ((int64_t)1 << 30), WHO ": rows x ld above the entry's 2^30");
      OP_PTR("src", ptrs[0], 4); OP_PTR("out", ptrs[1], 4); OP_PTR("scratch", ptrs[2], 4);
      launch_sum_all(FP(0), (int)d[0], (int)d[1], (int)d[2], FP(1), FP(2), s);
      break;
    }
    case 9: {                                            // segan_lsgan: ptrs logits, dlogits (may be NULL), loss3;  dims B, mode, fake_pass, P
      OP_DIM("B", d[0], 1); OP_DIM("P", d[3], 1);
      OP_REFUSE(d[1] < 0 || d[1] > 1, WHO ": mode = %lld outside 0 (D-run) .. 1 (G-run)", (long long)d[1]);
      OP_REFUSE(d[2] < 0 || d[2] >= d[3], WHO ": fake_pass = %lld outside [0, P = %lld)", (long long)d[2], (long long)d[3]);
      OP_REFUSE(d[0] * d[3] > (1 << 24), WHO ": P x B above the entry's 2^24");
      OP_PTR("logits", ptrs[0], 4); OP_OPT("dlogits", ptrs[1], 4); OP_PTR("loss3", ptrs[2], 4);
      launch_segan_lsgan(FP(0), (int)d[0], (int)d[1], (int)d[2], (int)d[3], FP(1), FP(2), s);
      break;
    }
    case 10: {                                           // segan_l1: ptrs G, labels, lambda, dG (may be NULL), loss3;  dims n, accumulate
      OP_DIM("n", d[0], 1); OP_FLAG("accumulate", d[1]);
      OP_PTR("G", ptrs[0], 4); OP_PTR("labels", ptrs[1], 4); OP_PTR("lambda", ptrs[2], 4); OP_OPT("dG", ptrs[3], 4); OP_PTR("loss3", ptrs[4], 4);
      launch_segan_l1(FP(0), FP(1), (int)d[0], FP(2), FP(3), d[1] != 0, FP(4), s);
      break;
    }
    default: {                                           // rmsprop: ptrs w, g, ms, lr;  dims n;  fl decay, eps
      OP_DIM("n", d[0], 1);
      OP_PTR("w", ptrs[0], 4); OP_PTR("g", ptrs[1], 4); OP_PTR("ms", ptrs[2], 4); OP_PTR("lr", ptrs[3], 4);
      launch_rmsprop(FP(0), FP(1), FP(2), FP(3), fl[0], fl[1], (size_t)d[0], s);
      break;
    }
  }
  OP_LAUNCHED(WHO);
}
#undef WHO

#define WHO "op_segan_dhead"
int rsrgan_op_segan_dhead(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream) {
  (void)fl;
  OP_TABLES(0);
  OP_REFUSE(op < 0 || op > 1, WHO ": op = %d outside 0 (dhead_fwd), 1 (dhead_bwd)", op);
  const int64_t* d = dims;                               // dims R, Ld, C, k, ldfc
  OP_DIM("R", d[0], 1); OP_DIM("Ld", d[1], 1); OP_DIM("C", d[2], 1); OP_DIM("k", d[3], 1); OP_DIM("ldfc", d[4], 1);
  OP_REFUSE(d[0] * d[1] * d[2] > ((int64_t)1 << 28) || d[3] * d[2] > (1 << 24), WHO ": R x Ld x C above the entry's 2^28");
  if (op == 0) {                                         // ptrs h, W, wfc, bfc, conv_out, logits
    const char* names[6] = {"h", "W", "wfc", "bfc", "conv_out", "logits"};
    for (int i = 0; i < 6; ++i) OP_PTR(names[i], ptrs[i], 4);
    launch_dhead_fwd(FP(0), (int)d[0], (int)d[1], (int)d[2], (int)d[3], FP(1), FP(2), (int)d[4], FP(3), FP(4), FP(5), (hipStream_t)stream);
  } else {                                               // ptrs dlogit, h, conv_out, W, wfc, dW, dwfc, dbfc (all three or none), dh
    const char* names[9] = {"dlogit", "h", "conv_out", "W", "wfc", "dW", "dwfc", "dbfc", "dh"};
    for (int i = 0; i < 9; ++i) { if (i >= 5 && i <= 7) OP_OPT(names[i], ptrs[i], 4); else OP_PTR(names[i], ptrs[i], 4); }
    OP_REFUSE((!ptrs[5]) != (!ptrs[6]) || (!ptrs[5]) != (!ptrs[7]), WHO ": dW, dwfc and dbfc must all be given or all be null");
    launch_dhead_bwd(FP(0), (int)d[0], (int)d[1], (int)d[2], (int)d[3], FP(1), FP(2), FP(3), FP(4), (int)d[4], FP(5), FP(6), FP(7), FP(8), (hipStream_t)stream);
  }
  OP_LAUNCHED(WHO);
}
#undef WHO

// ---- unit-test entries of the step's small kernels (kernels.hip: losses, the discriminator's fused head, L2, clip_by_norm, the updates,
// dropout, lrelu') on caller-owned buffers (tests/test_gpu_update_ops.py, test_gpu_loss_ops.py, test_update_op_args.py).  Same form as
// the SEGAN entries: op selects the launcher the model calls, ptrs / dims / fl are HOST tables in the order include/rsrgan.h lists.
#define OP_BP(rows_name, rows, Bp, Bt) do { \
    OP_REFUSE((Bp) < 0 || (Bp) > (1 << 20), WHO ": Bp = %lld outside 0 .. 2^20", (long long)(Bp)); \
    if ((Bp) > 0) { \
      OP_REFUSE((Bt) < 1 || (Bt) > (Bp), WHO ": Bt = %lld outside 1 .. Bp = %lld", (long long)(Bt), (long long)(Bp)); \
      OP_REFUSE((rows) % (Bp), WHO ": %s = %lld is not divisible by Bp = %lld", rows_name, (long long)(rows), (long long)(Bp)); \
    } } while (0)
static const int64_t g_up_max_tensors = 4096;

// tensors [n][3] = (float offset, floats, l2 flag): every error named; 0 = fine.  buf_floats < 0: no buffer to fit
static int up_tensors_ok(const char* who, const int64_t* tensors, int64_t n, int64_t buf_floats) {
  OP_REFUSE(!tensors, "%s: null pointer (tensors)", who);
  OP_REFUSE(n < 1 || n > g_up_max_tensors, "%s: n_tensors = %lld outside 1 .. %lld", who, (long long)n, (long long)g_up_max_tensors);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t off = tensors[3 * i], fl = tensors[3 * i + 1], l2 = tensors[3 * i + 2];
    OP_REFUSE(off < 0 || (off & 3), "%s: offset %lld of tensor %lld is negative or not a multiple of 4", who, (long long)off, (long long)i);
    OP_REFUSE(fl < 1 || (fl & 3), "%s: length %lld of tensor %lld is below 1 or not a multiple of 4", who, (long long)fl, (long long)i);
    OP_REFUSE(off > ((int64_t)1 << 30) || fl > ((int64_t)1 << 30), "%s: tensor %lld reaches beyond 2^30 floats", who, (long long)i);
    OP_REFUSE(l2 < 0 || l2 > 1, "%s: l2 flag %lld of tensor %lld is neither 0 nor 1", who, (long long)l2, (long long)i);
    OP_REFUSE(buf_floats >= 0 && off + fl > buf_floats, "%s: tensor %lld ends at %lld, beyond the buffer's %lld floats", who, (long long)i,
              (long long)(off + fl), (long long)buf_floats);
  }
  return RSRGAN_OK;
}
static void up_table(const int64_t* tensors, int n, ChunkTableHost& h) {
  std::vector<int64_t> off(n), fl(n);
  std::vector<int> l2(n);
  for (int i = 0; i < n; ++i) { off[i] = tensors[3 * i]; fl[i] = tensors[3 * i + 1]; l2[i] = (int)tensors[3 * i + 2]; }
  chunk_table_host(off.data(), fl.data(), l2.data(), n, h);
}

#define WHO "op_chunks"
int rsrgan_op_chunks(const int64_t* tensors, int32_t n_tensors, int32_t* out, int64_t out_ints, int32_t* n_chunks) {
  return guard(WHO, [&]() -> int {
    OP_REFUSE(!n_chunks, WHO ": null pointer (n_chunks)");
    if (int rc = up_tensors_ok(WHO, tensors, n_tensors, -1)) return rc;
    ChunkTableHost h;
    up_table(tensors, n_tensors, h);
    *n_chunks = (int32_t)h.tensor.size();
    if (!out) return RSRGAN_OK;
    const int64_t need = 3 * (int64_t)h.tensor.size() + 3 * (int64_t)n_tensors;
    OP_REFUSE(out_ints < need, WHO ": out of %lld ints below the table's %lld", (long long)out_ints, (long long)need);
    for (const std::vector<int>* v : {&h.tensor, &h.off, &h.len, &h.t_first, &h.t_count, &h.t_l2})
      for (int x : *v) *out++ = x;
    return RSRGAN_OK;
  });
}
#undef WHO

#define WHO "op_update"
int rsrgan_op_update(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream) {
  (void)fl;
  return guard(WHO, [&]() -> int {
    OP_TABLES(0);
    OP_REFUSE(op < 0 || op > 4, WHO ": op = %d outside 0 (sumsq), 1 (dw_reduce), 2 (l2), 3 (apply_sgd), 4 (apply_adam)", op);
    const int64_t* d = dims;
    const int64_t nt = d[0], buf_floats = d[1], partial_floats = d[2];
    OP_DIM("buf_floats", buf_floats, 4);
    if (int rc = up_tensors_ok(WHO, d + 6, nt, buf_floats)) return rc;
    ChunkTableHost h;
    up_table(d + 6, (int)nt, h);
    const int nc = (int)h.tensor.size();
    OP_REFUSE(partial_floats < nc, WHO ": partial of %lld floats below the table's %d chunks", (long long)partial_floats, nc);
    static const char* const names[5][7] = {{"g", "partial"}, {"ws", "g", "partial"}, {"w", "g", "l2_scale", "partial"},
                                            {"w", "g", "ema", "partial", "dyn"}, {"w", "g", "m", "v", "ema", "partial", "dyn"}};
    // bytes of alignment, beside the names: 16 for the flat buffers the kernels move as float4, 4 for scalars and partial; negative: may be NULL
    static const int align[5][7] = {{16, 4}, {16, 16, 4}, {16, 16, 4, 4}, {16, 16, -16, 4, 4}, {16, 16, 16, 16, -16, 4, 4}};
    static const int np[5] = {2, 3, 4, 5, 7};
    for (int i = 0; i < np[op]; ++i) {
      if (align[op][i] < 0) OP_OPT(names[op][i], ptrs[i], -align[op][i]); else OP_PTR(names[op][i], ptrs[i], align[op][i]);
    }
    std::vector<long long> src;
    if (op == 1) {                                       // dims[3..5] stride, ntiles, ws_floats; src [n_tensors] behind the tensors
      const int64_t stride = d[3], ntiles = d[4], ws_floats = d[5];
      OP_DIM("stride", stride, 4); OP_MUL4("stride", stride); OP_DIM("ws_floats", ws_floats, 4);
      OP_REFUSE(ntiles < 1 || ntiles > 64, WHO ": ntiles = %lld outside 1 .. 64", (long long)ntiles);
      for (int64_t i = 0; i < nt; ++i) {
        const int64_t so = d[6 + 3 * nt + i], n = d[6 + 3 * i + 1];
        OP_REFUSE(so < -1 || (so >= 0 && (so & 3)), WHO ": src %lld of tensor %lld is neither -1 nor a non-negative multiple of 4", (long long)so, (long long)i);
        OP_REFUSE(so >= 0 && so + n > stride, WHO ": tensor %lld at src %lld does not fit a record of stride %lld", (long long)i, (long long)so, (long long)stride);
        OP_REFUSE(so >= 0 && (ntiles - 1) * stride + so + n > ws_floats, WHO ": ws of %lld floats below tensor %lld's last record", (long long)ws_floats, (long long)i);
        src.push_back(so);
      }
    }
    if (op == 4) OP_REFUSE(d[3] != DYN_ADAM_LRT && d[3] != DYN_ADAM_LRT_D, WHO ": lrt_slot = %lld is neither %d (G) nor %d (D)", (long long)d[3], (int)DYN_ADAM_LRT, (int)DYN_ADAM_LRT_D);
    // the table on the device for the length of the call
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> host;
    for (const std::vector<int>* v : {&h.tensor, &h.off, &h.len, &h.t_first, &h.t_count, &h.t_l2}) host.insert(host.end(), v->begin(), v->end());
    int* dev = nullptr;
    long long* dsrc = nullptr;
    HIPC(hipMalloc((void**)&dev, host.size() * sizeof(int)));
    struct Free { int*& a; long long*& b; ~Free() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); } } fr{dev, dsrc};
    HIPC(hipMemcpy(dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice));
    if (op == 1) {
      HIPC(hipMalloc((void**)&dsrc, src.size() * sizeof(long long)));
      HIPC(hipMemcpy(dsrc, src.data(), src.size() * sizeof(long long), hipMemcpyHostToDevice));
    }
    ChunkTable ct{};
    ct.tensor = dev; ct.off = dev + nc; ct.len = dev + 2 * nc;
    ct.t_first = dev + 3 * nc; ct.t_count = dev + 3 * nc + nt; ct.t_l2 = dev + 3 * nc + 2 * nt;
    ct.n_chunks = nc; ct.n_tensors = (int)nt;
    switch (op) {
      case 0: launch_sumsq(FP(0), ct, FP(1), s); break;
      case 1: launch_dw_reduce(FP(0), (size_t)d[3], (int)d[4], dsrc, FP(1), ct, FP(2), s); break;
      case 2: launch_l2(FP(0), FP(1), ct, FP(2), FP(3), s); break;
      case 3: launch_apply_sgd(FP(0), FP(1), FP(2), ct, FP(3), FP(4), s); break;
      default: launch_apply_adam(FP(0), FP(1), FP(2), FP(3), FP(4), ct, FP(5), FP(6), s, (int)d[3]); break;
    }
    OP_LAUNCH_OK(WHO);
    HIPC(hipStreamSynchronize(s));                       // (the table is freed on return)
    return RSRGAN_OK;
  });
}
#undef WHO

#define WHO "op_step_elem"
int rsrgan_op_step_elem(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream) {
  OP_REFUSE(!ptrs, WHO ": null table (ptrs)");
  OP_REFUSE(op < 0 || op > 8, WHO ": op = %d outside 0 .. 8", op);
  OP_REFUSE(op != 3 && !dims, WHO ": null table (dims)");
  OP_REFUSE((op == 0 || op >= 5) && !fl, WHO ": null table (fl: the clip bounds, the betas, keep or alpha)");
  const int64_t* d = dims;
  hipStream_t s = (hipStream_t)stream;
  switch (op) {
    case 0: {                                            // lsgan: ptrs logits, dlogits?, t_real, t_fake, loss3;  dims T, Nd, n_real, ldl, clip_on, Bp, Bt;  fl lo, hi
      OP_DIM("T", d[0], 1); OP_DIM("Nd", d[1], 1); OP_LD("ldl", d[3], 1); OP_FLAG("clip_on", d[4]);
      OP_REFUSE(d[2] < 0 || d[2] > d[1], WHO ": n_real = %lld outside 0 .. Nd = %lld", (long long)d[2], (long long)d[1]);
      OP_REFUSE(d[0] * d[1] > (1 << 24), WHO ": T x Nd above the entry's 2^24");
      OP_BP("Nd", d[1], d[5], d[6]); OP_BP("n_real", d[2], d[5], d[6]);
      OP_PTR("logits", ptrs[0], 4); OP_OPT("dlogits", ptrs[1], 4); OP_PTR("t_real", ptrs[2], 4); OP_PTR("t_fake", ptrs[3], 4); OP_PTR("loss3", ptrs[4], 4);
      launch_lsgan(FP(0), (int)d[3], FP(1), (int)d[0], (int)d[1], (int)d[2], FP(2), FP(3), FP(4), s, d[4] != 0, fl[0], fl[1], (int)d[5], (int)d[6]);
      break;
    }
    case 1: {                                            // dhead: ptrs top, w, b, logits, dlogits?, dout?, gw?, gb?, t_real, t_fake, loss3, part
      // dims T, Nd, n_real, dR, ldt, ldw, ldl, ldo, want_grads, want_wgrads, Bp, Bt, part_floats
      OP_DIM("T", d[0], 1); OP_DIM("Nd", d[1], 1); OP_DIM("dR", d[3], 1); OP_MUL4("dR", d[3]);
      OP_REFUSE(d[3] + 3 > 64, WHO ": dR = %lld above 60 (k_dhead2 sums 3 + dR <= 64 quantities)", (long long)d[3]);
      OP_REFUSE(d[2] < 0 || d[2] > d[1], WHO ": n_real = %lld outside 0 .. Nd = %lld", (long long)d[2], (long long)d[1]);
      OP_REFUSE(d[0] * d[1] > (1 << 24), WHO ": T x Nd above the entry's 2^24");
      OP_FLAG("want_grads", d[8]); OP_FLAG("want_wgrads", d[9]);
      OP_LD("ldt", d[4], d[3]); OP_MUL4("ldt", d[4]); OP_LD("ldw", d[5], 1); OP_LD("ldl", d[6], 1);
      if (d[8]) { OP_LD("ldo", d[7], d[3]); OP_MUL4("ldo", d[7]); }
      OP_BP("Nd", d[1], d[10], d[11]); OP_BP("n_real", d[2], d[10], d[11]);
      static const char* const names[12] = {"top", "w", "b", "logits", "dlogits", "dout", "gw", "gb", "t_real", "t_fake", "loss3", "part"};
      for (int i = 0; i < 12; ++i) {
        const bool wanted = i < 4 || i > 7 || (i < 6 ? d[8] != 0 : d[9] != 0);
        const int align = (i == 0 || i == 5) ? 16 : 4;
        if (wanted) OP_PTR(names[i], ptrs[i], align); else OP_OPT(names[i], ptrs[i], align);
      }
      const int64_t need = (d[0] * d[1] + 63) / 64 * (DH_MAXR + 3);
      OP_REFUSE(d[12] < need, WHO ": part of %lld floats below ceil(T x Nd / 64) x %d = %lld", (long long)d[12], DH_MAXR + 3, (long long)need);
      DHeadArgs a{};
      a.top = FP(0); a.ldt = (int)d[4]; a.w = FP(1); a.ldw = (int)d[5]; a.b = FP(2);
      a.logits = FP(3); a.ldl = (int)d[6]; a.dlogits = FP(4); a.dout = FP(5); a.ldo = (int)d[7]; a.gw = FP(6); a.gb = FP(7);
      a.T = (int)d[0]; a.Nd = (int)d[1]; a.n_real = (int)d[2]; a.dR = (int)d[3]; a.t_real = FP(8); a.t_fake = FP(9); a.loss3 = FP(10); a.part = FP(11);
      a.want_grads = (int)d[8]; a.want_wgrads = (int)d[9]; a.Bp = (int)d[10]; a.Bt = (int)d[11];
      launch_dhead(a, s);
      break;
    }
    case 2: {                                            // mse: ptrs y, lab, dy?, lambda, loss, scratch;  dims rows, D, ld, accumulate, Bp, Bt, scratch_floats
      OP_DIM("rows", d[0], 1); OP_DIM("D", d[1], 1); OP_LD("ld", d[2], d[1]); OP_FLAG("accumulate", d[3]);
      OP_REFUSE(d[0] * d[2] > ((int64_t)1 << 30), WHO ": rows x ld above the entry's 2^30");
      OP_BP("rows", d[0], d[4], d[5]);
      OP_REFUSE(d[6] < 1024, WHO ": scratch of %lld floats below launch_mse's 1024", (long long)d[6]);
      OP_PTR("y", ptrs[0], 4); OP_PTR("lab", ptrs[1], 4); OP_OPT("dy", ptrs[2], 4); OP_PTR("lambda", ptrs[3], 4); OP_PTR("loss", ptrs[4], 4); OP_PTR("scratch", ptrs[5], 4);
      launch_mse(FP(0), FP(1), (int)d[2], FP(2), (int)d[0], (int)d[1], FP(3), d[3] != 0, FP(4), FP(5), s, (int)d[4], (int)d[5]);
      break;
    }
    case 3:                                              // g_total: ptrs l4, lambda
      OP_PTR("l4", ptrs[0], 4); OP_PTR("lambda", ptrs[1], 4);
      launch_g_total(FP(0), FP(1), s);
      break;
    case 4:                                              // l2_total: ptrs partial, l2_scale, out;  dims n
      OP_DIM("n", d[0], 1);
      OP_PTR("partial", ptrs[0], 4); OP_PTR("l2_scale", ptrs[1], 4); OP_PTR("out", ptrs[2], 4);
      launch_l2_total(FP(0), (int)d[0], FP(1), FP(2), s);
      break;
    case 5: {                                            // adam_tick: ptrs dyn, t;  dims lr_slot, lrt_slot;  fl beta1, beta2
      const bool g = d[0] == DYN_G_LR && d[1] == DYN_ADAM_LRT, dd = d[0] == DYN_D_LR && d[1] == DYN_ADAM_LRT_D;
      OP_REFUSE(!g && !dd, WHO ": slots (%lld, %lld) are neither (%d, %d) (G) nor (%d, %d) (D)", (long long)d[0], (long long)d[1], (int)DYN_G_LR,
                (int)DYN_ADAM_LRT, (int)DYN_D_LR, (int)DYN_ADAM_LRT_D);
      OP_REFUSE(!(fl[0] >= 0.f && fl[0] < 1.f) || !(fl[1] >= 0.f && fl[1] < 1.f), WHO ": beta1 = %g or beta2 = %g outside [0, 1)", (double)fl[0], (double)fl[1]);
      OP_PTR("dyn", ptrs[0], 4); OP_PTR("t", ptrs[1], 4);
      launch_adam_tick(FP(0), (int*)ptrs[1], (double)fl[0], (double)fl[1], s, (int)d[0], (int)d[1]);
      break;
    }
    case 6: case 7: case 8: {                            // dropout_fwd: ptrs y;  dims rows, cols, ld, key, thr;  fl keep
      // dropout_bwd: ptrs y, d;  dims rows, cols, ld;  fl keep.   lrelu_bwd: ptrs h, d;  dims rows, cols, ld;  fl alpha
      OP_DIM("rows", d[0], 1); OP_DIM("cols", d[1], 1); OP_LD("ld", d[2], d[1]);
      OP_REFUSE(d[0] * d[2] > ((int64_t)1 << 30), WHO ": rows x ld above the entry's 2^30");
      if (op != 8) OP_REFUSE(!(fl[0] > 0.f && fl[0] <= 1.f), WHO ": keep = %g outside (0, 1]", (double)fl[0]);
      if (op == 6) OP_REFUSE(d[4] < 0 || d[4] > (1 << 24), WHO ": thr = %lld outside 0 .. 2^24", (long long)d[4]);
      OP_PTR(op == 8 ? "h" : "y", ptrs[0], 4);
      if (op != 6) OP_PTR("d", ptrs[1], 4);
      if (op == 6) launch_dropout_fwd(FP(0), (size_t)d[0], (int)d[1], (int)d[2], (unsigned long long)d[3], (unsigned)d[4], fl[0], s);
      else if (op == 7) launch_dropout_bwd(FP(0), FP(1), (size_t)d[0], (int)d[1], (int)d[2], fl[0], s);
      else launch_lrelu_bwd(FP(0), FP(1), (size_t)d[0], (int)d[1], (int)d[2], fl[0], s);
      break;
    }
  }
  OP_LAUNCHED(WHO);
}
#undef WHO

// ---- unit-test entry of the layout, staging and weight-copy kernels (kernels.hip: the batch-major <-> time-major packs, the
// discriminator's input rows, the transposed and fragment-tiled weight copies, R-CED's patch matrix and its adjoint, the carried state,
// the small buffer kernels) on caller-owned buffers (tests/test_gpu_layout_ops.py, test_layout_op_args.py).  Same form as the entries
// above; the list ops name a job's argument as "<name> of job <j>".
#define OP_JOB_NAME(buf, name, j) char buf[48]; snprintf(buf, sizeof(buf), "%s of job %d", name, (int)(j))
#define WHO "op_layout"
int rsrgan_op_layout(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream) {
  OP_REFUSE(!ptrs || !dims, WHO ": null table (ptrs or dims)");
  OP_REFUSE(op < 0 || op > 18, WHO ": op = %d outside 0 .. 18", op);
  OP_REFUSE(op == 14 && !fl, WHO ": null table (fl: the fill value)");
  const int64_t* d = dims;
  const int64_t lim = (int64_t)1 << 30;
  hipStream_t s = (hipStream_t)stream;
  switch (op) {
    case 0: case 1: {                                    // pack_tm / unpack_bm: ptrs src, dst;  dims B, T, D, ld (+ Bt)
      OP_DIM("B", d[0], 1); OP_DIM("T", d[1], 1); OP_DIM("D", d[2], 1); OP_LD("ld", d[3], d[2]);
      OP_REFUSE(d[0] * d[1] * d[3] > lim || d[0] > 65535, WHO ": B x T x ld above the entry's 2^30, or B above the grid's 65535");
      if (op == 1) OP_REFUSE(d[4] < 0 || d[4] > d[0], WHO ": Bt = %lld outside 0 (all rows) .. B = %lld", (long long)d[4], (long long)d[0]);
      OP_PTR("src", ptrs[0], 4); OP_PTR("dst", ptrs[1], 4);
      if (op == 0) launch_pack_tm(FP(0), FP(1), (int)d[0], (int)d[1], (int)d[2], (int)d[3], s);
      else launch_unpack_bm(FP(0), (int)d[3], FP(1), (int)d[0], (int)d[1], (int)d[2], s, (int)d[4]);
      break;
    }
    case 2: {                                            // stage_inputs: ptrs (src, dst) of pack 0, 1, of copy 0 .. 3;  dims B, T, Bt, D0, ld0, D1, ld1, n0 .. n3
      OP_DIM("B", d[0], 1); OP_DIM("T", d[1], 1);
      OP_REFUSE(d[0] > 65535, WHO ": B = %lld above the grid's 65535", (long long)d[0]);
      OP_REFUSE(d[2] < 0 || d[2] > d[0], WHO ": Bt = %lld outside 0 (all rows) .. B = %lld", (long long)d[2], (long long)d[0]);
      StageJobs j{};
      j.B = (int)d[0]; j.T = (int)d[1]; j.Bt = (int)d[2];
      for (int k = 0; k < 2; ++k) {
        if (!ptrs[2 * k]) continue;                      // (a NULL src skips the slot: its dst and sizes are not looked at)
        OP_JOB_NAME(ns, "src", k); OP_JOB_NAME(nd, "dst", k); OP_JOB_NAME(nD, "D", k); OP_JOB_NAME(nl, "ld", k);
        OP_PTR(ns, ptrs[2 * k], 4); OP_PTR(nd, ptrs[2 * k + 1], 4);
        OP_DIM(nD, d[3 + 2 * k], 1); OP_LD(nl, d[4 + 2 * k], d[3 + 2 * k]);
        OP_REFUSE(d[0] * d[1] * d[4 + 2 * k] > lim, WHO ": B x T x ld of pack %d above the entry's 2^30", k);
        j.pack[k] = StagePack{FP(2 * k), FP(2 * k + 1), (int)d[3 + 2 * k], (int)d[4 + 2 * k]};
      }
      for (int k = 0; k < 4; ++k) {
        if (!ptrs[4 + 2 * k]) continue;
        OP_JOB_NAME(ns, "copy src", k); OP_JOB_NAME(nd, "copy dst", k); OP_JOB_NAME(nn, "n", k);
        OP_PTR(ns, ptrs[4 + 2 * k], 4); OP_PTR(nd, ptrs[5 + 2 * k], 4); OP_DIM(nn, d[7 + k], 1);
        j.copy[k] = StageCopy{ptrs[4 + 2 * k], (void*)ptrs[5 + 2 * k], (int)d[7 + k]};
      }
      launch_stage_inputs(j, s);
      break;
    }
    case 3: {                                            // build_d_input: ptrs lab (with_real), y, nr?, nf?, xd;  dims B, T, D, ld, with_real
      OP_DIM("B", d[0], 1); OP_DIM("T", d[1], 1); OP_DIM("D", d[2], 1); OP_LD("ld", d[3], d[2]); OP_FLAG("with_real", d[4]);
      OP_REFUSE(2 * d[0] * d[1] * d[3] > lim, WHO ": 2 B x T x ld above the entry's 2^30");
      if (d[4]) OP_PTR("lab", ptrs[0], 4); else OP_OPT("lab", ptrs[0], 4);
      OP_PTR("y", ptrs[1], 4); OP_OPT("nr", ptrs[2], 4); OP_OPT("nf", ptrs[3], 4); OP_PTR("xd", ptrs[4], 4);
      launch_build_d_input(FP(0), FP(1), FP(2), FP(3), FP(4), (int)d[0], (int)d[1], (int)d[2], (int)d[3], d[4] != 0, s);
      break;
    }
    case 4: {                                            // add_noise_rows: ptrs src, noise?, dst;  dims B, T, D, ld, Ns, row0
      OP_DIM("B", d[0], 1); OP_DIM("T", d[1], 1); OP_DIM("D", d[2], 1); OP_LD("ld", d[3], d[2]); OP_DIM("Ns", d[4], 1); OP_DIM("row0", d[5], 0);
      OP_REFUSE(d[5] + d[0] > d[4], WHO ": rows [row0 = %lld, row0 + B = %lld) outside Ns = %lld", (long long)d[5], (long long)(d[5] + d[0]), (long long)d[4]);
      OP_REFUSE(d[4] * d[1] * d[3] > lim, WHO ": Ns x T x ld above the entry's 2^30");
      OP_PTR("src", ptrs[0], 4); OP_OPT("noise", ptrs[1], 4); OP_PTR("dst", ptrs[2], 4);
      launch_add_noise_rows(FP(0), FP(1), FP(2), (int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4], (int)d[5], s);
      break;
    }
    case 5: {                                            // transpose: ptrs src, dst;  dims lds, ldd, R, C
      OP_DIM("R", d[2], 1); OP_DIM("C", d[3], 1); OP_LD("lds", d[0], d[3]); OP_LD("ldd", d[1], d[2]);
      OP_REFUSE(d[2] * d[0] > lim || d[3] * d[1] > lim || d[2] > (65535 << 5), WHO ": R x lds or C x ldd above the entry's 2^30, or R above the grid's 65535 tiles");
      OP_PTR("src", ptrs[0], 4); OP_PTR("dst", ptrs[1], 4);
      launch_transpose(FP(0), (int)d[0], FP(1), (int)d[1], (int)d[2], (int)d[3], s);
      break;
    }
    case 6: {                                            // transpose_many: ptrs (src, dst) per job;  dims n, then lds, ldd, R, C per job
      TransposeList tl{};
      OP_REFUSE(d[0] < 1 || d[0] > (int64_t)(sizeof(tl.j) / sizeof(tl.j[0])), WHO ": n = %lld jobs outside the list (1 .. %d)", (long long)d[0],
                (int)(sizeof(tl.j) / sizeof(tl.j[0])));
      tl.n = (int)d[0];
      for (int j = 0; j < tl.n; ++j) {
        const int64_t* q = d + 1 + 4 * j;
        OP_JOB_NAME(ns, "src", j); OP_JOB_NAME(nd, "dst", j); OP_JOB_NAME(nR, "R", j); OP_JOB_NAME(nC, "C", j); OP_JOB_NAME(n0, "lds", j); OP_JOB_NAME(n1, "ldd", j);
        OP_DIM(nR, q[2], 1); OP_DIM(nC, q[3], 1); OP_LD(n0, q[0], q[3]); OP_LD(n1, q[1], q[2]);
        OP_REFUSE(q[2] * q[0] > ((int64_t)1 << 26) || q[3] * q[1] > ((int64_t)1 << 26), WHO ": R x lds or C x ldd of job %d above the entry's 2^26", j);
        OP_PTR(ns, ptrs[2 * j], 4); OP_PTR(nd, ptrs[2 * j + 1], 4);
        tl.j[j] = TransposeJob{FP(2 * j), FP(2 * j + 1), (int)q[0], (int)q[1], (int)q[2], (int)q[3], 0};
      }
      launch_transpose_many(tl, s);
      break;
    }
    case 7: {                                            // swizzle_many: ptrs (src, dst) per job;  dims n, then ld, gates, H, C, c0, K1, I, P, kx, nct, nkb per job
      SwizzleList sl{};
      OP_REFUSE(d[0] < 1 || d[0] > (int64_t)(sizeof(sl.j) / sizeof(sl.j[0])), WHO ": n = %lld jobs outside the list (1 .. %d)", (long long)d[0],
                (int)(sizeof(sl.j) / sizeof(sl.j[0])));
      sl.n = (int)d[0];
      for (int j = 0; j < sl.n; ++j) {
        const int64_t* q = d + 1 + 11 * j;
        const int64_t ld = q[0], gates = q[1], H = q[2], C_ = q[3], c0 = q[4], K1 = q[5], I = q[6], P = q[7], kx = q[8], nct = q[9], nkb = q[10];
        OP_JOB_NAME(ns, "src", j); OP_JOB_NAME(nd, "dst", j); OP_JOB_NAME(nl, "ld", j); OP_JOB_NAME(nn, "nct", j); OP_JOB_NAME(nk, "nkb", j);
        OP_DIM(nn, nct, 1); OP_DIM(nk, nkb, 1);
        OP_REFUSE(nct * nkb > ((int64_t)1 << 20), WHO ": nct x nkb of job %d above the entry's 2^20 tiles", j);
        OP_REFUSE(gates < 0 || gates > 4, WHO ": gates = %lld of job %d outside 0 (rows of a k-contiguous matrix) .. 4", (long long)gates, j);
        if (gates == 0) {
          OP_JOB_NAME(nC, "C", j); OP_JOB_NAME(n0, "c0", j); OP_JOB_NAME(nK, "K1", j);
          OP_DIM(nC, C_, 1); OP_DIM(n0, c0, 0); OP_DIM(nK, K1, 1); OP_LD(nl, ld, K1);
          OP_REFUSE((c0 + C_) * ld > lim, WHO ": (c0 + C) x ld of job %d above the entry's 2^30", j);
        } else {
          OP_JOB_NAME(nH, "H", j); OP_JOB_NAME(nI, "I", j); OP_JOB_NAME(nP, "P", j); OP_JOB_NAME(nx, "kx", j);
          OP_DIM(nH, H, 1); OP_DIM(nI, I, 0); OP_DIM(nP, P, 0); OP_DIM(nx, kx, 0); OP_LD(nl, ld, gates * H);
          OP_REFUSE(I + P < 1 || (I + P) * ld > lim, WHO ": I + P = %lld source rows of job %d below 1, or (I + P) x ld above the entry's 2^30", (long long)(I + P), j);
          OP_REFUSE(nct < gates * ((H + 15) / 16), WHO ": nct = %lld of job %d below gates x ceil(H / 16) = %lld: the logical matrix must cover the source",
                    (long long)nct, j, (long long)(gates * ((H + 15) / 16)));
        }
        OP_PTR(ns, ptrs[2 * j], 4); OP_PTR(nd, ptrs[2 * j + 1], 16);
        sl.j[j] = SwizzleJob{FP(2 * j), FP(2 * j + 1), (int)ld, (int)gates, (int)H, (int)C_, (int)c0, (int)K1, (int)I, (int)P, (int)kx, (int)nct, (int)nkb, 0};
      }
      launch_swizzle_many(sl, s);
      break;
    }
    case 8: case 9: {                                    // im2col: ptrs src, col;  dims row_stride, ldc, C, S, W, kh, kw, ldk, M
      // col2im: ptrs dcol, dst;  dims ldk, C, S, W, kh, kw, ldc, M
      const int64_t rs = op == 8 ? d[0] : 0, ldc = op == 8 ? d[1] : d[6], C_ = op == 8 ? d[2] : d[1], S = op == 8 ? d[3] : d[2], W = op == 8 ? d[4] : d[3],
                    kh = op == 8 ? d[5] : d[4], kw = op == 8 ? d[6] : d[5], ldk = op == 8 ? d[7] : d[0], M = op == 8 ? d[8] : d[7];
      OP_DIM("C", C_, 1); OP_DIM("S", S, 1); OP_DIM("W", W, 1); OP_DIM("kh", kh, 1); OP_DIM("kw", kw, 1); OP_DIM("M", M, 1);
      OP_REFUSE(kh * kw * C_ > ((int64_t)1 << 24), WHO ": kh x kw x C above the entry's 2^24");
      OP_REFUSE(M % (S * W), WHO ": M = %lld positions are no whole frames of S x W = %lld", (long long)M, (long long)(S * W));
      OP_LD("ldc", ldc, C_); OP_LD("ldk", ldk, kh * kw * C_);
      OP_REFUSE(M * ldk > lim || M * ldc > lim, WHO ": M x ldk or M x ldc above the entry's 2^30");
      if (op == 8) {
        OP_LD("row_stride", rs, (S * W - 1) * ldc + C_);
        const int al = (C_ % 4 == 0 && ldc % 4 == 0) ? 16 : 4;      // launch_im2col's float4 form looks at C and ldc alone
        if (al == 16) { OP_MUL4("row_stride", rs); OP_MUL4("ldk", ldk); }
        OP_PTR("src", ptrs[0], al); OP_PTR("col", ptrs[1], al);
        launch_im2col(FP(0), (size_t)rs, (int)ldc, (int)C_, (int)S, (int)W, (int)kh, (int)kw, FP(1), (int)ldk, (size_t)M, s);
      } else {
        OP_MUL4("C", C_); OP_MUL4("ldc", ldc); OP_MUL4("ldk", ldk);
        OP_PTR("dcol", ptrs[0], 16); OP_PTR("dst", ptrs[1], 16);
        launch_col2im(FP(0), (int)ldk, (int)C_, (int)S, (int)W, (int)kh, (int)kw, FP(1), (int)ldc, (size_t)M, s);
      }
      break;
    }
    case 10: {                                           // expand_c4: ptrs src, dst;  dims ld_src, n, rows
      OP_DIM("n", d[1], 1); OP_DIM("rows", d[2], 1); OP_LD("ld_src", d[0], d[1]);
      OP_REFUSE(d[2] * d[0] > lim || d[2] * d[1] * 4 > lim, WHO ": rows x ld_src or rows x n x 4 above the entry's 2^30");
      OP_PTR("src", ptrs[0], 4); OP_PTR("dst", ptrs[1], 16);
      launch_expand_c4(FP(0), (int)d[0], (int)d[1], FP(1), (size_t)d[2], s);
      break;
    }
    case 11: {                                           // gstate: ptrs state, mask?, then (c, mst) per layer;  dims nl, SF, rows, dir, slot, then H, P, ldP, off per layer
      OP_REFUSE(d[0] < 1 || d[0] > GP_MAXL, WHO ": nl = %lld layers outside 1 .. %d", (long long)d[0], GP_MAXL);
      OP_DIM("SF", d[1], 1); OP_DIM("rows", d[2], 0); OP_DIM("slot", d[4], 0);
      OP_REFUSE(d[2] > 65535, WHO ": rows = %lld above the grid's 65535", (long long)d[2]);
      OP_REFUSE(d[3] < 0 || d[3] > 2, WHO ": dir = %lld outside 0 (state -> slot), 1 (slot -> state), 2 (zero)", (long long)d[3]);
      OP_PTR("state", ptrs[0], 4); OP_OPT("mask", ptrs[1], 4);
      GStateArgs a{};
      a.nl = (int)d[0]; a.SF = (int)d[1]; a.rows = (int)d[2]; a.dir = (int)d[3]; a.state = FP(0); a.slot = (size_t)d[4]; a.mask = (const int*)ptrs[1];
      for (int l = 0; l < a.nl; ++l) {
        const int64_t* q = d + 5 + 4 * l;
        OP_JOB_NAME(nc, "c", l); OP_JOB_NAME(nm, "mst", l); OP_JOB_NAME(nH, "H", l); OP_JOB_NAME(nP, "P", l); OP_JOB_NAME(nl, "ldP", l);
        OP_DIM(nH, q[0], 1); OP_DIM(nP, q[1], 0); OP_LD(nl, q[2], q[1]);
        OP_REFUSE(q[3] < 0 || q[3] + q[0] + q[1] > d[1], WHO ": layer %d at offset %lld with H + P = %lld does not fit SF = %lld", l, (long long)q[3],
                  (long long)(q[0] + q[1]), (long long)d[1]);
        OP_REFUSE((d[4] + d[2]) * std::max(q[0], q[2]) > lim, WHO ": (slot + rows) x H or ldP of layer %d above the entry's 2^30", l);
        if (a.dir < 2) {                                 // (dir 2 touches the state alone; a layer without a projection, ldP = 0, has no mst)
          OP_PTR(nc, ptrs[2 + 2 * l], 4);
          if (q[2] > 0) OP_PTR(nm, ptrs[3 + 2 * l], 4);
        }
        a.L[l] = GStateLayer{FP(2 + 2 * l), FP(3 + 2 * l), (int)q[0], (int)q[1], (int)q[2], (int)q[3]};
      }
      OP_REFUSE(d[2] * d[1] > lim, WHO ": rows x SF above the entry's 2^30");
      launch_gstate(a, s);
      break;
    }
    case 12: {                                           // window_len: ptrs len, dst (int32);  dims n, t0, Tw
      OP_DIM("n", d[0], 0); OP_DIM("t0", d[1], 0); OP_DIM("Tw", d[2], 0);
      OP_PTR("len", ptrs[0], 4); OP_PTR("dst", ptrs[1], 4);
      launch_window_len((const int*)ptrs[0], (int*)ptrs[1], (int)d[0], (int)d[1], (int)d[2], s);
      break;
    }
    case 13: {                                           // zero_many: ptrs p per buffer;  dims n, then the floats of each
      ZeroList zl{};
      OP_REFUSE(d[0] < 1 || d[0] > (int64_t)(sizeof(zl.p) / sizeof(zl.p[0])), WHO ": n = %lld buffers outside the list (1 .. %d)", (long long)d[0],
                (int)(sizeof(zl.p) / sizeof(zl.p[0])));
      zl.n = (int)d[0];
      for (int j = 0; j < zl.n; ++j) {
        OP_JOB_NAME(np_, "p", j); OP_JOB_NAME(nn, "len", j);
        OP_DIM(nn, d[1 + j], 1); OP_PTR(np_, ptrs[j], 4);
        zl.p[j] = FP(j); zl.len[j] = (unsigned)d[1 + j];
      }
      launch_zero_many(zl, s);
      break;
    }
    case 14:                                             // fill: ptrs p;  dims n;  fl v
      OP_DIM("n", d[0], 1); OP_PTR("p", ptrs[0], 4);
      launch_fill(FP(0), (size_t)d[0], fl[0], s);
      break;
    case 15: {                                           // build_joint: ptrs x (dim > 0), tail, joint;  dims ldx, off, dim, ldt, Dt, ldj, row0, R
      OP_DIM("off", d[1], 0); OP_DIM("dim", d[2], 0); OP_DIM("Dt", d[4], 1); OP_DIM("row0", d[6], 0); OP_DIM("R", d[7], 1);
      if (d[2] > 0) { OP_LD("ldx", d[0], d[1] + d[2]); OP_PTR("x", ptrs[0], 4); } else OP_OPT("x", ptrs[0], 4);
      OP_LD("ldt", d[3], d[4]); OP_LD("ldj", d[5], d[2] + d[4]);
      OP_REFUSE((d[6] + d[7]) * d[5] > lim || d[7] * std::max(d[0], d[3]) > lim, WHO ": (row0 + R) x ldj, R x ldx or R x ldt above the entry's 2^30");
      OP_PTR("tail", ptrs[1], 4); OP_PTR("joint", ptrs[2], 4);
      launch_build_joint(FP(0), (int)d[0], (int)d[1], (int)d[2], FP(1), (int)d[3], (int)d[4], FP(2), (int)d[5], (int)d[6], (int)d[7], s);
      break;
    }
    case 16: {                                           // slice_cols: ptrs src, dst;  dims lds, off, ldd, R, C
      OP_DIM("off", d[1], 0); OP_DIM("R", d[3], 1); OP_DIM("C", d[4], 1); OP_LD("lds", d[0], d[1] + d[4]); OP_LD("ldd", d[2], d[4]);
      OP_REFUSE(d[3] * std::max(d[0], d[2]) > lim, WHO ": R x lds or R x ldd above the entry's 2^30");
      OP_PTR("src", ptrs[0], 4); OP_PTR("dst", ptrs[1], 4);
      launch_slice_cols(FP(0), (int)d[0], (int)d[1], FP(1), (int)d[2], (int)d[3], (int)d[4], s);
      break;
    }
    case 17: {                                           // pad_copy: ptrs dense, padded;  dims rows, cols, ld, to_padded
      OP_DIM("rows", d[0], 1); OP_DIM("cols", d[1], 1); OP_LD("ld", d[2], d[1]); OP_FLAG("to_padded", d[3]);
      OP_REFUSE(d[0] * d[2] > lim, WHO ": rows x ld above the entry's 2^30");
      OP_PTR("dense", ptrs[0], 4); OP_PTR("padded", ptrs[1], 4);
      launch_pad_copy(FP(0), FP(1), (int)d[0], (int)d[1], (int)d[2], d[3] != 0, s);
      break;
    }
    default:                                             // copy_f: ptrs src, dst;  dims n
      OP_DIM("n", d[0], 1); OP_PTR("src", ptrs[0], 4); OP_PTR("dst", ptrs[1], 4);
      launch_copy_f(FP(0), FP(1), (int)d[0], s);
      break;
  }
  OP_LAUNCHED(WHO);
}
#undef WHO
#undef OP_JOB_NAME

// ---- unit-test entry of the launch-per-phase LSTM step kernels (kernels.hip k_fwd_gates, k_fwd_proj, k_bwd_a2, k_bwd_b, k_bwd_bp +
// k_bwd_b_red) through their five launchers, on caller-owned buffers and without a handle (tests/test_gpu_lstm_step_ops.py,
// test_lstm_step_op_args.py).  dims[0] = n jobs (1 .. MAXJ), then one fixed-length record per job; ptrs one fixed-length group per job; a
// NULL pointer selects the optional forms as kernels.h documents them.  The job structs are filled field by field, nblk_c and kb_max with
// model.cpp's expressions (fill_gate .. fill_bwd_b, kb16), and the unchanged launch_* function runs.  The refusals include the kernels' own
// limits (their register weight slices, their float4 moves, the stand-in reads of their optional operands).
#define SJ(name) (snprintf(nbuf, sizeof(nbuf), "%s of job %d", name, j), nbuf)
static inline int op_kb16(int64_t ld) { return (int)((ld + 15) >> 4); }
#define WHO "op_lstm_step"
int rsrgan_op_lstm_step(int32_t op, const void* const* ptrs, const int64_t* dims, const float* fl, void* stream) {
  OP_REFUSE(!ptrs || !dims, WHO ": null table (ptrs or dims)");
  OP_REFUSE(op < 0 || op > 4, WHO ": op = %d outside 0 .. 4", op);
  OP_REFUSE(op == 0 && !fl, WHO ": null table (fl: forget_bias)");
  OP_REFUSE(dims[0] < 1 || dims[0] > MAXJ, WHO ": n = %lld jobs outside 1 .. %d", (long long)dims[0], MAXJ);
  const int n = (int)dims[0];
  const int64_t lim = (int64_t)1 << 30;
  hipStream_t s = (hipStream_t)stream;
  char nbuf[64];
  switch (op) {
    case 0: {      // fwd_gates: ptrs x?, KxT?, m, KhT?, Wsw, zx?, bias?, wf, wi, wo, c_prev, c_out, gates, h, len, np_m_out?, np_out?, np_res_in?, np_res_out?
      FwdGateJobs jobs{};                                //            dims N, H, ldx, ldm, ldh, t;  fl forget_bias
      jobs.n = n; jobs.forget_bias = fl[0];
      int kb_max = 0, blocks = 0;
      for (int j = 0; j < n; ++j) {
        const void* const* p = ptrs + 19 * j;
        const int64_t* q = dims + 1 + 6 * j;
        const int64_t N = q[0], H = q[1], ldx = q[2], ldm = q[3], ldh = q[4], t = q[5];
        OP_DIM(SJ("N"), N, 1); OP_DIM(SJ("H"), H, 1); OP_DIM(SJ("t"), t, 0);
        OP_REFUSE(!p[0] && !p[5], WHO ": null pointer (%s): one of x and zx holds the x-part", SJ("x and zx"));
        OP_REFUSE(p[0] && p[5], WHO ": %s both given: zx holds the x-part, or x is multiplied", SJ("x and zx"));
        if (p[0]) { OP_LD(SJ("ldx"), ldx, 4); OP_MUL4(SJ("ldx"), ldx); OP_PTR(SJ("x"), p[0], 16); OP_PTR(SJ("bias"), p[6], 4); }
        else OP_PTR(SJ("zx"), p[5], 4);
        OP_LD(SJ("ldm"), ldm, 4); OP_MUL4(SJ("ldm"), ldm); OP_LD(SJ("ldh"), ldh, H);
        const int64_t ktot = (p[0] ? ldx : 0) + ldm;
        OP_REFUSE(ktot > 1024, WHO ": %s = %lld above 1024: a wave of k_fwd_gates holds at most 32 k-blocks of weights", SJ("ldx + ldm"), (long long)ktot);
        OP_REFUSE(N * std::max(std::max(p[0] ? ldx : 0, ldm), std::max(ldh, 4 * H)) > lim, WHO ": %s above the entry's 2^30", SJ("N x ld"));
        OP_OPT(SJ("KxT"), p[1], 4); OP_PTR(SJ("m"), p[2], 16); OP_OPT(SJ("KhT"), p[3], 4); OP_PTR(SJ("Wsw"), p[4], 16);
        OP_OPT(SJ("bias"), p[6], 4); OP_PTR(SJ("wf"), p[7], 4); OP_PTR(SJ("wi"), p[8], 4); OP_PTR(SJ("wo"), p[9], 4);
        OP_PTR(SJ("c_prev"), p[10], 4); OP_PTR(SJ("c_out"), p[11], 4); OP_PTR(SJ("gates"), p[12], 4); OP_PTR(SJ("h"), p[13], 4);
        OP_PTR(SJ("len"), p[14], 4);
        OP_OPT(SJ("np_m_out"), p[15], 4); OP_OPT(SJ("np_out"), p[16], 4); OP_OPT(SJ("np_res_in"), p[17], 4); OP_OPT(SJ("np_res_out"), p[18], 4);
        if (p[15]) {
          OP_REFUSE(ldm < H, WHO ": leading dimension %s = %lld below its row of %lld (m = h without a projection)", SJ("ldm"), (long long)ldm, (long long)H);
          OP_REFUSE(p[18] && !p[17], WHO ": null pointer (%s): np_res_out = h + np_res_in", SJ("np_res_in"));
        } else OP_REFUSE(p[16] || p[17] || p[18], WHO ": %s given without np_m_out", SJ("np_out, np_res_in or np_res_out"));
        FwdGateJob& a = jobs.j[j];
        a.x = (const float*)p[0]; a.KxT = (const float*)p[1]; a.m = (const float*)p[2]; a.KhT = (const float*)p[3]; a.Wsw = (const float*)p[4];
        a.zx = (const float*)p[5]; a.bias = (const float*)p[6]; a.wf = (const float*)p[7]; a.wi = (const float*)p[8]; a.wo = (const float*)p[9];
        a.c_prev = (const float*)p[10]; a.c_out = (float*)p[11]; a.gates = (float*)p[12]; a.h = (float*)p[13]; a.len = (const int*)p[14];
        a.np_m_out = (float*)p[15]; a.np_out = (float*)p[16]; a.np_res_in = (const float*)p[17]; a.np_res_out = (float*)p[18];
        a.ldx = p[0] ? (int)ldx : 0; a.ldm = (int)ldm; a.ldh = (int)ldh; a.t = (int)t; a.N = (int)N; a.H = (int)H;
        a.nblk_c = (int)((H + 15) / 16);
        kb_max = std::max(kb_max, (p[0] ? op_kb16(ldx) : 0) + op_kb16(ldm));
        blocks += job_blocks(a.nblk_c, a.N, fwd_gates_rows());
      }
      launch_fwd_gates(jobs, blocks, kb_max, s);
      break;
    }
    case 1: {      // fwd_proj: ptrs h, WpT, WpT_sw?, m_prev?, m_out, out, res_in?, res_out?, len?, bias?, noise?, drop_ctr?
      FwdProjJobs jobs{};                                //           dims N, P, ldh, ldm, ldo, t, drop seed, tag, thr;  fl keep per job
      jobs.n = n;
      int kb_max = 0, blocks = 0;
      for (int j = 0; j < n; ++j) {
        const void* const* p = ptrs + 12 * j;
        const int64_t* q = dims + 1 + 9 * j;
        const int64_t N = q[0], P = q[1], ldh = q[2], ldm = q[3], ldo = q[4], t = q[5];
        OP_DIM(SJ("N"), N, 1); OP_DIM(SJ("P"), P, 1); OP_DIM(SJ("t"), t, 0);
        OP_LD(SJ("ldh"), ldh, 4); OP_MUL4(SJ("ldh"), ldh); OP_LD(SJ("ldm"), ldm, P); OP_LD(SJ("ldo"), ldo, P);
        OP_REFUSE(N * std::max(ldh, std::max(ldm, ldo)) > lim || P * ldh > lim, WHO ": %s above the entry's 2^30", SJ("N x ld or P x ldh"));
        OP_PTR(SJ("h"), p[0], 16); OP_PTR(SJ("WpT"), p[1], 16); OP_OPT(SJ("WpT_sw"), p[2], 16); OP_OPT(SJ("m_prev"), p[3], 4);
        OP_PTR(SJ("m_out"), p[4], 4); OP_PTR(SJ("out"), p[5], 4); OP_OPT(SJ("res_in"), p[6], 4); OP_OPT(SJ("res_out"), p[7], 4);
        OP_OPT(SJ("len"), p[8], 4); OP_OPT(SJ("bias"), p[9], 4); OP_OPT(SJ("noise"), p[10], 4); OP_OPT(SJ("drop_ctr"), p[11], 8);
        OP_REFUSE(p[8] && !p[3], WHO ": null pointer (%s): masked rows keep m_prev", SJ("m_prev"));
        OP_REFUSE(p[7] && !p[6], WHO ": null pointer (%s): res_out = out + res_in", SJ("res_in"));
        OP_REFUSE(!p[8] && N > P * ldh, WHO ": %s = %lld above P x ldh = %lld without len: k_fwd_proj reads the stand-in of len from WpT", SJ("N"),
                  (long long)N, (long long)(P * ldh));
        FwdProjJob& a = jobs.j[j];
        if (p[11]) {
          OP_REFUSE(!fl, WHO ": null table (fl: keep of a job with drop_ctr)");
          OP_REFUSE(!(fl[j] > 0.f && fl[j] <= 1.f), WHO ": %s = %g outside (0, 1]", SJ("keep"), (double)fl[j]);
          OP_REFUSE(q[8] < 0 || q[8] > (1 << 24), WHO ": %s = %lld outside 0 .. 2^24", SJ("thr"), (long long)q[8]);
          a.drop = DropSpec{(const unsigned long long*)p[11], (unsigned long long)q[6], (unsigned long long)q[7], (unsigned)q[8], fl[j]};
        }
        a.h = (const float*)p[0]; a.WpT = (const float*)p[1]; a.WpT_sw = (const float*)p[2]; a.m_prev = (const float*)p[3]; a.m_out = (float*)p[4];
        a.out = (float*)p[5]; a.res_in = (const float*)p[6]; a.res_out = (float*)p[7]; a.len = (const int*)p[8]; a.bias = (const float*)p[9];
        a.noise = (const float*)p[10];
        a.ldh = (int)ldh; a.ldm = (int)ldm; a.ldo = (int)ldo; a.P = (int)P; a.t = (int)t; a.N = (int)N;
        a.nblk_c = (int)((P + 15) / 16);
        kb_max = std::max(kb_max, op_kb16(ldh));
        blocks += job_blocks(a.nblk_c, a.N);
      }
      launch_fwd_proj(jobs, blocks, kb_max, s);
      break;
    }
    case 2: {      // bwd_a: ptrs dout?, dmst, Wp?, Wp_sw?, dmt (NULL without a projection), gates, c_prev, c_cur, wf, wi, wo, dc, len, drop_ctr?
      BwdAJobs jobs{};                                   //        dims N, P, H, ldm, t, drop seed, tag, thr;  fl keep per job
      jobs.n = n;
      int kb_max = 0, blocks = 0;
      for (int j = 0; j < n; ++j) {
        const void* const* p = ptrs + 14 * j;
        const int64_t* q = dims + 1 + 8 * j;
        const int64_t N = q[0], P = q[1], H = q[2], ldm = q[3], t = q[4];
        OP_DIM(SJ("N"), N, 1); OP_DIM(SJ("P"), P, 1); OP_DIM(SJ("H"), H, 1); OP_DIM(SJ("t"), t, 0);
        OP_LD(SJ("ldm"), ldm, P); OP_MUL4(SJ("ldm"), ldm);
        OP_REFUSE(N * std::max(ldm, 4 * H) > lim, WHO ": %s above the entry's 2^30", SJ("N x ldm or N x 4H"));
        OP_REFUSE(!p[2] != !p[3], WHO ": null pointer (%s): a projected job needs both, num_proj=None neither", SJ(p[2] ? "Wp_sw" : "Wp"));
        if (p[2]) {
          OP_REFUSE(ldm > 384, WHO ": %s = %lld above 384 with a projection: a wave of k_bwd_a2 holds at most 24 k-blocks of weights", SJ("ldm"), (long long)ldm);
          OP_PTR(SJ("dmt"), p[4], 16);
        } else {
          OP_REFUSE(P != H, WHO ": %s = %lld is not H = %lld without a projection (m = h)", SJ("P"), (long long)P, (long long)H);
          OP_OPT(SJ("dmt"), p[4], 16);
        }
        OP_OPT(SJ("dout"), p[0], 16); OP_PTR(SJ("dmst"), p[1], 16); OP_OPT(SJ("Wp"), p[2], 4); OP_OPT(SJ("Wp_sw"), p[3], 16);
        OP_PTR(SJ("gates"), p[5], 4); OP_PTR(SJ("c_prev"), p[6], 4); OP_PTR(SJ("c_cur"), p[7], 4); OP_PTR(SJ("wf"), p[8], 4);
        OP_PTR(SJ("wi"), p[9], 4); OP_PTR(SJ("wo"), p[10], 4); OP_PTR(SJ("dc"), p[11], 4); OP_PTR(SJ("len"), p[12], 4);
        OP_OPT(SJ("drop_ctr"), p[13], 8);
        BwdAJob& a = jobs.j[j];
        if (p[13]) {
          OP_REFUSE(!fl, WHO ": null table (fl: keep of a job with drop_ctr)");
          OP_REFUSE(!(fl[j] > 0.f && fl[j] <= 1.f), WHO ": %s = %g outside (0, 1]", SJ("keep"), (double)fl[j]);
          OP_REFUSE(q[7] < 0 || q[7] > (1 << 24), WHO ": %s = %lld outside 0 .. 2^24", SJ("thr"), (long long)q[7]);
          a.drop = DropSpec{(const unsigned long long*)p[13], (unsigned long long)q[5], (unsigned long long)q[6], (unsigned)q[7], fl[j]};
        }
        a.dout = (const float*)p[0]; a.dmst = (const float*)p[1]; a.Wp = (const float*)p[2]; a.Wp_sw = (const float*)p[3]; a.dmt = (float*)p[4];
        a.gates = (float*)p[5]; a.c_prev = (const float*)p[6]; a.c_cur = (const float*)p[7]; a.wf = (const float*)p[8]; a.wi = (const float*)p[9];
        a.wo = (const float*)p[10]; a.dc = (float*)p[11]; a.len = (const int*)p[12];
        a.ldm = (int)ldm; a.P = (int)P; a.t = (int)t; a.N = (int)N; a.H = (int)H;
        a.nblk_c = (int)((H + bwd_a_cells() - 1) / bwd_a_cells());
        kb_max = std::max(kb_max, op_kb16(ldm));
        blocks += job_blocks(a.nblk_c, a.N);
      }
      launch_bwd_a(jobs, blocks, kb_max, s);
      break;
    }
    default: {     // bwd_b, bwd_b_splitk: ptrs dz, K?, Ksw?, dx?, dmst?, len?;  dims N, I, n_begin, n_end, lddx, ldm, t, H4, dx_accumulate
      BwdBJobs jobs{};                                   // bwd_b_splitk: ptrs[6 n] = ws, dims[1 + 9 n] = the floats of ws
      jobs.n = n;
      int kb_max = 0, blocks = 0;
      for (int j = 0; j < n; ++j) {
        const void* const* p = ptrs + 6 * j;
        const int64_t* q = dims + 1 + 9 * j;
        const int64_t N = q[0], I = q[1], nb = q[2], ne = q[3], lddx = q[4], ldm = q[5], t = q[6], H4 = q[7];
        OP_DIM(SJ("N"), N, 1); OP_DIM(SJ("I"), I, 0); OP_DIM(SJ("n_begin"), nb, 0); OP_DIM(SJ("t"), t, 0); OP_FLAG(SJ("dx_accumulate"), q[8]);
        OP_REFUSE(ne <= nb || ne > lim, WHO ": %s = %lld not above n_begin = %lld (or above 2^30)", SJ("n_end"), (long long)ne, (long long)nb);
        OP_LD(SJ("H4"), H4, 4); OP_MUL4(SJ("H4"), H4);
        OP_PTR(SJ("dz"), p[0], 16); OP_OPT(SJ("K"), p[1], 16); OP_OPT(SJ("Ksw"), p[2], 16); OP_OPT(SJ("dx"), p[3], 4); OP_OPT(SJ("dmst"), p[4], 4);
        OP_OPT(SJ("len"), p[5], 4);
        OP_REFUSE(!p[1] && !p[2], WHO ": null pointer (%s): the row-major K or its fragment-tiled copy", SJ("K and Ksw"));
        if (nb < I) { OP_PTR(SJ("dx"), p[3], 4); OP_LD(SJ("lddx"), lddx, std::min(I, ne)); }
        if (ne > I) { OP_PTR(SJ("dmst"), p[4], 4); OP_LD(SJ("ldm"), ldm, ne - I); }
        OP_REFUSE(N * std::max(H4, std::max(nb < I ? lddx : 0, ne > I ? ldm : 0)) > lim || ne * H4 > lim, WHO ": %s above the entry's 2^30",
                  SJ("N x ld or n_end x H4"));
        BwdBJob& b = jobs.j[j];
        b.dz = (const float*)p[0]; b.K = (const float*)p[1]; b.Ksw = (const float*)p[2]; b.dx = (float*)p[3]; b.dmst = (float*)p[4];
        b.len = (const int*)p[5];
        b.I = (int)I; b.n_begin = (int)nb; b.n_end = (int)ne; b.lddx = (int)lddx; b.ldm = (int)ldm; b.t = (int)t; b.N = (int)N; b.H4 = (int)H4;
        b.dx_accumulate = (int)q[8];
        b.nblk_c = (int)((ne - nb + 15) / 16);
        kb_max = std::max(kb_max, op_kb16(H4));
        blocks += job_blocks(b.nblk_c, b.N, op_kb16(H4) <= 64 ? 16 : 32);
      }
      if (op == 3) { launch_bwd_b(jobs, blocks, kb_max, s); break; }
      const int64_t ws_floats = dims[1 + 9 * n];
      OP_PTR("ws", ptrs[6 * n], 4);
      const size_t need = bwd_b_plan(jobs, nullptr);
      OP_REFUSE(ws_floats < 0 || (size_t)ws_floats < need, WHO ": ws of %lld floats below the plan's need of %lld", (long long)ws_floats, (long long)need);
      for (int j = 0; j < n; ++j)
        OP_REFUSE((jobs.j[j].kpg + 1) / 2 > 12, WHO ": %s = %d: a wave of k_bwd_bp holds at most 12 k-blocks of weights, (kpg + 1) / 2", SJ("kpg"),
                  jobs.j[j].kpg);
      bwd_b_plan(jobs, (float*)ptrs[6 * n]);
      launch_bwd_b_splitk(jobs, s);
      break;
    }
  }
  OP_LAUNCHED(WHO);
}
#undef WHO
#undef SJ

int rsrgan_op_lstm_step_last_plan(int32_t out[16]) {
  OP_REFUSE(!out, "op_lstm_step_last_plan: null pointer");
  const StepPlanRecord& p = g_step_last_plan;
  const int v[10] = {p.form, p.threads, p.grid, p.map_valid, p.KG, p.kpg, p.grid2, p.lds, p.groups, p.tiled};
  for (int i = 0; i < 16; ++i) out[i] = i < 10 ? v[i] : 0;
  return RSRGAN_OK;
}

}  // extern "C"
