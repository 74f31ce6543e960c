// extern "C" boundary of libopadpo_hip.so (declared in include/opadpo_hip.h).
// Host-side validation only; every kernel launch is asynchronous on the caller's stream.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "kernels.h"
#include <dlfcn.h>

namespace {
thread_local char g_err[512] = "";

int fail(hipError_t e, const char* where) {
  snprintf(g_err, sizeof(g_err), "%s: %s (%d)", where, hipGetErrorString(e), (int)e);
  return (int)e;
}
int bad(const char* where, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s: %s", where, what);
  return (int)hipErrorInvalidValue;
}
inline int done(hipError_t e, const char* where) { return e == hipSuccess ? 0 : fail(e, where); }
inline hipStream_t S(void* s) { return (hipStream_t)s; }

KernelFlags g_flags;      // opadpo_set_flags

// opadpo_gemm_nt's validation and argument block
int gemm_nt_args(GemmNTArgs& a, const char* fn, const uint16_t* A1, int lda1, const uint16_t* B1, int ldb1, int K1,
                 const uint16_t* A2, int lda2, const uint16_t* B2, int ldb2, int K2, int a2_group_n, int a2_group_stride, int a1_group_n, int a1_group_stride,
                 void* C, int ldc, int out_f32, const void* R, int ldr, int res_f32, const uint16_t* bias, int M, int N, float alpha, int act) {
  if (M < 0 || N <= 0 || N % 128) return bad(fn, "N must be a positive multiple of 128");
  if (K1 < 0 || K2 < 0 || K1 % 64 || K2 % 64 || K1 + K2 == 0) return bad(fn, "K1/K2 must be multiples of 64");
  if ((K1 && (!A1 || !B1)) || (K2 && (!A2 || !B2)) || !C) return bad(fn, "null operand");
  if (lda1 % 8 || ldb1 % 8 || (K2 && (lda2 % 8 || ldb2 % 8)) || ldc % 4 || (R && ldr % 4))
    return bad(fn, "leading dimensions must keep 16-byte operand / 8-byte output alignment");
  if ((a2_group_n && a2_group_n % 128) || (a1_group_n && a1_group_n % 128))
    return bad(fn, "group widths must be multiples of the 128-column tile");
  a.A1 = A1; a.B1 = B1; a.A2 = A2; a.B2 = B2; a.C = C; a.R = R; a.bias = bias;
  a.M = M; a.N = N; a.K1 = K1; a.K2 = K2;
  a.lda1 = lda1; a.ldb1 = ldb1; a.lda2 = lda2; a.ldb2 = ldb2; a.ldc = ldc; a.ldr = ldr;
  a.a2_group_n = a2_group_n; a.a2_group_stride = a2_group_stride;
  a.a1_group_n = a1_group_n; a.a1_group_stride = a1_group_stride;
  a.alpha = alpha; a.act = act; a.out_f32 = out_f32; a.r_f32 = res_f32;
  return 0;
}

// The op-level entries have no context: the K-folded products (gemm_nt_workspace_bytes) take their partial sums from one library-owned
// buffer, used in stream order (grown on demand: a device-synchronising hipFree + hipMalloc, first steps only)
hipError_t gemm_nt_op(const GemmNTArgs& a, hipStream_t st) {
  static void* ws = nullptr;
  static size_t ws_bytes = 0;
  const size_t need = gemm_nt_workspace_bytes(a, g_flags);
  if (need > ws_bytes) {
    if (ws) (void)hipFree(ws);
    ws = nullptr; ws_bytes = 0;
    if (hipMalloc(&ws, need + need / 4) != hipSuccess) { (void)hipGetLastError(); return hipErrorOutOfMemory; }
    ws_bytes = need + need / 4;
  }
  return launch_gemm_nt(a, g_flags, st, ws, ws_bytes);
}
}  // namespace

KernelFlags kernel_flags(int gemm_variant, int use_tr) {
  KernelFlags f;
  f.variant = gemm_variant;
  f.use_tr = (use_tr & 1) != 0;
  f.attn_dma = (use_tr & 2) != 0;
  f.tn_w4 = (use_tr & 8) == 0;
  f.skinny8 = (use_tr & 16) == 0;
  f.dec64_variant = (use_tr >> 5) & 3;
  f.dec64x_nw = (use_tr >> 7) & 3;
  f.sample_compact = (use_tr & 512) == 0;
  f.w4s_few = (use_tr & 1024) != 0;
  f.w4_nodeep = (use_tr & 2048) != 0;
  f.w4_chunk_deal = (use_tr & 4096) != 0;
  return f;
}
const KernelFlags& process_flags() { return g_flags; }
KernelOverrides kernel_overrides(int gemm_variant, int use_tr) {
  KernelOverrides o;
  o.gemm_variant = gemm_variant;
  o.word = use_tr >= 0;
  o.use_tr = o.word && (use_tr & 1);
  o.tn_w4 = o.word && !(use_tr & 8);
  o.attn_rows16 = o.word && (use_tr & 256);
  return o;
}
KernelFlags resolve_flags(const KernelFlags& process, const KernelOverrides& o) {
  KernelFlags f = process;
  if (o.gemm_variant >= 0) f.variant = o.gemm_variant;
  if (o.word) { f.use_tr = o.use_tr; f.tn_w4 = o.tn_w4; f.attn_rows16 = o.attn_rows16; }
  return f;
}

// the same reporting for extern "C" entry points that live in other translation units (kernels.h)
int opadpo_report_bad(const char* where, const char* what) { return bad(where, what); }
int opadpo_report_done(hipError_t e, const char* where) { return done(e, where); }

extern "C" {

int opadpo_abi_version(void) { return OPADPO_ABI_VERSION; }
const char* opadpo_last_error(void) { return g_err; }
void opadpo_set_flags(int use_glds, int use_tr) { g_flags = kernel_flags(use_glds, use_tr); }

int opadpo_gemm_nt(const uint16_t* A1, int lda1, const uint16_t* B1, int ldb1, int K1,
                   const uint16_t* A2, int lda2, const uint16_t* B2, int ldb2, int K2,
                   int a2_group_n, int a2_group_stride, int a1_group_n, int a1_group_stride,
                   void* C, int ldc, int out_f32, const void* R, int ldr, int res_f32, const uint16_t* bias,
                   int M, int N, float alpha, int act, void* stream) {
  GemmNTArgs a;
  const int rc = gemm_nt_args(a, "opadpo_gemm_nt", A1, lda1, B1, ldb1, K1, A2, lda2, B2, ldb2, K2, a2_group_n, a2_group_stride, a1_group_n, a1_group_stride,
                              C, ldc, out_f32, R, ldr, res_f32, bias, M, N, alpha, act);
  return rc ? rc : done(gemm_nt_op(a, S(stream)), "opadpo_gemm_nt");
}

// test entry point (not in the public header): the launches opadpo_gemm_nt would make under opadpo_set_flags(gemm_variant, use_tr) on `cus` CUs,
// as text (one line per launch: kernel grid.x grid.y block LDS); nothing is launched.  rope: 1 the table form of opadpo_gemm_nt_rope, 2 the table-free
// form of opadpo_gemm_nt_rope_pos (both over all N columns; the operand pointers are never read)
int opadpo_debug_gemm_nt_plan(const uint16_t* A1, int lda1, const uint16_t* B1, int ldb1, int K1,
                              const uint16_t* A2, int lda2, const uint16_t* B2, int ldb2, int K2,
                              int a2_group_n, int a2_group_stride, int a1_group_n, int a1_group_stride,
                              void* C, int ldc, int out_f32, const void* R, int ldr, int res_f32, const uint16_t* bias,
                              int M, int N, float alpha, int act, int gemm_variant, int use_tr, int rope, int cus, char* out, int out_len) {
  GemmNTArgs a;
  const char* fn = "opadpo_debug_gemm_nt_plan";
  const int rc = gemm_nt_args(a, fn, A1, lda1, B1, ldb1, K1, A2, lda2, B2, ldb2, K2, a2_group_n, a2_group_stride, a1_group_n, a1_group_stride,
                              C, ldc, out_f32, R, ldr, res_f32, bias, M, N, alpha, act);
  if (rc) return rc;
  if (!out || out_len <= 0 || cus <= 0 || rope < 0 || rope > 2) return bad(fn, "output buffer, CU count or rope selector");
  static const float tab = 0.f;
  static const int32_t pos = 0;
  a.rope_cols = rope ? N : 0;
  if (rope == 1) { a.rope_cos = &tab; a.rope_sin = &tab; a.rope_L = 4096; }
  if (rope == 2) { a.rope_pos = &pos; a.rope_l2theta = log2f(10000.f); }
  return done(gemm_nt_plan_text(a, kernel_flags(gemm_variant, use_tr), cus, out, (size_t)out_len), fn);
}

int opadpo_gemm_nt_rope(const uint16_t* A1, int lda1, const uint16_t* B1, int ldb1, int K1,
                        const uint16_t* A2, int lda2, const uint16_t* B2, int ldb2, int K2, int a2_group_n, int a2_group_stride,
                        uint16_t* C, int ldc, int M, int N, const float* cos_tab, const float* sin_tab, int L, int rope_cols,
                        int seg_prefix, int seg_len, void* stream) {
  if (M < 0 || N <= 0 || N % 256) return bad("opadpo_gemm_nt_rope", "N must be a positive multiple of 256");
  if (K1 <= 0 || K2 < 0 || K1 % 64 || K2 % 64) return bad("opadpo_gemm_nt_rope", "K1/K2 must be multiples of 64");
  if (!A1 || !B1 || (K2 && (!A2 || !B2)) || !C || !cos_tab || !sin_tab) return bad("opadpo_gemm_nt_rope", "null operand");
  if (lda1 % 8 || ldb1 % 8 || (K2 && (lda2 % 8 || ldb2 % 8)) || ldc % 8) return bad("opadpo_gemm_nt_rope", "leading dimensions must keep 16-byte alignment");
  if (a2_group_n && a2_group_n % 256) return bad("opadpo_gemm_nt_rope", "group width must be a multiple of the 256-column tile");
  if (L < 4 || rope_cols < 0 || rope_cols > N || rope_cols % 128 || seg_prefix < 0 || seg_len < 0 || (seg_len > 0 && seg_len < 4))
    return bad("opadpo_gemm_nt_rope", "rope_cols must be whole heads of 128 within N; L >= 4; seg_len 0 or >= 4");
  GemmNTArgs a;
  a.A1 = A1; a.B1 = B1; a.A2 = A2; a.B2 = B2; a.C = C; a.R = nullptr; a.bias = nullptr;
  a.M = M; a.N = N; a.K1 = K1; a.K2 = K2;
  a.lda1 = lda1; a.ldb1 = ldb1; a.lda2 = lda2; a.ldb2 = ldb2; a.ldc = ldc; a.ldr = 0;
  a.a2_group_n = a2_group_n; a.a2_group_stride = a2_group_stride; a.a1_group_n = 0; a.a1_group_stride = 0;
  a.alpha = 1.0f; a.act = 0; a.out_f32 = 0; a.r_f32 = 0;
  a.rope_cos = cos_tab; a.rope_sin = sin_tab; a.rope_L = L; a.rope_cols = rope_cols; a.rope_seg_prefix = seg_prefix; a.rope_seg_len = seg_len;
  return done(gemm_nt_op(a, S(stream)), "opadpo_gemm_nt_rope");
}

int opadpo_gemm_nt_rope_pos(const uint16_t* A1, int lda1, const uint16_t* B1, int ldb1, int K1,
                            const uint16_t* A2, int lda2, const uint16_t* B2, int ldb2, int K2, int a2_group_n, int a2_group_stride,
                            uint16_t* C, int ldc, int M, int N, const int32_t* row_pos, float theta, int rope_cols, void* stream) {
  if (M < 0 || N <= 0 || N % 256) return bad("opadpo_gemm_nt_rope_pos", "N must be a positive multiple of 256");
  if (K1 <= 0 || K2 < 0 || K1 % 64 || K2 % 64) return bad("opadpo_gemm_nt_rope_pos", "K1/K2 must be multiples of 64");
  if (!A1 || !B1 || (K2 && (!A2 || !B2)) || !C || !row_pos) return bad("opadpo_gemm_nt_rope_pos", "null operand");
  if (lda1 % 8 || ldb1 % 8 || (K2 && (lda2 % 8 || ldb2 % 8)) || ldc % 8) return bad("opadpo_gemm_nt_rope_pos", "leading dimensions must keep 16-byte alignment");
  if (a2_group_n && a2_group_n % 256) return bad("opadpo_gemm_nt_rope_pos", "group width must be a multiple of the 256-column tile");
  if (rope_cols < 0 || rope_cols > N || rope_cols % 128 || !(theta > 1.0f)) return bad("opadpo_gemm_nt_rope_pos", "rope_cols must be whole heads of 128 within N; theta > 1");
  GemmNTArgs a;
  a.A1 = A1; a.B1 = B1; a.A2 = A2; a.B2 = B2; a.C = C; a.R = nullptr; a.bias = nullptr;
  a.M = M; a.N = N; a.K1 = K1; a.K2 = K2;
  a.lda1 = lda1; a.ldb1 = ldb1; a.lda2 = lda2; a.ldb2 = ldb2; a.ldc = ldc; a.ldr = 0;
  a.a2_group_n = a2_group_n; a.a2_group_stride = a2_group_stride; a.a1_group_n = 0; a.a1_group_stride = 0;
  a.alpha = 1.0f; a.act = 0; a.out_f32 = 0; a.r_f32 = 0;
  a.rope_pos = row_pos; a.rope_l2theta = log2f(theta); a.rope_cols = rope_cols;
  return done(gemm_nt_op(a, S(stream)), "opadpo_gemm_nt_rope_pos");
}

int opadpo_gemm_nt_decode(const uint16_t* A, int lda, const uint16_t* B, int ldb, int K, void* C, int ldc, int mode, int M, int N, int splits,
                          void* stream) {
  if (M < 0 || M > 64) return bad("opadpo_gemm_nt_decode", "M must be 0..64 (one token per sequence)");
  if (N <= 0 || N % 128 || K <= 0 || K % 64) return bad("opadpo_gemm_nt_decode", "N must be a multiple of 128, K of 64");
  if (!A || !B || !C || lda % 8 || ldb % 8 || ldc % 4 || mode < 0 || mode > 2) return bad("opadpo_gemm_nt_decode", "null operand, misaligned leading dimension or bad mode");
  GemmNTArgs a;
  a.A1 = A; a.B1 = B; a.A2 = nullptr; a.B2 = nullptr; a.C = C; a.R = nullptr; a.bias = nullptr;
  a.M = M; a.N = N; a.K1 = K; a.K2 = 0; a.lda1 = lda; a.ldb1 = ldb; a.lda2 = 0; a.ldb2 = 0; a.ldc = ldc; a.ldr = 0;
  a.a2_group_n = 0; a.a2_group_stride = 0; a.a1_group_n = 0; a.a1_group_stride = 0; a.alpha = 1.f; a.act = 0; a.out_f32 = mode == 1; a.r_f32 = 0;
  return done(launch_gemm_nt_dec64(a, mode, splits, g_flags, S(stream)), "opadpo_gemm_nt_decode");
}
// shared by the two decode entry points: the checks after the M range, then the argument block
static int decode_gemm_args(GemmNTArgs& a, const char* fn, const uint16_t* A, int lda, const uint16_t* B, int ldb, int K, void* C, int ldc, int mode, int M, int N) {
  if (N <= 0 || N % 128 || K <= 0 || K % 64) return bad(fn, "N must be a multiple of 128, K of 64");
  if (!A || !B || !C || lda % 8 || ldb % 8 || ldc % 4 || mode < 0 || mode > 2) return bad(fn, "null operand, misaligned leading dimension or bad mode");
  a.A1 = A; a.B1 = B; a.A2 = nullptr; a.B2 = nullptr; a.C = C; a.R = nullptr; a.bias = nullptr;
  a.M = M; a.N = N; a.K1 = K; a.K2 = 0; a.lda1 = lda; a.ldb1 = ldb; a.lda2 = 0; a.ldb2 = 0; a.ldc = ldc; a.ldr = 0;
  a.a2_group_n = 0; a.a2_group_stride = 0; a.a1_group_n = 0; a.a1_group_stride = 0; a.alpha = 1.f; a.act = 0; a.out_f32 = mode == 1; a.r_f32 = 0;
  return 0;
}
int opadpo_gemm_nt_decode_wide(const uint16_t* A, int lda, const uint16_t* B, int ldb, int K, void* C, int ldc, int mode, int M, int N, int splits,
                               void* stream) {
  const char* fn = "opadpo_gemm_nt_decode_wide";
  if (M < 65 || M > 256) return bad(fn, "M must be 65..256 (opadpo_gemm_nt_decode takes 0..64)");
  GemmNTArgs a;
  const int rc = decode_gemm_args(a, fn, A, lda, B, ldb, K, C, ldc, mode, M, N);
  return rc ? rc : done(launch_gemm_nt_decw(a, mode, splits, g_flags, S(stream)), fn);
}
// test entry point (not in the public header): the launch opadpo_gemm_nt_decode (M <= 64) / opadpo_gemm_nt_decode_wide (M >= 65) would make under
// process word use_tr, as one `kernel grid.x grid.y block LDS` line; the same validation, nothing is launched, the operand pointers are never read
int opadpo_debug_gemm_nt_decode_plan(int M, int N, int K, int mode, int splits, int use_tr, char* out, int out_len) {
  const char* fn = "opadpo_debug_gemm_nt_decode_plan";
  if (M < 1 || M > 256) return bad(fn, "M must be 1..256");
  if (!out || out_len <= 0) return bad(fn, "output buffer");
  GemmNTArgs a;
  static const uint16_t dummy[8] = {};
  const int rc = decode_gemm_args(a, fn, dummy, K, dummy, K, K, (void*)dummy, mode == 2 ? N / 2 : N, mode, M, N);
  return rc ? rc : done(gemm_nt_decode_plan_text(a, mode, splits, kernel_flags(10, use_tr), out, (size_t)out_len), fn);
}
int opadpo_gemm_nt_decode_splits(int N, int K, int splits) { return (N > 0 && K >= 64) ? gemm_nt_dec64_splits(N, K, splits, g_flags) : 1; }
int opadpo_rmsnorm_sum_fwd(const void* resid, int resid_f32, const float* partials, int n_partials, size_t partial_stride, const uint16_t* w,
                           float* x_out, uint16_t* y, float* rstd, int rows, int H, float eps, void* stream) {
  if (!resid || !w || !x_out) return bad("opadpo_rmsnorm_sum_fwd", "null operand");
  return done(launch_rmsnorm_sum_fwd(resid, resid_f32, partials, n_partials, partial_stride, w, x_out, y, rstd, rows, H, eps, S(stream)),
              "opadpo_rmsnorm_sum_fwd");
}
int opadpo_gemm_tn(const uint16_t* P, int ldp, const uint16_t* Q, int ldq, float* C, int ldc,
                   int M, int N1, int N2, int q_group_n1, int q_group_stride, float alpha, int splits,
                   void* stream) {
  if (N1 <= 0 || N2 <= 0 || N1 % 128 || N2 % 128) return bad("opadpo_gemm_tn", "N1/N2 must be positive multiples of 128");
  if (!P || !Q || !C || ldp % 8 || ldq % 8) return bad("opadpo_gemm_tn", "null operand or misaligned leading dimension");
  if (q_group_n1 && q_group_n1 % 128) return bad("opadpo_gemm_tn", "q_group_n1 must be a multiple of 128");
  GemmTNArgs a;
  a.P = P; a.Q = Q; a.C = C; a.M = M; a.N1 = N1; a.N2 = N2; a.ldp = ldp; a.ldq = ldq; a.ldc = ldc;
  a.q_group_n1 = q_group_n1; a.q_group_stride = q_group_stride; a.alpha = alpha; a.splits = splits;
  return done(launch_gemm_tn(a, g_flags, S(stream)), "opadpo_gemm_tn");
}

int opadpo_gemm_tn_group(int n, const uint16_t* const* P, const int* ldp, const uint16_t* const* Q, const int* ldq, float* const* C, const int* ldc,
                         int M, const int* N1, const int* N2, const int* q_group_n1, const int* q_group_stride, float alpha, void* stream) {
  if (n < 0 || n > 8 || (n && (!P || !ldp || !Q || !ldq || !C || !ldc || !N1 || !N2))) return bad("opadpo_gemm_tn_group", "0..8 problems, non-null arrays");
  GemmTNArgs list[8];
  for (int i = 0; i < n; ++i) {
    if (N1[i] <= 0 || N2[i] <= 0 || N1[i] % 128 || N2[i] % 128) return bad("opadpo_gemm_tn_group", "N1/N2 must be positive multiples of 128");
    if (!P[i] || !Q[i] || !C[i] || ldp[i] % 8 || ldq[i] % 8) return bad("opadpo_gemm_tn_group", "null operand or misaligned leading dimension");
    GemmTNArgs& a = list[i];
    a.P = P[i]; a.Q = Q[i]; a.C = C[i]; a.M = M; a.N1 = N1[i]; a.N2 = N2[i]; a.ldp = ldp[i]; a.ldq = ldq[i]; a.ldc = ldc[i];
    a.q_group_n1 = q_group_n1 ? q_group_n1[i] : 0; a.q_group_stride = q_group_stride ? q_group_stride[i] : 0; a.alpha = alpha; a.splits = 0;
    if (a.q_group_n1 && a.q_group_n1 % 128) return bad("opadpo_gemm_tn_group", "q_group_n1 must be a multiple of 128");
  }
  return done(launch_gemm_tn_group(list, n, g_flags, S(stream)), "opadpo_gemm_tn_group");
}

static int tn_group_list(const char* fn, GemmTNArgs* list, int n, const uint16_t* const* P, const int* ldp, const uint16_t* const* Q, const int* ldq, float* const* C,
                         const int* ldc, int M, const int* N1, const int* N2, const int* q_group_n1, const int* q_group_stride, float alpha, bool shapes_only) {
  if (n < 0 || n > 8 || (n && (!N1 || !N2 || (!shapes_only && (!P || !ldp || !Q || !ldq || !C || !ldc))))) return bad(fn, "0..8 problems, non-null arrays");
  for (int i = 0; i < n; ++i) {
    if (N1[i] <= 0 || N2[i] <= 0 || N1[i] % 128 || N2[i] % 128) return bad(fn, "N1/N2 must be positive multiples of 128");
    GemmTNArgs& a = list[i];
    a.M = M; a.N1 = N1[i]; a.N2 = N2[i];
    a.q_group_n1 = q_group_n1 ? q_group_n1[i] : 0; a.q_group_stride = q_group_stride ? q_group_stride[i] : 0; a.alpha = alpha; a.splits = 0;
    if (a.q_group_n1 && a.q_group_n1 % 128) return bad(fn, "q_group_n1 must be a multiple of 128");
    if (shapes_only) { a.P = a.Q = nullptr; a.C = nullptr; a.ldp = N1[i]; a.ldq = N2[i] * (a.q_group_n1 ? N1[i] / a.q_group_n1 : 1); a.ldc = N2[i]; continue; }
    if (!P[i] || !Q[i] || !C[i] || ldp[i] % 8 || ldq[i] % 8) return bad(fn, "null operand or misaligned leading dimension");
    a.P = P[i]; a.Q = Q[i]; a.C = C[i]; a.ldp = ldp[i]; a.ldq = ldq[i]; a.ldc = ldc[i];
  }
  return 0;
}

size_t opadpo_gemm_tn_group_workspace_bytes(int n, int M, const int* N1, const int* N2, const int* q_group_n1) {
  GemmTNArgs list[8];
  if (M <= 0 || tn_group_list("opadpo_gemm_tn_group_workspace_bytes", list, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, M, N1, N2, q_group_n1, nullptr, 1.f, true)) return 0;
  return gemm_tn_group_workspace_bytes(list, n, g_flags);
}

int opadpo_gemm_tn_group_det(int n, const uint16_t* const* P, const int* ldp, const uint16_t* const* Q, const int* ldq, float* const* C, const int* ldc,
                             int M, const int* N1, const int* N2, const int* q_group_n1, const int* q_group_stride, float alpha,
                             void* workspace, size_t workspace_bytes, void* stream) {
  GemmTNArgs list[8];
  if (const int rc = tn_group_list("opadpo_gemm_tn_group_det", list, n, P, ldp, Q, ldq, C, ldc, M, N1, N2, q_group_n1, q_group_stride, alpha, false)) return rc;
  const size_t need = gemm_tn_group_workspace_bytes(list, n, g_flags);
  if (need == 0) return bad("opadpo_gemm_tn_group_det", "these problems do not run on the 256x256 kernel (N1, N2, q_group_n1 % 256): no deterministic form");
  if (!workspace || workspace_bytes < need) return bad("opadpo_gemm_tn_group_det", "workspace smaller than opadpo_gemm_tn_group_workspace_bytes");
  return done(launch_gemm_tn_group(list, n, g_flags, S(stream), workspace, workspace_bytes), "opadpo_gemm_tn_group_det");
}

int opadpo_attn_fwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, int ld, uint16_t* o, int ldo,
                    float* lse, const uint8_t* key_mask, int S_, int L, int nh, int hd, int causal, float scale,
                    int seg_prefix, int seg_len, void* stream) {
  if (hd != 64 && hd != 128) return bad("opadpo_attn_fwd", "head_dim must be 64 or 128");
  // head_dim 128 runs the 32-rows-per-wave kernel, which writes O (also the zeros of an all-padding tile) as 16-byte pieces: ldo % 8
  if (!q || !k || !v || !o || ld % 8 || ldo % (hd == 128 ? 8 : 4)) return bad("opadpo_attn_fwd", "null operand or misaligned leading dimension (ld % 8, ldo % 8 at head_dim 128, ldo % 4 at 64)");
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.k = k; a.v = v; a.o = o; a.lse = lse; a.key_mask = key_mask;
  a.S = S_; a.L = L; a.nh = nh; a.hd = hd; a.ld = ld; a.ldo = ldo; a.causal = causal; a.scale = scale;
  if (seg_len < 0 || seg_prefix < 0 || (seg_len > 0 && !causal)) return bad("opadpo_attn_fwd", "packed responses need causal attention and seg_prefix, seg_len >= 0");
  a.seg_prefix = seg_prefix; a.seg_len = seg_len;
  return done(launch_attn_fwd(a, g_flags, S(stream)), "opadpo_attn_fwd");
}

int opadpo_attn_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, int ld, const uint16_t* o,
                    const uint16_t* dout, int ldo, const float* lse, const uint8_t* key_mask,
                    uint16_t* dq, uint16_t* dk, uint16_t* dv, float* dq_f32, float* delta,
                    int S_, int L, int nh, int hd, int causal, float scale, int seg_prefix, int seg_len, void* stream) {
  if (hd != 64 && hd != 128) return bad("opadpo_attn_bwd", "head_dim must be 64 or 128");
  if (seg_len < 0 || seg_prefix < 0 || (seg_len > 0 && !causal)) return bad("opadpo_attn_bwd", "packed responses need causal attention and seg_prefix, seg_len >= 0");
  if (!q || !k || !v || !o || !dout || !lse || (!dq && !dq_f32) || !dk || !dv || !delta || ld % 8 || ldo % 8)
    return bad("opadpo_attn_bwd", "null operand or misaligned leading dimension");
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.k = k; a.v = v; a.o = (uint16_t*)o; a.lse = (float*)lse; a.key_mask = key_mask;
  a.S = S_; a.L = L; a.nh = nh; a.hd = hd; a.ld = ld; a.ldo = ldo; a.causal = causal; a.scale = scale;
  a.dout = dout; a.dq_acc = dq_f32; a.dq = dq; a.dk = dk; a.dv = dv; a.delta = delta;
  a.seg_prefix = seg_prefix; a.seg_len = seg_len;
  return done(launch_attn_bwd(a, g_flags, S(stream)), "opadpo_attn_bwd");
}

int opadpo_rmsnorm_fwd(const void* x, int x_f32, const uint16_t* w, uint16_t* y, float* rstd, int rows, int H, float eps, void* stream) {
  return done(launch_rmsnorm_fwd(x, x_f32, w, y, rstd, rows, H, eps, S(stream)), "opadpo_rmsnorm_fwd");
}
int opadpo_rmsnorm_bwd(const uint16_t* dy, const void* x, int x_f32, const uint16_t* w, const float* rstd,
                       const void* dres, int dres_f32, float* dx_f32, uint16_t* dx_bf16, int rows, int H, void* stream) {
  if (!dx_f32 && !dx_bf16) return bad("opadpo_rmsnorm_bwd", "no output buffer");
  return done(launch_rmsnorm_bwd(dy, x, x_f32, w, rstd, dres, dres_f32, dx_f32, dx_bf16, rows, H, S(stream)), "opadpo_rmsnorm_bwd");
}
int opadpo_layernorm_fwd(const uint16_t* x, const uint16_t* w, const uint16_t* b, uint16_t* y, int rows, int H, float eps, void* stream) {
  return done(launch_layernorm_fwd(x, w, b, y, rows, H, eps, S(stream)), "opadpo_layernorm_fwd");
}
int opadpo_layernorm_fwd_f32(const float* x, const uint16_t* w, const uint16_t* b, void* y, int y_f32, int rows, int H, float eps, void* stream) {
  if (!x || !w || !b || !y) return bad("opadpo_layernorm_fwd_f32", "null operand");
  return done(launch_layernorm_fwd(x, w, b, y, rows, H, eps, S(stream), 1, y_f32 ? 1 : 0), "opadpo_layernorm_fwd_f32");
}
int opadpo_layernorm_bwd(const uint16_t* dy, const uint16_t* x, const uint16_t* w, const uint16_t* dres, uint16_t* dx, int rows, int H,
                         float eps, void* stream) {
  return done(launch_layernorm_bwd(dy, x, w, dres, dx, rows, H, eps, S(stream)), "opadpo_layernorm_bwd");
}
int opadpo_act_fwd(const uint16_t* z, uint16_t* out, size_t n, int act, void* stream) {
  return done(launch_act_fwd(z, out, n, act, S(stream)), "opadpo_act_fwd");
}
int opadpo_act_bwd(const uint16_t* dout, const uint16_t* z, uint16_t* dz, size_t n, int act, void* stream) {
  return done(launch_act_bwd(dout, z, dz, n, act, S(stream)), "opadpo_act_bwd");
}
int opadpo_rope(uint16_t* qk, int ld, const float* cos_tab, const float* sin_tab, int rows, int L, int n_heads, int hd,
                int inverse, const int32_t* pos_base, int seg_prefix, int seg_len, void* stream) {
  if (ld % 8) return bad("opadpo_rope", "misaligned leading dimension");
  return done(launch_rope(qk, ld, cos_tab, sin_tab, rows, L, n_heads, hd, inverse, pos_base, seg_prefix, seg_len, S(stream)), "opadpo_rope");
}
int opadpo_silu_mul_fwd(const uint16_t* gu, uint16_t* act, int rows, int F, void* stream) {
  return done(launch_silu_mul_fwd(gu, act, rows, F, S(stream)), "opadpo_silu_mul_fwd");
}
int opadpo_silu_mul_bwd(const uint16_t* dact, const uint16_t* gu, uint16_t* dgu, int rows, int F, void* stream) {
  return done(launch_silu_mul_bwd(dact, gu, dgu, rows, F, S(stream)), "opadpo_silu_mul_bwd");
}
int opadpo_lora_dropout_fwd(const uint16_t* x, uint16_t* out, int rows, int K, int g, double p, uint64_t seed, uint64_t call, int layer, int module0,
                            const int32_t* row_idx, void* stream) {
  LoraDropout dp;
  if (lora_dropout_make(p, seed, call, &dp)) return bad("opadpo_lora_dropout_fwd", "need 0 <= p < 1 and seed < 2^32");
  if (!x || !out || rows < 0 || K <= 0 || K % 8) return bad("opadpo_lora_dropout_fwd", "null operand, or K not a positive multiple of 8");
  if (g < 1 || module0 < 0 || module0 + g > 7 || layer < 0) return bad("opadpo_lora_dropout_fwd", "modules outside 0..6 or negative layer");
  return done(launch_lora_dropout_fwd(x, out, rows, K, g, dp, layer, module0, row_idx, S(stream)), "opadpo_lora_dropout_fwd");
}
int opadpo_lora_dropout_bwd_add(uint16_t* dx, const uint16_t* u, int rows, int K, int g, double p, uint64_t seed, uint64_t call, int layer, int module0,
                                const int32_t* row_idx, void* stream) {
  LoraDropout dp;
  if (lora_dropout_make(p, seed, call, &dp)) return bad("opadpo_lora_dropout_bwd_add", "need 0 <= p < 1 and seed < 2^32");
  if (!dx || !u || rows < 0 || K <= 0 || K % 8) return bad("opadpo_lora_dropout_bwd_add", "null operand, or K not a positive multiple of 8");
  if (g < 1 || module0 < 0 || module0 + g > 7 || layer < 0) return bad("opadpo_lora_dropout_bwd_add", "modules outside 0..6 or negative layer");
  return done(launch_lora_dropout_bwd_add(dx, u, rows, K, g, dp, layer, module0, row_idx, S(stream)), "opadpo_lora_dropout_bwd_add");
}
int opadpo_embed_splice(const int32_t* ids, const uint8_t* text_mask, const uint16_t* embed, const uint16_t* feats,
                        const int32_t* feat_row, const uint8_t* image_mask, void* x, int x_f32, uint8_t* key_mask,
                        int S_, int n_txt, int P, int H, int image_token, void* stream) {
  if (!ids || !text_mask || !embed || !feats || !feat_row || !x || !key_mask) return bad("opadpo_embed_splice", "null operand");
  return done(launch_embed_splice(ids, text_mask, embed, feats, feat_row, image_mask, x, x_f32, key_mask, S_, n_txt, P, H,
                                  image_token, S(stream)), "opadpo_embed_splice");
}
int opadpo_im2col(const uint16_t* pixels, uint16_t* out, int B, int image_size, int patch, int kpad, void* stream) {
  if (image_size % patch || kpad < 3 * patch * patch) return bad("opadpo_im2col", "bad geometry");
  return done(launch_im2col(pixels, out, B, image_size, patch, kpad, S(stream)), "opadpo_im2col");
}
int opadpo_vision_embed(const uint16_t* patches, const uint16_t* cls, const uint16_t* pos, uint16_t* x, int B, int P, int h, void* stream) {
  return done(launch_vision_embed(patches, cls, pos, x, B, P, h, S(stream)), "opadpo_vision_embed");
}
int opadpo_vision_embed_f32(const uint16_t* patches, const uint16_t* cls, const uint16_t* pos, float* x, int B, int P, int h, void* stream) {
  return done(launch_vision_embed(patches, cls, pos, x, B, P, h, S(stream), 1), "opadpo_vision_embed_f32");
}
int opadpo_gather_rows(const uint16_t* src, int ld_src, const int32_t* rows_idx, uint16_t* dst, int n, int H, void* stream) {
  if (ld_src % 8) return bad("opadpo_gather_rows", "misaligned leading dimension");
  return done(launch_gather_rows(src, ld_src, rows_idx, dst, n, H, S(stream)), "opadpo_gather_rows");
}
int opadpo_scatter_rows(const uint16_t* src, const int32_t* rows_idx, uint16_t* dst, int ld_dst, int n, int H, void* stream) {
  if (ld_dst % 8) return bad("opadpo_scatter_rows", "misaligned leading dimension");
  return done(launch_scatter_rows(src, rows_idx, dst, ld_dst, n, H, S(stream)), "opadpo_scatter_rows");
}
int opadpo_scatter_add_rows_f32(const float* src, const int32_t* rows_idx, float* dst, int ld_dst, int n, int H, void* stream) {
  return done(launch_scatter_add_rows_f32(src, rows_idx, dst, ld_dst, n, H, S(stream)), "opadpo_scatter_add_rows_f32");
}
int opadpo_transpose(const uint16_t* in, uint16_t* out, int R, int C, void* stream) {
  return done(launch_transpose(in, out, R, C, S(stream)), "opadpo_transpose");
}
int opadpo_transpose_batched(const uint16_t* src, uint16_t* dst, const int64_t* jobs, int n_jobs, int max_tiles, void* stream) {
  if (n_jobs > 0 && (!src || !dst || !jobs)) return bad("opadpo_transpose_batched", "null operand");
  return done(launch_transpose_batched(src, dst, (const long long*)jobs, n_jobs, max_tiles, S(stream)), "opadpo_transpose_batched");
}
int opadpo_f32_to_bf16(const float* in, uint16_t* out, size_t n, void* stream) {
  return done(launch_f32_to_bf16(in, out, n, S(stream)), "opadpo_f32_to_bf16");
}
int opadpo_bf16_to_f32(const uint16_t* in, float* out, size_t n, void* stream) {
  if (n && ((uintptr_t)in % 16 || (uintptr_t)out % 16)) return bad("opadpo_bf16_to_f32", "buffers must be 16-byte aligned");
  return done(launch_bf16_to_f32(in, out, n, S(stream)), "opadpo_bf16_to_f32");
}
int opadpo_f32_to_bf16_strided(const float* in, uint16_t* out, size_t rows, int C, int ld, void* stream) {
  if (ld % 4) return bad("opadpo_f32_to_bf16_strided", "misaligned leading dimension");
  return done(launch_f32_to_bf16_strided(in, out, rows, C, ld, S(stream)), "opadpo_f32_to_bf16_strided");
}
int opadpo_head_fwd(const float* logits, int ldl, const int32_t* labels, float inv_temp, float* logp, float* ent,
                    float* lse, int rows, int V, void* stream) {
  if (!logits || !labels || !logp || !ent || !lse) return bad("opadpo_head_fwd", "null operand");
  return done(launch_head_fwd(logits, ldl, labels, inv_temp, logp, ent, lse, rows, V, S(stream)), "opadpo_head_fwd");
}
int opadpo_head_bwd(const float* logits, int ldl, const int32_t* labels, const float* lse, const float* dlogp,
                    const float* ent, const float* dent, float inv_temp, uint16_t* dz, int ldz, int rows, int V, void* stream) {
  if (!logits || !labels || !lse || !dlogp || !dz || (dent && !ent)) return bad("opadpo_head_bwd", "null operand");
  return done(launch_head_bwd(logits, ldl, labels, lse, dlogp, ent, dent, inv_temp, dz, ldz, rows, V, S(stream)), "opadpo_head_bwd");
}
int opadpo_sumsq(const float* g, size_t n, float* out, void* stream) {
  return done(launch_sumsq(g, n, out, S(stream)), "opadpo_sumsq");
}
int opadpo_adamw(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, size_t n, double lr, double beta1,
                 double beta2, double eps, double weight_decay, int step, const float* sumsq, double max_norm,
                 double grad_div, void* stream) {
  if (step < 1) return bad("opadpo_adamw", "step is 1-based");
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  return done(launch_adamw(p, g, m, v, p_bf16, n, (float)lr, (float)beta1, (float)beta2, (float)eps, (float)weight_decay,
                           (float)bc1, (float)sqrt(bc2), sumsq, (float)max_norm, (float)grad_div, S(stream)), "opadpo_adamw");
}
int opadpo_attn_decode(const uint16_t* q, int ldq, const uint16_t* k_cache, const uint16_t* v_cache, uint16_t* o,
                       const uint8_t* key_mask, int B, int nh, int hd, int ctx, const int32_t* ctx_ptr, int max_ctx,
                       float scale, void* workspace, size_t workspace_bytes, void* stream) {
  if (ctx > max_ctx) return bad("opadpo_attn_decode", "ctx > max_ctx");
  if (ldq % 8) return bad("opadpo_attn_decode", "misaligned leading dimension");
  return done(launch_attn_decode(q, k_cache, v_cache, o, key_mask, B, nh, hd, ctx, ctx_ptr, max_ctx, ldq, scale, workspace,
                                 workspace_bytes, S(stream)),
              "opadpo_attn_decode");
}
size_t opadpo_attn_decode_workspace_bytes(int B, int nh, int hd, int max_ctx) {
  return (B > 0 && nh > 0) ? attn_decode_workspace_bytes(B, nh, hd, max_ctx) : 0;
}
int opadpo_attn_decode_fused(const uint16_t* qkv, int ld, const float* cos_tab, const float* sin_tab, uint16_t* k_cache, uint16_t* v_cache,
                             uint16_t* o, const uint8_t* key_mask, int B, int nh, int hd, const int32_t* pos_ptr, int max_ctx, float scale,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (!pos_ptr) return bad("opadpo_attn_decode_fused", "pos_ptr is required");
  if (ld % 8 || ld < 3 * nh * hd) return bad("opadpo_attn_decode_fused", "qkv rows must hold [q|k|v] with an aligned leading dimension");
  return done(launch_attn_decode_fused(qkv, ld, cos_tab, sin_tab, k_cache, v_cache, o, key_mask, B, nh, hd, pos_ptr, max_ctx, scale,
                                       workspace, workspace_bytes, S(stream)),
              "opadpo_attn_decode_fused");
}
int opadpo_attn_decode_fused_rows(const uint16_t* qkv, int ld, const float* cos_tab, const float* sin_tab, uint16_t* k_cache, uint16_t* v_cache,
                                  uint16_t* o, const uint8_t* key_mask, int B, int nh, int hd, const int32_t* pos_rows, int max_ctx, float scale,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "opadpo_attn_decode_fused_rows";
  if (!qkv || !cos_tab || !sin_tab || !k_cache || !v_cache || !o || !pos_rows) return bad(fn, "null operand (pos_rows [B] is required)");
  if (B <= 0 || nh <= 0 || max_ctx < 1) return bad(fn, "bad shape: need B >= 1, nh >= 1, max_ctx >= 1");
  if (hd != 64 && hd != 128) return bad(fn, "head_dim must be 64 or 128");
  if (ld % 8 || ld < 3 * nh * hd) return bad(fn, "qkv rows must hold [q|k|v] with an aligned leading dimension");
  return done(launch_attn_decode_fused_rows(qkv, ld, cos_tab, sin_tab, k_cache, v_cache, o, key_mask, B, nh, hd, pos_rows, max_ctx, scale, workspace,
                                            workspace_bytes, S(stream)),
              fn);
}
int opadpo_attn_decode_beam(const uint16_t* qkv, int ld, const float* cos_tab, const float* sin_tab, const uint16_t* k_prefix,
                            const uint16_t* v_prefix, uint16_t* k_suffix, uint16_t* v_suffix, uint16_t* o, const uint8_t* prefix_mask, int B, int k,
                            int nh, int hd, const int32_t* pos_ptr, int Lp, int max_new, const int32_t* table, float scale, void* workspace,
                            size_t workspace_bytes, void* stream) {
  const char* fn = "opadpo_attn_decode_beam";
  if (!qkv || !cos_tab || !sin_tab || !k_prefix || !v_prefix || !k_suffix || !v_suffix || !o || !pos_ptr || !table) return bad(fn, "null operand");
  if (B <= 0 || k <= 0 || k > OPADPO_MAX_BEAMS || Lp <= 0 || max_new <= 0) return bad(fn, "bad shape");
  if (ld % 8 || ld < 3 * nh * hd) return bad(fn, "qkv rows must hold [q|k|v] with an aligned leading dimension");
  return done(launch_attn_decode_beam(qkv, ld, cos_tab, sin_tab, k_prefix, v_prefix, k_suffix, v_suffix, o, prefix_mask, B, k, nh, hd, pos_ptr, Lp,
                                      max_new, table, 0, scale, workspace, workspace_bytes, S(stream)),
              fn);
}
size_t opadpo_attn_decode_shared_workspace_bytes(int items, int n, int nh, int hd, int Lp, int max_new) {
  return attn_decode_shared_workspace_bytes(items, n, nh, hd, Lp, max_new);
}
int opadpo_attn_decode_shared(const uint16_t* qkv, int ld, const float* cos_tab, const float* sin_tab, const uint16_t* k_prefix,
                              const uint16_t* v_prefix, uint16_t* k_suffix, uint16_t* v_suffix, uint16_t* o, const uint8_t* prefix_mask, int items,
                              int n, int nh, int hd, const int32_t* pos_ptr, int Lp, int max_new, float scale, void* workspace,
                              size_t workspace_bytes, int form, void* stream) {
  const char* fn = "opadpo_attn_decode_shared";
  if (!qkv || !cos_tab || !sin_tab || !k_prefix || !v_prefix || !k_suffix || !v_suffix || !o || !pos_ptr) return bad(fn, "null operand");
  if (n < 1 || n > OPADPO_MAX_RETURN_SEQUENCES) return bad(fn, "num_return_sequences must be in 1..OPADPO_MAX_RETURN_SEQUENCES (16)");
  if (items <= 0 || nh <= 0 || Lp <= 0 || max_new <= 0) return bad(fn, "bad shape");
  if (hd != 64 && hd != 128) return bad(fn, "head_dim must be 64 or 128");
  if (form < 0 || form > 2) return bad(fn, "form must be 0 (the library's choice), 1 (per-row) or 2 (grouped)");
  if (form == 2 && hd != 128) return bad(fn, "the grouped form (2) needs head_dim 128");
  if (ld % 8 || ld < 3 * nh * hd) return bad(fn, "qkv rows must hold [q|k|v] with an aligned leading dimension");
  const size_t need = attn_decode_shared_workspace_bytes(items, n, nh, hd, Lp, max_new);
  if (need && (!workspace || workspace_bytes < need)) return bad(fn, "workspace smaller than opadpo_attn_decode_shared_workspace_bytes");
  return done(launch_attn_decode_shared(qkv, ld, cos_tab, sin_tab, k_prefix, v_prefix, k_suffix, v_suffix, o, prefix_mask, items, n, nh, hd, pos_ptr,
                                        Lp, max_new, scale, workspace, workspace_bytes, form, S(stream)),
              fn);
}
int opadpo_beam_step(const float* logits, int ldl, int B, int k, int V, int step, int max_new, int eos_id, int pad_id, float* run_score,
                     float* cand_val, int32_t* cand_tok, float* fin_score, int32_t* fin_info, int32_t* fin_n, uint8_t* done_, int32_t* cur_tok,
                     int32_t* bp, int32_t* table, void* stream) {
  const char* fn = "opadpo_beam_step";
  if (!logits || !run_score || !cand_val || !cand_tok || !fin_score || !fin_info || !fin_n || !done_ || !cur_tok || !bp || !table) return bad(fn, "null operand");
  if (B <= 0 || k <= 0 || k > OPADPO_MAX_BEAMS) return bad(fn, "num_beams must be in 1..OPADPO_MAX_BEAMS");
  if (B * k > 64) return bad(fn, "B * num_beams above 64 rows");
  if (V < 2 * k || V > 32768 || ldl < V) return bad(fn, "vocabulary must hold 2 * num_beams .. 32768 tokens");
  if (step < 0 || step >= max_new) return bad(fn, "step out of range");
  const BeamState s{run_score, cand_val, cand_tok, fin_score, fin_info, fin_n, done_, cur_tok, bp, table, (long long)B * k * max_new};
  return done(launch_beam_step(logits, ldl, 1, B, k, V, max_new, eos_id, pad_id, nullptr, step, s, S(stream)), fn);
}
int opadpo_rope_kv_append(uint16_t* qkv, int ld, const float* cos_tab, const float* sin_tab, uint16_t* k_cache, uint16_t* v_cache,
                          int B, int nh, int hd, const int32_t* pos_ptr, int max_ctx, void* stream) {
  return done(launch_rope_kv_append(qkv, ld, cos_tab, sin_tab, k_cache, v_cache, B, nh, hd, pos_ptr, max_ctx, S(stream)),
              "opadpo_rope_kv_append");
}
int opadpo_sample(const float* logits, int ldl, int rows, int V, float temperature, int top_k, float top_p,
                  uint64_t seed, uint64_t step, const int32_t* step_ptr, uint8_t* finished, int pad_id, int eos_id,
                  int32_t* out, int32_t* history, void* stream) {
  if (temperature <= 0.f) return bad("opadpo_sample", "temperature must be > 0");
  return done(launch_sample(logits, ldl, rows, V, temperature, top_k, top_p, seed, step, step_ptr, finished, pad_id, eos_id, out,
                            history, S(stream)),
              "opadpo_sample");
}
int opadpo_sample_rows(const float* logits, int ldl, int rows, int V, float temperature, int top_k, float top_p, const uint64_t* seed_rows,
                       int32_t* step_rows, const int32_t* cap_rows, int max_steps, uint8_t* finished, int pad_id, int eos_id, int32_t* out,
                       int32_t* history, void* stream) {
  const char* fn = "opadpo_sample_rows";
  if (!(temperature > 0.f)) return bad(fn, "temperature must be > 0");
  if (rows < 1 || V < 1 || ldl < V || max_steps < 1) return bad(fn, "bad shape: need rows >= 1, V >= 1, ldl >= V, max_steps >= 1");
  if (!logits || !seed_rows || !step_rows || !cap_rows || !finished || !out) return bad(fn, "null operand (only history is nullable)");
  return done(launch_sample_rows(logits, ldl, rows, V, temperature, top_k, top_p, seed_rows, step_rows, cap_rows, max_steps, nullptr, 0, finished, pad_id,
                                 eos_id, out, history, S(stream)),
              fn);
}
// the launch wrappers refuse (hipErrorInvalidValue, nothing launched) what the message lists; the text is written here, where the caller reads it
int opadpo_logit_bias_add(float* logits, int ldl, int rows, int V, const int32_t* ids, const float* bias, const int32_t* ids_host, int n,
                          void* stream) {
  const hipError_t e = launch_logit_bias_add(logits, ldl, rows, V, ids, bias, ids_host, n, S(stream));
  if (e == hipErrorInvalidValue)
    return bad("opadpo_logit_bias_add", "need rows <= 64, 0 <= n <= 64, ldl >= V, non-null logits / ids / bias / ids_host, distinct ids inside [0, V)");
  return done(e, "opadpo_logit_bias_add");
}
int opadpo_gather_scores(const float* logits, int ldl, int rows, int V, const int32_t* ids, const int32_t* ids_host, int m, float temperature,
                         int top_k, float top_p, float* scores, void* stream) {
  const hipError_t e = launch_gather_scores(logits, ldl, rows, V, ids, ids_host, m, temperature, top_k, top_p, scores, S(stream));
  if (e == hipErrorInvalidValue)
    return bad("opadpo_gather_scores", "need rows <= 64, 0 <= m <= 64, ldl >= V, temperature >= 0, non-null logits / ids / ids_host / scores, ids inside [0, V)");
  return done(e, "opadpo_gather_scores");
}
int opadpo_token_logprobs(const float* logits, int ldl, int rows, int V, const int32_t* tokens, float temperature, int pad_id, float* logp,
                          float* ent, void* stream) {
  const hipError_t e = launch_token_logprobs(logits, ldl, rows, V, tokens, temperature, pad_id, nullptr, 1, logp, ent, S(stream));
  if (e == hipErrorInvalidValue)
    return bad("opadpo_token_logprobs", "need rows >= 1, V % 4 == 0, ldl % 4 == 0, ldl >= V, temperature >= 0, non-null 16-byte aligned logits, non-null tokens / logp");
  return done(e, "opadpo_token_logprobs");
}

// ---- gradient exchange for binders that do not go through torch.distributed (opadpo_allreduce_grads) -----------------------
// The collective library is NOT linked: the entry points resolve ncclAllReduce / ncclReduceScatter / ncclAllGather at first use from whatever RCCL the
// process has loaded (dlsym on the global scope; librccl.so by name as the fall-back), so a host that already carries an RCCL - PyTorch ships its own -
// keeps exactly one copy.  comm is the caller's ncclComm_t; one process per GPU, every call asynchronous on `stream`.
typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_reducescatter_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
static void* rccl_sym(const char* name) {
  void* f = dlsym(RTLD_DEFAULT, name);
  if (!f) {
    static void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (h) f = dlsym(h, name);
  }
  return f;
}
static int rccl_dtype(int dtype) { return dtype == 0 ? 7 /* ncclFloat32 */ : dtype == 1 ? 9 /* ncclBfloat16 */ : -1; }
int opadpo_allreduce_grads(void* nccl_comm, void* flat_grad, size_t count, int dtype, void* stream) {
  static nccl_allreduce_fn fn = (nccl_allreduce_fn)rccl_sym("ncclAllReduce");
  if (!fn) return bad("opadpo_allreduce_grads", "ncclAllReduce not found: no RCCL loaded in this process and librccl.so not on the loader path");
  if (!nccl_comm || !flat_grad || rccl_dtype(dtype) < 0) return bad("opadpo_allreduce_grads", "null communicator / buffer, or dtype not 0 (fp32) / 1 (bf16)");
  const int rc = fn(flat_grad, flat_grad, count, rccl_dtype(dtype), 0 /* ncclSum */, nccl_comm, S(stream));
  if (rc != 0) { snprintf(g_err, sizeof(g_err), "opadpo_allreduce_grads: ncclAllReduce returned %d", rc); return rc; }
  return 0;
}
int opadpo_reduce_scatter_grads(void* nccl_comm, const void* flat_grad, void* shard, size_t shard_count, int dtype, void* stream) {
  static nccl_reducescatter_fn fn = (nccl_reducescatter_fn)rccl_sym("ncclReduceScatter");
  if (!fn) return bad("opadpo_reduce_scatter_grads", "ncclReduceScatter not found: no RCCL loaded in this process and librccl.so not on the loader path");
  if (!nccl_comm || !flat_grad || !shard || rccl_dtype(dtype) < 0) return bad("opadpo_reduce_scatter_grads", "null communicator / buffer, or dtype not 0 / 1");
  const int rc = fn(flat_grad, shard, shard_count, rccl_dtype(dtype), 0, nccl_comm, S(stream));
  if (rc != 0) { snprintf(g_err, sizeof(g_err), "opadpo_reduce_scatter_grads: ncclReduceScatter returned %d", rc); return rc; }
  return 0;
}
int opadpo_all_gather_params(void* nccl_comm, const void* shard, void* flat, size_t shard_count, int dtype, void* stream) {
  static nccl_allgather_fn fn = (nccl_allgather_fn)rccl_sym("ncclAllGather");
  if (!fn) return bad("opadpo_all_gather_params", "ncclAllGather not found: no RCCL loaded in this process and librccl.so not on the loader path");
  if (!nccl_comm || !shard || !flat || rccl_dtype(dtype) < 0) return bad("opadpo_all_gather_params", "null communicator / buffer, or dtype not 0 / 1");
  const int rc = fn(shard, flat, shard_count, rccl_dtype(dtype), nccl_comm, S(stream));
  if (rc != 0) { snprintf(g_err, sizeof(g_err), "opadpo_all_gather_params: ncclAllGather returned %d", rc); return rc; }
  return 0;
}

}  // extern "C"
