// libgget_hip.so - operator-level entry points (gget_op_*, gget_debug_occupy): the launchers of kernels.h / gemm.h behind the C ABI, for
// tests and tools.  None of them takes a handle: of the engine this file uses only the split-K rules that engine.h declares (gget_op_slab_plan).
#include <string.h>

#include "common.h"
#include "engine.h"
#include "gemm.h"
#include "kernels.h"

// Stand-in for a collective's kernel in co-residency measurements (tools/coresidency.py): `blocks` workgroups of 256 threads
// with `lds_bytes` of LDS each stay resident for ~`microseconds`, streaming a little memory (a ring step's copy / reduce
// traffic) while they wait.  No reference counterpart: a measurement aid like gget_debug_set.
__global__ void __launch_bounds__(256) occupy_kernel(float* buf, size_t n, long long ticks) {
  extern __shared__ float occ_lds[];
  const long long t0 = wall_clock64();
  float acc = 0.f;
  size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) % n;
  while (wall_clock64() - t0 < ticks) {
    acc += buf[i];
    i = (i + 65536) % n;
    if (threadIdx.x == 0) occ_lds[0] = acc;
  }
  if (acc == 1.2345e-30f) buf[0] = acc;
}
// ... with the REGISTER footprint of RCCL's kernel (menu key 16, occupy_fat): rcclGenericKernel allocates 261 - 280 registers per lane (its
// gfx950 code object) - one wave of it per SIMD leaves no room for the two waves of a GEMM workgroup, whatever LDS is
// free.  The clobbers make the compiler allocate 256 vector + 8 accumulation registers; the loop is the same.
__global__ void __launch_bounds__(256) occupy_fat_kernel(float* buf, size_t n, long long ticks) {
  extern __shared__ float occ_lds[];
  asm volatile("" ::: "v255", "a7");
  const long long t0 = wall_clock64();
  float acc = 0.f;
  size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) % n;
  while (wall_clock64() - t0 < ticks) {
    acc += buf[i];
    i = (i + 65536) % n;
    if (threadIdx.x == 0) occ_lds[0] = acc;
  }
  if (acc == 1.2345e-30f) buf[0] = acc;
}
extern "C" int gget_debug_occupy(void* scratch, uint64_t scratch_bytes, int blocks, int lds_bytes, int microseconds, void* stream) {
  GGET_REQUIRE(scratch && scratch_bytes >= 4096 && blocks > 0 && lds_bytes >= 4 && lds_bytes <= 160 * 1024, "debug_occupy: bad arguments");
  static bool attr = false;
  if (!attr) {
    GGET_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&occupy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    GGET_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&occupy_fat_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr = true;
  }
  if (menu().occupy_fat) {
    hipLaunchKernelGGL(occupy_fat_kernel, dim3(blocks), dim3(256), lds_bytes, (hipStream_t)stream, (float*)scratch, scratch_bytes / 4,
                       (long long)microseconds * 100);
    GGET_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(occupy_kernel, dim3(blocks), dim3(256), lds_bytes, (hipStream_t)stream, (float*)scratch, scratch_bytes / 4,
                     (long long)microseconds * 100);   // wall_clock64 ticks at 100 MHz
  GGET_LAUNCH_CHECK();
  return 0;
}
extern "C" int gget_op_gemm(int mode, int epilogue, const void* A, const void* B, void* C, const void* R, int M, int N, int K,
                            int lda, int ldb, int ldc, int split_k, void* stream) {
  return gget_gemm_single(mode, epilogue, A, B, C, R, M, N, K, lda, ldb, ldc, nullptr, nullptr, split_k, (hipStream_t)stream);
}
extern "C" int gget_op_gemm_streamk(int mode, int epilogue, const void* A, const void* B, void* C, const void* R, int M, int N, int K,
                                    int lda, int ldb, int ldc, void* streamk_ws, void* stream) {
  GGET_REQUIRE(streamk_ws != nullptr, "gemm_streamk: null workspace");
  gget_gemm_streamk_workspace(streamk_ws);
  const int rc = gget_gemm_single(mode, epilogue, A, B, C, R, M, N, K, lda, ldb, ldc, nullptr, nullptr, 1, (hipStream_t)stream);
  gget_gemm_streamk_workspace(nullptr);
  return rc;
}
extern "C" uint64_t gget_op_gemm_streamk_bytes(void) { return gget_gemm_streamk_bytes(); }
extern "C" int gget_op_gemm_grouped(int mode, int count, const void* const* A, const void* const* B, void* const* Cs, const int* M,
                                   const int* N, const int* K, const int* lda, const int* ldb, const int* ldc, void* stream) {
  GGET_REQUIRE(count >= 1 && count <= GGET_MAX_GROUP && A && B && Cs && M && N && K && lda && ldb && ldc, "gemm_grouped: bad arguments");
  GemmGroup g;
  memset(&g, 0, sizeof(g));
  g.count = count;
  for (int i = 0; i < count; ++i) {
    GemmProblem& p = g.p[i];
    p.A = static_cast<const bf16_t*>(A[i]); p.B = static_cast<const bf16_t*>(B[i]); p.C = Cs[i];
    p.M = M[i]; p.N = N[i]; p.K = K[i]; p.lda = lda[i]; p.ldb = ldb[i]; p.ldc = ldc[i];
  }
  return gget_gemm_launch(mode, GGET_EPI_NONE, g, 1, (hipStream_t)stream);
}
// ---- test-only: the device-sized and split-K slab launches of the SMTP head and the shed weight gradients (include/gget.h) ----
extern "C" int gget_op_gemm_dyn(int mode, int epilogue, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                                const int32_t* m_dev, const int32_t* k_dev, int k_pad_zero, int split_k, const int32_t* c_rows, void* stream) {
  GGET_REQUIRE(A && B && C && M >= 0 && N > 0 && K >= 0, "gemm_dyn: bad arguments");
  GGET_REQUIRE(epilogue == GGET_EPI_NONE || epilogue == GGET_EPI_SLAB_F32, "gemm_dyn: the plain or the fp32 slab epilogue");
  GGET_REQUIRE(!k_pad_zero || k_dev, "gemm_dyn: k_pad_zero needs k_dev");
  return gget_gemm_single(mode, epilogue, A, B, C, nullptr, M, N, K, lda, ldb, ldc, m_dev, k_dev, split_k, (hipStream_t)stream, k_pad_zero != 0,
                          c_rows);
}
extern "C" int gget_op_gemm_grouped_slab(int mode, int count, const void* const* A, const void* const* B, void* const* Cs, const int* M,
                                         const int* N, const int* K, const int* lda, const int* ldb, const int* ldc, int64_t slab_stride,
                                         int split_k, void* stream) {
  GGET_REQUIRE(count >= 1 && count <= GGET_MAX_GROUP && A && B && Cs && M && N && K && lda && ldb && ldc && slab_stride > 0 && split_k >= 1,
               "gemm_grouped_slab: bad arguments");
  GemmGroup g;
  memset(&g, 0, sizeof(g));
  g.count = count;
  for (int i = 0; i < count; ++i) {
    GemmProblem& p = g.p[i];
    p.A = static_cast<const bf16_t*>(A[i]); p.B = static_cast<const bf16_t*>(B[i]); p.C = Cs[i];
    p.M = M[i]; p.N = N[i]; p.K = K[i]; p.lda = lda[i]; p.ldb = ldb[i]; p.ldc = ldc[i];
    p.slab_stride = (long)slab_stride;
  }
  return gget_gemm_launch(mode, GGET_EPI_SLAB_F32, g, split_k, (hipStream_t)stream);
}
extern "C" int gget_op_slab_reduce(const float* slabs, int64_t slab_stride, int nslab, void* dst, uint64_t n, int f32_out, void* stream) {
  GGET_REQUIRE(slabs && dst && nslab >= 1 && n % 4 == 0 && slab_stride % 4 == 0 && (nslab == 1 || slab_stride >= (int64_t)n),
               "slab_reduce: bad arguments (n and slab_stride are multiples of 4)");
  if (n == 0) return 0;
  return k_slab_reduce(slabs, (long)slab_stride, nslab, dst, (size_t)n, (hipStream_t)stream, f32_out != 0);
}
extern "C" int gget_op_slab_plan(int which, int d, int V, int T, int* split) {
  GGET_REQUIRE(split && d > 0 && V > 0 && T >= 0, "slab_plan: bad arguments");
  switch (which) {
    case GGET_SLAB_PLAN_LM_HEAD: *split = lm_wgrad_split(V, d); return 0;
    case GGET_SLAB_PLAN_SHED_QKVO: *split = shed_wgrad_split(true, d, T); return 0;
    case GGET_SLAB_PLAN_SHED_O: *split = shed_wgrad_split(false, d, T); return 0;
    case GGET_SLAB_PLAN_QKVO: *split = qkvo_wgrad_split(T); return 0;
  }
  gget_set_error("slab_plan: unknown launch %d", which);
  return 2;
}
extern "C" int gget_op_qkv_rope(const void* x, const void* wqkv, void* qkv, const float* cos_tab, const float* sin_tab,
                                const int64_t* position_ids, int T, int S, int d, void* stream) {
  GGET_REQUIRE(x && wqkv && qkv && cos_tab && sin_tab, "qkv_rope: null argument");
  GGET_REQUIRE(d > 0 && d % 64 == 0 && T > 0 && S > 0, "qkv_rope: bad shape T %d S %d d %d", T, S, d);
  GemmGroup g;
  memset(&g, 0, sizeof(g));
  g.count = 1;
  GemmProblem& p = g.p[0];
  p.A = static_cast<const bf16_t*>(x); p.B = static_cast<const bf16_t*>(wqkv); p.C = qkv;
  p.M = T; p.N = 3 * d; p.K = d; p.lda = d; p.ldb = d; p.ldc = 3 * d;
  p.rope_cos = cos_tab; p.rope_sin = sin_tab; p.rope_pos = position_ids; p.rope_S = S; p.rope_cols = 2 * d;
  return gget_gemm_launch(GGET_GEMM_NT, GGET_EPI_ROPE, g, 1, (hipStream_t)stream);
}
extern "C" int gget_op_smtp2d(const int64_t* ids_in, int ld_in, const int64_t* node_idx, int ld_node, int64_t* ids_out,
                              int64_t* labels_out, int B, int S, int F, float smtp_2d_rate, float power, float replace_rate,
                              int vocab, int global_2d_mask, uint32_t seed, void* stream) {
  GGET_REQUIRE(ids_in && node_idx && ids_out && labels_out, "smtp2d: null argument");
  GGET_REQUIRE(B >= 0 && S >= 0 && F >= 1 && ld_in >= F && ld_node >= 1 && vocab >= 2, "smtp2d: bad shape");
  return k_smtp2d(ids_in, ld_in, node_idx, ld_node, ids_out, labels_out, B, S, F, smtp_2d_rate, power, replace_rate, vocab,
                  global_2d_mask, seed, (hipStream_t)stream);
}
extern "C" int gget_op_token_sample(const void* logits, int ld, int R, int V, int mode, float temperature, float top_p, int top_k,
                                   float alg_temp, uint32_t seed, float* conf, int64_t* tok, void* stream) {
  GGET_REQUIRE(logits && conf && tok && R >= 0 && V >= 1 && ld >= V && mode >= 0 && mode <= 2, "token_sample: bad arguments");
  return k_token_sample(logits, ld, R, V, mode, temperature, top_p, top_k, alg_temp, seed, conf, tok, nullptr, 0, (hipStream_t)stream);
}
extern "C" int gget_op_token_sample_probs(const void* logits, int ld, int R, int V, int mode, float temperature, float top_p, int top_k,
                                         float alg_temp, uint32_t seed, float* conf, int64_t* tok, float* probs, int ld_p, void* stream) {
  GGET_REQUIRE(logits && conf && tok && R >= 0 && V >= 1 && ld >= V && mode >= 0 && mode <= 2, "token_sample_probs: bad arguments");
  GGET_REQUIRE(!probs || ld_p >= V, "token_sample_probs: ld_p %d below V %d", ld_p, V);
  return k_token_sample(logits, ld, R, V, mode, temperature, top_p, top_k, alg_temp, seed, conf, tok, probs, ld_p, (hipStream_t)stream);
}
extern "C" int gget_op_unmask_origin(int64_t* x, const int64_t* cand, int B, int N, float p_transfer, uint32_t seed, int mask_token_id,
                                     void* stream) {
  GGET_REQUIRE(x && cand && B >= 0 && N >= 0, "unmask_origin: bad arguments");
  return k_unmask_origin(x, cand, B, N, p_transfer, seed, mask_token_id, (hipStream_t)stream);
}
extern "C" int gget_op_unmask_origin_rows(int64_t* x, const int64_t* cand, int B, int N, const float* p_transfer, uint32_t seed,
                                          int mask_token_id, void* stream) {
  GGET_REQUIRE(x && cand && p_transfer && B >= 0 && N >= 0, "unmask_origin_rows: bad arguments");
  return k_unmask_origin_rows(x, cand, B, N, p_transfer, seed, mask_token_id, (hipStream_t)stream);
}
extern "C" int gget_op_token_confidence(const void* logits, int ld, int R, int V, int mode, float* conf, int64_t* tok, void* stream) {
  GGET_REQUIRE(logits && conf && tok, "token_confidence: null argument");
  GGET_REQUIRE(R >= 0 && V >= 2 && ld >= V && mode >= 0 && mode <= 2, "token_confidence: bad arguments (R %d V %d ld %d mode %d)", R, V, ld, mode);
  return k_token_confidence(logits, ld, R, V, mode, conf, tok, (hipStream_t)stream);
}
extern "C" int gget_op_smtp_rows(const int64_t* ids_in, const int32_t* lengths, int64_t* ids_out, int64_t* labels_out,
                                 float* wgt_out, int B, int S, int F, double umr_min, double umr_max, double power, uint32_t seed,
                                 void* stream) {
  GGET_REQUIRE(ids_in && lengths && ids_out && labels_out, "smtp_rows: null argument");
  GGET_REQUIRE(B >= 0 && S >= 1 && F >= 1 && (long)S * F < (1l << 20), "smtp_rows: bad shape (S*F must be < 2^20)");
  GGET_REQUIRE(0.0 <= umr_min && umr_min <= umr_max && umr_max <= 1.0 && power > 0.0, "smtp_rows: bad schedule");
  return k_smtp_rows(ids_in, lengths, ids_out, labels_out, wgt_out, B, S, F, umr_min, umr_max, power, seed, (hipStream_t)stream);
}
extern "C" int gget_op_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int T, int d, float eps, void* stream) {
  return k_rmsnorm_fwd(x, w, y, rstd, T, d, eps, (hipStream_t)stream);
}
extern "C" int gget_op_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx,
                                   float* dw_accum, int T, int d, void* stream) {
  return k_rmsnorm_bwd(dy, x, w, rstd, dres, dx, dw_accum, T, d, (hipStream_t)stream);
}
// (the _drop entries: embedding dropout from (elem_p, elem_seed, elem_rows) through elem_drop; the plain ones call them with it off)
extern "C" int gget_op_embed_fwd_drop(const int64_t* ids, const void* emb, const void* gate, void* out, int T, int F, int ldF, int d,
                                      float elem_p, uint32_t elem_seed, const int32_t* elem_rows, void* stream) {
  GGET_REQUIRE(elem_p < 1.f, "embed_fwd: bad mask arguments");
  return k_embed_fwd(ids, emb, gate, out, T, F, ldF, d, (hipStream_t)stream, elem_drop(elem_p, elem_seed, elem_rows));
}
extern "C" int gget_op_embed_fwd(const int64_t* ids, const void* emb, const void* gate, void* out, int T, int F, int ldF, int d,
                                 void* stream) {
  return gget_op_embed_fwd_drop(ids, emb, gate, out, T, F, ldF, d, 0.f, 0u, nullptr, stream);
}
extern "C" int gget_op_embed_bwd_drop(const int64_t* ids, const void* dx, const void* emb, const void* gate, float* demb_accum,
                                      float* dgate_accum, int T, int F, int ldF, int d, int V, int pad_id, float elem_p, uint32_t elem_seed,
                                      const int32_t* elem_rows, void* stream) {
  GGET_REQUIRE(elem_p < 1.f, "embed_bwd: bad mask arguments");
  // (before the workspaces are sized from them; the launchers check again)
  GGET_REQUIRE(ids && dx && demb_accum && (!gate || (emb && dgate_accum)), "embed_bwd: null argument");
  GGET_REQUIRE(T >= 0 && F >= 1 && ldF >= F && d > 0 && d % 8 == 0 && V >= 1, "embed_bwd: bad shape T %d F %d ldF %d d %d V %d", T, F, ldF, d, V);
  int32_t* ws = nullptr;
  GGET_HIP_CHECK(hipMalloc(&ws, k_embed_bwd_ws_elems((size_t)T * F, (size_t)V) * sizeof(int32_t)));  // test-only entry point
  void* cnt = nullptr;   // (GGET_EMBED_SORTED=1 forces the sorted scatter-add)
  if (k_embed_dense_ok(V, gate != nullptr))
    GGET_HIP_CHECK(hipMalloc(&cnt, (size_t)T * align_up((uint64_t)V, 64) * 2 + (size_t)kEmbDenseSplit * V * d * 4));
  void* slab = cnt ? static_cast<unsigned char*>(cnt) + (size_t)T * align_up((uint64_t)V, 64) * 2 : nullptr;
  const int rc = embed_bwd(ids, dx, emb, gate, demb_accum, dgate_accum, T, F, ldF, d, V, pad_id, ws, cnt, slab, (hipStream_t)stream,
                           elem_drop(elem_p, elem_seed, elem_rows));
  (void)hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(ws);
  if (cnt) (void)hipFree(cnt);
  return rc;
}
extern "C" int gget_op_embed_bwd(const int64_t* ids, const void* dx, const void* emb, const void* gate, float* demb_accum,
                                 float* dgate_accum, int T, int F, int ldF, int d, int V, int pad_id, void* stream) {
  return gget_op_embed_bwd_drop(ids, dx, emb, gate, demb_accum, dgate_accum, T, F, ldF, d, V, pad_id, 0.f, 0u, nullptr, stream);
}
extern "C" int gget_op_rope(void* qkv, const float* cos_tab, const float* sin_tab, const int64_t* position_ids, int B, int S,
                            int H, int inverse, void* stream) {
  return k_rope(qkv, cos_tab, sin_tab, position_ids, B * S, S, H, inverse, (hipStream_t)stream);
}
extern "C" int gget_op_attn_fwd(const void* qkv, const int32_t* key_len, void* out, float* lse, int B, int S, int H, int causal,
                                const float* cos_tab, const float* sin_tab, const int64_t* position_ids, float dropout_p,
                                uint32_t dropout_seed, void* stream) {
  return k_attn_fwd(qkv, key_len, out, lse, B, S, H, causal, cos_tab, sin_tab, position_ids, dropout_p, dropout_seed,
                    (hipStream_t)stream);
}
extern "C" int gget_op_attn_oproj_fwd(const void* qkv, const int32_t* key_len, const int32_t* row_base, void* attn_out, float* lse,
                                      const void* wo, const void* x_in, void* x_mid, const void* norm_w, void* xn, float* rstd, int B, int S,
                                      int H, int causal, float eps, float dropout_p, uint32_t dropout_seed, void* stream, int32_t* taken) {
  GGET_REQUIRE(qkv && attn_out && wo && x_in && x_mid && norm_w && xn && taken, "null argument");
  int t = 0;
  const int rc = k_attn_oproj_fwd(qkv, key_len, row_base, attn_out, lse, wo, x_in, x_mid, norm_w, xn, rstd, B, S, H, causal, eps, dropout_p,
                                  dropout_seed, (hipStream_t)stream, &t);
  *taken = t;
  return rc;
}
extern "C" int gget_op_pack_wo(const void* w, uint64_t layer_stride, void* fwd, void* bwd, int d, int layers, void* stream) {
  GGET_REQUIRE(w && fwd && bwd, "null argument");
  return k_pack_wo(w, (size_t)layer_stride, fwd, bwd, d, layers, (hipStream_t)stream);
}
extern "C" int gget_op_attn_oproj_bwd(const void* dxn, const void* x_mid, const void* norm_w, const float* rstd, const void* dres, void* dx_mid,
                                      float* dw_accum, int copies, uint64_t copy_stride, const void* wot_packed, const void* qkv, const float* lse,
                                      const int32_t* key_len, const int32_t* row_base, void* dqkv, int B, int S, int H, int causal,
                                      const float* cos_tab, const float* sin_tab, const int64_t* position_ids, float dropout_p,
                                      uint32_t dropout_seed, int t_rows, void* stream, int32_t* taken, void* dattn_long) {
  GGET_REQUIRE(dxn && x_mid && norm_w && rstd && dres && dx_mid && dw_accum && wot_packed && qkv && lse && dqkv && taken, "null argument");
  int t = 0;
  const int rc = k_attn_oproj_bwd(dxn, x_mid, norm_w, rstd, dres, dx_mid, dw_accum, copies, copy_stride, wot_packed, qkv, lse, key_len, row_base,
                                  dqkv, B, S, H, causal, cos_tab, sin_tab, position_ids, dropout_p, dropout_seed, t_rows, (hipStream_t)stream, &t,
                                  dattn_long, nullptr);
  *taken = t;
  return rc;
}
extern "C" int gget_op_attn_oproj_bwd_list(const void* dxn, const void* x_mid, const void* norm_w, const float* rstd, const void* dres,
                                           void* dx_mid, float* dw_accum, int copies, uint64_t copy_stride, const void* wot_packed,
                                           const void* qkv, const float* lse, const int32_t* key_len, const int32_t* row_base, void* dqkv, int B,
                                           int S, int H, int causal, const float* cos_tab, const float* sin_tab, const int64_t* position_ids,
                                           float dropout_p, uint32_t dropout_seed, int t_rows, void* stream, int32_t* taken, void* dattn_long,
                                           const int32_t* long_list) {
  GGET_REQUIRE(dxn && x_mid && norm_w && rstd && dres && dx_mid && dw_accum && wot_packed && qkv && lse && dqkv && taken, "null argument");
  GGET_REQUIRE(!long_list || row_base, "attn_oproj_bwd_list: the list of long samples belongs to the var-len layout");
  int t = 0;
  const int rc = k_attn_oproj_bwd(dxn, x_mid, norm_w, rstd, dres, dx_mid, dw_accum, copies, copy_stride, wot_packed, qkv, lse, key_len, row_base,
                                  dqkv, B, S, H, causal, cos_tab, sin_tab, position_ids, dropout_p, dropout_seed, t_rows, (hipStream_t)stream, &t,
                                  dattn_long, long_list);
  *taken = t;
  return rc;
}
extern "C" int gget_op_attn_fwd_ranges(const void* qkv, const int32_t* key_lo, const int32_t* key_hi, void* out, float* lse, int B,
                                       int S, int H, int causal, float dropout_p, uint32_t dropout_seed, void* stream) {
  GGET_REQUIRE(key_lo && key_hi, "attn_fwd_ranges: null ranges");
  return k_attn_fwd(qkv, nullptr, out, lse, B, S, H, causal, nullptr, nullptr, nullptr, dropout_p, dropout_seed,
                    (hipStream_t)stream, key_lo, key_hi);
}
extern "C" int gget_op_attn_bwd_ranges(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_lo,
                                       const int32_t* key_hi, void* dqkv, float* delta_ws, int B, int S, int H, int causal,
                                       float dropout_p, uint32_t dropout_seed, void* stream) {
  GGET_REQUIRE(key_lo && key_hi, "attn_bwd_ranges: null ranges");
  return k_attn_bwd(qkv, out, dout, lse, nullptr, dqkv, delta_ws, B, S, H, causal, nullptr, nullptr, nullptr, 0, dropout_p,
                    dropout_seed, (hipStream_t)stream, key_lo, key_hi);
}
extern "C" int gget_op_attn_probs(const void* qkv, const float* lse, const int32_t* key_len, const int32_t* row_base, const int32_t* key_lo,
                                  const int32_t* key_hi, void* out, int B, int S, int H, int causal, float dropout_p, uint32_t dropout_seed,
                                  void* stream) {
  return k_attn_probs(qkv, lse, key_len, row_base, key_lo, key_hi, out, B, S, H, causal, dropout_p, dropout_seed, (hipStream_t)stream);
}
// The head-width-parameterised entries: head_dim 64 forwards to the kernels above with the same arguments (q, k rotated in qkv), 32 runs
// the family of attention32.hip.  Every check is made here, before any launch.
static int hd_check(const char* who, int B, int S, int H, int head_dim, const int32_t* key_len, const int32_t* row_base, const int32_t* key_lo,
                    const int32_t* key_hi) {
  GGET_REQUIRE(head_dim == 64 || head_dim == 32, "%s: unsupported head_dim %d (64 or 32)", who, head_dim);
  GGET_REQUIRE(B > 0 && S > 0 && H > 0 && B <= 65535 && H <= 65535, "%s: bad shape B %d S %d H %d", who, B, S, H);
  GGET_REQUIRE(!key_lo == !key_hi, "%s: half a key range", who);
  GGET_REQUIRE(!row_base || (key_len && !key_lo), "%s: the var-len token layout needs key_len and excludes per-token key ranges", who);
  return 0;
}
extern "C" int gget_op_rope_hd(void* qkv, const float* cos_tab, const float* sin_tab, const int64_t* position_ids, int B, int S, int H,
                               int head_dim, int inverse, void* stream) {
  GGET_REQUIRE(head_dim == 64 || head_dim == 32, "rope_hd: unsupported head_dim %d (64 or 32)", head_dim);
  GGET_REQUIRE(qkv && cos_tab && sin_tab, "rope_hd: null argument");
  GGET_REQUIRE(B > 0 && S > 0 && H > 0, "rope_hd: bad shape B %d S %d H %d", B, S, H);
  if (head_dim == 64) return k_rope(qkv, cos_tab, sin_tab, position_ids, B * S, S, H, inverse, (hipStream_t)stream);
  return k_rope32(qkv, cos_tab, sin_tab, position_ids, B * S, S, H, inverse, (hipStream_t)stream);
}
extern "C" int gget_op_rope_f32_hd(const float* src, void* qkv, const float* cos_tab, const float* sin_tab, const int64_t* position_ids, int B,
                                   int S, int H, int head_dim, void* stream) {
  GGET_REQUIRE(head_dim == 32, "rope_f32_hd: unsupported head_dim %d (32: the 64-wide projection rotates in its GEMM epilogue)", head_dim);
  GGET_REQUIRE(src && qkv && cos_tab && sin_tab, "rope_f32_hd: null argument");
  GGET_REQUIRE(B > 0 && S > 0 && H > 0, "rope_f32_hd: bad shape B %d S %d H %d", B, S, H);
  return k_rope32_f32(src, qkv, cos_tab, sin_tab, position_ids, B * S, S, H, (hipStream_t)stream);
}
extern "C" int gget_op_attn_fwd_hd(const void* qkv, const int32_t* key_len, const int32_t* row_base, const int32_t* key_lo,
                                   const int32_t* key_hi, void* out, float* lse, int B, int S, int H, int head_dim, int causal,
                                   float dropout_p, uint32_t dropout_seed, void* stream) {
  if (int e = hd_check("attn_fwd_hd", B, S, H, head_dim, key_len, row_base, key_lo, key_hi)) return e;
  GGET_REQUIRE(qkv && out && lse, "attn_fwd_hd: null argument");
  return k_attn_fwd(qkv, key_lo ? nullptr : key_len, out, lse, B, S, H, causal, nullptr, nullptr, nullptr, dropout_p, dropout_seed,
                    (hipStream_t)stream, key_lo, key_hi, row_base, nullptr, head_dim);
}
extern "C" int gget_op_attn_bwd_hd(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len,
                                   const int32_t* row_base, const int32_t* key_lo, const int32_t* key_hi, void* dqkv, float* delta_ws, int B,
                                   int S, int H, int head_dim, int causal, const float* cos_tab, const float* sin_tab,
                                   const int64_t* position_ids, float dropout_p, uint32_t dropout_seed, void* stream) {
  if (int e = hd_check("attn_bwd_hd", B, S, H, head_dim, key_len, row_base, key_lo, key_hi)) return e;
  GGET_REQUIRE(qkv && out && dout && lse && dqkv && delta_ws, "attn_bwd_hd: null argument");
  GGET_REQUIRE(!cos_tab == !sin_tab, "attn_bwd_hd: half an angle table");
  return k_attn_bwd(qkv, out, dout, lse, key_lo ? nullptr : key_len, dqkv, delta_ws, B, S, H, causal, cos_tab, sin_tab, position_ids,
                    /*qk_rotated=*/1, dropout_p, dropout_seed, (hipStream_t)stream, key_lo, key_hi, row_base, nullptr, 0, nullptr, head_dim);
}
extern "C" int gget_op_attn_probs_hd(const void* qkv, const float* lse, const int32_t* key_len, const int32_t* row_base, const int32_t* key_lo,
                                     const int32_t* key_hi, void* out, int B, int S, int H, int head_dim, int causal, float dropout_p,
                                     uint32_t dropout_seed, void* stream) {
  if (int e = hd_check("attn_probs_hd", B, S, H, head_dim, key_len, row_base, key_lo, key_hi)) return e;
  GGET_REQUIRE(qkv && lse && out, "attn_probs_hd: null argument");
  GGET_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "attn_probs_hd: dropout_p %g outside [0, 1)", (double)dropout_p);
  return k_attn_probs(qkv, lse, key_len, row_base, key_lo, key_hi, out, B, S, H, causal, dropout_p, dropout_seed, (hipStream_t)stream,
                      head_dim);
}
extern "C" int gget_op_ranges_from_mask3d(const int64_t* mask3d, int32_t* key_lo, int32_t* key_hi, int B, int S, void* stream) {
  GGET_REQUIRE(mask3d && key_lo && key_hi, "ranges_from_mask3d: null argument");
  return k_ranges_from_mask3d(mask3d, key_lo, key_hi, B, S, (hipStream_t)stream);
}
extern "C" int gget_op_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len,
                                void* dqkv, float* delta_ws, int B, int S, int H, int causal, const float* cos_tab,
                                const float* sin_tab, const int64_t* position_ids, float dropout_p, uint32_t dropout_seed,
                                void* stream) {
  return k_attn_bwd(qkv, out, dout, lse, key_len, dqkv, delta_ws, B, S, H, causal, cos_tab, sin_tab, position_ids,
                    /*qk_rotated=*/0, dropout_p, dropout_seed, (hipStream_t)stream);
}
extern "C" int gget_op_copy_from_host(const void* src_pinned_host, void* dst_dev, uint64_t bytes, void* stream) {
  GGET_REQUIRE(src_pinned_host && dst_dev, "copy_from_host: null argument");
  return k_copy_from_host(src_pinned_host, dst_dev, (size_t)bytes, (hipStream_t)stream);
}
extern "C" int gget_op_attn_fwd_varlen(const void* qkv, const int32_t* key_len, const int32_t* row_base, void* out, float* lse, int B, int S,
                                       int H, int causal, const float* cos_tab, const float* sin_tab, const int64_t* position_ids,
                                       int qk_rotated, float dropout_p, uint32_t dropout_seed, void* stream) {
  GGET_REQUIRE(qkv && key_len && row_base && out, "attn_fwd_varlen: null argument");
  // (rotated q / k: the forward reads them as they are)
  return k_attn_fwd(qkv, key_len, out, lse, B, S, H, causal, qk_rotated ? nullptr : cos_tab, qk_rotated ? nullptr : sin_tab,
                    qk_rotated ? nullptr : position_ids, dropout_p, dropout_seed, (hipStream_t)stream, nullptr, nullptr, row_base);
}
extern "C" int gget_op_attn_bwd_varlen(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len,
                                       const int32_t* row_base, void* dqkv, float* delta_ws, int B, int S, int H, int causal,
                                       const float* cos_tab, const float* sin_tab, const int64_t* position_ids, int qk_rotated,
                                       float dropout_p, uint32_t dropout_seed, void* stream) {
  GGET_REQUIRE(qkv && dout && key_len && row_base && dqkv, "attn_bwd_varlen: null argument");
  return k_attn_bwd(qkv, out, dout, lse, key_len, dqkv, delta_ws, B, S, H, causal, cos_tab, sin_tab, position_ids, qk_rotated, dropout_p,
                    dropout_seed, (hipStream_t)stream, nullptr, nullptr, row_base);
}
extern "C" int gget_op_attn_bwd_varlen_list(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len,
                                            const int32_t* row_base, void* dqkv, float* delta_ws, int B, int S, int H, int causal,
                                            const float* cos_tab, const float* sin_tab, const int64_t* position_ids, int qk_rotated,
                                            float dropout_p, uint32_t dropout_seed, void* stream, const int32_t* long_list) {
  GGET_REQUIRE(qkv && dout && key_len && row_base && dqkv, "attn_bwd_varlen_list: null argument");
  return k_attn_bwd(qkv, out, dout, lse, key_len, dqkv, delta_ws, B, S, H, causal, cos_tab, sin_tab, position_ids, qk_rotated, dropout_p,
                    dropout_seed, (hipStream_t)stream, nullptr, nullptr, row_base, nullptr, 0, long_list);
}
extern "C" int gget_op_attn_bwd_fused(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len,
                                      const int32_t* key_lo, const int32_t* key_hi, void* dqkv, float* delta_ws, void* dq_ws, int B, int S,
                                      int H, int causal, float dropout_p, uint32_t dropout_seed, void* stream) {
  GGET_REQUIRE(dq_ws && (!key_lo == !key_hi), "attn_bwd_fused: null workspace / half a key range");
  return k_attn_bwd(qkv, out, dout, lse, key_lo ? nullptr : key_len, dqkv, delta_ws, B, S, H, causal, nullptr, nullptr, nullptr, 0, dropout_p,
                    dropout_seed, (hipStream_t)stream, key_lo, key_hi, nullptr, dq_ws, (size_t)B * S * H * 64);
}
extern "C" int gget_op_gateup_geglu(const void* x, const void* wgu, void* gu, void* h, int T, int d, int ff, void* stream) {
  GGET_REQUIRE(x && wgu && gu && h && T > 0, "gateup_geglu: null argument");
  return gateup_geglu((const bf16_t*)x, (const bf16_t*)wgu, (bf16_t*)gu, (bf16_t*)h, T, d, ff, (hipStream_t)stream);
}
extern "C" int gget_op_down_dgrad_geglu(const void* dy, const void* wdown, const void* gu, void* dgu, void* dh_scratch, int T, int d,
                                        int ff, void* stream) {
  GGET_REQUIRE(dy && wdown && gu && dgu && T > 0, "down_dgrad_geglu: null argument");
  GGET_REQUIRE(dh_scratch || geglu_fusable(d, ff), "down_dgrad_geglu: this shape needs the [T][ff] dh scratch buffer");
  return down_dgrad_geglu((const bf16_t*)dy, (const bf16_t*)wdown, (const bf16_t*)gu, (bf16_t*)dgu, (bf16_t*)dh_scratch, T, d, ff,
                          (hipStream_t)stream);
}
extern "C" int gget_op_geglu_fwd(const void* gu, void* h, int T, int ff, void* stream) {
  return k_geglu_fwd(gu, h, T, ff, (hipStream_t)stream);
}
extern "C" int gget_op_geglu_bwd(const void* gu, const void* dh, void* dgu, int T, int ff, void* stream) {
  return k_geglu_bwd(gu, dh, dgu, T, ff, (hipStream_t)stream);
}
extern "C" int gget_op_ce_fwd_bwd(const void* logits, int ld, const int32_t* labels, const float* row_wgt,
                                  const int32_t* n_rows_dev, int n_rows_cap, int V, float* loss_sum, void* dlogits,
                                  float grad_scale_base, int mean_over_rows, void* stream) {
  GGET_REQUIRE(row_wgt == nullptr, "per-row weights go through the engine path (sample_wgt)");
  return k_ce_fwd_bwd(logits, ld, labels, nullptr, nullptr, 1, n_rows_dev, n_rows_cap, V, loss_sum, dlogits, grad_scale_base,
                      mean_over_rows, nullptr, (hipStream_t)stream);
}
// test-only entries of the element-wise kernels: every argument of the launcher, no arithmetic here
extern "C" int gget_op_rope_table(float* cos_tab, float* sin_tab, int max_pos, float theta, void* stream) {
  GGET_REQUIRE(cos_tab && sin_tab && max_pos >= 1 && theta > 0.f, "rope_table: bad arguments");
  return k_rope_table(cos_tab, sin_tab, max_pos, theta, (hipStream_t)stream);
}
extern "C" int gget_op_rope_range_table(const int64_t* pos, float* cos_tab, float* sin_tab, int64_t* ids, int B, int S, float range, float theta,
                                        void* stream) {
  GGET_REQUIRE(pos && cos_tab && sin_tab && ids && B >= 0 && S >= 1 && range > 0.f && theta > 0.f, "rope_range_table: bad arguments");
  return k_rope_range_table(pos, cos_tab, sin_tab, ids, B, S, range, theta, (hipStream_t)stream);
}
extern "C" int gget_op_clamp_positions(const int64_t* pos, int64_t* out, int32_t* flag, int64_t n, int max_pos, void* stream) {
  GGET_REQUIRE(pos && out && flag && n >= 0 && max_pos >= 1, "clamp_positions: bad arguments");
  return k_clamp_positions(pos, out, flag, (long)n, max_pos, (hipStream_t)stream);
}
extern "C" int gget_op_embed_long_ratio(const int64_t* ids, void* x, int T, int F, int ldF, int d, void* stream) {
  return k_embed_long_ratio(ids, x, T, F, ldF, d, (hipStream_t)stream);
}
// test-only entries of the RMSNorm and cross-entropy families: every argument of the launcher, no arithmetic here
extern "C" int gget_op_rmsnorm_bwd_copies(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx,
                                          float* dw_accum, int T, int d, int copies, uint64_t copy_stride, void* stream) {
  GGET_REQUIRE(dy && x && w && rstd && dx && dw_accum && T >= 0 && copies >= 1 && copy_stride >= (uint64_t)d, "rmsnorm_bwd_copies: bad arguments");
  return k_rmsnorm_bwd(dy, x, w, rstd, dres, dx, dw_accum, T, d, (hipStream_t)stream, copies, copy_stride);
}
extern "C" int gget_op_rmsnorm_dw(const void* dy, const void* x, const float* rstd, float* dw_accum, int T, int d, int copies,
                                  uint64_t copy_stride, void* stream) {
  GGET_REQUIRE(dy && x && rstd && dw_accum && T >= 0 && copies >= 1 && copy_stride >= (uint64_t)d, "rmsnorm_dw: bad arguments");
  return k_rmsnorm_dw(dy, x, rstd, dw_accum, T, d, (hipStream_t)stream, copies, copy_stride);
}
// test-only entries of the dropout / DropPath / LayerScale family (tests/test_gpu_drop.py): every argument of the launcher, no arithmetic
// here.  The masks: (elem_p, elem_seed, elem_rows) becomes the ElemDropArg through elem_drop (kernels.h) - the engine's threshold rule -
// and (path_rate, path_seed, path_S, path_row_b) is the PathDropArg as it stands.  The entries without masks call these with everything off.
static PathDropArg path_arg(float rate, uint32_t seed, int S, const int32_t* row_b) { return PathDropArg{rate, seed, S, row_b}; }
static int check_masks(const char* entry, float elem_p, float path_rate, int path_S, const int32_t* path_row_b) {
  GGET_REQUIRE(elem_p < 1.f && path_rate < 1.f && (path_rate <= 0.f || path_row_b || path_S >= 1), "%s: bad mask arguments", entry);
  return 0;
}
extern "C" int gget_op_ls_rmsnorm_fwd_drop(const void* res, const void* y, const void* lam, void* out, const void* w, void* xn, float* rstd,
                                           int T, int d, float eps, float elem_p, uint32_t elem_seed, const int32_t* elem_rows,
                                           float path_rate, uint32_t path_seed, int path_S, const int32_t* path_row_b, void* stream) {
  GGET_REQUIRE(res && y && out && w && xn && rstd && T >= 0, "ls_rmsnorm_fwd: null argument");
  GGET_REQUIRE(d > 0 && d % 8 == 0 && d <= 2048, "ls_rmsnorm_fwd: d=%d unsupported", d);
  if (int e = check_masks("ls_rmsnorm_fwd", elem_p, path_rate, path_S, path_row_b)) return e;
  if (T == 0) return 0;
  return k_ls_rmsnorm_fwd((const bf16_t*)res, (const bf16_t*)y, (const bf16_t*)lam, (bf16_t*)out, (const bf16_t*)w, (bf16_t*)xn, rstd, T, d, eps,
                          path_arg(path_rate, path_seed, path_S, path_row_b), elem_drop(elem_p, elem_seed, elem_rows), (hipStream_t)stream);
}
extern "C" int gget_op_ls_rmsnorm_fwd(const void* res, const void* y, const void* lam, void* out, const void* w, void* xn, float* rstd, int T,
                                      int d, float eps, void* stream) {
  return gget_op_ls_rmsnorm_fwd_drop(res, y, lam, out, w, xn, rstd, T, d, eps, 0.f, 0u, nullptr, 0.f, 0u, 1, nullptr, stream);
}
extern "C" int gget_op_ls_fwd(const void* res, const void* y, const void* lam, void* out, int T, int d, float elem_p, uint32_t elem_seed,
                              const int32_t* elem_rows, float path_rate, uint32_t path_seed, int path_S, const int32_t* path_row_b,
                              void* stream) {
  GGET_REQUIRE(res && y && out && T >= 0, "ls_fwd: null argument");
  GGET_REQUIRE(d > 0 && d % 8 == 0 && d <= 2048, "ls_fwd: d=%d unsupported", d);
  if (int e = check_masks("ls_fwd", elem_p, path_rate, path_S, path_row_b)) return e;
  return k_ls_fwd((const bf16_t*)res, (const bf16_t*)y, (const bf16_t*)lam, (bf16_t*)out, T, d, path_arg(path_rate, path_seed, path_S, path_row_b),
                  elem_drop(elem_p, elem_seed, elem_rows), (hipStream_t)stream);
}
/* dlam_accum: the kAccumCopies replicas of gget_op_accum_layout, or NULL */
extern "C" int gget_op_ls_bwd(const void* dy, const void* y, const void* lam, void* dsc, float* dlam_accum, int T, int d, float elem_p,
                              uint32_t elem_seed, const int32_t* elem_rows, float path_rate, uint32_t path_seed, int path_S,
                              const int32_t* path_row_b, void* stream) {
  GGET_REQUIRE(dy && y && dsc && T >= 0, "ls_bwd: null argument");
  GGET_REQUIRE(d > 0 && d % 8 == 0 && d <= 2048, "ls_bwd: d=%d unsupported", d);
  if (int e = check_masks("ls_bwd", elem_p, path_rate, path_S, path_row_b)) return e;
  return k_ls_bwd((const bf16_t*)dy, (const bf16_t*)y, (const bf16_t*)lam, (bf16_t*)dsc, dlam_accum, T, d,
                  path_arg(path_rate, path_seed, path_S, path_row_b), elem_drop(elem_p, elem_seed, elem_rows), (hipStream_t)stream);
}
extern "C" int gget_op_elem_dropout(void* x, int64_t T, int n, uint32_t stream_id, float elem_p, uint32_t elem_seed, const int32_t* elem_rows,
                                    void* stream) {
  GGET_REQUIRE(x && T >= 0 && n > 0 && elem_p < 1.f, "elem_dropout: bad arguments");
  return k_elem_dropout(x, (long)T, n, stream_id, elem_drop(elem_p, elem_seed, elem_rows), (hipStream_t)stream);
}
extern "C" int gget_op_accum_layout(int d, int* copies, uint64_t* copy_stride) {
  GGET_REQUIRE(copies && copy_stride && d > 0, "accum_layout: bad arguments");
  *copies = kAccumCopies;
  *copy_stride = align_up((uint64_t)d, 128);
  return 0;
}
extern "C" int gget_op_rmsnorm_bwd_ls_drop(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx,
                                           float* dw_accum, const void* y, const void* lam, void* dsc, float* dlam_accum, int T, int d,
                                           float elem_p, uint32_t elem_seed, const int32_t* elem_rows, float path_rate, uint32_t path_seed,
                                           int path_S, const int32_t* path_row_b, void* stream) {
  GGET_REQUIRE(dy && x && w && rstd && dx && dw_accum && y && dsc && T >= 0, "rmsnorm_bwd_ls: null argument");
  GGET_REQUIRE(d > 0 && d % 8 == 0 && d <= 2048, "rmsnorm_bwd_ls: d=%d unsupported", d);
  if (int e = check_masks("rmsnorm_bwd_ls", elem_p, path_rate, path_S, path_row_b)) return e;
  return k_rmsnorm_bwd_ls((const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)w, rstd, (const bf16_t*)dres, (bf16_t*)dx, dw_accum, (const bf16_t*)y,
                          (const bf16_t*)lam, (bf16_t*)dsc, dlam_accum, T, d, path_arg(path_rate, path_seed, path_S, path_row_b),
                          elem_drop(elem_p, elem_seed, elem_rows), (hipStream_t)stream);
}
extern "C" int gget_op_rmsnorm_bwd_ls(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx,
                                      float* dw_accum, const void* y, const void* lam, void* dsc, float* dlam_accum, int T, int d,
                                      void* stream) {
  return gget_op_rmsnorm_bwd_ls_drop(dy, x, w, rstd, dres, dx, dw_accum, y, lam, dsc, dlam_accum, T, d, 0.f, 0u, nullptr, 0.f, 0u, 1, nullptr,
                                     stream);
}
extern "C" int gget_op_ce_full(const void* logits, int ld, const int32_t* labels, const int32_t* sel_tok, const float* sample_wgt, int S,
                               const int32_t* n_rows_dev, int n_rows_cap, int V, float* loss_sum, void* dlogits, float scale_base,
                               int mean_over_rows, float* loss_out, float focal_gamma, float* loss_part, int loss_part_cap, void* stream) {
  GGET_REQUIRE(logits && labels && loss_sum && n_rows_cap >= 0 && V >= 1 && ld >= V, "ce_full: bad arguments");
  GGET_REQUIRE(!sample_wgt || (sel_tok && S >= 1), "ce_full: sample weights need sel_tok and S >= 1");
  return k_ce_fwd_bwd(logits, ld, labels, sel_tok, sample_wgt, S, n_rows_dev, n_rows_cap, V, loss_sum, dlogits, scale_base, mean_over_rows,
                      loss_out, (hipStream_t)stream, focal_gamma, loss_part, loss_part_cap);
}
// fine-tune heads and task losses: the launchers of csrc/kernels.h as they are (no arithmetic here)
extern "C" int gget_op_score_fwd(const void* hidden, const int32_t* pool_row, const void* w, const void* bias, float* logits,
                                 void* pooled_h, int B, int C, int d, void* stream) {
  GGET_REQUIRE(hidden && pool_row && w && logits && B > 0 && C > 0 && d > 0, "score_fwd: null argument or empty shape");
  return k_score_fwd(hidden, pool_row, w, bias, logits, pooled_h, B, C, d, (hipStream_t)stream);
}
extern "C" int gget_op_score_bwd(const float* dlogits, const void* hidden, const int32_t* pool_row, const void* w, float* dw,
                                 float* dbias, void* dhidden, int B, int C, int d, void* stream) {
  GGET_REQUIRE(dlogits && hidden && pool_row && w && dw && dhidden && B > 0 && C > 0 && d > 0, "score_bwd: null argument or empty shape");
  return k_score_bwd(dlogits, hidden, pool_row, w, dw, dbias, dhidden, B, C, d, (hipStream_t)stream);
}
extern "C" int gget_op_tok_score_fwd(const void* hidden, const void* w, const void* bias, float* logits, int T, int C, int d,
                                     void* stream) {
  GGET_REQUIRE(hidden && w && logits && T >= 0 && C > 0, "tok_score_fwd: null argument or empty shape");
  return k_tok_score_fwd(hidden, w, bias, logits, T, C, d, (hipStream_t)stream);
}
extern "C" int gget_op_tok_intra_fwd(const void* hidden, const int32_t* row_start, const int64_t* cls_idx, float* logits, int B, int C,
                                     int d, void* stream) {
  GGET_REQUIRE(hidden && row_start && cls_idx && logits && B >= 0, "tok_intra_fwd: null argument or empty shape");
  return k_tok_intra_fwd(hidden, row_start, cls_idx, logits, B, C, d, (hipStream_t)stream);
}
extern "C" int gget_op_tok_intra_bwd(const float* dl, const float* stat, const void* hidden, const int32_t* row_start,
                                     const int64_t* cls_idx, void* dhidden, int B, int C, int d, void* stream) {
  GGET_REQUIRE(dl && stat && hidden && row_start && cls_idx && dhidden && B >= 0, "tok_intra_bwd: null argument or empty shape");
  return k_tok_intra_bwd(dl, stat, hidden, row_start, cls_idx, dhidden, B, C, d, (hipStream_t)stream);
}
extern "C" int gget_op_tok_ce(const float* logits, const int64_t* labels, float* dl, float* stat, float* loss_out, int T, int C,
                              const int32_t* rows_map, int n_logical, void* stream) {
  GGET_REQUIRE(logits && labels && dl && stat && loss_out && T >= 0 && C > 0, "tok_ce: null argument or empty shape");
  return k_tok_ce(logits, labels, dl, stat, loss_out, T, C, (hipStream_t)stream, rows_map, n_logical);
}
extern "C" int gget_op_tok_score_bwd(const float* dl, const float* stat, const void* hidden, const void* w, float* dw, float* dbias,
                                     void* dhidden, int T, int C, int d, void* stream) {
  GGET_REQUIRE(dl && stat && hidden && w && dw && dhidden && T >= 0 && C > 0, "tok_score_bwd: null argument or empty shape");
  GGET_REQUIRE(d % 64 == 0 && d > 0 && d <= 1024, "token-level head: d=%d unsupported", d);
  return k_tok_score_bwd(dl, stat, hidden, w, dw, dbias, dhidden, T, C, d, (hipStream_t)stream);
}
extern "C" int gget_op_task_loss(const float* logits, const void* labels, const float* sample_wgt, int problem, int B, int C,
                                 float* loss_out, float* dlogits, void* stream) {
  GGET_REQUIRE(logits && labels && loss_out && dlogits && B > 0 && C > 0, "task_loss: null argument or empty shape");
  GGET_REQUIRE(problem == GGET_PROBLEM_SINGLE_LABEL || problem == GGET_PROBLEM_REGRESSION_L1 || problem == GGET_PROBLEM_REGRESSION_MSE ||
                   problem == GGET_PROBLEM_MULTI_LABEL,
               "task_loss: problem type %d has a kernel of its own", problem);
  return k_task_loss(logits, labels, sample_wgt, problem, B, C, loss_out, dlogits, (hipStream_t)stream);
}
extern "C" int gget_op_auc_loss(const float* logits, const int64_t* labels, int B, int C, int num_neg, uint32_t seed, float* loss_out,
                                float* dlogits, int32_t* lists, void* stream) {
  GGET_REQUIRE(logits && labels && loss_out && dlogits && lists, "auc_loss: null argument");
  return k_auc_loss(logits, labels, B, C, num_neg, seed, loss_out, dlogits, lists, (hipStream_t)stream);
}
extern "C" int gget_op_pool_rows(const void* hidden, const int32_t* pool_row, void* out, int B, int d, void* stream) {
  GGET_REQUIRE(hidden && pool_row && out && B > 0 && d > 0, "pool_rows: null argument or empty shape");
  return k_pool_rows(hidden, pool_row, out, B, d, (hipStream_t)stream);
}
extern "C" int gget_op_scatter_rows_f32(const float* src, const int32_t* pool_row, void* dhidden, int B, int d, void* stream) {
  GGET_REQUIRE(src && pool_row && dhidden && B > 0 && d > 0, "scatter_rows_f32: null argument or empty shape");
  return k_scatter_rows_f32(src, pool_row, dhidden, B, d, (hipStream_t)stream);
}
// (the _drop entries: head dropout from (elem_p, elem_seed, elem_rows) through elem_drop - the head kernels key the mask by the
//  pooled row b and never read elem_rows; the plain entries are evaluation mode: they call the _drop ones with the dropout off)
extern "C" int gget_op_head_linear_fwd_drop(const void* x, void* a, const void* w, const void* bias, void* y, float* y32, int B, int Din,
                                            int Dout, int layer, float elem_p, uint32_t elem_seed, const int32_t* elem_rows, void* stream) {
  GGET_REQUIRE(x && a && w && y && B > 0 && Din > 0 && Dout > 0, "head_linear_fwd: null argument or empty shape");
  GGET_REQUIRE(elem_p < 1.f, "head_linear_fwd: bad mask arguments");
  return k_head_linear_fwd(x, a, w, bias, y, y32, B, Din, Dout, layer, elem_drop(elem_p, elem_seed, elem_rows), (hipStream_t)stream);
}
extern "C" int gget_op_head_linear_fwd(const void* x, void* a, const void* w, const void* bias, void* y, float* y32, int B, int Din,
                                       int Dout, int layer, void* stream) {
  return gget_op_head_linear_fwd_drop(x, a, w, bias, y, y32, B, Din, Dout, layer, 0.f, 0u, nullptr, stream);
}
extern "C" int gget_op_head_linear_bwd_drop(const float* dy, const void* x, const void* a, const void* w, float* dw, float* dbias, float* dx,
                                            int B, int Din, int Dout, int layer, float elem_p, uint32_t elem_seed, const int32_t* elem_rows,
                                            void* stream) {
  GGET_REQUIRE(dy && x && a && w && dw && dx && B > 0 && Din > 0 && Dout > 0, "head_linear_bwd: null argument or empty shape");
  GGET_REQUIRE(elem_p < 1.f, "head_linear_bwd: bad mask arguments");
  return k_head_linear_bwd(dy, x, a, w, dw, dbias, dx, B, Din, Dout, layer, elem_drop(elem_p, elem_seed, elem_rows), (hipStream_t)stream);
}
extern "C" int gget_op_head_linear_bwd(const float* dy, const void* x, const void* a, const void* w, float* dw, float* dbias, float* dx,
                                       int B, int Din, int Dout, int layer, void* stream) {
  return gget_op_head_linear_bwd_drop(dy, x, a, w, dw, dbias, dx, B, Din, Dout, layer, 0.f, 0u, nullptr, stream);
}
// batch layout and SMTP-head index kernels: the launchers of csrc/kernels.h as they are (tests/test_gpu_plan.py)
extern "C" int gget_op_lengths(const int64_t* mask, const int64_t* ids, int ldF, int pad_id, int32_t* key_len, int32_t* pool_row, int B,
                               int S, void* stream) {
  GGET_REQUIRE((key_len || pool_row) && (!pool_row || ids) && B > 0 && S > 0 && (!ids || ldF >= 1), "lengths: null argument or empty shape");
  return k_lengths(mask, ids, ldF, pad_id, key_len, pool_row, B, S, (hipStream_t)stream);
}
extern "C" int gget_op_sum_lengths(const int32_t* key_len, int B, int32_t* out, void* stream) {
  GGET_REQUIRE(key_len && out && B > 0, "sum_lengths: null argument or empty shape");
  return k_sum_lengths(key_len, B, out, (hipStream_t)stream, nullptr);
}
extern "C" int gget_op_varlen_plan(const int64_t* ids, int ldF, int F, const int64_t* pos, int32_t* key_len, int32_t* pool_row, int32_t* cu,
                                   int64_t* ids_c, int64_t* pos_c, int32_t* row_b, int32_t* pad2c, int32_t* c2p, int32_t* status, int B,
                                   int S, int tc, int t_rows, int pad_id, int32_t* long_list, void* stream) {
  GGET_REQUIRE(ids && key_len && cu && ids_c && pos_c && row_b && pad2c && c2p && status, "varlen_plan: null argument");
  GGET_REQUIRE(B > 0 && S > 0 && F >= 1 && ldF >= F && tc >= 0 && t_rows >= tc, "varlen_plan: bad shape B %d S %d F %d ldF %d tc %d t_rows %d", B, S,
               F, ldF, tc, t_rows);
  return k_varlen_plan(ids, ldF, F, pos, key_len, pool_row, cu, ids_c, pos_c, row_b, pad2c, c2p, status, B, S, tc, t_rows, pad_id,
                       (hipStream_t)stream, long_list);
}
extern "C" int gget_op_rows_to_grid(const void* src, const int32_t* pad2c, void* out, int64_t n_pos, int d, void* stream) {
  GGET_REQUIRE(src && pad2c && out && n_pos >= 0 && d > 0 && d % 8 == 0, "rows_to_grid: null argument or bad shape (d must be a multiple of 8)");
  return k_rows_to_grid(src, pad2c, out, (long)n_pos, d, (hipStream_t)stream);
}
extern "C" uint64_t gget_op_head_compact_ws_bytes(int T) { return T > 0 ? (uint64_t)k_head_compact_ws_bytes(T) : 0; }
extern "C" int gget_op_head_compact(const int64_t* labels, int T, int n, int32_t* cnt, int32_t* m_off, int32_t* l_off, int32_t* counts,
                                    int32_t* row_idx, int32_t* sel_src, int32_t* sel_label, int32_t* sel_tok, int32_t* ws,
                                    int32_t* slot_hist, void* stream) {
  GGET_REQUIRE(cnt && m_off && l_off && counts && row_idx && sel_src && sel_label && sel_tok && ws, "head_compact: null argument");
  GGET_REQUIRE(T > 0 && n >= 1, "head_compact: bad shape T %d n %d", T, n);
  return k_head_compact(labels, T, n, cnt, m_off, l_off, counts, row_idx, sel_src, sel_label, sel_tok, ws, slot_hist, (hipStream_t)stream);
}
extern "C" int gget_op_head_slot_sort(const int32_t* sel_src, const int32_t* row_idx, const int32_t* lm_count, int32_t* slot_state,
                                      int32_t* a_tok, int32_t* a_cell, int32_t* c_l, int32_t* cellpos, int32_t* tile_off, int32_t* total_p,
                                      int cap, int n, int64_t slot_elems, int tile_rows, void* stream) {
  GGET_REQUIRE(sel_src && row_idx && lm_count && slot_state && a_tok && a_cell && c_l && cellpos && tile_off && total_p,
               "head_slot_sort: null argument");
  GGET_REQUIRE(cap > 0 && n >= 1 && tile_rows > 0 && slot_elems >= 0, "head_slot_sort: bad shape cap %d n %d tile_rows %d", cap, n, tile_rows);
  return k_head_slot_sort(sel_src, row_idx, lm_count, slot_state, a_tok, a_cell, c_l, cellpos, tile_off, total_p, cap, n, (long)slot_elems,
                          tile_rows, (hipStream_t)stream);
}
extern "C" int gget_op_head_cell_sum(const void* dxs, const int32_t* cellpos, const int32_t* cnt, const int32_t* l_off, const int32_t* pad2c,
                                     void* dhid, int TP, int d, int pad_row, void* stream) {
  GGET_REQUIRE(dxs && cellpos && cnt && l_off && dhid && TP > 0 && d > 0 && d % 8 == 0 && pad_row >= 0,
               "head_cell_sum: null argument or bad shape (d must be a multiple of 8)");
  return k_head_cell_sum(dxs, cellpos, cnt, l_off, pad2c, dhid, TP, d, pad_row, (hipStream_t)stream);
}
extern "C" int gget_op_gather_rows(const void* src, const int32_t* idx, const int32_t* count, void* dst, int cap, int d, int scatter,
                                   void* stream) {
  GGET_REQUIRE(src && idx && count && dst && cap >= 0 && d > 0 && d % 8 == 0, "gather_rows: null argument or bad shape (d must be a multiple of 8)");
  return k_gather_rows(src, idx, count, dst, cap, d, scatter, (hipStream_t)stream);
}
extern "C" int gget_op_gather_rows_remap(const void* src, int32_t* idx, const int32_t* count, const int32_t* pad2c, void* dst, int cap, int d,
                                         int pad_row, int32_t* status, void* stream) {
  GGET_REQUIRE(src && idx && count && pad2c && dst && cap >= 0 && d > 0 && d % 8 == 0 && pad_row >= 0,
               "gather_rows_remap: null argument or bad shape (d must be a multiple of 8)");
  return k_gather_rows_remap(src, idx, count, pad2c, dst, cap, d, pad_row, status, (hipStream_t)stream);
}
extern "C" int gget_op_sample_mask_wgt(const int64_t* labels, float* w, int B, int cells, void* stream) {
  GGET_REQUIRE(labels && w && B >= 0 && cells >= 1, "sample_mask_wgt: null argument or empty shape");
  return k_sample_mask_wgt(labels, w, B, cells, (hipStream_t)stream);
}
extern "C" int gget_op_raw_blend(const float* raw, const int64_t* labels, int n, int first_only, const void* tok, void* out, int32_t* flag,
                                 int T, int e, const int32_t* rows_map, int n_logical, void* stream) {
  GGET_REQUIRE(raw && tok && out && flag && T >= 0 && e > 0 && (!labels || n >= 1) && (!rows_map || n_logical >= 0),
               "raw_blend: null argument or bad shape");
  return k_raw_blend(raw, labels, n, first_only != 0, tok, out, flag, T, e, (hipStream_t)stream, rows_map, n_logical);
}
extern "C" int gget_op_raw_tok_grad(const void* dx, const int32_t* flag, float* dtok, int T, int e, void* stream) {
  GGET_REQUIRE(dx && flag && dtok && T >= 0 && e > 0, "raw_tok_grad: null argument or empty shape");
  return k_raw_tok_grad(dx, flag, dtok, T, e, (hipStream_t)stream);
}
// test-only entries of the step replay (tests/_step_replay.py): the launchers as the engine's step calls them, no arithmetic here
extern "C" int gget_op_attn_bwd_rotated(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len,
                                        const int32_t* row_base, void* dqkv, float* delta_ws, int B, int S, int H, int causal,
                                        const float* cos_tab, const float* sin_tab, const int64_t* position_ids, float dropout_p,
                                        uint32_t dropout_seed, void* dq_ws, uint64_t dq_slab_stride, const int32_t* long_list, void* stream) {
  GGET_REQUIRE(qkv && dout && lse && dqkv && cos_tab && sin_tab, "attn_bwd_rotated: null argument");
  GGET_REQUIRE(!long_list || row_base, "attn_bwd_rotated: the list of long samples belongs to the var-len layout");
  return k_attn_bwd(qkv, out, dout, lse, key_len, dqkv, delta_ws, B, S, H, causal, cos_tab, sin_tab, position_ids, /*qk_rotated=*/1, dropout_p,
                    dropout_seed, (hipStream_t)stream, nullptr, nullptr, row_base, dq_ws, (size_t)dq_slab_stride, long_list);
}
extern "C" int gget_op_convert_segments(const float* scratch, void* grads, const uint64_t* segs_dev, int nseg, void* stream) {
  GGET_REQUIRE(scratch && grads && (segs_dev || nseg == 0) && nseg >= 0, "convert_segments: bad arguments");
  static_assert(sizeof(GgetSegment) == 5 * sizeof(uint64_t), "gget_op_convert_segments: a segment is five uint64 (include/gget.h)");
  return k_convert_segments(scratch, grads, reinterpret_cast<const GgetSegment*>(segs_dev), nseg, (hipStream_t)stream);
}
extern "C" int gget_op_gemm_indexed(int mode, const void* A, const void* B, void* C, int M_cap, int N, int K, int lda, int ldb, int ldc,
                                    const int32_t* m_dev, const int32_t* a_rows, const int32_t* b_tile_off, int b_tile_rows,
                                    const int32_t* c_rows, void* stream) {
  GGET_REQUIRE(A && B && C && M_cap >= 0 && N > 0 && K > 0, "gemm_indexed: null argument or empty shape");
  if (!a_rows && !b_tile_off)
    return gget_gemm_single(mode, GGET_EPI_NONE, A, B, C, nullptr, M_cap, N, K, lda, ldb, ldc, m_dev, nullptr, 1, (hipStream_t)stream, false,
                            c_rows);
  GGET_REQUIRE(b_tile_rows == 128 || b_tile_rows == 256, "gemm_indexed: b_tile_rows %d is neither 128 nor 256", b_tile_rows);
  GemmGroup g;
  memset(&g, 0, sizeof(g));
  g.count = 1;
  GemmProblem& p = g.p[0];
  p.A = static_cast<const bf16_t*>(A); p.B = static_cast<const bf16_t*>(B); p.C = C;
  p.M = M_cap; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.m_dev = m_dev;
  p.a_rows = a_rows; p.b_tile_off = b_tile_off; p.c_rows = c_rows;
  p.b_tile_rows = b_tile_rows;
  return gget_gemm_launch(mode, GGET_EPI_NONE, g, 1, (hipStream_t)stream);
}
