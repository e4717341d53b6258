// Self-attention core for head width 32 on gfx950 MFMA (32x32x16 bf16): the model sizes tiny6 (d 128, 4 heads) and small12 (d 384,
// 12 heads) of the reference's launch scripts, whose hf Llama layers run head_dim = hidden_size / num_attention_heads = 32.
//   P = softmax_fp32(Q K^T * 32^-1/2 + mask) ; O = bf16(P) V, bidirectional or causal
// qkv is [rows, 3d] (q | k | v, head h at column h * 32) with q and k ALREADY rotated (the engine's layout: at this width the q|k|v
// projection leaves its fp32 accumulators in a scratch buffer and rope32_f32_kernel rotates the q and k columns on the way to bf16, one
// rounding; rope32_kernel is the in-place operator on bf16 rows); the tables handed to the backward only rotate dq / dk back.
//
// Formulation: the one of attention.hip (scores TRANSPOSED, S^T[key][query] = K_tile Q_tile^T, so a lane owns one query column and the
// softmax statistics are lane-local; the bf16 P^T registers are the B operand of O^T[dh][query] += V^T[dh][key] P^T[key][query]; V^T,
// K^T, Q^T, dO^T through ds_read_b64_tr_b16; backward = dQ kernel per query tile + dK/dV kernel per key tile, P recomputed from the
// saved log-sum-exp, delta = sum_k m p dP in fp32 by a first walk of the dQ kernel over its key tiles, no atomics).  With dh = 32 the
// score product is two k-steps and the output accumulator ONE 32x32 tile.
// A compact, correctness-first family: one wave per 32-row tile, every tile staged by its own wave, the mask evaluated on every tile,
// any S by looping over key tiles.  No S-keyed variants, no LDS-DMA, no per-sample fused launch.
//
// Scale: 32^-1/2 is not a power of two.  The forward and the probability recomputations use ONE fp32 constant, fl(32^-1/2 * log2 e),
// inside p = exp2(fma(s, c, -m2)) (scores carried in the log2 domain as in attention.hip); dS is multiplied by the fp32 constant
// fl(32^-1/2).  lse is the natural log ((m2 + log2 l) / log2 e).
#include <stdlib.h>
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "attn_common.h"

#define LDS_AS __attribute__((address_space(3)))

namespace {

constexpr float kScale32 = 0.17677669529663687f;                         // 32^-1/2
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kScaleL2_32 = (float)(0.17677669529663687 * 1.4426950408889634);   // one rounding of the product
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// [32 rows][64 B] tile: the 16-byte chunk index is XORed with (row >> 2) & 3, so that the ds_read_b128 of one chunk over 16
// consecutive rows meets 16 distinct 16-byte slots; the four rows of one transposing read share a chunk permutation.
__device__ __forceinline__ int swz32(int row, int byte_in_row) {
  return row * 64 + ((((byte_in_row >> 4) ^ ((row >> 2) & 3)) << 4) | (byte_in_row & 15));
}

// [32 rows][32 dh] bf16 tile -> LDS, one wave: unconditional loads of clamped rows, rows >= row_lim zero-filled (attn_common.h)
__device__ __forceinline__ void load_tile32(unsigned char* lds, const bf16_t* __restrict__ base, int r0, int row_lim, size_t pitch,
                                            int lane) {
  uint4 v[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = lane + i * 64;
    const int row = c >> 2, ch = c & 3;
    v[i] = *reinterpret_cast<const uint4*>(base + (size_t)clamp_row(r0 + row, row_lim) * pitch + ch * 8);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = lane + i * 64;
    const int row = c >> 2, ch = c & 3;
    *reinterpret_cast<uint4*>(lds + swz32(row, ch * 16)) = zero_if(r0 + row >= row_lim, v[i]);
  }
}
// MFMA operand whose row / column index is the tile row (lane & 31) and whose k-chunk is dh [16 s + 8 hi, + 8), s = 0, 1
__device__ __forceinline__ bf16x8_t frag_rows32(const unsigned char* lds, int s, int lane) {
  const uint4 v = *reinterpret_cast<const uint4*>(lds + swz32(lane & 31, (2 * s + (lane >> 5)) * 16));
  return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ bf16x8_t frag_global32(const bf16_t* __restrict__ base, int row, int row_lim, size_t pitch, int s,
                                                  int lane) {
  const uint4 v = *reinterpret_cast<const uint4*>(base + (size_t)clamp_row(row, row_lim) * pitch + 16 * s + (lane >> 5) * 8);
  return __builtin_bit_cast(bf16x8_t, zero_if(row >= row_lim, v));
}
// transposed operand: MFMA row = dh (lane & 31), k = tile rows {16 j + 4 hi + (e & 3) + 8 (e >> 2)} - the order of acc_to_b
__device__ __forceinline__ bf16x8_t frag_tr32(const unsigned char* lds, int j, int lane) {
  const int li = lane & 15, g = lane >> 4, hi = lane >> 5;
  const int colb = ((g & 1) * 16 + (li & 3) * 4) * 2;
  const int ra = 16 * j + 4 * hi + (li >> 2);
  const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4_t*)(lds + swz32(ra, colb)));
  const bf16x4_t up = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4_t*)(lds + swz32(ra + 8, colb)));
  bf16x8_t o;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3];
  o[4] = up[0]; o[5] = up[1]; o[6] = up[2]; o[7] = up[3];
  return o;
}
// store a transposed accumulator (O^T[dh][row]) as row-major bf16 [row][32 dh]; lane owns row (lane & 31).  Registers [4 rr, 4 rr + 4)
// are dh 8 rr + 4 hi .. + 3 of its row; the two lanes of a row trade pieces (v_permlane32_swap) so that the hi = 0 lane stores the 16
// bytes dh [8 rr, 8 rr + 8) of the even rr and the hi = 1 lane those of the odd rr.  Both lanes of a row are active together.
__device__ __forceinline__ void store_t32(bf16_t* __restrict__ dst_row, const f32x16_t& a, float mul, int hi) {
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    const int e = 2 * pr, o = 2 * pr + 1;
    const unsigned e0 = pack2bf(a[4 * e + 0] * mul, a[4 * e + 1] * mul), e1 = pack2bf(a[4 * e + 2] * mul, a[4 * e + 3] * mul);
    const unsigned o0 = pack2bf(a[4 * o + 0] * mul, a[4 * o + 1] * mul), o1 = pack2bf(a[4 * o + 2] * mul, a[4 * o + 3] * mul);
    const hw_u32x2_t w0 = __builtin_amdgcn_permlane32_swap(e0, o0, false, false);
    const hw_u32x2_t w1 = __builtin_amdgcn_permlane32_swap(e1, o1, false, false);
    uint4 v;
    v.x = w0[0]; v.y = w1[0]; v.z = w0[1]; v.w = w1[1];
    *reinterpret_cast<uint4*>(dst_row + 8 * (hi ? o : e)) = v;
  }
}
// gradient of a rotated row back to the un-rotated one, x = R(-theta) x', pairing j <-> j + 16: registers [4 rr, 4 rr + 4), rr = 0, 1
// (dh 8 rr + 4 hi .. + 3) pair with registers [4 (rr + 2), ..) of the same lane.  Tables [max_pos][16].
__device__ __forceinline__ void unrope_acc32(f32x16_t& a, const Rope& R, int pos, int hi) {
  if (!R.cos_tab) return;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int j0 = 8 * rr + 4 * hi;
    const float4 c = *reinterpret_cast<const float4*>(R.cos_tab + (size_t)pos * 16 + j0);
    const float4 sn = *reinterpret_cast<const float4*>(R.sin_tab + (size_t)pos * 16 + j0);
    const float cc[4] = {c.x, c.y, c.z, c.w}, ss[4] = {sn.x, sn.y, sn.z, sn.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = a[4 * rr + e], up = a[4 * (rr + 2) + e];
      a[4 * rr + e] = lo * cc[e] + up * ss[e];
      a[4 * (rr + 2) + e] = up * cc[e] - lo * ss[e];
    }
  }
}

// the per-lane inclusive key range [qlo, qhi] of query row qrow and the wave's union [ulo, uhi] (key tiles outside are skipped)
struct Keys32 { int qlo, qhi, ulo, uhi; };
template <bool PK>
__device__ __forceinline__ Keys32 query_keys(const KeyRange& KR, int b, int S, int SL, int qrow) {
  Keys32 k;
  k.qlo = 0; k.qhi = min(KR.key_len ? KR.key_len[b] : S, S) - 1;
  k.ulo = 0; k.uhi = k.qhi;
  if (PK) {
    const bool v = qrow < SL;
    const size_t i = (size_t)b * S + min(qrow, S - 1);
    k.qlo = v ? max(KR.lo[i], 0) : 0;
    k.qhi = v ? min(KR.hi[i], S - 1) : -1;
    k.ulo = wave_imin(k.qhi >= k.qlo ? k.qlo : S);
    k.uhi = wave_imax(k.qhi >= k.qlo ? k.qhi + 1 : 0) - 1;
  }
  return k;
}

// ------------------------------------------------------------------------------------------------
// forward: block = one wave = one 32-query tile of one (batch, head); grid (ceil(S / 32), H, B)
template <bool PK>
__global__ void __launch_bounds__(64) attn32_fwd_kernel(const bf16_t* __restrict__ qkv, KeyRange KR, bf16_t* __restrict__ out,
                                                        float* __restrict__ lse, int B, int S, int H, int causal, Drop D) {
  __shared__ __attribute__((aligned(16))) unsigned char kt[2048];
  __shared__ __attribute__((aligned(16))) unsigned char vt[2048];
  const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  // var-len token layout (KR.row_base): sample b owns rows [rb, rb + SL) of the token-major buffers; padded layout: rb = b * S, SL = S
  const int rb = KR.row_base ? KR.row_base[b] : b * S;
  const int SL = KR.row_base ? min(KR.key_len[b], S) : S;
  const int q0 = blockIdx.x * 32;
  if (q0 >= SL) return;     // (var-len layout: no rows of this sample in the block)
  const int d = H * 32;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 32;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const int qrow = q0 + l31;
  const Keys32 Q = query_keys<PK>(KR, b, S, SL, qrow);
  bf16x8_t qf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) qf[s] = frag_global32(qb, qrow, SL, pitch, s, lane);
  f32x16_t o = zero16();
  float m = -INFINITY, l = 0.f;
  const unsigned dbase = drop_base(D, b * H + h, qrow, 0);
  const int kend = min(Q.uhi + 1, causal ? q0 + 32 : SL);     // (wave-uniform)
  for (int k0 = 0; k0 < kend; k0 += 32) {
    if (k0 + 31 < Q.ulo) continue;
    __syncthreads();  // previous tile fully consumed
    load_tile32(kt, kb, k0, SL, pitch, lane);
    load_tile32(vt, vb, k0, SL, pitch, lane);
    __syncthreads();
    f32x16_t sc = zero16();
#pragma unroll
    for (int s = 0; s < 2; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows32(kt, s, lane), qf[s], sc, 0, 0, 0);
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + acc_row(r, hi);
      const bool ok = key >= Q.qlo && key <= Q.qhi && (!causal || key <= qrow);
      sc[r] = ok ? sc[r] : -INFINITY;
      mx = fmaxf(mx, sc[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx * kScaleL2_32);     // the constant is positive: max commutes with the scaling
    const bool dead = m_new == -INFINITY;
    const float alpha = dead ? 1.f : fast_exp2(m - m_new);
    const float nm = dead ? 0.f : -m_new;
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = fast_exp2(fmaf(sc[r], kScaleL2_32, nm));   // masked scores are -inf -> 0
      rs += p;                                                   // softmax normaliser: before dropout
      sc[r] = p * drop_mul_x(D, dbase + (unsigned)((k0 + acc_row(r, hi)) >> 1) * 0xC2B2AE3Du, r & 1);   // (acc_row parity = r & 1)
    }
    rs += __shfl_xor(rs, 32, 64);
    l = l * alpha + rs;
    m = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] *= alpha;
    o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr32(vt, 0, lane), acc_to_b(sc, 0), o, 0, 0, 0);
    o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr32(vt, 1, lane), acc_to_b(sc, 1), o, 0, 0, 0);
  }
  if (qrow < SL) {
    const float inv = l > 0.f ? 1.f / l : 0.f;   // (the keep scale 1 / (1 - p) is already folded into the dropped P)
    store_t32(out + ((size_t)rb + qrow) * d + h * 32, o, inv, hi);
    if (hi == 0) lse[((size_t)b * H + h) * S + qrow] = l > 0.f ? (m + log2f(l)) * (1.0f / kLog2e) : 0.f;   // natural log
  }
}

// dQ^T[dh][q] = sum_keys K^T[dh][key] dS^T[key][q],  dS^T = P^T (m dP^T - delta_q) * 32^-1/2; also leaves delta_q in `delta`.
// delta_q = sum_k m p dP over the query's allowed keys, in fp32 from the same p and dP that form dS (a first walk over the key tiles): the
// row sum of dS is then zero up to fp32 rounding.  Formed as rowsum(dO o out) from the bf16 out, its 2^-9 rounding leaves delta_err * p_k in
// every dS_k - for the near-uniform softmax of a freshly initialised model, where dS is what survives the cancellation in m dP - delta, that
// was 6 % of the first layer's q-projection gradient at six layers.  `out` is not read.
template <bool PK>
__global__ void __launch_bounds__(64) attn32_bwd_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out,
                                                           const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                           float* __restrict__ delta, KeyRange KR, bf16_t* __restrict__ dqkv, int B,
                                                           int S, int H, int causal, Rope R, Drop D) {
  __shared__ __attribute__((aligned(16))) unsigned char kt[2048];
  __shared__ __attribute__((aligned(16))) unsigned char vt[2048];
  const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const int rb = KR.row_base ? KR.row_base[b] : b * S;
  const int SL = KR.row_base ? min(KR.key_len[b], S) : S;
  const int q0 = blockIdx.x * 32;
  if (q0 >= SL) return;
  const int d = H * 32;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 32;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const bf16_t* dob = dout + (size_t)rb * d + h * 32;
  const int qrow = q0 + l31;
  const Keys32 Q = query_keys<PK>(KR, b, S, SL, qrow);
  bf16x8_t qf[2], dof[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    qf[s] = frag_global32(qb, qrow, SL, pitch, s, lane);
    dof[s] = frag_global32(dob, qrow, SL, (size_t)d, s, lane);
  }
  const size_t sidx = ((size_t)b * H + h) * S + min(qrow, S - 1);
  const float nlse2 = -lse[sidx] * kLog2e;
  const unsigned dbase = drop_base(D, b * H + h, qrow, 0);
  const int kend = min(Q.uhi + 1, causal ? q0 + 32 : SL);
  // first walk: delta_q = sum_k m p dP (the lane sums its 16 keys of every tile; the row's other keys sit in lane ^ 32)
  float dl = 0.f;
  for (int k0 = 0; k0 < kend; k0 += 32) {
    if (k0 + 31 < Q.ulo) continue;
    __syncthreads();
    load_tile32(kt, kb, k0, SL, pitch, lane);
    load_tile32(vt, vb, k0, SL, pitch, lane);
    __syncthreads();
    f32x16_t dp = zero16(), sc = zero16();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows32(vt, s, lane), dof[s], dp, 0, 0, 0);
      sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows32(kt, s, lane), qf[s], sc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + acc_row(r, hi);
      float p = fast_exp2(fmaf(sc[r], kScaleL2_32, nlse2));
      p = (key >= Q.qlo && key <= Q.qhi && (!causal || key <= qrow) && qrow < SL) ? p : 0.f;
      dl = fmaf(p * drop_mul_x(D, dbase + (unsigned)(key >> 1) * 0xC2B2AE3Du, key & 1), dp[r], dl);
    }
  }
  dl += __shfl_xor(dl, 32, 64);
  if (hi == 0 && qrow < SL) delta[sidx] = dl;
  const float ndl = -dl;
  f32x16_t acc = zero16();
  for (int k0 = 0; k0 < kend; k0 += 32) {
    if (k0 + 31 < Q.ulo) continue;
    __syncthreads();
    load_tile32(kt, kb, k0, SL, pitch, lane);
    load_tile32(vt, vb, k0, SL, pitch, lane);
    __syncthreads();
    f32x16_t dp = zero16(), sc = zero16();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows32(vt, s, lane), dof[s], dp, 0, 0, 0);
      sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows32(kt, s, lane), qf[s], sc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + acc_row(r, hi);
      float p = fast_exp2(fmaf(sc[r], kScaleL2_32, nlse2));
      p = (key >= Q.qlo && key <= Q.qhi && (!causal || key <= qrow) && qrow < SL) ? p : 0.f;
      sc[r] = p * fmaf(dp[r], drop_mul_x(D, dbase + (unsigned)(key >> 1) * 0xC2B2AE3Du, key & 1), ndl) * kScale32;
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr32(kt, 0, lane), acc_to_b(sc, 0), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr32(kt, 1, lane), acc_to_b(sc, 1), acc, 0, 0, 0);
  }
  if (qrow < SL) {
    unrope_acc32(acc, R, rope_pos(R, b, qrow), hi);
    store_t32(dqkv + ((size_t)rb + qrow) * pitch + h * 32, acc, 1.f, hi);
  }
}

// dV^T[dh][key] = sum_q dO^T[dh][q] P[q][key] ; dK^T[dh][key] = sum_q Q^T[dh][q] dS[q][key]
// block = one wave = one 32-key tile; every 32-query Q tile, dO tile and their lse / delta / key ranges go through LDS
template <bool PK>
__global__ void __launch_bounds__(64) attn32_bwd_dkv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                            const float* __restrict__ lse, const float* __restrict__ delta,
                                                            KeyRange KR, bf16_t* __restrict__ dqkv, int B, int S, int H, int causal,
                                                            Rope R, Drop D) {
  __shared__ __attribute__((aligned(16))) unsigned char qt[2048];
  __shared__ __attribute__((aligned(16))) unsigned char dot_[2048];
  __shared__ float lse_s[32], dl_s[32];
  __shared__ int qlo_s[32], qhi_s[32];
  const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const int rb = KR.row_base ? KR.row_base[b] : b * S;
  const int SL = KR.row_base ? min(KR.key_len[b], S) : S;
  const int k0 = blockIdx.x * 32;
  if (k0 >= SL) return;
  const int d = H * 32;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 32;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const bf16_t* dob = dout + (size_t)rb * d + h * 32;
  const int klen = PK ? S : min(KR.key_len ? KR.key_len[b] : S, S);
  const int krow = k0 + l31;
  bf16x8_t kf[2], vf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    kf[s] = frag_global32(kb, krow, SL, pitch, s, lane);
    vf[s] = frag_global32(vb, krow, SL, pitch, s, lane);
  }
  f32x16_t dk = zero16(), dv = zero16();
  const unsigned dbase = drop_base(D, b * H + h, 0, (unsigned)krow >> 1);
  const bool key_ok = krow < klen;                 // right-padded rows: one key length per batch row
  if (k0 < klen) {
    for (int q0 = causal ? k0 : 0; q0 < SL; q0 += 32) {     // queries before the tile's first key never see it
      __syncthreads();
      load_tile32(qt, qb, q0, SL, pitch, lane);
      load_tile32(dot_, dob, q0, SL, (size_t)d, lane);
      if (lane < 32) {
        const int q = min(q0 + lane, S - 1);
        const bool v = q0 + lane < SL;
        lse_s[lane] = -lse[((size_t)b * H + h) * S + q] * kLog2e;
        // (var-len layout: the dQ kernel writes delta for the sample's own rows only; behind them the workspace holds whatever it held)
        dl_s[lane] = v ? -delta[((size_t)b * H + h) * S + q] : 0.f;
        if (PK) {
          qlo_s[lane] = v ? KR.lo[(size_t)b * S + q] : 0;
          qhi_s[lane] = v ? KR.hi[(size_t)b * S + q] : -1;
        }
      }
      __syncthreads();
      f32x16_t sc = zero16(), dp = zero16();
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows32(qt, s, lane), kf[s], sc, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows32(dot_, s, lane), vf[s], dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qi = acc_row(r, hi);
        const int q = q0 + qi;
        float p = fast_exp2(fmaf(sc[r], kScaleL2_32, lse_s[qi]));          // lse_s holds -lse * log2(e)
        const bool in_range = PK ? (krow >= qlo_s[qi] && krow <= qhi_s[qi]) : key_ok;
        p = (in_range && q < SL && (!causal || krow <= q)) ? p : 0.f;
        const float dm = drop_mul_x(D, dbase + (unsigned)q * 0x85EBCA77u, krow & 1);
        sc[r] = p * dm;                                    // dropped probabilities: what multiplied V in forward
        dp[r] = p * fmaf(dp[r], dm, dl_s[qi]) * kScale32;  // dl_s holds -delta
      }
      dv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr32(dot_, 0, lane), acc_to_b(sc, 0), dv, 0, 0, 0);
      dv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr32(dot_, 1, lane), acc_to_b(sc, 1), dv, 0, 0, 0);
      dk = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr32(qt, 0, lane), acc_to_b(dp, 0), dk, 0, 0, 0);
      dk = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr32(qt, 1, lane), acc_to_b(dp, 1), dk, 0, 0, 0);
    }
  }
  if (krow < SL) {
    bf16_t* row = dqkv + ((size_t)rb + krow) * pitch + h * 32;
    unrope_acc32(dk, R, rope_pos(R, b, krow), hi);
    store_t32(row + d, dk, 1.f, hi);
    store_t32(row + 2 * d, dv, 1.f, hi);
  }
}

// Attention weights (`output_attentions`): out[b, h, q, k] = bf16(m * exp(<q, k> * 32^-1/2 - lse[b, h, q])) on the allowed keys, 0
// elsewhere; out bf16 [B, H, S, S], every element written.  The rules of attn_probs_kernel (attention.hip): rows of padding queries are
// zero; packed rows lo <= k <= hi; m the forward's keep multiplier.  A lane owns a query row; registers [4 g, 4 g + 4) are four
// consecutive keys of it: one 8-byte store when vec != 0 (S % 4 == 0 and out 8-byte aligned), element stores otherwise.
template <bool PK>
__global__ void __launch_bounds__(64) attn32_probs_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ lse, KeyRange KR,
                                                          bf16_t* __restrict__ out, int B, int S, int H, int causal, Drop D, int vec) {
  __shared__ __attribute__((aligned(16))) unsigned char kt[2048];
  const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const int len = KR.key_len ? max(min(KR.key_len[b], S), 0) : S;
  const int rb = KR.row_base ? KR.row_base[b] : b * S;
  const int SL = KR.row_base ? len : S;      // rows the sample owns in the token-major buffer: no load leaves them (clamp_row)
  const int q0 = blockIdx.x * 32;
  const int d = H * 32;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 32;
  const bf16_t* kb = qb + d;
  const int qrow = q0 + l31;
  int qlo = 0, qhi = (qrow < len) ? len - 1 : -1;
  if (PK) {
    const bool v = qrow < S;
    const size_t i = (size_t)b * S + min(qrow, S - 1);
    qlo = v ? max(KR.lo[i], 0) : 0;
    qhi = v ? min(KR.hi[i], S - 1) : -1;
  }
  const bool row_live = qhi >= qlo;
  const int uhi = wave_imax(row_live ? qhi + 1 : 0) - 1;
  const int kend = SL > 0 ? min(uhi + 1, causal ? q0 + 32 : S) : 0;     // keys this wave computes (wave-uniform); zeros behind them
  bf16x8_t qf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) qf[s] = __builtin_bit_cast(bf16x8_t, make_uint4(0u, 0u, 0u, 0u));
  if (kend > 0) {
#pragma unroll
    for (int s = 0; s < 2; ++s) qf[s] = frag_global32(qb, qrow, SL, pitch, s, lane);
  }
  const float nlse2 = row_live ? -lse[((size_t)b * H + h) * S + qrow] * kLog2e : 0.f;
  const unsigned dbase = drop_base(D, b * H + h, qrow, 0);
  bf16_t* orow = out + ((size_t)(b * H + h) * S + min(qrow, S - 1)) * S;
  for (int k0 = 0; k0 < S; k0 += 32) {
    f32x16_t sc = zero16();
    if (k0 < kend) {
      __syncthreads();
      load_tile32(kt, kb, k0, SL, pitch, lane);
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 2; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows32(kt, s, lane), qf[s], sc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + acc_row(r, hi);
        const bool ok = key >= qlo && key <= qhi && (!causal || key <= qrow);
        const float p = fast_exp2(fmaf(sc[r], kScaleL2_32, nlse2)) * drop_mul_x(D, dbase + (unsigned)(key >> 1) * 0xC2B2AE3Du, key & 1);
        sc[r] = ok ? p : 0.f;
      }
    }
    if (qrow < S) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {      // registers [4 g, 4 g + 4) = keys k0 + 8 g + 4 hi .. + 3 of the lane's query
        const int k = k0 + 8 * g + 4 * hi;
        if (vec) {
          if (k < S) {
            uint2 v;
            v.x = pack2bf(sc[4 * g + 0], sc[4 * g + 1]);
            v.y = pack2bf(sc[4 * g + 2], sc[4 * g + 3]);
            *reinterpret_cast<uint2*>(orow + k) = v;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (k + e < S) orow[k + e] = f2bf(sc[4 * g + e]);
        }
      }
    }
  }
}

// RoPE in place on the q and k thirds of qkv [T, 3 d], head width 32: hf apply_rotary_pos_emb / rotate_half with the pair (j, j + 16),
// j < 16; tables [max_pos][16]; fp32 arithmetic, one rounding.  inverse = 1 applies the transpose rotation.
__global__ void __launch_bounds__(256) rope32_kernel(bf16_t* __restrict__ qkv, const float* __restrict__ cos_tab,
                                                     const float* __restrict__ sin_tab, const int64_t* __restrict__ position_ids, int T,
                                                     int S, int H, int inverse) {
  const int d = H * 32;
  const long total = (long)T * 2 * H * 2;
  for (long w = (long)blockIdx.x * 256 + threadIdx.x; w < total; w += (long)gridDim.x * 256) {
    const int j8 = (int)(w & 1);
    long r = w >> 1;
    const int h = (int)(r % H); r /= H;
    const int sec = (int)(r & 1);
    const int t = (int)(r >> 1);
    const int pos = position_ids ? (int)position_ids[t] : (t % S);
    bf16_t* p = qkv + (size_t)t * 3 * d + sec * d + h * 32 + j8 * 8;
    float a[8], b[8], c[8], s[8];
    unpack8(*reinterpret_cast<const uint4*>(p), a);
    unpack8(*reinterpret_cast<const uint4*>(p + 16), b);
    const float4* ct = reinterpret_cast<const float4*>(cos_tab + (size_t)pos * 16 + j8 * 8);
    const float4* stb = reinterpret_cast<const float4*>(sin_tab + (size_t)pos * 16 + j8 * 8);
    const float4 c0 = ct[0], c1 = ct[1], s0 = stb[0], s1 = stb[1];
    c[0] = c0.x; c[1] = c0.y; c[2] = c0.z; c[3] = c0.w; c[4] = c1.x; c[5] = c1.y; c[6] = c1.z; c[7] = c1.w;
    s[0] = s0.x; s[1] = s0.y; s[2] = s0.z; s[3] = s0.w; s[4] = s1.x; s[5] = s1.y; s[6] = s1.z; s[7] = s1.w;
    float oa[8], ob[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float sn = inverse ? -s[e] : s[e];
      oa[e] = a[e] * c[e] - b[e] * sn;
      ob[e] = b[e] * c[e] + a[e] * sn;
    }
    *reinterpret_cast<uint4*>(p) = pack8(oa);
    *reinterpret_cast<uint4*>(p + 16) = pack8(ob);
  }
}

// The engine's form: q | k | v of a layer as the projection GEMM's fp32 accumulators (src fp32 [T, 3 d], the fp32 slab epilogue) -> bf16
// qkv [T, 3 d] with the q and k columns rotated in fp32 and v copied, ONE rounding each - the cast points of the 64-wide projection,
// whose RoPE epilogue rotates the accumulators before their rounding.  (Rotating the rounded projection in place rounds q and k twice;
// the big-weight parity cases turn single bf16 flips of q / k into 1e-4 of loss.)
__global__ void __launch_bounds__(256) rope32_f32_kernel(const float* __restrict__ src, bf16_t* __restrict__ qkv, const float* __restrict__ cos_tab,
                                                         const float* __restrict__ sin_tab, const int64_t* __restrict__ position_ids, int T,
                                                         int S, int H) {
  const int d = H * 32;
  const long total = (long)T * 3 * H * 2;
  for (long w = (long)blockIdx.x * 256 + threadIdx.x; w < total; w += (long)gridDim.x * 256) {
    const int j8 = (int)(w & 1);
    long r = w >> 1;
    const int h = (int)(r % H); r /= H;
    const int sec = (int)(r % 3);
    const int t = (int)(r / 3);
    const size_t off = (size_t)t * 3 * d + sec * d + h * 32 + j8 * 8;
    const float4* pa = reinterpret_cast<const float4*>(src + off);
    const float4* pb = reinterpret_cast<const float4*>(src + off + 16);
    const float4 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1];
    const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    float oa[8], ob[8];
    if (sec < 2) {
      const int pos = position_ids ? (int)position_ids[t] : (t % S);
      const float4* ct = reinterpret_cast<const float4*>(cos_tab + (size_t)pos * 16 + j8 * 8);
      const float4* stb = reinterpret_cast<const float4*>(sin_tab + (size_t)pos * 16 + j8 * 8);
      const float4 c0 = ct[0], c1 = ct[1], s0 = stb[0], s1 = stb[1];
      const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w}, s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {     // (the contraction of the 64-wide epilogue, gemm.hip)
        oa[e] = fmaf(a[e], c[e], -(b[e] * s[e]));
        ob[e] = fmaf(b[e], c[e], a[e] * s[e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) { oa[e] = a[e]; ob[e] = b[e]; }
    }
    *reinterpret_cast<uint4*>(qkv + off) = pack8(oa);
    *reinterpret_cast<uint4*>(qkv + off + 16) = pack8(ob);
  }
}

// hf LlamaRotaryEmbedding.forward :111-127 at head width 32: inv_freq_j = theta^(-2 j / 32), j < 16; the evaluation of rope_table_kernel
__global__ void rope_table32_kernel(float* cos_tab, float* sin_tab, int max_pos, float theta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= max_pos * 16) return;
  const int pos = i >> 4, j = i & 15;
  const float inv_freq = 1.0f / powf(theta, (float)(2 * j) / 32.0f);
  const float fr = (float)pos * inv_freq;
  cos_tab[i] = (float)cos((double)fr);
  sin_tab[i] = (float)sin((double)fr);
}
// rope_range > 0 at head width 32: per-token angle tables [T][16] and the identity position list (rope_range_table_kernel's rule)
__global__ void __launch_bounds__(256) rope_range_table32_kernel(const int64_t* __restrict__ pos, float* __restrict__ cos_t,
                                                                 float* __restrict__ sin_t, int64_t* __restrict__ ids, int S, float range,
                                                                 float theta) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const int64_t* row = pos + (size_t)b * S;
  float mx = -INFINITY;
  for (int s = threadIdx.x; s < S; s += 256) mx = fmaxf(mx, (float)row[s]);     // (positions < 2^24: exact in fp32)
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float den = mx + 1.0f;
  for (int i = threadIdx.x; i < S * 16; i += 256) {
    const int s = i >> 4, j = i & 15;
    const float scaled = (float)row[s] * range / den;
    const float inv_freq = 1.0f / powf(theta, (float)(2 * j) / 32.0f);
    const float fr = scaled * inv_freq;
    cos_t[((size_t)b * S + s) * 16 + j] = (float)cos((double)fr);
    sin_t[((size_t)b * S + s) * 16 + j] = (float)sin((double)fr);
    if (j == 0) ids[(size_t)b * S + s] = (int64_t)b * S + s;
  }
}

}  // namespace

int k_attn32_fwd(const void* qkv, const int32_t* key_len, void* out, float* lse, int B, int S, int H, int causal, float dropout_p,
                 unsigned dropout_seed, hipStream_t st, const int32_t* key_lo, const int32_t* key_hi, const int32_t* row_base) {
  GGET_REQUIRE(qkv && out && lse, "attention (head width 32): null argument");
  GGET_REQUIRE(!key_lo == !key_hi, "attention (head width 32): half a key range");
  GGET_REQUIRE(!row_base || (key_len && !key_lo), "attention: the var-len token layout needs key_len and excludes per-token key ranges");
  if (B == 0 || S == 0) return 0;
  GGET_REQUIRE(B > 0 && S > 0 && H > 0 && B <= 65535 && H <= 65535, "attention (head width 32): bad shape B %d S %d H %d", B, S, H);
  const KeyRange KR{key_lo ? nullptr : key_len, key_lo, key_hi, row_base};
  const Drop D = make_drop(dropout_p, dropout_seed);
  const dim3 grid((S + 31) / 32, H, B);
  if (key_lo) hipLaunchKernelGGL((attn32_fwd_kernel<true>), grid, dim3(64), 0, st, (const bf16_t*)qkv, KR, (bf16_t*)out, lse, B, S, H, causal, D);
  else hipLaunchKernelGGL((attn32_fwd_kernel<false>), grid, dim3(64), 0, st, (const bf16_t*)qkv, KR, (bf16_t*)out, lse, B, S, H, causal, D);
  GGET_LAUNCH_CHECK();
  return 0;
}

int k_attn32_bwd(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len, void* dqkv, float* delta_ws,
                 int B, int S, int H, int causal, const float* cos_tab, const float* sin_tab, const int64_t* position_ids, float dropout_p,
                 unsigned dropout_seed, hipStream_t st, const int32_t* key_lo, const int32_t* key_hi, const int32_t* row_base) {
  GGET_REQUIRE(qkv && out && dout && lse && dqkv && delta_ws, "attention backward (head width 32): null argument");
  GGET_REQUIRE(!key_lo == !key_hi, "attention backward (head width 32): half a key range");
  GGET_REQUIRE(!cos_tab == !sin_tab, "attention backward (head width 32): half an angle table");
  GGET_REQUIRE(!row_base || (key_len && !key_lo), "attention: the var-len token layout needs key_len and excludes per-token key ranges");
  if (B == 0 || S == 0) return 0;
  GGET_REQUIRE(B > 0 && S > 0 && H > 0 && B <= 65535 && H <= 65535, "attention (head width 32): bad shape B %d S %d H %d", B, S, H);
  const KeyRange KR{key_lo ? nullptr : key_len, key_lo, key_hi, row_base};
  const Rope R{cos_tab, sin_tab, cos_tab ? position_ids : nullptr, S};     // rotation of dq, dk back to the un-rotated projections
  const Drop D = make_drop(dropout_p, dropout_seed);
  const dim3 grid((S + 31) / 32, H, B);
#define GGET_ATTN32_BWD(PK)                                                                                                        \
  do {                                                                                                                             \
    hipLaunchKernelGGL((attn32_bwd_dq_kernel<PK>), grid, dim3(64), 0, st, (const bf16_t*)qkv, (const bf16_t*)out, (const bf16_t*)dout, \
                       lse, delta_ws, KR, (bf16_t*)dqkv, B, S, H, causal, R, D);                                                   \
    hipLaunchKernelGGL((attn32_bwd_dkv_kernel<PK>), grid, dim3(64), 0, st, (const bf16_t*)qkv, (const bf16_t*)dout, lse, delta_ws, KR, \
                       (bf16_t*)dqkv, B, S, H, causal, R, D);                                                                      \
  } while (0)
  if (key_lo) GGET_ATTN32_BWD(true);
  else GGET_ATTN32_BWD(false);
#undef GGET_ATTN32_BWD
  GGET_LAUNCH_CHECK();
  return 0;
}

int k_attn32_probs(const void* qkv, const float* lse, const int32_t* key_len, const int32_t* row_base, const int32_t* key_lo,
                   const int32_t* key_hi, void* out, int B, int S, int H, int causal, float dropout_p, unsigned dropout_seed,
                   hipStream_t st) {
  GGET_REQUIRE(qkv && lse && out, "attn_probs: null argument");
  GGET_REQUIRE(B > 0 && S > 0 && H > 0 && B <= 65535 && H <= 65535, "attn_probs: bad shape B %d S %d H %d", B, S, H);
  GGET_REQUIRE(!key_lo == !key_hi, "attn_probs: half a key range");
  GGET_REQUIRE(!row_base || (key_len && !key_lo), "attn_probs: the var-len token layout needs key_len and excludes per-token key ranges");
  GGET_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "attn_probs: dropout_p %g outside [0, 1)", (double)dropout_p);
  const KeyRange KR{key_lo ? nullptr : key_len, key_lo, key_hi, row_base};
  const Drop D = make_drop(dropout_p, dropout_seed);
  const int vec = (S % 4 == 0) && (((uintptr_t)out & 7) == 0);
  const dim3 grid((S + 31) / 32, H, B);
  if (key_lo) hipLaunchKernelGGL((attn32_probs_kernel<true>), grid, dim3(64), 0, st, (const bf16_t*)qkv, lse, KR, (bf16_t*)out, B, S, H, causal, D, vec);
  else hipLaunchKernelGGL((attn32_probs_kernel<false>), grid, dim3(64), 0, st, (const bf16_t*)qkv, lse, KR, (bf16_t*)out, B, S, H, causal, D, vec);
  GGET_LAUNCH_CHECK();
  return 0;
}

int k_rope32(void* qkv, const float* cos_tab, const float* sin_tab, const int64_t* position_ids, int T, int S, int H, int inverse,
             hipStream_t st) {
  GGET_REQUIRE(qkv && cos_tab && sin_tab, "rope: null argument");
  GGET_REQUIRE(T >= 0 && H >= 1 && S >= 1, "rope: bad shape T %d S %d H %d", T, S, H);
  if (T == 0) return 0;
  const long n = (long)T * 4 * H;
  hipLaunchKernelGGL(rope32_kernel, dim3((unsigned)std::min<long>(4096, (n + 255) / 256)), dim3(256), 0, st, (bf16_t*)qkv, cos_tab, sin_tab,
                     position_ids, T, S, H, inverse);
  GGET_LAUNCH_CHECK();
  return 0;
}

int k_rope32_f32(const float* src, void* qkv, const float* cos_tab, const float* sin_tab, const int64_t* position_ids, int T, int S, int H,
                 hipStream_t st) {
  GGET_REQUIRE(src && qkv && cos_tab && sin_tab, "rope: null argument");
  GGET_REQUIRE(T >= 0 && H >= 1 && S >= 1, "rope: bad shape T %d S %d H %d", T, S, H);
  if (T == 0) return 0;
  const long n = (long)T * 6 * H;
  hipLaunchKernelGGL(rope32_f32_kernel, dim3((unsigned)std::min<long>(4096, (n + 255) / 256)), dim3(256), 0, st, src, (bf16_t*)qkv, cos_tab,
                     sin_tab, position_ids, T, S, H);
  GGET_LAUNCH_CHECK();
  return 0;
}

int k_rope_table_hd(float* cos_tab, float* sin_tab, int max_pos, float theta, int head_dim, hipStream_t st) {
  if (head_dim == 64) return k_rope_table(cos_tab, sin_tab, max_pos, theta, st);
  GGET_REQUIRE(head_dim == 32, "rope table: unsupported head_dim %d", head_dim);
  hipLaunchKernelGGL(rope_table32_kernel, dim3((max_pos * 16 + 255) / 256), dim3(256), 0, st, cos_tab, sin_tab, max_pos, theta);
  GGET_LAUNCH_CHECK();
  return 0;
}

int k_rope_range_table_hd(const int64_t* pos, float* cos_t, float* sin_t, int64_t* ids, int B, int S, float range, float theta, int head_dim,
                          hipStream_t st) {
  if (head_dim == 64) return k_rope_range_table(pos, cos_t, sin_t, ids, B, S, range, theta, st);
  GGET_REQUIRE(head_dim == 32, "rope range table: unsupported head_dim %d", head_dim);
  if (B * S == 0) return 0;
  hipLaunchKernelGGL(rope_range_table32_kernel, dim3(B), dim3(256), 0, st, pos, cos_t, sin_t, ids, S, range, theta);
  GGET_LAUNCH_CHECK();
  return 0;
}
