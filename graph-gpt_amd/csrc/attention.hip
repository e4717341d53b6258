// Self-attention core of the Graph Eulerian Transformer on gfx950 MFMA (32x32x16 bf16).
// reference: hf eager_attention_forward :191-214 / SDPA as selected by LlamaAttention.forward :243-281:
//   P = softmax_fp32(Q K^T * dh^-1/2 + mask) ; O = bf16(P) V, bidirectional or causal, keys >= key_len[b]
// masked (the reference's additive [B,1,S,S] mask is never materialised: right padding => a length).
// qkv is [T,3d] (q | k | v, head h at column h*64), q/k UN-rotated: RoPE is applied on the operand loads.
//
// Formulation (one wave per 32-row tile, dh = 64): scores are computed TRANSPOSED,
//   S^T[key][query] = K_tile Q_tile^T, so a lane owns ONE query column: the softmax statistics
// (m, l, lse, delta) are lane-local scalars, and the bf16 P^T accumulator registers are directly the
// B operand of the next MFMA  O^T[dh][query] += V^T[dh][key] P^T[key][query].  The only transposed
// operand (V^T, K^T, Q^T, dO^T: contraction index strided in memory) is read from a 4 KB LDS tile with
// gfx950's ds_read_b64_tr_b16.  Backward = delta kernel + dQ kernel (per query tile) + dK/dV kernel
// (per key tile); no atomics, P recomputed from the saved log-sum-exp.
#include <stdlib.h>
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "attn_common.h"
#include <type_traits>

#define LDS_AS __attribute__((address_space(3)))

namespace {

constexpr float kScale = 0.125f;  // head_dim^-0.5, head_dim = 64
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kScaleL2 = kScale * kLog2e;
// v_exp_f32 alone: the library exp2f wraps it in a range check + scaling (6 instructions) to keep denormal results, which a
// probability never needs - the softmax loops are VALU-bound (PMC: 225 VALU instructions per 32x32 score tile before, 62 % VALU busy)
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }   // scores are carried in the log2 domain: p = exp2(s * kScaleL2 - m2)

// [32 rows][128 B] tile: the 16-byte chunk index is XORed with a 3-bit function of the row so that both access patterns
// are bank-conflict free: ds_read_b128 of one chunk over 16 consecutive rows (rows of equal parity need 8 distinct chunk
// slots: f is a bijection of (row>>1)&7) and ds_read_b64_tr_b16 over 4 consecutive rows x 64 B (rows r and r+2 must fall
// into different 64-byte halves: bit 2 of f = bit 0 of row>>1).  PMC before: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE
// 0.32-0.45 with the old single-bit swizzle.
__device__ __forceinline__ int swz(int row, int byte_in_row) {
  const int x = (row >> 1) & 7;
  const int f = ((x & 1) << 2) | (x >> 1);
  return row * 128 + ((((byte_in_row >> 4) ^ f) << 4) | (byte_in_row & 15));
}

// RoPE fused into the operand loads (hf apply_rotary_pos_emb :138-160, half-split pairing j <-> j+32): q and k stay
// un-rotated in HBM; they are rotated in registers on the way into the MFMAs and dq/dk are rotated back on the way out.
// lo holds dh [j0, j0+8), up holds dh [j0+32, j0+40); rotate both in place by the angle table row `pos`
__device__ __forceinline__ void rope_pair(uint4& lo, uint4& up, const Rope& R, int pos, int j0) {
  float a[8], b[8], c[8], sn[8];
  unpack8(lo, a);
  unpack8(up, b);
  const float4* ct = reinterpret_cast<const float4*>(R.cos_tab + (size_t)pos * 32 + j0);
  const float4* st = reinterpret_cast<const float4*>(R.sin_tab + (size_t)pos * 32 + j0);
  const float4 c0 = ct[0], c1 = ct[1], s0 = st[0], s1 = st[1];
  c[0] = c0.x; c[1] = c0.y; c[2] = c0.z; c[3] = c0.w; c[4] = c1.x; c[5] = c1.y; c[6] = c1.z; c[7] = c1.w;
  sn[0] = s0.x; sn[1] = s0.y; sn[2] = s0.z; sn[3] = s0.w; sn[4] = s1.x; sn[5] = s1.y; sn[6] = s1.z; sn[7] = s1.w;
  float oa[8], ob[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    oa[e] = a[e] * c[e] - b[e] * sn[e];
    ob[e] = b[e] * c[e] + a[e] * sn[e];
  }
  lo = pack8(oa);
  up = pack8(ob);
}


// [32 rows][64 dh] bf16 tile -> LDS (rows >= row_lim are zero-filled so masked probabilities never meet NaNs)
__device__ __forceinline__ void load_tile(unsigned char* lds, const bf16_t* __restrict__ base, int r0, int row_lim,
                                          size_t pitch, int lane) {
  uint4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + i * 64;
    const int row = c >> 3, ch = c & 7;
    v[i] = *reinterpret_cast<const uint4*>(base + (size_t)clamp_row(r0 + row, row_lim) * pitch + ch * 8);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + i * 64;
    const int row = c >> 3, ch = c & 7;
    *reinterpret_cast<uint4*>(lds + swz(row, ch * 16)) = zero_if(r0 + row >= row_lim, v[i]);
  }
}
// same, rotating every row by its position (each lane fetches its chunk and the chunk 32 channels away).
// Cooperative: the NT threads of the block split the tile's 256 16-byte chunks.
template <int NT>
__device__ __forceinline__ void load_tile_coop(unsigned char* lds, const bf16_t* __restrict__ base, int r0, int row_lim,
                                               size_t pitch, int tid, const Rope& R, int b) {
  constexpr int N = 256 / NT;
  if (R.cos_tab) {
    uint4 lo[N], up[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = tid + i * NT;
      const int row = c >> 3, ch = c & 7;
      const bf16_t* rp = base + (size_t)clamp_row(r0 + row, row_lim) * pitch;
      lo[i] = *reinterpret_cast<const uint4*>(rp + (ch & 3) * 8);
      up[i] = *reinterpret_cast<const uint4*>(rp + (ch & 3) * 8 + 32);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = tid + i * NT;
      const int row = c >> 3, ch = c & 7;
      const int gr = r0 + row;
      rope_pair(lo[i], up[i], R, rope_pos(R, b, clamp_row(gr, row_lim)), (ch & 3) * 8);
      *reinterpret_cast<uint4*>(lds + swz(row, ch * 16)) = zero_if(gr >= row_lim, (ch & 4) ? up[i] : lo[i]);
    }
  } else {
    uint4 v[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = tid + i * NT;
      const int row = c >> 3, ch = c & 7;
      v[i] = *reinterpret_cast<const uint4*>(base + (size_t)clamp_row(r0 + row, row_lim) * pitch + ch * 8);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = tid + i * NT;
      const int row = c >> 3, ch = c & 7;
      *reinterpret_cast<uint4*>(lds + swz(row, ch * 16)) = zero_if(r0 + row >= row_lim, v[i]);
    }
  }
}
// Register-prefetched variant of load_tile_coop: `tile_fetch` only issues the global loads of a tile (they stay in flight
// while the block computes on the tile already in LDS), `tile_commit` rotates (if asked) and writes them to LDS later.
template <int NT>
struct TilePref {
  uint4 lo[256 / NT];
  uint4 up[256 / NT];   // the chunk 32 channels away (RoPE partner); only loaded when a rotation is applied
};
template <int NT>
__device__ __forceinline__ void tile_fetch(TilePref<NT>& p, const bf16_t* __restrict__ base, int r0, int row_lim, size_t pitch,
                                           int tid, const Rope& R) {
  if (R.cos_tab) {
#pragma unroll
    for (int i = 0; i < 256 / NT; ++i) {
      const int c = tid + i * NT;
      const int row = c >> 3, ch = c & 7;
      const bf16_t* rp = base + (size_t)clamp_row(r0 + row, row_lim) * pitch;
      p.lo[i] = *reinterpret_cast<const uint4*>(rp + (ch & 3) * 8);
      p.up[i] = *reinterpret_cast<const uint4*>(rp + (ch & 3) * 8 + 32);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 256 / NT; ++i) {
      const int c = tid + i * NT;
      const int row = c >> 3, ch = c & 7;
      p.lo[i] = *reinterpret_cast<const uint4*>(base + (size_t)clamp_row(r0 + row, row_lim) * pitch + ch * 8);
    }
  }
}
template <int NT>
__device__ __forceinline__ void tile_commit(unsigned char* lds, TilePref<NT>& p, int r0, int row_lim, int tid, const Rope& R,
                                            int b) {
  if (R.cos_tab) {
#pragma unroll
    for (int i = 0; i < 256 / NT; ++i) {
      const int c = tid + i * NT;
      const int row = c >> 3, ch = c & 7;
      const int gr = r0 + row;
      uint4 lo = p.lo[i], up = p.up[i];
      rope_pair(lo, up, R, rope_pos(R, b, clamp_row(gr, row_lim)), (ch & 3) * 8);
      *reinterpret_cast<uint4*>(lds + swz(row, ch * 16)) = zero_if(gr >= row_lim, (ch & 4) ? up : lo);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 256 / NT; ++i) {
      const int c = tid + i * NT;
      const int row = c >> 3, ch = c & 7;
      *reinterpret_cast<uint4*>(lds + swz(row, ch * 16)) = zero_if(r0 + row >= row_lim, p.lo[i]);
    }
  }
}
__device__ __forceinline__ void load_tile_rope(unsigned char* lds, const bf16_t* __restrict__ base, int r0, int row_lim,
                                               size_t pitch, int lane, const Rope& R, int b) {
  load_tile_coop<64>(lds, base, r0, row_lim, pitch, lane, R, b);
}

// MFMA operand whose "row/col" index is the tile row (lane&31) and whose k-chunk is dh [16s + 8*hi, +8)
__device__ __forceinline__ bf16x8_t frag_rows(const unsigned char* lds, int s, int lane) {
  const uint4 v = *reinterpret_cast<const uint4*>(lds + swz(lane & 31, (2 * s + (lane >> 5)) * 16));
  return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ bf16x8_t frag_global(const bf16_t* __restrict__ base, int row, int row_lim, size_t pitch, int s,
                                                int lane) {
  const uint4 v = *reinterpret_cast<const uint4*>(base + (size_t)clamp_row(row, row_lim) * pitch + 16 * s + (lane >> 5) * 8);
  return __builtin_bit_cast(bf16x8_t, zero_if(row >= row_lim, v));
}

// the 4 dh-fragments of one row (dh chunk [16s + 8hi, +8), s = 0..3), rotated: chunks s and s+2 are 32 channels apart
__device__ __forceinline__ void frags_global_rope(bf16x8_t (&f)[4], const bf16_t* __restrict__ base, int row, int row_lim,
                                                  size_t pitch, int lane, const Rope& R, int b) {
  uint4 v[4];
  const int rowc = clamp_row(row, row_lim);
#pragma unroll
  for (int s = 0; s < 4; ++s) v[s] = *reinterpret_cast<const uint4*>(base + (size_t)rowc * pitch + 16 * s + (lane >> 5) * 8);
  if (R.cos_tab) {
    const int pos = rope_pos(R, b, rowc);
    rope_pair(v[0], v[2], R, pos, (lane >> 5) * 8);
    rope_pair(v[1], v[3], R, pos, 16 + (lane >> 5) * 8);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) f[s] = __builtin_bit_cast(bf16x8_t, zero_if(row >= row_lim, v[s]));
}
// transposed operand: MFMA row = dh (dhb*32 + lane&31), k = tile rows {16j + 4hi + (e&3) + 8(e>>2)}
__device__ __forceinline__ bf16x8_t frag_tr(const unsigned char* lds, int dhb, int j, int lane) {
  const int li = lane & 15, g = lane >> 4, hi = lane >> 5;
  const int colb = (dhb * 32 + (g & 1) * 16 + (li & 3) * 4) * 2;
  const int ra = 16 * j + 4 * hi + (li >> 2);
  const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4_t*)(lds + swz(ra, colb)));
  const bf16x4_t up = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4_t*)(lds + swz(ra + 8, colb)));
  bf16x8_t o;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3];
  o[4] = up[0]; o[5] = up[1]; o[6] = up[2]; o[7] = up[3];
  return o;
}

// store a transposed accumulator pair (O^T[dh][row]) as row-major bf16 [row][64 dh]; lane owns row (lane&31)
// Registers [4 rr, 4 rr + 4) of a lane are dh 8 rr + 4 hi ..+3 of its row: 8 bytes.  The two lanes of a row (hi = 0 / 1) trade pieces with
// v_permlane32_swap so that the hi = 0 lane holds the 16 bytes dh [8 rr, 8 rr + 8) of the even rr and the hi = 1 lane those of the odd
// rr: four 16-byte stores per lane (32 contiguous bytes per row and instruction) instead of eight 8-byte ones - S <= 32 forward 12.4 ->
// 10.8 us, backward 24.6 -> 20.2 us, C1 step 7.18 -> 7.14 ms, C3 37.9 -> 37.6 ms (same box, libraries alternated).  Both lanes of a row
// are active or inactive together (the callers predicate on the row).
__device__ __forceinline__ void store_t(bf16_t* __restrict__ dst_row, const f32x16_t& a0, const f32x16_t& a1, float mul,
                                        int hi) {
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const f32x16_t& a = half ? a1 : a0;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const int e = 2 * pr, o = 2 * pr + 1;
      const unsigned e0 = pack2bf(a[4 * e + 0] * mul, a[4 * e + 1] * mul), e1 = pack2bf(a[4 * e + 2] * mul, a[4 * e + 3] * mul);
      const unsigned o0 = pack2bf(a[4 * o + 0] * mul, a[4 * o + 1] * mul), o1 = pack2bf(a[4 * o + 2] * mul, a[4 * o + 3] * mul);
      const hw_u32x2_t w0 = __builtin_amdgcn_permlane32_swap(e0, o0, false, false);
      const hw_u32x2_t w1 = __builtin_amdgcn_permlane32_swap(e1, o1, false, false);
      uint4 v;
      v.x = w0[0]; v.y = w1[0]; v.z = w0[1]; v.w = w1[1];
      *reinterpret_cast<uint4*>(dst_row + 32 * half + 8 * (hi ? o : e)) = v;
    }
  }
}

// gradient of a rotated row back to the un-rotated one: x = R(-theta) x'   (a0 = dh 0..31, a1 = dh 32..63)
__device__ __forceinline__ void unrope_acc(f32x16_t& a0, f32x16_t& a1, const Rope& R, int pos, int hi) {
  if (!R.cos_tab) return;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int j0 = 8 * rr + 4 * hi;
    const float4 c = *reinterpret_cast<const float4*>(R.cos_tab + (size_t)pos * 32 + j0);
    const float4 sn = *reinterpret_cast<const float4*>(R.sin_tab + (size_t)pos * 32 + j0);
    const float cc[4] = {c.x, c.y, c.z, c.w}, ss[4] = {sn.x, sn.y, sn.z, sn.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = a0[4 * rr + e], up = a1[4 * rr + e];
      a0[4 * rr + e] = lo * cc[e] + up * ss[e];
      a1[4 * rr + e] = up * cc[e] - lo * ss[e];
    }
  }
}

constexpr int kRopePitch = 36;      // floats per staged angle-table row (32 + 4: the lanes' 16-byte reads of 32 rows spread over the banks)
// the same with the lane's angle-table pieces already in registers (rope_fetch): the per-sample backward requests them before its matrix
// work - behind the MFMAs the position -> cos / sin chain was two dependent global round trips at the very end of the kernel, twice
__device__ __forceinline__ void rope_fetch(const Rope& R, int pos, int hi, float4 (&c)[4], float4 (&sn)[4]) {
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int j0 = 8 * rr + 4 * hi;
    c[rr] = *reinterpret_cast<const float4*>(R.cos_tab + (size_t)pos * 32 + j0);
    sn[rr] = *reinterpret_cast<const float4*>(R.sin_tab + (size_t)pos * 32 + j0);
  }
}
__device__ __forceinline__ void unrope_acc_pre(f32x16_t& a0, f32x16_t& a1, const float4 (&c)[4], const float4 (&sn)[4]) {
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const float cc[4] = {c[rr].x, c[rr].y, c[rr].z, c[rr].w}, ss[4] = {sn[rr].x, sn[rr].y, sn[rr].z, sn[rr].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = a0[4 * rr + e], up = a1[4 * rr + e];
      a0[4 * rr + e] = lo * cc[e] + up * ss[e];
      a1[4 * rr + e] = up * cc[e] - lo * ss[e];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Block = NW waves = NW consecutive 32-query tiles of one (batch, head); every 32-key K tile and V tile is brought into
// LDS ONCE per block (K rotated on the way in when R is given) and shared by the NW waves: K as the A operand of
// S^T = K Q^T (ds_read_b128), V through the transposing read for O^T += V^T P^T.
template <int NW, bool PK>
__global__ void __launch_bounds__(NW * 64, NW == 1 ? 3 : 2) attn_fwd_kernel(const bf16_t* __restrict__ qkv, KeyRange KR,
                                                           bf16_t* __restrict__ out, float* __restrict__ lse, int B, int S,
                                                           int H, int causal, Rope R, Drop D) {
  __shared__ __attribute__((aligned(16))) unsigned char kt[4096];
  __shared__ __attribute__((aligned(16))) unsigned char vt[4096];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.y, b = blockIdx.z;
  // var-len token layout (KR.row_base): sample b owns rows [rb, rb + SL) of the token-major buffers; padded layout: rb = b * S, SL = S
  const int rb = KR.row_base ? KR.row_base[b] : b * S;
  const int SL = KR.row_base ? KR.key_len[b] : S;
  // var-len layout: the grid is sized by the padded width S (the batch's longest graph, reference src/data/collator.py:70-111), the
  // sample owns SL rows - blocks wholly behind them have nothing to load or store (at S = 40 / 56 nineteen graphs in twenty are <= 32
  // tokens: without this exit their second block staged every K / V tile for nothing, 20.0 us per launch against 11.9 at S = 32)
  if (KR.row_base && (int)blockIdx.x * NW * 32 >= SL) return;
  const int q0 = (blockIdx.x * NW + wave) * 32;
  const int d = H * 64;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const int qrow = q0 + l31;
  const Rope Rnone{nullptr, nullptr, nullptr, S};
  // per-lane inclusive key range [qlo, qhi]; wave-uniform union [ulo, uhi] (tiles outside are skipped) and intersection
  // [ilo, ihi] (tiles inside need no mask)
  constexpr bool packed = PK;   // per-token key ranges (KR.lo / KR.hi) instead of one key length per batch row
  int qlo = 0, qhi = (KR.key_len ? KR.key_len[b] : S) - 1;
  int ulo = 0, uhi = qhi, ilo = 0, ihi = qhi;
  if (packed) {
    const bool v = qrow < SL;
    qlo = v ? KR.lo[(size_t)b * S + qrow] : 0;
    qhi = v ? KR.hi[(size_t)b * S + qrow] : -1;
    ulo = wave_imin(qhi >= qlo ? qlo : S); uhi = wave_imax(qhi >= qlo ? qhi + 1 : 0) - 1;
    ilo = wave_imax(v ? qlo : 0); ihi = wave_imin(v ? qhi + 1 : S) - 1;
  }
  const int klen = packed ? S : qhi + 1;     // block-level upper bound of the key loop

  bf16x8_t qf[4];
  frags_global_rope(qf, qb, qrow, SL, pitch, lane, R, b);
  f32x16_t o0 = zero16(), o1 = zero16();
  float m = -INFINITY, l = 0.f;
  const unsigned dbase = drop_base(D, b * H + h, qrow, 0);
  const int q_end_blk = min(SL, (int)(blockIdx.x + 1) * NW * 32);       // one past the block's last query row
  const int kend_blk = causal ? min(klen, q_end_blk) : klen;
  const int kend = (q0 < SL) ? min(uhi + 1, causal ? q0 + 32 : SL) : 0;  // this wave's own key range
  constexpr bool PF = NW > 1;   // single-wave blocks see one tile (S <= 32): nothing to prefetch, registers are tight
  TilePref<NW * 64> pk, pv;
  if (PF && kend_blk > 0) {
    tile_fetch<NW * 64>(pk, kb, 0, SL, pitch, tid, R);
    tile_fetch<NW * 64>(pv, vb, 0, SL, pitch, tid, Rnone);
  }
  for (int k0 = 0; k0 < kend_blk; k0 += 32) {
    __syncthreads();  // previous tile fully consumed
    if constexpr (PF) {
      tile_commit<NW * 64>(kt, pk, k0, SL, tid, R, b);
      tile_commit<NW * 64>(vt, pv, k0, SL, tid, Rnone, b);
    } else {
      load_tile_coop<NW * 64>(kt, kb, k0, SL, pitch, tid, R, b);
      load_tile_coop<NW * 64>(vt, vb, k0, SL, pitch, tid, Rnone, b);
    }
    __syncthreads();
    if (PF && k0 + 32 < kend_blk) {   // next tile's loads fly while this one is computed
      tile_fetch<NW * 64>(pk, kb, k0 + 32, SL, pitch, tid, R);
      tile_fetch<NW * 64>(pv, vb, k0 + 32, SL, pitch, tid, Rnone);
    }
    if (k0 >= kend || k0 + 31 < ulo) continue;
    f32x16_t sc = zero16();
#pragma unroll
    for (int s = 0; s < 4; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(kt, s, lane), qf[s], sc, 0, 0, 0);
    // The loop is VALU-bound (head_dim 64: ~0.25 MFMA cycles but several VALU cycles per score), so: scores stay raw
    // until one fma + exp2 (scale and log2(e) folded, running max kept in the log2 domain); the key / causal mask is only
    // evaluated on tiles that touch the sequence end or the diagonal; O is rescaled only when some lane's max moved.
    const bool edge = (k0 < ilo) || (k0 + 31 > ihi) || (causal && k0 + 31 > q0) || (q0 + 32 > SL);
    float mx = -INFINITY;
    if (edge) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + acc_row(r, hi);
        const bool ok = key >= qlo && key <= qhi && (!causal || key <= qrow);
        sc[r] = ok ? sc[r] : -INFINITY;
        mx = fmaxf(mx, sc[r]);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx * kScaleL2);     // kScaleL2 > 0: max commutes with the scaling
    const bool dead = m_new == -INFINITY;
    const float alpha = dead ? 1.f : fast_exp2(m - m_new);
    const float nm = dead ? 0.f : -m_new;
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = fast_exp2(fmaf(sc[r], kScaleL2, nm));   // masked scores are -inf -> 0
      rs += p;                                                                    // softmax normaliser: before dropout
      sc[r] = p * drop_mul_x(D, dbase + (unsigned)((k0 + acc_row(r, hi)) >> 1) * 0xC2B2AE3Du, r & 1);   // what multiplies V (acc_row parity = r & 1)
    }
    rs += __shfl_xor(rs, 32, 64);
    l = l * alpha + rs;
    m = m_new;
    if (__any(alpha != 1.f)) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
    }
    const bf16x8_t pb0 = acc_to_b(sc, 0), pb1 = acc_to_b(sc, 1);
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 0, 0, lane), pb0, o0, 0, 0, 0);
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 0, 1, lane), pb1, o0, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 1, 0, lane), pb0, o1, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 1, 1, lane), pb1, o1, 0, 0, 0);
  }
  if (qrow < SL) {
    const float inv = l > 0.f ? 1.f / l : 0.f;   // (the keep scale 1/(1-p) is already folded into the dropped P)
    store_t(out + ((size_t)rb + qrow) * d + h * 64, o0, o1, inv, hi);
    if (hi == 0 && lse) lse[((size_t)b * H + h) * S + qrow] = l > 0.f ? (m + log2f(l)) * (1.0f / kLog2e) : 0.f;   // natural log
  }
}

// Var-len layout, 32 < S <= 64 (round 6): one wave per (sample, head, 32-query tile), keyed on the sample's OWN row count.  The collator pads
// a batch to the width of its LONGEST graph (reference src/data/collator.py:70-111), so at B = 256 the padded width is 40 - 56 while nineteen
// graphs in twenty are one 32-row tile.  The launch is ONE round of thousands of one-wave blocks and lasts as long as its slowest block;
// under that load every dependent global round trip of a block costs ~3 us, and attn_fwd_kernel<1> walks the key tiles one round trip at
// a time (20.0 us per launch at S = 40 against 11.9 at S = 32; a separate sparse launch for the long samples: 10.3 + 6.6 us).  Here a
// block requests EVERYTHING at once - Q rows, both K tiles, both V tiles, as whole-row tile loads (K rows fetched directly as MFMA
// operands, 32-byte pieces 4.6 KB apart, cost 14.5 us per launch: the texture addresser coalesces neighbouring lanes only) - and stages
// them through the SAME 8 KiB of LDS in two steps: K tiles in, K operands out to registers, V tiles in.  A 33 .. 64-row sample costs one
// round trip like the others; blocks behind a sample's rows exit.  The arithmetic is attn_fwd_kernel's, step by step (online softmax over
// key tile 0, then 1): same bits.  q / k are read as they are in memory (rotated - the engine's layout - or plain).
__global__ void __launch_bounds__(64, 3) attn_fwd_rows64_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ key_len,
                                                                const int32_t* __restrict__ row_base, bf16_t* __restrict__ out,
                                                                float* __restrict__ lse, int B, int S, int H, int causal, Drop D) {
  __shared__ __attribute__((aligned(16))) unsigned char tl[2][4096];
  const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;
  // grid (H, B, tiles), the LAST query tile first in dispatch order: the blocks behind a sample's rows (most of that tile's) flash through
  // at the start of the launch and the second tiles of the long samples begin with it, not behind three thousand first tiles
  const int h = blockIdx.x, b = blockIdx.y;
  const int rb = row_base[b];
  const int SL = min(key_len[b], 64);
  const int q0 = ((int)gridDim.z - 1 - (int)blockIdx.z) * 32;
  if (q0 >= SL) return;
  const int d = H * 64;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const int qrow = q0 + l31;
  const int kend = causal ? min(SL, q0 + 32) : SL;     // keys [0, kend) concern this tile
  const bool two = kend > 32;                           // (wave-uniform)
  const Rope Rnone{nullptr, nullptr, nullptr, S};
  bf16x8_t qf[4], kf[2][4];
  uint4 kraw[2][4], vraw[2][4];
  frags_global_rope(qf, qb, qrow, SL, pitch, lane, Rnone, b);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j == 1 && !two) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + i * 64, row = c >> 3, ch = c & 7;
      const size_t off = (size_t)clamp_row(32 * j + row, SL) * pitch + ch * 8;
      kraw[j][i] = *reinterpret_cast<const uint4*>(kb + off);
      vraw[j][i] = *reinterpret_cast<const uint4*>(vb + off);
    }
  }
  if (two) {
    // two key tiles: K0 | K1 through the LDS first, their MFMA operands parked in registers, then V0 | V1 take the same bytes
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = lane + i * 64, row = c >> 3, ch = c & 7;
        *reinterpret_cast<uint4*>(tl[j] + swz(row, ch * 16)) = zero_if(32 * j + row >= SL, kraw[j][i]);
      }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int s = 0; s < 4; ++s) kf[j][s] = frag_rows(tl[j], s, lane);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = lane + i * 64, row = c >> 3, ch = c & 7;
        *reinterpret_cast<uint4*>(tl[j] + swz(row, ch * 16)) = zero_if(32 * j + row >= SL, vraw[j][i]);
      }
    __syncthreads();
  } else {
    // one key tile (nineteen samples in twenty): K in the first half, V in the second - attn_fwd_kernel<1>'s staging
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + i * 64, row = c >> 3, ch = c & 7;
      *reinterpret_cast<uint4*>(tl[1] + swz(row, ch * 16)) = zero_if(row >= SL, kraw[0][i]);
      *reinterpret_cast<uint4*>(tl[0] + swz(row, ch * 16)) = zero_if(row >= SL, vraw[0][i]);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) kf[0][s] = frag_rows(tl[1], s, lane);
  }
  f32x16_t o0 = zero16(), o1 = zero16();
  float m = -INFINITY, l = 0.f;
  const unsigned dbase = drop_base(D, b * H + h, qrow, 0);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k0 = 32 * j;
    if (k0 >= kend) break;
    const unsigned char* vt = tl[j];
    f32x16_t sc = zero16();
#pragma unroll
    for (int s = 0; s < 4; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[j][s], qf[s], sc, 0, 0, 0);
    const bool edge = (k0 + 31 > SL - 1) || (causal && k0 + 31 > q0) || (q0 + 32 > SL);
    float mx = -INFINITY;
    if (edge) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + acc_row(r, hi);
        const bool ok = key < SL && (!causal || key <= qrow);
        sc[r] = ok ? sc[r] : -INFINITY;
        mx = fmaxf(mx, sc[r]);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx * kScaleL2);
    const bool dead = m_new == -INFINITY;
    const float alpha = dead ? 1.f : fast_exp2(m - m_new);
    const float nm = dead ? 0.f : -m_new;
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = fast_exp2(fmaf(sc[r], kScaleL2, nm));
      rs += p;
      sc[r] = p * drop_mul_x(D, dbase + (unsigned)((k0 + acc_row(r, hi)) >> 1) * 0xC2B2AE3Du, r & 1);
    }
    rs += __shfl_xor(rs, 32, 64);
    l = l * alpha + rs;
    m = m_new;
    if (__any(alpha != 1.f)) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
    }
    const bf16x8_t pb0 = acc_to_b(sc, 0), pb1 = acc_to_b(sc, 1);
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 0, 0, lane), pb0, o0, 0, 0, 0);
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 0, 1, lane), pb1, o0, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 1, 0, lane), pb0, o1, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 1, 1, lane), pb1, o1, 0, 0, 0);
  }
  if (qrow < SL) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    store_t(out + ((size_t)rb + qrow) * d + h * 64, o0, o1, inv, hi);
    if (hi == 0 && lse) lse[((size_t)b * H + h) * S + qrow] = l > 0.f ? (m + log2f(l)) * (1.0f / kLog2e) : 0.f;
  }
}

// dQ^T[dh][q] = sum_keys K^T[dh][key] dS^T[key][q],  dS^T = P^T (dP^T - delta_q) * scale
// Block = NW query tiles; the K tile (rotated if Rin) and the V tile are shared through LDS.
template <int NW, bool PK>
__global__ void __launch_bounds__(NW * 64, NW == 1 ? 3 : 2) attn_bwd_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                                              const float* __restrict__ lse, float* __restrict__ delta,
                                                              KeyRange KR, bf16_t* __restrict__ dqkv,
                                                              int B, int S, int H, int causal, Rope Rin, Rope R, Drop D) {
  __shared__ __attribute__((aligned(16))) unsigned char kt[4096];
  __shared__ __attribute__((aligned(16))) unsigned char vt[4096];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.y, b = blockIdx.z;
  // var-len token layout (KR.row_base): sample b owns rows [rb, rb + SL) of the token-major buffers; padded layout: rb = b * S, SL = S
  const int rb = KR.row_base ? KR.row_base[b] : b * S;
  const int SL = KR.row_base ? KR.key_len[b] : S;
  if (KR.row_base && (int)blockIdx.x * NW * 32 >= SL) return;     // (var-len layout: no rows of this sample in the block, see attn_fwd_kernel)
  const int q0 = (blockIdx.x * NW + wave) * 32;
  const int d = H * 64;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const bf16_t* dob = dout + (size_t)rb * d + h * 64;
  const int qrow = q0 + l31;
  const Rope Rnone{nullptr, nullptr, nullptr, S};
  constexpr bool packed = PK;      // see attn_fwd_kernel
  int qlo = 0, qhi = (KR.key_len ? KR.key_len[b] : S) - 1;
  int ulo = 0, uhi = qhi, ilo = 0, ihi = qhi;
  if (packed) {
    const bool v = qrow < SL;
    qlo = v ? KR.lo[(size_t)b * S + qrow] : 0;
    qhi = v ? KR.hi[(size_t)b * S + qrow] : -1;
    ulo = wave_imin(qhi >= qlo ? qlo : S); uhi = wave_imax(qhi >= qlo ? qhi + 1 : 0) - 1;
    ilo = wave_imax(v ? qlo : 0); ihi = wave_imin(v ? qhi + 1 : S) - 1;
  }
  const int klen = packed ? S : qhi + 1;
  bf16x8_t qf[4], dof[4];
  frags_global_rope(qf, qb, qrow, SL, pitch, lane, Rin, b);
#pragma unroll
  for (int s = 0; s < 4; ++s) dof[s] = frag_global(dob, qrow, SL, (size_t)d, s, lane);
  const size_t sidx = ((size_t)b * H + h) * S + min(qrow, S - 1);
  // delta_q = sum_dh dO*O of this query row (the lane holds half of the row's dO already; the other half sits in lane^32);
  // stored for the dK/dV kernel that follows on the same stream
  float dl = 0.f;
  {
    const bf16_t* ob = out + (size_t)rb * d + h * 64;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float a[8], gg[8];
      unpack8(__builtin_bit_cast(uint4, frag_global(ob, qrow, SL, (size_t)d, s, lane)), a);
      unpack8(__builtin_bit_cast(uint4, dof[s]), gg);
#pragma unroll
      for (int e = 0; e < 8; ++e) dl += a[e] * gg[e];
    }
    dl += __shfl_xor(dl, 32, 64);
    if (hi == 0 && qrow < SL) delta[sidx] = dl;
  }
  const float nlse2 = -lse[sidx] * kLog2e, ndl = -dl;
  const unsigned dbase = drop_base(D, b * H + h, qrow, 0);
  f32x16_t a0 = zero16(), a1 = zero16();
  const int q_end_blk = min(SL, (int)(blockIdx.x + 1) * NW * 32);
  const int kend_blk = causal ? min(klen, q_end_blk) : klen;
  const int kend = (q0 < SL) ? min(uhi + 1, causal ? q0 + 32 : SL) : 0;
  constexpr bool PF = NW > 1;
  TilePref<NW * 64> pk, pv;
  if (PF && kend_blk > 0) {
    tile_fetch<NW * 64>(pk, kb, 0, SL, pitch, tid, Rin);
    tile_fetch<NW * 64>(pv, vb, 0, SL, pitch, tid, Rnone);
  }
  for (int k0 = 0; k0 < kend_blk; k0 += 32) {
    __syncthreads();
    if constexpr (PF) {
      tile_commit<NW * 64>(kt, pk, k0, SL, tid, Rin, b);
      tile_commit<NW * 64>(vt, pv, k0, SL, tid, Rnone, b);
    } else {
      load_tile_coop<NW * 64>(kt, kb, k0, SL, pitch, tid, Rin, b);
      load_tile_coop<NW * 64>(vt, vb, k0, SL, pitch, tid, Rnone, b);
    }
    __syncthreads();
    if (PF && k0 + 32 < kend_blk) {
      tile_fetch<NW * 64>(pk, kb, k0 + 32, SL, pitch, tid, Rin);
      tile_fetch<NW * 64>(pv, vb, k0 + 32, SL, pitch, tid, Rnone);
    }
    if (k0 >= kend || k0 + 31 < ulo) continue;
    f32x16_t dp = zero16(), sc = zero16();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(vt, s, lane), dof[s], dp, 0, 0, 0);
      sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(kt, s, lane), qf[s], sc, 0, 0, 0);
    }
    const bool edge = (k0 < ilo) || (k0 + 31 > ihi) || (causal && k0 + 31 > q0) || (q0 + 32 > SL);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + acc_row(r, hi);
      float p = fast_exp2(fmaf(sc[r], kScaleL2, nlse2));
      if (edge) p = (key >= qlo && key <= qhi && (!causal || key <= qrow) && qrow < SL) ? p : 0.f;
      sc[r] = p * fmaf(dp[r], drop_mul_x(D, dbase + (unsigned)(key >> 1) * 0xC2B2AE3Du, key & 1), ndl) * kScale;
    }
    const bf16x8_t ds0 = acc_to_b(sc, 0), ds1 = acc_to_b(sc, 1);
    a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(kt, 0, 0, lane), ds0, a0, 0, 0, 0);
    a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(kt, 0, 1, lane), ds1, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(kt, 1, 0, lane), ds0, a1, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(kt, 1, 1, lane), ds1, a1, 0, 0, 0);
  }
  if (qrow < SL) {
    unrope_acc(a0, a1, R, rope_pos(R, b, qrow), hi);
    store_t(dqkv + ((size_t)rb + qrow) * pitch + h * 64, a0, a1, 1.f, hi);
  }
}

// dV^T[dh][key] = sum_q dO^T[dh][q] P[q][key] ; dK^T[dh][key] = sum_q Q^T[dh][q] dS[q][key]
// Block = NW key tiles; every 32-query Q tile (rotated if Rin), dO tile and their lse/delta are shared through LDS.
template <int NW, bool PK>
__global__ void __launch_bounds__(NW * 64, NW == 1 ? 3 : 2) attn_bwd_dkv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                               KeyRange KR, bf16_t* __restrict__ dqkv,
                                                               int B, int S, int H, int causal, Rope Rin, Rope R, Drop D) {
  __shared__ __attribute__((aligned(16))) unsigned char qt[4096];
  __shared__ __attribute__((aligned(16))) unsigned char dot_[4096];
  __shared__ float lse_s[32], dl_s[32];
  __shared__ int qlo_s[32], qhi_s[32];   // packed rows: inclusive key range of each query of the tile
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.y, b = blockIdx.z;
  // var-len token layout (KR.row_base): sample b owns rows [rb, rb + SL) of the token-major buffers; padded layout: rb = b * S, SL = S
  const int rb = KR.row_base ? KR.row_base[b] : b * S;
  const int SL = KR.row_base ? KR.key_len[b] : S;
  if (KR.row_base && (int)blockIdx.x * NW * 32 >= SL) return;     // (var-len layout: no rows of this sample in the block, see attn_fwd_kernel)
  const int k0 = (blockIdx.x * NW + wave) * 32;
  const int d = H * 64;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const bf16_t* dob = dout + (size_t)rb * d + h * 64;
  constexpr bool packed = PK;
  const int klen = packed ? S : (KR.key_len ? KR.key_len[b] : S);
  const int krow = k0 + l31;
  const Rope Rnone{nullptr, nullptr, nullptr, S};
  bf16x8_t kf[4], vf[4];
  frags_global_rope(kf, kb, krow, SL, pitch, lane, Rin, b);
#pragma unroll
  for (int s = 0; s < 4; ++s) vf[s] = frag_global(vb, krow, SL, pitch, s, lane);
  f32x16_t dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
  const unsigned dbase = drop_base(D, b * H + h, 0, (unsigned)krow >> 1);
  const bool key_ok = krow < klen;                 // right-padded rows: one key length per batch row
  const int kblk0 = blockIdx.x * NW * 32;          // first key of the block
  const int qstart = causal ? kblk0 : 0;           // queries before the block's first key never see it
  if (kblk0 < klen) {
    TilePref<NW * 64> pq, pdo;
    float p_lse = 0.f, p_dl = 0.f;
    int p_lo = 0, p_hi = klen - 1;
    auto fetch_q = [&](int q0) {
      tile_fetch<NW * 64>(pq, qb, q0, SL, pitch, tid, Rin);
      tile_fetch<NW * 64>(pdo, dob, q0, SL, (size_t)d, tid, Rnone);
      if (tid < 32) {
        const int q = min(q0 + tid, S - 1);
        p_lse = lse[((size_t)b * H + h) * S + q];
        // (var-len layout: the dQ kernel writes delta for the sample's own rows only; behind them the workspace holds whatever it held,
        //  and p = 0 times a NaN there is a NaN in dK of every key of the sample)
        p_dl = q0 + tid < SL ? delta[((size_t)b * H + h) * S + q] : 0.f;
        if (packed) {
          const bool v = q0 + tid < SL;
          p_lo = v ? KR.lo[(size_t)b * S + q] : 0;
          p_hi = v ? KR.hi[(size_t)b * S + q] : -1;
        }
      }
    };
    constexpr bool PF = NW > 1;
    if (PF && qstart < SL) fetch_q(qstart);
    for (int q0 = qstart; q0 < SL; q0 += 32) {
      __syncthreads();
      if constexpr (PF) {
        tile_commit<NW * 64>(qt, pq, q0, SL, tid, Rin, b);
        tile_commit<NW * 64>(dot_, pdo, q0, SL, tid, Rnone, b);
        if (tid < 32) {
          lse_s[tid] = -p_lse * kLog2e; dl_s[tid] = -p_dl;
          if (packed) { qlo_s[tid] = p_lo; qhi_s[tid] = p_hi; }
        }
      } else {
        load_tile_coop<NW * 64>(qt, qb, q0, SL, pitch, tid, Rin, b);
        load_tile_coop<NW * 64>(dot_, dob, q0, SL, (size_t)d, tid, Rnone, b);
        if (tid < 32) {
          const int q = min(q0 + tid, S - 1);
          lse_s[tid] = -lse[((size_t)b * H + h) * S + q] * kLog2e;
          dl_s[tid] = q0 + tid < SL ? -delta[((size_t)b * H + h) * S + q] : 0.f;     // (rows behind the sample: see fetch_q)
          if (packed) {
            const bool v = q0 + tid < SL;
            qlo_s[tid] = v ? KR.lo[(size_t)b * S + q] : 0;
            qhi_s[tid] = v ? KR.hi[(size_t)b * S + q] : -1;
          }
        }
      }
      __syncthreads();
      if (PF && q0 + 32 < SL) fetch_q(q0 + 32);
      if (k0 >= klen || (causal && q0 + 31 < k0)) continue;   // this wave's keys are padding / all in the future
      // packed rows: union / intersection of the tile's query ranges decide skipping and masking for this wave's 32 keys
      bool edge = (k0 + 32 > klen) || (q0 + 32 > SL) || (causal && k0 + 31 > q0);
      if (packed) {
        const int lo = qlo_s[l31], hi_ = qhi_s[l31];
        const int ulo = wave_imin(hi_ >= lo ? lo : S), uhi = wave_imax(hi_ >= lo ? hi_ + 1 : 0) - 1;
        if (uhi < k0 || ulo > k0 + 31) continue;
        const int ilo = wave_imax(lo), ihi = wave_imin(hi_ + 1) - 1;
        edge = edge || ilo > k0 || ihi < k0 + 31;
      }
      f32x16_t sc = zero16(), dp = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(qt, s, lane), kf[s], sc, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(dot_, s, lane), vf[s], dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qi = acc_row(r, hi);
        const int q = q0 + qi;
        float p = fast_exp2(fmaf(sc[r], kScaleL2, lse_s[qi]));          // lse_s holds -lse * log2(e)
        if (edge) {
          const bool in_range = packed ? (krow >= qlo_s[qi] && krow <= qhi_s[qi]) : key_ok;
          p = (in_range && q < SL && (!causal || krow <= q)) ? p : 0.f;
        }
        const float dm = drop_mul_x(D, dbase + (unsigned)q * 0x85EBCA77u, krow & 1);
        sc[r] = p * dm;                                  // dropped probabilities: what multiplied V in forward
        dp[r] = p * fmaf(dp[r], dm, dl_s[qi]) * kScale;  // dl_s holds -delta
      }
      const bf16x8_t p0 = acc_to_b(sc, 0), p1 = acc_to_b(sc, 1);
      const bf16x8_t s0 = acc_to_b(dp, 0), s1 = acc_to_b(dp, 1);
      dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 0, 0, lane), p0, dv0, 0, 0, 0);
      dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 0, 1, lane), p1, dv0, 0, 0, 0);
      dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 1, 0, lane), p0, dv1, 0, 0, 0);
      dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 1, 1, lane), p1, dv1, 0, 0, 0);
      dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 0, 0, lane), s0, dk0, 0, 0, 0);
      dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 0, 1, lane), s1, dk0, 0, 0, 0);
      dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 1, 0, lane), s0, dk1, 0, 0, 0);
      dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 1, 1, lane), s1, dk1, 0, 0, 0);
    }
  }
  if (krow < SL) {
    bf16_t* row = dqkv + ((size_t)rb + krow) * pitch + h * 64;
    unrope_acc(dk0, dk1, R, rope_pos(R, b, krow), hi);
    store_t(row + d, dk0, dk1, 1.f, hi);
    store_t(row + 2 * d, dv0, dv1, 1.f, hi);
  }
}

// A sample of 33 .. 64 rows (round 6): the S <= 32 kernel below over 2 x 2 tiles, as its OWN launch next to it.  The collator pads a batch
// to the width of its LONGEST graph (reference src/data/collator.py:70-111), so at B = 256 the padded width is 40 - 56 while nineteen
// graphs in twenty are still <= 32 tokens: the backward is keyed on each sample's own row count, not on S (the S > 32 path before:
// attn_bwd_dq_kernel<1> 43.8 us + attn_bwd_dkv_kernel<1> 48.8 us per layer at S = 40 against 21 us for the one-tile kernel).
// Block = TWO waves on one (sample, head); samples outside 33 .. 64 rows exit at once (they are the one-tile kernel's).  All six tiles
// (K, Q, dO x two 32-row tiles, 24 KiB) are requested up front and staged once; then
//   part 1  wave w = query tile w: scores and dP against BOTH key tiles stay in registers, so delta = sum_k P dP covers the whole row as in
//           the one-tile kernel; dQ_w^T = sum_j K_j^T dS_wj^T
//   part 2  wave w = key tile w: dK_w^T = sum_i Q_i^T dS_iw, dV_w^T = sum_i dO_i^T P_iw
// Why a second launch and not a branch of the one-tile kernel: inlined there the body spilled 178 - 313 registers of the COMMON path's
// allocation (168 at three waves per SIMD), as a called function it ran from 1.3 KiB of scratch per lane - 116 us per launch.  These few
// blocks (5 % of the samples) want registers and no neighbours; the thousands of one-tile blocks want occupancy.
// q and k are read as they are in memory (rotated already - the engine's layout - or no rotation at all); R rotates dq / dk back.
__device__ __attribute__((noinline)) void attn_bwd_long_item(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                             const float* __restrict__ lse, bf16_t* __restrict__ dqkv, int b, int rb, int SL,
                                                             int klen_b, int S, int H, int causal, const Rope& R, const Drop& D) {
  __shared__ __attribute__((aligned(16))) unsigned char tiles[6][4096];   // K0 K1 Q0 Q1 dO0 dO1
  __shared__ float lse_s[64], dl_s[64];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.y;
  const int d = H * 64;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const bf16_t* dob = dout + (size_t)rb * d + h * 64;
  const int klen = min(klen_b, S);
  const Rope Rnone{nullptr, nullptr, nullptr, S};
  TilePref<128> pf[6];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    tile_fetch<128>(pf[t], kb, 32 * t, SL, pitch, tid, Rnone);
    tile_fetch<128>(pf[2 + t], qb, 32 * t, SL, pitch, tid, Rnone);
    tile_fetch<128>(pf[4 + t], dob, 32 * t, SL, (size_t)d, tid, Rnone);
  }
  // the wave's own 32 rows (query tile w in part 1, key tile w in part 2): V rows as MFMA operands, lse, the angle-table pieces of the
  // final rotation - all requested before the first wait
  const int myrow = 32 * w + l31;
  bf16x8_t vf[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int s = 0; s < 4; ++s) vf[j][s] = frag_global(vb, 32 * j + l31, SL, pitch, s, lane);
  const float nlse2 = -lse[((size_t)b * H + h) * S + min(myrow, S - 1)] * kLog2e;
  float4 rc[4], rs[4];
  if (R.cos_tab) rope_fetch(R, rope_pos(R, b, min(myrow, S - 1)), hi, rc, rs);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    tile_commit<128>(tiles[t], pf[t], 32 * t, SL, tid, Rnone, b);
    tile_commit<128>(tiles[2 + t], pf[2 + t], 32 * t, SL, tid, Rnone, b);
    tile_commit<128>(tiles[4 + t], pf[4 + t], 32 * t, SL, tid, Rnone, b);
  }
  if (hi == 0) lse_s[myrow] = nlse2;
  __syncthreads();
  const unsigned bh = b * H + h;
  {   // ---------------- part 1: dQ of query tile w (lane owns query myrow)
    const int qrow = myrow;
    const unsigned char* qt = tiles[2 + w];
    const unsigned char* dot_ = tiles[4 + w];
    const unsigned dbase = drop_base(D, bh, qrow, 0);
    f32x16_t sc[2], dp[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      sc[j] = zero16(); dp[j] = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        dp[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[j][s], frag_rows(dot_, s, lane), dp[j], 0, 0, 0);
        sc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(tiles[j], s, lane), frag_rows(qt, s, lane), sc[j], 0, 0, 0);
      }
    }
    float dl = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = 32 * j + acc_row(r, hi);
        const bool ok = key < klen && (!causal || key <= qrow) && qrow < SL;
        const float p = ok ? fast_exp2(fmaf(sc[j][r], kScaleL2, nlse2)) : 0.f;
        const float t = dp[j][r] * drop_mul_x(D, dbase + (unsigned)(key >> 1) * 0xC2B2AE3Du, key & 1);
        dl = fmaf(p, t, dl);
        sc[j][r] = p;
        dp[j][r] = t;
      }
    dl += __shfl_xor(dl, 32, 64);
    if (hi == 0) dl_s[qrow] = -dl;
    f32x16_t a0 = zero16(), a1 = zero16();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[j][r] = sc[j][r] * (dp[j][r] - dl) * kScale;
      const bf16x8_t ds0 = acc_to_b(sc[j], 0), ds1 = acc_to_b(sc[j], 1);
      a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(tiles[j], 0, 0, lane), ds0, a0, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(tiles[j], 0, 1, lane), ds1, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(tiles[j], 1, 0, lane), ds0, a1, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(tiles[j], 1, 1, lane), ds1, a1, 0, 0, 0);
    }
    if (qrow < SL) {
      if (R.cos_tab) unrope_acc_pre(a0, a1, rc, rs);
      store_t(dqkv + ((size_t)rb + qrow) * pitch + h * 64, a0, a1, 1.f, hi);
    }
  }
  __syncthreads();   // dl_s of both query tiles
  {   // ---------------- part 2: dK, dV of key tile w (lane owns key myrow)
    const int krow = myrow;
    const bool key_ok = krow < klen;
    const unsigned dbase = drop_base(D, bh, 0, (unsigned)krow >> 1);
    const unsigned char* kt = tiles[w];
    f32x16_t dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned char* qt = tiles[2 + i];
      const unsigned char* dot_ = tiles[4 + i];
      f32x16_t sc = zero16(), dp = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(qt, s, lane), frag_rows(kt, s, lane), sc, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(dot_, s, lane), w ? vf[1][s] : vf[0][s], dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = 32 * i + acc_row(r, hi);
        const bool ok = key_ok && q < SL && (!causal || krow <= q);
        const float p = ok ? fast_exp2(fmaf(sc[r], kScaleL2, lse_s[q])) : 0.f;
        const float dm = drop_mul_x(D, dbase + (unsigned)q * 0x85EBCA77u, krow & 1);
        sc[r] = p * dm;
        dp[r] = p * fmaf(dp[r], dm, dl_s[q]) * kScale;
      }
      const bf16x8_t p0 = acc_to_b(sc, 0), p1 = acc_to_b(sc, 1);
      const bf16x8_t s0 = acc_to_b(dp, 0), s1 = acc_to_b(dp, 1);
      dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 0, 0, lane), p0, dv0, 0, 0, 0);
      dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 0, 1, lane), p1, dv0, 0, 0, 0);
      dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 1, 0, lane), p0, dv1, 0, 0, 0);
      dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 1, 1, lane), p1, dv1, 0, 0, 0);
      dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 0, 0, lane), s0, dk0, 0, 0, 0);
      dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 0, 1, lane), s1, dk0, 0, 0, 0);
      dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 1, 0, lane), s0, dk1, 0, 0, 0);
      dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 1, 1, lane), s1, dk1, 0, 0, 0);
    }
    if (krow < SL) {
      bf16_t* row = dqkv + ((size_t)rb + krow) * pitch + h * 64;
      if (R.cos_tab) unrope_acc_pre(dk0, dk1, rc, rs);
      store_t(row + d, dk0, dk1, 1.f, hi);
      store_t(row + 2 * d, dv0, dv1, 1.f, hi);
    }
  }
}

// (the launch: a block walks the list of 33 .. 64-row samples with the grid's stride; the per-sample body is a real call so that its
//  registers are allocated once, not around the loop - inlined the loop form spilled 31 vector and 97 scalar registers)
__global__ void __launch_bounds__(128, 2) attn_bwd_long_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                               const float* __restrict__ lse, const int32_t* __restrict__ key_len,
                                                               bf16_t* __restrict__ dqkv, int B, int S, int H, int causal, Rope R, Drop D,
                                                               const int32_t* __restrict__ row_base, const int32_t* __restrict__ long_list) {
  // long_list (may be NULL): [0] = number n of 33 .. 64-row samples, [1 .. n] their indices, [1 + B ..] their first rows, [1 + 2 B ..] their row
  // counts (varlen_scan_kernel; all four words of a block's first item are requested together: one round trip); NULL = every block tests
  // its own sample
  int n_items = B;
  int b0 = blockIdx.z, rb0 = 0, sl0 = 0;
  if (long_list) {
    const int it = min((int)blockIdx.z, B - 1);
    n_items = long_list[0];
    b0 = long_list[1 + it]; rb0 = long_list[1 + B + it]; sl0 = long_list[1 + 2 * B + it];
    n_items = min(n_items, B);
  }
#pragma unroll 1
  for (int it = blockIdx.z; it < n_items; it += gridDim.z) {
    const bool first = it == (int)blockIdx.z;
    const int b = long_list ? (first ? b0 : long_list[1 + it]) : it;
    const int rb = long_list ? (first ? rb0 : long_list[1 + B + it]) : (row_base ? row_base[b] : b * S);
    const int kl = long_list ? (first ? sl0 : long_list[1 + 2 * B + it]) : (key_len ? key_len[b] : S);
    const int SL = row_base ? kl : S;
    if (SL <= 32 || SL > 64) continue;      // (block-uniform)
    __syncthreads();                         // (the previous item's tiles and tables are consumed)
    attn_bwd_long_item(qkv, dout, lse, dqkv, b, rb, SL, kl, S, H, causal, R, D);
  }
}

// rows <= 32: one wave holds the whole (batch, head) problem, so the backward is ONE launch: the K, Q and dO tiles go to
// LDS once (V stays in registers), then the dQ part (scores transposed, lane = query; it also yields the softmax-backward row
// term delta) and the dK/dV part (lane = key) run back to back on the same tiles.  Same arithmetic as attn_bwd_dq_kernel +
// attn_bwd_dkv_kernel except that delta comes from P and dP in registers instead of rowsum(dO * O).  Launched for S <= 64: a sample with
// more than 32 rows is attn_bwd_long_kernel's (above) and exits here.
__global__ void __launch_bounds__(64, 3) attn_bwd_small_kernel(const bf16_t* __restrict__ qkv,
                                                               const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                               const int32_t* __restrict__ key_len, bf16_t* __restrict__ dqkv,
                                                               int B, int S, int H, int causal, Rope Rin, Rope R, Drop D,
                                                               const int32_t* __restrict__ row_base) {
  __shared__ __attribute__((aligned(16))) unsigned char kt[4096];
  __shared__ __attribute__((aligned(16))) unsigned char qt[4096];
  __shared__ __attribute__((aligned(16))) unsigned char dot_[4096];
  __shared__ float lse_s[32], dl_s[32];
  const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  // var-len token layout (row_base): sample b owns rows [rb, rb + SL) of the token-major buffers; padded layout: rb = b * S, SL = S
  const int rb = row_base ? row_base[b] : b * S;
  const int SL = row_base ? key_len[b] : S;
  const int d = H * 64;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const bf16_t* dob = dout + (size_t)rb * d + h * 64;
  const int klen = key_len ? key_len[b] : S;
  const Rope Rnone{nullptr, nullptr, nullptr, S};
  if (SL > 32) return;      // (wave-uniform: the sample is attn_bwd_long_kernel's)
  // (one tile at a time: issuing all 17 loads of a problem before the first wait - or K + V first, then Q + dO - measured SLOWER,
  //  29.4 / 28.7 against 23.4 us: with all 3072 problems resident at once the chip's memory queues overflow; profiles/r03_step_experiments.txt, item 14)
  load_tile_coop<64>(kt, kb, 0, SL, pitch, lane, Rin, b);
  // V is only ever read row-wise (operand rows = keys): its fragments come straight from global memory, which keeps the
  // block at 12 KiB of LDS = 12 single-wave blocks per CU, i.e. B*H = 3072 problems of the headline shape in ONE round
  bf16x8_t vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) vf[s] = frag_global(vb, l31, SL, pitch, s, lane);
  load_tile_coop<64>(qt, qb, 0, SL, pitch, lane, Rin, b);
  load_tile_coop<64>(dot_, dob, 0, SL, (size_t)d, lane, Rnone, b);
  const float nlse2 = -lse[((size_t)b * H + h) * S + min(l31, S - 1)] * kLog2e;
  // the lane's angle-table pieces (dq / dk of row l31 are rotated back at the end of each half): requested here, ahead of the matrix
  // work - at the point of use the position -> table chain is two dependent global round trips with nothing left to cover them
  float4 rc[4], rs[4];
  if (R.cos_tab) rope_fetch(R, rope_pos(R, b, min(l31, S - 1)), hi, rc, rs);
  if (hi == 0) lse_s[l31] = nlse2;
  __syncthreads();
  const unsigned bh = b * H + h;
  {   // ---------------- dQ^T[dh][q] = K^T dS^T   (lane owns query l31)
    const int qrow = l31;
    const unsigned dbase = drop_base(D, bh, qrow, 0);
    f32x16_t dp = zero16(), sc = zero16();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[s], frag_rows(dot_, s, lane), dp, 0, 0, 0);
      sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(kt, s, lane), frag_rows(qt, s, lane), sc, 0, 0, 0);
    }
    // the whole key range of a query sits in this lane and its partner (lane ^ 32), so the softmax-backward row term
    // delta = sum_k P~[q,k] dP[q,k] (P~ = dropped P; equal to rowsum(dO * O), which the long-sequence kernels read from the
    // saved output) comes straight from the registers: no read of O
    float dl = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = acc_row(r, hi);
      const bool ok = key < klen && (!causal || key <= qrow) && qrow < SL;
      const float p = ok ? fast_exp2(fmaf(sc[r], kScaleL2, nlse2)) : 0.f;
      const float t = dp[r] * drop_mul_x(D, dbase + (unsigned)(key >> 1) * 0xC2B2AE3Du, key & 1);
      dl = fmaf(p, t, dl);
      sc[r] = p;
      dp[r] = t;
    }
    dl += __shfl_xor(dl, 32, 64);
    if (hi == 0) dl_s[l31] = -dl;
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[r] = sc[r] * (dp[r] - dl) * kScale;
    const bf16x8_t ds0 = acc_to_b(sc, 0), ds1 = acc_to_b(sc, 1);
    f32x16_t a0 = zero16(), a1 = zero16();
    a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(kt, 0, 0, lane), ds0, a0, 0, 0, 0);
    a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(kt, 0, 1, lane), ds1, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(kt, 1, 0, lane), ds0, a1, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(kt, 1, 1, lane), ds1, a1, 0, 0, 0);
    if (qrow < SL) {
      if (R.cos_tab) unrope_acc_pre(a0, a1, rc, rs);
      store_t(dqkv + ((size_t)rb + qrow) * pitch + h * 64, a0, a1, 1.f, hi);
    }
  }
  __syncthreads();   // dl_s (written above) is read per query below
  {   // ---------------- dV^T = dO^T P, dK^T = Q^T dS   (lane owns key l31)
    const int krow = l31;
    const bool key_ok = krow < klen;
    const unsigned dbase = drop_base(D, bh, 0, (unsigned)krow >> 1);
    f32x16_t sc = zero16(), dp = zero16();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(qt, s, lane), frag_rows(kt, s, lane), sc, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(dot_, s, lane), vf[s], dp, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = acc_row(r, hi);
      const bool ok = key_ok && q < SL && (!causal || krow <= q);
      const float p = ok ? fast_exp2(fmaf(sc[r], kScaleL2, lse_s[q])) : 0.f;
      const float dm = drop_mul_x(D, dbase + (unsigned)q * 0x85EBCA77u, krow & 1);
      sc[r] = p * dm;
      dp[r] = p * fmaf(dp[r], dm, dl_s[q]) * kScale;
    }
    const bf16x8_t p0 = acc_to_b(sc, 0), p1 = acc_to_b(sc, 1);
    const bf16x8_t s0 = acc_to_b(dp, 0), s1 = acc_to_b(dp, 1);
    f32x16_t dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
    dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 0, 0, lane), p0, dv0, 0, 0, 0);
    dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 0, 1, lane), p1, dv0, 0, 0, 0);
    dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 1, 0, lane), p0, dv1, 0, 0, 0);
    dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 1, 1, lane), p1, dv1, 0, 0, 0);
    dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 0, 0, lane), s0, dk0, 0, 0, 0);
    dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 0, 1, lane), s1, dk0, 0, 0, 0);
    dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 1, 0, lane), s0, dk1, 0, 0, 0);
    dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 1, 1, lane), s1, dk1, 0, 0, 0);
    if (krow < SL) {
      bf16_t* row = dqkv + ((size_t)rb + krow) * pitch + h * 64;
      if (R.cos_tab) unrope_acc_pre(dk0, dk1, rc, rs);
      store_t(row + d, dk0, dk1, 1.f, hi);
      store_t(row + 2 * d, dv0, dv1, 1.f, hi);
    }
  }
}

// ================================================================================================
// S <= 32, one WORKGROUP per sample (round 5): attention of all H heads, the o projection + residual add and the RMSNorm behind it in
// ONE launch.  Graph sequences of the headline workload are ~22 tokens: a sample is a single 32-row tile, and the three launches it
// replaces (attn_fwd_kernel<1> 11.9 us + the N = K = d GEMM 15.9 us + rmsnorm_fwd 6.1 us per layer at T = 5696) are latency chains,
// not work - the GEMM offers only 180 tiles to 256 CUs and spends most of its time in prologue / epilogue.
//   phase 1  wave h = head h: the single-tile form of attn_fwd_kernel<1> (same arithmetic, same dropout hash); the normalised output
//            tile goes to global memory (the backward and the o weight gradient read it) AND to an LDS tile O[32][d] (bf16)
//   phase 2  Y^T[n][q] = Wo[n][:] . O[q][:] on v_mfma_f32_16x16x32_bf16: wave w owns output channels [64 w, 64 w + 64); the Wo
//            fragments come straight from global memory into registers, from a FRAGMENT-MAJOR copy of the weight (pack_wo_kernel:
//            the 64 lanes' 16-byte pieces of one 16 x 32 MFMA operand are 1 KiB contiguous).  In the weight's own row-major layout a
//            fragment is 16 rows x 64 bytes with ADJACENT LANES IN DIFFERENT ROWS: the texture addresser coalesces neighbouring lanes
//            only, so that form issues 64 separate 16-byte requests per instruction - measured 5.9 TB/s over the chip = 10 B/clk per
//            CU, the whole launch 50.8 us against 36.0 us for the three launches it replaces (profiles/r05_attn_oproj_experiments.txt).
//            The O fragments come from LDS; residual added on the fp32 accumulator, ONE bf16 rounding (as the GEMM epilogue does),
//            the tile x_mid[32][d] goes back to LDS, the rows' sums of squares to a [H][32] table
//   phase 3  all threads: x_mid and xn = w * bf16(x_mid * rstd) (hf LlamaRMSNorm.forward :62-67) leave in whole 16-byte row pieces
// What bounds it: every sample streams the d x d weight through its CU's vector cache once (1.18 MB at 64 B/clk = 7.7 us for d = 768).
// reference: hf LlamaAttention.forward :243-281 (o_proj), LlamaDecoderLayer.forward :305-316 (residual, post_attention_layernorm).
// ================================================================================================
// LDS-DMA helpers (used by the per-sample kernels below and by the long-sequence kernels further down)
__device__ __forceinline__ void attn_glds16(const void* gsrc, const unsigned char* lds_dst) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(LDS_AS const void*)lds_dst);
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(dst)
      : "memory");
}
// piece p (0..7) of a 64-row stage array: rows [8p, 8p+8) x 128 B; lane -> (row, LDS slot), source chunk = slot ^ f(row)
__device__ __forceinline__ void stage_piece(unsigned char* arr, const bf16_t* __restrict__ base, size_t pitch, int r0, int row_lim,
                                            int p, int lane) {
  const int row = p * 8 + (lane >> 3), slot = lane & 7;
  const int x = (row >> 1) & 7;
  const int f = ((x & 1) << 2) | (x >> 1);
  const int gr = max(min(r0 + row, row_lim - 1), 0);
  attn_glds16(base + (size_t)gr * pitch + ((slot ^ f) << 3), arr + p * 1024);
}
__device__ __forceinline__ void attn_vm_wait0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Fragment-major copies of a [d][d] weight for the per-sample kernels below: fwd[((T KS + s) * 64 + lane) * 8 + e] = W[16 T + (lane & 15)]
// [32 s + 8 (lane >> 4) + e] (the A operand of v_mfma_f32_16x16x32_bf16 for rows 16 T .. 16 T + 15, contraction 32 s .. 32 s + 31; KS = d / 32),
// and the same of the TRANSPOSED weight in bwd (rows = W's columns).  One block per 64 x 64 tile of W; grid (d / 64, d / 64, layers).
__global__ void __launch_bounds__(256) pack_wo_kernel(const bf16_t* __restrict__ w0, size_t layer_stride, bf16_t* __restrict__ fwd,
                                                      bf16_t* __restrict__ bwd, int d) {
  __shared__ bf16_t tile[64][72];
  const int n0 = blockIdx.x * 64, k0 = blockIdx.y * 64, KS = d / 32;
  const bf16_t* w = w0 + (size_t)blockIdx.z * layer_stride;
  bf16_t* fo = fwd + (size_t)blockIdx.z * d * d;
  bf16_t* bo = bwd + (size_t)blockIdx.z * d * d;
  for (int c = threadIdx.x; c < 512; c += 256) {
    const int r = c >> 3, ch = c & 7;
    *reinterpret_cast<uint4*>(&tile[r][ch * 8]) = *reinterpret_cast<const uint4*>(w + (size_t)(n0 + r) * d + k0 + ch * 8);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 512; c += 256) {
    const int fr = c >> 6, lane = c & 63, li = lane & 15, g4 = lane >> 4;
    const int tl = fr >> 1, sl = fr & 1;      // 4 row tiles x 2 contraction steps inside the 64 x 64 block
    // forward: rows n, contraction k
    const uint4 v = *reinterpret_cast<const uint4*>(&tile[16 * tl + li][32 * sl + 8 * g4]);
    *reinterpret_cast<uint4*>(fo + ((size_t)((n0 / 16 + tl) * KS + (k0 / 32 + sl)) * 64 + lane) * 8) = v;
    // backward: rows k, contraction n (a column of the tile)
    bf16_t t8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t8[e] = tile[32 * sl + 8 * g4 + e][16 * tl + li];
    uint4 u;
    u.x = t8[0] | ((unsigned)t8[1] << 16); u.y = t8[2] | ((unsigned)t8[3] << 16);
    u.z = t8[4] | ((unsigned)t8[5] << 16); u.w = t8[6] | ((unsigned)t8[7] << 16);
    *reinterpret_cast<uint4*>(bo + ((size_t)((k0 / 16 + tl) * KS + (n0 / 32 + sl)) * 64 + lane) * 8) = u;
  }
}

#ifndef GGET_AO_PD_LONG
#define GGET_AO_PD_LONG 2   // the same for a 33 .. 64-row sample of the backward (64 accumulators per lane beside them: 3 and 4 spill inside the K loop)
#endif
#ifndef GGET_AO_PD
#define GGET_AO_PD 4      // K-steps of weight fragments in flight in the per-sample kernels (measurement knob: -DGGET_AO_PD=n)
#endif
// bf16 elements of padding per LDS row of the [32][d] tiles: the pitch is (d + 16) * 2 bytes = TWO 16-byte slots past a multiple of 16 slots.
// ds_read_b128 serves a wave in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH.md, LDS): in the MFMA
// operand READ (lane = row l & 15, chunk l >> 4) a group holds every row once with chunk c or c + 1, so slot = 2 row + chunk meets no
// bank twice; with ONE slot of padding (the first version) rows 11 / chunk 1 and 12 / chunk 0 met: SQ_LDS_BANK_CONFLICT / IDX_ACTIVE
// 0.32 - 0.37.  The reads are what the pitch is chosen for; the row-strided WRITES into the tile still collide - a row is 392 dwords =
// 8 mod 32 banks, so the O pieces of rows r and r + 4 (phase 1, 16-byte stores) and the x_mid pieces of every fourth row (phase 2,
// 8-byte stores) share banks: the forward kernel's 0.25 in profiles/r05_final_c1_pmc_mfma_lds.txt (the backward, whose tile is written
// by whole rows, 0.05).  ~12 store instructions per lane against ~50 operand reads: left as it is.
constexpr int kOPad = 16;
// LDS bytes of the per-sample forward: the [32][d + pad] tile, the sums of squares [H][32] + rstd [32], the waves' two 4 KiB tiles
template <int H>
constexpr int attn_oproj_fwd_lds() { return 32 * (H * 64 + kOPad) * 2 + (H * 32 + 32) * 4 + H * 8192; }

template <int H>
__global__ void __launch_bounds__(H * 64) attn_oproj_fwd_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ key_len,
                                                                const int32_t* __restrict__ row_base, bf16_t* __restrict__ attn_out,
                                                                float* __restrict__ lse, const bf16_t* __restrict__ wo,
                                                                const bf16_t* __restrict__ x_in, bf16_t* __restrict__ x_mid,
                                                                const bf16_t* __restrict__ nw, bf16_t* __restrict__ xn,
                                                                float* __restrict__ rstd_out, int B, int S, int causal, float eps, Drop D) {
  constexpr int d = H * 64, NT = H * 64, PITCH = (d + kOPad) * 2, KSTEPS = d / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char fa_lds[];
  unsigned char* otile = fa_lds;                                   // [32][PITCH]: O, later x_mid
  float* ss_part = reinterpret_cast<float*>(fa_lds + 32 * PITCH);  // [H][32] sums of squares, then [32] rstd behind it
  float* rstd_s = ss_part + H * 32;
  unsigned char* kv = fa_lds + 32 * PITCH + (H * 32 + 32) * 4;     // per wave: K tile, V tile (4 KiB each)
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int h = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  const int rb = row_base ? row_base[b] : b * S;
  const int SL = row_base ? key_len[b] : S;                        // rows of this sample in the token-major buffers
  const int klen = key_len ? min(key_len[b], S) : S;
  const size_t pitch = (size_t)3 * d;
  const int li = lane & 15, g4 = lane >> 4;
  // K order of phase 2: every workgroup streams the SAME weight; started at the same K-step they would all hit the same L2 lines at
  // the same time, so workgroup b starts at K-step (5 b) mod KSTEPS (wave-uniform: scalar address arithmetic)
  const int rot = __builtin_amdgcn_readfirstlane((b * 5) % KSTEPS);
  const bf16_t* wrow = wo + (size_t)4 * h * KSTEPS * 512 + lane * 8;   // packed: fragment (n-tile 4 h + t, K-step s) at ((4 h + t) KSTEPS + s) * 512
  constexpr int PD = GGET_AO_PD;         // K-steps of weight fragments in flight: PD x 4 16-byte loads per lane
  uint4 af[PD][4];
  // ---------------------------------------------------------------- phase 1: attention of head h (single 32 x 32 tile)
  {
    unsigned char* kt = kv + h * 8192;
    unsigned char* vt = kt + 4096;
    const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
    const bf16_t* kb = qb + d;
    const bf16_t* vb = qb + 2 * d;
    const int qrow = l31;
    const Rope Rnone{nullptr, nullptr, nullptr, S};
    bf16x8_t qf[4];
    frags_global_rope(qf, qb, qrow, SL, pitch, lane, Rnone, b);
    // (global loads first, then - behind them in the queue - the first weight fragments of phase 2: they stream in under the attention)
    uint4 kraw[4], vraw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + i * 64, row = c >> 3, ch = c & 7;
      kraw[i] = *reinterpret_cast<const uint4*>(kb + (size_t)clamp_row(row, SL) * pitch + ch * 8);
      vraw[i] = *reinterpret_cast<const uint4*>(vb + (size_t)clamp_row(row, SL) * pitch + ch * 8);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < PD; ++s) {
      const int sr = (s + rot) % KSTEPS;
#pragma unroll
      for (int t = 0; t < 4; ++t) af[s][t] = *reinterpret_cast<const uint4*>(wrow + (size_t)(t * KSTEPS + sr) * 512);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + i * 64, row = c >> 3, ch = c & 7;
      *reinterpret_cast<uint4*>(kt + swz(row, ch * 16)) = zero_if(row >= SL, kraw[i]);
      *reinterpret_cast<uint4*>(vt + swz(row, ch * 16)) = zero_if(row >= SL, vraw[i]);
    }
    __syncthreads();
    f32x16_t sc = zero16();
#pragma unroll
    for (int s = 0; s < 4; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(kt, s, lane), qf[s], sc, 0, 0, 0);
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = acc_row(r, hi);
      const bool ok = key < klen && (!causal || key <= qrow);
      sc[r] = ok ? sc[r] : -INFINITY;
      mx = fmaxf(mx, sc[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m = mx * kScaleL2;
    const bool dead = m == -INFINITY;
    const float nm = dead ? 0.f : -m;
    const unsigned dbase = drop_base(D, b * H + h, qrow, 0);
    float l = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = fast_exp2(fmaf(sc[r], kScaleL2, nm));
      l += p;                                                        // softmax normaliser: before dropout
      sc[r] = p * drop_mul_x(D, dbase + (unsigned)(acc_row(r, hi) >> 1) * 0xC2B2AE3Du, r & 1);
    }
    l += __shfl_xor(l, 32, 64);
    const bf16x8_t pb0 = acc_to_b(sc, 0), pb1 = acc_to_b(sc, 1);
    f32x16_t o0 = zero16(), o1 = zero16();
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 0, 0, lane), pb0, o0, 0, 0, 0);
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 0, 1, lane), pb1, o0, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 1, 0, lane), pb0, o1, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 1, 1, lane), pb1, o1, 0, 0, 0);
    const float inv = l > 0.f ? 1.f / l : 0.f;
    const bool live = qrow < SL;
    bf16_t* grow = attn_out + ((size_t)rb + min(qrow, max(SL - 1, 0))) * d + h * 64;
    unsigned char* lrow = otile + qrow * PITCH + h * 128;
    // (store_t's piece trade: the hi = 0 lane of a row ends up with the 16 bytes dh [8 rr, 8 rr + 8) of the even rr, the hi = 1 lane
    //  with those of the odd rr)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const f32x16_t& a = half ? o1 : o0;
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        const int e = 2 * pr, o = 2 * pr + 1;
        const unsigned e0 = pack2bf(a[4 * e + 0] * inv, a[4 * e + 1] * inv), e1 = pack2bf(a[4 * e + 2] * inv, a[4 * e + 3] * inv);
        const unsigned q0_ = pack2bf(a[4 * o + 0] * inv, a[4 * o + 1] * inv), q1_ = pack2bf(a[4 * o + 2] * inv, a[4 * o + 3] * inv);
        const hw_u32x2_t w0 = __builtin_amdgcn_permlane32_swap(e0, q0_, false, false);
        const hw_u32x2_t w1 = __builtin_amdgcn_permlane32_swap(e1, q1_, false, false);
        uint4 v;
        v.x = w0[0]; v.y = w1[0]; v.z = w0[1]; v.w = w1[1];
        const int off = 32 * half + 8 * (hi ? o : e);
        if (live) *reinterpret_cast<uint4*>(grow + off) = v;
        *reinterpret_cast<uint4*>(lrow + off * 2) = live ? v : make_uint4(0u, 0u, 0u, 0u);
      }
    }
    if (hi == 0 && live && lse) lse[((size_t)b * H + h) * S + qrow] = l > 0.f ? (m + log2f(l)) * (1.0f / kLog2e) : 0.f;
  }
  __syncthreads();
  // ---------------------------------------------------------------- phase 2: Y^T = Wo O^T, + residual, sums of squares
  {
    f32x4_t acc[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[t][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const unsigned char* orow = otile + li * PITCH + 16 * g4;           // + 16 u rows, + 64 s bytes
    // The scheduling fences keep the issue order written here (without them the compiler sinks every weight load to just before its
    // MFMA - one or two in flight, the loop then runs at the latency of an L2 round trip per K-step); the O fragments are fetched one
    // K-step ahead.  K-step s of the loop is K-step (s + rot) mod KSTEPS of the matrices.
    int sw = rot + PD; if (sw >= KSTEPS) sw -= KSTEPS;      // K-step the next weight load fetches
    int sb = rot;                                           // K-step of the O fragments in bq[s & 1]
    // the lane's residual values x_in[q = 16 u + li][n = 64 h + 16 t + 4 g4 + i] (8 bytes each): fetched under the K loop
    uint2 res[4][2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int q = 16 * u + li;
      const bf16_t* rrow = x_in + ((size_t)rb + min(q, max(SL - 1, 0))) * d + 64 * h + 4 * g4;
#pragma unroll
      for (int t = 0; t < 4; ++t) res[t][u] = *reinterpret_cast<const uint2*>(rrow + 16 * t);
    }
    __builtin_amdgcn_sched_barrier(0);
    uint4 bq[2][2];
    bq[0][0] = *reinterpret_cast<const uint4*>(orow + 64 * sb);
    bq[0][1] = *reinterpret_cast<const uint4*>(orow + 16 * PITCH + 64 * sb);
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      bf16x8_t a[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) a[t] = __builtin_bit_cast(bf16x8_t, af[s % PD][t]);
      __builtin_amdgcn_sched_barrier(0);
      if (s + PD < KSTEPS) {
#pragma unroll
        for (int t = 0; t < 4; ++t) af[s % PD][t] = *reinterpret_cast<const uint4*>(wrow + (size_t)(t * KSTEPS + sw) * 512);
        if (++sw == KSTEPS) sw = 0;
      }
      if (s + 1 < KSTEPS) {
        if (++sb == KSTEPS) sb = 0;
        bq[(s + 1) & 1][0] = *reinterpret_cast<const uint4*>(orow + 64 * sb);
        bq[(s + 1) & 1][1] = *reinterpret_cast<const uint4*>(orow + 16 * PITCH + 64 * sb);
      }
      __builtin_amdgcn_sched_barrier(0);
      const bf16x8_t b0 = __builtin_bit_cast(bf16x8_t, bq[s & 1][0]), b1 = __builtin_bit_cast(bf16x8_t, bq[s & 1][1]);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b0, acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b1, acc[t][1], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();     // every wave has read its O fragments: the tile is overwritten with x_mid
    float ssq[2] = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float r0 = acc[t][u][0] + __uint_as_float(res[t][u].x << 16), r1 = acc[t][u][1] + __uint_as_float(res[t][u].x & 0xffff0000u);
        const float r2 = acc[t][u][2] + __uint_as_float(res[t][u].y << 16), r3 = acc[t][u][3] + __uint_as_float(res[t][u].y & 0xffff0000u);
        uint2 o;
        o.x = pack2bf(r0, r1); o.y = pack2bf(r2, r3);
        const float f0 = __uint_as_float(o.x << 16), f1 = __uint_as_float(o.x & 0xffff0000u);
        const float f2 = __uint_as_float(o.y << 16), f3 = __uint_as_float(o.y & 0xffff0000u);
        ssq[u] += f0 * f0 + f1 * f1 + f2 * f2 + f3 * f3;
        *reinterpret_cast<uint2*>(otile + (16 * u + li) * PITCH + (64 * h + 16 * t + 4 * g4) * 2) = o;
      }
      // fold the four 16-lane rows (same token, other channels)
      hw_u32x2_t r = __builtin_amdgcn_permlane16_swap(__float_as_uint(ssq[u]), __float_as_uint(ssq[u]), false, false);
      ssq[u] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
      r = __builtin_amdgcn_permlane32_swap(__float_as_uint(ssq[u]), __float_as_uint(ssq[u]), false, false);
      ssq[u] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
      if (g4 == 0) ss_part[h * 32 + 16 * u + li] = ssq[u];
    }
  }
  __syncthreads();
  if (tid < 32) {
    float ss = 0.f;
#pragma unroll
    for (int w = 0; w < H; ++w) ss += ss_part[w * 32 + tid];
    const float rs = rsqrtf(ss / (float)d + eps);
    rstd_s[tid] = rs;
    if (tid < SL && rstd_out) rstd_out[rb + tid] = rs;
  }
  __syncthreads();
  // ---------------------------------------------------------------- phase 3: x_mid and xn leave in 16-byte row pieces
  constexpr int CPR = d / 8;
#pragma unroll
  for (int i = 0; i < (32 * CPR + NT - 1) / NT; ++i) {
    const int c = tid + i * NT;
    if (c >= 32 * CPR) break;
    const int q = c / CPR, cc = c % CPR;
    if (q >= SL) continue;
    const uint4 xv = *reinterpret_cast<const uint4*>(otile + q * PITCH + cc * 16);
    float v[8], wv[8], o[8];
    unpack8(xv, v);
    unpack8(*reinterpret_cast<const uint4*>(nw + cc * 8), wv);
    const float rs = rstd_s[q];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = wv[e] * bf2f(f2bf(v[e] * rs));
    *reinterpret_cast<uint4*>(x_mid + ((size_t)rb + q) * d + cc * 8) = xv;
    *reinterpret_cast<uint4*>(xn + ((size_t)rb + q) * d + cc * 8) = pack8(o);
  }
}

// The backward counterpart, one workgroup per sample (S <= 32): RMSNorm backward of post_attention_layernorm, the dgrad of the o
// projection and the attention backward of every head in ONE launch (three launches before: rmsnorm_bwd 10.9 us + the N = K = d NN GEMM
// 16.6 us + attn_bwd_small_kernel 21 us per layer at T = 5696).
//   phase A  wave w owns rows w, w + H, ...: dx_mid = dres + rstd (dy w - xhat mean(dy w xhat)) exactly as rmsnorm_bwd_kernel; the row
//            goes to global memory (the o weight gradient and the next RMSNorm backward read it) and to an LDS tile; the norm weight's
//            gradient is pre-reduced over the block's rows, one fp32 atomic per channel and block
//   phase B  dattn^T[k][q] = WoT[k][:] . dx_mid[q][:] (fragment-major copy of the TRANSPOSED weight, pack_wo_kernel); wave w owns the 64
//            channels of head w and writes them, rounded to bf16 like the GEMM's output, into its own swizzled dO tile - dattn never
//            exists in global memory
//   phase C  wave w: attn_bwd_small_kernel's arithmetic on head w (K, Q tiles from global memory, V in registers, dO from phase B)
// reference: hf LlamaRMSNorm :62-67, LlamaAttention.forward :243-281, eager_attention_forward :191-214 (their autograd).
// A sample of 33 .. 64 rows inside attn_oproj_bwd_kernel (round 6; var-len layout, S <= 64).  The collator pads a batch to the width of its
// LONGEST graph (reference src/data/collator.py:70-111): at B = 256 the width is 40 - 56 while nineteen graphs in twenty are one 32-row tile,
// so the kernel is keyed on each sample's own row count.  The long sample stays ONE workgroup (a second workgroup per extra tile would be a
// second round on a 256-CU chip at B = 256): phases A and B over
// two row tiles with the transposed weight streamed ONCE, dattn of these rows written to global memory (bf16, the GEMM's rounding) - the
// attention backward of such samples is attn_bwd_long_kernel's, launched behind this kernel on the same stream: its 24 KiB of K / Q / dO
// tiles per HEAD do not fit beside this workgroup's row tiles (twelve heads: 288 KiB).
//   phase A  wave w owns rows w, w + H, ...: rows 0 .. 31 go to region X, rows 32 .. 63 to region Y behind the waves' norm-weight partials
//   phase B  four 16-row blocks per weight fragment, two K-steps of fragments in flight
// A real call (own register allocation), decided by the kernel's first statements.
template <int H>
__device__ __attribute__((noinline)) void attn_oproj_bwd_long(const bf16_t* __restrict__ dxn, const bf16_t* __restrict__ x_mid,
                                                              const bf16_t* __restrict__ nw, const float* __restrict__ rstd,
                                                              const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx_mid,
                                                              float* __restrict__ dw_accum, int copies, uint64_t copy_stride,
                                                              const bf16_t* __restrict__ wot, bf16_t* __restrict__ dattn, int b, int rb, int SL) {
  constexpr int d = H * 64, NT = H * 64, PITCH = (d + kOPad) * 2, KSTEPS = d / 32, NCHUNK = d / 8, NCH = (NCHUNK + 63) / 64;
  constexpr int XB = 32 * PITCH > H * 4096 ? 32 * PITCH : H * 4096, YB = H * 8192 > H * d * 4 ? H * 8192 : H * d * 4;
  static_assert(H * d * 4 + 32 * PITCH <= YB, "the second row tile sits behind the norm-weight partials in region Y");
  extern __shared__ __attribute__((aligned(16))) unsigned char fb_lds[];
  unsigned char* dtile0 = fb_lds;
  float* dw_lds = reinterpret_cast<float*>(fb_lds + XB);
  unsigned char* dtile1 = fb_lds + XB + H * d * 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int h = __builtin_amdgcn_readfirstlane(tid >> 6);
  // ---------------------------------------------------------------- phase A: RMSNorm backward of this wave's rows (of 64)
  {
    float wv[NCH][8], dwp[NCH][8];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
#pragma unroll
      for (int e = 0; e < 8; ++e) { dwp[i][e] = 0.f; wv[i][e] = 0.f; }
      if (c < NCHUNK) unpack8(*reinterpret_cast<const uint4*>(nw + c * 8), wv[i]);
    }
    constexpr int RPW = (64 + H - 1) / H, RB = RPW < 3 ? RPW : 3;
#pragma unroll 1
    for (int j0 = 0; j0 < RPW; j0 += RB) {
      uint4 xr[RB][NCH], dr[RB][NCH], rr[RB][NCH];
      float rs[RB];
#pragma unroll
      for (int jj = 0; jj < RB; ++jj) {
        const int q = h + H * (j0 + jj);
        const size_t row = (size_t)rb + max(min(q, SL - 1), 0);
        rs[jj] = rstd[row];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
          const int c = min(lane + i * 64, NCHUNK - 1);
          xr[jj][i] = *reinterpret_cast<const uint4*>(x_mid + row * d + c * 8);
          dr[jj][i] = *reinterpret_cast<const uint4*>(dxn + row * d + c * 8);
          rr[jj][i] = *reinterpret_cast<const uint4*>(dres + row * d + c * 8);
        }
      }
#pragma unroll
      for (int jj = 0; jj < RB; ++jj) {
        const int q = h + H * (j0 + jj);
        if (q >= 64) break;                    // (wave-uniform)
        const bool live = q < SL;
        unsigned char* trow = q < 32 ? dtile0 + q * PITCH : dtile1 + (q - 32) * PITCH;
        float xh[NCH][8], g[NCH][8], res[NCH][8];
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
          const bool on = lane + i * 64 < NCHUNK;
          float xv[8], dv[8];
          unpack8(xr[jj][i], xv);
          unpack8(dr[jj][i], dv);
          unpack8(rr[jj][i], res[i]);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            xh[i][e] = xv[e] * rs[jj];
            g[i][e] = dv[e] * wv[i][e];
            if (on) dot += g[i][e] * xh[i][e];
            if (on && live) dwp[i][e] += dv[e] * xh[i][e];
          }
        }
        dot = wave_sum(dot) / (float)d;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
          const int c = lane + i * 64;
          if (c < NCHUNK) {
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = res[i][e] + rs[jj] * (g[i][e] - xh[i][e] * dot);
            const uint4 ov = live ? pack8(o) : make_uint4(0u, 0u, 0u, 0u);
            *reinterpret_cast<uint4*>(trow + c * 16) = ov;
            if (live) *reinterpret_cast<uint4*>(dx_mid + ((size_t)rb + q) * d + c * 8) = ov;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
      if (c < NCHUNK) {
        *reinterpret_cast<float4*>(dw_lds + h * d + c * 4) = make_float4(dwp[i][0], dwp[i][1], dwp[i][2], dwp[i][3]);
        *reinterpret_cast<float4*>(dw_lds + h * d + (d >> 1) + c * 4) = make_float4(dwp[i][4], dwp[i][5], dwp[i][6], dwp[i][7]);
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < d; t += NT) {
    constexpr int hd = d >> 1;
    const int pl = t >= hd ? 1 : 0, ix = t - pl * hd;
    const int j = (ix >> 2) * 8 + pl * 4 + (ix & 3);
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < H; ++w) sum += dw_lds[w * d + t];
    unsafeAtomicAdd(dw_accum + (size_t)(blockIdx.x % copies) * copy_stride + j, sum);
  }
  // ---------------------------------------------------------------- phase B: dattn^T = WoT dx_mid^T over 64 rows -> global memory
  {
    const int li = lane & 15, g4 = lane >> 4;
    const int rot = __builtin_amdgcn_readfirstlane((b * 5) % KSTEPS);
    f32x4_t acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[t][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const bf16_t* wrow = wot + (size_t)4 * h * KSTEPS * 512 + lane * 8;
    const unsigned char* orow0 = dtile0 + li * PITCH + 16 * g4;
    const unsigned char* orow1 = dtile1 + li * PITCH + 16 * g4;
    constexpr int PD = GGET_AO_PD_LONG;
    uint4 af[PD][4];
#pragma unroll
    for (int s = 0; s < PD; ++s) {
      const int sr = (s + rot) % KSTEPS;
#pragma unroll
      for (int t = 0; t < 4; ++t) af[s][t] = *reinterpret_cast<const uint4*>(wrow + (size_t)(t * KSTEPS + sr) * 512);
    }
    int sw = rot + PD; if (sw >= KSTEPS) sw -= KSTEPS;
    int sb = rot;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      bf16x8_t a[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) a[t] = __builtin_bit_cast(bf16x8_t, af[s % PD][t]);
      uint4 bq[4];
      bq[0] = *reinterpret_cast<const uint4*>(orow0 + 64 * sb);
      bq[1] = *reinterpret_cast<const uint4*>(orow0 + 16 * PITCH + 64 * sb);
      bq[2] = *reinterpret_cast<const uint4*>(orow1 + 64 * sb);
      bq[3] = *reinterpret_cast<const uint4*>(orow1 + 16 * PITCH + 64 * sb);
      if (++sb == KSTEPS) sb = 0;
      __builtin_amdgcn_sched_barrier(0);
      if (s + PD < KSTEPS) {
#pragma unroll
        for (int t = 0; t < 4; ++t) af[s % PD][t] = *reinterpret_cast<const uint4*>(wrow + (size_t)(t * KSTEPS + sw) * 512);
        if (++sw == KSTEPS) sw = 0;
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bf16x8_t bb = __builtin_bit_cast(bf16x8_t, bq[u]);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], bb, acc[t][u], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // lane holds dattn[q = 16 u + li][64 h + 16 t + 4 g4 + i]: 8 bytes of row q
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = 16 * u + li;
      if (q < SL) {
        bf16_t* grow = dattn + ((size_t)rb + q) * d + 64 * h + 4 * g4;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          uint2 o;
          o.x = pack2bf(acc[t][u][0], acc[t][u][1]);
          o.y = pack2bf(acc[t][u][2], acc[t][u][3]);
          *reinterpret_cast<uint2*>(grow + 16 * t) = o;
        }
      }
    }
  }
}

template <int H>
__global__ void __launch_bounds__(H * 64) attn_oproj_bwd_kernel(const bf16_t* __restrict__ dxn, const bf16_t* __restrict__ x_mid,
                                                                const bf16_t* __restrict__ nw, const float* __restrict__ rstd,
                                                                const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx_mid,
                                                                float* __restrict__ dw_accum, int copies, uint64_t copy_stride,
                                                                const bf16_t* __restrict__ wot, const bf16_t* __restrict__ qkv,
                                                                const float* __restrict__ lse, const int32_t* __restrict__ key_len,
                                                                const int32_t* __restrict__ row_base, bf16_t* __restrict__ dqkv, int B, int S,
                                                                int causal, Rope R, Drop D, int t_rows, bf16_t* __restrict__ dattn_long) {
  constexpr int d = H * 64, NT = H * 64, PITCH = (d + kOPad) * 2, KSTEPS = d / 32, NCHUNK = d / 8, NCH = (NCHUNK + 63) / 64;
  // LDS: region X = the dx_mid tile [32][PITCH] of phases A / B, overwritten by the heads' dO tiles [H][4096] once phase B's loop is
  // over; region Y = the heads' K and Q tiles [H][8192] (they arrive by LDS-DMA while phase B runs), whose first bytes hold the waves'
  // norm-weight gradient partials [H][d] during phase A
  constexpr int XB = 32 * PITCH > H * 4096 ? 32 * PITCH : H * 4096, YB = H * 8192 > H * d * 4 ? H * 8192 : H * d * 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char fb_lds[];
  unsigned char* dtile = fb_lds;
  unsigned char* dot_all = fb_lds;
  unsigned char* kq = fb_lds + XB;
  float* dw_lds = reinterpret_cast<float*>(fb_lds + XB);
  float* stat = reinterpret_cast<float*>(fb_lds + XB + YB);         // [H][64]: -lse * log2(e) and -delta per query
  float* rope_lds = stat + H * 64;                                  // cos [32][kRopePitch], sin [32][kRopePitch] of the sample's rows
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int h = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  const int rb = row_base ? row_base[b] : b * S;
  const int SL = row_base ? key_len[b] : S;
  if (SL > 32) {     // (workgroup-uniform; var-len layout with 32 < S <= 64 only: the launcher sees to that)
    if (b == B - 1)
      for (int c = (rb + SL) * NCHUNK + tid; c < t_rows * NCHUNK; c += NT) reinterpret_cast<uint4*>(dx_mid)[c] = make_uint4(0u, 0u, 0u, 0u);
    attn_oproj_bwd_long<H>(dxn, x_mid, nw, rstd, dres, dx_mid, dw_accum, copies, copy_stride, wot, dattn_long, b, rb, min(SL, 64));
    return;
  }
  const int klen = key_len ? min(key_len[b], S) : S;
  // Angle-table rows of the sample's 32 positions (phase C rotates dq and dk back): requested NOW (position, then its table piece: two
  // dependent global round trips) and parked in LDS behind phase A; the unrotation at the end of phase C reads LDS.  Fetched at the
  // point of use the chain sat exposed at the very end of the kernel, twice: 41.1 us per launch inside the step; requested at the top of
  // phase C 39.3 us; this form: profiles/r05_step_experiments.txt item 12.
  constexpr int RPC = (512 + NT - 1) / NT;       // 2 tables x 32 rows x 8 pieces of 16 bytes over the block's threads
  float4 rope_piece[RPC];
#pragma unroll
  for (int i = 0; i < RPC; ++i) {
    const int t = tid + i * NT;
    rope_piece[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (R.cos_tab && t < 512) {
      const int row = (t >> 3) & 31, q4 = t & 7;
      const int pos = rope_pos(R, b, min(row, S - 1));
      rope_piece[i] = *reinterpret_cast<const float4*>((t < 256 ? R.cos_tab : R.sin_tab) + (size_t)pos * 32 + q4 * 4);
    }
  }
  // var-len layout: the <= 63 pad rows behind the last sample belong to no workgroup; their gradient is zero (rmsnorm_bwd_kernel computed
  // exactly that from their zero inputs) and must read as zero in the o weight gradient (K = all rows) and the next RMSNorm backward
  if (row_base && b == B - 1)
    for (int c = (rb + SL) * NCHUNK + tid; c < t_rows * NCHUNK; c += NT) reinterpret_cast<uint4*>(dx_mid)[c] = make_uint4(0u, 0u, 0u, 0u);
  // ---------------------------------------------------------------- phase A: RMSNorm backward of this wave's rows
  {
    float wv[NCH][8], dwp[NCH][8];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
#pragma unroll
      for (int e = 0; e < 8; ++e) { dwp[i][e] = 0.f; wv[i][e] = 0.f; }
      if (c < NCHUNK) unpack8(*reinterpret_cast<const uint4*>(nw + c * 8), wv[i]);
    }
    constexpr int RPW = (32 + H - 1) / H, RB = RPW < 3 ? RPW : 3;
    for (int j0 = 0; j0 < RPW; j0 += RB) {
      uint4 xr[RB][NCH], dr[RB][NCH], rr[RB][NCH];
      float rs[RB];
#pragma unroll
      for (int jj = 0; jj < RB; ++jj) {
        const int q = h + H * (j0 + jj);
        const size_t row = (size_t)rb + max(min(q, SL - 1), 0);
        rs[jj] = rstd[row];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
          const int c = min(lane + i * 64, NCHUNK - 1);
          xr[jj][i] = *reinterpret_cast<const uint4*>(x_mid + row * d + c * 8);
          dr[jj][i] = *reinterpret_cast<const uint4*>(dxn + row * d + c * 8);
          rr[jj][i] = *reinterpret_cast<const uint4*>(dres + row * d + c * 8);
        }
      }
#pragma unroll
      for (int jj = 0; jj < RB; ++jj) {
        const int q = h + H * (j0 + jj);
        if (q >= 32) break;                    // (wave-uniform)
        const bool live = q < SL;
        float xh[NCH][8], g[NCH][8], res[NCH][8];
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
          const bool on = lane + i * 64 < NCHUNK;
          float xv[8], dv[8];
          unpack8(xr[jj][i], xv);
          unpack8(dr[jj][i], dv);
          unpack8(rr[jj][i], res[i]);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            xh[i][e] = xv[e] * rs[jj];
            g[i][e] = dv[e] * wv[i][e];
            if (on) dot += g[i][e] * xh[i][e];
            if (on && live) dwp[i][e] += dv[e] * xh[i][e];
          }
        }
        dot = wave_sum(dot) / (float)d;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
          const int c = lane + i * 64;
          if (c < NCHUNK) {
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = res[i][e] + rs[jj] * (g[i][e] - xh[i][e] * dot);
            const uint4 ov = live ? pack8(o) : make_uint4(0u, 0u, 0u, 0u);
            *reinterpret_cast<uint4*>(dtile + q * PITCH + c * 16) = ov;
            if (live) *reinterpret_cast<uint4*>(dx_mid + ((size_t)rb + q) * d + c * 8) = ov;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
      if (c < NCHUNK) {   // (two planes of d / 2 floats per wave, as rmsnorm_bwd_kernel: neighbouring lanes store neighbouring 16 bytes)
        *reinterpret_cast<float4*>(dw_lds + h * d + c * 4) = make_float4(dwp[i][0], dwp[i][1], dwp[i][2], dwp[i][3]);
        *reinterpret_cast<float4*>(dw_lds + h * d + (d >> 1) + c * 4) = make_float4(dwp[i][4], dwp[i][5], dwp[i][6], dwp[i][7]);
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < d; t += NT) {
    constexpr int hd = d >> 1;
    const int pl = t >= hd ? 1 : 0, ix = t - pl * hd;
    const int j = (ix >> 2) * 8 + pl * 4 + (ix & 3);
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < H; ++w) sum += dw_lds[w * d + t];
    unsafeAtomicAdd(dw_accum + (size_t)(blockIdx.x % copies) * copy_stride + j, sum);
  }
  if (R.cos_tab) {     // (its own LDS region; read behind phase B's barriers)
#pragma unroll
    for (int i = 0; i < RPC; ++i) {
      const int t = tid + i * NT;
      if (t < 512) *reinterpret_cast<float4*>(rope_lds + ((t < 256 ? 0 : 32) + ((t >> 3) & 31)) * kRopePitch + (t & 7) * 4) = rope_piece[i];
    }
  }
  __syncthreads();     // the partials are consumed: region Y takes the K / Q tiles
  unsigned char* kt = kq + h * 8192;
  unsigned char* qt = kt + 4096;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  // K and Q tile of head h by LDS-DMA (no registers; rows beyond the sample are clamped - finite - and masked below): in flight under phase B
#pragma unroll
  for (int pc = 0; pc < 4; ++pc) {
    stage_piece(kt, kb, pitch, 0, SL, pc, lane);
    stage_piece(qt, qb, pitch, 0, SL, pc, lane);
  }
  // ---------------------------------------------------------------- phase B: dattn^T = WoT dx_mid^T -> this head's dO tile
  unsigned char* dot_ = dot_all + h * 4096;
  bf16x8_t vf[4];
  {
    const int li = lane & 15, g4 = lane >> 4;
    const int rot = __builtin_amdgcn_readfirstlane((b * 5) % KSTEPS);      // (see attn_oproj_fwd_kernel)
    f32x4_t acc[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[t][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const bf16_t* wrow = wot + (size_t)4 * h * KSTEPS * 512 + lane * 8;
    const unsigned char* orow = dtile + li * PITCH + 16 * g4;
    constexpr int PD = GGET_AO_PD;
    uint4 af[PD][4];
#pragma unroll
    for (int s = 0; s < PD; ++s) {
      const int sr = (s + rot) % KSTEPS;
#pragma unroll
      for (int t = 0; t < 4; ++t) af[s][t] = *reinterpret_cast<const uint4*>(wrow + (size_t)(t * KSTEPS + sr) * 512);
    }
    int sw = rot + PD; if (sw >= KSTEPS) sw -= KSTEPS;
    int sb = rot;
    uint4 bq[2][2];
    bq[0][0] = *reinterpret_cast<const uint4*>(orow + 64 * sb);
    bq[0][1] = *reinterpret_cast<const uint4*>(orow + 16 * PITCH + 64 * sb);
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      bf16x8_t a[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) a[t] = __builtin_bit_cast(bf16x8_t, af[s % PD][t]);
      __builtin_amdgcn_sched_barrier(0);
      if (s + PD < KSTEPS) {
#pragma unroll
        for (int t = 0; t < 4; ++t) af[s % PD][t] = *reinterpret_cast<const uint4*>(wrow + (size_t)(t * KSTEPS + sw) * 512);
        if (++sw == KSTEPS) sw = 0;
      }
      if (s + 1 < KSTEPS) {
        if (++sb == KSTEPS) sb = 0;
        bq[(s + 1) & 1][0] = *reinterpret_cast<const uint4*>(orow + 64 * sb);
        bq[(s + 1) & 1][1] = *reinterpret_cast<const uint4*>(orow + 16 * PITCH + 64 * sb);
      }
      __builtin_amdgcn_sched_barrier(0);
      const bf16x8_t b0 = __builtin_bit_cast(bf16x8_t, bq[s & 1][0]), b1 = __builtin_bit_cast(bf16x8_t, bq[s & 1][1]);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b0, acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b1, acc[t][1], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // V is only ever read row-wise (operand rows = keys): its fragments come straight from global memory, under the barrier below
#pragma unroll
    for (int s = 0; s < 4; ++s) vf[s] = frag_global(vb, l31, SL, pitch, s, lane);
    __syncthreads();     // every wave is done with the dx_mid tile: its bytes become the dO tiles
    // lane holds dattn[q = 16 u + li][64 h + 16 t + 4 g4 + i]: 8 bytes of row q of the head's [32][64] tile
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        uint2 o;
        o.x = pack2bf(acc[t][u][0], acc[t][u][1]);
        o.y = pack2bf(acc[t][u][2], acc[t][u][3]);
        *reinterpret_cast<uint2*>(dot_ + swz(16 * u + li, (16 * t + 4 * g4) * 2)) = o;
      }
  }
  // ---------------------------------------------------------------- phase C: attention backward of head h (attn_bwd_small_kernel)
  {
    float* lse_s = stat + h * 64;
    float* dl_s = lse_s + 32;
    attn_vm_wait0();     // the K / Q tiles (DMA) have landed
    const float nlse2 = -lse[((size_t)b * H + h) * S + min(l31, S - 1)] * kLog2e;
    if (hi == 0) lse_s[l31] = nlse2;
    __syncthreads();
    const unsigned bh = b * H + h;
    {   // dQ^T[dh][q] = K^T dS^T   (lane owns query l31)
      const int qrow = l31;
      const unsigned dbase = drop_base(D, bh, qrow, 0);
      f32x16_t dp = zero16(), sc = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[s], frag_rows(dot_, s, lane), dp, 0, 0, 0);
        sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(kt, s, lane), frag_rows(qt, s, lane), sc, 0, 0, 0);
      }
      float dl = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = acc_row(r, hi);
        const bool ok = key < klen && (!causal || key <= qrow) && qrow < SL;
        const float p = ok ? fast_exp2(fmaf(sc[r], kScaleL2, nlse2)) : 0.f;
        const float t = dp[r] * drop_mul_x(D, dbase + (unsigned)(key >> 1) * 0xC2B2AE3Du, key & 1);
        dl = fmaf(p, t, dl);
        sc[r] = p;
        dp[r] = t;
      }
      dl += __shfl_xor(dl, 32, 64);
      if (hi == 0) dl_s[l31] = -dl;
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = sc[r] * (dp[r] - dl) * kScale;
      const bf16x8_t ds0 = acc_to_b(sc, 0), ds1 = acc_to_b(sc, 1);
      f32x16_t a0 = zero16(), a1 = zero16();
      a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(kt, 0, 0, lane), ds0, a0, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(kt, 0, 1, lane), ds1, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(kt, 1, 0, lane), ds0, a1, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(kt, 1, 1, lane), ds1, a1, 0, 0, 0);
      if (qrow < SL) {
        if (R.cos_tab) {
          float4 rc[4], rs[4];
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            rc[rr] = *reinterpret_cast<const float4*>(rope_lds + l31 * kRopePitch + 8 * rr + 4 * hi);
            rs[rr] = *reinterpret_cast<const float4*>(rope_lds + (32 + l31) * kRopePitch + 8 * rr + 4 * hi);
          }
          unrope_acc_pre(a0, a1, rc, rs);
        }
        store_t(dqkv + ((size_t)rb + qrow) * pitch + h * 64, a0, a1, 1.f, hi);
      }
    }
    __syncthreads();   // dl_s
    {   // dV^T = dO^T P, dK^T = Q^T dS   (lane owns key l31)
      const int krow = l31;
      const bool key_ok = krow < klen;
      const unsigned dbase = drop_base(D, bh, 0, (unsigned)krow >> 1);
      f32x16_t sc = zero16(), dp = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(qt, s, lane), frag_rows(kt, s, lane), sc, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(dot_, s, lane), vf[s], dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = acc_row(r, hi);
        const bool ok = key_ok && q < SL && (!causal || krow <= q);
        const float p = ok ? fast_exp2(fmaf(sc[r], kScaleL2, lse_s[q])) : 0.f;
        const float dm = drop_mul_x(D, dbase + (unsigned)q * 0x85EBCA77u, krow & 1);
        sc[r] = p * dm;
        dp[r] = p * fmaf(dp[r], dm, dl_s[q]) * kScale;
      }
      const bf16x8_t p0 = acc_to_b(sc, 0), p1 = acc_to_b(sc, 1);
      const bf16x8_t s0 = acc_to_b(dp, 0), s1 = acc_to_b(dp, 1);
      f32x16_t dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
      dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 0, 0, lane), p0, dv0, 0, 0, 0);
      dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 0, 1, lane), p1, dv0, 0, 0, 0);
      dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 1, 0, lane), p0, dv1, 0, 0, 0);
      dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 1, 1, lane), p1, dv1, 0, 0, 0);
      dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 0, 0, lane), s0, dk0, 0, 0, 0);
      dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 0, 1, lane), s1, dk0, 0, 0, 0);
      dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 1, 0, lane), s0, dk1, 0, 0, 0);
      dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 1, 1, lane), s1, dk1, 0, 0, 0);
      if (krow < SL) {
        bf16_t* row = dqkv + ((size_t)rb + krow) * pitch + h * 64;
        if (R.cos_tab) {
          float4 rc[4], rs[4];
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            rc[rr] = *reinterpret_cast<const float4*>(rope_lds + l31 * kRopePitch + 8 * rr + 4 * hi);
            rs[rr] = *reinterpret_cast<const float4*>(rope_lds + (32 + l31) * kRopePitch + 8 * rr + 4 * hi);
          }
          unrope_acc_pre(dk0, dk1, rc, rs);
        }
        store_t(row + d, dk0, dk1, 1.f, hi);
        store_t(row + 2 * d, dv0, dv1, 1.f, hi);
      }
    }
  }
}

// ================================================================================================
// Long-sequence kernels (S >= 256, q / k already rotated in memory - the engine's layout): 8 waves per block = 256 rows
// of one (batch, head); the operand that is streamed (K and V, or Q and dO) arrives by LDS-DMA in stages of 64 rows
// (2 arrays x 8 KiB, two [32][128 B] swizzled tiles each) through a double buffer: ONE barrier per 64 rows, the next stage's
// DMA is issued right behind it and flies under the 16-32 MFMAs + softmax of the current one; no VALU work for loading
// (the swizzle is a permutation of the per-lane source chunk, the LDS image of a piece is lane-linear).  The per-32x32 math
// is the one of the kernels above (transposed scores, lane-local statistics, P^T feeds the next MFMA from registers), with
// the paired dropout hash (one multiply per two scores where the lane walks along keys).  Rows beyond the sequence are
// clamped (finite) and masked.  Packed rows: the block's union of key ranges bounds the stage loop, so whole stages are
// neither loaded nor computed.
// ================================================================================================
// the block's 8 waves load one stage (two arrays): wave w issues pieces w and w + 8
__device__ __forceinline__ void stage_issue(unsigned char* buf /* [2][8192] */, const bf16_t* __restrict__ a0, size_t pitch0,
                                            const bf16_t* __restrict__ a1, size_t pitch1, int r0, int row_lim, int wave, int lane) {
  stage_piece(buf, a0, pitch0, r0, row_lim, wave, lane);
  stage_piece(buf + 8192, a1, pitch1, r0, row_lim, wave, lane);
}

// block-wide min / max of two small ints through LDS (packed rows: union of the waves' key ranges)
__device__ __forceinline__ void block_range(int& lo, int& hi, int* red /* [16] */, int wave, int lane) {
  if (lane == 0) { red[wave] = lo; red[8 + wave] = hi; }
  __syncthreads();
  int l = red[0], h = red[8];
#pragma unroll
  for (int i = 1; i < 8; ++i) { l = min(l, red[i]); h = max(h, red[8 + i]); }
  lo = l; hi = h;
  __syncthreads();
}

// Forward: a wave owns QT = 2 consecutive 32-query tiles, so every K fragment (ds_read_b128) and every transposed V fragment
// (ds_read_b64_tr_b16 pair) read from LDS feeds two MFMAs (the 32-query version spends one LDS KiB per MFMA: half of the CU's LDS
// bandwidth at full matrix rate) and the two score accumulators are independent MFMA chains.  Block = NWB waves.
template <bool PK, int QT, int NWB>
__global__ void __launch_bounds__(NWB * 64, QT == 1 ? 4 : 2) attn_fwd64_kernel(const bf16_t* __restrict__ qkv, KeyRange KR, bf16_t* __restrict__ out,
                                                                 float* __restrict__ lse, int B, int S, int H, int causal, Drop D) {
  __shared__ __attribute__((aligned(16))) unsigned char st[2][2 * 8192];
  __shared__ int red[16];
  constexpr int QB = NWB * QT * 32;   // queries per block
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.y, b = blockIdx.z;
  // var-len token layout (KR.row_base): sample b owns rows [rb, rb + SL) of the token-major buffers; padded layout: rb = b * S, SL = S
  const int rb = KR.row_base ? KR.row_base[b] : b * S;
  const int SL = KR.row_base ? KR.key_len[b] : S;
  const int q0 = blockIdx.x * QB + wave * (QT * 32);      // first query of this wave
  const int d = H * 64;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  int qlo[QT], qhi[QT];
  int ulo = S, uhi = -1, ilo = 0, ihi = S - 1;            // union / intersection over the wave's QT * 32 queries
  const int len = KR.key_len ? KR.key_len[b] : S;
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qrow = q0 + 32 * t + l31;
    qlo[t] = 0; qhi[t] = len - 1;
    if (PK) {
      const bool v = qrow < SL;
      qlo[t] = v ? KR.lo[(size_t)b * S + qrow] : 0;
      qhi[t] = v ? KR.hi[(size_t)b * S + qrow] : -1;
      ulo = min(ulo, wave_imin(qhi[t] >= qlo[t] ? qlo[t] : S)); uhi = max(uhi, wave_imax(qhi[t] >= qlo[t] ? qhi[t] + 1 : 0) - 1);
      ilo = max(ilo, wave_imax(v ? qlo[t] : 0)); ihi = min(ihi, wave_imin(v ? qhi[t] + 1 : S) - 1);
    }
  }
  if (!PK) { ulo = 0; uhi = len - 1; ilo = 0; ihi = len - 1; }
  const int klen = PK ? S : len;
  const int q_end_blk = min(SL, (int)(blockIdx.x + 1) * QB);
  int kbeg_blk = 0, kend_blk = causal ? min(klen, q_end_blk) : klen;
  // right padding: queries at or beyond the row's length are padding rows - nothing downstream reads their outputs and their
  // upstream gradient is zero - so a block (and below, a wave) made of them alone does no work and writes zeros
  if (!PK && (int)(blockIdx.x * QB) >= len) kend_blk = 0;
  if (PK) {
    int blo = ulo, bhi = uhi;
    block_range(blo, bhi, red, wave, lane);
    kbeg_blk = min(max(blo, 0), S) & ~63;
    kend_blk = min(kend_blk, bhi + 1);
  }
  const int kend = (q0 < SL && (PK || q0 < len)) ? min(uhi + 1, causal ? q0 + QT * 32 : SL) : 0;   // this wave's own key range

  bf16x8_t qf[QT][4];
  f32x16_t o0[QT], o1[QT];
  float m[QT], l[QT];
  unsigned dbase[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qrow = q0 + 32 * t + l31;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[t][s] = frag_global(qb, qrow, SL, pitch, s, lane);
    o0[t] = zero16(); o1[t] = zero16();
    m[t] = -INFINITY; l[t] = 0.f;
    dbase[t] = drop_base(D, b * H + h, qrow, 0);
  }
  constexpr int PPW = 16 / NWB;     // DMA pieces per wave per stage (16 pieces of 1 KiB: K 8, V 8)
  auto issue = [&](int buf, int r0) {
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int pc = wave * PPW + i;   // 0..15
      if (pc < 8) stage_piece(st[buf], kb, pitch, r0, SL, pc, lane);
      else stage_piece(st[buf] + 8192, vb, pitch, r0, SL, pc - 8, lane);
    }
  };
  const int nst = kend_blk > kbeg_blk ? (kend_blk - kbeg_blk + 63) >> 6 : 0;
  if (nst > 0) issue(0, kbeg_blk);
  for (int t = 0; t < nst; ++t) {
    const int ks = kbeg_blk + t * 64;
    attn_vm_wait0();          // this wave's pieces of stage t have landed
    __syncthreads();          // everyone's have; everyone is done with stage t-1 (the buffer refilled next)
    if (t + 1 < nst) issue((t + 1) & 1, ks + 64);
    const unsigned char* kst = st[t & 1];
    const unsigned char* vst = kst + 8192;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k0 = ks + 32 * j;
      if (k0 >= kend || k0 + 31 < ulo) continue;
      const unsigned char* kt = kst + 4096 * j;
      const unsigned char* vt = vst + 4096 * j;
      f32x16_t sc[QT];
#pragma unroll
      for (int t2 = 0; t2 < QT; ++t2) sc[t2] = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8_t kf = frag_rows(kt, s, lane);
#pragma unroll
        for (int t2 = 0; t2 < QT; ++t2) sc[t2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[t2][s], sc[t2], 0, 0, 0);
      }
      const bool edge = (k0 < ilo) || (k0 + 31 > ihi) || (causal && k0 + 31 > q0) || (q0 + QT * 32 > SL);
      bf16x8_t pb[QT][2];
#pragma unroll
      for (int t2 = 0; t2 < QT; ++t2) {
        const int qrow = q0 + 32 * t2 + l31;
        float mx = -INFINITY;
        if (edge) {
          // (the opaque copy keeps the 31 index / compare instructions of the mask INSIDE this rarely taken branch: hipcc
          // otherwise hoists them above it and every tile pays for them)
          int k0v = k0;
          asm volatile("" : "+v"(k0v));
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0v + acc_row(r, hi);
            const bool ok = key >= qlo[t2] && key <= qhi[t2] && (!causal || key <= qrow);
            sc[t2][r] = ok ? sc[t2][r] : -INFINITY;
            mx = fmaxf(mx, sc[t2][r]);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[t2][r]);
        }
        {
          const hw_u32x2_t sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
          mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        }
        const float m_new = fmaxf(m[t2], mx * kScaleL2);
        const bool dead = m_new == -INFINITY;
        const float alpha = dead ? 1.f : fast_exp2(m[t2] - m_new);
        const float nm = dead ? 0.f : -m_new;
        float rs = 0.f;
        if (D.thresh == 0) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float p = fast_exp2(fmaf(sc[t2][r], kScaleL2, nm));   // masked scores are -inf -> 0
            rs += p;
            sc[t2][r] = p;
          }
        } else {
          // registers (2 rp, 2 rp + 1) are keys (k, k + 1) = one hash word; (k >> 1) = (k0 >> 1) + 2 hi + (rp & 1) + 4 (rp >> 1): the
          // lane's part is one multiply per tile, the register's part a literal.  The keep scale 1 / (1 - p) is applied once to
          // O at the end (l sums the un-dropped probabilities), so a dropped score costs one select.
          const unsigned xb = dbase[t2] + (unsigned)((k0 >> 1) + 2 * hi) * 0xC2B2AE3Du;
#pragma unroll
          for (int rp = 0; rp < 8; ++rp) {
            const unsigned w = drop_word(xb + (unsigned)((rp & 1) + 4 * (rp >> 1)) * 0xC2B2AE3Du);
            const float p0 = fast_exp2(fmaf(sc[t2][2 * rp], kScaleL2, nm));
            const float p1 = fast_exp2(fmaf(sc[t2][2 * rp + 1], kScaleL2, nm));
            rs += p0 + p1;                                      // softmax normaliser: before dropout
            sc[t2][2 * rp] = (w & 0xffffu) < D.thresh ? 0.f : p0;      // what multiplies V (x 1 / (1 - p) at the end)
            sc[t2][2 * rp + 1] = (w >> 16) < D.thresh ? 0.f : p1;
          }
        }
        {
          const hw_u32x2_t sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(rs), __float_as_uint(rs), false, false);
          rs = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
        }
        l[t2] = l[t2] * alpha + rs;
        m[t2] = m_new;
        if (__any(alpha != 1.f)) {
#pragma unroll
          for (int r = 0; r < 16; ++r) { o0[t2][r] *= alpha; o1[t2][r] *= alpha; }
        }
        pb[t2][0] = acc_to_b(sc[t2], 0);
        pb[t2][1] = acc_to_b(sc[t2], 1);
      }
#pragma unroll
      for (int dhb = 0; dhb < 2; ++dhb)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const bf16x8_t vf = frag_tr(vt, dhb, jj, lane);
#pragma unroll
          for (int t2 = 0; t2 < QT; ++t2) {
            if (dhb == 0) o0[t2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pb[t2][jj], o0[t2], 0, 0, 0);
            else o1[t2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pb[t2][jj], o1[t2], 0, 0, 0);
          }
        }
    }
  }
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qrow = q0 + 32 * t + l31;
    if (qrow < SL) {
      const float inv = l[t] > 0.f ? D.inv_keep / l[t] : 0.f;   // (D.inv_keep = 1 without dropout)
      store_t(out + ((size_t)rb + qrow) * d + h * 64, o0[t], o1[t], inv, hi);
      if (hi == 0 && lse) lse[((size_t)b * H + h) * S + qrow] = l[t] > 0.f ? (m[t] + log2f(l[t])) * (1.0f / kLog2e) : 0.f;
    }
  }
}

// Forward for the dense case (one key length per batch row, not causal: fine-tuning batches), software-pipelined inside the
// wave.  Measured on gfx950 (tools/ubench/valu_mfma.hip, profiles/r02_valu_mfma_overlap.txt): a SIMD overlaps MFMA and VALU
// work only when they alternate in ONE wave's instruction stream - "all MFMAs, then all VALU" runs at ~86 % of the SUM of the
// two even with four waves per SIMD, and attn_fwd64_kernel sits exactly there (VALU 67 % + MFMA 30 % busy) - while the softmax
// of a 32x32 tile is more VALU time than its 8 MFMAs.  So step j issues the P.V MFMAs of tile j-1 and the score MFMAs of tile
// j+1 between the softmax instructions of tile j: eight chunks of {one MFMA, one LDS fragment fetch two chunks ahead, an eighth
// of the softmax}, pinned by scheduling fences (the compiler otherwise bunches the MFMAs, and a burst of MFMAs blocks the
// SIMD's vector issue of the other waves).  K stages are needed one tile early and V stages one tile late: two rings of
// three 8 KiB slots (K(t), K(t+1) resident + K(t+2) in flight; V(t-1), V(t) resident + V(t+1) in flight), one barrier per 64
// keys, the stage loop unrolled by three so every LDS address is lane offset + immediate.  All waves of a block see the same
// keys, so the loop is branch-free (the lazy rescale of the running output aside); the last one or two tiles (key_len not
// a multiple of 64) take the sequential masked path.
#define GGET_FENCE() __builtin_amdgcn_sched_barrier(0)
#ifndef GGET_FWD_DENSE_MINW
#define GGET_FWD_DENSE_MINW 4   // waves per SIMD the 8-wave form is compiled for (128 registers, two blocks per CU; 3 / 2 measured: see profiles/r05_step_experiments.txt item 16)
#endif
template <bool DROP, int NWB>
__global__ void __launch_bounds__(NWB * 64, NWB == 8 ? GGET_FWD_DENSE_MINW : 3) attn_fwd_dense_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ key_len,
                                                                                    bf16_t* __restrict__ out, float* __restrict__ lse, int B, int S,
                                                                                    int H, Drop D, const int32_t* __restrict__ row_base) {
  __shared__ __attribute__((aligned(16))) unsigned char kr[3][8192];
  __shared__ __attribute__((aligned(16))) unsigned char vr[3][8192];
  constexpr int QB = NWB * 32;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.y, b = blockIdx.z;
  // var-len token layout (row_base): sample b owns rows [rb, rb + SL) of the token-major buffers; padded layout: rb = b * S, SL = S
  const int rb = row_base ? row_base[b] : b * S;
  const int SL = row_base ? key_len[b] : S;
  const int q0 = blockIdx.x * QB + wave * 32;
  const int d = H * 64;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const int qrow = q0 + l31;
  const int row_len = key_len ? min(key_len[b], S) : S;
  // right padding: queries at or beyond the row's length are padding rows (nothing downstream reads their outputs): a block made of
  // them alone sees an empty key range and writes zeros, a wave made of them alone only feeds the DMA and the barriers
  const int len = (int)(blockIdx.x * QB) < row_len ? row_len : 0;
  const bool w_act = q0 < row_len;                   // wave-uniform
  const int nfull = len >> 5;                        // tiles whose 32 keys are all visible
  const int ntile = (len + 31) >> 5;
  const int nst = (ntile + 1) >> 1;
  const int nfs = nfull >> 1;                        // stages the pipelined loop covers (both tiles full)

  bf16x8_t qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = frag_global(qb, qrow, SL, pitch, s, lane);
  f32x16_t o0 = zero16(), o1 = zero16();
  float m = -INFINITY, l = 0.f;
  const unsigned dbase = drop_base(D, b * H + h, qrow, 0);

  constexpr int PPW = 16 / NWB;
  auto issue = [&](int t, unsigned char* kdst, unsigned char* vdst) {   // at the top of stage t: K(t+2) and V(t+1)
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int pc = wave * PPW + i;
      if (pc < 8) { if (t + 2 < nst) stage_piece(kdst, kb, pitch, (t + 2) * 64, SL, pc, lane); }
      else { if (t + 1 < nst) stage_piece(vdst, vb, pitch, (t + 1) * 64, SL, pc - 8, lane); }
    }
  };
  auto qk = [&](const unsigned char* kt, f32x16_t& sc) {
    sc = zero16();
#pragma unroll
    for (int s = 0; s < 4; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(kt, s, lane), qf[s], sc, 0, 0, 0);
  };
  auto pv = [&](const unsigned char* vt, const bf16x8_t (&pb)[2]) {
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 0, 0, lane), pb[0], o0, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 1, 0, lane), pb[0], o1, 0, 0, 0);
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 0, 1, lane), pb[1], o0, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(vt, 1, 1, lane), pb[1], o1, 0, 0, 0);
  };
  auto rescale = [&](float alpha) {
    if (__any(alpha != 1.f)) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
    }
  };
  // pieces of the softmax of one tile (sc -> probabilities in place)
  const hw_f32x2_t sc2 = {kScaleL2, kScaleL2};
  auto drop_pair = [&](unsigned xb, int rp, hw_f32x2_t& pp2) {
    // registers (2 rp, 2 rp + 1) are keys (k, k + 1) = one hash word (see attn_fwd64_kernel); 1 / (1 - p) is applied at the end
    const unsigned w = drop_word(xb + (unsigned)((rp & 1) + 4 * (rp >> 1)) * 0xC2B2AE3Du);
    pp2[0] = (w & 0xffffu) < D.thresh ? 0.f : pp2[0];
    pp2[1] = (w >> 16) < D.thresh ? 0.f : pp2[1];
  };
  // the sequential form (tail tiles): masked when the tile is the partial one
  auto softmax_seq = [&](int k0, bool edge, f32x16_t& sc, bf16x8_t (&pb)[2]) -> float {
    if (edge) {
      int k0v = k0;
      asm volatile("" : "+v"(k0v));
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = (k0v + acc_row(r, hi) < len) ? sc[r] : -INFINITY;
    }
    float mx = sc[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sc[r]);
    {
      const hw_u32x2_t sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
      mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
    }
    const float m_new = fmaxf(m, mx * kScaleL2);      // finite: key 0 of the tile is visible
    const float alpha = fast_exp2(m - m_new);
    const hw_f32x2_t nm2 = {-m_new, -m_new};
    hw_f32x2_t rs2 = {0.f, 0.f};
    const unsigned xb = DROP ? dbase + (unsigned)((k0 >> 1) + 2 * hi) * 0xC2B2AE3Du : 0u;
#pragma unroll
    for (int rp = 0; rp < 8; ++rp) {
      hw_f32x2_t x = {sc[2 * rp], sc[2 * rp + 1]};
      x = x * sc2 + nm2;
      hw_f32x2_t pp2 = {fast_exp2(x[0]), fast_exp2(x[1])};
      rs2 += pp2;
      if (DROP) drop_pair(xb, rp, pp2);
      sc[2 * rp] = pp2[0]; sc[2 * rp + 1] = pp2[1];
    }
    float rs = rs2[0] + rs2[1];
    {
      const hw_u32x2_t sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(rs), __float_as_uint(rs), false, false);
      rs = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    l = l * alpha + rs;
    m = m_new;
    pb[0] = acc_to_b(sc, 0);
    pb[1] = acc_to_b(sc, 1);
    return alpha;
  };
  // step j (a full tile): O += V_{j-1} P_{j-1} and S_{j+1} = K_{j+1} Q^T on the matrix pipe under softmax(S_j) on the vector pipe
  auto step = [&](int k0, const unsigned char* kt_next, const unsigned char* vt_prev, f32x16_t& sc, f32x16_t& sn, const bf16x8_t (&pp)[2],
                  bf16x8_t (&pc)[2]) {
    // LDS fragments through a ring of four: the V_{j-1} fragments are fetched at the top (the row maximum covers their round
    // trip), chunk i < 4 consumes F[i] and refills it with K_{j+1} row fragment i, consumed four chunks later
    bf16x8_t F[4];
    auto fetch_k = [&](int i) { F[i] = frag_rows(kt_next, i, lane); };
#pragma unroll
    for (int i = 0; i < 4; ++i) F[i] = frag_tr(vt_prev, i & 1, i >> 1, lane);
    float mx = sc[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sc[r]);
    {
      const hw_u32x2_t sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
      mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
    }
    const float m_new = fmaxf(m, mx * kScaleL2);
    const float alpha = fast_exp2(m - m_new);
    const unsigned xb = DROP ? dbase + (unsigned)((k0 >> 1) + 2 * hi) * 0xC2B2AE3Du : 0u;
    const float nm = -m_new;
    float rsa = 0.f, rsb = 0.f;
    auto arg = [&](int rp) {
      sc[2 * rp] = fmaf(sc[2 * rp], kScaleL2, nm);
      sc[2 * rp + 1] = fmaf(sc[2 * rp + 1], kScaleL2, nm);
    };
    auto ex2 = [&](int rp) {   // two pairs: four exps back to back, then their sums (single-instruction f32 ops: see build.py)
      float e0 = fast_exp2(sc[2 * rp]), e1 = fast_exp2(sc[2 * rp + 1]), e2 = fast_exp2(sc[2 * rp + 2]), e3 = fast_exp2(sc[2 * rp + 3]);
      rsa += e0; rsb += e1; rsa += e2; rsb += e3;
      if (DROP) {
        hw_f32x2_t pa = {e0, e1}, pb2 = {e2, e3};
        drop_pair(xb, rp, pa); drop_pair(xb, rp + 1, pb2);
        e0 = pa[0]; e1 = pa[1]; e2 = pb2[0]; e3 = pb2[1];
      }
      sc[2 * rp] = e0; sc[2 * rp + 1] = e1; sc[2 * rp + 2] = e2; sc[2 * rp + 3] = e3;
    };
    GGET_FENCE();
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F[0], pp[0], o0, 0, 0, 0);
    fetch_k(0);
    arg(0); arg(1); arg(2); arg(3); ex2(0);
    GGET_FENCE();
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F[1], pp[0], o1, 0, 0, 0);
    fetch_k(1);
    ex2(2); arg(4); arg(5); arg(6); arg(7);
    GGET_FENCE();
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F[2], pp[1], o0, 0, 0, 0);
    fetch_k(2);
    ex2(4);
    GGET_FENCE();
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F[3], pp[1], o1, 0, 0, 0);
    fetch_k(3);
    ex2(6);
    GGET_FENCE();
    sn = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F[0], qf[0], zero16(), 0, 0, 0);
    float rs = rsa + rsb;
    {
      const hw_u32x2_t sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(rs), __float_as_uint(rs), false, false);
      rs = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    l = l * alpha + rs;
    m = m_new;
    pc[0] = acc_to_b(sc, 0);
    GGET_FENCE();
    sn = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F[1], qf[1], sn, 0, 0, 0);
    pc[1] = acc_to_b(sc, 1);
    GGET_FENCE();
    sn = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F[2], qf[2], sn, 0, 0, 0);
    GGET_FENCE();
    sn = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F[3], qf[3], sn, 0, 0, 0);
    rescale(alpha);
  };

  // prologue: K(0), K(1), V(0); the V slot "before stage 0" is zeroed (step 0 multiplies it by P = 0)
  if (nst > 0) {
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int pc = wave * PPW + i;
      if (pc < 8) {
        stage_piece(kr[0], kb, pitch, 0, SL, pc, lane);
        if (nst > 1) stage_piece(kr[1], kb, pitch, 64, SL, pc, lane);
      } else stage_piece(vr[0], vb, pitch, 0, SL, pc - 8, lane);
    }
  }
  for (int i = tid; i < 512; i += NWB * 64) reinterpret_cast<uint4*>(vr[2])[i] = make_uint4(0, 0, 0, 0);
  attn_vm_wait0();
  __syncthreads();
  f32x16_t sA = zero16(), sB = zero16();
  bf16x8_t pA[2], pB[2];
  {
    const uint4 z = make_uint4(0, 0, 0, 0);
    pB[0] = pB[1] = pA[0] = pA[1] = __builtin_bit_cast(bf16x8_t, z);
  }
  if (ntile > 0 && w_act) qk(kr[0], sA);
  auto stage = [&](int t, auto SL) {
    constexpr int sl = decltype(SL)::value, s1 = (sl + 1) % 3, s2 = (sl + 2) % 3;
    attn_vm_wait0();                // K(t+1), V(t): issued one stage ago
    __syncthreads();                // ... by everyone; everyone is past stage t-1
    issue(t, kr[s2], vr[s1]);
    if (w_act) {
      step(64 * t, kr[sl] + 4096, vr[s2] + 4096, sA, sB, pB, pA);         // tile 2t:   K tile 2t+1, V tile 2t-1
      step(64 * t + 32, kr[s1], vr[sl], sB, sA, pA, pB);                  // tile 2t+1: K tile 2t+2, V tile 2t
    }
  };
  int t = 0;
  while (t < nfs) {
    stage(t, std::integral_constant<int, 0>{}); if (++t >= nfs) break;
    stage(t, std::integral_constant<int, 1>{}); if (++t >= nfs) break;
    stage(t, std::integral_constant<int, 2>{}); ++t;
  }
  // tail: the pending P.V of tile 2 nfs - 1, then at most two more tiles (a full one and / or the partial one), sequentially
  if (nfs < nst) {
    attn_vm_wait0();
    __syncthreads();
  }
  if (nfs > 0 && w_act) pv(vr[(nfs - 1) % 3] + 4096, pB);
  const int jt = 2 * nfs;
  if (jt < ntile && w_act) {
    rescale(softmax_seq(32 * jt, jt >= nfull, sA, pA));
    pv(vr[nfs % 3], pA);
  }
  if (jt + 1 < ntile && w_act) {
    qk(kr[nfs % 3] + 4096, sB);
    rescale(softmax_seq(32 * jt + 32, true, sB, pB));
    pv(vr[nfs % 3] + 4096, pB);
  }
  if (qrow < SL) {
    const float inv = l > 0.f ? D.inv_keep / l : 0.f;
    store_t(out + ((size_t)rb + qrow) * d + h * 64, o0, o1, inv, hi);
    if (hi == 0 && lse) lse[((size_t)b * H + h) * S + qrow] = l > 0.f ? (m + log2f(l)) * (1.0f / kLog2e) : 0.f;
  }
}

// dQ for long sequences: same stage machinery as attn_fwd64_kernel (K and V streamed), one 32-query tile per wave.
template <bool PK, int NWB>
__global__ void __launch_bounds__(NWB * 64, NWB == 4 ? 3 : 4) attn_bwd_dq64_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out,
                                                                    const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                                    float* __restrict__ delta, KeyRange KR, bf16_t* __restrict__ dqkv,
                                                                    int B, int S, int H, int causal, Drop D, Rope Rout) {
  __shared__ __attribute__((aligned(16))) unsigned char st[2][2 * 8192];
  __shared__ int red[16];
  constexpr int QB = NWB * 32;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.y, b = blockIdx.z;
  // var-len token layout (KR.row_base): sample b owns rows [rb, rb + SL) of the token-major buffers; padded layout: rb = b * S, SL = S
  const int rb = KR.row_base ? KR.row_base[b] : b * S;
  const int SL = KR.row_base ? KR.key_len[b] : S;
  const int q0 = blockIdx.x * QB + wave * 32;
  const int d = H * 64;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const bf16_t* dob = dout + (size_t)rb * d + h * 64;
  const int qrow = q0 + l31;
  const int len = KR.key_len ? KR.key_len[b] : S;
  int qlo = 0, qhi = len - 1;
  int ulo = 0, uhi = qhi, ilo = 0, ihi = qhi;
  if (PK) {
    const bool v = qrow < SL;
    qlo = v ? KR.lo[(size_t)b * S + qrow] : 0;
    qhi = v ? KR.hi[(size_t)b * S + qrow] : -1;
    ulo = wave_imin(qhi >= qlo ? qlo : S); uhi = wave_imax(qhi >= qlo ? qhi + 1 : 0) - 1;
    ilo = wave_imax(v ? qlo : 0); ihi = wave_imin(v ? qhi + 1 : S) - 1;
  }
  const int klen = PK ? S : len;
  const int q_end_blk = min(SL, (int)(blockIdx.x + 1) * QB);
  int kbeg_blk = 0, kend_blk = causal ? min(klen, q_end_blk) : klen;
  // right padding: queries at or beyond the row's length are padding rows - nothing downstream reads their outputs and their
  // upstream gradient is zero - so a block (and below, a wave) made of them alone does no work and writes zeros
  if (!PK && (int)(blockIdx.x * QB) >= len) kend_blk = 0;
  if (PK) {
    int blo = ulo, bhi = uhi;
    block_range(blo, bhi, red, wave, lane);
    kbeg_blk = min(max(blo, 0), S) & ~63;
    kend_blk = min(kend_blk, bhi + 1);
  }
  const int kend = (q0 < SL && (PK || q0 < len)) ? min(uhi + 1, causal ? q0 + 32 : SL) : 0;

  bf16x8_t qf[4], dof[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = frag_global(qb, qrow, SL, pitch, s, lane);
    dof[s] = frag_global(dob, qrow, SL, (size_t)d, s, lane);
  }
  const size_t sidx = ((size_t)b * H + h) * S + min(qrow, S - 1);
  float dl = 0.f;   // delta_q = rowsum(dO * O): the softmax-backward row term, stored for the dK/dV kernel
  {
    const bf16_t* ob = out + (size_t)rb * d + h * 64;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float a[8], gg[8];
      unpack8(__builtin_bit_cast(uint4, frag_global(ob, qrow, SL, (size_t)d, s, lane)), a);
      unpack8(__builtin_bit_cast(uint4, dof[s]), gg);
#pragma unroll
      for (int e = 0; e < 8; ++e) dl += a[e] * gg[e];
    }
    const hw_u32x2_t sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(dl), __float_as_uint(dl), false, false);
    dl = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    if (hi == 0 && qrow < SL) delta[sidx] = dl;
  }
  const float nlse2 = -lse[sidx] * kLog2e;
  const float ndl_k = -dl * kScale;                        // ds = p * (dp * keep * scale - delta * scale)
  const float keep_k = D.inv_keep * kScale;
  const unsigned dbase = drop_base(D, b * H + h, qrow, 0);
  f32x16_t a0 = zero16(), a1 = zero16();
  constexpr int PPW = 16 / NWB;
  auto issue = [&](int buf, int r0) {
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int pc = wave * PPW + i;
      if (pc < 8) stage_piece(st[buf], kb, pitch, r0, SL, pc, lane);
      else stage_piece(st[buf] + 8192, vb, pitch, r0, SL, pc - 8, lane);
    }
  };
  const int nst = kend_blk > kbeg_blk ? (kend_blk - kbeg_blk + 63) >> 6 : 0;
  if (nst > 0) issue(0, kbeg_blk);
  // (the stage loop is unrolled by two: with a static buffer every LDS address is lane offset + immediate, which is what lets the
  // 8-wave build stay inside 128 registers)
  auto stage = [&](int t, auto BUF) {
    constexpr int buf = decltype(BUF)::value;
    const int ks = kbeg_blk + t * 64;
    attn_vm_wait0();
    __syncthreads();
    if (t + 1 < nst) issue(buf ^ 1, ks + 64);
    const unsigned char* kst = st[buf];
    const unsigned char* vst = kst + 8192;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k0 = ks + 32 * j;
      if (k0 >= kend || k0 + 31 < ulo) continue;
      const unsigned char* kt = kst + 4096 * j;
      const unsigned char* vt = vst + 4096 * j;
      f32x16_t dp = zero16(), sc = zero16();
      {   // fenced: two LDS fragments in flight (unfenced, the scheduler hoists every read of the tile and the 128-register build spills)
        bf16x8_t fa = frag_rows(kt, 0, lane), fb = frag_rows(vt, 0, lane);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, qf[s], sc, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb, dof[s], dp, 0, 0, 0);
          if (s < 3) { fa = frag_rows(kt, s + 1, lane); fb = frag_rows(vt, s + 1, lane); }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      const bool edge = (k0 < ilo) || (k0 + 31 > ihi) || (causal && k0 + 31 > q0) || (q0 + 32 > SL);
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = fast_exp2(fmaf(sc[r], kScaleL2, nlse2));      // P (un-dropped)
      if (edge) {
        int k0v = k0;
        asm volatile("" : "+v"(k0v));    // keeps the mask arithmetic inside this rarely taken branch
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = k0v + acc_row(r, hi);
          sc[r] = (key >= qlo && key <= qhi && (!causal || key <= qrow) && qrow < SL) ? sc[r] : 0.f;
        }
      }
      if (D.thresh == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = sc[r] * fmaf(dp[r], kScale, ndl_k);
      } else {
        const unsigned xb = dbase + (unsigned)((k0 >> 1) + 2 * hi) * 0xC2B2AE3Du;
#pragma unroll
        for (int rp = 0; rp < 8; ++rp) {
          const unsigned w = drop_word(xb + (unsigned)((rp & 1) + 4 * (rp >> 1)) * 0xC2B2AE3Du);
          const float k0m = (w & 0xffffu) < D.thresh ? 0.f : keep_k;
          const float k1m = (w >> 16) < D.thresh ? 0.f : keep_k;
          sc[2 * rp] = sc[2 * rp] * fmaf(dp[2 * rp], k0m, ndl_k);
          sc[2 * rp + 1] = sc[2 * rp + 1] * fmaf(dp[2 * rp + 1], k1m, ndl_k);
        }
      }
      const bf16x8_t ds0 = acc_to_b(sc, 0), ds1 = acc_to_b(sc, 1);
      __builtin_amdgcn_sched_barrier(0);
      {
        bf16x8_t fa = frag_tr(kt, 0, 0, lane), fb = frag_tr(kt, 1, 0, lane);
        __builtin_amdgcn_sched_barrier(0);
        a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, ds0, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb, ds0, a1, 0, 0, 0);
        fa = frag_tr(kt, 0, 1, lane); fb = frag_tr(kt, 1, 1, lane);
        __builtin_amdgcn_sched_barrier(0);
        a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, ds1, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb, ds1, a1, 0, 0, 0);
      }
    }
  };
  for (int t = 0; t < nst; t += 2) {
    stage(t, std::integral_constant<int, 0>{});
    if (t + 1 < nst) stage(t + 1, std::integral_constant<int, 1>{});
  }
  if (qrow < SL) {
    unrope_acc(a0, a1, Rout, rope_pos(Rout, b, qrow), hi);     // q is stored rotated (engine layout): rotate dq back; no-op without tables
    store_t(dqkv + ((size_t)rb + qrow) * pitch + h * 64, a0, a1, 1.f, hi);
  }
}

#ifdef GGET_ATTN_STAMPS
// measurement build only (tools/attn_stamps.sh): s_memtime stamps of block (0,0,0)'s waves in the dK/dV kernel,
// [wave][stage][point]: 0 stage top, 1 past wait + barrier, 2 DMA issued, then per tile j (3 + 5 j): fragments + S/dP MFMAs issued,
// exponentials done, dS done, operands packed, dV/dK MFMAs issued
__device__ unsigned long long g_attn_stamps[8][40][16];
#define GGET_STAMP(pt)                                                                                   \
  do {                                                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
    if (stamp_on && t < 40 && lane == 0) g_attn_stamps[wave][t][pt] = __builtin_amdgcn_s_memtime();       \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
  } while (0)
#else
#define GGET_STAMP(pt) do { } while (0)
#endif
// dK / dV for long sequences: a wave owns a 32-key tile (K and V fragments in registers), Q and dO are streamed in 64-query
// stages together with the queries' lse / delta (and key ranges for packed rows).
// STG = query rows per stage (one barrier per stage): 128 halves the barriers - every barrier re-aligns the two waves of a SIMD
// pair, which the matrix pipe serves one after the other (the early one waits ~700 cycles each time)
template <bool PK, int NWB, int STG = 64>
__global__ void __launch_bounds__(NWB * 64, 2) attn_bwd_dkv64_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                     const float* __restrict__ lse, const float* __restrict__ delta,
                                                                     KeyRange KR, bf16_t* __restrict__ dqkv, int B, int S, int H, int causal,
                                                                     Drop D, Rope Rout) {
  constexpr int ARR = STG * 128;      // bytes of one staged array (rows x 128 B)
  constexpr int NTILE = STG / 32;
  __shared__ __attribute__((aligned(16))) unsigned char st[2][2 * ARR];
  __shared__ __attribute__((aligned(16))) float lse_s[2][STG], dl_s[2][STG];
  __shared__ int qlo_s[2][PK ? STG : 1], qhi_s[2][PK ? STG : 1];
  constexpr int KB = NWB * 32;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.y, b = blockIdx.z;
  // var-len token layout (KR.row_base): sample b owns rows [rb, rb + SL) of the token-major buffers; padded layout: rb = b * S, SL = S
  const int rb = KR.row_base ? KR.row_base[b] : b * S;
  const int SL = KR.row_base ? KR.key_len[b] : S;
  const int k0 = blockIdx.x * KB + wave * 32;
  const int d = H * 64;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const bf16_t* dob = dout + (size_t)rb * d + h * 64;
  const int klen = PK ? S : (KR.key_len ? KR.key_len[b] : S);
  const int krow = k0 + l31;
  bf16x8_t kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = frag_global(kb, krow, SL, pitch, s, lane);
    vf[s] = frag_global(vb, krow, SL, pitch, s, lane);
  }
  f32x16_t dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
  const unsigned dbase = drop_base(D, b * H + h, 0, (unsigned)krow >> 1);
  const int kodd = krow & 1;
  const bool key_ok = krow < klen;
  const int kblk0 = blockIdx.x * KB;
  const int qbeg = causal ? (kblk0 & ~(STG - 1)) : 0;     // queries before the block's first key never see it
  const int qlim = PK ? S : min(S, klen);          // right padding: queries beyond the row's length carry a zero upstream gradient
  const int nst = (kblk0 < klen && qbeg < qlim) ? (qlim - qbeg + STG - 1) / STG : 0;
  constexpr int PPW = (STG / 4) / NWB;      // 1 KiB pieces per wave per stage (two arrays of STG / 8 pieces)
  auto issue = [&](int buf, int r0) {
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int pc = wave * PPW + i;
      if (pc < STG / 8) stage_piece(st[buf], qb, pitch, r0, SL, pc, lane);
      else stage_piece(st[buf] + ARR, dob, (size_t)d, r0, SL, pc - STG / 8, lane);
    }
  };
  // the stage's per-query scalars: fetched by the first 64 threads one stage ahead (registers), written to LDS behind the compute
  float p_lse = 0.f, p_dl = 0.f;
  int p_lo = 0, p_hi = -1;
  auto fetch_vec = [&](int r0) {
    if (tid < STG) {
      const int q = min(r0 + tid, S - 1);
      p_lse = lse[((size_t)b * H + h) * S + q];          // raw: the scaling waits for commit_vec (no wait for the load here)
      // (var-len layout: delta is written for the sample's own rows only - p = 0 times a stale NaN behind them is a NaN in dK)
      p_dl = r0 + tid < SL ? delta[((size_t)b * H + h) * S + q] : 0.f;
      if (PK) {
        const bool v = r0 + tid < SL;
        p_lo = v ? KR.lo[(size_t)b * S + q] : 0;
        p_hi = v ? KR.hi[(size_t)b * S + q] : -1;
      }
    }
  };
  auto commit_vec = [&](int buf) {
    if (tid < STG) {
      lse_s[buf][tid] = -p_lse * kLog2e; dl_s[buf][tid] = -p_dl * kScale;
      if (PK) { qlo_s[buf][tid] = p_lo; qhi_s[buf][tid] = p_hi; }
    }
  };
  if (nst > 0) { issue(0, qbeg); fetch_vec(qbeg); commit_vec(0); }
  const float keep_k = D.inv_keep * kScale;
#ifdef GGET_ATTN_STAMPS
  const bool stamp_on = blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0;
#endif
  for (int t = 0; t < nst; ++t) {
    const int qs = qbeg + t * STG;
    GGET_STAMP(0);
    attn_vm_wait0();
    GGET_STAMP(13);
    __syncthreads();
    GGET_STAMP(1);
    // Waves w and w + 4 share a SIMD and leave the barrier together: in lock-step their MFMA phases collide and then their
    // VALU phases do (stamps: every phase takes twice its own time).  The upper four issue the next stage's DMA now (~600
    // cycles of address-path queueing), the lower four behind their first MFMA group - half a phase apart from then on.
    const bool dma_late = wave < NWB / 2;
    bool dma_due = t + 1 < nst;
    if (dma_due && !dma_late) { issue((t + 1) & 1, qs + STG); fetch_vec(qs + STG); dma_due = false; }
    GGET_STAMP(2);
    const unsigned char* qst = st[t & 1];
    const unsigned char* dst_ = qst + ARR;
    const int vb_ = t & 1;
#pragma unroll
    for (int j = 0; j < NTILE; ++j) {
      const int q0 = qs + 32 * j;
      if (k0 >= klen || q0 >= SL || (causal && q0 + 31 < k0)) continue;
      bool edge = (k0 + 32 > klen) || (q0 + 32 > SL) || (causal && k0 + 31 > q0);
      if (PK) {
        const int lo = qlo_s[vb_][32 * j + l31], hi_ = qhi_s[vb_][32 * j + l31];
        const int ulo = wave_imin(hi_ >= lo ? lo : S), uhi = wave_imax(hi_ >= lo ? hi_ + 1 : 0) - 1;
        if (uhi < k0 || ulo > k0 + 31) continue;
        const int ilo = wave_imax(lo), ihi = wave_imin(hi_ + 1) - 1;
        edge = edge || ilo > k0 || ihi < k0 + 31;
      }
      const unsigned char* qt = qst + 4096 * j;
      const unsigned char* dot_ = dst_ + 4096 * j;
      f32x16_t sc = zero16(), dp = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(qt, s, lane), kf[s], sc, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(dot_, s, lane), vf[s], dp, 0, 0, 0);
      }
      if (dma_due) { issue((t + 1) & 1, qs + STG); fetch_vec(qs + STG); dma_due = false; }
      if (j < 2) GGET_STAMP(3 + 5 * j);
      // the lane's 16 queries are 4 runs of 4 consecutive rows: the per-query scalars come as 4 + 4 ds_read_b128
      float nl[16], dlv[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 a4 = *reinterpret_cast<const float4*>(&lse_s[vb_][32 * j + 8 * g + 4 * hi]);
        const float4 b4 = *reinterpret_cast<const float4*>(&dl_s[vb_][32 * j + 8 * g + 4 * hi]);
        nl[4 * g] = a4.x; nl[4 * g + 1] = a4.y; nl[4 * g + 2] = a4.z; nl[4 * g + 3] = a4.w;
        dlv[4 * g] = b4.x; dlv[4 * g + 1] = b4.y; dlv[4 * g + 2] = b4.z; dlv[4 * g + 3] = b4.w;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = fast_exp2(fmaf(sc[r], kScaleL2, nl[r]));
      if (j < 2) GGET_STAMP(4 + 5 * j);
      if (edge) {
        int q0v = q0;
        asm volatile("" : "+v"(q0v));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qi = 32 * j + acc_row(r, hi);
          const int q = q0v + acc_row(r, hi);
          const bool in_range = PK ? (krow >= qlo_s[vb_][qi] && krow <= qhi_s[vb_][qi]) : key_ok;
          sc[r] = (in_range && q < SL && (!causal || krow <= q)) ? sc[r] : 0.f;
        }
      }
      if (D.thresh == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dp[r] = sc[r] * fmaf(dp[r], kScale, dlv[r]);
      } else {
        // the lane's key is fixed, the queries move along the registers: one hash per score (field = the key's parity)
        const unsigned xb = dbase + (unsigned)(q0 + 4 * hi) * 0x85EBCA77u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const unsigned w = drop_word(xb + (unsigned)((r & 3) + 8 * (r >> 2)) * 0x85EBCA77u);
          const bool drop = (kodd ? (w >> 16) : (w & 0xffffu)) < D.thresh;
          dp[r] = sc[r] * fmaf(dp[r], drop ? 0.f : keep_k, dlv[r]);
          sc[r] = drop ? 0.f : sc[r];      // dropped probabilities: what multiplied V in forward (their 1 / (1 - p) goes onto dV at the end)
        }
      }
      if (j < 2) GGET_STAMP(5 + 5 * j);
      const bf16x8_t p0 = acc_to_b(sc, 0), p1 = acc_to_b(sc, 1);
      const bf16x8_t s0 = acc_to_b(dp, 0), s1 = acc_to_b(dp, 1);
      if (j < 2) GGET_STAMP(6 + 5 * j);
      dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 0, 0, lane), p0, dv0, 0, 0, 0);
      dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 0, 1, lane), p1, dv0, 0, 0, 0);
      dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 1, 0, lane), p0, dv1, 0, 0, 0);
      dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 1, 1, lane), p1, dv1, 0, 0, 0);
      dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 0, 0, lane), s0, dk0, 0, 0, 0);
      dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 0, 1, lane), s1, dk0, 0, 0, 0);
      dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 1, 0, lane), s0, dk1, 0, 0, 0);
      dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 1, 1, lane), s1, dk1, 0, 0, 0);
      if (j < 2) GGET_STAMP(7 + 5 * j);
    }
    if (dma_due) { issue((t + 1) & 1, qs + STG); fetch_vec(qs + STG); }     // (both tiles of the stage skipped)
    if (t + 1 < nst) commit_vec((t + 1) & 1);
  }
  if (krow < SL) {
    bf16_t* row = dqkv + ((size_t)rb + krow) * pitch + h * 64;
    unrope_acc(dk0, dk1, Rout, rope_pos(Rout, b, krow), hi);
    store_t(row + d, dk0, dk1, 1.f, hi);
    store_t(row + 2 * d, dv0, dv1, D.inv_keep, hi);
  }
}

// ================================================================================================
// Fused backward for long sequences (round 4): dK, dV AND dQ from ONE pass over the (key tile, query tile) pairs - S, dP and the
// softmax backward are computed once instead of twice (5 matmuls instead of the 7 of the dQ + dK/dV kernel pair).
// Built on attn_bwd_dkv64_kernel (a wave owns 32 keys, Q / dO streamed in 64-query stages); what is new is the dQ side:
//  * a wave holds dS with its KEY along the lanes and the queries along the registers - the layout dK += dS^T Q wants, the transpose
//    of what dQ += dS K wants.  The bf16 dS tile goes to LDS as [key row][64 queries of the stage] (4 x ds_write_b64 per tile, the
//    swizzle of every [32][128 B] tile here), and is read back through the transposing read as the A operand (m = query, k = key) of
//    v_mfma_f32_16x16x32_bf16; the B operand (k = key, n = head channel) comes the same way from the block's 256 K rows, kept in LDS.
//  * the 64 x 64 dQ tile of a stage is 16 blocks of 16 x 16; each of the 8 waves owns two of them (one 16-channel column block, two
//    16-query row blocks) and reduces them over ALL 256 keys of the block - 16 MFMAs per wave and stage, no cross-wave reduction.
//  * the dS buffer is double-buffered by stage: the dQ MFMAs of stage t run at the top of stage t + 1, behind the barrier the stage
//    loop has anyway.
//  * every key block writes its dQ tiles as bf16 into its OWN slab [rows][d] (plain 8-byte stores, the MFMA run with K as the first
//    operand so that a lane holds 4 consecutive channels); attn_dq_finish_kernel adds the S / 256 slabs of a row in fp32, in block order,
//    rotates the row back (q is stored rotated) and writes the bf16 dq part of dqkv.  Reproducible; costs one extra bf16 rounding of
//    every 256-key partial sum.  First version: fp32 atomics into one accumulator - 8 wave-atomics per wave and stage are 0.8 GB of
//    read-modify-write per layer at the memory side (the L2s are per XCD): B16 / S2048 / H12 backward 959 us; 16 atomics (32 x 32 output
//    quadrants, a third less fragment traffic) 1373 us.
// delta = rowsum(dO * O) comes from attn_delta_kernel (it was a by-product of the dQ kernel).
// ================================================================================================
// 16x16x32 MFMA operand from a swizzled [32 rows][128 B] tile: the operand's M / N index runs along 16 tile columns (bf16 column col0 on),
// its k index along the 32 tile rows: lane (c = l % 16, g = l / 16) gets column col0 + c, rows 8 g .. 8 g + 7
__device__ __forceinline__ bf16x8_t frag_tr16(const unsigned char* tile, int col0, int lane) {
  const int li = lane & 15, g = lane >> 4;
  const int colb = (col0 + (li & 3) * 4) * 2;
  const int ra = 8 * g + (li >> 2);
  const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4_t*)(tile + swz(ra, colb)));
  const bf16x4_t up = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4_t*)(tile + swz(ra + 4, colb)));
  bf16x8_t o;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3];
  o[4] = up[0]; o[5] = up[1]; o[6] = up[2]; o[7] = up[3];
  return o;
}

// delta[b, h, q] = sum_dh dO * O   (the softmax-backward row term; [B,H,S]-indexed like lse).  Block = 32 rows x 8 lanes.
__global__ void __launch_bounds__(256) attn_delta_kernel(const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout, float* __restrict__ delta,
                                                         const int32_t* __restrict__ key_len, const int32_t* __restrict__ row_base, int S, int H) {
  const int b = blockIdx.y, q = blockIdx.x * 32 + (threadIdx.x >> 3), ch = threadIdx.x & 7;
  const int rb = row_base ? row_base[b] : b * S;
  const int SL = row_base ? key_len[b] : S;
  if (q >= SL) {           // (whole groups of 8 lanes leave together) rows of the [B,H,S] grid without a token: a finite value
    if (q < S && ch == 0)
      for (int h = 0; h < H; ++h) delta[((size_t)b * H + h) * S + q] = 0.f;
    return;
  }
  const size_t d = (size_t)H * 64;
  const bf16_t* o = out + ((size_t)rb + q) * d + ch * 8;
  const bf16_t* g = dout + ((size_t)rb + q) * d + ch * 8;
  for (int h = 0; h < H; ++h) {
    float a[8], c[8];
    unpack8(*reinterpret_cast<const uint4*>(o + h * 64), a);
    unpack8(*reinterpret_cast<const uint4*>(g + h * 64), c);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf(a[e], c[e], s);
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
    if (ch == 0) delta[((size_t)b * H + h) * S + q] = s;
  }
}

// dq rows: the key blocks' bf16 partials are summed in fp32 (in block order: reproducible), rotated back, written as bf16 into the q part of
// dqkv.  Key block kb wrote the rows [causal ? 256 kb : 0, min(row length, S)) of its slab when it held a visible key (kb * 256 < length);
// packed rows (ranges): every block writes every row.  8 lanes per (row, head): lane c holds channels [4 c, 4 c + 4) and [32 + 4 c, + 4)
// (the rotation pairs j <-> j + 32).
__global__ void __launch_bounds__(256) attn_dq_finish_kernel(const bf16_t* __restrict__ slabs, size_t slab_stride, bf16_t* __restrict__ dqkv,
                                                             const int32_t* __restrict__ key_len, const int32_t* __restrict__ row_base, int S, int H,
                                                             int causal, int ranges, Rope R) {
  const int b = blockIdx.z, h = blockIdx.y, q = blockIdx.x * 32 + (threadIdx.x >> 3), c = threadIdx.x & 7;
  const int rb = row_base ? row_base[b] : b * S;
  const int SL = row_base ? key_len[b] : S;
  if (q >= SL) return;
  const int len = ranges ? S : (key_len ? min(key_len[b], S) : S);
  int nkb = q < len ? (len + 255) / 256 : 0;
  if (causal) nkb = min(nkb, q / 256 + 1);
  const size_t d = (size_t)H * 64;
  const bf16_t* a = slabs + ((size_t)rb + q) * d + h * 64 + 4 * c;
  float lo[4] = {0.f, 0.f, 0.f, 0.f}, up[4] = {0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < nkb; ++kb) {
    const uint2 l = *reinterpret_cast<const uint2*>(a + (size_t)kb * slab_stride);
    const uint2 u = *reinterpret_cast<const uint2*>(a + (size_t)kb * slab_stride + 32);
    lo[0] += __uint_as_float(l.x << 16); lo[1] += __uint_as_float(l.x & 0xffff0000u);
    lo[2] += __uint_as_float(l.y << 16); lo[3] += __uint_as_float(l.y & 0xffff0000u);
    up[0] += __uint_as_float(u.x << 16); up[1] += __uint_as_float(u.x & 0xffff0000u);
    up[2] += __uint_as_float(u.y << 16); up[3] += __uint_as_float(u.y & 0xffff0000u);
  }
  if (R.cos_tab) {
    const int pos = rope_pos(R, b, q);
    const float4 cs4 = *reinterpret_cast<const float4*>(R.cos_tab + (size_t)pos * 32 + 4 * c);
    const float4 sn4 = *reinterpret_cast<const float4*>(R.sin_tab + (size_t)pos * 32 + 4 * c);
    const float cs[4] = {cs4.x, cs4.y, cs4.z, cs4.w}, sn[4] = {sn4.x, sn4.y, sn4.z, sn4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float l2 = lo[e] * cs[e] + up[e] * sn[e], u2 = up[e] * cs[e] - lo[e] * sn[e];
      lo[e] = l2; up[e] = u2;
    }
  }
  bf16_t* o = dqkv + ((size_t)rb + q) * 3 * d + h * 64 + 4 * c;
  *reinterpret_cast<uint2*>(o) = make_uint2(pack2bf(lo[0], lo[1]), pack2bf(lo[2], lo[3]));
  *reinterpret_cast<uint2*>(o + 32) = make_uint2(pack2bf(up[0], up[1]), pack2bf(up[2], up[3]));
}

constexpr int kFusedLds = 2 * 2 * 8192 + 2 * 8 * 4096 + 8 * 4096 + 4 * 64 * 4 + 4 * 64 * 4;   // stages + dS (x2) + K + lse / delta (+ key ranges)
template <bool PK>
__global__ void __launch_bounds__(512, 2) attn_bwd_fused64_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                  const float* __restrict__ lse, const float* __restrict__ delta,
                                                                  KeyRange KR, bf16_t* __restrict__ dqkv, bf16_t* __restrict__ dq_slabs, size_t slab_stride,
                                                                  int B, int S, int H, int causal, Drop D, Rope Rout) {
  constexpr int NWB = 8, STG = 64, ARR = STG * 128, NTILE = 2, DQB = 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  unsigned char (*st)[2 * ARR] = reinterpret_cast<unsigned char (*)[2 * ARR]>(fsm);                     // [2][16 KiB]: Q | dO of a stage
  unsigned char (*dsb)[NWB * 4096] = reinterpret_cast<unsigned char (*)[NWB * 4096]>(fsm + 2 * 2 * ARR);   // [2][32 KiB]: dS of a stage
  unsigned char* kt_s = fsm + 2 * 2 * ARR + 2 * NWB * 4096;                                                // 32 KiB: the block's K rows
  float (*lse_s)[STG] = reinterpret_cast<float (*)[STG]>(kt_s + NWB * 4096);
  float (*dl_s)[STG] = lse_s + 2;
  int (*qlo_s)[STG] = reinterpret_cast<int (*)[STG]>(dl_s + 2);
  int (*qhi_s)[STG] = qlo_s + 2;
  constexpr int KB = NWB * 32;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.y, b = blockIdx.z;
  const int rb = KR.row_base ? KR.row_base[b] : b * S;
  const int SL = KR.row_base ? KR.key_len[b] : S;
  const int k0 = blockIdx.x * KB + wave * 32;
  const int d = H * 64;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const bf16_t* vb = qb + 2 * d;
  const bf16_t* dob = dout + (size_t)rb * d + h * 64;
  bf16_t* dq_slab = dq_slabs + (size_t)blockIdx.x * slab_stride;      // this key block's dQ partials
  const int klen = PK ? S : (KR.key_len ? KR.key_len[b] : S);
  const int krow = k0 + l31;
  bf16x8_t vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) vf[s] = frag_global(vb, krow, SL, pitch, s, lane);
  // the block's K rows: every wave's dQ operand from stage 1 on (behind the stage barrier), and this wave's own S operand (its own tile,
  // read back four fragments per query tile: 16 registers less than holding them)
  load_tile(kt_s + wave * 4096, kb, k0, SL, pitch, lane);
  const unsigned char* kmine = kt_s + wave * 4096;
  f32x16_t dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
  const unsigned dbase = drop_base(D, b * H + h, 0, (unsigned)krow >> 1);
  const int kodd = krow & 1;
  const bool key_ok = krow < klen;
  const int kblk0 = blockIdx.x * KB;
  const int qbeg = causal ? (kblk0 & ~(STG - 1)) : 0;
  const int qlim = PK ? S : min(S, klen);
  const int nst = (kblk0 < klen && qbeg < qlim) ? (qlim - qbeg + STG - 1) / STG : 0;
  constexpr int PPW = (STG / 4) / NWB;
  auto issue = [&](int buf, int r0) {
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int pc = wave * PPW + i;
      if (pc < STG / 8) stage_piece(st[buf], qb, pitch, r0, SL, pc, lane);
      else stage_piece(st[buf] + ARR, dob, (size_t)d, r0, SL, pc - STG / 8, lane);
    }
  };
  float p_lse = 0.f, p_dl = 0.f;
  int p_lo = 0, p_hi = -1;
  auto fetch_vec = [&](int r0) {
    if (tid < STG) {
      const int q = min(r0 + tid, S - 1);
      p_lse = lse[((size_t)b * H + h) * S + q];
      p_dl = delta[((size_t)b * H + h) * S + q];
      if (PK) {
        const bool v = r0 + tid < SL;
        p_lo = v ? KR.lo[(size_t)b * S + q] : 0;
        p_hi = v ? KR.hi[(size_t)b * S + q] : -1;
      }
    }
  };
  auto commit_vec = [&](int buf) {
    if (tid < STG) {
      lse_s[buf][tid] = -p_lse * kLog2e; dl_s[buf][tid] = -p_dl * kScale;
      if (PK) { qlo_s[buf][tid] = p_lo; qhi_s[buf][tid] = p_hi; }
    }
  };
  // dQ of one finished stage (queries [qs, qs + 64), its dS in dsb[buf]): this wave's two 16 x 16 blocks over the block's 256 keys.
  // Runs between tiles, where few registers are live: the fragments of four key chunks are fetched in one burst (24 transposing reads in
  // flight) before their eight MFMAs.  Measured (B16 / S2048 / H12, p = 0.1, whole backward; the two-kernel form: 1052 us): this 959 us; one
  // chunk at a time 1011 us (every MFMA pair waits out an LDS round trip); the chunks spread over the NEXT stage's softmax-backward
  // arithmetic (fetch behind the S / dP MFMAs, multiply behind the exponentials ...) spills 42 registers in the tile loop: 1791 us.
  // The phase is bound by LDS bandwidth: 24 KiB of fragments per wave and stage, all eight waves at once.
  const int qrows = min(SL, qlim);
  const int dq4 = wave & 3, qq = wave >> 2;
  auto dq_stage = [&](int buf, int qs) {
    f32x4_t c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cb = 0; cb < NWB; cb += DQB) {
      bf16x8_t bk[DQB], a0[DQB], a1[DQB];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < DQB; ++c) {
        bk[c] = frag_tr16(kt_s + (cb + c) * 4096, 16 * dq4, lane);
        a0[c] = frag_tr16(dsb[buf] + (cb + c) * 4096, 32 * qq, lane);
        a1[c] = frag_tr16(dsb[buf] + (cb + c) * 4096, 32 * qq + 16, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < DQB; ++c) {      // (K as the first operand: the tile comes out transposed - a lane holds 4 consecutive channels of one query)
        c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bk[c], a0[c], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bk[c], a1[c], c1, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    const int q_a = qs + 32 * qq + (lane & 15);
    bf16_t* dst = dq_slab + ((size_t)rb + q_a) * d + h * 64 + 16 * dq4 + 4 * (lane >> 4);
    if (q_a < qrows) *reinterpret_cast<uint2*>(dst) = make_uint2(pack2bf(c0[0], c0[1]), pack2bf(c0[2], c0[3]));
    if (q_a + 16 < qrows) *reinterpret_cast<uint2*>(dst + (size_t)16 * d) = make_uint2(pack2bf(c1[0], c1[1]), pack2bf(c1[2], c1[3]));
  };
  if (nst > 0) { issue(0, qbeg); fetch_vec(qbeg); commit_vec(0); }
  const float keep_k = D.inv_keep * kScale;
  // byte selectors of the dropout field (see the dropout loop): low half of the own word / high half of the partner's word ...
  const unsigned selA = kodd ? 0x0c0c0706u : 0x0c0c0100u, selB = kodd ? 0x0c0c0302u : 0x0c0c0504u;
  for (int t = 0; t < nst; ++t) {
    const int qs = qbeg + t * STG;
    attn_vm_wait0();
    __syncthreads();
    const bool dma_late = wave < NWB / 2;
    bool dma_due = t + 1 < nst;
    if (dma_due && !dma_late) { issue((t + 1) & 1, qs + STG); fetch_vec(qs + STG); dma_due = false; }
    // stage t - 1's dQ.  (Measured, same shape: the lower four waves here and the upper four behind the stage's tiles - so that the two waves
    //  of a SIMD are never in this MFMA / LDS-only phase together - 1053 us: the second call site costs 14 spilled registers.)
    if (t > 0) dq_stage((t - 1) & 1, qs - STG);
    const unsigned char* qst = st[t & 1];
    const unsigned char* dst_ = qst + ARR;
    const int vb_ = t & 1;
    unsigned char* dsw = dsb[t & 1] + wave * 4096;
#pragma unroll
    for (int j = 0; j < NTILE; ++j) {
      const int q0 = qs + 32 * j;
      bool skip = k0 >= klen || q0 >= SL || (causal && q0 + 31 < k0);
      bool edge = (k0 + 32 > klen) || (q0 + 32 > SL) || (causal && k0 + 31 > q0);
      if (PK && !skip) {
        const int lo = qlo_s[vb_][32 * j + l31], hi_ = qhi_s[vb_][32 * j + l31];
        const int ulo = wave_imin(hi_ >= lo ? lo : S), uhi = wave_imax(hi_ >= lo ? hi_ + 1 : 0) - 1;
        if (uhi < k0 || ulo > k0 + 31) skip = true;
        const int ilo = wave_imax(lo), ihi = wave_imin(hi_ + 1) - 1;
        edge = edge || ilo > k0 || ihi < k0 + 31;
      }
      if (skip) {   // (wave-uniform) nothing to add to dK / dV; the dQ MFMAs read this tile's dS: zeros
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) *reinterpret_cast<uint2*>(dsw + swz(l31, 64 * j + 16 * gq + 8 * hi)) = make_uint2(0u, 0u);
        continue;
      }
      const unsigned char* qt = qst + 4096 * j;
      const unsigned char* dot_ = dst_ + 4096 * j;
      f32x16_t sc = zero16(), dp = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(qt, s, lane), frag_rows(kmine, s, lane), sc, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(dot_, s, lane), vf[s], dp, 0, 0, 0);
      }
      if (dma_due) { issue((t + 1) & 1, qs + STG); fetch_vec(qs + STG); dma_due = false; }
      float nl[16], dlv[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 a4 = *reinterpret_cast<const float4*>(&lse_s[vb_][32 * j + 8 * g + 4 * hi]);
        const float4 b4 = *reinterpret_cast<const float4*>(&dl_s[vb_][32 * j + 8 * g + 4 * hi]);
        nl[4 * g] = a4.x; nl[4 * g + 1] = a4.y; nl[4 * g + 2] = a4.z; nl[4 * g + 3] = a4.w;
        dlv[4 * g] = b4.x; dlv[4 * g + 1] = b4.y; dlv[4 * g + 2] = b4.z; dlv[4 * g + 3] = b4.w;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = fast_exp2(fmaf(sc[r], kScaleL2, nl[r]));
      if (edge) {
        int q0v = q0;
        asm volatile("" : "+v"(q0v));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qi = 32 * j + acc_row(r, hi);
          const int q = q0v + acc_row(r, hi);
          const bool in_range = PK ? (krow >= qlo_s[vb_][qi] && krow <= qhi_s[vb_][qi]) : key_ok;
          sc[r] = (in_range && q < SL && (!causal || krow <= q)) ? sc[r] : 0.f;
        }
      }
      if (D.thresh == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dp[r] = sc[r] * fmaf(dp[r], kScale, dlv[r]);
      } else {
        // The two lanes of a key pair (k, k + 1) need the same 16 hash words (one word serves both keys).  Each computes HALF of them -
        // the even key's lane those of query registers 0..7, the odd key's lane those of 8..15 (16 queries further) - and reads the
        // other half from its partner (DPP quad_perm [1,0,3,2]); v_perm_b32 with a per-lane selector then picks the lane's 16-bit field
        // out of its own or the partner's word: 8 hashes + 8 lane swaps instead of 16 hashes per 16 scores, same mask.
        const unsigned xb = dbase + (unsigned)(q0 + 4 * hi + 16 * kodd) * 0x85EBCA77u;
        unsigned mine[8], theirs[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) mine[i] = drop_word(xb + (unsigned)((i & 3) + 8 * (i >> 2)) * 0x85EBCA77u);
#pragma unroll
        for (int i = 0; i < 8; ++i) theirs[i] = (unsigned)__builtin_amdgcn_mov_dpp((int)mine[i], 0xB1, 0xF, 0xF, true);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          // v_perm_b32 {S0 = partner's word, S1 = own word}: registers 0..7 are the even lane's own words / the odd lane's partner words
          const unsigned f = __builtin_amdgcn_perm(theirs[r & 7], mine[r & 7], r < 8 ? selA : selB);
          const bool drop = f < D.thresh;
          dp[r] = sc[r] * fmaf(dp[r], drop ? 0.f : keep_k, dlv[r]);
          sc[r] = drop ? 0.f : sc[r];      // (1 / (1 - p) goes onto dV at the end)
        }
      }
      const bf16x8_t p0 = acc_to_b(sc, 0), p1 = acc_to_b(sc, 1);
      const bf16x8_t s0 = acc_to_b(dp, 0), s1 = acc_to_b(dp, 1);
      {   // dS to LDS for the dQ MFMAs of the next stage: this lane's key row, queries 8 gq + 4 hi .. + 3 of the tile per 8-byte piece
        const uint4 u0 = __builtin_bit_cast(uint4, s0), u1 = __builtin_bit_cast(uint4, s1);
        *reinterpret_cast<uint2*>(dsw + swz(l31, 64 * j + 0 + 8 * hi)) = make_uint2(u0.x, u0.y);
        *reinterpret_cast<uint2*>(dsw + swz(l31, 64 * j + 16 + 8 * hi)) = make_uint2(u0.z, u0.w);
        *reinterpret_cast<uint2*>(dsw + swz(l31, 64 * j + 32 + 8 * hi)) = make_uint2(u1.x, u1.y);
        *reinterpret_cast<uint2*>(dsw + swz(l31, 64 * j + 48 + 8 * hi)) = make_uint2(u1.z, u1.w);
      }
      dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 0, 0, lane), p0, dv0, 0, 0, 0);
      dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 0, 1, lane), p1, dv0, 0, 0, 0);
      dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 1, 0, lane), p0, dv1, 0, 0, 0);
      dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(dot_, 1, 1, lane), p1, dv1, 0, 0, 0);
      dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 0, 0, lane), s0, dk0, 0, 0, 0);
      dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 0, 1, lane), s1, dk0, 0, 0, 0);
      dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 1, 0, lane), s0, dk1, 0, 0, 0);
      dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(qt, 1, 1, lane), s1, dk1, 0, 0, 0);
    }
    if (dma_due) { issue((t + 1) & 1, qs + STG); fetch_vec(qs + STG); }
    if (t + 1 < nst) commit_vec((t + 1) & 1);
  }
  if (nst > 0) {     // the last stage's dQ
    __syncthreads();
    dq_stage((nst - 1) & 1, qbeg + (nst - 1) * STG);
  }
  if (krow < SL) {
    bf16_t* row = dqkv + ((size_t)rb + krow) * pitch + h * 64;
    unrope_acc(dk0, dk1, Rout, rope_pos(Rout, b, krow), hi);
    store_t(row + d, dk0, dk1, 1.f, hi);
    store_t(row + 2 * d, dv0, dv1, D.inv_keep, hi);
  }
}

// ------------------------------------------------------------------------------------------------
// Attention weights of one layer (`output_attentions=True`; reference: the attn_weights hf eager_attention_forward returns,
// modeling_llama.py:191-214, after its dropout in training mode):
//   out[b, h, q, k] = bf16(m * exp(<q_bhq, k_bhk> / 8 - lse[b, h, q]))  for an allowed key, 0 otherwise;  out bf16 [B, H, S, S].
// The forward kernels never hold a row of probabilities, so the scores are recomputed here (S^T = K Q^T on 32x32x16 bf16 MFMA, fp32
// accumulators, q and k as they sit in qkv: rotated already) and normalised with the log-sum-exp the forward saved.
// lse convention - the same in EVERY producer (attn_fwd_kernel, attn_fwd_rows64_kernel, attn_oproj_fwd_kernel, attn_fwd64_kernel with and
// without key ranges, attn_fwd_dense_kernel): lse[(b * H + h) * S + q] = NATURAL log of sum_k exp(score / 8) over the allowed keys, taken
// before dropout ((m + log2 l) / log2 e of the log2-domain online softmax); 0 for a query without keys; not written for rows behind a
// sample on the var-len layout (never read here: such rows are zero by the rule).
// Allowed keys: right padding (either token layout) q < len_b, k < len_b, k <= q when causal - rows of padding queries are ZERO, where the
// padded-layout forward computes a softmax nothing consumes; packed rows lo[b,q] <= k <= hi[b,q] (and k <= q when causal).
// m: the forward's keep multiplier (drop_mul_x with the forward's hash coordinates (seed, b * H + h, q, k)), 1 when D.thresh == 0.
// The launch is bound by its stores (2 B written per 128 FLOP): a block = NW query tiles of one (b, h) walks the keys 64 at a time, the K
// rows staged once per block; a wave transposes its 32 x 64 probabilities through a private LDS tile so that a lane stores 16 bytes along
// the key axis and eight lanes cover the 128 contiguous bytes of a row - four 16-byte store instructions per lane and step.  Every element
// of out is written (zeros included); no atomics: reruns are bit-identical.  vec == 0 (S % 8 != 0 or an unaligned out): element stores.
template <int NW, bool PK>
__global__ void __launch_bounds__(NW * 64) attn_probs_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ lse, KeyRange KR,
                                                             bf16_t* __restrict__ out, int B, int S, int H, int causal, Drop D, int vec) {
  constexpr int kPitch = 144;   // bytes per staged row: 64 keys + one 16-byte piece, so the lanes' 16-byte reads of 8 rows spread over the banks
  __shared__ __attribute__((aligned(16))) unsigned char kt[2][4096];
  __shared__ __attribute__((aligned(16))) unsigned char pt[NW][32 * kPitch];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.y, b = blockIdx.z;
  const int len = KR.key_len ? max(min(KR.key_len[b], S), 0) : S;
  const int rb = KR.row_base ? KR.row_base[b] : b * S;
  const int SL = KR.row_base ? len : S;      // rows the sample owns in the token-major buffer: no load leaves them (clamp_row)
  const int q0 = (blockIdx.x * NW + wave) * 32;
  const int d = H * 64;
  const size_t pitch = (size_t)3 * d;
  const bf16_t* qb = qkv + (size_t)rb * pitch + h * 64;
  const bf16_t* kb = qb + d;
  const int qrow = q0 + l31;
  const Rope Rnone{nullptr, nullptr, nullptr, S};
  // per-lane inclusive key range [qlo, qhi] (empty: qhi < qlo); uhi = the wave's largest allowed key
  int qlo = 0, qhi = (qrow < len) ? len - 1 : -1;
  if constexpr (PK) {
    const bool v = qrow < S;
    qlo = v ? max(KR.lo[(size_t)b * S + qrow], 0) : 0;
    qhi = v ? min(KR.hi[(size_t)b * S + qrow], S - 1) : -1;
  }
  const bool row_live = qhi >= qlo;
  const int uhi = wave_imax(row_live ? qhi + 1 : 0) - 1;
  // keys every lane of the wave allows, [ilo, ihi]: a tile inside (and below the diagonal) needs no mask; empty when a lane has no keys
  const int ilo = wave_imax(row_live ? qlo : S), ihi = wave_imin(row_live ? qhi + 1 : 0) - 1;
  const int klen = PK ? S : len;
  const int kend_blk = SL > 0 ? (causal ? min(klen, (int)(blockIdx.x + 1) * NW * 32) : klen) : 0;   // keys the block stages
  const int kend = SL > 0 ? min(uhi + 1, causal ? q0 + 32 : S) : 0;                                  // keys this wave computes (<= kend_blk)
  bf16x8_t qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = __builtin_bit_cast(bf16x8_t, make_uint4(0u, 0u, 0u, 0u));
  if (kend > 0) frags_global_rope(qf, qb, qrow, SL, pitch, lane, Rnone, b);
  const float nlse2 = row_live ? -lse[((size_t)b * H + h) * S + qrow] * kLog2e : 0.f;
  const unsigned dbase = drop_base(D, b * H + h, qrow, 0);
  bf16_t* obase = out + (size_t)(b * H + h) * S * S;
  unsigned char* mypt = pt[wave];
  constexpr bool PF = NW > 1;    // one-wave blocks (S < 64) take one step: nothing to prefetch, and the registers are better spent on occupancy
  TilePref<NW * 64> pk[2];
  if constexpr (PF) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (32 * j < kend_blk) tile_fetch<NW * 64>(pk[j], kb, 32 * j, SL, pitch, tid, Rnone);
  }
  for (int k0 = 0; k0 < S; k0 += 64) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (k0 + 32 * j < kend_blk) {
        if constexpr (PF) tile_commit<NW * 64>(kt[j], pk[j], k0 + 32 * j, SL, tid, Rnone, b);
        else load_tile_coop<NW * 64>(kt[j], kb, k0 + 32 * j, SL, pitch, tid, Rnone, b);
      }
    __syncthreads();
    if constexpr (PF) {            // the next step's K rows fly while this one is computed and stored
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (k0 + 64 + 32 * j < kend_blk) tile_fetch<NW * 64>(pk[j], kb, k0 + 64 + 32 * j, SL, pitch, tid, Rnone);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kk = k0 + 32 * j;
      f32x16_t sc = zero16();
      if (kk < kend) {
#pragma unroll
        for (int s = 0; s < 4; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(kt[j], s, lane), qf[s], sc, 0, 0, 0);
        // the mask is evaluated only on tiles that touch a key-range end or the diagonal (the loop is VALU work beside the stores)
        const bool edge = kk < ilo || kk + 31 > ihi || (causal && kk + 31 > q0);
        if (edge) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kk + acc_row(r, hi);
            const bool ok = key >= qlo && key <= qhi && (!causal || key <= qrow);
            const float p = fast_exp2(fmaf(sc[r], kScaleL2, nlse2)) * drop_mul_x(D, dbase + (unsigned)(key >> 1) * 0xC2B2AE3Du, key & 1);
            sc[r] = ok ? p : 0.f;
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            sc[r] = fast_exp2(fmaf(sc[r], kScaleL2, nlse2)) * drop_mul_x(D, dbase + (unsigned)((kk + acc_row(r, hi)) >> 1) * 0xC2B2AE3Du, r & 1);
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {      // registers [4g, 4g + 4) = keys kk + 8g + 4hi .. + 3 of the lane's query: 8 bytes of its row
        uint2 v;
        v.x = pack2bf(sc[4 * g + 0], sc[4 * g + 1]);
        v.y = pack2bf(sc[4 * g + 2], sc[4 * g + 3]);
        *reinterpret_cast<uint2*>(mypt + l31 * kPitch + (32 * j + 8 * g + 4 * hi) * 2) = v;
      }
    }
    __syncthreads();     // the block is done with kt (next step's loads may land) and every wave's tile is complete in LDS
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 8 * i + (lane >> 3), c = lane & 7;
      const int q = q0 + r, k = k0 + 8 * c;
      if (q < S && k < S) {
        const uint4 v = *reinterpret_cast<const uint4*>(mypt + r * kPitch + c * 16);
        bf16_t* dst = obase + (size_t)q * S + k;
        if (vec) {
          typedef __attribute__((ext_vector_type(4))) unsigned nt_u32x4_t;
          const nt_u32x4_t nv = {v.x, v.y, v.z, v.w};
          __builtin_nontemporal_store(nv, reinterpret_cast<nt_u32x4_t*>(dst));      // S % 8 == 0: the piece ends inside the row; written once, not re-read here
        } else {
          const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (k + e < S) dst[e] = (bf16_t)(e & 1 ? w[e >> 1] >> 16 : w[e >> 1] & 0xffffu);
        }
      }
    }
  }
}

// rotated q|k|v of one layer as [B, S, w] (w = 3 d): rows of a sample from either token layout, zeros behind its tokens (packed rows: at
// tokens without keys); one thread per 16-byte piece
__global__ void __launch_bounds__(256) qkv_grid_kernel(const bf16_t* __restrict__ src, KeyRange KR, bf16_t* __restrict__ out, int B, int S, int w) {
  const int cpr = w / 8;
  const long n = (long)B * S * cpr;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long pos = i / cpr;
    const int c = (int)(i % cpr);
    const int b = (int)(pos / S), s = (int)(pos % S);
    bool live;
    long row = pos;
    if (KR.lo) live = KR.lo[pos] <= KR.hi[pos];
    else {
      live = s < (KR.key_len ? KR.key_len[b] : S);
      if (KR.row_base) row = (long)KR.row_base[b] + s;
    }
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (live) v = *reinterpret_cast<const uint4*>(src + (size_t)row * w + c * 8);
    *reinterpret_cast<uint4*>(out + (size_t)pos * w + c * 8) = v;
  }
}

// waves (= 32-row tiles) per block: long sequences share each K/V (or Q/dO) tile among 4 waves through LDS
int attn_waves(int S) { return S >= 128 ? 4 : (S >= 64 ? 2 : 1); }
// GGET_ATTN_BY_SAMPLE=0: the S-keyed launches of rounds 1 - 5 for 32 < S <= 64 (A/B switch of the per-sample dispatch)
bool attn_by_sample_rows() { return menu().attn_by_sample != 0; }
constexpr int kLongGrid = 32;      // sample slots of a list-driven long launch (a block walks the list with this stride)

}  // namespace

int k_attn_fwd(const void* qkv, const int32_t* key_len, void* out, float* lse, int B, int S, int H, int causal,
               const float* cos_tab, const float* sin_tab, const int64_t* position_ids, float dropout_p,
               unsigned dropout_seed, hipStream_t st, const int32_t* key_lo, const int32_t* key_hi, const int32_t* row_base,
               const int32_t* long_list, int head_dim) {
  if (head_dim == 32) {     // the compact family of attention32.hip: q, k rotated in memory
    GGET_REQUIRE(!cos_tab && !sin_tab, "attention: head_dim 32 takes q and k already rotated (no rotation on load)");
    return k_attn32_fwd(qkv, key_len, out, lse, B, S, H, causal, dropout_p, dropout_seed, st, key_lo, key_hi, row_base);
  }
  GGET_REQUIRE(head_dim == 64, "attention: unsupported head_dim %d", head_dim);
  GGET_REQUIRE(!row_base || (key_len && !key_lo), "attention: the var-len token layout needs key_len and excludes per-token key ranges");
  const KeyRange KR{key_len, key_lo, key_hi, row_base};
  if (B == 0 || S == 0) return 0;
  const Rope R{cos_tab, sin_tab, position_ids, S};
  const Drop D = make_drop(dropout_p, dropout_seed);
  // var-len layout, 32 < S <= 64 (the collator pads to the batch's longest graph, most samples are still one 32-row tile): every sample by
  // its OWN row count (attn_fwd_rows64_kernel)
  if (row_base && S > 32 && S <= 64 && !cos_tab && attn_by_sample_rows()) {
    hipLaunchKernelGGL(attn_fwd_rows64_kernel, dim3(H, B, (S + 31) / 32), dim3(64), 0, st, (const bf16_t*)qkv, key_len, row_base, (bf16_t*)out, lse, B, S, H,
                       causal, D);
    GGET_LAUNCH_CHECK();
    return 0;
  }
  if (S >= 256 && !cos_tab && menu().attn_big) {   // long sequences with q / k already rotated (the engine's layout): 64-row DMA stages
#define GGET_FWD64(PK) hipLaunchKernelGGL((attn_fwd64_kernel<PK, 1, 8>), dim3((S + 255) / 256, H, B), dim3(512), 0, st, (const bf16_t*)qkv, KR, \
                                          (bf16_t*)out, lse, B, S, H, causal, D)
    if (menu().attn_dense && !key_lo && !causal && S >= 512) {   // (shorter rows: the pipeline's fill and drain cost more than it hides)
      if (D.thresh) hipLaunchKernelGGL((attn_fwd_dense_kernel<true, 8>), dim3((S + 255) / 256, H, B), dim3(512), 0, st, (const bf16_t*)qkv, key_len,
                                       (bf16_t*)out, lse, B, S, H, D, row_base);
      else hipLaunchKernelGGL((attn_fwd_dense_kernel<false, 8>), dim3((S + 255) / 256, H, B), dim3(512), 0, st, (const bf16_t*)qkv, key_len,
                              (bf16_t*)out, lse, B, S, H, D, row_base);
    } else if (key_lo) GGET_FWD64(true);
    else GGET_FWD64(false);   // (one query tile per wave at 4 waves / SIMD beat two tiles per wave at 2)
#undef GGET_FWD64
    GGET_LAUNCH_CHECK();
    return 0;
  }
  const int nw = attn_waves(S);
  dim3 grid((S + 32 * nw - 1) / (32 * nw), H, B);
#define GGET_ATTN_FWD(NW, PK) hipLaunchKernelGGL((attn_fwd_kernel<NW, PK>), grid, dim3(NW * 64), 0, st, (const bf16_t*)qkv, KR, \
                                             (bf16_t*)out, lse, B, S, H, causal, R, D)
  if (key_lo) { if (nw == 4) GGET_ATTN_FWD(4, true); else if (nw == 2) GGET_ATTN_FWD(2, true); else GGET_ATTN_FWD(1, true); }
  else { if (nw == 4) GGET_ATTN_FWD(4, false); else if (nw == 2) GGET_ATTN_FWD(2, false); else GGET_ATTN_FWD(1, false); }
#undef GGET_ATTN_FWD
  GGET_LAUNCH_CHECK();
  return 0;
}

// attention weights of one layer from its rotated q | k and the forward's log-sum-exp (attn_probs_kernel); writes all of out [B,H,S,S]
int k_attn_probs(const void* qkv, const float* lse, const int32_t* key_len, const int32_t* row_base, const int32_t* key_lo,
                 const int32_t* key_hi, void* out, int B, int S, int H, int causal, float dropout_p, unsigned dropout_seed, hipStream_t st,
                 int head_dim) {
  if (head_dim == 32) return k_attn32_probs(qkv, lse, key_len, row_base, key_lo, key_hi, out, B, S, H, causal, dropout_p, dropout_seed, st);
  GGET_REQUIRE(head_dim == 64, "attn_probs: unsupported head_dim %d", head_dim);
  GGET_REQUIRE(qkv && lse && out, "attn_probs: null argument");
  GGET_REQUIRE(B > 0 && S > 0 && H > 0 && B <= 65535 && H <= 65535, "attn_probs: bad shape B %d S %d H %d", B, S, H);
  GGET_REQUIRE(!key_lo == !key_hi, "attn_probs: half a key range");
  GGET_REQUIRE(!row_base || (key_len && !key_lo), "attn_probs: the var-len token layout needs key_len and excludes per-token key ranges");
  GGET_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "attn_probs: dropout_p %g outside [0, 1)", (double)dropout_p);
  const KeyRange KR{key_lo ? nullptr : key_len, key_lo, key_hi, row_base};
  const Drop D = make_drop(dropout_p, dropout_seed);
  const int vec = (S % 8 == 0) && (((uintptr_t)out & 15) == 0);
  const int nw = attn_waves(S);
  dim3 grid((S + 32 * nw - 1) / (32 * nw), H, B);
#define GGET_ATTN_PROBS(NW, PK) hipLaunchKernelGGL((attn_probs_kernel<NW, PK>), grid, dim3(NW * 64), 0, st, (const bf16_t*)qkv, lse, KR, \
                                                   (bf16_t*)out, B, S, H, causal, D, vec)
  if (key_lo) { if (nw == 4) GGET_ATTN_PROBS(4, true); else if (nw == 2) GGET_ATTN_PROBS(2, true); else GGET_ATTN_PROBS(1, true); }
  else { if (nw == 4) GGET_ATTN_PROBS(4, false); else if (nw == 2) GGET_ATTN_PROBS(2, false); else GGET_ATTN_PROBS(1, false); }
#undef GGET_ATTN_PROBS
  GGET_LAUNCH_CHECK();
  return 0;
}
// rotated q | k | v rows of a layer -> [B, S, w] (qkv_grid_kernel); w a multiple of 8
int k_qkv_grid(const void* src, const int32_t* key_len, const int32_t* row_base, const int32_t* key_lo, const int32_t* key_hi, void* out,
               int B, int S, int w, hipStream_t st) {
  GGET_REQUIRE(src && out && B > 0 && S > 0 && w > 0 && w % 8 == 0, "qkv_grid: bad arguments");
  const KeyRange KR{key_lo ? nullptr : key_len, key_lo, key_hi, row_base};
  const long n = (long)B * S * (w / 8);
  hipLaunchKernelGGL(qkv_grid_kernel, dim3((unsigned)std::min<long>(4096, (n + 255) / 256)), dim3(256), 0, st, (const bf16_t*)src, KR, (bf16_t*)out, B, S, w);
  GGET_LAUNCH_CHECK();
  return 0;
}

// attention + o projection + residual + RMSNorm of one decoder layer for S <= 32 (attn_oproj_fwd_kernel); returns 1 via *taken when
// the fused form ran, 0 when the shape is not covered (the caller then runs the three launches)
int k_pack_wo(const void* w0, size_t layer_stride, void* fwd, void* bwd, int d, int layers, hipStream_t st) {
  GGET_REQUIRE(d % 64 == 0 && layers > 0, "pack_wo: d must be a multiple of 64");
  hipLaunchKernelGGL(pack_wo_kernel, dim3(d / 64, d / 64, layers), dim3(256), 0, st, (const bf16_t*)w0, layer_stride, (bf16_t*)fwd, (bf16_t*)bwd, d);
  GGET_LAUNCH_CHECK();
  return 0;
}
bool attn_oproj_enabled() { return menu().attn_oproj && !menu().attn_oproj_off; }   // (attn_oproj_off: in-process A/B of the fused form)
template <int H>
static int launch_attn_oproj(const void* qkv, const int32_t* key_len, const int32_t* row_base, void* attn_out, float* lse, const void* wo,
                             const void* x_in, void* x_mid, const void* nw, void* xn, float* rstd, int B, int S, int causal, float eps,
                             const Drop& D, hipStream_t st) {
  constexpr int lds = attn_oproj_fwd_lds<H>();
  static_assert(lds <= 160 * 1024, "per-sample forward: LDS");
  static bool attr = false;
  if (!attr) {
    GGET_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_oproj_fwd_kernel<H>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    attr = true;
  }
  hipLaunchKernelGGL((attn_oproj_fwd_kernel<H>), dim3(B), dim3(H * 64), lds, st, (const bf16_t*)qkv, key_len, row_base, (bf16_t*)attn_out, lse,
                     (const bf16_t*)wo, (const bf16_t*)x_in, (bf16_t*)x_mid, (const bf16_t*)nw, (bf16_t*)xn, rstd, B, S, causal, eps, D);
  GGET_LAUNCH_CHECK();
  return 0;
}
int k_attn_oproj_fwd(const void* qkv, const int32_t* key_len, const int32_t* row_base, void* attn_out, float* lse, const void* wo,
                     const void* x_in, void* x_mid, const void* nw, void* xn, float* rstd, int B, int S, int H, int causal, float eps,
                     float dropout_p, unsigned dropout_seed, hipStream_t st, int* taken, int head_dim) {
  *taken = 0;
  if (head_dim != 64) return 0;     // (the per-sample kernels hold 64-wide heads)
  // (S <= 32 only: a 33 .. 64-row sample inside this kernel - one workgroup over two row tiles - was built and measured slower than the
  //  three launches, profiles/r06_attn_oproj_fwd_long_experiment.diff; the backward counterpart is kept)
  if (B == 0 || S == 0 || S > 32 || !attn_oproj_enabled()) return 0;
  GGET_REQUIRE(!row_base || key_len, "attention: the var-len token layout needs key_len");
  const Drop D = make_drop(dropout_p, dropout_seed);
#define GGET_AO(HH) case HH: *taken = 1; return launch_attn_oproj<HH>(qkv, key_len, row_base, attn_out, lse, wo, x_in, x_mid, nw, xn, rstd, B, S, causal, eps, D, st)
  switch (H) {
    GGET_AO(2); GGET_AO(4); GGET_AO(8); GGET_AO(12);     // (H = 16: the tiles of 16 waves do not fit 160 KiB of LDS)
    default: return 0;
  }
#undef GGET_AO
}

template <int H>
static int launch_attn_oproj_bwd(const void* dxn, const void* x_mid, const void* nw, const float* rstd, const void* dres, void* dx_mid,
                                 float* dw_accum, int copies, uint64_t copy_stride, const void* wot, const void* qkv, const float* lse,
                                 const int32_t* key_len, const int32_t* row_base, void* dqkv, int B, int S, int causal, const Rope& R,
                                 const Drop& D, int t_rows, hipStream_t st, void* dattn_long) {
  constexpr int d = H * 64, PITCH = (d + kOPad) * 2;
  constexpr int XB = 32 * PITCH > H * 4096 ? 32 * PITCH : H * 4096, YB = H * 8192 > H * d * 4 ? H * 8192 : H * d * 4;
  constexpr int lds = XB + YB + H * 64 * 4 + 2 * 32 * kRopePitch * 4;      // + the sample's cos / sin rows (attn_oproj_bwd_kernel)
  static_assert(lds <= 160 * 1024, "per-sample backward: LDS");
  static bool attr = false;
  if (!attr) {
    GGET_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_oproj_bwd_kernel<H>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    attr = true;
  }
  hipLaunchKernelGGL((attn_oproj_bwd_kernel<H>), dim3(B), dim3(H * 64), lds, st, (const bf16_t*)dxn, (const bf16_t*)x_mid, (const bf16_t*)nw, rstd,
                     (const bf16_t*)dres, (bf16_t*)dx_mid, dw_accum, copies, copy_stride, (const bf16_t*)wot, (const bf16_t*)qkv, lse, key_len,
                     row_base, (bf16_t*)dqkv, B, S, causal, R, D, t_rows, (bf16_t*)dattn_long);
  GGET_LAUNCH_CHECK();
  return 0;
}
int k_attn_oproj_bwd(const void* dxn, const void* x_mid, const void* nw, const float* rstd, const void* dres, void* dx_mid, float* dw_accum,
                     int copies, uint64_t copy_stride, const void* wot_packed, const void* qkv, const float* lse, const int32_t* key_len,
                     const int32_t* row_base, void* dqkv, int B, int S, int H, int causal, const float* cos_tab, const float* sin_tab,
                     const int64_t* position_ids, float dropout_p, unsigned dropout_seed, int t_rows, hipStream_t st, int* taken,
                     void* dattn_long, const int32_t* long_list, int head_dim) {
  *taken = 0;
  if (head_dim != 64) return 0;     // (the per-sample kernels hold 64-wide heads)
  // S <= 32, or - var-len layout, with room for the long samples' dattn rows - S <= 64: every sample by its own row count
  if (B == 0 || S == 0 || S > 64 || (S > 32 && (!row_base || !dattn_long || !attn_by_sample_rows())) || !attn_oproj_enabled())
    return 0;
  if (H != 2 && H != 4 && H != 8 && H != 12) return 0;
  GGET_REQUIRE(!row_base || key_len, "attention: the var-len token layout needs key_len");
  if (copies < 1) copies = 1;
  // Reproducible mode: the kernel's norm-weight gradient goes to one zeroed row per sample instead of the shared replicas (copies = B:
  // block b owns row b, and its at most two adds onto zero are exact in either order); the rows are then summed in block order
  float* part = nullptr;
  float* dw_out = dw_accum;
  if (menu().deterministic) {
    const int d = H * 64;
    if (int e = k_det_scratch((size_t)(B + (B + 63) / 64) * d, &part)) return e;
    GGET_HIP_CHECK(hipMemsetAsync(part, 0, (size_t)B * d * sizeof(float), st));
    dw_accum = part;
    copies = B;
    copy_stride = (uint64_t)d;
  }
  const Rope R{cos_tab, sin_tab, position_ids, S};     // rotation of dq, dk back to the un-rotated projections (q, k in memory are rotated)
  const Drop D = make_drop(dropout_p, dropout_seed);
  int rc = 0;
#define GGET_AOB(HH) case HH: rc = launch_attn_oproj_bwd<HH>(dxn, x_mid, nw, rstd, dres, dx_mid, dw_accum, copies, copy_stride, wot_packed, qkv, lse, key_len, row_base, dqkv, B, S, causal, R, D, t_rows, st, dattn_long); break
  switch (H) {
    GGET_AOB(2); GGET_AOB(4); GGET_AOB(8); GGET_AOB(12);
  }
#undef GGET_AOB
  if (rc) return rc;
  *taken = 1;
  if (part)
    if (int e = k_ordered_colsum(part, B, H * 64, dw_out, st)) return e;
  if (S > 32) {     // the attention backward of the 33 .. 64-row samples, from the dattn rows the kernel above wrote for them
    hipLaunchKernelGGL(attn_bwd_long_kernel, dim3(1, H, long_list ? std::min(B, kLongGrid) : B), dim3(128), 0, st, (const bf16_t*)qkv, (const bf16_t*)dattn_long,
                       lse, key_len, (bf16_t*)dqkv, B, S, H, causal, R, D, row_base, long_list);
    GGET_LAUNCH_CHECK();
  }
  return 0;
}
int k_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len, void* dqkv,
               float* delta_ws, int B, int S, int H, int causal, const float* cos_tab, const float* sin_tab,
               const int64_t* position_ids, int qk_rotated, float dropout_p, unsigned dropout_seed, hipStream_t st,
               const int32_t* key_lo, const int32_t* key_hi, const int32_t* row_base, void* dq_ws, size_t dq_slab_stride,
               const int32_t* long_list, int head_dim) {
  if (head_dim == 32) {     // the compact family of attention32.hip: q, k rotated in memory, the tables only rotate dq / dk back
    GGET_REQUIRE(!cos_tab || qk_rotated, "attention: head_dim 32 takes q and k already rotated (no rotation on load)");
    return k_attn32_bwd(qkv, out, dout, lse, key_len, dqkv, delta_ws, B, S, H, causal, cos_tab, sin_tab, position_ids, dropout_p, dropout_seed,
                        st, key_lo, key_hi, row_base);
  }
  GGET_REQUIRE(head_dim == 64, "attention: unsupported head_dim %d", head_dim);
  GGET_REQUIRE(!row_base || (key_len && !key_lo), "attention: the var-len token layout needs key_len and excludes per-token key ranges");
  const KeyRange KR{key_len, key_lo, key_hi, row_base};
  if (B == 0 || S == 0) return 0;
  const Rope R{cos_tab, sin_tab, position_ids, S};     // rotation of dq, dk back to the un-rotated projections
  const Rope Rin = qk_rotated ? Rope{nullptr, nullptr, nullptr, S} : R;   // q,k in memory are already rotated?
  const Drop D = make_drop(dropout_p, dropout_seed);
  const LaunchMenu& m = menu();
  if ((S <= 32 || (S <= 64 && !Rin.cos_tab && attn_by_sample_rows())) && !key_lo && m.attn_small) {      // every sample by its OWN row count: one 32-row tile, or (33 .. 64 rows) 2 x 2
    if (S <= 32 || row_base)        // (padded layout with S > 32: every sample owns S rows - nothing for the one-tile kernel)
      hipLaunchKernelGGL(attn_bwd_small_kernel, dim3(1, H, B), dim3(64), 0, st, (const bf16_t*)qkv,
                         (const bf16_t*)dout, lse, key_len, (bf16_t*)dqkv, B, S, H, causal, Rin, R, D, row_base);
    if (S > 32) {
      // (on a second stream beside the dense launch the sparse one made the step SLOWER - 7.39 -> 7.80 ms at S = 40: the fork / join
      //  barrier packets cost more than the 15 us they hide; profiles/r06_attn_side_lane_experiment.diff)
      const int32_t* list = row_base ? long_list : nullptr;
      hipLaunchKernelGGL(attn_bwd_long_kernel, dim3(1, H, list ? std::min(B, kLongGrid) : B), dim3(128), 0, st, (const bf16_t*)qkv, (const bf16_t*)dout, lse,
                         key_len, (bf16_t*)dqkv, B, S, H, causal, R, D, row_base, list);
    }
    GGET_LAUNCH_CHECK();
    return 0;
  }
  // (q, k rotated in memory - the engine's layout - or no rotation at all: the staged kernels read them as they are and rotate dq / dk
  // back in their epilogues; q, k to be rotated on load, the plain-op form of the tests, stays on the register-prefetch kernels)
  if (S >= 256 && (!cos_tab || qk_rotated) && m.attn_big) {
    // fused form (one pass; the caller provides room for the key blocks' dQ partials: bf16 [ceil(S / 256)][dq_slab_stride], dq_slab_stride >=
    // rows x H x 64): see attn_bwd_fused64_kernel.  (S = 256, one key block per row: still ahead of the two-kernel form once the partials are
    // plain stores - C3 step 40.06 -> 39.69 ms, same box; GGET_ATTN_FUSED_MIN_S moves the threshold.)
    if (dq_ws && m.attn_fused && S >= m.attn_fused_min_s) {
      static bool attr = false;
      if (!attr) {
        GGET_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_fused64_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, kFusedLds));
        GGET_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_fused64_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, kFusedLds));
        attr = true;
      }
      hipLaunchKernelGGL(attn_delta_kernel, dim3((S + 31) / 32, B), dim3(256), 0, st, (const bf16_t*)out, (const bf16_t*)dout, delta_ws, key_len, row_base, S, H);
      if (key_lo) hipLaunchKernelGGL((attn_bwd_fused64_kernel<true>), dim3((S + 255) / 256, H, B), dim3(512), kFusedLds, st, (const bf16_t*)qkv, (const bf16_t*)dout,
                                     lse, delta_ws, KR, (bf16_t*)dqkv, (bf16_t*)dq_ws, dq_slab_stride, B, S, H, causal, D, R);
      else hipLaunchKernelGGL((attn_bwd_fused64_kernel<false>), dim3((S + 255) / 256, H, B), dim3(512), kFusedLds, st, (const bf16_t*)qkv, (const bf16_t*)dout,
                              lse, delta_ws, KR, (bf16_t*)dqkv, (bf16_t*)dq_ws, dq_slab_stride, B, S, H, causal, D, R);
      hipLaunchKernelGGL(attn_dq_finish_kernel, dim3((S + 31) / 32, H, B), dim3(256), 0, st, (const bf16_t*)dq_ws, dq_slab_stride, (bf16_t*)dqkv, key_len, row_base,
                         S, H, causal, key_lo ? 1 : 0, R);
      GGET_LAUNCH_CHECK();
      return 0;
    }
    const int stg128 = m.attn_stg128;
#define GGET_BWD64(PK)                                                                                                           \
  do {                                                                                                                           \
    hipLaunchKernelGGL((attn_bwd_dq64_kernel<PK, 4>), dim3((S + 127) / 128, H, B), dim3(256), 0, st, (const bf16_t*)qkv,             \
                       (const bf16_t*)out, (const bf16_t*)dout, lse, delta_ws, KR, (bf16_t*)dqkv, B, S, H, causal, D, R);          \
    if (stg128 && S >= 512) hipLaunchKernelGGL((attn_bwd_dkv64_kernel<PK, 8, 128>), dim3((S + 255) / 256, H, B), dim3(512), 0, st,   \
                       (const bf16_t*)qkv, (const bf16_t*)dout, lse, delta_ws, KR, (bf16_t*)dqkv, B, S, H, causal, D, R);          \
    else hipLaunchKernelGGL((attn_bwd_dkv64_kernel<PK, 8>), dim3((S + 255) / 256, H, B), dim3(512), 0, st, (const bf16_t*)qkv,       \
                       (const bf16_t*)dout, lse, delta_ws, KR, (bf16_t*)dqkv, B, S, H, causal, D, R);                              \
  } while (0)
    // dQ: 4-wave blocks at 3 waves / SIMD (168 registers; the 128-register 8-wave build spills in its dropout / edge paths and
    // runs 1216 us against 894 for the pair); dK/dV: 8-wave blocks at 2 waves / SIMD (two independent 4-wave blocks per CU, whose
    // waves are not barrier-locked to their SIMD partner, measured equal: 872 / 1071 us against 850 / 1081 for the pair)
    if (key_lo) GGET_BWD64(true);
    else GGET_BWD64(false);
#undef GGET_BWD64
    GGET_LAUNCH_CHECK();
    return 0;
  }
  const int nw = attn_waves(S);
  dim3 grid((S + 32 * nw - 1) / (32 * nw), H, B);
#define GGET_ATTN_BWD(NW, PK)                                                                                                \
  do {                                                                                                                     \
    hipLaunchKernelGGL((attn_bwd_dq_kernel<NW, PK>), grid, dim3(NW * 64), 0, st, (const bf16_t*)qkv, (const bf16_t*)out,     \
                       (const bf16_t*)dout, lse,   \
                       delta_ws, KR, (bf16_t*)dqkv, B, S, H, causal, Rin, R, D);                                      \
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<NW, PK>), grid, dim3(NW * 64), 0, st, (const bf16_t*)qkv, (const bf16_t*)dout, lse,  \
                       delta_ws, KR, (bf16_t*)dqkv, B, S, H, causal, Rin, R, D);                                      \
  } while (0)
  if (key_lo) { if (nw == 4) GGET_ATTN_BWD(4, true); else if (nw == 2) GGET_ATTN_BWD(2, true); else GGET_ATTN_BWD(1, true); }
  else { if (nw == 4) GGET_ATTN_BWD(4, false); else if (nw == 2) GGET_ATTN_BWD(2, false); else GGET_ATTN_BWD(1, false); }
#undef GGET_ATTN_BWD
  GGET_LAUNCH_CHECK();
  return 0;
}

#ifdef GGET_ATTN_STAMPS
extern "C" int gget_debug_attn_stamps(unsigned long long* host_out /* [8][40][16] */) {
  GGET_HIP_CHECK(hipDeviceSynchronize());
  GGET_HIP_CHECK(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_attn_stamps), sizeof(unsigned long long) * 8 * 40 * 16));
  return 0;
}
#endif
