// What the attention units share (attention.hip: head width 64, attention32.hip: head width 32): the RoPE operand, the counter-hash
// attention dropout, the key restriction of a launch and the clamped-row load helpers.  One definition, so the two families draw the
// same dropout mask and mean the same thing by a key range.
#pragma once
#include <algorithm>

#include "common.h"

namespace {

// RoPE (hf apply_rotary_pos_emb :138-160, half-split pairing j <-> j + head_dim/2).  The 64-wide kernels may rotate q and k on the
// operand loads (q and k un-rotated in HBM) and rotate dq/dk back on the way out; the 32-wide ones only rotate dq/dk back.
struct Rope {
  const float* cos_tab;  // [max_pos][head_dim/2] fp32, nullptr => no rotation (plain attention op)
  const float* sin_tab;
  const int64_t* pos;    // [B,S] or nullptr => position = index in the sequence
  int S;
};
__device__ __forceinline__ int rope_pos(const Rope& R, int b, int s) {
  return R.pos ? (int)R.pos[(size_t)b * R.S + s] : s;
}

// Global loads of these helpers are UNCONDITIONAL: the row index is clamped into the sample ([0, row_lim - 1], at least 0) and rows
// beyond the limit are zeroed with a select afterwards.  Written as `if (row < row_lim) v = load` the compiler branches around every
// load and waits vmcnt(0) behind each one (round 3, ISA of the S <= 32 kernels: twelve serialised load -> wait -> ds_write round trips
// per problem plus four for the V fragments - the kernels were bound by that chain, not by bytes); the RoPE test is made once per tile,
// outside the chunk loops, for the same reason.
__device__ __forceinline__ uint4 zero_if(bool dead, const uint4& v) {
  return make_uint4(dead ? 0u : v.x, dead ? 0u : v.y, dead ? 0u : v.z, dead ? 0u : v.w);
}
__device__ __forceinline__ int clamp_row(int gr, int row_lim) { return max(min(gr, row_lim - 1), 0); }

// Attention dropout (hf eager_attention_forward :210: dropout on the softmax output, training only; every reference
// launch script sets attention_dropout=0.1).  Counter-based: the keep decision of element (batch*head, query, key) is a
// hash of (seed, coordinates), so forward and the two backward kernels regenerate the same mask without storing it.
struct Drop {
  unsigned thresh;   // drop when the 16-bit field < thresh  (thresh = p * 2^16); 0 => no dropout
  float inv_keep;    // 1 / (1 - p)
  unsigned seed;
};
// One hash serves TWO scores: w(seed, bh, q, k >> 1) = mix((seed ^ bh*C0) + q*C1 + (k>>1)*C2), mix = one multiply between two
// xor-shifts; key k uses the low (k even) or high (k odd) 16 bits of w.  The multiply is the full-rate 24-bit one (v_mul_u32_u24:
// low 24 bits of the folded word x a 24-bit constant, low 32 bits of the product); a hash word is {v_add, v_xor sdwa, v_mul_u32_u24,
// v_lshrrev, v_xor}.  (Round 3: replacing the quarter-rate 32-bit multiply changed NO kernel time - B16/S2048/H12 with p = 0.1: forward
// 438.6 us, backward 1097 us before and after; what the dropout costs at head_dim 64 is its instruction COUNT beside the MFMAs, five
// per score on top of 6.6, not the rate of any one of them.  The 24-bit mix stays for its better mask statistics.)
// Measured on 3 x 6.3 M scores (tools/drop_hash_eval.py): drop rates 0.1000-0.1003 / 0.2997-0.3003 for
// p = 0.1 / 0.3 in both fields; correlations between the two fields of a word, keys 1 / 2 apart, queries 1 / 2 apart, neighbouring
// heads and the two diagonals all <= 1.5e-3 (noise floor 4e-4; the 32-bit multiply it replaces: <= 5e-3); per-row and per-column
// drop-rate dispersion 0.98-1.02 of binomial.  In the kernels whose lanes walk along keys (forward, dQ) a lane's accumulator
// registers come in (k, k+1) pairs, so one word serves two scores.  Callers pass the partial sum of everything fixed for the lane
// (drop_base) and add the moving term.  tests/test_gpu_ops.py:_drop_mask is the Python twin.  bh = b * H + h with H the launch's
// head count (hidden / head width).
__device__ __forceinline__ unsigned drop_base(const Drop& D, unsigned bh, unsigned q_or_0, unsigned khalf_or_0) {
  return (D.seed ^ (bh * 0x9E3779B1u)) + q_or_0 * 0x85EBCA77u + khalf_or_0 * 0xC2B2AE3Du;
}
__device__ __forceinline__ unsigned drop_word(unsigned x) {
  x ^= x >> 16;
  x = __umul24(x, 0x9E3779u);
  x ^= x >> 15;
  return x;
}
// keep-multiplier of key parity `odd` from the pair's hash word
__device__ __forceinline__ float drop_mul_w(const Drop& D, unsigned w, int odd) {
  const unsigned f = odd ? (w >> 16) : (w & 0xffffu);
  return f < D.thresh ? 0.f : D.inv_keep;
}
// single score: x = drop_base(D, bh, q, 0) + (k >> 1) * C2 already summed by the caller
__device__ __forceinline__ float drop_mul_x(const Drop& D, unsigned x, int odd) {
  if (D.thresh == 0) return 1.f;
  return drop_mul_w(D, drop_word(x), odd);
}
inline Drop make_drop(float p, unsigned seed) {
  Drop d;
  d.thresh = p > 0.f ? (unsigned)(p * 65536.0f) : 0u;
  d.inv_keep = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
  d.seed = seed;
  return d;
}

// Which keys a query may attend: right padding gives one length per batch row (key_len[b], keys [0, len)); packed rows
// (several graphs back to back, block-diagonal [B,S,S] mask of reference src/utils/tokenizer_utils.py:349-355 /
// modeling_helpers.py:51-64) give every token the inclusive key range [lo, hi] of its own graph.
struct KeyRange {
  const int32_t* key_len;   // [B] or nullptr (=> S); ignored when lo/hi are given
  const int32_t* lo;        // [B,S] or nullptr
  const int32_t* hi;        // [B,S]
  // var-len (padding-free) token layout: first row of sample b in the token-major buffers (qkv / out / dout / dqkv); its rows are
  // [row_base[b], row_base[b] + key_len[b]).  nullptr = padded layout, sample b at rows [b * S, b * S + S).  Logical [B,S] arrays
  // (lse, delta, position ids, the dropout hash coordinates) keep their (b, s) indexing in both layouts.  Not combined with lo / hi.
  const int32_t* row_base;
};
// wave-uniform min / max of small non-negative integers (exact in fp32)
__device__ __forceinline__ int wave_imin(int v) { return (int)-wave_max(-(float)v); }
__device__ __forceinline__ int wave_imax(int v) { return (int)wave_max((float)v); }

// accumulator registers [8j, 8j+8) of a 32x32 MFMA result -> bf16 B operand of the next one (k = the result's rows
// {16j + 4hi + (e&3) + 8(e>>2)}, the order of the transposing LDS reads)
__device__ __forceinline__ bf16x8_t acc_to_b(const f32x16_t& a, int j) {
  uint4 v;
  v.x = pack2bf(a[8 * j + 0], a[8 * j + 1]);
  v.y = pack2bf(a[8 * j + 2], a[8 * j + 3]);
  v.z = pack2bf(a[8 * j + 4], a[8 * j + 5]);
  v.w = pack2bf(a[8 * j + 6], a[8 * j + 7]);
  return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ int acc_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

__device__ __forceinline__ f32x16_t zero16() {
  f32x16_t z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

}  // namespace
