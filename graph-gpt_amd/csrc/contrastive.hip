// Contrastive pre-training head (task_type = "pretrain-cl"): cl_proj on the pooled row, L2 normalisation, the symmetric InfoNCE loss
// between the two views of every graph, and its backward.
// replaces: GraphGPTPretrainBase.cl_proj + the discriminative branch of its forward (src/models/graphgpt/modeling_pretrain.py:96-115,
// :238-257), _get_sequence_len / the pooled row (modeling_helpers.py:201-227) and the contrastive loss with its all-gather
// (src/utils/loss_utils.py:89-167).
//
//   z_b = W h_b  (h_b = hidden[pool_row[b]], bf16; fp32 accumulation)        e_b = z_b / max(|z_b|, 1e-12)
//   E [N, d] fp32: the caller's own rows (N = B) or the gathered matrix of all ranks; p(i) = i ^ 1 is the other view of row i
//   scores[i][j] = 20 <E[i], E[p(j)]>, scores[i][p(i)] (the self-similarity) masked; loss = ratio / 2 (CE(scores, arange) + CE(scores^T, arange))
//
// Symmetry.  With S = 20 E E^T (symmetric) the row term of i is  lse_{k != i} S[i][k] - S[i][p(i)]  (j runs over all columns, so p(j) runs
// over all rows k; the masked column is k = i).  The transposed term of i is  lse_{j != p(i)} 20 <E[j], E[p(i)]> - 20 <E[i], E[p(i)]>, which
// is the row term of p(i): both cross-entropies sum the same N terms, and loss = ratio / N sum_i (lse_i - S[i][p(i)]).  The kernels
// compute that; tests/_cl_ref.py states both cross-entropies literally in float64.
//
// Gradient.  dloss / dS[i][k] = ratio / N (P[i][k] - [k == p(i)]) from row i, P[i][k] = exp(S[i][k] - lse_i) (k != i).  Row i of E meets
// S[i][k] as the query of its own term and as the key of row k's term:
//   dE_i = 20 g ratio / N  sum_{k != i} (P[i][k] + P[k][i] - 2 [k == p(i)]) E_k          (g = the upstream gradient)
//   dz_i = (dE_i - e_i <e_i, dE_i>) / |z_i|     dW += dz^T h     dhidden[pool_row[b]] += dz_b W
// Only the caller's own rows receive a gradient (the reference's GatherLayer hands back the local slice).
//
// Every sum has a fixed order (wave partials combined in wave order, samples in batch order): no atomics, two calls give the same bits.
#include <math.h>

#include "common.h"
#include "kernels.h"
#include "../../include/gget.h"

namespace {

constexpr int kClBlock = 256;          // 4 waves
constexpr int kClWaves = kClBlock / 64;
constexpr int kClMaxD = 1024;
constexpr int kClMaxN = 2048;
constexpr int kClQ = 4;                // query rows one workgroup of the loss kernel keeps in LDS
constexpr int kClChunks = kClMaxD / 4 / 64;   // float4 chunks of one embedding row a lane holds (4)
constexpr float kClTemp = 20.0f;       // 1 / temperature (loss_utils.py:89-167: temperature 0.05)
constexpr float kClEps = 1e-12f;       // F.normalize eps
constexpr int kClRows = 4;             // rows (of cl_proj's weight, or keys of the backward) a wave keeps in flight together
constexpr int kClDwTile = 64;          // dW tile edge
constexpr int kClDwRows = 16;          // samples staged per round of the dW kernel

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// the float4 chunks lane + 64 t (t < kClChunks) of row `p` (zeros past d)
__device__ __forceinline__ void cl_load_row(const float* __restrict__ p, int d4, int lane, float4 (&v)[kClChunks]) {
#pragma unroll
  for (int t = 0; t < kClChunks; ++t) {
    const int c = lane + 64 * t;
    v[t] = c < d4 ? ld4(p + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
// <v, q> with q in LDS, summed over the wave
__device__ __forceinline__ float cl_dot_lds(const float4 (&v)[kClChunks], const float* q, int d4, int lane) {
  float a = 0.f;
#pragma unroll
  for (int t = 0; t < kClChunks; ++t) {
    const int c = lane + 64 * t;
    if (c < d4) {
      const float4 w = *reinterpret_cast<const float4*>(q + 4 * c);
      a = fmaf(v[t].x, w.x, a); a = fmaf(v[t].y, w.y, a); a = fmaf(v[t].z, w.z, a); a = fmaf(v[t].w, w.w, a);
    }
  }
  return wave_sum(a);
}
// sum over the workgroup in wave order; red: kClWaves floats of LDS (reusable after the call)
__device__ __forceinline__ float cl_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < kClWaves; ++w) s += red[w];
  return s;
}

// ---- z = W h, e = z / max(|z|, eps): one workgroup per sample, a wave per output row ----
__global__ void __launch_bounds__(kClBlock) cl_embed_fwd_kernel(const bf16_t* __restrict__ hidden, const int32_t* __restrict__ pool_row,
                                                                const bf16_t* __restrict__ w, float* __restrict__ z, float* __restrict__ e,
                                                                float* __restrict__ rnorm, int d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cl_lds[];
  float* hs = reinterpret_cast<float*>(cl_lds);   // [d]
  float* zs = hs + d;                             // [d]
  float* red = zs + d;                            // [kClWaves]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16_t* hrow = hidden + (size_t)pool_row[b] * d;
  const int d8 = d / 8;
  for (int c = tid; c < d8; c += kClBlock) {
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(hrow + 8 * c), f);
#pragma unroll
    for (int u = 0; u < 8; ++u) hs[8 * c + u] = f[u];
  }
  __syncthreads();
  // kClRows output rows at a time: their loads and their wave reductions are independent chains in flight together (d % 16 == 0)
  for (int o0 = wave * kClRows; o0 < d; o0 += kClWaves * kClRows) {
    float a[kClRows];
#pragma unroll
    for (int r = 0; r < kClRows; ++r) a[r] = 0.f;
    for (int c = lane; c < d8; c += 64) {
      uint4 raw[kClRows];
#pragma unroll
      for (int r = 0; r < kClRows; ++r) raw[r] = *reinterpret_cast<const uint4*>(w + (size_t)(o0 + r) * d + 8 * c);
#pragma unroll
      for (int r = 0; r < kClRows; ++r) {
        float f[8];
        unpack8(raw[r], f);
#pragma unroll
        for (int u = 0; u < 8; ++u) a[r] = fmaf(f[u], hs[8 * c + u], a[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < kClRows; ++r) a[r] = wave_sum(a[r]);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < kClRows; ++r) zs[o0 + r] = a[r];
    }
  }
  __syncthreads();
  float ss = 0.f;
  for (int j = tid; j < d; j += kClBlock) ss = fmaf(zs[j], zs[j], ss);
  ss = cl_block_sum(ss, red);
  const float rn = 1.0f / fmaxf(sqrtf(ss), kClEps);
  for (int c = tid; c < d / 4; c += kClBlock) {
    const float4 v = *reinterpret_cast<const float4*>(zs + 4 * c);
    *reinterpret_cast<float4*>(z + (size_t)b * d + 4 * c) = v;
    *reinterpret_cast<float4*>(e + (size_t)b * d + 4 * c) = make_float4(v.x * rn, v.y * rn, v.z * rn, v.w * rn);
  }
  if (tid == 0) rnorm[b] = rn;
}

// ---- row statistics of S = 20 E E^T without its diagonal: kClQ query rows per workgroup, the key rows stream through the waves ----
// stat [3][N]: row max, log-sum-exp, lse - S[i][p(i)] (the row's loss term)
__global__ void __launch_bounds__(kClBlock) cl_loss_rows_kernel(const float* __restrict__ E, float* __restrict__ stat, int N, int d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cl_lds[];
  float* q = reinterpret_cast<float*>(cl_lds);    // [kClQ][d]
  float* wm = q + kClQ * d;                       // [kClWaves][kClQ] running max
  float* wsum = wm + kClWaves * kClQ;             // [kClWaves][kClQ] running sum
  float* wpos = wsum + kClWaves * kClQ;           // [kClQ] S[i][p(i)]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * kClQ, d4 = d / 4;
  for (int c = tid; c < kClQ * d4; c += kClBlock) {
    const int r = c / d4, cc = c % d4;
    *reinterpret_cast<float4*>(q + (size_t)r * d + 4 * cc) =
        i0 + r < N ? ld4(E + (size_t)(i0 + r) * d + 4 * cc) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  float m[kClQ], s[kClQ];
#pragma unroll
  for (int r = 0; r < kClQ; ++r) { m[r] = -INFINITY; s[r] = 0.f; }
  // two keys at a time: eight dot products and their wave reductions in flight together; the running sums take the keys in order
  for (int k0 = wave * 2; k0 < N; k0 += kClWaves * 2) {     // (N is even: k0 + 1 < N)
    float4 ek[2][kClChunks];
    float sc[2][kClQ];
#pragma unroll
    for (int u = 0; u < 2; ++u) cl_load_row(E + (size_t)(k0 + u) * d, d4, lane, ek[u]);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < kClQ; ++r) sc[u][r] = kClTemp * cl_dot_lds(ek[u], q + (size_t)r * d, d4, lane);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = k0 + u;
#pragma unroll
      for (int r = 0; r < kClQ; ++r) {
        const int i = i0 + r;
        if (k == i || i >= N) continue;     // the masked self-similarity contributes exp(-max float) = 0
        if (k == (i ^ 1) && lane == 0) wpos[r] = sc[u][r];
        const float mn = fmaxf(m[r], sc[u][r]);
        s[r] = s[r] * __expf(m[r] - mn) + __expf(sc[u][r] - mn);
        m[r] = mn;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < kClQ; ++r) { wm[wave * kClQ + r] = m[r]; wsum[wave * kClQ + r] = s[r]; }
  }
  __syncthreads();
  if (tid < kClQ && i0 + tid < N) {
    const int r = tid, i = i0 + r;
    float mx = wm[r];
    for (int w = 1; w < kClWaves; ++w) mx = fmaxf(mx, wm[w * kClQ + r]);
    float tot = 0.f;
    for (int w = 0; w < kClWaves; ++w) tot += wsum[w * kClQ + r] * __expf(wm[w * kClQ + r] - mx);   // (a wave without keys: 0 * exp(-inf) = 0)
    const float lse = mx + __logf(tot);
    stat[i] = mx;
    stat[N + i] = lse;
    stat[2 * N + i] = lse - wpos[r];
  }
}
// loss = ratio / N * sum_i term_i, the terms added in row order by one workgroup
__global__ void __launch_bounds__(kClBlock) cl_loss_finish_kernel(const float* __restrict__ stat, float* __restrict__ loss, int N, float ratio) {
  __shared__ float red[kClWaves];
  float a = 0.f;
  for (int i = threadIdx.x; i < N; i += kClBlock) a += stat[2 * N + i];
  a = cl_block_sum(a, red);
  if (threadIdx.x == 0) loss[0] = ratio * (a / (float)N);
}

// ---- backward of one local row: dE (query and key side), dz, and dhidden[pool_row] += dz W ----
__global__ void __launch_bounds__(kClBlock) cl_bwd_rows_kernel(const float* __restrict__ E, const float* __restrict__ stat,
                                                               const int32_t* __restrict__ row_map, const float* __restrict__ rnorm,
                                                               const int32_t* __restrict__ pool_row, const bf16_t* __restrict__ w,
                                                               float coef, float* __restrict__ dz, bf16_t* __restrict__ dhidden, int N, int d,
                                                               int part_floats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cl_lds[];
  float* q = reinterpret_cast<float*>(cl_lds);    // [d]: e_i, later dz_i
  float* part = q + d;                            // [part_floats]: per-wave partial dE, later the per-group partial dh
  float* red = part + part_floats;                // [kClWaves]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d4 = d / 4;
  int i = row_map ? row_map[b] : b;
  i = i < 0 ? 0 : (i >= N ? N - 1 : i);
  for (int c = tid; c < d4; c += kClBlock) *reinterpret_cast<float4*>(q + 4 * c) = ld4(E + (size_t)i * d + 4 * c);
  __syncthreads();
  const float lse_i = stat[N + i];
  float4 acc[kClChunks];
#pragma unroll
  for (int t = 0; t < kClChunks; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  // kClRows keys at a time (loads and dot products in flight together), accumulated in key order
  for (int k0 = wave * kClRows; k0 < N; k0 += kClWaves * kClRows) {
    float4 ek[kClRows][kClChunks];
    float sc[kClRows];
#pragma unroll
    for (int r = 0; r < kClRows; ++r) cl_load_row(E + (size_t)min(k0 + r, N - 1) * d, d4, lane, ek[r]);
#pragma unroll
    for (int r = 0; r < kClRows; ++r) sc[r] = kClTemp * cl_dot_lds(ek[r], q, d4, lane);
#pragma unroll
    for (int r = 0; r < kClRows; ++r) {
      const int k = k0 + r;
      if (k >= N || k == i) continue;
      // query side P[i][k], key side P[k][i] (S is symmetric), and the target column of both cross-entropies
      const float g = coef * (__expf(sc[r] - lse_i) + __expf(sc[r] - stat[N + k]) - (k == (i ^ 1) ? 2.0f : 0.0f));
#pragma unroll
      for (int t = 0; t < kClChunks; ++t) {
        acc[t].x = fmaf(g, ek[r][t].x, acc[t].x); acc[t].y = fmaf(g, ek[r][t].y, acc[t].y);
        acc[t].z = fmaf(g, ek[r][t].z, acc[t].z); acc[t].w = fmaf(g, ek[r][t].w, acc[t].w);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < kClChunks; ++t) {
    const int c = lane + 64 * t;
    if (c < d4) *reinterpret_cast<float4*>(part + (size_t)wave * d + 4 * c) = acc[t];
  }
  __syncthreads();
  float dot = 0.f;
  for (int j = tid; j < d; j += kClBlock) {
    float v = part[j];
#pragma unroll
    for (int ww = 1; ww < kClWaves; ++ww) v += part[(size_t)ww * d + j];
    part[j] = v;                        // dE_i[j] (this thread's element only)
    dot = fmaf(q[j], v, dot);
  }
  dot = cl_block_sum(dot, red);
  const float rn = rnorm[b];
  if (rn >= 1.0f / kClEps) dot = 0.f;   // |z| below eps: e = z / eps, no projection term
  for (int j = tid; j < d; j += kClBlock) q[j] = (part[j] - q[j] * dot) * rn;
  __syncthreads();
  for (int c = tid; c < d4; c += kClBlock) *reinterpret_cast<float4*>(dz + (size_t)b * d + 4 * c) = *reinterpret_cast<const float4*>(q + 4 * c);
  // dh = dz W: 8 columns per thread (16-byte loads of W's rows), the d rows of W dealt out to `groups` thread groups
  const int d8 = d / 8, groups = kClBlock / d8;
  const int grp = tid / d8, cg = tid % d8;
  if (grp < groups) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int o0 = grp; o0 < d; o0 += groups * kClRows) {      // kClRows rows of W in flight together, added in row order
      uint4 raw[kClRows];
#pragma unroll
      for (int r = 0; r < kClRows; ++r) raw[r] = *reinterpret_cast<const uint4*>(w + (size_t)min(o0 + r * groups, d - 1) * d + 8 * cg);
#pragma unroll
      for (int r = 0; r < kClRows; ++r) {
        const int o = o0 + r * groups;
        if (o >= d) break;
        float f[8];
        unpack8(raw[r], f);
        const float zo = q[o];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = fmaf(zo, f[u], a[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) part[(size_t)grp * d + 8 * cg + u] = a[u];
  }
  __syncthreads();
  // added onto what the row already holds (the generative head's gradient): bf16 read, fp32 sum, one rounding
  bf16_t* drow = dhidden + (size_t)pool_row[b] * d;
  for (int jp = tid; jp < d / 2; jp += kClBlock) {
    float v0 = 0.f, v1 = 0.f;
    for (int gq = 0; gq < groups; ++gq) { v0 += part[(size_t)gq * d + 2 * jp]; v1 += part[(size_t)gq * d + 2 * jp + 1]; }
    const unsigned old = *reinterpret_cast<const unsigned*>(drow + 2 * jp);
    *reinterpret_cast<unsigned*>(drow + 2 * jp) = pack2bf(__uint_as_float(old << 16) + v0, __uint_as_float(old & 0xffff0000u) + v1);
  }
}

// ---- dW[o][c] += sum_b dz[b][o] h[pool_row[b]][c]: 64 x 64 tiles, 4 x 4 outputs per thread, the samples in batch order ----
__global__ void __launch_bounds__(kClBlock) cl_dw_kernel(const float* __restrict__ dz, const bf16_t* __restrict__ hidden,
                                                         const int32_t* __restrict__ pool_row, float* __restrict__ dw, int B, int d) {
  __shared__ __attribute__((aligned(16))) float za[kClDwRows][kClDwTile];
  __shared__ __attribute__((aligned(16))) float ha[kClDwRows][kClDwTile];
  const int tid = threadIdx.x, ty = tid / 16, tx = tid % 16;
  const int o0 = blockIdx.y * kClDwTile, c0 = blockIdx.x * kClDwTile;
  float acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
  const int lr = tid / 16, lc = (tid % 16) * 4;     // this thread's staging slot: sample lr of the round, 4 columns from lc
  // this thread's share of the round that starts at sample b0 (zeros past B)
  auto stage = [&](int b0, float4& zv, uint2& raw) {
    const int b = b0 + lr;
    zv = make_float4(0.f, 0.f, 0.f, 0.f);
    raw = make_uint2(0u, 0u);
    if (b < B) {
      zv = ld4(dz + (size_t)b * d + o0 + lc);
      raw = *reinterpret_cast<const uint2*>(hidden + (size_t)pool_row[b] * d + c0 + lc);
    }
  };
  float4 zv;
  uint2 raw;
  stage(0, zv, raw);
  for (int b0 = 0; b0 < B; b0 += kClDwRows) {
    __syncthreads();
    *reinterpret_cast<float4*>(&za[lr][lc]) = zv;
    *reinterpret_cast<float4*>(&ha[lr][lc]) = make_float4(__uint_as_float(raw.x << 16), __uint_as_float(raw.x & 0xffff0000u),
                                                           __uint_as_float(raw.y << 16), __uint_as_float(raw.y & 0xffff0000u));
    __syncthreads();
    if (b0 + kClDwRows < B) stage(b0 + kClDwRows, zv, raw);      // the next round's loads fly under this round's products
#pragma unroll
    for (int r = 0; r < kClDwRows; ++r) {
      const float4 a = *reinterpret_cast<const float4*>(&za[r][ty * 4]);
      const float4 hh = *reinterpret_cast<const float4*>(&ha[r][tx * 4]);
      const float av[4] = {a.x, a.y, a.z, a.w}, hq[4] = {hh.x, hh.y, hh.z, hh.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(av[u], hq[v], acc[u][v]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    float* p = dw + (size_t)(o0 + ty * 4 + u) * d + c0 + tx * 4;
    const float4 old = ld4(p);
    *reinterpret_cast<float4*>(p) = make_float4(old.x + acc[u][0], old.y + acc[u][1], old.z + acc[u][2], old.w + acc[u][3]);
  }
}

#define GGET_CL_REQUIRE_D(d) \
  GGET_REQUIRE((d) > 0 && (d) % 64 == 0 && (d) <= kClMaxD, "contrastive head: d=%d unsupported (d %% 64 == 0, d <= 1024)", (d))
#define GGET_CL_REQUIRE_N(N) \
  GGET_REQUIRE((N) >= 2 && (N) <= kClMaxN && (N) % 2 == 0, "contrastive head: N=%d unsupported (2 <= N <= 2048, N even)", (N))

}  // namespace

int k_cl_embed_fwd(const void* hidden, const int32_t* pool_row, const void* w, float* z, float* e, float* rnorm, int B, int d, hipStream_t st) {
  GGET_CL_REQUIRE_D(d);
  GGET_REQUIRE(B >= 0, "contrastive head: negative batch");
  if (B == 0) return 0;
  const int lds = (2 * d + kClWaves) * 4;
  hipLaunchKernelGGL(cl_embed_fwd_kernel, dim3(B), dim3(kClBlock), lds, st, (const bf16_t*)hidden, pool_row, (const bf16_t*)w, z, e, rnorm, d);
  GGET_LAUNCH_CHECK();
  return 0;
}

int k_cl_loss_fwd(const float* E, int N, int d, float ratio, float* stat, float* loss, hipStream_t st) {
  GGET_CL_REQUIRE_D(d);
  GGET_CL_REQUIRE_N(N);
  const int lds = (kClQ * d + 2 * kClWaves * kClQ + kClQ) * 4;
  hipLaunchKernelGGL(cl_loss_rows_kernel, dim3((N + kClQ - 1) / kClQ), dim3(kClBlock), lds, st, E, stat, N, d);
  hipLaunchKernelGGL(cl_loss_finish_kernel, dim3(1), dim3(kClBlock), 0, st, (const float*)stat, loss, N, ratio);
  GGET_LAUNCH_CHECK();
  return 0;
}

int k_cl_bwd(const float* E, const float* stat, const int32_t* row_map, const float* rnorm, const void* hidden, const int32_t* pool_row,
             const void* w, float scale, float* dz, float* dw, void* dhidden, int N, int B, int d, hipStream_t st) {
  GGET_CL_REQUIRE_D(d);
  GGET_CL_REQUIRE_N(N);
  GGET_REQUIRE(B >= 0 && B <= N, "contrastive head: %d local rows of N=%d", B, N);
  if (B == 0) return 0;
  const int part = 4 * d > 2048 ? 4 * d : 2048;      // kClWaves partial rows of dE; (256 / (d / 8)) partial rows of dh = at most 2048 floats
  const int lds = (d + part + kClWaves) * 4;
  const float coef = kClTemp * scale / (float)N;
  hipLaunchKernelGGL(cl_bwd_rows_kernel, dim3(B), dim3(kClBlock), lds, st, E, stat, row_map, rnorm, pool_row, (const bf16_t*)w, coef, dz,
                     (bf16_t*)dhidden, N, d, part);
  hipLaunchKernelGGL(cl_dw_kernel, dim3(d / kClDwTile, d / kClDwTile), dim3(kClBlock), 0, st, (const float*)dz, (const bf16_t*)hidden, pool_row,
                     dw, B, d);
  GGET_LAUNCH_CHECK();
  return 0;
}

// ---- operator-level entry points (include/gget.h) ----
extern "C" int gget_op_cl_embed_fwd(const void* hidden, const int32_t* pool_row, const void* w, float* z, float* e, float* rnorm, int B,
                                    int d, void* stream) {
  GGET_REQUIRE(hidden && pool_row && w && z && e && rnorm, "cl_embed_fwd: null argument");
  return k_cl_embed_fwd(hidden, pool_row, w, z, e, rnorm, B, d, (hipStream_t)stream);
}
extern "C" int gget_op_cl_loss_fwd(const float* E, int N, int d, float ratio, float* stat, float* loss, void* stream) {
  GGET_REQUIRE(E && stat && loss, "cl_loss_fwd: null argument");
  return k_cl_loss_fwd(E, N, d, ratio, stat, loss, (hipStream_t)stream);
}
extern "C" int gget_op_cl_bwd(const float* E, const float* stat, const int32_t* row_map, const float* rnorm, const void* hidden,
                              const int32_t* pool_row, const void* w, float scale, float* dz, float* dw, void* dhidden, int N, int B, int d,
                              void* stream) {
  GGET_REQUIRE(E && stat && rnorm && hidden && pool_row && w && dz && dw && dhidden, "cl_bwd: null argument");
  return k_cl_bwd(E, stat, row_map, rnorm, hidden, pool_row, w, scale, dz, dw, dhidden, N, B, d, (hipStream_t)stream);
}
