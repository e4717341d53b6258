// Update and scoring steps of the generation evaluation (reference src/utils/generation_utils.py:138-237, :317-463 and
// src/utils/log_eval_dump_utils.py:308-447) as integer / compare work: nothing here sums floats, so every result is exact and the same
// from run to run.
//
//   unmask_ranked_kernel  one workgroup per sample: counts the sample's <mask> cells, n = floor(n_masked * p) with ONE fp32 multiply, and
//                         writes the candidates of the n most confident masked cells (ties: lower cell index first - the order of
//                         torch.sort(descending=True, stable=True)).  Radix select on an order-preserving 32-bit key, most significant
//                         byte first: four histogram passes over the (L2-resident) row find the key of the n-th cell and how many cells
//                         of that key are still owed; a last pass in index order writes every masked cell above the key and the first
//                         owed cells of the key by a running prefix count.  LDS: one 256-bin histogram and a few words, whatever N is.
//   gen_plan_kernel       the batch's step rule (:171-184): from max_b n_masked[b] advance i through the p table until
//                         floor(max * p_tab[i]) >= 1 (floor(n * p) is monotone in n, so the maximum decides k) or i == steps.
//   gen_acc_kernel        per sample {sum (gen == labels) & (input_ids == mask), sum (input_ids == mask)}.
#include <math.h>

#include "common.h"
#include "../../include/gget.h"

namespace {

constexpr int kGenBlock = 256;                 // threads of the per-sample launches = bins of the radix histogram
constexpr int kGenWaves = kGenBlock / 64;
constexpr int kPlanBlock = 1024;               // gen_plan_kernel: one workgroup, a wave per sample
constexpr int kPlanWaves = kPlanBlock / 64;

// larger confidence <=> larger key; -0.0 and +0.0 compare equal as floats and share a key
__device__ __forceinline__ unsigned conf_key(float c) {
  unsigned b = __float_as_uint(c);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the workgroup, returned to every thread; `red` (kGenWaves words of LDS) is free again on return
__device__ __forceinline__ int block_sum_int(int v, int* red) {
  v = wave_sum_int(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < kGenWaves; ++w) s += red[w];
  __syncthreads();
  return s;
}

__global__ void __launch_bounds__(kGenBlock) unmask_ranked_kernel(int64_t* __restrict__ x, const float* __restrict__ conf,
                                                                  const int64_t* __restrict__ cand, int N, int64_t mask_id,
                                                                  const float* __restrict__ p, int p_stride,
                                                                  int32_t* __restrict__ n_revealed) {
  __shared__ unsigned hist[kGenBlock];
  __shared__ int red[kGenWaves];
  __shared__ unsigned sel[2];                  // digit of the pass, cells still owed inside it
  __shared__ int tie_cnt[2][kGenWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int64_t* xr = x + (size_t)b * N;
  const float* cf = conf + (size_t)b * N;
  const int64_t* cr = cand + (size_t)b * N;

  int cnt = 0;
  for (int c = tid; c < N; c += kGenBlock) cnt += xr[c] == mask_id;
  const int n_masked = block_sum_int(cnt, red);
  const float scaled = (float)n_masked * p[(size_t)b * p_stride];     // the one fp32 multiply of torch.floor(n_masked * p)
  int n = (int)floorf(scaled);
  n = max(0, min(n, n_masked));
  if (tid == 0 && n_revealed) n_revealed[b] = n;
  if (n == 0) return;
  if (n == n_masked) {                         // the last step (p = 1): every masked cell, no ranking
    for (int c = tid; c < N; c += kGenBlock)
      if (xr[c] == mask_id) xr[c] = cr[c];
    return;
  }

  // the key of the n-th most confident masked cell: fix its bytes from the top, `owed` counts the cells still to find among the keys
  // that share the fixed bytes
  unsigned prefix = 0u, fixed = 0u;
  int owed = n;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0u;
    __syncthreads();
    for (int c = tid; c < N; c += kGenBlock) {
      if (xr[c] != mask_id) continue;
      const unsigned k = conf_key(cf[c]);
      if ((k & fixed) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (wv == 0) {                             // lane l owns bins 255 - 4l .. 252 - 4l: a scan from the largest digit down
      unsigned h[4], s = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) { h[j] = hist[255 - 4 * lane - j]; s += h[j]; }
      unsigned incl = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      unsigned above = incl - s;               // cells in larger digits
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (above < (unsigned)owed && (unsigned)owed <= above + h[j]) { sel[0] = 255u - 4u * lane - j; sel[1] = (unsigned)owed - above; }
        above += h[j];
      }
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    fixed |= 0xFFu << shift;
    owed = (int)sel[1];
    __syncthreads();
  }

  // cells above the key all reveal; of the cells AT the key the first `owed` in index order
  int running = 0;
  for (int base = 0, it = 0; base < N; base += kGenBlock, ++it) {
    const int c = base + tid;
    bool above = false, tie = false;
    if (c < N && xr[c] == mask_id) {
      const unsigned k = conf_key(cf[c]);
      above = k > prefix;
      tie = k == prefix;
    }
    const unsigned long long bal = __ballot(tie);
    if (lane == 0) tie_cnt[it & 1][wv] = __popcll(bal);
    __syncthreads();                           // (two buffers: the next round's writers cannot pass this round's readers)
    int before = running, total = 0;
#pragma unroll
    for (int w = 0; w < kGenWaves; ++w) {
      const int t = tie_cnt[it & 1][w];
      before += w < wv ? t : 0;
      total += t;
    }
    const int rank = before + __popcll(bal & ((1ull << lane) - 1ull));
    if (above || (tie && rank < owed)) xr[c] = cr[c];
    running += total;
  }
}

__global__ void __launch_bounds__(kPlanBlock) gen_plan_kernel(const int64_t* __restrict__ x, int B, int N, int64_t mask_id,
                                                              const float* __restrict__ p_tab, int steps, int32_t* __restrict__ state_i,
                                                              float* __restrict__ p_word, int32_t* __restrict__ pair) {
  __shared__ int red[kPlanWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int mx = 0;
  for (int b = wv; b < B; b += kPlanWaves) {
    const int64_t* xr = x + (size_t)b * N;
    int cnt = 0;
    for (int c = lane; c < N; c += 64) cnt += xr[c] == mask_id;
    mx = max(mx, wave_sum_int(cnt));
  }
  if (lane == 0) red[wv] = mx;
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < kPlanWaves; ++w) mx = max(mx, red[w]);
  int i = max(*state_i, 0);
  float p_last = 0.f;
  if (mx > 0) {
    while (i < steps) {
      p_last = p_tab[i];
      ++i;
      const float scaled = (float)mx * p_last;
      if ((int)floorf(scaled) >= 1) break;
    }
  }
  *state_i = i;
  *p_word = p_last;
  pair[0] = i;
  pair[1] = mx > 0 ? 1 : 0;
}

__global__ void __launch_bounds__(kGenBlock) gen_acc_kernel(const int64_t* __restrict__ gen, const int64_t* __restrict__ labels,
                                                            const int64_t* __restrict__ ids, int N, int64_t mask_id,
                                                            int32_t* __restrict__ counts) {
  __shared__ int red[kGenWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t off = (size_t)b * N;
  int hit = 0, msk = 0;
  for (int c = tid; c < N; c += kGenBlock) {
    const bool m = ids[off + c] == mask_id;
    msk += m;
    hit += m && gen[off + c] == labels[off + c];
  }
  hit = block_sum_int(hit, red);
  msk = block_sum_int(msk, red);
  if (tid == 0) { counts[2 * b] = hit; counts[2 * b + 1] = msk; }
}

}  // namespace

extern "C" int gget_op_unmask_ranked(int64_t* x, const float* conf, const int64_t* cand, int B, int N, int mask_token_id, const float* p,
                                     int p_stride, int32_t* n_revealed, void* stream) {
  GGET_REQUIRE(B >= 0 && N >= 0, "unmask_ranked: B = %d, N = %d", B, N);
  GGET_REQUIRE(p_stride == 0 || p_stride == 1, "unmask_ranked: p_stride = %d (0: one p for the batch, 1: one per sample)", p_stride);
  GGET_REQUIRE(x && conf && cand && p, "unmask_ranked: null argument");
  if (B == 0) return 0;
  hipLaunchKernelGGL(unmask_ranked_kernel, dim3(B), dim3(kGenBlock), 0, (hipStream_t)stream, x, conf, cand, N, (int64_t)mask_token_id, p,
                     p_stride, n_revealed);
  GGET_LAUNCH_CHECK();
  return 0;
}

extern "C" int gget_op_gen_plan(const int64_t* x, int B, int N, int mask_token_id, const float* p_tab, int steps, int32_t* state_i,
                                float* p_word, int32_t* host_pair, void* stream) {
  GGET_REQUIRE(B >= 0 && N >= 0 && steps >= 0, "gen_plan: B = %d, N = %d, steps = %d", B, N, steps);
  GGET_REQUIRE(x && state_i && p_word && host_pair && (p_tab || steps == 0), "gen_plan: null argument");
  void* pair_dev = nullptr;
  if (hipHostGetDevicePointer(&pair_dev, host_pair, 0) != hipSuccess || !pair_dev) {
    (void)hipGetLastError();
    gget_set_error("gen_plan: host_pair is not pinned host memory the device can write");
    return 2;
  }
  hipLaunchKernelGGL(gen_plan_kernel, dim3(1), dim3(kPlanBlock), 0, (hipStream_t)stream, x, B, N, (int64_t)mask_token_id, p_tab, steps,
                     state_i, p_word, (int32_t*)pair_dev);
  GGET_LAUNCH_CHECK();
  return 0;
}

extern "C" int gget_op_gen_acc(const int64_t* gen, const int64_t* labels, const int64_t* input_ids, int B, int N, int mask_token_id,
                               int32_t* counts, void* stream) {
  GGET_REQUIRE(B >= 0 && N >= 0, "gen_acc: B = %d, N = %d", B, N);
  GGET_REQUIRE(gen && labels && input_ids && counts, "gen_acc: null argument");
  if (B == 0) return 0;
  hipLaunchKernelGGL(gen_acc_kernel, dim3(B), dim3(kGenBlock), 0, (hipStream_t)stream, gen, labels, input_ids, N, (int64_t)mask_token_id,
                     counts);
  GGET_LAUNCH_CHECK();
  return 0;
}
