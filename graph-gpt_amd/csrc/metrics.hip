// Rank metrics of the multi-label evaluation pass: per-column ROC-AUC and average precision as EXACT pair counts.
// replaces: the host-side scikit-learn loops of the reference's evaluators (src/utils/ogb_utils.py:13-29 `_eval_rocauc`, OGB's `_eval_ap`
// behind :187-195) and torcheval's BinaryAUROC(num_tasks) inside MultiLabelClassificationMetrics.compute (src/utils/metrics_utils.py:112-114).
//
// For a positive i of column c, over the column's labelled entries:
//   a_i = negatives with score <  s_i,   e_i = negatives with score == s_i,   g_i = positives with score >= s_i
//   ROC-AUC = sum_i (2 a_i + e_i) / (2 n_pos n_neg)          (Mann-Whitney U, ties count one half)
//   AP      = sum_i g_i / (g_i + n_neg - a_i) / n_pos        (every positive of a tie group takes the precision at the END of its group)
// No sort: n_pos * n compare-and-adds per column on integer counters, so the counts are exact, independent of the launch geometry and
// identical from run to run; the only floating-point sum (the AP terms, fp64) runs over the positives in list order with a fixed tree.
//
// Five launches on the caller's stream:
//   rank_class_kernel   every (segment of kRankSeg rows, column): positives / negatives / bad entries of the segment
//   rank_scan_kernel    per column: exclusive scan of the segment counts (row order) -> list offsets; n_pos, n_neg, n_bad
//   rank_fill_kernel    STABLE compaction: column c's positive scores, then its negative scores, in row order, into list[c][0, n_pos + n_neg)
//                       (count then fill - no slot is handed out by an atomic: the list order is the order of the fp64 sum)
//   rank_count_kernel   grid (tiles of kRankTile positives, C): a lane keeps kRankPer positives in registers; the negative list, then the
//                       positive list, streams through LDS in chunks of kRankChunk floats; all lanes read the same LDS address (broadcast)
//   rank_finish_kernel  per column: sum (2 a + e) in uint64 and the AP terms in fp64
#include <float.h>
#include <math.h>

#include "common.h"
#include "../../include/gget.h"

namespace {

constexpr int kRankBlock = 256;                      // threads of every launch below (4 waves)
constexpr int kRankSeg = 64;                         // rows one thread classifies (a segment); a block = 4 segments x 64 columns
constexpr int kRankPer = 4;                          // positives a lane keeps in registers
constexpr int kRankTile = kRankBlock * kRankPer;     // positives per workgroup of rank_count_kernel
constexpr int kRankChunk = 1024;                     // floats of one LDS chunk (4 KiB): 16 K compare-and-adds per lane between barriers
constexpr int kRankMaxCols = 65535;                  // grid.y

enum { kUnlabelled = 0, kPositive = 1, kNegative = 2, kBad = 3 };

// NaN label = unlabelled (the score is then never looked at); otherwise the label must be 0 or 1 and the score finite
__device__ __forceinline__ int rank_class(float s, float y) {
  if (y != y) return kUnlabelled;
  if (!(fabsf(s) <= FLT_MAX)) return kBad;
  return y == 1.f ? kPositive : y == 0.f ? kNegative : kBad;
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// seg_* are [C][nseg]: the scan reads them coalesced
__global__ void __launch_bounds__(kRankBlock) rank_class_kernel(const float* __restrict__ scores, int ld_s, const float* __restrict__ labels,
                                                                int ld_y, int n, int C, int nseg, int32_t* __restrict__ seg_pos,
                                                                int32_t* __restrict__ seg_neg, int32_t* __restrict__ seg_bad) {
  const int c = blockIdx.y * 64 + (threadIdx.x & 63);
  const int seg = blockIdx.x * (kRankBlock / 64) + (threadIdx.x >> 6);
  if (c >= C || seg >= nseg) return;
  const int r0 = seg * kRankSeg, r1 = min(n, r0 + kRankSeg);
  int np = 0, nn = 0, nb = 0;
  for (int r = r0; r < r1; ++r) {
    const int k = rank_class(scores[(size_t)r * ld_s + c], labels[(size_t)r * ld_y + c]);
    np += k == kPositive;
    nn += k == kNegative;
    nb += k == kBad;
  }
  const size_t o = (size_t)c * nseg + seg;
  seg_pos[o] = np;
  seg_neg[o] = nn;
  seg_bad[o] = nb;
}

// one wave per column; seg_pos / seg_neg become exclusive offsets in place
__global__ void __launch_bounds__(64) rank_scan_kernel(int32_t* __restrict__ seg_pos, int32_t* __restrict__ seg_neg,
                                                       const int32_t* __restrict__ seg_bad, int nseg, int64_t* __restrict__ n_pos,
                                                       int64_t* __restrict__ n_neg, int32_t* __restrict__ n_bad) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const size_t base = (size_t)c * nseg;
  int cp = 0, cn = 0, cb = 0;     // carries (wave-uniform)
  for (int s0 = 0; s0 < nseg; s0 += 64) {
    const int s = s0 + lane;
    const int p = s < nseg ? seg_pos[base + s] : 0, q = s < nseg ? seg_neg[base + s] : 0, b = s < nseg ? seg_bad[base + s] : 0;
    const int ip = wave_incl_scan(p, lane), iq = wave_incl_scan(q, lane), ib = wave_incl_scan(b, lane);
    if (s < nseg) {
      seg_pos[base + s] = cp + ip - p;
      seg_neg[base + s] = cn + iq - q;
    }
    cp += __shfl(ip, 63, 64);
    cn += __shfl(iq, 63, 64);
    cb += __shfl(ib, 63, 64);
  }
  if (lane == 0) {
    n_pos[c] = cp;
    n_neg[c] = cn;
    n_bad[c] = cb;
  }
}

// list is [C][n]: positives of column c at [0, n_pos), its negatives at [n_pos, n_pos + n_neg), both in row order
__global__ void __launch_bounds__(kRankBlock) rank_fill_kernel(const float* __restrict__ scores, int ld_s, const float* __restrict__ labels,
                                                               int ld_y, int n, int C, int nseg, const int32_t* __restrict__ seg_pos,
                                                               const int32_t* __restrict__ seg_neg, const int64_t* __restrict__ n_pos,
                                                               float* __restrict__ list) {
  const int c = blockIdx.y * 64 + (threadIdx.x & 63);
  const int seg = blockIdx.x * (kRankBlock / 64) + (threadIdx.x >> 6);
  if (c >= C || seg >= nseg) return;
  const int r0 = seg * kRankSeg, r1 = min(n, r0 + kRankSeg);
  const size_t o = (size_t)c * nseg + seg;
  float* col = list + (size_t)c * n;
  int ip = seg_pos[o], in = (int)n_pos[c] + seg_neg[o];
  for (int r = r0; r < r1; ++r) {
    const float s = scores[(size_t)r * ld_s + c];
    const int k = rank_class(s, labels[(size_t)r * ld_y + c]);
    if (k == kPositive) col[ip++] = s;          // (ip < n_pos <= n and in < n_pos + n_neg <= n by the scan of the same classification)
    else if (k == kNegative) col[in++] = s;
  }
}

// One chunked pass of `m` list entries against the lane's positives.  kNeg: lt += v < s, le += v <= s; otherwise ge += v >= s.
// The chunk's tail is padded to a multiple of 4 with +inf (negatives) / -inf (positives): the lists hold finite scores only, so a pad
// entry satisfies none of the three comparisons.
template <bool kNeg>
__device__ __forceinline__ void rank_stream(const float* __restrict__ src, int m, const float (&s)[kRankPer], int (&c0)[kRankPer],
                                            int (&c1)[kRankPer], float* buf) {
  const float pad = kNeg ? INFINITY : -INFINITY;
  for (int base = 0; base < m; base += kRankChunk) {
    const int len = min(kRankChunk, m - base), len4 = (len + 3) & ~3;      // len4 <= kRankChunk (a multiple of 4)
    for (int k = threadIdx.x; k < len4; k += kRankBlock) buf[k] = k < len ? src[base + k] : pad;
    __syncthreads();
    for (int k = 0; k < len4; k += 4) {
      const float4 v = *reinterpret_cast<const float4*>(buf + k);       // the same address in every lane: an LDS broadcast
      const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int p = 0; p < kRankPer; ++p) {
          if (kNeg) {
            c0[p] += vv[j] < s[p];
            c1[p] += vv[j] <= s[p];
          } else {
            c0[p] += vv[j] >= s[p];
          }
        }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kRankBlock) rank_count_kernel(const float* __restrict__ list, int n, const int64_t* __restrict__ n_pos,
                                                                const int64_t* __restrict__ n_neg, int32_t* __restrict__ a_out,
                                                                int32_t* __restrict__ e_out, int32_t* __restrict__ g_out) {
  __shared__ __attribute__((aligned(16))) float buf[kRankChunk];
  const int c = blockIdx.y;
  const int np = (int)n_pos[c], nn = (int)n_neg[c];
  const int i0 = blockIdx.x * kRankTile;
  if (i0 >= np) return;                                  // (block-uniform: no barrier is skipped by part of a block)
  const float* pos = list + (size_t)c * n;
  const float* neg = pos + np;
  float s[kRankPer];
  int lt[kRankPer], le[kRankPer], ge[kRankPer];
#pragma unroll
  for (int p = 0; p < kRankPer; ++p) {
    const int i = i0 + p * kRankBlock + threadIdx.x;
    s[p] = i < np ? pos[i] : 0.f;
    lt[p] = le[p] = ge[p] = 0;
  }
  rank_stream<true>(neg, nn, s, lt, le, buf);
  rank_stream<false>(pos, np, s, ge, ge, buf);
  const size_t o = (size_t)c * n;
#pragma unroll
  for (int p = 0; p < kRankPer; ++p) {
    const int i = i0 + p * kRankBlock + threadIdx.x;
    if (i < np) {
      a_out[o + i] = lt[p];
      e_out[o + i] = le[p] - lt[p];
      g_out[o + i] = ge[p];
    }
  }
}

// thread t adds the positives t, t + 256, ... in that order, then a fixed binary tree over the 256 partial sums
__global__ void __launch_bounds__(kRankBlock) rank_finish_kernel(const int32_t* __restrict__ a_in, const int32_t* __restrict__ e_in,
                                                                 const int32_t* __restrict__ g_in, int n, const int64_t* __restrict__ n_pos,
                                                                 const int64_t* __restrict__ n_neg, uint64_t* __restrict__ auc2,
                                                                 double* __restrict__ ap_sum) {
  __shared__ unsigned long long su[kRankBlock];
  __shared__ double sd[kRankBlock];
  const int c = blockIdx.x, t = threadIdx.x;
  const int np = (int)n_pos[c], nn = (int)n_neg[c];
  const size_t o = (size_t)c * n;
  unsigned long long u = 0;
  double d = 0.0;
  if (np > 0 && nn > 0)
    for (int i = t; i < np; i += kRankBlock) {
      const int a = a_in[o + i], e = e_in[o + i], g = g_in[o + i];
      u += 2ull * (unsigned long long)a + (unsigned long long)e;
      d += (double)g / ((double)g + (double)(nn - a));
    }
  su[t] = u;
  sd[t] = d;
  for (int w = kRankBlock / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w) {
      su[t] += su[t + w];
      sd[t] += sd[t + w];
    }
  }
  if (t == 0) {
    auc2[c] = su[0];
    ap_sum[c] = sd[0];
  }
}

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct RankLayout {
  size_t list, a, e, g, seg_pos, seg_neg, seg_bad, total;
  int nseg;
};

RankLayout rank_layout(int n, int C) {
  RankLayout L{};
  L.nseg = (n + kRankSeg - 1) / kRankSeg;
  const size_t cell = up256((size_t)n * C * 4), seg = up256((size_t)L.nseg * C * 4);
  size_t o = 0;
  L.list = o; o += cell;
  L.a = o; o += cell;
  L.e = o; o += cell;
  L.g = o; o += cell;
  L.seg_pos = o; o += seg;
  L.seg_neg = o; o += seg;
  L.seg_bad = o; o += seg;
  L.total = o;
  return L;
}

}  // namespace

extern "C" size_t gget_op_rank_metrics_workspace(int n, int C) {
  if (n <= 0 || C <= 0) return 0;
  return rank_layout(n, C).total;
}

extern "C" int gget_op_rank_metrics(const float* scores, int ld_s, const float* labels, int ld_y, int n, int C, int64_t* n_pos,
                                    int64_t* n_neg, uint64_t* auc2, double* ap_sum, int32_t* n_bad, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  GGET_REQUIRE(n >= 0 && C >= 0, "rank_metrics: n = %d, C = %d", n, C);
  if (n == 0 || C == 0) return 0;
  GGET_REQUIRE(C <= kRankMaxCols, "rank_metrics: C = %d > %d columns", C, kRankMaxCols);
  GGET_REQUIRE(ld_s >= C && ld_y >= C, "rank_metrics: row strides %d / %d below C = %d", ld_s, ld_y, C);
  GGET_REQUIRE(scores && labels && n_pos && n_neg && auc2 && ap_sum && n_bad, "rank_metrics: null argument");
  const RankLayout L = rank_layout(n, C);
  GGET_REQUIRE(workspace && workspace_bytes >= L.total, "rank_metrics: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : 0,
               L.total);
  GGET_REQUIRE(((uintptr_t)workspace & 15) == 0, "rank_metrics: workspace not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* list = (float*)(ws + L.list);
  int32_t *a = (int32_t*)(ws + L.a), *e = (int32_t*)(ws + L.e), *g = (int32_t*)(ws + L.g);
  int32_t *seg_pos = (int32_t*)(ws + L.seg_pos), *seg_neg = (int32_t*)(ws + L.seg_neg), *seg_bad = (int32_t*)(ws + L.seg_bad);
  const dim3 cells((L.nseg + kRankBlock / 64 - 1) / (kRankBlock / 64), (C + 63) / 64);
  hipLaunchKernelGGL(rank_class_kernel, cells, dim3(kRankBlock), 0, st, scores, ld_s, labels, ld_y, n, C, L.nseg, seg_pos, seg_neg, seg_bad);
  GGET_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_scan_kernel, dim3(C), dim3(64), 0, st, seg_pos, seg_neg, seg_bad, L.nseg, n_pos, n_neg, n_bad);
  GGET_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_fill_kernel, cells, dim3(kRankBlock), 0, st, scores, ld_s, labels, ld_y, n, C, L.nseg, seg_pos, seg_neg, n_pos, list);
  GGET_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_count_kernel, dim3((n + kRankTile - 1) / kRankTile, C), dim3(kRankBlock), 0, st, list, n, n_pos, n_neg, a, e, g);
  GGET_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_finish_kernel, dim3(C), dim3(kRankBlock), 0, st, a, e, g, n, n_pos, n_neg, auc2, ap_sum);
  GGET_LAUNCH_CHECK();
  return 0;
}
