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
#include "kernels.h"
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

// ------------------------------------------------------------------------------------------------ link prediction: Hits@K and MRR
// replaces: OGB's link evaluators on the tensors the reference's metric object keeps on the device (src/utils/metrics_utils.py:38-73):
// `_reformat_pred_for_hr_eval` + `_eval_hits` (src/utils/ogb_utils.py:141-152 behind :82-90 ogbl-ppa, :131-138 ogbl-ddi: torch.topk of the
// negatives, then compare-and-sum) and `_reformat_pred_for_mrr_eval` + `_eval_mrr` (:155-170 behind :92-128 ogbl-citation2 / ogbl-wikikg2:
// torch.sort by idx, mask, reshape, two compare-and-sums per row).  Integer counters only; the one fp64 sum has a fixed order.
constexpr int kLinkBlock = 256;        // threads of the streaming launches (4 waves)
constexpr int kLinkVec = 4;            // entries per lane and grid-stride round on the aligned body: one 16-byte score load, two label loads
constexpr int kLinkGrid = 1024;        // workgroups at most (4 per CU of a 256-CU chip; menu key 18 overrides): the rest is grid-stride
constexpr int kLinkBins = 256;         // 8-bit digits, most significant first: four passes over the 32-bit key
constexpr int kLinkSeg = 256;          // entries of one partition segment of the MRR path: a wave, 4 consecutive entries per lane
constexpr int kLinkWaves = kLinkBlock / 64;

struct LinkHitsState {                 // device words between the passes (zeroed together with the histograms)
  int n_pos, n_neg, n_bad;
  int none;                            // fewer than K negatives: kth = -inf, the later passes return at once
  unsigned prefix;                     // the digits chosen so far
  int krem;                            // the K-th largest of the whole list is the krem-th largest among the entries matching prefix
  int pad[2];
};

__device__ __forceinline__ int link_class(float s, long long y) {
  if (!(fabsf(s) <= FLT_MAX)) return kBad;
  return y == 1 ? kPositive : y == 0 ? kNegative : kBad;
}

// order-preserving key of a finite fp32: -0.0 becomes +0.0, then negative numbers have all bits flipped, the others the sign bit
__device__ __forceinline__ unsigned link_key(float s) {
  unsigned b = __float_as_uint(s);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float link_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// f(score, label) once for every entry of [0, n): 16-byte loads on the body that starts at the first 16-byte aligned score (when the
// labels are 16-byte aligned there, too), single loads for the at most 3 + 3 entries in front of and behind it, or for everything
template <typename F>
__device__ __forceinline__ void link_for_each(const float* __restrict__ scores, const long long* __restrict__ labels, int n, F f) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nt = (long)gridDim.x * blockDim.x;
  const int head = min(n, (int)(((16u - (unsigned)((uintptr_t)scores & 15u)) & 15u) >> 2));
  if (((uintptr_t)(labels + head) & 15u) != 0) {
    for (long i = tid; i < n; i += nt) f(scores[i], labels[i]);
    return;
  }
  const int nvec = (n - head) / kLinkVec, rest = head + nvec * kLinkVec;
  const float4* s4 = reinterpret_cast<const float4*>(scores + head);
  const longlong2* y2 = reinterpret_cast<const longlong2*>(labels + head);
  for (long v = tid; v < nvec; v += nt) {
    const float4 s = s4[v];
    const longlong2 a = y2[2 * v], b = y2[2 * v + 1];
    f(s.x, a.x);
    f(s.y, a.y);
    f(s.z, b.x);
    f(s.w, b.y);
  }
  if (tid < head) f(scores[tid], labels[tid]);                                      // (the grid holds at least 64 threads)
  else if (tid - head < n - rest) f(scores[rest + tid - head], labels[rest + tid - head]);
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// pass `kPass` of the radix select: histogram of digit kPass of the negatives whose higher digits equal st->prefix; pass 0 classifies, too
template <int kPass>
__global__ void __launch_bounds__(kLinkBlock) link_hist_kernel(const float* __restrict__ scores, const long long* __restrict__ labels, int n,
                                                               LinkHitsState* __restrict__ st, unsigned* __restrict__ hist) {
  __shared__ unsigned bins[kLinkBins];
  unsigned prefix = 0;
  if (kPass > 0) {
    if (st->none) return;                       // (uniform over the grid)
    prefix = st->prefix;
  }
  for (int b = threadIdx.x; b < kLinkBins; b += kLinkBlock) bins[b] = 0;
  __syncthreads();
  int np = 0, nn = 0, nb = 0;
  link_for_each(scores, labels, n, [&](float s, long long y) {
    const int k = link_class(s, y);
    if (kPass == 0) {
      np += k == kPositive;
      nn += k == kNegative;
      nb += k == kBad;
    }
    if (k == kNegative) {
      const unsigned key = link_key(s);
      if (kPass == 0 || (key >> (32 - 8 * kPass)) == prefix) atomicAdd(&bins[(key >> (24 - 8 * kPass)) & 255u], 1u);
    }
  });
  if (kPass == 0) {
    np = wave_sum_int(np);
    nn = wave_sum_int(nn);
    nb = wave_sum_int(nb);
    if ((threadIdx.x & 63) == 0) {
      if (np) atomicAdd(&st->n_pos, np);
      if (nn) atomicAdd(&st->n_neg, nn);
      if (nb) atomicAdd(&st->n_bad, nb);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kLinkBins; b += kLinkBlock)
    if (bins[b]) atomicAdd(&hist[b], bins[b]);
}

// one wave: lane l owns the bins 255 - 4 l ... 252 - 4 l; walking from the top, the digit whose bin holds the krem-th entry extends the
// prefix.  The last pass writes the outputs (hits = 0: link_hits_count_kernel adds to it).
__global__ void __launch_bounds__(64) link_select_kernel(LinkHitsState* __restrict__ st, const unsigned* __restrict__ hist, int pass,
                                                         long long K, long long* __restrict__ n_pos, long long* __restrict__ n_neg,
                                                         float* __restrict__ kth, long long* __restrict__ hits, int* __restrict__ n_bad) {
  const int lane = threadIdx.x;
  const int none = pass == 0 ? (K > (long long)st->n_neg) : st->none;
  const int krem = pass == 0 ? (none ? 0 : (int)K) : st->krem;
  unsigned prefix = pass == 0 ? 0u : st->prefix;
  if (!none) {
    int h[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      h[j] = (int)hist[255 - 4 * lane - j];
      sum += h[j];
    }
    const int incl = wave_incl_scan(sum, lane);
    int acc = incl - sum, digit = 0, left = 0;
    const bool mine = acc < krem && krem <= incl;          // true in exactly one lane: the bins hold at least krem entries
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (mine && left == 0 && krem <= acc + h[j]) {
        digit = 255 - 4 * lane - j;
        left = krem - acc;                                   // >= 1
      }
      acc += h[j];
    }
    const unsigned long long who = __ballot(mine);
    const int src = who ? __ffsll((long long)who) - 1 : 0;
    digit = __shfl(digit, src, 64);
    left = __shfl(left, src, 64);
    prefix = (prefix << 8) | (unsigned)digit;
    if (lane == 0) {
      st->prefix = prefix;
      st->krem = left;
    }
  }
  if (lane == 0) {
    if (pass == 0) st->none = none;
    if (pass == 3) {
      *n_pos = st->n_pos;
      *n_neg = st->n_neg;
      *n_bad = st->n_bad;
      *kth = none ? -INFINITY : link_unkey(prefix);
      *hits = 0;
    }
  }
}

// positives scored above kth (a float comparison: -0.0 == +0.0); every finite score is above -inf
__global__ void __launch_bounds__(kLinkBlock) link_hits_count_kernel(const float* __restrict__ scores, const long long* __restrict__ labels,
                                                                     int n, const float* __restrict__ kth, unsigned long long* __restrict__ hits) {
  const float t = *kth;
  int c = 0;
  link_for_each(scores, labels, n, [&](float s, long long y) { c += link_class(s, y) == kPositive && s > t; });
  c = wave_sum_int(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(hits, (unsigned long long)c);
}

// ---- MRR
enum { kMrrBadIdx = 0, kMrrBadEntry = 1, kMrrWords = 16 };       // words of the counter block behind the class marks

// "sort by idx" as a scatter: entry i goes to slot idx[i].  The slot's mark (0 = empty) is claimed with a compare-and-swap and holds the
// entry's class + 1 afterwards; a slot that is already claimed, or an index outside [0, n), is counted.
__global__ void __launch_bounds__(kLinkBlock) mrr_scatter_kernel(const float* __restrict__ scores, const long long* __restrict__ labels,
                                                                 const long long* __restrict__ idx, int n, float* __restrict__ sorted,
                                                                 unsigned* __restrict__ mark, int* __restrict__ counters) {
  const long nt = (long)gridDim.x * blockDim.x;
  int bad = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nt) {
    const long long j = idx[i];
    if (j < 0 || j >= n) {
      ++bad;
      continue;
    }
    const float s = scores[i];
    if (atomicCAS(&mark[j], 0u, (unsigned)link_class(s, labels[i]) + 1u) != 0u) ++bad;
    else sorted[j] = s;
  }
  bad = wave_sum_int(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&counters[kMrrBadIdx], bad);
}

// a wave per segment of kLinkSeg slots, lane l the slots 4 l ... 4 l + 3 of it (one 16-byte load; the mark array is 16-byte aligned and
// padded to whole segments with empty marks)
__device__ __forceinline__ void mrr_segment_marks(const unsigned* __restrict__ mark, long seg, int lane, int (&k)[4]) {
  const uint4 m = reinterpret_cast<const uint4*>(mark)[seg * (kLinkSeg / 4) + lane];
  k[0] = (int)m.x - 1;
  k[1] = (int)m.y - 1;
  k[2] = (int)m.z - 1;
  k[3] = (int)m.w - 1;
}

__global__ void __launch_bounds__(kLinkBlock) mrr_class_kernel(const unsigned* __restrict__ mark, int nseg, int32_t* __restrict__ seg_pos,
                                                               int32_t* __restrict__ seg_neg, int32_t* __restrict__ seg_bad) {
  const int lane = threadIdx.x & 63;
  for (long seg = (long)blockIdx.x * kLinkWaves + (threadIdx.x >> 6); seg < nseg; seg += (long)gridDim.x * kLinkWaves) {
    int k[4], np = 0, nn = 0, nb = 0;
    mrr_segment_marks(mark, seg, lane, k);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      np += k[j] == kPositive;
      nn += k[j] == kNegative;
      nb += k[j] == kBad;
    }
    np = wave_sum_int(np);
    nn = wave_sum_int(nn);
    nb = wave_sum_int(nb);
    if (lane == 0) {
      seg_pos[seg] = np;
      seg_neg[seg] = nn;
      seg_bad[seg] = nb;
    }
  }
}

// STABLE partition in slot (= idx) order: positives to list[0, n_pos), negatives to list[n_pos, n_pos + n_neg); the offsets come from
// rank_scan_kernel over the segment counts and a wave scan inside the segment - no slot is handed out by an atomic
__global__ void __launch_bounds__(kLinkBlock) mrr_fill_kernel(const float* __restrict__ sorted, const unsigned* __restrict__ mark, int n,
                                                              int nseg, const int32_t* __restrict__ seg_pos, const int32_t* __restrict__ seg_neg,
                                                              const int64_t* __restrict__ n_pos, float* __restrict__ list) {
  const int lane = threadIdx.x & 63;
  const int np_all = (int)*n_pos;
  for (long seg = (long)blockIdx.x * kLinkWaves + (threadIdx.x >> 6); seg < nseg; seg += (long)gridDim.x * kLinkWaves) {
    int k[4], np = 0, nn = 0;
    mrr_segment_marks(mark, seg, lane, k);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      np += k[j] == kPositive;
      nn += k[j] == kNegative;
    }
    int ip = seg_pos[seg] + wave_incl_scan(np, lane) - np;
    int in = np_all + seg_neg[seg] + wave_incl_scan(nn, lane) - nn;
    const long s0 = seg * kLinkSeg + 4 * lane;
#pragma unroll
    for (int j = 0; j < 4; ++j) {       // (a marked slot lies below n; ip < n_pos and in < n_pos + n_neg <= n by the scan of the same marks)
      if (k[j] == kPositive) list[ip++] = sorted[s0 + j];
      else if (k[j] == kNegative) list[in++] = sorted[s0 + j];
    }
  }
}

// every index valid and distinct, every entry well-formed, and cnt_neg negatives per positive: then n_pos = P and the rows exist
__device__ __forceinline__ bool mrr_ok(const int* counters, const int32_t* bad_entries, long long np, long long nn, int P, int cnt_neg) {
  return counters[kMrrBadIdx] == 0 && *bad_entries == 0 && np == P && nn == (long long)P * cnt_neg;
}

// a wave per row: lane l takes the columns l, l + 64, ...; with two groups the even columns are group 0 and the odd ones group 1, which
// is the lane's parity (the stride is even), so the reduction leaves out the exchange between neighbouring lanes
__global__ void __launch_bounds__(kLinkBlock) mrr_row_kernel(const float* __restrict__ list, const int* __restrict__ counters,
                                                             const int32_t* __restrict__ bad_entries, const int64_t* __restrict__ n_pos,
                                                             const int64_t* __restrict__ n_neg, int P, int cnt_neg, int groups,
                                                             int32_t* __restrict__ optimistic, int32_t* __restrict__ pessimistic) {
  if (!mrr_ok(counters, bad_entries, *n_pos, *n_neg, P, cnt_neg)) return;
  const int lane = threadIdx.x & 63;
  const float* neg = list + P;
  for (long r = (long)blockIdx.x * kLinkWaves + (threadIdx.x >> 6); r < P; r += (long)gridDim.x * kLinkWaves) {
    const float p = list[r];
    const float* row = neg + (size_t)r * cnt_neg;
    int gt = 0, ge = 0;
    for (int c = lane; c < cnt_neg; c += 64) {
      const float v = row[c];
      gt += v > p;
      ge += v >= p;
    }
    for (int o = 32; o >= groups; o >>= 1) {
      gt += __shfl_xor(gt, o, 64);
      ge += __shfl_xor(ge, o, 64);
    }
    if (lane < groups) {
      optimistic[(size_t)lane * P + r] = gt;
      pessimistic[(size_t)lane * P + r] = ge;
    }
  }
}

// rank = (optimistic + pessimistic) / 2 + 1 over the groups * P entries in list order: thread t adds the entries t, t + 256, ..., then
// a fixed binary tree (as rank_finish_kernel); rank <= 1 / 3 / 10 are integer tests of optimistic + pessimistic
__global__ void __launch_bounds__(kLinkBlock) mrr_finish_kernel(const int32_t* __restrict__ optimistic, const int32_t* __restrict__ pessimistic,
                                                                const int* __restrict__ counters, const int32_t* __restrict__ bad_entries,
                                                                const int64_t* __restrict__ n_pos, const int64_t* __restrict__ n_neg, int P,
                                                                int cnt_neg, int groups, int64_t* __restrict__ hits, double* __restrict__ mrr_sum,
                                                                int32_t* __restrict__ n_bad) {
  __shared__ int sh[3][kLinkBlock];
  __shared__ double sd[kLinkBlock];
  const int t = threadIdx.x;
  const bool ok = mrr_ok(counters, bad_entries, *n_pos, *n_neg, P, cnt_neg);
  int h1 = 0, h3 = 0, h10 = 0;
  double d = 0.0;
  if (ok)
    for (long i = t; i < (long)groups * P; i += kLinkBlock) {
      const int two = optimistic[i] + pessimistic[i];        // 2 (rank - 1)
      h1 += two <= 0;
      h3 += two <= 4;
      h10 += two <= 18;
      d += 1.0 / (0.5 * (double)two + 1.0);
    }
  sh[0][t] = h1;
  sh[1][t] = h3;
  sh[2][t] = h10;
  sd[t] = d;
  for (int w = kLinkBlock / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w) {
      sh[0][t] += sh[0][t + w];
      sh[1][t] += sh[1][t + w];
      sh[2][t] += sh[2][t + w];
      sd[t] += sd[t + w];
    }
  }
  if (t == 0) {
    hits[0] = sh[0][0];
    hits[1] = sh[1][0];
    hits[2] = sh[2][0];
    *mrr_sum = sd[0];
    n_bad[0] = counters[kMrrBadIdx];
    n_bad[1] = *bad_entries ? *bad_entries : (*n_neg != *n_pos * (int64_t)cnt_neg ? -1 : 0);
  }
}

struct MrrLayout {
  size_t list, sorted, mark, counters, seg_pos, seg_neg, seg_bad, total;
  int nseg;
};

MrrLayout mrr_layout(int n) {
  MrrLayout L{};
  L.nseg = (n + kLinkSeg - 1) / kLinkSeg;
  const size_t cell = up256((size_t)L.nseg * kLinkSeg * 4), seg = up256((size_t)L.nseg * 4);
  size_t o = 0;
  L.list = o; o += cell;
  L.sorted = o; o += cell;
  L.mark = o; o += cell;                       // (mark and counters are zeroed by one memset)
  L.counters = o; o += up256(kMrrWords * 4);
  L.seg_pos = o; o += seg;
  L.seg_neg = o; o += seg;
  L.seg_bad = o; o += seg;
  L.total = o;
  return L;
}

constexpr size_t kHitsHistBytes = 4 * kLinkBins * sizeof(unsigned);
constexpr size_t kHitsBytes = kHitsHistBytes + 256;

inline int link_grid(long units) {                // workgroups for `units` workgroup-rounds of work
  const int cap = menu().link_grid > 0 ? menu().link_grid : kLinkGrid;
  return (int)(units < 1 ? 1 : units > cap ? cap : units);
}

// ------------------------------------------------------------------------------------------------ graph clustering: token-level heads
// replaces: GraphClusteringMetrics.update (src/utils/metrics_utils.py:231-295: torch.argmax, two .nonzero() per sample) and
// `get_acc_per_graph` (:340-348: per distinct label and per distinct prediction one .nonzero(), one .unique() and one len(...) - a
// device-to-host synchronisation each, inside a Python loop over the samples).  As counts: over the kept positions of a sample (selected:
// raw_node_idx != -100; kept: selected and label != -100), recall = t_r / n_r with n_r = distinct labels and t_r = those whose positions
// all carry one prediction; precision = t_p / n_p with the roles swapped.  No sort and no ordered atomic: four int32 tables of C entries
// in LDS - per label value the min and max prediction seen, per prediction value the min and max label seen - filled with LDS integer
// min / max atomics; a value is present when its max was written, its group uniform when min == max.  Every output is an exact integer,
// independent of lane order and launch geometry.
//
// One launch, one workgroup per sample (grid-stride over samples).  The arg-max (first index of the maximum, a NaN is maximal and the
// first NaN wins, -0.0 ties +0.0) has two lane mappings:
//   C <= kClusterStageC  the sample's logits are one contiguous run of S * C floats: tiles of whole rows (at most kClusterTile floats)
//                        are copied to LDS with adjacent lanes on adjacent addresses - 16-byte loads on the tile's 16-byte aligned body,
//                        the LDS image shifted by the pointer's misalignment so that the 16-byte LDS stores are aligned too - then a
//                        lane scans one row out of LDS.  For an even C lane t starts its row at column t % C and wraps, which spreads the
//                        lanes of a bank group over the banks (row stride C dwords); the comparison carries the column, so the order of
//                        the scan does not matter.
//   C >  kClusterStageC  a wave per row, lane l the columns l, l + 64, ... straight from global memory, then a wave reduction.
constexpr int kClusterBlock = 256;
constexpr int kClusterWaves = kClusterBlock / 64;
constexpr int kClusterTile = 4096;       // floats of one LDS tile (16 KiB): 64 rows at C = 64, 512 at C = 8
constexpr int kClusterStageC = 64;
constexpr long long kClusterIgnore = -100;

// the arg-max order: does (v, j) go in front of (best, bj)?
__device__ __forceinline__ bool cluster_gt(float v, float best) { return v > best || (v != v && best == best); }
__device__ __forceinline__ bool cluster_before(float v, int j, float best, int bj) {
  return cluster_gt(v, best) || (!cluster_gt(best, v) && j < bj);
}

struct ClusterTables {
  int *lab_min, *lab_max, *prd_min, *prd_max;
};

// one position with its prediction: totals in registers, the four tables through LDS atomics
__device__ __forceinline__ void cluster_visit(long long pred, long long lab, long long raw, int C, bool check_pred, const ClusterTables& T,
                                              int (&tot)[4]) {
  if (raw == kClusterIgnore) return;
  const bool labelled = lab != kClusterIgnore;
  if ((labelled && (lab < 0 || lab >= C)) || (check_pred && (pred < 0 || pred >= C))) {
    ++tot[3];
    return;
  }
  ++tot[2];
  if (!labelled) return;
  ++tot[1];
  tot[0] += pred == lab;
  const int p = (int)pred, y = (int)lab;       // both inside [0, C): the table indices are in bounds
  atomicMin(&T.lab_min[y], p);
  atomicMax(&T.lab_max[y], p);
  atomicMin(&T.prd_min[p], y);
  atomicMax(&T.prd_max[p], y);
}

__global__ void __launch_bounds__(kClusterBlock) cluster_kernel(const void* __restrict__ pred_or_logits, int is_logits,
                                                                const long long* __restrict__ labels, const long long* __restrict__ raw_node_idx,
                                                                int B, int S, int C, long long* __restrict__ y_pred,
                                                                int32_t* __restrict__ counts, unsigned long long* __restrict__ totals) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cluster_smem[];
  float* tile = reinterpret_cast<float*>(cluster_smem);                         // kClusterTile + 4 floats
  int* cnt = reinterpret_cast<int*>(cluster_smem) + kClusterTile + 4;           // t_r, n_r, t_p, n_p of the sample
  int* blk = cnt + 4;                                                           // the workgroup's share of the four totals
  ClusterTables T;
  T.lab_min = blk + 4;
  T.lab_max = T.lab_min + C;
  T.prd_min = T.lab_max + C;
  T.prd_max = T.prd_min + C;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int tot[4] = {0, 0, 0, 0};                                                    // n_correct, n_kept, n_selected, n_bad of this thread
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const size_t row0 = (size_t)b * S;
    const long long* lab_b = labels + row0;
    const long long* raw_b = raw_node_idx + row0;
    long long* out_b = y_pred + row0;
    for (int c = t; c < C; c += kClusterBlock) {
      T.lab_min[c] = T.prd_min[c] = 0x7fffffff;
      T.lab_max[c] = T.prd_max[c] = -1;
    }
    if (t < 4) cnt[t] = 0;          // (thread t read cnt[t] of the previous sample itself: program order)
    __syncthreads();
    if (!is_logits) {
      const long long* pr = reinterpret_cast<const long long*>(pred_or_logits) + row0;
      for (int s = t; s < S; s += kClusterBlock) {
        const long long p = pr[s];
        out_b[s] = p;
        cluster_visit(p, lab_b[s], raw_b[s], C, true, T, tot);
      }
    } else if (C <= kClusterStageC) {
      const float* lg = reinterpret_cast<const float*>(pred_or_logits) + row0 * C;
      const int rows_per_tile = kClusterTile / C;                              // >= 64
      for (int r0 = 0; r0 < S; r0 += rows_per_tile) {
        const int nrows = min(rows_per_tile, S - r0), n = nrows * C;           // n <= kClusterTile floats at g[0, n)
        const float* g = lg + (size_t)r0 * C;
        const int pad = (int)(((uintptr_t)g >> 2) & 3u);                       // g + head is 16-byte aligned, and so is img + head
        const int head = min(n, (4 - pad) & 3);
        const int nvec = (n - head) >> 2, rest = head + 4 * nvec;
        float* img = tile + pad;                                                // img[0, n): the last index is pad + n - 1 <= kClusterTile + 2
        const float4* g4 = reinterpret_cast<const float4*>(g + head);
        long long lab0 = 0, raw0 = kClusterIgnore;                              // the lane's first row of the tile: asked for with the logits
        if (t < nrows) {
          lab0 = lab_b[r0 + t];
          raw0 = raw_b[r0 + t];
        }
        for (int v = t; v < nvec; v += kClusterBlock) *reinterpret_cast<float4*>(img + head + 4 * v) = g4[v];
        if (t < head) img[t] = g[t];
        else if (t - head < n - rest) img[rest + t - head] = g[rest + t - head];
        __syncthreads();
        for (int r = t; r < nrows; r += kClusterBlock) {
          const float* row = img + r * C;
          int j = (C & 1) ? 0 : t % C;
          float best = row[j];
          int bj = j;
          for (int k = 1; k < C; ++k) {
            j = j + 1 == C ? 0 : j + 1;
            const float v = row[j];
            if (cluster_before(v, j, best, bj)) {
              best = v;
              bj = j;
            }
          }
          const int s = r0 + r;
          out_b[s] = bj;
          cluster_visit(bj, r == t ? lab0 : lab_b[s], r == t ? raw0 : raw_b[s], C, false, T, tot);
        }
        __syncthreads();                                                        // the tile is overwritten by the next round
      }
    } else {
      const float* lg = reinterpret_cast<const float*>(pred_or_logits) + row0 * C;
      for (int s = wave; s < S; s += kClusterWaves) {
        const float* row = lg + (size_t)s * C;
        float best = row[lane];                                                 // C > 64: every lane owns a column
        int bj = lane;
        for (int j = lane + 64; j < C; j += 64) {
          const float v = row[j];
          if (cluster_gt(v, best)) {                                            // (rising columns: a tie keeps the earlier one)
            best = v;
            bj = j;
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float v = __shfl_xor(best, o, 64);
          const int j = __shfl_xor(bj, o, 64);
          if (cluster_before(v, j, best, bj)) {
            best = v;
            bj = j;
          }
        }
        if (lane == 0) {
          out_b[s] = bj;
          cluster_visit(bj, lab_b[s], raw_b[s], C, false, T, tot);
        }
      }
    }
    __syncthreads();
    int c4[4] = {0, 0, 0, 0};
    for (int c = t; c < C; c += kClusterBlock) {
      const bool has_l = T.lab_max[c] >= 0, has_p = T.prd_max[c] >= 0;
      c4[0] += has_l && T.lab_min[c] == T.lab_max[c];
      c4[1] += has_l;
      c4[2] += has_p && T.prd_min[c] == T.prd_max[c];
      c4[3] += has_p;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c4[k] = wave_sum_int(c4[k]);
      if (lane == 0 && c4[k]) atomicAdd(&cnt[k], c4[k]);
    }
    __syncthreads();                                                            // every table read and every add to cnt lies behind
    if (t < 4) counts[(size_t)b * 4 + t] = cnt[t];
  }
  // one global atomic per workgroup and non-zero counter: every workgroup adds to the same four words, and adds to one address queue up
  if (t < 4) blk[t] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = wave_sum_int(tot[k]);      // a workgroup's share of one launch stays below 2^31 positions (B * S < 2^31 is required)
    if (lane == 0 && v) atomicAdd(&blk[k], v);
  }
  __syncthreads();
  if (t < 4 && blk[t]) atomicAdd(&totals[t], (unsigned long long)blk[t]);
}

inline size_t cluster_lds_bytes(int C) { return (size_t)(kClusterTile + 4 + 4 + 4) * 4 + (size_t)C * 16; }

// one workgroup per sample up to 8 per CU of a 256-CU chip (the work of a sample is a chain of dependent round trips: residency hides
// it); menu key 18 sets another cap, as for the link metrics
inline int cluster_grid(int B) {
  const int cap = menu().link_grid > 0 ? menu().link_grid : 2048;
  return B < 1 ? 1 : B > cap ? cap : B;
}

}  // namespace

extern "C" int gget_op_cluster_metrics(const void* pred_or_logits, int is_logits, const int64_t* labels, const int64_t* raw_node_idx, int B,
                                       int S, int C, int64_t* y_pred, int32_t* counts, int64_t* totals, void* stream) {
  GGET_REQUIRE(B >= 0 && S >= 0 && C >= 1, "cluster_metrics: B = %d, S = %d, C = %d", B, S, C);
  GGET_REQUIRE(C <= kClusterMaxC, "cluster_metrics: C = %d classes, above GGET_CLUSTER_MAX_C = %d (four int32 tables of C entries in LDS)",
               C, kClusterMaxC);
  GGET_REQUIRE((long long)B * S < (1ll << 31) && (long long)S * C < (1ll << 31), "cluster_metrics: B * S = %lld, S * C = %lld (both below 2^31)",
               (long long)B * S, (long long)S * C);
  if (B == 0 || S == 0) return 0;
  GGET_REQUIRE(pred_or_logits && labels && raw_node_idx && y_pred && counts && totals, "cluster_metrics: null argument");
  GGET_REQUIRE(((uintptr_t)pred_or_logits & (is_logits ? 3 : 7)) == 0 && ((uintptr_t)labels & 7) == 0 && ((uintptr_t)raw_node_idx & 7) == 0 &&
                   ((uintptr_t)y_pred & 7) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)totals & 7) == 0,
               "cluster_metrics: an argument is not aligned to its element size");
  hipLaunchKernelGGL(cluster_kernel, dim3(cluster_grid(B)), dim3(kClusterBlock), cluster_lds_bytes(C), (hipStream_t)stream, pred_or_logits,
                     is_logits ? 1 : 0, (const long long*)labels, (const long long*)raw_node_idx, B, S, C, (long long*)y_pred, counts,
                     (unsigned long long*)totals);
  GGET_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gget_op_link_hits_workspace(int n) { return n <= 0 ? 0 : kHitsBytes; }

extern "C" int gget_op_link_hits(const float* scores, const int64_t* labels, int n, int64_t K, int64_t* n_pos, int64_t* n_neg, float* kth,
                                 int64_t* hits, int32_t* n_bad, void* workspace, size_t workspace_bytes, void* stream) {
  GGET_REQUIRE(n >= 0, "link_hits: n = %d (the entry takes n < 2^31 entries)", n);
  GGET_REQUIRE(K >= 1, "link_hits: K = %lld", (long long)K);
  if (n == 0) return 0;
  GGET_REQUIRE(scores && labels && n_pos && n_neg && kth && hits && n_bad, "link_hits: null argument");
  GGET_REQUIRE(((uintptr_t)scores & 3) == 0 && ((uintptr_t)labels & 7) == 0, "link_hits: scores / labels not aligned to their element size");
  GGET_REQUIRE(workspace && workspace_bytes >= kHitsBytes, "link_hits: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : 0,
               kHitsBytes);
  GGET_REQUIRE(((uintptr_t)workspace & 15) == 0, "link_hits: workspace not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  unsigned* hist = (unsigned*)workspace;
  LinkHitsState* state = (LinkHitsState*)((char*)workspace + kHitsHistBytes);
  const long long* y = (const long long*)labels;
  GGET_HIP_CHECK(hipMemsetAsync(workspace, 0, kHitsBytes, st));
  const dim3 grid(link_grid(((long)n + kLinkBlock * kLinkVec - 1) / (kLinkBlock * kLinkVec))), block(kLinkBlock);
#define GGET_LINK_PASS(p)                                                                                                        \
  hipLaunchKernelGGL(link_hist_kernel<p>, grid, block, 0, st, scores, y, n, state, hist + p * kLinkBins);                        \
  GGET_LAUNCH_CHECK();                                                                                                           \
  hipLaunchKernelGGL(link_select_kernel, dim3(1), dim3(64), 0, st, state, hist + p * kLinkBins, p, (long long)K, (long long*)n_pos, \
                     (long long*)n_neg, kth, (long long*)hits, n_bad);                                                           \
  GGET_LAUNCH_CHECK()
  GGET_LINK_PASS(0);
  GGET_LINK_PASS(1);
  GGET_LINK_PASS(2);
  GGET_LINK_PASS(3);
#undef GGET_LINK_PASS
  hipLaunchKernelGGL(link_hits_count_kernel, grid, block, 0, st, scores, y, n, kth, (unsigned long long*)hits);
  GGET_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gget_op_link_mrr_workspace(int n) { return n <= 0 ? 0 : mrr_layout(n).total; }

extern "C" int gget_op_link_mrr(const float* scores, const int64_t* labels, const int64_t* idx, int n, int cnt_neg, int groups, int64_t* n_pos,
                                int64_t* n_neg, int32_t* optimistic, int32_t* pessimistic, int64_t* hits_1_3_10, double* mrr_sum, int32_t* n_bad,
                                void* workspace, size_t workspace_bytes, void* stream) {
  GGET_REQUIRE(n >= 0, "link_mrr: n = %d (the entry takes n < 2^31 entries)", n);
  GGET_REQUIRE(cnt_neg >= 1 && (groups == 1 || groups == 2), "link_mrr: cnt_neg = %d, groups = %d", cnt_neg, groups);
  GGET_REQUIRE(cnt_neg % groups == 0, "link_mrr: cnt_neg = %d is not a multiple of groups = %d", cnt_neg, groups);
  GGET_REQUIRE((long long)n % (1ll + cnt_neg) == 0, "link_mrr: n = %d is not a multiple of 1 + cnt_neg = %lld", n, 1ll + cnt_neg);
  if (n == 0) return 0;
  GGET_REQUIRE(scores && labels && idx && n_pos && n_neg && optimistic && pessimistic && hits_1_3_10 && mrr_sum && n_bad,
               "link_mrr: null argument");
  const MrrLayout L = mrr_layout(n);
  GGET_REQUIRE(workspace && workspace_bytes >= L.total, "link_mrr: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : 0, L.total);
  GGET_REQUIRE(((uintptr_t)workspace & 15) == 0, "link_mrr: workspace not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float *list = (float*)(ws + L.list), *sorted = (float*)(ws + L.sorted);
  unsigned* mark = (unsigned*)(ws + L.mark);
  int* counters = (int*)(ws + L.counters);
  int32_t *seg_pos = (int32_t*)(ws + L.seg_pos), *seg_neg = (int32_t*)(ws + L.seg_neg), *seg_bad = (int32_t*)(ws + L.seg_bad);
  int32_t* bad_entries = counters + kMrrBadEntry;
  const int P = (int)(n / (1ll + cnt_neg));
  const long long *y = (const long long*)labels, *ix = (const long long*)idx;
  GGET_HIP_CHECK(hipMemsetAsync(mark, 0, L.seg_pos - L.mark, st));
  const dim3 block(kLinkBlock), by_entry(link_grid(((long)n + kLinkBlock - 1) / kLinkBlock));
  const dim3 by_seg(link_grid(((long)L.nseg + kLinkWaves - 1) / kLinkWaves)), by_row(link_grid(((long)P + kLinkWaves - 1) / kLinkWaves));
  hipLaunchKernelGGL(mrr_scatter_kernel, by_entry, block, 0, st, scores, y, ix, n, sorted, mark, counters);
  GGET_LAUNCH_CHECK();
  hipLaunchKernelGGL(mrr_class_kernel, by_seg, block, 0, st, mark, L.nseg, seg_pos, seg_neg, seg_bad);
  GGET_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(64), 0, st, seg_pos, seg_neg, seg_bad, L.nseg, n_pos, n_neg, bad_entries);
  GGET_LAUNCH_CHECK();
  hipLaunchKernelGGL(mrr_fill_kernel, by_seg, block, 0, st, sorted, mark, n, L.nseg, seg_pos, seg_neg, n_pos, list);
  GGET_LAUNCH_CHECK();
  hipLaunchKernelGGL(mrr_row_kernel, by_row, block, 0, st, list, counters, bad_entries, n_pos, n_neg, P, cnt_neg, groups, optimistic, pessimistic);
  GGET_LAUNCH_CHECK();
  hipLaunchKernelGGL(mrr_finish_kernel, dim3(1), block, 0, st, optimistic, pessimistic, counters, bad_entries, n_pos, n_neg, P, cnt_neg, groups,
                     hits_1_3_10, mrr_sum, n_bad);
  GGET_LAUNCH_CHECK();
  return 0;
}

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
