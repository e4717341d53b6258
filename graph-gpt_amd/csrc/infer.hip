// Collection kernels of the prediction passes (reference src/utils/log_eval_dump_utils.py:41-74 ft_infer_hidden_states and
// src/utils/misc_utils.py:426-469 process_data): what the reference gathers batch by batch on the host (`.half()` per batch, a vstack
// at the end, `.cpu()` per batch) stays in device arenas, and the host copies once when the pass is over.  Conversions and integer
// compaction only: every result is exact and the same from run to run.
//
//   infer_append_kernel    one launch per batch: logits f32 -> fp16, hidden bf16 -> fp16 (widened to f32 exactly, rounded once) and the
//                          sample indices, each into its arena at row `row0`.  Rounding is the hardware's float -> half conversion in
//                          the default mode: nearest even, overflow to +-inf, fp16 subnormals produced, NaN stays NaN - tensor.half().
//   node_count_kernel      records, first launch: nodes (raw_node_idx != -100) per chunk of kRecChunk positions, and a copy of the cursor.
//   node_write_kernel      records, second launch: a chunk's first record sits at cursor + (nodes of the chunks before it); inside the
//                          chunk a ballot / popcount rank keeps the position order.  No atomic decides a place: the order is the
//                          ascending flat position whatever the scheduling.  The last chunk advances the cursor.
#include <map>
#include <mutex>
#include <utility>

#include "common.h"
#include "../../include/gget.h"

namespace {

constexpr int kAppendBlock = 256;
constexpr int kAppendMaxBlocks = 2048;
constexpr int kRecBlock = 256;
constexpr int kRecWaves = kRecBlock / 64;
constexpr int kRecRounds = 4;
constexpr int kRecChunk = kRecBlock * kRecRounds;                      // positions per workgroup
constexpr int64_t kRecMaxPos = (int64_t)GGET_NODE_RECORDS_MAX_POS;
constexpr int kRecMaxChunks = (int)(kRecMaxPos / kRecChunk);           // 1024: one chunk count per thread-quad of the prefix sum
constexpr size_t kRecWsBytes = 8 + sizeof(int32_t) * kRecMaxChunks;    // [cursor copy i64][chunk counts i32]

__device__ __forceinline__ unsigned short f2h_bits(float f) {
  const _Float16 h = (_Float16)f;
  return __builtin_bit_cast(unsigned short, h);
}

__device__ __forceinline__ unsigned pack2h(unsigned two_bf16) {
  const float lo = __uint_as_float(two_bf16 << 16), hi = __uint_as_float(two_bf16 & 0xffff0000u);
  return (unsigned)f2h_bits(lo) | ((unsigned)f2h_bits(hi) << 16);
}

__global__ void __launch_bounds__(kAppendBlock) infer_append_kernel(const float* __restrict__ logits, const uint4* __restrict__ hidden,
                                                                    const int64_t* __restrict__ idx, unsigned short* __restrict__ out_logits,
                                                                    uint4* __restrict__ out_hidden, int64_t* __restrict__ out_idx,
                                                                    int64_t n_logits, int64_t n_hidden8, int64_t n_idx) {
  const int64_t stride = (int64_t)gridDim.x * kAppendBlock;
  const int64_t t0 = (int64_t)blockIdx.x * kAppendBlock + threadIdx.x;
  for (int64_t i = t0; i < n_hidden8; i += stride) {                   // 8 values per thread: 16 bytes in, 16 bytes out
    const uint4 v = hidden[i];
    uint4 o;
    o.x = pack2h(v.x); o.y = pack2h(v.y); o.z = pack2h(v.z); o.w = pack2h(v.w);
    out_hidden[i] = o;
  }
  for (int64_t i = t0; i < n_logits; i += stride) out_logits[i] = f2h_bits(logits[i]);
  for (int64_t i = t0; i < n_idx; i += stride) out_idx[i] = idx[i];
}

__device__ __forceinline__ int rec_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the workgroup, returned to every thread; `red` (kRecWaves words of LDS) is free again on return
__device__ __forceinline__ int rec_block_sum(int v, int* red) {
  v = rec_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < kRecWaves; ++w) s += red[w];
  __syncthreads();
  return s;
}

__global__ void __launch_bounds__(kRecBlock) node_count_kernel(const int64_t* __restrict__ raw, int n_pos, const int64_t* __restrict__ state,
                                                               int64_t* __restrict__ ws_cursor, int32_t* __restrict__ ws_counts) {
  __shared__ int red[kRecWaves];
  const int base = blockIdx.x * kRecChunk;
  int cnt = 0;
#pragma unroll
  for (int r = 0; r < kRecRounds; ++r) {
    const int p = base + r * kRecBlock + threadIdx.x;
    cnt += (p < n_pos && raw[p] != -100) ? 1 : 0;
  }
  cnt = rec_block_sum(cnt, red);
  if (threadIdx.x == 0) {
    ws_counts[blockIdx.x] = cnt;
    if (blockIdx.x == 0) *ws_cursor = state[0];
  }
}

// torch.argmax over one row of C values: the first maximal class, a NaN counting as maximal (so the first NaN)
__device__ __forceinline__ int64_t argmax_row(const float* __restrict__ v, int C) {
  float best = v[0];
  int bi = 0;
  for (int c = 1; c < C; ++c) {
    const float x = v[c];
    if (!(best != best) && (x != x || x > best)) { best = x; bi = c; }
  }
  return (int64_t)bi;
}

__global__ void __launch_bounds__(kRecBlock) node_write_kernel(const float* __restrict__ logits, const int64_t* __restrict__ pred,
                                                               const int64_t* __restrict__ raw, const int64_t* __restrict__ idx,
                                                               int64_t* __restrict__ records, int64_t* __restrict__ state, int64_t cap,
                                                               int n_pos, int S, int C, const int64_t* __restrict__ ws_cursor,
                                                               const int32_t* __restrict__ ws_counts) {
  __shared__ int red[kRecWaves];
  __shared__ int wave_cnt[kRecRounds][kRecWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, blk = blockIdx.x;
  int before = 0;                                                      // nodes of the chunks in front of this one
  for (int k = tid; k < blk; k += kRecBlock) before += ws_counts[k];
  before = rec_block_sum(before, red);
  int64_t cursor = *ws_cursor;
  cursor = cursor < 0 ? 0 : (cursor > cap ? cap : cursor);

  int64_t raw_v[kRecRounds];
  unsigned long long bal[kRecRounds];
#pragma unroll
  for (int r = 0; r < kRecRounds; ++r) {
    const int p = blk * kRecChunk + r * kRecBlock + tid;
    raw_v[r] = p < n_pos ? raw[p] : (int64_t)-100;
    bal[r] = __ballot(raw_v[r] != -100);
    if (lane == 0) wave_cnt[r][wv] = __popcll(bal[r]);
  }
  __syncthreads();
  int running = 0;
#pragma unroll
  for (int r = 0; r < kRecRounds; ++r) {
    int in_front = running;
#pragma unroll
    for (int w = 0; w < kRecWaves; ++w) {
      const int t = wave_cnt[r][w];
      in_front += w < wv ? t : 0;
      running += t;
    }
    if (raw_v[r] == -100) continue;
    const int64_t slot = cursor + before + in_front + __popcll(bal[r] & ((1ull << lane) - 1ull));
    if (slot >= cap) continue;                                         // counted below, not written
    const int p = blk * kRecChunk + r * kRecBlock + tid;
    const int64_t y = logits ? argmax_row(logits + (size_t)p * C, C) : pred[p];
    int64_t* rec = records + slot * 3;
    rec[0] = idx[p / S];
    rec[1] = raw_v[r];
    rec[2] = y;
  }
  if (blk == (int)gridDim.x - 1 && tid == 0) {
    const int64_t total = (int64_t)before + running, room = cap - cursor;
    const int64_t written = total < room ? total : room;
    state[0] = cursor + written;
    state[1] += total - written;
  }
}

// scratch of the launch pair: one small buffer per (device, stream), so that calls on different streams never share one; allocated on
// first use and kept for the life of the process (4 KiB each)
void* records_workspace(hipStream_t stream) {
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, void*> table;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  void*& slot = table[std::make_pair(dev, stream)];
  if (!slot && hipMalloc(&slot, kRecWsBytes) != hipSuccess) {
    (void)hipGetLastError();
    slot = nullptr;
  }
  return slot;
}

}  // namespace

extern "C" int gget_op_infer_append(const float* logits, const void* hidden, const int64_t* idx, void* out_logits, void* out_hidden,
                                    int64_t* out_idx, int64_t row0, int64_t capacity, int B, int C, int d, void* stream) {
  GGET_REQUIRE(B >= 1 && C >= 1, "infer_append: empty shape (B = %d, C = %d)", B, C);
  GGET_REQUIRE(d >= 0 && d % 64 == 0, "infer_append: unsupported hidden width d = %d (a multiple of 64, or 0 without hidden states)", d);
  GGET_REQUIRE(logits && idx && out_logits && out_idx, "infer_append: null argument");
  GGET_REQUIRE((hidden != nullptr) == (out_hidden != nullptr), "infer_append: hidden and out_hidden go together (both, or both NULL)");
  GGET_REQUIRE(!hidden || d > 0, "infer_append: hidden states given with d = 0");
  GGET_REQUIRE(!hidden || (((uintptr_t)hidden | (uintptr_t)out_hidden) & 15u) == 0, "infer_append: hidden / out_hidden must be 16-byte aligned");
  GGET_REQUIRE(row0 >= 0 && capacity >= 0 && row0 <= capacity && (int64_t)B <= capacity - row0,
               "infer_append: rows %lld .. %lld do not fit an arena of %lld rows", (long long)row0, (long long)row0 + B - 1, (long long)capacity);
  const int64_t n_logits = (int64_t)B * C, n_hidden8 = hidden ? (int64_t)B * (d / 8) : 0;
  const int64_t work = n_logits > n_hidden8 ? n_logits : n_hidden8;
  int64_t blocks = (work + kAppendBlock - 1) / kAppendBlock;
  if (blocks > kAppendMaxBlocks) blocks = kAppendMaxBlocks;
  hipLaunchKernelGGL(infer_append_kernel, dim3((unsigned)blocks), dim3(kAppendBlock), 0, (hipStream_t)stream, logits, (const uint4*)hidden, idx,
                     (unsigned short*)out_logits + row0 * C, hidden ? (uint4*)out_hidden + row0 * (d / 8) : nullptr, out_idx + row0, n_logits,
                     n_hidden8, (int64_t)B);
  GGET_LAUNCH_CHECK();
  return 0;
}

extern "C" int gget_op_node_records(const float* logits, const int64_t* pred, const int64_t* raw_node_idx, const int64_t* idx,
                                    int64_t* records, int64_t* state, int64_t cap, int B, int S, int C, void* stream) {
  GGET_REQUIRE(B >= 1 && S >= 1, "node_records: empty shape (B = %d, S = %d)", B, S);
  GGET_REQUIRE((logits != nullptr) != (pred != nullptr), "node_records: exactly one of logits / pred is given");
  GGET_REQUIRE(!logits || C >= 1, "node_records: C = %d classes", C);
  GGET_REQUIRE(raw_node_idx && idx && records && state, "node_records: null argument");
  GGET_REQUIRE(cap >= 0, "node_records: cap = %lld", (long long)cap);
  const int64_t n_pos = (int64_t)B * S;
  GGET_REQUIRE(n_pos <= kRecMaxPos, "node_records: B * S = %lld positions, at most %lld (GGET_NODE_RECORDS_MAX_POS) per call", (long long)n_pos,
               (long long)kRecMaxPos);
  char* ws = (char*)records_workspace((hipStream_t)stream);
  if (!ws) {
    gget_set_error("node_records: could not allocate %zu bytes of scratch", kRecWsBytes);
    return 1;
  }
  const int chunks = (int)((n_pos + kRecChunk - 1) / kRecChunk);      // <= kRecMaxChunks
  hipLaunchKernelGGL(node_count_kernel, dim3(chunks), dim3(kRecBlock), 0, (hipStream_t)stream, raw_node_idx, (int)n_pos, state, (int64_t*)ws,
                     (int32_t*)(ws + 8));
  GGET_LAUNCH_CHECK();
  hipLaunchKernelGGL(node_write_kernel, dim3(chunks), dim3(kRecBlock), 0, (hipStream_t)stream, logits, pred, raw_node_idx, idx, records, state,
                     cap, (int)n_pos, S, C, (const int64_t*)ws, (const int32_t*)(ws + 8));
  GGET_LAUNCH_CHECK();
  return 0;
}
