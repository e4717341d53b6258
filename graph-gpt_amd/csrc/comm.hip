// libgget_hip.so - data-parallel gradient exchange over RCCL (reference: DDP all-reduce opt_utils.py:13,
// DeepSpeed ZeRO-2 reduce-scatter ds_config2_pt.json:29-32, communicator setup misc_utils.py:519-526)
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "engine.h"
#include <rccl/rccl.h>   // types and enums only: the library is bound with dlopen (below)

// The library is bound with dlopen("librccl.so.1") at the first gget_comm_* call: inside a PyTorch process that is the copy
// torch already loaded (one RCCL per process), and a caller that never exchanges gradients never needs RCCL at all.
namespace {

struct RcclApi {
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*ReduceScatter)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool ok = false;
  char why[256] = "symbols missing";     // dlerror() text captured once, at the failing dlopen (a second dlerror() call returns NULL)
};

RcclApi* rccl() {
  static RcclApi api;
  static bool tried = false;
  if (!tried) {
    tried = true;
    void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) {
      const char* e = dlerror();
      snprintf(api.why, sizeof(api.why), "%s", e ? e : "dlopen failed");
    }
    if (lib) {
      api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
      api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
      api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
      api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(lib, "ncclAllReduce"));
      api.ReduceScatter = reinterpret_cast<decltype(api.ReduceScatter)>(dlsym(lib, "ncclReduceScatter"));
      api.AllGather = reinterpret_cast<decltype(api.AllGather)>(dlsym(lib, "ncclAllGather"));
      api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(dlsym(lib, "ncclGroupStart"));
      api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(dlsym(lib, "ncclGroupEnd"));
      api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
      api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllReduce && api.ReduceScatter && api.AllGather &&
               api.GroupStart && api.GroupEnd && api.GetErrorString;
    }
  }
  return &api;
}

#define GGET_RCCL_CHECK(expr)                                                                          \
  do {                                                                                                 \
    ncclResult_t _r = (expr);                                                                          \
    if (_r != ncclSuccess) {                                                                           \
      gget_set_error("%s failed: %s (%s:%d)", #expr, rccl()->GetErrorString(_r), __FILE__, __LINE__);  \
      return 1;                                                                                        \
    }                                                                                                  \
  } while (0)

__global__ void __launch_bounds__(256) bf16_to_f32_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, uint64_t n) {
  // n is a multiple of 128 (flat-arena alignment): 8 elements per thread, 16-byte loads, two 16-byte stores
  for (uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < n; i += (uint64_t)gridDim.x * 256 * 8) {
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(src + i), f);
    *reinterpret_cast<float4*>(dst + i) = make_float4(f[0], f[1], f[2], f[3]);
    *reinterpret_cast<float4*>(dst + i + 4) = make_float4(f[4], f[5], f[6], f[7]);
  }
}

}  // namespace

extern "C" int gget_comm_unique_id(void* out_bytes) {
  GGET_REQUIRE(out_bytes, "comm_unique_id: null argument");
  GGET_REQUIRE(rccl()->ok, "RCCL (librccl.so.1) could not be loaded: %s", rccl()->why);
  static_assert(sizeof(ncclUniqueId) == GGET_UNIQUE_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  GGET_RCCL_CHECK(rccl()->GetUniqueId(&id));
  memcpy(out_bytes, &id, sizeof(id));
  return 0;
}

extern "C" int gget_comm_init(gget_handle_t h, int rank, int world, const void* unique_id_bytes) {
  GGET_REQUIRE(h && unique_id_bytes && world >= 1 && rank >= 0 && rank < world, "comm_init: bad arguments (rank %d world %d)", rank, world);
  GGET_REQUIRE(h->comm == nullptr, "comm_init: this handle already has a communicator");
  GGET_REQUIRE(rccl()->ok, "RCCL (librccl.so.1) could not be loaded: %s", rccl()->why);
  ncclUniqueId id;
  memcpy(&id, unique_id_bytes, sizeof(id));
  ncclComm_t c = nullptr;
  GGET_RCCL_CHECK(rccl()->CommInitRank(&c, world, id, rank));
  h->comm = c;
  h->comm_rank = rank;
  h->comm_world = world;
  return 0;
}

extern "C" int gget_comm_destroy(gget_handle_t h) {
  if (!h) return 0;
  if (h->comm) {
    rccl()->CommDestroy(static_cast<ncclComm_t>(h->comm));
    h->comm = nullptr;
  }
  if (h->comm_f32) {
    (void)hipFree(h->comm_f32);
    h->comm_f32 = nullptr;
    h->comm_f32_elems = 0;
  }
  h->comm_world = 1;
  h->comm_loopback = false;
  return 0;
}

extern "C" int gget_comm_move(gget_handle_t dst, gget_handle_t src) {
  // A handle that is re-created with larger capacities (a bigger batch arrived) must keep exchanging gradients with the SAME
  // communicator: creating a new one is a collective, and only the ranks whose batch grew would enter it.
  GGET_REQUIRE(dst && src && dst != src, "comm_move: bad arguments");
  GGET_REQUIRE(dst->comm == nullptr && !dst->comm_loopback, "comm_move: the destination handle already has a communicator");
  GGET_REQUIRE(dst->plan.n_params == src->plan.n_params, "comm_move: the two handles hold different models");
  dst->comm = src->comm;
  dst->comm_loopback = src->comm_loopback;
  src->comm_loopback = false;
  dst->comm_rank = src->comm_rank;
  dst->comm_world = src->comm_world;
  dst->comm_f32 = src->comm_f32;
  dst->comm_f32_elems = src->comm_f32_elems;
  src->comm = nullptr;
  src->comm_f32 = nullptr;
  src->comm_f32_elems = 0;
  src->comm_world = 1;
  return 0;
}

__global__ void __launch_bounds__(256) scale_bf16_kernel(bf16_t* __restrict__ g, uint64_t n, float mul) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) g[i] = f2bf(bf2f(g[i]) * mul);
}

extern "C" int gget_comm_init_loopback(gget_handle_t h, int world) {
  GGET_REQUIRE(h && world >= 1, "comm_init_loopback: bad arguments (world %d)", world);
  GGET_REQUIRE(h->comm == nullptr && !h->comm_loopback, "comm_init_loopback: this handle already has a communicator");
  h->comm_loopback = true;
  h->comm_rank = 0;
  h->comm_world = world;
  return 0;
}

// the communicator's fp32 staging buffer (grown to the largest bucket) holding the widened [g, g + n)
static int widen_to_stage(gget_handle_t h, const bf16_t* g, uint64_t n, hipStream_t st) {
  if (h->comm_f32_elems < n) {
    if (h->comm_f32) GGET_HIP_CHECK(hipFree(h->comm_f32));
    h->comm_f32 = nullptr;
    uint64_t cap = 0;
    for (const auto& r : h->bucket_range) cap = std::max<uint64_t>(cap, r.second - r.first);
    cap = std::max<uint64_t>(cap, n);
    GGET_HIP_CHECK(hipMalloc(&h->comm_f32, cap * sizeof(float)));
    h->comm_f32_elems = cap;
  }
  const int grid = (int)std::min<uint64_t>(4096, (n / 8 + 255) / 256);
  hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(grid), dim3(256), 0, st, g, h->comm_f32, n);
  GGET_LAUNCH_CHECK();
  return 0;
}

extern "C" int gget_allreduce_range_async(gget_handle_t h, uint64_t offset, uint64_t count, int fp32_accumulate, void* side_stream) {
  GGET_REQUIRE(h && (h->comm || h->comm_loopback), "allreduce_grads: call gget_comm_init first");
  GGET_REQUIRE(offset <= h->plan.n_params && count <= h->plan.n_params - offset, "allreduce_range: [%llu, +%llu) leaves the gradient array",
               (unsigned long long)offset, (unsigned long long)count);
  if (count == 0) return 0;
  hipStream_t st = (hipStream_t)side_stream;
  bf16_t* g = h->G + offset;
  const uint64_t n = count;
  if (h->comm_loopback) {   // world identical contributions: the sum is world x (exact in bf16 for a power of two)
    const int grid = (int)std::min<uint64_t>(4096, (n + 255) / 256);
    hipLaunchKernelGGL(scale_bf16_kernel, dim3(grid), dim3(256), 0, st, g, n, (float)h->comm_world);
    GGET_LAUNCH_CHECK();
    return 0;
  }
  ncclComm_t c = static_cast<ncclComm_t>(h->comm);
  if (!fp32_accumulate) {
    GGET_RCCL_CHECK(rccl()->AllReduce(g, g, n, ncclBfloat16, ncclSum, c, st));
    return 0;
  }
  // fp32 reduction: a bf16 ring sum rounds after every hop (world - 1 roundings); widening the bucket first makes the sum
  // exact up to the single final rounding, at twice the bytes on the wire.  Staging buffer owned by the communicator.
  if (int e = widen_to_stage(h, g, n, st)) return e;
  GGET_RCCL_CHECK(rccl()->AllReduce(h->comm_f32, h->comm_f32, n, ncclFloat32, ncclSum, c, st));
  return k_f32_to_bf16(h->comm_f32, g, n, st);
}

extern "C" int gget_reduce_scatter_grads_async(gget_handle_t h, int bucket, int fp32_accumulate, void* side_stream) {
  GGET_REQUIRE(h && (h->comm || h->comm_loopback), "reduce_scatter_grads: call gget_comm_init first");
  GGET_REQUIRE(h->shard_world > 0, "reduce_scatter_grads: call gget_shard_init first");
  GGET_REQUIRE(bucket >= 0 && bucket < (int)h->shard_plan.size(), "reduce_scatter_grads: bucket %d out of range", bucket);
  const ShardBucket& b = h->shard_plan[bucket];
  if (b.cnt == 0) return 0;     // (a frozen bucket, gget_set_frozen: nothing to exchange)
  // the loopback stands for world ranks with this rank's gradients and does the work of all of them: body and tail are world x
  if (h->comm_loopback) return gget_allreduce_range_async(h, b.off, b.cnt, 0, side_stream);
  hipStream_t st = (hipStream_t)side_stream;
  ncclComm_t c = static_cast<ncclComm_t>(h->comm);
  const uint64_t body = (uint64_t)h->shard_world * b.slice, mine = (uint64_t)h->shard_rank * b.slice;
  bf16_t* g = h->G + b.off;
  // in-place reduce-scatter (recvbuff = sendbuff + rank * recvcount) of the body and all-reduce of the tail, one group
  if (!fp32_accumulate) {
    GGET_RCCL_CHECK(rccl()->GroupStart());
    ncclResult_t r1 = ncclSuccess, r2 = ncclSuccess;
    if (b.slice) r1 = rccl()->ReduceScatter(g, g + mine, b.slice, ncclBfloat16, ncclSum, c, st);
    if (b.tail_cnt) r2 = rccl()->AllReduce(g + body, g + body, b.tail_cnt, ncclBfloat16, ncclSum, c, st);
    GGET_RCCL_CHECK(rccl()->GroupEnd());
    GGET_RCCL_CHECK(r1);
    GGET_RCCL_CHECK(r2);
    return 0;
  }
  // fp32 reduction, as gget_allreduce_range_async: the bucket widened once, the two collectives on the staging copy, this rank's slice
  // and the tail rounded back
  if (int e = widen_to_stage(h, g, b.cnt, st)) return e;
  float* w = h->comm_f32;
  GGET_RCCL_CHECK(rccl()->GroupStart());
  ncclResult_t r1 = ncclSuccess, r2 = ncclSuccess;
  if (b.slice) r1 = rccl()->ReduceScatter(w, w + mine, b.slice, ncclFloat32, ncclSum, c, st);
  if (b.tail_cnt) r2 = rccl()->AllReduce(w + body, w + body, b.tail_cnt, ncclFloat32, ncclSum, c, st);
  GGET_RCCL_CHECK(rccl()->GroupEnd());
  GGET_RCCL_CHECK(r1);
  GGET_RCCL_CHECK(r2);
  if (b.slice)
    if (int e = k_f32_to_bf16(w + mine, g + mine, b.slice, st)) return e;
  if (b.tail_cnt)
    if (int e = k_f32_to_bf16(w + body, g + body, b.tail_cnt, st)) return e;
  return 0;
}

extern "C" int gget_shard_allgather_async(gget_handle_t h, int what, float* slots_dev, void* stream) {
  GGET_REQUIRE(h && (h->comm || h->comm_loopback), "shard_allgather: call gget_comm_init first");
  GGET_REQUIRE(h->shard_world > 0, "shard_allgather: call gget_shard_init first");
  GGET_REQUIRE(what >= GGET_SHARD_PARAMS && what <= GGET_SHARD_EMA, "shard_allgather: unknown arena %d", what);
  GGET_REQUIRE(what != GGET_SHARD_SLOTS || slots_dev, "shard_allgather: null slot vector");
  GGET_REQUIRE(what != GGET_SHARD_EMA || h->ema, "shard_allgather: no EMA arena (gget_ema_attach)");
  GGET_REQUIRE(what == GGET_SHARD_PARAMS || what == GGET_SHARD_SLOTS || what == GGET_SHARD_EMA || (h->master && h->am && h->av),
               "shard_allgather: no fp32 state");
  if (h->comm_loopback) return 0;    // (the loopback handle updated and summed every rank's share itself)
  hipStream_t st = (hipStream_t)stream;
  ncclComm_t c = static_cast<ncclComm_t>(h->comm);
  const int rank = h->shard_rank;
  if (what == GGET_SHARD_SLOTS) {
    GGET_RCCL_CHECK(rccl()->AllGather(slots_dev + (size_t)rank * h->shard_slots, slots_dev, h->shard_slots, ncclFloat32, c, st));
    return 0;
  }
  // in place (sendbuff = recvbuff + rank * sendcount), one collective per bucket body in the order the forward reads them: embeddings,
  // layer 0, ..., heads (= the buckets backwards)
  for (int bi = (int)h->shard_plan.size() - 1; bi >= 0; --bi) {
    const ShardBucket& b = h->shard_plan[bi];
    if (!b.slice) continue;
    const uint64_t mine = b.off + (uint64_t)rank * b.slice;
    if (what == GGET_SHARD_PARAMS) {
      GGET_RCCL_CHECK(rccl()->AllGather(h->P + mine, h->P + b.off, b.slice, ncclBfloat16, c, st));
    } else {
      float* x = what == GGET_SHARD_MASTER ? h->master : what == GGET_SHARD_ADAM_M ? h->am : what == GGET_SHARD_ADAM_V ? h->av : h->ema;
      GGET_RCCL_CHECK(rccl()->AllGather(x + mine, x + b.off, b.slice, ncclFloat32, c, st));
    }
  }
  return 0;
}

extern "C" int gget_allreduce_grads_async(gget_handle_t h, int bucket, int fp32_accumulate, void* side_stream) {
  GGET_REQUIRE(h && (h->comm || h->comm_loopback), "allreduce_grads: call gget_comm_init first");
  GGET_REQUIRE(bucket >= -1 && bucket < (int)h->bucket_range.size(), "allreduce_grads: bucket %d out of range", bucket);
  if (h->frozen >= 0) {     // the trainable share only: of the bucket, or (-1) every trainable range
    if (bucket >= 0) {
      const auto r = h->bucket_train_range(bucket);
      return gget_allreduce_range_async(h, r.first, r.second, fp32_accumulate, side_stream);
    }
    for (const auto& r : h->train_ranges)
      if (int e = gget_allreduce_range_async(h, r.first, r.second, fp32_accumulate, side_stream)) return e;
    return 0;
  }
  const uint64_t lo = bucket < 0 ? 0 : h->bucket_range[bucket].first;
  const uint64_t hi = bucket < 0 ? h->plan.n_params : h->bucket_range[bucket].second;
  return gget_allreduce_range_async(h, lo, hi - lo, fp32_accumulate, side_stream);
}
