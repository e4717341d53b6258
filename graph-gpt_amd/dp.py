"""Data parallelism: one process per GPU; gradients live in ONE flat bf16 array cut into L+2 buckets in the order
backward completes them; each bucket is all-reduced (RCCL, sum) on a side HIP stream as soon as its backward stage is enqueued, so
communication overlaps the remaining backward; 1/world is folded into the fused AdamW.  No DeepSpeed, no DDP hooks.
Here: the collectives, the one read of the DP environment (DpOptions), the three ways a GgetEngine exchanges (torch.distributed, the
C-ABI communicator, none), the rank partition rules and the process-group setup; the schedule is training.GgetEngine.backward."""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Any, Dict, Optional

import torch
import torch.distributed as dist

from . import _lib as L


def dist_ready() -> bool:
    return dist.is_available() and dist.is_initialized()


# ----------------------------------------------------------------------------- bucket collectives
class _Fp32Reduce:
    """Handle of an fp32-accumulated bucket reduction: wait() finishes the collective and rounds the sum back into the bf16
    gradient slice (one rounding instead of the world-1 a bf16 ring sum applies)."""

    def __init__(self, work, wide, dst):
        self.work, self.wide, self.dst = work, wide, dst

    def wait(self):
        if self.work is not None:
            self.work.wait()
        self.dst.copy_(self.wide)


def all_reduce_bucket(flat: torch.Tensor, bucket, group=None, async_op: bool = True, fp32_accumulate: bool = False):
    """Sum-all-reduce ONE gradient bucket (a contiguous [offset, offset+count) slice of the flat gradient array).
    Device-agnostic: RCCL on GPU tensors, gloo on CPU tensors (the CPU tests drive exactly this function).
    fp32_accumulate: widen the slice to fp32 for the reduction (twice the wire bytes, a single final rounding)."""
    off, cnt = bucket
    sl = flat[off: off + cnt]
    if not fp32_accumulate:
        return dist.all_reduce(sl, op=dist.ReduceOp.SUM, group=group, async_op=async_op)
    wide = sl.to(torch.float32)
    work = dist.all_reduce(wide, op=dist.ReduceOp.SUM, group=group, async_op=async_op)
    h = _Fp32Reduce(work if async_op else None, wide, sl)
    if not async_op:
        h.wait()
        return None
    return h


def gather_cl_embeddings(e_local: torch.Tensor, group=None):
    """The embedding matrix of the contrastive loss over all ranks, as the reference builds it for world > 1 (src/utils/loss_utils.py
    :119-124 and cos_sim :149-152): the even rows (`left`) and the odd rows (`right`) of every rank's [B,d] embeddings are all-gathered
    separately, concatenated in rank order, and interleaved again - row 2m of the result is gathered-left[m], row 2m + 1 gathered-right[m].
    With m = r B/2 + m' that puts sample b of rank r at row r B + b.  Returns (E [world B, d], int32 [B] positions of the local rows);
    every rank must hold the same even B.  No gradient flows through the gather: the engine's backward differentiates the loss for the
    local rows only, which is what GatherLayer.backward hands back (loss_utils.py:99-104)."""
    B, d = e_local.shape
    assert B % 2 == 0, f"pretrain-cl needs an even batch, got {B}"
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    halves = []
    for part in (e_local[0::2].contiguous(), e_local[1::2].contiguous()):
        out = [torch.empty_like(part) for _ in range(world)]
        dist.all_gather(out, part, group=group)
        halves.append(torch.cat(out, dim=0))                       # [world B/2, d]
    E = torch.stack(halves, dim=1).reshape(world * B, d)           # hstack([left, right]).reshape(-1, d)
    m = rank * (B // 2) + torch.arange(B // 2, device=e_local.device)
    pos = torch.stack([2 * m, 2 * m + 1], dim=1).reshape(-1).to(torch.int32)
    return E, pos


def _host_staged(flat: torch.Tensor, group) -> bool:
    # gloo's reduce-scatter / all-gather are fed host tensors: a device arena is staged through host memory (NCCL takes device tensors)
    return flat.is_cuda and dist.get_backend(group) == "gloo"


def reduce_scatter_bucket(flat: torch.Tensor, plan, rank: int, world: int, group=None, fp32_accumulate: bool = False):
    """Sharded exchange of ONE gradient bucket (ZeRO-2): the body [off, off + world * slice) reduce-scattered (SUM; rank r's slice
    [off + r slice, off + (r + 1) slice) receives the sum) and the tail [tail_off, tail_off + tail_cnt) all-reduced.  `plan` = the bucket's
    (offset, count, slice, tail_offset, tail_count) of gget_shard_plan.  Synchronous; device-agnostic like all_reduce_bucket (the CPU tests
    drive it on gloo).  Outside the rank's slice the body keeps its local values."""
    off, _, sl, toff, tcnt = plan
    body, mine, tail = flat[off: off + world * sl], flat[off + rank * sl: off + (rank + 1) * sl], flat[toff: toff + tcnt]
    wide = torch.float32 if fp32_accumulate else flat.dtype
    dev = torch.device("cpu") if _host_staged(flat, group) else flat.device
    if sl:
        src = body.to(device=dev, dtype=wide)
        out = torch.empty(sl, dtype=wide, device=dev)
        dist.reduce_scatter_tensor(out, src, op=dist.ReduceOp.SUM, group=group)
        mine.copy_(out)
    if tcnt:
        t = tail.to(device=dev, dtype=wide)
        if t.data_ptr() == tail.data_ptr():
            t = t.clone()
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        tail.copy_(t)


def all_gather_bucket(flat: torch.Tensor, plan, rank: int, world: int, group=None):
    """The inverse of reduce_scatter_bucket's partition: every rank's body slice of `flat` (any dtype: the bf16 weights, the fp32 master /
    Adam arenas) gathered into the body on every rank.  Tails are not touched (every rank holds the same).  Synchronous."""
    off, _, sl, _, _ = plan
    if not sl:
        return
    body, mine = flat[off: off + world * sl], flat[off + rank * sl: off + (rank + 1) * sl]
    dev = torch.device("cpu") if _host_staged(flat, group) else flat.device
    out = torch.empty(world * sl, dtype=flat.dtype, device=dev)
    dist.all_gather_into_tensor(out, mine.to(dev).clone(), group=group)
    body.copy_(out)


def exchange_groups(buckets, bucket_mb: float) -> Dict[int, Any]:
    """{last bucket of a group: (offset, count)} - what one collective covers.  Buckets are numbered in completion order and laid
    out back to front in the flat array, so consecutive buckets are adjacent ranges; a group is closed when it reaches
    GGET_DP_BUCKET_MB (or at the last bucket).  Non-adjacent neighbours (never the case for the engine's layout) close a group too."""
    groups, lo, hi = {}, None, None
    thresh = bucket_mb * 2 ** 20 / 2        # elements (bf16)
    nb = len(buckets)
    for b, (off, cnt) in enumerate(buckets):
        if cnt == 0:        # a frozen bucket (Engine.trainable_buckets): nothing to exchange; what is open goes with the bucket before it
            if lo is not None:
                groups[b - 1] = (lo, hi - lo)
                lo = hi = None
            continue
        if lo is not None and (off + cnt == lo or off == hi):
            lo, hi = min(lo, off), max(hi, off + cnt)
        else:
            if lo is not None:
                groups[b - 1] = (lo, hi - lo)
            lo, hi = off, off + cnt
        if hi - lo >= thresh or b == nb - 1:
            groups[b] = (lo, hi - lo)
            lo = hi = None
    return groups


def _check_zero_stage(stage) -> int:
    stage = int(stage)
    if stage not in (0, 1, 2):
        raise ValueError(f"zero_stage {stage}: only 0 (replicated optimizer step) and 1 / 2 (sharded optimizer step) exist; stage 3 "
                         "(partitioned parameters) is not implemented")
    return stage


# ----------------------------------------------------------------------------- the DP environment
def _env(name: str, default, parse):
    """A record field read from the environment when the record is constructed."""
    return field(default_factory=lambda: parse(os.environ.get(name, default)))


def _flag(s) -> bool:
    return bool(int(s))


def _cus(s) -> int:
    return max(0, int(s))


@dataclass(frozen=True)
class DpOptions:
    """`DpOptions()` reads the environment, once per GgetEngine, which copies the values into attributes that callers may rewrite."""
    force_staged: bool = _env("GGET_FORCE_STAGED", "0", _flag)      # run the bucketed path at world 1
    # GGET_DP_OVERLAP=0: one all-reduce of the whole flat gradient array after the monolithic backward instead of the
    # bucketed exchange overlapped with it (to be decided by measurement on a multi-GPU node)
    overlap: bool = _env("GGET_DP_OVERLAP", "1", _flag)
    # GGET_DP_FP32_REDUCE=1: reduce every bucket in fp32 (see all_reduce_bucket).  GGET_DP_BACKEND=abi: issue the
    # collectives through the C ABI (gget_comm_init / gget_allreduce_grads_async = RCCL on a HIP side stream, no
    # torch.distributed on the data path; the unique id travels once over the existing process group).
    fp32_reduce: bool = _env("GGET_DP_FP32_REDUCE", "0", _flag)
    abi: bool = _env("GGET_DP_BACKEND", "torch", lambda s: s == "abi")
    # GGET_DP_LOOPBACK_WORLD=W (with GGET_DP_BACKEND=abi, single process): the C-ABI exchange runs as rank 0 of W ranks that all hold
    # this rank's gradients (gget_comm_init_loopback) - the schedule of a W-rank job (bucket ranges, side-stream waits, 1/W folded
    # into AdamW) on a one-GPU box; the step must equal the single-rank step
    loopback_world: int = _env("GGET_DP_LOOPBACK_WORLD", "0", lambda s: int(s) if os.environ.get("GGET_DP_BACKEND") == "abi" else 0)
    # GGET_DP_BUCKET_MB=N: consecutive buckets (completion order) are exchanged in ONE collective once they add up to >= N MiB -
    # fewer, larger messages (14 buckets of ~19 MB for the base model; 60 -> 4-5 collectives).  0 (default) = one per bucket.
    bucket_mb: float = _env("GGET_DP_BUCKET_MB", "0", float)
    # sharded optimizer step (ZeRO stage 1 / 2 = one path; OptimConfig.zero_stage, GGET_ZERO_STAGE overrides, None = unset): gradients are
    # reduce-scattered per bucket, every rank runs clip + AdamW over its 1/world of the fp32 state (gget_adamw_step_sharded) and the
    # bf16 weights are all-gathered behind the step.  Taken only when the exchange is live: world > 1, a loopback world, or
    # GGET_FORCE_STAGED=1 with a process group or the C-ABI communicator; otherwise the replicated step runs, unchanged.
    zero_stage: Optional[int] = _env("GGET_ZERO_STAGE", None, lambda s: None if s is None else _check_zero_stage(s))
    # the data-parallel share of the launch menu, carried by the model's handle (GgetEngine.set_dp_menu):
    # GGET_DP_LDS_HEADROOM=1 opts in to the LDS-headroom menu of rounds 2 - 4, GGET_DP_RESERVE_CUS=R leaves R CUs to the collective.
    # From world > 1 on a collective's kernel shares the chip with the compute stream.  (Rounds 2 - 4 kept LDS headroom on every CU for
    # every multi-rank job; round 5's stand-in with RCCL's real register footprint - tools/dp_standin.py - shows the rule buys
    # nothing against such a kernel and costs 0.08 ms alone, 0.2 ms beside it: opt-in now.)  In a real multi-process job that asks
    # for it, the GEMM launches leave GGET_DP_RESERVE_CUS CUs (default 0 = off) FREE for the collective's workgroups, which are held
    # to as many channels (NCCL_MAX_NCHANNELS, unless the user set it; dp_env_defaults() sets it ahead of init_process_group): an
    # RCCL workgroup (256 threads x 261 - 280 registers, 19.7 KiB LDS) cannot share a CU with any 8-wave GEMM workgroup, and a GEMM
    # launch that finds one of "its" CUs taken runs a second round (csrc/gemm.hip).  That rule supersedes the
    # LDS headroom; the RMSNorm backward goes back to its many-small-blocks form for the same reason.
    lds_headroom: bool = _env("GGET_DP_LDS_HEADROOM", "0", _flag)
    reserve_cus: int = _env("GGET_DP_RESERVE_CUS", "0", _cus)
    # single-rank step: nothing touches the gradient array between this backward and AdamW - the engine MAY take the layers' share
    # of the gradient norm from its weight-gradient launches (include/gget.h GGET_OPT_NORM_FROM_BACKWARD).  Opt-in
    # (GGET_NORM_FROM_BACKWARD=1, "" = off): measured in the step it saves its 31 us of norm pass and loses them again in AdamW, whose
    # gradient reads the full pass had warmed the memory-side cache for (7.095 against 7.093 ms, profiles/r04_step_experiments.txt)
    norm_from_backward: bool = _env("GGET_NORM_FROM_BACKWARD", "0", lambda s: bool(int(s or 0)))


# ----------------------------------------------------------------------------- one transport per way of exchanging
# `g` is the GgetEngine (pg / rank / world / fp32_reduce are read when a collective is issued), `e` the native Engine handle.  Every
# collective goes to the CURRENT stream: the schedule (GgetEngine.backward) selects the side stream around the call.
class NoTransport:
    """Single-rank dry run of the staged path (tests): the exchange is the identity.  (Sharding needs a live exchange.)"""
    live, name = False, "torch.distributed/none"

    def __init__(self, g):
        self.g = g

    def ready(self, e):
        pass

    def all_reduce(self, e, off, cnt):      # -> something step() must wait() on, or None
        return None

    def all_reduce_all(self, e):
        pass


class TorchTransport(NoTransport):
    """torch.distributed.  (A ONE-rank process group with GGET_FORCE_STAGED=1 still issues the bucket collectives: the real backend -
    RCCL - runs the whole exchange schedule on a one-GPU box, tests/test_gpu_dist.py::test_torch_rccl_one_rank_group_through_staged_backward)"""
    live = True

    @property
    def name(self) -> str:
        return f"torch.distributed/{dist.get_backend(self.g.pg) if dist_ready() else 'none'}"

    def all_reduce(self, e, off, cnt):
        return all_reduce_bucket(e.grad_bf16, (off, cnt), self.g.pg, async_op=True, fp32_accumulate=self.g.fp32_reduce)

    def all_reduce_all(self, e):
        if self.g.world > 1:
            for rng in e.train_ranges:      # (the whole array unless a prefix is frozen: Engine.set_frozen)
                all_reduce_bucket(e.grad_bf16, rng, self.g.pg, async_op=False, fp32_accumulate=self.g.fp32_reduce)

    def reduce_scatter(self, e, b: int):
        reduce_scatter_bucket(e.grad_bf16, e.shard_buckets[b], self.g.rank, self.g.world, self.g.pg, self.g.fp32_reduce)

    def all_gather(self, e, what: int):
        arena = {L.SHARD_PARAMS: e.param_bf16, L.SHARD_MASTER: e.master, L.SHARD_ADAM_M: e.adam_m, L.SHARD_ADAM_V: e.adam_v,
                 L.SHARD_SLOTS: e.shard_slots, L.SHARD_EMA: e.ema}[what]
        # the norm partials: one "bucket" without a tail; an arena: embeddings, layer 0, ..., heads - the order the forward reads them
        plans = [(0, 0, arena.numel() // self.g.world, 0, 0)] if what == L.SHARD_SLOTS else reversed(e.shard_buckets)
        for plan in plans:
            all_gather_bucket(arena, plan, self.g.rank, self.g.world, self.g.pg)


class AbiTransport(NoTransport):
    """RCCL through the C ABI (works at world 1 too: a one-rank communicator), or its loopback world."""
    live, name = True, "rccl-via-c-abi"

    def ready(self, e):
        # readiness belongs to the ENGINE INSTANCE: a model that re-creates its engine for a larger batch hands the
        # communicator over (Engine.comm_adopt), so this collective bootstrap runs once per job, on every rank together
        g = self.g
        if e.comm_world > 0:
            return
        if g.loopback_world > 0:
            e.comm_init_loopback(g.loopback_world)
            return
        rank = dist.get_rank(g.pg) if g.world > 1 else 0
        uid = [e.comm_unique_id() if rank == 0 else None]
        if g.world > 1:
            dist.broadcast_object_list(uid, src=0, group=g.pg)
        e.comm_init(rank, g.world, uid[0])

    def all_reduce(self, e, off, cnt):
        e.allreduce_range_async(off, cnt, self.g.fp32_reduce)

    def all_reduce_all(self, e):
        e.allreduce_grads_async(-1, self.g.fp32_reduce)

    def reduce_scatter(self, e, b: int):
        e.reduce_scatter_grads_async(b, self.g.fp32_reduce)

    def all_gather(self, e, what: int):     # (SHARD_SLOTS is a no-op on the loopback, which summed every rank's chunks itself)
        e.shard_allgather_async(what)


def pick_transport(g) -> NoTransport:
    """The one place that decides how `g` exchanges.  Evaluated per call: `force_staged`, `abi_comm` and `world` stay writable."""
    if g.abi_comm:
        return AbiTransport(g)
    if g.world > 1 or (g.force_staged and dist_ready()):
        return TorchTransport(g)
    return NoTransport(g)


# ----------------------------------------------------------------------------- rank partition rules
def shard_seed(base_seed: int, rank: int) -> int:
    """Per-rank data seed: ranks draw independent batches (reference misc_utils.py:536-538 seeds with
    `initial_seed - rank`; the synthetic generator uses base + rank)."""
    return int(base_seed) + int(rank)


def pretrain_rank_sampler(sample_idx, epochs: int, seed: int, rank: int):
    """Pre-training partition rule (reference get_pt_train_valid_test_sampler loader_utils.py:328-333, reset_pt_train_sampler
    :412-442, seeding misc_utils.py:536-538): every rank keeps the FULL index list repeated `epochs` times and shuffles it
    with its own generator seeded `seed - rank` - ranks draw independently, not disjointly (the token budget, not the
    epoch, bounds the run).  Python's `random` module like the reference, so the order is the reference's order."""
    import random
    idx = [int(i) for i in sample_idx] * max(1, int(epochs))
    random.Random(int(seed) - int(rank)).shuffle(idx)
    return idx


def finetune_rank_sampler(sample_idx, world_size: int, rank: int, seed: int, epoch: int = 0):
    """Fine-tune partition rule (reference distribute_sampler_with_rnd_seed loader_utils.py:78-90, called with
    seed = finetune.seed + epoch at :622-627): one permutation per epoch shared by all ranks, truncated to a multiple of the
    world size, rank r takes positions r, r + world, ...  -> disjoint shards of equal length that change every epoch."""
    sample_idx = torch.as_tensor(sample_idx)
    g = torch.Generator()
    g.manual_seed(int(seed) + int(epoch))
    indices = torch.randperm(len(sample_idx), generator=g).tolist()
    total = (len(sample_idx) // world_size) * world_size
    return sample_idx[indices[rank:total:world_size]].tolist()


def eval_rank_sampler(sample_idx, world_size: int, rank: int, shuffle_seed: Optional[int] = None):
    """Evaluation partition rule (reference distribute_sampler loader_utils.py:70-75, used for the valid / test samplers at
    :256, :270): indices sorted, rank r keeps those at sorted positions i with i % world == r (every sample exactly once
    across ranks, shard sizes differ by at most one), then shuffled locally (order is irrelevant to the metrics)."""
    import random
    vec = sorted(int(i) for i in sample_idx)
    out = [vec[i] for i in range(len(vec)) if i % world_size == rank]
    if shuffle_seed is not None:
        random.Random(shuffle_seed).shuffle(out)
    return out


def all_gather_varlen(q: torch.Tensor) -> torch.Tensor:
    """reference misc_utils.all_gather (:472-504): concatenates per-rank tensors of different lengths along dim 0."""
    ws = dist.get_world_size()
    local = torch.tensor(q.shape[0], device=q.device)
    sizes = [torch.zeros_like(local) for _ in range(ws)]
    dist.all_gather(sizes, local)
    mx = int(max(sizes).item())
    if mx > q.shape[0]:
        q = torch.cat([q, torch.zeros([mx - q.shape[0]] + list(q.shape[1:]), device=q.device, dtype=q.dtype)], dim=0)
    out = [torch.zeros_like(q) for _ in range(ws)]
    dist.all_gather(out, q)
    return torch.cat([o[: int(n)] for o, n in zip(out, sizes)])


# ----------------------------------------------------------------------------- distributed env
def dp_env_defaults() -> int:
    """Environment a multi-process job wants BEFORE its process group / communicator exists: the collective library is held to as many
    channels (= workgroups) as the GEMM launches leave CUs free - GGET_DP_RESERVE_CUS = R, OFF by default (0: tools/dp_standin.py measured that
    16 free CUs do not protect the exact-fit launches and that 32 cost more than the collisions they prevent at the 8-GPU residency of the
    collectives); an NCCL_MAX_NCHANNELS the user set wins.  Returns R (GgetEngine applies the GEMM side: the handle's data-parallel menu)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    r = _cus(os.environ.get("GGET_DP_RESERVE_CUS", "0")) if world > 1 else 0
    if r:
        os.environ.setdefault("NCCL_MAX_NCHANNELS", str(r))
    return r


def set_dist_env(backend: Optional[str] = None):
    """reference misc_utils.set_dist_env (:507-539): env:// rendezvous, one process per GPU, barrier."""
    dp_env_defaults()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if torch.cuda.is_available():
        torch.cuda.set_device(local)
    if world > 1 and not dist.is_initialized():
        backend = backend or ("nccl" if torch.cuda.is_available() else "gloo")
        kw = {}
        if backend == "nccl":
            kw["device_id"] = torch.device("cuda", local)
        dist.init_process_group(backend=backend, init_method="env://", **kw)
        dist.barrier()
    return rank, local, world
