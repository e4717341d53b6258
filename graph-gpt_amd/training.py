"""Training-side surface for the hot path: the engine object the reference gets from
`deepspeed.initialize` (SURVEY.md 8b "Engine protocol": .module/.backward/.step/.save_checkpoint/
.load_checkpoint/.global_steps/.device), the per-step loop of `batch_training` / `ft_batch_training`
(reference src/utils/training_utils.py:7-95, :98-205), the LR schedules (loss_utils.py:322-367,
ds_config2_pt.json:20-28) and a lean `TrainingPipeline` / `TrainingMode` (reference
src/training/pipeline.py:60-95, mode.py:46-89) that drives them from any iterable of collated batches.

Data parallelism: GgetEngine.backward is the exchange schedule; the collectives, transports and rank rules are in dp.py.
"""
from __future__ import annotations

import abc
import contextlib
import math
import os
import time
from typing import Any, Callable, Dict, Iterable, Optional

import numpy as np
import torch
import torch.distributed as dist

from .dp import (DpOptions, _check_zero_stage, _Fp32Reduce, _host_staged, all_gather_bucket, all_gather_varlen,  # noqa: F401  (re-exported)
                 all_reduce_bucket, dist_ready, dp_env_defaults, eval_rank_sampler, exchange_groups, finetune_rank_sampler,
                 pick_transport, pretrain_rank_sampler, reduce_scatter_bucket, set_dist_env, shard_seed)
from .modeling import GraphGPTPretrainBase, GraphGPTTaskModel, _GgetModel


# ----------------------------------------------------------------------------- LR schedules
def one_cycle_lr(step: int, max_lr: float, total_steps: int, pct_start: float, min_lr: float = 0.0) -> float:
    """torch OneCycleLR(anneal='cos', div_factor=25) exactly as `_py_one_cycle` configures it
    (reference src/utils/loss_utils.py:322-367); `step` is the 0-based scheduler step."""
    initial = max_lr / 25.0
    final = min_lr if min_lr > 0 else initial / 1e4
    up_end = float(pct_start * total_steps) - 1
    down_end = total_steps - 1

    def cos_anneal(a, b, pct):
        return b + (a - b) / 2.0 * (math.cos(math.pi * pct) + 1)

    if step <= up_end:
        return cos_anneal(initial, max_lr, step / up_end if up_end > 0 else 1.0)
    return cos_anneal(max_lr, final, (step - up_end) / (down_end - up_end))


def warmup_decay_lr(step: int, max_lr: float, min_lr: float, warmup: int, total: int) -> float:
    """DeepSpeed WarmupDecayLR as named by examples/ds_config2_pt.json:20-28 (log warm-up, linear decay)."""
    if step < warmup:
        gamma = math.log(step + 1) / math.log(max(2, warmup))
    else:
        gamma = max(0.0, (total - step) / max(1.0, total - warmup))
    return min_lr + (max_lr - min_lr) * gamma


class OptimConfig:
    """Defaults = the reference pre-train launch script (examples/graph_lvl/pcqm4m_v2_pretrain.sh:53-57)."""

    def __init__(self, lr=3e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1, max_grad_norm=1.0, min_lr=0.0,
                 warmup_num_steps=0, total_num_steps=0, schedule="constant", onecycle_extra_step=1, gradient_accumulation_steps=1,
                 zero_stage=0, use_ema=False, ema_decay=0.9999, layerwise_lr_decay=None, layerwise_lr_version=1, no_decay_1d=False):
        # parameter groups built by initialize(): layer-wise lr decay (reference loss_utils.py:370-412, see layerwise_lr_scales; None =
        # off, version 1 or 3) and the "no weight decay on 1-D parameters" split (norm weights, LayerScale, biases)
        self.layerwise_lr_decay = None if layerwise_lr_decay is None else float(layerwise_lr_decay)
        self.layerwise_lr_version, self.no_decay_1d = int(layerwise_lr_version), bool(no_decay_1d)
        if self.layerwise_lr_decay is not None and not self.layerwise_lr_decay >= 0.0:
            raise ValueError(f"layerwise_lr_decay {layerwise_lr_decay} is not >= 0")
        if self.layerwise_lr_version not in (1, 3):
            raise ValueError(f"layerwise_lr_version {layerwise_lr_version}: 1 or 3 (the reference's v2 follows module registration order)")
        # `training.optimizer.use_ema` / `ema_decay` (reference base_configs.py:75-87; the fine-tune launch scripts run use_ema=true with
        # 0.9999): GgetEngine keeps an exponential moving average of the fp32 master weights (see GgetEngine.ema_decay_at / step)
        self.use_ema, self.ema_decay = bool(use_ema), float(ema_decay)
        if not 0.0 <= self.ema_decay <= 1.0:
            raise ValueError(f"ema_decay {ema_decay} outside [0, 1]")
        # DeepSpeed's zero_optimization.stage (examples/ds_config2_pt.json:29-32): 1 and 2 select the sharded optimizer step of a
        # data-parallel run (see GgetEngine; this engine partitions the work, not the buffers, so the two stages are one path), 0 the
        # replicated step; the environment variable GGET_ZERO_STAGE overrides it
        self.zero_stage = _check_zero_stage(zero_stage)
        # micro-batches per optimizer step (the DeepSpeed engine's `gradient_accumulation_steps`, conf_utils.py:59-66): see GgetEngine.step
        self.gradient_accumulation_steps = max(1, int(gradient_accumulation_steps))
        self.lr, self.betas, self.eps, self.weight_decay = lr, tuple(betas), eps, weight_decay
        self.max_grad_norm, self.min_lr = max_grad_norm, min_lr
        self.warmup_num_steps, self.total_num_steps, self.schedule = warmup_num_steps, total_num_steps, schedule
        # OneCycleLR's total_steps: total_num_steps + 1 on the reference's DDP path (opt_utils.py:30, "to avoid error of
        # lr_scheduler.step() in last step"), total_num_steps on its DeepSpeed fine-tune path (conf_utils.py:124)
        self.onecycle_extra_step = int(onecycle_extra_step)

    def lr_at(self, step: int) -> float:
        if self.schedule == "onecycle" and self.total_num_steps > 0:
            total = self.total_num_steps + self.onecycle_extra_step
            return one_cycle_lr(min(step, total - 1), self.lr, total,
                                self.warmup_num_steps / max(1, self.total_num_steps), self.min_lr)
        if self.schedule == "warmup_decay" and self.total_num_steps > 0:
            return warmup_decay_lr(step, self.lr, self.min_lr, self.warmup_num_steps, self.total_num_steps)
        return self.lr


def schedule_steps(total_tokens: float, tokens_per_sample: float, batch_size: int, world_size: int) -> int:
    """Optimizer steps of a token-budgeted run (reference base_configs.py:54-60): the global batch is world * batch_size."""
    return int(total_tokens // (tokens_per_sample * batch_size * world_size))


# ----------------------------------------------------------------------------- parameter groups
_EMBED_SIDE = ("embed_layernorm.", "embed_proj.", "emb_mask_token")     # feed the token embeddings (embed_dim > 0)
_HEAD_SIDE = ("n_token_proj.", "cl_proj.")                              # feed / sit beside lm_head


def layerwise_depths(names, num_layers: int, version: int = 1, feat_agg_group: bool = True) -> Dict[str, int]:
    """Depth of every state-dict name in the reference's layer-wise groups, counted down from the head (depth 0).
    version 1 (loss_utils.py:370-387) - the groups in order: embed_tokens, stacked_feat_agg (`feat_agg_group`: the reference adds the
    group whenever the module exists, with or without parameters), one per decoder layer, model.norm, lm_head, score (each head if the
    model has it); depth = groups behind it.  version 3 (:398-412): heads 0, everything else 1.
    Names the reference's groups leave out take the depth of the group they feed: n_token_proj / cl_proj that of lm_head,
    embed_layernorm / embed_proj / emb_mask_token that of embed_tokens."""
    names = list(names)
    heads = [h for h in ("lm_head", "score") if any(n.startswith(h + ".") for n in names)]
    if version == 3:
        return {n: 0 if n.startswith(tuple(h + "." for h in heads) + _HEAD_SIDE) else 1 for n in names}
    if version != 1:
        raise ValueError(f"layer-wise lr version {version}: 1 or 3")
    order = ["embed"] + (["agg"] if feat_agg_group else []) + [f"layer{i}" for i in range(num_layers)] + ["norm"] + heads
    depth_of = {g: len(order) - 1 - i for i, g in enumerate(order)}
    out = {}
    for n in names:
        parts = n.split(".")
        if n.startswith("model.embed_tokens.") or n.startswith(_EMBED_SIDE):
            g = "embed"
        elif n.startswith("stacked_feat_agg."):
            g = "agg"
        elif parts[:2] == ["model", "layers"]:
            g = f"layer{int(parts[2])}"
        elif n.startswith("model.norm."):
            g = "norm"
        elif n.startswith(_HEAD_SIDE):
            g = "lm_head"
        elif parts[0] in heads:
            g = parts[0]
        else:
            raise KeyError(f"layerwise_depths: {n!r} belongs to no group")
        out[n] = depth_of[g]
    return out


def _feat_agg_group(model) -> bool:
    """Whether the reference's model has a `stacked_feat_agg` module (modeling_pretrain.py:67 always; modeling_finetune.py:74 only for
    stack_method short / long) - v1 gives it a group of its own even when the module has no parameters."""
    return isinstance(model, GraphGPTPretrainBase) or getattr(model.config, "stack_method", None) in ("short", "long")


def layerwise_lr_scales(model, lr_decay: float, version: int = 1) -> Dict[str, float]:
    """State-dict name -> lr_decay ** depth: the learning-rate scales of the reference's get_layerwise_param_groups (version 1) or
    get_layerwise_param_groups_v3 (version 3), for Engine.set_param_scales / GgetEngine.set_param_scales.
    The one deliberate difference: the reference's groups leave n_token_proj, cl_proj, embed_layernorm, embed_proj (and emb_mask_token)
    out of the optimizer altogether - they would never train.  Here they take the depth of the group they feed: n_token_proj and
    cl_proj with lm_head, embed_layernorm / embed_proj / emb_mask_token with embed_tokens."""
    depths = layerwise_depths(model._flat, model.config.num_hidden_layers, version, _feat_agg_group(model))
    return {n: math.pow(lr_decay, d) for n, d in depths.items()}


# ----------------------------------------------------------------------------- engine protocol
def _refuse_stale_state(module, prefix, keep_vars):
    e = getattr(module, "_engine", None)
    if e is not None and e.shard_stale:
        raise RuntimeError("state_dict(): the fp32 master weights are partitioned after a sharded (ZeRO-2) optimizer step and stale outside "
                           "this rank's share; call engine.consolidate() on every rank first")


class GgetEngine:
    """What `deepspeed.initialize(model=...)` returns in the reference (pretrain_mode.py:281-287), rebuilt on
    the HIP engine: forward via `engine(...)`, `engine.backward(loss)`, `engine.step()`."""

    def __init__(self, model: _GgetModel, optim: Optional[OptimConfig] = None, process_group=None):
        self.module = model
        self.optim = optim or OptimConfig()
        self.global_steps = 0
        self.pg = process_group
        real_world = dist.get_world_size(process_group) if dist_ready() else 1
        self.world = real_world
        self._comm_stream = None
        self._pending = []
        # the DP environment (dp.DpOptions describes every knob), copied into attributes that callers may rewrite afterwards
        o = DpOptions()
        self.force_staged, self.overlap, self.fp32_reduce, self.bucket_mb = o.force_staged, o.overlap, o.fp32_reduce, o.bucket_mb
        self.abi_comm, self.loopback_world = o.abi, o.loopback_world
        self._dp_lds_headroom, self._norm_from_backward = o.lds_headroom, o.norm_from_backward
        if self.loopback_world > 0:
            assert self.world == 1, "the loopback communicator replaces the process group: run it in a single process"
            self.world = self.loopback_world
            self.force_staged = True
        self.zero_stage = o.zero_stage if o.zero_stage is not None else _check_zero_stage(getattr(self.optim, "zero_stage", 0))
        self.rank = dist.get_rank(process_group) if dist_ready() and self.loopback_world == 0 else 0
        # the sharded optimizer step is taken only when the exchange is live (not the single-rank shortcut, and a transport behind it)
        self.sharded = self.zero_stage > 0 and (self.world > 1 or self.force_staged) and pick_transport(self).live
        if self.sharded:
            model.register_state_dict_pre_hook(_refuse_stale_state)
        # measurement switch (bench.py `dp.exposed_comm_ms`): False runs the same staged backward WITHOUT issuing the collectives -
        # the ranks then drift apart, so it is only ever set for a few untimed-for-throughput diagnostic steps
        self.exchange = True
        self.reserved_cus = 0
        # gradient accumulation (DeepSpeed branch, conf_utils.py:59-66 -> the DS engine steps at the boundary only): the micro-batches'
        # gradients are summed in the engine's fp32 accumulator arena (Engine.grad_accumulate, one HIP launch); step() k - 1 times out of
        # k only does that.  micro_steps counts every such call; _grad_acc is the arena view (None before the first k > 1 step)
        self.micro_steps = 0
        self._grad_acc = None
        # GradScaler's rule of the reference's DDP branch (training_utils.py:46-86): an optimizer step whose gradient norm is inf / NaN is
        # skipped (weights and Adam state untouched, Adam's step count not advanced) while the LR schedule still advances
        self.skip_nonfinite = False
        self.skipped_steps = 0
        # parameter groups (set_param_groups / set_param_scales): ({name: lr_scale}, {name: wd_scale}) over every parameter, or None;
        # the table lives on the engine instance and is handed to a re-created one in step(), as skip_nonfinite is
        self._param_scales = None
        # weight EMA (optim.use_ema): step() calls so far that averaged = the reference's `train_stats.j` at its update_ema call
        self.ema_updates = 0
        if self.world > 1 and torch.cuda.is_available():     # (DpOptions.reserve_cus: a real multi-process job only, not a loopback world)
            if real_world > 1:
                self.reserved_cus = o.reserve_cus
            model.set_dp_menu(self.reserved_cus, self._dp_lds_headroom)
        model.materialize_grads = False  # fused path: gradients stay in the flat bf16 arena
        model._managed_by_engine = True  # the bucketed exchange below replaces the all-reduce of _autograd_backward

    @property
    def device(self):
        return self.module.device

    def __call__(self, *a, **k):
        if self.module._engine is not None:
            self.module._engine.await_params()    # (the engine's forwards wait too; explicit for readers that bypass them)
        return self.module(*a, **k)

    def train(self, mode=True):
        self.module.train(mode)
        return self

    def eval(self):
        return self.train(False)

    # -- backward: the exchange schedule (dp.pick_transport says how a bucket travels)
    def backward(self, loss=None):
        e = self.module._engine
        tx = pick_transport(self)
        tx.ready(e)
        fold = self.world == 1 and not self.force_staged and self._norm_from_backward
        if getattr(e, "_norm_fold", None) != fold:
            from . import _lib as L
            e.set_option(L.OPT_NORM_FROM_BACKWARD, int(fold))
            e._norm_fold = fold
        if self.world == 1 and not self.force_staged:
            e.backward()
            return
        if self.sharded:
            self._ensure_shard(e)
        if not self.overlap:                # one exchange behind the monolithic backward
            e.backward()
            if self.exchange and self.sharded:
                for b in range(len(e.buckets)):
                    tx.reduce_scatter(e, b)
            elif self.exchange:
                tx.all_reduce_all(e)
            return
        L_ = e.spec.num_layers
        # sharded: no coalescing, one reduce-scatter + tail all-reduce per bucket; replicated: one all-reduce per group of buckets
        groups = None if self.sharded else self.exchange_groups(e)

        def exchange_bucket(b):
            if groups is not None and b not in groups:   # a bucket inside a coalesced group: exchanged with the group's last bucket
                return
            with torch.cuda.stream(self._comm_behind_main(e)):
                work = None                 # (`exchange` off, a dry run or a stream-ordered collective: nothing for step() to wait on)
                if self.exchange:
                    work = tx.reduce_scatter(e, b) if groups is None else tx.all_reduce(e, *groups[b])
                self._pending.append(work)

        e.backward_begin()
        exchange_bucket(0)
        for i in range(L_ - 1, -1, -1):
            e.backward_layer(i)
            exchange_bucket(L_ - i)
        e.backward_end()
        exchange_bucket(L_ + 1)

    def _comm_behind_main(self, e):
        """The side stream, made to wait for everything the current stream holds so far."""
        if self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(device=e.device)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._comm_stream.wait_event(ev)
        return self._comm_stream

    # -- sharded optimizer step (ZeRO stage 2)
    def _ensure_shard(self, e):
        # the plan belongs to the engine instance (a model that re-creates its engine for a larger batch gets it again; not a collective)
        if e.shard != (self.world, self.rank):
            e.shard_init(self.world, self.rank)

    def _sharded_update(self, e, lr, o, grad_scale):
        from . import _lib as L
        tx = pick_transport(self)
        e.shard_sqnorm_partials()
        tx.all_gather(e, L.SHARD_SLOTS)
        gn = e.adamw_step_sharded(lr, o.betas[0], o.betas[1], o.eps, o.weight_decay, o.max_grad_norm, grad_scale)
        # the bf16 weights: every rank's updated slices gathered on the side stream behind AdamW; the next reader of the weights waits
        with torch.cuda.stream(self._comm_behind_main(e)):
            tx.all_gather(e, L.SHARD_PARAMS)
            done = torch.cuda.Event()
            done.record(self._comm_stream)
        e._params_ready = done
        return gn

    def consolidate(self):
        """Collective (every rank calls it): after sharded steps, all-gather the fp32 master weights and the Adam moments so that every
        rank holds the whole optimizer state again (what DeepSpeed's zero_to_fp32 does offline) - and the weight EMA, which every rank
        averages over its share only.  Needed before module.state_dict(), save_checkpoint, Engine.sync_params, ema_weights and
        save_ema_checkpoint; a no-op when nothing is stale."""
        e = self.module._engine
        if e is None or not (e.shard_stale or e.ema_stale):
            return
        e.await_params()
        from . import _lib as L
        tx = pick_transport(self)
        if e.shard_stale:
            for what in (L.SHARD_MASTER, L.SHARD_ADAM_M, L.SHARD_ADAM_V):
                tx.all_gather(e, what)
            e.shard_stale = False
        if e.ema_stale:
            tx.all_gather(e, L.SHARD_EMA)
            e.ema_stale = False

    def exchange_groups(self, e) -> Dict[int, Any]:
        """{last bucket of a group: (offset, count)} - what one collective covers at this engine's `bucket_mb` (dp.exchange_groups)."""
        return exchange_groups(e.trainable_buckets() if getattr(e, "frozen", -1) >= 0 else e.buckets, self.bucket_mb)

    # -- the data-parallel launch menu, decided by measurement on the machine the job runs on
    def set_dp_menu(self, overlap: Optional[bool] = None, reserve_cus: Optional[int] = None):
        """Switch the exchange arrangement of a running engine: `overlap` = bucketed collectives beside the backward (True) or one
        collective behind it (False); `reserve_cus` = CUs the GEMM launch plans leave free for the collective's workgroups (the GEMM side
        of GGET_DP_RESERVE_CUS; the collective library's channel count is fixed when its communicator is created - dp_env_defaults)."""
        if overlap is not None:
            self.overlap = bool(overlap)
        if reserve_cus is not None:
            self.reserved_cus = max(0, int(reserve_cus))
            self.module.set_dp_menu(self.reserved_cus, self._dp_lds_headroom)

    def probe_dp_menu(self, step_fn: Callable[[], Any], steps: int = 10, warm: int = 2, menus=None) -> Dict[str, Any]:
        """No 1 -> 8 GPU curve of this engine has been measured: instead of a default chosen from a model, a
        multi-rank job TIMES the arrangements on its own machine at start-up and keeps the fastest - `steps` training steps each
        (after `warm`), max over ranks, the decision broadcast from rank 0 so that every rank takes the same.  `step_fn()` runs one
        step (forward + backward + step) on this rank.  The probe steps are ordinary training steps (the replicas stay identical).
        Returns {"menus": [...], "chosen": {...}}; a single-rank engine returns without measuring."""
        if self.world <= 1 or not dist_ready():
            return {"menus": [], "chosen": {"overlap": self.overlap, "reserve_cus": self.reserved_cus}, "probed": False}
        if menus is None:
            menus = [dict(overlap=True, reserve_cus=0), dict(overlap=False, reserve_cus=0), dict(overlap=True, reserve_cus=32)]
        dev = self.module.device if dist.get_backend(self.pg) == "nccl" else torch.device("cpu")
        rows = []
        for m in menus:
            self.set_dp_menu(**m)
            for _ in range(warm):
                step_fn()
            torch.cuda.synchronize()
            dist.barrier(self.pg)
            t0 = time.perf_counter()
            for _ in range(steps):
                step_fn()
            torch.cuda.synchronize()
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.pg)
            rows.append(dict(m, ms_per_step=float(t[0]) / steps * 1e3))
        best = min(range(len(rows)), key=lambda i: rows[i]["ms_per_step"])
        pick = torch.tensor([best], dtype=torch.int64, device=dev)
        dist.broadcast(pick, src=0, group=self.pg)
        chosen = menus[int(pick[0])]
        self.set_dp_menu(**chosen)
        return {"menus": rows, "chosen": dict(chosen), "probed": True, "steps_per_menu": steps}

    def describe_dp(self) -> Dict[str, Any]:
        """What the data-parallel exchange of this engine looks like (bench.py prints it on N > 1 lines)."""
        e = self.module._engine
        info = {"world": self.world, "backend": pick_transport(self).name,
                "n_buckets": len(e.buckets) if e is not None else None, "overlap_with_backward": bool(self.overlap),
                "reduce_dtype": "fp32" if self.fp32_reduce else "bf16",
                "bucket_mb": [round(c * 2 / 2 ** 20, 1) for _, c in e.buckets] if e is not None else None,
                "collectives_per_step": len(self.exchange_groups(e)) if e is not None else None,
                "collective_mb": [round(c * 2 / 2 ** 20, 1) for _, c in self.exchange_groups(e).values()] if e is not None else None,
                "reserved_cus": self.reserved_cus, "nccl_max_nchannels": os.environ.get("NCCL_MAX_NCHANNELS"),
                "zero_stage": self.zero_stage, "optimizer": "sharded" if self.sharded else "replicated"}
        if self.sharded and e is not None:
            # (GGET_DP_BUCKET_MB coalescing does not apply: one reduce-scatter + one tail all-reduce per bucket)
            from .engine import Engine
            plan = e.shard_buckets or Engine.shard_plan_of(e.cfg, self.world, len(e.buckets))
            info.update(bucket_coalescing="off (sharded step)", collective_mb=[round(p[1] * 2 / 2 ** 20, 1) for p in plan],
                        owned_elements={"body": sum(p[2] for p in plan), "tail": sum(p[4] for p in plan)},
                        collectives_per_step={"reduce_scatter": sum(1 for p in plan if p[2]), "all_reduce_tail": sum(1 for p in plan if p[4]),
                                              "all_gather_norm_partials": 1, "all_gather_params": sum(1 for p in plan if p[2])})
        try:
            v = torch.cuda.nccl.version()
            info["rccl_version"] = ".".join(str(x) for x in v) if isinstance(v, tuple) else str(v)
        except Exception:
            info["rccl_version"] = None
        return info

    def set_skip_nonfinite(self, on: bool):
        """The DDP branch's step rule (see __init__): the engine leaves weights / Adam state alone when the gradient norm is not finite
        (GGET_OPT_SKIP_NONFINITE_STEP); step() then takes Adam's step count back and counts the skipped step."""
        on = bool(on)
        e = self.module._engine
        if e is not None and getattr(e, "_skip_nonfinite", None) != on:
            from . import _lib as L
            e.set_option(L.OPT_SKIP_NONFINITE_STEP, int(on))
            e._skip_nonfinite = on
        self.skip_nonfinite = on

    # -- parameter groups (reference: torch parameter groups from loss_utils.py:370-412 handed to AdamW)
    def set_param_scales(self, lr_scale: Optional[Dict[str, float]] = None, wd_scale: Optional[Dict[str, float]] = None):
        """Per-parameter scales by state-dict name (a missing name takes 1.0, an unknown one raises); both None switches the groups off.
        Every step then runs parameter `name` at lr_at(step) * lr_scale[name] and weight_decay * wd_scale[name] (Engine.set_param_scales)."""
        if lr_scale is None and wd_scale is None:
            self._param_scales = None
        else:
            names = list(self.module._flat)
            for what, d in (("lr_scale", lr_scale or {}), ("wd_scale", wd_scale or {})):
                unknown = sorted(k for k in d if k not in self.module._flat)
                if unknown:
                    raise KeyError(f"set_param_scales: {what} names no parameter of this model: {unknown[:6]}")
            self._param_scales = ({n: float((lr_scale or {}).get(n, 1.0)) for n in names}, {n: float((wd_scale or {}).get(n, 1.0)) for n in names})
        e = self.module._engine
        if e is not None:
            self._apply_param_scales(e)

    def _apply_param_scales(self, e):
        e.set_param_scales(*(self._param_scales or (None, None)))
        e._param_scales_from = self._param_scales

    def set_param_groups(self, groups, rest_lr_scale: Optional[float] = None):
        """torch-style parameter groups.  Every group is a dict: "params" = Parameters of the module or state-dict names (any iterable);
        "lr" (absolute, divided by optim.lr) or "lr_scale"; "weight_decay" (absolute, divided by optim.weight_decay) or "wd_scale" -
        all optional, default scale 1.  Every group follows the one schedule shape: lr_at(step) times its scale.  A parameter in two
        groups raises.  A parameter in no group raises with the names - torch would silently never train it - unless `rest_lr_scale`
        is given: those parameters then run at that scale (0.0 = torch's behaviour, said out loud)."""
        o = self.optim
        name_of = {id(p): n for n, p in self.module._flat.items()}
        lr_s, wd_s, twice = {}, {}, []
        for gi, g in enumerate(groups):
            if ("lr" in g and "lr_scale" in g) or ("weight_decay" in g and "wd_scale" in g):
                raise ValueError(f"set_param_groups: group {gi} gives both an absolute value and a scale")
            ls = float(g["lr"]) / float(o.lr) if "lr" in g else float(g.get("lr_scale", 1.0))
            if "weight_decay" in g:
                if float(o.weight_decay) == 0.0 and float(g["weight_decay"]) != 0.0:
                    raise ValueError(f"set_param_groups: group {gi} asks for weight_decay {g['weight_decay']} but optim.weight_decay is 0 "
                                     "(the group's value is a scale of it)")
                ws = float(g["weight_decay"]) / float(o.weight_decay) if float(o.weight_decay) != 0.0 else 1.0
            else:
                ws = float(g.get("wd_scale", 1.0))
            for p in ([g["params"]] if isinstance(g["params"], (str, torch.Tensor)) else list(g["params"])):
                n = p if isinstance(p, str) else name_of.get(id(p))
                if n is None or n not in self.module._flat:
                    raise KeyError(f"set_param_groups: group {gi} holds {'a tensor that is' if n is None else repr(n) + ','} no parameter of this model")
                if n in lr_s:
                    twice.append(n)
                lr_s[n], wd_s[n] = ls, ws
        if twice:
            raise ValueError(f"set_param_groups: some parameters appear in more than one parameter group: {twice}")
        rest = [n for n in self.module._flat if n not in lr_s]
        if rest and rest_lr_scale is None:
            raise ValueError(f"set_param_groups: {len(rest)} parameters are in no group and would never train: {rest}; put them in a group "
                             "or pass rest_lr_scale (0.0 = leave them untrained on purpose)")
        for n in rest:
            lr_s[n], wd_s[n] = float(rest_lr_scale), 1.0
        self.set_param_scales(lr_s, wd_s)

    @property
    def last_lrs(self) -> Dict[str, float]:
        """State-dict name -> learning rate of the last step: lr_at(step) times the parameter's scale."""
        lr = getattr(self, "last_lr", None)         # (set by the first step)
        if lr is None:
            return {}
        lr_s = self._param_scales[0] if self._param_scales is not None else {}
        return {n: lr * lr_s.get(n, 1.0) for n in self.module._flat}

    # -- weight EMA (reference: EMAStats + timm ModelEmaV3, src/conf/stats_configs.py:102-146, src/utils/patch_utils.py:5-42)
    def ema_decay_at(self, step: int) -> float:
        """The decay of the update made when `step` loop iterations were done before it (the reference passes `train_stats.j`,
        finetune_mode.py:413 / pretrain_mode.py:460).  timm's `ModelEmaV3.get_decay` with the defaults the reference constructs it with
        (`update_after_step = 0`, `use_warmup = False`): 0.0 while step - 1 <= 0, the configured decay afterwards - the first two updates
        copy the weights, from the third on it averages.  timm is a third-party dependency that is not installed here: the rule is
        RESTATED from its published source and UNPINNED (no run of timm itself was available to check it against), like DeepSpeed's
        WarmupDecayLR."""
        return 0.0 if int(step) - 1 <= 0 else float(self.optim.ema_decay)

    def _ema_engine(self, what: str):
        e = self.module._engine
        if e is None or e.ema is None or not e.ema_live:
            raise RuntimeError(f"{what}: this engine holds no weight EMA (OptimConfig(use_ema=True) and at least one step, or load_ema_checkpoint)")
        if e.shard_stale or e.ema_stale:
            raise RuntimeError(f"{what}: the optimizer state is partitioned after a sharded (ZeRO-2) step; call engine.consolidate() "
                               "on every rank before saving")
        return e

    def _ema_next_decay(self, e) -> float:
        """Attach + seed on first use (ModelEmaV3.__init__ deep-copies the model: the d = 0 update), then the decay of this update."""
        if e.ema is None or not e.ema_live:
            e.ema_attach()
            e.ema_update(0.0)
        d = self.ema_decay_at(self.ema_updates)
        self.ema_updates += 1
        return d

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block every forward of `engine.module` runs on the averaged weights (the bf16 compute copy is rewritten from the
        EMA arena); on exit the live weights are back.  This is `ft_evaluate(ema_stats.model_ema, ...)` of the reference
        (log_eval_dump_utils.py:720-793) without a second model.  `step()` inside the block raises: it would rewrite the bf16 copy
        from the live weights and the rest of the block would silently evaluate those."""
        e = self._ema_engine("ema_weights")
        if self.module._dirty:          # (an external write of the master weights is still owed to the bf16 copy: it must not land inside the block)
            e.sync_params()
            self.module._dirty = False
        e.ema_to_params()
        try:
            yield self.module
        finally:
            self.module._engine.sync_params()       # (the model may have re-created its engine for a larger batch inside the block)

    def ema_state_dict(self):
        """The averaged weights in the module's reference shapes (what `get_state_dict(model_ema, unwrap_model)` returns there)."""
        e = self._ema_engine("ema_state_dict")
        return e.ema_state_dict({k: tuple(p.shape) for k, p in self.module._flat.items()})

    def save_ema_checkpoint(self, output_dir: str, best: bool = False):
        """`EMAStats.save_ema_ckp` (stats_configs.py:138-146): model_ema.pt - and model_ema_best.pt when `best` - as a plain state dict."""
        from . import checkpoint as CK
        self._ema_engine("save_ema_checkpoint")
        return CK.save_ema_state_dict(self.ema_state_dict(), output_dir, best=best)

    def load_ema_checkpoint(self, output_dir: str):
        """`EMAStats.load_ema_ckp` (stats_configs.py:125-129): <output_dir>/model_ema.pt into the EMA arena."""
        from . import checkpoint as CK
        e = self.module._engine
        if e is None:
            e = self.module._ensure_engine(1, 8)
        path = os.path.join(output_dir, CK.EMA_NAME)
        e.load_ema_state_dict(CK.read_state_dict(path))
        return path

    def step(self):
        """One `engine.step()` of the reference's loop.  With `gradient_accumulation_steps = k > 1` (DeepSpeed branch) the call is made
        after every micro-batch like there, and like the DS engine only every k-th call updates the weights: the others add the
        micro-batch's (exchanged) gradient to the engine's fp32 accumulator (one launch, the first of a window overwrites) and return
        None; at the boundary the norm, the clip and AdamW read that fp32 sum - it is never rounded back to bf16 - with 1 / (world * k),
        the mean over the k * world micro-batches; clip and LR schedule once per update, and the update closes the window.
        With `optim.use_ema` every call averages, as the reference calls `update_ema` after every batch: inside the AdamW launch at an
        update (also when the skip rule drops it), by the stand-alone lerp on the other micro-steps."""
        e = self.module._engine
        if e is not None and e._params_are_ema:
            raise RuntimeError("step() inside ema_weights(): the bf16 weights are the averaged ones (the gradients were taken on them, and "
                               "the update would put the live weights back for the rest of the block); leave the block before training")
        if self._pending:
            for w in self._pending:
                if w is not None:
                    w.wait()  # makes the current stream wait for the comm stream's collectives
            self._pending = []
            torch.cuda.current_stream().wait_stream(self._comm_stream)
        o = self.optim
        k = getattr(o, "gradient_accumulation_steps", 1)
        ema_decay = None
        if getattr(o, "use_ema", False):
            if self.sharded:
                self._ensure_shard(e)       # (the seed and the stand-alone lerp run over this rank's share)
            ema_decay = self._ema_next_decay(e)
        if k > 1:
            e.grad_accumulate()         # (attaches the arena on first use; a re-created engine carries an open window over)
            self._grad_acc = e.grad_acc
            self.micro_steps += 1
            if self.micro_steps % k != 0:
                if ema_decay is not None:
                    e.ema_update(ema_decay)
                return None
        lr = o.lr_at(self.global_steps)
        if self.skip_nonfinite and getattr(e, "_skip_nonfinite", None) is not True:
            self.set_skip_nonfinite(True)       # (the model re-created its engine: the option lives on the engine instance)
        if getattr(e, "_param_scales_from", None) is not self._param_scales:
            self._apply_param_scales(e)         # (the same for the parameter groups)
        if ema_decay is not None:
            e.set_ema_decay(ema_decay)
        if self.sharded:
            self._ensure_shard(e)
            gn = self._sharded_update(e, lr, o, 1.0 / (self.world * k))
        else:
            gn = e.adamw_step(lr, o.betas[0], o.betas[1], o.eps, o.weight_decay, o.max_grad_norm, 1.0 / (self.world * k))
        self.global_steps += 1
        self.last_lr, self.last_grad_norm = lr, gn
        if self.skip_nonfinite and not bool(torch.isfinite(gn)):   # (GradScaler.step reads found_inf back as well: one sync per step on this branch)
            e.step_count -= 1                   # optimizer.step() did not run; lr_scheduler.step() did (global_steps stays advanced)
            self.skipped_steps += 1
        return gn

    # -- checkpoint = reference DDP layout (misc_utils.py:105-121): model.pt / optimizer.pt keyed by state-dict names
    def save_checkpoint(self, save_dir: str, tag: Optional[str] = None):
        e = self.module._engine
        if e is not None and (e.shard_stale or e.ema_stale):     # (no collective here: the pipeline saves on rank 0 only; it consolidates on every rank first)
            raise RuntimeError("save_checkpoint: the optimizer state is partitioned after a sharded (ZeRO-2) step; call engine.consolidate() "
                               "on every rank before saving")
        if e is not None:
            e.await_params()
        d = os.path.join(save_dir, tag) if tag else save_dir
        os.makedirs(d, exist_ok=True)
        from . import checkpoint as CK
        # the MODULE's state dict: reference shapes (emb_mask_token is [1,1,embed_dim] there, flat in the engine arena)
        torch.save({k: v.detach().cpu().clone() for k, v in self.module.state_dict().items()}, os.path.join(d, "model.pt"))
        # (a checkpoint inside an accumulation window carries the partial fp32 sum: checkpoint.optimizer_state)
        window = e.grad_acc is not None and e.grad_acc_count() > 0
        torch.save(CK.optimizer_state({k: e.view(k, "m").cpu() for k in e.params}, {k: e.view(k, "v").cpu() for k in e.params},
                                      e.step_count, self.global_steps, self.ema_updates, self.micro_steps,
                                      {k: e.view(k, "grad_acc").cpu() for k in e.params} if window else None),
                   os.path.join(d, "optimizer.pt"))
        if e.ema is not None and e.ema_live:        # the average travels with the checkpoint: a resumed run continues it (pipeline.py:202)
            self.save_ema_checkpoint(d)
        self.module.config.save_pretrained(d)

    def load_checkpoint(self, load_dir: str, tag: Optional[str] = None):
        d = os.path.join(load_dir, tag) if tag else load_dir
        e = self.module._engine
        if e is None:
            e = self.module._ensure_engine(1, 8)
        from . import checkpoint as CK
        e.load_state_dict(torch.load(os.path.join(d, "model.pt"), map_location="cpu"))
        opt_path = os.path.join(d, "optimizer.pt")
        if os.path.exists(opt_path):
            st = torch.load(opt_path, map_location="cpu")
            for k in e.params:
                e.view(k, "m").copy_(st["m"][k].to(e.device))
                e.view(k, "v").copy_(st["v"][k].to(e.device))
            e.step_count = int(st["step"])
            self.global_steps = int(st["global_steps"])
            self.ema_updates = int(st.get("ema_updates", 0))
            e.shard_stale = False       # (every arena was written in full)
            # an open accumulation window continues where it was: the partial sum back into the arena, the count back into the engine
            self.micro_steps, acc, n = CK.read_accumulation(st, getattr(self.optim, "gradient_accumulation_steps", 1), list(e.params))
            if acc is not None:
                e.grad_acc_attach().zero_()
                for k in e.params:
                    e.view(k, "grad_acc").copy_(acc[k].to(e.device))
                self._grad_acc = e.grad_acc
            e.grad_acc_set_count(n)
        # (a run that does not average leaves a model_ema.pt it finds alone: no arena, nothing carried into its next save)
        if getattr(self.optim, "use_ema", False) and os.path.exists(os.path.join(d, CK.EMA_NAME)):
            self.load_ema_checkpoint(d)
        return d, {}


def initialize(model: _GgetModel, optim: Optional[OptimConfig] = None, process_group=None) -> GgetEngine:
    eng = GgetEngine(model, optim, process_group)
    o = eng.optim
    decay, no_decay = getattr(o, "layerwise_lr_decay", None), getattr(o, "no_decay_1d", False)
    if decay is not None or no_decay:
        lr_s = layerwise_lr_scales(model, decay, getattr(o, "layerwise_lr_version", 1)) if decay is not None else {}
        wd_s = {n: 0.0 for n, p in model._flat.items() if p.ndim == 1} if no_decay else {}
        eng.set_param_scales(lr_s, wd_s)
    return eng


# ----------------------------------------------------------------------------- one optimisation step
def _reference_step_args(model, train_cfg, train_stats):
    """The reference's positional form `batch_training(data, model, train_cfg, train_stats, opt_stats)` (training_utils.py:7-13):
    `model` is the engine `deepspeed.initialize` returned, `train_stats` carries `.device`, `.has_embeds_input`, `.use_deepspeed`."""
    return getattr(train_stats, "device", None) or model.device, bool(getattr(train_stats, "has_embeds_input", False))


def _reference_optimizer_step(model, train_cfg, train_stats, loss):
    """backward + optimizer step of the reference's two branches on the engine.
    DeepSpeed branch (training_utils.py:44-45): model.backward(loss); model.step().
    DDP branch (`train_stats.use_deepspeed` False, :46-86): zero_grad; fp16 autocast forward; scaler.scale(loss).backward();
    scaler.unscale_; clip_grad_norm_(max_grad_norm); scaler.step (SKIPPED when a gradient is inf / NaN); scaler.update; lr_scheduler.step().
    On this engine the forward / backward arithmetic is bf16 with fp32 accumulation whatever the branch (fp16 autocast is not reproduced:
    bf16 has fp32's exponent range, so the loss scale is 1 and never changes); what the branch changes is the step rule - GradScaler's
    skip of a non-finite step (GGET_OPT_SKIP_NONFINITE_STEP: weights and Adam state untouched, Adam's step count not advanced) while the
    LR schedule still advances, and `optimizer.gradient_accumulation_steps` must be 1 (the reference asserts it, :47-49)."""
    ddp = not getattr(train_stats, "use_deepspeed", True)
    if model.skip_nonfinite != ddp:
        model.set_skip_nonfinite(ddp)       # (the rule itself - Adam's step count taken back, the skipped-steps counter - lives in GgetEngine.step)
    if ddp:
        oc = getattr(train_cfg, "optimizer", None)
        assert oc is None or getattr(oc, "gradient_accumulation_steps", 1) == 1, \
            "https://pytorch.org/docs/stable/notes/amp_examples.html#gradient-accumulation"
    model.backward(loss)
    return model.step()


def batch_training(data: Dict[str, torch.Tensor], engine: GgetEngine, train_cfg=None, train_stats=None, opt_stats=None):
    """reference training_utils.batch_training DeepSpeed branch (:30-45): loss = head1 (+head2); backward; step.
    position_ids are NOT passed in pre-training (reference comments them out at :35).

    Two call forms.  `batch_training(data, engine)`: host tensors go to the engine as they are; `data["num_tokens"]` (optional host
    int = sum of the attention mask) or the host-side mask itself gives the var-len layout its row count for free.
    `batch_training(data, model, train_cfg, train_stats, opt_stats)` - the reference's own signature (training_utils.py:7-13): every
    tensor is moved to `train_stats.device` first, exactly like :17-26, the model sees device tensors only (the engine then counts
    the mask on the device), and the losses / shapes are recorded on `train_stats` like :87-95."""
    if train_stats is None:
        out = engine(input_ids=data["input_ids"], attention_mask=data["attention_mask"], labels=data["labels"],
                     inputs_raw_embeds=data.get("embed"), sample_wgt=data.get("wgt"), num_tokens=data.get("num_tokens"))
        loss = out.head1_loss
        if out.head2_loss is not None:
            loss = loss + out.head2_loss
        engine.backward(loss)
        engine.step()
        return loss
    model = engine
    device, has_embeds = _reference_step_args(model, train_cfg, train_stats)
    input_ids = data["input_ids"].to(device)
    attention_mask = data["attention_mask"].to(device)
    labels = data["labels"].to(device)
    inputs_raw_embeds = data["embed"].to(device) if has_embeds else None
    sample_wgt = data["wgt"].to(device) if "wgt" in data else None
    output = model(input_ids=input_ids, attention_mask=attention_mask, labels=labels, inputs_raw_embeds=inputs_raw_embeds,
                   sample_wgt=sample_wgt)
    main_loss, aux_loss = output.head1_loss, output.head2_loss
    loss = main_loss + aux_loss if aux_loss is not None else main_loss
    _reference_optimizer_step(model, train_cfg, train_stats, loss)
    train_stats.loss, train_stats.main_loss, train_stats.aux_loss = loss, main_loss, aux_loss
    train_stats.inputs_shape = input_ids.shape
    train_stats.sliced_raw_embeds = inputs_raw_embeds[:2, :8] if inputs_raw_embeds is not None else None
    return loss


def ft_batch_training(data: Dict[str, torch.Tensor], engine: GgetEngine, *ref_args, label_key: str = "task_labels"):
    """reference training_utils.ft_batch_training (:98-205): passes position_ids, task labels, sample weights.
    `ft_batch_training(data, engine[, label_key=])` or the reference's positional form
    `ft_batch_training(data, model, fthead_cfg, train_cfg, train_stats, opt_stats)` (tensors moved to the device first, :114-133;
    `fthead_cfg.task_type` names the label key, multi-label targets become float, the losses are recorded on `train_stats`)."""
    if not ref_args:
        out = engine(input_ids=data["input_ids"], attention_mask=data["attention_mask"], position_ids=data.get("position_ids"),
                     task_labels=data[label_key], cls_idx=data.get("cls_idx"), inputs_raw_embeds=data.get("embed"),
                     sample_wgt=data.get("wgt"), num_tokens=data.get("num_tokens"))
        loss = out.task_loss
        engine.backward(loss)
        engine.step()
        return loss, out.task_logits
    if len(ref_args) != 4:
        raise TypeError("ft_batch_training(data, model, fthead_cfg, train_cfg, train_stats, opt_stats)")
    fthead_cfg, train_cfg, train_stats, _opt_stats = ref_args
    model = engine
    device, has_embeds = _reference_step_args(model, train_cfg, train_stats)
    if getattr(getattr(train_cfg, "finetune", None), "use_aux", False):
        raise NotImplementedError("finetune.use_aux (the double-heads fine-tune model) is outside the hot-path scope")
    task_labels = data[f"{fthead_cfg.task_type}_labels"].to(device)
    if fthead_cfg.problem_type == "multi_label_classification":
        task_labels = task_labels.float()
    output = model(input_ids=data["input_ids"].to(device), attention_mask=data["attention_mask"].to(device), pretrain_labels=None,
                   task_labels=task_labels, cls_idx=data["cls_idx"].to(device) if "cls_idx" in data else None,
                   inputs_raw_embeds=data["embed"].to(device) if has_embeds else None,
                   sample_wgt=data["wgt"].to(device) if "wgt" in data else None, position_ids=data["position_ids"].to(device))
    task_loss = output.task_loss
    loss = task_loss.float()
    _reference_optimizer_step(model, train_cfg, train_stats, loss)
    train_stats.loss, train_stats.main_loss, train_stats.aux_loss = loss, task_loss, None
    return loss, output.task_logits


def _host_token_count(data) -> Optional[int]:
    """Real tokens of a collated batch when that is free to know: `data["num_tokens"]`, or the sum of a HOST-side 2-D attention mask (the
    evaluation loops receive CPU batches and move them: counting before the move costs nothing) - lets the engine run the batch on the
    padding-free token layout (modeling._GgetModel._token_count).  None = unknown (device-side mask): padded layout."""
    if data.get("num_tokens") is not None:
        return int(data["num_tokens"])
    am = data.get("attention_mask")
    if am is not None and am.dim() == 2 and am.device.type == "cpu":
        return int((am != 0).sum())
    return None


def _layout_kw(model, data) -> Dict[str, Any]:
    """`num_tokens=` for the engine-backed model classes only (the reference's call keeps its exact keyword set for any other model)."""
    n = _host_token_count(data) if isinstance(getattr(model, "module", model), _GgetModel) else None
    return {} if n is None else {"num_tokens": n}


# ----------------------------------------------------------------------------- batch hand-over (host -> device)
class DevicePrefetcher:
    """The reference's step moves every tensor of the batch to the device at its top (training_utils.py:17-26, `.to(device)` on pageable
    DataLoader output: a synchronous staging copy per tensor in front of the forward).  Here the host half of the hand-over of batch
    t + 1 runs DURING step t: the collated batch is copied into pinned staging buffers one batch ahead (three sets, used in turn), and
    the device half is one copy kernel per tensor from the pinned buffer into persistent device buffers, enqueued on the COMPUTE stream
    right in front of the step that reads them (1.8 MB for a C1 batch: ~35 us of a 6.7 ms step) - stream order alone keeps a device set
    from being overwritten before the step that read it has run; one event per pinned set tells the host when it may refill it.
    What comes out is the same dict with device tensors plus `num_tokens` = the host-side sum of a 2-D attention mask (free here, and
    what lets the engine run the padding-free layout without reading a count back).  `batch_training(data, model, train_cfg,
    train_stats, ...)` - the reference's form - sees tensors that are already on `train_stats.device`: its `.to(device)` calls return
    them as they are.

        for data in DevicePrefetcher(loader, device):
            batch_training(data, engine)

    The device tensors of a batch are reused for the batch three steps later: consume them inside the step (as the training step does).
    Measured (tools/prefetch_probe.py, C1 step, one box): device-resident batches 6.80 ms, this class 6.87 ms (+0.9 %), the reference's
    synchronous `.cuda()` per tensor 6.95 ms (+2.2 %).  Two traps on the way there: (1) `pinned.copy_(pageable)` - torch's copy_ INTO a
    pinned tensor synchronises with the device (3 ms on average, up to 94 ms under load): the staging buffers are filled through their
    numpy views (14 us); (2) the device half as hipMemcpyAsync (`dst.copy_(pinned, non_blocking=True)`) is a copy-engine job, 6.92 ms: the
    kernel form (gget_op_copy_from_host reads the pinned buffer over the host link) stays in the compute queue.
    Non-tensor entries pass through; tensors already on the device are left alone."""

    SETS = 3

    def __init__(self, batches: Iterable, device=None, count_tokens: bool = True):
        self.batches = batches
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.count_tokens = count_tokens
        self._pinned = [dict() for _ in range(self.SETS)]        # key -> pinned host tensor
        self._dev = [dict() for _ in range(self.SETS)]           # key -> device tensor
        self._copied = [None] * self.SETS                        # compute-stream event behind the set's last pinned -> device copies

    def __len__(self):
        return len(self.batches)

    def _stage(self, data, slot):
        """host half: the batch into pinned set `slot` (+ the token count)"""
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()     # (the device copy that last read this pinned set: three steps old)
            self._copied[slot] = None
        out, pend = {}, []
        for k, v in data.items():
            if not torch.is_tensor(v) or v.device == self.device:
                out[k] = v
                continue
            buf = self._pinned[slot].get(k)
            if buf is None or buf.shape != v.shape or buf.dtype != v.dtype:
                buf = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
                self._pinned[slot][k] = buf
                self._dev[slot][k] = torch.empty(v.shape, dtype=v.dtype, device=self.device)
            # (NOT buf.copy_(v): torch's copy_ into a pinned tensor synchronises with the device - 3 ms on average, up to 94 ms with the
            #  GPU busy, against 14 us for the same bytes through the buffers' numpy views; that alone took the C1 step from 6.7 to 10 - 20 ms)
            np.copyto(buf.view(torch.uint8).numpy(), v.contiguous().view(torch.uint8).numpy())
            pend.append(k)
        if self.count_tokens and "num_tokens" not in out:
            am = data.get("attention_mask")
            if torch.is_tensor(am) and am.dim() == 2 and am.device.type == "cpu":
                out["num_tokens"] = int((am != 0).sum())
        return out, pend, slot

    def _to_device(self, staged):
        """device half, on the current (compute) stream, in front of the step"""
        out, pend, slot = staged
        if pend:
            import ctypes as C
            from . import _lib as L
            lib, st = L.load(), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        for k in pend:
            src, dst = self._pinned[slot][k], self._dev[slot][k]
            if os.environ.get("GGET_PF_COPY", "kernel") == "kernel":      # (memcpy: the copy-engine form, kept for tools/prefetch_probe.py)
                L.check(lib.gget_op_copy_from_host(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), src.numel() * src.element_size(), st))
            else:
                dst.copy_(src, non_blocking=True)
            out[k] = dst
        if pend:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._copied[slot] = ev
        return out

    def __iter__(self):
        it = iter(self.batches)
        try:
            cur = self._stage(next(it), 0)
        except StopIteration:
            return
        slot = 1
        data = self._to_device(cur)
        while cur is not None:
            try:
                nxt = self._stage(next(it), slot)       # the host half of the NEXT batch, before the consumer's step on this one is enqueued
            except StopIteration:
                nxt = None
            slot = (slot + 1) % self.SETS
            yield data
            # (the device half on a side stream, joined by an event, so that it runs beside the step: 6.88 ms against 6.74 - the fork / join
            #  packets cost more than the 35 us of copy they hide, as with the attention launches, profiles/r06_step_experiments.txt)
            data = self._to_device(nxt) if nxt is not None else None
            cur = nxt


# ----------------------------------------------------------------------------- evaluation pass
@torch.no_grad()
def evaluate(model, loader, eval_name: str = "valid", do_eval: bool = True):
    """Pre-train evaluation pass, reference log_eval_dump_utils.evaluate (:242-304): eval mode, one forward per batch with
    labels and sample weights but WITHOUT position_ids (the reference comments them out), head1 loss sum-reduced to rank 0
    and divided by the world size there, mean over the batches; returns (loss, None) and puts the model back in train mode.
    `do_eval=False` returns (None, None)."""
    if not do_eval:
        return None, None
    world = dist.get_world_size() if dist_ready() else 1
    rank = dist.get_rank() if world > 1 else 0
    model.eval()
    device = model.device
    losses, aux_losses = [], []
    for data in loader:
        out = model(input_ids=data["input_ids"].to(device), attention_mask=data["attention_mask"].to(device),
                    labels=data["labels"].to(device),
                    inputs_raw_embeds=data["embed"].to(device) if "embed" in data else None,     # log_eval_dump_utils.py:53-59
                    sample_wgt=data["wgt"].to(device) if "wgt" in data else None, **_layout_kw(model, data))
        loss, aux = out.head1_loss.clone(), out.head2_loss
        if world > 1:
            dist.reduce(loss, 0)
            if aux is not None:
                aux = aux.clone()
                dist.reduce(aux, 0)
            if rank == 0:
                loss = loss / world
                aux = aux / world if aux is not None else None
        losses.append(loss)
        if aux is not None and not torch.isnan(aux).item():
            aux_losses.append(aux)
    model.train()
    _check_deferred_all_ranks(model)
    if not losses:
        raise ValueError(f"evaluate: the {eval_name} loader yielded no batch")
    return sum(losses) / len(losses), None


def _check_deferred_all_ranks(model):
    """`model.check_deferred()` so that EVERY rank raises when any rank's device-side input guard fired: a single rank raising in
    front of a collective would leave the others blocked in it.  The flag is max-reduced over the default group."""
    m = getattr(model, "module", model)
    if not hasattr(m, "check_deferred"):
        return
    err = None
    try:
        m.check_deferred()
    except (IndexError, ValueError) as ex:
        err = ex
    if dist_ready() and dist.get_world_size() > 1:
        dev = m.device if dist.get_backend() == "nccl" else torch.device("cpu")
        flag = torch.tensor([1 if err is not None else 0], device=dev, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if err is None and int(flag.item()):
            err = RuntimeError("another rank's device-side input guard fired (position_ids outside the RoPE table or a var-len token "
                               "count mismatch): see that rank's error")
    if err is not None:
        raise err


@torch.no_grad()
def ft_evaluate(model, loader, *, problem_type: str = "single_label_classification", num_labels: int = 2,
                task_level: str = "task", metric_type: Optional[str] = None, dataset_name: str = "", eval_name: str = "valid",
                cnt_neg: int = 1000):
    """Fine-tune evaluation pass, reference log_eval_dump_utils.ft_evaluate (:77-163): eval mode; per batch one forward WITH
    task labels, sample weights and position_ids; the task loss is averaged over the batches, logits feed the metric object
    (`update(task_logits, labels, idx)`); with several ranks every entry of the metric's tensor dict is gathered from all
    ranks (variable length); the dataset's OGB-style evaluator runs on the gathered dict when there is one, otherwise the
    metric object's own results are returned.  Returns (loss, metrics, eval_result, input_dict) like the reference; the
    keyword arguments replace the fields the reference reads from its Hydra config (`cnt_neg`: the negatives per positive of the
    ogbl-citation2 / ogbl-wikikg2 evaluators, 1000 in the reference).  A two-class single-label problem on a GPU keeps its
    accumulations on the device, ranks there (metrics.link_hits / link_mrr / rank_metrics) and copies the tensor dict to the host once,
    after the metrics; ogbl-citation2 / ogbl-wikikg2 are not ranked for eval_name == "train" (reference :153-160): the metric
    object's own results are returned then.  A batch with a "raw_node_idx" column (token-level heads, metric_type
    "graph_clustering") hands `(idx, raw_node_idx)` to `update`, as the reference does (:130-131)."""
    from . import metrics as M
    model.eval()
    device = model.device
    on_device = (torch.device(device).type == "cuda" and num_labels == 2
                 and (metric_type or problem_type) == "single_label_classification")
    cls_metrics = M.get_metrics(metric_type or problem_type, device, num_labels=num_labels, on_device=on_device)
    test_loss, j = 0, 0
    for j, data in enumerate(loader, 1):
        labels = data[f"{task_level}_labels"].to(device)
        labels = labels.float() if problem_type == "multi_label_classification" else labels
        res = model(input_ids=data["input_ids"].to(device), attention_mask=data["attention_mask"].to(device),
                    task_labels=labels, cls_idx=data["cls_idx"].to(device) if "cls_idx" in data else None,
                    inputs_raw_embeds=data["embed"].to(device) if "embed" in data else None,     # log_eval_dump_utils.py:108-110
                    sample_wgt=data["wgt"].to(device) if "wgt" in data else None, **_layout_kw(model, data),
                    position_ids=data["position_ids"].to(device) if "position_ids" in data else None)
        test_loss = test_loss + res.task_loss.detach()
        idx = data["idx"].to(device) if "idx" in data else torch.arange(labels.shape[0], device=device) + (j - 1) * labels.shape[0]
        if "raw_node_idx" in data:        # the nodev2 collator's column: the clustering metric takes (idx, raw_node_idx), log_eval_dump_utils.py:130-131
            idx = (idx, data["raw_node_idx"].to(device))
        cls_metrics.update(res.task_logits, labels, idx)
    model.train()
    _check_deferred_all_ranks(model)      # (a collective itself: every rank raises together, none is left inside the gathers below)
    if j == 0:
        raise ValueError(f"ft_evaluate: the {eval_name} loader yielded no batch")
    test_loss = test_loss / j
    input_dict = cls_metrics.to_dict()
    world = dist.get_world_size() if dist_ready() else 1
    ranked = not (eval_name == "train" and dataset_name in M.MRR_DATASETS)
    ogb = lambda d: M.evaluate_ogb(dataset_name, d, cnt_neg=cnt_neg) if ranked else None      # noqa: E731
    if on_device:
        # as the multi-label branch below: metrics from the device-resident accumulations, then the ONE host transfer of the tensor dict
        sync = cls_metrics.sync_dict()
        if world > 1:
            gdev = device if dist.get_backend() == "nccl" else torch.device("cpu")
            input_dict = {k: all_gather_varlen(v.to(gdev)) for k, v in input_dict.items()}
            sync = dict(input_dict, prob=all_gather_varlen(sync["prob"].to(gdev)))
        cls_metrics.compute(sync)
        res = ogb(input_dict)
        if res is None:
            res = cls_metrics.results_in_dict()
        return test_loss, cls_metrics, res, {k: v.cpu() for k, v in input_dict.items()}
    if isinstance(cls_metrics, M.GraphClusteringMetrics):
        # as the multi-label branch below: per-sample counts and totals were taken on the device batch by batch (metrics.cluster_metrics);
        # compute() makes their one host transfer, the tensor dict follows in one copy at the end
        sync = cls_metrics.sync_dict()
        if world > 1:
            gdev = device if dist.get_backend() == "nccl" else torch.device("cpu")
            input_dict = {k: all_gather_varlen(v.to(gdev)) for k, v in input_dict.items()}
            sync = {k: all_gather_varlen(v.to(gdev)) for k, v in sync.items()}
        cls_metrics.compute(sync)
        res = M.evaluate_ogb(dataset_name, input_dict)
        if res is None:
            res = cls_metrics.results_in_dict()
        return test_loss, cls_metrics, res, {k: v.cpu() for k, v in input_dict.items()}
    if isinstance(cls_metrics, M.MultiLabelClassificationMetrics):
        # rank metrics from the device-resident accumulations (the gathered tensors on the collective's device with several ranks): the HIP
        # rank kernels for CUDA tensors; the ONE host transfer of the tensor dict comes after them
        if world > 1:
            gdev = device if dist.get_backend() == "nccl" else torch.device("cpu")
            input_dict = {k: all_gather_varlen(v.to(gdev)) for k, v in input_dict.items()}
        cls_metrics.compute(input_dict)
        res = M.evaluate_ogb(dataset_name, input_dict)
        if res is None:
            res = cls_metrics.results_in_dict()
        return test_loss, cls_metrics, res, {k: v.cpu() for k, v in input_dict.items()}
    if world > 1:
        gdev = device if dist.get_backend() == "nccl" else torch.device("cpu")
        input_dict = {k: all_gather_varlen(v.to(gdev)).cpu() for k, v in input_dict.items()}
        # the reference's torchmetrics objects synchronise across ranks inside compute(): feed ours the gathered lists
        cls_metrics.compute({k: all_gather_varlen(v.to(gdev)).cpu().numpy() for k, v in cls_metrics.sync_dict().items()})
    else:
        cls_metrics.compute()
    res = ogb({k: v.numpy() for k, v in input_dict.items()})
    if res is None:
        res = cls_metrics.results_in_dict()
    return test_loss, cls_metrics, res, input_dict


def _format_eval_res(eval_res, rnd: int = 6):
    """reference `format_ogb_output_for_csv` (ogb_utils.py:207-213): "key,value" pairs of a result dict, values rounded to 6 places."""
    if isinstance(eval_res, dict):
        return ",".join(f"{k},{round(v, rnd)}" for k, v in eval_res.items())
    return eval_res


# ----------------------------------------------------------------------------- pipeline
class TrainingMode(abc.ABC):
    """Strategy interface of the reference (src/training/mode.py:46-89).  The dataset / tokenizer / sampler halves of
    `prepare_data` stay on the host: a mode is constructed with what they would have produced -
    `batches` (an iterable of collated batches), and for a reference-shaped `Config` the figures the schedule arithmetic
    needs (`tokens_per_sample`, `samples_per_gpu`, `vocab_size` ...)."""

    model_cls = GraphGPTPretrainBase
    skip_keys = False                      # (mode.py: fine-tuning drops the `score` head of a pre-trained checkpoint)
    finetune = False

    def __init__(self, batches: Optional[Iterable] = None, tokens_per_sample: Optional[float] = None,
                 samples_per_gpu: Optional[int] = None, vocab_size: Optional[int] = None, bos_token_id: Optional[int] = None,
                 eos_token_id: Optional[int] = None, mask_inside_model: bool = False):
        self.batches, self.tokens_per_sample, self.samples_per_gpu = batches, tokens_per_sample, samples_per_gpu
        self.vocab_size, self.bos_token_id, self.eos_token_id = vocab_size, bos_token_id, eos_token_id
        # the tokenizer configuration's `pretrain_mlm.method == "inside_model"` (pretrain_mode.py:121-128): the SMTP masking runs in the
        # model's forward; the tokenizer half of the reference lives on the host, so the caller says which it is
        self.mask_inside_model = bool(mask_inside_model)

    @abc.abstractmethod
    def train_step(self, engine: GgetEngine, batch) -> torch.Tensor: ...

    def update_config(self, pipeline) -> None:
        return None

    def prepare_data(self, pipeline) -> None:
        return None

    def _set_model_config(self, pipeline):
        """modules_utils.set_model_config (:57-81): causal flag by task type, next_n_token = stacked_feat, tokenizer-derived ids."""
        from . import conf as CF
        mc, task = pipeline.model_cfg, CF._get(pipeline.train_cfg, "task_type")
        if CF._get(mc, "intermediate_size") == 0 and CF._get(mc, "num_attention_heads") == 0:      # modules_utils.py:37-42, :63-70
            hidden = CF._get(mc, "hidden_size")
            assert hidden % 64 == 0
            CF._set(mc, "intermediate_size", hidden * 4)
            CF._set(mc, "num_attention_heads", hidden // 64)
            CF._set(mc, "head_dim", 64)
        CF._set(mc, "causal_attention", bool(0 if task == "pretrain-mlm" else CF._get(mc, "causal_attention")))
        CF._set(CF._get(mc, "pt_head"), "next_n_token", CF._get(CF._get(mc, "graph_input"), "stacked_feat"))
        for name in ("vocab_size", "bos_token_id", "eos_token_id"):
            if getattr(self, name) is not None:
                CF._set(mc, name, getattr(self, name))
        return mc

    def post_model_setup(self, pipeline) -> bool:
        return False

    def allow_resume(self) -> bool:
        return True

    def allow_save_config(self) -> bool:
        return True

    def setup_optimizer(self, pipeline) -> None:
        if pipeline.reference_cfg:
            from . import conf as CF
            pipeline.optim = CF.optim_from_training(pipeline.train_cfg, pipeline.use_deepspeed, self.finetune)
        pipeline.engine = initialize(pipeline.model, pipeline.optim)
        pipeline.device = pipeline.model.device
        if pipeline.reference_cfg and not pipeline.use_deepspeed:
            # an empty `deepspeed_conf_file` selects the reference's DDP / AMP branch (training_utils.py:46-86): its optimizer step is
            # GradScaler.step, which SKIPS a step whose gradients are inf / NaN - the modes' train_step goes through engine.step(), so
            # the rule is set on the engine here (the lean `batch_training(batch, engine)` form never saw `use_deepspeed`)
            pipeline.engine.skip_nonfinite = True

    def setup_training(self, pipeline) -> None:
        return None

    def run_training(self, pipeline) -> None:
        t0 = time.time()
        tokens = None   # accumulated where the mask lives (no device->host read per step); read at log time only
        # a resumed run (pipeline._resume_checkpoint restored engine.global_steps) does the REMAINDER of the schedule, like the reference
        # continuing from its checkpoint's epoch / j_init (pipeline.py:178-202) - not max_steps further steps
        done0 = int(pipeline.engine.global_steps)
        if pipeline.max_steps and done0 >= pipeline.max_steps:
            pipeline.model.check_deferred()
            return
        # host batches are handed over one step ahead (pinned staging + a side stream: DevicePrefetcher); GGET_PREFETCH=0 = as they come
        source = pipeline.batches
        if bool(int(os.environ.get("GGET_PREFETCH", "1"))) and torch.cuda.is_available() and pipeline.batches is not None:
            source = DevicePrefetcher(pipeline.batches, pipeline.model.device)
        for step, batch in enumerate(source):
            loss = self.train_step(pipeline.engine, batch)
            pipeline.last_loss = loss
            am = batch["attention_mask"]
            n = batch["num_tokens"] if batch.get("num_tokens") is not None else \
                (am.sum() if am.dim() == 2 else am.diagonal(dim1=1, dim2=2).sum())   # packed rows: [B,S,S] block-diagonal
            tokens = n if tokens is None else tokens + n
            if pipeline.log_every and (step + 1) % pipeline.log_every == 0:
                torch.cuda.synchronize()
                dt = time.time() - t0
                pipeline.log(f"step {pipeline.engine.global_steps} loss {float(loss):.5f} lr {pipeline.engine.last_lr:.3e} "
                             f"tokens/s/gpu {int(tokens) / dt:.0f}")
                pipeline.log_lines.append(f"{pipeline.engine.global_steps},{float(loss):.6f},{pipeline.engine.last_lr:.6e}\n")
                pipeline.model.check_deferred()      # device-side input guards (position ids), read where the loop syncs anyway
            self.after_step(pipeline)
            if pipeline.max_steps and pipeline.engine.global_steps >= pipeline.max_steps:
                break
        pipeline.model.check_deferred()

    def after_step(self, pipeline) -> None:
        """Called by the step loop behind every `train_step` (FinetuneMode: the epoch's end)."""
        return None


class PretrainMode(TrainingMode):
    model_cls = GraphGPTPretrainBase

    def prepare_data(self, pipeline):
        """The schedule / model-config half of reference pretrain_mode.py:96-230 (the dataset half is the constructor's arguments):
        optimizer.min_lr rule (:108), steps_per_saving (:114-116), smtp_inside off unless the tokenizer masks inside the model
        (:121-128), token-budget -> total / warm-up steps (:205-207), epochs (:213-215), nested model config -> flat (:219-220)."""
        if not pipeline.reference_cfg:
            return
        from . import conf as CF
        from .modeling import convert_to_legacy_config
        oc, sc, tc = pipeline.optim_cfg, pipeline.sched_cfg, pipeline.train_cfg
        CF._set(oc, "min_lr", CF._get(oc, "lr") * 0.1 if pipeline.use_deepspeed else 0)
        bs = CF._get(tc, "batch_size")
        if CF._get(sc, "samples_per_saving"):
            CF._set(sc, "steps_per_saving", CF._get(sc, "samples_per_saving") // (pipeline.world_size * bs))
        if self.tokens_per_sample is None:
            raise ValueError("PretrainMode(tokens_per_sample=...): the mean un-padded length the reference estimates from its "
                             "tokenizer (misc_utils.estimate_tokens_per_sample) is needed to turn the token budget into steps")
        # pretrain_mode.py:121-128: smtp_inside follows the tokenizer's masking method, whatever the model config said
        pt_head = CF._get(pipeline.model_cfg, "pt_head")
        if pt_head is not None:
            CF._set(pt_head, "smtp_inside", self.mask_inside_model)
        if self.mask_inside_model:
            assert CF._get(tc, "task_type") in ("pretrain-mlm", "pretrain-smtp")
            CF._set(tc, "task_type", "pretrain-smtp")
        tps = CF._get(pipeline.model_cfg, "max_position_embeddings") if CF._get(tc, "pack_tokens", 0) > 0 else self.tokens_per_sample
        if CF._get(tc, "task_type") == "pretrain-euler":        # pretrain_mode.py:191-195
            tps = tps // 2
        CF.update_num_steps(sc, tps, bs, pipeline.world_size)
        if self.samples_per_gpu:
            CF.update_epochs(sc, tps, self.samples_per_gpu, pipeline.world_size)
        pipeline.model_cfg = self._set_model_config(pipeline)
        pipeline.config = convert_to_legacy_config(pipeline.model_cfg)

    def train_step(self, engine, batch):
        return batch_training(batch, engine)


class FinetuneMode(TrainingMode):
    """Fine-tuning.  Constructed with evaluation loaders (`valid_loader` / `test_loader`, optionally `train_loader_for_eval`) the mode
    closes every epoch the way the reference's `log_dump_ft_training_stats` does (log_eval_dump_utils.py:648-799, see `end_of_epoch`);
    without them the run is the plain step loop.  An epoch is `steps_per_epoch` optimizer steps (default: samples_per_gpu //
    batch_size of a reference-shaped config).  The `training.ft_eval` fields - `epoch_per_eval`, `save_pred`, `save_hidden_states`,
    `eval_only`, `infer_only` - are read from a reference-shaped config; a keyword given here replaces the config's value.
    `eval_kwargs` are `ft_evaluate`'s keywords (problem_type, num_labels, task_level, metric_type, dataset_name); what is not given
    comes from the config (`model.ft_head`, `tokenization.data.dataset`) or the model.  `eval_only` trains nothing: every `epoch_k`
    checkpoint under the checkpoint path (`training.pretrain_cpt`; `output_dir` of the lean config form) is loaded and evaluated
    (finetune_mode.py:351-431).  `infer_only` replaces the evaluation by `dump_results` into `infer_writer`, any object with
    `write(records, indices)` (:433-444; the reference's ODPS writer stays on the host side)."""

    model_cls = GraphGPTTaskModel
    skip_keys = True
    finetune = True
    _FT_EVAL_DEFAULTS = dict(epoch_per_eval=1, save_pred=False, save_hidden_states=False, eval_only=False, infer_only=False)

    def __init__(self, *args, valid_loader=None, test_loader=None, train_loader_for_eval=None, steps_per_epoch: Optional[int] = None,
                 epoch_per_eval: Optional[int] = None, save_pred: Optional[bool] = None, save_hidden_states: Optional[bool] = None,
                 eval_only: Optional[bool] = None, infer_only: Optional[bool] = None, infer_writer=None,
                 eval_kwargs: Optional[Dict[str, Any]] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self.valid_loader, self.test_loader, self.train_loader_for_eval = valid_loader, test_loader, train_loader_for_eval
        self.steps_per_epoch, self.infer_writer, self.eval_kwargs = steps_per_epoch, infer_writer, dict(eval_kwargs or {})
        self.epoch_per_eval, self.save_pred, self.save_hidden_states = epoch_per_eval, save_pred, save_hidden_states
        self.eval_only, self.infer_only = eval_only, infer_only
        self.best_res = self.best_epoch = None      # the best validation result so far (the EMA weights' when an EMA is attached)
        self.epoch_results = []                     # one dict per evaluated epoch: losses, results, the files written
        self._epochs_closed = 0

    @property
    def has_eval_loaders(self) -> bool:
        return self.valid_loader is not None or self.test_loader is not None

    # -- the ft_eval fields: keyword > reference-shaped config > default
    def _resolve_ft_eval(self, cfg) -> None:
        from . import conf as CF
        tc = CF._get(cfg, "training") if cfg is not None and CF.is_reference_config(cfg) else None
        ft_eval = CF._get(tc, "ft_eval") if tc is not None else None
        for name, default in self._FT_EVAL_DEFAULTS.items():
            if getattr(self, name) is None:
                setattr(self, name, type(default)(CF._get(ft_eval, name, default) if ft_eval is not None else default))

    def update_config(self, pipeline):
        self._resolve_ft_eval(pipeline.cfg)

    def allow_resume(self) -> bool:
        return not self.eval_only           # finetune_mode.py: an eval_only run loads the epoch checkpoints itself

    def allow_save_config(self) -> bool:
        return not self.eval_only           # ... and writes neither a config nor a checkpoint

    def setup_training(self, pipeline):
        from . import conf as CF
        self._resolve_ft_eval(pipeline.cfg)
        if not self.has_eval_loaders:
            if self.eval_only or self.infer_only:
                raise ValueError("FinetuneMode(eval_only / infer_only): valid_loader / test_loader are needed")
            return
        if (self.eval_only or not self.infer_only) and (self.valid_loader is None or self.test_loader is None):
            raise ValueError("FinetuneMode: the epoch's end evaluates valid AND test (log_dump_ft_training_stats): give both loaders")
        if self.infer_only and (self.infer_writer is None or self.test_loader is None):
            raise ValueError("FinetuneMode(infer_only=True): test_loader and infer_writer (an object with write(records, indices)) are needed")
        if self.steps_per_epoch is None and pipeline.reference_cfg and self.samples_per_gpu:
            self.steps_per_epoch = max(1, int(self.samples_per_gpu) // int(CF._get(pipeline.train_cfg, "batch_size")))
        if not self.eval_only and not self.steps_per_epoch:
            raise ValueError("FinetuneMode(steps_per_epoch=...): the optimizer steps of one epoch are needed to know where an epoch ends")
        kw = self.eval_kwargs
        if pipeline.reference_cfg:
            head = CF._get(pipeline.model_cfg, "ft_head")
            for ours, theirs in (("problem_type", "problem_type"), ("num_labels", "num_labels"), ("task_level", "task_type"),
                                 ("metric_type", "metric_type")):
                if ours not in kw and head is not None and CF._get(head, theirs) is not None:
                    kw[ours] = CF._get(head, theirs)
            if "dataset_name" not in kw and pipeline.data_cfg is not None and CF._get(pipeline.data_cfg, "dataset"):
                kw["dataset_name"] = CF._get(pipeline.data_cfg, "dataset")
        kw.setdefault("num_labels", int(pipeline.model.config.num_labels))
        kw.setdefault("problem_type", pipeline.model.config.problem_type or ("regression" if kw["num_labels"] == 1 else "single_label_classification"))

    # -- the epoch's end
    def after_step(self, pipeline):
        if not self.has_eval_loaders or not self.steps_per_epoch:
            return
        done = int(pipeline.engine.global_steps) // int(self.steps_per_epoch)
        if done <= self._epochs_closed or int(pipeline.engine.global_steps) % int(self.steps_per_epoch):
            return
        self._epochs_closed = done
        epoch = done - 1
        if (epoch + 1) % int(self.epoch_per_eval) == 0:
            self.end_of_epoch(pipeline, epoch)

    def end_of_epoch(self, pipeline, epoch: int):
        """reference log_dump_ft_training_stats (log_eval_dump_utils.py:648-799), in its order: (1) the checkpoint `epoch_<k>` (not under
        eval_only); (2) `ft_evaluate` on train-for-eval, valid and test - with an EMA attached the valid pass once more under
        `engine.ema_weights()`, and the test pass and the inference pass on the averaged weights; (3) the best validation result so far
        by `compare_metrics_res` (the EMA result's when there is one; a result dict that names no single key to compare on - several
        keys, none starting with "ema" - is not ranked, where the reference would stop on an assertion); with an EMA the rank-0 files
        model_ema.pt / model_ema_best.pt follow it (EMAStats.save_ema_ckp); (4) one line on `pipeline.log_lines`; (5) on rank 0 the
        prediction triplets as epoch_<k>/{train,valid,test}_results.csv when `save_pred`; (6) `ft_infer_hidden_states` on the test loader
        and `dump_infer_results`.  With `infer_only` steps 2 to 6 are `dump_results` into `infer_writer`.  Checkpoints of earlier epochs
        are kept (the reference deletes epoch k - 5)."""
        from . import inference as INF
        from . import metrics as M
        engine, model, out_dir = pipeline.engine, pipeline.model, pipeline.output_dir
        if not out_dir:
            raise ValueError("FinetuneMode: the epoch's end writes files; the pipeline needs an output_dir")
        ep_dir = os.path.join(out_dir, f"epoch_{epoch}")
        if not self.eval_only:
            engine.consolidate()            # (a collective of every rank)
            if pipeline.rank == 0:
                engine.save_checkpoint(out_dir, tag=f"epoch_{epoch}")
        if self.infer_only:
            n = INF.dump_results(model, self.test_loader, pipeline.device, self.infer_writer, pipeline.rank, epoch=epoch)
            model.train()
            self.epoch_results.append({"epoch": epoch, "records": n})
            return
        e = model._engine
        use_ema = not self.eval_only and e is not None and e.ema is not None and e.ema_live
        kw = self.eval_kwargs
        tr_loss, _, tr_res, tr_triplet = (ft_evaluate(model, self.train_loader_for_eval, eval_name="train", **kw)
                                          if self.train_loader_for_eval is not None else (0, None, None, None))
        val_loss, val_metrics, val_res, val_triplet = ft_evaluate(model, self.valid_loader, eval_name="valid", **kw)
        val_res_ema = None
        with (engine.ema_weights() if use_ema else contextlib.nullcontext()):
            if use_ema:
                _, _, val_res_ema, _ = ft_evaluate(model, self.valid_loader, eval_name="valid", **kw)
            test_loss, test_metrics, test_res, test_triplet = ft_evaluate(model, self.test_loader, eval_name="test", **kw)
            idx, logits, hidden = INF.ft_infer_hidden_states(model, self.test_loader, None, "test", save_hidden_states=self.save_hidden_states)
        model.train()
        ranked = val_res_ema if use_ema else val_res
        is_best = False
        if isinstance(ranked, dict) and (len(ranked) == 1 or sum(k.lower().startswith("ema") for k in ranked) == 1):
            is_best, self.best_res = (True, ranked) if self.best_res is None else M.compare_metrics_res(ranked, self.best_res)
            if is_best:
                self.best_epoch = epoch
        pipeline.log(f"[epoch {epoch}][global {engine.global_steps}] train_loss: {tr_loss}, valid_loss: {val_loss}, test_loss: {test_loss}, "
                     f"train: {tr_res}, valid: {val_res}, EMA valid: {val_res_ema}, test: {test_res}")
        tup = lambda m: ",".join(str(v) for v in m.results_in_tuple())      # noqa: E731
        pipeline.log_lines.append(f"{epoch},{engine.global_steps},{float(tr_loss)},{float(val_loss)},{float(test_loss)},{tup(val_metrics)},"
                                  f"{_format_eval_res(val_res)},{tup(test_metrics)},{_format_eval_res(test_res)}\n")
        files = []
        if pipeline.rank == 0:
            os.makedirs(ep_dir, exist_ok=True)
            if self.save_pred:
                for name, triplet in (("train", tr_triplet), ("valid", val_triplet), ("test", test_triplet)):
                    if triplet:
                        files.append(INF.save_pred_results(triplet, ep_dir, name))
            if use_ema:
                engine.save_ema_checkpoint(out_dir, best=bool(is_best))
        files += INF.dump_infer_results(out_dir, epoch, idx=idx, logits=logits, hidden_states=hidden)
        self.epoch_results.append({"epoch": epoch, "train_loss": float(tr_loss), "valid_loss": float(val_loss), "test_loss": float(test_loss),
                                   "train": tr_res, "valid": val_res, "valid_ema": val_res_ema, "test": test_res, "is_best": bool(is_best),
                                   "files": files, "idx": idx, "logits": logits, "hidden_states": hidden})

    def run_training(self, pipeline):
        if not self.eval_only:
            return super().run_training(pipeline)
        # eval_only (finetune_mode.py:419-431): no step; every epoch_<k> under the checkpoint path is loaded by name and evaluated
        from . import checkpoint as CK
        root = pipeline.pretrain_cpt or pipeline.output_dir
        if not root or not os.path.isdir(root):
            raise ValueError(f"FinetuneMode(eval_only=True): no checkpoint directory at {root!r}")
        for epoch in CK._scan_ckps(root):
            ckp = os.path.join(root, f"epoch_{epoch}")
            if not os.path.isdir(ckp) or (epoch + 1) % int(self.epoch_per_eval):
                continue
            CK.load_from_ckp_with_try(pipeline.model, ckp, skip_keys=False)
            self.end_of_epoch(pipeline, epoch)
        pipeline.model.check_deferred()

    def prepare_data(self, pipeline):
        """reference finetune_mode.py:181-192: epoch budget -> steps, set_ft_model_config (modules_utils.py:84-92), nested -> flat."""
        if not pipeline.reference_cfg:
            return
        from . import conf as CF
        from .modeling import convert_to_legacy_config
        if self.samples_per_gpu is None:
            raise ValueError("FinetuneMode(samples_per_gpu=...): train samples per rank (len(sampler) // world) are needed for the schedule")
        CF.update_ft_num_steps(pipeline.train_cfg, self.samples_per_gpu)
        mc = self._set_model_config(pipeline)
        if len(CF._get(pipeline.train_cfg, "pretrain_cpt", "") or "") == 0:
            CF._set(mc, "num_key_value_heads", CF._get(mc, "num_attention_heads"))
        CF._set(mc, "tie_word_embeddings", False)
        CF._set(CF._get(mc, "pt_head"), "next_n_token", 1)
        pipeline.model_cfg = mc
        pipeline.config = convert_to_legacy_config(mc)

    def post_model_setup(self, pipeline):
        """reference finetune_mode.py:204-212: `finetune.freeze > -1` freezes embed_tokens and the first `freeze` layers
        (modules_utils.freeze_llama_layers), then config.num_params = the trainable count print_trainable_parameters reports."""
        from .modeling import freeze_llama_layers, print_trainable_parameters
        freeze = -1
        if pipeline.reference_cfg:
            from . import conf as CF
            ft = CF._get(pipeline.train_cfg, "finetune", None)
            freeze = int(CF._get(ft, "freeze", -1)) if ft is not None else -1
        if freeze > -1:
            freeze_llama_layers(pipeline.model, freeze)
        pipeline.model.config.num_params = print_trainable_parameters(pipeline.model)
        return False

    def setup_optimizer(self, pipeline):
        if pipeline.reference_cfg:
            from . import conf as CF
            CF.set_finetune_cfg(CF._get(pipeline.train_cfg, "finetune"))       # finetune_mode.py:224
        super().setup_optimizer(pipeline)

    def train_step(self, engine, batch):
        return ft_batch_training(batch, engine)[0]


class TrainingPipeline:
    """`TrainingPipeline(cfg, mode).run()` (reference src/training/pipeline.py:15-216), the same phases in the same order.

    `cfg` is either the reference's `Config` shape - `cfg.model` = nested GraphGPTModelConfig, `cfg.training` with `.batch_size`,
    `.deepspeed_conf_file`, `.pretrain_cpt`, `.output_dir`, `.schedule`, `.optimizer`, `.distributed` (graph-gpt_amd/conf.py names the
    fields read; any attribute tree works: the reference's dataclasses, OmegaConf, SimpleNamespace) - or the lean form of earlier
    rounds: `model` (GraphGPTConfig or kwargs), `optim` (OptimConfig or kwargs), `batches`, `max_steps`, `log_every`, `output_dir`,
    `resume_from`.  With the reference shape the batch source is the mode's (`PretrainMode(batches=..., tokens_per_sample=...)`);
    the run is `training.schedule.total_num_steps` optimizer steps long."""

    def __init__(self, cfg: Any, mode: TrainingMode):
        from . import conf as CF
        self.cfg, self.mode = cfg, mode
        self.reference_cfg = CF.is_reference_config(cfg)
        get = (lambda k, d=None: cfg.get(k, d)) if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
        self.token_cfg = self.model_cfg = self.train_cfg = self.data_cfg = self.sched_cfg = self.optim_cfg = None
        self.use_deepspeed, self.pretrain_cpt, self.world_size, self.rank = False, "", 1, 0
        self.config = self.model = self.device = None
        self.engine: Optional[GgetEngine] = None
        self.last_loss = None
        self.log_lines = []        # "step,loss,lr" lines of this run -> <output_dir>/log.csv (the file whose presence means "resume", pipeline.py:129)
        self.max_steps, self.log_every = get("max_steps", 0) or 0, get("log_every", 0) or 0
        if self.reference_cfg:
            self.optim, self.batches = None, get("batches") if get("batches") is not None else mode.batches
            self.output_dir, self.resume_from = None, None
        else:
            from .modeling import GraphGPTConfig
            mc = get("model")
            self.config = mc if isinstance(mc, GraphGPTConfig) else GraphGPTConfig(**mc)
            oc = get("optim", {})
            self.optim = oc if isinstance(oc, OptimConfig) else OptimConfig(**(oc or {}))
            self.batches = get("batches") if get("batches") is not None else mode.batches
            self.output_dir, self.resume_from = get("output_dir"), get("resume_from")

    @property
    def model_config(self):                 # (name of earlier rounds)
        return self.config

    def log(self, msg: str):
        if self.rank == 0:
            print(msg, flush=True)

    # -- shared phases, reference-shaped config only (pipeline.py:97-139)
    def _extract_config(self):
        from . import conf as CF
        g = CF._get
        CF.sync_config(self.cfg)      # (task_type "pretrain-cl" -> pt_head.use_discriminative, base_configs.py:246-247)
        self.token_cfg, self.model_cfg, self.train_cfg = g(self.cfg, "tokenization"), g(self.cfg, "model"), g(self.cfg, "training")
        self.data_cfg = g(self.token_cfg, "data") if self.token_cfg is not None else None
        self.sched_cfg, self.optim_cfg = g(self.train_cfg, "schedule"), g(self.train_cfg, "optimizer")

    def _setup_deepspeed_flag(self):
        from . import conf as CF
        tc = self.train_cfg
        self.pretrain_cpt, self.output_dir = CF._get(tc, "pretrain_cpt", "") or "", CF._get(tc, "output_dir", None)
        self.use_deepspeed = len(CF._get(tc, "deepspeed_conf_file", "") or "") > 0
        CF._set(tc, "use_deepspeed", self.use_deepspeed)
        if self.output_dir and os.path.exists(os.path.join(self.output_dir, "log.csv")):
            self.log(f"log file {os.path.join(self.output_dir, 'log.csv')} exists, resume training from {self.output_dir} instead of "
                     f"initializing from pre-train ckp {self.pretrain_cpt}!")
            self.pretrain_cpt = self.output_dir

    def _setup_distributed(self):
        from . import conf as CF
        self.rank, _, self.world_size = set_dist_env()
        dc = CF._get(self.train_cfg, "distributed", None) if self.reference_cfg else None
        if dc is not None:
            CF._set(dc, "world_size", self.world_size)
            CF._set(dc, "rank", self.rank)

    def _create_model(self):
        self.model = self.mode.model_cls(self.config)
        self.model.gradient_checkpointing_enable()
        self.model.config.use_cache = False

    def _load_initial_ckp(self):
        """pipeline.py:165-176: a pre-trained checkpoint that is not the run's own output directory is loaded by name."""
        from . import checkpoint as CK
        self.model = CK.load_from_ckp(self.pretrain_cpt, self.output_dir or "", self.model, self.config, skip_keys=self.mode.skip_keys)

    def _resume_checkpoint(self):
        """pipeline.py:178-202: weights + optimizer state of the run's own latest checkpoint."""
        from . import checkpoint as CK
        if not (len(self.pretrain_cpt) > 0 and self.pretrain_cpt == self.output_dir and self.mode.allow_resume()):
            return
        ckp, _ = CK.get_latest_ckp(self.pretrain_cpt)
        if os.path.exists(os.path.join(ckp, "model.pt")):
            self.engine.load_checkpoint(ckp)

    def _save_model_config(self):
        if self.rank != 0 or not self.mode.allow_save_config() or not self.output_dir:
            return
        os.makedirs(self.output_dir, exist_ok=True)
        self.model.config.save_pretrained(self.output_dir)

    def run(self):
        if self.reference_cfg:
            self._extract_config()
            self.mode.update_config(self)
            self._setup_deepspeed_flag()
            self._setup_distributed()
            self.mode.prepare_data(self)
            if self.config is None:
                raise ValueError("the mode's prepare_data did not set pipeline.config (convert_to_legacy_config(pipeline.model_cfg))")
            from . import conf as CF
            if not self.max_steps:
                self.max_steps = int(CF._get(self.sched_cfg, "total_num_steps") or 0)
            if not self.log_every:
                self.log_every = 0
            self._create_model()
            if self.mode.post_model_setup(self):
                return self
            self._load_initial_ckp()
            self.model.cuda()
            self.mode.setup_optimizer(self)
            self._resume_checkpoint()
            self._save_model_config()
            self.mode.setup_training(self)
            self.mode.run_training(self)
            if self.output_dir and self.mode.allow_save_config() and getattr(self, "engine", None) is not None:
                self.engine.consolidate()       # (a collective of every rank: the sharded step leaves the optimizer state partitioned)
            if self.output_dir and self.rank == 0 and self.mode.allow_save_config():
                self.engine.save_checkpoint(self.output_dir)
                # the reference's save_all writes log.csv next to its checkpoints (misc_utils.py:150-154); its presence in output_dir is
                # what makes the next run with this output_dir a RESUME (_setup_deepspeed_flag above / pipeline.py:129)
                with open(os.path.join(self.output_dir, "log.csv"), "a") as fh:
                    fh.writelines(self.log_lines or [f"{self.engine.global_steps},{float(self.last_loss) if self.last_loss is not None else float('nan'):.6f},"
                                                     f"{getattr(self.engine, 'last_lr', float('nan')):.6e}\n"])
            return self
        self._setup_distributed()
        self.mode.update_config(self)
        self.mode.prepare_data(self)
        self._create_model()
        if self.mode.post_model_setup(self):
            return self
        self.model.cuda()
        self.mode.setup_optimizer(self)
        if self.resume_from:
            self.engine.load_checkpoint(self.resume_from)
        self.mode.setup_training(self)
        self.mode.run_training(self)
        if self.output_dir and self.mode.allow_save_config() and getattr(self, "engine", None) is not None:
            self.engine.consolidate()
        if self.output_dir and self.rank == 0 and self.mode.allow_save_config():
            self.engine.save_checkpoint(self.output_dir)
        return self


def launch(fn: Callable, *args, **kwargs):
    """Entry-point wrapper with the reference's name (`launch(train)`, pipeline.py:229-257).  Ranks are created by
    `python -m torch.distributed.run`, one per GPU; the only thing the shim has to do is drop the launcher-injected `--local_rank*`
    arguments before the entry point reads sys.argv.  The reference's Hydra override rewriting is CLI-side and out of scope
    (DESIGN.md section 7): pass overrides as `key=value`."""
    import sys
    sys.argv = [a for a in sys.argv if not a.startswith("--local_rank")]
    return fn(*args, **kwargs)
