"""Python host side of the engine: owns the HBM arenas (as torch tensors: PyTorch is the allocator
and stream provider, nothing more), binds them to a `gget_handle_t`, and exposes forward / backward /
optimizer step on raw device pointers.  Mirrors what the reference gets from
`deepspeed.initialize(...)` / DDP+AdamW (SURVEY.md section 8b "Engine protocol")."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from .spec import KIND_PRETRAIN, KIND_TASK, ModelSpec


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rope_tables(max_position: int, head_dim: int, theta: float):
    """fp32 cos/sin [max_position, head_dim/2], computed exactly like hf LlamaRotaryEmbedding.forward
    :111-127 does on the host (fp32 inv_freq, fp32 outer product, fp32 cos/sin)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    freqs = torch.arange(max_position, dtype=torch.float32)[:, None] * inv_freq[None, :]
    return freqs.cos().contiguous(), freqs.sin().contiguous()


def make_config(spec: ModelSpec, max_tokens: int, max_batch: int) -> "L.GgetConfig":
    """The gget_config_t of a model spec and its capacities (what Engine hands to gget_create; the handle-free planning entries -
    gget_shard_plan, gget_group_plan - take the same struct)."""
    cfg = L.GgetConfig()
    (cfg.kind, cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_layers, cfg.num_heads,
     cfg.stacked_feat, cfg.next_n_token, cfg.gated_agg, cfg.causal, cfg.max_position, cfg.num_labels,
     cfg.score_bias, cfg.pad_token_id) = spec.as_c_ints()
    cfg.rms_eps, cfg.rope_theta, cfg.layer_scale_init = spec.rms_eps, spec.rope_theta, spec.layer_scale_init
    cfg.max_tokens, cfg.max_batch = int(max_tokens), int(max_batch)
    cfg.path_pdrop = float(getattr(spec, "path_pdrop", 0.0))
    cfg.mlp_pdrop = float(getattr(spec, "mlp_pdrop", 0.0))
    hm = [int(x) for x in getattr(spec, "head_mlp", ())]
    assert len(hm) <= 4, "the MLP score head holds at most 4 hidden layers"
    cfg.head_mlp_layers = len(hm)
    for i, x in enumerate(hm):
        cfg.head_mlp[i] = x
    cfg.embed_dim = int(getattr(spec, "embed_dim", 0) or 0)
    return cfg


class Engine:
    def __init__(self, spec: ModelSpec, max_tokens: int, max_batch: int, device: Optional[torch.device] = None,
                 with_optimizer: bool = True):
        if not torch.cuda.is_available():
            raise L.GgetError("the gget engine needs a GPU (torch.cuda.is_available() is False); there is no CPU path")
        self.lib = L.load()
        self.spec = spec
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        cfg = make_config(spec, max_tokens, max_batch)
        self.cfg = cfg
        sz = L.GgetSizes()
        L.check(self.lib.gget_query_sizes(C.byref(cfg), C.byref(sz)))
        self.n_params = int(sz.n_params)
        dev = self.device
        with torch.cuda.device(dev):
            self.param_bf16 = torch.zeros(self.n_params, dtype=torch.bfloat16, device=dev)
            self.grad_bf16 = torch.zeros(self.n_params, dtype=torch.bfloat16, device=dev)
            self.master = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
            if with_optimizer:
                self.adam_m = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
                self.adam_v = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
            else:
                self.adam_m = self.adam_v = None
            self.workspace = torch.zeros(int(sz.workspace_bytes), dtype=torch.uint8, device=dev)
            cos, sin = rope_tables(spec.max_position, spec.head_dim, spec.rope_theta)
            self.rope_cos, self.rope_sin = cos.to(dev), sin.to(dev)
            self._loss = torch.zeros(1, dtype=torch.float32, device=dev)
            self._gnorm = torch.zeros(1, dtype=torch.float32, device=dev)
        bufs = L.GgetBuffers(_ptr(self.param_bf16), _ptr(self.master), _ptr(self.adam_m), _ptr(self.adam_v),
                             _ptr(self.grad_bf16), _ptr(self.workspace), _ptr(self.rope_cos), _ptr(self.rope_sin))
        h = C.c_void_p()
        # gget_create clears parts of the workspace and uploads tables on the NULL stream; the arenas above were zero-filled on
        # torch's current stream (possibly a non-blocking side stream): order the two
        torch.cuda.current_stream(dev).synchronize()
        L.check(self.lib.gget_create(C.byref(cfg), C.byref(bufs), C.byref(h)))
        self.h = h
        self.workspace_bytes = int(sz.workspace_bytes)
        # parameter table
        self.varlen_mode: Optional[str] = None     # per-engine override of GGET_VARLEN (see _set_layout)
        self.params: "OrderedDict[str, dict]" = OrderedDict()
        info = L.GgetParamInfo()
        for i in range(self.lib.gget_param_count(self.h)):
            L.check(self.lib.gget_param_info(self.h, i, C.byref(info)))
            shape = tuple(int(info.shape[k]) for k in range(info.ndim))
            n = int(np.prod(shape))
            off = int(info.offset)
            self.params[info.name.decode()] = dict(shape=shape, offset=off, numel=n, layer=int(info.layer))
        self.buckets = []
        o, c = C.c_uint64(), C.c_uint64()
        for b in range(self.lib.gget_bucket_count(self.h)):
            L.check(self.lib.gget_bucket_range(self.h, b, C.byref(o), C.byref(c)))
            self.buckets.append((int(o.value), int(c.value)))
        self.step_count = 0
        self.comm_world = 0     # > 0 once this handle owns an RCCL communicator (comm_init / comm_adopt)
        # sharded optimizer step (ZeRO-2, shard_init): (world, rank) of the plan, its per-bucket ranges, the norm's partial vector
        self.shard = None
        self.shard_buckets = []
        self.shard_slots = None
        # True while master / m / v hold stale values outside this rank's share (after a sharded step, until a consolidation)
        self.shard_stale = False
        # weight EMA (ema_attach): the sixth arena, allocated on demand; `ema_live` = it holds an average (seeded or loaded), `ema_stale` =
        # partitioned by sharded steps like master / m / v; `_params_are_ema` = the bf16 copy currently holds the averaged weights
        self.ema = None
        self.ema_live = False
        self.ema_stale = False
        self._params_are_ema = False
        # gradient accumulation (grad_acc_attach): the seventh arena, allocated on demand - the fp32 sum of a window's micro-batch gradients
        self.grad_acc = None
        # frozen prefix (set_frozen): -1 = everything trains; `train_ranges` = [(offset, count)] of the trainable elements of the flat arenas
        self.frozen = -1
        self.train_ranges = [(0, self.n_params)]
        self._params_ready = None   # event behind the all-gather of the bf16 copy: the next reader of the weights waits for it
        self._keep = None  # keeps the last batch tensors alive until backward has consumed them

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.gget_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ parameters
    def view(self, name: str, which: str = "master") -> torch.Tensor:
        p = self.params[name]
        arena = {"master": self.master, "bf16": self.param_bf16, "grad": self.grad_bf16, "m": self.adam_m,
                 "v": self.adam_v, "ema": self.ema, "grad_acc": self.grad_acc}[which]
        if arena is None:
            raise L.GgetError(f"view({name!r}, {which!r}): this engine has no such arena")
        return arena[p["offset"]: p["offset"] + p["numel"]].view(p["shape"])

    def load_state_dict(self, state: Dict[str, "np.ndarray | torch.Tensor"], strict: bool = True):
        missing = [k for k in self.params if k not in state]
        unexpected = [k for k in state if k not in self.params]
        if strict and (missing or unexpected):
            raise KeyError(f"state dict mismatch: missing {missing[:4]} unexpected {unexpected[:4]}")
        for k, p in self.params.items():
            if k in state:
                t = torch.as_tensor(state[k]).to(torch.float32).reshape(p["shape"])
                self.view(k, "master").copy_(t.to(self.device))
        self.await_params()
        if not missing:
            self.shard_stale = False    # (every master weight written)
        self.sync_params()
        return missing, unexpected

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict((k, self.view(k, "master").detach().clone()) for k in self.params)

    def sync_params(self):
        if self.shard_stale:
            raise L.GgetError("sync_params: the fp32 master weights are partitioned after a sharded (ZeRO-2) step - outside this rank's "
                              "share they are stale; call GgetEngine.consolidate() on every rank first")
        L.check(self.lib.gget_sync_params(self.h, _stream()))
        self._params_are_ema = False

    # ------------------------------------------------------------------ frozen prefix (finetune.freeze)
    def set_frozen(self, k: int):
        """Freeze embed_tokens and the first k layers (gget_set_frozen; -1 = nothing, the reference's freeze_llama_layers pattern): norm,
        clip, AdamW, EMA, accumulation and the exchange then touch `train_ranges` only, and the backward stops at the lowest trainable unit
        when nothing trainable sits upstream of layer 0.  An active shard plan is rebuilt for the new ranges."""
        L.check(self.lib.gget_set_frozen(self.h, int(k)))
        self.frozen = int(k)
        out, n = (C.c_uint64 * 4)(), C.c_int32(0)
        L.check(self.lib.gget_trainable_ranges(self.h, out, C.byref(n)))
        self.train_ranges = [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n.value)]
        if self.shard is not None:
            self.shard_init(*self.shard)

    def bucket_train_range(self, b: int):
        """(offset, count) of bucket b's trainable share: the bucket, nothing (count 0), or the embedding bucket's gate / raw-embedding part."""
        o, c = C.c_uint64(), C.c_uint64()
        L.check(self.lib.gget_bucket_train_range(self.h, int(b), C.byref(o), C.byref(c)))
        return int(o.value), int(c.value)

    def trainable_buckets(self):
        """The exchange's view of `buckets`: every bucket cut to its trainable share (count 0 = nothing to exchange)."""
        return [self.bucket_train_range(b) for b in range(len(self.buckets))]

    def is_frozen(self, name: str) -> bool:
        p = self.params[name]
        return not any(off <= p["offset"] < off + n for off, n in self.train_ranges)

    # ------------------------------------------------------------------ parameter groups (per-parameter lr / weight-decay scales)
    @staticmethod
    def scale_arrays(names, lr_scale=None, wd_scale=None):
        """Two fp32 arrays indexed like `names` from {state-dict name: scale} dicts: a missing name takes 1.0, an unknown one raises."""
        names = list(names)
        out = []
        for what, d in (("lr_scale", lr_scale or {}), ("wd_scale", wd_scale or {})):
            unknown = sorted(k for k in d if k not in set(names))
            if unknown:
                raise KeyError(f"set_param_scales: {what} names no parameter of this model: {unknown[:6]}")
            out.append(np.array([float(d.get(k, 1.0)) for k in names], dtype=np.float32))
        return out

    def set_param_scales(self, lr_scale: Optional[Dict[str, float]] = None, wd_scale: Optional[Dict[str, float]] = None):
        """Parameter groups (gget_set_param_scales): every step runs parameter `name` at lr * lr_scale[name] and weight_decay *
        wd_scale[name], one fp32 product each.  Keys are state-dict names; a missing name takes 1.0, an unknown one raises.  Both None
        switches the groups off.  The table stays on the handle through set_frozen / shard_init, in either call order."""
        if lr_scale is None and wd_scale is None:
            L.check(self.lib.gget_set_param_scales(self.h, None, None, 0))
            return
        lr, wd = self.scale_arrays(self.params, lr_scale, wd_scale)
        fp = C.POINTER(C.c_float)
        L.check(self.lib.gget_set_param_scales(self.h, lr.ctypes.data_as(fp), wd.ctypes.data_as(fp), len(self.params)))

    def param_scales(self):
        """({name: lr_scale}, {name: wd_scale}) as the handle holds them (gget_param_scales); ones while no groups are set."""
        n = len(self.params)
        lr, wd = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.float32)
        fp = C.POINTER(C.c_float)
        L.check(self.lib.gget_param_scales(self.h, lr.ctypes.data_as(fp), wd.ctypes.data_as(fp), n))
        return ({k: float(x) for k, x in zip(self.params, lr)}, {k: float(x) for k, x in zip(self.params, wd)})

    @staticmethod
    def plan_params_of(cfg):
        """The parameter table of a configuration without a handle (gget_plan_param_count / gget_plan_param_info): name -> dict as
        `Engine.params`, plus `ndim`."""
        lib, info = L.load(), L.GgetParamInfo()
        n = lib.gget_plan_param_count(C.byref(cfg))
        if n < 0:
            raise L.GgetError(f"gget error: {lib.gget_last_error().decode()}")
        out = OrderedDict()
        for i in range(n):
            L.check(lib.gget_plan_param_info(C.byref(cfg), i, C.byref(info)))
            shape = tuple(int(info.shape[k]) for k in range(info.ndim))
            out[info.name.decode()] = dict(shape=shape, offset=int(info.offset), numel=int(np.prod(shape)), layer=int(info.layer),
                                           ndim=int(info.ndim))
        return out

    @staticmethod
    def group_plan_of(cfg, lr_scale=None, wd_scale=None, frozen_layers: int = -1, world: int = 0, rank: int = -1):
        """[(offset, count, lr_scale, wd_scale)]: the work items of the step of this configuration (gget_group_plan; defined once, in
        C, from the configuration alone).  lr_scale / wd_scale: fp32 arrays indexed like the parameter table, or None = ones."""
        lib, fp = L.load(), C.POINTER(C.c_float)
        arr = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (lr_scale, wd_scale)]
        n = max([0] + [len(a) for a in arr if a is not None])
        ptr = [None if a is None else a.ctypes.data_as(fp) for a in arr]
        args = (C.byref(cfg), ptr[0], ptr[1], n, int(frozen_layers), int(world), int(rank))
        cnt = C.c_int32(0)
        L.check(lib.gget_group_plan(*args, None, 0, C.byref(cnt)))
        items = (L.GgetGroupItem * max(1, cnt.value))()
        L.check(lib.gget_group_plan(*args, items, cnt.value, C.byref(cnt)))
        return [(int(it.off), int(it.cnt), float(it.lr_scale), float(it.wd_scale)) for it in items[:cnt.value]]

    # ------------------------------------------------------------------ gradient accumulation (optimizer.gradient_accumulation_steps)
    def grad_acc_attach(self):
        """Allocate the accumulator arena (fp32 [n_params]) and hand it to the handle (gget_grad_acc_attach); a no-op when it exists.
        No window is open: the first grad_accumulate() overwrites it."""
        if self.grad_acc is None:
            self.grad_acc = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
            L.check(self.lib.gget_grad_acc_attach(self.h, _ptr(self.grad_acc)))
        return self.grad_acc

    def grad_acc_detach(self):
        L.check(self.lib.gget_grad_acc_attach(self.h, None))
        self.grad_acc = None

    def grad_accumulate(self):
        """grad_acc (+)= grad_bf16 in fp32, one launch (gget_grad_accumulate); the first call of a window overwrites.  Until the next
        adamw_step / adamw_step_sharded, which closes the window, norm, clip and update read the fp32 sum."""
        self.grad_acc_attach()
        L.check(self.lib.gget_grad_accumulate(self.h, _stream()))

    def grad_acc_count(self) -> int:
        """Micro-steps summed in the open window (gget_grad_acc_count); 0 = none open."""
        n = C.c_int32(0)
        L.check(self.lib.gget_grad_acc_count(self.h, C.byref(n)))
        return int(n.value)

    def grad_acc_set_count(self, n: int):
        """Re-open a window at `n` micro-steps over what the arena holds (gget_grad_acc_set_count: the resume path); 0 closes it."""
        if int(n) > 0:
            self.grad_acc_attach()
        L.check(self.lib.gget_grad_acc_set_count(self.h, int(n)))

    # ------------------------------------------------------------------ weight EMA (optimizer.use_ema)
    def ema_attach(self):
        """Allocate the EMA arena (zero-filled fp32 [n_params]) and hand it to the handle (gget_ema_attach); a no-op when it exists.
        The arena holds nothing yet: seed it (ema_update(0.0)) or load one (load_ema_state_dict)."""
        if self.ema is None:
            self.ema = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()    # (gget_ema_attach clears the pad rows on the NULL stream)
            L.check(self.lib.gget_ema_attach(self.h, _ptr(self.ema)))
        return self.ema

    def ema_detach(self):
        L.check(self.lib.gget_ema_attach(self.h, None))
        self.ema, self.ema_live, self.ema_stale = None, False, False

    def set_ema_decay(self, decay: float):
        """The decay the NEXT adamw_step / adamw_step_sharded applies inside its launch (gget_set_ema_decay); negative = leave the EMA alone."""
        L.check(self.lib.gget_set_ema_decay(self.h, float(decay)))

    def ema_update(self, decay: float):
        """The stand-alone lerp ema <- master + decay * (ema - master) (gget_ema_update); decay 0 copies the master weights bit for bit."""
        L.check(self.lib.gget_ema_update(self.h, float(decay), _stream()))
        self.ema_live = True
        if self.shard is not None and self.shard[0] > 1 and not getattr(self, "_loopback", False):
            self.ema_stale = True       # (a shard plan: only this rank's share was averaged)

    def ema_to_params(self):
        """bf16 compute copy <- EMA arena (gget_ema_to_params): forwards run on the averaged weights until sync_params()."""
        if self.ema is None or not self.ema_live:
            raise L.GgetError("ema_to_params: this engine holds no weight EMA")
        if self.ema_stale:
            raise L.GgetError("ema_to_params: the weight EMA is partitioned after a sharded (ZeRO-2) step - outside this rank's share it "
                              "is stale; call GgetEngine.consolidate() on every rank first")
        self.await_params()
        L.check(self.lib.gget_ema_to_params(self.h, _stream()))
        self._params_are_ema = True

    def ema_state_dict(self, shapes=None) -> "OrderedDict[str, torch.Tensor]":
        """The averaged weights by state-dict name (clones); `shapes` = {name: shape} overrides the engine's own shapes with the
        module's reference shapes (emb_mask_token is [1,1,embed_dim] there, flat in the arena)."""
        if self.ema is None or not self.ema_live:
            raise L.GgetError("ema_state_dict: this engine holds no weight EMA")
        if self.ema_stale:
            raise L.GgetError("ema_state_dict: the weight EMA is partitioned after a sharded (ZeRO-2) step and stale outside this rank's "
                              "share; call GgetEngine.consolidate() on every rank first")
        shapes = shapes or {}
        return OrderedDict((k, self.view(k, "ema").detach().clone().reshape(tuple(shapes.get(k, p["shape"])))) for k, p in self.params.items())

    def load_ema_state_dict(self, state: Dict[str, "np.ndarray | torch.Tensor"], strict: bool = True):
        missing = [k for k in self.params if k not in state]
        unexpected = [k for k in state if k not in self.params]
        if strict and (missing or unexpected):
            raise KeyError(f"EMA state dict mismatch: missing {missing[:4]} unexpected {unexpected[:4]}")
        self.ema_attach()
        for k, p in self.params.items():
            if k in state:
                self.view(k, "ema").copy_(torch.as_tensor(state[k]).to(torch.float32).reshape(p["shape"]).to(self.device))
        if not missing:
            self.ema_live, self.ema_stale = True, False
        return missing, unexpected

    def await_params(self):
        """Make the current stream wait for the all-gather of the bf16 weights a sharded step left in flight (no-op otherwise)."""
        ev, self._params_ready = self._params_ready, None
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)

    def grads(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict((k, self.view(k, "grad")) for k in self.params)

    # ------------------------------------------------------------------ forward / backward / step
    @staticmethod
    def _i64(t, dev):
        return None if t is None else t.to(device=dev, dtype=torch.int64).contiguous()

    def _set_layout(self, att, num_tokens):
        """Token layout of the forward about to run.  `num_tokens`: a host int (real tokens of the batch, no device traffic), the
        string "auto" (the engine sums the key lengths of the 2-D device mask and reads the total back: 4 bytes + one stream
        synchronisation - what the model classes pass for a device-resident mask) or None (unknown: padded layout, the default of this
        low-level class).  GGET_VARLEN=0 keeps the padded layout whatever the caller passed; =sync counts even when the caller passed
        nothing; =nosync never counts on the device.  `self.varlen_mode` (the same strings; set through the model classes'
        `token_layout` attribute) overrides the environment for this engine."""
        import os
        mode = self.varlen_mode if self.varlen_mode is not None else os.environ.get("GGET_VARLEN", "")
        n = None if mode == "0" else num_tokens
        if n is None and mode == "sync":
            n = "auto"
        if n == "auto" and (mode == "nosync" or att is None or att.dim() != 2):
            n = None
        self.set_token_count(L.TOKENS_AUTO if n == "auto" else n)

    def forward_pretrain(self, input_ids, attention_mask, labels=None, sample_wgt=None, position_ids=None, num_tokens=None):
        self.await_params()
        dev = self.device
        ids = self._i64(input_ids, dev)
        if ids.dim() == 2:
            ids = ids[:, :, None].contiguous()
        B, S, F = ids.shape
        assert F == self.spec.stacked_feat, f"input_ids has {F} stacked features, model expects {self.spec.stacked_feat}"
        att = self._i64(attention_mask, dev)
        lab = self._i64(labels, dev)
        if lab is not None and lab.dim() == 2:
            lab = lab[:, :, None].contiguous()
        wgt = None if sample_wgt is None else sample_wgt.to(device=dev, dtype=torch.float32).contiguous()
        pos = self._i64(position_ids, dev)
        self._keep = (ids, att, lab, wgt, pos)
        self._set_layout(att, num_tokens)   # (full-logit inference runs var-len too since round 5: the logits keep their [B S F, V] cell order)
        if att is not None and att.dim() == 3:      # packed rows: block-diagonal [B,S,S] mask
            assert att.shape == (B, S, S), f"3-D attention mask must be [B,S,S], got {tuple(att.shape)}"
            fn = self.lib.gget_forward_pretrain_packed
        else:
            fn = self.lib.gget_forward_pretrain
        # (a fresh 1-element result tensor per call - a host-side allocator operation - instead of one buffer whose value every caller
        #  had to copy out with a kernel before the next step overwrote it)
        self._loss = torch.empty(1, dtype=torch.float32, device=dev)
        L.check(fn(self.h, _ptr(ids), _ptr(att), _ptr(lab), _ptr(wgt), _ptr(pos), B, S, _ptr(self._loss), _stream()))
        self._cl_keep = None
        return self._loss[0] if lab is not None else None

    # ------------------------------------------------------------------ contrastive head (KIND_PRETRAIN_CL)
    def _cl_view(self, getter, B: int) -> torch.Tensor:
        p = C.c_void_p()
        L.check(getter(self.h, C.byref(p)))
        off = p.value - self.workspace.data_ptr()
        return self.workspace[off: off + B * self.spec.hidden_size * 4].view(torch.float32).view(B, self.spec.hidden_size)

    def cl_logits(self, B: int) -> torch.Tensor:
        """fp32 [B,d] contrastive logits z = cl_proj(h at the pooled row) of the last forward (gget_cl_logits; a copy)."""
        return self._cl_view(self.lib.gget_cl_logits, B).clone()

    def cl_embeddings(self, B: int) -> torch.Tensor:
        """fp32 [B,d] L2-normalised embeddings of the last forward (gget_cl_embeddings; a view of the workspace)."""
        return self._cl_view(self.lib.gget_cl_embeddings, B)

    def cl_set_gathered(self, E: torch.Tensor, row_map: torch.Tensor):
        """Hand the embeddings of all ranks [N,d] and the positions of this rank's rows in them to the handle (gget_cl_set_gathered): the
        contrastive loss and its backward then run over the N rows.  Both tensors are kept alive until the next forward."""
        E = E.to(device=self.device, dtype=torch.float32).contiguous()
        row_map = row_map.to(device=self.device, dtype=torch.int32).contiguous()
        self._cl_keep = (E, row_map)
        L.check(self.lib.gget_cl_set_gathered(self.h, _ptr(E), int(E.shape[0]), _ptr(row_map), _stream()))

    def cl_loss(self) -> torch.Tensor:
        """The contrastive loss (ratio_dis applied) of the last forward, or of the gathered matrix set since (gget_cl_loss): a device scalar."""
        out = torch.empty(1, dtype=torch.float32, device=self.device)
        L.check(self.lib.gget_cl_loss(self.h, _ptr(out), _stream()))
        return out[0]

    def cl_set_backward_scales(self, generative: float = 1.0, contrastive: float = 1.0):
        """Upstream gradients of head1_loss / head2_loss for the NEXT backward (gget_cl_set_backward_scales); generative is 0 or 1."""
        L.check(self.lib.gget_cl_set_backward_scales(self.h, float(generative), float(contrastive)))

    def forward_task(self, input_ids, attention_mask, position_ids=None, task_labels=None, sample_wgt=None,
                     problem: int = L.PROBLEM_SINGLE_LABEL, num_tokens=None):
        self.await_params()
        dev = self.device
        ids = self._i64(input_ids, dev)
        if ids.dim() == 2:
            ids = ids[:, :, None]
        ids = ids[:, :, : self.spec.stacked_feat].contiguous()
        B, S, _ = ids.shape
        att = self._i64(attention_mask, dev)
        pos = self._i64(position_ids, dev)
        y = None
        if task_labels is not None:
            if problem in (L.PROBLEM_SINGLE_LABEL, L.PROBLEM_AUC, L.PROBLEM_TOKEN_CE, L.PROBLEM_TOKEN_CE_INTRA):
                y = task_labels.to(device=dev, dtype=torch.int64).contiguous()
            else:
                y = task_labels.to(device=dev, dtype=torch.float32).contiguous()
        wgt = None if sample_wgt is None else sample_wgt.to(device=dev, dtype=torch.float32).contiguous()
        if problem in (L.PROBLEM_TOKEN_CE, L.PROBLEM_TOKEN_CE_INTRA):   # token-level task: labels and logits per row
            assert y is None or tuple(y.shape) == (B, S), f"token-level labels must be [B,S], got {tuple(y.shape)}"
            logits = torch.empty(B, S, self.spec.num_labels, dtype=torch.float32, device=dev)
        else:
            logits = torch.empty(B, self.spec.num_labels, dtype=torch.float32, device=dev)
        hid = torch.empty(B, self.spec.hidden_size, dtype=torch.bfloat16, device=dev)
        self._keep = (ids, att, pos, y, wgt)
        self._set_layout(att, num_tokens)
        self._loss = torch.empty(1, dtype=torch.float32, device=dev)
        L.check(self.lib.gget_forward_task(self.h, _ptr(ids), _ptr(att), _ptr(pos), _ptr(y), _ptr(wgt), problem, B, S,
                                           _ptr(self._loss), _ptr(logits), _ptr(hid), _stream()))
        return (self._loss[0] if y is not None else None), logits, hid

    def set_dropout(self, attention_p: float = 0.0, path_p: float = 0.0, seed: int = 0):
        """Attention dropout / stochastic depth for the NEXT forward+backward (training mode); zeros = eval."""
        L.check(self.lib.gget_set_dropout(self.h, float(attention_p), float(path_p), int(seed) & 0xFFFFFFFF))

    def set_dropout_ex(self, embed_p: float = 0.0, mlp_p: float = 0.0, head_p: float = 0.0):
        """Embedding dropout, the two MLP dropouts and the MLP score head's dropout for the NEXT forward+backward (masks keyed
        by set_dropout's seed)."""
        L.check(self.lib.gget_set_dropout_ex(self.h, float(embed_p), float(mlp_p), float(head_p)))

    def debug_probe(self, enable: bool):
        """Measurement aid (gget_debug_probe): switch the in-step event probe on / off; returns the mean launch durations in ms
        recorded so far (grouped weight-gradient launch, gate|up + GEGLU launch)."""
        out = (C.c_float * 2)()
        L.check(self.lib.gget_debug_probe(self.h, int(bool(enable)), out))
        return float(out[0]), float(out[1])

    def set_focal_gamma(self, gamma: float = 0.0):
        """config.focal_gamma: > 0 = focal loss on the SMTP head (un-weighted path)."""
        L.check(self.lib.gget_set_focal_gamma(self.h, float(gamma)))

    def set_stack_method(self, stack_long: bool):
        """config.stack_method == "long": per-token 1/nnz embedding ratio + per-feature-level SMTP loss weights."""
        L.check(self.lib.gget_set_stack_method(self.h, int(bool(stack_long))))

    def set_raw_embeds(self, raw_embeds, first_label_only: bool = False):
        """inputs_raw_embeds [B,S,embed_dim] of the NEXT forward (config.embed_dim > 0); first_label_only = the smtp_inside mask rule."""
        if raw_embeds is None:
            self._raw_keep = None
            L.check(self.lib.gget_set_raw_embeds(self.h, None, 0))
            return
        assert raw_embeds.dim() == 3 and raw_embeds.shape[-1] == self.cfg.embed_dim, \
            f"inputs_raw_embeds must be [B,S,{self.cfg.embed_dim}], got {tuple(raw_embeds.shape)} (the [B,S,S,e] form is not supported)"
        self._raw_keep = raw_embeds.to(device=self.device, dtype=torch.float32).contiguous()
        L.check(self.lib.gget_set_raw_embeds(self.h, _ptr(self._raw_keep), int(bool(first_label_only))))

    def set_dp_menu(self, reserve_cus: int = 0, lds_headroom: bool = False):
        """The data-parallel share of the launch menu, carried by this handle (gget_set_dp_menu): (0, False) = the single-GPU selection."""
        L.check(self.lib.gget_set_dp_menu(self.h, int(reserve_cus), int(bool(lds_headroom))))

    def set_rope_range(self, rope_range: float):
        """config.rope_range: > 0 rescales the position ids of a forward to [0, rope_range) per row (per-token rotary angles)."""
        L.check(self.lib.gget_set_rope_range(self.h, float(rope_range)))

    def set_token_count(self, n_real_tokens: Optional[int]):
        """sum(attention_mask) of the NEXT forward's batch, when the host knows it: switches that step to the var-len (padding-free)
        token layout (gget_set_token_count).  None / 0 = unknown -> padded layout."""
        L.check(self.lib.gget_set_token_count(self.h, int(n_real_tokens or -1)))   # (L.TOKENS_AUTO = -2 passes through)

    def set_option(self, option: int, value: int):
        L.check(self.lib.gget_set_option(self.h, int(option), int(value)))

    def positions_clamped(self) -> bool:
        """True if a forward since the last call met position_ids outside [0, max_position) (they were clamped into the RoPE table);
        clears the flag; synchronises."""
        out = C.c_int32(0)
        L.check(self.lib.gget_position_status(self.h, C.byref(out), _stream()))
        return bool(out.value)

    def deferred_status(self):
        """(positions clamped, var-len token count / label mismatch) since the last call (gget_deferred_status); clears both; synchronises.
        `self.cls_idx_clamped` is set when a cls_idx of the intra-instance token head lay outside its sample since the last call."""
        out = (C.c_int32 * 2)()
        L.check(self.lib.gget_deferred_status(self.h, out, _stream()))
        self.cls_idx_clamped = bool(out[0] & 2)
        return bool(out[0] & 1), bool(out[1])

    def varlen_status(self):
        """(ran var-len, rows, count mismatch) of the last forward; synchronises."""
        out = (C.c_int32 * 3)()
        L.check(self.lib.gget_varlen_status(self.h, out, _stream()))
        return bool(out[0]), int(out[1]), bool(out[2])

    def set_cls_idx(self, cls_idx):
        """cls_idx [B] of the NEXT forward_task(problem=PROBLEM_TOKEN_CE_INTRA): the first label row inside every sample (gget_set_cls_idx).
        The tensor is kept alive until the next call; None clears it."""
        if cls_idx is None:
            self._cls_keep = None
            L.check(self.lib.gget_set_cls_idx(self.h, None))
            return
        self._cls_keep = cls_idx.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        L.check(self.lib.gget_set_cls_idx(self.h, _ptr(self._cls_keep)))

    def set_auc(self, num_neg: int = 1, seed: int = 0):
        """Negatives per positive and the sampling seed of the NEXT forward_task(problem=PROBLEM_AUC)."""
        L.check(self.lib.gget_set_auc(self.h, int(num_neg), int(seed) & 0xFFFFFFFF))

    def backward(self):
        L.check(self.lib.gget_backward(self.h, 1.0, _stream()))

    def backward_begin(self):
        L.check(self.lib.gget_backward_begin(self.h, 1.0, _stream()))

    def backward_layer(self, i: int):
        L.check(self.lib.gget_backward_layer(self.h, i, _stream()))

    def backward_end(self):
        L.check(self.lib.gget_backward_end(self.h, _stream()))

    def _adamw(self, entry, slots, lr, beta1, beta2, eps, weight_decay, max_grad_norm, grad_scale):
        """one optimizer step through `entry` (gget_adamw_step, or gget_adamw_step_sharded with the gathered partial vector `slots`):
        counts the step and returns the pre-clip gradient norm, a device scalar"""
        self.step_count += 1
        self._gnorm = torch.empty(1, dtype=torch.float32, device=self.device)     # (fresh per step: nothing to copy out, see forward_pretrain)
        L.check(entry(self.h, lr, beta1, beta2, eps, weight_decay, max_grad_norm, grad_scale, self.step_count, *slots, _ptr(self._gnorm),
                      _stream()))
        return self._gnorm[0]

    def adamw_step(self, lr, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1, max_grad_norm=1.0, grad_scale=1.0):
        return self._adamw(self.lib.gget_adamw_step, (), lr, beta1, beta2, eps, weight_decay, max_grad_norm, grad_scale)

    # ------------------------------------------------------------------ sharded optimizer step (ZeRO stage 2)
    @staticmethod
    def shard_plan_of(cfg, world: int, n_buckets: int):
        """[(offset, count, slice, tail_offset, tail_count)] of every bucket for `world` ranks (gget_shard_plan: the plan is defined once,
        in C, from the configuration alone)."""
        lib, out = L.load(), (C.c_uint64 * 5)()
        plan = []
        for b in range(n_buckets):
            L.check(lib.gget_shard_plan(C.byref(cfg), int(world), b, out))
            plan.append(tuple(int(x) for x in out))
        return plan

    def shard_init(self, world: int, rank: int):
        """Switch this handle to the sharded step of rank `rank` of `world` (gget_shard_init; world 0 = back to the replicated step)."""
        n = C.c_int32(0)
        L.check(self.lib.gget_shard_init(self.h, int(world), int(rank), C.byref(n)))
        if world <= 0:
            self.shard, self.shard_buckets, self.shard_slots = None, [], None
            return
        self.shard = (int(world), int(rank))
        out = (C.c_uint64 * 5)()     # the handle's plan: every bucket's trainable share cut for `world` ranks (gget_shard_bucket)
        self.shard_buckets = []
        for b in range(len(self.buckets)):
            L.check(self.lib.gget_shard_bucket(self.h, b, out))
            self.shard_buckets.append(tuple(int(x) for x in out))
        self.shard_slots = torch.zeros(int(world) * n.value, dtype=torch.float32, device=self.device)

    def reduce_scatter_grads_async(self, bucket: int, fp32_accumulate: bool = False, stream: Optional[torch.cuda.Stream] = None):
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        L.check(self.lib.gget_reduce_scatter_grads_async(self.h, int(bucket), int(bool(fp32_accumulate)), st))

    def shard_sqnorm_partials(self):
        L.check(self.lib.gget_shard_sqnorm_partials(self.h, _ptr(self.shard_slots), _stream()))

    def shard_allgather_async(self, what: int, stream: Optional[torch.cuda.Stream] = None):
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        L.check(self.lib.gget_shard_allgather_async(self.h, int(what), _ptr(self.shard_slots), st))

    def adamw_step_sharded(self, lr, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1, max_grad_norm=1.0, grad_scale=1.0):
        """clip + AdamW over this rank's share (gget_adamw_step_sharded); the partial vector must have been gathered.  Marks the fp32
        state stale (a world-1 plan owns everything and stays coherent)."""
        gnorm = self._adamw(self.lib.gget_adamw_step_sharded, (_ptr(self.shard_slots),), lr, beta1, beta2, eps, weight_decay, max_grad_norm,
                            grad_scale)
        if self.shard[0] > 1 and not getattr(self, "_loopback", False):    # (the loopback handle updates every rank's share itself)
            self.shard_stale = True
            self.ema_stale = self.ema is not None and self.ema_live
        return gnorm

    # ------------------------------------------------------------------ data-parallel exchange through the C ABI (RCCL)
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        L.check(L.load().gget_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        assert len(unique_id) == 128
        L.check(self.lib.gget_comm_init(self.h, int(rank), int(world), C.create_string_buffer(unique_id, 128)))
        self.comm_world = int(world)

    def comm_init_loopback(self, world: int):
        """A peer-less communicator (gget_comm_init_loopback): every all-reduce multiplies the range by `world` - the exchange schedule
        of a `world`-rank job on one GPU."""
        L.check(self.lib.gget_comm_init_loopback(self.h, int(world)))
        self.comm_world = int(world)
        self._loopback = True

    def comm_destroy(self):
        L.check(self.lib.gget_comm_destroy(self.h))
        self.comm_world = 0
        self._loopback = False

    def comm_adopt(self, other: "Engine"):
        """Take over `other`'s communicator (gget_comm_move): used when the model re-creates its engine with larger capacities,
        so that the ranks whose batch grew keep the communicator the other ranks still use (no collective re-init)."""
        if other.comm_world > 0:
            L.check(self.lib.gget_comm_move(self.h, other.h))
            self.comm_world, other.comm_world = other.comm_world, 0
            self._loopback, other._loopback = getattr(other, "_loopback", False), False

    def allreduce_grads_async(self, bucket: int = -1, fp32_accumulate: bool = False, stream: Optional[torch.cuda.Stream] = None):
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        L.check(self.lib.gget_allreduce_grads_async(self.h, int(bucket), int(bool(fp32_accumulate)), st))

    def allreduce_range_async(self, offset: int, count: int, fp32_accumulate: bool = False, stream: Optional[torch.cuda.Stream] = None):
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        L.check(self.lib.gget_allreduce_range_async(self.h, int(offset), int(count), int(bool(fp32_accumulate)), st))

    # ------------------------------------------------------------------ head outputs
    def head_counts(self):
        c = (C.c_int32 * 2)()
        L.check(self.lib.gget_head_counts(self.h, C.byref(c), _stream()))
        return int(c[0]), int(c[1])

    def head_logits(self) -> torch.Tensor:
        """bf16 [Lm, V] logits of the last pre-train forward (a copy)."""
        _, lm = self.head_counts()
        p, ld = C.c_void_p(), C.c_int32()
        L.check(self.lib.gget_head_logits(self.h, C.byref(p), C.byref(ld)))
        off = p.value - self.workspace.data_ptr()
        raw = self.workspace[off: off + lm * ld.value * 2].view(torch.bfloat16).view(lm, ld.value)
        return raw[:, : self.spec.vocab_size].clone()

    def token_confidence(self, rows: int, mode: int = 0):
        """Arg-max token and unmasking confidence of the first `rows` rows of the head logits of the last forward, computed
        in place on the workspace (no copy of the [rows, V] logits): (conf f32 [rows], token i64 [rows])."""
        p, ld = C.c_void_p(), C.c_int32()
        L.check(self.lib.gget_head_logits(self.h, C.byref(p), C.byref(ld)))
        conf = torch.empty(rows, dtype=torch.float32, device=self.device)
        tok = torch.empty(rows, dtype=torch.int64, device=self.device)
        L.check(self.lib.gget_op_token_confidence(p, ld.value, int(rows), self.spec.vocab_size, int(mode), _ptr(conf), _ptr(tok),
                                                  _stream()))
        return conf, tok

    def hidden_states(self, B: int, S: int) -> torch.Tensor:
        """bf16 [B,S,d] final-normed hidden states of the last forward (a copy; either token layout - gget_hidden_states_grid)."""
        return self._hidden_grid(-1, B, S)

    def layer_hidden_states(self, layer: int, B: int, S: int) -> torch.Tensor:
        """bf16 [B,S,d] residual stream entering decoder layer `layer` (num_layers = leaving the last one) of the last forward (a copy)."""
        return self._hidden_grid(int(layer), B, S)

    def attention_probs(self, layer: int, B: int, S: int, apply_dropout: bool = False) -> torch.Tensor:
        """bf16 [B,H,S,S] attention weights of decoder layer `layer` of the last forward (gget_attention_probs: recomputed from the layer's
        rotated q | k and log-sum-exp; either token layout, packed rows too).  apply_dropout: with that forward's dropout mask applied."""
        out = torch.empty(B, self.spec.num_heads, S, S, dtype=torch.bfloat16, device=self.device)
        L.check(self.lib.gget_attention_probs(self.h, int(layer), _ptr(out), int(bool(apply_dropout)), _stream()))
        return out

    def layer_qkv(self, layer: int, B: int, S: int) -> torch.Tensor:
        """bf16 [B,S,3d] rotated q | k | v of decoder layer `layer` of the last forward (a copy; either token layout; zeros behind a
        sample's tokens - gget_layer_qkv_grid)."""
        out = torch.empty(B, S, 3 * self.spec.hidden_size, dtype=torch.bfloat16, device=self.device)
        L.check(self.lib.gget_layer_qkv_grid(self.h, int(layer), _ptr(out), _stream()))
        return out

    def _hidden_grid(self, layer: int, B: int, S: int) -> torch.Tensor:
        out = torch.empty(B, S, self.spec.hidden_size, dtype=torch.bfloat16, device=self.device)
        L.check(self.lib.gget_hidden_states_grid(self.h, layer, _ptr(out), _stream()))
        return out
