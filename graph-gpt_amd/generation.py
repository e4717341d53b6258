"""Iterative unmasking generation (MaskGIT / dLLM style) on top of the pre-train forward - SURVEY.md next item N3.

Restates the reference's `sample_per_batch` + `_batch_unmask_without_for_loop` + `sample_tokens`
(src/utils/generation_utils.py:22-237) with every setting: `alg` in {"origin", "maskgit_plus", "topk_margin", "entropy"},
candidate temperature / top-p / top-k, Gumbel-perturbed ranking (`alg_temp`).  Each iteration is one forward with
`labels=None` (logits for all B*S*F feature tokens stay in the engine's workspace), one pass of the HIP sampling kernel
(`gget_op_token_sample`: filters, softmax, candidate, confidence, Gumbel noise) over those logits, and either the "origin"
update kernel (`gget_op_unmask_origin`) or a per-sample ranking on the [B, S*F] confidences.

Randomness: where the reference draws from torch's global RNG (Categorical.sample, torch.rand, torch.rand_like) the kernels use
a counter hash of (seed, iteration, stream, row / cell) - the same scheme as the SMTP masking kernels - so a run is a pure
function of `GenerationConfig.seed` and `draws()` below regenerates the uniforms bit-exactly for the parity tests.

One deliberate difference: the reference scatters a fixed k = max_b(n_reveal[b]) positions per sample and writes <mask> over
the surplus; when k exceeds a sample's masked count the surplus targets are already-revealed positions picked by torch.topk's
tie order among -inf confidences (device dependent), i.e. it re-masks arbitrary known tokens.  Here only the first
n_reveal[b] ranked positions of a sample are written (ranking = stable descending sort: ties go to the lower index), which
is deterministic on every device and never destroys revealed tokens.

Where the update runs: the ranked algorithms' step rule and reveal are two HIP launches per iteration (`gget_op_gen_plan`: batch
maximum of the masked counts -> i, p; `gget_op_unmask_ranked`: radix select of the floor(n_masked * p) most confident masked cells
of every sample), x / conf / cand never leave the device, nothing is sorted, and the loop reads one pinned {i, any_masked} pair
(8 bytes) per iteration to know when to stop.  `unmask_step` / `reveal_counts` below stay as the torch statement of the same rule:
GGET_GEN_DEVICE=0 selects them (the tests compare the two paths token by token).

The evaluation built on the sampler (reference src/utils/log_eval_dump_utils.py:308-447): `evaluate_generation` sweeps ten mask-rate
bands and averages per-sample reconstruction accuracy, through `eval_gen_per_batch` (`parallel_gen=True`) or `eval_gen_per_sample`
(the reference's default).  `sample_per_example` follows the reference's per-sample schedule (:317-436: steps_b = min(n_masked_b,
steps), the sample's own linspace(1, eps, steps_b + 1), no skip rule, the transfer count from the sample's current masked count) but
runs it for the whole batch at once - max_b steps_b forwards instead of sum_b steps_b - with a [max_steps, B] table of per-sample p
(0 for a finished sample) and no host read inside the loop; the var-len layout keeps right-padded samples independent.  Two
deliberate differences of that path:
  * with alg_temp > 0 the reference draws torch.multinomial without replacement from softmax(conf / alg_temp); here the ranking is
    Gumbel-top-k on conf / alg_temp (the sampling kernel's perturbation) - the same distribution, a different draw;
  * the "origin" transfer draws are indexed by (sample, cell) of the padded batch, not drawn per masked cell in order.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .conf import _get, _set
from .dp import dist_ready
from .smtp import _rng24

_MODES = {"origin": 0, "maskgit_plus": 0, "topk_margin": 1, "entropy": 2}   # GGET_CONF_* of include/gget.h


@dataclasses.dataclass
class GenerationConfig:
    """Fields of the reference's `GenerationConfig` (src/conf/generation/generation_configs.py) that the loop reads, plus the
    seed of the counter-hash draws."""
    alg: str = "maskgit_plus"
    alg_temp: Optional[float] = None
    steps: int = 512
    eps: float = 1e-3
    temperature: float = 0.0
    top_p: Optional[float] = None
    top_k: Optional[int] = None
    output_history: bool = False
    mask_token_id: int = 1
    seed: int = 0
    parallel_gen: bool = False      # generation_configs.py:43: False = the per-example schedule (`eval_gen_per_sample`)
    pad_token_id: int = 0

    def validate(self):
        if self.alg not in _MODES:
            raise ValueError(f"alg={self.alg!r}: expected one of {sorted(_MODES)}")
        if self.temperature is not None and self.temperature < 0:
            raise ValueError("temperature must be >= 0")


def iteration_seed(seed: int, iteration: int) -> int:
    return (int(seed) * 0x9E3779B1 + (int(iteration) + 1) * 0x85EBCA6B) & 0xFFFFFFFF


def draws(seed: int, iteration: int, B: int, N: int):
    """Python twin of the kernels' draws of one iteration: (u_categorical [B*N], u_gumbel [B*N], u_transfer [B, N]) fp32."""
    s = iteration_seed(seed, iteration)
    inv = np.float32(1.0 / 16777216.0)
    rows = np.arange(B * N)
    u_cat = _rng24(s, 32, rows, 0).astype(np.float32) * inv
    u_gum = _rng24(s, 33, rows, 0).astype(np.float32) * inv
    u_tr = (_rng24(s, 34, np.arange(B)[:, None], np.arange(N)[None, :]).astype(np.float32) * inv)
    T = torch.from_numpy
    return T(u_cat), T(u_gum), T(u_tr)


def token_sample(engine, rows: int, cfg: GenerationConfig, seed: int, gumbel: bool):
    """Candidates and confidences of the first `rows` rows of the head logits of the last forward (in place on the
    workspace): (conf f32 [rows], token i64 [rows])."""
    p, ld = C.c_void_p(), C.c_int32()
    L.check(engine.lib.gget_head_logits(engine.h, C.byref(p), C.byref(ld)))
    conf = torch.empty(rows, dtype=torch.float32, device=engine.device)
    tok = torch.empty(rows, dtype=torch.int64, device=engine.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    top_p = float(cfg.top_p) if (cfg.top_p is not None and cfg.top_p < 1) else 0.0
    top_k = int(cfg.top_k) if cfg.top_k is not None else 0
    alg_temp = float(cfg.alg_temp) if (gumbel and cfg.alg_temp is not None and cfg.alg_temp > 0) else 0.0
    L.check(engine.lib.gget_op_token_sample(p, ld.value, int(rows), engine.spec.vocab_size, _MODES[cfg.alg],
                                            float(cfg.temperature or 0.0), top_p, top_k, alg_temp, int(seed) & 0xFFFFFFFF,
                                            C.c_void_p(conf.data_ptr()), C.c_void_p(tok.data_ptr()), st))
    return conf, tok


def reveal_counts(x: torch.Tensor, timesteps: torch.Tensor, i: int, mask_token_id: int):
    """Step bookkeeping of the confidence-ranked algorithms (reference :166-178): advance i until some sample may reveal at
    least one token; returns (n_reveal int32 [B], k, i)."""
    steps = len(timesteps) - 1
    n_masked = (x == mask_token_id).sum(dim=1)
    k = 0
    n_reveal = torch.zeros_like(n_masked, dtype=torch.int32)
    if int(n_masked.sum().item()) > 0:
        while k == 0 and i < steps:
            t, s = timesteps[i], timesteps[i + 1]
            p = 1 - s / t if i < steps - 1 else 1.0
            n_reveal = torch.floor(n_masked * p).int()
            k = int(n_reveal.max().item())
            i += 1
    return n_reveal, k, i


def unmask_step(x: torch.Tensor, conf: torch.Tensor, cand: torch.Tensor, timesteps: torch.Tensor, i: int,
                cfg: GenerationConfig) -> Tuple[torch.Tensor, int]:
    """One confidence-ranked update (reference :163-236): x [B, N] tokens, conf / cand [B, N] from the sampling kernel.
    Every sample reveals its floor(n_masked * p) most confident masked positions (see the module docstring for the one
    difference from the reference's fixed-k scatter)."""
    n_reveal, k, i = reveal_counts(x, timesteps, i, cfg.mask_token_id)
    if k == 0:
        return x, i
    masked = x == cfg.mask_token_id
    conf = conf.masked_fill(~masked, float("-inf"))
    order = torch.sort(conf, dim=1, descending=True, stable=True).indices[:, :k]     # [B, k] most confident first
    new = torch.gather(cand, 1, order)
    keep = torch.arange(k, device=x.device)[None, :] < n_reveal[:, None]
    old = torch.gather(x, 1, order)
    x = x.scatter(1, order, torch.where(keep, new, old))
    return x, i


def device_update_enabled() -> bool:
    """GGET_GEN_DEVICE=0 runs the ranked update through the torch statement (`unmask_step`) instead of the two HIP launches."""
    return os.environ.get("GGET_GEN_DEVICE", "1") != "0"


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def step_p_table(timesteps: torch.Tensor) -> torch.Tensor:
    """p of every step of one time grid (reference :177-178): 1 - t[i+1] / t[i], the last entry 1.0; fp32 on the grid's device."""
    p = 1 - timesteps[1:] / timesteps[:-1]
    if p.numel():
        p[-1] = 1.0
    return p.contiguous()


def unmask_ranked(lib, x: torch.Tensor, conf: torch.Tensor, cand: torch.Tensor, mask_token_id: int, p: torch.Tensor,
                  n_revealed: Optional[torch.Tensor] = None):
    """`gget_op_unmask_ranked` on x [B, N] (in place): p is a device fp32 tensor of 1 element (the batch's p) or B elements."""
    B, N = x.shape
    assert x.is_contiguous() and conf.is_contiguous() and cand.is_contiguous() and p.dtype == torch.float32 and p.is_contiguous()
    assert conf.dtype == torch.float32 and x.dtype == torch.int64 and cand.dtype == torch.int64
    assert p.numel() in (1, B), f"p has {p.numel()} elements for a batch of {B}"
    L.check(lib.gget_op_unmask_ranked(_ptr(x), _ptr(conf), _ptr(cand), B, N, int(mask_token_id), _ptr(p), 0 if p.numel() == 1 else 1,
                                      _ptr(n_revealed), _stream()))


class _Plan:
    """Device state of the batch step rule (`gget_op_gen_plan`): the p table, i, the p of the step in flight and the pinned
    {i, any_masked} pair the host reads once per iteration."""

    def __init__(self, lib, timesteps: torch.Tensor):
        dev = timesteps.device
        self.lib, self.p_tab = lib, step_p_table(timesteps)
        self.steps = int(self.p_tab.numel())
        self.i = torch.zeros(1, dtype=torch.int32, device=dev)
        self.p = torch.zeros(1, dtype=torch.float32, device=dev)
        self.pair = torch.zeros(2, dtype=torch.int32).pin_memory()

    def launch(self, x: torch.Tensor, mask_token_id: int):
        B, N = x.shape
        L.check(self.lib.gget_op_gen_plan(_ptr(x), B, N, int(mask_token_id), _ptr(self.p_tab), self.steps, _ptr(self.i), _ptr(self.p),
                                          _ptr(self.pair), _stream()))

    def read(self) -> Tuple[int, bool]:
        """The one host read of an iteration: waits for the stream, then the 8 pinned bytes."""
        torch.cuda.current_stream().synchronize()
        i, any_masked = self.pair.tolist()
        return int(i), bool(any_masked)


@torch.no_grad()
def sample_per_batch(model, cfg: GenerationConfig, *, input_ids: torch.Tensor, attention_mask: torch.Tensor,
                     inputs_raw_embeds=None) -> Tuple[torch.Tensor, Optional[List[torch.Tensor]]]:
    """Fill the `<mask>` cells of input_ids [B, S, F].  Returns (tokens [B, S*F], history or None)."""
    cfg = as_generation_config(cfg)
    cfg.validate()
    assert input_ids.dim() == 3, "expect [bz, seq, next_n]"
    assert inputs_raw_embeds is None
    model.eval()
    B, S, F = input_ids.shape
    dev = torch.device("cuda", torch.cuda.current_device())
    x = input_ids.to(dev).reshape(B, S * F).clone()
    att = attention_mask.to(dev)
    n_steps = min(int((x == cfg.mask_token_id).sum(dim=-1).max().item()), cfg.steps)
    timesteps = torch.linspace(1, cfg.eps, n_steps + 1, device=dev)
    history = [] if cfg.output_history else None
    lib = model._engine.lib
    plan = _Plan(lib, timesteps) if (cfg.alg != "origin" and device_update_enabled()) else None
    i = it = 0
    while i < n_steps:
        model(input_ids=x.view(B, S, F), attention_mask=att, labels=None)      # logits for all B*S*F rows, in the workspace
        seed = iteration_seed(cfg.seed, it)
        conf, cand = token_sample(model._engine, B * S * F, cfg, seed, gumbel=cfg.alg != "origin")
        any_masked = True
        if cfg.alg == "origin":
            t, s = timesteps[i], timesteps[i + 1]
            p_transfer = float(1 - s / t) if i < n_steps - 1 else 1.0
            L.check(lib.gget_op_unmask_origin(C.c_void_p(x.data_ptr()), C.c_void_p(cand.data_ptr()), B, S * F,
                                              p_transfer, seed, int(cfg.mask_token_id), _stream()))
            i += 1
        elif plan is not None:
            plan.launch(x, cfg.mask_token_id)
            unmask_ranked(lib, x, conf.view(B, S * F), cand.view(B, S * F), cfg.mask_token_id, plan.p)
            i, any_masked = plan.read()
        else:
            x, i = unmask_step(x, conf.view(B, S * F), cand.view(B, S * F), timesteps, i, cfg)
        it += 1
        if history is not None:
            history.append(x.view(B, S, F).clone())
        if not any_masked:        # nothing left to fill: the torch rule would not advance i either
            break
    return x, history


def example_p_table(n_masked, steps: int, eps: float) -> torch.Tensor:
    """Per-sample p of every iteration of the per-example schedule (reference :350-354, :380, :402-407), fp32 [max_steps, B] on
    the host: sample b runs steps_b = min(n_masked[b], steps) iterations on its own linspace(1, eps, steps_b + 1) with
    p = 1 - t[j+1] / t[j], 1.0 in its last iteration and 0 once it has finished."""
    steps_b = [min(int(n), int(steps)) for n in n_masked]
    tab = torch.zeros(max(steps_b, default=0), len(steps_b), dtype=torch.float32)
    for b, sb in enumerate(steps_b):
        if sb > 0:
            tab[:sb, b] = step_p_table(torch.linspace(1, eps, sb + 1))
    return tab


@torch.no_grad()
def sample_per_example(model, cfg: GenerationConfig, *, input_ids: torch.Tensor, attention_mask: torch.Tensor,
                       inputs_raw_embeds=None) -> Tuple[torch.Tensor, Optional[List[torch.Tensor]]]:
    """The reference's per-sample schedule (src/utils/generation_utils.py:317-436) for a whole batch at once.  input_ids
    [B, S, F] with attention_mask [B, S], or the reference's signature: input_ids [S, F] with attention_mask [1, S] (a batch of
    one).  Returns (tokens [B, S*F], history or None); see the module docstring for the two deliberate differences."""
    cfg = as_generation_config(cfg)
    cfg.validate()
    assert inputs_raw_embeds is None
    if input_ids.dim() == 2:
        input_ids = input_ids.unsqueeze(0)
        attention_mask = attention_mask.reshape(1, -1)
    assert input_ids.dim() == 3, "expect [seq, next_n] or [bz, seq, next_n]"
    model.eval()
    B, S, F = input_ids.shape
    N = S * F
    dev = torch.device("cuda", torch.cuda.current_device())
    x = input_ids.to(dev).reshape(B, N).clone()
    att = attention_mask.to(dev)
    p_tab = example_p_table((x == cfg.mask_token_id).sum(dim=-1).tolist(), cfg.steps, cfg.eps).to(dev)
    history = [] if cfg.output_history else None
    lib = model._engine.lib
    for it in range(p_tab.shape[0]):
        model(input_ids=x.view(B, S, F), attention_mask=att, labels=None)
        seed = iteration_seed(cfg.seed, it)
        conf, cand = token_sample(model._engine, B * N, cfg, seed, gumbel=cfg.alg != "origin")
        if cfg.alg == "origin":
            L.check(lib.gget_op_unmask_origin_rows(_ptr(x), _ptr(cand), B, N, _ptr(p_tab[it]), seed, int(cfg.mask_token_id), _stream()))
        else:
            unmask_ranked(lib, x, conf.view(B, N), cand.view(B, N), cfg.mask_token_id, p_tab[it])
        if history is not None:
            history.append(x.clone())
    return x, history


def gen_acc_counts(mask_token_id: int, input_ids: torch.Tensor, labels: torch.Tensor, gen_res: torch.Tensor) -> torch.Tensor:
    """`gget_op_gen_acc`: i32 [B, 2] = per sample {correct masked cells, masked cells}; input_ids / labels [B, ...], gen_res [B, N]."""
    if not input_ids.is_cuda:
        raise L.GgetError("generation accuracy counts run on the GPU only (their CPU statement is test infrastructure)")
    B = input_ids.shape[0]
    ids = input_ids.reshape(B, -1).contiguous()
    lab = labels.to(ids.device).reshape(B, -1).contiguous()
    gen = gen_res.to(ids.device).reshape(B, -1).contiguous()
    assert ids.shape == lab.shape == gen.shape and ids.dtype == lab.dtype == gen.dtype == torch.int64
    counts = torch.empty(B, 2, dtype=torch.int32, device=ids.device)
    L.check(L.load().gget_op_gen_acc(_ptr(gen), _ptr(lab), _ptr(ids), B, ids.shape[1], int(mask_token_id), _ptr(counts), _stream()))
    return counts


def cal_gen_acc_batch(gen_cfg, input_ids, labels, gen_res) -> torch.Tensor:
    """reference generation_utils.py:448-463: per-sample share of the masked cells of input_ids [B, S, F] that gen_res [B, S*F]
    rebuilt, fp32 [B]; 0 / 0 = NaN for a sample without a masked cell, as in the reference."""
    c = gen_acc_counts(_get(gen_cfg, "mask_token_id", 1), input_ids, labels, gen_res)
    return c[:, 0].float() / c[:, 1].float()


def cal_gen_acc_per_sample(gen_cfg, input_ids, labels, gen_res) -> torch.Tensor:
    """reference generation_utils.py:439-445: one sample, input_ids / labels [S, F], gen_res [S*F] or [1, S*F]; a 0-dim fp32."""
    return cal_gen_acc_batch(gen_cfg, input_ids.unsqueeze(0), labels.unsqueeze(0), gen_res.reshape(1, -1))[0]


def eval_gen_per_batch(model, cfg, *, input_ids, attention_mask, labels, inputs_raw_embeds=None) -> torch.Tensor:
    """reference log_eval_dump_utils.py:387-406: `sample_per_batch`, then the per-sample accuracies [B]."""
    gen_res, _ = sample_per_batch(model, cfg, input_ids=input_ids, attention_mask=attention_mask, inputs_raw_embeds=inputs_raw_embeds)
    return cal_gen_acc_batch(cfg, input_ids.to(gen_res.device), labels, gen_res)


def eval_gen_per_sample(model, cfg, *, input_ids, attention_mask, labels, inputs_raw_embeds=None) -> torch.Tensor:
    """reference log_eval_dump_utils.py:409-447 without its loop over the samples: `sample_per_example` on the batch (every
    sample on its own schedule), then the count kernel.  Padding cells are never <mask>, so they count nowhere."""
    gen_res, _ = sample_per_example(model, cfg, input_ids=input_ids, attention_mask=attention_mask, inputs_raw_embeds=inputs_raw_embeds)
    return cal_gen_acc_batch(cfg, input_ids.to(gen_res.device), labels, gen_res)


def as_generation_config(gen_cfg) -> GenerationConfig:
    """A `GenerationConfig` from whatever `cfg.generation` is: ours, the reference's dataclass / DictConfig, or a dict."""
    if isinstance(gen_cfg, GenerationConfig):
        return gen_cfg
    kw = {f.name: _get(gen_cfg, f.name, f.default) for f in dataclasses.fields(GenerationConfig)}
    return GenerationConfig(**kw)


GEN_EVAL_INTERVALS = 10


@torch.no_grad()
def evaluate_generation(model, loader, eval_name: str = "valid", do_eval: bool = True, cfg=None) -> str:
    """reference log_eval_dump_utils.evaluate_generation (:308-384): ten mask-rate bands from np.linspace(0.01, 0.99, 11), each
    written into cfg.training.pretrain_mlm.params.umr_clip BEFORE the loader is iterated (the loader masks from it) and restored
    afterwards; per band the per-sample accuracies of every batch (`eval_gen_per_batch` if parallel_gen else `eval_gen_per_sample`)
    are summed, for world > 1 the [10] sums and the sample counts of all ranks are gathered, and the averages come back as the
    comma-joined 4-decimal string of result.csv's gen_acc columns.  Returns "" when do_eval is false; leaves the model in train mode."""
    if not do_eval:
        return ""
    world = torch.distributed.get_world_size() if dist_ready() else 1
    model.eval()
    device = model.device
    gen_raw = _get(cfg, "generation")
    _set(gen_raw, "output_history", False)
    gen_cfg = as_generation_config(gen_raw)
    gen_cfg.validate()
    params = _get(_get(_get(cfg, "training"), "pretrain_mlm"), "params")
    default_umr_clip = list(_get(params, "umr_clip"))
    sp = np.linspace(0.01, 0.99, num=GEN_EVAL_INTERVALS + 1)
    acc_mat = []
    try:
        for j in range(GEN_EVAL_INTERVALS):
            _set(params, "umr_clip", [float(sp[j]), float(sp[j + 1])])
            for data in loader:
                assert "embed" not in data, "raw-embedding generation is not supported"
                eval_func = eval_gen_per_batch if gen_cfg.parallel_gen else eval_gen_per_sample
                acc_mat.append(eval_func(model, gen_cfg, input_ids=data["input_ids"].to(device),
                                         attention_mask=data["attention_mask"].to(device), labels=data["labels"].to(device),
                                         inputs_raw_embeds=None))
    finally:
        _set(params, "umr_clip", default_umr_clip)
    if not acc_mat:
        raise ValueError(f"evaluate_generation: the {eval_name} loader yielded no batch")
    acc_mat = torch.hstack(acc_mat).reshape((GEN_EVAL_INTERVALS, -1)).T          # [samples, intervals]
    acc_sum = acc_mat.float().sum(dim=0)
    num_samp = torch.tensor([acc_mat.shape[0]], dtype=acc_sum.dtype, device=acc_sum.device)
    if world > 1:
        dist = torch.distributed
        gdev = device if dist.get_backend() == "nccl" else torch.device("cpu")
        sums = [torch.zeros(GEN_EVAL_INTERVALS, dtype=acc_sum.dtype, device=gdev) for _ in range(world)]
        nums = [torch.zeros(1, dtype=acc_sum.dtype, device=gdev) for _ in range(world)]
        dist.all_gather(sums, acc_sum.to(gdev))
        dist.all_gather(nums, num_samp.to(gdev))
        acc_sum, num_samp = torch.stack(sums).sum(dim=0), torch.stack(nums).sum()
    acc_avg = (acc_sum / num_samp).cpu().numpy()
    model.train()
    return ",".join(acc_avg.round(4).astype(str))
