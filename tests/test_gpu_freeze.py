"""`training.finetune.freeze = k` on the device (reference freeze_llama_layers, src/utils/modules_utils.py:45-54): embed_tokens and the
first k layers are not trained.  Model: GraphGPTTaskModel d128 / H2 / ff512, L = 3 (an interior boundary, k = L and k > L), F 4, V 300,
seeded weights; variants plain, LayerScale (the has_res / fused-LS backward) and gated aggregation (a trainable parameter upstream of
layer 0: the backward is NOT truncated).  Batches B 8 / S 32 (the per-sample fused kernels) and B 4 / S 72 (the three-launch path).

1. gradients  - every trainable parameter's bf16 gradient against the never-frozen engine on the same weights and batch.  The decoder
   layers' 2-D weights (written by GEMMs) bit for bit.  The parameters summed in the fp32 scratch - the norm weights, lambda_1/2, the gate
   and, in this model kind, score.weight (k_score_bwd adds it with fp32 atomics: an fp32-accumulated small parameter like the others) -
   may differ by summation order only, since the boundary kernel sums the norm weight gradient in another order.  Their bound is
   measured from EXISTING code: D = the largest per-element difference of those parameters between two never-frozen runs on the same
   input, one under KEY_DETERMINISTIC and one without; allowed: 4 D + one bf16 ulp of the value.
2. truncation - a finite sentinel written into the frozen ranges of the gradient array before the backward is still there afterwards
   (plain, LayerScale; the gated variant runs the full chain).
3. step       - inf in a frozen gradient element, a finite norm, master / m / v / bf16 copy of the trainable ranges per element against the
   float64 restatement (tests/_adamw_ref.py verify_step, unchanged) with the norm rebuilt from the trainable gradients only, the clip
   active; the frozen ranges of master, m, v, bf16 copy and EMA bit-identical over three steps; every launch form.
4. surface    - TrainingPipeline with finetune.freeze = 1, requires_grad / .grad, a re-created engine, save / load / continue, ema_weights.
5. default    - freeze = -1 equals a model that never heard of freezing."""
import copy
import importlib
import os
import types

import numpy as np
import pytest
import torch

import _adamw_ref as R
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
M = importlib.import_module("graph-gpt_amd.modeling")
T = importlib.import_module("graph-gpt_amd.training")
synth = importlib.import_module("graph-gpt_amd.synth")

NL = 3
CFG = dict(hidden_act="gelu", vocab_size=300, hidden_size=128, intermediate_size=512, num_hidden_layers=NL, num_attention_heads=2,
           max_position_embeddings=128, causal_attention=False, stacked_feat=4, num_labels=2)
VARIANTS = {"plain": {}, "ls": {"layer_scale_init_value": 1.0}, "gated": {"stacked_feat_agg_method": "gated"}}
SHAPES = {"b8s32": (8, 32), "b4s72": (4, 72)}
KS = (0, 1, 2, 3, 5)
SENTINEL = 3.0
_DP_ENV = ("GGET_DP_BACKEND", "GGET_DP_LOOPBACK_WORLD", "GGET_FORCE_STAGED", "GGET_ZERO_STAGE", "GGET_DP_FP32_REDUCE", "GGET_NORM_FROM_BACKWARD")


def _batch(shape, seed=5):
    B, S = SHAPES[shape]
    return {k: torch.from_numpy(v) for k, v in synth.make_task_batch(B=B, S=S, F=4, V=300, seed=seed).items() if k != "lengths"}


def _make(monkeypatch, variant="plain", k=-1, layout="auto", world=0, zero=0, fold=False, **optim):
    for name in _DP_ENV:
        monkeypatch.delenv(name, raising=False)
    if world:
        monkeypatch.setenv("GGET_DP_BACKEND", "abi")
        monkeypatch.setenv("GGET_DP_LOOPBACK_WORLD", str(world))
        monkeypatch.setenv("GGET_FORCE_STAGED", "1")
        monkeypatch.setenv("GGET_ZERO_STAGE", str(zero))
    if fold:
        monkeypatch.setenv("GGET_NORM_FROM_BACKWARD", "1")
    model = M.GraphGPTTaskModel(M.GraphGPTConfig(**CFG, **VARIANTS[variant]), seed=7).cuda().eval()
    model.token_layout = layout
    if k >= 0:
        model.freeze_layers(k)
    eng = T.initialize(model, T.OptimConfig(**{"lr": 1e-3, "max_grad_norm": 1.0, **optim}))
    assert eng.sharded == (zero > 0)
    return model, eng


def _finish(model):
    e = model._engine
    if e is not None and e.comm_world:
        e.comm_destroy()


def _fwd_bwd(eng, b, before_backward=None):
    out = eng(input_ids=b["input_ids"], attention_mask=b["attention_mask"], position_ids=b["position_ids"], task_labels=b["task_labels"])
    if before_backward is not None:
        before_backward(eng.module._engine)
    eng.backward(out.task_loss)
    torch.cuda.synchronize()            # (every stream: a loopback exchange runs on the side stream)
    return out.task_loss


def _mask(e, names):
    m = torch.zeros(e.n_params, dtype=torch.bool, device="cuda")
    for n in names:
        p = e.params[n]
        m[p["offset"]: p["offset"] + p["numel"]] = True
    return m


def _train_mask(e):
    m = torch.zeros(e.n_params, dtype=torch.bool, device="cuda")
    for off, cnt in e.train_ranges:
        m[off: off + cnt] = True
    return m


def _ulp_bf16(v):
    a = v.abs().double()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(1e-300))) - 7), torch.zeros_like(a))


# ------------------------------------------------------------------------------------------------ the plan, read back from the handle
@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("frozen", [-1, 0, 1, 2])
def test_shard_plan_of_the_handle_follows_the_written_rule(frozen, world):
    """gget_bucket_train_range = the intersection of gget_bucket_range with gget_trainable_ranges, and gget_shard_bucket = that share cut
    into `world` slices of whole GGET_SHARD_CHUNK chunks plus a tail - the rule written out here, with no device arithmetic.  The tiny
    pre-train model (2 layers: frozen = 2 is num_layers) with gated aggregation: two trainable ranges, a partial embedding bucket."""
    import ctypes as C
    spec_mod = importlib.import_module("graph-gpt_amd.spec")
    spec = spec_mod.spec_from_size("tiny", vocab_size=756, stacked_feat=13, next_n_token=13, gated_agg=True)
    assert spec.num_layers == 2
    e = importlib.import_module("graph-gpt_amd.engine").Engine(spec, max_tokens=256, max_batch=8)
    e.comm_init_loopback(world)
    e.set_frozen(frozen)
    e.shard_init(world, 0)
    if frozen >= 0:
        assert len(e.train_ranges) == 2 and e.train_ranges[0][1] > 0
    out, o, c = (C.c_uint64 * 5)(), C.c_uint64(), C.c_uint64()
    partial = 0
    for b, (lo, cnt) in enumerate(e.buckets):
        meet = [(max(lo, off), min(lo + cnt, off + n)) for off, n in e.train_ranges]
        meet = [(a, z - a) for a, z in meet if a < z]
        assert len(meet) <= 1
        want = meet[0] if meet else (lo, 0)
        L.check(e.lib.gget_bucket_train_range(e.h, b, C.byref(o), C.byref(c)))
        assert (o.value, c.value) == want == e.bucket_train_range(b)
        partial += 0 < want[1] < cnt
        off, n = want
        sl = n // (world * R.SHARD_CHUNK) * R.SHARD_CHUNK
        L.check(e.lib.gget_shard_bucket(e.h, b, out))
        assert tuple(out) == (off, n, sl, off + world * sl, n - world * sl) == e.shard_buckets[b]
        if frozen < 0:
            L.check(e.lib.gget_shard_plan(C.byref(e.cfg), world, b, out))
            assert tuple(out) == e.shard_buckets[b]
    assert partial == (1 if frozen >= 0 else 0)         # (the embedding bucket keeps its gate parameters only)
    e.comm_destroy()


# ------------------------------------------------------------------------------------------------ the never-frozen reference, once
_REF = {}


def _reference(monkeypatch, variant, shape, layout):
    """(gradient array of the never-frozen engine, D): computed once per (variant, shape, layout) and left unchanged"""
    key = (variant, shape, layout)
    if key not in _REF:
        b = _batch(shape)
        runs = []
        for det in (0, 1):
            with L.debug_menu({L.KEY_DETERMINISTIC: det}):
                model, eng = _make(monkeypatch, variant, -1, layout)
                _fwd_bwd(eng, b)
                runs.append(model._engine.grad_bf16.clone())
                names = [n for n, p in model._engine.params.items() if not (len(p["shape"]) == 2 and 0 <= p["layer"] < NL)]
                small = _mask(model._engine, names)
        D = float((runs[0].double() - runs[1].double()).abs()[small].max())
        _REF[key] = (runs[0], D)
    return _REF[key]


# ------------------------------------------------------------------------------------------------ 1 + 2. gradients, truncation
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("variant,shape,layout", [("plain", "b8s32", "auto"), ("plain", "b8s32", "padded"), ("plain", "b4s72", "auto"),
                                                  ("plain", "b4s72", "padded"), ("ls", "b8s32", "auto"), ("ls", "b4s72", "padded"),
                                                  ("gated", "b8s32", "auto"), ("gated", "b4s72", "padded")])
def test_trainable_gradients_equal_the_unfrozen_run_and_frozen_ones_are_not_written(monkeypatch, variant, shape, layout, k):
    ref, D = _reference(monkeypatch, variant, shape, layout)
    model, eng = _make(monkeypatch, variant, k, layout)
    frozen_names = set(model.frozen_names())

    def fill(e):
        e.grad_bf16[~_train_mask(e)] = SENTINEL

    _fwd_bwd(eng, _batch(shape), before_backward=fill)
    e = model._engine
    assert e.frozen == k and len(e.train_ranges) == (2 if variant == "gated" else 1)
    got = e.grad_bf16
    worst = 0.0
    for name, p in e.params.items():
        sl = slice(p["offset"], p["offset"] + p["numel"])
        if name in frozen_names:
            assert e.is_frozen(name)
            if variant != "gated":
                assert bool((got[sl] == SENTINEL).all()), f"{name}: the frozen gradient range was written (the backward was not truncated)"
            continue
        assert not e.is_frozen(name)
        if len(p["shape"]) == 2 and 0 <= p["layer"] < NL:
            assert torch.equal(got[sl].view(torch.int16), ref[sl].view(torch.int16)), f"{name}: a GEMM-written gradient differs"
            continue
        err = (got[sl].double() - ref[sl].double()).abs()
        bound = 4.0 * D + _ulp_bf16(ref[sl])
        worst = max(worst, float((err - bound).max()))
        assert bool((err <= bound).all()), f"{name}: max |diff| {float(err.max()):.3g}, D = {D:.3g}"
    if variant != "gated":      # gaps belong to no parameter: whatever is outside the trainable ranges kept the sentinel
        assert bool((got[~_train_mask(e)] == SENTINEL).all())
    print(f"[freeze] {variant} {shape} {layout} k={k}: D = {D:.3g}, largest (|diff| - bound) = {worst:.3g}", flush=True)
    record_error(f"freeze_grads_{variant}_{shape}_{layout}_k{k}", "small_param_diff_minus_bound", worst, 0.0)
    record_error(f"freeze_grads_{variant}_{shape}_{layout}", "det_vs_atomic_max_diff_D", D, D)


# ------------------------------------------------------------------------------------------------ 3. the step, every launch form
FORMS = {
    "replicated": dict(),
    "ema_fused": dict(use_ema=True),
    "accum_k2": dict(gradient_accumulation_steps=2),
    "norm_from_backward": dict(fold=True),
    "loopback2": dict(world=2),
    "loopback2_zero2": dict(world=2, zero=2),
}
STEP_CASES = [("plain", 1, f) for f in FORMS] + [("plain", 0, "replicated"), ("plain", 3, "replicated"), ("plain", 5, "replicated"),
                                                 ("ls", 2, "replicated"), ("ls", 2, "loopback2_zero2"), ("gated", 1, "replicated"),
                                                 ("gated", 1, "loopback2_zero2"), ("gated", 1, "ema_fused")]


def _arenas(e):
    e.await_params()
    torch.cuda.synchronize()
    d = dict(w=e.master.clone(), m=e.adam_m.clone(), v=e.adam_v.clone(), P=e.param_bf16.clone())
    if e.ema is not None:
        d["ema"] = e.ema.clone()
    return d


@pytest.mark.parametrize("variant,k,form", STEP_CASES)
def test_step_touches_the_trainable_ranges_only(monkeypatch, variant, k, form):
    kw = dict(FORMS[form])
    world, zero, fold = kw.pop("world", 0), kw.pop("zero", 0), kw.pop("fold", False)
    acc = kw.get("gradient_accumulation_steps", 1)
    model, eng = _make(monkeypatch, variant, k, world=world, zero=zero, fold=fold, **kw)
    try:
        batches = [_batch("b8s32", seed=5 + i) for i in range(3 * acc)]
        e = model._ensure_engine(8, 32)
        if kw.get("use_ema"):           # the average exists before the first snapshot: ModelEmaV3.__init__ copies the model (d = 0)
            e.ema_attach()
            e.ema_update(0.0)
            torch.cuda.synchronize()
            assert torch.equal(e.ema, e.master)
        tm = _train_mask(e)
        emb = e.params["model.embed_tokens.weight"]["offset"]
        gs = 1.0 / (max(1, world) * acc)
        gsum, pre = None, None
        for i in range(acc):
            if i == acc - 1:
                pre = _arenas(e)
            _fwd_bwd(eng, batches[i])
            e.grad_bf16[emb + 5] = float("inf")      # a frozen element: neither the norm nor the update may read it
            g = e.grad_bf16[tm].double()
            gsum = g if gsum is None else gsum + g
            if i < acc - 1:
                assert eng.step() is None
        # the clip is active: half the float64 norm of the trainable gradients
        want = R.norm64(gsum, gs)
        eng.optim.max_grad_norm = 0.5 * want
        gn = eng.step()
        nrm = float(gn)
        assert np.isfinite(nrm), "the norm read a frozen gradient element"
        post = _arenas(e)
        h = R.Hyper(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.1, max_norm=0.5 * want, gs=gs)
        c = R.coef64(h, nrm)
        assert c < h.gs * 0.75, "the clip is not active"
        out = R.verify_step(dict(w=pre["w"][tm], m=pre["m"][tm], v=pre["v"][tm], g=gsum), {q: post[q][tm] for q in "wmvP"}, h, 1, c)
        n_train = int(tm.sum())
        chain = (R.chain_shard(e.trainable_buckets()) if zero else R.chain_chunks(n_train, 0)) + (2 if acc > 1 else 0)
        r, ref = R.norm_ratio(nrm, gsum, h.gs, chain)
        out["norm"] = (r, int(not r <= 1.0))
        # ... and the check can tell the two norms apart: all gradients of the never-frozen run against the trainable ones
        full, _ = _reference(monkeypatch, variant, "b8s32", "auto")
        if acc == 1:
            n_all, n_tr = R.norm64(full.double(), 1.0), R.norm64(full[tm].double(), 1.0)
            assert abs(n_all - n_tr) > (chain + 4) * R.U * n_tr, "the frozen gradients do not separate the two norms"
        print(f"[freeze] step {variant} k={k} {form}: norm {nrm:.6g} (float64 {ref:.6g}), max |err| / bound = "
              + ", ".join(f"{q} {x:.4f}" for q, (x, _) in sorted(out.items())), flush=True)
        for q, (x, _) in out.items():
            record_error(f"freeze_step_{variant}_k{k}_{form}", f"{q}_err_over_bound", x, 1.0)
        bad = {q: (n, round(x, 3)) for q, (x, n) in out.items() if n}
        assert not bad, f"elements outside the bound (count, largest ratio) {bad}"
        for s in range(1, 3):           # two more updates: three in all
            for i in range(acc):
                _fwd_bwd(eng, batches[s * acc + i])
                e.grad_bf16[emb + 5] = float("inf")
                assert np.isfinite(float(eng.step() if i == acc - 1 else (eng.step() or 0.0)))
        if zero:
            eng.consolidate()
        last = _arenas(e)
        assert e is model._engine and eng.global_steps == 3
        for q in last:
            assert torch.equal(last[q][~tm].view(torch.int32 if last[q].dtype == torch.float32 else torch.int16),
                               pre[q][~tm].view(torch.int32 if pre[q].dtype == torch.float32 else torch.int16)), f"frozen range of {q} changed"
            if q != "ema":
                assert not torch.equal(last[q][tm], pre[q][tm])
        if "ema" in last:
            assert torch.equal(last["ema"][~tm], last["w"][~tm]) and not torch.equal(last["ema"][tm], pre["ema"][tm])
    finally:
        _finish(model)


def test_set_frozen_is_refused_inside_an_accumulation_window(monkeypatch):
    model, eng = _make(monkeypatch, "plain", -1, gradient_accumulation_steps=2)
    _fwd_bwd(eng, _batch("b8s32"))
    assert eng.step() is None and model._engine.grad_acc_count() == 1
    with pytest.raises(L.GgetError, match="accumulation window"):
        model._engine.set_frozen(1)
    assert model._engine.frozen == -1 and model._engine.train_ranges == [(0, model._engine.n_params)]


# ------------------------------------------------------------------------------------------------ 4. surface
def _ft_cfg(tmp_path, freeze):
    from test_pipeline_config import _tiny_reference_cfg
    cfg, _ = _tiny_reference_cfg(tmp_path, "ft")
    cfg.training.deepspeed_conf_file = ""
    cfg.training.schedule.epochs, cfg.training.schedule.warmup_epochs = 2, 0.5
    cfg.training.finetune.freeze = freeze
    return cfg


def test_pipeline_honours_finetune_freeze(tmp_path):
    """TrainingPipeline with finetune.freeze = 1 leaves embed_tokens and layer 0 bit-unchanged over its steps (a build that ignores the
    field updates them), and config.num_params is the trainable count."""
    batches = [{k: torch.from_numpy(v) for k, v in synth.make_task_batch(B=8, S=32, F=4, V=41245, seed=70 + i).items()} for i in range(6)]
    mode = T.FinetuneMode(batches=batches, samples_per_gpu=16, vocab_size=41245, bos_token_id=1, eos_token_id=2)
    p = T.TrainingPipeline(_ft_cfg(tmp_path, 1), mode).run()
    assert p.engine.global_steps == 4 and np.isfinite(float(p.last_loss))
    frozen = set(p.model.frozen_names())
    assert p.model.config.num_params == sum(q.numel() for n, q in p.model.named_parameters() if n not in frozen)
    fresh = M.GraphGPTTaskModel(copy.deepcopy(p.config))    # same seed -> the initial weights (a model writes num_params into its config)
    assert "model.embed_tokens.weight" in frozen and any(n.startswith("model.layers.0.") for n in frozen)
    assert not any(n.startswith("model.layers.1.") or n.startswith("score") or n == "model.norm.weight" for n in frozen)
    now = p.model.state_dict()
    for name, w0 in fresh.state_dict().items():
        same = torch.equal(now[name].cpu(), w0)
        assert same == (name in frozen), f"{name}: {'changed though frozen' if name in frozen else 'not trained'}"
    assert p.model.config.num_params == sum(q.numel() for n, q in p.model.named_parameters() if n not in frozen)
    for name, q in p.model.named_parameters():
        assert q.requires_grad == (name not in frozen)
        if name in frozen:
            assert q.grad is None


def test_grad_attribute_engine_recreation_checkpoint_and_ema(monkeypatch, tmp_path):
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):
        # (a) autograd-style use: .grad of a frozen parameter stays None, the others are filled
        for name in _DP_ENV:
            monkeypatch.delenv(name, raising=False)
        model = M.GraphGPTTaskModel(M.GraphGPTConfig(**CFG), seed=7).cuda().eval()
        model.freeze_layers(1)
        b = _batch("b8s32")
        model(input_ids=b["input_ids"], attention_mask=b["attention_mask"], task_labels=b["task_labels"]).task_loss.backward()
        frozen = set(model.frozen_names())
        for name, q in model.named_parameters():
            assert (q.grad is None) == (name in frozen) and q.requires_grad == (name not in frozen)
        # (b) uninterrupted: 2 steps, save, a larger batch (the engine is re-created and stays frozen), 1 more step
        model, eng = _make(monkeypatch, "plain", 1, use_ema=True)
        small = [_batch("b8s32", seed=20 + i) for i in range(2)]
        big = {k: torch.from_numpy(v) for k, v in synth.make_task_batch(B=16, S=40, F=4, V=300, seed=30).items() if k != "lengths"}
        for bb in small:
            _fwd_bwd(eng, bb)
            eng.step()
        first = model._engine
        eng.save_checkpoint(str(tmp_path / "ck"))
        _fwd_bwd(eng, big)
        eng.step()
        e = model._engine
        assert e is not first and e.frozen == 1 and e.train_ranges == first.train_ranges
        want = _arenas(e)
        tm = _train_mask(e)
        init = M.GraphGPTTaskModel(M.GraphGPTConfig(**CFG), seed=7).state_dict()
        for name in model.frozen_names():
            assert torch.equal(e.view(name, "master").cpu(), init[name])
        # inside ema_weights the frozen weights equal the live ones
        live = e.param_bf16.clone()
        with eng.ema_weights():
            torch.cuda.synchronize()
            assert torch.equal(model._engine.param_bf16[~tm], live[~tm]) and not torch.equal(model._engine.param_bf16[tm], live[tm])
        # (c) load into a fresh frozen engine and continue: the same bits
        model2, eng2 = _make(monkeypatch, "plain", 1, use_ema=True)
        eng2.load_checkpoint(str(tmp_path / "ck"))
        _fwd_bwd(eng2, big)
        eng2.step()
        got = _arenas(model2._engine)
        for q in want:
            assert torch.equal(got[q], want[q]), f"{q}: the resumed run differs from the uninterrupted one"
        # (d) the checkpoint keeps its format both ways: written frozen, it loads into a run that does not freeze
        model3, eng3 = _make(monkeypatch, "plain", -1, use_ema=True)
        eng3.load_checkpoint(str(tmp_path / "ck"))
        _fwd_bwd(eng3, big)
        assert np.isfinite(float(eng3.step()))
        eng3.save_checkpoint(str(tmp_path / "ck3"))
        eng2.load_checkpoint(str(tmp_path / "ck3"))
        _fwd_bwd(eng2, big)
        assert np.isfinite(float(eng2.step()))


# ------------------------------------------------------------------------------------------------ 5. the default is unchanged
def test_freeze_minus_one_is_the_unfrozen_model(monkeypatch):
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):
        res = []
        for call in (False, True):
            model, eng = _make(monkeypatch, "ls", -1)
            if call:
                model.freeze_layers(-1)
                model._engine.set_frozen(-1)
            losses = []
            for i in range(3):
                losses.append(float(_fwd_bwd(eng, _batch("b8s32", seed=40 + i))))
                eng.step()
            res.append((losses, _arenas(model._engine)))
        assert res[0][0] == res[1][0]
        for q in res[0][1]:
            assert torch.equal(res[0][1][q], res[1][1][q])
