"""The clip + AdamW step on the device, every element of every arena against a float64 restatement, in every launch form: the
replicated kernel (adamw_kernel<2>), its fused-EMA instantiation, the sharded work-item kernel (adamw_items_kernel) on a world-1
plan and on loopback worlds of 2 and 4, the three gradient-norm paths, and the skip rule.  State and gradients are written through
Engine.view per parameter (gaps and pad rows stay zero and are checked to stay zero); every step is compared from the device's OWN
state before it, so chained steps test each step and accumulate no reference drift.

The restatement, the per-element bounds and their derivation: tests/_adamw_ref.py (validated on the CPU by tests/test_adamw_bound.py,
where an fp32 restatement of the kernel uses at most a third of each bound and seven wrong formulas leave them).  In short, u = 2^-24:
    |dm'| <= 6u (|b1 m| + |(1 - b1) ge|)      |dv'| <= 11u v'      |dw'| <= 8u |w| + (24u + d1 + d2) U      P' == RNE-bf16(master') bitwise
with d1 = d_bc(b1, t), d2 = d_bc(b2, t) / 2 + u, d_bc(b, t) = u (1 + 2 b^t / (1 - b^t)) - the real precision of an fp32 bias
correction: d2 = 500.8 u at (b2, t) = (0.999, 2), where the host's sqrtf(1.0f - powf(b2, 2)) was observed 55.6 u off the float64
value in one run (d1 = 9.5 u at (0.9, 2), observed 1.26 u; tests/test_adamw_bound.py prints the current figures).  The coefficient is rebuilt in float64 from the norm the device reported,
c = gs min(1, max_norm / (nrm + float32(1e-6))), so the norm's summation error stays out of the element check.

The norm is checked on its own: |nrm - sqrt(sum g^2) gs| <= (L + 4) u nrm64 with the sum in float64 over the gradient arena as the
step met it.  L = the longest chain of fp32 additions a term passes through (squares are non-negative: L additions bound the sum by
L u and the root by half; 4 = the multiply, the root, the grad_scale multiply):
  full pass (k_grad_sqnorm)              8 ceil(nv / (blocks 256)) serial in a thread (nv = n / 8 vectors, blocks = min(1024,
                                         ceil(nv / 256))) + 6 (wave_sum) + 4 (waves) + ceil(blocks / 256) + 8 (tree of 256)
  chunks + tile partials                 max(8 ceil(chunk / 2048) + 6 + 4, 72 + 6 + 8) + ceil(1024 / 256) + layers + 8, chunk <=
                                         max(32768, ceil(n / 900)): a table chunk, or a 192 x 192 weight-gradient tile over 512
                                         threads; the tile sums square the value after its bf16 rounding (gemm.hip sq_add), i.e.
                                         the stored gradient - no extra term.  The handle falls back to the full pass when a layer
                                         left no partials and does not say so: the bound uses the larger L of the two paths.
  shard partials + slots                 16 + 6 + 4 per 4096-element chunk, ceil(chunks / 1024) per thread of the one block + 10

The replicated launch (grid min(65536, ceil(n / 2048)) blocks, two float4 groups per thread) runs its outer loop once below 1.3e8
elements: the tiny and the 2-layer d = 768 model exercise the second group and its `i >= nv` break (n / 8 is no multiple of 256
there), the 24-layer d = 1024 model (3.2e8 elements, capped grid) the repeated loop and its break in the last pass.

Not run here: a real multi-rank RCCL exchange (a loopback world does every rank's share on one device)."""
import importlib
import json
import os

import pytest
import torch

import _adamw_ref as R
from _util import spec_mod

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
_RATIOS = {}
_ENGINES = {}
EMA_EPS = 8.0 * R.U


def _spec(model):
    if model == "d768":
        return spec_mod.ModelSpec(kind=spec_mod.KIND_PRETRAIN, vocab_size=756, hidden_size=768, intermediate_size=3072, num_layers=2,
                                  num_heads=12, head_dim=64, stacked_feat=13, next_n_token=13, causal=False, max_position=1024)
    return spec_mod.spec_from_size(model, vocab_size=756, stacked_feat=13, next_n_token=13)


def _new_engine(model):
    e = importlib.import_module("graph-gpt_amd.engine").Engine(_spec(model), max_tokens=256, max_batch=8)
    e.covered = torch.zeros(e.n_params, dtype=torch.bool, device="cuda")
    for p in e.params.values():
        e.covered[p["offset"]: p["offset"] + p["numel"]] = True
    assert int((~e.covered).sum()) > 0, "the model must have gaps"
    return e


def _engine(model):
    """one raw engine per model for the replicated cases (every case writes the whole state before its first step)"""
    if model not in _ENGINES:
        _ENGINES[model] = _new_engine(model)
    return _ENGINES[model]


def _inject(e, **arenas):
    """flat [n_params] tensors into the arenas, parameter by parameter (the gaps are never written)"""
    for which, flat in arenas.items():
        for k, p in e.params.items():
            e.view(k, which).copy_(flat[p["offset"]: p["offset"] + p["numel"]].view(p["shape"]))


def _pre(e):
    torch.cuda.synchronize()
    return dict(w=e.master.clone(), m=e.adam_m.clone(), v=e.adam_v.clone(), g=e.grad_bf16.clone())


def _post(e):
    e.await_params()
    torch.cuda.synchronize()
    return dict(w=e.master, m=e.adam_m, v=e.adam_v, P=e.param_bf16)


def _record(what, out):
    _RATIOS[what] = {k: round(r, 6) for k, (r, _) in out.items()}
    print(f"[adamw] {what}: max |err| / bound = " + ", ".join(f"{k} {r:.4f}" for k, (r, _) in sorted(out.items())), flush=True)
    bad = {k: (n, round(r, 3)) for k, (r, n) in out.items() if n}
    assert not bad, f"{what}: elements outside the bound (count, largest ratio) {bad}"


def _gaps_zero(e, what):
    gap = ~e.covered
    for name, arena in (("master", e.master), ("m", e.adam_m), ("v", e.adam_v), ("P", e.param_bf16), ("grad", e.grad_bf16), ("ema", e.ema)):
        if arena is not None:
            assert not bool(arena[gap].any()), f"{what}: a gap or pad-row element of {name} is not zero"


def _verify(e, pre, gn, h, chain, what):
    """the element check of every arena, the norm check and the gaps of the step that just ran (t = e.step_count)"""
    post = _post(e)
    nrm = float(gn)
    out = R.verify_step(pre, post, h, e.step_count, R.coef64(h, nrm))
    r, _ = R.norm_ratio(nrm, pre["g"], h.gs, chain)
    out["norm"] = (r, int(not r <= 1.0))
    _record(what, out)
    _gaps_zero(e, what)
    return post


def _step(e, h, sharded=False):
    kw = dict(beta1=h.b1, beta2=h.b2, eps=h.eps, weight_decay=h.wd, max_grad_norm=h.max_norm, grad_scale=h.gs)
    if sharded:
        e.shard_sqnorm_partials()
        return e.adamw_step_sharded(h.lr, **kw)
    return e.adamw_step(h.lr, **kw)


def _case(e, h0, clip, what, seed, steps=((None, 3), (6, 1), (99, 1), (999, 1)), sharded=False, world=1, chain=None):
    """`steps`: (step_count preset or None = go on, number of chained steps).  The whole state is written before the first step of
    every group, fresh gradients before every step."""
    small = clip == "small"
    chain = chain or R.chain_full(e.n_params)
    e.step_count = 0
    for preset, count in steps:
        if preset is not None:
            e.step_count = preset
        for i in range(count):
            w, m, v, g, h = R.make_inputs(e.n_params, seed + 31 * e.step_count, h0, device="cuda", covered=e.covered, small=small,
                                          world=world, clip=clip)
            _inject(e, grad=g, **(dict(master=w, m=m, v=v) if i == 0 else {}))
            if world > 1:
                for b in range(len(e.buckets)):
                    e.reduce_scatter_grads_async(b)        # (the loopback exchange: the arena times `world`)
            pre = _pre(e)
            if world > 1:
                assert torch.equal(pre["g"].float(), g.float() * world)
            gn = _step(e, h, sharded)
            _verify(e, pre, gn, h, chain, f"{what}_t{e.step_count}")


@pytest.fixture(scope="module", autouse=True)
def _write_ratios():
    yield
    _ENGINES.clear()
    path = os.environ.get("GGET_ADAMW_PARITY_OUT")          # profiles/adamw_parity.json is a whole run of this file written there on request
    if _RATIOS and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        worst = {}
        for r in _RATIOS.values():
            for k, x in r.items():
                worst[k] = max(worst.get(k, 0.0), x)
        with open(path, "w") as fh:
            json.dump({"what": "largest |device - float64 restatement| / bound per check of tests/test_gpu_adamw_exact.py (bounds: "
                               "tests/_adamw_ref.py), every element of every arena checked; P = 1 if any bf16 bit differs from "
                               "RNE(master'); ratios are findings, not thresholds", "largest": worst, "ratios": _RATIOS}, fh, indent=1)


# ------------------------------------------------------------------------------------------------ the replicated launch
@pytest.mark.parametrize("gs", [1.0, 0.25])
@pytest.mark.parametrize("clip", ["off", "negative", "inactive", "active", "small"])
@pytest.mark.parametrize("model", ["tiny", "d768"])
def test_replicated_step(model, clip, gs):
    """k_adamw: clip off (max_norm 0 and negative), inactive, active, active at a norm of 1e-4 (where the 1e-6 of the denominator is
    1 % of it); grad_scale 1 and 0.25; steps 1, 2, 3 chained, then one step each from step_count 6, 99 and 999."""
    _case(_engine(model), R.Hyper(gs=gs), clip, f"replicated_{model}_{clip}_gs{gs}", seed=100)


@pytest.mark.parametrize("model", ["tiny", "d768"])
def test_replicated_step_beta2_999(model):
    """(0.9, 0.999): the bias correction of v at its least precise (d2 = 1000.5 u at t = 1, 500.8 u at t = 2)"""
    _case(_engine(model), R.Hyper(b2=0.999, gs=0.25), "active", f"replicated_{model}_b2_0.999", seed=200)


def test_replicated_step_capped_grid():
    """24 layers of d = 1024 (3.2e8 elements): the grid is capped at 65536 blocks, the grid-stride loop runs three times and ends inside
    its unrolled pair."""
    e = _new_engine("large")
    assert e.n_params // 8 > 65536 * 256 and (e.n_params // 4) % (2 * 65536 * 256) != 0
    _case(e, R.Hyper(), "active", "replicated_large", seed=300, steps=((None, 1),))


@pytest.mark.parametrize("model", ["tiny", "d768"])
def test_fused_ema_step(model):
    """adamw_kernel<2, .., EMA>: the same element check on master, m, v and P, and the EMA within 8u max(|ema|, |w'|) of
    w' + d32 (ema - w') against the NEW master weights read back"""
    e = _engine(model)
    e.ema_attach()
    for d in (0.5, 0.9999):
        w, m, v, g, h = R.make_inputs(e.n_params, 400, R.Hyper(), device="cuda", covered=e.covered, clip="active")
        ema0 = torch.where(e.covered, 0.05 * torch.randn(e.n_params, device="cuda", generator=torch.Generator("cuda").manual_seed(9)),
                           torch.zeros((), device="cuda"))
        _inject(e, master=w, m=m, v=v, grad=g, ema=ema0)
        e.step_count = 1
        pre = _pre(e)
        e.set_ema_decay(d)
        gn = _step(e, h)
        post = _verify(e, pre, gn, h, R.chain_full(e.n_params), f"fused_ema_{model}_d{d}")
        w64, e64 = post["w"].double(), ema0.double()
        err = (e.ema.double() - (w64 + R.f32(d) * (e64 - w64))).abs()
        bound = EMA_EPS * torch.maximum(w64.abs(), e64.abs())
        r, bad = R._ratio(err, bound)
        _record(f"fused_ema_{model}_d{d}_ema", {"ema": (r, bad)})
        assert not torch.equal(e.ema, ema0)
    e.ema_detach()


# ------------------------------------------------------------------------------------------------ the sharded launch
@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("model", ["tiny", "d768"])
def test_sharded_step(model, world):
    """k_adamw_items over the work items of a shard plan, the norm through per-chunk partials and the slot sum: a world-1 plan, and
    loopback worlds of 2 and 4 (the exchange multiplies the gradients by world, AdamW takes grad_scale = 1 / world; the loopback
    handle does every rank's share, so the whole arena is checked)."""
    e = _new_engine(model)
    if world > 1:
        e.comm_init_loopback(world)
    e.shard_init(world, 0)
    try:
        for clip in ("off", "active", "small"):
            _case(e, R.Hyper(gs=1.0 / world), clip, f"sharded_{model}_world{world}_{clip}", seed=500, steps=((None, 2), (99, 1)),
                  sharded=True, world=world, chain=R.chain_shard(e.buckets))
    finally:
        if e.comm_world:
            e.comm_destroy()


# ------------------------------------------------------------------------------------------------ the norm of a real backward
@pytest.mark.parametrize("fold", [True, False])
def test_norm_of_a_real_backward(monkeypatch, fold):
    """A backward of the 2-layer d = 768 model with GGET_NORM_FROM_BACKWARD on (chunks + the weight-gradient tiles' partials) and off
    (full pass): the reported norm against the float64 norm of the gradient arena under that path's L."""
    M = importlib.import_module("graph-gpt_amd.modeling")
    tr = importlib.import_module("graph-gpt_amd.training")
    synth = importlib.import_module("graph-gpt_amd.synth")
    if fold:
        monkeypatch.setenv("GGET_NORM_FROM_BACKWARD", "1")
    else:
        monkeypatch.delenv("GGET_NORM_FROM_BACKWARD", raising=False)
    cfg = M.GraphGPTConfig(hidden_act="gelu", vocab_size=756, hidden_size=768, intermediate_size=3072, num_hidden_layers=2,
                           num_attention_heads=12, max_position_embeddings=1024, causal_attention=False, stacked_feat=13, next_n_token=13)
    batch = synth.make_pretrain_batch(B=64, S=32, F=13, V=756, seed=21)
    dev = {k: torch.from_numpy(v).cuda() for k, v in batch.items() if k != "lengths"}
    model = M.GraphGPTPretrainBase(cfg, seed=4).cuda()
    eng = tr.initialize(model, tr.OptimConfig(lr=1e-3, max_grad_norm=0.05))
    for s in range(2):
        out = eng(input_ids=dev["input_ids"], attention_mask=dev["attention_mask"], labels=dev["labels"])
        eng.backward(out.head1_loss)
        e = model._engine
        torch.cuda.synchronize()
        g = e.grad_bf16.clone()
        gn = float(eng.step())
        torch.cuda.synchronize()
        assert torch.equal(e.grad_bf16, g)
        chain = R.chain_full(e.n_params)
        if fold:
            chain = max(chain, R.chain_chunks(e.n_params, 2))
        r, ref = R.norm_ratio(gn, g, 1.0, chain)
        assert ref > 0.05, "the clip must be active"
        _record(f"norm_backward_{'tiles' if fold else 'full'}_step{s + 1}", {"norm": (r, int(not r <= 1.0))})


# ------------------------------------------------------------------------------------------------ the skip rule
@pytest.mark.parametrize("model", ["tiny", "d768"])
def test_skip_rule_leaves_the_state_alone(model):
    """GGET_OPT_SKIP_NONFINITE_STEP: one inf, then one NaN gradient - master, m, v and P unchanged bit for bit, the reported norm
    non-finite; the finite step that follows satisfies the bounds."""
    e = _engine(model)
    e.set_option(L.OPT_SKIP_NONFINITE_STEP, 1)
    try:
        w, m, v, g, h = R.make_inputs(e.n_params, 600, R.Hyper(), device="cuda", covered=e.covered, clip="active")
        _inject(e, master=w, m=m, v=v, grad=g)
        e.step_count = 0
        _verify(e, _pre(e), _step(e, h), h, R.chain_full(e.n_params), f"skip_{model}_before")        # (P now holds RNE(master))
        at = int(torch.nonzero(e.covered)[12345])
        for bad in (float("inf"), float("nan")):
            _inject(e, grad=g)
            e.grad_bf16[at] = bad
            torch.cuda.synchronize()
            before = {k: x.clone() for k, x in _post(e).items()}
            gn = _step(e, h)
            e.step_count -= 1                                  # (the step did not run: GgetEngine.step does the same)
            after = _post(e)
            assert not bool(torch.isfinite(gn))
            for k in before:
                assert torch.equal(before[k].view(torch.int32 if k != "P" else torch.int16),
                                   after[k].view(torch.int32 if k != "P" else torch.int16)), f"{k} moved in a skipped step ({bad})"
        _inject(e, grad=g)
        pre = _pre(e)
        _verify(e, pre, _step(e, h), h, R.chain_full(e.n_params), f"skip_{model}_after")
        assert e.step_count == 2
    finally:
        e.set_option(L.OPT_SKIP_NONFINITE_STEP, 0)
