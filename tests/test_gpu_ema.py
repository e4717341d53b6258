"""The weight EMA (`optimizer.use_ema`) on the device, through the C ABI and the Python surface: nothing moves when it is attached, the
fused lerp equals the stand-alone one bit for bit, both equal a float64 restatement within the rounding bound of the formula, seeding,
gaps, the skipped step, gradient accumulation, evaluation on the averaged weights, checkpoints, the sharded step and the pipeline.
Comparisons across runs use the reproducible mode (GGET_DETERMINISTIC=1).

The float64 restatement (issue: the formula is fixed, `ema' = w + d * (ema - w)` in fp32 with d the fp32 decay as it crossed the ABI):
one update from identical fp32 inputs is at most three fp32 roundings (the difference, the product, the sum; two with a fused
multiply-add), each at most 2^-24 of a quantity no larger than 2 max(|ema|, |w|), so per element
    |got - (w + d32 (ema - w))| <= 8 * 2^-24 * max(|ema|, |w|),         d32 = float64(float32(d)),
and n chained updates stay within n times that (the errors are contracted by d < 1: the linear sum is an upper bound)."""
import importlib
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _util import ROOT

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
EPS = 8.0 * 2.0 ** -24
_RATIOS = {}


def _mods():
    return (importlib.import_module("graph-gpt_amd.modeling"), importlib.import_module("graph-gpt_amd.training"),
            importlib.import_module("graph-gpt_amd.synth"))


def _cfg(modeling, **kw):
    base = dict(hidden_act="gelu", vocab_size=756, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                max_position_embeddings=1024, causal_attention=False, stacked_feat=13, next_n_token=13, attention_dropout=0.0)
    base.update(kw)
    return modeling.GraphGPTConfig(**base)


def _ft_cfg(modeling):
    return _cfg(modeling, vocab_size=1000, stacked_feat=4, next_n_token=1, num_labels=2)


def _batch(synth, seed):
    b = synth.make_pretrain_batch(B=8, S=32, F=13, V=756, seed=700 + seed)
    return {k: torch.from_numpy(v).cuda() for k, v in b.items() if k != "lengths"}


def _ft_batch(synth, seed, B=8, S=24):
    b = synth.make_task_batch(B=B, S=S, F=4, V=1000, seed=300 + seed)
    return {k: torch.from_numpy(v).cuda() for k, v in b.items() if k != "lengths"}


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy().copy()


def _state(e):
    torch.cuda.synchronize()
    return {k: _bits(getattr(e, a)) for k, a in (("master", "master"), ("m", "adam_m"), ("v", "adam_v"), ("P", "param_bf16"))}


def _lerp64(w, ema, d):
    """the float64 restatement and its per-element bound; `d` is rounded to fp32 first - the value the kernel was given"""
    d32 = float(np.float32(d))
    w64, e64 = w.double(), ema.double()
    return w64 + d32 * (e64 - w64), EPS * torch.maximum(w64.abs(), e64.abs())


def _check(got, ref, bound, what):
    """every element: |got - ref| <= bound; returns (and records) the largest ratio to the bound"""
    err = (got.double() - ref).abs()
    ok = err <= bound
    ratio = float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
    _RATIOS[what] = max(_RATIOS.get(what, 0.0), ratio)
    print(f"[ema] {what}: max |err| / bound = {ratio:.4f}", flush=True)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} elements outside the bound, largest ratio {ratio:.3f}"
    return ratio


@pytest.fixture
def reproducible():
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):
        yield


@pytest.fixture(scope="module", autouse=True)
def _write_ratios():
    yield
    if _RATIOS:
        path = os.environ.get("GGET_EMA_PARITY_OUT")       # profiles/ema_parity.json is a whole run of this file written there on request
        if not path:
            return
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"what": "largest |kernel - float64 restatement| / bound per check of tests/test_gpu_ema.py; bound = n * 8 * 2^-24 * "
                               "max(|ema|, |w|) per element for n chained updates, every element checked", "ratios": _RATIOS}, fh, indent=1)


# ------------------------------------------------------------------------------------------------ items 1, 2, 5, 10: training runs
def _env(monkeypatch, world, zero):
    backend = "abi" if zero else "torch"        # (world 0, zero 0: the plain single-GPU step; world 0, zero 2: the one-rank RCCL communicator)
    monkeypatch.setenv("GGET_DP_BACKEND", backend)
    monkeypatch.setenv("GGET_DP_LOOPBACK_WORLD", str(world) if backend == "abi" and world else "0")
    monkeypatch.setenv("GGET_FORCE_STAGED", "1" if zero else "0")
    monkeypatch.setenv("GGET_ZERO_STAGE", str(zero))
    monkeypatch.setenv("GGET_DP_FP32_REDUCE", "0")


def _train(monkeypatch, mode, world=0, zero=0, steps=5, decay=0.9, before_consolidate=None):
    """`steps` training steps of the tiny pre-train model.  mode: "off" (no EMA), "fused" (OptimConfig(use_ema=True): the lerp inside the
    AdamW launch), "standalone" (plain steps, each followed by gget_ema_update with the decay the fused run used).  Returns per step
    (loss bits, norm bits, state bits, ema bits or None) and the final ema after consolidate()."""
    modeling, tr, synth = _mods()
    _env(monkeypatch, world, zero)
    model = modeling.GraphGPTPretrainBase(_cfg(modeling), seed=1)
    eng = tr.initialize(model, tr.OptimConfig(lr=1e-3, max_grad_norm=0.05, use_ema=(mode == "fused"), ema_decay=decay))
    assert eng.sharded == (zero > 0)
    rows = []
    for s in range(steps):
        loss = tr.batch_training(_batch(synth, s % 2), eng)
        e = model._engine
        if mode == "standalone":
            e.ema_attach()
            if s == 0:
                e.ema_update(0.0)       # (the seed; the first two updates copy anyway)
            e.ema_update(eng.ema_decay_at(s))
        e.await_params()
        torch.cuda.synchronize()
        rows.append((_bits(loss.detach().float().reshape(1)), _bits(eng.last_grad_norm.reshape(1)), _state(e),
                     None if mode == "off" else _bits(e.ema)))
    e = model._engine
    if before_consolidate is not None:
        before_consolidate(eng, e)
    eng.consolidate()
    final = None if mode == "off" else _bits(e.ema)
    if mode == "off":
        assert e.ema is None
    if e.comm_world:
        e.comm_destroy()
    return rows, final, e


@pytest.mark.parametrize("world,zero", [(0, 0), (2, 2), (4, 2)])
def test_attached_ema_moves_nothing_and_fused_equals_standalone(monkeypatch, reproducible, world, zero):
    """Items 1 and 2: loss, gradient norm, master, m, v and the bf16 copy bit-identical at every step with and without the EMA - replicated
    step and loopback worlds 2 / 4 of the sharded step; the fused arena equals the plain step + gget_ema_update arena bit for bit."""
    off, _, _ = _train(monkeypatch, "off", world, zero)
    fused, _, _ = _train(monkeypatch, "fused", world, zero)
    alone, _, _ = _train(monkeypatch, "standalone", world, zero)
    for s, (a, b, c) in enumerate(zip(off, fused, alone)):
        np.testing.assert_array_equal(a[0], b[0], err_msg=f"loss step {s}")
        np.testing.assert_array_equal(a[1], b[1], err_msg=f"norm step {s}")
        for k in a[2]:
            np.testing.assert_array_equal(a[2][k], b[2][k], err_msg=f"{k} step {s}")
        np.testing.assert_array_equal(b[3], c[3], err_msg=f"fused vs stand-alone arena, step {s}")
    assert not np.array_equal(fused[-1][3], fused[-1][2]["master"]), "after five steps the average must differ from the weights"


def test_gaps_and_pad_rows_stay_zero(monkeypatch, reproducible):
    """Item 5: after 5 steps every element of the arena that belongs to no parameter (gaps, lm_head pad rows) is zero."""
    _, final, e = _train(monkeypatch, "fused")
    covered = np.zeros(e.n_params, dtype=bool)
    for p in e.params.values():
        covered[p["offset"]: p["offset"] + p["numel"]] = True
    assert (~covered).sum() > 0, "the test model must have gaps"
    assert not final[~covered].any()
    assert final[covered].any()


@pytest.mark.parametrize("world", [1, 2, 4])
def test_sharded_loopback_arena_equals_world1(monkeypatch, reproducible, world):
    """Item 10 (loopback): after consolidate() the arena of a loopback world of 2 / 4 is bit-identical to the world-1 sharded step's - and
    that one to the replicated step's arena up to the norm's summation order (the weights themselves differ by that, so it is compared
    to world 1, as the sharded weights are)."""
    _, ref, _ = _train(monkeypatch, "fused", 1, 2)
    _, got, _ = _train(monkeypatch, "fused", world, 2)
    np.testing.assert_array_equal(got, ref)


def test_one_rank_rccl_arena_equals_world1(monkeypatch, reproducible):
    """Item 10 (the real RCCL path of the C ABI, one rank, GGET_FORCE_STAGED=1): the consolidated arena equals the loopback world 1's."""
    _, ref, _ = _train(monkeypatch, "fused", 1, 2)
    _, got, _ = _train(monkeypatch, "fused", 0, 2)
    np.testing.assert_array_equal(got, ref)


# ------------------------------------------------------------------------------------------------ item 10 on a REAL partition: two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, tmp):
    os.environ["GGET_DETERMINISTIC"] = "1"
    os.environ["GGET_VARLEN"] = "0"
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="env://")
    modeling, tr, synth = _mods()
    L.check(L.load().gget_debug_set(L.KEY_DETERMINISTIC, 1))
    out = {}
    for zero in (0, 2):
        model = modeling.GraphGPTPretrainBase(_cfg(modeling), seed=1)
        eng = tr.initialize(model, tr.OptimConfig(lr=1e-3, max_grad_norm=0.0, zero_stage=zero, use_ema=True, ema_decay=0.9))
        assert eng.sharded == (zero > 0) and eng.world == world
        data = _batch(synth, rank)
        for _ in range(4):
            tr.batch_training(data, eng)
        e = model._engine
        refused = 0
        if zero:
            assert e.shard_stale and e.ema_stale
            for attempt in (lambda: eng.ema_weights().__enter__(), lambda: eng.save_ema_checkpoint(os.path.join(tmp, f"r{rank}")),
                            lambda: eng.ema_state_dict()):
                try:
                    attempt()
                except RuntimeError as ex:
                    refused += "consolidate()" in str(ex)
        eng.consolidate()
        assert not e.shard_stale and not e.ema_stale
        with eng.ema_weights():
            pass
        torch.cuda.synchronize()
        out[zero] = dict(ema=_bits(e.ema), master=_bits(e.master), refused=refused)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_gloo_sharded_ema_refuses_then_equals_replicated(tmp_path):
    """Item 10 where the state is REALLY partitioned (two ranks on cuda:0 over gloo; a loopback world and a one-rank communicator hold
    every share themselves, so nothing is stale there and - like save_checkpoint - nothing refuses): before consolidate() ema_weights,
    save_ema_checkpoint and ema_state_dict refuse with save_checkpoint's wording; after it the arena is identical on both ranks and,
    with clipping off, bit-identical to the replicated two-rank run's."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in ps:
        p.start()
    res = [r[1] for r in sorted((q.get(timeout=300) for _ in range(2)), key=lambda t: t[0])]
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    assert res[0][2]["refused"] == 3 and res[1][2]["refused"] == 3
    np.testing.assert_array_equal(res[0][2]["ema"], res[1][2]["ema"])
    np.testing.assert_array_equal(res[0][2]["master"], res[0][0]["master"])
    np.testing.assert_array_equal(res[0][2]["ema"], res[0][0]["ema"])
    assert not np.array_equal(res[0][2]["ema"], res[0][2]["master"])


# ------------------------------------------------------------------------------------------------ item 3: against float64
def _raw_engine(size):
    eng_mod = importlib.import_module("graph-gpt_amd.engine")
    spec = importlib.import_module("graph-gpt_amd.spec").spec_from_size(size, vocab_size=756, stacked_feat=13, next_n_token=13)
    e = eng_mod.Engine(spec, max_tokens=256, max_batch=8)
    e.ema_attach()
    return e


def _random_arena(n, gen):
    """zeros, tiny normal values (1e-30), 1e4-sized values and ordinary weights, mixed by position"""
    x = torch.randn(n, generator=gen, device="cuda") * 0.05
    kind = torch.randint(0, 8, (n,), generator=gen, device="cuda")
    x = torch.where(kind == 0, torch.zeros_like(x), x)
    x = torch.where(kind == 1, torch.sign(x) * 1e-30, x)
    x = torch.where(kind == 2, x * 2e5, x)
    return x


@pytest.mark.parametrize("size", ["tiny", "base"])
@pytest.mark.parametrize("d", [0.0, 0.5, 0.9999])
def test_one_update_against_float64(size, d):
    """Item 3, one update, EVERY element of the arena: the stand-alone launch, the fused launch (against the new weights read back) and
    the fused launch of a skipped step (against the unchanged weights), on arenas that hold zeros, 1e-30 and 1e4-sized values."""
    e = _raw_engine(size)
    gen = torch.Generator(device="cuda").manual_seed(11)
    w, ema0 = _random_arena(e.n_params, gen), _random_arena(e.n_params, gen)
    assert bool((w == 0).any()) and bool((w.abs() == 1e-30).any()) and bool((w.abs() > 1e3).any())
    e.master.copy_(w)
    e.ema.copy_(ema0)
    e.ema_update(d)
    torch.cuda.synchronize()
    ref, bound = _lerp64(w, ema0, d)
    _check(e.ema, ref, bound, f"standalone_{size}_d{d}")
    if d == 0.0:
        np.testing.assert_array_equal(_bits(e.ema), _bits(w))          # item 4: decay 0 copies the weights bit for bit
    # fused: AdamW on injected gradients, the lerp against the NEW weights
    e.ema.copy_(ema0)
    e.grad_bf16.copy_((torch.randn(e.n_params, generator=gen, device="cuda") * 0.01).to(torch.bfloat16))
    e.set_ema_decay(d)
    e.adamw_step(1e-3, max_grad_norm=1.0)
    torch.cuda.synchronize()
    assert not torch.equal(e.master, w)
    ref, bound = _lerp64(e.master, ema0, d)
    _check(e.ema, ref, bound, f"fused_{size}_d{d}")
    # the decay was consumed: the next step leaves the arena alone
    before = e.ema.clone()
    e.adamw_step(1e-3, max_grad_norm=1.0)
    torch.cuda.synchronize()
    assert torch.equal(e.ema, before)
    # fused, a step the skip rule drops (a non-finite gradient written into the gradient arena): the lerp against the UNCHANGED weights
    e.set_option(L.OPT_SKIP_NONFINITE_STEP, 1)
    w1, m1, v1 = e.master.clone(), e.adam_m.clone(), e.adam_v.clone()
    e.ema.copy_(ema0)
    e.grad_bf16[12345] = float("inf")
    e.set_ema_decay(d)
    gn = e.adamw_step(1e-3, max_grad_norm=1.0)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(gn))
    assert torch.equal(e.master, w1) and torch.equal(e.adam_m, m1) and torch.equal(e.adam_v, v1)
    ref, bound = _lerp64(w1, ema0, d)
    _check(e.ema, ref, bound, f"fused_skipped_{size}_d{d}")


def test_fifty_chained_updates_against_float64():
    """Item 3, n = 50 chained fused steps at d = 0.9999 and 0.5: a float64 chain driven by the engine's OWN master weights read back after
    each step (AdamW's rounding is not in the comparison), bound n * 8 * 2^-24 * (largest max(|ema|, |w|) of the element so far)."""
    for d in (0.9999, 0.5):
        e = _raw_engine("tiny")
        gen = torch.Generator(device="cuda").manual_seed(5)
        e.master.copy_(_random_arena(e.n_params, gen))
        e.ema_update(0.0)
        ref = e.master.double().clone()
        big = ref.abs()
        for n in range(1, 51):
            e.grad_bf16.copy_((torch.randn(e.n_params, generator=gen, device="cuda") * 0.01).to(torch.bfloat16))
            e.set_ema_decay(d)
            e.adamw_step(1e-3, max_grad_norm=1.0)
            big = torch.maximum(big, torch.maximum(ref.abs(), e.master.double().abs()))
            ref, _ = _lerp64(e.master, ref, d)
            if n in (1, 10, 50):
                torch.cuda.synchronize()
                _check(e.ema, ref, n * EPS * big, f"chain_n{n}_d{d}")


# ------------------------------------------------------------------------------------------------ item 4: seeding through GgetEngine
def test_first_two_steps_copy_third_averages(reproducible):
    modeling, tr, synth = _mods()
    model = modeling.GraphGPTPretrainBase(_cfg(modeling), seed=1)
    eng = tr.initialize(model, tr.OptimConfig(lr=1e-3, use_ema=True, ema_decay=0.9999))
    same = []
    for s in range(3):
        tr.batch_training(_batch(synth, s), eng)
        torch.cuda.synchronize()
        e = model._engine
        same.append(bool(torch.equal(e.ema, e.master)))
    assert same == [True, True, False] and eng.ema_updates == 3


# ------------------------------------------------------------------------------------------------ item 6: the skipped step
@pytest.mark.parametrize("world,zero", [(0, 0), (2, 2)])
def test_skipped_step_still_averages(monkeypatch, reproducible, world, zero):
    modeling, tr, synth = _mods()
    _env(monkeypatch, world, zero)
    model = modeling.GraphGPTPretrainBase(_cfg(modeling), seed=1)
    eng = tr.initialize(model, tr.OptimConfig(lr=1e-2, use_ema=True, ema_decay=0.5))
    eng.set_skip_nonfinite(True)
    for s in range(3):
        tr.batch_training(_batch(synth, s), eng)
    e = model._engine
    e.await_params()
    torch.cuda.synchronize()
    assert not torch.equal(e.ema, e.master)
    w0, m0, v0, ema0, p0 = e.master.clone(), e.adam_m.clone(), e.adam_v.clone(), e.ema.clone(), e.param_bf16.clone()
    b = _batch(synth, 3)
    out = eng(input_ids=b["input_ids"], attention_mask=b["attention_mask"], labels=b["labels"])
    eng.backward(out.head1_loss)
    torch.cuda.synchronize()
    e.grad_bf16[12345] = float("inf")       # (the GradScaler path: a non-finite gradient, written into the gradient arena)
    gn = eng.step()
    e.await_params()
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(gn)) and eng.skipped_steps == 1 and e.step_count == 3
    assert torch.equal(e.master, w0) and torch.equal(e.adam_m, m0) and torch.equal(e.adam_v, v0) and torch.equal(e.param_bf16, p0)
    assert eng.ema_decay_at(3) == 0.5
    ref, bound = _lerp64(w0, ema0, 0.5)
    _check(e.ema, ref, bound, f"skipped_step_world{world}")
    assert not torch.equal(e.ema, ema0)
    if e.comm_world:
        e.comm_destroy()


# ------------------------------------------------------------------------------------------------ item 7: gradient accumulation
def test_gradient_accumulation_averages_on_every_micro_step(reproducible):
    """k = 2: every step() call averages - the stand-alone lerp against the old weights on the non-boundary micro-step, the fused lerp
    against the new ones at the update - as the reference calls update_ema after every micro-batch."""
    modeling, tr, synth = _mods()
    model = modeling.GraphGPTPretrainBase(_cfg(modeling), seed=1)
    eng = tr.initialize(model, tr.OptimConfig(lr=1e-2, use_ema=True, ema_decay=0.5, gradient_accumulation_steps=2))
    model.cuda()
    ref = model._engine.master.double().clone()
    big = ref.abs()
    updates = 0
    for i in range(6):
        w_before = model._engine.master.clone()
        tr.batch_training(_batch(synth, i), eng)
        torch.cuda.synchronize()
        e = model._engine
        changed = not torch.equal(e.master, w_before)
        assert changed == (i % 2 == 1), f"micro-step {i}"
        updates += changed
        big = torch.maximum(big, torch.maximum(ref.abs(), e.master.double().abs()))
        ref, _ = _lerp64(e.master, ref, eng.ema_decay_at(i))
        _check(e.ema, ref, (i + 1) * EPS * big, f"accumulation_micro_step{i}")
    assert updates == 3 and eng.global_steps == 3 and eng.ema_updates == 6
    assert not torch.equal(e.ema, e.master)


# ------------------------------------------------------------------------------------------------ item 8: evaluation on the averaged weights
@pytest.mark.parametrize("S", [24, 256])
def test_eval_inside_ema_weights(reproducible, S):
    """Inside ema_weights() the eval-mode loss and logits equal, bitwise, those of a second model loaded from ema_state_dict(); after the
    block the live model's again.  S = 24 runs the per-sample kernels (packed o weights), S = 256 the GEMM path - and makes the model
    re-create its engine for the larger batch INSIDE the block."""
    modeling, tr, synth = _mods()
    model = modeling.GraphGPTTaskModel(_ft_cfg(modeling), seed=1)
    eng = tr.initialize(model, tr.OptimConfig(lr=1e-2, use_ema=True, ema_decay=0.5))
    for s in range(4):
        tr.ft_batch_training(_ft_batch(synth, s), eng)
    b = _ft_batch(synth, 50, B=4, S=S)
    kw = dict(input_ids=b["input_ids"], attention_mask=b["attention_mask"], task_labels=b["task_labels"])

    def run(m):
        o = m(**kw)
        torch.cuda.synchronize()
        return _bits(o.task_loss.detach().float().reshape(1)), _bits(o.task_logits.detach().float())

    model.eval()
    live = run(model)
    with eng.ema_weights():
        inside = run(model)
        with pytest.raises(RuntimeError, match="ema_weights"):      # training inside the block fails loudly
            eng.step()
    after = run(model)
    other = modeling.GraphGPTTaskModel(_ft_cfg(modeling), seed=2)
    other.load_state_dict(eng.ema_state_dict())
    other.cuda()
    other.eval()
    want = run(other)
    for a, b_ in zip(inside, want):
        np.testing.assert_array_equal(a, b_)
    for a, b_ in zip(after, live):
        np.testing.assert_array_equal(a, b_)
    assert not np.array_equal(inside[1], live[1]), "the averaged weights must give other logits than the live ones"
    # training goes on from the live weights
    model.train()
    tr.ft_batch_training(_ft_batch(synth, 9), eng)


# ------------------------------------------------------------------------------------------------ item 9: checkpoints
def test_checkpoint_round_trip_continues_the_average(reproducible, tmp_path):
    modeling, tr, synth = _mods()
    CK = importlib.import_module("graph-gpt_amd.checkpoint")
    optim = lambda: tr.OptimConfig(lr=1e-2, use_ema=True, ema_decay=0.5)

    def fresh():
        m = modeling.GraphGPTTaskModel(_ft_cfg(modeling), seed=1)
        m.cuda()
        return m, tr.initialize(m, optim())
    m1, e1 = fresh()
    for s in range(6):
        tr.ft_batch_training(_ft_batch(synth, s), e1)
    m2, e2 = fresh()
    for s in range(3):
        tr.ft_batch_training(_ft_batch(synth, s), e2)
    ckp = str(tmp_path / "run" / "epoch_1")
    e2.save_checkpoint(ckp)
    assert os.path.isfile(os.path.join(ckp, "model.pt")) and os.path.isfile(os.path.join(ckp, "model_ema.pt"))
    m3, e3 = fresh()
    e3.load_checkpoint(ckp)
    assert e3.ema_updates == 3 and m3._engine.ema_live
    for s in range(3, 6):
        tr.ft_batch_training(_ft_batch(synth, s), e3)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(m3._engine.master), _bits(m1._engine.master))
    np.testing.assert_array_equal(_bits(m3._engine.ema), _bits(m1._engine.ema))
    assert not torch.equal(m1._engine.ema, m1._engine.master)
    # model_ema_best.pt next to the epoch directories is what load_from_ckp_with_try(..., use_ema=True) reads
    e1.save_ema_checkpoint(str(tmp_path / "run"), best=True)
    m4 = modeling.GraphGPTTaskModel(_ft_cfg(modeling), seed=3)
    CK.load_from_ckp_with_try(m4, ckp, skip_keys=False, strict=True, use_ema=True)
    assert m4.last_load_result == ([], [])
    sd = e1.ema_state_dict()
    for k, v in m4.state_dict().items():
        assert v.shape == sd[k].shape and torch.equal(v.cpu(), sd[k].cpu()), k
    # a run that does not average leaves the model_ema.pt of the checkpoint alone: no arena
    m6 = modeling.GraphGPTTaskModel(_ft_cfg(modeling), seed=1)
    m6.cuda()
    e6 = tr.initialize(m6, tr.OptimConfig(lr=1e-2))
    e6.load_checkpoint(ckp)
    assert m6._engine.ema is None and e6.global_steps == 3
    # load_ema_checkpoint = EMAStats.load_ema_ckp
    m5, e5 = fresh()
    e5.load_ema_checkpoint(str(tmp_path / "run"))
    assert torch.equal(m5._engine.ema, m1._engine.ema)


# ------------------------------------------------------------------------------------------------ item 11: the pipeline
@pytest.mark.parametrize("use_ema", [True, False])
def test_finetune_pipeline_writes_model_ema(tmp_path, use_ema):
    import copy
    import types
    T = importlib.import_module("graph-gpt_amd.training")
    synth = importlib.import_module("graph-gpt_amd.synth")
    with open(os.path.join(ROOT, "tests", "golden", "pipeline_config.json")) as fh:
        case = json.load(fh)["finetune_ds"]

    def ns(o):
        return types.SimpleNamespace(**{k: ns(v) for k, v in o.items()}) if isinstance(o, dict) else o
    cfg = types.SimpleNamespace(tokenization=None, model=ns(copy.deepcopy(case["model_nested"])), training=ns(copy.deepcopy(case["training"])),
                                generation=None)
    m = cfg.model
    m.hidden_size, m.num_hidden_layers, m.intermediate_size, m.num_attention_heads, m.head_dim = 128, 2, 512, 2, 64
    m.num_key_value_heads, m.max_position_embeddings = 2, 64
    m.dropout_settings.attention_dropout = m.dropout_settings.path_dropout = 0.0
    m.layer_scale_init_value = 0.0
    t = cfg.training
    t.output_dir, t.batch_size, t.deepspeed_conf_file = str(tmp_path / "out"), 8, ""
    t.schedule.epochs, t.schedule.warmup_epochs = 2, 0.5
    t.optimizer.use_ema, t.optimizer.ema_decay = use_ema, 0.5
    batches = [{k: torch.from_numpy(v) for k, v in synth.make_task_batch(B=8, S=32, F=4, V=41245, seed=70 + i).items()} for i in range(6)]
    p = T.TrainingPipeline(cfg, T.FinetuneMode(batches=batches, samples_per_gpu=16, vocab_size=41245, bos_token_id=1, eos_token_id=2)).run()
    assert p.engine.global_steps == 4 and p.optim.use_ema is use_ema
    path = os.path.join(t.output_dir, "model_ema.pt")
    assert os.path.isfile(os.path.join(t.output_dir, "model.pt"))
    e = p.model._engine
    if not use_ema:
        assert not os.path.exists(path) and e.ema is None
        return
    assert p.optim.ema_decay == 0.5 and p.engine.ema_updates == 4
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert list(sd) == list(p.model.state_dict())
    torch.cuda.synchronize()
    for k, v in sd.items():
        assert torch.equal(v.reshape(-1), e.view(k, "ema").reshape(-1).cpu()), k
    assert not torch.equal(e.ema, e.master)
