"""Gradient accumulation on the device (`optimizer.gradient_accumulation_steps = k`, reference conf_utils.py:59-66 -> the DeepSpeed
engine's fp32 accumulation): the accumulate kernel bit for bit, and the boundary step - norm, clip, AdamW - reading the fp32 sum in
every launch form, each element against the float64 restatement of tests/_adamw_ref.py under the bounds tests/test_gpu_adamw_exact.py
applies (R.verify_step, unchanged).

The model is the tiny one of the existing accumulation tests (d128 / L2 / H2, F 13, V 756, B 8, S 32) and the two micro-batches are
`synth.make_pretrain_batch` seeds 3 and 4, the pair test_gradient_accumulation_steps_on_the_deepspeed_branch uses.

What the element check sees.  The reference is fed the float64 sum g1 + g2 of the two recorded bf16 gradient arrays (exact in float64)
and grad_scale 1 / (world k); the coefficient is rebuilt in float64 from the norm the device reported, as in test_gpu_adamw_exact.
At step 1 (m = v = 0) the bound on m' is 6u |(1 - b1) ge|, u = 2^-24.  The device's ge starts from the fp32 sum, one rounding (u) away
from the float64 sum; a step that rounds the sum to bf16 first is 2^-9 = 32768 u away and fails.  Every test asserts that separation
on its own inputs (some element of m' of the two references differs by more than the bound), so a pass says something.

The norm: the device squares the fp32 sum, each square within 2u of the float64 one - two more units than R.norm_ratio's L counts."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _adamw_ref as R
from _util import ROOT, record_error, spec_mod

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
CFG = dict(hidden_act="gelu", vocab_size=756, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
           max_position_embeddings=64, causal_attention=False, stacked_feat=13, next_n_token=13)
_DP_ENV = ("GGET_DP_BACKEND", "GGET_DP_LOOPBACK_WORLD", "GGET_FORCE_STAGED", "GGET_ZERO_STAGE", "GGET_DP_FP32_REDUCE",
           "GGET_NORM_FROM_BACKWARD")


def _mods():
    return (importlib.import_module("graph-gpt_amd.modeling"), importlib.import_module("graph-gpt_amd.training"),
            importlib.import_module("graph-gpt_amd.synth"))


def _batches():
    synth = _mods()[2]
    return [{k: torch.from_numpy(v) for k, v in synth.make_pretrain_batch(B=8, S=32, F=13, V=756, seed=s).items() if k != "lengths"}
            for s in (3, 4)]


@pytest.fixture(scope="module")
def batches():
    return _batches()


@pytest.fixture
def reproducible():
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):
        yield


def _make(monkeypatch, k=2, clip=1.0, world=0, zero=0, fold=False, use_ema=False, seed=2):
    """(model, GgetEngine) under the data-parallel environment of one launch form; world 0 = the plain single-rank step"""
    M, T, _ = _mods()
    for name in _DP_ENV:
        monkeypatch.delenv(name, raising=False)
    if world:
        monkeypatch.setenv("GGET_DP_BACKEND", "abi")
        monkeypatch.setenv("GGET_DP_LOOPBACK_WORLD", str(world))
        monkeypatch.setenv("GGET_FORCE_STAGED", "1")
        monkeypatch.setenv("GGET_ZERO_STAGE", str(zero))
    if fold:
        monkeypatch.setenv("GGET_NORM_FROM_BACKWARD", "1")
    model = M.GraphGPTPretrainBase(M.GraphGPTConfig(**CFG), seed=seed).cuda().eval()
    eng = T.initialize(model, T.OptimConfig(lr=1e-3, max_grad_norm=clip, gradient_accumulation_steps=k, use_ema=use_ema))
    assert eng.sharded == (zero > 0)
    return model, eng


def _micro(eng, batch, poison=None):
    """forward + backward of one micro-batch; the gradient array as step() will meet it (behind the exchange), then step()"""
    out = eng(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"])
    eng.backward(out.head1_loss)
    e = eng.module._engine
    torch.cuda.synchronize()            # (every stream: a loopback exchange runs on the side stream)
    if poison is not None:
        e.grad_bf16[poison] = float("inf")
    g = e.grad_bf16.clone()
    return g, eng.step()


def _state(e):
    e.await_params()
    torch.cuda.synchronize()
    return dict(w=e.master.clone(), m=e.adam_m.clone(), v=e.adam_v.clone(), P=e.param_bf16.clone())


def _finish(model):
    e = model._engine
    if e is not None and e.comm_world:
        e.comm_destroy()


def _window_check(monkeypatch, batches, what, world=0, **form):
    """One k = 2 window over the two micro-batches; master, m, v and P of the boundary step per element against the float64 clip + AdamW
    of (g1 + g2) / (2 world), and the proof that the bf16-rounded sum would not pass."""
    model, eng = _make(monkeypatch, k=2, clip=1.0, world=world, **form)
    try:
        g1, r1 = _micro(eng, batches[0])
        e = model._engine
        assert r1 is None and eng.global_steps == 0 and eng.micro_steps == 1
        pre = _state(e)
        g2, gn = _micro(eng, batches[1])
        assert eng.global_steps == 1 and e.step_count == 1 and eng.micro_steps == 2
        assert eng._grad_acc is not None and eng._grad_acc.dtype == torch.float32
        post = _state(e)
        h = R.Hyper(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.1, max_norm=1.0, gs=1.0 / (2 * max(1, world)))
        gsum = g1.double() + g2.double()            # exact: two bf16 values in float64
        nrm = float(gn)
        c = R.coef64(h, nrm)
        out = R.verify_step(dict(w=pre["w"], m=pre["m"], v=pre["v"], g=gsum), post, h, 1, c)
        chain = (R.chain_shard(e.buckets) if form.get("zero") else R.chain_full(e.n_params)) + 2
        r, ref = R.norm_ratio(nrm, gsum, h.gs, chain)
        out["norm"] = (r, int(not r <= 1.0))
        print(f"[grad_accum] {what}: norm {nrm:.6g} (float64 {ref:.6g}), coefficient {c:.6g}, max |err| / bound = "
              + ", ".join(f"{k} {x:.4f}" for k, (x, _) in sorted(out.items())), flush=True)
        for k, (x, _) in out.items():
            record_error(f"grad_accum_{what}", f"{k}_err_over_bound", x, 1.0)
        # what the bf16 round trip of the sum would give: its m' against the un-rounded m', in units of the bound on m'
        gb = (g1.float() + g2.float()).to(torch.bfloat16).double()
        cb = R.coef64(h, R.f32(R.norm64(gb, h.gs)))
        m_new, m_old = (1.0 - h.b1) * gsum * c, (1.0 - h.b1) * gb * cb
        bound = 6 * R.U * m_new.abs()
        apart = int(((m_new - m_old).abs() > bound).sum())
        sep = float(((m_new - m_old).abs()[bound > 0] / bound[bound > 0]).max())
        print(f"[grad_accum] {what}: {apart} of {int((gsum != 0).sum())} elements of m' separate the bf16-rounded sum by more than the "
              f"bound (largest {sep:.1f} bounds)", flush=True)
        assert apart > 0, "the inputs do not tell the fp32 sum from its bf16 rounding"
        bad = {k: (n, round(x, 3)) for k, (x, n) in out.items() if n}
        assert not bad, f"{what}: elements outside the bound (count, largest ratio) {bad}"
        covered = torch.zeros(e.n_params, dtype=torch.bool, device="cuda")
        for p in e.params.values():
            covered[p["offset"]: p["offset"] + p["numel"]] = True
        for name, arena in (("master", e.master), ("m", e.adam_m), ("v", e.adam_v), ("grad_acc", e.grad_acc)):
            assert not bool(arena[~covered].any()), f"{what}: a gap or pad-row element of {name} is not zero"
        assert e.grad_acc_count() == 0
        return e, post
    finally:
        _finish(model)


# ------------------------------------------------------------------------------------------------ 1. the kernel, element by element
def test_accumulate_kernel_is_the_fp32_sum_bit_for_bit():
    """gget_grad_accumulate through the C ABI over three seeded bf16 arrays of magnitudes 2^-20 .. 2^4: after every call the arena is
    the running sum rounded to fp32 once per addition - numpy fp32 adds in the same order, and the float64 sum rounded once -, the count
    reads 1, 2, 3, gaps and pad rows are zero, and a bf16 rounding of the sum would be visible.  A closed window is overwritten."""
    import ctypes as C
    spec = spec_mod.spec_from_size("tiny", vocab_size=756, stacked_feat=13, next_n_token=13)
    e = importlib.import_module("graph-gpt_amd.engine").Engine(spec, max_tokens=256, max_batch=8)
    covered = torch.zeros(e.n_params, dtype=torch.bool, device="cuda")
    for p in e.params.values():
        covered[p["offset"]: p["offset"] + p["numel"]] = True
    assert int((~covered).sum()) > 0 and e.n_params // 8 > 256, "gaps, and more than one block"
    assert e.grad_acc is None
    acc = e.grad_acc_attach()
    acc.fill_(float("nan"))             # (whatever the arena holds: the first micro-step overwrites)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, ref32, ref64 = C.c_int32(-1), None, None
    for i, seed in enumerate((11, 12, 13)):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        mag = torch.exp2(-20.0 + 24.0 * torch.rand(e.n_params, generator=gen, device="cuda"))
        sign = torch.where(torch.rand(e.n_params, generator=gen, device="cuda") < 0.5, -1.0, 1.0)
        g = torch.where(covered, sign * mag, torch.zeros((), device="cuda")).to(torch.bfloat16)
        e.grad_bf16.copy_(g)
        L.check(e.lib.gget_grad_accumulate(e.h, st))
        L.check(e.lib.gget_grad_acc_count(e.h, C.byref(n)))
        assert n.value == i + 1
        torch.cuda.synchronize()
        g32 = g.float().cpu().numpy()
        got = acc.cpu().numpy()
        ref64 = g32.astype(np.float64) if ref32 is None else (ref32.astype(np.float64) + g32.astype(np.float64)).astype(np.float32)
        ref32 = g32.copy() if ref32 is None else ref32 + g32            # (numpy float32 add: one rounding)
        assert ref32.dtype == np.float32
        wrong = int((got.view(np.int32) != ref32.view(np.int32)).sum())
        wrong64 = int((got != ref64.astype(np.float32)).sum())
        record_error("grad_accum_kernel", f"bits_wrong_after_{i + 1}", wrong, 0)
        print(f"[grad_accum] kernel call {i + 1}: {wrong} elements differ from the fp32 sum, {wrong64} from the float64 sum rounded once", flush=True)
        assert wrong == 0 and wrong64 == 0
        assert not bool(acc[~covered].any()), "a gap or pad-row element of the accumulator is not zero"
        if i:
            assert int((acc != acc.to(torch.bfloat16).float()).sum()) > e.n_params // 4, "a bf16 rounding of the sum must be visible"
    # a closed window (count 0) is overwritten, not added to
    L.check(e.lib.gget_grad_acc_set_count(e.h, 0))
    L.check(e.lib.gget_grad_accumulate(e.h, st))
    torch.cuda.synchronize()
    assert torch.equal(acc, e.grad_bf16.float()) and e.grad_acc_count() == 1
    e.grad_acc_set_count(3)
    assert e.grad_acc_count() == 3
    e.grad_acc_detach()
    assert e.grad_acc_count() == 0 and e.grad_acc is None


# ------------------------------------------------------------------------------------------------ 2. AdamW consumes the un-rounded sum
def test_boundary_step_reads_the_unrounded_fp32_sum(monkeypatch, batches):
    """The replicated step.  Fails where the sum goes back to bf16 before AdamW: m' then carries a 2^-9 rounding against a bound of 6u."""
    _window_check(monkeypatch, batches, "replicated")


# ------------------------------------------------------------------------------------------------ 3. every launch form
def test_boundary_step_fused_ema(monkeypatch, batches):
    """adamw_kernel<.., EMA> on the fp32 source; the average follows the new weights (decay 0 on the first two updates: ema == master)"""
    e, post = _window_check(monkeypatch, batches, "fused_ema", use_ema=True)
    assert e.ema is not None and torch.equal(e.ema, post["w"])


@pytest.mark.parametrize("world", [1, 2])
def test_boundary_step_sharded(monkeypatch, batches, world):
    """adamw_items_kernel and the per-chunk norm partials on the fp32 source (ZeRO-2 on loopback worlds 1 and 2: the accumulator sums
    what the exchange left in the gradient array, world x the gradient)"""
    _window_check(monkeypatch, batches, f"sharded_world{world}", world=world, zero=2)


def test_boundary_step_norm_from_backward(monkeypatch, batches):
    """GGET_OPT_NORM_FROM_BACKWARD: the last backward's tile partials say nothing about a sum - the norm is the full pass over it"""
    _window_check(monkeypatch, batches, "norm_from_backward", fold=True)


def test_sharded_window_equals_replicated_without_clipping(monkeypatch, batches, reproducible):
    """k = 2 on a loopback world of 2, clipping off: the sharded and the replicated boundary step are bit-identical"""
    states = []
    for zero in (0, 2):
        model, eng = _make(monkeypatch, k=2, clip=0.0, world=2, zero=zero)
        try:
            for b in batches:
                _micro(eng, b)
            assert eng.global_steps == 1
            states.append(_state(model._engine))
        finally:
            _finish(model)
    for key in states[0]:
        assert torch.equal(states[0][key], states[1][key]), key


# ------------------------------------------------------------------------------------------------ 4. k = 1 is untouched
_K1_CHILD = """
import sys
import pytest, torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_gpu_grad_accum as G
G.L.check(G.L.load().gget_debug_set(G.L.KEY_DETERMINISTIC, 1))
mp = pytest.MonkeyPatch()
torch.save(G._k1_master(mp, G._batches()).cpu(), {out!r})
mp.undo()
print("k1-ok")
"""


def _k1_master(monkeypatch, bs):
    """master after three k = 1 steps (micro-batches A, B, A)"""
    model, eng = _make(monkeypatch, k=1)
    for b in (bs[0], bs[1], bs[0]):
        _, gn = _micro(eng, b)
        assert gn is not None
    e = model._engine
    assert eng.global_steps == 3 and e.step_count == 3
    assert e.grad_acc is None and e.grad_acc_count() == 0 and eng._grad_acc is None
    torch.cuda.synchronize()
    return e.master.clone()


def test_k1_attaches_nothing_and_is_bit_identical(monkeypatch, batches, reproducible, tmp_path):
    """Three k = 1 steps leave the count at 0 and attach no accumulator; master equals, bit for bit, the same three steps in a process
    in which no k > 1 engine ever existed (a fresh interpreter - what this test is about), although this process ran a k = 2 window
    first."""
    model, eng = _make(monkeypatch, k=2)
    for b in batches:
        _micro(eng, b)
    assert model._engine.grad_acc is not None
    here = _k1_master(monkeypatch, batches)
    out = str(tmp_path / "k1_master.pt")
    env = {k: v for k, v in os.environ.items() if k not in _DP_ENV}
    res = subprocess.run([sys.executable, "-c", _K1_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "k1-ok" in res.stdout, res.stderr[-2000:]
    there = torch.load(out, map_location="cuda")
    assert torch.equal(here, there)


# ------------------------------------------------------------------------------------------------ 5. the skip rule
def test_skipped_boundary_closes_the_window(monkeypatch, batches, reproducible):
    """set_skip_nonfinite(True) and an inf written into the first micro-batch's gradient (through the grad_bf16 view): the boundary step
    is skipped - weights and moments unchanged, one skipped step, the window closed - and the next window's update equals a fresh
    engine's first window, bit for bit."""
    def first_window(eng):
        for b in batches:
            _micro(eng, b)
        return _state(eng.module._engine)
    model0, eng0 = _make(monkeypatch, k=2)
    eng0.set_skip_nonfinite(True)
    want = first_window(eng0)
    assert eng0.skipped_steps == 0 and eng0.global_steps == 1

    model, eng = _make(monkeypatch, k=2)
    eng.set_skip_nonfinite(True)
    _, r = _micro(eng, batches[0], poison=54321)
    e = model._engine
    assert r is None and e.grad_acc_count() == 1
    assert any(p["offset"] <= 54321 < p["offset"] + p["numel"] for p in e.params.values()), "the poisoned element must be a parameter's"
    before = _state(e)
    _, gn = _micro(eng, batches[1])
    after = _state(e)
    assert not bool(torch.isfinite(gn))
    for k in before:
        assert torch.equal(before[k], after[k]), f"{k} moved in a skipped step"
    assert eng.skipped_steps == 1 and e.step_count == 0 and eng.global_steps == 1
    assert e.grad_acc_count() == 0
    got = first_window(eng)
    assert eng.skipped_steps == 1 and e.step_count == 1 and bool(torch.isfinite(eng.last_grad_norm))
    for k in want:
        assert torch.equal(want[k], got[k]), f"{k}: the window after a skipped one differs from a fresh engine's first"


# ------------------------------------------------------------------------------------------------ 6. a checkpoint inside a window
def test_checkpoint_inside_a_window_resumes_it(monkeypatch, batches, reproducible, tmp_path):
    """k = 2: one micro-step, save_checkpoint, a new engine, load_checkpoint, the second micro-step - master, m and v bit-identical to the
    uninterrupted run.  An optimizer.pt in the earlier layout (without micro_steps / grad_acc) still loads, with no window open."""
    model0, eng0 = _make(monkeypatch, k=2)
    for b in batches:
        _micro(eng0, b)
    want = _state(model0._engine)

    model1, eng1 = _make(monkeypatch, k=2)
    _micro(eng1, batches[0])
    eng1.save_checkpoint(str(tmp_path / "ck"))
    st = torch.load(str(tmp_path / "ck" / "optimizer.pt"), map_location="cpu")
    assert st["micro_steps"] == 1 and set(st["grad_acc"]) == set(model1._engine.params)

    model2, eng2 = _make(monkeypatch, k=2, seed=5)         # (other weights: the load must bring everything)
    eng2.load_checkpoint(str(tmp_path / "ck"))
    assert eng2.micro_steps == 1 and model2._engine.grad_acc_count() == 1
    _, gn = _micro(eng2, batches[1])
    assert gn is not None and eng2.global_steps == 1 and eng2.micro_steps == 2
    got = _state(model2._engine)
    for k in ("w", "m", "v", "P"):
        assert torch.equal(want[k], got[k]), f"{k}: the resumed window differs from the uninterrupted one"

    # the earlier layout: no window, and a checkpoint at a boundary carries no partial sum
    old = {k: v for k, v in st.items() if k not in ("micro_steps", "grad_acc")}
    os.makedirs(str(tmp_path / "old"))
    torch.save(old, str(tmp_path / "old" / "optimizer.pt"))
    torch.save(torch.load(str(tmp_path / "ck" / "model.pt"), map_location="cpu"), str(tmp_path / "old" / "model.pt"))
    model3, eng3 = _make(monkeypatch, k=2, seed=6)
    eng3.load_checkpoint(str(tmp_path / "old"))
    assert eng3.micro_steps == 0 and model3._engine.grad_acc_count() == 0
    assert torch.equal(model3._engine.adam_m, model1._engine.adam_m)
    eng2.save_checkpoint(str(tmp_path / "ck2"))
    st2 = torch.load(str(tmp_path / "ck2" / "optimizer.pt"), map_location="cpu")
    assert st2["micro_steps"] == 2 and "grad_acc" not in st2
