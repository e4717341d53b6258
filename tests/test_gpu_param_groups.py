"""Parameter groups on the device (gget_set_param_scales): the clip + AdamW step with per-parameter scales of lr and weight decay,
every element of every arena against the float64 restatement of tests/_adamw_ref.py.

Method.  The kernel forms lr_i = lr * lr_scale and wd_i = wd * wd_scale per work item, one fp32 product each, and the two values enter
the per-element update unchanged - so the arenas are cut into segments of equal scales (a parameter reaches to the next parameter's
offset: its alignment gap and, behind lm_head.weight, the pad rows ride with it) and R.verify_step runs per segment on slices of the pre
and post arenas with Hyper(lr = f32(f32(lr) f32(s)), wd = f32(f32(wd) f32(sw))) and the bounds of tests/_adamw_ref.py unchanged.  Every
element of every arena is checked, none is filtered; the norm is checked on its own (over all trainable gradients whatever their scale)
and gaps and pad rows must stay zero.  Inputs: R.make_inputs as tests/test_gpu_adamw_exact.py, on the tiny and the 2-layer d = 768 model.
Scales unless a case says otherwise: the reference's layer-wise lr decay v1 at 0.5 (six different lr scales, 1 down to 1/32) and
weight-decay scale 0 on every 1-D parameter.

GGET_PARAM_GROUPS_PARITY_OUT=<path> writes the ratios of a whole run of this file there (profiles/param_groups_parity.json)."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest
import torch

import _adamw_ref as R
from _util import spec_mod

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
_RATIOS = {}
_ENGINES = {}
EMA_EPS = 8.0 * R.U
MODELS = ["tiny", "d768"]


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
    """one raw engine per model for the replicated, unfrozen cases (every case writes the whole state and sets its own table)"""
    if model not in _ENGINES:
        _ENGINES[model] = _new_engine(model)
    return _ENGINES[model]


def _scales(e, lr_decay=0.5):
    """({name: lr_scale}, {name: wd_scale}): layer-wise lr decay v1 and no weight decay on 1-D parameters"""
    T = importlib.import_module("graph-gpt_amd.training")
    depth = T.layerwise_depths(e.params, e.spec.num_layers, 1, True)
    lr_s = {k: lr_decay ** d for k, d in depth.items()}
    wd_s = {k: 0.0 if len(p["shape"]) == 1 else 1.0 for k, p in e.params.items()}
    assert len(set(lr_s.values())) == e.spec.num_layers + 3 and 0.0 in wd_s.values() and 1.0 in wd_s.values()
    return lr_s, wd_s


def _segments(e, lr_s, wd_s, ranges=None):
    """[(lo, hi, lr_scale, wd_scale)]: the arena cut where a scale changes, clipped to `ranges` ([(offset, count)]; None = everything)"""
    names = list(e.params)
    offs = [e.params[k]["offset"] for k in names]
    assert offs == sorted(offs) and offs[0] == 0
    segs = []
    for k, lo, hi in zip(names, offs, offs[1:] + [e.n_params]):
        a, b = float(lr_s.get(k, 1.0)), float(wd_s.get(k, 1.0))
        if segs and segs[-1][2:] == (a, b):
            segs[-1] = (segs[-1][0], hi, a, b)
        else:
            segs.append((lo, hi, a, b))
    if ranges is None:
        return segs
    return [(max(lo, o), min(hi, o + c), a, b) for lo, hi, a, b in segs for o, c in ranges if max(lo, o) < min(hi, o + c)]


def _inject(e, **arenas):
    for which, flat in arenas.items():
        for k, p in e.params.items():
            e.view(k, which).copy_(flat[p["offset"]: p["offset"] + p["numel"]].view(p["shape"]))


def _pre(e, g=None):
    torch.cuda.synchronize()
    return dict(w=e.master.clone(), m=e.adam_m.clone(), v=e.adam_v.clone(), g=e.grad_bf16.clone() if g is None else g, P=e.param_bf16.clone())


def _post(e):
    e.await_params()
    torch.cuda.synchronize()
    return dict(w=e.master, m=e.adam_m, v=e.adam_v, P=e.param_bf16)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b, what, sl=slice(None)):
    for k in a:
        if k in b and k != "g":
            assert torch.equal(_bits(a[k][sl]), _bits(b[k][sl])), f"{what}: {k} differs"


def _record(what, out):
    _RATIOS[what] = {k: round(r, 6) for k, (r, _) in out.items()}
    print(f"[param_groups] {what}: max |err| / bound = " + ", ".join(f"{k} {r:.4f}" for k, (r, _) in sorted(out.items())), flush=True)
    bad = {k: (n, round(r, 3)) for k, (r, n) in out.items() if n}
    assert not bad, f"{what}: elements outside the bound (count, largest ratio) {bad}"


def _gaps_zero(e, what):
    gap = ~e.covered
    for name, arena in (("master", e.master), ("m", e.adam_m), ("v", e.adam_v), ("P", e.param_bf16), ("grad", e.grad_bf16), ("ema", e.ema),
                        ("grad_acc", e.grad_acc)):
        if arena is not None:
            assert not bool(arena[gap].any()), f"{what}: a gap or pad-row element of {name} is not zero"


def _verify(e, pre, gn, h, chain, what, lr_s, wd_s, ranges=None):
    """the element check of every segment, the norm check and the gaps of the step that just ran (t = e.step_count); with `ranges` (the
    trainable ones) everything outside them must keep its bits"""
    post = _post(e)
    nrm = float(gn)
    c = R.coef64(h, nrm)
    out = {"m": (0.0, 0), "v": (0.0, 0), "w": (0.0, 0), "P": (0.0, 0)}
    seen = torch.zeros(e.n_params, dtype=torch.bool, device="cuda")
    for lo, hi, a, b in _segments(e, lr_s, wd_s, ranges):
        hs = h.replace(lr=np.float32(h.lr) * np.float32(a), wd=np.float32(h.wd) * np.float32(b))      # (one fp32 product each)
        o = R.verify_step({k: x[lo:hi] for k, x in pre.items()}, {k: x[lo:hi] for k, x in post.items()}, hs, e.step_count, c)
        out = {k: (max(out[k][0], o[k][0]), out[k][1] + o[k][1]) for k in out}
        seen[lo:hi] = True
    if ranges is None:
        assert bool(seen.all())
        g = pre["g"]
    else:
        _same_bits({k: x[~seen] for k, x in pre.items()}, {k: x[~seen] for k, x in post.items()}, f"{what} (frozen ranges)")
        g = torch.where(seen, pre["g"], torch.zeros_like(pre["g"]))
    r, _ = R.norm_ratio(nrm, g, h.gs, chain)
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


def _case(e, h0, clip, what, seed, lr_s, wd_s, steps=((None, 3), (99, 1)), sharded=False, world=1, chain=None, ranges=None):
    """`steps`: (step_count preset or None = go on, number of chained steps): t = 1, 2, 3 and 100 by default.  The whole state is
    written before the first step of every group, fresh gradients before every step."""
    chain = chain or R.chain_full(e.n_params)
    e.step_count = 0
    for preset, count in steps:
        if preset is not None:
            e.step_count = preset
        for i in range(count):
            w, m, v, g, h = R.make_inputs(e.n_params, seed + 31 * e.step_count, h0, device="cuda", covered=e.covered, world=world, clip=clip)
            _inject(e, grad=g, **(dict(master=w, m=m, v=v) if i == 0 else {}))
            if world > 1:
                for b in range(len(e.buckets)):
                    e.reduce_scatter_grads_async(b)        # (the loopback exchange: the arena times `world`)
            pre = _pre(e)
            gn = _step(e, h, sharded)
            _verify(e, pre, gn, h, chain, f"{what}_t{e.step_count}", lr_s, wd_s, ranges)


@pytest.fixture(scope="module", autouse=True)
def _write_ratios():
    yield
    _ENGINES.clear()
    path = os.environ.get("GGET_PARAM_GROUPS_PARITY_OUT")
    if _RATIOS and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        worst = {}
        for r in _RATIOS.values():
            for k, x in r.items():
                worst[k] = max(worst.get(k, 0.0), x)
        with open(path, "w") as fh:
            json.dump({"what": "largest |device - float64 restatement| / bound per check of tests/test_gpu_param_groups.py (bounds: "
                               "tests/_adamw_ref.py, per scale segment with lr = f32(lr * lr_scale), wd = f32(wd * wd_scale)), every element "
                               "of every arena checked; P = 1 if any bf16 bit differs from RNE(master'); ratios are findings, not thresholds",
                       "largest": worst, "ratios": _RATIOS}, fh, indent=1)


# ------------------------------------------------------------------------------------------------ 1: the replicated grouped step
@pytest.mark.parametrize("clip", ["off", "active"])
@pytest.mark.parametrize("model", MODELS)
def test_grouped_replicated_step(model, clip):
    """the whole arena as work items (adamw_group_items_kernel instead of the grid-stride launch): clip off and active, t = 1, 2, 3
    chained and t = 100; the norm (the full pass, over every gradient whatever its scale) inside its bound, gaps and pad rows zero.
    Scales that are accepted and ignored fail here: the embedding runs at lr / 32, every 1-D parameter without weight decay."""
    e = _engine(model)
    lr_s, wd_s = _scales(e)
    e.set_param_scales(lr_s, wd_s)
    got = e.param_scales()
    assert got == (lr_s, wd_s)      # (powers of two: exact in fp32)
    try:
        _case(e, R.Hyper(), clip, f"replicated_{model}_{clip}", 100, lr_s, wd_s)
    finally:
        e.set_param_scales(None, None)
    assert set(e.param_scales()[0].values()) == {1.0} and set(e.param_scales()[1].values()) == {1.0}


# ------------------------------------------------------------------------------------------------ 2: all ones = no table, bit for bit
@pytest.mark.parametrize("model", MODELS)
def test_all_ones_equal_the_ungrouped_step_bit_for_bit(model):
    e = _engine(model)
    ones = {k: 1.0 for k in e.params}
    runs = []
    for table in (None, ones):
        e.set_param_scales(table, table)
        e.step_count = 0
        snaps = []
        for i in range(2):
            w, m, v, g, h = R.make_inputs(e.n_params, 700 + i, R.Hyper(), device="cuda", covered=e.covered, clip="active")
            _inject(e, grad=g, **(dict(master=w, m=m, v=v) if i == 0 else {}))
            gn = _step(e, h)
            snaps.append({**{k: x.clone() for k, x in _post(e).items()}, "norm": gn.reshape(1).clone()})
        runs.append(snaps)
    e.set_param_scales(None, None)
    for a, b in zip(*runs):
        _same_bits(a, b, f"all ones {model}")


# ------------------------------------------------------------------------------------------------ 3: one layer at lr_scale 0
@pytest.mark.parametrize("model", MODELS)
def test_lr_scale_zero_keeps_master_and_bf16_bits(model):
    """torch's lr = 0 group: m and v of layer 1 move (inside their bounds), its master weights and bf16 copy keep their bits; every
    other element is what it is when layer 1 trains (the clip norm is over all gradients either way)."""
    e = _engine(model)
    lr_s, wd_s = _scales(e)
    layer1 = [k for k, p in e.params.items() if p["layer"] == 1]
    lo = e.params[layer1[0]]["offset"]
    hi = e.params["model.norm.weight"]["offset"]
    assert all(lo <= e.params[k]["offset"] < hi for k in layer1) and len(layer1) >= 9
    zero = dict(lr_s, **{k: 0.0 for k in layer1})
    w, m, v, g, h = R.make_inputs(e.n_params, 800, R.Hyper(), device="cuda", covered=e.covered, clip="active")
    snaps = []
    try:
        for table in (zero, lr_s):
            e.set_param_scales(table, wd_s)
            _inject(e, master=w, m=m, v=v, grad=g)
            e.sync_params()                     # (the bf16 copy is RNE(master) before the step, as after any step)
            e.step_count = 4
            pre = _pre(e)
            p0 = e.param_bf16.clone()
            post = _verify(e, pre, _step(e, h), h, R.chain_full(e.n_params), f"lr0_{model}_{'zero' if table is zero else 'train'}", table, wd_s)
            snaps.append({k: x.clone() for k, x in post.items()})
            if table is zero:
                assert torch.equal(_bits(post["w"][lo:hi]), _bits(pre["w"][lo:hi])), "master of the lr_scale 0 layer moved"
                assert torch.equal(_bits(post["P"][lo:hi]), _bits(p0[lo:hi])), "bf16 copy of the lr_scale 0 layer moved"
                assert not torch.equal(post["m"][lo:hi], pre["m"][lo:hi]) and not torch.equal(post["v"][lo:hi], pre["v"][lo:hi])
            else:
                assert not torch.equal(post["w"][lo:hi], pre["w"][lo:hi])
    finally:
        e.set_param_scales(None, None)
    a, b = snaps
    for sl in (slice(0, lo), slice(hi, e.n_params)):
        _same_bits(a, b, f"lr0 {model}: outside layer 1", sl)
    _same_bits({k: a[k] for k in "mv"}, {k: b[k] for k in "mv"}, f"lr0 {model}: moments of layer 1", slice(lo, hi))


# ------------------------------------------------------------------------------------------------ 4: fused EMA
def test_fused_ema_with_groups():
    """the EMA instantiation of the grouped kernel: the element check, and the EMA within 8u max(|ema|, |w'|) of w' + d32 (ema - w')
    against the NEW master weights read back (the check of test_fused_ema_step)"""
    e = _engine("tiny")
    lr_s, wd_s = _scales(e)
    e.set_param_scales(lr_s, wd_s)
    e.ema_attach()
    try:
        for d in (0.5, 0.9999):
            w, m, v, g, h = R.make_inputs(e.n_params, 400, R.Hyper(), device="cuda", covered=e.covered, clip="active")
            ema0 = torch.where(e.covered, 0.05 * torch.randn(e.n_params, device="cuda", generator=torch.Generator("cuda").manual_seed(9)),
                               torch.zeros((), device="cuda"))
            _inject(e, master=w, m=m, v=v, grad=g, ema=ema0)
            e.step_count = 1
            pre = _pre(e)
            e.set_ema_decay(d)
            post = _verify(e, pre, _step(e, h), h, R.chain_full(e.n_params), f"fused_ema_tiny_d{d}", lr_s, wd_s)
            w64, e64 = post["w"].double(), ema0.double()
            err = (e.ema.double() - (w64 + R.f32(d) * (e64 - w64))).abs()
            r, bad = R._ratio(err, EMA_EPS * torch.maximum(w64.abs(), e64.abs()))
            _record(f"fused_ema_tiny_d{d}_ema", {"ema": (r, bad)})
            assert not torch.equal(e.ema, ema0)
    finally:
        e.ema_detach()
        e.set_param_scales(None, None)


# ------------------------------------------------------------------------------------------------ 5: frozen prefix
@pytest.mark.parametrize("order", ["freeze_first", "scales_first"])
@pytest.mark.parametrize("model", MODELS)
def test_frozen_prefix_with_groups(model, order):
    """gget_set_frozen(1) and the table in either call order: the trainable ranges per element, the frozen ones bit for bit, the norm
    over the trainable gradients (the chunk pass)"""
    e = _new_engine(model)
    lr_s, wd_s = _scales(e)
    if order == "freeze_first":
        e.set_frozen(1)
        e.set_param_scales(lr_s, wd_s)
    else:
        e.set_param_scales(lr_s, wd_s)
        e.set_frozen(1)
    assert e.param_scales()[1] == wd_s
    n_train = sum(c for _, c in e.train_ranges)
    assert 0 < n_train < e.n_params
    _case(e, R.Hyper(), "active", f"frozen1_{model}_{order}", 900, lr_s, wd_s, steps=((None, 2),), chain=R.chain_chunks(n_train, 0),
          ranges=e.train_ranges)


# ------------------------------------------------------------------------------------------------ 6: the sharded step
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("model", MODELS)
def test_sharded_step_with_groups(model, world):
    """loopback worlds 1 and 2 (the handle does every rank's share): the element check with the clip active, and - clip off - every
    arena bit for bit what the replicated grouped step gives on the same gradients"""
    e = _new_engine(model)
    lr_s, wd_s = _scales(e)
    if world > 1:
        e.comm_init_loopback(world)
    e.shard_init(world, 0)
    e.set_param_scales(lr_s, wd_s)          # (after the plan: the call rebuilds it)
    try:
        h0 = R.Hyper(gs=1.0 / world)
        _case(e, h0, "active", f"sharded_{model}_world{world}_active", 500, lr_s, wd_s, steps=((None, 2), (99, 1)), sharded=True, world=world,
              chain=R.chain_shard(e.buckets))
        _case(e, h0, "off", f"sharded_{model}_world{world}_off", 510, lr_s, wd_s, steps=((5, 1),), sharded=True, world=world,
              chain=R.chain_shard(e.buckets))
        sharded = {k: x.clone() for k, x in _post(e).items()}
        # the same step, replicated: the gradients as the exchange left them
        r = _engine(model)
        r.set_param_scales(lr_s, wd_s)
        try:
            w, m, v, g, h = R.make_inputs(r.n_params, 510 + 31 * 5, h0, device="cuda", covered=r.covered, world=world, clip="off")
            _inject(r, master=w, m=m, v=v, grad=(g.float() * world).to(torch.bfloat16))
            assert torch.equal(r.grad_bf16, e.grad_bf16)
            r.step_count = 5
            _step(r, h)
            _same_bits(sharded, _post(r), f"sharded world {world} against replicated ({model})")
        finally:
            r.set_param_scales(None, None)
    finally:
        if e.comm_world:
            e.comm_destroy()


# ------------------------------------------------------------------------------------------------ 7: an fp32 accumulation window
@pytest.mark.parametrize("model", MODELS)
def test_accumulation_window_closed_by_a_grouped_step(model):
    """k = 2: the same gradients accumulated twice (the fp32 sum is 2 g exactly), grad_scale 1/2; norm, clip and the grouped update
    read the accumulator"""
    e = _engine(model)
    lr_s, wd_s = _scales(e)
    e.set_param_scales(lr_s, wd_s)
    try:
        w, m, v, g, h = R.make_inputs(e.n_params, 1000, R.Hyper(gs=0.5), device="cuda", covered=e.covered, world=2, clip="active")
        _inject(e, master=w, m=m, v=v, grad=g)
        e.grad_accumulate()
        e.grad_accumulate()
        assert e.grad_acc_count() == 2
        torch.cuda.synchronize()
        acc = e.grad_acc.clone()
        assert torch.equal(acc, g.float() * 2)
        e.step_count = 2
        pre = _pre(e, g=acc)
        _verify(e, pre, _step(e, h), h, R.chain_full(e.n_params), f"accum2_{model}", lr_s, wd_s)
        assert e.grad_acc_count() == 0
    finally:
        e.grad_acc_detach()
        e.set_param_scales(None, None)


# ------------------------------------------------------------------------------------------------ 8: the skip rule
def test_skip_rule_with_groups_changes_nothing():
    e = _engine("tiny")
    lr_s, wd_s = _scales(e)
    e.set_param_scales(lr_s, wd_s)
    e.set_option(L.OPT_SKIP_NONFINITE_STEP, 1)
    try:
        w, m, v, g, h = R.make_inputs(e.n_params, 600, R.Hyper(), device="cuda", covered=e.covered, clip="active")
        _inject(e, master=w, m=m, v=v, grad=g)
        e.sync_params()
        at = int(torch.nonzero(e.covered)[12345])
        for bad in (float("inf"), float("nan")):
            _inject(e, grad=g)
            e.grad_bf16[at] = bad
            e.step_count = 0
            before = {k: x.clone() for k, x in _post(e).items()}
            gn = _step(e, h)
            assert not bool(torch.isfinite(gn))
            _same_bits(before, _post(e), f"skipped step ({bad})")
        _inject(e, grad=g)
        e.step_count = 0
        _verify(e, _pre(e), _step(e, h), h, R.chain_full(e.n_params), "skip_tiny_after", lr_s, wd_s)
    finally:
        e.set_option(L.OPT_SKIP_NONFINITE_STEP, 0)
        e.set_param_scales(None, None)


# ------------------------------------------------------------------------------------------------ the table itself
def test_table_errors_and_read_back():
    e = _engine("tiny")
    n = len(e.params)
    with pytest.raises(KeyError):
        e.set_param_scales({"no.such.weight": 0.5}, None)
    fp = C.POINTER(C.c_float)
    ok = np.ones(n, dtype=np.float32)
    for bad in (-1.0, float("nan"), float("inf")):
        arr = ok.copy()
        arr[2] = bad
        assert e.lib.gget_set_param_scales(e.h, arr.ctypes.data_as(fp), None, n) == 2
        assert b"lr_scale[2]" in e.lib.gget_last_error()
        assert e.lib.gget_set_param_scales(e.h, None, arr.ctypes.data_as(fp), n) == 2
    assert e.lib.gget_set_param_scales(e.h, ok.ctypes.data_as(fp), None, n - 1) == 2
    assert e.lib.gget_param_scales(e.h, ok.ctypes.data_as(fp), None, n + 1) == 2
    assert set(e.param_scales()[0].values()) == {1.0}          # (a refused call changes nothing)
    e.set_param_scales({"lm_head.weight": 0.25}, None)         # a NULL array = all ones; a missing name = 1.0
    lr, wd = e.param_scales()
    assert lr["lm_head.weight"] == 0.25 and lr["model.norm.weight"] == 1.0 and set(wd.values()) == {1.0}
    e.set_param_scales(None, None)


# ------------------------------------------------------------------------------------------------ 9: model level
def test_model_level_initialize_applies_the_groups():
    """initialize(model, OptimConfig(layerwise_lr_decay=0.5, no_decay_1d=True)) on the tiny pre-train model, two batch_training steps:
    the weights bit for bit those of a second model stepped with the same scales set by hand through Engine.set_param_scales; last_lrs =
    lr_at(step) * scale; after the model re-created its engine (a larger batch) the new handle holds the table again."""
    M = importlib.import_module("graph-gpt_amd.modeling")
    T = importlib.import_module("graph-gpt_amd.training")
    synth = importlib.import_module("graph-gpt_amd.synth")
    cfg = dict(hidden_act="gelu", vocab_size=756, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
               max_position_embeddings=64, causal_attention=False, stacked_feat=13, next_n_token=13)
    batches = [{k: torch.from_numpy(v) for k, v in synth.make_pretrain_batch(B=B, S=32, F=13, V=756, seed=s).items() if k != "lengths"}
               for B, s in ((8, 3), (8, 4), (12, 5))]
    sched = dict(lr=1e-3, max_grad_norm=1.0, schedule="warmup_decay", warmup_num_steps=2, total_num_steps=10, min_lr=1e-5)
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):
        model = M.GraphGPTPretrainBase(M.GraphGPTConfig(**cfg), seed=2).cuda()
        eng = T.initialize(model, T.OptimConfig(layerwise_lr_decay=0.5, no_decay_1d=True, **sched))
        lr_s = T.layerwise_lr_scales(model, 0.5, 1)
        wd_s = {n: 0.0 if p.ndim == 1 else 1.0 for n, p in model._flat.items()}
        f32 = lambda d: {k: float(np.float32(x)) for k, x in d.items()}     # noqa: E731
        assert model._engine.param_scales() == (f32(lr_s), wd_s)
        other = M.GraphGPTPretrainBase(M.GraphGPTConfig(**cfg), seed=2).cuda()
        plain = T.initialize(other, T.OptimConfig(**sched))
        other._ensure_engine(8, 32).set_param_scales(lr_s, wd_s)
        ungrouped = M.GraphGPTPretrainBase(M.GraphGPTConfig(**cfg), seed=2).cuda()
        base = T.initialize(ungrouped, T.OptimConfig(**sched))
        for step, b in enumerate(batches[:2]):
            for en in (eng, plain, base):
                T.batch_training(b, en)
            lr = eng.optim.lr_at(step)
            assert eng.last_lr == lr and eng.last_lrs == {n: lr * s for n, s in lr_s.items()}
            assert set(base.last_lrs.values()) == {lr}
        torch.cuda.synchronize()
        e, o, u = model._engine, other._engine, ungrouped._engine
        assert o is not None and e.step_count == o.step_count == 2
        for k in e.params:
            for which in ("master", "bf16", "m", "v"):
                assert torch.equal(_bits(e.view(k, which)), _bits(o.view(k, which))), f"{k} ({which}) differs from the hand-set scales"
        assert not torch.equal(e.view("model.embed_tokens.weight"), u.view("model.embed_tokens.weight")), "the groups change nothing"
        # a larger batch: the model re-creates its engine, the step hands the table to the new handle
        T.batch_training(batches[2], eng)
        assert model._engine is not e and model._engine.param_scales() == (f32(lr_s), wd_s)
        assert eng.last_lrs["model.embed_tokens.weight"] == eng.optim.lr_at(2) * 0.5 ** 5
