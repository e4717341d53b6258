"""config.loss_type = "token_ce_intra" through the drop-in class (GraphGPTTaskModel; modeling_finetune.py:140-165, :198-202) on both
token layouts: loss, logits and gradients against the reference fixture (tests/golden/ft_tiny_tokence_intra.npz, tools/make_golden.py),
the head in isolation against the float64 statement of tests/_intra_ref.py applied to the engine's own final hidden states, the error
paths of `cls_idx`, and one optimizer step under finetune.freeze."""
import importlib
import os

import numpy as np
import pytest
import torch

import _heads_ref as H
import _intra_ref as R
from _util import GOLDEN, record_error, spec_mod, weights_mod

pytestmark = pytest.mark.gpu

M = importlib.import_module("graph-gpt_amd.modeling")
T = importlib.import_module("graph-gpt_amd.training")

C_ = 5
TAG = "ft_tiny_tokence_intra"


def _fixture():
    z = np.load(os.path.join(GOLDEN, TAG + ".npz"))
    spec = spec_mod.spec_from_size("tiny", kind=spec_mod.KIND_TASK, vocab_size=756, stacked_feat=13, next_n_token=1, num_labels=C_)
    seed, std, hstd = z["meta_init"]
    state = weights_mod.make_state_dict(spec, seed=int(seed), std=float(std), head_std=float(hstd))
    b = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    return z, spec, state, b


def _model(spec, state, layout="auto", load=True, **extra):
    cfg = M.GraphGPTConfig(hidden_act="gelu", vocab_size=756, hidden_size=spec.hidden_size, intermediate_size=spec.intermediate_size,
                           num_hidden_layers=spec.num_layers, num_attention_heads=spec.num_heads,
                           max_position_embeddings=spec.max_position, causal_attention=False, stacked_feat=13, next_n_token=1,
                           num_labels=C_, loss_type="token_ce_intra", problem_type="single_label_classification", **extra)
    model = M.GraphGPTTaskModel(cfg, seed=1)
    if load:
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model.token_layout = layout
    return model.eval()


def _call(model, b, labels=True, **over):
    kw = dict(input_ids=b["input_ids"], attention_mask=b["attention_mask"], position_ids=b["position_ids"], cls_idx=b["cls_idx"])
    if labels:
        kw["task_labels"] = b["task_labels"]
    kw.update(over)
    return model(**kw)


@pytest.mark.parametrize("layout", ["padded", "varlen"])
def test_intra_head_matches_reference_fixture(layout):
    """Tolerances against the fp32 fixture are those of the token_ce test in tests/test_gpu_model.py: loss 5e-3 relative, logits 3e-2 of
    the largest logit on the real rows, gradients 6e-2 (there a relative L2 distance to the oracle's gradient; here the fixture stores
    norms, so the norm of every parameter's gradient within 6e-2 of max(its norm, 1e-2 of the largest), and the relative L2 distance
    of the one stored gradient, layers.1.mlp.down_proj).  The head in isolation is held to the element-wise bound of _intra_ref: the
    engine's logits against the float64 head applied to the engine's own bf16 final hidden states."""
    z, spec, state, b = _fixture()
    model = _model(spec, state, layout)
    out = _call(model, b)
    e = model._engine
    assert e.varlen_status()[0] == (layout == "varlen")
    loss, ref = float(out.task_loss.item()), float(z["loss"])
    out.task_loss.backward()
    lg = out.task_logits.float().cpu()
    assert tuple(lg.shape) == tuple(z["logits"].shape) == (10, 24, C_)
    real = b["attention_mask"].bool()
    # the head alone: the engine's own hidden states through the float64 statement
    hid = e.hidden_states(10, 24).cpu()
    i = dict(hidden=hid.reshape(240, -1), row_start=(torch.arange(11) * 24).to(torch.int32), cls_idx=b["cls_idx"], C=C_, B=10,
             d=hid.shape[-1], inside=real.reshape(-1))
    ratio, msgs = H.settle(R.intra_fwd_check(i, lg.reshape(240, C_)))
    record_error(TAG + "_" + layout, "head_logits_err_over_bound_vs_float64_on_engine_hidden", ratio, 1.0)
    print(f"[intra {layout}] head logits against float64 on the engine's hidden states: max err / bound = {ratio:.4f}")
    assert not msgs, "\n".join(msgs)
    if layout == "varlen":
        assert bool((lg[~real] == 0).all())
    # the loss the float64 head gives on the engine's hidden states: how much of the distance to the fixture the backbone accounts for
    loss_h = float(R.token_ce(R.intra_logits_grid(torch.where(real[:, :, None], hid.double(), torch.ones(1, dtype=torch.float64)),
                                                  b["cls_idx"], C_), b["task_labels"]))
    lerr = abs(loss - ref) / ref
    gerr = float(np.abs(lg.numpy() - z["logits"])[real.numpy()].max()) / float(np.abs(z["logits"][real.numpy()]).max())
    print(f"[intra {layout}] loss {loss:.6f} fixture {ref:.6f} rel {lerr:.3e} (float64 head on engine hidden: {loss_h:.6f}, rel "
          f"{abs(loss_h - ref) / ref:.3e}); logits max err / max |logit| {gerr:.3e}")
    record_error(TAG + "_" + layout, "loss_rel_vs_reference_fp32", lerr, 5e-3)
    record_error(TAG + "_" + layout, "logits_max_rel_vs_reference_fp32 (real rows)", gerr, 3e-2)
    # gradients
    got = e.grads()
    names = [str(n) for n in z["names"]]
    want = dict(zip(names, [float(x) for x in z["grad_norms"]]))
    gmax = max(want.values())
    worst = ("", 0.0)
    for k in names:
        gn = float(got[k].float().norm())
        r = abs(gn - want[k]) / max(want[k], 1e-2 * gmax)
        worst = max(worst, (k, r), key=lambda t: t[1])
    w = z["grad_l1_down"]
    derr = float(np.linalg.norm(got["model.layers.1.mlp.down_proj.weight"].float().cpu().numpy() - w)) / float(np.linalg.norm(w))
    print(f"[intra {layout}] gradient norms: worst {worst[0]} {worst[1]:.3e}; layers.1.mlp.down_proj rel L2 {derr:.3e}")
    record_error(TAG + "_" + layout, "grad_norm_rel_worst", worst[1], 6e-2)
    record_error(TAG + "_" + layout, "grad_rel_l2 model.layers.1.mlp.down_proj.weight", derr, 6e-2)
    assert lerr <= 5e-3, (loss, ref)
    assert gerr < 3e-2, gerr
    assert worst[1] < 6e-2, worst
    assert derr < 6e-2, derr
    assert want["score.weight"] == 0.0 and float(got["score.weight"].abs().max()) == 0.0      # `score` is outside the graph
    # evaluation without labels returns the same all-row logits
    with torch.no_grad():
        ev = _call(model, b, labels=False)
    assert ev.task_loss is None and torch.equal(ev.task_logits, out.task_logits)
    model.check_deferred()


def test_both_layouts_agree():
    z, spec, state, b = _fixture()
    res = {}
    for layout in ("padded", "varlen"):
        model = _model(spec, state, layout)
        out = _call(model, b)
        out.task_loss.backward()
        torch.cuda.synchronize()
        res[layout] = (float(out.task_loss.item()), out.task_logits.float().cpu(), {k: v.float().cpu().numpy().copy() for k, v in model._engine.grads().items()})
    (lp, zp, gp), (lv, zv, gv) = res["padded"], res["varlen"]
    real = b["attention_mask"].bool()
    assert abs(lv - lp) <= 2e-5 * abs(lp), (lv, lp)
    assert float((zv[real] - zp[real]).abs().max()) <= 2e-3 * max(1.0, float(zp[real].abs().max()))
    gmax = max(float(np.linalg.norm(x)) for x in gp.values())
    for k in gp:
        assert float(np.linalg.norm(gv[k] - gp[k])) / max(float(np.linalg.norm(gp[k])), 1e-2 * gmax) < 1e-2, k


def test_cls_idx_error_paths():
    z, spec, state, b = _fixture()
    model = _model(spec, state)
    with pytest.raises(ValueError, match="cls_idx"):
        _call(model, b, cls_idx=None)
    lens = b["attention_mask"].sum(1)
    for bad in (lens - C_ + 1, torch.where(torch.arange(10) == 4, -1, b["cls_idx"])):       # past the real rows; negative
        with pytest.raises(IndexError, match="cls_idx"):
            _call(model, b, cls_idx=bad)
    # device tensors are not read back: the engine clamps them, the step runs, check_deferred() reports once
    dev = {k: v.cuda() for k, v in b.items()}
    out = _call(model, dev)
    model.check_deferred()
    good = out.task_logits.clone()
    out = _call(model, dev, cls_idx=(lens - C_ + 1).cuda())
    assert bool(torch.isfinite(out.task_logits).all())
    with pytest.raises(IndexError, match="cls_idx"):
        model.check_deferred()
    model.check_deferred()                       # the flag is cleared
    out = _call(model, dev)
    assert torch.equal(out.task_logits, good)    # the clamped copy did not outlive its call
    model.check_deferred()
    with pytest.raises(NotImplementedError, match="MLP"):
        _call(_model(spec, state, load=False, mlp=[32]), b)


def test_one_step_under_freeze_changes_the_trainable_ranges_only():
    """finetune.freeze = 1 (embed_tokens and layer 0 frozen): the truncated backward and the step over the trainable ranges see nothing
    new in the intra head - the frozen ranges of the master weights keep their bits, trainable ones move, `score` (zero gradient, so only
    the decoupled weight decay acts on it) included."""
    z, spec, state, b = _fixture()
    model = _model(spec, state).cuda()
    model.freeze_layers(1)
    eng = T.initialize(model, T.OptimConfig(lr=1e-3, max_grad_norm=1.0))
    out = eng(input_ids=b["input_ids"], attention_mask=b["attention_mask"], position_ids=b["position_ids"], task_labels=b["task_labels"],
              cls_idx=b["cls_idx"])
    e = model._engine
    e.await_params()
    torch.cuda.synchronize()
    pre = e.master.clone()
    eng.backward(out.task_loss)
    gn = float(eng.step())
    e.await_params()
    torch.cuda.synchronize()
    assert np.isfinite(gn) and gn > 0
    tm = torch.zeros(e.n_params, dtype=torch.bool, device="cuda")
    for off, cnt in e.train_ranges:
        tm[off: off + cnt] = True
    frozen = model.frozen_names()
    assert "model.embed_tokens.weight" in frozen and any(n.startswith("model.layers.0.") for n in frozen)
    for n in frozen:
        p = e.params[n]
        assert not bool(tm[p["offset"]: p["offset"] + p["numel"]].any())
    post = e.master
    assert torch.equal(post[~tm].view(torch.int32), pre[~tm].view(torch.int32)), "a frozen range changed"
    p = e.params["model.layers.1.mlp.down_proj.weight"]
    assert bool((post[p["offset"]: p["offset"] + p["numel"]] != pre[p["offset"]: p["offset"] + p["numel"]]).any())
    model.check_deferred()
