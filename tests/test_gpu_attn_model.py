"""`output_attentions=True` through the model classes (graph-gpt_amd/modeling.py -> Engine.attention_probs -> gget_attention_probs):
the tiny pre-train and fine-tune models at B = 3 and S = 24, 48, 96, 256 - one forward kernel family each (the per-sample S <= 32
kernel; the 33 .. 64-row kernels; the generic tiled forward; the long-sequence forward), lengths 1 and S among them - on both token
layouts (GGET_VARLEN=0, and the default with a token count), a packed batch and a causal configuration.  Every layer's tensor is
checked per element against the float64 statement of tests/_attn_ref.py fed with that forward's own rotated q | k
(Engine.layer_qkv), with lse formed exactly there and its fp32 term in the bound; against the reference's own tensors
(tests/golden/attn_tiny_*.npz, tools/make_golden_attn.py); and in training mode against the dropout twin."""
import importlib
import os

import numpy as np
import pytest
import torch

import _attn_ref as R
import _heads_ref as H
from _util import GOLDEN, record_error, rel_l2, spec_mod, synth, weights_mod

pytestmark = pytest.mark.gpu

M = importlib.import_module("graph-gpt_amd.modeling")
L = importlib.import_module("graph-gpt_amd._lib")
E = importlib.import_module("graph-gpt_amd.engine")

V, F_PT, F_FT = 756, 13, 4
SIZES = [24, 48, 96, 256]


def config(spec, **kw):
    return M.GraphGPTConfig(hidden_act="gelu", vocab_size=spec.vocab_size, hidden_size=spec.hidden_size,
                            intermediate_size=spec.intermediate_size, num_hidden_layers=spec.num_layers,
                            num_attention_heads=spec.num_heads, max_position_embeddings=spec.max_position,
                            causal_attention=spec.causal, stacked_feat=spec.stacked_feat, rms_norm_eps=spec.rms_eps,
                            pad_token_id=spec.pad_token_id, **kw)


def pt_model(causal=False, attention_dropout=0.0, state=None):
    spec = spec_mod.spec_from_size("tiny", vocab_size=V, stacked_feat=F_PT, next_n_token=F_PT, causal=causal)
    model = M.GraphGPTPretrainBase(config(spec, next_n_token=F_PT, attention_dropout=attention_dropout), seed=3)
    if state is not None:
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return model.cuda()


def ft_model(state=None):
    spec = spec_mod.spec_from_size("tiny", kind=spec_mod.KIND_TASK, vocab_size=V, stacked_feat=F_FT, next_n_token=1, num_labels=2)
    model = M.GraphGPTTaskModel(config(spec, num_labels=2, problem_type="single_label_classification"), seed=4)
    if state is not None:
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return model.cuda()


def lengths(S):
    return (S, S // 2 + 1, 1)


def cut(batch, lens):
    """A full-row batch right-padded to `lens`."""
    for b, n in enumerate(lens):
        batch["input_ids"][b, n:] = 0
        batch["attention_mask"][b, n:] = 0
        batch["position_ids"][b, n:] = 0
        if "labels" in batch:
            batch["labels"][b, n:] = -100
    batch.pop("lengths", None)
    return {k: torch.from_numpy(v) for k, v in batch.items()}


def pt_batch(S):
    return cut(synth.make_pretrain_batch(B=3, S=S, F=F_PT, V=V, seed=900 + S, lengths="full"), lengths(S))


def ft_batch(S):
    return cut(synth.make_task_batch(B=3, S=S, F=F_FT, V=V, seed=950 + S, lengths="full", num_labels=2), lengths(S))


def set_layout(monkeypatch, layout):
    if layout == "padded":
        monkeypatch.setenv("GGET_VARLEN", "0")
    else:
        monkeypatch.delenv("GGET_VARLEN", raising=False)


def run(model, b, layout, **kw):
    """One forward; on the var-len layout the token count goes in as the collator would hand it over."""
    n = int(b["attention_mask"].sum()) if (layout == "varlen" and b["attention_mask"].dim() == 2) else None
    args = {k: v for k, v in b.items() if k in ("input_ids", "attention_mask", "position_ids", "labels", "task_labels")}
    with torch.no_grad():
        out = model(num_tokens=n, **args, **kw)
    assert model._engine.varlen_status()[0] == (n is not None), "the forward did not run on the requested token layout"
    return out


def finish(case, results):
    ratio, msgs = H.settle(results)
    record_error("attn_model_elementwise", case, ratio, 1.0)
    print(f"attn_model_elementwise {case}: max err / bound = {ratio:.4f}")
    assert not msgs, f"{case}:\n" + "\n".join(msgs)


def allowed_of(b, causal):
    m = b["attention_mask"]
    if m.dim() == 3:
        return m.bool()
    return R.allowed_padded(m.shape[0], m.shape[1], m.sum(1).tolist(), causal)


def check_layers(case, model, b, att, keep_of=None, p_drop=0.0):
    """Shape and dtype of the tuple; every layer per element against float64 from the forward's own q | k; the zero structure; in eval
    the rows of real queries sum to 1 within 2^-8 (every term carries one rounding of at most 2^-9 relative to its binade, the fp32
    terms of the bound are far below)."""
    spec, e = model.spec, model._engine
    B, S = b["input_ids"].shape[:2]
    ok = allowed_of(b, bool(spec.causal))
    assert isinstance(att, tuple) and len(att) == spec.num_layers
    for i, a in enumerate(att):
        assert tuple(a.shape) == (B, spec.num_heads, S, S) and a.dtype == torch.bfloat16 and a.device == model.device
        qkv = e.layer_qkv(i, B, S).cpu()
        dead = ~ok.any(-1)
        assert bool((qkv[dead] == 0).all()), "layer_qkv: rows behind a sample's tokens are not zero"
        q, k = R.split_qk(qkv, B, S, spec.num_heads)
        keep = keep_of(i) if keep_of is not None else None
        got = a.cpu()
        finish(f"{case} layer {i}", R.attn_check(got, q, k, ok, keep=keep, p_drop=p_drop))
        if keep is None:
            sums = got.double().sum(-1)                                     # [B,H,S]
            live = ok.any(-1)[:, None].expand_as(sums)
            assert float((sums[live] - 1.0).abs().max()) <= 2.0 ** -8, float((sums[live] - 1.0).abs().max())
            assert bool((sums[~live] == 0).all())


@pytest.mark.parametrize("layout", ["padded", "varlen"])
@pytest.mark.parametrize("S", SIZES)
def test_pretrain_attentions(monkeypatch, S, layout):
    set_layout(monkeypatch, layout)
    model = pt_model().eval()
    b = pt_batch(S)
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):       # (the loss sum and two gradient reductions use fp32 atomics otherwise)
        plain = run(model, b, layout)
        loss0, logits0 = plain.head1_loss.clone(), plain.head1_logits.clone()      # (views of the engine's buffers: the next forward rewrites them)
        out = run(model, b, layout, output_attentions=True)
        assert plain.attentions is None and plain.hidden_states is None and out.hidden_states is None
        assert torch.equal(loss0, out.head1_loss) and torch.equal(logits0, out.head1_logits)
        check_layers(f"pretrain-S{S}-{layout}", model, b, out.attentions)
        # one training step's gradients after a forward with the flag are those after a plain forward
        grads = []
        for flag in (False, True):
            n = int(b["attention_mask"].sum()) if layout == "varlen" else None
            o = model(input_ids=b["input_ids"], attention_mask=b["attention_mask"], position_ids=b["position_ids"], labels=b["labels"],
                      num_tokens=n, output_attentions=flag)
            assert (o.attentions is not None) == flag
            o.head1_loss.backward()
            torch.cuda.synchronize()
            grads.append(model._engine.grad_bf16.clone())
        assert torch.equal(grads[0].view(torch.int16), grads[1].view(torch.int16)), "gradients differ after an output_attentions forward"


@pytest.mark.parametrize("layout", ["padded", "varlen"])
@pytest.mark.parametrize("S", SIZES)
def test_finetune_attentions(monkeypatch, S, layout):
    set_layout(monkeypatch, layout)
    model = ft_model().eval()
    b = ft_batch(S)
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):
        plain = run(model, b, layout)
        loss0, logits0 = plain.task_loss.clone(), plain.task_logits.clone()
        out = run(model, b, layout, output_attentions=True)
        assert plain.attentions is None
        assert torch.equal(loss0, out.task_loss) and torch.equal(logits0, out.task_logits)
        check_layers(f"finetune-S{S}-{layout}", model, b, out.attentions)


def test_config_flag_is_the_default_of_the_call_flag(monkeypatch):
    """hf rule: the call's flag, else config.output_attentions."""
    set_layout(monkeypatch, "padded")
    model = pt_model().eval()
    b = pt_batch(24)
    model.config.output_attentions = True
    assert run(model, b, "padded").attentions is not None
    assert run(model, b, "padded", output_attentions=False).attentions is None
    model.config.output_attentions = False
    assert run(model, b, "padded").attentions is None


def test_packed_batch_attentions(monkeypatch):
    set_layout(monkeypatch, "varlen")
    model = pt_model().eval()
    raw = synth.make_packed_pretrain_batch(B=3, S=64, F=F_PT, V=V, seed=77)
    assert raw["attention_mask"].shape == (3, 64, 64) and int((raw["attention_mask"].sum(-1) == 0).sum()) > 0     # some padding rows
    raw.pop("segments")
    raw.pop("lengths")
    b = {k: torch.from_numpy(v) for k, v in raw.items()}
    loss0 = run(model, b, "padded").head1_loss.clone()
    out = run(model, b, "padded", output_attentions=True)
    assert torch.equal(loss0, out.head1_loss)
    check_layers("pretrain-packed-S64", model, b, out.attentions)


@pytest.mark.parametrize("layout", ["padded", "varlen"])
def test_causal_attentions(monkeypatch, layout):
    set_layout(monkeypatch, layout)
    model = pt_model(causal=True).eval()
    b = pt_batch(48)
    out = run(model, b, layout, output_attentions=True)
    a = out.attentions[0].cpu()
    assert bool((a[:, :, 0, 0] == 1).all()) and bool((torch.triu(a.float(), 1) == 0).all())
    check_layers(f"pretrain-causal-S48-{layout}", model, b, out.attentions)


def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = [int(x) for x in z["meta_spec"]]
    kw = dict(vocab_size=m[1], stacked_feat=m[6], next_n_token=m[7])
    if m[0] == spec_mod.KIND_TASK:
        kw.update(kind=spec_mod.KIND_TASK, num_labels=m[11])
    spec = spec_mod.spec_from_size("tiny", **kw)
    seed, std, hstd = z["meta_init"]
    state = weights_mod.make_state_dict(spec, seed=int(seed), std=float(std), head_std=float(hstd))
    b = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    return z, state, b


@pytest.mark.parametrize("name", ["attn_tiny_pt", "attn_tiny_ft"])
def test_attentions_match_the_reference_fixture(monkeypatch, name):
    """The reference's own `outputs.attentions` (fp32, eager): rel_l2 over the real (q, k) entries of every layer < 2e-2, the bf16-class
    tolerance tests/test_gpu_metrics.py holds hidden_states to against the fp32 oracle (a quantity of the same chain); both token
    layouts give the same bits."""
    z, state, b = fixture(name)
    lens = b.pop("lengths").tolist()
    model = (pt_model(state=state) if name.endswith("_pt") else ft_model(state=state)).eval()
    got = {}
    for layout in ("padded", "varlen"):
        set_layout(monkeypatch, layout)
        got[layout] = [a.cpu() for a in run(model, b, layout, output_attentions=True).attentions]
    for i, (a, c) in enumerate(zip(got["padded"], got["varlen"])):
        assert torch.equal(a.view(torch.int16), c.view(torch.int16)), f"layer {i}: the token layouts differ"
        for bb, n in enumerate(lens):
            err = rel_l2(a[bb, :, :n, :n].float().numpy(), z["attentions"][i, bb, :, :n, :n])
            record_error(f"attn_fixture/{name}", f"layer {i} sample {bb}", err, 2e-2)
            assert err < 2e-2, (i, bb, err)
            assert bool((a[bb, :, :, n:] == 0).all()) and bool((a[bb, :, n:] == 0).all())


@pytest.mark.parametrize("layout", ["padded", "varlen"])
def test_training_mode_applies_the_forwards_dropout_mask(monkeypatch, layout):
    """train() with attention_dropout = 0.1: the zero pattern inside the allowed keys is the twin's with the per-layer seed, the kept
    elements are the weights over 1 - p under the bound; eval() on the same model returns the weights without a mask."""
    set_layout(monkeypatch, layout)
    p = 0.1
    model = pt_model(attention_dropout=p).train()
    b = pt_batch(48)
    out = run(model, b, layout, output_attentions=True)
    seed = model.last_dropout_seed
    B, S, Hn = 3, 48, model.spec.num_heads
    check_layers(f"pretrain-train-S48-{layout}", model, b, out.attentions,
                 keep_of=lambda i: R.attn_drop_keep(R.layer_seed(seed, i), B, Hn, S, p), p_drop=p)
    a0 = out.attentions[0].cpu()
    ok = allowed_of(b, False)[:, None].expand_as(a0)
    rate = float((a0[ok] == 0).double().mean())
    assert 0.05 < rate < 0.15, rate
    model.eval()
    check_layers(f"pretrain-train-then-eval-S48-{layout}", model, b, run(model, b, layout, output_attentions=True).attentions)


def test_refusals():
    """Before any forward, and for a layer out of range: the error code and its text, no fault."""
    spec = spec_mod.spec_from_size("tiny", vocab_size=V, stacked_feat=F_PT, next_n_token=F_PT)
    e = E.Engine(spec, max_tokens=3 * 24, max_batch=3)
    with pytest.raises(L.GgetError, match="no valid forward"):
        e.attention_probs(0, 3, 24)
    with pytest.raises(L.GgetError, match="no valid forward"):
        e.layer_qkv(0, 3, 24)
    b = pt_batch(24)
    e.forward_pretrain(b["input_ids"], b["attention_mask"], b["labels"], None, b["position_ids"])
    assert tuple(e.attention_probs(1, 3, 24).shape) == (3, 2, 24, 24)
    for layer in (-1, 2, 99):
        with pytest.raises(L.GgetError, match="out of range"):
            e.attention_probs(layer, 3, 24)
        with pytest.raises(L.GgetError, match="out of range"):
            e.layer_qkv(layer, 3, 24)
