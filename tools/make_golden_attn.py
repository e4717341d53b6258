#!/usr/bin/env python
"""Generate tests/golden/attn_tiny_pt.npz and attn_tiny_ft.npz: `outputs.attentions` of the REAL reference
(modeling_pretrain.py:265, modeling_finetune.py:325; the softmax weights of hf eager_attention_forward, modeling_llama.py:191-214)
for the tiny pre-train model (d128 / L2 / H2 / F13 / V756, bi-directional) and the tiny fine-tune model (F4, 2 classes), fp32, eval(),
config._attn_implementation = "eager", output_attentions=True, on a batch B = 3, S = 40 with lengths 40 / 23 / 1.

Runs on the build machine only (the reference is imported by the recipe of SURVEY.md Appendix A, tools/make_golden.py
import_reference).  The fixtures hold data only: the inputs, the seed of the weight generator and the attention tensors."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

B, S, LENS = 3, 40, (40, 23, 1)


def cut(batch):
    """Right-pad the full-row batch to LENS: pad ids, no labels, mask and positions zero behind a sample's tokens."""
    for b, n in enumerate(LENS):
        batch["input_ids"][b, n:] = 0
        batch["attention_mask"][b, n:] = 0
        batch["position_ids"][b, n:] = 0
        if "labels" in batch:
            batch["labels"][b, n:] = -100
    batch["lengths"] = np.array(LENS, np.int64)
    return batch


def attentions_of(model, call):
    """outputs.attentions when the installed transformers routes them through, else the second output of every self_attn module
    (the eager forward returns (attn_output, attn_weights)) taken by forward hooks."""
    got = []
    hooks = [layer.self_attn.register_forward_hook(lambda m, a, o: got.append(o[1])) for layer in model.model.layers]
    try:
        with torch.no_grad():
            out = call()
    finally:
        for h in hooks:
            h.remove()
    att = getattr(out, "attentions", None)
    if att is None or any(a is None for a in att):
        att = got
    assert len(att) == len(model.model.layers) and all(a is not None for a in att), "the reference returned no attention weights"
    return [a.detach().float().numpy() for a in att]


def check(att, name):
    """What the tests rely on: exact zeros at padded keys, rows that sum to 1 (every row, padding queries included)."""
    for i, a in enumerate(att):
        assert a.shape == (B, a.shape[1], S, S), a.shape
        for b, n in enumerate(LENS):
            assert np.all(a[b, :, :, n:] == 0.0), f"{name} layer {i} sample {b}: a padded key has weight"
            assert np.all(a[b, :, :, :n] > 0.0)
        assert np.abs(a.sum(-1) - 1.0).max() < 1e-5, f"{name} layer {i}: rows do not sum to 1"


def run(name, kind, spec_kw, batch, seed, make_model):
    spec = MG.spec_mod.spec_from_size("tiny", kind=kind, **spec_kw)
    assert (spec.hidden_size, spec.num_layers, spec.num_heads, bool(spec.causal)) == (128, 2, 2, False)
    state = MG.weights_mod.make_state_dict(spec, seed=seed, std=0.06, head_std=0.3)
    model = make_model(spec)
    model.config._attn_implementation = "eager"
    if hasattr(model, "model") and hasattr(model.model, "config"):
        model.model.config._attn_implementation = "eager"
    MG.load_weights(model, state)
    model.eval()
    tb = {k: torch.from_numpy(v) for k, v in batch.items()}
    kw = dict(input_ids=tb["input_ids"], attention_mask=tb["attention_mask"], position_ids=tb["position_ids"], output_attentions=True)
    if "labels" in tb:
        kw["labels"] = tb["labels"]
    att = attentions_of(model, lambda: model(**kw))
    check(att, name)
    res = {"meta_spec": np.array(spec.as_c_ints(), np.int64), "meta_init": np.array([seed, 0.06, 0.3]),
           "attentions": np.stack(att).astype(np.float32)}
    for k, v in batch.items():
        res["in_" + k] = v
    path = os.path.join(MG.ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **res)
    print(f"{name} written: attentions {res['attentions'].shape}, {os.path.getsize(path)} bytes")


def main():
    PT, FT, Cfg = MG.import_reference()
    pt = cut(MG.synth.make_pretrain_batch(B=B, S=S, F=13, V=756, seed=171, lengths="full"))
    run("attn_tiny_pt", MG.spec_mod.KIND_PRETRAIN, dict(vocab_size=756, stacked_feat=13, next_n_token=13), pt, 1711,
        lambda spec: PT(MG.ref_config(Cfg, spec)))
    ft = cut(MG.synth.make_task_batch(B=B, S=S, F=4, V=756, seed=172, lengths="full", num_labels=2))
    ft.pop("task_labels")
    run("attn_tiny_ft", MG.spec_mod.KIND_TASK, dict(vocab_size=756, stacked_feat=4, next_n_token=1, num_labels=2), ft, 1712,
        lambda spec: FT(MG.ref_config(Cfg, spec, num_labels=2, problem_type="single_label_classification")))


if __name__ == "__main__":
    main()
