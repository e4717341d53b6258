#!/usr/bin/env python
"""Generate the fixtures of the two model sizes with 32-wide attention heads (spec.MODEL_SIZES "tiny6": d128 / L6 / H4 / ff512, and
"small12": d384 / L12 / H12 / ff384; hf head_dim = hidden_size // num_attention_heads = 32) from the REAL reference, through the recipe of
tools/make_golden.py (import_reference / ref_config / run_case) and tools/make_golden_attn.py (the reference's own `outputs.attentions`).

    pt_tiny6_f13, pt_tiny6_s72, pt_tiny6_causal, pt_tiny6_packed, ft_tiny6_f4_b32   run_case at size "tiny6" (full gradients)
    pt_small12_f13                                                                   run_case at size "small12" (the "big" storage form:
                                                                                     gradient norms and 64 x 64 corner blocks)
    attn_tiny6_padded   tiny6 pre-train model, B 3 / S 40, lengths 40 / 23 / 1: attentions [L, B, H, S, S] fp32, eager
    attn_tiny6_packed   the same model on packed rows (B 2 / S 72, block-diagonal [B, S, S] mask)

Conditioning of the pre-train fixtures.  The engine computes with bf16 copies of the weights, so it cannot lie closer to the reference's
fp32 loss than the loss of the bf16-ROUNDED weights in exact arithmetic does - a property of the fixture alone, evaluated here with the
CPU oracle in fp32.  The parity test's tolerance (tests/_util.py:loss_tolerance: 1e-4, or 1.5 x the reference's own bf16-vs-fp32 gap) is
taken from the same fixture; a fixture whose weight-rounding shift alone uses more than half of it says nothing about the arithmetic
under test.  weight_rounding_shift() measures it; a case with several seeds takes the FIRST whose fixture is conditioned and prints the
rejected ones (the practice of make_golden.run_case's L1-regression margin: "pick another seed").  Seed 41 of pt_tiny6_s72: shift
3.71e-4 against a tolerance of 3.44e-4.

Runs on the build machine only.  The fixtures hold data only: inputs, the seed of the weight generator, the reference's outputs."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402
import make_golden_attn as MGA  # noqa: E402

PT13 = dict(vocab_size=756, stacked_feat=13, next_n_token=13)
BIGW = dict(std=0.06, head_std=0.15)
CASES = [
    ("pt_tiny6_f13", "pt", PT13, dict(B=4, S=24, seed=40), dict(size="tiny6")),
    ("pt_tiny6_s72", "pt", PT13, dict(B=3, S=72, seed=(41, 46, 47, 48, 49), lengths="uniform", min_len=20), dict(size="tiny6", **BIGW)),
    ("pt_tiny6_causal", "pt", dict(causal=True, **PT13), dict(B=4, S=24, seed=42), dict(size="tiny6")),
    ("pt_tiny6_packed", "pt", PT13, dict(B=3, S=72, seed=43, packed=True), dict(size="tiny6", **BIGW)),
    ("ft_tiny6_f4_b32", "ft", dict(vocab_size=1000, stacked_feat=4, next_n_token=1, num_labels=2), dict(B=32, S=24, seed=44),
     dict(size="tiny6", **BIGW)),
    ("pt_small12_f13", "pt", PT13, dict(B=4, S=32, seed=45), dict(size="small12")),
]


def attn_fixture(name, batch, seed, classes, packed):
    PT, _, Cfg = classes
    spec = MG.spec_mod.spec_from_size("tiny6", kind=MG.spec_mod.KIND_PRETRAIN, **PT13)
    assert (spec.hidden_size, spec.num_layers, spec.num_heads, spec.head_dim) == (128, 6, 4, 32)
    state = MG.weights_mod.make_state_dict(spec, seed=seed, std=0.06, head_std=0.3)
    model = PT(MG.ref_config(Cfg, spec))
    model.config._attn_implementation = "eager"
    if hasattr(model, "model") and hasattr(model.model, "config"):
        model.model.config._attn_implementation = "eager"
    assert model.model.layers[0].self_attn.head_dim == 32
    MG.load_weights(model, state)
    model.eval()
    tb = {k: torch.from_numpy(v) for k, v in batch.items()}
    kw = dict(input_ids=tb["input_ids"], attention_mask=tb["attention_mask"], output_attentions=True, labels=tb["labels"])
    if not packed:
        kw["position_ids"] = tb["position_ids"]
    att = MGA.attentions_of(model, lambda: model(**kw))
    if packed:
        m = batch["attention_mask"].astype(bool)                       # [B,S,S]
        live = m.any(-1)
        for i, a in enumerate(att):
            assert np.all(a[np.broadcast_to(~m[:, None], a.shape) & np.broadcast_to(live[:, None, :, None], a.shape)] == 0.0), (name, i)
            assert np.abs(a.sum(-1)[np.broadcast_to(live[:, None], a.shape[:3])] - 1.0).max() < 1e-5
    else:
        MGA.check(att, name)
    res = {"meta_spec": np.array(spec.as_c_ints(), np.int64), "meta_init": np.array([seed, 0.06, 0.3]),
           "attentions": np.stack(att).astype(np.float32)}
    for k, v in batch.items():
        res["in_" + k] = v
    path = os.path.join(MG.ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **res)
    print(f"{name} written: attentions {res['attentions'].shape}, {os.path.getsize(path)} bytes")


def weight_rounding_shift(name):
    """(relative shift of the fp32-arithmetic loss when the weights are rounded to bf16, the parity test's loss tolerance) of a written
    pre-train fixture - oracle and fixture only."""
    sys.path.insert(0, os.path.join(MG.ROOT, "tests"))
    sys.path.insert(0, MG.ROOT)
    from _hd32_util import load_case32
    from _util import loss_tolerance, tb
    from oracle import gget_oracle as O
    z, spec, state, batch = load_case32(name)
    b = tb(batch)
    st = {k: torch.from_numpy(v).to(torch.bfloat16).float().numpy() for k, v in state.items()}
    with torch.no_grad():
        loss = O.pretrain_forward(spec, O.to_params(st, torch.float32, requires_grad=False), b["input_ids"], b["attention_mask"], b["labels"],
                                  b.get("wgt"))["head1_loss"].item()
    return abs(loss - float(z["loss"])) / abs(float(z["loss"])), loss_tolerance(z, factor=1.5)


def main():
    only = set(sys.argv[1:])
    classes = MG.import_reference()
    for name, kind, skw, bkw, ikw in CASES:
        if only and name not in only:
            continue
        seeds = bkw["seed"] if isinstance(bkw["seed"], tuple) else (bkw["seed"],)
        for seed in seeds:
            MG.run_case(name, kind, dict(skw), dict(bkw, seed=seed), dict(ikw), classes)
            print(f"  {os.path.getsize(os.path.join(MG.ROOT, 'tests', 'golden', name + '.npz'))} bytes")
            if kind != "pt":
                break
            shift, tol = weight_rounding_shift(name)
            print(f"  {name} seed {seed}: bf16 weight rounding alone moves the loss by {shift:.3e}, loss tolerance {tol:.3e}")
            if shift <= 0.5 * tol:
                break
            print(f"  {name} seed {seed} REJECTED: the weight rounding alone uses more than half of the tolerance")
        else:
            raise SystemExit(f"{name}: no conditioned seed among {seeds}")
    if only and not only & {"attn_tiny6_padded", "attn_tiny6_packed"}:
        return
    padded = MGA.cut(MG.synth.make_pretrain_batch(B=MGA.B, S=MGA.S, F=13, V=756, seed=173, lengths="full"))
    attn_fixture("attn_tiny6_padded", padded, 1713, classes, packed=False)
    packed = MG.synth.make_packed_pretrain_batch(B=2, S=72, F=13, V=756, seed=174)
    attn_fixture("attn_tiny6_packed", packed, 1714, classes, packed=True)


if __name__ == "__main__":
    main()
