#!/usr/bin/env python3
"""Generate tests/golden/layerwise_lr.json: the learning rate the reference's layer-wise parameter groups give every parameter -
get_layerwise_param_groups (v1) and get_layerwise_param_groups_v3 of src/utils/loss_utils.py:370-412, run on three reference models:

    pt_tiny      tiny pre-train model, F = 13, stack_method "short"
    ft_linear    tiny task model with a Linear `score`
    ft_mlp_ls    tiny task model with an MLP `score` (48, 32, biased), LayerScale and embed_dim = 64

as {case: {version: {state-dict name: lr}}} with BASE_LR and the functions' own default decays (v1 0.95, v3 0.5).  A parameter
the reference's groups leave out has no entry.  Data only; the import recipe and the helpers are those of tools/make_golden.py.
tests/test_layerwise_lr.py builds the same three models of this project (CASES there mirrors CASES here).

    python tools/make_golden_llrd.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

BASE_LR = 3e-4
S = MG.spec_mod
CASES = {
    "pt_tiny": ("pt", dict(kind=S.KIND_PRETRAIN, vocab_size=756, stacked_feat=13, next_n_token=13), dict(stack_method="short")),
    "ft_linear": ("ft", dict(kind=S.KIND_TASK, vocab_size=1000, stacked_feat=4, next_n_token=1, num_labels=2),
                  dict(num_labels=2, loss_type=None, mlp=[])),
    "ft_mlp_ls": ("ft", dict(kind=S.KIND_TASK, vocab_size=756, stacked_feat=13, next_n_token=1, num_labels=1, score_bias=True,
                             head_mlp=(48, 32), layer_scale_init=1.0, embed_dim=64),
                  dict(num_labels=1, loss_type=None, mlp=[48, 32], embed_dim=64, problem_type="regression")),
}


def main():
    PT, FT, Cfg = MG.import_reference()
    from src.utils import loss_utils          # (the reference's: import_reference put its `src` first)
    out = {}
    for case, (kind, spec_kw, cfg_kw) in CASES.items():
        spec = S.spec_from_size("tiny", **spec_kw)
        model = (PT if kind == "pt" else FT)(MG.ref_config(Cfg, spec, **cfg_kw))
        name_of = {id(p): n for n, p in model.named_parameters()}
        out[case] = {}
        for version, fn in (("v1", loss_utils.get_layerwise_param_groups), ("v3", loss_utils.get_layerwise_param_groups_v3)):
            lrs = {}
            for g in fn(model, BASE_LR):
                for p in g["params"]:
                    assert name_of[id(p)] not in lrs, f"{case} {version}: {name_of[id(p)]} is in two groups"
                    lrs[name_of[id(p)]] = float(g["lr"])
            out[case][version] = lrs
            left = sorted(set(name_of.values()) - set(lrs))
            print(f"{case} {version}: {len(lrs)} parameters in groups, left out: {left}")
    path = os.path.join(MG.ROOT, "tests", "golden", "layerwise_lr.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print(f"{path} written")


if __name__ == "__main__":
    main()
