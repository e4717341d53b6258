"""`training.finetune.freeze` on the host (no GPU): `freeze_layers(k)` leaves exactly the reference's names with requires_grad = False
and `print_trainable_parameters` reports the reference's count (tests/golden/freeze_names.json, written from the real reference by
tools/make_golden.py freeze_names: L = 3, with / without gated aggregation and LayerScale, freeze in {-1, 0, 1, 2, 3, 5}), and
`FinetuneMode.post_model_setup` applies a reference-shaped Config."""
import importlib
import json
import os
import types

import pytest

from _util import GOLDEN

M = importlib.import_module("graph-gpt_amd.modeling")
T = importlib.import_module("graph-gpt_amd.training")

with open(os.path.join(GOLDEN, "freeze_names.json")) as _fh:
    FIX = json.load(_fh)


def _model(gated=False, layer_scale=0.0):
    m = FIX["model"]
    return M.GraphGPTTaskModel(M.GraphGPTConfig(
        hidden_act="gelu", vocab_size=m["vocab_size"], hidden_size=m["hidden_size"], intermediate_size=m["intermediate_size"],
        num_hidden_layers=m["num_layers"], num_attention_heads=m["num_heads"], causal_attention=False, stacked_feat=m["stacked_feat"],
        num_labels=m["num_labels"], stacked_feat_agg_method="gated" if gated else "sum", layer_scale_init_value=layer_scale))


@pytest.mark.parametrize("case", FIX["cases"], ids=lambda c: f"gate{int(c['gated'])}_ls{int(c['layer_scale'] > 0)}_k{c['freeze']}")
def test_frozen_names_and_trainable_count_match_the_reference(case):
    from src.utils import modules_utils
    model = _model(case["gated"], case["layer_scale"])
    assert sum(p.numel() for p in model.parameters()) == case["total"]
    if case["freeze"] > -1:
        modules_utils.freeze_llama_layers(model, case["freeze"])
    frozen = sorted(n for n, p in model.named_parameters() if not p.requires_grad)
    assert frozen == case["frozen"]
    assert sorted(model.frozen_names()) == case["frozen"]
    assert modules_utils.print_trainable_parameters(model) == case["trainable"]
    assert all(p.grad is None for n, p in model.named_parameters() if n in set(frozen))
    assert len(model.state_dict()) == len(list(model.named_parameters()))     # frozen entries stay in the state dict


def test_freeze_minus_one_touches_nothing():
    model = _model()
    model.freeze_layers(-1)
    assert model._frozen_layers == -1 and model.frozen_names() == []
    assert all(p.requires_grad for p in model.parameters())


def _pipeline(freeze):
    cfg = types.SimpleNamespace(tokenization=None, model=types.SimpleNamespace(), generation=None,
                                training=types.SimpleNamespace(finetune=types.SimpleNamespace(freeze=freeze), optimizer=types.SimpleNamespace(),
                                                               schedule=types.SimpleNamespace()))
    p = T.TrainingPipeline(cfg, T.FinetuneMode(batches=[]))
    assert p.reference_cfg
    p._extract_config()
    p.model = _model(layer_scale=1.0)
    return p


@pytest.mark.parametrize("freeze", [-1, 0, 2, 5])
def test_finetune_mode_post_model_setup_applies_the_config(freeze):
    """reference finetune_mode.py:204-212: freeze > -1 -> freeze_llama_layers; config.num_params = the trainable count; no early exit."""
    case = next(c for c in FIX["cases"] if not c["gated"] and c["layer_scale"] > 0 and c["freeze"] == freeze)
    p = _pipeline(freeze)
    assert p.mode.post_model_setup(p) is False
    assert sorted(n for n, q in p.model.named_parameters() if not q.requires_grad) == case["frozen"]
    assert p.model.config.num_params == case["trainable"]
    assert p.model._frozen_layers == (freeze if freeze > -1 else -1)


def test_pretrain_mode_does_not_read_the_field():
    p = _pipeline(1)
    assert T.PretrainMode(batches=[]).post_model_setup(p) is False
    assert all(q.requires_grad for q in p.model.parameters())
