"""Layer-wise learning-rate decay and parameter groups, host side (no GPU): the drop-in group builders of src/utils/loss_utils.py
against tests/golden/layerwise_lr.json - the reference's get_layerwise_param_groups (v1) and get_layerwise_param_groups_v3 run on
three reference models (tools/make_golden_llrd.py; CASES here mirrors CASES there) -, layerwise_lr_scales, and the host logic of
GgetEngine.set_param_groups / initialize(OptimConfig(layerwise_lr_decay=, no_decay_1d=)) against a stub engine that records the
table it is handed."""
import importlib
import json
import math
import os

import pytest
import torch

from _util import GOLDEN

M = importlib.import_module("graph-gpt_amd.modeling")
T = importlib.import_module("graph-gpt_amd.training")
from src.utils import loss_utils  # noqa: E402

BASE_LR = 3e-4
DECAY = {"v1": 0.95, "v3": 0.5}       # the reference functions' own defaults (what the fixture was made with)
TINY = dict(hidden_act="gelu", hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, causal_attention=False,
            stack_method="short")
CASES = {
    "pt_tiny": (M.GraphGPTPretrainBase, dict(vocab_size=756, stacked_feat=13, next_n_token=13)),
    "ft_linear": (M.GraphGPTTaskModel, dict(vocab_size=1000, stacked_feat=4, num_labels=2)),
    "ft_mlp_ls": (M.GraphGPTTaskModel, dict(vocab_size=756, stacked_feat=13, num_labels=1, mlp=[48, 32], layer_scale_init_value=1.0, problem_type="regression",
                                            embed_dim=64)),
}
# what the reference's groups leave out, and the group whose depth they take here
LEFT_OUT = {"pt_tiny": {"n_token_proj.weight": "lm_head.weight"},
            "ft_linear": {},
            "ft_mlp_ls": {"embed_layernorm.weight": "model.embed_tokens.weight", "embed_proj.weight": "model.embed_tokens.weight"}}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "layerwise_lr.json")) as fh:
        return json.load(fh)


_BUILT = {}


def _model(case):
    if case not in _BUILT:
        cls, kw = CASES[case]
        _BUILT[case] = cls(M.GraphGPTConfig(**TINY, **kw))
    return _BUILT[case]


def _lrs(model, groups):
    name_of = {id(p): n for n, p in model._flat.items()}
    out = {}
    for g in groups:
        for p in g["params"]:
            assert name_of[id(p)] not in out
            out[name_of[id(p)]] = g["lr"]
    return out


@pytest.mark.parametrize("version", ["v1", "v3"])
@pytest.mark.parametrize("case", list(CASES))
def test_drop_in_groups_reproduce_the_reference(golden, case, version):
    model = _model(case)
    fn = {"v1": loss_utils.get_layerwise_param_groups, "v3": loss_utils.get_layerwise_param_groups_v3}[version]
    got = _lrs(model, fn(model, BASE_LR))
    want = golden[case][version]
    assert set(got) == set(want), f"membership differs: {sorted(set(got) ^ set(want))}"
    assert set(model._flat) - set(got) == set(LEFT_OUT[case])
    for name, lr in want.items():
        assert got[name] == lr, (name, got[name], lr)      # (the same float64 expression: math.pow(decay, depth) * base_lr)
    assert len(set(want.values())) == (2 if version == "v3" else model.config.num_hidden_layers + 3)


@pytest.mark.parametrize("version", [1, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_layerwise_lr_scales_equal_lr_over_base_lr(golden, case, version):
    model = _model(case)
    decay = DECAY[f"v{version}"]
    scales = T.layerwise_lr_scales(model, decay, version)
    assert set(scales) == set(model._flat)
    want = golden[case][f"v{version}"]
    for name, lr in want.items():
        assert scales[name] == pytest.approx(lr / BASE_LR, rel=1e-14), name
        assert scales[name] * BASE_LR == pytest.approx(lr, rel=1e-14)
    # the parameters the reference leaves out take the depth of the group they feed
    for name, like in LEFT_OUT[case].items():
        assert scales[name] == scales[like], (name, like)
    depths = T.layerwise_depths(model._flat, model.config.num_hidden_layers, version, True)
    assert all(scales[n] == math.pow(decay, d) for n, d in depths.items())
    if version == 1:
        head = "lm_head.weight" if case == "pt_tiny" else [n for n in model._flat if n.startswith("score.")][0]
        L_ = model.config.num_hidden_layers
        assert depths[head] == 0 and depths["model.norm.weight"] == 1 and depths["model.layers.0.mlp.down_proj.weight"] == L_ + 1
        assert depths["model.embed_tokens.weight"] == L_ + 3        # (behind the stacked_feat_agg group, which holds no parameter here)


def test_version_2_is_not_offered():
    assert not hasattr(loss_utils, "get_layerwise_param_groups_v2")
    with pytest.raises(ValueError):
        T.layerwise_lr_scales(_model("pt_tiny"), 0.5, 2)
    with pytest.raises(ValueError):
        T.OptimConfig(layerwise_lr_decay=0.5, layerwise_lr_version=2)


# ------------------------------------------------------------------------------------------------ set_param_groups on a stub engine
class _StubEngine:
    """what GgetEngine hands the table to: records it (Engine.set_param_scales checks the names the same way)"""

    def __init__(self, names):
        self.params = {n: {} for n in names}
        self.calls = []
        self._params_are_ema = False

    def set_param_scales(self, lr_scale=None, wd_scale=None):
        for d in (lr_scale or {}, wd_scale or {}):
            assert set(d) <= set(self.params)
        self.calls.append((lr_scale, wd_scale))


def _engine(case, optim=None, stub=True):
    cls, kw = CASES[case]
    model = cls(M.GraphGPTConfig(**TINY, **kw))
    if stub:
        model._engine = _StubEngine(model._flat)
    return model, T.initialize(model, optim or T.OptimConfig(lr=BASE_LR, weight_decay=0.1))


def test_param_in_no_group_raises_with_the_names():
    model, eng = _engine("pt_tiny")
    groups = loss_utils.get_layerwise_param_groups(model, BASE_LR, 0.5)
    with pytest.raises(ValueError, match="n_token_proj.weight") as ei:
        eng.set_param_groups(groups)
    assert "no group" in str(ei.value) and not model._engine.calls and eng._param_scales is None


def test_rest_lr_scale_is_honoured_and_lr_is_divided_by_the_base():
    model, eng = _engine("pt_tiny")
    groups = loss_utils.get_layerwise_param_groups(model, BASE_LR, 0.5)
    eng.set_param_groups(groups, rest_lr_scale=0.25)
    (lr_s, wd_s), = model._engine.calls
    assert set(lr_s) == set(wd_s) == set(model._flat)
    assert lr_s["n_token_proj.weight"] == 0.25 and wd_s["n_token_proj.weight"] == 1.0
    want = _lrs(model, groups)
    for n, lr in want.items():
        assert lr_s[n] == lr / BASE_LR and wd_s[n] == 1.0
    assert lr_s["lm_head.weight"] == 1.0 and lr_s["model.norm.weight"] == 0.5 and lr_s["model.embed_tokens.weight"] == 0.5 ** 5
    # names, lr_scale, weight_decay and wd_scale keys
    eng.set_param_groups([{"params": ["lm_head.weight", "n_token_proj.weight"], "lr_scale": 2.0, "weight_decay": 0.05},
                          {"params": model.model.layers[0].parameters(), "wd_scale": 0.0}], rest_lr_scale=1.0)
    lr_s, wd_s = model._engine.calls[-1]
    assert lr_s["lm_head.weight"] == 2.0 and wd_s["n_token_proj.weight"] == 0.05 / 0.1
    assert wd_s["model.layers.0.mlp.up_proj.weight"] == 0.0 and lr_s["model.layers.0.mlp.up_proj.weight"] == 1.0
    assert lr_s["model.layers.1.mlp.up_proj.weight"] == 1.0 and wd_s["model.layers.1.mlp.up_proj.weight"] == 1.0
    # the learning rates of a step: lr_at(step) times the scale
    eng.last_lr = 1e-4
    assert eng.last_lrs["lm_head.weight"] == 2e-4 and eng.last_lrs["model.norm.weight"] == 1e-4


def test_param_in_two_groups_raises():
    model, eng = _engine("ft_linear")
    groups = [{"params": list(model.parameters())}, {"params": [model.score.weight], "lr": 1e-3}]
    with pytest.raises(ValueError, match="more than one parameter group") as ei:
        eng.set_param_groups(groups)
    assert "score.weight" in str(ei.value) and not model._engine.calls
    with pytest.raises(KeyError):
        eng.set_param_groups([{"params": ["no.such.weight"]}], rest_lr_scale=1.0)
    with pytest.raises(KeyError):
        eng.set_param_groups([{"params": [torch.nn.Parameter(torch.zeros(3))]}], rest_lr_scale=1.0)
    with pytest.raises(ValueError):
        eng.set_param_groups([{"params": ["score.weight"], "lr": 1e-3, "lr_scale": 2.0}], rest_lr_scale=1.0)


@pytest.mark.parametrize("case", list(CASES))
def test_initialize_applies_layerwise_decay_and_no_decay_1d(case):
    model, eng = _engine(case, T.OptimConfig(lr=BASE_LR, layerwise_lr_decay=0.5, layerwise_lr_version=1, no_decay_1d=True))
    (lr_s, wd_s), = model._engine.calls
    assert lr_s == T.layerwise_lr_scales(model, 0.5, 1)
    one_d = {n for n, p in model._flat.items() if p.ndim == 1}
    assert {n for n, s in wd_s.items() if s == 0.0} == one_d and all(s == 1.0 for n, s in wd_s.items() if n not in one_d)
    assert "model.norm.weight" in one_d and "model.layers.0.input_layernorm.weight" in one_d and "model.embed_tokens.weight" not in one_d
    if case == "ft_mlp_ls":
        assert {"model.layers.1.lambda_2", "score.mlp_modules.0.bias", "embed_layernorm.weight"} <= one_d


def test_groups_reach_an_engine_created_later():
    """no engine yet (the model has not met the GPU): the table is kept and handed over by step(), and again to a re-created engine"""
    model, eng = _engine("ft_linear", T.OptimConfig(lr=BASE_LR, no_decay_1d=True), stub=False)
    assert model._engine is None and eng._param_scales is not None
    for _ in range(2):      # (a second stub = the model re-created its engine)
        stub = _StubEngine(model._flat)
        assert getattr(stub, "_param_scales_from", None) is not eng._param_scales
        eng._apply_param_scales(stub)
        assert stub._param_scales_from is eng._param_scales and stub.calls[0][1]["model.norm.weight"] == 0.0
    model2, eng2 = _engine("ft_linear")
    assert eng2._param_scales is None and not model2._engine.calls      # (no option set: nothing is handed over)
