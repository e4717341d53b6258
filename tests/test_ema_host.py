"""Host-side checks of the weight EMA (`training.optimizer.use_ema`): the decay rule, the config plumbing on both optimizer branches and
both modes, the C ABI entries (header = exports = ctypes table; a NULL handle is an error, not a crash), the model_ema.pt layout and the
reference-named fronts in `src.conf`.  No GPU."""
import copy
import ctypes as C
import importlib
import json
import os
import re
import types

import pytest
import torch

from _util import ROOT

L = importlib.import_module("graph-gpt_amd._lib")
EMA_ENTRIES = ("gget_ema_attach", "gget_set_ema_decay", "gget_ema_update", "gget_ema_to_params")


def _ns(obj):
    if isinstance(obj, dict):
        return types.SimpleNamespace(**{k: _ns(v) for k, v in obj.items()})
    return obj


def _engine_without_gpu(**optim_kw):
    """A GgetEngine around a model that never touches the device (the decay rule is host logic)."""
    tr = importlib.import_module("graph-gpt_amd.training")
    M = importlib.import_module("graph-gpt_amd.modeling")
    model = M.GraphGPTPretrainBase(M.GraphGPTConfig(hidden_act="gelu", vocab_size=300, hidden_size=128, intermediate_size=512,
                                                    num_hidden_layers=2, num_attention_heads=2, causal_attention=False, stacked_feat=1,
                                                    next_n_token=1))
    return tr.GgetEngine(model, tr.OptimConfig(**optim_kw))


@pytest.mark.parametrize("d", [0.9999, 0.9995, 0.5])
def test_ema_decay_at_copies_twice_then_averages(d):
    eng = _engine_without_gpu(use_ema=True, ema_decay=d)
    assert [eng.ema_decay_at(s) for s in range(4)] == [0.0, 0.0, d, d]
    assert eng.ema_decay_at(10 ** 6) == d


def test_optim_config_defaults_and_range():
    tr = importlib.import_module("graph-gpt_amd.training")
    o = tr.OptimConfig()
    assert o.use_ema is False and o.ema_decay == 0.9999
    assert tr.OptimConfig(use_ema=True, ema_decay=0.5).use_ema is True
    with pytest.raises(ValueError):
        tr.OptimConfig(use_ema=True, ema_decay=1.5)


@pytest.mark.parametrize("case_name,finetune", [("pretrain_ds", False), ("pretrain_ddp", False), ("finetune_ds", True)])
@pytest.mark.parametrize("use_deepspeed", [True, False])
def test_optim_from_training_carries_use_ema(case_name, finetune, use_deepspeed):
    """`training.optimizer.use_ema / ema_decay` reach OptimConfig on the DeepSpeed and the DDP branch, for both modes.  Fine-tuning hands
    the configured decay on (finetune_mode.py:256); pre-training averages with timm's default 0.9999 whatever `ema_decay` says, because
    the reference calls init_ema(model) without it (pretrain_mode.py:302) - reproduced."""
    CF = importlib.import_module("graph-gpt_amd.conf")
    with open(os.path.join(ROOT, "tests", "golden", "pipeline_config.json")) as fh:
        training = copy.deepcopy(json.load(fh)[case_name]["training"])
    training["schedule"]["total_num_steps"], training["schedule"]["warmup_num_steps"] = 100, 10
    training["deepspeed_conf_file"] = "ds_config2.json" if use_deepspeed else ""      # (absent: the stage's default scheduler type)
    for use_ema, decay in ((False, 0.9999), (True, 0.9995)):
        training["optimizer"]["use_ema"], training["optimizer"]["ema_decay"] = use_ema, decay
        for tree in (_ns(training), training):
            o = CF.optim_from_training(tree, use_deepspeed, finetune)
            assert o.use_ema is use_ema
            assert o.ema_decay == (decay if finetune else 0.9999)


@pytest.fixture(scope="module")
def lib():
    importlib.import_module("graph-gpt_amd.build").build()
    return L.load()


def test_abi_declares_exports_and_lists_the_ema_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "gget.h")).read()
    declared = set(re.findall(r"\b(gget_[a-z0-9_]+)\s*\(", hdr))
    for name in EMA_ENTRIES:
        assert name in declared, f"{name} is not declared in include/gget.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES
    assert re.search(r"#define\s+GGET_SHARD_EMA\s+5\b", hdr) and L.SHARD_EMA == 5


def test_abi_null_handle_is_an_error_not_a_crash(lib):
    assert lib.gget_ema_update(None, C.c_float(0.5), None) != 0
    assert b"ema_update" in lib.gget_last_error() and len(lib.gget_last_error()) > 0
    assert lib.gget_ema_attach(None, None) != 0 and b"ema_attach" in lib.gget_last_error()
    assert lib.gget_set_ema_decay(None, C.c_float(0.5)) != 0 and b"set_ema_decay" in lib.gget_last_error()
    assert lib.gget_ema_to_params(None, None) != 0 and b"ema_to_params" in lib.gget_last_error()


def test_ema_state_dict_file_round_trip(tmp_path):
    """The EMA save path (fed from a CPU tensor dict, no engine) writes what `read_state_dict(<dir>/ckp, use_ema=True)` reads from
    <dir>/ckp/../model_ema_best.pt: identical keys, shapes and bits."""
    CK = importlib.import_module("graph-gpt_amd.checkpoint")
    g = torch.Generator().manual_seed(5)
    sd = {"model.embed_tokens.weight": torch.randn(7, 16, generator=g), "model.layers.0.mlp.down_proj.weight": torch.randn(16, 64, generator=g),
          "model.norm.weight": torch.randn(16, generator=g), "emb_mask_token": torch.randn(1, 1, 16, generator=g)}
    sd["model.norm.weight"][3] = 1e-30
    out = tmp_path / "run"
    path = CK.save_ema_state_dict(sd, str(out), best=True)
    assert os.path.basename(path) == "model_ema.pt" and os.path.isfile(out / "model_ema.pt") and os.path.isfile(out / "model_ema_best.pt")
    os.makedirs(out / "ckp")
    for got in (CK.read_state_dict(str(out / "ckp"), use_ema=True), CK.read_state_dict(str(out / "model_ema.pt"))):
        assert list(got) == list(sd)
        for k in sd:
            assert got[k].shape == sd[k].shape and got[k].dtype == torch.float32
            assert torch.equal(got[k].view(torch.int32), sd[k].view(torch.int32)), k
    # without `best` only model_ema.pt is (re)written
    out2 = tmp_path / "run2"
    CK.save_ema_state_dict(sd, str(out2))
    assert os.path.isfile(out2 / "model_ema.pt") and not os.path.exists(out2 / "model_ema_best.pt")


def test_src_conf_has_the_reference_names():
    import dataclasses
    from src.conf import EMAConfig, EMAStats
    c = EMAConfig()
    assert (c.use_ema, c.ema_file, c.ema_file_best) == (False, "model_ema.pt", "model_ema_best.pt")
    s = EMAStats(ema_cfg=EMAConfig(use_ema=True))
    assert {f.name for f in dataclasses.fields(EMAStats)} >= {"model_ema", "ema_cfg", "ema_best_flag", "ema_best_res"}
    assert s.model_ema is None and s.ema_best_flag is False and s.ema_best_res is None
    for name in ("init_ema", "update_ema", "save_ema_ckp", "load_ema_ckp", "ema2device"):
        assert callable(getattr(s, name))
    # the front switches the ENGINE's averaging on and leaves the update to it
    eng = _engine_without_gpu()
    assert eng.optim.use_ema is False
    s.init_ema(eng, None, 0.9995)
    assert s.model_ema is eng and eng.optim.use_ema is True and eng.optim.ema_decay == 0.9995
    assert s.update_ema(eng, step=3, ft=True) is None and eng.ema_updates == 0
    with pytest.raises(RuntimeError):        # an engine nobody switched on would go un-averaged
        s.update_ema(_engine_without_gpu(), step=3, ft=True)
    off = EMAStats()
    off.init_ema(eng, None, 0.5)
    assert off.model_ema is None and eng.optim.ema_decay == 0.9995
    assert off.update_ema(eng, step=0) is None
    off.save_ema_ckp("/nonexistent")        # (no EMA: nothing is written, nothing raises - stats_configs.py:138-139)
