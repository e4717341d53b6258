"""Host side of the two model sizes with 32-wide attention heads (tiny6, small12 of the reference's launch scripts): the size table,
ModelSpec / GraphGPTConfig guards and gget_query_sizes; no GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from _hd32_util import load_case32

L = importlib.import_module("graph-gpt_amd._lib")
spec_mod = importlib.import_module("graph-gpt_amd.spec")
modeling = importlib.import_module("graph-gpt_amd.modeling")
engine_mod = importlib.import_module("graph-gpt_amd.engine")

# the rows of the reference's architecture table (examples/graph_lvl/pcqm4m_v2_pretrain.sh:158-240): hidden, layers, heads, intermediate
TABLE = {"tiny6": (128, 6, 4, 512), "small12": (384, 12, 12, 384)}
FIXTURE = {"tiny6": "pt_tiny6_f13", "small12": "pt_small12_f13"}


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.mark.parametrize("size", sorted(TABLE))
def test_size_table_builds_a_spec_with_head_dim_32(size):
    d, layers, heads, ff = TABLE[size]
    assert spec_mod.MODEL_SIZES[size] == dict(hidden_size=d, num_layers=layers, num_heads=heads, intermediate_size=ff)
    spec = spec_mod.spec_from_size(size, vocab_size=756, stacked_feat=13, next_n_token=13)
    assert (spec.hidden_size, spec.num_layers, spec.num_heads, spec.intermediate_size, spec.head_dim) == (d, layers, heads, ff, 32)
    # the parameter table of the reference: names and shapes of the weights the fixture's generator made for the reference model
    z, fspec, state, _ = load_case32(FIXTURE[size])
    assert list(spec.as_c_ints()) == [int(x) for x in z["meta_spec"]]
    table = spec.param_table()
    assert list(table) == list(state) and all(tuple(state[n].shape) == tuple(table[n]) for n in table)
    assert len(z["grad_norms"]) == len(table)


def test_existing_sizes_are_unchanged():
    for name, (d, layers) in dict(tiny=(128, 2), mini=(256, 4), small=(512, 4), medium=(512, 8), base=(768, 12), base24=(768, 24),
                                  large=(1024, 24)).items():
        s = spec_mod.spec_from_size(name)
        assert (s.hidden_size, s.num_layers, s.num_heads, s.head_dim, s.intermediate_size) == (d, layers, d // 64, 64, 4 * d)


def test_rope_tables_follow_the_head_width():
    cos, sin = engine_mod.rope_tables(40, 32, 10000.0)
    assert tuple(cos.shape) == tuple(sin.shape) == (40, 16)
    inv = 1.0 / (10000.0 ** (np.arange(16, dtype=np.float32) * 2 / 32))
    np.testing.assert_allclose(cos[7].numpy(), np.cos(np.float32(7) * inv), rtol=0, atol=1e-6)


@pytest.mark.parametrize("hidden,heads,head_dim", [(64, 4, 16), (256, 2, 128), (128, 2, 32), (128, 4, 64)])
def test_other_widths_and_inconsistent_triples_raise(hidden, heads, head_dim):
    with pytest.raises(AssertionError, match="head_dim"):
        spec_mod.ModelSpec(hidden_size=hidden, num_heads=heads, head_dim=head_dim)
    cfg = modeling.GraphGPTConfig(hidden_act="gelu", hidden_size=hidden, num_attention_heads=heads, head_dim=head_dim,
                                  intermediate_size=4 * hidden)
    with pytest.raises(NotImplementedError, match="head_dim"):
        cfg.to_spec(spec_mod.KIND_PRETRAIN)


@pytest.mark.parametrize("size", sorted(TABLE))
def test_config_passes_the_head_width_through(size):
    d, layers, heads, ff = TABLE[size]
    for kw in (dict(), dict(head_dim=32)):       # hf: head_dim None -> hidden_size // num_attention_heads
        cfg = modeling.GraphGPTConfig(hidden_act="gelu", hidden_size=d, num_attention_heads=heads, intermediate_size=ff, num_hidden_layers=layers, **kw)
        spec = cfg.to_spec(spec_mod.KIND_PRETRAIN)
        assert (spec.head_dim, spec.num_heads, spec.hidden_size) == (32, heads, d)


def _cfg(spec):
    cfg = L.GgetConfig()
    (cfg.kind, cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_layers, cfg.num_heads, cfg.stacked_feat,
     cfg.next_n_token, cfg.gated_agg, cfg.causal, cfg.max_position, cfg.num_labels, cfg.score_bias,
     cfg.pad_token_id) = spec.as_c_ints()
    cfg.rms_eps, cfg.rope_theta, cfg.layer_scale_init, cfg.max_tokens, cfg.max_batch = 1e-6, 1e4, 0.0, 8192, 256
    return cfg


@pytest.mark.parametrize("size", sorted(TABLE))
def test_query_sizes_accepts_head_width_32(lib, size):
    spec = spec_mod.spec_from_size(size, vocab_size=756, stacked_feat=13, next_n_token=13)
    cfg, sz = _cfg(spec), L.GgetSizes()
    L.check(lib.gget_query_sizes(C.byref(cfg), C.byref(sz)))
    assert sz.n_params >= spec.num_params() and sz.n_params - spec.num_params() < 64 * 1024 * (spec.num_layers + 2)
    assert sz.workspace_bytes > 0


def test_query_sizes_rejects_head_width_48(lib):
    spec = spec_mod.spec_from_size("small12", vocab_size=756, stacked_feat=13, next_n_token=13)
    cfg, sz = _cfg(spec), L.GgetSizes()
    cfg.num_heads = 8          # 384 / 8 = 48
    assert lib.gget_query_sizes(C.byref(cfg), C.byref(sz)) == 2
    msg = lib.gget_last_error().decode()
    assert "unsupported" in msg and "head_dim" in msg, msg
    cfg.num_heads = 0
    assert lib.gget_query_sizes(C.byref(cfg), C.byref(sz)) != 0
