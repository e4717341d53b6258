"""The launch menu on the device: the data-parallel share of it belongs to the handle (gget_set_dp_menu), so two handles in one process
plan their GEMMs each with its own menu whatever the other does, and GgetEngine.set_dp_menu(reserve_cus=0) gives back exactly the
single-GPU selection.  The GEMM selection is observed through gget_debug_gemm_probe's launch count: with CUs reserved for a collective,
the q|k|v and o weight gradients of a d = 768 layer leave the grouped one-tile-per-CU launch for the split-K path (more launches)."""
import ctypes as C
import gc
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
eng_mod = importlib.import_module("graph-gpt_amd.engine")
modeling = importlib.import_module("graph-gpt_amd.modeling")
tr = importlib.import_module("graph-gpt_amd.training")
synth = importlib.import_module("graph-gpt_amd.synth")
spec_mod = importlib.import_module("graph-gpt_amd.spec")
weights_mod = importlib.import_module("graph-gpt_amd.weights")

B, S, F, V, D = 32, 32, 13, 756, 768


def _batch():
    b = synth.make_pretrain_batch(B=B, S=S, F=F, V=V, seed=77)
    return {k: torch.from_numpy(v).cuda() for k, v in b.items() if k != "lengths"}


def _probed(fn):
    """(GEMM launches of fn(), fn()'s result)"""
    lib = L.load()
    L.check(lib.gget_debug_gemm_probe(1, None, None, None, None))
    out = fn()
    torch.cuda.synchronize()
    n = C.c_int32()
    L.check(lib.gget_debug_gemm_probe(0, None, None, C.byref(n), None))
    return n.value, out


def test_two_handles_keep_their_own_launch_menu():
    spec = spec_mod.ModelSpec(kind=spec_mod.KIND_PRETRAIN, vocab_size=V, hidden_size=D, intermediate_size=4 * D, num_layers=2,
                              num_heads=D // 64, head_dim=64, stacked_feat=F, next_n_token=F, causal=False, max_position=1024)
    state = weights_mod.make_state_dict(spec, seed=9, std=0.02, head_std=0.05)
    b = _batch()

    def make(reserve_cus):
        e = eng_mod.Engine(spec, max_tokens=B * S, max_batch=B)
        e.load_state_dict(state)
        e.set_dp_menu(reserve_cus, False)
        return e

    def step(e):
        loss = float(e.forward_pretrain(b["input_ids"], b["attention_mask"], b["labels"]))
        e.backward()
        return loss, e.grad_bf16.clone()

    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):      # (the same handle, the same kernels -> the same bits)
        plain = make(0)
        n0, (l0, g0) = _probed(lambda: step(plain))
        dp = make(32)
        n_dp, _ = _probed(lambda: step(dp))
        assert n_dp > n0, (n_dp, n0)                    # the DP handle's wgrad plan differs ...
        n1, (l1, g1) = _probed(lambda: step(plain))
        assert (n1, l1) == (n0, l0) and torch.equal(g1, g0)     # ... and the plain handle's does not follow it
        del dp
        gc.collect()
        n2, (l2, g2) = _probed(lambda: step(plain))
        assert (n2, l2) == (n0, l0) and torch.equal(g2, g0)
        n3, _ = _probed(lambda: step(make(0)))          # a handle created after the DP one died: the single-GPU plan
        assert n3 == n0
        # ... and the DP handle's plan does not depend on a plain handle dying either
        dp2 = make(32)
        del plain
        gc.collect()
        n4, _ = _probed(lambda: step(dp2))
        assert n4 == n_dp
    assert (L.debug_get(L.KEY_GEMM_CU_RESERVE), L.debug_get(L.KEY_RMS_WIDE), L.debug_get(L.KEY_GEMM_LDS_HEADROOM)) == (0, 1, 1)


def test_set_dp_menu_zero_is_the_single_gpu_selection(monkeypatch):
    monkeypatch.delenv("GGET_DP_LDS_HEADROOM", raising=False)
    cfg = modeling.GraphGPTConfig(hidden_act="gelu", vocab_size=V, hidden_size=D, intermediate_size=4 * D, num_hidden_layers=2,
                                  num_attention_heads=D // 64, max_position_embeddings=1024, causal_attention=False,
                                  stacked_feat=F, next_n_token=F)
    b = _batch()

    def step(model, en):
        out = en(input_ids=b["input_ids"], attention_mask=b["attention_mask"], labels=b["labels"])
        en.backward(out.head1_loss)
        return float(out.head1_loss)

    fresh_m = modeling.GraphGPTPretrainBase(cfg, seed=1)
    fresh = tr.initialize(fresh_m, tr.OptimConfig(lr=1e-3))
    n_fresh, _ = _probed(lambda: step(fresh_m, fresh))
    model = modeling.GraphGPTPretrainBase(cfg, seed=1)
    en = tr.initialize(model, tr.OptimConfig(lr=1e-3))
    en.set_dp_menu(reserve_cus=32)
    n32, _ = _probed(lambda: step(model, en))
    assert n32 > n_fresh, (n32, n_fresh)
    en.set_dp_menu(reserve_cus=0)
    assert en.reserved_cus == 0
    assert L.debug_get(L.KEY_GEMM_LDS_HEADROOM) == 1 and L.debug_get(L.KEY_GEMM_CU_RESERVE) == 0 and L.debug_get(L.KEY_RMS_WIDE) == 1
    n0, _ = _probed(lambda: step(model, en))
    assert n0 == n_fresh, (n0, n_fresh)
    # the menu follows the model to the handle it re-creates for a bigger batch
    en.set_dp_menu(reserve_cus=32)
    old = model._engine
    model._ensure_engine(2 * B, S)
    assert model._engine is not old
    n_big, _ = _probed(lambda: step(model, en))
    assert n_big == n32, (n_big, n32)
    assert np.isfinite(step(model, en))
