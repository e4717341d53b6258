"""The unchanged CPU oracle (oracle/gget_oracle.py) against every fixture of the model sizes with 32-wide heads (tiny6, small12;
tools/make_golden_hd32.py captured them from the real reference): loss, logits and gradient norms to the tolerances
tests/test_oracle_golden.py holds the 64-wide tiny and full-width cases to."""
import numpy as np
import pytest
import torch

from _hd32_util import BIG32, FT32, PT32, load_case32
from _util import ADAM, CLIP, ft_problem, rel_l2, tb
from oracle import gget_oracle as O


def _fwd_fn(spec, b, kind, name=""):
    if kind == "pt":
        def fn(p):
            return O.pretrain_forward(spec, p, b["input_ids"], b["attention_mask"], b["labels"], b.get("wgt"))
        return fn, "head1_loss", "head1_logits"
    problem, loss_type = ft_problem(spec, b, name)

    def fn(p):
        return O.task_forward(spec, p, b["input_ids"], b["attention_mask"], b["position_ids"], b["task_labels"],
                              sample_wgt=b.get("wgt"), problem_type=problem, loss_type=loss_type)
    return fn, "task_loss", "task_logits"


@pytest.mark.parametrize("name", PT32 + FT32)
def test_oracle_fp32_matches_reference_at_head_width_32(name):
    z, spec, state, batch = load_case32(name)
    assert (spec.hidden_size, spec.num_layers, spec.num_heads, spec.intermediate_size) == (128, 6, 4, 512)
    kind = "pt" if name.startswith("pt") else "ft"
    b = tb(batch)
    p = O.to_params(state, torch.float32)
    fn, lk, gk = _fwd_fn(spec, b, kind, name)
    out, grads = O.loss_and_grads(fn, p, lk)
    assert abs(out[lk].item() - float(z["loss"])) <= 1e-5 * abs(float(z["loss"])) + 1e-6
    lg = out[gk].detach().float().numpy()
    assert tuple(lg.shape) == tuple(int(x) for x in z["logits_shape"])
    np.testing.assert_allclose(lg[:64], z["logits"], rtol=2e-4, atol=2e-5)
    gn = np.array([float(grads[n].norm()) for n in state.keys()])
    np.testing.assert_allclose(gn, z["grad_norms"], rtol=2e-4, atol=1e-7)
    assert rel_l2(grads["model.embed_tokens.weight"].numpy(), z["grad_embed"]) < 1e-4
    assert rel_l2(grads["model.layers.0.self_attn.q_proj.weight"].numpy(), z["grad_l0_q"]) < 1e-4
    assert rel_l2(grads["model.layers.1.mlp.down_proj.weight"].numpy(), z["grad_l1_down"]) < 1e-4


@pytest.mark.parametrize("name", BIG32)
def test_oracle_fp32_matches_reference_small12(name):
    """small12 (d384 / L12 / H12 / ff384): loss, logits, every per-parameter gradient norm and 64 x 64 gradient blocks, at the
    tolerances of the full-width cases of tests/test_oracle_golden.py."""
    z, spec, state, batch = load_case32(name)
    assert (spec.hidden_size, spec.num_layers, spec.num_heads, spec.intermediate_size) == (384, 12, 12, 384)
    b = tb(batch)
    p = O.to_params(state, torch.float32)
    fn, lk, gk = _fwd_fn(spec, b, "pt", name)
    out, grads = O.loss_and_grads(fn, p, lk)
    assert abs(out[lk].item() - float(z["loss"])) <= 2e-5 * abs(float(z["loss"]))
    np.testing.assert_allclose(out[gk].detach().float().numpy()[:64], z["logits"], rtol=5e-4, atol=5e-4)
    gn = np.array([float(grads[n].norm()) for n in state.keys()])
    np.testing.assert_allclose(gn, z["grad_norms"], rtol=5e-4, atol=1e-7)
    for tag, pn in (("l0_q", "model.layers.0.self_attn.q_proj.weight"), ("l0_k", "model.layers.0.self_attn.k_proj.weight"),
                    ("l11_q", "model.layers.11.self_attn.q_proj.weight"), ("l11_k", "model.layers.11.self_attn.k_proj.weight"),
                    ("l5_down", "model.layers.5.mlp.down_proj.weight"), ("l5_gate", "model.layers.5.mlp.gate_proj.weight")):
        assert rel_l2(grads[pn].numpy()[:64, :64], z["gradblk_" + tag]) < 5e-4, tag


@pytest.mark.parametrize("name", ["pt_tiny6_f13", "pt_tiny6_s72"])
def test_oracle_bf16_tracks_reference_bf16_at_head_width_32(name):
    """(pre-train cases, as tests/test_oracle_golden.py holds the big-weight cases: the 2-class CE of 32 big-weight samples moves by
    5e-3 between two bf16 evaluation orders - its own bf16-vs-fp32 gap, what loss_tolerance takes from the fixture)"""
    z, spec, state, batch = load_case32(name)
    kind = "pt" if name.startswith("pt") else "ft"
    b = tb(batch)
    p = O.to_params(state, torch.bfloat16, requires_grad=False)
    fn, lk, gk = _fwd_fn(spec, b, kind, name)
    with torch.no_grad():
        out = fn(p)
    assert abs(out[lk].item() - float(z["loss_bf16"])) <= 2e-3 * abs(float(z["loss_bf16"])) + 1e-3
    assert rel_l2(out[gk].float().numpy()[:64], z["logits_bf16"]) < 2e-2


@pytest.mark.parametrize("name", ["pt_tiny6_f13", "ft_tiny6_f4_b32"])
def test_oracle_adamw_trajectory_at_head_width_32(name):
    z, spec, state, batch = load_case32(name)
    kind = "pt" if name.startswith("pt") else "ft"
    b = tb(batch)
    p = O.to_params(state, torch.float32)
    fn, lk, _ = _fwd_fn(spec, b, kind, name)
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(v_) for k, v_ in p.items()}
    losses, gns = [], []
    for step in range(1, 4):
        out, grads = O.loss_and_grads(fn, p, lk)
        losses.append(out[lk].item())
        with torch.no_grad():
            gns.append(O.adamw_step({k: t for k, t in p.items()}, grads, m, v, step, ADAM["lr"], ADAM["beta1"],
                                    ADAM["beta2"], ADAM["eps"], ADAM["wd"], CLIP))
    with torch.no_grad():
        losses.append(fn(p)[lk].item())
    np.testing.assert_allclose(losses, z["adamw_losses"], rtol=3e-4, atol=1e-5)
    np.testing.assert_allclose(gns, z["adamw_gnorms"], rtol=3e-4)
    fin = np.array([float(p[n].detach().norm()) for n in state.keys()])
    np.testing.assert_allclose(fin, z["adamw_final_norms"], rtol=1e-4)
