"""The float64 statement of the attention weights (tests/_attn_ref.py) against the reference fixtures, and its bound against a correct
fp32 statement (inside, ratio < 1) and planted faults (noticed) on the shapes the GPU test uses - what shows that
tests/test_gpu_attn_probs.py would notice a subtly wrong kernel.  The new C ABI names are declared on both sides."""
import os
import re

import numpy as np
import pytest
import torch

import _attn_ref as R
import _heads_ref as H
from _util import GOLDEN, ROOT, spec_mod, weights_mod
from oracle import gget_oracle as O


def case(shape, kind):
    B, S, Hn, lens = shape
    qkv = R.attn_inputs(B, S, Hn, kind, R.case_seed(B, S, Hn, kind))
    q, k = R.split_qk(qkv, B, S, Hn)
    return B, S, Hn, lens, q, k


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("causal", [False, True], ids=["bidir", "causal"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_fp32_statement_is_inside_the_bound(shape, causal, kind):
    B, S, Hn, lens, q, k = case(shape, kind)
    ok = R.allowed_padded(B, S, lens, causal)
    ratio = H.must_hold(R.attn_check(R.attn_probs_fp32(q, k, lens, causal), q, k, ok))
    assert ratio < 1.0, ratio
    for p in (0.1, 0.5):
        keep = R.attn_drop_keep(77, B, Hn, S, p)
        ratio = H.must_hold(R.attn_check(R.attn_probs_fp32(q, k, lens, causal, keep=keep), q, k, ok, keep=keep, p_drop=p))
        assert ratio < 1.0, ratio


def test_fp32_statement_is_inside_the_bound_on_packed_rows():
    lo, hi = R.packed_ranges()
    for kind in R.KINDS:
        qkv = R.attn_inputs(2, 64, 2, kind, R.case_seed(2, 64, 2, kind) + 1)
        q, k = R.split_qk(qkv, 2, 64, 2)
        ok = R.allowed_packed(lo, hi)
        assert not bool(ok[:, 57:].any()) and int(ok[0, 0].sum()) == 1 and int(ok[1, 21].sum()) == 1      # trailing padding; one-token graphs
        ratio = H.must_hold(R.attn_check(R.attn_probs_fp32(q, k, None, False, packed=(lo, hi)), q, k, ok))
        assert ratio < 1.0, ratio


def test_inputs_hold_what_the_kinds_promise():
    """"unit": scores of order 1.  "peaked": key 0 dominates every row, and the row's weights run from about 1 down to underflow."""
    B, S, Hn, lens, q, k = case(R.SHAPES[5], "unit")
    r = R.attn_probs64(q, k, R.allowed_padded(B, S, lens, False))
    assert 0.5 < float(r["x"].std()) < 2.0
    B, S, Hn, lens, q, k = case(R.SHAPES[5], "peaked")
    r = R.attn_probs64(q, k, R.allowed_padded(B, S, lens, False))
    live = r["ref"][0, :, :lens[0], :lens[0]]
    assert float(live[:, :, 0].min()) > 0.5
    assert float(live.min()) < H.TINY and int(((live > H.TINY) & (live < 1e-30)).sum()) > 0 and int(((live > 1e-6) & (live < 0.1)).sum()) > 0


# every planted fault on the smallest shape that can show it (H = 2 for the layout fault, a short sample for the key limit)
FAULTS = ["swap_qk", "no_scale", "lse_log2", "key_limit", "no_diagonal", "bqhk"]


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_faults_are_noticed(fault):
    B, S, Hn, lens, q, k = case(R.SHAPES[2], "unit")        # (2, 40, 2, [33, 40])
    causal = fault == "no_diagonal"
    ok = R.allowed_padded(B, S, lens, causal)
    H.must_hold(R.attn_check(R.attn_probs_fp32(q, k, lens, causal), q, k, ok))
    assert H.settle(R.attn_check(R.attn_probs_fp32(q, k, lens, causal, fault=fault), q, k, ok))[1], "the planted fault went unnoticed"


def test_planted_dropout_field_swap_is_noticed():
    B, S, Hn, lens, q, k = case(R.SHAPES[2], "unit")
    ok = R.allowed_padded(B, S, lens, False)
    keep = R.attn_drop_keep(77, B, Hn, S, 0.5)
    bad = R.attn_drop_keep(77, B, Hn, S, 0.5, swap_fields=True)
    assert not torch.equal(keep, bad)
    assert H.settle(R.attn_check(R.attn_probs_fp32(q, k, lens, False, keep=bad), q, k, ok, keep=keep, p_drop=0.5))[1]


def test_dropout_twin_is_the_projects_twin():
    """tests/_attn_ref.py holds a COPY of the twin: it must stay the function the model tests use."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_gpu_model_for_twin", os.path.join(ROOT, "tests", "test_gpu_model.py"))
    with open(spec.origin) as f:
        src = f.read()
    body = src[src.index("def _attn_drop_keep("):]
    body = body[:body.index("\n\n\n")]
    ns = {"np": np, "torch": torch}
    exec(body, ns)
    for seed, p in ((1, 0.1), (0xDEADBEEF, 0.5)):
        assert torch.equal(ns["_attn_drop_keep"](seed, 2, 3, 40, p), R.attn_drop_keep(seed, 2, 3, 40, p))
    assert R.layer_seed(0xFFFFFFF0, 1) == (0xFFFFFFF0 + 0x9E37) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------ reference fixtures
def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = [int(x) for x in z["meta_spec"]]
    kw = dict(vocab_size=m[1], stacked_feat=m[6], next_n_token=m[7])
    if m[0] == spec_mod.KIND_TASK:
        kw.update(kind=spec_mod.KIND_TASK, num_labels=m[11])
    spec = spec_mod.spec_from_size("tiny", **kw)
    assert m == list(spec.as_c_ints())
    seed, std, hstd = z["meta_init"]
    state = weights_mod.make_state_dict(spec, seed=int(seed), std=float(std), head_std=float(hstd))
    b = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    return z, spec, state, b


def oracle_qk(spec, state, b):
    """Rotated q, k [B,H,S,64] of every layer in fp32 from the oracle's own functions: the layer inputs of backbone(collect=), then
    rmsnorm, the projection weights and rope_cos_sin / apply_rope."""
    p = O.to_params(state, torch.float32, requires_grad=False)
    ids = b["input_ids"][:, :, :spec.stacked_feat]
    x, _ = O.stacked_embed(p["model.embed_tokens.weight"], ids, p.get("stacked_feat_agg.weight"))
    outs = []
    O.backbone(spec, p, x, b["attention_mask"], b["position_ids"], collect=outs)
    B, S, _ = x.shape
    cos, sin = O.rope_cos_sin(b["position_ids"], spec.head_dim, spec.rope_theta, x.dtype)
    res = []
    for i, xin in enumerate([x] + outs[:-1]):
        pre = f"model.layers.{i}."
        h = O.rmsnorm(xin, p[pre + "input_layernorm.weight"], spec.rms_eps)
        q = (h @ p[pre + "self_attn.q_proj.weight"].t()).view(B, S, spec.num_heads, spec.head_dim).transpose(1, 2)
        k = (h @ p[pre + "self_attn.k_proj.weight"].t()).view(B, S, spec.num_heads, spec.head_dim).transpose(1, 2)
        res.append(O.apply_rope(q, k, cos, sin))
    return res


@pytest.mark.parametrize("name", ["attn_tiny_pt", "attn_tiny_ft"])
def test_float64_statement_reproduces_the_reference_fixture(name):
    """The reference's own `outputs.attentions` (fp32, eager): exact zeros at padded keys and rows that sum to 1 - the fixture's own
    properties the GPU tests rely on - and on the rows of real queries the float64 statement, at the fp32 tolerance
    tests/test_oracle_golden.py holds the oracle's activations to (rtol 2e-4, atol 2e-5).  The rows of padding queries are the stated
    difference: the reference's softmax of meaningless queries over the real keys, zero here."""
    z, spec, state, b = fixture(name)
    att = z["attentions"]
    lens = b["lengths"].tolist()
    assert att.shape == (spec.num_layers, 3, spec.num_heads, 40, 40) and lens == [40, 23, 1]
    assert bool((b["attention_mask"].sum(1) == b["lengths"]).all())
    for bb, n in enumerate(lens):
        assert np.all(att[:, bb, :, :, n:] == 0.0)
    assert np.abs(att.sum(-1) - 1.0).max() < 1e-5
    ok = R.allowed_padded(3, 40, lens, bool(spec.causal))
    for i, (q, k) in enumerate(oracle_qk(spec, state, b)):
        r = R.attn_probs64(q, k, ok)
        for bb, n in enumerate(lens):
            np.testing.assert_allclose(r["ref"][bb, :, :n].numpy(), att[i, bb, :, :n].astype(np.float64), rtol=2e-4, atol=2e-5)
            assert bool((r["ref"][bb, :, n:] == 0).all())


def test_new_abi_names_are_declared_on_both_sides():
    with open(os.path.join(ROOT, "include", "gget.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "graph-gpt_amd", "_lib.py")) as f:
        lib = f.read()
    for name in ("gget_attention_probs", "gget_layer_qkv_grid", "gget_op_attn_probs"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert f'"{name}"' in lib, name
