"""tests/_attn32_ref.py held to itself on the CPU: a correct fp32 statement of the head-width-32 contract passes every check, planted
faults do not (the 64-wide scale 1/8, RoPE pairing at distance 32 or 8, the dropout hash keyed with H = d / 64, a missing rotate-back,
lse left in the log2 domain), and the float64 statements reproduce the reference's own attention tensors of the tiny6 model
(tests/golden/attn_tiny6_padded.npz, attn_tiny6_packed.npz; tools/make_golden_hd32.py)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import _attn32_ref as A
import _heads_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gget_oracle as O  # noqa: E402

spec_mod = importlib.import_module("graph-gpt_amd.spec")
weights_mod = importlib.import_module("graph-gpt_amd.weights")
DH = 32

# one case per layout and mask / dropout / table form, small enough for the CPU: two key tiles, ragged lengths, an empty range
CPU_CASES = [A._case(3, 40, 4, (40, 1, 25), 0, 0.0, "unit"), A._case(3, 40, 4, (40, 1, 25), 1, 0.0, "rising", "memory", True),
             A._case(3, 40, 4, (40, 1, 25), 0, 0.1, "rising", "memory", False), A._case(2, 65, 3, (65, 33), 1, 0.1, "unit"),
             A._case(2, 40, 4, None, 0, 0.0, "rising", "memory", True, packed=True), A._case(2, 40, 4, None, 1, 0.1, "unit", packed=True),
             A._case(1, 1, 1, (1,), 0, 0.0, "unit")]


def run_fp32(pr, fwd_fault=None, bwd_fault=None):
    out, lse = A.forward_fp32(pr, fwd_fault)
    good_out, good_lse = (out, lse) if fwd_fault is None else A.forward_fp32(pr)
    dqkv = A.backward_fp32(pr, good_lse, good_out, bwd_fault)
    return out, lse, dqkv, good_out, good_lse


@pytest.mark.parametrize("c", CPU_CASES, ids=[c["id"] for c in CPU_CASES])
def test_fp32_statement_passes(c):
    pr = A.problem_of(c, DH)
    out, lse, dqkv, _, _ = run_fp32(pr)
    res = A.forward_check(pr, out, lse, zero_rows=pr.packed) + A.backward_check(pr, dqkv, lse, out)
    q, k, _ = A.split_qkv(pr.qkv, pr.B, pr.S, pr.Hn, DH)
    res += A.probs_check(A.probs_fp32(q, k, pr.allowed, DH, keep=pr.keep), q, k, pr.allowed, DH, keep=pr.keep, p_drop=pr.p)
    ratio = H.must_hold(res)
    assert ratio > 0.02 or pr.S == 1, "the bounds are far above what a correct fp32 statement needs"     # (S = 1: p = 1, nothing rounds)


def test_fp32_rope_statement_passes_and_pair_distance_is_noticed():
    B, S, Hn = 2, 33, 4
    qkv = H.randn_bf16(H.gen(11), B * S, 3 * Hn * DH)
    cos, sin = A.rope_tables(S + 16, DH)
    pos = torch.arange(S)[None].repeat(B, 1) + 5
    for inverse in (False, True):
        H.must_hold(A.rope_check(A.rope_fp32(qkv, cos, sin, pos, B, S, Hn, DH, inverse), qkv, cos, sin, pos, B, S, Hn, DH, inverse))
        assert H.settle(A.rope_check(A.rope_fp32(qkv, cos, sin, pos, B, S, Hn, DH, inverse, dist=8), qkv, cos, sin, pos, B, S, Hn, DH, inverse))[1]
        assert H.settle(A.rope_check(A.rope_fp32(qkv, cos, sin, pos, B, S, Hn, DH, not inverse), qkv, cos, sin, pos, B, S, Hn, DH, inverse))[1]
    # the 64-wide pairing (distance 32) on the same memory: channel j of one head with channel j of the next
    q64 = A.rope_fp32(qkv, torch.cat((cos, cos), -1), torch.cat((sin, sin), -1), pos, B, S, Hn // 2, 2 * DH)
    assert H.settle(A.rope_check(q64, qkv, cos, sin, pos, B, S, Hn, DH))[1], "RoPE at pair distance 32 went unnoticed"


FAULTS = [("scale_1_8", "fwd"), ("scale_1_8", "bwd"), ("hash_H64", "fwd"), ("hash_H64", "bwd"), ("lse_log2", "fwd"), ("no_rotate_back", "bwd"),
          ("pair_32", "bwd"), ("pair_8", "bwd")]


@pytest.mark.parametrize("fault,where", FAULTS, ids=[f"{f}-{w}" for f, w in FAULTS])
def test_planted_faults_are_noticed(fault, where):
    c = A._case(3, 40, 4, (40, 1, 25), 0, 0.1 if fault == "hash_H64" else 0.0, "rising", "memory", True)
    pr = A.problem_of(c, DH)
    out, lse, dqkv, good_out, good_lse = run_fp32(pr, fault if where == "fwd" else None, fault if where == "bwd" else None)
    if where == "fwd":
        assert H.settle(A.forward_check(pr, out, lse))[1], "the planted fault went unnoticed"
    else:
        H.must_hold(A.forward_check(pr, good_out, good_lse))
        assert H.settle(A.backward_check(pr, dqkv, good_lse, good_out))[1], "the planted fault went unnoticed"


@pytest.mark.parametrize("fault", ["scale_1_8", "lse_log2"])
def test_planted_faults_in_the_weights_are_noticed(fault):
    pr = A.problem_of(A._case(2, 40, 4, (40, 17), 0, 0.0, "unit"), DH)
    q, k, _ = A.split_qkv(pr.qkv, pr.B, pr.S, pr.Hn, DH)
    assert H.settle(A.probs_check(A.probs_fp32(q, k, pr.allowed, DH, fault=fault), q, k, pr.allowed, DH))[1]


def test_dropout_hash_with_another_head_count_is_another_mask():
    keep, bad = A.drop_keep(77, 3, 4, 40, 0.1), A.drop_keep(77, 3, 4, 40, 0.1, heads_in_hash=2)
    assert torch.equal(keep[0], bad[0]) and not torch.equal(keep[1:], bad[1:])
    assert torch.equal(keep, A.attn_drop_keep(77, 3, 4, 40, 0.1))


# ------------------------------------------------------------------------------------------------------------------ reference fixtures
def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = [int(x) for x in z["meta_spec"]]
    spec = spec_mod.spec_from_size("tiny6", vocab_size=m[1], stacked_feat=m[6], next_n_token=m[7])
    assert m == list(spec.as_c_ints()) and spec.head_dim == m[2] // m[5] == 32
    seed, std, hstd = z["meta_init"]
    state = weights_mod.make_state_dict(spec, seed=int(seed), std=float(std), head_std=float(hstd))
    b = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    return z, spec, state, b


def oracle_qk(spec, state, b):
    """Rotated q, k [B,H,S,32] of every layer in fp32 from the oracle's own functions (tests/test_attn_ref.py:oracle_qk)."""
    p = O.to_params(state, torch.float32, requires_grad=False)
    ids = b["input_ids"][:, :, :spec.stacked_feat]
    x, _ = O.stacked_embed(p["model.embed_tokens.weight"], ids, p.get("stacked_feat_agg.weight"))
    outs = []
    pos = b.get("position_ids") if b["attention_mask"].dim() == 2 else None
    O.backbone(spec, p, x, b["attention_mask"], pos, collect=outs)
    B, S, _ = x.shape
    rp = pos if pos is not None else torch.arange(S)[None].repeat(B, 1)
    cos, sin = O.rope_cos_sin(rp, spec.head_dim, spec.rope_theta, x.dtype)
    res = []
    for i, xin in enumerate([x] + outs[:-1]):
        pre = f"model.layers.{i}."
        h = O.rmsnorm(xin, p[pre + "input_layernorm.weight"], spec.rms_eps)
        q = (h @ p[pre + "self_attn.q_proj.weight"].t()).view(B, S, spec.num_heads, spec.head_dim).transpose(1, 2)
        k = (h @ p[pre + "self_attn.k_proj.weight"].t()).view(B, S, spec.num_heads, spec.head_dim).transpose(1, 2)
        res.append(O.apply_rope(q, k, cos, sin))
    return res


def test_float64_statement_reproduces_the_padded_reference_fixture():
    """The reference's own `outputs.attentions` of the tiny6 model (fp32, eager, head_dim 32): exact zeros at padded keys, rows that sum
    to 1, and on the rows of real queries the float64 statement at rtol 2e-4 / atol 2e-5 (the tolerance of tests/test_attn_ref.py)."""
    z, spec, state, b = fixture("attn_tiny6_padded")
    att = z["attentions"]
    lens = b["lengths"].tolist()
    assert att.shape == (6, 3, 4, 40, 40) and lens == [40, 23, 1]
    ok = A.allowed_padded(3, 40, lens, False)
    for i, (q, k) in enumerate(oracle_qk(spec, state, b)):
        r = A.probs64(q, k, ok, None, DH)
        for bb, n in enumerate(lens):
            assert np.all(att[i, bb, :, :, n:] == 0.0)
            np.testing.assert_allclose(r["ref"][bb, :, :n].numpy(), att[i, bb, :, :n].astype(np.float64), rtol=2e-4, atol=2e-5)
            assert bool((r["ref"][bb, :, n:] == 0).all())


def test_float64_statement_reproduces_the_packed_reference_fixture():
    """The same on packed rows: the allowed keys are the block-diagonal mask's rows (contiguous ranges: allowed_packed of their first
    and last 1), the tokens behind the packed length have no keys and are zero in the statement."""
    z, spec, state, b = fixture("attn_tiny6_packed")
    att = z["attentions"]
    m = b["attention_mask"].bool()
    B, S = m.shape[:2]
    live = m.any(-1)
    idx = torch.arange(S)[None, None, :]
    lo = torch.where(m, idx, S).amin(-1).masked_fill(~live, 0).int()
    hi = torch.where(m, idx, -1).amax(-1).int()
    ok = A.allowed_packed(lo, hi, False)
    assert torch.equal(ok, m), "the packed mask is not one contiguous key range per token"
    assert bool((~live).any()) and att.shape == (6, B, 4, S, S)
    for i, (q, k) in enumerate(oracle_qk(spec, state, b)):
        r = A.probs64(q, k, ok, None, DH)
        for bb in range(B):
            rows = live[bb]
            np.testing.assert_allclose(r["ref"][bb][:, rows].numpy(), att[i, bb][:, rows.numpy()].astype(np.float64), rtol=2e-4, atol=2e-5)
            assert bool((r["ref"][bb][:, ~rows] == 0).all())
