"""The float64 statement of the intra-instance token head (tests/_intra_ref.py) against the reference fixture, and its bounds against
a correct fp32 statement (inside, ratio < 1) and planted faults (noticed) on the inputs the GPU test uses - what shows that
tests/test_gpu_intra_head.py would notice a subtly wrong kernel.  The new C ABI names are declared on both sides."""
import os
import re

import numpy as np
import pytest
import torch

import _heads_ref as H
import _intra_ref as R
from _util import GOLDEN, ROOT, spec_mod, weights_mod
from oracle import gget_oracle as O


def params(cases):
    return [pytest.param(*args, id=name) for name, args in cases]


def intra_fixture():
    z = np.load(os.path.join(GOLDEN, "ft_tiny_tokence_intra.npz"))
    spec = spec_mod.spec_from_size("tiny", kind=spec_mod.KIND_TASK, vocab_size=756, stacked_feat=13, next_n_token=1, num_labels=5)
    assert [int(x) for x in z["meta_spec"]] == list(spec.as_c_ints())
    seed, std, hstd = z["meta_init"]
    state = weights_mod.make_state_dict(spec, seed=int(seed), std=float(std), head_std=float(hstd))
    b = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    return z, spec, state, b


def test_float64_statement_reproduces_the_reference_fixture():
    """The oracle's final hidden states (fp32, the reference's own precision) through _intra_ref in float64: the fixture's logits to
    fp32 round-off (a cosine of two fp32 rows of d = 128 terms times 20: 1e-4 absolute is 5e-6 of the largest possible logit, the
    tolerance the token_ce sibling in tests/test_oracle_golden.py uses relative to its logits of order 1) and its loss to 1e-5."""
    z, spec, state, b = intra_fixture()
    C = 5
    lens = b["attention_mask"].sum(1)
    assert bool((b["cls_idx"] == lens - C).all()) and int(lens.min()) >= C + 2
    lab = b["task_labels"]
    assert tuple(lab.shape) == (10, 24) and int((lab[3] >= 0).sum()) == 0 and int((lab >= 0).sum()) > 20
    for i in range(10):      # -100 on the label rows and the pads
        assert bool((lab[i, int(b["cls_idx"][i]):] == -100).all())
    p = O.to_params(state, torch.float32, requires_grad=False)
    out = O.task_forward(spec, p, b["input_ids"], b["attention_mask"], b["position_ids"])
    logits = R.intra_logits_grid(out["hidden"], b["cls_idx"], C)
    assert tuple(logits.shape) == tuple(z["logits"].shape) == (10, 24, C)
    np.testing.assert_allclose(logits.numpy(), z["logits"].astype(np.float64), rtol=1e-4, atol=1e-4)
    loss = float(R.token_ce(logits, lab))
    assert abs(loss - float(z["loss"])) <= 1e-5 * abs(float(z["loss"])), (loss, float(z["loss"]))
    names = [str(n) for n in z["names"]]
    gn = dict(zip(names, z["grad_norms"]))
    assert gn["score.weight"] == 0.0 and gn["model.layers.1.mlp.down_proj.weight"] > 0.0      # `score` is outside the graph


def test_float64_backward_is_the_gradient_of_the_float64_forward():
    """intra_backward against autograd through the float64 forward + cross-entropy on one of the GPU test's inputs."""
    i = R.intra_case(64, 2, (3, 7, 130), False, "last")
    h = i["hidden"].double().requires_grad_(True)
    nx = h.norm(dim=-1).clamp_min(R.EPS)
    xh = h / nx[:, None]
    z = torch.randn(i["rows"], i["C"], generator=H.gen(1), dtype=torch.float64)
    total = 0.0
    for b in range(i["B"]):
        rs, re, k = int(i["row_start"][b]), int(i["row_start"][b + 1]), int(i["cls_idx"][b])
        total = total + (R.INV_TEMP * xh[rs:re] @ xh[rs + k:rs + k + i["C"]].t() * z[rs:re]).sum()
    total.backward()
    ref, _ = R.intra_backward(i["hidden"], i["row_start"], i["cls_idx"], i["C"], R.INV_TEMP * z)
    assert float((ref - h.grad).abs().max()) <= 1e-12 * float(h.grad.abs().max())


@pytest.mark.parametrize("d,Cn,lens,padded,place", params(R.INTRA_CASES))
def test_fp32_statement_is_inside_the_bounds(d, Cn, lens, padded, place):
    i = R.intra_case(d, Cn, lens, padded, place)
    assert any(n == Cn + 1 for n in lens) or len(lens) == 1 or min(lens) > Cn + 1
    ratio = H.must_hold(R.intra_fwd_check(i, R.intra_fwd_fp32(i)))
    assert ratio < 1.0, ratio
    ratio = H.must_hold(R.intra_bwd_check(i, R.INV_N, R.intra_bwd_fp32(i, R.INV_N)))
    assert ratio < 1.0, ratio
    H.must_hold(R.intra_bwd_check(i, 0.0, R.intra_bwd_fp32(i, 0.0)))


def test_inputs_hold_what_the_cases_promise():
    i = R.intra_case(768, 5, (6, 13, 67, 1024), True, "last")
    rs, k, C = i["row_start"].tolist(), i["cls_idx"].tolist(), i["C"]
    assert rs[0] == R.LEAD and rs[1] - rs[0] > 6 and not bool(i["inside"][:R.LEAD].any())
    lab = i["labelled"]
    assert int(lab[rs[1]:rs[2]].sum()) == 0                                         # a sample without a labelled row
    assert bool(lab[rs[0] + k[0] + C // 2]) and int(lab[rs[0] + k[0]:rs[0] + k[0] + C].sum()) == 1      # one labelled label row
    assert int(lab[rs[0]:rs[0] + k[0]].sum()) == 1                                  # the one other row of the C + 1 sample
    assert bool((i["dl"][~lab] == 0).all()) and bool((i["dl"][lab].abs().sum(1) > 0).all())
    assert not bool(lab[rs[3] + 1024:rs[4]].any())                                  # pad rows carry no label


@pytest.mark.parametrize("fault", ["no_projection", "no_label_sum"])
def test_planted_backward_faults_are_noticed(fault):
    i = R.intra_case(768, 5, (6, 13, 67, 1024), True, "last")
    msgs = H.settle(R.intra_bwd_check(i, R.INV_N, R.intra_bwd_fp32(i, R.INV_N, fault=fault)))[1]
    assert msgs, "the planted fault went unnoticed"


def test_planted_forward_faults_are_noticed():
    i = R.intra_case(128, 12, (13, 37, 66), False, "mid")
    good = R.intra_fwd_fp32(i)
    j = dict(i, cls_idx=i["cls_idx"] + 1)                    # label rows one row late
    assert H.settle(R.intra_fwd_check(i, R.intra_fwd_fp32(j)))[1]
    assert H.settle(R.intra_fwd_check(i, (good / R.INV_TEMP * 19.0).to(torch.bfloat16).float()))[1]     # a wrong temperature
    x = i["hidden"].float()
    unnorm = torch.cat([(x[int(a):int(b)] @ x[int(a) + int(k):int(a) + int(k) + 12].t()) for a, b, k in
                        zip(i["row_start"][:-1], i["row_start"][1:], i["cls_idx"])])
    assert H.settle(R.intra_fwd_check(i, unnorm.to(torch.bfloat16).float()))[1]                           # no normalisation


def test_new_abi_names_are_declared_on_both_sides():
    with open(os.path.join(ROOT, "include", "gget.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "graph-gpt_amd", "_lib.py")) as f:
        lib = f.read()
    for name in ("gget_op_tok_intra_fwd", "gget_op_tok_intra_bwd", "gget_set_cls_idx"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert f'"{name}"' in lib, name
    assert re.search(r"#define GGET_PROBLEM_TOKEN_CE_INTRA 6\b", header)
    assert re.search(r"^PROBLEM_TOKEN_CE_INTRA = 6\b", lib, re.M)
