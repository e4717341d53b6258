"""The references and bounds of tests/_heads_ref.py, checked on the CPU with the inputs the GPU test uses (tests/test_gpu_heads.py):
a correct fp32 statement of every operation stays inside its per-element bound (ratio < 1), and one planted fault at a time - a row
shifted by one, a class column swapped, a slice of the batch dropped from a weight-gradient sum, a missing 1/n and their like - does
not.  The second half is what shows that the GPU test would notice a subtly wrong kernel."""
import importlib

import pytest
import torch

import _heads_ref as R

M = importlib.import_module("graph-gpt_amd.modeling")


def params(cases):
    return [pytest.param(*args, id=name) for name, args in cases]


def passes(results):
    ratio = R.must_hold(results)
    assert ratio < 1.0, ratio
    return ratio


def caught(results, where=None):
    msgs = R.settle(results)[1]
    assert msgs, "the planted fault went unnoticed"
    if where is not None:
        assert any(where in m for m in msgs), (where, msgs)


# ------------------------------------------------------------------------------------------------------------------ fp32 statements pass
@pytest.mark.parametrize("B,Cn,d,bias", params(R.SCORE_CASES))
def test_score_head_fp32_statement_is_inside_the_bounds(B, Cn, d, bias):
    i = R.score_case(B, Cn, d, bias)
    passes(R.score_fwd_check(i, *R.score_fwd_fp32(i)))
    passes(R.score_bwd_check(i, *R.score_bwd_fp32(i)))


@pytest.mark.parametrize("T,Cn,d,bias", params(R.TOK_CASES))
def test_tok_score_head_fp32_statement_is_inside_the_bounds(T, Cn, d, bias):
    i = R.tok_case(T, Cn, d, bias)
    passes(R.tok_score_fwd_check(i, R.tok_score_fwd_fp32(i)))
    for inv_n in (1.0 / 64, 0.0):
        passes(R.tok_score_bwd_check(i, inv_n, *R.tok_score_bwd_fp32(i, inv_n)))


@pytest.mark.parametrize("T,Cn,ignore,rows_map", params(R.TOK_CE_CASES))
def test_tok_ce_fp32_statement_is_inside_the_bounds(T, Cn, ignore, rows_map):
    i = R.tok_ce_case(T, Cn, ignore, rows_map)
    if rows_map:
        y = R.tok_ce_row_labels(i)
        assert bool((i["rows_map"][-5:] >= i["n_logical"]).all()) and bool((y[-5:] == -100).all()) and not bool((i["rows_map"][:-5] >= i["n_logical"]).any())
    passes(R.tok_ce_check(i, *R.tok_ce_fp32(i)))


@pytest.mark.parametrize("problem,B,Cn,weights,nan", params(R.TASK_CASES))
def test_task_loss_fp32_statement_is_inside_the_bounds(problem, B, Cn, weights, nan):
    i = R.task_case(problem, B, Cn, weights, nan)
    x = i["logits"]
    assert torch.equal(x, x.to(torch.bfloat16).float()) and (B < 4 or (float(x[1].min()) > 20 and float(x[2].max()) < -20))
    if problem in (R.L1, R.MSE):
        assert (bool((x == i["labels"]).any()) or B * Cn == 1) and not bool((x == i["labels"]).all())
    if problem == R.MULTI:
        lab = ~torch.isnan(i["labels"])
        assert int(lab.sum()) == (0 if nan == 1.0 else B * Cn if nan == 0.0 else int(lab.sum())) and (nan in (0.0, 1.0) or 0 < int(lab.sum()) < B * Cn)
    passes(R.task_loss_check(i, *R.task_loss_fp32(i)))


@pytest.mark.parametrize("B,num_neg,Cn,labels", params(R.AUC_CASES))
def test_auc_fp32_statement_is_inside_the_bounds(B, num_neg, Cn, labels):
    i = R.auc_case(B, num_neg, Cn, labels)
    idx = M.auc_pairs(i["labels"].numpy(), num_neg, R.AUC_SEED + B)
    assert int((i["labels"] != 0).sum()) * num_neg <= 8192
    passes(R.auc_check(i, idx, *R.auc_fp32(i, idx)))


@pytest.mark.parametrize("B,Din,Dout,bias", params(R.HEAD_CASES))
def test_head_linear_fp32_statement_is_inside_the_bounds(B, Din, Dout, bias):
    i = R.head_case(B, Din, Dout, bias)
    a, y, y32 = R.head_fwd_fp32(i)
    passes(R.head_fwd_check(i, a, y, y32))
    passes(R.head_bwd_check(i, a, *R.head_bwd_fp32(i, a)))


def test_pool_sample_is_a_distinct_unsorted_sample_with_both_ends():
    for B in (1, 2, 15, 17, 33, 300):
        pr = R.pool_sample(R.gen(B), B, 2 * B + 3).tolist()
        assert len(set(pr)) == B and 2 * B + 2 in pr and (B == 1 or (0 in pr and pr != sorted(pr)))


# ------------------------------------------------------------------------------------------------------------------ planted faults
def test_planted_faults_in_the_pooled_head_are_caught():
    i = R.score_case(17, 5, 128, True)
    logits, pooled = R.score_fwd_fp32(i)
    caught(R.score_fwd_check(i, logits.roll(1, 0), pooled), "logits")                    # every row one off
    swapped = logits.clone()
    swapped[:, [1, 3]] = logits[:, [3, 1]]
    caught(R.score_fwd_check(i, swapped, pooled), "logits")                               # two class columns swapped
    nobias = logits.clone()
    nobias[:, 4] = ((logits[:, 4].double() - i["bias"][4].double()).float()).to(torch.bfloat16).float()
    caught(R.score_fwd_check(i, nobias, pooled), "logits")                                # the last class without its bias
    wrong = pooled.clone()
    wrong[16, 127] = wrong[15, 127]
    caught(R.score_fwd_check(i, logits, wrong), "pooled_h")
    dw, dbias, dh = R.score_bwd_fp32(i)
    pr, dl = i["pool_row"].long(), i["dlogits"]
    # slice 8 of kScoreSplit = 16 (B = 17: per = 2, the slice holds row 16 alone) dropped from the dw / dbias sums
    caught(R.score_bwd_check(i, dw - dl[16:].t() @ i["hidden"].float()[pr[16:]], dbias, dh), "dw")
    caught(R.score_bwd_check(i, dw, dbias - dl[16], dh), "dbias")
    caught(R.score_bwd_check(i, dw - i["dw0"], dbias, dh), "dw")                          # overwritten instead of accumulated
    moved = torch.zeros_like(dh)
    moved[(pr + 1) % i["rows"]] = dh[pr]
    caught(R.score_bwd_check(i, dw, dbias, moved), "dhidden")                             # written one row off
    stray = dh.clone()
    free = [r for r in range(i["rows"]) if r not in pr.tolist()][0]
    stray[free, 0] = 2.0 ** -20
    caught(R.score_bwd_check(i, dw, dbias, stray), "dhidden")                             # a row outside pool_row touched


def test_planted_faults_in_the_token_head_are_caught():
    i = R.tok_case(513, 65, 768, False)
    logits = R.tok_score_fwd_fp32(i)
    last_row = logits.clone()
    last_row[512] = logits[511]
    caught(R.tok_score_fwd_check(i, last_row), "logits")                                  # the row of the last, one-row block
    no_round2 = logits.clone()
    no_round2[:, 64] = 0.0
    caught(R.tok_score_fwd_check(i, no_round2), "logits")                                 # the second c0 round never stored
    not_bf16 = logits.clone()
    not_bf16[3, 3] += 2.0 ** -12
    caught(R.tok_score_fwd_check(i, not_bf16), "bf16 values")
    inv_n = 1.0 / 64
    dw, dbias, dh = R.tok_score_bwd_fp32(i, inv_n)
    g = R.tok_grad(i, inv_n).float()
    caught(R.tok_score_bwd_check(i, inv_n, dw - g[512:].t() @ i["hidden"].float()[512:], dbias, dh), "dw")   # the second 512-row slab dropped
    one_class = dw.clone()
    one_class[64] = i["dw0"][64]
    caught(R.tok_score_bwd_check(i, inv_n, one_class, dbias, dh), "dw")                   # class 64 (the ninth group of 8) never added
    caught(R.tok_score_bwd_check(i, inv_n, dw, dbias, (i["dl"] @ i["w"].float() * inv_n).roll(1, 0).to(torch.bfloat16)), "dhidden")
    caught(R.tok_score_bwd_check(i, 0.0, dw, dbias, dh))                                  # gradients although no row is labelled
    ib = R.tok_case(1030, 9, 768, True)
    dw, dbias, dh = R.tok_score_bwd_fp32(ib, inv_n)
    gb = R.tok_grad(ib, inv_n).float()
    caught(R.tok_score_bwd_check(ib, inv_n, dw, dbias + 2 * gb.sum(0), dh), "dbias")      # dbias added in each of the three j0 rounds


def test_planted_faults_in_the_token_cross_entropy_are_caught():
    i = R.tok_ce_case(513, 65, 0.3, False)
    dl, stat, loss = R.tok_ce_fp32(i)
    n = float(stat[1])
    caught(R.tok_ce_check(i, dl, stat, loss * n), "loss")                                 # the missing 1 / n
    caught(R.tok_ce_check(i, dl.roll(1, 0), stat, loss), "dl")
    caught(R.tok_ce_check(i, dl / n, stat, loss), "dl")                                   # dl is NOT yet divided by n
    y = R.tok_ce_row_labels(i)
    t = int((y >= 0).nonzero()[-1])
    one = dl.clone()
    one[t, int(y[t])] += 1.0
    caught(R.tok_ce_check(i, one, stat, loss), f"row(s) [{t}]")                           # the one-hot not subtracted in the last labelled row
    fewer = stat.clone()
    fewer[1] -= 1
    caught(R.tok_ce_check(i, dl, fewer, loss), "stat[1]")
    unl = int((y < 0).nonzero()[0])
    leak = dl.clone()
    leak[unl] = torch.softmax(i["logits"][unl], 0)
    caught(R.tok_ce_check(i, leak, stat, loss), f"row(s) [{unl}]")                         # an ignored row with a gradient
    im = R.tok_ce_case(513, 9, 0.3, True)
    dl, stat, loss = R.tok_ce_fp32(im)
    direct = dict(im, rows_map=None, n_logical=513, labels=im["labels"][:513])            # rows_map ignored: labels read by the compact row
    caught(R.tok_ce_check(im, *R.tok_ce_fp32(direct)))
    ia = R.tok_ce_case(17, 7, 1.0, False)
    dl, stat, loss = R.tok_ce_fp32(ia)
    caught(R.tok_ce_check(ia, dl, stat, torch.zeros(1)), "loss")                          # 0 where the reference's mean over nothing is NaN


def test_planted_faults_in_the_task_loss_are_caught():
    i = R.task_case(R.SINGLE, 257, 128, False, 0.0)
    loss, dl = R.task_loss_fp32(i)
    x, y = i["logits"], i["labels"]
    row = (torch.logsumexp(x[256], 0) - x[256, y[256]]) / 257
    caught(R.task_loss_check(i, loss - row, dl), "loss")                                  # row 256, the second round of b += 256, not summed
    caught(R.task_loss_check(i, loss, dl * 257 / 256), "dlogits")                         # mean over 256 rows
    hot = dl.clone()
    hot[256, y[256]] += 1.0 / 257
    caught(R.task_loss_check(i, loss, hot), "row(s) [256]")                               # the one-hot not subtracted in the last row
    iw = R.task_case(R.SINGLE, 1000, 5, True, 0.0)
    loss, dl = R.task_loss_fp32(iw)
    sw = iw["sample_wgt"]
    caught(R.task_loss_check(iw, loss, dl * (sw.sum() / sw[:768].sum())), "dlogits")      # the weight sum without its last round
    ir = R.task_case(R.L1, 257, 3, False, 0.0)
    loss, dl = R.task_loss_fp32(ir)
    same = ir["logits"] == ir["labels"]
    caught(R.task_loss_check(ir, loss, torch.where(same, torch.full_like(dl, 1.0 / 771), dl)), "dlogits")   # sign(0) = 1
    caught(R.task_loss_check(ir, loss * 3, dl), "loss")                                   # mean over B, not B * C
    im = R.task_case(R.MULTI, 255, 5, False, 0.4)
    loss, dl = R.task_loss_fp32(im)
    n = float((~torch.isnan(im["labels"])).sum())
    caught(R.task_loss_check(im, loss * n / (255 * 5), dl), "loss")                       # mean over every entry, labelled or not
    caught(R.task_loss_check(im, loss, dl * n / (255 * 5)), "dlogits")
    col = dl.clone()
    col[:, [0, 4]] = dl[:, [4, 0]]
    caught(R.task_loss_check(im, loss, col), "dlogits")
    ia = R.task_case(R.MULTI, 6, 5, False, 1.0)
    caught(R.task_loss_check(ia, torch.zeros(1), torch.zeros(6, 5)), "loss")              # loss 0 where the reference gives NaN


def test_planted_faults_in_the_auc_loss_are_caught():
    i = R.auc_case(300, 8, 2, "mixed")
    idx = M.auc_pairs(i["labels"].numpy(), 8, R.AUC_SEED + 300)
    loss, dl, pos, neg = R.auc_fp32(i, idx)
    caught(R.auc_check(i, idx, loss, dl[:, [1, 0]], pos, neg), "dlogits")                 # the two logit columns swapped
    pos0, neg0, bp, bn = R.auc_pairing(i, idx)
    x = i["logits"]
    t = 1 - ((x[bp[-1], 1] - x[bp[-1], 0]) - (x[bn[-1], 1] - x[bn[-1], 0]))
    g = 2 * t / len(bp)
    one = dl.clone()
    one[bp[-1], 1] += g
    caught(R.auc_check(i, idx, loss, one, pos, neg), f"row(s) [{int(bp[-1])}]")           # the last pair's term missing at one element
    caught(R.auc_check(i, idx, loss - t * t / len(bp), dl, pos, neg), "loss")             # the last pair missing from the loss
    other = idx.copy()
    other[0] = (other[0] + 1) % len(neg0)
    caught(R.auc_check(i, other, loss, dl, pos, neg), "dlogits")                          # one pair with another negative
    caught(R.auc_check(i, idx, loss, dl, pos, neg.roll(1)), "lists (negatives)")
    i0 = R.auc_case(24, 4, 2, "no_negative")
    idx0 = M.auc_pairs(i0["labels"].numpy(), 4, R.AUC_SEED + 24)
    loss, dl, pos, neg = R.auc_fp32(i0, idx0)
    caught(R.auc_check(i0, idx0, torch.zeros(1), dl, pos, neg), "loss")


def test_planted_faults_in_the_mlp_head_are_caught():
    i = R.head_case(17, 768, 256, True)
    a, y, y32 = R.head_fwd_fp32(i)
    caught(R.head_fwd_check(i, a, y.roll(1, 0), y32.roll(1, 0)), "y")
    caught(R.head_fwd_check(i, a, y, (y.float() + 2.0 ** -10)), "y32")
    tanh = torch.nn.functional.gelu(i["x"].float(), approximate="tanh").to(torch.bfloat16)
    caught(R.head_fwd_check(i, tanh, *R.head_fwd_fp32(i)[1:]), "a")                       # the tanh form of GELU instead of the erf form
    dx, dw, dbias = R.head_bwd_fp32(i, a)
    caught(R.head_bwd_check(i, a, dx, dw - i["dy"][16:].t() @ a.float()[16:], dbias), "dw")    # the last batch row dropped from dw
    caught(R.head_bwd_check(i, a, dx, dw, dbias - i["dy"][16]), "dbias")
    caught(R.head_bwd_check(i, a, i["dy"] @ i["w"].float(), dw, dbias), "dx")              # without the activation's derivative
    short = dx - (i["dy"][:, 255:] @ i["w"].float()[255:]) * (dx / (i["dy"] @ i["w"].float()))
    caught(R.head_bwd_check(i, a, short, dw, dbias), "dx")                                 # the last output column dropped from dx
