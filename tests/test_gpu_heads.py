"""The fine-tune heads and task losses, one kernel launcher at a time through the C ABI (gget_op_score_*, gget_op_tok_*, gget_op_task_loss,
gget_op_auc_loss, gget_op_head_linear_*, gget_op_pool_rows, gget_op_scatter_rows_f32), every output element against a float64 statement
of the same operation on the same bf16 / fp32 inputs (tests/_heads_ref.py: references, bounds and their derivation).  Outputs land in
buffers pre-filled with NaN sentinels with pad rows behind them; accumulating outputs start from known non-zero values.  The shapes are
the smallest that reach each branch of the kernels; the branch is named next to the case."""
import importlib

import pytest
import torch

import _heads_ref as R
from _gpu_out import SENT16, Out, P, ST, dev
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
M = importlib.import_module("graph-gpt_amd.modeling")


@pytest.fixture(scope="module")
def lib():
    return L.load()


def params(cases):
    return [pytest.param(*args, id=name) for name, args in cases]


def finish(op, case, results):
    """Record max(err / bound) of the case, then fail on whatever was out of bound."""
    ratio, msgs = R.settle(results)
    record_error(f"heads_elementwise/{op}", case, ratio, 1.0)
    assert not msgs, f"{op} {case}:\n" + "\n".join(msgs)


# ------------------------------------------------------------------------------------------------------------------ pooled head
@pytest.mark.parametrize("B,Cn,d,bias", params(R.SCORE_CASES))
def test_score_head(lib, request, B, Cn, d, bias):
    i = R.score_case(B, Cn, d, bias)
    hidden, pool_row, w, b = dev(i["hidden"]), dev(i["pool_row"]), dev(i["w"]), dev(i["bias"])
    logits, pooled = Out(B, Cn, torch.float32), Out(B, d, torch.bfloat16)
    L.check(lib.gget_op_score_fwd(P(hidden), P(pool_row), P(w), P(b), P(logits.buf), P(pooled.buf), B, Cn, d, ST()))
    finish("score_fwd", request.node.callspec.id, R.score_fwd_check(i, logits.body(), pooled.body()))
    # backward: dw / dbias accumulate onto known values, dhidden is pre-zeroed and only the pooled rows are written
    dw, dbias = Out(Cn, d, torch.float32, i["dw0"]), Out(1, Cn, torch.float32, i["db0"]) if bias else None
    dh = Out(i["rows"], d, torch.bfloat16, torch.zeros(i["rows"], d, dtype=torch.bfloat16))
    dlogits = dev(i["dlogits"])
    L.check(lib.gget_op_score_bwd(P(dlogits), P(hidden), P(pool_row), P(w), P(dw.buf), P(dbias.buf if bias else None), P(dh.buf),
                                  B, Cn, d, ST()))
    finish("score_bwd", request.node.callspec.id, R.score_bwd_check(i, dw.body(), dbias.body().view(-1) if bias else None, dh.body()))


# ------------------------------------------------------------------------------------------------------------------ token-level head
@pytest.mark.parametrize("T,Cn,d,bias", params(R.TOK_CASES))
def test_tok_score_head(lib, request, T, Cn, d, bias):
    i = R.tok_case(T, Cn, d, bias)
    hidden, w, b, dl_in = dev(i["hidden"]), dev(i["w"]), dev(i["bias"]), dev(i["dl"])      # (held in names: a freed block is reused)
    logits = Out(T, Cn, torch.float32)
    L.check(lib.gget_op_tok_score_fwd(P(hidden), P(w), P(b), P(logits.buf), T, Cn, d, ST()))
    finish("tok_score_fwd", request.node.callspec.id, R.tok_score_fwd_check(i, logits.body()))
    # backward with 1 / n = 1 / 64: bf16(dl / n) is exact in the reference
    for inv_n, tag in ((1.0 / 64, ""), (0.0, " no labelled row")):
        stat = torch.tensor([123.0, 64.0, inv_n, 0.0], device="cuda")
        dw, dbias, dh = Out(Cn, d, torch.float32, i["dw0"]), Out(1, Cn, torch.float32, i["db0"]) if bias else None, Out(T, d, torch.bfloat16)
        L.check(lib.gget_op_tok_score_bwd(P(dl_in), P(stat), P(hidden), P(w), P(dw.buf), P(dbias.buf if bias else None), P(dh.buf), T, Cn,
                                          d, ST()))
        finish("tok_score_bwd", request.node.callspec.id + tag,
               R.tok_score_bwd_check(i, inv_n, dw.body(), dbias.body().view(-1) if bias else None, dh.body()))


def test_tok_score_rejects_unsupported_widths(lib):
    """d % 64 != 0 and d > 1024 = 64 * kTokMaxCols are refused with the error code; nothing is launched, the output stays untouched."""
    T, Cn = 4, 3
    for d in (96, 1088):
        i = R.tok_inputs(T, Cn, d, True, seed=5)
        hidden, w, b, dl_in, stat = dev(i["hidden"]), dev(i["w"]), dev(i["bias"]), dev(i["dl"]), torch.zeros(4, device="cuda")
        logits = Out(T, Cn, torch.float32)
        rc = lib.gget_op_tok_score_fwd(P(hidden), P(w), P(b), P(logits.buf), T, Cn, d, ST())
        assert rc == 2 and b"unsupported" in lib.gget_last_error(), (d, rc, lib.gget_last_error())
        dw, dh = Out(Cn, d, torch.float32), Out(T, d, torch.bfloat16)
        rc = lib.gget_op_tok_score_bwd(P(dl_in), P(stat), P(hidden), P(w), P(dw.buf), None, P(dh.buf), T, Cn, d, ST())
        assert rc == 2 and b"unsupported" in lib.gget_last_error(), (d, rc, lib.gget_last_error())
        assert logits.untouched() and dw.untouched() and dh.untouched()


@pytest.mark.parametrize("T,Cn,ignore,rows_map", params(R.TOK_CE_CASES))
def test_tok_ce(lib, request, T, Cn, ignore, rows_map):
    i = R.tok_ce_case(T, Cn, ignore, rows_map)
    dl, stat, loss = Out(T, Cn, torch.float32), Out(1, 4, torch.float32), Out(1, 1, torch.float32)
    logits, labels, rm = dev(i["logits"]), dev(i["labels"]), dev(i["rows_map"])
    L.check(lib.gget_op_tok_ce(P(logits), P(labels), P(dl.buf), P(stat.buf), P(loss.buf), T, Cn, P(rm), i["n_logical"] if rows_map else 0, ST()))
    finish("tok_ce", request.node.callspec.id, R.tok_ce_check(i, dl.body(), stat.body().view(-1), loss.body().view(-1)))


# ------------------------------------------------------------------------------------------------------------------ task loss
@pytest.mark.parametrize("problem,B,Cn,weights,nan", params(R.TASK_CASES))
def test_task_loss(lib, request, problem, B, Cn, weights, nan):
    i = R.task_case(problem, B, Cn, weights, nan)
    loss, dl = Out(1, 1, torch.float32), Out(B, Cn, torch.float32)
    logits, labels, sw = dev(i["logits"]), dev(i["labels"]), dev(i["sample_wgt"])
    L.check(lib.gget_op_task_loss(P(logits), P(labels), P(sw), problem, B, Cn, P(loss.buf), P(dl.buf), ST()))
    finish("task_loss", request.node.callspec.id, R.task_loss_check(i, loss.body().view(-1), dl.body()))


def test_task_loss_refuses_the_problem_types_with_their_own_kernels(lib):
    loss, dl = Out(1, 1, torch.float32), Out(4, 2, torch.float32)
    logits, labels = torch.zeros(4, 2, device="cuda"), torch.zeros(4, dtype=torch.long, device="cuda")
    for problem in (L.PROBLEM_AUC, L.PROBLEM_TOKEN_CE, 9):
        rc = lib.gget_op_task_loss(P(logits), P(labels), None, problem, 4, 2, P(loss.buf), P(dl.buf), ST())
        assert rc == 2, (problem, rc)
    assert loss.untouched() and dl.untouched()


# ------------------------------------------------------------------------------------------------------------------ AUC surrogate
@pytest.mark.parametrize("B,num_neg,Cn,labels", params(R.AUC_CASES))
def test_auc_loss(lib, request, B, num_neg, Cn, labels):
    seed = R.AUC_SEED + B
    i = R.auc_case(B, num_neg, Cn, labels)
    idx = M.auc_pairs(i["labels"].numpy(), num_neg, seed)
    loss, dl, lists = Out(1, 1, torch.float32), Out(B, Cn, torch.float32), Out(2, B, torch.int32)
    logits, labels = dev(i["logits"]), dev(i["labels"])
    L.check(lib.gget_op_auc_loss(P(logits), P(labels), B, Cn, num_neg, seed, P(loss.buf), P(dl.buf), P(lists.buf), ST()))
    li = lists.body()
    n_pos = int((i["labels"] != 0).sum())
    assert bool((li[0, n_pos:] == -7).all()) and bool((li[1, B - n_pos:] == -7).all()), "wrote list entries past the two counts"
    finish("auc_loss", request.node.callspec.id, R.auc_check(i, idx, loss.body().view(-1), dl.body(), li[0, :n_pos], li[1, :B - n_pos]))


def test_auc_pair_limit_is_enforced_by_the_launcher(lib):
    """8192 pairs size the kernel's keys[] array in LDS: 8192 is accepted (B = 1024 positives x 8 would fill it), 8193 is error 2 from
    the launcher itself - nothing is launched, the outputs stay untouched."""
    B = 8193
    loss, dl, lists = Out(1, 1, torch.float32), Out(B, 2, torch.float32), Out(2, B, torch.int32)
    logits, labels = torch.zeros(B, 2, device="cuda"), torch.ones(B, dtype=torch.long, device="cuda")
    rc = lib.gget_op_auc_loss(P(logits), P(labels), B, 2, 1, 3, P(loss.buf), P(dl.buf), P(lists.buf), ST())
    assert rc == 2 and b"8192 pairs" in lib.gget_last_error(), (rc, lib.gget_last_error())
    assert loss.untouched() and dl.untouched() and lists.untouched()
    assert lib.gget_op_auc_loss(P(logits), P(labels), 4, 1, 1, 3, P(loss.buf), P(dl.buf), P(lists.buf), ST()) == 2   # (C = 1: no second column)
    assert loss.untouched() and dl.untouched() and lists.untouched()


# ------------------------------------------------------------------------------------------------------------------ MLP head
@pytest.mark.parametrize("B,Din,Dout,bias", params(R.HEAD_CASES))
def test_head_linear(lib, request, B, Din, Dout, bias):
    i = R.head_case(B, Din, Dout, bias)
    x, w, b = dev(i["x"]), dev(i["w"]), dev(i["bias"])
    a, y, y32 = Out(B, Din, torch.bfloat16), Out(B, Dout, torch.bfloat16), Out(B, Dout, torch.float32)
    L.check(lib.gget_op_head_linear_fwd(P(x), P(a.buf), P(w), P(b), P(y.buf), P(y32.buf), B, Din, Dout, 0, ST()))
    a_got = a.body()
    finish("head_linear_fwd", request.node.callspec.id, R.head_fwd_check(i, a_got, y.body(), y32.body()))
    dx, dw, dbias = Out(B, Din, torch.float32), Out(Dout, Din, torch.float32, i["dw0"]), Out(1, Dout, torch.float32, i["db0"]) if bias else None
    dy = dev(i["dy"])
    L.check(lib.gget_op_head_linear_bwd(P(dy), P(x), P(a.buf), P(w), P(dw.buf), P(dbias.buf if bias else None), P(dx.buf), B, Din,
                                        Dout, 0, ST()))
    finish("head_linear_bwd", request.node.callspec.id, R.head_bwd_check(i, a_got, dx.body(), dw.body(), dbias.body().view(-1) if bias else None))


@pytest.mark.parametrize("B,d", [(1, 64), (33, 768)], ids=["B1-d64", "B33-d768: three rounds of the column loop"])
def test_pool_and_scatter_rows(lib, request, B, d):
    """pool_rows gathers bit for bit; scatter_rows_f32 writes bf16(src[b]) to row pool_row[b] and to no other row."""
    g = R.gen(7000 + B)
    rows = 2 * B + 3
    hidden, pool_row = R.randn_bf16(g, rows, d), R.pool_sample(g, B, rows)
    out = Out(B, d, torch.bfloat16)
    hidden_d, pool_d = dev(hidden), dev(pool_row)
    L.check(lib.gget_op_pool_rows(P(hidden_d), P(pool_d), P(out.buf), B, d, ST()))
    finish("pool_rows", request.node.callspec.id, [R.held_equal("out", out.body(), hidden[pool_row.long()])])
    src = torch.randn(B, d, generator=g)
    dh = Out(rows, d, torch.bfloat16)
    src_d = dev(src)
    L.check(lib.gget_op_scatter_rows_f32(P(src_d), P(pool_d), P(dh.buf), B, d, ST()))
    got = dh.body()
    rest = torch.ones(rows, dtype=torch.bool)
    rest[pool_row.long()] = False
    assert bool((got[rest].view(torch.int16) == SENT16).all()), "scatter_rows_f32 wrote a row that is not in pool_row"
    finish("scatter_rows_f32", request.node.callspec.id, [R.held_equal("dhidden", got[pool_row.long()], src.to(torch.bfloat16))])
