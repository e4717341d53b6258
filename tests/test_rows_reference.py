"""The references and bounds of tests/_rows_ref.py, checked on the CPU with the inputs the GPU test uses (tests/test_gpu_rows.py): an
fp32 statement of every operation with the kernel's rounding points stays inside its per-element bound (ratio < 1), and one planted
fault at a time - a row normalised with its neighbour's rstd, one swapped LDS plane of the weight-gradient reduction, a replica left out,
the pad columns inside the softmax sum, a weight indexed by the row - does not; every fault names the check that rejects it."""
import pytest
import torch

import _rows_ref as R

N_CU = 256      # (the device's on the GPU; here it only sizes the two cases around the 16-wave form's limit)


def params(cases):
    return [pytest.param(*args, id=name) for name, args in cases]


def passes(results):
    ratio, msgs = R.settle(results)
    assert not msgs, "\n".join(msgs)
    assert ratio < 1.0, ratio
    return ratio


def caught(results, where):
    msgs = R.settle(results)[1]
    assert msgs, "the planted fault went unnoticed"
    assert any(m.startswith(where) for m in msgs), (where, msgs)


def rows_of(T):
    return {-1: 64 * N_CU, -2: 64 * N_CU + 1}.get(T, T)


# ------------------------------------------------------------------------------------------------------------------ fp32 statements pass
@pytest.mark.parametrize("T,d", params(R.FWD_CASES))
def test_rmsnorm_forward_fp32_statement_is_inside_the_bounds(T, d):
    for scale in R.SCALES:
        i = R.fwd_case(T, d, scale)
        if T >= 3:
            assert not bool(i["x"][1].any()) and int((i["x"][2] != 0).sum()) == 1
        passes(R.rms_fwd_check(i, *R.rms_fwd_fp32(i)))
        for lam in (True, False):
            i = R.fwd_case(T, d, scale, fused=True, lam=lam)
            passes(R.ls_fwd_check(i, *R.ls_fwd_fp32(i)))


@pytest.mark.parametrize("form,T,d", params(R.BWD_CASES))
def test_rmsnorm_backward_fp32_statement_is_inside_the_bounds(form, T, d):
    for dres in (True, False):
        for copies in (1, 8):
            i = R.bwd_case(rows_of(T), d, dres, copies)
            passes(R.rms_bwd_check(i, *R.rms_bwd_fp32(i)))


@pytest.mark.parametrize("T,d", params(R.DET_CASES))
def test_rmsnorm_backward_fp32_statement_is_inside_the_bounds_at_the_reproducible_shapes(T, d):
    i = R.bwd_case(T, d, True)
    dx, dw = R.rms_bwd_fp32(i)
    passes(R.rms_bwd_check(i, dx, dw))
    passes(R.rms_bwd_check(i, None, dw))


@pytest.mark.parametrize("T,d,wide", params([c for c in R.LS_BWD_CASES if not c[1][2]]))
def test_fused_layerscale_backward_fp32_statement_is_inside_the_bounds(T, d, wide):
    for lam, dres in ((True, True), (False, False)) if T > 1000 else ((True, True), (True, False), (False, True), (False, False)):
        i = R.bwd_case(T, d, dres, 8, fused=True, lam=lam)
        passes(R.ls_bwd_check(i, *R.ls_bwd_fp32(i)))


@pytest.mark.parametrize("V,ld,generic", params(R.CE_GEOMETRIES[:6]))
def test_cross_entropy_fp32_statement_is_inside_the_bounds(V, ld, generic):
    i = R.ce_case(R.CE_ROWS, V, ld)
    x = i["logits"].float()
    assert bool((x[:, V:] == R.PAD_LOGIT).all()) and float(x[1, :V].min()) > 20 and float(x[2, :V].max()) < -20
    assert int(i["labels"][4]) == 0 and int(i["labels"][5]) == V - 1 and int(i["labels"][6]) == int(x[6, :V].argmax())
    for nd, mean, gamma, wts in R.ce_variants():
        n = R.ce_rows(i, nd)
        scale = R.ce_scale(n, mean, R.CE_SCALE_BASE)
        dl, s, lo = R.ce_fp32(i, n, gamma, wts, scale)
        passes(R.ce_check(i, n, gamma, wts, scale, dl, s, lo))


def test_cross_entropy_fp32_statement_is_inside_the_bounds_at_the_grid_cap():
    i = R.ce_case(R.CE_BIG_ROWS, 97, 104)
    assert R.ce_grid(R.CE_BIG_ROWS) == 2048 and R.ce_grid(R.CE_ROWS) == 3
    n = R.CE_BIG_ROWS - 37
    dl, s, lo = R.ce_fp32(i, n, 2.0, True, 1.0 / n)
    passes(R.ce_check(i, n, 2.0, True, 1.0 / n, dl, s, lo))


# ------------------------------------------------------------------------------------------------------------------ planted faults
def test_planted_faults_in_the_rmsnorm_forward_are_caught():
    i = R.fwd_case(37, 520, 1.0)
    y, rstd = R.rms_fwd_fp32(i)
    x, w = i["x"].float(), i["w"].float()
    caught(R.rms_fwd_check(i, (w * (x * rstd[:, None])).to(R.BF), rstd), "y is bf16(")          # y without its inner bf16 rounding
    wrong = y.clone()
    wrong[20] = (w * R.bf(x[20] * rstd[21])).to(R.BF)
    caught(R.rms_fwd_check(i, wrong, rstd), "y:")                                               # row 20 normalised with row 21's rstd
    caught(R.rms_fwd_check(i, y, rstd.roll(1)), "rstd")                                         # rstd written one row off
    last = y.clone()
    last[:, 512:] = y[:, 504:512]
    caught(R.rms_fwd_check(i, last, rstd), "y:")                                                # lane 0's second chunk = its first neighbour's
    i = R.fwd_case(37, 520, 1.0, fused=True)
    out, xn, rstd = R.ls_fwd_fp32(i)
    sloppy = (i["res"].float() + i["lam"].float() * i["y"].float()).to(R.BF)                    # LayerScale product not rounded to bf16
    caught(R.ls_fwd_check(i, sloppy, *R.rms_fwd_fp32(dict(i, x=sloppy))), "out is bf16(")
    pre = R.rms_fwd_fp32(dict(i, x=(i["res"].float() + R.bf(i["lam"].float() * i["y"].float()))))   # norm of the UNROUNDED residual stream
    assert not torch.equal(pre[0], xn)
    caught(R.ls_fwd_check(i, out, *pre), "y (of out) is bf16(")


def test_planted_faults_in_the_rmsnorm_backward_are_caught():
    i = R.bwd_case(70, 520, True, 8)
    dx, dw = R.rms_bwd_fp32(i)
    caught(R.rms_bwd_check(i, R._dx_fp32(i, mean_div=1024)[0], dw), "dx")                       # m over the padded chunk count 2 x 64 x 8
    nores = dx.clone()
    nores[69] = R._dx_fp32(dict(i, dres=None))[0][69]
    caught(R.rms_bwd_check(i, nores, dw), "dx")                                                 # dres dropped on the last row
    t = i["dy"].float() * (i["x"].float() * i["rstd"][:, None])
    short = dw.clone()
    short[(69 // 16) % 8] -= t[69]
    caught(R.rms_bwd_check(i, dx, short), "dw")                                                 # dw without the last row
    planes = dw.clone()
    c = 64                                                                                      # (lane 0's second chunk)
    planes[:, 8 * c:8 * c + 4], planes[:, 8 * c + 4:8 * c + 8] = dw[:, 8 * c + 4:8 * c + 8], dw[:, 8 * c:8 * c + 4]
    caught(R.rms_bwd_check(i, dx, planes), "dw")                                                # one chunk's two LDS planes swapped
    lost = dw.clone()
    lost[3] = i["dw0"][3]
    caught(R.rms_bwd_check(i, dx, lost), "dw")                                                  # replica 3 of 8 never added to
    caught(R.rms_bwd_check(i, None, short), "dw")                                               # (the same through the dw-only check)
    i = R.bwd_case(70, 72, True, 8, fused=True)
    dx, dw, dsc, dlam = R.ls_bwd_fp32(i)
    caught(R.ls_bwd_check(i, dx, dw, dx, dlam), "dsc is bf16(")                                 # dsc without lam
    caught(R.ls_bwd_check(i, dx, dw, dsc, dlam - (dx.float() * i["y"].float())[69] * (torch.arange(8) == 4)[:, None]), "dlam")
    caught(R.ls_bwd_check(i, dx, dw, dsc, R._replicas_fp32(i, i["dlam0"], i["dy"].float() * i["y"].float())), "dlam")   # dlam from dy, not dx


def test_planted_faults_in_the_cross_entropy_are_caught():
    i = R.ce_case(R.CE_ROWS, 97, 104)
    rows = R.CE_ROWS
    n, scale = rows, 1.0 / rows
    caught(R.ce_check(i, n, 0.0, False, scale, *R.ce_fp32(i, n, 0.0, False, scale, pad_in_sum=True)), "dlogits")      # pad columns in the sum
    caught(R.ce_check(i, n, 0.0, False, scale, *R.ce_fp32(i, n, 0.0, False, scale, pad_in_sum=True)), "loss_sum")
    caught(R.ce_check(i, n, 0.0, False, scale, *R.ce_fp32(i, n, 0.0, False, scale, label_shift=1)), "dlogits")        # label off by one
    nd = rows - 37
    caught(R.ce_check(i, nd, 0.0, False, 1.0 / nd, *R.ce_fp32(i, nd, 0.0, False, 1.0 / rows)), "dlogits")             # 1 / n_rows_cap
    caught(R.ce_check(i, nd, 0.0, False, 1.0 / nd, *R.ce_fp32(i, nd, 0.0, False, 1.0 / rows)), "loss_out")
    for gamma in (1.0, 2.0):
        caught(R.ce_check(i, n, gamma, False, scale, *R.ce_fp32(i, n, gamma, False, scale, focal_in_grad=False)), "dlogits")   # focal: loss only
    caught(R.ce_check(i, n, 0.0, True, scale, *R.ce_fp32(i, n, 0.0, True, scale, weight_by_row=True)), "dlogits")     # weight by row
    caught(R.ce_check(i, n, 0.0, True, scale, *R.ce_fp32(i, n, 0.0, True, scale, weight_by_row=True)), "loss_sum")
    caught(R.ce_check(i, n, 0.0, False, scale, *R.ce_fp32(i, n, 0.0, False, scale, zero_pad=False)), "dlogits")       # pad columns unwritten
    dl, s, lo = R.ce_fp32(i, n, 0.0, False, scale)
    caught(R.ce_check(i, n, 0.0, False, scale, dl, s, lo * rows), "loss_out")                                         # loss_out without the scale
