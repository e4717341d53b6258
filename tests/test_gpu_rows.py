"""The RMSNorm and cross-entropy kernel families, one launcher at a time through the C ABI (gget_op_rmsnorm_fwd, gget_op_rmsnorm_bwd_copies,
gget_op_rmsnorm_dw, gget_op_ls_rmsnorm_fwd, gget_op_rmsnorm_bwd_ls, gget_op_ce_full), every output element against a float64 statement of
the same operation on the same bf16 / fp32 inputs (tests/_rows_ref.py: references, bounds and their derivation).  Outputs land in buffers
pre-filled with NaN sentinels with pad rows behind them; accumulating outputs start from known non-zero values; the pad columns of the
logits hold +60.  The shapes are the smallest that reach each launch form; the form is named next to the case, and launch-menu keys are
set through L.debug_menu, which restores them."""
import ctypes as C
import importlib
import itertools

import pytest
import torch

import _rows_ref as R
from _gpu_out import PAD_ROWS, SENT16, SENT32, Out, P, ST, dev
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def lib():
    return L.load()


def params(cases):
    return [pytest.param(*args, id=name) for name, args in cases]


def tagged(tag, results):
    return [type(t)((f"[{tag}] {t[0]}", t[1], None if t[2] is None else f"[{tag}] {t[2]}")) for t in results]


def finish(op, case, results):
    """Record max(err / bound) of the case - overall, and per bounded quantity over the case's variants - then fail on whatever was out
    of bound."""
    ratio, msgs = R.settle(results)
    record_error(f"rows_elementwise/{op}", case, ratio, 1.0)
    worst = {}
    for t in results:
        if isinstance(t, R.Bounded):          # (the bit-for-bit and the yes / no checks have no ratio)
            q = t[0].split("] ")[-1]
            worst[q] = max(worst.get(q, 0.0), t[1])
    for q, r in worst.items():
        record_error(f"rows_elementwise/{op}/{q}", case, r, 1.0)
    assert not msgs, f"{op} {case}:\n" + "\n".join(msgs)


class Accum:
    """fp32 accumulator replicas [copies][stride] in a sentinel buffer; the first d columns of every replica start from `init`."""

    def __init__(self, copies, stride, d, init):
        self.copies, self.stride, self.d = copies, stride, d
        self.buf = torch.full(((copies + PAD_ROWS) * stride,), SENT32, dtype=torch.int32, device="cuda").view(F32)
        self.buf[:copies * stride].view(copies, stride)[:, :d] = init.cuda()

    def replicas(self):
        """[copies, d] on the CPU, after checking that the columns d.. of every replica and the rows behind the last are as they were."""
        torch.cuda.synchronize()
        n = self.copies * self.stride
        assert bool((self.buf[n:].view(torch.int32) == SENT32).all()), "wrote behind the last accumulator replica"
        body = self.buf[:n].view(self.copies, self.stride)
        assert bool((body[:, self.d:].view(torch.int32) == SENT32).all()), f"wrote columns past d = {self.d} of an accumulator replica"
        return body[:, :self.d].cpu()


def n_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("T,d", params(R.FWD_CASES))
def test_rmsnorm_fwd(lib, request, T, d):
    results = []
    for scale in R.SCALES:
        i = R.fwd_case(T, d, scale)
        x, w = dev(i["x"]), dev(i["w"])
        y, rstd = Out(T, d, BF), Out(T, 1, F32)
        L.check(lib.gget_op_rmsnorm_fwd(P(x), P(w), P(y.buf), P(rstd.buf), T, d, i["eps"], ST()))
        results += tagged(f"scale {scale:g}", R.rms_fwd_check(i, y.body(), rstd.body().view(-1)))
    finish("rmsnorm_fwd", request.node.callspec.id, results)


@pytest.mark.parametrize("T,d", params(R.FWD_CASES))
def test_ls_rmsnorm_fwd(lib, request, T, d):
    results = []
    for scale, lam in itertools.product(R.SCALES, (True, False)):
        i = R.fwd_case(T, d, scale, fused=True, lam=lam)
        res, yb, lm, w = dev(i["res"]), dev(i["y"]), dev(i["lam"]), dev(i["w"])
        out, xn, rstd = Out(T, d, BF), Out(T, d, BF), Out(T, 1, F32)
        L.check(lib.gget_op_ls_rmsnorm_fwd(P(res), P(yb), P(lm), P(out.buf), P(w), P(xn.buf), P(rstd.buf), T, d, i["eps"], ST()))
        results += tagged(f"scale {scale:g}, {'lam' if lam else 'no lam'}", R.ls_fwd_check(i, out.body(), xn.body(), rstd.body().view(-1)))
    finish("ls_rmsnorm_fwd", request.node.callspec.id, results)


# ------------------------------------------------------------------------------------------------------------------ backward
def run_bwd(lib, i, dx_too=True):
    """(dx or None, dw replicas) of gget_op_rmsnorm_bwd_copies, or of gget_op_rmsnorm_dw (dx_too = False)."""
    T, d = i["T"], i["d"]
    dy, x, w, rstd, dres = dev(i["dy"]), dev(i["x"]), dev(i["w"]), dev(i["rstd"]), dev(i["dres"])
    dw = Accum(i["copies"], i["stride"], d, i["dw0"])
    if not dx_too:
        L.check(lib.gget_op_rmsnorm_dw(P(dy), P(x), P(rstd), P(dw.buf), T, d, i["copies"], i["stride"], ST()))
        return None, dw.replicas()
    dx = Out(T, d, BF)
    L.check(lib.gget_op_rmsnorm_bwd_copies(P(dy), P(x), P(w), P(rstd), P(dres), P(dx.buf), P(dw.buf), T, d, i["copies"], i["stride"], ST()))
    return dx.body(), dw.replicas()


@pytest.mark.parametrize("form,T,d", params(R.BWD_CASES))
def test_rmsnorm_bwd(lib, request, form, T, d):
    T = {-1: 64 * n_cu(), -2: 64 * n_cu() + 1}.get(T, T)
    results = []
    with L.debug_menu({L.KEY_RMS_WIDE: 0 if form == "4wave" else 1, L.KEY_DETERMINISTIC: 0}):
        for dres, copies in itertools.product((True, False), (1, 8)):
            i = R.bwd_case(T, d, dres, copies)
            tag = f"{'dres' if dres else 'no dres'}, copies {copies}"
            dx, dw = run_bwd(lib, i)
            results += tagged(tag, R.rms_bwd_check(i, dx, dw))
            _, dw_only = run_bwd(lib, i, dx_too=False)
            results += tagged(tag + ", rmsnorm_dw", R.rms_bwd_check(i, None, dw_only) + [R.dw_pair_check(i, dw_only, dw)])
    finish("rmsnorm_bwd", request.node.callspec.id, results)


@pytest.mark.parametrize("T,d", params(R.DET_CASES))
def test_rmsnorm_bwd_reproducible_mode(lib, request, T, d):
    """KEY_DETERMINISTIC = 1: per-block partials summed in block order by ordered_colsum_kernel.  Two calls give the same bits, and the
    weight-gradient-only kernel leaves the bits of the full backward's 4-wave form."""
    results = []
    # (the 16-wave form takes d <= 1024 and T <= 64 n_cu; past that KEY_RMS_WIDE = 1 reaches the 4-wave form again: run once)
    for wide in ((0, 1) if d <= 1024 and T <= 64 * n_cu() else (0,)):
        with L.debug_menu({L.KEY_RMS_WIDE: wide, L.KEY_DETERMINISTIC: 1}):
            for copies in ((1, 8) if T <= 1040 else (1,)):
                i = R.bwd_case(T, d, True, copies)
                tag = f"{'16-wave' if wide else '4-wave'} form, copies {copies}"
                dx, dw = run_bwd(lib, i)
                dx2, dw2 = run_bwd(lib, i)
                _, dw_only = run_bwd(lib, i, dx_too=False)
                res = R.rms_bwd_check(i, dx, dw) + R.rms_bwd_check(i, None, dw_only)
                res += [R.held_equal("dx of a second call", dx2, dx), R.held_equal("dw of a second call", dw2, dw),
                        R.held_equal("replicas 1.. keep their initial values", dw[1:], i["dw0"][1:])]
                if not wide:
                    res.append(R.held_equal("dw of rmsnorm_dw is the full backward's, bit for bit", dw_only, dw))
                results += tagged(tag, res)
    finish("rmsnorm_bwd_reproducible", request.node.callspec.id, results)


@pytest.mark.parametrize("T,d,wide", params(R.LS_BWD_CASES))
def test_rmsnorm_bwd_ls(lib, request, T, d, wide):
    copies, stride = C.c_int32(0), C.c_uint64(0)
    L.check(lib.gget_op_accum_layout(d, C.byref(copies), C.byref(stride)))
    copies, stride = copies.value, stride.value
    assert copies >= 1 and stride >= d
    combos = ((True, True), (False, False)) if T > 1000 else tuple(itertools.product((True, False), (True, False)))
    results = []
    with L.debug_menu({L.KEY_LS_NORM_BWD_WIDE: wide}):
        for lam, dres in combos:
            i = R.bwd_case(T, d, dres, copies, fused=True, lam=lam)
            dy, x, w, rstd, dr, yb, lm = (dev(i[k]) for k in ("dy", "x", "w", "rstd", "dres", "y", "lam"))
            dx, dsc = Out(T, d, BF), Out(T, d, BF)
            dw = Accum(copies, stride, d, i["dw0"])
            dlam = Accum(copies, stride, d, i["dlam0"]) if (lam or dres) else None       # (no lam, no dres: no dlam accumulator either)
            L.check(lib.gget_op_rmsnorm_bwd_ls(P(dy), P(x), P(w), P(rstd), P(dr), P(dx.buf), P(dw.buf), P(yb), P(lm), P(dsc.buf),
                                               P(dlam.buf) if dlam else None, T, d, ST()))
            results += tagged(f"{'lam' if lam else 'no lam'}, {'dres' if dres else 'no dres'}",
                              R.ls_bwd_check(i, dx.body(), dw.replicas(), dsc.body(), dlam.replicas() if dlam else None))
    finish("rmsnorm_bwd_ls", request.node.callspec.id, results)


# ------------------------------------------------------------------------------------------------------------------ cross-entropy
def run_ce(lib, i, D, nd, mean, gamma, wts, form, ref=None):
    """One launch of gget_op_ce_full on the device copies D of the inputs i; returns the checks."""
    rows, V, ld = i["rows"], i["V"], i["ld"]
    n = R.ce_rows(i, nd)
    scale = R.ce_scale(n, mean, R.CE_SCALE_BASE)
    grid = R.ce_grid(rows)
    cap = {"parts": grid + 2, "parts-cap-short": grid - 1, "no-parts-buffer": 0, "parts-key-off": grid + 2}[form]
    part = Out(1, max(cap, 1), F32) if form != "no-parts-buffer" else None
    n_dev = torch.tensor([nd], dtype=torch.int32, device="cuda") if nd is not None else None
    dl, loss_sum, loss_out = Out(rows, ld, BF), Out(1, 1, F32, torch.tensor([123.0])), Out(1, 1, F32)
    with L.debug_menu({L.KEY_CE_PARTS: 0 if form == "parts-key-off" else 1}):
        L.check(lib.gget_op_ce_full(P(D["logits"]), ld, P(D["labels"]), P(D["sel_tok"]) if wts else None, P(D["sample_wgt"]) if wts else None,
                                    i["S"] if wts else 1, P(n_dev), rows, V, P(loss_sum.buf), P(dl.buf), R.CE_SCALE_BASE, mean, P(loss_out.buf),
                                    gamma, P(part.buf) if part else None, cap, ST()))
    body = dl.body()
    out = R.ce_check(i, n, gamma, wts, scale, body, loss_sum.body().view(-1), loss_out.body().view(-1), ref=ref)
    out.append(R.held_true("rows past the count", bool((body[n:].view(torch.int16) == SENT16).all()), "a row at or past n_rows was written"))
    if part is not None:
        vec = ld % 8 == 0 and ld <= 2048 and not L.debug_get(L.KEY_CE_GENERIC)
        pb = part.body().view(-1)
        if form == "parts" and vec:
            ok = bool(torch.isfinite(pb[:grid]).all()) and bool((pb[grid:].view(torch.int32) == SENT32).all())
            out.append(R.held_true("loss_part", ok, f"expected one partial per block in the first {grid} slots and nothing behind them"))
            # (the finalising launch's fixed-order sum of the partials is loss_sum, to the roundings of a `grid`-term sum)
            out.append(R.held("loss_part sum", pb[:grid].double().sum(), loss_sum.body().view(-1)[0],
                              grid * R.U * pb[:grid].double().abs().sum() + R.TINY))
        else:
            out.append(R.held_true("loss_part", bool((pb.view(torch.int32) == SENT32).all()), "the atomic form must leave loss_part alone"))
    return out


@pytest.mark.parametrize("V,ld,generic", params(R.CE_GEOMETRIES))
def test_cross_entropy(lib, request, V, ld, generic):
    i = R.ce_case(R.CE_ROWS, V, ld)
    D = {k: dev(i[k]) for k in ("logits", "labels", "sel_tok", "sample_wgt")}
    results = []
    with L.debug_menu({L.KEY_CE_GENERIC: generic}):
        for nd, mean, gamma, wts in R.ce_variants():
            n = R.ce_rows(i, nd)
            ref = R.ce_ref(i, n, gamma, wts, R.ce_scale(n, mean, R.CE_SCALE_BASE))
            for form in R.CE_LOSS_FORMS:
                tag = f"n_rows_dev {nd}, mean_over_rows {mean}, gamma {gamma:g}, {'weights' if wts else 'no weights'}, {form}"
                results += tagged(tag, run_ce(lib, i, D, nd, mean, gamma, wts, form, ref=ref))
    finish("cross_entropy", request.node.callspec.id, results)


def test_cross_entropy_grid_at_its_cap(lib, request):
    """rows = 65 541 > 2048 blocks x 32 rows: every wave takes its rows in more than one grid-stride trip."""
    V, ld = 97, 104
    i = R.ce_case(R.CE_BIG_ROWS, V, ld)
    assert R.ce_grid(i["rows"]) == 2048
    D = {k: dev(i[k]) for k in ("logits", "labels", "sel_tok", "sample_wgt")}
    results = []
    for nd, mean, gamma, wts, form in ((None, 1, 2.0, True, "parts"), (R.CE_BIG_ROWS - 37, 0, 0.0, False, "parts-cap-short")):
        results += tagged(f"n_rows_dev {nd}, mean_over_rows {mean}, gamma {gamma:g}, {form}", run_ce(lib, i, D, nd, mean, gamma, wts, form))
    finish("cross_entropy", f"V{V}-ld{ld}-rows{R.CE_BIG_ROWS}: grid at its 2048 cap", results)
