"""The dropout / DropPath / LayerScale kernels with their masks ON, one launcher at a time through the C ABI (gget_op_ls_rmsnorm_fwd_drop,
gget_op_rmsnorm_bwd_ls_drop, gget_op_ls_fwd, gget_op_ls_bwd, gget_op_elem_dropout, gget_op_embed_fwd_drop, gget_op_embed_bwd_drop,
gget_op_head_linear_fwd_drop, gget_op_head_linear_bwd_drop): every output element against a float64 statement of the same operation on the
same bf16 / fp32 inputs and on the multipliers the numpy twins of the two counter hashes give (tests/_drop_ref.py: twins, references, bounds
and their derivation).  Outputs land in buffers pre-filled with NaN sentinels with pad rows behind them; accumulating outputs start from
known non-zero values; launch-menu keys are set through L.debug_menu, which restores them.  Every test also runs the masks-off call through
the new entry and holds it to the old entry's output - bit for bit, or, where fp32 atomics of several blocks meet in one replica, within the
bound two sums of the same terms can differ by - so that delegating the old entries is shown to change nothing."""
import ctypes as C
import importlib

import pytest
import torch

import _drop_ref as D
import _rows_ref as R
from _gpu_out import Out, P, ST, dev
from _util import record_error
from test_gpu_rows import Accum, params, tagged

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def lib():
    return L.load()


def finish(op, case, results):
    """Record max(err / bound) of the case - overall, and per bounded quantity over the case's settings - then fail on whatever was out of
    bound."""
    ratio, msgs = D.settle(results)
    record_error(f"drop_elementwise/{op}", case, ratio, 1.0)
    worst = {}
    for t in results:
        if isinstance(t, D.Bounded):
            q = t[0].split("] ")[-1]
            worst[q] = max(worst.get(q, 0.0), t[1])
    for q, r in worst.items():
        record_error(f"drop_elementwise/{op}/{q}", case, r, 1.0)
    assert not msgs, f"{op} {case}:\n" + "\n".join(msgs)


_ROW_MAPS = {}


class Masks:
    """The mask arguments of a setting with the row maps on the device.  The maps are module-lived: the argument tuples hold raw pointers,
    which must stay valid until the launch whatever becomes of the Masks object."""

    def __init__(self, m, lay):
        if lay["kind"] not in _ROW_MAPS:
            _ROW_MAPS[lay["kind"]] = (dev(lay["rows"]), dev(lay["row_b"]))
        self.m, (self.rows, self.row_b), self.S = m, _ROW_MAPS[lay["kind"]], lay["S"]

    def elem(self):
        on = self.m["elem_p"] > 0
        return self.m["elem_p"], self.m["elem_seed"], P(self.rows) if on else None

    def both(self):
        on = self.m["path_rate"] > 0
        return self.elem() + (self.m["path_rate"], self.m["path_seed"], self.S if on else 1, P(self.row_b) if on else None)


NO_ELEM = (0.0, 0, None)
NO_MASKS = NO_ELEM + (0.0, 0, 1, None)


def accum_layout(lib, d):
    copies, stride = C.c_int32(0), C.c_uint64(0)
    L.check(lib.gget_op_accum_layout(d, C.byref(copies), C.byref(stride)))
    assert copies.value >= 1 and stride.value >= d
    return copies.value, stride.value


def same_sum(name, new, old, init, tabs, T):
    """Two runs of one accumulating launch: replicas that several blocks add to with fp32 atomics need not agree bit for bit - both lie
    within the bound of the same sum."""
    bound = 2 * (2 * (T + 1) * R.U * (init.double().abs().sum(0) + tabs) + R.TINY)
    return R.held(name, new.double().sum(0), old.double().sum(0), bound)


# ------------------------------------------------------------------------------------------------------------------ fused forward
def run_ls_fused_fwd(lib, i, margs, old=False):
    T, d = i["T"], i["d"]
    res, yb, lm, w = dev(i["res"]), dev(i["y"]), dev(i["lam"]), dev(i["w"])
    out, xn, rstd = Out(T, d, BF), Out(T, d, BF), Out(T, 1, F32)
    if old:
        L.check(lib.gget_op_ls_rmsnorm_fwd(P(res), P(yb), P(lm), P(out.buf), P(w), P(xn.buf), P(rstd.buf), T, d, i["eps"], ST()))
    else:
        L.check(lib.gget_op_ls_rmsnorm_fwd_drop(P(res), P(yb), P(lm), P(out.buf), P(w), P(xn.buf), P(rstd.buf), T, d, i["eps"], *margs, ST()))
    return out.body(), xn.body(), rstd.body().view(-1)


@pytest.mark.parametrize("T,d,kind,names", params(D.LS_FWD_CASES + [D.LS_FWD_LONG]))
def test_ls_rmsnorm_fwd_drop(lib, request, T, d, kind, names):
    results = []
    for name in names:
        lay, m, em, keep = D.ls_masks(T, d, kind, name)
        i = D.ls_fwd_inputs(T, d, D.case_seed(T, d), lam=m["lam"])
        got = run_ls_fused_fwd(lib, i, Masks(m, lay).both())
        results += tagged(name, D.ls_fwd_check(i, em, keep, m["path_rate"], *got))
    i = D.ls_fwd_inputs(T, d, D.case_seed(T, d))
    new, old = run_ls_fused_fwd(lib, i, NO_MASKS), run_ls_fused_fwd(lib, i, None, old=True)
    results += tagged("masks off", [R.held_bits("out of the new entry is the old entry's", new[0], old[0]),
                                    R.held_bits("xn of the new entry is the old entry's", new[1], old[1]),
                                    R.held_equal("rstd of the new entry is the old entry's", new[2], old[2])])
    finish("ls_rmsnorm_fwd", request.node.callspec.id, results)


# ------------------------------------------------------------------------------------------------------------------ fused backward
def run_ls_fused_bwd(lib, i, margs, old=False, dlam=True):
    T, d = i["T"], i["d"]
    dy, x, w, rstd, dr, yb, lm = (dev(i[k]) for k in ("dy", "x", "w", "rstd", "dres", "y", "lam"))
    dx, dsc = Out(T, d, BF), Out(T, d, BF)
    dw = Accum(i["copies"], i["stride"], d, i["dw0"])
    dl = Accum(i["copies"], i["stride"], d, i["dlam0"]) if dlam else None
    args = (P(dy), P(x), P(w), P(rstd), P(dr), P(dx.buf), P(dw.buf), P(yb), P(lm), P(dsc.buf), P(dl.buf) if dl else None, T, d)
    if old:
        L.check(lib.gget_op_rmsnorm_bwd_ls(*args, ST()))
    else:
        L.check(lib.gget_op_rmsnorm_bwd_ls_drop(*args, *margs, ST()))
    return dx.body(), dw.replicas(), dsc.body(), dl.replicas() if dl else None


@pytest.mark.parametrize("T,d,wide,kind,names", params(D.LS_BWD_CASES + [D.LS_BWD_LONG]))
def test_rmsnorm_bwd_ls_drop(lib, request, T, d, wide, kind, names):
    copies, stride = accum_layout(lib, d)
    results = []
    with L.debug_menu({L.KEY_LS_NORM_BWD_WIDE: wide}):
        for name in names:
            lay, m, em, keep = D.ls_masks(T, d, kind, name)
            i = D.ls_bwd_inputs(T, d, D.case_seed(T, d), copies, lam=m["lam"])
            assert i["stride"] == stride
            results += tagged(name, D.ls_bwd_check(i, em, keep, *run_ls_fused_bwd(lib, i, Masks(m, lay).both())))
        i = D.ls_bwd_inputs(T, d, D.case_seed(T, d), copies)
        new, old = run_ls_fused_bwd(lib, i, NO_MASKS), run_ls_fused_bwd(lib, i, None, old=True)
    _, _, _, tabs = R.bwd_ref(i)
    labs = (old[0].double() * i["y"].double()).abs().sum(0)
    results += tagged("masks off", [R.held_bits("dx of the new entry is the old entry's", new[0], old[0]),
                                    R.held_bits("dsc of the new entry is the old entry's", new[2], old[2]),
                                    same_sum("dw of the new entry against the old entry's", new[1], old[1], i["dw0"], tabs, T),
                                    same_sum("dlam of the new entry against the old entry's", new[3], old[3], i["dlam0"], labs, T)])
    finish("rmsnorm_bwd_ls", request.node.callspec.id, results)


# ------------------------------------------------------------------------------------------------------------------ the unfused kernels
def run_ls_fwd(lib, i, margs):
    T, d = i["T"], i["d"]
    res, yb, lm = dev(i["res"]), dev(i["y"]), dev(i["lam"])
    out = Out(T, d, BF)
    L.check(lib.gget_op_ls_fwd(P(res), P(yb), P(lm), P(out.buf), T, d, *margs, ST()))
    return out.body()


@pytest.mark.parametrize("T,d,kind,names", params(D.UNFUSED_CASES + [D.UNFUSED_LONG]))
def test_ls_fwd(lib, request, T, d, kind, names):
    results = []
    for name in names:
        lay, m, em, keep = D.ls_masks(T, d, kind, name)
        i = D.ls_fwd_inputs(T, d, D.case_seed(T, d), lam=m["lam"])
        results += tagged(name, D.ls_out_check(i, em, keep, m["path_rate"], run_ls_fwd(lib, i, Masks(m, lay).both())))
    for lam in (True, False):      # masks off: the statement of _rows_ref, bit for bit
        i = D.ls_fwd_inputs(T, d, D.case_seed(T, d), lam=lam)
        results += tagged(f"masks off, {'lam' if lam else 'no lam'}",
                          [R.held_bits("out is bf16(res + bf16(lam * y))", run_ls_fwd(lib, i, NO_MASKS), R._ls_out(i))])
    finish("ls_fwd", request.node.callspec.id, results)


def run_ls_bwd(lib, i, margs, dlam=True):
    T, d = i["T"], i["d"]
    dy, yb, lm = dev(i["dy"]), dev(i["y"]), dev(i["lam"])
    dsc = Out(T, d, BF)
    dl = Accum(i["copies"], i["stride"], d, i["dlam0"]) if dlam else None
    L.check(lib.gget_op_ls_bwd(P(dy), P(yb), P(lm), P(dsc.buf), P(dl.buf) if dl else None, T, d, *margs, ST()))
    return dsc.body(), dl.replicas() if dl else None


@pytest.mark.parametrize("T,d,kind,names", params(D.UNFUSED_CASES + [D.UNFUSED_LONG]))
def test_ls_bwd(lib, request, T, d, kind, names):
    copies, stride = accum_layout(lib, d)
    results = []
    for name in names:
        lay, m, em, keep = D.ls_masks(T, d, kind, name)
        i = D.ls_bwd_inputs(T, d, D.case_seed(T, d), copies, lam=m["lam"], fused=False)
        assert i["stride"] == stride
        for dlam in (True, False):
            results += tagged(f"{name}, {'dlam' if dlam else 'no dlam accumulator'}",
                              D.scale_checks(i, em, keep, i["dy"], *run_ls_bwd(lib, i, Masks(m, lay).both(), dlam=dlam)))
    i = D.ls_bwd_inputs(T, d, D.case_seed(T, d), copies, fused=False)      # masks off: bf16(lam * dy), bit for bit
    dsc, dlam = run_ls_bwd(lib, i, NO_MASKS)
    one = torch.ones(T, d)
    results += tagged("masks off", [R.held_bits("dsc is bf16(lam * dy)", dsc, (i["lam"].float() * i["dy"].float()).to(BF))]
                      + D.scale_checks(i, one, one[:, 0], i["dy"], dsc, dlam))
    finish("ls_bwd", request.node.callspec.id, results)


PAIR_CASES = [(f"T{T}-d{d}-{kind}", (T, d, kind)) for d in (72, 768, 1032) for T, kind in ((35, "identity"), (D.VARLEN_T, "varlen"))]


@pytest.mark.parametrize("T,d,kind", params(PAIR_CASES))
def test_unfused_forward_is_the_fused_one(lib, request, T, d, kind):
    """ls_fwd + rmsnorm_fwd against ls_rmsnorm_fwd_drop on the same inputs and masks: out bit for bit."""
    lay, m, em, keep = D.ls_masks(T, d, kind, "both")
    i = D.ls_fwd_inputs(T, d, D.case_seed(T, d))
    ma = Masks(m, lay)
    fused = run_ls_fused_fwd(lib, i, ma.both())
    out = run_ls_fwd(lib, i, ma.both())
    xn, rstd, od, wd = Out(T, d, BF), Out(T, 1, F32), dev(out), dev(i["w"])
    L.check(lib.gget_op_rmsnorm_fwd(P(od), P(wd), P(xn.buf), P(rstd.buf), T, d, i["eps"], ST()))
    results = [R.held_bits("out of ls_fwd is out of the fused kernel", out, fused[0])]
    results += R._norm_checks(out, i["w"], i["eps"], xn.body(), rstd.body().view(-1), tag=" (rmsnorm_fwd of out)")
    finish("ls_fwd_pair", request.node.callspec.id, results)


BWD_PAIR_CASES = ([(f"chunk-{name}", (*args, 1)) for name, args in PAIR_CASES]
                  + [(f"ls4-T{T}-d768-{kind}", (T, 768, kind, 0)) for T, kind in ((35, "identity"), (D.VARLEN_T, "varlen"))])


@pytest.mark.parametrize("T,d,kind,wide", params(BWD_PAIR_CASES))
def test_unfused_backward_is_the_fused_one(lib, request, T, d, kind, wide):
    """rmsnorm_bwd_copies + ls_bwd against rmsnorm_bwd_ls_drop (the 16-byte-chunk form, and the 4-element-lane form at d = 768) on the
    same inputs and masks: the zero pattern of dsc identical, the values within the pair bound."""
    copies, stride = accum_layout(lib, d)
    lay, m, em, keep = D.ls_masks(T, d, kind, "both")
    i = D.ls_bwd_inputs(T, d, D.case_seed(T, d), copies)
    ma = Masks(m, lay)
    with L.debug_menu({L.KEY_LS_NORM_BWD_WIDE: wide}):
        fused = run_ls_fused_bwd(lib, i, ma.both())
    dy, x, w, rstd, dr = (dev(i[k]) for k in ("dy", "x", "w", "rstd", "dres"))
    dx, dw = Out(T, d, BF), Accum(copies, stride, d, i["dw0"])
    L.check(lib.gget_op_rmsnorm_bwd_copies(P(dy), P(x), P(w), P(rstd), P(dr), P(dx.buf), P(dw.buf), T, d, copies, stride, ST()))
    dxb = dx.body()
    dsc, dlam = run_ls_bwd(lib, dict(i, dy=dxb), ma.both())
    results = D.dsc_pair_check(i, em, keep, fused[2], dsc) + tagged("unfused", D.scale_checks(i, em, keep, dxb, dsc, dlam))
    finish("ls_bwd_pair", request.node.callspec.id, results)


# ------------------------------------------------------------------------------------------------------------------ elem_dropout
def run_drop(lib, i, stream, margs):
    x = Out(i["T"], i["n"], BF, i["x"])
    L.check(lib.gget_op_elem_dropout(P(x.buf), i["T"], i["n"], stream, *margs, ST()))
    return x.body()


@pytest.mark.parametrize("T,n,stream,kind", params(D.DROP_CASES + [D.DROP_LONG]))
def test_elem_dropout(lib, request, T, n, stream, kind):
    results = []
    i = D.drop_inputs(T, n, D.case_seed(T, n))
    for name in D.ELEM_SETTINGS if T < 1000 else ("elem",):
        lay, m, em = D.drop_masks(T, n, stream, kind, name)
        results += tagged(name, D.drop_check(i, em, run_drop(lib, i, stream, Masks(m, lay).elem())))
    results.append(R.held_bits("p = 0 leaves x as it was", run_drop(lib, i, stream, NO_ELEM), i["x"]))
    sent = Out(T, n, BF)
    L.check(lib.gget_op_elem_dropout(P(sent.buf), T, n, stream, *NO_ELEM, ST()))
    results.append(R.held_true("p = 0 writes nothing", sent.untouched(), "a buffer of sentinels was written with the dropout off"))
    finish("elem_dropout", request.node.callspec.id, results)


# ------------------------------------------------------------------------------------------------------------------ embedding
def run_embed_fwd(lib, i, DV, margs, old=False):
    out = Out(i["T"], i["d"], BF)
    args = (P(DV["ids"]), P(DV["emb"]), P(DV["gate"]), P(out.buf), i["T"], i["F"], i["ldF"], i["d"])
    L.check(lib.gget_op_embed_fwd(*args, ST()) if old else lib.gget_op_embed_fwd_drop(*args, *margs, ST()))
    return out.body()


def run_embed_bwd(lib, i, DV, margs, old=False):
    demb = Out(i["V"], i["d"], F32, i["demb0"])
    dgate = Out(i["F"], i["d"], F32, i["dgate0"]) if i["gate"] is not None else None
    args = (P(DV["ids"]), P(DV["dx"]), P(DV["emb"]), P(DV["gate"]), P(demb.buf), P(dgate.buf) if dgate else None, i["T"], i["F"], i["ldF"],
            i["d"], i["V"], i["pad_id"])
    L.check(lib.gget_op_embed_bwd(*args, ST()) if old else lib.gget_op_embed_bwd_drop(*args, *margs, ST()))
    return demb.body(), dgate.body() if dgate else None


@pytest.mark.parametrize("F,ldF,d,gated,kind", params(D.EMBED_CASES))
def test_embed_fwd_drop(lib, request, F, ldF, d, gated, kind):
    results = []
    for name in D.ELEM_SETTINGS:
        lay, m, em = D.embed_masks(F, d, kind, name)
        i = D.embed_inputs(lay["T"], F, ldF, d, gated, D.case_seed(F, d, gated))
        DV = {k: dev(i[k]) for k in ("ids", "emb", "gate")}
        results += tagged(name, D.embed_fwd_check(i, em, run_embed_fwd(lib, i, DV, Masks(m, lay).elem())))
    results.append(R.held_bits("masks off: out of the new entry is the old entry's", run_embed_fwd(lib, i, DV, NO_ELEM),
                               run_embed_fwd(lib, i, DV, None, old=True)))
    finish("embed_fwd", request.node.callspec.id, results)


@pytest.mark.parametrize("F,ldF,d,gated,kind", params(D.EMBED_CASES))
def test_embed_bwd_drop(lib, request, F, ldF, d, gated, kind):
    results = []
    for name in D.ELEM_SETTINGS:
        lay, m, em = D.embed_masks(F, d, kind, name)
        i = D.embed_inputs(lay["T"], F, ldF, d, gated, D.case_seed(F, d, gated))
        DV = {k: dev(i[k]) for k in ("ids", "dx", "emb", "gate")}
        ma = Masks(m, lay)
        with L.debug_menu({L.KEY_EMBED_SORTED: 0}):
            demb, dgate = run_embed_bwd(lib, i, DV, ma.elem())
        results += tagged(name, D.embed_bwd_check(i, em, demb, dgate))
        if name == "elem":          # un-gated V = 97 takes the count-matrix form WITHOUT a mask; with one the entry must choose the sorted form
            with L.debug_menu({L.KEY_EMBED_SORTED: 1}):
                forced, _ = run_embed_bwd(lib, i, DV, ma.elem())
            results += tagged(name, [D.embed_pair_check(i, em, demb, forced)])
    one = torch.ones(lay["T"], F, d)
    new, old = run_embed_bwd(lib, i, DV, NO_ELEM), run_embed_bwd(lib, i, DV, None, old=True)
    results += tagged("masks off", D.embed_bwd_check(i, one, *new)
                      + [D.embed_pair_check(i, one, new[0], old[0], name="demb of the new entry against the old entry's")])
    finish("embed_bwd", request.node.callspec.id, results)


# ------------------------------------------------------------------------------------------------------------------ MLP head
def run_head_fwd(lib, i, layer, margs, old=False):
    B, Din, Dout = i["B"], i["Din"], i["Dout"]
    x, w, b = dev(i["x"]), dev(i["w"]), dev(i["bias"])
    a, y, y32 = Out(B, Din, BF), Out(B, Dout, BF), Out(B, Dout, F32)
    args = (P(x), P(a.buf), P(w), P(b), P(y.buf), P(y32.buf), B, Din, Dout, layer)
    L.check(lib.gget_op_head_linear_fwd(*args, ST()) if old else lib.gget_op_head_linear_fwd_drop(*args, *margs, ST()))
    return a.body(), y.body(), y32.body()


def run_head_bwd(lib, i, a, layer, margs, old=False):
    B, Din, Dout = i["B"], i["Din"], i["Dout"]
    dy, x, w, av = dev(i["dy"]), dev(i["x"]), dev(i["w"]), dev(a)
    dx, dw, db = Out(B, Din, F32), Out(Dout, Din, F32, i["dw0"]), Out(1, Dout, F32, i["db0"])
    args = (P(dy), P(x), P(av), P(w), P(dw.buf), P(db.buf), P(dx.buf), B, Din, Dout, layer)
    L.check(lib.gget_op_head_linear_bwd(*args, ST()) if old else lib.gget_op_head_linear_bwd_drop(*args, *margs, ST()))
    return dx.body(), dw.body(), db.body().view(-1)


@pytest.mark.parametrize("B,Din,Dout,layer", params(D.HEAD_CASES))
def test_head_linear_fwd_drop(lib, request, B, Din, Dout, layer):
    results = []
    i = D.head_inputs(B, Din, Dout, D.case_seed(B, Din, Dout))
    for name in D.ELEM_SETTINGS:
        lay, m, em = D.head_masks(B, Din, layer, name)
        results += tagged(name, D.head_fwd_check(i, em, *run_head_fwd(lib, i, layer, Masks(m, lay).elem())))
    new, old = run_head_fwd(lib, i, layer, NO_ELEM), run_head_fwd(lib, i, layer, None, old=True)
    results += tagged("masks off", [R.held_bits("a of the new entry is the old entry's", new[0], old[0]),
                                    R.held_bits("y of the new entry is the old entry's", new[1], old[1]),
                                    R.held_equal("y32 of the new entry is the old entry's", new[2], old[2])])
    finish("head_linear_fwd", request.node.callspec.id, results)


@pytest.mark.parametrize("B,Din,Dout,layer", params(D.HEAD_CASES))
def test_head_linear_bwd_drop(lib, request, B, Din, Dout, layer):
    results = []
    i = D.head_inputs(B, Din, Dout, D.case_seed(B, Din, Dout))
    for name in D.ELEM_SETTINGS:
        lay, m, em = D.head_masks(B, Din, layer, name)
        a = D.head_fwd_fp32(i, em)[0]          # (the a of the CPU statement: the backward answers for itself)
        results += tagged(name, D.head_bwd_check(i, em, a, *run_head_bwd(lib, i, a, layer, Masks(m, lay).elem())))
    a = D.head_fwd_fp32(i, torch.ones(B, Din))[0]
    new, old = run_head_bwd(lib, i, a, layer, NO_ELEM), run_head_bwd(lib, i, a, layer, None, old=True)
    results += tagged("masks off", [R.held_equal(f"{q} of the new entry is the old entry's", n, o) for q, n, o in zip(("dx", "dw", "dbias"), new, old)])
    finish("head_linear_bwd", request.node.callspec.id, results)
