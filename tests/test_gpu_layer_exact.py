"""The fused attention + o-projection kernels through the C ABI (default launch menu): every element of attn_out, lse, x_mid, rstd, xn of
gget_op_attn_oproj_fwd and of dx_mid, the dw replicas, dattn_long and dq, dk, dv of gget_op_attn_oproj_bwd against the float64 statements
of tests/_layer_ref.py under their bounds (statements, bounds and their derivation are there; tests/test_layer_ref.py holds them to a
correct fp32 statement, to planted faults and to a cap on vacuous bounds).  Outputs go into NaN-sentinel buffers with guard rows behind
them (tests/_gpu_out.py): every row of a sample must be written, no other row may be; the pad rows hold what the weight-gradient GEMMs
rely on.  Every case asserts *taken == 1.  The backward is handed the lse gget_op_attn_fwd wrote for the same q | k | v.

Cases (tests/_layer_ref.py) and what they reach:
 forward   H 2 | 4 | 8 | 12, B = 2 H + 1, S = 32 (lens 32, 17, 29, 1, ...)   attn_oproj_fwd_kernel<H>: every K-step start (5 b) mod 2 H, padded and
                                                                            var-len layout, "unit" and "cancelling" residuals
           S = 24 padded; S = 8, B = 1, one token                           dead rows of the tile; a sample of one row
 backward  the same geometries, RoPE tables or none, copies 1 | 4 | B + 3   attn_oproj_bwd_kernel<H>: phases A, B, C; the replica of sample b
           (Wo with four terms per element, or dense with exact sums:       (dattn of a one-tile sample never reaches memory; _layer_ref
           the dO the kernel formed is then known to the bit)               sparse_wo says what a dense random weight would leave of the bounds)
           var-len S = 40 | 64, H 2 | 12, lens 1 .. 64 mixed                attn_oproj_bwd_long<H> + attn_bwd_long_kernel beside the one-tile
                                                                            path; the tail zeroing of the last long (:1710) / short (:1734) sample
           B = 70 with 40 long samples, B = 40 with 3, through the _list    attn_bwd_long_kernel walking the engine's long_list (a block takes a
           entries and gget_op_varlen_plan's list                           second item / blocks without one): bounds, and the bits of long_list = NULL
           reproducible mode (menu key 4)                                   one zeroed row per sample + k_ordered_colsum: equal bits twice, dw in copy 0
"""
import ctypes as C
import importlib

import pytest
import torch

import _attn_out_ref as A
import _heads_ref as H
import _layer_ref as Y
from _gpu_out import Out, P, ST, dev
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
FWD, BWD, LIST, DET = Y.forward_cases(), Y.backward_cases(), Y.list_cases(), Y.det_cases()


@pytest.fixture(scope="module")
def lib():
    return L.load()


def ids(cs):
    return [c["id"] for c in cs]


def finish(cid, results):
    for name, ratio, _ in results:
        if name in Y.BOUNDED:
            record_error(f"layer_exact/{cid}", f"{name}_worst_ratio", ratio, 1.0)
            print(f"layer_exact/{cid}: {name} max err / bound = {ratio:.4f}")
    msgs = H.settle(results)[1]
    assert not msgs, f"{cid}:\n" + "\n".join(msgs)


class Staged:
    """The device side of a case: the layout's index vectors, the packed weight, and (backward) the inputs and the forward's lse."""

    def __init__(self, lib, ly, backward):
        self.ly, pr = ly, ly.pr
        B, S, Hn, d = ly.B, ly.S, ly.Hn, ly.d
        self.key_len = torch.tensor(ly.c["lens"], dtype=I32).cuda()
        self.row_base = torch.tensor(ly.first, dtype=I32).cuda() if ly.varlen else None
        self.qkv, self.nw = dev(ly.buf(pr.qkv)), dev(ly.nw)
        wo = dev(ly.wo)
        self.wo_f, self.wo_b = torch.empty_like(wo), torch.empty_like(wo)
        L.check(lib.gget_op_pack_wo(P(wo), 0, P(self.wo_f), P(self.wo_b), d, 1, ST()))
        if not backward:
            self.x_in = dev(ly.buf(ly.x_in_g))
            return
        self.x_mid, self.dxn, self.dres, self.rstd = (dev(ly.buf(t)) for t in (ly.x_mid_g, ly.dxn_g, ly.dres_g, ly.rstd_g))
        tab = pr.rope is not None
        self.cos, self.sin, self.pos = (pr.cos.cuda(), pr.sin.cuda(), pr.pos.cuda()) if tab else (None, None, None)
        # lse (and out) of the attention on these q | k | v: the stand-alone forward on the padded grid, lse keeps its [B,H,S] indexing
        out_p = torch.zeros(B * S, d, dtype=BF16, device="cuda")
        self.lse = torch.zeros(B, Hn, S, dtype=F32, device="cuda")
        L.check(lib.gget_op_attn_fwd(P(dev(pr.qkv)), P(self.key_len), P(out_p), P(self.lse), B, S, Hn, pr.causal, None, None, None, pr.p,
                                     pr.dseed, ST()))
        torch.cuda.synchronize()
        self.out_p = out_p.cpu()
        self.lse_cpu = self.lse.cpu()


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("c", FWD, ids=ids(FWD))
def test_fused_forward_per_element(lib, c):
    ly = Y.Layer(c)
    st, pr = Staged(lib, ly, False), ly.pr
    attn, x_mid, xn = (Out(ly.t_rows, ly.d, BF16) for _ in range(3))
    rstd, lse = Out(ly.t_rows, 1, F32), Out(ly.B * ly.Hn, ly.S, F32)
    taken = C.c_int32(0)
    L.check(lib.gget_op_attn_oproj_fwd(P(st.qkv), P(st.key_len), P(st.row_base), P(attn.buf), P(lse.buf), P(st.wo_f), P(st.x_in), P(x_mid.buf),
                                       P(st.nw), P(xn.buf), P(rstd.buf), ly.B, ly.S, ly.Hn, pr.causal, Y.EPS, pr.p, pr.dseed, ST(), C.byref(taken)))
    assert taken.value == 1, "the fused attention + o-projection form was not taken"
    finish(c["id"], Y.forward_check(ly, attn.body(), lse.body().view(ly.B, ly.Hn, ly.S), x_mid.body(), xn.body(), rstd.body().view(-1)))


# ------------------------------------------------------------------------------------------------------------------ backward
def run_backward(lib, st, long_list=False):
    """gget_op_attn_oproj_bwd, or the _list entry (long_list: None or a device tensor): dx_mid, dw, dattn_long, dqkv on the CPU."""
    ly, pr = st.ly, st.ly.pr
    d = ly.d
    dx_mid, dattn, dqkv = Out(ly.t_rows, d, BF16), Out(ly.t_rows, d, BF16), Out(ly.t_rows, 3 * d, BF16)
    dw = Out(ly.copies + 2, ly.stride, F32, init=ly.dw_start())
    taken = C.c_int32(0)
    args = [P(st.dxn), P(st.x_mid), P(st.nw), P(st.rstd), P(st.dres), P(dx_mid.buf), P(dw.buf), ly.copies, ly.stride, P(st.wo_b), P(st.qkv),
            P(st.lse), P(st.key_len), P(st.row_base), P(dqkv.buf), ly.B, ly.S, ly.Hn, pr.causal, P(st.cos), P(st.sin), P(st.pos), pr.p, pr.dseed,
            ly.t_rows, ST(), C.byref(taken), P(dattn.buf)]
    if long_list is False:
        L.check(lib.gget_op_attn_oproj_bwd(*args))
    else:
        L.check(lib.gget_op_attn_oproj_bwd_list(*args, P(long_list)))
    assert taken.value == 1, "the fused backward was not taken"
    return dx_mid.body(), dw.body(), dattn.body(), dqkv.body()


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int16 if x.dtype == BF16 else I32), y.view(torch.int16 if y.dtype == BF16 else I32)) for x, y in zip(a, b))


@pytest.mark.parametrize("c", BWD, ids=ids(BWD))
def test_fused_backward_per_element(lib, c):
    ly = Y.Layer(c)
    st = Staged(lib, ly, True)
    finish(c["id"], Y.backward_check(ly, st.lse_cpu, *run_backward(lib, st)))


def plan_list(lib, ly):
    """long_list as the engine gets it: gget_op_varlen_plan into a zeroed buffer."""
    B, S, t_rows = ly.B, ly.S, ly.t_rows
    z = lambda n, dt=I32: torch.zeros(n, dtype=dt, device="cuda")          # noqa: E731
    tok = torch.full((B, S, 1), 5, dtype=torch.int64, device="cuda")
    key_len = torch.tensor(ly.c["lens"], dtype=I32).cuda()
    ll = z(3 * B + 1)
    L.check(lib.gget_op_varlen_plan(P(tok), 1, 1, None, P(key_len), None, P(z(B + 1)), P(z(t_rows, torch.int64)), P(z(t_rows, torch.int64)),
                                    P(z(t_rows)), P(z(B * S)), P(z(t_rows)), P(z(3)), B, S, ly.n, t_rows, 0, P(ll), ST()))
    torch.cuda.synchronize()
    assert torch.equal(ll.cpu(), Y.long_list_of(ly.c)), "gget_op_varlen_plan wrote another list than the statement's"
    return ll


@pytest.mark.parametrize("c", LIST, ids=ids(LIST))
def test_list_driven_long_launch(lib, c):
    """Both _list entries with the engine's long_list: under the bounds, and the bits of the same call with long_list = NULL."""
    ly = Y.Layer(c)
    st, pr = Staged(lib, ly, True), ly.pr
    ll = plan_list(lib, ly)
    listed, plain = run_backward(lib, st, ll), run_backward(lib, st, None)
    results = Y.backward_check(ly, st.lse_cpu, *listed)
    results.append(H.held_true("gget_op_attn_oproj_bwd_list: the bits of long_list = NULL", same_bits(listed, plain), "an output differs"))
    assert same_bits(plain, run_backward(lib, st)), "gget_op_attn_oproj_bwd_list(NULL) differs from gget_op_attn_oproj_bwd"
    # the stand-alone attention backward on the same layout, the problem's own dout
    out, dout = dev(ly.buf(st.out_p)), dev(ly.buf(pr.dout))
    got = []
    for lst in (ll, None):
        dqkv, delta = Out(ly.t_rows, 3 * ly.d, BF16), Out(ly.B * ly.Hn, ly.S, F32)
        L.check(lib.gget_op_attn_bwd_varlen_list(P(st.qkv), P(out), P(dout), P(st.lse), P(st.key_len), P(st.row_base), P(dqkv.buf), P(delta.buf),
                                                 ly.B, ly.S, ly.Hn, pr.causal, P(st.cos), P(st.sin), P(st.pos), 1, pr.p, pr.dseed, ST(), P(lst)))
        got.append(dqkv.body())
    results += [(f"attn_bwd_varlen_list: {r[0]}",) + tuple(r[1:]) for r in
                A.backward_check(pr, ly.grid(got[0]), st.lse_cpu, st.out_p, False, pad_zero=False)]
    results.append(H.held_true("gget_op_attn_bwd_varlen_list: no row behind the last sample is written", Y.intact(got[0][ly.n:]), "a pad row was written"))
    results.append(H.held_true("gget_op_attn_bwd_varlen_list: the bits of long_list = NULL", same_bits(got[:1], got[1:]), "dqkv differs"))
    for name, ratio, _ in results:
        if name.startswith("attn_bwd_varlen_list: d"):
            record_error(f"layer_exact/{c['id']}", f"varlen_list_{name[-2:]}_worst_ratio", ratio, 1.0)
    finish(c["id"], results)


@pytest.mark.parametrize("c", DET, ids=ids(DET))
def test_reproducible_mode(lib, c):
    """KEY_DETERMINISTIC: two calls give identical bits in every output; dw under its bound in copy 0, the other copies untouched."""
    ly = Y.Layer(c)
    st = Staged(lib, ly, True)
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):
        one, two = run_backward(lib, st), run_backward(lib, st)
    results = Y.backward_check(ly, st.lse_cpu, *one, det=True)
    results.append(H.held_true("reproducible mode: two calls give the same bits", same_bits(one, two), "an output differs between two calls"))
    results.append(H.held_true("reproducible mode: the copies behind the first are untouched",
                               torch.equal(one[1][1:ly.copies, :ly.d], ly.dw0[1:]), "a replica other than the first changed"))
    finish(c["id"], results)
