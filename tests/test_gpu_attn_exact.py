"""Attention output, log-sum-exp and gradients of every attention kernel of csrc/attention.hip through the C ABI (default launch menu, no
switches): every element of out, lse, dq, dk, dv on the rows that hold a token against the float64 statement of tests/_attn_out_ref.py
under its bound (statement, bounds and their derivation are there; tests/test_attn_out_ref.py holds them to a correct fp32 statement,
to planted faults and to a cap on vacuous bounds).  Buffers are pre-filled with a NaN sentinel: every real row must be written, rows
behind the buffers not; pad rows of dqkv hold what the weight-gradient GEMM relies on (exact zeros on the padded grid, untouched rows
behind the last sample of the var-len layout).  The backward is handed the out and lse the forward entry of the same family wrote.

Cases (tests/_attn_out_ref.py forward_cases / backward_cases; kinds "unit" and "rising" everywhere, "peaked" at S <= 72; both masks and
p in {0, 0.1} without the full product) and the kernels they reach:

 forward, gget_op_attn_fwd                 S 8 (1) | 32 (32, 17, 1) | 40 (33, 40)                  attn_fwd_kernel<1>
                                           S 64 (64, 31) | 72 (65, 72)                             attn_fwd_kernel<2>
                                           S 160 (160, 129, 97)                                    attn_fwd_kernel<4>
                                           S 256 (255) | 320 (320, 129) | 520 causal               attn_fwd64_kernel
                                           S 520 (520, 263), no mask, p = 0 / 0.1                  attn_fwd_dense_kernel<false / true>
                                           S 32, H = 12                                            attn_fwd_kernel<1>, grid y = 12
                                           S 40 | 264 with RoPE on load                            attn_fwd_kernel<1> | <4>
          gget_op_attn_fwd_varlen          S 40 (40, 33, 1) | 64 (64, 32, 31) | 64 (47, 1, 33)     attn_fwd_rows64_kernel
                                           S 24 | 72 | 160 | 320 | 520                             the kernels above through row_base
          gget_op_attn_fwd_ranges          S 40 | 64 | 160 | 320                                   PK = true of attn_fwd_kernel<1 / 2 / 4>, attn_fwd64_kernel
          gget_op_attn_oproj_fwd           S <= 32, H 2 | 4 | 8 | 12 (attn_out and lse here; x_mid,  attn_oproj_fwd_kernel<H> (*taken asserted)
                                           xn, rstd and the fused backward gget_op_attn_oproj_bwd:
                                           tests/test_gpu_layer_exact.py)
 backward, gget_op_attn_bwd                S 8 | 32                                                attn_bwd_small_kernel
                                           S 40 | 64                                               attn_bwd_long_kernel
                                           S 40 | 160 with RoPE on load                            attn_bwd_dq_kernel / attn_bwd_dkv_kernel <1> | <4>
                                           S 72 | 160                                              attn_bwd_dq_kernel / attn_bwd_dkv_kernel <2> | <4>
                                           S 320 | 520                                             attn_bwd_dq64_kernel + attn_bwd_dkv64_kernel<.., 8> | <.., 8, 128>
          gget_op_attn_bwd_varlen          S 40 | 64, qk_rotated = 1, with and without tables     attn_bwd_small_kernel + attn_bwd_long_kernel
                                           S 160 | 320                                             attn_bwd_dq(64)_kernel / attn_bwd_dkv(64)_kernel through row_base
          gget_op_attn_bwd_ranges          S 40 | 72 | 160 | 320 | 520                             PK = true of the two-kernel forms
          gget_op_attn_bwd_fused           S 256 | 320 | 520 (1, 2, 3 slabs), padded and packed    attn_delta_kernel, attn_bwd_fused64_kernel<PK>, attn_dq_finish_kernel
"""
import ctypes as C
import importlib

import pytest
import torch

import _attn_out_ref as A
import _heads_ref as H
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")

SENT16 = 0x7FC1          # bf16 NaN payload no kernel writes (as tests/test_gpu_attn_probs.py)
GUARD = 8                # rows behind every row buffer that must stay untouched
FWD, BWD = A.forward_cases(), A.backward_cases()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ST():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def nan16(rows, width):
    return torch.full((rows + GUARD, width), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def nan32(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


class Staged:
    """The device side of a case: padded grid, or (var-len entries) the samples' real rows back to back."""

    def __init__(self, pr, c):
        self.pr, self.c = pr, c
        B, S = pr.B, pr.S
        self.varlen = c["entry"].endswith("varlen")
        self.sel = pr.real.reshape(-1).nonzero().squeeze(1) if self.varlen else None
        self.rows = len(self.sel) if self.varlen else B * S
        self.qkv, self.dout = self.to_dev(pr.qkv), self.to_dev(pr.dout)
        self.key_len = None if c["packed"] else torch.tensor(pr.lens, dtype=torch.int32, device="cuda")
        self.row_base = None
        if self.varlen:
            n = torch.tensor(pr.lens)
            self.row_base = (torch.cumsum(n, 0) - n).to(torch.int32).cuda()
        self.lo = pr.lo.cuda() if c["packed"] else None
        self.hi = pr.hi.cuda() if c["packed"] else None
        tab = pr.rope is not None
        self.cos, self.sin, self.pos = (pr.cos.cuda(), pr.sin.cuda(), pr.pos.cuda()) if tab else (None, None, None)

    def to_dev(self, grid):
        t = grid[self.sel] if self.varlen else grid
        return torch.cat([t, torch.zeros(GUARD, t.shape[1], dtype=t.dtype)]).cuda()

    def to_grid(self, t, what):
        """A row buffer back on the padded grid (var-len: rows of no sample are zeros); the guard rows behind it must be untouched."""
        torch.cuda.synchronize()
        assert bool((t[self.rows:].view(torch.int16) == SENT16).all()), f"{what}: rows behind the buffer were written"
        body = t[:self.rows].cpu()
        if not self.varlen:
            return body
        grid = torch.zeros(self.pr.B * self.pr.S, t.shape[1], dtype=t.dtype)
        grid[self.sel] = body
        return grid


def forward(lib, st):
    """The forward entry of the case's family: out (row buffer, device) and lse [B,H,S] (device), both pre-filled with NaN."""
    pr, c = st.pr, st.c
    B, S, Hn, d = pr.B, pr.S, pr.Hn, pr.Hn * A.DH
    out, lse = nan16(st.rows, d), nan32(B, Hn, S)
    e = c["entry"]
    if e == "oproj_fwd":
        g = H.gen(99)
        wo = H.randn_bf16(g, d, d, scale=0.03).cuda()
        x_in = H.randn_bf16(g, st.rows + GUARD, d).cuda()
        nw = torch.ones(d, dtype=torch.bfloat16, device="cuda")
        wo_f, wo_b = torch.empty_like(wo), torch.empty_like(wo)
        x_mid, xn, rstd = nan16(st.rows, d), nan16(st.rows, d), nan32(st.rows + GUARD)
        taken = C.c_int32(0)
        L.check(lib.gget_op_pack_wo(P(wo), 0, P(wo_f), P(wo_b), d, 1, ST()))
        L.check(lib.gget_op_attn_oproj_fwd(P(st.qkv), P(st.key_len), None, P(out), P(lse), P(wo_f), P(x_in), P(x_mid), P(nw), P(xn), P(rstd), B, S, Hn,
                                           pr.causal, 1e-6, pr.p, pr.dseed, ST(), C.byref(taken)))
        assert taken.value == 1, "the fused attention + o-projection form was not taken"
    elif c["packed"]:
        L.check(lib.gget_op_attn_fwd_ranges(P(st.qkv), P(st.lo), P(st.hi), P(out), P(lse), B, S, Hn, pr.causal, pr.p, pr.dseed, ST()))
    elif st.varlen:
        L.check(lib.gget_op_attn_fwd_varlen(P(st.qkv), P(st.key_len), P(st.row_base), P(out), P(lse), B, S, Hn, pr.causal, P(st.cos), P(st.sin),
                                            P(st.pos), 1, pr.p, pr.dseed, ST()))
    else:
        L.check(lib.gget_op_attn_fwd(P(st.qkv), P(st.key_len), P(out), P(lse), B, S, Hn, pr.causal, P(st.cos), P(st.sin), P(st.pos), pr.p,
                                     pr.dseed, ST()))
    return out, lse


def finish(cid, results):
    for name, ratio, _ in results:
        if name in ("out", "lse", "dq", "dk", "dv"):
            record_error(f"attn_exact/{cid}", f"{name}_worst_ratio", ratio, 1.0)
            print(f"attn_exact/{cid}: {name} max err / bound = {ratio:.4f}")
    msgs = H.settle(results)[1]
    assert not msgs, f"{cid}:\n" + "\n".join(msgs)


@pytest.mark.parametrize("c", FWD, ids=[c["id"] for c in FWD])
def test_attention_forward_per_element(lib, c):
    pr = A.problem_of(c)
    st = Staged(pr, c)
    out, lse = forward(lib, st)
    finish(c["id"], A.forward_check(pr, st.to_grid(out, "out"), lse.cpu(), zero_rows=c["packed"]))


@pytest.mark.parametrize("c", BWD, ids=[c["id"] for c in BWD])
def test_attention_backward_per_element(lib, c):
    pr = A.problem_of(c)
    st = Staged(pr, c)
    B, S, Hn, d = pr.B, pr.S, pr.Hn, pr.Hn * A.DH
    out, lse = forward(lib, st)
    dqkv, delta = nan16(st.rows, 3 * d), nan32(B, Hn, S)
    slabs = A.slabs_of(c)
    e = c["entry"]
    if e == "bwd_fused":
        ws = torch.full((max(slabs, 1), B * S, d), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)     # scratch: contents irrelevant
        L.check(lib.gget_op_attn_bwd_fused(P(st.qkv), P(out), P(st.dout), P(lse), P(st.key_len), P(st.lo), P(st.hi), P(dqkv), P(delta), P(ws), B, S, Hn,
                                           pr.causal, pr.p, pr.dseed, ST()))
    elif c["packed"]:
        L.check(lib.gget_op_attn_bwd_ranges(P(st.qkv), P(out), P(st.dout), P(lse), P(st.lo), P(st.hi), P(dqkv), P(delta), B, S, Hn, pr.causal, pr.p,
                                            pr.dseed, ST()))
    elif st.varlen:
        L.check(lib.gget_op_attn_bwd_varlen(P(st.qkv), P(out), P(st.dout), P(lse), P(st.key_len), P(st.row_base), P(dqkv), P(delta), B, S, Hn, pr.causal,
                                            P(st.cos), P(st.sin), P(st.pos), 1, pr.p, pr.dseed, ST()))
    else:
        L.check(lib.gget_op_attn_bwd(P(st.qkv), P(out), P(st.dout), P(lse), P(st.key_len), P(dqkv), P(delta), B, S, Hn, pr.causal, P(st.cos),
                                     P(st.sin), P(st.pos), pr.p, pr.dseed, ST()))
    from_out = A.delta_from_out(S, c["packed"], pr.rope)
    finish(c["id"], A.backward_check(pr, st.to_grid(dqkv, "dqkv"), lse.cpu(), st.to_grid(out, "out"), from_out, slabs, pad_zero=not st.varlen))
