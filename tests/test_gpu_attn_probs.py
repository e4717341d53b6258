"""Attention weights through the operator entry gget_op_attn_probs (csrc/attention.hip attn_probs_kernel): every output element against
the float64 statement of tests/_attn_ref.py on the same bf16 q | k (reference, bound and its derivation are there;
tests/test_attn_ref.py holds them to a correct fp32 statement and to planted faults).  The log-sum-exp the kernel is handed comes from
the existing forward entries on the same tensors - gget_op_attn_fwd (padded grid), gget_op_attn_fwd_varlen (compact rows) and
gget_op_attn_fwd_ranges (packed rows) - so the lse convention of the producers is part of what is checked.  Outputs land in buffers
pre-filled with a NaN sentinel (the launch must write every element) with pad elements behind them (it must write nothing else)."""
import ctypes as C
import importlib

import pytest
import torch

import _attn_ref as R
import _heads_ref as H
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")

SENT16 = 0x7FC1                      # bf16 NaN payload no kernel writes (as tests/test_gpu_heads.py)
PAD = 512


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ST():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    return L.load()


class Out:
    """bf16 [B,H,S,S] filled with the NaN sentinel, PAD more elements behind it."""

    def __init__(self, B, Hn, S):
        self.shape = (B, Hn, S, S)
        self.n = B * Hn * S * S
        self.buf = torch.full((self.n + PAD,), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)

    def body(self):
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:].view(torch.int16) == SENT16).all()), "wrote behind the output"
        return self.buf[:self.n].view(self.shape).cpu()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf.view(torch.int16) == SENT16).all())


def finish(case, results):
    ratio, msgs = H.settle(results)
    record_error("attn_probs_elementwise", case, ratio, 1.0)
    print(f"attn_probs_elementwise {case}: max err / bound = {ratio:.4f}")
    assert not msgs, f"{case}:\n" + "\n".join(msgs)


def nan_lse(B, Hn, S):
    return torch.full((B, Hn, S), float("nan"), device="cuda")


def probs(lib, qkv, lse, key_len, row_base, lo, hi, B, S, Hn, causal, p=0.0, seed=0):
    out = Out(B, Hn, S)
    L.check(lib.gget_op_attn_probs(P(qkv), P(lse), P(key_len), P(row_base), P(lo), P(hi), P(out.buf), B, S, Hn, int(causal), p, seed, ST()))
    return out.body()


def run_checks(lib, case, qkv_dev, lse, key_len, row_base, lo, hi, B, S, Hn, causal, q, k, ok):
    a = probs(lib, qkv_dev, lse, key_len, row_base, lo, hi, B, S, Hn, causal)
    b = probs(lib, qkv_dev, lse, key_len, row_base, lo, hi, B, S, Hn, causal)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "two runs differ"
    finish(case, R.attn_check(a, q, k, ok))
    for p, seed in ((0.1, 12345), (0.5, 0xC0FFEE11)):
        keep = R.attn_drop_keep(seed, B, Hn, S, p)
        d = probs(lib, qkv_dev, lse, key_len, row_base, lo, hi, B, S, Hn, causal, p, seed)
        finish(f"{case} p={p}", R.attn_check(d, q, k, ok, keep=keep, p_drop=p, what=f"attention weights after dropout {p}"))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("layout", ["padded", "varlen"])
@pytest.mark.parametrize("causal", [False, True], ids=["bidir", "causal"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_attn_probs(lib, request, shape, causal, layout, kind):
    B, S, Hn, lens = shape
    d = Hn * R.DH
    qkv = R.attn_inputs(B, S, Hn, kind, R.case_seed(B, S, Hn, kind))
    q, k = R.split_qk(qkv, B, S, Hn)
    ok = R.allowed_padded(B, S, lens, causal)
    key_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    lse = nan_lse(B, Hn, S)                       # (rows the forward does not write stay NaN: they must not reach the output)
    if layout == "padded":
        qkv_dev, row_base = qkv.cuda(), None
        attn = torch.empty(B * S, d, dtype=torch.bfloat16, device="cuda")
        L.check(lib.gget_op_attn_fwd(P(qkv_dev), P(key_len), P(attn), P(lse), B, S, Hn, int(causal), None, None, None, 0.0, 0, ST()))
    else:
        grid = qkv.view(B, S, 3 * d)
        qkv_dev = torch.cat([grid[b, :n] for b, n in enumerate(lens)]).contiguous().cuda()       # exactly sum(lens) rows
        base = [0]
        for n in lens[:-1]:
            base.append(base[-1] + n)
        row_base = torch.tensor(base, dtype=torch.int32, device="cuda")
        attn = torch.empty(sum(lens), d, dtype=torch.bfloat16, device="cuda")
        L.check(lib.gget_op_attn_fwd_varlen(P(qkv_dev), P(key_len), P(row_base), P(attn), P(lse), B, S, Hn, int(causal), None, None, None, 1,
                                            0.0, 0, ST()))
    run_checks(lib, request.node.callspec.id, qkv_dev, lse, key_len, row_base, None, None, B, S, Hn, causal, q, k, ok)


@pytest.mark.parametrize("kind", R.KINDS)
def test_attn_probs_packed_rows(lib, kind):
    """(2, 64, 2), three graphs per row (one of a single token), trailing positions padding: lse from gget_op_attn_fwd_ranges."""
    B, S, Hn = 2, 64, 2
    lo, hi = R.packed_ranges()
    qkv = R.attn_inputs(B, S, Hn, kind, R.case_seed(B, S, Hn, kind) + 1)
    q, k = R.split_qk(qkv, B, S, Hn)
    ok = R.allowed_packed(lo, hi)
    qkv_dev, lo_d, hi_d = qkv.cuda(), lo.cuda(), hi.cuda()
    lse = nan_lse(B, Hn, S)
    attn = torch.empty(B * S, Hn * R.DH, dtype=torch.bfloat16, device="cuda")
    L.check(lib.gget_op_attn_fwd_ranges(P(qkv_dev), P(lo_d), P(hi_d), P(attn), P(lse), B, S, Hn, 0, 0.0, 0, ST()))
    run_checks(lib, f"packed-B2-S64-H2-{kind}", qkv_dev, lse, None, None, lo_d, hi_d, B, S, Hn, False, q, k, ok)


def test_attn_probs_refusals(lib):
    """NULL operands, S <= 0 and half a key range return the error code with its text; nothing is launched: the output stays untouched."""
    B, S, Hn = 2, 40, 2
    qkv = R.attn_inputs(B, S, Hn, "unit", 5).cuda()
    lse = torch.zeros(B, Hn, S, device="cuda")
    key_len = torch.tensor([33, 40], dtype=torch.int32, device="cuda")
    lo = torch.zeros(B, S, dtype=torch.int32, device="cuda")
    out = Out(B, Hn, S)
    calls = [(None, lse, out.buf, None, B, S), (qkv, None, out.buf, None, B, S), (qkv, lse, None, None, B, S), (qkv, lse, out.buf, None, B, 0),
             (qkv, lse, out.buf, None, B, -8), (qkv, lse, out.buf, lo, B, S), (qkv, lse, out.buf, None, 0, S)]
    for a, l, o, klo, b, s in calls:
        rc = lib.gget_op_attn_probs(P(a), P(l), P(key_len), None, P(klo), None, P(o), b, s, Hn, 0, 0.0, 0, ST())
        assert rc != 0 and b"attn_probs" in lib.gget_last_error(), (rc, lib.gget_last_error())
    assert out.untouched()
