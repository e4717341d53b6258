"""The head-width-parameterised operator entries (gget_op_attn_fwd_hd / _bwd_hd / _probs_hd / gget_op_rope_hd) through the C ABI.

head_dim 32 (csrc/attention32.hip): every element of out, lse, dq, dk, dv and of the attention weights against the float64 statements
of tests/_attn32_ref.py under their bounds (tests/test_attn32_ref.py holds statements and bounds to a correct fp32 statement and to
planted faults).  Shapes (tests/_attn32_ref.py SHAPES): H in {1, 3, 4, 12}, B in {1, 3}, S in {1, 8, 31, 32, 33, 64, 65, 130, 257} and
S = 1030 (B 1, H 2); ragged lengths with a length of 1 and a full-length sample on the padded and the var-len layout, packed ranges with
an empty range, causal on and off, dropout 0 and 0.1 (the zeros of the weights equal the Python twin's mask exactly), tables with
position ids and with NULL ids.  Buffers are pre-filled with a NaN sentinel: every real row must be written, rows behind the buffers
not.  Also: the one-allowed-key row bit for bit, lse 0 / out 0 for a key-less query, pad rows of dqkv exact zeros (inside the checks of
_attn32_ref), two runs bit-identical, every _hd entry at head_dim 64 bit-equal to its existing counterpart on one shape per layout, the
error cases (return 2, nothing launched: a canary-filled output stays untouched), gget_op_rope_hd with its inverse, and
gget_op_rope_f32_hd - the engine's projection form, fp32 q | k | v to bf16 with q and k rotated - rounding every element once.
"""
import ctypes as C
import importlib

import pytest
import torch

import _attn32_ref as A
import _heads_ref as H
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")

SENT16 = 0x7FC1          # bf16 NaN payload no kernel writes
GUARD = 8                # rows behind every row buffer that must stay untouched
DH = 32
CASES = A.cases()


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
    """The device side of a case: padded grid, or (var-len) the samples' real rows back to back."""

    def __init__(self, pr, varlen):
        self.pr, self.varlen = pr, varlen
        B, S = pr.B, pr.S
        self.sel = pr.real.reshape(-1).nonzero().squeeze(1) if varlen else None
        self.rows = len(self.sel) if varlen else B * S
        self.qkv, self.dout = self.to_dev(pr.qkv), self.to_dev(pr.dout)
        self.key_len = None if pr.packed else torch.tensor(pr.lens, dtype=torch.int32, device="cuda")
        self.row_base = None
        if varlen:
            n = torch.tensor(pr.lens)
            self.row_base = (torch.cumsum(n, 0) - n).to(torch.int32).cuda()
        self.lo = pr.lo.cuda() if pr.packed else None
        self.hi = pr.hi.cuda() if pr.packed else None
        self.cos, self.sin = (pr.cos.cuda(), pr.sin.cuda()) if pr.rope else (None, None)
        self.pos = pr.pos.cuda() if pr.pos is not None else None

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


def fwd_hd(lib, st, hd=DH):
    pr = st.pr
    out, lse = nan16(st.rows, pr.Hn * hd), nan32(pr.B, pr.Hn, pr.S)
    L.check(lib.gget_op_attn_fwd_hd(P(st.qkv), P(st.key_len), P(st.row_base), P(st.lo), P(st.hi), P(out), P(lse), pr.B, pr.S, pr.Hn, hd,
                                    pr.causal, pr.p, pr.dseed, ST()))
    return out, lse


def bwd_hd(lib, st, out, lse, hd=DH):
    pr = st.pr
    dqkv, delta = nan16(st.rows, 3 * pr.Hn * hd), nan32(pr.B, pr.Hn, pr.S)
    L.check(lib.gget_op_attn_bwd_hd(P(st.qkv), P(out), P(st.dout), P(lse), P(st.key_len), P(st.row_base), P(st.lo), P(st.hi), P(dqkv), P(delta),
                                    pr.B, pr.S, pr.Hn, hd, pr.causal, P(st.cos), P(st.sin), P(st.pos), pr.p, pr.dseed, ST()))
    return dqkv


def probs_hd(lib, st, lse, hd=DH):
    pr = st.pr
    w = torch.full((pr.B, pr.Hn, pr.S, pr.S), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    L.check(lib.gget_op_attn_probs_hd(P(st.qkv), P(lse), P(st.key_len), P(st.row_base), P(st.lo), P(st.hi), P(w), pr.B, pr.S, pr.Hn, hd, pr.causal,
                                      pr.p, pr.dseed, ST()))
    return w


def finish(cid, results):
    for name, ratio, _ in results:
        if name in ("out", "lse", "dq", "dk", "dv", "attention weights", "rope q|k"):
            record_error(f"attn32/{cid}", f"{name.replace(' ', '_')}_worst_ratio", ratio, 1.0)
            print(f"attn32/{cid}: {name} max err / bound = {ratio:.4f}")
    msgs = H.settle(results)[1]
    assert not msgs, f"{cid}:\n" + "\n".join(msgs)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_attention32_per_element(lib, c):
    """forward, backward and attention weights of one case, the backward and the weights handed the forward's out and lse; a second run
    of all three gives the same bits."""
    pr = A.problem_of(c, DH)
    st = Staged(pr, c["varlen"])
    out, lse = fwd_hd(lib, st)
    dqkv = bwd_hd(lib, st, out, lse)
    w = probs_hd(lib, st, lse)
    out_g, lse_h, dqkv_g = st.to_grid(out, "out"), lse.cpu(), st.to_grid(dqkv, "dqkv")
    if c["varlen"]:      # lse behind a sample's rows is not written on the var-len layout
        assert bool(torch.isnan(lse_h[~pr.real_h]).all()), "lse: rows behind a sample were written on the var-len layout"
        lse_h = lse_h.masked_fill(~pr.real_h, 0.0)
    res = A.forward_check(pr, out_g, lse_h, zero_rows=pr.packed)
    res += A.backward_check(pr, dqkv_g, lse_h, out_g, pad_zero=not c["varlen"])
    q, k, _ = A.split_qkv(pr.qkv, pr.B, pr.S, pr.Hn, DH)
    allowed = pr.allowed if pr.packed else A.allowed_padded(pr.B, pr.S, pr.lens, bool(pr.causal))
    res += A.probs_check(w.cpu(), q, k, allowed, DH, keep=pr.keep, p_drop=pr.p)
    finish(c["id"], res)
    out2, lse2 = fwd_hd(lib, st)
    dqkv2 = bwd_hd(lib, st, out, lse)
    w2 = probs_hd(lib, st, lse)
    torch.cuda.synchronize()
    for a, b, nm in ((out, out2, "out"), (dqkv, dqkv2, "dqkv"), (w, w2, "weights")):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{nm}: two runs differ"
    assert torch.equal(lse.view(torch.int32), lse2.view(torch.int32)), "lse: two runs differ"


@pytest.mark.parametrize("B,S,Hn,ids,inverse", [(3, 33, 3, True, 0), (1, 8, 12, False, 0), (3, 33, 4, True, 1), (1, 257, 1, False, 1)])
def test_rope_hd_width32(lib, B, S, Hn, ids, inverse):
    g = H.gen(4100 + S + Hn)
    qkv = H.randn_bf16(g, B * S, 3 * Hn * DH)
    cos, sin = A.rope_tables(S + 16, DH)
    pos = None
    if ids:
        pos = torch.arange(S)[None].repeat(B, 1)
        pos[0, S // 2:] += 7
    buf = torch.cat([qkv, torch.full((GUARD, qkv.shape[1]), SENT16, dtype=torch.int16).view(torch.bfloat16)]).cuda()
    cos_d, sin_d, pos_d = cos.cuda(), sin.cuda(), (pos.cuda() if ids else None)
    L.check(lib.gget_op_rope_hd(P(buf), P(cos_d), P(sin_d), P(pos_d), B, S, Hn, DH, inverse, ST()))
    torch.cuda.synchronize()
    assert bool((buf[B * S:].view(torch.int16) == SENT16).all()), "rope: rows behind the buffer were written"
    finish(f"rope-B{B}S{S}H{Hn}-inv{inverse}", A.rope_check(buf[:B * S].cpu(), qkv, cos, sin, pos, B, S, Hn, DH, bool(inverse)))


@pytest.mark.parametrize("B,S,Hn,ids", [(3, 33, 3, True), (1, 8, 12, False), (2, 257, 4, True)])
def test_rope_f32_hd_rounds_once(lib, B, S, Hn, ids):
    """The engine's projection form: fp32 q | k | v -> bf16 with q, k rotated, one rounding per element; head_dim 64 is refused."""
    g = H.gen(4200 + S + Hn)
    src = torch.randn(B * S, 3 * Hn * DH, generator=g) * 2.0
    cos, sin = A.rope_tables(S + 16, DH)
    pos = None
    if ids:
        pos = torch.arange(S)[None].repeat(B, 1)
        pos[0, S // 2:] += 7
    src_d, cos_d, sin_d, pos_d = src.cuda(), cos.cuda(), sin.cuda(), (pos.cuda() if ids else None)
    out = nan16(B * S, 3 * Hn * DH)
    L.check(lib.gget_op_rope_f32_hd(P(src_d), P(out), P(cos_d), P(sin_d), P(pos_d), B, S, Hn, DH, ST()))
    torch.cuda.synchronize()
    assert bool((out[B * S:].view(torch.int16) == SENT16).all()), "rope: rows behind the buffer were written"
    res = A.rope_f32_check(out[:B * S].cpu(), src, cos, sin, pos, B, S, Hn, DH)
    for name, ratio, _ in res:
        record_error(f"attn32/rope_f32-B{B}S{S}H{Hn}", f"{name.replace(' ', '_')}_worst_ratio", ratio, 1.0)
    assert not H.settle(res)[1], "\n".join(H.settle(res)[1])
    canary = nan16(B * S, 3 * Hn * DH)
    assert lib.gget_op_rope_f32_hd(P(src_d), P(canary), P(cos_d), P(sin_d), P(pos_d), B, S, Hn, 64, ST()) == 2
    assert "unsupported" in lib.gget_last_error().decode()
    torch.cuda.synchronize()
    assert bool((canary.view(torch.int16) == SENT16).all())


def _problem64(layout):
    import _attn_out_ref as A64
    B, S, Hn = 3, 72, 2
    if layout == "packed":
        return A64.Problem(B, S, Hn, packed=True, causal=1, p=0.1, kind="rising", rope="memory")
    return A64.Problem(B, S, Hn, lens=(72, 1, 45), causal=0, p=0.1, kind="rising", rope="memory")


@pytest.mark.parametrize("layout", ["padded", "varlen", "packed"])
def test_hd_entries_at_width_64_are_the_existing_kernels(lib, layout):
    """Every _hd entry with head_dim = 64 against its existing counterpart (q, k rotated in memory): the same bits."""
    pr = _problem64(layout)
    pr.packed = layout == "packed"
    st = Staged(pr, layout == "varlen")
    B, S, Hn, d = pr.B, pr.S, pr.Hn, pr.Hn * 64
    out, lse = fwd_hd(lib, st, 64)
    dqkv = bwd_hd(lib, st, out, lse, 64)
    w = probs_hd(lib, st, lse, 64)
    out0, lse0 = nan16(st.rows, d), nan32(B, Hn, S)
    dqkv0, delta0 = nan16(st.rows, 3 * d), nan32(B, Hn, S)
    w0 = torch.full((B, Hn, S, S), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    if layout == "packed":
        L.check(lib.gget_op_attn_fwd_ranges(P(st.qkv), P(st.lo), P(st.hi), P(out0), P(lse0), B, S, Hn, pr.causal, pr.p, pr.dseed, ST()))
        # (the existing ranges entry takes no tables: compare the un-rotated gradients)
        st.cos = st.sin = st.pos = None
        dqkv = bwd_hd(lib, st, out, lse, 64)
        L.check(lib.gget_op_attn_bwd_ranges(P(st.qkv), P(out0), P(st.dout), P(lse0), P(st.lo), P(st.hi), P(dqkv0), P(delta0), B, S, Hn, pr.causal, pr.p,
                                            pr.dseed, ST()))
    elif layout == "varlen":
        L.check(lib.gget_op_attn_fwd_varlen(P(st.qkv), P(st.key_len), P(st.row_base), P(out0), P(lse0), B, S, Hn, pr.causal, P(st.cos), P(st.sin),
                                            P(st.pos), 1, pr.p, pr.dseed, ST()))
        L.check(lib.gget_op_attn_bwd_varlen(P(st.qkv), P(out0), P(st.dout), P(lse0), P(st.key_len), P(st.row_base), P(dqkv0), P(delta0), B, S, Hn,
                                            pr.causal, P(st.cos), P(st.sin), P(st.pos), 1, pr.p, pr.dseed, ST()))
    else:
        L.check(lib.gget_op_attn_fwd(P(st.qkv), P(st.key_len), P(out0), P(lse0), B, S, Hn, pr.causal, None, None, None, pr.p, pr.dseed, ST()))
        L.check(lib.gget_op_attn_bwd_rotated(P(st.qkv), P(out0), P(st.dout), P(lse0), P(st.key_len), None, P(dqkv0), P(delta0), B, S, Hn, pr.causal,
                                             P(st.cos), P(st.sin), P(st.pos), pr.p, pr.dseed, None, 0, None, ST()))
    L.check(lib.gget_op_attn_probs(P(st.qkv), P(lse0), P(st.key_len), P(st.row_base), P(st.lo), P(st.hi), P(w0), B, S, Hn, pr.causal, pr.p, pr.dseed, ST()))
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), out0.view(torch.int16)), "out differs from the existing entry"
    assert torch.equal(lse.view(torch.int32), lse0.view(torch.int32)), "lse differs from the existing entry"
    assert torch.equal(w.view(torch.int16), w0.view(torch.int16)), "attention weights differ from the existing entry"
    assert torch.equal(dqkv.view(torch.int16), dqkv0.view(torch.int16)), "dqkv differs from the existing entry"


def test_rope_hd_at_width_64_is_the_existing_kernel(lib):
    import _attn_out_ref as A64
    B, S, Hn = 2, 40, 3
    qkv = H.randn_bf16(H.gen(5), B * S, 3 * Hn * 64)
    cos, sin = (t.cuda() for t in A64.rope_tables(S + 16))
    pos = (torch.arange(S)[None].repeat(B, 1) + 3).cuda()
    for inverse in (0, 1):
        a, b = qkv.clone().cuda(), qkv.clone().cuda()
        L.check(lib.gget_op_rope_hd(P(a), P(cos), P(sin), P(pos), B, S, Hn, 64, inverse, ST()))
        L.check(lib.gget_op_rope(P(b), P(cos), P(sin), P(pos), B, S, Hn, inverse, ST()))
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_error_cases_launch_nothing(lib):
    """Any other head_dim, a NULL operand, B, S or H <= 0, half a key range, row_base together with ranges: error 2, the message names
    the unsupported head width, and canary-filled outputs stay untouched."""
    pr = A.Problem(2, 40, 2, DH, packed=True, rope="memory")
    st = Staged(pr, False)
    B, S, Hn, d = pr.B, pr.S, pr.Hn, pr.Hn * DH
    kl = torch.tensor([40, 17], dtype=torch.int32, device="cuda")
    rbase = torch.tensor([0, 40], dtype=torch.int32, device="cuda")
    out, lse = nan16(st.rows, d), nan32(B, Hn, S)
    dqkv, delta = nan16(st.rows, 3 * d), nan32(B, Hn, S)
    w = torch.full((B, Hn, S, S), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    lse_in = torch.zeros(B, Hn, S, device="cuda")
    qkv_c = st.qkv.clone()

    def fwd(qkv=st.qkv, key_len=None, row_base=None, lo=st.lo, hi=st.hi, o=out, l=lse, b=B, s=S, h=Hn, hd=DH):
        return lib.gget_op_attn_fwd_hd(P(qkv), P(key_len), P(row_base), P(lo), P(hi), P(o), P(l), b, s, h, hd, 0, 0.0, 1, ST())

    def bwd(hd=DH, lo=st.lo, hi=st.hi, row_base=None, key_len=None, dq=dqkv, b=B, cos=st.cos, sin=st.sin):
        return lib.gget_op_attn_bwd_hd(P(st.qkv), P(out), P(st.dout), P(lse_in), P(key_len), P(row_base), P(lo), P(hi), P(dq), P(delta), b, S, Hn, hd, 0,
                                       P(cos), P(sin), None, 0.0, 1, ST())

    def probs(hd=DH, lo=st.lo, hi=st.hi, row_base=None, key_len=None, o=w, h=Hn):
        return lib.gget_op_attn_probs_hd(P(st.qkv), P(lse_in), P(key_len), P(row_base), P(lo), P(hi), P(o), B, S, h, hd, 0, 0.0, 1, ST())

    def rope(hd=DH, cos=st.cos, s=S):
        return lib.gget_op_rope_hd(P(qkv_c), P(cos), P(st.sin), None, B, s, Hn, hd, 0, ST())

    for hd in (16, 48, 128, 0):
        for call in (fwd, bwd, probs, rope):
            assert call(hd=hd) == 2
            msg = lib.gget_last_error().decode()
            assert "unsupported" in msg and "head_dim" in msg, msg
    bad = [fwd(qkv=None), fwd(o=None), fwd(l=None), fwd(b=0), fwd(s=0), fwd(h=0), fwd(b=-1), fwd(hi=None), fwd(lo=None),
           fwd(key_len=kl, row_base=rbase), fwd(lo=None, hi=None, row_base=rbase),
           bwd(dq=None), bwd(b=0), bwd(hi=None), bwd(key_len=kl, row_base=rbase), bwd(sin=None),
           probs(o=None), probs(h=0), probs(lo=None), probs(key_len=kl, row_base=rbase),
           rope(cos=None), rope(s=0)]
    assert bad == [2] * len(bad), bad
    torch.cuda.synchronize()
    for t, nm in ((out, "out"), (dqkv, "dqkv"), (w, "weights")):
        assert bool((t.view(torch.int16) == SENT16).all()), f"{nm}: an error case wrote its output"
    assert bool(torch.isnan(lse).all()) and bool(torch.isnan(delta).all()), "an error case wrote lse / delta"
    assert torch.equal(qkv_c.view(torch.int16), st.qkv.view(torch.int16)), "an error case rotated qkv"
