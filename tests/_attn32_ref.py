"""Attention at head width 32 (csrc/attention32.hip behind gget_op_attn_fwd_hd / _bwd_hd / _probs_hd / gget_op_rope_hd): float64 statements
of forward (out, lse), backward (dq, dk, dv with the rotate-back), attention weights and RoPE with the head width `dh` as a PARAMETER,
seeded inputs, per-element bounds and the checks that hold an implementation to them.  The allowed-key rules, the dropout twin and the
`held` machinery are those of tests/_attn_ref.py / tests/_heads_ref.py; the bounds are counted the way tests/_attn_ref.py and
tests/_attn_out_ref.py count them (read those docstrings for the derivation), with what the width changes:

 * scores x = <q, k> * dh^-1/2.  fp32 accumulation of K = dh terms, c_acc K u A with c_acc = 2, times the scale:  2 dh^1/2 u A_qk
   (16 u A at dh 64, 11.4 u A at dh 32).  dP accumulates K = dh terms: 2 dh u |dO| |V|^T.
 * the scale is not a power of two at dh 32: the forward and every recomputation of p use ONE fp32 constant fl(dh^-1/2 log2 e) inside
   exp2(fma(s, c, -m2)) - a rounded constant, relative error u, absolute u |x| on the exponent: the term `|x|` of attn_exp_err and `X_q` of
   the lse bound that _attn_ref already carries for the rounded log2(e) / 8 (there too the constant is rounded once).  dS is multiplied by
   the fp32 constant fl(dh^-1/2): its rounding and the product, 2 u |dS|, beside the 2^-8 |dS| of the bf16 rounding.
 * online softmax: one rescale per 32-key tile (the kernels' only tile), the count of _attn_ref.attn_sum_const.
 * delta is sum_k p m dP, formed in fp32 by the dQ kernel from the recomputed p and dP (a first walk over the row's key tiles; the
   handed out is not read): err delta = sum_k m p err dP + sum_k (e^Eb - 1) m p |dP| + 2 S u sum_k m p |dP|, the from-P form of
   tests/_attn_out_ref.py.
 * q and k lie rotated in memory; the tables only rotate dq / dk back (pair j <-> j + dh/2): the bound before the output rounding goes
   through the rotation, |c| b_lo + |s| b_up, plus 4 u (|lo c| + |up s|); the output rounding comes last.
 * RoPE kernel (in place, one rounding): |got - ref| <= 2^-8 |ref| + 4 u (|a c| + |b s|) + 2^-126, fp32 products and sum.
Nothing here is fitted to the kernel: every constant is a count of roundings of the contract in include/gget.h.
"""
import math

import numpy as np
import torch

import _attn_ref as R
import _heads_ref as H

U, TINY = R.U, R.TINY
BF = 2.0 ** -8
SURE = R.SURE
allowed_padded, allowed_packed, attn_drop_keep, layer_seed = R.allowed_padded, R.allowed_packed, R.attn_drop_keep, R.layer_seed


def scale_of(dh):
    return float(dh) ** -0.5


# ------------------------------------------------------------------------------------------------------------------ layout
def heads(t, B, S, Hn, dh):
    """[B*S, Hn*dh] -> [B,H,S,dh]"""
    return t.reshape(B, S, Hn, dh).transpose(1, 2)


def rows2d(t):
    """[B,H,S,dh] -> [B*S, Hn*dh]"""
    B, Hn, S, dh = t.shape
    return t.transpose(1, 2).reshape(B * S, Hn * dh)


def split_qkv(qkv, B, S, Hn, dh):
    t = qkv.reshape(B, S, 3, Hn, dh)
    return tuple(t[:, :, i].transpose(1, 2) for i in range(3))


# ------------------------------------------------------------------------------------------------------------------ RoPE
def rope_tables(max_pos, dh, theta=10000.0):
    """fp32 cos / sin [max_pos, dh/2] as graph-gpt_amd/engine.py:rope_tables builds them (inv_freq_j = theta^(-2j/dh))."""
    inv = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.float32) / dh))
    fr = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().contiguous(), fr.sin().contiguous()


def rotate(x, c, s, sign=1.0, dist=None):
    """hf apply_rotary_pos_emb on [..., dh]: pairs j <-> j + dh/2; sign = -1: the inverse (= transposed) rotation.  dist: a planted
    pair distance (the fault of tests/test_attn32_ref.py) - channel j pairs with j + dist inside every block of 2 dist channels."""
    dh = x.shape[-1]
    half = dh // 2
    if dist is None or dist == half:
        lo, up = x[..., :half], x[..., half:]
        return torch.cat((lo * c - sign * up * s, up * c + sign * lo * s), -1)
    blocks = []
    for b0 in range(0, dh, 2 * dist):
        lo, up = x[..., b0:b0 + dist], x[..., b0 + dist:b0 + 2 * dist]
        cc, ss = c[..., b0 // 2:b0 // 2 + dist], s[..., b0 // 2:b0 // 2 + dist]
        blocks += [lo * cc - sign * up * ss, up * cc + sign * lo * ss]
    return torch.cat(blocks, -1)


def rotate_abs(b, c, s):
    half = b.shape[-1] // 2
    return torch.cat((b[..., :half] * c.abs() + b[..., half:] * s.abs(), b[..., half:] * c.abs() + b[..., :half] * s.abs()), -1)


def rope64(qkv, cos, sin, pos, B, S, Hn, dh, inverse=False):
    """Float64 statement of the in-place RoPE kernel on the q and k thirds of bf16 qkv [B*S, 3 Hn dh]: (ref, bound) [B*S, 3 d]; the v third
    is untouched (bound 0).  pos int [B,S] or None (position = index in the sequence)."""
    p = pos if pos is not None else torch.arange(S)[None].repeat(B, 1)
    c, s = cos[p][:, None].double(), sin[p][:, None].double()          # [B,1,S,dh/2]
    q, k, v = (t.double() for t in split_qkv(qkv, B, S, Hn, dh))
    sign = -1.0 if inverse else 1.0
    ref, bound = [], []
    for t in (q, k):
        r = rotate(t, c, s, sign)
        ref.append(rows2d(r))
        bound.append(rows2d(BF * r.abs() + 4 * U * rotate_abs(t.abs(), c, s) + TINY))
    ref.append(rows2d(v))
    bound.append(torch.zeros_like(ref[-1]))
    return torch.stack(ref, 1).reshape(B * S, -1), torch.stack(bound, 1).reshape(B * S, -1)


def rope_fp32(qkv, cos, sin, pos, B, S, Hn, dh, inverse=False, dist=None):
    """The fp32 CPU statement of the same (one rounding), bf16 [B*S, 3 d]; dist: the planted pair distance."""
    p = pos if pos is not None else torch.arange(S)[None].repeat(B, 1)
    c, s = cos[p][:, None].float(), sin[p][:, None].float()
    q, k, v = (t.float() for t in split_qkv(qkv, B, S, Hn, dh))
    sign = -1.0 if inverse else 1.0
    out = [rows2d(rotate(t, c, s, sign, dist)) for t in (q, k)] + [rows2d(v)]
    return torch.stack(out, 1).reshape(B * S, -1).to(torch.bfloat16)


def rope_check(got, qkv, cos, sin, pos, B, S, Hn, dh, inverse=False):
    ref, bound = rope64(qkv, cos, sin, pos, B, S, Hn, dh, inverse)
    d = Hn * dh
    res = [H.held("rope q|k", got[:, :2 * d], ref[:, :2 * d], bound[:, :2 * d]),
           H.held_equal("rope: v untouched", got[:, 2 * d:].contiguous(), qkv[:, 2 * d:].contiguous())]
    return res


def rope_f32_check(got, src, cos, sin, pos, B, S, Hn, dh):
    """The engine's form (gget_op_rope_f32_hd): fp32 q | k | v [B*S, 3 d] -> bf16 with q, k rotated, every element rounded ONCE.  q, k
    under 2^-8 |ref| + 4 u (|a c| + |b s|) + 2^-126 (two fp32 products and a sum, or a product and an fma); v is bf16(src) bit for bit."""
    p = pos if pos is not None else torch.arange(S)[None].repeat(B, 1)
    c, s = cos[p][:, None].double(), sin[p][:, None].double()
    q, k, v = split_qkv(src.double(), B, S, Hn, dh)
    g = split_qkv(got, B, S, Hn, dh)
    res = []
    for nm, t, gt in (("rope f32 q", q, g[0]), ("rope f32 k", k, g[1])):
        r = rotate(t, c, s)
        res.append(H.held(nm, gt, r, BF * r.abs() + 4 * U * rotate_abs(t.abs(), c, s) + TINY))
    res.append(H.held_equal("rope f32: v is the rounded projection", g[2].contiguous(), v.float().to(torch.bfloat16).contiguous()))
    return res


# ------------------------------------------------------------------------------------------------------------------ weights
def probs64(q, k, allowed, keep, dh):
    """_attn_ref.attn_probs64 with x = <q, k> dh^-1/2."""
    q, k = q.double(), k.double()
    x = q @ k.transpose(2, 3) * scale_of(dh)
    A = q.abs() @ k.abs().transpose(2, 3)
    ok = allowed[:, None].expand_as(x)
    xm = x.masked_fill(~ok, float("-inf"))
    has = ok.any(-1)
    lse = torch.logsumexp(xm.masked_fill(~has[..., None], 0.0), -1).masked_fill(~has, 0.0)
    p = torch.exp(xm - lse[..., None]).masked_fill(~ok, 0.0)
    ref = p if keep is None else p * keep.double()
    return dict(ref=ref, p=p, x=x, A=A, lse=lse, W=(p * A).sum(-1), X=(p * x.abs()).sum(-1), allowed=ok)


def acc_coeff(dh):
    """c_acc K u A times the scale, in units of u A: 2 dh dh^-1/2."""
    return 2.0 * dh * scale_of(dh)


def exp_err(r, S, dh):
    """E: the absolute error of the exponent x - lse, [B,H,S,S] (module docstring; _attn_ref.attn_exp_err with K = dh)."""
    lse, x = r["lse"][..., None], r["x"]
    const = R.attn_sum_const(S) + 3
    a = acc_coeff(dh)
    return U * (a * r["A"] + a * r["W"][..., None] + const + r["X"][..., None] + 5 * lse.abs() + x.abs() + (x - lse).abs())


def probs_bound(r, S, dh, m_max=1.0):
    E = exp_err(r, S, dh)
    ref = r["ref"]
    return (BF * ref + 1.01 * ref * torch.expm1(E) + TINY * max(1.0, m_max)).masked_fill(~r["allowed"], 0.0)


def probs_check(got, q, k, allowed, dh, keep=None, p_drop=0.0, what="attention weights"):
    """got bf16 [B,H,S,S]: every element under the bound; exact zeros exactly where the rule and the mask put them."""
    S = got.shape[-1]
    m_max = 1.0 / (1.0 - p_drop) if keep is not None else 1.0
    r = probs64(q, k, allowed, keep, dh)
    g = got.double()
    out = [H.held(what, g, r["ref"], probs_bound(r, S, dh, m_max))]
    off = ~r["allowed"] if keep is None else (~r["allowed"] | (keep == 0))
    out.append(H.held_true(what + ": zeros where the rule puts them", bool((g[off] == 0).all()),
                           f"{int((g[off] != 0).sum())} elements outside the allowed (kept) keys are not zero"))
    sure = ~off & (r["ref"] >= SURE)
    out.append(H.held_true(what + ": no zero inside", bool((g[sure] != 0).all()),
                           f"{int((g[sure] == 0).sum())} allowed elements with a weight above 2^-120 are zero"))
    return out


def probs_fp32(q, k, allowed, dh, keep=None, fault=None):
    """A plain fp32 CPU statement of the weights, bf16 [B,H,S,S].  fault: "scale_1_8", "lse_log2"."""
    x = (q.float() @ k.float().transpose(2, 3)) * (0.125 if fault == "scale_1_8" else np.float32(scale_of(dh)))
    ok4 = allowed[:, None].expand_as(x)
    xm = x.masked_fill(~ok4, float("-inf"))
    has = ok4.any(-1)
    lse = torch.logsumexp(xm.masked_fill(~has[..., None], 0.0), -1).masked_fill(~has, 0.0)
    if fault == "lse_log2":
        p = torch.exp2(xm * 1.4426950408889634 - lse[..., None])
    else:
        p = torch.exp(xm - lse[..., None])
    p = p.masked_fill(~ok4, 0.0)
    if keep is not None:
        p = p * keep
    return p.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ dropout twin
def drop_keep(seed, B, Hn, S, p, heads_in_hash=None):
    """_attn_ref.attn_drop_keep, keyed by (seed, b * Hn + h, q, k).  heads_in_hash: the planted fault - the hash keyed with another head
    count (b * heads_in_hash + h, what a kernel computing H as d / 64 would do)."""
    if heads_in_hash is None or heads_in_hash == Hn:
        return attn_drop_keep(seed, B, Hn, S, p)
    n = (B - 1) * heads_in_hash + Hn
    flat = attn_drop_keep(seed, 1, n, S, p)[0]                       # [n,S,S] for bh = 0 .. n - 1
    bh = torch.arange(B)[:, None] * heads_in_hash + torch.arange(Hn)[None, :]
    return flat[bh]


# ------------------------------------------------------------------------------------------------------------------ inputs
RISE_MAX, V0, Q_ALPHA, K_SIGMA = 0.03, 1.0, 2.0, 1.0


def attn_inputs(B, S, Hn, dh, kind, seed):
    """bf16 q | k | v rows [B*S, 3 Hn dh] on the padded grid; rows behind a sample's tokens hold finite values like the others.  "unit":
    N(0,1).  "rising" (the kind of _attn_out_ref.attn_inputs at width dh): q = Q_ALPHA s + N(0,1), k_j = (j + 1) min(4.2 / S, RISE_MAX) /
    Q_ALPHA s + noise orthogonal to the sign vector s: the score grows with the key index, so the last allowed key of a row carries the
    largest weight on average and a key just outside the mask would outweigh it if it leaked in."""
    g = H.gen(seed)
    d = Hn * dh
    qkv = torch.randn(B * S, 3 * d, generator=g)
    if kind == "rising":
        t = qkv.view(B, S, 3, Hn, dh)
        v = (torch.randint(0, 2, (B, 1, Hn, dh), generator=g).float() * 2.0 - 1.0) * V0
        rise = ((torch.arange(S).float() + 1) * min(4.2 / S, RISE_MAX) / Q_ALPHA)[None, :, None, None]
        noise = t[:, :, 1] - (t[:, :, 1] * v).sum(-1, keepdim=True) / (V0 * V0 * dh) * v
        t[:, :, 0] = t[:, :, 0] + Q_ALPHA * v
        t[:, :, 1] = noise * K_SIGMA + rise * v
    else:
        assert kind == "unit"
    return qkv.to(torch.bfloat16)


def ranges_for(B, S):
    """Packed rows at any S >= 8: up to three graphs per row (one of a single token where there is room), a padded tail of 1 + b
    positions with the EMPTY range lo = 0, hi = -1, and - S >= 40 - graph boundaries that are no multiple of 32.  int32 lo, hi [B,S]."""
    lo = torch.zeros(B, S, dtype=torch.int32)
    hi = torch.full((B, S), -1, dtype=torch.int32)
    for b in range(B):
        n_real = max(S - 1 - b, 1)
        if n_real >= 3:
            a = max((n_real - 1) * 9 // 16, 1)
            if S >= 40 and ((a + 1) % 32 == 0 or a % 32 == 0):
                a += 3
            sizes = (1, a, n_real - 1 - a) if b % 2 == 0 else (a, 1, n_real - 1 - a)
        else:
            sizes = (n_real,)
        n = 0
        for ln in sizes:
            if ln < 1:
                continue
            lo[b, n:n + ln] = n
            hi[b, n:n + ln] = n + ln - 1
            n += ln
        assert n == n_real
    return lo, hi


class Problem:
    """One case on the padded [B,S] grid at head width dh.  rope: None or "memory" (q / k in memory are taken as rotated; the tables
    rotate dq / dk back); pos_ids: arbitrary position ids (else NULL: position = index)."""

    def __init__(self, B, S, Hn, dh=32, lens=None, packed=False, causal=0, p=0.0, kind="unit", rope=None, pos_ids=True, seed=None,
                 dseed=0x5EED1234):
        self.B, self.S, self.Hn, self.dh, self.causal, self.p, self.kind, self.rope, self.dseed = B, S, Hn, dh, int(causal), float(p), kind, rope, dseed
        self.packed = packed
        self.lens = None if packed else tuple(lens if lens is not None else [S] * B)
        seed = seed if seed is not None else 8300 + 11 * B + 3 * S + Hn + dh + {"unit": 0, "rising": 2000}[kind]
        self.qkv = attn_inputs(B, S, Hn, dh, kind, seed)
        if packed:
            self.lo, self.hi = ranges_for(B, S)
            self.allowed = allowed_packed(self.lo, self.hi, bool(causal))
            self.real = self.hi >= self.lo
        else:
            self.lo = self.hi = None
            self.allowed = allowed_padded(B, S, self.lens, bool(causal))
            self.real = torch.arange(S)[None, :] < torch.tensor(self.lens)[:, None]
        self.keep = drop_keep(dseed, B, Hn, S, p) if p > 0 else None
        self.m_max = 1.0 / (1.0 - p) if p > 0 else 1.0
        dout = H.randn_bf16(H.gen(seed + 1), B * S, Hn * dh)
        self.dout = (dout.view(B, S, -1) * self.real[:, :, None]).reshape(B * S, -1).contiguous()     # zero on rows without a token
        self.cos = self.sin = self.pos = None
        if rope:
            self.cos, self.sin = rope_tables(S + 16, dh)
            if pos_ids:
                self.pos = torch.arange(S)[None].repeat(B, 1)
                self.pos[0, S // 2:] += 7          # arbitrary (fine-tune style) position ids
        self.real_h = self.real[:, None, :].expand(B, Hn, S)

    def angles(self, dtype):
        """cos, sin [B,1,S,dh/2] of every position."""
        p = self.pos if self.pos is not None else torch.arange(self.S)[None].repeat(self.B, 1)
        return self.cos[p][:, None].to(dtype), self.sin[p][:, None].to(dtype)


# ------------------------------------------------------------------------------------------------------------------ forward
def forward64(pr):
    """Float64 statement and bounds of the forward: out, out_bound [B,H,S,dh], lse, lse_bound [B,H,S], the weights r."""
    S, dh = pr.S, pr.dh
    q, k, v = (t.double() for t in split_qkv(pr.qkv, pr.B, S, pr.Hn, dh))
    r = probs64(q, k, pr.allowed, pr.keep, dh)
    pm = r["ref"]
    E = exp_err(r, S, dh)
    lse_b = U * (acc_coeff(dh) * r["W"] + R.attn_sum_const(S) + r["X"] + 3 * r["lse"].abs())
    out = pm @ v
    pv = pm @ v.abs()
    live = r["allowed"].double() @ v.abs()
    inner = BF * pv + (torch.expm1(E) * pm) @ v.abs() + (2 * S + math.ceil(S / 32) + 3) * U * pv
    bound = BF * out.abs() + 1.01 * inner + TINY * (1 + pr.m_max * live)
    return dict(out=out, out_bound=bound, lse=r["lse"], lse_bound=lse_b, r=r, v=v)


def forward_check(pr, out, lse, f=None, zero_rows=False):
    """out bf16 [B*S, d] and lse fp32 [B,H,S] on the padded grid: every element of the rows that hold a token under its bound; a real row
    without an allowed key has out 0 and lse 0; a row with one allowed key and no dropout is that v row bit for bit; zero_rows: rows
    without a token (packed padding) are exact zeros in out and lse."""
    B, S, Hn, dh = pr.B, pr.S, pr.Hn, pr.dh
    f = f or forward64(pr)
    g = heads(out, B, S, Hn, dh)
    l3 = lse.reshape(B, Hn, S)
    rows = pr.real_h
    res = [H.held("out", g[rows], f["out"][rows], f["out_bound"][rows]),
           H.held("lse", l3[rows], f["lse"][rows], f["lse_bound"][rows])]
    ok = f["r"]["allowed"]
    none = ~ok.any(-1) & (rows | zero_rows)
    res.append(H.held_true("out, lse: a query without an allowed key has out 0 and lse 0",
                           bool((g[none] == 0).all()) and bool((l3[none] == 0).all()), "a query without keys is not zero"))
    if pr.p == 0:
        one = rows & (ok.sum(-1) == 1)
        if bool(one.any()):
            key = ok.double().argmax(-1)
            vrow = torch.gather(heads(pr.qkv.view(B * S, 3, -1)[:, 2], B, S, Hn, dh), 2, key[..., None].expand(B, Hn, S, dh))
            res.append(H.held_equal("out: a row with one allowed key is that v row", g[one].contiguous(), vrow[one].contiguous()))
    return res


# ------------------------------------------------------------------------------------------------------------------ backward
def backward64(pr, lse, out):
    """Float64 statement and bounds of dq, dk, dv [B,H,S,dh] from the handed lse (fp32 [B,H,S]); delta = sum_k p m dP (the handed out,
    bf16 [B*S, d], is not read).  With pr.rope the gradients are rotated back."""
    B, S, Hn, dh = pr.B, pr.S, pr.Hn, pr.dh
    sc = scale_of(dh)
    q, k, v = (t.double() for t in split_qkv(pr.qkv, B, S, Hn, dh))
    ok = pr.allowed[:, None].expand(B, Hn, S, S)
    lse = lse.reshape(B, Hn, S).double().masked_fill(~pr.real_h, 0.0)[..., None]
    x = q @ k.transpose(2, 3) * sc
    A = q.abs() @ k.abs().transpose(2, 3)
    p = torch.exp((x - lse).masked_fill(~ok, float("-inf")))
    m = pr.keep.double() if pr.keep is not None else torch.ones_like(p)
    pm = p * m
    dO = heads(pr.dout, B, S, Hn, dh).double()
    Eb = U * (acc_coeff(dh) * A + 2 * lse.abs() + x.abs() + (x - lse).abs() + 3)
    eE = torch.expm1(Eb).masked_fill(~ok, 0.0)
    dP = dO @ v.transpose(2, 3)
    e_dP = 2 * dh * U * (dO.abs() @ v.abs().transpose(2, 3))
    delta = (pm * dP).sum(-1, keepdim=True)
    e_dl = (pm * e_dP + eE * pm * dP.abs() + 2 * S * U * pm * dP.abs()).sum(-1, keepdim=True)
    dS = p * (m * dP - delta)
    e_dS = 1.01 * ((BF + eE + 2 * U) * dS.abs() + p * (m * e_dP + e_dl) + 4 * U * p * (m * dP.abs() + delta.abs()))
    acc = 2 * S * U * 1.01
    ref = dict(dv=pm.transpose(2, 3) @ dO, dq=dS @ k * sc, dk=dS.transpose(2, 3) @ q * sc)
    aq, ak = dS.abs() @ k.abs() * sc, dS.abs().transpose(2, 3) @ q.abs() * sc
    inner = dict(dv=(1.01 * (BF + eE + 2 * U) * pm + acc * pm).transpose(2, 3) @ dO.abs(),
                 dq=e_dS @ k.abs() * sc + acc * aq,
                 dk=e_dS.transpose(2, 3) @ q.abs() * sc + acc * ak)
    floor = dict(dv=TINY * (1 + pr.m_max * dO.abs().sum(2, keepdim=True)), dq=TINY * (1 + k.abs().sum(2, keepdim=True) * sc),
                 dk=TINY * (1 + q.abs().sum(2, keepdim=True) * sc))
    if pr.rope:
        c, s = pr.angles(torch.float64)
        for nm in ("dq", "dk"):
            g = ref[nm]
            inner[nm] = rotate_abs(inner[nm], c, s) + 4 * U * rotate_abs(g.abs(), c, s)
            floor[nm] = 2 * floor[nm]
            ref[nm] = rotate(g, c, s, -1.0)
    bound = {nm: BF * ref[nm].abs() + inner[nm] + floor[nm] for nm in ref}
    return dict(ref=ref, bound=bound)


def grads(dqkv, B, S, Hn, dh):
    return dict(zip(("dq", "dk", "dv"), split_qkv(dqkv, B, S, Hn, dh)))


def backward_check(pr, dqkv, lse, out, bw=None, pad_zero=True):
    """dqkv bf16 [B*S, 3 d] on the padded grid: every element of the rows that hold a token under its bound, rows without a token exact
    zeros (what the weight-gradient GEMM relies on)."""
    bw = bw or backward64(pr, lse, out)
    g = grads(dqkv, pr.B, pr.S, pr.Hn, pr.dh)
    rows = pr.real_h
    res = [H.held(nm, g[nm][rows], bw["ref"][nm][rows], bw["bound"][nm][rows]) for nm in ("dq", "dk", "dv")]
    if pad_zero:
        pad = ~pr.real.reshape(-1)
        res.append(H.held_true("dqkv: rows without a token are zero", bool((dqkv[pad] == 0).all()), "a row without a token is not zero"))
    return res


# ------------------------------------------------------------------------------------------------------------------ fp32 statements
def forward_fp32(pr, fault=None):
    """A plain fp32 CPU statement of the forward with the kernels' bf16 roundings (P o m, out): out bf16 [B*S, d], lse fp32 [B,H,S].
    fault: "scale_1_8" (the 64-wide scale), "hash_H64" (dropout hash keyed with H = d / 64), "lse_log2" (lse left in the log2 domain)."""
    B, S, Hn, dh = pr.B, pr.S, pr.Hn, pr.dh
    q, k, v = (t.float() for t in split_qkv(pr.qkv, B, S, Hn, dh))
    ok4 = pr.allowed[:, None].expand(B, Hn, S, S)
    x = (q @ k.transpose(2, 3)) * (0.125 if fault == "scale_1_8" else np.float32(scale_of(dh)))
    xm = x.masked_fill(~ok4, float("-inf"))
    has = ok4.any(-1)
    lse = torch.logsumexp(xm.masked_fill(~has[..., None], 0.0), -1).masked_fill(~has, 0.0)
    p = torch.exp(xm - lse[..., None]).masked_fill(~ok4, 0.0)
    if pr.keep is not None:
        p = p * (drop_keep(pr.dseed, B, Hn, S, pr.p, heads_in_hash=max(Hn // 2, 1)) if fault == "hash_H64" else pr.keep)
    o = p.to(torch.bfloat16).float() @ v
    o = o * (pr.real_h | pr.packed)[..., None]
    if fault == "lse_log2":
        lse = lse * 1.4426950408889634
    return rows2d(o).to(torch.bfloat16), lse.masked_fill(~pr.real_h, 0.0)


def backward_fp32(pr, lse, out, fault=None):
    """The same of the backward (P o m and dS to bf16, outputs to bf16): dqkv bf16 [B*S, 3 d].  fault: "scale_1_8", "hash_H64",
    "no_rotate_back", "pair_32", "pair_8" (the rotate-back at another pair distance)."""
    B, S, Hn, dh = pr.B, pr.S, pr.Hn, pr.dh
    sc = 0.125 if fault == "scale_1_8" else np.float32(scale_of(dh))
    q, k, v = (t.float() for t in split_qkv(pr.qkv, B, S, Hn, dh))
    ok = pr.allowed[:, None].expand(B, Hn, S, S)
    lse = lse.reshape(B, Hn, S).float().masked_fill(~pr.real_h, 0.0)[..., None]
    x = (q @ k.transpose(2, 3)) * sc
    p = torch.exp((x - lse).masked_fill(~ok, float("-inf")))
    m = torch.ones_like(p)
    if pr.keep is not None:
        m = drop_keep(pr.dseed, B, Hn, S, pr.p, heads_in_hash=max(Hn // 2, 1)) if fault == "hash_H64" else pr.keep
    pm = p * m
    dO = heads(pr.dout, B, S, Hn, dh).float()
    dP = dO @ v.transpose(2, 3)
    delta = (pm * dP).sum(-1, keepdim=True)
    dS = (p * (m * dP - delta) * sc).to(torch.bfloat16).float()
    dv = pm.to(torch.bfloat16).float().transpose(2, 3) @ dO
    dq = dS @ k
    dk = dS.transpose(2, 3) @ q
    if pr.rope and fault != "no_rotate_back":
        c, s = pr.angles(torch.float32)
        dist = {"pair_32": 32, "pair_8": 8}.get(fault)
        if dist == 32:        # the 64-wide pairing on two neighbouring heads: channel j of head 2i with channel j of head 2i + 1
            def rot_pairs(g):
                g2 = g.transpose(1, 2).reshape(B, S, Hn // 2, 2 * dh).transpose(1, 2)
                cc, ss = torch.cat((c, c), -1), torch.cat((s, s), -1)
                r = rotate(g2, cc, ss, -1.0)
                return r.transpose(1, 2).reshape(B, S, Hn, dh).transpose(1, 2)
            dq, dk = rot_pairs(dq), rot_pairs(dk)
        else:
            dq, dk = rotate(dq, c, s, -1.0, dist), rotate(dk, c, s, -1.0, dist)
    t = torch.stack([rows2d(g * pr.real_h[..., None]) for g in (dq, dk, dv)], 1)
    return t.reshape(B * S, -1).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ the case table
def _case(B, S, Hn, lens=None, causal=0, p=0.0, kind="unit", rope=None, pos_ids=True, packed=False, varlen=False):
    lens = None if packed else tuple(lens if lens is not None else [S] * B)
    c = dict(B=B, S=S, Hn=Hn, lens=lens, causal=causal, p=p, kind=kind, rope=rope, pos_ids=pos_ids, packed=packed, varlen=varlen)
    c["id"] = (f"B{B}S{S}H{Hn}-" + ("packed" if packed else ("varlen" if varlen else "len") + "_".join(map(str, lens)))
               + f"-c{causal}-p{p}-{kind}" + (f"-rope{'_ids' if pos_ids else '_noids'}" if rope else ""))
    return c


def problem_of(c, dh=32):
    return Problem(c["B"], c["S"], c["Hn"], dh, lens=c["lens"], packed=c["packed"], causal=c["causal"], p=c["p"], kind=c["kind"], rope=c["rope"],
                   pos_ids=c["pos_ids"])


def ragged(B, S):
    """Ragged lengths of a batch: the full length, and - where there is room - a length of 1 and one that ends inside a tile."""
    if B == 1:
        return (S,)
    return (S, 1, max((S * 5) // 8, 1))[:B] if B == 3 else (S, 1)


# (B, S, H): H in {1, 3, 4, 12}, B in {1, 3}, S in {1, 8, 31, 32, 33, 64, 65, 130, 257} (one tile; the tile boundary +- 1; two tiles and
# +1; a partial fifth tile; past 256), and S = 1030 with B 1, H 2 (33 key tiles)
SHAPES = [(1, 1, 1), (3, 8, 3), (3, 31, 4), (1, 32, 12), (3, 33, 1), (3, 64, 4), (1, 65, 3), (3, 130, 1), (1, 257, 4), (1, 1030, 2)]
# (causal, p, kind, rope, position ids)
COMBOS = ((0, 0.0, "unit", None, True), (1, 0.0, "rising", "memory", True), (0, 0.1, "rising", "memory", False), (1, 0.1, "unit", None, True))


def cases():
    """padded, var-len and packed cases over SHAPES; every shape sees both masks and both dropout settings, tables with and without ids."""
    cs = []
    for i, (B, S, Hn) in enumerate(SHAPES):
        lens = ragged(B, S) if S > 1 else (1,) * B
        combos = COMBOS if S <= 130 else (COMBOS[(i) % 4], COMBOS[(i + 1) % 4])
        for causal, p, kind, rope, ids in combos:
            cs.append(_case(B, S, Hn, lens, causal, p, kind, rope, ids))
        for causal, p, kind, rope, ids in combos[1:3]:
            cs.append(_case(B, S, Hn, lens, causal, p, kind, rope, ids, varlen=True))
        if S >= 8:
            for causal, p, kind, rope, ids in combos[:2]:
                cs.append(_case(B, S, Hn, None, causal, p, kind, rope, ids, packed=True))
    return cs
