"""Attention weights (`output_attentions=True`; csrc/attention.hip attn_probs_kernel behind gget_op_attn_probs / gget_attention_probs):
a float64 statement of the definition, seeded inputs, the per-element error bound and the checks that hold an implementation to it
(the machinery of tests/_heads_ref.py).  tests/test_gpu_attn_probs.py and tests/test_gpu_attn_model.py feed the checks with the HIP
kernel's output, tests/test_attn_ref.py with the fp32 CPU statement below (which must pass), with planted faults (which must not) and
with the reference fixtures.

The definition, per (b, h, q, k), from the bf16 rows q_bhq, k_bhk (rotated already), head_dim 64:
    x = <q, k> / 8        lse_q = log sum_{k allowed} exp(x_qk)        out = bf16(m_qk exp(x_qk - lse_q)) if k is allowed for q, else 0
Allowed keys: right padding  q < len_b, k < len_b, and k <= q when causal;  packed rows  lo[b,q] <= k <= hi[b,q] (and k <= q when causal).
m = 1 without dropout, else the forward's keep multiplier 0 or 1 / (1 - p) (attn_drop_keep, the twin of drop_mul_x).
The statement forms lse itself, in float64, from the same q and k: the lse an implementation is handed (the forward's, fp32) is part of
what is checked, and its error is part of the bound.

Bound.  u = 2^-24.  |got - ref| <= 2^-8 |ref| + 1.01 ref (e^E - 1) + floor, E the absolute error of the exponent x - lse:
 * 2^-8 |ref|: the single rounding to bf16 (assert_elementwise's output term; the factor 1.01 carries it over to the erroneous value).
 * the recomputed score: an fp32 accumulation of K = 64 terms in any order, c_acc K u sum_j |q_j k_j| with c_acc = 2 (the rule of
   _heads_ref), times 1/8:  16 u A_qk,  A_qk = sum_j |q_j k_j|.
 * the scores inside the supplied lse: the forward forms every x_qk' the same way; d lse = sum_k' p_k' d x_k':  16 u W_q,
   W_q = sum_k' p_qk' A_qk'  (p the un-dropped weights).
 * the sum and the log of the forward's online softmax, relative to the sum = absolute in lse:
     - at most S positive terms added in any order and grouping: (S - 1) u;
     - the running sum is rescaled when the maximum moves, at most once per 32-key tile (the smallest tile of any forward kernel):
       a product (u), the factor exp2(m - m') with its instruction error (2 u) and its rounded argument, whose effect
       u |m - m'| ln 2 * 2^-|m - m'| is below 0.4 u:  under 4 u per tile, 4 ceil(S / 32) u;
     - every term exp2(fma(s, log2(e) / 8, -m)): the instruction 2 u, the rounded argument u |x_k - m|, weighted by the term's share:
       sum_k p_k (m - x_k) = (m - lse) + entropy <= ln S, so (ln S + 2) u; the rounded constant log2(e) / 8: u sum_k p_k |x_k| = u X_q;
     - log2 of the sum (2 u of a value in [0, log2 S]): 2 ln S u;
   together (S + 4 ceil(S / 32) + 3 ln S + 1) u + u X_q, the "(S + const) u" of the sum.
 * the conversions of lse: m + log2(sum) is rounded (u |lse|), multiplied by the rounded 1 / log2(e) (2 u |lse|) when it is stored, and by
   the rounded log2(e) when it is read back (2 u |lse|):  5 u |lse_q|.
 * the exponent itself, fma(s, log2(e) / 8, -lse log2(e)): the rounded constant u |x_qk|, the rounded result u |x_qk - lse_q|.
 * the exponential instruction (1 ulp = 2 u relative) and the product with m (u): 3 u.  All of these enter as ref (e^E - 1).
 * floor = 2^-126 max(1, m): exp2 of the hardware flushes a result below the smallest normal fp32 number to zero (so does the bf16
   conversion); the product with m comes after.
Nothing here is fitted to the kernel: every constant is the count of roundings of the contract above.
"""
import math

import numpy as np
import torch

import _heads_ref as H

U = H.U
TINY = H.TINY
DH = 64
SURE = 2.0 ** -120      # a weight above this cannot flush to zero under the bound: where zeros are decided by the rule (and the mask) alone


# ------------------------------------------------------------------------------------------------------------------ allowed keys
def allowed_padded(B, S, lens, causal):
    """bool [B, S(query), S(key)]: q < len_b, k < len_b, k <= q when causal."""
    pos = torch.arange(S)
    real = pos[None, :] < torch.as_tensor(lens, dtype=torch.int64)[:, None]          # [B,S]
    ok = real[:, :, None] & real[:, None, :]
    if causal:
        ok = ok & (pos[None, None, :] <= pos[None, :, None])
    return ok


def allowed_packed(lo, hi, causal=False):
    """bool [B,S,S] from inclusive per-token key ranges int [B,S] (empty: hi < lo)."""
    S = lo.shape[1]
    pos = torch.arange(S)
    ok = (pos[None, None, :] >= lo[:, :, None].long()) & (pos[None, None, :] <= hi[:, :, None].long())
    if causal:
        ok = ok & (pos[None, None, :] <= pos[None, :, None])
    return ok


def split_qk(qkv, B, S, Hn):
    """q, k as [B,H,S,64] from the [B*S, 3*64H] (or [B,S,3*64H]) q | k | v buffer."""
    d = Hn * DH
    t = qkv.reshape(B, S, 3 * d)
    q = t[:, :, :d].reshape(B, S, Hn, DH).transpose(1, 2)
    k = t[:, :, d:2 * d].reshape(B, S, Hn, DH).transpose(1, 2)
    return q, k


# ------------------------------------------------------------------------------------------------------------------ float64 statement
def attn_probs64(q, k, allowed, keep=None):
    """q, k [B,H,S,64] (any float dtype), allowed bool [B,S,S], keep [B,H,S,S] or None.  Returns dict of float64 tensors [B,H,S,S]:
    ref (the definition), p (before dropout), x, A = sum_j |q_j k_j|; and per query [B,H,S]: lse (0 for a query without keys),
    W = sum_k p A, X = sum_k p |x|."""
    q, k = q.double(), k.double()
    x = q @ k.transpose(2, 3) / 8.0
    A = q.abs() @ k.abs().transpose(2, 3)
    ok = allowed[:, None].expand_as(x)
    xm = x.masked_fill(~ok, float("-inf"))
    has = ok.any(-1)
    lse = torch.logsumexp(xm.masked_fill(~has[..., None], 0.0), -1).masked_fill(~has, 0.0)
    p = torch.exp(xm - lse[..., None]).masked_fill(~ok, 0.0)
    ref = p if keep is None else p * keep.double()
    return dict(ref=ref, p=p, x=x, A=A, lse=lse, W=(p * A).sum(-1), X=(p * x.abs()).sum(-1), allowed=ok)


def attn_sum_const(S):
    """The "(S + const)" of the sum and the log of the online softmax, in units of u (module docstring)."""
    return S + 4 * math.ceil(S / 32) + 3 * math.log(S) + 1


def attn_exp_err(r, S):
    """E of the module docstring: the absolute error of the exponent x - lse, [B,H,S,S]."""
    lse, x = r["lse"][..., None], r["x"]
    const = attn_sum_const(S) + 3
    return U * (16 * r["A"] + 16 * r["W"][..., None] + const + r["X"][..., None] + 5 * lse.abs() + x.abs() + (x - lse).abs())


def attn_bound(r, S, m_max=1.0):
    """The per-element bound of the module docstring from attn_probs64's result."""
    E = attn_exp_err(r, S)
    ref = r["ref"]
    return (2.0 ** -8 * ref + 1.01 * ref * torch.expm1(E) + TINY * max(1.0, m_max)).masked_fill(~r["allowed"], 0.0)


# ------------------------------------------------------------------------------------------------------------------ dropout twin
def attn_drop_keep(seed, B, Hn, S, p, swap_fields=False):
    """Python twin of drop_mul_x() in csrc/attention.hip (a copy of tests/test_gpu_model.py:_attn_drop_keep): keep multiplier
    [B,H,S(query),S(key)], 0 or 1 / (1 - p), of the counter-based mask keyed by (seed, b * H + h, q, k).  swap_fields: the planted
    fault - odd keys read the low 16-bit field and even keys the high one."""
    bh = np.arange(B * Hn, dtype=np.uint64)[:, None, None]
    q = np.arange(S, dtype=np.uint64)[None, :, None]
    k = np.arange(S, dtype=np.uint64)[None, None, :]
    M32 = np.uint64(0xFFFFFFFF)
    x = (np.uint64(seed) ^ ((bh * np.uint64(0x9E3779B1)) & M32)) & M32
    x = (x + q * np.uint64(0x85EBCA77) + (k >> np.uint64(1)) * np.uint64(0xC2B2AE3D)) & M32
    x ^= x >> np.uint64(16)
    x = ((x & np.uint64(0xFFFFFF)) * np.uint64(0x9E3779)) & M32      # v_mul_u32_u24: the low 24 bits times a 24-bit constant
    w = x ^ (x >> np.uint64(15))
    odd = (k & np.uint64(1)) == (0 if swap_fields else 1)
    f = np.where(odd, w >> np.uint64(16), w & np.uint64(0xFFFF))
    thresh = np.uint64(int(np.float32(p) * np.float32(65536.0)))
    keep = f >= thresh
    return torch.from_numpy((keep.astype(np.float32) / (1.0 - p)).reshape(B, Hn, S, S))


def layer_seed(seed, layer):
    """The seed the forward hands layer `layer`'s attention (csrc/engine.hip; tests/test_gpu_parity_stats.py:219 restates it)."""
    return (int(seed) + 0x9E37 * int(layer)) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------ inputs
def attn_inputs(B, S, Hn, kind, seed):
    """bf16 q | k | v rows [B*S, 3*64H] on the padded grid; rows behind a sample's tokens hold finite values like the others (nothing
    may depend on them).  kind "unit": N(0,1) entries, scores x of order 1.  kind "peaked": every query sits near a direction v of its
    (b, h) (entries +-2 plus N(0,1)), key j near (4 - 0.25 [j > 0] - j * 4.2 / S) v: x is about 128 at key 0, 8 lower at key 1 (key 0
    dominates the row) and falls by about 134 / S per key from there, so the weights of a row run from about 1 down through the smallest
    normal number (e^-87) to values that flush to zero."""
    g = H.gen(seed)
    d = Hn * DH
    qkv = torch.randn(B * S, 3 * d, generator=g)
    if kind == "peaked":
        t = qkv.view(B, S, 3, Hn, DH)
        v = (torch.randint(0, 2, (B, 1, Hn, DH), generator=g).float() * 4.0 - 2.0)
        j = torch.arange(S).float()
        fall = (4.0 - 0.25 * (j > 0).float() - j * 4.2 / S)[None, :, None, None]
        t[:, :, 0] = t[:, :, 0] + v
        t[:, :, 1] = t[:, :, 1] * 0.5 + fall * v
    else:
        assert kind == "unit"
    return qkv.to(torch.bfloat16)


def packed_ranges():
    """The packed case (B, S, H) = (2, 64, 2): three graphs per row, one of a single token, ending before the row's last position;
    the trailing positions are padding (lo = 0, hi = -1: an empty range).  int32 lo, hi [2, 64]."""
    S = 64
    lo = torch.zeros(2, S, dtype=torch.int32)
    hi = torch.full((2, S), -1, dtype=torch.int32)
    for b, sizes in enumerate(((1, 30, 25), (21, 1, 35))):
        n = 0
        for ln in sizes:
            lo[b, n:n + ln] = n
            hi[b, n:n + ln] = n + ln - 1
            n += ln
        assert n < S - 1
    return lo, hi


# (B, S, H, lengths): S <= 32 one tile; 40 two tiles, the second partial; 64 the two-wave block; 72 a third partial tile; 256 the
# four-wave block and the long-sequence forward kernels; 320 = 2.5 blocks of 128 queries, 5 key steps; lengths of 1, S, S - 1, 32 +- 1
SHAPES = [(1, 8, 1, (1,)), (3, 32, 2, (32, 17, 1)), (2, 40, 2, (33, 40)), (2, 64, 1, (64, 31)), (2, 72, 2, (65, 72)),
          (1, 256, 2, (255,)), (2, 320, 1, (320, 129))]
KINDS = ("unit", "peaked")


def shape_id(s):
    return f"B{s[0]}-S{s[1]}-H{s[2]}-len{'_'.join(str(n) for n in s[3])}"


def case_seed(B, S, Hn, kind):
    return 9100 + 7 * B + 3 * S + Hn + (1000 if kind == "peaked" else 0)


# ------------------------------------------------------------------------------------------------------------------ checks
def attn_check(got, q, k, allowed, keep=None, p_drop=0.0, what="attention weights"):
    """got: bf16 (or float) [B,H,S,S].  Every element under the bound; exact zeros exactly where the rule (and the mask) put them:
    zero on every key that is not allowed and on every dropped one, non-zero on every allowed, kept element whose weight is SURE."""
    S = got.shape[-1]
    m_max = 1.0 / (1.0 - p_drop) if keep is not None else 1.0
    r = attn_probs64(q, k, allowed, keep)
    bound = attn_bound(r, S, m_max)
    g = got.double()
    out = [H.held(what, g, r["ref"], bound)]
    off = ~r["allowed"] if keep is None else (~r["allowed"] | (keep == 0))
    out.append(H.held_true(what + ": zeros where the rule puts them", bool((g[off] == 0).all()),
                           f"{int((g[off] != 0).sum())} elements outside the allowed (kept) keys are not zero"))
    sure = ~off & (r["ref"] >= SURE)
    out.append(H.held_true(what + ": no zero inside", bool((g[sure] != 0).all()),
                           f"{int((g[sure] == 0).sum())} allowed elements with a weight above 2^-120 are zero"))
    return out


# ------------------------------------------------------------------------------------------------------------------ fp32 statement
def attn_probs_fp32(q, k, lens, causal, keep=None, fault=None, packed=None):
    """A plain fp32 CPU statement of the contract (must stay inside the bound), bf16 [B,H,S,S].  fault: the planted faults of
    tests/test_attn_ref.py."""
    B, Hn, S, _ = q.shape
    qf, kf = q.float(), k.float()
    if fault == "swap_qk":
        qf, kf = kf, qf
    x = (qf @ kf.transpose(2, 3)) * (1.0 if fault == "no_scale" else 0.125)
    if packed is not None:
        ok = allowed_packed(packed[0], packed[1], causal)
    else:
        ok = allowed_padded(B, S, [n + 1 if fault == "key_limit" else n for n in lens], causal)
        if fault == "key_limit":
            ok = ok & allowed_padded(B, S, lens, False).any(-1)[:, :, None]       # (the query limit stays right)
        if fault == "no_diagonal":
            ok = ok & ~torch.eye(S, dtype=torch.bool)[None]
    ok4 = ok[:, None].expand_as(x)
    xm = x.masked_fill(~ok4, float("-inf"))
    has = ok4.any(-1)
    lse = torch.logsumexp(xm.masked_fill(~has[..., None], 0.0), -1).masked_fill(~has, 0.0)
    if fault == "lse_log2":       # the stored natural log read as a log2 value
        p = torch.exp2(xm * 1.4426950408889634 - lse[..., None])
    else:
        p = torch.exp(xm - lse[..., None])
    p = p.masked_fill(~ok4, 0.0)
    if keep is not None:
        p = p * keep
    if fault == "bqhk":           # written as (b, q, h, k) into the (b, h, q, k) buffer
        p = p.permute(0, 2, 1, 3).contiguous().view(B, Hn, S, S)
    return p.to(torch.bfloat16)
