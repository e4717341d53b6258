"""Attention output, log-sum-exp and gradients (csrc/attention.hip behind gget_op_attn_fwd / _bwd and their _varlen, _ranges, _fused and
oproj forms): the float64 statement of the operator on its real inputs, seeded inputs, per-element error bounds and the checks that hold
an implementation to them - the machinery of tests/_attn_ref.py (mask, dropout twin, exponent error) and tests/_heads_ref.py (held).
tests/test_gpu_attn_exact.py feeds the checks with the HIP kernels' outputs, tests/test_attn_out_ref.py with the fp32 CPU statements
below (which must pass) and with planted faults (which must not).

Statement, per (b, h), on the bf16 q | k | v rows as they lie in memory, dout, the allowed mask (allowed_padded / allowed_packed) and the
keep multiplier m (attn_drop_keep; 1 without dropout):
    x = q k^T / 8      lse = log sum_allowed exp x      p = exp(x - lse)      O = sum_k m_k p_k v_k
    dV = (m o p)^T dO      dP = dO V^T      dS = p o (m o dP - delta)      dQ = dS K / 8      dK = dS^T Q / 8
The backward forms p from the lse it is handed (the forward's fp32 values); delta as the entry under test forms it: rowsum(dO o out) of the
handed bf16 out where the kernels read out (attn_bwd_dq_kernel :675-689, attn_bwd_dq64_kernel :2532-2545, attn_delta_kernel :2869-2892),
sum_k p m dP where they do not (attn_bwd_small_kernel :1110-1124, attn_bwd_long_item :947-961); delta_from_out() restates the dispatch
of k_attn_bwd :3526.  RoPE: rotated on load (cos_tab given, qk_rotated = 0) the statement rotates q / k in float64 and rounds them to
bf16 as rope_pair :55-72 does, and returns gradients w.r.t. the un-rotated q / k (straight through the rounding, rotated back); rotated
in memory (qk_rotated = 1) q / k are used as they are and dq / dk are rotated back.

Bounds.  u = 2^-24; b = 2^-8, the unit roundoff of bf16 (8 significant bits, round to nearest: |bf16(t) - t| <= 2^-8 |t|).  E =
attn_exp_err of _attn_ref (fp32 score accumulation 16 u A, online-softmax sum with a rescale per 32-key stage - the smallest stage of any
forward kernel, the 64-key stages of attn_fwd64_kernel / attn_fwd_dense_kernel rescale less often -, exp2, constants).  Every bf16-rounded
MFMA operand costs b times the abs-product sum of its contraction; 1.01 carries first-order terms to the erroneous values.  (Half of b per
operand, 2^-9, is the AVERAGE error of a rounding, not its bound: the fp32 statement of the contract below exceeds such a bound by 18 %
on the 32-row shape, and the kernels reach 0.88 of the bounds here.)
 out :  b |O|                                   the output rounding (store_t :321)
      + b sum_k m p |v|                         P o m is rounded to bf16 before the PV MFMA (acc_to_b :484, :621, :1358, :2193, :2343, :2407) and
                                                nothing takes the rounding back: every forward kernel sums the row sum l from the UNROUNDED p
                                                (:474, :1354, :2165, :2178, :2332, :2374) - c_P 2^-9 of the two possible counts with c_P = 2
      + sum_k (e^E - 1) m p |v|                 the exponent error of every weight
      + (2 S + ceil(S / 32) + 3) u sum m p |v|  fp32 accumulation of S terms in any order (2 S u, the rule of _heads_ref), one product per
                                                stage rescale of O (:482, :2191), the keep product (:475), 1 / l and its product (:491, :2213)
      + 2^-126 (1 + m_max sum_allowed |v|)      exp2 and the conversions flush below the smallest normal number
 lse :  u (16 W + attn_sum_const(S) + X + 3 |lse|): the lse terms of _attn_ref (scores inside the sum, the sum and its log, the rounding
      of m + log2 l and the product with the rounded 1 / log2(e), :493), absolute.
 RoPE on load: the rotated q / k are rounded to bf16 (pack8 :70) - and so they are in the statement, so what remains is a rounding that the
      error of the fp32 rotation (two products and a sum: 4 u (|a c| + |b s|)) flips: _rotate_round marks the elements whose exact value
      lies that close to a rounding boundary, each may differ by one bf16 spacing (fq, fk), a score by F = (fq |k| + |q| fk + fq fk) / 8
      (flip_scores; zero for all but a handful of scores), lse by sum_k p F.  This stays below the 2 * 2^-9 A / 8 that rounding the
      kernel's side alone would cost unless the flipped channels carry half of A, and it says where.  The operands of dQ = dS K and dK = dS^T Q carry the same fk, fq.
 backward, Eb = u (16 A + 2 |lse| + |x| + |x - lse| + 3) (+ F): the recomputed score, lse read back through the rounded log2(e) (:691,
      :808), the fma's rounded constant and result, exp2 and one product.  lse itself is an input: no error of its own.
      err dP = 2 * 64 u |dO| |V|^T (fp32 MFMA over 64 channels)
      err delta = 2 * 64 u sum_j |dO_j out_j|  (from out; :686, :2889)   or, from P:  sum_k m p err dP + sum_k (e^Eb - 1) m p |dP| +
                  2 S u sum_k m p |dP|   (:1119, :956)
      err dS = 1.01 [ (b + e^Eb - 1) |dS|  +  p (m err dP + err delta)  +  4 u p (m |dP| + |delta|) ]: the bf16 rounding of dS
               (acc_to_b :732, :857, :967, :1127, :2617, :2812, :3133), the exponent error, the propagated errors of dP and delta and the
               fp32 products - all from magnitudes, so the cancellation in m dP - delta is covered
      dV :  b |dV| + 1.01 [(b + e^Eb - 1 + 2 u) m p]^T |dO| + 2 S u 1.01 (m p)^T |dO| + floor.  P o m is rounded to bf16 (:856, :1004,
            :1158); attn_bwd_dkv64_kernel / attn_bwd_fused64_kernel round p and apply 1 / (1 - p) at the store (:2831, :3161): the same count.
      dQ :  b |dQ| + err dS |K| / 8 + 2 S u 1.01 |dS| |K| / 8 + floor; the fused form rounds every 256-key slab of dQ to bf16 (:3041):
            b times the slab's own partial sum (taken from the statement, plus b times the error so far) - and sums the ceil(S / 256) slabs
            in fp32 (:2912-2919).
      dK :  the same with Q for K and the transposed dS.
      dq / dk rotated back (unrope_acc :333, attn_dq_finish_kernel :2920): the bound before the output rounding goes through the rotation,
            |c| b_lo + |s| b_up, plus 4 u (|lo c| + |up s|) for the fp32 rotation; the output rounding comes last.
      e_dO: where the entry under test forms dO itself (attn_oproj_bwd_kernel rounds its fp32 dattn = dx_mid Wo to bf16, :1898-1903, and
            dattn never reaches memory) the statement forms dO = bf16(float64 product) and round_flips marks the elements whose exact
            value lies within the fp32 accumulation error of a rounding boundary: each may differ by one bf16 spacing, e_dO.  It
            propagates linearly: err dP += e_dO |V|^T, the dV bound += 1.01 (m p)^T e_dO, err delta from out += sum_j e_dO_j |out_j|;
            delta from P and dS carry it through err dP.  Zero (the default) where dO is an input.
Where kernel classes differ in a count the larger is used (32-key stages; 5 u |lse| inside E for the forward, which has no conversion).
Nothing here is fitted to the kernel: every constant is a count of roundings of the contract above.

Pad rows.  The q | k | v weight-gradient GEMM of csrc/engine.hip (layer_backward, K = T rows) reads EVERY row of dqkv: on the padded grid the rows
behind a sample's tokens (and packed padding rows) must be exact zeros - they are, given dout = 0 there and out / lse as the forward wrote
them -; on the var-len layout the rows behind the last sample are zeroed once per step (gget_backward_begin) and no attention launch may write them.
"""
import math

import torch

import _attn_ref as R
import _heads_ref as H

U, TINY, DH = R.U, R.TINY, R.DH
BF = 2.0 ** -8          # unit roundoff of bf16 (8 significant bits, round to nearest): the relative error of one rounding
RISE_MAX, V0, Q_ALPHA, K_SIGMA = 0.03, 1.0, 2.0, 1.0          # the "rising" kind (attn_inputs)


# ------------------------------------------------------------------------------------------------------------------ inputs
def attn_inputs(B, S, Hn, kind, seed):
    """_attn_ref.attn_inputs plus kind "rising", the mirror of "peaked": key j lies near ((j + 1) * 4.2 / S) * dir, so the score grows
    with the key index and the last allowed key of a row carries the largest weight on average; every key just outside the mask would
    outweigh it if it leaked in.  Rows behind a sample's tokens continue the pattern.  v is N(0,1).
    With a sign vector s of the (b, h) (entries +-V0): q = Q_ALPHA s + N(0,1), k_j = (j + 1) min(4.2 / S, RISE_MAX) / Q_ALPHA s + K_SIGMA n_j,
    n_j N(0,1) made orthogonal to s: x_j = 8 V0^2 (j + 1) min(4.2 / S, RISE_MAX) - a rise of 33.6 / S, at most 0.24, per key - plus noise
    of about K_SIGMA.  The constants keep what q and the keys of a row's live window have in common as small as what sets them apart:
    dq = sum_k dS_k k_k / 8 and dk = sum_q dS_qk q_q / 8 are then no differences of large numbers.  (With entries +-2 and the rise of
    "peaked" the bf16 rounding of dS alone exceeds 5 % of dq, the cap tests/test_attn_out_ref.py holds the bounds to.)"""
    if kind != "rising":
        return R.attn_inputs(B, S, Hn, kind, seed)
    g = H.gen(seed)
    d = Hn * DH
    qkv = torch.randn(B * S, 3 * d, generator=g)
    t = qkv.view(B, S, 3, Hn, DH)
    v = (torch.randint(0, 2, (B, 1, Hn, DH), generator=g).float() * 2.0 - 1.0) * V0
    rise = ((torch.arange(S).float() + 1) * min(4.2 / S, RISE_MAX) / Q_ALPHA)[None, :, None, None]
    noise = t[:, :, 1] - (t[:, :, 1] * v).sum(-1, keepdim=True) / (V0 * V0 * DH) * v
    t[:, :, 0] = t[:, :, 0] + Q_ALPHA * v
    t[:, :, 1] = noise * K_SIGMA + rise * v
    return qkv.to(torch.bfloat16)


def ranges_for(B, S):
    """Packed rows like _attn_ref.packed_ranges at any S >= 24: three graphs per row, one of a single token (first in even rows, second in
    odd ones), a padded tail of 3 + b positions (lo = 0, hi = -1), and graph boundaries that are no multiple of 32.  int32 lo, hi [B,S]."""
    lo = torch.zeros(B, S, dtype=torch.int32)
    hi = torch.full((B, S), -1, dtype=torch.int32)
    for b in range(B):
        n_real = S - 3 - b
        a = (n_real - 1) * 9 // 16
        if (a + 1) % 32 == 0 or a % 32 == 0:
            a += 3
        sizes = (1, a, n_real - 1 - a) if b % 2 == 0 else (a, 1, n_real - 1 - a)
        n = 0
        for ln in sizes:
            assert ln >= 1
            lo[b, n:n + ln] = n
            hi[b, n:n + ln] = n + ln - 1
            n += ln
        assert n == n_real and (sizes[0] + sizes[1]) % 32 != 0
    return lo, hi


def rope_tables(max_pos, theta=10000.0):
    """fp32 cos / sin [max_pos, 32] as graph-gpt_amd/engine.py:rope_tables builds them."""
    inv = 1.0 / (theta ** (torch.arange(0, DH, 2, dtype=torch.float32) / DH))
    fr = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().contiguous(), fr.sin().contiguous()


class Problem:
    """One case on the padded [B,S] grid.  rope: None, "load" (tables given, q / k un-rotated in memory) or "memory" (q / k in memory are
    taken as rotated; the tables rotate dq / dk back)."""

    def __init__(self, B, S, Hn, lens=None, packed=False, causal=0, p=0.0, kind="unit", rope=None, seed=None, dseed=0x5EED1234):
        self.B, self.S, self.Hn, self.causal, self.p, self.kind, self.rope, self.dseed = B, S, Hn, int(causal), float(p), kind, rope, dseed
        self.lens = None if packed else tuple(lens if lens is not None else [S] * B)
        seed = seed if seed is not None else 7300 + 11 * B + 3 * S + Hn + {"unit": 0, "peaked": 1000, "rising": 2000}[kind]
        self.qkv = attn_inputs(B, S, Hn, kind, seed)
        if packed:
            self.lo, self.hi = ranges_for(B, S)
            self.allowed = R.allowed_packed(self.lo, self.hi, bool(causal))
            self.real = self.hi >= self.lo
        else:
            self.lo = self.hi = None
            self.allowed = R.allowed_padded(B, S, self.lens, bool(causal))
            self.real = torch.arange(S)[None, :] < torch.tensor(self.lens)[:, None]
        self.keep = R.attn_drop_keep(dseed, B, Hn, S, p) if p > 0 else None
        self.m_max = 1.0 / (1.0 - p) if p > 0 else 1.0
        dout = H.randn_bf16(H.gen(seed + 1), B * S, Hn * DH)
        self.dout = (dout.view(B, S, -1) * self.real[:, :, None]).reshape(B * S, -1).contiguous()     # zero on rows without a token
        self.cos = self.sin = self.pos = None
        if rope:
            self.cos, self.sin = rope_tables(S + 16)
            self.pos = torch.arange(S)[None].repeat(B, 1)
            self.pos[0, S // 2:] += 7          # arbitrary (fine-tune style) position ids
        self.real_h = self.real[:, None, :].expand(B, Hn, S)

    def angles(self, dtype):
        """cos, sin [B,1,S,32] of every position."""
        return self.cos[self.pos][:, None].to(dtype), self.sin[self.pos][:, None].to(dtype)


def heads(t, B, S, Hn):
    """[B*S, Hn*64] -> [B,H,S,64]"""
    return t.reshape(B, S, Hn, DH).transpose(1, 2)


def rows2d(t):
    """[B,H,S,64] -> [B*S, Hn*64]"""
    B, Hn, S, _ = t.shape
    return t.transpose(1, 2).reshape(B * S, Hn * DH)


def split_qkv(qkv, B, S, Hn):
    t = qkv.reshape(B, S, 3, Hn, DH)
    return tuple(t[:, :, i].transpose(1, 2) for i in range(3))


def rotate(x, c, s, sign=1.0):
    """hf apply_rotary_pos_emb on [B,H,S,64] (pairs j <-> j + 32); sign = -1: the inverse (= transposed) rotation."""
    lo, up = x[..., :32], x[..., 32:]
    return torch.cat((lo * c - sign * up * s, up * c + sign * lo * s), -1)


def rotate_abs(b, c, s):
    return torch.cat((b[..., :32] * c.abs() + b[..., 32:] * s.abs(), b[..., 32:] * c.abs() + b[..., :32] * s.abs()), -1)


def delta_from_out(S, packed, rope):
    """k_attn_bwd :3526: S <= 32, or S <= 64 with q / k not rotated on load, and no key ranges -> attn_bwd_small_kernel /
    attn_bwd_long_kernel, which form delta from P and dP; every other launch reads out."""
    return not ((S <= 32 or (S <= 64 and rope != "load")) and not packed)


def round_flips(r, eps):
    """bf16(r) of the float64 r, and per element how far a kernel's bf16 value may lie from it when the kernel rounds an fp32 value within
    eps of r: 0, or - where r is within eps of a rounding boundary - one bf16 spacing."""
    rb = r.float().to(torch.bfloat16).double()
    sp = torch.exp2(torch.floor(torch.log2(rb.abs().clamp_min(TINY))) - 7)
    dist = (r - rb).abs()
    near = torch.minimum((dist - sp / 2).abs(), (dist - sp / 4).abs()) <= eps         # (sp / 4: the boundary below a power of two)
    return rb, torch.where(near, sp, torch.zeros_like(sp))


def _rotate_round(t, c, s):
    """bf16(rotation of t) from float64, and per element how far the kernel's value may lie from it: 0, or - where the exact value is
    within the fp32 rotation's error 4 u (|a c| + |b s|) (two products, one sum) of a rounding boundary - one bf16 spacing."""
    return round_flips(rotate(t, c, s), 4 * U * rotate_abs(t.abs(), c, s))


def operands64(pr, flips=False):
    """q, k, v [B,H,S,64] float64 as the kernels multiply them; flips: also the possible deviations fq, fk of the kernel's rotated q / k
    (zeros unless q / k are rotated on load)."""
    q, k, v = (t.double() for t in split_qkv(pr.qkv, pr.B, pr.S, pr.Hn))
    fq, fk = torch.zeros_like(q), torch.zeros_like(k)
    if pr.rope == "load":
        c, s = pr.angles(torch.float64)
        (q, fq), (k, fk) = _rotate_round(q, c, s), _rotate_round(k, c, s)
    return (q, k, v, fq, fk) if flips else (q, k, v)


def flip_scores(q, k, fq, fk):
    """How far a score x can move when the kernel's rotated q / k differ from the statement's by fq / fk."""
    return (fq @ k.abs().transpose(2, 3) + q.abs() @ fk.transpose(2, 3) + fq @ fk.transpose(2, 3)) / 8


# ------------------------------------------------------------------------------------------------------------------ forward
def forward64(pr):
    """Float64 statement and bounds of the forward: dict with out, out_bound [B,H,S,64], lse, lse_bound [B,H,S], the weights r."""
    S = pr.S
    q, k, v, fq, fk = operands64(pr, flips=True)
    r = R.attn_probs64(q, k, pr.allowed, pr.keep)
    pm = r["ref"]
    E = R.attn_exp_err(r, S)
    lse_b = U * (16 * r["W"] + R.attn_sum_const(S) + r["X"] + 3 * r["lse"].abs())
    if pr.rope == "load":
        F = flip_scores(q, k, fq, fk)
        Fl = (r["p"] * F).sum(-1)
        E = E + F + Fl[..., None]
        lse_b = lse_b + Fl
    out = pm @ v
    pv = pm @ v.abs()
    live = r["allowed"].double() @ v.abs()
    inner = BF * pv + (torch.expm1(E) * pm) @ v.abs() + (2 * S + math.ceil(S / 32) + 3) * U * pv
    bound = 2.0 ** -8 * out.abs() + 1.01 * inner + TINY * (1 + pr.m_max * live)
    return dict(out=out, out_bound=bound, lse=r["lse"], lse_bound=lse_b, r=r, v=v)


def forward_check(pr, out, lse, f=None, zero_rows=False):
    """out bf16 [B*S, d] and lse fp32 [B,H,S] of an implementation on the padded grid.  Every element of the rows that hold a token under
    its bound; a row with one allowed key and no dropout is that v row bit for bit; zero_rows: rows without a token (packed padding) are
    exact zeros in out and lse."""
    B, S, Hn = pr.B, pr.S, pr.Hn
    f = f or forward64(pr)
    g = heads(out, B, S, Hn)
    rows = pr.real_h
    res = [H.held("out", g[rows], f["out"][rows], f["out_bound"][rows]),
           H.held("lse", lse.reshape(B, Hn, S)[rows], f["lse"][rows], f["lse_bound"][rows])]
    ok = f["r"]["allowed"]
    none = rows & ~ok.any(-1)
    res.append(H.held_true("out: rows without an allowed key are zero", bool((g[none] == 0).all()), "a real row without keys is not zero"))
    if zero_rows:
        res.append(H.held_true("out, lse: rows without a token are zero", bool((g[~rows] == 0).all()) and bool((lse.reshape(B, Hn, S)[~rows] == 0).all()),
                               "a row without a token is not zero"))
    if pr.p == 0:
        one = rows & (ok.sum(-1) == 1)
        if bool(one.any()):
            key = ok.double().argmax(-1)                                                             # [B,H,S]
            vrow = torch.gather(heads(pr.qkv.view(B * S, 3, -1)[:, 2], B, S, Hn), 2, key[..., None].expand(B, Hn, S, DH))
            res.append(H.held_equal("out: a row with one allowed key is that v row", g[one].contiguous(), vrow[one].contiguous()))
    return res


# ------------------------------------------------------------------------------------------------------------------ backward
def backward64(pr, lse, out, from_out, slabs=0, dO=None, e_dO=None):
    """Float64 statement and bounds of dq, dk, dv [B,H,S,64] from the handed lse (fp32 [B,H,S]) and out (bf16 [B*S, d]).  from_out: delta =
    rowsum(dO o out), else sum_k p m dP.  slabs > 0: the fused form's per-slab bf16 rounding of dQ.  dO ([B*S, d], any float type): the
    output gradient in place of pr.dout; e_dO [B,H,S,64]: how far the kernel's own dO may lie from it (module docstring)."""
    B, S, Hn = pr.B, pr.S, pr.Hn
    q, k, v, fq, fk = operands64(pr, flips=True)
    ok = pr.allowed[:, None].expand(B, Hn, S, S)
    lse = lse.reshape(B, Hn, S).double().masked_fill(~pr.real_h, 0.0)[..., None]
    x = q @ k.transpose(2, 3) / 8.0
    A = q.abs() @ k.abs().transpose(2, 3)
    p = torch.exp((x - lse).masked_fill(~ok, float("-inf")))
    m = pr.keep.double() if pr.keep is not None else torch.ones_like(p)
    pm = p * m
    dO = heads(pr.dout if dO is None else dO, B, S, Hn).double()
    Eb = U * (16 * A + 2 * lse.abs() + x.abs() + (x - lse).abs() + 3)
    if pr.rope == "load":
        Eb = Eb + flip_scores(q, k, fq, fk)
    eE = torch.expm1(Eb).masked_fill(~ok, 0.0)
    dP = dO @ v.transpose(2, 3)
    e_dP = 128 * U * (dO.abs() @ v.abs().transpose(2, 3))
    if e_dO is not None:
        e_dP = e_dP + e_dO @ v.abs().transpose(2, 3)
    if from_out:
        o = heads(out, B, S, Hn).double()
        delta = (dO * o).sum(-1, keepdim=True)
        e_dl = 128 * U * (dO * o).abs().sum(-1, keepdim=True)
        if e_dO is not None:
            e_dl = e_dl + (e_dO * o.abs()).sum(-1, keepdim=True)
    else:
        delta = (pm * dP).sum(-1, keepdim=True)
        e_dl = (pm * e_dP + eE * pm * dP.abs() + 2 * S * U * pm * dP.abs()).sum(-1, keepdim=True)
    dS = p * (m * dP - delta)
    e_dS = 1.01 * ((BF + eE) * dS.abs() + p * (m * e_dP + e_dl) + 4 * U * p * (m * dP.abs() + delta.abs()))
    acc = 2 * S * U * 1.01
    ref = dict(dv=pm.transpose(2, 3) @ dO, dq=dS @ k / 8, dk=dS.transpose(2, 3) @ q / 8)
    aq, ak = dS.abs() @ k.abs() / 8, dS.abs().transpose(2, 3) @ q.abs() / 8
    inner = dict(dv=(1.01 * (BF + eE + 2 * U) * pm + acc * pm).transpose(2, 3) @ dO.abs(),
                 dq=e_dS @ k.abs() / 8 + acc * aq + dS.abs() @ fk / 8,
                 dk=e_dS.transpose(2, 3) @ q.abs() / 8 + acc * ak + dS.abs().transpose(2, 3) @ fq / 8)
    if e_dO is not None:
        inner["dv"] = inner["dv"] + 1.01 * pm.transpose(2, 3) @ e_dO
    if slabs:      # every 256-key partial of dQ is rounded to bf16: 2^-8 of the partial (its own error included), then summed in fp32
        part = sum((dS[..., 256 * i:256 * (i + 1)] @ k[:, :, 256 * i:256 * (i + 1)] / 8).abs() for i in range(slabs))
        inner["dq"] = inner["dq"] + 1.01 * BF * (part + inner["dq"]) + slabs * U * aq
    floor = dict(dv=TINY * (1 + pr.m_max * dO.abs().sum(2, keepdim=True)), dq=TINY * (1 + k.abs().sum(2, keepdim=True) / 8),
                 dk=TINY * (1 + q.abs().sum(2, keepdim=True) / 8))
    if pr.rope:
        c, s = pr.angles(torch.float64)
        for nm in ("dq", "dk"):
            g = ref[nm]
            inner[nm] = rotate_abs(inner[nm], c, s) + 4 * U * rotate_abs(g.abs(), c, s)
            floor[nm] = 2 * floor[nm]
            ref[nm] = rotate(g, c, s, -1.0)
    bound = {nm: 2.0 ** -8 * ref[nm].abs() + inner[nm] + floor[nm] for nm in ref}
    return dict(ref=ref, bound=bound)


def grads(dqkv, B, S, Hn):
    return dict(zip(("dq", "dk", "dv"), split_qkv(dqkv, B, S, Hn)))


def backward_check(pr, dqkv, lse, out, from_out, slabs=0, bw=None, pad_zero=True):
    """dqkv bf16 [B*S, 3 d] on the padded grid: every element of the rows that hold a token under its bound (a NaN left from a pre-filled
    buffer fails), rows without a token exact zeros (what the weight-gradient GEMM relies on; module docstring)."""
    bw = bw or backward64(pr, lse, out, from_out, slabs)
    g = grads(dqkv, pr.B, pr.S, pr.Hn)
    rows = pr.real_h
    res = [H.held(nm, g[nm][rows], bw["ref"][nm][rows], bw["bound"][nm][rows]) for nm in ("dq", "dk", "dv")]
    if pad_zero:
        pad = ~pr.real.reshape(-1)
        res.append(H.held_true("dqkv: rows without a token are zero", bool((dqkv[pad] == 0).all()), "a row without a token is not zero"))
    return res


def vacuous_share(ref, bound, rows):
    """Share of the real elements whose bound exceeds 0.05 (|ref| + rms of the element's row) - a bound that would accept anything.  A
    row whose rms is below 1 % of the rms of the tensor's real rows is held to the tensor's rms: a row with one live key (one allowed key, or one kept by the
    dropout) has p = 1, dS = p (1 - p) m dP and dq = dk = 0 up to the roundings of the handed lse and out - it has no scale of its own."""
    rms = ref.pow(2).mean(-1, keepdim=True).sqrt()
    whole = ref[rows].pow(2).mean().sqrt()
    rms = torch.where(rms <= 0.01 * whole, whole, rms)
    return float((bound > 0.05 * (ref.abs() + rms))[rows].double().mean())


def problem_rel_l2(got, ref, rows):
    """The per-(sample, head) rel-L2 of tests/test_gpu_ops.py:_per_problem_rel on [B,H,S,64], its maximum, and the rel-L2 over the whole
    tensor (what test_attention_dropout, _packed_ranges and _bwd_fused there take)."""
    w = rows[..., None].double()
    num = (((got.double() - ref) ** 2) * w).sum((2, 3))
    den = ((ref ** 2) * w).sum((2, 3))
    per = torch.where(den > 0, (num / den.clamp_min(1e-300)).sqrt(), num.sqrt())
    return float(per.max()), float((num.sum() / den.sum()).sqrt())


# ------------------------------------------------------------------------------------------------------------------ fp32 statements
FWD_FAULTS = ("key_len", "stage_last_key", "no_diagonal", "key_hi_exclusive", "row_scale", "keep_no_scale", "swap_fields", "swap_heads")
BWD_FAULTS = ("dk_no_scale", "delta_before_dropout", "dv_no_keep", "dq_slab_missing", "dq_rot_forward", "dk_last_row_zero")


def _operands32(pr):
    q, k, v = (t.float() for t in split_qkv(pr.qkv, pr.B, pr.S, pr.Hn))
    if pr.rope == "load":
        c, s = pr.angles(torch.float32)
        q, k = (rotate(t, c, s).to(torch.bfloat16).float() for t in (q, k))
    return q, k, v


def forward_fp32(pr, fault=None):
    """A plain fp32 CPU statement of the forward with the kernels' bf16 roundings (P o m, out): out bf16 [B*S, d], lse fp32 [B,H,S].
    fault: the planted faults of tests/test_attn_out_ref.py."""
    B, S, Hn = pr.B, pr.S, pr.Hn
    q, k, v = _operands32(pr)
    ok = pr.allowed
    pos = torch.arange(S)
    if fault == "key_len":              # key `len` allowed (the query limit stays right)
        ok = R.allowed_padded(B, S, [n + 1 for n in pr.lens], bool(pr.causal)) & pr.real[:, :, None]
    elif fault == "stage_last_key":     # the last key of the sample's last full 32-key stage dropped for the rows of the first query tile
        last = (torch.tensor(pr.lens) // 32 * 32 - 1)[:, None, None]
        ok = ok & ~((pos[None, :, None] < 32) & (pos[None, None, :] == last))
    elif fault == "no_diagonal":
        ok = ok & ~torch.eye(S, dtype=torch.bool)[None]
    elif fault == "key_hi_exclusive":
        ok = R.allowed_packed(pr.lo, pr.hi - 1, bool(pr.causal))
    ok4 = ok[:, None].expand(B, Hn, S, S)
    x = (q @ k.transpose(2, 3)) * 0.125
    xm = x.masked_fill(~ok4, float("-inf"))
    has = ok4.any(-1)
    lse = torch.logsumexp(xm.masked_fill(~has[..., None], 0.0), -1).masked_fill(~has, 0.0)
    p = torch.exp(xm - lse[..., None]).masked_fill(~ok4, 0.0)
    if pr.keep is not None:
        keep = pr.keep
        if fault == "keep_no_scale":
            keep = keep * (1.0 - pr.p)
        elif fault == "swap_fields":
            keep = R.attn_drop_keep(pr.dseed, B, Hn, S, pr.p, swap_fields=True)
        p = p * keep
    o = p.to(torch.bfloat16).float() @ v
    if fault == "row_scale":
        o[0, 0, min(5, S - 1)] *= 1.1
    elif fault == "swap_heads":
        o = o[:, [1, 0] + list(range(2, Hn))]
    o = o * pr.real_h[..., None]
    return rows2d(o).to(torch.bfloat16), lse.masked_fill(~pr.real_h, 0.0)


def backward_fp32(pr, lse, out, from_out, slabs=0, fault=None, dO=None):
    """The same of the backward (P o m and dS to bf16, outputs to bf16, per-slab dQ to bf16 for the fused form): dqkv bf16 [B*S, 3 d].
    dO ([B*S, d]): the output gradient in place of pr.dout."""
    B, S, Hn = pr.B, pr.S, pr.Hn
    q, k, v = _operands32(pr)
    ok = pr.allowed[:, None].expand(B, Hn, S, S)
    lse = lse.reshape(B, Hn, S).float().masked_fill(~pr.real_h, 0.0)[..., None]
    x = (q @ k.transpose(2, 3)) * 0.125
    p = torch.exp((x - lse).masked_fill(~ok, float("-inf")))
    m = pr.keep if pr.keep is not None else torch.ones_like(p)
    pm = p * m
    dO = heads(pr.dout if dO is None else dO, B, S, Hn).float()
    dP = dO @ v.transpose(2, 3)
    if fault == "delta_before_dropout":
        delta = (p * dP).sum(-1, keepdim=True)
    elif from_out:
        delta = (dO * heads(out, B, S, Hn).float()).sum(-1, keepdim=True)
    else:
        delta = (pm * dP).sum(-1, keepdim=True)
    dS = (p * (m * dP - delta) * 0.125).to(torch.bfloat16).float()
    dv = (p if fault == "dv_no_keep" else pm).to(torch.bfloat16).float().transpose(2, 3) @ dO
    if slabs:
        dq = torch.zeros_like(q)
        for i in range(slabs):
            if fault == "dq_slab_missing" and i == slabs - 1:
                continue
            dq = dq + (dS[..., 256 * i:256 * (i + 1)] @ k[:, :, 256 * i:256 * (i + 1)]).to(torch.bfloat16).float()
    else:
        dq = dS @ k
    dk = dS.transpose(2, 3) @ q
    if fault == "dk_no_scale":
        dk = dk * 8.0
    if pr.rope:
        c, s = pr.angles(torch.float32)
        dq = rotate(dq, c, s, 1.0 if fault == "dq_rot_forward" else -1.0)
        dk = rotate(dk, c, s, -1.0)
    if fault == "dk_last_row_zero":
        for b in range(B):
            dk[b, :, int(pr.real[b].nonzero().max())] = 0.0
    t = torch.stack([rows2d(g * pr.real_h[..., None]) for g in (dq, dk, dv)], 1)            # [B*S, 3, d]
    return t.reshape(B * S, -1).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ the case table
def _case(entry, B, S, Hn, lens=None, causal=0, p=0.0, kind="unit", rope=None, packed=False, tables=True):
    lens = None if packed else tuple(lens if lens is not None else [S] * B)
    c = dict(entry=entry, B=B, S=S, Hn=Hn, lens=lens, causal=causal, p=p, kind=kind, rope=rope, packed=packed, tables=tables)
    c["id"] = (f"{entry}-B{B}S{S}H{Hn}-" + ("packed" if packed else "len" + "_".join(map(str, lens))) + f"-c{causal}-p{p}-{kind}"
               + (f"-rope_{rope}" if rope else "") + ("" if tables else "-notab"))
    return c


def problem_of(c):
    return Problem(c["B"], c["S"], c["Hn"], lens=c["lens"], packed=c["packed"], causal=c["causal"], p=c["p"], kind=c["kind"], rope=c["rope"])


# (causal, p, kind): both masks and both dropout forms on both kinds, without the full product
COMBOS = ((0, 0.0, "unit"), (0, 0.0, "rising"), (1, 0.0, "rising"), (0, 0.1, "rising"), (1, 0.1, "unit"))
COMBOS_SHORT = COMBOS + ((1, 0.0, "peaked"),)                   # S <= 72
PADDED = [(1, 8, 1, (1,)), (3, 32, 2, (32, 17, 1)), (2, 40, 2, (33, 40)), (2, 64, 1, (64, 31)), (2, 72, 2, (65, 72)),
          (3, 160, 1, (160, 129, 97)), (1, 256, 2, (255,)), (2, 320, 1, (320, 129)), (2, 520, 1, (520, 263))]
VARLEN = [(3, 24, 2, (24, 1, 17)), (3, 40, 2, (40, 33, 1)), (3, 64, 1, (64, 32, 31)), (3, 64, 2, (47, 1, 33)), (2, 72, 1, (72, 33)),
          (2, 160, 1, (160, 97)), (2, 320, 1, (129, 320)), (2, 520, 1, (263, 520))]
ROPE_UNIT = ((0, 0.0, "unit"), (1, 0.1, "unit"))                 # rotated on load: "unit" only (a rotation undoes the other kinds' pattern)


def forward_cases():
    cs = []
    for B, S, Hn, lens in PADDED:
        for causal, p, kind in (COMBOS_SHORT if S <= 72 else COMBOS):
            cs.append(_case("fwd", B, S, Hn, lens, causal, p, kind))
    cs.append(_case("fwd", 2, 32, 12, (32, 17), 0, 0.1, "rising"))          # grid y = 12 heads
    for B, S, Hn, lens in ((2, 40, 2, (33, 40)), (2, 264, 1, (264, 131))):
        for causal, p, kind in ROPE_UNIT:
            cs.append(_case("fwd", B, S, Hn, lens, causal, p, kind, rope="load"))
    for B, S, Hn, lens in VARLEN:
        for causal, p, kind in COMBOS[1:] if S > 72 else COMBOS[1:4]:
            cs.append(_case("fwd_varlen", B, S, Hn, lens, causal, p, kind))
    for S in (40, 64, 160, 320):
        for causal, p, kind in COMBOS[:4]:
            cs.append(_case("fwd_ranges", 2, S, 2 if S < 160 else 1, None, causal, p, kind, packed=True))
    for Hn, S, causal, p in ((2, 32, 0, 0.0), (4, 24, 1, 0.1), (8, 32, 1, 0.0), (12, 32, 0, 0.1)):
        cs.append(_case("oproj_fwd", 2, S, Hn, (S, 17), causal, p, "rising"))
        cs.append(_case("oproj_fwd", 3, 16, Hn, (16, 1, 9), 1 - causal, 0.0, "unit"))
    return cs


# Backward at S >= 160: "rising" goes with the causal mask.  Without it every query of a sample puts its weight on the same last keys, and
# their dk / dv sum N >= 160 like-sized terms of either sign: the worst case of the bf16-rounded operands grows as 2^-8 N, the result
# as sqrt(N), and no count of roundings stays under the 5 % cap of tests/test_attn_out_ref.py.  The other mask runs on "unit".
BWD_SHORT = COMBOS[1:]
BWD_LONG = ((0, 0.0, "unit"), (1, 0.0, "rising"), (0, 0.1, "unit"), (1, 0.1, "rising"))
# (S = 520 without mask and dropout: the 520 like-sized terms of a dv element put 1.5 % of its "unit" bounds above the cap - that combination
#  stops at S = 320; at 520 the unmasked rows run with dropout)
BWD_520 = BWD_LONG[1:]


def backward_cases():
    cs = []
    for B, S, Hn, lens in PADDED:
        if S == 256:
            continue
        if S == 8:
            B, lens = 2, (8, 1)        # (a one-row sample alone has dq = dk = 0: nothing to hold a bound against)
        for causal, p, kind in (BWD_SHORT if S <= 72 else BWD_520 if S == 520 else BWD_LONG):
            cs.append(_case("bwd", B, S, Hn, lens, causal, p, kind))
    cs.append(_case("bwd", 2, 32, 12, (32, 17), 0, 0.1, "rising"))
    for B, S, Hn, lens in ((2, 40, 2, (33, 40)), (2, 160, 1, (160, 97))):
        for causal, p, kind in ROPE_UNIT:
            cs.append(_case("bwd", B, S, Hn, lens, causal, p, kind, rope="load"))
    for B, S, Hn, lens in ((3, 40, 2, (40, 33, 1)), (3, 64, 1, (64, 32, 31))):
        for causal, p, kind in ((0, 0.0, "rising"), (1, 0.1, "rising")):
            cs.append(_case("bwd_varlen", B, S, Hn, lens, causal, p, kind, rope="memory"))
        cs.append(_case("bwd_varlen", B, S, Hn, lens, 1, 0.0, "unit", tables=False))
    for B, S, Hn, lens in ((2, 160, 1, (160, 97)), (2, 320, 1, (129, 320))):
        for causal, p, kind in BWD_LONG[:3]:
            cs.append(_case("bwd_varlen", B, S, Hn, lens, causal, p, kind, rope="memory" if causal else None))
    for S in (40, 72, 160, 320, 520):
        for causal, p, kind in (BWD_SHORT[:3] if S <= 72 else BWD_LONG[1:]):
            cs.append(_case("bwd_ranges", 2, S, 2 if S < 160 else 1, None, causal, p, kind, packed=True))
    for B, S, Hn, lens in ((1, 256, 2, (255,)), (2, 320, 1, (320, 129)), (2, 520, 1, (520, 263))):
        for causal, p, kind in (BWD_520 if S == 520 else BWD_LONG[:2] + BWD_LONG[3:]):
            cs.append(_case("bwd_fused", B, S, Hn, lens, causal, p, kind))
        for causal, p, kind in BWD_LONG[1:3]:
            cs.append(_case("bwd_fused", 2, S, 1, None, causal, p, kind, packed=True))
    return cs


def slabs_of(c):
    """dQ slabs of 256 keys the fused entry sums (S >= 256; k_attn_bwd :3546), else 0."""
    return (c["S"] + 255) // 256 if c["entry"] == "bwd_fused" and c["S"] >= 256 else 0
