"""The two row-reduction kernel families of every pre-training step - RMSNorm (csrc/kernels.hip K4 and the LayerScale-fused forms of
csrc/residual.hip) and the cross-entropy (K14): seeded inputs, float64 statements of every operation on the bf16 / fp32 inputs the kernel
gets, the per-element error bounds and the checks that hold an implementation to them.  tests/test_gpu_rows.py feeds the checks with the
HIP kernels' outputs, tests/test_rows_reference.py with the fp32 CPU statements below (which must pass) and with planted faults (which
must not).

Bounds.  u = 2^-24 is fp32's unit roundoff, ub = 2^-8 the bf16 term of tests/_util.py:assert_elementwise; every bound adds TINY = 2^-126
(a flushed denormal).
 * rstd = (mean(x^2) + eps)^-1/2:  |err| <= (d/2 + 4) u |ref|.  Products of bf16 values are exact in fp32; their sum is within (d - 1) u
   of the exact one in any order; the divide and the eps add round once each; the square root halves the relative error of its argument;
   rsqrt is good to 1 ulp = 2 u:  (d - 1) / 2 + 1/2 + 1/2 + 2 < d/2 + 4.
 * y = w bf16(x rstd):  (1) with the rstd that was returned, bf16(w * bf16(fp32(x * rstd))) is one IEEE product and one RNE conversion,
   twice: bit for bit what the CPU computes (inputs in the normal range).  (2) |err| <= (2 x 1.01 ub + (d/2 + 6) u) |ref|: two bf16
   roundings, the error of rstd and the two products.
 * out = bf16(res + bf16(lam y)) of the fused forward: lam y is exact in fp32, the rest is one addition and two conversions: bit for bit.
   Its xn / rstd are held as y / rstd of x := the out that was written (the norm sees the rounded residual stream).
 * dx = dres + rs (g - xh m), g = dy w, xh = x rs, m = mean(g xh), A = mean|g xh|, rs an INPUT (the float64 value rounded to fp32):
   |err| <= 1.01 ub |ref| + 2 u [(d + 4) rs |xh| A + 4 (|dres| + rs (|g| + |xh| |m|))].  The first bracket is the d-term mean (products
   rounded once each, any order, the division) as it reaches the element; the second the four roundings of the element's own chain.
 * dw = dw0 + sum_r dy xh (and dlam = dlam0 + sum_r dx y):  |err| <= 2 (T + 1) u sum|term|, any order - the atomics over the `copies`
   replicas included, once the replicas are summed (here in float64).  The initial values count as a term.
 * dsc = bf16(lam bf16(dx)): a product of two bf16 values, exact on the CPU from the dx that was written; dlam's terms use that dx too.
 * Cross-entropy, per row with k = EXP_C0 + EXP_CX max_c|x_c - mx| + V (tests/_heads_ref.py):
     p:           |err| <= k u p + TINY
     row loss:    |err| <= L = u (2 max|x| + EXP_C0 + EXP_CX span + V + 4 |lse| + 4)
     p_t = exp(x_y - lse) as the focal weight computes it: the argument is minus the row loss (error L), the exponential adds
                  (EXP_C0 + EXP_CX |log p_t|) u relative:  dpt = p_t (L + (EXP_C0 + EXP_CX |log p_t|) u) + TINY
     focal weight f = om^gamma, om = 1 - p_t (one rounding: dom = dpt + u om), gamma in {1, 2} (for gamma < 1 the derivative is unbounded
                  at p_t -> 1): f is increasing and convex in om, so the propagated error is at most (om + dom)^gamma - om^gamma - the
                  first-order gamma om^(gamma - 1) dom plus its remainder dom^2 at gamma = 2 - and exp2(gamma log2 om) itself adds
                  (EXP_C0 + EXP_CX gamma |log om|) u f.
     row weight wr = sample_wgt[sel_tok[row] / S] f:  dwr = sample_wgt df + u |wr| (exactly 0 without weights and focal term).
     dlogits = (p - onehot) wr scale:  1.01 ub |ref| + (k u p + TINY + 2 u (p + onehot)) |wr scale| + |p - onehot| |scale| (dwr + 4 u |wr|)
                  - the last term, which vanishes for wr = 1, is the weight's own error, the product wr * scale and the division 1 / n.
     loss sum = sum_r wr loss_r:  sum_r (|wr| L_r + dwr |loss_r| + u |wr loss_r|) + n u sum_r |wr loss_r|.
     loss_out = loss sum * scale:  that bound times |scale|, plus 4 u |ref| (1 / n, the product).
"""
import torch

import _heads_ref
from _heads_ref import EXP_C0, EXP_CX, TINY, U, gen, head_logits, held_equal, held_true, randn_bf16, settle  # noqa: F401

UB = 2.0 ** -8
EPS = 1e-6
BF = torch.bfloat16


class Bounded(tuple):
    """A (name, max err / bound, failure text or None) that came from a bound - its ratio is a measurement, which a bit-for-bit or a
    yes / no check has none of."""


def held(name, got, ref64, bound64):
    return Bounded(_heads_ref.held(name, got, ref64, bound64))


def held_bits(name, got, want):
    """bf16 tensors, bit pattern for bit pattern (the sign of a zero included)."""
    assert got.dtype == BF and want.dtype == BF, (name, got.dtype, want.dtype)
    name, ratio, msg = held_equal(name, got.view(torch.int16), want.view(torch.int16))
    if msg is not None:
        at = (got.view(torch.int16) != want.view(torch.int16)).reshape(-1, got.shape[-1]).nonzero()[0]
        r, c = int(at[0]), int(at[1])
        msg += f" (bf16 values {float(got.reshape(-1, got.shape[-1])[r, c])!r} and {float(want.reshape(-1, got.shape[-1])[r, c])!r})"
    return name, ratio, msg


def align_up(x, a):
    return (x + a - 1) // a * a


def bf(t):
    """RNE to bf16 and back to fp32."""
    return t.to(BF).float()


# ------------------------------------------------------------------------------------------------------------------ RMSNorm forward
def rms_inputs(T, d, scale, seed, fused=False, lam=True):
    """x (or res, y, lam of the fused form) at `scale`; from T >= 3 on row 1 is all zeros (rstd = eps^-1/2) and row 2 holds a single
    non-zero.  Everything stays in bf16's normal range."""
    g = gen(seed)
    i = dict(T=T, d=d, eps=EPS, w=(torch.randn(d, generator=g) * 0.1 + 1).to(BF))
    x = randn_bf16(g, T, d, scale=scale)
    if not fused:
        if T >= 3:
            x[1] = 0
            x[2] = 0
            x[2, d - 3] = scale * 1.5
        i["x"] = x
        return i
    y = randn_bf16(g, T, d, scale=scale)
    i["lam"] = (torch.randn(d, generator=g) * 0.3 + 0.5).to(BF) if lam else None
    if T >= 3:
        x[1], y[1] = 0, 0
        x[2], y[2] = 0, 0
        y[2, d - 3] = scale * 1.5
    i["res"], i["y"] = x, y
    return i


def _norm_checks(x, w, eps, y_got, rstd_got, tag=""):
    d = x.shape[1]
    x64, w64 = x.double(), w.double()
    rs = (x64.pow(2).mean(1) + eps).rsqrt()
    ref = w64 * (x64 * rs[:, None])
    replay = (w.float() * bf(x.float() * rstd_got[:, None])).to(BF)
    return [held(f"rstd{tag}", rstd_got, rs, (d / 2 + 4) * U * rs.abs() + TINY),
            held_bits(f"y{tag} is bf16(w * bf16(x * rstd)) of the rstd returned", y_got, replay),
            held(f"y{tag}", y_got, ref, (2 * 1.01 * UB + (d / 2 + 6) * U) * ref.abs() + TINY)]


def rms_fwd_check(i, y, rstd):
    return _norm_checks(i["x"], i["w"], i["eps"], y, rstd)


def rms_fwd_fp32(i):
    x = i["x"].float()
    rstd = torch.rsqrt((x * x).sum(1) / i["d"] + i["eps"])
    return (i["w"].float() * bf(x * rstd[:, None])).to(BF), rstd


def ls_fwd_check(i, out, xn, rstd):
    return [held_bits("out is bf16(res + bf16(lam * y))", out, _ls_out(i))] + _norm_checks(out, i["w"], i["eps"], xn, rstd, tag=" (of out)")


def _ls_out(i):
    ly = i["y"].float() if i["lam"] is None else bf(i["lam"].float() * i["y"].float())
    return (i["res"].float() + ly).to(BF)


def ls_fwd_fp32(i):
    out = _ls_out(i)
    return (out,) + rms_fwd_fp32(dict(i, x=out))


# ------------------------------------------------------------------------------------------------------------------ RMSNorm backward
def bwd_inputs(T, d, dres, seed, copies=1, fused=False, lam=True):
    """dy, x, w, the float64 rstd rounded to fp32, the residual gradient (or None) and the initial values of the replicated accumulators
    ([copies][align_up(d, 128)]; the columns d.. of a replica belong to nobody)."""
    g = gen(seed)
    x = randn_bf16(g, T, d)
    i = dict(T=T, d=d, copies=copies, stride=align_up(d, 128), x=x, dy=randn_bf16(g, T, d), w=(torch.randn(d, generator=g) * 0.1 + 1).to(BF),
             rstd=(x.double().pow(2).mean(1) + EPS).rsqrt().float(), dres=randn_bf16(g, T, d) if dres else None,
             dw0=torch.randn(copies, d, generator=g))
    if fused:
        i["y"] = randn_bf16(g, T, d)
        i["lam"] = (torch.randn(d, generator=g) * 0.3 + 0.5).to(BF) if lam else None
        i["dlam0"] = torch.randn(copies, d, generator=g)
    return i


def _bwd_ref(i):
    """float64: dx with its bound, the dw terms' sum and absolute sum (without the initial values)."""
    d = i["d"]
    x, dy, w, rs = i["x"].double(), i["dy"].double(), i["w"].double(), i["rstd"].double()[:, None]
    xh, g = x * rs, dy * w
    gx = g * xh
    m, A = gx.mean(1, keepdim=True), gx.abs().mean(1, keepdim=True)
    core = rs * (g - xh * m)
    dres = i["dres"].double() if i["dres"] is not None else torch.zeros_like(x)
    ref = dres + core
    bound = 1.01 * UB * ref.abs() + 2 * U * ((d + 4) * rs * xh.abs() * A + 4 * (dres.abs() + rs * (g.abs() + xh.abs() * m.abs()))) + TINY
    t = dy * xh
    return ref, bound, t.sum(0), t.abs().sum(0)


def bwd_ref(i):
    """(computed once per inputs: the launch forms of one case share it)"""
    if "_ref" not in i:
        i["_ref"] = _bwd_ref(i)
    return i["_ref"]


def _accum_check(name, got, init, tsum, tabs, T):
    """got [copies, d] replicas (summed here in float64) against init.sum + the terms' sum."""
    ref = init.double().sum(0) + tsum
    return held(name, got.double().sum(0), ref, 2 * (T + 1) * U * (init.double().abs().sum(0) + tabs) + TINY)


def dw_pair_check(i, dw_only, dw_full):
    """The weight-gradient-only kernel against the full backward: both within the bound of the same float64 sum."""
    _, _, _, tabs = bwd_ref(i)
    bound = 2 * (2 * (i["T"] + 1) * U * (i["dw0"].double().abs().sum(0) + tabs) + TINY)
    return held("dw of the dw-only kernel against the full backward's", dw_only.double().sum(0), dw_full.double().sum(0), bound)


def rms_bwd_check(i, dx, dw):
    """dx bf16 [T, d] (None: the weight-gradient-only kernel), dw fp32 [copies, d]."""
    ref, bound, tsum, tabs = bwd_ref(i)
    out = [] if dx is None else [held("dx", dx, ref, bound)]
    return out + [_accum_check("dw", dw, i["dw0"], tsum, tabs, i["T"])]


def _dx_fp32(i, mean_div=None):
    x, dy, w, rs = i["x"].float(), i["dy"].float(), i["w"].float(), i["rstd"][:, None]
    xh, g = x * rs, dy * w
    m = (g * xh).sum(1, keepdim=True) / float(mean_div or i["d"])
    dres = i["dres"].float() if i["dres"] is not None else torch.zeros_like(x)
    return (dres + rs * (g - xh * m)).to(BF), dy * xh


def _replicas_fp32(i, init, terms, rows_per_block=16):
    """Block b = rows [16 b, 16 b + 16) adds its partial to replica b % copies."""
    out = init.clone()
    T = terms.shape[0]
    for b in range((T + rows_per_block - 1) // rows_per_block):
        out[b % i["copies"]] += terms[b * rows_per_block:(b + 1) * rows_per_block].sum(0)
    return out


def rms_bwd_fp32(i):
    dx, t = _dx_fp32(i)
    return dx, _replicas_fp32(i, i["dw0"], t)


def ls_bwd_check(i, dx, dw, dsc, dlam):
    """dlam None: the kernel was given no dlam accumulator."""
    ref, bound, tsum, tabs = bwd_ref(i)
    dxf = dx.float()
    want_dsc = dx if i["lam"] is None else (i["lam"].float() * dxf).to(BF)
    out = [held("dx", dx, ref, bound), _accum_check("dw", dw, i["dw0"], tsum, tabs, i["T"]),
           held_bits("dsc is bf16(lam * dx) of the dx written", dsc, want_dsc)]
    if dlam is not None:
        t = dxf.double() * i["y"].double()
        out.append(_accum_check("dlam", dlam, i["dlam0"], t.sum(0), t.abs().sum(0), i["T"]))
    return out


def ls_bwd_fp32(i):
    dx, t = _dx_fp32(i)
    dsc = dx if i["lam"] is None else (i["lam"].float() * dx.float()).to(BF)
    return dx, _replicas_fp32(i, i["dw0"], t), dsc, _replicas_fp32(i, i["dlam0"], dx.float() * i["y"].float())


# ------------------------------------------------------------------------------------------------------------------ cross-entropy
PAD_LOGIT = 60.0     # what the columns V..ld hold: a kernel that lets them into the softmax sum is off by e^60
CE_S = 8             # tokens per sample of sel_tok


def ce_inputs(rows, V, ld, seed):
    """bf16 logits [rows, ld] of magnitude about 4 with +60 in the pad columns; row 0 all equal, row 1 at +30, row 2 at -30, row 3
    alternating +-30; the label of row 4 at column 0, of row 5 at column V - 1, of row 6 at the row's maximum, of row 7 at its minimum.
    sel_tok: `rows` distinct tokens of ceil(rows / S) + 3 samples of S tokens in random (unsorted) order; one weight per sample."""
    g = gen(seed)
    x = head_logits(g, rows, V)
    labels = torch.randint(0, V, (rows,), generator=g)
    if rows >= 8:
        labels[4], labels[5], labels[6], labels[7] = 0, V - 1, int(x[6].argmax()), int(x[7].argmin())
    logits = torch.full((rows, ld), PAD_LOGIT, dtype=BF)
    logits[:, :V] = x.to(BF)
    n_samp = (rows + CE_S - 1) // CE_S + 3
    sel_tok = torch.randperm(n_samp * CE_S, generator=g)[:rows]
    assert rows < 8 or not bool((sel_tok[1:] // CE_S >= sel_tok[:-1] // CE_S).all())
    return dict(rows=rows, V=V, ld=ld, S=CE_S, logits=logits, labels=labels.to(torch.int32), sel_tok=sel_tok.to(torch.int32),
                sample_wgt=torch.rand(n_samp, generator=g) + 0.25)


def ce_grid(rows):
    """Blocks of the launch (k_ce_fwd_bwd: 32 rows per block, at most 2048)."""
    return max(1, min(2048, (rows + 31) // 32))


def ce_rows(i, n_rows_dev):
    return i["rows"] if n_rows_dev is None else max(0, min(i["rows"], n_rows_dev))


def ce_scale(n, mean_over_rows, scale_base):
    return (1.0 / n if n > 0 else 0.0) if mean_over_rows else scale_base


def ce_ref(i, n, gamma, weights, scale):
    """float64 over the first n rows: dlogits [n, ld] with its bound, the loss sum with its bound."""
    V = i["V"]
    if n == 0:
        return torch.zeros(0, i["ld"], dtype=torch.float64), torch.zeros(0, i["ld"], dtype=torch.float64), torch.tensor(0.0), torch.tensor(TINY)
    x = i["logits"][:n, :V].double()
    y = i["labels"][:n].long()
    mx = x.max(1, keepdim=True).values
    z = x - mx
    span = z.abs().max(1, keepdim=True).values
    se = z.exp().sum(1, keepdim=True)
    p, lse = z.exp() / se, mx + se.log()
    k = EXP_C0 + EXP_CX * span + V
    on = torch.zeros_like(p)
    on[torch.arange(n), y] = 1.0
    xy = (x * on).sum(1, keepdim=True)
    loss = lse - xy
    L = U * (2 * x.abs().max(1, keepdim=True).values + EXP_C0 + EXP_CX * span + V + 4 * lse.abs() + 4)
    sw = i["sample_wgt"].double()[(i["sel_tok"][:n].long() // i["S"])][:, None] if weights else torch.ones_like(loss)
    if gamma > 0:
        pt = (-loss).exp()
        dpt = pt * (L + (EXP_C0 + EXP_CX * loss.abs()) * U) + TINY
        om = (1 - pt).clamp_min(0)
        dom = dpt + U * om
        f = om.pow(gamma)
        df = (om + dom).pow(gamma) - f + (EXP_C0 + EXP_CX * gamma * om.clamp_min(1e-300).log().abs()) * U * f
    else:
        f, df = torch.ones_like(loss), torch.zeros_like(loss)
    wr = sw * f
    dwr = sw * df + (U * wr.abs() if (weights and gamma > 0) else 0.0)
    ws = wr * scale
    dl = torch.zeros(n, i["ld"], dtype=torch.float64)
    dl_bound = torch.zeros_like(dl)           # (pad columns: exactly zero)
    dl[:, :V] = (p - on) * ws
    dl_bound[:, :V] = (1.01 * UB * dl[:, :V].abs() + (k * U * p + TINY + 2 * U * (p + on)) * ws.abs()
                       + (p - on).abs() * abs(scale) * (dwr + (4 * U * wr.abs() if (weights or gamma > 0) else 0.0)) + TINY)
    t = wr * loss
    s = t.sum()
    s_bound = (wr.abs() * L + dwr * loss.abs() + U * t.abs()).sum() + n * U * t.abs().sum() + TINY
    return dl, dl_bound, s, s_bound


def ce_check(i, n, gamma, weights, scale, dlogits, loss_sum, loss_out, ref=None):
    """dlogits bf16 [rows, ld]: the first n rows are held (pad columns: exactly zero); the rows behind them belong to the caller."""
    dl, dl_bound, s, s_bound = ref if ref is not None else ce_ref(i, n, gamma, weights, scale)
    out = [held("dlogits", dlogits[:n], dl, dl_bound),
           held("loss_sum", loss_sum, s, s_bound)]
    if loss_out is not None:
        out.append(held("loss_out", loss_out, s * scale, s_bound * abs(scale) + 4 * U * abs(s * scale) + TINY))
    return out


def ce_fp32(i, n, gamma, weights, scale, label_shift=0, pad_in_sum=False, weight_by_row=False, focal_in_grad=True, zero_pad=True,
            fill=None):
    """The kernel's arithmetic in fp32 on the CPU (dlogits [rows, ld] bf16 with `fill` in what is not written); the keyword switches
    plant one fault each."""
    V, ld, rows = i["V"], i["ld"], i["rows"]
    cols = ld if pad_in_sum else V
    x = i["logits"][:n, :cols].float()
    y = (i["labels"][:n].long() + label_shift) % V
    mx = x.max(1, keepdim=True).values
    e = (x - mx).exp()
    se = e.sum(1, keepdim=True)
    lse = mx + se.log()
    xy = x.gather(1, y[:, None])
    sw = torch.ones(n, 1)
    if weights:
        idx = (torch.arange(n) % len(i["sample_wgt"])) if weight_by_row else i["sel_tok"][:n].long() // i["S"]
        sw = i["sample_wgt"][idx][:, None]
    f = (1 - (xy - lse).exp()).clamp_min(0).pow(gamma) if gamma > 0 else torch.ones(n, 1)
    w = sw * f
    on = torch.zeros_like(e)
    on[torch.arange(n), y] = 1.0
    dl = torch.full((rows, ld), float("nan") if fill is None else fill)
    dl[:n, :cols] = (e * (1.0 / se) - on) * ((w if focal_in_grad else sw) * torch.tensor(scale, dtype=torch.float32))
    if zero_pad:
        dl[:n, V:] = 0.0
    s = (w * (lse - xy)).sum()
    return dl.to(BF), s.reshape(1), (s * torch.tensor(scale, dtype=torch.float32)).reshape(1)


# ------------------------------------------------------------------------------------------------------------------ the cases
WIDTHS = (8, 72, 520, 768, 1024, 1032, 2048)
WIDTH_NOTE = {8: "one lane active", 72: "nine chunks", 520: "lane 0 alone in the second chunk", 768: "the headline width", 1024: "NCH = 2 full",
              1032: "the smallest NCH = 4", 2048: "NCH = 4 full"}
SCALES = (1e-3, 1.0, 30.0)

FWD_CASES = [(f"T{T}-d{d}: {WIDTH_NOTE[d]}", (T, d)) for d in WIDTHS for T in (1, 5, 37)] + [
    (f"T8197-d{d}: second trip of the pipelined row loop ({WIDTH_NOTE[d]})", (8197, d)) for d in (72, 1032)]

# form: "4wave" (KEY_RMS_WIDE = 0), "wide" (the 16-wave kernel), "nch4" (d > 1024: always the 4-wave kernel).  T = -1 / -2: 64 n_cu rows (the
# last launch the 16-wave form takes) / 64 n_cu + 1 (the first that falls back to the 4-wave form), n_cu from the device properties.
BWD_CASES = ([(f"4wave-T{T}-d{d}", ("4wave", T, d)) for d in (8, 72, 520, 768, 1024) for T in (1, 3, 70, 1030)]
             + [(f"wide-T{T}-d{d}", ("wide", T, d)) for d in (8, 72, 520, 768, 1024) for T in (1, 15, 16, 17, 23, 70)]
             + [("wide-T64ncu-d72: the last launch of the 16-wave form", ("wide", -1, 72)),
                ("wide-T64ncu+1-d72: one row past the 16-wave form (both forms give the same bits, so only the result is checked, not the dispatch)", ("wide", -2, 72))]
             + [(f"nch4-T{T}-d{d}", ("nch4", T, d)) for d in (1032, 2048) for T in (3, 70)])
DET_CASES = ([(f"det-T{T}-d{d}" + (": more than 64 blocks, two-level sum" if T == 1040 else ""), (T, d)) for d in (72, 1024, 1032) for T in (70, 1040)]
             + [("det-T65552-d72: grid at its 4096 cap", (65552, 72))])
LS_BWD_CASES = ([(f"ls4-T{T}-d{d}" + (": past the 1280-block grid" if T == 20500 else ""), (T, d, 0)) for d in (512, 768, 1024) for T in (3, 70, 20500)]
                + [(f"ls4-width-in-16-byte-form-T{T}-d{d}", (T, d, 1)) for d in (512, 768, 1024) for T in (3, 70, 20500)]
                + [(f"ls-T{T}-d{d}: rmsnorm_bwd_ls_kernel<{2 if d <= 1024 else 4}>", (T, d, 0)) for d in (72, 1032) for T in (3, 70, 20500)])

CE_GEOMETRIES = [  # V, ld, generic key
    ("V97-ld104: CH = 1, V not a multiple of 8", (97, 104, 0)),
    ("V512-ld512: V = ld", (512, 512, 0)),
    ("V756-ld768: CH = 2", (756, 768, 0)),
    ("V1500-ld1536: CH = 4", (1500, 1536, 0)),
    ("V2100-ld2104: generic, wide", (2100, 2104, 0)),
    ("V211-ld212: generic, ld % 8 != 0", (211, 212, 0)),
    ("V97-ld104-generic-key: generic by the menu key", (97, 104, 1)),
]
CE_ROWS, CE_BIG_ROWS = 70, 65541
CE_SCALE_BASE = 0.37
CE_LOSS_FORMS = ("parts", "parts-cap-short", "no-parts-buffer", "parts-key-off")


def ce_variants():
    """(n_rows_dev or None, mean_over_rows, gamma, weights) at rows = 70."""
    return [(nd, mean, gamma, wts) for nd in (None, CE_ROWS - 37, 0) for mean in (1, 0) for gamma in (0.0, 1.0, 2.0) for wts in (False, True)]


def fwd_case(T, d, scale, fused=False, lam=True):
    return rms_inputs(T, d, scale, seed=7000 + T + d + int(fused) * 2 + int(lam), fused=fused, lam=lam)


def bwd_case(T, d, dres, copies=1, fused=False, lam=True):
    return bwd_inputs(T, d, dres, seed=8000 + T + d + copies, copies=copies, fused=fused, lam=lam)


def ce_case(rows, V, ld):
    return ce_inputs(rows, V, ld, seed=9000 + rows + V + ld)
