"""Fine-tune heads and task losses (csrc/kernels.hip K15 and what follows it): seeded inputs, float64 statements of every operation,
the per-element error bounds and the checks that hold an implementation to them.  tests/test_gpu_heads.py feeds the checks with the
HIP kernels' outputs, tests/test_heads_reference.py with the fp32 CPU statements below (which must pass) and with planted faults
(which must not).

Bounds.  u = 2^-24 is fp32's unit roundoff.
 * Dot products: assert_elementwise's c_out 2^-8 |ref| + c_acc K u (|a| . |b|), K the number of terms (an accumulating output counts
   its initial value as one term).  c_acc = 2: any summation order of K terms is within (K - 1) u sum|term|, and a product of an fp32
   and a bf16 factor is itself rounded once (u) - together below 2 K u sum|term| to first order.
 * exp / log intrinsics: __expf(x) is exp2 of a rounded product, relative error about 1.45 |x| u from the argument plus a few ulp of
   the instruction.  A softmax probability p_c = e_c / sum e carries that error twice plus the C roundings of the sum, the reciprocal
   and the product: |p_c - ref| <= (EXP_C0 + EXP_CX max_c |x_c - mx| + C) u ref + 2^-126 (a flushed denormal).  A sigmoid is the C = 1
   case of it.  EXP_C0 = 4 and EXP_CX = 3 are the starting values (2 x 1.45 rounded up, and 2 x 2 ulp).
 * Scalar losses: sum over the terms of the term's own error, plus n_terms u sum|term| for the summation in any order.
"""
import math

import torch

from _util import assert_elementwise

U = 2.0 ** -24
TINY = 2.0 ** -126
EXP_C0, EXP_CX = 4.0, 3.0
# Phi(x) of csrc/common.h:gelu_parts: 7.5e-8 from the Abramowitz-Stegun 7.1.26 form itself, and about 10 fp32 roundings (reciprocal,
# four fma, two products, exp2 and its argument) relative to q <= 1/2 plus the one of 1 - q: 6 u.  The derivative adds x phi(x) <= 0.25
# with 4 more roundings and the argument error of exp2, (x^2 / 2) |x| phi(x) u <= 0.23 u: below 4 u in all.
PHI_ATOL = 7.5e-8 + 6 * U
GELU_GRAD_ATOL = PHI_ATOL + 4 * U


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn_bf16(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def pool_sample(g, B, rows):
    """B distinct rows of [0, rows), unsorted, row 0 and the last row among them (B = 1: the last row alone)."""
    if B == 1:
        return torch.tensor([rows - 1], dtype=torch.int32)
    inner = torch.randperm(rows - 2, generator=g)[:B - 2] + 1
    pr = torch.cat([torch.tensor([rows - 1]), inner, torch.tensor([0])])
    if B > 2:
        pr = pr[torch.randperm(B, generator=g)]
        if bool((pr[1:] > pr[:-1]).all()):
            pr = pr.flip(0)
    assert len(set(pr.tolist())) == B and 0 in pr.tolist() and rows - 1 in pr.tolist() and not bool((pr[1:] > pr[:-1]).all())
    return pr.to(torch.int32)


def head_logits(g, rows, C):
    """fp32 logits that bf16 holds exactly (the heads round them): magnitude about 4; row 0 all equal, row 1 at +30, row 2 at -30 and
    row 3 alternating +-30 (a softmax without the max subtraction overflows or underflows there), as far as there are rows."""
    x = torch.randn(rows, C, generator=g) * 4.0
    noise = torch.randn(4, C, generator=g)
    alt = torch.tensor([30.0 if c % 2 == 0 else -30.0 for c in range(C)])
    special = [torch.full((C,), 1.5), 30.0 + noise[1], -30.0 + noise[2], alt + noise[3]]
    for r in range(min(rows, 4)):
        x[r] = special[r]
    return x.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------------------------------ checks
def _as2d(t):
    return t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])


def held(name, got, ref64, bound64):
    """(name, max err / bound, failure text or None) of |got - ref| <= bound in every element."""
    got, ref64, bound64 = _as2d(got.double()), _as2d(ref64.double()), _as2d(bound64.double().expand_as(ref64))
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    err = (got - ref64).abs()
    bad = ~(err <= bound64)
    ratio = float((err / bound64.clamp_min(1e-300)).nan_to_num(float("inf")).max()) if err.numel() else 0.0
    if not bool(bad.any()):
        return name, ratio, None
    idx = bad.nonzero()
    ex = (err - bound64)[bad].nan_to_num(float("inf"))
    top = ex.argsort(descending=True)[:6].tolist()
    rows = sorted({int(r) for r in idx[:, 0].tolist()})
    cols = sorted({int(c) for c in idx[:, 1].tolist()})
    lines = [f"  ({int(idx[t, 0])}, {int(idx[t, 1])}): got {float(got[idx[t, 0], idx[t, 1]]):.9g} ref {float(ref64[idx[t, 0], idx[t, 1]]):.9g} "
             f"bound {float(bound64[idx[t, 0], idx[t, 1]]):.3g}" for t in top]
    return name, ratio, (f"{name}: {int(bad.sum())} of {bad.numel()} elements out of bound in {len(rows)} row(s) {rows[:8]} and "
                         f"{len(cols)} column(s) {cols[:8]}; worst:\n" + "\n".join(lines))


def held_dot(name, got, ref64, absprod64, K, c_out, c_acc, atol=0.0):
    """The same through assert_elementwise (its bound, its message with the tile coordinates)."""
    got, ref64, absprod64 = _as2d(got), _as2d(ref64.double()), _as2d(absprod64.double())
    atol = _as2d(atol.double()) if torch.is_tensor(atol) else atol
    bound = c_out * 2.0 ** -8 * ref64.abs() + c_acc * K * U * absprod64 + atol
    _, ratio, msg = held(name, got, ref64, bound)
    if msg is not None:
        try:
            assert_elementwise(got, ref64, absprod64, K, c_out=c_out, c_acc=c_acc, atol=atol, what=name)
        except AssertionError as e:
            msg = str(e)
    return name, ratio, msg


def held_equal(name, got, want):
    """Bit for bit (values compared, both NaN-free)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    same = got == want
    if bool(same.all()):
        return name, 0.0, None
    idx = (~_as2d(same)).nonzero()
    r, c = int(idx[0, 0]), int(idx[0, 1])
    return name, float("inf"), (f"{name}: {int((~same).sum())} of {same.numel()} elements differ, the first at ({r}, {c}): "
                                f"got {float(_as2d(got)[r, c])!r} want {float(_as2d(want)[r, c])!r}")


def held_true(name, ok, text):
    return name, 0.0 if ok else float("inf"), None if ok else f"{name}: {text}"


def settle(results):
    """(largest ratio, texts of the failed checks)."""
    return max([r for _, r, _ in results], default=0.0), [m for _, _, m in results if m is not None]


def must_hold(results):
    ratio, msgs = settle(results)
    assert not msgs, "\n".join(msgs)
    return ratio


# ------------------------------------------------------------------------------------------------------------------ pooled head
def score_inputs(B, C, d, bias, seed):
    g = gen(seed)
    rows = 2 * B + 3
    return dict(B=B, C=C, d=d, rows=rows, hidden=randn_bf16(g, rows, d), pool_row=pool_sample(g, B, rows), w=randn_bf16(g, C, d, scale=d ** -0.5),
                bias=randn_bf16(g, C) if bias else None, dlogits=torch.randn(B, C, generator=g), dw0=torch.randn(C, d, generator=g),
                db0=torch.randn(C, generator=g))


def _linear64(h, w, bias):
    ref, ab = h @ w.t(), h.abs() @ w.abs().t()
    if bias is not None:
        ref, ab = ref + bias.double(), ab + bias.double().abs()
    return ref, ab


def score_fwd_check(i, logits, pooled_h):
    h = i["hidden"][i["pool_row"].long()]
    ref, ab = _linear64(h.double(), i["w"].double(), i["bias"])
    return [held_dot("logits", logits, ref, ab, i["d"], 1, 2),
            held_equal("logits are bf16 values", logits, logits.to(torch.bfloat16).float()),
            held_equal("pooled_h", pooled_h, h)]


def score_fwd_fp32(i):
    h = i["hidden"][i["pool_row"].long()]
    y = h.float() @ i["w"].float().t()
    if i["bias"] is not None:
        y = y + i["bias"].float()
    return y.to(torch.bfloat16).float(), h.clone()


def score_bwd_check(i, dw, dbias, dhidden):
    pr, dl, w = i["pool_row"].long(), i["dlogits"].double(), i["w"].double()
    h = i["hidden"].double()[pr]
    ref = torch.zeros(i["rows"], i["d"], dtype=torch.float64)
    ab = torch.zeros_like(ref)
    ref[pr], ab[pr] = dl @ w, dl.abs() @ w.abs()
    out = [held_dot("dhidden", dhidden, ref, ab, i["C"], 1, 2),      # (rows outside pool_row: ref 0, bound 0)
           held_dot("dw", dw, i["dw0"].double() + dl.t() @ h, i["dw0"].double().abs() + dl.abs().t() @ h.abs(), i["B"] + 1, 0, 2)]
    if dbias is not None:
        out.append(held_dot("dbias", dbias, i["db0"].double() + dl.sum(0), i["db0"].double().abs() + dl.abs().sum(0), i["B"] + 1, 0, 2))
    return out


def score_bwd_fp32(i):
    pr, dl = i["pool_row"].long(), i["dlogits"]
    dh = torch.zeros(i["rows"], i["d"], dtype=torch.bfloat16)
    dh[pr] = (dl @ i["w"].float()).to(torch.bfloat16)
    return i["dw0"] + dl.t() @ i["hidden"].float()[pr], (i["db0"] + dl.sum(0)) if i["bias"] is not None else None, dh


# ------------------------------------------------------------------------------------------------------------------ token-level head
def tok_inputs(T, C, d, bias, seed):
    g = gen(seed)
    return dict(T=T, C=C, d=d, hidden=randn_bf16(g, T, d), w=randn_bf16(g, C, d, scale=d ** -0.5), bias=randn_bf16(g, C) if bias else None,
                dl=torch.randn(T, C, generator=g), dw0=torch.randn(C, d, generator=g), db0=torch.randn(C, generator=g))


def tok_score_fwd_check(i, logits):
    ref, ab = _linear64(i["hidden"].double(), i["w"].double(), i["bias"])
    return [held_dot("logits", logits, ref, ab, i["d"], 1, 2),
            held_equal("logits are bf16 values", logits, logits.to(torch.bfloat16).float())]


def tok_score_fwd_fp32(i):
    y = i["hidden"].float() @ i["w"].float().t()
    if i["bias"] is not None:
        y = y + i["bias"].float()
    return y.to(torch.bfloat16).float()


def tok_grad(i, inv_n):
    """bf16(dl * inv_n) - exact in fp32 for inv_n a power of two, so the documented intermediate rounding is reproduced, not bounded."""
    assert inv_n == 0.0 or math.frexp(inv_n)[0] == 0.5
    return (i["dl"] * inv_n).to(torch.bfloat16)


def tok_score_bwd_check(i, inv_n, dw, dbias, dhidden):
    if inv_n == 0.0:     # no labelled row: nothing flows
        out = [held_equal("dhidden", dhidden, torch.zeros(i["T"], i["d"], dtype=torch.bfloat16)), held_equal("dw", dw, i["dw0"])]
        return out + ([held_equal("dbias", dbias, i["db0"])] if dbias is not None else [])
    g, h, w = tok_grad(i, inv_n).double(), i["hidden"].double(), i["w"].double()
    out = [held_dot("dhidden", dhidden, g @ w, g.abs() @ w.abs(), i["C"], 1, 2),
           held_dot("dw", dw, i["dw0"].double() + g.t() @ h, i["dw0"].double().abs() + g.abs().t() @ h.abs(), i["T"] + 1, 0, 2)]
    if dbias is not None:
        out.append(held_dot("dbias", dbias, i["db0"].double() + g.sum(0), i["db0"].double().abs() + g.abs().sum(0), i["T"] + 1, 0, 2))
    return out


def tok_score_bwd_fp32(i, inv_n):
    g = tok_grad(i, inv_n).float()
    return i["dw0"] + g.t() @ i["hidden"].float(), (i["db0"] + g.sum(0)) if i["bias"] is not None else None, (g @ i["w"].float()).to(torch.bfloat16)


def tok_ce_inputs(T, C, seed, ignore=0.3, rows_map=False):
    """ignore: share of rows labelled -100 (1.0: every row).  rows_map: a compact layout of T rows over a logical grid of T + 37 label
    slots, whose last 5 rows (at most) are pad rows mapped at or past the grid's end."""
    g = gen(seed)
    n_logical = T + 37 if rows_map else T
    labels = torch.randint(0, C, (n_logical,), generator=g)
    labels[torch.rand(n_logical, generator=g) < ignore] = -100
    rm = None
    if rows_map:
        pad = min(5, T - 1)
        real = torch.randperm(n_logical, generator=g)[:T - pad].sort().values
        rm = torch.cat([real, n_logical + torch.arange(pad)]).to(torch.int32)
    lt = rm.long() if rows_map else torch.arange(T)
    if ignore < 1.0:      # the rows with the special logits carry a label
        first = lt[:min(T, 4)]
        first = first[first < n_logical]
        labels[first] = torch.randint(0, C, (len(first),), generator=g)
    return dict(T=T, C=C, logits=head_logits(g, T, C), labels=labels, rows_map=rm, n_logical=n_logical)


def tok_ce_row_labels(i):
    lt = i["rows_map"].long() if i["rows_map"] is not None else torch.arange(i["T"])
    inside = lt < i["n_logical"]
    y = torch.full((i["T"],), -100, dtype=torch.long)
    y[inside] = i["labels"][lt[inside]]
    return y


def _softmax64(x):
    """p, lse, mx and the constant k of the probability bound k u p + 2^-126, per row of float64 logits."""
    mx = x.max(1, keepdim=True).values
    z = x - mx
    se = z.exp().sum(1, keepdim=True)
    k = EXP_C0 + EXP_CX * z.abs().max(1, keepdim=True).values + x.shape[1]
    return z.exp() / se, mx + se.log(), mx, k


def _ce_terms(x, y):
    """Rows with label y >= 0: dl = p - onehot with its bound, the row loss lse - x_y with its own error (the error of log(sum e) is
    the relative error of the sum, k u; the two additions and their operands' magnitudes give the rest)."""
    p, lse, mx, k = _softmax64(x)
    on = torch.zeros_like(p)
    lab = y >= 0
    on[lab, y[lab]] = 1.0
    xy = (x * on).sum(1, keepdim=True)
    dl, dl_bound = p - on, k * U * p + TINY + U * on
    term = lse - xy
    term_err = (k + 4 * (mx.abs() + (lse - mx).abs() + xy.abs())) * U
    return dl, dl_bound, term.squeeze(1), term_err.squeeze(1), lab


def tok_ce_check(i, dl, stat, loss):
    y = tok_ce_row_labels(i)
    rdl, bdl, term, term_err, lab = _ce_terms(i["logits"].double(), y)
    rdl, bdl = rdl * lab[:, None], bdl * lab[:, None]        # unlabelled rows: exactly zero
    n = int(lab.sum())
    out = [held("dl", dl, rdl, bdl), held_equal("stat[1] (labelled rows)", stat[1], torch.tensor(float(n))),
           held_equal("stat[3]", stat[3], torch.tensor(0.0))]
    if n == 0:
        out += [held_equal("stat[0]", stat[0], torch.tensor(0.0)), held_equal("stat[2]", stat[2], torch.tensor(0.0)),
                held_true("loss", bool(torch.isnan(loss).all()), f"no labelled row must give NaN, got {float(loss)}")]
        return out
    s = term[lab].sum()
    s_bound = term_err[lab].sum() + n * U * term[lab].abs().sum()
    # (1 / n: correctly rounded, u, or the compiler's fast division, 2.5 ulp = 5 u)
    out += [held("stat[0] (loss sum)", stat[0], s, s_bound), held("stat[2] (1/n)", stat[2], torch.tensor(1.0 / n), torch.tensor(5 * U / n)),
            held("loss", loss, s / n, s_bound / n + 2 * U * (s / n).abs())]
    return out


def tok_ce_fp32(i):
    y = tok_ce_row_labels(i)
    x, lab = i["logits"], y >= 0
    p = torch.softmax(x, 1)
    on = torch.zeros_like(p)
    on[lab, y[lab]] = 1.0
    dl = (p - on) * lab[:, None]
    rows = (torch.logsumexp(x, 1) - (x * on).sum(1))[lab]
    n = float(lab.sum())
    s = rows.sum()
    stat = torch.stack([s, torch.tensor(n), torch.tensor(1.0 / n if n else 0.0), torch.tensor(0.0)])
    return dl, stat, (s / n if n else torch.tensor(float("nan"))).reshape(1)


# ------------------------------------------------------------------------------------------------------------------ task loss
SINGLE, L1, MSE, MULTI = 0, 1, 2, 3      # GGET_PROBLEM_* of include/gget.h


def task_inputs(problem, B, C, seed, weights=False, nan=0.0):
    g = gen(seed)
    x = head_logits(g, B, C)
    i = dict(problem=problem, B=B, C=C, logits=x, sample_wgt=None)
    if problem == SINGLE:
        i["labels"] = torch.randint(0, C, (B,), generator=g)
        if weights:
            i["sample_wgt"] = torch.rand(B, generator=g) + 0.25
    elif problem in (L1, MSE):
        y = x + torch.randn(B, C, generator=g)
        same = torch.rand(B, C, generator=g) < 0.15         # logits == labels: L1's sign is 0 there
        same.view(-1)[0] = B * C > 1
        i["labels"] = torch.where(same, x, y)
    else:
        y = torch.randint(0, 2, (B, C), generator=g).float()
        drop = torch.rand(B, C, generator=g) < nan
        if 0.0 < nan < 1.0:
            drop.view(-1)[0] = False       # (at least one labelled entry, at least one not)
            drop.view(-1)[-1] = B * C > 1
        y[drop] = float("nan")
        i["labels"] = y
    return i


def task_loss_check(i, loss, dlogits):
    x, B, C, problem = i["logits"].double(), i["B"], i["C"], i["problem"]
    if problem == SINGLE:
        rdl, bdl, term, term_err, _ = _ce_terms(x, i["labels"])
        if i["sample_wgt"] is not None:     # weight sw_b / sum(sw): the sum's (B - 1) u, the division and the product
            sw = i["sample_wgt"].double()
            wgt, kw = sw / sw.sum(), B + 3
        else:
            wgt, kw = torch.full((B,), 1.0 / B, dtype=torch.float64), 3
        ref = rdl * wgt[:, None]
        terms = term * wgt
        return [held("dlogits", dlogits, ref, bdl * wgt[:, None] + kw * U * ref.abs()),
                held("loss", loss, terms.sum(), (term_err * wgt + kw * U * terms.abs()).sum() + B * U * terms.abs().sum())]
    if problem in (L1, MSE):
        n = B * C
        df = x - i["labels"].double()
        # df, the term and 1 / n are rounded once each, the square once more: 4 u (L1) and 6 u (MSE) per term; the gradient 2 u and 4 u
        if problem == L1:
            terms, ref, kt, kg = df.abs() / n, df.sign() / n, 4, 2
        else:
            terms, ref, kt, kg = df * df / n, 2 * df / n, 6, 4
        return [held("dlogits", dlogits, ref, kg * U * ref.abs()),
                held("loss", loss, terms.sum(), kt * U * terms.sum() + n * U * terms.sum())]
    y = i["labels"].double()
    lab = ~torch.isnan(y)
    n = int(lab.sum())
    if n == 0:      # BCEWithLogitsLoss over an empty selection
        return [held_equal("dlogits", dlogits, torch.zeros(B, C)),
                held_true("loss", bool(torch.isnan(loss).all()), f"every label NaN must give NaN, got {float(loss)}")]
    y0 = torch.where(lab, y, torch.zeros_like(y))
    s = torch.sigmoid(x)
    k = EXP_C0 + EXP_CX * x.abs() + 1
    ref = (s - y0) / n * lab
    bdl = ((k * U * s + 2 * U * (s - y0).abs()) / n + 2 * U * ref.abs() + TINY) * lab
    e = (-x.abs()).exp()
    terms = (x.clamp_min(0) - x * y0 + torch.log1p(e)) / n * lab
    term_err = (k * U * e / (1 + e) + 4 * U * (x.abs() + torch.log1p(e))) / n * lab
    return [held("dlogits", dlogits, ref, bdl), held("loss", loss, terms.sum(), term_err.sum() + n * U * terms.abs().sum())]


def task_loss_fp32(i):
    x, B, C, problem = i["logits"], i["B"], i["C"], i["problem"]
    if problem == SINGLE:
        p = torch.softmax(x, 1)
        on = torch.nn.functional.one_hot(i["labels"], C).float()
        wgt = i["sample_wgt"] / i["sample_wgt"].sum() if i["sample_wgt"] is not None else torch.full((B,), 1.0 / B)
        return ((torch.logsumexp(x, 1) - (x * on).sum(1)) * wgt).sum().reshape(1), (p - on) * wgt[:, None]
    if problem in (L1, MSE):
        df = x - i["labels"]
        inv = 1.0 / (B * C)
        if problem == L1:
            return (df.abs() * inv).sum().reshape(1), df.sign() * inv
        return (df * df * inv).sum().reshape(1), 2 * df * inv
    y = i["labels"]
    lab = ~torch.isnan(y)
    n = float(lab.sum())
    if n == 0:
        return torch.tensor([float("nan")]), torch.zeros(B, C)
    y0 = torch.where(lab, y, torch.zeros_like(y))
    terms = (x.clamp_min(0) - x * y0 + torch.log1p((-x.abs()).exp())) / n * lab
    return terms.sum().reshape(1), (torch.sigmoid(x) - y0) / n * lab


# ------------------------------------------------------------------------------------------------------------------ AUC surrogate
def auc_inputs(B, num_neg, seed, C=2, labels="mixed"):
    g = gen(seed)
    y = torch.randint(0, 2, (B,), generator=g)
    y[0], y[-1] = 1, 0
    if labels != "mixed":
        y[:] = 1 if labels == "no_negative" else 0
    return dict(B=B, C=C, num_neg=num_neg, logits=head_logits(g, B, C), labels=y)


def auc_pairing(i, idx):
    """(positive row, negative row) of every pair; idx = modeling.auc_pairs(labels, num_neg, seed)."""
    pos, neg = (i["labels"] != 0).nonzero().view(-1), (i["labels"] == 0).nonzero().view(-1)
    cnt = len(pos) * i["num_neg"]
    if cnt == 0 or len(neg) == 0:
        return pos, neg, None, None
    return pos, neg, pos[torch.arange(cnt) // i["num_neg"]], neg[torch.as_tensor(idx).long()]


def auc_check(i, idx, loss, dlogits, lists_pos, lists_neg):
    B, C = i["B"], i["C"]
    pos, neg, bp, bn = auc_pairing(i, idx)
    out = [held_equal("lists (positives)", lists_pos, pos.to(torch.int32)), held_equal("lists (negatives)", lists_neg, neg.to(torch.int32))]
    if bp is None:      # torch's mean over no pair
        return out + [held_equal("dlogits", dlogits, torch.zeros(B, C)),
                      held_true("loss", bool(torch.isnan(loss).all()), f"no pair must give NaN, got {float(loss)}")]
    x = i["logits"].double()
    y = x[:, 1] - x[:, 0]
    cnt = len(bp)
    t = 1 - (y[bp] - y[bn])
    # t carries the roundings of y_p, y_n, their difference and 1 - d: u (2 |y_p| + 2 |y_n| + |t|); g = 2 t / cnt two more, t^2 / cnt three
    t_err = 2 * U * (y[bp].abs() + y[bn].abs() + 1 + t.abs())
    g = 2 * t / cnt
    g_err = 2 * t_err / cnt + 3 * U * g.abs()
    ref, ab, er, nt = (torch.zeros(B * C, dtype=torch.float64) for _ in range(4))
    for rows, col, sign in ((bp, 1, -1.0), (bp, 0, 1.0), (bn, 1, 1.0), (bn, 0, -1.0)):
        at = rows * C + col
        ref.index_add_(0, at, sign * g)
        ab.index_add_(0, at, g.abs())
        er.index_add_(0, at, g_err)
        nt.index_add_(0, at, torch.ones_like(g))
    terms = t * t / cnt
    return out + [held("dlogits", dlogits, ref.view(B, C), (er + nt * U * ab).view(B, C)),      # (columns past 1: ref 0, bound 0)
                  held("loss", loss, terms.sum(), (2 * t.abs() * t_err / cnt + 4 * U * terms).sum() + cnt * U * terms.sum())]


def auc_fp32(i, idx):
    B, C = i["B"], i["C"]
    pos, neg, bp, bn = auc_pairing(i, idx)
    if bp is None:
        return torch.tensor([float("nan")]), torch.zeros(B, C), pos.to(torch.int32), neg.to(torch.int32)
    x = i["logits"]
    y = x[:, 1] - x[:, 0]
    inv = 1.0 / len(bp)
    t = 1 - (y[bp] - y[bn])
    g = 2 * t * inv
    dl = torch.zeros(B * C)
    for rows, col, sign in ((bp, 1, -1.0), (bp, 0, 1.0), (bn, 1, 1.0), (bn, 0, -1.0)):
        dl.index_add_(0, rows * C + col, sign * g)
    return (t * t * inv).sum().reshape(1), dl.view(B, C), pos.to(torch.int32), neg.to(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ MLP head
def head_inputs(B, Din, Dout, bias, seed):
    g = gen(seed)
    x = torch.randn(B, Din, generator=g) * 1.5
    x[0, 0], x[0, 1], x[0, 2] = -6.0, 6.0, 0.0          # both tails of the activation and its origin
    return dict(B=B, Din=Din, Dout=Dout, x=x.to(torch.bfloat16), w=randn_bf16(g, Dout, Din, scale=Din ** -0.5),
                bias=randn_bf16(g, Dout) if bias else None, dy=torch.randn(B, Dout, generator=g), dw0=torch.randn(Dout, Din, generator=g),
                db0=torch.randn(Dout, generator=g))


def _phi64(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0))


def head_fwd_check(i, a, y, y32):
    """a = bf16(gelu(x)) against float64; y against the float64 product of the a that was produced (so each stage answers for itself)."""
    x = i["x"].double()
    ra = x * _phi64(x)
    ref, ab = _linear64(a.double(), i["w"].double(), i["bias"])
    return [held("a", a, ra, 2.0 ** -8 * ra.abs() + 1.01 * (x.abs() * PHI_ATOL + U * ra.abs())),
            held_dot("y", y, ref, ab, i["Din"], 1, 2), held_equal("y32", y32, y.float())]


def head_fwd_fp32(i):
    x = i["x"].float()
    a = (x * 0.5 * torch.erfc(-x / math.sqrt(2.0))).to(torch.bfloat16)
    y = a.float() @ i["w"].float().t()
    if i["bias"] is not None:
        y = y + i["bias"].float()
    y = y.to(torch.bfloat16)
    return a, y, y.float()


def head_bwd_check(i, a, dx, dw, dbias):
    x, dy, w, B = i["x"].double(), i["dy"].double(), i["w"].double(), i["B"]
    gp = _phi64(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    s = dy @ w
    ref = s * gp
    out = [held_dot("dx", dx, ref, (dy.abs() @ w.abs()) * gp.abs(), i["Dout"], 0, 2, atol=s.abs() * GELU_GRAD_ATOL + 3 * U * ref.abs()),
           held_dot("dw", dw, i["dw0"].double() + dy.t() @ a.double(), i["dw0"].double().abs() + dy.abs().t() @ a.double().abs(), B + 1, 0, 2)]
    if dbias is not None:
        out.append(held_dot("dbias", dbias, i["db0"].double() + dy.sum(0), i["db0"].double().abs() + dy.abs().sum(0), B + 1, 0, 2))
    return out


def head_bwd_fp32(i, a):
    x, dy = i["x"].float(), i["dy"]
    gp = 0.5 * torch.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return (dy @ i["w"].float()) * gp, i["dw0"] + dy.t() @ a.float(), (i["db0"] + dy.sum(0)) if i["bias"] is not None else None


# ------------------------------------------------------------------------------------------------------------------ the cases
# (id, arguments): the smallest shapes that reach each branch of the kernels, the branch named in the id.  Shared by the GPU test and
# by the host-side test of these references, which runs the same inputs.
SCORE_CASES = [  # B, C, d, bias
    ("B1-C1-d64: one row, one class, one 64-lane pass", (1, 1, 64, True)),
    ("B1-C5-d768: per = 1, slices 1..15 empty; d > 256 in the backward's column loop", (1, 5, 768, False)),
    ("B15-C2-d128: per = 1, slice 15 empty", (15, 2, 128, False)),
    ("B17-C5-d128: per = 2, slice 8 holds one row, slices 9..15 empty", (17, 5, 128, True)),
    ("B17-C128-d1024: 128 classes, widest row", (17, 128, 1024, False)),
    ("B33-C1-d128: per = 3, slices 11..15 empty", (33, 1, 128, True)),
    ("B33-C2-d768", (33, 2, 768, True)),
    ("B300-C128-d64: B > 256, per = 19, last slice 15 rows", (300, 128, 64, False)),
    ("B300-C5-d1024", (300, 5, 1024, True)),
]

TOK_CASES = [  # T, C, d, bias
    ("T1-C1-d64: one row of a wave's four, nc = 1", (1, 1, 64, True)),
    ("T3-C7-d128: T % 4 tail, C % 8 tail", (3, 7, 128, False)),
    ("T16-C8-d128: exactly one block of rows, one class group", (16, 8, 128, True)),
    ("T17-C9-d64: T % 16 tail (second block holds one row), second class group holds one class", (17, 9, 64, True)),
    ("T17-C65-d1024: second c0 round holds one class, nc = 16 = kTokMaxCols, four j0 rounds", (17, 65, 1024, False)),
    ("T511-C64-d128: one slab less a row, a full c0 round (lane 63 hand-off)", (511, 64, 128, True)),
    ("T513-C65-d768: second slab holds one row, nc = 12, three j0 rounds", (513, 65, 768, False)),
    ("T513-C7-d64", (513, 7, 64, True)),
    ("T1030-C130-d1024: three slabs, three c0 rounds, dbias taken at j == 0 of four j0 rounds", (1030, 130, 1024, True)),
    ("T1030-C9-d768: dbias with three j0 rounds", (1030, 9, 768, True)),
]

TOK_CE_CASES = [  # T, C, share of rows labelled -100, rows_map
    ("T1-C1: one labelled row, one class (p = 1)", (1, 1, 0.0, False)),
    ("T3-C7", (3, 7, 0.3, False)),
    ("T16-C8", (16, 8, 0.3, False)),
    ("T17-C9", (17, 9, 0.3, False)),
    ("T17-C7-all-ignored: loss NaN, dl zeros, stat[2] = 0", (17, 7, 1.0, False)),
    ("T511-C64: two blocks, the second partly idle", (511, 64, 0.3, False)),
    ("T513-C65: a third block with one row", (513, 65, 0.3, False)),
    ("T513-C9-rows_map: compact rows, the last 5 map at or past n_logical", (513, 9, 0.3, True)),
    ("T1030-C130", (1030, 130, 0.3, False)),
    ("T300000-C2: past one grid-stride round of 1024 x 256 rows", (300000, 2, 0.3, False)),
]

TASK_CASES = [  # problem, B, C, sample weights, share of NaN labels
    ("single-B1-C2: one busy thread in the 256-wide tree", (SINGLE, 1, 2, False, 0.0)),
    ("single-B6-C5-weights", (SINGLE, 6, 5, True, 0.0)),
    ("single-B255-C1: one idle thread", (SINGLE, 255, 1, False, 0.0)),
    ("single-B255-C2-weights", (SINGLE, 255, 2, True, 0.0)),
    ("single-B257-C128: second round of b += 256 holds one row", (SINGLE, 257, 128, False, 0.0)),
    ("single-B1000-C5-weights: four rounds, the last partly idle; weight sum over four rounds", (SINGLE, 1000, 5, True, 0.0)),
    ("l1-B6-C1: sign 0 where logits == labels", (L1, 6, 1, False, 0.0)),
    ("l1-B257-C3", (L1, 257, 3, False, 0.0)),
    ("l1-B1000-C1", (L1, 1000, 1, False, 0.0)),
    ("mse-B1-C1", (MSE, 1, 1, False, 0.0)),
    ("mse-B255-C3", (MSE, 255, 3, False, 0.0)),
    ("mse-B1000-C1", (MSE, 1000, 1, False, 0.0)),
    ("multi-B6-C5-no-nan", (MULTI, 6, 5, False, 0.0)),
    ("multi-B257-C128-no-nan", (MULTI, 257, 128, False, 0.0)),
    ("multi-B1-C2-nan40", (MULTI, 1, 2, False, 0.4)),
    ("multi-B255-C5-nan40", (MULTI, 255, 5, False, 0.4)),
    ("multi-B1000-C128-nan40: ogbg-molpcba's label width, count over 500 rounds", (MULTI, 1000, 128, False, 0.4)),
    ("multi-B6-C5-all-nan: loss NaN, dlogits zeros", (MULTI, 6, 5, False, 1.0)),
    ("multi-B257-C128-all-nan", (MULTI, 257, 128, False, 1.0)),
]

AUC_CASES = [  # B, num_neg, C, labels
    ("B24-neg4: the fixture's shape, under 256 pairs", (24, 4, 2, "mixed")),
    ("B24-neg4-C3: a third logit column stays out of it (dlogits zero there)", (24, 4, 3, "mixed")),
    ("B300-neg8: B > 256 (per = 2 in the list building), over 1000 pairs", (300, 8, 2, "mixed")),
    ("B1000-neg8: per = 4, about 4000 pairs", (1000, 8, 2, "mixed")),
    ("B24-no-positive: loss NaN, dlogits zeros", (24, 4, 2, "no_positive")),
    ("B24-no-negative: loss NaN, dlogits zeros", (24, 4, 2, "no_negative")),
]
HEAD_CASES = [(f"{name}-{'bias' if bias else 'nobias'}", (*shape, bias)) for bias in (True, False) for name, shape in (
    ("B1-128to64: columns < 256", (1, 128, 64)), ("B17-768to256: three rounds of the column loops", (17, 768, 256)),
    ("B33-256to1: a single output", (33, 256, 1)), ("B300-128to128: B > 256", (300, 128, 128)))]   # B, Din, Dout, bias
AUC_SEED = 77


def score_case(B, C, d, bias):
    return score_inputs(B, C, d, bias, seed=1000 + B + C + d)


def tok_case(T, C, d, bias):
    return tok_inputs(T, C, d, bias, seed=2000 + T + C + d)


def tok_ce_case(T, C, ignore, rows_map):
    return tok_ce_inputs(T, C, seed=3000 + T + C, ignore=ignore, rows_map=rows_map)


def task_case(problem, B, C, weights, nan):
    return task_inputs(problem, B, C, seed=4000 + 7 * problem + B + C, weights=weights, nan=nan)


def auc_case(B, num_neg, C, labels):
    return auc_inputs(B, num_neg, seed=5000 + B + C, C=C, labels=labels)


def head_case(B, Din, Dout, bias):
    return head_inputs(B, Din, Dout, bias, seed=6000 + B + Din + Dout)
