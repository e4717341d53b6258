"""Contrastive pre-training head (csrc/contrastive.hip: gget_op_cl_embed_fwd, gget_op_cl_loss_fwd, gget_op_cl_bwd): seeded inputs,
float64 statements of the three operations, the per-element error bounds and the checks that hold an implementation to them.
tests/test_gpu_cl_head.py feeds the checks with the HIP kernels' outputs, tests/test_cl_reference.py with the fp32 CPU statements
below (which must pass) and with planted faults (which must not).

What the reference computes (src/models/graphgpt/modeling_helpers.py:201-227, src/utils/loss_utils.py:107-167), restated:
  z_b = cl_proj(h_b), h_b the final-norm output at the pooled row; e_b = z_b / max(|z_b|, 1e-12)
  left = e[0::2], right = e[1::2]; with world > 1 both are all-gathered and concatenated in rank order
  left_new = hstack([left, right]).reshape(-1, d), right_new = hstack([right, left]).reshape(-1, d): row 2m of left_new is left[m], row
  2m + 1 is right[m], and right_new[j] = left_new[j ^ 1]
  scores = 20 left_new right_new^T; scores[i][i ^ 1] = finfo.min; loss = 0.5 (CE(scores, arange) + CE(scores^T, arange)); times ratio_dis
Row mapping for world > 1: gathered-left[m] with m = r B/2 + m' is sample 2 m' of rank r, so sample b of rank r sits at row
2 m + (b & 1) = r B + b of left_new (`gathered_positions`; tests/test_cl_reference.py checks dp.gather_cl_embeddings against the literal
hstack / reshape).  Gradient returns to the local rows only (GatherLayer.backward).

Bounds follow tests/_heads_ref.py.  u = 2^-24.
 * Dot products: c_out 2^-8 |ref| + 2 K u sum|a||b| (c_out = 0 for the fp32 outputs z, dz, dW; 1 for the bf16 dhidden, which is ONE
   rounding of an fp32 sum: the value already in the buffer counts as one more term).
 * exp / log: an exp of argument x carries (EXP_C0 + EXP_CX |x|) u relative.  The row log-sum-exp is taken online: every term passes its
   own exp, and a wave rescales its running sum at most once per key it meets (each an exp again, whose arguments telescope to at most
   the row's score range), plus N additions: relative error of the sum <= (EXP_C0 + 2 EXP_CX range + (EXP_C0 + 2) N) u, which is the
   absolute error of its log.  log-sum-exp is 1-Lipschitz in the largest score error.
 * Scalar loss: the sum of the row terms' bounds plus N u sum|term| for the summation, scaled by ratio / N.
 * Everything downstream of a bounded quantity propagates that bound linearly (first order), as written next to each check.
"""
import torch

import _heads_ref as H
from _heads_ref import EXP_C0, EXP_CX, TINY, U, gen, held, held_dot, held_equal, pool_sample, randn_bf16  # noqa: F401

TEMP = 20.0
EPS = 1e-12
RATIO = 0.5                       # ratio_dis beside the generative head
UPSTREAM = 1.25                   # upstream gradient of head2_loss in the backward cases (scale = UPSTREAM * RATIO)
MASKED = float(torch.finfo(torch.float32).min)

# (N, d): one pair; a block of partial query rows (6 = 4 + 2); several workgroups of every kernel at the base width; more rows than one
# wave pass, no multiple of the 4 query rows per workgroup, at the widest supported d
CASES = [("N2_d64", (2, 64)), ("N6_d128", (6, 128)), ("N64_d768", (64, 768)), ("N130_d1024", (130, 1024))]
GATHERED = ("N16_local4_d128", (16, 4, 128, [5, 4, 11, 10]))     # N, local rows, d, their (interleaved, unsorted) positions
BAD_D = (32, 65, 1088)
BAD_N = (3, 0, 2050)


def gathered_positions(rank, B):
    """Rows of the reference's score problem that hold the B samples of `rank`: r B + b (module docstring)."""
    return torch.arange(B, dtype=torch.int64) + rank * B


def normalize64(z):
    return z / z.norm(dim=-1, keepdim=True).clamp_min(EPS)


def inputs(N, d, seed, local=None, positions=None):
    """One case.  B = `local` rows of this rank (default: all N).  hidden bf16 [rows,d] with B pooled rows (unsorted, row 0 and the
    last row among them), w bf16 [d,d].  With B >= 6: sample 0 has |z| near 1e-3; samples 1 and 4 (different pairs) hold the same
    hidden row - equal embeddings, cosine 1; sample 3 holds minus sample 2's row - a pair at cosine -1.  E fp32 [N,d]: the local
    embeddings (float64 statement rounded to fp32) at `positions`, seeded unit rows elsewhere; stat / rnorm: the float64 statements
    rounded to fp32 - the backward takes them as given.  dw0 / dh0: what the accumulating outputs hold before the call."""
    g = gen(seed)
    B = N if local is None else local
    rows = 2 * B + 3
    hidden = randn_bf16(g, rows, d)
    pr = pool_sample(g, B, rows)
    w = randn_bf16(g, d, d, scale=d ** -0.5)
    if B >= 6:
        p = pr.long()
        hidden[p[0]] = (torch.randn(d, generator=g) * (1e-3 * d ** -0.5)).to(torch.bfloat16)
        hidden[p[4]] = hidden[p[1]]
        hidden[p[3]] = -hidden[p[2]]
    i = dict(N=N, B=B, d=d, rows=rows, hidden=hidden, pool_row=pr, w=w, scale=UPSTREAM * RATIO,
             dw0=torch.randn(d, d, generator=g), dh0=randn_bf16(g, rows, d))
    z, e, rn = embed64(i)
    i["rnorm"] = rn.float()
    if local is None:
        i["row_map"], i["E"] = None, e.float()
    else:
        pos = torch.tensor(positions, dtype=torch.int64)
        assert len(positions) == B and len(set(positions)) == B
        E = normalize64(torch.randn(N, d, generator=g, dtype=torch.float64)).float()
        E[pos] = e.float()
        i["row_map"], i["E"] = pos.to(torch.int32), E
    i["stat"] = stats64(i["E"].double()).float()
    return i


def case(name):
    for k, (N, d) in CASES:
        if k == name:
            return inputs(N, d, seed=7000 + N + d)
    N, B, d, pos = GATHERED[1]
    assert name == GATHERED[0]
    return inputs(N, d, seed=7777, local=B, positions=pos)


# ------------------------------------------------------------------------------------------------------------------ float64 statements
def embed64(i):
    h = i["hidden"].double()[i["pool_row"].long()]
    z = h @ i["w"].double().t()
    n = z.norm(dim=-1)
    return z, z / n.clamp_min(EPS)[:, None], 1.0 / n.clamp_min(EPS)


def scores_literal(E):
    """scores of cos_sim (loss_utils.py:140-167), literally: the interleave of left / right, the product, the mask."""
    N, d = E.shape
    left, right = E[0::2], E[1::2]
    left_new = torch.hstack([left, right]).reshape(-1, d)
    right_new = torch.hstack([right, left]).reshape(-1, d)
    scores = (left_new @ right_new.t()) * TEMP
    x = torch.arange(N)
    y = x + 1 - (x % 2) * 2
    scores = scores.clone()
    scores[x, y] = MASKED
    return scores


def loss_literal(E, ratio=RATIO):
    """ratio * 0.5 (CE(scores, arange) + CE(scores^T, arange)) - both cross-entropies, nothing folded (differentiable)."""
    scores = scores_literal(E)
    lab = torch.arange(E.shape[0])
    ce = torch.nn.functional.cross_entropy
    return ratio * 0.5 * (ce(scores, lab) + ce(scores.t(), lab))


def stats64(E):
    """[3,N]: row max and log-sum-exp of S = 20 E E^T without its diagonal, and the row term lse_i - S[i][i ^ 1]."""
    N = E.shape[0]
    S = TEMP * (E @ E.t())
    S = S.masked_fill(torch.eye(N, dtype=torch.bool), float("-inf"))
    lse = torch.logsumexp(S, dim=1)
    part = S[torch.arange(N), torch.arange(N) ^ 1]
    return torch.stack([S.max(dim=1).values, lse, lse - part])


def head_autograd64(h, w, ratio=RATIO, upstream=1.0, E_other=None, positions=None):
    """The whole head in float64 autograd from the pooled rows h [B,d] and cl_proj's weight: (loss, z, dz, dW, dh).  With E_other
    [N,d] the local embeddings replace its rows `positions` (gradient to the local rows only)."""
    h = h.double().clone().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    z = h @ w.t()
    z.retain_grad()
    e = normalize64(z)
    if E_other is None:
        E = e
    else:
        E = E_other.double().clone()
        E = E.index_put((positions.long(),), e)
    loss = loss_literal(E, ratio)
    (upstream * loss).backward()
    return loss.detach(), z.detach(), z.grad, w.grad, h.grad


# ------------------------------------------------------------------------------------------------------------------ checks
def _score_bounds(E):
    """S = 20 E E^T in float64 and the bound of an fp32 evaluation of one entry: the d-term dot product, the factor 20."""
    d = E.shape[1]
    S = TEMP * (E @ E.t())
    A = E.abs() @ E.abs().t()
    return S, TEMP * 2 * d * U * A + U * S.abs()


def embed_check(i, z, e, rnorm):
    d = i["d"]
    h, w = i["hidden"].double()[i["pool_row"].long()], i["w"].double()
    zr, er, rr = embed64(i)
    bz = 2 * d * U * (h.abs() @ w.abs().t())
    n2 = (zr * zr).sum(-1)
    rel_n = (zr.abs() * bz).sum(-1) / n2 + (d + 4) * U      # relative error of |z|: the propagated dot errors, d squares and their sum, the root
    return [held("z", z, zr, bz),
            held("rnorm", rnorm.view(1, -1), rr.view(1, -1), (rr * (rel_n + 2 * U)).view(1, -1)),
            held("e", e, er, bz * rr[:, None] + er.abs() * (rel_n[:, None] + 3 * U))]


def loss_check(i, stat, loss, ratio=RATIO):
    E = i["E"].double()
    N = E.shape[0]
    eye = torch.eye(N, dtype=torch.bool)
    S, bS = _score_bounds(E)
    ref = stats64(E)
    So = S.masked_fill(eye, float("-inf"))
    bmax = bS.masked_fill(eye, 0.0).max(dim=1).values
    rng = (ref[0][:, None] - So).masked_fill(eye, 0.0).max(dim=1).values      # score range of the row
    b_lse = bmax + (EXP_C0 + 2 * EXP_CX * rng + (EXP_C0 + 2) * N) * U + U * ref[1].abs()
    part = torch.arange(N) ^ 1
    b_term = b_lse + bS[torch.arange(N), part] + U * ref[2].abs()
    lref = loss_literal(E, ratio)
    b_loss = ratio / N * (b_term.sum() + N * U * ref[2].abs().sum()) + 4 * U * lref.abs()
    return [held("row max", stat[0:1], ref[0:1], bmax.view(1, -1)),
            held("row lse", stat[1:2], ref[1:2], b_lse.view(1, -1)),
            held("row term", stat[2:3], ref[2:3], b_term.view(1, -1)),
            held("loss", loss.view(1, 1), lref.view(1, 1), b_loss.view(1, 1))]


def bwd64(i):
    """The backward's float64 statement on its own inputs (E, stat, rnorm as given): dE by autograd over the literal loss with the
    local rows as the variables, then the normalisation, cl_proj and the accumulating outputs.  Returns the references and bounds."""
    E, N, B, d = i["E"].double(), i["N"], i["B"], i["d"]
    pos = torch.arange(B) if i["row_map"] is None else i["row_map"].long()
    pr = i["pool_row"].long()
    h, w, rn = i["hidden"].double()[pr], i["w"].double(), i["rnorm"].double()
    assert bool((rn < 1.0 / EPS).all())
    e_loc = E[pos].clone().requires_grad_(True)
    (i["scale"] / RATIO * loss_literal(E.index_put((pos,), e_loc), RATIO)).backward()
    dE = e_loc.grad
    # bound of dE: the coefficients G[i][k] = c (P[i][k] + P[k][i] - 2 [k == i ^ 1]), c = 20 scale / N, from scores within bS and the
    # GIVEN fp32 lse; then the N-term sum over the rows of E
    S, bS = _score_bounds(E)
    lse = i["stat"][1].double()
    eye = torch.eye(N, dtype=torch.bool)
    X = (S - lse[:, None]).masked_fill(eye, float("-inf"))
    P = X.exp()
    bP = (P * (bS + U * X.abs().masked_fill(eye, 0.0) + (EXP_C0 + EXP_CX * X.abs().masked_fill(eye, 0.0)) * U)).masked_fill(eye, 0.0) + TINY
    c = TEMP * i["scale"] / N
    hit = torch.zeros(N, N, dtype=torch.float64)
    hit[torch.arange(N), torch.arange(N) ^ 1] = 1.0
    G = c * (P + P.t() - 2 * hit)
    bG = c * (bP + bP.t()) + 4 * U * c * (P + P.t() + 2 * hit)
    b_dE = (bG[pos] @ E.abs()) + 2 * N * U * (G[pos].abs() @ E.abs())
    e = E[pos]
    t = (e * dE).sum(-1, keepdim=True)
    b_t = (e.abs() * b_dE).sum(-1, keepdim=True) + 2 * d * U * (e.abs() * dE.abs()).sum(-1, keepdim=True)
    dz = (dE - e * t) * rn[:, None]
    b_dz = rn[:, None] * (b_dE + e.abs() * b_t) + 4 * U * rn[:, None] * (dE.abs() + e.abs() * t.abs())
    add = dz @ w
    b_add = b_dz @ w.abs() + 2 * d * U * (dz.abs() @ w.abs())
    dh0 = i["dh0"].double()
    dh, b_dh = dh0.clone(), torch.zeros_like(dh0)
    dh[pr] = dh0[pr] + add
    b_dh[pr] = 2.0 ** -8 * dh[pr].abs() + b_add + U * (dh0[pr].abs() + add.abs())
    dw0 = i["dw0"].double()
    dw = dw0 + dz.t() @ h
    b_dw = b_dz.t() @ h.abs() + 2 * (B + 1) * U * (dw0.abs() + dz.abs().t() @ h.abs())
    return dict(dz=dz, b_dz=b_dz, dh=dh, b_dh=b_dh, dw=dw, b_dw=b_dw)


def bwd_check(i, dz, dw, dhidden):
    r = bwd64(i)
    pr = i["pool_row"].long()
    rest = torch.ones(i["rows"], dtype=torch.bool)
    rest[pr] = False
    return [held("dz", dz, r["dz"], r["b_dz"]), held("dw", dw, r["dw"], r["b_dw"]),
            held("dhidden", dhidden, r["dh"], r["b_dh"]),
            held_equal("dhidden outside the pooled rows", dhidden[rest], i["dh0"][rest])]


# ------------------------------------------------------------------------------------------------------------------ fp32 CPU statements
FAULTS = ("self_unmasked", "partner_next", "transpose_dropped", "key_side_missing", "dh_stored", "no_projection", "temperature_1", "ratio_1")


def embed_fp32(i):
    h = i["hidden"].float()[i["pool_row"].long()]
    z = h @ i["w"].float().t()
    rn = 1.0 / z.norm(dim=-1).clamp_min(EPS)
    return z, z * rn[:, None], rn


def _partner(N, fault):
    k = torch.arange(N)
    return (k + 1) % N if fault == "partner_next" else k ^ 1


def loss_fp32(E, ratio=RATIO, fault=None):
    """stat [3,N] and the loss from fp32 operations; `fault` plants one of FAULTS."""
    N = E.shape[0]
    temp = 1.0 if fault == "temperature_1" else TEMP
    S = temp * (E @ E.t())
    if fault != "self_unmasked":
        S = S.masked_fill(torch.eye(N, dtype=torch.bool), float("-inf"))
    lse = torch.logsumexp(S, dim=1)
    term = lse - S[torch.arange(N), _partner(N, fault)]
    loss = (1.0 if fault == "ratio_1" else ratio) * term.mean()
    if fault == "transpose_dropped":      # the transposed cross-entropy left out and not replaced by the symmetry
        loss = loss * 0.5
    return torch.stack([S.max(dim=1).values, lse, term]), loss


def bwd_fp32(i, fault=None):
    E, N, B, d = i["E"], i["N"], i["B"], i["d"]
    pos = torch.arange(B) if i["row_map"] is None else i["row_map"].long()
    pr = i["pool_row"].long()
    temp = 1.0 if fault == "temperature_1" else TEMP
    S = temp * (E @ E.t())
    lse = i["stat"][1]
    if fault == "temperature_1":          # (a faulty forward hands its own statistics to its backward)
        lse = torch.logsumexp(S.masked_fill(torch.eye(N, dtype=torch.bool), float("-inf")), dim=1)
    if fault == "self_unmasked":
        lse = torch.logsumexp(S, dim=1)
    P = (S - lse[:, None]).exp()
    if fault != "self_unmasked":
        P = P.masked_fill(torch.eye(N, dtype=torch.bool), 0.0)
    hit = torch.zeros(N, N)
    hit[torch.arange(N), _partner(N, fault)] = 1.0
    scale = i["scale"] * (2.0 if fault == "ratio_1" else 1.0)
    if fault in ("key_side_missing", "transpose_dropped"):
        G = (temp * scale / N) * (P - hit)
    else:
        G = (temp * scale / N) * (P + P.t() - hit - hit.t())
    dE = G[pos] @ E
    e = E[pos]
    t = torch.zeros(B, 1) if fault == "no_projection" else (e * dE).sum(-1, keepdim=True)
    dz = (dE - e * t) * i["rnorm"][:, None]
    dw = i["dw0"] + dz.t() @ i["hidden"].float()[pr]
    dh = i["dh0"].clone()
    add = dz @ i["w"].float()
    dh[pr] = (add if fault == "dh_stored" else dh[pr].float() + add).to(torch.bfloat16)
    return dz, dw, dh
