"""The intra-instance token head (loss_type = "token_ce_intra", csrc/kernels.hip tok_intra_*): a float64 statement of the forward, the
loss and the backward, seeded inputs, per-element error bounds and the checks that hold an implementation to them (the machinery of
tests/_heads_ref.py).  tests/test_gpu_intra_head.py feeds the checks with the HIP kernels' outputs, tests/test_intra_ref.py with the
fp32 CPU statement below (which must pass), with planted faults (which must not) and with the reference fixture.

The head, per sample b with rows rs .. rs + n, C = num_labels and k = cls_idx[b]:
    h^_s = h_s / max(|h_s|, 1e-12)        e^_c = h^_{k+c}        logits[s,c] = 20 <h^_s, e^_c>
and from z = dloss / dlogits:
    dh^_s = sum_c z[s,c] e^_c  (+ sum_s' z[s',c] h^_s' when s = k + c)        dh_s = (dh^_s - h^_s <h^_s, dh^_s>) / max(|h_s|, 1e-12)

Bounds.  u = 2^-24.  The contract: norms, dots and the normalise-backward in fp32 from the bf16 rows, a logit and a dhidden element
rounded to bf16 once (2^-8 |ref|, assert_elementwise's output term).
 * 1 / max(|h|, eps): the sum of d squares in any order d u, the square root halves it and adds u, the reciprocal (correctly rounded or
   the fast form, 2.5 ulp) at most 5 u: R = (d / 2 + 6) u relative.
 * logit: the d-term dot 2 d u sum_j |h_sj h_cj| (the c_acc = 2 rule of _heads_ref), scaled by 20 / (|h_s| |h_c|); the two reciprocal
   norms 2 R and the three products 3 u relative to the logit: 2^-8 |ref| + 40 d u sum|h_s h_c| / (|h_s| |h_c|) + (d + 15) u |ref|.
 * dhidden: dh^_sj is a sum of K_s terms (C, plus the sample's rows with a gradient on a label row), each the product of z, a rounded
   reciprocal norm and a bf16 value: (K_s + d / 2 + 8) u A_sj with A_sj the sum of the terms' magnitudes.  <h^_s, dh^_s> adds its own d
   terms and the rounding of h^: its error is at most (K_s + 2 d + 12) u D_s, D_s = sum_j |h^_sj| A_sj.  The difference, the product
   with h^ and the final reciprocal norm add (d / 2 + 8) u of (A_sj + |h^_sj| D_s).  Together, with |dh^_sj| <= A_sj and |dot| <= D_s:
       (K_s + 2.5 d + 20) u (A_sj + |h^_sj| D_s) / max(|h_s|, eps)
   and 2^-8 of the value that is rounded (|ref| plus that error: the factor 1.01).  A row nothing flows into has A = 0: exactly zero.
"""
import math

import torch

import _heads_ref as H

U = H.U
INV_TEMP = 20.0
EPS = 1e-12


# ------------------------------------------------------------------------------------------------------------------ float64 statement
def _norms(h):
    return h.norm(dim=-1).clamp_min(EPS)


def intra_logits(h, row_start, cls_idx, C):
    """float64 logits [rows, C] of hidden `h` [rows, d] (any float dtype): NaN on the rows of no sample.  Also the |.| companion
    20 sum_j |h_sj h_cj| / (|h_s| |h_c|) of the accumulation bound."""
    h = h.double()
    out = torch.full((h.shape[0], C), float("nan"), dtype=torch.float64)
    ab = torch.zeros_like(out)
    for b in range(len(cls_idx)):
        rs, re, k = int(row_start[b]), int(row_start[b + 1]), int(cls_idx[b])
        x = h[rs:re]
        assert 0 <= k and k + C <= re - rs, (b, k, C, re - rs)
        nx = _norms(x)
        e, ne = x[k:k + C], nx[k:k + C]
        out[rs:re] = INV_TEMP * (x / nx[:, None]) @ (e / ne[:, None]).t()
        ab[rs:re] = INV_TEMP * (x.abs() @ e.abs().t()) / (nx[:, None] * ne[None, :])
    return out, ab


def intra_logits_grid(hidden, cls_idx, C):
    """The same on a [B,S,d] grid (the reference's call shape): float64 [B,S,C]."""
    B, S, d = hidden.shape
    lg, _ = intra_logits(hidden.reshape(B * S, d), torch.arange(B + 1) * S, cls_idx, C)
    return lg.view(B, S, C)


def token_ce(logits, labels):
    """Mean cross-entropy over the rows with labels != -100, float64 (NaN when there is none, as torch's)."""
    lg, y = logits.reshape(-1, logits.shape[-1]).double(), labels.reshape(-1)
    lab = y >= 0
    if not bool(lab.any()):
        return torch.tensor(float("nan"), dtype=torch.float64)
    x = lg[lab]
    return (torch.logsumexp(x, 1) - x.gather(1, y[lab][:, None]).squeeze(1)).mean()


def intra_backward(h, row_start, cls_idx, C, z):
    """float64 dhidden [rows, d] from z = dloss / dlogits [rows, C] (zeros on the rows of no sample, which the kernel does not write),
    and the bound's companion (K + 2.5 d + 20) (A + |h^| D) / max(|h|, eps) per element."""
    h, z = h.double(), z.double()
    d = h.shape[1]
    ref, comp = torch.zeros_like(h), torch.zeros_like(h)
    for b in range(len(cls_idx)):
        rs, re, k = int(row_start[b]), int(row_start[b + 1]), int(cls_idx[b])
        x, zz = h[rs:re], z[rs:re]
        nx = _norms(x)
        xh = x / nx[:, None]
        e = xh[k:k + C]
        dxh, A = zz @ e, zz.abs() @ e.abs()
        K = torch.full((re - rs,), float(C), dtype=torch.float64)
        dxh[k:k + C] += zz.t() @ xh
        A[k:k + C] += zz.abs().t() @ xh.abs()
        K[k:k + C] += float((zz != 0).any(1).sum())
        dot = (xh * dxh).sum(1, keepdim=True)
        D = (xh.abs() * A).sum(1, keepdim=True)
        ref[rs:re] = (dxh - xh * dot) / nx[:, None]
        comp[rs:re] = (K[:, None] + 2.5 * d + 20) * (A + xh.abs() * D) / nx[:, None]
    return ref, comp


# ------------------------------------------------------------------------------------------------------------------ inputs
LEAD = 3      # rows in front of the first sample on the padded layout: they belong to no sample


def intra_inputs(d, C, lens, padded, place, seed):
    """Samples of `lens` real rows each (every one >= C + 1) in one [rows, d] bf16 buffer.  padded = False: back to back from row 0 (the
    compact layout).  padded = True: sample b is followed by 1 + 2 b % 5 pad rows that row_start counts as its own (the padded grid: a
    sample owns S rows, its real rows in front; pad rows hold finite values, get logits nobody reads and a zero gradient), and LEAD rows
    in front of the first sample belong to none (never written).  place = "last" puts the label rows at the end of the real rows, "mid"
    in their middle.  About a third of the other real rows carry a gradient; the second sample (if there are three or more) carries none
    at all; in the first sample one label row carries one too (it receives both parts of dh^), the other label rows receive de^ only.  A
    sample of C + 1 rows has its one other row labelled.  dl is shaped as tok_ce leaves it: (softmax - onehot) rows, zero rows where
    there is no label, here times 16; the backward runs with stat[2] = 1/64, so that bf16(dl / 64) is exact in the float64 statement."""
    g = H.gen(seed)
    B = len(lens)
    row_start, cls_idx = [LEAD if padded else 0], []
    for b, n in enumerate(lens):
        assert n >= C + 1
        cls_idx.append(n - C if place == "last" else (n - C) // 2)
        row_start.append(row_start[-1] + n + (1 + (2 * b) % 5 if padded else 0))
    rows = row_start[-1]
    hidden = H.randn_bf16(g, rows, d)
    dl = torch.zeros(rows, C)
    labelled = torch.zeros(rows, dtype=torch.bool)
    for b, n in enumerate(lens):
        rs, k = row_start[b], cls_idx[b]
        if B >= 3 and b == 1:
            continue
        other = torch.ones(n, dtype=torch.bool)
        other[k:k + C] = False
        pick = other & (torch.rand(n, generator=g) < 0.34)
        if not bool(pick.any()):
            pick[other.nonzero()[0]] = True
        if b == 0:
            pick[k + C // 2] = True       # a label row that is labelled itself
        labelled[rs:rs + n] = pick
    nl = int(labelled.sum())
    p = torch.softmax(torch.randn(nl, C, generator=g) * 2.0, 1)
    p[torch.arange(nl), torch.randint(0, C, (nl,), generator=g)] -= 1.0
    dl[labelled] = p * 16.0
    inside = torch.zeros(rows, dtype=torch.bool)
    inside[row_start[0]:] = True
    return dict(d=d, C=C, B=B, rows=rows, lens=list(lens), hidden=hidden, dl=dl, row_start=torch.tensor(row_start, dtype=torch.int32),
                cls_idx=torch.tensor(cls_idx, dtype=torch.int64), inside=inside, labelled=labelled)


INV_N = 1.0 / 64


def intra_z(i, inv_n):
    """z = 20 bf16(dl inv_n): exact in fp32 for inv_n a power of two (or zero), so the documented rounding is reproduced, not bounded."""
    assert inv_n == 0.0 or math.frexp(inv_n)[0] == 0.5
    return INV_TEMP * (i["dl"] * inv_n).to(torch.bfloat16).double()


# ------------------------------------------------------------------------------------------------------------------ checks
def intra_fwd_check(i, logits):
    """logits: f32 [rows, C] as the kernel left it (rows of no sample still hold whatever was there: checked by the caller)."""
    ref, ab = intra_logits(i["hidden"], i["row_start"], i["cls_idx"], i["C"])
    m, d = i["inside"], i["d"]
    bound = 2.0 ** -8 * ref[m].abs() + 2 * d * U * ab[m] + (d + 15) * U * ref[m].abs()
    got = logits[m]
    return [H.held("logits", got, ref[m], bound), H.held_equal("logits are bf16 values", got, got.to(torch.bfloat16).float())]


def intra_bwd_check(i, inv_n, dhidden):
    m = i["inside"]
    if inv_n == 0.0:      # no labelled row in the batch: nothing flows
        return [H.held_equal("dhidden", dhidden[m], torch.zeros(int(m.sum()), i["d"], dtype=torch.bfloat16))]
    ref, comp = intra_backward(i["hidden"], i["row_start"], i["cls_idx"], i["C"], intra_z(i, inv_n))
    bound = 2.0 ** -8 * ref[m].abs() + 1.01 * U * comp[m]
    out = [H.held("dhidden", dhidden[m], ref[m], bound)]
    # the rows nothing flows into are exactly zero: every row of a sample without a labelled row, and the unlabelled rows that are no label row
    quiet = m & (comp.sum(1) == 0)
    out.append(H.held_equal("dhidden (rows without a gradient)", dhidden[quiet], torch.zeros(int(quiet.sum()), i["d"], dtype=torch.bfloat16)))
    return out


# ------------------------------------------------------------------------------------------------------------------ fp32 statement
def _f32_rows(h):
    x = h.float()
    inv = 1.0 / x.norm(dim=-1).clamp_min(EPS)
    return x, inv


def intra_fwd_fp32(i):
    """A plain fp32 CPU statement of the contract: must stay inside the bounds."""
    x, inv = _f32_rows(i["hidden"])
    out = torch.full((i["rows"], i["C"]), float("nan"))
    for b in range(i["B"]):
        rs, re, k = int(i["row_start"][b]), int(i["row_start"][b + 1]), int(i["cls_idx"][b])
        e, ie = x[rs + k:rs + k + i["C"]], inv[rs + k:rs + k + i["C"]]
        out[rs:re] = (INV_TEMP * ((x[rs:re] @ e.t()) * inv[rs:re, None] * ie[None, :])).to(torch.bfloat16).float()
    return out


def intra_bwd_fp32(i, inv_n, fault=None):
    """The backward in fp32.  fault: "no_projection" drops h^ <h^, dh^>, "no_label_sum" drops de^ - planted faults for the host test."""
    x, inv = _f32_rows(i["hidden"])
    z = intra_z(i, inv_n).float()
    C = i["C"]
    out = torch.zeros(i["rows"], i["d"])
    for b in range(i["B"]):
        rs, re, k = int(i["row_start"][b]), int(i["row_start"][b + 1]), int(i["cls_idx"][b])
        xh = x[rs:re] * inv[rs:re, None]
        zz = z[rs:re]
        dxh = zz @ xh[k:k + C]
        if fault != "no_label_sum":
            dxh[k:k + C] += zz.t() @ xh
        dot = (xh * dxh).sum(1, keepdim=True)
        if fault == "no_projection":
            dot = dot * 0
        out[rs:re] = (dxh - xh * dot) * inv[rs:re, None]
    return out.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ the cases
# (id, (d, C, real rows per sample, padded, place)).  A wave of the kernels owns 4 rows (forward) / 2 of 8 (backward), a round of the
# backward is 64 rows, the backward is compiled for C <= 8, 16, 32, 48 and 64, a lane holds the column pairs 128 q + 2 lane (d = 64 and
# d = 192 leave the last q half empty).
INTRA_CASES = [
    ("d64-C2: samples of C + 1, 7 and 130 rows, compact, label rows last", (64, 2, (3, 7, 130), False, "last")),
    ("d768-C5: C + 1, 13, 67 and 1024 rows, padded grid, label rows last", (768, 5, (6, 13, 67, 1024), True, "last")),
    ("d128-C12: second template width, compact, label rows in the middle", (128, 12, (13, 37, 66), False, "mid")),
    ("d192-C20: third template width, half-filled last column pair, padded", (192, 20, (21, 65), True, "mid")),
    ("d1024-C47: widest row, compact, label rows in the middle", (1024, 47, (48, 131), False, "mid")),
    ("d1024-C64: widest row and most classes (the LDS maximum), padded", (1024, 64, (65, 200), True, "mid")),
    ("d768-C47: one sample of 1024 rows (the products-like shape)", (768, 47, (1024,), False, "last")),
    ("d64-C64: more classes than column pairs per lane", (64, 64, (65, 70, 129), False, "last")),
]


def intra_case(d, C, lens, padded, place):
    return intra_inputs(d, C, lens, padded, place, seed=8000 + d + C + len(lens))
