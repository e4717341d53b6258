"""The dropout / DropPath / LayerScale family - the counter hashes elem_drop_mul (csrc/common.h) and path_keep (csrc/kernels.h) and every
kernel that applies them in the forward and regenerates them from coordinates in the backward: numpy twins of the two hashes, seeded inputs,
float64 statements of every operation on the bf16 / fp32 inputs the kernel gets, the per-element bounds and the checks that hold an
implementation to them.  tests/test_gpu_drop.py feeds the checks with the HIP kernels' outputs, tests/test_drop_reference.py with the fp32
CPU statements below (which must pass) and with planted faults (which must not).

The masks.  em = the element multiplier: 0 where hash24(seed, stream, a, b) < thresh = (unsigned)(fp32(p) * 2^24), else inv = fp32(1 / (1 - p));
a = the LOGICAL row rows[t] (t itself without a row map; the embedding: rows[t] * F + f; the head: the pooled row b), b = the column.
keep = the sample multiplier: 0 where fp32(hash24(seed, sample)) * 2^-24 < rate, else fp32(1 / (1 - rate)); sample = row_b[t] or t / S.
Both multipliers are INPUTS of the statements below, as the fp32 values the twins give.

Bounds.  u = 2^-24 is fp32's unit roundoff, ub = 2^-8 the bf16 term of tests/_util.py:assert_elementwise, with the factor 1.01 that absorbs
the fp32 roundings relative to the result itself; every bound adds TINY = 2^-126.
 * v = bf16(y * em) and q = bf16(lam * v): one IEEE fp32 product and one RNE conversion each (lam * v is exact in fp32) - REPLAYED bit for bit
   on the CPU, never bounded.  The same holds for bf16(emb * em) of the embedding and for bf16(x * em) of elem_dropout.
 * out = bf16(res + keep * q).  keep = 1 (rate = 0) or keep = 0 (the sample is dropped: out = res): a product by 1 or 0 and one addition,
   fused or not, give the same fp32 value - bit for bit.  Elsewhere the product by keep and the addition may be contracted into one fma:
   |err| <= 1.01 ub |ref| + 2 u (|res| + |keep q|) + TINY (the product and the sum round once each, or once together).
   xn / rstd: _rows_ref._norm_checks on the out that was written.
 * dx, dw of the fused backward: _rows_ref.ls_bwd_check's, on inputs the masks do not touch.
 * dsc = bf16(((lam * keep) * dx) * em) of the dx that was written: three fp32 products and one conversion,
   |err| <= (1.01 ub + 3 u) |ref| + TINY; exactly +-0 where em = 0 or keep = 0 (a product by 0.f of finite values).
 * dlam = dlam0 + sum_t (keep * dx) * bf16(y * em): _rows_ref._accum_check's replica-sum bound 2 (T + 1) u (sum|dlam0| + sum|term|): a term
   carries two roundings of its own (2 u |term|) and the sum in any order, atomics included, (T - 1 + copies) u sum|.|: below it for T >= 1.
 * elem_dropout: x = bf16(x * em), bit for bit; a dropped element is x * 0.f, i.e. a ZERO WITH THE SIGN OF x (the kernel multiplies, it does
   not select), and the conversion keeps the sign.
 * embedding forward: out = bf16(sum_f bf16(W[id_f] * em_f) (* G_f)) in feature order.  The inner rounding is replayed, so the one extra
   rounding of the masked form costs the bound nothing: plain stacking stays bit for bit, gated stacking keeps _elem_ref.embed_fwd_check's
   1.01 ub |ref| + F u sum_f |v_f G_f| + TINY.
 * embedding backward (always the sorted scatter-add with a mask): demb[v] = demb0[v] + sum_cells (dx * em) * G_f - a term carries two
   roundings, the sum of n_v terms and the initial value (n_v + 1) u: below _elem_ref's 2 (n_v + 1) u (|demb0| + sum|term|) + TINY;
   dgate[f] = dgate0[f] + sum_t dx * bf16(W[id] * em): 2 (T + 1) u (|dgate0| + sum|term|) + TINY.  Rows no cell holds keep demb0's bits.
 * head forward: a = bf16(bf16(gelu(x)) * em): _heads_ref's bound of bf16(gelu(x)) reaches a multiplied by em, then one more rounding:
   |err| <= em (ub |g| + 1.01 (|x| PHI_ATOL + u |g|)) + 1.01 ub |g em| + TINY, g = gelu(x); exactly +-0 where em = 0.  y: _heads_ref's dot
   bound against the product of the a that was written.
 * head backward: dx = ((dy . W) * em) * gelu'(x): _heads_ref's bound with every term multiplied by em and one more product:
   2 Dout u em sum|dy W| |gelu'| + em |dy . W| GELU_GRAD_ATOL + 4 u |ref|; exactly +-0 where em = 0.  dw, dbias: _heads_ref's, from the
   a that was written (which carries the mask).
 * fused against unfused backward (two kernels whose dx may differ by a rounding of the row mean): the zero pattern of dsc is the masks'
   and must be identical; the values differ by at most |lam keep em| (2 x the dx bound) + 2 x the dsc bound.

Inputs.  y, dy, x, emb, lam (and the gate) of every masked case have magnitudes >= 2^-2: sign * (0.25 + |randn|) rounded to bf16, so that a
kept and a dropped element differ by far more than any bound.  The row family keeps its special rows (row 1 all zeros, row 2 one non-zero).
An element whose bound is at least |value with every mask keeping it - value with a mask dropping it| is VACUOUS: the check could not see a
flipped mask bit there.  The share is counted over the elements whose masked operand is non-zero (a zero of the special rows is dropped or
kept to the same value under any check).  *_vacuous below compute it from the reference alone; tests/test_drop_reference.py holds it to 0
for out, dsc, elem_dropout, the embedding forward and the head's a, and to 1 % for dlam, demb, dgate and the head's dx.  A sum of T terms
cannot show one term once 2 (T + 1) u sum|term| passes it: the long-T cases of the backward (T > 256) therefore keep y non-zero in four rows
only, with magnitudes >= 4 (dsc, which does not read y, still sees both masks in every row; the forward's y is dense at every T).
"""
import math

import numpy as np
import torch

import _elem_ref as EL
import _heads_ref as H
import _rows_ref as R
from _rows_ref import BF, TINY, U, UB, Bounded, align_up, bf, gen, held, held_bits, held_equal, held_true, settle  # noqa: F401

F32, F64 = torch.float32, torch.float64
STREAM_EMBED, STREAM_MLP_ACT, STREAM_MLP_OUT, STREAM_HEAD, STREAM_RAW = 48, 49, 50, 51, 60

# ------------------------------------------------------------------------------------------------------------------ the mask twins
_M32 = np.uint64(0xFFFFFFFF)
_C = {k: np.uint64(v) for k, v in dict(phi=0x9E3779B1, a=0x85EBCA77, b=0xC2B2AE3D, m1=0x7FEB352D, m2=0x846CA68B).items()}
_S8, _S15, _S16 = np.uint64(8), np.uint64(15), np.uint64(16)


def _u32(x):
    return np.asarray(x).astype(np.int64).astype(np.uint64) & _M32


def _mix24(x):
    """The finaliser both hashes share, on uint64 holding 32-bit values; the top 24 bits."""
    x = x ^ (x >> _S16)
    x = (x * _C["m1"]) & _M32
    x = x ^ (x >> _S15)
    x = (x * _C["m2"]) & _M32
    x = x ^ (x >> _S16)
    return x >> _S8


def elem_hash(seed, stream, a, b):
    """hash24 of elem_drop_mul: a, b wrap to 32 bits as the device's `unsigned` does."""
    x = _u32(seed) ^ ((_u32(stream) * _C["phi"]) & _M32)
    x = (x + ((_u32(a) * _C["a"]) & _M32) + ((_u32(b) * _C["b"]) & _M32)) & _M32
    return _mix24(x)


def elem_thresh(p):
    return int(np.float32(p) * np.float32(16777216.0))


def elem_inv(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def elem_keep(seed, stream, a, b, p):
    """fp32 multiplier of element (a, b) of `stream`: 0 or 1 / (1 - p); p <= 0: 1."""
    h = elem_hash(seed, stream, a, b)
    if p <= 0 or elem_thresh(p) == 0:
        return np.ones(h.shape, np.float32)
    return np.where(h < np.uint64(elem_thresh(p)), np.float32(0), elem_inv(p)).astype(np.float32)


def path_keep(seed, sample, rate):
    """fp32 multiplier of every row of `sample`: 0 or 1 / (1 - rate); rate <= 0: 1."""
    x = _mix24((_u32(seed) + ((_u32(sample) * _C["a"]) & _M32)) & _M32)
    if rate <= 0:
        return np.ones(x.shape, np.float32)
    u = x.astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.where(u < np.float32(rate), np.float32(0), np.float32(1.0) / (np.float32(1.0) - np.float32(rate))).astype(np.float32)


def model_path_keep(seed, layer, which, B, rate):
    """Python twin of path_keep() in csrc/kernels.h behind the engine's seed derivation per (layer, branch): the multiplier of each of the B
    samples (what tests/test_gpu_model.py feeds the oracle)."""
    if rate <= 0:
        return torch.ones(B)
    M32 = 0xFFFFFFFF
    s = (seed ^ ((0xD6E8FEB8 * (layer * 2 + which + 1)) & M32)) & M32
    out = []
    for b in range(B):
        x = (s + b * 0x85EBCA77) & M32
        x ^= x >> 16; x = (x * 0x7FEB352D) & M32
        x ^= x >> 15; x = (x * 0x846CA68B) & M32
        x ^= x >> 16
        u = np.float32(x >> 8) * np.float32(1.0 / 16777216.0)
        out.append(0.0 if u < np.float32(rate) else float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate))))
    return torch.tensor(out)


# ------------------------------------------------------------------------------------------------------------------ row maps and settings
VARLEN_LENS, VARLEN_S = (1, 9, 13, 4), 16
VARLEN_T = sum(VARLEN_LENS)


def layout(kind, T=None):
    """identity: the rows are the logical rows, sample = t / S (S = 7: T = 35 is B = 5 samples; the shorter cases take S = 2, one row S = 1).
    varlen: the compact rows of samples of 1, 9, 13 and 4 rows on a padded S = 16 grid - rows = c2p, row_b given, and a path_S that is
    deliberately wrong (1), so that a kernel that ignores row_b fails."""
    if kind == "identity":
        S = 7 if T >= 14 else (2 if T >= 2 else 1)
        t = np.arange(T)
        return dict(kind=kind, T=T, rows=None, row_b=None, S=S, logical=t, sample=t // S)
    assert kind == "varlen" and T in (None, VARLEN_T)
    c2p = np.concatenate([b * VARLEN_S + np.arange(n) for b, n in enumerate(VARLEN_LENS)])
    row_b = np.concatenate([np.full(n, b) for b, n in enumerate(VARLEN_LENS)])
    return dict(kind=kind, T=VARLEN_T, rows=torch.from_numpy(c2p).to(torch.int32), row_b=torch.from_numpy(row_b).to(torch.int32), S=1,
                logical=c2p, sample=row_b)


SETTINGS = ("elem", "path", "both", "path-nolam", "thresh-below", "thresh-above")
ELEM_SETTINGS = ("elem", "thresh-below", "thresh-above")


def setting(name, lay, stream, seed0, known, path=True):
    """The mask arguments of one setting.  elem: p = 0.2; path: rate = 0.5 with a seed for which, by the twin, one sample is kept and one
    dropped (where the layout has two); thresh-below / -above: p = h / 2^24 and (h + 1) / 2^24 with h the hash of the element `known` =
    (a, b): thresh = h keeps it (h < h is false), thresh = h + 1 drops it - which fixes the `<` of the comparison."""
    m = dict(name=name, elem_p=0.0, elem_seed=0, path_rate=0.0, path_seed=0, lam=name != "path-nolam", known=None, stream=stream)
    if name in ("elem", "both"):
        m.update(elem_p=0.2, elem_seed=(seed0 * 2654435761 + 12345) & 0xFFFFFFFF)
    if name in ("path", "both", "path-nolam"):
        assert path
        m["path_rate"] = 0.5
        samples = np.unique(lay["sample"])
        for s in range(seed0 + 1, seed0 + 200):
            k = path_keep(s, samples, 0.5)
            if len(samples) < 2 or (bool((k == 0).any()) and bool((k != 0).any())):
                m["path_seed"] = s
                break
        else:
            raise AssertionError("no path seed found")
    if name.startswith("thresh"):
        for s in range(seed0 + 1, seed0 + 400):
            h = int(elem_hash(s, stream, known[0], known[1]))
            if 0.15 * 2 ** 24 <= h <= 0.25 * 2 ** 24:
                break
        else:
            raise AssertionError("no threshold seed found")
        k = h if name == "thresh-below" else h + 1
        p = float(np.float32(k) / np.float32(16777216.0))
        assert elem_thresh(p) == k
        m.update(elem_p=p, elem_seed=s, known=known)
    return m


OFF = dict(name="off", elem_p=0.0, elem_seed=0, path_rate=0.0, path_seed=0, lam=True, known=None, stream=0)


def elem_mult(m, lay, cols, stream=None, F=None):
    """em fp32 [T, cols] (F: [T, F, cols], a = logical row * F + f)."""
    a = lay["logical"].astype(np.int64)
    stream = m["stream"] if stream is None else stream
    if F is None:
        return torch.from_numpy(elem_keep(m["elem_seed"], stream, a[:, None], np.arange(cols)[None, :], m["elem_p"]))
    cell = a[:, None] * F + np.arange(F)[None, :]
    return torch.from_numpy(elem_keep(m["elem_seed"], stream, cell[:, :, None], np.arange(cols)[None, None, :], m["elem_p"]))


def keep_mult(m, lay):
    """keep fp32 [T]."""
    return torch.from_numpy(path_keep(m["path_seed"], lay["sample"], m["path_rate"]))


def mag_bf16(g, *shape, base=0.25, spread=1.0, cap=None):
    """sign * (base + spread |randn|) rounded to bf16."""
    r = torch.randn(*shape, generator=g)
    v = base + spread * r.abs()
    if cap is not None:
        v = v.clamp_max(cap)
    return (torch.where(r < 0, -v, v)).to(BF)


def _share(vac, where):
    n = int(where.sum())
    return float((vac & where).sum()) / n if n else 0.0


LONG_T = 256


def _branch_y(g, T, d):
    """y of the backward's residual branch; past LONG_T rows only four rows are non-zero, with magnitudes >= 4 (see the docstring)."""
    if T <= LONG_T:
        return mag_bf16(g, T, d)
    y = torch.zeros(T, d, dtype=BF)
    at = torch.tensor([3, T // 3, T // 2 + 1, T - 2])
    y[at] = mag_bf16(g, 4, d, base=4.0)
    return y


# ------------------------------------------------------------------------------------------------------------------ LayerScale forward
def ls_fwd_inputs(T, d, seed, lam=True):
    g = gen(seed)
    i = dict(T=T, d=d, eps=R.EPS, w=(torch.randn(d, generator=g) * 0.1 + 1).to(BF), res=R.randn_bf16(g, T, d), y=mag_bf16(g, T, d),
             lam=mag_bf16(g, d) if lam else None)
    if T >= 3:
        i["res"][1], i["y"][1] = 0, 0
        i["res"][2], i["y"][2] = 0, 0
        i["y"][2, d - 3] = 1.5
    return i


def _branch_q(i, em, round_v=True):
    """q = bf16(lam * bf16(y * em)) as fp32 values, replayed."""
    v = i["y"].float() * em
    if round_v:
        v = bf(v)
    return v if i["lam"] is None else bf(i["lam"].float() * v)


def _out_bound(res64, kq64):
    return 1.01 * UB * (res64 + kq64).abs() + 2 * U * (res64.abs() + kq64.abs()) + TINY


def ls_out_check(i, em, keep, rate, out):
    q = _branch_q(i, em)
    exact = (keep == 0) if rate > 0 else torch.ones_like(keep, dtype=torch.bool)
    replay = (i["res"].float() + keep[:, None] * q).to(BF)
    res = []
    if bool(exact.any()):
        res.append(held_bits("out is bf16(res + keep * bf16(lam * bf16(y * em))) where keep is 0 or 1", out[exact], replay[exact]))
    if bool((~exact).any()):
        r64, kq = i["res"].double()[~exact], keep.double()[~exact][:, None] * q.double()[~exact]
        res.append(held("out", out[~exact], r64 + kq, _out_bound(r64, kq)))
    return res


def ls_fwd_check(i, em, keep, rate, out, xn, rstd):
    return ls_out_check(i, em, keep, rate, out) + R._norm_checks(out, i["w"], i["eps"], xn, rstd, tag=" (of out)")


def ls_fwd_fp32(i, em, keep, fault=None):
    """fault: "no-round" - y * em is not rounded to bf16."""
    out = (i["res"].float() + keep[:, None] * _branch_q(i, em, round_v=fault != "no-round")).to(BF)
    return (out,) + R.rms_fwd_fp32(dict(i, x=out))


def ls_fwd_vacuous(i, m):
    """out with every mask keeping the element against out = res."""
    inv = torch.tensor(float(elem_inv(m["elem_p"])) if m["elem_p"] > 0 else 1.0)
    k = 1.0 / (1.0 - m["path_rate"]) if m["path_rate"] > 0 else 1.0
    q = _branch_q(i, inv.expand_as(i["y"].float()))
    res = i["res"].double()
    if m["path_rate"] > 0:
        vac = _out_bound(res, k * q.double()) >= (k * q.double()).abs()
    else:
        vac = (i["res"].float() + q).to(BF) == i["res"]
    return dict(out=_share(vac, i["y"] != 0))


# ------------------------------------------------------------------------------------------------------------------ LayerScale backward
def ls_bwd_inputs(T, d, seed, copies, lam=True, fused=True, dres=True):
    """fused: the inputs of _rows_ref.bwd_inputs(fused=True) with dy, x, y, lam at magnitudes >= 2^-2.  Not fused: dy IS the gradient of
    the residual stream (what the fused form calls dx)."""
    g = gen(seed)
    i = dict(T=T, d=d, copies=copies, stride=align_up(d, 128), dy=mag_bf16(g, T, d), y=_branch_y(g, T, d), lam=mag_bf16(g, d) if lam else None,
             dlam0=torch.randn(copies, d, generator=g))
    if fused:
        x = mag_bf16(g, T, d)
        i.update(x=x, w=(torch.randn(d, generator=g) * 0.1 + 1).to(BF), rstd=(x.double().pow(2).mean(1) + R.EPS).rsqrt().float(),
                 dres=R.randn_bf16(g, T, d) if dres else None, dw0=torch.randn(copies, d, generator=g))
    return i


def _dsc_ref(i, em, keep, dx):
    lam = i["lam"].double() if i["lam"] is not None else 1.0
    ref = lam * keep.double()[:, None] * dx.double() * em.double()
    return ref, (1.01 * UB + 3 * U) * ref.abs() + TINY


def _dlam_terms(i, em, keep, dx, masked_y=True):
    return keep.double()[:, None] * dx.double() * (bf(i["y"].float() * em) if masked_y else i["y"].float()).double()


def scale_checks(i, em, keep, dx, dsc, dlam):
    """dsc and dlam of the LayerScale / DropPath backward from the dx it read (bf16 [T, d]); dlam None: no accumulator was given."""
    ref, bound = _dsc_ref(i, em, keep, dx)
    dropped = (em == 0) | (keep == 0)[:, None]
    out = [held_true("dsc is +-0 where a mask drops", bool((dsc[dropped] == 0).all()), "a dropped element of dsc is not zero"),
           held("dsc", dsc, ref, bound)]
    if dlam is not None:
        t = _dlam_terms(i, em, keep, dx)
        out.append(R._accum_check("dlam", dlam, i["dlam0"], t.sum(0), t.abs().sum(0), i["T"]))
    return out


def ls_bwd_check(i, em, keep, dx, dw, dsc, dlam):
    """The fused form: dx and dw exactly as _rows_ref.ls_bwd_check holds them (the masks must not touch them), dsc / dlam with the masks."""
    return R.ls_bwd_check(dict(i, lam=None), dx, dw, dx, None)[:2] + scale_checks(i, em, keep, dx, dsc, dlam)


def scale_fp32(i, em, keep, dx, fault=None):
    """(dsc, dlam replicas) in fp32.  Faults: "dlam-unmasked-y", "dsc-no-keep", "dsc-no-em"."""
    lam = i["lam"].float() if i["lam"] is not None else torch.ones(i["d"])
    k = keep[:, None] if fault != "dsc-no-keep" else torch.ones(i["T"], 1)
    e = em if fault != "dsc-no-em" else torch.ones_like(em)
    dsc = (((lam * k) * dx.float()) * e).to(BF)
    yv = bf(i["y"].float() * em) if fault != "dlam-unmasked-y" else i["y"].float()
    return dsc, R._replicas_fp32(i, i["dlam0"], (keep[:, None] * dx.float()) * yv)


def ls_bwd_fp32(i, em, keep, fault=None):
    dx, t = R._dx_fp32(i)
    return (dx, R._replicas_fp32(i, i["dw0"], t)) + scale_fp32(i, em, keep, dx, fault)


def scale_vacuous(i, m, em, keep, dx):
    inv = float(elem_inv(m["elem_p"])) if m["elem_p"] > 0 else 1.0
    k = 1.0 / (1.0 - m["path_rate"]) if m["path_rate"] > 0 else 1.0
    full = torch.full_like(em, inv)
    ref, bound = _dsc_ref(i, full, torch.full_like(keep, k), dx)
    t = _dlam_terms(i, em, keep, dx)
    bl = 2 * (i["T"] + 1) * U * (i["dlam0"].double().abs().sum(0) + t.abs().sum(0)) + TINY
    tk = _dlam_terms(i, full, torch.full_like(keep, k), dx)
    return dict(dsc=_share(bound >= ref.abs(), torch.ones_like(em, dtype=torch.bool)), dlam=_share(bl[None, :] >= tk.abs(), i["y"] != 0))


def dsc_pair_check(i, em, keep, dsc_fused, dsc_unfused):
    """rmsnorm_bwd_copies + ls_bwd against the fused kernel on the same inputs and masks."""
    ref, bound, _, _ = R.bwd_ref(i)
    lam = i["lam"].double().abs() if i["lam"] is not None else 1.0
    scale = lam * keep.double()[:, None] * em.double()
    _, own = _dsc_ref(i, em, keep, ref)
    return [held_true("dsc zero pattern of the fused and the unfused form", bool(((dsc_fused == 0) == (dsc_unfused == 0)).all()),
                      "the two forms drop different elements"),
            held("dsc fused against unfused", dsc_fused, dsc_unfused.double(), 2 * scale * bound + 2 * own + TINY)]


# ------------------------------------------------------------------------------------------------------------------ elem_dropout
def drop_inputs(T, n, seed):
    return dict(T=T, n=n, x=mag_bf16(gen(seed), T, n))


def drop_fp32(i, em):
    return (i["x"].float() * em).to(BF)


def drop_check(i, em, got):
    want = drop_fp32(i, em)
    z = em == 0
    sign_ok = bool((got[z].view(torch.int16) == (i["x"][z].view(torch.int16) & -32768)).all())
    return [held_bits("x is bf16(x * em)", got, want),
            held_true("a dropped element is a zero with the sign of x", sign_ok, "a dropped element is not the signed zero of x * 0")]


def drop_vacuous(i, m):
    return dict(x=_share((i["x"].float() * float(elem_inv(m["elem_p"]))).to(BF) == 0, torch.ones_like(i["x"], dtype=torch.bool)))


# ------------------------------------------------------------------------------------------------------------------ embedding
EMB_V = 97


def embed_inputs(T, F, ldF, d, gated, seed):
    """_elem_ref's ids of the forward and of the backward (pad id 0, the last five ids in no cell) with emb and the gate at magnitudes
    >= 2^-2 / 2^-1, dx >= 2^-2, and non-zero initial accumulators."""
    i = EL.embed_bwd_inputs(T, F, ldF, d, EMB_V, 0, gated, seed)
    g = gen(seed + 1)
    i.update(emb=mag_bf16(g, EMB_V, d), dx=mag_bf16(g, T, d), gate=mag_bf16(g, F, d, base=0.5, spread=0.5) if gated else None)
    i["ids"][0, :F] = 0          # (token 0 all pad: the forward stacks the pad row like any other)
    i.pop("_ref", None)
    return i


def _embed_v(i, em, f, round_v=True):
    v = i["emb"][i["ids"][:, f]].float() * em[:, f]
    return bf(v) if round_v else v


def embed_fwd_fp32(i, em, fault=None):
    """fault "after-sum": the mask of feature 0's cell multiplies the stacked sum instead of every gathered row."""
    acc = torch.zeros(i["T"], i["d"])
    for f in range(i["F"]):
        v = _embed_v(i, em if fault != "after-sum" else torch.ones_like(em), f)
        acc = acc + (v * i["gate"][f].float() if i["gate"] is not None else v)
    if fault == "after-sum":
        acc = acc * em[:, 0]
    return acc.to(BF)


def embed_fwd_check(i, em, out):
    if i["gate"] is None:
        return [held_bits("out is bf16 of the fp32 sum of bf16(W * em) in feature order", out, embed_fwd_fp32(i, em))]
    ref, mag = torch.zeros(i["T"], i["d"], dtype=F64), torch.zeros(i["T"], i["d"], dtype=F64)
    for f in range(i["F"]):
        t = _embed_v(i, em, f).double() * i["gate"][f].double()
        ref += t
        mag += t.abs()
    return [held("out (gated)", out, ref, 1.01 * UB * ref.abs() + i["F"] * U * mag + TINY)]


def embed_fwd_vacuous(i, m):
    """Every (cell, channel): the sum with every element kept against the sum without that cell's term."""
    T, F, d = i["T"], i["F"], i["d"]
    full = torch.full((T, F, d), float(elem_inv(m["elem_p"])))
    terms = torch.stack([_embed_v(i, full, f) * (i["gate"][f].float() if i["gate"] is not None else 1.0) for f in range(F)], 1)   # [T, F, d]
    if i["gate"] is None:
        tot = embed_fwd_fp32(i, full)
        vac = torch.stack([embed_fwd_fp32(i, torch.cat([full[:, :f], torch.zeros(T, 1, d), full[:, f + 1:]], 1)) == tot for f in range(F)], 1)
    else:
        ref = terms.double().sum(1, keepdim=True)
        bound = 1.01 * UB * ref.abs() + F * U * terms.double().abs().sum(1, keepdim=True) + TINY
        vac = bound >= terms.double().abs()
    return dict(out=_share(vac, torch.ones_like(vac)))


def _embed_bwd_terms(i, em):
    """float64 per feature: (demb term [T, d], dgate term [T, d] or None)."""
    dx = i["dx"].double()
    for f in range(i["F"]):
        t = dx * em[:, f].double() * (i["gate"][f].double() if i["gate"] is not None else 1.0)
        yield f, t, (dx * _embed_v(i, em, f).double() if i["gate"] is not None else None)


def embed_bwd_ref(i, em):
    T, F, d, V = i["T"], i["F"], i["d"], i["V"]
    s, a, n = torch.zeros(V, d, dtype=F64), torch.zeros(V, d, dtype=F64), torch.zeros(V, dtype=F64)
    gs = ga = None
    if i["gate"] is not None:
        gs, ga = torch.zeros(F, d, dtype=F64), torch.zeros(F, d, dtype=F64)
    for f, t, tg in _embed_bwd_terms(i, em):
        idf = i["ids"][:, f]
        keep = idf != i["pad_id"]
        s.index_add_(0, idf[keep], t[keep])
        a.index_add_(0, idf[keep], t[keep].abs())
        n.index_add_(0, idf[keep], torch.ones(int(keep.sum()), dtype=F64))
        if gs is not None:
            gs[f], ga[f] = tg.sum(0), tg.abs().sum(0)
    return s, a, n, gs, ga


def _embed_bwd_bounds(i, a, n, ga):
    bd = 2 * (n[:, None] + 1) * U * (i["demb0"].double().abs() + a) + TINY
    bg = 2 * (i["T"] + 1) * U * (i["dgate0"].double().abs() + ga) + TINY if ga is not None else None
    return bd, bg


def embed_bwd_check(i, em, demb, dgate):
    s, a, n, gs, ga = embed_bwd_ref(i, em)
    bd, bg = _embed_bwd_bounds(i, a, n, ga)
    assert float(n[i["pad_id"]]) == 0 and int((n == 0).sum()) >= 6
    out = [held("demb", demb, i["demb0"].double() + s, bd),
           held_equal("the pad-id row and the rows of ids no cell holds keep demb0", demb[n == 0], i["demb0"][n == 0])]
    if gs is not None:
        out.append(held("dgate", dgate, i["dgate0"].double() + gs, bg))
    return out


def embed_bwd_fp32(i, em, fault=None):
    demb = i["demb0"].clone()
    dgate = i["dgate0"].clone() if i["gate"] is not None else None
    for f in range(i["F"]):
        idf = i["ids"][:, f]
        keep = idf != i["pad_id"]
        t = i["dx"].float() * em[:, f]
        if i["gate"] is not None:
            t = t * i["gate"][f].float()
            dgate[f] += (i["dx"].float() * _embed_v(i, em, f)).sum(0)
        demb.index_add_(0, idf[keep], t[keep])
    return demb, dgate


def embed_pair_check(i, em, demb, demb_sorted, name="demb of the form chosen against the sorted form forced"):
    """The form the entry chose with a mask against the sorted form forced by the menu key: both within the bound of the same sum."""
    _, a, n, _, ga = embed_bwd_ref(i, em)
    bd, _ = _embed_bwd_bounds(i, a, n, ga)
    return held(name, demb, demb_sorted.double(), 2 * bd)


def embed_bwd_vacuous(i, m, em):
    T, F, d = i["T"], i["F"], i["d"]
    full = torch.full((T, F, d), float(elem_inv(m["elem_p"])))
    _, a, n, _, ga = embed_bwd_ref(i, em)
    bd, bg = _embed_bwd_bounds(i, a, n, ga)
    vd, wd, vg = [], [], []
    for f, t, tg in _embed_bwd_terms(i, full):
        idf = i["ids"][:, f]
        vd.append(bd[idf] >= t.abs())
        wd.append((idf != i["pad_id"])[:, None].expand(T, d))
        if tg is not None:
            vg.append(bg[f][None, :] >= tg.abs())
    out = dict(demb=_share(torch.stack(vd), torch.stack(wd)))
    if vg:
        out["dgate"] = _share(torch.stack(vg), torch.ones_like(torch.stack(vg)))
    return out


# ------------------------------------------------------------------------------------------------------------------ MLP head
def head_inputs(B, Din, Dout, seed):
    """_heads_ref.head_inputs with x at magnitudes in [2^-2, 3] (gelu(x) of a large negative x is below its own absolute bound: the mask
    could not be seen there) and without the three special values."""
    i = H.head_inputs(B, Din, Dout, True, seed)
    i["x"] = mag_bf16(gen(seed + 1), B, Din, cap=3.0)
    return i


def head_a_ref(i, em):
    x = i["x"].double()
    g = x * H._phi64(x)
    e = em.double()
    return g * e, e * (UB * g.abs() + 1.01 * (x.abs() * H.PHI_ATOL + U * g.abs())) + 1.01 * UB * (g * e).abs() + TINY


def head_fwd_check(i, em, a, y, y32):
    ra, ba = head_a_ref(i, em)
    ref, ab = H._linear64(a.double(), i["w"].double(), i["bias"])
    return [held("a", a, ra, ba), held_true("a is +-0 where em = 0", bool((a[em == 0] == 0).all()), "a dropped element of a is not zero"),
            H.held_dot("y", y, ref, ab, i["Din"], 1, 2), held_equal("y32", y32, y.float())]


def head_fwd_fp32(i, em):
    x = i["x"].float()
    a = (bf(x * 0.5 * torch.erfc(-x / math.sqrt(2.0))) * em).to(BF)
    y = (a.float() @ i["w"].float().t() + i["bias"].float()).to(BF)
    return a, y, y.float()


def head_dx_ref(i, em):
    x, dy, w, e = i["x"].double(), i["dy"].double(), i["w"].double(), em.double()
    gp = H._phi64(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    s = dy @ w
    ref = s * gp * e
    return ref, 2 * i["Dout"] * U * (dy.abs() @ w.abs()) * gp.abs() * e + e * s.abs() * H.GELU_GRAD_ATOL + 4 * U * ref.abs() + TINY


def head_bwd_check(i, em, a, dx, dw, dbias):
    ref, bound = head_dx_ref(i, em)
    return [held("dx", dx, ref, bound), held_true("dx is +-0 where em = 0", bool((dx[em == 0] == 0).all()), "a dropped element of dx is not zero")
            ] + H.head_bwd_check(i, a, dx, dw, dbias)[1:]


def head_bwd_fp32(i, em, a, fault=None):
    """fault "no-em": the backward forgets the mask."""
    dx, dw, db = H.head_bwd_fp32(i, a)
    return (dx * em if fault != "no-em" else dx), dw, db


def head_vacuous(i, m):
    full = torch.full((i["B"], i["Din"]), float(elem_inv(m["elem_p"])))
    ra, ba = head_a_ref(i, full)
    rd, bd = head_dx_ref(i, full)
    every = torch.ones_like(full, dtype=torch.bool)
    return dict(a=_share(ba >= ra.abs(), every), dx=_share(bd >= rd.abs(), every))


# ------------------------------------------------------------------------------------------------------------------ the cases
# (id, arguments): the smallest shapes that reach each form; the settings of a case run inside it (crossed sparingly: every setting on the
# identity rows of every shape, three of them on the var-len rows; the long-T cases are single cases).
FWD_WIDTHS = (8, 72, 520, 768, 1024, 1032, 2048)
LS_FWD_CASES = ([(f"T{T}-d{d}-identity", (T, d, "identity", SETTINGS)) for d in FWD_WIDTHS for T in (5, 35)]
                + [(f"T{VARLEN_T}-d{d}-varlen", (VARLEN_T, d, "varlen", ("elem", "path", "both"))) for d in FWD_WIDTHS])
LS_FWD_LONG = ("T8200-d768: past the 2048-block grid, every wave makes a second trip", (8200, 768, "identity", ("both",)))

# wide: KEY_LS_NORM_BWD_WIDE (1: the 16-byte-chunk form at every width)
LS_BWD_CASES = ([(f"ls4-T{T}-d{d}-identity", (T, d, 0, "identity", SETTINGS)) for d in (512, 768, 1024) for T in (3, 35, 70)]
                + [(f"ls4-T{VARLEN_T}-d{d}-varlen", (VARLEN_T, d, 0, "varlen", ("elem", "path", "both"))) for d in (512, 768, 1024)]
                + [(f"chunk-T35-d{d}-identity", (35, d, 1, "identity", SETTINGS)) for d in (72, 520, 768, 1032, 2048)]
                + [(f"chunk-T{VARLEN_T}-d{d}-varlen", (VARLEN_T, d, 1, "varlen", ("elem", "path", "both"))) for d in (72, 768, 1032)])
LS_BWD_LONG = ("ls4-T20500-d768: past the 1280-block grid, both masks", (20500, 768, 0, "identity", ("both",)))

# the unfused pair: d = 8, 72, 520, 768, 2048 give RL = 256, 28 (four idle threads), 3, 2 and 1 row lanes in ls_bwd
UNFUSED_WIDTHS = (8, 72, 520, 768, 2048)
UNFUSED_CASES = ([(f"T{T}-d{d}-identity", (T, d, "identity", SETTINGS)) for d in UNFUSED_WIDTHS for T in (1, 35)]
                 + [(f"T{VARLEN_T}-d{d}-varlen", (VARLEN_T, d, "varlen", ("elem", "path", "both"))) for d in UNFUSED_WIDTHS])
UNFUSED_LONG = ("T1030-d768: RL = 2, the 512-block grid strides (ls_fwd: 98 880 chunks)", (1030, 768, "identity", ("both",)))

DROP_CASES = ([(f"T{T}-n{n}-stream{s}-identity", (T, n, s, "identity")) for n in (8, 72, 3072) for T in (1, 37) for s in (STREAM_MLP_ACT, STREAM_RAW)]
              + [(f"T{VARLEN_T}-n{n}-stream{STREAM_MLP_ACT}-varlen", (VARLEN_T, n, STREAM_MLP_ACT, "varlen")) for n in (8, 72, 3072)])
DROP_LONG = ("T2740-n3072: T n / 8 = 1 052 160 chunks, past the 4096 x 256 grid", (2740, 3072, STREAM_MLP_ACT, "identity"))

EMBED_CASES = [(f"F{F}-ldF{F + 3}-d{d}-{'gated' if gt else 'plain'}-{kind}", (F, F + 3, d, gt, kind))
               for F in (1, 4, 5, 13) for d in (64, 768) for gt in (True, False) for kind in ("identity", "varlen")]
EMBED_T = 35

HEAD_CASES = [(f"B{B}-48to32-layer{layer}", (B, 48, 32, layer)) for B in (1, 7) for layer in (0, 1)]


def case_seed(*key):
    return 31000 + sum((k + 1) * int(v) for k, v in enumerate(key))


def ls_known(lay, d):
    """The element whose hash the threshold settings sit on: the last row (its LOGICAL row), column d - 3."""
    return int(lay["logical"][-1]), d - 3


def ls_masks(T, d, kind, name):
    """(layout, setting, em [T, d], keep [T]) of one setting of the residual kernels (stream 50 = mlp_out)."""
    lay = layout(kind, T)
    m = setting(name, lay, STREAM_MLP_OUT, case_seed(T, d), ls_known(lay, d))
    return lay, m, elem_mult(m, lay, d), keep_mult(m, lay)


def drop_masks(T, n, stream, kind, name):
    lay = layout(kind, T)
    m = setting(name, lay, stream, case_seed(T, n, stream), ls_known(lay, n), path=False)
    return lay, m, elem_mult(m, lay, n)


def embed_masks(F, d, kind, name):
    """The known cell of the threshold settings: the last row's last feature, channel d - 3."""
    lay = layout(kind, EMBED_T if kind == "identity" else None)
    m = setting(name, lay, STREAM_EMBED, case_seed(F, d), (int(lay["logical"][-1]) * F + F - 1, d - 3), path=False)
    return lay, m, elem_mult(m, lay, d, F=F)


def head_masks(B, Din, layer, name):
    lay = layout("identity", B)
    m = setting(name, lay, STREAM_HEAD + layer, case_seed(B, Din, layer), (B - 1, Din - 3), path=False)
    return lay, m, elem_mult(m, lay, Din)
