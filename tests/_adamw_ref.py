"""The float64 restatement of one clip + AdamW step, its per-element rounding bounds, the bound of the gradient norm and the input
families - shared by tests/test_adamw_bound.py (CPU: the bounds validated against an fp32 restatement of the kernel) and
tests/test_gpu_adamw_exact.py (the device).  torch tensors on any device; nothing here touches the engine.

Restatement (csrc/kernels.hip adamw_update4 / adamw_coef; w, m, v fp32 and g bf16 as they are in the arenas BEFORE the step, the
hyper-parameters rounded to fp32 first - the values that crossed the ABI -, t the 1-based step, c the coefficient; u = 2^-24,
everything in float64):
    ge = g c                      m' = b1 m + (1 - b1) ge               v' = b2 v + (1 - b2) ge^2
    bc1 = 1 - b1^t                bc2 = 1 - b2^t                        denom = sqrt(v') / sqrt(bc2) + eps
    U  = (lr / bc1) (|b1 m| + |(1 - b1) ge|) / denom                    (the update's magnitude before cancellation)
    w' = w (1 - lr wd) - (lr / bc1) m' / denom
Bounds, from counting the roundings of adamw_update4 (a fused multiply-add only removes roundings; 1 - b is exact in fp32 for
b >= 0.5; the kernel's fp32 c is within 3u of the float64 c rebuilt from the norm the device reported: one sum, one quotient, one
product):
    ge: 3u + 1 = 4u.
    m': b1 m carries its product and the sum (2u), (1 - b1) ge carries 4u + product + sum (6u):  |dm'| <= 6u (|b1 m| + |(1 - b1) ge|)
    v': ((1 - b2) ge) ge carries 4u + 4u + two products + the sum (11u), b2 v 2u:                |dv'| <= 11u v'
    w': w (1 - lr wd) carries lr wd (negligible), 1 - x (u/2), the product (u) and the final difference (u |w'| <= u |w| + u U);
        the update carries m' (6u, relative to U), sqrt(v') (11u/2 + 1), the quotient by sqrt(bc2) (1 + d2), the sum with eps (1),
        m' / denom (1), lr / bc1 (1 + d1), their product (1) and its share of the final difference (1) = 19.5u + d1 + d2:
                                                                                     |dw'| <= 8u |w| + (24u + d1 + d2) U
    P' == round-to-nearest-even bf16 of the device's own master', bit for bit.
d1, d2: the errors of the host's fp32 bias corrections, 1.0f - powf(b, t) then sqrtf.  With powf within 1 ulp (2u relative) and the
difference exact or rounded once:  d_bc(b, t) = u (1 + 2 b^t / (1 - b^t)),  d1 = d_bc(b1, t),  d2 = d_bc(b2, t) / 2 + u.
Input condition (asserted, never filtered): every element has ge == 0 or (1 - b2) ge^2 >= 2^-100 - nothing underflows."""
import math

import numpy as np
import torch

U = 2.0 ** -24
KBLOCK = 256                # csrc/kernels.hip kBlock
SQNORM_BLOCKS = 1024        # kSqnormBlocks
SLOTS_BLOCK = 1024          # kSlotsBlock
SHARD_CHUNK = 4096          # include/gget.h GGET_SHARD_CHUNK
SQ_TILES_PER_LAYER = 256    # csrc/optimizer.hip kSqTilesPerLayer
WG_TILE = 192 * 192         # elements of one weight-gradient tile (csrc/optimizer.hip wg_tiles), summed by a block of 512 threads
WG_THREADS = 512
_SLICE = 1 << 24            # elements per slice of a check (bounds the float64 temporaries)


def f32(x):
    """the value after it crossed the ABI as a C float"""
    return float(np.float32(x))


class Hyper:
    def __init__(self, lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.1, max_norm=1.0, gs=1.0):
        self.lr, self.b1, self.b2, self.eps, self.wd, self.max_norm, self.gs = (f32(x) for x in (lr, b1, b2, eps, wd, max_norm, gs))

    def replace(self, **kw):
        h = Hyper(self.lr, self.b1, self.b2, self.eps, self.wd, self.max_norm, self.gs)
        for k, x in kw.items():
            setattr(h, k, f32(x))
        return h


def d_bc(b, t):
    p = b ** t
    return U * (1.0 + 2.0 * p / (1.0 - p))


def d1_d2(h, t):
    return d_bc(h.b1, t), d_bc(h.b2, t) / 2.0 + U


def host_bias_corrections(b1, b2, t):
    """(bc1, sqrt(bc2)) as k_adamw forms them in fp32: 1.0f - powf(b, (float)t), sqrtf"""
    one = np.float32(1.0)
    bc1 = one - np.power(np.float32(b1), np.float32(t), dtype=np.float32)
    bc2 = one - np.power(np.float32(b2), np.float32(t), dtype=np.float32)
    return np.float32(bc1), np.sqrt(np.float32(bc2), dtype=np.float32)


def coef64(h, nrm32):
    """the coefficient rebuilt in float64 from the fp32 norm the device reported"""
    if h.max_norm <= 0.0:
        return h.gs
    return h.gs * min(1.0, h.max_norm / (float(nrm32) + f32(1e-6)))


def norm64(g, gs=1.0):
    """sqrt(sum g^2) gs with the sum in float64"""
    s = 0.0
    for o in range(0, g.numel(), _SLICE):
        s += float(g[o: o + _SLICE].double().pow(2).sum())
    return math.sqrt(s) * gs


# ------------------------------------------------------------------------------------------------ L: the longest chain of fp32 additions
def _cdiv(a, b):
    return -(-a // b)


def chain_full(n):
    """k_grad_sqnorm: blocks = min(1024, ceil((n/8) / 256)); a thread adds the 8 squares of every 16-byte vector it owns, serially
    (ceil(nv / (blocks 256)) vectors), wave_sum folds 64 lanes in 6 steps, thread 0 adds the 4 wave sums, the final block adds
    ceil(blocks / 256) partials per thread and folds 256 threads in an 8-level tree."""
    nv = n // 8
    blocks = max(1, min(SQNORM_BLOCKS, _cdiv(nv, KBLOCK)))
    return 8 * _cdiv(nv, blocks * KBLOCK) + 6 + KBLOCK // 64 + _cdiv(blocks, KBLOCK) + 8


def chain_chunks(n, layers):
    """k_grad_sqnorm_chunks + the weight-gradient tiles' partials.  A chunk of the table is max(32768, (other + 899) / 900 rounded
    up to 128) elements, `other` <= n the elements outside the layers' matrices (n is used here: conservative): 8 ceil(chunk / 8 / 256) serial additions, 6 (wave_sum), 4 (waves).  A tile partial is 192 x 192 stored bf16
    values over 512 threads: 72 serial additions, 6, 8 (waves).  The final block adds at most ceil(1024 / 256) chunk partials and
    layers x 256 / 256 tile partials per thread, then the 8-level tree.  The tile sums square the value AFTER its bf16 rounding
    (csrc/gemm.hip sq_add: bf2f(f2bf(v))) - the stored gradient, so no extra term."""
    chunk = max(32768, _cdiv((n + 899) // 900, 128) * 128)      # (optimizer.hip cuts `other` <= n elements, the non-matrix share: an upper bound)
    in_block = max(8 * _cdiv(chunk // 8, KBLOCK) + 6 + KBLOCK // 64, WG_TILE // WG_THREADS + 6 + WG_THREADS // 64)
    return in_block + _cdiv(1024, KBLOCK) + _cdiv(layers * SQ_TILES_PER_LAYER, KBLOCK) + 8


def chain_shard(buckets):
    """k_grad_sqnorm_partials + k_grad_sqnorm_slots: a chunk is at most 4096 elements (16 serial additions per thread, 6, 4); the one
    block of 1024 threads adds ceil(chunks / 1024) slots per thread and folds them in a 10-level tree.  buckets: [(offset, count)]."""
    nglobal = sum(_cdiv(c, SHARD_CHUNK) for _, c in buckets)
    return 8 * _cdiv(SHARD_CHUNK // 8, KBLOCK) + 6 + KBLOCK // 64 + _cdiv(nglobal, SLOTS_BLOCK) + 10


def norm_ratio(nrm32, g, gs, chain):
    """|nrm - nrm64| / ((L + 4) u nrm64): squares are non-negative, so L additions bound the sum's relative error by L u and the
    root's by half that; the 4 covers the multiply, the root and the grad_scale multiply."""
    ref = norm64(g, gs)
    return abs(float(nrm32) - ref) / ((chain + 4) * U * ref), ref


# ------------------------------------------------------------------------------------------------ the per-element check
def _ratio(err, bound):
    """(largest err / bound, elements outside); where the bound is 0 the error must be 0"""
    bad = int((err > bound).sum())
    pos = bound > 0
    r = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    return r, bad


def verify_step(pre, post, h, t, c):
    """pre / post: dicts of flat tensors w, m, v (fp32), g (bf16; pre only), P (bf16; post only).  Every element of every arena is
    checked; returns {check: (largest |err| / bound, elements outside the bound)} - `P` counts the bits that differ."""
    d1, d2 = d1_d2(h, t)
    bc1, bc2 = 1.0 - h.b1 ** t, 1.0 - h.b2 ** t
    out = {"m": (0.0, 0), "v": (0.0, 0), "w": (0.0, 0), "P": (0.0, 0)}
    n = pre["w"].numel()
    for o in range(0, n, _SLICE):
        s = slice(o, o + _SLICE)
        w, m, v, g = (pre[k][s].double() for k in ("w", "m", "v", "g"))
        ge = g * c
        small = (ge != 0) & ((1.0 - h.b2) * ge * ge < 2.0 ** -100)
        assert not bool(small.any()), f"input condition: {int(small.sum())} elements have (1 - b2) ge^2 below 2^-100"
        a, b = h.b1 * m, (1.0 - h.b1) * ge
        m1 = a + b
        v1 = h.b2 * v + (1.0 - h.b2) * ge * ge
        denom = v1.sqrt() / math.sqrt(bc2) + h.eps
        mag = (h.lr / bc1) * (a.abs() + b.abs()) / denom
        w1 = w * (1.0 - h.lr * h.wd) - (h.lr / bc1) * m1 / denom
        for key, ref, bound in (("m", m1, 6 * U * (a.abs() + b.abs())), ("v", v1, 11 * U * v1),
                                ("w", w1, 8 * U * w.abs() + (24 * U + d1 + d2) * mag)):
            got = post[key][s].double()
            err = (got - ref).abs()
            err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
            r, bad = _ratio(err, bound)
            out[key] = (max(out[key][0], r), out[key][1] + bad)
        want = post["w"][s].to(torch.bfloat16).view(torch.int16)          # (torch rounds to nearest even)
        diff = int((want != post["P"][s].view(torch.int16)).sum())
        mismatches = out["P"][1] + diff
        out["P"] = (1.0 if mismatches else 0.0, mismatches)      # (no ratio for a bitwise check: 1.0 = some bf16 value differs)
    return out


# ------------------------------------------------------------------------------------------------ the input families
FAMILIES = ("typical", "typical", "typical", "near_cancelling", "large_v_tiny_g", "tiny_v_large_g", "sweep", "all_zero")
BLOCK = 1024    # elements per family block: kind = (index / 1024) mod 8


def _randn(n, gen, dev):
    """a standard normal kept away from 0 (|x| >= 0.05): no element underflows by chance"""
    x = torch.randn(n, generator=gen, device=dev)
    return torch.where(x < 0, -torch.ones_like(x), torch.ones_like(x)) * x.abs().clamp_min(0.05)


def make_inputs(n, seed, h, device="cpu", covered=None, small=False, world=1, clip="off"):
    """(w, m, v fp32, g bf16, hyper) of an arena of n elements, zero outside `covered` (bool [n]; None = everything):
      typical          w ~ 0.05 N, m ~ 1e-3 N, v ~ (1e-3 N)^2, g ~ 1e-2 N
      near_cancelling  b1 m = -(1 - b1) ge (1 + 1e-3 N): m' is a thousandth of its two terms
      large_v_tiny_g   v ~ 1e2, |g| ~ 1e-9 (1e-3 when `small`);   tiny_v_large_g  v ~ 1e-16, |g| ~ 1
      sweep            |g| = 10^x, x uniform in [-10, 2] ([-3, 1] when `small`)
      all_zero         g = m = v = 0, w != 0
    `small`: the gradients are scaled so that the norm (grad_scale included) is 1e-4.  `world`: a loopback exchange multiplies the
    arena by `world` before the step (and grad_scale is 1 / world): the near-cancelling block is built for the gradients it will
    meet.  `clip`: "off" / "negative" (max_norm 0 / -1), "inactive" (max_norm = 2 norm), "active" (norm / 2), "small" (1e-5; with
    small=True) - the returned hyper carries the max_norm."""
    gen = torch.Generator(device=device).manual_seed(seed)
    idx = torch.arange(n, device=device)
    kind = (idx // BLOCK) % len(FAMILIES)
    fam = lambda name: torch.isin(kind, torch.tensor([i for i, f in enumerate(FAMILIES) if f == name], device=device))
    w = 0.05 * _randn(n, gen, device)
    m = 1e-3 * _randn(n, gen, device)
    v = (1e-3 * _randn(n, gen, device)) ** 2
    g = 1e-2 * _randn(n, gen, device)
    sign = torch.where(torch.rand(n, generator=gen, device=device) < 0.5, -1.0, 1.0)
    lo, hi = (-3.0, 1.0) if small else (-10.0, 2.0)
    g = torch.where(fam("sweep"), sign * 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=gen, device=device)), g)
    g = torch.where(fam("large_v_tiny_g"), sign * (1e-3 if small else 1e-9) * (1.0 + torch.rand(n, generator=gen, device=device)), g)
    v = torch.where(fam("large_v_tiny_g"), 1e2 * (1.0 + torch.rand(n, generator=gen, device=device)), v)
    g = torch.where(fam("tiny_v_large_g"), sign * (1.0 + torch.rand(n, generator=gen, device=device)), g)
    v = torch.where(fam("tiny_v_large_g"), 1e-16 * (1.0 + torch.rand(n, generator=gen, device=device)), v)
    zero = fam("all_zero")
    g, m, v = (torch.where(zero, torch.zeros_like(x), x) for x in (g, m, v))
    if covered is not None:
        w, m, v, g = (torch.where(covered, x, torch.zeros_like(x)) for x in (w, m, v, g))
    if small:
        g = g * (1e-4 / (norm64(g.to(torch.bfloat16)) * h.gs * world))
    g = g.to(torch.bfloat16)
    nrm = norm64(g, h.gs * world)   # (what the device will report, after the exchange multiplied the arena by `world`)
    max_norm = {"off": 0.0, "negative": -1.0, "inactive": 2.0 * nrm, "active": 0.5 * nrm, "small": 1e-5}[clip]
    h = h.replace(max_norm=max_norm)
    ge = g.double() * (world * coef64(h, f32(nrm)))
    nc = fam("near_cancelling") if covered is None else fam("near_cancelling") & covered
    cancel = -(1.0 - h.b1) / h.b1 * ge * (1.0 + 1e-3 * _randn(n, gen, device).double())
    m = torch.where(nc, cancel.float(), m)
    return w, m, v, g, h
