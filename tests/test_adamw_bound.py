"""The bounds of tests/_adamw_ref.py validated without a device: csrc/kernels.hip adamw_coef + adamw_update4 restated in numpy float32,
operation by operation in the kernel's order - once with every product and sum rounded on its own, once with every multiply-add
fused (computed in float64, rounded once) - must stay inside the bounds on the input families meant for the device, at steps 1, 2, 7,
100 and 1000 and both beta pairs; seven wrong restatements must each leave them.  The largest ratios are printed: they show how much
of the bound the arithmetic alone uses before any kernel runs.

One observation (it depends on the C library's powf; the test prints the current figures), (b2, t) = (0.999, 2): sqrt(bc2) as the
host forms it in fp32 was 55.6 u off against d2 = 500.8 u, bc1 (b1 = 0.9) 1.26 u off against d1 = 9.5 u - the formulas assume a full
ulp of powf and are kept as
derived (test_host_bias_corrections_within_d1_d2 prints every pair).  In that run the fp32 restatement used at most 0.33 of the m
bound, 0.28 of the v bound and 0.28 of the w bound."""
import math
import os
import re

import numpy as np
import pytest
import torch

import _adamw_ref as R

F = np.float32
STEPS = (1, 2, 7, 100, 1000)
BETAS = ((0.9, 0.95), (0.9, 0.999))
N = 1 << 17


def _rne_bf16_bits(x):
    b = x.view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def kernel_f32(w, m, v, g, h, t, fused=False, mut=None):
    """(w', m', v', P' bits, reported norm) of one step in fp32, as the kernels order it.  g: the bf16 gradients widened to fp32 (exact);
    the sum of squares is taken in float64 and rounded once (the norm's summation is checked on its own).  mut: one of the wrong
    restatements of test_wrong_restatement_leaves_the_bound."""
    lr, b1, b2, eps, wd, max_norm, gs = (F(x) for x in (h.lr, h.b1, h.b2, h.eps, h.wd, h.max_norm, h.gs))
    one = F(1.0)
    fma = (lambda a, b, c: (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F)) if fused else (lambda a, b, c: a * b + c)
    # adamw_coef
    sq = F(np.sum(g.astype(np.float64) ** 2))
    nrm = np.sqrt(sq) * (one if mut == "scale_after_clip" else gs)
    coef = gs
    if max_norm > 0:
        coef = coef * min(one, max_norm / (nrm if mut == "no_1e-6" else nrm + F(1e-6)))
    # k_adamw (host)
    bc1, bc2_sqrt = R.host_bias_corrections(b1, b2, t)
    if mut == "no_bc2":
        bc2_sqrt = one
    # adamw_update4
    ge = g * coef
    if mut == "l2_decay":
        ge = ge + wd * w
    m1 = fma(m, b1, (one - b1) * ge)
    v1 = fma(v, b2, (one - b2) * ge * ge)
    decay = (one - np.float64(lr) * np.float64(wd)).astype(F) if fused else one - lr * wd
    denom = np.sqrt(v1 + eps) / bc2_sqrt if mut == "eps_in_root" else np.sqrt(v1) / bc2_sqrt + eps
    q = m1 / denom
    if mut == "l2_decay":
        w1 = fma(q, -(lr / bc1), w)
    elif mut == "decay_after":
        w1 = fma(q, -(lr / bc1), w) * decay
    else:
        w1 = fma(q, -(lr / bc1), w * decay)
    P = (w1.view(np.uint32) >> 16).astype(np.uint16) if mut == "truncate_bf16" else _rne_bf16_bits(w1)
    return w1, m1, v1, P, nrm


def _run(seed, h, t, clip, small=False, world=1, fused=False, mut=None, n=N):
    """one restated step on the families; {check: (ratio, elements outside)} incl. the norm against float64"""
    w, m, v, g, h = R.make_inputs(n, seed, h, small=small, world=world, clip=clip)
    g_arena = (g.float() * world).to(torch.bfloat16)            # (what a loopback exchange leaves; exact for a power of two)
    wn, mn, vn, gn = (x.numpy() for x in (w, m, v, g_arena.float()))
    with np.errstate(all="raise", under="ignore"):
        w1, m1, v1, P, nrm = kernel_f32(wn, mn, vn, gn, h, t, fused=fused, mut=mut)
    pre = dict(w=w, m=m, v=v, g=g_arena)
    post = dict(w=torch.from_numpy(w1), m=torch.from_numpy(m1), v=torch.from_numpy(v1),
                P=torch.from_numpy(P.view(np.int16)).view(torch.bfloat16))
    out = R.verify_step(pre, post, h, t, R.coef64(h, nrm))
    r, _ = R.norm_ratio(nrm, g_arena, h.gs, 1)                  # (one rounding of the sum here: L = 1)
    out["norm"] = (r, int(r > 1.0))
    return out


CASES = [("off", False, 1.0, 1), ("negative", False, 0.25, 1), ("inactive", False, 1.0, 1), ("active", False, 1.0, 1),
         ("active", False, 0.25, 1), ("small", True, 1.0, 1), ("small", True, 0.25, 1), ("active", False, 0.5, 2), ("active", False, 0.25, 4)]


@pytest.mark.parametrize("b1,b2", BETAS)
def test_fp32_restatement_stays_inside_the_bounds(b1, b2):
    worst = {}
    for t in STEPS:
        for clip, small, gs, world in CASES:
            for fused in (False, True):
                out = _run(7 + t, R.Hyper(b1=b1, b2=b2, gs=gs), t, clip, small=small, world=world, fused=fused)
                for k, (r, bad) in out.items():
                    worst[k] = max(worst.get(k, 0.0), r)
                    assert bad == 0, f"{k}: {bad} elements outside the bound (ratio {r:.3f}) at t={t} clip={clip} gs={gs} fused={fused}"
    print(f"[adamw-bound] betas ({b1}, {b2}): largest |fp32 restatement - float64| / bound = "
          + ", ".join(f"{k} {r:.4f}" for k, r in sorted(worst.items())))
    assert worst["w"] > 0 and worst["m"] > 0 and worst["v"] > 0       # (the comparison is not vacuous)


def test_input_condition_holds_at_the_device_sizes():
    """the families at the arena sizes of the tiny and a 2-layer d = 768 model (the small-norm scaling depends on n)"""
    for n in (1_300_000, 22_000_000):
        for clip, small, gs in (("small", True, 0.25), ("active", False, 0.25)):
            h0 = R.Hyper(b2=0.999, gs=gs)
            w, m, v, g, h = R.make_inputs(n, 3, h0, small=small, clip=clip)
            nrm = R.norm64(g, h.gs)
            ge = g.double() * R.coef64(h, R.f32(nrm))
            assert bool(((ge == 0) | ((1.0 - h.b2) * ge * ge >= 2.0 ** -100)).all())
            if small:
                assert abs(nrm - 1e-4) < 2e-6 and h.max_norm == R.f32(1e-5)


@pytest.mark.parametrize("mut,clip,small,gs", [("eps_in_root", "off", False, 1.0), ("no_bc2", "off", False, 1.0),
                                               ("l2_decay", "off", False, 1.0), ("decay_after", "off", False, 1.0),
                                               ("no_1e-6", "small", True, 1.0), ("scale_after_clip", "active", False, 0.25),
                                               ("truncate_bf16", "off", False, 1.0)])
@pytest.mark.parametrize("b1,b2", BETAS)
def test_wrong_restatement_leaves_the_bound(mut, clip, small, gs, b1, b2):
    """each defect the suite could not see before puts elements outside a bound (step 2: d2 is at its widest but one there)"""
    good = _run(11, R.Hyper(b1=b1, b2=b2, gs=gs), 2, clip, small=small)
    assert all(bad == 0 for _, bad in good.values())
    out = _run(11, R.Hyper(b1=b1, b2=b2, gs=gs), 2, clip, small=small, mut=mut)
    caught = {k: bad for k, (_, bad) in out.items() if bad}
    print(f"[adamw-bound] {mut} ({b1}, {b2}): outside the bound {caught}")
    assert caught, f"{mut} stays inside every bound"


def test_host_bias_corrections_within_d1_d2():
    """the 1-ulp assumption on powf behind d_bc, for every (b, t) used, against float64; the measured errors of bc1 and sqrt(bc2)"""
    for b1, b2 in BETAS:
        for t in STEPS + (3,):
            for b in (R.f32(b1), R.f32(b2)):
                p32 = float(np.power(F(b), F(t), dtype=F))
                p64 = b ** t
                # 1 ulp is at most 2u relative - or the smallest fp32 step where b^t underflows (0.9^1000 = 1.7e-46: bc is exactly 1 then)
                assert abs(p32 - p64) <= max(2.0 * R.U * p64, 2.0 ** -149), (b, t)
            h = R.Hyper(b1=b1, b2=b2)
            bc1, bc2s = R.host_bias_corrections(h.b1, h.b2, t)
            e1 = abs(float(bc1) - (1.0 - h.b1 ** t)) / (1.0 - h.b1 ** t)
            e2 = abs(float(bc2s) - math.sqrt(1.0 - h.b2 ** t)) / math.sqrt(1.0 - h.b2 ** t)
            d1, d2 = R.d1_d2(h, t)
            print(f"[adamw-bound] ({b1}, {b2}) t={t}: bc1 off by {e1 / R.U:.2f} u (d1 = {d1 / R.U:.1f} u), "
                  f"sqrt(bc2) off by {e2 / R.U:.2f} u (d2 = {d2 / R.U:.1f} u)")
            assert e1 <= d1 and e2 <= d2


def test_chain_lengths():
    """L of the three norm paths at sizes worked out by hand"""
    assert R.chain_full(8 * 256 * 1024) == 8 + 6 + 4 + 4 + 8            # one vector per thread, 1024 blocks
    assert R.chain_full(2048) == 8 + 6 + 4 + 1 + 8                      # one block
    assert R.chain_full(8 * 256 * 1024 * 7 + 8) == 64 + 6 + 4 + 4 + 8   # the eighth vector of the first thread
    assert R.chain_shard([(0, 4096 * 1024), (4096 * 1024, 4096)]) == 16 + 6 + 4 + 2 + 10
    assert R.chain_chunks(1_000_000, 2) == 128 + 6 + 4 + 4 + 2 + 8      # 32768-element chunks dominate the 72-element tile share


def test_launch_constants_match_the_sources():
    """the constants behind L are restated in _adamw_ref.py: each is read back from the source that owns it, so a changed launch shape
    fails here and not silently in the norm bound"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = lambda *p: open(os.path.join(root, *p)).read()
    kernels, optimizer, gemm, header = (src("graph-gpt_amd", "csrc", f) for f in ("kernels.hip", "optimizer.hip", "gemm.hip", "kernels.h"))
    const = lambda text, name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert const(kernels, "kBlock") == R.KBLOCK
    assert const(kernels, "kSqnormBlocks") == R.SQNORM_BLOCKS
    assert const(kernels, "kSlotsBlock") == R.SLOTS_BLOCK
    assert const(optimizer, "kSqTilesPerLayer") == R.SQ_TILES_PER_LAYER
    assert const(header, "kAdamwItemElems") == 8 * R.KBLOCK
    assert int(re.search(r"#define GGET_SHARD_CHUNK (\d+)", src("include", "gget.h")).group(1)) == R.SHARD_CHUNK
    # the chunk rule of the norm's table, the cap of that table, the tile of the grouped weight-gradient launch and its eight waves
    assert "std::max<uint64_t>(32768, align_up((other + 899) / 900, 128))" in optimizer and "chunks.size() <= 1024" in optimizer
    assert "/ (192 * 192)" in optimizer and R.WG_TILE == 192 * 192
    assert "for (int w = 0; w < 8; ++w) t += red[w];" in gemm and R.WG_THREADS == 8 * 64
    # the loop shapes the chains count: eight squares per vector, lanes by wave_sum, waves by thread 0, a halving tree
    assert kernels.count("for (int e = 0; e < 8; ++e) s += v[e] * v[e];") == 3
    assert "for (int j0 = threadIdx.x; j0 < n; j0 += 8 * kSlotsBlock)" in kernels
