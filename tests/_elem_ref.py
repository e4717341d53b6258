"""The element-wise half of every training step - GEGLU (csrc/kernels.hip K9 and the two fused GEMM epilogues), RoPE with its angle tables
(K6, the epilogue of the q|k|v projection) and the stacked-token embedding with its backward forms (K1): seeded inputs, float64 statements
of every operation on the bf16 / fp32 inputs the kernel gets, the per-element error bounds and the checks that hold an implementation to
them.  tests/test_gpu_elem.py feeds the checks with the HIP kernels' outputs, tests/test_elem_reference.py with the fp32 CPU statements
below (which must pass) and with planted faults (which must not).

Bounds.  u = 2^-24 is fp32's unit roundoff, ub = 2^-8 the bf16 term of tests/_util.py:assert_elementwise, always with the factor 1.01 that
absorbs the fp32 roundings relative to the result itself; TINY = 2^-126 is a flushed denormal.  1 ulp of a hardware function counts as 2 u.

GEGLU.  gelu(g) = g Phi(g); csrc/common.h:gelu_parts evaluates q = 1/2 erfc(|g| / sqrt 2) = 1/2 t P(t) gauss, t = 1 / (1 + p |g|),
gauss = exp2(g g k), and Phi = 1 - q or q.  C_CDF bounds the ABSOLUTE error of that Phi, term by term (the suprema over g are taken on a
float64 grid by tests/test_elem_reference.py:test_the_cdf_budget_is_what_the_docstring_says, which holds the literals below to them):
   7.5e-8                half of Abramowitz-Stegun 7.1.26's |eps| <= 1.5e-7 on erf (measured on the grid: 6.97e-8)
   4 K_T u,  K_T = 1.73  t: the fp32 constant p, the fma 1 + p |g| and v_rcp_f32 (1 ulp) are 4 u relative on t, which reaches q through
                         d(t P(t))/dt: K_T = sup 1/2 gauss t |(t P)'(t)| = 1.7222 (at g = 0, where the alternating polynomial cancels most)
   K_H u,    K_H = 1.59  the four Horner fma steps, each u relative to its own intermediate value: sup 1/2 gauss t sum_i |p_i| t^(4-i) = 1.5833
   K_C u,    K_C = 2.24  the five coefficients as fp32 constants: sup 1/2 gauss t sum_i |a_i| t^(i-1) = 2.2376
   (1/2 + 1/2) u         the products p * t and (p t) * gauss, relative to q <= 1/2 (the factor 0.5 is exact)
   1 u                   v_exp_f32, 1 ulp relative to q <= 1/2
   3 K_A u,  K_A = 0.083 the exponent argument g * g * k: two products and the fp32 constant k are 3 u relative on the argument, which is
                         |arg| ln 2 = g^2 / 2 relative on gauss - it scales with |arg| q: K_A = sup (g^2 / 2) q(g) = 0.0829
   1 u                   1 - q (g >= 0)
 C_CDF = 7.5e-8 + (4 K_T + K_H + K_C + 3 + 3 K_A) u = 7.5e-8 + 13.999 u = 9.09e-7.  The fp32 emulation of the formula with an exact
 reciprocal and exp2 (gelu_parts_fp32 below) over all 65 280 finite bf16 inputs measures max |g cdf - gelu(g)| / |g| = 2.2e-7
 (tests/test_elem_reference.py asserts it is below C_CDF and prints it).  The GPU's figure is only recorded, never used to choose C_CDF.
 With u_, dh the up value and the incoming gradient, phi the normal density, all references with torch.special.erfc in float64:
   h  = bf16(bf16(gelu(g)) * u_):  |err| <= 2 x 1.01 ub |ref| + C_CDF |g u_| + TINY (1 + |u_|)
   du = bf16(dh * gelu(g)):        |err| <= 1.01 ub |ref| + C_CDF |g dh| + TINY (1 + |dh|)
   dg = bf16(dh * u_ * gelu'(g)), gelu' = Phi + g phi:
                                   |err| <= 1.01 ub |ref| + |dh u_| (C_CDF + k u (Phi + |g| phi) + 3 K_G u) + 2 TINY
 k = 6: the final fma and the product with dh * u_ (exact: two bf16 factors) are 2 u on the whole of gelu'; the constant 1 / sqrt(2 pi),
 the product g * const and v_exp_f32 (2 u) are 4 u on g phi alone.  3 K_G u, K_G = 0.232: the 3 u of the exponent argument scale with
 g^2 / 2 and reach the derivative through |g| phi: sup (|g|^3 / 2) phi(g) = 0.2313 - an absolute term, because relative to Phi + |g| phi
 it is unbounded in the lower tail.  The TINY terms are multiplied by what a flushed denormal intermediate (bf16(gelu), dh * u_) is
 multiplied with before it reaches the output.  Every finite input must give a finite output (checked by itself; |u_|, |dh| <= 1 where
 |g| >= 2^120, so that no exact result leaves bf16's range).

RoPE.  out_a = a c - b s, out_b = b c + a s on the half-split pairs (j, j + 32) of every head of the q and k thirds, c / s the fp32 table
 values AS INPUTS (inverse: s -> -s):  |err| <= 1.01 ub |ref| + 3 u (|a c| + |b s|) + TINY - two products and the difference, fused into an
 fma or not (so no bit-for-bit claim); the v third and everything behind the last row keep their bits.  inverse(forward(x)) against
 (c^2 + s^2) x: the bound of the inverse pass on the forward's OUTPUT as written, plus the forward's bound carried through the transpose
 rotation, |c| B_a + |s| B_b (and |c| B_b + |s| B_a).
 Tables: angle = pos * inv_freq, inv_freq = 1 / powf(theta, 2j / 64) (the exponent is exact), cos / sin evaluated in double and rounded once:
 |err| <= C_TAB u |angle| + u against the float64 angle of the float64 inverse frequency.  C_TAB = 2 POW_ULP + 2: powf at its documented
 bound (16 ulp = 32 u: the OpenCL bound the device library's pow is built to; HIP's own table lists 1 ulp, CUDA's 4), the division and the
 product; float(pos) is exact.  j = 0 (inv_freq = 1 exactly) must be the correctly rounded cos / sin of the integer position: bit for bit.
 The range table, scaled = float(p) * range / float(max + 1), adds that product and that division: C_RANGE = C_TAB + 2.  The device table
 against the host twin graph-gpt_amd/engine.py:rope_tables is held to the same bound.
 A table whose angle is formed as pos / powf(...) instead of pos * (1 / powf(...)) differs by at most 1.5 u |angle| - a tenth of what the
 documented powf bound allows - so that planted fault cannot be told from a correct table and is not in the list.

Embedding.  Plain stacking sums fp32 values in feature order: bf16(((W[id_0] + W[id_1]) + ...)) is bit for bit what the CPU computes.  Gated
 stacking: |err| <= 1.01 ub |ref| + F u sum_f |W G| + TINY (F products, fused or not, and F - 1 additions).  stack_method = "long":
 ratio = min(1, bf16(1 / (nnz + 1e-7f))) and bf16(x * ratio) are single IEEE operations: bit for bit; rows with ratio == 1 keep their bits.
 Backward, accumulating into demb0 / dgate0:  row v |err| <= 2 (n_v + 1) u (|demb0| + sum_cells |term|) + TINY with n_v the cells that hold
 v - any summation order, atomics included; the dense count-matrix form (a split-K GEMM over the T tokens) 2 (T + 1) u (...); dgate the same
 with T terms.  The pad-id row and the row of every id no cell holds are demb0 bit for bit.
"""
import importlib
import math

import torch

from _heads_ref import TINY, U, gen, held_equal, held_true, randn_bf16, settle  # noqa: F401
from _rows_ref import BF, UB, Bounded, bf, held, held_bits  # noqa: F401

engine = importlib.import_module("graph-gpt_amd.engine")
F32, F64, I64 = torch.float32, torch.float64, torch.int64


def c32(x):
    """A constant as the compiler holds it: rounded to fp32."""
    return torch.tensor(x, dtype=F32)


def fma32(a, b, c):
    """fp32 fma: the product is exact in float64, the sum is rounded to float64 and then to fp32."""
    return (a.double() * b.double() + c.double()).float()


# ------------------------------------------------------------------------------------------------------------------ GEGLU
K_T, K_H, K_C, K_A, K_G = 1.73, 1.59, 2.24, 0.083, 0.232
AS_EPS = 7.5e-8
C_CDF = AS_EPS + (4 * K_T + K_H + K_C + 3 + 3 * K_A) * U
K_GRAD = 6
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
AS_P = 0.3275911
SQRT1_2 = 0.70710678118654752440
EXP2_K = -0.72134752044448170368
INV_SQRT_2PI = 0.39894228040143267794


def cdf_budget(n=400_001):
    """The suprema of the C_CDF derivation on a float64 grid over 0 <= g <= 14 (beyond it gauss < 3e-43 and every term vanishes)."""
    x = torch.linspace(0, 14, n, dtype=F64)
    a = AS_A
    t = 1 / (1 + AS_P * SQRT1_2 * x)
    G = torch.exp(-x * x / 2)
    p1 = a[4] * t + a[3]
    p2 = p1 * t + a[2]
    p3 = p2 * t + a[1]
    p4 = p3 * t + a[0]
    dE = a[0] + 2 * a[1] * t + 3 * a[2] * t ** 2 + 4 * a[3] * t ** 3 + 5 * a[4] * t ** 4
    q = 0.5 * torch.special.erfc(x * SQRT1_2)
    mx = lambda v: float(v.max())   # noqa: E731
    return dict(K_T=mx(0.5 * G * t * dE.abs()), K_H=mx(0.5 * G * t * (p1.abs() * t ** 3 + p2.abs() * t ** 2 + p3.abs() * t + p4.abs())),
                K_C=mx(0.5 * G * t * sum(abs(a[k]) * t ** k for k in range(5))), K_A=mx(x * x / 2 * q),
                K_G=mx(x ** 3 / 2 * G * INV_SQRT_2PI), AS_EPS=mx((0.5 * p4 * t * G - q).abs()))


def bf16_patterns(n):
    """bf16 [n]: element i holds the bit pattern i mod 65 536; the 256 non-finite patterns are overwritten with the patterns of
    -3 ... -13.9, the tail where the polynomial leaves the exactly rounded result."""
    idx = torch.arange(n, dtype=I64) % 65536
    tail = 0xC040 + (idx & 0xFF) + ((idx >> 15) & 1) * 0x20
    bits = torch.where((idx & 0x7F80) == 0x7F80, tail, idx)
    return ((bits ^ 0x8000) - 0x8000).to(torch.int16).view(BF)


PAIR_VALUES = (1.0, -1.0, 0.37, -2.75, 3.0, -0.0045, 1.5 * 2.0 ** -20, -2.0 ** -60, 0.0, -0.71, 1.5e-3, -3.0, 0.11, 2.0, -1.17, 2.0 ** -100)
GEGLU_VARIANTS = 4


def _paired(n, mul, rep_mul, shift, gate):
    i = torch.arange(n, dtype=I64)
    v = torch.tensor(PAIR_VALUES, dtype=F32)[((i % 65536) * mul + (i // 65536) * rep_mul + shift) % len(PAIR_VALUES)]
    big = gate.float().abs() >= 2.0 ** 120
    return torch.where(big, v.clamp(-1.0, 1.0), v).to(BF)


def geglu_inputs(T, ff, variant=0):
    """gu [T, 2 ff] (gate | up) and dh [T, ff]: the gate columns hold every finite bf16 pattern by linear index, each paired with up / dh
    values of both signs and several magnitudes - another one in every repeat of the 65 536 patterns and in every variant."""
    n = T * ff
    gate = bf16_patterns(n)
    assert bool(torch.isfinite(gate.float()).all())
    up = _paired(n, 5, 1, variant * 4, gate)
    dh = _paired(n, 3, 7, variant * 4 + 5, gate)
    gu = torch.cat([gate.view(T, ff), up.view(T, ff)], dim=1).contiguous()
    return dict(T=T, ff=ff, gu=gu, dh=dh.view(T, ff).contiguous())


def covers_every_finite_pattern(i):
    seen = torch.zeros(65536, dtype=torch.bool)
    seen[i["gu"][:, :i["ff"]].contiguous().view(torch.int16).long().view(-1) & 0xFFFF] = True
    idx = torch.arange(65536)
    return bool((seen == ((idx & 0x7F80) != 0x7F80)).all())


def geglu_ref(i):
    """float64 references and bounds of h, dg, du (computed once per inputs)."""
    if "_ref" in i:
        return i["_ref"]
    ff = i["ff"]
    g, u_, dh = i["gu"][:, :ff].double(), i["gu"][:, ff:].double(), i["dh"].double()
    cdf = 0.5 * torch.special.erfc(-g * SQRT1_2)
    gphi = g.abs() * torch.exp(-g * g / 2) * INV_SQRT_2PI
    gelu = g * cdf
    h = gelu * u_
    du = dh * gelu
    dg = dh * u_ * (cdf + torch.sign(g) * gphi)
    gu_abs, gd_abs, du_abs = (g * u_).abs(), (g * dh).abs(), (dh * u_).abs()
    i["_ref"] = dict(h=(h, 2 * 1.01 * UB * h.abs() + C_CDF * gu_abs + TINY * (1 + u_.abs())),
                     du=(du, 1.01 * UB * du.abs() + C_CDF * gd_abs + TINY * (1 + dh.abs())),
                     dg=(dg, 1.01 * UB * dg.abs() + du_abs * (C_CDF + K_GRAD * U * (cdf + gphi) + 3 * K_G * U) + 2 * TINY))
    return i["_ref"]


def _finite(name, t):
    return held_true(f"{name} is finite", bool(torch.isfinite(t.float()).all()), "a finite input gave a non-finite output")


def geglu_fwd_check(i, h):
    ref, bound = geglu_ref(i)["h"]
    return [held("h", h, ref, bound), _finite("h", h)]


def geglu_bwd_check(i, dgu):
    r, ff = geglu_ref(i), i["ff"]
    return [held("dg", dgu[:, :ff], *r["dg"]), held("du", dgu[:, ff:], *r["du"]), _finite("dgu", dgu)]


def gelu_parts_fp32(x):
    """csrc/common.h:gelu_parts in fp32 with an exactly rounded reciprocal and exp2: (cdf, gauss)."""
    t = 1.0 / fma32(c32(AS_P) * c32(SQRT1_2), x.abs(), c32(1.0))
    gauss = torch.exp2(x * x * c32(EXP2_K))
    p = fma32(c32(AS_A[4]), t, c32(AS_A[3]))
    for k in (2, 1, 0):
        p = fma32(p, t, c32(AS_A[k]))
    q = 0.5 * (p * t) * gauss
    return torch.where(x >= 0, 1.0 - q, q), gauss


def gelu_tanh_fp32(x):
    return 0.5 * x * (1.0 + torch.tanh(c32(math.sqrt(2.0 / math.pi)) * (x + c32(0.044715) * x * x * x)))


def geglu_fwd_fp32(i, tanh=False):
    ff = i["ff"]
    g, u_ = i["gu"][:, :ff].float(), i["gu"][:, ff:].float()
    val = gelu_tanh_fp32(g) if tanh else g * gelu_parts_fp32(g)[0]
    return (bf(val) * u_).to(BF)


def geglu_bwd_fp32(i, drop_x_phi=False):
    ff = i["ff"]
    g, u_, dh = i["gu"][:, :ff].float(), i["gu"][:, ff:].float(), i["dh"].float()
    cdf, gauss = gelu_parts_fp32(g)
    grad = cdf if drop_x_phi else fma32(g * c32(INV_SQRT_2PI), gauss, cdf)
    return torch.cat([(dh * u_ * grad).to(BF), (dh * (g * cdf)).to(BF)], dim=1)


def identity_bf16(n, copies=1):
    """`copies` n x n identities stacked along the rows: a projection weight that hands the input through exactly."""
    return torch.eye(n, dtype=BF).repeat(copies, 1).contiguous()


# (T, ff, note): (a) the smallest that hold every pattern once, (b) one work item past the 4096 x 256 grid
GEGLU_CASES = [("T911-ff72: every pattern once, ff = 8 x 9", (911, 72, GEGLU_VARIANTS)),
               ("T8192-ff8: every pattern once, one chunk per row", (8192, 8, GEGLU_VARIANTS)),
               ("T65552-ff128: every thread takes a second grid-stride trip", (65552, 128, 1))]
GEGLU_FUSED_CASES = [("T512-ff128", (512, 128)), ("T171-ff384", (171, 384))]


# ------------------------------------------------------------------------------------------------------------------ RoPE
THETA = 10000.0
POW_ULP = 16
C_TAB = 2 * POW_ULP + 2
C_RANGE = C_TAB + 2


def rope_inputs(B, S, H, max_pos, positions, seed):
    """qkv bf16 [B S, 3 x 64 H], the host tables [max_pos][32] and position ids (None: t % S) - unsorted, with a repeat, with 0 and with
    max_pos - 1, the last table row."""
    g = gen(seed)
    T = B * S
    cos, sin = engine.rope_tables(max_pos, 64, THETA)
    pos = None
    if positions:
        pos = torch.randint(0, max_pos, (T,), generator=g)
        pos[0], pos[1], pos[2] = max_pos - 1, 0, pos[3]
        assert T < 8 or not bool((pos[1:] >= pos[:-1]).all())
    return dict(B=B, S=S, H=H, T=T, qkv=randn_bf16(g, T, 3 * 64 * H), cos=cos, sin=sin, pos=pos, max_pos=max_pos)


def _positions(i):
    return i["pos"] if i["pos"] is not None else torch.arange(i["T"]) % i["S"]


def _rotate64(x, c, s):
    """x [T, 2, H, 2, 32] float64 (the q and k thirds, halves split), c / s [T, 1, 1, 32]: the rotated value and its bound."""
    a, b = x[:, :, :, 0], x[:, :, :, 1]
    oa, ob = a * c - b * s, b * c + a * s
    ref = torch.stack([oa, ob], dim=3)
    mag = torch.stack([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], dim=3)
    return ref, 1.01 * UB * ref.abs() + 3 * U * mag + TINY


def _qk(i, t):
    return t[:, :2 * 64 * i["H"]].double().reshape(i["T"], 2, i["H"], 2, 32)


def _cs(i, inverse, pos=None):
    pos = _positions(i) if pos is None else pos
    c, s = i["cos"][pos].double()[:, None, None, :], i["sin"][pos].double()[:, None, None, :]
    return c, (-s if inverse else s)


def rope_check(i, inverse, got, x=None, tag=""):
    """got [T, 3 d] against the rotation of x (default: the inputs' qkv)."""
    x = i["qkv"] if x is None else x
    d2 = 2 * 64 * i["H"]
    ref, bound = _rotate64(_qk(i, x), *_cs(i, inverse))
    return [held(f"q|k{tag}", got[:, :d2], ref.reshape(i["T"], d2), bound.reshape(i["T"], d2)),
            held_bits(f"the v third keeps its bits{tag}", got[:, d2:].contiguous(), x[:, d2:].contiguous())]


def rope_roundtrip_check(i, y, z):
    """z = inverse(y), y = forward(qkv), both as written: against (c^2 + s^2) qkv with the composition of the two bounds."""
    d2 = 2 * 64 * i["H"]
    c, s = _cs(i, False)
    _, b1 = _rotate64(_qk(i, i["qkv"]), c, s)
    _, b2 = _rotate64(_qk(i, y), c, -s)
    carried = torch.stack([c.abs() * b1[:, :, :, 0] + s.abs() * b1[:, :, :, 1], c.abs() * b1[:, :, :, 1] + s.abs() * b1[:, :, :, 0]], dim=3)
    ref = (c * c + s * s).unsqueeze(3) * _qk(i, i["qkv"])
    return [held("inverse(forward(q|k))", z[:, :d2], ref.reshape(i["T"], d2), (b2 + carried).reshape(i["T"], d2)),
            held_bits("the v third keeps its bits through both passes", z[:, d2:].contiguous(), i["qkv"][:, d2:].contiguous())]


def rope_fp32(i, inverse, x=None, flip_chunk=None, neighbour=False):
    """The kernel's arithmetic in fp32, products and difference rounded one by one; flip_chunk: the sign of sin flipped on the 8-wide chunk
    of that number; neighbour: every token rotated by the position of the token before it."""
    x = i["qkv"] if x is None else x
    T, H = i["T"], i["H"]
    pos = _positions(i)
    if neighbour:
        pos = pos.roll(1)
    c, s = i["cos"][pos][:, None, None, :], i["sin"][pos][:, None, None, :]
    s = -s if inverse else s
    if flip_chunk is not None:
        s = s.clone()
        s[..., 8 * flip_chunk:8 * flip_chunk + 8] *= -1
    qk = x[:, :2 * 64 * H].float().reshape(T, 2, H, 2, 32)
    a, b = qk[:, :, :, 0], qk[:, :, :, 1]
    out = x.clone()
    out[:, :2 * 64 * H] = torch.stack([a * c - b * s, b * c + a * s], dim=3).reshape(T, -1).to(BF)
    return out


def table_ref(pos64, theta):
    """float64 angle [n, 32] of float64 positions with the float64 inverse frequency, its cos / sin and the bound's |angle|."""
    inv = float(c32(theta)) ** (-2.0 * torch.arange(32, dtype=F64) / 64.0)
    angle = pos64.double().reshape(-1, 1) * inv
    return angle.cos(), angle.sin(), angle.abs()


def table_check(cos, sin, max_pos, theta):
    """The device table [max_pos][32] against float64 and against the host twin, both inside C_TAB u |angle| + u; column 0 bit for bit."""
    pos = torch.arange(max_pos, dtype=F64)
    rc, rs, ang = table_ref(pos, theta)
    bound = C_TAB * U * ang + U
    hc, hs = engine.rope_tables(max_pos, 64, theta)
    return [held("cos table", cos, rc, bound), held("sin table", sin, rs, bound),
            held("cos table against the host table", cos, hc.double(), bound), held("sin table against the host table", sin, hs.double(), bound),
            held_equal("cos table, j = 0: the rounded cos of the position", cos[:, 0], pos.cos().float()),
            held_equal("sin table, j = 0: the rounded sin of the position", sin[:, 0], pos.sin().float())]


def table_fp32(max_pos, theta, neighbour_freq=False):
    """The kernel's arithmetic on the CPU (the host twin evaluates cos / sin in fp32; the kernel in double, rounded once)."""
    inv = 1.0 / (c32(theta) ** (torch.arange(0, 64, 2, dtype=F32) / 64))
    if neighbour_freq:
        inv = inv.roll(1)
    fr = torch.arange(max_pos, dtype=F32)[:, None] * inv[None, :]
    return fr.double().cos().float(), fr.double().sin().float()


def range_inputs(B, S, seed):
    """Positions [B, S] below 2^24: row 0 all zeros (den = 1), the maximum of row 1 first, of row 2 last, of row 3 in the middle."""
    g = gen(seed)
    assert B >= 4
    pos = torch.randint(0, 5000, (B, S), generator=g)
    pos[0] = 0
    pos[1, 0], pos[2, S - 1], pos[3, S // 2] = 70001, 8191, 2 ** 24 - 2
    return dict(B=B, S=S, pos=pos, range=float(c32(37.5)), theta=THETA)


def range_check(i, cos, sin, ids):
    B, S = i["B"], i["S"]
    p = i["pos"].double()
    scaled = p * i["range"] / (p.max(1, keepdim=True).values + 1.0)
    rc, rs, ang = table_ref(scaled.reshape(-1), i["theta"])
    bound = C_RANGE * U * ang + U
    return [held("cos range table", cos, rc, bound), held("sin range table", sin, rs, bound),
            held_equal("ids are the identity list", ids.reshape(-1), torch.arange(B * S, dtype=I64))]


def range_fp32(i, max_of_neighbour=False):
    p = i["pos"].float()
    mx = p.max(1, keepdim=True).values
    if max_of_neighbour:
        mx = mx.roll(1, 0)
    scaled = p * c32(i["range"]) / (mx + 1.0)
    inv = 1.0 / (c32(i["theta"]) ** (torch.arange(0, 64, 2, dtype=F32) / 64))
    fr = (scaled.reshape(-1, 1) * inv[None, :]).double()
    return fr.cos().float(), fr.sin().float(), torch.arange(i["B"] * i["S"], dtype=I64)


def clamp_inputs(n, max_pos, clamped, seed):
    g = gen(seed)
    pos = torch.randint(0, max_pos, (n,), generator=g)
    pos[0], pos[n - 1] = 0, max_pos - 1
    if clamped:
        pos[1], pos[2], pos[n // 2], pos[n - 2] = -1, max_pos, -2 ** 40, 2 ** 40
    return pos


def clamp_check(pos, max_pos, flag0, out, flag):
    inside = (pos >= 0) & (pos < max_pos)
    want_flag = 1 if (flag0 or not bool(inside.all())) else 0
    return [held_equal("clamped positions", out, pos.clamp(0, max_pos - 1)), held_equal("positions in range are handed through", out[inside], pos[inside]),
            held_true("flag", int(flag) == want_flag, f"the sticky flag is {int(flag)}, expected {want_flag} (preset {flag0})")]


ROPE_CASES = [(f"B3-S40-H{H}-{'ids' if p else 'no-ids'}", (3, 40, H, 64, p)) for H in (1, 2, 3, 12) for p in (False, True)]
ROPE_BIG = ("B257-S256-H2: T x H = 131 584, the grid-stride loop runs twice", (257, 256, 2, 256, False))
TABLE_SIZES = (1, 64, 2048)
RANGE_CASES = [("B5-S40", (5, 40)), ("B4-S300: the row loop passes 256 threads", (4, 300))]
QKV_ROPE_CASES = [(f"B{B}-S{S}-d{d}-{'ids' if p else 'no-ids'}", (B, S, d, p))
                  for B, S, d in ((3, 40, 128), (64, 32, 768), (128, 64, 384), (16, 72, 1024)) for p in (False, True)]


def rope_case(B, S, H, max_pos, positions):
    return rope_inputs(B, S, H, max_pos, positions, seed=11000 + B + S + 7 * H + int(positions))


# ------------------------------------------------------------------------------------------------------------------ embedding forward
def embed_fwd_inputs(T, F, ldF, d, V, gated, seed):
    """ids [T, ldF]: about 40 % the hot id 1, token 0 all pad (0), token 1 all hot; the gap columns F..ldF hold V - 1 (in range, so a kernel
    that read them would not fault - it would be off by a row of W)."""
    g = gen(seed)
    ids = torch.randint(0, V, (T, ldF), generator=g)
    ids[torch.rand(T, ldF, generator=g) < 0.4] = 1
    ids[0] = 0
    if T > 1:
        ids[1] = 1
    ids[:, F:] = V - 1
    return dict(T=T, F=F, ldF=ldF, d=d, V=V, ids=ids, emb=randn_bf16(g, V, d), gate=(torch.randn(F, d, generator=g) * 0.5 + 1).to(BF) if gated else None)


def embed_fwd_fp32(i, skip_last=False):
    """The sum in feature order, fp32; skip_last: the last feature left out when F % 4 != 0."""
    acc = torch.zeros(i["T"], i["d"])
    for f in range(i["F"]):
        if skip_last and i["F"] % 4 and f == i["F"] - 1:
            break
        w = i["emb"][i["ids"][:, f]].float()
        acc = acc + (w * i["gate"][f].float() if i["gate"] is not None else w)
    return acc.to(BF)


def embed_fwd_check(i, out):
    if i["gate"] is None:
        return [held_bits("out is bf16 of the fp32 sum in feature order", out, embed_fwd_fp32(i))]
    ref, mag = torch.zeros(i["T"], i["d"], dtype=F64), torch.zeros(i["T"], i["d"], dtype=F64)
    for f in range(i["F"]):
        t = i["emb"][i["ids"][:, f]].double() * i["gate"][f].double()
        ref += t
        mag += t.abs()
    return [held("out (gated)", out, ref, 1.01 * UB * ref.abs() + i["F"] * U * mag + TINY)]


def long_inputs(T, F, ldF, d, seed):
    """ids whose rows hold 0, 1, 2, 3, F non-zero ids in turn (the gap columns are non-zero: they do not count), x bf16 [T, d]."""
    g = gen(seed)
    ids = torch.zeros(T, ldF, dtype=I64)
    nnz = [(0, 1, 2, 3, F)[t % 5] for t in range(T)]
    for t, n in enumerate(nnz):
        ids[t, torch.randperm(F, generator=g)[:min(n, F)]] = 5 + t
    ids[:, F:] = 9
    return dict(T=T, F=F, ldF=ldF, d=d, ids=ids, x=randn_bf16(g, T, d), nnz=torch.tensor([min(n, F) for n in nnz]))


def long_fp32(i, round_ratio=True):
    nnz = (i["ids"][:, :i["F"]] != 0).sum(1).float()
    r = 1.0 / (nnz + c32(1e-7))
    ratio = torch.minimum(bf(r) if round_ratio else r, c32(1.0))[:, None]
    return torch.where(ratio == 1.0, i["x"], (i["x"].float() * ratio).to(BF)), ratio.view(-1)


def long_check(i, x):
    want, ratio = long_fp32(i)
    keep = ratio == 1.0
    assert bool(keep[i["nnz"] <= 1].all()) and not bool(keep[i["nnz"] >= 2].any())
    return [held_bits("x is bf16(x * min(1, bf16(1 / (nnz + 1e-7))))", x, want),
            held_bits("rows with ratio 1 keep their bits", x[keep].contiguous(), i["x"][keep].contiguous())]


EMBED_FWD_CASES = [(f"T37-F{F}-ldF{F + 3}-d{d}-{'gated' if gt else 'plain'}", (37, F, F + 3, d, 211, gt))
                   for F, d in ((1, 64), (3, 768), (4, 1088), (5, 64), (13, 768), (13, 1088)) for gt in (False, True)]
LONG_CASES = [(f"T23-F{F}-ldF{F + 2}-d{d}", (23, F, F + 2, d)) for F, d in ((4, 64), (13, 768), (5, 1088))]


def embed_fwd_case(T, F, ldF, d, V, gated):
    return embed_fwd_inputs(T, F, ldF, d, V, gated, seed=12000 + F + d + int(gated))


# ------------------------------------------------------------------------------------------------------------------ embedding backward
SEG, HIST_CELLS = 128, 4096


def _bwd_ids(T, F, ldF, V, pad_id, layout, g):
    """Cell ids with a chosen histogram.  `big` (the hot id 1, or 0 when 1 is the pad id) takes most cells: its run in the sorted order
    spans several whole 128-cell segments and ends 100 cells into one; the next id has the 28 cells up to that segment's end (a run that
    ends exactly on a boundary, inside one segment); the other ids have 1, 2, 3, 1, ... cells (runs inside a segment, some cut by a
    boundary); the last five ids and the pad id have none in the sum.  layout "waves": the hot cells fill 60 of 64 lanes of the first
    waves and no lane of the others."""
    ncell = T * F
    if layout == "pad-only":
        ids = torch.full((T, ldF), pad_id, dtype=I64)
        ids[:, F:] = V - 1
        return ids, dict(big=None, hot=0, pads=ncell)
    big = 1 if pad_id != 1 else 0
    if ncell <= HIST_CELLS:     # (too few cells for the histogram above: about 40 % hot, 10 % pad, the others at random)
        ids = torch.randint(0, V - 5, (T, ldF), generator=g)
        r = torch.rand(T, ldF, generator=g)
        ids[r < 0.4] = big
        ids[r > 0.9] = pad_id
        ids[:, F:] = V - 1
        return ids, dict(big=big, hot=int((ids[:, :F] == big).sum()), pads=int((ids[:, :F] == pad_id).sum()))
    small = [v for v in range(V - 5) if v not in (pad_id, big)]
    before = [v for v in small if v < big]
    after = [v for v in small if v > big]
    counts = {v: 2 for v in before}
    budget = ncell - 7 - sum(counts.values()) - (3 * SEG + 100) - 28
    assert budget > 0 and after, (T, F, V)
    counts[after[0]] = 28
    for k, v in enumerate(after[1:]):
        c = 1 + k % 3
        if c > budget:
            break
        counts[v] = c
        budget -= c
    n_before = sum(counts[v] for v in before)
    hot = 3 * SEG + 100 + budget
    hot -= (n_before + hot - 100) % SEG
    assert hot >= 3 * SEG and (n_before + hot) % SEG == 100
    others = torch.cat([torch.full((c,), v, dtype=I64) for v, c in counts.items()])
    pads = ncell - hot - len(others)
    assert 7 <= pads < 7 + SEG
    others = torch.cat([others, torch.full((pads,), pad_id, dtype=I64)])
    others = others[torch.randperm(len(others), generator=g)]
    if layout == "waves":
        nw = hot // 60
        assert nw * 4 <= len(others) and hot % 60 <= len(others) - nw * 4
        head = torch.cat([torch.full((nw, 60), big, dtype=I64), others[:nw * 4].view(nw, 4)], dim=1).view(-1)
        rest = torch.cat([torch.full((hot % 60,), big, dtype=I64), others[nw * 4:]])
        rest = torch.cat([rest[:64][torch.randperm(min(64, len(rest)), generator=g)], rest[64:]])
        cells = torch.cat([head, rest])
    else:
        cells = torch.cat([torch.full((hot,), big, dtype=I64), others])
        cells = cells[torch.randperm(ncell, generator=g)]
    assert len(cells) == ncell
    ids = torch.full((T, ldF), V - 1, dtype=I64)
    ids[:, :F] = cells.view(T, F)
    return ids, dict(big=big, hot=hot, pads=pads)


def embed_bwd_inputs(T, F, ldF, d, V, pad_id, gated, seed, layout="random"):
    g = gen(seed)
    ids, meta = _bwd_ids(T, F, ldF, V, pad_id, layout, g)
    return dict(T=T, F=F, ldF=ldF, d=d, V=V, pad_id=pad_id, ids=ids, meta=meta, dx=randn_bf16(g, T, d), emb=randn_bf16(g, V, d),
                gate=(torch.randn(F, d, generator=g) * 0.5 + 1).to(BF) if gated else None, demb0=torch.randn(V, d, generator=g),
                dgate0=torch.randn(F, d, generator=g) if gated else None)


def embed_bwd_ref(i):
    """float64 (computed once per inputs): the sum of every row's cells, their absolute sum, the cell count per id; the same for dgate."""
    if "_ref" in i:
        return i["_ref"]
    T, F, d, V = i["T"], i["F"], i["d"], i["V"]
    dx = i["dx"].double()
    s, a, n = torch.zeros(V, d, dtype=F64), torch.zeros(V, d, dtype=F64), torch.zeros(V, dtype=F64)
    gs = ga = None
    if i["gate"] is not None:
        gs, ga = torch.zeros(F, d, dtype=F64), torch.zeros(F, d, dtype=F64)
    for f in range(F):
        idf = i["ids"][:, f]
        m = idf != i["pad_id"]
        term = dx * i["gate"][f].double() if i["gate"] is not None else dx
        s.index_add_(0, idf[m], term[m])
        a.index_add_(0, idf[m], term[m].abs())
        n.index_add_(0, idf[m], torch.ones(int(m.sum()), dtype=F64))
        if gs is not None:      # (the forward stacks the pad row like any other: its gate gradient counts every token)
            tg = dx * i["emb"][idf].double()
            gs[f], ga[f] = tg.sum(0), tg.abs().sum(0)
    i["_ref"] = (s, a, n, gs, ga)
    return i["_ref"]


def embed_bwd_check(i, demb, dgate, dense=False):
    """demb fp32 [V, d] (dgate fp32 [F, d] or None) after the launch; dense: the count-matrix form's T-term bound."""
    s, a, n, gs, ga = embed_bwd_ref(i)
    d0 = i["demb0"].double()
    terms = torch.full_like(n, float(i["T"])) if dense else n
    out = [held("demb", demb, d0 + s, 2 * (terms[:, None] + 1) * U * (d0.abs() + a) + TINY),
           held_equal("the pad-id row and the rows of ids no cell holds keep demb0", demb[n == 0], i["demb0"][n == 0])]
    assert float(n[i["pad_id"]]) == 0 and int((n == 0).sum()) >= 6
    if gs is not None:
        g0 = i["dgate0"].double()
        out.append(held("dgate", dgate, g0 + gs, 2 * (i["T"] + 1) * U * (g0.abs() + ga) + TINY))
    return out


def sorted_cells(i):
    """(id, cell) of the non-pad cells in the order of the counting sort's result (by id; the order inside a run is the launch's own)."""
    F = i["F"]
    flat = i["ids"][:, :F].reshape(-1)
    cells = (flat != i["pad_id"]).nonzero().view(-1)
    order = torch.sort(flat[cells], stable=True)
    return order.values, cells[order.indices]


def run_paths(i):
    """How many runs of the sorted order lie inside one 128-cell segment (read-add-store), how many are cut by a boundary (atomics), and
    whether some run inside a segment ends exactly on its boundary."""
    idv, _ = sorted_cells(i)
    if not len(idv):
        return dict(inside=0, cut=0, ends_on_boundary=False)
    _, counts = torch.unique_consecutive(idv, return_counts=True)
    end = counts.cumsum(0)
    beg = end - counts
    inside = beg // SEG == (end - 1) // SEG
    return dict(inside=int(inside.sum()), cut=int((~inside).sum()), ends_on_boundary=bool((inside & (end % SEG == 0)).any()),
                whole_segments=int(((end // SEG) - ((beg + SEG - 1) // SEG)).clamp_min(0).max()))


def embed_bwd_sorted_fp32(i, fault=None):
    """The sorted scatter-add in fp32: every 128-cell segment of the sorted cells adds one partial sum per run to its row.  Faults:
    "pad" - the pad cells are summed into the pad row; "overwrite" - a run inside one segment stores its sum instead of adding it to the
    accumulator; "lose-cut" - of a run cut by a segment boundary only the first part is added."""
    F = i["F"]
    idv, cells = sorted_cells(i)
    if fault == "pad":
        flat = i["ids"][:, :F].reshape(-1)
        order = torch.sort(flat, stable=True)
        idv, cells = order.values, order.indices
    terms = i["dx"].float()[cells // F]
    if i["gate"] is not None:
        terms = terms * i["gate"].float()[cells % F]
    out = i["demb0"].clone()
    if len(idv):
        _, counts = torch.unique_consecutive(idv, return_counts=True)
        end = counts.cumsum(0).tolist()
        b = 0
        for e in end:
            v = int(idv[b])
            first = True
            while b < e:
                stop = min(e, (b // SEG + 1) * SEG)
                part = terms[b:stop].sum(0)
                whole = first and stop == e
                if fault == "overwrite" and whole:
                    out[v] = part
                elif not (fault == "lose-cut" and not first):
                    out[v] += part
                first = False
                b = stop
    dgate = None
    if i["gate"] is not None:
        dgate = i["dgate0"].clone()
        for f in range(F):
            dgate[f] += (i["dx"].float() * i["emb"][i["ids"][:, f]].float()).sum(0)
    return out, dgate


def dense_plan(T, V, d, num_cu=256):
    """(64-row K-tiles, split asked for, K-tiles per slab, slabs) of csrc/engine.hip:embed_bwd on a device of num_cu CUs."""
    ktiles = (T + 63) // 64
    split = min(max(ktiles // 4, 1), 8)
    t_big, t_small = ((V + 255) // 256) * ((d + 127) // 128), ((V + 127) // 128) * ((d + 127) // 128)
    tiles = t_big if t_big * split >= 160 else t_small
    while split > 1 and tiles * split > num_cu:
        split -= 1
    per = (ktiles + split - 1) // split
    return ktiles, split, per, (ktiles + per - 1) // per


def embed_bwd_dense_fp32(i, drop_last_slab=False):
    """The count-matrix form in fp32: one partial product C^T dX per slab of `per` K-tiles, summed in slab order onto the accumulator."""
    T, F, V = i["T"], i["F"], i["V"]
    cnt = torch.zeros(T, V)
    for f in range(F):
        idf = i["ids"][:, f]
        m = idf != i["pad_id"]
        cnt[m.nonzero().view(-1), idf[m]] += 1
    _, _, per, nslab = dense_plan(T, V, i["d"])
    acc = None
    for sl in range(nslab - (1 if drop_last_slab else 0)):
        r = slice(sl * per * 64, min(T, (sl + 1) * per * 64))
        part = cnt[r].t() @ i["dx"][r].float()
        acc = part if acc is None else acc + part
    return (i["demb0"] + acc if acc is not None else i["demb0"].clone()), None


# name -> (T, F, ldF, d, V, pad_id, gated, layout); T F > 4096 cells (two histogram blocks) and no multiple of 128
EMBED_SORTED_CASES = [
    ("lds-histogram-V97-gated-d768", (331, 13, 15, 768, 97, 0, True, "random")),
    ("lds-histogram-V1500-plain-d1088", (331, 13, 15, 1088, 1500, 0, False, "random")),
    ("lds-histogram-V1500-plain-d64-pad-id-2", (331, 13, 14, 64, 1500, 2, False, "random")),
    ("lds-histogram-V97-gated-d64-pad-id-1: the hot id is the pad id", (331, 13, 15, 64, 97, 1, True, "random")),
    ("ballot-V8193-plain-d64: the hot id in 60 lanes of some waves, in none of the others", (1400, 13, 14, 64, 8193, 0, False, "waves")),
    ("ballot-V8193-gated-d64-pad-id-1", (1400, 13, 14, 64, 8193, 1, True, "random")),
    ("pad-ids-only-V97-gated-d64", (331, 13, 15, 64, 97, 0, True, "pad-only")),
    ("pad-ids-only-V8193-plain-d64", (331, 13, 15, 64, 8193, 0, False, "pad-only")),
]


def _dense_note(T, V, d):
    kt, split, per, nslab = dense_plan(T, V, d)
    edge = "one partial K-tile" if kt == 1 else (f"nslab {nslab} < split {split}" if nslab < split else "several slabs")
    return f"{kt} K-tiles, split {split}, {per} per slab, {nslab} slabs ({edge}, on 256 CUs)"


# un-gated V <= 1024: the count-matrix form (key 0) and the sorted form (key 1) on the same inputs
EMBED_BOTH_CASES = [(f"V{V}-T{T}-d{d}: {_dense_note(T, V, d)}", (T, 13, 15, d, V, 0, False, "random"))
                    for V, d in ((97, 64), (97, 1088), (756, 768)) for T in (37, 777, 2100)]


def embed_bwd_case(T, F, ldF, d, V, pad_id, gated, layout):
    return embed_bwd_inputs(T, F, ldF, d, V, pad_id, gated, seed=13000 + T + d + V + 3 * pad_id + int(gated), layout=layout)
