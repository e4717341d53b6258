"""The fused attention + o-projection kernels of csrc/attention.hip behind gget_op_attn_oproj_fwd / gget_op_attn_oproj_bwd (and the
list-driven launch of attn_bwd_long_kernel behind the two _list entries): float64 statements and per-element bounds, stage by stage, the
seeded inputs, the case table and plain fp32 CPU statements with planted faults.  tests/test_gpu_layer_exact.py feeds the checks with the
HIP kernels' outputs, tests/test_layer_ref.py with the fp32 statements (which must pass) and the faults (which must not).

Every stage is stated on the inputs THE KERNEL ITSELF consumed: where the kernel wrote that tensor (attn_out, x_mid, dx_mid, dattn_long)
the check takes the kernel's bf16 values, so a bound counts one stage's roundings.  Attention (out, lse, dq, dk, dv; Problem, held,
round_flips) is tests/_attn_out_ref.py's, the RMSNorm forward / backward and the replica sums tests/_rows_ref.py's; what is stated here:

 forward (attn_oproj_fwd_kernel<H>)
   attn_out, lse   _attn_out_ref.forward_check; q / k are taken as rotated in memory (phase 1, :1302-1390)
   x_mid           x_in + attn_out_got Wo^T.  The residual is added on the fp32 accumulator and the sum is rounded once (:1449-1452):
                   b |ref|  +  1.01 * 2 (d + 1) u (|x_in| + sum |a| |w|)  +  2^-126: one bf16 rounding (pack2bf :1452), fp32 accumulation
                   of d products and the residual in any order (the 2 n u rule of _heads_ref; the K loop :1419-1442 starts at K-step
                   (5 b) mod (d / 32) and wraps, the order differs per sample), 1.01 for the rounding of the erroneous sum, the flush floor.
   rstd, xn        _rows_ref._norm_checks on the kernel's bf16 x_mid: the sum of squares is taken from the rounded values (:1453-1455).
   rows of no sample (var-len layout: everything behind the last sample, lse behind a sample's rows) are untouched.
 backward (attn_oproj_bwd_kernel<H>, attn_oproj_bwd_long<H>, attn_bwd_long_kernel)
   dx_mid          _rows_ref.bwd_ref on the samples' rows (phase A :1737-1799, :1533-1597: rmsnorm_bwd_kernel's arithmetic)
   dw              per replica r, from its non-zero start: dw0[r] + sum over the rows of the samples b with b % copies == r (:1817, :1615;
                   the partials leave through the two-plane permutation j = (ix >> 2) * 8 + pl * 4 + (ix & 3), :1810-1817) under
                   _rows_ref._accum_check's bound with T = those rows; reproducible mode: everything in replica 0 (:3490-3509).
                   Columns past d and replicas past `copies` are untouched.
   dattn_long      rows of 33 .. 64-row samples: dx_mid_got Wo;  b |ref| + 1.01 * 2 n u sum |dx| |w| + 2^-126 (pack2bf :1674, the K loop
                   :1640-1664).  Other rows untouched.
   dqkv            samples of <= 32 rows: dattn never reaches memory, the statement forms dO = bf16(float64(dx_mid_got Wo)) and
                   _attn_out_ref.round_flips the possible one-spacing deviation e_dO where the exact value lies within the fp32
                   accumulation error 2 n u sum |dx| |w| (n non-zero terms) of a rounding boundary (:1866-1903); samples of 33 .. 64 rows: dO =
                   dattn_long_got, e_dO = 0.  Then _attn_out_ref.backward64 with delta from P and dP (:1923-1935, :947-961); with
                   tables the RoPE kind is "memory": dq and dk are rotated back.
   pad rows        the generator puts zeros in dxn and dres on rows without a token, as the engine's gradients are there.  Padded layout:
                   those rows of dx_mid and dqkv are exact zeros.  Var-len layout: rows [cu[B], t_rows) of dx_mid are exact zeros (:1734,
                   and :1710 when the last sample is long) and no row of dqkv there is written.

Wo is dense N(0, 0.03^2) in the forward and where every sample is long; where the backward holds samples of <= 32 rows it is "sparse"
(sparse_wo says why) or, with dxn = 0, "exact" (dense integers; Layer).

Input kinds of the o projection: "unit" - seeded normal x_in, Wo scaled 0.03; "cancelling" - x_in = -bf16(attn Wo^T) + small with the
attention output of the fp32 statement, so |x_mid| << |y| = |attn Wo^T| and a second rounding of the GEMM output before the add (2^-9 |y|)
stands far above the bound.  Its bounds are held to the vacuous cap of tests/test_layer_ref.py on |y|'s scale, not on |x_mid|'s: x_mid
there is the difference of two numbers fifty times its size.
"""
import torch

import _attn_out_ref as A
import _gpu_out as G
import _heads_ref as H
import _rows_ref as R

U, TINY, BF, DH = A.U, A.TINY, A.BF, A.DH
EPS = 1e-6
LONG_GRID = 32            # kLongGrid of csrc/attention.hip :3326
PD = 4                    # GGET_AO_PD :1260
SMALL = 0.02              # "cancelling": x_mid is about SMALL times the mean |y|
BOUNDED = ("out", "lse", "x_mid", "rstd", "xn", "dx_mid", "dw", "dattn_long", "dq", "dk", "dv")


def sent16(*shape):
    return torch.full(shape, G.SENT16, dtype=torch.int16).view(torch.bfloat16)


def sent32(*shape):
    return torch.full(shape, G.SENT32, dtype=torch.int32).view(torch.float32)


def intact(t):
    """Every element still holds the NaN sentinel of tests/_gpu_out.py."""
    if t.numel() == 0:
        return True
    if t.dtype == torch.bfloat16:
        return bool((t.view(torch.int16) == G.SENT16).all())
    return bool((t.contiguous().view(torch.int32) == G.SENT32).all())


# ------------------------------------------------------------------------------------------------------------------ the case table
def _case(entry, B, S, Hn, lens, varlen, causal=0, p=0.0, kind="unit", rope=False, copies=1, det=False, listed=False, akind=None, wkind=None):
    lens = tuple(lens)
    assert len(lens) == B and max(lens) <= S
    # q | k | v: "unit" in the forward; "rising" in the backward, whose dq / dk bounds on N(0,1) inputs without a mask exceed the cap on vacuous
    # bounds (the note at BWD_SHORT of _attn_out_ref) - q / k are rotated in memory here, so the kind's pattern survives the RoPE cases
    akind = akind or ("unit" if entry == "fwd" else "rising")
    # Wo: dense N(0, 0.03^2), but "sparse" (sparse_wo) wherever the backward holds a sample of <= 32 rows to the e_dO statement
    wkind = wkind or ("dense" if entry == "fwd" or (varlen and min(lens) > 32) else "sparse")
    c = dict(entry=entry, B=B, S=S, Hn=Hn, lens=lens, varlen=varlen, causal=causal, p=p, kind=kind, rope=rope, copies=copies, det=det,
             listed=listed, akind=akind, wkind=wkind)
    ln = "_".join(map(str, lens)) if B <= 6 else f"{B}lens"
    c["id"] = (f"{entry}-H{Hn}B{B}S{S}-{'varlen' if varlen else 'padded'}-len{ln}-c{causal}-p{p}-{kind}" + ("-rope" if rope else "")
               + {"dense": "", "sparse": "-sparse_wo", "exact": "-exact_wo"}[wkind] + (f"-copies{copies}" if entry != "fwd" else "")
               + ("-det" if det else "") + ("-list" if listed else ""))
    return c


def cyc(B, pattern):
    return tuple(pattern[i % len(pattern)] for i in range(B))


COMBOS = ((0, 0.0), (1, 0.0), (0, 0.1))          # (causal, p): both masks and dropout, not the full product
HEADS = (2, 4, 8, 12)
LENS32 = (32, 17, 29, 1)


def forward_cases():
    """B = 2 H + 1: gcd(5, 2 H) = 1, so the samples start the K loop at every K-step (5 b) mod 2 H, the wrapping ones included."""
    cs = []
    for i, Hn in enumerate(HEADS):
        B = 2 * Hn + 1
        for j, (varlen, kind) in enumerate(((False, "unit"), (True, "unit"), (True, "cancelling"))):
            causal, p = COMBOS[(i + j) % 3]
            cs.append(_case("fwd", B, 32, Hn, cyc(B, LENS32), varlen, causal, p, kind))
    cs.append(_case("fwd", 3, 24, 4, (24, 9, 1), False, 1, 0.1))          # rows [S, 32) of the tile are dead
    cs.append(_case("fwd", 1, 8, 2, (1,), False))
    return cs


def backward_cases():
    cs = []
    for i, Hn in enumerate(HEADS):
        B = 2 * Hn + 1
        for j, (varlen, rope, copies) in enumerate(((False, False, 1), (True, True, 4), (bool(i % 2), not i % 2, B + 3))):
            causal, p = COMBOS[(i + j) % 3]
            cs.append(_case("bwd", B, 32, Hn, cyc(B, LENS32), varlen, causal, p, rope=rope, copies=copies))
    cs.append(_case("bwd", 3, 24, 4, (24, 9, 1), False, 1, 0.1, rope=True, copies=4))
    for i, Hn in enumerate(HEADS):      # the dense K loop under the one-tile samples' dqkv: operands whose fp32 sums are exact (Layer)
        causal, p = COMBOS[(i + 1) % 3]
        cs.append(_case("bwd", 2 * Hn + 1, 32, Hn, cyc(2 * Hn + 1, LENS32), bool(i % 2), causal, p, rope=not i % 2, copies=4, wkind="exact"))
    cs.append(_case("bwd", 2, 8, 2, (8, 1), False, copies=1))   # (a one-row sample alone has dq = dk = 0: nothing to hold a bound against)
    # var-len layout with 32 < S <= 64: the last sample long (:1710 zeroes the tail) and short (:1734 does)
    cs.append(_case("bwd_long", 5, 40, 2, (33, 1, 40, 32, 36), True, 0, 0.1, rope=True, copies=4))
    cs.append(_case("bwd_long", 5, 64, 2, (47, 64, 1, 33, 32), True, 1, 0.0, rope=False, copies=1))
    cs.append(_case("bwd_long", 5, 40, 12, (36, 40, 1, 33, 32), True, 1, 0.0, rope=True, copies=8))
    cs.append(_case("bwd_long", 5, 64, 12, (33, 1, 64, 32, 47), True, 0, 0.1, rope=False, copies=4))
    # long samples only: the dense weight (their dO is the dattn that was written, no e_dO)
    cs.append(_case("bwd_long", 3, 64, 2, (33, 64, 47), True, 0, 0.1, rope=True, copies=4))
    cs.append(_case("bwd_long", 3, 40, 12, (40, 33, 36), True, 1, 0.0, rope=False, copies=1))
    return cs


def _list_lens(B, n_long):
    """n_long samples of 33 .. 64 rows spread over the batch, the others short."""
    lens, k = [], 0
    for b in range(B):
        if (b * n_long) // B != ((b + 1) * n_long) // B:
            lens.append((64, 33, 47, 40, 58)[k % 5])
            k += 1
        else:
            lens.append((1, 32, 17, 8)[b % 4])
    assert k == n_long
    return tuple(lens)


def list_cases():
    """More long samples than the LONG_GRID block slots (blocks take a second item) and fewer.  copies = B + 3: every replica takes one
    sample's atomic add, so dw too has the same bits in two launches."""
    return [_case("bwd_list", 70, 64, 2, _list_lens(70, 40), True, 0, 0.1, rope=True, copies=73, listed=True),
            _case("bwd_list", 40, 64, 2, _list_lens(40, 3), True, 1, 0.0, rope=False, copies=43, listed=True)]


def det_cases():
    return [_case("bwd", 9, 32, 4, cyc(9, LENS32), True, 0, 0.1, rope=True, copies=4, det=True),
            _case("bwd_long", 5, 64, 2, (33, 1, 64, 32, 47), True, 1, 0.0, rope=False, copies=4, det=True)]


def long_list_of(c):
    """What gget_op_varlen_plan writes into a zeroed int32 [3 B + 1] (tests/_plan_ref.py varlen_ref)."""
    B = c["B"]
    ll = torch.zeros(3 * B + 1, dtype=torch.int32)
    n, first = 0, 0
    for b, ln in enumerate(c["lens"]):
        if 32 < ln <= 64:
            ll[1 + n], ll[1 + B + n], ll[1 + 2 * B + n] = b, first, ln
            n += 1
        first += ln
    ll[0] = n
    return ll


# ------------------------------------------------------------------------------------------------------------------ inputs
WO_NNZ = 4
EXACT_N = 4               # "exact" operands: integers of at most this magnitude times a power of two


def sparse_wo(g, d):
    """Wo with WO_NNZ non-zeros in every row and column - on the diagonals (k - n) mod d = i (d / 4 + 9), which between them meet every
    K-step of 32 channels - at the dense weight's output scale (0.03 sqrt(d / 4) N(0,1)).
    Why: for the samples of <= 32 rows the backward's dO = bf16(dx_mid Wo) never reaches memory, and the statement can only say that it
    is bf16 of the float64 product unless that product lies within the fp32 accumulation error of a rounding boundary (e_dO of
    _attn_out_ref).  Over d dense terms that error, 2 d u sum |dx| |w|, is of the size of a bf16 half-spacing: 30 % (d = 128) to 97 %
    (d = 768) of the elements would have to be taken as uncertain by a whole spacing, and 10 % to 97 % of the dq / dk bounds would lie
    above the 0.05 (|ref| + rms) that tests/test_layer_ref.py allows 1 % of them (as measured on the fp32 statement; no count of
    roundings avoids it - a k-ordered chain of d additions has that worst case).  With four terms the sum is good to 8 u of its abs-product sum and the
    uncertain elements are a few in ten thousand.  The K loop is the same: every K-step still feeds every accumulator, a skipped or
    doubled step changes the elements whose non-zeros lie in it, and the per-element check says which."""
    w = torch.zeros(d, d)
    n = torch.arange(d)
    for i in range(WO_NNZ):
        w[n, (n + i * (d // 4 + 9)) % d] = torch.randn(d, generator=g) * 0.03 * (d / 4) ** 0.5
    return w.to(torch.bfloat16)


class Layer:
    """The inputs of one case.  Tensors named *_g lie on the padded [B * S] grid, buffers (buf()) hold t_rows rows as the kernel sees
    them: the grid itself (padded layout), or the samples' real rows back to back and pad rows up to a multiple of 64 (var-len)."""

    def __init__(self, c):
        self.c = c
        B, S, Hn = c["B"], c["S"], c["Hn"]
        self.B, self.S, self.Hn, self.d, self.varlen, self.copies = B, S, Hn, Hn * DH, c["varlen"], c["copies"]
        self.pr = pr = A.Problem(B, S, Hn, lens=c["lens"], causal=c["causal"], p=c["p"], kind=c["akind"], rope="memory" if c["rope"] else None)
        lens = torch.tensor(c["lens"])
        self.own = pr.real if self.varlen else torch.ones(B, S, dtype=torch.bool)          # rows the kernels compute
        self.sel = self.own.reshape(-1).nonzero().squeeze(1)
        self.n = len(self.sel)
        self.rows_of = (lens if self.varlen else torch.full((B,), S)).tolist()
        self.first = [sum(self.rows_of[:b]) for b in range(B)]
        self.t_rows = (self.n + 63) // 64 * 64 if self.varlen else B * S
        assert not self.varlen or self.t_rows > self.n, "the var-len cases keep pad rows behind the last sample"
        self.long = [self.varlen and r > 32 for r in self.rows_of]
        self.stride = R.align_up(self.d, 128)
        d = self.d
        g = H.gen(4100 + 7 * B + S + 13 * Hn)
        self.wo = {"dense": lambda: H.randn_bf16(g, d, d, scale=0.03), "sparse": lambda: sparse_wo(g, d),
                   "exact": lambda: (torch.randint(-EXACT_N, EXACT_N + 1, (d, d), generator=g) * 2.0 ** -6).to(torch.bfloat16)}[c["wkind"]]()
        self.nnz = int((self.wo != 0).sum(0).max())          # non-zero terms of a dattn element at the most (zeros add exactly)
        self.nw = (torch.randn(d, generator=g) * 0.1 + 1).to(torch.bfloat16)
        self.x_in_g = H.randn_bf16(g, B * S, d)
        if c["kind"] == "cancelling":
            y = A.forward_fp32(pr)[0].float() @ self.wo.float().t()
            self.x_in_g = (-y.to(torch.bfloat16).float() + torch.randn(B * S, d, generator=g) * SMALL * float(y.abs().mean())).to(torch.bfloat16)
        # the backward's own inputs (independent of the forward: x_mid and rstd as bwd_inputs of _rows_ref makes them)
        tok = pr.real.reshape(-1)[:, None]
        self.x_mid_g = H.randn_bf16(g, B * S, d)
        self.dxn_g = H.randn_bf16(g, B * S, d, scale=0.5) * tok
        self.dres_g = H.randn_bf16(g, B * S, d, scale=0.5) * tok
        if c["wkind"] == "exact":
            # dxn = 0: dx_mid = dres bit for bit (dres + rstd (0 - xhat 0)), and dres and Wo are integers |n| <= EXACT_N times a power of
            # two - every product and every partial sum of dattn = dx_mid Wo, in any order, is an integer multiple of 2^-8 below 2^24 of
            # them (d EXACT_N^2 <= 768 * 16): the fp32 accumulation of the DENSE K loop is exact, the kernel's dO is bf16 of the exact sum
            # and e_dO is zero without a flip to consider (the exact operands of tests/_util.py).  dw stays at its start.
            self.dxn_g = torch.zeros_like(self.dxn_g)
            self.dres_g = (torch.randint(-EXACT_N, EXACT_N + 1, (B * S, d), generator=g) * 0.25).to(torch.bfloat16) * tok
            assert d * EXACT_N ** 2 < 2 ** 24
        self.rstd_g = (self.x_mid_g.double().pow(2).mean(1) + EPS).rsqrt().float()
        self.dw0 = torch.randn(self.copies, d, generator=g)

    def buf(self, grid, fill=0.0):
        t = torch.full((self.t_rows,) + tuple(grid.shape[1:]), fill, dtype=grid.dtype)
        t[:self.n] = grid[self.sel]
        return t

    def grid(self, buf):
        g = torch.zeros((self.B * self.S,) + tuple(buf.shape[1:]), dtype=buf.dtype)
        g[self.sel] = buf[:self.n]
        return g

    def sample_rows(self, b):
        return slice(self.first[b], self.first[b] + self.rows_of[b])

    def long_rows(self):
        m = torch.zeros(self.t_rows, dtype=torch.bool)
        for b in range(self.B):
            if self.long[b]:
                m[self.sample_rows(b)] = True
        return m

    def rows_inputs(self, dres=True):
        """The dict _rows_ref's backward statement takes, on the samples' rows."""
        s = self.sel
        return dict(T=self.n, d=self.d, copies=self.copies, x=self.x_mid_g[s], dy=self.dxn_g[s], w=self.nw, rstd=self.rstd_g[s],
                    dres=self.dres_g[s] if dres else None, dw0=self.dw0)

    def dw_start(self):
        """fp32 [copies + 2, stride]: dw0 in the replicas' first d columns, the sentinel everywhere else."""
        t = sent32(self.copies + 2, self.stride)
        t[:self.copies, :self.d] = self.dw0
        return t


# ------------------------------------------------------------------------------------------------------------------ forward
def x_mid64(ly, attn):
    """(ref, bound, y) of x_mid on the samples' rows from the attention output that was written (bf16 [t_rows, d])."""
    a, w, x = attn[:ly.n].double(), ly.wo.double(), ly.buf(ly.x_in_g)[:ly.n].double()
    y = a @ w.t()
    ref = x + y
    bound = BF * ref.abs() + 1.01 * 2 * (ly.d + 1) * U * (x.abs() + a.abs() @ w.abs().t()) + TINY
    return ref, bound, y


def forward_check(ly, attn, lse, x_mid, xn, rstd, f=None):
    """attn, x_mid, xn bf16 [t_rows, d], rstd fp32 [t_rows], lse fp32 [B,H,S]; what the kernel did not write holds the NaN sentinel."""
    pr, n = ly.pr, ly.n
    res = A.forward_check(pr, ly.grid(attn), lse, f)
    ref, bound, _ = x_mid64(ly, attn)
    res.append(H.held("x_mid", x_mid[:n], ref, bound))
    res += [type(r)(("xn" + r[0][1:],) + tuple(r[1:])) if r[0].startswith("y") else r for r in R._norm_checks(x_mid[:n], ly.nw, EPS, xn[:n], rstd[:n])]
    own_h = ly.own[:, None, :].expand(ly.B, ly.Hn, ly.S)
    ok = all(intact(t[n:]) for t in (attn, x_mid, xn, rstd)) and intact(lse.reshape(ly.B, ly.Hn, ly.S)[~own_h])
    res.append(H.held_true("rows of no sample are untouched", ok, "attn_out, x_mid, xn, rstd or lse was written outside the samples' rows"))
    return res


FWD_FAULTS = ("x_mid_twice", "ss_unrounded", "k_step_twice", "residual_neighbour")
BWD_FAULTS = ("dw_no_permutation", "dw_rows_past_len", "dw_replica0", "dx_no_dres", "dattn_unrounded", "tail_not_zeroed", "list_skips_items",
              "dq_rot_forward")


def wrapping_sample(ly):
    """A sample whose first PD weight fragments wrap around the end of the K loop: (5 b) mod KSTEPS + PD > KSTEPS."""
    ks = ly.d // 32
    return next(b for b in range(ly.B) if (5 * b) % ks + PD > ks and ly.rows_of[b] > 1)


def forward_fp32(ly, fault=None):
    """A plain fp32 CPU statement of the fused forward with the kernel's rounding points: attn, lse, x_mid, xn, rstd as forward_check takes
    them.  fault: the planted faults of tests/test_layer_ref.py."""
    pr, n, d = ly.pr, ly.n, ly.d
    a_g, lse = A.forward_fp32(pr)
    own_h = ly.own[:, None, :].expand(ly.B, ly.Hn, ly.S)
    lse = torch.where(own_h, lse, sent32(1).expand_as(lse))
    attn, x_mid, xn, rstd = sent16(ly.t_rows, d), sent16(ly.t_rows, d), sent16(ly.t_rows, d), sent32(ly.t_rows)
    a = a_g[ly.sel]
    attn[:n] = a
    x_in = ly.x_in_g[ly.sel].float()
    w = ly.wo.float()
    y = a.float() @ w.t()
    if fault == "k_step_twice":      # one K-step used twice and the next one skipped, for one sample
        b = wrapping_sample(ly)
        s = (5 * b) % (d // 32)
        mult = torch.ones(d)
        mult[32 * s:32 * s + 32] = 2.0
        s2 = (s + 1) % (d // 32)
        mult[32 * s2:32 * s2 + 32] = 0.0
        y[ly.sample_rows(b)] = (a.float()[ly.sample_rows(b)] * mult) @ w.t()
    elif fault == "residual_neighbour":
        b = 1
        x_in[ly.sample_rows(b)] = x_in[ly.first[b + 1]:ly.first[b + 1] + ly.rows_of[b]]
    s32 = x_in + (y.to(torch.bfloat16).float() if fault == "x_mid_twice" else y)
    xm = s32.to(torch.bfloat16)
    sq = s32 if fault == "ss_unrounded" else xm.float()
    rs = torch.rsqrt((sq * sq).sum(1) / d + EPS)
    x_mid[:n], rstd[:n] = xm, rs
    xn[:n] = (ly.nw.float() * R.bf(xm.float() * rs[:, None])).to(torch.bfloat16)
    return attn, lse, x_mid, xn, rstd


# ------------------------------------------------------------------------------------------------------------------ backward
def dattn64(ly, dx_mid):
    """dx_mid_got Wo on every row of the buffer (float64) and the fp32 accumulation error 2 n u sum |dx| |w|, n the non-zero terms of an
    element (d for the dense weight; a zero product adds exactly) - zero for the "exact" operands, as long as the dx_mid that was written
    is made of them.  Rows the kernel did not write are taken as zeros."""
    dx = dx_mid.double().nan_to_num(0.0)
    w = ly.wo.double()
    exact = ly.c["wkind"] == "exact" and bool((dx * 4 == (dx * 4).round()).all()) and float(dx.abs().max()) <= EXACT_N / 4
    return dx @ w, (0.0 if exact else 2 * ly.nnz * U) * (dx.abs() @ w.abs())


def dw64(ly, det=False):
    """Per replica: (ref [copies, d], abs-term sums [copies, d], term counts [copies]) without the initial values."""
    i = ly.rows_inputs()
    t = i["dy"].double() * (i["x"].double() * i["rstd"].double()[:, None])
    ref, tabs = torch.zeros(ly.copies, ly.d, dtype=torch.float64), torch.zeros(ly.copies, ly.d, dtype=torch.float64)
    cnt = torch.zeros(ly.copies, dtype=torch.long)
    for b in range(ly.B):
        r = 0 if det else b % ly.copies
        ref[r] += t[ly.sample_rows(b)].sum(0)
        tabs[r] += t[ly.sample_rows(b)].abs().sum(0)
        cnt[r] += ly.rows_of[b]
    return ref, tabs, cnt


def backward64(ly, lse, dx_mid, dattn_long):
    """_attn_out_ref.backward64 on the dO the kernels multiplied: bf16(dx_mid_got Wo) with its possible deviation for the samples of <= 32
    rows, the dattn rows that were written for the longer ones."""
    pr = ly.pr
    exact, eps = dattn64(ly, dx_mid)
    rb, flip = A.round_flips(exact, eps)
    lr = ly.long_rows()[:, None]
    dO = torch.where(lr, dattn_long.double(), rb)
    flip = torch.where(lr | (eps == 0), torch.zeros_like(flip), flip)      # (an exact sum: its tie goes to even in the kernel as here, pack2bf)
    return A.backward64(pr, lse, None, False, dO=ly.grid(dO), e_dO=A.heads(ly.grid(flip), pr.B, pr.S, pr.Hn))


def backward_check(ly, lse, dx_mid, dw, dattn_long, dqkv, det=False, bw=None):
    """dx_mid, dattn_long bf16 [t_rows, d], dqkv bf16 [t_rows, 3 d], dw fp32 [copies + 2, stride] that started as Layer.dw_start()."""
    pr, n, d = ly.pr, ly.n, ly.d
    ref, bound, _, _ = R.bwd_ref(ly.rows_inputs())
    res = [R.held("dx_mid", dx_mid[:n], ref, bound)]
    # the replicas, each from its own start
    dref, dabs, cnt = dw64(ly, det)
    per = [R._accum_check(f"dw replica {r}", dw[r:r + 1, :d], ly.dw0[r:r + 1], dref[r], dabs[r], int(cnt[r])) for r in range(ly.copies)]
    res.append(R.Bounded(("dw", max(x[1] for x in per), "\n".join(x[2] for x in per if x[2] is not None) or None)))
    res.append(H.held_true("dw: columns past d and replicas past `copies` are untouched", intact(dw[:, d:]) and intact(dw[ly.copies:]),
                           "the accumulator was written outside its replicas"))
    # dattn of the long samples
    lr = ly.long_rows()
    if bool(lr.any()):
        exact, eps = dattn64(ly, dx_mid)
        res.append(H.held("dattn_long", dattn_long[lr], exact[lr], BF * exact[lr].abs() + 1.01 * eps[lr] + TINY))
    res.append(H.held_true("dattn_long: rows of no long sample are untouched", intact(dattn_long[~lr]), "a dattn row of another sample was written"))
    # attention backward
    bw = bw or backward64(ly, lse, dx_mid, dattn_long)
    res += A.backward_check(pr, ly.grid(dqkv), lse, None, False, bw=bw, pad_zero=not ly.varlen)
    if ly.varlen:
        res.append(H.held_true("dx_mid: the pad rows behind the last sample are zero", bool((dx_mid[n:] == 0).all()), "a pad row is not zero"))
        res.append(H.held_true("dqkv: no row behind the last sample is written", intact(dqkv[n:]), "a pad row of dqkv was written"))
    else:
        pad = ~pr.real.reshape(-1)
        res.append(H.held_true("dx_mid: rows without a token are zero", bool((dx_mid[pad] == 0).all()), "a row without a token is not zero"))
    return res


def plane_permutation(d):
    """j of the kernel's plane index t (:1810-1813): channel the partial at t belongs to."""
    t = torch.arange(d)
    pl = (t >= d // 2).long()
    ix = t - pl * (d // 2)
    return (ix >> 2) * 8 + pl * 4 + (ix & 3)


def backward_fp32(ly, lse, fault=None, det=False, listed=False):
    """The fused backward in fp32 on the CPU with the kernels' rounding points: dx_mid, dw, dattn_long, dqkv as backward_check takes them."""
    pr, n, d, B = ly.pr, ly.n, ly.d, ly.B
    i = ly.rows_inputs(dres=fault != "dx_no_dres")
    dx, t = R._dx_fp32(i)
    dx_mid, dattn_long, dqkv = sent16(ly.t_rows, d), sent16(ly.t_rows, d), sent16(ly.t_rows, 3 * d)
    dx_mid[:n] = dx
    if ly.varlen and not (fault == "tail_not_zeroed" and ly.long[B - 1]):
        dx_mid[n:] = 0
    dw = ly.dw_start()
    for b in range(B):
        part = t[ly.sample_rows(b)].sum(0)
        if fault == "dw_rows_past_len" and not ly.long[b]:      # the rows [len, 32) of the tile, clamped to the sample's last row, counted
            part = part + (32 - ly.rows_of[b]) * t[ly.first[b] + ly.rows_of[b] - 1]
        if fault == "dw_no_permutation":
            part = part[plane_permutation(d)]
        dw[0 if (det or fault == "dw_replica0") else b % ly.copies, :d] += part
    da32 = dx.float() @ ly.wo.float()
    da = da32.to(torch.bfloat16)
    lr = ly.long_rows()
    dattn_long[lr] = da[lr[:n]]
    dO = torch.zeros(ly.t_rows, d)
    dO[:n] = da32 if fault == "dattn_unrounded" else da.float()
    g = A.backward_fp32(pr, lse, None, False, 0, "dq_rot_forward" if fault == "dq_rot_forward" else None, dO=ly.grid(dO))
    dqkv[:n] = g[ly.sel]
    if fault == "list_skips_items" and listed:      # a launch of LONG_GRID blocks that take one item each
        ll = long_list_of(ly.c)
        for it in range(LONG_GRID, int(ll[0])):
            dqkv[ly.sample_rows(int(ll[1 + it]))] = sent16(1, 1)
    return dx_mid, dw, dattn_long, dqkv
