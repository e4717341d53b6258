"""Plain float64 statements of the GEMM launches whose shape lives on the device (GemmProblem::m_dev / k_dev / k_pad_zero, c_rows) and of
the split-K slab launches with their reduce (csrc/gemm.hip gemm_kernel / gemm_persist_kernel, csrc/kernels.hip slab_reduce_kernel), the
inputs tests/test_gpu_head_gemm.py runs them on, and the checks it holds the kernels to.  tests/test_headgemm_reference.py validates all
of it on the CPU, planted faults included.

The rules:
  m_dev   rows m >= min(M, *m_dev) of the product are not stored;
  c_rows  row m is stored at row c_rows[m] of C, a negative entry means the row is not stored;
  k_dev   the reduction runs over K rows [0, min(K, *k_dev));
  slabs   ktiles = ceil(K / 64) over the K actually reduced, per = ceil(ktiles / split), slice s owns K rows [64 s per, min(K, 64 (s + 1) per)),
          live = ceil(ktiles / per), slabs >= live are not written; the reduce sums slabs in order in fp32 and rounds once (bf16, to nearest
          even), or adds the sum to an fp32 accumulator.
"""
import torch

from _util import assert_elementwise, exact_operands

NT, NN, TN = 0, 1, 2
EPI_NONE, EPI_SLAB = 0, 3
SENT16 = 0x7FC1                      # bf16 NaN payload no kernel writes
SENT32 = 0x7FC01234                  # fp32 NaN payload
PAD_ROWS = 16                        # sentinel rows behind every output
HUGE = 3e38                          # finite bf16 (max 3.39e38): what the B side of a k_pad_zero pad row may hold

WIDTHS = (128, 192)                  # 192 reaches the N % 192 tile plans
N_TOK = 3                            # next_n_token
VOCABS = (200, 205)                  # Vp = 256 for both; 205: the odd vocabulary, NT stores up to 208
T_CAPS = (192, 200)                  # % 64 == 0: the persistent kernel; 200: gemm_kernel with the zero-filling K tail
LAUNCHES = ("ntp_fwd", "lm_fwd", "lm_dgrad", "lm_dgrad_scatter", "lm_wgrad", "ntp_dgrad", "ntp_wgrad")
LM_SPLITS = (1, 2, 5)                # next to the engine's own choice


def counts_for(cap):
    return sorted({0, 1, 63, 64, 65, cap - 1, cap})


def round_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------ the rules
def slab_slices(K, split):
    """K ranges of the live slices of a split-K slab launch over K reduced rows (len = live; K = 0: none)."""
    ktiles = (K + 63) // 64
    if ktiles == 0:
        return []
    per = (ktiles + split - 1) // split
    live = (ktiles + per - 1) // per
    return [(64 * s * per, min(K, 64 * (s + 1) * per)) for s in range(live)]


def product64(mode, A, B, rows, N, k0, k1):
    """fp64 (op(A)[:rows, k0:k1] @ op(B)[k0:k1, :N], |.| @ |.|) from the memory layouts of `mode`: only these elements are read, so
    whatever lies outside them (NaN rows behind a count) cannot reach the result.  An empty K range gives zeros."""
    a = A[k0:k1, :rows].double().t() if mode == TN else A[:rows, k0:k1].double()
    b = B[:N, k0:k1].double().t() if mode == NT else B[k0:k1, :N].double()
    return a @ b + 0.0, a.abs() @ b.abs()       # (+ 0.0: an accumulator that starts at +0 never ends at -0)


def stored_rows(M, m_count, c_rows):
    """(source rows of the product, destination rows of C) that a launch stores."""
    rows = M if m_count is None else max(0, min(M, int(m_count)))
    src = torch.arange(rows)
    if c_rows is None:
        return src, src.clone()
    dst = c_rows[:rows].long().cpu()
    keep = dst >= 0
    return src[keep], dst[keep]


def reduce_ref(slabs, nslab, n, acc=None):
    """slab_reduce_kernel on a flat fp32 buffer of slabs `stride` apart (slabs: [nslab, >= n]): the fp32 sum in slab order, then one RNE
    rounding to bf16, or added to the fp32 accumulator."""
    a = slabs[0, :n].clone()
    for s in range(1, nslab):
        a = a + slabs[s, :n]
    return a + acc[:n] if acc is not None else a.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------ buffers and bit patterns
def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def out_buf(rows, ld, fp32=False, device="cpu", pad=True):
    """[rows + PAD_ROWS][ld] of sentinels."""
    n = (rows + (PAD_ROWS if pad else 0)) * ld
    if fp32:
        return torch.full((n,), SENT32, dtype=torch.int32, device=device).view(torch.float32)
    return torch.full((n,), SENT16, dtype=torch.int16, device=device).view(torch.bfloat16)


def check_image(buf, ld, dst, N, nw, want, what):
    """`buf` (flat, rows of `ld`) holds `want` [len(dst), N] bit for bit at rows `dst`, columns [0, N); columns [N, nw) of those rows are
    free (an odd width is stored up to the next multiple of 4); every other element is the sentinel.  want = None: only the sentinels.
    Returns the stored block."""
    sent = SENT32 if buf.dtype == torch.float32 else SENT16
    img = bits(buf).view(-1, ld)
    free = torch.zeros(img.shape, dtype=torch.bool, device=buf.device)
    dst = dst.to(buf.device)
    free[dst, :nw] = True
    stray = (img != sent) & ~free
    if bool(stray.any()):
        ij = stray.nonzero()
        raise AssertionError(f"{what}: {int(stray.sum())} elements written where nothing is stored (rows {sorted(set(ij[:, 0].tolist()))[:8]}, "
                             f"first (row, col) {ij[:4].tolist()})")
    got = buf.view(-1, ld)[dst][:, :N]
    if want is not None:
        bad = bits(got) != bits(want.to(buf.device))
        if bool(bad.any()):
            ij = bad.nonzero()
            unwritten = int((bits(got) == sent).sum())
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} stored elements differ from the exact result ({unwritten} still the "
                                 f"sentinel); first (source row, col) {ij[:4].tolist()}, 64x64 tiles "
                                 f"{sorted({(r // 64, c // 64) for r, c in ij.tolist()})[:6]}")
    return got


# ------------------------------------------------------------------------------------------ the engine's six head launches
class Case:
    """One launch: operands in the engine's layouts and leading dimensions, its capacities, the count on the device."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def m_count(self):
        return self.count if self.dyn == "m" else None

    @property
    def k_red(self):
        return min(self.K, self.count) if self.dyn == "k" else self.K

    @property
    def nw(self):
        return round_up(self.N, 4)


def launch_shape(launch, d, V, T, n=N_TOK):
    """mode, epilogue, (M, N, K) capacities, ldc, rows of the C buffer, which count is on the device, the count's capacity."""
    Vp = round_up(V, 64)
    return {
        "ntp_fwd": (NT, EPI_NONE, T, n * d, d, n * d, T, "m", T),                        # P = Hm W_ntp^T
        "lm_fwd": (NT, EPI_NONE, T * n, V, d, Vp, T * n, "m", T * n),                      # logits = Hl W_lm^T, ldc = Vp
        "lm_dgrad": (NN, EPI_NONE, T * n, d, Vp, d, T * n, "m", T * n),                    # dHl = dlogits W_lm, K = Vp
        "lm_dgrad_scatter": (NN, EPI_NONE, T * n, d, Vp, d, T * n, "m", T * n),            # ... scattered into dP by sel_src
        "lm_wgrad": (TN, EPI_SLAB, V, d, T * n, d, V, "k", T * n),                         # dW_lm = dlogits^T Hl, lda = Vp
        "ntp_dgrad": (NN, EPI_NONE, T, d, n * d, d, T, "m", T),                            # dHm = dP W_ntp, scattered by row_idx
        "ntp_wgrad": (TN, EPI_NONE, n * d, d, T, d, n * d, "k", T),                        # dW_ntp = dP^T Hm
    }[launch]


def scatter_rows(cap, seed, device):
    """c_rows of a scattering launch: a permutation of [0, cap) with every seventh entry negative (row not stored; never one of the
    rows next to a count of counts_for, so that a count off by one shows)."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(cap, generator=g).to(torch.int32)
    perm[torch.arange(cap) % 7 == 5] = -1
    return perm.to(device)


def make_case(launch, d, V, T, count, exact=True, k_pad_zero=0, seed=0, device="cpu"):
    """Operands of one of the engine's head launches with `count` on the device.  Operand rows at or beyond the count hold NaN; under
    k_pad_zero rows [count, max(64, round_up(count, 64))) of A are zero and those of B are HUGE (the contract of the persistent form: whole
    K-tiles, at least one), NaN behind them."""
    mode, epi, M, N, K, ldc, c_rows_total, dyn, cap = launch_shape(launch, d, V, T)
    assert 0 <= count <= cap
    Vp = round_up(V, 64)
    if exact:
        A, B, _ = exact_operands(M, N, K, seed, mode=mode, device=device)
    else:
        g = torch.Generator(device=device).manual_seed(seed)
        sa, sb = {NT: ((M, K), (N, K)), NN: ((M, K), (K, N)), TN: ((K, M), (K, N))}[mode]
        A = torch.randn(*sa, generator=g, device=device).to(torch.bfloat16)
        B = torch.randn(*sb, generator=g, device=device).to(torch.bfloat16)
    lda, ldb = A.shape[1], B.shape[1]
    if launch == "lm_fwd":                                   # W_lm is allocated [Vp, d], pad rows zero
        B = torch.cat([B, torch.zeros(Vp - V, d, dtype=B.dtype, device=device)])
    if launch in ("lm_dgrad", "lm_dgrad_scatter"):           # K = Vp: zero pads on both sides
        A[:, V:] = 0
        B[V:] = 0
    if launch == "lm_wgrad":                                 # dlogits [T n, Vp] read as M = V columns
        A = torch.cat([A, torch.zeros(K, Vp - V, dtype=A.dtype, device=device)], 1).contiguous()
        lda = Vp
    nan = float("nan")
    if dyn == "m":
        A[count:] = nan
    else:
        pad_end = min(K, max(64, round_up(count, 64))) if k_pad_zero else count
        A[count:pad_end] = 0
        B[count:pad_end] = HUGE
        A[pad_end:] = nan
        B[pad_end:] = nan
    c_rows = scatter_rows(cap, seed + 101, device) if launch in ("lm_dgrad_scatter", "ntp_dgrad") else None
    return Case(launch=launch, mode=mode, epi=epi, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, c_total=c_rows_total, dyn=dyn, cap=cap,
                count=count, k_pad_zero=k_pad_zero, A=A, B=B, c_rows=c_rows, exact=exact, d=d, V=V, T=T)


def name_of(c, split=1):
    return (f"{c.launch} d{c.d} V{c.V} T{c.T} {'m' if c.dyn == 'm' else 'k'}_dev={c.count}/{c.cap} kpz{c.k_pad_zero} split{split} "
            f"{'exact' if c.exact else 'random'}")


def plain_expected(c):
    """(source rows, destination rows, fp64 values [rows, N], fp64 |A| @ |B|) of a plain-epilogue launch."""
    src, dst = stored_rows(c.M, c.m_count, c.c_rows)
    rows = int(src.max()) + 1 if len(src) else 0
    ref, ab = product64(c.mode, c.A, c.B, rows, c.N, 0, c.k_red)
    src = src.to(ref.device)
    return src, dst, ref[src], ab[src]


def check_plain(c, buf):
    """The C buffer of a plain-epilogue launch of case `c` (flat bf16, c.c_total + PAD_ROWS rows of c.ldc).  Exact operands: bit for bit;
    random ones: per element under the fp32 accumulation + bf16 rounding bound.  Sentinels everywhere else.  Returns error / bound."""
    what = name_of(c)
    src, dst, ref, ab = plain_expected(c)
    if c.exact:
        want = ref.float()
        assert torch.equal(want.double(), ref), "operands are not exact"
        check_image(buf, c.ldc, dst, c.N, c.nw, want.to(torch.bfloat16), what)
        return 0.0
    got = check_image(buf, c.ldc, dst, c.N, c.nw, None, what)
    if not len(dst):
        return 0.0
    return assert_elementwise(got, ref, ab, max(c.k_red, 1), c_out=1.0, c_acc=1.0, what=what)


def slab_expected(c, split):
    """[(fp64 values [M, N], |A| @ |B|)] of the live slabs of a slab launch, each over its own K range."""
    return [product64(c.mode, c.A, c.B, c.M, c.N, k0, k1) for k0, k1 in slab_slices(c.k_red, split)]


def check_slabs(c, buf, split):
    """The slab buffer of an EPI_SLAB_F32 launch (flat fp32, `split` slabs of [M][ldc] + PAD_ROWS rows): every live slab against its own K
    range (exact: bit for bit; random: per element, c_out = 0), slabs >= live and the pad rows still sentinels.  Returns error / bound."""
    what = name_of(c, split)
    exp = slab_expected(c, split)
    live = len(exp)
    rows = torch.arange(live * c.M)
    if c.exact:
        want = torch.cat([r.float() for r, _ in exp]) if live else torch.zeros(0, c.N)
        if live:
            assert torch.equal(want.double(), torch.cat([r for r, _ in exp])), "operands are not exact"
        check_image(buf, c.ldc, rows, c.N, c.nw, want, what)
        return 0.0
    got = check_image(buf, c.ldc, rows, c.N, c.nw, None, what)
    worst = 0.0
    ks = slab_slices(c.k_red, split)
    for s, (r, ab) in enumerate(exp):
        worst = max(worst, assert_elementwise(got[s * c.M:(s + 1) * c.M], r, ab, ks[s][1] - ks[s][0], c_out=0.0, c_acc=1.0,
                                              what=f"{what} slab {s}"))
    return worst


def check_reduced(c, dst, split, n_rows=None):
    """bf16 [M][N] (flat, + PAD_ROWS rows) left by the reduce over the slabs of case `c`: bf16_rne(exact) bit for bit, or per element with
    c_acc = 1 + live for random operands.  K = 0 reduces cleared slabs: zeros."""
    what = name_of(c, split) + " reduced"
    ref, ab = product64(c.mode, c.A, c.B, c.M, c.N, 0, c.k_red)
    live = len(slab_slices(c.k_red, split))
    rows = torch.arange(c.M)
    if c.exact:
        check_image(dst, c.N, rows, c.N, c.N, ref.float().to(torch.bfloat16), what)
        return 0.0
    got = check_image(dst, c.N, rows, c.N, c.N, None, what)
    return assert_elementwise(got, ref, ab, max(c.k_red, 1), c_out=1.0, c_acc=1.0 + live, what=what)


# ------------------------------------------------------------------------------------------ what a kernel leaves, right or wrong
FAULTS_M = ("count + 1", "count - 1", "a row in [count, cap) included", "c_rows ignored")
FAULTS_K = ("count + 1", "count - 1", "a row in [count, cap) included")
FAULTS_SLAB = ("one slice dropped", "a trailing empty slab summed")


def _round_out(v64, fp32):
    return v64.float() if fp32 else v64.float().to(torch.bfloat16)


def model_plain(c, fault=None):
    """The C buffer a plain-epilogue kernel leaves on case `c`: the rules above, or one of them broken."""
    buf = out_buf(c.c_total, c.ldc, device=c.A.device)
    img = buf.view(-1, c.ldc)
    count = c.count + (1 if fault == "count + 1" else -1 if fault == "count - 1" else 0)
    m_count = count if c.dyn == "m" else None
    k_red = min(c.K, count) if c.dyn == "k" else c.K
    c_rows = None if fault == "c_rows ignored" else c.c_rows
    src, dst = stored_rows(c.M, m_count, c_rows)
    rows = int(src.max()) + 1 if len(src) else 0
    ref, _ = product64(c.mode, c.A, c.B, rows, c.N, 0, max(k_red, 0))
    if fault == "a row in [count, cap) included":
        extra = min(c.cap - 1, c.count + 2)
        if c.dyn == "k":
            ref = ref + product64(c.mode, c.A, c.B, rows, c.N, extra, extra + 1)[0]
        else:
            one = product64(c.mode, c.A[extra:extra + 1], c.B, 1, c.N, 0, c.K)[0]
            img[extra if c.c_rows is None else max(int(c.c_rows[extra]), 0), :c.N] = _round_out(one, False)[0]
    if len(dst):
        img[dst.to(buf.device), :c.N] = _round_out(ref[src.to(ref.device)], False)
    return buf


def model_slabs(c, split, fault=None, clear=False):
    """The slab buffer a slab kernel leaves (sentinels, or zeros with `clear`, where it writes nothing)."""
    buf = out_buf(split * c.M, c.ldc, fp32=True, device=c.A.device)
    if clear:
        buf.view(-1, c.ldc)[:split * c.M] = 0
    exp = slab_expected(c, split)
    for s, (r, _) in enumerate(exp):
        if fault == "one slice dropped" and s == len(exp) - 1:
            continue
        buf.view(-1, c.ldc)[s * c.M:(s + 1) * c.M, :c.N] = r.float()
    return buf


def model_reduced(c, slab_buf, split, nslab):
    """The bf16 destination slab_reduce leaves from `nslab` slabs of `slab_buf`."""
    n = c.M * c.ldc
    dst = out_buf(c.M, c.N, device=c.A.device)
    dst[:n] = reduce_ref(slab_buf[:split * n].view(split, n), nslab, n)
    return dst


def brute_force(mode, A, B, M, N, K, m_count=None, k_count=None, c_rows=None, split=None):
    """The rules as loops over (slice, m, n, k) in Python floats (exact for the exact operands).  Returns {(slab, dest row, col): value}:
    one entry per stored element."""
    a = (lambda m, k: float(A[k, m])) if mode == TN else (lambda m, k: float(A[m, k]))
    b = (lambda k, n: float(B[n, k])) if mode == NT else (lambda k, n: float(B[k, n]))
    rows = M if m_count is None else min(M, m_count)
    kr = K if k_count is None else min(K, k_count)
    out = {}
    ktiles = -(-kr // 64)
    if split is None:
        ranges = [(0, kr)]
    else:
        per = -(-ktiles // split) if ktiles else 0
        ranges = [(64 * s * per, min(kr, 64 * (s + 1) * per)) for s in range(split)]
        ranges = [r for r in ranges if r[0] < r[1]]
    for s, (k0, k1) in enumerate(ranges):
        for m in range(rows):
            r = m if c_rows is None else int(c_rows[m])
            if r < 0:
                continue
            for n in range(N):
                acc = 0.0
                for k in range(k0, k1):
                    acc += a(m, k) * b(k, n)
                out[(s, r, n)] = acc
    return out


# ------------------------------------------------------------------------------------------ grouped slab launches (shed weight gradients)
GROUP_T = (256, 200, 3072)          # 3072: the first T at which the d % 192 != 0 rule splits by three
GROUP_SPLITS = (1, 3)               # next to the engine's own choice


def make_group(d, T, with_qkv, exact=True, seed=0, device="cpu"):
    """The shed weight-gradient problems (TN, K = T): q|k|v [3d, d] at offset 0 and o [d, d] at 3 d^2 of a 4 d^2 slab, or o alone in a d^2
    slab.  Returns (cases, offsets, slab_stride)."""
    def one(M, s):
        if exact:
            A, B, _ = exact_operands(M, d, T, s, mode=TN, device=device)
        else:
            g = torch.Generator(device=device).manual_seed(s)
            A = torch.randn(T, M, generator=g, device=device).to(torch.bfloat16)
            B = torch.randn(T, d, generator=g, device=device).to(torch.bfloat16)
        return Case(launch=f"wgrad[{M}x{d}]", mode=TN, epi=EPI_SLAB, M=M, N=d, K=T, lda=M, ldb=d, ldc=d, c_total=M, dyn=None, cap=T, count=T,
                    k_pad_zero=0, A=A, B=B, c_rows=None, exact=exact, d=d, V=0, T=T)
    if with_qkv:
        return [one(3 * d, seed), one(d, seed + 1)], [0, 3 * d * d], 4 * d * d
    return [one(d, seed + 1)], [0], d * d


def group_expected(cases, offsets, slab_stride, split):
    """fp64 image [live][slab_stride] of a grouped slab launch and its |A| @ |B| image; the problems tile the slab."""
    live = len(slab_slices(cases[0].K, split))
    dev = cases[0].A.device
    ref = torch.zeros(live, slab_stride, dtype=torch.float64, device=dev)
    ab = torch.zeros_like(ref)
    covered = torch.zeros(slab_stride, dtype=torch.bool, device=dev)
    for c, off in zip(cases, offsets):
        for s, (r, a) in enumerate(slab_expected(c, split)):
            ref[s, off:off + c.M * c.N] = r.reshape(-1)
            ab[s, off:off + c.M * c.N] = a.reshape(-1)
        covered[off:off + c.M * c.N] = True
    return ref, ab, covered


def check_group(cases, offsets, slab_stride, split, buf, what):
    """Flat fp32 buffer of `split` shared slabs + PAD_ROWS * 64 elements: every problem's live slabs at its own offset, nothing between or
    behind them.  Returns (error / bound, live)."""
    ref, ab, covered = group_expected(cases, offsets, slab_stride, split)
    live = ref.shape[0]
    img = bits(buf)
    body = img[:split * slab_stride].view(split, slab_stride)
    stray = (body[:live][:, ~covered] != SENT32).sum() + (body[live:] != SENT32).sum() + (img[split * slab_stride:] != SENT32).sum()
    assert int(stray) == 0, f"{what}: {int(stray)} elements written between or behind the problems' live slabs"
    got = buf[:live * slab_stride].view(live, slab_stride)
    if cases[0].exact:
        want = ref.float()
        assert torch.equal(want.double(), ref), "operands are not exact"
        bad = bits(got) != bits(want)
        if bool(bad.any()):
            ij = bad.nonzero()
            raise AssertionError(f"{what}: {int(bad.sum())} slab elements differ from the exact result; first (slab, offset) {ij[:4].tolist()}")
        return 0.0, live
    ks = slab_slices(cases[0].K, split)
    worst = 0.0
    for s in range(live):
        worst = max(worst, assert_elementwise(got[s:s + 1, covered], ref[s:s + 1, covered], ab[s:s + 1, covered], ks[s][1] - ks[s][0],
                                              c_out=0.0, c_acc=1.0, what=f"{what} slab {s}"))
    return worst, live


def check_group_reduced(cases, offsets, slab_stride, split, dst, what):
    """bf16 [slab_stride] (+ PAD_ROWS * 64 sentinels) left by the reduce of the live slabs: the contiguous q|k|v|o block."""
    ref, ab, covered = group_expected(cases, offsets, slab_stride, 1)
    live = len(slab_slices(cases[0].K, split))
    assert bool((bits(dst)[slab_stride:] == SENT16).all()), f"{what}: the reduce wrote behind its n elements"
    got = dst[:slab_stride].view(1, -1)
    if cases[0].exact:
        bad = bits(got) != bits(ref.float().to(torch.bfloat16))
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} reduced elements differ from bf16_rne(exact); first {bad.nonzero()[:4].tolist()}"
        return 0.0
    return assert_elementwise(got[:, covered], ref[:, covered], ab[:, covered], cases[0].K, c_out=1.0, c_acc=1.0 + live, what=what)


def model_group(cases, offsets, slab_stride, split, fault=None):
    """The shared slab buffer a grouped slab kernel leaves; fault "second problem at offset 0" = slab_stride / C pointers mixed up."""
    buf = out_buf(split * slab_stride // 64, 64, fp32=True, device=cases[0].A.device)
    for i, (c, off) in enumerate(zip(cases, offsets)):
        stride = slab_stride if fault != "own stride" else c.M * c.N
        for s, (r, _) in enumerate(slab_expected(c, split)):
            if fault == "one slice dropped" and i == len(cases) - 1 and s == 0:
                continue
            buf[s * stride + off:s * stride + off + c.M * c.N] = r.float().reshape(-1)
    return buf


# ------------------------------------------------------------------------------------------ slab_reduce alone
REDUCE_NSLAB = (1, 2, 3, 4, 5)
REDUCE_N = (4, 1020, 256 * 1024 + 4)      # one thread, a partial block, several grid strides


def reduce_inputs(nslab, n, seed=0, device="cpu"):
    """fp32 slabs [nslab][stride] (stride = n + 12: the gap holds NaN, it is never read) of mixed magnitudes, so that the order of the
    sum and the single rounding show in the bits, and a non-zero fp32 accumulator."""
    g = torch.Generator(device=device).manual_seed(seed + 7 * nslab + n)
    stride = n + 12
    s = torch.randn(nslab, stride, generator=g, device=device) * torch.exp2(torch.randint(-6, 7, (nslab, stride), generator=g, device=device).float())
    s[:, n:] = float("nan")
    acc = torch.randn(n, generator=g, device=device) * 3
    return s.contiguous(), stride, acc
