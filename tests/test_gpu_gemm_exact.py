"""GEMM kernels bit for bit, in every element: exact operands (tests/_util.py: exact_operands) make fp32 accumulation exact in any
summation order, so every tile shape, K split, stream-K partial and grouped launch the launcher (csrc/gemm.hip launch_t / launch_mode)
can pick must return bf16_rne(fp64 product) exactly - under every launch menu the process can select (menu keys 1, 2, 3, 15: csrc/menu.h).
Random-normal operands are held element-wise to the fp32 accumulation + bf16 rounding bound (assert_elementwise).  Output buffers are
surrounded by sentinels (columns in [N, ldc), rows past M)."""
import ctypes as C
import importlib

import pytest
import torch

from _util import assert_elementwise, exact_operands, gemm_expected, gemm_ref64, record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
eng = importlib.import_module("graph-gpt_amd.engine")

NT, NN, TN = L.GEMM_NT, L.GEMM_NN, L.GEMM_TN
EPI_NONE, EPI_RES, EPI_ATOMIC, EPI_SLAB = L.EPI_NONE, L.EPI_RESIDUAL, L.EPI_ATOMIC_F32, L.EPI_SLAB_F32
SENT16 = 0x7FC1                      # bf16 NaN payload no kernel writes
SENT32 = 0x7FC01234                  # fp32 NaN payload
PAD_ROWS = 64
VAR, HEADROOM, RESERVE = L.KEY_GEMM_VARIANT, L.KEY_GEMM_LDS_HEADROOM, L.KEY_GEMM_CU_RESERVE

# Launch menus (key -> value) whose kernel selection differs from the default somewhere in the cases below: the KEY_GEMM_VARIANT bits
# (csrc/menu.h kGemm*), KEY_GEMM_LDS_HEADROOM 0 (the 4-slot rings) and 2 (no two-blocks-per-CU launch), KEY_GEMM_CU_RESERVE (CUs held
# back for a collective).
MENUS = [{}, {VAR: L.GEMM_NO_KSPLIT_ND}, {VAR: L.GEMM_NO_KSPLIT_WGRAD}, {VAR: L.GEMM_NO_192_ROWS}, {VAR: L.GEMM_KSPLIT_128_ONLY},
         {VAR: L.GEMM_ONE_BLOCK_PER_CU}, {VAR: L.GEMM_KSPLIT_DMA8}, {VAR: L.GEMM_AREA_RULE}, {VAR: L.GEMM_NO_KSPLIT_ND | L.GEMM_NO_192_ROWS},
         {HEADROOM: 0}, {HEADROOM: 2}, {RESERVE: 16}, {RESERVE: 32}, {RESERVE: 64}, {RESERVE: 16, HEADROOM: 2}, {RESERVE: 64, HEADROOM: 0},
         {RESERVE: 32, VAR: L.GEMM_KSPLIT_DMA8}]
D, FF = 768, 3072
ROWS = [1408, 2880, 5184, 5376, 5696, 6144, 8192, 12032, 41472]   # tools/rows_sweep.py / seq_sweep.py batches, the headline, ogbl-ppa rows


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ST():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def name(keys):
    return ",".join(f"k{k}={v}" for k, v in sorted(keys.items())) or "default"


def rnd(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, generator=g, device="cuda").to(torch.bfloat16)


def layout(mode, M, N, K):
    """(A shape, B shape, lda, ldb) of the dense operands of `mode`."""
    if mode == NT:
        return (M, K), (N, K), K, K
    if mode == NN:
        return (M, K), (K, N), K, N
    return (K, M), (K, N), M, N


def out_buf(M, ldc, fp32=False, slabs=1):
    """Output buffer full of sentinels: slabs x [M][ldc] (+ PAD_ROWS rows behind the last slab)."""
    n = slabs * M * ldc + PAD_ROWS * ldc
    if fp32:
        return torch.full((n,), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((n,), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def assert_sentinels(buf, M, ldc, Nw, what, slabs=1, untouched_slabs=()):
    """Nothing written at columns [Nw, ldc) of any row, behind the last row, or in the slabs listed."""
    v = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int16)
    s = SENT32 if buf.dtype == torch.float32 else SENT16
    body = v[:slabs * M * ldc].view(slabs, M, ldc)
    assert bool((v[slabs * M * ldc:] == s).all()), f"{what}: wrote rows past M = {M}"
    if Nw < ldc:
        assert bool((body[:, :, Nw:] == s).all()), f"{what}: wrote columns [{Nw}, {ldc})"
    for i in untouched_slabs:
        assert bool((body[i] == s).all()), f"{what}: slab {i} (a slice past the end of K) was written"


def run_gemm(lib, mode, epi, A, B, R, M, N, K, ldc, split_k=1, ws=None):
    """One launch through gget_op_gemm (or _streamk with a workspace) into a fresh sentinel buffer; returns the buffer."""
    _, _, lda, ldb = layout(mode, M, N, K)
    fp32 = epi in (EPI_ATOMIC, EPI_SLAB)
    slabs = split_k if epi == EPI_SLAB else 1
    buf = out_buf(M, ldc, fp32, slabs)
    if epi == EPI_ATOMIC:
        buf[:M * ldc].view(M, ldc)[:, :N] = 0
    if ws is not None:
        L.check(lib.gget_op_gemm_streamk(mode, epi, P(A), P(B), P(buf), P(R), M, N, K, lda, ldb, ldc, P(ws), ST()))
    else:
        L.check(lib.gget_op_gemm(mode, epi, P(A), P(B), P(buf), P(R), M, N, K, lda, ldb, ldc, split_k, ST()))
    torch.cuda.synchronize()
    return buf


def check_single(lib, mode, epi, M, N, K, ldc=None, split_k=1, menus=MENUS, seed=0, case=""):
    """Exact operands under every menu (bit-exact, sentinels), then random-normal operands under the default menu (element-wise)."""
    ldc = ldc or (N + 7) // 8 * 8
    nw = (N + 3) // 4 * 4                      # NT with N % 4 != 0 writes up to the next multiple of 4 (gemm.hip: odd widths)
    res = epi == EPI_RES
    A, B, R = exact_operands(M, N, K, seed, mode=mode, residual=res, device="cuda")
    want16, want32 = gemm_expected(mode, A, B, R)
    slabs = split_k if epi == EPI_SLAB else 1
    ktiles = (K + 63) // 64
    per = (ktiles + split_k - 1) // split_k
    live = (ktiles + per - 1) // per          # slices that own K-tiles (gemm_kernel: 64-aligned slices of `per` tiles)
    for keys in menus:
        what = f"{case} mode {mode} epi {epi} {M}x{N}x{K} ldc {ldc} split {split_k} [{name(keys)}]"
        with L.debug_menu(keys):
            buf = run_gemm(lib, mode, epi, A, B, R, M, N, K, ldc, split_k)
        assert_sentinels(buf, M, ldc, nw, what, slabs, range(live, slabs) if epi == EPI_SLAB else ())
        body = buf[:slabs * M * ldc].view(slabs, M, ldc)[:, :, :N]
        if epi == EPI_SLAB:
            got = body[:live].double().sum(0)
            assert torch.equal(got, want32.double()), f"{what}: slab sum not exact ({int((got != want32.double()).sum())} elements)"
        elif epi == EPI_ATOMIC:
            assert torch.equal(body[0], want32), f"{what}: fp32 result not exact ({int((body[0] != want32).sum())} elements)"
        else:
            bad = (body[0].view(torch.int16) != want16.view(torch.int16))
            if bool(bad.any()):
                ij = bad.nonzero()
                raise AssertionError(f"{what}: {int(bad.sum())} elements differ from bf16_rne(exact); first (row, col) "
                                     f"{ij[:4].tolist()}, 64x64 tiles {sorted({(r // 64, c // 64) for r, c in ij.tolist()})[:6]}")
    # random-normal operands: the error bound of fp32 accumulation + one bf16 rounding, per element
    sa, sb, _, _ = layout(mode, M, N, K)
    A, B = rnd(*sa, seed=seed + 1), rnd(*sb, seed=seed + 2)
    R = rnd(M, N, seed=seed + 3) if res else None
    buf = run_gemm(lib, mode, epi, A, B, R, M, N, K, ldc, split_k)
    ref, ab = gemm_ref64(mode, A, B, R)
    body = buf[:slabs * M * ldc].view(slabs, M, ldc)[:, :, :N]
    got = body[:live].double().sum(0) if epi == EPI_SLAB else body[0]
    fp32 = epi in (EPI_ATOMIC, EPI_SLAB)
    r = assert_elementwise(got, ref, ab, K, c_out=0.0 if fp32 else 1.0, c_acc=1.0 + live, what=f"{case} random {mode}/{epi} {M}x{N}x{K}")
    record_error(f"gemm_elementwise/{case}", f"{mode}_{epi}_{M}x{N}x{K}_s{split_k}", r, 1.0)
    return want16


# ------------------------------------------------------------------------------------------ the shapes of tests/test_gpu_ops.py
OPS_MODES = [(128, 128, 64), (256, 384, 192), (200, 136, 72), (1000, 756, 128), (64, 2304, 768), (333, 768, 3072), (4096, 2304, 128),
             (2048, 768, 512), (4096, 4096, 192), (8192, 2304, 64)]
OPS_128x192 = [(8192, 768, 768), (1000, 768, 256), (40000, 384, 128), (41472, 768, 768), (41413, 768, 2304), (33000, 1536, 320)]
OPS_STREAMK = [(5696, 768, 3072, True), (5696, 768, 2304, False), (5632, 768, 6144, False), (5700, 768, 3072, True),
               (41000, 768, 3072, False), (3000, 768, 2048, True), (9000, 768, 1536, False), (10900, 768, 3072, True),
               (12000, 768, 2304, False), (1000, 768, 1536, True), (8192, 768, 3072, True), (6100, 384, 1536, False)]


@pytest.mark.parametrize("mode", [NT, NN, TN])
@pytest.mark.parametrize("M,N,K", OPS_MODES)
def test_exact_gemm_modes(lib, mode, M, N, K):
    if (mode == NN and N % 8) or (mode == TN and (N % 8 or M % 8)):
        pytest.skip("operand layout needs M / N % 8 == 0 (as in test_gemm_modes)")
    check_single(lib, mode, EPI_NONE, M, N, K, case="modes")


def test_exact_gemm_residual_atomic_slab(lib):
    M, N, K = 300, 256, 320
    check_single(lib, NT, EPI_RES, M, N, K, case="epilogues")
    for split in (1, 3):
        check_single(lib, NT, EPI_ATOMIC, M, N, K, split_k=split, menus=[{}], case="epilogues")
    for split in (2, 4):                               # K = 320: 5 K-tiles -> split 4 leaves slice 3 empty
        check_single(lib, NT, EPI_SLAB, M, N, K, split_k=split, menus=[{}], case="epilogues")
    for M, N, K, split in ((768, 768, 5696, 8), (2304, 768, 5184, 6), (1000, 760, 700, 5)):   # the weight-gradient slab shapes (TN, K = T)
        check_single(lib, TN, EPI_SLAB, M, N, K, split_k=split, menus=[{}, {RESERVE: 32}], case="wgrad_slab")
        check_single(lib, TN, EPI_ATOMIC, M, N, K, split_k=split, menus=[{}], case="wgrad_atomic")


@pytest.mark.parametrize("mode", [NT, NN])
@pytest.mark.parametrize("M,N,K", OPS_128x192)
def test_exact_gemm_tile_128x192(lib, mode, M, N, K):
    check_single(lib, mode, EPI_RES, M, N, K, case="tile_128x192")


@pytest.mark.parametrize("M,N,K", [(1536, 768, 2048), (768, 3072, 1024), (768, 768, 8192), (6144, 768, 512)])
def test_exact_gemm_tn_tile_192x192(lib, M, N, K):
    check_single(lib, TN, EPI_NONE, M, N, K, case="tn_192")


@pytest.mark.parametrize("M,N,K", [(300, 211, 128), (5000, 41245 // 8 + 1, 64)])
def test_exact_gemm_nt_odd_width(lib, M, N, K):
    check_single(lib, NT, EPI_NONE, M, N, K, ldc=(N + 63) // 64 * 64, case="odd_width")


@pytest.mark.parametrize("mode", [NT, NN])
@pytest.mark.parametrize("M,N,K,res", OPS_STREAMK)
def test_exact_gemm_stream_k(lib, mode, M, N, K, res):
    """The split of the last round (key 3) moves fp32 partial tiles between workgroups: with exact operands the result must be the
    plain launch's and the expected bits exactly, launch after launch on the same workspace, under the menus that change its plan."""
    epi = EPI_RES if res else EPI_NONE
    want16 = check_single(lib, mode, epi, M, N, K, menus=[{}, {RESERVE: 32}], case="stream_k")
    A, B, R = exact_operands(M, N, K, 0, mode=mode, residual=res, device="cuda")
    ws = torch.zeros(int(lib.gget_op_gemm_streamk_bytes()), dtype=torch.uint8, device="cuda")
    SPLIT, NO_KS = L.KEY_GEMM_SPLIT_LAST, L.GEMM_NO_KSPLIT_ND
    for keys in ({SPLIT: 1, VAR: NO_KS}, {SPLIT: 1, VAR: NO_KS, HEADROOM: 0}, {SPLIT: 1, VAR: NO_KS, RESERVE: 32}, {SPLIT: 1}):
        what = f"stream-K mode {mode} {M}x{N}x{K} res {res} [{name(keys)}]"
        with L.debug_menu(keys):
            for it in range(2):
                buf = run_gemm(lib, mode, epi, A, B, R, M, N, K, N, ws=ws)
                assert_sentinels(buf, M, N, N, what)
                assert torch.equal(buf[:M * N].view(M, N).view(torch.int16), want16.view(torch.int16)), f"{what} launch {it}: not bit-exact"
        err_flag = int(ws[512 * 4: 512 * 4 + 4].view(torch.int32)[0])
        assert err_flag == 0, f"{what}: a stream-K owner gave up waiting for its contributor"


# ------------------------------------------------------------------------------------------ the headline decoder layer
def _rope64(x, pos, cos, sin, ncols):
    """fp64 RoPE (hf apply_rotary_pos_emb) of columns [0, ncols) of x [T, *] with the engine's tables; pos [T]."""
    T = x.shape[0]
    h = x[:, :ncols].reshape(T, ncols // 64, 64)
    c = cos.double()[pos][:, None, :].repeat(1, 1, 2)
    s = sin.double()[pos][:, None, :].repeat(1, 1, 2)
    rot = torch.cat((-h[..., 32:], h[..., :32]), -1)
    return (h * c + rot * s).reshape(T, ncols)


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / 2.0 ** 0.5))


def _gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / 2.0 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2.0 * torch.pi) ** 0.5


def layer_forward_fused(lib, T, d, ff, menus, seed):
    """q|k|v + RoPE and gate|up + GEGLU as the engine issues them: the GEMM part exact, the epilogue element-wise."""
    cos, sin = eng.rope_tables(1024, 64, 10000.0)
    cos, sin = cos.cuda(), sin.cuda()
    g = torch.Generator(device="cuda").manual_seed(seed)
    pos = torch.randint(0, 1024, (T,), generator=g, device="cuda", dtype=torch.int64)
    x, w, _ = exact_operands(T, 3 * d, d, seed, mode=NT, device="cuda")
    qkv64 = gemm_expected(NT, x, w)[1].double()
    want_v = qkv64[:, 2 * d:].float().to(torch.bfloat16)
    ref_qk = _rope64(qkv64, pos, cos, sin, 2 * d)
    first = None
    for keys in menus:
        what = f"qkv_rope T {T} [{name(keys)}]"
        qkv = out_buf(T, 3 * d)
        with L.debug_menu(keys):
            L.check(lib.gget_op_qkv_rope(P(x), P(w), P(qkv), P(cos), P(sin), P(pos), T, 32, d, ST()))
            torch.cuda.synchronize()
        assert_sentinels(qkv, T, 3 * d, 3 * d, what)
        q = qkv[:T * 3 * d].view(T, 3 * d)
        assert torch.equal(q[:, 2 * d:].view(torch.int16), want_v.view(torch.int16)), f"{what}: v columns not exact"
        r = assert_elementwise(q[:, :2 * d], ref_qk, qkv64[:, :2 * d].abs(), 1, c_out=1.0, atol=2.0 ** -20 * qkv64[:, :2 * d].abs().max(), what=what)
        record_error("gemm_layer/qkv_rope", f"T{T}_{name(keys)}", r, 1.0)
        first = q.clone() if first is None else first
        assert torch.equal(q, first), f"{what}: differs from the default menu's bits"
    # gate|up + GEGLU (fused) and dh + GEGLU' (fused)
    xn, wgu, _ = exact_operands(T, 2 * ff, d, seed + 1, mode=NT, device="cuda")
    gu16 = gemm_expected(NT, xn, wgu)[0]
    gate, up = gu16[:, :ff].double(), gu16[:, ff:].double()
    h_ref = _gelu64(gate) * up
    dy, wdn, _ = exact_operands(T, ff, d, seed + 2, mode=NN, device="cuda")
    dh = gemm_expected(NN, dy, wdn)[0].double()               # the fused launch rounds dh to bf16 as the un-fused GEMM does
    dg_ref, du_ref = dh * up * _gelu_grad64(gate), dh * _gelu64(gate)
    tiny = 2.0 ** -20
    for keys in menus:
        what = f"gateup_geglu T {T} [{name(keys)}]"
        gu, h = out_buf(T, 2 * ff), out_buf(T, ff)
        dgu = out_buf(T, 2 * ff)
        with L.debug_menu(keys):
            L.check(lib.gget_op_gateup_geglu(P(xn), P(wgu), P(gu), P(h), T, d, ff, ST()))
            L.check(lib.gget_op_down_dgrad_geglu(P(dy), P(wdn), P(gu16), P(dgu), None, T, d, ff, ST()))
            torch.cuda.synchronize()
        for b, wdt in ((gu, 2 * ff), (h, ff), (dgu, 2 * ff)):
            assert_sentinels(b, T, wdt, wdt, what)
        assert torch.equal(gu[:T * 2 * ff].view(T, 2 * ff).view(torch.int16), gu16.view(torch.int16)), f"{what}: gate|up not exact"
        hh = h[:T * ff].view(T, ff)
        r = assert_elementwise(hh, h_ref, gate.abs() * up.abs(), 1, c_out=2.0, atol=tiny * (1 + gate.abs()) * up.abs(), what=what + " h")   # (2 roundings)
        record_error("gemm_layer/geglu_h", f"T{T}_{name(keys)}", r, 1.0)
        dd = dgu[:T * 2 * ff].view(T, 2 * ff)
        r1 = assert_elementwise(dd[:, :ff], dg_ref, dh.abs() * up.abs() * (1 + gate.abs()), 1, c_out=1.25,
                                atol=tiny * dh.abs() * up.abs() * (1 + gate.abs()), what=what + " dgate")
        r2 = assert_elementwise(dd[:, ff:], du_ref, dh.abs() * gate.abs(), 1, c_out=1.25, atol=tiny * dh.abs() * (1 + gate.abs()),
                                what=what + " dup")
        record_error("gemm_layer/geglu_bwd", f"T{T}_{name(keys)}", max(r1, r2), 1.0)


def layer_plain(lib, T, d, ff, menus, seed):
    """The plain GEMMs of one layer, with the engine's modes, epilogues and leading dimensions (csrc/engine.hip)."""
    shapes = [(NT, EPI_RES, T, d, d), (NT, EPI_RES, T, d, ff),            # o + residual, down + residual
              (NN, EPI_NONE, T, d, 2 * ff), (NN, EPI_NONE, T, d, 3 * d), (NN, EPI_NONE, T, d, d)]   # dxn2, dxn1, dattn
    for i, (mode, epi, M, N, K) in enumerate(shapes):
        check_single(lib, mode, epi, M, N, K, menus=menus, seed=seed + 10 * i, case=f"layer_T{T}")


def grouped_problems(T, d, ff, which, seed, exact=True):
    """The engine's weight-gradient problems (TN, K = T): 0 gate|up [2ff, d], 1 down [d, ff], 2 q|k|v [3d, d], 3 o [d, d]."""
    dims = {0: (2 * ff, d), 1: (d, ff), 2: (3 * d, d), 3: (d, d)}
    out = []
    for j, q in enumerate(which):
        M, N = dims[q] if isinstance(q, int) else q[:2]
        K = T if isinstance(q, int) else q[2]
        if exact:
            A, B, _ = exact_operands(M, N, K, seed + j, mode=TN, device="cuda")
        else:
            A, B = rnd(K, M, seed=seed + 2 * j), rnd(K, N, seed=seed + 2 * j + 1)
        out.append((A, B, M, N, K))
    return out


def check_grouped(lib, probs, menus, what0):
    wants = [gemm_expected(TN, A, B)[0] for A, B, M, N, K in probs]
    for keys in menus:
        what = f"{what0} {[(M, N, K) for _, _, M, N, K in probs]} [{name(keys)}]"
        bufs = [out_buf(M, N) for _, _, M, N, K in probs]
        with L.debug_menu(keys):
            L.check(L.gemm_grouped(lib, TN, [(A, B, c, M, N, K, M, N, N) for (A, B, M, N, K), c in zip(probs, bufs)], ST()))
            torch.cuda.synchronize()
        for j, ((A, B, M, N, K), c, want) in enumerate(zip(probs, bufs, wants)):
            assert_sentinels(c, M, N, N, f"{what} problem {j}")
            bad = c[:M * N].view(M, N).view(torch.int16) != want.view(torch.int16)
            if bool(bad.any()):
                ij = bad.nonzero()
                raise AssertionError(f"{what} problem {j}: {int(bad.sum())} elements differ from bf16_rne(exact); 192x192 tiles "
                                     f"{sorted({(r // 192, c_ // 192) for r, c_ in ij.tolist()})[:6]}")


def check_grouped_random(lib, probs, what):
    bufs = [out_buf(M, N) for _, _, M, N, K in probs]
    L.check(L.gemm_grouped(lib, TN, [(A, B, c, M, N, K, M, N, N) for (A, B, M, N, K), c in zip(probs, bufs)], ST()))
    torch.cuda.synchronize()
    worst = 0.0
    for (A, B, M, N, K), c in zip(probs, bufs):
        ref, ab = gemm_ref64(TN, A, B)
        worst = max(worst, assert_elementwise(c[:M * N].view(M, N), ref, ab, K, tile=(192, 192), what=f"{what} random {M}x{N}x{K}"))
    record_error("gemm_grouped/random", what, worst, 1.0)


LAYER_MENUS = [{}, {1: 1}, {1: 4}, {1: 16}, {1: 32}, {1: 128}, {1: 512}, {2: 0}, {2: 2}, {15: 16, 2: 2}, {15: 64}]
GROUPED_MENUS = [{}, {1: 2}, {1: 64}, {1: 128}, {2: 0}, {15: 16}, {15: 32}, {15: 64}]


@pytest.mark.parametrize("T", ROWS)
def test_exact_layer_launch_table(lib, T):
    """Every GEMM one d = 768 / ff = 3072 decoder layer issues at T rows; each T reaches some branch of the plan rule.  The headline
    (5 696) and its neighbours run under the full menu list, the others under the menus that change a layer GEMM's kernel."""
    menus = MENUS if T in (2880, 5696, 8192) else LAYER_MENUS
    layer_forward_fused(lib, T, D, FF, menus if T != 41472 else [{}, {1: 4}, {2: 0}, {15: 64}], seed=T)
    layer_plain(lib, T, D, FF, menus if T != 41472 else [{}, {1: 4}, {2: 0}, {15: 64}], seed=T + 1)
    probs = grouped_problems(T, D, FF, [0, 1, 2, 3], seed=T)
    check_grouped(lib, probs, GROUPED_MENUS, f"grouped4 T {T}")
    check_grouped_random(lib, grouped_problems(T, D, FF, [0, 1, 2, 3], seed=T, exact=False), f"grouped4_T{T}")


@pytest.mark.parametrize("T", [5696, 1408, 41472, 5700, 2900])   # the last two: K % 64 != 0 (the non-persistent gemm_kernel)
@pytest.mark.parametrize("which", [[0], [1, 3], [0, 1, 2], [3, 2, 1, 0], [2, 0]])
def test_exact_grouped_subsets(lib, T, which):
    """Groups of 1 - 4 of the engine's problems, in the engine's order and shuffled (tile_begin / tiles_n bookkeeping)."""
    probs = grouped_problems(T, D, FF, which, seed=7 * T)
    check_grouped(lib, probs, GROUPED_MENUS if T in (5696, 5700) else [{}, {1: 2}, {15: 32}], f"grouped T {T}")


@pytest.mark.parametrize("probs", [
    [(384, 576, 4096), (1152, 192, 1344), (192, 768, 640)],            # M, N and K differ per problem
    [(960, 384, 2048), (192, 192, 5696), (576, 1152, 320), (384, 768, 3008)],
    [(768, 192, 128), (192, 960, 8192)],
    [(200, 264, 1000), (1024, 96, 704), (64, 64, 64)],                  # no multiple of 192: the 256x128 / 128x128 tilings
])
def test_exact_grouped_mixed(lib, probs):
    ps = grouped_problems(0, D, FF, probs, seed=sum(p[2] for p in probs))
    check_grouped(lib, ps, GROUPED_MENUS, "grouped mixed")
    check_grouped_random(lib, grouped_problems(0, D, FF, probs, seed=5, exact=False), f"mixed_{len(probs)}")


@pytest.mark.parametrize("d,ff,T", [(512, 2048, 5696), (1024, 4096, 5696), (128, 512, 2880), (1024, 4096, 12032)])
def test_exact_grouped_other_widths(lib, d, ff, T):
    """Widths whose weight gradients are no 192x192 grid (the engine's two-problem gate|up + down group), and their layer GEMMs."""
    probs = grouped_problems(T, d, ff, [0, 1], seed=d + T)
    check_grouped(lib, probs, [{}, {1: 2}, {2: 0}, {15: 32}], f"grouped d {d}")
    layer_plain(lib, T, d, ff, [{}, {1: 4}, {15: 32}], seed=d)
    layer_forward_fused(lib, T, d, ff, [{}, {1: 4}, {2: 2}], seed=d)
