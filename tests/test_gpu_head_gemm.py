"""The GEMM launches whose shape is read from device memory (GemmProblem::m_dev, k_dev / k_pad_zero, c_rows: the SMTP head) and the split-K
slab launches with their reduce (the lm_head weight gradient, the q|k|v / o weight gradients shed from the grouped launch), through the
test-only entries gget_op_gemm_dyn / gget_op_gemm_grouped_slab / gget_op_slab_reduce / gget_op_slab_plan, against tests/_headgemm_ref.py.
Exact operands (tests/_util.py exact_operands) are held bit for bit, random-normal ones per element under the fp32 accumulation + output
rounding bound; every output starts as sentinels with pad rows behind it and pad columns in [N, ldc), so "not stored" is checked as well.
Operand rows at or beyond the device-side count hold NaN (zero / finite-and-huge inside the K-tile a k_pad_zero launch may read).
tests/test_headgemm_reference.py shows on the CPU that these checks reject a wrong count, row, slice or scatter."""
import ctypes as C
import importlib

import pytest
import torch

import _headgemm_ref as H
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
eng_mod = importlib.import_module("graph-gpt_amd.engine")

RESERVE, HEADROOM = L.KEY_GEMM_CU_RESERVE, L.KEY_GEMM_LDS_HEADROOM
GROUP_MENUS = [{}, {RESERVE: 32}, {RESERVE: 64}, {HEADROOM: 0}]


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ST():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def name(keys):
    return ",".join(f"k{k}={v}" for k, v in sorted(keys.items())) or "default"


def dev_int(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def launch(lib, c, buf, split=1):
    cnt = dev_int(c.count)
    L.check(lib.gget_op_gemm_dyn(c.mode, c.epi, P(c.A), P(c.B), P(buf), c.M, c.N, c.K, c.lda, c.ldb, c.ldc, P(cnt) if c.dyn == "m" else None,
                                 P(cnt) if c.dyn == "k" else None, c.k_pad_zero, split, P(c.c_rows), ST()))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the engine's six head launches
PLAIN = [(lc, d, T) for lc in H.LAUNCHES if lc != "lm_wgrad" for d in H.WIDTHS for T in H.T_CAPS]


@pytest.mark.parametrize("launch_name,d,T", PLAIN)
def test_head_launch_with_device_side_count(lib, launch_name, d, T):
    """n_token_proj / lm_head forward and input gradients (m_dev, with and without the c_rows scatter) and the n_token_proj weight gradient
    (k_dev, k_pad_zero 1 and 0: the persistent kernel at T % 64 == 0 with k_pad_zero, gemm_kernel otherwise), every count of counts_for."""
    vocabs = H.VOCABS if launch_name.startswith("lm_") else H.VOCABS[:1]
    kpzs = (1, 0) if launch_name == "ntp_wgrad" else (0,)
    for V in vocabs:
        cap = H.launch_shape(launch_name, d, V, T)[-1]
        worst = 0.0
        for count in H.counts_for(cap):
            for kpz in kpzs:
                for exact in (True, False):
                    c = H.make_case(launch_name, d, V, T, count, exact=exact, k_pad_zero=kpz, seed=count + 1000 * kpz, device="cuda")
                    buf = H.out_buf(c.c_total, c.ldc, device="cuda")
                    launch(lib, c, buf)
                    worst = max(worst, H.check_plain(c, buf))
        record_error(f"head_gemm/{launch_name}", f"d{d}_V{V}_T{T}", worst, 1.0)


@pytest.mark.parametrize("d", H.WIDTHS)
@pytest.mark.parametrize("T", H.T_CAPS)
@pytest.mark.parametrize("V", H.VOCABS)
def test_lm_head_wgrad_slabs(lib, d, T, V):
    """dW_lm = dlogits^T Hl with K = Lm on the device (TN, lda = Vp, M = V) into fp32 slabs, K slices as the engine picks them and 1, 2, 5:
    every live slab against its own K range, slabs >= live untouched; then the reduce over all `split` pre-cleared slabs."""
    cap = T * H.N_TOK
    plan = L.slab_plan(L.SLAB_PLAN_LM_HEAD, d, V, T)
    assert 1 <= plan <= 16
    worst = worst_red = 0.0
    for count in H.counts_for(cap):
        for split in sorted(set(H.LM_SPLITS) | {plan}):
            for exact in (True, False):
                c = H.make_case("lm_wgrad", d, V, T, count, exact=exact, seed=count, device="cuda")
                buf = H.out_buf(split * c.M, c.ldc, fp32=True, device="cuda")
                launch(lib, c, buf, split)
                worst = max(worst, H.check_slabs(c, buf, split))
                n = c.M * c.ldc
                buf[:split * n] = 0                              # the engine clears the slabs, then sums all of them
                launch(lib, c, buf, split)
                dst = H.out_buf(c.M, c.N, device="cuda")
                L.check(lib.gget_op_slab_reduce(P(buf), n, split, P(dst), n, 0, ST()))
                torch.cuda.synchronize()
                worst_red = max(worst_red, H.check_reduced(c, dst, split))
    record_error("head_gemm/lm_wgrad_slabs", f"d{d}_V{V}_T{T}", worst, 1.0)
    record_error("head_gemm/lm_wgrad_reduced", f"d{d}_V{V}_T{T}", worst_red, 1.0)


# ------------------------------------------------------------------------------------------ grouped slabs
@pytest.mark.parametrize("d", H.WIDTHS)
@pytest.mark.parametrize("T", H.GROUP_T)
@pytest.mark.parametrize("with_qkv", [True, False])
def test_grouped_slab_launch(lib, d, T, with_qkv):
    """q|k|v + o (C = wg, wg + 3 d^2, one shared slab_stride of 4 d^2) and o alone, as layer_backward sheds them, under the menus that
    change the plan; K slices from the engine's rule for this width and 1, 3.  Then the reduce of the live slabs into the contiguous block."""
    whichs = ([L.SLAB_PLAN_SHED_QKVO] if with_qkv else [L.SLAB_PLAN_SHED_O]) if d % 192 == 0 else ([L.SLAB_PLAN_QKVO] if with_qkv else [])
    worst = worst_red = 0.0
    for exact in (True, False):
        cases, offs, stride = H.make_group(d, T, with_qkv, exact=exact, seed=T + d, device="cuda")
        for keys in (GROUP_MENUS if exact else [{}]):
            with L.debug_menu(keys):
                splits = sorted(set(H.GROUP_SPLITS) | {L.slab_plan(w, d, 1, T) for w in whichs})
                for split in splits:
                    what = f"grouped slabs d{d} T{T} qkv{with_qkv} split{split} [{name(keys)}] {'exact' if exact else 'random'}"
                    buf = H.out_buf(split * stride // 64, 64, fp32=True, device="cuda")
                    probs = [(c.A, c.B, buf[off:], c.M, c.N, c.K, c.lda, c.ldb, c.ldc) for c, off in zip(cases, offs)]
                    L.check(L.gemm_grouped_slab(lib, H.TN, probs, stride, split, ST()))
                    torch.cuda.synchronize()
                    r, live = H.check_group(cases, offs, stride, split, buf, what)
                    dst = H.out_buf(stride // 64, 64, device="cuda")
                    L.check(lib.gget_op_slab_reduce(P(buf), stride, live, P(dst), stride, 0, ST()))
                    torch.cuda.synchronize()
                    worst, worst_red = max(worst, r), max(worst_red, H.check_group_reduced(cases, offs, stride, split, dst, what))
    if T == 3072 and d % 192 != 0 and with_qkv:
        assert L.slab_plan(L.SLAB_PLAN_QKVO, d, 1, T) == 3 and L.slab_plan(L.SLAB_PLAN_QKVO, d, 1, T - 1) == 1
    record_error("head_gemm/grouped_slabs", f"d{d}_T{T}_qkv{int(with_qkv)}", worst, 1.0)
    record_error("head_gemm/grouped_reduced", f"d{d}_T{T}_qkv{int(with_qkv)}", worst_red, 1.0)


# ------------------------------------------------------------------------------------------ slab_reduce alone
@pytest.mark.parametrize("n", H.REDUCE_N)
def test_slab_reduce(lib, n):
    """bf16 output = RNE(sequential fp32 sum) bit for bit; f32_out adds the sum onto a non-zero accumulator; nothing behind n."""
    for nslab in H.REDUCE_NSLAB:
        s, stride, acc = H.reduce_inputs(nslab, n, device="cuda")
        dst = torch.full((n + 64,), H.SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        L.check(lib.gget_op_slab_reduce(P(s), stride, nslab, P(dst), n, 0, ST()))
        acc_buf = torch.full((n + 64,), H.SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
        acc_buf[:n] = acc
        L.check(lib.gget_op_slab_reduce(P(s), stride, nslab, P(acc_buf), n, 1, ST()))
        torch.cuda.synchronize()
        what = f"slab_reduce nslab {nslab} n {n}"
        assert bool((H.bits(dst)[n:] == H.SENT16).all()) and bool((H.bits(acc_buf)[n:] == H.SENT32).all()), f"{what}: wrote behind n"
        bad = H.bits(dst[:n]) != H.bits(H.reduce_ref(s, nslab, n))
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} bf16 elements differ from RNE(sequential fp32 sum); first {bad.nonzero()[:4].tolist()}"
        bad = H.bits(acc_buf[:n]) != H.bits(H.reduce_ref(s, nslab, n, acc))
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} fp32 elements differ from accumulator + sum; first {bad.nonzero()[:4].tolist()}"
    record_error("head_gemm/slab_reduce", f"n{n}", 0.0, 1.0)


# ------------------------------------------------------------------------------------------ the engine: no stale head gradients
def _step(e, ids, att, lab):
    e.forward_pretrain(ids, att, lab)
    e.backward()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in e.grads().items()}


@pytest.mark.parametrize("B,S", [(2, 24), (8, 32)])
def test_engine_head_gradients_do_not_outlive_their_step(B, S):
    """T = 48 takes gemm_kernel for the n_token_proj weight gradient (K = T % 64 != 0), T = 256 the persistent kernel.  A step without a
    labelled cell after a labelled one leaves every gradient exactly zero; a short selection after a long one gives the lm_head and
    n_token_proj gradients of a fresh engine bit for bit (KEY_DETERMINISTIC: no fp32 atomics in the sums)."""
    from _util import spec_mod, weights_mod, synth, tb
    F, V = 13, 756
    spec = spec_mod.spec_from_size("tiny", vocab_size=V, stacked_feat=F, next_n_token=F)
    state = weights_mod.make_state_dict(spec, seed=5, std=0.05)
    b = tb(synth.make_pretrain_batch(B=B, S=S, F=F, V=V, seed=3))
    ids, att, lab = b["input_ids"], b["attention_mask"], b["labels"]
    none = torch.full_like(lab, -100)
    short = none.clone()
    short[0, :5] = lab[0, :5]
    assert int((short != -100).sum()) > 0 and int((lab != -100).sum()) > 4 * int((short != -100).sum())
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):
        e = eng_mod.Engine(spec, max_tokens=B * S, max_batch=B)
        e.load_state_dict(state)
        g = _step(e, ids, att, lab)
        assert float(g["n_token_proj.weight"].float().abs().max()) > 0 and float(g["lm_head.weight"].float().abs().max()) > 0
        g0 = _step(e, ids, att, none)
        assert e.head_counts() == (0, 0)
        stale = {k: int((v.float() != 0).sum()) for k, v in g0.items() if bool((v.float() != 0).any())}
        assert not stale, f"B {B} S {S}: gradients of a step without labels are not zero after a labelled step (non-zero elements: {stale})"
        _step(e, ids, att, lab)
        g_short = _step(e, ids, att, short)
        fresh = eng_mod.Engine(spec, max_tokens=B * S, max_batch=B)
        fresh.load_state_dict(state)
        g_fresh = _step(fresh, ids, att, short)
        for k in ("lm_head.weight", "n_token_proj.weight"):
            bad = H.bits(g_short[k]) != H.bits(g_fresh[k])
            assert not bool(bad.any()), f"B {B} S {S}: {k} after a longer selection differs from a fresh engine's in {int(bad.sum())} elements"
