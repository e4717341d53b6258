"""tests/_headgemm_ref.py on the CPU: the float64 statements agree with a brute-force loop over (slice, m, n, k); the checks pass on what the
rules leave for the very inputs tests/test_gpu_head_gemm.py runs; and one broken rule at a time - the count off by one in either direction,
a row in [count, cap) included, one slice dropped, a trailing empty slab summed, c_rows ignored - leaves bits that the checks reject.  No
wrong kernel is built or run anywhere: this is where the GPU test's teeth are shown."""
import pytest
import torch

import _headgemm_ref as H
from _util import exact_operands


# ------------------------------------------------------------------------------------------ the rules against loops
@pytest.mark.parametrize("mode", [H.NT, H.NN, H.TN])
def test_product_and_row_rules_match_brute_force(mode):
    M, N, K = 9, 8, 70
    A, B, _ = exact_operands(M, N, K, seed=mode, mode=mode)
    c_rows = torch.tensor([4, -1, 0, 7, 8, -3, 2, 1, 5], dtype=torch.int32)
    for m_count, k_count, cr in ((None, None, None), (5, None, None), (0, None, None), (9, None, c_rows), (6, None, c_rows), (None, 65, None),
                                 (None, 0, None), (None, 1, None), (12, 90, None)):
        want = H.brute_force(mode, A, B, M, N, K, m_count, k_count, cr)
        src, dst = H.stored_rows(M, m_count, cr)
        rows = int(src.max()) + 1 if len(src) else 0
        ref, ab = H.product64(mode, A, B, rows, N, 0, K if k_count is None else min(K, k_count))
        got = {(0, int(r), n): float(ref[int(s), n]) for s, r in zip(src, dst) for n in range(N)}
        assert got == want, (mode, m_count, k_count)
        assert bool((ab >= ref.abs()).all())


@pytest.mark.parametrize("K,split", [(70, 1), (70, 2), (320, 4), (576, 16), (600, 5), (1, 3), (64, 2), (65, 2), (0, 3), (200, 3)])
def test_slab_slices_match_brute_force(K, split):
    M, N = 3, 4
    A, B, _ = exact_operands(M, N, max(K, 1), seed=K, mode=H.TN)
    want = H.brute_force(H.TN, A, B, M, N, max(K, 1), k_count=K, split=split)
    ks = H.slab_slices(K, split)
    got = {}
    for s, (k0, k1) in enumerate(ks):
        ref, _ = H.product64(H.TN, A, B, M, N, k0, k1)
        got.update({(s, m, n): float(ref[m, n]) for m in range(M) for n in range(N)})
    assert got == want
    assert len(ks) <= split and all(a < b for a, b in ks) and (not ks or (ks[0][0] == 0 and ks[-1][1] == K))
    assert all(ks[i][1] == ks[i + 1][0] and ks[i][0] % 64 == 0 for i in range(len(ks) - 1))
    if (K, split) == (320, 4):
        assert len(ks) == 3, "5 K-tiles in 4 slices of 2: the last slab is empty"
    if (K, split) == (576, 16):
        assert len(ks) == 9


def test_reduce_ref_is_the_sequential_fp32_sum():
    s, stride, acc = H.reduce_inputs(4, 1020)
    want = [0.0] * 1020
    import numpy as np
    v = s.numpy()
    a = v[0, :1020].copy()
    for i in range(1, 4):
        a = (a + v[i, :1020]).astype(np.float32)
    assert torch.equal(H.reduce_ref(s, 4, 1020, acc), torch.from_numpy((a + acc.numpy()).astype(np.float32)))
    assert torch.equal(H.reduce_ref(s, 4, 1020), torch.from_numpy(a).to(torch.bfloat16))
    # the order and the single rounding show: another order, or a bf16 rounding per slab, gives other bits somewhere
    other = ((s[3, :1020] + s[2, :1020]) + s[1, :1020]) + s[0, :1020]
    assert not torch.equal(other, torch.from_numpy(a))
    per_slab = sum(s[i, :1020].to(torch.bfloat16).float() for i in range(4)).to(torch.bfloat16)
    assert not torch.equal(per_slab, H.reduce_ref(s, 4, 1020))
    assert len(want) == 1020 and bool(torch.isnan(s[:, 1020:]).all())


# ------------------------------------------------------------------------------------------ the GPU test's inputs: right and wrong kernels
PLAIN = [(lc, d, T) for lc in H.LAUNCHES if lc != "lm_wgrad" for d in H.WIDTHS for T in H.T_CAPS]


def rejected(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


@pytest.mark.parametrize("launch,d,T", PLAIN)
def test_plain_launches_right_and_wrong(launch, d, T):
    V = 205 if (d + T) % 3 else 200            # (both vocabularies over the grid; the GPU test runs both everywhere)
    cap = H.launch_shape(launch, d, V, T)[-1]
    for count in H.counts_for(cap):
        c = H.make_case(launch, d, V, T, count, seed=count)
        H.check_plain(c, H.model_plain(c))
        faults = H.FAULTS_M if c.dyn == "m" else H.FAULTS_K
        for f in faults:
            if (f == "count + 1" and count == cap) or (f == "count - 1" and count == 0) or (f.startswith("a row") and count >= cap - 1):
                continue
            if f == "c_rows ignored" and (c.c_rows is None or count == 0):
                continue
            rejected(H.check_plain, c, H.model_plain(c, f))
        if c.dyn == "k":
            for kpz_count in (count,):
                cz = H.make_case(launch, d, V, T, kpz_count, k_pad_zero=1, seed=count)
                H.check_plain(cz, H.model_plain(cz))
                pad_end = min(cz.K, max(64, H.round_up(count, 64)))
                assert bool((cz.A[count:pad_end] == 0).all()) and bool((cz.B[count:pad_end].float() > 1e38).all())
                assert bool(torch.isnan(cz.A[pad_end:]).all()) and bool(torch.isnan(cz.B[pad_end:]).all())
                # whole K-tiles up to the round-up are the contract: a kernel that reads them leaves the same bits
                full = H.Case(**{**cz.__dict__, "count": pad_end, "dyn": "k"})
                assert torch.equal(H.bits(H.model_plain(full)), H.bits(H.model_plain(cz)))
    # random operands: the element-wise bound accepts the rounded fp64 result and rejects a dropped K row
    c = H.make_case(launch, d, V, T, cap // 2 + 2, exact=False, seed=5)
    assert H.check_plain(c, H.model_plain(c)) <= 1.0
    rejected(H.check_plain, c, H.model_plain(c, "count - 1"))


@pytest.mark.parametrize("d,T", [(d, T) for d in H.WIDTHS for T in H.T_CAPS])
def test_slab_launch_right_and_wrong(d, T):
    V = 205 if d == 128 else 200
    cap = T * H.N_TOK
    for count in H.counts_for(cap):
        c = H.make_case("lm_wgrad", d, V, T, count, seed=count)
        for split in H.LM_SPLITS + (16,):
            live = len(H.slab_slices(count, split))
            buf = H.model_slabs(c, split)
            H.check_slabs(c, buf, split)
            cleared = H.model_slabs(c, split, clear=True)
            H.check_reduced(c, H.model_reduced(c, cleared, split, split), split)
            if split not in (2, 16):         # (the faults on two of the splits: one with every slab live at most counts, one with empty slabs)
                continue
            if live:
                rejected(H.check_slabs, c, H.model_slabs(c, split, "one slice dropped"), split)
                rejected(H.check_reduced, c, H.model_reduced(c, H.model_slabs(c, split, "one slice dropped", clear=True), split, split), split)
            if live < split:      # a reduce that reads one slab too many of a buffer nobody cleared
                rejected(H.check_reduced, c, H.model_reduced(c, buf, split, live + 1), split)
            for f in ("count + 1", "count - 1"):
                if split != 2 or (f == "count + 1" and count == cap) or (f == "count - 1" and count == 0):
                    continue
                w = H.Case(**{**c.__dict__, "count": count + (1 if f == "count + 1" else -1)})
                rejected(H.check_slabs, c, H.model_slabs(w, split), split)
    assert len(H.slab_slices(cap, 16)) == (9 if T == 192 else 10) and len(H.slab_slices(65, 5)) == 2 and H.slab_slices(0, 5) == []


@pytest.mark.parametrize("d", H.WIDTHS)
@pytest.mark.parametrize("T", H.GROUP_T[:2])
@pytest.mark.parametrize("with_qkv", [True, False])
def test_grouped_slabs_right_and_wrong(d, T, with_qkv):
    cases, offs, stride = H.make_group(d, T, with_qkv, seed=T)
    for split in (1, 3, 5):
        what = f"d{d} T{T} qkv{with_qkv} split{split}"
        buf = H.model_group(cases, offs, stride, split)
        _, live = H.check_group(cases, offs, stride, split, buf, what)
        assert live == len(H.slab_slices(T, split)) <= split
        dst = H.out_buf(stride // 64, 64, device="cpu")
        dst[:stride] = H.reduce_ref(buf[:split * stride].view(split, stride), live, stride)
        H.check_group_reduced(cases, offs, stride, split, dst, what)
        rejected(H.check_group, cases, offs, stride, split, H.model_group(cases, offs, stride, split, "one slice dropped"), what)
        if with_qkv and split > 1:
            rejected(H.check_group, cases, offs, stride, split, H.model_group(cases, offs, stride, split, "own stride"), what)
        if live < split:
            dst[:stride] = H.reduce_ref(buf[:split * stride].view(split, stride), live + 1, stride)
            rejected(H.check_group_reduced, cases, offs, stride, split, dst, what)
        if live > 1:
            dst[:stride] = H.reduce_ref(buf[:split * stride].view(split, stride), live - 1, stride)
            rejected(H.check_group_reduced, cases, offs, stride, split, dst, what)
    assert (3 * d * d + d * d == stride) if with_qkv else stride == d * d
