"""The element-wise GEMM check helpers of tests/_util.py (CPU): exact operands really give exact fp32 sums in any order, and the
faults a whole-matrix rel-L2 cannot see break the exact and the element-wise checks."""
import numpy as np
import pytest
import torch

from _util import assert_elementwise, exact_bound, exact_operands, gemm_expected, gemm_ref64, rel_l2


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_exact_operands_sum_exactly_in_any_order(mode):
    M, N, K = 12, 10, 3072
    A, B, R = exact_operands(M, N, K, seed=3, mode=mode, residual=True)
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16
    assert A.shape == ((K, M) if mode == 2 else (M, K)) and B.shape == ((N, K) if mode == 0 else (K, N))
    a = (A.double().t() if mode == 2 else A.double()).numpy()
    b = (B.double().t() if mode == 0 else B.double()).numpy()
    assert (a == 0).any() and len(np.unique(np.abs(a[a != 0]))) > 4       # zeros and several octaves present
    want = a @ b + R.double().numpy()
    prod = a[:, None, :] * b.T[None, :, :]                                  # [M, N, K] products (exact in fp32)
    assert np.array_equal(prod.astype(np.float32).astype(np.float64), prod)
    rng = np.random.default_rng(0)
    for _ in range(4):                                                      # sequential fp32 sums in random K orders
        perm = rng.permutation(K)
        s = np.cumsum(prod[:, :, perm].astype(np.float32), axis=2, dtype=np.float32)[:, :, -1] + R.float().numpy()
        assert np.array_equal(s.astype(np.float64), want)
    s = prod.astype(np.float32).reshape(M, N, 48, 64).sum(axis=3, dtype=np.float32)   # 64-deep K-tile partials, then the tiles
    assert np.array_equal(s[:, :, ::-1].sum(axis=2, dtype=np.float32).astype(np.float64), a @ b)
    c16, c32 = gemm_expected(mode, A, B, R)
    assert torch.equal(c32.double(), torch.from_numpy(want)) and torch.equal(c16, c32.to(torch.bfloat16))
    assert exact_bound(41472, residual=True) < 2 ** 24                     # the longest K the GPU tests use (K = T of ogbl-ppa rows)
    with pytest.raises(AssertionError):
        exact_operands(4, 4, 2 ** 20, seed=0)


def test_local_faults_pass_rel_l2_but_not_the_elementwise_checks():
    """A row that missed one 64-deep K-tile, a row whose last 4 columns were not stored and one 16x16 fragment that missed a K-tile, in
    a 5 696 x 192 x 3 072 product (the headline row count): each keeps the whole-matrix rel-L2 below the old 4e-3 bound, and each is
    caught by the exact comparison and by assert_elementwise, which names the broken tile."""
    M, N, K = 5696, 192, 3072
    A, B, _ = exact_operands(M, N, K, seed=11)
    want16, _ = gemm_expected(0, A, B)
    ref, ab = gemm_ref64(0, A, B)
    a, b = A.double(), B.double()
    assert assert_elementwise(want16, ref, ab, K, what="exact result") <= 1.0
    ktile = lambda rows, cols, t: a[rows, 64 * t:64 * t + 64] @ b[cols, 64 * t:64 * t + 64].t()   # noqa: E731
    faults = {}
    f = ref.clone()
    f[1234] -= ktile(slice(1234, 1235), slice(None), 17)[0]
    faults["row 1234 without K-tile 17"] = (f, (1234 // 64, 0))
    f = ref.clone()
    f[M - 1, N - 4:] = 0
    faults["last row, last 4 columns not stored"] = (f, ((M - 1) // 64, (N - 4) // 64))
    f = ref.clone()
    f[4096:4112, 128:144] -= ktile(slice(4096, 4112), slice(128, 144), 47)
    faults["16x16 fragment without the last K-tile"] = (f, (4096 // 64, 128 // 64))
    for name, (f, tile) in faults.items():
        got = f.float().to(torch.bfloat16)
        assert rel_l2(got.float().numpy(), ref.numpy()) < 4e-3, name      # the gap: the old whole-matrix check passes
        assert not torch.equal(got, want16), name
        with pytest.raises(AssertionError, match=f"64x64 tile\\(s\\) \\[\\({tile[0]}, {tile[1]}\\)"):
            assert_elementwise(got, ref, ab, K, what=name)
