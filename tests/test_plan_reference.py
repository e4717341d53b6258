"""tests/_plan_ref.py on the CPU: every checker, fed the reference's own output on the inputs tests/test_gpu_plan.py runs, reports nothing;
one planted fault at a time is rejected by the check that names it; and the chosen inputs reach the forms they are named for."""
import numpy as np
import pytest

import _plan_ref as R
from _util import assert_elementwise


def clean(results):
    _, msgs = R.settle(results)
    assert not msgs, "\n".join(msgs)


def rejected(results, name):
    failed = R.names_failed(results)
    assert any(name in f for f in failed), f"the fault was not caught by '{name}' (failed: {failed})"


# ------------------------------------------------------------------------------------------------------------------ lengths
@pytest.mark.parametrize("S", R.LENGTHS_S)
def test_lengths_reference(S):
    i = R.lengths_inputs(S)
    for with_mask in (True, False):
        k, p = R.lengths_ref(i, with_mask)
        clean(R.lengths_check(i, with_mask, k, p))
    k, p = R.lengths_ref(i, True)
    assert k[3] == 0 and p[3] == 3 * S + S - 1 and (R.lengths_ref(i, False)[0] == S).all()
    if S > 2:
        assert 0 < k[2] < S and (i["mask"][2] != 0).sum() == k[2] and (i["mask"][2, :k[2]] == 0).any(), "sample 2 must have holes"
    rejected(R.lengths_check(i, True, k + (np.arange(6) == 2), p), "key_len")
    rejected(R.lengths_check(i, True, k, p + (np.arange(6) == 3)), "pool_row")


# ------------------------------------------------------------------------------------------------------------------ varlen_plan
ALL_VARLEN = [(c, k, v) for c in R.VARLEN_CASES for k in range(len(R.VARLEN_CASES[c][3])) for v in range(len(R.VARLEN_VARIANTS))]


@pytest.mark.parametrize("case,k,v", ALL_VARLEN)
def test_varlen_reference_is_clean(case, k, v):
    i = R.varlen_inputs(case, k, v)
    w = R.varlen_ref(i)
    clean(R.varlen_check(i, w))
    kind = R.VARLEN_VARIANTS[v]["tc"]
    if kind == "sum":
        assert i["tc"] == i["total"] and w["status"][0] == 0 and w["status"][2] == R.UNW
        assert w["cu"][-1] == i["total"] and (w["key_len"] == i["key_len"]).all()
    elif kind == "less":
        cut = w["key_len"] != i["key_len"]
        assert cut.any() and ((w["key_len"] > 0) & cut).any(), "one sample must be cut partly"
        assert w["status"][0] == 1 and w["status"][2] == 1 and w["cu"][-1] == i["tc"]
    else:
        assert i["tc"] > i["total"] and w["status"][0] == 1 and w["status"][2] == 1
        assert (w["row_b"][i["total"]:i["tc"]] == R.UNW).all()
    assert (i["t_rows"] % 64 == 0) == R.VARLEN_VARIANTS[v]["round"] or i["tc"] % 64 == 0


def test_varlen_inputs_reach_their_forms():
    seen = set()
    for lens in R.VARLEN_CASES["B3-S72"][3]:
        seen |= set(int(x) for x in lens)
    assert {0, 1, 32, 33, 64, 65, 72} <= seen
    i = R.varlen_inputs("B2049-S66-long-samples-in-every-pass", 0, 0)
    ln = i["key_len"]
    is_long = (ln > 32) & (ln <= 64)
    for p0 in (0, 1024, 2048):       # a 33 .. 64-row sample in each pass of the 1024-thread scan
        assert is_long[p0:p0 + 1024].any(), p0
    assert is_long[1023] and is_long[1024] and is_long[2048] and not is_long[1500] and not is_long[1501]
    w = R.varlen_ref(i)
    assert w["long_list"][0] == is_long.sum() > 3
    assert [R.VARLEN_CASES[c][0] for c in ("B1024-S8", "B1025-S8", "B2049-S4")] == [1024, 1025, 2049]


def _plant(w, key, fn):
    g = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}
    fn(g[key])
    return g


def test_varlen_planted_faults():
    i = R.varlen_inputs("B3-S72", 1, 0)               # lengths (33, 64, 65), long_list given
    w = R.varlen_ref(i)

    def off_by_one(cu):
        cu[1] += 1
    rejected(R.varlen_check(i, _plant(w, "cu", off_by_one)), "cu")

    def neighbour(p):                                 # the last token of sample 0 mapped to the first row of sample 1
        p[32] = w["cu"][1]
    rejected(R.varlen_check(i, _plant(w, "pad2c", neighbour)), "pad2c")

    def missing(ll):                                  # one entry fewer: the count and the lists
        ll[0] -= 1
        ll[ll[0] + 1] = R.UNW
    rejected(R.varlen_check(i, _plant(w, "long_list", missing)), "long_list")

    def tail(ids_c):
        ids_c[-1] = 0
    j = R.varlen_inputs("B3-S72", 1, 1)
    rejected(R.varlen_check(j, _plant(R.varlen_ref(j), "ids_c", tail)), "tail rows")

    j = R.varlen_inputs("B3-S72", 1, 2)               # tc < sum
    wj = R.varlen_ref(j)
    b = int(np.flatnonzero(wj["key_len"] != j["key_len"])[0])

    def not_cut(kl):
        kl[b] = j["key_len"][b]
    rejected(R.varlen_check(j, _plant(wj, "key_len", not_cut)), "key_len")

    def flag(st):
        st[0] = 0
    rejected(R.varlen_check(j, _plant(wj, "status", flag)), "status")


# ------------------------------------------------------------------------------------------------------------------ grid, ranges
@pytest.mark.parametrize("S", R.RANGES_S)
def test_ranges_reference(S):
    i = R.ranges_inputs(S)
    lo, hi = R.ranges_ref(i)
    m = i["mask"].reshape(-1, S)
    for r in range(m.shape[0]):
        nz = np.flatnonzero(m[r])
        assert (lo[r], hi[r]) == ((nz[0], nz[-1]) if len(nz) else (0, -1))
    assert (hi == -1).any() and ((lo == hi) & (hi >= 0)).any()
    if S > 2:
        assert ((hi - lo) > 1).any()


def test_grid_reference():
    for d in R.GRID_D:
        i = R.grid_inputs(d)
        out = R.grid_ref(i)
        assert (i["pad2c"] < 0).sum() == i["n_pos"] - 41 and not out[0].any() and (out[i["pad2c"] >= 0].any(1)).all()


# ------------------------------------------------------------------------------------------------------------------ head_compact
@pytest.mark.parametrize("T", R.COMPACT_T)
@pytest.mark.parametrize("n", R.COMPACT_N)
def test_compact_reference(T, n):
    for pattern in R.COMPACT_PATTERNS:
        lab = R.compact_labels(T, n, pattern)
        hist0 = np.arange(1, 34, dtype=np.int32)[:max(n, 33)]
        w = R.compact_ref(lab, T, n, hist0)
        clean(R.compact_check(lab, T, n, w, hist0))
        M, Lm = w["counts"]
        if pattern == "labels NULL" or pattern == "none -100":
            assert (M, Lm) == (T, T * n)
        elif pattern == "all -100":
            assert (M, Lm) == (0, 0) and (w["row_idx"] == R.UNW).all()
        elif pattern == "last token only":
            assert (M, Lm) == (1, n) and w["row_idx"][0] == T - 1
        elif T * n > 50:
            assert 0 < Lm < T * n
        # every labelled cell, by brute force
        cells = [(t, f) for t in range(T) for f in range(n) if lab is None or lab[t, f] != -100]
        assert [int(x) for x in w["sel_tok"][:Lm]] == [t for t, _ in cells]
        assert [int(x) % n for x in w["sel_src"][:Lm]] == [f for _, f in cells]
        assert (w["slot_hist"][:n].sum() - hist0[:n].sum() == Lm) if n <= 32 else (w["slot_hist"] == hist0).all()
        if Lm > 1:
            g = dict(w, sel_src=w["sel_src"].copy())
            g["sel_src"][[0, 1]] = g["sel_src"][[1, 0]]
            rejected(R.compact_check(lab, T, n, g, hist0), "sel_src")


# ------------------------------------------------------------------------------------------------------------------ head_slot_sort
def sort_runs(name):
    T, n, tr, recipes = R.SORT_CASES[name]
    return [R.sort_inputs(T, n, tr, R.sort_labels(T, n, tr, rec, k)) for k, rec in enumerate(recipes)]


@pytest.mark.parametrize("name", list(R.SORT_CASES))
def test_sort_reference_is_clean_in_any_order(name):
    for i in sort_runs(name):
        clean(R.sort_check(i, R.sort_any_order(i)))
        clean(R.sort_check(i, R.sort_any_order(i, np.random.default_rng(5))))


def test_sort_inputs_reach_their_forms():
    runs = {name: sort_runs(name) for name in R.SORT_CASES}
    assert 0 < runs["Lm<1024-empty-slot"][0]["Lm"] < 1024 and runs["Lm<1024-empty-slot"][0]["cells"][5] == 0
    for name, f, tr in (("Lm>4096-slot-of-exactly-128", 2, 128), ("Lm>4096-tile-256-slot-of-exactly-256", 3, 256), ("n32-cells-then-Lm=0", 31, 256)):
        i = runs[name][0]
        assert i["Lm"] > 4096 and i["cells"][f] == tr == i["tile_rows"], name
    assert runs["Lm>4096-tile-256-slot-of-exactly-256"][0]["cells"][7] == 0
    assert runs["Lm=0-then-cells"][0]["Lm"] == 0 and runs["Lm=0-then-cells"][1]["Lm"] > 0
    assert runs["n32-cells-then-Lm=0"][1]["Lm"] == 0
    for name, (a, b) in runs.items():       # the second forward differs from the first
        assert not np.array_equal(a["cells"], b["cells"]), name


def test_sort_planted_faults():
    i = sort_runs("Lm>4096-slot-of-exactly-128")[0]
    w = R.sort_any_order(i, np.random.default_rng(6))
    start, cells = R.sort_plan(i)

    def plant(fn):
        g = {k: v.copy() for k, v in w.items()}
        fn(g)
        return R.sort_check(i, g)

    def swap(g):           # two cells of different slots trade places, consistently in every list
        p, q = int(start[0]), int(start[1])
        for k in ("a_tok", "a_cell", "c_l"):
            g[k][[p, q]] = g[k][[q, p]]
        g["cellpos"][g["c_l"][p]], g["cellpos"][g["c_l"][q]] = p, q
    rejected(plant(swap), "every slot's range holds exactly its cells")

    pad = int(start[0] + cells[0])
    assert pad < start[1]

    def pad_zero(g):
        g["c_l"][pad] = 0
    rejected(plant(pad_zero), "pad rows: c_l = -1")

    def wrong_tile(g):
        g["tile_off"][int(start[1]) // 128] = 0
    rejected(plant(wrong_tile), "tile_off")

    def cursors(g):
        g["slot_state"][i["n"] + 3] = int(cells[3])
    rejected(plant(cursors), "counts, cursors and ticket are zero")

    def ticket(g):
        g["slot_state"][3 * i["n"] + 1] = 1
    rejected(plant(ticket), "counts, cursors and ticket are zero")

    def tok(g):
        g["a_tok"][int(start[2]) + 1] += 1
    rejected(plant(tok), "a_tok[p] == row_idx")

    def pos(g):
        g["cellpos"][7] += 1
    rejected(plant(pos), "cellpos[c_l[p]] == p")

    def stale_start(g):    # the starts of the previous forward
        g["slot_state"][2 * i["n"] + 1] += 128
    rejected(plant(stale_start), "total and padded starts")

    def behind(g):
        g["a_tok"][int(start[-1])] = 0
    rejected(plant(behind), "nothing written behind")


# ------------------------------------------------------------------------------------------------------------------ gather, remap
@pytest.mark.parametrize("d", R.GATHER_D)
def test_gather_reference(d):
    for count in R.GATHER_COUNTS:
        for scatter in (0, 1):
            i = R.gather_inputs(d, count, scatter)
            w = R.gather_ref(i)
            clean(R.gather_check(i, w))
            n = min(i["cap"], count)
            assert (w == R.SENT16).all(1).sum() == i["dst_rows"] - (n if scatter else n), "untouched rows"
            if not scatter:        # a gathered row from idx[i + 1]
                g = w.copy()
                g[3] = i["src"][i["idx"][4]]
                assert i["idx"][3] != i["idx"][4]
                rejected(R.gather_check(i, g), "rows moved")
            if n < i["dst_rows"]:  # an unstored row that was written
                g = w.copy()
                g[np.flatnonzero((w == R.SENT16).all(1))[0], 0] = 0
                rejected(R.gather_check(i, g), "stay untouched")
        for variant in R.REMAP_VARIANTS:
            i = R.remap_inputs(d, R.GATHER_COUNTS[1], variant)
            idx, dst, status = R.remap_ref(i)
            clean(R.remap_check(i, idx, dst, status))
            assert (status[2] == 1) == (variant != "no -1 and status") and status[0] == R.UNW
            if variant == "a -1 and status":
                assert (idx == i["pad_row"]).sum() == 1
                rejected(R.remap_check(i, i["idx"], dst, status), "idx rewritten")
                rejected(R.remap_check(i, idx, dst, np.full(3, R.UNW, np.int32)), "status")


# ------------------------------------------------------------------------------------------------------------------ head_cell_sum
@pytest.mark.parametrize("d", R.CELLSUM_D)
def test_cellsum_reference(d):
    for with_pad2c in (False, True):
        i = R.cellsum_inputs(d, with_pad2c)
        w = R.cellsum_ref(i)
        clean(R.cellsum_check(i, w))
        assert set(i["cnt"].tolist()) == set(R.CELLSUM_COUNTS)
        assert (w == R.SENT16).all(1).sum() == (i["cnt"] == 0).sum()
        if with_pad2c:
            assert (i["pad2c"] < 0).sum() == 1 and i["cnt"][i["pad2c"] < 0][0] > 0
        x = R.f32_of_bits(i["dxs"])
        t = int(np.flatnonzero(i["cnt"] == 13)[0])
        rows = i["cellpos"][i["l_off"][t]:i["l_off"][t] + 13]
        row = R.cellsum_row(i, t)

        g = w.copy()           # a cell summed twice
        acc = np.zeros(d, np.float32)
        for r in list(rows) + [rows[4]]:
            acc = (acc + x[r]).astype(np.float32)
        g[row] = R.rne_bits(acc)
        rejected(R.cellsum_check(i, g), "fp32 sum in cell order, one rounding")

        g = w.copy()           # a sum rounded per cell
        acc = np.zeros(d, np.float32)
        for r in rows:
            acc = R.f32_of_bits(R.rne_bits((acc + x[r]).astype(np.float32)))
        g[row] = R.rne_bits(acc)
        rejected(R.cellsum_check(i, g), "fp32 sum in cell order, one rounding")

        g = w.copy()           # an unstored row that was written
        g[np.flatnonzero((w == R.SENT16).all(1))[0]] = 0
        rejected(R.cellsum_check(i, g), "keep their sentinel")


def test_cellsum_order_shows():
    """The inputs are such that the fp32 sum depends on the order of the additions: a sum in reversed cell order is rejected."""
    for d in R.CELLSUM_D:
        i = R.cellsum_inputs(d, False)
        j = dict(i, cellpos=i["cellpos"].copy())
        for t in range(i["TP"]):
            lo, c = i["l_off"][t], i["cnt"][t]
            j["cellpos"][lo:lo + c] = i["cellpos"][lo:lo + c][::-1]
        rejected(R.cellsum_check(i, R.cellsum_ref(j)), "fp32 sum in cell order, one rounding")


# ------------------------------------------------------------------------------------------------------------------ gemm_indexed
@pytest.mark.parametrize("name", [n for n in R.GEMM_CASES if "300-tiles" not in n])
def test_gemm_reference(name):
    i = R.gemm_inputs(name)
    mode, N, K, passed, cells, m_kind, exact = R.GEMM_CASES[name]
    assert i["tile"] == (256 if "tile256" in name and "falls-back" not in name else 128)
    assert len(i["tile_off"]) * i["tile"] == i["total"] and (np.diff(i["tile_off"]) >= 0).all()
    m, dst = R.gemm_stored(i)
    assert len(set(dst.tolist())) == len(dst) and (len(m) == 0) == (m_kind == "zero")
    assert (i["c_rows"][:i["total"]] < 0).sum() > (i["total"] - i["cells"].sum()), "negative c_rows on real cells too"
    if not exact:
        dst, ref, ab = R.gemm_ref64(i)
        assert_elementwise(ref.float().to(R.torch.bfloat16), ref, ab, K, what=name)
        return
    assert len(np.unique(i["a_rows"][m])) < len(m) or len(m) == 0, "a_rows with repeats"
    w = R.gemm_ref_exact(i)
    clean(R.gemm_check_exact(i, w))
    if len(m):
        g = w.copy()       # a cell that lands in the neighbouring slot's weight block
        f = int(i["slot_of"][m[0]])
        other = (f + 1) % i["ns"]
        g[dst[0]] = R.bits_of(R.gemm_expected(mode, R.bf16_of(i["A"]), R._slot_B(i, other))[0])[i["a_rows"][m[0]]]
        rejected(R.gemm_check_exact(i, g), "stored rows")
    g = w.copy()           # an unstored row that was written
    g[np.flatnonzero((w == R.SENT16).all(1))[0], 5] = 0
    rejected(R.gemm_check_exact(i, g), "keep their sentinel")


def test_gemm_big_case_has_more_tiles_than_compute_units():
    for mn in ("NT", "NN"):
        mode, N, K, passed, cells, m_kind, exact = R.GEMM_CASES[f"{mn}-192-300-tiles"]
        padded = [(c + 127) // 128 * 128 for c in cells]
        assert sum(padded) == 300 * 128 and 300 > 256 and len(set(padded)) == 1


def test_plain_reference():
    i = R.plain_inputs()
    w = R.plain_ref(i)
    stored = (w != R.SENT16).any(1)
    m = np.arange(i["m_dev"])
    assert stored.sum() == (i["c_rows"][m] >= 0).sum() < i["m_dev"] < i["M"]


# ------------------------------------------------------------------------------------------------------------------ row selection
def test_wgt_reference():
    for cells in R.WGT_CELLS:
        lab = R.wgt_inputs(cells)
        w = R.wgt_ref(lab)
        assert w.dtype == np.float32 and w[0] == np.float32(1) / np.float32(1e-7) and np.isfinite(w).all()
        assert w[1] == np.float32(1) / (np.float32(cells) + np.float32(1e-7))


def test_blend_reference():
    for e in R.BLEND_E:
        i = R.blend_inputs(e, 0, True, True)
        out, flag = R.blend_ref(i)
        gone = i["rows_map"] >= i["n_logical"]
        assert gone.sum() == 3 and not out[gone].any() and not flag[gone].any()
        a, b = R.blend_ref(R.blend_inputs(e, 0, True, False)), R.blend_ref(R.blend_inputs(e, 1, True, False))
        assert a[1][2] == 0 and b[1][2] == 1 and a[1][0] == 0 and a[1][1] == 0 and a[1][3] == 1
        none = R.blend_ref(R.blend_inputs(e, 0, False, False))
        assert not none[1].any()
        # the ties: row 1 rounds down to the even value, row 2 up to the even value, rows 3 / 4 are just off the tie
        j = R.blend_inputs(e, 0, False, False)
        base = R.rne_bits(j["raw"])
        lo = (j["raw"].view(np.uint32) >> 16).astype(np.uint16)
        assert (j["raw"][1:3].view(np.uint32) & 0xFFFF == 0x8000).all()
        assert (base[1] % 2 == 0).all() and (base[2] % 2 == 0).all() and (base[1] == lo[1]).any() and (base[2] == lo[2] + 1).any()
        assert (base[3] == lo[3] + 1).all() and (base[4] == lo[4]).all()


def test_tokgrad_reference():
    for T in R.TOKGRAD_T:
        i = R.tokgrad_inputs(T)
        w = R.tokgrad_ref(i)
        assert w.dtype == np.float32 and (i["dtok0"] != 0).any() and (w != i["dtok0"]).any()
