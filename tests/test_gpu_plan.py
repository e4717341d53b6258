"""The integer machinery of a pre-training step, one launcher at a time through the C ABI (gget_op_lengths, gget_op_sum_lengths,
gget_op_varlen_plan, gget_op_rows_to_grid, gget_op_ranges_from_mask3d, gget_op_head_compact, gget_op_head_slot_sort, gget_op_head_cell_sum,
gget_op_gather_rows, gget_op_gather_rows_remap, gget_op_gemm_indexed, gget_op_sample_mask_wgt, gget_op_raw_blend, gget_op_raw_tok_grad)
against the plain statements of tests/_plan_ref.py.  Every comparison is integer-exact or bit for bit - no tolerance - except the two
random-normal GEMM cases, which are held to tests/_util.py assert_elementwise as every other GEMM plan is.  Outputs land in buffers
pre-filled with sentinels (tests/_gpu_out.py) with pad rows behind them, and the expected arrays carry the sentinel wherever the contract
says "not written".  Where the kernel leaves an order free (a cell's position inside its slot) the invariant is checked."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _plan_ref as R
from _gpu_out import Out, P, ST
from _util import assert_elementwise, record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
BF, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64


@pytest.fixture(scope="module")
def lib():
    return L.load()


def dev(a):
    """numpy integer / float array (or None) -> device tensor."""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dbf(bits):
    return R.bf16_of(bits).cuda()


def ints(n, dtype=I32, init=None):
    return Out(n, 1, dtype, None if init is None else torch.from_numpy(np.ascontiguousarray(init)))


def ival(o):
    return o.body().reshape(-1).numpy()


def bval(o):
    return R.bits_of(o.body())


def tagged(tag, results):
    return [(f"[{tag}] {n}", r, None if m is None else f"[{tag}] {m}") for n, r, m in results]


def finish(op, case, results):
    """Record the case as pass (0) or fail (1), then fail on whatever differed."""
    _, msgs = R.settle(results)
    record_error(f"plan/{op}", case, 1.0 if msgs else 0.0, 0.0)
    assert not msgs, f"{op} {case}:\n" + "\n".join(msgs)


# ------------------------------------------------------------------------------------------------------------------ lengths
@pytest.mark.parametrize("S", R.LENGTHS_S)
def test_lengths(lib, S):
    i = R.lengths_inputs(S)
    mask, ids = dev(i["mask"]), dev(i["ids"])
    results = []
    for with_mask in (True, False):
        k, p = ints(i["B"]), ints(i["B"])
        L.check(lib.gget_op_lengths(P(mask) if with_mask else None, P(ids), i["ldF"], i["pad_id"], P(k.buf), P(p.buf), i["B"], S, ST()))
        results += tagged("mask" if with_mask else "mask NULL", R.lengths_check(i, with_mask, ival(k), ival(p)))
    k = ints(i["B"])      # key_len alone: ids NULL, pool_row NULL
    L.check(lib.gget_op_lengths(P(mask), None, 0, 0, P(k.buf), None, i["B"], S, ST()))
    results += tagged("key_len alone", [R.same("key_len", ival(k), R.lengths_ref(i, True)[0])])
    finish("lengths", f"S{S}", results)


@pytest.mark.parametrize("B", R.SUM_B)
def test_sum_lengths(lib, B):
    kl = R.sum_inputs(B)
    d_kl, out = dev(kl), ints(1)
    L.check(lib.gget_op_sum_lengths(P(d_kl), B, P(out.buf), ST()))
    finish("sum_lengths", f"B{B}", [R.same("sum", ival(out), np.array([kl.sum()], np.int32))])


# ------------------------------------------------------------------------------------------------------------------ varlen_plan
def run_varlen(lib, i):
    B, S, F, t_rows = i["B"], i["S"], i["F"], i["t_rows"]
    ids, pos = dev(i["ids"]), dev(i["pos"])
    o = dict(key_len=ints(B, init=i["key_len"]), cu=ints(B + 1), ids_c=Out(t_rows, F, I64), pos_c=ints(t_rows, I64), row_b=ints(t_rows),
             pad2c=ints(B * S), c2p=ints(t_rows), status=ints(3))
    if i["pool_row"] is not None:
        o["pool_row"] = ints(B, init=i["pool_row"])
    if i["long"]:
        o["long_list"] = ints(3 * B + 1)
    ptr = lambda k: P(o[k].buf) if k in o else None      # noqa: E731
    L.check(lib.gget_op_varlen_plan(P(ids), i["ldF"], F, P(pos), ptr("key_len"), ptr("pool_row"), ptr("cu"), ptr("ids_c"), ptr("pos_c"),
                                    ptr("row_b"), ptr("pad2c"), ptr("c2p"), ptr("status"), B, S, i["tc"], t_rows, i["pad_id"],
                                    ptr("long_list"), ST()))
    return {k: (v.body().numpy() if k == "ids_c" else ival(v)) for k, v in o.items()}


@pytest.mark.parametrize("case", list(R.VARLEN_CASES))
def test_varlen_plan(lib, case):
    results = []
    for k in range(len(R.VARLEN_CASES[case][3])):
        for v, var in enumerate(R.VARLEN_VARIANTS):
            i = R.varlen_inputs(case, k, v)
            results += tagged(f"lengths {k}, {var['name']}", R.varlen_check(i, run_varlen(lib, i)))
    finish("varlen_plan", case, results)


# ------------------------------------------------------------------------------------------------------------------ rows_to_grid, ranges
@pytest.mark.parametrize("d", R.GRID_D)
def test_rows_to_grid(lib, d):
    i = R.grid_inputs(d)
    src, pad2c, out = dbf(i["src"]), dev(i["pad2c"]), Out(i["n_pos"], d, BF)
    L.check(lib.gget_op_rows_to_grid(P(src), P(pad2c), P(out.buf), i["n_pos"], d, ST()))
    finish("rows_to_grid", f"d{d}", [R.same("grid rows, zero rows where pad2c is -1", bval(out), R.grid_ref(i))])


@pytest.mark.parametrize("S", R.RANGES_S)
def test_ranges_from_mask3d(lib, S):
    i = R.ranges_inputs(S)
    mask, lo, hi = dev(i["mask"]), ints(i["B"] * S), ints(i["B"] * S)
    L.check(lib.gget_op_ranges_from_mask3d(P(mask), P(lo.buf), P(hi.buf), i["B"], S, ST()))
    w_lo, w_hi = R.ranges_ref(i)
    finish("ranges_from_mask3d", f"S{S}", [R.same("key_lo", ival(lo), w_lo), R.same("key_hi", ival(hi), w_hi)])


# ------------------------------------------------------------------------------------------------------------------ head_compact
def run_compact(lib, lab, T, n, hist):
    """hist: an Out of the slot histogram / slot_state to add to, or None."""
    d_lab = dev(lab)
    ws = torch.empty(int(lib.gget_op_head_compact_ws_bytes(T)) // 4 + 1, dtype=I32, device="cuda")
    o = dict(cnt=ints(T), m_off=ints(T), l_off=ints(T), counts=ints(2), row_idx=ints(T), sel_src=ints(T * n), sel_label=ints(T * n),
             sel_tok=ints(T * n))
    L.check(lib.gget_op_head_compact(P(d_lab), T, n, *[P(o[k].buf) for k in ("cnt", "m_off", "l_off", "counts", "row_idx", "sel_src",
                                                                                 "sel_label", "sel_tok")], P(ws),
                                     None if hist is None else P(hist.buf), ST()))
    return o


@pytest.mark.parametrize("T", R.COMPACT_T)
@pytest.mark.parametrize("n", R.COMPACT_N)
def test_head_compact(lib, T, n):
    assert lib.gget_op_head_compact_ws_bytes(T) >= 8 * ((T + 255) // 256)
    results = []
    for pattern in R.COMPACT_PATTERNS:
        lab = R.compact_labels(T, n, pattern)
        hist0 = np.arange(1, 34, dtype=np.int32)           # (n = 33: one entry more than the kernel may ever touch)
        hist = ints(33, init=hist0)
        o = run_compact(lib, lab, T, n, hist)
        got = {k: ival(v) for k, v in o.items()}
        got["slot_hist"] = ival(hist)
        results += tagged(pattern, R.compact_check(lab, T, n, got, hist0))
    o = run_compact(lib, R.compact_labels(T, n, "half"), T, n, None)
    results += tagged("slot_hist NULL", [t for t in R.compact_check(R.compact_labels(T, n, "half"), T, n, {k: ival(v) for k, v in o.items()})])
    finish("head_compact", f"T{T}-n{n}", results)


# ------------------------------------------------------------------------------------------------------------------ head_slot_sort
def lm_ptr(c):
    """Pointer to counts[1] = Lm of a run_compact result."""
    return ctypes.c_void_p(c["counts"].buf.data_ptr() + 4)


@pytest.mark.parametrize("name", list(R.SORT_CASES))
def test_head_slot_sort(lib, name):
    """head_compact -> head_slot_sort, twice in a row on different labels through ONE slot_state: the second result must hold as well."""
    T, n, tr, recipes = R.SORT_CASES[name]
    state = ints(3 * n + 2, init=np.zeros(3 * n + 2, np.int32))       # (cleared once, as the workspace is at creation)
    results = []
    for k, rec in enumerate(recipes):
        lab = R.sort_labels(T, n, tr, rec, k)
        i = R.sort_inputs(T, n, tr, lab)
        c = run_compact(lib, lab, T, n, state)
        results += tagged(f"forward {k}, compaction", R.compact_check(lab, T, n, {key: ival(v) for key, v in c.items()}))
        results += tagged(f"forward {k}", [R.same("slot counts in slot_state[0, n)", ival(state)[:n], i["cells"].astype(np.int32))])
        size = i["cap"] + n * tr
        o = dict(a_tok=ints(size), a_cell=ints(size), c_l=ints(size), cellpos=ints(i["cap"]), tile_off=ints(size // tr + 1), total=ints(1))
        L.check(lib.gget_op_head_slot_sort(P(c["sel_src"].buf), P(c["row_idx"].buf), lm_ptr(c), P(state.buf), P(o["a_tok"].buf), P(o["a_cell"].buf),
                                           P(o["c_l"].buf), P(o["cellpos"].buf), P(o["tile_off"].buf), P(o["total"].buf), i["cap"], n,
                                           i["slot_elems"], tr, ST()))
        got = {key: ival(v) for key, v in o.items()}
        got["slot_state"] = ival(state)
        results += tagged(f"forward {k}", R.sort_check(i, got))
    finish("head_slot_sort", name, results)


# ------------------------------------------------------------------------------------------------------------------ gather_rows
@pytest.mark.parametrize("d", R.GATHER_D)
def test_gather_rows(lib, d):
    results = []
    for count in R.GATHER_COUNTS:
        for scatter in (0, 1):
            i = R.gather_inputs(d, count, scatter)
            src, idx, cnt, dst = dbf(i["src"]), dev(i["idx"]), dev(np.array([count], np.int32)), Out(i["dst_rows"], d, BF)
            L.check(lib.gget_op_gather_rows(P(src), P(idx), P(cnt), P(dst.buf), i["cap"], d, scatter, ST()))
            results += tagged(f"count {count}, {'scatter' if scatter else 'gather'}", R.gather_check(i, bval(dst)))
    finish("gather_rows", f"d{d}", results)


@pytest.mark.parametrize("d", R.GATHER_D)
def test_gather_rows_remap(lib, d):
    results = []
    for count in R.GATHER_COUNTS:
        for variant in R.REMAP_VARIANTS:
            i = R.remap_inputs(d, count, variant)
            src, pad2c, cnt = dbf(i["src"]), dev(i["pad2c"]), dev(np.array([count], np.int32))
            idx, dst, status = ints(i["cap"], init=i["idx"]), Out(i["cap"], d, BF), ints(3)
            L.check(lib.gget_op_gather_rows_remap(P(src), P(idx.buf), P(cnt), P(pad2c), P(dst.buf), i["cap"], d, i["pad_row"],
                                                  P(status.buf) if i["status"] else None, ST()))
            results += tagged(f"count {count}, {variant}", R.remap_check(i, ival(idx), bval(dst), ival(status)))
    finish("gather_rows_remap", f"d{d}", results)


# ------------------------------------------------------------------------------------------------------------------ head_cell_sum
@pytest.mark.parametrize("d", R.CELLSUM_D)
def test_head_cell_sum(lib, d):
    results = []
    for with_pad2c in (False, True):
        i = R.cellsum_inputs(d, with_pad2c)
        dxs, cellpos, cnt, l_off, pad2c = dbf(i["dxs"]), dev(i["cellpos"]), dev(i["cnt"]), dev(i["l_off"]), dev(i["pad2c"])
        dhid = Out(i["rows"], d, BF)
        L.check(lib.gget_op_head_cell_sum(P(dxs), P(cellpos), P(cnt), P(l_off), P(pad2c), P(dhid.buf), i["TP"], d, i["pad_row"], ST()))
        results += tagged("pad2c with a -1" if with_pad2c else "pad2c NULL", R.cellsum_check(i, bval(dhid)))
    finish("head_cell_sum", f"d{d}", results)


# ------------------------------------------------------------------------------------------------------------------ gemm_indexed
@pytest.mark.parametrize("name", list(R.GEMM_CASES))
def test_gemm_indexed(lib, name):
    i = R.gemm_inputs(name)
    N, K = i["N"], i["K"]
    A, B, C = dbf(i["A"]), dbf(i["B"]), Out(i["c_total"], N, BF)
    m_dev, a_rows, c_rows, tile_off = dev(np.array([i["m_dev"]], np.int32)), dev(i["a_rows"]), dev(i["c_rows"]), dev(i["tile_off"])
    L.check(lib.gget_op_gemm_indexed(i["mode"], P(A), P(B), P(C.buf), i["M_cap"], N, K, K, K if i["mode"] == R.NT else N, N, P(m_dev),
                                     P(a_rows), P(tile_off), i["passed"], P(c_rows), ST()))
    got = C.body()
    if i["exact"]:
        finish("gemm_indexed", name, R.gemm_check_exact(i, R.bits_of(got)))
        return
    dst, ref, ab = R.gemm_ref64(i)
    wr = np.zeros(i["c_total"], bool)
    wr[dst] = True
    results = [R.same("unstored rows keep their sentinel", R.bits_of(got)[~wr], R.sent_rows(int((~wr).sum()), N))]
    try:
        assert_elementwise(got[torch.from_numpy(dst.astype(np.int64))], ref, ab, K, what=name)
    except AssertionError as e:
        results.append(("stored rows within the GEMM bound", float("inf"), str(e)))
    finish("gemm_indexed", name, results)


def test_gemm_plain_path_with_c_rows(lib):
    """a_rows and b_tile_off NULL: the ordinary single-problem launch with the row scatter in its epilogue."""
    i = R.plain_inputs()
    A, B, C = dbf(i["A"]), dbf(i["B"]), Out(i["c_total"], i["N"], BF)
    m_dev, c_rows = dev(np.array([i["m_dev"]], np.int32)), dev(i["c_rows"])
    L.check(lib.gget_op_gemm_indexed(R.NN, P(A), P(B), P(C.buf), i["M"], i["N"], i["K"], i["K"], i["N"], i["N"], P(m_dev), None, None, 0,
                                     P(c_rows), ST()))
    finish("gemm_indexed", "plain-NN-200x192x128-c_rows-m_dev150", [R.same("C, bit for bit, sentinels on the unstored rows", bval(C), R.plain_ref(i))])


# ------------------------------------------------------------------------------------------------------------------ row selection
@pytest.mark.parametrize("cells", R.WGT_CELLS)
def test_sample_mask_wgt(lib, cells):
    lab = R.wgt_inputs(cells)
    d_lab, w = dev(lab), Out(lab.shape[0], 1, F32)
    L.check(lib.gget_op_sample_mask_wgt(P(d_lab), P(w.buf), lab.shape[0], cells, ST()))
    got = w.body().reshape(-1).numpy()
    finish("sample_mask_wgt", f"cells{cells}", [R.same("w, bit for bit", got.view(np.uint32), R.wgt_ref(lab).view(np.uint32))])


@pytest.mark.parametrize("e", R.BLEND_E)
def test_raw_blend(lib, e):
    results = []
    for first_only, with_labels, with_map in ((0, True, False), (1, True, False), (0, False, False), (0, True, True), (1, True, True),
                                              (0, False, True)):
        i = R.blend_inputs(e, first_only, with_labels, with_map)
        raw, lab, tok, rows_map = dev(i["raw"]), dev(i["labels"]), dbf(i["tok"]), dev(i["rows_map"])
        out, flag = Out(i["T"], e, BF), ints(i["T"])
        L.check(lib.gget_op_raw_blend(P(raw), P(lab), i["n"], first_only, P(tok), P(out.buf), P(flag.buf), i["T"], e, P(rows_map),
                                      i["n_logical"], ST()))
        w_out, w_flag = R.blend_ref(i)
        tag = f"first_only {first_only}, labels {'given' if with_labels else 'NULL'}, rows_map {'given' if with_map else 'NULL'}"
        results += tagged(tag, [R.same("out, bit for bit", bval(out), w_out), R.same("flag", ival(flag), w_flag)])
    finish("raw_blend", f"e{e}", results)


@pytest.mark.parametrize("T", R.TOKGRAD_T)
def test_raw_tok_grad(lib, T):
    i = R.tokgrad_inputs(T)
    dx, flag = dbf(i["dx"]), dev(i["flag"])
    dtok = Out(1, i["e"], F32, torch.from_numpy(i["dtok0"]))
    L.check(lib.gget_op_raw_tok_grad(P(dx), P(flag), P(dtok.buf), T, i["e"], ST()))
    got = dtok.body().reshape(-1).numpy()
    finish("raw_tok_grad", f"T{T}", [R.same("dtok = dtok0 + flagged rows, exact", got, R.tokgrad_ref(i))])
