"""The integer machinery of a pre-training step - the padding-free token layout (k_lengths, k_sum_lengths, k_varlen_plan, k_rows_to_grid,
k_ranges_from_mask3d), the SMTP head's compaction, slot sort and scatter (k_head_compact, k_head_slot_sort, k_head_cell_sum, k_gather_rows,
k_gather_rows_remap), the indexed GEMM that feeds the sorted head and the small row-selection kernels (k_sample_mask_wgt, k_raw_blend,
k_raw_tok_grad): seeded inputs, plain numpy statements of every operation written from the contract in include/gget.h, and the checks
that hold an implementation to them.  tests/test_gpu_plan.py feeds the checks with the HIP kernels' outputs, tests/test_plan_reference.py
with the statements' own outputs (which must pass) and with planted faults (which must not).

Everything here is integer-exact or bit for bit; there is no tolerance.  Output buffers start from a sentinel (tests/_gpu_out.py: UNW in an
integer buffer, SENT16 in a bf16 one) and the expected arrays carry the sentinel wherever the contract says "not written",
so one comparison covers the values and the untouched entries.  Where the kernel leaves an order free (the position of a cell inside its
slot comes from atomics) the check is the invariant, not one array.  bf16 arrays travel as numpy uint16 bit patterns.

A finding is (name, 0.0 or inf, failure text or None), as in tests/_heads_ref.py."""
import numpy as np
import torch

from _gpu_out import SENT16
from _util import exact_operands, gemm_expected

UNW = -7          # what tests/_gpu_out.py Out leaves in an integer buffer nobody wrote
INF = float("inf")
I32, I64, U16, F32 = np.int32, np.int64, np.uint16, np.float32


# ------------------------------------------------------------------------------------------------------------------ findings
def same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return name, INF, f"{name}: shape {got.shape}, want {want.shape}"
    bad = got != want
    if not bad.any():
        return name, 0.0, None
    at = tuple(int(x) for x in np.argwhere(bad)[0])
    return name, INF, f"{name}: {int(bad.sum())} of {bad.size} entries differ, the first at {at}: got {got[at]!r} want {want[at]!r}"


def true(name, ok, text):
    return name, 0.0 if ok else INF, None if ok else f"{name}: {text}"


def settle(results):
    return max([r for _, r, _ in results], default=0.0), [m for _, _, m in results if m is not None]


def names_failed(results):
    return [n for n, _, m in results if m is not None]


# ------------------------------------------------------------------------------------------------------------------ bf16 as bits
def bits_of(t):
    """torch bf16 tensor -> uint16 bit patterns."""
    return t.contiguous().view(torch.int16).numpy().view(U16).copy()


def bf16_of(bits):
    """uint16 bit patterns -> torch bf16 tensor (CPU)."""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def f32_of_bits(bits):
    return (np.asarray(bits, U16).astype(np.uint32) << 16).view(F32)


def rne_bits(a32):
    """fp32 -> bf16 bit patterns, round to nearest even."""
    return bits_of(torch.from_numpy(np.ascontiguousarray(a32, dtype=F32)).to(torch.bfloat16))


def randn_bits(rng, rows, cols, spread=0):
    a = rng.standard_normal((rows, cols)).astype(F32)
    if spread:
        a = a * np.exp2(rng.integers(-spread, spread + 1, (rows, 1))).astype(F32)
    return rne_bits(a)


def sent_rows(rows, cols):
    return np.full((rows, cols), SENT16, U16)


# ------------------------------------------------------------------------------------------------------------------ lengths
LENGTHS_S = [1, 63, 64, 65, 200]
LENGTHS_PAD = 3


def lengths_inputs(S):
    """Six samples: full, right-padded, a mask with holes (and non-zeros other than 1), all-pad, one token, random."""
    rng = np.random.default_rng(100 + S)
    B, ldF = 6, 3
    mask = np.zeros((B, S), I64)
    ids = np.full((B, S, ldF), LENGTHS_PAD, I64)
    ln = [S, max(S * 2 // 3, 1), S, 0, 1, int(rng.integers(0, S + 1))]
    for b in range(B):
        mask[b, :ln[b]] = 1
        ids[b, :ln[b], 0] = rng.integers(LENGTHS_PAD + 1, 900, ln[b])
    mask[2] = rng.integers(0, 2, S) * rng.choice(np.array([1, 2, -1, 1 << 40], I64), S)
    ids[..., 1:] = rng.integers(0, 900, (B, S, ldF - 1))      # (the other features are not looked at: some of them ARE the pad id)
    ids[1, 0, 1] = LENGTHS_PAD
    return dict(B=B, S=S, ldF=ldF, pad_id=LENGTHS_PAD, mask=mask, ids=ids)


def lengths_ref(i, with_mask):
    B, S = i["B"], i["S"]
    key_len = np.count_nonzero(i["mask"], axis=1) if with_mask else np.full(B, S)
    real = np.count_nonzero(i["ids"][:, :, 0] != i["pad_id"], axis=1)
    pool_row = np.arange(B) * S + np.where(real > 0, real - 1, S - 1)
    return key_len.astype(I32), pool_row.astype(I32)


def lengths_check(i, with_mask, key_len, pool_row):
    k, p = lengths_ref(i, with_mask)
    return [same("key_len", key_len, k), same("pool_row", pool_row, p)]


SUM_B = [1, 1024, 1025, 5000]


def sum_inputs(B):
    return np.random.default_rng(200 + B).integers(0, 201, B).astype(I32)


# ------------------------------------------------------------------------------------------------------------------ varlen_plan
VARLEN_VARIANTS = [
    dict(name="tc == sum, t_rows == tc, pos / pool_row NULL, long_list", extra=0, pos=False, pool=False, long=True, round=False, tc="sum"),
    dict(name="tc == sum, t_rows rounded to 64, ldF > F, pos, pool_row, long_list NULL", extra=2, pos=True, pool=True, long=False, round=True,
         tc="sum"),
    dict(name="tc < sum", extra=1, pos=True, pool=True, long=True, round=True, tc="less"),
    dict(name="tc > sum", extra=0, pos=False, pool=True, long=True, round=True, tc="more"),
]


def _big_lens(B, S, seed):
    return np.random.default_rng(seed).integers(0, S + 1, B)


def _long_lens(B, S, seed):
    """Mostly 0 .. 3 rows, and samples of 33 .. 64 rows in every 1024-sample pass of the scan (at its first and last sample too)."""
    ln = np.random.default_rng(seed).integers(0, 4, B)
    for b, v in ((0, 33), (5, 40), (1023, 64), (1024, 34), (1500, 32), (1501, 65), (2047, 50), (2048, 33)):
        ln[b] = v
    return ln


# name -> (B, S, F, list of length vectors)
VARLEN_CASES = {
    "B3-S72": (3, 72, 2, [np.array([0, 1, 32]), np.array([33, 64, 65]), np.array([72, 33, 0])]),
    "B1024-S8": (1024, 8, 1, [_big_lens(1024, 8, 1)]),
    "B1025-S8": (1025, 8, 1, [_big_lens(1025, 8, 2)]),
    "B2049-S4": (2049, 4, 1, [_big_lens(2049, 4, 3)]),
    "B2049-S66-long-samples-in-every-pass": (2049, 66, 1, [_long_lens(2049, 66, 4)]),
}
VARLEN_PAD = 2


def varlen_inputs(case, k, v):
    """Length vector k of `case` under variant v of VARLEN_VARIANTS."""
    B, S, F, lens = VARLEN_CASES[case]
    var = VARLEN_VARIANTS[v]
    ln = lens[k].astype(I32)
    rng = np.random.default_rng(1000 * v + 10 * k + B)
    ldF = F + var["extra"]
    ids = rng.integers(3, 1 << 40, (B, S, ldF)).astype(I64)        # (ids wider than 32 bits: a narrowing copy shows)
    pos = rng.integers(0, 5000, (B, S)).astype(I64) if var["pos"] else None
    total = int(ln.sum())
    if var["tc"] == "sum":
        tc = total
    elif var["tc"] == "more":
        tc = total + 5
    elif B <= 3:      # inside the last non-empty sample
        last = int(np.flatnonzero(ln)[-1])
        tc = total - 1 - int(ln[last]) // 2
    else:             # many samples cut away, one of them partly
        tc = total * 3 // 5
    t_rows = (tc + 63) // 64 * 64 if var["round"] else tc
    pool = None
    if var["pool"]:   # the row k_lengths would give: the last real token, or the last grid row of an empty sample; one row past the length
        p = np.where(ln > 0, ln - 1, S - 1)
        p[B // 2] = S - 1
        pool = (np.arange(B) * S + p).astype(I32)
    return dict(B=B, S=S, F=F, ldF=ldF, ids=ids, pos=pos, key_len=ln, pool_row=pool, tc=tc, t_rows=t_rows, pad_id=VARLEN_PAD,
                long=var["long"], total=total)


def varlen_ref(i):
    """Sample b owns the compact rows [first_b, first_b + len_b) clipped to [0, tc); rows [tc, t_rows) are pad tokens."""
    B, S, F, tc, t_rows = i["B"], i["S"], i["F"], i["tc"], i["t_rows"]
    ln = i["key_len"].astype(np.int64)
    first = np.concatenate([[0], np.cumsum(ln)])
    total = int(first[B])
    start, end = np.minimum(first[:B], tc), np.minimum(first[1:], tc)
    new = end - start
    o = dict(key_len=new.astype(I32), cu=np.append(start, min(total, tc)).astype(I32),
             ids_c=np.full((t_rows, F), UNW, I64), pos_c=np.full(t_rows, UNW, I64), row_b=np.full(t_rows, UNW, I32),
             c2p=np.full(t_rows, UNW, I32), pad2c=np.full((B, S), -1, I32))
    for b in range(B):
        n, r = int(new[b]), int(start[b])
        if n == 0:
            continue
        o["ids_c"][r:r + n] = i["ids"][b, :n, :F]
        o["pos_c"][r:r + n] = i["pos"][b, :n] if i["pos"] is not None else np.arange(n)
        o["row_b"][r:r + n] = b
        o["c2p"][r:r + n] = b * S + np.arange(n)
        o["pad2c"][b, :n] = r + np.arange(n)
    o["ids_c"][tc:] = i["pad_id"]
    o["pos_c"][tc:] = 0
    o["row_b"][tc:] = 0
    o["c2p"][tc:] = B * S + np.arange(t_rows - tc)
    o["pad2c"] = o["pad2c"].reshape(-1)
    if i["pool_row"] is not None:
        p = i["pool_row"].astype(np.int64) - np.arange(B) * S
        moved = start + np.clip(p, 0, np.maximum(new - 1, 0))
        o["pool_row"] = np.minimum(moved, max(tc - 1, 0)).astype(I32)
    if i["long"]:
        sel = np.flatnonzero((new > 32) & (new <= 64))
        ll = np.full(3 * B + 1, UNW, I32)
        ll[0] = len(sel)
        ll[1:1 + len(sel)] = sel
        ll[1 + B:1 + B + len(sel)] = start[sel]
        ll[1 + 2 * B:1 + 2 * B + len(sel)] = new[sel]
        o["long_list"] = ll
    o["status"] = np.array([int(total != tc), UNW, 1 if total != tc else UNW], I32)
    return o


def varlen_check(i, got):
    """got: the arrays named as in varlen_ref, each the whole buffer (sentinels where nothing was written)."""
    w = varlen_ref(i)
    tc = i["tc"]
    res = [same("cu", got["cu"], w["cu"]), same("key_len", got["key_len"], w["key_len"]), same("pad2c", got["pad2c"], w["pad2c"]),
           same("status", got["status"], w["status"])]
    for k in ("ids_c", "pos_c", "row_b", "c2p"):
        res.append(same(k, got[k][:tc], w[k][:tc]))
        res.append(same(f"tail rows ({k})", got[k][tc:], w[k][tc:]))
    if "pool_row" in w:
        res.append(same("pool_row", got["pool_row"], w["pool_row"]))
    if "long_list" in w:
        res.append(same("long_list", got["long_list"], w["long_list"]))
    return res


# ------------------------------------------------------------------------------------------------------------------ rows_to_grid, ranges
GRID_D = [8, 192]


def grid_inputs(d):
    rng = np.random.default_rng(300 + d)
    rows, n_pos = 41, 70
    pad2c = np.full(n_pos, -1, I32)
    at = 1 + rng.permutation(n_pos - 1)[:rows]          # (position 0 holds no token)
    pad2c[at] = rng.permutation(rows)
    return dict(d=d, n_pos=n_pos, src=randn_bits(rng, rows, d), pad2c=pad2c)


def grid_ref(i):
    out = np.zeros((i["n_pos"], i["d"]), U16)
    on = i["pad2c"] >= 0
    out[on] = i["src"][i["pad2c"][on]]
    return out


RANGES_S = [1, 64, 65, 130]


def ranges_inputs(S):
    """Two [S,S] masks whose rows cycle through: all zero, a single one, first and last with zeros between, the last column alone, a
    random run."""
    rng = np.random.default_rng(400 + S)
    m = np.zeros((2, S, S), I64)
    for b in range(2):
        for r in range(S):
            kind = (r + b) % 5
            if kind == 0:
                continue                                   # all zero
            if kind == 1:
                m[b, r, rng.integers(0, S)] = 1            # a single one
            elif kind == 2:
                lo, hi = sorted(rng.integers(0, S, 2))
                m[b, r, lo], m[b, r, hi] = 1, 7            # first and last, zeros between
            elif kind == 3:
                m[b, r, S - 1] = 1                         # the last column alone
            else:
                lo, hi = sorted(rng.integers(0, S, 2))
                m[b, r, lo:hi + 1] = rng.integers(0, 2, hi + 1 - lo)
                m[b, r, lo], m[b, r, hi] = 1, 1
    return dict(B=2, S=S, mask=m)


def ranges_ref(i):
    m = i["mask"] != 0
    S = i["S"]
    anyone = m.any(-1)
    lo = np.where(anyone, m.argmax(-1), 0)
    hi = np.where(anyone, S - 1 - m[..., ::-1].argmax(-1), -1)
    return lo.astype(I32).reshape(-1), hi.astype(I32).reshape(-1)


# ------------------------------------------------------------------------------------------------------------------ head_compact
COMPACT_T = [1, 255, 256, 257, 1000]
COMPACT_N = [1, 13, 32, 33]
COMPACT_PATTERNS = ["labels NULL", "all -100", "none -100", "half", "last token only"]


def compact_labels(T, n, pattern, seed=0):
    rng = np.random.default_rng(500 + 7 * T + n + seed)
    lab = rng.integers(0, 700, (T, n)).astype(I64)
    if pattern == "labels NULL":
        return None
    if pattern == "all -100":
        lab[:] = -100
    elif pattern == "half":
        lab[rng.random((T, n)) < 0.5] = -100
    elif pattern == "last token only":
        lab[:T - 1] = -100
    else:
        assert pattern == "none -100"
    return lab


def compact_ref(lab, T, n, hist0=None):
    """Selected tokens and labelled cells in (token, slot) order.  Whole buffers: row_idx [T], sel_* [T n], UNW behind M / Lm."""
    sel = np.ones((T, n), bool) if lab is None else lab != -100
    cnt = sel.sum(1)
    tok = cnt > 0
    t_of, f_of = np.nonzero(sel)                     # (row-major: token after token, slot after slot)
    M, Lm = int(tok.sum()), len(t_of)
    m_off = np.cumsum(tok) - tok
    o = dict(cnt=cnt, m_off=m_off, l_off=np.cumsum(cnt) - cnt, counts=np.array([M, Lm]), row_idx=np.full(T, UNW), sel_src=np.full(T * n, UNW),
             sel_label=np.full(T * n, UNW), sel_tok=np.full(T * n, UNW))
    o["row_idx"][:M] = np.flatnonzero(tok)
    o["sel_src"][:Lm] = m_off[t_of] * n + f_of
    o["sel_label"][:Lm] = 0 if lab is None else lab[t_of, f_of]
    o["sel_tok"][:Lm] = t_of
    if hist0 is not None:
        o["slot_hist"] = hist0 + np.bincount(f_of, minlength=len(hist0))[:len(hist0)] if n <= 32 else hist0.copy()
    return {k: np.asarray(v).astype(I32) for k, v in o.items()}


def compact_check(lab, T, n, got, hist0=None):
    w = compact_ref(lab, T, n, hist0)
    return [same(k, got[k], w[k]) for k in w]


# ------------------------------------------------------------------------------------------------------------------ head_slot_sort
SLOT_ELEMS = 192 * 192
# name -> (T, n, tile_rows, two label recipes run one after the other through ONE slot_state)
SORT_CASES = {
    "Lm<1024-empty-slot": (60, 13, 128, [dict(p=0.5, empty=5), dict(p=0.3)]),
    "Lm>4096-slot-of-exactly-128": (700, 13, 128, [dict(p=0.5, exact=2), dict(p=0.6, empty=0)]),
    "Lm>4096-tile-256-slot-of-exactly-256": (700, 13, 256, [dict(p=0.55, exact=3, empty=7), dict(p=0.5)]),
    "Lm=0-then-cells": (40, 4, 128, [dict(p=0.0), dict(p=0.5)]),
    "n32-cells-then-Lm=0": (300, 32, 256, [dict(p=0.5, exact=31), dict(p=0.0)]),
    "n1": (1500, 1, 128, [dict(p=0.7), dict(p=0.2)]),
}


def sort_labels(T, n, tile_rows, recipe, seed):
    rng = np.random.default_rng(600 + seed + T + n)
    lab = rng.integers(0, 700, (T, n)).astype(I64)
    lab[rng.random((T, n)) >= recipe["p"]] = -100
    if recipe.get("exact") is not None:
        f = recipe["exact"]
        lab[:, f] = -100
        lab[rng.permutation(T)[:tile_rows], f] = 9
    if recipe.get("empty") is not None:
        lab[:, recipe["empty"]] = -100
    return lab


def sort_inputs(T, n, tile_rows, lab):
    """What k_head_compact hands to the sort (here from compact_ref; the GPU test takes the kernel's own output)."""
    c = compact_ref(lab, T, n, np.zeros(n, I32))
    Lm = int(c["counts"][1])
    return dict(T=T, n=n, tile_rows=tile_rows, cap=T * n, slot_elems=SLOT_ELEMS, Lm=Lm, sel_src=c["sel_src"], row_idx=c["row_idx"],
                cells=c["slot_hist"].astype(np.int64), compact=c)


def sort_plan(i):
    """(padded slot starts [n + 1], cells per slot)."""
    tr = i["tile_rows"]
    padded = (i["cells"] + tr - 1) // tr * tr
    return np.concatenate([[0], np.cumsum(padded)]), i["cells"]


def sort_any_order(i, rng=None):
    """One output that satisfies the contract: cells of a slot in l order, or shuffled inside their slot when rng is given."""
    n, Lm, tr, cap = i["n"], i["Lm"], i["tile_rows"], i["cap"]
    start, cells = sort_plan(i)
    size = cap + n * tr
    o = dict(a_tok=np.full(size, UNW, I32), a_cell=np.full(size, UNW, I32), c_l=np.full(size, UNW, I32), cellpos=np.full(cap, UNW, I32),
             tile_off=np.full(size // tr + 1, UNW, I32), total=np.array([start[n]], I32), slot_state=np.zeros(3 * n + 2, I32))
    src = i["sel_src"][:Lm].astype(np.int64)
    for f in range(n):
        ls = np.flatnonzero(src % n == f)
        if rng is not None:
            ls = rng.permutation(ls)
        p = start[f] + np.arange(len(ls))
        o["a_cell"][p], o["a_tok"][p], o["c_l"][p] = src[ls], i["row_idx"][src[ls] // n], ls
        o["cellpos"][ls] = p
        pad = np.arange(start[f] + cells[f], start[f + 1])
        o["a_cell"][pad], o["a_tok"][pad], o["c_l"][pad] = 0, 0, -1
        o["tile_off"][start[f] // tr:start[f + 1] // tr] = f * i["slot_elems"]
    o["slot_state"][2 * n:3 * n + 1] = start
    return o


def sort_check(i, got):
    """The invariants of the slot sort (include/gget.h gget_op_head_slot_sort); got: whole buffers as in sort_any_order."""
    n, Lm, tr = i["n"], i["Lm"], i["tile_rows"]
    start, cells = sort_plan(i)
    total = int(start[n])
    src = i["sel_src"][:Lm].astype(np.int64)
    a_tok, a_cell, c_l, cellpos = (np.asarray(got[k]).astype(np.int64) for k in ("a_tok", "a_cell", "c_l", "cellpos"))
    is_cell = np.zeros(total, bool)
    slot_ok, slot_msg = True, ""
    for f in range(n):
        lo, hi = int(start[f]), int(start[f] + cells[f])
        is_cell[lo:hi] = True
        want = np.sort(src[src % n == f])
        have = np.sort(a_cell[lo:hi])
        if slot_ok and not np.array_equal(want, have):
            slot_ok, slot_msg = False, f"slot {f}: positions [{lo}, {hi}) do not hold exactly the slot's {len(want)} cells, each once"
    cp, pp = np.flatnonzero(is_cell), np.flatnonzero(~is_cell)
    res = [same("total and padded starts", np.append(got["total"], got["slot_state"][2 * n:3 * n + 1]), np.append(total, start).astype(I32)),
           true("every slot's range holds exactly its cells", slot_ok, slot_msg)]
    l_ok = bool(((c_l[cp] >= 0) & (c_l[cp] < Lm)).all())
    res.append(true("c_l names a cell", l_ok, "a cell position carries a c_l outside [0, Lm)"))
    if l_ok:
        res += [same("a_cell[p] == sel_src[c_l[p]]", a_cell[cp], src[c_l[cp]]), same("cellpos[c_l[p]] == p", cellpos[c_l[cp]], cp)]
    in_rows = bool(((a_cell[cp] >= 0) & (a_cell[cp] // n < len(i["row_idx"]))).all())
    res.append(true("a_cell names a selected row", in_rows, "a cell position carries an a_cell outside the selected rows"))
    if in_rows:
        res.append(same("a_tok[p] == row_idx[a_cell[p] / n]", a_tok[cp], i["row_idx"].astype(np.int64)[a_cell[cp] // n]))
    res += [same("pad rows: a_tok = 0", a_tok[pp], np.zeros(len(pp), np.int64)), same("pad rows: a_cell = 0", a_cell[pp], np.zeros(len(pp), np.int64)),
            same("pad rows: c_l = -1", c_l[pp], np.full(len(pp), -1, np.int64))]
    tiles = np.repeat(np.arange(n), (start[1:] - start[:-1]) // tr) * i["slot_elems"]
    res.append(same("tile_off[t] == f * slot_elems", np.asarray(got["tile_off"])[:len(tiles)], tiles.astype(I32)))
    res.append(true("counts, cursors and ticket are zero after the launch",
                    not np.asarray(got["slot_state"])[:2 * n].any() and got["slot_state"][3 * n + 1] == 0,
                    f"slot_state[0, 2n) = {np.asarray(got['slot_state'])[:2 * n].tolist()}, ticket {got['slot_state'][3 * n + 1]}"))
    behind = [np.asarray(got[k])[total:] for k in ("a_tok", "a_cell", "c_l")] + [np.asarray(got["cellpos"])[Lm:], np.asarray(got["tile_off"])[len(tiles):]]
    res.append(true("nothing written behind the padded total / Lm", all((b == UNW).all() for b in behind), "an entry behind the lists was written"))
    return res


# ------------------------------------------------------------------------------------------------------------------ gather_rows
GATHER_D = [8, 192, 576]
GATHER_CAP = 20
GATHER_COUNTS = [13, 20, 29]          # < cap, == cap, > cap


def gather_inputs(d, count, scatter):
    rng = np.random.default_rng(700 + d + count + scatter)
    rows = 37                                                   # rows of the indexed side
    idx = (rng.permutation(rows)[:GATHER_CAP] if scatter else rng.integers(0, rows, GATHER_CAP)).astype(I32)
    if not scatter:
        idx[1], idx[2] = idx[0], rows - 1                       # (a repeat, the last row)
    elif rows - 1 not in idx:
        idx[2] = rows - 1
    src_rows = GATHER_CAP if scatter else rows
    return dict(d=d, cap=GATHER_CAP, count=count, scatter=scatter, idx=idx, src=randn_bits(rng, src_rows, d),
                dst_rows=rows if scatter else GATHER_CAP)


def gather_ref(i):
    n = min(i["cap"], i["count"])
    out = sent_rows(i["dst_rows"], i["d"])
    if i["scatter"]:
        out[i["idx"][:n]] = i["src"][:n]
    else:
        out[:n] = i["src"][i["idx"][:n]]
    return out


def gather_check(i, dst):
    w = gather_ref(i)
    n = min(i["cap"], i["count"])
    wr = np.zeros(i["dst_rows"], bool)
    wr[i["idx"][:n] if i["scatter"] else np.arange(n)] = True
    return [same("rows moved", dst[wr], w[wr]), same("rows at or behind count stay untouched", dst[~wr], w[~wr])]


REMAP_VARIANTS = ["a -1 and status", "no -1 and status", "a -1 and status NULL"]


def remap_inputs(d, count, variant):
    rng = np.random.default_rng(800 + d + count + len(variant))
    grid, rows = 50, 31                       # padded positions, compact rows (pad_row = the row behind them)
    pad2c = np.full(grid, -1, I32)
    pad2c[np.sort(rng.permutation(grid)[:rows - 1])] = np.arange(rows - 1)
    on, off = np.flatnonzero(pad2c >= 0), np.flatnonzero(pad2c < 0)
    idx = np.sort(rng.permutation(on)[:GATHER_CAP]).astype(I32)
    if variant != "no -1 and status":
        idx[4] = off[0]
        idx = np.sort(idx)
    return dict(d=d, cap=GATHER_CAP, count=count, idx=idx, pad2c=pad2c, pad_row=rows - 1, src=randn_bits(rng, rows, d),
                status=variant != "a -1 and status NULL")


def remap_ref(i):
    n = min(i["cap"], i["count"])
    r = i["pad2c"][i["idx"]]
    miss = r < 0
    r = np.where(miss, i["pad_row"], r)
    idx = i["idx"].copy()
    idx[:n] = r[:n]
    dst = sent_rows(i["cap"], i["d"])
    dst[:n] = i["src"][r[:n]]
    status = np.array([UNW, UNW, 1 if miss[:n].any() else UNW], I32)
    return idx, dst, status


def remap_check(i, idx, dst, status):
    w_idx, w_dst, w_status = remap_ref(i)
    res = [same("idx rewritten in place", idx, w_idx), same("rows gathered, rows at or behind count untouched", dst, w_dst)]
    if i["status"]:
        res.append(same("status", status, w_status))
    return res


# ------------------------------------------------------------------------------------------------------------------ head_cell_sum
CELLSUM_D = [192, 576, 768, 1152]
CELLSUM_COUNTS = [0, 1, 3, 4, 5, 13, 32]


def cellsum_inputs(d, with_pad2c):
    """23 tokens (six blocks of four waves) whose cell counts run through CELLSUM_COUNTS; the cells' rows of dxs are scattered, of widely
    different magnitudes (fp32 sums that round, so the order of the additions shows) and surrounded by rows nobody may read."""
    rng = np.random.default_rng(900 + d + with_pad2c)
    TP = 23
    cnt = np.array([CELLSUM_COUNTS[(3 * t + 1) % len(CELLSUM_COUNTS)] for t in range(TP)], I32)
    l_off = (np.cumsum(cnt) - cnt).astype(I32)
    Lm = int(cnt.sum())
    P = Lm + 9
    cellpos = rng.permutation(P)[:Lm].astype(I32)
    dxs = randn_bits(rng, P, d, spread=9)
    # a token whose result depends on the order: ((1 + 2^-8) + 2^-24) + 2^-24 stays on bf16's tie in fp32 and rounds to 1, while
    # ((2^-24 + 2^-24) + 2^-8) + 1 is exact in fp32, lies above the tie and rounds to 1 + 2^-7
    t4 = int(np.flatnonzero(cnt == 4)[0])
    for j, v in enumerate((1.0, 2.0 ** -8, 2.0 ** -24, 2.0 ** -24)):
        dxs[cellpos[l_off[t4] + j]] = rne_bits(np.full(d, v, F32))
    pad2c, pad_row, rows = None, 0, TP
    if with_pad2c:
        pad2c = rng.permutation(TP).astype(I32)
        lost = int(np.flatnonzero(cnt == 13)[0])
        pad2c[pad2c > pad2c[lost]] -= 1
        pad2c[lost] = -1
        pad_row, rows = TP - 1, TP
    return dict(d=d, TP=TP, cnt=cnt, l_off=l_off, cellpos=cellpos, dxs=dxs, pad2c=pad2c, pad_row=pad_row, rows=rows)


def cellsum_row(i, t):
    return t if i["pad2c"] is None else (int(i["pad2c"][t]) if i["pad2c"][t] >= 0 else i["pad_row"])


def cellsum_ref(i):
    """fp32 sum in cell order, one RNE rounding; rows of tokens without cells keep the sentinel."""
    out = sent_rows(i["rows"], i["d"])
    x = f32_of_bits(i["dxs"])
    for t in range(i["TP"]):
        c = int(i["cnt"][t])
        if c == 0:
            continue
        acc = np.zeros(i["d"], F32)
        for j in range(c):
            acc = (acc + x[i["cellpos"][i["l_off"][t] + j]]).astype(F32)
        out[cellsum_row(i, t)] = rne_bits(acc)
    return out


def cellsum_check(i, dhid):
    w = cellsum_ref(i)
    wr = np.zeros(i["rows"], bool)
    for t in range(i["TP"]):
        if i["cnt"][t]:
            wr[cellsum_row(i, t)] = True
    return [same("token rows: fp32 sum in cell order, one rounding", dhid[wr], w[wr]),
            same("rows of tokens without cells keep their sentinel", dhid[~wr], w[~wr])]


# ------------------------------------------------------------------------------------------------------------------ gemm_indexed
NT, NN = 0, 1
# name -> (mode, N, K, b_tile_rows passed, cells per slot, m_dev kind, exact)
GEMM_CASES = {}
for _mode, _mn in ((NT, "NT"), (NN, "NN")):
    for _m in ("zero", "tile", "cap"):
        GEMM_CASES[f"{_mn}-192-tile128-slots(130,0,128)-m_dev-{_m}"] = (_mode, 192, 192, 128, [130, 0, 128], _m, True)
    GEMM_CASES[f"{_mn}-768-tile128"] = (_mode, 768, 768, 128, [100, 129, 0, 1], "cap", True)
    GEMM_CASES[f"{_mn}-768-tile256"] = (_mode, 768, 768, 256, [257, 0, 256, 3], "cap", True)
    GEMM_CASES[f"{_mn}-576-tile256-falls-back-to-128"] = (_mode, 576, 576, 256, [130, 256, 5], "cap", True)
    GEMM_CASES[f"{_mn}-192-300-tiles"] = (_mode, 192, 192, 128, [100 * 128 - 3, 128 * 100, 128 * 99 + 1], "cap", True)
    GEMM_CASES[f"{_mn}-192-random-normal"] = (_mode, 192, 192, 128, [130, 0, 128], "cap", False)
GEMM_A_ROWS = 48


def gemm_tile(N, passed):
    """The row-tile height the launcher runs: 256 x 256 tiles need N % 256 == 0."""
    return 256 if passed == 256 and N % 256 == 0 else 128


def gemm_inputs(name):
    mode, N, K, passed, cells, m_kind, exact = GEMM_CASES[name]
    seed = 11 + sorted(GEMM_CASES).index(name)
    rng = np.random.default_rng(seed)
    tr = gemm_tile(N, passed)
    cells = np.array(cells)
    padded = (cells + tr - 1) // tr * tr
    start = np.concatenate([[0], np.cumsum(padded)])
    total, ncell, ns = int(start[-1]), int(cells.sum()), len(cells)
    m_cap = total + 256
    if exact:
        ops = [exact_operands(GEMM_A_ROWS, N, K, seed * 100 + f, mode=mode) for f in range(ns)]
        A, Bs = ops[0][0], [o[1] for o in ops]
    else:
        g = torch.Generator().manual_seed(seed)
        A = torch.randn(GEMM_A_ROWS, K, generator=g).to(torch.bfloat16)
        Bs = [(torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16) for _ in range(ns)]     # (NT: [N,K]; NN: the same bits read as [K,N], N == K)
        assert N == K
    a_rows, c_rows = np.zeros(m_cap, I32), np.full(m_cap, -1, I32)
    slot_of = np.full(m_cap, -1)
    dest = rng.permutation(ncell + 5)[:ncell]                     # rows of C, 5 of them never targeted
    k = 0
    for f in range(ns):
        p = np.arange(start[f], start[f] + cells[f])
        a_rows[p] = rng.integers(0, GEMM_A_ROWS, len(p))          # (repeats: far more cells than rows of A)
        c_rows[p] = dest[k:k + len(p)]
        slot_of[start[f]:start[f + 1]] = f
        k += len(p)
    drop = np.flatnonzero(c_rows >= 0)[::17]                      # real cells that are not stored either
    c_rows[drop] = -1 - (drop % 3)
    tile_off = np.repeat(np.arange(ns), padded // tr).astype(I32) * (N * K)
    m_dev = {"zero": 0, "tile": tr, "cap": total}[m_kind]
    return dict(mode=mode, N=N, K=K, passed=passed, tile=tr, M_cap=m_cap, m_dev=m_dev, A=bits_of(A), B=np.concatenate([bits_of(b) for b in Bs]),
                a_rows=a_rows, c_rows=c_rows, tile_off=tile_off, slot_of=slot_of, c_total=ncell + 5, exact=exact, ns=ns, total=total, cells=cells)


def _slot_B(i, f):
    rows = i["N"] if i["mode"] == NT else i["K"]
    return bf16_of(i["B"][f * rows:(f + 1) * rows])


def gemm_stored(i):
    """(product rows m that are stored, their rows of C)."""
    m = np.arange(i["m_dev"])
    m = m[i["c_rows"][m] >= 0]
    return m, i["c_rows"][m]


def gemm_ref_exact(i):
    """C bit for bit: row c_rows[m] = bf16_rne(A[a_rows[m]] . W of the tile's slot) for the stored rows below m_dev, the sentinel elsewhere."""
    out = sent_rows(i["c_total"], i["N"])
    A = bf16_of(i["A"])
    prod = [bits_of(gemm_expected(i["mode"], A, _slot_B(i, f))[0]) for f in range(i["ns"])]      # (rows of the product are independent)
    m, dst = gemm_stored(i)
    for f in range(i["ns"]):
        on = i["slot_of"][m] == f
        out[dst[on]] = prod[f][i["a_rows"][m[on]]]
    return out


def gemm_check_exact(i, C):
    w = gemm_ref_exact(i)
    wr = np.zeros(i["c_total"], bool)
    wr[gemm_stored(i)[1]] = True
    return [same("stored rows, bit for bit", C[wr], w[wr]), same("unstored rows and rows behind m_dev keep their sentinel", C[~wr], w[~wr])]


def gemm_ref64(i):
    """(rows of C, fp64 reference, fp64 |A| |B|) of the stored rows."""
    A = bf16_of(i["A"]).double()
    m, dst = gemm_stored(i)
    ref, ab = torch.zeros(len(m), i["N"], dtype=torch.float64), torch.zeros(len(m), i["N"], dtype=torch.float64)
    for f in range(i["ns"]):
        on = torch.from_numpy(i["slot_of"][m] == f)
        b = _slot_B(i, f).double()
        b = b.t() if i["mode"] == NT else b
        a = A[torch.from_numpy(i["a_rows"][m].astype(np.int64))][on]
        ref[on], ab[on] = a @ b, a.abs() @ b.abs()
    return dst, ref, ab


PLAIN = dict(mode=NN, M=200, N=192, K=128, m_dev=150)


def plain_inputs():
    rng = np.random.default_rng(77)
    A, B, _ = exact_operands(PLAIN["M"], PLAIN["N"], PLAIN["K"], 77, mode=NN)
    c_rows = rng.permutation(PLAIN["M"] + 6)[:PLAIN["M"]].astype(I32)
    c_rows[::13] = -2
    return dict(PLAIN, A=bits_of(A), B=bits_of(B), c_rows=c_rows, c_total=PLAIN["M"] + 6)


def plain_ref(i):
    out = sent_rows(i["c_total"], i["N"])
    prod = bits_of(gemm_expected(NN, bf16_of(i["A"]), bf16_of(i["B"]))[0])
    m = np.arange(i["m_dev"])
    m = m[i["c_rows"][m] >= 0]
    out[i["c_rows"][m]] = prod[m]
    return out


# ------------------------------------------------------------------------------------------------------------------ row selection
WGT_CELLS = [1, 255, 257, 3000]


def wgt_inputs(cells):
    rng = np.random.default_rng(1100 + cells)
    lab = rng.integers(0, 700, (5, cells)).astype(I64)
    lab[0] = -100                                    # a sample without a labelled cell
    lab[2][rng.random(cells) < 0.5] = -100
    lab[3][:cells - 1] = -100
    lab[4][0] = -100
    return lab


def wgt_ref(lab):
    tot = np.count_nonzero(lab != -100, axis=1)
    return (F32(1) / (tot.astype(F32) + F32(1e-7))).astype(F32)


BLEND_E = [8, 100]


def blend_inputs(e, first_only, with_labels, with_map):
    rng = np.random.default_rng(1200 + e + 2 * first_only + 4 * with_labels + 8 * with_map)
    L, n = 11, 3                                     # logical rows, labels per row
    raw = rng.standard_normal((L, e)).astype(F32)
    # bf16 rounding ties: a bf16 value plus exactly half a unit in its last place (even and odd last bits), and just off the tie
    base = f32_of_bits(rne_bits(raw[1])).view(np.uint32)
    raw[1] = (base | 0x8000).view(F32)
    raw[2] = ((base + 0x10000) | 0x8000).view(F32)
    raw[3] = (base | 0x8001).view(F32)
    raw[4] = (base | 0x7FFF).view(F32)
    lab = None
    if with_labels:
        lab = rng.integers(0, 700, (L, n)).astype(I64)
        lab[0] = -100
        lab[1, 0] = -100                             # the first unset: raw under both rules
        lab[2, 1] = -100                             # the first set, another unset: the two rules differ
        lab[5, 2] = -100
    rows_map, T, n_logical = None, L, L
    if with_map:
        rows_map = np.concatenate([rng.permutation(L)[:8], [L, L + 3, 2 * L]]).astype(I32)
        T = len(rows_map)
    tok = rne_bits(rng.standard_normal((1, e)).astype(F32))[0]
    return dict(e=e, n=n, T=T, first_only=first_only, raw=raw, labels=lab, rows_map=rows_map, n_logical=n_logical, tok=tok)


def blend_ref(i):
    T, e = i["T"], i["e"]
    lt = np.arange(T) if i["rows_map"] is None else i["rows_map"]
    out, flag = np.zeros((T, e), U16), np.zeros(T, I32)
    cast = rne_bits(i["raw"])
    for t in range(T):
        if lt[t] >= i["n_logical"]:
            continue
        lab = None if i["labels"] is None else i["labels"][lt[t]]
        masked = lab is not None and bool(((lab[:1] if i["first_only"] else lab) != -100).all())
        flag[t] = int(masked)
        out[t] = i["tok"] if masked else cast[lt[t]]
    return out, flag


TOKGRAD_T = [1, 256, 257, 700]


def tokgrad_inputs(T):
    """Small integers times 2^-3: every partial sum is exact in fp32, whatever the order of the atomics."""
    rng = np.random.default_rng(1300 + T)
    e = 100
    dx = (rng.integers(-8, 9, (T, e)) * 0.125).astype(F32)
    flag = (rng.random(T) < 0.6).astype(I32) * rng.integers(1, 4, T).astype(I32)       # (any non-zero flag counts)
    flag[0] = 1
    dtok0 = (rng.integers(-40, 41, e) * 0.125).astype(F32)
    return dict(T=T, e=e, dx=rne_bits(dx), flag=flag, dtok0=dtok0)


def tokgrad_ref(i):
    x = f32_of_bits(i["dx"]).astype(np.float64)
    s = i["dtok0"].astype(np.float64) + x[i["flag"] != 0].sum(0)
    assert np.array_equal(s.astype(F32).astype(np.float64), s)
    return s.astype(F32)
