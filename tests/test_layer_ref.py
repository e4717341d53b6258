"""The per-element bounds of tests/_layer_ref.py against a correct fp32 statement of the fused attention + o-projection kernels (inside,
on every case of the GPU table: the bounds are not too tight), against planted faults (rejected: they are not too loose) and against the
cap on vacuous bounds of tests/test_attn_out_ref.py.  Runs without a GPU."""
import functools

import pytest
import torch

import _attn_out_ref as A
import _heads_ref as H
import _layer_ref as Y
import _rows_ref as R
from test_attn_out_ref import VACUOUS_CAP

FWD, BWD, LIST, DET = Y.forward_cases(), Y.backward_cases(), Y.list_cases(), Y.det_cases()
ALL_BWD = BWD + LIST + DET


def test_case_table():
    ids = [c["id"] for c in FWD + ALL_BWD]
    assert len(set(ids)) == len(ids)
    for Hn in Y.HEADS:      # every K-step start (5 b) mod (d / 32) occurs, forward and backward
        for table in (FWD, BWD):
            assert any(c["Hn"] == Hn and {(5 * b) % (2 * Hn) for b in range(c["B"])} == set(range(2 * Hn)) for c in table)
    assert {c["copies"] - c["B"] for c in BWD} >= {3} and {c["copies"] for c in BWD} >= {1, 4}
    # one-tile samples under the dense K loop ("exact") and under a random weight ("sparse") for every H; the random dense weight where all are long
    assert all({"sparse", "exact"} <= {c["wkind"] for c in BWD if c["Hn"] == Hn and c["S"] == 32} for Hn in Y.HEADS)
    assert {c["Hn"] for c in BWD if c["wkind"] == "dense"} == {2, 12} and all(c["wkind"] == "dense" for c in FWD)
    long_last = [c["lens"][-1] > 32 for c in BWD if c["entry"] == "bwd_long"]
    assert True in long_last and False in long_last
    n_long = [sum(n > 32 for n in c["lens"]) for c in LIST]
    assert max(n_long) > Y.LONG_GRID > min(n_long) > 0
    assert max(c["B"] * c["S"] * c["Hn"] for c in FWD + ALL_BWD) <= 25 * 32 * 12


@functools.lru_cache(maxsize=None)
def layer(cid):
    return Y.Layer(next(c for c in FWD + ALL_BWD if c["id"] == cid))


@functools.lru_cache(maxsize=None)
def lse_of(cid):
    return A.forward_fp32(layer(cid).pr)[1]


def shares(case, tensors):
    """tensors: name -> (ref, bound, rows).  Prints every share, then asserts the cap."""
    got = {nm: A.vacuous_share(ref, bound, rows) for nm, (ref, bound, rows) in tensors.items()}
    print(f"{case}: share of vacuous bounds " + "  ".join(f"{nm} {s:.4f}" for nm, s in got.items()))
    assert max(got.values()) <= VACUOUS_CAP, f"{case}: bounds above 0.05 (|ref| + rms of the row): {got}"


def all_rows(t):
    return torch.ones(t.shape[:-1], dtype=torch.bool)


@pytest.mark.parametrize("c", FWD, ids=[c["id"] for c in FWD])
def test_fp32_forward_is_inside_the_bounds(c):
    ly = layer(c["id"])
    attn, lse, x_mid, xn, rstd = Y.forward_fp32(ly)
    f = A.forward64(ly.pr)
    res = Y.forward_check(ly, attn, lse, x_mid, xn, rstd, f)
    ratio = H.must_hold(res)
    print(f"{c['id']}: max err / bound = {ratio:.4f}  (" + "  ".join(f"{nm} {r:.3f}" for nm, r, _ in res if nm in Y.BOUNDED) + ")")
    assert ratio < 1.0
    ref, bound, y = Y.x_mid64(ly, attn)
    # ("cancelling": on |y|'s scale - x_mid is the small difference of x_in and y, module docstring of _layer_ref)
    scale = y if c["kind"] == "cancelling" else ref
    shares(c["id"], dict(out=(f["out"], f["out_bound"], ly.pr.real_h), lse=(f["lse"][..., None], f["lse_bound"][..., None], ly.pr.real_h),
                         x_mid=(scale, bound, all_rows(ref))))


@pytest.mark.parametrize("c", ALL_BWD, ids=[c["id"] for c in ALL_BWD])
def test_fp32_backward_is_inside_the_bounds(c):
    ly, lse = layer(c["id"]), lse_of(c["id"])
    dx_mid, dw, dattn_long, dqkv = Y.backward_fp32(ly, lse, det=c["det"])
    bw = Y.backward64(ly, lse, dx_mid, dattn_long)
    res = Y.backward_check(ly, lse, dx_mid, dw, dattn_long, dqkv, det=c["det"], bw=bw)
    ratio = H.must_hold(res)
    print(f"{c['id']}: max err / bound = {ratio:.4f}  (" + "  ".join(f"{nm} {r:.3f}" for nm, r, _ in res if nm in Y.BOUNDED) + ")")
    assert ratio < 1.0
    t = {nm: (bw["ref"][nm], bw["bound"][nm], ly.pr.real_h) for nm in ("dq", "dk", "dv")}
    ref, bound, _, _ = R.bwd_ref(ly.rows_inputs())
    t["dx_mid"] = (ref, bound, all_rows(ref))
    dref, dabs, cnt = Y.dw64(ly, c["det"])
    dw_ref = ly.dw0.double() + dref
    t["dw"] = (dw_ref, 2 * (cnt[:, None] + 1) * Y.U * (ly.dw0.double().abs() + dabs) + Y.TINY, all_rows(dw_ref))
    lr = ly.long_rows()
    if bool(lr.any()):
        exact, eps = Y.dattn64(ly, dx_mid)
        t["dattn_long"] = (exact[lr], Y.BF * exact[lr].abs() + 1.01 * eps[lr] + Y.TINY, all_rows(exact[lr]))
    shares(c["id"], t)


def test_e_do_defaults_leave_backward64_as_it_was():
    """backward64 with dO = the problem's own dout and e_dO = 0 is backward64 without them, bit for bit."""
    pr = A.Problem(3, 32, 2, lens=(32, 17, 1), p=0.1, rope="memory")
    out, lse = A.forward_fp32(pr)
    a = A.backward64(pr, lse, out, False)
    b = A.backward64(pr, lse, out, False, dO=pr.dout, e_dO=torch.zeros(3, 2, 32, 64, dtype=torch.float64))
    for nm in ("dq", "dk", "dv"):
        assert torch.equal(a["ref"][nm], b["ref"][nm]) and torch.equal(a["bound"][nm], b["bound"][nm])


# ------------------------------------------------------------------------------------------------------------------ planted faults
def pick(table, **want):
    return next(c for c in table if all(c[k] == v for k, v in want.items()))


# fault -> the case that must reject it
FAULTS = {
    "x_mid_twice": pick(FWD, Hn=2, kind="cancelling"),
    "ss_unrounded": pick(FWD, Hn=2, kind="unit", varlen=False),
    "k_step_twice": pick(FWD, Hn=2, kind="unit", varlen=True),          # KSTEPS = PD = 4: every start but 0 wraps
    "residual_neighbour": pick(FWD, Hn=4, kind="unit", varlen=True),
    "dw_no_permutation": pick(BWD, Hn=2, varlen=False, copies=1, S=32),
    "dw_rows_past_len": pick(BWD, Hn=4, varlen=True, copies=4),
    "dw_replica0": pick(BWD, Hn=8, varlen=True, copies=4),
    "dx_no_dres": pick(BWD, Hn=2, varlen=True, copies=4),
    "dattn_unrounded": pick(BWD, Hn=2, S=8),
    "tail_not_zeroed": pick(BWD, entry="bwd_long", Hn=12, S=64),
    "list_skips_items": pick(LIST, B=70),
    "dq_rot_forward": pick(BWD, Hn=12, varlen=True, copies=4),
}


def test_every_planted_fault_has_its_case():
    assert tuple(FAULTS) == Y.FWD_FAULTS + Y.BWD_FAULTS
    assert "dq_rot_forward" in A.BWD_FAULTS
    assert FAULTS["tail_not_zeroed"]["lens"][-1] > 32 and FAULTS["dq_rot_forward"]["rope"] and FAULTS["list_skips_items"]["listed"]
    ly = layer(FAULTS["k_step_twice"]["id"])
    b = Y.wrapping_sample(ly)
    assert (5 * b) % (ly.d // 32) + Y.PD > ly.d // 32


@functools.lru_cache(maxsize=None)
def planted(fault):
    """(rejected, texts) of a planted fault on its case; the clean statement must pass there."""
    c = FAULTS[fault]
    ly = layer(c["id"])
    if fault in Y.FWD_FAULTS:
        good, bad = Y.forward_fp32(ly), Y.forward_fp32(ly, fault)
        H.must_hold(Y.forward_check(ly, *good))
        msgs = H.settle(Y.forward_check(ly, *bad))[1]
    else:
        lse = lse_of(c["id"])
        good, bad = Y.backward_fp32(ly, lse, listed=c["listed"]), Y.backward_fp32(ly, lse, fault, listed=c["listed"])
        H.must_hold(Y.backward_check(ly, lse, *good))
        msgs = H.settle(Y.backward_check(ly, lse, *bad))[1]
    assert not all(torch.equal(g.view(torch.int16 if g.dtype == torch.bfloat16 else torch.int32),
                               b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)) for g, b in zip(good, bad)), \
        "the fault changes nothing on this case"
    return bool(msgs), msgs


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_is_rejected(fault):
    rejected, msgs = planted(fault)
    first = msgs[0].splitlines()[0] if msgs else "-"
    print(f"{fault} on {FAULTS[fault]['id']}: per-element rejected {rejected}: {first}")
    assert rejected, "the planted fault went unnoticed"


def test_table_of_faults_and_their_cases(capsys):
    lines = [f"  {f:22s}{FAULTS[f]['id']:75s}{'rejects' if planted(f)[0] else 'passes':>8s}   {(planted(f)[1] or ['-'])[0].splitlines()[0][:90]}"
             for f in FAULTS]
    with capsys.disabled():
        print("\nplanted faults of the fused attention + o-projection kernels and the case that rejects each\n" + "\n".join(lines))
