"""The mask twins, references and bounds of tests/_drop_ref.py, checked on the CPU with the inputs the GPU test uses (tests/test_gpu_drop.py):
the twins agree with the ones the whole-model tests use; an fp32 statement of every operation with the kernel's rounding points passes every
check on every listed case; no listed case leaves more than its share of elements where a flipped mask bit could hide; and one planted fault
at a time - a wrong coordinate convention, a wrong stream, a missing factor or rounding - is rejected by a named case."""
import importlib

import numpy as np
import pytest
import torch

import _drop_ref as D

modeling = importlib.import_module("graph-gpt_amd.modeling")
smtp = importlib.import_module("graph-gpt_amd.smtp")

ZERO_SHARE = ("out", "dsc", "x", "a")            # (every other bounded quantity: at most 1 %)


def params(cases):
    return [pytest.param(*args, id=name) for name, args in cases]


def passes(results):
    ratio, msgs = D.settle(results)
    assert not msgs, "\n".join(msgs)
    assert ratio < 1.0, ratio


def caught(results, where):
    msgs = D.settle(results)[1]
    assert msgs, "the planted fault went unnoticed"
    assert any(m.startswith(where) for m in msgs), (where, msgs)


def shares_hold(shares, case):
    for q, s in shares.items():
        assert s <= (0.0 if q in ZERO_SHARE else 0.01), f"{case}: {100 * s:.3f} % of {q} could not show a flipped mask bit"


def setting_is_sound(lay, m, em, keep):
    """A path setting keeps one sample and drops one; the threshold settings keep / drop the known element and nothing else differs."""
    if m["path_rate"] > 0 and len(np.unique(lay["sample"])) >= 2:
        assert bool((keep == 0).any()) and bool((keep != 0).any())
    if m["elem_p"] > 0:
        assert bool((em == 0).any()) and bool((em != 0).any())


# ------------------------------------------------------------------------------------------------------------------ the twins
def test_elem_twin_agrees_with_the_model_level_twin():
    seed, p = 777, 0.3
    for which, layer, stream, s in (("embed", 0, 48, seed ^ 0x5BD1E995), ("raw", 0, 60, seed ^ 0x5BD1E995), ("mlp_act", 2, 49, seed + 0x7F4A7C15 * 3),
                                    ("mlp_out", 1, 50, seed + 0x7F4A7C15 * 2), ("head", 1, 52, seed ^ 0x2545F491)):
        want = modeling.elem_drop_keep(seed, which, layer, 37, 72, p)
        got = D.elem_keep(s & 0xFFFFFFFF, stream, np.arange(37)[:, None], np.arange(72)[None, :], p)
        assert got.dtype == np.float32 and np.array_equal(got, want), which
        assert 0.2 < float((got == 0).mean()) < 0.4
    a, b = np.arange(5)[:, None] + 2 ** 32 - 2, np.arange(7)[None, :]          # (32-bit wrap of the coordinates)
    assert np.array_equal(D.elem_hash(9, 48, a, b).astype(np.int64), smtp._rng24(9, 48, a & 0xFFFFFFFF, b))
    assert bool((D.elem_keep(1, 49, a, b, 0.0) == 1).all())


def test_path_twin_agrees_with_the_model_level_twin():
    seed, B = 777, 64
    for layer, which, rate in ((0, 0, 0.5), (1, 1, 0.2), (3, 0, 0.07)):
        s = (seed ^ ((0xD6E8FEB8 * (layer * 2 + which + 1)) & 0xFFFFFFFF)) & 0xFFFFFFFF
        want = D.model_path_keep(seed, layer, which, B, rate)
        got = D.path_keep(s, np.arange(B), rate)
        assert got.dtype == np.float32 and np.array_equal(got, want.numpy().astype(np.float32))
        assert bool((got == 0).any()) and bool((got != 0).any())
    assert bool((D.path_keep(5, np.arange(9), 0.0) == 1).all())


def test_threshold_settings_sit_on_the_known_element():
    lay = D.layout("varlen")
    below, above = (D.setting(n, lay, 50, 123, D.ls_known(lay, 72)) for n in ("thresh-below", "thresh-above"))
    eb, ea = D.elem_mult(below, lay, 72), D.elem_mult(above, lay, 72)
    assert below["elem_seed"] == above["elem_seed"] and D.elem_thresh(above["elem_p"]) == D.elem_thresh(below["elem_p"]) + 1
    diff = ((eb == 0) != (ea == 0)).nonzero()
    assert diff.tolist() == [[D.VARLEN_T - 1, 69]] and float(eb[-1, 69]) != 0 and float(ea[-1, 69]) == 0


# ------------------------------------------------------------------------------------------------------------------ fp32 statements pass
@pytest.mark.parametrize("T,d,kind,names", params(D.LS_FWD_CASES + [D.LS_FWD_LONG] + D.UNFUSED_CASES + [D.UNFUSED_LONG]))
def test_layerscale_forward_statement_passes_and_sees_every_mask_bit(request, T, d, kind, names):
    for name in names:
        lay, m, em, keep = D.ls_masks(T, d, kind, name)
        setting_is_sound(lay, m, em, keep)
        i = D.ls_fwd_inputs(T, d, D.case_seed(T, d), lam=m["lam"])
        if T >= 3:
            assert not bool(i["y"][1].any()) and int((i["y"][2] != 0).sum()) == 1
        passes(D.ls_fwd_check(i, em, keep, m["path_rate"], *D.ls_fwd_fp32(i, em, keep)))
        shares_hold(D.ls_fwd_vacuous(i, m), f"{request.node.callspec.id} {name}")


@pytest.mark.parametrize("T,d,wide,kind,names", params(D.LS_BWD_CASES + [D.LS_BWD_LONG]))
def test_fused_backward_statement_passes_and_sees_every_mask_bit(request, T, d, wide, kind, names):
    for name in names:
        lay, m, em, keep = D.ls_masks(T, d, kind, name)
        setting_is_sound(lay, m, em, keep)
        i = D.ls_bwd_inputs(T, d, D.case_seed(T, d), 8, lam=m["lam"])
        dx, dw, dsc, dlam = D.ls_bwd_fp32(i, em, keep)
        passes(D.ls_bwd_check(i, em, keep, dx, dw, dsc, dlam))
        passes(D.dsc_pair_check(i, em, keep, dsc, D.scale_fp32(i, em, keep, dx)[0]))
        shares_hold(D.scale_vacuous(i, m, em, keep, dx), f"{request.node.callspec.id} {name}")


@pytest.mark.parametrize("T,d,kind,names", params(D.UNFUSED_CASES + [D.UNFUSED_LONG]))
def test_unfused_backward_statement_passes_and_sees_every_mask_bit(request, T, d, kind, names):
    for name in names:
        lay, m, em, keep = D.ls_masks(T, d, kind, name)
        i = D.ls_bwd_inputs(T, d, D.case_seed(T, d), 8, lam=m["lam"], fused=False)
        dsc, dlam = D.scale_fp32(i, em, keep, i["dy"])
        passes(D.scale_checks(i, em, keep, i["dy"], dsc, dlam))
        passes(D.scale_checks(i, em, keep, i["dy"], dsc, None))
        shares_hold(D.scale_vacuous(i, m, em, keep, i["dy"]), f"{request.node.callspec.id} {name}")


@pytest.mark.parametrize("T,n,stream,kind", params(D.DROP_CASES + [D.DROP_LONG]))
def test_elem_dropout_statement_passes_and_sees_every_mask_bit(request, T, n, stream, kind):
    for name in D.ELEM_SETTINGS if T < 1000 else ("elem",):
        lay, m, em = D.drop_masks(T, n, stream, kind, name)
        i = D.drop_inputs(T, n, D.case_seed(T, n))
        passes(D.drop_check(i, em, D.drop_fp32(i, em)))
        shares_hold(D.drop_vacuous(i, m), f"{request.node.callspec.id} {name}")
        if T * n >= 64:
            assert bool((em == 0).any()) and bool((i["x"][em == 0] < 0).any())       # (a negative zero is among the dropped)


@pytest.mark.parametrize("F,ldF,d,gated,kind", params(D.EMBED_CASES))
def test_embedding_statements_pass_and_see_every_mask_bit(request, F, ldF, d, gated, kind):
    for name in D.ELEM_SETTINGS:
        lay, m, em = D.embed_masks(F, d, kind, name)
        i = D.embed_inputs(lay["T"], F, ldF, d, gated, D.case_seed(F, d, gated))
        passes(D.embed_fwd_check(i, em, D.embed_fwd_fp32(i, em)))
        passes(D.embed_bwd_check(i, em, *D.embed_bwd_fp32(i, em)))
        case = f"{request.node.callspec.id} {name}"
        shares_hold(D.embed_fwd_vacuous(i, m), case)
        shares_hold(D.embed_bwd_vacuous(i, m, em), case)


@pytest.mark.parametrize("B,Din,Dout,layer", params(D.HEAD_CASES))
def test_head_statements_pass_and_see_every_mask_bit(request, B, Din, Dout, layer):
    for name in D.ELEM_SETTINGS:
        lay, m, em = D.head_masks(B, Din, layer, name)
        i = D.head_inputs(B, Din, Dout, D.case_seed(B, Din, Dout))
        a, y, y32 = D.head_fwd_fp32(i, em)
        passes(D.head_fwd_check(i, em, a, y, y32))
        passes(D.head_bwd_check(i, em, a, *D.head_bwd_fp32(i, em, a)))
        shares_hold(D.head_vacuous(i, m), f"{request.node.callspec.id} {name}")


# ------------------------------------------------------------------------------------------------------------------ planted faults
def ls_fault_masks(T, d, kind, name, fault):
    """em / keep as a kernel with one wrong coordinate convention would draw them."""
    lay, m, em, keep = D.ls_masks(T, d, kind, name)
    cols = np.arange(d)
    if fault == "compact-row":                  # the mask keyed by the compact row instead of rows[t]
        em = torch.from_numpy(D.elem_keep(m["elem_seed"], 50, np.arange(T)[:, None], cols[None, :], m["elem_p"]))
    elif fault == "keep-by-row":                # the path multiplier keyed by the row instead of the sample
        keep = torch.from_numpy(D.path_keep(m["path_seed"], np.arange(T), m["path_rate"]))
    elif fault == "no-row_b":                   # row_b ignored: sample = t / path_S
        keep = torch.from_numpy(D.path_keep(m["path_seed"], np.arange(T) // lay["S"], m["path_rate"]))
    elif fault == "no-p256":                    # the ls4 layout's column without its p * 256 term
        em = torch.from_numpy(D.elem_keep(m["elem_seed"], 50, lay["logical"][:, None], (cols % 256)[None, :], m["elem_p"]))
    elif fault == "c4":                         # column c * 4 + e instead of c * 8 + e
        em = torch.from_numpy(D.elem_keep(m["elem_seed"], 50, lay["logical"][:, None], (cols // 8 * 4 + cols % 8)[None, :], m["elem_p"]))
    elif fault == "stream-49":                  # the backward on stream 49 against the forward's 50
        em = torch.from_numpy(D.elem_keep(m["elem_seed"], 49, lay["logical"][:, None], cols[None, :], m["elem_p"]))
    elif fault == "no-inv-keep":
        em = (em != 0).float()
    elif fault == "le":                         # <= for < at the threshold
        h = D.elem_hash(m["elem_seed"], 50, lay["logical"][:, None], cols[None, :])
        em = torch.from_numpy(np.where(h <= D.elem_thresh(m["elem_p"]), np.float32(0), D.elem_inv(m["elem_p"])).astype(np.float32))
    return D.ls_masks(T, d, kind, name), em, keep


LS_FAULTS = [  # fault, (T, d, kind, setting), the check that rejects it in the forward, ... in the backward
    ("compact-row", (D.VARLEN_T, 768, "varlen", "elem"), "out is bf16", "dsc"),
    ("keep-by-row", (35, 768, "identity", "path"), "out", "dsc"),
    ("no-row_b", (D.VARLEN_T, 768, "varlen", "path"), "out", "dsc"),
    ("no-p256", (35, 768, "identity", "elem"), "out is bf16", "dsc"),
    ("c4", (35, 72, "identity", "elem"), "out is bf16", "dsc"),
    ("stream-49", (35, 768, "identity", "elem"), "out is bf16", "dsc"),
    ("no-inv-keep", (35, 768, "identity", "elem"), "out is bf16", "dsc"),
    ("le", (35, 768, "identity", "thresh-below"), "out is bf16", "dsc"),
]


@pytest.mark.parametrize("fault,case,fwd_check,bwd_check", [pytest.param(*f, id=f[0]) for f in LS_FAULTS])
def test_wrong_mask_conventions_are_rejected(fault, case, fwd_check, bwd_check):
    T, d, kind, name = case
    (lay, m, em, keep), em_f, keep_f = ls_fault_masks(T, d, kind, name, fault)
    i = D.ls_fwd_inputs(T, d, D.case_seed(T, d), lam=m["lam"])
    caught(D.ls_fwd_check(i, em, keep, m["path_rate"], *D.ls_fwd_fp32(i, em_f, keep_f)), fwd_check)
    b = D.ls_bwd_inputs(T, d, D.case_seed(T, d), 8, lam=m["lam"])
    caught(D.ls_bwd_check(b, em, keep, *D.ls_bwd_fp32(b, em_f, keep_f)), bwd_check)
    u = D.ls_bwd_inputs(T, d, D.case_seed(T, d), 8, lam=m["lam"], fused=False)
    caught(D.scale_checks(u, em, keep, u["dy"], *D.scale_fp32(u, em_f, keep_f, u["dy"])), bwd_check)
    if fault not in ("keep-by-row", "no-row_b", "no-p256"):
        x = D.drop_inputs(T, d, 5)
        caught(D.drop_check(x, em, D.drop_fp32(x, em_f)), "x is bf16")


def test_a_forward_on_one_stream_and_a_backward_on_another_disagree():
    """fwd on stream 50, bwd on stream 49: the gradient is wrong exactly where the two masks differ, and dsc's zero pattern shows it."""
    (lay, m, em, keep), em49, _ = ls_fault_masks(35, 768, "identity", "elem", "stream-49")
    b = D.ls_bwd_inputs(35, 768, 1, 8)
    assert 0.2 < float(((em == 0) != (em49 == 0)).float().mean()) < 0.45
    caught(D.ls_bwd_check(b, em, keep, *D.ls_bwd_fp32(b, em49, keep)), "dsc is +-0")


@pytest.mark.parametrize("fault,where", [("no-round", "out is bf16"), ("dlam-unmasked-y", "dlam"), ("dsc-no-keep", "dsc"), ("dsc-no-em", "dsc")])
def test_missing_factors_and_roundings_are_rejected(fault, where):
    T, d = 35, 768
    name = "elem" if fault in ("no-round", "dsc-no-em") else "both"
    lay, m, em, keep = D.ls_masks(T, d, "identity", name)
    if fault == "no-round":
        i = D.ls_fwd_inputs(T, d, D.case_seed(T, d))
        return caught(D.ls_fwd_check(i, em, keep, m["path_rate"], *D.ls_fwd_fp32(i, em, keep, fault=fault)), where)
    b = D.ls_bwd_inputs(T, d, D.case_seed(T, d), 8)
    caught(D.ls_bwd_check(b, em, keep, *D.ls_bwd_fp32(b, em, keep, fault=fault)), where)
    u = D.ls_bwd_inputs(T, d, D.case_seed(T, d), 8, fused=False)
    caught(D.scale_checks(u, em, keep, u["dy"], *D.scale_fp32(u, em, keep, u["dy"], fault=fault)), where)


@pytest.mark.parametrize("fault", ["cell-f-major", "after-sum"])
def test_embedding_mask_faults_are_rejected(fault):
    F, d, gated = 5, 64, True
    lay, m, em = D.embed_masks(F, d, "identity", "elem")
    i = D.embed_inputs(lay["T"], F, F + 3, d, gated, D.case_seed(F, d, gated))
    if fault == "after-sum":
        return caught(D.embed_fwd_check(i, em, D.embed_fwd_fp32(i, em, fault=fault)), "out (gated)")
    T = lay["T"]                                  # cell index f * T + t instead of t * F + f
    cell = np.arange(F)[None, :] * T + np.arange(T)[:, None]
    em_f = torch.from_numpy(D.elem_keep(m["elem_seed"], 48, cell[:, :, None], np.arange(d)[None, None, :], m["elem_p"]))
    caught(D.embed_fwd_check(i, em, D.embed_fwd_fp32(i, em_f)), "out (gated)")
    caught(D.embed_bwd_check(i, em, *D.embed_bwd_fp32(i, em_f)), "demb")
    caught(D.embed_bwd_check(i, em, *D.embed_bwd_fp32(i, em_f)), "dgate")


@pytest.mark.parametrize("fault,where", [("stream-without-layer", "a"), ("bwd-no-em", "dx")])
def test_head_mask_faults_are_rejected(fault, where):
    B, Din, Dout, layer = 7, 48, 32, 1
    lay, m, em = D.head_masks(B, Din, layer, "elem")
    i = D.head_inputs(B, Din, Dout, D.case_seed(B, Din, Dout))
    if fault == "stream-without-layer":
        em_f = D.elem_mult(m, lay, Din, stream=D.STREAM_HEAD)
        a, y, y32 = D.head_fwd_fp32(i, em_f)
        caught(D.head_fwd_check(i, em, a, y, y32), where)
        return caught(D.head_bwd_check(i, em, D.head_fwd_fp32(i, em)[0], *D.head_bwd_fp32(i, em_f, D.head_fwd_fp32(i, em)[0])), "dx")
    a = D.head_fwd_fp32(i, em)[0]
    caught(D.head_bwd_check(i, em, a, *D.head_bwd_fp32(i, em, a, fault="no-em")), where)
