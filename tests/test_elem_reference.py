"""The references and bounds of tests/_elem_ref.py, checked on the CPU with the inputs the GPU test uses (tests/test_gpu_elem.py): an fp32
statement of every operation with the kernel's rounding points stays inside its per-element bound (ratio < 1), and one planted fault at
a time - a tanh GELU, a GELU' without its x phi(x) term, a flipped sine on one chunk, the neighbouring token's position, a feature left out,
a pad row that is added to, an accumulator row overwritten, the cut runs of the sorted sum lost, a slab left out, an unrounded ratio - does
not; every fault names the check that rejects it."""
import pytest
import torch

import _elem_ref as E


def params(cases):
    return [pytest.param(*args, id=name) for name, args in cases]


def passes(results):
    ratio, msgs = E.settle(results)
    assert not msgs, "\n".join(msgs)
    assert ratio < 1.0, ratio
    return ratio


def caught(results, where):
    msgs = E.settle(results)[1]
    assert msgs, "the planted fault went unnoticed"
    assert any(m.startswith(where) for m in msgs), (where, msgs)


# ------------------------------------------------------------------------------------------------------------------ GEGLU
def test_the_cdf_budget_is_what_the_docstring_says():
    got = E.cdf_budget()
    for k in ("K_T", "K_H", "K_C", "K_A", "K_G"):
        assert got[k] <= getattr(E, k) <= 1.05 * got[k], (k, got[k], getattr(E, k))
    assert 6.9e-8 < got["AS_EPS"] <= E.AS_EPS == 7.5e-8          # (the published bound, not the grid's figure)
    assert abs(E.C_CDF - (7.5e-8 + 13.999 * E.U)) < 1e-12
    # the emulation with an exact reciprocal and exp2 over every finite bf16 value: max |g cdf - gelu(g)| / |g|
    g = E.bf16_patterns(65536).float()
    g = g[g != 0]
    val = (g * E.gelu_parts_fp32(g)[0]).double()
    ref = g.double() * 0.5 * torch.special.erfc(-g.double() * E.SQRT1_2)
    worst = float(((val - ref).abs() / g.double().abs()).max())
    print(f"derived C_CDF {E.C_CDF:.3e}, emulation maximum {worst:.3e}")
    assert 1e-7 < worst < E.C_CDF


@pytest.mark.parametrize("T,ff,variants", params(E.GEGLU_CASES))
def test_geglu_fp32_statement_is_inside_the_bounds(T, ff, variants):
    for v in range(variants):
        i = E.geglu_inputs(T, ff, v)
        assert E.covers_every_finite_pattern(i)
        passes(E.geglu_fwd_check(i, E.geglu_fwd_fp32(i)) + E.geglu_bwd_check(i, E.geglu_bwd_fp32(i)))
    up = i["gu"][:, ff:].float()
    assert float(up.min()) < -2 and float(up.max()) > 2 and bool((up == 0).any()) and float(up[up != 0].abs().min()) < 1e-20


def test_planted_faults_in_geglu_are_caught():
    i = E.geglu_inputs(911, 72, 0)
    caught(E.geglu_fwd_check(i, E.geglu_fwd_fp32(i, tanh=True)), "h:")                           # tanh-approximation GELU
    caught(E.geglu_bwd_check(i, E.geglu_bwd_fp32(i, drop_x_phi=True)), "dg:")                    # GELU' = Phi alone
    swapped = E.geglu_bwd_fp32(i)
    caught(E.geglu_bwd_check(i, torch.cat([swapped[:, 72:], swapped[:, :72]], dim=1)), "du:")    # dg and du in each other's columns
    # the tanh form against the bound, where it is worst: the factor the issue quotes
    ref, bound = E.geglu_ref(i)["h"]
    ratio = float(((E.geglu_fwd_fp32(i, tanh=True).double() - ref).abs() / bound).max())
    assert ratio > 10, ratio


# ------------------------------------------------------------------------------------------------------------------ RoPE
@pytest.mark.parametrize("B,S,H,max_pos,positions", params(E.ROPE_CASES + [E.ROPE_BIG]))
def test_rope_fp32_statement_is_inside_the_bounds(B, S, H, max_pos, positions):
    i = E.rope_case(B, S, H, max_pos, positions)
    if positions:
        p = i["pos"]
        assert int(p.max()) == max_pos - 1 and int(p.min()) == 0 and int(p[2]) == int(p[3])
    y = E.rope_fp32(i, 0)
    passes(E.rope_check(i, 0, y))
    if B * S > 10000:
        return
    passes(E.rope_check(i, 1, E.rope_fp32(i, 1)))
    passes(E.rope_roundtrip_check(i, y, E.rope_fp32(i, 1, x=y)))


def test_planted_faults_in_rope_are_caught():
    i = E.rope_case(3, 40, 3, 64, True)
    for k in range(4):
        caught(E.rope_check(i, 0, E.rope_fp32(i, 0, flip_chunk=k)), "q|k")                       # sin flipped on one 8-wide chunk
    caught(E.rope_check(i, 0, E.rope_fp32(i, 0, neighbour=True)), "q|k")                         # the neighbouring token's position
    j = E.rope_case(3, 40, 3, 64, False)
    caught(E.rope_check(j, 1, E.rope_fp32(j, 1, neighbour=True)), "q|k")
    y = E.rope_fp32(i, 0)
    caught(E.rope_roundtrip_check(i, y, E.rope_fp32(i, 0, x=y)), "inverse(")                     # the inverse pass rotates forward again
    v = y.clone()
    v[5, 2 * 64 * 3 + 7] = 0
    caught(E.rope_check(i, 0, v), "the v third")


@pytest.mark.parametrize("max_pos", E.TABLE_SIZES)
def test_rope_table_fp32_statement_is_inside_the_bounds(max_pos):
    passes(E.table_check(*E.table_fp32(max_pos, E.THETA), max_pos, E.THETA))


def test_planted_faults_in_the_rope_tables_are_caught():
    caught(E.table_check(*E.table_fp32(64, E.THETA, neighbour_freq=True), 64, E.THETA), "cos table")     # inv_freq of j - 1
    cos, sin = E.table_fp32(64, E.THETA)
    caught(E.table_check(sin, cos, 64, E.THETA), "sin table")                                           # the two tables swapped
    caught(E.table_check(cos.roll(1, 0), sin.roll(1, 0), 64, E.THETA), "cos table, j = 0")              # one position off
    # pos / powf(...) in place of pos * (1 / powf(...)): inside the bound (docstring), so it is no planted fault
    inv_pow = E.c32(E.THETA) ** (torch.arange(0, 64, 2, dtype=torch.float32) / 64)
    fr = (torch.arange(2048, dtype=torch.float32)[:, None] / inv_pow[None, :]).double()
    passes(E.table_check(fr.cos().float(), fr.sin().float(), 2048, E.THETA))
    i = E.range_inputs(5, 40, 3)
    caught(E.range_check(i, *E.range_fp32(i, max_of_neighbour=True)), "cos range table")                # the row maximum of another row
    c, s, ids = E.range_fp32(i)
    caught(E.range_check(i, c, s, ids.roll(1)), "ids")


@pytest.mark.parametrize("B,S", params(E.RANGE_CASES))
def test_rope_range_table_fp32_statement_is_inside_the_bounds(B, S):
    i = E.range_inputs(B, S, seed=B + S)
    assert not bool(i["pos"][0].any()) and int(i["pos"][1].argmax()) == 0 and int(i["pos"][2].argmax()) == S - 1
    passes(E.range_check(i, *E.range_fp32(i)))


def test_clamp_positions_statement():
    for clamped in (False, True):
        for flag0 in (0, 1):
            pos = E.clamp_inputs(1000, 64, clamped, 5)
            passes(E.clamp_check(pos, 64, flag0, pos.clamp(0, 63), 1 if (clamped or flag0) else 0))
    pos = E.clamp_inputs(1000, 64, True, 5)
    caught(E.clamp_check(pos, 64, 0, pos.clamp(0, 63), 0), "flag")
    caught(E.clamp_check(pos, 64, 0, pos.clamp(0, 64), 1), "clamped positions")
    caught(E.clamp_check(E.clamp_inputs(1000, 64, False, 5), 64, 0, pos.clamp(0, 63), 1), "flag")       # set although nothing was clamped


# ------------------------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("T,F,ldF,d,V,gated", params(E.EMBED_FWD_CASES))
def test_embedding_forward_fp32_statement_is_inside_the_bounds(T, F, ldF, d, V, gated):
    i = E.embed_fwd_case(T, F, ldF, d, V, gated)
    assert not bool(i["ids"][0, :F].any()) and bool((i["ids"][:, F:] == V - 1).all())
    passes(E.embed_fwd_check(i, E.embed_fwd_fp32(i)))


def test_planted_faults_in_the_embedding_forward_are_caught():
    for F, gated, where in ((5, False, "out is bf16"), (13, True, "out (gated)"), (1, False, "out is bf16")):
        i = E.embed_fwd_case(37, F, F + 3, 64, 211, gated)
        caught(E.embed_fwd_check(i, E.embed_fwd_fp32(i, skip_last=True)), where)                        # the last feature left out
        wide = dict(i, F=F + 1)                                                                        # a gap column read into the sum
        if not gated:
            caught(E.embed_fwd_check(i, E.embed_fwd_fp32(wide)), where)
    i = E.long_inputs(23, 13, 15, 64, 1)
    caught(E.long_check(i, E.long_fp32(i, round_ratio=False)[0]), "x is bf16(")                         # the reciprocal not rounded to bf16
    x = E.long_fp32(i)[0].clone()
    x[0] = (x[0].float() * 0.5).to(E.BF)
    caught(E.long_check(i, x), "rows with ratio 1")


@pytest.mark.parametrize("T,F,ldF,d", params(E.LONG_CASES))
def test_long_ratio_statement(T, F, ldF, d):
    i = E.long_inputs(T, F, ldF, d, seed=T + F + d)
    assert sorted(set(i["nnz"].tolist())) == sorted({0, 1, 2, 3, F})
    passes(E.long_check(i, E.long_fp32(i)[0]))


@pytest.mark.parametrize("T,F,ldF,d,V,pad_id,gated,layout", params(E.EMBED_SORTED_CASES))
def test_embedding_backward_sorted_fp32_statement_is_inside_the_bounds(T, F, ldF, d, V, pad_id, gated, layout):
    i = E.embed_bwd_case(T, F, ldF, d, V, pad_id, gated, layout)
    assert T * F > E.HIST_CELLS and (T * F) % E.SEG
    paths = E.run_paths(i)
    if layout == "pad-only":
        assert paths["inside"] == 0 and paths["cut"] == 0
    else:
        assert paths["inside"] > 50 and paths["cut"] >= 2 and paths["ends_on_boundary"] and paths["whole_segments"] >= 3, paths
    if layout == "waves":
        lanes = (i["ids"][:, :F].reshape(-1)[:(T * F) // 64 * 64].view(-1, 64) == 1).sum(1)
        assert int((lanes == 60).sum()) >= 20 and int((lanes == 0).sum()) >= 100
    passes(E.embed_bwd_check(i, *E.embed_bwd_sorted_fp32(i)))


@pytest.mark.parametrize("T,F,ldF,d,V,pad_id,gated,layout", params(E.EMBED_BOTH_CASES))
def test_embedding_backward_both_forms_fp32_statement_is_inside_the_bounds(T, F, ldF, d, V, pad_id, gated, layout):
    i = E.embed_bwd_case(T, F, ldF, d, V, pad_id, gated, layout)
    passes(E.embed_bwd_check(i, *E.embed_bwd_dense_fp32(i), dense=True))
    passes(E.embed_bwd_check(i, *E.embed_bwd_sorted_fp32(i)))


def test_the_dense_cases_reach_the_slab_edges():
    plans = {T: E.dense_plan(T, 97, 64) for T in (37, 777, 2100)}
    assert plans[37] == (1, 1, 1, 1) and plans[777] == (13, 3, 5, 3) and plans[2100] == (33, 8, 5, 7)
    assert E.dense_plan(2100, 756, 768) == (33, 7, 5, 7)


def test_planted_faults_in_the_embedding_backward_are_caught():
    i = E.embed_bwd_case(331, 13, 15, 64, 97, 0, True, "random")
    caught(E.embed_bwd_check(i, *E.embed_bwd_sorted_fp32(i, fault="pad")), "the pad-id row")            # the pad row is added to
    caught(E.embed_bwd_check(i, *E.embed_bwd_sorted_fp32(i, fault="overwrite")), "demb")                # a row overwritten, demb0 lost
    caught(E.embed_bwd_check(i, *E.embed_bwd_sorted_fp32(i, fault="lose-cut")), "demb")                 # the cut runs' later parts lost
    demb, dgate = E.embed_bwd_sorted_fp32(i)
    caught(E.embed_bwd_check(i, demb, dgate - i["dgate0"]), "dgate")                                    # dgate0 overwritten
    k = E.embed_bwd_case(331, 13, 15, 64, 1500, 0, False, "random")
    caught(E.embed_bwd_check(k, *E.embed_bwd_sorted_fp32(dict(k, F=14))), "the pad-id row")             # a gap column summed (into row V - 1)
    j = E.embed_bwd_case(2100, 13, 15, 64, 97, 0, False, "random")
    caught(E.embed_bwd_check(j, *E.embed_bwd_dense_fp32(j, drop_last_slab=True), dense=True), "demb")   # the last slab left out
    caught(E.embed_bwd_check(j, E.embed_bwd_dense_fp32(j)[0] - j["demb0"], None, dense=True), "demb")   # the dense form overwrites
