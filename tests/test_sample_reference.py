"""The statement, bounds, inputs and checks of tests/_sample_ref.py, checked on the CPU with the cases the GPU test uses
(tests/test_gpu_sample.py): the draws are the twins the generation loop already has; the pinned seeds draw what they promise; a numpy
float32 twin of token_sample_kernel / token_confidence_kernel, with the kernels' operation order per lane, passes every check on every
case; no case leaves more than its share of rows where a wrong kept set or a wrong candidate could hide; and each of 22 planted faults - and a 23rd, the kernel's own V = 1
margin before it was fixed - is rejected by a named case."""
import importlib

import numpy as np
import pytest

import _sample_ref as S

gen = importlib.import_module("graph-gpt_amd.generation")
smtp = importlib.import_module("graph-gpt_amd.smtp")


def passes(results):
    ratio, msgs = S.settle(results)
    assert not msgs, "\n".join(msgs)
    assert ratio < 1.0, ratio


def caught(results, where):
    msgs = S.settle(results)[1]
    assert msgs, "the planted fault went unnoticed"
    assert any(m.startswith(where) for m in msgs), (where, msgs)


# ------------------------------------------------------------------------------------------------------------------ draws and seeds
def test_draws_are_the_generation_loops_twins():
    seed, it, B, N = 4242, 3, 7, 37
    u_cat, u_gum, _ = gen.draws(seed, it, B, N)
    s = gen.iteration_seed(seed, it)
    assert np.array_equal(S.draw(s, 32, B * N), u_cat.numpy()) and np.array_equal(S.draw(s, 33, B * N), u_gum.numpy())
    assert S.draw(s, 32, B * N).dtype == np.float32 and 0.0 <= float(S.draw(s, 32, B * N).min()) and float(S.draw(s, 32, B * N).max()) < 1.0


@pytest.mark.parametrize("key", [k for k, c in S.CASES.items() if c["pin"]])
def test_pinned_seeds_draw_what_they_promise(key):
    i = S.inputs(key)
    stream, who, u24 = i["pin"]
    row = i["names"].index(who)
    assert int(smtp._rng24(i["seed"], stream, row, 0)) == u24
    assert float(S.draw(i["seed"], stream, i["R"])[row]) == (0.0 if u24 == 0 else 1.0 - 2.0 ** -24)
    for stream, row, u24 in ((32, 0, 0), (33, 5, S.U24_MAX), (32, 8194, 12345), (33, 32772, 1)):
        assert int(smtp._rng24(S.seed_for(stream, row, u24), stream, row, 0)) == u24


# ------------------------------------------------------------------------------------------------------------------ the cases themselves
def test_the_cases_cover_what_they_are_there_for():
    C = S.CASES
    assert {c["V"] for c in C.values()} == {1, 2, 63, 64, 65, 128, 300, 1024, 1025, 8192}
    assert all(c["ld"] == c["V"] for c in C.values() if c["V"] in (65, 1025)) and all(c["ld"] % 64 == 0 for c in C.values() if c["V"] not in (65, 1025))
    assert all(c["R"] == 8 for c in C.values() if c["V"] == 8192)
    assert any(c["V"] == 64 and c["R"] == 4 * 8192 + 5 for c in C.values()) and any(c["V"] == 1025 and c["R"] == 8192 + 3 for c in C.values())
    for V in (1, 2, 63, 64, 65, 128, 300, 1024, 1025):
        mine = {c["R"] for c in C.values() if c["V"] == V}
        assert 259 in mine and len(mine) >= 2, V                     # (all the named rows, and fewer rows than one block has waves)
    assert {c["R"] for c in C.values()} >= {1, 3, 8, 259}
    for on_p in (False, True):
        for on_k in (False, True):
            mine = [c for c in C.values() if (0 < c["top_p"] < 1) == on_p and (c["top_k"] > 0) == on_k]
            assert {c["mode"] for c in mine} == {0, 1, 2}, (on_p, on_k)
            for mode in range(3):
                sub = [c for c in mine if c["mode"] == mode]
                assert {c["T"] > 0 for c in sub} == {False, True} and {c["alg"] > 0 for c in sub} == {False, True}, (on_p, on_k, mode)
    assert any(c["top_k"] == 1 for c in C.values()) and any(c["top_k"] == c["V"] for c in C.values()) and any(c["top_k"] > c["V"] for c in C.values())
    assert any(c["top_p"] == 1e-6 for c in C.values()) and any(abs(c["T"] - 0.05) < 1e-6 for c in C.values()) and any(c["T"] == 50.0 for c in C.values())
    assert all(c["V"] <= 128 for c in list(C.values()) + list(S.CONF_CASES.values()) if c["rows"] == "gaussian")
    assert {(c["V"], c["R"]) for c in S.CONF_CASES.values()} == {(V, R) for V in (2, 63, 64, 65, 97, 41245) for R in (1, 3, 259)} | {(64, 4 * 4096 + 5)}
    assert all(c["ld"] == 41280 for c in S.CONF_CASES.values() if c["V"] == 41245)


def test_every_named_row_appears_where_it_can():
    names = set(S.inputs("pk-mode0-T1-V300-R259")["names"]) - {None}
    assert names == {"all-equal", "tie-at-k", "tie-at-p", "top2-lane", "top2-lane-swapped", "top2-ends", "top2-ends-swapped", "max-last", "head-past-70", "tail-past"} | {
        f"top2-xor-{j}{sw}" for j in range(6) for sw in ("", "-swapped")}
    i = S.inputs("pk-mode0-T1-V300-R259")
    r = S.reference("pk-mode0-T1-V300-R259")
    kept = r["alive"].sum(1)
    row = {n: i["names"].index(n) for n in names}
    assert kept[row["tie-at-k"]] == i["top_k"] + 1                                   # (k + 1 tokens survive the tie at k)
    tied = np.nonzero(i["x"][row["tie-at-p"]] == 4.0)[0]
    alive = r["alive"][row["tie-at-p"]]
    assert len(tied) == 10 and alive[tied[:9]].all() and not alive[tied[9]] and alive.sum() == 9      # (the lower indices survive)
    assert not r["alive"][row["head-past-70"], :70].any() and not r["alive"][row["tail-past"], -70:].any()
    x = i["x"][row["top2-lane"]]
    a, b = np.argsort(-x, kind="stable")[:2]
    assert abs(int(a) - int(b)) == 64
    for j in range(6):
        a, b = np.argsort(-i["x"][row[f"top2-xor-{j}"]], kind="stable")[:2]
        assert int(a) ^ int(b) == 1 << j
    assert int(np.argmax(i["x"][row["max-last"]])) == i["V"] - 1
    # one survivor at top_p = 1e-6: the margin is p1 itself and the entropy lies within its bound of 0
    for key in ("topp1e-6-V300-mode1", "topp1e-6-V65-mode2"):
        r = S.reference(key)
        assert (r["alive"].sum(1) == 1).all() and (r["P1"] == 1.0).all() and (r["P2"] == 0.0).all() and (np.abs(r["ent"]) <= r["ent_b"]).all()
    # T = 0.05: probabilities below FLT_MIN among the survivors; T = 50: a flat row
    r = S.reference("T0.05-V128-mode2")
    assert ((r["P"] < S.FLT_MIN) & r["alive"]).any()
    r = S.reference("T50-V65-mode2")
    assert float((r["P"].max(1) / r["P"].min(1)).max()) < 100.0
    # the exact-mass case: top_p IS the mass ahead of token V / 2 of an all-equal row, which stays
    r = S.reference("exact-mass-V64")
    assert (r["alive"].sum(1) == 33).all() and not r["amb"].any()


@pytest.mark.parametrize("key", [k for k, c in S.CASES.items() if c["R"] >= 259 and c["top_p"] == S.TOP_P and c["T"] <= 16 and c["rows"] == "structured"])
def test_filtered_cases_keep_one_a_few_and_many_tokens(key):
    kept = S.kept_counts(key)
    assert (kept == 1).any() and ((kept >= 2) & (kept <= 8)).any() and (kept > 8).any()


# ------------------------------------------------------------------------------------------------------------------ the twin passes
@pytest.mark.parametrize("key", list(S.CASES))
def test_twin_passes_and_the_shares_hold(key):
    S.shares_hold(key)
    i = S.inputs(key)
    assert np.isnan(i["xpad"][:, i["V"]:]).all() and (i["ld"] == i["V"] or i["xpad"].shape[1] > i["V"])
    passes(S.check(key, *S.twin(key)))


@pytest.mark.parametrize("key", list(S.CONF_CASES))
def test_confidence_twin_passes(key):
    for mode in range(3):
        conf, tok = S.conf_twin(key, mode)
        passes(S.conf_check(key, mode, conf, tok))
    # token_sample at T = 0 without filters and noise computes the same thing another way
    if S.CONF_CASES[key]["V"] <= 8192:
        for mode in range(3):
            _, conf, tok = S.twin(key, mode=mode)
            c2, t2 = S.conf_twin(key, mode)
            assert np.array_equal(tok, t2)
            passes([S.conf_pair_check(key, mode, conf, c2)])


def test_confidence_faults_are_rejected():
    caught(S.conf_check("conf-V64-R259", 0, *S.conf_twin("conf-V64-R259", 0, fault=13)), "token_confidence tok")
    caught(S.conf_check("conf-V97-R259", 1, *S.conf_twin("conf-V97-R259", 1, fault=14)), "token_confidence conf")
    caught(S.conf_check("conf-V65-R259", 1, *S.conf_twin("conf-V65-R259", 1, fault=15)), "token_confidence conf")
    caught(S.conf_check("conf-V65-R259", 2, *S.conf_twin("conf-V65-R259", 2, fault=17)), "token_confidence conf")


# ------------------------------------------------------------------------------------------------------------------ planted faults
PLANTED = {   # fault: (the case that rejects it, the check that fails there)
    1: ("exact-mass-V64", "probs"),
    2: ("p-mode1-T0.7-V300-R259", "probs zero pattern"),
    3: ("topp1e-6-V300-mode1", "probs zero pattern"),
    4: ("k-mode1-T1-V300-R259", "probs"),
    5: ("topk-gtV-V300", "probs zero pattern"),
    6: ("k-mode1-T1-V300-R259", "probs zero pattern"),
    7: ("pk-mode0-T1-V300-R259", "probs"),
    8: ("p-mode1-T0.7-V300-R259", "probs zero pattern"),
    9: ("pk-mode0-T1-V300-R259", "tok is a member"),
    10: ("u32-max-V300", "tok in [0, V)"),
    11: ("u32-zero-V300", "tok is a member"),
    12: ("u32-max-V300", "tok is a member"),
    13: ("p-mode1-T0-alg0-V64-R259", "tok is the lowest index"),
    14: ("k-mode1-T1-V300-R259", "conf"),
    15: ("k-mode1-T1-V300-R259", "conf"),
    16: ("p-mode1-T0.7-V300-R259", "conf"),
    17: ("T50-V65-mode2", "conf"),
    18: ("pk-mode0-T1-V300-R259", "conf"),
    19: ("u33-zero-V300", "conf"),
    20: ("u33-zero-V300", "conf"),
    21: ("p-mode1-T0.7-V300-R259", "probs"),
    22: ("pk-mode0-T1-V300-R259", "probs"),
    23: ("none-mode1-T0.7-alg0-V1-R259", "conf"),
}


def _with_fallback(key):
    """The case, or a copy of it with other generic rows, in which the twin's row with u = 1 - 2^-24 runs out of accumulated mass (whether an
    fp32 sum of probabilities ends below 1 - 2^-24 depends on the last bit of the exponentials)."""
    for n in range(16):
        k = key if n == 0 else S.variant(key, rowseed=n)
        info = {}
        S.twin(k, info=info)
        if bool(info["fellback"].any()):
            return k
    raise AssertionError("no row takes the fallback branch")


@pytest.mark.parametrize("fault", sorted(PLANTED))
def test_planted_fault_is_rejected(fault):
    key, where = PLANTED[fault]
    assert fault in S.FAULTS
    if fault in (10, 12):
        key = _with_fallback(key)
        S.shares_hold(key)
        passes(S.check(key, *S.twin(key)))
    caught(S.check(key, *S.twin(key, fault=fault)), where)


def test_the_named_rows_are_what_rejects_the_lane_faults():
    """Faults 14 and 15 on the one row built for each: both maxima in one lane, and the pair that meets at butterfly stage 4."""
    key = "k-mode1-T1-V300-R259"
    i, r = S.inputs(key), S.reference(key)
    good = S.twin(key)[1]
    for fault, name in ((14, "top2-lane"), (15, "top2-xor-2")):
        row = i["names"].index(name)
        bad = S.twin(key, fault=fault)[1]
        ref = r["P1"][row] - r["P2"][row]
        bound = r["k"][row] * S.U * (r["P1"][row] + r["P2"][row]) + 2 * S.TINY
        assert abs(good[row] - ref) <= bound < abs(bad[row] - ref), (fault, name)
