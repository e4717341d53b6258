"""Host-side checks of the step replay (tests/_step_replay.py): the comparer passes on identical tensors and fails, at the right place,
on planted faults; the dispatch mirror's table for the cases of tests/test_gpu_step_replay.py is written out here (a change of the rule is
a visible diff); the three-buffer rotation of the residual-stream gradient; the restated parameter plan against the library's."""
import importlib

import pytest
import torch

import _step_replay as R

L = importlib.import_module("graph-gpt_amd._lib")
eng = importlib.import_module("graph-gpt_amd.engine")
spec_mod = importlib.import_module("graph-gpt_amd.spec")
BF = torch.bfloat16


def spec_of(size="tiny", layers=2, **kw):
    d = {"tiny": 128, "base": 768}[size]
    base = dict(kind=spec_mod.KIND_TASK, vocab_size=300, hidden_size=d, intermediate_size=4 * d, num_layers=layers, num_heads=d // 64,
                stacked_feat=4, next_n_token=1, max_position=128, num_labels=2)
    base.update(kw)
    return spec_mod.ModelSpec(**base)


# ------------------------------------------------------------------------------------------------ the comparer
def observables(seed=0, layers=3, rows=12, cols=16):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(layers):
        out.append((f"hidden[{i}]", torch.randn(rows, cols, generator=g).to(BF)))
        out.append((f"qkv[{i}]", torch.randn(rows, 3 * cols, generator=g).to(BF)))
    out.append(("loss", torch.randn(1, generator=g)))
    return out


def pairs_of(got, want):
    return [(n, g, w) for (n, g), (_, w) in zip(got, want)]


def test_comparer_passes_on_identical_tensors():
    a, b = observables(), observables()
    assert R.first_difference(pairs_of(a, b)) is None
    assert R.compare_bits("x", torch.tensor([0.0, -0.0]), torch.tensor([0.0, -0.0])) is None
    # integers, not values: the sign of a zero is a difference, and a NaN equals itself
    assert R.compare_bits("x", torch.tensor([0.0]), torch.tensor([-0.0])) is not None
    nan = torch.full((4,), R.SENT16, dtype=torch.int16).view(BF)
    assert R.compare_bits("x", nan, nan.clone()) is None


def planted(fault):
    got, want = observables(), observables()
    name, t = got[2]                      # hidden[1]
    t = t.clone()
    if fault == "low bit":
        t.view(torch.int16)[5, 7] ^= 1
    elif fault == "row swap":
        t[[4, 5]] = t[[5, 4]]
    elif fault == "sentinel row":
        t.view(torch.int16)[9] = R.SENT16
    elif fault == "other layer":
        t = got[4][1].clone()             # hidden[2]
    got[2] = (name, t)
    return R.first_difference(pairs_of(got, want))


def test_comparer_names_one_flipped_low_bit():
    msg = planted("low bit")
    assert msg.startswith("first differing observable in step order - hidden[1]: 1 of 192 elements differ in 1 row(s) [5] (scattered elements)")
    assert "(5, 7) got" in msg and "also differing" not in msg


def test_comparer_sees_a_row_swapped_with_its_neighbour_as_whole_rows():
    msg = planted("row swap")
    assert "hidden[1]: 32 of 192 elements differ in 2 row(s) [4, 5] (WHOLE rows)" in msg


def test_comparer_says_when_a_row_is_still_at_the_sentinel():
    msg = planted("sentinel row")
    assert "hidden[1]: 16 of 192 elements differ in 1 row(s) [9] (WHOLE rows, 16 still at the sentinel)" in msg


def test_comparer_localises_a_tensor_equal_to_another_layers():
    msg = planted("other layer")
    assert msg.startswith("first differing observable in step order - hidden[1]:") and "in 12 row(s)" in msg


def test_comparer_reports_the_first_in_step_order_and_lists_the_rest():
    got, want = observables(), observables()
    for k in (3, 1, 6):                   # qkv[1], qkv[0], loss - planted out of order
        got[k] = (got[k][0], got[k][1] + 1)
    msg = R.first_difference(pairs_of(got, want))
    assert msg.startswith("first differing observable in step order - qkv[0]:") and "also differing later: ['qkv[1]', 'loss']" in msg


def test_guard_rows_and_round_up_rows_of_a_buffer():
    b = R.Buf(6, 8, BF, real=4, device="cpu")
    assert b.guard_intact() and b.rows_at_sentinel().tolist() == [True] * 4 + [False] * 2 and bool((b.body()[4:] == 0).all())
    b.body()[:] = 1.0
    assert b.guard_intact() and not bool(b.rows_at_sentinel().any())
    b.t[6 * 8 + 3] = 2.0                  # one element of the first guard row
    assert not b.guard_intact()
    f = R.Buf(3, 4, torch.float32, device="cpu")
    assert f.guard_intact()
    f.t[3 * 4 + R.GUARD_ROWS * 4 - 1] = 0.0   # the last element of the last guard row
    assert not f.guard_intact()


def test_bound_of_an_atomic_sum():
    ref, ab = torch.tensor([1.0, -2.0]).double(), torch.tensor([3.0, 5.0]).double()
    assert R.held_sum("s", ref.float().to(BF), ref, ab, 10)[1] is None
    ratio, fail = R.held_sum("s", torch.tensor([1.0, -2.02]), ref, ab, 10)
    assert ratio > 1 and "1 of 2 elements outside" in fail
    assert R.held_sum("s", torch.tensor([float("nan"), -2.0]), ref, ab, 10)[1] is not None


# ------------------------------------------------------------------------------------------------ the dispatch mirror, written out
PLAIN_2 = {1: "plain", 0: "plain"}
TABLE = {
    #        spec kwargs, B, S, tokens, options                 -> layout, T, pack_wo, attn_fwd, attn_bwd, geglu / mlp_bwd, wgrad, ln1_bwd, final norm fwd / bwd, embed_bwd
    "A": (dict(), 5, 32, None, dict(),
          ("padded", 160, "per-forward", "per-sample", "per-sample", "fused", "fused", "grouped-2+qkvo-slabs-split1", PLAIN_2, "own-launch", "plain", "dense")),
    "B": (dict(size="base", vocab_size=756), 6, 32, 102, dict(),
          ("varlen", 128, "per-forward", "per-sample", "per-sample", "fused", "fused", "grouped-4", PLAIN_2, "own-launch", "plain", "dense")),
    "C-S72-padded": (dict(), 3, 72, None, dict(),
                     ("padded", 216, "none", "three-launch", "norm-bwd+dgrad+attn-bwd", "fused", "fused", "grouped-2+qkvo-slabs-split1", PLAIN_2, "own-launch",
                      "plain", "dense")),
    # (the o weights are packed for the BACKWARD's per-sample kernel alone: the forward of 33 .. 64-row samples stays on three launches)
    "C-S48-varlen": (dict(), 4, 48, 102, dict(),
                     ("varlen", 128, "per-forward", "three-launch", "per-sample+long_list", "fused", "fused", "grouped-2+qkvo-slabs-split1", PLAIN_2,
                      "own-launch", "plain", "dense")),
    "D": (dict(layers=3, layer_scale_init=1.0, path_pdrop=0.2), 4, 32, None, dict(),
          ("padded", 128, "none", "ls-residual", "ls-norm-bwd+dgrad+attn-bwd", "fused", "fused", "grouped-2+qkvo-slabs-split1",
           {2: "fuse_next", 1: "fuse_next", 0: "plain"}, "from-last-layer", "fused-ls2", "dense")),
    "D-mlp-dropout-on": (dict(layers=3, layer_scale_init=1.0, path_pdrop=0.2, mlp_pdrop=0.1), 4, 32, None, dict(mlp_drop=0.1),
                         ("padded", 128, "none", "ls-residual", "ls-norm-bwd+dgrad+attn-bwd", "fused", "gemm+dropout+geglu'", "grouped-2+qkvo-slabs-split1",
                          {2: "fuse_next", 1: "fuse_next", 0: "plain"}, "from-last-layer", "fused-ls2", "dense")),
    "E": (dict(gated_agg=True, num_labels=1, score_bias=True), 4, 32, None, dict(),
          ("padded", 128, "per-forward", "per-sample", "per-sample", "fused", "fused", "grouped-2+qkvo-slabs-split1", PLAIN_2, "own-launch", "plain", "sorted")),
    "F": (dict(), 5, 32, None, dict(frozen=1),
          ("padded", 160, "per-forward", "per-sample", "per-sample", "fused", "fused", "grouped-2+qkvo-slabs-split1", {1: "dw-only"}, "own-launch", "plain", "none")),
    "G-step2": (dict(), 3, 24, 35, dict(),
                ("varlen", 64, "per-forward", "per-sample", "per-sample", "fused", "fused", "grouped-2+qkvo-slabs-split1", PLAIN_2, "own-launch", "plain", "dense")),
}
KEYS = ("layout", "T", "pack_wo", "attn_fwd", "attn_bwd", "geglu", "mlp_bwd", "wgrad", "ln1_bwd", "final_norm", "final_norm_bwd", "embed_bwd")


@pytest.mark.parametrize("case", sorted(TABLE))
def test_dispatch_mirror_table(case):
    kw, B, S, tokens, opt, want = TABLE[case]
    f = R.forms(spec_of(**kw), B, S, tokens, **opt)
    assert tuple(f[k] for k in KEYS) == want


def test_dispatch_mirror_edges():
    tiny = spec_of()
    # a token count that does not compact (round-up reaches B S): padded layout, but the o weights are still packed at 32 < S <= 64
    f = R.forms(tiny, 2, 48, 90)
    assert (f["layout"], f["T"], f["pack_wo"], f["attn_bwd"]) == ("padded", 96, "per-forward", "norm-bwd+dgrad+attn-bwd")
    assert R.forms(tiny, 2, 48, None)["pack_wo"] == "none" and R.forms(tiny, 2, 65, 70)["pack_wo"] == "none"
    # 16 heads: no per-sample kernel (its tiles do not fit the LDS)
    assert R.forms(spec_of(hidden_size=1024, num_heads=16, intermediate_size=4096), 4, 32)["attn_fwd"] == "three-launch"
    # the K-slice rule of the slab launch, the GEGLU fusion width, everything frozen
    assert R.qkvo_split(3071) == 1 and R.qkvo_split(3072) == 3
    assert R.forms(spec_of(intermediate_size=448), 4, 32)["geglu"] == "gemm+elementwise"
    f = R.forms(tiny, 4, 32, frozen=2)
    assert (f["first_layer"], f["ln1_bwd"], f["final_norm_bwd"], f["embed_bwd"]) == (2, {}, "dw-only", "none")
    # a trainable gate upstream: the chain is not truncated
    f = R.forms(spec_of(gated_agg=True), 4, 32, frozen=1)
    assert (f["first_layer"], f["ln1_bwd"], f["embed_bwd"]) == (0, PLAIN_2, "sorted")
    # a full last round of the CUs or none
    assert R.forms(tiny, 288, 32)["pack_wo"] == "none" and R.forms(tiny, 448, 32)["pack_wo"] == "per-forward"


def test_which_tensors_are_not_owed_equality():
    tiny = spec_of()
    names = lambda s, **o: sorted(R.inexact_tensors(s, R.forms(s, 4, 32, **o)))   # noqa: E731
    norms = sorted([f"model.layers.{i}.{n}_layernorm.weight" for i in (0, 1) for n in ("input", "post_attention")] + ["model.norm.weight"])
    assert names(tiny) == sorted(norms + ["score.weight"])
    assert names(tiny, reproducible=True) == ["score.weight"]
    gated = spec_of(gated_agg=True, score_bias=True, num_labels=1)
    assert names(gated, reproducible=True) == ["model.embed_tokens.weight", "score.bias", "score.weight", "stacked_feat_agg.weight"]
    ls = spec_of(layer_scale_init=1.0)
    assert names(ls, reproducible=True) == sorted([f"model.layers.{i}.lambda_{k}" for i in (0, 1) for k in (1, 2)] + ["score.weight"])


# ------------------------------------------------------------------------------------------------ the three-buffer rotation
def test_buffer_rotation_matches_layer_backward():
    """engine.hip: gget_backward_begin keeps d(final-norm output) in dxb and writes d(x_L) into dxa; layer_backward finds dx_out = dx_cur in
    {dxa, dxb, dxc}, takes the next buffer for dx_mid and the one after for dx_in, which becomes dx_cur."""
    assert R.rotation(1) == {0: ("a", "b", "c")}
    assert R.rotation(2) == {1: ("a", "b", "c"), 0: ("c", "a", "b")}
    assert R.rotation(3) == {2: ("a", "b", "c"), 1: ("c", "a", "b"), 0: ("b", "c", "a")}
    for Ln in (1, 2, 3, 7):
        rot = R.rotation(Ln)
        assert rot[Ln - 1][0] == "a" and rot[Ln - 1][1] == "b"      # the top layer's dx_mid reuses the head's (dead) gradient buffer
        for i in range(Ln):
            assert sorted(rot[i]) == ["a", "b", "c"]
            if i + 1 < Ln:
                assert rot[i][0] == rot[i + 1][2]                   # a layer reads what the layer above wrote
    assert R.rotation(3, first=1) == {2: ("a", "b", "c"), 1: ("c", "a", "b")}


# ------------------------------------------------------------------------------------------------ the plan, restated
@pytest.fixture(scope="module")
def lib():
    importlib.import_module("graph-gpt_amd.build").build()
    return L.load()


@pytest.mark.parametrize("kw", [dict(), dict(size="base", vocab_size=756), dict(layers=3, layer_scale_init=1.0, path_pdrop=0.2),
                                dict(gated_agg=True, num_labels=1, score_bias=True)], ids=["tiny", "base", "layerscale", "gated-regression"])
def test_restated_plan_is_the_librarys(lib, kw):
    spec = spec_of(**kw)
    offs, total = R.param_offsets(spec)
    plan = eng.Engine.plan_params_of(eng.make_config(spec, 256, 8))
    assert {k: (v["offset"], v["numel"], v["layer"]) for k, v in plan.items()} == offs
    assert list(plan) == list(spec.param_table())
    s32, n32 = R.scratch_layout(spec)
    segs = R.segment_table(spec)
    assert len(segs) == spec.num_layers + 2 and sum(len(b) for b in segs) == len(s32)
    flat = sorted((src, cnt * cp) for b in segs for src, _, cnt, cp, _ in b)
    assert flat[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(flat, flat[1:])) and flat[-1][0] + flat[-1][1] == n32
    assert [name for name in spec.param_table() if name in s32] == list(s32)
