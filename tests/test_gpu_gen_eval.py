"""The generation-evaluation kernels (csrc/generation.hip, gget_op_unmask_origin_rows) through the C ABI against the numpy twin
(tests/_gen_ref.py) and the torch statement of the rule, then the samplers and `evaluate_generation` end to end on the tiny model of
tests/golden/generation.npz.  Integer / compare work only: everything is compared for equality."""
import ctypes as C
import importlib
import os
import types

import numpy as np
import pytest
import torch

import _gen_ref as R
from _util import GOLDEN

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
gen = importlib.import_module("graph-gpt_amd.generation")
MASK = 1


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ST():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    return L.load()


# ------------------------------------------------------------------------------------------ gget_op_unmask_ranked
def _sample(rs, N, kind):
    """One sample (x, conf, cand, p) of a named kind; cand never holds <mask>, so a revealed cell is recognisable."""
    x = rs.randint(2, 90, N).astype(np.int64)
    conf = rs.randn(N).astype(np.float32)
    cand = rs.randint(100, 190, N).astype(np.int64)
    p = 0.5
    masked = rs.rand(N) < 0.6
    if kind == "no_mask":
        masked[:] = False
    elif kind == "all_mask":
        masked[:] = True
        p = 0.37
    elif kind == "all_equal":                  # n < n_masked among equal confidences: the lowest indices win
        conf[:] = 0.25
        p = 0.4
    elif kind == "tie_straddle":               # ~20 % at 1.0, ~70 % at 0.5, the rest at -1: the cut (p = 0.5) falls inside the 0.5 group
        u = rs.rand(N)
        conf = np.where(u < 0.2, 1.0, np.where(u < 0.9, 0.5, -1.0)).astype(np.float32)
    elif kind == "zeros":                      # +0.0 beside -0.0 (equal: the cut falls among them), a few negatives below them
        conf = np.where(rs.rand(N) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        conf[rs.rand(N) < 0.2] = -1.0
    elif kind == "negative_ignore_unmasked":   # masked cells all negative, unmasked cells carry larger confidences
        masked = rs.rand(N) < 0.3
        conf = np.where(masked, -np.abs(conf) - 0.1, np.abs(conf) + 5.0).astype(np.float32)
    elif kind == "p_zero":
        p = 0.0
    elif kind == "p_one":
        p = 1.0
    elif kind == "one_masked":
        masked[:] = False
        masked[rs.randint(N)] = True
        p = 1.0
    elif kind == "random":
        p = float(rs.rand())
    x[masked] = MASK
    return x, conf, cand, np.float32(p)


BATCHES = (("no_mask", "all_mask", "all_equal", "tie_straddle", "zeros"),
           ("negative_ignore_unmasked", "p_zero", "p_one", "random", "one_masked"))


def _run_ranked(lib, x, conf, cand, p):
    """Launch on copies; returns (x after, n_revealed) and checks that conf and cand are bit-unchanged."""
    xd, cd, td, pd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, conf, cand, np.atleast_1d(p).astype(np.float32)))
    c0, t0 = cd.clone(), td.clone()
    B, N = x.shape
    nr = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    L.check(lib.gget_op_unmask_ranked(P(xd), P(cd), P(td), B, N, MASK, P(pd), 0 if pd.numel() == 1 else 1, P(nr), ST()))
    torch.cuda.synchronize()
    assert torch.equal(cd.view(torch.int32), c0.view(torch.int32)) and torch.equal(td, t0), "conf / cand were written"
    return xd.cpu().numpy(), nr.cpu().numpy()


def _check_ranked(lib, x, conf, cand, p):
    got, nr = _run_ranked(lib, x, conf, cand, p)
    want, n_want = R.ranked_reveal(x, conf, cand, MASK, p)
    keep = x != MASK
    assert np.array_equal(got[keep], x[keep]), "an unmasked cell was written"
    assert np.array_equal(nr, n_want), f"n_revealed {nr} != {n_want}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} cells differ from the twin, first (sample, cell) {bad[:4].tolist()}"
    return want, n_want


@pytest.mark.parametrize("p_stride", [0, 1])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_unmask_ranked_matches_twin(lib, N, p_stride):
    rs = np.random.RandomState(1000 * p_stride + N)
    for kinds in BATCHES:
        xs, cs, ts, ps = (np.stack(a) for a in zip(*[_sample(rs, N, k) for k in kinds]))
        for p in ([ps] if p_stride else [np.float32(v) for v in sorted(set(ps.tolist()))]):
            want, n = _check_ranked(lib, xs, cs, ts, p)
            pb = np.broadcast_to(np.atleast_1d(p), (len(kinds),))
            if not p_stride:
                continue
            for b, kind in enumerate(kinds):         # (per-sample p) the arranged case really is the case
                idx = np.nonzero(xs[b] == MASK)[0]
                if kind == "no_mask":
                    assert len(idx) == 0 and n[b] == 0
                if kind in ("p_zero", "p_one", "one_masked"):
                    assert n[b] == (0 if kind == "p_zero" else len(idx)) and (kind == "p_zero" or (want[b] != MASK).all())
                if N < 63:
                    continue
                if kind in ("all_mask", "all_equal", "tie_straddle"):
                    assert 0 < n[b] < len(idx) and (kind != "all_mask" or len(idx) == N)
                if kind == "all_equal":
                    assert np.array_equal(np.nonzero(want[b] != xs[b])[0], idx[: n[b]])
                if kind == "tie_straddle":
                    ranked = np.sort(cs[b, idx])[::-1]
                    assert ranked[n[b] - 1] == ranked[n[b]], "the cut does not fall inside a tie group: pick another seed"
                if kind == "zeros":
                    z = cs[b, idx][cs[b, idx] == 0]
                    assert np.signbit(z).any() and (~np.signbit(z)).any() and (cs[b, idx] == 0).sum() > n[b] > 0
                if kind == "negative_ignore_unmasked":
                    assert cs[b, idx].max() < 0 < cs[b, xs[b] != MASK].min() and 0 < n[b]


def test_unmask_ranked_longest_reference_row(lib):
    """N = 13 312 (S 1024 x F 13), B = 2: one sample of distinct confidences, one of 16 values (tie groups of hundreds of cells)."""
    rs = np.random.RandomState(5)
    N = 13312
    x = rs.randint(2, 90, (2, N)).astype(np.int64)
    x[rs.rand(2, N) < 0.7] = MASK
    conf = np.stack([rs.randn(N), rs.randint(-8, 8, N) / 8]).astype(np.float32)
    cand = rs.randint(100, 190, (2, N)).astype(np.int64)
    _, n = _check_ranked(lib, x, conf, cand, np.array([0.3, 0.5], np.float32))
    assert (n > 2000).all()
    _check_ranked(lib, x, conf, cand, np.float32(0.9))


def test_new_entries_reject_bad_arguments(lib):
    t = torch.zeros(8, dtype=torch.int64, device="cuda")
    f = torch.zeros(8, dtype=torch.float32, device="cuda")
    i = torch.zeros(2, dtype=torch.int32, device="cuda")
    pin = torch.zeros(2, dtype=torch.int32).pin_memory()
    bad = [lib.gget_op_unmask_ranked(None, P(f), P(t), 1, 8, MASK, P(f), 0, None, ST()),
           lib.gget_op_unmask_ranked(P(t), P(f), P(t), -1, 8, MASK, P(f), 0, None, ST()),
           lib.gget_op_unmask_ranked(P(t), P(f), P(t), 1, 8, MASK, P(f), 2, None, ST()),
           lib.gget_op_gen_plan(P(t), 1, 8, MASK, None, 3, P(i), P(f), P(pin), ST()),
           lib.gget_op_gen_plan(P(t), 1, -8, MASK, P(f), 3, P(i), P(f), P(pin), ST()),
           lib.gget_op_gen_plan(P(t), 1, 8, MASK, P(f), 3, P(i), P(f), None, ST()),
           lib.gget_op_unmask_origin_rows(P(t), P(t), 1, 8, None, 1, MASK, ST()),
           lib.gget_op_gen_acc(P(t), P(t), None, 1, 8, MASK, P(i), ST()),
           lib.gget_op_gen_acc(P(t), P(t), P(t), 1, -1, MASK, P(i), ST())]
    assert all(rc != 0 for rc in bad), bad
    assert lib.gget_last_error()
    torch.cuda.synchronize()
    assert int(t.sum()) == 0


# ------------------------------------------------------------------------------------------ gget_op_gen_plan
def test_gen_plan_matches_reveal_counts(lib):
    """A whole loop of the batch rule: 40 steps for at most 7 masked cells, so the first calls skip several steps (k = 0), the last
    step has p = 1, and once nothing is masked the rule stops without advancing."""
    rs = np.random.RandomState(3)
    B, N, steps = 4, 50, 40
    x = torch.from_numpy(rs.randint(2, 90, (B, N)).astype(np.int64))
    for b, n in enumerate((0, 7, 3, 5)):
        x[b, torch.from_numpy(rs.permutation(N)[:n])] = MASK
    x = x.cuda()
    ts = torch.linspace(1, 1e-3, steps + 1, device="cuda")
    plan = gen._Plan(lib, ts)
    p_tab = plan.p_tab.cpu().numpy()
    assert np.array_equal(p_tab, R.step_p_table(ts.cpu().numpy())) and p_tab[-1] == 1.0
    i, jumps, p_seen = 0, [], []
    nr = torch.zeros(B, dtype=torch.int32, device="cuda")
    while i < steps:
        n_reveal, k, i_want = gen.reveal_counts(x, ts, i, MASK)
        i_twin, p_twin, any_twin = R.plan_rule(int((x == MASK).sum(dim=1).max()), p_tab, i)
        plan.launch(x, MASK)
        i_got, any_got = plan.read()
        assert (i_got, any_got) == (i_want, True) == (i_twin, any_twin) and int(plan.i.item()) == i_want
        assert float(plan.p.item()) == float(p_twin) == float(p_tab[i_want - 1])
        conf = torch.from_numpy(rs.randn(B, N).astype(np.float32)).cuda()
        cand = torch.from_numpy(rs.randint(100, 190, (B, N)).astype(np.int64)).cuda()
        gen.unmask_ranked(lib, x, conf, cand, MASK, plan.p, nr)
        assert torch.equal(nr, n_reveal) and int(nr.max()) == k >= 1
        jumps.append(i_want - i)
        p_seen.append(float(plan.p.item()))
        i = i_want
    assert max(jumps) > 1 and p_seen[-1] == 1.0 and not bool((x == MASK).any())
    plan.launch(x, MASK)                                   # nothing masked: i stays, p = 0, any_masked = 0
    assert plan.read() == (steps, False) and float(plan.p.item()) == 0.0
    x[1, 4] = MASK                                         # masked cells but no step left: no rule iteration either
    plan.launch(x, MASK)
    assert plan.read() == (steps, True) and float(plan.p.item()) == 0.0
    plan.i.zero_()                                         # an unmasked batch at i = 0
    x[1, 4] = 5
    plan.launch(x, MASK)
    assert plan.read() == (0, False) and float(plan.p.item()) == 0.0 and int(plan.i.item()) == 0


# ------------------------------------------------------------------------------------------ origin rows, accuracy counts
def test_unmask_origin_rows_matches_draws(lib):
    rs = np.random.RandomState(8)
    B, N, seed, it = 5, 333, 21, 3
    x = rs.randint(2, 90, (B, N)).astype(np.int64)
    x[rs.rand(B, N) < 0.5] = MASK
    cand = rs.randint(100, 190, (B, N)).astype(np.int64)
    p = np.array([0.0, 0.3, 1.0, 0.62, 1e-3], np.float32)
    u = gen.draws(seed, it, B, N)[2].numpy()
    want = np.where((x == MASK) & (u < p[:, None]), cand, x)
    xd, td, pd = (torch.from_numpy(a).cuda() for a in (x, cand, p))
    L.check(lib.gget_op_unmask_origin_rows(P(xd), P(td), B, N, P(pd), gen.iteration_seed(seed, it), MASK, ST()))
    got = xd.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], x[0]) and (got[2] != MASK).all() and 0 < (got[1] == MASK).sum() < (x[1] == MASK).sum()


def test_gen_acc_matches_twin(lib):
    rs = np.random.RandomState(9)
    B, S, F = 5, 111, 3
    ids = rs.randint(2, 20, (B, S, F)).astype(np.int64)
    ids[rs.rand(B, S, F) < 0.4] = MASK
    ids[2] = 7                                             # a sample without a masked cell: counts {0, 0}, accuracy 0 / 0 = NaN
    labels = rs.randint(2, 6, (B, S, F)).astype(np.int64)
    res = rs.randint(2, 6, (B, S * F)).astype(np.int64)
    res[4] = labels[4].reshape(-1)                         # a sample rebuilt exactly
    want = R.acc_counts(res, labels, ids, MASK)
    cfg = gen.GenerationConfig(mask_token_id=MASK)
    idd, ld, rd = (torch.from_numpy(a).cuda() for a in (ids, labels, res))
    assert np.array_equal(gen.gen_acc_counts(MASK, idd, ld, rd).cpu().numpy(), want)
    acc = gen.cal_gen_acc_batch(cfg, idd, ld, rd).cpu().numpy()
    ref = R.acc_from_counts(want)
    assert acc.dtype == np.float32 and np.array_equal(acc.view(np.uint32), ref.view(np.uint32))
    assert np.isnan(acc[2]) and acc[4] == 1.0 and 0 < acc[0] < 1
    one = gen.cal_gen_acc_per_sample(cfg, idd[1], ld[1], rd[1])
    assert one.dim() == 0 and float(one) == float(ref[1])


# ------------------------------------------------------------------------------------------ end to end on the tiny model
@pytest.fixture(scope="module")
def tiny():
    modeling = importlib.import_module("graph-gpt_amd.modeling")
    weights = importlib.import_module("graph-gpt_amd.weights")
    g = np.load(os.path.join(GOLDEN, "generation.npz"))
    e = np.load(os.path.join(GOLDEN, "gen_eval.npz"))
    std, head_std, seed = g["meta_init"]
    cfg = modeling.GraphGPTConfig(hidden_act="gelu", vocab_size=300, hidden_size=128, intermediate_size=512, num_hidden_layers=2,
                                  num_attention_heads=2, max_position_embeddings=1024, causal_attention=False, stacked_feat=4,
                                  next_n_token=4)
    model = modeling.GraphGPTPretrainBase(cfg, seed=0).cuda()
    sd = weights.make_state_dict(model.spec, seed=int(seed), std=float(std), head_std=float(head_std))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    assert np.array_equal(g["in_input_ids"], e["in_input_ids"])
    ids, att, lab = (torch.from_numpy(e[k]).cuda() for k in ("in_input_ids", "in_attention_mask", "in_labels"))
    return model, ids, att, lab


BATCH_CASES = {
    "maskgit_plus": dict(alg="maskgit_plus", steps=6),
    "maskgit_plus_skips": dict(alg="maskgit_plus", steps=64),          # more steps than masked cells: the rule skips steps
    "topk_margin": dict(alg="topk_margin", steps=6),
    "entropy": dict(alg="entropy", steps=6),
    "sampled_gumbel": dict(alg="maskgit_plus", steps=6, temperature=0.5, top_p=0.9, top_k=30, alg_temp=0.4, seed=12),
}


@pytest.mark.parametrize("case", sorted(BATCH_CASES))
def test_sample_per_batch_device_path_equals_torch_path(tiny, monkeypatch, case):
    model, ids, att, _ = tiny
    gcfg = gen.GenerationConfig(eps=1e-3, mask_token_id=MASK, output_history=True, **BATCH_CASES[case])
    monkeypatch.setenv("GGET_GEN_DEVICE", "1")
    x_dev, h_dev = gen.sample_per_batch(model, gcfg, input_ids=ids, attention_mask=att)
    monkeypatch.setenv("GGET_GEN_DEVICE", "0")
    x_ref, h_ref = gen.sample_per_batch(model, gcfg, input_ids=ids, attention_mask=att)
    assert len(h_dev) == len(h_ref) >= 3
    for it, (a, b) in enumerate(zip(h_dev, h_ref)):
        assert torch.equal(a, b), f"{case}: token grid differs after iteration {it}"
    assert torch.equal(x_dev, x_ref) and not bool((x_dev == MASK).any())
    start = ids.view(3, -1) == MASK
    assert torch.equal(x_dev[~start], ids.view(3, -1)[~start]), "given tokens must never be rewritten"


EXAMPLE_CASES = {
    "maskgit_plus": dict(alg="maskgit_plus", steps=6),
    "entropy_own_schedules": dict(alg="entropy", steps=64),            # steps_b = n_masked_b: every sample its own schedule
    "topk_margin_gumbel": dict(alg="topk_margin", steps=6, temperature=0.7, top_k=40, alg_temp=0.3, seed=5),
    "origin": dict(alg="origin", steps=6, temperature=0.8, top_p=0.9, seed=11),
}


@pytest.mark.parametrize("case", sorted(EXAMPLE_CASES))
def test_sample_per_example_equals_twin_loop(tiny, case):
    """The engine's loop against the twin's per-example loop driven by the SAME per-iteration sampling-kernel outputs (and, for
    "origin", the Python twin of the transfer draws), grid by grid."""
    model, ids, att, _ = tiny
    gcfg = gen.GenerationConfig(eps=1e-3, mask_token_id=MASK, output_history=True, **EXAMPLE_CASES[case])
    B, S, F = ids.shape
    N = S * F
    x, hist = gen.sample_per_example(model, gcfg, input_ids=ids, attention_mask=att)
    x0 = ids.view(B, N).cpu().numpy()
    tab = R.example_p_table((x0 == MASK).sum(axis=1), gcfg.steps, gcfg.eps)
    assert np.array_equal(tab, gen.example_p_table((x0 == MASK).sum(axis=1).tolist(), gcfg.steps, gcfg.eps).numpy())
    if case == "entropy_own_schedules":
        assert len(set((tab > 0).sum(axis=0).tolist())) > 1
    assert len(hist) == tab.shape[0]
    cur = x0.copy()
    for it in range(tab.shape[0]):
        with torch.no_grad():
            model(input_ids=torch.from_numpy(cur).cuda().view(B, S, F), attention_mask=att, labels=None)
        conf, cand = gen.token_sample(model._engine, B * N, gcfg, gen.iteration_seed(gcfg.seed, it), gumbel=gcfg.alg != "origin")
        conf, cand = conf.view(B, N).cpu().numpy(), cand.view(B, N).cpu().numpy()
        if gcfg.alg == "origin":
            u = gen.draws(gcfg.seed, it, B, N)[2].numpy()
            cur = np.where((cur == MASK) & (u < tab[it][:, None]), cand, cur)
        else:
            cur, _ = R.ranked_reveal(cur, conf, cand, MASK, tab[it])
        assert np.array_equal(hist[it].cpu().numpy(), cur), f"{case}: token grid differs after iteration {it}"
    assert np.array_equal(x.cpu().numpy(), cur) and (cur != MASK).all()
    assert np.array_equal(cur[x0 != MASK], x0[x0 != MASK]), "given tokens must never be rewritten"


def test_sample_per_example_takes_one_unpadded_sample(tiny):
    """The reference's signature: input_ids [S, F], attention_mask [1, S]."""
    model, ids, att, _ = tiny
    n = int(att[1].sum())
    one = ids[1, :n]
    x, hist = gen.sample_per_example(model, gen.GenerationConfig(steps=6, mask_token_id=MASK), input_ids=one,
                                     attention_mask=att[1, :n].unsqueeze(0), inputs_raw_embeds=None)
    assert hist is None and tuple(x.shape) == (1, one.numel()) and not bool((x == MASK).any())
    keep = one.reshape(-1) != MASK
    assert torch.equal(x[0][keep], one.reshape(-1)[keep])


@pytest.mark.parametrize("alg", ["maskgit_plus", "entropy"])
def test_eval_gen_accuracies_equal_twin_on_returned_tokens(tiny, alg):
    model, ids, att, lab = tiny
    gcfg = gen.GenerationConfig(alg=alg, steps=6, eps=1e-3, mask_token_id=MASK)
    for sampler, evaluator in ((gen.sample_per_batch, gen.eval_gen_per_batch), (gen.sample_per_example, gen.eval_gen_per_sample)):
        tokens, _ = sampler(model, gcfg, input_ids=ids, attention_mask=att)
        acc = evaluator(model, gcfg, input_ids=ids, attention_mask=att, labels=lab, inputs_raw_embeds=None)
        want = R.acc_from_counts(R.acc_counts(tokens.cpu().numpy(), lab.cpu().numpy(), ids.cpu().numpy(), MASK))
        assert tuple(acc.shape) == (3,) and np.array_equal(acc.cpu().numpy().view(np.uint32), want.view(np.uint32))


class _RemaskingLoader:
    """Two batches of the fixture's unmasked tokens, masked again on every pass from the CURRENT umr_clip (as the reference's
    collator does when the loader is iterated)."""

    def __init__(self, tokens, att, params):
        self.tokens, self.att, self.params, self.bands = tokens, att, params, []

    def __iter__(self):
        smtp = importlib.import_module("graph-gpt_amd.smtp")
        lo, hi = self.params.umr_clip
        self.bands.append((lo, hi))
        for seed in (1, 2):
            masked, labels = smtp.smtp_mask_rows(self.tokens, self.att.sum(dim=1), umr_min=lo, umr_max=hi, seed=100 * len(self.bands) + seed)
            yield {"input_ids": masked, "attention_mask": self.att, "labels": labels}


@pytest.mark.parametrize("parallel_gen", [False, True])
def test_evaluate_generation_on_the_engine(tiny, parallel_gen):
    model, ids, att, lab = tiny
    tokens = torch.where(lab != -100, lab, ids)
    params = types.SimpleNamespace(umr_clip=[0.3, 0.6])
    cfg = types.SimpleNamespace(generation=gen.GenerationConfig(alg="maskgit_plus", steps=4, mask_token_id=MASK, output_history=True,
                                                                parallel_gen=parallel_gen),
                                training=types.SimpleNamespace(pretrain_mlm=types.SimpleNamespace(params=params)))
    loader = _RemaskingLoader(tokens, att, params)
    model.train()
    out = gen.evaluate_generation(model, loader, "valid", True, cfg)
    vals = [float(v) for v in out.split(",")]
    assert len(vals) == 10 and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in vals), out
    sp = np.linspace(0.01, 0.99, 11)
    assert np.allclose(loader.bands, list(zip(sp[:-1], sp[1:])))
    assert params.umr_clip == [0.3, 0.6] and model.training and cfg.generation.output_history is False
