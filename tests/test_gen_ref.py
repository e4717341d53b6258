"""CPU checks of the generation evaluation: the numpy twin (tests/_gen_ref.py) against the reference's recorded runs
(tests/golden/gen_eval.npz, written by tools/make_golden_gen_eval.py) and against the torch statement of the batch rule
(generation.unmask_step / reveal_counts); the band / string / reduction logic of `evaluate_generation` against stub models."""
import importlib
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _gen_ref as R
from _util import GOLDEN

gen = importlib.import_module("graph-gpt_amd.generation")
tr = importlib.import_module("graph-gpt_amd.training")

TAGS = ("maskgit_plus", "topk_margin", "entropy", "maskgit_plus_s64")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "gen_eval.npz"))


def _stripped(fx, b):
    keep = fx["in_attention_mask"][b] != 0
    return fx["in_input_ids"][b][keep], fx["in_labels"][b][keep]


@pytest.mark.parametrize("tag", TAGS)
def test_twin_reveal_reproduces_every_recorded_iteration(fx, tag):
    """Every `x before -> x after` of the reference's sample_per_example, from the recorded confidence grid and candidates and the p
    of the per-example schedule.  The s64 run gives every sample its own number of iterations (steps_b = n_masked_b)."""
    eps, mask_id = float(fx["meta_gen"][0]), int(fx["meta_gen"][1])
    steps = int(fx[f"{tag}_steps"])
    iters = []
    for b in range(fx["in_input_ids"].shape[0]):
        before, conf, cand, after = (fx[f"{tag}_b{b}_{k}"] for k in ("before", "conf", "cand", "after"))
        ids, _ = _stripped(fx, b)
        assert np.array_equal(before[0], ids.reshape(-1))
        tab = R.example_p_table([(before[0] == mask_id).sum()], steps, eps)[:, 0]
        assert len(tab) == before.shape[0], "the schedule's iteration count differs from the reference's"
        for it in range(len(tab)):
            got, n = R.ranked_reveal(before[it][None], conf[it][None], cand[it][None], mask_id, tab[it])
            assert np.array_equal(got[0], after[it]), f"{tag} sample {b} iteration {it}"
            assert n[0] == R.n_reveal((before[it] == mask_id).sum(), tab[it]) and (it < len(tab) - 1 or (got != mask_id).all())
        assert np.array_equal(after[-1], fx[f"{tag}_b{b}_final"])
        iters.append(len(tab))
    if tag == "maskgit_plus_s64":
        assert len(set(iters)) > 1, "the long run is there for samples with different schedules"


def test_twin_loop_reproduces_the_recorded_runs(fx):
    """The whole per-example loop on the PADDED batch, fed with the recorded grids: samples on different schedules in one batch."""
    eps, mask_id = float(fx["meta_gen"][0]), int(fx["meta_gen"][1])
    tag, steps = "maskgit_plus_s64", int(fx["maskgit_plus_s64_steps"])
    ids = fx["in_input_ids"]
    B, S, F = ids.shape
    N = S * F

    def conf_fn(it, x):
        conf = np.full((B, N), -np.inf, np.float32)
        cand = np.full((B, N), mask_id, np.int64)
        for b in range(B):
            rec = fx[f"{tag}_b{b}_conf"]
            if it < rec.shape[0]:
                n = rec.shape[1]
                assert np.array_equal(x[b, :n], fx[f"{tag}_b{b}_before"][it])
                conf[b, :n], cand[b, :n] = rec[it], fx[f"{tag}_b{b}_cand"][it]
        return conf, cand

    x, hist = R.per_example_loop(ids.reshape(B, N), mask_id, steps, eps, conf_fn)
    assert len(hist) == max(fx[f"{tag}_b{b}_conf"].shape[0] for b in range(B))
    for b in range(B):
        fin = fx[f"{tag}_b{b}_final"]
        assert np.array_equal(x[b, :len(fin)], fin) and np.array_equal(x[b, len(fin):], ids.reshape(B, N)[b, len(fin):])


@pytest.mark.parametrize("seed", range(6))
def test_twin_batch_rule_equals_torch_statement(seed):
    """`batch_step` of the twin against generation.unmask_step (reveal_counts inside it) on CPU tensors, whole loops: random grids with
    ties, and time grids far longer than the masked counts so that the skip loop advances i several times in one call."""
    g = torch.Generator().manual_seed(seed)
    B, N = 4, 37
    mask_id = 1
    x = torch.randint(2, 50, (B, N), generator=g)
    n_mask = [0, 3, 9, N][seed % 4:] + [5, 1, 2][: seed % 4]
    for b in range(B):
        x[b, torch.randperm(N, generator=g)[: n_mask[b]]] = mask_id
    n_steps = (6, 40, 200)[seed % 3]
    ts = torch.linspace(1, 1e-3, n_steps + 1)
    p_tab = R.step_p_table(ts.numpy())
    assert np.array_equal(p_tab, gen.step_p_table(ts).numpy())
    cfg = gen.GenerationConfig(mask_token_id=mask_id)
    xt, xn, i_t, i_n, jumps = x.clone(), x.numpy().copy(), 0, 0, []
    while i_t < n_steps:
        conf = (torch.randint(-3, 4, (B, N), generator=g).float() / 4) if seed % 2 else torch.randn(B, N, generator=g)
        cand = torch.randint(2, 50, (B, N), generator=g)
        k = gen.reveal_counts(xt, ts, i_t, mask_id)
        i_prev = i_t
        xt, i_t = gen.unmask_step(xt, conf, cand, ts, i_t, cfg)
        i_w, p_w, any_w = R.plan_rule(int((xn == mask_id).sum(axis=1).max()), p_tab, i_n)
        xn, i_n = R.batch_step(xn, conf.numpy(), cand.numpy(), p_tab, i_n, mask_id)
        assert (i_w, i_n) == (k[2], i_t) and np.array_equal(xn, xt.numpy())
        assert np.array_equal(R.ranked_reveal(xn, conf.numpy(), cand.numpy(), mask_id, 0.0)[0], xn)      # p = 0: a no-op
        jumps.append(i_t - i_prev)
        if not any_w:
            break
    assert (xn != mask_id).all() or n_steps == 0
    if n_steps >= 40:
        assert max(jumps) > 1, "no call advanced i more than once"


@pytest.mark.parametrize("tag", TAGS)
def test_twin_accuracies_equal_the_fixture_bit_for_bit(fx, tag):
    mask_id = int(fx["meta_gen"][1])
    ids, lab = fx["in_input_ids"], fx["in_labels"]
    B = ids.shape[0]
    got = R.acc_from_counts(R.acc_counts(fx[f"{tag}_batch_final"], lab, ids, mask_id))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), fx[f"{tag}_acc_per_batch"].view(np.uint32))
    for b in range(B):
        i_b, l_b = _stripped(fx, b)
        a = R.acc_from_counts(R.acc_counts(fx[f"{tag}_b{b}_final"][None], l_b[None], i_b[None], mask_id))
        assert np.array_equal(a.view(np.uint32), fx[f"{tag}_acc_per_sample"][b:b + 1].view(np.uint32))
    c = R.acc_counts(np.zeros((1, 4), np.int64), np.zeros((1, 4), np.int64), np.full((1, 4), 7), mask_id)
    assert c.tolist() == [[0, 0]] and np.isnan(R.acc_from_counts(c)[0])          # no masked cell: 0 / 0


# ------------------------------------------------------------------------------------------ evaluate_generation on stubs
class _StubModel:
    device = torch.device("cpu")

    def __init__(self):
        self.mode = "train"

    def eval(self):
        self.mode = "eval"

    def train(self):
        self.mode = "train"


class _BandLoader:
    """A loader that, like the reference's, reads umr_clip when it is ITERATED: every batch carries the band it was masked with."""

    def __init__(self, params, sizes, get):
        self.params, self.sizes, self.get = params, sizes, get

    def __iter__(self):
        lo, hi = self.get(self.params)
        for n in self.sizes:
            yield {"input_ids": torch.full((n, 2, 1), lo), "attention_mask": torch.ones(n, 2, dtype=torch.int64),
                   "labels": torch.full((n, 2, 1), hi)}


def _stub_eval(calls, name, offset):
    def fn(model, cfg, *, input_ids, attention_mask, labels, inputs_raw_embeds):
        assert model.mode == "eval" and inputs_raw_embeds is None and cfg.output_history is False
        calls.append(name)
        n = input_ids.shape[0]
        return input_ids[:, 0, 0].float() + offset + torch.arange(n).float() / 16       # the band's lower edge + a per-sample term
    return fn


def _cfg(as_dict, parallel_gen):
    gcfg = dict(alg="entropy", alg_temp=None, steps=8, eps=1e-3, temperature=0.0, top_p=None, top_k=None, output_history=True,
                mask_token_id=1, pad_token_id=0, parallel_gen=parallel_gen)
    params = dict(umr_clip=[0.2, 0.7])
    if as_dict:
        return {"generation": gcfg, "training": {"pretrain_mlm": {"params": params}}}, params
    ns = types.SimpleNamespace
    params = ns(**params)
    return ns(generation=ns(**gcfg), training=ns(pretrain_mlm=ns(params=params))), params


def _expected(sizes, offset):
    sp = np.linspace(0.01, 0.99, 11)
    per = np.concatenate([np.arange(n, dtype=np.float32) / 16 for n in sizes])
    sums = [(torch.tensor(float(sp[j]), dtype=torch.float32) + offset + torch.from_numpy(per)).float().sum(dim=0) for j in range(10)]
    return torch.stack(sums), float(len(per))


@pytest.mark.parametrize("as_dict,parallel_gen", [(False, False), (True, True)])
def test_evaluate_generation_bands_and_string(monkeypatch, as_dict, parallel_gen):
    cfg, params = _cfg(as_dict, parallel_gen)
    get = (lambda p: p["umr_clip"]) if as_dict else (lambda p: p.umr_clip)
    calls = []
    monkeypatch.setattr(gen, "eval_gen_per_batch", _stub_eval(calls, "batch", 0.0))
    monkeypatch.setattr(gen, "eval_gen_per_sample", _stub_eval(calls, "sample", 0.0))
    m = _StubModel()
    sizes = [3, 2]
    out = gen.evaluate_generation(m, _BandLoader(params, sizes, get), "valid", True, cfg)
    sums, n = _expected(sizes, 0.0)
    want = ",".join((sums / n).numpy().round(4).astype(str))
    assert out == want and len(out.split(",")) == 10
    assert calls == ["batch" if parallel_gen else "sample"] * 20
    assert get(params) == [0.2, 0.7] and m.mode == "train"
    g = cfg["generation"] if as_dict else cfg.generation
    assert (g["output_history"] if as_dict else g.output_history) is False
    # the bands themselves: the stub's accuracy starts at the band's lower edge
    sp = np.linspace(0.01, 0.99, 11)
    first = [float(v) for v in out.split(",")]
    assert np.allclose(first, sp[:10] + np.mean(np.concatenate([np.arange(k) / 16 for k in sizes])), atol=1e-4)
    assert gen.evaluate_generation(m, None, "valid", False, cfg) == ""
    lu = importlib.import_module("src.utils.log_eval_dump_utils")
    gu = importlib.import_module("src.utils.generation_utils")
    assert lu.evaluate_generation is gen.evaluate_generation and gu.sample_per_example is gen.sample_per_example
    assert gen.GenerationConfig().parallel_gen is False and gen.GenerationConfig().pad_token_id == 0


def test_evaluate_generation_restores_umr_clip_when_a_batch_fails(monkeypatch):
    cfg, params = _cfg(False, False)

    def boom(*a, **k):
        raise RuntimeError("sampler failed")
    monkeypatch.setattr(gen, "eval_gen_per_sample", boom)
    with pytest.raises(RuntimeError):
        gen.evaluate_generation(_StubModel(), _BandLoader(params, [1], lambda p: p.umr_clip), "valid", True, cfg)
    assert params.umr_clip == [0.2, 0.7]


def test_accuracy_entries_refuse_cpu_tensors():
    """No eager fall-back: the counts are a kernel."""
    L = importlib.import_module("graph-gpt_amd._lib")
    z = torch.zeros(1, 2, 2, dtype=torch.int64)
    with pytest.raises(L.GgetError):
        gen.cal_gen_acc_batch(gen.GenerationConfig(), z, z, z.view(1, 4))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gen_eval_worker(rank, world, port, q):
    torch.cuda.is_available = lambda: False
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    tr.set_dist_env(backend="gloo")
    cfg, params = _cfg(False, False)
    calls = []
    gen.eval_gen_per_sample = _stub_eval(calls, "sample", float(rank))
    m = _StubModel()
    out = gen.evaluate_generation(m, _BandLoader(params, [3, 2] if rank == 0 else [4], lambda p: p.umr_clip), "test", True, cfg)
    q.put((rank, out, m.mode, params.umr_clip))
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_generation_gathers_sums_and_counts_gloo_world2():
    """world 2 (reference :367-374): the [10] accuracy sums and the sample counts of both ranks are gathered; ranks hold different
    numbers of samples, both return the same string."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_gen_eval_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    (s0, n0), (s1, n1) = _expected([3, 2], 0.0), _expected([4], 1.0)
    want = ",".join(((s0 + s1) / (n0 + n1)).numpy().round(4).astype(str))
    for rank, out, mode, clip in res:
        assert out == want and mode == "train" and clip == [0.2, 0.7]
