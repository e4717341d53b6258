"""A14, link prediction on the host: `link_hits` / `link_mrr` (the NumPy statements of the counts of include/gget.h gget_op_link_hits /
gget_op_link_mrr), the ogbl-ppa / ogbl-ddi / ogbl-citation2 / ogbl-wikikg2 entries of `evaluate_ogb` and the `on_device` form of
SingleLabelClassificationMetrics, against an independent torch-CPU statement of OGB's formulas (`_eval_hits`: torch.topk(neg, K)[0][-1]
and a compare-and-sum; `_eval_mrr`: (neg > pos).sum(1), (neg >= pos).sum(1), rank = their mean + 1) and against
tests/golden/link_reformat.npz, which holds what the REAL reference's `_reformat_pred_for_hr_eval` / `_reformat_pred_for_mrr_eval`
(src/utils/ogb_utils.py:141-170) returned for shuffled inputs (tools/make_golden.py link_reformat_fixture).
Counts are integers and compared exactly; a mean of R reciprocal ranks in fp64 against another summation order: R * 2^-52 relative."""
import importlib
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _util import GOLDEN

M = importlib.import_module("graph-gpt_amd.metrics")
tr = importlib.import_module("graph-gpt_amd.training")


# ------------------------------------------------------------------------------------------------ OGB's formulas in torch (CPU)
def ogb_hits(pos, neg, k):
    pos, neg = torch.as_tensor(pos), torch.as_tensor(neg)
    if len(neg) < k:
        return 1.0
    kth = torch.topk(neg, k)[0][-1]
    return float((pos > kth).sum()) / len(pos)


def ogb_mrr(pos, neg):
    """{hits@1_list, hits@3_list, hits@10_list, mrr_list} of OGB `_eval_mrr` (torch branch), in fp64"""
    pos, neg = torch.as_tensor(pos).view(-1, 1), torch.as_tensor(neg)
    optimistic = (neg > pos).sum(dim=1)
    pessimistic = (neg >= pos).sum(dim=1)
    rank = 0.5 * (optimistic + pessimistic).double() + 1
    return {"hits@1_list": (rank <= 1).double(), "hits@3_list": (rank <= 3).double(), "hits@10_list": (rank <= 10).double(),
            "mrr_list": 1.0 / rank}, optimistic.numpy(), pessimistic.numpy()


def torch_reformat_mrr(idx, y_true, y_pred, cnt_neg):
    order = torch.sort(torch.as_tensor(idx))[1]
    y, s = torch.as_tensor(y_true)[order], torch.as_tensor(y_pred)[order]
    return s[y.bool()], s[~y.bool()].reshape(-1, cnt_neg)


def mrr_case(P, cnt_neg, seed, kind="random", blocked=False):
    """(scores, labels, idx) of P positives with cnt_neg negatives each, shuffled; in idx order every positive stands in front of its
    negatives, or all positives first (`blocked`)"""
    rng = np.random.RandomState(seed)
    n = P * (1 + cnt_neg)
    y = np.concatenate([np.ones(P), np.zeros(P * cnt_neg)]) if blocked else np.tile(np.r_[1, np.zeros(cnt_neg)], P)
    s = (rng.randn(n) + y).astype(np.float32)
    if kind == "ties":
        s = np.round(s, 1)
    elif kind == "equal":
        s[:] = 0.75
    elif kind == "zeros":
        s = np.where(rng.rand(n) < 0.5, -0.0, 0.0).astype(np.float32)
    perm = rng.permutation(n)
    return s[perm], y[perm].astype(np.int64), perm.astype(np.int64)


def hits_case(n, seed, kind="random", pos_rate=0.3):
    rng = np.random.RandomState(seed)
    y = (rng.rand(n) < pos_rate).astype(np.int64)
    s = (rng.randn(n) + y).astype(np.float32)
    if kind == "ties":
        s = np.round(s, 1)
    elif kind == "equal":
        s[:] = 0.75
    elif kind == "zeros":
        s = np.where(rng.rand(n) < 0.5, -0.0, 0.0).astype(np.float32)
    return s, y


# ------------------------------------------------------------------------------------------------ link_hits
@pytest.mark.parametrize("kind", ["random", "ties", "equal", "zeros"])
@pytest.mark.parametrize("n", [1, 65, 700])
def test_link_hits_numpy_matches_topk_statement(n, kind):
    s, y = hits_case(n, seed=n, kind=kind)
    pos, neg = s[y == 1], s[y == 0]
    for k in sorted({1, 20, 100, max(len(neg), 1), len(neg) + 1}):
        r = M.link_hits(s, y, k)
        assert (r["n_pos"], r["n_neg"]) == (len(pos), len(neg))
        if len(neg) < k:
            assert r["kth"] == -np.inf and r["hits"] == len(pos) and r["hits@k"] == 1.0
            continue
        kth = torch.topk(torch.from_numpy(neg), k)[0][-1].numpy()
        assert r["kth"] == kth and r["kth"].dtype == np.float32
        assert r["kth"] != 0 or not np.signbit(r["kth"])                               # a zero reads as +0.0
        assert r["hits"] == int((pos > kth).sum())
        if len(pos):
            assert r["hits@k"] == ogb_hits(pos, neg, k) == M.hits_at_k(pos, neg, k)
    # tensors take the same path as arrays
    assert M.link_hits(torch.from_numpy(s), torch.from_numpy(y), 3)["hits"] == M.link_hits(s, y, 3)["hits"]


def test_link_hits_signed_zero_and_errors():
    # K-th negative is -0.0: a +0.0 positive is NOT a hit (a float comparison), and kth reads as +0.0
    s = np.array([0.0, -0.0, 1.0, -0.0, -1.0], np.float32)
    y = np.array([1, 1, 1, 0, 0])
    r = M.link_hits(s, y, 1)
    assert r["hits"] == 1 and r["kth"] == 0 and not np.signbit(r["kth"])
    with pytest.raises(ValueError, match="1 entries"):
        M.link_hits(s, np.array([1, 1, 2, 0, 0]), 1)
    with pytest.raises(ValueError, match="1 entries"):
        M.link_hits(np.array([0.0, np.nan, 1.0, 0.0, -1.0], np.float32), y, 1)
    with pytest.raises(ValueError):
        M.link_hits(s, y, 0)
    with pytest.raises(ValueError):
        M.link_hits(s[:, None], y[:, None], 1)
    assert M.link_hits(np.zeros(0, np.float32), np.zeros(0, np.int64), 5)["hits@k"] == 1.0


# ------------------------------------------------------------------------------------------------ link_mrr
@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("kind", ["random", "ties", "equal", "zeros"])
@pytest.mark.parametrize("P,cnt_neg", [(1, 1), (3, 8), (65, 64), (12, 1000)])
def test_link_mrr_numpy_matches_ogb_statement(P, cnt_neg, kind, blocked):
    s, y, idx = mrr_case(P, cnt_neg, seed=P + cnt_neg, kind=kind, blocked=blocked)
    pos, neg = torch_reformat_mrr(idx, y, s, cnt_neg)
    want, opt, pes = ogb_mrr(pos, neg)
    r = M.link_mrr(s, y, idx, cnt_neg=cnt_neg)
    assert r["optimistic"].shape == (1, P) and np.array_equal(r["optimistic"][0], opt) and np.array_equal(r["pessimistic"][0], pes)
    for k in (1, 3, 10):
        assert r[f"hits@{k}"] == float(want[f"hits@{k}_list"].mean())             # integer counts over P
    assert abs(r["mrr"] - float(want["mrr_list"].mean())) <= P * 2.0 ** -52 * r["mrr"]
    assert r["mrr"] == M.mrr(pos.numpy(), neg.numpy())                              # the existing definition, to the bit
    if kind in ("equal", "zeros"):                                                  # every negative ties: rank = cnt_neg / 2 + 1
        assert not r["optimistic"].any() and (r["pessimistic"] == cnt_neg).all() and abs(r["mrr"] - 1 / (cnt_neg / 2 + 1)) < 1e-15
    if cnt_neg % 2 == 0:                                                            # wikikg2: head / tail = two calls on the even / odd columns
        r2 = M.link_mrr(s, y, idx, cnt_neg=cnt_neg, groups=2)
        halves = []
        for g in (0, 1):
            w, o, p = ogb_mrr(pos, neg[:, g::2])
            assert np.array_equal(r2["optimistic"][g], o) and np.array_equal(r2["pessimistic"][g], p)
            halves.append(w)
        both = {k: torch.cat([halves[0][k], halves[1][k]]) for k in halves[0]}      # ogb_utils.py:121-126
        for k in (1, 3, 10):
            assert r2[f"hits@{k}"] == float(both[f"hits@{k}_list"].mean())
        assert abs(r2["mrr"] - float(both["mrr_list"].mean())) <= 2 * P * 2.0 ** -52 * r2["mrr"]
    else:
        with pytest.raises(ValueError, match="groups"):
            M.link_mrr(s, y, idx, cnt_neg=cnt_neg, groups=2)


def test_link_reformat_matches_the_reference_fixture():
    """the sort / mask / reshape, against what the real reference returned"""
    z = np.load(os.path.join(GOLDEN, "link_reformat.npz"))
    for tag in ("a", "b"):
        idx, y, s, cnt_neg = z[f"{tag}_idx"], z[f"{tag}_y_true"], z[f"{tag}_y_pred"], int(z[f"{tag}_cnt_neg"])
        pos, neg = z[f"{tag}_mrr_pos"], z[f"{tag}_mrr_neg"]
        assert neg.shape == (len(pos), cnt_neg) and not np.array_equal(idx, np.arange(len(idx)))
        want, opt, pes = ogb_mrr(pos, neg)
        r = M.link_mrr(s, y, idx, cnt_neg=cnt_neg)
        assert np.array_equal(r["optimistic"][0], opt) and np.array_equal(r["pessimistic"][0], pes)
        assert r["mrr"] == M.mrr(pos, neg)
        res = M.evaluate_ogb("ogbl-citation2", {"y_true": y, "y_pred": s, "idx": idx}, cnt_neg=cnt_neg)
        assert res["ema_mrr_list"] == r["mrr"] and res["hits@3_list"] == float(want["hits@3_list"].mean())
        # a different shuffle of the same samples gives the same lists: only idx decides the order
        p2 = np.random.RandomState(3).permutation(len(idx))
        r2 = M.link_mrr(s[p2], y[p2], idx[p2], cnt_neg=cnt_neg)
        assert np.array_equal(r2["optimistic"], r["optimistic"]) and r2["mrr"] == r["mrr"]
        hr_pos, hr_neg = z[f"{tag}_hr_pos"], z[f"{tag}_hr_neg"]
        for k in (1, 3, len(hr_neg), len(hr_neg) + 1):
            h = M.link_hits(s, y, k)
            assert (h["n_pos"], h["n_neg"]) == (len(hr_pos), len(hr_neg)) and h["hits@k"] == ogb_hits(hr_pos, hr_neg, k)


def test_link_mrr_errors():
    s, y, idx = mrr_case(5, 4, seed=1)
    M.link_mrr(s, y, idx, cnt_neg=4)
    dup = idx.copy()
    dup[3] = dup[7]
    with pytest.raises(ValueError, match="not a permutation.*1 entries"):
        M.link_mrr(s, y, dup, cnt_neg=4)
    for bad in (-1, len(idx)):
        out = idx.copy()
        out[0] = bad
        with pytest.raises(ValueError, match="not a permutation"):
            M.link_mrr(s, y, out, cnt_neg=4)
    y2 = y.copy()
    y2[np.flatnonzero(y == 0)[0]] = 1                       # 6 positives, 19 negatives
    with pytest.raises(ValueError, match="19 negatives for 6 positives"):
        M.link_mrr(s, y2, idx, cnt_neg=4)
    y2[np.flatnonzero(y == 0)[0]] = 2
    with pytest.raises(ValueError, match="1 entries with a label"):
        M.link_mrr(s, y2, idx, cnt_neg=4)
    s2 = s.copy()
    s2[4] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        M.link_mrr(s2, y, idx, cnt_neg=4)
    with pytest.raises(ValueError, match="multiple of 1 \\+ cnt_neg"):
        M.link_mrr(s[:-1], y[:-1], idx[:-1], cnt_neg=4)
    with pytest.raises(ValueError):
        M.link_mrr(s, y, idx[:-1], cnt_neg=4)
    with pytest.raises(ValueError):
        M.link_mrr(s, y, idx, cnt_neg=0)


# ------------------------------------------------------------------------------------------------ evaluate_ogb
def test_evaluate_ogb_link_entries():
    s, y, idx = mrr_case(9, 8, seed=5, kind="ties")
    pos, neg = torch_reformat_mrr(idx, y, s, 8)
    d = {"y_true": y, "y_pred": s, "idx": idx}
    # ogbl-citation2: the means under the reference's key names (ogb_utils.py:100-101)
    res = M.evaluate_ogb("ogbl-citation2", d, cnt_neg=8)
    want, _, _ = ogb_mrr(pos, neg)
    assert list(res) == ["hits@1_list", "hits@3_list", "hits@10_list", "ema_mrr_list"]
    assert [res[k] for k in list(res)[:3]] == [float(want[k].mean()) for k in list(res)[:3]]
    assert abs(res["ema_mrr_list"] - float(want["mrr_list"].mean())) <= 9 * 2.0 ** -52
    assert res == M.evaluate_ogb("ogbl-citation2", {k: torch.from_numpy(v) for k, v in d.items()}, cnt_neg=8)
    # ogbl-wikikg2: head / tail = the even / odd columns, each a groups = 1 problem of its own
    res2 = M.evaluate_ogb("ogbl-wikikg2", d, cnt_neg=8)
    parts = []
    for g in (0, 1):
        keep = np.r_[True, (np.arange(8) % 2 == g)]                       # per sample in idx order: the positive and its group's negatives
        sel = np.flatnonzero(np.tile(keep, 9))
        inv = np.argsort(idx)                                             # position in the shuffled lists of sample j
        sub = inv[sel]
        parts.append(M.link_mrr(s[sub], y[sub], np.arange(len(sub)), cnt_neg=4))
    for k in (1, 3, 10):
        assert res2[f"hits@{k}_list"] == (parts[0][f"hits@{k}"] + parts[1][f"hits@{k}"]) / 2
    assert abs(res2["ema_mrr_list"] - (parts[0]["mrr"] + parts[1]["mrr"]) / 2) <= 18 * 2.0 ** -52
    # the default is the reference's 1000 negatives per positive
    with pytest.raises(ValueError, match="1001"):
        M.evaluate_ogb("ogbl-citation2", d)
    # ogbl-ddi: Hits@20; ogbl-ppa: unchanged for NumPy input
    s, y = hits_case(400, seed=6, kind="ties")
    assert M.evaluate_ogb("ogbl-ddi", {"y_true": y, "y_pred": s}) == {"hits@20": ogb_hits(s[y == 1], s[y == 0], 20)}
    assert M.evaluate_ogb("ogbl-ppa", {"y_true": y, "y_pred": s}) == {"hits@100": M.hits_at_k(s[y == 1], s[y == 0], 100)}
    assert M.evaluate_ogb("ogbl-ppa", {"y_true": torch.from_numpy(y), "y_pred": torch.from_numpy(s)}) == \
        {"hits@100": ogb_hits(s[y == 1], s[y == 0], 100)}
    assert M.evaluate_ogb("ogbl-ddi", {"y_true": y[:30], "y_pred": s[:30]}) == {"hits@20": 1.0 if (y[:30] == 0).sum() < 20 else
                                                                                  ogb_hits(s[:30][y[:30] == 1], s[:30][y[:30] == 0], 20)}


# ------------------------------------------------------------------------------------------------ the metric object, on_device form
def test_single_label_on_device_keeps_tensors_and_agrees_with_host_form():
    class Spy(torch.Tensor):
        @staticmethod
        def __new__(cls, x):
            return torch.Tensor._make_subclass(cls, x)

        def cpu(self, *a, **k):
            assert not Spy.in_update, ".cpu() inside update()"
            return torch.Tensor.cpu(self, *a, **k)

    rng = np.random.RandomState(0)
    lg = np.round(rng.randn(40, 2), 1).astype(np.float32)
    y = (rng.rand(40) < 0.4).astype(np.int64)
    dev, host = M.get_metrics("single_label_classification", None, 2, on_device=True), M.get_metrics("single_label_classification", None, 2)
    assert dev.on_device and not host.on_device
    assert not M.get_metrics("single_label_classification", None, 5, on_device=True).on_device
    for a in range(0, 40, 16):
        sl = slice(a, a + 16)
        Spy.in_update = True
        dev.update(Spy(torch.from_numpy(lg[sl])), Spy(torch.from_numpy(y[sl])), Spy(torch.arange(40)[sl]))
        Spy.in_update = False
        host.update(torch.from_numpy(lg[sl]), torch.from_numpy(y[sl]), torch.arange(40)[sl])
    dev.compute()
    host.compute()
    assert dev.acc == host.acc                                              # an integer count over n
    assert abs(dev.auroc - host.auroc) <= 4 * 2.0 ** -52                    # the same pair count: two fp64 evaluations of a ratio <= 1
    for k, v in host.to_dict().items():
        assert torch.equal(dev.to_dict()[k], v)
    assert torch.equal(dev.sync_dict()["prob"], host.sync_dict()["prob"])


# ------------------------------------------------------------------------------------------------ ft_evaluate, gloo world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


P_ALL, CNT_NEG = 5, 8
N_ALL = P_ALL * (1 + CNT_NEG)


def _all_samples():
    """sample j of the evaluation set: (score, label); j is its idx"""
    s, y, idx = mrr_case(P_ALL, CNT_NEG, seed=33, kind="ties")
    inv = np.argsort(idx)
    return s[inv], y[inv]


class _FakeLinkModel:
    """Stands in for GraphGPTTaskModel: the edge score of a sample is looked up by the sample's id"""
    device = torch.device("cpu")

    def __init__(self, scores):
        self.mode, self.scores = "train", torch.from_numpy(scores)

    def eval(self):
        self.mode = "eval"

    def train(self):
        self.mode = "train"

    def __call__(self, **kw):
        assert self.mode == "eval"
        s = self.scores[kw["input_ids"][:, 0, 0]]
        return types.SimpleNamespace(task_loss=s.mean(), task_logits=torch.stack([torch.zeros_like(s), s], dim=1))


def _run_eval(ids, dataset_name, eval_name="valid"):
    s, y = _all_samples()
    m = _FakeLinkModel(s)
    loader = []
    for a in range(0, len(ids), 4):
        b = torch.tensor(ids[a:a + 4])
        loader.append({"input_ids": b.view(-1, 1, 1).repeat(1, 3, 2), "attention_mask": torch.ones(len(b), 3, dtype=torch.int64),
                       "position_ids": torch.arange(3)[None].repeat(len(b), 1), "task_labels": torch.from_numpy(y)[b], "idx": b})
    loss, met, res, d = tr.ft_evaluate(m, loader, problem_type="single_label_classification", num_labels=2, dataset_name=dataset_name,
                                       eval_name=eval_name, cnt_neg=CNT_NEG)
    return res, {k: v.tolist() for k, v in d.items()}, m.mode


NAMES = ("ogbl-citation2", "ogbl-wikikg2", "ogbl-ddi")


def _link_worker(rank, world, port, q):
    torch.cuda.is_available = lambda: False                     # the host path (gloo, CPU tensors) on any box
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    tr.set_dist_env(backend="gloo")
    mine = tr.eval_rank_sampler(list(range(N_ALL)), world, rank)
    q.put((rank, len(mine), [_run_eval(mine, name) for name in NAMES]))
    dist.barrier()
    dist.destroy_process_group()


def test_ft_evaluate_link_datasets_single_process():
    s, y = _all_samples()
    order = list(np.random.RandomState(2).permutation(N_ALL))               # the loader's order does not matter: idx does
    res, d, mode = _run_eval(order, "ogbl-citation2")
    assert mode == "train" and d["idx"] == order
    want = M.link_mrr(s, y, np.arange(N_ALL), cnt_neg=CNT_NEG)
    assert res == {"hits@1_list": want["hits@1"], "hits@3_list": want["hits@3"], "hits@10_list": want["hits@10"], "ema_mrr_list": want["mrr"]}
    # not ranked on the training split (log_eval_dump_utils.py:153-160): the metric object's own results
    res_t, _, _ = _run_eval(order, "ogbl-citation2", eval_name="train")
    assert set(res_t) == {"auroc", "acc"}
    assert set(_run_eval(order, "ogbl-ddi", eval_name="train")[0]) == {"hits@20"}


def test_ft_evaluate_link_gloo_world2_equals_single_process():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_link_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = sorted(q.get(timeout=120) for _ in range(2))
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    assert [g[1] for g in got] == [(N_ALL + 1) // 2, N_ALL // 2]
    order = list(range(0, N_ALL, 2)) + list(range(1, N_ALL, 2))              # rank 0's samples, then rank 1's: the gathered order
    for k, name in enumerate(NAMES):
        res, d, mode = _run_eval(order, name)
        assert mode == "train" and res is not None and not set(res) & {"auroc", "acc"}
        for rank, _, out in got:
            assert out[k] == (res, d, "train")                                   # exactly: integer counts, one fp64 sum in idx order
