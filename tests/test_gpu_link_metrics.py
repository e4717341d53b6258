"""The HIP kernels behind the link-prediction metrics (csrc/metrics.hip, include/gget.h gget_op_link_hits / gget_op_link_mrr), op level
through the C ABI against the NumPy statements of the same counts (graph-gpt_amd/metrics.py `_link_hits_numpy` / `_link_mrr_numpy`,
themselves pinned against OGB's formulas and the reference's reformat functions in tests/test_metrics_link.py), and model level:
`ft_evaluate` on a two-class fixture with dataset_name ogbl-ppa / ogbl-citation2 / ogbl-wikikg2.

Geometry of the launches (csrc/metrics.hip): every streaming launch has workgroups of 256 lanes (kLinkBlock) and at most 1024 of them
(kLinkGrid; menu key 18, `_lib.KEY_LINK_GRID`, sets another cap), the rest is grid-stride.  Hits: a lane takes 4 entries per round
(kLinkVec: one 16-byte score load, two 16-byte label loads) on the body behind the first 16-byte aligned score, single loads for the at
most 3 + 3 entries around it, or for everything when the labels are not aligned there - so one workgroup-round is 1024 entries and one
grid-stride round cap * 1024; the radix select takes 8-bit digits (kLinkBins = 256 bins), four passes, the most significant first.
n = 63 / 65 straddle a wave, 257 a workgroup's lanes, 5000 gives 5 workgroups with a ragged last one; under a cap of 16 workgroups
n = 16384 + 1029 is one full grid-stride round, one more workgroup-round and a ragged tail.  MRR: the scatter takes one entry per lane, the
partition a wave per segment of 256 slots (kLinkSeg, 4 per lane), the row kernel a wave per row, 4 rows per workgroup, lane l the columns
l, l + 64, ...; the sums one workgroup of 256.  cnt_neg = 1 / 8 leave most lanes of a row idle, 64 fills them once, 1000 takes 16 rounds
with a ragged last; P = 65 and 300 are more than one workgroup of rows, and under a cap of 16 more than one grid-stride round (64 rows)."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from _util import load_case

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
met = importlib.import_module("graph-gpt_amd.metrics")
Mod = importlib.import_module("graph-gpt_amd.modeling")
tr = importlib.import_module("graph-gpt_amd.training")

KINDS = ("random", "ties", "equal", "zeros", "lowbyte", "denormal")


def make_scores(n, kind, rng, y):
    if kind == "random":                                     # mixed sign
        return (rng.randn(n) + y).astype(np.float32)
    if kind == "ties":                                       # one decimal: many ties at the K-th value
        return np.round(rng.randn(n) + y, 1).astype(np.float32)
    if kind == "equal":
        return np.full(n, 0.75, np.float32)
    if kind == "zeros":                                      # -0.0 / +0.0 only
        return np.where(rng.rand(n) < 0.5, -0.0, 0.0).astype(np.float32)
    if kind == "lowbyte":                                    # equal but for the lowest mantissa byte: decided by the last radix pass
        bits = np.uint32(0x3F800000) + rng.randint(0, 256, n).astype(np.uint32)
        return (bits.view(np.float32) * np.where(rng.rand(n) < 0.5, -1, 1)).astype(np.float32)
    if kind == "denormal":
        return (rng.randint(-40, 41, n).astype(np.int64) * 2.0 ** -149).astype(np.float32)
    raise KeyError(kind)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ Hits
def run_hits(s, y, k, s_off=0, y_off=0, ws_bytes=None):
    """gget_op_link_hits on device copies that start `s_off` / `y_off` elements into their allocations; (rc, the five outputs)"""
    lib = L.load()
    n = len(s)
    sd, yd = torch.full((n + s_off + 1,), float("nan"), device="cuda"), torch.full((n + y_off + 1,), 7, dtype=torch.int64, device="cuda")
    sd[s_off:s_off + n], yd[y_off:y_off + n] = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
    out = [torch.full((1,), -3, dtype=dt, device="cuda") for dt in (torch.int64, torch.int64, torch.float32, torch.int64, torch.int32)]
    need = int(lib.gget_op_link_hits_workspace(n))
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    rc = lib.gget_op_link_hits(sd[s_off:].data_ptr(), yd[y_off:].data_ptr(), n, k, *[o.data_ptr() for o in out], ws.data_ptr(), nbytes, stream())
    torch.cuda.synchronize()
    return rc, tuple(o.cpu().numpy()[0] for o in out)


def check_hits(s, y, what, offs=(0, 0)):
    n_neg = int((y == 0).sum())
    for k in sorted({1, 20, 100, max(n_neg, 1), n_neg + 1}):
        rc, got = run_hits(s, y, k, *offs)
        assert rc == 0, L.load().gget_last_error()
        n_pos_w, n_neg_w, kth_w, hits_w, bad_w = met._link_hits_numpy(s, y, k)
        assert (int(got[0]), int(got[1]), int(got[3]), int(got[4])) == (n_pos_w, n_neg_w, hits_w, bad_w), (what, k, got)
        assert got[2].tobytes() == np.float32(kth_w).tobytes(), (what, k, got[2], kth_w)            # the bits of kth
        rc2, again = run_hits(s, y, k, *offs)
        assert rc2 == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), (what, k)   # bit-identical from run to run


@pytest.mark.parametrize("n", [1, 63, 65, 257, 5000])
def test_hits_op_matches_numpy_counts(n):
    rng = np.random.RandomState(n)
    for kind in KINDS:
        y = (rng.rand(n) < 0.3).astype(np.int64)
        check_hits(make_scores(n, kind, rng, y), y, f"n={n} {kind}")
    y = (rng.rand(n) < 0.3).astype(np.int64)
    s = make_scores(n, "ties", rng, y)
    check_hits(s, np.ones_like(y), f"n={n} no negative")
    check_hits(s, np.zeros_like(y), f"n={n} no positive")
    # a 3-entry head in front of the aligned body, and labels that are not 16-byte aligned where the scores are: single loads
    check_hits(s, y, f"n={n} head", offs=(1, 1))
    check_hits(s, y, f"n={n} labels off", offs=(1, 0))


def test_hits_op_past_one_grid_stride_round():
    n = 16 * 1024 + 1029
    rng = np.random.RandomState(7)
    with L.debug_menu({L.KEY_LINK_GRID: 16}):
        for kind in ("random", "ties", "lowbyte"):
            y = (rng.rand(n) < 0.3).astype(np.int64)
            check_hits(make_scores(n, kind, rng, y), y, f"n={n} {kind} cap 16", offs=(3, 1))


def test_hits_signed_zero_rule():
    """a +0.0 positive is not a hit over a -0.0 K-th negative; kth reads as +0.0"""
    s = np.array([0.0, -0.0, 1.0, -0.0, -1.0], np.float32)
    y = np.array([1, 1, 1, 0, 0])
    rc, got = run_hits(s, y, 1)
    assert rc == 0 and int(got[3]) == 1 and got[2].tobytes() == np.float32(0.0).tobytes()
    r = met.link_hits(torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda(), 1)
    assert r["hits"] == 1 and r["hits@k"] == 1 / 3 and r == met.link_hits(s, y, 1)


# ------------------------------------------------------------------------------------------------ MRR
def mrr_inputs(P, cnt_neg, kind, blocked, rng):
    n = P * (1 + cnt_neg)
    y = np.concatenate([np.ones(P), np.zeros(P * cnt_neg)]) if blocked else np.tile(np.r_[1, np.zeros(cnt_neg)], P)
    s = make_scores(n, kind, rng, y)
    perm = rng.permutation(n)
    return s[perm], y[perm].astype(np.int64), perm.astype(np.int64)


def run_mrr(s, y, idx, cnt_neg, groups, ws_bytes=None):
    lib = L.load()
    n = len(s)
    P = n // (1 + cnt_neg)
    sd, yd, xd = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(idx).cuda()
    out = [torch.full(shape, -3, dtype=dt, device="cuda") for shape, dt in
           (((1,), torch.int64), ((1,), torch.int64), ((groups, P), torch.int32), ((groups, P), torch.int32), ((3,), torch.int64),
            ((1,), torch.float64), ((2,), torch.int32))]
    need = int(lib.gget_op_link_mrr_workspace(n))
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    rc = lib.gget_op_link_mrr(sd.data_ptr(), yd.data_ptr(), xd.data_ptr(), n, cnt_neg, groups, *[o.data_ptr() for o in out], ws.data_ptr(),
                              nbytes, stream())
    torch.cuda.synchronize()
    return rc, tuple(o.cpu().numpy() for o in out)


def check_mrr(s, y, idx, cnt_neg, groups, what):
    rc, got = run_mrr(s, y, idx, cnt_neg, groups)
    assert rc == 0, L.load().gget_last_error()
    n_pos, n_neg, opt, pes, hits, mrr_sum, n_bad = met._link_mrr_numpy(s, y, idx, cnt_neg, groups)
    assert (int(got[0][0]), int(got[1][0])) == (n_pos, n_neg) and not got[6].any() and not n_bad.any(), (what, got[6])
    assert np.array_equal(got[2], opt) and np.array_equal(got[3], pes) and np.array_equal(got[4], hits), what      # exact integers
    tol = groups * n_pos * 2.0 ** -52 * mrr_sum
    dev = abs(float(got[5][0]) - mrr_sum)
    print(f"{what}: mrr_sum |dev| {dev:.3e} (bound {tol:.3e})")
    assert dev <= tol, (what, got[5][0], mrr_sum)
    rc2, again = run_mrr(s, y, idx, cnt_neg, groups)
    assert rc2 == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), what                            # bit-identical


@pytest.mark.parametrize("cnt_neg", [1, 8, 64, 1000])
@pytest.mark.parametrize("P", [1, 3, 65, 300])
def test_mrr_op_matches_numpy_counts(P, cnt_neg):
    rng = np.random.RandomState(1000 * P + cnt_neg)
    for blocked in (False, True):
        for kind in KINDS:
            s, y, idx = mrr_inputs(P, cnt_neg, kind, blocked, rng)
            for groups in ((1, 2) if cnt_neg % 2 == 0 else (1,)):
                check_mrr(s, y, idx, cnt_neg, groups, f"P={P} cnt_neg={cnt_neg} {kind} blocked={blocked} groups={groups}")


def test_mrr_op_past_one_grid_stride_round():
    rng = np.random.RandomState(11)
    with L.debug_menu({L.KEY_LINK_GRID: 16}):                   # 300 rows > 64 per round; 19 500 slots = 77 segments > 64 per round
        for kind in ("random", "ties"):
            s, y, idx = mrr_inputs(300, 64, kind, False, rng)
            for groups in (1, 2):
                check_mrr(s, y, idx, 64, groups, f"P=300 cnt_neg=64 {kind} cap 16 groups={groups}")


# ------------------------------------------------------------------------------------------------ guards
def test_link_ops_workspace_and_empty_calls():
    lib = L.load()
    rng = np.random.RandomState(3)
    s, y, idx = mrr_inputs(5, 8, "random", False, rng)
    need_h, need_m = int(lib.gget_op_link_hits_workspace(45)), int(lib.gget_op_link_mrr_workspace(45))
    assert need_h > 0 and need_m > 0 and lib.gget_op_link_hits_workspace(0) == 0 and lib.gget_op_link_mrr_workspace(0) == 0
    rc, got = run_hits(s, y, 3, ws_bytes=need_h - 1)
    assert rc != 0 and b"workspace" in lib.gget_last_error() and all(float(g) == -3 for g in got)          # refused before any launch
    rc, got = run_mrr(s, y, idx, 8, 1, ws_bytes=need_m - 1)
    assert rc != 0 and b"workspace" in lib.gget_last_error() and all((g == -3).all() for g in got)
    # n == 0 launches nothing (no pointer is looked at); a negative n, K < 1, a ragged n and an odd cnt_neg with two groups are refused
    assert lib.gget_op_link_hits(None, None, 0, 5, None, None, None, None, None, None, 0, None) == 0
    assert lib.gget_op_link_mrr(None, None, None, 0, 8, 1, None, None, None, None, None, None, None, None, 0, None) == 0
    assert lib.gget_op_link_hits(None, None, -1, 5, None, None, None, None, None, None, 0, None) != 0
    assert lib.gget_op_link_hits(None, None, 4, 0, None, None, None, None, None, None, 0, None) != 0
    assert lib.gget_op_link_mrr(None, None, None, -9, 8, 1, None, None, None, None, None, None, None, None, 0, None) != 0
    assert lib.gget_op_link_mrr(None, None, None, 44, 8, 1, None, None, None, None, None, None, None, None, 0, None) != 0
    assert lib.gget_op_link_mrr(None, None, None, 40, 7, 2, None, None, None, None, None, None, None, None, 0, None) != 0
    e = torch.zeros(0, device="cuda")
    assert met.link_hits(e, e.long(), 5)["hits@k"] == 1.0
    assert np.isnan(met.link_mrr(e, e.long(), e.long(), cnt_neg=8)["mrr"])


def test_link_ops_bad_entry_guards():
    rng = np.random.RandomState(5)
    s, y, idx = mrr_inputs(5, 8, "random", False, rng)
    cu = lambda a: torch.from_numpy(a).cuda()       # noqa: E731
    s2, y2 = s.copy(), y.copy()
    s2[3], y2[7] = np.nan, 2
    rc, got = run_hits(s2, y2, 3)
    want = met._link_hits_numpy(s2, y2, 3)
    assert rc == 0 and int(got[4]) == 2 == want[4] and (int(got[0]), int(got[1]), int(got[3])) == (want[0], want[1], want[3])
    with pytest.raises(ValueError, match="2 entries"):
        met.link_hits(cu(s2), cu(y2), 3)
    rc, got = run_mrr(s2, y2, idx, 8, 1)
    assert rc == 0 and got[6].tolist() == [0, 2] == met._link_mrr_numpy(s2, y2, idx, 8, 1)[6].tolist()
    assert not got[4].any() and got[5][0] == 0 and (got[2] == -3).all()                       # sums 0, the lists not written
    with pytest.raises(ValueError, match="2 entries with a label"):
        met.link_mrr(cu(s2), cu(y2), cu(idx), cnt_neg=8)
    # a duplicated index (its twin's slot stays empty) and indices outside [0, n)
    dup = idx.copy()
    dup[3] = dup[9]
    rc, got = run_mrr(s, y, dup, 8, 1)
    assert rc == 0 and got[6][0] == 1 == met._link_mrr_numpy(s, y, dup, 8, 1)[6][0] and got[5][0] == 0
    with pytest.raises(ValueError, match="not a permutation"):
        met.link_mrr(cu(s), cu(y), cu(dup), cnt_neg=8)
    out = idx.copy()
    out[0], out[1] = -1, len(idx)
    rc, got = run_mrr(s, y, out, 8, 1)
    assert rc == 0 and got[6][0] == 2
    # a label flipped: 6 positives, 39 negatives
    y3 = y.copy()
    y3[np.flatnonzero(y == 0)[0]] = 1
    rc, got = run_mrr(s, y3, idx, 8, 1)
    assert rc == 0 and got[6].tolist() == [0, -1] and (int(got[0][0]), int(got[1][0])) == (6, 39)
    with pytest.raises(ValueError, match="39 negatives for 6 positives"):
        met.link_mrr(cu(s), cu(y3), cu(idx), cnt_neg=8)
    # the surface on clean device tensors equals the host path
    r_dev, r_host = met.link_mrr(cu(s), cu(y), cu(idx), cnt_neg=8, groups=2), met.link_mrr(s, y, idx, cnt_neg=8, groups=2)
    assert np.array_equal(r_dev["optimistic"], r_host["optimistic"]) and np.array_equal(r_dev["pessimistic"], r_host["pessimistic"])
    assert all(r_dev[k] == r_host[k] for k in ("hits@1", "hits@3", "hits@10")) and abs(r_dev["mrr"] - r_host["mrr"]) <= 10 * 2.0 ** -52


# ------------------------------------------------------------------------------------------------ model level
P_EVAL, CNT_NEG = 3, 8
N_EVAL = P_EVAL * (1 + CNT_NEG)


@pytest.fixture(scope="module")
def link_case():
    """the two-class fixture of tests/test_gpu_metrics.py; 27 of its samples stand for 3 positives with 8 negatives each (the labels only
    enter the loss and the metrics), handed to the model in a shuffled order in batches that carry `idx`"""
    z, spec, state, batch = load_case("ft_tiny_f4_b32")
    assert batch["input_ids"].shape[0] >= N_EVAL and spec.num_labels == 2
    cfg = Mod.GraphGPTConfig(hidden_act="gelu", vocab_size=spec.vocab_size, hidden_size=spec.hidden_size,
                             intermediate_size=spec.intermediate_size, num_hidden_layers=spec.num_layers,
                             num_attention_heads=spec.num_heads, max_position_embeddings=spec.max_position,
                             causal_attention=spec.causal, stacked_feat=spec.stacked_feat, num_labels=spec.num_labels,
                             problem_type="single_label_classification", loss_type=None, layer_scale_init_value=spec.layer_scale_init,
                             rms_norm_eps=spec.rms_eps, pad_token_id=spec.pad_token_id,
                             stacked_feat_agg_method="gated" if spec.gated_agg else "sum")
    model = Mod.GraphGPTTaskModel(cfg, seed=1)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    labels = np.tile(np.r_[1, np.zeros(CNT_NEG)], P_EVAL).astype(np.int64)            # label of sample j (= its idx)
    order = np.random.RandomState(4).permutation(N_EVAL)
    loader = []
    for a in range(0, N_EVAL, 10):
        rows = order[a:a + 10]
        d = {k: torch.from_numpy(np.ascontiguousarray(v[rows])) for k, v in batch.items() if k not in ("lengths", "task_labels")}
        d["task_labels"], d["idx"] = torch.from_numpy(labels[rows]), torch.from_numpy(rows.astype(np.int64))
        loader.append(d)
    return model.cuda(), loader, labels, order


@pytest.mark.parametrize("dataset_name", ["ogbl-ppa", "ogbl-citation2", "ogbl-wikikg2"])
def test_ft_evaluate_link_datasets_on_device(link_case, dataset_name, monkeypatch):
    model, loader, labels, order = link_case
    calls = []
    for name in ("link_hits", "link_mrr", "rank_metrics"):
        real = getattr(met, name)
        monkeypatch.setattr(met, name, lambda *a, _n=name, _r=real, **k: (calls.append((_n, getattr(getattr(a[0], "device", None), "type", "host"))), _r(*a, **k))[1])
    loss, m, res, d = tr.ft_evaluate(model, loader, problem_type="single_label_classification", num_labels=2, dataset_name=dataset_name,
                                     cnt_neg=CNT_NEG)
    assert model.training and m.on_device and np.isfinite(float(loss))
    assert calls == [("rank_metrics", "cuda"), ("link_hits" if dataset_name == "ogbl-ppa" else "link_mrr", "cuda")], calls
    assert all(v.device.type == "cpu" for v in d.values())                      # the one host transfer, after the metrics
    assert d["idx"].tolist() == order.tolist() and d["y_true"].tolist() == labels[order].tolist()
    s, y, idx = d["y_pred"].numpy(), d["y_true"].numpy(), d["idx"].numpy()
    assert s.dtype == np.float32 and np.isfinite(s).all()
    # the host path on the same logits
    if dataset_name == "ogbl-ppa":
        assert res == {"hits@100": 1.0} == met.evaluate_ogb(dataset_name, {"y_true": y, "y_pred": s})      # 24 negatives < 100
        for k in (1, 3, 24):
            r_dev, r_host = met.link_hits(d["y_pred"].cuda(), d["y_true"].cuda(), k), met.link_hits(s, y, k)
            assert r_dev == r_host, (k, r_dev, r_host)                           # integers, the bits of kth and the ratio
    else:
        host = met.evaluate_ogb(dataset_name, {"y_true": y, "y_pred": s, "idx": idx}, cnt_neg=CNT_NEG)
        assert list(res) == list(host) == ["hits@1_list", "hits@3_list", "hits@10_list", "ema_mrr_list"]
        assert all(res[k] == host[k] for k in list(res)[:3])                     # integer counts over groups * P
        groups = met.MRR_DATASETS[dataset_name]
        assert abs(res["ema_mrr_list"] - host["ema_mrr_list"]) <= groups * P_EVAL * 2.0 ** -52 * host["ema_mrr_list"]
    # the metric object: accuracy from an integer count, AUROC as a count ratio - both exact against the host statements
    prob = m.sync_dict()["prob"]
    assert prob.device.type == "cuda"
    p = prob.cpu().numpy()
    assert m.acc == float(((p > 0.5).astype(np.int64) == y).mean())
    r = met._rank_counts_numpy(p[:, None], y[:, None].astype(np.float32))
    assert m.auroc == float(r[2][0]) / (2.0 * float(r[0][0]) * float(r[1][0]))
    assert abs(m.auroc - met.auroc(p, y)) <= 4 * 2.0 ** -52
    # ogbl-citation2 / ogbl-wikikg2 are not ranked on the training split
    if dataset_name != "ogbl-ppa":
        calls.clear()
        _, m2, res2, _ = tr.ft_evaluate(model, loader, problem_type="single_label_classification", num_labels=2, dataset_name=dataset_name,
                                        eval_name="train", cnt_neg=CNT_NEG)
        assert res2 == {"auroc": m.auroc, "acc": m.acc} and calls == [("rank_metrics", "cuda")]
