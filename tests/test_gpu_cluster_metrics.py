"""The HIP kernel behind the graph-clustering metrics (csrc/metrics.hip, include/gget.h gget_op_cluster_metrics), op level through the
C ABI against the NumPy statement of the same counts (graph-gpt_amd/metrics.py `_cluster_numpy`, itself pinned against the set statement
of tests/_cluster_ref.py and the reference fixture in tests/test_metrics_cluster.py), and model level: `ft_evaluate(...,
metric_type="graph_clustering")` on the tiny token_ce / token_ce_intra fixtures, both token layouts.

Geometry (csrc/metrics.hip): one workgroup of 256 lanes per sample, grid-stride over the samples past the cap of 2048 workgroups (menu
key 18, `_lib.KEY_LINK_GRID`, sets another cap).  C <= 64: tiles of whole rows, at most 4096 floats, are staged in LDS (16-byte loads
behind the first 16-byte aligned float of the tile, single loads for the at most 3 + 3 floats around it), then a lane scans one row;
C > 64: a wave per row, lane l the columns l, l + 64, ...  S = 63 / 65 straddle a wave of rows, 257 / 300 the workgroup's lanes (a
second round of rows in one tile at C = 8; at C = 64 a tile holds 64 rows, so 257 rows are five tiles with a one-row last one), C = 64
/ 65 the two arg-max paths, C = 1000 takes 16 columns per lane with a ragged last round, B = 300 under a cap of 16 workgroups is 19
grid-stride rounds, C = 2048 is the class limit (32 KiB of tables)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch

import _cluster_ref as R
from _util import GOLDEN, spec_mod, weights_mod

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
met = importlib.import_module("graph-gpt_amd.metrics")
Mod = importlib.import_module("graph-gpt_amd.modeling")
tr = importlib.import_module("graph-gpt_amd.training")

SHAPES = [(1, 1, 2), (3, 8, 3), (5, 63, 8), (5, 65, 8), (2, 257, 64), (2, 300, 65), (1, 1024, 1000), (300, 16, 8), (2, 40, 2048)]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_cluster(p, y, raw, ncls, p_off=1, y_off=1, totals=None):
    """gget_op_cluster_metrics on device copies that start `p_off` / `y_off` elements into their allocations (labels and raw_node_idx
    alike); (rc, y_pred, counts, totals) with the outputs as NumPy arrays and `totals` the device tensor that was added to"""
    lib = L.load()
    B, S = y.shape
    is_logits = p.ndim == 3
    pd = torch.full((p.size + p_off + 1,), float("nan") if is_logits else 7, dtype=torch.float32 if is_logits else torch.int64, device="cuda")
    yd, rd = (torch.full((y.size + y_off + 1,), 7, dtype=torch.int64, device="cuda") for _ in range(2))
    pd[p_off:p_off + p.size] = torch.from_numpy(p.reshape(-1)).cuda()
    yd[y_off:y_off + y.size], rd[y_off:y_off + y.size] = torch.from_numpy(y.reshape(-1)).cuda(), torch.from_numpy(raw.reshape(-1)).cuda()
    y_pred = torch.full((B * S + 1,), -3, dtype=torch.int64, device="cuda")
    counts = torch.full((B * 4 + 1,), -3, dtype=torch.int32, device="cuda")
    totals = torch.zeros(4, dtype=torch.int64, device="cuda") if totals is None else totals
    rc = lib.gget_op_cluster_metrics(pd[p_off:].data_ptr(), int(is_logits), yd[y_off:].data_ptr(), rd[y_off:].data_ptr(), B, S, ncls,
                                     y_pred.data_ptr(), counts.data_ptr(), totals.data_ptr(), stream())
    torch.cuda.synchronize()
    assert int(y_pred[-1]) == -3 and int(counts[-1]) == -3                       # nothing written behind the outputs
    return rc, y_pred[:-1].reshape(B, S).cpu().numpy(), counts[:-1].reshape(B, 4).cpu().numpy(), totals


def check_cluster(p, y, raw, ncls, what, offs=(1, 1)):
    rc, y_pred, counts, totals = run_cluster(p, y, raw, ncls, *offs)
    assert rc == 0, L.load().gget_last_error()
    want_pred, want_counts, want_totals = met._cluster_numpy(p, y, raw, ncls)
    assert np.array_equal(y_pred, want_pred), (what, np.argwhere(y_pred != want_pred)[:4])
    assert np.array_equal(counts, want_counts), (what, np.argwhere(counts != want_counts)[:4])
    assert totals.cpu().numpy().tolist() == want_totals.tolist(), (what, totals, want_totals)
    rc2, y_pred2, counts2, totals2 = run_cluster(p, y, raw, ncls, *offs, totals=totals)       # the second call adds to the first one's totals
    assert rc2 == 0 and y_pred2.tobytes() == y_pred.tobytes() and counts2.tobytes() == counts.tobytes(), what     # bit-identical
    assert totals2.cpu().numpy().tolist() == (2 * want_totals).tolist(), what
    return want_totals


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cluster_op_matches_numpy_counts(shape):
    B, S, ncls = shape
    rng = np.random.RandomState(B * 1000 + S * 10 + ncls)
    y, raw = R.make_labels(B, S, ncls, "mixed", rng)
    for kind in R.LOGIT_KINDS:
        check_cluster(R.make_logits(B, S, ncls, kind, rng), y, raw, ncls, f"{shape} {kind}")
    lg = R.make_logits(B, S, ncls, "ties", rng)
    for lab_kind in R.LABEL_KINDS[1:]:
        y2, raw2 = R.make_labels(B, S, ncls, lab_kind, rng)
        tot = check_cluster(lg, y2, raw2, ncls, f"{shape} {lab_kind}")
        if lab_kind == "bad":
            assert tot[3] == (2 if B * S > 1 else 1)
    # every misalignment of the logits against 16 bytes, with the labels 16-byte aligned or not
    for offs in ((0, 0), (2, 0), (3, 1), (1, 0)):
        check_cluster(lg, y, raw, ncls, f"{shape} offsets {offs}", offs)
    # integer predictions in place of logits; some outside [0, C)
    pred = rng.randint(0, ncls, (B, S)).astype(np.int64)
    check_cluster(pred, y, raw, ncls, f"{shape} given predictions")
    pred[rng.rand(B, S) < 0.2] = ncls + 3
    pred[0, 0] = -1
    check_cluster(pred, y, raw, ncls, f"{shape} given predictions, some out of range")


def test_cluster_op_past_one_grid_stride_round():
    B, S, ncls = 300, 16, 8
    rng = np.random.RandomState(17)
    with L.debug_menu({L.KEY_LINK_GRID: 16}):
        for lab_kind in ("mixed", "first_empty", "bad"):
            y, raw = R.make_labels(B, S, ncls, lab_kind, rng)
            check_cluster(R.make_logits(B, S, ncls, "ties", rng), y, raw, ncls, f"cap 16 {lab_kind}", (3, 1))


def test_cluster_op_guards_and_class_limit():
    lib = L.load()
    assert L.CLUSTER_MAX_C == 2048
    B, S, ncls = 2, 5, L.CLUSTER_MAX_C + 1
    rng = np.random.RandomState(2)
    lg = R.make_logits(B, S, ncls, "ties", rng)
    y, raw = R.make_labels(B, S, ncls, "mixed", rng)
    rc, y_pred, counts, totals = run_cluster(lg, y, raw, ncls)
    assert rc != 0 and b"2048" in lib.gget_last_error() and (y_pred == -3).all() and (counts == -3).all() and not totals.any()
    # the surface takes the host path for such a C and still answers with device tensors
    cu = lambda a: torch.from_numpy(a).cuda()       # noqa: E731
    r = met.cluster_metrics(cu(lg), cu(y), cu(raw), ncls)
    want = met._cluster_numpy(lg, y, raw, ncls)
    assert all(r[k].device.type == "cuda" and np.array_equal(r[k].cpu().numpy(), w) for k, w in zip(("y_pred", "counts", "totals"), want))
    # empty calls launch nothing; negative sizes, C < 1 and null pointers are refused
    assert lib.gget_op_cluster_metrics(None, 1, None, None, 0, 5, 3, None, None, None, None) == 0
    assert lib.gget_op_cluster_metrics(None, 1, None, None, 4, 0, 3, None, None, None, None) == 0
    assert lib.gget_op_cluster_metrics(None, 1, None, None, -1, 5, 3, None, None, None, None) != 0
    assert lib.gget_op_cluster_metrics(None, 1, None, None, 4, 5, 0, None, None, None, None) != 0
    assert lib.gget_op_cluster_metrics(None, 1, None, None, 4, 5, 3, None, None, None, None) != 0 and b"null" in lib.gget_last_error()
    e = met.cluster_metrics(torch.zeros(0, 4, 3, device="cuda"), torch.zeros(0, 4, dtype=torch.long, device="cuda"),
                            torch.zeros(0, 4, dtype=torch.long, device="cuda"), 3)
    assert tuple(e["counts"].shape) == (0, 4) and not e["totals"].any()


def test_metric_object_on_device_equals_host_and_bad_labels_raise():
    z = np.load(os.path.join(GOLDEN, "cluster_metrics.npz"))
    host, dev = met.GraphClusteringMetrics(num_labels=5), met.GraphClusteringMetrics(num_labels=5)
    for k in range(3):
        args = [torch.from_numpy(z[f"{n}_{k}"]) for n in ("logits", "labels", "idx", "raw_node_idx")]
        host.update(args[0], args[1], (args[2], args[3]))
        dev.update(args[0].cuda(), args[1].cuda(), (args[2].cuda(), args[3]))              # raw_node_idx as the collator delivers it
    host.compute()
    dev.compute()
    assert dev.totals.device.type == "cuda" and dev.results_in_tuple() == host.results_in_tuple() and dev.n_empty == 0
    assert dev.ls_recall.tobytes() == z["ls_recall"].tobytes() and dev.ls_precision.tobytes() == z["ls_precision"].tobytes()
    d = dev.to_dict()
    assert all(v.device.type == "cuda" and np.array_equal(v.cpu().numpy(), z[k]) for k, v in d.items())
    bad = met.GraphClusteringMetrics(num_labels=5)
    y = z["labels_0"].copy()
    y[0, 0], y[1, 1] = 5, -1                                                               # (both positions are selected in the fixture)
    assert z["raw_node_idx_0"][0, 0] != -100 and z["raw_node_idx_0"][1, 1] != -100
    bad.update(torch.from_numpy(z["logits_0"]).cuda(), torch.from_numpy(y).cuda(), (torch.from_numpy(z["idx_0"]).cuda(),
                                                                                     torch.from_numpy(z["raw_node_idx_0"]).cuda()))
    assert int(bad.totals[3]) == 2
    with pytest.raises(ValueError, match="2 selected positions"):
        bad.compute()


# ------------------------------------------------------------------------------------------------ model level
def _token_case(loss_type):
    tag, ncls = ("ft_tiny_tokence", 7) if loss_type == "token_ce" else ("ft_tiny_tokence_intra", 5)
    z = np.load(os.path.join(GOLDEN, tag + ".npz"))
    spec = spec_mod.spec_from_size("tiny", kind=spec_mod.KIND_TASK, vocab_size=756, stacked_feat=13, next_n_token=1, num_labels=ncls)
    seed, std, hstd = z["meta_init"]
    state = weights_mod.make_state_dict(spec, seed=int(seed), std=float(std), head_std=float(hstd))
    b = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    cfg = Mod.GraphGPTConfig(hidden_act="gelu", vocab_size=756, hidden_size=spec.hidden_size, intermediate_size=spec.intermediate_size,
                             num_hidden_layers=spec.num_layers, num_attention_heads=spec.num_heads,
                             max_position_embeddings=spec.max_position, causal_attention=False, stacked_feat=13, next_n_token=1,
                             num_labels=ncls, loss_type=loss_type, problem_type="single_label_classification")
    model = Mod.GraphGPTTaskModel(cfg, seed=1)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return model, b, ncls


@pytest.mark.parametrize("layout", ["padded", "varlen"])
@pytest.mark.parametrize("loss_type", ["token_ce", "token_ce_intra"])
def test_ft_evaluate_graph_clustering(loss_type, layout, monkeypatch):
    model, b, ncls = _token_case(loss_type)
    model.token_layout = layout
    model = model.cuda()
    Bn, S = b["task_labels"].shape
    rng = np.random.RandomState(8)
    real = b["attention_mask"].bool().numpy()
    raw = np.where(real & (rng.rand(Bn, S) < 0.8), np.arange(S)[None] + 50, -100).astype(np.int64)       # padding and repeats: -100
    raw[:, 0] = 50                                                                                       # (the first token is real)
    assert real[:, 0].all()
    keys = [k for k in ("input_ids", "attention_mask", "position_ids", "task_labels", "cls_idx") if k in b]
    loader, plain = [], []
    rows = [0, 1, 2, 4, 5, 6, 7, 8, 9]                            # (sample 3 of the intra fixture has no labelled row: the NaN case is op level)
    assert ((raw[rows] != -100) & (b["task_labels"].numpy()[rows] != -100)).any(1).all()
    for a in range(0, 9, 3):                                       # three batches of three samples
        d = {k: b[k][rows[a:a + 3]].contiguous() for k in keys}
        d["idx"] = torch.tensor(rows[a:a + 3]) + 100
        plain.append(dict(d, idx=d["idx"][:, None].expand(3, S).contiguous()))
        loader.append(dict(d, raw_node_idx=torch.from_numpy(raw[rows[a:a + 3]])))
    seen = []
    real_update = met.GraphClusteringMetrics.update
    monkeypatch.setattr(met.GraphClusteringMetrics, "update",
                        lambda self, lg, y, idx: (seen.append((lg.detach().float().cpu(), y.cpu(), idx[0].cpu(), idx[1].cpu())), real_update(self, lg, y, idx))[1])
    loss, m, res, d = tr.ft_evaluate(model, loader, problem_type="single_label_classification", num_labels=ncls, metric_type="graph_clustering")
    assert model.training and isinstance(m, met.GraphClusteringMetrics) and m.totals.device.type == "cuda" and np.isfinite(float(loss))
    assert len(seen) == 3 and all(tuple(s[0].shape) == (3, S, ncls) for s in seen)
    # the host path on the same task_logits
    host = met.GraphClusteringMetrics(num_labels=ncls)
    for lg, y, idx, rw in seen:
        real_update(host, lg, y, (idx, rw))
    host.compute()
    assert m.results_in_tuple() == host.results_in_tuple() and res == host.results_in_dict() == m.results_in_dict()
    assert list(res) == [" ACC", " Recall", " Precision", "EMA F1"] and m.n_empty == 0 and 0.0 <= m.acc <= 1.0
    hd = host.to_dict()
    n_sel = int((raw[rows] != -100).sum())
    assert list(d) == ["y_true", "y_pred", "idx", "node_idx"]
    assert all(v.device.type == "cpu" and len(v) == n_sel and torch.equal(v, hd[k]) for k, v in d.items())
    assert d["idx"].tolist() == np.repeat(np.array(rows) + 100, S).reshape(9, S)[raw[rows] != -100].tolist()
    # the loss does not depend on the metric object
    loss_plain, m_plain, _, _ = tr.ft_evaluate(model, plain, problem_type="single_label_classification", num_labels=ncls)
    assert isinstance(m_plain, met.SingleLabelClassificationMetrics) and torch.equal(loss_plain, loss)
    model.check_deferred()
