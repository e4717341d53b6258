"""Graph-clustering metrics of the token-level heads on the host (graph-gpt_amd/metrics.py `_cluster_numpy`, `cluster_metrics`,
`GraphClusteringMetrics`): the NumPy count form against the independent set statement of tests/_cluster_ref.py, the arg-max rule, and
the metric object against what the reference's GraphClusteringMetrics returned for tests/golden/cluster_metrics.npz
(tools/make_golden.py `cluster_metrics_fixture`)."""
import importlib
import os

import numpy as np
import pytest
import torch

import _cluster_ref as R
from _util import GOLDEN

met = importlib.import_module("graph-gpt_amd.metrics")

SHAPES = [(1, 1, 2), (3, 8, 3), (4, 17, 8), (2, 40, 65)]


def check_counts(p, y, raw, C, what):
    y_pred, counts, totals = met._cluster_numpy(p, y, raw, C)
    want_pred, want_counts, want_totals = R.cluster_sets(p, y, raw, C)
    assert y_pred.dtype == np.int64 and counts.dtype == np.int32 and totals.dtype == np.int64
    assert y_pred.tolist() == want_pred, what
    assert counts.tolist() == want_counts, (what, counts.tolist(), want_counts)
    assert totals.tolist() == want_totals, (what, totals.tolist(), want_totals)
    return counts, totals


@pytest.mark.parametrize("shape", SHAPES)
def test_count_form_equals_set_statement(shape):
    B, S, C = shape
    rng = np.random.RandomState(B * 1000 + S * 10 + C)
    for lab_kind in R.LABEL_KINDS:
        y, raw = R.make_labels(B, S, C, lab_kind, rng)
        for kind in ("random", "ties"):
            counts, totals = check_counts(R.make_logits(B, S, C, kind, rng), y, raw, C, f"{shape} {lab_kind} {kind}")
        # integer predictions as input, some of them outside [0, C) (bad at a selected position)
        pred = rng.randint(0, C, (B, S)).astype(np.int64)
        check_counts(pred, y, raw, C, f"{shape} {lab_kind} given predictions")
        pred[rng.rand(B, S) < 0.2] = C + 3
        pred[0, 0] = -1
        check_counts(pred, y, raw, C, f"{shape} {lab_kind} given predictions, some out of range")
        if lab_kind == "bad":
            assert totals[3] == (2 if B * S > 1 else 1)
        if lab_kind == "none_selected":
            assert not counts.any() and not totals.any()
        if lab_kind == "one_kept":
            assert (counts == 1).all() and totals[1] == B
        if lab_kind == "first_empty":
            assert not counts[0].any()


def test_closed_form_cases():
    C = 4
    raw = np.arange(6)[None]
    # all labels equal, predictions split: recall 0 / 1, precision 2 / 2
    _, counts, totals = met._cluster_numpy(np.array([[0, 0, 1, 1, 0, 1]]), np.array([[2, 2, 2, 2, 2, 2]]), raw, C)
    assert counts.tolist() == [[0, 1, 2, 2]] and totals.tolist() == [0, 6, 6, 0]
    # all distinct labels, one prediction: recall 4 / 4, precision 0 / 1
    _, counts, totals = met._cluster_numpy(np.array([[1, 1, 1, 1, 1, 1]]), np.array([[0, 1, 2, 3, -100, -100]]), raw, C)
    assert counts.tolist() == [[4, 4, 0, 1]] and totals.tolist() == [1, 4, 6, 0]
    # a label of C and a label of -1 are bad, whatever the prediction; an unselected one is not looked at
    raw2 = np.array([[0, 1, 2, -100, 4, 5]])
    _, counts, totals = met._cluster_numpy(np.array([[1, 1, 2, 2, 3, 3]]), np.array([[C, -1, 2, C, 3, -100]]), raw2, C)
    assert counts.tolist() == [[2, 2, 2, 2]] and totals.tolist() == [2, 2, 3, 2]


def test_argmax_rule():
    nan, inf = np.nan, np.inf
    rows = np.array([[1.0, 3.0, 3.0, 2.0],          # tie: the first maximum
                     [-0.0, 0.0, -1.0, 0.0],        # -0.0 ties +0.0
                     [0.0, -0.0, -1.0, -0.0],
                     [5.0, nan, 9.0, nan],          # a NaN is maximal, the first NaN wins
                     [nan, inf, nan, 0.0],
                     [-inf, -inf, -inf, -inf],      # all -inf: index 0
                     [-inf, -inf, -7.0, -inf],
                     [inf, inf, -inf, nan]], np.float32)
    want = [1, 0, 0, 1, 0, 0, 2, 3]
    assert met._argmax_first(rows).tolist() == want == [R.argmax_first(r.tolist()) for r in rows]
    assert torch.argmax(torch.from_numpy(rows), dim=-1).tolist() == want
    rng = np.random.RandomState(0)
    for kind in R.LOGIT_KINDS:
        lg = R.make_logits(3, 9, 6, kind, rng)
        assert np.array_equal(met._argmax_first(lg), torch.argmax(torch.from_numpy(lg), dim=-1).numpy()), kind
        y_pred = met._cluster_numpy(lg, np.zeros((3, 9), np.int64), np.zeros((3, 9), np.int64), 6)[0]
        assert y_pred.tolist() == R.cluster_sets(lg, np.zeros((3, 9), np.int64), np.zeros((3, 9), np.int64), 6)[0], kind


def _fixture():
    z = np.load(os.path.join(GOLDEN, "cluster_metrics.npz"))
    batches = [(z[f"logits_{k}"], z[f"labels_{k}"], z[f"idx_{k}"], z[f"raw_node_idx_{k}"]) for k in range(3)]
    return z, batches


def _feed(m, batches):
    for lg, y, idx, raw in batches:
        m.update(torch.from_numpy(lg), torch.from_numpy(y), (torch.from_numpy(idx), torch.from_numpy(raw)))
    return m


def test_metric_object_against_reference_fixture():
    """Per-sample fp32 quotients bit-equal; recall / precision within N 2^-23 (the reference's sequential fp32 sum of N values in [0, 1]
    against the fp64 mean here); acc within 2^-23 (the reference's fp32 division of two exact counts); the to_dict arrays equal."""
    z, batches = _fixture()
    m = _feed(met.get_metrics("graph_clustering", num_labels=5), batches)
    assert isinstance(m, met.GraphClusteringMetrics)
    m.compute()
    N = len(z["ls_recall"])
    assert N == 24 and m.n_empty == 0
    assert m.ls_recall.dtype == np.float32 and m.ls_recall.tobytes() == z["ls_recall"].tobytes()
    assert m.ls_precision.dtype == np.float32 and m.ls_precision.tobytes() == z["ls_precision"].tobytes()
    print(f"recall |dev| {abs(m.recall - float(z['recall'])):.3e}, precision |dev| {abs(m.precision - float(z['precision'])):.3e} "
          f"(bound {N * 2.0 ** -23:.3e}); acc |dev| {abs(m.acc - float(z['acc'])):.3e} (bound {2.0 ** -23:.3e})")
    assert abs(m.recall - float(z["recall"])) <= N * 2.0 ** -23
    assert abs(m.precision - float(z["precision"])) <= N * 2.0 ** -23
    assert abs(m.acc - float(z["acc"])) <= 2.0 ** -23
    d = m.to_dict()
    assert list(d) == ["y_true", "y_pred", "idx", "node_idx"]
    for k in d:
        assert d[k].dtype == torch.int64 and np.array_equal(d[k].numpy(), z[k]), k
    res = m.results_in_dict(prefix="valid")
    assert list(res) == z["results_keys"].tolist() == ["valid ACC", "valid Recall", "valid Precision", "EMA F1"]
    assert res["EMA F1"] == 2 * m.recall * m.precision / (m.recall + m.precision)
    assert np.abs(np.array(list(res.values())) - z["results_values"]).max() <= N * 2.0 ** -23
    assert m.results_in_tuple() == (m.acc, m.recall, m.precision) and m.results_in_str_tuple() == (str(m.acc), str(m.recall), str(m.precision))
    assert m.results_in_details("v") == f"v Recall: {m.recall}, v Precision: {m.precision}, v ACC: {m.acc}"
    assert m.get_output_shape(7, "idx") == 7
    # integer predictions in place of logits give the same object
    m2 = met.get_metrics("graph_clustering", num_labels=5)
    for lg, y, idx, raw in batches:
        m2.update(torch.from_numpy(lg).argmax(-1), torch.from_numpy(y), (torch.from_numpy(idx), torch.from_numpy(raw)))
    m2.compute()
    assert m2.results_in_tuple() == m.results_in_tuple()


def test_compute_on_gathered_halves_equals_compute_on_the_whole():
    z, batches = _fixture()
    whole = _feed(met.GraphClusteringMetrics(num_labels=5), batches)
    whole.compute()
    a, b = _feed(met.GraphClusteringMetrics(num_labels=5), batches[:1]), _feed(met.GraphClusteringMetrics(num_labels=5), batches[1:])
    sa, sb = a.sync_dict(), b.sync_dict()
    assert sorted(sa) == ["counts", "totals"] and tuple(sa["counts"].shape) == (8, 4) and tuple(sb["totals"].shape) == (4,)
    a.compute({k: torch.cat([sa[k], sb[k]]) for k in sa})
    assert a.results_in_tuple() == whole.results_in_tuple() and a.n_empty == whole.n_empty
    b.compute({k: np.concatenate([sb[k].numpy(), sa[k].numpy()]) for k in sa})          # arrays, the other order
    assert b.acc == whole.acc and abs(b.recall - whole.recall) <= 24 * 2.0 ** -52 and abs(b.precision - whole.precision) <= 24 * 2.0 ** -52


def test_empty_single_and_bad_samples():
    m = met.GraphClusteringMetrics(num_labels=3)
    lg = torch.tensor([[[0.0, 1.0, 0.0], [2.0, 1.0, 0.0]], [[0.0, 1.0, 0.0], [0.0, 0.0, 3.0]]])
    # sample 0: one selected position, kept -> 1 / 1; sample 1: one selected position, not labelled -> NaN (the means are NaN with it)
    m.update(lg, torch.tensor([[1, 0], [-100, 2]]), (torch.tensor([4, 9]), torch.tensor([[7, -100], [3, -100]])))
    m.compute()
    assert m.ls_recall[0] == 1.0 and m.ls_precision[0] == 1.0 and np.isnan(m.ls_recall[1]) and np.isnan(m.ls_precision[1])
    assert np.isnan(m.recall) and np.isnan(m.precision) and m.acc == 1.0 and m.n_empty == 1
    d = m.to_dict()
    assert d["idx"].tolist() == [4, 9] and d["node_idx"].tolist() == [7, 3] and d["y_true"].tolist() == [1, -100] and d["y_pred"].tolist() == [1, 1]
    with pytest.raises(AssertionError, match="tuple"):
        m.update(lg, torch.tensor([[1, 0], [-100, 2]]), torch.tensor([4, 9]))
    bad = met.GraphClusteringMetrics(num_labels=3)
    bad.update(lg, torch.tensor([[3, 0], [-1, 2]]), (torch.tensor([0, 1]), torch.tensor([[0, 1], [0, -100]])))
    with pytest.raises(ValueError, match="2 selected positions"):
        bad.compute()
    with pytest.raises(ValueError, match="num_labels"):
        met.cluster_metrics(lg, torch.zeros(2, 2, dtype=torch.long), torch.zeros(2, 2, dtype=torch.long), 4)


def test_registry():
    assert isinstance(met.get_metrics("graph_clustering", "cpu", num_labels=7), met.GraphClusteringMetrics)
    for name in ("sequence_classification", "clustering", ""):
        with pytest.raises(NotImplementedError, match="sequence metrics are outside"):
            met.get_metrics(name)
