"""Fine-tune metrics computed from `task_logits`: build-side counterparts of
  SingleLabelClassificationMetrics.update   reference src/utils/metrics_utils.py:38-56   (score = logit1 - logit0 -> AUROC / ACC)
  _eval_ogbl_ppa (OGB Hits@K)               reference src/utils/ogb_utils.py:83-90       (K = 100)
  _eval_ogbl_citation2 (OGB MRR)            reference src/utils/ogb_utils.py:93
  RegressionMetrics / _eval_pcqm4mv2 (MAE)  reference src/utils/metrics_utils.py:143-189, src/utils/ogb_utils.py:199-204
  MultiLabelClassificationMetrics           reference src/utils/metrics_utils.py:91-140     (per-task ROC-AUC of sigmoid(logits))
  _eval_rocauc / OGB _eval_ap               reference src/utils/ogb_utils.py:13-29, :71-79, :173-195 (ogbn-proteins, ogbg-molhiv, ogbg-molpcba)
The reference delegates to `torchmetrics` / `ogb` (not installed here); these are plain NumPy statements of the
published definitions, pinned in tests against scikit-learn and closed-form cases."""
from __future__ import annotations

import numpy as np


def edge_score(task_logits: np.ndarray) -> np.ndarray:
    """y = logit[:,1] - logit[:,0] in fp32 (metrics_utils.py:45-48; also `auc_loss` input, modeling_finetune.py:203-206)."""
    lg = np.asarray(task_logits, np.float32)
    return lg[:, 1] - lg[:, 0]


def accuracy(task_logits: np.ndarray, labels: np.ndarray) -> float:
    return float((np.asarray(task_logits).argmax(-1) == np.asarray(labels)).mean())


def auroc(scores: np.ndarray, labels: np.ndarray) -> float:
    """Area under the ROC curve = Mann-Whitney U statistic with mid-ranks for ties."""
    s = np.asarray(scores, np.float64)
    y = np.asarray(labels).astype(bool)
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    order = np.argsort(s, kind="mergesort")
    ranks = np.empty(len(s), np.float64)
    ss = s[order]
    i = 0
    while i < len(ss):
        j = i
        while j + 1 < len(ss) and ss[j + 1] == ss[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return float((ranks[y].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def hits_at_k(pos_scores: np.ndarray, neg_scores: np.ndarray, k: int = 100) -> float:
    """OGB link-prediction Hits@K (ogb.linkproppred.Evaluator._eval_hits): fraction of positive edges scored above
    the K-th best negative edge; 1.0 when there are fewer than K negatives."""
    pos, neg = np.asarray(pos_scores, np.float64), np.asarray(neg_scores, np.float64)
    if len(neg) < k:
        return 1.0
    kth = np.sort(neg)[-k]
    return float((pos > kth).mean())


def mrr(pos_scores: np.ndarray, neg_scores: np.ndarray) -> float:
    """OGB MRR (ogb.linkproppred.Evaluator._eval_mrr): pos [N], neg [N, n_neg]; mean of 1/rank of the positive among its
    own negatives with OGB's tie handling (average of the optimistic and pessimistic rank)."""
    pos = np.asarray(pos_scores, np.float64)[:, None]
    neg = np.asarray(neg_scores, np.float64)
    optimistic = (neg > pos).sum(1)
    pessimistic = (neg >= pos).sum(1)
    rank = 0.5 * (optimistic + pessimistic) + 1.0
    return float((1.0 / rank).mean())


def mae(pred: np.ndarray, target: np.ndarray) -> float:
    return float(np.abs(np.asarray(pred, np.float64).reshape(-1) - np.asarray(target, np.float64).reshape(-1)).mean())


# ----------------------------------------------------------------------------- rank metrics of [n, C] score / label matrices (multi-label)
RANK_DATASETS = {"ogbg-molpcba": "ap", "ogbn-proteins": "rocauc", "ogbg-molhiv": "rocauc"}


def _is_cuda(x) -> bool:
    return getattr(getattr(x, "device", None), "type", None) == "cuda"


def _rank_counts_numpy(scores, labels):
    """The count form of include/gget.h `gget_op_rank_metrics` in NumPy (the host path, and what the GPU tests compare the kernel with):
    per column, over its labelled entries, a_i / e_i = negatives scored below / equal to the positive i, g_i = positives scored >= it, from
    binary searches in the sorted lists (no loop over samples).  Returns (n_pos, n_neg, auc2, ap_sum, n_bad) per column."""
    s, y = np.asarray(scores, np.float64), np.asarray(labels, np.float64)
    C = s.shape[1]
    n_pos, n_neg, auc2 = np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros(C, np.uint64)
    ap_sum, n_bad = np.zeros(C, np.float64), np.zeros(C, np.int32)
    lab = ~np.isnan(y)
    ok = lab & np.isfinite(s) & ((y == 0) | (y == 1))
    n_bad[:] = (lab & ~ok).sum(0)
    for c in range(C):
        pos, neg = s[ok[:, c] & (y[:, c] == 1), c], np.sort(s[ok[:, c] & (y[:, c] == 0), c])
        n_pos[c], n_neg[c] = len(pos), len(neg)
        if len(pos) == 0 or len(neg) == 0:
            continue
        a = np.searchsorted(neg, pos, side="left")
        a_e = np.searchsorted(neg, pos, side="right")                          # a + e
        g = len(pos) - np.searchsorted(np.sort(pos), pos, side="left")
        auc2[c] = int((a + a_e).sum())
        ap_sum[c] = (g / (g + (len(neg) - a)).astype(np.float64)).sum()
    return n_pos, n_neg, auc2, ap_sum, n_bad


def _rank_counts_hip(scores, labels):
    """The same five vectors from the HIP kernels (csrc/metrics.hip) for CUDA tensors: five launches on the current stream, then one
    synchronisation (the first copy) and five small copies.  No fallback: a library without the entry is an error."""
    import ctypes as C
    import torch
    from . import _lib
    lib = _lib.load()
    s, y = scores.detach().float(), labels.detach().to(scores.device).float()
    n, ncol = s.shape
    rows_ok = lambda t: t.stride(1) == 1 and t.stride(0) >= ncol      # noqa: E731  (a row-strided view, e.g. x[:, :C], is read in place)
    s, y = (s if rows_ok(s) else s.contiguous()), (y if rows_ok(y) else y.contiguous())
    dev = s.device
    out = [torch.zeros(ncol, dtype=dt, device=dev) for dt in (torch.int64, torch.int64, torch.int64, torch.float64, torch.int32)]
    if n and ncol:
        with torch.cuda.device(dev):
            nbytes = int(lib.gget_op_rank_metrics_workspace(n, ncol))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.gget_op_rank_metrics(s.data_ptr(), s.stride(0), y.data_ptr(), y.stride(0), n, ncol, *[o.data_ptr() for o in out],
                                                ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    n_pos, n_neg, auc2, ap_sum, n_bad = [o.cpu().numpy() for o in out]
    return n_pos, n_neg, auc2.view(np.uint64), ap_sum, n_bad


def rank_metrics(scores, labels):
    """Per-column ROC-AUC and average precision of scores [n, C] against labels [n, C] (1 positive, 0 negative, NaN unlabelled), over each
    column's labelled entries: scikit-learn's `roc_auc_score` / `average_precision_score` column by column (what the reference's evaluators
    loop over, src/utils/ogb_utils.py:13-29), as exact pair counts (include/gget.h `gget_op_rank_metrics`).  CUDA tensors go through the HIP
    kernels (scores are compared in fp32); anything else through the NumPy statement of the same counts (scores compared in fp64).
    Returns {"n_pos", "n_neg", "auroc", "ap", "n_bad"}, NumPy vectors [C]; auroc / ap are NaN for a column without both classes.
    Raises ValueError when a labelled entry has a label other than 0 / 1 or a score that is not finite (scikit-learn raises on these too)."""
    if _is_cuda(scores):
        if scores.dim() != 2 or tuple(labels.shape) != tuple(scores.shape):
            raise ValueError(f"rank_metrics: scores {tuple(scores.shape)} and labels {tuple(labels.shape)} must be equal 2-D shapes")
        n_pos, n_neg, auc2, ap_sum, n_bad = _rank_counts_hip(scores, labels)
    else:
        to_np = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)     # noqa: E731
        s, y = to_np(scores), to_np(labels)
        if s.ndim != 2 or s.shape != y.shape:
            raise ValueError(f"rank_metrics: scores {s.shape} and labels {y.shape} must be equal 2-D shapes")
        n_pos, n_neg, auc2, ap_sum, n_bad = _rank_counts_numpy(s, y)
    if n_bad.any():
        c = int(np.flatnonzero(n_bad)[0])
        raise ValueError(f"rank_metrics: {int(n_bad.sum())} labelled entries with a label other than 0 / 1 or a non-finite score "
                         f"(first in column {c}: {int(n_bad[c])})")
    valid = (n_pos > 0) & (n_neg > 0)
    pairs = np.where(valid, 2.0 * n_pos.astype(np.float64) * n_neg.astype(np.float64), 1.0)
    auroc_vec = np.where(valid, auc2.astype(np.float64) / pairs, np.nan)
    ap_vec = np.where(valid, ap_sum / np.maximum(n_pos, 1), np.nan)
    return {"n_pos": n_pos, "n_neg": n_neg, "auroc": auroc_vec, "ap": ap_vec, "n_bad": n_bad}


# ----------------------------------------------------------------------------- accumulating metric objects of the fine-tune evaluation pass
class SingleLabelClassificationMetrics:
    """Counterpart of the reference class of the same name (src/utils/metrics_utils.py:17-80): per batch `update(logits,
    labels, idx)`; two classes: probability of class 1 feeds AUROC / accuracy, the edge score logit1 - logit0 (fp32) is what
    is kept for the OGB evaluators; more classes: arg-max accuracy.  torchmetrics is replaced by the NumPy statements above."""

    def __init__(self, device=None, num_labels: int = 2, **kwargs):
        self.device, self.num_labels = device, num_labels
        self.auroc = self.acc = None
        self.ls_prob, self.ls_pred, self.ls_labels, self.ls_idx = [], [], [], []

    def update(self, logits, labels, idx):
        import torch
        lg = logits.detach().float()
        if self.num_labels == 2:
            self.ls_prob.append(lg.softmax(dim=-1)[:, 1].cpu())
            y_pred = lg[:, 1] - lg[:, 0]
        else:
            y_pred = torch.argmax(lg, dim=-1)
            labels, idx = labels.reshape(y_pred.shape), idx.reshape(y_pred.shape)
        self.ls_pred.append(y_pred.cpu())
        self.ls_labels.append(labels.detach().cpu())
        self.ls_idx.append(idx.detach().cpu())

    def compute(self, gathered=None):
        """`gathered`: {"y_true", "prob" | "y_pred"} collected from ALL ranks (the reference's torchmetrics objects synchronise
        across ranks inside compute(); here the caller passes what it gathered).  None = this rank's own lists."""
        import torch
        y = torch.hstack(self.ls_labels).numpy() if gathered is None else np.asarray(gathered["y_true"])
        if self.num_labels == 2:
            prob = torch.hstack(self.ls_prob).numpy() if gathered is None else np.asarray(gathered["prob"])
            self.auroc = auroc(prob, y)
            self.acc = float(((prob > 0.5).astype(np.int64) == y).mean())
        else:
            self.auroc = -1
            pred = torch.hstack(self.ls_pred).numpy() if gathered is None else np.asarray(gathered["y_pred"])
            self.acc = float((pred == y).mean())

    def sync_dict(self):
        """what compute() needs from every rank (superset of to_dict for the two-class case: the class-1 probabilities)"""
        import torch
        d = {"y_true": torch.hstack(self.ls_labels), "y_pred": torch.hstack(self.ls_pred)}
        if self.num_labels == 2:
            d["prob"] = torch.hstack(self.ls_prob)
        return d

    def to_dict(self):
        import torch
        return {"y_true": torch.hstack(self.ls_labels), "y_pred": torch.hstack(self.ls_pred), "idx": torch.hstack(self.ls_idx)}

    def results_in_tuple(self):
        return self.auroc, self.acc

    def results_in_dict(self):
        return {"auroc": self.auroc, "acc": self.acc}


class RegressionMetrics:
    """Counterpart of the reference RegressionMetrics (src/utils/metrics_utils.py:143-189): mean absolute / squared error."""

    def __init__(self, device=None, num_labels: int = 1, **kwargs):
        self.device = device
        self.mae = self.mse = None
        self.ls_pred, self.ls_labels, self.ls_idx = [], [], []

    def update(self, logits, labels, idx):
        self.ls_pred.append(logits.detach().float().reshape(-1).cpu())
        self.ls_labels.append(labels.detach().float().reshape(-1).cpu())
        self.ls_idx.append(idx.detach().reshape(-1).cpu())

    def compute(self, gathered=None):
        import torch
        if gathered is None:
            p, y = torch.hstack(self.ls_pred).numpy(), torch.hstack(self.ls_labels).numpy()
        else:
            p, y = np.asarray(gathered["y_pred"]), np.asarray(gathered["y_true"])
        self.mae = mae(p, y)
        self.mse = float(((p.astype(np.float64) - y) ** 2).mean())

    def to_dict(self):
        import torch
        return {"y_true": torch.hstack(self.ls_labels), "y_pred": torch.hstack(self.ls_pred), "idx": torch.hstack(self.ls_idx)}

    def sync_dict(self):
        import torch
        return {"y_true": torch.hstack(self.ls_labels), "y_pred": torch.hstack(self.ls_pred)}

    def results_in_tuple(self):
        return self.mse, self.mae       # the reference's order (metrics_utils.py:184-185)

    def results_in_dict(self):
        return {"mae": self.mae, "mse": self.mse}


class MultiLabelClassificationMetrics:
    """Counterpart of the reference class of the same name (src/utils/metrics_utils.py:91-140): per batch `update(logits, labels, idx)`
    keeps `logits.float()`, the labels and the indices ON THE DEVICE THEY ARRIVE ON (no host copy, no synchronisation per batch);
    `compute()` takes the per-task ROC-AUC of sigmoid(logits) in fp32 - the torch sigmoid, applied once - over each task's labelled
    (non-NaN) entries with `rank_metrics`, on the device for CUDA tensors.  torcheval's BinaryAUROC(num_tasks) is replaced by the count
    form pinned against scikit-learn.  A task without both classes gets 0.5: torcheval's rule for a constant target; torcheval is not
    installed where this package is tested, so this one rule is a stated convention, not pinned against it."""

    def __init__(self, device=None, num_labels: int = 2, **kwargs):
        self.device, self.num_labels = device, num_labels
        self.auroc_vec = self.auroc_mean = None
        self.ls_logits, self.ls_labels, self.ls_idx = [], [], []

    def update(self, logits, labels, idx):
        self.ls_logits.append(logits.detach().float())       # [batch, num_labels]
        self.ls_labels.append(labels.detach())               # [batch, num_labels]
        self.ls_idx.append(idx.detach().reshape(-1))         # [batch]

    def compute(self, gathered=None):
        """`gathered`: {"y_true", "y_pred"} collected from ALL ranks (tensors or arrays); None = this rank's own lists."""
        import torch
        d = self.sync_dict() if gathered is None else gathered
        logits, y = torch.as_tensor(d["y_pred"]).float(), torch.as_tensor(d["y_true"])
        r = rank_metrics(torch.sigmoid(logits), y.to(logits.device).float())
        self.auroc_vec = np.where((r["n_pos"] > 0) & (r["n_neg"] > 0), r["auroc"], 0.5)
        self.auroc_mean = float(self.auroc_vec.mean())

    def sync_dict(self):
        import torch
        return {"y_true": torch.vstack(self.ls_labels), "y_pred": torch.vstack(self.ls_logits)}

    def to_dict(self):
        """y_true [N, C], y_pred [N, C] (the raw logits: what the OGB evaluators rank), idx [N] - on the device the batches arrived on"""
        import torch
        return dict(self.sync_dict(), idx=torch.cat(self.ls_idx))

    def get_output_shape(self, dim, key=None):
        return dim if key == "idx" else (dim, self.num_labels)

    def results_in_tuple(self):
        return [self.auroc_mean]

    def results_in_dict(self, prefix=""):
        return {"auroc_mean": self.auroc_mean}

    def results_in_details(self, prefix=""):
        return f"{prefix} mean AUROC: {self.auroc_mean}"

    def results_in_full_details(self, prefix=""):
        return f"{prefix} mean AUROC: {self.auroc_mean}, detailed AUROC: {','.join(self.auroc_vec.astype(str))}"


def get_metrics(metric_type: str, device=None, num_labels: int = 2):
    """reference `get_metrics` registry (metrics_utils.py:11-13): the two problem types of the BASELINE configs and the multi-label one."""
    if metric_type == "single_label_classification":
        return SingleLabelClassificationMetrics(device, num_labels=num_labels)
    if metric_type == "regression":
        return RegressionMetrics(device, num_labels=num_labels)
    if metric_type == "multi_label_classification":
        return MultiLabelClassificationMetrics(device, num_labels=num_labels)
    raise NotImplementedError(f"metric_type={metric_type!r} (sequence metrics are outside the hot-path scope)")


def evaluate_ogb(dataset_name: str, input_dict):
    """reference `evaluate_ogb` for the datasets of the BASELINE configs (src/utils/ogb_utils.py:83-90 ogbl-ppa Hits@100 over
    positive / negative edges split by label; :199-204 PCQM4Mv2 MAE) and the multi-label ones (:187-195 ogbg-molpcba mean AP, :71-79
    ogbn-proteins / :173-184 ogbg-molhiv mean ROC-AUC over the columns that hold both classes - `_eval_rocauc` :13-29; the rank metrics
    are taken on the raw logits as the reference feeds them; tensors or arrays, CUDA tensors through the HIP kernels).  None for a
    dataset this package has no evaluator for."""
    if dataset_name in RANK_DATASETS:
        return _evaluate_rank(dataset_name, input_dict["y_true"], input_dict["y_pred"])
    y_true, y_pred = np.asarray(input_dict["y_true"]), np.asarray(input_dict["y_pred"], np.float64)
    if dataset_name == "ogbl-ppa":
        return {"hits@100": hits_at_k(y_pred[y_true == 1], y_pred[y_true == 0], 100)}
    if dataset_name == "PCQM4Mv2":
        return {"mae": mae(y_pred, y_true)}
    return None


def _evaluate_rank(dataset_name: str, y_true, y_pred):
    key = RANK_DATASETS[dataset_name]
    if not hasattr(y_pred, "detach"):
        y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    if dataset_name == "ogbg-molhiv" and y_pred.ndim != 2:        # (one task: ogb_utils.py:180-182)
        y_true, y_pred = y_true.reshape(-1, 1), y_pred.reshape(-1, 1)
    r = rank_metrics(y_pred, y_true)
    vals = r["auroc" if key == "rocauc" else "ap"][(r["n_pos"] > 0) & (r["n_neg"] > 0)]
    if len(vals) == 0:                                            # ogb_utils.py:24-27
        raise RuntimeError(f"No positively labeled data available. Cannot compute {'ROC-AUC' if key == 'rocauc' else 'Average Precision'}.")
    return {key: float(vals.sum() / len(vals))}
