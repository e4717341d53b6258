"""Fine-tune metrics computed from `task_logits`: build-side counterparts of
  SingleLabelClassificationMetrics.update   reference src/utils/metrics_utils.py:38-56   (score = logit1 - logit0 -> AUROC / ACC)
  _eval_ogbl_ppa / _eval_ogbl_ddi (Hits@K)  reference src/utils/ogb_utils.py:82-90, :131-138, :141-152  (K = 100 / 20; `link_hits`)
  _eval_ogbl_citation2 / _eval_ogbl_wikikg2 reference src/utils/ogb_utils.py:92-128, :155-170              (OGB MRR, Hits@1/3/10; `link_mrr`)
  RegressionMetrics / _eval_pcqm4mv2 (MAE)  reference src/utils/metrics_utils.py:143-189, src/utils/ogb_utils.py:199-204
  MultiLabelClassificationMetrics           reference src/utils/metrics_utils.py:91-140     (per-task ROC-AUC of sigmoid(logits))
  _eval_rocauc / OGB _eval_ap               reference src/utils/ogb_utils.py:13-29, :71-79, :173-195 (ogbn-proteins, ogbg-molhiv, ogbg-molpcba)
The reference delegates to `torchmetrics` / `ogb` (not installed here); these are plain NumPy statements of the
published definitions, pinned in tests against scikit-learn and closed-form cases.  CUDA tensors take the HIP kernels of
csrc/metrics.hip (`rank_metrics`, `link_hits`, `link_mrr`); host arrays take the NumPy statements."""
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


# ----------------------------------------------------------------------------- link prediction: Hits@K and MRR of flat score / label lists
def _to_np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _link_bad(s, y):
    return ~(np.isfinite(s) & ((y == 0) | (y == 1)))


def _link_hits_numpy(scores, labels, k):
    """The counts of include/gget.h `gget_op_link_hits` in NumPy (the host path, and what the GPU tests compare the kernels with):
    (n_pos, n_neg, kth, hits, n_bad); kth in the scores' own floating-point type, a zero as +0.0, -inf when n_neg < k."""
    s, y = np.asarray(scores), np.asarray(labels)
    s = s if s.dtype.kind == "f" else s.astype(np.float64)
    bad = _link_bad(s, y)
    pos, neg = s[~bad & (y == 1)], s[~bad & (y == 0)]
    if len(neg) < k:
        return len(pos), len(neg), s.dtype.type(-np.inf), len(pos), int(bad.sum())
    kth = np.partition(neg, len(neg) - k)[len(neg) - k] + s.dtype.type(0.0)          # (-0.0 + 0.0 = +0.0)
    return len(pos), len(neg), kth, int((pos > kth).sum()), int(bad.sum())


def _link_hits_hip(scores, labels, k):
    """The same five values from the HIP kernels for CUDA tensors: ten launches on the current stream, then one synchronisation (the
    first copy) and five scalar copies.  No fallback: a library without the entry is an error."""
    import ctypes as C
    import torch
    from . import _lib
    lib = _lib.load()
    s = scores.detach().float().contiguous()
    y = labels.detach().to(s.device).long().contiguous()
    n, dev = s.numel(), s.device
    out = [torch.zeros(1, dtype=dt, device=dev) for dt in (torch.int64, torch.int64, torch.float32, torch.int64, torch.int32)]
    if n:
        with torch.cuda.device(dev):
            nbytes = int(lib.gget_op_link_hits_workspace(n))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.gget_op_link_hits(s.data_ptr(), y.data_ptr(), n, int(k), *[o.data_ptr() for o in out], ws.data_ptr(), nbytes,
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    else:
        out[2].fill_(float("-inf"))
    n_pos, n_neg, kth, hits, n_bad = [o.cpu().numpy()[0] for o in out]
    return int(n_pos), int(n_neg), kth, int(hits), int(n_bad)


def link_hits(scores, labels, k: int):
    """OGB Hits@K of flat edge scores [n] against labels [n] (1 = positive edge, 0 = negative edge): `_reformat_pred_for_hr_eval` + OGB
    `_eval_hits` (src/utils/ogb_utils.py:141-152), as exact counts (include/gget.h `gget_op_link_hits`).  CUDA tensors go through the HIP
    kernels (fp32 scores); anything else through NumPy, where "hits@k" is `hits_at_k` of the two lists.  Returns {"n_pos", "n_neg",
    "kth" (K-th largest negative score, -inf with fewer than K negatives), "hits" (positives above it), "hits@k" (hits / n_pos; 1.0 with
    fewer than K negatives, as OGB)}.  Raises ValueError on a label other than 0 / 1 or a score that is not finite."""
    if k < 1:
        raise ValueError(f"link_hits: k = {k}")
    if _is_cuda(scores):
        if scores.dim() != 1 or tuple(labels.shape) != tuple(scores.shape):
            raise ValueError(f"link_hits: scores {tuple(scores.shape)} and labels {tuple(labels.shape)} must be equal 1-D shapes")
        n_pos, n_neg, kth, hits, n_bad = _link_hits_hip(scores, labels, k)
        ratio = None
    else:
        s, y = _to_np(scores), _to_np(labels)
        if s.ndim != 1 or s.shape != y.shape:
            raise ValueError(f"link_hits: scores {s.shape} and labels {y.shape} must be equal 1-D shapes")
        n_pos, n_neg, kth, hits, n_bad = _link_hits_numpy(s, y, k)
        ratio = None if n_bad else hits_at_k(s[y == 1], s[y == 0], k)
    if n_bad:
        raise ValueError(f"link_hits: {n_bad} entries with a label other than 0 / 1 or a non-finite score")
    if ratio is None:
        ratio = 1.0 if n_neg < k else float(np.float64(hits) / np.float64(n_pos)) if n_pos else float("nan")
    return {"n_pos": n_pos, "n_neg": n_neg, "kth": kth, "hits": hits, "hits@k": ratio}


def _link_mrr_numpy(scores, labels, idx, cnt_neg, groups):
    """The counts of include/gget.h `gget_op_link_mrr` in NumPy: (n_pos, n_neg, optimistic [groups, P], pessimistic [groups, P],
    hits_1_3_10, mrr_sum, n_bad [2]).  With a non-zero n_bad the arrays are empty and the sums 0."""
    s, y, ix = np.asarray(scores), np.asarray(labels), np.asarray(idx).astype(np.int64)
    s = s if s.dtype.kind == "f" else s.astype(np.float64)
    n = len(s)
    P = n // (1 + cnt_neg)
    in_range = (ix >= 0) & (ix < n)
    n_bad = np.zeros(2, np.int32)
    n_bad[0] = int((~in_range).sum()) + int(in_range.sum() - len(np.unique(ix[in_range])))
    ss, ys = np.zeros(n, s.dtype), np.full(n, -1, np.int64)
    ss[ix[in_range]], ys[ix[in_range]] = s[in_range], y[in_range]               # the scatter ("sort by idx"; a repeat leaves a slot empty)
    filled = np.zeros(n, bool)
    filled[ix[in_range]] = True
    bad = filled & _link_bad(ss, ys)
    pos, neg = ss[filled & ~bad & (ys == 1)], ss[filled & ~bad & (ys == 0)]
    n_bad[1] = int(bad.sum()) or (-1 if len(neg) != len(pos) * cnt_neg else 0)
    empty = np.zeros((groups, 0), np.int32)
    if n_bad.any():
        return len(pos), len(neg), empty, empty, np.zeros(3, np.int64), 0.0, n_bad
    n_neg, neg = len(neg), neg.reshape(P, cnt_neg)
    opt = np.stack([(neg[:, g::groups] > pos[:, None]).sum(1) for g in range(groups)]).astype(np.int32)
    pes = np.stack([(neg[:, g::groups] >= pos[:, None]).sum(1) for g in range(groups)]).astype(np.int32)
    rank = 0.5 * (opt + pes).reshape(-1) + 1.0
    return len(pos), n_neg, opt, pes, np.array([(rank <= t).sum() for t in (1, 3, 10)], np.int64), float((1.0 / rank).sum()), n_bad


def _link_mrr_hip(scores, labels, idx, cnt_neg, groups):
    """The same seven values from the HIP kernels for CUDA tensors: seven launches on the current stream, then one synchronisation (the
    first copy).  No fallback: a library without the entry is an error."""
    import ctypes as C
    import torch
    from . import _lib
    lib = _lib.load()
    s = scores.detach().float().contiguous()
    y, ix = labels.detach().to(s.device).long().contiguous(), idx.detach().to(s.device).long().contiguous()
    n, dev = s.numel(), s.device
    P = n // (1 + cnt_neg)
    out = [torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
           torch.zeros(groups, P, dtype=torch.int32, device=dev), torch.zeros(groups, P, dtype=torch.int32, device=dev),
           torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev),
           torch.zeros(2, dtype=torch.int32, device=dev)]
    if n:
        with torch.cuda.device(dev):
            nbytes = int(lib.gget_op_link_mrr_workspace(n))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.gget_op_link_mrr(s.data_ptr(), y.data_ptr(), ix.data_ptr(), n, cnt_neg, groups, *[o.data_ptr() for o in out],
                                            ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    n_pos, n_neg, opt, pes, hits, mrr_sum, n_bad = [o.cpu().numpy() for o in out]
    return int(n_pos[0]), int(n_neg[0]), opt, pes, hits, float(mrr_sum[0]), n_bad


def link_mrr(scores, labels, idx, cnt_neg: int = 1000, groups: int = 1):
    """OGB MRR and Hits@1/3/10 of flat edge scores [n] against labels [n] with the sample order `idx` [n], a permutation of 0 .. n-1:
    `_reformat_pred_for_mrr_eval` (src/utils/ogb_utils.py:155-170: sort by idx; the positives, and the negatives as rows of `cnt_neg`)
    + OGB `_eval_mrr`, as exact counts (include/gget.h `gget_op_link_mrr`).  groups = 2 is ogbl-wikikg2 (:105-128): the even negative
    columns and the odd ones are ranked apart and the two lists concatenated.  CUDA tensors go through the HIP kernels (fp32 scores);
    anything else through NumPy; for groups = 1 "mrr" is then `mrr(pos, neg)`.  Returns {"mrr", "hits@1", "hits@3", "hits@10"} (means over
    the groups * P ranks, fp64 - OGB takes them of its fp32 lists) and {"optimistic", "pessimistic"} (int32 [groups, P]: negatives scored
    > / >= the positive; rank = their mean + 1).  Raises ValueError on an index outside 0 .. n-1 or a repeated one, on a label other than
    0 / 1 or a score that is not finite, and when the negatives are not cnt_neg per positive (the reference asserts those)."""
    if cnt_neg < 1 or groups not in (1, 2) or cnt_neg % groups:
        raise ValueError(f"link_mrr: cnt_neg = {cnt_neg}, groups = {groups} (1, or 2 with an even cnt_neg)")
    cuda = _is_cuda(scores)
    if not cuda:
        scores, labels, idx = _to_np(scores), _to_np(labels), _to_np(idx)
    shape = tuple(scores.shape)
    if len(shape) != 1 or tuple(labels.shape) != shape or tuple(idx.shape) != shape:
        raise ValueError(f"link_mrr: scores {shape}, labels {tuple(labels.shape)} and idx {tuple(idx.shape)} must be equal 1-D shapes")
    if shape[0] % (1 + cnt_neg):
        raise ValueError(f"link_mrr: {shape[0]} entries are not a multiple of 1 + cnt_neg = {1 + cnt_neg}")
    n_pos, n_neg, opt, pes, hits, mrr_sum, n_bad = (_link_mrr_hip if cuda else _link_mrr_numpy)(scores, labels, idx, cnt_neg, groups)
    if n_bad[0]:
        raise ValueError(f"link_mrr: idx is not a permutation of 0 .. {shape[0] - 1}: {int(n_bad[0])} entries out of range or repeated")
    if n_bad[1] > 0:
        raise ValueError(f"link_mrr: {int(n_bad[1])} entries with a label other than 0 / 1 or a non-finite score")
    if n_bad[1]:
        raise ValueError(f"link_mrr: {n_neg} negatives for {n_pos} positives, not {cnt_neg} each")
    m = max(groups * n_pos, 1)
    res = {"mrr": mrr_sum / m, "hits@1": float(hits[0]) / m, "hits@3": float(hits[1]) / m, "hits@10": float(hits[2]) / m}
    if n_pos == 0:
        res = {k: float("nan") for k in res}
    return dict(res, optimistic=opt, pessimistic=pes)


# ----------------------------------------------------------------------------- accumulating metric objects of the fine-tune evaluation pass
class SingleLabelClassificationMetrics:
    """Counterpart of the reference class of the same name (src/utils/metrics_utils.py:17-80): per batch `update(logits,
    labels, idx)`; two classes: probability of class 1 feeds AUROC / accuracy, the edge score logit1 - logit0 (fp32) is what
    is kept for the OGB evaluators; more classes: arg-max accuracy.  torchmetrics is replaced by the NumPy statements above.
    `on_device=True` (two classes, what `ft_evaluate` asks for on a GPU): `update` keeps the four tensors on the device they arrive on,
    as the reference does (:38-57) - no host copy, no synchronisation per batch; `compute` takes the accuracy from an integer count and
    the AUROC from `rank_metrics` on a one-column view (exact pair counts; n_pos * n compare-and-adds), `to_dict` / `sync_dict` return
    device tensors."""

    def __init__(self, device=None, num_labels: int = 2, on_device: bool = False, **kwargs):
        self.device, self.num_labels, self.on_device = device, num_labels, bool(on_device)
        self.auroc = self.acc = None
        self.ls_prob, self.ls_pred, self.ls_labels, self.ls_idx = [], [], [], []

    def update(self, logits, labels, idx):
        import torch
        lg = logits.detach().float()
        keep = (lambda t: t) if self.on_device else (lambda t: t.cpu())
        if self.num_labels == 2:
            self.ls_prob.append(keep(lg.softmax(dim=-1)[:, 1]))
            y_pred = lg[:, 1] - lg[:, 0]
        else:
            y_pred = torch.argmax(lg, dim=-1)
            labels, idx = labels.reshape(y_pred.shape), idx.reshape(y_pred.shape)
        self.ls_pred.append(keep(y_pred))
        self.ls_labels.append(keep(labels.detach()))
        self.ls_idx.append(keep(idx.detach()))

    def compute(self, gathered=None):
        """`gathered`: {"y_true", "prob" | "y_pred"} collected from ALL ranks (the reference's torchmetrics objects synchronise
        across ranks inside compute(); here the caller passes what it gathered).  None = this rank's own lists."""
        import torch
        if self.on_device and self.num_labels == 2:
            d = self.sync_dict() if gathered is None else gathered
            prob, y = torch.as_tensor(d["prob"]).float(), torch.as_tensor(d["y_true"])
            y = y.to(prob.device)
            n = int(y.numel())
            r = rank_metrics(prob.reshape(-1, 1), y.reshape(-1, 1).float())
            self.auroc = float(r["auroc"][0])
            self.acc = int(((prob > 0.5).long() == y).sum()) / n if n else float("nan")
            return
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


def get_metrics(metric_type: str, device=None, num_labels: int = 2, on_device: bool = False):
    """reference `get_metrics` registry (metrics_utils.py:11-13): the two problem types of the BASELINE configs and the multi-label one.
    `on_device`: the two-class single-label object keeps its accumulations on the device (the multi-label one always does)."""
    if metric_type == "single_label_classification":
        return SingleLabelClassificationMetrics(device, num_labels=num_labels, on_device=on_device and num_labels == 2)
    if metric_type == "regression":
        return RegressionMetrics(device, num_labels=num_labels)
    if metric_type == "multi_label_classification":
        return MultiLabelClassificationMetrics(device, num_labels=num_labels)
    raise NotImplementedError(f"metric_type={metric_type!r} (sequence metrics are outside the hot-path scope)")


HITS_DATASETS = {"ogbl-ppa": 100, "ogbl-ddi": 20}           # K of OGB's Hits@K evaluators
MRR_DATASETS = {"ogbl-citation2": 1, "ogbl-wikikg2": 2}      # groups of `link_mrr` (wikikg2: head / tail batches)


def evaluate_ogb(dataset_name: str, input_dict, cnt_neg: int = 1000):
    """reference `evaluate_ogb` for the datasets of the BASELINE configs (src/utils/ogb_utils.py:82-90 ogbl-ppa Hits@100 and :131-138
    ogbl-ddi Hits@20 over positive / negative edges split by label; :92-128 ogbl-citation2 / ogbl-wikikg2: the means of OGB's Hits@1/3/10
    and MRR lists under the reference's key names, :100-101, rows of `cnt_neg` negatives in the order of input_dict["idx"]; :199-204
    PCQM4Mv2 MAE) and the multi-label ones (:187-195 ogbg-molpcba mean AP, :71-79 ogbn-proteins / :173-184 ogbg-molhiv mean ROC-AUC over
    the columns that hold both classes - `_eval_rocauc` :13-29; the rank metrics are taken on the raw logits as the reference feeds
    them).  Tensors or arrays; CUDA tensors go through the HIP kernels.  None for a dataset this package has no evaluator for."""
    if dataset_name in RANK_DATASETS:
        return _evaluate_rank(dataset_name, input_dict["y_true"], input_dict["y_pred"])
    if dataset_name in MRR_DATASETS:
        r = link_mrr(input_dict["y_pred"], input_dict["y_true"], input_dict["idx"], cnt_neg=cnt_neg, groups=MRR_DATASETS[dataset_name])
        return {"hits@1_list": r["hits@1"], "hits@3_list": r["hits@3"], "hits@10_list": r["hits@10"], "ema_mrr_list": r["mrr"]}
    if dataset_name in HITS_DATASETS and _is_cuda(input_dict["y_pred"]):
        k = HITS_DATASETS[dataset_name]
        return {f"hits@{k}": link_hits(input_dict["y_pred"], input_dict["y_true"], k)["hits@k"]}
    y_true, y_pred = np.asarray(_to_np(input_dict["y_true"])), np.asarray(_to_np(input_dict["y_pred"]), np.float64)
    if dataset_name in HITS_DATASETS:
        k = HITS_DATASETS[dataset_name]
        return {f"hits@{k}": hits_at_k(y_pred[y_true == 1], y_pred[y_true == 0], k)}
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
