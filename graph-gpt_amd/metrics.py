"""Fine-tune metrics computed from `task_logits`: build-side counterparts of
  SingleLabelClassificationMetrics.update   reference src/utils/metrics_utils.py:38-56   (score = logit1 - logit0 -> AUROC / ACC)
  _eval_ogbl_ppa / _eval_ogbl_ddi (Hits@K)  reference src/utils/ogb_utils.py:82-90, :131-138, :141-152  (K = 100 / 20; `link_hits`)
  _eval_ogbl_citation2 / _eval_ogbl_wikikg2 reference src/utils/ogb_utils.py:92-128, :155-170              (OGB MRR, Hits@1/3/10; `link_mrr`)
  RegressionMetrics / _eval_pcqm4mv2 (MAE)  reference src/utils/metrics_utils.py:143-189, src/utils/ogb_utils.py:199-204
  MultiLabelClassificationMetrics           reference src/utils/metrics_utils.py:91-140     (per-task ROC-AUC of sigmoid(logits))
  _eval_rocauc / OGB _eval_ap               reference src/utils/ogb_utils.py:13-29, :71-79, :173-195 (ogbn-proteins, ogbg-molhiv, ogbg-molpcba)
  GraphClusteringMetrics                    reference src/utils/metrics_utils.py:211-348     (token-level heads: accuracy, clustering recall / precision)
The reference delegates to `torchmetrics` / `ogb` (not installed here); these are plain NumPy statements of the
published definitions, pinned in tests against scikit-learn and closed-form cases.  CUDA tensors take the HIP kernels of
csrc/metrics.hip (`rank_metrics`, `link_hits`, `link_mrr`, `cluster_metrics`); host arrays take the NumPy statements."""
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


# ----------------------------------------------------------------------------- graph clustering: token-level heads (nodev2)
IGNORE = -100       # an unlabelled position in `labels`; a position that is not the one counted occurrence of a node in `raw_node_idx`


def _argmax_first(logits: np.ndarray) -> np.ndarray:
    """torch.argmax over the last axis, stated: the first index of the maximum; a NaN is maximal and the first NaN wins; -0.0 ties +0.0.
    (np.argmax has the same rule; the NaN half of it is spelled out here so that it does not rest on NumPy's propagation.)"""
    lg = np.asarray(logits)
    nan = np.isnan(lg)
    return np.where(nan.any(-1), nan.argmax(-1), np.where(nan, -np.inf, lg).argmax(-1)).astype(np.int64)


def _cluster_numpy(pred_or_logits, labels, raw_node_idx, num_labels):
    """The count form of include/gget.h `gget_op_cluster_metrics` in NumPy (the host path, and what the GPU tests compare the kernel
    with): (y_pred i64 [B,S], counts i32 [B,4] = (t_r, n_r, t_p, n_p), totals i64 [4] = (n_correct, n_kept, n_selected, n_bad)).
    Per (sample, label) the min and max prediction over the kept positions and per (sample, prediction) the min and max label: a value
    is present when its max was written, its group uniform when min == max."""
    p, y, raw = np.asarray(pred_or_logits), np.asarray(labels).astype(np.int64), np.asarray(raw_node_idx).astype(np.int64)
    C = int(num_labels)
    is_logits = p.ndim == 3
    y_pred = _argmax_first(p) if is_logits else p.astype(np.int64)
    B = y.shape[0]
    sel, lab = raw != IGNORE, y != IGNORE
    bad = sel & (lab & ((y < 0) | (y >= C)) | (False if is_logits else (y_pred < 0) | (y_pred >= C)))
    sel = sel & ~bad
    kept = sel & lab
    totals = np.array([(kept & (y_pred == y)).sum(), kept.sum(), sel.sum(), bad.sum()], np.int64)
    b_of = np.broadcast_to(np.arange(B)[:, None], y.shape)[kept]
    yk, pk = y[kept], y_pred[kept]
    counts = np.zeros((B, 4), np.int32)
    for col, key, val in ((0, yk, pk), (2, pk, yk)):
        lo, hi = np.full(B * C, np.iinfo(np.int64).max), np.full(B * C, -1, np.int64)
        np.minimum.at(lo, b_of * C + key, val)
        np.maximum.at(hi, b_of * C + key, val)
        present = (hi >= 0).reshape(B, C)
        counts[:, col] = (present & (lo == hi).reshape(B, C)).sum(1)
        counts[:, col + 1] = present.sum(1)
    return y_pred, counts, totals


def _cluster_hip(pred_or_logits, labels, raw_node_idx, num_labels, totals=None):
    """The same three results from the HIP kernel for CUDA tensors, as device tensors: one launch on the current stream, no
    synchronisation, no copy.  `totals` (i64 [4] on the device) is added to.  No fallback: a library without the entry is an error."""
    import ctypes as C
    import torch
    from . import _lib
    lib = _lib.load()
    is_logits = pred_or_logits.dim() == 3
    dev = pred_or_logits.device
    p = (pred_or_logits.detach().float() if is_logits else pred_or_logits.detach().long()).contiguous()
    y, raw = labels.detach().to(dev).long().contiguous(), raw_node_idx.detach().to(dev).long().contiguous()
    B, S = y.shape
    y_pred = torch.empty(B, S, dtype=torch.int64, device=dev)
    counts = torch.zeros(B, 4, dtype=torch.int32, device=dev)
    totals = torch.zeros(4, dtype=torch.int64, device=dev) if totals is None else totals
    with torch.cuda.device(dev):
        _lib.check(lib.gget_op_cluster_metrics(p.data_ptr(), int(is_logits), y.data_ptr(), raw.data_ptr(), B, S, int(num_labels),
                                               y_pred.data_ptr(), counts.data_ptr(), totals.data_ptr(),
                                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return y_pred, counts, totals


def cluster_metrics(pred_or_logits, labels, raw_node_idx, num_labels: int, totals=None):
    """What GraphClusteringMetrics.update takes from one batch (reference src/utils/metrics_utils.py:231-295 and `get_acc_per_graph`
    :340-348), as exact integer counts (include/gget.h `gget_op_cluster_metrics`).  pred_or_logits: logits [B,S,C] (prediction = arg-max,
    torch's rule) or integer predictions [B,S]; labels [B,S], -100 = unlabelled; raw_node_idx [B,S], -100 = not a counted position.
    Returns {"y_pred" i64 [B,S], "counts" i32 [B,4] = (t_r, n_r, t_p, n_p) per sample, "totals" i64 [4] = (n_correct, n_kept, n_selected,
    n_bad)}; a `totals` that is passed in is added to and returned.  CUDA tensors go through the HIP kernel and stay on the device (one
    launch, no synchronisation); CPU tensors and arrays through the NumPy statement of the same counts (tensors in, tensors out).  CUDA
    tensors with num_labels above the kernel's class limit (`_lib.CLUSTER_MAX_C`) take the NumPy statement too, through a host copy, and
    come back as device tensors."""
    from . import _lib
    shape = tuple(labels.shape)
    if len(shape) != 2 or tuple(raw_node_idx.shape) != shape or tuple(pred_or_logits.shape[:2]) != shape or len(pred_or_logits.shape) not in (2, 3):
        raise ValueError(f"cluster_metrics: pred_or_logits {tuple(pred_or_logits.shape)}, labels {shape} and raw_node_idx "
                         f"{tuple(raw_node_idx.shape)} must be [B,S,C] or [B,S], [B,S] and [B,S]")
    if len(pred_or_logits.shape) == 3 and pred_or_logits.shape[2] != num_labels:
        raise ValueError(f"cluster_metrics: logits of {pred_or_logits.shape[2]} classes, num_labels = {num_labels}")
    if _is_cuda(pred_or_logits) and num_labels <= _lib.CLUSTER_MAX_C:
        y_pred, counts, totals = _cluster_hip(pred_or_logits, labels, raw_node_idx, num_labels, totals)
        return {"y_pred": y_pred, "counts": counts, "totals": totals}
    y_pred, counts, tot = _cluster_numpy(_to_np(pred_or_logits), _to_np(labels), _to_np(raw_node_idx), num_labels)
    if hasattr(pred_or_logits, "detach"):
        import torch
        dev = pred_or_logits.device
        y_pred, counts, tot = torch.from_numpy(y_pred).to(dev), torch.from_numpy(counts).to(dev), torch.from_numpy(tot).to(dev)
    if totals is not None:
        totals += tot
        tot = totals
    return {"y_pred": y_pred, "counts": counts, "totals": tot}


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


class GraphClusteringMetrics:
    """Counterpart of the reference class of the same name (src/utils/metrics_utils.py:211-348; `metric_type = "graph_clustering"`, the
    metric of the token-level heads): per batch `update(logits, labels, (idx, raw_node_idx))` with logits [B,S,C] (or integer predictions
    [B,S]), labels [B,S] (-100 = unlabelled), idx [B] and raw_node_idx [B,S] (-100 at every position that is not the one counted
    occurrence of a node).  A position is selected when raw_node_idx != -100 and kept when it is selected and labelled.
      acc        n_correct / n_kept over all batches: the micro accuracy of torchmetrics' multiclass `Accuracy`, which the reference
                 uses.  torchmetrics is not installed where this package is tested, so this one rule is restated, not pinned against it.
      recall     mean over the samples of t_r / n_r (fp32 quotient, as the reference's mean of an fp32 0 / 1 list): n_r distinct labels
                 among the sample's kept positions, t_r those whose positions all carry one prediction.
      precision  the same with the roles of label and prediction swapped (t_p / n_p).
    A sample without a kept position gives 0 / 0 = NaN on both sides and makes the means NaN, as in the reference (mean of an empty
    tensor); `n_empty` counts such samples.  The reference raises IndexError for a sample with exactly ONE selected position (squeeze()
    to 0-dim, then indexing, :271-280); here such a sample is defined by the count form: 1 / 1 if the position is kept, NaN if not.
    `update` keeps everything on the device it arrives on - predictions, labels, raw_node_idx, idx, the per-sample counts and one
    `totals` tensor for the whole pass (`cluster_metrics`: one kernel launch per batch for CUDA tensors) - and never synchronises;
    `compute` makes the one host transfer (counts and totals in one tensor), takes the means in fp64 over the fp32 per-sample
    quotients, and raises ValueError when a selected position carried a label outside [0, num_labels) (or, for integer predictions, a
    prediction outside it).  `sync_dict` returns the per-sample counts and the totals, so `compute(gathered)` on the concatenation from
    all ranks gives the means over ALL samples - deliberately different from the reference, whose recall / precision stay per rank and
    whose accuracy alone is synchronised (by torchmetrics)."""

    def __init__(self, device=None, num_labels: int = 2, **kwargs):
        self.device, self.num_labels = device, num_labels
        self.acc = self.recall = self.precision = self.n_empty = None
        self.ls_recall = self.ls_precision = None             # fp32 per-sample quotients, after compute()
        self.totals = None
        self.ls_pred, self.ls_labels, self.ls_idx, self.ls_node_idx, self.ls_counts = [], [], [], [], []

    def update(self, logits, labels, idx):
        assert isinstance(idx, tuple), f"idx type should be tuple, but it is {type(idx)}"
        idx, raw_node_idx = idx
        assert len(logits.shape) in {2, 3}, f"logits shape: {logits.shape}"
        assert len(labels.shape) == 2, f"labels shape: {labels.shape}"
        logits, labels = logits.detach(), labels.detach()
        raw_node_idx, idx = raw_node_idx.detach().to(logits.device), idx.detach().to(logits.device)
        r = cluster_metrics(logits, labels, raw_node_idx, self.num_labels, totals=self.totals)
        self.totals = r["totals"]
        self.ls_pred.append(r["y_pred"].reshape(-1))
        self.ls_labels.append(labels.reshape(-1))
        self.ls_node_idx.append(raw_node_idx.reshape(-1))
        self.ls_idx.append(idx.reshape(-1, 1).expand(-1, labels.shape[1]).reshape(-1))       # metrics_utils.py:261-263
        self.ls_counts.append(r["counts"])

    def sync_dict(self):
        """what compute() needs from every rank: counts i32 [N,4] per sample, totals i64 [4]"""
        import torch
        return {"counts": torch.cat(self.ls_counts), "totals": self.totals}

    def compute(self, gathered=None):
        """`gathered`: {"counts" [N,4], "totals" [4 k]} concatenated from ALL ranks (tensors or arrays); None = this rank's own."""
        import torch
        d = self.sync_dict() if gathered is None else gathered
        counts, totals = torch.as_tensor(d["counts"]), torch.as_tensor(d["totals"])
        flat = torch.cat([counts.reshape(-1).long(), totals.reshape(-1).long().to(counts.device)]).cpu().numpy()      # the one transfer
        n4 = counts.numel()
        c, tot = flat[:n4].reshape(-1, 4), flat[n4:].reshape(-1, 4).sum(0)
        n_correct, n_kept, _, n_bad = (int(v) for v in tot)
        if n_bad:
            raise ValueError(f"GraphClusteringMetrics: {n_bad} selected positions with a label (or a given prediction) outside "
                             f"[0, {self.num_labels})")
        with np.errstate(invalid="ignore", divide="ignore"):
            self.ls_recall = c[:, 0].astype(np.float32) / c[:, 1].astype(np.float32)
            self.ls_precision = c[:, 2].astype(np.float32) / c[:, 3].astype(np.float32)
        nan = float("nan")
        self.recall = float(self.ls_recall.astype(np.float64).mean()) if len(c) else nan
        self.precision = float(self.ls_precision.astype(np.float64).mean()) if len(c) else nan
        self.n_empty = int((c[:, 1] == 0).sum())
        self.acc = n_correct / n_kept if n_kept else nan

    def to_dict(self):
        """y_true, y_pred, idx (the sample's idx repeated) and node_idx over the selected positions in row-major order - one boolean
        index per tensor, on the device the batches arrived on"""
        import torch
        node = torch.cat(self.ls_node_idx)
        sel = node != IGNORE
        return {"y_true": torch.cat(self.ls_labels)[sel], "y_pred": torch.cat(self.ls_pred)[sel], "idx": torch.cat(self.ls_idx)[sel],
                "node_idx": node[sel]}

    def get_output_shape(self, dim, key=None):
        return dim

    def results_in_tuple(self):
        return self.acc, self.recall, self.precision

    def results_in_str_tuple(self):
        return str(self.acc), str(self.recall), str(self.precision)

    def results_in_details(self, prefix=""):
        return f"{prefix} Recall: {self.recall}, {prefix} Precision: {self.precision}, {prefix} ACC: {self.acc}"

    def results_in_dict(self, prefix=""):
        r, p = self.recall, self.precision
        return {f"{prefix} ACC": self.acc, f"{prefix} Recall": r, f"{prefix} Precision": p,
                "EMA F1": 2 * r * p / (r + p) if r + p != 0 else float("nan")}


def get_metrics(metric_type: str, device=None, num_labels: int = 2, on_device: bool = False):
    """reference `get_metrics` registry (metrics_utils.py:11-13): the two problem types of the BASELINE configs, the multi-label one and
    the graph-clustering one of the token-level heads.
    `on_device`: the two-class single-label object keeps its accumulations on the device (the multi-label and clustering ones always do)."""
    if metric_type == "graph_clustering":
        return GraphClusteringMetrics(device, num_labels=num_labels)
    if metric_type == "single_label_classification":
        return SingleLabelClassificationMetrics(device, num_labels=num_labels, on_device=on_device and num_labels == 2)
    if metric_type == "regression":
        return RegressionMetrics(device, num_labels=num_labels)
    if metric_type == "multi_label_classification":
        return MultiLabelClassificationMetrics(device, num_labels=num_labels)
    raise NotImplementedError(f"metric_type={metric_type!r} (sequence metrics are outside the hot-path scope)")


def compare_metrics_res(curr_res, prev_best_res):
    """reference `compare_metrics_res` (metrics_utils.py:192-208): (is `curr_res` the new best, the result to keep).  The result dicts
    are compared on ONE key: their only key, or the single key that starts with "ema" (any case); a key that names an MAE or a loss is
    better when smaller, every other one when larger, and a tie keeps the previous best."""
    keys = list(curr_res.keys())
    if len(keys) > 1:
        keys = [k for k in keys if k.lower().startswith("ema")]
        assert len(keys) == 1, f"curr_res keys: {list(curr_res.keys())}"
    key = keys[0]
    smaller_wins = any(word in key.lower() for word in ("mae", "loss"))
    better = curr_res[key] < prev_best_res[key] if smaller_wins else curr_res[key] > prev_best_res[key]
    return (True, curr_res) if better else (False, prev_best_res)


HITS_DATASETS = {"ogbl-ppa": 100, "ogbl-ddi": 20}         # K of OGB's Hits@K evaluators
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
    if dataset_name not in HITS_DATASETS and dataset_name != "PCQM4Mv2":      # (before the host copies below: device tensors stay put)
        return None
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
