"""An independent statement of the graph-clustering counts (graph-gpt_amd/metrics.py `cluster_metrics`, include/gget.h
`gget_op_cluster_metrics`) with Python sets, and the input patterns that tests/test_metrics_cluster.py and
tests/test_gpu_cluster_metrics.py share.

Per sample, over its kept positions (raw_node_idx != -100 and label != -100, bad positions left out): by_label = {label: set of the
predictions seen with it}, by_pred = {prediction: set of the labels seen with it}.  n_r = len(by_label), t_r = the labels whose set has
one element; n_p / t_p the same of by_pred.  A selected position is bad when its label is neither -100 nor in [0, C), or - for
predictions that were given, not taken from logits - its prediction is outside [0, C)."""
import math

import numpy as np

IGNORE = -100


def argmax_first(row):
    """first index of the maximum; a NaN is maximal and the first NaN wins; -0.0 == +0.0"""
    for j, v in enumerate(row):
        if math.isnan(v):
            return j
    best = 0
    for j, v in enumerate(row):
        if v > row[best]:
            best = j
    return best


def cluster_sets(pred_or_logits, labels, raw_node_idx, C):
    """(y_pred [B,S], counts [B,4] = (t_r, n_r, t_p, n_p), totals [4] = (n_correct, n_kept, n_selected, n_bad)) as nested Python lists"""
    p, y, raw = np.asarray(pred_or_logits), np.asarray(labels), np.asarray(raw_node_idx)
    given = p.ndim == 2
    B, S = y.shape
    y_pred = [[int(p[b, s]) if given else argmax_first([float(v) for v in p[b, s]]) for s in range(S)] for b in range(B)]
    counts, totals = [], [0, 0, 0, 0]
    for b in range(B):
        by_label, by_pred = {}, {}
        for s in range(S):
            if int(raw[b, s]) == IGNORE:
                continue
            lab, pred = int(y[b, s]), y_pred[b][s]
            if (lab != IGNORE and not 0 <= lab < C) or (given and not 0 <= pred < C):
                totals[3] += 1
                continue
            totals[2] += 1
            if lab == IGNORE:
                continue
            totals[1] += 1
            totals[0] += int(pred == lab)
            by_label.setdefault(lab, set()).add(pred)
            by_pred.setdefault(pred, set()).add(lab)
        counts.append([sum(len(v) == 1 for v in by_label.values()), len(by_label), sum(len(v) == 1 for v in by_pred.values()), len(by_pred)])
    return y_pred, counts, totals


# ------------------------------------------------------------------------------------------------ shared input patterns
LOGIT_KINDS = ("random", "ties", "equal", "zeros", "nan", "neginf")


def make_logits(B, S, C, kind, rng):
    if kind == "random":
        return rng.randn(B, S, C).astype(np.float32)
    if kind == "ties":                                       # one decimal: ties inside a row
        return np.round(rng.randn(B, S, C), 1).astype(np.float32)
    if kind == "equal":
        return np.full((B, S, C), 0.75, np.float32)
    if kind == "zeros":                                      # -0.0 / +0.0 only: index 0 everywhere
        return np.where(rng.rand(B, S, C) < 0.5, -0.0, 0.0).astype(np.float32)
    if kind == "nan":                                        # NaN at about a third of the positions, sometimes twice in a row
        lg = np.round(rng.randn(B, S, C), 1).astype(np.float32)
        lg[rng.rand(B, S, C) < 0.5 / C] = np.nan
        return lg
    if kind == "neginf":                                     # rows of -inf only, and rows with one finite entry
        lg = np.full((B, S, C), -np.inf, np.float32)
        one = rng.rand(B, S) < 0.5
        lg[one, rng.randint(0, C, int(one.sum()))] = rng.randn(int(one.sum())).astype(np.float32)
        return lg
    raise KeyError(kind)


LABEL_KINDS = ("mixed", "first_empty", "one_kept", "all_equal", "all_distinct", "none_selected", "bad")


def make_labels(B, S, C, kind, rng):
    """(labels, raw_node_idx) int64 [B,S]; "bad" puts a label of C and a label of -1 at selected positions"""
    y = rng.randint(0, C, (B, S)).astype(np.int64)
    raw = np.tile(np.arange(S, dtype=np.int64), (B, 1))
    if kind in ("mixed", "first_empty", "bad"):
        y[rng.rand(B, S) < 0.25] = IGNORE
        raw[rng.rand(B, S) < 0.25] = IGNORE
    if kind == "first_empty":                                # sample 0 has selected positions but none labelled
        y[0] = IGNORE
    if kind == "one_kept":                                   # exactly one kept position per sample
        keep = rng.randint(0, S, B)
        lab = y[np.arange(B), keep]
        y[:] = IGNORE
        y[np.arange(B), keep] = lab
    if kind == "all_equal":
        y[:] = rng.randint(0, C)
    if kind == "all_distinct":                               # the first min(S, C) positions carry a permutation of the labels, the rest none
        y[:] = IGNORE
        n = min(S, C)
        for b in range(B):
            y[b, :n] = rng.permutation(C)[:n]
    if kind == "none_selected":
        raw[:] = IGNORE
    if kind == "bad":
        raw[0, 0], y[0, 0] = 0, C
        raw[B - 1, S - 1], y[B - 1, S - 1] = S - 1, -1
    return y, raw
