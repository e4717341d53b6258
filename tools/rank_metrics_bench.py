"""What the multi-label evaluation metrics cost per evaluation pass: the HIP rank kernels (graph-gpt_amd/metrics.py rank_metrics on device
tensors: five launches, one synchronisation, five small copies) against the host path the reference's evaluators take (scikit-learn column
by column on the labelled rows, src/utils/ogb_utils.py:13-29), on synthetic scores at the two validation-split shapes:

  molpcba-valid    n = 43 793, C = 128, ~1.4 % positives, ~40 % NaN labels, metric AP
  proteins-valid   n = 24 679, C = 112, ~50 % positives, no NaN,            metric ROC-AUC

Kernel path: HIP events around rank_metrics (copies included) after warm-up, median.  Host path: a host clock around the scikit-learn loop
on the same arrays (already on the host: the device-to-host copy of the [n, C] tensors it would need first is not charged).  The two
results are compared, too.  Writes profiles/rank_metrics_bench.json.

    python tools/rank_metrics_bench.py [--iters 20] [--host-iters 2] [--out profiles/rank_metrics_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = {"molpcba-valid": dict(n=43793, C=128, pos_rate=0.014, nan_rate=0.40, metric="ap"),
          "proteins-valid": dict(n=24679, C=112, pos_rate=0.50, nan_rate=0.0, metric="auroc")}


def synth(n, C, pos_rate, nan_rate, seed):
    rng = np.random.RandomState(seed)
    y = (rng.rand(n, C) < pos_rate).astype(np.float32)
    s = (rng.randn(n, C) + 1.5 * y).astype(np.float32)
    if nan_rate:
        y[rng.rand(n, C) < nan_rate] = np.nan
    return s, y


def host_path(s, y, metric):
    from sklearn.metrics import average_precision_score, roc_auc_score
    fn = average_precision_score if metric == "ap" else roc_auc_score
    out = np.full(s.shape[1], np.nan)
    for c in range(s.shape[1]):
        if np.sum(y[:, c] == 1) > 0 and np.sum(y[:, c] == 0) > 0:
            lab = y[:, c] == y[:, c]
            out[c] = fn(y[lab, c], s[lab, c])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_metrics_bench.json"))
    a = ap.parse_args()
    importlib.import_module("graph-gpt_amd.build").build()
    met = importlib.import_module("graph-gpt_amd.metrics")
    lib = importlib.import_module("graph-gpt_amd._lib").load()
    torch.cuda.set_device(0)
    rows = {}
    for name, sh in SHAPES.items():
        s, y = synth(sh["n"], sh["C"], sh["pos_rate"], sh["nan_rate"], seed=len(name))
        sd, yd = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
        for _ in range(a.warmup):
            r = met.rank_metrics(sd, yd)
        ms = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = met.rank_metrics(sd, yd)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        host_s = []
        for _ in range(a.host_iters):
            t0 = time.perf_counter()
            want = host_path(s, y, sh["metric"])
            host_s.append(time.perf_counter() - t0)
        dev = float(np.nanmax(np.abs(r[sh["metric"]] - want)))
        agrees = bool(np.array_equal(np.isnan(want), np.isnan(r[sh["metric"]])) and dev <= sh["n"] * 2.0 ** -52)
        n_pos, n_neg = r["n_pos"].astype(np.float64), r["n_neg"].astype(np.float64)
        compares = float((n_pos * (n_pos + n_neg)).sum())
        k_ms, h_ms = statistics.median(ms), statistics.median(host_s) * 1e3
        rows[name] = dict(n=sh["n"], C=sh["C"], metric=sh["metric"], mean_n_pos=round(float(n_pos.mean()), 1),
                          mean_n_neg=round(float(n_neg.mean()), 1), workspace_MB=round(lib.gget_op_rank_metrics_workspace(sh["n"], sh["C"]) / 2 ** 20, 1),
                          kernel_path_ms_median=round(k_ms, 3), kernel_path_ms_min=round(min(ms), 3), kernel_path_ms_max=round(max(ms), 3),
                          pair_compares=compares, giga_compares_per_s=round(compares / (k_ms * 1e-3) / 1e9, 1),
                          host_sklearn_ms_median=round(h_ms, 1), host_over_kernel=round(h_ms / k_ms, 1), max_abs_dev_vs_sklearn=dev,
                          agrees_with_sklearn_to_n_ulp=agrees)
    res = {"what": "rank_metrics on device tensors (HIP events, final copies included, median after warm-up) against scikit-learn column by "
                   "column on the same arrays on the host (host clock); pair_compares = sum over columns of n_pos (n_pos + n_neg)",
           "device": torch.cuda.get_device_name(0), "iters": a.iters, "host_iters": a.host_iters, "rows": rows}
    print(json.dumps(res, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
