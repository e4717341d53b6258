"""What the link-prediction evaluation metrics cost per evaluation pass: the HIP kernels (graph-gpt_amd/metrics.py link_hits / link_mrr and
the on-device AUROC of SingleLabelClassificationMetrics, i.e. rank_metrics on one column) against the host statements the parent commit
had (metrics.hits_at_k, metrics.mrr, metrics.auroc) on the same synthetic arrays, at about the size of the two validation splits:

  ppa-valid        n = 4 221 824 positives + 3 000 000 negatives = 7 221 824 edges,          Hits@100
  citation2-valid  n = 86 596 positives x (1 + 1000) = 86 682 596 edges, idx a random permutation, MRR

Device path: "kernels" = HIP events around the C-ABI call alone (inputs and workspace on the device, nothing copied), median after
warm-up; "end_to_end" = a host clock around the Python surface on device tensors, which allocates the workspace, launches, synchronises
and copies the results to the host (for link_mrr that includes the two [groups, P] count lists).  Host path: a host clock around the
NumPy statement on arrays that are already on the host (the device-to-host copy it would need first is timed apart, as "d2h").
metrics.auroc's tie handling is a Python loop over every element, so it is timed on a prefix of `--auroc-host-n` entries and NOT
extrapolated; the on-device AUROC (n_pos * n compare-and-adds) is timed once per shape at full size unless --skip-auroc.
`--scale` shrinks both shapes (a rehearsal; the file says so).  Writes profiles/link_metrics_bench.json.

    python tools/link_metrics_bench.py [--iters 10] [--scale 1.0] [--skip-auroc] [--out profiles/link_metrics_bench.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def synth_ppa(scale, seed=0):
    n_pos, n_neg = int(4_221_824 * scale), int(3_000_000 * scale)
    rng = np.random.RandomState(seed)
    y = np.concatenate([np.ones(n_pos, np.int64), np.zeros(n_neg, np.int64)])
    s = (rng.randn(n_pos + n_neg) + 1.5 * y).astype(np.float32)
    perm = rng.permutation(n_pos + n_neg)
    return s[perm], y[perm]


def synth_citation2(scale, cnt_neg=1000, seed=1):
    P = max(int(86_596 * scale), 1)
    rng = np.random.RandomState(seed)
    n = P * (1 + cnt_neg)
    y = np.zeros(n, np.int64)
    y[::1 + cnt_neg] = 1                                 # in idx order every positive stands in front of its negatives
    s = rng.standard_normal(n, dtype=np.float32) + 2.0 * y.astype(np.float32)
    perm = rng.permutation(n)
    return s[perm], y[perm], perm.astype(np.int64), P


def events_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def clock_ms(fn, iters, warmup=0):
    for _ in range(warmup):
        fn()
    ts = []
    out = None
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return (statistics.median(ts), min(ts), max(ts)), out


def stat(t):
    return {"median_ms": round(t[0], 4), "min_ms": round(t[1], 4), "max_ms": round(t[2], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--skip-auroc", action="store_true")
    ap.add_argument("--auroc-host-n", type=int, default=1_000_000)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git rev-parse HEAD of the tree)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_metrics_bench.json"))
    a = ap.parse_args()
    importlib.import_module("graph-gpt_amd.build").build()
    met = importlib.import_module("graph-gpt_amd.metrics")
    _lib = importlib.import_module("graph-gpt_amd._lib")
    lib = _lib.load()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)       # noqa: E731
    res = {"what": "link-prediction metrics on device tensors (HIP events around the C-ABI call = kernels; host clock around the Python "
                   "surface = end to end with workspace allocation and the final copies) against the NumPy statements on host arrays",
           "device": torch.cuda.get_device_name(0), "scale": a.scale, "iters": a.iters, "shapes": {}}
    res["commit"] = a.commit
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass

    # ------------------------------------------------------------------ ppa-valid: Hits@100
    s, y = synth_ppa(a.scale)
    n = len(s)
    sd, yd = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
    out = [torch.zeros(1, dtype=dt, device="cuda") for dt in (torch.int64, torch.int64, torch.float32, torch.int64, torch.int32)]
    nbytes = int(lib.gget_op_link_hits_workspace(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    call = lambda: _lib.check(lib.gget_op_link_hits(sd.data_ptr(), yd.data_ptr(), n, 100, *[o.data_ptr() for o in out], ws.data_ptr(),   # noqa: E731
                                                    nbytes, st()))
    t_k = events_ms(call, a.iters, a.warmup)
    t_e, r_dev = clock_ms(lambda: met.link_hits(sd, yd, 100), a.iters, 1)
    t_c, _ = clock_ms(lambda: (sd.cpu(), yd.cpu()), 2)
    t_h, r_host = clock_ms(lambda: met.hits_at_k(s[y == 1], s[y == 0], 100), a.host_iters)
    assert r_dev["hits@k"] == r_host, (r_dev, r_host)
    row = {"n": n, "n_pos": int(y.sum()), "n_neg": int(n - y.sum()), "K": 100, "hits@100": r_host, "results_equal": True,
           "bytes_read_per_call": 5 * n * 12, "workspace_bytes": nbytes, "device_kernels": stat(t_k), "device_end_to_end": stat(t_e),
           "d2h_scores_labels": stat(t_c), "host_hits_at_k": stat(t_h)}
    print("ppa-valid", json.dumps(row), flush=True)
    res["shapes"]["ppa-valid"] = row
    ppa = (sd, yd, s, y)

    # ------------------------------------------------------------------ citation2-valid: MRR
    s, y, idx, P = synth_citation2(a.scale)
    n = len(s)
    sd, yd, xd = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(idx).cuda()
    out = [torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"),
           torch.zeros(1, P, dtype=torch.int32, device="cuda"), torch.zeros(1, P, dtype=torch.int32, device="cuda"),
           torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"),
           torch.zeros(2, dtype=torch.int32, device="cuda")]
    nbytes = int(lib.gget_op_link_mrr_workspace(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    call = lambda: _lib.check(lib.gget_op_link_mrr(sd.data_ptr(), yd.data_ptr(), xd.data_ptr(), n, 1000, 1, *[o.data_ptr() for o in out],   # noqa: E731
                                                   ws.data_ptr(), nbytes, st()))
    t_k = events_ms(call, a.iters, a.warmup)
    del ws
    t_e, r_dev = clock_ms(lambda: met.link_mrr(sd, yd, xd, cnt_neg=1000), max(a.iters // 2, 1), 1)
    t_c, _ = clock_ms(lambda: (sd.cpu(), yd.cpu(), xd.cpu()), 2)

    def host_mrr():
        order = np.argsort(idx, kind="stable")
        ys, ss = y[order], s[order]
        return met.mrr(ss[ys == 1], ss[ys == 0].reshape(-1, 1000))

    t_h, r_host = clock_ms(host_mrr, a.host_iters)
    assert abs(r_dev["mrr"] - r_host) <= P * 2.0 ** -52 * r_host, (r_dev["mrr"], r_host)
    row = {"n": n, "P": P, "cnt_neg": 1000, "mrr": r_host, "mrr_abs_dev_device_vs_host": abs(r_dev["mrr"] - r_host),
           "workspace_bytes": nbytes, "device_kernels": stat(t_k), "device_end_to_end": stat(t_e), "d2h_scores_labels_idx": stat(t_c),
           "host_sort_by_idx_and_mrr": stat(t_h)}
    print("citation2-valid", json.dumps(row), flush=True)
    res["shapes"]["citation2-valid"] = row

    # ------------------------------------------------------------------ AUROC of the metric object (class-1 probability stands in: any score)
    m = min(a.auroc_host_n, len(ppa[2]))
    t_h, au_host = clock_ms(lambda: met.auroc(ppa[2][:m], ppa[3][:m]), 1)
    t_d, r_small = clock_ms(lambda: met.rank_metrics(ppa[0][:m].reshape(-1, 1), ppa[1][:m].reshape(-1, 1).float()), 1, 1)
    assert abs(float(r_small["auroc"][0]) - au_host) <= 1e-9
    res["auroc"] = {"host_prefix": {"n": m, "host_auroc_python_loop": stat(t_h), "device_rank_metrics_same_prefix": stat(t_d),
                                    "auroc": au_host, "note": "metrics.auroc on the first n entries of ppa-valid; not extrapolated"}}
    print("auroc prefix", json.dumps(res["auroc"]["host_prefix"]), flush=True)
    if not a.skip_auroc:
        for name, (d_s, d_y) in (("ppa-valid", (ppa[0], ppa[1])), ("citation2-valid", (sd, yd))):
            t_d, r = clock_ms(lambda: met.rank_metrics(d_s.reshape(-1, 1), d_y.reshape(-1, 1).float()), 1)
            n_pos, n_all = int(r["n_pos"][0]), int(r["n_pos"][0] + r["n_neg"][0])
            res["auroc"][name] = {"n": n_all, "n_pos": n_pos, "compare_and_adds": n_pos * n_all, "auroc": float(r["auroc"][0]),
                                  "device_rank_metrics_once": stat(t_d)}
            print("auroc", name, json.dumps(res["auroc"][name]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
