"""What the graph-clustering metric of the token-level heads costs per evaluation batch: the HIP kernel (gget_op_cluster_metrics,
csrc/metrics.hip) alone and the metric object end to end (graph-gpt_amd/metrics.py GraphClusteringMetrics: update + compute + to_dict
on device tensors), with the host path (the NumPy count form on arrays that are already on the host) for context, at two shapes:

  small-C   B = 4096, S = 128, C = 8      (16.8 MB of logits)
  wide-C    B = 1024, S = 256, C = 64     (67.1 MB of logits)

"kernel" = HIP events around the C-ABI call alone (inputs and outputs on the device, nothing allocated or copied), median over
`--iters` calls after `--warmup` calls.  bytes_read = B S C 4 (logits) + 2 B S 8 (labels, raw_node_idx); bytes_written = B S 8 (y_pred)
+ B 16 (counts); the rate is (read + written) / kernel time, given as a fraction of the MI355X HBM peak (8 TB/s) and of the achievable
streaming rate (6.3 TB/s).  Both shapes fit the 256 MiB Infinity Cache, so repeated calls on the same arrays may be served from it: the
`rotating` rows time the same call over `--sets` different input sets (together above 256 MiB), which is the figure for a cold batch.
"end_to_end" = a host clock around update (one batch) + compute + to_dict on device tensors, ending in a synchronise.  No threshold is
attached to these numbers.  `--scale` shrinks B (a rehearsal; the file says so).  Writes profiles/cluster_metrics_bench.json.

    python tools/cluster_metrics_bench.py [--iters 50] [--warmup 5] [--scale 1.0] [--out profiles/cluster_metrics_bench.json]
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

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12          # bytes / s
SHAPES = (("small-C", 4096, 128, 8), ("wide-C", 1024, 256, 64))


def synth(B, S, ncls, seed):
    """logits with a planted clustering (the label's column is raised), a quarter of the positions not counted, a fifth unlabelled"""
    rng = np.random.RandomState(seed)
    y = rng.randint(0, ncls, (B, S)).astype(np.int64)
    lg = rng.randn(B, S, ncls).astype(np.float32)
    np.put_along_axis(lg, y[:, :, None], np.take_along_axis(lg, y[:, :, None], 2) + 1.5, 2)
    raw = np.tile(np.arange(S, dtype=np.int64), (B, 1))
    raw[rng.rand(B, S) < 0.25] = -100
    y[rng.rand(B, S) < 0.2] = -100
    return lg, y, raw


def events_ms(fns, iters, warmup):
    """median / min / max of HIP-event times; call i runs fns[i % len(fns)]"""
    for i in range(max(warmup, len(fns))):
        fns[i % len(fns)]()
    torch.cuda.synchronize()
    ts = []
    for i in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fns[i % len(fns)]()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def clock_ms(fn, iters, warmup=0):
    for _ in range(warmup):
        fn()
    ts, out = [], None
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return (statistics.median(ts), min(ts), max(ts)), out


def stat(t):
    return {"median_ms": round(t[0], 4), "min_ms": round(t[1], 4), "max_ms": round(t[2], 4)}


def rate(nbytes, t):
    bps = nbytes / (t[0] * 1e-3)
    return {"bytes_per_s": round(bps, 1), "fraction_of_hbm_peak_8TBs": round(bps / HBM_PEAK, 4),
            "fraction_of_hbm_achievable_6.3TBs": round(bps / HBM_ACHIEVABLE, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--sets", type=int, default=0, help="input sets of the rotating rows (0: as many as exceed 256 MiB together)")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git rev-parse HEAD of the tree)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_metrics_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_metrics_bench: no GPU visible (a time taken without one says nothing)")
    importlib.import_module("graph-gpt_amd.build").build()
    met = importlib.import_module("graph-gpt_amd.metrics")
    _lib = importlib.import_module("graph-gpt_amd._lib")
    lib = _lib.load()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)       # noqa: E731
    res = {"what": "graph-clustering metrics on device tensors (HIP events around the C-ABI call = kernel; host clock around update + "
                   "compute + to_dict = end to end) against the NumPy count form on host arrays; no threshold attached",
           "device": torch.cuda.get_device_name(0), "scale": a.scale, "iters": a.iters, "warmup": a.warmup,
           "hbm_bytes_per_s": {"peak": HBM_PEAK, "achievable": HBM_ACHIEVABLE}, "shapes": {}}
    res["commit"] = a.commit
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    for name, B, S, ncls in SHAPES:
        B = max(int(B * a.scale), 1)
        read, written = B * S * ncls * 4 + 2 * B * S * 8, B * S * 8 + B * 16
        n_sets = a.sets or (2 ** 28) // read + 2
        sets = []
        for k in range(n_sets):
            lg, y, raw = synth(B, S, ncls, seed=k)
            sets.append((torch.from_numpy(lg).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(raw).cuda()))
            if k == 0:
                host = (lg, y, raw)
        y_pred = torch.empty(B, S, dtype=torch.int64, device="cuda")
        counts = torch.empty(B, 4, dtype=torch.int32, device="cuda")
        totals = torch.zeros(4, dtype=torch.int64, device="cuda")

        def call(k):
            lg, y, raw = sets[k]
            return lambda: _lib.check(lib.gget_op_cluster_metrics(lg.data_ptr(), 1, y.data_ptr(), raw.data_ptr(), B, S, ncls, y_pred.data_ptr(),
                                                                  counts.data_ptr(), totals.data_ptr(), st()))

        t_same = events_ms([call(0)], a.iters, a.warmup)
        t_rot = events_ms([call(k) for k in range(n_sets)], max(a.iters, 2 * n_sets), a.warmup)
        # the kernel's integers against the host statement, on the first set
        totals.zero_()
        call(0)()
        want = met._cluster_numpy(*host, ncls)
        assert np.array_equal(y_pred.cpu().numpy(), want[0]) and np.array_equal(counts.cpu().numpy(), want[1])
        assert totals.cpu().numpy().tolist() == want[2].tolist()

        def end_to_end(args, dev):
            m = met.GraphClusteringMetrics(num_labels=ncls)
            lg, y, raw = args
            m.update(lg, y, (torch.arange(B, device=dev), raw))
            m.compute()
            d = m.to_dict()
            return m.results_in_tuple(), int(d["y_pred"].numel())

        t_e, r_dev = clock_ms(lambda: end_to_end(sets[0], "cuda"), min(a.iters, 10), 1)
        cpu = tuple(torch.from_numpy(x) for x in host)
        t_h, r_host = clock_ms(lambda: end_to_end(cpu, "cpu"), a.host_iters)
        t_n, _ = clock_ms(lambda: met._cluster_numpy(*host, ncls), a.host_iters)
        assert r_dev == r_host, (r_dev, r_host)
        row = {"B": B, "S": S, "C": ncls, "bytes_read_per_call": read, "bytes_written_per_call": written, "input_sets": n_sets,
               "acc_recall_precision": list(r_host[0]), "results_equal": True,
               "kernel_same_inputs": dict(stat(t_same), **rate(read + written, t_same)),
               "kernel_rotating_inputs": dict(stat(t_rot), **rate(read + written, t_rot)),
               "device_end_to_end_update_compute_to_dict": stat(t_e), "host_end_to_end_update_compute_to_dict": stat(t_h),
               "host_count_form_alone": stat(t_n)}
        print(name, json.dumps(row), flush=True)
        res["shapes"][name] = row
        del sets
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
