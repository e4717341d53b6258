"""What returning the attention weights (`output_attentions=True`) costs per decoder layer: the HIP kernel behind gget_attention_probs
(gget_op_attn_probs, csrc/attention.hip attn_probs_kernel) alone, at the shapes of the project's workloads:

  C1   B = 256, S = 32,   H = 12      (6.3 MB written)
  C3   B = 256, S = 256,  H = 12      (403 MB written)
  C4   B = 16,  S = 2048, H = 12      (1.6 GB written)

Full-length samples, bi-directional, no dropout (and one row per shape with p = 0.1: the hash per element).  Time = HIP events around
the C-ABI call alone (q | k, lse and the output on the device, nothing allocated or copied), median over `--iters` calls after
`--warmup` calls.  The kernel writes B H S^2 2 bytes (and reads 2 B S H 128 bytes of q | k plus the lse, 1 / S of that and less) against
128 B H S^2 FLOP: it is bound by its stores, so each row carries bytes written / time as a fraction of the achievable HBM rate
(6.3 TB/s; peak 8 TB/s).  The C1 output fits the 256 MiB Infinity Cache: its figure is a launch-latency figure, not a bandwidth one.
There is no parent-commit time to compare with and no threshold is attached.  `--scale` shrinks B (a rehearsal; the file says so).

    python tools/attn_probs_bench.py [--iters 30] [--warmup 3] [--scale 1.0] [--out profiles/attn_probs.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12          # bytes / s
SHAPES = (("C1", 256, 32, 12), ("C3", 256, 256, 12), ("C4", 16, 2048, 12))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git rev-parse HEAD of the tree)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_probs.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_probs_bench: no GPU visible (a time taken without one says nothing)")
    importlib.import_module("graph-gpt_amd.build").build()
    _lib = importlib.import_module("graph-gpt_amd._lib")
    lib = _lib.load()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)       # noqa: E731
    P = lambda t: C.c_void_p(t.data_ptr())                                  # noqa: E731
    res = {"what": "attention weights of one decoder layer (gget_op_attn_probs): HIP events around the C-ABI call; bytes written / time "
                   "against the achievable HBM rate; no threshold attached",
           "device": torch.cuda.get_device_name(0), "scale": a.scale, "iters": a.iters, "warmup": a.warmup,
           "hbm_bytes_per_s": {"peak": HBM_PEAK, "achievable": HBM_ACHIEVABLE}, "shapes": {}}
    res["commit"] = a.commit
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    for name, B, S, H in SHAPES:
        B = max(int(B * a.scale), 1)
        d = 64 * H
        g = torch.Generator(device="cuda").manual_seed(S)
        qkv = torch.randn(B * S, 3 * d, generator=g, device="cuda").to(torch.bfloat16)
        key_len = torch.full((B,), S, dtype=torch.int32, device="cuda")
        attn = torch.empty(B * S, d, dtype=torch.bfloat16, device="cuda")
        lse = torch.empty(B, H, S, device="cuda")
        _lib.check(lib.gget_op_attn_fwd(P(qkv), P(key_len), P(attn), P(lse), B, S, H, 0, None, None, None, 0.0, 0, st()))
        out = torch.empty(B, H, S, S, dtype=torch.bfloat16, device="cuda")
        written = out.numel() * 2
        read = 2 * B * S * d * 2 + lse.numel() * 4
        row = {"B": B, "S": S, "H": H, "bytes_written": written, "bytes_read_once": read, "flop": 128 * B * H * S * S}
        for tag, p in (("no_dropout", 0.0), ("dropout_0.1", 0.1)):
            t = events_ms(lambda: _lib.check(lib.gget_op_attn_probs(P(qkv), P(lse), P(key_len), None, None, None, P(out), B, S, H, 0, p, 77,
                                                                    st())), a.iters, a.warmup)
            bps = written / (t[0] * 1e-3)
            row[tag] = {"median_ms": round(t[0], 4), "min_ms": round(t[1], 4), "max_ms": round(t[2], 4),
                        "written_bytes_per_s": round(bps, 1), "fraction_of_hbm_achievable_6.3TBs": round(bps / HBM_ACHIEVABLE, 4),
                        "fraction_of_hbm_peak_8TBs": round(bps / HBM_PEAK, 4)}
        # a sanity check of what was timed: rows of the un-dropped weights sum to 1 (bf16 roundings of S terms)
        _lib.check(lib.gget_op_attn_probs(P(qkv), P(lse), P(key_len), None, None, None, P(out), B, S, H, 0, 0.0, 0, st()))
        sums = out[:: max(B // 4, 1), ::5].float().sum(-1)
        row["row_sum_max_deviation"] = round(float((sums - 1.0).abs().max()), 6)
        assert row["row_sum_max_deviation"] < 2.0 ** -7, row
        print(name, json.dumps(row), flush=True)
        res["shapes"][name] = row
        del out, qkv, attn, lse
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
