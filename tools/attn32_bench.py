#!/usr/bin/env python
"""Forward and backward of the head-width-32 attention kernels (csrc/attention32.hip, gget_op_attn_fwd_hd / _bwd_hd) alone, under HIP
events, at B 256 / S 32 / H 12 and B 16 / S 2048 / H 12 - and, for scale only, the 64-wide GENERAL kernels (attn_fwd_kernel /
attn_bwd_dq_kernel / attn_bwd_dkv_kernel: the long-sequence, per-sample and one-pass forms switched off through the launch menu's
environment keys) at the same T * d (H 6).  Random operands, full-length rows, dropout 0 and 0.1; every shape is warmed up, the four
calls of a shape are alternated over the rounds in one process, and the median and the minimum of the rounds are kept.

    python tools/attn32_bench.py [--out profiles/hd32_attention.json] [--rounds 7]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

for key in ("GGET_ATTN_BIG", "GGET_ATTN_DENSE", "GGET_ATTN_SMALL", "GGET_ATTN_FUSED", "GGET_ATTN_BY_SAMPLE"):     # before the library reads its menu
    os.environ[key] = "0"

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
L = importlib.import_module("graph-gpt_amd._lib")

SHAPES = [(256, 32, 12), (16, 2048, 12)]      # (B, S, H at head width 32)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per call


def problem(lib, B, S, H, hd, p, st):
    d, T = H * hd, B * S
    g = torch.Generator(device="cuda").manual_seed(1234 + hd)
    qkv = torch.randn(T, 3 * d, device="cuda", generator=g).to(torch.bfloat16)
    dout = torch.randn(T, d, device="cuda", generator=g).to(torch.bfloat16)
    out, dqkv = torch.empty(T, d, dtype=torch.bfloat16, device="cuda"), torch.empty_like(qkv)
    lse, delta = torch.empty(B * H * S, device="cuda"), torch.empty(B * H * S, device="cuda")
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    keep = (qkv, dout, out, dqkv, lse, delta, lens)

    def fwd():
        L.check(lib.gget_op_attn_fwd_hd(P(qkv), P(lens), None, None, None, P(out), P(lse), B, S, H, hd, 0, p, 7, st))

    def bwd():
        L.check(lib.gget_op_attn_bwd_hd(P(qkv), P(out), P(dout), P(lse), P(lens), None, None, None, P(dqkv), P(delta), B, S, H, hd, 0, None, None,
                                        None, p, 7, st))
    return fwd, bwd, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn32_bench: no GPU (a timing needs the device; nothing is measured on the CPU)")
    lib = L.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "unit": "us per call (HIP events)",
           "menu": "GGET_ATTN_BIG=0 GGET_ATTN_DENSE=0 GGET_ATTN_SMALL=0 GGET_ATTN_FUSED=0 GGET_ATTN_BY_SAMPLE=0 (64-wide: general kernels)",
           "cases": []}
    for B, S, H in SHAPES:
        for p in (0.0, 0.1):
            calls = {}
            for hd, heads in ((32, H), (64, H // 2)):
                f, b, keep = problem(lib, B, S, heads, hd, p, st)
                calls[f"fwd_hd{hd}"], calls[f"bwd_hd{hd}"], calls[f"_keep{hd}"] = f, b, keep
            names = [n for n in calls if not n.startswith("_")]
            iters = 20 if S <= 64 else 5
            for n in names:                       # warm-up: code objects, clocks
                timed(calls[n], 3)
            runs = {n: [] for n in names}
            for _ in range(a.rounds):             # alternated in one process
                for n in names:
                    runs[n].append(timed(calls[n], iters))
            flops = 4.0 * B * H * S * S * 32      # QK^T and PV of the forward (the same count at H / 2 heads of width 64)
            case = {"B": B, "S": S, "H_hd32": H, "H_hd64": H // 2, "dropout_p": p, "forward_flop": flops}
            for n in names:
                r = sorted(runs[n])
                case[n] = {"median_us": round(r[len(r) // 2], 2), "min_us": round(r[0], 2), "max_us": round(r[-1], 2)}
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
