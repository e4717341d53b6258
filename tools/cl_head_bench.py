#!/usr/bin/env python3
"""What the contrastive head costs a pre-training step: the base model at B 256 / S 32 / F 13, forward + backward + AdamW of the
pretrain-cl engine kind against the plain pre-train kind in ONE process, alternated, and the three operator-level launches alone
(gget_op_cl_embed_fwd, gget_op_cl_loss_fwd, gget_op_cl_bwd on [256, 768] operands).  Writes profiles/cl_head.json (or --out).
Recorded, not gated.

    python tools/cl_head_bench.py [--rounds 5] [--steps 30] [--out profiles/cl_head.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spec_mod = importlib.import_module("graph-gpt_amd.spec")
synth = importlib.import_module("graph-gpt_amd.synth")
weights = importlib.import_module("graph-gpt_amd.weights")
eng_mod = importlib.import_module("graph-gpt_amd.engine")
L = importlib.import_module("graph-gpt_amd._lib")

B, S, F, V = 256, 32, 13, 756


def make_engine(kind, batch):
    spec = spec_mod.spec_from_size("base", kind=kind, vocab_size=V, stacked_feat=F, next_n_token=F, causal=False, max_position=1024)
    e = eng_mod.Engine(spec, B * S, B)
    e.load_state_dict(weights.make_state_dict(spec, seed=0))
    return e


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cl_head.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cl_head_bench: no GPU visible; this tool measures, it has no CPU form")
    batch = synth.make_pretrain_batch(B=B, S=S, F=F, V=V, seed=1234)
    n_tok = int(batch["attention_mask"].sum())
    dev = {k: torch.from_numpy(v).cuda() for k, v in batch.items() if k != "lengths"}
    engines = {"pretrain": make_engine(spec_mod.KIND_PRETRAIN, batch), "pretrain_cl": make_engine(spec_mod.KIND_PRETRAIN_CL, batch)}

    def steps(e, n):
        for _ in range(n):
            e.set_dropout(0.1, 0.0, 7)
            e.forward_pretrain(dev["input_ids"], dev["attention_mask"], dev["labels"], num_tokens=n_tok)
            e.backward()
            e.adamw_step(3e-4)

    def timed(e, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(e, n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for e in engines.values():
        steps(e, 5)
    rounds = {k: [] for k in engines}
    for r in range(a.rounds):
        for k, e in engines.items():      # alternated: both kinds see the same state of the box
            rounds[k].append(timed(e, a.steps))
        print(f"round {r}: " + "  ".join(f"{k} {rounds[k][-1]:.3f} ms/step" for k in engines), flush=True)

    # the three operator-level launches alone, on the operands of this step ([256, 768]; hidden [B S, 768])
    d = 768
    g = torch.Generator().manual_seed(3)
    hidden = torch.randn(B * S, d, generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn(d, d, generator=g) * d ** -0.5).to(torch.bfloat16).cuda()
    pool = (torch.arange(B, dtype=torch.int32) * S + torch.randint(8, S, (B,), generator=g, dtype=torch.int32)).cuda()
    z, e_, rn = torch.empty(B, d, device="cuda"), torch.empty(B, d, device="cuda"), torch.empty(B, device="cuda")
    stat, loss = torch.empty(3, B, device="cuda"), torch.empty(1, device="cuda")
    dz, dw, dh = torch.empty(B, d, device="cuda"), torch.zeros(d, d, device="cuda"), torch.zeros(B * S, d, dtype=torch.bfloat16, device="cuda")
    lib = L.load()
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ops = {
        "cl_embed_fwd": lambda: L.check(lib.gget_op_cl_embed_fwd(P(hidden), P(pool), P(w), P(z), P(e_), P(rn), B, d, st)),
        "cl_loss_fwd": lambda: L.check(lib.gget_op_cl_loss_fwd(P(e_), B, d, 0.5, P(stat), P(loss), st)),
        "cl_bwd": lambda: L.check(lib.gget_op_cl_bwd(P(e_), P(stat), None, P(rn), P(hidden), P(pool), P(w), 0.5, P(dz), P(dw), P(dh), B, B,
                                                     d, st)),
    }
    op_us = {}
    for name, fn in ops.items():
        for _ in range(10):
            fn()
        per = []
        for _ in range(a.rounds):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(200):
                fn()
            t1.record()
            torch.cuda.synchronize()
            per.append(t0.elapsed_time(t1) / 200 * 1e3)
        op_us[name] = median(per)
        print(f"{name}: {op_us[name]:.1f} us per call (median of {a.rounds} x 200 back-to-back calls, launches included)", flush=True)

    res = {"workload": dict(model="base", B=B, S=S, F=F, V=V, real_tokens=n_tok, attention_dropout=0.1, steps_per_round=a.steps, rounds=a.rounds),
           "step_ms": {k: dict(median=median(v), rounds=v) for k, v in rounds.items()},
           "step_ms_delta_median": median(rounds["pretrain_cl"]) - median(rounds["pretrain"]),
           "op_us": op_us, "device": torch.cuda.get_device_name(0),
           # (the runtime's marketing name can be a generic one; the architecture and the CU count say which card it was)
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "compute_units": torch.cuda.get_device_properties(0).multi_processor_count}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res["step_ms_delta_median"]), "ms/step added by the contrastive head ->", a.out)


if __name__ == "__main__":
    main()
