#!/usr/bin/env python3
"""Time per iteration of `generation.sample_per_batch` with the update on the device (gget_op_gen_plan + gget_op_unmask_ranked, one
8-byte host read per iteration) and with the torch statement of the same rule (GGET_GEN_DEVICE=0: reveal_counts + unmask_step, two
.item() reads per pass of the skip loop, a full sort), next to the forward's own time.

Base model (d768 / L12), B 256, S 32, F 13, V 756, alg maskgit_plus, all iterations of one call.  The two paths alternate in one
process (other people's work shares the host: a drift hits both), each call is timed by the host clock around work that ends in a
device synchronise, after both paths have been warmed up; the tokens of the two paths are compared.  No threshold is attached
here: the requirement is only that the device path is not the slower one.  Writes profiles/gen_eval_loop.json.

    python tools/gen_loop_bench.py [--steps 64] [--repeats 7] [--warmup 2] [--out profiles/gen_eval_loop.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gen = importlib.import_module("graph-gpt_amd.generation")
modeling = importlib.import_module("graph-gpt_amd.modeling")
synth = importlib.import_module("graph-gpt_amd.synth")


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--S", type=int, default=32)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=12, help="12 = the base model; fewer is a rehearsal (the file says so)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_eval_loop.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gen_loop_bench: no GPU visible (a time taken without one says nothing)")
    F, V = 13, 756
    cfg = modeling.GraphGPTConfig(hidden_act="gelu", vocab_size=V, hidden_size=768, intermediate_size=3072, num_hidden_layers=a.layers,
                                  num_attention_heads=12, max_position_embeddings=1024, causal_attention=False, stacked_feat=F,
                                  next_n_token=F)
    model = modeling.GraphGPTPretrainBase(cfg, seed=0).cuda()
    batch = synth.make_pretrain_batch(B=a.B, S=a.S, F=F, V=V, seed=3)
    ids, att = torch.from_numpy(batch["input_ids"]).cuda(), torch.from_numpy(batch["attention_mask"]).cuda()
    n_masked = (ids.view(a.B, -1) == 1).sum(dim=1)

    def call(device_path, history=False):
        os.environ["GGET_GEN_DEVICE"] = "1" if device_path else "0"
        gcfg = gen.GenerationConfig(alg="maskgit_plus", steps=a.steps, eps=1e-3, mask_token_id=1, output_history=history)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, hist = gen.sample_per_batch(model, gcfg, input_ids=ids, attention_mask=att)
        torch.cuda.synchronize()
        return x, hist, (time.perf_counter() - t0) * 1e3

    x_dev, h_dev, _ = call(True, history=True)
    x_ref, h_ref, _ = call(False, history=True)
    iters = len(h_dev)
    equal = len(h_ref) == iters and torch.equal(x_dev, x_ref) and all(torch.equal(p, q) for p, q in zip(h_dev, h_ref))
    for _ in range(a.warmup):
        call(True), call(False)
    t_dev, t_ref = [], []
    for _ in range(a.repeats):                         # alternate: device, torch, device, torch, ...
        t_dev.append(call(True)[2] / iters)
        t_ref.append(call(False)[2] / iters)
    model.eval()
    fwd = []
    with torch.no_grad():
        for k in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                model(input_ids=ids, attention_mask=att, labels=None)
            torch.cuda.synchronize()
            if k >= a.warmup:
                fwd.append((time.perf_counter() - t0) * 1e3 / iters)
    res = {"what": "sample_per_batch, alg maskgit_plus: host clock around one whole call (ends in a device synchronise) / iterations of the "
                   "call; device path = gget_op_gen_plan + gget_op_unmask_ranked, torch path = GGET_GEN_DEVICE=0 (reveal_counts + "
                   "unmask_step); the two alternate in one process; forward = the labels=None forward alone, back to back",
           "device": torch.cuda.get_device_name(0), "model": {"hidden": 768, "layers": a.layers, "rehearsal": a.layers != 12},
           "B": a.B, "S": a.S, "F": F, "V": V, "steps": a.steps, "iterations_per_call": iters,
           "masked_cells_per_sample": {"min": int(n_masked.min()), "max": int(n_masked.max())},
           "tokens_and_history_equal": bool(equal),
           "ms_per_iteration": {"device_path": stats(t_dev), "torch_path": stats(t_ref), "forward_alone": stats(fwd)},
           "sampling_kernel_plus_update_ms_per_iteration": {"device_path": round(statistics.median(t_dev) - statistics.median(fwd), 4),
                                                    "torch_path": round(statistics.median(t_ref) - statistics.median(fwd), 4)},
           "device_path_not_slower": bool(statistics.median(t_dev) <= statistics.median(t_ref))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if not equal:
        raise SystemExit("gen_loop_bench: the two paths gave different tokens")


if __name__ == "__main__":
    main()
