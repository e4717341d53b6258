#!/usr/bin/env python3
"""Time of one inference pass (`inference.ft_infer_hidden_states` with hidden states, then the host copy of its three results) with the
device-resident collection (one gget_op_infer_append launch per batch into arenas sized from the dataset) against the reference's
statement on the same engine (per batch `.half()` of logits and hidden states into Python lists, `vstack` at the end, then the same
host copy), next to the forwards alone.

Base task model (d768 / L12), B 256, S 32, F 13, V 756, 128 labels, 64 batches (eight distinct device-resident batches in turn).  The
two paths alternate in one process (other people's work shares the host: a drift hits both); each pass is timed by the host clock
around work that ends in the host copy, after both paths have been warmed up; the results of the two paths are compared for equality.
No threshold is attached.  Writes profiles/infer_pass.json.

    python tools/infer_pass_bench.py [--batches 64] [--repeats 7] [--warmup 2] [--out profiles/infer_pass.json]
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
L = importlib.import_module("graph-gpt_amd._lib")
inf = importlib.import_module("graph-gpt_amd.inference")
modeling = importlib.import_module("graph-gpt_amd.modeling")
synth = importlib.import_module("graph-gpt_amd.synth")


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


class Loader(list):
    def __init__(self, batches, n_samples):
        super().__init__(batches)
        self.dataset = range(n_samples)


@torch.no_grad()
def reference_pass(model, loader):
    """log_eval_dump_utils.py:41-74 as written there"""
    model.eval()
    ls_idx, ls_logits, ls_states = [], [], []
    for d in loader:
        res = model(input_ids=d["input_ids"], attention_mask=d["attention_mask"], position_ids=d["position_ids"])
        ls_idx.append(d["idx"].view((-1, 1)))
        ls_logits.append(res.task_logits.half())
        ls_states.append(res.task_hidden_states.half())
    return torch.vstack(ls_idx), torch.vstack(ls_logits), torch.vstack(ls_states)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--S", type=int, default=32)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--labels", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=12, help="12 = the base model; fewer is a rehearsal (the file says so)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer_pass.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("infer_pass_bench: no GPU visible (a time taken without one says nothing)")
    F, V = 13, 756
    cfg = modeling.GraphGPTConfig(hidden_act="gelu", vocab_size=V, hidden_size=768, intermediate_size=3072, num_hidden_layers=a.layers,
                                  num_attention_heads=12, max_position_embeddings=1024, causal_attention=False, stacked_feat=F,
                                  next_n_token=1, num_labels=a.labels, problem_type="multi_label_classification")
    model = modeling.GraphGPTTaskModel(cfg, seed=0).cuda()
    distinct = []
    for k in range(8):
        b = synth.make_task_batch(B=a.B, S=a.S, F=F, V=V, seed=11 + k, num_labels=a.labels, multi_label=True)
        distinct.append({n: torch.from_numpy(v).cuda() for n, v in b.items() if n not in ("lengths", "task_labels")})
    loader = Loader([dict(distinct[k % 8], idx=torch.arange(a.B, device="cuda") + k * a.B) for k in range(a.batches)], a.B * a.batches)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = tuple(t.cpu() for t in fn())
        return out, (time.perf_counter() - t0) * 1e3

    device_pass = lambda: inf.ft_infer_hidden_states(model, loader, save_hidden_states=True)      # noqa: E731
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):         # (the comparison only: two forwards of a batch then give the same bits)
        got, _ = timed(device_pass)
        want, _ = timed(lambda: reference_pass(model, loader))
    equal = all(torch.equal(g.view(torch.int16) if g.dtype == torch.float16 else g, w.view(torch.int16) if w.dtype == torch.float16 else w)
                for g, w in zip(got, want))
    for _ in range(a.warmup):
        timed(device_pass), timed(lambda: reference_pass(model, loader))
    t_dev, t_ref = [], []
    for _ in range(a.repeats):                         # alternate: device, reference, device, reference, ...
        t_dev.append(timed(device_pass)[1])
        t_ref.append(timed(lambda: reference_pass(model, loader))[1])
    fwd = []
    model.eval()
    with torch.no_grad():
        for k in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for d in loader:
                model(input_ids=d["input_ids"], attention_mask=d["attention_mask"], position_ids=d["position_ids"])
            torch.cuda.synchronize()
            if k >= a.warmup:
                fwd.append((time.perf_counter() - t0) * 1e3)
    res = {"what": "one inference pass with hidden states over device-resident batches, host clock from the first forward to the end of "
                   "the host copy of (idx, logits fp16, hidden fp16); device collection = gget_op_infer_append into arenas sized from the "
                   "dataset, reference statement = per-batch .half() + vstack (log_eval_dump_utils.py:41-74); the two alternate in one "
                   "process; forwards alone = the same forwards back to back, no collection, no copy",
           "device": torch.cuda.get_device_name(0), "model": {"hidden": 768, "layers": a.layers, "rehearsal": a.layers != 12},
           "B": a.B, "S": a.S, "F": F, "V": V, "labels": a.labels, "batches": a.batches, "samples": a.B * a.batches,
           "results_equal": bool(equal),
           "ms_per_pass": {"device_collection": stats(t_dev), "reference_statement": stats(t_ref), "forwards_alone": stats(fwd)},
           "collection_and_copy_ms_per_pass": {"device_collection": round(statistics.median(t_dev) - statistics.median(fwd), 4),
                                               "reference_statement": round(statistics.median(t_ref) - statistics.median(fwd), 4)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if not equal:
        raise SystemExit("infer_pass_bench: the two paths gave different results")


if __name__ == "__main__":
    main()
