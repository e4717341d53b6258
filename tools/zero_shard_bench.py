"""Rank 0's sharded optimizer pass (ZeRO stage 2: chunk partials of the norm, the one-block sum of the gathered partials, AdamW over the
rank's segments - no collectives) against the replicated pass (gget_adamw_step: full norm + AdamW over every parameter) on the base model,
for W = 1, 2, 4, 8, timed with HIP events in the same process, the two alternated.  Writes profiles/zero_shard_optimizer_pass.json.

    python tools/zero_shard_bench.py [--iters 50] [--out profiles/zero_shard_optimizer_pass.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--worlds", default="1,2,4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zero_shard_optimizer_pass.json"))
    a = ap.parse_args()
    importlib.import_module("graph-gpt_amd.build").build()
    eng_mod = importlib.import_module("graph-gpt_amd.engine")
    spec = importlib.import_module("graph-gpt_amd.spec").spec_from_size("base", vocab_size=756, stacked_feat=13, next_n_token=13)
    torch.cuda.set_device(0)
    rep = eng_mod.Engine(spec, max_tokens=1024, max_batch=8)
    sh = eng_mod.Engine(spec, max_tokens=1024, max_batch=8)
    gen = torch.Generator(device="cuda").manual_seed(0)
    for e in (rep, sh):
        e.master.copy_(torch.randn(e.n_params, generator=gen, device="cuda") * 0.02)
        e.grad_bf16.copy_((torch.randn(e.n_params, generator=gen, device="cuda") * 1e-3).to(torch.bfloat16))
    torch.cuda.synchronize()

    def timed(fn):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        t.record()
        t.synchronize()
        return s.elapsed_time(t)

    def rep_pass():
        rep.step_count = 0
        rep.adamw_step(1e-4, max_grad_norm=1.0)

    rows = []
    for W in [int(x) for x in a.worlds.split(",")]:
        sh.shard_init(W, 0)

        def sh_pass():
            sh.step_count = 0
            sh.shard_sqnorm_partials()
            sh.adamw_step_sharded(1e-4, max_grad_norm=1.0)

        for _ in range(5):
            rep_pass()
            sh_pass()
        tr, ts = [], []
        for _ in range(a.iters):      # alternated: the two passes see the same clocks and the same memory-side cache state
            tr.append(timed(rep_pass))
            ts.append(timed(sh_pass))
        owned = sum(p[2] for p in sh.shard_buckets) + sum(p[4] for p in sh.shard_buckets)
        r = dict(world=W, replicated_us=round(statistics.median(tr) * 1e3, 1), sharded_us=round(statistics.median(ts) * 1e3, 1),
                 owned_elements=owned, n_params=sh.n_params)
        r["ratio"] = round(r["sharded_us"] / r["replicated_us"], 4)
        rows.append(r)
        print(json.dumps(r), flush=True)
    res = {"what": "rank 0's optimizer pass, base model, median of alternated HIP-event timings (includes launch gaps of 2 launches "
                   "replicated / 2 launches sharded)", "device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows,
           "done_when": "W=8 ratio <= 0.2", "w8_ok": any(r["world"] == 8 and r["ratio"] <= 0.2 for r in rows)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"w8_ok": res["w8_ok"]}))


if __name__ == "__main__":
    main()
