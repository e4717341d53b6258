"""What parameter groups cost in the optimizer launch, base pre-train model (122 M parameters), HIP events around the launches, the
variants alternated in one process on one box:

  ungrouped        gget_adamw_step with no scale table: the grid-stride launch, as before the feature existed - compared with the same
                   launch of ANOTHER build of the library (--parent-lib: the parent commit's libgget_hip.so) bound to the SAME arenas;
                   the claim is "the same launch", so the margin is two handles of the parent library on those arenas against each
                   other, recorded next to it.  Where the allocator put the arenas moves the launch by several per cent and so does
                   what ran in front of it: there are two sets of arenas (A, B), every variant runs on both, and every round runs the
                   variants in a fresh random order
  grouped          gget_adamw_step with the layer-wise lr decay v1 table (0.5) and weight-decay scale 0 on 1-D parameters: the whole
                   arena as work items of <= 2048 elements cut at the group boundaries
  grouped_sharded  the same table under a world-1 shard plan (gget_adamw_step_sharded): the plan's items cut at the same boundaries

No norm pass is timed (max_grad_norm = 0, no gnorm pointer): the figures are the AdamW launch alone, 28 B per parameter.  The grouped
figures are reported, not gated.  Writes profiles/param_groups.json.

    python tools/param_groups_bench.py [--iters 200] [--parent-lib path/to/parent/libgget_hip.so] [--out profiles/param_groups.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


class Arenas:
    """One set of flat arenas (base model: 2 GB); several handles, of any build of the library, may be bound to it - only one runs at a time"""

    def __init__(self, n, ws_bytes, gen):
        dev = "cuda"
        self.P = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        self.G = (torch.randn(n, generator=gen, device=dev) * 1e-3).to(torch.bfloat16)
        self.master = torch.randn(n, generator=gen, device=dev) * 0.02
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)


class RawHandle:
    """A handle of `lib` (any build of the library) over a set of arenas; only what the AdamW launch needs."""

    def __init__(self, lib, L, cfg, a):
        self.lib, self.arenas = lib, a
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        bufs = L.GgetBuffers(p(a.P), p(a.master), p(a.m), p(a.v), p(a.G), p(a.ws), None, None)
        self.h = C.c_void_p()
        torch.cuda.synchronize()
        rc = lib.gget_create(C.byref(cfg), C.byref(bufs), C.byref(self.h))
        assert rc == 0, lib.gget_last_error()

    def set_scales(self, lr, wd):
        fp = C.POINTER(C.c_float)
        rc = self.lib.gget_set_param_scales(self.h, lr.ctypes.data_as(fp), wd.ctypes.data_as(fp), len(lr))
        assert rc == 0, self.lib.gget_last_error()

    def shard(self):
        assert self.lib.gget_shard_init(self.h, 1, 0, None) == 0, self.lib.gget_last_error()

    def adamw(self, st):
        rc = self.lib.gget_adamw_step(self.h, 1e-4, 0.9, 0.95, 1e-8, 0.1, 0.0, 1.0, 1, None, st)
        assert rc == 0, self.lib.gget_last_error()

    def adamw_sharded(self, st):
        rc = self.lib.gget_adamw_step_sharded(self.h, 1e-4, 0.9, 0.95, 1e-8, 0.1, 0.0, 1.0, 1, None, None, st)
        assert rc == 0, self.lib.gget_last_error()


def bind(lib, L, names):
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_groups.json"))
    a = ap.parse_args()
    importlib.import_module("graph-gpt_amd.build").build()
    import numpy as np
    L = importlib.import_module("graph-gpt_amd._lib")
    eng_mod = importlib.import_module("graph-gpt_amd.engine")
    T = importlib.import_module("graph-gpt_amd.training")
    spec = importlib.import_module("graph-gpt_amd.spec").spec_from_size("base", vocab_size=756, stacked_feat=13, next_n_token=13)
    torch.cuda.set_device(0)
    probe = eng_mod.Engine(spec, max_tokens=1024, max_batch=8)      # (configuration + sizes from the package's own path)
    cfg, n, ws_bytes = probe.cfg, probe.n_params, probe.workspace_bytes
    depth = T.layerwise_depths(probe.params, spec.num_layers, 1, True)
    lr = np.array([0.5 ** depth[k] for k in probe.params], dtype=np.float32)
    wd = np.array([0.0 if len(p["shape"]) == 1 else 1.0 for p in probe.params.values()], dtype=np.float32)
    items = {"grouped": len(eng_mod.Engine.group_plan_of(cfg, lr, wd, -1, 0, -1)),
             "grouped_sharded": len(eng_mod.Engine.group_plan_of(cfg, lr, wd, -1, 1, 0))}
    del probe
    gen = torch.Generator(device="cuda").manual_seed(0)
    lib = L.load()
    core = ("gget_last_error", "gget_create", "gget_adamw_step")
    parent = bind(C.CDLL(os.path.abspath(a.parent_lib)), L, core) if a.parent_lib else None
    # Where the allocator put a handle's arenas moves the launch by several per cent (two handles of ONE library differed by 8 %), so
    # every variant runs on the SAME arenas: two sets, A and B, and on each set handles of both libraries.  parent_X / parent_X_2 are
    # two handles of the parent library on one set - the margin of a comparison on equal arenas.
    handles = {}
    for tag in ("A", "B"):
        ar = Arenas(n, ws_bytes, gen)
        if parent is not None:
            handles[f"parent_{tag}"] = RawHandle(parent, L, cfg, ar)
            handles[f"parent_{tag}_2"] = RawHandle(parent, L, cfg, ar)
        for k in ("ungrouped", "grouped", "grouped_sharded"):
            handles[f"{k}_{tag}"] = RawHandle(lib, L, cfg, ar)
        handles[f"grouped_{tag}"].set_scales(lr, wd)
        handles[f"grouped_sharded_{tag}"].shard()
        handles[f"grouped_sharded_{tag}"].set_scales(lr, wd)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    variants = {k: ((lambda h=h: h.adamw_sharded(st)) if k.startswith("grouped_sharded") else (lambda h=h: h.adamw(st))) for k, h in handles.items()}

    def timed(fn):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        t.record()
        t.synchronize()
        return s.elapsed_time(t)

    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    times = {k: [] for k in variants}
    order, rng = list(variants), random.Random(0)
    for it in range(a.iters):         # alternated, every round in a fresh random order: no variant keeps its predecessor
        rng.shuffle(order)
        for k in order:
            times[k].append(timed(variants[k]))
    us = {k: statistics.median(v) * 1e3 for k, v in times.items()}
    rows = {k: dict(median_us=round(us[k], 2), min_us=round(min(times[k]) * 1e3, 2), TBps=round(28 * n / (us[k] * 1e-6) / 1e12, 3),
                    **({"items": items[k[:-2]]} if k[:-2] in items else {})) for k in times}
    ratio = lambda x, y: round(us[x] / us[y], 4)      # noqa: E731
    res = {"what": "the AdamW launch of the base model (no norm pass, 28 B per parameter), median of HIP-event timings, every round in a "
                   "fresh random order; _A / _B = the set of arenas the handle is bound to (all variants of a set run on the same memory); "
                   "ungrouped = gget_adamw_step with no scale table (the grid-stride launch), grouped = with the layer-wise v1 table "
                   "(0.5) and weight-decay scale 0 on 1-D parameters (work items over the whole arena), grouped_sharded = the same "
                   "table under a world-1 shard plan, parent_X / parent_X_2 = two handles of the parent commit's library",
           "device": torch.cuda.get_device_name(0), "iters": a.iters, "n_params": n, "distinct_lr_scales": len(set(lr.tolist())), "rows": rows,
           "grouped_over_ungrouped": {t: ratio(f"grouped_{t}", f"ungrouped_{t}") for t in "AB"},
           "grouped_sharded_over_ungrouped": {t: ratio(f"grouped_sharded_{t}", f"ungrouped_{t}") for t in "AB"},
           "arenas_B_over_A_ungrouped": ratio("ungrouped_B", "ungrouped_A")}
    if parent is not None:
        res["ungrouped_over_parent"] = {t: ratio(f"ungrouped_{t}", f"parent_{t}") for t in "AB"}
        res["parent_2_over_parent"] = {t: ratio(f"parent_{t}_2", f"parent_{t}") for t in "AB"}      # the margin: one build against itself
    print(json.dumps(res, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
