"""What the weight EMA costs in the optimizer launch, base model arenas, HIP events around the launches, the variants alternated in one
process:

  (a)  gget_adamw_step without EMA on this build against the same launch of ANOTHER build of the library (--parent-lib: the parent
       commit's libgget_hip.so) - the claim is "unchanged", so the margin is the spread of two handles of the parent library against
       each other, recorded next to it;
  (b)  the fused step (gget_set_ema_decay + gget_adamw_step: 36 B per parameter);
  (c)  the plain step followed by gget_ema_update (28 + 12 B per parameter, two launches).

No norm pass is timed (max_grad_norm = 0, no gnorm pointer): the figures are the AdamW launch alone.  Writes profiles/ema_update.json.

    python tools/ema_bench.py [--iters 200] [--parent-lib path/to/parent/libgget_hip.so] [--out profiles/ema_update.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


class RawHandle:
    """A handle of `lib` (any build of the library) over arenas of its own; only what the AdamW launch needs."""

    def __init__(self, lib, L, cfg, n, ws_bytes, gen):
        dev = "cuda"
        self.lib, self.n = lib, n
        self.P = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        self.G = (torch.randn(n, generator=gen, device=dev) * 1e-3).to(torch.bfloat16)
        self.master = torch.randn(n, generator=gen, device=dev) * 0.02
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
        self.ema = None
        p = lambda t: C.c_void_p(t.data_ptr())
        bufs = L.GgetBuffers(p(self.P), p(self.master), p(self.m), p(self.v), p(self.G), p(self.ws), None, None)
        self.h = C.c_void_p()
        torch.cuda.synchronize()
        rc = lib.gget_create(C.byref(cfg), C.byref(bufs), C.byref(self.h))
        assert rc == 0, lib.gget_last_error()

    def attach_ema(self):
        self.ema = self.master.clone()
        torch.cuda.synchronize()
        assert self.lib.gget_ema_attach(self.h, C.c_void_p(self.ema.data_ptr())) == 0

    def adamw(self, st, ema_decay=None):
        if ema_decay is not None:
            assert self.lib.gget_set_ema_decay(self.h, ema_decay) == 0
        rc = self.lib.gget_adamw_step(self.h, 1e-4, 0.9, 0.95, 1e-8, 0.1, 0.0, 1.0, 1, None, st)
        assert rc == 0, self.lib.gget_last_error()

    def ema_update(self, st, d):
        assert self.lib.gget_ema_update(self.h, d, st) == 0


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_update.json"))
    a = ap.parse_args()
    importlib.import_module("graph-gpt_amd.build").build()
    L = importlib.import_module("graph-gpt_amd._lib")
    eng_mod = importlib.import_module("graph-gpt_amd.engine")
    spec = importlib.import_module("graph-gpt_amd.spec").spec_from_size("base", vocab_size=756, stacked_feat=13, next_n_token=13)
    torch.cuda.set_device(0)
    probe = eng_mod.Engine(spec, max_tokens=1024, max_batch=8)      # (configuration + sizes from the package's own path)
    cfg, n, ws_bytes = probe.cfg, probe.n_params, probe.workspace_bytes
    gen = torch.Generator(device="cuda").manual_seed(0)
    lib = L.load()
    core = ("gget_last_error", "gget_create", "gget_adamw_step")
    handles = {"plain": RawHandle(lib, L, cfg, n, ws_bytes, gen), "fused": RawHandle(lib, L, cfg, n, ws_bytes, gen),
               "separate": RawHandle(lib, L, cfg, n, ws_bytes, gen)}
    handles["fused"].attach_ema()
    handles["separate"].attach_ema()
    if a.parent_lib:
        parent = bind(C.CDLL(os.path.abspath(a.parent_lib)), L, core)
        handles["parent_1"] = RawHandle(parent, L, cfg, n, ws_bytes, gen)
        handles["parent_2"] = RawHandle(parent, L, cfg, n, ws_bytes, gen)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d = 0.9999

    def separate():
        handles["separate"].adamw(st)
        handles["separate"].ema_update(st, d)

    variants = {}
    if "parent_1" in handles:
        variants["parent_1"] = lambda: handles["parent_1"].adamw(st)
    variants["plain"] = lambda: handles["plain"].adamw(st)
    if "parent_2" in handles:
        variants["parent_2"] = lambda: handles["parent_2"].adamw(st)
    variants.update(fused=lambda: handles["fused"].adamw(st, d), separate=separate)

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
    order = list(variants)
    for it in range(a.iters):         # alternated, and the round's order rotated: a launch's time depends on what ran in front of it (the
        for j in range(len(order)):   # one behind the 40-byte `separate` form is the slow one), so every variant takes every position
            k = order[(it + j) % len(order)]
            times[k].append(timed(variants[k]))
    us = {k: statistics.median(v) * 1e3 for k, v in times.items()}
    bytes_per_param = {"plain": 28, "fused": 36, "separate": 40, "parent_1": 28, "parent_2": 28}
    rows = {k: dict(median_us=round(us[k], 2), min_us=round(min(times[k]) * 1e3, 2), bytes_per_param=bytes_per_param[k],
                    TBps=round(bytes_per_param[k] * n / (us[k] * 1e-6) / 1e12, 3)) for k in us}
    res = {"what": "the AdamW launch of the base model (no norm pass), median of alternated HIP-event timings; plain = gget_adamw_step "
                   "without EMA, fused = with gget_set_ema_decay, separate = plain + gget_ema_update (two launches), parent_1 / parent_2 = "
                   "two handles of the parent commit's library",
           "device": torch.cuda.get_device_name(0), "iters": a.iters, "n_params": n, "decay": d, "rows": rows,
           "fused_over_plain": round(us["fused"] / us["plain"], 4), "bytes_predict_fused_over_plain": round(36 / 28, 4),
           "fused_over_separate": round(us["fused"] / us["separate"], 4), "fused_kept": us["fused"] < us["separate"]}
    if "parent_1" in us:
        res["plain_over_parent_1"] = round(us["plain"] / us["parent_1"], 4)
        res["plain_over_parent_2"] = round(us["plain"] / us["parent_2"], 4)
        res["parent_2_over_parent_1"] = round(us["parent_2"] / us["parent_1"], 4)      # the margin: one build against itself
    print(json.dumps(res, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
