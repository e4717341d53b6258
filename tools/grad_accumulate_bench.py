"""What gradient accumulation costs around the optimizer step, base model arenas, HIP events around the launches, the variants
alternated in one process:

  new     gget_grad_accumulate on the first micro-step of a window (6 B per parameter: the arena is overwritten) and on a later one
          (10 B), and the boundary step - norm pass + AdamW - reading the fp32 accumulator (4 + 30 B);
  parent  what GgetEngine.step did before the accumulator lived in the engine: `acc += grad_bf16` in torch per micro-step (10 B), and at
          the boundary `grad_bf16.copy_(acc)` (6 B), `acc.zero_()` (4 B), then the norm pass + AdamW on the bf16 array (2 + 28 B).

The window totals are formed for k = 2 and k = 4 micro-steps from the medians.  Writes profiles/grad_accumulate.json.

    python tools/grad_accumulate_bench.py [--iters 100] [--out profiles/grad_accumulate.json]
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
    """A handle over arenas of its own; only what the accumulate and AdamW launches need."""

    def __init__(self, lib, L, cfg, n, ws_bytes, gen):
        dev = "cuda"
        self.lib, self.n = lib, n
        self.P = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        self.G = (torch.randn(n, generator=gen, device=dev) * 1e-3).to(torch.bfloat16)
        self.master = torch.randn(n, generator=gen, device=dev) * 0.02
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
        self.acc = torch.zeros(n, dtype=torch.float32, device=dev)
        self.gnorm = torch.zeros(1, dtype=torch.float32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        bufs = L.GgetBuffers(p(self.P), p(self.master), p(self.m), p(self.v), p(self.G), p(self.ws), None, None)
        self.h = C.c_void_p()
        torch.cuda.synchronize()
        self.check(lib.gget_create(C.byref(cfg), C.byref(bufs), C.byref(self.h)))

    def check(self, rc):
        assert rc == 0, self.lib.gget_last_error()

    def attach(self):
        self.check(self.lib.gget_grad_acc_attach(self.h, C.c_void_p(self.acc.data_ptr())))

    def accumulate(self, st, first):
        self.check(self.lib.gget_grad_acc_set_count(self.h, 0 if first else 1))
        self.check(self.lib.gget_grad_accumulate(self.h, st))

    def adamw(self, st, window, scale):
        """norm pass + clip + AdamW; window = micro-steps of the open window the step reads (0: the bf16 gradient array)"""
        self.check(self.lib.gget_grad_acc_set_count(self.h, window))
        self.check(self.lib.gget_adamw_step(self.h, 1e-4, 0.9, 0.95, 1e-8, 0.1, 1.0, scale, 1, C.c_void_p(self.gnorm.data_ptr()), st))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accumulate.json"))
    a = ap.parse_args()
    importlib.import_module("graph-gpt_amd.build").build()
    L = importlib.import_module("graph-gpt_amd._lib")
    eng_mod = importlib.import_module("graph-gpt_amd.engine")
    spec = importlib.import_module("graph-gpt_amd.spec").spec_from_size("base", vocab_size=756, stacked_feat=13, next_n_token=13)
    torch.cuda.set_device(0)
    probe = eng_mod.Engine(spec, max_tokens=1024, max_batch=8)      # (configuration + sizes from the package's own path)
    cfg, n, ws_bytes = probe.cfg, probe.n_params, probe.workspace_bytes
    del probe
    gen = torch.Generator(device="cuda").manual_seed(0)
    lib = L.load()
    new, old = RawHandle(lib, L, cfg, n, ws_bytes, gen), RawHandle(lib, L, cfg, n, ws_bytes, gen)
    new.attach()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def parent_micro():
        old.acc += old.G

    def parent_boundary():
        old.G.copy_(old.acc)
        old.acc.zero_()
        old.adamw(st, 0, 0.5)

    variants = {"new_first": lambda: new.accumulate(st, True), "parent_micro": parent_micro,
                "new_later": lambda: new.accumulate(st, False), "parent_boundary": parent_boundary,
                "new_boundary": lambda: new.adamw(st, 2, 0.5), "bf16_step": lambda: old.adamw(st, 0, 1.0)}

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
    for it in range(a.iters):         # alternated, and the round's order rotated: every variant takes every position
        for j in range(len(order)):
            k = order[(it + j) % len(order)]
            times[k].append(timed(variants[k]))
    us = {k: statistics.median(v) * 1e3 for k, v in times.items()}
    bytes_per_param = {"new_first": 6, "new_later": 10, "new_boundary": 34, "parent_micro": 10, "parent_boundary": 40, "bf16_step": 30}
    rows = {k: dict(median_us=round(us[k], 2), min_us=round(min(times[k]) * 1e3, 2), bytes_per_param=bytes_per_param[k],
                    TBps=round(bytes_per_param[k] * n / (us[k] * 1e-6) / 1e12, 3)) for k in us}
    window = {}
    for k in (2, 4):
        t_new = us["new_first"] + (k - 1) * us["new_later"] + us["new_boundary"]
        t_old = k * us["parent_micro"] + us["parent_boundary"]
        window[f"k{k}"] = dict(new_us=round(t_new, 2), parent_us=round(t_old, 2), new_over_parent=round(t_new / t_old, 4),
                               bytes_predict=round((6 + 10 * (k - 1) + 34) / (10 * k + 40), 4))
    res = {"what": "gradient accumulation around the optimizer step of the base model, median of alternated HIP-event timings; new_first / "
                   "new_later = gget_grad_accumulate on the first / a later micro-step of a window, new_boundary = norm pass + AdamW reading "
                   "the fp32 accumulator; parent_micro = torch `acc += grad_bf16`, parent_boundary = torch copy_ + zero_ and the norm pass + "
                   "AdamW on the bf16 array; bf16_step = norm pass + AdamW on the bf16 array alone (the k = 1 step).  window: accumulation "
                   "+ boundary of one update of k micro-steps",
           "device": torch.cuda.get_device_name(0), "iters": a.iters, "n_params": n, "rows": rows, "window": window,
           "not_slower_than_parent": all(w["new_over_parent"] <= 1.0 for w in window.values())}
    print(json.dumps(res, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
