#!/usr/bin/env python3
"""What does a collective's kernel cost the exact-fit GEMM launches when it shares the chip?
One GPU: the C1 training step runs on the compute stream while a stand-in kernel (gget_debug_occupy: N workgroups of 256
threads with a given LDS footprint, resident for the whole backward, streaming a little memory) sits on a side stream, the way
RCCL's ring kernels would during the overlapped bucketed all-reduce.  Reports ms/step for N = 0 .. 64 and two LDS sizes."""
import ctypes as C, importlib, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
L = importlib.import_module("graph-gpt_amd._lib")
modeling = importlib.import_module("graph-gpt_amd.modeling")
training = importlib.import_module("graph-gpt_amd.training")
synth = importlib.import_module("graph-gpt_amd.synth")
spec_mod = importlib.import_module("graph-gpt_amd.spec")
lib = L.load()
headroom0 = L.debug_get(L.KEY_GEMM_LDS_HEADROOM)   # (restored at the end)
B, S, F, V = 256, 32, 13, 756
sz = spec_mod.MODEL_SIZES["base"]
cfg = modeling.GraphGPTConfig(hidden_act="gelu", vocab_size=V, hidden_size=sz["hidden_size"], intermediate_size=4 * sz["hidden_size"],
                              num_hidden_layers=sz["num_layers"], num_attention_heads=sz["hidden_size"] // 64,
                              max_position_embeddings=1024, causal_attention=False, stacked_feat=F, next_n_token=F, attention_dropout=0.1)
model = modeling.GraphGPTPretrainBase(cfg, seed=0)
model._ensure_engine(B, S)
eng = training.initialize(model, training.OptimConfig(lr=3e-4))
batch = synth.make_pretrain_batch(B=B, S=S, F=F, V=V, seed=1234)
dev = {k: torch.from_numpy(v).cuda() for k, v in batch.items() if k != "lengths"}
side = torch.cuda.Stream()
scratch = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
rows = []


def run(blocks, lds, steps=12, warm=3):
    def step():
        if blocks:
            ev = torch.cuda.Event(); ev.record()
            side.wait_event(ev)
            # resident for ~the whole step (9 ms): what an all-reduce of the layer buckets spread over the backward looks like
            L.check(lib.gget_debug_occupy(C.c_void_p(scratch.data_ptr()), scratch.numel(), blocks, lds, 9000, C.c_void_p(side.cuda_stream)))
        out = training.batch_training(dev, eng)
        if blocks:
            torch.cuda.current_stream().wait_stream(side)
        return out
    for _ in range(warm): step()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps): step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


base = base2 = None
for headroom in (0, 1):
    L.check(lib.gget_debug_set(L.KEY_GEMM_LDS_HEADROOM, headroom))
    b0 = run(0, 4)
    base = base if base is not None else b0
    print(f"[128x192 ring {'3 slots = 120 KiB' if headroom else '4 slots = 160 KiB'}] no side-stream kernel: {b0:.3f} ms/step")
    for lds in (4096, 32768):
        for blocks in (1, 4, 8, 32, 128):
            ms = run(blocks, lds)
            rows.append({"lds_headroom": headroom, "blocks": blocks, "lds_bytes": lds, "ms_per_step": ms, "slowdown_vs_same_config": ms / b0})
            print(f"  side kernel {blocks:4d} workgroups x {lds // 1024:3d} KiB LDS: {ms:.3f} ms/step  ({(ms / b0 - 1) * 100:+.1f} %)", flush=True)
L.check(lib.gget_debug_set(L.KEY_GEMM_LDS_HEADROOM, headroom0))
base2 = run(0, 4)
print(f"no side-stream kernel (again): {base2:.3f} ms/step")
json.dump({"baseline_ms": [base, base2], "rows": rows, "note": "step includes waiting for the ~9 ms stand-in at its end, so ms/step >= ~9.0 when blocks > 0; compare against max(baseline, 9.0)"},
          open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "coresidency.json"), "w"), indent=1)
