"""What the intra-instance token head (loss_type = "token_ce_intra") costs per step, forward + backward of the head alone, at a
products-like shape: B = 64 samples of 1024 rows, d = 768, C = 47 classes whose label rows are the last 47 rows of every sample, one
labelled row in three among the others.

  hip    gget_op_tok_intra_fwd, gget_op_tok_ce, gget_op_tok_intra_bwd through the C ABI on device buffers (three calls)
  torch  the reference's own op chain on the same device and inputs (modeling_finetune.py:140-165, :198-202): F.normalize, the index
         gather of the label rows, torch.matmul, * 20, CrossEntropyLoss over the fp32 logits, autograd back to the bf16 hidden states

Both are timed with device events around one forward + backward, alternating the two in the same loop after a warm-up, median over the
iterations; the forward and the backward of the HIP path are also timed apart.  Bytes: the floor is one read of `hidden` per direction
plus one write of `dhidden` (3 rows d 2 bytes); "moved" adds what the HIP path cannot avoid on top of it - the logits written and read,
dl written and read - and is what the achieved rate is computed from.  Also compares the two paths' loss and dhidden.  Writes
profiles/intra_head.json.

    python tools/intra_head_bench.py [--iters 50] [--warmup 10] [--out profiles/intra_head.json]
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


def stat(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--C", type=int, default=47)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git rev-parse HEAD of the tree)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intra_head.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("intra_head_bench needs a GPU: nothing is measured without one")
    importlib.import_module("graph-gpt_amd.build").build()
    _lib = importlib.import_module("graph-gpt_amd._lib")
    lib = _lib.load()
    B, S, d, Cn = a.B, a.S, a.d, a.C
    T = B * S
    g = torch.Generator().manual_seed(0)
    hidden = torch.randn(T, d, generator=g).to(torch.bfloat16).cuda()
    cls = torch.full((B,), S - Cn, dtype=torch.int64)
    labels = torch.randint(0, Cn, (B, S), generator=g)
    labels[torch.rand(B, S, generator=g) > 1.0 / 3] = -100
    labels[:, S - Cn:] = -100
    labels, cls = labels.cuda(), cls.cuda()
    row_start = (torch.arange(B + 1, dtype=torch.int32) * S).cuda()
    logits = torch.empty(T, Cn, dtype=torch.float32, device="cuda")
    dl = torch.empty(T, Cn, dtype=torch.float32, device="cuda")
    stat4, loss = torch.zeros(4, device="cuda"), torch.zeros(1, device="cuda")
    dhid = torch.empty(T, d, dtype=torch.bfloat16, device="cuda")
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)       # noqa: E731
    P = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731

    def hip_fwd():
        _lib.check(lib.gget_op_tok_intra_fwd(P(hidden), P(row_start), P(cls), P(logits), B, Cn, d, st()))
        _lib.check(lib.gget_op_tok_ce(P(logits), P(labels), P(dl), P(stat4), P(loss), T, Cn, None, 0, st()))

    def hip_bwd():
        _lib.check(lib.gget_op_tok_intra_bwd(P(dl), P(stat4), P(hidden), P(row_start), P(cls), P(dhid), B, Cn, d, st()))

    def hip():
        hip_fwd()
        hip_bwd()

    h3 = hidden.view(B, S, d)
    idx1 = torch.arange(B, device="cuda").reshape(-1, 1).expand(-1, Cn).contiguous()
    idx2 = torch.arange(Cn, device="cuda").reshape(1, -1).expand(B, -1).contiguous() + cls.reshape(-1, 1)
    ce = torch.nn.CrossEntropyLoss()

    def chain():
        x = h3.detach().requires_grad_(True)
        hn = torch.nn.functional.normalize(x, dim=-1)
        lg = torch.matmul(hn, hn[idx1, idx2].transpose(-2, -1)) * 20
        ls = ce(lg.view(-1, Cn).float(), labels.view(-1))
        ls.backward()
        return ls.detach(), x.grad

    for _ in range(a.warmup):
        hip()
        chain()
    torch.cuda.synchronize()
    t_hip, t_torch, t_f, t_b = [], [], [], []
    for _ in range(a.iters):      # alternating: both see the same machine
        t_hip.append(timed(hip)[0])
        t_torch.append(timed(chain)[0])
        t_f.append(timed(hip_fwd)[0])
        t_b.append(timed(hip_bwd)[0])
    ref_loss, ref_dx = chain()
    hip()
    torch.cuda.synchronize()
    dx = dhid.float().view(B, S, d)
    rdx = ref_dx.float()
    floor = 3 * T * d * 2
    moved = floor + 2 * T * Cn * 4 * 2
    med = statistics.median(t_hip)
    res = {"what": "forward + backward of the intra-instance token head alone: HIP kernels through the C ABI against the reference's torch "
                   "op chain on the same device (device events, alternating, median)",
           "device": torch.cuda.get_device_name(0), "shape": {"B": B, "S": S, "d": d, "C": Cn, "labelled_rows": int((labels >= 0).sum())},
           "iters": a.iters, "warmup": a.warmup, "hip_fwd_bwd": stat(t_hip), "torch_chain_fwd_bwd": stat(t_torch),
           "hip_forward_with_ce": stat(t_f), "hip_backward": stat(t_b),
           "hip_over_torch": round(med / statistics.median(t_torch), 4),
           "floor_bytes": floor, "moved_bytes": moved, "floor_GBps": round(floor / med / 1e6, 1), "moved_GBps": round(moved / med / 1e6, 1),
           "launches": {"hip": 5, "note": "intra fwd, tok_ce (memset + 2 kernels), intra bwd"},
           "loss": {"hip": float(loss), "torch": float(ref_loss)},
           "dhidden_rel_l2_hip_vs_torch": float((dx - rdx).norm() / rdx.norm())}
    res["commit"] = a.commit
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
