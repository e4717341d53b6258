"""What `training.finetune.freeze = k` buys on the fine-tune step of the C3 workload shape (bench.py "ogbl-ppa-finetune-base": base model
with LayerScale + DropPath, B 256, S 256, F 4, V 41245), freeze in {-1, 0, 6, 12}: one model per setting in ONE process, the settings
alternated step by step (the order rotated every round), every step timed by a host clock around a device synchronise, median and
spread per setting.  freeze = -1 is the step of a build without the option (the same launches): its repeat spread is the noise the
other figures are read against.

Next to each measured saving stands what the removed work predicts, from HIP-event timings of the never-frozen model's own stages:
  backward  (the decoder layers' backward stages) x k / L + the embedding backward (gget_backward_end)
  optimizer (the norm pass + AdamW launch) x the frozen share of the arenas
so a shortfall is visible.  Writes profiles/freeze_bench.json.

    python tools/freeze_bench.py [--iters 20] [--warmup 3] [--freeze=-1,0,6,12] [--out profiles/freeze_bench.json]

`--freeze=-1` needs nothing of the option, so the same file copied into a checkout of an earlier commit times that commit's step: the
figure freeze = -1 of this build is held against.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEFAULT_FREEZE = (-1, 0, 6, 12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq-len", type=int, default=256)
    ap.add_argument("--freeze", default=",".join(str(k) for k in DEFAULT_FREEZE), help="comma-separated settings; -1 (never frozen) is always timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freeze_bench.json"))
    a = ap.parse_args()
    FREEZE = tuple(dict.fromkeys([-1] + [int(x) for x in a.freeze.replace(" ", "").split(",") if x]))
    if not torch.cuda.is_available():
        raise SystemExit("freeze_bench: no GPU visible (a timing needs the device; there is no fallback)")
    importlib.import_module("graph-gpt_amd.build").build()
    M = importlib.import_module("graph-gpt_amd.modeling")
    T = importlib.import_module("graph-gpt_amd.training")
    synth = importlib.import_module("graph-gpt_amd.synth")
    sz = importlib.import_module("graph-gpt_amd.spec").MODEL_SIZES["base"]
    B, S, F, V = a.batch, a.seq_len, 4, 41245
    nl = sz["num_layers"]
    batches = [{k: torch.from_numpy(v).cuda() for k, v in
                synth.make_task_batch(B=B, S=S, F=F, V=V, seed=1234 + 1000 * i, lengths="uniform", min_len=S // 4).items() if k != "lengths"}
               for i in range(4)]

    def make(k):
        cfg = M.GraphGPTConfig(hidden_act="gelu", vocab_size=V, hidden_size=sz["hidden_size"], intermediate_size=4 * sz["hidden_size"],
                               num_hidden_layers=nl, num_attention_heads=sz["hidden_size"] // 64, max_position_embeddings=max(1024, S),
                               causal_attention=False, stacked_feat=F, next_n_token=1, attention_dropout=0.1, layer_scale_init_value=1.0,
                               path_pdrop=0.2, num_labels=2, problem_type="single_label_classification")
        model = M.GraphGPTTaskModel(cfg, seed=0)
        if k >= 0:
            model.freeze_layers(k)
        model._ensure_engine(B, S)
        model.train()
        return model, T.initialize(model, T.OptimConfig(lr=3e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1, max_grad_norm=1.0))

    runs = {k: make(k) for k in FREEZE}
    count = [0]

    def step(k):
        count[0] += 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss, _ = T.ft_batch_training(batches[count[0] % len(batches)], runs[k][1])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(loss)

    for _ in range(a.warmup):
        for k in FREEZE:
            step(k)
    times = {k: [] for k in FREEZE}
    loss = {}
    for it in range(a.iters):
        for j in range(len(FREEZE)):
            k = FREEZE[(it + j) % len(FREEZE)]
            ms, loss[k] = step(k)
            times[k].append(ms)

    # the never-frozen model's own stages, HIP events on the launch stream: what the prediction is made of
    model, eng = runs[-1]
    e = model._engine
    o = eng.optim

    def ev():
        return torch.cuda.Event(enable_timing=True)

    stage = {"begin": [], "layers": [], "end": [], "optimizer": []}
    for it in range(max(5, a.iters // 2)):
        b = batches[it % len(batches)]
        model(input_ids=b["input_ids"], attention_mask=b["attention_mask"], position_ids=b["position_ids"], task_labels=b["task_labels"])
        marks = [ev() for _ in range(5)]
        marks[0].record()
        e.backward_begin()
        marks[1].record()
        for i in range(nl - 1, -1, -1):
            e.backward_layer(i)
        marks[2].record()
        e.backward_end()
        marks[3].record()
        e.adamw_step(o.lr, o.betas[0], o.betas[1], o.eps, o.weight_decay, o.max_grad_norm, 1.0)
        marks[4].record()
        marks[4].synchronize()
        for name, i in (("begin", 0), ("layers", 1), ("end", 2), ("optimizer", 3)):
            stage[name].append(marks[i].elapsed_time(marks[i + 1]))
    st = {k: statistics.median(v) for k, v in stage.items()}

    med = {k: statistics.median(v) for k, v in times.items()}
    rows = {}
    for k in FREEZE:
        fe = runs[k][0]._engine
        frozen_share = 1.0 - sum(c for _, c in getattr(fe, "train_ranges", [(0, fe.n_params)])) / fe.n_params
        kk = min(max(k, 0), nl)
        predicted = 0.0 if k < 0 else st["layers"] * kk / nl + st["end"] + st["optimizer"] * frozen_share
        q = statistics.quantiles(times[k], n=4)
        rows[str(k)] = dict(median_ms=round(med[k], 3), min_ms=round(min(times[k]), 3), iqr_ms=round(q[2] - q[0], 3),
                            frozen_share_of_arenas=round(frozen_share, 4), saved_ms=round(med[-1] - med[k], 3),
                            predicted_saved_ms=round(predicted, 3), predicted_backward_ms=round(0.0 if k < 0 else st["layers"] * kk / nl + st["end"], 3),
                            predicted_optimizer_ms=round(0.0 if k < 0 else st["optimizer"] * frozen_share, 3), last_loss=loss[k])
    res = {"what": "fine-tune step of the C3 workload shape with finetune.freeze = k, one model per k alternated in one process; median of "
                   "host-clock step times around a device synchronise; saved_ms = median(-1) - median(k); predicted_saved_ms = backward "
                   "layer stages x k / L + embedding backward + (norm pass + AdamW) x frozen share, from HIP-event medians of the "
                   "never-frozen model's stages (stages_ms); iqr_ms of the -1 row = the same-box noise",
           "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "batch": B, "seq_len": S, "num_layers": nl,
           "stages_ms": {k: round(v, 3) for k, v in st.items()}, "rows": rows}
    print(json.dumps(res, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
