#!/usr/bin/env python3
"""Generate tests/golden/gen_eval.npz by importing the REAL reference, the same way tools/make_golden.py does (build container
only; the fixture holds arrays, none of the reference's text).

The reference's generation evaluation on the tiny fp32 model of generation.npz (V 300, d 128, L 2, F 4, B 3, ragged lengths):
`sample_per_example` (src/utils/generation_utils.py:317-436) through `eval_gen_per_sample`, `sample_per_batch` through
`eval_gen_per_batch` (src/utils/log_eval_dump_utils.py:387-447) and `cal_gen_acc_*`, for maskgit_plus / topk_margin / entropy at
temperature 0, alg_temp None.  Per run (tag = the algorithm, or maskgit_plus_s64 for the run with steps = 64) and sample b
(padding stripped, as eval_gen_per_sample strips it) the per-example run is recorded iteration by iteration:

    {tag}_b{b}_before   i64 [iters, n_b]   x when the iteration starts
    {tag}_b{b}_conf     f32 [iters, n_b]   the full confidence grid (-inf at unmasked cells)
    {tag}_b{b}_cand     i64 [iters, n_b]   the candidates (<mask> at unmasked cells)
    {tag}_b{b}_after    i64 [iters, n_b]   x when the iteration ends
    {tag}_b{b}_final    i64 [n_b]          the returned tokens

next to the inputs, the labels and the accuracy vectors of both paths.

    python tools/make_golden_gen_eval.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

# tag -> (alg, steps): steps 6 as in generation.npz (every sample runs 6 iterations); steps 64 exceeds every sample's masked count, so
# the samples run DIFFERENT numbers of iterations (steps_b = n_masked_b), one reveal each
RUNS = {"maskgit_plus": ("maskgit_plus", 6), "topk_margin": ("topk_margin", 6), "entropy": ("entropy", 6),
        "maskgit_plus_s64": ("maskgit_plus", 64)}
MASK, PAD, EPS = 1, 0, 1e-3


def import_reference_eval():
    """The reference's model classes, generation_utils and the four evaluation functions of log_eval_dump_utils.  That module
    imports the whole training stack at its top; everything it does not need for those functions is stubbed."""
    classes = MG.import_reference()
    gen = importlib.import_module("src.utils.generation_utils")
    for n in ["torchmetrics", "torchmetrics.classification", "tensorboardX", "torch.utils.tensorboard", "src.conf",
              "src.utils.misc_utils", "src.utils.metrics_utils", "src.utils.ogb_utils", "src.utils.loader_utils"]:
        if n not in sys.modules:
            m = types.ModuleType(n)
            m.__path__ = []
            m.__getattr__ = lambda name, _n=n: type(name, (), {})
            sys.modules[n] = m
    utils = sys.modules["src.utils"]
    for n in ("misc_utils", "metrics_utils", "ogb_utils", "loader_utils"):
        setattr(utils, n, sys.modules["src.utils." + n])
    utils.generation_utils = gen
    for n in ("get_metrics", "evaluate_ogb", "format_ogb_output_for_csv"):
        setattr(utils, n, None)
    led = importlib.import_module("src.utils.log_eval_dump_utils")
    return classes, gen, led


def main():
    (PT, FT, Cfg), gen, led = import_reference_eval()
    spec = MG.spec_mod.spec_from_size("tiny", kind=MG.spec_mod.KIND_PRETRAIN, vocab_size=300, stacked_feat=4, next_n_token=4)
    state = MG.weights_mod.make_state_dict(spec, seed=321, std=0.08, head_std=0.2)
    model = PT(MG.ref_config(Cfg, spec))
    MG.load_weights(model, state)
    model.eval()
    batch = MG.synth.make_pretrain_batch(B=3, S=16, F=4, V=300, seed=77)
    old = np.load(os.path.join(MG.ROOT, "tests", "golden", "generation.npz"))
    assert np.array_equal(old["in_input_ids"], batch["input_ids"]), "not the batch of generation.npz"
    ids, att, lab = (torch.from_numpy(batch[k]) for k in ("input_ids", "attention_mask", "labels"))
    B = ids.shape[0]
    res = {"in_input_ids": batch["input_ids"], "in_attention_mask": batch["attention_mask"], "in_labels": batch["labels"],
           "meta_spec": np.array(spec.as_c_ints(), np.int64), "meta_init": np.array([0.08, 0.2, 321], np.float64),
           "meta_gen": np.array([EPS, MASK, PAD], np.float64)}
    real_sample_tokens, real_spe = gen.sample_tokens, gen.sample_per_example
    for tag, (alg, steps) in RUNS.items():
        res[f"{tag}_steps"] = np.int64(steps)
        cfg = types.SimpleNamespace(eps=EPS, steps=steps, mask_token_id=MASK, pad_token_id=PAD, output_history=True, temperature=0.0,
                                    top_p=None, top_k=None, alg=alg, alg_temp=None, parallel_gen=False)
        rec = {"calls": [], "runs": []}

        def sample_tokens(*a, **k):
            conf, x0 = real_sample_tokens(*a, **k)
            rec["calls"].append((conf.clone(), x0.clone()))
            return conf, x0

        def sample_per_example(model_, cfg_, *, input_ids, attention_mask, inputs_raw_embeds):
            rec["calls"] = []
            x, hist = real_spe(model_, cfg_, input_ids=input_ids, attention_mask=attention_mask, inputs_raw_embeds=inputs_raw_embeds)
            rec["runs"].append((input_ids.clone(), x.clone(), [h.clone() for h in hist], rec["calls"]))
            return x, hist

        gen.sample_tokens, gen.sample_per_example = sample_tokens, sample_per_example
        try:
            acc_s = led.eval_gen_per_sample(model, cfg, input_ids=ids.clone(), attention_mask=att, labels=lab, inputs_raw_embeds=None)
        finally:
            gen.sample_tokens, gen.sample_per_example = real_sample_tokens, real_spe
        assert len(rec["runs"]) == B
        for b, (x_in, x_out, hist, calls) in enumerate(rec["runs"]):
            n = x_in.numel()
            assert len(hist) == len(calls) and len(hist) >= 1
            before, confs, cands, after = [], [], [], []
            cur = x_in.reshape(-1).clone()
            for h, (conf, x0) in zip(hist, calls):
                m = cur == MASK
                assert int(m.sum()) == conf.numel()
                cg = torch.full((n,), float("-inf"), dtype=torch.float32)
                tg = torch.full((n,), MASK, dtype=torch.int64)
                cg[m], tg[m] = conf.float(), x0
                before.append(cur.numpy().copy()); confs.append(cg.numpy()); cands.append(tg.numpy())
                cur = h.reshape(-1).clone()
                after.append(cur.numpy().copy())
            assert torch.equal(cur, x_out.reshape(-1))
            acc1 = gen.cal_gen_acc_per_sample(cfg, x_in, lab[b][att[b] != PAD], x_out)
            assert torch.equal(acc1, acc_s[b])
            res.update({f"{tag}_b{b}_before": np.stack(before), f"{tag}_b{b}_conf": np.stack(confs), f"{tag}_b{b}_cand": np.stack(cands),
                        f"{tag}_b{b}_after": np.stack(after), f"{tag}_b{b}_final": x_out.reshape(-1).numpy().copy()})
        cfg.output_history = False
        x_batch, _ = gen.sample_per_batch(model, cfg, input_ids=ids.clone(), attention_mask=att, inputs_raw_embeds=None)
        acc_b = led.eval_gen_per_batch(model, cfg, input_ids=ids.clone(), attention_mask=att, labels=lab, inputs_raw_embeds=None)
        assert torch.equal(acc_b, gen.cal_gen_acc_batch(cfg, ids, lab, x_batch))
        res.update({f"{tag}_acc_per_sample": acc_s.numpy(), f"{tag}_acc_per_batch": acc_b.numpy(), f"{tag}_batch_final": x_batch.numpy()})
        print(tag, "per-sample iterations", [len(r[2]) for r in rec["runs"]], "acc per sample", acc_s.numpy(), "per batch", acc_b.numpy())
    out = os.path.join(MG.ROOT, "tests", "golden", "gen_eval.npz")
    np.savez_compressed(out, **res)
    print("gen_eval written:", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
