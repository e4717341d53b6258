#!/usr/bin/env python3
"""Generate tests/golden/pt_tiny_cl.npz: the reference's contrastive pre-training model (task_type "pretrain-cl": use_generative and
use_discriminative, modeling_pretrain.py:96-115, :238-257) on one seeded batch - head1_loss, head2_loss, head2_logits, the pooled
rows of its final-norm output, the per-parameter gradient norms of (head1 + head2).backward() and two full gradients.  Data only;
the import recipe and the helpers are those of tools/make_golden.py.

    python tools/make_golden_cl.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

NAME = "pt_tiny_cl"
B, S, F, V = 6, 24, 13, 756
INIT = dict(std=0.06, head_std=0.15)
MIN_COSINE_SPAN = 0.2     # off-diagonal cosines of the reference embeddings must span more than this (see run)


def run(seed):
    PT, _, Cfg = MG.import_reference()
    spec = MG.spec_mod.spec_from_size("tiny", kind=MG.spec_mod.KIND_PRETRAIN_CL, vocab_size=V, stacked_feat=F, next_n_token=F)
    state = MG.weights_mod.make_state_dict(spec, seed=100 + seed, **INIT)
    names = list(state.keys())
    batch = MG.synth.make_pretrain_batch(F=F, V=V, B=B, S=S, seed=seed)      # pcqm lengths: the last real rows differ per sample
    cfg = MG.ref_config(Cfg, spec, use_generative=True, use_discriminative=True)
    tb = {k: torch.from_numpy(v) for k, v in batch.items()}

    def build(dtype=None):
        m = PT(cfg)
        MG.load_weights(m, state)
        return (m if dtype is None else m.to(dtype)).eval()

    def fwd(m):
        return m(input_ids=tb["input_ids"], attention_mask=tb["attention_mask"], labels=tb["labels"], inputs_raw_embeds=None,
                 output_hidden_states=True)

    model = build()
    assert model.ratio_dis == 0.5 and model.world_size == 1
    o = fwd(model)
    z = o.head2_logits.detach().double()
    e = z / z.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    cos = (e @ e.t())[~torch.eye(B, dtype=torch.bool)]
    span = float(cos.max() - cos.min())
    # with collinear embeddings every score is 20 and the loss at temperature 20 probes nothing: another seed then
    assert span > MIN_COSINE_SPAN, f"seed {seed}: off-diagonal cosines span {span:.3f} only"
    model.zero_grad()
    (o.head1_loss + o.head2_loss).backward()
    g = dict(model.named_parameters())
    out = {"loss": np.float64(o.head1_loss.item()), "head2_loss": np.float64(o.head2_loss.item()),
           "head2_logits": o.head2_logits.detach().float().numpy().copy(), "cosine_span": np.float64(span),
           "grad_norms": MG.grad_norms(model, names),
           "grad_cl_proj": g["cl_proj.weight"].grad.numpy().copy(),
           "grad_l1_down": g["model.layers.1.mlp.down_proj.weight"].grad.numpy().copy()}
    # the rows cl_proj reads: the final-norm output at r_b = (non-pad entries of input_ids[b, :, 0]) - 1
    r = (tb["input_ids"][:, :, 0] != cfg.pad_token_id).sum(-1) - 1
    out["pool_rows"] = r.numpy().astype(np.int64)
    out["cl_hidden_rows"] = o.hidden_states[-1][torch.arange(B), r].detach().float().numpy().copy()
    # head1 alone: cl_proj gets no gradient from it
    model.zero_grad()
    fwd(model).head1_loss.backward()
    out["grad_norms_head1_only"] = MG.grad_norms(model, names)
    # the reference's own bf16 module path: the loss gaps the tolerances derive from
    with torch.no_grad():
        ob = fwd(build(torch.bfloat16))
    out["loss_bf16"] = np.float64(ob.head1_loss.item())
    out["head2_loss_bf16"] = np.float64(ob.head2_loss.item())
    out["head2_logits_bf16"] = ob.head2_logits.float().numpy().copy()
    for k, v in batch.items():
        out["in_" + k] = v
    out["meta_spec"] = np.array(spec.as_c_ints(), np.int64)
    out["meta_layer_scale"] = np.float64(spec.layer_scale_init)
    out["meta_init"] = np.array([INIT["std"], INIT["head_std"], 100 + seed], np.float64)
    out["meta_size"] = np.array("tiny")
    path = os.path.join(MG.ROOT, "tests", "golden", NAME + ".npz")
    np.savez_compressed(path, **out)
    print(f"{NAME}: seed {seed} head1 {out['loss']:.6f} (bf16 {out['loss_bf16']:.6f}) head2 {out['head2_loss']:.6f} "
          f"(bf16 {out['head2_loss_bf16']:.6f}) cosine span {span:.3f} rows {out['pool_rows'].tolist()} -> {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 31)
