"""The fixtures of the model sizes with 32-wide attention heads (tools/make_golden_hd32.py) for the parity tests: tests/_util.py:load_case
with the head width derived from the stored spec as hidden / heads (that loader fixes 64)."""
import os

import numpy as np

from _util import GOLDEN, spec_mod, weights_mod

PT32 = ["pt_tiny6_f13", "pt_tiny6_s72", "pt_tiny6_causal", "pt_tiny6_packed"]
FT32 = ["ft_tiny6_f4_b32"]
BIG32 = ["pt_small12_f13"]       # the "big" storage form: gradient norms and 64 x 64 corner blocks
ATTN32 = ["attn_tiny6_padded", "attn_tiny6_packed"]


def spec_of(z, layer_scale=0.0):
    m = [int(x) for x in z["meta_spec"]]
    assert m[2] % m[5] == 0
    return spec_mod.ModelSpec(kind=m[0], vocab_size=m[1], hidden_size=m[2], intermediate_size=m[3], num_layers=m[4], num_heads=m[5],
                              head_dim=m[2] // m[5], stacked_feat=m[6], next_n_token=m[7], gated_agg=bool(m[8]), causal=bool(m[9]),
                              max_position=m[10], num_labels=m[11], score_bias=bool(m[12]), pad_token_id=m[13], layer_scale_init=layer_scale)


def load_case32(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    spec = spec_of(z, float(z["meta_layer_scale"]))
    assert spec.head_dim == 32 and list(spec.as_c_ints()) == [int(x) for x in z["meta_spec"]]
    std, head_std, seed = [float(x) for x in z["meta_init"]]
    state = weights_mod.make_state_dict(spec, seed=int(seed), std=std, head_std=None if head_std < 0 else head_std)
    batch = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    return z, spec, state, batch


def load_attn32(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    spec = spec_of(z)
    seed, std, hstd = z["meta_init"]
    state = weights_mod.make_state_dict(spec, seed=int(seed), std=float(std), head_std=float(hstd))
    batch = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    return z, spec, state, batch
