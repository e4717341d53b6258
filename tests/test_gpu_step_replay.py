"""The engine's fine-tune step (csrc/engine.hip: backbone_forward, layer_forward, gget_forward_task, gget_backward_begin, layer_backward,
gget_backward_end, convert_bucket) against its replay through the operator entries (tests/_step_replay.py), bit for bit.

Every case builds an Engine, loads seeded weights (the norm vectors and LayerScale vectors drawn per layer - a layer that reads its
neighbour's vector must show), runs forward_task + backward, runs the replay on the same inputs and compares every observable in step
order as integers: the hidden grid of layers 0 .. L and -1, layer_qkv of every layer, logits, pooled hidden, loss, then every tensor
of e.grads() in completion order.  The tensors that are summed with fp32 atomics (tests/_step_replay.py names them and says why) are
held to the float64 sum of the replay's own stage inputs instead.  Lengths are ragged with a sample of length 1 and one of full length.

Cases (forms reached; tests/test_step_replay_host.py writes the table out):
  A  tiny, S 32 padded, T = 160: per-sample forward and backward kernels, two-problem weight-gradient group + q|k|v|o slabs, K tail;
     default and reproducible mode; with the float64 audit of the GEMM-class launches
  B  base width (d 768), 2 layers, S 32 var-len: four-problem grouped weight gradient, pad-row rule of dqkv, c2p / pad2c, dense embedding
     backward; with the audit
  C  tiny, S 72 padded (three-launch forward, two-kernel attention backward) and S 48 var-len (three-launch forward, per-sample backward
     with long_list)
  D  tiny, 3 layers, LayerScale, DropPath 0.2, MLP dropout off / on (training mode), S 32 padded: the k_ls_rmsnorm_fwd chain with the final
     norm from the last layer; k_rmsnorm_bwd_ls with fuse_next at layers 2 and 1 and not at 0; dscaled alive under the down_proj weight
     gradient; the mask seeds through the Python twins of tests/_drop_ref.py; with the audit
  E  tiny, gated stacked embedding, explicit positions with one out of range, regression head with bias: clamp, gate gradient, sorted
     embedding backward
  F  case A with set_frozen(1): boundary k_rmsnorm_dw, frozen ranges untouched
  G  one engine, three steps (A's batch, a smaller batch on the other layout, A's again; the parameters overwritten in between)
  staged: case C's var-len batch through backward_begin / backward_layer / backward_end (per-bucket conversion).
"""
import importlib

import numpy as np
import pytest
import torch

import _step_replay as R
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
eng = importlib.import_module("graph-gpt_amd.engine")
spec_mod = importlib.import_module("graph-gpt_amd.spec")
weights = importlib.import_module("graph-gpt_amd.weights")

MAXPOS = 128
FROZEN_FILL = 3.0


def make_spec(size="tiny", layers=2, **kw):
    d = {"tiny": 128, "base": 768}[size]
    base = dict(kind=spec_mod.KIND_TASK, vocab_size=300, hidden_size=d, intermediate_size=4 * d, num_layers=layers, num_heads=d // 64,
                stacked_feat=4, next_n_token=1, max_position=MAXPOS, num_labels=2)
    base.update(kw)
    return spec_mod.ModelSpec(**base)


def make_state(spec, seed):
    """Seeded weights; every norm vector 1 + 0.1 N(0,1) and every LayerScale vector 0.5 + 0.3 N(0,1), drawn per tensor."""
    st = weights.make_state_dict(spec, seed=seed, std=0.05, head_std=0.1)
    rng = np.random.RandomState(seed + 1000)
    for k, v in st.items():
        if v.ndim == 1 and (k.endswith("layernorm.weight") or k == "model.norm.weight"):
            st[k] = (1.0 + 0.1 * rng.standard_normal(v.shape)).astype(np.float32)
        elif k.endswith("lambda_1") or k.endswith("lambda_2"):
            st[k] = (0.5 + 0.3 * rng.standard_normal(v.shape)).astype(np.float32)
        elif k == "score.bias":
            st[k] = (0.1 * rng.standard_normal(v.shape)).astype(np.float32)
    return st


def make_batch(spec, lens, S, seed, bad_pos=False, regression=False):
    rng = np.random.RandomState(seed)
    B, F = len(lens), spec.stacked_feat
    ids = np.zeros((B, S, F), np.int64)
    mask = np.zeros((B, S), np.int64)
    pos = np.zeros((B, S), np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = rng.randint(22, spec.vocab_size, size=(n, F))
        mask[b, :n] = 1
        pos[b, :n] = np.arange(n)
    if bad_pos:
        pos[0, 3] = MAXPOS + 5           # out of range: clamped to MAXPOS - 1
        pos[2, :lens[2]] = np.arange(lens[2])[::-1] + 7    # and a sample whose positions are no arange
    y = rng.standard_normal(size=(B,)).astype(np.float32) if regression else rng.randint(0, spec.num_labels, size=(B,)).astype(np.int64)
    return dict(ids=torch.from_numpy(ids).cuda(), mask=torch.from_numpy(mask).cuda(), pos=torch.from_numpy(pos).cuda(),
                y=torch.from_numpy(y).cuda(), lens=list(lens), S=S, tokens=int(sum(lens)))


def completion_order(spec):
    """The names of e.grads() in the order the backward finishes them: heads, layers L-1 .. 0, embeddings."""
    offs, _ = R.param_offsets(spec)
    Ln = spec.num_layers
    return sorted(offs, key=lambda n: (R.bucket_of(offs[n][2], Ln), offs[n][0]))


def grid_of(rep, buf, cols, qkv=False):
    """The replay's rows in the [B, S, cols] grid: var-len rows through the replay's OWN pad2c (zeros behind a sample); the q|k|v accessor
    zeroes the positions behind a sample on the padded layout as well."""
    B, S = rep.B, rep.S
    body = buf.body()
    if rep.f["layout"] == "varlen":
        p2c = rep.pad2c[:B * S].long()
        out = torch.zeros(B * S, cols, dtype=body.dtype, device="cuda")
        live = p2c >= 0
        out[live] = body[p2c[live]]
        return out.view(B, S, cols)
    out = body[:B * S].clone().view(B, S, cols)
    if qkv:
        s = torch.arange(S, device="cuda")[None, :] >= rep.key_len[:B, None]
        out[s] = 0
    return out


def run_step(e, spec, batch, *, varlen=False, frozen=-1, reproducible=False, staged=False, audit=False, problem=L.PROBLEM_SINGLE_LABEL,
             path_p=0.0, mlp_p=0.0, seed=0, case="?"):
    """One engine step and its replay; raises with the first differing observable.  Returns the replay."""
    B, S = batch["ids"].shape[:2]
    Ln, d = spec.num_layers, spec.hidden_size
    nt = batch["tokens"] if varlen else None
    menu = {L.KEY_DETERMINISTIC: 1} if reproducible else {}
    offs, _ = R.param_offsets(spec)
    assert {k: v["offset"] for k, v in e.params.items()} == {k: v[0] for k, v in offs.items()}, "the replay's parameter offsets are not the plan's"
    with L.debug_menu(menu):
        if frozen >= 0:
            e.grad_bf16.fill_(FROZEN_FILL)
        e.set_dropout(0.0, path_p, seed)
        if mlp_p > 0:
            e.set_dropout_ex(0.0, mlp_p, 0.0)
        loss, logits, pooled = e.forward_task(batch["ids"], batch["mask"], batch["pos"], batch["y"], problem=problem, num_tokens=nt)
        assert e.varlen_status()[0] == varlen, "the engine did not run the layout the case is about"
        obs = []
        for i in range(Ln + 1):
            obs.append((f"hidden[{i}]", e.layer_hidden_states(i, B, S).clone()))
            if i < Ln:
                obs.append((f"qkv[{i}]", e.layer_qkv(i, B, S).clone()))
        obs.append(("hidden[-1] (final norm)", e.hidden_states(B, S).clone()))
        obs += [("task logits", logits.clone()), ("pooled hidden", pooled.clone()), ("loss", loss.reshape(1).clone())]
        if staged:
            e.backward_begin()
            for i in range(Ln - 1, -1, -1):
                e.backward_layer(i)
            e.backward_end()
        else:
            e.backward()
        torch.cuda.synchronize()
        grads = {k: v.clone() for k, v in e.grads().items()}
        rep = R.Replay(spec, e.param_bf16.clone(), tuple(t.cuda() for t in eng.rope_tables(MAXPOS, 64, spec.rope_theta)), MAXPOS, num_tokens=nt,
                       seed=seed, path_p=path_p, mlp_p=mlp_p, frozen=frozen, reproducible=reproducible, staged=staged, audit=audit, problem=problem)
        rep.forward(batch["ids"], batch["mask"], batch["pos"], batch["y"]).backward()
    assert rep.f["layout"] == ("varlen" if varlen else "padded")
    want = {}
    for i in range(Ln + 1):
        want[f"hidden[{i}]"] = grid_of(rep, rep.x[i], d)
        if i < Ln:
            want[f"qkv[{i}]"] = grid_of(rep, rep.lw[i]["qkv"], 3 * d, qkv=True)
    want["hidden[-1] (final norm)"] = grid_of(rep, rep.hidden, d)
    want["task logits"], want["pooled hidden"], want["loss"] = rep.logits.body(), rep.pooled.body(), rep.loss.body().reshape(1)
    pairs = [(f"{case}: {n}", g, want[n]) for n, g in obs]
    first = rep.f["first_layer"]
    trunc = R.truncated(spec, frozen)
    frozen_names = []
    for n in completion_order(spec):
        layer = offs[n][2]
        is_frozen = frozen >= 0 and (layer < first if layer >= 0 else (n == "model.embed_tokens.weight")) and layer != Ln
        if is_frozen and trunc:
            frozen_names.append(n)
        elif is_frozen:
            continue                      # (a frozen tensor above a trainable gate: computed by the full chain, read by nobody)
        elif n not in rep.inexact:
            pairs.append((f"{case}: grad {n}", grads[n], rep.grad(n)))
    msg = R.first_difference(pairs)
    assert msg is None, msg
    # the frozen ranges: untouched in the engine, still at the sentinel in the replay
    for n in frozen_names:
        assert bool((grads[n].float() == FROZEN_FILL).all()), f"{case}: the engine wrote the frozen gradient {n}"
        assert bool((rep.grad(n).contiguous().view(torch.int16) == R.SENT16).all()), f"{case}: the replay wrote the frozen gradient {n}"
    # the atomically summed tensors: the float64 sum of the replay's stage inputs
    worst = 0.0
    for who, gr in (("engine", grads), ("replay", {k: rep.grad(k) for k in grads})):
        for n, (ratio, fail) in rep.check_bounded(gr, who).items():
            assert fail is None, f"{case}: {fail}"
            worst = max(worst, ratio)
    missing = [n for n in rep.inexact if n not in rep.sums and n not in frozen_names and not (frozen >= 0 and offs[n][2] < first)]
    assert not missing, f"{case}: no float64 statement for {missing}"
    record_error(f"step_replay/{case}", "atomic sums: worst err / bound", worst, 1.0)
    # guard rows of every buffer of the replay
    bufs = [(k, v) for k, v in vars(rep).items() if isinstance(v, R.Buf)] + [(f"x[{i}]", b) for i, b in enumerate(rep.x)] + \
           [(f"dx[{k}]", b) for k, b in rep.dx.items()] + [(f"L{i}.{k}", b) for i, w in enumerate(rep.lw) for k, b in w.items()]
    torn = [k for k, b in bufs if not b.guard_intact()]
    assert not torn, f"{case}: guard rows written behind {torn}"
    if audit:
        assert rep.audit_ratio, "the audit ran over nothing"
        for k, r in rep.audit_ratio.items():
            record_error(f"step_replay/{case}", f"float64 audit: {k}", r, 1.0)
    return rep


def new_engine(spec, state, max_tokens, max_batch):
    e = eng.Engine(spec, max_tokens=max_tokens, max_batch=max_batch)
    e.load_state_dict(state)
    return e


LENS_A = (32, 26, 1, 17, 9)           # T = 160: two K-tiles and a tail of 32 rows; real tokens in the rows that case G's second step leaves as round-up rows


@pytest.mark.parametrize("reproducible", [False, True], ids=["default", "reproducible"])
def test_case_a_tiny_padded(reproducible):
    spec = make_spec()
    e = new_engine(spec, make_state(spec, 11), 160, 5)
    rep = run_step(e, spec, make_batch(spec, LENS_A, 32, 21), reproducible=reproducible, audit=not reproducible,
                   case="A-reproducible" if reproducible else "A")
    assert (rep.f["attn_fwd"], rep.f["attn_bwd"], rep.f["wgrad"], rep.f["embed_bwd"]) == ("per-sample", "per-sample", "grouped-2+qkvo-slabs-split1", "dense")


def test_case_b_base_width_varlen():
    spec = make_spec("base", vocab_size=756)
    lens = (32, 1, 20, 7, 29, 13)       # 102 real tokens -> 128 rows, 26 round-up rows
    e = new_engine(spec, make_state(spec, 12), 6 * 32, 6)
    rep = run_step(e, spec, make_batch(spec, lens, 32, 22), varlen=True, audit=True, case="B")
    assert (rep.f["T"], rep.f["wgrad"], rep.f["embed_bwd"], rep.f["attn_bwd"]) == (128, "grouped-4", "dense", "per-sample")


def test_case_c_long_rows():
    spec = make_spec()
    st = make_state(spec, 13)
    e = new_engine(spec, st, 3 * 72, 4)
    rep = run_step(e, spec, make_batch(spec, (72, 40, 1), 72, 23), case="C-S72-padded")
    assert (rep.f["attn_fwd"], rep.f["attn_bwd"], rep.f["pack_wo"]) == ("three-launch", "norm-bwd+dgrad+attn-bwd", "none")
    # (same engine: rows 102 .. 127 of the q|k|v gradient hold the step above's real tokens - the pad-row clear of this step has work to do)
    rep = run_step(e, spec, make_batch(spec, (48, 1, 33, 20), 48, 24), varlen=True, case="C-S48-varlen")
    assert (rep.f["attn_fwd"], rep.f["attn_bwd"], rep.f["T"]) == ("three-launch", "per-sample+long_list", 128)


@pytest.mark.parametrize("mlp_p", [0.0, 0.1], ids=["mlp-dropout-off", "mlp-dropout-on"])
def test_case_d_layerscale_droppath(mlp_p):
    spec = make_spec(layers=3, layer_scale_init=1.0, path_pdrop=0.2, mlp_pdrop=mlp_p)
    e = new_engine(spec, make_state(spec, 19), 128, 4)
    rep = run_step(e, spec, make_batch(spec, (32, 1, 15, 24), 32, 29), path_p=0.2, mlp_p=mlp_p, seed=1234, audit=True,
                   case="D-mlp-dropout-on" if mlp_p else "D")
    assert rep.f["ln1_bwd"] == {2: "fuse_next", 1: "fuse_next", 0: "plain"} and rep.f["final_norm"] == "from-last-layer"
    assert (rep.f["attn_fwd"], rep.f["final_norm_bwd"], rep.f["pack_wo"]) == ("ls-residual", "fused-ls2", "none")
    keeps = [float(k) for i in range(3) for w in (0, 1) for k in __import__("_drop_ref").path_keep(rep.path(i, w)[1], np.arange(4), rep.path(i, w)[0])]
    assert 0.0 in keeps and max(keeps) > 1.0, "the batch and seed of this case must drop a sample's branch and keep another"


def test_staged_backward_converts_per_bucket():
    spec = make_spec()
    e = new_engine(spec, make_state(spec, 14), 4 * 48, 4)
    run_step(e, spec, make_batch(spec, (48, 1, 33, 20), 48, 25), varlen=True, staged=True, case="staged-S48-varlen")


def test_case_e_gated_embedding_clamped_positions_regression():
    spec = make_spec(gated_agg=True, num_labels=1, score_bias=True)
    e = new_engine(spec, make_state(spec, 15), 128, 4)
    rep = run_step(e, spec, make_batch(spec, (32, 1, 15, 24), 32, 26, bad_pos=True, regression=True), problem=L.PROBLEM_REGRESSION_L1, case="E")
    assert rep.f["embed_bwd"] == "sorted" and int(rep.pos_flag[0]) == 1 and e.positions_clamped()


def test_case_f_frozen_prefix():
    spec = make_spec()
    e = new_engine(spec, make_state(spec, 11), 160, 5)
    e.set_frozen(1)
    rep = run_step(e, spec, make_batch(spec, LENS_A, 32, 21), frozen=1, case="F")
    assert rep.f["ln1_bwd"] == {1: "dw-only"} and rep.f["embed_bwd"] == "none"


def test_case_g_three_steps_on_one_engine():
    """Stale rows of reused workspaces and the per-forward repack of the o weights: the parameters are overwritten between the steps."""
    spec = make_spec()
    e = new_engine(spec, make_state(spec, 16), 160, 5)
    a = make_batch(spec, LENS_A, 32, 27)
    run_step(e, spec, a, case="G-step1")
    e.load_state_dict(make_state(spec, 17))
    run_step(e, spec, make_batch(spec, (24, 1, 10), 24, 28), varlen=True, case="G-step2")
    # (a caller's own write into the bf16 arena, past gget_sync_params: the forward still has to repack what it reads)
    for k, v in make_state(spec, 18).items():
        e.view(k, "bf16").copy_(torch.from_numpy(v).to(torch.bfloat16))
    run_step(e, spec, a, case="G-step3")
