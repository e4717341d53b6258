"""The prediction passes on the device model (graph-gpt_amd/inference.py, the epoch's end of training.FinetuneMode): the tiny task model
of the ft_tiny_f4 fixture and the tiny token_ce model, both token layouts.  The launch menu is pinned to its deterministic selection, so
that a second forward of the same batch gives the same bits and the passes can be compared with the model's own outputs for equality."""
import importlib
import os

import numpy as np
import pytest
import torch

import _infer_ref as R
from _util import GOLDEN, load_case, spec_mod, synth, weights_mod

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
Mod = importlib.import_module("graph-gpt_amd.modeling")
tr = importlib.import_module("graph-gpt_amd.training")
inf = importlib.import_module("graph-gpt_amd.inference")


@pytest.fixture(autouse=True)
def reproducible():
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):
        yield


def _ft_config(spec):
    return Mod.GraphGPTConfig(hidden_act="gelu", vocab_size=spec.vocab_size, hidden_size=spec.hidden_size,
                              intermediate_size=spec.intermediate_size, num_hidden_layers=spec.num_layers,
                              num_attention_heads=spec.num_heads, max_position_embeddings=spec.max_position, causal_attention=spec.causal,
                              stacked_feat=spec.stacked_feat, num_labels=spec.num_labels, problem_type="single_label_classification",
                              layer_scale_init_value=spec.layer_scale_init, rms_norm_eps=spec.rms_eps, pad_token_id=spec.pad_token_id)


def _ft_model(layout):
    _, spec, state, batch = load_case("ft_tiny_f4")
    model = Mod.GraphGPTTaskModel(_ft_config(spec), seed=1)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model.token_layout = layout
    return model.cuda(), spec, batch["input_ids"].shape[1]


def _batches(spec, S, sizes, seed):
    """collated CPU batches of the given sizes with ragged lengths and sample indices that are neither sorted nor small"""
    out, first = [], 0
    for k, B in enumerate(sizes):
        b = synth.make_task_batch(B=B, S=S, F=spec.stacked_feat, V=spec.vocab_size, seed=seed + k, num_labels=spec.num_labels)
        d = {n: torch.from_numpy(v) for n, v in b.items() if n != "lengths"}
        d["idx"] = 3_000_000_000 - 7 * (torch.arange(B) + first)
        first += B
        out.append(d)
    return out


class _SizedLoader(list):
    """a loader with a `.dataset` that knows its length (the arenas are sized once)"""

    def __init__(self, batches):
        super().__init__(batches)
        self.dataset = range(sum(len(b["idx"]) for b in batches))


def _per_batch(model, loader):
    """the reference's statement: per batch model(...) without labels (on the token layout ft_evaluate's `_layout_kw` selects), .half(),
    stacked"""
    model.eval()
    dev = model.device
    lg, hs = [], []
    with torch.no_grad():
        for d in loader:
            res = model(input_ids=d["input_ids"].to(dev), attention_mask=d["attention_mask"].to(dev), position_ids=d["position_ids"].to(dev),
                        **tr._layout_kw(model, d))
            lg.append(res.task_logits.half())
            hs.append(res.task_hidden_states.half())
    return torch.vstack(lg), torch.vstack(hs)


@pytest.mark.parametrize("layout", ["padded", "varlen"])
def test_ft_infer_hidden_states_equals_the_per_batch_statement(layout):
    model, spec, S = _ft_model(layout)
    batches = _batches(spec, S, (4, 4, 2), 40)
    want_l, want_h = _per_batch(model, batches)
    want_idx = torch.cat([b["idx"] for b in batches])
    for loader in (_SizedLoader(batches), batches):
        idx, logits, hidden = inf.ft_infer_hidden_states(model, loader, save_hidden_states=True)
        assert not model.training and idx.is_cuda and logits.is_cuda and hidden.is_cuda
        assert idx.dtype == torch.int64 and tuple(idx.shape) == (10, 1) and torch.equal(idx.view(-1).cpu(), want_idx)
        assert logits.dtype == hidden.dtype == torch.float16
        assert tuple(logits.shape) == (10, spec.num_labels) and tuple(hidden.shape) == (10, spec.hidden_size)
        assert torch.equal(logits.view(torch.int16), want_l.view(torch.int16)) and torch.equal(hidden.view(torch.int16), want_h.view(torch.int16))
    # growth by doubling: a first batch of one sample sizes the arenas for four rows; 1 + 4 + 4 + 2 rows double them twice
    ragged = _batches(spec, S, (1, 4, 4, 2), 60)
    want_l, want_h = _per_batch(model, ragged)
    idx, logits, hidden = inf.ft_infer_hidden_states(model, ragged, save_hidden_states=True)
    assert torch.equal(idx.view(-1).cpu(), torch.cat([b["idx"] for b in ragged]))
    assert torch.equal(logits.view(torch.int16), want_l.view(torch.int16)) and torch.equal(hidden.view(torch.int16), want_h.view(torch.int16))
    # hidden states only when asked for: the keyword, or the reference-shaped config's flag
    assert inf.ft_infer_hidden_states(model, batches)[2] is None
    ns = lambda **k: type("NS", (), k)()       # noqa: E731
    cfg = ns(training=ns(ft_eval=ns(save_hidden_states=True)))
    out = inf.ft_infer_hidden_states(model, batches, cfg, "test")
    assert torch.equal(out[2].view(torch.int16), _per_batch(model, batches)[1].view(torch.int16))
    cfg.training.ft_eval.save_hidden_states = False
    assert inf.ft_infer_hidden_states(model, batches, cfg, "test")[2] is None
    model.check_deferred()


def test_inference_under_ema_weights_differs_and_restores():
    model, spec, S = _ft_model("padded")
    eng = tr.initialize(model, tr.OptimConfig(lr=1e-2, use_ema=True, ema_decay=0.5))
    for d in _batches(spec, S, (8, 8, 8, 8), 90):
        tr.ft_batch_training({k: v.cuda() for k, v in d.items() if k != "idx"}, eng)
    batches = _batches(spec, S, (4, 4, 2), 40)
    live = inf.ft_infer_hidden_states(model, batches, save_hidden_states=True)
    with eng.ema_weights():
        ema = inf.ft_infer_hidden_states(model, batches, save_hidden_states=True)
        want_l, want_h = _per_batch(model, batches)
    after = inf.ft_infer_hidden_states(model, batches, save_hidden_states=True)
    assert torch.equal(ema[1].view(torch.int16), want_l.view(torch.int16)) and torch.equal(ema[2].view(torch.int16), want_h.view(torch.int16))
    assert not torch.equal(ema[1], live[1]) and not torch.equal(ema[2], live[2]), "the averaged weights must give other outputs"
    for a, b in zip(after, live):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a, b.view(torch.int16) if b.dtype == torch.float16 else b)


# ------------------------------------------------------------------------------------------------ node-level records
def _token_model(layout):
    z = np.load(os.path.join(GOLDEN, "ft_tiny_tokence.npz"))
    ncls = 7
    spec = spec_mod.spec_from_size("tiny", kind=spec_mod.KIND_TASK, vocab_size=756, stacked_feat=13, next_n_token=1, num_labels=ncls)
    seed, std, hstd = z["meta_init"]
    state = weights_mod.make_state_dict(spec, seed=int(seed), std=float(std), head_std=float(hstd))
    b = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    cfg = Mod.GraphGPTConfig(hidden_act="gelu", vocab_size=756, hidden_size=spec.hidden_size, intermediate_size=spec.intermediate_size,
                             num_hidden_layers=spec.num_layers, num_attention_heads=spec.num_heads,
                             max_position_embeddings=spec.max_position, causal_attention=False, stacked_feat=13, next_n_token=1,
                             num_labels=ncls, loss_type="token_ce", problem_type="single_label_classification")
    model = Mod.GraphGPTTaskModel(cfg, seed=1)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model.token_layout = layout
    return model.cuda(), b, ncls


@pytest.mark.parametrize("layout", ["padded", "varlen"])
def test_process_data_equals_the_twin_on_the_models_logits(layout):
    model, b, ncls = _token_model(layout)
    B, S = b["attention_mask"].shape
    rng = np.random.RandomState(8)
    real = b["attention_mask"].bool().numpy()
    raw = np.where(real & (rng.rand(B, S) < 0.7), rng.randint(0, 2 ** 40, (B, S)), -100).astype(np.int64)
    idx = np.arange(B, dtype=np.int64) * 11 + 2 ** 32
    data = {"input_ids": b["input_ids"], "attention_mask": b["attention_mask"], "idx": idx, "raw_node_idx": torch.from_numpy(raw)}
    model.eval()
    with torch.no_grad():
        logits = model(input_ids=b["input_ids"].cuda(), attention_mask=b["attention_mask"].cuda(), **tr._layout_kw(model, data)).task_logits
    assert tuple(logits.shape) == (B, S, ncls)
    want = R.node_records(R.argmax_first(logits.cpu().numpy()), raw, idx)
    rec = inf.process_data(model, data, model.device)
    assert isinstance(rec, list) and len(rec) == int((raw != -100).sum()) > 0 and all(isinstance(r, tuple) and len(r) == 3 for r in rec)
    assert np.array(rec, dtype=np.int64).tolist() == want.tolist()
    # idx as a tensor; the device form with one arena and one cursor over two batches; a writer per batch
    assert inf.process_data(model, dict(data, idx=torch.from_numpy(idx)), model.device) == rec
    n = len(rec)
    records = torch.full((2 * n + 1, 3), -5, dtype=torch.int64, device="cuda")
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    for _ in range(2):
        got = inf.node_records(model, data, records=records, state=state)
        assert got[0] is records and got[1] is state
    assert state.tolist() == [2 * n, 0] and records[:2 * n].cpu().numpy().tolist() == want.tolist() * 2 and (records[2 * n:] == -5).all()
    rec1, st1 = inf.node_records(model, data)
    assert st1.tolist() == [n, 0] and rec1[:n].cpu().numpy().tolist() == want.tolist()
    seen = []
    writer = type("W", (), {"write": lambda self, records, indices: seen.append((records, indices))})()
    assert inf.dump_results(model, [data, data], model.device, writer, slice_id=0) == 2 * n
    assert [s[1] for s in seen] == [[0, 1, 2]] * 2 and seen[0][0] == rec and seen[1][0] == rec
    model.check_deferred()


# ------------------------------------------------------------------------------------------------ the fine-tune epoch's end
@pytest.mark.parametrize("use_ema", [False, True])
def test_finetune_mode_closes_the_epoch_and_eval_only_reproduces_it(tmp_path, use_ema, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    _, spec, _, fixture = load_case("ft_tiny_f4")
    S = fixture["input_ids"].shape[1]
    train = [{k: v for k, v in d.items() if k != "idx"} for d in _batches(spec, S, (8, 8), 10)]
    valid, test, train_eval = _batches(spec, S, (4, 4, 2), 40), _batches(spec, S, (4, 4, 2), 50), _batches(spec, S, (4,), 10)
    out_dir = str(tmp_path / "out")
    kw = dict(problem_type="single_label_classification", num_labels=spec.num_labels, dataset_name="ogbl-ppa")
    mode = tr.FinetuneMode(batches=train, valid_loader=valid, test_loader=test, train_loader_for_eval=train_eval, steps_per_epoch=2,
                           save_pred=True, save_hidden_states=True, eval_kwargs=kw)
    cfg = dict(model=_ft_config(spec), optim=tr.OptimConfig(lr=1e-3, use_ema=use_ema, ema_decay=0.5), batches=train, max_steps=2,
               output_dir=out_dir)
    p = tr.TrainingPipeline(cfg, mode).run()
    assert p.engine.global_steps == 2 and len(mode.epoch_results) == 1 and p.model.training
    r = mode.epoch_results[0]
    ep = os.path.join(out_dir, "epoch_0")
    names = sorted(os.listdir(ep))
    for want in ("model.pt", "task_logits_0.csv", "hidden_states_0.csv", "train_results.csv", "valid_results.csv", "test_results.csv"):
        assert want in names, names
    assert (os.path.exists(os.path.join(out_dir, "model_ema.pt")), r["valid_ema"] is not None) == (use_ema, use_ema)
    assert list(r["valid"]) == ["hits@100"] and r["is_best"] and mode.best_epoch == 0
    assert mode.best_res == (r["valid_ema"] if use_ema else r["valid"])
    assert len(p.log_lines) == 1 and p.log_lines[0].startswith("0,2,") and p.log_lines[0].endswith("\n")
    # the dumped rows decode to the returned tensors, in loader order
    for stem, t in (("task_logits", r["logits"]), ("hidden_states", r["hidden_states"])):
        with open(os.path.join(ep, f"{stem}_0.csv")) as fh:
            rows = [ln.rstrip("\n").split(",") for ln in fh]
        assert [int(x[0]) for x in rows] == r["idx"].view(-1).tolist() == torch.cat([b["idx"] for b in test]).tolist()
        assert np.stack([inf.decode_numpy_array(x[1]) for x in rows]).tobytes() == t.cpu().numpy().tobytes()
    with open(os.path.join(ep, "valid_results.csv")) as fh:
        lines = fh.read().splitlines()
    assert lines[0] == "y_true,y_pred,idx" and len(lines) == 11
    # eval_only over the same directory: the same validation result from the checkpoint, nothing trained, nothing rewritten
    read = lambda path: open(path, "rb").read()        # noqa: E731
    epoch_model, root_model = read(os.path.join(ep, "model.pt")), read(os.path.join(out_dir, "model.pt"))
    os.remove(os.path.join(ep, "task_logits_0.csv"))
    mode2 = tr.FinetuneMode(valid_loader=valid, test_loader=test, eval_only=True, save_hidden_states=False, eval_kwargs=kw)
    assert not mode2.allow_resume() and not mode2.allow_save_config()
    p2 = tr.TrainingPipeline(dict(model=_ft_config(spec), optim=tr.OptimConfig(lr=1e-3), batches=[], output_dir=out_dir), mode2).run()
    assert p2.engine.global_steps == 0 and len(mode2.epoch_results) == 1
    r2 = mode2.epoch_results[0]
    assert r2["epoch"] == 0 and r2["valid"] == r["valid"] and r2["valid_ema"] is None
    # the same weights (model.pt holds the fp32 masters the first run evaluated) on an engine created for another batch size: the loss and
    # the logits agree to the bf16 rounding of the activations (2^-8 relative per rounding, a handful of them behind a logit of order 1)
    assert r2["valid_loss"] == pytest.approx(r["valid_loss"], rel=2e-2)
    if not use_ema:         # (with an EMA the first run tested on the averaged weights)
        assert r2["test"] == r["test"] and torch.allclose(r2["logits"].float(), r["logits"].float(), rtol=2e-2, atol=2e-2)
    assert r2["hidden_states"] is None and os.path.exists(os.path.join(ep, "task_logits_0.csv"))
    ck = torch.load(os.path.join(ep, "model.pt"), map_location="cpu")
    sd = p2.model.state_dict()
    assert all(torch.equal(sd[k].cpu().reshape(v.shape), v) for k, v in ck.items())
    assert read(os.path.join(ep, "model.pt")) == epoch_model and read(os.path.join(out_dir, "model.pt")) == root_model
    # infer_only: the records go to the caller's writer instead of the evaluation.  (A graph-level model's [B, C] output is process_data's
    # prediction form: C positions per sample, the logit truncated to an integer.)
    node_test = [dict(b, raw_node_idx=torch.tensor([[5, -100]] * len(b["idx"])) + torch.arange(len(b["idx"]))[:, None] * torch.tensor([1, 0]))
                 for b in test]
    got = []
    writer = type("W", (), {"write": lambda self, records, indices: got.append((records, indices))})()
    mode3 = tr.FinetuneMode(valid_loader=valid, test_loader=node_test, eval_only=True, infer_only=True, infer_writer=writer, eval_kwargs=kw)
    tr.TrainingPipeline(dict(model=_ft_config(spec), batches=[], output_dir=out_dir), mode3).run()
    assert mode3.epoch_results == [{"epoch": 0, "records": 10}] and [len(g[0]) for g in got] == [4, 4, 2] and all(g[1] == [0, 1, 2] for g in got)
    assert [int(r[0]) for g in got for r in g[0]] == torch.cat([b["idx"] for b in test]).tolist()
    assert [int(r[1]) for r in got[0][0]] == [5, 6, 7, 8]
    assert [int(r[2]) for g in got for r in g[0]] == r2["logits"][:, 0].float().cpu().numpy().astype(np.int64).tolist()
    assert read(os.path.join(out_dir, "model.pt")) == root_model and not os.path.exists(os.path.join(out_dir, "epoch_1"))
    with pytest.raises(ValueError, match="infer_writer"):
        tr.TrainingPipeline(dict(model=_ft_config(spec), batches=[], output_dir=out_dir),
                            tr.FinetuneMode(test_loader=test, infer_only=True, eval_only=True, valid_loader=valid)).run()
