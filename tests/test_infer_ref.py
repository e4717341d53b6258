"""Host side of the prediction passes (graph-gpt_amd/inference.py): the NumPy twins the GPU tests compare the kernels with
(tests/_infer_ref.py) are pinned against torch's CPU `.half()` and a torch statement of `process_data`; the dump / save functions and
`process_data` reproduce the reference's output recorded in tests/golden/infer_dump.json (tools/make_golden_infer.py) byte for byte;
`compare_metrics_res` keeps the reference's best-result rule."""
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

import _infer_ref as R
from _util import GOLDEN

inf = importlib.import_module("graph-gpt_amd.inference")
met = importlib.import_module("graph-gpt_amd.metrics")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "infer_dump.json")) as fh:
        return json.load(fh)


def _f16(bits, shape):
    return torch.from_numpy(np.array(bits, dtype=np.int64).astype(np.uint16).view(np.int16).reshape(shape)).view(torch.float16)


# ------------------------------------------------------------------------------------------------ rounding twins
def test_bf16_twin_equals_torch_half_on_every_pattern():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    want = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).half().view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_to_f16_bits(bits)
    assert R.same_f16(got, want), np.argwhere((got != want) & ~R.f16_is_nan(want))[:8]
    assert int(R.f16_is_nan(want).sum()) == 2 * 127               # every bf16 NaN stays a NaN


def test_f32_twin_equals_torch_half_on_curated_and_random_patterns():
    rng = np.random.RandomState(0)
    bits = np.concatenate([R.CURATED_F32.view(np.uint32), rng.randint(0, 2 ** 32, 2 ** 16, dtype=np.uint64).astype(np.uint32)])
    want = torch.from_numpy(bits.view(np.float32)).half().view(torch.int16).numpy().view(np.uint16)
    got = R.f32_to_f16_bits(bits)
    assert R.same_f16(got, want), [(hex(b), hex(g), hex(w)) for b, g, w in zip(bits, got, want) if g != w and not R.f16_is_nan([w])[0]][:8]
    # the curated list, spelled out: the answers themselves, not only agreement
    cur = dict(zip(R.CURATED_F32.tolist(), got[:len(R.CURATED_F32)].tolist()))
    assert cur[2.0 ** -25] == 0x0000 and cur[-2.0 ** -25] == 0x8000 and cur[3 * 2.0 ** -25] == 0x0002 and cur[2.0 ** -24] == 0x0001
    assert cur[2.0 ** -14] == 0x0400 and cur[float(np.float32(2.0 ** -14 - 2.0 ** -25))] == 0x0400
    assert cur[65504.0] == 0x7BFF and cur[float(np.float32(65519.996))] == 0x7BFF and cur[65520.0] == 0x7C00 and cur[-65520.0] == 0xFC00
    assert got[0] == 0x0000 and got[1] == 0x8000 and cur[float("inf")] == 0x7C00 and cur[float("-inf")] == 0xFC00
    assert R.f16_is_nan(got[list(R.CURATED_F32.view(np.uint32)).index(np.float32(np.nan).view(np.uint32))])


# ------------------------------------------------------------------------------------------------ records
def _torch_process_data(logits, raw, idx):
    """process_data's statement, directly (misc_utils.py:444-468)"""
    y = torch.argmax(logits, dim=-1) if logits.dim() == 3 else logits
    flat = raw.reshape(-1)
    keep = torch.where(flat != -100)[0].unique()
    who = np.tile(idx.reshape((-1, 1)), (1, y.shape[1])).reshape(-1)[keep.numpy()]
    return list(zip(who, flat[keep].numpy().astype(int), y.reshape(-1)[keep].numpy().astype(int)))


@pytest.mark.parametrize("shape", [(1, 1, 2), (3, 9, 4), (4, 33, 1), (2, 70, 5)])
def test_record_twin_equals_torch_statement(shape):
    B, S, Cn = shape
    g = torch.Generator().manual_seed(B * 100 + S)
    logits = torch.randn(B, S, Cn, generator=g)
    logits[0, 0, :] = 1.0
    if Cn > 2:
        logits[-1, -1, 1] = float("nan")
        logits[-1, 0, 2] = float("nan")
        logits[-1, 0, 1] = float("nan")
    idx = np.arange(B, dtype=np.int64) * 3 + 2 ** 33
    for density in (0.0, 1.0, 0.34):
        raw = torch.randint(0, 500, (B, S), generator=g)
        raw[torch.rand(B, S, generator=g) >= density] = -100
        raw[-1, -1] = 77
        want = _torch_process_data(logits, raw, idx)
        pred = R.argmax_first(logits.numpy())
        assert np.array_equal(pred, torch.argmax(logits, -1).numpy())
        got = R.node_records(pred, raw.numpy(), idx)
        assert got.tolist() == [[int(a), int(b), int(c)] for a, b, c in want]
        # the package's own torch statement (the CPU path of process_data) and the prediction form
        mine = inf._records_torch(logits, raw, torch.from_numpy(idx))
        assert mine.dtype == torch.int64 and mine.numpy().tolist() == got.tolist()
        assert inf._records_torch(torch.from_numpy(pred), raw, torch.from_numpy(idx)).numpy().tolist() == got.tolist()


class _Stub:
    def __init__(self, out):
        self.out, self.calls, self.device = out, 0, torch.device("cpu")

    def __call__(self, input_ids=None, attention_mask=None, cls_idx=None):
        self.calls += 1
        return types.SimpleNamespace(task_logits=self.out)


def test_process_data_and_dump_results_reproduce_the_reference(golden):
    assert len(golden["records"]) == 4
    for case in golden["records"]:
        B, S, Cn = case["shape"]
        logits = torch.tensor(case["logits"], dtype=torch.float32).reshape(B, S, Cn)
        raw = torch.tensor(case["raw_node_idx"], dtype=torch.int64).reshape(B, S)
        out = logits.argmax(-1) if case["pred_form"] else logits
        for idx in (np.array(case["idx"], dtype=np.int64), torch.tensor(case["idx"], dtype=torch.int64)):
            data = {"input_ids": torch.zeros(B, S, 1, dtype=torch.int64), "attention_mask": torch.ones(B, S, dtype=torch.int64), "idx": idx,
                    "raw_node_idx": raw}
            if case["with_cls"]:
                data["cls_idx"] = torch.zeros(B, dtype=torch.int64)
            model = _Stub(out)
            rec = inf.process_data(model, data, torch.device("cpu"))
            assert isinstance(rec, list) and all(isinstance(r, tuple) and len(r) == 3 for r in rec), case["tag"]
            assert [[int(v) for v in r] for r in rec] == case["records"], case["tag"]
            assert R.node_records(R.argmax_first(logits.numpy()), raw.numpy(), case["idx"]).tolist() == case["records"], case["tag"]
    # dump_results: one writer.write(records, [0, 1, 2]) per batch, in loader order
    written = []
    writer = types.SimpleNamespace(write=lambda records, indices: written.append((list(records), indices)))
    c = golden["records"][0]
    B, S, Cn = c["shape"]
    data = {"input_ids": torch.zeros(B, S, 1, dtype=torch.int64), "attention_mask": torch.ones(B, S, dtype=torch.int64),
            "idx": np.array(c["idx"], dtype=np.int64), "raw_node_idx": torch.tensor(c["raw_node_idx"]).reshape(B, S)}
    n = inf.dump_results(_Stub(torch.tensor(c["logits"]).reshape(B, S, Cn)), [data, data], torch.device("cpu"), writer, slice_id=0)
    assert n == 2 * len(c["records"]) and len(written) == 2 and all(w[1] == [0, 1, 2] for w in written)
    assert [[int(v) for v in r] for r in written[1][0]] == c["records"]
    misc = importlib.import_module("src.utils.misc_utils")
    assert misc.process_data is inf.process_data and misc.dump_results is inf.dump_results


# ------------------------------------------------------------------------------------------------ files
def test_codec_round_trips_and_matches_the_reference(golden):
    assert len(golden["codec"]) == 5
    for case in golden["codec"]:
        arr = np.frombuffer(bytes.fromhex(case["hex"]), dtype=np.dtype(case["dtype"])).reshape(case["shape"])
        enc = inf.encode_numpy_array(arr)
        assert enc == case["encoded"]
        back = inf.decode_numpy_array(enc)
        assert back.dtype == arr.dtype and back.shape == arr.shape and back.tobytes() == arr.tobytes()
    rng = np.random.RandomState(4)
    for dt, shape in ((np.float16, (7,)), (np.float32, (2, 3, 4)), (np.int64, (0,)), (np.uint8, (5, 1))):
        x = (rng.randn(*shape) * 100).astype(dt)
        y = inf.decode_numpy_array(inf.encode_numpy_array(x))
        assert y.dtype == x.dtype and y.shape == x.shape and y.tobytes() == x.tobytes()


def test_dump_infer_results_is_byte_identical(golden, tmp_path, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    assert len(golden["dump"]) == 4
    for k, case in enumerate(golden["dump"]):
        idx = torch.tensor(case["idx"], dtype=torch.int64).view(-1, 1)
        logits = _f16(case["logits_bits"], case["logits_shape"])
        hidden = None if case["hidden_shape"] is None else _f16(case["hidden_bits"], case["hidden_shape"])
        out = tmp_path / f"case{k}"
        paths = inf.dump_infer_results(str(out), case["epoch"], idx=idx, logits=logits, hidden_states=hidden)
        ep = out / f"epoch_{case['epoch']}"
        assert sorted(os.listdir(ep)) == sorted(case["files"]) == sorted(os.path.basename(p) for p in paths), case["tag"]
        for name, text in case["files"].items():
            with open(ep / name, newline="") as fh:
                assert fh.read() == text, (case["tag"], name)
        # the twin's statement of the row format, and the rows decode back to the tensors
        assert R.csv_rows(case["idx"], logits.numpy()) == case["files"]["task_logits_0.csv"], case["tag"]
        if logits.shape[1] > 1:
            rows = [ln.rstrip("\n").split(",") for ln in case["files"]["task_logits_0.csv"].splitlines()]
            assert [int(r[0]) for r in rows] == case["idx"]
            assert np.stack([inf.decode_numpy_array(r[1]) for r in rows]).tobytes() == logits.numpy().tobytes()
    monkeypatch.setenv("RANK", "3")
    inf.dump_infer_results(str(tmp_path / "r3"), 0, idx=torch.tensor([[1]]), logits=torch.ones(1, 2).half())
    assert os.listdir(tmp_path / "r3" / "epoch_0") == ["task_logits_3.csv"]


def test_save_pred_results_is_byte_identical(golden, tmp_path):
    assert len(golden["pred"]) == 2
    for case in golden["pred"]:
        d = {k: torch.tensor(v["values"], dtype=torch.float32).to(getattr(torch, v["dtype"])) for k, v in case["dict"].items()}
        path = inf.save_pred_results(d, str(tmp_path), case["name"])
        assert os.path.basename(path) == f"{case['name']}_results.csv"
        with open(path, newline="") as fh:
            assert fh.read() == case["text"], case["name"]


# ------------------------------------------------------------------------------------------------ best-result rule
def test_compare_metrics_res(golden):
    assert len(golden["compare"]) == 7
    for case in golden["compare"]:
        flag, best = met.compare_metrics_res(case["curr"], case["prev"])
        assert flag is case["flag"] and best == case["best"], case
        assert best is (case["curr"] if flag else case["prev"])
    assert met.compare_metrics_res({"MAE": 0.3}, {"MAE": 0.5})[0] and not met.compare_metrics_res({"valid_loss": 2.0}, {"valid_loss": 1.0})[0]
    assert met.compare_metrics_res({" ACC": 0.0, "EMA F1": 0.6}, {" ACC": 1.0, "EMA F1": 0.5}) == (True, {" ACC": 0.0, "EMA F1": 0.6})
    with pytest.raises(AssertionError):
        met.compare_metrics_res({"a": 1, "b": 2}, {"a": 1, "b": 2})
    assert importlib.import_module("src.utils.metrics_utils").compare_metrics_res is met.compare_metrics_res


def test_ft_infer_hidden_states_on_cpu_tensors_is_the_torch_statement():
    """A model without an engine (CPU tensors): the reference's per-batch .half() and vstack; the config flag and the keyword."""
    g = torch.Generator().manual_seed(1)
    outs = [(torch.randn(b, 3, generator=g) * 300, torch.randn(b, 8, generator=g).bfloat16()) for b in (4, 4, 2)]

    class M:
        device, k, mode = torch.device("cpu"), 0, None

        def eval(self):
            self.mode = "eval"

        def __call__(self, **kw):
            assert "task_labels" not in kw and kw["position_ids"] is not None
            lg, h = outs[self.k]
            self.k += 1
            return types.SimpleNamespace(task_logits=lg, task_hidden_states=h)

    loader = [{"input_ids": torch.zeros(len(lg), 5, 1, dtype=torch.int64), "attention_mask": torch.ones(len(lg), 5, dtype=torch.int64),
               "position_ids": torch.arange(5).expand(len(lg), 5), "idx": torch.arange(len(lg)) + 10 * k} for k, (lg, _) in enumerate(outs)]
    cfg = types.SimpleNamespace(training=types.SimpleNamespace(ft_eval=types.SimpleNamespace(save_hidden_states=True)))
    m = M()
    idx, logits, hidden = inf.ft_infer_hidden_states(m, loader, cfg, "test")
    assert m.mode == "eval" and idx.shape == (10, 1) and idx.view(-1).tolist() == [0, 1, 2, 3, 10, 11, 12, 13, 20, 21]
    assert logits.dtype == hidden.dtype == torch.float16
    assert torch.equal(logits, torch.vstack([o[0].half() for o in outs])) and torch.equal(hidden, torch.vstack([o[1].half() for o in outs]))
    assert R.same_f16(logits.view(torch.int16).numpy().view(np.uint16), R.f32_to_f16_bits(torch.vstack([o[0] for o in outs]).numpy().view(np.uint32)))
    m = M()
    assert inf.ft_infer_hidden_states(m, loader, save_hidden_states=False)[2] is None
    m = M()
    assert inf.ft_infer_hidden_states(m, loader, cfg, save_hidden_states=False)[2] is None        # the keyword replaces the config's flag
    with pytest.raises(ValueError, match="no batch"):
        inf.ft_infer_hidden_states(M(), [])
    assert importlib.import_module("src.utils.log_eval_dump_utils").ft_infer_hidden_states is inf.ft_infer_hidden_states


def test_finetune_mode_reads_the_ft_eval_fields():
    """keyword > training.ft_eval of a reference-shaped config > default; without loaders the mode is the plain step loop"""
    T = importlib.import_module("graph-gpt_amd.training")
    ns = types.SimpleNamespace
    cfg = ns(training=ns(optimizer=ns(), schedule=ns(), ft_eval=ns(epoch_per_eval=3, save_pred=1, save_hidden_states=False, eval_only=0, infer_only=0)))
    m = T.FinetuneMode(batches=[], save_hidden_states=True)
    assert not m.has_eval_loaders and m.allow_resume() and m.allow_save_config()
    m._resolve_ft_eval(cfg)
    assert (m.epoch_per_eval, m.save_pred, m.save_hidden_states, m.eval_only, m.infer_only) == (3, True, True, False, False)
    m = T.FinetuneMode(batches=[], valid_loader=[1], test_loader=[1], eval_only=True)
    m._resolve_ft_eval({"model": None})
    assert (m.epoch_per_eval, m.save_pred, m.eval_only) == (1, False, True) and m.has_eval_loaders
    assert not m.allow_resume() and not m.allow_save_config()
    for bad in (T.FinetuneMode(batches=[], eval_only=True), T.FinetuneMode(batches=[], valid_loader=[1]),
                T.FinetuneMode(batches=[], valid_loader=[1], test_loader=[1], infer_only=True),
                T.FinetuneMode(batches=[], valid_loader=[1], test_loader=[1])):
        with pytest.raises(ValueError, match="FinetuneMode"):
            bad.setup_training(ns(cfg={"model": None}, reference_cfg=False))
