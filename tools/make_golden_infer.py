#!/usr/bin/env python3
"""Generate tests/golden/infer_dump.json by importing the REAL reference's src/utils/misc_utils.py and metrics_utils.py, in the manner
of tools/make_golden_gen_eval.py (build container only; the fixture holds tensors in and file contents / records out, none of the
reference's text).

    dump      dump_infer_results (misc_utils.py:322-346): idx i64 [N,1], logits fp16 [N,C] and hidden fp16 [N,d] (stored as their bit
              patterns) -> the text of epoch_k/task_logits_0.csv and hidden_states_0.csv.  C = 1 takes the plain-number row, C > 1
              the encoded row; hidden None / empty writes no second file.
    codec     encode_numpy_array (:254-278) on arrays of several dtypes and shapes -> the strings.
    pred      save_pred_results (:62-66): a triplet dict -> the text of <name>_results.csv.
    records   process_data (:426-469) for seeded batches against a stub model that returns fixed logits ([B,S,C], and the [B,S]
              prediction form) -> the list of (idx, raw_node_idx, class) records.
    compare   compare_metrics_res (metrics_utils.py:192-208) on the mae / loss / ema-key cases -> (flag, kept result).

    python tools/make_golden_infer.py
"""
import importlib
import importlib.machinery
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("GGET_REFERENCE", "/root/reference")


def import_reference_utils():
    """misc_utils and metrics_utils of the reference without `src.utils.__init__` (which pulls the whole training stack): the packages
    are bare, and what the two modules import at their top and the fixture never calls (deepspeed, torchmetrics, the config package)
    is stubbed."""
    sys.path.insert(0, REF)

    class _Stub(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return sys.modules.get(self.__name__ + "." + name) or type(name, (), {"__init__": lambda self, *a, **k: None})

    def stub(name):
        parts = name.split(".")
        for i in range(1, len(parts) + 1):
            n = ".".join(parts[:i])
            if n not in sys.modules:
                m = _Stub(n)
                m.__path__ = []
                m.__spec__ = importlib.machinery.ModuleSpec(n, None, is_package=True)
                sys.modules[n] = m

    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    for name, path in (("src", REF + "/src"), ("src.utils", REF + "/src/utils")):
        m = types.ModuleType(name)
        m.__path__ = [path]
        m.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
        sys.modules[name] = m
    for n in ["deepspeed", "torcheval", "torchmetrics", "torchmetrics.classification", "src.conf", "ogb", "ogb.graphproppred", "ogb.linkproppred",
              "ogb.nodeproppred", "ogb.lsc", "sklearn", "sklearn.metrics"]:
        try:
            importlib.import_module(n)
        except Exception:
            stub(n)
    misc = importlib.import_module("src.utils.misc_utils")
    try:
        met = importlib.import_module("src.utils.metrics_utils")
    except Exception as ex:          # (a top-level statement the stubs do not carry: the compare cases are then left out, and said so)
        print("metrics_utils not importable:", repr(ex))
        met = None
    return misc, met


def bits(t):
    return t.contiguous().view(torch.int16).numpy().astype(np.int64).reshape(-1).tolist()


def dump_case(misc, tag, epoch, idx, logits, hidden):
    with tempfile.TemporaryDirectory() as d:
        misc.dump_infer_results(d, epoch, idx=idx, logits=logits, hidden_states=hidden)
        files = {}
        for fn in sorted(os.listdir(os.path.join(d, f"epoch_{epoch}"))):
            with open(os.path.join(d, f"epoch_{epoch}", fn), newline="") as fh:
                files[fn] = fh.read()
    return {"tag": tag, "epoch": epoch, "idx": idx.reshape(-1).tolist(), "logits_shape": list(logits.shape), "logits_bits": bits(logits),
            "hidden_shape": None if hidden is None else list(hidden.shape), "hidden_bits": None if hidden is None else bits(hidden),
            "files": files}


class StubModel:
    """What process_data needs of a model: a call that takes the three keywords and returns `.task_logits`."""

    def __init__(self, out):
        self.out, self.calls = out, []

    def __call__(self, input_ids=None, attention_mask=None, cls_idx=None):
        self.calls.append((tuple(input_ids.shape), tuple(attention_mask.shape), cls_idx is not None))
        return types.SimpleNamespace(task_logits=self.out)


def records_case(misc, tag, B, S, C, seed, density, with_cls, pred_form=False):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, S, C, generator=g)
    if C > 1:
        logits[0, 0, :] = 0.5                      # a full tie: the first class
        logits[-1, -1, C - 1] = logits[-1, -1, 0]  # a two-way tie
    raw = torch.randint(0, 1000, (B, S), generator=g)
    raw[torch.rand(B, S, generator=g) >= density] = -100
    idx = np.arange(B, dtype=np.int64) * 7 + 3_000_000_000
    out = logits.argmax(-1) if pred_form else logits
    data = {"input_ids": torch.zeros(B, S, 1, dtype=torch.int64), "attention_mask": torch.ones(B, S, dtype=torch.int64), "idx": idx,
            "raw_node_idx": raw}
    if with_cls:
        data["cls_idx"] = torch.zeros(B, dtype=torch.int64)
    model = StubModel(out)
    rec = misc.process_data(model, data, torch.device("cpu"))
    assert model.calls == [((B, S, 1), (B, S), with_cls)]
    return {"tag": tag, "shape": [B, S, C], "pred_form": pred_form, "with_cls": with_cls, "logits": logits.reshape(-1).tolist(),
            "raw_node_idx": raw.reshape(-1).tolist(), "idx": idx.tolist(), "records": [[int(a), int(b), int(c)] for a, b, c in rec]}


def main():
    misc, met = import_reference_utils()
    g = torch.Generator().manual_seed(20)
    res = {"dump": [], "codec": [], "pred": [], "records": [], "compare": []}
    mk = lambda *s: (torch.randn(*s, generator=g) * 3).half()      # noqa: E731
    idx5 = torch.tensor([[4], [0], [3_000_000_000], [7], [-2]], dtype=torch.int64)
    special = torch.tensor([[0.0], [-0.0], [65504.0], [float("inf")], [6e-8]]).half()
    res["dump"].append(dump_case(misc, "one logit, no hidden", 0, idx5, special, None))
    res["dump"].append(dump_case(misc, "three logits, hidden", 3, idx5, mk(5, 3), mk(5, 8)))
    res["dump"].append(dump_case(misc, "128 logits, empty hidden", 1, idx5[:2], mk(2, 128), torch.zeros(0, 8).half()))
    res["dump"].append(dump_case(misc, "two logits, one hidden column", 12, idx5[:3], mk(3, 2), mk(3, 1)))
    for arr in (np.arange(6, dtype=np.float16).reshape(2, 3) / 7, np.array([1.5, -2.25], np.float32), np.array([], np.float16),
                np.array([[3_000_000_000, -1]], np.int64), np.float16(0.333) * np.ones((), np.float16)):
        enc = misc.encode_numpy_array(arr)
        back = misc.decode_numpy_array(enc)
        assert back.dtype == arr.dtype and back.shape == arr.shape and back.tobytes() == arr.tobytes()
        res["codec"].append({"dtype": str(arr.dtype), "shape": list(arr.shape), "hex": arr.tobytes().hex(), "encoded": enc})
    trip = {"y_true": torch.tensor([1, 0, 1, 1]), "y_pred": torch.tensor([0.25, -1.5, 3.1415927, 1e-9]), "idx": torch.tensor([10, 11, 12, 16777217])}
    trip2 = {"y_true": torch.tensor([0.5, float("nan")]), "y_pred": torch.tensor([0.1, 0.2]).bfloat16(), "idx": torch.tensor([0, 1])}
    for name, t in (("valid", trip), ("test", trip2)):
        with tempfile.TemporaryDirectory() as d:
            misc.save_pred_results(t, d, name)
            with open(os.path.join(d, f"{name}_results.csv"), newline="") as fh:
                text = fh.read()
        res["pred"].append({"name": name, "text": text,
                            "dict": {k: {"dtype": str(v.dtype).replace("torch.", ""), "values": v.float().tolist()} for k, v in t.items()}})
    res["records"].append(records_case(misc, "third", 3, 9, 4, 5, 0.34, False))
    res["records"].append(records_case(misc, "all, with cls_idx", 2, 5, 3, 6, 2.0, True))
    res["records"].append(records_case(misc, "none", 2, 4, 2, 7, -1.0, False))
    res["records"].append(records_case(misc, "predictions given", 3, 6, 5, 8, 0.5, False, pred_form=True))
    if met is not None:
        cases = [({"MAE": 0.3}, {"MAE": 0.5}), ({"MAE": 0.5}, {"MAE": 0.3}), ({"valid_loss": 1.0}, {"valid_loss": 1.0}),
                 ({"rocauc": 0.8}, {"rocauc": 0.7}), ({"rocauc": 0.7}, {"rocauc": 0.7}),
                 ({" ACC": 0.1, " Recall": 0.9, "EMA F1": 0.6}, {" ACC": 0.9, " Recall": 0.1, "EMA F1": 0.5}),
                 ({" ACC": 0.9, "ema mae": 0.6}, {" ACC": 0.1, "ema mae": 0.5})]
        for cur, prev in cases:
            flag, best = met.compare_metrics_res(cur, prev)
            res["compare"].append({"curr": cur, "prev": prev, "flag": bool(flag), "best": best})
    out = os.path.join(ROOT, "tests", "golden", "infer_dump.json")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("infer_dump written:", os.path.getsize(out), "bytes;", {k: len(v) for k, v in res.items()})


if __name__ == "__main__":
    main()
