"""Prediction passes: what turns a trained checkpoint into files.

`ft_infer_hidden_states` (reference src/utils/log_eval_dump_utils.py:41-74) runs a loader through a fine-tuned model and returns the
sample indices, the task logits and - on request - the pooled hidden states, all fp16 like the reference's `.half()`.  The reference
keeps a Python list of per-batch tensors and stacks them at the end; here one launch per batch (`gget_op_infer_append`: both
conversions and the index copy) appends to three device arenas, sized from `len(loader.dataset)` when the loader has one and grown by
doubling otherwise.  Nothing is read back inside the loop; the caller's dump makes the one host transfer.

`node_records` / `process_data` / `dump_results` (src/utils/misc_utils.py:392-469) are the node-level dump: every position that is a
node's counted occurrence (`raw_node_idx != -100`) becomes the record (sample idx, raw_node_idx, predicted class).  The reference takes
the arg-max, filters and copies three arrays to the host per batch; `gget_op_node_records` compacts the records on the device in
position order behind a device cursor, and `process_data` makes one host copy of cursor and records together.

`dump_infer_results` / `save_pred_results` (misc_utils.py:322-346, :57-66) and the array codec of the CSV rows (:254-304) write the
files; tests/golden/infer_dump.json pins them byte for byte against the reference's output.

Tensors that live on the CPU (a model without an engine) take the torch statement of the same rules."""
from __future__ import annotations

import base64
import ctypes as C
import json
import os
import time
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .conf import _get
from .training import _layout_kw


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ----------------------------------------------------------------------------- logits / hidden-state collection
def infer_append(logits: torch.Tensor, hidden: Optional[torch.Tensor], idx: torch.Tensor, out_logits: torch.Tensor,
                 out_hidden: Optional[torch.Tensor], out_idx: torch.Tensor, row0: int):
    """`gget_op_infer_append`: logits f32 [B, C], hidden bf16 [B, d] or None and idx i64 [B] into rows row0 .. row0 + B - 1 of the
    arenas out_logits fp16 [cap, C], out_hidden fp16 [cap, d] or None, out_idx i64 [cap]."""
    B, Cn = logits.shape
    assert logits.dtype == torch.float32 and logits.is_contiguous() and idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == B
    assert out_logits.dtype == torch.float16 and out_logits.is_contiguous() and out_logits.shape[1] == Cn
    assert out_idx.dtype == torch.int64 and out_idx.is_contiguous() and out_idx.shape[0] == out_logits.shape[0]
    d = 0
    if hidden is not None:
        d = hidden.shape[1]
        assert hidden.dtype == torch.bfloat16 and hidden.is_contiguous() and hidden.shape[0] == B
        assert out_hidden is not None and out_hidden.dtype == torch.float16 and out_hidden.is_contiguous()
        assert tuple(out_hidden.shape) == (out_logits.shape[0], d)
    L.check(L.load().gget_op_infer_append(_ptr(logits), _ptr(hidden), _ptr(idx), _ptr(out_logits), _ptr(out_hidden if hidden is not None else None),
                                          _ptr(out_idx), int(row0), int(out_logits.shape[0]), B, Cn, d, _stream()))


class _Arenas:
    """The three result arenas of one pass and the host-side row count (B is a shape: no device read is needed to know where the next
    batch goes).  A batch that does not fit doubles them, with a device-to-device copy of the rows in use."""

    def __init__(self, device, n_logits: int, d: int, capacity: int):
        self.device, self.n_logits, self.d, self.rows = device, n_logits, d, 0
        self.logits = self.hidden = self.idx = None
        self._allocate(max(1, int(capacity)))

    def _allocate(self, capacity: int):
        old = (self.logits, self.hidden, self.idx)
        self.logits = torch.empty(capacity, self.n_logits, dtype=torch.float16, device=self.device)
        self.hidden = torch.empty(capacity, self.d, dtype=torch.float16, device=self.device) if self.d else None
        self.idx = torch.empty(capacity, dtype=torch.int64, device=self.device)
        for new, prev in zip((self.logits, self.hidden, self.idx), old):
            if prev is not None and self.rows:
                new[:self.rows].copy_(prev[:self.rows])

    def append(self, logits, hidden, idx):
        B = logits.shape[0]
        cap = self.logits.shape[0]
        if self.rows + B > cap:
            while self.rows + B > cap:
                cap *= 2
            self._allocate(cap)
        infer_append(logits, hidden, idx, self.logits, self.hidden, self.idx, self.rows)
        self.rows += B


def _save_hidden_flag(cfg, save_hidden_states) -> bool:
    if save_hidden_states is not None or cfg is None:
        return bool(save_hidden_states)
    ft_eval = _get(_get(cfg, "training"), "ft_eval")
    return bool(_get(ft_eval, "save_hidden_states", False))


@torch.no_grad()
def ft_infer_hidden_states(model, loader, cfg=None, eval_name: str = "test", *, save_hidden_states: Optional[bool] = None):
    """reference log_eval_dump_utils.ft_infer_hidden_states (:41-74): eval mode, one forward per batch WITHOUT labels, and
    (idx i64 [N, 1], logits fp16 [N, C], hidden fp16 [N, d] or None) on the model's device, in loader order.  Whether the hidden states
    are kept is `cfg.training.ft_eval.save_hidden_states` when a config is given; the keyword replaces it.  The model stays in eval
    mode, as in the reference.  Token-level logits [B, S, C] come back as [N, S, C] (every batch must then share one S, as the
    reference's vstack demands)."""
    save = _save_hidden_flag(cfg, save_hidden_states)
    model.eval()
    device = model.device
    arenas, host, tail = None, [], None
    for data in loader:
        res = model(input_ids=data["input_ids"].to(device), attention_mask=data["attention_mask"].to(device),
                    inputs_raw_embeds=data["embed"].to(device) if "embed" in data else None,
                    position_ids=data["position_ids"].to(device) if "position_ids" in data else None,
                    **({"cls_idx": data["cls_idx"].to(device)} if "cls_idx" in data else {}), **_layout_kw(model, data))
        idx = torch.as_tensor(data["idx"]).to(device=device, dtype=torch.int64).reshape(-1)
        logits, hidden = res.task_logits, (res.task_hidden_states if save else None)
        if tail is None:
            tail = tuple(logits.shape[1:])
        elif tuple(logits.shape[1:]) != tail:
            raise ValueError(f"ft_infer_hidden_states: a batch's logits are [B, {tuple(logits.shape[1:])}], the pass began with [B, {tail}]")
        if not logits.is_cuda:              # no engine behind these tensors: the reference's statement
            host.append((idx.view(-1, 1), logits.half(), hidden.half() if save else None))
            continue
        if logits.dtype != torch.float32 or (save and hidden.dtype != torch.bfloat16):
            raise L.GgetError(f"ft_infer_hidden_states: the collection kernel takes f32 logits and bf16 hidden states, got {logits.dtype}"
                              f"{' / ' + str(hidden.dtype) if save else ''}")
        B = logits.shape[0]
        if arenas is None:
            known = len(loader.dataset) if hasattr(loader, "dataset") and hasattr(loader.dataset, "__len__") else 0
            arenas = _Arenas(device, int(np.prod(tail, dtype=np.int64)) if tail else 1, hidden.shape[1] if save else 0, known or 4 * B)
        arenas.append(logits.reshape(B, -1).contiguous(), hidden.contiguous() if save else None, idx.contiguous())
    if hasattr(model, "check_deferred"):
        model.check_deferred()
    if arenas is None and not host:
        raise ValueError(f"ft_infer_hidden_states: the {eval_name} loader yielded no batch")
    if host:
        return (torch.vstack([h[0] for h in host]), torch.vstack([h[1] for h in host]),
                torch.vstack([h[2] for h in host]) if save else None)
    n = arenas.rows
    return arenas.idx[:n].view(-1, 1), arenas.logits[:n].view(n, *tail), (arenas.hidden[:n] if save else None)


@torch.no_grad()
def pt_infer_hidden_states(model, loader, cfg=None):
    """reference log_eval_dump_utils.pt_infer_hidden_states (:166-194): the embeddings of a contrastively pre-trained model - eval mode,
    one forward per batch without labels (position_ids passed, as there), and (idx i64 [N, 1], head2_logits fp16 [N, d], None) on the
    model's device in loader order; head2_logits is the un-normalised cl_proj output.  Every batch must hold an even number of samples
    (the model pairs them; build the loader with conf.eval_loader_drop_last)."""
    model.eval()
    device = model.device
    ls_idx, ls_logits = [], []
    for data in loader:
        res = model(input_ids=data["input_ids"].to(device), attention_mask=data["attention_mask"].to(device),
                    inputs_raw_embeds=data["embed"].to(device) if "embed" in data else None,
                    position_ids=data["position_ids"].to(device) if "position_ids" in data else None, **_layout_kw(model, data))
        if res.head2_logits is None:
            raise ValueError("pt_infer_hidden_states: the model has no contrastive head (head2_logits is None); build it with "
                             "use_discriminative=True / task_type 'pretrain-cl'")
        ls_idx.append(torch.as_tensor(data["idx"]).to(device=res.head2_logits.device, dtype=torch.int64).view(-1, 1))
        ls_logits.append(res.head2_logits.half())
    if hasattr(model, "check_deferred"):
        model.check_deferred()
    if not ls_idx:
        raise ValueError("pt_infer_hidden_states: the loader yielded no batch")
    return torch.vstack(ls_idx), torch.vstack(ls_logits), None


# ----------------------------------------------------------------------------- node-level records
def append_node_records(out: torch.Tensor, raw_node_idx: torch.Tensor, idx: torch.Tensor, records: torch.Tensor, state: torch.Tensor):
    """`gget_op_node_records` on device tensors: `out` is the model's output, f32 logits [B, S, C] or the predictions [B, S] (any
    integer or float type, truncated like the reference's astype(int)); raw_node_idx i64 [B, S]; idx i64 [B]; records i64 [cap, 3] and
    state i64 [2] = (cursor, records that did not fit) are added to.  A batch of more than `_lib.NODE_RECORDS_MAX_POS` positions is
    handed over in slices of whole samples: the cursor carries the order across them."""
    assert out.dim() in (2, 3), f"logits shape: {tuple(out.shape)}"
    B, S = out.shape[:2]
    assert tuple(raw_node_idx.shape) == (B, S) and idx.numel() == B
    assert records.dtype == torch.int64 and records.is_contiguous() and records.dim() == 2 and records.shape[1] == 3
    assert state.dtype == torch.int64 and state.numel() == 2
    if out.dim() == 3:
        logits, pred, Cn = out.to(torch.float32).contiguous(), None, out.shape[2]
    else:
        logits, pred, Cn = None, out.to(torch.int64).contiguous(), 0
    raw, idx = raw_node_idx.to(torch.int64).contiguous(), idx.to(torch.int64).contiguous()
    lib, rows = L.load(), max(1, L.NODE_RECORDS_MAX_POS // max(S, 1))
    for b0 in range(0, B, rows):
        nb = min(rows, B - b0)
        L.check(lib.gget_op_node_records(_ptr(logits[b0:b0 + nb]) if logits is not None else None,
                                         _ptr(pred[b0:b0 + nb]) if pred is not None else None, _ptr(raw[b0:b0 + nb]), _ptr(idx[b0:b0 + nb]),
                                         _ptr(records), _ptr(state), int(records.shape[0]), nb, S, Cn, _stream()))
    return records, state


def _records_torch(out, raw_node_idx, idx) -> torch.Tensor:
    """The torch statement of misc_utils.py:444-468 on tensors of any device: i64 [n, 3]."""
    assert out.dim() in (2, 3), f"logits shape: {tuple(out.shape)}"
    y = torch.argmax(out, dim=-1) if out.dim() == 3 else out
    raw = raw_node_idx.reshape(-1)
    keep = torch.where(raw != -100)[0]
    who = idx.reshape(-1, 1).expand(-1, y.shape[1]).reshape(-1)
    return torch.stack((who[keep].to(torch.int64), raw[keep].to(torch.int64), y.reshape(-1)[keep].to(torch.int64)), dim=1)


def _node_forward(model, test_data, device):
    out = model(input_ids=test_data["input_ids"].to(device), attention_mask=test_data["attention_mask"].to(device),
                cls_idx=test_data["cls_idx"].to(device) if "cls_idx" in test_data else None, **_layout_kw(model, test_data)).task_logits
    idx = torch.as_tensor(test_data["idx"]).to(device=out.device, dtype=torch.int64).reshape(-1)
    return out, test_data["raw_node_idx"].to(out.device), idx


@torch.no_grad()
def node_records(model, test_data, *, records: Optional[torch.Tensor] = None,
                 state: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The device form of `process_data`: one forward, then the batch's records appended to `records` i64 [cap, 3] behind the cursor
    `state[0]` (both created for this batch - cap = B * S, state zero - when not given).  Returns (records, state); nothing is read
    back.  `state[1]` counts records that did not fit in `cap`."""
    out, raw, idx = _node_forward(model, test_data, model.device)
    if not out.is_cuda:
        raise L.GgetError("node_records is the device form: the model's logits are on the CPU (process_data takes the torch statement there)")
    if records is None:
        records = torch.empty(max(1, raw.numel()), 3, dtype=torch.int64, device=out.device)
    if state is None:
        state = torch.zeros(2, dtype=torch.int64, device=out.device)
    return append_node_records(out, raw, idx, records, state)


@torch.no_grad()
def process_data(model, test_data, device) -> List[tuple]:
    """reference misc_utils.process_data (:426-469): the batch's list of (sample idx, raw_node_idx, predicted class) 3-tuples in
    position order.  `test_data["idx"]` may be a NumPy array (the reference asserts so) or a tensor.  One host copy: the cursor and the
    records travel together."""
    out, raw, idx = _node_forward(model, test_data, device)
    if out.is_cuda:
        records = torch.empty(max(1, raw.numel()) + 1, 3, dtype=torch.int64, device=out.device)     # (row 0 holds the state)
        append_node_records(out, raw, idx, records[1:], records[0, :2].zero_())
        host = records.cpu().numpy()
        n, lost = int(host[0, 0]), int(host[0, 1])
        assert lost == 0, f"{lost} records did not fit an arena sized for every position"
        arr = host[1:1 + n]
    else:
        arr = _records_torch(out, raw, idx).numpy()
    return list(zip(arr[:, 0], arr[:, 1], arr[:, 2]))


@torch.no_grad()
def dump_results(model, loader, device, writer, slice_id, epoch=1, ds_split="test"):
    """reference misc_utils.dump_results (:392-423): every batch's records go to `writer.write(records, [0, 1, 2])` (the reference's
    writer is an ODPS table writer; any object with that method does), with a progress line every 10000 records.  Returns the number of
    records written."""
    t0 = t_last = time.time()
    done = reported = 0
    for test_data in loader:
        records = process_data(model, test_data, device)
        done += len(records)
        if done // 10000 > reported // 10000:
            now = time.time()
            print(f"[{slice_id}][epoch {epoch}][{ds_split}] {done} records, {(done - reported) / max(now - t_last, 1e-9):.0f} records/s "
                  f"({done / max(now - t0, 1e-9):.0f} records/s over the pass)")
            t_last, reported = now, done
        writer.write(records, [0, 1, 2])
    return done


# ----------------------------------------------------------------------------- files
def encode_numpy_array(arr: np.ndarray) -> str:
    """reference misc_utils.encode_numpy_array (:254-278): {"dtype", "shape", "data": base64 of the raw bytes} as JSON, the whole
    URL-safe base64 encoded - one CSV field without a comma in it."""
    inner = base64.b64encode(arr.tobytes()).decode("ascii")
    text = json.dumps({"dtype": str(arr.dtype), "shape": arr.shape, "data": inner})
    return base64.urlsafe_b64encode(text.encode("utf-8")).decode("ascii")


def decode_numpy_array(encoded_str: str) -> np.ndarray:
    """The inverse (reference :281-304): a read-only array over the decoded bytes."""
    payload = json.loads(base64.urlsafe_b64decode(encoded_str.encode("ascii")).decode("utf-8"))
    raw = base64.b64decode(payload["data"].encode("ascii"))
    return np.frombuffer(raw, dtype=np.dtype(payload["dtype"])).reshape(tuple(payload["shape"]))


def _format_infer_results(idx: torch.Tensor, tensor: torch.Tensor) -> List[str]:
    """reference :307-319: one "idx,value" line per sample; a single column is written as the number itself, anything wider encoded."""
    idx = idx.reshape(-1)
    plain = tensor.size(1) == 1
    if plain:
        tensor = tensor.reshape(-1)
    assert idx.size(0) == tensor.size(0), f"{idx.size(0)} != {tensor.size(0)}"
    rows = zip(idx.cpu().numpy(), tensor.cpu().numpy())        # (the pass's one host transfer per tensor)
    return [f"{i},{t if plain else encode_numpy_array(t)}\n" for i, t in rows]


def dump_infer_results(output_dir, epoch, *, idx: Optional[torch.Tensor] = None, logits: Optional[torch.Tensor] = None,
                       hidden_states: Optional[torch.Tensor] = None):
    """reference misc_utils.dump_infer_results (:322-346): <output_dir>/epoch_<epoch>/task_logits_<RANK>.csv and, when there are hidden
    states, hidden_states_<RANK>.csv.  Returns the paths written."""
    ckp_dir = os.path.join(output_dir, f"epoch_{epoch}")
    os.makedirs(ckp_dir, exist_ok=True)
    rank = int(os.environ.get("RANK", 0))
    written = []
    todo = [("task_logits", logits)]
    if hidden_states is not None and hidden_states.numel() > 0:
        todo.append(("hidden_states", hidden_states))
    for stem, tensor in todo:
        path = os.path.join(ckp_dir, f"{stem}_{rank}.csv")
        with open(path, "w") as fh:
            fh.writelines(_format_infer_results(idx, tensor))
        written.append(path)
    return written


def convert_dict_to_df(dict_):
    """reference :57-59: every tensor of the triplet as a float32 column."""
    import pandas as pd
    return pd.DataFrame({key: val.float().detach().cpu().numpy() for key, val in dict_.items()})


def save_pred_results(dict_, model_dir, name):
    """reference misc_utils.save_pred_results (:62-66): the prediction triplet of `ft_evaluate` as <model_dir>/<name>_results.csv."""
    path = os.path.join(model_dir, f"{name}_results.csv")
    convert_dict_to_df(dict_).to_csv(path, index=False)
    return path
