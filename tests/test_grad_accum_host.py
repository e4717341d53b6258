"""Host side of gradient accumulation: the two keys optimizer.pt gained (`micro_steps`, and `grad_acc` inside a window) - written by
checkpoint.optimizer_state, read by checkpoint.read_accumulation - for files of both layouts.  No GPU."""
import importlib

import pytest
import torch

CK = importlib.import_module("graph-gpt_amd.checkpoint")
NAMES = ["model.embed_tokens.weight", "model.norm.weight"]


def _moments():
    return {n: torch.full((3,), float(i)) for i, n in enumerate(NAMES)}, {n: torch.full((3,), 10.0 + i) for i, n in enumerate(NAMES)}


def test_state_at_a_boundary_carries_the_count_and_no_sum(tmp_path):
    m, v = _moments()
    st = CK.optimizer_state(m, v, step=4, global_steps=5, ema_updates=10, micro_steps=10)
    assert set(st) == {"m", "v", "step", "global_steps", "ema_updates", "micro_steps"}
    torch.save(st, tmp_path / "optimizer.pt")
    back = torch.load(tmp_path / "optimizer.pt", map_location="cpu")
    assert CK.read_accumulation(back, 2, NAMES) == (10, None, 0)
    assert back["step"] == 4 and back["global_steps"] == 5 and back["ema_updates"] == 10
    assert torch.equal(back["m"][NAMES[1]], m[NAMES[1]])


def test_state_inside_a_window_round_trips_the_partial_sum(tmp_path):
    m, v = _moments()
    acc = {n: torch.tensor([1.0 + 2.0 ** -20, -3.0, 2.0 ** -18], dtype=torch.float32) for n in NAMES}      # (not bf16 values)
    st = CK.optimizer_state(m, v, 2, 2, micro_steps=7, grad_acc=acc)
    assert set(st) - {"m", "v", "step", "global_steps", "ema_updates"} == {"micro_steps", "grad_acc"}
    torch.save(st, tmp_path / "optimizer.pt")
    back = torch.load(tmp_path / "optimizer.pt", map_location="cpu")
    micro, got, n = CK.read_accumulation(back, 3, NAMES)
    assert micro == 7 and n == 1                       # the seventh micro-step is the first of the third window of k = 3
    assert set(got) == set(NAMES) and all(got[k].dtype == torch.float32 and torch.equal(got[k], acc[k]) for k in NAMES)
    assert CK.read_accumulation(back, 4, NAMES)[2] == 3
    with pytest.raises(ValueError, match="gradient_accumulation_steps"):
        CK.read_accumulation(back, 7, NAMES)           # k = 7 would have stepped at micro-step 7: no window to continue
    with pytest.raises(KeyError):
        CK.read_accumulation(back, 3, NAMES + ["lm_head.weight"])


def test_a_file_of_the_earlier_layout_loads_without_a_window():
    m, v = _moments()
    old = {"m": m, "v": v, "step": 3, "global_steps": 3, "ema_updates": 0}
    assert CK.read_accumulation(old, 1, NAMES) == (0, None, 0)
    assert CK.read_accumulation(old, 4, NAMES) == (0, None, 0)
    oldest = {"m": m, "v": v, "step": 3, "global_steps": 3}         # (before the EMA key)
    assert CK.read_accumulation(oldest, 2) == (0, None, 0)
    with pytest.raises(ValueError):
        CK.read_accumulation(dict(old, grad_acc={}), 2)             # a sum without its count is not a file this project wrote
