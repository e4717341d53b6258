"""`src.utils.modules_utils` of the reference, the part the fine-tune pipeline calls after the model exists: `freeze_llama_layers`
(modules_utils.py:45-54) and - for callers that import it from here - `print_trainable_parameters` (inspection_utils.py:13-32)."""
import importlib as _il

_m = _il.import_module("graph-gpt_amd.modeling")
freeze_llama_layers = _m.freeze_llama_layers
print_trainable_parameters = _m.print_trainable_parameters

__all__ = ["freeze_llama_layers", "print_trainable_parameters"]
