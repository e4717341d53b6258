"""`src.utils.generation_utils` of the reference: the unmasking samplers and the accuracy of their output
(generation_utils.py:84-237, :317-463)."""
import importlib as _il

_g = _il.import_module("graph-gpt_amd.generation")
sample_per_batch = _g.sample_per_batch
sample_per_example = _g.sample_per_example
cal_gen_acc_per_sample = _g.cal_gen_acc_per_sample
cal_gen_acc_batch = _g.cal_gen_acc_batch

__all__ = ["sample_per_batch", "sample_per_example", "cal_gen_acc_per_sample", "cal_gen_acc_batch"]
