"""`src.utils.log_eval_dump_utils` of the reference: the inference pass (log_eval_dump_utils.py:41-74), the evaluation passes
(:77-163, :242-304), the contrastive model's embedding pass (:166-194) and the generation evaluation (:308-447)."""
import importlib as _il

_t = _il.import_module("graph-gpt_amd.training")
_g = _il.import_module("graph-gpt_amd.generation")
_i = _il.import_module("graph-gpt_amd.inference")
evaluate = _t.evaluate
ft_evaluate = _t.ft_evaluate
ft_infer_hidden_states = _i.ft_infer_hidden_states
pt_infer_hidden_states = _i.pt_infer_hidden_states
evaluate_generation = _g.evaluate_generation
eval_gen_per_batch = _g.eval_gen_per_batch
eval_gen_per_sample = _g.eval_gen_per_sample

__all__ = ["evaluate", "ft_evaluate", "ft_infer_hidden_states", "pt_infer_hidden_states", "evaluate_generation", "eval_gen_per_batch", "eval_gen_per_sample"]
