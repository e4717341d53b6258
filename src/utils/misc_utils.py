"""`src.utils.misc_utils` of the reference: checkpoint naming / saving (misc_utils.py:33-49, :105-121), the prediction and inference
dumps with their array codec (:57-66, :254-346), the node-level record dump (:392-469), the variable-length all-gather (:472-504) and
the distributed environment (:507-539)."""
import importlib as _il

_c = _il.import_module("graph-gpt_amd.checkpoint")
_t = _il.import_module("graph-gpt_amd.training")
_i = _il.import_module("graph-gpt_amd.inference")
get_latest_ckp = _c.get_latest_ckp
MODEL_NAME = _c.MODEL_NAME
save_model = _c.save_model
all_gather = _t.all_gather_varlen
set_dist_env = _t.set_dist_env
dump_infer_results = _i.dump_infer_results
save_pred_results = _i.save_pred_results
convert_dict_to_df = _i.convert_dict_to_df
encode_numpy_array = _i.encode_numpy_array
decode_numpy_array = _i.decode_numpy_array
process_data = _i.process_data
dump_results = _i.dump_results

__all__ = ["get_latest_ckp", "MODEL_NAME", "save_model", "all_gather", "set_dist_env", "dump_infer_results", "save_pred_results",
           "convert_dict_to_df", "encode_numpy_array", "decode_numpy_array", "process_data", "dump_results"]
