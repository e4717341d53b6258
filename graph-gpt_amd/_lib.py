"""ctypes binding of libgget_hip.so (C ABI: include/gget.h).  There is NO CPU fallback: if the
library is missing or does not load, importing the engine raises."""
from __future__ import annotations

import contextlib
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GGET_LIB_PATH") or os.path.join(HERE, "lib", "libgget_hip.so")   # override: A/B builds in one run

i32, i64, u64, f32, vp, cp = C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_void_p, C.c_char_p


class GgetConfig(C.Structure):
    _fields_ = [(n, i32) for n in ("kind", "vocab_size", "hidden_size", "intermediate_size", "num_layers", "num_heads",
                                   "stacked_feat", "next_n_token", "gated_agg", "causal", "max_position", "num_labels",
                                   "score_bias", "pad_token_id")] + \
               [("rms_eps", f32), ("rope_theta", f32), ("layer_scale_init", f32), ("max_tokens", i32), ("max_batch", i32),
                ("path_pdrop", f32), ("mlp_pdrop", f32), ("head_mlp_layers", i32), ("head_mlp", i32 * 4), ("embed_dim", i32)]


class GgetSizes(C.Structure):
    _fields_ = [(n, u64) for n in ("n_params", "param_bf16_bytes", "master_bytes", "adam_bytes", "grad_bf16_bytes",
                                   "workspace_bytes")]


class GgetBuffers(C.Structure):
    _fields_ = [(n, vp) for n in ("param_bf16_dev", "master_dev", "adam_m_dev", "adam_v_dev", "grad_bf16_dev",
                                  "workspace_dev", "rope_cos_dev", "rope_sin_dev")]


class GgetParamInfo(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("ndim", i32), ("shape", i64 * 2), ("offset", u64), ("layer", i32)]


class GgetGroupItem(C.Structure):
    """gget_group_item_t: one work item of a grouped optimizer step (gget_group_plan)"""
    _fields_ = [("off", u64), ("cnt", u64), ("lr_scale", f32), ("wd_scale", f32)]


# name -> (restype, argtypes); every symbol declared in include/gget.h
SIGNATURES = {
    "gget_last_error": (cp, []),
    "gget_version": (i32, []),
    "gget_query_sizes": (i32, [C.POINTER(GgetConfig), C.POINTER(GgetSizes)]),
    "gget_create": (i32, [C.POINTER(GgetConfig), C.POINTER(GgetBuffers), C.POINTER(vp)]),
    "gget_destroy": (i32, [vp]),
    "gget_param_count": (i32, [vp]),
    "gget_param_info": (i32, [vp, i32, C.POINTER(GgetParamInfo)]),
    "gget_bucket_count": (i32, [vp]),
    "gget_bucket_range": (i32, [vp, i32, C.POINTER(u64), C.POINTER(u64)]),
    "gget_sync_params": (i32, [vp, vp]),
    "gget_grad_acc_attach": (i32, [vp, vp]),
    "gget_grad_accumulate": (i32, [vp, vp]),
    "gget_grad_acc_count": (i32, [vp, C.POINTER(i32)]),
    "gget_grad_acc_set_count": (i32, [vp, i32]),
    "gget_set_frozen": (i32, [vp, i32]),
    "gget_trainable_ranges": (i32, [vp, vp, vp]),
    "gget_bucket_train_range": (i32, [vp, i32, C.POINTER(u64), C.POINTER(u64)]),
    "gget_ema_attach": (i32, [vp, vp]),
    "gget_set_ema_decay": (i32, [vp, f32]),
    "gget_ema_update": (i32, [vp, f32, vp]),
    "gget_ema_to_params": (i32, [vp, vp]),
    "gget_forward_pretrain": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]),
    "gget_forward_pretrain_packed": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]),
    "gget_forward_task": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "gget_backward": (i32, [vp, f32, vp]),
    "gget_backward_begin": (i32, [vp, f32, vp]),
    "gget_backward_layer": (i32, [vp, i32, vp]),
    "gget_backward_end": (i32, [vp, vp]),
    "gget_adamw_step": (i32, [vp, f32, f32, f32, f32, f32, f32, f32, i32, vp, vp]),
    "gget_comm_unique_id": (i32, [vp]),
    "gget_comm_init": (i32, [vp, i32, i32, vp]),
    "gget_comm_destroy": (i32, [vp]),
    "gget_comm_move": (i32, [vp, vp]),
    "gget_allreduce_grads_async": (i32, [vp, i32, i32, vp]),
    "gget_allreduce_range_async": (i32, [vp, u64, u64, i32, vp]),
    "gget_comm_init_loopback": (i32, [vp, i32]),
    "gget_shard_plan": (i32, [C.POINTER(GgetConfig), i32, i32, C.POINTER(u64)]),
    "gget_shard_init": (i32, [vp, i32, i32, C.POINTER(i32)]),
    "gget_shard_bucket": (i32, [vp, i32, C.POINTER(u64)]),
    "gget_reduce_scatter_grads_async": (i32, [vp, i32, i32, vp]),
    "gget_shard_sqnorm_partials": (i32, [vp, vp, vp]),
    "gget_shard_allgather_async": (i32, [vp, i32, vp, vp]),
    "gget_adamw_step_sharded": (i32, [vp, f32, f32, f32, f32, f32, f32, f32, i32, vp, vp, vp]),
    "gget_set_param_scales": (i32, [vp, C.POINTER(f32), C.POINTER(f32), i32]),
    "gget_param_scales": (i32, [vp, C.POINTER(f32), C.POINTER(f32), i32]),
    "gget_plan_param_count": (i32, [C.POINTER(GgetConfig)]),
    "gget_plan_param_info": (i32, [C.POINTER(GgetConfig), i32, C.POINTER(GgetParamInfo)]),
    "gget_group_plan": (i32, [C.POINTER(GgetConfig), C.POINTER(f32), C.POINTER(f32), i32, i32, i32, i32, C.POINTER(GgetGroupItem), i32,
                              C.POINTER(i32)]),
    "gget_head_counts": (i32, [vp, C.POINTER(i32 * 2), vp]),
    "gget_head_logits": (i32, [vp, C.POINTER(vp), C.POINTER(i32)]),
    "gget_hidden_states": (i32, [vp, C.POINTER(vp)]),
    "gget_layer_hidden_states": (i32, [vp, i32, C.POINTER(vp)]),
    "gget_hidden_states_grid": (i32, [vp, i32, vp, vp]),
    "gget_attention_probs": (i32, [vp, i32, vp, i32, vp]),
    "gget_layer_qkv_grid": (i32, [vp, i32, vp, vp]),
    "gget_op_attn_probs": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, C.c_uint32, vp]),
    "gget_op_gemm": (i32, [i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "gget_op_gemm_streamk": (i32, [i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
    "gget_op_gemm_streamk_bytes": (u64, []),
    "gget_debug_set": (i32, [i32, i32]),
    "gget_debug_get": (i32, [i32, C.POINTER(i32)]),
    "gget_debug_occupy": (i32, [vp, u64, i32, i32, i32, vp]),
    "gget_op_gemm_grouped": (i32, [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "gget_op_rmsnorm_fwd": (i32, [vp, vp, vp, vp, i32, i32, f32, vp]),
    "gget_op_rmsnorm_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]),
    "gget_op_embed_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "gget_op_embed_bwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "gget_op_qkv_rope": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "gget_op_smtp2d": (i32, [vp, i32, vp, i32, vp, vp, i32, i32, i32, f32, f32, f32, i32, i32, C.c_uint32, vp]),
    "gget_op_token_sample": (i32, [vp, i32, i32, i32, i32, f32, f32, i32, f32, C.c_uint32, vp, vp, vp]),
    "gget_op_token_sample_probs": (i32, [vp, i32, i32, i32, i32, f32, f32, i32, f32, C.c_uint32, vp, vp, vp, i32, vp]),
    "gget_op_unmask_origin": (i32, [vp, vp, i32, i32, f32, C.c_uint32, i32, vp]),
    "gget_op_unmask_origin_rows": (i32, [vp, vp, i32, i32, vp, C.c_uint32, i32, vp]),
    "gget_op_unmask_ranked": (i32, [vp, vp, vp, i32, i32, i32, vp, i32, vp, vp]),
    "gget_op_gen_plan": (i32, [vp, i32, i32, i32, vp, i32, vp, vp, vp, vp]),
    "gget_op_gen_acc": (i32, [vp, vp, vp, i32, i32, i32, vp, vp]),
    "gget_op_token_confidence": (i32, [vp, i32, i32, i32, i32, vp, vp, vp]),
    "gget_op_smtp_rows": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, C.c_double, C.c_double, C.c_double, C.c_uint32, vp]),
    "gget_op_rope": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "gget_op_attn_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, f32, C.c_uint32, vp]),
    "gget_op_attn_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, f32, C.c_uint32, vp]),
    "gget_op_rope_hd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "gget_op_rope_f32_hd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "gget_op_attn_fwd_hd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, C.c_uint32, vp]),
    "gget_op_attn_bwd_hd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, f32, C.c_uint32, vp]),
    "gget_op_attn_probs_hd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, C.c_uint32, vp]),
    "gget_op_copy_from_host": (i32, [vp, vp, C.c_uint64, vp]),
    "gget_op_attn_fwd_varlen": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, f32, C.c_uint32, vp]),
    "gget_op_attn_bwd_varlen": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, f32, C.c_uint32, vp]),
    "gget_op_attn_oproj_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, C.c_uint32, vp, vp]),
    "gget_op_pack_wo": (i32, [vp, C.c_uint64, vp, vp, i32, i32, vp]),
    "gget_op_attn_oproj_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, C.c_uint64, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, f32,
                                      C.c_uint32, i32, vp, vp, vp]),
    "gget_op_attn_bwd_varlen_list": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, f32, C.c_uint32, vp, vp]),
    "gget_op_attn_oproj_bwd_list": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, C.c_uint64, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp,
                                           f32, C.c_uint32, i32, vp, vp, vp, vp]),
    "gget_op_attn_fwd_ranges": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, C.c_uint32, vp]),
    "gget_op_attn_bwd_ranges": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, C.c_uint32, vp]),
    "gget_op_ranges_from_mask3d": (i32, [vp, vp, vp, i32, i32, vp]),
    "gget_op_attn_bwd_fused": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, C.c_uint32, vp]),
    "gget_set_dropout": (i32, [vp, f32, f32, C.c_uint32]),
    "gget_set_auc": (i32, [vp, i32, C.c_uint32]),
    "gget_set_token_count": (i32, [vp, C.c_int64]),
    "gget_set_option": (i32, [vp, i32, i32]),
    "gget_set_dp_menu": (i32, [vp, i32, i32]),
    "gget_varlen_status": (i32, [vp, vp, vp]),
    "gget_position_status": (i32, [vp, vp, vp]),
    "gget_deferred_status": (i32, [vp, vp, vp]),
    "gget_set_focal_gamma": (i32, [vp, f32]),
    "gget_set_stack_method": (i32, [vp, i32]),
    "gget_set_rope_range": (i32, [vp, f32]),
    "gget_set_raw_embeds": (i32, [vp, vp, i32]),
    "gget_debug_probe": (i32, [vp, i32, C.POINTER(f32)]),
    "gget_debug_gemm_probe": (i32, [i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(i32)]),
    "gget_set_dropout_ex": (i32, [vp, f32, f32, f32]),
    "gget_op_gateup_geglu": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "gget_op_down_dgrad_geglu": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "gget_op_geglu_fwd": (i32, [vp, vp, i32, i32, vp]),
    "gget_op_geglu_bwd": (i32, [vp, vp, vp, i32, i32, vp]),
    "gget_op_ce_fwd_bwd": (i32, [vp, i32, vp, vp, vp, i32, i32, vp, vp, f32, i32, vp]),
    "gget_op_rmsnorm_bwd_copies": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, u64, vp]),
    "gget_op_rmsnorm_dw": (i32, [vp, vp, vp, vp, i32, i32, i32, u64, vp]),
    "gget_op_ls_rmsnorm_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp]),
    "gget_op_accum_layout": (i32, [i32, C.POINTER(i32), C.POINTER(u64)]),
    "gget_op_rmsnorm_bwd_ls": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]),
    # masks on: (elem_p, elem_seed, elem_rows) and, for the residual kernels, (path_rate, path_seed, path_S, path_row_b) before the stream
    "gget_op_ls_rmsnorm_fwd_drop": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, C.c_uint32, vp, f32, C.c_uint32, i32, vp, vp]),
    "gget_op_rmsnorm_bwd_ls_drop": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, C.c_uint32, vp, f32, C.c_uint32, i32, vp, vp]),
    "gget_op_ls_fwd": (i32, [vp, vp, vp, vp, i32, i32, f32, C.c_uint32, vp, f32, C.c_uint32, i32, vp, vp]),
    "gget_op_ls_bwd": (i32, [vp, vp, vp, vp, vp, i32, i32, f32, C.c_uint32, vp, f32, C.c_uint32, i32, vp, vp]),
    "gget_op_elem_dropout": (i32, [vp, i64, i32, C.c_uint32, f32, C.c_uint32, vp, vp]),
    "gget_op_embed_fwd_drop": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32, C.c_uint32, vp, vp]),
    "gget_op_embed_bwd_drop": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, C.c_uint32, vp, vp]),
    "gget_op_head_linear_fwd_drop": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, C.c_uint32, vp, vp]),
    "gget_op_head_linear_bwd_drop": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, C.c_uint32, vp, vp]),
    "gget_op_rope_table": (i32, [vp, vp, i32, f32, vp]),
    "gget_op_rope_range_table": (i32, [vp, vp, vp, vp, i32, i32, f32, f32, vp]),
    "gget_op_clamp_positions": (i32, [vp, vp, vp, i64, i32, vp]),
    "gget_op_embed_long_ratio": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "gget_op_ce_full": (i32, [vp, i32, vp, vp, vp, i32, vp, i32, i32, vp, vp, f32, i32, vp, f32, vp, i32, vp]),
    "gget_op_score_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "gget_op_score_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "gget_op_tok_score_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "gget_op_tok_intra_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "gget_op_tok_intra_bwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "gget_set_cls_idx": (i32, [vp, vp]),
    "gget_op_tok_ce": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, i32, vp]),
    "gget_op_tok_score_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "gget_op_task_loss": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "gget_op_auc_loss": (i32, [vp, vp, i32, i32, i32, C.c_uint32, vp, vp, vp, vp]),
    "gget_op_pool_rows": (i32, [vp, vp, vp, i32, i32, vp]),
    "gget_op_scatter_rows_f32": (i32, [vp, vp, vp, i32, i32, vp]),
    "gget_op_head_linear_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "gget_op_head_linear_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "gget_op_lengths": (i32, [vp, vp, i32, i32, vp, vp, i32, i32, vp]),
    "gget_op_sum_lengths": (i32, [vp, i32, vp, vp]),
    "gget_op_varlen_plan": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    "gget_op_rows_to_grid": (i32, [vp, vp, vp, i64, i32, vp]),
    "gget_op_head_compact_ws_bytes": (u64, [i32]),
    "gget_op_head_compact": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "gget_op_head_slot_sort": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i64, i32, vp]),
    "gget_op_head_cell_sum": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "gget_op_gather_rows": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "gget_op_gather_rows_remap": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "gget_op_sample_mask_wgt": (i32, [vp, vp, i32, i32, vp]),
    "gget_op_raw_blend": (i32, [vp, vp, i32, i32, vp, vp, vp, i32, i32, vp, i32, vp]),
    "gget_op_raw_tok_grad": (i32, [vp, vp, vp, i32, i32, vp]),
    "gget_op_gemm_indexed": (i32, [i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp]),
    "gget_op_gemm_dyn": (i32, [i32, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp]),
    "gget_op_gemm_grouped_slab": (i32, [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp]),
    "gget_op_slab_reduce": (i32, [vp, i64, i32, vp, u64, i32, vp]),
    "gget_op_slab_plan": (i32, [i32, i32, i32, i32, C.POINTER(i32)]),
    "gget_op_attn_bwd_rotated": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, f32, C.c_uint32, vp, u64, vp, vp]),
    "gget_op_convert_segments": (i32, [vp, vp, vp, i32, vp]),
    "gget_op_rank_metrics_workspace": (C.c_size_t, [i32, i32]),
    "gget_op_rank_metrics": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "gget_op_link_hits_workspace": (C.c_size_t, [i32]),
    "gget_op_link_hits": (i32, [vp, vp, i32, i64, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "gget_op_link_mrr_workspace": (C.c_size_t, [i32]),
    "gget_op_link_mrr": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "gget_op_cluster_metrics": (i32, [vp, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "gget_op_infer_append": (i32, [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, vp]),
    "gget_op_node_records": (i32, [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp]),
    "gget_op_cl_embed_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, vp]),
    "gget_op_cl_loss_fwd": (i32, [vp, i32, i32, f32, vp, vp, vp]),
    "gget_op_cl_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, i32, i32, i32, vp]),
    "gget_cl_logits": (i32, [vp, C.POINTER(vp)]),
    "gget_cl_embeddings": (i32, [vp, C.POINTER(vp)]),
    "gget_cl_loss": (i32, [vp, vp, vp]),
    "gget_cl_set_gathered": (i32, [vp, vp, i32, vp, vp]),
    "gget_cl_set_backward_scales": (i32, [vp, f32, f32]),
}
CL_MAX_N, CL_MAX_D = 2048, 1024   # include/gget.h "Contrastive pre-training head": 2 <= N <= 2048 (even), d % 64 == 0, d <= 1024
NODE_RECORDS_MAX_POS = 1 << 20   # include/gget.h GGET_NODE_RECORDS_MAX_POS: positions (B * S) one gget_op_node_records call takes
CLUSTER_MAX_C = 2048  # include/gget.h GGET_CLUSTER_MAX_C: the classes the LDS tables of gget_op_cluster_metrics hold

GEMM_NT, GEMM_NN, GEMM_TN = 0, 1, 2
OPT_NORM_FROM_BACKWARD = 1   # gget_set_option
OPT_SKIP_NONFINITE_STEP = 2
SHARD_CHUNK = 4096   # include/gget.h GGET_SHARD_CHUNK: the sharded norm's chunk grid and the granule of the body slices
SHARD_PARAMS, SHARD_MASTER, SHARD_ADAM_M, SHARD_ADAM_V, SHARD_SLOTS, SHARD_EMA = 0, 1, 2, 3, 4, 5   # gget_shard_allgather_async arenas
TOKENS_AUTO = -2   # gget_set_token_count: count the real tokens on the device (include/gget.h GGET_TOKENS_AUTO)
EPI_NONE, EPI_RESIDUAL, EPI_ATOMIC_F32, EPI_SLAB_F32 = 0, 1, 2, 3

# gget_debug_set / gget_debug_get keys of the process launch menu (csrc/menu.h kMenuRows, INTEGRATION.md "Kernel-selection knobs")
KEY_GEMM_VARIANT, KEY_GEMM_LDS_HEADROOM, KEY_GEMM_SPLIT_LAST, KEY_DETERMINISTIC, KEY_GEMM_STAGGER = 1, 2, 3, 4, 5
KEY_GEMM_ABLATE, KEY_HEAD_DENSE, KEY_HEAD_TILE, KEY_ATTN_OPROJ_OFF, KEY_LS_NORM_BWD_WIDE = 7, 8, 9, 10, 11
KEY_RMS_WIDE, KEY_CE_PARTS, KEY_GEMM_CU_RESERVE, KEY_OCCUPY_FAT, KEY_LINK_GRID, KEY_CE_GENERIC = 13, 14, 15, 16, 18, 19
KEY_EMBED_SORTED = 20
MENU_KEYS = (1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 13, 14, 15, 16, 18, 19, 20)
# KEY_GEMM_VARIANT bits (csrc/menu.h kGemm*): the first six switch a variant OFF, the last two switch one ON
GEMM_NO_KSPLIT_ND, GEMM_NO_KSPLIT_WGRAD, GEMM_NO_192_ROWS, GEMM_NO_SPLIT_LAST, GEMM_KSPLIT_128_ONLY, GEMM_ONE_BLOCK_PER_CU = 1, 2, 4, 8, 16, 32
GEMM_KSPLIT_DMA8, GEMM_AREA_RULE = 128, 512


def debug_get(key: int) -> int:
    v = i32()
    check(load().gget_debug_get(int(key), C.byref(v)))
    return int(v.value)


@contextlib.contextmanager
def debug_menu(keys):
    """Set process launch-menu keys ({key: value}) for the body and restore the values they had before."""
    saved = {k: debug_get(k) for k in keys}
    try:
        for k, v in keys.items():
            check(load().gget_debug_set(int(k), int(v)))
        yield
    finally:
        for k, v in saved.items():
            check(load().gget_debug_set(k, v))


def gemm_grouped(lib, mode, problems, stream):
    """problems: list of (A, B, C, M, N, K, lda, ldb, ldc) with torch tensors; one persistent launch."""
    n = len(problems)
    PA, IA = vp * n, i32 * n
    ptr = lambda k: PA(*[p[k].data_ptr() for p in problems])
    num = lambda k: IA(*[int(p[k]) for p in problems])
    return lib.gget_op_gemm_grouped(mode, n, ptr(0), ptr(1), ptr(2), num(3), num(4), num(5), num(6), num(7), num(8), stream)


def gemm_grouped_slab(lib, mode, problems, slab_stride, split_k, stream):
    """problems as for gemm_grouped, C fp32: one split-K launch into slabs `slab_stride` elements apart (GGET_EPI_SLAB_F32)."""
    n = len(problems)
    PA, IA = vp * n, i32 * n
    ptr = lambda k: PA(*[p[k].data_ptr() for p in problems])
    num = lambda k: IA(*[int(p[k]) for p in problems])
    return lib.gget_op_gemm_grouped_slab(mode, n, ptr(0), ptr(1), ptr(2), num(3), num(4), num(5), num(6), num(7), num(8), int(slab_stride),
                                         int(split_k), stream)


SLAB_PLAN_LM_HEAD, SLAB_PLAN_SHED_QKVO, SLAB_PLAN_SHED_O, SLAB_PLAN_QKVO = 0, 1, 2, 3   # include/gget.h GGET_SLAB_PLAN_*


def slab_plan(which: int, d: int, V: int, T: int) -> int:
    """K slices the engine's backward asks for under the current launch menu (gget_op_slab_plan)."""
    v = i32()
    check(load().gget_op_slab_plan(int(which), int(d), int(V), int(T), C.byref(v)))
    return int(v.value)
PROBLEM_SINGLE_LABEL, PROBLEM_REGRESSION_L1, PROBLEM_REGRESSION_MSE, PROBLEM_MULTI_LABEL, PROBLEM_AUC = 0, 1, 2, 3, 4
PROBLEM_TOKEN_CE_INTRA = 6   # loss_type = "token_ce_intra": as token_ce, logits = 20 <h^_s, h^_{cls_idx + c}> inside every sample
PROBLEM_TOKEN_CE = 5   # loss_type = "token_ce": score + cross-entropy on every labelled row, logits [B,S,C]

_lib = None


class GgetError(RuntimeError):
    pass


def load(path: str = LIB_PATH):
    """dlopen the engine.  Raises (never falls back) when the HIP library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # The HIP runtime must be the one PyTorch ships (torch/lib/libamdhip64.so): torch owns the device memory and the
    # streams we are handed, and a second runtime loaded first does not see the GPU on the pool's boxes.  Importing
    # torch first makes our DT_NEEDED libamdhip64 resolve to the already-loaded copy.
    import torch  # noqa: F401
    if not os.path.exists(path):
        raise GgetError(f"{path} is missing: build it with `python graph-gpt_amd/build.py` "
                        "(or __graft_entry__.build()); this engine has no CPU fallback")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        raise GgetError(f"gget error {rc}: {load().gget_last_error().decode()}")
