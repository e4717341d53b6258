/*
 * gget.h - C ABI of libgget_hip.so, the MI355X (gfx950) engine for the GraphGPT
 * Graph-Eulerian-Transformer hot path.
 *
 * The reference (alibaba/graph-gpt) has no FFI layer: its operator API for this path is the
 * Python nn.Module surface.  This header is the boundary a binding for that
 * surface sits on; every entry point cites the reference interface it replaces
 * (paths relative to the reference repo root).  The build's own ctypes binding is
 * graph-gpt_amd/_lib.py; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; gget_last_error() gives the text;
 *     nothing throws across the ABI;
 *   - all pointers named *_dev are device (HBM) pointers owned by the caller; the engine never
 *     allocates, frees or copies across PCIe behind the caller's back (the caller - PyTorch in
 *     our binding - owns memory and streams);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no host sync unless
 *     the function says so;
 *   - not thread-safe per handle; one handle per GPU per process (one process per GPU).
 *   - integer batch tensors use the reference's dtypes: int64 ids/labels/masks.
 */
#ifndef GGET_H_
#define GGET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GGET_KIND_PRETRAIN 0 /* GraphGPTPretrainBase (src/models/graphgpt/modeling_pretrain.py:57) */
#define GGET_KIND_TASK 1     /* GraphGPTTaskModel    (src/models/graphgpt/modeling_finetune.py:64) */
#define GGET_KIND_PRETRAIN_CL 2 /* GraphGPTPretrainBase with use_generative and use_discriminative (task_type "pretrain-cl", modeling_pretrain.py:96-115): the pre-train parameter plan plus cl_proj.weight [d,d]; everything said of GGET_KIND_PRETRAIN holds for it, see "Contrastive pre-training head" below */

#define GGET_PROBLEM_SINGLE_LABEL 0 /* CrossEntropy on pooled logits (modeling_finetune.py:209-214) */
#define GGET_PROBLEM_REGRESSION_L1 1 /* L1Loss  (modeling_finetune.py:183-197) */
#define GGET_PROBLEM_REGRESSION_MSE 2 /* MSELoss */
#define GGET_PROBLEM_TOKEN_CE 5 /* loss_type = "token_ce" (node-level tasks, modeling_finetune.py:162-164, :198-202): `score` on EVERY row, task_labels int64 [B,S] with -100 = unlabelled, mean cross-entropy over the labelled rows; task_logits_dev is then f32 [B,S,num_labels] (the reference hands the all-row logits back as `task_logits`), with or without labels */
#define GGET_PROBLEM_TOKEN_CE_INTRA 6 /* loss_type = "token_ce_intra" (modeling_finetune.py:140-165, :198-202): as GGET_PROBLEM_TOKEN_CE, but the logits of `score` are replaced by 20 <h^_s, h^_{cls_idx[b]+c}>, h^ = the L2-normalised final hidden row - every row against the num_labels label rows of its own sample; needs gget_set_cls_idx before the forward; `score` gets a zero gradient */
#define GGET_PROBLEM_AUC 4 /* pairwise squared-hinge AUC surrogate on logit[:,1]-logit[:,0] (src/utils/loss_utils.py:25-53, modeling_finetune.py:203-207); see gget_set_auc */
#define GGET_PROBLEM_MULTI_LABEL 3 /* BCEWithLogitsLoss on the non-NaN entries of float labels [B,num_labels] (modeling_finetune.py:227-230) */

/* Field meaning = GraphGPTConfig (src/models/graphgpt/configuration_graphgpt.py:26-110). */
typedef struct gget_config_t {
  int32_t kind;           /* GGET_KIND_* */
  int32_t vocab_size;
  int32_t hidden_size;    /* d, multiple of 64 */
  int32_t intermediate_size; /* ff, multiple of 64 */
  int32_t num_layers;
  int32_t num_heads;      /* d / 64 (head_dim 64: src/utils/modules_utils.py:37-42) or d / 32 (the tiny6 / small12 sizes of the launch
                           * scripts, hf head_dim = hidden_size / num_attention_heads); the head width is hidden_size / num_heads */
  int32_t stacked_feat;   /* F */
  int32_t next_n_token;   /* pre-train: F; 1 => n_token_proj is Identity */
  int32_t gated_agg;      /* stacked_feat_agg_method == "gated" */
  int32_t causal;         /* causal_attention */
  int32_t max_position;   /* max_position_embeddings */
  int32_t num_labels;     /* fine-tune head width */
  int32_t score_bias;     /* problem_type == "regression" */
  int32_t pad_token_id;
  float rms_eps;
  float rope_theta;
  float layer_scale_init; /* >0 => lambda_1 / lambda_2 per layer (utils_graphgpt.py:95-104) */
  int32_t max_tokens;     /* capacity: max B*S of any forward call */
  int32_t max_batch;      /* capacity: max B */
  float path_pdrop;       /* >0 => stochastic depth is available (rate linspace(0,path_pdrop,L), utils_graphgpt.py:184) */
  float mlp_pdrop;        /* >0 => MLP dropouts are available (utils_graphgpt.py:69-80): the residual adds run as their own kernels */
  int32_t head_mlp_layers;/* fine-tune: hidden layers of the `MLP` score head (len(config.mlp), src/utils/modules_utils.py:8-34); 0 = Linear */
  int32_t head_mlp[4];    /* their widths */
  int32_t embed_dim;      /* >0 => raw-embedding inputs [B,S,embed_dim] are projected and added to the token embeddings (config.embed_dim; modeling_pretrain.py:69-84, :131-149; modeling_helpers.py:127-139); multiple of 64 */
} gget_config_t;

/* Arena sizes the caller must provide (all 256-byte aligned device buffers). */
typedef struct gget_sizes_t {
  uint64_t n_params;        /* parameter elements (flat) */
  uint64_t param_bf16_bytes;/* compute copy of the parameters, bf16 [n_params] */
  uint64_t master_bytes;    /* fp32 master weights [n_params] */
  uint64_t adam_bytes;      /* fp32 m and v, 2*[n_params] */
  uint64_t grad_bf16_bytes; /* bf16 gradients [n_params] (what the DP all-reduce moves) */
  uint64_t workspace_bytes; /* activations + scratch for max_tokens */
} gget_sizes_t;

typedef struct gget_buffers_t {
  void* param_bf16_dev;
  void* master_dev;
  void* adam_m_dev;
  void* adam_v_dev;
  void* grad_bf16_dev;
  void* workspace_dev;
  const float* rope_cos_dev; /* [max_position][head_dim / 2] fp32 (32 columns at head width 64, 16 at 32), hf LlamaRotaryEmbedding
                              * tables; NULL => engine computes */
  const float* rope_sin_dev;
} gget_buffers_t;

typedef struct gget_param_info_t {
  char name[96];      /* reference state-dict key, e.g. "model.layers.3.mlp.down_proj.weight" */
  int32_t ndim;
  int64_t shape[2];
  uint64_t offset;    /* element offset into the flat param / master / adam / grad arrays */
  int32_t layer;      /* decoder layer index, -1 embeddings, num_layers = final norm + heads */
} gget_param_info_t;

typedef struct gget_engine* gget_handle_t;

const char* gget_last_error(void);
int gget_version(void);

/* replaces: GraphGPTPretrainBase.__init__/GraphGPTTaskModel.__init__ (modeling_pretrain.py:58-117,
 * modeling_finetune.py:67-105): computes the flat parameter layout and workspace need.
 * The flat arrays hold the named parameters (gget_param_info) at 128-element aligned offsets; the gaps, and for the
 * pre-train model round_up(V,64)-V zero rows behind lm_head.weight (its dgrad GEMM runs over K = round_up(V,64)), belong to
 * no parameter: the caller provides all arenas ZERO-FILLED (gradients and AdamW state of the gaps then stay zero).
 * gget_create additionally clears the workspace and the lm_head pad rows of every arena it is given (synchronously). */
int gget_query_sizes(const gget_config_t* cfg, gget_sizes_t* out);
int gget_create(const gget_config_t* cfg, const gget_buffers_t* bufs, gget_handle_t* out);
int gget_destroy(gget_handle_t h);

/* replaces: nn.Module.named_parameters()/state_dict() key+shape enumeration. */
int gget_param_count(gget_handle_t h);
int gget_param_info(gget_handle_t h, int index, gget_param_info_t* out);
/* number of DP gradient buckets (embeddings | one per decoder layer | final norm + heads) and their
 * element ranges in the flat gradient array, in the order backward completes them. */
int gget_bucket_count(gget_handle_t h);
int gget_bucket_range(gget_handle_t h, int bucket, uint64_t* offset, uint64_t* count);

/* replaces: `attention_dropout` / `path_pdrop` of the config + model.train()/eval() (reference launch scripts set
 * attention_dropout 0.1, e.g. examples/graph_lvl/pcqm4m_v2_pretrain.sh:20; ogbl-ppa fine-tuning adds path dropout 0.2,
 * examples/edge_lvl/ppa_supervised.sh:21-25): probabilities and RNG seed used by the NEXT forward and its backward;
 * zeros (default) are evaluation behaviour.  path_p is the LAST layer's rate (layer l uses path_p*l/(L-1)) and needs a
 * handle created with config.path_pdrop > 0. */
int gget_set_dropout(gget_handle_t h, float attention_p, float path_p, uint32_t seed);

/* Var-len (padding-free) token layout.  replaces: nothing the reference has as an operator - it runs every token-wise module over the
 * padded [B,S] grid and masks attention (src/models/graphgpt/modeling_helpers.py:38-64); its only remedy against padding is the
 * collator-side `pack_tokens` option (src/data/tokenizer.py:359-415, served by gget_forward_pretrain_packed).  n_real_tokens =
 * sum(attention_mask) of the NEXT gget_forward_pretrain / gget_forward_task batch, one of
 *     n > 0              the caller's count (the host knows it from its collator): no device->host traffic at all;
 *     GGET_TOKENS_AUTO   counted by the engine: the key lengths are summed on the device and the total is read back before the
 *                        launches are sized - 4 bytes and ONE host wait per forward (the counting kernel stores the total into a
 *                        pinned, coherent host word and the host polls it: no copy packet and no event in the stream since round 6;
 *                        the launches that do not need the count - head compaction, packed o weights - are enqueued in front of the
 *                        wait).  This is what the model classes
 *                        pass for a device-resident mask, i.e. for a call shaped exactly like the reference's step, which has just
 *                        synchronised on `.to(device)` of every batch tensor (src/utils/training_utils.py:17-26): the stream is
 *                        drained, the read costs a kernel launch + a 4-byte store over the host link (measured: bench.py `layouts`);
 *     anything else      unknown -> padded layout (the default of a bare C-ABI forward).
 * The count is consumed at the ENTRY of the next forward call, whether that call succeeds or not.
 * In the var-len layout the engine compacts the real tokens once (sample b owns rows [cu[b], cu[b] + len[b]))
 * and runs embedding, every GEMM / norm / residual of the layer stack, attention (per-sample row offsets) and the backward on
 * round_up(n_real_tokens, 64) rows instead of B*S.  Results are those of the padded layout (pad rows never influence real rows; the
 * loss, its normalisers, the dropout streams and all [B,S]-shaped inputs / outputs keep their logical coordinates: element-dropout hashes
 * and rope_range tables are keyed by the logical row, full-logit inference keeps the [B S F, V] cell order of its logits, the token-level
 * head writes task_logits [B,S,C] with zeros at padded positions, raw-embedding inputs are read at the logical row).  The engine falls back
 * to the padded layout by itself for packed rows only.  gget_hidden_states / gget_layer_hidden_states (pointers into the workspace) refuse after a var-len forward; gget_hidden_states_grid copies out of either layout.
 * A caller's count that DISAGREES with the mask cannot go unnoticed: the samples are cut at the count (no kernel leaves the rows of
 * the step), the step's loss is NaN, and a sticky device flag is raised that gget_deferred_status reports; the same flag is raised by
 * a label != -100 at a padded position (the reference's collator pads labels with -100; such a row does not exist in the compact
 * layout - its loss term is taken from a pad-token row instead of the padded grid's row).
 * gget_varlen_status: out[0] = 1 if the last forward ran var-len, out[1] = rows it ran on, out[2] = 1 if sum(key lengths) on the
 * device differed from n_real_tokens; synchronises the stream. */
#define GGET_TOKENS_AUTO (-2)
int gget_set_token_count(gget_handle_t h, int64_t n_real_tokens);
/* position_ids of a forward index the RoPE table precomputed for config.max_position rows (the reference evaluates the rotary embedding
 * per call, hf LlamaRotaryEmbedding.forward :111-127, and accepts any position): the engine reads them through a copy clamped to
 * [0, max_position) and raises a sticky device-side flag when it had to clamp.  *clamped_out = that flag (then cleared); synchronises
 * the stream - call it when convenient (end of an epoch, a logging step), not per step. */
int gget_position_status(gget_handle_t h, int32_t* clamped_out, void* stream);
int gget_varlen_status(gget_handle_t h, int32_t out[3], void* stream);
/* The sticky device-side input guards in one read (then cleared; synchronises the stream - call it where the loop synchronises anyway):
 * out[0] = position_ids were clamped into the RoPE table (as gget_position_status), out[1] = a var-len step ran on a token count the
 * mask contradicted, or met a label at a padded position (see gget_set_token_count).  replaces: the IndexError / shape error the
 * reference's nn.Embedding / rotary embedding raise synchronously for such inputs. */
int gget_deferred_status(gget_handle_t h, int32_t out[2], void* stream);
/* (out[0] is a bit set: 1 = position_ids clamped, 2 = a cls_idx of gget_set_cls_idx lay outside its sample and was clamped) */

/* replaces: `embed_pdrop` / `mlp_pdrop` of the config + model.train()/eval(): nn.Dropout on the gathered token embeddings
 * (modeling_helpers.py:96-98) and the two dropouts of the decoder MLP - on act(gate)*up and on down_proj's output
 * (utils_graphgpt.py:69-80) - for the NEXT forward and its backward, keyed by the seed of gget_set_dropout; zeros (default)
 * are evaluation behaviour.  mlp_p > 0 needs a handle created with config.mlp_pdrop > 0.  head_p: `config.dropout`, the
 * dropout between activation and Linear inside the MLP score head (src/utils/modules_utils.py:27-33). */
int gget_set_dropout_ex(gget_handle_t h, float embed_p, float mlp_p, float head_p);

/* replaces: the `inputs_raw_embeds` argument of the model forwards (config.embed_dim > 0): fp32 [B,S,embed_dim] on the device, consumed by the
 * NEXT gget_forward_* call (then forgotten).  Pre-train (modeling_pretrain.py:131-149): rows that carry a label are replaced by the learned
 * `emb_mask_token` (ALL of its next_n_token labels set - or, first_label_only != 0 = the smtp_inside rule, its first label), then RMSNorm (`embed_layernorm`), dropout (embed_pdrop of gget_set_dropout_ex) and `embed_proj`, added to the stacked token
 * embeddings; fine-tune (modeling_helpers.py:127-139): the same without the mask token.  A forward of a handle created with embed_dim > 0
 * fails without it, as the reference's does. */
int gget_set_raw_embeds(gget_handle_t h, const float* raw_embeds_dev, int first_label_only);

/* replaces: `config.rope_range` (configuration_graphgpt.py:42; utils_graphgpt.reset_pos_ids :574-581 through resolve_forward_defaults,
 * modeling_common.py:185-203): when > 0 and position ids are passed to a forward, the positions of every row are rescaled to
 * float(p) * rope_range / float(max_s p + 1) before the rotary embedding.  The engine then evaluates the angles per token (the
 * precomputed integer-position table does not apply).  Default 0 = off; forwards without position ids are not affected, as in the
 * reference. */
int gget_set_rope_range(gget_handle_t h, float rope_range);

/* replaces: `config.stack_method` ("short" | "long", configuration_graphgpt.py:50; examples/node_lvl/proteins_supervised.sh:31 runs
 * "long").  stack_long != 0: (i) the stacked embedding of every token is multiplied by min(1, 1 / (its non-zero feature ids + 1e-7))
 * (_get_stacked_inputs_embeds, modeling_helpers.py:106-110) in forward and backward, both model kinds; (ii) the SMTP head weighs
 * every labelled cell of sample b by 1 / (labelled cells of b + 1e-7) and sums / (B S F) - the per-feature-level path
 * (_prepare_for_stacked_feat_labels_per_feat_lvl :327-342 -> _get_dlm_ce_loss :180-198, modeling_pretrain.py:230-236); a
 * sample_wgt passed to the forward is ignored then, as in the reference (:368-374).  Default 0 = "short". */
int gget_set_stack_method(gget_handle_t h, int stack_long);

/* replaces: `config.focal_gamma` (configs/training/base.yaml:60): > 0 turns the SMTP head's mean cross-entropy into the focal loss
 * of utils_graphgpt.FocalLoss (:340-376) - every row weighted by (1 - p_target)^gamma, the weight detached as in the reference.
 * Applies to gget_forward_pretrain[_packed] without sample_wgt (_get_ce_loss, modeling_helpers.py:158-160). */
int gget_set_focal_gamma(gget_handle_t h, float gamma);

/* replaces: `config.num_neg` + the torch RNG behind `torch.randperm` in auc_loss (src/utils/loss_utils.py:25-43): negatives per
 * positive and the seed of the counter-hash permutation the NEXT gget_forward_task(problem_type = GGET_PROBLEM_AUC) draws its
 * negative samples with (idx = perm(P * num_neg) % N_neg; perm = rank of the hashed keys). */
int gget_set_auc(gget_handle_t h, int num_neg, uint32_t seed);

/* replaces: the `cls_idx` argument of GraphGPTTaskModel.forward (modeling_finetune.py:236-250; tokenizer_utils.py:729-747 appends the
 * label tokens and records where they start): int64 [B] on the device, the first of the num_labels label rows inside every sample, read
 * by the NEXT gget_forward_task(problem_type = GGET_PROBLEM_TOKEN_CE_INTRA), which keeps its own clamped copy for the backward (the
 * pointer is consumed by that forward: set it before every call; such a forward without it is error 2).  0 <= cls_idx[b] and cls_idx[b] + num_labels <= the sample's real row
 * count; a value outside is clamped into that range and reported by gget_deferred_status (bit 2 of out[0]). */
int gget_set_cls_idx(gget_handle_t h, const int64_t* cls_idx_dev);

/* replaces: load_state_dict + `.to(bfloat16)`: refresh the bf16 compute copy from the fp32 master. */
int gget_sync_params(gget_handle_t h, void* stream);

/* replaces: GraphGPTPretrainBase.forward (modeling_pretrain.py:152-266).
 *   input_ids i64 [B,S,F]; attention_mask i64 [B,S] (1 real / 0 right padding);
 *   labels i64 [B,S,next_n] (-100 = not predicted) or NULL (=> logits for every cell, no loss);
 *   sample_wgt f32 [B] or NULL (dLM weighting, modeling_pretrain.py:230-236);
 *   position_ids i64 [B,S] or NULL (=> arange(S), hf LlamaModel.forward :389-392).
 *   loss_dev: f32[1] device scalar (head1_loss).  Logits stay in the workspace: gget_head_logits. */
int gget_forward_pretrain(gget_handle_t h, const int64_t* input_ids_dev, const int64_t* attention_mask_dev,
                          const int64_t* labels_dev, const float* sample_wgt_dev, const int64_t* position_ids_dev,
                          int B, int S, float* loss_dev, void* stream);

/* replaces: GraphGPTTaskModel.forward + calculate_task_loss (modeling_finetune.py:236-326, :167-234).
 *   task_labels: i64 [B] (single label) or f32 [B] (regression), NULL => no loss;
 *   task_logits_dev f32 [B,num_labels] (pooled "last" row, returned as .float());
 *   task_hidden_dev bf16 [B,d] or NULL. */
/* replaces: the same forward on PACKED rows (reference GraphsMapDataset.pack_token_seq, src/data/tokenizer.py:359-415;
 * block-diagonal mask built at src/utils/tokenizer_utils.py:349-355 and expanded by _expand_mask_from_3d_mask,
 * modeling_helpers.py:51-64): attention_mask3d is int64 [B,S,S]; a token attends exactly the contiguous key range of its
 * own graph (first .. last non-zero of its mask row), all-zero rows are padding.  backward / adamw as usual. */
int gget_forward_pretrain_packed(gget_handle_t h, const int64_t* input_ids_dev, const int64_t* attention_mask3d_dev,
                                 const int64_t* labels_dev, const float* sample_wgt_dev, const int64_t* position_ids_dev,
                                 int B, int S, float* loss_dev, void* stream);
int gget_forward_task(gget_handle_t h, const int64_t* input_ids_dev, const int64_t* attention_mask_dev,
                      const int64_t* position_ids_dev, const void* task_labels_dev, const float* sample_wgt_dev,
                      int problem_type, int B, int S, float* loss_dev, float* task_logits_dev,
                      void* task_hidden_dev, void* stream);

/* replaces: loss.backward() / engine.backward(loss) (src/utils/training_utils.py:44,66).
 * Full backward of the last forward; bf16 gradients of every parameter land in grad_bf16_dev.
 * The staged form lets the caller overlap the DP all-reduce of bucket k with the backward of the
 * next layers (one HIP event per bucket on the caller's side):
 *   gget_backward_begin  -> head + final norm   (bucket 0 complete)
 *   gget_backward_layer(i) for i = L-1..0       (bucket L-i complete)
 *   gget_backward_end    -> embedding scatter   (last bucket complete)
 * The backward reads the SAME bf16 weights the forward used (the caller's arena): do not write parameters between a forward and its
 * backward.  gget_sync_params / gget_adamw_step in between are tolerated - the per-sample kernels' fragment-major o-weight copies of that
 * forward are dropped and the backward takes the three-launch form on the live weights - but the gradients then mix two weight versions. */
int gget_backward(gget_handle_t h, float loss_scale, void* stream);
int gget_backward_begin(gget_handle_t h, float loss_scale, void* stream);
int gget_backward_layer(gget_handle_t h, int layer, void* stream);
int gget_backward_end(gget_handle_t h, void* stream);

/* Engine options (no reference counterpart: promises of the caller that let the engine skip work).
 * GGET_OPT_NORM_FROM_BACKWARD = 1: "nothing rewrites the bf16 gradient array between gget_backward* and gget_adamw_step" (a single-rank
 *   step; any exchange rewrites it).  gget_adamw_step then takes the squared norm of the decoder layers' weight-gradient matrices
 *   (93 % of the base model's parameters) from per-tile partial sums their weight-gradient launches left behind and reads only the
 *   remaining tensors again - the clip + AdamW step (reference: torch.nn.utils.clip_grad_norm_ + AdamW, src/utils/training_utils.py
 *   :72-82, DeepSpeed's gradient_clipping) loses its 244 MB norm pass.  Ignored (full pass) whenever grad_scale != 1 or a layer's launch
 *   left no partials.  The norm is the same sum in another (fixed) order: equal to fp32 rounding. */
#define GGET_OPT_NORM_FROM_BACKWARD 1
/* GGET_OPT_SKIP_NONFINITE_STEP = 1: gget_adamw_step touches nothing (weights, Adam moments, bf16 copy) when the global gradient norm is
 *   inf / NaN - what torch.cuda.amp.GradScaler.step does on the reference's DDP branch (src/utils/training_utils.py:46-86: scale,
 *   backward, unscale_, clip, scaler.step, scaler.update).  The norm still reaches gnorm_dev, so the caller can tell (and keep its
 *   1-based step count for the skipped step).  Off by default: DeepSpeed's bf16 optimizer, the path the engine reproduces, has no such guard. */
#define GGET_OPT_SKIP_NONFINITE_STEP 2
int gget_set_option(gget_handle_t h, int option, int value);
/* The data-parallel share of the launch menu, carried by the handle: during this handle's forward / backward calls its launches plan with
 * the process menu (gget_debug_set) overlaid by these fields.  reserve_cus = R > 0: every GEMM plan counts the device's CUs minus R
 * (rounded down to a multiple of 8), which leaves R CUs to the collective library's workgroups (these cannot share a CU with a GEMM
 * workgroup); the 128x192 / 192x128 tiles keep their 3-slot rings and the short RMSNorm backward launches take the 4-wave blocks.
 * lds_headroom != 0 with reserve_cus = 0: no GEMM launch with two LDS-filling workgroups per CU and the three-launch S <= 32 backward,
 * so that a collective's workgroup can share a CU.  (0, 0), the state of a new handle: the process menu as it is,
 * i.e. the single-GPU selection.  Op-level entries (gget_op_*) always see the process menu. */
int gget_set_dp_menu(gget_handle_t h, int reserve_cus, int lds_headroom);

/* ------------------------------------------------------------------------------------------
 * Data-parallel gradient exchange.  replaces: the DDP gradient all-reduce (src/utils/opt_utils.py:13),
 * DeepSpeed ZeRO-2's reduce-scatter/all-gather (examples/ds_config2_pt.json:29-32) and the communicator bootstrap of
 * set_dist_env (src/utils/misc_utils.py:507-539, init_process_group at :519-526).  One process per GPU; rank 0 obtains a
 * unique id and hands it to the other ranks out of band (launcher store, MPI, torch.distributed broadcast ...).
 * gget_allreduce_grads_async enqueues the SUM all-reduce of one gradient bucket (gget_bucket_range; -1 = the whole flat
 * array) on `side_stream`: the caller makes that stream wait for the backward stage that finalises the bucket
 * (gget_backward_begin / _layer / _end) and makes the compute stream wait for it before gget_adamw_step, whose grad_scale
 * = 1/world turns the sum into the mean.  fp32_accumulate != 0 widens the bucket to fp32 for the reduction (one rounding
 * instead of world-1) at twice the wire bytes.  RCCL is bound lazily (dlopen of librccl.so.1).
 * ------------------------------------------------------------------------------------------ */
#define GGET_UNIQUE_ID_BYTES 128
int gget_comm_unique_id(void* out_bytes /* GGET_UNIQUE_ID_BYTES */);
int gget_comm_init(gget_handle_t h, int rank, int world, const void* unique_id_bytes);
int gget_comm_destroy(gget_handle_t h);
/* hands the communicator of `src` (and its staging buffer) to `dst`, a handle of the same model created with other capacities
 * (the host re-creates the handle when a larger batch arrives): no collective, so ranks may do it independently. */
int gget_comm_move(gget_handle_t dst, gget_handle_t src);
int gget_allreduce_grads_async(gget_handle_t h, int bucket, int fp32_accumulate, void* side_stream);
/* the same collective over an arbitrary element range [offset, offset + count) of the flat gradient array: several consecutive
 * buckets in ONE collective (fewer, larger messages - xGMI rings are per-link bound; the host picks the coalescing, e.g.
 * GGET_DP_BUCKET_MB in graph-gpt_amd/training.py).  The range must lie inside [0, n_params). */
int gget_allreduce_range_async(gget_handle_t h, uint64_t offset, uint64_t count, int fp32_accumulate, void* side_stream);
/* A communicator that needs no peers (tests / dry runs of the exchange schedule on one GPU): the handle behaves as rank 0 of `world`
 * ranks that all hold THIS rank's gradients, i.e. every "all-reduce" multiplies the range by `world` on the side stream (the same
 * stream / event protocol as the RCCL collective; with grad_scale = 1/world the step equals the single-rank step).  No reference
 * counterpart - RCCL refuses two ranks on one device, and the exchange schedule (bucket ranges, stream waits, the 1/world folded into
 * AdamW) must be testable beyond world 1 on a one-GPU box. */
int gget_comm_init_loopback(gget_handle_t h, int world);

/* replaces: clip_grad_norm_ + AdamW.step / FusedAdam (training_utils.py:68-80, opt_utils.py:18-24,
 * examples/ds_config2_pt.json:11-19).  grad_scale multiplies every gradient first (1/world after a
 * sum all-reduce); max_grad_norm <= 0 disables clipping; step is 1-based.
 * gnorm_dev (f32[1], may be NULL) receives the pre-clip global L2 norm. */
int gget_adamw_step(gget_handle_t h, float lr, float beta1, float beta2, float eps, float weight_decay,
                    float max_grad_norm, float grad_scale, int step, float* gnorm_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradient accumulation (`training.optimizer.gradient_accumulation_steps = k`).  replaces: the fp32 accumulation of the DeepSpeed engine
 * the reference hands k to (src/conf/conf_utils.py:59-66; its bf16 optimizer adds every micro-batch's gradient to an fp32 buffer and steps
 * at the boundary only).  The sum is a SEVENTH, optional arena: fp32 [n_params] with the offsets of the other six.  While a window is open
 * (count > 0) gget_adamw_step, gget_adamw_step_sharded, gget_shard_sqnorm_partials and the rules of GGET_OPT_NORM_FROM_BACKWARD (ignored:
 * the last backward's partials say nothing about a sum) and GGET_OPT_SKIP_NONFINITE_STEP read the fp32 sum instead of the bf16 gradient
 * array - the same kernels with an fp32 load, so the sum of k * world bf16 gradients is never rounded back to bf16 - and the two AdamW
 * entries close the window (count = 0), also when the skip rule drops the update.  grad_scale = 1 / (k * world) turns the sum into the mean.
 * A handle that never attaches an accumulator allocates nothing and launches nothing new.
 * ------------------------------------------------------------------------------------------ */
/* replaces: the allocation of DeepSpeed's fp32 gradient buffer at deepspeed.initialize (conf_utils.py:59-66 carries k into its config).
 * The arena: n_params floats owned by the caller (its contents do not matter: the first micro-step of a window overwrites); NULL detaches.
 * No window is open afterwards. */
int gget_grad_acc_attach(gget_handle_t h, float* acc_dev);
/* replaces: the per-micro-batch accumulation of the DeepSpeed engine's backward (conf_utils.py:59-66 -> gradient_accumulation_steps):
 * acc[i] = (count == 0 ? 0 : acc[i]) + float(grad_bf16[i]) over the whole flat gradient array - gaps and lm_head pad rows included, zero
 * in, zero out - in one launch of 16-byte loads and stores (6 B per parameter on the first micro-step, which overwrites instead of adding:
 * there is no zero-fill pass; 10 B afterwards); count += 1.  Call it once the micro-batch's exchange has been waited for on `stream`. */
int gget_grad_accumulate(gget_handle_t h, void* stream);
/* replaces: DeepSpeed's micro_steps bookkeeping inside a window (engine.is_gradient_accumulation_boundary, driven by conf_utils.py:59-66):
 * micro-steps summed so far in the open window; 0 = no window open (or no accumulator). */
int gget_grad_acc_count(gget_handle_t h, int32_t* out);
/* replaces: the restore of that bookkeeping when DeepSpeed loads a checkpoint taken inside a window (conf_utils.py:59-66's engine): the
 * resume path - after the caller has written a saved partial sum into the arena, n > 0 re-opens the window at n micro-steps; 0 closes it. */
int gget_grad_acc_set_count(gget_handle_t h, int32_t n);

/* ------------------------------------------------------------------------------------------
 * Frozen prefix (`training.finetune.freeze = k`, configs/training/base.yaml:65 "-1->no, 0->embedding").  replaces:
 * modules_utils.freeze_llama_layers (src/utils/modules_utils.py:45-54) as FinetuneMode.post_model_setup calls it
 * (src/training/finetune_mode.py:204-212) plus what torch does with requires_grad = False: no gradient, no share of the clip's norm, no
 * optimizer update.  Only this prefix pattern exists; there is no per-parameter mask.
 * ------------------------------------------------------------------------------------------ */
/* replaces: freeze_llama_layers(model, k) (modules_utils.py:45-54).  frozen_layers = -1: nothing is frozen (the state of a new handle; every
 * launch is then what it was without this entry).  k >= 0: model.embed_tokens.weight and every parameter of layers [0, min(k, L)) are
 * frozen (a Python slice: k >= L freezes all layers); gate / raw-embedding parameters, lambda_1 / lambda_2 of the layers >= k, model.norm
 * and the heads stay trainable.  From the next call on, norm, clip, AdamW, the EMA lerp (fused and gget_ema_update with decay > 0; decay
 * = 0, the seed, still copies every weight), gget_grad_accumulate, the shard plan (a bucket's sharded range = its trainable share, count 0
 * = skipped everywhere; an active plan is rebuilt, its slots_per_rank may shrink: gget_shard_init reports it) and gget_allreduce_grads_async touch
 * the trainable ranges only: master, m, v, the bf16 copy and the EMA of the frozen ranges are never written.  If nothing trainable sits
 * upstream of layer 0 (no gated aggregation, embed_dim = 0) the backward is truncated: gget_backward_layer(i < k) and gget_backward_end
 * return 0 without a launch, the frozen gradient ranges are not written, and the lowest trainable unit - layer k's input_layernorm, or
 * model.norm for k >= L - runs a weight-gradient-only RMSNorm backward.  Otherwise the full chain runs (the upstream gradients need the
 * dgrad through the frozen layers) and frozen gradients are written but never read.  Callable between steps; refused while a
 * gradient-accumulation window is open.  Synchronous (uploads the work-item tables of the ranges). */
int gget_set_frozen(gget_handle_t h, int frozen_layers);
/* replaces: the `p.requires_grad` filter the reference's optimizers and clip_grad_norm_ apply to model.parameters() (modules_utils.py:45-54
 * sets the flags; src/utils/training_utils.py:68-80 consumes them): the trainable element ranges of the flat arenas, out = {offset0, count0,
 * offset1, count1}, *n_out = how many are valid (1 = everything, [0, n_params), when nothing is frozen; else at most two:
 * [end of embed_tokens, start of layer 0) - empty and dropped without gate / raw-embedding parameters - and [start of layer min(k, L),
 * n_params)).  The host builds its exchange groups from them. */
int gget_trainable_ranges(gget_handle_t h, uint64_t out[4], int32_t* n_out);
/* replaces: the same `p.requires_grad` filter seen per gradient bucket (what DDP's reducer and DeepSpeed's partitioning skip for a frozen
 * parameter; modules_utils.py:45-54): {offset, count} of the trainable share of bucket `bucket` of gget_bucket_range - the bucket itself,
 * nothing (count 0, offset = the bucket's), or the embedding bucket's gate / raw-embedding parameters.  A bucket meets at most one of the
 * trainable ranges, in one piece.  What the exchange and the shard plan cut; the rule lives here only. */
int gget_bucket_train_range(gget_handle_t h, int bucket, uint64_t* offset, uint64_t* count);

/* ------------------------------------------------------------------------------------------
 * Weight EMA (`training.optimizer.use_ema` / `ema_decay`; the reference's fine-tune launch scripts switch it on, e.g.
 * examples/graph_lvl/pcqm4m_v2_supervised.sh:65).  replaces: timm's ModelEmaV3 as the reference patches and drives it -
 * src/utils/patch_utils.py:11-42 (apply_update_: every bf16 DeepSpeed weight cast to fp32, torch._foreach_lerp_ over the module's tensors)
 * and src/conf/stats_configs.py:102-146 (EMAStats: init_ema deep-copies the module, update_ema after every batch, save / load of
 * model_ema.pt).  Here the average is a SIXTH arena, fp32 [n_params] with the offsets of the other five, and lives inside the AdamW launch.
 * THE formula, fused or stand-alone (one device function):  ema' = w + d * (ema - w)  in fp32, evaluated as fmaf(d, ema - w, w) with d the
 * fp32 decay exactly as it crossed this ABI (timm's ema.lerp_(w, 1 - d) written without the 1 - d).  d = 0 gives ema' == w bit for bit -
 * how the arena is seeded - and no 1 - d is formed.  w = the fp32 MASTER weights: the one deliberate difference to the reference's
 * DeepSpeed branch, which averages the bf16 module weights cast to fp32 because it cannot reach the master copy (patch_utils.py:8; its DDP
 * branch averages fp32 parameters as this does).  Gaps and lm_head pad rows stay zero (zero in, zero out).
 * ------------------------------------------------------------------------------------------ */
/* replaces: EMAStats.init_ema -> ModelEmaV3.__init__ (stats_configs.py:109-116; the deep copy itself is the d = 0 update below).  The
 * arena: n_params floats, ZERO-FILLED by the caller like the others; NULL detaches.  Clears its lm_head pad rows like gget_create
 * (synchronously) and forgets a pending decay. */
int gget_ema_attach(gget_handle_t h, float* ema_dev);
/* replaces: the `decay` ModelEmaV3.update hands to apply_update_ (timm ModelEmaV3.get_decay; patch_utils.py:11-42): the decay the NEXT
 * gget_adamw_step / gget_adamw_step_sharded applies inside its launch, consumed by it - the lerp runs against the NEW weights, from the
 * registers (28 -> 36 B per parameter), and a step that GGET_OPT_SKIP_NONFINITE_STEP drops still averages, against the unchanged weights,
 * as the reference calls update_ema whether or not the optimizer stepped (src/training/finetune_mode.py:405-413).  A negative value (the
 * state of a new handle) = that step leaves the EMA alone.  The per-step rule (which decay at which step) lives on the host. */
int gget_set_ema_decay(gget_handle_t h, float decay);
/* replaces: EMAStats.update_ema -> ModelEmaV3.update (stats_configs.py:131-136) where no AdamW launch runs: the stand-alone lerp over the
 * whole arena, or over this rank's share (body slices + tails) when a shard plan is active.  decay in [0, 1]; 0 copies the master weights. */
int gget_ema_update(gget_handle_t h, float decay, void* stream);
/* replaces: evaluating `ema_stats.model_ema.module` instead of the model (src/utils/log_eval_dump_utils.py:720-793): the bf16 compute copy
 * is rewritten from the EMA arena (gget_sync_params with another source; the fragment-major o-weight copies are dropped like there).
 * gget_sync_params restores the live weights. */
int gget_ema_to_params(gget_handle_t h, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sharded optimizer step (ZeRO stage 2).  replaces: DeepSpeed's `"zero_optimization": {"stage": 2}` of the reference's pre-training
 * (examples/ds_config2_pt.json:29-32, engine built at src/training/pretrain_mode.py:281-287): gradients are reduce-scattered, every rank
 * runs clip + AdamW over its 1/world of the fp32 state only, and the bf16 compute copy is all-gathered.  The fp32 arenas keep their full
 * size (only the WORK is partitioned); outside a rank's share master / m / v are stale after a sharded step until gget_shard_allgather_async
 * of GGET_SHARD_MASTER / _ADAM_M / _ADAM_V (the consolidation DeepSpeed's zero_to_fp32 does offline).
 * Plan (per bucket b of gget_bucket_range, C = GGET_SHARD_CHUNK): slice = floor(cnt / (world C)) C; rank r owns the body slice
 * [off + r slice, off + (r + 1) slice); the tail [off + world slice, off + cnt) (< world C elements) is all-reduced and updated by every
 * rank.  The gradient norm is summed over the fixed chunk grid off + j C of every bucket, which does not depend on world: every rank
 * writes the sums of the chunks it owns (rank 0 also the tails') into its `slots_per_rank` entries of a caller-owned fp32 vector
 * [world][slots_per_rank], the vector is all-gathered, and gget_adamw_step_sharded adds the chunks in global order (fixed tree): the same
 * bits on every rank and for every world size, equal to gget_adamw_step's norm to fp32 rounding (another order).  Given the same
 * coefficient the update of an element is bit-identical to gget_adamw_step's (one device function).
 * A loopback communicator (gget_comm_init_loopback) stands for `world` ranks holding this rank's gradients: the handle then does the work
 * of every rank (all bodies, all chunks) and the all-gathers are no-ops - the schedule of a `world`-rank job on one GPU.
 * ------------------------------------------------------------------------------------------ */
#define GGET_SHARD_CHUNK 4096
#define GGET_SHARD_PARAMS 0 /* the bf16 compute copy (after every sharded step, before anything reads the weights) */
#define GGET_SHARD_MASTER 1 /* fp32 master weights */
#define GGET_SHARD_ADAM_M 2
#define GGET_SHARD_ADAM_V 3
#define GGET_SHARD_SLOTS 4  /* the norm's partial vector (slots_dev) */
#define GGET_SHARD_EMA 5    /* the weight-EMA arena (gget_ema_attach): every rank averages its share only */
/* replaces: DeepSpeed stage-2 partitioning (deepspeed/runtime/zero/stage_1_and_2.py, driven by ds_config2_pt.json:29-32).  The plan of
 * one bucket for `world` ranks, from the configuration alone (no device): out = {offset, count, slice, tail_offset, tail_count}. */
int gget_shard_plan(const gget_config_t* cfg, int world, int bucket, uint64_t out[5]);
/* replaces: the partition set-up of deepspeed.initialize with stage 2 (pretrain_mode.py:281-287).  Switches the handle to the plan of
 * rank `rank` of `world` (world 0 = off) and builds the device tables (AdamW work items, norm chunks, chunk -> slot map), owned by the
 * handle; synchronous.  With a communicator, rank / world must be its own.  *slots_per_rank (may be NULL) = entries per rank of the
 * partial vector. */
int gget_shard_init(gget_handle_t h, int world, int rank, int32_t* slots_per_rank);
/* replaces: reading back DeepSpeed's partition boundaries (stage_1_and_2.py keeps them per parameter group): the ACTIVE plan of one bucket,
 * out = {offset, count, slice, tail_offset, tail_count} as gget_shard_plan - cut from the bucket's trainable share (gget_bucket_train_range),
 * so equal to gget_shard_plan's only while nothing is frozen.  An error when no plan is active. */
int gget_shard_bucket(gget_handle_t h, int bucket, uint64_t out[5]);
/* replaces: the bucketed reduce-scatter of DeepSpeed stage 2 (reduce_scatter: true in ds_config2_pt.json's zero_optimization): the body of
 * bucket `bucket` reduce-scattered in place (this rank's slice receives the sum) and the tail all-reduced, one group on `side_stream`
 * (stream protocol and fp32_accumulate as gget_allreduce_grads_async; the loopback multiplies the whole bucket by world). */
int gget_reduce_scatter_grads_async(gget_handle_t h, int bucket, int fp32_accumulate, void* side_stream);
/* replaces: the squared-norm part of DeepSpeed's clip over partitioned gradients (stage_1_and_2.py get_grad_norm, gradient_clipping of
 * ds_config2_pt.json): the sums of the chunks this rank owns into slots_dev[rank * slots_per_rank ...] (all ranks' for the loopback). */
int gget_shard_sqnorm_partials(gget_handle_t h, float* slots_dev, void* stream);
/* replaces: the all-gather of the updated bf16 partitions (stage_1_and_2.py step -> all_gather_dp_groups) and, for the fp32 arenas, the
 * consolidation of zero_to_fp32.py.  `what` = GGET_SHARD_*: the bucket bodies of that arena gathered in place, embeddings first (the order
 * the forward reads them), one collective per bucket; GGET_SHARD_SLOTS gathers the partial vector slots_dev.  No-op for the loopback. */
int gget_shard_allgather_async(gget_handle_t h, int what, float* slots_dev, void* stream);
/* replaces: clip + FusedAdam.step over the rank's partition (DeepSpeed stage 2; training_utils.py:68-80 for the clip rule).  Arguments as
 * gget_adamw_step; slots_dev = the GATHERED partial vector (may be NULL when no norm is needed: max_grad_norm <= 0, gnorm_dev NULL and
 * GGET_OPT_SKIP_NONFINITE_STEP off).  Updates this rank's body slices and every tail (master, m, v and the bf16 copy) in one launch;
 * GGET_OPT_SKIP_NONFINITE_STEP applies (every rank sees the same norm, so all skip together). */
int gget_adamw_step_sharded(gget_handle_t h, float lr, float beta1, float beta2, float eps, float weight_decay, float max_grad_norm,
                            float grad_scale, int step, const float* slots_dev, float* gnorm_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Parameter groups (per-parameter learning-rate and weight-decay scales).  replaces: torch parameter groups handed to AdamW(params=groups)
 * - the reference's layer-wise lr decay (src/utils/loss_utils.py:370-412, get_layerwise_param_groups: lr = base_lr * lr_decay**depth per
 * group) and the usual "no weight decay on norm weights" split.  The table holds two fp32 scales per parameter, indexed like
 * gget_param_info.  With a table set, every optimizer step runs over work items (at most 2048 elements, one block each) cut so that no
 * item crosses a parameter boundary at which either scale changes; the alignment gap behind a parameter, and the zero rows behind
 * lm_head.weight, ride with the parameter in front of them (zeros: they stay zero under any scale).  The kernel forms
 *     lr_i = lr * lr_scale        wd_i = weight_decay * wd_scale        (one fp32 product each)
 * per item and the update runs with these two values in place of lr and weight_decay - nothing else differs, so an element's result is
 * that of gget_adamw_step called with (lr_i, wd_i): with both scales 1.0f the bits equal the ungrouped step's.  lr_scale = 0 follows
 * torch: m and v are updated, the master weight and its bf16 copy keep their bits.  The clip norm is over ALL trainable gradients whatever
 * their scale (clip_grad_norm_ over model.parameters()); norm chunks, slots, GGET_OPT_NORM_FROM_BACKWARD, the fused and the stand-alone
 * EMA, the fp32 accumulator and GGET_OPT_SKIP_NONFINITE_STEP work as without a table.  A parameter that belongs to no group of the
 * caller's has no special state here: it takes whatever scale the caller wrote for it (1.0 = the step's own lr) - a caller that wants
 * torch's "not in the optimizer" must freeze it or say lr_scale 0.  With no table set no launch changes.
 * ------------------------------------------------------------------------------------------ */
/* one work item of a grouped step: elements [off, off + cnt) of the flat arenas (multiples of 4, cnt <= 2048) and their two scales */
typedef struct gget_group_item_t {
  uint64_t off;
  uint64_t cnt;
  float lr_scale;
  float wd_scale;
} gget_group_item_t;
/* replaces: the `lr` / `weight_decay` entries of torch parameter groups (loss_utils.py:383-386, :408-411).  n must equal
 * gget_param_count; a NULL array means all ones; NULL, NULL, 0 switches the feature off (the state of a new handle).  Every scale must be
 * finite and >= 0: a wrong n or a bad value is error 2 and nothing changes.  The table stays on the handle: gget_set_frozen and
 * gget_shard_init apply it to the lists they build, and this call rebuilds theirs, so the call order does not matter.  Synchronous
 * (uploads work-item tables).  The replicated step of an unfrozen model then runs over items covering the whole arena instead of the
 * grid-stride launch. */
int gget_set_param_scales(gget_handle_t h, const float* lr_scale, const float* wd_scale, int n);
/* replaces: reading `optimizer.param_groups[i]["lr"]` back.  The table (ones while the feature is off) into lr_out / wd_out (either may
 * be NULL); n must equal gget_param_count. */
int gget_param_scales(gget_handle_t h, float* lr_out, float* wd_out, int n);
/* replaces: nn.Module.named_parameters() before any device exists (what the reference's group builders walk): gget_param_count /
 * gget_param_info from the configuration alone.  The count is -1 for a bad configuration. */
int gget_plan_param_count(const gget_config_t* cfg);
int gget_plan_param_info(const gget_config_t* cfg, int index, gget_param_info_t* out);
/* replaces: nothing in the reference (torch iterates groups tensor by tensor); the handle-free twin of the lists above, as gget_shard_plan
 * is of gget_shard_init: the work items the step of this configuration runs.  lr_scale / wd_scale / n as gget_set_param_scales (NULL,
 * NULL, 0 = all ones); frozen_layers as gget_set_frozen; world = 0 the replicated step (gget_adamw_step), world >= 1 the sharded step
 * of rank `rank`, rank = -1 every rank's share (the loopback communicator).  *n_out = the number of items; the first min(cap, *n_out)
 * are written to items_out (cap = 0 with items_out NULL asks for the count).  Bad scales, n or ranks are error 2. */
int gget_group_plan(const gget_config_t* cfg, const float* lr_scale, const float* wd_scale, int n, int frozen_layers, int world, int rank,
                    gget_group_item_t* items_out, int cap, int32_t* n_out);

/* Head bookkeeping of the last pre-train forward.  counts[0] = M (positions with >=1 masked
 * feature), counts[1] = Lm (masked feature tokens).  Synchronises `stream`.
 * logits: bf16 [Lm][ld] with ld = round_up(V,64) (pad columns are zero). */
int gget_head_counts(gget_handle_t h, int32_t counts[2], void* stream);
int gget_head_logits(gget_handle_t h, const void** logits_dev, int32_t* ld);
/* final hidden states bf16 [B*S][d] of the last forward (outputs[0] of the backbone) */
int gget_hidden_states(gget_handle_t h, const void** hidden_dev);
/* residual stream bf16 [B*S][d] ENTERING decoder layer `layer` (layer = num_layers: leaving the last layer, before the final norm) of
 * the last forward.  replaces: `output_hidden_states=True` of the reference's backbone (hf LlamaModel.forward modeling_llama.py
 * :401-414 collects exactly these tensors); used by the per-layer error budget of tests/test_error_budget.py.  Padded layout only. */
int gget_layer_hidden_states(gget_handle_t h, int layer, const void** hidden_dev);
/* Both of the above as a COPY in the reference's [B,S,d] layout, after a forward on either token layout: layer = -1 the final-normed
 * hidden states (`outputs.hidden_states[-1]` of modeling_pretrain.py:264 / modeling_finetune.py:323), 0 .. num_layers the residual
 * stream entering that layer (hf LlamaModel.forward :401-414).  After a var-len forward the rows go back to their (b, s) positions;
 * positions behind a sample's tokens read as zero.  out_dev: bf16 [B * S * hidden] for the last forward's B and S. */
int gget_hidden_states_grid(gget_handle_t h, int layer, void* out_dev, void* stream);
/* replaces: `output_attentions=True` - `outputs.attentions` as the model classes hand it through (modeling_pretrain.py:265,
 * modeling_finetune.py:325, documented at modeling_common.py:79): the softmax weights of hf eager_attention_forward (modeling_llama.py
 * :191-214) of decoder layer `layer` of the LAST forward, recomputed from that layer's rotated q | k and its log-sum-exp, which every
 * forward mode keeps in the workspace - pre-train, packed and fine-tune forwards, either token layout, with or without labels: no mode is
 * refused.  out_dev: bf16 [B, H, S, S] for that forward's B and S, every element written (the caller may pass uninitialised memory).
 * apply_dropout != 0: the weights after the attention dropout of that forward (its mask, kept elements times 1 / (1 - p), what the
 * reference returns in training mode); no effect when that forward's attention dropout was 0.  The probability and seed are the ones
 * gget_set_dropout holds: as for the backward, do not change them between the forward and this call.
 * One stated difference: the rows of padding queries (q >= the sample's length; a packed token without keys) read as ZERO, where the
 * reference returns a softmax of meaningless queries that nothing consumes (gget_hidden_states_grid follows the same rule).
 * Error (text in gget_last_error) and no launch: no valid forward on the handle, `layer` outside [0, num_layers). */
int gget_attention_probs(gget_handle_t h, int layer, void* out_dev, int apply_dropout, void* stream);
/* replaces: the query_states / key_states / value_states of hf LlamaAttention.forward (modeling_llama.py:243-281) behind
 * apply_rotary_pos_emb, of decoder layer `layer` of the last forward: a COPY of the layer's q | k | v (q and k rotated) in the
 * [B, S, 3 hidden] layout (q | k | v, head h at column h * 64 of each third), after a forward on either token layout; zeros behind a
 * sample's tokens.  The twin of gget_hidden_states_grid for the operands of gget_attention_probs.  out_dev: bf16 [B * S * 3 * hidden]. */
int gget_layer_qkv_grid(gget_handle_t h, int layer, void* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Operator-level entry points (the individual HIP kernels), used by the parity tests and by
 * callers that only want one op.  bf16 tensors unless stated; row-major; ld* in elements.
 * ------------------------------------------------------------------------------------------ */
#define GGET_GEMM_NT 0 /* C[M,N] = A[M,K] * B[N,K]^T   (forward  y = x W^T) */
#define GGET_GEMM_NN 1 /* C[M,N] = A[M,K] * B[K,N]     (dgrad    dx = dy W) */
#define GGET_GEMM_TN 2 /* C[M,N] = A[K,M]^T * B[K,N]   (wgrad    dW = dy^T x) */
#define GGET_EPI_NONE 0
#define GGET_EPI_RESIDUAL 1 /* C = A*B + R (R bf16 [M,N], ldr = ldc) */
#define GGET_EPI_ATOMIC_F32 2 /* C is fp32, C += A*B with atomics (split-K) */
#define GGET_EPI_ROPE 4 /* C = rope(A*B) on columns [0, rope_cols): RoPE fused into the q|k|v projection (engine only) */
#define GGET_EPI_SLAB_F32 3 /* C is fp32 [split_k][M][ldc]: slice s of K writes slab s (reduced by the caller) */
#define GGET_EPI_GEGLU_FWD 5 /* gate|up projection with the gated-GELU product fused into the epilogue (gget_op_gateup_geglu) */
#define GGET_EPI_GEGLU_BWD 6 /* dh = dy W_down with the gated-GELU backward fused into the epilogue (gget_op_down_dgrad_geglu) */
int gget_op_gemm(int mode, int epilogue, const void* A, const void* B, void* C, const void* R, int M, int N, int K,
                 int lda, int ldb, int ldc, int split_k, void* stream);
/* the same contraction with stream-K allowed (csrc/gemm.h): `streamk_ws` = gget_op_gemm_streamk_bytes() of device memory zeroed ONCE by
 * the caller and reusable by later calls on the same stream; launches whose tile count is no multiple of the CU count then cut the
 * K range of their boundary tiles between neighbouring workgroups (fp32 partial tiles through the workspace).  The engine does this
 * by itself with a slice of its workspace arena. */
int gget_op_gemm_streamk(int mode, int epilogue, const void* A, const void* B, void* C, const void* R, int M, int N, int K,
                         int lda, int ldb, int ldc, void* streamk_ws, void* stream);
uint64_t gget_op_gemm_streamk_bytes(void);
/* up to 4 independent GEMMs of one mode in ONE persistent launch (plain bf16 epilogue): how the engine issues the four
 * weight gradients of a decoder layer (dW = dY^T X for gate|up, down, q|k|v, o: hf LlamaMLP / LlamaAttention Linear backward) -
 * exactly 256 tiles of 192x192 for d = 768, one per CU */
int gget_op_gemm_grouped(int mode, int count, const void* const* A, const void* const* B, void* const* C, const int* M,
                         const int* N, const int* K, const int* lda, const int* ldb, const int* ldc, void* stream);
/* measurement knobs (tools/ and tests; no reference counterpart): the process launch menu, one row per knob in csrc/menu.h kMenuRows
 * (INTEGRATION.md "Kernel-selection knobs" lists them).  The environment sets the initial values when the library loads; these two read and
 * write a knob by its key afterwards, and a value written before the first launch holds.  Both return 2 and set gget_last_error for a key
 * that is not in the table.
 * key 1 = bit mask of GEMM kernel variants, 0 = the shipped selection.  Bits that switch a variant OFF: 1 kGemmNoKsplitNd (the K-split
 *   kernel for one-round N = d launches), 2 kGemmNoKsplitWgrad (the K-split kernel for the grouped weight gradients), 4 kGemmNo192Rows (the
 *   192-row tiles), 8 kGemmNoSplitLast (the split of the last round), 16 kGemmKsplit128Only (the 64- / 96-row tiles of the K-split kernel),
 *   32 kGemmOneBlockPerCu (two co-resident workgroups per CU for the dh + GEGLU' launch).  Bits that switch a variant ON: 128
 *   kGemmKsplitDma8 (all eight waves of the K-split kernel issue its LDS-DMA), 512 kGemmAreaRule (N = d launches keep the default tiling
 *   whenever its rounds x area is the smaller one).
 * key 2 = LDS headroom of the 128x192 / 192x128 tiles: 1 (default) 3-slot rings, 0 4-slot rings, 2 also no launch with two LDS-filling
 *   workgroups per CU.
 * key 3 = 1: split the K range of the last, partial round's tiles among the idle workgroups (off by default).
 * key 4 = 1 (also env GGET_DETERMINISTIC=1): reproducible mode of the pre-train step - the RMSNorm weight gradients, the one sum of that
 *   gradient path added with fp32 atomics, are summed in block order instead (same kernel selection, the per-sample kernels included); two
 *   runs then produce bit-identical parameters.
 * key 5 = start delay, in 100 MHz ticks, of a CU's second workgroup in the two-per-CU GEMM launches.  key 7 = GEMM ablation bits (timing
 *   only; 0 = none).  key 8 = 1: the dense SMTP head.  key 9 = 128 / 256: its slot tile rows.
 * key 10 = 1: the per-sample kernels of S <= 32 off (the three launches each replaces run).  key 11 = 1: the fused RMSNorm + LayerScale
 *   backward in its 16-byte-chunk form for every width (0: the 8-byte, all-lanes form for d = 512 / 768 / 1024).
 * key 13 = 0: the RMSNorm backward of short launches (<= 64 rows per CU) in 4-wave blocks as everywhere else (1, default: one 16-wave block
 *   per CU, same bits).  key 14 = 0: the engine's cross-entropy launch adds its loss with one atomic per block (1, default: one partial sum
 *   per block, summed in block order by the finalising launch).  key 15 = R: every GEMM launch plan counts the device's CUs minus R (0,
 *   default: the whole chip; a data-parallel handle sets its own with gget_set_dp_menu).  key 16 = 1: gget_debug_occupy's stand-in takes
 *   the register footprint of RCCL's kernel (264 registers per lane) besides the LDS asked for.  key 19 = 1: the cross-entropy launch never
 *   takes the row-in-registers kernels (what the presence of GGET_CE_GENERIC selects at load).  key 20 = 1: the embedding backward always
 *   as the sorted scatter-add, never the count-matrix product (what the presence of GGET_EMBED_SORTED selects at load). */
int gget_debug_set(int key, int value);
int gget_debug_get(int key, int* value);
/* measurement aid: with enable != 0 the engine brackets, with HIP events on the launch stream, the grouped weight-gradient launch
 * (avg_ms_out[0]) and the gate|up + GEGLU launch (avg_ms_out[1]) of every layer of the following forward / backward calls;
 * avg_ms_out (may be NULL) receives the mean durations recorded so far.  bench.py uses it for the roofline of the dominant kernel
 * as it runs INSIDE a step. */
int gget_debug_probe(gget_handle_t h, int enable, float* avg_ms_out);
/* measurement aid behind bench.py's time-weighted GEMM figure (no reference counterpart).  enable = 1: start recording every GEMM
 * launch of the process between HIP events; enable = 0: stop and report the sum of the algorithmic FLOPs (2 M N K) and of the
 * durations of the recorded launches, how many were summed and how many were left out (row / K counts that live on the device) */
int gget_debug_gemm_probe(int enable, double* flops_out, double* ms_out, int* launches_out, int* skipped_out);
/* measurement aid (tools/coresidency.py; no reference counterpart): occupies `blocks` CU slots (256 threads, lds_bytes of LDS
 * each) for ~microseconds on `stream`, as a stand-in for a collective's kernel running beside the compute stream */
int gget_debug_occupy(void* scratch, uint64_t scratch_bytes, int blocks, int lds_bytes, int microseconds, void* stream);
/* replaces: q_proj/k_proj/v_proj + apply_rotary_pos_emb (hf LlamaAttention.forward :253-262, :138-160) as ONE GEMM:
 * qkv[T,3d] = x[T,d] * wqkv[3d,d]^T with RoPE applied to the q|k columns in the fp32 accumulators (position of row t is
 * position_ids[t], or t % S when position_ids is NULL; cos/sin tables [max_position][32] fp32). */
int gget_op_qkv_rope(const void* x, const void* wqkv, void* qkv, const float* cos_tab, const float* sin_tab,
                     const int64_t* position_ids, int T, int S, int d, void* stream);
/* replaces: prepare_for_2d_smtp_inputs_labels (src/models/graphgpt/modeling_helpers.py:399-449) as called by
 * GraphGPTPretrainBase.forward when config.smtp_inside (modeling_pretrain.py:175-189): per-sample mask rate r ~ U, a cell
 * (node, feature) is masked when U > r^power (looked up through node_idx), masked ids -> 1, labels = original id or -100,
 * optional replacement of masked cells by id + round(10 * N(0,1)) mod vocab.  ids_in [B,S,ld_in] (first F columns are
 * used), node_idx [B,S] with element stride ld_node, outputs dense [B,S,F].  Draws are a counter hash of `seed`
 * (graph-gpt_amd/smtp.py is the bit-exact Python twin). */
int gget_op_smtp2d(const int64_t* ids_in, int ld_in, const int64_t* node_idx, int ld_node, int64_t* ids_out, int64_t* labels_out,
                   int B, int S, int F, float smtp_2d_rate, float power, float replace_rate, int vocab, int global_2d_mask,
                   uint32_t seed, void* stream);
/* replaces: sample_tokens at temperature 0 (src/utils/generation_utils.py:45-82) inside the unmasking loop
 * (_batch_unmask_without_for_loop :139-237): per row of bf16 logits [R, ld] (V valid columns) the arg-max token and its
 * confidence: mode 0 max softmax probability ("maskgit_plus"), 1 top1 - top2 probability ("topk_margin"),
 * 2 sum p log(p + 1e-10) ("entropy").  Ties resolve to the lowest index. */
#define GGET_CONF_MAXPROB 0
#define GGET_CONF_MARGIN 1
#define GGET_CONF_NEG_ENTROPY 2
int gget_op_token_confidence(const void* logits, int ld, int R, int V, int mode, float* conf, int64_t* tok, void* stream);
/* replaces: sample_tokens with every option (src/utils/generation_utils.py:22-82: temperature, top-p, top-k, categorical
 * sampling, margin / entropy confidence) and the Gumbel-max perturbation of the confidence ranking (:199-209, alg_temp).
 * temperature 0 = arg-max; top_p outside (0,1) and top_k 0 = filter off; alg_temp 0 = no perturbation.  Draws: counter hash
 * of (seed, stream, row) (graph-gpt_amd/generation.py holds the Python twin); V <= 8192. */
int gget_op_token_sample(const void* logits, int ld, int R, int V, int mode, float temperature, float top_p, int top_k,
                         float alg_temp, uint32_t seed, float* conf, int64_t* tok, void* stream);
/* test-only: gget_op_token_sample that also shows the distribution the candidate is drawn from - probs f32 [R, ld_p], ld_p >= V, takes
 * every row's probabilities after the filters (a filtered token: +0); columns [V, ld_p) are not written.  probs NULL: nothing is written
 * and conf / tok are gget_op_token_sample's. */
int gget_op_token_sample_probs(const void* logits, int ld, int R, int V, int mode, float temperature, float top_p, int top_k,
                               float alg_temp, uint32_t seed, float* conf, int64_t* tok, float* probs, int ld_p, void* stream);
/* replaces: the alg = "origin" update of _batch_unmask_without_for_loop (src/utils/generation_utils.py:150-162): x[b][n] takes
 * cand[b][n] where it is <mask> and the cell's own uniform draw is below p_transfer. */
int gget_op_unmask_origin(int64_t* x, const int64_t* cand, int B, int N, float p_transfer, uint32_t seed, int mask_token_id,
                          void* stream);
/* replaces: the alg = "origin" update of sample_per_example (src/utils/generation_utils.py:379-392) for a whole batch whose samples
 * each walk their own time grid: as gget_op_unmask_origin with p_transfer[b] (f32 [B], device) read per sample. */
int gget_op_unmask_origin_rows(int64_t* x, const int64_t* cand, int B, int N, const float* p_transfer, uint32_t seed,
                               int mask_token_id, void* stream);
/* replaces: the confidence-ranked update - confidence[~mask] = -inf, torch.topk, gather, where, scatter_ of
 * _batch_unmask_without_for_loop (src/utils/generation_utils.py:197-236) and the topk / index write of sample_per_example
 * (:402-433).  x i64 [B,N] in place, conf f32 [B,N], cand i64 [B,N]; p f32 on the device, read at p[b * p_stride] (p_stride 0: one
 * value for the batch, 1: one per sample); n_revealed i32 [B] or NULL.  One workgroup per sample: n = (int)floorf((float)n_masked * p)
 * (one fp32 multiply, = torch.floor(n_masked * p).int() and int(num_mask_token * (1 - s / t))), then cand is written into the n masked
 * cells of largest confidence, ties to the lower cell index (torch.sort(descending=True, stable=True)); -0.0 == +0.0; unmasked cells
 * are neither ranked nor written; confidences of masked cells must not be NaN.  Any N >= 0 (radix select over the row, no LDS per cell). */
int gget_op_unmask_ranked(int64_t* x, const float* conf, const int64_t* cand, int B, int N, int mask_token_id, const float* p,
                          int p_stride, int32_t* n_revealed, void* stream);
/* replaces: the step rule of _batch_unmask_without_for_loop (src/utils/generation_utils.py:171-184) with its two .item() reads.
 * p_tab f32 [steps] (device) holds 1 - t[i+1] / t[i], last entry 1; state_i (device word) holds i.  From m = max_b n_masked[b] the
 * kernel advances i while i < steps until floorf(m * p_tab[i]) >= 1, stores i back, the p of the last rule iteration (0 when none
 * ran: nothing masked, or i == steps) into p_word (device), and {i, any cell masked} into host_pair: two int32 of PINNED host memory,
 * valid once the stream has passed the launch. */
int gget_op_gen_plan(const int64_t* x, int B, int N, int mask_token_id, const float* p_tab, int steps, int32_t* state_i, float* p_word,
                     int32_t* host_pair, void* stream);
/* replaces: the counts behind cal_gen_acc_batch / cal_gen_acc_per_sample (src/utils/generation_utils.py:439-463): counts i32 [B,2] =
 * {sum (gen == labels) & (input_ids == mask), sum (input_ids == mask)} over the N cells of every sample (all i64 [B,N]). */
int gget_op_gen_acc(const int64_t* gen, const int64_t* labels, const int64_t* input_ids, int B, int N, int mask_token_id,
                    int32_t* counts, void* stream);
/* replaces: the collator's SMTP masking (prepare_inputs_for_pretrain_mlm, src/utils/tokenizer_utils.py:259-271 polynomial
 * schedule + _mask_stacked_input_ids_v2 :112-148, mtp (1,0,0)) for a right-padded batch ids [B,S,F] with lengths [B]:
 * per sample t = umr_min + (umr_max - umr_min) U, exactly ceil(len*F*(1 - t^power)) of its cells are masked (id -> 1
 * unless pad, label = original id; all other labels -100); optional wgt_out[b] = power / t (dlm_wgt).  Draws are a
 * counter hash of `seed` (graph-gpt_amd/smtp.py holds the bit-exact twin). */
int gget_op_smtp_rows(const int64_t* ids_in, const int32_t* lengths, int64_t* ids_out, int64_t* labels_out, float* wgt_out, int B,
                      int S, int F, double umr_min, double umr_max, double power, uint32_t seed, void* stream);
int gget_op_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int T, int d, float eps, void* stream);
int gget_op_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* dres,
                        void* dx, float* dw_accum, int T, int d, void* stream);
/* the element-wise entries (embed, rope, geglu) check their shapes on the host and return an error before any launch: non-NULL pointers,
 * d > 0 and d % 8 == 0, F >= 1, ldF >= F, V >= 1, H >= 1, S >= 1, ff > 0 and ff % 8 == 0 */
int gget_op_embed_fwd(const int64_t* ids, const void* emb, const void* gate, void* out, int T, int F, int ldF,
                      int d, void* stream);
/* demb_accum [V][d] (and dgate_accum [F][d] with a gate) fp32 are ADDED to, in the sorted scatter-add and in the count-matrix form alike;
 * the pad_id row receives nothing */
int gget_op_embed_bwd(const int64_t* ids, const void* dx, const void* emb, const void* gate, float* demb_accum,
                      float* dgate_accum, int T, int F, int ldF, int d, int V, int pad_id, void* stream);
int gget_op_rope(void* qkv, const float* cos_tab, const float* sin_tab, const int64_t* position_ids, int B, int S,
                 int H, int inverse, void* stream);
/* (head_dim 64 in these entries; either width: the _hd forms below.)
 * cos_tab/sin_tab ([max_pos][32] fp32, hf LlamaRotaryEmbedding tables) non-NULL: RoPE (hf apply_rotary_pos_emb
 * :138-160) is applied to q,k inside the kernels and undone on dq,dk; qkv / dqkv are the UN-rotated projections.
 * dropout_p > 0: attention dropout on the softmax output (hf eager_attention_forward :210), counter-based mask
 * keyed by (dropout_seed, batch*head, query, key) - see drop_mul() in csrc/attention.hip.
 *
 * Numerical contract of gget_op_attn_fwd / _bwd and their _varlen, _ranges and _fused forms (what the per-element bounds of
 * tests/_attn_out_ref.py count; head_dim 64, scores x = q k / 8):
 *  - forward: scores, the running maximum, the row sum l and the O accumulator are fp32.  l sums the UNROUNDED, un-dropped p.  P (after the
 *    keep multiplier m = 0 or 1 / (1 - p); the long-sequence kernels drop in P and apply 1 / (1 - p) with 1 / l at the end) is rounded to
 *    bf16 once, as the operand of the P V MFMA.  out = bf16(O / l): one rounding.  lse = fp32 natural log of sum_allowed exp(x), before
 *    dropout; 0 for a query without an allowed key, whose out row is 0.  A query with ONE allowed key and no dropout returns that v row
 *    bit for bit.  With RoPE on load the rotated q / k are rounded to bf16 before the score MFMA.
 *  - backward: p = exp(x - lse) is recomputed in fp32 from the lse handed in.  dP = dO V^T is fp32.  delta is the softmax-backward row
 *    term: rowsum(dO * out) in fp32 from the bf16 out handed in - in the dQ kernels of the two-kernel forms, which leave it in delta_ws
 *    for the dK / dV kernel, and in the first launch of the fused form - or, where one launch holds a whole row (one key length per row and S <= 32, or
 *    S <= 64 without RoPE on load: these do not read out or delta_ws), sum_k m p dP from registers.  dS = p (m dP - delta) / 8 is rounded to bf16
 *    once, as the operand of both dQ = dS K and dK = dS^T Q; P (times m) is rounded to bf16 once, as the operand of dV = P^T dO; the
 *    accumulators are fp32 and dq, dk, dv are rounded to bf16 once.  The fused form (S >= 256) rounds the dQ partial of every block of 256
 *    keys to bf16 (its slab of dq_ws) and sums the slabs in fp32.  dq / dk are rotated back in fp32 before their rounding.
 *  - delta_ws, dq_ws: workspaces, contents irrelevant on entry; rows of delta_ws behind a sample's tokens are not read.
 *  - pad rows of dqkv.  Padded grid and packed rows: EVERY row is written; the rows without a token (behind key_len[b]; empty key range)
 *    are exact zeros provided dout is zero there and out / lse are the forward's - the q | k | v weight-gradient GEMM sums over all rows.
 *    Var-len layout: only the samples' rows are written; rows behind the last sample are the caller's (the engine zeroes them once). */
int gget_op_attn_fwd(const void* qkv, const int32_t* key_len, void* out, float* lse, int B, int S, int H,
                     int causal, const float* cos_tab, const float* sin_tab, const int64_t* position_ids,
                     float dropout_p, uint32_t dropout_seed, void* stream);
int gget_op_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len,
                     void* dqkv, float* delta_ws, int B, int S, int H, int causal, const float* cos_tab,
                     const float* sin_tab, const int64_t* position_ids, float dropout_p, uint32_t dropout_seed,
                     void* stream);
/* Head-width-parameterised forms of gget_op_rope, the attention forward / backward and gget_op_attn_probs: head_dim 64 or 32 (any other
 * width, a NULL operand, B, S or H <= 0, half a key range, or row_base together with ranges: error 2, "unsupported head_dim" for the width,
 * nothing is launched).  qkv is [rows, 3 * H * head_dim] bf16 with q and k ALREADY rotated (the engine's layout); the tables of the backward
 * ([max_pos][head_dim / 2]) only rotate dq / dk back, NULL tables = no rotation.  Key restriction: key_len (padded layout), key_len +
 * row_base (var-len token layout), key_lo / key_hi (packed rows; key_len is ignored then), causal.  lse fp32 [B, H, S], delta_ws fp32
 * [B, H, S] workspace.  head_dim 64 forwards to the kernels of the entries above with the same arguments (qk_rotated = 1): same bits.
 * head_dim 32 (csrc/attention32.hip, H = hidden / 32) keeps the numerical contract above with x = <q, k> * 32^-1/2: the scale is not a
 * power of two and is applied as ONE fp32 constant fl(32^-1/2 * log2 e) inside p = exp2(fma(s, c, -m2)) (forward and every recomputation
 * of p; lse stays the natural log) and as the fp32 constant fl(32^-1/2) on dS; delta is sum_k m p dP in fp32 from the recomputed p and dP
 * (a first walk of the dQ kernel over the row's key tiles; `out` is not read), left in delta_ws for the dK / dV kernel; the dropout mask is the same counter hash keyed by (seed, b * H + h, q, k >> 1); the pad-row rule is the one above; no
 * atomics.  gget_op_rope_hd at width 32 pairs channel j with j + 16 (hf apply_rotary_pos_emb) in place on bf16 rows, fp32 arithmetic, one
 * rounding.  gget_op_rope_f32_hd (head_dim 32 only) is the engine's form: src fp32 [B S, 3 d] - the q | k | v projection's fp32
 * accumulators, written by the GEMM's fp32 slab epilogue - -> bf16 qkv with the q and k columns rotated and v copied, each element
 * rounded ONCE: the cast points of the 64-wide projection, whose RoPE epilogue rotates the accumulators before their rounding. */
int gget_op_rope_f32_hd(const float* src, void* qkv, const float* cos_tab, const float* sin_tab, const int64_t* position_ids, int B, int S,
                        int H, int head_dim, void* stream);
int gget_op_rope_hd(void* qkv, const float* cos_tab, const float* sin_tab, const int64_t* position_ids, int B, int S, int H, int head_dim,
                    int inverse, void* stream);
int gget_op_attn_fwd_hd(const void* qkv, const int32_t* key_len, const int32_t* row_base, const int32_t* key_lo, const int32_t* key_hi,
                        void* out, float* lse, int B, int S, int H, int head_dim, int causal, float dropout_p, uint32_t dropout_seed,
                        void* stream);
int gget_op_attn_bwd_hd(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len, const int32_t* row_base,
                        const int32_t* key_lo, const int32_t* key_hi, void* dqkv, float* delta_ws, int B, int S, int H, int head_dim,
                        int causal, const float* cos_tab, const float* sin_tab, const int64_t* position_ids, float dropout_p,
                        uint32_t dropout_seed, void* stream);
int gget_op_attn_probs_hd(const void* qkv, const float* lse, const int32_t* key_len, const int32_t* row_base, const int32_t* key_lo,
                          const int32_t* key_hi, void* out, int B, int S, int H, int head_dim, int causal, float dropout_p,
                          uint32_t dropout_seed, void* stream);
/* replaces: the `.to(device)` calls at the top of the reference's step (src/utils/training_utils.py:17-26) for a batch that sits in PINNED
 * host memory (hipHostMalloc / torch pin_memory: device-mapped): a kernel on `stream` reads it over the host link into dst_dev.  Stays in
 * the compute queue - an in-stream hipMemcpyAsync from pinned memory is a copy-engine job whose dependencies the runtime resolves on the
 * host (four per step: the C1 step 6.7 -> 12 - 20 ms).  Both pointers 16-byte aligned; the host buffer must stay untouched until the
 * kernel has run (record an event behind it).  graph-gpt_amd/training.py DevicePrefetcher is the caller. */
int gget_op_copy_from_host(const void* src_pinned_host, void* dst_dev, uint64_t bytes, void* stream);
/* The two above on the padding-free (var-len) token layout: row_base (int32 [B]) = first row of sample b in the token-major buffers
 * (qkv / out / dout / dqkv hold the samples' real rows back to back, key_len[b] of them for sample b); lse / delta keep their [B, H, S]
 * indexing, S = the padded width the collator produced (8 * ceil(longest graph / 8), reference src/data/collator.py:70-111).  Every
 * sample is processed by its OWN row count: blocks behind a sample's rows exit at once, and the backward for S <= 64 is one launch whose
 * waves take one 32-row tile or - a sample of 33 .. 64 rows - 2 x 2 tiles (csrc/attention.hip: attn_bwd_small_kernel).  qk_rotated != 0:
 * q and k in qkv are rotated already (the engine's layout); the tables then only rotate dq / dk back. */
int gget_op_attn_fwd_varlen(const void* qkv, const int32_t* key_len, const int32_t* row_base, void* out, float* lse, int B, int S, int H,
                            int causal, const float* cos_tab, const float* sin_tab, const int64_t* position_ids, int qk_rotated,
                            float dropout_p, uint32_t dropout_seed, void* stream);
int gget_op_attn_bwd_varlen(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len,
                            const int32_t* row_base, void* dqkv, float* delta_ws, int B, int S, int H, int causal, const float* cos_tab,
                            const float* sin_tab, const int64_t* position_ids, int qk_rotated, float dropout_p, uint32_t dropout_seed,
                            void* stream);
/* S <= 32 (graph sequences of PCQM4M-v2): attention of every head of a sample, the o projection + residual add and the RMSNorm behind
 * it in ONE launch, one workgroup per sample (csrc/attention.hip: attn_oproj_fwd_kernel).  replaces, for one decoder layer:
 * hf LlamaAttention.forward :243-281 (attention on rotated q / k + o_proj), LlamaDecoderLayer.forward :305-316 (residual add,
 * post_attention_layernorm = LlamaRMSNorm.forward :62-67).  wo_packed: the FRAGMENT-MAJOR copy of o_proj.weight [d][d] written by
 * gget_op_pack_wo (its `fwd` output; the 64 lanes' 16-byte pieces of one 16 x 32 MFMA operand are contiguous - in the weight's row-major
 * layout a fragment load is 64 separate 16-byte requests and the launch runs at 10 B/clk per CU).
 * qkv [rows, 3 * 64 H] bf16 with q / k ALREADY rotated (the engine's layout);
 * row_base (int32 [B], may be NULL): first row of sample b in the token-major buffers (var-len layout; then key_len[b] rows belong to it),
 * NULL = padded layout, sample b at rows [b S, b S + S).  Outputs: attn_out [rows, d] bf16, lse fp32 [B, H, S] (natural log), x_mid =
 * x_in + attn_out Wo^T (bf16, residual added on the fp32 accumulator: one rounding), xn = norm_w * bf16(x_mid * rstd) and rstd fp32 [rows].
 * *taken = 1 when the fused form ran; 0 when the shape is not covered (S > 32, H not in {2, 4, 8, 12}, GGET_ATTN_OPROJ=0) - nothing
 * is written then and the caller runs gget_op_attn_fwd, a GEMM and gget_op_rmsnorm_fwd. */
int gget_op_attn_oproj_fwd(const void* qkv, const int32_t* key_len, const int32_t* row_base, void* attn_out, float* lse, const void* wo_packed,
                           const void* x_in, void* x_mid, const void* norm_w, void* xn, float* rstd, int B, int S, int H, int causal,
                           float eps, float dropout_p, uint32_t dropout_seed, void* stream, int32_t* taken);
/* fwd[((T KS + s) 64 + lane) 8 + e] = w[16 T + lane % 16][32 s + 8 (lane / 16) + e], KS = d / 32; bwd: the same of w transposed.
 * `layers` weights, `layer_stride` elements apart in w, are packed back to back ([layers][d][d] each output).  d % 64 == 0. */
int gget_op_pack_wo(const void* w, uint64_t layer_stride, void* fwd, void* bwd, int d, int layers, void* stream);
/* The backward counterpart of gget_op_attn_oproj_fwd, one workgroup per sample (csrc/attention.hip: attn_oproj_bwd_kernel): RMSNorm
 * backward of post_attention_layernorm - dx_mid = dres + rstd (dxn w - xhat mean(dxn w xhat)), dw_accum[j] += sum_rows dxn xhat (fp32,
 * `copies` replicas `copy_stride` floats apart, as gget_op_rmsnorm_bwd's) - then dattn = dx_mid Wo (never written to memory) and the
 * attention backward of every head: dqkv [rows, 3 d] with dq / dk rotated BACK by cos_tab / sin_tab / position_ids (NULL tables: no
 * rotation).  wot_packed = gget_op_pack_wo's `bwd` output.  t_rows = rows of the token-major buffers (var-len layout: dx_mid of the pad
 * rows behind the last sample is zeroed).  *taken as above.  In the reproducible mode (gget_debug_set(4, 1)) the norm-weight gradient
 * goes through one zeroed row per sample, summed in block order into dw_accum's first copy.
 * Var-len layout (row_base != NULL) with 32 < S <= 64: every sample by its own row count.  A sample of 33 .. 64 rows takes the first two
 * steps in its workgroup, over two row tiles; its dattn rows go to dattn_long (bf16 [t_rows, d]; rows of other samples are not touched;
 * NULL: the launch is not taken for S > 32) and a second launch on the same stream (attn_bwd_long_kernel) does its attention backward. */
int gget_op_attn_oproj_bwd(const void* dxn, const void* x_mid, const void* norm_w, const float* rstd, const void* dres, void* dx_mid,
                           float* dw_accum, int copies, uint64_t copy_stride, const void* wot_packed, const void* qkv, const float* lse,
                           const int32_t* key_len, const int32_t* row_base, void* dqkv, int B, int S, int H, int causal, const float* cos_tab,
                           const float* sin_tab, const int64_t* position_ids, float dropout_p, uint32_t dropout_seed, int t_rows,
                           void* stream, int32_t* taken, void* dattn_long);
/* gget_op_attn_bwd_varlen and gget_op_attn_oproj_bwd in the engine's launch form for 32 < S <= 64: long_list (int32 [3 B + 1], may be NULL)
 * is what gget_op_varlen_plan wrote - [0] the number n of 33 .. 64-row samples, [1 ..] their indices, [1 + B ..] their first rows,
 * [1 + 2 B ..] their row counts.  attn_bwd_long_kernel then runs at most 32 block slots per head that walk the list with the grid's stride
 * instead of one block per sample.  NULL: exactly the entries above.  Same results, bit for bit. */
int gget_op_attn_bwd_varlen_list(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len,
                                 const int32_t* row_base, void* dqkv, float* delta_ws, int B, int S, int H, int causal, const float* cos_tab,
                                 const float* sin_tab, const int64_t* position_ids, int qk_rotated, float dropout_p, uint32_t dropout_seed,
                                 void* stream, const int32_t* long_list);
int gget_op_attn_oproj_bwd_list(const void* dxn, const void* x_mid, const void* norm_w, const float* rstd, const void* dres, void* dx_mid,
                                float* dw_accum, int copies, uint64_t copy_stride, const void* wot_packed, const void* qkv, const float* lse,
                                const int32_t* key_len, const int32_t* row_base, void* dqkv, int B, int S, int H, int causal,
                                const float* cos_tab, const float* sin_tab, const int64_t* position_ids, float dropout_p,
                                uint32_t dropout_seed, int t_rows, void* stream, int32_t* taken, void* dattn_long, const int32_t* long_list);
/* attention with a per-token inclusive key range [key_lo, key_hi] (int32 [B,S]; packed rows) instead of one length per
 * batch row; gget_op_ranges_from_mask3d derives the ranges from a block-diagonal int64 [B,S,S] mask. */
int gget_op_attn_fwd_ranges(const void* qkv, const int32_t* key_lo, const int32_t* key_hi, void* out, float* lse, int B, int S,
                            int H, int causal, float dropout_p, uint32_t dropout_seed, void* stream);
int gget_op_attn_bwd_ranges(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_lo,
                            const int32_t* key_hi, void* dqkv, float* delta_ws, int B, int S, int H, int causal,
                            float dropout_p, uint32_t dropout_seed, void* stream);
int gget_op_ranges_from_mask3d(const int64_t* mask3d, int32_t* key_lo, int32_t* key_hi, int B, int S, void* stream);
/* replaces: the attn_weights hf eager_attention_forward returns (modeling_llama.py:191-214: softmax of the masked scores in fp32, cast, then
 * dropout) - the operator behind gget_attention_probs with every argument:
 *   out[b,h,q,k] = bf16(m * exp(<q_bhq, k_bhk> / 8 - lse[b,h,q])) for an allowed key, 0 otherwise;  out bf16 [B, H, S, S], all written.
 * qkv holds ROTATED q | k (the engine's layout; v is not read), [B * S, 3 * 64 H] or - row_base != NULL, int32 [B] - the var-len token
 * layout of gget_op_attn_fwd_varlen.  lse: f32 [B, H, S] as every forward entry writes it - the NATURAL log of sum_k exp(score / 8) over
 * the allowed keys, before dropout.  Allowed keys: k < key_len[b] for queries q < key_len[b] (key_len NULL = S), k <= q when causal;
 * or - key_lo / key_hi != NULL, int32 [B, S], packed rows - key_lo[b,q] <= k <= key_hi[b,q] (an empty range gives a zero row).
 * m = 1 for dropout_p = 0, else the keep multiplier 0 or 1 / (1 - p) of the forward run with the same (dropout_p, dropout_seed).
 * MFMA scores with fp32 accumulation, fp32 exponent, one rounding to bf16; no atomics (reruns are bit-identical).  NULL qkv / lse / out,
 * B, S or H <= 0 and half a key range are errors and launch nothing. */
int gget_op_attn_probs(const void* qkv, const float* lse, const int32_t* key_len, const int32_t* row_base, const int32_t* key_lo,
                       const int32_t* key_hi, void* out, int B, int S, int H, int causal, float dropout_p, uint32_t dropout_seed,
                       void* stream);
/* gget_op_attn_bwd / _ranges (no RoPE) through the ONE-PASS long-sequence backward (S >= 256; shorter rows run the usual kernels and leave
 * the workspace alone): S, dP and the softmax backward are evaluated once, dK / dV and dQ come out of the same pass (5 matmuls of hf
 * eager_attention_forward's autograd graph, modeling_llama.py:191-214, instead of the 7 of the two-kernel form).  dq_ws: bf16
 * [ceil(S / 256)][B * S][H * 64] scratch (contents irrelevant on entry): every block of 256 keys writes its dQ partials into its own
 * slab, the last launch sums the slabs in fp32 in block order - reproducible - into the q part of dqkv.
 * key_lo / key_hi both NULL: one key length per row (key_len, may be NULL = S). */
int gget_op_attn_bwd_fused(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len,
                           const int32_t* key_lo, const int32_t* key_hi, void* dqkv, float* delta_ws, void* dq_ws, int B, int S,
                           int H, int causal, float dropout_p, uint32_t dropout_seed, void* stream);
/* replaces: LlamaMLP.forward (hf :174-176) up to the down projection, as ONE GEMM with the gated-GELU product in its
 * epilogue: gu[T,2ff] = x[T,d] * wgu[2ff,d]^T (gate | up pre-activations, kept for the backward),
 * h[T,ff] = bf16(gelu(gate)) * up.  Falls back to GEMM + gget_op_geglu_fwd when ff % 128 != 0. */
int gget_op_gateup_geglu(const void* x, const void* wgu, void* gu, void* h, int T, int d, int ff, void* stream);
/* backward counterpart: dgu[T,2ff] = (dh * up * gelu'(gate) | dh * gelu(gate)) with dh = dy[T,d] * wdown[d,ff] computed in
 * the same launch and never stored (dh_scratch [T,ff] is only used by the un-fused fallback, may be NULL when ff % 128 == 0) */
int gget_op_down_dgrad_geglu(const void* dy, const void* wdown, const void* gu, void* dgu, void* dh_scratch, int T, int d, int ff,
                             void* stream);
int gget_op_geglu_fwd(const void* gu, void* h, int T, int ff, void* stream);
int gget_op_geglu_bwd(const void* gu, const void* dh, void* dgu, int T, int ff, void* stream);
int gget_op_ce_fwd_bwd(const void* logits, int ld, const int32_t* labels, const float* row_wgt, const int32_t* n_rows_dev,
                       int n_rows_cap, int V, float* loss_sum, void* dlogits, float grad_scale_base, int mean_over_rows,
                       void* stream);

/* ---- test-only entries of the RMSNorm and cross-entropy kernel families: the launcher with every argument, no arithmetic of their own ---- */
/* gget_op_rmsnorm_bwd with the replicated accumulator: block b adds its weight-gradient partial to dw_accum[(b % copies) * copy_stride + j]
 * (dw_accum: copies * copy_stride floats, copy_stride >= d; the weight gradient is the sum of the replicas).  In the reproducible mode
 * (gget_debug_set(4, 1)) the sum goes into the first replica in block order. */
int gget_op_rmsnorm_bwd_copies(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx, float* dw_accum,
                               int T, int d, int copies, uint64_t copy_stride, void* stream);
/* the weight gradient of gget_op_rmsnorm_bwd_copies alone: dw[j] += sum_r dy[r,j] * (x[r,j] * rstd[r]); no dx.  In the reproducible mode
 * the bits are those of the full backward's 4-wave form. */
int gget_op_rmsnorm_dw(const void* dy, const void* x, const float* rstd, float* dw_accum, int T, int d, int copies, uint64_t copy_stride,
                       void* stream);
/* out = bf16(res + bf16(lam * y)) (lam bf16 [d] or NULL = 1), then xn = w * bf16(out * rstd), rstd[r] = rsqrt(mean(out[r]^2) + eps) on the
 * ROUNDED out, in one launch; DropPath and element dropout off.  d % 8 == 0, d <= 2048. */
int gget_op_ls_rmsnorm_fwd(const void* res, const void* y, const void* lam, void* out, const void* w, void* xn, float* rstd, int T, int d,
                           float eps, void* stream);
/* the layout gget_op_rmsnorm_bwd_ls accumulates into: *copies replicas (kAccumCopies), *copy_stride = align_up(d, 128) floats apart */
int gget_op_accum_layout(int d, int* copies, uint64_t* copy_stride);
/* RMSNorm backward fused with the LayerScale backward behind it: dx = bf16(dres + rstd (dy w - xhat mean(dy w xhat))) (dres may be NULL),
 * dsc = bf16(lam * dx) on the rounded dx (lam may be NULL = 1), dw_accum += sum_r dy xhat, dlam_accum += sum_r dx y (dlam_accum may be
 * NULL); dropout off.  BOTH accumulators are [kAccumCopies][align_up(d, 128)] floats (gget_op_accum_layout returns the two numbers); the
 * gradient is the sum of the replicas. */
int gget_op_rmsnorm_bwd_ls(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx, float* dw_accum,
                           const void* y, const void* lam, void* dsc, float* dlam_accum, int T, int d, void* stream);
/* The dropout / DropPath / LayerScale family with its masks on (tests/test_gpu_drop.py).  The mask arguments are the same everywhere:
 *  - elem_p, elem_seed, elem_rows: element dropout.  Element (a, b) of stream s is dropped when the 24-bit hash of (elem_seed, s, a, b) is
 *    BELOW (unsigned)(elem_p * 2^24); a kept one is multiplied by 1 / (1 - elem_p).  a = elem_rows[t] (int32 [T], the logical row of compact
 *    row t) or t when elem_rows is NULL; elem_p <= 0: off.
 *  - path_rate, path_seed, path_S, path_row_b: DropPath per SAMPLE path_row_b[t] (int32 [T]) or t / path_S when path_row_b is NULL: the
 *    sample's rows are multiplied by 0 when hash24(path_seed, sample) * 2^-24 < path_rate, else by 1 / (1 - path_rate); path_rate <= 0: off.
 * gget_op_ls_rmsnorm_fwd_drop: out = bf16(res + keep * bf16(lam * bf16(y * em))) (stream 50, b = the column), then the norm of out.
 * gget_op_rmsnorm_bwd_ls_drop: dx, dw as gget_op_rmsnorm_bwd_ls; dsc = bf16(lam * keep * dx * em), dlam += sum_t keep * dx * bf16(y * em).
 * gget_op_ls_fwd / gget_op_ls_bwd: the same residual add / its backward as kernels of their own (dy of ls_bwd = the dx above); dlam_accum
 *   has the layout of gget_op_accum_layout or is NULL.
 * gget_op_elem_dropout: x bf16 [T][n] (n % 8 == 0) in place, x = bf16(x * em(stream_id, row, column)); elem_p <= 0 leaves x untouched.
 * gget_op_embed_*_drop: stream 48, a = row * F + f, b = the channel, on the gathered rows before the gate; with a mask the backward is always
 *   the sorted scatter-add.  gget_op_head_linear_*_drop: stream 51 + layer, (a, b) = (b, j) of the activation a; elem_rows is not read. */
int gget_op_ls_rmsnorm_fwd_drop(const void* res, const void* y, const void* lam, void* out, const void* w, void* xn, float* rstd, int T,
                                int d, float eps, float elem_p, uint32_t elem_seed, const int32_t* elem_rows, float path_rate,
                                uint32_t path_seed, int path_S, const int32_t* path_row_b, void* stream);
int gget_op_rmsnorm_bwd_ls_drop(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx, float* dw_accum,
                                const void* y, const void* lam, void* dsc, float* dlam_accum, int T, int d, float elem_p, uint32_t elem_seed,
                                const int32_t* elem_rows, float path_rate, uint32_t path_seed, int path_S, const int32_t* path_row_b,
                                void* stream);
int gget_op_ls_fwd(const void* res, const void* y, const void* lam, void* out, int T, int d, float elem_p, uint32_t elem_seed,
                   const int32_t* elem_rows, float path_rate, uint32_t path_seed, int path_S, const int32_t* path_row_b, void* stream);
int gget_op_ls_bwd(const void* dy, const void* y, const void* lam, void* dsc, float* dlam_accum, int T, int d, float elem_p,
                   uint32_t elem_seed, const int32_t* elem_rows, float path_rate, uint32_t path_seed, int path_S, const int32_t* path_row_b,
                   void* stream);
int gget_op_elem_dropout(void* x, int64_t T, int n, uint32_t stream_id, float elem_p, uint32_t elem_seed, const int32_t* elem_rows,
                         void* stream);
int gget_op_embed_fwd_drop(const int64_t* ids, const void* emb, const void* gate, void* out, int T, int F, int ldF, int d, float elem_p,
                           uint32_t elem_seed, const int32_t* elem_rows, void* stream);
int gget_op_embed_bwd_drop(const int64_t* ids, const void* dx, const void* emb, const void* gate, float* demb_accum, float* dgate_accum,
                           int T, int F, int ldF, int d, int V, int pad_id, float elem_p, uint32_t elem_seed, const int32_t* elem_rows,
                           void* stream);
int gget_op_head_linear_fwd_drop(const void* x, void* a, const void* w, const void* bias, void* y, float* y32, int B, int Din, int Dout,
                                 int layer, float elem_p, uint32_t elem_seed, const int32_t* elem_rows, void* stream);
int gget_op_head_linear_bwd_drop(const float* dy, const void* x, const void* a, const void* w, float* dw, float* dbias, float* dx, int B,
                                 int Din, int Dout, int layer, float elem_p, uint32_t elem_seed, const int32_t* elem_rows, void* stream);
/* gget_op_ce_fwd_bwd with every argument of the launcher: row weight sample_wgt[sel_tok[row] / S] (f32, both NULL = 1) times the focal
 * weight (1 - p_label)^focal_gamma (0 = off); n = min(n_rows_cap, *n_rows_dev) rows (n_rows_dev NULL: n_rows_cap); loss_sum[0] = the
 * weighted sum of the row losses; dlogits bf16 [n_rows_cap, ld] (may be NULL) = (softmax - onehot) * weight * (mean_over_rows ? 1 / n :
 * scale_base) on the first n rows, zeros in the columns V..ld, rows past n untouched; loss_out (may be NULL) = loss_sum * that scale.
 * loss_part (may be NULL; loss_part_cap floats): one partial sum per block instead of an atomic when the row-in-registers kernels run and
 * the grid fits into it. */
int gget_op_ce_full(const void* logits, int ld, const int32_t* labels, const int32_t* sel_tok, const float* sample_wgt, int S,
                    const int32_t* n_rows_dev, int n_rows_cap, int V, float* loss_sum, void* dlogits, float scale_base, int mean_over_rows,
                    float* loss_out, float focal_gamma, float* loss_part, int loss_part_cap, void* stream);

/* ---- test-only entries of the element-wise kernels: the launcher with every argument, no arithmetic of their own ---- */
/* the RoPE angle tables every handle builds at creation: cos / sin [max_pos][32] fp32 of pos * theta^(-2j/64) (angle in fp32) */
int gget_op_rope_table(float* cos_tab, float* sin_tab, int max_pos, float theta, void* stream);
/* config.rope_range: per-token tables cos / sin [B*S][32] of the positions rescaled per row, float(p) * range / float(max_s p + 1), and the
 * identity position list ids[b*S + s] = b*S + s that addresses them */
int gget_op_rope_range_table(const int64_t* pos, float* cos_tab, float* sin_tab, int64_t* ids, int B, int S, float range, float theta,
                             void* stream);
/* out[i] = pos[i] clamped to [0, max_pos); *flag = 1 when any position was clamped, otherwise left as it was */
int gget_op_clamp_positions(const int64_t* pos, int64_t* out, int32_t* flag, int64_t n, int max_pos, void* stream);
/* stack_method = "long", in place: x[t,:] = bf16(x[t,:] * ratio_t), ratio_t = min(1, bf16(1 / (nnz_t + 1e-7f))), nnz_t the non-zero ids among
 * ids[t*ldF .. t*ldF + F); rows with ratio 1 are not written */
int gget_op_embed_long_ratio(const int64_t* ids, void* x, int T, int F, int ldF, int d, void* stream);

/* ---- fine-tune heads and task losses, one launcher each (the kernels gget_forward_task / gget_backward run after the last norm) ---- */
/* logits[b,c] = bf16(hidden[pool_row[b]] . w[c] + bias[c]) as f32 [B,C]; pooled_h (optional) bf16 [B,d] = the gathered rows; bias may be NULL */
int gget_op_score_fwd(const void* hidden, const int32_t* pool_row, const void* w, const void* bias, float* logits, void* pooled_h,
                      int B, int C, int d, void* stream);
/* dw f32 [C,d] += dlogits^T hidden[pool_row], dbias f32 [C] += column sums (NULL: none), dhidden[pool_row[b]] = bf16(dlogits[b] w): dhidden
 * is zeroed by the caller and only the pooled rows are written */
int gget_op_score_bwd(const float* dlogits, const void* hidden, const int32_t* pool_row, const void* w, float* dw, float* dbias,
                      void* dhidden, int B, int C, int d, void* stream);
/* token-level head: logits f32 [T,C] = bf16(hidden[t] . w[c] + bias[c]) on every row; d % 64 == 0 and d <= 1024, else error 2 */
int gget_op_tok_score_fwd(const void* hidden, const void* w, const void* bias, float* logits, int T, int C, int d, void* stream);
/* cross-entropy with ignore_index -100 over the rows: dl f32 [T,C] = softmax - onehot on labelled rows (not yet divided by their number n),
 * zeros elsewhere; stat f32 [4] = {sum of row losses, n, 1/n (0 when n = 0), 0}; loss_out = mean, NaN when n = 0.  rows_map (optional,
 * int32 [T]): row t reads labels[rows_map[t]], and carries no label when rows_map[t] >= n_logical */
int gget_op_tok_ce(const float* logits, const int64_t* labels, float* dl, float* stat, float* loss_out, int T, int C,
                   const int32_t* rows_map, int n_logical, void* stream);
/* with g = bf16(dl * stat[2]): dhidden bf16 [T,d] = bf16(g w) (overwritten), dw f32 [C,d] += g^T hidden, dbias f32 [C] += column sums of g */
int gget_op_tok_score_bwd(const float* dl, const float* stat, const void* hidden, const void* w, float* dw, float* dbias, void* dhidden,
                          int T, int C, int d, void* stream);
/* intra-instance token head (GGET_PROBLEM_TOKEN_CE_INTRA).  Sample b owns the rows row_start[b] .. row_start[b+1] (int32 [B+1]; gaps
 * between samples are allowed: b S on a padded grid) of hidden bf16 [rows,d]; k_b = cls_idx[b] (int64 [B]) clamped into [0, rows_b - C].
 * logits f32 [rows,C]: logits[s,c] = bf16(20 <h^_s, h^_{k_b+c}>), h^ = h / max(|h|, 1e-12), for the rows of every sample (other rows are
 * not written; a sample of fewer than C rows gets zeros).  d % 64 == 0, d <= 1024, 2 <= C <= 64, else error 2 ("unsupported"). */
int gget_op_tok_intra_fwd(const void* hidden, const int32_t* row_start, const int64_t* cls_idx, float* logits, int B, int C, int d,
                          void* stream);
/* with z = 20 bf16(dl * stat[2]) (dl, stat of gget_op_tok_ce): dh^_s = sum_c z[s,c] h^_{k+c}, + sum_s' z[s',c] h^_s' on label row k + c;
 * dhidden bf16 [rows,d] = bf16((dh^ - h^ <h^, dh^>) / max(|h|, 1e-12)), overwritten for the rows of every sample (zeros where nothing
 * flows).  No atomics: two calls give the same bits. */
int gget_op_tok_intra_bwd(const float* dl, const float* stat, const void* hidden, const int32_t* row_start, const int64_t* cls_idx,
                          void* dhidden, int B, int C, int d, void* stream);
/* loss_out[0] and dlogits f32 [B,C] of GGET_PROBLEM_SINGLE_LABEL (labels int64 [B], optional sample_wgt f32 [B]), _REGRESSION_L1 / _MSE
 * (labels f32 [B,C]) or _MULTI_LABEL (labels f32 [B,C], NaN = unlabelled; every label NaN: loss NaN, dlogits zeros) */
int gget_op_task_loss(const float* logits, const void* labels, const float* sample_wgt, int problem, int B, int C, float* loss_out,
                      float* dlogits, void* stream);
/* AUC surrogate (see gget_set_auc) on logits f32 [B,C >= 2], labels int64 [B]; lists int32 [2B] scratch receives the ordered positive
 * (at 0) and negative (at B) sample lists; B * num_neg <= 8192, else error 2; no positive or no negative: loss NaN, dlogits zeros */
int gget_op_auc_loss(const float* logits, const int64_t* labels, int B, int C, int num_neg, uint32_t seed, float* loss_out,
                     float* dlogits, int32_t* lists, void* stream);
/* MLP score head: out bf16 [B,d] = hidden[pool_row]; dhidden[pool_row[b]] = bf16(src[b]) (other rows untouched) */
int gget_op_pool_rows(const void* hidden, const int32_t* pool_row, void* out, int B, int d, void* stream);
int gget_op_scatter_rows_f32(const float* src, const int32_t* pool_row, void* dhidden, int B, int d, void* stream);
/* one Linear of the MLP head with the activation in front of it, dropout off: a bf16 [B,Din] = bf16(gelu(x)),
 * y bf16 [B,Dout] = bf16(a w^T + bias), y32 (optional) the same values as f32 */
int gget_op_head_linear_fwd(const void* x, void* a, const void* w, const void* bias, void* y, float* y32, int B, int Din, int Dout,
                            int layer, void* stream);
/* its backward: dx f32 [B,Din] = (dy w) gelu'(x), dw f32 [Dout,Din] += dy^T a, dbias f32 [Dout] += column sums of dy (NULL: none) */
int gget_op_head_linear_bwd(const float* dy, const void* x, const void* a, const void* w, float* dw, float* dbias, float* dx, int B,
                            int Din, int Dout, int layer, void* stream);

/* ------------------------------------------------------------------------------------------
 * The integer machinery of a pre-training step, one launcher at a time (csrc/kernels.h; no arithmetic in the wrappers): the padding-free
 * token layout, the SMTP head's compaction / slot sort / scatter, the indexed GEMM that feeds the sorted head, and the small
 * row-selection kernels.  tests/test_gpu_plan.py holds every output integer-exact or bit for bit (tests/_plan_ref.py states each
 * operation); INTEGRATION.md "The batch-layout and SMTP-head index kernels" lists the contract each entry is held to.
 * ------------------------------------------------------------------------------------------ */
/* key_len[b] (may be NULL) = non-zeros of mask int64 [B,S] (mask NULL: S); pool_row[b] (may be NULL, needs ids) = b S + (p - 1 + S) % S with
 * p = entries of ids[b, :, 0] (int64 [B,S,ldF]) that differ from pad_id - an all-pad row gives b S + S - 1 */
int gget_op_lengths(const int64_t* mask, const int64_t* ids, int ldF, int pad_id, int32_t* key_len, int32_t* pool_row, int B, int S,
                    void* stream);
/* *out = sum of key_len int32 [B] (one block, any B >= 1) */
int gget_op_sum_lengths(const int32_t* key_len, int B, int32_t* out, void* stream);
/* Var-len layout of a right-padded batch on tc token rows rounded up to t_rows.  cu int32 [B+1] = exclusive scan of key_len (cu[B] = the
 * total), every sample cut at tc (key_len is rewritten where it was cut); ids_c int64 [t_rows,F], pos_c int64 [t_rows] (pos NULL: the
 * token's s), row_b int32 [t_rows], c2p int32 [t_rows] (= b S + s) of compact row cu[b] + s; pad2c int32 [B S] = compact row or -1; tail
 * rows [tc, t_rows): pad_id, position 0, sample 0, c2p = B S + (r - tc).  pool_row (may be NULL; b S + p on entry) becomes
 * cu[b] + clamp(p, 0, len - 1).  long_list (may be NULL) int32 [3 B + 1]: [0] = number of samples of 33 .. 64 rows, then their indices,
 * first rows (at 1 + B) and row counts (at 1 + 2 B) in batch order.  status int32 [3]: [0] = 1 if sum(key_len) != tc else 0, [2] = 1
 * (sticky, never cleared here) in the same case, [1] untouched.  With tc > sum the rows [sum, tc) are not written. */
int gget_op_varlen_plan(const int64_t* ids, int ldF, int F, const int64_t* pos, int32_t* key_len, int32_t* pool_row, int32_t* cu,
                        int64_t* ids_c, int64_t* pos_c, int32_t* row_b, int32_t* pad2c, int32_t* c2p, int32_t* status, int B, int S, int tc,
                        int t_rows, int pad_id, int32_t* long_list, void* stream);
/* out bf16 [n_pos,d] = src[pad2c[i]], a zero row where pad2c[i] < 0; d % 8 == 0 */
int gget_op_rows_to_grid(const void* src, const int32_t* pad2c, void* out, int64_t n_pos, int d, void* stream);
/* SMTP head compaction over labels int64 [T,n] (NULL: every cell selected; -100 = unlabelled), in (token, slot) order: cnt[t] = labelled
 * cells of token t, m_off[t] / l_off[t] = selected tokens / labelled cells before t, counts = (M, Lm); row_idx[m] = token of selected row
 * m; per labelled cell l: sel_src[l] = m n + f, sel_label[l], sel_tok[l] = t.  Entries at or behind M / Lm are not written.  slot_hist
 * (may be NULL) int32 [n]: the cells of every slot are ADDED to it when n <= 32, it is left alone when n > 32.  ws: int32 scratch of
 * gget_op_head_compact_ws_bytes(T) bytes.  T >= 1. */
uint64_t gget_op_head_compact_ws_bytes(int T);
int gget_op_head_compact(const int64_t* labels, int T, int n, int32_t* cnt, int32_t* m_off, int32_t* l_off, int32_t* counts,
                         int32_t* row_idx, int32_t* sel_src, int32_t* sel_label, int32_t* sel_tok, int32_t* ws, int32_t* slot_hist,
                         void* stream);
/* Sorts the min(cap, *lm_count) labelled cells by slot f = sel_src % n, every slot padded to a multiple of tile_rows.  slot_state int32
 * [3 n + 2]: [0, n) the cells per slot on entry (gget_op_head_compact's slot_hist), [n, 2 n) cursors and [3 n + 1] a ticket, zero on entry;
 * on return [0, 2 n) and the ticket are zero again (self-clearing: the next call needs no memset) and [2 n, 3 n] hold the padded slot
 * starts.  Position p of slot f's range [start_f, start_f + cells_f): a_cell[p] = the cell's sel_src, a_tok[p] = row_idx[a_cell[p] / n],
 * c_l[p] = its l, cellpos[l] = p - the ORDER INSIDE A SLOT IS FREE (it comes from atomics).  Pad positions up to start_{f+1}: a_tok =
 * a_cell = 0, c_l = -1.  tile_off[t] = f * slot_elems for every tile_rows-row tile of slot f; *total_p = the padded total.  n <= 32,
 * cap >= 1; a_tok / a_cell / c_l hold cap + n * tile_rows entries. */
int gget_op_head_slot_sort(const int32_t* sel_src, const int32_t* row_idx, const int32_t* lm_count, int32_t* slot_state, int32_t* a_tok,
                           int32_t* a_cell, int32_t* c_l, int32_t* cellpos, int32_t* tile_off, int32_t* total_p, int cap, int n,
                           int64_t slot_elems, int tile_rows, void* stream);
/* dhid bf16 row r(t) = bf16_rne(fp32 sum over j = 0 .. cnt[t] - 1, in that order, of dxs[cellpos[l_off[t] + j]]) for every token t < TP
 * with cnt[t] > 0 (cnt <= 64); r(t) = t, or pad2c[t] (pad_row where that is negative) when pad2c is given; rows of tokens with cnt == 0
 * are not written.  d % 8 == 0. */
int gget_op_head_cell_sum(const void* dxs, const int32_t* cellpos, const int32_t* cnt, const int32_t* l_off, const int32_t* pad2c,
                          void* dhid, int TP, int d, int pad_row, void* stream);
/* rows i < min(cap, *count): gather dst[i] = src[idx[i]], or scatter (scatter != 0) dst[idx[i]] = src[i]; bf16 rows of d % 8 == 0
 * elements; other rows of dst are not written */
int gget_op_gather_rows(const void* src, const int32_t* idx, const int32_t* count, void* dst, int cap, int d, int scatter, void* stream);
/* rows i < min(cap, *count): r = pad2c[idx[i]] (pad_row and status[2] = 1 where that is negative; status may be NULL), dst[i] = src[r],
 * idx[i] = r (rewritten in place).  Without a negative entry status is not written. */
int gget_op_gather_rows_remap(const void* src, int32_t* idx, const int32_t* count, const int32_t* pad2c, void* dst, int cap, int d,
                              int pad_row, int32_t* status, void* stream);
/* w[b] = 1.0f / ((float)tot_b + 1e-7f), tot_b = entries of labels int64 [B,cells] that are not -100 */
int gget_op_sample_mask_wgt(const int64_t* labels, float* w, int B, int cells, void* stream);
/* raw-embedding inputs: out bf16 [T,e] row t = bf16_rne(raw f32 row lt), or tok bf16 [e] when every label (first_only: the first label) of
 * labels int64 row lt [n] is set (!= -100); flag[t] = 1 on the replaced rows, else 0.  lt = rows_map[t] (NULL: t); lt >= n_logical: a zero
 * row, flag 0.  labels NULL: no row is replaced. */
int gget_op_raw_blend(const float* raw, const int64_t* labels, int n, int first_only, const void* tok, void* out, int32_t* flag, int T,
                      int e, const int32_t* rows_map, int n_logical, void* stream);
/* dtok f32 [e] += sum over the rows t < T with flag[t] != 0 of dx bf16 [T,e] (fp32 atomics, one per 256-row block and column) */
int gget_op_raw_tok_grad(const void* dx, const int32_t* flag, float* dtok, int T, int e, void* stream);
/* The indexed GEMM of the slot-sorted head, C = op(A) op(B) in bf16 with the plain epilogue, mode GGET_GEMM_NT / GGET_GEMM_NN, rows
 * m < min(M_cap, *m_dev) (m_dev is required with a_rows / b_tile_off):
 *   a_rows      row m of the product reads row a_rows[m] of A (repeats allowed);
 *   b_tile_off  the B operand of row tile t starts b_tile_off[t] ELEMENTS behind B; the tile height is b_tile_rows = 256 when N % 256 == 0,
 *               else 128 (a b_tile_rows of 256 falls back to 128-row tiles, and b_tile_off is then indexed by 128-row tile);
 *   c_rows      row m is stored at row c_rows[m] of C; a NEGATIVE entry means the row is NOT STORED.
 * N % 192 == 0, K % 64 == 0.  With a_rows and b_tile_off both NULL this is the plain single-problem launch with the c_rows scatter
 * (any mode the plain epilogue supports; m_dev optional). */
int gget_op_gemm_indexed(int mode, const void* A, const void* B, void* C, int M_cap, int N, int K, int lda, int ldb, int ldc,
                         const int32_t* m_dev, const int32_t* a_rows, const int32_t* b_tile_off, int b_tile_rows, const int32_t* c_rows,
                         void* stream);

/* ---- test-only entries of the device-sized and split-K slab GEMM launches (the SMTP head, the shed weight gradients): the launcher with
 * every argument, no arithmetic of their own (tests/test_gpu_head_gemm.py against tests/_headgemm_ref.py) ---- */
/* One problem through gget_gemm_single, epilogue GGET_EPI_NONE (C bf16 [M][ldc]) or GGET_EPI_SLAB_F32 (C fp32 [split_k][M][ldc]).  M and K are
 * CAPACITIES: the host sizes the grid for them, the kernel reads the counts.
 *   m_dev   rows m >= min(M, *m_dev) are neither read nor stored (*m_dev == 0: C is untouched); NULL = M
 *   k_dev   the reduction runs over K rows [0, min(K, *k_dev)); NULL = K.  *k_dev == 0: the plain epilogue stores ZEROS (both kernels), the slab
 *           epilogue writes no slab (the caller clears what it sums).
 *   k_pad_zero (with k_dev) allows the persistent kernel when K % 64 == 0: it reads whole 64-row K-tiles up to round_up(*k_dev, 64), at least
 *           one, so rows [*k_dev, max(64, round_up(*k_dev, 64))) of A must be zero and those of B finite; without it (or K % 64 != 0) the
 *           non-persistent kernel zero-fills its K tail and reads nothing at or behind *k_dev
 *   split_k K slices of a slab launch: ktiles = ceil(K' / 64) over the K' actually reduced, per = ceil(ktiles / split_k), slice s owns K rows
 *           [64 s per, min(K', 64 (s + 1) per)) and writes slab s; slabs >= ceil(ktiles / per) are NOT written
 *   c_rows  (plain epilogue) row m is stored at row c_rows[m] of C, a negative entry means the row is not stored; NULL = row m */
int gget_op_gemm_dyn(int mode, int epilogue, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                     const int32_t* m_dev, const int32_t* k_dev, int k_pad_zero, int split_k, const int32_t* c_rows, void* stream);
/* up to 4 problems of one mode in ONE split-K launch with GGET_EPI_SLAB_F32 into slabs that share `slab_stride` (fp32 elements between the
 * slabs of consecutive K slices): problem i's slice s lands at C[i] + s slab_stride, [M[i]][ldc[i]].  How the engine issues the q|k|v and o
 * weight gradients it sheds from the grouped launch (C = wg and wg + 3 d^2, slab_stride = 4 d^2). */
int gget_op_gemm_grouped_slab(int mode, int count, const void* const* A, const void* const* B, void* const* C, const int* M, const int* N,
                              const int* K, const int* lda, const int* ldb, const int* ldc, int64_t slab_stride, int split_k, void* stream);
/* dst[i] = bf16_rne(slabs[i] + slabs[slab_stride + i] + ... ) for i < n, summed in slab order in fp32 (f32_out = 0: dst bf16, overwritten), or
 * dst[i] += that sum (f32_out = 1: dst fp32, an accumulator).  n % 4 == 0, slab_stride % 4 == 0; elements at or behind n are untouched. */
int gget_op_slab_reduce(const float* slabs, int64_t slab_stride, int nslab, void* dst, uint64_t n, int f32_out, void* stream);
/* the K slices the engine's backward asks for (csrc/engine.h: the same host functions), under the launch menu of the calling thread */
#define GGET_SLAB_PLAN_LM_HEAD 0   /* lm_head weight gradient [V, d] */
#define GGET_SLAB_PLAN_SHED_QKVO 1 /* q|k|v + o shed from the grouped weight-gradient launch (d % 192 == 0, CUs reserved), K = T */
#define GGET_SLAB_PLAN_SHED_O 2    /* o alone shed from it */
#define GGET_SLAB_PLAN_QKVO 3      /* q|k|v + o at d % 192 != 0 */
int gget_op_slab_plan(int which, int d, int V, int T, int* split);

/* ---- test-only entries of the step replay (tests/_step_replay.py replays gget_forward_task + gget_backward launch by launch): the
 * launchers as the engine's step calls them, no arithmetic of their own ---- */
/* The attention backward on the engine's operands: q | k in `qkv` are ALREADY rotated (the q|k|v projection's RoPE epilogue), dq / dk are
 * rotated back with cos_tab / sin_tab / position_ids ([B,S]-indexed).  row_base NULL = padded layout, else the var-len layout (needs
 * key_len; long_list as gget_op_attn_bwd_varlen_list).  dq_ws / dq_slab_stride as gget_op_attn_bwd_fused, or NULL / 0. */
int gget_op_attn_bwd_rotated(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* key_len,
                             const int32_t* row_base, void* dqkv, float* delta_ws, int B, int S, int H, int causal, const float* cos_tab,
                             const float* sin_tab, const int64_t* position_ids, float dropout_p, uint32_t dropout_seed, void* dq_ws,
                             uint64_t dq_slab_stride, const int32_t* long_list, void* stream);
/* The fp32 accumulators -> bf16 gradients: segment i = segs_dev[5 i ..] = {src, dst, count, copies, stride} (uint64 elements: offset of
 * replica 0 in `scratch`, offset in `grads`, elements - a multiple of 4 -, replicas to sum, elements between replicas);
 * grads[dst + j] = bf16_rne(sum over the replicas of scratch[src + c stride + j]) in fp32, replica order.  nseg = 0: nothing. */
int gget_op_convert_segments(const float* scratch, void* grads, const uint64_t* segs_dev, int nseg, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rank metrics of the multi-label evaluation pass (csrc/metrics.hip; the Python surface is graph-gpt_amd/metrics.py rank_metrics).
 * replaces: MultiLabelClassificationMetrics.compute (src/utils/metrics_utils.py:112-114: torcheval BinaryAUROC over num_labels tasks),
 * `_eval_rocauc` (src/utils/ogb_utils.py:13-29: scikit-learn roc_auc_score column by column on the host - ogbn-proteins :71-79, ogbg-molhiv
 * :173-184) and OGB's `_eval_ap` for ogbg-molpcba (:187-195: average_precision_score column by column).
 * scores f32 [n, C] (row stride ld_s elements), labels f32 [n, C] (row stride ld_y): 1 = positive, 0 = negative, NaN = unlabelled (the
 * entry is skipped, whatever its score).  Per column c, over its labelled entries, with a_i / e_i = negatives scored below / equal to the
 * positive i and g_i = positives scored >= it:
 *   n_pos[c], n_neg[c]  i64   positives and negatives
 *   auc2[c]             u64   sum_i (2 a_i + e_i):            ROC-AUC = auc2 / (2 n_pos n_neg), the Mann-Whitney statistic with mid-ranks
 *   ap_sum[c]           f64   sum_i g_i / (g_i + n_neg - a_i): AP = ap_sum / n_pos, scikit-learn's average_precision_score with its tie rule
 *   n_bad[c]            i32   labelled entries whose label is neither 0 nor 1 or whose score is not finite (left out of every count above;
 *                             the caller decides - the Python surface raises, as scikit-learn does on such input)
 * The counts are exact integers (compare-and-add, no sort); the fp64 sum runs over the positives in row order with a fixed tree: all five
 * outputs are bit-identical from run to run and independent of the launch geometry.  -0.0 == 0.0.  A column with n_pos == 0 or
 * n_neg == 0 gets auc2 = 0 and ap_sum = 0.  n == 0 or C == 0 is a valid call that launches nothing (the outputs are not written).
 * workspace: device memory of at least the bytes the _workspace query returns for (n, C), 16-byte aligned, contents irrelevant; a smaller
 * one is refused with an error before anything is launched.  Five launches on `stream`, no host sync.  C <= 65535.
 * ------------------------------------------------------------------------------------------ */
size_t gget_op_rank_metrics_workspace(int n, int C);
int gget_op_rank_metrics(const float* scores, int ld_s, const float* labels, int ld_y, int n, int C, int64_t* n_pos, int64_t* n_neg,
                         uint64_t* auc2, double* ap_sum, int32_t* n_bad, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Link-prediction metrics of the two-class evaluation pass (csrc/metrics.hip; the Python surface is graph-gpt_amd/metrics.py link_hits /
 * link_mrr), on the flat device tensors the metric object holds: scores f32 [n], labels i64 [n] (1 = positive edge, 0 = negative edge),
 * idx i64 [n].  An entry whose label is neither 0 nor 1 or whose score is not finite is "bad": counted, and left out of every other count.
 * Both entries: n < 2^31 (a negative n is refused); n == 0 is a valid call that launches nothing (the outputs are not written);
 * workspace = device memory of at least the bytes the _workspace(n) query returns (0 for n <= 0), 16-byte aligned, contents irrelevant -
 * a smaller one is refused with an error before anything is launched; every launch goes to `stream`, no host sync.  Integer counters
 * only (no floating-point atomic): every output is exact, independent of the launch geometry and bit-identical from run to run.
 *
 * gget_op_link_hits     replaces: `_reformat_pred_for_hr_eval` (src/utils/ogb_utils.py:141-152) + OGB `_eval_hits` (torch.topk of the negatives,
 *                       compare-and-sum) behind `_eval_ogbl_ppa` :82-90 and `_eval_ogbl_ddi` :131-138.
 *   n_pos, n_neg  i64   positives and negatives
 *   kth           f32   the K-th largest negative score (-0.0 reads as +0.0); -inf when n_neg < K
 *   hits          i64   positives with score > kth (a float comparison: -0.0 == +0.0); n_pos when n_neg < K.  Hits@K = hits / n_pos
 *   n_bad         i32   bad entries
 *   Exact selection without a sort: the negatives' fp32 bits become order-preserving 32-bit keys; four passes of a most-significant-digit
 *   radix select (8-bit digits; LDS histogram per workgroup, merged with integer atomics; a one-wave step picks the digit that holds the
 *   K-th entry), the classification fused into the first; a last pass counts the positives above kth.  K >= 1.
 *
 * gget_op_link_mrr      replaces: `_reformat_pred_for_mrr_eval` (src/utils/ogb_utils.py:155-170: sort by idx, mask, reshape [-1, cnt_neg]) + OGB
 *                       `_eval_mrr` behind `_eval_ogbl_citation2` :92-102 (groups = 1) and `_eval_ogbl_wikikg2` :105-128 (groups = 2: the even
 *                       negative columns are the head batch, the odd ones the tail batch, :112-113; cnt_neg must be even).
 *   idx must be a permutation of 0 .. n-1: entry i takes position idx[i].  In that order the positives are p[0, P) and the negatives the rows
 *   [r cnt_neg, (r + 1) cnt_neg), P = n / (1 + cnt_neg) (n % (1 + cnt_neg) != 0 is refused).
 *   n_pos, n_neg             i64
 *   optimistic, pessimistic  i32 [groups][P]   negatives of the (group, row) scored > / >= the row's positive
 *   hits_1_3_10              i64 [3]           entries with rank <= 1 / 3 / 10, rank = (optimistic + pessimistic) / 2 + 1
 *   mrr_sum                  f64               sum of 1 / rank over the groups * P entries in list order with a fixed tree
 *   n_bad                    i32 [2]           [0] indices outside [0, n) or repeated; [1] bad entries, or -1 when there are none but
 *                                              n_neg != n_pos * cnt_neg.  When either is non-zero the reference asserts; here optimistic /
 *                                              pessimistic are not written and hits_1_3_10 / mrr_sum are 0.
 *   Scatter by idx (a per-slot mark finds repeats), stable partition by count / scan / fill (no slot handed out by an atomic), one wave
 *   per row, one block for the sums.
 * ------------------------------------------------------------------------------------------ */
size_t gget_op_link_hits_workspace(int n);
int gget_op_link_hits(const float* scores, const int64_t* labels, int n, int64_t K, int64_t* n_pos, int64_t* n_neg, float* kth, int64_t* hits,
                      int32_t* n_bad, void* workspace, size_t workspace_bytes, void* stream);
size_t gget_op_link_mrr_workspace(int n);
int gget_op_link_mrr(const float* scores, const int64_t* labels, const int64_t* idx, int n, int cnt_neg, int groups, int64_t* n_pos,
                     int64_t* n_neg, int32_t* optimistic, int32_t* pessimistic, int64_t* hits_1_3_10, double* mrr_sum, int32_t* n_bad,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Graph-clustering metrics of the token-level heads (loss_type "token_ce" / "token_ce_intra"; csrc/metrics.hip; the Python surface is
 * graph-gpt_amd/metrics.py cluster_metrics / GraphClusteringMetrics).
 * replaces: GraphClusteringMetrics.update (src/utils/metrics_utils.py:231-295: torch.argmax, then per sample two .nonzero()) and
 * `get_acc_per_graph` (:340-348: per distinct label and per distinct prediction a .nonzero(), a .unique() and a len(...), each a
 * device-to-host synchronisation inside a Python loop).
 *   pred_or_logits  is_logits = 1: f32 [B][S][C], rows contiguous; prediction = arg-max over C with torch's rule (the first index of the
 *                   maximum; a NaN is maximal and the first NaN wins; -0.0 ties +0.0).  is_logits = 0: i64 [B][S], the predictions.
 *   labels          i64 [B][S], -100 = unlabelled
 *   raw_node_idx    i64 [B][S], -100 at every position that is not the one counted occurrence of a node (padding included)
 * A position is SELECTED when raw_node_idx != -100 and KEPT when it is selected and its label != -100.  A selected position is BAD when
 * its label is neither -100 nor in [0, C), or (is_logits = 0) its prediction is outside [0, C): it is counted in n_bad and left out of
 * every other count.
 *   y_pred  i64 [B][S]   the arg-max, or a copy of the given predictions, at every position, selected or not
 *   counts  i32 [B][4]   (t_r, n_r, t_p, n_p) over the sample's kept positions: n_r distinct labels, t_r those whose positions all carry
 *                        one and the same prediction; n_p distinct predictions, t_p those whose positions all carry one label.
 *                        recall = t_r / n_r, precision = t_p / n_p; a sample without a kept position gets four zeros
 *   totals  i64 [4]      (n_correct, n_kept, n_selected, n_bad): the call ADDS to these (integer atomics); the caller zeroes them once
 *                        per evaluation pass.  n_correct: kept positions with prediction == label; accuracy = n_correct / n_kept
 * One launch on `stream`, one workgroup per sample (grid-stride), no workspace, no host sync.  Per label value the min and max
 * prediction and per prediction value the min and max label are kept in four int32 LDS tables of C entries (LDS integer min / max
 * atomics): every output is an exact integer, independent of lane order and launch geometry and bit-identical from run to run.  The
 * tables bound C: C > GGET_CLUSTER_MAX_C is refused with an error naming the limit.  B * S and S * C below 2^31; B == 0 or S == 0 is a
 * valid call that launches nothing (the outputs are not written).
 * ------------------------------------------------------------------------------------------ */
#define GGET_CLUSTER_MAX_C 2048 /* 4 tables x 2048 x 4 bytes = 32 KiB of LDS */
int gget_op_cluster_metrics(const void* pred_or_logits, int is_logits, const int64_t* labels, const int64_t* raw_node_idx, int B, int S,
                            int C, int64_t* y_pred, int32_t* counts, int64_t* totals, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prediction passes (csrc/infer.hip; the Python surface is graph-gpt_amd/inference.py).
 *
 * gget_op_infer_append
 * replaces: the per-batch collection of ft_infer_hidden_states (src/utils/log_eval_dump_utils.py:63-67: idx.view((-1, 1)),
 * res.task_logits.half(), res.task_hidden_states.half() appended to Python lists) and the vstack at its end (:68-73).
 * One launch appends a batch to three device arenas at row `row0` (the host knows it: B is a shape):
 *   logits   f32 [B][C]            -> out_logits fp16 [capacity][C], rows row0 .. row0 + B - 1
 *   hidden   bf16 [B][d] or NULL   -> out_hidden fp16 [capacity][d] (NULL exactly when hidden is), same rows
 *   idx      i64 [B]               -> out_idx    i64  [capacity], copied as is
 * f32 -> fp16 rounds to nearest even, as tensor.half() does: overflow to +-inf, fp16 subnormals produced, NaN stays NaN; bf16 -> fp16
 * widens to f32 (exact) and rounds once.  Nothing outside the B rows is written.  C >= 1, B >= 1, d % 64 == 0 (d = 0 without hidden
 * states); hidden / out_hidden 16-byte aligned.  row0 + B > capacity, a null pointer, an empty or an unsupported shape: error 2, no
 * launch.
 *
 * gget_op_node_records
 * replaces: the record building of process_data (src/utils/misc_utils.py:436-468: torch.argmax, torch.where(raw_node_idx != -100)
 * [0].unique(), three gathers, two .cpu() copies and a np.tile per batch).
 *   logits        f32 [B][S][C] or NULL   prediction = arg-max over C with torch's rule (the first maximal class; a NaN is maximal)
 *   pred          i64 [B][S]    or NULL   the predictions themselves; exactly one of logits / pred is given
 *   raw_node_idx  i64 [B][S]              -100 at every position that is not a node's one counted occurrence
 *   idx           i64 [B]                 the samples' indices
 *   records       i64 [cap][3]            every flat position p with raw_node_idx[p] != -100 becomes (idx[p / S], raw_node_idx[p], pred[p]),
 *                                         in ascending p, appended at the device cursor state[0]
 *   state         i64 [2]                 [0] the cursor, advanced by the records written; [1] += the records that did not fit in cap
 *                                         (they are not written).  The caller zeroes both once per pass.
 * Two launches on `stream` (nodes per chunk of 1024 positions; then a chunk's first record sits at cursor + the nodes of the chunks
 * before it, with a ballot rank inside the chunk): no atomic decides a record's place, so two calls on the same input give identical
 * bytes.  Scratch (4 KiB per device and stream) is the library's own.  B, S >= 1, B * S <= GGET_NODE_RECORDS_MAX_POS, C >= 1 with logits;
 * anything else is error 2 without a launch.
 * ------------------------------------------------------------------------------------------ */
#define GGET_NODE_RECORDS_MAX_POS (1 << 20)
int gget_op_infer_append(const float* logits, const void* hidden, const int64_t* idx, void* out_logits, void* out_hidden, int64_t* out_idx,
                         int64_t row0, int64_t capacity, int B, int C, int d, void* stream);
int gget_op_node_records(const float* logits, const int64_t* pred, const int64_t* raw_node_idx, const int64_t* idx, int64_t* records,
                         int64_t* state, int64_t cap, int B, int S, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Contrastive pre-training head (GGET_KIND_PRETRAIN_CL; task_type = "pretrain-cl").  replaces: `cl_proj` and the discriminative branch of
 * GraphGPTPretrainBase (src/models/graphgpt/modeling_pretrain.py:96-115, :238-257), _get_cl_logits_loss (modeling_helpers.py:201-227) and
 * _dist_infonce / cos_sim / GatherLayer (src/utils/loss_utils.py:89-167).
 *   r_b = (entries of input_ids[b,:,0] that differ from pad_token_id) - 1, h_b = the final-norm output at row r_b (bf16)
 *   z_b = cl_proj(h_b), fp32 accumulation, kept in fp32: the contrastive logits (head2_logits)       e_b = z_b / max(|z_b|, 1e-12)
 *   samples 2m and 2m + 1 are the two views of one graph: p(i) = i ^ 1; E [N,d] = the embeddings of all ranks (N = B for one rank)
 *   scores[i][j] = 20 <E[i], E[p(j)]>, scores[i][p(i)] = the most negative float (the self-similarity is masked)
 *   loss = ratio / 2 (CE(scores, arange(N)) + CE(scores^T, arange(N))), ratio = 0.5 beside the generative head (ratio_dis)
 * Shapes: d % 64 == 0, d <= 1024, 2 <= N <= 2048, N even; anything else is error 2 ("unsupported") without a launch.
 * The N x N scores are never stored and never rounded to bf16; every sum has a fixed order (no atomics: two calls give the same bits).
 * ------------------------------------------------------------------------------------------ */
/* replaces: hidden_states[bz_idx, sequence_lengths], cl_proj and F.normalize (modeling_helpers.py:213-218).  hidden bf16 [rows,d],
 * pool_row int32 [B] (rows of `hidden`), w bf16 [d,d]; z, e f32 [B,d]; rnorm f32 [B] = 1 / max(|z_b|, 1e-12).  B = 0: nothing to do. */
int gget_op_cl_embed_fwd(const void* hidden, const int32_t* pool_row, const void* w, float* z, float* e, float* rnorm, int B, int d,
                         void* stream);
/* replaces: _dist_infonce after the gather (loss_utils.py:127-137; cos_sim :140-167).  E f32 [N,d], rows in the order of cos_sim's
 * `left_new`.  stat f32 [3][N]: max_{k != i} 20 <E_i, E_k>, its log-sum-exp over k != i, and the row's loss term lse_i - 20 <E_i, E_p(i)>;
 * loss[0] = ratio / N * sum of the terms (the transposed cross-entropy sums the same N terms: the term of column i is the term of row p(i)). */
int gget_op_cl_loss_fwd(const float* E, int N, int d, float ratio, float* stat, float* loss, void* stream);
/* replaces: autograd through the above for the caller's own B rows (GatherLayer.backward, loss_utils.py:99-104, keeps the local slice).
 * row_map int32 [B]: the position of local row b in E (NULL: b itself, N = B); stat of gget_op_cl_loss_fwd on the same E; rnorm, hidden,
 * pool_row, w of gget_op_cl_embed_fwd; scale = upstream gradient * ratio.
 *   dE_b = 20 scale / N sum_{k != i} (P[i][k] + P[k][i] - 2 [k == p(i)]) E_k, i = row_map[b], P[i][k] = exp(20 <E_i, E_k> - lse_i)
 *          (row i as the query of its own term and as a key of every other row's)
 *   dz f32 [B,d] = (dE_b - e_b <e_b, dE_b>) rnorm_b (overwritten);  dw f32 [d,d] += dz^T h;
 *   dhidden bf16 [rows,d]: row pool_row[b] += dz_b w (bf16 read, fp32 sum, one rounding; other rows untouched). */
int gget_op_cl_bwd(const float* E, const float* stat, const int32_t* row_map, const float* rnorm, const void* hidden, const int32_t* pool_row,
                   const void* w, float scale, float* dz, float* dw, void* dhidden, int N, int B, int d, void* stream);
/* Engine calls of a GGET_KIND_PRETRAIN_CL handle.  gget_forward_pretrain runs the generative head as for GGET_KIND_PRETRAIN and then the
 * contrastive forward on the batch's own rows (B even, B <= 2048; labels may be NULL: the contrastive loss needs none); a packed [B,S,S]
 * mask is refused (the reference's pretrain-cl masks on the host and never packs).
 * replaces: `head2_logits` / `head2_loss` of the model output (modeling_pretrain.py:250-262): z f32 [B,d] and e f32 [B,d] of the last
 * forward (pointers into the workspace), and the loss scalar copied to loss_dev f32[1] on `stream`. */
int gget_cl_logits(gget_handle_t h, const float** z_dev);
int gget_cl_embeddings(gget_handle_t h, const float** e_dev);
int gget_cl_loss(gget_handle_t h, float* loss_dev, void* stream);
/* replaces: the two GatherLayer.apply + torch.cat of _dist_infonce for world > 1 (loss_utils.py:119-124).  After a forward, hands the
 * gathered matrix E_dev f32 [N,d] (caller-owned, alive until the backward has run) and row_map_dev int32 [B] (the positions of this
 * rank's rows in it) to the handle: the loss and the row statistics are recomputed over the N rows at once, gget_cl_loss then returns
 * that loss and the backward differentiates it for the local rows.  Holds until the next forward. */
int gget_cl_set_gathered(gget_handle_t h, const float* E_dev, int N, const int32_t* row_map_dev, void* stream);
/* replaces: the upstream gradients of `head1_loss` and `head2_loss` (autograd; src/utils/training_utils.py:44,66 backpropagates their
 * sum): the scales the NEXT gget_backward_begin / gget_backward applies to the generative and the contrastive loss, consumed by it
 * (default 1, 1).  generative = 1 or 0 (0: the generative head's backward is skipped, its weight gradients are zero; required when the
 * forward had no labels); contrastive: any float, 0 skips the contrastive backward (cl_proj's gradient is then exactly zero). */
int gget_cl_set_backward_scales(gget_handle_t h, float generative, float contrastive);

#ifdef __cplusplus
}
#endif
#endif /* GGET_H_ */
