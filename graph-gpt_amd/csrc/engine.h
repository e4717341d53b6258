// The engine object behind a gget_handle_t and the plans it is built from (internal: not installed).  Shared by engine.hip (plan and
// workspace construction, forward, backward), optimizer.hip (the step and what it runs over) and comm.hip (the data-parallel exchange).
#pragma once
#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "common.h"
#include "gemm.h"
#include "kernels.h"

struct ParamRec {
  std::string name;
  int ndim;
  int64_t shape[2];
  uint64_t off;     // elements into flat arrays
  uint64_t count;   // elements (unpadded)
  int layer;        // -1 embeddings, 0..L-1, L = final norm + heads
  bool accum32;     // gradient accumulated in fp32 scratch (atomics), converted to bf16 afterwards
  uint64_t off32;   // element offset in the fp32 scratch
};

struct LayerOff {
  uint64_t ln1, wqkv, wo, lam1, ln2, wgu, wdown, lam2;
  uint64_t ln1_32, lam1_32, ln2_32, lam2_32;
};

struct Plan {
  std::vector<ParamRec> params;
  uint64_t n_params = 0;    // padded flat length
  uint64_t lm_pad_off = 0, lm_pad_count = 0;   // zero rows behind lm_head.weight (see make_plan)
  uint64_t n_scratch32 = 0; // fp32 accumulation elements
  std::vector<LayerOff> layers;
  uint64_t emb = 0, emb32 = 0, gate = 0, gate32 = 0, normf = 0, normf32 = 0;
  uint64_t raw_ln = 0, raw_ln32 = 0, raw_tok = 0, raw_tok32 = 0, raw_proj = 0;   // raw-embedding inputs (embed_dim > 0)
  uint64_t cl = 0, cl32 = 0;   // cl_proj.weight (contrastive kind) and its fp32 accumulator
  uint64_t ntp = 0, lm = 0, lm32 = 0, score = 0, score32 = 0, sbias = 0, sbias32 = 0;
  bool has_gate = false, has_ntp = false, has_ls = false;
  // MLP score head (config.head_mlp_layers > 0): n_lin = layers + 1 Linears of widths head_dim[0] = d, ..., head_dim[n_lin] = num_labels
  int n_lin = 0;
  int head_dim[6] = {0, 0, 0, 0, 0, 0};
  uint64_t head_w[5] = {0}, head_w32[5] = {0}, head_b[5] = {0}, head_b32[5] = {0};
  bool has_res = false;  // residual adds run as their own kernels (LayerScale and/or DropPath) instead of GEMM epilogues
};

// bump allocator over the workspace arena
struct Bump {
  uint64_t off = 0;
  uint64_t take(uint64_t bytes) {
    const uint64_t o = off;
    off += align_up(bytes, 256);
    return o;
  }
};

struct LayerWs {
  uint64_t rstd1, xn1, qkv, lse, attn, araw, xmid, rstd2, xn2, gu, h, mraw;
};

struct Ws {
  uint64_t key_len, pool_row, cos_tab, sin_tab, key_lo, key_hi;
  std::vector<uint64_t> xres;  // L+1 residual-stream snapshots
  std::vector<LayerWs> lw;
  uint64_t rstd_f, hidden;
  uint64_t dxa, dxb, dxc, dxn, dqkv, dattn, dgu, dh, delta, dq_acc, dscaled, dscaled2;
  uint64_t scratch32, loss_sum, loss_part, sqnorm, counts, segs, emb_sort, emb_cnt, emb_slab, wg32, lm_slab;
  uint64_t sq_chunks, sq_tiles;   // gradient-norm shortcut: chunk table of everything but the layers' weight matrices; per-tile sums of those
  // pre-train head
  uint64_t cnt, hc_tot, m_off, l_off, row_idx, sel_src, sel_label, sel_tok, Hm, Pp, Hl, logits, dlogits, dHl, dP, dHm;
  // slot-sorted n_token_proj (kernels.hip k_head_slot_sort): sorted cell lists (token row / dP row / cell index per sorted position), the
  // sorted position of every cell, weight offset per 128-row tile, slot counters, padded total
  uint64_t ss_tok, ss_cell, ss_l, ss_pos, ss_tile, ss_state, ss_total;
  // task head
  uint64_t tlogits, tdlogits, pooled_h, auc_lists;
  uint64_t cl_z = 0, cl_e = 0, cl_dz = 0, cl_rn = 0, cl_stat = 0, cl_loss = 0;   // contrastive head (make_ws)
  uint64_t raw_x, raw_xn, raw_rstd, raw_dxn, raw_dx, raw_flag;   // raw-embedding inputs: blended bf16 [T,e], normalised [T,e], 1/rms [T], their gradients, mask flags [T]
  uint64_t qkv32 = 0;                // head width 32: the q | k | v projection's fp32 accumulators [T][3 d], rotated and rounded once by rope32_f32_kernel
  uint64_t rr_cos, rr_sin, rr_ids;   // rope_range: per-token angle tables [T][head_dim / 2] fp32 (room for 32 columns) and the identity position list [T] int64
  uint64_t tok_stat;   // token-level head: loss sum, labelled rows, 1 / rows
  uint64_t intra_rs, intra_cls;   // intra-instance token head: first row of every sample (int32 [max_batch + 1]), cls_idx clamped (int64 [max_batch])
  uint64_t long_wgt;   // stack_method = "long": per-sample loss weights (fp32 [max_batch])
  // var-len token layout: first compact row of every sample [max_batch + 1], per compact row its sample index / position / ids, the
  // padded -> compact row map [max_tokens], a status word
  uint64_t vl_cu, vl_rowb, vl_pos, vl_ids, vl_pad2c, vl_c2p, vl_status;   // (vl_c2p: compact -> padded row map [max_tokens])
  uint64_t vl_long;   // [3 max_batch + 1] int32: count, indices, first rows and row counts of the batch's 33 .. 64-row samples (varlen_scan_kernel)
  uint64_t wo_pack = 0, wot_pack = 0;   // fragment-major copies of every layer's o weight / its transpose (S <= 32 per-sample kernels), [L][d][d] bf16
  uint64_t pos_safe;   // position ids clamped into the RoPE table (int64 [max_tokens]); the sticky "clamped" flag is vl_status[1]
  uint64_t sk_ws;      // stream-K GEMM launches: flags + one fp32 partial tile per block (gemm.h)
  uint64_t head_x[6] = {0}, head_a[5] = {0}, head_d[2] = {0};   // MLP head: layer inputs / activations (bf16), fp32 gradient ping-pong
  uint64_t total;
};

// gradient buckets in completion order: heads (layer L) first, then layers L-1..0, then the embeddings (layer -1)
inline int bucket_of(int layer, int L) { return layer == L ? 0 : layer < 0 ? L + 1 : L - layer; }

// plan construction (engine.hip)
int check_cfg(const gget_config_t* c);
Plan make_plan(const gget_config_t& c);
std::vector<std::pair<uint64_t, uint64_t>> bucket_ranges(const gget_config_t& cfg, const Plan& plan);
void fill_param_info(const ParamRec& p, gget_param_info_t* out);     // (gget_param_info and its handle-free twin gget_plan_param_info)

// ZeRO-2 shard plan of one bucket (include/gget.h gget_shard_plan): `world` equal body slices of slice = floor(cnt / (world C)) C elements,
// rank r owning [off + r slice, off + (r + 1) slice); the tail [off + world slice, off + cnt) (< world C elements) is all-reduced and updated
// by every rank
struct ShardBucket { uint64_t off, cnt, slice, tail_off, tail_cnt; };

// The work list of an optimizer step that does not run over the whole arena (a frozen prefix, a rank's shard), one device allocation: the
// AdamW / EMA work items, the chunks the norm sums and - the sharded form - the slot of each of those chunks in the gathered partial vector
// (chunk_slot) and of every chunk of the global grid (slot_of); with parameter groups (gget_set_param_scales) the items are cut at every
// boundary where a scale changes and `scales` holds {lr_scale, wd_scale} per item - else it is null
struct OptWork {
  unsigned char* tab = nullptr;
  const GgetSqChunk* items = nullptr;
  const GgetSqChunk* chunks = nullptr;
  const int32_t* chunk_slot = nullptr;
  const int32_t* slot_of = nullptr;
  const float* scales = nullptr;
  int nitems = 0, nchunks = 0, nglobal = 0;
  int reset() {
    unsigned char* t = tab;
    *this = OptWork();
    if (t) GGET_HIP_CHECK(hipFree(t));
    return 0;
  }
  int upload(const std::vector<GgetSqChunk>& it, const std::vector<GgetSqChunk>& ch, const std::vector<int32_t>& ch_slot = {},
             const std::vector<int32_t>& global_slot = {}, const std::vector<float>& item_scales = {}) {
    if (int e = reset()) return e;
    const size_t b_it = it.size() * sizeof(GgetSqChunk), b_ch = ch.size() * sizeof(GgetSqChunk);
    const size_t b_cs = ch_slot.size() * sizeof(int32_t), b_gs = global_slot.size() * sizeof(int32_t);
    const size_t b_sc = item_scales.size() * sizeof(float);     // (2 per item, or none)
    if (b_it + b_ch + b_cs + b_gs == 0) return 0;
    GGET_HIP_CHECK(hipMalloc(&tab, b_it + b_ch + b_cs + b_gs + b_sc));
    items = reinterpret_cast<const GgetSqChunk*>(tab);
    chunks = items + it.size();
    chunk_slot = reinterpret_cast<const int32_t*>(chunks + ch.size());
    slot_of = chunk_slot + ch_slot.size();
    auto put = [](const void* dst, const void* src, size_t bytes) {
      return bytes ? hipMemcpy(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    GGET_HIP_CHECK(put(items, it.data(), b_it));
    GGET_HIP_CHECK(put(chunks, ch.data(), b_ch));
    GGET_HIP_CHECK(put(chunk_slot, ch_slot.data(), b_cs));
    GGET_HIP_CHECK(put(slot_of, global_slot.data(), b_gs));
    if (b_sc) {
      scales = reinterpret_cast<const float*>(slot_of + global_slot.size());
      GGET_HIP_CHECK(put(scales, item_scales.data(), b_sc));
    }
    nitems = (int)it.size();
    nchunks = (int)ch.size();
    nglobal = (int)global_slot.size();
    return 0;
  }
};

// [offset, count) of the trainable share of the bucket [lo, hi) (gget_engine::bucket_train_range; frozen < 0 = the bucket itself)
inline std::pair<uint64_t, uint64_t> bucket_train_share(std::pair<uint64_t, uint64_t> bucket, int frozen,
                                                        const std::vector<std::pair<uint64_t, uint64_t>>& train_ranges) {
  const uint64_t lo = bucket.first, hi = bucket.second;
  if (frozen < 0) return {lo, hi - lo};
  for (const auto& r : train_ranges) {
    const uint64_t a = std::max(lo, r.first), b = std::min(hi, r.first + r.second);
    if (a < b) return {a, b - a};
  }
  return {lo, 0};
}

struct gget_engine {
  gget_config_t cfg;
  Plan plan;
  Ws ws;
  bf16_t* P;
  float* master;
  float* am;
  float* av;
  float* ema = nullptr;           // weight-EMA arena (gget_ema_attach; fp32 [n_params], the offsets of the other arenas), or none
  float ema_decay_next = -1.f;    // decay the NEXT gget_adamw_step[_sharded] applies (gget_set_ema_decay); < 0 = that step leaves the EMA alone
  bf16_t* G;
  // gradient accumulation (gget_grad_acc_attach): the fp32 sum of a window's micro-batch gradients, [n_params] with the offsets of the other
  // arenas, or none; grad_acc_count = micro-steps summed so far in the open window (0 = closed: the next gget_grad_accumulate overwrites)
  float* grad_acc = nullptr;
  int grad_acc_count = 0;
  // what the norm passes and AdamW read: the accumulator while a window is open, else the bf16 gradient array
  bool grad_from_acc() const { return grad_acc != nullptr && grad_acc_count > 0; }
  const void* grad_src() const { return grad_from_acc() ? (const void*)grad_acc : (const void*)G; }
  unsigned char* W;
  const float* cos_tab;
  const float* sin_tab;
  // bucket -> [first,last) params, segments
  std::vector<std::pair<uint64_t, uint64_t>> bucket_range;  // elements
  std::vector<std::pair<int, int>> bucket_segs;              // [first, count) into the device segment table
  // state of the last forward
  // T = rows of the token-major activation buffers: B * S (padded layout) or round_up(real tokens, 64) (var-len layout, see
  // backbone_forward); TP = B * S always (the index space of ids / labels / the SMTP head's selections)
  int B = 0, S = 0, T = 0, TP = 0;
  bool varlen = false;            // the last forward ran on the compacted (padding-free) token layout
  bool wo_packed = false;         // the last forward built the fragment-major o weights (S <= 32 per-sample kernels)
  int tc = 0;                     // its number of real tokens
  long tc_next = -1;              // real-token count of the NEXT forward's batch (gget_set_token_count); -1 = unknown -> padded layout,
                                  // GGET_TOKENS_AUTO = count on the device and read back; consumed (reset) at the ENTRY of every forward
  // gget_set_option(GGET_OPT_NORM_FROM_BACKWARD): the squared gradient norm of the layers' weight matrices comes from partial sums
  // their weight-gradient launches left behind (sq_layers = layers of the last backward that did), the rest from a chunked pass
  bool opt_norm_from_backward = false;
  bool opt_skip_nonfinite = false;     // GGET_OPT_SKIP_NONFINITE_STEP: gget_adamw_step leaves the parameters alone when the gradient norm is inf / NaN
  bool step_needs_norm(float max_grad_norm, const float* gnorm_dev) const { return max_grad_norm > 0.f || gnorm_dev != nullptr || opt_skip_nonfinite; }
  int sq_layers = 0;
  int n_sq_chunks = 0;
  bool emb_cnt_cleared = false;   // this backward's first launch cleared the embedding gradient's count matrix (gget_backward_begin)
  bool head_sorted_fwd = false;   // the last pre-train forward ran the slot-sorted n_token_proj (its lists feed the backward)
  bool tc_from_caller = false;    // the last var-len forward ran on a caller's count (a wrong one poisons the loss, see poison_loss)
  int32_t* host_word = nullptr;   // pinned host word the counted total lands in
  int32_t* host_word_dev = nullptr;   // ... and its device-side address (sum_lengths_kernel stores to it)
  const int64_t* pos_rows = nullptr;   // position of every ROW (GEMM RoPE epilogue): pos_cur, or the compacted positions
  const int32_t* row_base() const { return varlen ? wsp<int32_t>(ws.vl_cu) : nullptr; }
  const int32_t* long_list() const { return varlen ? wsp<int32_t>(ws.vl_long) : nullptr; }
  const int64_t* ids = nullptr;
  const int64_t* pos = nullptr;
  const float* sample_wgt = nullptr;
  bool have_labels = false;
  int problem = 0;
  int auc_num_neg = 1;
  const int64_t* cls_idx_next = nullptr;   // cls_idx of the NEXT forward_task (gget_set_cls_idx; loss_type = "token_ce_intra")
  float focal_gamma = 0.f;        // focal loss on the SMTP head (config.focal_gamma)
  bool stack_long = false;        // config.stack_method == "long" (gget_set_stack_method)
  float rope_range = 0.f;         // config.rope_range (gget_set_rope_range)
  const float* raw_next = nullptr;  // inputs_raw_embeds of the NEXT forward (gget_set_raw_embeds)
  bool raw_first_label_only = false;   // smtp_inside: the mask-token rule looks at labels[:, :, 0] only (modeling_pretrain.py:136-137)
  bool ls2_done = false;          // the LayerScale / DropPath backward of the next layer_backward's down branch is already done (fused)
  bool raw_used = false;          // the last forward consumed raw embeddings (its backward owes their gradients)
  const float* cos_cur = nullptr; // angle tables / position list of the last forward (the per-token ones under rope_range)
  const float* sin_cur = nullptr;
  const int64_t* pos_cur = nullptr;
  // in-step kernel probe (gget_debug_probe): HIP events around the grouped weight-gradient launch [0] and the gate|up + GEGLU launch [1]
  // of every layer, on the stream they are launched on - the bench reads the launch durations INSIDE a step from them
  bool probe = false;
  std::vector<hipEvent_t> probe_ev[2];
  hipEvent_t probe_event(int which, int idx) {
    auto& v = probe_ev[which];
    while ((int)v.size() <= idx) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; v.push_back(e); }
    return v[idx];
  }
  // GGET_TOKENS_AUTO: work of the forward that does not depend on the token count (the SMTP head's row / cell compaction, the packed copies
  // of the o weights) is enqueued BEHIND the 4-byte read-back and BEFORE the host waits for it, so that the device has ~35 us of kernels to
  // run while the host wakes up and enqueues the layer stack (the step trace showed the device idle for 25-37 us there)
  std::function<int(hipStream_t)> presync_work;
  bool presync_done = false;
  hipEvent_t count_event = nullptr;
  unsigned auc_seed = 0;
  bool fwd_valid = false;
  // contrastive head (GGET_KIND_PRETRAIN_CL): the embedding matrix the loss of the last forward was taken over - the batch's own rows in
  // the workspace, or the caller's gathered matrix with the positions of the local rows (gget_cl_set_gathered) - and the upstream scales of
  // the NEXT backward (gget_cl_set_backward_scales; consumed by gget_backward_begin)
  const float* cl_E = nullptr;
  const int32_t* cl_map = nullptr;
  int cl_N = 0;
  bool cl_valid = false;
  float cl_gen_scale = 1.f, cl_scale = 1.f;
  float attn_drop_p = 0.f;       // attention dropout of the NEXT forward (training mode); 0 = off
  float path_drop_p = 0.f;        // stochastic-depth rate of the last layer (layer l: p*l/(L-1))
  unsigned attn_drop_seed = 0;
  float embed_drop_p = 0.f;       // embed_dropout / mlp dropouts of the NEXT forward (training mode); 0 = off
  float mlp_drop_p = 0.f;
  float head_drop_p = 0.f;        // dropout inside the MLP score head
  ElemDropArg head_drop() const { return elem_drop(head_drop_p, attn_drop_seed ^ 0x2545F491u); }
  // token-wise masks are keyed by the logical [B,S] row: on the var-len layout through the compact -> padded row map (vl_c2p)
  const int32_t* drop_rows() const { return varlen ? wsp<int32_t>(ws.vl_c2p) : nullptr; }
  ElemDropArg embed_drop() const { return elem_drop(embed_drop_p, attn_drop_seed ^ 0x5BD1E995u, drop_rows()); }
  ElemDropArg mlp_drop(int layer) const { return elem_drop(mlp_drop_p, attn_drop_seed + 0x7F4A7C15u * (unsigned)(layer + 1), drop_rows()); }
  PathDropArg path_drop(int layer, int which) const {
    const int L = cfg.num_layers;
    const float rate = (path_drop_p > 0.f && L > 1) ? path_drop_p * (float)layer / (float)(L - 1) : 0.f;
    return PathDropArg{rate, attn_drop_seed ^ (0xD6E8FEB8u * (unsigned)(layer * 2 + which + 1)), S, varlen ? wsp<int32_t>(ws.vl_rowb) : nullptr};
  }
  bf16_t* dx_cur = nullptr;  // gradient w.r.t. the residual stream entering the next backward stage
  bool packed = false;       // last forward used a 3-D block-diagonal attention mask (per-token key ranges)
  bool defer_convert = false;
  // data-parallel exchange (gget_comm_*): RCCL communicator of this rank and an fp32 staging buffer for the largest bucket
  void* comm = nullptr;
  bool comm_loopback = false;     // gget_comm_init_loopback: no peers, an all-reduce multiplies by comm_world
  int comm_rank = 0, comm_world = 1;
  // the data-parallel share of the launch menu (gget_set_dp_menu; CallScope applies it to this handle's calls)
  int dp_reserve_cus = 0;
  bool dp_lds_headroom = false;
  float* comm_f32 = nullptr;
  uint64_t comm_f32_elems = 0;
  // sharded optimizer step (ZeRO stage 2, gget_shard_init): the plan per bucket and the work list of this rank's share
  int shard_world = 0, shard_rank = 0;   // shard_world 0 = off (the replicated step)
  int shard_slots = 0;                   // partial-vector slots per rank
  std::vector<ShardBucket> shard_plan;
  OptWork shard_work;
  // frozen prefix (gget_set_frozen; reference freeze_llama_layers): -1 = everything trains and nothing below is used.  >= 0: embed_tokens
  // and the layers [0, frozen) are not trained - the trainable element ranges of the flat arenas (at most two) and their work list
  int frozen = -1;
  std::vector<std::pair<uint64_t, uint64_t>> train_ranges;   // [offset, count)
  OptWork frozen_work;
  // parameter groups (gget_set_param_scales): per-parameter scales of lr and weight decay, indexed like plan.params; empty = off (every
  // launch is then what it was without them).  group_work: the whole arena cut at the scale boundaries, what the replicated step of an
  // unfrozen model runs over instead of the grid-stride kernel (items and scales only: the norm paths do not change)
  std::vector<float> lr_scale, wd_scale;
  bool grouped() const { return !lr_scale.empty(); }
  OptWork group_work;
  // what a step, or an EMA lerp, runs over: the shard's work list (`sharded`: a plan is active and the caller runs its form), else the
  // trainable ranges', else none - the whole arena
  const OptWork* opt_work(bool sharded) const { return sharded ? &shard_work : frozen >= 0 ? &frozen_work : nullptr; }
  // nothing trainable sits upstream of layer 0: the backward stops at the lowest trainable unit (else the full chain runs - the gate /
  // raw-embedding gradients need the dgrad through the frozen layers)
  bool truncated() const { return frozen >= 0 && !plan.has_gate && cfg.embed_dim == 0; }
  int first_trainable_layer() const { return frozen < 0 ? 0 : std::min(frozen, cfg.num_layers); }
  // [offset, count) of a bucket's trainable share: the bucket itself, nothing (count 0), or - the embedding bucket - its gate /
  // raw-embedding parameters.  A bucket meets at most one of the ranges, in one piece.
  std::pair<uint64_t, uint64_t> bucket_train_range(int bucket) const { return bucket_train_share(bucket_range[bucket], frozen, train_ranges); }
  const int32_t* klo() const { return packed ? wsp<int32_t>(ws.key_lo) : nullptr; }
  const int32_t* khi() const { return packed ? wsp<int32_t>(ws.key_hi) : nullptr; }

  template <typename Tp>
  Tp* wsp(uint64_t off) const { return reinterpret_cast<Tp*>(W + off); }
  int bucket_of_layer(int layer) const { return bucket_of(layer, cfg.num_layers); }
};

// Every forward / backward call of a handle runs inside one CallScope.  It installs (a) the handle's stream-K workspace slice (zeroed at
// creation), through which the engine's GEMM launches may run stream-K, and (b) the menu the call plans with: the process menu overlaid
// by the handle's data-parallel fields (gget_set_dp_menu).  Op-level calls of the same thread afterwards see neither.
struct CallScope {
  LaunchMenu m;
  explicit CallScope(gget_engine* h) : m(g_menu) {
    if (h->dp_reserve_cus > 0) {   // CUs of their own for the collective: the 3-slot rings, the RMSNorm backward in its many-small-blocks form
      m.gemm_cu_reserve = h->dp_reserve_cus;
      m.gemm_lds_headroom = 1;
      m.rms_wide = 0;
    } else if (h->dp_lds_headroom) {
      m.gemm_lds_headroom = 2;
    }
    t_call_menu = &m;
    gget_gemm_streamk_workspace(h->W + h->ws.sk_ws);
  }
  ~CallScope() {
    gget_gemm_streamk_workspace(nullptr);
    t_call_menu = nullptr;
  }
};

// the gradient-norm shortcut's share of the plan (optimizer.hip): tile slots a layer's grouped weight-gradient launch may fill, the tiles
// it has, and the chunk table of everything else (uploaded at creation)
extern const int kSqTilesPerLayer;
long wg_tiles(int d, int ff);
int upload_sq_chunks(gget_engine* h);

// K slices of the backward's split-K slab launches (engine.hip), each fitted to one round of gget_gemm_num_cu() CUs under the menu of the
// calling thread: the lm_head weight gradient; q|k|v|o (with_qkv) or o alone when they are shed from the grouped weight-gradient launch;
// q|k|v + o at a width with d % 192 != 0.  The test-only gget_op_slab_plan (ops.hip) returns exactly these.
int lm_wgrad_split(int V, int d);
int shed_wgrad_split(bool with_qkv, int d, int T);
int qkvo_wgrad_split(int T);
