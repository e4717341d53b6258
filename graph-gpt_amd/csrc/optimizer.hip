// libgget_hip.so - optimizer: arenas, gradient accumulation, frozen prefix, weight EMA, the step, the sharded step (ZeRO stage 2;
// reference: DeepSpeed zero_optimization.stage 2, examples/ds_config2_pt.json:29-32, engine built at src/training/pretrain_mode.py:281-287)
// and the plan helpers only the step uses.  The kernels are in kernels.hip.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "engine.h"

// ================================================================================================
// the gradient-norm shortcut (GGET_OPT_NORM_FROM_BACKWARD): what the backward's weight-gradient launches leave behind, and the rest
// ================================================================================================
constexpr int kSqTilesPerLayer = 256;   // tiles of a layer's grouped weight-gradient launch that may leave norm partials (one per CU)

// tiles of a layer's grouped weight-gradient launch (192 x 192 over gate|up, down, q|k|v and o; engine.hip layer_backward)
long wg_tiles(int d, int ff) { return ((long)2 * ff * d + (long)d * ff + (long)4 * d * d) / (192 * 192); }

// chunk table of every gradient that is NOT one of the layers' seven projection matrices (those carry per-tile partial sums), uploaded
// into the workspace at creation
int upload_sq_chunks(gget_engine* h) {
  const int L = h->cfg.num_layers;
  uint64_t other = 0;
  auto is_layer_matrix = [&](const ParamRec& p) { return p.layer >= 0 && p.layer < L && !p.accum32 && p.ndim == 2; };
  for (const ParamRec& p : h->plan.params)
    if (!is_layer_matrix(p)) other += align_up(p.count, 128);
  const uint64_t chunk = std::max<uint64_t>(32768, align_up((other + 899) / 900, 128));
  std::vector<GgetSqChunk> chunks;
  for (const ParamRec& p : h->plan.params) {
    if (is_layer_matrix(p)) continue;
    const uint64_t n = align_up(p.count, 128);
    for (uint64_t o = 0; o < n; o += chunk) chunks.push_back(GgetSqChunk{p.off + o, std::min(chunk, n - o)});
  }
  if (h->plan.lm_pad_count) chunks.push_back(GgetSqChunk{h->plan.lm_pad_off, align_up(h->plan.lm_pad_count, 128)});   // (zeros; kept for symmetry with the full pass)
  if (chunks.size() <= 1024) {
    h->n_sq_chunks = (int)chunks.size();
    if (!chunks.empty() &&
        hipMemcpy(h->W + h->ws.sq_chunks, chunks.data(), chunks.size() * sizeof(GgetSqChunk), hipMemcpyHostToDevice) != hipSuccess) {
      gget_set_error("norm chunk table upload failed");
      return 1;
    }
  } else {
    h->n_sq_chunks = -1;   // (never with the chunk size above; the full pass is used then)
  }
  return 0;
}

// ================================================================================================
// work lists
// ================================================================================================
static ShardBucket shard_bucket(uint64_t off, uint64_t cnt, int world) {
  const uint64_t C = GGET_SHARD_CHUNK, slice = cnt / ((uint64_t)world * C) * C;
  return ShardBucket{off, cnt, slice, off + (uint64_t)world * slice, cnt - (uint64_t)world * slice};
}

// Parameter groups (gget_set_param_scales): the arena [0, n_params) as runs of equal {lr_scale, wd_scale}.  A parameter's run reaches to
// the next parameter's offset - the alignment gap behind it and, behind lm_head.weight, the pad rows ride with it (zeros: any scale keeps
// them zero) - and neighbours with the same two scales are one run, so a run boundary is a parameter offset (a multiple of 128) where a
// scale differs.  lr / wd: indexed like plan.params, nullptr = all ones.
struct ScaleRun { uint64_t off, end; float lr, wd; };
static std::vector<ScaleRun> scale_runs(const Plan& pl, const float* lr, const float* wd) {
  std::vector<int> order(pl.params.size());
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return pl.params[a].off < pl.params[b].off; });
  std::vector<ScaleRun> runs;
  for (int i : order) {
    const float l = lr ? lr[i] : 1.f, w = wd ? wd[i] : 1.f;
    if (runs.empty()) {
      runs.push_back(ScaleRun{0, pl.n_params, l, w});
    } else if (l != runs.back().lr || w != runs.back().wd) {
      runs.back().end = pl.params[i].off;
      runs.push_back(ScaleRun{pl.params[i].off, pl.n_params, l, w});
    }
  }
  return runs;
}

// [offset, count) ranges cut into the work items of the item kernels (k_adamw_items, k_ema_lerp_items: one block per item); with `runs`
// no item crosses a run boundary and `scales` holds the two scales of every item
struct WorkItems {
  std::vector<GgetSqChunk> items;
  std::vector<float> scales;
};
static WorkItems cut_items(const std::vector<std::pair<uint64_t, uint64_t>>& ranges, const std::vector<ScaleRun>* runs = nullptr) {
  WorkItems w;
  auto cut = [&](uint64_t lo, uint64_t hi, const ScaleRun* run) {
    for (uint64_t o = lo; o < hi; o += kAdamwItemElems) {
      w.items.push_back(GgetSqChunk{o, std::min<uint64_t>(kAdamwItemElems, hi - o)});
      if (run) w.scales.push_back(run->lr), w.scales.push_back(run->wd);
    }
  };
  for (const auto& r : ranges) {
    if (!runs) {
      cut(r.first, r.first + r.second, nullptr);
      continue;
    }
    for (const ScaleRun& run : *runs) {
      const uint64_t lo = std::max(r.first, run.off), hi = std::min(r.first + r.second, run.end);
      if (lo < hi) cut(lo, hi, &run);
    }
  }
  return w;
}

// the element ranges a sharded step updates: the body slice of rank `rank` of every bucket (every rank's when `all_ranks`: the loopback
// communicator) and every tail
static std::vector<std::pair<uint64_t, uint64_t>> shard_share(const std::vector<ShardBucket>& plan, int world, int rank, bool all_ranks) {
  std::vector<std::pair<uint64_t, uint64_t>> share;
  for (const ShardBucket& b : plan) {
    for (int r = 0; r < world; ++r)
      if (all_ranks || r == rank) share.push_back({b.off + (uint64_t)r * b.slice, b.slice});
    share.push_back({b.tail_off, b.tail_cnt});
  }
  return share;
}

// ================================================================================================
// entry points
// ================================================================================================
extern "C" int gget_ema_attach(gget_handle_t h, float* ema_dev) {
  GGET_REQUIRE(h != nullptr, "ema_attach: null handle");
  h->ema = ema_dev;
  h->ema_decay_next = -1.f;
  if (ema_dev && h->plan.lm_pad_count)    // as gget_create: the pad rows read as zeros whatever the caller's arena held
    GGET_HIP_CHECK(hipMemset(ema_dev + h->plan.lm_pad_off, 0, h->plan.lm_pad_count * 4));
  return 0;
}

extern "C" int gget_grad_acc_attach(gget_handle_t h, float* acc_dev) {
  GGET_REQUIRE(h != nullptr, "grad_acc_attach: null handle");
  h->grad_acc = acc_dev;
  h->grad_acc_count = 0;      // (no window is open: the first gget_grad_accumulate overwrites whatever the arena holds)
  return 0;
}

extern "C" int gget_grad_accumulate(gget_handle_t h, void* stream) {
  GGET_REQUIRE(h != nullptr, "grad_accumulate: null handle");
  GGET_REQUIRE(h->grad_acc, "grad_accumulate: no accumulator arena (gget_grad_acc_attach)");
  if (h->frozen >= 0) {      // the trainable ranges only (every rank's: the exchange follows): the frozen share is never written and never read
    for (const auto& r : h->train_ranges)
      if (int e = k_grad_accumulate(h->G + r.first, h->grad_acc + r.first, r.second, h->grad_acc_count == 0, (hipStream_t)stream)) return e;
  } else if (int e = k_grad_accumulate(h->G, h->grad_acc, h->plan.n_params, h->grad_acc_count == 0, (hipStream_t)stream)) return e;
  ++h->grad_acc_count;
  return 0;
}

extern "C" int gget_grad_acc_count(gget_handle_t h, int32_t* out) {
  GGET_REQUIRE(h != nullptr && out != nullptr, "grad_acc_count: null argument");
  *out = h->grad_acc_count;
  return 0;
}

extern "C" int gget_grad_acc_set_count(gget_handle_t h, int32_t n) {
  GGET_REQUIRE(h != nullptr, "grad_acc_set_count: null handle");
  GGET_REQUIRE(n >= 0, "grad_acc_set_count: count %d < 0", (int)n);
  GGET_REQUIRE(n == 0 || h->grad_acc, "grad_acc_set_count: no accumulator arena (gget_grad_acc_attach)");
  h->grad_acc_count = n;
  return 0;
}

// the trainable element ranges for `frozen_layers` = k >= 0 with the parameter order of make_plan: [end of embed_tokens, start of layer 0)
// (gate / raw-embedding parameters; usually empty) and [start of layer min(k, L), n_params); empty ranges are dropped
static std::vector<std::pair<uint64_t, uint64_t>> frozen_train_ranges(const gget_config_t& c, const Plan& pl, int k) {
  const int L = c.num_layers;
  const uint64_t emb_end = pl.emb + align_up((uint64_t)c.vocab_size * c.hidden_size, 128);
  const uint64_t layer0 = L > 0 ? pl.layers[0].ln1 : pl.normf;
  const uint64_t from = k < L ? pl.layers[k].ln1 : pl.normf;
  std::vector<std::pair<uint64_t, uint64_t>> r;
  if (layer0 > emb_end) r.push_back({emb_end, layer0 - emb_end});
  if (pl.n_params > from) r.push_back({from, pl.n_params - from});
  return r;
}

// The work lists of the handle for its frozen prefix (h->frozen), its scale table and its shard plan, built again: what gget_set_frozen
// and gget_set_param_scales end in, in either call order (gget_shard_init cuts its own from the two others)
static int rebuild_work(gget_engine* h) {
  if (int e = h->frozen_work.reset()) return e;
  if (int e = h->group_work.reset()) return e;
  h->train_ranges.clear();
  std::vector<ScaleRun> runs;
  if (h->grouped()) runs = scale_runs(h->plan, h->lr_scale.data(), h->wd_scale.data());
  if (h->grouped() && h->frozen < 0) {      // the replicated step of an unfrozen model: the whole arena as items
    const WorkItems it = cut_items({{0, h->plan.n_params}}, &runs);
    if (int e = h->group_work.upload(it.items, {}, {}, {}, it.scales)) return e;
  }
  if (h->frozen >= 0) {
    h->train_ranges = frozen_train_ranges(h->cfg, h->plan, std::min(h->frozen, h->cfg.num_layers));
    uint64_t total = 0;
    for (const auto& r : h->train_ranges) total += r.second;
    // at most 1024 norm chunks (one block and one partial sum each)
    const uint64_t chunk = std::max<uint64_t>(32768, align_up((total + 999) / 1000, 128));
    std::vector<GgetSqChunk> chunks;
    for (const auto& r : h->train_ranges)
      for (uint64_t o = 0; o < r.second; o += chunk) chunks.push_back(GgetSqChunk{r.first + o, std::min(chunk, r.second - o)});
    GGET_REQUIRE(chunks.size() <= 1024, "set_frozen: %d norm chunks", (int)chunks.size());
    const WorkItems it = cut_items(h->train_ranges, h->grouped() ? &runs : nullptr);
    if (int e = h->frozen_work.upload(it.items, chunks, {}, {}, it.scales)) return e;
  }
  // a shard plan cuts the trainable share of every bucket: built again for the new ranges and scales
  if (h->shard_world > 0) return gget_shard_init(h, h->shard_world, h->shard_rank, nullptr);
  return 0;
}

extern "C" int gget_set_frozen(gget_handle_t h, int frozen_layers) {
  GGET_REQUIRE(h != nullptr, "set_frozen: null handle");
  GGET_REQUIRE(frozen_layers >= -1, "set_frozen: %d frozen layers (-1 = none, k >= 0 = embed_tokens and the first k layers)", frozen_layers);
  GGET_REQUIRE(h->grad_acc_count == 0, "set_frozen: a gradient-accumulation window is open (%d micro-steps summed); step first", h->grad_acc_count);
  h->frozen = frozen_layers;
  return rebuild_work(h);
}

// ================================================================================================
// parameter groups
// ================================================================================================
// finite and >= 0 (NaN fails the comparison); nullptr = all ones
static int check_scales(const char* who, const char* which, const float* s, int n, const Plan& pl) {
  for (int i = 0; s && i < n; ++i)
    GGET_REQUIRE(s[i] >= 0.f && std::isfinite(s[i]), "%s: %s[%d] = %g (%s) is not a finite value >= 0", who, which, i, (double)s[i],
                 pl.params[i].name.c_str());
  return 0;
}

extern "C" int gget_set_param_scales(gget_handle_t h, const float* lr_scale, const float* wd_scale, int n) {
  GGET_REQUIRE(h != nullptr, "set_param_scales: null handle");
  const int np = (int)h->plan.params.size();
  const bool off = !lr_scale && !wd_scale && n == 0;
  GGET_REQUIRE(off || n == np, "set_param_scales: %d scales for %d parameters (NULL, NULL, 0 switches the groups off)", n, np);
  if (int e = check_scales("set_param_scales", "lr_scale", lr_scale, n, h->plan)) return e;
  if (int e = check_scales("set_param_scales", "wd_scale", wd_scale, n, h->plan)) return e;
  h->lr_scale.assign(off ? 0 : np, 1.f);
  h->wd_scale.assign(off ? 0 : np, 1.f);
  for (int i = 0; i < n; ++i) {      // (+ 0.0f: a -0.0 is stored as 0.0)
    if (lr_scale) h->lr_scale[i] = lr_scale[i] + 0.f;
    if (wd_scale) h->wd_scale[i] = wd_scale[i] + 0.f;
  }
  return rebuild_work(h);
}

extern "C" int gget_param_scales(gget_handle_t h, float* lr_out, float* wd_out, int n) {
  GGET_REQUIRE(h != nullptr, "param_scales: null handle");
  const int np = (int)h->plan.params.size();
  GGET_REQUIRE(n == np, "param_scales: room for %d scales, the model has %d parameters", n, np);
  for (int i = 0; i < np; ++i) {
    if (lr_out) lr_out[i] = h->grouped() ? h->lr_scale[i] : 1.f;
    if (wd_out) wd_out[i] = h->grouped() ? h->wd_scale[i] : 1.f;
  }
  return 0;
}

extern "C" int gget_plan_param_count(const gget_config_t* cfg) {
  if (check_cfg(cfg)) return -1;
  return (int)make_plan(*cfg).params.size();
}

extern "C" int gget_plan_param_info(const gget_config_t* cfg, int index, gget_param_info_t* out) {
  if (int e = check_cfg(cfg)) return e;
  GGET_REQUIRE(out != nullptr, "plan_param_info: null argument");
  const Plan pl = make_plan(*cfg);
  GGET_REQUIRE(index >= 0 && index < (int)pl.params.size(), "param index %d out of range", index);
  fill_param_info(pl.params[index], out);
  return 0;
}

extern "C" int gget_group_plan(const gget_config_t* cfg, const float* lr_scale, const float* wd_scale, int n, int frozen_layers, int world,
                               int rank, gget_group_item_t* items_out, int cap, int32_t* n_out) {
  if (int e = check_cfg(cfg)) return e;
  const Plan pl = make_plan(*cfg);
  const int np = (int)pl.params.size();
  GGET_REQUIRE(n_out != nullptr && cap >= 0 && (items_out != nullptr || cap == 0), "group_plan: bad output arguments (cap %d)", cap);
  GGET_REQUIRE((!lr_scale && !wd_scale && n == 0) || n == np, "group_plan: %d scales for %d parameters", n, np);
  if (int e = check_scales("group_plan", "lr_scale", lr_scale, n, pl)) return e;
  if (int e = check_scales("group_plan", "wd_scale", wd_scale, n, pl)) return e;
  GGET_REQUIRE(frozen_layers >= -1, "group_plan: %d frozen layers", frozen_layers);
  GGET_REQUIRE(world >= 0 && (world == 0 || (rank >= -1 && rank < world)), "group_plan: bad arguments (rank %d world %d)", rank, world);
  std::vector<std::pair<uint64_t, uint64_t>> train, ranges;
  if (frozen_layers >= 0) train = frozen_train_ranges(*cfg, pl, std::min(frozen_layers, cfg->num_layers));
  if (world == 0) {
    ranges = frozen_layers >= 0 ? train : std::vector<std::pair<uint64_t, uint64_t>>{{0, pl.n_params}};
  } else {
    std::vector<ShardBucket> plan;
    for (const auto& b : bucket_ranges(*cfg, pl)) {
      const auto r = bucket_train_share(b, frozen_layers, train);
      plan.push_back(shard_bucket(r.first, r.second, world));
    }
    ranges = shard_share(plan, world, rank, rank < 0);
  }
  const std::vector<ScaleRun> runs = scale_runs(pl, lr_scale, wd_scale);
  const WorkItems w = cut_items(ranges, &runs);
  *n_out = (int32_t)w.items.size();
  for (size_t i = 0; i < w.items.size() && i < (size_t)cap; ++i)
    items_out[i] = gget_group_item_t{w.items[i].off, w.items[i].cnt, w.scales[2 * i], w.scales[2 * i + 1]};
  return 0;
}

extern "C" int gget_trainable_ranges(gget_handle_t h, uint64_t out[4], int32_t* n_out) {
  GGET_REQUIRE(h != nullptr && out != nullptr && n_out != nullptr, "trainable_ranges: null argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (h->frozen < 0) {
    out[1] = h->plan.n_params;
    *n_out = 1;
    return 0;
  }
  *n_out = (int32_t)h->train_ranges.size();
  for (size_t i = 0; i < h->train_ranges.size(); ++i) {
    out[2 * i] = h->train_ranges[i].first;
    out[2 * i + 1] = h->train_ranges[i].second;
  }
  return 0;
}

extern "C" int gget_bucket_train_range(gget_handle_t h, int bucket, uint64_t* offset, uint64_t* count) {
  GGET_REQUIRE(h != nullptr && offset != nullptr && count != nullptr, "bucket_train_range: null argument");
  GGET_REQUIRE(bucket >= 0 && bucket < (int)h->bucket_range.size(), "bucket_train_range: bucket %d out of range", bucket);
  const auto r = h->bucket_train_range(bucket);
  *offset = r.first;
  *count = r.second;
  return 0;
}

extern "C" int gget_set_ema_decay(gget_handle_t h, float decay) {
  GGET_REQUIRE(h != nullptr, "set_ema_decay: null handle");
  GGET_REQUIRE(decay <= 1.f, "set_ema_decay: decay %g > 1", (double)decay);     // (NaN fails the comparison too)
  GGET_REQUIRE(decay < 0.f || h->ema, "set_ema_decay: no EMA arena (gget_ema_attach)");
  h->ema_decay_next = decay < 0.f ? -1.f : decay;
  return 0;
}

extern "C" int gget_ema_update(gget_handle_t h, float decay, void* stream) {
  GGET_REQUIRE(h != nullptr, "ema_update: null handle");
  GGET_REQUIRE(h->ema && h->master, "ema_update: no EMA arena (gget_ema_attach) or no fp32 master arena");
  GGET_REQUIRE(decay >= 0.f && decay <= 1.f, "ema_update: decay %g outside [0, 1]", (double)decay);
  // frozen weights are constant: lerp(ema, w) == w there once the arena was seeded, so the average skips them - bit-identical to timm's lerp
  // over every entry.  decay == 0 IS the seed (ema = master): it also copies the frozen ranges (the complement of the trainable ones)
  if (h->frozen >= 0 && decay == 0.f) {
    uint64_t at = 0;
    for (size_t i = 0; i <= h->train_ranges.size(); ++i) {
      const uint64_t end = i < h->train_ranges.size() ? h->train_ranges[i].first : h->plan.n_params;
      if (end > at)
        if (int e = k_ema_lerp(h->master + at, h->ema + at, end - at, 0.f, (hipStream_t)stream)) return e;
      if (i < h->train_ranges.size()) at = h->train_ranges[i].first + h->train_ranges[i].second;
    }
  }
  // a shard plan: this rank's share (body slices + every tail; all of them for the loopback), as the sharded AdamW step
  if (const OptWork* w = h->opt_work(h->shard_world > 0)) return k_ema_lerp_items(h->master, h->ema, w->items, w->nitems, decay, (hipStream_t)stream);
  return k_ema_lerp(h->master, h->ema, h->plan.n_params, decay, (hipStream_t)stream);
}

extern "C" int gget_ema_to_params(gget_handle_t h, void* stream) {
  GGET_REQUIRE(h != nullptr, "ema_to_params: null handle");
  GGET_REQUIRE(h->ema, "ema_to_params: no EMA arena (gget_ema_attach)");
  h->wo_packed = false;      // a parameter write, as gget_sync_params: the per-sample kernels must not keep evaluating the live weights' packed copies
  return k_f32_to_bf16(h->ema, h->P, h->plan.n_params, (hipStream_t)stream);
}

// norm + clip + AdamW (+ EMA) of one step, the body of both entry points.  sharded: over the plan's work list, the norm from the gathered
// partial vector slots_dev; else over the trainable ranges of a frozen model, or the whole arena
static int optimizer_step(gget_engine* h, bool sharded, float lr, float beta1, float beta2, float eps, float weight_decay, float max_grad_norm,
                          float grad_scale, int step, const float* slots_dev, float* gnorm_dev, hipStream_t st) {
  GgetAdamwArgs a{};
  a.master = h->master, a.m = h->am, a.v = h->av, a.param = h->P;
  a.lr = lr, a.beta1 = beta1, a.beta2 = beta2, a.eps = eps, a.wd = weight_decay, a.step = step;
  a.max_norm = max_grad_norm, a.grad_scale = grad_scale, a.gnorm_out = gnorm_dev, a.skip_nonfinite = h->opt_skip_nonfinite;
  a.ema_decay = h->ema_decay_next;      // (gget_set_ema_decay: consumed by this call)
  h->ema_decay_next = -1.f;
  a.ema = a.ema_decay >= 0.f ? h->ema : nullptr;
  h->wo_packed = false;      // (see gget_sync_params; the next forward rebuilds the copies - the sharded step's from the gathered weights)
  float* sq = h->wsp<float>(h->ws.sqnorm);
  const bool need_norm = h->step_needs_norm(max_grad_norm, gnorm_dev);
  a.sqnorm = need_norm ? sq : nullptr;
  // an open accumulation window (gget_grad_accumulate): norm, clip, skip rule and update read the fp32 sum, and this call closes the window
  // whether or not the skip rule drops the update (GradScaler drops the whole update, not one micro-batch of it)
  a.grad_f32 = h->grad_from_acc();
  a.grad = h->grad_src();
  h->grad_acc_count = 0;
  const OptWork* w = h->opt_work(sharded);
  // parameter groups: the replicated step of an unfrozen model runs over the whole arena as items (the norm paths below do not change)
  const OptWork* iw = w ? w : h->grouped() ? &h->group_work : nullptr;
  if (need_norm) {
    if (sharded) {
      if (int e = k_grad_sqnorm_slots(slots_dev, w->slot_of, w->nglobal, sq, st)) return e;
    } else if (w) {
      // frozen prefix: a plain chunk pass over the trainable ranges (GGET_OPT_NORM_FROM_BACKWARD falls back to it)
      if (int e = k_grad_sqnorm_chunks(a.grad, w->chunks, w->nchunks, nullptr, 0, sq, st, a.grad_f32)) return e;
    } else if (h->opt_norm_from_backward && !a.grad_f32 && grad_scale == 1.0f && h->sq_layers == h->cfg.num_layers && h->n_sq_chunks >= 0) {
      // the shortcut holds only while the gradient array is exactly what the last backward wrote: the caller promised that
      // (GGET_OPT_NORM_FROM_BACKWARD), grad_scale != 1 means an exchange happened anyway, and every layer must have left its partials;
      // the partials of the last backward say nothing about a sum of several (grad_f32: the full pass over the accumulator)
      if (int e = k_grad_sqnorm_chunks(h->G, h->wsp<GgetSqChunk>(h->ws.sq_chunks), h->n_sq_chunks, h->wsp<float>(h->ws.sq_tiles),
                                       h->cfg.num_layers * kSqTilesPerLayer, sq, st))
        return e;
    } else if (int e = k_grad_sqnorm(a.grad, h->plan.n_params, sq, st, a.grad_f32)) return e;
  }
  // the item kernels share the per-element update with the grid-stride one: the same bits per element, given the same coefficient
  if (!iw) return k_adamw(a, h->plan.n_params, st);
  return iw->scales ? k_adamw_group_items(a, iw->items, iw->scales, iw->nitems, st) : k_adamw_items(a, iw->items, iw->nitems, st);
}

extern "C" int gget_adamw_step(gget_handle_t h, float lr, float beta1, float beta2, float eps, float weight_decay,
                               float max_grad_norm, float grad_scale, int step, float* gnorm_dev, void* stream) {
  GGET_REQUIRE(h && h->master && h->am && h->av, "adamw needs master/m/v arenas");
  GGET_REQUIRE(step >= 1, "step is 1-based");
  return optimizer_step(h, false, lr, beta1, beta2, eps, weight_decay, max_grad_norm, grad_scale, step, nullptr, gnorm_dev, (hipStream_t)stream);
}

extern "C" int gget_shard_plan(const gget_config_t* cfg, int world, int bucket, uint64_t out[5]) {
  if (int e = check_cfg(cfg)) return e;
  GGET_REQUIRE(out && world >= 1, "shard_plan: bad arguments (world %d)", world);
  GGET_REQUIRE(bucket >= 0 && bucket < cfg->num_layers + 2, "shard_plan: bucket %d out of range", bucket);
  const auto r = bucket_ranges(*cfg, make_plan(*cfg))[bucket];
  const ShardBucket sb = shard_bucket(r.first, r.second - r.first, world);
  out[0] = sb.off, out[1] = sb.cnt, out[2] = sb.slice, out[3] = sb.tail_off, out[4] = sb.tail_cnt;
  return 0;
}

extern "C" int gget_shard_init(gget_handle_t h, int world, int rank, int32_t* slots_per_rank) {
  GGET_REQUIRE(h && world >= 0 && (world == 0 || (rank >= 0 && rank < world)), "shard_init: bad arguments (rank %d world %d)", rank, world);
  GGET_REQUIRE(world == 0 || !(h->comm || h->comm_loopback) || (world == h->comm_world && rank == h->comm_rank),
               "shard_init: rank %d of %d does not match the communicator (rank %d of %d)", rank, world, h->comm_rank, h->comm_world);
  if (int e = h->shard_work.reset()) return e;
  h->shard_world = h->shard_rank = h->shard_slots = 0;
  h->shard_plan.clear();
  if (slots_per_rank) *slots_per_rank = 0;
  if (world == 0) return 0;
  // the loopback communicator stands for `world` ranks that hold this rank's gradients: the handle then does the work of all of them
  const bool all_ranks = h->comm_loopback;
  const uint64_t C = GGET_SHARD_CHUNK;
  std::vector<ShardBucket> plan;
  // (a frozen prefix, gget_set_frozen: a bucket's sharded range is its trainable share; an empty one - count 0 - is skipped everywhere)
  for (int b = 0; b < (int)h->bucket_range.size(); ++b) {
    const auto r = h->bucket_train_range(b);
    plan.push_back(shard_bucket(r.first, r.second, world));
  }
  // the norm's chunk grid: off_b + j C inside every bucket (independent of world: slices are multiples of C); owner = the rank of the body
  // slice, rank 0 for the tail
  std::vector<GgetSqChunk> grid;
  std::vector<int> owner;
  for (const ShardBucket& b : plan)
    for (uint64_t j = 0; j * C < b.cnt; ++j) {
      grid.push_back(GgetSqChunk{b.off + j * C, std::min(C, b.cnt - j * C)});
      owner.push_back(j * C < (uint64_t)world * b.slice ? (int)(j * C / b.slice) : 0);
    }
  std::vector<int> count(world, 0);
  std::vector<int32_t> local(grid.size());
  for (size_t j = 0; j < grid.size(); ++j) local[j] = count[owner[j]]++;
  const int S = *std::max_element(count.begin(), count.end());
  std::vector<int32_t> slot_of(grid.size()), chunk_slot;
  std::vector<GgetSqChunk> chunks;
  for (size_t j = 0; j < grid.size(); ++j) {
    slot_of[j] = owner[j] * S + local[j];
    if (all_ranks || owner[j] == rank) {
      chunks.push_back(grid[j]);
      chunk_slot.push_back(slot_of[j]);
    }
  }
  // AdamW work items: this rank's body slice of every bucket (all of them for the loopback) and every tail, cut at the boundaries of the
  // parameter groups when a scale table is set
  std::vector<ScaleRun> runs;
  if (h->grouped()) runs = scale_runs(h->plan, h->lr_scale.data(), h->wd_scale.data());
  const WorkItems it = cut_items(shard_share(plan, world, rank, all_ranks), h->grouped() ? &runs : nullptr);
  if (int e = h->shard_work.upload(it.items, chunks, chunk_slot, slot_of, it.scales)) return e;
  h->shard_world = world;
  h->shard_rank = rank;
  h->shard_slots = S;
  h->shard_plan = plan;
  if (slots_per_rank) *slots_per_rank = S;
  return 0;
}

extern "C" int gget_shard_bucket(gget_handle_t h, int bucket, uint64_t out[5]) {
  GGET_REQUIRE(h != nullptr && out != nullptr, "shard_bucket: null argument");
  GGET_REQUIRE(h->shard_world > 0, "shard_bucket: no plan is active (gget_shard_init)");
  GGET_REQUIRE(bucket >= 0 && bucket < (int)h->shard_plan.size(), "shard_bucket: bucket %d out of range", bucket);
  const ShardBucket& sb = h->shard_plan[bucket];
  out[0] = sb.off, out[1] = sb.cnt, out[2] = sb.slice, out[3] = sb.tail_off, out[4] = sb.tail_cnt;
  return 0;
}

extern "C" int gget_shard_sqnorm_partials(gget_handle_t h, float* slots_dev, void* stream) {
  GGET_REQUIRE(h && h->shard_world > 0 && slots_dev, "shard_sqnorm_partials: call gget_shard_init first (and pass the slot vector)");
  // (an open accumulation window: the chunks of the fp32 sum; the window stays open for gget_adamw_step_sharded, which closes it)
  const OptWork& w = h->shard_work;
  return k_grad_sqnorm_partials(h->grad_src(), w.chunks, w.chunk_slot, w.nchunks, slots_dev, (hipStream_t)stream, h->grad_from_acc());
}

extern "C" int gget_adamw_step_sharded(gget_handle_t h, float lr, float beta1, float beta2, float eps, float weight_decay,
                                       float max_grad_norm, float grad_scale, int step, const float* slots_dev, float* gnorm_dev, void* stream) {
  GGET_REQUIRE(h && h->master && h->am && h->av, "adamw needs master/m/v arenas");
  GGET_REQUIRE(h->shard_world > 0, "adamw_step_sharded: call gget_shard_init first");
  GGET_REQUIRE(step >= 1, "step is 1-based");
  GGET_REQUIRE(slots_dev || !h->step_needs_norm(max_grad_norm, gnorm_dev), "adamw_step_sharded: the norm needs the gathered partial vector");
  return optimizer_step(h, true, lr, beta1, beta2, eps, weight_decay, max_grad_norm, grad_scale, step, slots_dev, gnorm_dev, (hipStream_t)stream);
}
