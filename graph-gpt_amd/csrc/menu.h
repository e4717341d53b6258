// The launch menu: every knob that steers kernel selection in libgget_hip.so, in one struct and one table.
//
// kMenuRows is the one description of the knobs (INTEGRATION.md "Kernel-selection knobs" mirrors it row for row).  The process menu is
// read from the environment once, when the library loads (menu.hip); gget_debug_set / gget_debug_get write and read it by key
// afterwards.  A handle that carries a data-parallel menu (gget_set_dp_menu) overlays its fields on the process menu for the length of
// each of its calls (engine.h CallScope); menu() returns what the current call plans with.  The defaults are the measured best.
#pragma once

struct LaunchMenu {
  // GEMM launch plans (gemm.hip)
  int gemm_variant;         // bit mask of kGemm* below
  int gemm_lds_headroom;    // 1: 3-slot rings for the 128x192 / 192x128 tiles, 0: 4 slots, 2: also no launch with two LDS-filling blocks per CU
  int gemm_split_last;      // split the K range of the last, partial round's tiles among the idle blocks (stream-K)
  int gemm_stagger_ticks;   // MODE 2 launches: start delay of a CU's second workgroup in 100 MHz ticks
  int gemm_ablate;          // diagnostics: 1 no LDS-DMA, 2 no MFMA / ds_read, 4 no C store, 32 persistent kernel without the epilogue
  int gemm_cu_reserve;      // CUs every GEMM plan leaves free for a collective's workgroups
  int gemm_num_cu;          // > 0: plan for this many CUs instead of the device's
  int gemm_no_persist;      // no persistent kernels
  int gemm_no_dyn;          // no persistent kernels for launches whose row / K count lives on the device
  int gemm_no_256;          // no 256x256 tiles
  int gemm_bk64;            // 256x256 NT tiles with 64-deep K-tiles (0: 32-deep)
  int gemm_192;             // 128x192 / 192x192 tiles
  int gemm_super;           // > 0: tile-order supergroup size of every launch
  // attention (attention.hip)
  int attn_by_sample;       // var-len layout, 32 < S <= 64: every sample by its own row count
  int attn_big;             // S >= 256: the 64-row staged kernels
  int attn_dense;           // S >= 512 without key ranges / causal mask: the dense forward
  int attn_small;           // S <= 64: the per-sample backward kernels
  int attn_fused;           // S >= attn_fused_min_s: the one-pass backward
  int attn_fused_min_s;
  int attn_stg128;          // S >= 512: dK / dV kernel with 128-row stages (0: 64)
  int attn_oproj;           // S <= 32: attention + o projection + residual + RMSNorm per sample (environment switch)
  int attn_oproj_off;       // ... the same form switched off at run time
  // engine (engine.hip; ls_norm_bwd_wide is read in residual.hip, occupy_fat in ops.hip)
  int head_sorted;          // SMTP head: the labelled cells sorted by slot
  int head_dense;           // SMTP head: dense projection of every selected row through all slots
  int head_tile;            // 0: 256-row slot tiles when d % 256 == 0, else 128; 128 / 256: forced
  int no_head_scatter_fusion;
  int no_geglu_fusion;
  int no_ls_norm_fusion;
  int ls_norm_bwd_wide;     // fused RMSNorm + LayerScale backward in the 16-byte-chunk form for every width
  int no_varlen;
  int count_copy;           // the token count comes back by copy + event instead of a polled pinned word
  int embed_sorted;         // embedding backward: always the sorted scatter-add
  int occupy_fat;           // gget_debug_occupy: the stand-in takes RCCL's register footprint
  // small kernels (kernels.hip)
  int deterministic;        // reproducible mode: RMSNorm weight gradients summed in block order
  int rms_wide;             // short RMSNorm backward launches: one 16-wave block per CU
  int rms_rows;             // RMSNorm backward: rows per wave
  int ce_parts;             // cross-entropy: one partial loss sum per block instead of an atomic
  int ce_generic;           // cross-entropy: never the vectorised row kernels
  // evaluation metrics (metrics.hip)
  int link_grid;            // > 0: most workgroups a streaming launch of the link metrics takes (0: 1024, four per CU)
};

// gget_debug_set / gget_debug_get key 1: bits that switch GEMM kernel variants (0 = the shipped selection)
enum : int {
  kGemmNoKsplitNd = 1,      // OFF: the K-split kernel for one-round N = d launches
  kGemmNoKsplitWgrad = 2,   // OFF: the K-split kernel for the grouped weight gradients
  kGemmNo192Rows = 4,       // OFF: the 192-row tiles
  kGemmNoSplitLast = 8,     // OFF: the split of the last round
  kGemmKsplit128Only = 16,  // OFF: the 64- / 96-row tiles of the K-split kernel
  kGemmOneBlockPerCu = 32,  // OFF: two co-resident workgroups per CU for the dh + GEGLU' launch
  kGemmKsplitDma8 = 128,    // ON: all eight waves of the K-split kernel issue its LDS-DMA (default: four)
  kGemmAreaRule = 512,      // ON: N = d launches keep the default tiling whenever its rounds x area is the smaller one
};

struct MenuRow {
  int LaunchMenu::*field;
  int key;             // gget_debug_set / gget_debug_get key, 0 = none
  const char* env;     // environment variable, nullptr = none
  bool env_presence;   // the variable's presence sets 1 (its value is not read)
  int def;
  const char* meaning;
};

inline constexpr MenuRow kMenuRows[] = {
    {&LaunchMenu::gemm_variant, 1, "GGET_GEMM_VARIANT", false, 0, "bit mask of GEMM kernel variants (kGemm*)"},
    {&LaunchMenu::gemm_lds_headroom, 2, "GGET_GEMM_LDS_HEADROOM", false, 1, "LDS headroom of the 128x192 / 192x128 tiles: 0 4-slot rings, 1 3-slot, 2 also one block per CU"},
    {&LaunchMenu::gemm_split_last, 3, "GGET_GEMM_SPLIT_LAST", false, 0, "1: split the K range of the last, partial round's tiles among the idle blocks"},
    {&LaunchMenu::deterministic, 4, "GGET_DETERMINISTIC", false, 0, "1: reproducible mode, RMSNorm weight gradients summed in block order"},
    {&LaunchMenu::gemm_stagger_ticks, 5, "GGET_GEMM_STAGGER", false, 0, "MODE 2 GEMM launches: start delay of a CU's second workgroup (100 MHz ticks)"},
    {&LaunchMenu::gemm_ablate, 7, "GGET_GEMM_ABLATE", false, 0, "GEMM diagnostics: 1 no LDS-DMA, 2 no MFMA, 4 no C store, 32 no epilogue (timing only)"},
    {&LaunchMenu::head_dense, 8, nullptr, false, 0, "1: SMTP head as a dense projection through all slots"},
    {&LaunchMenu::head_tile, 9, nullptr, false, 0, "SMTP head slot tile rows: 0 automatic, 128 / 256 forced"},
    {&LaunchMenu::attn_oproj_off, 10, nullptr, false, 0, "1: S <= 32 attention, o projection, RMSNorm as three launches"},
    {&LaunchMenu::ls_norm_bwd_wide, 11, "GGET_LS_NORM_BWD_WIDE", false, 0, "1: fused RMSNorm + LayerScale backward in its 16-byte-chunk form for every width"},
    {&LaunchMenu::rms_wide, 13, "GGET_RMS_WIDE", false, 1, "0: short RMSNorm backward launches in 4-wave blocks instead of one 16-wave block per CU"},
    {&LaunchMenu::ce_parts, 14, "GGET_CE_PARTS", false, 1, "0: cross-entropy adds its loss with one atomic per block instead of per-block partial sums"},
    {&LaunchMenu::gemm_cu_reserve, 15, nullptr, false, 0, "CUs every GEMM plan leaves free for a collective's workgroups"},
    {&LaunchMenu::occupy_fat, 16, nullptr, false, 0, "1: gget_debug_occupy's stand-in takes RCCL's register footprint"},
    {&LaunchMenu::link_grid, 18, nullptr, false, 0, "> 0: most workgroups a streaming launch of the link metrics takes (0: 1024)"},
    {&LaunchMenu::gemm_num_cu, 0, "GGET_GEMM_NUM_CU", false, 0, "> 0: GEMM plans pretend the chip has this many CUs"},
    {&LaunchMenu::gemm_no_persist, 0, "GGET_GEMM_NO_PERSIST", true, 0, "set: no persistent GEMM kernels"},
    {&LaunchMenu::gemm_no_dyn, 0, "GGET_GEMM_NO_DYN", true, 0, "set: no persistent GEMM kernels for device-sized launches"},
    {&LaunchMenu::gemm_no_256, 0, "GGET_GEMM_NO_256", true, 0, "set: no 256x256 GEMM tiles"},
    {&LaunchMenu::gemm_bk64, 0, "GGET_GEMM_BK64", false, 1, "0: 256x256 NT tiles with 32-deep instead of 64-deep K-tiles"},
    {&LaunchMenu::gemm_192, 0, "GGET_GEMM_192", false, 1, "0: no 128x192 / 192x192 GEMM tiles"},
    {&LaunchMenu::gemm_super, 0, "GGET_GEMM_SUPER", false, 0, "> 0: tile-order supergroup size of every GEMM launch"},
    {&LaunchMenu::attn_by_sample, 0, "GGET_ATTN_BY_SAMPLE", false, 1, "0: var-len 32 < S <= 64 attention keyed by S instead of every sample's own rows"},
    {&LaunchMenu::attn_big, 0, "GGET_ATTN_BIG", false, 1, "0: S >= 256 attention on the register-prefetch kernels"},
    {&LaunchMenu::attn_dense, 0, "GGET_ATTN_DENSE", false, 1, "0: no dense attention forward for S >= 512"},
    {&LaunchMenu::attn_small, 0, "GGET_ATTN_SMALL", false, 1, "0: no per-sample attention backward for S <= 64"},
    {&LaunchMenu::attn_fused, 0, "GGET_ATTN_FUSED", false, 1, "0: long-sequence attention backward as two kernels instead of one pass"},
    {&LaunchMenu::attn_fused_min_s, 0, "GGET_ATTN_FUSED_MIN_S", false, 256, "sequence length from which the one-pass attention backward runs"},
    {&LaunchMenu::attn_stg128, 0, "GGET_ATTN_STG128", false, 1, "0: S >= 512 dK / dV kernel with 64-row instead of 128-row stages"},
    {&LaunchMenu::attn_oproj, 0, "GGET_ATTN_OPROJ", false, 1, "0: S <= 32 attention, o projection, RMSNorm as three launches"},
    {&LaunchMenu::head_sorted, 0, "GGET_HEAD_SORTED", false, 1, "0: SMTP head as a dense projection through all slots"},
    {&LaunchMenu::no_head_scatter_fusion, 0, "GGET_NO_HEAD_SCATTER_FUSION", true, 0, "set: SMTP head rows scattered by their own launch (implies the dense head)"},
    {&LaunchMenu::no_geglu_fusion, 0, "GGET_NO_GEGLU_FUSION", true, 0, "set: GEGLU as GEMM + element-wise kernel"},
    {&LaunchMenu::no_ls_norm_fusion, 0, "GGET_NO_LS_NORM_FUSION", true, 0, "set: LayerScale residual and the next RMSNorm as separate launches"},
    {&LaunchMenu::no_varlen, 0, "GGET_NO_VARLEN", true, 0, "set: the padded token grid instead of the var-len layout"},
    {&LaunchMenu::count_copy, 0, "GGET_COUNT_COPY", false, 0, "1: token count back by device-to-host copy + event instead of a polled host word"},
    {&LaunchMenu::embed_sorted, 20, "GGET_EMBED_SORTED", true, 0, "set: embedding backward always as the sorted scatter-add"},
    {&LaunchMenu::rms_rows, 0, "GGET_RMS_ROWS", false, 4, "RMSNorm backward rows per wave"},
    {&LaunchMenu::ce_generic, 19, "GGET_CE_GENERIC", true, 0, "set: cross-entropy never on the vectorised row kernels"},
};

extern LaunchMenu g_menu;                              // the process menu (menu.hip)
extern thread_local const LaunchMenu* t_call_menu;    // the menu of the handle call running on this thread, or nullptr
inline const LaunchMenu& menu() { return t_call_menu ? *t_call_menu : g_menu; }
