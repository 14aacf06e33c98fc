// c3_plan: which kernels one conv3x3 layer runs, as a function of its SHAPE alone -- precision, batch, map size, channels, fused pool, whether
// the full-resolution map is kept, the dup_hi layout, the two split-precision options and the device's CU count. No device call, no pointer:
// launch_conv3x3 (conv3x3.hip) computes the plan once and every launcher below it (c3_run_*, c3_dispatch, c3_launch_edge) takes its decision
// from the plan, so what ctpn_debug_conv3x3_plan reports IS the code path. tests/conv_forms.py enumerates the plans the network can reach.
#pragma once
#include "common.h"

namespace ctpn {

constexpr int C3_BM = 256;                   // output pixels of one tile
constexpr int C3_LDS_MAX = 160 * 1024;       // a CU's LDS: the budget of every launch here, and what raise_dynamic_lds (common.h) asks for per kernel

// The main launch. Names (c3_main_name) are part of the debug ABI: tests and failure messages quote them.
enum C3Main : int {
  C3M_NONE = -1,          // no kernel for this shape (split precision: Co must be <= 64 or a multiple of 128, with ReLU)
  C3M_WR = 0,             // "wr":          weights-in-registers kernel (16-bit modes, Ci = 64, Co = 64 / 128): conv3x3_wr.h
  C3M_P64,                // "p64":         persistent kernel's 64-channel form (split precision, Co = 64, option conv_p64)
  C3M_T64,                // "t64":         non-persistent kernel, 256 x 64 tiles (Co <= 64)
  C3M_P_FLAT,             // "p_flat":      persistent, flat windows of 256 pixels
  C3M_P_FLAT64,           // "p_flat64":    persistent, flat 64-pixel x 128-channel items (one round on the machine)
  C3M_P_16X16,            // "p_16x16":     persistent, 16 x 16 patches
  C3M_P_8X32,             // "p_8x32":      persistent, 8 x 32 patches
  C3M_P_8X32_HALF,        // "p_8x32_half": persistent, 8 x 32 patches with the half-tile tail (one or two images)
  C3M_T_FLAT,             // "t_flat":      non-persistent 256 x 128 tiles (Co not a multiple of 128, or no ReLU), flat windows
  C3M_T_16X16,            // "t_16x16":     ... 16 x 16 patches
  C3M_T_8X32,             // "t_8x32":      ... 8 x 32 patches
  C3M_COUNT
};
// What happens to the ragged right-hand pixel columns of a 2D tiling.
enum C3Strip : int {
  C3S_NONE = 0,           // "none":      the main launch covers the whole width (padded last tile column)
  C3S_EDGE,               // "edge":      one or two columns beyond a multiple of 16 through conv3x3_edge_kernel
  C3S_EDGE_POOL,          // "edge_pool": two or four columns of a pooled layer through the edge kernel's pooled form (and, when the full map is
                          //              kept, through its plain form as well)
  C3S_IM2COL,             // "im2col":    one to eight columns beyond a multiple of 32 through the im2col GEMM (igemm.hip)
  C3S_COUNT
};
static inline const char* c3_main_name(int m) {
  static const char* const names[C3M_COUNT] = {"wr", "p64", "t64", "p_flat", "p_flat64", "p_16x16", "p_8x32", "p_8x32_half", "t_flat", "t_16x16", "t_8x32"};
  return m >= 0 && m < C3M_COUNT ? names[m] : nullptr;
}
static inline const char* c3_strip_name(int s) {
  static const char* const names[C3S_COUNT] = {"none", "edge", "edge_pool", "im2col"};
  return s >= 0 && s < C3S_COUNT ? names[s] : nullptr;
}

struct C3Plan {
  int main_form;      // C3Main
  int strip;          // C3Strip
  int strip_cols;     // columns [w - strip_cols, w) belong to the strip (0: none)
  int w_cover;        // columns [0, w_cover) belong to the main launch; 0 = all of them
  int deep;           // edge strips: 1 = the deep form in the layer's own stream behind the main launch, 0 = forked onto the helper stream
                      // (the im2col strip is always forked)
  int edge_ks;        // edge strips: waves that share one tile's K steps (split precision: 3 or 6 by Ci; else 1). 0 without an edge strip
};

// pixels the 2D tiling has to cover: a fused 2x2 VALID pool that does not keep the full-resolution map never reads an
// odd last row / column (150 x 225 -> 75 x 112 uses 150 x 224), which for W = 225 = 7 * 32 + 1 removes a whole tile column
static inline void c3_extent_of(int h, int w, bool pool, bool keep_full, int w_cover, int& he, int& we) {
  he = (pool && !keep_full) ? (h & ~1) : h;
  we = (pool && !keep_full) ? (w & ~1) : w;
  if (w_cover > 0 && w_cover < we) we = w_cover;
}
static inline long long c3_tiles2d_of(int h, int w, bool pool, bool keep_full, int w_cover, int tw) {
  int he, we;
  c3_extent_of(h, w, pool, keep_full, w_cover, he, we);
  const int th = C3_BM / tw;
  return (long long)((we + tw - 1) / tw) * ((he + th - 1) / th);
}
// flat windows need 256 + 2(W+2) + 2 rows per buffer; they must fit LDS twice next to nb weight strips
static inline bool c3_flat_ok_of(int w, int co, bool pool, int nb = 3) {
  const int flat_rows = (C3_BM + 2 * (w + 2) + 2 + 7) & ~7;
  const int bias_bytes = ((co + 127) / 128) * 128 * 4;      // the persistent kernel keeps the bias vector in LDS as well
  return !pool && (w + 2) <= 114 && (2 * flat_rows * 128 + nb * 128 * 128 + bias_bytes) <= C3_LDS_MAX;
}

// ci / co: the layer's channel counts (split precision too). keep_full: the full-resolution map is stored (always, without a pool).
// split_opts: bit 0 = option conv_p64, bit 1 = option split_edge. ncu: the device's CU count (> 0).
static inline C3Plan c3_plan(DType t, int n, int h, int w, int ci, int co, bool pool, bool keep_full, int dup_hi, bool relu, bool has_bias,
                             int split_opts, int ncu) {
  (void)dup_hi;      // a layout of the stores (split precision: [hi | lo | hi]); it selects no kernel
  C3Plan p{};
  const bool half = dtype_is_half(t), split = t == DType::SPLIT;
  const bool flat = c3_flat_ok_of(w, co, pool);
  // ---- the strip ----
  // Ragged last tile column (W = 225 = 7 * 32 + 1 wastes an eighth of the tiles on one pixel column): the 2D launch covers
  // the multiple of 32 and the few remaining columns go through the im2col kernel (igemm.hip) as a [N*H*r] x Co GEMM (fp32).
  // 16-bit modes: one or two columns beyond a multiple of 16 go through conv3x3_edge_kernel, which shares the CUs with the main
  // launch (W = 113 then tiles as 7 x 16 instead of 8 x 16); otherwise up to 8 columns beyond a multiple of 32 go through igemm.
  // Split precision (round 6): the same edge kernel over [hi | lo] planes (three K blocks per tap); no igemm strip there.
  const bool half_or_split = half || (split && (split_opts & 2) != 0);
  const bool can_strip = !pool && !flat && w > 32 && keep_full;
  const bool edge = can_strip && half_or_split && has_bias && co % 64 == 0 && w % 16 >= 1 && w % 16 <= 2;
  // 16-bit layers with a fused pool and no full-resolution output (conv1_2: W = 900 = 28 * 32 + 4; conv2_2: 450 = 28 * 16 + 2): two or
  // four columns beyond the main launch's tile width go through the pooled form of the edge kernel (whole pooled pixels lie inside them)
  const bool wr_layer = half && ci == 64 && (co == 64 || co == 128) && has_bias && relu;
  const int rp = w % (wr_layer ? 32 : 16);
  // (when the full-resolution map is kept as well -- keep_acts -- the same columns also go through the plain edge kernel: both
  // forms accumulate in the same order, so the stored pool stays the exact max of the stored map and equal to the production path's)
  // NOT for conv1_2 (Ci = Co = 64 with the pool): since conv1_1 is computed inside its window stage the persistent workgroups fill 456 of a
  // SIMD's 512 registers, ONE edge wave fits next to them instead of three, and the strip -- which also needs conv1_1 for its own columns
  // first -- ended 15 us AFTER the main launch instead of inside it, its one-wave workgroups crowding onto the CUs of the previous batch's NMS
  // (1.3 ms instead of 0.54). The padded 29th tile column costs the main launch 3.5 %; the decision depends on the layer's shape only, so the
  // stored (keep_acts) form takes the same columns through the same kernel family.
  const bool conv1_2_like = wr_layer && co == 64 && pool;
  const bool edge_pool = !conv1_2_like && pool && half_or_split && has_bias && co % 64 == 0 && w > 64 && h >= 2 && (w & 1) == 0 && (rp == 2 || rp == 4);
  const int r = edge_pool ? rp : (edge ? w % 16 : w % 32);
  // (which columns go to a strip depends on the layer's shape only, never on the batch: the edge kernel and the main kernels sum K in
  // different orders, and a batch must reproduce its images run alone bit for bit)
  const bool strip = edge_pool || (can_strip && (edge || (!split && r >= 1 && r <= 8)));
  if (strip) {
    p.strip = edge_pool ? C3S_EDGE_POOL : (edge ? C3S_EDGE : C3S_IM2COL);
    p.strip_cols = r;
    p.w_cover = w - r;
  }
  if (p.strip == C3S_EDGE || p.strip == C3S_EDGE_POOL) {
    // One or two images: the edge kernel runs in the layer's own stream, behind the main launch, in its DEEP form (conv3x3_edge.h) -- no fork,
    // no join. WHICH columns it takes is still a function of the layer's shape alone, and the deep form issues the same MFMAs in the same
    // order, so a batch and its images run alone still agree bit for bit.
    // Split precision, any batch: in the stream as well. Beside the main launch (forked, in front of it or behind it) the one-wave workgroups
    // run for as long as the main launch does -- its two waves per SIMD hold 2 x 183 .. 246 of the 512 registers, the edge waves take the places
    // of main workgroups that then start late -- and end 60 .. 270 us after it: -3 % images/s against a padded tile column. Behind the main
    // launch on an empty machine the deep form takes 30 .. 60 us per layer: +1.8 % (tools/r6_split_edge_ab.sh, one context per process).
    p.deep = (n <= 2 || split) ? 1 : 0;
    p.edge_ks = 1;
    if (split) {
      // K split over waves, by Ci alone: S = 27 Ci / 16 K steps = 108 / 216 / 432 for Ci = 64 / 128 / 256 -> 3 / 6 / 6 waves of 36 / 36 / 72 steps
      const int S = 27 * (ci / 16);
      p.edge_ks = S % 24 == 0 && S / 6 >= 36 ? 6 : (S % 12 == 0 && S / 3 >= 36 ? 3 : 1);
    }
  }
  // ---- the main launch ----
  auto tiles = [&](int tw) { return c3_tiles2d_of(h, w, pool, keep_full, p.w_cover, tw); };
  if (wr_layer) { p.main_form = C3M_WR; return p; }
  // conv1_2 in split precision (option conv_p64, default 1): the persistent kernel's 64-channel form, 3.56 ms against the
  // non-persistent kernel's 4.53 at batch 32 (same box: 1145 against 1115 images/s, profiles/r06_ab_split_conv1.txt). NOT fp32: exact-fp32
  // MFMAs are 16 x slower per flop, the per-tile fixed costs the persistent form removes are 1 % there (measured: 352.3 against 353.4
  // images/s at batch 8)
  if (split && co == 64 && relu && (split_opts & 1) != 0) { p.main_form = C3M_P64; return p; }
  if (co <= 64) { p.main_form = C3M_T64; return p; }
  const bool persist = co % 128 == 0 && relu;      // the persistent kernel's epilogue has the ReLU built in
  // 16 x 16 patches where they cover the map with fewer tiles. (Round 6 also tried choosing by ROUNDS of the persistent walk for one-image
  // problems -- conv3_x of one 600 x 900 image is 266 8 x 32-patch tiles on 256 CUs, two rounds for ten tiles, against 280 16 x 16-patch tiles =
  // one round + a half-tile tail: measured 45.0 / 28.2 / 45.4 / 46.7 us for conv2_2 .. conv3_3 against 39.0 / 29.3 / 48.2 / 45.5 with this
  // rule -- the 16 x 16 kernel's tile is slower than the 8 x 32 kernel's by what the tail saves; profiles/r06_timeline_sync_1image_tiling_by_rounds.txt.)
  const bool tw16 = !flat && tiles(16) < tiles(32);
  if (!persist) {
    p.main_form = split ? C3M_NONE : (flat ? C3M_T_FLAT : (tw16 ? C3M_T_16X16 : C3M_T_8X32));
    return p;
  }
  const long long tn = (co + 127) / 128;
  if (flat) {
    // one image per call (conv5_x / rpn_conv of a 600 x 900 image: 36 tiles of 256 x 128): 64-pixel x 128-channel items, one round on the machine
    const long long m_total = (long long)n * (h + 2) * (w + 2);
    const long long t256 = (m_total + 255) / 256 * tn, t64 = (m_total + 63) / 64 * tn;
    p.main_form = (2 * (w + 2) + 66 <= 37 * 8 && 2 * t256 <= ncu && t64 <= ncu) ? C3M_P_FLAT64 : C3M_P_FLAT;
    return p;
  }
  if (tw16) { p.main_form = C3M_P_16X16; return p; }
  p.main_form = C3M_P_8X32;
  // one or two images per call: 8 x 32 patches with a half-tile tail where the walk's last round is at most half full (conv3_x of one
  // 600 x 900 image: 266 tiles on 256 CUs -- the ten tiles of the second round as twenty halves: 1.59 rounds instead of 2).
  // (At batch 32 -- conv3_x: 33 rounds + 64 tiles -- the same form measured -0.5 % images/s in bf16, +0.2 % in split precision, round 6 on
  // the final tree: the tail it shortens is where the forked edge kernels run. Not used there.)
  if (n <= 2 && ncu > 0) {
    const long long tt = tiles(32) * n * tn;
    const long long G = tt < ncu ? tt : ncu, full = tt / G, rr = tt % G;
    if (2 * tt <= ncu || (rr > 0 && 2 * rr <= G && full <= 3)) p.main_form = C3M_P_8X32_HALF;
  }
  return p;
}

// c3_walk: how the main launch of a persistent form (conv3x3_p_kernel) or of the weights-in-registers kernel (conv3x3_wr_kernel) walks its
// tiles, again as a function of the shape and the CU count alone. c3_dispatch / c3_launch_wr compute it and the launchers copy it into the
// kernel argument, so what ctpn_debug_conv3x3_walk_plan reports IS the launch. tests/conv_walks.py enumerates the situations of the walk.
struct C3Walk {
  int main_form;            // C3Main; a form without a walk (t64, t_*) leaves everything below zero
  // the kernel instantiation the form names (c3_launch_p checks them against its template arguments)
  int flat, tw, bn, bm, ht; // flat windows / patch width / channels and pixels of one tile / does the form split its tail tiles into halves
  int tiles_x, tiles_y;     // 2D patches: tile columns; tile rows per image (stacked: of the whole bordered batch). wr: per image
  int tiles_n;              // channel slices (p: of bn channels; wr: of 64)
  int stacked;              // p, 2D patches without a fused pool: tile rows run over the bordered rows of the whole batch
  long long m_total;        // p, flat windows: bordered pixels of the batch
  long long ptiles;         // pixel tiles
  long long ptiles_total;   // p: work items of whole tiles = ptiles x tiles_n. wr: = ptiles (every slice walks all of them)
  long long workers;        // p: the grid. wr: workgroups per group and channel slice
  long long grid;           // workgroups of the launch
  long long ht_full;        // p: tiles [0, ht_full) are walked whole ...
  int ht_r;                 // ... and the ht_r tiles behind them as two halves each (0: no halves)
  int groups, per_group;    // wr: tile ranges (one per XCD) and tiles per range; the last range may be shorter, or empty
};

// the instantiation of conv3x3_p_kernel behind a main form (c3_dispatch's table): false for a form the persistent kernel does not serve
static inline bool c3_walk_p_shape(int form, C3Walk& k) {
  k.flat = 0; k.tw = 32; k.bn = 128; k.bm = C3_BM; k.ht = 0;
  switch (form) {
    case C3M_P64: k.bn = 64; return true;
    case C3M_P_FLAT: k.flat = 1; k.ht = 1; return true;
    case C3M_P_FLAT64: k.flat = 1; k.bm = 64; return true;
    case C3M_P_16X16: k.tw = 16; k.ht = 1; return true;
    case C3M_P_8X32: return true;
    case C3M_P_8X32_HALF: k.ht = 1; return true;
    default: return false;
  }
}

// n, h, w, co: the layer (split precision: its channel count, not the planes'). keep_full: the full-resolution map is stored.
// w_cover: the plan's (columns of the main launch; 0 = all). ncu: the CU count the launch is laid out for (> 0).
static inline C3Walk c3_walk(int form, int n, int h, int w, int co, bool pool, bool keep_full, int w_cover, int ncu) {
  C3Walk k{};
  k.main_form = form;
  int he, we;
  c3_extent_of(h, w, pool, keep_full, w_cover, he, we);
  if (form == C3M_WR) {
    k.tw = 32; k.bn = 64; k.bm = C3_BM;
    k.tiles_x = (we + 31) / 32;
    k.tiles_y = (he + 7) / 8;
    k.tiles_n = co / 64;
    k.ptiles = (long long)n * k.tiles_x * k.tiles_y;
    k.ptiles_total = k.ptiles;
    k.groups = 8;                                                      // one tile range per XCD (kernel comment)
    const long long per_group = (k.ptiles + k.groups - 1) / k.groups;
    k.per_group = (int)(per_group < 0x7fffffffLL ? per_group : 0x7fffffffLL);
    long long workers = k.tiles_n > 0 ? (ncu / k.tiles_n) / (long long)k.groups : 0;      // per group and channel slice
    if (workers < 1) workers = 1;
    if (workers > per_group) workers = per_group;
    k.workers = workers;
    k.grid = workers * k.groups * k.tiles_n;
    return k;
  }
  if (!c3_walk_p_shape(form, k)) { k.tw = k.bn = k.bm = 0; return k; }
  k.tiles_n = (co + k.bn - 1) / k.bn;
  if (k.flat) {
    k.m_total = (long long)n * (h + 2) * (w + 2);
    k.ptiles = (k.m_total + k.bm - 1) / k.bm;
  } else {
    const int th = C3_BM / k.tw;
    k.tiles_x = (we + k.tw - 1) / k.tw;
    k.tiles_y = (he + th - 1) / th;
    k.ptiles = (long long)n * k.tiles_x * k.tiles_y;
    // Stacked tile rows (no fused pool): the bordered NHWC batch is ONE tall image of N (H + 2) rows -- image i's bottom border row is
    // followed by image i + 1's top border row, which is exactly the zero halo both need -- so tile rows can run over the batch's
    // N (H + 2) - 2 rows instead of restarting per image: 75-row maps in 16-row patches pay 80 rows per image, stacked 2462 rows pay 2464
    // (conv4_1 / conv4_2: 1078 instead of 1120 tiles). Border rows that fall inside a tile are computed and not stored (the output's
    // borders must stay zero).
    if (!pool) {
      const long long ty_st = ((long long)n * (h + 2) - 2 + th - 1) / th;
      if (h >= 16 && n > 1 && ty_st < (long long)n * k.tiles_y && ty_st * k.tiles_x < 0x7fffffffLL) {
        k.stacked = 1;
        k.tiles_y = (int)ty_st;
        k.ptiles = (long long)k.tiles_x * k.tiles_y;
      }
    }
  }
  k.ptiles_total = k.ptiles * k.tiles_n;
  k.workers = k.ptiles_total < ncu ? k.ptiles_total : ncu;
  // half-tile tail (kernel comment): the r tiles of a last partial round as 2 r halves; a launch with at most half as many tiles as CUs
  // (small batches: conv5_x of ONE 600 x 900 image is 36 tiles) is split into halves altogether -- a half runs one wave per SIMD and takes
  // 0.59 of a tile's time. Same K order per output either way: results do not depend on the split.
  k.ht_full = k.ptiles_total; k.ht_r = 0;
  if (k.ht && k.ptiles_total > 0) {
    if (2 * k.ptiles_total <= ncu) { k.ht_full = 0; k.ht_r = (int)k.ptiles_total; k.workers = 2 * k.ptiles_total; }
    else {
      const long long r = k.ptiles_total % k.workers;
      if (r > 0 && 2 * r <= k.workers) { k.ht_r = (int)r; k.ht_full = k.ptiles_total - r; }
    }
  }
  k.grid = k.workers;
  return k;
}

}  // namespace ctpn
