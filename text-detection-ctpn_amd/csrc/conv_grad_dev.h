// The backward pass through the conv stack (include/ctpn_hip.h, "the conv stack: backward"): the per-thread text of conv_grad.hip's kernels as
// host + device functions. The kernels call these bodies with their own indices; tests/conv_grad_host.cpp compiles this same text with g++
// under ASan + UBSan (-ffp-contract=off, as the Makefile gives conv_grad.hip) and calls it from loops over whole small problems.
//   cg_pixel_coords    flat pixel index (image, row, column order) -> (row, column) inside its image
//   cg_tap_ok          border and image-seam predicate: does the pixel (dy, dx) away from (i, j) lie inside the SAME image
//   cg_tap_offset      the flat distance to that pixel, valid where cg_tap_ok holds
//   cg_relu_mask       dZ = d_y where the stored post-ReLU output is positive
//   cg_pool_first_max  the 2x2 window's first maximum in (row, column) scan order: torch's rule for exact ties
//   cg_pool_backward   one element of d_full
//   cg_plan            the weight gradient's pixel blocks: a function of the shape alone
// The ordered pass over the blocks' partial sums and the bias sums over one block are the tail's (tb_tn_reduce, tb_colsum_block).
// Nothing here includes a HIP header.
#pragma once
#include "tail_grad_dev.h"

#define CG_HD TB_HD

namespace ctpn {

constexpr int CG_MAX_BLOCKS = 32;        // partial sums per element of d_w at the most: scratch stays at or below 32 copies of d_w
constexpr int CG_BLOCK_UNIT = 64;        // a block is a multiple of this many pixels
constexpr int CG_TARGET_GROUPS = 1024;   // workgroups the weight-gradient launch aims at: a constant, not the device's CU count
constexpr int CG_C_TILE = 16;            // input channels per workgroup of the weight gradient
constexpr int CG_O_TILE = 64;            // output channels per workgroup of the weight gradient

CG_HD void cg_pixel_coords(long long p, int h, int w, int& i, int& j) {
  j = (int)(p % w);
  i = (int)((p / w) % h);
}

CG_HD bool cg_tap_ok(int h, int w, int i, int j, int dy, int dx) { return i + dy >= 0 && i + dy < h && j + dx >= 0 && j + dx < w; }
CG_HD long long cg_tap_offset(int w, int dy, int dx) { return (long long)dy * w + dx; }

CG_HD float cg_relu_mask(float d_y, float y) { return y > 0.f ? d_y : 0.f; }

// v[0..3] = the window's values at (0,0), (0,1), (1,0), (1,1) -> the index of the first one no later value exceeds
CG_HD int cg_pool_first_max(float v0, float v1, float v2, float v3) {
  int k = 0;
  float best = v0;
  if (v1 > best) { best = v1; k = 1; }
  if (v2 > best) { best = v2; k = 2; }
  if (v3 > best) { best = v3; k = 3; }
  return k;
}

// d_full at (i, j) of an h x w map, channel stride c: y_img / d_pool_img point at channel ch of the image's first pixel. The last row or
// column of an odd-sized map lies in no window
CG_HD float cg_pool_backward(const float* y_img, const float* d_pool_img, int h, int w, size_t c, int i, int j) {
  const int hp = h / 2, wp = w / 2, wi = i / 2, wj = j / 2;
  if (wi >= hp || wj >= wp) return 0.f;
  const float* y0 = y_img + ((size_t)(2 * wi) * w + (size_t)(2 * wj)) * c;
  const int k = cg_pool_first_max(y0[0], y0[c], y0[(size_t)w * c], y0[(size_t)w * c + c]);
  return k == (i & 1) * 2 + (j & 1) ? d_pool_img[((size_t)wi * wp + (size_t)wj) * c] : 0.f;
}

// The weight gradient's plan. The launch has ceil(ci / 16) x (co / 64) workgroups per block of pixels; the blocks wanted are what brings
// that to CG_TARGET_GROUPS, between 1 and CG_MAX_BLOCKS; a block is the pixel count divided by that, rounded up to a multiple of
// CG_BLOCK_UNIT. blocks = ceil(M / block) then never exceeds the wanted count. M = n h w
CG_HD void cg_plan(long long M, int ci, int co, long long& block, int& blocks) {
  const long long tiles = (long long)((ci + CG_C_TILE - 1) / CG_C_TILE) * (co / CG_O_TILE);
  long long want = (CG_TARGET_GROUPS + tiles - 1) / tiles;
  if (want < 1) want = 1;
  if (want > CG_MAX_BLOCKS) want = CG_MAX_BLOCKS;
  long long b = (M + want - 1) / want;
  b = (b + CG_BLOCK_UNIT - 1) / CG_BLOCK_UNIT * CG_BLOCK_UNIT;
  block = b;
  blocks = (int)((M + b - 1) / b);
}

}  // namespace ctpn
