// JPEG files of mixed sizes into one ragged canvas (include/ctpn_hip.h, ctpn_decode_jpeg_batch_ragged): the per-thread text of
// jpeg_ragged.hip's two kernels as __host__ __device__ functions. The kernels call them with their thread indices;
// tests/jpeg_ragged_host.cpp compiles this same text with g++ under ASan + UBSan and calls them from loops over those indices.
//   IDCT            jpeg_idct_kernel's two passes (jpeg_pixel.h: jidct_load + jidct_pass1 by column, the block's zero-rows flag in between, the caller's transpose, jidct_pass2 by row with the
//                   clamp and one 8-byte store) with the image found per 8 x 8 block from a descriptor table instead of one JpegGeom for
//                   the batch. The kernel's barrier (the host's loop over a workgroup's threads) stands between the passes.
//   colour + resize jpeg_color_kernel followed by resize_linear_kernel (preprocess.hip) in one pass over the CANVAS: every canvas pixel is
//                   zero below its image, jpeg_pixel at jpeg_orient of itself where the factor is 1, and otherwise the resize's uint8 formula
//                   over four neighbours that are jpeg_pixel values -- the file-size BGR image the uniform path stores between its two
//                   kernels is never stored. Same functions, same order: the bytes are the uniform path's.
// Nothing here includes a HIP header; the unit that builds the kernels is compiled with -ffp-contract=off (resize_pixel.h).
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)      // a host compiler: jpeg_pixel.h spells its qualifiers out
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#include "jpeg_pixel.h"
#include "resize_pixel.h"

namespace ctpn {

// one image of the call, as both kernels read it from device memory
struct JrImage {
  JpegGeom g;               // plane_off / coef_off: inside the image's own plane / coefficient block
  long long coef_base;      // int16 offset of the image's coefficient block (prefix sum of the files' own capacities)
  long long plane_base;     // byte offset of its plane block (packed the same way: one byte per coefficient)
  long long block0;         // first global 8 x 8 block of the image: prefix sum of g.blocks_per_img
  double inv_f;             // 1 / factor, as launch_resize_linear passes it (unused where resize == 0)
  int resize;               // 0: the factor is 1, the canvas pixel is the decoded pixel
  int height;               // rows of the canvas slot the image fills; the rows below are zero
};

constexpr int JR_BLOCKS_PER_WG = 32;      // 8 threads per 8 x 8 block, 256 per workgroup (jpeg_idct_kernel's shape)

struct JrBlockPos { int live, img, c, by, bx; long long b; };      // b: the block's index inside its component

// global block gb -> image (the last one whose block0 <= gb: a search over at most log2(n) + 1 entries), component, block row and column
RS_HD JrBlockPos jr_block_locate(const JrImage* __restrict__ tab, int n, long long total_blocks, long long gb) {
  JrBlockPos p = {0, 0, 0, 0, 0, 0};
  if (gb >= total_blocks) return p;      // a padding lane: it stays alive through the barrier and loads / stores nothing
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].block0 <= gb) lo = mid; else hi = mid - 1;
  }
  const JpegGeom& g = tab[lo].g;
  long long b = gb - tab[lo].block0;
  int c = 0;
  while (c + 1 < g.ncomp && b >= (long long)g.bw[c] * g.bh[c]) { b -= (long long)g.bw[c] * g.bh[c]; ++c; }
  p.live = 1; p.img = lo; p.c = c; p.b = b;
  p.by = (int)(b / g.bw[c]); p.bx = (int)(b - (long long)p.by * g.bw[c]);
  return p;
}

// the two passes (jpeg_pixel.h) on the block jr_block_locate found. A padding lane reads no descriptor and hands the pass null pointers,
// which a lane that is not live never dereferences
// (load: the dequantised column and the OR of its raw rows 1 .. 7; the caller ORs the block's eight and runs jidct_pass1)
RS_HD int jr_idct_load(const JrImage* __restrict__ tab, const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt /* [n][3][64] */,
                       const JrBlockPos& p, int t, int (&x)[8]) {
  const int16_t* blk = nullptr;
  if (p.live) { const JrImage& d = tab[p.img]; blk = coef + d.coef_base + d.g.coef_off[p.c] + p.b * 64; }
  return jidct_load(blk, qt + ((long long)p.img * 3 + p.c) * 64, p.live != 0, t, x);
}

// (pass 1 in one call, the flag read from the block itself: jpeg_pixel.h's form for a caller that runs the columns one after the other)
RS_HD void jr_idct_pass1(const JrImage* __restrict__ tab, const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt /* [n][3][64] */,
                         const JrBlockPos& p, int t, int (&o)[8]) {
  const int16_t* blk = nullptr;
  if (p.live) { const JrImage& d = tab[p.img]; blk = coef + d.coef_base + d.g.coef_off[p.c] + p.b * 64; }
  jidct_pass1(blk, qt + ((long long)p.img * 3 + p.c) * 64, p.live != 0, t, o);
}

RS_HD void jr_idct_pass2(const JrImage* __restrict__ tab, uint8_t* __restrict__ planes, const JrBlockPos& p, int t, const int (&x)[8]) {
  uint8_t* dst = nullptr;
  if (p.live) { const JrImage& d = tab[p.img]; dst = planes + d.plane_base + d.g.plane_off[p.c] + ((long long)(p.by * 8 + t) * (d.g.bw[p.c] * 8) + p.bx * 8); }
  jidct_pass2(dst, p.live != 0, x);
}

// pixel (y, x) of the TURNED image (what cv2.imread returns): B | G << 8 | R << 16
RS_HD uint32_t jr_turned_pixel(const uint8_t* __restrict__ P, const JpegGeom& g, int y, int x) {
  int sy, sx;
  jpeg_orient(g.orient, g.h, g.w, y, x, sy, sx);
  return jpeg_pixel(P, g, sy, sx);
}

// Thread index grp: the four consecutive pixels 4 grp .. 4 grp + 3 of the canvas's linear order (n x hc x wc), stored as three aligned
// dwords; the batch's last thread may hold fewer and stores them byte by byte. wc need not be a multiple of 4: every pixel steps its own
// coordinates, and a group may straddle a row or an image. Nothing is written at or behind n x hc x wc x 3 bytes.
RS_HD void jr_color_resize_thread(const uint8_t* __restrict__ planes, uint8_t* __restrict__ canvas, const JrImage* __restrict__ tab, int n, int hc, int wc,
                                  long long grp) {
  const long long per = (long long)hc * wc, total = per * n;
  const long long p0 = grp * 4;
  if (p0 >= total) return;
  int img, dy, dx;
  if (total <= 0x7fffffffLL) {      // (uniform: 32-bit divisions where the batch allows them)
    img = (int)((unsigned)p0 / (unsigned)per);
    const unsigned rem = (unsigned)p0 - (unsigned)img * (unsigned)per;
    dy = (int)(rem / (unsigned)wc); dx = (int)(rem - (unsigned)dy * (unsigned)wc);
  } else {
    img = (int)(p0 / per);
    const long long rem = p0 - (long long)img * per;
    dy = (int)(rem / wc); dx = (int)(rem - (long long)dy * wc);
  }
  uint32_t px[4] = {0, 0, 0, 0};
  int y0 = 0, y1 = 0, b0 = 0, b1 = 0;
  bool row_known = false;           // (y0, y1, b0, b1) belong to the current (img, dy)
  int cx0 = -1, cx1 = -1;           // the previous pixel's two source columns in this row (-1: none) ...
  uint32_t ct0 = 0, cb0 = 0, ct1 = 0, cb1 = 0;      // ... and their pixels in rows y0 (t) and y1 (b)
  for (int k = 0; k < 4; ++k) {
    if (p0 + k < total && dy < tab[img].height) {
      const JrImage& d = tab[img];
      const JpegGeom& g = d.g;
      const uint8_t* P = planes + d.plane_base;
      if (!d.resize) px[k] = jr_turned_pixel(P, g, dy, dx);
      else {
        int sx, sy, a0, a1;
        float fx, fy;
        if (!row_known) {
          rs_coord(dy, d.inv_f, g.oh, 0, sy, fy);
          y0 = sy < 0 ? 0 : (sy < g.oh ? sy : g.oh - 1);
          y1 = sy + 1 < 0 ? 0 : (sy + 1 < g.oh ? sy + 1 : g.oh - 1);
          rs_weights(fy, b0, b1);
          row_known = true;
        }
        rs_coord(dx, d.inv_f, g.ow, 1, sx, fx);
        const int x1 = sx + 1 < g.ow ? sx + 1 : g.ow - 1;
        rs_weights(fx, a0, a1);
        // the two source columns, each as its pixels in rows y0 and y1: taken from the previous pixel of this row where it had them (an
        // upscale repeats them; a downscale by less than 2 shares one every other pixel), converted from the planes otherwise
        uint32_t p00, p10, p01, p11;
        if (sx == cx0) { p00 = ct0; p10 = cb0; }
        else if (sx == cx1) { p00 = ct1; p10 = cb1; }
        else { p00 = jr_turned_pixel(P, g, y0, sx); p10 = jr_turned_pixel(P, g, y1, sx); }
        if (x1 == sx) { p01 = p00; p11 = p10; }
        else if (x1 == cx1) { p01 = ct1; p11 = cb1; }
        else { p01 = jr_turned_pixel(P, g, y0, x1); p11 = jr_turned_pixel(P, g, y1, x1); }
        cx0 = sx; ct0 = p00; cb0 = p10;
        cx1 = x1; ct1 = p01; cb1 = p11;
        uint32_t v = 0;
        for (int c = 0; c < 3; ++c)
          v |= (uint32_t)rs_u8((int)((p00 >> (8 * c)) & 255u), (int)((p01 >> (8 * c)) & 255u), (int)((p10 >> (8 * c)) & 255u), (int)((p11 >> (8 * c)) & 255u),
                               a0, a1, b0, b1) << (8 * c);
        px[k] = v;
      }
    }
    if (++dx == wc) {
      dx = 0; row_known = false; cx0 = cx1 = -1;
      if (++dy == hc) { dy = 0; if (img + 1 < n) ++img; }      // (behind the last image nothing more is computed: p0 + k >= total)
    }
  }
  jpeg_store4(canvas, p0, total, px);
}

}  // namespace ctpn
