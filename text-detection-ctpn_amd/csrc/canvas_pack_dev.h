// BGR uint8 images of mixed sizes into one ragged canvas (include/ctpn_hip.h, ctpn_pack_canvas): the per-thread text of canvas_pack.hip's
// kernel as __host__ __device__ functions. The kernel calls cp_thread with its thread index; tests/canvas_pack_host.cpp compiles this same
// text with g++ under ASan + UBSan and calls it from a loop over those indices.
//   CpImage      one image of the call, as canvas_pack_kernel reads it from device memory
//   cp_describe  an image's descriptor: where its pixels lie, its size, its 1 / f, the rows of its slot it fills
//   cp_pixel     one source pixel, read byte by byte: no alignment of the source or of its pitch is assumed
//   cp_store4    four canvas pixels as three aligned dwords, or byte by byte at the canvas's end; nothing at or behind its last byte
//   cp_thread    four consecutive pixels of the canvas's linear order, each finding its own (slot, row, column)
// The canvas is n x hc x wc x 3 at pitch 3 wc, wc any value. Slot i holds image i resized by its own factor in rows [0, dh_i) and ZEROS in
// rows [dh_i, hc): the kernel writes every byte of the canvas and reads none of it, so what the buffer held before does not matter.
// The thread mapping is jr_color_resize_thread's (jpeg_ragged_dev.h): one division pair per THREAD where the batch has fewer than 2^31 pixels
// (32-bit, uniform choice), after which the four pixels step their coordinates; the stores of a wave are 768 consecutive bytes. The
// arithmetic is resize_pixel.h's (rs_coord, rs_weights, rs_u8), called as rm_quad (resize_mixed_dev.h) and resize_linear_kernel call it, and
// at f <= 0 or f == 1 the pixel is the source pixel, as where the uniform path skips its resize: slot i's rows are launch_resize_linear's of
// image i alone, byte for byte. Every unit that includes this file for its kernel is built with -ffp-contract=off.
// Nothing here includes a HIP header.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "resize_pixel.h"

namespace ctpn {

struct CpImage {
  long long src_off;           // byte offset of the image's first pixel from the call's source base
  long long src_pitch;         // bytes from one source row to the next (>= 3 w)
  double inv_f;                // 1 / f, as launch_resize_linear computes it from f (unused where resize == 0)
  int h, w;                    // source size
  int dh;                      // rows of the canvas slot the image fills (16 .. hc); the rows below are zero
  int resize;                  // 0: f <= 0 or f == 1, the canvas pixel is the source pixel
};

constexpr int CP_THREADS = 256;

RS_HD void cp_describe(CpImage& d, long long src_off, long long src_pitch, int h, int w, double f, int dh) {
  d.src_off = src_off; d.src_pitch = src_pitch; d.h = h; d.w = w; d.dh = dh;
  d.resize = (f > 0.0 && f != 1.0) ? 1 : 0;
  d.inv_f = d.resize ? 1.0 / f : 1.0;
}

// threads the canvas takes: one per four pixels, the last one possibly fewer
RS_HD long long cp_groups(int n, int hc, int wc) { return ((long long)n * hc * wc + 3) / 4; }

// pixel (y, x) of image d, 0 <= y < h and 0 <= x < w: B | G << 8 | R << 16
RS_HD uint32_t cp_pixel(const uint8_t* img, const CpImage& d, int y, int x) {
  const uint8_t* p = img + (long long)y * d.src_pitch + (long long)x * 3;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// the four pixels p0 .. p0 + 3 (p0 a multiple of 4, canvas 4-byte aligned) of a canvas of `total` pixels
RS_HD void cp_store4(uint8_t* canvas, long long p0, long long total, const uint32_t (&px)[4]) {
  if (p0 < 0 || p0 >= total) return;
  if (p0 + 4 <= total) {
    uint32_t* o = reinterpret_cast<uint32_t*>(canvas + p0 * 3);
    o[0] = px[0] | (px[1] << 24);
    o[1] = (px[1] >> 8) | (px[2] << 16);
    o[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
    uint8_t* ob = canvas + p0 * 3;
    const int left = (int)(total - p0);      // 1 .. 3
    for (int k = 0; k < left; ++k) { ob[3 * k] = (uint8_t)px[k]; ob[3 * k + 1] = (uint8_t)(px[k] >> 8); ob[3 * k + 2] = (uint8_t)(px[k] >> 16); }
  }
}

// Thread index grp: canvas pixels 4 grp .. 4 grp + 3. src: the call's source base (image i at src + tab[i].src_off).
RS_HD void cp_thread(const uint8_t* src, uint8_t* canvas, const CpImage* tab, int n, int hc, int wc, long long grp) {
  const long long per = (long long)hc * wc, total = per * n;
  const long long p0 = grp * 4;
  if (grp < 0 || p0 >= total) return;
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
    if (p0 + k < total && dy < tab[img].dh) {
      const CpImage& d = tab[img];
      const uint8_t* P = src + d.src_off;
      if (!d.resize) { if (dy < d.h && dx < d.w) px[k] = cp_pixel(P, d, dy, dx); }
      else {
        int sx, sy, a0, a1;
        float fx, fy;
        if (!row_known) {
          rs_coord(dy, d.inv_f, d.h, 0, sy, fy);
          y0 = sy < 0 ? 0 : (sy < d.h ? sy : d.h - 1);
          y1 = sy + 1 < 0 ? 0 : (sy + 1 < d.h ? sy + 1 : d.h - 1);
          rs_weights(fy, b0, b1);
          row_known = true;
        }
        rs_coord(dx, d.inv_f, d.w, 1, sx, fx);
        const int x1 = sx + 1 < d.w ? sx + 1 : d.w - 1;
        rs_weights(fx, a0, a1);
        // the two source columns, each as its pixels in rows y0 and y1: taken from the previous pixel of this row where it had them (an
        // upscale repeats them; a downscale by less than 2 shares one every other pixel), loaded otherwise
        uint32_t p00, p10, p01, p11;
        if (sx == cx0) { p00 = ct0; p10 = cb0; }
        else if (sx == cx1) { p00 = ct1; p10 = cb1; }
        else { p00 = cp_pixel(P, d, y0, sx); p10 = cp_pixel(P, d, y1, sx); }
        if (x1 == sx) { p01 = p00; p11 = p10; }
        else if (x1 == cx1) { p01 = ct1; p11 = cb1; }
        else { p01 = cp_pixel(P, d, y0, x1); p11 = cp_pixel(P, d, y1, x1); }
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
  cp_store4(canvas, p0, total, px);
}

}  // namespace ctpn
