// TEST INFRASTRUCTURE (never part of the product library): the text-line crops' per-sample source text -- csrc/crop_pixel.h, the functions
// crop_lines_kernel is made of -- compiled for the host with the HIP qualifiers defined away and driven the way the kernel drives it: per
// line one "thread" for every four output columns up to max_w, which computes its four columns once, walks the crop_h rows and stores three
// dwords per row (the row tail behind Wc and the padding included). tests/test_crop.py builds this file with g++ -ffp-contract=off and
// compares it with a numpy restatement of the definition, so the arithmetic is pinned on the CPU from the very text hipcc compiles.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../text-detection-ctpn_amd/csrc/crop_pixel.h"

#include <string.h>

extern "C" int crop_width_host(const double* rec9, int crop_h, int max_w) { return ctpn::crop_width(rec9, crop_h, max_w); }

// img: h x w x 3; recs: lines x 9; widths: lines; out: lines x crop_h x max_w x 3 (max_w % 4 == 0)
extern "C" int crop_lines_host(const uint8_t* img, int h, int w, const double* recs, const int* widths, int lines, int crop_h, int max_w, int pad, uint8_t* out) {
  using namespace ctpn;
  if (max_w < 4 || (max_w & 3)) return -1;
  for (int l = 0; l < lines; ++l) {
    CropDesc d;
    for (int k = 0; k < 8; ++k) d.q[k] = recs[9 * l + k];
    d.img = 0; d.wc = widths[l]; d.out_off = (unsigned long long)l * crop_h * max_w * 3;
    for (int u0 = 0; u0 < max_w; u0 += 4) {                      // one thread
      CropColumn cols[4];
      for (int k = 0; k < 4; ++k) cols[k] = crop_column(d.q, u0 + k, d.wc);
      for (int v = 0; v < crop_h; ++v) {
        uint32_t px[3];
        crop_quad(img, h, w, cols, u0, d.wc, v, crop_h, pad, px);
        memcpy(out + d.out_off + ((size_t)v * max_w + u0) * 3, px, 12);      // (little-endian, like the device)
      }
    }
  }
  return 0;
}
