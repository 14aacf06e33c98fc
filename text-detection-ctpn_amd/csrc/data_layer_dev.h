// The training data layer (include/ctpn_hip_data_layer.h: ctpn_split_labels, ctpn_train_page, ctpn_train_boxes): the per-thread text of
// data_layer.hip's kernels as host + device functions. tests/data_layer_host.cpp compiles this same text with g++ under ASan + UBSan
// (-ffp-contract=off, as the Makefile gives data_layer.hip) and walks whole label sets, pages and box lists the way the kernels do.
//   dl_scale         int(v / file * resized): one IEEE double division, one multiplication, truncated towards zero (split_label.py:40-47)
//   dl_sort4         a quad's four points by x, stably (np.argsort of four values: an insertion sort)
//   dl_span          pt1 .. pt4, then xmin, xmax, ymin, ymax clamped to the resized page (split_label.py:53-79)
//   dl_quad_span     the three above for one label line on its page
//   dl_strip_count   how many 16-px strips split_label.py:85-104 writes for (xmin, xmax) -- its quirks are listed at ctpn_split_labels
//   dl_strip         the k-th of them
//   dl_upper         the row of an offsets table an element falls in
//   dl_page_group    16 consecutive bytes of a training page: ctpn_resize's sample (resize_pixel.h), the row mirrored AFTER the resize
//   dl_blob          (double)pixel - PIXEL_MEANS[c], rounded once to float32
//   dl_box           one gt box: the uint16 flip of imdb.append_flipped_images, wrap and clamp included, then x scale in double
// Nothing here includes a HIP header.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "resize_pixel.h"

#if defined(__HIPCC__)
#define DL_HD __host__ __device__ inline
#else
#define DL_HD inline
#endif

namespace ctpn {

constexpr int DL_GROUP = 16;      // bytes of image_out a thread writes: one 16-byte store

// |v / file * resized| beyond this, or a NaN, saturates (Python's int() would raise or return a bignum): far outside any page either way
constexpr double DL_COORD_LIMIT = 1073741824.0;

DL_HD int dl_scale(double v, int file, int resized) {
  double t = v / (double)file;
  t = t * (double)resized;
  if (!(t > -DL_COORD_LIMIT)) t = -DL_COORD_LIMIT;
  if (t > DL_COORD_LIMIT) t = DL_COORD_LIMIT;
  return (int)t;
}

DL_HD void dl_sort4(int x[4], int y[4]) {
  for (int i = 1; i < 4; ++i) {
    const int vx = x[i], vy = y[i];
    int j = i;
    for (; j > 0 && x[j - 1] > vx; --j) { x[j] = x[j - 1]; y[j] = y[j - 1]; }
    x[j] = vx; y[j] = vy;
  }
}

struct DlSpan { int xmin, xmax, ymin, ymax; };

// x, y: sorted by x. The left pair gives pt1 (upper) and pt3 (lower), the right pair pt2 (upper) and pt4 (lower)
DL_HD DlSpan dl_span(const int x[4], const int y[4], int rh, int rw) {
  const int i1 = y[0] < y[1] ? 0 : 1, i3 = 1 - i1;
  const int i2 = y[2] < y[3] ? 2 : 3, i4 = 5 - i2;
  DlSpan s;
  s.xmin = x[i1] < x[i2] ? x[i1] : x[i2];
  s.ymin = y[i1] < y[i2] ? y[i1] : y[i2];
  s.xmax = x[i2] > x[i4] ? x[i2] : x[i4];
  s.ymax = y[i3] > y[i4] ? y[i3] : y[i4];
  if (s.xmin < 0) s.xmin = 0;
  if (s.xmax > rw - 1) s.xmax = rw - 1;
  if (s.ymin < 0) s.ymin = 0;
  if (s.ymax > rh - 1) s.ymax = rh - 1;
  return s;
}

// q8: x1, y1, .. x4, y4 of a label line; dims4: file h, file w, resized h, resized w
DL_HD DlSpan dl_quad_span(const double* q8, const int* dims4) {
  int x[4], y[4];
  for (int k = 0; k < 4; ++k) {
    x[k] = dl_scale(q8[2 * k], dims4[1], dims4[3]);
    y[k] = dl_scale(q8[2 * k + 1], dims4[0], dims4[2]);
  }
  dl_sort4(x, y);
  return dl_span(x, y, dims4[2], dims4[3]);
}

// the first multiple of 16 above xmin (xmin >= 0 after the clamp), and how many multiples of 16 lie strictly between xmin and xmax
DL_HD int dl_strip_start(int xmin) { return xmin - xmin % 16 + 16; }
DL_HD int dl_strip_inner(int xmin, int xmax) {
  const int start = dl_strip_start(xmin);
  return start < xmax ? (xmax - 1 - start) / 16 + 1 : 0;
}

DL_HD int dl_strip_count(int xmin, int xmax) {
  if (xmin == xmax) return 0;                    // the reference stops here (np.delete out of bounds): no strip
  const int inner = dl_strip_inner(xmin, xmax), drop = xmin % 16 == 15;      // drop: the first strip has x_left == x_right and is deleted
  return (inner == 0 ? 1 : inner + 1) - drop;
}

// k in 0 .. dl_strip_count - 1, left to right
DL_HD void dl_strip(int xmin, int xmax, int k, int& x1, int& x2) {
  const int start = dl_strip_start(xmin), inner = dl_strip_inner(xmin, xmax);
  const int j = k + (xmin % 16 == 15);
  if (j == 0) { x1 = xmin; x2 = start - 1; return; }      // with inner == 0 this is the only strip, and it ignores xmax
  x1 = start + 16 * (j - 1);
  x2 = j == inner ? xmax : x1 + 15;
}

// offs: n + 1 ascending ints from 0; e < offs[n] -> the row r with offs[r] <= e < offs[r + 1] (empty rows are stepped over)
DL_HD int dl_upper(const int* offs, int n, int e) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (offs[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

struct DlPage {
  int h, w;             // the source page
  long long pitch;      // bytes between its rows
  int oh, ow;           // the output: resize_out_dim of h and w by the factor
  int resize;           // 0: factor <= 0 or 1, the pixel is the source pixel
  int flip;             // 1: output column dx holds the resized page's column ow - 1 - dx
  double inv_f;         // 1 / factor, as launch_resize_linear forms it
};

DL_HD size_t dl_page_bytes(const DlPage& p) { return (size_t)p.oh * p.ow * 3; }
DL_HD size_t dl_page_groups(const DlPage& p) { return (dl_page_bytes(p) + DL_GROUP - 1) / DL_GROUP; }

// bytes [16 g, 16 g + count) of image_out -> v; count is 16 except in the last group
DL_HD int dl_page_group(const uint8_t* src, const DlPage& p, size_t g, uint8_t v[DL_GROUP]) {
  const size_t total = dl_page_bytes(p), b0 = g * DL_GROUP;
  const int count = (int)(total - b0 < (size_t)DL_GROUP ? total - b0 : (size_t)DL_GROUP);
  size_t pix = b0 / 3;
  int c = (int)(b0 - pix * 3);
  int dy = (int)(pix / (size_t)p.ow), dx = (int)(pix - (size_t)dy * p.ow);
  bool fresh = true;
  const uint8_t *r0 = nullptr, *r1 = nullptr;
  int sx = 0, x1 = 0, a0 = 0, a1 = 0, b0w = 0, b1w = 0;
  for (int k = 0; k < count; ++k) {
    if (fresh) {
      const int rx = p.flip ? p.ow - 1 - dx : dx;      // the resized page's column this output column shows
      if (p.resize) {
        int sy;
        float fx, fy;
        rs_coord(rx, p.inv_f, p.w, 1, sx, fx);
        rs_coord(dy, p.inv_f, p.h, 0, sy, fy);
        x1 = sx + 1 < p.w ? sx + 1 : p.w - 1;
        const int y0 = sy < 0 ? 0 : (sy < p.h ? sy : p.h - 1);
        const int y1 = sy + 1 < 0 ? 0 : (sy + 1 < p.h ? sy + 1 : p.h - 1);
        r0 = src + (long long)y0 * p.pitch;
        r1 = src + (long long)y1 * p.pitch;
        rs_weights(fx, a0, a1);
        rs_weights(fy, b0w, b1w);
      } else {
        sx = rx;
        r0 = src + (long long)dy * p.pitch;
      }
      fresh = false;
    }
    v[k] = p.resize ? (uint8_t)rs_u8((int)r0[sx * 3 + c], (int)r0[x1 * 3 + c], (int)r1[sx * 3 + c], (int)r1[x1 * 3 + c], a0, a1, b0w, b1w) : r0[sx * 3 + c];
    if (++c == 3) {
      c = 0;
      fresh = true;
      if (++dx == p.ow) { dx = 0; ++dy; }
    }
  }
  return count;
}

// c: the channel of flat byte index b, b % 3. PIXEL_MEANS, BGR (reference lib/fast_rcnn/config.py:200)
DL_HD float dl_blob(uint8_t v, int c) {
  const double mean = c == 0 ? 102.9801 : c == 1 ? 115.9465 : 122.7717;
  return (float)((double)v - mean);
}

// s4: a strip x1, y1, x2, y2 -> out5; false (out5 untouched) where a value lies outside 0 .. 65535: pascal_voc.py:134 holds boxes as uint16
DL_HD bool dl_box(const float* s4, int page_width, int flip, double scale, float out5[5]) {
  uint16_t b[4];
  for (int k = 0; k < 4; ++k) {
    if (!(s4[k] >= 0.f && s4[k] <= 65535.f)) return false;
    b[k] = (uint16_t)s4[k];
  }
  if (flip) {
    const uint16_t W = (uint16_t)page_width, ox1 = b[0], ox2 = b[2];
    b[0] = (uint16_t)((uint16_t)(W - ox2) - 1u);      // uint16 arithmetic: it wraps where x2 >= W
    b[2] = (uint16_t)((uint16_t)(W - ox1) - 1u);
    if (b[2] < b[0]) b[0] = 0;
  }
  for (int k = 0; k < 4; ++k) out5[k] = (float)((double)b[k] * scale);
  out5[4] = 1.f;
  return true;
}

}  // namespace ctpn
