// cv2.resize(INTER_LINEAR) of a TABLE of uint8 BGR images of different sizes, each by its own factor, into outputs of different sizes
// (include/ctpn_hip.h, ctpn_write_annotated_files_ragged: the images of a ragged canvas back at their files' sizes): what
// resize_mixed.hip's kernel shares with the host, as __host__ __device__ text.
//   RmImage      one image of the call, as resize_linear_mixed_kernel reads it from device memory
//   rm_describe  an image's descriptor: source and destination geometry, its 1 / f
//   rm_prefix    the table's prefix sums: first work item of every image
//   rm_locate    work item -> (image, output row, segment): the last image whose first item is not behind it (jem_locate's search)
//   rm_quad      four consecutive output pixels of one row as the three dwords they are stored in
// A WORK ITEM is one workgroup (one wave) of the kernel: one output row by one segment of RM_SEG_PIXELS pixels. Image i has
// dh_i * rm_segments(dw_i) of them, segments fastest; no item belongs to two images. A thread owns four consecutive output pixels: 12
// bytes, three whole dwords. Destination rows are rm_pitch(dw) bytes apart -- a multiple of 12 that holds the last thread's four pixels
// --, so the pixels behind dw in a row are padding (zeros); the JPEG encoder takes pitches and never reads them.
// The arithmetic is resize_pixel.h's (rs_coord, rs_weights, rs_u8), called as resize_linear_kernel calls it: image i's output is
// launch_resize_linear's of that image alone, byte for byte. Every unit that includes this file is built with -ffp-contract=off.
// hipcc builds the kernel from this text; tests/resize_mixed_host.cpp compiles the same text with g++ under ASan + UBSan and drives it
// with loops over the work items and thread indices. Nothing here includes a HIP header.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "resize_pixel.h"

namespace ctpn {

struct RmImage {
  int h, w;                    // source size
  int dh, dw;                  // destination size: resize_out_dim of h and w by f
  long long src_off;           // byte offset of the source's first pixel in the source buffer
  long long src_pitch;         // bytes from one source row to the next (>= 3 w)
  long long dst_off;           // byte offset of the destination block in the destination buffer; a multiple of 4
  long long dst_pitch;         // bytes from one destination row to the next: rm_pitch(dw)
  double inv_f;                // 1 / f, as launch_resize_linear computes it from f
  long long item0;             // first work item of the image: prefix sum of rm_items
};

constexpr int RM_THREADS = 64;                         // one wave
constexpr int RM_SEG_PIXELS = 4 * RM_THREADS;
constexpr long long RM_MAX_ITEMS = 0x7fffffffLL;       // a one-dimensional grid holds no more workgroups

RS_HD int rm_segments(int dw) { return (dw + RM_SEG_PIXELS - 1) / RM_SEG_PIXELS; }
RS_HD long long rm_pitch(int dw) { return (long long)((dw + 3) / 4) * 12; }
RS_HD long long rm_items(const RmImage& d) { return (long long)d.dh * rm_segments(d.dw); }
RS_HD long long rm_block_bytes(const RmImage& d) { return (long long)d.dh * d.dst_pitch; }

// everything of a descriptor but the prefix sum
RS_HD void rm_describe(RmImage& d, int h, int w, int dh, int dw, long long src_off, long long src_pitch, long long dst_off, double inv_f) {
  d.h = h; d.w = w; d.dh = dh; d.dw = dw; d.src_off = src_off; d.src_pitch = src_pitch; d.dst_off = dst_off; d.dst_pitch = rm_pitch(dw);
  d.inv_f = inv_f; d.item0 = 0;
}

// item0 of every image. Returns the number of work items, or -1 above RM_MAX_ITEMS
RS_HD long long rm_prefix(RmImage* tab, int n) {
  long long items = 0;
  for (int i = 0; i < n; ++i) {
    tab[i].item0 = items;
    items += rm_items(tab[i]);
    if (items > RM_MAX_ITEMS) return -1;
  }
  return items;
}

struct RmItem { int img, row, seg; };

// item: 0 <= item < the table's total (the grid covers exactly that many). Every image has at least one item, so item0 rises strictly
RS_HD RmItem rm_locate(const RmImage* tab, int n, long long item) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].item0 <= item) lo = mid; else hi = mid - 1;
  }
  const int segs = rm_segments(tab[lo].dw), r = (int)(item - tab[lo].item0);
  RmItem p;
  p.img = lo; p.row = r / segs; p.seg = r - p.row * segs;
  return p;
}

// output pixels u0 .. u0 + 3 (u0 % 4 == 0, u0 < dw) of output row dy of image d, whose source begins at src: resize_linear_kernel's
// uint8 branch per pixel. Pixels from dw on are zeros
RS_HD void rm_quad(const uint8_t* src, const RmImage& d, int dy, int u0, uint32_t (&out)[3]) {
  int sy, b0, b1;
  float fy;
  rs_coord(dy, d.inv_f, d.h, 0, sy, fy);
  rs_weights(fy, b0, b1);
  const int y0 = sy < 0 ? 0 : (sy < d.h ? sy : d.h - 1);
  const int y1 = sy + 1 < 0 ? 0 : (sy + 1 < d.h ? sy + 1 : d.h - 1);
  const uint8_t* r0 = src + (long long)y0 * d.src_pitch;
  const uint8_t* r1 = src + (long long)y1 * d.src_pitch;
  uint32_t b[12];
  for (int k = 0; k < 4; ++k) {
    b[3 * k] = b[3 * k + 1] = b[3 * k + 2] = 0u;
    if (u0 + k >= d.dw) continue;
    int sx, a0, a1;
    float fx;
    rs_coord(u0 + k, d.inv_f, d.w, 1, sx, fx);
    rs_weights(fx, a0, a1);
    const int x1 = sx + 1 < d.w ? sx + 1 : d.w - 1;
    for (int c = 0; c < 3; ++c)
      b[3 * k + c] = (uint32_t)rs_u8((int)r0[sx * 3 + c], (int)r0[x1 * 3 + c], (int)r1[sx * 3 + c], (int)r1[x1 * 3 + c], a0, a1, b0, b1);
  }
  for (int q = 0; q < 3; ++q) out[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
}

// One thread of one work item: its three dwords into the image's own block, or nothing. dst: the destination buffer (4-byte aligned).
// The store is checked against the block: a thread whose twelve bytes do not lie inside [0, dh * dst_pitch) stores nothing.
RS_HD void rm_thread(const uint8_t* src, uint8_t* dst, const RmImage* tab, int n, long long item, int tid) {
  const RmItem p = rm_locate(tab, n, item);
  const RmImage& d = tab[p.img];
  const int u0 = (p.seg * RM_THREADS + tid) * 4;
  if (u0 >= d.dw || p.row >= d.dh) return;
  const long long at = (long long)p.row * d.dst_pitch + (long long)u0 * 3;
  if (at < 0 || at + 12 > rm_block_bytes(d)) return;
  uint32_t px[3];
  rm_quad(src + d.src_off, d, p.row, u0, px);
  uint32_t* o = reinterpret_cast<uint32_t*>(dst + d.dst_off + at);
  o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
}

}  // namespace ctpn
