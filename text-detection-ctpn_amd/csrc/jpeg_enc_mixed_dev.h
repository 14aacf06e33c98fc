// The JPEG writer's pixel half over a TABLE of images of different sizes and row pitches (include/ctpn_hip.h, ctpn_encode_jpeg_mixed,
// ctpn_write_line_crops): what jpeg_enc.hip's two forward-DCT kernels share with the host, as __host__ __device__ text.
//   JemImage      one image of the call, as jpeg_fdct_mixed_kernel reads it from device memory
//   jem_describe  an image's descriptor: the block grid jpeg_enc_geom gives an h x w image, its place in the source and in the coefficients
//   jem_prefix    the table's prefix sums: first work item and coefficient block of every image
//   jem_locate    work item -> (image, MCU row, tile): the last image whose first item is not behind it, a search over at most
//                 log2(n) + 1 entries (jr_block_locate's, jpeg_ragged_dev.h)
//   jenc_load4    the kernels' pixel read (both the uniform and the mixed one)
// A WORK ITEM is one workgroup of either kernel: one MCU row by one tile of 8 MCUs (16 x 128 pixels). Image i has
// jem_tiles(w_i) * bh[1] of them, tiles fastest; no item belongs to two images.
// hipcc builds the kernels from this text; tests/jpeg_enc_mixed_host.cpp compiles the same text with g++ under ASan + UBSan and drives it
// with loops over the work items and thread indices. Nothing here includes a HIP header.
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)      // a host compiler: jpeg_enc_pixel.h spells its qualifiers out
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#include "jpeg_enc_pixel.h"

namespace ctpn {

struct JemImage {
  int h, w;
  int bw[3], bh[3];            // blocks per row / column of every component over the MCU grid (4:2:0), as jpeg_enc_geom computes them
  long long pitch;             // bytes from one pixel row to the next (>= 3 w)
  long long src_off;           // byte offset of the first pixel in the source buffer
  long long coef_base;         // int16 offset of the image's coefficient block: prefix sum of the images' own coefficient counts
  long long coef_off[3];       // int16 offset of component c inside that block
  long long item0;             // first work item of the image: prefix sum of jem_items
};

constexpr long long JEM_MAX_ITEMS = 0x7fffffffLL;      // a one-dimensional grid holds no more workgroups

__host__ __device__ __forceinline__ int jem_tiles(int w) { return ((w + 15) / 16 + 7) / 8; }
__host__ __device__ __forceinline__ long long jem_items(const JemImage& d) { return (long long)jem_tiles(d.w) * d.bh[1]; }
__host__ __device__ __forceinline__ long long jem_coef_count(const JemImage& d) { return d.coef_off[2] + (long long)d.bw[2] * d.bh[2] * 64; }

// everything of a descriptor but the two prefix sums
__host__ __device__ __forceinline__ void jem_describe(JemImage& d, int h, int w, long long pitch, long long src_off) {
  d.h = h; d.w = w; d.pitch = pitch; d.src_off = src_off; d.coef_base = 0; d.item0 = 0;
  const int mcux = (w + 15) / 16, mcuy = (h + 15) / 16;
  long long co = 0;
  for (int c = 0; c < 3; ++c) {
    d.bw[c] = c ? mcux : 2 * mcux; d.bh[c] = c ? mcuy : 2 * mcuy;
    d.coef_off[c] = co;
    co += (long long)d.bw[c] * d.bh[c] * 64;
  }
}

// item0 and coef_base of every image; *coef_total: the call's coefficients. Returns the number of work items, or -1 above JEM_MAX_ITEMS
__host__ __device__ __forceinline__ long long jem_prefix(JemImage* tab, int n, long long* coef_total) {
  long long items = 0, coef = 0;
  for (int i = 0; i < n; ++i) {
    tab[i].item0 = items; tab[i].coef_base = coef;
    items += jem_items(tab[i]); coef += jem_coef_count(tab[i]);
    if (items > JEM_MAX_ITEMS) return -1;
  }
  if (coef_total) *coef_total = coef;
  return items;
}

struct JemItem { int img, my, tile; };

// item: 0 <= item < the table's total (the grid covers exactly that many). Every image has at least one item, so item0 rises strictly
__host__ __device__ __forceinline__ JemItem jem_locate(const JemImage* __restrict__ tab, int n, long long item) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].item0 <= item) lo = mid; else hi = mid - 1;
  }
  const int tiles = jem_tiles(tab[lo].w), r = (int)(item - tab[lo].item0);
  JemItem p;
  p.img = lo; p.my = r / tiles; p.tile = r - p.my * tiles;
  return p;
}

// Four pixels (B | G << 8 | R << 16) of row y of an image (first pixel at img, rows `pitch` bytes apart) from column x0 on, the last column
// repeated behind the image. A run inside the image is read as the aligned dwords that hold its 12 bytes: three where its address is a
// multiple of 4, else four -- the fourth ends up to THREE BYTES BEHIND THE RUN, and the first begins up to three bytes in front of it. Inside
// an image those bytes are its neighbours' (or the pitch's padding); around the last row's last run and the first row's first they are
// not the image's. So: a source whose rows start 4-byte aligned is never read outside its pixels (x0 is a multiple of 4, a run's offset
// one of 12) -- ctpn_write_line_crops' crops, tests/jpeg_enc_mixed_host.cpp under ASan --; any other device source must be readable over
// the aligned dwords its pixels touch, i.e. three bytes past its last pixel (staged host sources carry 256 bytes of slack; device
// allocations begin 256-byte aligned).
__host__ __device__ __forceinline__ void jenc_load4(const uint8_t* __restrict__ img, long long pitch, int y, int x0, int w, uint32_t (&px)[4]) {
  const uint8_t* row = img + (long long)y * pitch;
  if (x0 + 4 <= w) {
    const uintptr_t a = (uintptr_t)(row + (long long)x0 * 3);
    const uint32_t* p = (const uint32_t*)(a & ~(uintptr_t)3);
    const int sh = (int)(a & 3) * 8;
    uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
    if (sh) {      // (the fourth dword holds the run's last bytes)
      const uint32_t d3 = p[3];
      d0 = (d0 >> sh) | (d1 << (32 - sh)); d1 = (d1 >> sh) | (d2 << (32 - sh)); d2 = (d2 >> sh) | (d3 << (32 - sh));
    }
    px[0] = d0 & 0xffffffu; px[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8); px[2] = (d1 >> 16) | ((d2 & 0xffu) << 16); px[3] = d2 >> 8;
  } else {      // the run crosses the right edge: byte by byte
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int x = x0 + k;
      x = x < w ? x : w - 1;
      const uint8_t* q = row + (long long)x * 3;
      px[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    }
  }
}

}  // namespace ctpn
