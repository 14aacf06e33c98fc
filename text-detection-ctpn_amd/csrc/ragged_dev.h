// Ragged batches (images of one width and different heights in one canvas; definition: include/ctpn_hip.h, ctpn_forward_ragged): the index
// arithmetic and the per-thread bodies of ragged.hip's two kernels as __host__ __device__ functions. The kernels call them with their
// thread indices; tests/ragged_host.cpp compiles this same text with g++ under ASan + UBSan and calls them from loops over those indices.
// Nothing here includes a HIP header.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RG_HD __host__ __device__ __forceinline__
#else
#define RG_HD inline
#endif

namespace ctpn {

// valid rows of an image of `height` pixel rows at pooling level `level`: every 2x2/2 VALID pool drops an odd last row
RG_HD int ragged_valid_rows(int height, int level) { return height >> level; }

// One stored map of a canvas batch, as the mask kernel sees it: bytes only. A bordered activation buffer ((hl + 2) x (wl + 2) pixels per image,
// the interior at +1, +1) has top = 1, left_bytes = pixel bytes; the q-image (common.h) top = 2, left_bytes = 16. Split precision's [hi | lo]
// and rpn_conv/3x3's [hi | lo | hi] pixels are just wider pixels. Every byte count is even (the narrowest element is a 16-bit value).
struct RaggedMap {
  long long img_bytes;      // from one image's block to the next
  long long row_bytes;      // row pitch, frame included
  int top;                  // frame rows above interior row 0
  int left_bytes;           // frame bytes in front of an interior row's first pixel
  int span_bytes;           // an interior row's bytes: wl x pixel bytes
  int rows;                 // interior rows of the canvas at this level
  int level;                // pooling level of the map: image i keeps ragged_valid_rows(heights[i], level) rows
};

constexpr int RG_CHUNK = 16;                 // bytes one store clears
constexpr int RG_PER_WG = 4 * 256;           // chunks of ONE row a workgroup covers (four per thread, strided by the workgroup's size)

// 16-byte ALIGNED chunks that can touch a span of that many bytes, wherever it starts
RG_HD int ragged_chunks_per_row(int span_bytes) { return (span_bytes + RG_CHUNK - 1) / RG_CHUNK + 1; }
// workgroups per padded row, and for the rows [valid, rows) of one image: workgroup b clears chunks [RG_PER_WG (b % per_row), ...) of row
// valid + b / per_row (the only division is the workgroup's, on a uniform value)
RG_HD int ragged_wgs_per_row(int span_bytes) { return (ragged_chunks_per_row(span_bytes) + RG_PER_WG - 1) / RG_PER_WG; }
RG_HD long long ragged_mask_wgs(const RaggedMap& m, int valid) {
  return valid >= m.rows ? 0 : (long long)(m.rows - valid) * ragged_wgs_per_row(m.span_bytes);
}
// the bytes [lo, hi) of a span, counted from its first byte, that chunk k covers: the k-th aligned 16 bytes from the span's start rounded
// down (mis = the start's address mod 16), cut to the span; empty: lo >= hi
RG_HD void ragged_chunk(int mis, int span_bytes, int k, int& lo, int& hi) {
  const int c0 = RG_CHUNK * k - mis;
  lo = c0 < 0 ? 0 : c0;
  hi = c0 + RG_CHUNK < span_bytes ? c0 + RG_CHUNK : span_bytes;
}

struct alignas(16) RgVec16 { uint32_t v[4]; };

// chunk k of interior row `row` of image img. Whole chunks go out as one 16-byte store, a row's cut first and last chunk in 16-bit pieces.
// The frame is never written.
RG_HD void ragged_mask_thread(const RaggedMap& m, unsigned char* base, int img, int row, int k) {
  if (row >= m.rows || k >= ragged_chunks_per_row(m.span_bytes)) return;
  unsigned char* a = base + ((long long)img * m.img_bytes + (long long)(m.top + row) * m.row_bytes + m.left_bytes);
  int lo, hi;
  ragged_chunk((int)((uintptr_t)a & (RG_CHUNK - 1)), m.span_bytes, k, lo, hi);
  if (lo >= hi) return;
  if (hi - lo == RG_CHUNK) *(RgVec16*)(a + lo) = RgVec16{{0u, 0u, 0u, 0u}};
  else for (int p = lo; p < hi; p += 2) *(uint16_t*)(a + p) = (uint16_t)0;
}

// The net.data blob of a canvas (oracle/network.py image_blob: numpy's float32 -= float64, i.e. the difference in double, rounded once) with
// 0.0f below every image -- what SAME padding gives the image alone, AFTER the mean subtraction. Thread index t: the four consecutive floats
// 4 t .. 4 t + 3 of the flat n x hc x w x 3 blob (16-byte store; the batch's last thread may hold fewer).
RG_HD float ragged_blob_value(unsigned char p, int c) {
  const double mean = c == 0 ? 102.9801 : c == 1 ? 115.9465 : 122.7717;      // PIXEL_MEANS, BGR (reference lib/fast_rcnn/config.py:200)
  return (float)((double)p - mean);
}
RG_HD void ragged_blob_thread(const unsigned char* canvas, float* blob, const int* heights, int n, int hc, int w, long long t) {
  const long long total = (long long)n * hc * w * 3, e0 = 4 * t;
  if (e0 >= total) return;
  const long long row_elems = (long long)w * 3;
  long long grow;                                   // row of the whole canvas batch
  int img;
  if (total <= 0x7fffffffLL) {                      // (uniform: 32-bit divisions where the batch allows them, a tenth of the 64-bit ones' instructions)
    grow = (unsigned)e0 / (unsigned)row_elems;
    img = (int)((unsigned)grow / (unsigned)hc);
  } else {
    grow = e0 / row_elems;
    img = (int)(grow / hc);
  }
  int rem = (int)(e0 - grow * row_elems);           // element within the row
  int y = (int)(grow - (long long)img * hc), c = rem % 3;
  int height = heights[img];
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  const int cnt = total - e0 < 4 ? (int)(total - e0) : 4;
  for (int j = 0; j < cnt; ++j) {
    v[j] = y < height ? ragged_blob_value(canvas[e0 + j], c) : 0.0f;
    if (++c == 3) c = 0;
    if (++rem == row_elems) {
      rem = 0;
      if (++y == hc) { y = 0; ++img; if (img < n) height = heights[img]; }
    }
  }
  if (cnt == 4) { RgVec16 o; for (int j = 0; j < 4; ++j) o.v[j] = __builtin_bit_cast(uint32_t, v[j]); *(RgVec16*)(blob + e0) = o; }
  else for (int j = 0; j < cnt; ++j) blob[e0 + j] = v[j];
}

}  // namespace ctpn
