// Rectified crops of detected text lines, cut out of a batch that is already on the device: what a recogniser behind the detector reads,
// one image of fixed height per line. The arithmetic -- width, sample positions (double), the four-tap uint8 sample -- is crop_pixel.h's,
// pinned on the CPU from that very text (tests/test_crop.py); this unit holds the kernel around it and the host's descriptor table.
// Built with -ffp-contract=off (csrc/Makefile), like text_connector.cpp: the widths here and the positions in the kernel are double sums
// and products in a fixed order.
//   One workgroup = one line x CROP_COLS output columns; a thread owns four consecutive output pixels (12 bytes = three whole dwords: no
//   byte stores, and a wave's three stores fill 768 contiguous bytes of an output row) and walks the crop_h rows. A line's image is slot d.img of the
//   batch; over a ragged canvas (heights != null) the row axis clamps at that image's own last row (crop_pixel.h crop_image). The row tail behind Wc
//   and the padding up to max_w go through the same stores. The source taps are byte gathers along a near-horizontal line: neighbouring
//   lanes read neighbouring pixels of (at most a few) image rows. HBM-bound and small next to the network; its rate is unmeasured.
#include <cmath>

#include "common.h"
#include "crop_pixel.h"

namespace ctpn {

constexpr int CROP_THREADS = 64;                  // one wave: 256 output columns
constexpr int CROP_COLS = 4 * CROP_THREADS;

__global__ __launch_bounds__(CROP_THREADS) void crop_lines_kernel(const uint8_t* __restrict__ imgs, const CropDesc* __restrict__ descs, uint8_t* __restrict__ out,
                                                                  int slot_h, int w, const int* __restrict__ heights, int crop_h, int max_w, int pad, int chunks) {
  const CropDesc& d = descs[blockIdx.x / (unsigned)chunks];
  const int u0 = ((int)(blockIdx.x % (unsigned)chunks) * CROP_THREADS + (int)threadIdx.x) * 4;
  if (u0 >= max_w) return;                        // (max_w % 4 == 0: a thread's four columns are all inside a row, or none is)
  const int wc = d.wc;
  double q[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] = d.q[k];
  CropColumn cols[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) cols[k] = crop_column(q, u0 + k, wc);      // (those from wc on are not read)
  int h;
  const uint8_t* img = crop_image(imgs, d.img, slot_h, w, heights, h);      // (a ragged canvas: the image's own height)
  uint32_t* o = reinterpret_cast<uint32_t*>(out + d.out_off) + (size_t)u0 / 4 * 3;
  const size_t row_dwords = (size_t)max_w / 4 * 3;
  for (int v = 0; v < crop_h; ++v, o += row_dwords) {
    uint32_t px[3];
    crop_quad(img, h, w, cols, u0, wc, v, crop_h, pad, px);
    o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
  }
}

static_assert(sizeof(CropDesc) == CROP_DESC_BYTES, "common.h sizes the descriptor table");

int crop_line_width(const double* rec9, int crop_h, int max_w) { return crop_width(rec9, crop_h, max_w); }

void crop_fill_desc(const double* rec9, int img, int wc, size_t out_off, void* desc) {
  CropDesc& d = *static_cast<CropDesc*>(desc);
  for (int k = 0; k < 8; ++k) d.q[k] = rec9[k];
  d.img = img; d.wc = wc; d.out_off = out_off;
}

int launch_crop_lines(const uint8_t* imgs_dev, const void* descs_dev, int total, uint8_t* out_dev, int h, int w, const int* heights_dev, int crop_h, int max_w, int pad,
                      hipStream_t s) {
  if (total <= 0 || h <= 0 || w <= 0 || crop_h <= 0 || max_w < 4 || (max_w & 3) || ((uintptr_t)out_dev & 3)) return fail(CTPN_ERR_ARG, "crop_lines: bad geometry");
  const int chunks = (max_w + CROP_COLS - 1) / CROP_COLS;
  if ((long long)total * chunks > 0x7fffffffLL) return fail(CTPN_ERR_ARG, "crop_lines: too many lines for one launch");
  hipLaunchKernelGGL(crop_lines_kernel, dim3((unsigned)(total * chunks)), dim3(CROP_THREADS), 0, s, imgs_dev, (const CropDesc*)descs_dev, out_dev, h, w, heights_dev,
                     crop_h, max_w, pad, chunks);
  return launch_status("crop_lines");
}

}  // namespace ctpn
