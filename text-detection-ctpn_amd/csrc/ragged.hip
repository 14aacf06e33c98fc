// Ragged batches: images of one width and different heights in one canvas (definition: include/ctpn_hip.h, ctpn_forward_ragged).
//   ragged_mask_kernel   clears the interior rows below every image of one stored map, between two layers of the forward: to the image above
//                        them, cleared rows are the zero padding it would have had alone
//   ragged_blob_kernel   uint8 canvas -> the float feed of fp32 / split precision with 0.0f below every image (a uint8 pixel cannot say
//                        "equal to PIXEL_MEANS")
// Both are plain HBM writers: per-thread bodies and index arithmetic in ragged_dev.h, which the host test compiles too.
#include "common.h"
#include "ragged_dev.h"

namespace ctpn {

// grid (x: the workgroups of the tallest padding among the images, RG_PER_WG chunks of one row each; y: image). heights: the batch's pixel
// heights on the device. A workgroup whose row lies behind its image's padding returns at once: an image as tall as the canvas costs its
// workgroups' dispatch only. Stores: 16 bytes per lane, consecutive lanes consecutive chunks; four chunks per thread, strided by the
// workgroup's size.
__global__ __launch_bounds__(256) void ragged_mask_kernel(unsigned char* __restrict__ base, RaggedMap m, const int* __restrict__ heights) {
  const int img = blockIdx.y;
  const int valid = ragged_valid_rows(heights[img], m.level);
  if ((long long)blockIdx.x >= ragged_mask_wgs(m, valid)) return;
  const int per_row = ragged_wgs_per_row(m.span_bytes);
  const int row = valid + (int)(blockIdx.x / (unsigned)per_row), k0 = (int)(blockIdx.x % (unsigned)per_row) * RG_PER_WG;
#pragma unroll
  for (int j = 0; j < RG_PER_WG / 256; ++j) ragged_mask_thread(m, base, img, row, k0 + j * 256 + (int)threadIdx.x);
}

__global__ __launch_bounds__(256) void ragged_blob_kernel(const unsigned char* __restrict__ canvas, float* __restrict__ blob,
                                                          const int* __restrict__ heights, int n, int hc, int w) {
  ragged_blob_thread(canvas, blob, heights, n, hc, w, (long long)blockIdx.x * 256 + threadIdx.x);
}

// max_pad_rows: the most rows any image of the batch lacks at the map's level (the host knows the heights); 0: nothing to launch
int launch_ragged_mask(void* base, const RaggedMap& m, const int* heights_dev, int n, int max_pad_rows, hipStream_t s) {
  if (max_pad_rows <= 0) return CTPN_OK;
  if (max_pad_rows > m.rows || m.span_bytes <= 0 || ((m.span_bytes | m.left_bytes) & 1) || ((m.row_bytes | m.img_bytes) & 1) || ((uintptr_t)base & 1))
    return fail(CTPN_ERR_ARG, "ragged_mask: bad map");
  const long long gx = (long long)max_pad_rows * ragged_wgs_per_row(m.span_bytes);
  if (gx > 0x7fffffffLL || n > 65535) return fail(CTPN_ERR_ARG, "ragged_mask: grid out of range");
  hipLaunchKernelGGL(ragged_mask_kernel, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, s, (unsigned char*)base, m, heights_dev);
  return launch_status("ragged_mask");
}

int launch_ragged_blob(const uint8_t* canvas, float* blob, const int* heights_dev, int n, int hc, int w, hipStream_t s) {
  const long long threads = ((long long)n * hc * w * 3 + 3) / 4;
  const long long gx = (threads + 255) / 256;
  if (gx <= 0 || gx > 0x7fffffffLL) return fail(CTPN_ERR_ARG, "ragged_blob: grid out of range");
  hipLaunchKernelGGL(ragged_blob_kernel, dim3((unsigned)gx), dim3(256), 0, s, canvas, blob, heights_dev, n, hc, w);
  return launch_status("ragged_blob");
}

}  // namespace ctpn

extern "C" int ctpn_ragged_valid_rows(int height, int level) {
  if (height < 0 || level < 0 || level > 4) return -1;
  return ctpn::ragged_valid_rows(height, level);
}
