// The pixel half of the JPEG decoder for files of mixed sizes, layouts and orientations in one call (ctpn_decode_jpeg_batch_ragged): the
// coefficients of every file, packed at per-file bases, become one ragged canvas n x hc x wc x 3 -- image i resized by its own factor in rows
// [0, height_i) of slot i, zeros below.
//   jpeg_idct_ragged_kernel          jpeg_idct_kernel (jpeg.hip) over a per-image descriptor table: a workgroup's 32 blocks each find their
//                                    image by a search of the block prefix, so a workgroup may straddle two images
//   jpeg_color_resize_ragged_kernel  jpeg_color_kernel + resize_linear_kernel (preprocess.hip) in one pass over the canvas: the plane gathers
//                                    of up to four neighbours per pixel replace the store and the re-read of the file-size BGR image
// Per-thread bodies: jpeg_ragged_dev.h, which the host test compiles too. Built with -ffp-contract=off (the resize's sample positions).
// Memory path: the planes are read through the vector L1 / L2 (neighbouring lanes read neighbouring plane bytes, up to 3 x 2 rows per
// pixel), the descriptor table (n <= a few dozen entries of 184 bytes) stays cache-resident; stores are three aligned dwords per lane,
// consecutive lanes consecutive addresses. No LDS beyond the IDCT's transpose buffer, no synchronisation between workgroups.
#include "common.h"
#include "jpeg_ragged_dev.h"

namespace ctpn {

__global__ __launch_bounds__(256) void jpeg_idct_ragged_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt /* [n][3][64] */,
                                                                uint8_t* __restrict__ planes, const JrImage* __restrict__ tab, int n, long long total_blocks) {
  __shared__ int ws[JR_BLOCKS_PER_WG][8][9];
  const int tid = threadIdx.x, lb = tid >> 3, t = tid & 7;
  const JrBlockPos p = jr_block_locate(tab, n, total_blocks, (long long)blockIdx.x * JR_BLOCKS_PER_WG + lb);
  int x[8], o[8];
  const int ac = jr_idct_load(tab, coef, qt, p, t, x);
  jidct_pass1(x, jidct_group8_or(ac), o);                               // (every lane shuffles, padding lanes with zero)
#pragma unroll
  for (int k = 0; k < 8; ++k) ws[lb][k][t] = o[k];                      // ws[row][col]
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = ws[lb][t][k];
  jr_idct_pass2(tab, planes, p, t, x);
}

__global__ __launch_bounds__(256) void jpeg_color_resize_ragged_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ canvas,
                                                                        const JrImage* __restrict__ tab, int n, int hc, int wc) {
  jr_color_resize_thread(planes, canvas, tab, n, hc, wc, (long long)blockIdx.x * 256 + threadIdx.x);
}

// coef_dev / planes_dev: the files' blocks at tab[i].coef_base / plane_base; qt_dev [n][3][64]; tab_dev: n descriptors in device memory;
// canvas_dev: n x hc x wc x 3 bytes, every one of them written
int launch_jpeg_pixels_ragged(const int16_t* coef_dev, const uint16_t* qt_dev, uint8_t* planes_dev, uint8_t* canvas_dev, const JrImage* tab_dev, int n,
                              long long total_blocks, int hc, int wc, hipStream_t s) {
  const long long wgs = (total_blocks + JR_BLOCKS_PER_WG - 1) / JR_BLOCKS_PER_WG;
  const long long groups = ((long long)n * hc * wc + 3) / 4, cwgs = (groups + 255) / 256;
  if (n <= 0 || hc <= 0 || wc <= 0 || total_blocks <= 0 || wgs > 0x7fffffffLL || cwgs > 0x7fffffffLL) return fail(CTPN_ERR_ARG, "jpeg_ragged: grid out of range");
  hipLaunchKernelGGL(jpeg_idct_ragged_kernel, dim3((unsigned)wgs), dim3(256), 0, s, coef_dev, qt_dev, planes_dev, tab_dev, n, total_blocks);
  hipLaunchKernelGGL(jpeg_color_resize_ragged_kernel, dim3((unsigned)cwgs), dim3(256), 0, s, (const uint8_t*)planes_dev, canvas_dev, tab_dev, n, hc, wc);
  return launch_status("jpeg_ragged");
}

}  // namespace ctpn
