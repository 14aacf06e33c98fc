// BGR uint8 images of mixed sizes, each resized by its own factor, into one ragged canvas n x hc x wc x 3 in ONE launch (ctpn_pack_canvas,
// ctpn_decode_png_files_ragged: api_canvas_pack.hip): image i in rows [0, dh_i) of slot i, zeros below, written by the same kernel -- no
// memset in front of it and no read of what the buffer held. The per-thread text -- descriptor, the byte-wise source pixel, the four-pixel
// walk over the canvas, the checked store -- is canvas_pack_dev.h's, pinned on the CPU from that very text (tests/test_canvas_pack.py); the
// arithmetic under it is resize_pixel.h's, shared with resize_linear_kernel (preprocess.hip). Built with -ffp-contract=off (csrc/Makefile),
// like preprocess: the sample position is a double product and difference in a fixed order.
//   It is resize_linear_mixed_kernel (resize_mixed.hip) with another destination: that kernel writes one padded block per image, at a pitch
//   that is a multiple of 12, one workgroup per row segment; a canvas has pitch 3 wc with wc any value and rows that no image fills, so here
//   a thread owns four consecutive pixels of the canvas's LINEAR order (three aligned dwords; a wave's stores fill 768 contiguous bytes) and
//   each pixel finds its own slot, row and column -- jpeg_color_resize_ragged_kernel's mapping (jpeg_ragged.hip). One pair of 32-bit
//   divisions by hc x wc and wc per thread, none per pixel. The source taps are byte gathers from two source rows through the vector L1 / L2;
//   the descriptor table (40 bytes per image) stays cache-resident. No LDS, no synchronisation. HBM-bound.
#include "common.h"
#include "canvas_pack_dev.h"

namespace ctpn {

__global__ __launch_bounds__(CP_THREADS) void canvas_pack_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ canvas, const CpImage* __restrict__ tab, int n,
                                                                 int hc, int wc) {
  cp_thread(src, canvas, tab, n, hc, wc, (long long)blockIdx.x * CP_THREADS + threadIdx.x);
}

static_assert(sizeof(CpImage) == CP_DESC_BYTES, "common.h sizes the descriptor table");

void canvas_pack_fill(void* table, int n, const long long* src_off, const long long* src_pitch, const int* h, const int* w, const double* f, const int* dh) {
  CpImage* tab = static_cast<CpImage*>(table);
  for (int i = 0; i < n; ++i) cp_describe(tab[i], src_off[i], src_pitch[i], h[i], w[i], f[i], dh[i]);
}

// tab_dev: n descriptors (canvas_pack_fill) in device memory; image i's pixels at src_dev + its src_off; canvas_dev: n x hc x wc x 3 bytes,
// 4-byte aligned, every one of them written
int launch_canvas_pack(const uint8_t* src_dev, uint8_t* canvas_dev, const void* tab_dev, int n, int hc, int wc, hipStream_t s) {
  if (n <= 0 || hc <= 0 || wc <= 0 || ((uintptr_t)canvas_dev & 3)) return fail(CTPN_ERR_ARG, "canvas_pack: grid out of range");
  const long long wgs = (cp_groups(n, hc, wc) + CP_THREADS - 1) / CP_THREADS;
  if (wgs > 0x7fffffffLL) return fail(CTPN_ERR_ARG, "canvas_pack: grid out of range");
  hipLaunchKernelGGL(canvas_pack_kernel, dim3((unsigned)wgs), dim3(CP_THREADS), 0, s, src_dev, canvas_dev, (const CpImage*)tab_dev, n, hc, wc);
  return launch_status("canvas_pack");
}

}  // namespace ctpn
