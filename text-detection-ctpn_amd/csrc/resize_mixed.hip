// cv2.resize(INTER_LINEAR) of n uint8 BGR images of different sizes by n different factors in ONE launch: the images of a ragged canvas
// resized back to their files' sizes by 1 / scale_i for the annotated writer (api_out_ragged.hip). The per-thread text -- descriptor,
// work-item search, the four-pixel sample, the checked store -- is resize_mixed_dev.h's, pinned on the CPU from that very text
// (tests/test_out_ragged.py); the arithmetic under it is resize_pixel.h's, shared with resize_linear_kernel (preprocess.hip). Built with
// -ffp-contract=off (csrc/Makefile), like preprocess: the sample position is a double product and difference in a fixed order.
//   One workgroup = one wave = one output row x RM_SEG_PIXELS output pixels of one image, found by a binary search of the items' prefix
//   sums (uniform over the workgroup: scalar loads); a thread owns four consecutive output pixels, stored as three whole dwords (a wave's
//   stores fill 768 contiguous bytes of an output row). The source taps are byte gathers from two source rows. HBM-bound.
#include "common.h"
#include "resize_mixed_dev.h"

namespace ctpn {

__global__ __launch_bounds__(RM_THREADS) void resize_linear_mixed_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const RmImage* __restrict__ tab, int n) {
  rm_thread(src, dst, tab, n, (long long)blockIdx.x, (int)threadIdx.x);
}

static_assert(sizeof(RmImage) == RM_DESC_BYTES, "common.h sizes the descriptor table");

long long resize_mixed_fill(void* table, int n, const int* h, const int* w, const int* dh, const int* dw, const long long* src_off, const long long* src_pitch,
                            const long long* dst_off, const double* inv_f) {
  RmImage* tab = static_cast<RmImage*>(table);
  for (int i = 0; i < n; ++i) rm_describe(tab[i], h[i], w[i], dh[i], dw[i], src_off[i], src_pitch[i], dst_off[i], inv_f[i]);
  return rm_prefix(tab, n);
}

size_t resize_mixed_pitch(int dw) { return (size_t)rm_pitch(dw); }

// tab_dev: n descriptors with their prefix sums (resize_mixed_fill), total_items work items in all; dst_dev 4-byte aligned
int launch_resize_linear_mixed(const uint8_t* src_dev, uint8_t* dst_dev, const void* tab_dev, int n, long long total_items, hipStream_t s) {
  if (n <= 0 || total_items < n || total_items > RM_MAX_ITEMS || ((uintptr_t)dst_dev & 3)) return fail(CTPN_ERR_ARG, "resize (mixed sizes): grid out of range");
  hipLaunchKernelGGL(resize_linear_mixed_kernel, dim3((unsigned)total_items), dim3(RM_THREADS), 0, s, src_dev, dst_dev, (const RmImage*)tab_dev, n);
  return launch_status("resize (mixed sizes)");
}

}  // namespace ctpn
