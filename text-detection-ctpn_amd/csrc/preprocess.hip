// Input pipeline on device: cv2.resize(..., fx, fy, INTER_LINEAR) of the two places the reference
// rescales an image -- ctpn/demo.py:21-25 (resize_im, uint8 BGR) and lib/fast_rcnn/test.py:17-27 (_get_image_blob, float32
// after the mean subtraction). OpenCV (opencv_python==3.4.0.12, requirements.txt) is not in the reference tree, so this
// follows its published algorithm (modules/imgproc/src/resize.cpp, 3.4 branch) -- PARITY UNPINNED against the real cv2:
//   dsize = cvRound(src * f) (round half to even); sample position fx = (float)((dx + 0.5) / f - 0.5), sx = floor(fx);
//   sx < 0 -> sx = 0, fx = 0; sx >= w - 1 -> sx = w - 1, fx = 0 (columns only; rows are clamped instead);
//   uint8: 11-bit fixed-point weights a = cvRound(w * 2048) as short, horizontal sums in int,
//          dst = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
//   float: S = s0 * a0 + s1 * a1 per row, dst = S0 * b0 + S1 * b1, all in fp32 without contraction.
// One thread per output pixel (3 channels); HBM-bound and tiny next to the convolutions.
#include <cmath>

#include "common.h"
#include "resize_pixel.h"      // rs_coord, rs_short, rs_weights, rs_u8: the per-sample arithmetic (shared with jpeg_ragged.hip)

namespace ctpn {

template <typename T>
__global__ void resize_linear_kernel(const T* __restrict__ src, T* __restrict__ dst, int n, int h, int w, int dh, int dw, double inv_fx,
                                     double inv_fy) {
  const long long total = (long long)n * dh * dw;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x) {
    const int dx = (int)(p % dw);
    const int dy = (int)((p / dw) % dh);
    const int img = (int)(p / ((long long)dw * dh));
    int sx, sy;
    float fx, fy;
    rs_coord(dx, inv_fx, w, 1, sx, fx);
    rs_coord(dy, inv_fy, h, 0, sy, fy);
    const int x1 = sx + 1 < w ? sx + 1 : w - 1;
    const int y0 = sy < 0 ? 0 : (sy < h ? sy : h - 1);
    const int y1 = sy + 1 < 0 ? 0 : (sy + 1 < h ? sy + 1 : h - 1);
    const T* r0 = src + ((long long)img * h + y0) * w * 3;
    const T* r1 = src + ((long long)img * h + y1) * w * 3;
    T* o = dst + p * 3;
    if constexpr (sizeof(T) == 1) {
      int a0, a1, b0, b1;
      rs_weights(fx, a0, a1);
      rs_weights(fy, b0, b1);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        o[c] = (T)rs_u8((int)r0[sx * 3 + c], (int)r0[x1 * 3 + c], (int)r1[sx * 3 + c], (int)r1[x1 * 3 + c], a0, a1, b0, b1);
    } else {
      const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float S0 = __fadd_rn(__fmul_rn((float)r0[sx * 3 + c], a0), __fmul_rn((float)r0[x1 * 3 + c], a1));
        const float S1 = __fadd_rn(__fmul_rn((float)r1[sx * 3 + c], a0), __fmul_rn((float)r1[x1 * 3 + c], a1));
        o[c] = (T)__fadd_rn(__fmul_rn(S0, b0), __fmul_rn(S1, b1));
      }
    }
  }
}

// cvRound: round half to even
int resize_out_dim(int src, double f) { return (int)std::nearbyint((double)src * f); }

int launch_resize_linear(const void* src, void* dst, int is_f32, int n, int h, int w, int dh, int dw, double fx, double fy, hipStream_t s) {
  if (n <= 0 || h <= 0 || w <= 0 || dh <= 0 || dw <= 0 || !(fx > 0.0) || !(fy > 0.0)) return fail(CTPN_ERR_ARG, "resize: bad geometry");
  const long long total = (long long)n * dh * dw;
  const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 65536);
  if (is_f32)
    hipLaunchKernelGGL(resize_linear_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)src, (float*)dst, n, h, w, dh, dw, 1.0 / fx, 1.0 / fy);
  else
    hipLaunchKernelGGL(resize_linear_kernel<uint8_t>, dim3(grid), dim3(256), 0, s, (const uint8_t*)src, (uint8_t*)dst, n, h, w, dh, dw, 1.0 / fx, 1.0 / fy);
  return launch_status("resize");
}

}  // namespace ctpn
