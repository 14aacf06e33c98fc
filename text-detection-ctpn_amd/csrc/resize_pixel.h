// The per-sample arithmetic of cv2.resize(INTER_LINEAR) as the library restates it (preprocess.hip's header has the algorithm and its source),
// in a header of its own so that ONE text serves resize_linear_kernel (preprocess.hip) and the fused colour + resize kernel of the ragged JPEG
// path (jpeg_ragged.hip, through jpeg_ragged_dev.h), and compiles for the host as well (tests/jpeg_ragged_host.cpp). Every unit that includes
// this file for its kernels is built with -ffp-contract=off: the sample position is a double product and difference in a fixed order.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD inline
#endif

namespace ctpn {

RS_HD void rs_coord(int d, double inv_f, int n, int clamp_w, int& s, float& f) {
  f = (float)(((double)d + 0.5) * inv_f - 0.5);
  s = (int)floorf(f);
  f -= (float)s;
  if (clamp_w) {
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n - 1) { s = n - 1; f = 0.f; }
  }
}

RS_HD int rs_short(float v) {   // saturate_cast<short>(float): round half to even, saturate
  const int r = (int)rintf(v);
  return r < -32768 ? -32768 : (r > 32767 ? 32767 : r);
}

// the uint8 form: 11-bit weights of a fraction, and one channel of one output pixel from its four neighbours (p<row><column>)
RS_HD void rs_weights(float f, int& w0, int& w1) {
  w0 = rs_short((1.f - f) * 2048.f);
  w1 = rs_short(f * 2048.f);
}

RS_HD int rs_u8(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1) {
  const int S0 = p00 * a0 + p01 * a1;
  const int S1 = p10 * a0 + p11 * a1;
  const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

}  // namespace ctpn
