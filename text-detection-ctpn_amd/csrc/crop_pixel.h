// The per-sample arithmetic of the text-line crops (crop.hip), in a header of its own for the reason jpeg_pixel.h and jpeg_enc_pixel.h are:
// ONE source for two compilers. hipcc builds crop_lines_kernel from these functions; tests/test_crop.py compiles the same text with g++
// (tests/crop_host.cpp, the HIP qualifiers defined away) and compares it with a numpy restatement bit for bit, on the CPU.
// A crop is the bilinear map of a crop_h x Wc rectangle onto the line's quadrilateral P0 (top-left), P1 (top-right), P2 (bottom-left),
// P3 (bottom-right) -- the order ctpn_draw_boxes connects them --, sampled with resize_linear_kernel's uint8 arithmetic (preprocess.hip).
// Every unit that includes this file is built with -ffp-contract=off: the positions are double sums and products in a fixed order.
#pragma once
#include <math.h>
#include <stdint.h>

namespace ctpn {

// what the kernel reads per line: the eight coordinates of the record, the image the line lies in, its width and where its crop starts
struct CropDesc {
  double q[8];                     // x0, y0, x1, y1, x2, y2, x3, y3
  int img, wc;
  unsigned long long out_off;      // bytes from the start of the output; a multiple of 12 (crop_h x max_w x 3 per line, max_w % 4 == 0)
};

// Width of a line's crop at height crop_h: the mean of the two long edges over the mean of the two short ones, rounded half to even, in
// [1, max_w] -- a longer line is squeezed, not cut. Host only (the kernel takes it from the descriptor).
__host__ __device__ inline int crop_width(const double* r, int crop_h, int max_w) {
  const double tdx = r[2] - r[0], tdy = r[3] - r[1], bdx = r[6] - r[4], bdy = r[7] - r[5];
  const double ldx = r[4] - r[0], ldy = r[5] - r[1], rdx = r[6] - r[2], rdy = r[7] - r[3];
  const double top = sqrt(tdx * tdx + tdy * tdy), bottom = sqrt(bdx * bdx + bdy * bdy);
  const double left = sqrt(ldx * ldx + ldy * ldy), right = sqrt(rdx * rdx + rdy * rdy);
  const double wlen = (top + bottom) / 2;
  double hlen = (left + right) / 2;
  if (!(hlen >= 1.0)) hlen = 1.0;
  const double wc = nearbyint((double)crop_h * wlen / hlen);
  if (!(wc >= 1.0)) return 1;      // (also what a sum that overflowed to NaN gives)
  return wc > (double)max_w ? max_w : (int)wc;
}

// output column u of a crop Wc wide: the points of the top and the bottom edge it runs between
struct CropColumn { double tx, ty, bx, by; };
__host__ __device__ __forceinline__ CropColumn crop_column(const double* q, int u, int wc) {
  const double s = ((double)u + 0.5) / (double)wc;
  CropColumn c;
  c.tx = q[0] + s * (q[2] - q[0]);
  c.ty = q[1] + s * (q[3] - q[1]);
  c.bx = q[4] + s * (q[6] - q[4]);
  c.by = q[5] + s * (q[7] - q[5]);
  return c;
}

// ... and the source position of its pixel in output row v (pixel centres at .5, like cv2.resize)
__host__ __device__ __forceinline__ void crop_position(const CropColumn& c, int v, int crop_h, double& X, double& Y) {
  const double t = ((double)v + 0.5) / (double)crop_h;
  X = c.tx + t * (c.bx - c.tx) - 0.5;
  Y = c.ty + t * (c.by - c.ty) - 0.5;
}

// saturate_cast<short>(float): round half to even, saturate (preprocess.hip rs_short)
__host__ __device__ __forceinline__ int crop_short(float v) {
  const int r = (int)rintf(v);
  return r < -32768 ? -32768 : (r > 32767 ? 32767 : r);
}

// one axis of a sample: the two source indices and their 11-bit weights. Positions in front of the first pixel and from the last one on
// take that pixel with weight 1 -- on BOTH axes (the resize clamps its rows' indices only): the image's border is replicated without end.
// The comparisons are made on the float, before it becomes an int: any position is safe, the infinite ones and NaN (-> pixel 0) included.
__host__ __device__ __forceinline__ void crop_axis(double pos, int dim, int& i0, int& i1, int& w0, int& w1) {
  float f = (float)pos;
  const float fl = floorf(f);
  f -= fl;
  if (!(fl >= 0.f)) { i0 = 0; f = 0.f; }
  else if (fl >= (float)(dim - 1)) { i0 = dim - 1; f = 0.f; }
  else i0 = (int)fl;
  i1 = i0 + 1 < dim ? i0 + 1 : dim - 1;
  w0 = crop_short((1.f - f) * 2048.f);
  w1 = crop_short(f * 2048.f);
}

// the four-tap sample at (X, Y) of one h x w x 3 uint8 image: resize_linear_kernel's integer formula
__host__ __device__ __forceinline__ void crop_sample(const uint8_t* img, int h, int w, double X, double Y, int (&bgr)[3]) {
  int x0, x1, a0, a1, y0, y1, b0, b1;
  crop_axis(X, w, x0, x1, a0, a1);
  crop_axis(Y, h, y0, y1, b0, b1);
  const uint8_t* r0 = img + (size_t)y0 * w * 3;
  const uint8_t* r1 = img + (size_t)y1 * w * 3;
  for (int c = 0; c < 3; ++c) {
    const int S0 = (int)r0[x0 * 3 + c] * a0 + (int)r0[x1 * 3 + c] * a1;
    const int S1 = (int)r1[x0 * 3 + c] * a0 + (int)r1[x1 * 3 + c] * a1;
    const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
    bgr[c] = v < 0 ? 0 : (v > 255 ? 255 : v);
  }
}

// The image a line lies in: slot `img` of a batch whose slots are slot_h rows of w pixels. heights == null: a uniform batch, the image
// fills its slot. Else a ragged canvas: the image is rows [0, heights[img]) of its slot -- h is what crop_sample clamps the row axis at,
// so a line that hangs below its image reads the image's last row and never a canvas row under it.
__host__ __device__ __forceinline__ const uint8_t* crop_image(const uint8_t* imgs, int img, int slot_h, int w, const int* heights, int& h) {
  h = heights ? heights[img] : slot_h;
  return imgs + (size_t)img * slot_h * w * 3;
}

// four consecutive output pixels of one row, columns u0 .. u0 + 3 (u0 % 4 == 0), as the three dwords they are stored in: columns from wc
// on hold pad. cols: crop_column of the four (those from wc on are not read).
__host__ __device__ __forceinline__ void crop_quad(const uint8_t* img, int h, int w, const CropColumn (&cols)[4], int u0, int wc, int v, int crop_h,
                                                   int pad, uint32_t (&out)[3]) {
  uint32_t b[12];
  for (int k = 0; k < 4; ++k) {
    int px[3] = {pad, pad, pad};
    if (u0 + k < wc) {
      double X, Y;
      crop_position(cols[k], v, crop_h, X, Y);
      crop_sample(img, h, w, X, Y, px);
    }
    for (int c = 0; c < 3; ++c) b[3 * k + c] = (uint32_t)px[c];
  }
  for (int d = 0; d < 3; ++d) out[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
}

}  // namespace ctpn
