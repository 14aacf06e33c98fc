// The per-sample arithmetic of the JPEG ENCODER's device half (jpeg_enc.hip), in a header of its own for the reason jpeg_pixel.h is one: ONE
// source for two compilers. hipcc builds jpeg_fdct_kernel from these functions; tests/test_jpeg_encode.py compiles the same text with g++
// (tests/jpeg_enc_host.cpp, the HIP qualifiers defined away) and compares the files it leads to with Pillow's, byte for byte, on the CPU.
// libjpeg's integer arithmetic restated from the published algorithms (libjpeg 6b API level, which libjpeg-turbo implements bit for bit):
// jccolor.c rgb_ycc_convert, jcsample.c h2v2_downsample, jfdctint.c jpeg_fdct_islow, jcdctmgr.c's quantiser, jccoefct.c's dummy blocks.
#pragma once
#include <stdint.h>

namespace ctpn {

// position in the zig-zag sequence of the coefficient at natural index 8 * row + column (the inverse of jpeg.hip's kZigzag)
#define CTPN_JENC_ZIGZAG_POS                                                                                                                  \
  {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, \
   54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63}

// jccolor.c: SCALEBITS 16, FIX(x) = (int)(x * 65536 + 0.5), ONE_HALF = 1 << 15, CBCR_OFFSET = 128 << 16; the chroma rows carry
// CBCR_OFFSET + ONE_HALF - 1 (libjpeg folds the rounding term into the B -> Cb and R -> Cr tables, both FIX(0.5))
__host__ __device__ __forceinline__ void jenc_ycc(int b, int g, int r, int& y, int& cb, int& cr) {
  y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// jcsample.c h2v2_downsample: the mean of a 2 x 2 cell with the bias 1, 2, 1, 2, ... along the OUTPUT columns (no smoothing)
__host__ __device__ __forceinline__ int jenc_h2v2(int p00, int p01, int p10, int p11, int out_col) {
  return (p00 + p01 + p10 + p11 + 1 + (out_col & 1)) >> 2;
}

// the downsampled row a chroma row of the MCU grid takes its samples from: rows below the component repeat its LAST downsampled row
// (jcprepct.c expand_bottom_edge on the downsampled data) -- not the downsampling of repeated pixel rows, which differs for even heights
__host__ __device__ __forceinline__ int jenc_chroma_row(int cy, int h) {
  const int last = ((h + 1) >> 1) - 1;
  return cy < last ? cy : last;
}

// jfdctint.c: one 8-point pass of the islow forward DCT (CONST_BITS 13, PASS1_BITS 2). first = true: the row pass (outputs scaled up by
// 1 << PASS1_BITS), false: the column pass (PASS1_BITS removed again; the result stays scaled by 8, which the quantiser divides out)
__host__ __device__ __forceinline__ void jfdct_1d(const int (&d)[8], int (&o)[8], bool first) {
  const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  const int sh = first ? 13 - 2 : 13 + 2, rnd = 1 << (sh - 1);
  if (first) { o[0] = (tmp10 + tmp11) << 2; o[4] = (tmp10 - tmp11) << 2; }
  else { o[0] = (tmp10 + tmp11 + 2) >> 2; o[4] = (tmp10 - tmp11 + 2) >> 2; }
  int z1 = (tmp12 + tmp13) * 4433;
  o[2] = (z1 + tmp13 * 6270 + rnd) >> sh;
  o[6] = (z1 + tmp12 * (-15137) + rnd) >> sh;
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
  z1 *= -7373; z2 *= -20995; z3 = z3 * (-16069) + z5; z4 = z4 * (-3196) + z5;
  o[7] = (t4 + z1 + z3 + rnd) >> sh;
  o[5] = (t5 + z2 + z4 + rnd) >> sh;
  o[3] = (t6 + z2 + z3 + rnd) >> sh;
  o[1] = (t7 + z1 + z4 + rnd) >> sh;
}

// jcdctmgr.c: sign(c) * ((|c| + 4 q) / (8 q)) -- the FDCT's result is scaled by 8. The division is a multiplication by
// magic = floor(2^32 / (8 q)) + 1 (jenc_magic): exact for |c| + 4 q < 2^20 and 8 q < 2^11, which 8-bit samples and baseline tables
// (q <= 255) never leave (|c| <= 8 * 1024 * 1.4)
struct JencQ { uint32_t magic, half; };      // half = 4 q
__host__ __device__ __forceinline__ uint32_t jenc_magic(uint32_t q) { return (uint32_t)((1ull << 32) / (8ull * q)) + 1u; }
__host__ __device__ __forceinline__ int jenc_quant(int c, const JencQ& q) {
  const uint32_t a = (uint32_t)(c < 0 ? -c : c) + q.half;
  const int v = (int)(((uint64_t)a * q.magic) >> 32);
  return c < 0 ? -v : v;
}

// jccoefct.c compress_data: a luma block of the MCU grid that lies wholly outside the component (right of its last block column, below its
// last block row) is a DUMMY: all AC zero, DC = the DC of the block BEFORE it in the MCU's block order (so its DC difference codes as 0) --
// for a block of a dummy row that is the last block of the row above, whichever column it is in. (by, bx): the block inside its 2 x 2 MCU;
// col1_outside / row1_outside: the MCU's second block column / row lies outside the component (its first never does).
// Returns the in-MCU index 2 * by + bx of the REAL block whose quantised DC it takes, or -1 for a real block.
__host__ __device__ __forceinline__ int jenc_dummy_src(int by, int bx, bool col1_outside, bool row1_outside) {
  if (by == 1 && row1_outside) return col1_outside ? 0 : 1;      // the last block of the row above: (0, 1) -- itself a dummy of (0, 0) when column 1 is outside
  if (bx == 1 && col1_outside) return 2 * by;
  return -1;
}

}  // namespace ctpn
