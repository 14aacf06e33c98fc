// The per-sample arithmetic of the JPEG decoder's device half (jpeg.hip), in a header of its own so that ONE source serves two compilers:
// hipcc compiles it into jpeg_idct_kernel / jpeg_color_kernel and their ragged forms (jpeg_ragged.hip); tests/test_jpeg.py compiles the same text with g++ (the HIP qualifiers
// defined away) into a small checker library and compares it with Pillow's decode on the CPU -- a new layout's arithmetic is pinned before
// it ever reaches a GPU. Nothing here is product host code: the library itself only ever calls these functions from its kernels.
#pragma once
#include <stdint.h>

namespace ctpn {

struct JpegGeom {
  int h, w, ncomp, hs0, vs0;         // luma sampling factors: 1 x 1 (4:4:4 / gray), 2 x 2 (4:2:0), 2 x 1 (4:2:2), 1 x 2 (4:4:0); the chroma planes' are 1 x 1
  int orient, oh, ow;                // EXIF orientation 1 .. 8 (cv2.imread applies it) and the size of the turned image: (h, w) for 1 .. 4, (w, h) for 5 .. 8
  int bw[3], bh[3];                  // blocks per row / column of every component
  long long coef_off[3];             // int16 offset of component c inside an image's coefficient block
  long long plane_off[3];            // byte offset of component c inside an image's plane block
  long long coef_per_img, plane_per_img;
  long long blocks_per_img;
};

// The IDCT restates libjpeg-turbo's x86 SIMD "islow" (jsimd_idct_islow_sse2 / _avx2: what Pillow and cv2 run on x86-64), not jidctint.c in
// full-width integers. On every coefficient an encoder can write from 8-bit pixels the two agree; beyond that range (tables scaled up,
// 16-bit tables, coefficients no forward DCT produces) the SIMD code's 16-bit lanes show, and its picture is the pin:
//   coef * q keeps its low 16 bits, signed (pmullw);   in0 + in4, in0 - in4, in7 + in3 and in5 + in1 are 16-bit lanes and wrap;
//   every other sum is a pair of 16 x 16 products in a 32-bit lane (pmaddwd, the constants folded pairwise);
//   each pass ends in (sum + rounding) >> descale, saturated to int16 (packssdw); pass 2 then saturates to -128 .. 127 and adds 128
//   (pass 2 below saturates once, to -128 .. 127: the same value);
//   a block whose rows 1 .. 7 are all zero skips pass 1: every workspace row is row 0 << PASS1_BITS, wrapped to 16 bits, not saturated.
// A libjpeg-turbo that runs without SIMD follows jidctint.c's masked range-limit table instead and differs from both out of range.
// No signed overflow anywhere: int16 x uint16 is at most 32768 x 65535 = 2 147 450 880 < 2^31, and the inputs of a pass are 16-bit values,
// so every sum below stays inside 31 bits (largest: 2 115 960 832). Nothing needs unsigned arithmetic; tests/jpeg_idct_ubsan_host.cpp
// runs both passes under UBSan.
__host__ __device__ __forceinline__ int jidct_wrap16(int v) { return (int)(int16_t)(uint16_t)(uint32_t)v; }
__host__ __device__ __forceinline__ int jidct_sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

__host__ __device__ __forceinline__ int jidct_sat8(int v) { return v < -128 ? -128 : (v > 127 ? 127 : v); }

// x: eight 16-bit values; o: (sum + rounding) >> descale, not yet saturated
__host__ __device__ __forceinline__ void jidct_1d(const int (&x)[8], int (&o)[8], int descale) {
  // even part: tmp2 = z2 * F0.541 + z3 * (F0.541 - F1.847), tmp3 = z2 * (F0.541 + F0.765) + z3 * F0.541
  const int tmp2 = x[2] * 4433 + x[6] * (-10704), tmp3 = x[2] * 10703 + x[6] * 4433;
  const int tmp0 = jidct_wrap16(x[0] + x[4]) * 8192, tmp1 = jidct_wrap16(x[0] - x[4]) * 8192;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  // odd part: z3 = in7 + in3, z4 = in5 + in1 (16-bit); z5 folded into both
  const int z3w = jidct_wrap16(x[7] + x[3]), z4w = jidct_wrap16(x[5] + x[1]);
  const int z3 = z3w * (-6436) + z4w * 9633, z4 = z3w * 9633 + z4w * 6437;
  const int t0 = x[7] * (-4927) + x[1] * (-7373) + z3;
  const int t1 = x[5] * (-4176) + x[3] * (-20995) + z4;
  const int t2 = x[5] * (-20995) + x[3] * 4177 + z3;
  const int t3 = x[7] * (-7373) + x[1] * 4926 + z4;
  const int r = 1 << (descale - 1);
  o[0] = (tmp10 + t3 + r) >> descale; o[7] = (tmp10 - t3 + r) >> descale;
  o[1] = (tmp11 + t2 + r) >> descale; o[6] = (tmp11 - t2 + r) >> descale;
  o[2] = (tmp12 + t1 + r) >> descale; o[5] = (tmp12 - t1 + r) >> descale;
  o[3] = (tmp13 + t0 + r) >> descale; o[4] = (tmp13 - t0 + r) >> descale;
}

// The two passes of one 8 x 8 block's IDCT as thread t of the block's eight runs them. The caller finds the block (blk: its 64 coefficients,
// q: its component's table, dst: row t of the block in its plane, 8-byte aligned), keeps the transpose buffer and puts its barrier between
// the passes. A lane that is not live computes on zeros and neither loads nor stores: its pointers are never dereferenced.
// load: column t (elements t, t + 8, ...) dequantised into x; returns the OR of the column's seven RAW coefficients of rows 1 .. 7. The
// caller ORs the eight columns' answers (the kernels: jidct_group8_or; a host loop: over t) -- zero means the block takes the shortcut
__host__ __device__ __forceinline__ int jidct_load(const int16_t* __restrict__ blk, const uint16_t* __restrict__ q, bool live, int t, int (&x)[8]) {
  int ac = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = 0;
  if (live) {      // (one branch around the sixteen loads, not a select per element: a load cannot be hoisted out of a select)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = blk[8 * k + t];
      if (k) ac |= c;
      x[k] = jidct_wrap16(c * (int)q[8 * k + t]);      // (|c| <= 32768, q <= 65535: the product stays inside 31 bits)
    }
  }
  return ac;
}

#if defined(__HIPCC__)
// the OR of v over the eight consecutive lanes of a block's threads (tid >> 3 names the block, so a group is one half of a DPP row and
// never straddles a wave): an xor butterfly over lane distances 1, 2, 4 as three DPP moves -- quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// then row_half_mirror (lane i of the eight reads lane 7 - i, i.e. the other quad, whose four lanes agree by then). No LDS, no barrier.
// Every lane of the wave runs it, dead lanes with v = 0: the kernels call it outside any branch, with the whole workgroup active
__device__ __forceinline__ int jidct_group8_or(int v) {
  v |= __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
  v |= __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
  v |= __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);
  return v;
}
#endif

// pass 1: x from jidct_load, block_ac the block's OR; o[k] goes to row k, column t of the transpose buffer.
// The shortcut without a second path: with rows 1 .. 7 zero the general pass gives every o[k] = sat16(4 x[0]) exactly
// ((x[0] * 8192 + 1024) >> 11 = 4 x[0]), where the shortcut wants wrap16(4 x[0]). wrap16(4 x[0]) is 4 times x[0]'s low 14 bits taken as a
// signed value, which the general pass reproduces without saturating -- so a flat block only swaps x[0] for that (one select, no branch:
// a wave mixes both kinds of block)
__host__ __device__ __forceinline__ void jidct_pass1(const int (&x)[8], int block_ac, int (&o)[8]) {
  int y[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) y[k] = x[k];
  y[0] = block_ac == 0 ? jidct_wrap16(x[0] * 4) >> 2 : x[0];
  jidct_1d(y, o, 13 - 2);
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = jidct_sat16(o[k]);
}

// pass 1 in one call, for a caller that runs a block's columns one after the other and has no lanes to exchange the flag between (a host
// loop over t that keeps no per-column state): the block's flag is read from the block itself, rows 1 .. 7 of all eight columns. Same
// loads, same flag, same pass as the three-step form above; the kernels do not use it (56 loads per thread instead of 7 and three moves)
__host__ __device__ __forceinline__ void jidct_pass1(const int16_t* __restrict__ blk, const uint16_t* __restrict__ q, bool live, int t, int (&o)[8]) {
  int x[8], ac = 0;
  jidct_load(blk, q, live, t, x);
  if (live)
    for (int k = 8; k < 64; ++k) ac |= blk[k];
  jidct_pass1(x, ac, o);
}

struct alignas(8) JpegVec8 { uint32_t lo, hi; };

// pass 2: row t (x: that row of the transpose buffer); eight samples as one 8-byte store
__host__ __device__ __forceinline__ void jidct_pass2(uint8_t* __restrict__ dst, bool live, const int (&x)[8]) {
  int y[8], o[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) y[k] = jidct_wrap16(x[k]);      // (pass 1's results are 16-bit values already; saying so buys 24-bit multiplies)
  jidct_1d(y, o, 13 + 2 + 3);
  if (!live) return;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {      // (packssdw, then packsswb: saturating to int16 first changes nothing)
    lo |= (uint32_t)(jidct_sat8(o[k]) + 128) << (8 * k);
    hi |= (uint32_t)(jidct_sat8(o[k + 4]) + 128) << (8 * k);
  }
  *(JpegVec8*)dst = JpegVec8{lo, hi};
}

// the four pixels p0 .. p0 + 3 (B | G << 8 | R << 16 each; p0 a multiple of 4) of an image of `total` pixels at out: three aligned dwords,
// or byte by byte where fewer than four are left. Nothing is written at or behind total x 3 bytes.
__host__ __device__ __forceinline__ void jpeg_store4(uint8_t* __restrict__ out, long long p0, long long total, const uint32_t (&px)[4]) {
  if (p0 + 4 <= total) {
    uint32_t* o = (uint32_t*)(out + p0 * 3);
    o[0] = px[0] | (px[1] << 24);
    o[1] = (px[1] >> 8) | (px[2] << 16);
    o[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
    uint8_t* ob = out + p0 * 3;
    for (int k = 0; k < 4 && p0 + k < total; ++k) { ob[3 * k] = (uint8_t)px[k]; ob[3 * k + 1] = (uint8_t)(px[k] >> 8); ob[3 * k + 2] = (uint8_t)(px[k] >> 16); }
  }
}

// pixel (oy, ox) of the image as cv2.imread returns it -> the stored pixel it is (EXIF orientation, tag 0x0112: 2 mirrored left-right,
// 3 turned by 180 degrees, 4 mirrored top-bottom, 5 transposed, 6 needs a quarter turn clockwise, 7 transverse, 8 a quarter turn
// anti-clockwise); h, w: the STORED size
__host__ __device__ __forceinline__ void jpeg_orient(int orient, int h, int w, int oy, int ox, int& y, int& x) {
  switch (orient) {
    case 2: y = oy; x = w - 1 - ox; break;
    case 3: y = h - 1 - oy; x = w - 1 - ox; break;
    case 4: y = h - 1 - oy; x = ox; break;
    case 5: y = ox; x = oy; break;
    case 6: y = h - 1 - ox; x = oy; break;
    case 7: y = h - 1 - ox; x = w - 1 - oy; break;
    case 8: y = ox; x = w - 1 - oy; break;
    default: y = oy; x = ox; break;
  }
}

// one pixel: chroma upsampling + colour conversion -> B | G << 8 | R << 16
__host__ __device__ __forceinline__ uint32_t jpeg_pixel(const uint8_t* __restrict__ P, const JpegGeom& g, int y, int x) {
  const int Y = P[g.plane_off[0] + (long long)y * (g.bw[0] * 8) + x];
  if (g.ncomp == 1) return (uint32_t)Y * 0x010101u;
  int cb, cr;
  if (g.hs0 == 1 && g.vs0 == 1) {
    cb = P[g.plane_off[1] + (long long)y * (g.bw[1] * 8) + x];
    cr = P[g.plane_off[2] + (long long)y * (g.bw[2] * 8) + x];
  } else if (g.hs0 == 1) {
    // jdsample.c h1v2_fancy_upsample (4:4:0; libjpeg-turbo >= 1.5): 3/4 nearer + 1/4 further ROW of the same column, + 1 for the upper and
    // + 2 for the lower output row of a pair; the row above the first / below the last real chroma row is that row again (the context rows
    // of jdmainct.c). Unlike the h2v1 / h2v2 filters it has no narrow-image exception (jinit_upsampler takes it whenever fancy upsampling is on)
    const int dh = (g.h + 1) >> 1;
    const int cy = y >> 1;
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : (fy > dh - 1 ? dh - 1 : fy);
    const int bias = (y & 1) ? 2 : 1;
    int v[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint8_t* C = P + g.plane_off[1 + k];
      const int pitch = g.bw[1 + k] * 8;
      v[k] = (3 * C[(long long)cy * pitch + x] + C[(long long)fy * pitch + x] + bias) >> 2;
    }
    cb = v[0]; cr = v[1];
  } else if (g.vs0 == 1) {
    // jdsample.c h2v1_fancy_upsample (4:2:2): 3/4 nearer + 1/4 further column of the SAME row, + 1 for even and + 2 for odd output columns;
    // the first and the last output column are the edge sample itself; plain replication where the downsampled width is <= 2
    const int dw = (g.w + 1) >> 1;
    const int cx = x >> 1;
    const int nx = (x & 1) ? cx + 1 : cx - 1;
    const bool edge = dw <= 2 || nx < 0 || nx > dw - 1;
    int v[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint8_t* C = P + g.plane_off[1 + k] + (long long)y * (g.bw[1 + k] * 8);
      v[k] = edge ? C[cx] : (3 * C[cx] + C[nx] + ((x & 1) ? 2 : 1)) >> 2;
    }
    cb = v[0]; cr = v[1];
  } else {
    // jdsample.c h2v2_fancy_upsample: 3/4 nearer + 1/4 further in each direction; rows replicated at the top / bottom of the image,
    // the first / last column use (4 * colsum + 8 | 7) >> 4; + 8 for even output columns, + 7 for odd ones
    const int dw = (g.w + 1) >> 1, dh = (g.h + 1) >> 1;
    const int cy = y >> 1, cx = x >> 1;
    int v[2];
    if (dw > 2) {
      int fy = (y & 1) ? cy + 1 : cy - 1;
      fy = fy < 0 ? 0 : (fy > dh - 1 ? dh - 1 : fy);
      const int nx = (x & 1) ? cx + 1 : cx - 1;
      const bool edge = nx < 0 || nx > dw - 1;
      const int bias = (x & 1) ? 7 : 8;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const uint8_t* C = P + g.plane_off[1 + k];
        const int pitch = g.bw[1 + k] * 8;
        const int cs = 3 * C[(long long)cy * pitch + cx] + C[(long long)fy * pitch + cx];
        const int ns = edge ? 0 : 3 * C[(long long)cy * pitch + nx] + C[(long long)fy * pitch + nx];
        v[k] = edge ? (cs * 4 + bias) >> 4 : (cs * 3 + ns + bias) >> 4;
      }
    } else {      // jinit_upsampler takes the fancy filter only for downsampled_width > 2: narrower images get plain 2 x 2 replication
#pragma unroll
      for (int k = 0; k < 2; ++k) v[k] = P[g.plane_off[1 + k] + (long long)cy * (g.bw[1 + k] * 8) + cx];
    }
    cb = v[0]; cr = v[1];
  }
  // jdcolor.c: SCALEBITS 16, FIX(x) = (int)(x * 65536 + 0.5)
  const int xb = cb - 128, xr = cr - 128;
  int R = Y + ((91881 * xr + 32768) >> 16);
  int B = Y + ((116130 * xb + 32768) >> 16);
  int G = Y + ((-22554 * xb + 32768 - 46802 * xr) >> 16);
  R = R < 0 ? 0 : (R > 255 ? 255 : R); G = G < 0 ? 0 : (G > 255 ? 255 : G); B = B < 0 ? 0 : (B > 255 ? 255 : B);
  return (uint32_t)B | ((uint32_t)G << 8) | ((uint32_t)R << 16);          // BGR, like cv2.imread
}

}  // namespace ctpn
