// TEST INFRASTRUCTURE (never part of the product library): the JPEG encoder's per-sample source text -- csrc/jpeg_enc_pixel.h, the functions
// jpeg_fdct_kernel is made of -- compiled for the host with the HIP qualifiers defined away and driven the way the kernel drives it: a tile
// of 8 MCUs (128 x 16 pixels), 4 x 2 pixels per "thread" with the last column / row repeated, luma and downsampled chroma tiles, then per
// 8 x 8 block a row pass, a column pass, the quantiser, zig-zag order, and the dummy-block rule for luma blocks outside the component.
// tests/test_jpeg_encode.py builds this file with g++, feeds its coefficients to the library's entropy coder and compares the file with
// Pillow's, so the arithmetic is pinned on the CPU from the very text hipcc compiles.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../text-detection-ctpn_amd/csrc/jpeg_enc_pixel.h"

#include <stddef.h>
#include <string.h>

// bgr: h x w x 3; q2x64: the two quantisation tables (natural order); coef: [Y: 2 mcuy x 2 mcux][Cb: mcuy x mcux][Cr][64] int16, zig-zag order
extern "C" int jpeg_enc_coefficients_host(const uint8_t* bgr, int h, int w, const uint16_t* q2x64, int16_t* coef) {
  using namespace ctpn;
  static const uint8_t zzpos[64] = CTPN_JENC_ZIGZAG_POS;
  JencQ sq[2][64];
  for (int c = 0; c < 2; ++c)
    for (int k = 0; k < 64; ++k) { sq[c][k].magic = jenc_magic(q2x64[64 * c + k]); sq[c][k].half = 4u * q2x64[64 * c + k]; }
  const int mcux = (w + 15) / 16, mcuy = (h + 15) / 16;
  const int bw[3] = {2 * mcux, mcux, mcux};
  const long long off[3] = {0, (long long)4 * mcux * mcuy * 64, (long long)5 * mcux * mcuy * 64};
  const int real_bw0 = (w + 7) >> 3, real_bh0 = (h + 7) >> 3;
  for (int my = 0; my < mcuy; ++my)
    for (int tile = 0; tile < (mcux + 7) / 8; ++tile) {
      uint8_t sY[16][128], sC[2][8][64];
      for (int tid = 0; tid < 256; ++tid) {                      // stage 1
        const int gx = tid & 31, ry = tid >> 5, x0 = tile * 128 + gx * 4;
        const int cy = jenc_chroma_row(my * 8 + ry, h);
        int cb[2][4], cr[2][4];
        for (int r = 0; r < 2; ++r) {
          int y = my * 16 + ry * 2 + r, yc = 2 * cy + r;
          y = y < h ? y : h - 1;
          yc = yc < h ? yc : h - 1;
          for (int k = 0; k < 4; ++k) {
            int x = x0 + k;
            x = x < w ? x : w - 1;
            const uint8_t* p = bgr + ((long long)y * w + x) * 3;
            int Y, Yc;
            jenc_ycc(p[0], p[1], p[2], Y, cb[r][k], cr[r][k]);
            sY[ry * 2 + r][gx * 4 + k] = (uint8_t)Y;
            if (yc != y) { p = bgr + ((long long)yc * w + x) * 3; jenc_ycc(p[0], p[1], p[2], Yc, cb[r][k], cr[r][k]); }
          }
        }
        for (int j = 0; j < 2; ++j) {
          sC[0][ry][gx * 2 + j] = (uint8_t)jenc_h2v2(cb[0][2 * j], cb[0][2 * j + 1], cb[1][2 * j], cb[1][2 * j + 1], j);
          sC[1][ry][gx * 2 + j] = (uint8_t)jenc_h2v2(cr[0][2 * j], cr[0][2 * j + 1], cr[1][2 * j], cr[1][2 * j + 1], j);
        }
      }
      for (int it = 0; it < 2; ++it) {                           // stage 2
        int16_t zq[32][64];
        const int nb = it == 0 ? 32 : 16;
        for (int lb = 0; lb < nb; ++lb) {
          const int c = it == 0 ? 0 : (lb < 8 ? 1 : 2);
          const int by = c == 0 ? lb >> 4 : 0, bx = c == 0 ? lb & 15 : lb & 7;
          int ws[8][8], x[8], o[8];
          for (int t = 0; t < 8; ++t) {                          // lane t: row t
            const uint8_t* src = c == 0 ? &sY[by * 8 + t][bx * 8] : &sC[c - 1][t][bx * 8];
            for (int k = 0; k < 8; ++k) x[k] = (int)src[k] - 128;
            jfdct_1d(x, o, true);
            for (int k = 0; k < 8; ++k) ws[t][k] = o[k];
          }
          for (int t = 0; t < 8; ++t) {                          // lane t: column t
            for (int k = 0; k < 8; ++k) x[k] = ws[k][t];
            jfdct_1d(x, o, false);
            for (int k = 0; k < 8; ++k) zq[lb][zzpos[8 * k + t]] = (int16_t)jenc_quant(o[k], sq[c ? 1 : 0][8 * k + t]);
          }
        }
        for (int lb = 0; lb < nb; ++lb) {
          const int c = it == 0 ? 0 : (lb < 8 ? 1 : 2);
          const int by = c == 0 ? lb >> 4 : 0, bx = c == 0 ? lb & 15 : lb & 7;
          const int bxg = (c == 0 ? tile * 16 : tile * 8) + bx, byg = (c == 0 ? my * 2 : my) + by;
          if (bxg >= bw[c]) continue;
          int16_t* dst = coef + off[c] + ((long long)byg * bw[c] + bxg) * 64;
          memcpy(dst, zq[lb], 64 * sizeof(int16_t));
          if (c == 0) {
            const int s = jenc_dummy_src(by, bx & 1, (bxg | 1) >= real_bw0, my * 2 + 1 >= real_bh0);
            if (s >= 0) { memset(dst, 0, 64 * sizeof(int16_t)); dst[0] = zq[(s >> 1) * 16 + (bx & ~1) + (s & 1)][0]; }
          }
        }
      }
    }
  return 0;
}

// the quantiser's multiply-and-shift against plain division, for every baseline table value and every magnitude the FDCT can produce
extern "C" long long jpeg_enc_quant_mismatches(int cmax) {
  using namespace ctpn;
  long long bad = 0;
  for (uint32_t q = 1; q <= 255; ++q) {
    const JencQ jq = {jenc_magic(q), 4u * q};
    for (int c = -cmax; c <= cmax; ++c) {
      const int a = c < 0 ? -c : c, v = (a + 4 * (int)q) / (8 * (int)q);
      bad += jenc_quant(c, jq) != (c < 0 ? -v : v);
    }
  }
  return bad;
}
