// BGR uint8 -> baseline JPEG: what cv2.imwrite does for the reference's annotated images (ctpn/demo.py:52), split where the work splits --
// the mirror image of jpeg.hip.
//   device : BGR -> YCbCr, 2 x 2 chroma downsampling, the 8 x 8 forward DCT and the quantiser in ONE launch (jpeg_fdct_kernel: the component
//            planes live in LDS only), int16 coefficients in zig-zag order, [block rows][block columns][64] per component over the MCU grid
//            (JpegGeom, as the decoder); draw_boxes_kernel, ctpn_draw_boxes on device images;
//   host   : baseline Huffman coding with the standard tables K.3 - K.6 and the header (one image per worker thread of the ctx's pool).
//            (The opt-in second form codes on the device too: jpeg_huff_enc.hip; the host then adds header and EOI, jpeg_enc_assemble.)
// cv2.imwrite's defaults are libjpeg at quality 95, 4:2:0, islow DCT, standard Huffman tables, no optimisation; Pillow's
// save(quality = 95, subsampling = 2) is the same encoder family (libjpeg-turbo) with the same settings, and the files written here are
// byte-equal to Pillow's (tests/test_jpeg_encode.py on the CPU from the kernels' own source text, tests/test_gpu_jpeg_encode.py through the
// C ABI). Parity with a real cv2.imwrite is UNPINNED (cv2 is not installed): it rests on cv2 linking the same encoder with these defaults.
// Marker sequence (libjpeg's, as Pillow writes it): SOI, JFIF APP0 (1.01, density unit 0, 1 x 1), DQT 0, DQT 1, SOF0, DHT DC0, AC0, DC1,
// AC1, SOS, entropy-coded data, EOI. Not written: optimised tables, progressive / 4:4:4 / 4:2:2 / gray files, restart markers, EXIF.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "jpeg_enc_mixed_dev.h"
#include "jpeg_enc_pixel.h"
#include "jpeg_enc_tables.h"

namespace ctpn {

static const uint8_t kZigzagNat[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                                       57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---------------------------------------------------------------------------------------------
// tables: ITU-T T.81 Annex K
// ---------------------------------------------------------------------------------------------
static const uint8_t kLumaQ[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// jcparam.c: jpeg_quality_scaling + jpeg_add_quant_table with force_baseline (1 .. 255). qt: 3 x 64, natural order (component 2 = component 1's)
void jpeg_enc_qtables(int quality, uint16_t* qt3x64, JencQ* q2x64) {
  const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
  for (int c = 0; c < 2; ++c)
    for (int k = 0; k < 64; ++k) {
      long v = ((long)(c ? kChromaQ[k] : kLumaQ[k]) * scale + 50L) / 100L;
      v = v < 1 ? 1 : (v > 255 ? 255 : v);
      if (qt3x64) { qt3x64[64 * c + k] = (uint16_t)v; if (c) qt3x64[128 + k] = (uint16_t)v; }
      if (q2x64) { q2x64[64 * c + k].magic = jenc_magic((uint32_t)v); q2x64[64 * c + k].half = 4u * (uint32_t)v; }
    }
}

// geometry of an h x w image written as 4:2:0 (MCU = 16 x 16 pixels: four luma blocks, one block of each chroma component)
void jpeg_enc_geom(int h, int w, JpegGeom& g) {
  g.h = h; g.w = w; g.ncomp = 3; g.hs0 = 2; g.vs0 = 2; g.orient = 1; g.oh = h; g.ow = w;
  const int mcux = (w + 15) / 16, mcuy = (h + 15) / 16;
  long long co = 0;
  for (int c = 0; c < 3; ++c) {
    g.bw[c] = c ? mcux : 2 * mcux; g.bh[c] = c ? mcuy : 2 * mcuy;
    g.coef_off[c] = g.plane_off[c] = co;
    co += (long long)g.bw[c] * g.bh[c] * 64;
  }
  g.coef_per_img = g.plane_per_img = co;
  g.blocks_per_img = co / 64;
}

// ---------------------------------------------------------------------------------------------
// host: baseline Huffman coding (jchuff.c encode_one_block) + the header
// ---------------------------------------------------------------------------------------------
static const int kHeaderBytes = 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 14;      // SOI .. SOS

// Upper bound of one h x w file. A block costs at most: its DC code (<= 11 bits in table K.4, 9 in K.3) + 11 magnitude bits, and 63 AC
// coefficients of <= 16 code bits + 10 magnitude bits each (ZRL and EOB codes only stand where coefficients are zero, which cost nothing
// else, and sixteen zeros cost one 11-bit ZRL: less than one coded coefficient): 22 + 63 * 26 = 1660 bits < 208 bytes; every byte may
// be 0xFF and need a stuffed zero behind it: 416. The final padding byte (and its stuffing), EOI.
size_t jpeg_encode_capacity(int h, int w) {
  const size_t mcus = (size_t)((w + 15) / 16) * (size_t)((h + 15) / 16);
  return (size_t)kHeaderBytes + mcus * 6 * 416 + 2 + 2;
}

struct JencHuff { uint16_t code[256]; uint8_t len[256]; };
static void jenc_huff_build(JencHuff& h, const uint8_t bits[16], const uint8_t* vals) {
  std::memset(&h, 0, sizeof(h));
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) { h.code[vals[k]] = (uint16_t)code; h.len[vals[k]] = (uint8_t)l; }
    code <<= 1;
  }
}
struct JencTables {
  JencHuff dc[2], ac[2];
  JencTables() { for (int c = 0; c < 2; ++c) { jenc_huff_build(dc[c], kBitsDc[c], kValsDc); jenc_huff_build(ac[c], kBitsAc[c], kValsAc[c]); } }
};
static const JencTables& jenc_tables() { static const JencTables t; return t; }

// bytes behind `cap` are counted, not written: a too-small buffer still learns the size it needs
struct JencSink {
  uint8_t* out; size_t cap, n = 0;
  uint64_t acc = 0; int bits = 0;
  inline void byte(uint8_t b) { if (n < cap) out[n] = b; ++n; }
  inline void put(uint32_t code, int len) {
    acc = (acc << len) | code; bits += len;
    while (bits >= 8) {
      const uint8_t b = (uint8_t)(acc >> (bits - 8));
      byte(b);
      if (b == 0xFF) byte(0);
      bits -= 8;
    }
  }
  inline void flush() { if (bits) put((1u << (8 - bits)) - 1u, 8 - bits); }      // jchuff.c flush_bits: the last byte is filled with 1-bits (and stuffed like any other)
  inline void u16(int v) { byte((uint8_t)(v >> 8)); byte((uint8_t)v); }
  inline void raw(const uint8_t* p, size_t k) { for (size_t i = 0; i < k; ++i) byte(p[i]); }
};

static inline int jenc_nbits(int v) { return v ? 32 - __builtin_clz((unsigned)v) : 0; }

template <bool ZZ>
static inline bool jenc_block(JencSink& s, const int16_t* blk, int& pred, const JencHuff& dc, const JencHuff& ac) {
  int diff = (int)blk[0] - pred;
  pred = blk[0];
  int mag = diff < 0 ? -diff : diff;
  int nb = jenc_nbits(mag);
  if (nb > 11) return false;
  s.put(dc.code[nb], dc.len[nb]);
  if (nb) s.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u), nb);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = blk[ZZ ? k : kZigzagNat[k]];
    if (!v) { ++run; continue; }
    while (run > 15) { s.put(ac.code[0xF0], ac.len[0xF0]); run -= 16; }
    mag = v < 0 ? -v : v;
    nb = jenc_nbits(mag);
    if (nb > 10) return false;
    const int sym = (run << 4) | nb;
    s.put(ac.code[sym], ac.len[sym]);
    s.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u), nb);
    run = 0;
  }
  if (run) s.put(ac.code[0], ac.len[0]);
  return true;
}

// what both entropy forms ask of a file's frame before a byte is written
static int jenc_check(int h, int w, int hs, int vs, const uint16_t* qt3x64) {
  if (h <= 0 || w <= 0 || h > 65535 || w > 65535 || (hs != 1 && hs != 2) || (vs != 1 && vs != 2)) return fail(CTPN_ERR_ARG, "jpeg encode: bad size / sampling");
  for (int k = 0; k < 192; ++k) if (qt3x64[k] < 1 || qt3x64[k] > 255) return fail(CTPN_ERR_UNSUPPORTED, "jpeg encode: baseline files hold 8-bit quantisation values (1 .. 255)");
  if (std::memcmp(qt3x64 + 64, qt3x64 + 128, 64 * sizeof(uint16_t)) != 0) return fail(CTPN_ERR_UNSUPPORTED, "jpeg encode: the two chroma components share one quantisation table");
  return CTPN_OK;
}

// SOI .. SOS: kHeaderBytes bytes
static void jenc_header(JencSink& s, int h, int w, int hs, int vs, const uint16_t* qt3x64) {
  static const uint8_t kHead[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  s.raw(kHead, 20);
  for (int t = 0; t < 2; ++t) {
    s.byte(0xFF); s.byte(0xDB); s.u16(67); s.byte((uint8_t)t);
    for (int k = 0; k < 64; ++k) s.byte((uint8_t)qt3x64[64 * t + kZigzagNat[k]]);
  }
  s.byte(0xFF); s.byte(0xC0); s.u16(17); s.byte(8); s.u16(h); s.u16(w); s.byte(3);
  for (int c = 0; c < 3; ++c) { s.byte((uint8_t)(c + 1)); s.byte((uint8_t)(c ? 0x11 : (hs << 4) | vs)); s.byte((uint8_t)(c ? 1 : 0)); }
  for (int t = 0; t < 2; ++t) {
    s.byte(0xFF); s.byte(0xC4); s.u16(2 + 1 + 16 + 12); s.byte((uint8_t)t); s.raw(kBitsDc[t], 16); s.raw(kValsDc, 12);
    s.byte(0xFF); s.byte(0xC4); s.u16(2 + 1 + 16 + 162); s.byte((uint8_t)(0x10 | t)); s.raw(kBitsAc[t], 16); s.raw(kValsAc[t], 162);
  }
  static const uint8_t kSos[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  s.raw(kSos, 14);
}

// EOI, the file's size, and the verdict on the buffer
static int jenc_close(JencSink& s, size_t* bytes_out) {
  s.byte(0xFF); s.byte(0xD9);
  if (bytes_out) *bytes_out = s.n;
  if (s.n > s.cap) return fail(CTPN_ERR_CAPACITY, "jpeg encode: output buffer too small (" + std::to_string(s.n) + " bytes needed)");
  return CTPN_OK;
}

int jpeg_enc_check(int h, int w, int hs, int vs, const uint16_t* qt3x64) { return jenc_check(h, w, hs, vs, qt3x64); }

// the file around a scan body that is already coded and stuffed (the device-entropy form, jpeg_huff_enc.hip): of its scan_bytes bytes the
// first `have` are at `scan` -- all of them, or as many as the buffer can still take behind the header
int jpeg_enc_assemble(int h, int w, int hs, int vs, const uint16_t* qt3x64, const uint8_t* scan, size_t have, size_t scan_bytes, uint8_t* out, size_t capacity, size_t* bytes_out) {
  const int rc = jenc_check(h, w, hs, vs, qt3x64);
  if (rc) return rc;
  JencSink s{out, out ? capacity : 0};
  jenc_header(s, h, w, hs, vs, qt3x64);
  have = have < scan_bytes ? have : scan_bytes;
  const size_t room = s.cap > s.n ? s.cap - s.n : 0, put = have < room ? have : room;
  if (put) std::memcpy(s.out + s.n, scan, put);
  s.n += scan_bytes;
  return jenc_close(s, bytes_out);
}

// coef: [component][block rows][block columns][64] over the MCU grid, zig-zag (zigzag = true: what jpeg_fdct_kernel writes) or natural
// order (what ctpn_jpeg_entropy_decode returns); three components, luma sampling hs x vs, chroma 1 x 1; qt: 3 x 64, natural order.
// *bytes_out = the size of the file, also when it does not fit (CTPN_ERR_CAPACITY)
int jpeg_entropy_encode(const int16_t* coef, bool zigzag, int h, int w, int hs, int vs, const uint16_t* qt3x64, uint8_t* out, size_t capacity, size_t* bytes_out) {
  const int rc = jenc_check(h, w, hs, vs, qt3x64);
  if (rc) return rc;
  const JencTables& T = jenc_tables();
  JencSink s{out, out ? capacity : 0};
  jenc_header(s, h, w, hs, vs, qt3x64);
  const int mcux = (w + 8 * hs - 1) / (8 * hs), mcuy = (h + 8 * vs - 1) / (8 * vs);
  const int16_t* base[3]; int bw[3], ch[3], cv[3];
  {
    size_t off = 0;
    for (int c = 0; c < 3; ++c) { ch[c] = c ? 1 : hs; cv[c] = c ? 1 : vs; bw[c] = mcux * ch[c]; base[c] = coef + off; off += (size_t)mcuy * cv[c] * bw[c] * 64; }
  }
  int pred[3] = {0, 0, 0};
  bool ok = true;
  for (int my = 0; my < mcuy && ok; ++my)
    for (int mx = 0; mx < mcux && ok; ++mx)
      for (int c = 0; c < 3 && ok; ++c)
        for (int by = 0; by < cv[c] && ok; ++by)
          for (int bx = 0; bx < ch[c] && ok; ++bx) {
            const int16_t* blk = base[c] + ((size_t)(my * cv[c] + by) * bw[c] + (mx * ch[c] + bx)) * 64;
            ok = zigzag ? jenc_block<true>(s, blk, pred[c], T.dc[c ? 1 : 0], T.ac[c ? 1 : 0]) : jenc_block<false>(s, blk, pred[c], T.dc[c ? 1 : 0], T.ac[c ? 1 : 0]);
          }
  if (!ok) return fail(CTPN_ERR_ARG, "jpeg encode: a coefficient is outside what 8-bit baseline JPEG codes (DC difference 11 bits, AC 10 bits)");
  s.flush();
  return jenc_close(s, bytes_out);
}

// ---------------------------------------------------------------------------------------------
// device: pixels -> quantised coefficients. One workgroup = 8 MCUs of one MCU row (128 x 16 pixels).
//   stage 1  a thread takes 4 x 2 pixels: two runs of 12 bytes read as whole dwords (the run's address is rarely dword-aligned: three or
//            four aligned dwords, shifted), converted to Y / Cb / Cr; 8 luma samples and 2 + 2 downsampled chroma samples go to LDS. Pixels
//            right of / below the image repeat the last column / row (jcprepct.c / jcsample.c edge expansion, before the conversion here:
//            the conversion is per pixel, so the order does not matter)
//   stage 2  8 lanes per 8 x 8 block, a row each, then -- through LDS -- a column each (the IDCT kernel's pattern in reverse): 32 luma blocks
//            in the first round, 8 + 8 chroma blocks in the second; quantised, put into zig-zag order in LDS, stored as 16 bytes per lane
// ---------------------------------------------------------------------------------------------
__constant__ uint8_t d_jenc_zzpos[64] = CTPN_JENC_ZIGZAG_POS;

// One work item (jpeg_enc_mixed_dev.h): 8 MCUs `tile` of MCU row `my` of ONE h x w image whose first pixel is at img, rows `pitch` bytes
// apart; coef: the image's own coefficient block, bw / coef_off its components' block columns and offsets. The whole sequence -- load,
// colour conversion, downsampling, both DCT passes, quantiser, dummy blocks, store -- of both kernels below; every thread of the workgroup
// runs through all of its barriers.
__device__ __forceinline__ void jenc_fdct_item(const uint8_t* __restrict__ img, long long pitch, int h, int w, int16_t* __restrict__ coef, const int* __restrict__ bw,
                                               const long long* __restrict__ coef_off, const JencQ* __restrict__ qtab /* [2][64] */, int tile, int my) {
  __shared__ __attribute__((aligned(16))) uint8_t sY[16][128];
  __shared__ __attribute__((aligned(16))) uint8_t sC[2][8][64];
  __shared__ int ws[32][8][9];
  __shared__ __attribute__((aligned(16))) int16_t zq[32][64];
  __shared__ JencQ sq[2][64];
  const int tid = threadIdx.x;
  if (tid < 128) sq[tid >> 6][tid & 63] = qtab[tid];
  {
    const int gx = tid & 31, ry = tid >> 5;
    const int x0 = tile * 128 + gx * 4;
    // below the image the LUMA rows repeat the last pixel row, the CHROMA rows the last DOWNSAMPLED row (jcprepct.c pads the colour-converted
    // rows to one row group only, then expand_bottom_edge works on every component's own, downsampled, rows)
    const int cy = jenc_chroma_row(my * 8 + ry, h);
    int cb[2][4], cr[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      int y = my * 16 + ry * 2 + r, yc = 2 * cy + r;
      y = y < h ? y : h - 1;
      yc = yc < h ? yc : h - 1;
      uint32_t px[4];
      jenc_load4(img, pitch, y, x0, w, px);
      uint32_t yy = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int Y;
        jenc_ycc((int)(px[k] & 0xff), (int)((px[k] >> 8) & 0xff), (int)(px[k] >> 16), Y, cb[r][k], cr[r][k]);
        yy |= (uint32_t)Y << (8 * k);
      }
      *(uint32_t*)&sY[ry * 2 + r][gx * 4] = yy;
      if (yc != y) {      // (the rows below the image only)
        jenc_load4(img, pitch, yc, x0, w, px);
#pragma unroll
        for (int k = 0; k < 4; ++k) { int Y; jenc_ycc((int)(px[k] & 0xff), (int)((px[k] >> 8) & 0xff), (int)(px[k] >> 16), Y, cb[r][k], cr[r][k]); }
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {      // output columns tile * 64 + gx * 2 + j: the bias alternates with j
      sC[0][ry][gx * 2 + j] = (uint8_t)jenc_h2v2(cb[0][2 * j], cb[0][2 * j + 1], cb[1][2 * j], cb[1][2 * j + 1], j);
      sC[1][ry][gx * 2 + j] = (uint8_t)jenc_h2v2(cr[0][2 * j], cr[0][2 * j + 1], cr[1][2 * j], cr[1][2 * j + 1], j);
    }
  }
  __syncthreads();
  const int lb = tid >> 3, t = tid & 7;
  const int real_bw0 = (w + 7) >> 3, real_bh0 = (h + 7) >> 3;
#pragma unroll 1
  for (int it = 0; it < 2; ++it) {
    const bool active = it == 0 || lb < 16;
    const int c = it == 0 ? 0 : (lb < 8 ? 1 : 2);
    const int by = c == 0 ? lb >> 4 : 0, bx = c == 0 ? lb & 15 : lb & 7;
    int x[8], o[8];
    if (active) {
      const uint2 v = c == 0 ? *(const uint2*)&sY[by * 8 + t][bx * 8] : *(const uint2*)&sC[c - 1][t][bx * 8];
#pragma unroll
      for (int k = 0; k < 4; ++k) { x[k] = (int)((v.x >> (8 * k)) & 0xff) - 128; x[k + 4] = (int)((v.y >> (8 * k)) & 0xff) - 128; }
      jfdct_1d(x, o, true);
#pragma unroll
      for (int k = 0; k < 8; ++k) ws[lb][t][k] = o[k];
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int k = 0; k < 8; ++k) x[k] = ws[lb][k][t];
      jfdct_1d(x, o, false);
#pragma unroll
      for (int k = 0; k < 8; ++k) zq[lb][d_jenc_zzpos[8 * k + t]] = (int16_t)jenc_quant(o[k], sq[c ? 1 : 0][8 * k + t]);
    }
    __syncthreads();
    if (active) {
      const int bxg = (c == 0 ? tile * 16 : tile * 8) + bx, byg = (c == 0 ? my * 2 : my) + by;
      if (bxg < bw[c]) {
        uint4 v = *(const uint4*)&zq[lb][t * 8];
        if (c == 0) {
          const int s = jenc_dummy_src(by, bx & 1, (bxg | 1) >= real_bw0, my * 2 + 1 >= real_bh0);
          if (s >= 0) {
            v = make_uint4(0, 0, 0, 0);
            if (t == 0) v.x = (uint32_t)(uint16_t)zq[(s >> 1) * 16 + (bx & ~1) + (s & 1)][0];
          }
        }
        *(uint4*)(coef + coef_off[c] + ((long long)byg * bw[c] + bxg) * 64 + t * 8) = v;
      }
    }
    __syncthreads();
  }
}

// n images of one size, tightly packed: grid (tiles, MCU rows, n), one JpegGeom for the batch
__global__ __launch_bounds__(256) void jpeg_fdct_kernel(const uint8_t* __restrict__ img, int16_t* __restrict__ coef, const JencQ* __restrict__ qtab /* [2][64] */, JpegGeom g) {
  const int im = blockIdx.z;
  jenc_fdct_item(img + (long long)im * g.h * g.w * 3, (long long)g.w * 3, g.h, g.w, coef + (long long)im * g.coef_per_img, g.bw, g.coef_off, qtab, (int)blockIdx.x, (int)blockIdx.y);
}

// n images of any mix of sizes and pitches in one source buffer: a one-dimensional grid over the table's work items, the image of a
// workgroup found in the items' prefix (uniform over the workgroup: no thread leaves in front of a barrier)
__global__ __launch_bounds__(256) void jpeg_fdct_mixed_kernel(const uint8_t* __restrict__ src, int16_t* __restrict__ coef, const JencQ* __restrict__ qtab /* [2][64] */,
                                                              const JemImage* __restrict__ tab, int n) {
  const JemItem p = jem_locate(tab, n, (long long)blockIdx.x);
  const JemImage& d = tab[p.img];
  jenc_fdct_item(src + d.src_off, d.pitch, d.h, d.w, coef + d.coef_base, d.bw, d.coef_off, qtab, p.tile, p.my);
}

// ctpn_draw_boxes (text_connector.cpp) on n device images: one workgroup per image; lines, and the four segments of a line, in the host
// function's order, the samples of a segment spread over the lanes. Later lines overwrite earlier ones, so a barrier stands wherever the
// colour changes (segments of one colour write the same bytes, in whatever order). The sample positions are the host's doubles: this unit
// is compiled without FMA contraction, like text_connector.cpp.
// The body, for ONE h x w image at img with its lines at rr: both kernels below run it, every thread of the workgroup through all of its barriers
__device__ __forceinline__ void draw_boxes_image(uint8_t* __restrict__ img, const double* __restrict__ rr, int n_lines, int h, int w) {
  int last_green = -1;
  for (int li = 0; li < n_lines; ++li) {
    const double* b = rr + (long long)li * 9;
    if (fabs(b[0] - b[1]) < 5.0 || fabs(b[3] - b[0]) < 5.0) continue;
    bool sane = true;
    for (int k = 0; k < 8; ++k) sane = sane && isfinite(b[k]) && fabs(b[k]) < 1e12;
    if (!sane) continue;
    const int green = b[8] >= 0.9 ? 1 : 0;
    if (last_green >= 0 && green != last_green) { __threadfence_block(); __syncthreads(); }
    last_green = green;
    const uint8_t c0 = green ? 0 : 255, c1 = green ? 255 : 0;
    const long long px[4] = {(long long)b[0], (long long)b[2], (long long)b[6], (long long)b[4]};
    const long long py[4] = {(long long)b[1], (long long)b[3], (long long)b[7], (long long)b[5]};
    for (int k = 0; k < 4; ++k) {
      const long long x0 = px[k], y0 = py[k], x1 = px[(k + 1) & 3], y1 = py[(k + 1) & 3];
      const long long dxa = x1 > x0 ? x1 - x0 : x0 - x1, dya = y1 > y0 ? y1 - y0 : y0 - y1;
      const long long n = (dxa > dya ? dxa : dya) + 1;
      // the samples that can touch the image, as the host function bounds them (every pixel is still tested against the image)
      long long lo = 0, hi = n - 1;
      for (int ax = 0; ax < 2; ++ax) {
        const long long a = ax ? y0 : x0, e = ax ? y1 : x1, size = ax ? h : w;
        if (n <= 1 || a == e) { if (a < -2 || a > size + 1) hi = -1; continue; }
        const double step = ((double)e - (double)a) / (double)(n - 1);
        double t0 = (-2.0 - (double)a) / step, t1 = ((double)size + 1.0 - (double)a) / step;
        if (t0 > t1) { const double tt = t0; t0 = t1; t1 = tt; }
        if (t1 < 0.0 || t0 > (double)(n - 1)) { hi = -1; continue; }
        const long long l2 = (long long)floor(t0 > 0.0 ? t0 : 0.0) - 2, h2 = (long long)ceil(t1 < (double)(n - 1) ? t1 : (double)(n - 1)) + 2;
        lo = lo > l2 ? lo : l2;
        hi = hi < h2 ? hi : h2;
      }
      lo = lo > 0 ? lo : 0;
      hi = hi < n - 1 ? hi : n - 1;
      const double sx = n > 1 ? ((double)x1 - (double)x0) / (double)(n - 1) : 0.0, sy = n > 1 ? ((double)y1 - (double)y0) / (double)(n - 1) : 0.0;
      for (long long i = lo + threadIdx.x; i <= hi; i += blockDim.x) {
        const double fx = (n > 1 && i == n - 1) ? (double)x1 : (double)x0 + (double)i * sx;
        const double fy = (n > 1 && i == n - 1) ? (double)y1 : (double)y0 + (double)i * sy;
        const long long cx = (long long)rint(fx), cy = (long long)rint(fy);
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const long long yy = cy + dy, xx = cx + dx;
            if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
            uint8_t* p = img + ((long long)yy * w + xx) * 3;
            p[0] = c0; p[1] = c1; p[2] = 0;
          }
      }
    }
  }
}

// n images of one size, tightly packed
__global__ __launch_bounds__(256) void draw_boxes_kernel(uint8_t* __restrict__ imgs, const double* __restrict__ recs, const int* __restrict__ counts, int line_capacity, int h, int w) {
  const int n_lines = counts[blockIdx.x];
  draw_boxes_image(imgs + (long long)blockIdx.x * h * w * 3, recs + (long long)blockIdx.x * line_capacity * 9, n_lines < line_capacity ? n_lines : line_capacity, h, w);
}

// the slots of a ragged canvas n x hc x w x 3: image i is rows [0, heights[i]) of slot i. Row bounds and the clipping of the sample ranges
// take the image's own height (clamped to the slot's), so nothing is drawn into the rows below an image
__global__ __launch_bounds__(256) void draw_boxes_ragged_kernel(uint8_t* __restrict__ canvas, const double* __restrict__ recs, const int* __restrict__ counts,
                                                                const int* __restrict__ heights, int line_capacity, int hc, int w) {
  const int n_lines = counts[blockIdx.x], hi = heights[blockIdx.x];
  const int h = hi < 0 ? 0 : (hi < hc ? hi : hc);
  draw_boxes_image(canvas + (long long)blockIdx.x * hc * w * 3, recs + (long long)blockIdx.x * line_capacity * 9, n_lines < line_capacity ? n_lines : line_capacity, h, w);
}

int launch_jpeg_fdct(const uint8_t* img_dev, int16_t* coef_dev, const JencQ* qtab_dev, const JpegGeom& g, int n, hipStream_t s) {
  const int mcux = g.bw[1], mcuy = g.bh[1];
  if (n <= 0 || n > 65535 || mcuy > 65535 || mcux <= 0) return fail(CTPN_ERR_ARG, "jpeg encode: grid out of range");
  hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((unsigned)((mcux + 7) / 8), (unsigned)mcuy, (unsigned)n), dim3(256), 0, s, img_dev, coef_dev, qtab_dev, g);
  return launch_status("jpeg encode");
}

// tab_dev: n descriptors with their prefix sums (jem_prefix), total_items work items in all
int launch_jpeg_fdct_mixed(const uint8_t* src_dev, int16_t* coef_dev, const JencQ* qtab_dev, const JemImage* tab_dev, int n, long long total_items, hipStream_t s) {
  if (n <= 0 || total_items < n || total_items > JEM_MAX_ITEMS) return fail(CTPN_ERR_ARG, "jpeg encode: grid out of range");
  hipLaunchKernelGGL(jpeg_fdct_mixed_kernel, dim3((unsigned)total_items), dim3(256), 0, s, src_dev, coef_dev, qtab_dev, tab_dev, n);
  return launch_status("jpeg encode (mixed sizes)");
}

int launch_draw_boxes(uint8_t* imgs_dev, const double* recs_dev, const int* counts_dev, int line_capacity, int n, int h, int w, hipStream_t s) {
  if (n <= 0) return fail(CTPN_ERR_ARG, "draw_boxes: empty batch");
  hipLaunchKernelGGL(draw_boxes_kernel, dim3((unsigned)n), dim3(256), 0, s, imgs_dev, recs_dev, counts_dev, line_capacity, h, w);
  return launch_status("draw_boxes");
}

int launch_draw_boxes_ragged(uint8_t* canvas_dev, const double* recs_dev, const int* counts_dev, const int* heights_dev, int line_capacity, int n, int hc, int w, hipStream_t s) {
  if (n <= 0 || hc <= 0 || w <= 0 || !heights_dev) return fail(CTPN_ERR_ARG, "draw_boxes: empty batch");
  hipLaunchKernelGGL(draw_boxes_ragged_kernel, dim3((unsigned)n), dim3(256), 0, s, canvas_dev, recs_dev, counts_dev, heights_dev, line_capacity, hc, w);
  return launch_status("draw_boxes (ragged)");
}

}  // namespace ctpn
