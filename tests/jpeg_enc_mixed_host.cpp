// Host harness of the JPEG writer's mixed-size pixel half (csrc/jpeg_enc.hip: jpeg_fdct_mixed_kernel): compiles the text the kernel shares
// with the host -- csrc/jpeg_enc_mixed_dev.h (descriptors, work-item prefix and search, jenc_load4) and csrc/jpeg_enc_pixel.h (the
// arithmetic) -- with g++ under AddressSanitizer + UBSan and runs one call's table the way the kernel runs it: a loop over the work items
// (the grid), the image of an item found by jem_locate, then the body's stages as loops over a workgroup's threads (the barriers are the
// ends of those loops), shaped like tests/jpeg_enc_host.cpp.
//   jpeg_enc_mixed_host <batch.bin> <coef.out>
// batch.bin: int32 n; uint16 q[2][64] (natural order); per image int32 h, w and its h x w x 3 BGR bytes, tightly packed.
// coef.out: int64 count, then the call's int16 coefficients (zig-zag order), image i at the prefix sum of the images' own counts.
// The SOURCE of every image is a heap block of its own of exactly (h - 1) * pitch + 3 w bytes at pitch 3 * 512, rows 4-byte aligned, the
// bytes between a row's end and the next row filled with 0xA5 -- a read outside an image's pixels that leaves the block is ASan's, and one
// that stays inside reads padding, which the second run (padding 0x5A) shows in the coefficients. The table addresses the blocks through
// one base pointer (the lowest block) and byte offsets, as the kernel does. The coefficient buffer is exactly as large as the table says.
// Checked here: every work item maps back to its (image, MCU row, tile); every coefficient offset lies inside its image's block and every
// coefficient is written exactly once; jenc_load4 over unaligned, tightly packed rows (three bytes of slack: its documented contract) equals
// a byte-by-byte read. The test compares the files the coefficients lead to with Pillow's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../text-detection-ctpn_amd/csrc/jpeg_enc_mixed_dev.h"

using namespace ctpn;

static const int kPitch = 3 * 512;
static bool rd(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "jpeg_enc_mixed_host: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

struct Source { uint8_t* mem; size_t bytes; };

// one work item: jenc_fdct_item's stages
static int run_item(const uint8_t* img, long long pitch, int h, int w, const JemImage& d, const JencQ (&sq)[2][64], int tile, int my, int16_t* coef, long long coef_total,
                    std::vector<uint8_t>& written) {
  static const uint8_t zzpos[64] = CTPN_JENC_ZIGZAG_POS;
  uint8_t sY[16][128], sC[2][8][64];
  for (int tid = 0; tid < 256; ++tid) {                      // stage 1
    const int gx = tid & 31, ry = tid >> 5, x0 = tile * 128 + gx * 4;
    const int cy = jenc_chroma_row(my * 8 + ry, h);
    int cb[2][4], cr[2][4];
    for (int r = 0; r < 2; ++r) {
      int y = my * 16 + ry * 2 + r, yc = 2 * cy + r;
      y = y < h ? y : h - 1;
      yc = yc < h ? yc : h - 1;
      uint32_t px[4];
      jenc_load4(img, pitch, y, x0, w, px);
      for (int k = 0; k < 4; ++k) {
        int Y;
        jenc_ycc((int)(px[k] & 0xff), (int)((px[k] >> 8) & 0xff), (int)(px[k] >> 16), Y, cb[r][k], cr[r][k]);
        sY[ry * 2 + r][gx * 4 + k] = (uint8_t)Y;
      }
      if (yc != y) {
        jenc_load4(img, pitch, yc, x0, w, px);
        for (int k = 0; k < 4; ++k) { int Y; jenc_ycc((int)(px[k] & 0xff), (int)((px[k] >> 8) & 0xff), (int)(px[k] >> 16), Y, cb[r][k], cr[r][k]); }
      }
    }
    for (int j = 0; j < 2; ++j) {
      sC[0][ry][gx * 2 + j] = (uint8_t)jenc_h2v2(cb[0][2 * j], cb[0][2 * j + 1], cb[1][2 * j], cb[1][2 * j + 1], j);
      sC[1][ry][gx * 2 + j] = (uint8_t)jenc_h2v2(cr[0][2 * j], cr[0][2 * j + 1], cr[1][2 * j], cr[1][2 * j + 1], j);
    }
  }
  const int real_bw0 = (w + 7) >> 3, real_bh0 = (h + 7) >> 3;
  for (int it = 0; it < 2; ++it) {                           // stage 2
    int16_t zq[32][64];
    const int nb = it == 0 ? 32 : 16;
    for (int lb = 0; lb < nb; ++lb) {
      const int c = it == 0 ? 0 : (lb < 8 ? 1 : 2);
      const int by = c == 0 ? lb >> 4 : 0, bx = c == 0 ? lb & 15 : lb & 7;
      int ws[8][8], x[8], o[8];
      for (int t = 0; t < 8; ++t) {
        const uint8_t* src = c == 0 ? &sY[by * 8 + t][bx * 8] : &sC[c - 1][t][bx * 8];
        for (int k = 0; k < 8; ++k) x[k] = (int)src[k] - 128;
        jfdct_1d(x, o, true);
        for (int k = 0; k < 8; ++k) ws[t][k] = o[k];
      }
      for (int t = 0; t < 8; ++t) {
        for (int k = 0; k < 8; ++k) x[k] = ws[k][t];
        jfdct_1d(x, o, false);
        for (int k = 0; k < 8; ++k) zq[lb][zzpos[8 * k + t]] = (int16_t)jenc_quant(o[k], sq[c ? 1 : 0][8 * k + t]);
      }
    }
    for (int lb = 0; lb < nb; ++lb) {
      const int c = it == 0 ? 0 : (lb < 8 ? 1 : 2);
      const int by = c == 0 ? lb >> 4 : 0, bx = c == 0 ? lb & 15 : lb & 7;
      const int bxg = (c == 0 ? tile * 16 : tile * 8) + bx, byg = (c == 0 ? my * 2 : my) + by;
      if (bxg >= d.bw[c]) continue;
      const long long in_img = d.coef_off[c] + ((long long)byg * d.bw[c] + bxg) * 64;
      CHECK(in_img >= 0 && in_img + 64 <= jem_coef_count(d), "a coefficient offset leaves its image's block (component %d, block %d, %d)", c, byg, bxg);
      const long long at = d.coef_base + in_img;
      CHECK(at >= 0 && at + 64 <= coef_total, "a coefficient offset leaves the call's buffer");
      int16_t* dst = coef + at;
      memcpy(dst, zq[lb], 64 * sizeof(int16_t));
      if (c == 0) {
        const int s = jenc_dummy_src(by, bx & 1, (bxg | 1) >= real_bw0, my * 2 + 1 >= real_bh0);
        if (s >= 0) { memset(dst, 0, 64 * sizeof(int16_t)); dst[0] = zq[(s >> 1) * 16 + (bx & ~1) + (s & 1)][0]; }
      }
      for (int k = 0; k < 64; ++k) ++written[(size_t)at + k];
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: jpeg_enc_mixed_host batch.bin coef.out\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int n;
  uint16_t q[128];
  if (!rd(f, &n, 4) || n <= 0 || !rd(f, q, sizeof(q))) return 2;
  JencQ sq[2][64];
  for (int c = 0; c < 2; ++c)
    for (int k = 0; k < 64; ++k) { sq[c][k].magic = jenc_magic(q[64 * c + k]); sq[c][k].half = 4u * q[64 * c + k]; }
  std::vector<int> hs((size_t)n), wsz((size_t)n);
  std::vector<std::vector<uint8_t>> tight((size_t)n);
  for (int i = 0; i < n; ++i) {
    int hw[2];
    if (!rd(f, hw, 8) || hw[0] < 1 || hw[1] < 1 || hw[1] > 512) return 2;
    hs[i] = hw[0]; wsz[i] = hw[1];
    tight[i].resize((size_t)hw[0] * hw[1] * 3);
    if (!rd(f, tight[i].data(), tight[i].size())) return 2;
  }
  fclose(f);

  // jenc_load4 on unaligned rows: tightly packed copies with the three bytes of slack the contract asks for, against a byte-by-byte read
  for (int i = 0; i < n; ++i) {
    const int h = hs[i], w = wsz[i];
    std::vector<uint8_t> buf(tight[i].size() + 3);
    buf.shrink_to_fit();
    memcpy(buf.data(), tight[i].data(), tight[i].size());
    for (int y = 0; y < h; ++y)
      for (int x0 = 0; x0 < ((w + 127) / 128) * 128; x0 += 4) {
        uint32_t px[4];
        jenc_load4(buf.data(), (long long)w * 3, y, x0, w, px);
        for (int k = 0; k < 4; ++k) {
          const int x = x0 + k < w ? x0 + k : w - 1;
          const uint8_t* p = tight[i].data() + ((size_t)y * w + x) * 3;
          CHECK(px[k] == ((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16)), "jenc_load4 differs at image %d, row %d, column %d", i, y, x0 + k);
        }
      }
  }

  // the source blocks, exactly sized
  std::vector<Source> src((size_t)n);
  uintptr_t lowest = ~(uintptr_t)0;
  for (int i = 0; i < n; ++i) {
    src[i].bytes = (size_t)(hs[i] - 1) * kPitch + (size_t)wsz[i] * 3;
    src[i].mem = (uint8_t*)malloc(src[i].bytes);
    CHECK(src[i].mem && ((uintptr_t)src[i].mem & 3) == 0, "no aligned block");
    if ((uintptr_t)src[i].mem < lowest) lowest = (uintptr_t)src[i].mem;
  }
  const uint8_t* base = (const uint8_t*)lowest;

  // the table, as the host pipeline builds it
  std::vector<JemImage> tab((size_t)n);
  for (int i = 0; i < n; ++i) jem_describe(tab[i], hs[i], wsz[i], kPitch, (long long)((uintptr_t)src[i].mem - lowest));
  long long coef_total = 0;
  const long long items = jem_prefix(tab.data(), n, &coef_total);
  CHECK(items >= n, "no work items");
  tab.shrink_to_fit();

  // the descriptors against the definition of the geometry, and every work item against the enumeration
  long long item = 0, coef_at = 0;
  for (int i = 0; i < n; ++i) {
    const int mcux = (wsz[i] + 15) / 16, mcuy = (hs[i] + 15) / 16, tiles = (mcux + 7) / 8;
    const JemImage& d = tab[i];
    CHECK(d.bw[0] == 2 * mcux && d.bw[1] == mcux && d.bw[2] == mcux && d.bh[0] == 2 * mcuy && d.bh[1] == mcuy && d.bh[2] == mcuy, "block grid of image %d", i);
    CHECK(d.coef_off[0] == 0 && d.coef_off[1] == 256LL * mcux * mcuy && d.coef_off[2] == 320LL * mcux * mcuy && jem_coef_count(d) == 384LL * mcux * mcuy, "coefficient offsets of image %d", i);
    CHECK(d.item0 == item && d.coef_base == coef_at, "prefix sums of image %d", i);
    for (int my = 0; my < mcuy; ++my)
      for (int tile = 0; tile < tiles; ++tile, ++item) {
        const JemItem p = jem_locate(tab.data(), n, item);
        CHECK(p.img == i && p.my == my && p.tile == tile, "work item %lld maps to (%d, %d, %d), not (%d, %d, %d)", item, p.img, p.my, p.tile, i, my, tile);
      }
    coef_at += 384LL * mcux * mcuy;
  }
  CHECK(item == items && coef_at == coef_total, "totals");

  std::vector<int16_t> coef[2];
  for (int run = 0; run < 2; ++run) {
    const uint8_t fill = run == 0 ? 0xA5 : 0x5A;
    for (int i = 0; i < n; ++i) {
      memset(src[i].mem, fill, src[i].bytes);
      for (int y = 0; y < hs[i]; ++y) memcpy(src[i].mem + (size_t)y * kPitch, tight[i].data() + (size_t)y * wsz[i] * 3, (size_t)wsz[i] * 3);
    }
    coef[run].assign((size_t)coef_total, 0x7777);
    coef[run].shrink_to_fit();
    std::vector<uint8_t> written((size_t)coef_total, 0);
    for (long long it = 0; it < items; ++it) {      // the grid
      const JemItem p = jem_locate(tab.data(), n, it);
      const JemImage& d = tab[p.img];
      if (int rc = run_item(base + d.src_off, d.pitch, d.h, d.w, d, sq, p.tile, p.my, coef[run].data(), coef_total, written)) return rc;
    }
    for (long long k = 0; k < coef_total; ++k) CHECK(written[(size_t)k] == 1, "coefficient %lld was written %d times", k, (int)written[(size_t)k]);
  }
  CHECK(coef[0] == coef[1], "the padding bytes changed the coefficients");

  f = fopen(argv[2], "wb");
  const long long cnt = coef_total;
  if (!f || fwrite(&cnt, 8, 1, f) != 1 || fwrite(coef[0].data(), 2, (size_t)cnt, f) != (size_t)cnt) return 2;
  fclose(f);
  for (int i = 0; i < n; ++i) free(src[i].mem);
  printf("images %d work items %lld coefficients %lld ok\n", n, items, coef_total);
  return 0;
}
