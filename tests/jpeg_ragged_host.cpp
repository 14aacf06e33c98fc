// Host harness of the ragged JPEG pixel kernels (csrc/jpeg_ragged.hip): compiles their per-thread source, csrc/jpeg_ragged_dev.h, with g++
// under AddressSanitizer + UBSan and runs both kernels as loops over workgroup and thread indices, shaped like the kernels' own bodies (the
// IDCT's barrier is the end of the first loop over a workgroup's threads).
//   jpeg_ragged_host <batch.bin> <canvas.out>
// batch.bin: int32 n, hc, wc; then per file int32 layout8[8] (as ctpn_jpeg_entropy_decode fills it), double factor, int32 coefficient count,
// uint16 qt[192], int16 coefficients. canvas.out: int32 heights[n], then the n x hc x wc x 3 canvas bytes. The test compares them with
// Pillow's decode resized by oracle/resize_ref.py. Every buffer is exactly as large as the kernels may touch: a byte further is ASan's.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../text-detection-ctpn_amd/csrc/jpeg_ragged_dev.h"

using namespace ctpn;

static bool rd(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: jpeg_ragged_host batch.bin canvas.out\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int hdr[3];
  if (!rd(f, hdr, sizeof(hdr))) return 2;
  const int n = hdr[0], hc = hdr[1], wc = hdr[2];
  std::vector<JrImage> tab((size_t)n);
  std::vector<int16_t> coef;
  std::vector<uint16_t> qt((size_t)n * 192);
  std::vector<int> heights((size_t)n);
  long long blocks = 0;
  for (int i = 0; i < n; ++i) {
    int l8[8], cnt;
    double factor;
    if (!rd(f, l8, sizeof(l8)) || !rd(f, &factor, 8) || !rd(f, &cnt, 4) || !rd(f, qt.data() + (size_t)i * 192, 384)) return 2;
    JrImage& d = tab[i];
    memset(&d, 0, sizeof(d));
    JpegGeom& g = d.g;
    g.h = l8[0]; g.w = l8[1]; g.ncomp = l8[2]; g.hs0 = l8[3] & 0xff;
    g.orient = (l8[3] >> 8) + 1; g.oh = g.orient >= 5 ? g.w : g.h; g.ow = g.orient >= 5 ? g.h : g.w;
    long long co = 0;
    for (int c = 0; c < g.ncomp; ++c) {
      g.bw[c] = l8[c == 0 ? 4 : 5]; g.bh[c] = l8[c == 0 ? 6 : 7];
      g.coef_off[c] = g.plane_off[c] = co;
      co += (long long)g.bw[c] * g.bh[c] * 64;
      g.blocks_per_img += (long long)g.bw[c] * g.bh[c];
    }
    g.vs0 = g.ncomp == 3 ? g.bh[0] / g.bh[1] : 1;
    g.coef_per_img = g.plane_per_img = co;
    if (co != cnt) { fprintf(stderr, "file %d: %d coefficients for a layout of %lld\n", i, cnt, co); return 2; }
    d.coef_base = d.plane_base = (long long)coef.size();      // packed: the next file starts where this one ends
    d.block0 = blocks;
    blocks += g.blocks_per_img;
    d.resize = factor != 1.0;
    d.inv_f = 1.0 / factor;
    d.height = d.resize ? (int)std::nearbyint((double)g.oh * factor) : g.oh;
    const int width = d.resize ? (int)std::nearbyint((double)g.ow * factor) : g.ow;
    if (width != wc || d.height > hc) { fprintf(stderr, "file %d maps to %d x %d, canvas %d x %d\n", i, d.height, width, hc, wc); return 2; }
    heights[i] = d.height;
    coef.resize(coef.size() + (size_t)cnt);
    if (!rd(f, coef.data() + d.coef_base, (size_t)cnt * 2)) return 2;
  }
  fclose(f);
  const size_t plane_bytes = coef.size(), canvas_bytes = (size_t)n * hc * wc * 3;
  void* mem = nullptr;
  if (posix_memalign(&mem, 8, plane_bytes)) return 2;
  uint8_t* planes = (uint8_t*)mem;
  memset(planes, 0xAA, plane_bytes);
  uint8_t* canvas = (uint8_t*)malloc(canvas_bytes);
  if (!canvas) return 2;
  memset(canvas, 0x55, canvas_bytes);      // every byte must be written, the zeros below the images included
  // exact-size copies of what the kernels only read
  std::vector<int16_t> coef_exact(coef);
  coef_exact.shrink_to_fit();

  // jpeg_idct_ragged_kernel
  const long long wgs = (blocks + JR_BLOCKS_PER_WG - 1) / JR_BLOCKS_PER_WG;
  long long straddling = 0;
  for (long long bx = 0; bx < wgs; ++bx) {
    static int ws[JR_BLOCKS_PER_WG][8][9];
    JrBlockPos pos[256];
    static int col[256][8];
    int ac[JR_BLOCKS_PER_WG] = {0};
    for (int tid = 0; tid < 256; ++tid) {      // the loads, and each block's flag from its eight columns (the kernel's shuffles)
      pos[tid] = jr_block_locate(tab.data(), n, blocks, bx * JR_BLOCKS_PER_WG + (tid >> 3));
      ac[tid >> 3] |= jr_idct_load(tab.data(), coef_exact.data(), qt.data(), pos[tid], tid & 7, col[tid]);
    }
    for (int tid = 0; tid < 256; ++tid) {
      const int lb = tid >> 3, t = tid & 7;
      int o[8];
      jidct_pass1(col[tid], ac[lb], o);
      for (int k = 0; k < 8; ++k) ws[lb][k][t] = o[k];
    }
    if (pos[0].live && pos[255].live && pos[0].img != pos[255].img) ++straddling;
    for (int tid = 0; tid < 256; ++tid) {      // behind the barrier
      const int lb = tid >> 3, t = tid & 7;
      int x[8];
      for (int k = 0; k < 8; ++k) x[k] = ws[lb][t][k];
      jr_idct_pass2(tab.data(), planes, pos[tid], t, x);
    }
  }
  // jpeg_color_resize_ragged_kernel
  const long long groups = ((long long)n * hc * wc + 3) / 4, cwgs = (groups + 255) / 256;
  for (long long bx = 0; bx < cwgs; ++bx)
    for (int tid = 0; tid < 256; ++tid) jr_color_resize_thread(planes, canvas, tab.data(), n, hc, wc, bx * 256 + tid);

  f = fopen(argv[2], "wb");
  if (!f || fwrite(heights.data(), 4, (size_t)n, f) != (size_t)n || fwrite(canvas, 1, canvas_bytes, f) != canvas_bytes) return 2;
  fclose(f);
  free(canvas);
  free(planes);
  printf("images %d blocks %lld idct workgroups %lld straddling %lld colour workgroups %lld ok\n", n, blocks, wgs, straddling, cwgs);
  return 0;
}
