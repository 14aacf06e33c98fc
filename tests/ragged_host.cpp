// Host harness of the ragged-batch kernels (csrc/ragged.hip): compiles their per-thread source, csrc/ragged_dev.h, with g++ under
// AddressSanitizer + UBSan and runs both kernels as loops over workgroup and thread indices, shaped like the kernels' own bodies.
//   ragged_host <canvas.bin> <blob.out>
// canvas.bin: int32 n, hc, w, heights[n], then n x hc x w x 3 bytes; blob.out: the n x hc x w x 3 floats ragged_blob_thread writes (the test
// compares their bits with numpy's). The mask cases are generated and checked here, byte by byte, against the definition restated
// without ragged_dev.h's index functions: exactly the interior rows >= height >> level of every image are zero, every other byte -- frames,
// the bytes in front of the buffer, the rows above -- is the pattern it was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../text-detection-ctpn_amd/csrc/ragged_dev.h"

using namespace ctpn;

static unsigned char pattern(size_t i) { return (unsigned char)(1 + (i * 2654435761u >> 7) % 255); }      // never 0

// the kernel's body for workgroup (bx, img), every thread
static void mask_workgroup(unsigned char* base, const RaggedMap& m, const int* heights, long long bx, int img) {
  const int valid = ragged_valid_rows(heights[img], m.level);
  if (bx >= ragged_mask_wgs(m, valid)) return;
  const int per_row = ragged_wgs_per_row(m.span_bytes);
  const int row = valid + (int)(bx / per_row), k0 = (int)(bx % per_row) * RG_PER_WG;
  for (int tid = 0; tid < 256; ++tid)
    for (int j = 0; j < RG_PER_WG / 256; ++j) ragged_mask_thread(m, base, img, row, k0 + j * 256 + tid);
}

// one bordered map: n images of rows x wl pixels of pix bytes behind a frame of `top` rows and `left` pixels (right frame: fr pixels, bottom: top rows)
static int mask_case(int pix, int wl, int rows, int level, const std::vector<int>& heights, int top, int left_px, int right_px, int front) {
  const int n = (int)heights.size();
  RaggedMap m;
  m.row_bytes = (long long)(left_px + wl + right_px) * pix;
  m.img_bytes = (long long)(rows + 2 * top) * m.row_bytes;
  m.top = top; m.left_bytes = left_px * pix; m.span_bytes = wl * pix; m.rows = rows; m.level = level;
  const size_t bytes = (size_t)n * m.img_bytes;
  std::vector<unsigned char> store(front + bytes);      // the map ends where the allocation ends: a store past it is ASan's
  unsigned char* base = store.data() + front;
  for (size_t i = 0; i < store.size(); ++i) store[i] = pattern(i);
  int pad = 0;
  for (int i = 0; i < n; ++i) pad = rows - (heights[i] >> level) > pad ? rows - (heights[i] >> level) : pad;
  const long long gx = (long long)pad * ragged_wgs_per_row(m.span_bytes);
  for (int img = 0; img < n; ++img)
    for (long long bx = 0; bx < gx; ++bx) mask_workgroup(base, m, heights.data(), bx, img);
  long long cleared = 0;
  for (size_t i = 0; i < store.size(); ++i) {
    bool zero = false;
    if (i >= (size_t)front) {
      const size_t o = i - front;
      const int img = (int)(o / m.img_bytes);
      const size_t in_img = o % m.img_bytes;
      const int row = (int)(in_img / m.row_bytes) - top;
      const long long col = (long long)(in_img % m.row_bytes) - m.left_bytes;
      zero = row >= (heights[img] >> level) && row < rows && col >= 0 && col < m.span_bytes;
    }
    if (store[i] != (zero ? 0 : pattern(i))) {
      fprintf(stderr, "mask case pix %d wl %d rows %d level %d top %d front %d: byte %zu is %d, want %d\n", pix, wl, rows, level, top, front, i, store[i], zero ? 0 : pattern(i));
      return 1;
    }
    cleared += zero;
  }
  printf("mask pix %d wl %d rows %d level %d top %d front %d cleared %lld\n", pix, wl, rows, level, top, front, cleared);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: ragged_host canvas.bin blob.out\n"); return 2; }
  // valid rows per level
  for (int h = 0; h <= 1300; ++h)
    for (int l = 0; l <= 4; ++l) {
      int v = h;
      for (int k = 0; k < l; ++k) v /= 2;
      if (ragged_valid_rows(h, l) != v) { fprintf(stderr, "valid rows %d level %d\n", h, l); return 1; }
    }
  int cases = 0;
  const std::vector<int> hts = {96, 80, 49, 16, 33};      // canvas 96: image 0 has nothing to clear; 16 >> 4 = 1, 16 rows at level 4 of 6
  for (int pix : {2, 4, 8, 12})
    for (int wl : {1, 5, 8, 41, 82})
      for (int level = 0; level <= 4; ++level)
        for (int front : {0, 2, 6}) {
          if (mask_case(pix, wl, 96 >> level, level, hts, 1, 1, 1, front)) return 1;
          ++cases;
        }
  // heights all equal to the canvas: nothing is written, no workgroup runs
  if (mask_case(4, 7, 48, 1, {96, 96}, 1, 1, 1, 2)) return 1;
  // valid rows 0 at a deep level (the library admits heights >= 16 only; the arithmetic holds below)
  if (mask_case(12, 3, 6, 4, {96, 15, 8}, 1, 1, 1, 0)) return 1;
  // the q-image's shape: 8-byte pixels two rows and two pixels in, a wide right frame, odd width (the row's last chunk is cut)
  if (mask_case(8, 83, 96, 0, hts, 2, 2, 43, 0)) return 1;
  // more than one workgroup per row (a span above 64 KiB)
  if (mask_case(12, 6000, 24, 2, {96, 50, 17}, 1, 1, 1, 2)) return 1;
  cases += 4;

  // the blob
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int hdr[3];
  if (fread(hdr, 4, 3, f) != 3) return 2;
  const int n = hdr[0], hc = hdr[1], w = hdr[2];
  std::vector<int> heights(n);
  if (fread(heights.data(), 4, n, f) != (size_t)n) return 2;
  const size_t elems = (size_t)n * hc * w * 3;
  std::vector<unsigned char> canvas(elems);
  if (fread(canvas.data(), 1, elems, f) != elems) return 2;
  fclose(f);
  void* mem = nullptr;
  if (posix_memalign(&mem, 16, elems * 4)) return 2;      // exactly the blob: a store past it is ASan's
  float* blob = (float*)mem;
  const long long threads = ((long long)elems + 3) / 4, gx = (threads + 255) / 256;
  for (long long bx = 0; bx < gx; ++bx)
    for (int tid = 0; tid < 256; ++tid) ragged_blob_thread(canvas.data(), blob, heights.data(), n, hc, w, bx * 256 + tid);
  f = fopen(argv[2], "wb");
  if (!f || fwrite(blob, 4, elems, f) != elems) return 2;
  fclose(f);
  free(blob);
  printf("cases %d ok\n", cases);
  return 0;
}
