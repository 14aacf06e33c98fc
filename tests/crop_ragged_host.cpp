// TEST INFRASTRUCTURE (never part of the product library): crop_lines_kernel's per-thread source text over a RAGGED canvas --
// csrc/crop_pixel.h: crop_image (slot base and the image's own height), crop_column, crop_quad -- compiled for the host and driven the way
// the kernel drives it: per line one "thread" for every four output columns up to max_w. tests/test_out_ragged.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a subprocess.
//   in : int n, hc, w, lines, crop_h, max_w, pad; int heights[n]; int img[lines], wc[lines]; double q[lines][8]; uint8 canvas[n][hc][w][3]
//   out: lines x crop_h x max_w x 3
// The canvas is allocated at its exact size: a read outside it trips ASan; a read of the rows under an image changes bytes (the test fills
// them with a sentinel).
#define __host__
#define __device__
#define __forceinline__ inline
#include "../text-detection-ctpn_amd/csrc/crop_pixel.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace ctpn;

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: crop_ragged_host IN OUT\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int head[7];
  if (std::fread(head, sizeof(int), 7, f) != 7) return 2;
  const int n = head[0], hc = head[1], w = head[2], lines = head[3], crop_h = head[4], max_w = head[5], pad = head[6];
  if (n <= 0 || hc <= 0 || w <= 0 || lines <= 0 || crop_h <= 0 || max_w < 4 || (max_w & 3)) return 2;
  std::vector<int> heights(n), img(lines), wc(lines);
  std::vector<double> q((size_t)lines * 8);
  if (std::fread(heights.data(), sizeof(int), n, f) != (size_t)n || std::fread(img.data(), sizeof(int), lines, f) != (size_t)lines ||
      std::fread(wc.data(), sizeof(int), lines, f) != (size_t)lines || std::fread(q.data(), sizeof(double), q.size(), f) != q.size()) return 2;
  const size_t bytes = (size_t)n * hc * w * 3;
  uint8_t* canvas = new uint8_t[bytes];
  if (std::fread(canvas, 1, bytes, f) != bytes) return 2;
  std::fclose(f);
  const size_t line_bytes = (size_t)crop_h * max_w * 3;
  std::vector<uint8_t> out((size_t)lines * line_bytes, 0xEE);
  for (int l = 0; l < lines; ++l) {
    CropDesc d;
    for (int k = 0; k < 8; ++k) d.q[k] = q[(size_t)l * 8 + k];
    d.img = img[l]; d.wc = wc[l]; d.out_off = (unsigned long long)l * line_bytes;
    if (d.img < 0 || d.img >= n) return 2;
    for (int u0 = 0; u0 < max_w; u0 += 4) {                      // one thread
      CropColumn cols[4];
      for (int k = 0; k < 4; ++k) cols[k] = crop_column(d.q, u0 + k, d.wc);
      int h;
      const uint8_t* im = crop_image(canvas, d.img, hc, w, heights.data(), h);
      for (int v = 0; v < crop_h; ++v) {
        uint32_t px[3];
        crop_quad(im, h, w, cols, u0, d.wc, v, crop_h, pad, px);
        std::memcpy(out.data() + d.out_off + ((size_t)v * max_w + u0) * 3, px, 12);      // (little-endian, like the device)
      }
    }
  }
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  std::fwrite(out.data(), 1, out.size(), o);
  std::fclose(o);
  std::printf("lines %d ok\n", lines);
  delete[] canvas;
  return 0;
}
