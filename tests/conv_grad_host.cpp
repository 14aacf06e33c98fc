// Stand-alone host program over csrc/conv_grad_dev.h, the per-thread text of conv_grad.hip's kernels: built by tests/test_conv_grad.py with
// g++ -ffp-contract=off -fsanitize=address,undefined and run as a subprocess. It runs one whole small layer the way the kernels walk it -- the
// ReLU mask (cg_relu_mask), the data gradient as one fma chain per element over taps and output channels (cg_pixel_coords, cg_tap_ok,
// cg_tap_offset), the weight gradient as fma chains over the plan's pixel blocks (cg_plan) and the ordered pass (tb_tn_reduce), the bias sums
// (tb_colsum_block), and the max-pool backward (cg_pool_backward) -- from heap blocks of exactly the problem's size, so a read or write past
// an array's end stops the program.
//   conv_grad_host IN OUT [MUTANT]
// IN : int32 n, h, w, ci, co; then float32 x [M][ci], wt [9][ci][co], y [M][co], d_y [M][co], d_pool [n][h/2][w/2][co]; M = n h w
// OUT: int64 block_pixels, int64 blocks; then float32 d_w [9][ci][co], d_b [co], d_x [M][ci], d_full [M][co] (the pool backward of d_pool over y)
// MUTANT (the test asserts each one FAILS the comparison): 1 the data gradient with the kernel not rotated (w[2-ky][2-kx] where w[ky][kx]
// belongs), 2 taps crossing the image seam (rows are not checked against the image, only against the batch), 3 the mask y >= 0, 4 pool to the
// last maximum.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "conv_grad_dev.h"

using namespace ctpn;

static int mutant = 0;

static std::unique_ptr<float[]> block(size_t n) { return std::unique_ptr<float[]>(new float[n]()); }

static void read_all(FILE* f, void* p, size_t bytes) {
  if (bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "short read\n"); exit(2); }
}

// the predicate every tap goes through; mutant 2 keeps the column check and asks of the row only that the flat pixel stays inside the batch
static bool tap_ok(int h, int w, int i, int j, int dy, int dx, long long p, long long M) {
  if (mutant == 2) {
    const long long src = p + cg_tap_offset(w, dy, dx);
    return j + dx >= 0 && j + dx < w && src >= 0 && src < M;
  }
  return cg_tap_ok(h, w, i, j, dy, dx);
}

static int first_max(float a, float b, float c, float d) {
  if (mutant != 4) return cg_pool_first_max(a, b, c, d);
  int k = 0;
  float best = a;
  if (b >= best) { best = b; k = 1; }
  if (c >= best) { best = c; k = 2; }
  if (d >= best) { best = d; k = 3; }
  return k;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: conv_grad_host IN OUT [MUTANT]\n"); return 2; }
  if (argc > 3) mutant = atoi(argv[3]);
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t dims[5];
  read_all(f, dims, sizeof dims);
  const int n = dims[0], h = dims[1], w = dims[2], ci = dims[3], co = dims[4];
  const long long M = (long long)n * h * w;
  const size_t Mz = (size_t)M, wn = (size_t)9 * ci * co, pooled = (size_t)n * (h / 2) * (w / 2) * co;
  auto x = block(Mz * ci), wt = block(wn), y = block(Mz * co), d_y = block(Mz * co), d_pool = block(pooled);
  read_all(f, x.get(), Mz * ci * 4);
  read_all(f, wt.get(), wn * 4);
  read_all(f, y.get(), Mz * co * 4);
  read_all(f, d_y.get(), Mz * co * 4);
  read_all(f, d_pool.get(), pooled * 4);
  fclose(f);

  // cg_mask_kernel
  auto dz = block(Mz * co);
  for (size_t e = 0; e < Mz * co; ++e) dz[e] = mutant == 3 ? (y[e] >= 0.f ? d_y[e] : 0.f) : cg_relu_mask(d_y[e], y[e]);

  // cg_dx_kernel: one chain per element, taps in (ky, kx) order, output channels ascending
  auto d_x = block(Mz * ci);
  for (long long p = 0; p < M; ++p) {
    int i, j;
    cg_pixel_coords(p, h, w, i, j);
    for (int c = 0; c < ci; ++c) {
      float acc = 0.f;
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
          const int dy = 1 - ky, dx = 1 - kx;
          if (!tap_ok(h, w, i, j, dy, dx, p, M)) continue;
          const float* zrow = dz.get() + (size_t)(p + cg_tap_offset(w, dy, dx)) * co;
          const int tap = mutant == 1 ? (2 - ky) * 3 + (2 - kx) : ky * 3 + kx;
          const float* wrow = wt.get() + ((size_t)tap * ci + c) * co;
          for (int o = 0; o < co; ++o) acc = fmaf(wrow[o], zrow[o], acc);
        }
      d_x[(size_t)p * ci + c] = acc;
    }
  }

  // cg_dw_partial_kernel + cg_reduce_kernel, cg_colsum_kernel + cg_reduce_kernel
  long long blk;
  int P;
  cg_plan(M, ci, co, blk, P);
  auto d_w = block(wn), d_b = block((size_t)co);
  std::vector<float> parts((size_t)P);
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx)
      for (int c = 0; c < ci; ++c)
        for (int o = 0; o < co; ++o) {
          for (int pb = 0; pb < P; ++pb) {
            const long long lo = pb * blk, hi = lo + blk < M ? lo + blk : M;
            float acc = 0.f;
            for (long long p = lo; p < hi; ++p) {
              int i, j;
              cg_pixel_coords(p, h, w, i, j);
              const float a = tap_ok(h, w, i, j, ky - 1, kx - 1, p, M) ? x[(size_t)(p + cg_tap_offset(w, ky - 1, kx - 1)) * ci + c] : 0.f;
              acc = fmaf(a, dz[(size_t)p * co + o], acc);
            }
            parts[pb] = acc;
          }
          d_w[((size_t)(ky * 3 + kx) * ci + c) * co + o] = tb_tn_reduce(parts.data(), P, 1);
        }
  for (int o = 0; o < co; ++o) {
    for (int pb = 0; pb < P; ++pb) {
      const long long lo = pb * blk, hi = lo + blk < M ? lo + blk : M;
      parts[pb] = tb_colsum_block(dz.get() + (size_t)lo * co + o, hi - lo, (size_t)co);
    }
    d_b[o] = tb_tn_reduce(parts.data(), P, 1);
  }

  // cg_pool_kernel: every element of d_full
  auto d_full = block(Mz * co);
  const int hp = h / 2, wp = w / 2;
  for (int img = 0; img < n; ++img)
    for (int i = 0; i < h; ++i)
      for (int j = 0; j < w; ++j)
        for (int ch = 0; ch < co; ++ch) {
          const float* y_img = y.get() + (size_t)img * h * w * co + ch;
          const float* dp_img = d_pool.get() + (size_t)img * hp * wp * co + ch;
          float v;
          if (mutant != 4) v = cg_pool_backward(y_img, dp_img, h, w, (size_t)co, i, j);
          else {
            const int wi = i / 2, wj = j / 2;
            v = 0.f;
            if (wi < hp && wj < wp) {
              const float* y0 = y_img + ((size_t)(2 * wi) * w + (size_t)(2 * wj)) * co;
              const int k = first_max(y0[0], y0[co], y0[(size_t)w * co], y0[(size_t)w * co + co]);
              if (k == (i & 1) * 2 + (j & 1)) v = dp_img[((size_t)wi * wp + (size_t)wj) * co];
            }
          }
          d_full[(((size_t)img * h + i) * w + j) * co + ch] = v;
        }

  FILE* g = fopen(argv[2], "wb");
  if (!g) { perror(argv[2]); return 2; }
  const int64_t plan[2] = {blk, P};
  fwrite(plan, sizeof plan, 1, g);
  fwrite(d_w.get(), 4, wn, g);
  fwrite(d_b.get(), 4, (size_t)co, g);
  fwrite(d_x.get(), 4, Mz * ci, g);
  fwrite(d_full.get(), 4, Mz * co, g);
  fclose(g);
  return 0;
}
