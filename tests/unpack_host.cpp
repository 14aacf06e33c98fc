// Stand-alone host program over csrc/unpack_dev.h, the per-thread text of unpack.hip's kernel: built by tests/test_solver.py with g++
// -fsanitize=address,undefined and run as a subprocess. It unpacks one stored block quad by quad, as the kernel's threads do, from a heap block
// of exactly the stored size into one of exactly the tensor's size, so a read or write past either end stops the program.
//   unpack_host IN OUT
// IN : int32 n, H, W, C, ld, border, kind, gates; then the stored block: n (H + 2 border) (W + 2 border) ld values of 4 (kind 0) or 2 bytes
// OUT: float32 [n][H][W][C]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "unpack_dev.h"

using namespace ctpn;

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: unpack_host IN OUT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t h[8];
  if (fread(h, 4, 8, f) != 8) return 2;
  UnpackDesc d{};
  d.n = h[0]; d.H = h[1]; d.W = h[2]; d.C = h[3]; d.ld = h[4]; d.border = h[5]; d.kind = h[6]; d.gates = h[7];
  const size_t es = d.kind == UP_F32 ? 4 : 2;
  const size_t stored = (size_t)d.n * (d.H + 2 * d.border) * (d.W + 2 * d.border) * d.ld * es;
  // operator new: 16-byte aligned, as the device block is; exactly `stored` bytes
  std::unique_ptr<char[]> src(new char[stored]);
  if (stored && fread(src.get(), 1, stored, f) != stored) { fprintf(stderr, "short read\n"); return 2; }
  fclose(f);
  const size_t quads = up_quads(d);
  std::unique_ptr<float[]> out(new float[quads * 4]);
  for (size_t q = 0; q < quads; ++q) up_quad(src.get(), d, q, out.get() + 4 * q);
  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 2; }
  fwrite(out.get(), 4, quads * 4, o);
  fclose(o);
  return 0;
}
