// Stand-alone host program over csrc/data_layer_dev.h, the per-thread text of data_layer.hip's kernels: built by tests/test_data_layer.py with
// g++ -ffp-contract=off -fsanitize=address,undefined and run as a subprocess. It walks a label set, a page and a box list the way the kernels
// do -- one quad, one strip, one 16-byte group, one box at a time -- between heap blocks of exactly the arrays' sizes, so a read or write past
// an array's end stops the program.
//   data_layer_host split IN OUT [MUTANT]
//     IN : int32 pages, nq; int32 dims[pages][4]; int32 quad_offsets[pages + 1]; double quads[nq][8]
//     OUT: int32 total; int32 strip_offsets[pages + 1]; int32 quad_strip_offsets[nq + 1]; float strips[total][4]
//   data_layer_host page IN OUT [MUTANT]
//     IN : int32 h, w, pitch, offset, flip, oh, ow, pad; double factor; uint8 rows[(h - 1) pitch + 3 w]   (the image starts `offset` bytes
//          into a heap block of offset + that many bytes: pointer alignments 0 .. 3)
//     OUT: uint8 image[oh][ow][3]; float blob[oh][ow][3]
//   data_layer_host boxes IN OUT [MUTANT]
//     IN : int32 g, page_width, flip, pad; double scale; float strips[g][4]
//     OUT: int32 ok; float boxes[g][5] (ok = 0: a strip outside uint16, boxes unspecified)
// MUTANT (the test asserts each one FAILS the comparison): 1 the input mirrored instead of the output, 2 `<= xmax` in the strip walk, 3 a signed
// flip without the uint16 wrap, 4 multiply before dividing in the scaling, 5 an unstable tie order in the sort by x.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "data_layer_dev.h"

using namespace ctpn;

static int mutant = 0;

static void read_all(FILE* f, void* p, size_t bytes) {
  if (bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "short read\n"); exit(2); }
}

static DlSpan quad_span(const double* q8, const int* d4) {
  if (mutant != 4 && mutant != 5) return dl_quad_span(q8, d4);
  int x[4], y[4];
  for (int k = 0; k < 4; ++k) {
    if (mutant == 4) {
      x[k] = (int)(q8[2 * k] * (double)d4[3] / (double)d4[1]);
      y[k] = (int)(q8[2 * k + 1] * (double)d4[2] / (double)d4[0]);
    } else {
      x[k] = dl_scale(q8[2 * k], d4[1], d4[3]);
      y[k] = dl_scale(q8[2 * k + 1], d4[0], d4[2]);
    }
  }
  if (mutant == 5) {      // an insertion sort that moves past equal keys: ties come out reversed
    for (int i = 1; i < 4; ++i) {
      const int vx = x[i], vy = y[i];
      int j = i;
      for (; j > 0 && x[j - 1] >= vx; --j) { x[j] = x[j - 1]; y[j] = y[j - 1]; }
      x[j] = vx; y[j] = vy;
    }
  } else {
    dl_sort4(x, y);
  }
  return dl_span(x, y, d4[2], d4[3]);
}

// mutant 2: the multiples of 16 in (xmin, xmax] instead of (xmin, xmax)
static int strip_count(int xmin, int xmax) { return mutant == 2 ? (xmin == xmax ? 0 : dl_strip_count(xmin, xmax + 1)) : dl_strip_count(xmin, xmax); }
static void strip(int xmin, int xmax, int k, int& x1, int& x2) {
  if (mutant != 2) { dl_strip(xmin, xmax, k, x1, x2); return; }
  dl_strip(xmin, xmax + 1, k, x1, x2);
  if (x2 == xmax + 1) x2 = xmax;
}

static int run_split(FILE* f, FILE* o) {
  int32_t head[2];
  read_all(f, head, sizeof head);
  const int pages = head[0], nq = head[1];
  if (pages < 1 || nq < 0) return 2;
  std::unique_ptr<int32_t[]> dims(new int32_t[(size_t)pages * 4]), qoffs(new int32_t[(size_t)pages + 1]);
  std::unique_ptr<double[]> quads(new double[(size_t)nq * 8]);
  read_all(f, dims.get(), (size_t)pages * 16);
  read_all(f, qoffs.get(), ((size_t)pages + 1) * 4);
  read_all(f, quads.get(), (size_t)nq * 64);
  // pass 1: one quad at a time
  std::unique_ptr<DlSpan[]> spans(new DlSpan[(size_t)nq]);
  std::unique_ptr<int32_t[]> counts(new int32_t[(size_t)nq]), scan(new int32_t[(size_t)nq + 1]), poffs(new int32_t[(size_t)pages + 1]);
  for (int q = 0; q < nq; ++q) {
    const int page = dl_upper(qoffs.get(), pages, q);
    spans[(size_t)q] = quad_span(quads.get() + (size_t)q * 8, dims.get() + (size_t)page * 4);
    counts[(size_t)q] = strip_count(spans[(size_t)q].xmin, spans[(size_t)q].xmax);
  }
  // pass 2
  int32_t run = 0;
  for (int q = 0; q < nq; ++q) { scan[(size_t)q] = run; run += counts[(size_t)q]; }
  scan[(size_t)nq] = run;
  for (int p = 0; p <= pages; ++p) poffs[(size_t)p] = scan[(size_t)qoffs[(size_t)p]];
  // pass 3: one strip at a time
  const int32_t total = run;
  std::unique_ptr<float[]> strips(new float[(size_t)total * 4]);
  for (int s = 0; s < total; ++s) {
    const int q = dl_upper(scan.get(), nq, s);
    int x1, x2;
    strip(spans[(size_t)q].xmin, spans[(size_t)q].xmax, s - scan[(size_t)q], x1, x2);
    float* r = strips.get() + (size_t)s * 4;
    r[0] = (float)x1; r[1] = (float)spans[(size_t)q].ymin; r[2] = (float)x2; r[3] = (float)spans[(size_t)q].ymax;
  }
  fwrite(&total, 4, 1, o);
  fwrite(poffs.get(), 4, (size_t)pages + 1, o);
  fwrite(scan.get(), 4, (size_t)nq + 1, o);
  fwrite(strips.get(), 4, (size_t)total * 4, o);
  return 0;
}

static int run_page(FILE* f, FILE* o) {
  int32_t head[8];
  double factor;
  read_all(f, head, sizeof head);
  read_all(f, &factor, sizeof factor);
  DlPage p{};
  p.h = head[0]; p.w = head[1]; p.pitch = head[2]; p.flip = head[4]; p.oh = head[5]; p.ow = head[6];
  const int offset = head[3];
  if (p.h < 1 || p.w < 1 || p.pitch < 3LL * p.w || offset < 0 || p.oh < 1 || p.ow < 1) return 2;
  p.resize = factor > 0.0 && factor != 1.0;
  p.inv_f = p.resize ? 1.0 / factor : 0.0;
  const size_t bytes = (size_t)(p.h - 1) * (size_t)p.pitch + (size_t)p.w * 3;
  std::unique_ptr<uint8_t[]> block(new uint8_t[(size_t)offset + bytes]);
  uint8_t* src = block.get() + offset;
  read_all(f, src, bytes);
  if (mutant == 1 && p.flip) {      // the file mirrored first, then resized
    for (int y = 0; y < p.h; ++y)
      for (int x = 0; x < p.w / 2; ++x)
        for (int c = 0; c < 3; ++c) {
          uint8_t& a = src[(size_t)y * p.pitch + (size_t)x * 3 + c];
          uint8_t& b = src[(size_t)y * p.pitch + (size_t)(p.w - 1 - x) * 3 + c];
          const uint8_t t = a; a = b; b = t;
        }
    p.flip = 0;
  }
  const size_t total = dl_page_bytes(p), groups = dl_page_groups(p);
  std::unique_ptr<uint8_t[]> image(new uint8_t[total]);
  std::unique_ptr<float[]> blob(new float[total]);
  for (size_t g = 0; g < groups; ++g) {
    uint8_t v[DL_GROUP];
    const int count = dl_page_group(src, p, g, v);
    int c = (int)(g * DL_GROUP % 3);
    for (int k = 0; k < count; ++k) {
      image[g * DL_GROUP + k] = v[k];
      blob[g * DL_GROUP + k] = dl_blob(v[k], c);
      c = c == 2 ? 0 : c + 1;
    }
  }
  fwrite(image.get(), 1, total, o);
  fwrite(blob.get(), 4, total, o);
  return 0;
}

static int run_boxes(FILE* f, FILE* o) {
  int32_t head[4];
  double scale;
  read_all(f, head, sizeof head);
  read_all(f, &scale, sizeof scale);
  const int g = head[0], W = head[1], flip = head[2];
  if (g < 0) return 2;
  std::unique_ptr<float[]> strips(new float[(size_t)g * 4]), out(new float[(size_t)g * 5]);
  read_all(f, strips.get(), (size_t)g * 16);
  int32_t ok = 1;
  for (int i = 0; i < g; ++i) {
    float* r = out.get() + (size_t)i * 5;
    const float* s = strips.get() + (size_t)i * 4;
    if (mutant == 3 && flip) {
      int x1 = W - (int)s[2] - 1;
      const int x2 = W - (int)s[0] - 1;
      if (x2 < x1) x1 = 0;
      r[0] = (float)((double)x1 * scale); r[1] = (float)((double)s[1] * scale); r[2] = (float)((double)x2 * scale); r[3] = (float)((double)s[3] * scale);
      r[4] = 1.f;
    } else if (!dl_box(s, W, flip, scale, r)) {
      ok = 0;
      for (int k = 0; k < 5; ++k) r[k] = 0.f;
    }
  }
  fwrite(&ok, 4, 1, o);
  fwrite(out.get(), 4, (size_t)g * 5, o);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: data_layer_host split|page|boxes IN OUT [MUTANT]\n"); return 2; }
  if (argc > 4) mutant = atoi(argv[4]);
  FILE* f = fopen(argv[2], "rb");
  if (!f) { perror(argv[2]); return 2; }
  FILE* o = fopen(argv[3], "wb");
  if (!o) { perror(argv[3]); return 2; }
  int rc = 2;
  if (!strcmp(argv[1], "split")) rc = run_split(f, o);
  else if (!strcmp(argv[1], "page")) rc = run_page(f, o);
  else if (!strcmp(argv[1], "boxes")) rc = run_boxes(f, o);
  fclose(f);
  fclose(o);
  return rc;
}
