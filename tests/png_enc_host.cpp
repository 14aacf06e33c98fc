// TEST INFRASTRUCTURE (never part of the product library): the PNG writer's per-piece source text -- csrc/png_enc_dev.h, what the pnge_*
// kernels of png_enc.hip and the library's host form are made of -- compiled for the host with the HIP qualifiers defined away and driven
// the way the kernels and their launcher drive it: every pass a plain loop over thread indices (whole workgroups of 256: the threads
// behind an image's last piece run too), the atomics plain ones, the prefix sum a serial loop, every buffer of exactly the size the library
// gives it (the sanitizers guard the ends). tests/test_png_encode.py builds this file with g++ -fsanitize=address,undefined, writes the
// images into a file and runs the program as a child process. All images run as ONE batch of mixed sizes, twice: the write pass's threads
// in ascending and in descending order; the two must give the same bytes. Per image it writes OUTDIR/<index>.png and prints the literal
// count, the match count by distance and the total bits. With no image involved it checks the code-length builder first.
//
// usage: png_enc_host CASEFILE OUTDIR      exit status 0 = everything held
// case record: int32 h, w, flags (1 = matches at distance stride disabled: the size test's switch, not the library's), then h w 3 bytes BGR
#define __host__
#define __device__
#define __forceinline__ inline
#include "../text-detection-ctpn_amd/csrc/png_enc_dev.h"

#include <cstdio>
#include <string>

using namespace ctpn;

static uint32_t crc32_plain(const uint8_t* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
  }
  return ~c;
}

// tokens by kind, through the same pnge_piece
struct Tally {
  long long nlit = 0, near = 0, far = 0;
  static const bool BYTES = false;
  void lit(uint32_t) { ++nlit; }
  void match(uint32_t, bool f) { ++(f ? far : near); }
  void run(uint32_t, uint32_t) {}
  void byte(uint32_t) {}
};

// maximum length <= limit, Kraft sum exactly 1, zero length exactly for the unused symbols
static bool check_lengths(const char* what, const std::vector<uint32_t>& cnt, int limit) {
  std::vector<uint8_t> len(cnt.size(), 99);
  pnge_build_lengths(cnt.data(), (int)cnt.size(), limit, len.data());
  uint64_t kraft = 0;
  int mx = 0;
  bool ok = true;
  for (size_t i = 0; i < cnt.size(); ++i) {
    if ((cnt[i] == 0) != (len[i] == 0)) ok = false;
    if (len[i]) { kraft += (uint64_t)1 << (limit - std::min<int>(len[i], limit)); mx = std::max<int>(mx, len[i]); }
  }
  if (mx > limit || kraft != (uint64_t)1 << limit) ok = false;
  std::printf("lengths %s: max %d kraft %llu / %llu %s\n", what, mx, (unsigned long long)kraft, (unsigned long long)((uint64_t)1 << limit), ok ? "ok" : "FAIL");
  return ok;
}

static bool builder_selftest() {
  bool ok = true;
  std::vector<uint32_t> fib(40);      // Fibonacci counts: the unlimited Huffman code has depth 39
  uint32_t a = 1, b = 1;
  for (int i = 0; i < 40; ++i) { fib[i] = a; const uint32_t t = a + b; a = b; b = t; }
  ok &= check_lengths("fibonacci-40", fib, 15);
  ok &= check_lengths("two", {5, 0, 0, 9}, 15);
  ok &= check_lengths("three", {0, 1, 1000000, 3}, 15);
  std::vector<uint32_t> all(286);
  for (int i = 0; i < 286; ++i) all[i] = 1u + (uint32_t)((i * 2654435761u) >> 12);
  ok &= check_lengths("all-286", all, 15);
  std::vector<uint32_t> skew(286, 0u);      // a steep histogram with holes
  for (int i = 0; i < 286; i += 3) skew[i] = i < 120 ? fib[i / 3] : 1u;
  ok &= check_lengths("skewed-286", skew, 15);
  return ok;
}

struct Case { int h = 0, w = 0, flags = 0; std::vector<uint8_t> px; };

static bool read_case(FILE* f, Case& c) {
  int32_t hd[3];
  if (std::fread(hd, 1, sizeof(hd), f) != sizeof(hd)) return false;
  c.h = hd[0]; c.w = hd[1]; c.flags = hd[2];
  if (c.h <= 0 || c.w <= 0 || c.h > 65535 || c.w > 65535) return false;
  c.px.resize((size_t)c.h * c.w * 3);
  return std::fread(c.px.data(), 1, c.px.size(), f) == c.px.size();
}

// one batch over all cases; files[k]: the file of case k
static bool run_batch(const std::vector<Case>& cases, bool descending, std::vector<std::vector<uint8_t>>& files, bool print) {
  const size_t m = cases.size();
  std::vector<PngeImg> imgs(m);
  std::vector<PngeRes> res(m);
  std::vector<PngeCodes> codes(m);
  std::memset(res.data(), 0, m * sizeof(PngeRes));
  for (size_t k = 0; k < m; ++k) {      // png_code (api_png_out.hip), with images of any size
    pnge_describe(imgs[k], cases[k].h, cases[k].w);
    if (cases[k].flags & 1) imgs[k].far_ok = 0;
  }
  PngeTotals t;
  pnge_layout(imgs.data(), m, t);
  std::vector<uint8_t> px((size_t)t.pix);      // the batch's pixels in a block of exactly their size
  for (size_t k = 0; k < m; ++k) std::memcpy(px.data() + imgs[k].pix_off, cases[k].px.data(), cases[k].px.size());
  std::vector<uint32_t> hist(m * PNGE_NSYM, 0u), wd((size_t)t.words, 0u);
  std::vector<PngeLen> len((size_t)t.pieces);
  auto threads = [](uint32_t n) { return (n + 255u) / 256u * 256u; };
  for (size_t k = 0; k < m; ++k) {      // pnge_hist_kernel: a workgroup's counters, then the image's
    for (uint32_t g = 0; g < threads(imgs[k].npieces); g += 256) {
      uint32_t lds[PNGE_NSYM] = {0};
      for (uint32_t t = 0; t < 256; ++t) pnge_hist_thread(imgs[k], g + t, px.data(), lds);
      for (int q = 0; q < PNGE_NSYM; ++q) hist[k * PNGE_NSYM + q] += lds[q];
    }
    pnge_build_codes(imgs[k], hist.data() + k * PNGE_NSYM, codes[k]);
  }
  for (size_t k = 0; k < m; ++k)      // pnge_length_kernel
    for (uint32_t s = 0; s < threads(imgs[k].npieces); ++s) pnge_length_thread(imgs[k], s, px.data(), codes[k].ll, len.data());
  for (size_t k = 0; k < m; ++k) {      // pnge_scan_kernel
    uint32_t carry = codes[k].hdr_bits;
    uint64_t sa = 0, ss = 0;
    for (uint32_t s = 0; s < imgs[k].npieces; ++s) {
      PngeLen& r = len[imgs[k].piece0 + s];
      pnge_adler_term(imgs[k].n, pnge_piece_end(imgs[k], s), r.a, r.b, sa, ss);
      const uint32_t v = r.bits; r.bits = carry; carry += v;
    }
    pnge_scan_finish(imgs[k], carry, sa, ss, res[k]);
  }
  for (size_t k = 0; k < m; ++k)      // pnge_write_kernel
    for (uint32_t i = 0; i < threads(imgs[k].npieces); ++i) {
      const uint32_t s = descending ? threads(imgs[k].npieces) - 1 - i : i;
      pnge_write_thread(imgs[k], s, px.data(), codes[k].ll, codes[k].hdr, len.data(), wd.data(), &res[k].flag);
    }
  bool ok = true;
  files.assign(m, std::vector<uint8_t>());
  for (size_t k = 0; k < m; ++k) {
    if (res[k].flag) { std::printf("FAIL image %zu: flag 0x%x\n", k, res[k].flag); ok = false; continue; }
    files[k].resize((size_t)PNGE_FRAME_BYTES + res[k].bytes);
    std::memcpy(files[k].data() + PNGE_FRAME_FRONT, wd.data() + imgs[k].word0, res[k].bytes);
    pnge_frame(files[k].data(), cases[k].h, cases[k].w, res[k].bytes, res[k].adler, crc32_plain);
    if (print) {
      Tally t;
      for (uint32_t s = 0; s < imgs[k].npieces; ++s) pnge_piece(imgs[k], px.data() + imgs[k].pix_off, s, t);
      std::printf("image %zu lit %lld near %lld far %lld bits %u bytes %zu\n", k, t.nlit, t.near, t.far, res[k].bits, files[k].size());
    }
  }
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s CASEFILE OUTDIR\n", argv[0]); return 2; }
  bool ok = builder_selftest();
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open the case file\n"); return 2; }
  std::vector<Case> cases;
  for (Case c; read_case(f, c);) cases.push_back(c);
  std::fclose(f);
  std::vector<std::vector<uint8_t>> up, down;
  if (!cases.empty()) {
    ok &= run_batch(cases, false, up, true);
    ok &= run_batch(cases, true, down, false);
    for (size_t k = 0; k < cases.size(); ++k) {
      if (up[k] != down[k]) { std::printf("FAIL image %zu: the write pass's order changed the bytes\n", k); ok = false; }
      // the library's host form is the same text driven serially
      size_t need = 0;
      (void)pnge_encode_host(cases[k].px.data(), cases[k].h, cases[k].w, nullptr, 0, &need, crc32_plain);
      std::vector<uint8_t> host(need);
      if (!pnge_encode_host(cases[k].px.data(), cases[k].h, cases[k].w, host.data(), need, &need, crc32_plain) || (!(cases[k].flags & 1) && host != up[k])) {
        std::printf("FAIL image %zu: the serial host form differs\n", k); ok = false;
      }
      if (up[k].size() > pnge_capacity(cases[k].h, cases[k].w)) { std::printf("FAIL image %zu: above the capacity\n", k); ok = false; }
      const std::string path = std::string(argv[2]) + "/" + std::to_string(k) + ".png";
      FILE* o = std::fopen(path.c_str(), "wb");
      if (!o || std::fwrite(up[k].data(), 1, up[k].size(), o) != up[k].size()) { std::printf("FAIL image %zu: cannot write %s\n", k, path.c_str()); ok = false; }
      if (o) std::fclose(o);
    }
  }
  std::printf("cases %zu %s\n", cases.size(), ok ? "ok" : "FAIL");
  return ok ? 0 : 1;
}
