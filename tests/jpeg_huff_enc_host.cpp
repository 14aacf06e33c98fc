// TEST INFRASTRUCTURE (never part of the product library): the device Huffman coder's per-thread source text -- csrc/jpeg_huff_enc_dev.h,
// what the jhe_* kernels of jpeg_huff_enc.hip are made of -- compiled for the host with the HIP qualifiers defined away and driven the way
// the kernels and their launcher drive it: every pass a plain loop over thread indices (whole workgroups of 256: the threads behind an
// image's last block or chunk run too), the atomic OR a plain one, the two prefix sums serial loops, every buffer of exactly the size the
// library gives it (the sanitizers guard the ends). tests/test_jpeg_huff_enc_host.py builds this file with g++ -fsanitize=address,undefined,
// writes the cases (size, sampling, coefficients in natural order, the file ctpn_jpeg_entropy_encode writes for them) into a file and runs
// the program as a child process. All cases run as ONE launch group, twice: natural order with the write pass's threads in ascending order,
// zig-zag order (the coefficients converted) with them in descending order. The scan body must equal the file's bytes between the header and
// EOI -- header and EOI are the host's in both forms -- unless the host refused the coefficients: then the flag must be raised.
//
// usage: jpeg_huff_enc_host CASEFILE      exit status 0 = every case held in both runs
#define __host__
#define __device__
#define __forceinline__ inline
#include "../text-detection-ctpn_amd/csrc/jpeg_huff_enc_dev.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace ctpn;

struct Case {
  int h = 0, w = 0, hs = 0, vs = 0, host_status = 0, header = 0;
  std::vector<int16_t> coef;      // natural order
  std::vector<uint8_t> file;      // the host's file (empty if it refused)
};

static bool rd(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

static bool read_case(FILE* f, Case& c) {
  int32_t hd[8];
  if (!rd(f, hd, sizeof(hd))) return false;
  c.h = hd[0]; c.w = hd[1]; c.hs = hd[2]; c.vs = hd[3]; c.host_status = hd[4]; c.header = hd[5];
  if (hd[6] < 0 || hd[7] < 0 || hd[6] > (1 << 28) || hd[7] > (1 << 28)) return false;
  c.coef.resize((size_t)hd[6]); c.file.resize((size_t)hd[7]);
  return rd(f, c.coef.data(), c.coef.size() * 2) && rd(f, c.file.data(), c.file.size());
}

// one launch group over all cases; returns the number of cases that did not hold
static int run_group(const std::vector<Case>& cases, const JheTables& T, bool zigzag, long long& coded, long long& flagged) {
  const size_t m = cases.size();
  std::vector<JheImg> imgs(m);
  std::vector<JheRes> res(m);
  std::memset(res.data(), 0, m * sizeof(JheRes));
  long long elems = 0;
  for (size_t k = 0; k < m; ++k) {      // enc_huff_group (api_jpeg_out.hip)
    const Case& c = cases[k];
    JheImg& I = imgs[k];
    jhe_describe(I, c.h, c.w, c.hs, c.vs);
    I.coef_off = elems;
    if (c.coef.size() != (size_t)I.nblk * 64) { std::printf("FAIL case %zu: %zu coefficients for %u blocks\n", k, c.coef.size(), I.nblk); return (int)m; }
    elems += (long long)I.nblk * 64;
  }
  JheTotals t;
  jhe_layout(imgs.data(), m, t);
  // the batch's coefficients in a block of exactly their size, 16-byte aligned like the library's (a block is then 128-byte aligned)
  std::vector<int16_t> coef((size_t)elems);
  for (size_t k = 0; k < m; ++k) {
    int16_t* dst = coef.data() + imgs[k].coef_off;
    const int16_t* src = cases[k].coef.data();
    for (size_t b = 0; b < (size_t)imgs[k].nblk; ++b)
      for (int q = 0; q < 64; ++q) dst[b * 64 + q] = zigzag ? src[b * 64 + T.nat[q]] : src[b * 64 + q];
  }
  std::vector<uint32_t> len(t.blk), cnt(t.chunks), uns(t.words, 0u);
  std::vector<uint8_t> out(t.outb);
  auto threads = [](uint32_t n) { return (n + 255u) / 256u * 256u; };
  for (size_t k = 0; k < m; ++k)      // jhe_length_kernel
    for (uint32_t s = 0; s < threads(imgs[k].nblk); ++s) {
      if (zigzag) jhe_length_thread<true>(imgs[k], s, coef.data(), T, len.data(), &res[k].flag);
      else jhe_length_thread<false>(imgs[k], s, coef.data(), T, len.data(), &res[k].flag);
    }
  for (size_t k = 0; k < m; ++k) {      // jhe_scan_kernel<false>
    uint32_t carry = 0;
    for (uint32_t s = 0; s < imgs[k].nblk; ++s) { const uint32_t v = len[imgs[k].blk0 + s]; len[imgs[k].blk0 + s] = carry; carry += v; }
    jhe_scan_finish<false>(imgs[k], 0u, carry, res[k]);
  }
  for (size_t k = 0; k < m; ++k)      // jhe_write_kernel
    for (uint32_t i = 0; i < threads(imgs[k].nblk); ++i) {
      const uint32_t s = zigzag ? threads(imgs[k].nblk) - 1 - i : i;
      if (zigzag) jhe_write_thread<true>(imgs[k], s, coef.data(), T, len.data(), uns.data(), &res[k].flag);
      else jhe_write_thread<false>(imgs[k], s, coef.data(), T, len.data(), uns.data(), &res[k].flag);
    }
  for (size_t k = 0; k < m; ++k)      // jhe_count_kernel
    for (uint32_t q = 0; q < threads(imgs[k].nchunk); ++q) jhe_count_thread(imgs[k], q, res[k].bits, uns.data(), cnt.data());
  for (size_t k = 0; k < m; ++k) {      // jhe_scan_kernel<true>
    const uint32_t count = jhe_chunk_count(res[k].bits, imgs[k]);
    uint32_t carry = 0;
    for (uint32_t q = 0; q < count; ++q) { const uint32_t v = cnt[imgs[k].chunk0 + q]; cnt[imgs[k].chunk0 + q] = carry; carry += v; }
    jhe_scan_finish<true>(imgs[k], res[k].bits, carry, res[k]);
  }
  for (size_t k = 0; k < m; ++k)      // jhe_stuff_kernel
    for (uint32_t q = 0; q < threads(imgs[k].nchunk); ++q) jhe_stuff_thread(imgs[k], q, res[k].bits, uns.data(), cnt.data(), out.data(), &res[k].flag);
  int bad = 0;
  for (size_t k = 0; k < m; ++k) {
    const Case& c = cases[k];
    bool ok;
    if (c.host_status != 0) {
      ok = res[k].flag != 0;
    } else {
      const size_t hd = (size_t)c.header;
      ok = res[k].flag == 0 && c.file.size() == hd + res[k].bytes + 2 && std::memcmp(c.file.data() + hd, out.data() + imgs[k].out0, res[k].bytes) == 0 &&
           c.file[c.file.size() - 2] == 0xFF && c.file[c.file.size() - 1] == 0xD9;
    }
    if (res[k].flag) ++flagged; else ++coded;
    if (!ok) { ++bad; std::printf("FAIL case %zu (%s order): flag 0x%x bits %u bytes %u host status %d file %zu\n", k, zigzag ? "zig-zag" : "natural", res[k].flag, res[k].bits, res[k].bytes, c.host_status, c.file.size()); }
  }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open the case file\n"); return 2; }
  std::vector<Case> cases;
  for (Case c; read_case(f, c);) cases.push_back(c);
  std::fclose(f);
  JheTables T;
  jhe_build_tables(T);
  long long coded = 0, flagged = 0;
  int bad = 0;
  if (!cases.empty()) bad = run_group(cases, T, false, coded, flagged) + run_group(cases, T, true, coded, flagged);
  std::printf("cases %zu coded %lld flagged %lld bad %d\n", cases.size(), coded, flagged, bad);
  return bad ? 1 : 0;
}
