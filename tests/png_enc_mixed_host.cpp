// TEST INFRASTRUCTURE (never part of the product library): the PNG writer's TABLE form -- csrc/png_enc_dev.h, what the pnge_* kernels of
// png_enc.hip are made of -- compiled for the host with the HIP qualifiers defined away and driven the way the kernels and png_code_table
// (api_png_out.hip) drive it: all images as ONE table over ONE source block, every image at a pitch and an offset of its own, the hist,
// length and write passes as loops over the one-dimensional grid of work items (pnge_locate, then 256 threads per item), the scan a serial
// loop per image. tests/test_png_encode_mixed.py builds this file with g++ -fsanitize=address,undefined and runs it as a child process.
//
// The source block is sized EXACTLY: image i occupies (h - 1) * pitch + 3 w bytes, the images lie back to back, and every second image's
// pitch is wider than 3 w -- a read of a pad byte changes a file (the pads hold a sentinel), a read behind the block is an ASan report.
// The table runs as listed and reversed (another image ends the block), the write pass's items and threads ascending and descending: four
// runs, whose files must agree byte for byte. Per image of the listed run it writes OUTDIR/<index>.png and prints its numbers.
//
// usage: png_enc_mixed_host CASEFILE OUTDIR      exit status 0 = everything held
// case record: int32 h, w, flags (unused here), then h w 3 bytes BGR (tests/png_enc_host.cpp's format)
#define __host__
#define __device__
#define __forceinline__ inline
#include "../text-detection-ctpn_amd/csrc/png_enc_dev.h"

#include <cstdio>
#include <string>

using namespace ctpn;

static const uint8_t SENTINEL = 0xEE;

static uint32_t crc32_plain(const uint8_t* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
  }
  return ~c;
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

// the pitch of case k: 3 w for the even ones, a few bytes more (odd counts too: rows at every alignment) for the odd ones
static uint64_t pitch_of(const Case& c, size_t k) { return 3u * (uint64_t)c.w + ((k & 1) ? 1u + (k % 7u) : 0u); }

// one call over the cases in the given order; files[j]: the file of the j-th image OF THE ORDER
static bool run_table(const std::vector<Case>& cases, const std::vector<size_t>& order, bool descending, std::vector<std::vector<uint8_t>>& files, bool print) {
  const size_t m = order.size();
  bool ok = true;
  std::vector<PngeImg> imgs(m);
  std::vector<PngeRes> res(m);
  std::vector<PngeCodes> codes(m);
  std::memset(res.data(), 0, m * sizeof(PngeRes));
  for (size_t j = 0; j < m; ++j) pnge_describe(imgs[j], cases[order[j]].h, cases[order[j]].w);
  PngeTotals t;
  pnge_layout(imgs.data(), m, t);
  if (!pnge_totals_ok(t)) { std::printf("FAIL totals\n"); return false; }
  // the source: back to back, exactly sized
  uint64_t at = 0;
  for (size_t j = 0; j < m; ++j) {
    const Case& c = cases[order[j]];
    imgs[j].pitch = pitch_of(c, order[j]);
    imgs[j].pix_off = at;
    at += (uint64_t)(c.h - 1) * imgs[j].pitch + 3u * (uint64_t)c.w;
  }
  std::vector<uint8_t> px((size_t)at, SENTINEL);
  for (size_t j = 0; j < m; ++j) {
    const Case& c = cases[order[j]];
    for (int y = 0; y < c.h; ++y) std::memcpy(px.data() + imgs[j].pix_off + (size_t)y * imgs[j].pitch, c.px.data() + (size_t)y * c.w * 3, (size_t)c.w * 3);
  }
  // the item walk: every item maps back to its (image, group); the total is the sum of the images' groups
  uint64_t want_items = 0;
  for (size_t j = 0; j < m; ++j) {
    const uint32_t groups = (imgs[j].npieces + 255u) / 256u;
    if (imgs[j].group0 != want_items) { std::printf("FAIL image %zu: group0 %u, expected %llu\n", j, imgs[j].group0, (unsigned long long)want_items); ok = false; }
    for (uint32_t g = 0; g < groups; ++g) {
      const PngeItem it = pnge_locate(imgs.data(), (uint32_t)m, (uint32_t)(want_items + g));
      if (it.img != j || it.piece != g * 256u) { std::printf("FAIL item %llu: (%u, %u), expected (%zu, %u)\n", (unsigned long long)(want_items + g), it.img, it.piece, j, g * 256u); ok = false; }
    }
    want_items += groups;
  }
  if (t.items != want_items) { std::printf("FAIL items %llu, expected %llu\n", (unsigned long long)t.items, (unsigned long long)want_items); ok = false; }
  if (!ok) return false;
  const uint32_t items = (uint32_t)t.items;
  std::vector<uint32_t> hist(m * PNGE_NSYM, 0u), wd((size_t)t.words, 0u);
  std::vector<PngeLen> len((size_t)t.pieces);
  for (uint32_t item = 0; item < items; ++item) {      // pnge_hist_kernel: a workgroup's counters, then the image's
    const PngeItem it = pnge_locate(imgs.data(), (uint32_t)m, item);
    uint32_t lds[PNGE_NSYM] = {0};
    for (uint32_t th = 0; th < 256; ++th) pnge_hist_thread(imgs[it.img], it.piece + th, px.data(), lds);
    for (int q = 0; q < PNGE_NSYM; ++q) hist[(size_t)it.img * PNGE_NSYM + q] += lds[q];
  }
  for (size_t j = 0; j < m; ++j) pnge_build_codes(imgs[j], hist.data() + j * PNGE_NSYM, codes[j]);
  for (uint32_t item = 0; item < items; ++item) {      // pnge_length_kernel
    const PngeItem it = pnge_locate(imgs.data(), (uint32_t)m, item);
    for (uint32_t th = 0; th < 256; ++th) pnge_length_thread(imgs[it.img], it.piece + th, px.data(), codes[it.img].ll, len.data());
  }
  for (size_t j = 0; j < m; ++j) {      // pnge_scan_kernel
    uint32_t carry = codes[j].hdr_bits;
    uint64_t sa = 0, ss = 0;
    for (uint32_t s = 0; s < imgs[j].npieces; ++s) {
      PngeLen& r = len[imgs[j].piece0 + s];
      pnge_adler_term(imgs[j].n, pnge_piece_end(imgs[j], s), r.a, r.b, sa, ss);
      const uint32_t v = r.bits; r.bits = carry; carry += v;
    }
    pnge_scan_finish(imgs[j], carry, sa, ss, res[j]);
  }
  for (uint32_t i = 0; i < items; ++i) {      // pnge_write_kernel
    const PngeItem it = pnge_locate(imgs.data(), (uint32_t)m, descending ? items - 1u - i : i);
    for (uint32_t k = 0; k < 256; ++k) {
      const uint32_t th = descending ? 255u - k : k;
      pnge_write_thread(imgs[it.img], it.piece + th, px.data(), codes[it.img].ll, codes[it.img].hdr, len.data(), wd.data(), &res[it.img].flag);
    }
  }
  for (size_t i = 0; i < px.size(); ++i) px[i] = 0;      // (nothing reads the source from here on)
  files.assign(m, std::vector<uint8_t>());
  for (size_t j = 0; j < m; ++j) {
    const Case& c = cases[order[j]];
    if (res[j].flag) { std::printf("FAIL image %zu: flag 0x%x\n", order[j], res[j].flag); ok = false; continue; }
    files[j].resize((size_t)PNGE_FRAME_BYTES + res[j].bytes);
    std::memcpy(files[j].data() + PNGE_FRAME_FRONT, wd.data() + imgs[j].word0, res[j].bytes);
    pnge_frame(files[j].data(), c.h, c.w, res[j].bytes, res[j].adler, crc32_plain);
    if (print)
      std::printf("image %zu stream %llu pieces %u groups %u group0 %u far_ok %u pitch %llu bytes %zu\n", order[j], (unsigned long long)imgs[j].n, imgs[j].npieces,
                  (imgs[j].npieces + 255u) / 256u, imgs[j].group0, imgs[j].far_ok, (unsigned long long)imgs[j].pitch, files[j].size());
  }
  if (print) std::printf("items %u pieces %llu source %llu\n", items, (unsigned long long)t.pieces, (unsigned long long)at);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s CASEFILE OUTDIR\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open the case file\n"); return 2; }
  std::vector<Case> cases;
  for (Case c; read_case(f, c);) cases.push_back(c);
  std::fclose(f);
  const size_t m = cases.size();
  if (m == 0) { std::fprintf(stderr, "no cases\n"); return 2; }
  std::vector<size_t> listed(m), reversed(m);
  for (size_t k = 0; k < m; ++k) { listed[k] = k; reversed[k] = m - 1 - k; }
  bool ok = true;
  std::vector<std::vector<uint8_t>> first, other;
  ok &= run_table(cases, listed, false, first, true);
  if (ok) {
    for (int run = 1; run < 4 && ok; ++run) {
      const bool rev = run >= 2, desc = run & 1;
      ok &= run_table(cases, rev ? reversed : listed, desc, other, false);
      for (size_t j = 0; j < m && ok; ++j) {
        const size_t k = rev ? reversed[j] : j;
        if (other[j] != first[k]) { std::printf("FAIL image %zu: %s table, %s write order: other bytes\n", k, rev ? "reversed" : "listed", desc ? "descending" : "ascending"); ok = false; }
      }
    }
    for (size_t k = 0; k < m; ++k) {
      const std::string path = std::string(argv[2]) + "/" + std::to_string(k) + ".png";
      FILE* o = std::fopen(path.c_str(), "wb");
      if (!o || std::fwrite(first[k].data(), 1, first[k].size(), o) != first[k].size()) { std::printf("FAIL image %zu: cannot write %s\n", k, path.c_str()); ok = false; }
      if (o) std::fclose(o);
    }
  }
  std::printf("cases %zu %s\n", m, ok ? "ok" : "FAIL");
  return ok ? 0 : 1;
}
