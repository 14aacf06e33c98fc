// The per-piece source of the PNG writer (png_enc.hip), in a header of its own so that ONE text serves two compilers, like
// jpeg_huff_enc_dev.h: hipcc compiles it into the pnge_* kernels and into the library's host form (ctpn_png_encode);
// tests/png_enc_host.cpp compiles the same text with g++ under ASan / UBSan and runs every pass as a plain loop over thread indices.
//
// The file (docs/decode_pipeline.md, "PNG out"): signature, IHDR (8-bit RGB), ONE IDAT, IEND. The zlib stream is 78 01, one dynamic-Huffman
// DEFLATE block, Adler-32. The filtered stream -- per row the byte 1 (Sub) and 3 w bytes raw[x] - raw[x - 3] -- is never stored: pnge_byte
// computes a byte from the BGR pixels. It is cut into pieces of PNGE_P bytes, and a piece is tokenised on its own, greedily, with two
// candidates per position: a run of the byte before (distance 1) and a repeat of the row above (distance stride). So one thread takes one
// piece, and the passes are
//   hist     pnge_piece into a sink that counts symbols  -> the image's 286 counters; the host builds the literal/length code and the
//            block header from them (pnge_build_codes)
//   length   pnge_piece into a sink that counts bits     -> bits per piece, and the piece's Adler partials (sum b, sum (len - j) b_j)
//   scan     exclusive prefix sum per image              -> every piece's bit offset behind the header, the total, the Adler-32
//   write    pnge_piece into a sink that writes          -> the DEFLATE block, LSB first, in 32-bit words; a word that pieces share is
//            combined with an atomic OR into a buffer that was cleared before; the thread of the last piece adds EOB
// The three passes run the SAME pnge_piece: they cannot disagree. Every loop is bounded before it starts (PNGE_P positions per piece, 258
// bytes per candidate); every store is checked against the image's part of the buffer.
//
// A call is a TABLE of images of any sizes (PngeImg): image i's pixels begin at pix_off, its rows are `pitch` bytes apart (>= 3 w). The read
// is byte-wise (pnge_byte): the writer never touches a byte outside an image's h x w x 3 pixels, at any pitch or alignment -- not the
// pitch's padding, not a byte behind the last row's last pixel. That asks less of the caller than the JPEG writer's aligned-dword read
// (jpeg_enc_mixed_dev.h, jenc_load4). The hist, length and write kernels run over a one-dimensional grid of WORK ITEMS: an item is one
// workgroup, PNGE_GROUP pieces, of ONE image (the LDS counters and the staged code table belong to one image); image i has
// ceil(npieces_i / PNGE_GROUP) of them from group0 on (pnge_layout), and pnge_locate finds an item's image (jem_locate's search).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "bits_dev.h"

#define PNGE_HD BITS_HD

namespace ctpn {

enum : uint32_t { PNGE_FLAG_STORE = BITS_FLAG_STORE, PNGE_FLAG_SIZE = BITS_FLAG_SIZE };

enum {
  PNGE_P = 256,             // stream bytes per piece
  PNGE_GROUP = 256,         // pieces per work item (the threads of a workgroup)
  PNGE_NSYM = 286,          // literal/length symbols (HLIT = 29)
  PNGE_EOB = 256,
  PNGE_HDR_WORDS = 42,      // the block header: 17 + 57 + 4 (286 + 30) = 1338 bits at most
  PNGE_SCAN_ITEMS = 1024    // pieces one workgroup of the scan takes per step (256 threads x 4)
};
// the device form's limit of h (1 + 3 w): 15 bits per byte keep every bit offset below 2^31
static const uint64_t PNGE_MAX_STREAM = (uint64_t)1 << 27;
static const uint64_t PNGE_MAX_ITEMS = 0x7fffffffull;      // a one-dimensional grid holds no more workgroups

struct PngeImg {            // one image of a call
  uint64_t pix_off;         // byte offset of its first BGR pixel in the call's source
  uint64_t pitch;           // bytes from one pixel row to the next, >= 3 w
  uint64_t n;               // stream bytes: h (1 + 3 w)
  uint64_t word0, nwords;   // its part of the DEFLATE words
  uint32_t h, w, stride;    // stride = 1 + 3 w
  uint32_t npieces, piece0; // pieces; its first entry in the per-piece arrays
  uint32_t far_ok;          // stride <= 32768: the row above is within DEFLATE's window
  uint32_t far_bits, far_len;      // a far match's distance: the 1-bit code of symbol S (a 1) with the extra bits behind it; their count
  uint32_t dsym;            // S: the distance symbol of stride (the dummy symbol 1 when stride > 32768); HDIST covers 0 .. S
  uint32_t group0;          // its first work item: prefix sum of the images' ceil(npieces / PNGE_GROUP)
};

struct PngeCodes {          // per image, built on the host from the histogram
  uint32_t ll[PNGE_NSYM];   // length << 16 | code, bit-reversed (DEFLATE packs Huffman codes from their most significant bit); 0 = unused
  uint32_t hdr[PNGE_HDR_WORDS];    // the block header's bits, LSB first
  uint32_t hdr_bits, pad_;
};

struct PngeRes {            // what comes back per image
  uint32_t flag;            // 0, or PNGE_FLAG_*: the host form codes this image
  uint32_t bytes;           // the DEFLATE block's bytes, padded
  uint32_t adler;
  uint32_t bits;
};

struct PngeLen { uint32_t bits, a, b, pad_; };      // per piece: its bits (after the scan: its bit offset), sum b, sum (len - j) b_j

// the filtered byte c of row y (c = 0: the filter type); rows are `pitch` bytes apart. Reads the pixel's byte and its left neighbour's
PNGE_HD uint32_t pnge_byte(const uint8_t* img, uint64_t pitch, uint32_t y, uint32_t c) {
  if (c == 0) return 1u;
  const uint32_t x = c - 1u, q = x / 3u, k = x - 3u * q;
  const uint8_t* p = img + (size_t)y * (size_t)pitch + (size_t)q * 3u + (2u - k);
  uint32_t v = p[0];
  if (x >= 3u) v -= p[-3];
  return v & 0xffu;
}

// length L (3 .. 258) -> length symbol 257 + k, its extra bits
PNGE_HD void pnge_lsym(uint32_t L, uint32_t& k, uint32_t& ebits, uint32_t& eval) {
  const uint32_t l = L - 3u;
  if (L == 258u) { k = 28u; ebits = 0u; eval = 0u; return; }
  if (l < 8u) { k = l; ebits = 0u; eval = 0u; return; }
  const uint32_t e = (uint32_t)(31 - __builtin_clz(l)) - 2u;
  const uint32_t r = l - (4u << e);
  k = 4u * (e + 1u) + (r >> e); ebits = e; eval = r & ((1u << e) - 1u);
}

// piece p of the image: its tokens into the sink. Sink: lit(v); match(L, far); and, if Sink::BYTES, the bytes a match covers: run(b, L)
// for a near one, byte(v) L times for a far one
template <class Sink>
PNGE_HD void pnge_piece(const PngeImg& im, const uint8_t* img, uint64_t p, Sink& s) {
  const uint64_t p0 = p * (uint64_t)PNGE_P;
  const uint32_t len = (uint32_t)(im.n - p0 < (uint64_t)PNGE_P ? im.n - p0 : (uint64_t)PNGE_P);
  const uint32_t stride = im.stride;
  const uint64_t w = im.pitch;      // (what pnge_byte addresses a row by)
  uint32_t y = (uint32_t)(p0 / stride), c = (uint32_t)(p0 - (uint64_t)y * stride);
  bool have_prev = p0 >= 1;
  uint32_t prev = 0;
  if (have_prev) prev = c ? pnge_byte(img, w, y, c - 1u) : pnge_byte(img, w, y - 1u, stride - 1u);
  for (uint32_t i = 0; i < len;) {      // (PNGE_P rounds at most)
    const uint32_t room = len - i < 258u ? len - i : 258u;
    bool ok1 = have_prev, ok2 = im.far_ok && y >= 1u;      // position >= stride <=> y >= 1
    uint32_t L1 = 0, L2 = 0, v0 = 0, last2 = 0, ty = y, tc = c;
    for (uint32_t k = 0; k < room; ++k) {
      const uint32_t v = pnge_byte(img, w, ty, tc);
      if (k == 0) v0 = v;
      if (ok1) { if (v == prev) L1 = k + 1u; else ok1 = false; }
      if (ok2) { if (v == pnge_byte(img, w, ty - 1u, tc)) { L2 = k + 1u; last2 = v; } else ok2 = false; }
      if (!ok1 && !ok2) break;
      if (++tc == stride) { tc = 0; ++ty; }
    }
    const uint32_t L = L1 > L2 ? L1 : L2;
    uint32_t adv = 1;
    if (L >= 3u) {
      const bool far = L2 > L1;
      s.match(L, far);
      if (Sink::BYTES) {
        if (!far) {
          s.run(prev, L);
        } else {
          ty = y; tc = c;
          for (uint32_t k = 0; k < L; ++k) {
            s.byte(pnge_byte(img, w, ty, tc));
            if (++tc == stride) { tc = 0; ++ty; }
          }
        }
      }
      if (far) prev = last2;
      adv = L;
    } else {
      s.lit(v0);
      prev = v0;
    }
    have_prev = true;
    i += adv; c += adv;
    if (c >= stride) { const uint32_t q = c / stride; y += q; c -= q * stride; }
  }
}

struct PngeHist {
  uint32_t* cnt;            // 286 counters (the workgroup's, in LDS)
  static const bool BYTES = false;
  PNGE_HD void lit(uint32_t v) { BITS_ATOMIC_ADD(cnt + v, 1u); }
  PNGE_HD void match(uint32_t L, bool) { uint32_t k, eb, ev; pnge_lsym(L, k, eb, ev); BITS_ATOMIC_ADD(cnt + 257u + k, 1u); }
  PNGE_HD void run(uint32_t, uint32_t) {}
  PNGE_HD void byte(uint32_t) {}
};

// bits under the image's code, and Adler's two sums over the piece's bytes: s1 = sum b <= 65280, s2 = sum (len - j) b_j < 2^24
struct PngeCount {
  const uint32_t* ll;
  uint32_t far_len, bits, s1, s2;
  static const bool BYTES = true;
  PNGE_HD void byte(uint32_t v) { s1 += v; s2 += s1; }
  PNGE_HD void run(uint32_t b, uint32_t L) { s2 += L * s1 + b * (L * (L + 1u) / 2u); s1 += L * b; }
  PNGE_HD void lit(uint32_t v) { bits += ll[v] >> 16; byte(v); }
  PNGE_HD void match(uint32_t L, bool far) { uint32_t k, eb, ev; pnge_lsym(L, k, eb, ev); bits += (ll[257u + k] >> 16) + eb + (far ? far_len : 1u); }
};

// bits -> the image's words (WordSink, bits_dev.h), LSB first (a word's first stream byte is its lowest: the words are the bytes on a
// little-endian machine). The words a piece shares may hold several WHOLE pieces where the paper is flat. The index is 64 bits wide: the
// host form takes images beyond 2^32 bits
struct PngeWrite : WordSink<uint64_t> {
  const uint32_t* ll;
  uint32_t far_bits, far_len;
  uint64_t acc;             // the pending bits of word w are acc's lowest nb
  uint32_t nb;              // < 32 between two puts
  static const bool BYTES = false;
  PNGE_HD void start(const uint32_t* ll_, uint32_t fb, uint32_t fl, uint32_t* p, uint64_t n, uint64_t bit0) {
    WordSink<uint64_t>::start(p, n, bit0);
    ll = ll_; far_bits = fb; far_len = fl; acc = 0; nb = (uint32_t)(bit0 & 31u);
  }
  PNGE_HD uint64_t position() const { return WordSink<uint64_t>::position() + nb; }
  PNGE_HD void put(uint32_t v, uint32_t len) {      // len <= 16; v below 2^len
    acc |= (uint64_t)v << nb;
    nb += len;
    if (nb >= 32u) { emit((uint32_t)acc, true); acc >>= 32; nb -= 32u; }
  }
  PNGE_HD void sym(uint32_t e) { put(e & 0xffffu, e >> 16); }
  PNGE_HD void lit(uint32_t v) { sym(ll[v]); }
  PNGE_HD void match(uint32_t L, bool far) {
    uint32_t k, eb, ev;
    pnge_lsym(L, k, eb, ev);
    sym(ll[257u + k]);
    if (eb) put(ev, eb);
    if (far) put(far_bits, far_len); else put(0u, 1u);
  }
  PNGE_HD void run(uint32_t, uint32_t) {}
  PNGE_HD void byte(uint32_t) {}
  PNGE_HD void finish() { if (nb) { emit((uint32_t)acc, false); nb = 0; } }
};

struct PngeItem { uint32_t img, piece; };      // a work item: its image, and the first piece of its group

// item: 0 <= item < the table's total (the grid covers exactly that many). Every image has at least one item, so group0 rises strictly:
// the last image whose first item is not behind it, a search over at most log2(n) + 1 entries
PNGE_HD PngeItem pnge_locate(const PngeImg* imgs, uint32_t n, uint32_t item) {
  uint32_t lo = 0, hi = n - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (imgs[mid].group0 <= item) lo = mid; else hi = mid - 1u;
  }
  PngeItem p;
  p.img = lo; p.piece = (item - imgs[lo].group0) * (uint32_t)PNGE_GROUP;
  return p;
}

// ---- the passes, one call per thread -----------------------------------------------------------------------------------------------

// hist pass: thread s of image im. cnt: the 286 counters this thread's workgroup shares
PNGE_HD void pnge_hist_thread(const PngeImg& im, uint32_t s, const uint8_t* px, uint32_t* cnt) {
  if (s >= im.npieces) return;
  PngeHist hs;
  hs.cnt = cnt;
  pnge_piece(im, px + im.pix_off, s, hs);
  if (s == im.npieces - 1u) BITS_ATOMIC_ADD(cnt + PNGE_EOB, 1u);
}

// length pass: thread s of image im. ll: the image's code; out: the per-piece array. The last piece carries EOB
PNGE_HD void pnge_length_thread(const PngeImg& im, uint32_t s, const uint8_t* px, const uint32_t* ll, PngeLen* out) {
  if (s >= im.npieces) return;
  PngeCount c;
  c.ll = ll; c.far_len = im.far_len; c.bits = 0; c.s1 = 0; c.s2 = 0;
  pnge_piece(im, px + im.pix_off, s, c);
  if (s == im.npieces - 1u) c.bits += ll[PNGE_EOB] >> 16;
  PngeLen r;
  r.bits = c.bits; r.a = c.s1; r.b = c.s2; r.pad_ = 0;
  out[im.piece0 + s] = r;
}

// write pass: thread s of image im. off: the per-piece array after the scan; words: the call's DEFLATE words, cleared. The first
// PNGE_HDR_WORDS threads (there are always that many: whole workgroups run) put the header's words down
PNGE_HD void pnge_write_thread(const PngeImg& im, uint32_t s, const uint8_t* px, const uint32_t* ll, const uint32_t* hdr, const PngeLen* off, uint32_t* words, uint32_t* flag) {
  uint32_t bad = 0;
  if (s < (uint32_t)PNGE_HDR_WORDS && hdr[s]) {
    if ((uint64_t)s < im.nwords) BITS_ATOMIC_OR(words + im.word0 + s, hdr[s]); else bad = PNGE_FLAG_STORE;
  }
  if (s < im.npieces && !*flag) {
    PngeWrite wr;
    wr.start(ll, im.far_bits, im.far_len, words + im.word0, im.nwords, off[im.piece0 + s].bits);
    pnge_piece(im, px + im.pix_off, s, wr);
    if (s == im.npieces - 1u) wr.sym(ll[PNGE_EOB]);
    wr.finish();
    bad |= wr.bad;
  }
  if (bad) BITS_ATOMIC_OR(flag, bad);
}

// Adler-32 of the stream from the pieces' partials: s1 = 1 + sum A_p, s2 = n + sum_p [(n - end_p) A_p + B_p], mod 65521. One piece's
// terms, reduced, are added to sa / ss (64-bit: 2^35 at most for 2^19 pieces); pnge_adler_final folds the sums
PNGE_HD void pnge_adler_term(uint64_t n, uint64_t end, uint32_t a, uint32_t b, uint64_t& sa, uint64_t& ss) {
  sa += a;
  ss += ((n - end) % 65521u) * a % 65521u + b % 65521u;
}
PNGE_HD uint32_t pnge_adler_final(uint64_t n, uint64_t sa, uint64_t ss) {
  const uint32_t s1 = (uint32_t)((1u + sa) % 65521u), s2 = (uint32_t)((n % 65521u + ss) % 65521u);
  return (s2 << 16) | s1;
}
// the end of piece s in the stream
PNGE_HD uint64_t pnge_piece_end(const PngeImg& im, uint32_t s) { const uint64_t e = ((uint64_t)s + 1u) * PNGE_P; return e < im.n ? e : im.n; }
// what the scan leaves in the image's result record; carry: the block's bits, header included; sa, ss: the pieces' Adler terms
PNGE_HD void pnge_scan_finish(const PngeImg& im, uint32_t carry, uint64_t sa, uint64_t ss, PngeRes& r) {
  r.bits = carry;
  r.bytes = (carry >> 3) + ((carry & 7u) ? 1u : 0u);
  r.adler = pnge_adler_final(im.n, sa, ss);
  if ((uint64_t)r.bytes > im.nwords * 4u) BITS_ATOMIC_OR(&r.flag, (uint32_t)PNGE_FLAG_SIZE);
}

// ---- host only: ONE copy for the library's host form, the device form's host half and the test program ------------------------------

// the descriptor of an h x w image, dense (pitch 3 w; a table's caller sets pitch and, behind pnge_layout, pix_off); word0, nwords, piece0,
// group0: pnge_layout
inline void pnge_describe(PngeImg& I, int h, int w) {
  static const uint32_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  I = PngeImg();
  I.h = (uint32_t)h; I.w = (uint32_t)w; I.stride = 1u + 3u * (uint32_t)w;
  I.pitch = 3u * (uint64_t)w;
  I.n = (uint64_t)h * I.stride;
  I.npieces = (uint32_t)((I.n + PNGE_P - 1) / PNGE_P);
  I.far_ok = I.stride <= 32768u ? 1u : 0u;
  uint32_t S = 1;      // the dummy second distance symbol of a stream that has near matches only
  if (I.far_ok) for (S = 29; dbase[S] > I.stride; --S) {}
  const uint32_t dext = S < 4 ? 0u : S / 2u - 1u;
  I.far_bits = 1u | ((I.far_ok ? I.stride - dbase[S] : 0u) << 1);
  I.far_len = 1u + (I.far_ok ? dext : 0u);
  I.dsym = S;
}
// words of an image's part of the buffer: header, 15 bits per stream byte at most (a literal is one code; a match covers three bytes with
// 15 + 5 + 1 + 13 bits), EOB, and the last word
inline uint64_t pnge_words(const PngeImg& I) { return (1338u + 15u * I.n + 15u + 31u) / 32u + 1u; }

PNGE_HD uint32_t pnge_groups(const PngeImg& I) { return (I.npieces + (uint32_t)PNGE_GROUP - 1u) / (uint32_t)PNGE_GROUP; }

struct PngeTotals { uint64_t pix, pieces, words, items; };
// every image's part of every buffer of a call (the images described, of any sizes), its first work item, and the totals. pix_off is the
// dense packing's (image after image at pitch 3 w); a table over a source of its own sets pix_off behind this call. The caller keeps
// `pieces` below 2^32 and `items` at PNGE_MAX_ITEMS at most (pnge_totals_ok) before it uses piece0 / group0
inline void pnge_layout(PngeImg* imgs, size_t m, PngeTotals& t) {
  t = PngeTotals();
  for (size_t k = 0; k < m; ++k) {
    PngeImg& I = imgs[k];
    I.pix_off = t.pix; I.piece0 = (uint32_t)t.pieces; I.word0 = t.words; I.nwords = pnge_words(I); I.group0 = (uint32_t)t.items;
    t.pix += (uint64_t)I.h * I.w * 3u; t.pieces += I.npieces; t.words += I.nwords; t.items += pnge_groups(I);
  }
}
inline bool pnge_totals_ok(const PngeTotals& t) { return t.items <= PNGE_MAX_ITEMS && t.pieces < ((uint64_t)1 << 32); }

// code lengths of at most `limit` bits for the symbols with cnt > 0 (0 for the others): Huffman's lengths, and where they exceed the limit
// the Kraft sum is repaired -- clipped codes overdraw it; the deepest codes below the limit are lengthened until it holds, then codes are
// shortened again, longest first, until it is exactly 1 (a step of 2^-L always fits: the deficit is a multiple of the smallest term)
inline void pnge_build_lengths(const uint32_t* cnt, int nsym, int limit, uint8_t* len) {
  std::vector<int> used;
  for (int i = 0; i < nsym; ++i) { len[i] = 0; if (cnt[i]) used.push_back(i); }
  const int m = (int)used.size();
  if (m == 0) return;
  if (m == 1) { len[used[0]] = 1; return; }
  // Huffman: leaves sorted by (count, symbol), two queues
  std::sort(used.begin(), used.end(), [&](int a, int b) { return cnt[a] != cnt[b] ? cnt[a] < cnt[b] : a < b; });
  std::vector<uint64_t> wt((size_t)2 * m - 1);
  std::vector<int> parent((size_t)2 * m - 1, -1);
  for (int i = 0; i < m; ++i) wt[i] = cnt[used[i]];
  int leaf = 0, node = m, next = m;
  auto take = [&]() { if (leaf < m && (node >= next || wt[leaf] <= wt[node])) return leaf++; return node++; };
  for (; next < 2 * m - 1; ++next) {
    const int a = take(), b = take();
    wt[next] = wt[a] + wt[b]; parent[a] = next; parent[b] = next;
  }
  std::vector<int> depth((size_t)2 * m - 1, 0);
  for (int i = 2 * m - 3; i >= 0; --i) depth[i] = depth[parent[i]] + 1;
  uint64_t kraft = 0;      // in units of 2^-limit
  const uint64_t one = (uint64_t)1 << limit;
  std::vector<int> L((size_t)m);
  for (int i = 0; i < m; ++i) { L[i] = std::min(depth[i], limit); kraft += one >> L[i]; }
  while (kraft > one) {      // lengthen the least frequent of the deepest codes below the limit
    int best = -1;
    for (int i = 0; i < m; ++i) if (L[i] < limit && (best < 0 || L[i] > L[best])) best = i;
    kraft -= one >> (L[best] + 1); ++L[best];
  }
  while (kraft < one) {      // shorten the most frequent of the longest codes whose step fits
    int best = -1;
    for (int i = m - 1; i >= 0; --i) if (L[i] > 1 && (one >> L[i]) <= one - kraft && (best < 0 || L[i] > L[best])) best = i;
    kraft += one >> L[best]; --L[best];
  }
  for (int i = 0; i < m; ++i) len[used[i]] = (uint8_t)L[i];
}

// canonical codes (RFC 1951 3.2.2) of the lengths
inline void pnge_canonical(const uint8_t* len, int nsym, uint32_t* code) {
  uint32_t next[17] = {0}, count[17] = {0};
  for (int i = 0; i < nsym; ++i) ++count[len[i]];
  count[0] = 0;
  for (int b = 1; b <= 16; ++b) next[b] = (next[b - 1] + count[b - 1]) << 1;
  for (int i = 0; i < nsym; ++i) code[i] = len[i] ? next[len[i]]++ : 0u;
}
inline uint32_t pnge_reverse(uint32_t v, int bits) { uint32_t r = 0; for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1u) << (bits - 1 - i); return r; }

// the image's literal/length code from its histogram, and the dynamic block's header: BFINAL = 1, BTYPE = 2, HLIT = 29, HDIST = S,
// HCLEN = 15; the code-length code gives each of 0 .. 15 four bits (symbol l's canonical code is l) and 16 / 17 / 18 none; the distance
// code gives symbol 0 and symbol S one bit each
inline void pnge_build_codes(const PngeImg& I, const uint32_t* cnt, PngeCodes& C) {
  static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint8_t len[PNGE_NSYM];
  uint32_t code[PNGE_NSYM];
  pnge_build_lengths(cnt, PNGE_NSYM, 15, len);
  pnge_canonical(len, PNGE_NSYM, code);
  std::memset(&C, 0, sizeof(C));
  for (int i = 0; i < PNGE_NSYM; ++i) C.ll[i] = len[i] ? ((uint32_t)len[i] << 16) | pnge_reverse(code[i], len[i]) : 0u;
  uint32_t at = 0;
  auto put = [&](uint32_t v, uint32_t n) { for (uint32_t k = 0; k < n; ++k, ++at) C.hdr[at >> 5] |= ((v >> k) & 1u) << (at & 31u); };
  const uint32_t S = I.dsym;
  put(1, 1); put(2, 2); put(PNGE_NSYM - 257, 5); put(S, 5); put(19 - 4, 4);
  for (int k = 0; k < 19; ++k) put(order[k] < 16 ? 4u : 0u, 3);
  for (int i = 0; i < PNGE_NSYM; ++i) put(pnge_reverse(len[i], 4), 4);
  for (uint32_t d = 0; d <= S; ++d) put(pnge_reverse(d == 0 || d == S ? 1u : 0u, 4), 4);
  C.hdr_bits = at;
}

// the file around a DEFLATE block: 8 + 25 + (8 + 2 + bytes + 4 + 4) + 12 bytes
enum { PNGE_FRAME_BYTES = 63, PNGE_FRAME_FRONT = 43 };
typedef uint32_t (*PngeCrc)(const uint8_t*, size_t);
static inline void pnge_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }
// out: the file's buffer of PNGE_FRAME_BYTES + bytes, whose DEFLATE block is already at out + PNGE_FRAME_FRONT
inline void pnge_frame(uint8_t* out, int h, int w, size_t bytes, uint32_t adler, PngeCrc crc) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  std::memcpy(out, sig, 8);
  pnge_be32(out + 8, 13); std::memcpy(out + 12, "IHDR", 4);
  pnge_be32(out + 16, (uint32_t)w); pnge_be32(out + 20, (uint32_t)h);
  out[24] = 8; out[25] = 2; out[26] = 0; out[27] = 0; out[28] = 0;
  pnge_be32(out + 29, crc(out + 12, 17));
  pnge_be32(out + 33, (uint32_t)(bytes + 6)); std::memcpy(out + 37, "IDAT", 4);
  out[41] = 0x78; out[42] = 0x01;
  uint8_t* p = out + PNGE_FRAME_FRONT + bytes;
  pnge_be32(p, adler);
  pnge_be32(p + 4, crc(out + 37, 4 + bytes + 6));
  pnge_be32(p + 8, 0); std::memcpy(p + 12, "IEND", 4);
  pnge_be32(p + 16, crc(p + 12, 4));
}

// upper bound of one file: at most 15 bits per stream byte behind a header of 1338 bits, EOB and padding -- (1338 + 15 n + 15 + 7) / 8
// < 2 n + 171 bytes -- plus the frame
inline size_t pnge_capacity(int h, int w) { return 2 * (size_t)h * (1 + 3 * (size_t)w) + 171 + PNGE_FRAME_BYTES; }

// the host form: every pass as a loop over the pieces. bytes_out: the file's size, whether or not it was written; returns false when
// capacity is below it (nothing written then)
inline bool pnge_encode_host(const uint8_t* bgr, int h, int w, uint8_t* out, size_t capacity, size_t* bytes_out, PngeCrc crc) {
  PngeImg I;
  pnge_describe(I, h, w);
  std::vector<uint32_t> cnt(PNGE_NSYM, 0u);
  PngeHist hs;
  hs.cnt = cnt.data();
  for (uint64_t p = 0; p < I.npieces; ++p) pnge_piece(I, bgr, p, hs);
  ++cnt[PNGE_EOB];
  PngeCodes C;
  pnge_build_codes(I, cnt.data(), C);
  uint64_t bits = C.hdr_bits, sa = 0, ss = 0;
  for (uint32_t p = 0; p < I.npieces; ++p) {
    PngeCount c;
    c.ll = C.ll; c.far_len = I.far_len; c.bits = 0; c.s1 = 0; c.s2 = 0;
    pnge_piece(I, bgr, p, c);
    bits += c.bits;
    pnge_adler_term(I.n, pnge_piece_end(I, p), c.s1, c.s2, sa, ss);
  }
  bits += C.ll[PNGE_EOB] >> 16;
  const size_t bytes = (size_t)((bits + 7) / 8);
  *bytes_out = bytes + PNGE_FRAME_BYTES;
  if (capacity < *bytes_out) return false;
  std::vector<uint32_t> words((bytes + 3) / 4 + 1, 0u);
  for (int k = 0; k < PNGE_HDR_WORDS; ++k) if (C.hdr[k]) words[k] |= C.hdr[k];
  uint64_t at = C.hdr_bits;
  for (uint32_t p = 0; p < I.npieces; ++p) {
    PngeWrite wr;
    wr.start(C.ll, I.far_bits, I.far_len, words.data(), words.size(), at);
    pnge_piece(I, bgr, p, wr);
    if (p == I.npieces - 1u) wr.sym(C.ll[PNGE_EOB]);
    at = wr.position();
    wr.finish();
  }
  std::memcpy(out + PNGE_FRAME_FRONT, words.data(), bytes);
  pnge_frame(out, h, w, bytes, pnge_adler_final(I.n, sa, ss), crc);
  return true;
}

}  // namespace ctpn
