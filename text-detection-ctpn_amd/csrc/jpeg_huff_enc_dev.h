// The per-thread source of the device Huffman coder (jpeg_huff_enc.hip), in a header of its own so that ONE text serves two compilers, like
// jpeg_huff_dev.h: hipcc compiles it into the jhe_* kernels; tests/jpeg_huff_enc_host.cpp compiles the same text with g++ under ASan / UBSan
// and runs every pass as a plain loop over thread indices.
//
// Coding is the easy direction: a block's bits depend on its own 64 coefficients and on the DC of the previous block of its component in
// scan order, which lies in the coefficient array. So one thread takes one block, and the passes are
//   length   jhe_block into a sink that counts  -> bits per block, and the out-of-range verdict (DC difference above 11 bits, AC above 10)
//   scan     exclusive prefix sum per image     -> every block's bit offset, the image's total
//   write    jhe_block into a sink that writes  -> the UNSTUFFED stream, 32-bit words in byte order; a word that two blocks share is
//            combined with an atomic OR into a buffer that was cleared before (OR commutes: the bytes do not depend on the order); the
//            thread of the image's last block fills the last byte with 1-bits (jchuff.c flush_bits)
//   count    0xFF bytes per chunk of JHE_CHUNK unstuffed bytes; scan: exclusive prefix sum per image -> every chunk's stuffed offset
//   stuff    the scan body as the file holds it: 0x00 behind every 0xFF
// The length pass and the write pass run the SAME jhe_block: they cannot disagree. Every loop is bounded before it starts (64 coefficients,
// at most three ZRL codes per coefficient, JHE_CHUNK bytes); every store is checked against its buffer's size.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bits_dev.h"
#include "jpeg_enc_tables.h"

#define JHE_HD BITS_HD

namespace ctpn {

enum : uint32_t {
  JHE_FLAG_RANGE = 1,       // a DC difference above 11 bits or an AC coefficient above 10: the host half says so in its own words
  JHE_FLAG_STORE = BITS_FLAG_STORE, JHE_FLAG_SIZE = BITS_FLAG_SIZE
};

enum {
  JHE_BLOCK_BYTES = 208,    // bound of one block, unstuffed: 1660 bits (jpeg_encode_capacity)
  JHE_CHUNK = 64,           // unstuffed bytes per thread of the count and stuff passes
  JHE_SCAN_ITEMS = 1024,    // items one workgroup of the scan takes per step (256 threads x 4)
  JHE_MAX_BLOCKS = 1 << 20  // blocks per launch group (and so per image): bit offsets, word and byte offsets stay below 2^32
};

// code tables for the coder: length << 16 | code, 0 = no such symbol. tc: 0 = luma (K.3 / K.5), 1 = chroma (K.4 / K.6). nat: natural index
// of zig-zag position k
struct JheTables {
  uint32_t dc[2][16];
  uint32_t ac[2][256];
  uint8_t nat[64];
};

struct JheImg {             // one image of a launch group
  long long coef_off;       // int16 offset of its coefficients in the batch's block: [component][block rows][block columns][64] over the MCU grid
  uint32_t mcux, nmcu;      // MCUs per row; MCUs
  uint32_t hs, vs;          // luma sampling (chroma 1 x 1)
  uint32_t nblk, blk0;      // blocks; its first entry in the group's per-block array
  uint32_t word0, nwords;   // its part of the unstuffed stream, 32-bit words (JHE_BLOCK_BYTES / 4 per block)
  uint32_t chunk0, nchunk;  // its part of the per-chunk array
  uint32_t out0, out_cap;   // its part of the stuffed bytes (2 x JHE_BLOCK_BYTES per block)
};

struct JheRes {             // what comes back per image
  uint32_t flag;            // 0, or JHE_FLAG_*: the host half codes this image
  uint32_t bytes;           // the stuffed scan body's size
  uint32_t bits;            // the unstuffed stream's bits before padding
  uint32_t pad_;
};

// host only: canonical codes of a DHT segment's counts and values (ITU-T T.81 Annex C), packed for the coder
inline void jhe_build_codes(uint32_t* tab, const uint8_t bits[16], const uint8_t* vals) {
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) tab[vals[k]] = ((uint32_t)l << 16) | code;
    code <<= 1;
  }
}
inline void jhe_build_tables(JheTables& T) {
  T = JheTables();
  for (int tc = 0; tc < 2; ++tc) { jhe_build_codes(T.dc[tc], kBitsDc[tc], kValsDc); jhe_build_codes(T.ac[tc], kBitsAc[tc], kValsAc[tc]); }
  // the zig-zag walk of ITU-T T.81 figure 5
  int y = 0, x = 0;
  bool up = true;
  for (int k = 0; k < 64; ++k) {
    T.nat[k] = (uint8_t)(8 * y + x);
    if (up) { if (x == 7) { ++y; up = false; } else if (y == 0) { ++x; up = false; } else { --y; ++x; } }
    else { if (y == 7) { ++x; up = true; } else if (x == 0) { ++y; up = true; } else { ++y; --x; } }
  }
}

JHE_HD int jhe_nbits(int v) { return v ? 32 - __builtin_clz((unsigned)v) : 0; }

// block s of the image's scan order (MCU by MCU: the luma blocks of the MCU row-major, then Cb, then Cr): its coefficients' offset, its
// table class, and the scan-order index of the previous block of its component (-1: none, the prediction is 0)
JHE_HD long long jhe_locate(const JheImg& im, uint32_t s, int& tc, long long& prev) {
  const uint32_t nl = im.hs * im.vs, bpm = nl + 2;
  const uint32_t mcu = s / bpm, j = s - mcu * bpm;
  const uint32_t my = mcu / im.mcux, mx = mcu - my * im.mcux;
  const uint32_t mcuy = im.nmcu / im.mcux;
  long long off;
  if (j < nl) {
    const uint32_t by = j / im.hs, bx = j - by * im.hs;
    off = ((long long)(my * im.vs + by) * (im.mcux * im.hs) + (mx * im.hs + bx)) * 64;
    tc = 0;
    prev = j > 0 ? (long long)s - 1 : (mcu > 0 ? (long long)s - bpm + (nl - 1) : -1);
  } else {
    off = ((long long)mcuy * im.mcux * nl + (long long)(j - nl) * im.nmcu + ((long long)my * im.mcux + mx)) * 64;
    tc = 1;
    prev = mcu > 0 ? (long long)s - bpm : -1;
  }
  return im.coef_off + off;
}

// eight coefficients from zig-zag position 8 g on. ZZ: the block is in zig-zag order (one 16-byte load: a block is 128-byte aligned)
template <bool ZZ>
JHE_HD void jhe_load8(const int16_t* blk, int g, const uint8_t* nat, int16_t (&v)[8]) {
  if (ZZ) {
    __builtin_memcpy(v, (const int16_t*)__builtin_assume_aligned(blk, 16) + 8 * g, 16);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = blk[nat[8 * g + j]];
  }
}

// jchuff.c encode_one_block, as jenc_block (jpeg_enc.hip) restates it: false = a value baseline JPEG does not code (the sink then holds a
// prefix of the block and the image goes to the host half)
template <bool ZZ, class Sink>
JHE_HD bool jhe_block(Sink& s, const int16_t* blk, int pred, const JheTables& T, int tc) {
  const uint32_t* dc = T.dc[tc];
  const uint32_t* ac = T.ac[tc];
  const int diff = (int)blk[0] - pred;
  int nb = jhe_nbits(diff < 0 ? -diff : diff);
  if (nb > 11) return false;
  s.put(dc[nb] & 0xffffu, (int)(dc[nb] >> 16));
  if (nb) s.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u), nb);
  int run = 0;
  for (int g = 0; g < 8; ++g) {
    int16_t v8[8];
    jhe_load8<ZZ>(blk, g, T.nat, v8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (g == 0 && j == 0) continue;
      const int v = v8[j];
      if (!v) { ++run; continue; }
      for (; run > 15; run -= 16) s.put(ac[0xF0] & 0xffffu, (int)(ac[0xF0] >> 16));      // (three times at most: run <= 62)
      nb = jhe_nbits(v < 0 ? -v : v);
      if (nb > 10) return false;
      const uint32_t e = ac[(run << 4) | nb];
      s.put(e & 0xffffu, (int)(e >> 16));
      s.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u), nb);
      run = 0;
    }
  }
  if (run) s.put(ac[0] & 0xffffu, (int)(ac[0] >> 16));
  return true;
}

struct JheCount {
  uint32_t bits;
  JHE_HD void put(uint32_t, int len) { bits += (uint32_t)len; }
};

// bits -> the image's unstuffed words (WordSink, bits_dev.h), MSB first. A word's first stream byte is its lowest, a byte's first stream bit
// its highest: a full word is byte-swapped on its way out
struct JheWrite : WordSink<uint32_t> {
  uint64_t acc;             // the pending bits of word w are acc's lowest nb
  int nb;                   // < 32 between two puts
  JHE_HD void start(uint32_t* p, uint32_t n, uint32_t bit0) { WordSink<uint32_t>::start(p, n, bit0); acc = 0; nb = (int)(bit0 & 31u); }
  JHE_HD void put(uint32_t code, int len) {      // len <= 16
    acc = (acc << len) | code;
    nb += len;
    if (nb >= 32) { emit(__builtin_bswap32((uint32_t)(acc >> (nb - 32))), true); nb -= 32; }
  }
  JHE_HD uint32_t position() const { return WordSink<uint32_t>::position() + (uint32_t)nb; }
  JHE_HD void finish() { if (nb) { emit(__builtin_bswap32((uint32_t)(acc << (32 - nb))), false); nb = 0; } }
};

// ---- the passes, one call per thread -----------------------------------------------------------------------------------------------

// length pass: thread s of image im. len: the group's per-block array
template <bool ZZ>
JHE_HD void jhe_length_thread(const JheImg& im, uint32_t s, const int16_t* coef, const JheTables& T, uint32_t* len, uint32_t* flag) {
  if (s >= im.nblk) return;
  int tc;
  long long prev;
  const int16_t* blk = coef + jhe_locate(im, s, tc, prev);
  int ptc;
  long long pp;
  const int pred = prev < 0 ? 0 : (int)coef[jhe_locate(im, (uint32_t)prev, ptc, pp)];
  JheCount c;
  c.bits = 0;
  if (!jhe_block<ZZ>(c, blk, pred, T, tc)) BITS_ATOMIC_OR(flag, (uint32_t)JHE_FLAG_RANGE);
  len[im.blk0 + s] = c.bits;
}

// write pass: thread s of image im. off: the per-block array after the scan; uns: the group's unstuffed words, cleared
template <bool ZZ>
JHE_HD void jhe_write_thread(const JheImg& im, uint32_t s, const int16_t* coef, const JheTables& T, const uint32_t* off, uint32_t* uns, uint32_t* flag) {
  if (s >= im.nblk || *flag) return;
  int tc;
  long long prev;
  const int16_t* blk = coef + jhe_locate(im, s, tc, prev);
  int ptc;
  long long pp;
  const int pred = prev < 0 ? 0 : (int)coef[jhe_locate(im, (uint32_t)prev, ptc, pp)];
  JheWrite wr;
  wr.start(uns + im.word0, im.nwords, off[im.blk0 + s]);
  (void)jhe_block<ZZ>(wr, blk, pred, T, tc);
  if (s == im.nblk - 1) {      // jchuff.c flush_bits: the last byte is filled with 1-bits
    const int pad = (int)((8u - (wr.position() & 7u)) & 7u);
    if (pad) wr.put((1u << pad) - 1u, pad);
  }
  wr.finish();
  if (wr.bad) BITS_ATOMIC_OR(flag, wr.bad);
}

// the unstuffed bytes of an image whose length pass counted `bits`
JHE_HD uint32_t jhe_unstuffed_bytes(uint32_t bits) { return (bits >> 3) + ((bits & 7u) ? 1u : 0u); }

// count pass: thread q of image im counts the 0xFF bytes of its chunk. cnt: the group's per-chunk array
JHE_HD void jhe_count_thread(const JheImg& im, uint32_t q, uint32_t bits, const uint32_t* uns, uint32_t* cnt) {
  const uint32_t nbytes = jhe_unstuffed_bytes(bits);
  if (q >= im.nchunk || (uint64_t)q * JHE_CHUNK >= nbytes) return;
  const uint32_t b0 = q * JHE_CHUNK, b1 = b0 + JHE_CHUNK < nbytes ? b0 + JHE_CHUNK : nbytes;
  uint32_t n = 0;
  for (uint32_t wi = b0 >> 2; wi < (b1 + 3) >> 2 && wi < im.nwords; ++wi) {      // (16 words at most)
    const uint32_t v = uns[im.word0 + wi];
#pragma unroll
    for (int k = 0; k < 4; ++k) n += (wi * 4 + k < b1 && ((v >> (8 * k)) & 0xffu) == 0xffu) ? 1u : 0u;
  }
  cnt[im.chunk0 + q] = n;
}

// stuff pass: thread q of image im writes its chunk behind the 0xFF bytes of the chunks before it (pre: the per-chunk array after the scan)
JHE_HD void jhe_stuff_thread(const JheImg& im, uint32_t q, uint32_t bits, const uint32_t* uns, const uint32_t* pre, uint8_t* out, uint32_t* flag) {
  const uint32_t nbytes = jhe_unstuffed_bytes(bits);
  if (q >= im.nchunk || (uint64_t)q * JHE_CHUNK >= nbytes || *flag) return;
  const uint32_t b0 = q * JHE_CHUNK, b1 = b0 + JHE_CHUNK < nbytes ? b0 + JHE_CHUNK : nbytes;
  uint32_t at = b0 + pre[im.chunk0 + q];
  uint8_t* dst = out + im.out0;
  uint32_t bad = 0;
  for (uint32_t wi = b0 >> 2; wi < (b1 + 3) >> 2 && wi < im.nwords; ++wi) {
    const uint32_t v = uns[im.word0 + wi];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (wi * 4 + k >= b1) continue;
      const uint8_t b = (uint8_t)(v >> (8 * k));
      if (at < im.out_cap) dst[at] = b; else bad = JHE_FLAG_STORE;
      ++at;
      if (b == 0xff) {
        if (at < im.out_cap) dst[at] = 0; else bad = JHE_FLAG_STORE;
        ++at;
      }
    }
  }
  if (bad) BITS_ATOMIC_OR(flag, bad);
}

// the chunks the second scan sums: those the unstuffed bytes of `bits` fill
JHE_HD uint32_t jhe_chunk_count(uint32_t bits, const JheImg& im) {
  const uint32_t count = (jhe_unstuffed_bytes(bits) + JHE_CHUNK - 1) / JHE_CHUNK; return count < im.nchunk ? count : im.nchunk;
}
// what a scan leaves in the image's result record; carry: its total. CHUNKS = false: the blocks' bits. CHUNKS = true: the 0xFF bytes of
// the chunks of an unstuffed stream of `bits` -> the stuffed size, and whether both streams fit the image's parts
template <bool CHUNKS>
JHE_HD void jhe_scan_finish(const JheImg& im, uint32_t bits, uint32_t carry, JheRes& r) {
  if (!CHUNKS) { r.bits = carry; return; }
  const uint32_t nbytes = jhe_unstuffed_bytes(bits);
  r.bytes = nbytes + carry;
  if (nbytes > im.nwords * 4u || nbytes + carry > im.out_cap) BITS_ATOMIC_OR(&r.flag, (uint32_t)JHE_FLAG_SIZE);
}

// ---- host only: ONE copy for the library (api_jpeg_out.hip) and the test program --------------------------------------------------------
// the descriptor of an h x w image with hs x vs luma sampling (coef_off: the caller's; its parts: jhe_layout)
inline void jhe_describe(JheImg& I, int h, int w, int hs, int vs) {
  I = JheImg();
  I.hs = (uint32_t)hs; I.vs = (uint32_t)vs; I.mcux = (uint32_t)((w + 8 * hs - 1) / (8 * hs));
  I.nmcu = I.mcux * (uint32_t)((h + 8 * vs - 1) / (8 * vs)); I.nblk = I.nmcu * (uint32_t)(hs * vs + 2);
}
struct JheTotals { uint32_t blk, words, chunks, outb, max_blocks, max_chunks; };
// every image's part of every buffer of a launch group (the images described, JHE_MAX_BLOCKS blocks in all at most), and the buffers' sizes
inline void jhe_layout(JheImg* imgs, size_t m, JheTotals& t) {
  t = JheTotals();
  for (size_t k = 0; k < m; ++k) {
    JheImg& I = imgs[k];
    I.blk0 = t.blk; I.word0 = t.words; I.nwords = I.nblk * (JHE_BLOCK_BYTES / 4);
    I.chunk0 = t.chunks; I.nchunk = (I.nblk * JHE_BLOCK_BYTES + JHE_CHUNK - 1) / JHE_CHUNK;
    I.out0 = t.outb; I.out_cap = I.nblk * 2 * JHE_BLOCK_BYTES;
    t.blk += I.nblk; t.words += I.nwords; t.chunks += I.nchunk; t.outb += I.out_cap;
    t.max_blocks = I.nblk > t.max_blocks ? I.nblk : t.max_blocks; t.max_chunks = I.nchunk > t.max_chunks ? I.nchunk : t.max_chunks;
  }
}

}  // namespace ctpn
