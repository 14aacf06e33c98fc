// The per-thread source of the device Huffman decoder (jpeg_huff.hip), in a header of its own so that ONE text serves two compilers, like
// jpeg_pixel.h: hipcc compiles it into the jh_* kernels; tests/jpeg_huff_host.cpp compiles the same text with g++ under ASan / UBSan and runs
// every pass as a plain loop over thread indices, so the decoder -- its bounds on damaged files above all -- is pinned on the CPU first.
//
// The decode is the self-synchronising one: a restart segment is cut into subsequences of S bits, one thread each. A thread that starts at
// a wrong bit position falls into step with the true decode after a few codes, so: pass 1 decodes every subsequence from its first bit with
// a fresh state and stores the exit state; each sync round re-decodes subsequence i from the stored exit state of i - 1, until no exit state
// changes; a scan of the blocks begun per subsequence then tells every thread which blocks it is in, and the write pass decodes once more
// and stores the coefficients. All of it is integer arithmetic. Every loop is bounded by the bits of the subsequence: a code takes at
// least one bit. Nothing a file's bits say is used as an address without a range check (JhWrite::store, jh_peek16).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef JH_HD
#define JH_HD __host__ __device__ __forceinline__
#endif

namespace ctpn {

// per-file flag word: 0 = the device's coefficients are the host half's; anything else = the host half decodes this file
enum : uint32_t {
  JH_FLAG_CODE = 1,         // a bit pattern that is no code of the table
  JH_FLAG_DC_CAT = 2,       // DC category above 11
  JH_FLAG_RUN = 4,          // AC run past coefficient 63
  JH_FLAG_OVERRUN = 8,      // a code of a block the frame needs ends behind the segment's last bit
  JH_FLAG_COUNT = 16,       // a segment holds fewer blocks than its MCUs need
  JH_FLAG_UNSETTLED = 32,   // exit states still changing after the rounds run so far (the host runs more, up to the cap)
  JH_FLAG_SEGMENTS = 64     // host pass: fewer restart segments than the frame needs
};

enum { JH_MAX_TABLES = 6, JH_MAX_PATTERN = 6, JH_SUBSEQ_DEFAULT = 1024, JH_SUBSEQ_MIN = 128, JH_SUBSEQ_MAX = 4096 };

// one Huffman table: the host decoder's 9-bit lookup (length << 8 | symbol, 0 = longer than 9 bits) + canonical tail for lengths 10 .. 16
struct JhTable {
  uint16_t fast[512];
  int32_t maxcode[7];       // largest code of length 10 + j, -1 if none
  int32_t valoff[7];        // index of that length's first value minus its first code
  uint8_t vals[256];
};

struct JhSeg {              // one restart segment of one file
  uint32_t byte0;           // first byte, relative to the file's unstuffed bytes
  uint32_t nbits;
  uint32_t mcu0, nmcu;      // first MCU (scan order) and MCU count
  uint32_t sub0, nsub;      // first subsequence (batch-wide index) and their number (at least 1)
  uint32_t file, pad_;
};

struct JhFile {
  long long coef_base;      // int16 offset of the file's coefficient block
  long long coef_off[3];    // ... of component c inside it
  uint32_t bytes_off;       // byte offset (a multiple of 4) of the unstuffed scan bytes inside the byte block
  uint32_t nwords;          // 32-bit words of it that may be read (the bytes, zero-padded)
  uint32_t seg0, nseg;
  uint32_t tab0, ntab;      // the file's tables inside the table block
  int32_t ncomp, bpm;       // components; blocks per MCU
  int32_t mcux, mcuy;
  int32_t hs[3], vs[3], bw[3];
  uint8_t pat_comp[JH_MAX_PATTERN + 2];      // block b of the MCU pattern: its component ...
  uint8_t dc_tab[4], ac_tab[4];              // component c's tables (index into the file's tables)
};

struct JhState {            // decoder state between two codes
  uint32_t p;               // bit position inside the segment
  uint32_t bk;              // block index within the MCU pattern << 8 | zigzag position k (0: a DC code comes next)
};

JH_HD bool jh_same(const JhState& a, const JhState& b) { return a.p == b.p && a.bk == b.bk; }

JH_HD uint32_t jh_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// the file's bytes as the bit reader sees them: a window of two words, reloaded when the position leaves it
struct JhBits {
  const uint32_t* words;    // the file's unstuffed bytes (word-aligned, zero-padded to nwords)
  uint32_t nwords;
  uint32_t bit0;            // the segment's first bit inside them
  uint32_t nbits;           // the segment's length: bits behind it read as zero (JBits::fill feeds zeros behind a marker)
  uint32_t cw;              // cached word index (0xffffffff: none)
  uint32_t c0, c1;
};

JH_HD void jh_bits_init(JhBits& b, const uint32_t* words, uint32_t nwords, uint32_t byte0, uint32_t nbits) {
  b.words = words; b.nwords = nwords; b.bit0 = byte0 * 8u; b.nbits = nbits; b.cw = 0xffffffffu; b.c0 = b.c1 = 0;
}

// 16 bits from segment position p, zeros behind the segment's end
JH_HD uint32_t jh_peek16(JhBits& b, uint32_t p) {
  if (p >= b.nbits) return 0;
  const uint32_t a = b.bit0 + p, wi = a >> 5;
  if (wi != b.cw) {
    // (wi < nwords follows from p < nbits on a well-formed descriptor; the test keeps a damaged one inside the block all the same)
    b.c0 = wi < b.nwords ? jh_bswap(b.words[wi]) : 0u;
    b.c1 = wi + 1 < b.nwords ? jh_bswap(b.words[wi + 1]) : 0u;
    b.cw = wi;
  }
  const uint64_t win = ((uint64_t)b.c0 << 32) | b.c1;
  uint32_t v = (uint32_t)((win << (a & 31u)) >> 48);
  const uint32_t left = b.nbits - p;
  if (left < 16u) v &= 0xffffu << (16u - left);
  return v;
}

// one code at p: its symbol, or -1 for a pattern that is no code (16 bits are consumed then); len = the bits consumed
JH_HD int jh_code(const JhTable& t, uint32_t look, uint32_t& len) {
  const uint32_t e = t.fast[look >> 7];
  if (e >> 8) { len = e >> 8; return (int)(e & 0xffu); }
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int32_t code = (int32_t)(look >> (6 - j));
    if (code <= t.maxcode[j]) { len = 10u + j; return (int)t.vals[(uint32_t)(t.valoff[j] + code) & 0xffu]; }
  }
  len = 16u;
  return -1;
}

JH_HD int jh_extend(uint32_t v, int t) { return t == 0 ? 0 : ((int)v >= (1 << (t - 1)) ? (int)v : (int)v - (1 << t) + 1); }

// t bits (0 .. 15) at p
JH_HD uint32_t jh_get(JhBits& b, uint32_t p, int t) { return t ? jh_peek16(b, p) >> (16 - t) : 0u; }

#define JH_ZIGZAG_INIT {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, \
                        57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// what the write pass adds to the decode: where the blocks go. Block j of the segment (scan order) is block j % bpm of MCU mcu0 + j / bpm;
// blocks from seg_blocks on are the segment's trailing pad bits read as codes: the host decoder never reads them, so they are neither
// stored nor flagged
struct JhWrite {
  int16_t* coef;            // the file's coefficient block
  const uint8_t* zz;        // zigzag -> natural order
  const JhFile* f;
  uint32_t mcu0;
  long long seg_blocks;     // blocks the segment's MCUs need
  long long blk;            // the current block's index inside the segment (-1: none yet)
  int16_t* dst;             // ... and its 64 coefficients, null if it is not one of the frame's
  uint32_t flags;

  JH_HD void begin_block(long long j) {
    blk = j; dst = nullptr;
    if (j < 0 || j >= seg_blocks) return;
    const uint32_t mcu = mcu0 + (uint32_t)(j / f->bpm);
    int b = (int)(j % f->bpm);
    if (mcu >= (uint32_t)f->mcux * (uint32_t)f->mcuy) return;
    const int c = f->pat_comp[b];
    for (int q = 0; q < c; ++q) b -= f->hs[q] * f->vs[q];      // the block's index inside its component's part of the MCU
    const int by = b / f->hs[c], bx = b - by * f->hs[c];
    const int my = (int)(mcu / (uint32_t)f->mcux), mx = (int)(mcu - (uint32_t)my * (uint32_t)f->mcux);
    dst = coef + f->coef_off[c] + ((long long)(my * f->vs[c] + by) * f->bw[c] + (mx * f->hs[c] + bx)) * 64;
  }
  JH_HD bool live() const { return dst != nullptr; }
  JH_HD void store(int k, int v) { if (dst && k >= 0 && k < 64) dst[zz[k]] = (int16_t)v; }
};

// Decode the codes that START in [st.p, end) from state st; on return st is the exit state (st.p >= end unless nothing was left to do) and
// begun the number of blocks whose DC code was among them. W = nullptr: states only (pass 1, sync rounds). The loop runs at most
// end - st.p times: a code takes at least one bit. Conditions the host decoder refuses (an invalid code, DC category > 11, a run past 63)
// are decoded on by a fixed rule -- the states of a wrong guess must still be reproducible -- and, in the write pass, flagged.
JH_HD void jh_decode_sub(JhBits& bits, const JhFile& f, const JhTable* tabs, uint32_t end, JhState& st, uint32_t& begun, JhWrite* W, long long blk_base) {
  uint32_t p = st.p;
  int b = (int)(st.bk >> 8), k = (int)(st.bk & 0xffu);
  if (b >= f.bpm || b >= JH_MAX_PATTERN) b = 0;
  if (k > 63) k = 0;
  begun = 0;
  if (W) W->begin_block(k ? blk_base - 1 : -1);      // entered inside a block: the one begun last before this subsequence
  const uint32_t bound = end > p ? end - p : 0u;
  for (uint32_t it = 0; it < bound && p < end; ++it) {
    const int c = f.pat_comp[b];
    uint32_t len;
    bool done = false;
    if (k == 0) {
      const int t = jh_code(tabs[f.dc_tab[c]], jh_peek16(bits, p), len);
      ++begun;
      if (W) {
        W->begin_block(blk_base + (long long)begun - 1);
        if (W->live() && t < 0) W->flags |= JH_FLAG_CODE;
        if (W->live() && t > 11) W->flags |= JH_FLAG_DC_CAT;
      }
      const int cat = t < 0 ? 0 : (t & 15);
      p += len;
      if (W) W->store(0, jh_extend(jh_get(bits, p, cat), cat));      // the DC DIFFERENCE: jh_dc_kernel sums them per segment
      p += (uint32_t)cat;
      k = 1;
    } else {
      const int rs = jh_code(tabs[f.ac_tab[c]], jh_peek16(bits, p), len);
      if (W && W->live() && rs < 0) W->flags |= JH_FLAG_CODE;
      const int r = rs < 0 ? 0 : rs >> 4, s = rs < 0 ? 0 : rs & 15;
      p += len;
      if (s == 0) {
        if (r != 15) done = true;
        else { k += 16; done = k > 63; }
      } else {
        k += r;
        if (k > 63) { if (W && W->live()) W->flags |= JH_FLAG_RUN; done = true; }
        else {
          if (W) W->store(k, jh_extend(jh_get(bits, p, s), s));
          ++k;
          done = k > 63;
        }
        p += (uint32_t)s;
      }
    }
    if (W && W->live() && p > bits.nbits) W->flags |= JH_FLAG_OVERRUN;
    if (done) { k = 0; b = b + 1 >= f.bpm ? 0 : b + 1; }
  }
  st.p = p;
  st.bk = ((uint32_t)b << 8) | (uint32_t)k;
}

// the state a segment's decode starts from, and pass 1's guess for a subsequence that starts at bit p
JH_HD JhState jh_fresh(uint32_t p) { JhState s; s.p = p; s.bk = 0; return s; }

// ---------------------------------------------------------------------------------------------
// host: the one linear pass over a scan's bytes, and the table form. No code is decoded here.
// ---------------------------------------------------------------------------------------------
// src[0 .. n): the file from the first byte of its entropy-coded data. Removes byte stuffing (FF 00 -> FF), stops at the first marker that is
// not RSTn (or at any marker when the file has no restart interval), cuts at every RSTn. dst needs n bytes. Fills byte0 / nbits / mcu0 /
// nmcu of at most max_segs segments -- the frame needs ceil(total_mcus / dri) of them, what follows is never read -- and returns how many
// it found; *nbytes = bytes written to dst.
inline int jh_unstuff_segments(const uint8_t* src, size_t n, uint32_t dri, uint32_t total_mcus, uint8_t* dst, JhSeg* segs, int max_segs, uint32_t* nbytes) {
  size_t i = 0;
  uint32_t o = 0, start = 0;
  int ns = 0;
  auto close = [&]() {
    JhSeg& s = segs[ns];
    s.byte0 = start; s.nbits = (o - start) * 8u;
    s.mcu0 = dri ? (uint32_t)ns * dri : 0u;
    s.nmcu = dri ? (total_mcus - s.mcu0 < dri ? total_mcus - s.mcu0 : dri) : total_mcus;
    s.sub0 = s.nsub = s.file = s.pad_ = 0;
    ++ns; start = o;
  };
  while (i < n && ns < max_segs) {
    const uint8_t b = src[i];
    if (b != 0xFF) { dst[o++] = b; ++i; continue; }
    if (i + 1 >= n) break;                                       // a lone FF at the end of the file
    const uint8_t m = src[i + 1];
    if (m == 0) { dst[o++] = 0xFF; i += 2; continue; }
    if (dri && m >= 0xD0 && m <= 0xD7) { close(); i += 2; continue; }
    break;
  }
  if (ns < max_segs) close();
  *nbytes = o;
  return ns;
}

// the table form from a DHT segment's 16 counts and its values; false for counts no canonical code has (jhuff_build's rule)
inline bool jh_build_table(JhTable& t, const uint8_t counts[16], const uint8_t* vals, int nvals) {
  for (int i = 0; i < 512; ++i) t.fast[i] = 0;
  for (int i = 0; i < 256; ++i) t.vals[i] = 0;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int first = code, kfirst = k;
    for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
      if (k >= nvals || k >= 256 || code >= (1 << l)) return false;
      t.vals[k] = vals[k];
      if (l <= 9) {
        const int lo = code << (9 - l), cnt = 1 << (9 - l);
        for (int j = 0; j < cnt; ++j) t.fast[lo + j] = (uint16_t)((l << 8) | vals[k]);
      }
    }
    if (l >= 10) { t.maxcode[l - 10] = counts[l - 1] ? code - 1 : -1; t.valoff[l - 10] = kfirst - first; }
    if (code > (1 << l)) return false;
    code <<= 1;
  }
  return true;
}

}  // namespace ctpn
