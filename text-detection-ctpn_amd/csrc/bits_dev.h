// What the device bit-stream writers (jpeg_huff_enc_dev.h, png_enc_dev.h) share per thread: two flag values, the host / device switch of
// the atomics, the word sink under both accumulators. ONE text for hipcc and g++ (tests/*_host.cpp define the HIP qualifiers away).
#pragma once
#include <stdint.h>

#ifndef BITS_HD
#define BITS_HD __host__ __device__ __forceinline__
#endif
// an OR into a word / an add to a counter other threads may touch at the same time. On the host (the library's host forms and the test
// programs) an image's threads run one after the other: plain ones
#if defined(__HIP_DEVICE_COMPILE__)
#define BITS_ATOMIC_OR(p, v) atomicOr((p), (v))
#define BITS_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#else
#define BITS_ATOMIC_OR(p, v) (*(p) |= (v))
#define BITS_ATOMIC_ADD(p, v) (*(p) += (v))
#endif

namespace ctpn {

enum : uint32_t {           // bits of an image's result flag (1 is the JPEG coder's own: JHE_FLAG_RANGE)
  BITS_FLAG_STORE = 2,      // a store outside the image's part of a buffer was asked for (and not made): a count did not come out
  BITS_FLAG_SIZE = 4        // the totals do not fit the image's parts
};

// 32-bit words of a bit stream into the image's part of a cleared buffer. The first word a thread touches and its last, partial one may hold
// other threads' bits: those are ORed in (OR commutes: the bytes do not depend on the order). A word flushed full behind the first is the
// thread's alone and stored whole. An OR of zero is skipped: it is a no-op, so skipping it cannot change a byte. Every store is checked against
// the part's size; a refused one raises BITS_FLAG_STORE in `bad`. Index: the width of a word index and of a bit offset
template <class Index>
struct WordSink {
  uint32_t* words;          // the image's part
  Index nwords, w;          // w: the word the pending bits belong to
  bool shared;              // nothing emitted yet: the next word may hold another thread's bits
  uint32_t bad;
  BITS_HD void start(uint32_t* p, Index n, Index bit0) { words = p; nwords = n; w = bit0 >> 5; shared = true; bad = 0; }
  BITS_HD void emit(uint32_t v, bool whole) {
    if (w >= nwords) bad = BITS_FLAG_STORE;
    else if (whole && !shared) words[w] = v;
    else if (v) BITS_ATOMIC_OR(words + w, v);
    ++w;
    shared = false;
  }
  BITS_HD Index position() const { return w * 32u; }      // the bit offset of word w
};

}  // namespace ctpn
