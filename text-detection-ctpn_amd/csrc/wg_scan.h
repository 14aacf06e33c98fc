// The workgroup prefix sum of the codecs' scan kernels (jpeg_huff.hip, jpeg_huff_enc.hip, png_enc.hip), device only: 256 threads, wave64.
#pragma once
#include <stdint.h>

namespace ctpn {

// inclusive scan of one value per thread across a workgroup of 256 (wave64 shuffles, then the four wave totals through LDS); total: the
// workgroup's sum. Every thread calls it, the same number of times. Signed values scan exactly as their two's-complement words. Of the two
// barriers a step needs, the one between the wave totals' stores and their readers is in here. The CALLER owns the other: a __syncthreads()
// between this call's return and the next call, whose stores would overtake a reader still running (the end of the caller's step)
static __device__ __forceinline__ uint32_t wg_scan256(uint32_t v, uint32_t& total) {
  __shared__ uint32_t wsum[4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(v, d, 64); if (lane >= (uint32_t)d) v += t; }
  if (lane == 63u) wsum[w] = v;
  __syncthreads();
  uint32_t add = total = 0;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) { add += q < w ? wsum[q] : 0u; total += wsum[q]; }
  return v + add;
}

}  // namespace ctpn
