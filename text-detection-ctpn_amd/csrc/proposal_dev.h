// Device helpers shared by the units of the proposal layer (decode.hip, sort_keys.hip, nms.hip): what more than one of them needs, and nothing else.
#pragma once
#include "common.h"

namespace ctpn {

constexpr unsigned long long KEY_INVALID = 0xFFFFFFFFFFFFFFFFull;

// float -> uint32 whose unsigned order is the float order (negative values below positive ones); inverse below
__device__ __forceinline__ unsigned int score_order_bits(float f) {
  const unsigned int u = __builtin_bit_cast(unsigned int, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float score_from_order_bits(unsigned int o) {
  return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// column group of a box for the column-decomposed NMS kernels of nms.hip (16-px anchor grid; cs = im_scale for the connector's boxes / scale)
constexpr int NC_MAXN = 12288, NC_MAXCOL = 256, NC_TL_MAXN = 1024;
constexpr int NC_TL_LARGE_MAXN = 4096;      // the connector's NMS on a ctx whose capacity ctpn_reserve_proposals raised (CTPN_POST_NMS_CAPACITY_MAX)
__device__ __forceinline__ int nms_col_of(float x1, float cs, int ncols) {
  const int c = (int)(x1 * cs + 0.5f) >> 4;
  return c < 0 ? 0 : (c > ncols - 1 ? ncols - 1 : c);
}

// digit groups of a wave: the radix sort's (sort_keys.hip) and, with the column as the digit, the column NMS's partition of its ranks (nms.hip)
__device__ __forceinline__ unsigned long long rs_match(unsigned d, bool valid) {
  unsigned long long mask = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long bal = __ballot(bit);
    mask &= bit ? bal : ~bal;
  }
  return mask;      // lanes (valid ones) that hold the same digit as this lane
}

}  // namespace ctpn
