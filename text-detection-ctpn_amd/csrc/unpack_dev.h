// A stored activation as dense fp32 NHWC (include/ctpn_hip_train.h, ctpn_get_tensor_device): the per-thread text of unpack.hip's kernel as host +
// device functions. tests/unpack_host.cpp compiles this same text with g++ under ASan + UBSan and runs it over whole small maps.
//   up_bf16_to_f32 / up_f16_to_f32   exact widening from the bits (a NaN stays a NaN, quieted, as the hardware convert leaves it)
//   up_gate_col                      lstm_gate_col (bilstm.hip): TF gate column -> the device's permuted column, per direction
//   up_quad                          four consecutive output floats: border stripped, 16-bit values widened, hi + lo added, lstm_pre's gate
//                                    columns put back in TF's order, the pad columns of a row (ld > C) dropped
// Every C is a multiple of 4 and four consecutive TF gate columns are four consecutive device columns, so a quad never leaves its pixel and
// its source is one run of 4 values (split precision: one of hi, one of lo).
// Nothing here includes a HIP header.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define UP_HD __host__ __device__ inline
#else
#define UP_HD inline
#endif

namespace ctpn {

constexpr int UP_F32 = 0, UP_BF16 = 1, UP_F16 = 2, UP_SPLIT = 3;

// the source block: n images of (H + 2 border) x (W + 2 border) pixels of ld values; C of them, from column 0, are the tensor's
struct UnpackDesc {
  int n, H, W, C;
  int ld;           // values per stored pixel (split precision: 2 C or 3 C 16-bit values, hi first, lo at + C)
  int border;       // 1: conv and pool maps carry a one-pixel border
  int kind;         // UP_*
  int gates;        // 1: lstm_pre, 1024 columns in up_gate_col's order per 512
};

UP_HD float up_bits_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
UP_HD float up_bf16_to_f32(uint16_t b) { return up_bits_f32((uint32_t)b << 16); }
UP_HD float up_f16_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 31u, m = h & 0x3ffu;
  if (e == 31u) return up_bits_f32(sign | 0x7f800000u | (m << 13) | (m ? 0x400000u : 0u));
  if (e == 0u) {
    if (!m) return up_bits_f32(sign);
    e = 113u;      // m 2^-24 = 1.f 2^(e - 127) once bit 10 leads
    while (!(m & 0x400u)) { m <<= 1; --e; }
    return up_bits_f32(sign | (e << 23) | ((m & 0x3ffu) << 13));
  }
  return up_bits_f32(sign | ((e + 112u) << 23) | (m << 13));
}

UP_HD int up_gate_col(int c) {
  const int g = c >> 7, u = c & 127;
  return (u >> 4) * 64 + ((u >> 2) & 3) * 16 + g * 4 + (u & 3);
}

UP_HD size_t up_quads(const UnpackDesc& d) { return (size_t)d.n * d.H * d.W * d.C / 4; }

// the first source value of output quad q
UP_HD size_t up_src_index(const UnpackDesc& d, size_t q) {
  const size_t e = q * 4, pix = e / (size_t)d.C;
  const int ch = (int)(e - pix * (size_t)d.C);
  const size_t row = pix / (size_t)d.W, img = row / (size_t)d.H;
  const int x = (int)(pix - row * (size_t)d.W), y = (int)(row - img * (size_t)d.H);
  const size_t Hs = (size_t)d.H + 2 * d.border, Ws = (size_t)d.W + 2 * d.border;
  const int col = d.gates ? (ch & ~511) + up_gate_col(ch & 511) : ch;
  return ((img * Hs + (size_t)(y + d.border)) * Ws + (size_t)(x + d.border)) * (size_t)d.ld + (size_t)col;
}

// out[0..3] = the tensor's floats 4 q .. 4 q + 3
UP_HD void up_quad(const void* src, const UnpackDesc& d, size_t q, float out[4]) {
  const size_t s = up_src_index(d, q);
  if (d.kind == UP_F32) {
    const float* p = (const float*)__builtin_assume_aligned((const float*)src + s, 16);
    for (int k = 0; k < 4; ++k) out[k] = p[k];
    return;
  }
  const uint16_t* p = (const uint16_t*)__builtin_assume_aligned((const uint16_t*)src + s, 8);
  uint16_t a[4];
  for (int k = 0; k < 4; ++k) a[k] = p[k];
  if (d.kind == UP_SPLIT) {
    const uint16_t* pl = (const uint16_t*)__builtin_assume_aligned(p + d.C, 8);
    for (int k = 0; k < 4; ++k) out[k] = up_bf16_to_f32(a[k]) + up_bf16_to_f32(pl[k]);
  } else if (d.kind == UP_F16) {
    for (int k = 0; k < 4; ++k) out[k] = up_f16_to_f32(a[k]);
  } else {
    for (int k = 0; k < 4; ++k) out[k] = up_bf16_to_f32(a[k]);
  }
}

}  // namespace ctpn
