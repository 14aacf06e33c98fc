// ctpn_get_tensor_device's kernel: a stored activation -> dense fp32 NHWC in HBM (the per-thread text: unpack_dev.h). One thread per four
// output floats: a 16-byte (fp32) or 8-byte (16-bit; split precision: two of them) load and one 16-byte store where the output is 16-byte
// aligned, four 4-byte stores otherwise. A streaming copy: nothing is reused, so no LDS.
#include "common.h"
#include "unpack_dev.h"

namespace ctpn {

typedef __attribute__((ext_vector_type(4))) float up_f32x4;

template <bool ALIGNED>
__global__ __launch_bounds__(256) void unpack_kernel(const void* __restrict__ src, UnpackDesc d, size_t quads, float* __restrict__ out) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  float v[4];
  up_quad(src, d, q, v);
  if (ALIGNED) ((up_f32x4*)out)[q] = up_f32x4{v[0], v[1], v[2], v[3]};
  else
#pragma unroll
    for (int k = 0; k < 4; ++k) out[q * 4 + k] = v[k];
}

int launch_unpack(const void* src, const UnpackDesc& d, float* out, hipStream_t s) {
  if (d.C % 4 || d.ld < d.C || (d.gates && d.C != 1024)) return fail(CTPN_ERR_ARG, "unpack: C is a multiple of 4 within ld (lstm_pre: 1024)");
  const size_t quads = up_quads(d);
  if (!quads) return CTPN_OK;
  const size_t groups = (quads + 255) / 256;
  if (groups > 0x7fffffffULL) return fail(CTPN_ERR_ARG, "unpack: tensor beyond 2^41 floats");
  if ((reinterpret_cast<uintptr_t>(out) & 15) == 0) hipLaunchKernelGGL(unpack_kernel<true>, dim3((unsigned)groups), dim3(256), 0, s, src, d, quads, out);
  else hipLaunchKernelGGL(unpack_kernel<false>, dim3((unsigned)groups), dim3(256), 0, s, src, d, quads, out);
  return launch_status("unpack");
}

}  // namespace ctpn
