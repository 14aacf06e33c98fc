// The one-time weight repack: TF variable layout -> [out][k] rows used by the conv / GEMM kernels (at weight load).
#include <type_traits>

#include "common.h"

namespace ctpn {

__device__ __forceinline__ uint16_t f2bf(float f) { return ctpn_f32_to_bf16(f); }

// ---------------------------------------------------------------------------------------------
// pack: dst[c][r] = src[r][c]  (fp32 -> fp32 | bf16), 32x32 tiles through LDS
// ---------------------------------------------------------------------------------------------
template <typename OutT>
__global__ __launch_bounds__(256) void pack_transpose_kernel(const float* __restrict__ src, long long src_ld, OutT* __restrict__ dst,
                                                             long long dst_ld, int rows, int cols) {
  __shared__ float tile[32][33];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < rows && c < cols) ? src[(long long)r * src_ld + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + tx;
    if (c < cols && r < rows) {
      const float v = tile[tx][i];
      if constexpr (std::is_same<OutT, float>::value) dst[(long long)c * dst_ld + r] = v;
      else ((uint16_t*)dst)[(long long)c * dst_ld + r] = HalfOps<OutT>::from_f32(v);
    }
  }
}

__global__ void cvt_bf16_kernel(const float* __restrict__ in, uint16_t* __restrict__ out, int n, int hw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (2 * i + 1 >= n + 1) return;
  const float a = in[2 * i], b = (2 * i + 1 < n) ? in[2 * i + 1] : 0.f;
  unsigned int r = hw ? ctpn_cvt_pk_bf16(a, b) : ((unsigned int)f2bf(a) | ((unsigned int)f2bf(b) << 16));
  out[2 * i] = (uint16_t)r;
  if (2 * i + 1 < n) out[2 * i + 1] = (uint16_t)(r >> 16);
}
int launch_cvt_bf16(const float* in, uint16_t* out, int n, int hw, hipStream_t s) {
  hipLaunchKernelGGL(cvt_bf16_kernel, dim3((n / 2 + 256) / 256), dim3(256), 0, s, in, out, n, hw);
  return launch_status("cvt");
}

int launch_pack_transpose(const float* src, long long src_ld, void* dst, long long dst_ld, DType dst_t, int rows,
                          int cols, hipStream_t s) {
  dim3 grid((cols + 31) / 32, (rows + 31) / 32);
  if (dst_t == DType::F32)
    hipLaunchKernelGGL(pack_transpose_kernel<float>, grid, dim3(256), 0, s, src, src_ld, (float*)dst, dst_ld, rows, cols);
  else if (dst_t == DType::F16)
    hipLaunchKernelGGL(pack_transpose_kernel<h_f16>, grid, dim3(256), 0, s, src, src_ld, (h_f16*)dst, dst_ld, rows, cols);
  else if (dst_t == DType::BF16)
    hipLaunchKernelGGL(pack_transpose_kernel<h_bf16>, grid, dim3(256), 0, s, src, src_ld, (h_bf16*)dst, dst_ld, rows, cols);
  else
    return fail(CTPN_ERR_ARG, "pack_transpose: split precision packs through launch_pack_transpose_split");
  return launch_status("pack");
}

// split precision: src row k = tap * ci + c (TF HWIO flattened / [in][out]), column co -> dst[co][tap][hi(ci) | hi(ci) | lo(ci)] bf16:
// the K layout conv3x3's split kernels (and the LSTM projection GEMM over [hi | lo | hi] pixels) multiply against
__global__ __launch_bounds__(256) void pack_split_kernel(const float* __restrict__ src, long long src_ld, uint16_t* __restrict__ dst, int taps, int ci, int cols) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)cols * taps * ci;
  if (idx >= total) return;
  const int c = (int)(idx % ci);
  const int tap = (int)((idx / ci) % taps);
  const int co = (int)(idx / ((long long)ci * taps));
  const float v = src[((long long)tap * ci + c) * src_ld + co];
  const uint16_t hi = ctpn_f32_to_bf16(v);
  const uint16_t lo = ctpn_f32_to_bf16(v - ctpn_bf16_to_f32(hi));
  uint16_t* row = dst + ((long long)co * taps + tap) * 3 * ci;
  row[c] = hi; row[ci + c] = hi; row[2 * ci + c] = lo;
}
int launch_pack_transpose_split(const float* src, long long src_ld, void* dst, int taps, int ci, int cols, hipStream_t s) {
  const long long total = (long long)cols * taps * ci;
  hipLaunchKernelGGL(pack_split_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, src_ld, (uint16_t*)dst, taps, ci, cols);
  return launch_status("pack (split)");
}

}  // namespace ctpn
