// The backward pass through one 3x3 conv + bias + ReLU, and through the 2x2 max-pool (include/ctpn_hip.h, "the conv stack: backward"; the
// per-thread text and the block plan: conv_grad_dev.h). Plain dense fp32: NHWC activations, TF's HWIO weights, SAME padding by predicate.
//   cg_mask_kernel        dZ = d_y (y > 0), written ONCE to a block of the call; the two gradient kernels and the bias sums read it. (The other
//                         form, the mask applied at each of the three readers' loads, reads y three times and was not measured against this one.)
//   cg_dx_kernel          the data gradient: an implicit GEMM with M = pixels, N = ci, K = 9 co. One wave per 64 pixels x 32 input channels, 8
//                         accumulator tiles of v_mfma_f32_16x16x4_f32. K is contiguous in both operands as stored (co is innermost in HWIO and
//                         in NHWC), so each lane loads 16 bytes of either and feeds four MFMAs. Every element is ONE fma chain: taps in
//                         (ky, kx) order, output channels in a fixed order inside a tap
//   cg_dw_partial_kernel  the weight gradient over one block of pixels (cg_plan): a workgroup of 4 waves owns 16 input channels x 64 output
//                         channels x 9 taps; wave v owns output channels [16 v, 16 v + 16) and nine accumulator tiles, one per tap. The k
//                         dimension of the MFMA is the pixel index. A strip of x -- 128 consecutive pixels with the rows above and below and one
//                         pixel on either side, 3 x 130 x 16 floats -- is staged through LDS once per 128 pixels and read shifted nine times.
//                         Every element is an fma chain over the block's pixels in ascending order, from 0
//   cg_colsum_kernel      the bias gradient over the same blocks in tb_colsum_block's order: eight interleaved sums, one per wave, added pairwise
//   cg_reduce_kernel      the ordered pass over the blocks' partial sums (tb_tn_reduce)
//   cg_pool_kernel        the max-pool backward: every element of d_full is written (cg_pool_backward)
// No atomics: the order of every sum depends on the shape alone.
#include "common.h"
#include "conv_grad_dev.h"

namespace ctpn {

typedef __attribute__((ext_vector_type(4))) float f32x4;

__global__ __launch_bounds__(256) void cg_mask_kernel(const float* __restrict__ d_y, const float* __restrict__ y, float* __restrict__ dz, size_t quads) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  const f32x4 g = ((const f32x4*)d_y)[q], v = ((const f32x4*)y)[q];
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = cg_relu_mask(g[e], v[e]);
  ((f32x4*)dz)[q] = o;
}

// ---------------------------------------------------------------------------------------------
// d_x [M][ci] from dZ [M][co] and w [9][ci][co]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cg_dx_kernel(const float* __restrict__ dz, const float* __restrict__ wt, int h, int w, int ci, int co, long long M,
                                                   float* __restrict__ dx) {
  const int lane = threadIdx.x, r = lane & 15, q4 = lane >> 4;
  const long long p0 = (long long)blockIdx.x * 64;
  const int c0 = blockIdx.y * 32;
  // this lane's four pixels: the B operand's column and the column of the result
  long long pc[4];
  int pi[4], pj[4];
  bool p_ok[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const long long p = p0 + 16 * g + r;
    p_ok[g] = p < M;
    pc[g] = p_ok[g] ? p : M - 1;
    cg_pixel_coords(pc[g], h, w, pi[g], pj[g]);
  }
  f32x4 acc[2][4];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[n][g] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) {
      // d_x(i, j) takes w[ky][kx] times dZ(i - ky + 1, j - kx + 1)
      const int dy = 1 - ky, dxx = 1 - kx;
      const float* zrow[4];
      bool ok[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        ok[g] = p_ok[g] && cg_tap_ok(h, w, pi[g], pj[g], dy, dxx);
        zrow[g] = dz + (size_t)(ok[g] ? pc[g] + cg_tap_offset(w, dy, dxx) : pc[g]) * co + 4 * q4;
      }
      const float* wrow[2];
#pragma unroll
      for (int n = 0; n < 2; ++n) wrow[n] = wt + ((size_t)(ky * 3 + kx) * ci + c0 + 16 * n + r) * co + 4 * q4;
      for (int o = 0; o < co; o += 16) {
        f32x4 zv[4], wv[2];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 v = *(const f32x4*)(zrow[g] + o);
          zv[g] = ok[g] ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int n = 0; n < 2; ++n) wv[n] = *(const f32x4*)(wrow[n] + o);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[n][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[n][e], zv[g][e], acc[n][g], 0, 0, 0);
      }
    }
  // C/D: column (lane & 15) = the pixel, rows 4 (lane >> 4) + reg = four consecutive input channels
#pragma unroll
  for (int g = 0; g < 4; ++g)
    if (p_ok[g])
#pragma unroll
      for (int n = 0; n < 2; ++n) *(f32x4*)(dx + (size_t)pc[g] * ci + c0 + 16 * n + 4 * q4) = acc[n][g];
}

// ---------------------------------------------------------------------------------------------
// d_w partials [P][9][ci][co] from x [M][ci] and dZ [M][co]
// ---------------------------------------------------------------------------------------------
constexpr int CG_CHUNK = 128;             // pixels staged per round
constexpr int CG_BAND = CG_CHUNK + 2;     // with one pixel on either side

__global__ __launch_bounds__(256) void cg_dw_partial_kernel(const float* __restrict__ x, const float* __restrict__ dz, int h, int w, int ci, int co, long long M,
                                                            long long block, float* __restrict__ parts) {
  __shared__ __attribute__((aligned(16))) float xs[3][CG_BAND][CG_C_TILE];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_o = co / CG_O_TILE;
  const int c0 = (blockIdx.x / tiles_o) * CG_C_TILE, o0 = (blockIdx.x % tiles_o) * CG_O_TILE + 16 * wave;
  const long long m_lo = (long long)blockIdx.y * block, m_hi = m_lo + block < M ? m_lo + block : M;
  const bool vec = (ci % CG_C_TILE) == 0;      // otherwise ci = 3: one tile, channels 3..15 are zero
  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long pb = m_lo; pb < m_hi; pb += CG_CHUNK) {
    __syncthreads();      // every wave has read the strip before
    // band b holds the flat pixels pb + (b - 1) w - 1 .. + CG_BAND; pixels outside the batch are zero (no tap that is inside its image reads them)
    for (int e = tid; e < 3 * CG_BAND * 4; e += 256) {
      const int band = e / (CG_BAND * 4), rem = e - band * (CG_BAND * 4), pos = rem >> 2, c4 = rem & 3;
      const long long src = pb + (long long)(band - 1) * w + pos - 1;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (src >= 0 && src < M) {
        if (vec) v = *(const f32x4*)(x + (size_t)src * ci + c0 + 4 * c4);
        else
#pragma unroll
          for (int k = 0; k < 4; ++k) { const int c = 4 * c4 + k; if (c < ci) v[k] = x[(size_t)src * ci + c]; }
      }
      *(f32x4*)(&xs[band][pos][4 * c4]) = v;
    }
    __syncthreads();
    int i, j;
    cg_pixel_coords(pb + q4 < M ? pb + q4 : M - 1, h, w, i, j);
    const int steps = (int)((m_hi - pb < CG_CHUNK ? m_hi - pb : CG_CHUNK) + 3) / 4;
    for (int ks = 0; ks < steps; ++ks) {
      const int pos = 4 * ks + q4;      // this lane's pixel: k = lane >> 4 of both operands
      const long long p = pb + pos;
      const bool p_ok = p < m_hi;
      const float zb = dz[(size_t)(p_ok ? p : m_hi - 1) * co + o0 + r];
      const float b = p_ok ? zb : 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float av = xs[ky][pos + kx][r];
          const float a = (p_ok && cg_tap_ok(h, w, i, j, ky - 1, kx - 1)) ? av : 0.f;
          acc[ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[ky * 3 + kx], 0, 0, 0);
        }
      // four pixels on, in (image, row, column) order
      j += 4;
      while (j >= w) { j -= w; if (++i >= h) i = 0; }
    }
  }
  // C/D: column (lane & 15) = the output channel, rows 4 (lane >> 4) + reg = input channels
  float* out = parts + (size_t)blockIdx.y * 9 * ci * co;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c0 + 4 * q4 + e;
      if (c < ci) out[((size_t)t * ci + c) * co + o0 + r] = acc[t][e];
    }
}

// parts [P][co]: column sums of dZ over each block. Wave k of the workgroup takes the pixels with (m & 7) == k, ascending: tb_colsum_block's
// eight running sums, then its pairwise order
__global__ __launch_bounds__(512) void cg_colsum_kernel(const float* __restrict__ dz, int co, long long M, long long block, float* __restrict__ parts) {
  __shared__ float s[8][64];
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
  const long long m_lo = (long long)blockIdx.y * block, m_hi = m_lo + block < M ? m_lo + block : M;
  const int o = blockIdx.x * 64 + lane;
  const float* col = dz + (size_t)m_lo * co + o;
  const long long cells = m_hi - m_lo;
  float acc = 0.f;
  long long m = k;
  for (; m + 24 < cells; m += 32) {      // four loads in flight, added in ascending order
    const float v0 = col[(size_t)m * co], v1 = col[(size_t)(m + 8) * co], v2 = col[(size_t)(m + 16) * co], v3 = col[(size_t)(m + 24) * co];
    acc = acc + v0; acc = acc + v1; acc = acc + v2; acc = acc + v3;
  }
  for (; m < cells; m += 8) acc = acc + col[(size_t)m * co];
  s[k][lane] = acc;
  __syncthreads();
  if (k == 0) parts[(size_t)blockIdx.y * co + o] = ((s[0][lane] + s[1][lane]) + (s[2][lane] + s[3][lane])) + ((s[4][lane] + s[5][lane]) + (s[6][lane] + s[7][lane]));
}

// out[e] = the ordered sum of the P partials of element e
__global__ __launch_bounds__(256) void cg_reduce_kernel(const float* __restrict__ parts, int P, size_t total, float* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < total) out[e] = tb_tn_reduce(parts + e, P, total);
}

__global__ __launch_bounds__(256) void cg_pool_kernel(const float* __restrict__ y, const float* __restrict__ d_pool, int h, int w, int c, size_t total,
                                                      float* __restrict__ d_full) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const size_t pix = e / c;
  const int ch = (int)(e - pix * c);
  const size_t img = pix / ((size_t)h * w);
  const size_t in_img = pix - img * (size_t)h * w;
  const int i = (int)(in_img / w), j = (int)(in_img - (size_t)i * w);
  d_full[e] = cg_pool_backward(y + img * (size_t)h * w * c + ch, d_pool + img * (size_t)(h / 2) * (w / 2) * c + ch, h, w, (size_t)c, i, j);
}

int launch_conv_grad_mask(const float* d_y, const float* y, float* dz, long long M, int co, hipStream_t s) {
  const size_t quads = (size_t)M * co / 4;
  hipLaunchKernelGGL(cg_mask_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, d_y, y, dz, quads);
  return launch_status("conv_grad_mask");
}

int launch_conv_grad_dx(const float* dz, const float* wt, int h, int w, int ci, int co, long long M, float* dx, hipStream_t s) {
  if (ci % 32 || co % 16) return fail(CTPN_ERR_ARG, "conv_grad_dx: ci is a multiple of 32, co of 16");
  hipLaunchKernelGGL(cg_dx_kernel, dim3((unsigned)((M + 63) / 64), ci / 32), dim3(64), 0, s, dz, wt, h, w, ci, co, M, dx);
  return launch_status("conv_grad_dx");
}

int launch_conv_grad_dw(const float* x, const float* dz, int h, int w, int ci, int co, long long M, float* parts, float* bparts, float* d_w, float* d_b, hipStream_t s) {
  if (co % CG_O_TILE || (ci != 3 && ci % CG_C_TILE)) return fail(CTPN_ERR_ARG, "conv_grad_dw: co is a multiple of 64, ci is 3 or a multiple of 16");
  long long block;
  int P;
  cg_plan(M, ci, co, block, P);
  const int tiles = ((ci + CG_C_TILE - 1) / CG_C_TILE) * (co / CG_O_TILE);
  hipLaunchKernelGGL(cg_dw_partial_kernel, dim3(tiles, P), dim3(256), 0, s, x, dz, h, w, ci, co, M, block, parts);
  if (const int rc = launch_status("conv_grad_dw")) return rc;
  const size_t total = (size_t)9 * ci * co;
  hipLaunchKernelGGL(cg_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, parts, P, total, d_w);
  if (const int rc = launch_status("conv_grad_dw_reduce")) return rc;
  hipLaunchKernelGGL(cg_colsum_kernel, dim3(co / 64, P), dim3(512), 0, s, dz, co, M, block, bparts);
  if (const int rc = launch_status("conv_grad_colsum")) return rc;
  hipLaunchKernelGGL(cg_reduce_kernel, dim3((co + 255) / 256), dim3(256), 0, s, bparts, P, (size_t)co, d_b);
  return launch_status("conv_grad_colsum_reduce");
}

int launch_pool_grad(const float* y, const float* d_pool, int n, int h, int w, int c, float* d_full, hipStream_t s) {
  const size_t total = (size_t)n * h * w * c;
  hipLaunchKernelGGL(cg_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, y, d_pool, h, w, c, total, d_full);
  return launch_status("pool_grad");
}

}  // namespace ctpn
