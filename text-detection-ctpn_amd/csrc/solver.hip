// The solver step's two kernels (include/ctpn_hip.h, "the solver step"; the plan, the parameters and the per-element text: solver_dev.h).
// Both are streaming kernels over `blocks` workgroups of 256 threads (sv_plan: up to 2048 workgroups, eight per CU of a 256-CU device); lane l
// of a block takes the block's quads l, l + 256, ...: a wave reads 1 KiB of consecutive addresses per array and round.
//   sv_sums_kernel     pass 1, reads w and g: per lane the two running sums in double over its elements in ascending order, then the block's
//                      LDS tree (sv_tree_step), one pair of doubles per block. No atomics: the host adds the partials left to right.
//   sv_update_kernel   pass 2, reads w, g, s1 (and s2), writes w, s1 (and s2): sv_update per element
// VEC: every quad is one 16-byte access per array; it needs every array 16-byte aligned (a block starts at a multiple of 1024 floats, so the
// quads are then aligned too). Otherwise -- a base pointer at some other 4-byte alignment -- the same threads take the same elements with
// 4-byte accesses: which lane adds which element, and so the order of the sums, never depends on the address. The quad that count cuts short
// is read element by element in both forms. A thread finds its first element's segment by binary search once and walks forward from there.
#include "common.h"
#include "solver_dev.h"

namespace ctpn {

typedef __attribute__((ext_vector_type(4))) float sv_f32x4;

template <bool VEC>
__device__ __forceinline__ void sv_load4(const float* __restrict__ p, long long e0, int cnt, float v[4]) {
  if (VEC && cnt == 4) {
    const sv_f32x4 q = *(const sv_f32x4*)(p + e0);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < cnt ? p[e0 + k] : 0.f;
  }
}

template <bool VEC>
__device__ __forceinline__ void sv_store4(float* __restrict__ p, long long e0, int cnt, const float v[4]) {
  if (VEC && cnt == 4) *(sv_f32x4*)(p + e0) = sv_f32x4{v[0], v[1], v[2], v[3]};
  else {
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < cnt) p[e0 + k] = v[k];
  }
}

template <bool VEC>
__global__ __launch_bounds__(SV_LANES) void sv_sums_kernel(const float* __restrict__ w, const float* __restrict__ g, long long count, long long block,
                                                           SvSegments segs, double* __restrict__ partials) {
  __shared__ double s_sq[SV_LANES], s_reg[SV_LANES];
  const int lane = threadIdx.x;
  const long long lo = (long long)blockIdx.x * block, hi = lo + block < count ? lo + block : count;
  double sq = 0.0, reg = 0.0;
  long long e0 = lo + 4LL * lane;
  if (e0 < hi) {
    int seg = sv_seg_find(segs, e0);
    for (; e0 < hi; e0 += 4LL * SV_LANES) {
      const int cnt = hi - e0 < 4 ? (int)(hi - e0) : 4;
      float wv[4], gv[4];
      sv_load4<VEC>(w, e0, cnt, wv);
      sv_load4<VEC>(g, e0, cnt, gv);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) {
          seg = sv_seg_walk(segs, seg, e0 + k);
          sv_sum_terms(gv[k], wv[k], segs.decay[seg], sq, reg);
        }
    }
  }
  s_sq[lane] = sq;
  s_reg[lane] = reg;
  for (int stride = SV_LANES / 2; stride >= 1; stride >>= 1) {
    __syncthreads();
    sv_tree_step(s_sq, stride, lane);
    sv_tree_step(s_reg, stride, lane);
  }
  if (lane == 0) { partials[2 * (size_t)blockIdx.x] = s_sq[0]; partials[2 * (size_t)blockIdx.x + 1] = s_reg[0]; }
}

template <bool VEC, bool HAS_S2>
__global__ __launch_bounds__(SV_LANES) void sv_update_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ s1, float* __restrict__ s2,
                                                             long long count, long long block, SvSegments segs, SvParams p) {
  const int lane = threadIdx.x;
  const long long lo = (long long)blockIdx.x * block, hi = lo + block < count ? lo + block : count;
  long long e0 = lo + 4LL * lane;
  if (e0 >= hi) return;
  int seg = sv_seg_find(segs, e0);
  for (; e0 < hi; e0 += 4LL * SV_LANES) {
    const int cnt = hi - e0 < 4 ? (int)(hi - e0) : 4;
    float wv[4], gv[4], av[4], bv[4] = {0.f, 0.f, 0.f, 0.f};
    sv_load4<VEC>(w, e0, cnt, wv);
    sv_load4<VEC>(g, e0, cnt, gv);
    sv_load4<VEC>(s1, e0, cnt, av);
    if (HAS_S2) sv_load4<VEC>(s2, e0, cnt, bv);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) {
        seg = sv_seg_walk(segs, seg, e0 + k);
        sv_update(p, segs.decay[seg], gv[k], wv[k], av[k], bv[k]);
      }
    sv_store4<VEC>(w, e0, cnt, wv);
    sv_store4<VEC>(s1, e0, cnt, av);
    if (HAS_S2) sv_store4<VEC>(s2, e0, cnt, bv);
  }
}

static bool sv_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// partials: 2 x blocks doubles (sum of ge^2, sum of decay w^2 / 2 per block)
int launch_solver_sums(const float* w, const float* g, long long count, const SvSegments& segs, double* partials, hipStream_t s) {
  long long block;
  int blocks;
  sv_plan(count, block, blocks);
  if (sv_aligned16(w) && sv_aligned16(g)) hipLaunchKernelGGL(sv_sums_kernel<true>, dim3(blocks), dim3(SV_LANES), 0, s, w, g, count, block, segs, partials);
  else hipLaunchKernelGGL(sv_sums_kernel<false>, dim3(blocks), dim3(SV_LANES), 0, s, w, g, count, block, segs, partials);
  return launch_status("solver_sums");
}

int launch_solver_update(float* w, const float* g, float* s1, float* s2, long long count, const SvSegments& segs, const SvParams& p, hipStream_t s) {
  long long block;
  int blocks;
  sv_plan(count, block, blocks);
  const bool has2 = p.solver != SV_MOMENTUM;
  const bool vec = sv_aligned16(w) && sv_aligned16(g) && sv_aligned16(s1) && (!has2 || sv_aligned16(s2));
  const dim3 grid(blocks), wg(SV_LANES);
  if (has2) {
    if (vec) hipLaunchKernelGGL((sv_update_kernel<true, true>), grid, wg, 0, s, w, g, s1, s2, count, block, segs, p);
    else hipLaunchKernelGGL((sv_update_kernel<false, true>), grid, wg, 0, s, w, g, s1, s2, count, block, segs, p);
  } else {
    if (vec) hipLaunchKernelGGL((sv_update_kernel<true, false>), grid, wg, 0, s, w, g, s1, s2, count, block, segs, p);
    else hipLaunchKernelGGL((sv_update_kernel<false, false>), grid, wg, 0, s, w, g, s1, s2, count, block, segs, p);
  }
  return launch_status("solver_update");
}

}  // namespace ctpn
