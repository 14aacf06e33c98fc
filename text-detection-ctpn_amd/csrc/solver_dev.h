// The solver step over flat fp32 vectors (include/ctpn_hip.h, "the solver step"): the plan of the reductions, the step's parameters and the
// per-element text of solver.hip's two kernels as host + device functions. tests/solver_host.cpp compiles this same text with g++ under
// ASan + UBSan (-ffp-contract=off, as the Makefile gives solver.hip) and walks whole vectors the way the kernels do.
//   sv_plan          count -> block_floats (a multiple of 1024), blocks (at most 2048): a function of count alone
//   sv_params        hyper8, t and the global norm -> the fp32 constants of the update (Adam's lr_t in double, as ApplyAdam's caller forms it)
//   sv_seg_find      the segment of an element, a binary search: once per thread, then the thread walks forward (sv_seg_walk)
//   sv_ge            g + d w, the gradient of total_loss; d = 0 skips the product, so that ge == g in bits
//   sv_sum_terms     the element's terms of the two sums, in double
//   sv_lane_sums     one lane of a block: quads q = lane, lane + 256, ... of the block, elements ascending, one running sum each
//   sv_tree          the 256 lane sums of a block, added pairwise: stride 128, 64, .. 1
//   sv_update        one element of the update: clip, then Momentum / ApplyAdam / ApplyRMSProp
// fp32 throughout, every operation rounded (no contraction), / and sqrtf correctly rounded. Nothing here includes a HIP header.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SV_HD __host__ __device__ inline
#else
#define SV_HD inline
#endif

namespace ctpn {

constexpr int SV_MOMENTUM = 0, SV_ADAM = 1, SV_RMS = 2;
constexpr int SV_LANES = 256;                       // threads of a workgroup; a lane takes every 256th quad of its block
constexpr long long SV_BLOCK_UNIT = 4 * SV_LANES;   // a block is a multiple of this many floats: every lane gets whole quads
constexpr int SV_MAX_BLOCKS = 2048;                 // eight workgroups per CU of a 256-CU device; a constant, not the device's CU count
constexpr int SV_MAX_SEGMENTS = 64;
// hyper8: [0] lr  [1] momentum | beta1 | decay (rho)  [2] - | beta2 | RMS momentum  [3] - | epsilon | epsilon  [4] clip norm
//         [5] the value s1 starts at (RMS: ms = 1)  [6] the value s2 starts at  [7] reserved, zero
constexpr int SV_LR = 0, SV_A = 1, SV_B = 2, SV_EPS = 3, SV_CLIP = 4, SV_S1_INIT = 5, SV_S2_INIT = 6;

struct SvSegments {
  int n;
  long long end[SV_MAX_SEGMENTS];      // ascending; end[n - 1] = count
  float decay[SV_MAX_SEGMENTS];
};

struct SvParams {
  int solver;
  int clip_on;       // norm > clip
  float scale;       // (float)(clip / norm)
  float lr;          // Momentum, RMS
  float a;           // momentum (Momentum), RMS momentum
  float one_m_a;     // 1.0f - beta1 | 1.0f - rho
  float one_m_b;     // 1.0f - beta2
  float eps;
  float lr_t;        // Adam: (float)(lr sqrt(1 - beta2^t) / (1 - beta1^t))
};

SV_HD void sv_plan(long long count, long long& block_floats, int& blocks) {
  long long b = (count + SV_MAX_BLOCKS - 1) / SV_MAX_BLOCKS;
  b = (b + SV_BLOCK_UNIT - 1) / SV_BLOCK_UNIT * SV_BLOCK_UNIT;
  if (b < SV_BLOCK_UNIT) b = SV_BLOCK_UNIT;
  block_floats = b;
  blocks = (int)((count + b - 1) / b);
}

inline void sv_defaults(int solver, double* h) {
  for (int i = 0; i < 8; ++i) h[i] = 0.0;
  h[SV_LR] = 0.001;            // TRAIN.LEARNING_RATE of lib/fast_rcnn/config.py
  h[SV_CLIP] = 10.0;           // lib/fast_rcnn/train.py:108
  if (solver == SV_MOMENTUM) h[SV_A] = 0.9;
  else if (solver == SV_ADAM) { h[SV_A] = 0.9; h[SV_B] = 0.999; h[SV_EPS] = 1e-8; }
  else { h[SV_A] = 0.9; h[SV_B] = 0.0; h[SV_EPS] = 1e-10; h[SV_S1_INIT] = 1.0; }      // tf.train.RMSPropOptimizer: ms starts at ones
}

inline SvParams sv_params(int solver, const double* h, long long t, double norm) {
  SvParams p{};
  p.solver = solver;
  p.clip_on = norm > h[SV_CLIP] ? 1 : 0;
  p.scale = p.clip_on ? (float)(h[SV_CLIP] / norm) : 1.0f;
  p.lr = (float)h[SV_LR];
  p.eps = (float)h[SV_EPS];
  if (solver == SV_MOMENTUM) p.a = (float)h[SV_A];
  else if (solver == SV_ADAM) {
    p.one_m_a = 1.0f - (float)h[SV_A];
    p.one_m_b = 1.0f - (float)h[SV_B];
    p.lr_t = (float)(h[SV_LR] * sqrt(1.0 - pow(h[SV_B], (double)t)) / (1.0 - pow(h[SV_A], (double)t)));
  } else {
    p.one_m_a = 1.0f - (float)h[SV_A];
    p.a = (float)h[SV_B];
  }
  return p;
}

// the first segment whose end lies beyond element e (e < count)
SV_HD int sv_seg_find(const SvSegments& s, long long e) {
  int lo = 0, hi = s.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e < s.end[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// ... and from a segment at or before e's: elements are visited in ascending order, so this is a step or two per boundary crossed
SV_HD int sv_seg_walk(const SvSegments& s, int seg, long long e) {
  while (seg < s.n - 1 && e >= s.end[seg]) ++seg;
  return seg;
}

SV_HD float sv_ge(float g, float w, float d) { return d == 0.f ? g : g + d * w; }

SV_HD void sv_sum_terms(float g, float w, float d, double& sq, double& reg) {
  const double ge = (double)sv_ge(g, w, d);
  sq = sq + ge * ge;
  if (d != 0.f) reg = reg + 0.5 * ((double)d * ((double)w * (double)w));
}

// lane `lane` of the block [lo, hi): its quads in ascending order. The kernel reads a quad as one 16-byte access where both arrays allow it
SV_HD void sv_lane_sums(const float* w, const float* g, long long lo, long long hi, int lane, const SvSegments& segs, double& sq, double& reg) {
  sq = 0.0; reg = 0.0;
  long long e0 = lo + 4LL * lane;
  if (e0 >= hi) return;
  int seg = sv_seg_find(segs, e0);
  for (; e0 < hi; e0 += 4LL * SV_LANES) {
    const long long e1 = e0 + 4 < hi ? e0 + 4 : hi;
    for (long long e = e0; e < e1; ++e) {
      seg = sv_seg_walk(segs, seg, e);
      sv_sum_terms(g[e], w[e], segs.decay[seg], sq, reg);
    }
  }
}

// v[0 .. 255] -> v[0]: the kernel's LDS tree, one stride per barrier
SV_HD void sv_tree_step(double* v, int stride, int lane) { if (lane < stride) v[lane] = v[lane] + v[lane + stride]; }

SV_HD void sv_update(const SvParams& p, float d, float g, float& w, float& s1, float& s2) {
  const float ge = sv_ge(g, w, d);
  const float gc = p.clip_on ? ge * p.scale : ge;
  if (p.solver == SV_MOMENTUM) {
    s1 = p.a * s1 + gc;
    w = w - p.lr * s1;
  } else if (p.solver == SV_ADAM) {
    s1 = s1 + (gc - s1) * p.one_m_a;
    s2 = s2 + (gc * gc - s2) * p.one_m_b;
    w = w - (s1 * p.lr_t) / (sqrtf(s2) + p.eps);
  } else {
    s1 = s1 + (gc * gc - s1) * p.one_m_a;
    s2 = s2 * p.a + (gc * p.lr) / sqrtf(s1 + p.eps);
    w = w - s2;
  }
}

}  // namespace ctpn
