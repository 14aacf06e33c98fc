// The label side of training on the device (ctpn_bbox_overlaps, ctpn_anchor_targets, ctpn_rpn_loss: api_targets.hip): the dense anchor x
// ground-truth overlap, the anchor target layer, the RPN loss and its gradient at the heads. The per-thread text is targets_dev.h's, pinned on
// the CPU from that very text (tests/test_anchor_targets.py). This unit is compiled with -ffp-contract=off: the overlap, bbox_transform and
// the sums are the reference's double arithmetic, operation by operation.
//   tg_scan_kernel    a thread per anchor, the image's boxes staged through LDS TG_CHUNK at a time (all lanes read one box: a broadcast, no
//                     bank conflict): running first maximum and argmax in registers; column maxima by 64-bit atomicMax on the overlap's bit
//                     pattern (overlaps are >= 0, so the pattern orders as an integer; a maximum does not depend on arrival order), issued for
//                     positive overlaps only -- a strip meets a few hundred anchors, the table starts at 0
//   tg_mark_kernel    the same pairs from the same inlined body, against the finished column maxima: the equality rule, the hard boxes'
//                     maxima, a 32-bit atomicMin per (hard box, maximal anchor) for "the first maximal anchor"; then the label rules,
//                     bbox_transform, and everything an anchor's record holds but the weights
//   tg_hard_kernel    a thread per ground-truth box: a hard box's first maximal anchor is disabled
//   tg_sample_kernel  a workgroup per image: the counts, the radix select of the threshold key (eight passes of 256-bin LDS histograms; integer
//                     atomics), the labels after sampling and the two weight arrays
//   tg_loss_kernel    a workgroup per image: every thread sums its anchors i = t, t + TG_WG, ... in ascending order, a fixed tree joins the
//                     TG_WG partial sums. The order depends on hf * wf alone: no float atomic, image i of a batch gives the bytes of image i
//                     alone. The gradient is a second loop of the same workgroup, which by then knows the two counts
//   tg_overlaps_kernel  ctpn_bbox_overlaps: TG_ROWS boxes per workgroup, query boxes staged TG_CHUNK at a time with their areas, a thread per
//                     query box, so a wave writes 512 contiguous bytes of a row
#include "common.h"
#include "targets_dev.h"

namespace ctpn {
namespace {

__device__ inline void tg_stage(const float* __restrict__ gt, const unsigned long long* __restrict__ colmax, const int* __restrict__ hard, int g0, int cnt,
                                double* lds) {
  for (int j = threadIdx.x; j < cnt; j += TG_THREADS)
    tg_stage_box(gt + (size_t)(g0 + j) * 5, colmax ? __longlong_as_double((long long)colmax[g0 + j]) : 0.0, hard ? hard[g0 + j] == 1 : 0, lds + j * TG_BOX);
}

__global__ __launch_bounds__(TG_THREADS) void tg_scan_kernel(int A, int wf, const float* __restrict__ im_info, const float* __restrict__ gt,
                                                             const int* __restrict__ offs, unsigned long long* __restrict__ colmax,
                                                             double* __restrict__ best_out, int* __restrict__ arg_out) {
  __shared__ double lds[TG_CHUNK * TG_BOX];
  const int img = blockIdx.y;
  const long long idx = (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  const int g_lo = offs[img], G = offs[img + 1] - g_lo;
  double ax1 = 0, ay1 = 0, ax2 = 0, ay2 = 0;
  bool inside = false;
  if (idx < A) {
    tg_anchor(wf, idx, ax1, ay1, ax2, ay2);
    inside = tg_inside(ax1, ay1, ax2, ay2, im_info[img * 3], im_info[img * 3 + 1]);
  }
  const double aarea = tg_area(ax1, ay1, ax2, ay2);
  double best = -1.0;
  int arg = -1;
  for (int c0 = 0; c0 < G; c0 += TG_CHUNK) {
    const int cnt = min(TG_CHUNK, G - c0);
    __syncthreads();
    tg_stage(gt, nullptr, nullptr, g_lo + c0, cnt, lds);
    __syncthreads();
    if (inside)
      tg_scan_chunk(ax1, ay1, ax2, ay2, aarea, lds, cnt, c0, best, arg,
                    [&](int g, double ov) { atomicMax(colmax + g_lo + g, (unsigned long long)__double_as_longlong(ov)); });
  }
  if (idx < A) {
    const bool have = inside && G > 0;
    best_out[(size_t)img * A + idx] = have ? best : 0.0;
    arg_out[(size_t)img * A + idx] = have ? arg : -1;
  }
}

__global__ __launch_bounds__(TG_THREADS) void tg_mark_kernel(int A, int wf, const float* __restrict__ im_info, const float* __restrict__ gt,
                                                             const int* __restrict__ offs, const int* __restrict__ hard, const float* __restrict__ dc,
                                                             const int* __restrict__ dc_offs, TgCfg cfg, const unsigned long long* __restrict__ colmax,
                                                             int* __restrict__ hardfirst, const double* __restrict__ best_in, const int* __restrict__ arg_in,
                                                             uint8_t* __restrict__ flags, float* __restrict__ labels, float* __restrict__ targets) {
  __shared__ double lds[TG_CHUNK * TG_BOX];
  const int img = blockIdx.y;
  const long long idx = (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  const int g_lo = offs[img], G = offs[img + 1] - g_lo;
  double ax1 = 0, ay1 = 0, ax2 = 0, ay2 = 0;
  bool inside = false;
  if (idx < A) {
    tg_anchor(wf, idx, ax1, ay1, ax2, ay2);
    inside = tg_inside(ax1, ay1, ax2, ay2, im_info[img * 3], im_info[img * 3 + 1]);
  }
  const double aarea = tg_area(ax1, ay1, ax2, ay2);
  bool gtmax = false;
  double hardmax = -1.0;
  for (int c0 = 0; c0 < G; c0 += TG_CHUNK) {
    const int cnt = min(TG_CHUNK, G - c0);
    __syncthreads();
    tg_stage(gt, colmax, hard, g_lo + c0, cnt, lds);
    __syncthreads();
    if (inside)
      tg_mark_chunk(ax1, ay1, ax2, ay2, aarea, lds, cnt, c0, gtmax, hardmax, [&](int g) { atomicMin(hardfirst + g_lo + g, (int)idx); });
  }
  if (idx >= A) return;
  const size_t o = (size_t)img * A + idx;
  float t4[4] = {0.f, 0.f, 0.f, 0.f};
  float lab = -1.f;
  bool disabled = false;
  if (inside) {
    const int d_lo = dc ? dc_offs[img] : 0, D = dc ? dc_offs[img + 1] - d_lo : 0;
    const double dcsum = D > 0 ? tg_dontcare_sum(ax1, ay1, ax2, ay2, aarea, dc + (size_t)d_lo * 4, D) : 0.0;
    lab = (float)tg_label(cfg, G, best_in[o], gtmax, D > 0, dcsum, hardmax >= 0.0, hardmax, disabled);
    if (G > 0) tg_targets(ax1, ay1, ax2, ay2, gt + (size_t)(g_lo + arg_in[o]) * 5, t4);
  }
  labels[o] = lab;
  flags[o] = disabled ? 1 : 0;
  *reinterpret_cast<float4*>(targets + o * 4) = make_float4(t4[0], t4[1], t4[2], t4[3]);
}

__global__ __launch_bounds__(TG_THREADS) void tg_hard_kernel(int A, const int* __restrict__ offs, const int* __restrict__ hard, const int* __restrict__ hardfirst,
                                                             uint8_t* __restrict__ flags, float* __restrict__ labels) {
  const int img = blockIdx.y;
  const long long g = (long long)offs[img] + (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  if (g >= offs[img + 1] || hard[g] != 1) return;
  const int i = hardfirst[g];
  if (i < 0 || i >= A) return;      // (no inside anchor at all)
  labels[(size_t)img * A + i] = -1.f;
  flags[(size_t)img * A + i] = 1;
}

// the k-th smallest key (1-based) among the image's anchors whose label is cls; at least k such anchors exist. Every thread of the workgroup calls
__device__ uint64_t tg_select(const float* lab, int A, float cls, unsigned k, uint64_t seed, int img, unsigned* hist, uint64_t* s_prefix, unsigned* s_need) {
  if (threadIdx.x == 0) { *s_prefix = 0; *s_need = k; }
  for (int pass = 7; pass >= 0; --pass) {
    for (int b = threadIdx.x; b < 256; b += TG_WG) hist[b] = 0;
    __syncthreads();
    const uint64_t prefix = *s_prefix;
    for (int i = threadIdx.x; i < A; i += TG_WG)
      if (lab[i] == cls) {
        const uint64_t key = tg_key(seed, img, i);
        if (tg_sel_match(key, prefix, pass)) atomicAdd(&hist[tg_sel_bin(key, pass)], 1u);
      }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned need = *s_need;
      const int b = tg_sel_pick(hist, need);
      *s_need = need;
      *s_prefix = prefix | ((uint64_t)b << (8 * pass));
    }
    __syncthreads();
  }
  const uint64_t r = *s_prefix;
  __syncthreads();
  return r;
}

// labels of class cls beyond the `keep` smallest keys -> -1
__device__ void tg_subsample(float* lab, int A, float cls, long long have, long long keep, uint64_t seed, int img, unsigned* hist, uint64_t* s_prefix,
                             unsigned* s_need) {
  if (have <= keep) return;      // (uniform over the workgroup: both are its shared counts)
  if (keep <= 0) {
    for (int i = threadIdx.x; i < A; i += TG_WG) if (lab[i] == cls) lab[i] = -1.f;
    return;
  }
  const uint64_t thr = tg_select(lab, A, cls, (unsigned)keep, seed, img, hist, s_prefix, s_need);
  for (int i = threadIdx.x; i < A; i += TG_WG) if (lab[i] == cls && tg_key(seed, img, i) > thr) lab[i] = -1.f;
}

__global__ __launch_bounds__(TG_WG) void tg_sample_kernel(int A, int wf, const float* __restrict__ im_info, TgCfg cfg, unsigned long long seed,
                                                          const uint8_t* __restrict__ flags, float* __restrict__ labels, float* __restrict__ inside_w,
                                                          float* __restrict__ outside_w, int* __restrict__ stats, float* __restrict__ presample) {
  __shared__ unsigned hist[256];
  __shared__ uint64_t s_prefix;
  __shared__ unsigned s_need;
  __shared__ int cnt[6];
  const int img = blockIdx.x;
  float* lab = labels + (size_t)img * A;
  if (threadIdx.x < 6) cnt[threadIdx.x] = 0;
  __syncthreads();
  int c_in = 0, c_fg = 0, c_bg = 0, c_dis = 0;
  const float im_h = im_info[img * 3], im_w = im_info[img * 3 + 1];
  for (int i = threadIdx.x; i < A; i += TG_WG) {
    double x1, y1, x2, y2;
    tg_anchor(wf, i, x1, y1, x2, y2);
    c_in += tg_inside(x1, y1, x2, y2, im_h, im_w) ? 1 : 0;
    const float l = lab[i];
    c_fg += l == 1.f;
    c_bg += l == 0.f;
    c_dis += flags[(size_t)img * A + i] ? 1 : 0;
    if (presample) presample[(size_t)img * A + i] = l;
  }
  atomicAdd(&cnt[0], c_in); atomicAdd(&cnt[1], c_fg); atomicAdd(&cnt[2], c_bg); atomicAdd(&cnt[5], c_dis);
  __syncthreads();
  const long long fg = cnt[1], bg = cnt[2];
  if (cfg.batch > 0) {
    const long long num_fg = (long long)(cfg.fg_fraction * (double)cfg.batch);
    tg_subsample(lab, A, 1.f, fg, num_fg, seed, img, hist, &s_prefix, &s_need);
    const long long fg_after = fg < num_fg ? fg : num_fg;
    tg_subsample(lab, A, 0.f, bg, cfg.batch - fg_after, seed, img, hist, &s_prefix, &s_need);
  }
  int a_fg = 0, a_bg = 0;
  for (int i = threadIdx.x; i < A; i += TG_WG) {
    const float l = lab[i];
    const bool f = l == 1.f;
    a_fg += f;
    a_bg += l == 0.f;
    const size_t o = ((size_t)img * A + i) * 4;
    *reinterpret_cast<float4*>(inside_w + o) = f ? make_float4(cfg.inside_w[0], cfg.inside_w[1], cfg.inside_w[2], cfg.inside_w[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float w = f ? 1.f : 0.f;
    *reinterpret_cast<float4*>(outside_w + o) = make_float4(w, w, w, w);
  }
  atomicAdd(&cnt[3], a_fg); atomicAdd(&cnt[4], a_bg);
  __syncthreads();
  if (threadIdx.x < 6) stats[img * 6 + threadIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(TG_WG) void tg_loss_kernel(int A, const float* __restrict__ heads, int ld, const float* __restrict__ labels,
                                                        const float* __restrict__ targets, const float* __restrict__ inside_w,
                                                        const float* __restrict__ outside_w, double* __restrict__ losses, int* __restrict__ counts,
                                                        float* __restrict__ d_heads) {
  __shared__ double r_ce[TG_WG], r_box[TG_WG];
  __shared__ int r_kept[TG_WG], r_fg[TG_WG];
  const int img = blockIdx.x, t = threadIdx.x;
  const size_t cells = (size_t)(A / TG_A);
  const float* hrow = heads + (size_t)img * cells * ld;
  const size_t base = (size_t)img * A;
  double ce = 0.0, box = 0.0;
  int kept = 0, fg = 0;
  for (int i = t; i < A; i += TG_WG) {
    const float l = labels[base + i];
    if (l == -1.f) continue;
    const int a = i % TG_A;
    const float* h = hrow + (size_t)(i / TG_A) * ld;
    const int label = l == 1.f ? 1 : 0;
    ce = ce + tg_ce_term(h[40 + 2 * a], h[40 + 2 * a + 1], label);
    const size_t o = (base + i) * 4;
    double b4 = 0.0;
    for (int c = 0; c < 4; ++c) b4 = b4 + tg_box_term(h[4 * a + c], targets[o + c], inside_w[o + c], outside_w[o + c]);
    box = box + b4;
    kept += 1;
    fg += label;
  }
  r_ce[t] = ce; r_box[t] = box; r_kept[t] = kept; r_fg[t] = fg;
  __syncthreads();
  for (int s = TG_WG / 2; s > 0; s >>= 1) {
    if (t < s) { r_ce[t] = r_ce[t] + r_ce[t + s]; r_box[t] = r_box[t] + r_box[t + s]; r_kept[t] += r_kept[t + s]; r_fg[t] += r_fg[t + s]; }
    __syncthreads();
  }
  const int K = r_kept[0], F = r_fg[0];
  if (t == 0) {
    const double l_ce = K > 0 ? r_ce[0] / (double)K : 0.0, l_box = r_box[0] / ((double)F + 1.0);
    losses[img * 3] = l_ce; losses[img * 3 + 1] = l_box; losses[img * 3 + 2] = l_ce + l_box;
    counts[img * 2] = K; counts[img * 2 + 1] = F;
  }
  if (!d_heads) return;
  float* drow = d_heads + (size_t)img * cells * ld;
  for (int i = t; i < A; i += TG_WG) {
    const int a = i % TG_A;
    const float* h = hrow + (size_t)(i / TG_A) * ld;
    float* d = drow + (size_t)(i / TG_A) * ld;
    if (a == 0) for (int c = 60; c < ld; ++c) d[c] = 0.f;
    const float l = labels[base + i];
    if (l == -1.f) {
      for (int c = 0; c < 4; ++c) d[4 * a + c] = 0.f;
      d[40 + 2 * a] = 0.f; d[40 + 2 * a + 1] = 0.f;
      continue;
    }
    const size_t o = (base + i) * 4;
    for (int c = 0; c < 4; ++c) d[4 * a + c] = (float)(tg_box_grad(h[4 * a + c], targets[o + c], inside_w[o + c], outside_w[o + c]) / ((double)F + 1.0));
    double dbg, dfg;
    tg_ce_grad(h[40 + 2 * a], h[40 + 2 * a + 1], l == 1.f ? 1 : 0, dbg, dfg);
    d[40 + 2 * a] = (float)(dbg / (double)K);
    d[40 + 2 * a + 1] = (float)(dfg / (double)K);
  }
}

__global__ __launch_bounds__(TG_THREADS) void tg_overlaps_kernel(const double* __restrict__ boxes, int n, const double* __restrict__ query, int k,
                                                                 double* __restrict__ out, int intersections) {
  __shared__ double lds[TG_CHUNK * 5];
  const long long r0 = (long long)blockIdx.x * TG_ROWS;
  const int t = threadIdx.x;
  for (int c0 = 0; c0 < k; c0 += TG_CHUNK) {
    const int cnt = min(TG_CHUNK, k - c0);
    __syncthreads();
    if (t < cnt) {
      const double* q = query + (size_t)(c0 + t) * 4;
      double* s = lds + t * 5;
      s[0] = q[0]; s[1] = q[1]; s[2] = q[2]; s[3] = q[3];
      s[4] = tg_area(q[0], q[1], q[2], q[3]);
    }
    __syncthreads();
    if (t < cnt) {
      const double* s = lds + t * 5;
      for (int r = 0; r < TG_ROWS && r0 + r < n; ++r) {
        const double* b = boxes + (size_t)(r0 + r) * 4;
        out[(size_t)(r0 + r) * k + c0 + t] = tg_overlap(b[0], b[1], b[2], b[3], tg_area(b[0], b[1], b[2], b[3]), s[0], s[1], s[2], s[3], s[4], intersections != 0);
      }
    }
  }
}

}  // namespace

int launch_bbox_overlaps(const double* boxes, int n, const double* query, int k, double* out, int intersections, hipStream_t s) {
  if (n <= 0 || k <= 0 || !boxes || !query || !out) return fail(CTPN_ERR_ARG, "bbox_overlaps: bad arguments");
  hipLaunchKernelGGL(tg_overlaps_kernel, dim3((unsigned)((n + TG_ROWS - 1) / TG_ROWS)), dim3(TG_THREADS), 0, s, boxes, n, query, k, out, intersections);
  return launch_status("bbox_overlaps");
}

int launch_anchor_targets(int n, int hf, int wf, const float* im_info, const float* gt, const int* offs, int max_g, const int* hard, const float* dc,
                          const int* dc_offs, const TgCfg& cfg, unsigned long long seed, unsigned long long* colmax, int* hardfirst, uint8_t* flags,
                          float* labels, float* targets, float* inside_w, float* outside_w, int* stats, float* presample, double* max_overlap, int* argmax,
                          hipStream_t s) {
  const long long A64 = (long long)hf * wf * TG_A;
  if (n <= 0 || n > 65535 || hf <= 0 || wf <= 0 || A64 > TG_MAX_ANCHORS || max_g < 0 || !im_info || !offs || !colmax || !hardfirst || !flags || !labels || !targets ||
      !inside_w || !outside_w || !stats || !max_overlap || !argmax || (max_g > 0 && !gt) || (dc && !dc_offs) || ((uintptr_t)targets & 15) ||
      ((uintptr_t)inside_w & 15) || ((uintptr_t)outside_w & 15))
    return fail(CTPN_ERR_ARG, "anchor_targets: bad arguments (the three n x hf x wf x 40 arrays are 16-byte aligned)");
  const int A = (int)A64;
  const dim3 grid((unsigned)((A + TG_THREADS - 1) / TG_THREADS), (unsigned)n);
  const int* use_hard = cfg.preclude_hard ? hard : nullptr;
  hipLaunchKernelGGL(tg_scan_kernel, grid, dim3(TG_THREADS), 0, s, A, wf, im_info, gt, offs, colmax, max_overlap, argmax);
  hipLaunchKernelGGL(tg_mark_kernel, grid, dim3(TG_THREADS), 0, s, A, wf, im_info, gt, offs, use_hard, dc, dc_offs, cfg, colmax, hardfirst, max_overlap, argmax,
                     flags, labels, targets);
  if (use_hard && max_g > 0)
    hipLaunchKernelGGL(tg_hard_kernel, dim3((unsigned)((max_g + TG_THREADS - 1) / TG_THREADS), (unsigned)n), dim3(TG_THREADS), 0, s, A, offs, use_hard, hardfirst, flags,
                       labels);
  hipLaunchKernelGGL(tg_sample_kernel, dim3((unsigned)n), dim3(TG_WG), 0, s, A, wf, im_info, cfg, seed, flags, labels, inside_w, outside_w, stats, presample);
  return launch_status("anchor_targets");
}

int launch_rpn_loss(int n, int hf, int wf, const float* heads, int ld, const float* labels, const float* targets, const float* inside_w,
                    const float* outside_w, double* losses, int* counts, float* d_heads, hipStream_t s) {
  const long long A64 = (long long)hf * wf * TG_A;
  if (n <= 0 || hf <= 0 || wf <= 0 || A64 > TG_MAX_ANCHORS || (ld != 60 && ld != 64) || !heads || !labels || !targets || !inside_w || !outside_w || !losses || !counts)
    return fail(CTPN_ERR_ARG, "rpn_loss: bad arguments");
  hipLaunchKernelGGL(tg_loss_kernel, dim3((unsigned)n), dim3(TG_WG), 0, s, (int)A64, heads, ld, labels, targets, inside_w, outside_w, losses, counts, d_heads);
  return launch_status("rpn_loss");
}

}  // namespace ctpn
