// The label side of training (include/ctpn_hip.h, "anchor targets and the RPN loss"): the per-thread text of targets.hip's kernels as host +
// device functions. The kernels call these bodies with their thread index; tests/targets_host.cpp compiles this same text with g++ under
// ASan + UBSan (-ffp-contract=off, as the Makefile gives targets.hip) and calls it from loops over those indices.
//   tg_overlap        one box x query pair of lib/utils/bbox.pyx, both forms: THE overlap expression. The scan pass, the equality pass, the
//                     hard-box rules and ctpn_bbox_overlaps all inline this one body, so a pair has one bit pattern wherever it is computed
//   tg_anchor         anchor idx = (y * wf + x) * 10 + a of generate_anchors' table on the 16-px grid; tg_inside: _allowed_border = 0
//   tg_scan_chunk     a chunk of staged boxes against one anchor: running first maximum and its index, column maxima through `cm`
//   tg_mark_chunk     the same chunk again: is the anchor a column's maximum (np.where(overlaps == gt_max_overlaps)), the hard boxes' maximum
//                     at this anchor, and, through `hf`, the first maximal anchor of every hard box
//   tg_label          the label rules in the reference's order; tg_targets: bbox_transform, rounded to float
//   tg_key            the sampling key; tg_sel_*: the radix select's three steps (does a key belong to the prefix, its bin, the bin that holds rank k)
//   tg_ce_term / tg_box_term / tg_ce_grad / tg_box_grad   one anchor's terms of the loss and of its gradient
// A staged box is TG_BOX doubles: x1, y1, x2, y2, area, column maximum, hard flag. Nothing here includes a HIP header.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TG_HD __host__ __device__ inline
#else
#define TG_HD inline
#endif

namespace ctpn {

constexpr int TG_THREADS = 256;          // scan / mark / overlap kernels
constexpr int TG_CHUNK = 256;            // boxes staged in LDS at a time (ctpn_bbox_overlaps: query boxes)
constexpr int TG_BOX = 7;
constexpr int TG_ROWS = 16;              // ctpn_bbox_overlaps: boxes per workgroup
constexpr int TG_WG = 1024;              // one workgroup per image: sampling and the loss
constexpr int TG_A = 10;
constexpr long long TG_MAX_ANCHORS = 1LL << 24;      // hf * wf * 10 per image
constexpr int TG_NO_ANCHOR = 0x7f7f7f7f;             // a hard box's "first maximal anchor" before any anchor met it (a byte fill)

struct TgCfg {
  double neg, pos, fg_fraction, dc_hi;
  long long batch;
  int clobber, preclude_hard;
  float inside_w[4];
};

// ---- overlaps ----
TG_HD double tg_min(double a, double b) { return b < a ? b : a; }      // Cython's min / max of two C doubles
TG_HD double tg_max(double a, double b) { return b > a ? b : a; }
TG_HD double tg_area(double x1, double y1, double x2, double y2) { return (x2 - x1 + 1.0) * (y2 - y1 + 1.0); }

// bbox.pyx:33-54 (intersections = false: iw ih / (area(box) + area(query) - iw ih)) and :77-93 (true: iw ih / area(query)) for one pair
TG_HD double tg_overlap(double bx1, double by1, double bx2, double by2, double barea, double qx1, double qy1, double qx2, double qy2, double qarea,
                        bool intersections) {
  const double iw = tg_min(bx2, qx2) - tg_max(bx1, qx1) + 1.0;
  if (!(iw > 0.0)) return 0.0;
  const double ih = tg_min(by2, qy2) - tg_max(by1, qy1) + 1.0;
  if (!(ih > 0.0)) return 0.0;
  if (intersections) return iw * ih / qarea;
  const double ua = barea + qarea - iw * ih;
  return iw * ih / ua;
}

// ---- anchors ----
TG_HD void tg_anchor(int wf, long long idx, double& x1, double& y1, double& x2, double& y2) {
  // y1, y2 of generate_anchors' ten base anchors (x1 = 0, x2 = 15): decode.hip's table, tests/golden/anchors.npz
  const int ya[TG_A] = {2, 0, -4, -9, -16, -26, -41, -62, -91, -134};
  const int yb[TG_A] = {13, 15, 19, 24, 31, 41, 56, 77, 106, 149};
  const int a = (int)(idx % TG_A);
  const long long cell = idx / TG_A;
  const int x = (int)(cell % wf), y = (int)(cell / wf);
  x1 = (double)(x * 16);
  x2 = (double)(x * 16 + 15);
  y1 = (double)(y * 16 + ya[a]);
  y2 = (double)(y * 16 + yb[a]);
}
TG_HD bool tg_inside(double x1, double y1, double x2, double y2, float im_h, float im_w) {
  return x1 >= 0.0 && y1 >= 0.0 && x2 < (double)im_w && y2 < (double)im_h;
}

// one ground-truth row (x1, y1, x2, y2, class; float) -> a staged box. cmax: the column's maximum (0 before it is known)
TG_HD void tg_stage_box(const float* gt5, double cmax, int hard, double* s) {
  s[0] = (double)gt5[0]; s[1] = (double)gt5[1]; s[2] = (double)gt5[2]; s[3] = (double)gt5[3];
  s[4] = tg_area(s[0], s[1], s[2], s[3]);
  s[5] = cmax;
  s[6] = hard ? 1.0 : 0.0;
}

// overlaps of one inside anchor with staged boxes g0 .. g0 + cnt - 1: numpy's argmax (the first maximum wins: best starts below every overlap),
// cm(g, ov) for every positive overlap (a column's maximum starts at 0)
template <class ColMax>
TG_HD void tg_scan_chunk(double ax1, double ay1, double ax2, double ay2, double aarea, const double* boxes, int cnt, int g0, double& best, int& arg,
                         ColMax cm) {
  for (int j = 0; j < cnt; ++j) {
    const double* b = boxes + (size_t)j * TG_BOX;
    const double ov = tg_overlap(ax1, ay1, ax2, ay2, aarea, b[0], b[1], b[2], b[3], b[4], false);
    if (ov > best) { best = ov; arg = g0 + j; }
    if (ov > 0.0) cm(g0 + j, ov);
  }
}

// the same pairs again, now that the column maxima are known (b[5]): gtmax |= the anchor attains a column's maximum -- also a maximum of 0,
// the reference's quirk --; hardmax = max over the hard boxes; hf(g) for every hard box whose maximum this anchor attains
template <class HardFirst>
TG_HD void tg_mark_chunk(double ax1, double ay1, double ax2, double ay2, double aarea, const double* boxes, int cnt, int g0, bool& gtmax, double& hardmax,
                         HardFirst hf) {
  for (int j = 0; j < cnt; ++j) {
    const double* b = boxes + (size_t)j * TG_BOX;
    const double ov = tg_overlap(ax1, ay1, ax2, ay2, aarea, b[0], b[1], b[2], b[3], b[4], false);
    const bool top = ov == b[5];
    gtmax = gtmax || top;
    if (b[6] != 0.0) {
      if (ov > hardmax) hardmax = ov;
      if (top) hf(g0 + j);
    }
  }
}

// sum over the dontcare areas of the part of the anchor they cover (bbox_intersections(dontcare, anchors).sum(axis=0)), in index order
TG_HD double tg_dontcare_sum(double ax1, double ay1, double ax2, double ay2, double aarea, const float* dc4, int cnt) {
  double s = 0.0;
  for (int d = 0; d < cnt; ++d) {
    const double x1 = (double)dc4[d * 4], y1 = (double)dc4[d * 4 + 1], x2 = (double)dc4[d * 4 + 2], y2 = (double)dc4[d * 4 + 3];
    s = s + tg_overlap(x1, y1, x2, y2, tg_area(x1, y1, x2, y2), ax1, ay1, ax2, ay2, aarea, true);
  }
  return s;
}

// anchor_target_layer_tf.py:138-173 for one inside anchor, before the hard boxes' first maximal anchors (they need every anchor: a pass of
// their own) -> the label; disabled = the dontcare or the hard rule took it. G = 0 is this library's extension: label 0
TG_HD int tg_label(const TgCfg& c, int G, double best, bool gtmax, bool have_dc, double dcsum, bool have_hard, double hardmax, bool& disabled) {
  int lab = -1;
  if (G == 0) {
    lab = 0;
  } else {
    if (!c.clobber && best < c.neg) lab = 0;
    if (gtmax) lab = 1;
    if (best >= c.pos) lab = 1;
    if (c.clobber && best < c.neg) lab = 0;
  }
  disabled = (have_dc && dcsum > c.dc_hi) || (c.preclude_hard && have_hard && hardmax >= c.pos);
  return disabled ? -1 : lab;
}

// bbox_transform(anchor, gt) (lib/fast_rcnn/bbox_transform.py:10-29), rounded to float once. The reference's mixed precision is kept: the
// anchors are integers, so their side is double arithmetic; gt_rois is the layer's float32 array, so gt's width, height and centre are
// float32 arithmetic (numpy keeps float32 against the Python scalars 1.0 and 0.5), and the differences, quotients and logs are double
TG_HD void tg_targets(double ax1, double ay1, double ax2, double ay2, const float* gt5, float* out4) {
  const double ew = ax2 - ax1 + 1.0, eh = ay2 - ay1 + 1.0;
  const double ecx = ax1 + 0.5 * ew, ecy = ay1 + 0.5 * eh;
  const float gw = gt5[2] - gt5[0] + 1.0f, gh = gt5[3] - gt5[1] + 1.0f;
  const float gcx = gt5[0] + 0.5f * gw, gcy = gt5[1] + 0.5f * gh;
  out4[0] = (float)(((double)gcx - ecx) / ew);
  out4[1] = (float)(((double)gcy - ecy) / eh);
  out4[2] = (float)log((double)gw / ew);
  out4[3] = (float)log((double)gh / eh);
}

// ---- sampling ----
// splitmix64's finaliser over seed ^ (image << 32 | anchor). A bijection of 64 bits: the keys of one image are all different
TG_HD uint64_t tg_key(uint64_t seed, int image, long long anchor) {
  uint64_t z = seed ^ (((uint64_t)(uint32_t)image << 32) | (uint64_t)(uint32_t)anchor);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
// radix select from the top byte down, pass 7 .. 0: does key agree with prefix above the pass's byte; the pass's byte
TG_HD bool tg_sel_match(uint64_t key, uint64_t prefix, int pass) { return pass == 7 || (key >> (8 * pass + 8)) == (prefix >> (8 * pass + 8)); }
TG_HD int tg_sel_bin(uint64_t key, int pass) { return (int)((key >> (8 * pass)) & 255u); }
// the bin that holds the need-th smallest (1-based) of a histogram of at least `need` keys; need becomes the rank inside that bin
TG_HD int tg_sel_pick(const unsigned* hist, unsigned& need) {
  unsigned cum = 0;
  for (int b = 0; b < 256; ++b) {
    if (cum + hist[b] >= need) { need -= cum; return b; }
    cum += hist[b];
  }
  return 255;
}

// ---- loss (Network.build_loss, lib/networks/network.py:367-404), one anchor ----
// sparse softmax cross entropy of a (bg, fg) logit pair, max-shifted
TG_HD double tg_ce_term(float bg, float fg, int label) {
  const double a = (double)bg, b = (double)fg, m = a > b ? a : b;
  return m + log(exp(a - m) + exp(b - m)) - (label == 1 ? b : a);
}
// d ce / d (bg, fg) = softmax - onehot
TG_HD void tg_ce_grad(float bg, float fg, int label, double& dbg, double& dfg) {
  const double a = (double)bg, b = (double)fg, m = a > b ? a : b;
  const double ea = exp(a - m), eb = exp(b - m), s = ea + eb;
  dbg = ea / s - (label == 1 ? 0.0 : 1.0);
  dfg = eb / s - (label == 1 ? 1.0 : 0.0);
}
// outside * smooth_l1(inside * (pred - target)), sigma2 = 9, the strict < of network.py:370: |x| = 1/9 is linear
TG_HD double tg_box_term(float pred, float target, float inside, float outside) {
  const double x = (double)inside * ((double)pred - (double)target), ax = fabs(x);
  const double v = ax < 1.0 / 9.0 ? x * x * 0.5 * 9.0 : ax - 0.5 / 9.0;
  return (double)outside * v;
}
// d of that term / d pred
TG_HD double tg_box_grad(float pred, float target, float inside, float outside) {
  const double x = (double)inside * ((double)pred - (double)target), ax = fabs(x);
  const double d = ax < 1.0 / 9.0 ? 9.0 * x : (x > 0.0 ? 1.0 : -1.0);
  return (double)outside * d * (double)inside;
}

}  // namespace ctpn
