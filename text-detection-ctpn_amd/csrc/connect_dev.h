// The large form of the text-line connector (connect.hip, connect_large_kernel): 1025 .. 4096 kept proposals per image. Per-thread bodies as
// __host__ __device__ text, so that the CPU suite runs them as loops over thread indices (tests/connect_host.cpp), next to
// csrc/text_connector.cpp, whose records they give bit for bit. Needs <math.h> and nothing of the project.
//
// connect_kernel tests every proposal against every other one: 1e6 pair tests at 1000, 1.7e7 at 4096 on one workgroup. Here the proposals
// are first bucketed by anchor column (the column id the column NMS derives, nms_col_of), index order kept inside a column; a proposal then
// looks at the buckets that can hold a pixel column within MAX_HORIZONTAL_GAP only. The column id is monotone in x1, so the pixel columns
// [a, b] lie in the buckets [col(a), col(b)] wherever the boxes sit: nothing here presumes boxes on the anchor grid, the buckets only
// shorten the scan. The pair test, the choice among the matches and every rounding point are connect_kernel's:
//   precursor   the nearest matching pixel column to the left, the maximum score in it;
//   successor   the nearest matching pixel column to the right, the first maximum score in index order;
//   at most one out-edge per node; chains followed from every root in chain order; numpy's pairwise float32 sums (depth 5: 4096 nodes).
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define CONNL_HD __host__ __device__ __forceinline__
#else
#define CONNL_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ctpn {

constexpr int CONNL_MAX = 4096;        // proposals per image the large form holds (CTPN_POST_NMS_CAPACITY_MAX)
constexpr int CONNL_MAXCOL = 256;      // anchor columns (NC_MAXCOL)
constexpr int CONNL_REC = 20;          // doubles per root in the scratch: 9 (H) + keep flag + 9 (O) + keep flag

// the connector's share of ConnectorCfg, by value in the kernel arguments. gap_f = (float)gap (exact: the gap is at most 4096), what the
// reference's `x1 - MAX_HORIZONTAL_GAP` subtracts from the fp32 x1.
struct ConnectArgs {
  int gap; float gap_f;              // MAX_HORIZONTAL_GAP
  float min_v_overlaps, min_size_sim;
  double min_ratio, line_min_score, min_width;
};

// One image's state: views into a block of connl_state_bytes(cap) bytes (device: L2-resident global memory, written and read by the image's
// one workgroup only).
struct ConnlState {
  float *x1, *y1, *x2, *y2, *h, *s, *pmax;
  int* succ;
  unsigned short* list;                // proposal indices, bucketed by anchor column, ascending inside a bucket
  unsigned char *col, *has_in, *has_prec;
};
CONNL_HD size_t connl_state_bytes(int cap) { return (size_t)cap * 40; }      // 7 floats + 1 int + 1 short + 3 bytes = 37, rounded up
CONNL_HD ConnlState connl_views(char* base, int cap) {
  ConnlState st;
  float* f = (float*)base;
  st.x1 = f; st.y1 = f + cap; st.x2 = f + 2 * (size_t)cap; st.y2 = f + 3 * (size_t)cap; st.h = f + 4 * (size_t)cap; st.s = f + 5 * (size_t)cap;
  st.pmax = f + 6 * (size_t)cap;
  st.succ = (int*)(f + 7 * (size_t)cap);
  st.list = (unsigned short*)(base + (size_t)cap * 32);
  st.col = (unsigned char*)(base + (size_t)cap * 34);
  st.has_in = st.col + cap; st.has_prec = st.col + 2 * (size_t)cap;
  return st;
}

// nms_col_of (proposal_dev.h): the anchor column of a box / im_scale
CONNL_HD int connl_col_of(float x1, float cs, int ncols) {
  const int c = (int)(x1 * cs + 0.5f) >> 4;
  return c < 0 ? 0 : (c > ncols - 1 ? ncols - 1 : c);
}

// thread i < n: kept proposal i into the state; true: its x1 lies outside the image (the reference raises IndexError on boxes_table[int(x1)])
CONNL_HD bool connl_load(int i, const float* boxes, const float* scores, const int* keep, int stride, float cs, int ncols, int im_w, const ConnlState& st) {
  int src = keep[i];
  src = src < 0 ? 0 : (src > stride - 1 ? stride - 1 : src);
  const float* b = boxes + (size_t)src * 4;
  st.x1[i] = b[0]; st.y1[i] = b[1]; st.x2[i] = b[2]; st.y2[i] = b[3];
  st.h[i] = b[3] - b[1] + 1.0f;
  st.s[i] = scores[src];
  st.succ[i] = -1; st.has_in[i] = 0;
  st.col[i] = (unsigned char)connl_col_of(b[0], cs, ncols);
  const int pc = (int)b[0];
  return pc < 0 || pc >= im_w;
}

// The stable counting sort, spread over the workgroup: a column's proposals are counted and written by `parts` threads, each over one
// contiguous segment [lo, hi) of the indices (segments in index order keep the index order inside a column).
// thread (c, q): the proposals of anchor column c in the segment, counted ...
CONNL_HD int connl_count(int c, int lo, int hi, const unsigned char* col) {
  int m = 0;
  for (int i = lo; i < hi; ++i) m += col[i] == c ? 1 : 0;
  return m;
}
// ... and, once its start is known, written in index order
CONNL_HD void connl_fill(int c, int lo, int hi, const unsigned char* col, int pos, int end, unsigned short* list) {
  for (int i = lo; i < hi; ++i)
    if (col[i] == c && pos < end) list[pos++] = (unsigned short)i;
}
// Counts -> starts over groups x parts entries in (group, part) order, in three steps: thread g sums its group's parts; one thread scans the
// groups (base[g] = entries below group g, base[groups] = all); thread g turns its group's counts into starts. The bucket fill (groups =
// anchor columns) and the ordered compaction (32 groups of 32 threads) both use it.
CONNL_HD int connl_group_total(int g, int parts, const int* cnt) {
  int sum = 0;
  for (int q = 0; q < parts; ++q) sum += cnt[g * parts + q];
  return sum;
}
CONNL_HD void connl_scan(int groups, const int* totals, int* base) {
  int run = 0;
  for (int g = 0; g < groups; ++g) { base[g] = run; run += totals[g]; }
  base[groups] = run;
}
CONNL_HD void connl_group_starts(int g, int parts, int start, int* cnt) {
  for (int q = 0; q < parts; ++q) { const int v = cnt[g * parts + q]; cnt[g * parts + q] = start; start += v; }
}

CONNL_HD bool connl_meet_v_iou(const ConnlState& st, int a, int b, const ConnectArgs& ca) {
  const float h1 = st.h[a], h2 = st.h[b];
  const float y0 = fmaxf(st.y1[b], st.y1[a]);
  const float y1m = fminf(st.y2[b], st.y2[a]);
  const float ov = fmaxf(0.0f, y1m - y0 + 1.0f) / fminf(h1, h2);
  const float sim = fminf(h1, h2) / fmaxf(h1, h2);
  return ov >= ca.min_v_overlaps && sim >= ca.min_size_sim;
}

// thread b < n: the precursors of b -- nearest matching pixel column to the left within MAX_HORIZONTAL_GAP px, the maximum score in it
CONNL_HD void connl_precursor(int b, const ConnlState& st, const int* base, float cs, int ncols, const ConnectArgs& ca) {
  const int colb = (int)st.x1[b];
  int lo = (int)(st.x1[b] - ca.gap_f);
  lo = lo < 0 ? 0 : lo;
  const int p0 = base[connl_col_of((float)lo, cs, ncols)], p1 = base[(int)st.col[b] + 1];
  int cbest = -1;
  float pmax = -INFINITY;
  for (int p = p0; p < p1; ++p) {
    const int k = st.list[p];
    const int ck = (int)st.x1[k];
    if (ck < lo || ck >= colb || ck < cbest) continue;
    if (!connl_meet_v_iou(st, k, b, ca)) continue;
    if (ck > cbest) { cbest = ck; pmax = st.s[k]; }
    else pmax = fmaxf(pmax, st.s[k]);
  }
  st.has_prec[b] = cbest >= 0;
  st.pmax[b] = pmax;
}

// thread i < n, behind connl_precursor of every node: the successor of i -- nearest matching pixel column to the right, the first maximum
// score in index order (a pixel column may spread over two buckets where boxes are off the grid: the lower index wins a tie explicitly)
CONNL_HD void connl_successor(int i, const ConnlState& st, const int* base, float cs, int ncols, int im_w, const ConnectArgs& ca) {
  const int coli = (int)st.x1[i];
  const int hi = coli + ca.gap < im_w - 1 ? coli + ca.gap : im_w - 1;
  if (hi <= coli) return;
  const int p0 = base[st.col[i]], p1 = base[connl_col_of((float)(hi + 1), cs, ncols) + 1];
  int cbest = 0x7fffffff, best = -1;
  for (int p = p0; p < p1; ++p) {
    const int j = st.list[p];
    const int cj = (int)st.x1[j];
    if (cj <= coli || cj > hi || cj > cbest) continue;
    if (!connl_meet_v_iou(st, j, i, ca)) continue;
    if (cj < cbest) { cbest = cj; best = j; }
    else if (st.s[j] > st.s[best] || (st.s[j] == st.s[best] && j < best)) best = j;
  }
  if (best >= 0 && st.has_prec[best] && st.s[i] >= st.pmax[best]) { st.succ[i] = best; st.has_in[best] = 1; }
}

// np.polyfit(X, Y, 1) over a chain: double least squares, coefficients rounded to fp32 (polyfit1 of text_connector.cpp, same op order)
template <typename FX, typename FY>
CONNL_HD void connl_polyfit1(const int* succ, int root, int len, FX fx, FY fy, float& c0, float& c1) {
  double mx = 0, my = 0;
  int v = root;
  for (int q = 0; q < len; ++q, v = succ[v]) { mx += fx(v); my += fy(v); }
  mx /= (double)len; my /= (double)len;
  double sxx = 0, sxy = 0;
  v = root;
  for (int q = 0; q < len; ++q, v = succ[v]) {
    const double dx = fx(v) - mx;
    sxx += dx * dx;
    sxy += dx * (fy(v) - my);
  }
  const double slope = sxx > 0 ? sxy / sxx : 0.0;
  c0 = (float)slope;
  c1 = (float)(my - slope * mx);
}

CONNL_HD float connl_clampf(float v, float lo, float hi) { return fmaxf(fminf(v, hi), lo); }

// numpy's pairwise float32 sum above 128 elements: halves (the left one a multiple of 8), recursively; `leaf` consumes the next m chain
// nodes in order. D bounds the depth at compile time (m <= 128 << D).
template <int D, typename Leaf>
CONNL_HD void connl_sum_rec(int m, float& rs, float& rh, Leaf& leaf) {
  if constexpr (D > 0) {
    if (m > 128) {
      int n2 = m / 2;
      n2 -= n2 % 8;
      float s0, h0, s1, h1;
      connl_sum_rec<D - 1>(n2, s0, h0, leaf);
      connl_sum_rec<D - 1>(m - n2, s1, h1, leaf);
      rs = s0 + s1; rh = h0 + h1;
      return;
    }
  }
  leaf(m, rs, rh);
}

// thread i < n, behind connl_successor of every node: if i is a chain's root, the chain's records of both modes and whether they pass
// filter_boxes, into o[CONNL_REC]; n bounds the walk (a chain visits a node once: its pixel columns ascend)
CONNL_HD void connl_chain(int i, int n, const ConnlState& st, int im_h, int im_w, const ConnectArgs& ca, double* o) {
  o[9] = 0.0; o[19] = 0.0;
  if (st.has_in[i] || st.succ[i] < 0) return;
  const float *sx1 = st.x1, *sy1 = st.y1, *sx2 = st.x2, *sy2 = st.y2, *ss = st.s;
  const int* ssucc = st.succ;
  const float wl = (float)(im_w - 1), hl = (float)(im_h - 1);
  int len = 0;
  float x0 = INFINITY, x1m = -INFINITY;
  bool same_x = true;
  for (int v = i; v >= 0 && len < n; v = ssucc[v]) {
    ++len;
    x0 = fminf(x0, sx1[v]); x1m = fmaxf(x1m, sx2[v]);
    if (sx1[v] != sx1[i]) same_x = false;
  }
  // line score and mean height: numpy's float32 pairwise add.reduce over the chain in order (np_sum_f32 in text_connector.cpp); a chain
  // holds at most CONNL_MAX = 128 << 5 nodes
  float ssum, hsum;
  {
    int v = i;
    auto leaf = [&](int m, float& rs, float& rh) {          // consumes m chain nodes starting at v
      if (m < 8) {
        rs = 0.f; rh = 0.f;
        for (int q = 0; q < m; ++q, v = ssucc[v]) { rs += ss[v]; rh += sy2[v] - sy1[v]; }
        return;
      }
      float as[8], ah[8];
      for (int j = 0; j < 8; ++j, v = ssucc[v]) { as[j] = ss[v]; ah[j] = sy2[v] - sy1[v]; }
      int q = 8;
      for (; q < m - (m % 8); q += 8)
        for (int j = 0; j < 8; ++j, v = ssucc[v]) { as[j] += ss[v]; ah[j] += sy2[v] - sy1[v]; }
      rs = ((as[0] + as[1]) + (as[2] + as[3])) + ((as[4] + as[5]) + (as[6] + as[7]));
      rh = ((ah[0] + ah[1]) + (ah[2] + ah[3])) + ((ah[4] + ah[5]) + (ah[6] + ah[7]));
      for (; q < m; ++q, v = ssucc[v]) { rs += ss[v]; rh += sy2[v] - sy1[v]; }
    };
    connl_sum_rec<5>(len, ssum, hsum, leaf);
  }
  const float offset = (sx2[i] - sx1[i]) * 0.5f;
  const float xa = x0 + offset, xb = x1m - offset;
  float lt, rt, lb, rb;
  if (same_x) { lt = rt = sy1[i]; lb = rb = sy2[i]; }
  else {
    float c0, c1;
    connl_polyfit1(ssucc, i, len, [&](int v) { return (double)sx1[v]; }, [&](int v) { return (double)sy1[v]; }, c0, c1);
    lt = c0 * xa + c1; rt = c0 * xb + c1;
    connl_polyfit1(ssucc, i, len, [&](int v) { return (double)sx1[v]; }, [&](int v) { return (double)sy2[v]; }, c0, c1);
    lb = c0 * xa + c1; rb = c0 * xb + c1;
  }
  const float score = ssum / (float)len;
  const float top = fminf(lt, rt), bot = fmaxf(lb, rb);
  {   // H: clip_boxes (also clips the score column: reference quirk), 4-corner layout
    const float xmin = connl_clampf(x0, 0.f, wl), xmax = connl_clampf(x1m, 0.f, wl);
    const float ymin = connl_clampf(top, 0.f, hl), ymax = connl_clampf(bot, 0.f, hl);
    const float sc = connl_clampf(score, 0.f, wl);
    o[0] = xmin; o[1] = ymin; o[2] = xmax; o[3] = ymin; o[4] = xmin; o[5] = ymax; o[6] = xmax; o[7] = ymax; o[8] = sc;
  }
  {   // O: centre-line fit, height = mean(h) + 2.5, parallelogram + skew compensation, no clipping
    float k, b;
    connl_polyfit1(ssucc, i, len, [&](int v) { return (double)((sx1[v] + sx2[v]) / 2.0f); }, [&](int v) { return (double)((sy1[v] + sy2[v]) / 2.0f); }, k, b);
    const float height = hsum / (float)len + 2.5f;
    const float b1 = b - height / 2.0f, b2 = b + height / 2.0f;
    float px1 = x0, py1 = k * x0 + b1;
    float px2 = x1m, py2 = k * x1m + b1;
    float px3 = x0, py3 = k * x0 + b2;
    float px4 = x1m, py4 = k * x1m + b2;
    const float disX = px2 - px1, disY = py2 - py1;
    const float width = sqrtf(disX * disX + disY * disY);
    const float fTmp0 = py3 - py1;
    const float fTmp1 = fTmp0 * disY / width;
    const float dx = fabsf(fTmp1 * disX / width);
    const float dy = fabsf(fTmp1 * disY / width);
    if (k < 0) { px1 -= dx; py1 += dy; px4 += dx; py4 -= dy; }
    else { px2 += dx; py2 += dy; px3 -= dx; py3 -= dy; }
    o[10] = px1; o[11] = py1; o[12] = px2; o[13] = py2; o[14] = px3; o[15] = py3; o[16] = px4; o[17] = py4; o[18] = score;
  }
  for (int m = 0; m < 2; ++m) {   // filter_boxes in float64
    const double* r = o + 10 * m;
    const double heights = (fabs(r[5] - r[1]) + fabs(r[7] - r[3])) / 2.0 + 1;
    const double widths = (fabs(r[2] - r[0]) + fabs(r[6] - r[4])) / 2.0 + 1;
    o[10 * m + 9] = (widths / heights > ca.min_ratio && r[8] > ca.line_min_score && widths > ca.min_width) ? 1.0 : 0.0;
  }
}

// behind connl_chain of every node, the records of mode m that passed the filter, in root order (the reference's loop order): thread t
// counts those of its contiguous share [lo, hi) of the roots ...
CONNL_HD int connl_compact_count(int m, int lo, int hi, const double* scr) {
  int c = 0;
  for (int i = lo; i < hi; ++i) c += scr[(size_t)i * CONNL_REC + 10 * m + 9] != 0.0 ? 1 : 0;
  return c;
}
// ... and, once it knows how many lie before them (pos), stores them into dst[cap][9], those below cap
CONNL_HD void connl_compact_write(int m, int lo, int hi, const double* scr, int pos, double* dst, int cap) {
  for (int i = lo; i < hi; ++i) {
    const double* o = scr + (size_t)i * CONNL_REC + 10 * m;
    if (o[9] != 0.0) {
      if (pos < cap) for (int q = 0; q < 9; ++q) dst[(size_t)pos * 9 + q] = o[q];
      ++pos;
    }
  }
}

}  // namespace ctpn
