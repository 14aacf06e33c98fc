// Text-line tail on device: the connector's front end (score filter, boxes / im_scale) and the connector itself; its NMS 0.2 is nms.hip's.
#include "common.h"
#include "connect_dev.h"      // ConnectArgs; the large form's per-thread bodies

#pragma clang fp contract(off)

namespace ctpn {

// text-connector front end on device (reference lib/text_connector/detectors.py:21-26 + lib/fast_rcnn/test.py:57):
// rois are already in descending score order, so "score > 0.7, then sort" is the prefix of rows above the
// threshold; boxes are divided by im_scale exactly as test_ctpn does before the connector sees them.
__global__ __launch_bounds__(256) void lines_prep_kernel(const float* __restrict__ rois, const int* __restrict__ roi_counts,
                                                         const float* __restrict__ im_info, int post, float min_score,
                                                         float* __restrict__ tl_boxes, float* __restrict__ tl_scores,
                                                         int* __restrict__ tl_counts) {
  const int img = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= post) return;
  const int cnt = roi_counts[img];
  const float scale = im_info[img * 3 + 2];
  const float* r = rois + ((long long)img * post + i) * 5;
  const bool ok = i < cnt && r[0] > min_score;
  if (ok) {
    *(float4*)(tl_boxes + ((long long)img * post + i) * 4) = make_float4(r[1] / scale, r[2] / scale, r[3] / scale, r[4] / scale);
    tl_scores[(long long)img * post + i] = r[0];
    const bool next_ok = (i + 1 < cnt) && (i + 1 < post) && (r[5] > min_score);
    if (!next_ok) tl_counts[img] = i + 1;
  } else if (i == 0) {
    tl_counts[img] = 0;
  }
}

int launch_lines_prep(const float* rois, const int* roi_counts, const float* im_info, int post, float min_score,
                      float* tl_boxes, float* tl_scores, int* tl_counts, int n_img, hipStream_t s) {
  dim3 grid((post + 255) / 256, n_img);
  hipLaunchKernelGGL(lines_prep_kernel, grid, dim3(256), 0, s, rois, roi_counts, im_info, post, min_score, tl_boxes, tl_scores,
                     tl_counts);
  return launch_status("lines_prep");
}

// ---------------------------------------------------------------------------------------------
// Text-line connector on the device: TextProposalGraphBuilder.build_graph
// (lib/text_connector/text_proposal_graph_builder.py:6-78), Graph.sub_graphs_connected (other.py:20-29),
// TextProposalConnector.get_text_lines H (text_proposal_connector.py:21-64) and O
// (text_proposal_connector_oriented.py:24-105), clip_boxes (other.py:7-13) and TextDetector.filter_boxes
// (detectors.py:37-49) for the proposals that survived the score filter, the sort and NMS 0.2 (rows in descending score
// order). One workgroup per image, the proposals (<= 1000) in LDS; every fp32 / fp64 rounding point is the one of the
// host restatement csrc/text_connector.cpp (the two are compared bit for bit in tests/test_gpu_parity.py).
//   * the reference's column table (proposals bucketed by int(x1), searched column by column up to 50 px away) becomes an
//     all-pairs scan per proposal that keeps the NEAREST matching column and, inside it, the first maximum score in table
//     (= index) order: n^2 <= 1e6 cheap pair tests per image instead of pointer chasing;
//   * a node has at most one out-edge; chains are followed from every root by one thread each, three passes over the chain
//     (sums in chain order: the fp32 / fp64 results do not depend on the thread count);
//   * records of BOTH modes are produced (DETECT_MODE is an argument of ctpn_detect_collect, not of the submit).
// ---------------------------------------------------------------------------------------------
constexpr int CONN_MAX = 1024;          // proposals per image held in LDS (RPN_POST_NMS_TOP_N up to 1024; above: connect_large_kernel, below)

__device__ __forceinline__ bool conn_meet_v_iou(const float* y1, const float* y2, const float* hh, int a, int b, const ConnectArgs& ca) {
  const float h1 = hh[a], h2 = hh[b];
  const float y0 = fmaxf(y1[b], y1[a]);
  const float y1m = fminf(y2[b], y2[a]);
  const float ov = fmaxf(0.0f, y1m - y0 + 1.0f) / fminf(h1, h2);
  const float sim = fminf(h1, h2) / fmaxf(h1, h2);
  return ov >= ca.min_v_overlaps && sim >= ca.min_size_sim;
}

// np.polyfit(X, Y, 1) over a chain: double least squares, coefficients rounded to fp32 (same op order as polyfit1 on the host)
template <typename FX, typename FY>
__device__ __forceinline__ void conn_polyfit1(const int* succ, int root, int len, FX fx, FY fy, float& c0, float& c1) {
  double mx = 0, my = 0;
  for (int v = root; v >= 0; v = succ[v]) { mx += fx(v); my += fy(v); }
  mx /= (double)len; my /= (double)len;
  double sxx = 0, sxy = 0;
  for (int v = root; v >= 0; v = succ[v]) {
    const double dx = fx(v) - mx;
    sxx += dx * dx;
    sxy += dx * (fy(v) - my);
  }
  const double slope = sxx > 0 ? sxy / sxx : 0.0;
  c0 = (float)slope;
  c1 = (float)(my - slope * mx);
}

__device__ __forceinline__ float conn_clampf(float v, float lo, float hi) { return fmaxf(fminf(v, hi), lo); }

// numpy's pairwise float32 sum above 128 elements: halves (the left one a multiple of 8), recursively; `leaf` consumes the next m
// chain nodes in order. D bounds the depth at compile time (m <= 128 << D).
template <int D, typename Leaf>
__device__ __forceinline__ void conn_sum_rec(int m, float& rs, float& rh, Leaf& leaf) {
  if constexpr (D > 0) {
    if (m > 128) {
      int n2 = m / 2;
      n2 -= n2 % 8;
      float s0, h0, s1, h1;
      conn_sum_rec<D - 1>(n2, s0, h0, leaf);
      conn_sum_rec<D - 1>(m - n2, s1, h1, leaf);
      rs = s0 + s1; rh = h0 + h1;
      return;
    }
  }
  leaf(m, rs, rh);
}

__global__ __launch_bounds__(256) void connect_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                      const int* __restrict__ keep, const int* __restrict__ keep_counts, int stride,
                                                      const float* __restrict__ im_info, double* __restrict__ recs, int* __restrict__ counts,
                                                      double* __restrict__ scratch, int cap, const ConnectArgs ca) {
  __shared__ float sx1[CONN_MAX], sy1[CONN_MAX], sx2[CONN_MAX], sy2[CONN_MAX], sh[CONN_MAX], ss[CONN_MAX];
  __shared__ float spmax[CONN_MAX];
  __shared__ int ssucc[CONN_MAX];
  __shared__ unsigned char shas_in[CONN_MAX], shas_prec[CONN_MAX];
  __shared__ int sbad;
  const int img = blockIdx.x, tid = threadIdx.x;
  int n = keep_counts[img];
  n = n < 0 ? 0 : (n > CONN_MAX ? CONN_MAX : n);
  const int im_h = (int)im_info[3 * img], im_w = (int)im_info[3 * img + 1];
  if (tid == 0) sbad = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const int src = keep[(size_t)img * stride + i];
    const float4 b = *(const float4*)(boxes + ((size_t)img * stride + src) * 4);
    sx1[i] = b.x; sy1[i] = b.y; sx2[i] = b.z; sy2[i] = b.w;
    sh[i] = b.w - b.y + 1.0f;
    ss[i] = scores[(size_t)img * stride + src];
    ssucc[i] = -1; shas_in[i] = 0;
    const int col = (int)b.x;
    if (col < 0 || col >= im_w) sbad = 1;                 // the reference raises IndexError on boxes_table[int(x1)]
  }
  __syncthreads();
  int* cnt2 = counts + (size_t)img * 3;                    // lines H, lines O, status
  if (sbad) { if (tid == 0) { cnt2[0] = 0; cnt2[1] = 0; cnt2[2] = -1; } return; }

  // precursors of every node: nearest matching column to the left within MAX_HORIZONTAL_GAP px, max score in it
  for (int b = tid; b < n; b += 256) {
    const int colb = (int)sx1[b];
    int lo = (int)(sx1[b] - ca.gap_f);
    lo = lo < 0 ? 0 : lo;
    int cbest = -1;
    float pmax = -INFINITY;
    for (int k = 0; k < n; ++k) {
      const int ck = (int)sx1[k];
      if (ck < lo || ck >= colb || ck < cbest) continue;
      if (!conn_meet_v_iou(sy1, sy2, sh, k, b, ca)) continue;
      if (ck > cbest) { cbest = ck; pmax = ss[k]; }
      else pmax = fmaxf(pmax, ss[k]);
    }
    shas_prec[b] = cbest >= 0;
    spmax[b] = pmax;
  }
  __syncthreads();
  // successors: nearest matching column to the right within MAX_HORIZONTAL_GAP px, first maximum score in index order
  for (int i = tid; i < n; i += 256) {
    const int coli = (int)sx1[i];
    const int hi = coli + ca.gap < im_w - 1 ? coli + ca.gap : im_w - 1;
    int cbest = 0x7fffffff, best = -1;
    for (int j = 0; j < n; ++j) {
      const int cj = (int)sx1[j];
      if (cj <= coli || cj > hi || cj > cbest) continue;
      if (!conn_meet_v_iou(sy1, sy2, sh, j, i, ca)) continue;
      if (cj < cbest) { cbest = cj; best = j; }
      else if (ss[j] > ss[best]) best = j;
    }
    if (best >= 0 && shas_prec[best] && ss[i] >= spmax[best]) { ssucc[i] = best; shas_in[best] = 1; }
  }
  __syncthreads();

  // chains -> records (both modes) into per-root scratch slots; flag = passes filter_boxes
  double* scr = scratch + (size_t)img * CONN_MAX * 20;      // per root: 9 (H) + 1 (H keep) + 9 (O) + 1 (O keep)
  const float wl = (float)(im_w - 1), hl = (float)(im_h - 1);
  for (int i = tid; i < n; i += 256) {
    double* o = scr + (size_t)i * 20;
    o[9] = 0.0; o[19] = 0.0;
    if (shas_in[i] || ssucc[i] < 0) continue;
    int len = 0;
    float x0 = INFINITY, x1m = -INFINITY;
    bool same_x = true;
    for (int v = i; v >= 0; v = ssucc[v]) {
      ++len;
      x0 = fminf(x0, sx1[v]); x1m = fmaxf(x1m, sx2[v]);
      if (sx1[v] != sx1[i]) same_x = false;
    }
    // line score and mean height: numpy's float32 pairwise add.reduce over the chain in order (see np_sum_f32 in text_connector.cpp).
    // numpy splits recursively above 128 elements (left half a multiple of 8); a chain holds at most the image's <= 1000 kept
    // proposals, i.e. at most three levels (conn_sum_rec<3>: up to 1024).
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
#pragma unroll
        for (int j = 0; j < 8; ++j, v = ssucc[v]) { as[j] = ss[v]; ah[j] = sy2[v] - sy1[v]; }
        int q = 8;
        for (; q < m - (m % 8); q += 8) {
#pragma unroll
          for (int j = 0; j < 8; ++j, v = ssucc[v]) { as[j] += ss[v]; ah[j] += sy2[v] - sy1[v]; }
        }
        rs = ((as[0] + as[1]) + (as[2] + as[3])) + ((as[4] + as[5]) + (as[6] + as[7]));
        rh = ((ah[0] + ah[1]) + (ah[2] + ah[3])) + ((ah[4] + ah[5]) + (ah[6] + ah[7]));
        for (; q < m; ++q, v = ssucc[v]) { rs += ss[v]; rh += sy2[v] - sy1[v]; }
      };
      conn_sum_rec<3>(len, ssum, hsum, leaf);
    }
    const float offset = (sx2[i] - sx1[i]) * 0.5f;
    const float xa = x0 + offset, xb = x1m - offset;
    float lt, rt, lb, rb;
    if (same_x) { lt = rt = sy1[i]; lb = rb = sy2[i]; }
    else {
      float c0, c1;
      conn_polyfit1(ssucc, i, len, [&](int v) { return (double)sx1[v]; }, [&](int v) { return (double)sy1[v]; }, c0, c1);
      lt = c0 * xa + c1; rt = c0 * xb + c1;
      conn_polyfit1(ssucc, i, len, [&](int v) { return (double)sx1[v]; }, [&](int v) { return (double)sy2[v]; }, c0, c1);
      lb = c0 * xa + c1; rb = c0 * xb + c1;
    }
    const float score = ssum / (float)len;
    const float top = fminf(lt, rt), bot = fmaxf(lb, rb);
    {   // H: clip_boxes (also clips the score column: reference quirk), 4-corner layout
      const float xmin = conn_clampf(x0, 0.f, wl), xmax = conn_clampf(x1m, 0.f, wl);
      const float ymin = conn_clampf(top, 0.f, hl), ymax = conn_clampf(bot, 0.f, hl);
      const float sc = conn_clampf(score, 0.f, wl);
      o[0] = xmin; o[1] = ymin; o[2] = xmax; o[3] = ymin; o[4] = xmin; o[5] = ymax; o[6] = xmax; o[7] = ymax; o[8] = sc;
    }
    {   // O: centre-line fit, height = mean(h) + 2.5, parallelogram + skew compensation, no clipping
      float k, b;
      conn_polyfit1(ssucc, i, len, [&](int v) { return (double)((sx1[v] + sx2[v]) / 2.0f); }, [&](int v) { return (double)((sy1[v] + sy2[v]) / 2.0f); }, k, b);
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
#pragma unroll
    for (int m = 0; m < 2; ++m) {   // filter_boxes in float64
      const double* r = o + 10 * m;
      const double heights = (fabs(r[5] - r[1]) + fabs(r[7] - r[3])) / 2.0 + 1;
      const double widths = (fabs(r[2] - r[0]) + fabs(r[6] - r[4])) / 2.0 + 1;
      o[10 * m + 9] = (widths / heights > ca.min_ratio && r[8] > ca.line_min_score && widths > ca.min_width) ? 1.0 : 0.0;
    }
  }
  __syncthreads();
  __threadfence_block();
  // ordered compaction (roots in ascending index = the reference's loop order): two threads, one per mode
  if (tid < 2) {
    const int m = tid;
    int c = 0;
    double* dst = recs + ((size_t)img * 2 + m) * cap * 9;
    for (int i = 0; i < n; ++i) {
      const double* o = scr + (size_t)i * 20 + 10 * m;
      if (o[9] != 0.0) {
        if (c < cap) for (int q = 0; q < 9; ++q) dst[(size_t)c * 9 + q] = o[q];
        ++c;
      }
    }
    cnt2[m] = c;
    if (m == 0) cnt2[2] = 0;
  }
}

// ---------------------------------------------------------------------------------------------
// The large form: 1025 .. CONNL_MAX kept proposals per image (a ctx whose ctpn_reserve_proposals raised its capacity). One workgroup of
// 1024 threads per image; the image's state lives in its own block of `work` (global memory, a few hundred KB: L2-resident), the bucket
// starts in LDS. Every per-thread body is connect_dev.h's, where the scheme is described; every loop there runs over a range fixed before it
// starts (n, a bucket range, a chain of at most n nodes), no workgroup waits on another, and every index stored to is below n <= cap rows.
// ---------------------------------------------------------------------------------------------
constexpr int CONNL_THREADS = 1024;
__global__ __launch_bounds__(CONNL_THREADS) void connect_large_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                                      const int* __restrict__ keep, const int* __restrict__ keep_counts, int stride,
                                                                      const float* __restrict__ im_info, double* __restrict__ recs, int* __restrict__ counts,
                                                                      double* __restrict__ scratch, char* __restrict__ work, int cap, int ncols, const ConnectArgs ca) {
  __shared__ int s_sub[CONNL_THREADS], s_cnt[CONNL_MAXCOL], s_base[CONNL_MAXCOL + 1];
  __shared__ int s_cm[2][CONNL_THREADS], s_gt[2][32], s_gb[2][33];
  __shared__ int sbad;
  const int img = blockIdx.x, tid = threadIdx.x;
  int n = keep_counts[img];
  n = n < 0 ? 0 : (n > stride ? stride : n);
  const int im_h = (int)im_info[3 * img], im_w = (int)im_info[3 * img + 1];
  const float cs = im_info[3 * img + 2];
  const ConnlState st = connl_views(work + (size_t)img * connl_state_bytes(stride), stride);
  if (tid == 0) sbad = 0;
  __syncthreads();
  for (int i = tid; i < n; i += CONNL_THREADS)
    if (connl_load(i, boxes + (size_t)img * stride * 4, scores + (size_t)img * stride, keep + (size_t)img * stride, stride, cs, ncols, im_w, st)) sbad = 1;
  __syncthreads();
  int* cnt2 = counts + (size_t)img * 3;                    // lines H, lines O, status
  if (sbad) { if (tid == 0) { cnt2[0] = 0; cnt2[1] = 0; cnt2[2] = -1; } return; }
  {   // buckets: thread (c, q) = (tid / parts, tid % parts) takes column c's proposals of index segment q; ncols x parts <= 1024 threads
    const int parts = CONNL_THREADS / ncols < 16 ? CONNL_THREADS / ncols : 16;
    const int seg = (n + parts - 1) / parts;
    const int c = tid / parts, q = tid % parts;
    const bool active = c < ncols;
    const int lo = q * seg < n ? q * seg : n, hi = lo + seg < n ? lo + seg : n;
    if (active) s_sub[tid] = connl_count(c, lo, hi, st.col);
    __syncthreads();
    if (tid < ncols) s_cnt[tid] = connl_group_total(tid, parts, s_sub);
    __syncthreads();
    if (tid == 0) connl_scan(ncols, s_cnt, s_base);
    __syncthreads();
    if (tid < ncols) connl_group_starts(tid, parts, s_base[tid], s_sub);
    __syncthreads();
    if (active) connl_fill(c, lo, hi, st.col, s_sub[tid], s_base[c + 1], st.list);
    __syncthreads();
  }
  for (int b = tid; b < n; b += CONNL_THREADS) connl_precursor(b, st, s_base, cs, ncols, ca);
  __syncthreads();
  for (int i = tid; i < n; i += CONNL_THREADS) connl_successor(i, st, s_base, cs, ncols, im_w, ca);
  __syncthreads();
  double* scr = scratch + (size_t)img * stride * CONNL_REC;
  for (int i = tid; i < n; i += CONNL_THREADS) connl_chain(i, n, st, im_h, im_w, ca, scr + (size_t)i * CONNL_REC);
  __syncthreads();
  {   // ordered compaction: thread t's contiguous share of the roots, 32 groups of 32 threads, one scan per mode
    const int per = (n + CONNL_THREADS - 1) / CONNL_THREADS;
    const int lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    for (int m = 0; m < 2; ++m) s_cm[m][tid] = connl_compact_count(m, lo, hi, scr);
    __syncthreads();
    if (tid < 64) s_gt[tid >> 5][tid & 31] = connl_group_total(tid & 31, 32, s_cm[tid >> 5]);
    __syncthreads();
    if (tid < 2) connl_scan(32, s_gt[tid], s_gb[tid]);
    __syncthreads();
    if (tid < 64) connl_group_starts(tid & 31, 32, s_gb[tid >> 5][tid & 31], s_cm[tid >> 5]);
    __syncthreads();
    for (int m = 0; m < 2; ++m) connl_compact_write(m, lo, hi, scr, s_cm[m][tid], recs + ((size_t)img * 2 + m) * cap * 9, cap);
    if (tid < 2) cnt2[tid] = s_gb[tid][32];
    if (tid == 0) cnt2[2] = 0;
  }
}

// stride <= 1024: connect_kernel (scratch [n_img][1024][20]); above: connect_large_kernel (scratch [n_img][stride][20], work n_img x
// connl_state_bytes(stride), ncols = anchor columns of the widest image)
int launch_connect(const float* boxes, const float* scores, const int* keep, const int* keep_counts, int stride, const float* im_info,
                   double* recs, int* counts, double* scratch, int cap, int n_img, const ConnectorCfg& cfg, hipStream_t s, char* work, int ncols) {
  const ConnectArgs ca{cfg.max_gap, (float)cfg.max_gap, cfg.min_v_overlaps, cfg.min_size_sim, cfg.min_ratio, cfg.line_min_score, cfg.min_width};
  if (stride > CONN_MAX) {
    if (stride > CONNL_MAX || !work || ncols < 1 || ncols > CONNL_MAXCOL)
      return fail(CTPN_ERR_ARG, "connect: the large form takes up to 4096 proposals per image in up to 256 anchor columns, and needs its state block");
    hipLaunchKernelGGL(connect_large_kernel, dim3(n_img), dim3(CONNL_THREADS), 0, s, boxes, scores, keep, keep_counts, stride, im_info, recs, counts, scratch,
                       work, cap, ncols, ca);
    return launch_status("connect_large");
  }
  hipLaunchKernelGGL(connect_kernel, dim3(n_img), dim3(256), 0, s, boxes, scores, keep, keep_counts, stride, im_info, recs, counts, scratch, cap, ca);
  return launch_status("connect");
}
size_t connect_work_bytes(int stride) { return stride > CONN_MAX ? connl_state_bytes(stride) : 0; }

}  // namespace ctpn
