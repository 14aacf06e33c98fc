// Host harness of the large text-line connector (csrc/connect.hip, connect_large_kernel): compiles its per-thread source, csrc/connect_dev.h,
// with g++ under AddressSanitizer + UBSan and runs every pass the way the kernel runs it -- a loop over the thread indices of one workgroup
// per image, the passes in the kernel's order, every buffer of exactly the size the launcher gives it (the sanitizers guard the ends).
// csrc/text_connector.cpp is compiled into the same program: every case's records of both modes must equal connect_lines', byte for byte.
// tests/test_dense_pages.py builds this file, writes the cases, runs it as a subprocess and compares the records it writes with the oracle.
//
//   connect_host <cases.bin> <records.bin>
// cases.bin:   int32 cases; per case int32 n, im_h, im_w, gap; float32 scale; float32 boxes[n][4] (kept proposals in rank order, already
//              divided by scale); float32 scores[n]
// records.bin: per case int32 lines_H, lines_O; float64 H[lines_H][9]; float64 O[lines_O][9]
// stdout: one line per case, "ok <case> <n> <lines_H> <lines_O>" or "MISMATCH ..."; exit status 1 on a mismatch, 2 on a bad file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#if defined(__GNUC__) && !defined(__clang__) && __GNUC__ < 12
typedef float _Float16;      // g++ before 12 has no _Float16 in C++; common.h's two fp16 helpers are declared with it and not called here
#endif
#include "../text-detection-ctpn_amd/csrc/text_connector.cpp"      // connect_lines and what it needs (common.h's declarations)
#include "../text-detection-ctpn_amd/csrc/connect_dev.h"

// what text_connector.cpp calls outside itself
namespace ctpn {
static std::string g_err;
void set_error(const std::string& s) { g_err = s; }
int fail(int code, const std::string& s) { g_err = s; return code; }
}  // namespace ctpn
extern "C" int ctpn_nms(int*, int*, const float*, int, int, float, int) { return CTPN_ERR_NODEVICE; }      // (text_lines_host's device NMS: not reached)
extern "C" const char* ctpn_last_error(void) { return ctpn::g_err.c_str(); }

using namespace ctpn;

static constexpr int THREADS = 1024;      // CONNL_THREADS

// connect_large_kernel for one image: -> status (-1: a box outside the image), counts[2], recs [2][cap][9]
static int run_image(const std::vector<float>& boxes, const std::vector<float>& scores, int n, int im_h, int im_w, float scale, const ConnectArgs& ca, int cap,
                     std::vector<double>& recs, int counts[2]) {
  const int stride = n > 0 ? n : 1;
  std::vector<int> keep(stride);
  for (int i = 0; i < stride; ++i) keep[i] = i;
  std::vector<char> work(connl_state_bytes(stride));
  std::vector<double> scratch((size_t)stride * CONNL_REC);
  recs.assign((size_t)2 * cap * 9, 0.0);
  int wf = im_w >> 4;
  const int ncols = wf > CONNL_MAXCOL ? CONNL_MAXCOL : (wf < 1 ? 1 : wf);
  const ConnlState st = connl_views(work.data(), stride);
  std::vector<int> s_sub(THREADS, 0);
  int s_cnt[CONNL_MAXCOL], s_base[CONNL_MAXCOL + 1];
  int bad = 0;
  for (int tid = 0; tid < THREADS; ++tid)
    for (int i = tid; i < n; i += THREADS)
      if (connl_load(i, boxes.data(), scores.data(), keep.data(), stride, scale, ncols, im_w, st)) bad = 1;
  if (bad) { counts[0] = counts[1] = 0; return -1; }
  {   // buckets (the kernel's thread layout: (c, q) = (tid / parts, tid % parts))
    const int parts = THREADS / ncols < 16 ? THREADS / ncols : 16;
    const int seg = (n + parts - 1) / parts;
    auto lo_of = [&](int tid) { const int q = tid % parts; return q * seg < n ? q * seg : n; };
    auto hi_of = [&](int tid) { const int lo = lo_of(tid); return lo + seg < n ? lo + seg : n; };
    for (int tid = 0; tid < THREADS; ++tid) if (tid / parts < ncols) s_sub[tid] = connl_count(tid / parts, lo_of(tid), hi_of(tid), st.col);
    for (int tid = 0; tid < THREADS; ++tid) if (tid < ncols) s_cnt[tid] = connl_group_total(tid, parts, s_sub.data());
    connl_scan(ncols, s_cnt, s_base);
    for (int tid = 0; tid < THREADS; ++tid) if (tid < ncols) connl_group_starts(tid, parts, s_base[tid], s_sub.data());
    for (int tid = 0; tid < THREADS; ++tid) if (tid / parts < ncols) connl_fill(tid / parts, lo_of(tid), hi_of(tid), st.col, s_sub[tid], s_base[tid / parts + 1], st.list);
  }
  for (int tid = 0; tid < THREADS; ++tid) for (int b = tid; b < n; b += THREADS) connl_precursor(b, st, s_base, scale, ncols, ca);
  for (int tid = 0; tid < THREADS; ++tid) for (int i = tid; i < n; i += THREADS) connl_successor(i, st, s_base, scale, ncols, im_w, ca);
  for (int tid = 0; tid < THREADS; ++tid) for (int i = tid; i < n; i += THREADS) connl_chain(i, n, st, im_h, im_w, ca, scratch.data() + (size_t)i * CONNL_REC);
  {   // ordered compaction
    std::vector<int> s_cm[2] = {std::vector<int>(THREADS), std::vector<int>(THREADS)};
    int s_gt[2][32], s_gb[2][33];
    const int per = (n + THREADS - 1) / THREADS;
    auto lo_of = [&](int tid) { return tid * per < n ? tid * per : n; };
    auto hi_of = [&](int tid) { const int lo = lo_of(tid); return lo + per < n ? lo + per : n; };
    for (int tid = 0; tid < THREADS; ++tid) for (int m = 0; m < 2; ++m) s_cm[m][tid] = connl_compact_count(m, lo_of(tid), hi_of(tid), scratch.data());
    for (int tid = 0; tid < 64; ++tid) s_gt[tid >> 5][tid & 31] = connl_group_total(tid & 31, 32, s_cm[tid >> 5].data());
    for (int tid = 0; tid < 2; ++tid) connl_scan(32, s_gt[tid], s_gb[tid]);
    for (int tid = 0; tid < 64; ++tid) connl_group_starts(tid & 31, 32, s_gb[tid >> 5][tid & 31], s_cm[tid >> 5].data());
    for (int tid = 0; tid < THREADS; ++tid)
      for (int m = 0; m < 2; ++m) connl_compact_write(m, lo_of(tid), hi_of(tid), scratch.data(), s_cm[m][tid], recs.data() + (size_t)m * cap * 9, cap);
    for (int m = 0; m < 2; ++m) counts[m] = s_gb[m][32];
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: connect_host cases.bin records.bin\n"); return 2; }
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
  int cases = 0, bad = 0;
  if (std::fread(&cases, 4, 1, in) != 1 || cases < 0 || cases > 4096) return 2;
  for (int k = 0; k < cases; ++k) {
    int hdr[4]; float scale = 1.f;
    if (std::fread(hdr, 4, 4, in) != 4 || std::fread(&scale, 4, 1, in) != 1) return 2;
    const int n = hdr[0], im_h = hdr[1], im_w = hdr[2], gap = hdr[3];
    if (n < 0 || n > CONNL_MAX || im_h < 1 || im_w < 16) return 2;
    std::vector<float> boxes((size_t)n * 4 + 4), scores((size_t)n + 1);
    if ((n && std::fread(boxes.data(), 16, n, in) != (size_t)n) || (n && std::fread(scores.data(), 4, n, in) != (size_t)n)) return 2;
    boxes.resize((size_t)(n > 0 ? n : 1) * 4); scores.resize(n > 0 ? n : 1);
    ConnectorCfg cfg = default_connector_cfg();
    cfg.max_gap = gap;
    const ConnectArgs ca{cfg.max_gap, (float)cfg.max_gap, cfg.min_v_overlaps, cfg.min_size_sim, cfg.min_ratio, cfg.line_min_score, cfg.min_width};
    const int cap = n / 2 > 0 ? n / 2 : 1;
    std::vector<double> recs;
    int counts[2] = {0, 0};
    const int status = run_image(boxes, scores, n, im_h, im_w, scale, ca, cap, recs, counts);
    bool same = true;
    std::string why;
    for (int m = 0; m < 2; ++m) {
      std::vector<double> want;
      const int rc = connect_lines(boxes.data(), scores.data(), n, im_h, im_w, m, cfg, want);
      if ((rc != CTPN_OK) != (status != 0)) { same = false; why = "status"; break; }
      if (rc != CTPN_OK) continue;
      if ((int)(want.size() / 9) != counts[m] || counts[m] > cap) { same = false; why = "count mode " + std::to_string(m) + ": " + std::to_string(want.size() / 9) + " vs " + std::to_string(counts[m]); break; }
      if (counts[m] && std::memcmp(want.data(), recs.data() + (size_t)m * cap * 9, want.size() * sizeof(double)) != 0) { same = false; why = "bytes mode " + std::to_string(m); break; }
    }
    if (!same) { ++bad; std::printf("MISMATCH %d %d %s\n", k, n, why.c_str()); }
    else std::printf("ok %d %d %d %d%s\n", k, n, counts[0], counts[1], status ? " outside" : "");
    for (int m = 0; m < 2; ++m) counts[m] = counts[m] > cap ? cap : counts[m];      // (what is stored)
    std::fwrite(counts, 4, 2, out);
    for (int m = 0; m < 2; ++m) if (counts[m]) std::fwrite(recs.data() + (size_t)m * cap * 9, 72, counts[m], out);
  }
  std::fclose(in);
  if (std::fclose(out) != 0) return 2;
  return bad ? 1 : 0;
}
