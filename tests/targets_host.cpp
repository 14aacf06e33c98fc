// Host harness of csrc/targets_dev.h, the per-thread text of targets.hip's kernels (overlap, equality / label, hard boxes, sampling select,
// loss term, gradient term), compiled with g++ under AddressSanitizer + UBSan and -ffp-contract=off. Every buffer is a heap block of exactly
// the size the launcher gives the kernel (the sanitizers guard the ends); the loops below walk the kernels' thread indices, whole workgroups,
// and stage boxes TG_CHUNK at a time as the kernels do. tests/test_anchor_targets.py builds this file, writes the cases, runs it as a
// subprocess and compares what it writes with tests/anchor_target_ref.py.
//
//   targets_host overlaps <in.bin> <out.bin>
//     in:  int32 n, k, intersections; float64 boxes[n][4], query[k][4]          out: float64 [n][k]
//   targets_host scene <in.bin> <out.bin>
//     in:  int32 hf, wf, G, D, has_hard, ld, image; uint64 seed; float32 im_info[3]; float64 cfg12[12]; float32 gt[G][5]; int32 hard[G] (if
//          has_hard); float32 dc[D][4]; float32 heads[hf * wf][ld]
//     out: with N = hf * wf * 10: float32 labels[N], presample[N], targets[N][4], inside[N][4], outside[N][4]; float64 max_overlap[N];
//          int32 argmax[N], stats[6]; then the loss of those arrays against heads: float64 losses[3]; int32 counts[2]; float32 d_heads[hf * wf][ld]
// exit status 2 on a bad file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../text-detection-ctpn_amd/csrc/targets_dev.h"

using namespace ctpn;

template <typename T>
static bool rd(std::FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
template <typename T>
static bool wr(std::FILE* f, const T* p, size_t n) { return n == 0 || std::fwrite(p, sizeof(T), n, f) == n; }
template <typename T>
static std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(new T[n]); }      // exact size; n = 0 is a valid empty block

static int run_overlaps(std::FILE* in, std::FILE* out) {
  int hdr[3];
  if (!rd(in, hdr, 3)) return 2;
  const int n = hdr[0], k = hdr[1], inter = hdr[2];
  if (n < 1 || k < 1 || n > 4096 || k > 4096) return 2;
  auto boxes = block<double>((size_t)n * 4), query = block<double>((size_t)k * 4), o = block<double>((size_t)n * k);
  if (!rd(in, boxes.get(), (size_t)n * 4) || !rd(in, query.get(), (size_t)k * 4)) return 2;
  const int wgs = (n + TG_ROWS - 1) / TG_ROWS;
  for (int wg = 0; wg < wgs; ++wg)
    for (int c0 = 0; c0 < k; c0 += TG_CHUNK) {
      const int cnt = k - c0 < TG_CHUNK ? k - c0 : TG_CHUNK;
      auto lds = block<double>((size_t)cnt * 5);
      for (int t = 0; t < cnt; ++t) {
        const double* q = query.get() + (size_t)(c0 + t) * 4;
        double* s = lds.get() + t * 5;
        s[0] = q[0]; s[1] = q[1]; s[2] = q[2]; s[3] = q[3];
        s[4] = tg_area(q[0], q[1], q[2], q[3]);
      }
      for (int t = 0; t < TG_THREADS; ++t) {
        if (t >= cnt) continue;
        const double* s = lds.get() + t * 5;
        for (int r = 0; r < TG_ROWS && wg * TG_ROWS + r < n; ++r) {
          const double* b = boxes.get() + (size_t)(wg * TG_ROWS + r) * 4;
          o[(size_t)(wg * TG_ROWS + r) * k + c0 + t] = tg_overlap(b[0], b[1], b[2], b[3], tg_area(b[0], b[1], b[2], b[3]), s[0], s[1], s[2], s[3], s[4], inter != 0);
        }
      }
    }
  return wr(out, o.get(), (size_t)n * k) ? 0 : 2;
}

// tg_subsample of targets.hip: the workgroup's select, thread by thread
static void subsample(float* lab, int A, float cls, long long have, long long keep, uint64_t seed, int img) {
  if (have <= keep) return;
  if (keep <= 0) { for (int i = 0; i < A; ++i) if (lab[i] == cls) lab[i] = -1.f; return; }
  uint64_t prefix = 0;
  unsigned need = (unsigned)keep;
  for (int pass = 7; pass >= 0; --pass) {
    auto hist = block<unsigned>(256);
    std::memset(hist.get(), 0, 256 * sizeof(unsigned));
    for (int t = 0; t < TG_WG; ++t)
      for (int i = t; i < A; i += TG_WG)
        if (lab[i] == cls) {
          const uint64_t key = tg_key(seed, img, i);
          if (tg_sel_match(key, prefix, pass)) hist[tg_sel_bin(key, pass)] += 1;
        }
    const int b = tg_sel_pick(hist.get(), need);
    prefix |= (uint64_t)b << (8 * pass);
  }
  for (int i = 0; i < A; ++i) if (lab[i] == cls && tg_key(seed, img, i) > prefix) lab[i] = -1.f;
}

static int run_scene(std::FILE* in, std::FILE* out) {
  int hdr[7];
  uint64_t seed = 0;
  float im[3];
  double c[12];
  if (!rd(in, hdr, 7) || !rd(in, &seed, 1) || !rd(in, im, 3) || !rd(in, c, 12)) return 2;
  const int hf = hdr[0], wf = hdr[1], G = hdr[2], D = hdr[3], has_hard = hdr[4], ld = hdr[5], img = hdr[6];
  if (hf < 1 || wf < 1 || (long long)hf * wf > 4096 || G < 0 || G > 4096 || D < 0 || D > 64 || (ld != 60 && ld != 64) || img < 0) return 2;
  const int A = hf * wf * TG_A;
  TgCfg cfg;
  cfg.neg = c[0]; cfg.pos = c[1]; cfg.clobber = c[2] != 0.0; cfg.fg_fraction = c[3]; cfg.batch = (long long)c[4]; cfg.dc_hi = c[5];
  cfg.preclude_hard = c[6] != 0.0;
  for (int i = 0; i < 4; ++i) cfg.inside_w[i] = (float)c[7 + i];
  auto gt = block<float>((size_t)G * 5);
  auto hard = block<int>(has_hard ? G : 0);
  auto dc = block<float>((size_t)D * 4);
  auto heads = block<float>((size_t)hf * wf * ld);
  if (!rd(in, gt.get(), (size_t)G * 5) || (has_hard && !rd(in, hard.get(), G)) || !rd(in, dc.get(), (size_t)D * 4) || !rd(in, heads.get(), (size_t)hf * wf * ld)) return 2;
  const int* use_hard = has_hard && cfg.preclude_hard ? hard.get() : nullptr;

  auto labels = block<float>(A), presample = block<float>(A), targets = block<float>((size_t)A * 4), inside_w = block<float>((size_t)A * 4),
       outside_w = block<float>((size_t)A * 4);
  auto best = block<double>(A);
  auto arg = block<int>(A), hardfirst = block<int>(G > 0 ? G : 1);
  auto colmax = block<double>(G > 0 ? G : 1);
  auto flags = block<uint8_t>(A);
  for (int g = 0; g < (G > 0 ? G : 1); ++g) { colmax[g] = 0.0; hardfirst[g] = TG_NO_ANCHOR; }
  const int wgs = (A + TG_THREADS - 1) / TG_THREADS;

  // tg_scan_kernel, then tg_mark_kernel
  for (int pass = 0; pass < 2; ++pass)
    for (int wg = 0; wg < wgs; ++wg) {
      std::vector<double> r_best(TG_THREADS, -1.0), r_hmax(TG_THREADS, -1.0);
      std::vector<int> r_arg(TG_THREADS, -1);
      std::vector<char> r_gtmax(TG_THREADS, 0);
      for (int c0 = 0; c0 < G; c0 += TG_CHUNK) {
        const int cnt = G - c0 < TG_CHUNK ? G - c0 : TG_CHUNK;
        auto lds = block<double>((size_t)cnt * TG_BOX);
        for (int j = 0; j < cnt; ++j) tg_stage_box(gt.get() + (size_t)(c0 + j) * 5, pass ? colmax[c0 + j] : 0.0, pass && use_hard ? use_hard[c0 + j] == 1 : 0, lds.get() + j * TG_BOX);
        for (int t = 0; t < TG_THREADS; ++t) {
          const long long idx = (long long)wg * TG_THREADS + t;
          if (idx >= A) continue;
          double x1, y1, x2, y2;
          tg_anchor(wf, idx, x1, y1, x2, y2);
          if (!tg_inside(x1, y1, x2, y2, im[0], im[1])) continue;
          const double aarea = tg_area(x1, y1, x2, y2);
          if (pass == 0) {
            tg_scan_chunk(x1, y1, x2, y2, aarea, lds.get(), cnt, c0, r_best[t], r_arg[t], [&](int g, double ov) { if (ov > colmax[g]) colmax[g] = ov; });
          } else {
            bool gm = r_gtmax[t] != 0;
            tg_mark_chunk(x1, y1, x2, y2, aarea, lds.get(), cnt, c0, gm, r_hmax[t], [&](int g) { if ((int)idx < hardfirst[g]) hardfirst[g] = (int)idx; });
            r_gtmax[t] = gm;
          }
        }
      }
      for (int t = 0; t < TG_THREADS; ++t) {
        const long long idx = (long long)wg * TG_THREADS + t;
        if (idx >= A) continue;
        double x1, y1, x2, y2;
        tg_anchor(wf, idx, x1, y1, x2, y2);
        const bool ins = tg_inside(x1, y1, x2, y2, im[0], im[1]);
        if (pass == 0) {
          const bool have = ins && G > 0;
          best[idx] = have ? r_best[t] : 0.0;
          arg[idx] = have ? r_arg[t] : -1;
          continue;
        }
        float t4[4] = {0.f, 0.f, 0.f, 0.f};
        float lab = -1.f;
        bool disabled = false;
        if (ins) {
          const double aarea = tg_area(x1, y1, x2, y2);
          const double dcsum = D > 0 ? tg_dontcare_sum(x1, y1, x2, y2, aarea, dc.get(), D) : 0.0;
          lab = (float)tg_label(cfg, G, best[idx], r_gtmax[t] != 0, D > 0, dcsum, r_hmax[t] >= 0.0, r_hmax[t], disabled);
          if (G > 0) tg_targets(x1, y1, x2, y2, gt.get() + (size_t)arg[idx] * 5, t4);
        }
        labels[idx] = lab;
        flags[idx] = disabled ? 1 : 0;
        std::memcpy(targets.get() + (size_t)idx * 4, t4, sizeof(t4));
      }
    }
  // tg_hard_kernel
  if (use_hard)
    for (int g = 0; g < G; ++g) {
      if (use_hard[g] != 1) continue;
      const int i = hardfirst[g];
      if (i < 0 || i >= A) continue;
      labels[i] = -1.f;
      flags[i] = 1;
    }
  // tg_sample_kernel
  int stats[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < A; ++i) {
    double x1, y1, x2, y2;
    tg_anchor(wf, i, x1, y1, x2, y2);
    stats[0] += tg_inside(x1, y1, x2, y2, im[0], im[1]) ? 1 : 0;
    stats[1] += labels[i] == 1.f;
    stats[2] += labels[i] == 0.f;
    stats[5] += flags[i] ? 1 : 0;
    presample[i] = labels[i];
  }
  if (cfg.batch > 0) {
    const long long num_fg = (long long)(cfg.fg_fraction * (double)cfg.batch);
    subsample(labels.get(), A, 1.f, stats[1], num_fg, seed, img);
    const long long fg_after = stats[1] < num_fg ? stats[1] : num_fg;
    subsample(labels.get(), A, 0.f, stats[2], cfg.batch - fg_after, seed, img);
  }
  for (int i = 0; i < A; ++i) {
    const bool f = labels[i] == 1.f;
    stats[3] += f;
    stats[4] += labels[i] == 0.f;
    for (int k = 0; k < 4; ++k) { inside_w[(size_t)i * 4 + k] = f ? cfg.inside_w[k] : 0.f; outside_w[(size_t)i * 4 + k] = f ? 1.f : 0.f; }
  }
  // tg_loss_kernel: TG_WG partial sums in ascending order of the anchor, a fixed tree
  auto r_ce = block<double>(TG_WG), r_box = block<double>(TG_WG);
  auto r_kept = block<int>(TG_WG), r_fg = block<int>(TG_WG);
  for (int t = 0; t < TG_WG; ++t) {
    double ce = 0.0, box = 0.0;
    int kept = 0, fg = 0;
    for (int i = t; i < A; i += TG_WG) {
      if (labels[i] == -1.f) continue;
      const int a = i % TG_A;
      const float* h = heads.get() + (size_t)(i / TG_A) * ld;
      const int label = labels[i] == 1.f ? 1 : 0;
      ce = ce + tg_ce_term(h[40 + 2 * a], h[40 + 2 * a + 1], label);
      double b4 = 0.0;
      for (int k = 0; k < 4; ++k) b4 = b4 + tg_box_term(h[4 * a + k], targets[(size_t)i * 4 + k], inside_w[(size_t)i * 4 + k], outside_w[(size_t)i * 4 + k]);
      box = box + b4;
      kept += 1;
      fg += label;
    }
    r_ce[t] = ce; r_box[t] = box; r_kept[t] = kept; r_fg[t] = fg;
  }
  for (int s = TG_WG / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) { r_ce[t] = r_ce[t] + r_ce[t + s]; r_box[t] = r_box[t] + r_box[t + s]; r_kept[t] += r_kept[t + s]; r_fg[t] += r_fg[t + s]; }
  const int K = r_kept[0], F = r_fg[0];
  double losses[3];
  losses[0] = K > 0 ? r_ce[0] / (double)K : 0.0;
  losses[1] = r_box[0] / ((double)F + 1.0);
  losses[2] = losses[0] + losses[1];
  const int counts[2] = {K, F};
  auto d_heads = block<float>((size_t)hf * wf * ld);
  for (int i = 0; i < A; ++i) {
    const int a = i % TG_A;
    const float* h = heads.get() + (size_t)(i / TG_A) * ld;
    float* d = d_heads.get() + (size_t)(i / TG_A) * ld;
    if (a == 0) for (int k = 60; k < ld; ++k) d[k] = 0.f;
    if (labels[i] == -1.f) {
      for (int k = 0; k < 4; ++k) d[4 * a + k] = 0.f;
      d[40 + 2 * a] = 0.f; d[40 + 2 * a + 1] = 0.f;
      continue;
    }
    for (int k = 0; k < 4; ++k)
      d[4 * a + k] = (float)(tg_box_grad(h[4 * a + k], targets[(size_t)i * 4 + k], inside_w[(size_t)i * 4 + k], outside_w[(size_t)i * 4 + k]) / ((double)F + 1.0));
    double dbg, dfg;
    tg_ce_grad(h[40 + 2 * a], h[40 + 2 * a + 1], labels[i] == 1.f ? 1 : 0, dbg, dfg);
    d[40 + 2 * a] = (float)(dbg / (double)K);
    d[40 + 2 * a + 1] = (float)(dfg / (double)K);
  }
  const bool ok = wr(out, labels.get(), A) && wr(out, presample.get(), A) && wr(out, targets.get(), (size_t)A * 4) && wr(out, inside_w.get(), (size_t)A * 4) &&
                  wr(out, outside_w.get(), (size_t)A * 4) && wr(out, best.get(), A) && wr(out, arg.get(), A) && wr(out, stats, 6) && wr(out, losses, 3) &&
                  wr(out, counts, 2) && wr(out, d_heads.get(), (size_t)hf * wf * ld);
  return ok ? 0 : 2;
}

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: targets_host overlaps|scene in.bin out.bin\n"); return 2; }
  std::FILE* in = std::fopen(argv[2], "rb");
  std::FILE* out = std::fopen(argv[3], "wb");
  if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
  const int rc = std::strcmp(argv[1], "overlaps") == 0 ? run_overlaps(in, out) : std::strcmp(argv[1], "scene") == 0 ? run_scene(in, out) : 2;
  std::fclose(in);
  if (std::fclose(out) != 0) return 2;
  return rc;
}
