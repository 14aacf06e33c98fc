// Host harness of the page path's two device texts: csrc/page_dev.h (the cut kernel's per-thread body) and csrc/nms_column_dev.h (the page NMS's
// per-column body), compiled with g++ under AddressSanitizer + UBSan. Every buffer is a heap block of exactly the size the launcher gives the
// kernel (the sanitizers guard the ends). tests/test_page_plan.py builds this file, writes the cases, runs it as a subprocess and compares
// what it writes with tests/page_ref.py and oracle/nms_ref.c.
//
//   page_host cut <in.bin> <out.bin>
//     in:  int32 page_h, page_w, n, tile_h, tile_w; int64 pitch; int32 tiles[n][8]; the page: (page_h - 1) * pitch + 3 * page_w bytes
//     out: n * tile_h * tile_w * 3 bytes -- written by a loop over the kernel's thread indices (a whole number of workgroups) into a block
//          that held 0xCD
//   page_host nms <in.bin> <out.bin>
//     in:  int32 n, kcap; float32 thresh; float32 boxes[n][4] in rank (descending score) order
//     out: int32 kept; int32 keep[kept], ascending rank
//     The ranks are partitioned by column int(x1) >> 4, ascending inside a column, and every column is run by nms_column_greedy the way
//     nms_page_columns_kernel runs it: 64 lanes side by side -- here 64 threads that meet at every ballot, lane read and chunk end --, kept boxes
//     in a block of kcap (the kernel's LDS), the rest in the column's own spill slice of exactly its candidates.
// exit status 2 on a bad file.
#include <pthread.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "../text-detection-ctpn_amd/csrc/page_dev.h"

// ---- what nms_column_dev.h asks of a compiler that is not hipcc: float4, and a wave's cross-lane operations ----
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }

static pthread_barrier_t g_meet;
static thread_local int t_lane = 0;
static int g_vote[64], g_slot[64];
static void wave_meet() { const int rc = pthread_barrier_wait(&g_meet); if (rc != 0 && rc != PTHREAD_BARRIER_SERIAL_THREAD) std::abort(); }
static unsigned long long wave_ballot(bool p) {
  g_vote[t_lane] = p ? 1 : 0;
  wave_meet();
  unsigned long long m = 0;
  for (int i = 0; i < 64; ++i) m |= (unsigned long long)g_vote[i] << i;
  wave_meet();
  return m;
}
static int wave_readlane(int v, int i) {
  g_slot[t_lane] = v;
  wave_meet();
  const int r = g_slot[i];
  wave_meet();
  return r;
}
#define NMS_BALLOT(p) wave_ballot(p)
#define NMS_READLANE(v, i) wave_readlane(v, i)
#define NMS_FIRSTLANE(v) (v)
#define NMS_CHUNK_END(spilled) wave_meet()
#include "../text-detection-ctpn_amd/csrc/nms_column_dev.h"

using namespace ctpn;

template <typename T>
static bool rd(std::FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

static int run_cut(std::FILE* in, std::FILE* out) {
  int hdr[5];
  long long pitch = 0;
  if (!rd(in, hdr, 5) || !rd(in, &pitch, 1)) return 2;
  const int page_h = hdr[0], page_w = hdr[1], n = hdr[2], tile_h = hdr[3], tile_w = hdr[4];
  if (page_h < 1 || page_w < 1 || n < 1 || n > 4096 || tile_h < 16 || tile_w < 16 || (tile_w & 15) || pitch < 3LL * page_w) return 2;
  std::unique_ptr<PgTile[]> tiles(new PgTile[n]);
  if (!rd(in, tiles.get(), n)) return 2;
  for (int t = 0; t < n; ++t) if (!pg_tile_ok(tiles[t], page_h, page_w, tile_h, tile_w)) return 2;      // (what ctpn_page_cut checks)
  const size_t pbytes = (size_t)(page_h - 1) * pitch + (size_t)page_w * 3;
  std::unique_ptr<uint8_t[]> page(new uint8_t[pbytes]);
  if (!rd(in, page.get(), pbytes)) return 2;
  const size_t obytes = (size_t)n * tile_h * tile_w * 3;
  std::unique_ptr<uint8_t[]> o(new uint8_t[obytes]);
  std::memset(o.get(), 0xCD, obytes);
  const long long wgs = (pg_cut_groups(n, tile_h, tile_w) + PG_THREADS - 1) / PG_THREADS;
  for (long long grp = 0; grp < wgs * PG_THREADS; ++grp) pg_cut_thread(page.get(), pitch, tiles.get(), n, tile_h, tile_w, o.get(), grp);
  return std::fwrite(o.get(), 1, obytes, out) == obytes ? 0 : 2;
}

struct Column { std::vector<int> ranks; std::unique_ptr<float4[]> kept, spill; std::unique_ptr<float[]> karea; };
struct Job { const float4* boxes; std::vector<Column>* cols; int kcap; float thr; std::vector<char>* alive; int lane; };

static void* lane_main(void* arg) {
  const Job& j = *static_cast<const Job*>(arg);
  t_lane = j.lane;
  for (Column& c : *j.cols) {
    const int* ranks = c.ranks.data();
    nms_column_greedy(j.boxes, [&](int ci) { return ranks[ci]; }, (int)c.ranks.size(), c.kept.get(), c.karea.get(), j.kcap, c.spill.get(), j.thr, j.lane,
                      [&](int rank) { (*j.alive)[rank] = 1; });
    wave_meet();
  }
  return nullptr;
}

static int run_nms(std::FILE* in, std::FILE* out) {
  int hdr[2];
  float thr = 0.f;
  if (!rd(in, hdr, 2) || !rd(in, &thr, 1)) return 2;
  const int n = hdr[0], kcap = hdr[1];
  if (n < 0 || n > (1 << 20) || kcap < 1 || kcap > 4096) return 2;
  std::unique_ptr<float4[]> boxes(new float4[n > 0 ? n : 1]);
  if (!rd(in, boxes.get(), n)) return 2;
  std::map<int, std::vector<int>> by_col;
  for (int r = 0; r < n; ++r) by_col[(int)boxes[r].x >> 4].push_back(r);
  std::vector<Column> cols;
  for (auto& kv : by_col) {
    Column c;
    c.ranks = kv.second;
    c.kept.reset(new float4[kcap]);
    c.karea.reset(new float[kcap]);
    c.spill.reset(new float4[c.ranks.size()]);
    cols.push_back(std::move(c));
  }
  std::vector<char> alive(n > 0 ? n : 1, 0);
  if (pthread_barrier_init(&g_meet, nullptr, 64) != 0) return 2;
  std::vector<Job> jobs(64, Job{boxes.get(), &cols, kcap, thr, &alive, 0});
  std::vector<pthread_t> th(64);
  for (int l = 0; l < 64; ++l) { jobs[l].lane = l; if (pthread_create(&th[l], nullptr, lane_main, &jobs[l]) != 0) return 2; }
  for (int l = 0; l < 64; ++l) pthread_join(th[l], nullptr);
  pthread_barrier_destroy(&g_meet);
  std::vector<int> keep;
  for (int r = 0; r < n; ++r) if (alive[r]) keep.push_back(r);
  const int nk = (int)keep.size();
  if (std::fwrite(&nk, 4, 1, out) != 1 || (nk && std::fwrite(keep.data(), 4, nk, out) != (size_t)nk)) return 2;
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: page_host cut|nms in.bin out.bin\n"); return 2; }
  std::FILE* in = std::fopen(argv[2], "rb");
  std::FILE* out = std::fopen(argv[3], "wb");
  if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
  const int rc = std::strcmp(argv[1], "cut") == 0 ? run_cut(in, out) : std::strcmp(argv[1], "nms") == 0 ? run_nms(in, out) : 2;
  std::fclose(in);
  if (std::fclose(out) != 0) return 2;
  return rc;
}
