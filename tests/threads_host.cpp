// Stand-alone host program of tests/test_threads_host.py: the library's two host-side thread teams under ThreadSanitizer, with no device and
// no HIP runtime -- csrc/png.cpp (PngPool, one process-wide decode team behind job_mu_, and the g_png_zlib_only switch) as a second
// translation unit, and csrc/ctx.h's HostPool (one per ctx). This file supplies what they take from api_ctx.hip: the thread-local error text.
//
//   threads_host DIR      DIR holds t<T>_<h>x<w>_<k>.png for T in 0..3, (h, w) in {(8, 12), (33, 17)}, k in 0..2; t2_33x17_1.png is corrupt
//
// Prints one "ok <case> ..." line per case and "sum <file> <fnv1a64 of the decoded BGR bytes>" per good file (the test holds them against
// Pillow's pixels); any mismatch prints "FAIL ..." and the exit code is 1. ThreadSanitizer writes its reports to stderr.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../text-detection-ctpn_amd/csrc/ctx.h"

namespace ctpn {
static thread_local std::string t_err;
void set_error(const std::string& s) { t_err = s; }
int fail(int code, const std::string& s) { t_err = s; return code; }
}  // namespace ctpn

static std::atomic<int> g_failed(0);
#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stdout, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::fprintf(stdout, __VA_ARGS__); std::fprintf(stdout, "\n"); g_failed.store(1); } } while (0)

static const int kSizes[2][2] = {{8, 12}, {33, 17}};
static const int kThreads = 4, kFiles = 3, kCorruptThread = 2, kCorruptSize = 1, kCorruptFile = 1;

struct List {
  int h = 0, w = 0;
  std::vector<std::string> paths;
  std::vector<const char*> ptrs;
  std::vector<uint8_t> want;      // the single-threaded call's output
  int want_rc = 0;
  std::string want_err;
  size_t per() const { return (size_t)h * w * 3; }
  bool good(int k, int t, int s) const { (void)k; return !(t == kCorruptThread && s == kCorruptSize) || k != kCorruptFile; }
};

static uint64_t fnv(const uint8_t* p, size_t n) {
  uint64_t x = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) { x ^= p[i]; x *= 1099511628211ull; }
  return x;
}

// one call of ctpn_decode_png_files over a list, held against the single-threaded result: the good files' bytes, the code, this thread's text
static void decode_and_check(const List& L, int t, int s, const char* who) {
  std::vector<uint8_t> out(L.per() * kFiles, 0xEE);
  ctpn::t_err.clear();
  const int rc = ctpn_decode_png_files(L.ptrs.data(), kFiles, L.h, L.w, out.data(), kFiles);
  CHECK(rc == L.want_rc, "%s thread %d size %d: code %d, alone %d", who, t, s, rc, L.want_rc);
  CHECK(ctpn::t_err == L.want_err, "%s thread %d size %d: text '%s', alone '%s'", who, t, s, ctpn::t_err.c_str(), L.want_err.c_str());
  for (int k = 0; k < kFiles; ++k)
    if (L.good(k, t, s))
      CHECK(std::memcmp(out.data() + L.per() * k, L.want.data() + L.per() * k, L.per()) == 0, "%s thread %d size %d file %d: bytes differ from the single-threaded call's", who, t, s, k);
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: threads_host DIR\n"); return 2; }
  const std::string dir = argv[1];
  List lists[kThreads][2];
  // ---- the single-threaded calls, first, on the main thread
  for (int t = 0; t < kThreads; ++t)
    for (int s = 0; s < 2; ++s) {
      List& L = lists[t][s];
      L.h = kSizes[s][0]; L.w = kSizes[s][1];
      for (int k = 0; k < kFiles; ++k) L.paths.push_back(dir + "/t" + std::to_string(t) + "_" + std::to_string(L.h) + "x" + std::to_string(L.w) + "_" + std::to_string(k) + ".png");
      for (auto& p : L.paths) L.ptrs.push_back(p.c_str());
      L.want.assign(L.per() * kFiles, 0xEE);
      ctpn::t_err.clear();
      L.want_rc = ctpn_decode_png_files(L.ptrs.data(), kFiles, L.h, L.w, L.want.data(), kFiles);
      L.want_err = ctpn::t_err;
      const bool corrupt = t == kCorruptThread && s == kCorruptSize;
      CHECK((L.want_rc != 0) == corrupt, "single-threaded, thread %d size %d: code %d (%s)", t, s, L.want_rc, L.want_err.c_str());
      if (corrupt) {
        CHECK(L.want_err.find(L.paths[kCorruptFile]) != std::string::npos && L.want_err.find("file " + std::to_string(kCorruptFile) + " ") != std::string::npos,
              "the error does not name the corrupt file: '%s'", L.want_err.c_str());
      } else {
        CHECK(L.want_err.empty(), "a good list left a text: '%s'", L.want_err.c_str());
      }
      for (int k = 0; k < kFiles; ++k)
        if (L.good(k, t, s)) std::printf("sum t%d_%dx%d_%d.png %016llx\n", t, L.h, L.w, k, (unsigned long long)fnv(L.want.data() + L.per() * k, L.per()));
    }
  std::printf("ok alone\n");

  // ---- four threads decode at once, each its own two lists, 20 times over
  {
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; ++t)
      th.emplace_back([&, t] {
        for (int it = 0; it < 20; ++it)
          for (int s = 0; s < 2; ++s) decode_and_check(lists[t][s], t, s, "together");
      });
    for (auto& x : th) x.join();
    std::printf("ok together %d\n", kThreads * 20 * 2);
  }

  // ---- two threads flip the inflate backend between their calls while a third decodes: both backends give the same bytes
  {
    std::atomic<bool> stop(false);
    std::atomic<int> flips(0);
    std::vector<std::thread> th;
    for (int f = 0; f < 2; ++f)
      th.emplace_back([&, f] {
        for (int it = 0; !stop.load(); ++it) {
          ctpn_debug_png_backend((it + f) & 1);
          flips.fetch_add(1);
          decode_and_check(lists[f][(it >> 1) & 1], f, (it >> 1) & 1, "flipping");
        }
      });
    th.emplace_back([&] {
      for (int it = 0; it < 40; ++it) decode_and_check(lists[3][it & 1], 3, it & 1, "under flips");
      stop.store(true);
    });
    for (auto& x : th) x.join();
    ctpn_debug_png_backend(0);
    CHECK(flips.load() >= 2, "no flip happened");
    std::printf("ok backend_flips %d\n", flips.load() > 0 ? 1 : 0);
  }

  // ---- two HostPools run jobs from two threads while a third pool is constructed and destroyed
  {
    ctpn::HostPool a(4, -1), b(3, -1);
    std::atomic<bool> stop(false);
    std::atomic<long long> made(0);
    auto drive = [&](ctpn::HostPool& p, int seed) {
      for (int it = 0; it < 200; ++it) {
        const int n = 1 + (it * 7 + seed) % 67;
        std::vector<int> cell((size_t)n, 0);
        p.run(n, [&](int i) { cell[(size_t)i] += i + seed; }, it % 5);
        for (int i = 0; i < n; ++i) CHECK(cell[(size_t)i] == i + seed, "HostPool job %d of %d ran %s", i, n, cell[(size_t)i] ? "twice" : "never");
      }
    };
    std::thread ta([&] { drive(a, 1); }), tb([&] { drive(b, 1000); });
    std::thread tc([&] {
      while (!stop.load()) {
        ctpn::HostPool c(3, -1);
        std::atomic<int> sum(0);
        c.run(16, [&](int i) { sum.fetch_add(i); });
        CHECK(sum.load() == 120, "a short-lived HostPool summed %d", sum.load());
        made.fetch_add(1);
      }
    });
    ta.join(); tb.join();
    stop.store(true);
    tc.join();
    CHECK(made.load() >= 1, "no short-lived pool was made");
    std::printf("ok host_pools %d\n", made.load() > 0 ? 1 : 0);
  }
  return g_failed.load();
}
