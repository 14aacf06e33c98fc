// Stand-alone host program for tests/test_owned.py: csrc/owned.h, and nothing else of the library, against fakes of the nine HIP functions it
// calls. The fakes keep their own count of what is live, refuse a release of something they did not hand out, and can fail the k-th acquisition.
// Every scenario checks the handles' counters against the fakes' own; built with ASan + UBSan, so a leak or a double release also stops it.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../text-detection-ctpn_amd/csrc/owned.h"

using namespace ctpn;

// ---- the fakes -------------------------------------------------------------------------------------------------
static std::map<void*, size_t> g_dev, g_pin;
static std::map<void*, int> g_ev, g_st;
static long long g_acquired = 0;      // acquisitions asked for so far
static long long g_fail_at = -1;      // the acquisition with this index fails
static int g_created_events = 0, g_released = 0;
static std::string g_last_error;

static bool refuse() { return g_acquired++ == g_fail_at; }
static void die(const char* what) { std::fprintf(stderr, "owned_host: %s\n", what); std::abort(); }

static hipError_t fake_alloc(std::map<void*, size_t>& m, void** p, size_t n) {
  if (refuse()) return hipErrorOutOfMemory;
  *p = std::malloc(n ? n : 1);
  m[*p] = n;
  return hipSuccess;
}
static hipError_t fake_free(std::map<void*, size_t>& m, void* p) {
  auto it = m.find(p);
  if (it == m.end()) die("release of a block that is not live");
  m.erase(it);
  std::free(p);
  ++g_released;
  return hipSuccess;
}
template <class H> static hipError_t fake_create(std::map<void*, int>& m, H* h, unsigned flags) {
  if (refuse()) return hipErrorOutOfMemory;
  void* p = std::malloc(1);
  m[p] = (int)flags;
  *h = (H)p;
  return hipSuccess;
}
static hipError_t fake_destroy(std::map<void*, int>& m, void* p) {
  auto it = m.find(p);
  if (it == m.end()) die("destroy of a handle that is not live");
  m.erase(it);
  std::free(p);
  ++g_released;
  return hipSuccess;
}

extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return fake_alloc(g_dev, p, n); }
hipError_t hipFree(void* p) { return fake_free(g_dev, p); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return fake_alloc(g_pin, p, n); }
hipError_t hipHostFree(void* p) { return fake_free(g_pin, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  const hipError_t r = fake_create(g_ev, e, flags);
  if (r == hipSuccess) ++g_created_events;
  return r;
}
hipError_t hipEventDestroy(hipEvent_t e) { return fake_destroy(g_ev, (void*)e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) { return fake_create(g_st, s, flags); }
hipError_t hipStreamDestroy(hipStream_t s) { return fake_destroy(g_st, (void*)s); }
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "some error"; }
}

namespace ctpn {
int fail(int code, const std::string& s) { g_last_error = s; return code; }
}

// ---- the checks ------------------------------------------------------------------------------------------------
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "owned_host: line %d: CHECK(%s) failed\n", __LINE__, #cond); std::exit(1); } } while (0)

static long long sum(const std::map<void*, size_t>& m) { long long t = 0; for (auto& kv : m) t += (long long)kv.second; return t; }
// the handles' counters say what the fakes say
static bool agree() {
  return live_read(LIVE_DEV_BYTES) == sum(g_dev) && live_read(LIVE_PINNED_BYTES) == sum(g_pin) && live_read(LIVE_EVENTS) == (long long)g_ev.size() &&
         live_read(LIVE_STREAMS) == (long long)g_st.size();
}
static bool nothing_live() { return agree() && g_dev.empty() && g_pin.empty() && g_ev.empty() && g_st.empty(); }
static void no_failures() { g_fail_at = -1; }
static void fail_next() { g_fail_at = g_acquired; }

template <class B> static void moves_block() {
  B a, b;
  CHECK(a.alloc(100) == CTPN_OK && b.alloc(50) == CTPN_OK && agree());
  void* pa = a.get();
  B c(std::move(a));                                   // construction: the source is empty, nothing released
  CHECK(!a && a.bytes() == 0 && c.get() == pa && c.bytes() == 100 && agree());
  int before = g_released;
  b = std::move(c);                                    // assignment: the target's old block released once, the source empty
  CHECK(g_released == before + 1 && !c && c.bytes() == 0 && b.get() == pa && b.bytes() == 100 && agree());
  before = g_released;
  b = std::move(b);                                    // onto itself: nothing happens
  CHECK(g_released == before && b.get() == pa && agree());
  b.reset(); b.reset();
  CHECK(!b && b.bytes() == 0 && nothing_live());
}
template <class H> static void moves_handle() {
  H a, b;
  CHECK(a.ensure() == CTPN_OK && b.ensure() == CTPN_OK && agree());
  auto ha = a.get();
  H c(std::move(a));
  CHECK(a.get() == nullptr && c.get() == ha && agree());
  int before = g_released;
  b = std::move(c);
  CHECK(g_released == before + 1 && c.get() == nullptr && b.get() == ha && agree());
  b.reset(); b.reset();
  CHECK(b.get() == nullptr && nothing_live());
}
static void scenario_moves() {
  no_failures();
  moves_block<DevBuf>(); moves_block<PinnedBuf>(); moves_handle<Event>(); moves_handle<Stream>();
  {
    std::vector<DevBuf> v;                              // a vector that reallocates moves its blocks, releases none
    for (int i = 0; i < 20; ++i) { DevBuf b; CHECK(b.alloc(10 + i) == CTPN_OK); v.push_back(std::move(b)); }
    CHECK(agree() && g_dev.size() == 20);
  }
  CHECK(nothing_live());
}

// the typed accessor is a view of the same pointer
template <class B> static bool typed_views_agree(const B& b) { return b.template as<char>() == (char*)b.get() && b.template as<int>() == (int*)b.get(); }
template <class B> static void grows() {
  B b;
  CHECK(b.grow(0) == CTPN_OK && !b && agree());        // nothing asked for, nothing held
  CHECK(b.grow(64) == CTPN_OK && b.bytes() == 64 && agree());
  void* p = b.get();
  long long acq = g_acquired;
  CHECK(b.grow(10) == CTPN_OK && b.get() == p && b.bytes() == 64 && g_acquired == acq);      // below the size
  CHECK(b.grow(64) == CTPN_OK && b.get() == p && b.bytes() == 64 && g_acquired == acq);      // at the size
  int before = g_released;
  CHECK(b.grow(65) == CTPN_OK && b.bytes() == 65 && g_acquired == acq + 1 && g_released == before + 1 && agree());      // above: one release, one acquisition
  CHECK(typed_views_agree(b));
}
static void scenario_grow() {
  no_failures();
  grows<DevBuf>(); grows<PinnedBuf>();
  CHECK(nothing_live());
}

template <class B> static void grow_fails() {
  B b;
  CHECK(b.alloc(32) == CTPN_OK);
  int before = g_released;
  fail_next();
  CHECK(b.grow(33) == CTPN_ERR_HIP);                   // the old block released, {null, 0} left: no old size next to a null pointer
  CHECK(!b && b.get() == nullptr && b.bytes() == 0 && g_released == before + 1 && nothing_live());
  CHECK(g_last_error.find("Malloc(&p, bytes): out of memory") != std::string::npos);
  no_failures();
  CHECK(b.grow(33) == CTPN_OK && b.bytes() == 33 && agree());      // and usable again
  fail_next();
  CHECK(b.alloc(8) == CTPN_ERR_HIP && !b && b.bytes() == 0 && nothing_live());
  no_failures();
}
static void scenario_grow_fail() {
  grow_fails<DevBuf>(); grow_fails<PinnedBuf>();
  CHECK(nothing_live());
}

static void scenario_grow_retiring_fail() {
  no_failures();
  std::vector<DevBuf> retired;
  DevBuf b;
  CHECK(b.grow_retiring(40, retired) == CTPN_OK && b.bytes() == 40 && retired.empty());      // first use: nothing to retire
  void* p = b.get();
  int before = g_released;
  fail_next();
  CHECK(b.grow_retiring(41, retired) == CTPN_ERR_HIP);
  CHECK(b.get() == p && b.bytes() == 40 && retired.empty() && g_released == before && agree());      // the old block in place, `retired` unchanged
  no_failures();
  CHECK(b.grow_retiring(40, retired) == CTPN_OK && b.get() == p && retired.empty());      // large enough: no-op
}

static void scenario_grow_retiring_ok() {
  no_failures();
  {
    std::vector<DevBuf> retired;
    DevBuf b;
    CHECK(b.alloc(16) == CTPN_OK);
    char* old = b.as<char>();
    for (int i = 0; i < 16; ++i) old[i] = (char)(i + 1);
    int before = g_released;
    CHECK(b.grow_retiring(1000, retired) == CTPN_OK);
    CHECK(b.bytes() == 1000 && b.get() != (void*)old && retired.size() == 1 && retired[0].get() == (void*)old && retired[0].bytes() == 16);
    CHECK(g_released == before && agree() && sum(g_dev) == 1016);      // both live
    CHECK(b.grow_retiring(2000, retired) == CTPN_OK && retired.size() == 2 && agree() && sum(g_dev) == 16 + 1000 + 2000);
    for (int i = 0; i < 16; ++i) CHECK(old[i] == (char)(i + 1));      // a pointer handed out earlier is valid (ASan would say otherwise) until the vector dies
  }
  CHECK(nothing_live());
}

// what a ctx is, in small: several handles of every kind, acquired one after the other, any of which may fail
struct Several {
  Stream s0, s1;
  DevBuf a, b;
  PinnedBuf h;
  Event e0, e1;
  std::vector<DevBuf> blocks, retired;
  Event ring[2];
  int build() {
    int rc;
    if ((rc = s0.ensure()) || (rc = a.alloc(100)) || (rc = h.alloc(64)) || (rc = e0.ensure()) || (rc = s1.ensure())) return rc;
    for (int i = 0; i < 3; ++i) { DevBuf x; if ((rc = x.alloc(10 + i))) return rc; blocks.push_back(std::move(x)); }
    if ((rc = b.grow(10)) || (rc = b.grow(20)) || (rc = b.grow_retiring(30, retired)) || (rc = h.grow(128)) || (rc = e1.ensure_timed())) return rc;
    for (Event& e : ring) if ((rc = e.ensure())) return rc;
    return CTPN_OK;
  }
};
static int scenario_kth_failure() {
  no_failures();
  long long total;
  { const long long a0 = g_acquired; Several s; CHECK(s.build() == CTPN_OK && agree()); total = g_acquired - a0; CHECK(s.retired.size() == 1); }
  CHECK(nothing_live() && total == 15);
  for (long long k = 0; k < total; ++k) {
    {
      Several s;
      g_fail_at = g_acquired + k;
      CHECK(s.build() == CTPN_ERR_HIP);
      CHECK(agree());                                    // half built: the counters still say what is live
      no_failures();
    }
    CHECK(nothing_live());                               // out of scope: nothing left, for every k
  }
  return (int)total;
}

// a page-locked block and its device twin grown together, the way the device Huffman decoder's staging pair is: each block is tested against the
// need on its own, so a call in which one grew and the twin could not leaves a pair that the NEXT call of the same size completes
static int grow_pair(PinnedBuf& host, DevBuf& dev, size_t need) {
  int rc;
  if (need > host.bytes() && (rc = host.grow(need + need / 4))) return rc;
  if (need > dev.bytes() && (rc = dev.grow(need + need / 4))) return rc;
  return CTPN_OK;
}
static void scenario_pair_retry() {
  no_failures();
  PinnedBuf host; DevBuf dev;
  CHECK(grow_pair(host, dev, 100) == CTPN_OK && host.bytes() == 125 && dev.bytes() == 125 && agree());
  g_fail_at = g_acquired + 1;                           // the twin's allocation fails
  CHECK(grow_pair(host, dev, 200) == CTPN_ERR_HIP && host.bytes() == 250 && !dev && dev.bytes() == 0 && agree());
  no_failures();
  long long acq = g_acquired;
  CHECK(grow_pair(host, dev, 200) == CTPN_OK && g_acquired == acq + 1);      // the same size again: only the twin is acquired
  CHECK(host.bytes() == 250 && dev && dev.bytes() == 250 && agree());
  acq = g_acquired;
  CHECK(grow_pair(host, dev, 250) == CTPN_OK && g_acquired == acq);          // large enough: nothing
  fail_next();                                          // the first of the pair fails: {null, 0}, the twin untouched, and the next call completes it too
  CHECK(grow_pair(host, dev, 300) == CTPN_ERR_HIP && !host && host.bytes() == 0 && dev.bytes() == 250 && agree());
  no_failures();
  CHECK(grow_pair(host, dev, 300) == CTPN_OK && host.bytes() == 375 && dev.bytes() == 375 && agree());
}

static void scenario_event_ensure() {
  no_failures();
  {
    Event e;
    const int c0 = g_created_events;
    CHECK(e.get() == nullptr && (hipEvent_t)e == nullptr);
    CHECK(e.ensure() == CTPN_OK && g_created_events == c0 + 1);
    hipEvent_t h = e;
    CHECK(h != nullptr && g_ev.at((void*)h) == (int)hipEventDisableTiming);
    CHECK(e.ensure() == CTPN_OK && e.ensure_timed() == CTPN_OK && g_created_events == c0 + 1 && e.get() == h && agree());      // twice: created once
    Event t;
    CHECK(t.ensure_timed() == CTPN_OK && g_ev.at((void*)t.get()) == (int)hipEventDefault && agree());      // the profiler's form can be timed
    fail_next();
    Event f;
    CHECK(f.ensure() == CTPN_ERR_HIP && f.get() == nullptr && agree());
    CHECK(g_last_error == "hipEventCreateWithFlags(&e_, flags): out of memory");
    no_failures();
    Stream s;
    CHECK(s.ensure() == CTPN_OK && s.ensure() == CTPN_OK && g_st.size() == 1 && g_st.at((void*)s.get()) == (int)hipStreamNonBlocking && agree());
  }
  CHECK(nothing_live());
}

int main() {
  CHECK(nothing_live());
  scenario_moves(); std::printf("ok moves\n");
  scenario_grow(); std::printf("ok grow\n");
  scenario_grow_fail(); std::printf("ok grow_fail\n");
  scenario_grow_retiring_fail(); std::printf("ok grow_retiring_fail\n");
  scenario_grow_retiring_ok(); std::printf("ok grow_retiring_ok\n");
  const int total = scenario_kth_failure(); std::printf("ok kth_failure %d\n", total);
  scenario_pair_retry(); std::printf("ok pair_retry\n");
  scenario_event_ensure(); std::printf("ok event_ensure\n");
  CHECK(nothing_live());
  for (int k = 0; k < 4; ++k) CHECK(live_read(k) == 0);
  std::printf("ok exit acquisitions %lld releases %d\n", g_acquired, g_released);
  return 0;
}
