// Ownership of HIP resources on the host side of libctpn_hip.so: four move-only handle types over device blocks, page-locked host blocks,
// events and streams. The host units (api_*.hip, ctx.h) create and release such resources through these types only: a member or a local of
// one of them is released when it dies, on every way out, and a release has no other spelling. The handles also keep four process-wide
// counters of what is live (ctpn_debug_live_resources), which is how a test asks "was everything released" without a device.
// This header needs the HIP runtime's API header and two things of common.h (fail, the error codes), repeated below, and nothing else of
// the project: tests/owned_host.cpp compiles it alone, against fakes of the nine HIP functions it calls.
#pragma once
#include <atomic>
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#ifndef CTPN_OK      // include/ctpn_hip.h
#define CTPN_OK 0
#define CTPN_ERR_HIP -2
#endif

namespace ctpn {

int fail(int code, const std::string& s);      // common.h

// what the handles of this process hold right now: device bytes, page-locked bytes, events, streams. Relaxed: they are counts, they order nothing
enum { LIVE_DEV_BYTES = 0, LIVE_PINNED_BYTES = 1, LIVE_EVENTS = 2, LIVE_STREAMS = 3 };
inline std::atomic<long long> g_live[4] = {};
inline void live_add(int what, long long d) { g_live[what].fetch_add(d, std::memory_order_relaxed); }
inline long long live_read(int what) { return g_live[what].load(std::memory_order_relaxed); }

// CTPN_HIP_TRY's wording (common.h), for the calls made here
#define CTPN_OWNED_TRY(expr)                                                                             \
  do {                                                                                                   \
    const hipError_t err_ = (expr);                                                                      \
    if (err_ != hipSuccess) return ::ctpn::fail(CTPN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(err_)); \
  } while (0)

struct DevMem {
  static constexpr int kLive = LIVE_DEV_BYTES;
  static constexpr const char* kAcquire = "hipMalloc(&p, bytes)";
  static hipError_t acquire(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t release(void* p) { return hipFree(p); }
};
struct PinnedMem {
  static constexpr int kLive = LIVE_PINNED_BYTES;
  static constexpr const char* kAcquire = "hipHostMalloc(&p, bytes)";
  static hipError_t acquire(void** p, size_t bytes) { return hipHostMalloc(p, bytes); }
  static hipError_t release(void* p) { return hipHostFree(p); }
};

// A block of memory and its size. Empty is {null, 0}.
template <class Mem>
class Block {
 public:
  Block() = default;
  Block(Block&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  Block& operator=(Block&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
    return *this;
  }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  ~Block() { reset(); }

  // a block of exactly `bytes`, in place of whatever was held; a failure leaves {null, 0}
  int alloc(size_t bytes) {
    reset();
    const hipError_t e = Mem::acquire(&p_, bytes);
    if (e != hipSuccess) { p_ = nullptr; return fail(CTPN_ERR_HIP, std::string(Mem::kAcquire) + ": " + hipGetErrorString(e)); }
    bytes_ = bytes;
    live_add(Mem::kLive, (long long)bytes);
    return CTPN_OK;
  }
  // at least `need` bytes, the contents not kept: for a buffer nothing reads any more when it grows. The old block goes first (the two need
  // not fit side by side), so a failure leaves {null, 0}: never the old size next to a null pointer
  int grow(size_t need) { return need <= bytes_ ? CTPN_OK : alloc(need); }
  // at least `need` bytes where a pointer handed out earlier must stay valid: the new block first, then the old one moves into `retired`, which
  // its owner keeps for as long as such pointers may be used. A failure leaves the old block in place and `retired` as it was
  int grow_retiring(size_t need, std::vector<Block>& retired) {
    if (need <= bytes_) return CTPN_OK;
    Block next;
    if (const int rc = next.alloc(need)) return rc;
    if (p_) retired.push_back(std::move(*this));
    *this = std::move(next);
    return CTPN_OK;
  }
  void reset() {
    if (!p_) return;
    (void)Mem::release(p_);
    live_add(Mem::kLive, -(long long)bytes_);
    p_ = nullptr; bytes_ = 0;
  }
  template <class T = void> T* as() const { return static_cast<T*>(p_); }
  void* get() const { return p_; }
  size_t bytes() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};
using DevBuf = Block<DevMem>;          // hipMalloc / hipFree
using PinnedBuf = Block<PinnedMem>;    // hipHostMalloc / hipHostFree

// An event for ordering (hipEventDisableTiming), or, for the profiler's pairs, one that can be timed.
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; }
    return *this;
  }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { reset(); }

  int ensure() { return e_ ? CTPN_OK : create(hipEventDisableTiming); }      // created on first use
  int ensure_timed() { return e_ ? CTPN_OK : create(hipEventDefault); }
  void reset() {
    if (!e_) return;
    (void)hipEventDestroy(e_);
    live_add(LIVE_EVENTS, -1);
    e_ = nullptr;
  }
  operator hipEvent_t() const { return e_; }
  hipEvent_t get() const { return e_; }

 private:
  int create(unsigned flags) {
    CTPN_OWNED_TRY(hipEventCreateWithFlags(&e_, flags));
    live_add(LIVE_EVENTS, 1);
    return CTPN_OK;
  }
  hipEvent_t e_ = nullptr;
};

// A non-blocking stream. Whoever lets one die sees to it that nothing is queued on it any more.
class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept {
    if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; }
    return *this;
  }
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { reset(); }

  int ensure() {
    if (s_) return CTPN_OK;
    CTPN_OWNED_TRY(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
    live_add(LIVE_STREAMS, 1);
    return CTPN_OK;
  }
  void reset() {
    if (!s_) return;
    (void)hipStreamDestroy(s_);
    live_add(LIVE_STREAMS, -1);
    s_ = nullptr;
  }
  operator hipStream_t() const { return s_; }
  hipStream_t get() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

}  // namespace ctpn
