// C ABI of libctpn_hip.so, solver unit: one optimiser step over a flat fp32 vector (solver.hip). Stateless, with the gradient units'
// conventions: no ctx is read or written; the call runs on a stream of its own, which waits for no other stream; its device blocks are
// allocated by the call and released before it returns; the caller's current device is put back. It synchronises twice: after pass 1, whose
// block partials the host adds left to right (the norm decides the clip and whether the step is taken at all), and at its end.
// The definitions: include/ctpn_hip.h, "the solver step".
#include "ctx.h"
#include "solver_dev.h"

#include <cmath>

namespace {
using namespace ctpn;

constexpr long long kMaxCount = 1LL << 40;

struct DeviceGuard {
  int prev = -1;
  int enter(int device_id) {
    CTPN_HIP_TRY(hipGetDevice(&prev));
    CTPN_HIP_TRY(hipSetDevice(device_id));
    return CTPN_OK;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// a vector updated in place: the caller's device pointer, or a device block of this call filled from and copied back to the caller's host array
struct Vec {
  DevBuf buf;
  float* dev = nullptr;
  float* host = nullptr;
  size_t bytes = 0;
  int in(const float* p, size_t floats, int on_device, hipStream_t s) {
    bytes = floats * sizeof(float);
    if (!p) return CTPN_OK;
    if (on_device) { dev = const_cast<float*>(p); return CTPN_OK; }
    if (const int rc = buf.alloc(bytes)) return rc;
    dev = buf.as<float>();
    host = const_cast<float*>(p);
    CTPN_HIP_TRY(hipMemcpyAsync(dev, p, bytes, hipMemcpyHostToDevice, s));
    return CTPN_OK;
  }
  int back(hipStream_t s) {
    if (host) CTPN_HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
    return CTPN_OK;
  }
};

bool solver_ok(int solver) { return solver == SV_MOMENTUM || solver == SV_ADAM || solver == SV_RMS; }

}  // namespace

extern "C" {

int ctpn_solver_plan(long long count, long long* block_floats, int* blocks) {
  if (count < 1 || count > kMaxCount) return fail(CTPN_ERR_ARG, "ctpn_solver_plan: count is 1 .. 2^40");
  if (!block_floats || !blocks) return fail(CTPN_ERR_ARG, "ctpn_solver_plan: null pointer");
  sv_plan(count, *block_floats, *blocks);
  return CTPN_OK;
}

int ctpn_solver_defaults(int solver, double* hyper8) {
  if (!solver_ok(solver)) return fail(CTPN_ERR_ARG, "ctpn_solver_defaults: solver is CTPN_SOLVER_MOMENTUM, _ADAM or _RMS");
  if (!hyper8) return fail(CTPN_ERR_ARG, "ctpn_solver_defaults: null pointer");
  sv_defaults(solver, hyper8);
  return CTPN_OK;
}

int ctpn_solver_step(int device_id, int solver, long long count, float* w, const float* g, float* s1, float* s2, const long long* seg_end,
                     const float* seg_decay, int n_seg, const double* hyper8, long long t, int on_device, double* out2) {
  const char* who = "ctpn_solver_step";
  if (!solver_ok(solver)) return fail(CTPN_ERR_ARG, std::string(who) + ": solver is CTPN_SOLVER_MOMENTUM, _ADAM or _RMS");
  if (count < 1 || count > kMaxCount) return fail(CTPN_ERR_ARG, std::string(who) + ": count is 1 .. 2^40");
  if (!w || !g || !s1 || (!s2 && solver != SV_MOMENTUM) || !seg_end || !seg_decay || !hyper8 || !out2)
    return fail(CTPN_ERR_ARG, std::string(who) + ": null pointer (s2 may be NULL for Momentum)");
  if (n_seg < 1 || n_seg > SV_MAX_SEGMENTS) return fail(CTPN_ERR_ARG, std::string(who) + ": 1 .. 64 segments");
  if (on_device != 0 && on_device != 1) return fail(CTPN_ERR_ARG, std::string(who) + ": on_device is 0 or 1");
  if (t < 1) return fail(CTPN_ERR_ARG, std::string(who) + ": t is the 1-based step");
  if ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2)) & 3)
    return fail(CTPN_ERR_ARG, std::string(who) + ": pointers are 4-byte aligned");
  SvSegments segs{};
  segs.n = n_seg;
  long long prev = 0;
  for (int i = 0; i < n_seg; ++i) {
    if (seg_end[i] <= prev || !std::isfinite(seg_decay[i])) return fail(CTPN_ERR_ARG, std::string(who) + ": seg_end is ascending from above 0, seg_decay finite");
    segs.end[i] = prev = seg_end[i];
    segs.decay[i] = seg_decay[i];
  }
  if (prev != count) return fail(CTPN_ERR_ARG, std::string(who) + ": the last seg_end equals count");
  for (int i = 0; i < 8; ++i) if (!std::isfinite(hyper8[i])) return fail(CTPN_ERR_ARG, std::string(who) + ": hyper8 is finite");
  if (!(hyper8[SV_CLIP] > 0.0)) return fail(CTPN_ERR_ARG, std::string(who) + ": the clip norm is positive");
  const int ndev = ctpn_device_count();
  if (ndev <= 0) return fail(CTPN_ERR_NODEVICE, std::string(who) + ": no HIP device visible (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev || device_id >= 16) return fail(CTPN_ERR_ARG, std::string(who) + ": device_id out of range");
  DeviceGuard guard;
  int rc = guard.enter(device_id);
  if (rc) return rc;
  long long block;
  int blocks;
  sv_plan(count, block, blocks);
  Stream st;
  Vec v_w, v_g, v_s1, v_s2;      // released before the stream, on every way out
  DevBuf parts;
  if ((rc = st.ensure())) return rc;
  const size_t cz = (size_t)count;
  if ((rc = v_w.in(w, cz, on_device, st)) || (rc = v_g.in(g, cz, on_device, st)) || (rc = v_s1.in(s1, cz, on_device, st)) ||
      (rc = v_s2.in(solver == SV_MOMENTUM ? nullptr : s2, cz, on_device, st)) || (rc = parts.alloc((size_t)blocks * 2 * sizeof(double))))
    return rc;
  if ((rc = launch_solver_sums(v_w.dev, v_g.dev, count, segs, parts.as<double>(), st))) return rc;
  std::vector<double> hp((size_t)blocks * 2);
  CTPN_HIP_TRY(hipMemcpyAsync(hp.data(), parts.get(), hp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  double sq = 0.0, reg = 0.0;      // the single ordered pass over the block partials
  for (int b = 0; b < blocks; ++b) { sq = sq + hp[2 * (size_t)b]; reg = reg + hp[2 * (size_t)b + 1]; }
  out2[0] = sq;
  out2[1] = reg;
  if (!std::isfinite(sq)) return fail(CTPN_ERR_ARG, std::string(who) + ": the gradient's sum of squares is not finite; nothing was written");
  const SvParams p = sv_params(solver, hyper8, t, std::sqrt(sq));
  if ((rc = launch_solver_update(v_w.dev, v_g.dev, v_s1.dev, v_s2.dev, count, segs, p, st))) return rc;
  if ((rc = v_w.back(st)) || (rc = v_s1.back(st)) || (rc = v_s2.back(st))) return rc;
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

}  // extern "C"
