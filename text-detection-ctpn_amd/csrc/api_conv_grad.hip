// C ABI of libctpn_hip.so, conv-gradient unit: the backward pass through one conv + bias + ReLU layer and through the 2x2 max-pool
// (conv_grad.hip). Stateless, with the tail-gradient unit's conventions: no ctx is read or written; each call runs on a stream of its own, which
// waits for no other stream, and synchronises once, at its end; its device blocks are allocated by the call and released before it returns; the
// caller's current device is put back. The definitions: include/ctpn_hip.h, "the conv stack: backward".
#include "ctx.h"
#include "conv_grad_dev.h"

namespace {
using namespace ctpn;

constexpr long long kMaxPixels = 1LL << 28;
constexpr int kMaxSide = 1 << 20;
constexpr int kMaxChannels = 2048;

int grad_device(int device_id, const char* who) {
  const int ndev = ctpn_device_count();
  if (ndev <= 0) return fail(CTPN_ERR_NODEVICE, std::string(who) + ": no HIP device visible (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev || device_id >= 16) return fail(CTPN_ERR_ARG, std::string(who) + ": device_id out of range");
  return CTPN_OK;
}

// the caller's current device, put back on every way out
struct DeviceGuard {
  int prev = -1;
  int enter(int device_id) {
    CTPN_HIP_TRY(hipGetDevice(&prev));
    CTPN_HIP_TRY(hipSetDevice(device_id));
    return CTPN_OK;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// a tensor-sized argument: the caller's device pointer, or a device block of this call filled from / copied back to the caller's host array
struct Arg {
  DevBuf buf;
  float* dev = nullptr;
  void* host = nullptr;
  size_t bytes = 0;
  int in(const float* p, size_t floats, int on_device, hipStream_t s) {
    bytes = floats * sizeof(float);
    if (on_device) { dev = const_cast<float*>(p); return CTPN_OK; }
    if (const int rc = buf.alloc(bytes)) return rc;
    dev = buf.as<float>();
    CTPN_HIP_TRY(hipMemcpyAsync(dev, p, bytes, hipMemcpyHostToDevice, s));
    return CTPN_OK;
  }
  int out(float* p, size_t floats, int on_device) {
    bytes = floats * sizeof(float);
    if (!p) return CTPN_OK;
    if (on_device) { dev = p; return CTPN_OK; }
    if (const int rc = buf.alloc(bytes)) return rc;
    dev = buf.as<float>();
    host = p;
    return CTPN_OK;
  }
  int fetch(hipStream_t s) {
    if (host) CTPN_HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
    return CTPN_OK;
  }
};

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_map(const char* who, int n, int h, int w, int on_device, long long& M) {
  if (n <= 0 || h <= 0 || w <= 0) return fail(CTPN_ERR_ARG, std::string(who) + ": n, h, w >= 1");
  if (n > kMaxSide || h > kMaxSide || w > kMaxSide) return fail(CTPN_ERR_ARG, std::string(who) + ": n x h x w beyond 2^28 pixels");
  M = (long long)n * h;
  if (M > kMaxPixels || (M *= w) > kMaxPixels) return fail(CTPN_ERR_ARG, std::string(who) + ": n x h x w beyond 2^28 pixels");
  if (on_device != 0 && on_device != 1) return fail(CTPN_ERR_ARG, std::string(who) + ": on_device is 0 or 1");
  return CTPN_OK;
}

int check_channels(const char* who, int ci, int co) {
  if (!((ci == 3 || (ci > 0 && ci % 32 == 0)) && co > 0 && co % 64 == 0 && ci <= kMaxChannels && co <= kMaxChannels))
    return fail(CTPN_ERR_ARG, std::string(who) + ": ci is 3 or a multiple of 32, co a multiple of 64, both at most 2048");
  return CTPN_OK;
}

}  // namespace

extern "C" {

int ctpn_conv3x3_backward_plan(int n, int h, int w, int ci, int co, long long* block_pixels, int* blocks) {
  long long M;
  int rc = check_map("ctpn_conv3x3_backward_plan", n, h, w, 0, M);
  if (rc || (rc = check_channels("ctpn_conv3x3_backward_plan", ci, co))) return rc;
  if (!block_pixels || !blocks) return fail(CTPN_ERR_ARG, "ctpn_conv3x3_backward_plan: null pointer");
  cg_plan(M, ci, co, *block_pixels, *blocks);
  return CTPN_OK;
}

int ctpn_conv3x3_backward(int device_id, int n, int h, int w, int ci, int co, const float* x, const float* w_hwio, const float* y, const float* d_y,
                          int on_device, float* d_w, float* d_b, float* d_x) {
  long long M;
  int rc = check_map("ctpn_conv3x3_backward", n, h, w, on_device, M);
  if (rc || (rc = check_channels("ctpn_conv3x3_backward", ci, co))) return rc;
  if (!x || !w_hwio || !y || !d_y || !d_w || !d_b) return fail(CTPN_ERR_ARG, "ctpn_conv3x3_backward: null pointer");
  if (ci == 3 && d_x) return fail(CTPN_ERR_ARG, "ctpn_conv3x3_backward: ci = 3 is conv1_1, whose input has no gradient: d_x is NULL");
  if (on_device && !(aligned16(x) && aligned16(w_hwio) && aligned16(y) && aligned16(d_y) && aligned16(d_w) && aligned16(d_b) && aligned16(d_x)))
    return fail(CTPN_ERR_ARG, "ctpn_conv3x3_backward: device pointers are 16-byte aligned");
  if ((rc = grad_device(device_id, "ctpn_conv3x3_backward"))) return rc;
  DeviceGuard guard;
  if ((rc = guard.enter(device_id))) return rc;
  const size_t Mz = (size_t)M, wn = (size_t)9 * ci * co;
  long long block;
  int P;
  cg_plan(M, ci, co, block, P);
  Stream st;
  Arg a_x, a_w, a_y, a_dy, a_dw, a_db, a_dx;      // released before the stream, on every way out
  DevBuf dz, parts, bparts;
  if ((rc = st.ensure())) return rc;
  if ((rc = a_x.in(x, Mz * ci, on_device, st)) || (rc = a_y.in(y, Mz * co, on_device, st)) || (rc = a_dy.in(d_y, Mz * co, on_device, st)) ||
      (rc = a_dw.out(d_w, wn, on_device)) || (rc = a_db.out(d_b, (size_t)co, on_device)) || (rc = a_dx.out(d_x, Mz * ci, on_device)))
    return rc;
  if (d_x && (rc = a_w.in(w_hwio, wn, on_device, st))) return rc;      // the weights enter the data gradient alone
  if ((rc = dz.alloc(Mz * co * 4)) || (rc = parts.alloc((size_t)P * wn * 4)) || (rc = bparts.alloc((size_t)P * co * 4))) return rc;
  if ((rc = launch_conv_grad_mask(a_dy.dev, a_y.dev, dz.as<float>(), M, co, st))) return rc;
  if ((rc = launch_conv_grad_dw(a_x.dev, dz.as<float>(), h, w, ci, co, M, parts.as<float>(), bparts.as<float>(), a_dw.dev, a_db.dev, st))) return rc;
  if (d_x && (rc = launch_conv_grad_dx(dz.as<float>(), a_w.dev, h, w, ci, co, M, a_dx.dev, st))) return rc;
  if ((rc = a_dw.fetch(st)) || (rc = a_db.fetch(st)) || (rc = a_dx.fetch(st))) return rc;
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

int ctpn_maxpool2x2_backward(int device_id, int n, int h, int w, int c, const float* y_full, const float* d_pool, int on_device, float* d_full) {
  long long M;
  int rc = check_map("ctpn_maxpool2x2_backward", n, h, w, on_device, M);
  if (rc) return rc;
  if (c <= 0 || c % 4 || c > kMaxChannels) return fail(CTPN_ERR_ARG, "ctpn_maxpool2x2_backward: c is a multiple of 4, at most 2048");
  const size_t pooled = (size_t)n * (h / 2) * (w / 2) * c;
  if (!y_full || !d_full || (!d_pool && pooled)) return fail(CTPN_ERR_ARG, "ctpn_maxpool2x2_backward: null pointer");
  if (on_device && !(aligned16(y_full) && aligned16(d_full) && (!pooled || aligned16(d_pool))))
    return fail(CTPN_ERR_ARG, "ctpn_maxpool2x2_backward: device pointers are 16-byte aligned");
  if ((rc = grad_device(device_id, "ctpn_maxpool2x2_backward"))) return rc;
  DeviceGuard guard;
  if ((rc = guard.enter(device_id))) return rc;
  Stream st;
  Arg a_y, a_dp, a_df;
  if ((rc = st.ensure())) return rc;
  if ((rc = a_y.in(y_full, (size_t)M * c, on_device, st)) || (rc = a_df.out(d_full, (size_t)M * c, on_device))) return rc;
  if (pooled && (rc = a_dp.in(d_pool, pooled, on_device, st))) return rc;
  // an empty pooled map is never read: any valid pointer stands in for it
  if ((rc = launch_pool_grad(a_y.dev, pooled ? a_dp.dev : a_y.dev, n, h, w, c, a_df.dev, st)) || (rc = a_df.fetch(st))) return rc;
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

}  // extern "C"
