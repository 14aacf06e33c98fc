// C ABI of libctpn_hip.so, test hooks: ctpn_debug_* entry points that run one kernel on caller-supplied data, everything on the null stream.
// Not on the product path.
#include <algorithm>
#include "ctx.h"
#include "conv3x3_plan.h"

namespace {
// Guarded output buffers (the recurrent tail's, the first layer's and the conv walk's hooks): followed by DBG_GUARD_ROWS guard rows and filled
// with DBG_FILL bytes before the launch; dbg_map_bytes / dbg_fetch_map (below, with the first layer's hooks) size and check a bordered map
constexpr int DBG_GUARD_ROWS = 64;
constexpr int DBG_FILL = 0xC3;
size_t dbg_map_bytes(int n, int H, int W, size_t pix);
int dbg_fetch_map(const void* d_map, int n, int H, int W, size_t pix, std::vector<char>& host, const char* who);
}  // namespace

extern "C" {

// ---- diagnostics ---------------------------------------------------------------------------------------------
// One 3x3 conv (+bias+ReLU, optionally + 2x2 max-pool) on caller-supplied dense tensors: the unit-test hook for the
// conv kernels on shapes the VGG trunk never produces (odd sizes, tails, single rows). Not on the product path.
int ctpn_debug_cvt_bf16(int device_id, const float* in, uint16_t* out, int n, int use_hw_instruction) {
  if (!in || !out || n <= 0) return fail(CTPN_ERR_ARG, "ctpn_debug_cvt_bf16: bad argument");
  if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_cvt_bf16: no HIP device visible (no CPU fallback)");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  DevBuf d_in, d_out;
  int rc;
  if ((rc = d_in.alloc((size_t)n * 4)) || (rc = d_out.alloc((size_t)n * 2 + 4))) return rc;
  CTPN_HIP_TRY(hipMemcpy(d_in.get(), in, (size_t)n * 4, hipMemcpyHostToDevice));
  rc = launch_cvt_bf16(d_in.as<float>(), d_out.as<uint16_t>(), n, use_hw_instruction, nullptr);
  if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(CTPN_ERR_HIP, "ctpn_debug_cvt_bf16: kernel failed");
  if (!rc && hipMemcpy(out, d_out.get(), (size_t)n * 2, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(CTPN_ERR_HIP, "ctpn_debug_cvt_bf16: copy failed");
  return rc;
}

int ctpn_debug_lds_dma(int device_id, const uint8_t* src, size_t bytes, uint8_t* out_clobber, uint8_t* out_keep) {
  if (!src || !out_clobber || !out_keep || bytes == 0 || bytes % 1024 != 0 || bytes > ((size_t)1 << 30)) return fail(CTPN_ERR_ARG, "ctpn_debug_lds_dma: bytes must be a positive multiple of 1024 (<= 1 GiB)");
  if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_lds_dma: no HIP device visible (no CPU fallback)");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  DevBuf b_in, b_a, b_b;
  int rc;
  if ((rc = b_in.alloc(bytes)) || (rc = b_a.alloc(bytes)) || (rc = b_b.alloc(bytes))) return rc;
  char *d_in = b_in.as<char>(), *d_a = b_a.as<char>(), *d_b = b_b.as<char>();
  CTPN_HIP_TRY(hipMemcpy(d_in, src, bytes, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemset(d_a, 0xA5, bytes));
  CTPN_HIP_TRY(hipMemset(d_b, 0x5A, bytes));
  CTPN_HIP_TRY(hipDeviceSynchronize());
  if ((rc = launch_lds_dma_check(d_in, d_a, d_b, (int)(bytes / 1024), nullptr))) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(CTPN_ERR_HIP, "ctpn_debug_lds_dma: kernel failed");
  CTPN_HIP_TRY(hipMemcpy(out_clobber, d_a, bytes, hipMemcpyDeviceToHost));
  CTPN_HIP_TRY(hipMemcpy(out_keep, d_b, bytes, hipMemcpyDeviceToHost));
  return CTPN_OK;
}

}  // extern "C"
namespace {
// ctpn_debug_conv3x3 (guard = false: zeroed outputs, the interior fetched) and ctpn_debug_conv3x3_walk (guard = true: both output maps and
// DBG_GUARD_ROWS rows behind each hold DBG_FILL before the launch, and every border pixel and guard row must still hold it afterwards;
// cu_count: launch_conv3x3's)
int dbg_conv3x3_body(int device_id, const float* in_nhwc, const float* w_hwio, const float* bias, int n, int h, int w, int ci,
                     int co, int precision, int impl, int fuse_pool, float* out_full, float* out_pool, bool guard, int cu_count) {
  if (!in_nhwc || !w_hwio || !bias) return fail(CTPN_ERR_ARG, "null pointer");
  if (precision < CTPN_PREC_FP32 || precision > CTPN_PREC_SPLIT) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3: unknown precision");
  if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_conv3x3: no HIP device visible (no CPU fallback)");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  const DType t = prec_dtype(precision);
  const bool split = t == DType::SPLIT;
  if (impl != 0 && impl != 1 && impl != 3) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3: impl is 0 (im2col GEMM), 1 (the product kernels) or 3 (1 with the dup_hi layout)");
  if (split && impl == 0) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3: split precision exists in the tap-reuse kernels only (impl 1, 3)");
  if (impl == 3 && !split) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3: dup_hi (impl 3) is a split-precision layout");
  // impl 3: the full-resolution pixel is [hi | lo | hi] (what rpn_conv stores for the LSTM projection); the third plane must equal the first
  const int dup = impl == 3 ? 1 : 0;
  if (dup && (fuse_pool || !out_full)) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3: impl 3 stores the full-resolution map only");
  if (dup) impl = 1;
  const int es = split ? 2 : dtype_bytes(t);                 // bytes per stored scalar
  const int cin_p = split ? 2 * ci : ci, cout_p = split ? 2 * co : co;      // scalars per pixel: split precision stores [hi | lo] planes
  const int Hp = h + 2, Wp = w + 2, ho = h / 2, wo = w / 2;
  const size_t in_elems = ((size_t)n * Hp * Wp + act_slack_pixels(w)) * cin_p, out_elems = (size_t)n * Hp * Wp * (cout_p + (dup ? co : 0)), pool_elems = (size_t)n * (ho + 2) * (wo + 2) * cout_p;
  const int co_pad = (co + 127) / 128 * 128;
  std::vector<char> hin(in_elems * es, 0);
  for (int in = 0; in < n; ++in) for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) for (int c = 0; c < ci; ++c) {
    const float v = in_nhwc[(((size_t)in * h + y) * w + x) * ci + c];
    const size_t o = (((size_t)in * Hp + y + 1) * Wp + x + 1) * cin_p + c;
    if (t == DType::F32) std::memcpy(&hin[o * 4], &v, 4);
    else if (t == DType::F16) { const uint16_t b = host_f32_to_f16(v); std::memcpy(&hin[o * 2], &b, 2); }
    else {
      const uint16_t b = host_f32_to_bf16(v); std::memcpy(&hin[o * 2], &b, 2);
      if (split) { const uint16_t l = host_f32_to_bf16(v - host_bf16_to_f32(b)); std::memcpy(&hin[(o + ci) * 2], &l, 2); }
    }
  }
  hipStream_t s = nullptr;
  const size_t in_front = act_front_pixels(w) * cin_p * es;
  const size_t wt_bytes = (size_t)co_pad * 9 * ci * (split ? 6 : es);
  DevBuf b_in, b_out, b_pool, b_wt, b_w, b_b;
  int rc;
  const size_t pix_out = (size_t)(cout_p + (dup ? co : 0)) * es, pix_pool = (size_t)cout_p * es;
  const size_t out_bytes = guard ? dbg_map_bytes(n, h, w, pix_out) : out_elems * es, pool_bytes = guard ? dbg_map_bytes(n, ho, wo, pix_pool) : pool_elems * es + 256;
  const char* const who = guard ? "ctpn_debug_conv3x3_walk" : "ctpn_debug_conv3x3";
  if ((rc = b_in.alloc(in_front + in_elems * es)) || (rc = b_out.alloc(out_bytes)) || (rc = b_pool.alloc(pool_bytes)) || (rc = b_wt.alloc(wt_bytes)) ||
      (rc = b_w.alloc((size_t)9 * ci * co * 4)) || (rc = b_b.alloc((size_t)co_pad * 4))) return rc;
  CTPN_HIP_TRY(hipMemset(b_in.get(), 0, in_front));
  void *d_in = b_in.as<char>() + in_front, *d_out = b_out.get(), *d_pool = b_pool.get(), *d_wt = b_wt.get();
  float *d_w = b_w.as<float>(), *d_b = b_b.as<float>();
  CTPN_HIP_TRY(hipMemset(d_out, guard ? DBG_FILL : 0, out_bytes));
  CTPN_HIP_TRY(hipMemset(d_pool, guard ? DBG_FILL : 0, pool_bytes));
  CTPN_HIP_TRY(hipMemset(d_wt, 0, wt_bytes));
  CTPN_HIP_TRY(hipMemset(d_b, 0, (size_t)co_pad * 4));
  CTPN_HIP_TRY(hipMemcpy(d_in, hin.data(), in_elems * es, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemcpy(d_w, w_hwio, (size_t)9 * ci * co * 4, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemcpy(d_b, bias, (size_t)co * 4, hipMemcpyHostToDevice));
  rc = split ? launch_pack_transpose_split(d_w, co, d_wt, 9, ci, co, s) : launch_pack_transpose(d_w, co, d_wt, 9 * ci, t, 9 * ci, co, s);
  bool host_pool = false;
  if (!rc) {
    if (impl == 1) {
      rc = launch_conv3x3(d_in, d_wt, d_b, (out_full || !fuse_pool) ? d_out : nullptr, fuse_pool ? d_pool : nullptr, t, n, h, w, ci, co, 1, s, dup,
                          nullptr, nullptr, 3, cu_count);
    } else {
      // impl 0: the im2col GEMM (igemm.hip) as an independent reference of the same layer; its pool is taken on the host from the stored map
      IGemm g{};
      g.a = d_in; g.wt = d_wt; g.bias = d_b; g.out = d_out; g.M = (long long)n * h * w; g.Ci = ci; g.ntaps = 9; g.Co = co;
      g.H = h; g.W = w; g.out_bordered = 1; g.ldc = co; g.relu = 1;
      rc = launch_igemm(g, t, t, s);
      host_pool = fuse_pool != 0;
    }
  }
  if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(CTPN_ERR_HIP, "ctpn_debug_conv3x3: kernel failed");
  auto fetch = [&](void* dsrc, int H2, int W2, float* dst, int dup_plane) -> int {
    const int pitch = cout_p + (dup_plane ? co : 0);
    const size_t elems = (size_t)n * (H2 + 2) * (W2 + 2) * pitch;
    std::vector<char> tmp;
    if (guard) {
      if (const int frc = dbg_fetch_map(dsrc, n, H2, W2, (size_t)pitch * es, tmp, who)) return frc;
    } else {
      tmp.resize(elems * es);
      CTPN_HIP_TRY(hipMemcpy(tmp.data(), dsrc, elems * es, hipMemcpyDeviceToHost));
    }
    for (int in = 0; in < n; ++in) for (int y = 0; y < H2; ++y) for (int x = 0; x < W2; ++x) for (int c = 0; c < co; ++c) {
      const size_t o = (((size_t)in * (H2 + 2) + y + 1) * (W2 + 2) + x + 1) * pitch + c;
      float v;
      if (t == DType::F32) std::memcpy(&v, &tmp[o * 4], 4);
      else {
        uint16_t b; std::memcpy(&b, &tmp[o * 2], 2);
        if (t == DType::F16) v = host_f16_to_f32(b);
        else {
          v = host_bf16_to_f32(b);
          if (split) { uint16_t l; std::memcpy(&l, &tmp[(o + co) * 2], 2); v += host_bf16_to_f32(l); }
          if (dup_plane && std::memcmp(&tmp[(o + 2 * co) * 2], &b, 2) != 0) return fail(CTPN_ERR_STATE, std::string(who) + ": the dup_hi plane differs from the hi plane");
        }
      }
      dst[(((size_t)in * H2 + y) * W2 + x) * co + c] = v;
    }
    return CTPN_OK;
  };
  if (!rc && (out_full || host_pool)) {
    std::vector<float> full_tmp;
    float* fdst = out_full;
    if (!fdst) { full_tmp.resize((size_t)n * h * w * co); fdst = full_tmp.data(); }
    rc = fetch(d_out, h, w, fdst, dup);
    if (!rc && host_pool && out_pool)
      for (int in = 0; in < n; ++in) for (int y = 0; y < ho; ++y) for (int x = 0; x < wo; ++x) for (int c = 0; c < co; ++c) {
        auto at = [&](int yy, int xx) { return fdst[(((size_t)in * h + yy) * w + xx) * co + c]; };
        out_pool[(((size_t)in * ho + y) * wo + x) * co + c] = std::max(std::max(at(2 * y, 2 * x), at(2 * y, 2 * x + 1)), std::max(at(2 * y + 1, 2 * x), at(2 * y + 1, 2 * x + 1)));
      }
  }
  if (!rc && out_pool && fuse_pool && !host_pool) rc = fetch(d_pool, ho, wo, out_pool, 0);
  if (!rc && guard) {
    // a map the caller did not ask for (or the launch does not store) has borders and guard rows all the same
    std::vector<char> host;
    if (!out_full) rc = dbg_fetch_map(d_out, n, h, w, pix_out, host, who);
    if (!rc && !(out_pool && fuse_pool)) rc = dbg_fetch_map(d_pool, n, ho, wo, pix_pool, host, who);
  }
  return rc;
}
}  // namespace
extern "C" {

int ctpn_debug_conv3x3(int device_id, const float* in_nhwc, const float* w_hwio, const float* bias, int n, int h, int w, int ci,
                       int co, int precision, int impl, int fuse_pool, float* out_full, float* out_pool) {
  return dbg_conv3x3_body(device_id, in_nhwc, w_hwio, bias, n, h, w, ci, co, precision, impl, fuse_pool, out_full, out_pool, false, 0);
}

// ctpn_debug_conv3x3 through the product kernels (impl 1, 3) with the main launch's plan and tile walk laid out for cu_count CUs (1 .. the
// device's own; 0 = the device's), and with guarded outputs: a store into a border pixel of the full or the pooled map, or behind either, is
// CTPN_ERR_STATE naming the image and the bordered row.
int ctpn_debug_conv3x3_walk(int device_id, const float* in_nhwc, const float* w_hwio, const float* bias, int n, int h, int w, int ci,
                            int co, int precision, int impl, int fuse_pool, int cu_count, float* out_full, float* out_pool) {
  if (impl != 1 && impl != 3) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_walk: impl is 1 (the product kernels) or 3 (1 with the dup_hi layout)");
  if (cu_count < 0) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_walk: cu_count is 1 .. the device's CU count, or 0 for the device's");
  if (!out_full && !out_pool) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_walk: no output");
  if (n <= 0 || h <= 0 || w <= 0 || (long long)n * (h + 2) * (w + 2) > (1 << 22)) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_walk: n, h, w positive, at most 2^22 bordered pixels");
  return dbg_conv3x3_body(device_id, in_nhwc, w_hwio, bias, n, h, w, ci, co, precision, impl, fuse_pool, out_full, out_pool, true, cu_count);
}

// The plan of launch_conv3x3 (conv3x3_plan.h) for the widths w_first .. w_first + w_count - 1 of one layer: what ctpn_debug_conv3x3 and the
// forward would launch for that shape. Host arithmetic only; a device is asked for its CU count when cu_count is 0.
int ctpn_debug_conv3x3_plan(int precision, int n, int h, int w_first, int w_count, int ci, int co, int fuse_pool, int keep_full, int dup_hi,
                            int conv_p64, int split_edge, int cu_count, int* plans) {
  if (!plans || w_count <= 0) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_plan: no output");
  if (precision < CTPN_PREC_FP32 || precision > CTPN_PREC_SPLIT) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_plan: unknown precision");
  const DType t = prec_dtype(precision);
  if (n <= 0 || h <= 0 || w_first <= 0 || w_first > 0x7fffffff - w_count || ci <= 0 || ci % (t == DType::F32 ? 32 : 64) != 0 || co <= 0 || co % (t == DType::F32 ? 4 : 8) != 0)
    return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_plan: shape out of range (Ci a multiple of 32 / 64, Co of 4 / 8)");
  if (dup_hi && t != DType::SPLIT) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_plan: dup_hi is a split-precision layout");
  if (cu_count < 0) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_plan: cu_count is a CU count, or 0 for the current device's");
  if (cu_count == 0) {
    if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_conv3x3_plan: cu_count 0 asks the current device, and no HIP device is visible");
    int dev = 0, rc;
    if ((rc = current_device(dev)) || (rc = device_cu_count(dev, cu_count))) return rc;
  }
  for (int i = 0; i < w_count; ++i) {
    const C3Plan p = c3_plan(t, n, h, w_first + i, ci, co, fuse_pool != 0, keep_full != 0 || !fuse_pool, dup_hi, true, true, (conv_p64 ? 1 : 0) | (split_edge ? 2 : 0), cu_count);
    if (p.main_form == C3M_NONE) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_plan: no kernel for this shape (split precision: Co <= 64 or a multiple of 128)");
    int* o = plans + (size_t)i * CTPN_CONV_PLAN_INTS;
    o[0] = p.main_form; o[1] = p.strip; o[2] = p.strip_cols; o[3] = p.w_cover; o[4] = p.deep; o[5] = p.edge_ks;
  }
  return CTPN_OK;
}

const char* ctpn_debug_conv3x3_form_name(int kind, int id) { return kind == 0 ? c3_main_name(id) : (kind == 1 ? c3_strip_name(id) : nullptr); }

// ---- the recurrent tail's kernels alone ------------------------------------------------------------------------
// Every output buffer below is followed by DBG_GUARD_ROWS guard rows and filled with DBG_FILL bytes before the launch: a kernel that stores
// behind its last row, or into the pad columns of a row, changes a byte that the hook then finds changed (CTPN_ERR_STATE).
}  // extern "C"
namespace {
bool dbg_fill_intact(const char* p, size_t n) {
  for (size_t i = 0; i < n; ++i) if ((unsigned char)p[i] != DBG_FILL) return false;
  return true;
}
// one fp32 value as the 16-bit operand of mode t (split precision: the hi half)
inline uint16_t dbg_to16(DType t, float v) { return t == DType::F16 ? host_f32_to_f16(v) : host_f32_to_bf16(v); }
// a device block for the length of a hook: `bufs`, a local of the hook, owns it; *out is a view
int dbg_alloc(std::vector<DevBuf>& bufs, void** out, size_t bytes) {
  DevBuf b;
  if (const int rc = b.alloc(bytes)) return rc;
  *out = b.get();
  bufs.push_back(std::move(b));
  return CTPN_OK;
}
}  // namespace
extern "C" {

int ctpn_debug_live_resources(long long* out4) {
  if (!out4) return fail(CTPN_ERR_ARG, "ctpn_debug_live_resources: null pointer");
  for (int k = 0; k < 4; ++k) out4[k] = live_read(k);
  return CTPN_OK;
}

int ctpn_debug_forward_sets(ctpn_ctx* c, long long* out4) {
  if (!c || !out4) return fail(CTPN_ERR_ARG, "ctpn_debug_forward_sets: null pointer");
  out4[0] = c->set1_state == 1 ? 2 : 1;
  out4[1] = c->last == &c->fs[1] ? 1 : 0;
  out4[2] = (long long)c->set1_bytes;
  out4[3] = (c->slot[0].busy ? c->slot[0].set : 255) | (c->slot[1].busy ? c->slot[1].set : 255) << 8;
  return CTPN_OK;
}

int ctpn_debug_lstm_pre_plan(long long cells, int cu_count, int* plan_out) {
  if (!plan_out) return fail(CTPN_ERR_ARG, "ctpn_debug_lstm_pre_plan: no output");
  if (cells <= 0 || cells > 0x7fffffffLL) return fail(CTPN_ERR_ARG, "ctpn_debug_lstm_pre_plan: cells out of range (1 .. 2^31 - 1)");
  if (cu_count < 0) return fail(CTPN_ERR_ARG, "ctpn_debug_lstm_pre_plan: cu_count is a CU count, or 0 for the current device's");
  if (cu_count == 0) {
    if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_lstm_pre_plan: cu_count 0 asks the current device, and no HIP device is visible");
    int dev = 0, rc;
    if ((rc = current_device(dev)) || (rc = device_cu_count(dev, cu_count))) return rc;
  }
  const LstmPrePlan p = lstm_pre_plan(cells, cu_count);
  plan_out[0] = p.small ? 0 : 1; plan_out[1] = p.waves; plan_out[2] = (int)p.workgroups; plan_out[3] = p.idle_waves;
  return CTPN_OK;
}

int ctpn_debug_lstm_pre(int device_id, const float* x, const float* wx, const float* bias, int n, int hf, int wf, int precision, int cu_count, float* out) {
  if (!x || !wx || !bias || !out) return fail(CTPN_ERR_ARG, "ctpn_debug_lstm_pre: null pointer");
  if (precision < CTPN_PREC_FP32 || precision > CTPN_PREC_SPLIT) return fail(CTPN_ERR_ARG, "ctpn_debug_lstm_pre: unknown precision");
  if (n <= 0 || hf <= 0 || wf <= 0 || (long long)n * hf * wf > (1 << 24)) return fail(CTPN_ERR_ARG, "ctpn_debug_lstm_pre: n, hf, wf positive, at most 2^24 cells");
  if (cu_count < 0) return fail(CTPN_ERR_ARG, "ctpn_debug_lstm_pre: cu_count is a CU count, or 0 for the current device's");
  if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_lstm_pre: no HIP device visible (no CPU fallback)");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  const DType t = prec_dtype(precision);
  const bool split = t == DType::SPLIT, half = dtype_is_half(t);
  const long long M = (long long)n * hf * wf;
  const int Hp = hf + 2, Wp = wf + 2;
  const int es = t == DType::F32 ? 4 : 2, pix = split ? 1536 : 512;      // bytes per stored scalar, scalars per pixel (split precision: [hi | lo | hi])
  const int oes = half ? 2 : 4;                                           // lstm_pre is fp16 in the 16-bit modes, fp32 otherwise
  // the bordered map, operands rounded to the mode's type; the border is POISON (the product's is zero): an index that strays into it shows
  std::vector<char> hin((size_t)n * Hp * Wp * pix * es);
  auto put = [&](size_t pixel, int c, float v) {
    const size_t o = pixel * pix + c;
    if (t == DType::F32) { std::memcpy(&hin[o * 4], &v, 4); return; }
    const uint16_t b = dbg_to16(t, v);
    std::memcpy(&hin[o * 2], &b, 2);
    if (split) {
      const uint16_t l = host_f32_to_bf16(v - host_bf16_to_f32(b));
      std::memcpy(&hin[(o + 512) * 2], &l, 2);
      std::memcpy(&hin[(o + 1024) * 2], &b, 2);
    }
  };
  for (int in = 0; in < n; ++in) for (int y = 0; y < Hp; ++y) for (int xx = 0; xx < Wp; ++xx) {
    const size_t pixel = ((size_t)in * Hp + y) * Wp + xx;
    const bool inside = y >= 1 && y <= hf && xx >= 1 && xx <= wf;
    const float* src = inside ? x + (((size_t)in * hf + (y - 1)) * wf + (xx - 1)) * 512 : nullptr;
    for (int c = 0; c < 512; ++c) put(pixel, c, inside ? src[c] : 3e4f);
  }
  std::vector<DevBuf> bufs;
  void *d_a = nullptr, *d_wx = nullptr, *d_b = nullptr, *d_wt = nullptr, *d_wtf = nullptr, *d_bx = nullptr, *d_out = nullptr;
  const size_t row_bytes = split ? (size_t)3 * 512 * 2 : (size_t)512 * es;
  const size_t out_bytes = (size_t)M * 1024 * oes, guard_bytes = (size_t)DBG_GUARD_ROWS * 1024 * oes;
  int rc;
  if ((rc = dbg_alloc(bufs, &d_a, hin.size())) || (rc = dbg_alloc(bufs, &d_wx, (size_t)512 * 1024 * 4)) || (rc = dbg_alloc(bufs, &d_b, 1024 * 4)) ||
      (rc = dbg_alloc(bufs, &d_wt, 1024 * row_bytes)) || (half && (rc = dbg_alloc(bufs, &d_wtf, (size_t)1024 * 512 * 2))) || (rc = dbg_alloc(bufs, &d_bx, 1024 * 4)) ||
      (rc = dbg_alloc(bufs, &d_out, out_bytes + guard_bytes))) return rc;
  CTPN_HIP_TRY(hipMemcpy(d_a, hin.data(), hin.size(), hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemcpy(d_wx, wx, (size_t)512 * 1024 * 4, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemcpy(d_b, bias, 1024 * 4, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemset(d_out, DBG_FILL, out_bytes + guard_bytes));
  CTPN_HIP_TRY(hipDeviceSynchronize());
  // the product's weight chain (api_weights.hip) on wx [512][fw 512 | bw 512]: direction d's block starts at column 512 d, 1024 floats per row
  const float* const kx[2] = {(const float*)d_wx, (const float*)d_wx + 512};
  const float* const bx[2] = {(const float*)d_b, (const float*)d_b + 512};
  if ((rc = pack_lstm_projection(kx, 1024, bx, t, d_wt, row_bytes, (float*)d_bx, d_wtf, nullptr))) return rc;
  if (half) rc = launch_lstm_pre(d_a, d_wtf, (const float*)d_bx, d_out, t, n, hf, wf, nullptr, cu_count);
  else {      // the set-up of api_forward.hip
    IGemm g{};
    g.a = d_a; g.wt = d_wt; g.bias = (const float*)d_bx; g.out = d_out;
    g.M = M; g.Ci = split ? 1536 : 512; g.ntaps = 1; g.Co = 1024; g.a_plain = 0; g.H = hf; g.W = wf; g.tap_base_y = 1; g.tap_base_x = 1;
    g.out_bordered = 0; g.ldc = 1024; g.relu = 0;
    rc = launch_igemm(g, split ? DType::BF16 : t, DType::F32, nullptr);
  }
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(CTPN_ERR_HIP, "ctpn_debug_lstm_pre: kernel failed");
  std::vector<char> tmp(out_bytes + guard_bytes);
  CTPN_HIP_TRY(hipMemcpy(tmp.data(), d_out, tmp.size(), hipMemcpyDeviceToHost));
  if (!dbg_fill_intact(tmp.data() + out_bytes, guard_bytes)) return fail(CTPN_ERR_STATE, "ctpn_debug_lstm_pre: a guard row behind the last cell was written");
  for (long long m = 0; m < M; ++m)      // device layout: permuted gate columns -> TF's i | j | f | o order
    for (int ch = 0; ch < 1024; ++ch) {
      const size_t o = (size_t)m * 1024 + (ch & ~511) + lstm_gate_col(ch & 511);
      float v;
      if (half) { uint16_t b; std::memcpy(&b, &tmp[o * 2], 2); v = host_f16_to_f32(b); }
      else std::memcpy(&v, &tmp[o * 4], 4);
      out[(size_t)m * 1024 + ch] = v;
    }
  return CTPN_OK;
}

int ctpn_debug_bilstm(int device_id, const float* pre, const float* wh, int rows, int T, int split, int fast_gates, int pre_f16, float* out, int* form_out) {
  if (!pre || !wh || !out) return fail(CTPN_ERR_ARG, "ctpn_debug_bilstm: null pointer");
  if (rows <= 0 || T <= 0 || (long long)rows * T > (1 << 22)) return fail(CTPN_ERR_ARG, "ctpn_debug_bilstm: rows, T positive, at most 2^22 positions");
  split = split ? 1 : 0; fast_gates = fast_gates ? 1 : 0; pre_f16 = pre_f16 ? 1 : 0;
  if (!split && fast_gates != pre_f16)
    return fail(CTPN_ERR_ARG, "ctpn_debug_bilstm: the forward never launches exact gates on fp16 pre-activations or fast gates on fp32 ones (without split)");
  if (form_out) *form_out = bilstm_plan(rows, split, fast_gates).form;
  if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_bilstm: no HIP device visible (no CPU fallback)");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  const size_t pos = (size_t)rows * T;
  const int pes = pre_f16 ? 2 : 4;
  std::vector<char> hpre(pos * 1024 * pes);      // TF's i | j | f | o order -> the permuted order the kernels read, fp16 where asked
  for (size_t p = 0; p < pos; ++p)
    for (int ch = 0; ch < 1024; ++ch) {
      const float v = pre[p * 1024 + ch];
      const size_t o = p * 1024 + (ch & ~511) + lstm_gate_col(ch & 511);
      if (pre_f16) { const uint16_t b = host_f32_to_f16(v); std::memcpy(&hpre[o * 2], &b, 2); }
      else std::memcpy(&hpre[o * 4], &v, 4);
    }
  std::vector<DevBuf> bufs;
  void *d_pre = nullptr, *d_wh = nullptr, *d_out = nullptr;
  const size_t out_bytes = pos * 256 * 4, guard_bytes = (size_t)DBG_GUARD_ROWS * 256 * 4;
  int rc;
  if ((rc = dbg_alloc(bufs, &d_pre, hpre.size())) || (rc = dbg_alloc(bufs, &d_wh, (size_t)2 * 128 * 512 * 4)) || (rc = dbg_alloc(bufs, &d_out, out_bytes + guard_bytes))) return rc;
  CTPN_HIP_TRY(hipMemcpy(d_pre, hpre.data(), hpre.size(), hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemcpy(d_wh, wh, (size_t)2 * 128 * 512 * 4, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemset(d_out, DBG_FILL, out_bytes + guard_bytes));
  CTPN_HIP_TRY(hipDeviceSynchronize());
  if ((rc = launch_bilstm(d_pre, pre_f16, (const float*)d_wh, (float*)d_out, rows, T, nullptr, split, fast_gates))) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(CTPN_ERR_HIP, "ctpn_debug_bilstm: kernel failed");
  std::vector<char> guard(guard_bytes);
  CTPN_HIP_TRY(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
  CTPN_HIP_TRY(hipMemcpy(guard.data(), (const char*)d_out + out_bytes, guard_bytes, hipMemcpyDeviceToHost));
  if (!dbg_fill_intact(guard.data(), guard_bytes)) return fail(CTPN_ERR_STATE, "ctpn_debug_bilstm: a guard row behind the last position was written");
  return CTPN_OK;
}

int ctpn_debug_gemm(int device_id, const float* a, const float* w, const float* bias, int M, int K, int Co, int ldc, int in_precision, float* out) {
  if (!a || !w || !bias || !out) return fail(CTPN_ERR_ARG, "ctpn_debug_gemm: null pointer");
  if (in_precision < CTPN_PREC_FP32 || in_precision > CTPN_PREC_FP16) return fail(CTPN_ERR_ARG, "ctpn_debug_gemm: in_precision is fp32, bf16 or fp16");
  const DType t = prec_dtype(in_precision);
  const int es = dtype_bytes(t);
  if (M <= 0 || M > (1 << 22) || K <= 0 || K > 4096 || K % (128 / es) != 0 || Co <= 0 || Co > 4096 || Co % 4 != 0 || ldc < Co || ldc > 8192 || ldc % 4 != 0)
    return fail(CTPN_ERR_ARG, "ctpn_debug_gemm: M <= 2^22, K a multiple of the 128-byte strip, Co and ldc multiples of 4, Co <= ldc");
  if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_gemm: no HIP device visible (no CPU fallback)");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  std::vector<char> ha((size_t)M * K * es);      // operands rounded to the mode's type, as ctpn_debug_conv3x3 does
  for (size_t i = 0; i < (size_t)M * K; ++i) {
    if (t == DType::F32) std::memcpy(&ha[i * 4], &a[i], 4);
    else { const uint16_t b = dbg_to16(t, a[i]); std::memcpy(&ha[i * 2], &b, 2); }
  }
  // weight rows and bias padded to the N tile with zeros, as the ctx allocates them: the 64-wide tile of Co = 60 reads rows 60 .. 63
  const int co_pad = Co <= 64 ? 64 : (Co + 127) / 128 * 128;
  std::vector<DevBuf> bufs;
  void *d_a = nullptr, *d_w = nullptr, *d_wt = nullptr, *d_b = nullptr, *d_out = nullptr;
  const size_t out_bytes = (size_t)M * ldc * 4, guard_bytes = (size_t)DBG_GUARD_ROWS * ldc * 4;
  int rc;
  if ((rc = dbg_alloc(bufs, &d_a, ha.size())) || (rc = dbg_alloc(bufs, &d_w, (size_t)K * Co * 4)) || (rc = dbg_alloc(bufs, &d_wt, (size_t)co_pad * K * es)) ||
      (rc = dbg_alloc(bufs, &d_b, (size_t)co_pad * 4)) || (rc = dbg_alloc(bufs, &d_out, out_bytes + guard_bytes))) return rc;
  CTPN_HIP_TRY(hipMemcpy(d_a, ha.data(), ha.size(), hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemcpy(d_w, w, (size_t)K * Co * 4, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemset(d_wt, 0, (size_t)co_pad * K * es));
  CTPN_HIP_TRY(hipMemset(d_b, 0, (size_t)co_pad * 4));
  CTPN_HIP_TRY(hipMemcpy(d_b, bias, (size_t)Co * 4, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemset(d_out, DBG_FILL, out_bytes + guard_bytes));
  CTPN_HIP_TRY(hipDeviceSynchronize());
  if ((rc = launch_pack_transpose((const float*)d_w, Co, d_wt, K, t, K, Co, nullptr))) return rc;
  IGemm g{};
  g.a = d_a; g.wt = d_wt; g.bias = (const float*)d_b; g.out = d_out;
  g.M = M; g.Ci = K; g.ntaps = 1; g.Co = Co; g.a_plain = 1; g.lda = K; g.out_bordered = 0; g.ldc = ldc; g.relu = 0;
  if ((rc = launch_igemm(g, t, DType::F32, nullptr))) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(CTPN_ERR_HIP, "ctpn_debug_gemm: kernel failed");
  std::vector<char> guard(guard_bytes);
  CTPN_HIP_TRY(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));      // pad columns included: the caller sees the fill in them
  CTPN_HIP_TRY(hipMemcpy(guard.data(), (const char*)d_out + out_bytes, guard_bytes, hipMemcpyDeviceToHost));
  if (!dbg_fill_intact(guard.data(), guard_bytes)) return fail(CTPN_ERR_STATE, "ctpn_debug_gemm: a guard row behind the last row was written");
  for (int m = 0; m < M; ++m)
    if (ldc > Co && !dbg_fill_intact((const char*)(out + (size_t)m * ldc + Co), (size_t)(ldc - Co) * 4))
      return fail(CTPN_ERR_STATE, "ctpn_debug_gemm: a pad column (Co .. ldc - 1) was written");
  return CTPN_OK;
}

// ---- the proposal layer's kernels alone ------------------------------------------------------------------------
int ctpn_debug_proposal_plan(int nms_columns, int nms_prefix, int mw_scratch, int n, int hf_first, int hf_count, int wf_first, int wf_count,
                             int pre_nms_topn, int post_nms_topn, float nms_thresh, const float* im_widths, int* plans) {
  if (!plans || hf_count <= 0 || wf_count <= 0) return fail(CTPN_ERR_ARG, "ctpn_debug_proposal_plan: no output");
  if (n <= 0 || n > 4096 || hf_first <= 0 || wf_first <= 0 || hf_first > 8192 - hf_count || wf_first > 8192 - wf_count || pre_nms_topn <= 0 || post_nms_topn <= 0)
    return fail(CTPN_ERR_ARG, "ctpn_debug_proposal_plan: n 1 .. 4096, maps up to 8191 x 8191, positive top-N");
  if ((long long)(hf_first + hf_count - 1) * (wf_first + wf_count - 1) * 10 > (1 << 30)) return fail(CTPN_ERR_ARG, "ctpn_debug_proposal_plan: more than 2^30 anchors per image");
  std::vector<float> rows;
  if (im_widths) { rows.assign((size_t)n * 3, 0.f); for (int i = 0; i < n; ++i) rows[3 * i + 1] = im_widths[i]; }
  for (int a = 0; a < hf_count; ++a)
    for (int b = 0; b < wf_count; ++b) {
      const ProposalPlan p = proposal_plan(nms_columns, nms_prefix, mw_scratch != 0, n, hf_first + a, wf_first + b, pre_nms_topn, post_nms_topn, nms_thresh,
                                           im_widths ? rows.data() : nullptr);
      int* o = plans + ((size_t)a * wf_count + b) * CTPN_PROPOSAL_PLAN_INTS;
      o[0] = p.npad; o[1] = p.fill_keys; o[2] = p.sort_form; o[3] = p.seg_len; o[4] = p.last_seg; o[5] = p.merge_wgs; o[6] = p.nms_form; o[7] = p.group_wgs;
      o[8] = p.prefix_launches;
    }
  return CTPN_OK;
}

int ctpn_debug_text_line_plan(int nms_columns, int connect_device, int mw_scratch, int n, int wf, int rows, float nms_thresh, float max_scale, int* plan) {
  if (!plan) return fail(CTPN_ERR_ARG, "ctpn_debug_text_line_plan: no output");
  if (nms_columns < 0 || nms_columns > 3 || n <= 0 || wf <= 0 || rows <= 0 || rows > CTPN_POST_NMS_CAPACITY_MAX)
    return fail(CTPN_ERR_ARG, "ctpn_debug_text_line_plan: nms_columns 0 .. 3, n and wf positive, rows 1 .. 4096");
  const TextLinePlan p = text_line_plan(nms_columns, connect_device != 0, mw_scratch != 0, n, wf, rows, nms_thresh, max_scale);
  plan[0] = p.nms_form; plan[1] = p.conn_form; plan[2] = p.group_wgs;
  return CTPN_OK;
}

int ctpn_debug_proposal_fetch(ctpn_ctx* c, int what, void* out, size_t capacity_bytes) {
  if (!c || !out) return fail(CTPN_ERR_ARG, "ctpn_debug_proposal_fetch: null pointer");
  if (c->last_prop_n <= 0) return fail(CTPN_ERR_STATE, "ctpn_debug_proposal_fetch: no ctpn_proposals / ctpn_proposals_from_host call yet");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream));
  const ProposalPlan& p = c->last_plan;
  const size_t n = (size_t)c->last_prop_n, per_img = (size_t)c->last_hf * c->last_wf * 10, pre = (size_t)c->last_pre, post = (size_t)c->last_post;
  const void* src = nullptr;
  size_t row = 0, pitch = 0;      // bytes per image handed out, and between the images on the device
  switch (what) {
    case CTPN_PF_BOXES4: src = c->boxes4; row = pitch = per_img * 16; break;
    case CTPN_PF_SORTED_KEYS: src = p.sort_form == PP_SORT_SEGMENTED ? c->keys_tmp : c->keys; row = pitch = (size_t)p.npad * 8; break;
    case CTPN_PF_SORTED_BOXES: src = c->sorted_boxes; row = pitch = pre * 16; break;
    case CTPN_PF_SORTED_SCORES: src = c->sorted_scores; row = pitch = pre * 4; break;
    case CTPN_PF_SORTED_ANCHOR: src = c->sorted_anchor; row = pitch = pre * 4; break;
    case CTPN_PF_VALID_COUNTS: src = c->valid_counts; row = pitch = 4; break;
    case CTPN_PF_COLID:
      if (p.nms_form != PP_NMS_COLUMN_GROUPS) return fail(CTPN_ERR_STATE, "ctpn_debug_proposal_fetch: the last call wrote no column ids (not the multi-workgroup NMS)");
      src = c->nms_colid; row = pre; pitch = (pre + 15) & ~(size_t)15; break;
    case CTPN_PF_KEEP_IDX: src = c->keep_idx; row = post * 4; pitch = (size_t)c->topn_max * 4; break;
    case CTPN_PF_KEEP_COUNTS: src = c->keep_counts; row = pitch = 4; break;
    case CTPN_PF_MW_SCRATCH:
      if (!c->nms_mw_scratch || n > (size_t)NMS_MW_CAP_BATCH) return fail(CTPN_ERR_STATE, "ctpn_debug_proposal_fetch: no multi-workgroup scratch for that many images");
      src = c->nms_mw_scratch; row = pitch = NMS_MW_SCRATCH_BYTES; break;
    case CTPN_PF_IM_INFO: src = c->im_info_dev; row = pitch = 12; break;
    default: return fail(CTPN_ERR_ARG, "ctpn_debug_proposal_fetch: unknown intermediate");
  }
  if (capacity_bytes < n * row) return fail(CTPN_ERR_CAPACITY, "ctpn_debug_proposal_fetch: the intermediate takes " + std::to_string(n * row) + " bytes");
  CTPN_HIP_TRY(hipMemcpy2D(out, row, src, pitch, row, n, hipMemcpyDeviceToHost));
  return CTPN_OK;
}

// decode_kernel's production branch (heads != nullptr: the in-kernel pair softmax, head_ld = 64, valid_rows) on caller-supplied heads: what
// ctpn_proposals runs behind a forward, here behind an upload. A post-processing-only ctx has no heads buffer, so the rows live in a block of
// this call's own.
int ctpn_debug_proposals_from_heads(ctpn_ctx* c, const float* heads, int n, int hf, int wf, const float* im_info, const int* valid_rows,
                                    int pre_nms_topn, int post_nms_topn, float nms_thresh, float min_size, float* rois_out, int* counts_out,
                                    float* cls_prob_out, float* bbox_pred_out) {
  if (!c || !heads || !im_info || !rois_out || !counts_out) return fail(CTPN_ERR_ARG, "ctpn_debug_proposals_from_heads: null pointer");
  if (n <= 0 || n > c->max_batch || hf <= 0 || wf <= 0 || (size_t)n * hf * wf > c->m5_max)
    return fail(CTPN_ERR_CAPACITY, "ctpn_debug_proposals_from_heads: shape outside what the ctx was created for");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  const size_t m = (size_t)n * hf * wf;
  DevBuf d_heads, d_valid;
  int rc;
  if ((rc = d_heads.alloc(m * 64 * sizeof(float))) || (valid_rows && (rc = d_valid.alloc((size_t)n * sizeof(int))))) return rc;
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));   // the asynchronous detect path shares the proposal buffers
  CTPN_HIP_TRY(hipMemcpy(d_heads.get(), heads, m * 64 * sizeof(float), hipMemcpyHostToDevice));
  if (valid_rows) CTPN_HIP_TRY(hipMemcpy(d_valid.get(), valid_rows, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  hipStream_t s = c->stream;
  rc = enqueue_proposals(c, d_heads.as<float>(), /*heads_are_probs*/ 0, n, hf, wf, im_info, pre_nms_topn, post_nms_topn, nms_thresh, min_size, nullptr, nullptr,
                         valid_rows ? d_valid.as<int>() : nullptr);
  // (the blocks above are released on return: nothing of this call may still be in flight then, whatever it returns)
  if (!rc && (hipMemcpyAsync(counts_out, c->keep_counts, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
              hipMemcpyAsync(rois_out, c->rois, (size_t)n * post_nms_topn * 5 * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
              (cls_prob_out && hipMemcpyAsync(cls_prob_out, c->cls_prob, m * 20 * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess) ||
              (bbox_pred_out && hipMemcpyAsync(bbox_pred_out, c->bbox_pred, m * 40 * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess)))
    rc = fail(CTPN_ERR_HIP, "ctpn_debug_proposals_from_heads: copy failed");
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail(CTPN_ERR_HIP, "ctpn_debug_proposals_from_heads: kernel failed");
  return rc;
}

int ctpn_debug_sort_keys(int device_id, const unsigned long long* keys, int n_img, int per_img, int segmented, unsigned long long* out) {
  if (!keys || !out) return fail(CTPN_ERR_ARG, "ctpn_debug_sort_keys: null pointer");
  if (n_img <= 0 || n_img > 64 || per_img <= 0 || per_img > (1 << 20)) return fail(CTPN_ERR_ARG, "ctpn_debug_sort_keys: 1 .. 64 images of 1 .. 2^20 keys");
  if (segmented && !sort_is_segmented(n_img, per_img))
    return fail(CTPN_ERR_ARG, "ctpn_debug_sort_keys: the segmented form takes up to 4 images of 4097 .. 32768 keys");
  if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_sort_keys: no HIP device visible (no CPU fallback)");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  const size_t npad = (size_t)next_pow2(per_img), total = (size_t)n_img * npad, guard = npad;
  // both buffers: the caller's keys (first buffer only), everything else CTPN_SORT_POISON, a key that reads as VALID; then a guard row of fill bytes
  std::vector<unsigned long long> h0(total, CTPN_SORT_POISON), h1(total);
  for (int i = 0; i < n_img; ++i) std::memcpy(&h0[(size_t)i * npad], keys + (size_t)i * per_img, (size_t)per_img * 8);
  std::vector<DevBuf> bufs;
  void *d0 = nullptr, *d1 = nullptr;
  int rc;
  if ((rc = dbg_alloc(bufs, &d0, (total + guard) * 8)) || (rc = dbg_alloc(bufs, &d1, (total + guard) * 8))) return rc;
  CTPN_HIP_TRY(hipMemset(d0, DBG_FILL, (total + guard) * 8));
  CTPN_HIP_TRY(hipMemset(d1, DBG_FILL, (total + guard) * 8));
  CTPN_HIP_TRY(hipMemcpy(d0, h0.data(), total * 8, hipMemcpyHostToDevice));
  std::fill(h1.begin(), h1.end(), CTPN_SORT_POISON);
  CTPN_HIP_TRY(hipMemcpy(d1, h1.data(), total * 8, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipDeviceSynchronize());
  int in_tmp = 0;
  if ((rc = launch_sort_keys((unsigned long long*)d0, (unsigned long long*)d1, n_img, (int)npad, per_img, nullptr, segmented ? &in_tmp : nullptr))) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(CTPN_ERR_HIP, "ctpn_debug_sort_keys: kernel failed");
  if (in_tmp != (segmented ? 1 : 0)) return fail(CTPN_ERR_STATE, "ctpn_debug_sort_keys: the sort did not take the form asked for");
  std::vector<char> g(guard * 8);
  for (void* d : {d0, d1}) {
    CTPN_HIP_TRY(hipMemcpy(g.data(), (const char*)d + total * 8, guard * 8, hipMemcpyDeviceToHost));
    if (!dbg_fill_intact(g.data(), guard * 8)) return fail(CTPN_ERR_STATE, "ctpn_debug_sort_keys: a guard row behind a key buffer was written");
  }
  CTPN_HIP_TRY(hipMemcpy(out, in_tmp ? d1 : d0, total * 8, hipMemcpyDeviceToHost));
  return CTPN_OK;
}

// ---- the first layer's kernels alone ---------------------------------------------------------------------------
}  // extern "C"
namespace {
// The caller's image inside a larger block, at byte DBG_IMG_PAD + byte_offset of it, every other byte of the block DBG_POISON (uint8: pixel 71;
// four of them as a float: 5.1e4): a kernel that takes a byte outside the image for a pixel computes a visibly wrong value.
// Why 64 bytes either side are enough: the first-layer kernels read the image as single elements inside it (conv_first_kernel, the float feed
// of conv_first_mfma_kernel) or as 4-byte ALIGNED dwords that hold at least one image byte -- so at most 3 bytes in front of the first and 3
// behind the last image byte -- or as the aligned dword of the image's first byte (the redirect of dwords that hold none). 64 >= 3 keeps all of
// those inside the block for any byte_offset, with room for a 16-byte aligned vector around either end.
constexpr int DBG_IMG_PAD = 64;
constexpr int DBG_POISON = 0x47;
int dbg_stage_image(std::vector<DevBuf>& bufs, const void* image, size_t bytes, int byte_offset, const void** img_dev) {
  const size_t total = ((size_t)DBG_IMG_PAD + byte_offset + bytes + DBG_IMG_PAD + 3) & ~(size_t)3;
  std::vector<unsigned char> h(total, (unsigned char)DBG_POISON);
  std::memcpy(h.data() + DBG_IMG_PAD + byte_offset, image, bytes);
  void* d = nullptr;
  if (const int rc = dbg_alloc(bufs, &d, total)) return rc;
  CTPN_HIP_TRY(hipMemcpy(d, h.data(), total, hipMemcpyHostToDevice));
  *img_dev = (const char*)d + DBG_IMG_PAD + byte_offset;      // device blocks are aligned to 256 bytes: the pointer is byte_offset mod 4
  return CTPN_OK;
}
// conv1_1's weights as the ctx holds them (api_weights.hip): w_first = HWIO flattened [27][64], the bias, and the fragment block of
// pack_conv1_frags (split-bf16 fragments, then the q-image form's bf16 and fp16 sets: conv1_p_frags)
int dbg_conv1_weights(std::vector<DevBuf>& bufs, const float* w_hwio, const float* bias, void** d_w, void** d_b, void** d_frags) {
  int rc;
  if ((rc = dbg_alloc(bufs, d_w, 27 * 64 * 4)) || (rc = dbg_alloc(bufs, d_b, 64 * 4)) || (rc = dbg_alloc(bufs, d_frags, CF_FRAGS_TOTAL))) return rc;
  CTPN_HIP_TRY(hipMemcpy(*d_w, w_hwio, 27 * 64 * 4, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemcpy(*d_b, bias, 64 * 4, hipMemcpyHostToDevice));
  return pack_conv1_frags((const float*)*d_w, (const float*)*d_b, (uint4*)*d_frags);
}
// A bordered map [n][H + 2][W + 2] of pix-byte pixels followed by DBG_GUARD_ROWS rows of W + 2 pixels, all DBG_FILL before the launch
size_t dbg_map_bytes(int n, int H, int W, size_t pix) { return ((size_t)n * (H + 2) + DBG_GUARD_ROWS) * (W + 2) * pix; }
// ... fetched after it: every border pixel and every guard row must still hold the fill
int dbg_fetch_map(const void* d_map, int n, int H, int W, size_t pix, std::vector<char>& host, const char* who) {
  host.resize(dbg_map_bytes(n, H, W, pix));
  CTPN_HIP_TRY(hipMemcpy(host.data(), d_map, host.size(), hipMemcpyDeviceToHost));
  const size_t row = (size_t)(W + 2) * pix;
  if (!dbg_fill_intact(host.data() + (size_t)n * (H + 2) * row, (size_t)DBG_GUARD_ROWS * row)) return fail(CTPN_ERR_STATE, std::string(who) + ": a guard row behind the map was written");
  for (int in = 0; in < n; ++in)
    for (int y = 0; y < H + 2; ++y) {
      const char* r = host.data() + ((size_t)in * (H + 2) + y) * row;
      const bool whole = y == 0 || y == H + 1;
      if (!(whole ? dbg_fill_intact(r, row) : (dbg_fill_intact(r, pix) && dbg_fill_intact(r + row - pix, pix))))
        return fail(CTPN_ERR_STATE, std::string(who) + ": a border pixel of the map was written (image " + std::to_string(in) + ", bordered row " + std::to_string(y) + ")");
    }
  return CTPN_OK;
}
// the interior of a fetched map as dense fp32 (split precision: hi + lo) and, where asked, its stored 16-bit values [pixel][planes x 64]
void dbg_unpack_map(const std::vector<char>& host, DType t, int n, int H, int W, float* out, uint16_t* out_bits) {
  const int planes = t == DType::SPLIT ? 2 : 1;
  const size_t pix = (size_t)64 * planes * (t == DType::F32 ? 4 : 2);
  for (int in = 0; in < n; ++in) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
    const char* p = host.data() + (((size_t)in * (H + 2) + y + 1) * (W + 2) + x + 1) * pix;
    const size_t o = ((size_t)in * H + y) * W + x;
    if (t == DType::F32) { std::memcpy(out + o * 64, p, 256); continue; }
    if (out_bits) std::memcpy(out_bits + o * 64 * planes, p, pix);
    for (int c = 0; c < 64; ++c) {
      uint16_t b; std::memcpy(&b, p + 2 * c, 2);
      float v = t == DType::F16 ? host_f16_to_f32(b) : host_bf16_to_f32(b);
      if (planes == 2) { uint16_t l; std::memcpy(&l, p + 2 * (64 + c), 2); v += host_bf16_to_f32(l); }
      out[o * 64 + c] = v;
    }
  }
}
int dbg_conv1_shape_ok(int n, int h, int w) { return n >= 1 && n <= 64 && h >= 16 && w >= 16 && h <= 8192 && w <= 8192 && (long long)n * h * w <= (1 << 20); }
}  // namespace
extern "C" {

int ctpn_debug_conv1(int device_id, const void* image, int image_is_f32, int byte_offset, const float* w_hwio, const float* bias, int n, int h, int w,
                     int precision, int form, float* out, uint16_t* out_bits, uint16_t* q_out) {
  if (!image || !w_hwio || !bias || !out) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1: null pointer");
  if (precision < CTPN_PREC_FP32 || precision > CTPN_PREC_SPLIT) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1: unknown precision");
  const DType t = prec_dtype(precision);
  const bool f32in = image_is_f32 != 0;
  if (form < 0 || form > 2) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1: form is 0 (conv_first_kernel), 1 (conv_first_mfma_kernel) or 2 (image_to_q_kernel + conv_first_p_kernel)");
  if (form == 0 && t == DType::SPLIT) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1: conv_first_kernel (form 0) stores fp32, bf16 or fp16");
  if (form == 1 && t == DType::F32) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1: conv_first_mfma_kernel (form 1) stores bf16, fp16 or split precision");
  if (form == 2 && (!dtype_is_half(t) || f32in)) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1: the q-image form (form 2) is the uint8 feed of bf16 and fp16");
  if (byte_offset < 0 || byte_offset > 3 || (f32in && byte_offset)) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1: byte_offset is 0 .. 3, and 0 for the float feed");
  if (!dbg_conv1_shape_ok(n, h, w)) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1: n 1 .. 64, h and w 16 .. 8192, at most 2^20 pixels");
  if (out_bits && t == DType::F32) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1: fp32 stores no 16-bit values (out is the stored map)");
  if (q_out && form != 2) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1: only form 2 builds a q-image");
  if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_conv1: no HIP device visible (no CPU fallback)");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  std::vector<DevBuf> bufs;
  const void* d_img = nullptr;
  void *d_w = nullptr, *d_b = nullptr, *d_frags = nullptr, *d_out = nullptr, *d_qfill = nullptr, *d_q = nullptr;
  const size_t pix = (size_t)(t == DType::SPLIT ? 128 : 64) * (t == DType::F32 ? 4 : 2), map_bytes = dbg_map_bytes(n, h, w, pix);
  const size_t q_bytes = conv1_q_bytes(n, h, w);
  int rc;
  if ((rc = dbg_stage_image(bufs, image, (size_t)n * h * w * 3 * (f32in ? 4 : 1), byte_offset, &d_img)) || (rc = dbg_conv1_weights(bufs, w_hwio, bias, &d_w, &d_b, &d_frags)) ||
      (rc = dbg_alloc(bufs, &d_out, map_bytes))) return rc;
  CTPN_HIP_TRY(hipMemset(d_out, DBG_FILL, map_bytes));
  if (form == 2) {
    if ((rc = dbg_alloc(bufs, &d_qfill, q_bytes)) || (rc = dbg_alloc(bufs, &d_q, q_bytes))) return rc;
    CTPN_HIP_TRY(hipMemset(d_qfill, DBG_FILL, q_bytes));
    CTPN_HIP_TRY(hipMemset(d_q, 0, q_bytes));
  }
  CTPN_HIP_TRY(hipDeviceSynchronize());
  if (form == 2) {
    // the q-image twice: into a filled buffer, where a write outside the image's pixels shows, and into a zeroed one, the product's initial
    // state, which the conv then reads
    if ((rc = launch_image_to_q((const uint8_t*)d_img, d_qfill, t, n, h, w, nullptr)) || (rc = launch_image_to_q((const uint8_t*)d_img, d_q, t, n, h, w, nullptr)) ||
        (rc = launch_conv_first_from_q(d_q, conv1_p_frags(d_frags, t), d_out, t, n, h, w, 0, w, nullptr))) return rc;
  } else if ((rc = launch_conv_first(d_img, f32in ? 1 : 0, (const float*)d_w, (const float*)d_b, d_out, t, n, h, w, nullptr, form == 1 ? d_frags : nullptr))) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(CTPN_ERR_HIP, "ctpn_debug_conv1: kernel failed");
  if (form == 2) {
    const int hq = conv1_q_h(h), wq = conv1_q_w(w);
    std::vector<char> hq_img(q_bytes);
    CTPN_HIP_TRY(hipMemcpy(hq_img.data(), d_qfill, q_bytes, hipMemcpyDeviceToHost));
    const size_t qrow = (size_t)wq * 8, used = (size_t)n * hq * qrow;
    if (!dbg_fill_intact(hq_img.data() + used, q_bytes - used)) return fail(CTPN_ERR_STATE, "ctpn_debug_conv1: the q-image buffer was written behind the last image");
    for (int in = 0; in < n; ++in)
      for (int y = 0; y < hq; ++y) {
        const char* r = hq_img.data() + ((size_t)in * hq + y) * qrow;
        const bool inside = y >= 2 && y < 2 + h;
        if (!(inside ? (dbg_fill_intact(r, 16) && dbg_fill_intact(r + (size_t)(2 + w) * 8, qrow - (size_t)(2 + w) * 8)) : dbg_fill_intact(r, qrow)))
          return fail(CTPN_ERR_STATE, "ctpn_debug_conv1: a frame pixel of the q-image was written (image " + std::to_string(in) + ", q row " + std::to_string(y) + ")");
      }
    if (q_out) std::memcpy(q_out, hq_img.data(), used);
  }
  std::vector<char> host;
  if ((rc = dbg_fetch_map(d_out, n, h, w, pix, host, "ctpn_debug_conv1"))) return rc;
  dbg_unpack_map(host, t, n, h, w, out, out_bits);
  return CTPN_OK;
}

}  // extern "C"
namespace {
// ctpn_debug_conv1_fused (cu_count 0) and ctpn_debug_conv1_fused_walk (conv1_2's launch laid out for cu_count CUs: launch_conv3x3's argument)
int dbg_conv1_fused_body(int device_id, const uint8_t* image, int byte_offset, const float* w_hwio, const float* bias, const float* w2_hwio, const float* bias2,
                         int n, int h, int w, int precision, int cu_count, float* out_pool, uint16_t* out_bits) {
  if (!image || !w_hwio || !bias || !w2_hwio || !bias2 || !out_pool) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1_fused: null pointer");
  if (precision != CTPN_PREC_BF16 && precision != CTPN_PREC_FP16) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1_fused: the fused form is bf16 or fp16");
  if (byte_offset < 0 || byte_offset > 3) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1_fused: byte_offset is 0 .. 3");
  if (!dbg_conv1_shape_ok(n, h, w)) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1_fused: n 1 .. 64, h and w 16 .. 8192, at most 2^20 pixels");
  if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_conv1_fused: no HIP device visible (no CPU fallback)");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  const DType t = prec_dtype(precision);
  const int ho = h / 2, wo = w / 2;
  std::vector<DevBuf> bufs;
  const void* d_img = nullptr;
  void *d_w = nullptr, *d_b = nullptr, *d_frags = nullptr, *d_w2 = nullptr, *d_wt2 = nullptr, *d_b2 = nullptr, *d_q = nullptr, *d_pool = nullptr;
  const size_t pix = 64 * 2, map_bytes = dbg_map_bytes(n, ho, wo, pix), q_bytes = conv1_q_bytes(n, h, w), wt_bytes = (size_t)128 * 9 * 64 * 2;
  int rc;
  if ((rc = dbg_stage_image(bufs, image, (size_t)n * h * w * 3, byte_offset, &d_img)) || (rc = dbg_conv1_weights(bufs, w_hwio, bias, &d_w, &d_b, &d_frags)) ||
      (rc = dbg_alloc(bufs, &d_w2, (size_t)9 * 64 * 64 * 4)) || (rc = dbg_alloc(bufs, &d_wt2, wt_bytes)) || (rc = dbg_alloc(bufs, &d_b2, 128 * 4)) ||
      (rc = dbg_alloc(bufs, &d_q, q_bytes)) || (rc = dbg_alloc(bufs, &d_pool, map_bytes))) return rc;
  CTPN_HIP_TRY(hipMemcpy(d_w2, w2_hwio, (size_t)9 * 64 * 64 * 4, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemset(d_wt2, 0, wt_bytes));      // weight rows and bias padded to 128 channels with zeros, as ctpn_debug_conv3x3 does
  CTPN_HIP_TRY(hipMemset(d_b2, 0, 128 * 4));
  CTPN_HIP_TRY(hipMemcpy(d_b2, bias2, 64 * 4, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemset(d_q, 0, q_bytes));          // the zero frame is the buffer's initial state
  CTPN_HIP_TRY(hipMemset(d_pool, DBG_FILL, map_bytes));
  CTPN_HIP_TRY(hipDeviceSynchronize());
  // the production chain of api_forward.hip: bytes -> q-image, conv1_1 inside conv1_2's window stage (conv1_1's map is never stored: no `in`)
  if ((rc = launch_pack_transpose((const float*)d_w2, 64, d_wt2, 9 * 64, t, 9 * 64, 64, nullptr)) || (rc = launch_image_to_q((const uint8_t*)d_img, d_q, t, n, h, w, nullptr)) ||
      (rc = launch_conv3x3(nullptr, d_wt2, (const float*)d_b2, nullptr, d_pool, t, n, h, w, 64, 64, 1, nullptr, 0, d_q, conv1_p_frags(d_frags, t), 3, cu_count))) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(CTPN_ERR_HIP, "ctpn_debug_conv1_fused: kernel failed");
  std::vector<char> host;
  if ((rc = dbg_fetch_map(d_pool, n, ho, wo, pix, host, "ctpn_debug_conv1_fused"))) return rc;
  dbg_unpack_map(host, t, n, ho, wo, out_pool, out_bits);
  return CTPN_OK;
}
}  // namespace
extern "C" {

int ctpn_debug_conv1_fused(int device_id, const uint8_t* image, int byte_offset, const float* w_hwio, const float* bias, const float* w2_hwio, const float* bias2,
                           int n, int h, int w, int precision, float* out_pool, uint16_t* out_bits) {
  return dbg_conv1_fused_body(device_id, image, byte_offset, w_hwio, bias, w2_hwio, bias2, n, h, w, precision, 0, out_pool, out_bits);
}

int ctpn_debug_conv1_fused_walk(int device_id, const uint8_t* image, int byte_offset, const float* w_hwio, const float* bias, const float* w2_hwio, const float* bias2,
                                int n, int h, int w, int precision, int cu_count, float* out_pool, uint16_t* out_bits) {
  if (cu_count < 0) return fail(CTPN_ERR_ARG, "ctpn_debug_conv1_fused_walk: cu_count is 1 .. the device's CU count, or 0 for the device's");
  return dbg_conv1_fused_body(device_id, image, byte_offset, w_hwio, bias, w2_hwio, bias2, n, h, w, precision, cu_count, out_pool, out_bits);
}

// The tile walk of the main launch of one conv3x3 layer (c3_walk, conv3x3_plan.h: what c3_launch_p / c3_launch_wr copy into the kernel
// argument) for the widths w_first .. w_first + w_count - 1; arguments as ctpn_debug_conv3x3_plan. Host arithmetic only.
int ctpn_debug_conv3x3_walk_plan(int precision, int n, int h, int w_first, int w_count, int ci, int co, int fuse_pool, int keep_full, int dup_hi,
                                 int conv_p64, int split_edge, int cu_count, int* out) {
  if (!out || w_count <= 0) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_walk_plan: no output");
  if (precision < CTPN_PREC_FP32 || precision > CTPN_PREC_SPLIT) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_walk_plan: unknown precision");
  const DType t = prec_dtype(precision);
  if (n <= 0 || h <= 0 || w_first <= 0 || w_first > 0x7fffffff - w_count || ci <= 0 || ci % (t == DType::F32 ? 32 : 64) != 0 || co <= 0 || co % (t == DType::F32 ? 4 : 8) != 0)
    return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_walk_plan: shape out of range (Ci a multiple of 32 / 64, Co of 4 / 8)");
  if (dup_hi && t != DType::SPLIT) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_walk_plan: dup_hi is a split-precision layout");
  if (cu_count < 0) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_walk_plan: cu_count is a CU count, or 0 for the current device's");
  if (cu_count == 0) {
    if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_conv3x3_walk_plan: cu_count 0 asks the current device, and no HIP device is visible");
    int dev = 0, rc;
    if ((rc = current_device(dev)) || (rc = device_cu_count(dev, cu_count))) return rc;
  }
  const bool pool = fuse_pool != 0, keep = keep_full != 0 || !pool;
  for (int i = 0; i < w_count; ++i) {
    const int w = w_first + i;
    const C3Plan p = c3_plan(t, n, h, w, ci, co, pool, keep, dup_hi, true, true, (conv_p64 ? 1 : 0) | (split_edge ? 2 : 0), cu_count);
    if (p.main_form == C3M_NONE) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_walk_plan: no kernel for this shape (split precision: Co <= 64 or a multiple of 128)");
    const C3Walk k = c3_walk(p.main_form, n, h, w, co, pool, keep, p.w_cover, cu_count);
    if (k.ptiles_total > 0x7fffffffLL || k.grid > 0x7fffffffLL) return fail(CTPN_ERR_ARG, "ctpn_debug_conv3x3_walk_plan: more than 2^31 - 1 tiles");
    int* o = out + (size_t)i * CTPN_CONV_WALK_INTS;
    o[0] = k.main_form; o[1] = k.tiles_x; o[2] = k.tiles_y; o[3] = k.tiles_n; o[4] = k.stacked; o[5] = (int)k.ptiles_total; o[6] = (int)k.workers;
    o[7] = (int)k.ht_full; o[8] = k.ht_r; o[9] = k.groups; o[10] = k.per_group; o[11] = (int)k.grid;
    // 128-byte K chunks per tap = window refills per tile of the persistent kernel (split precision: three K blocks, hi / lo / hi)
    o[12] = (t == DType::SPLIT ? 3 * ci : ci) / (t == DType::F32 ? 32 : 64);
    o[13] = k.ht;
  }
  return CTPN_OK;
}

}  // extern "C"
