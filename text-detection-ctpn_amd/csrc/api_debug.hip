// C ABI of libctpn_hip.so, test hooks: ctpn_debug_* entry points that run one kernel on caller-supplied data, everything on the null stream.
// Not on the product path.
#include "ctx.h"
#include "conv3x3_plan.h"

extern "C" {

// ---- diagnostics ---------------------------------------------------------------------------------------------
// One 3x3 conv (+bias+ReLU, optionally + 2x2 max-pool) on caller-supplied dense tensors: the unit-test hook for the
// conv kernels on shapes the VGG trunk never produces (odd sizes, tails, single rows). Not on the product path.
int ctpn_debug_cvt_bf16(int device_id, const float* in, uint16_t* out, int n, int use_hw_instruction) {
  if (!in || !out || n <= 0) return fail(CTPN_ERR_ARG, "ctpn_debug_cvt_bf16: bad argument");
  if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_cvt_bf16: no HIP device visible (no CPU fallback)");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  float* d_in = nullptr; uint16_t* d_out = nullptr;
  CTPN_HIP_TRY(hipMalloc((void**)&d_in, (size_t)n * 4));
  CTPN_HIP_TRY(hipMalloc((void**)&d_out, (size_t)n * 2 + 4));
  CTPN_HIP_TRY(hipMemcpy(d_in, in, (size_t)n * 4, hipMemcpyHostToDevice));
  int rc = launch_cvt_bf16(d_in, d_out, n, use_hw_instruction, nullptr);
  if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(CTPN_ERR_HIP, "ctpn_debug_cvt_bf16: kernel failed");
  if (!rc && hipMemcpy(out, d_out, (size_t)n * 2, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(CTPN_ERR_HIP, "ctpn_debug_cvt_bf16: copy failed");
  (void)hipFree(d_in); (void)hipFree(d_out);
  return rc;
}

int ctpn_debug_lds_dma(int device_id, const uint8_t* src, size_t bytes, uint8_t* out_clobber, uint8_t* out_keep) {
  if (!src || !out_clobber || !out_keep || bytes == 0 || bytes % 1024 != 0 || bytes > ((size_t)1 << 30)) return fail(CTPN_ERR_ARG, "ctpn_debug_lds_dma: bytes must be a positive multiple of 1024 (<= 1 GiB)");
  if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_lds_dma: no HIP device visible (no CPU fallback)");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  char *d_in = nullptr, *d_a = nullptr, *d_b = nullptr;
  auto cleanup = [&]() { for (void* p : {(void*)d_in, (void*)d_a, (void*)d_b}) if (p) (void)hipFree(p); };
  struct Guard { decltype(cleanup)& f; ~Guard() { f(); } } guard{cleanup};
  CTPN_HIP_TRY(hipMalloc((void**)&d_in, bytes));
  CTPN_HIP_TRY(hipMalloc((void**)&d_a, bytes));
  CTPN_HIP_TRY(hipMalloc((void**)&d_b, bytes));
  CTPN_HIP_TRY(hipMemcpy(d_in, src, bytes, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemset(d_a, 0xA5, bytes));
  CTPN_HIP_TRY(hipMemset(d_b, 0x5A, bytes));
  CTPN_HIP_TRY(hipDeviceSynchronize());
  int rc = launch_lds_dma_check(d_in, d_a, d_b, (int)(bytes / 1024), nullptr);
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(CTPN_ERR_HIP, "ctpn_debug_lds_dma: kernel failed");
  CTPN_HIP_TRY(hipMemcpy(out_clobber, d_a, bytes, hipMemcpyDeviceToHost));
  CTPN_HIP_TRY(hipMemcpy(out_keep, d_b, bytes, hipMemcpyDeviceToHost));
  return CTPN_OK;
}

int ctpn_debug_conv3x3(int device_id, const float* in_nhwc, const float* w_hwio, const float* bias, int n, int h, int w, int ci,
                       int co, int precision, int impl, int fuse_pool, float* out_full, float* out_pool) {
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
  void *d_in = nullptr, *d_out = nullptr, *d_pool = nullptr, *d_wt = nullptr; float *d_w = nullptr, *d_b = nullptr;
  char* d_in_alloc = nullptr;
  hipStream_t s = nullptr;
  int rc = CTPN_OK;
  auto cleanup = [&]() { for (void* p : {(void*)d_in_alloc, d_out, d_pool, d_wt, (void*)d_w, (void*)d_b}) if (p) (void)hipFree(p); };
  struct Guard { decltype(cleanup)& f; ~Guard() { f(); } } guard{cleanup};
  const size_t in_front = act_front_pixels(w) * cin_p * es;
  const size_t wt_bytes = (size_t)co_pad * 9 * ci * (split ? 6 : es);
  CTPN_HIP_TRY(hipMalloc((void**)&d_in_alloc, in_front + in_elems * es));
  CTPN_HIP_TRY(hipMemset(d_in_alloc, 0, in_front));
  d_in = d_in_alloc + in_front;
  CTPN_HIP_TRY(hipMalloc(&d_out, out_elems * es));
  CTPN_HIP_TRY(hipMalloc(&d_pool, pool_elems * es + 256));
  CTPN_HIP_TRY(hipMalloc(&d_wt, wt_bytes));
  CTPN_HIP_TRY(hipMalloc((void**)&d_w, (size_t)9 * ci * co * 4));
  CTPN_HIP_TRY(hipMalloc((void**)&d_b, (size_t)co_pad * 4));
  CTPN_HIP_TRY(hipMemset(d_out, 0, out_elems * es));
  CTPN_HIP_TRY(hipMemset(d_pool, 0, pool_elems * es + 256));
  CTPN_HIP_TRY(hipMemset(d_wt, 0, wt_bytes));
  CTPN_HIP_TRY(hipMemset(d_b, 0, (size_t)co_pad * 4));
  CTPN_HIP_TRY(hipMemcpy(d_in, hin.data(), in_elems * es, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemcpy(d_w, w_hwio, (size_t)9 * ci * co * 4, hipMemcpyHostToDevice));
  CTPN_HIP_TRY(hipMemcpy(d_b, bias, (size_t)co * 4, hipMemcpyHostToDevice));
  rc = split ? launch_pack_transpose_split(d_w, co, d_wt, 9, ci, co, s) : launch_pack_transpose(d_w, co, d_wt, 9 * ci, t, 9 * ci, co, s);
  bool host_pool = false;
  if (!rc) {
    if (impl == 1) {
      rc = launch_conv3x3(d_in, d_wt, d_b, (out_full || !fuse_pool) ? d_out : nullptr, fuse_pool ? d_pool : nullptr, t, n, h, w, ci, co, 1, s, dup);
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
    std::vector<char> tmp(elems * es);
    CTPN_HIP_TRY(hipMemcpy(tmp.data(), dsrc, elems * es, hipMemcpyDeviceToHost));
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
          if (dup_plane && std::memcmp(&tmp[(o + 2 * co) * 2], &b, 2) != 0) return fail(CTPN_ERR_STATE, "ctpn_debug_conv3x3: the dup_hi plane differs from the hi plane");
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
  return rc;
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

}  // extern "C"
