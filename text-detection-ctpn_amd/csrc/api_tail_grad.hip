// C ABI of libctpn_hip.so, tail-gradient unit: the recurrent tail (BiLSTM, lstm_o FC, the two heads) forward with saved activations, and its
// backward pass (tail_grad.hip, bilstm.hip's saving form, the forward's own GEMM launcher). Stateless, with ctpn_anchor_targets' conventions: no
// ctx is read or written; each call runs on a stream of its own, which waits for no other stream, and synchronises once, at its end; its device
// blocks are allocated by the call and released before it returns; the caller's current device is put back. The definitions:
// include/ctpn_hip.h, "the recurrent tail: forward with saved activations, backward".
#include "ctx.h"
#include "tail_grad_dev.h"

namespace {
using namespace ctpn;

constexpr long long kMaxCells = 1LL << 21;      // cells x 1024 gate columns stays below 2^31

int tail_device(int device_id, const char* who) {
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
  // scratch: the call needs the array even where the caller does not ask for it
  int out(float* p, size_t floats, int on_device, bool scratch) {
    bytes = floats * sizeof(float);
    if (!p && !scratch) return CTPN_OK;
    if (p && on_device) { dev = p; return CTPN_OK; }
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

int check_shape(const char* who, int n, int hf, int wf, int on_device, long long& M) {
  if (n <= 0 || hf <= 0 || wf <= 0) return fail(CTPN_ERR_ARG, std::string(who) + ": n, hf, wf >= 1");
  M = (long long)n * hf * wf;
  if (M > kMaxCells) return fail(CTPN_ERR_ARG, std::string(who) + ": n x hf x wf beyond 2^21 cells");
  if (on_device != 0 && on_device != 1) return fail(CTPN_ERR_ARG, std::string(who) + ": on_device is 0 or 1");
  return CTPN_OK;
}

int plain_gemm(const float* a, int lda, const float* wt, const float* bias, float* out, long long M, int K, int Co, int ldc, hipStream_t s) {
  IGemm g{};
  g.a = a; g.wt = wt; g.bias = bias; g.out = out;
  g.M = M; g.Ci = K; g.ntaps = 1; g.Co = Co; g.a_plain = 1; g.lda = lda; g.out_bordered = 0; g.ldc = ldc; g.relu = 0;
  return launch_igemm(g, DType::F32, DType::F32, s);
}

}  // namespace

extern "C" {

long long ctpn_tail_saved_floats(int n, int hf, int wf) {
  long long M;
  if (check_shape("ctpn_tail_saved_floats", n, hf, wf, 0, M)) return -1;
  return M * TB_SAVED_PER_CELL;
}

int ctpn_tail_forward(int device_id, int n, int hf, int wf, const float* x, const float* tail, int on_device, float* heads, float* saved) {
  long long M;
  int rc = check_shape("ctpn_tail_forward", n, hf, wf, on_device, M);
  if (rc) return rc;
  if (!x || !tail || !heads) return fail(CTPN_ERR_ARG, "ctpn_tail_forward: null pointer");
  if (on_device && !(aligned16(x) && aligned16(tail) && aligned16(heads) && aligned16(saved)))
    return fail(CTPN_ERR_ARG, "ctpn_tail_forward: device pointers are 16-byte aligned");
  if ((rc = tail_device(device_id, "ctpn_tail_forward"))) return rc;
  DeviceGuard guard;
  if ((rc = guard.enter(device_id))) return rc;
  const size_t Mz = (size_t)M;
  Stream st;
  Arg a_x, a_tail, a_heads, a_saved;      // released before the stream, on every way out
  DevBuf wtmp, btmp, wt_x, b_x, wh, wt_fc, wt_h, b_h, xp, acts;
  if ((rc = st.ensure())) return rc;
  if ((rc = a_x.in(x, Mz * 512, on_device, st)) || (rc = a_tail.in(tail, TB_TAIL_FLOATS, on_device, st)) ||
      (rc = a_heads.out(heads, Mz * 64, on_device, true)) || (rc = a_saved.out(saved, Mz * TB_SAVED_PER_CELL, on_device, false)))
    return rc;
  if ((rc = wtmp.alloc((size_t)1024 * 512 * 4)) || (rc = btmp.alloc(1024 * 4)) || (rc = wt_x.alloc((size_t)1024 * 512 * 4)) || (rc = b_x.alloc(1024 * 4)) ||
      (rc = wh.alloc((size_t)2 * 128 * 512 * 4)) || (rc = wt_fc.alloc((size_t)512 * 256 * 4)) || (rc = wt_h.alloc((size_t)64 * 512 * 4)) || (rc = b_h.alloc(64 * 4)) || (rc = xp.alloc(Mz * 1024 * 4)))
    return rc;
  const float* T = a_tail.dev;
  // the weights in the forward's packed layouts (api_weights.hip pack_weights, fp32): [gate][in] rows in lstm_gate_col's order, [out][in] for the FC and
  // the heads (bbox | cls | four zero rows)
  for (int d = 0; d < 2; ++d) {
    if ((rc = launch_pack_transpose(T + tb_off_kernel(d), 512, wtmp.as<float>() + (size_t)d * 512 * 512, 512, DType::F32, 512, 512, st))) return rc;
    CTPN_HIP_TRY(hipMemcpyAsync(btmp.as<float>() + d * 512, T + tb_off_bias(d), 512 * 4, hipMemcpyDeviceToDevice, st));
  }
  if ((rc = launch_lstm_permute_rows(wtmp.get(), wt_x.get(), 512 * 4, st)) || (rc = launch_lstm_permute_rows(btmp.get(), b_x.get(), 4, st))) return rc;
  if ((rc = launch_pack_transpose(T + TB_OFF_WFC, 512, wt_fc.get(), 256, DType::F32, 256, 512, st))) return rc;
  CTPN_HIP_TRY(hipMemsetAsync(wt_h.get(), 0, wt_h.bytes(), st));
  CTPN_HIP_TRY(hipMemsetAsync(b_h.get(), 0, b_h.bytes(), st));
  if ((rc = launch_pack_transpose(T + TB_OFF_WBOX, 40, wt_h.get(), 512, DType::F32, 512, 40, st)) ||
      (rc = launch_pack_transpose(T + TB_OFF_WCLS, 20, wt_h.as<float>() + (size_t)40 * 512, 512, DType::F32, 512, 20, st)))
    return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(b_h.get(), T + TB_OFF_BBOX, 40 * 4, hipMemcpyDeviceToDevice, st));
  CTPN_HIP_TRY(hipMemcpyAsync(b_h.as<float>() + 40, T + TB_OFF_BCLS, 20 * 4, hipMemcpyDeviceToDevice, st));
  // without a saved block the two activations live in a block of this call and the plain recurrence runs
  float *lstm_out, *lstm_o;
  if (a_saved.dev) { lstm_out = a_saved.dev + tb_saved_lstm_out(Mz); lstm_o = a_saved.dev + tb_saved_lstm_o(Mz); }
  else {
    if ((rc = acts.alloc(Mz * (256 + 512) * 4))) return rc;
    lstm_out = acts.as<float>(); lstm_o = lstm_out + Mz * 256;
  }
  if ((rc = plain_gemm(a_x.dev, 512, wt_x.as<float>(), b_x.as<float>(), xp.as<float>(), M, 512, 1024, 1024, st))) return rc;
  // Wh = kernel[512:] of the two directions side by side, as the recurrence reads it
  for (int d = 0; d < 2; ++d)
    CTPN_HIP_TRY(hipMemcpyAsync(wh.as<float>() + (size_t)d * 128 * 512, T + tb_off_kernel(d) + (size_t)512 * 512, (size_t)128 * 512 * 4, hipMemcpyDeviceToDevice, st));
  if (a_saved.dev) rc = launch_bilstm_save(xp.as<float>(), wh.as<float>(), lstm_out, a_saved.dev + tb_saved_gates(Mz), n * hf, wf, st);
  else rc = launch_bilstm(xp.get(), 0, wh.as<float>(), lstm_out, n * hf, wf, st, 0, 0);
  if (rc) return rc;
  if ((rc = plain_gemm(lstm_out, 256, wt_fc.as<float>(), T + TB_OFF_BFC, lstm_o, M, 256, 512, 512, st))) return rc;
  CTPN_HIP_TRY(hipMemsetAsync(a_heads.dev, 0, Mz * 64 * 4, st));      // the GEMM writes columns 0..59
  if ((rc = plain_gemm(lstm_o, 512, wt_h.as<float>(), b_h.as<float>(), a_heads.dev, M, 512, 60, 64, st))) return rc;
  if ((rc = a_heads.fetch(st)) || (rc = a_saved.fetch(st))) return rc;
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

int ctpn_tail_backward(int device_id, int n, int hf, int wf, const float* x, const float* tail, const float* saved, const float* d_heads, int on_device,
                       float* d_tail, float* d_x) {
  long long M;
  int rc = check_shape("ctpn_tail_backward", n, hf, wf, on_device, M);
  if (rc) return rc;
  if (!x || !tail || !saved || !d_heads || !d_tail) return fail(CTPN_ERR_ARG, "ctpn_tail_backward: null pointer");
  if (on_device && !(aligned16(x) && aligned16(tail) && aligned16(saved) && aligned16(d_heads) && aligned16(d_tail) && aligned16(d_x)))
    return fail(CTPN_ERR_ARG, "ctpn_tail_backward: device pointers are 16-byte aligned");
  if ((rc = tail_device(device_id, "ctpn_tail_backward"))) return rc;
  DeviceGuard guard;
  if ((rc = guard.enter(device_id))) return rc;
  const size_t Mz = (size_t)M;
  const long long block = tb_block_cells(M);
  const size_t P = (size_t)((M + block - 1) / block);
  Stream st;
  Arg a_x, a_tail, a_saved, a_dh, a_dtail, a_dx;      // released before the stream, on every way out
  DevBuf dh64, hrows, d_lstm_o, d_lstm_out, d_pre, wxt, parts, bsum;
  if ((rc = st.ensure())) return rc;
  if ((rc = a_x.in(x, Mz * 512, on_device, st)) || (rc = a_tail.in(tail, TB_TAIL_FLOATS, on_device, st)) ||
      (rc = a_saved.in(saved, Mz * TB_SAVED_PER_CELL, on_device, st)) || (rc = a_dh.in(d_heads, Mz * 64, on_device, st)) ||
      (rc = a_dtail.out(d_tail, TB_TAIL_FLOATS, on_device, true)) || (rc = a_dx.out(d_x, Mz * 512, on_device, false)))
    return rc;
  if ((rc = dh64.alloc(Mz * 64 * 4)) || (rc = hrows.alloc((size_t)512 * 64 * 4)) || (rc = d_lstm_o.alloc(Mz * 512 * 4)) || (rc = d_lstm_out.alloc(Mz * 256 * 4)) ||
      (rc = d_pre.alloc(Mz * 1024 * 4)) || (rc = parts.alloc(P * 512 * 512 * 4)) || (rc = bsum.alloc(64 * 4)))
    return rc;
  const float* T = a_tail.dev;
  const float* lstm_out = a_saved.dev + tb_saved_lstm_out(Mz);
  const float* lstm_o = a_saved.dev + tb_saved_lstm_o(Mz);
  const float* gates = a_saved.dev + tb_saved_gates(Mz);
  float* G = a_dtail.dev;
  float* pt = parts.as<float>();
  // the data gradients down to d_pre. A product with the transposed weights reads them in TF's own [in][out] layout: it is the GEMM's [Co][K]
  if ((rc = launch_mask_dheads(a_dh.dev, dh64.as<float>(), M, st)) || (rc = launch_heads_rows(T, hrows.as<float>(), st))) return rc;
  if ((rc = plain_gemm(dh64.as<float>(), 64, hrows.as<float>(), nullptr, d_lstm_o.as<float>(), M, 64, 512, 512, st))) return rc;
  if ((rc = plain_gemm(d_lstm_o.as<float>(), 512, T + TB_OFF_WFC, nullptr, d_lstm_out.as<float>(), M, 512, 256, 256, st))) return rc;
  if ((rc = launch_bptt(d_lstm_out.as<float>(), gates, T, d_pre.as<float>(), n * hf, wf, st))) return rc;
  if (a_dx.dev) {
    if ((rc = wxt.alloc((size_t)512 * 1024 * 4))) return rc;
    for (int d = 0; d < 2; ++d)      // [512 in][fw 512 gates | bw 512 gates]
      CTPN_HIP_TRY(hipMemcpy2DAsync(wxt.as<float>() + d * 512, 1024 * 4, T + tb_off_kernel(d), 512 * 4, 512 * 4, 512, hipMemcpyDeviceToDevice, st));
    if ((rc = plain_gemm(d_pre.as<float>(), 1024, wxt.as<float>(), nullptr, a_dx.dev, M, 1024, 512, 512, st))) return rc;
  }
  // the weight gradients, tensor by tensor in d_tail's order; the partials block is reused in stream order
  for (int d = 0; d < 2; ++d) {
    const float* dp = d_pre.as<float>() + d * TB_GATES;
    if ((rc = launch_tail_tn(a_x.dev, 512, 0, dp, 1024, M, wf, 512, 512, pt, G + tb_off_kernel(d), 512, st))) return rc;
    // Wh: z_t took h of the step before in the direction's walk -- the cell to the left (fw) or to the right (bw)
    if ((rc = launch_tail_tn(lstm_out + d * TB_UNITS, 256, d ? 1 : -1, dp, 1024, M, wf, 128, 512, pt, G + tb_off_kernel(d) + (size_t)512 * 512, 512, st))) return rc;
    if ((rc = launch_tail_colsum(dp, 1024, M, 512, pt, G + tb_off_bias(d), st))) return rc;
  }
  if ((rc = launch_tail_tn(lstm_out, 256, 0, d_lstm_o.as<float>(), 512, M, wf, 256, 512, pt, G + TB_OFF_WFC, 512, st))) return rc;
  if ((rc = launch_tail_colsum(d_lstm_o.as<float>(), 512, M, 512, pt, G + TB_OFF_BFC, st))) return rc;
  if ((rc = launch_tail_tn(lstm_o, 512, 0, dh64.as<float>(), 64, M, wf, 512, 40, pt, G + TB_OFF_WBOX, 40, st))) return rc;
  if ((rc = launch_tail_tn(lstm_o, 512, 0, dh64.as<float>() + 40, 64, M, wf, 512, 20, pt, G + TB_OFF_WCLS, 20, st))) return rc;
  if ((rc = launch_tail_colsum(dh64.as<float>(), 64, M, 60, pt, bsum.as<float>(), st))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(G + TB_OFF_BBOX, bsum.get(), 40 * 4, hipMemcpyDeviceToDevice, st));
  CTPN_HIP_TRY(hipMemcpyAsync(G + TB_OFF_BCLS, bsum.as<float>() + 40, 20 * 4, hipMemcpyDeviceToDevice, st));
  if ((rc = a_dtail.fetch(st)) || (rc = a_dx.fetch(st))) return rc;
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

// test hook in ctpn_debug_gemm's style: the backward recurrence alone, host arrays. gates [rows * T][2][5][128] (the saved block's third
// part), d_lstm_out [rows * T][256] -> d_pre [rows * T][1024], the stage ctpn_tail_backward keeps to itself
int ctpn_debug_tail_bptt(int device_id, int rows, int T, const float* d_lstm_out, const float* gates, const float* tail, float* d_pre) {
  if (rows <= 0 || T <= 0 || (long long)rows * T > kMaxCells) return fail(CTPN_ERR_ARG, "ctpn_debug_tail_bptt: rows, T >= 1, rows x T <= 2^21");
  if (!d_lstm_out || !gates || !tail || !d_pre) return fail(CTPN_ERR_ARG, "ctpn_debug_tail_bptt: null pointer");
  int rc = tail_device(device_id, "ctpn_debug_tail_bptt");
  if (rc) return rc;
  DeviceGuard guard;
  if ((rc = guard.enter(device_id))) return rc;
  const size_t Mz = (size_t)rows * T;
  Stream st;
  Arg a_d, a_g, a_t, a_o;
  if ((rc = st.ensure())) return rc;
  if ((rc = a_d.in(d_lstm_out, Mz * 256, 0, st)) || (rc = a_g.in(gates, Mz * 2 * 5 * TB_UNITS, 0, st)) || (rc = a_t.in(tail, TB_TAIL_FLOATS, 0, st)) ||
      (rc = a_o.out(d_pre, Mz * 1024, 0, true)))
    return rc;
  if ((rc = launch_bptt(a_d.dev, a_g.dev, a_t.dev, a_o.dev, rows, T, st)) || (rc = a_o.fetch(st))) return rc;
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

}  // extern "C"
