// Internal declarations shared by the translation units of libctpn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/ctpn_hip.h"
#include "jpeg_pixel.h"
#include "jpeg_huff_dev.h"
#include "ragged_dev.h"

namespace ctpn {

// ---------------------------------------------------------------------------------------------
// 16-bit MFMA operand types. The throughput modes compute in bf16 (CTPN_PREC_BF16, BASELINE.json's dtype) or IEEE fp16
// (CTPN_PREC_FP16: same MFMA rate -- v_mfma_f32_32x32x16_f16 --, three more mantissa bits); the parity-grade
// mode CTPN_PREC_SPLIT stores every activation and weight as a (hi, lo) PAIR of bf16 and spends three bf16 MFMAs per product.
// Everything that only moves 16-bit payloads is type-blind; what differs is collected here: the packed convert, the widening, the
// MFMA opcode (builtin, and the mnemonic for the weights-in-registers kernel's inline asm).
// ---------------------------------------------------------------------------------------------
struct h_bf16 { uint16_t v; };
struct h_f16 { uint16_t v; };

#if defined(__HIPCC__)
typedef float ctpn_f32x2 __attribute__((ext_vector_type(2)));
typedef float ctpn_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 ctpn_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 ctpn_f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 ctpn_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 ctpn_f16x8 __attribute__((ext_vector_type(8)));
// two fp32 -> packed bf16 (lo in bits 15:0), round-to-nearest-even: one v_cvt_pk_bf16_f32 instead of ~12 VALU ops.
// Bit-identical to the integer RNE formula for finite inputs (tests/test_gpu_parity.py::test_bf16_convert_matches_rne).
// Written as a vector fptrunc (hipcc selects v_cvt_pk_bf16_f32 for it on gfx950), NOT as inline asm: the hazard
// recognizer does not look into asm operands, so an asm convert that is the first reader of an MFMA result runs before
// the accumulator is written back (seen as NaNs in conv_first_mfma_kernel).
__device__ __forceinline__ unsigned int ctpn_cvt_pk_bf16(float lo, float hi) {
  const ctpn_f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, ctpn_bf16x2));
}
__device__ __forceinline__ unsigned int ctpn_cvt_pk_f16(float lo, float hi) {
  const ctpn_f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, ctpn_f16x2));      // v_cvt_pk_f16_f32 (RNE)
}
__device__ __forceinline__ float ctpn_bf16_to_f32(unsigned short h) { return __builtin_bit_cast(float, (unsigned int)h << 16); }
__device__ __forceinline__ float ctpn_f16_to_f32(unsigned short h) { return (float)__builtin_bit_cast(_Float16, h); }
// fp32 -> one bf16 (software RNE, NaN-preserving: the reference formula the hardware convert is tested against)
__device__ __forceinline__ unsigned short ctpn_f32_to_bf16(float f) {
  unsigned int u = __builtin_bit_cast(unsigned int, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
template <typename H> struct HalfOps;
template <> struct HalfOps<h_bf16> {
  static __device__ __forceinline__ unsigned int cvt_pk(float lo, float hi) { return ctpn_cvt_pk_bf16(lo, hi); }
  static __device__ __forceinline__ float to_f32(unsigned short h) { return ctpn_bf16_to_f32(h); }
  static __device__ __forceinline__ unsigned short from_f32(float f) { return ctpn_f32_to_bf16(f); }
  static __device__ __forceinline__ ctpn_f32x16 mfma_32x32x16(const uint4& a, const uint4& b, const ctpn_f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(ctpn_bf16x8, a), __builtin_bit_cast(ctpn_bf16x8, b), c, 0, 0, 0);
  }
};
template <> struct HalfOps<h_f16> {
  static __device__ __forceinline__ unsigned int cvt_pk(float lo, float hi) { return ctpn_cvt_pk_f16(lo, hi); }
  static __device__ __forceinline__ float to_f32(unsigned short h) { return ctpn_f16_to_f32(h); }
  static __device__ __forceinline__ unsigned short from_f32(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
  static __device__ __forceinline__ ctpn_f32x16 mfma_32x32x16(const uint4& a, const uint4& b, const ctpn_f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(ctpn_f16x8, a), __builtin_bit_cast(ctpn_f16x8, b), c, 0, 0, 0);
  }
};
// (hi, lo) bf16 pair of an fp32 value: hi = RNE(x), lo = RNE(x - hi) -- x - hi is exact in fp32, so hi + lo carries 16 mantissa
// bits (|x - hi - lo| <= 2^-17 |x|). Two values at a time: the packed converts.
__device__ __forceinline__ void ctpn_split_pk_bf16(float a, float b, unsigned int& hi, unsigned int& lo) {
  hi = ctpn_cvt_pk_bf16(a, b);
  lo = ctpn_cvt_pk_bf16(a - __builtin_bit_cast(float, hi << 16), b - __builtin_bit_cast(float, hi & 0xffff0000u));
}
#endif

void set_error(const std::string& s);
int fail(int code, const std::string& s);

#define CTPN_HIP_TRY(expr)                                                                   \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return ::ctpn::fail(CTPN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// the tail of a launcher: the error of the launch just made, if any, as "<what> launch: <HIP's text>"
inline int launch_status(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CTPN_OK : fail(CTPN_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
}

// fp32 <-> one 16-bit value on the host: RNE, a NaN stays a NaN (ctpn_get_tensor, ctpn_debug_conv3x3; the hi / lo halves of pack_conv1_frags
// and of conv_first.hip's LUT)
static inline float host_bf16_to_f32(uint16_t b) { uint32_t u = (uint32_t)b << 16; float f; std::memcpy(&f, &u, 4); return f; }
static inline float host_f16_to_f32(uint16_t b) { _Float16 h; std::memcpy(&h, &b, 2); return (float)h; }
static inline uint16_t host_f32_to_bf16(float f) {
  uint32_t u; std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline uint16_t host_f32_to_f16(float f) { const _Float16 h = (_Float16)f; uint16_t b; std::memcpy(&b, &h, 2); return b; }

// ---------------------------------------------------------------------------------------------
// Launch state is PER DEVICE: the ABI allows any number of ctxs per device (each used by one host thread at a time; distinct ctxs and the
// stateless calls may run concurrently), and one process may hold ctxs on several GPUs. The CU count and the
// "MaxDynamicSharedMemorySize already raised for this kernel" flags are indexed by the current device (a function attribute set on
// device 0 does not carry over to device 1), under one mutex, which is what two ctxs launching from two host threads meet in. `done` is one
// flag array per kernel instantiation (a function-local static of the launcher template).
// ---------------------------------------------------------------------------------------------
constexpr int CTPN_MAX_DEV = 16;
inline std::mutex& launch_state_mutex() { static std::mutex mu; return mu; }
inline int current_device(int& dev) {
  CTPN_HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= CTPN_MAX_DEV) return fail(CTPN_ERR_ARG, "device index out of range (0..15)");
  return CTPN_OK;
}
inline int device_cu_count(int dev, int& ncu) {
  static int n[CTPN_MAX_DEV] = {0};
  std::lock_guard<std::mutex> lk(launch_state_mutex());
  if (!n[dev]) {
    hipDeviceProp_t p;
    CTPN_HIP_TRY(hipGetDeviceProperties(&p, dev));
    n[dev] = p.multiProcessorCount;
  }
  ncu = n[dev];
  return CTPN_OK;
}
inline int raise_dynamic_lds(const void* kern, int bytes, bool (&done)[CTPN_MAX_DEV], int dev) {
  std::lock_guard<std::mutex> lk(launch_state_mutex());
  if (!done[dev]) {
    CTPN_HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done[dev] = true;
  }
  return CTPN_OK;
}

// ---------------------------------------------------------------------------------------------
// Implicit-GEMM descriptor (conv3x3 over a zero-bordered NHWC buffer, or a plain row-major GEMM).
//   out[m][co] = act( bias[co] + sum_{tap, ci} A(m, tap, ci) * Wt[co][tap*Ci + ci] )
// A rows: conv mode -> pixel m = (n, y, x) of an n x (H+2) x (W+2) x Ci bordered buffer, tap (ky,kx)
// reads bordered pixel (y+ky, x+kx) (so ky=kx=1 is the centre); plain mode -> A[m*lda + ci].
// ---------------------------------------------------------------------------------------------
struct IGemm {
  const void* a;        // activations (T)
  const void* wt;       // packed weights, T, [co_pad][ntaps*Ci] (co_pad multiple of the N tile, zero rows)
  const float* bias;    // fp32 [co] or nullptr
  void* out;            // OutT
  long long M;          // rows (pixels)
  int Ci;               // channels per tap (multiple of 128/sizeof(T))
  int ntaps;            // 9 (3x3) or 1
  int Co;               // valid output channels
  // A addressing
  int a_plain;          // 1: A is row-major [M][lda]
  long long lda;        // plain: elements per row
  int H, W;             // conv: un-bordered spatial size of the input == output
  int rx0, rw;          // conv: rw > 0 restricts the rows to columns [rx0, rx0 + rw) of every image row (M = N*H*rw)
  int tap_base_y, tap_base_x;  // conv, ntaps==1: which bordered tap (1,1 = centre)
  // output addressing
  int out_bordered;     // 1: write into n x (H+2) x (W+2) x ldc bordered buffer at (y+1, x+1)
  long long ldc;        // elements per output row/pixel
  int relu;
};

// SPLIT: activations / weights as (hi, lo) bf16 pairs -- per pixel [hi(C) | lo(C)], per weight row and tap [hi(Ci) | hi(Ci) | lo(Ci)]
enum class DType { F32 = 0, BF16 = 1, F16 = 2, SPLIT = 3 };
static inline int dtype_bytes(DType t) { return (t == DType::BF16 || t == DType::F16) ? 2 : 4; }      // bytes per activation element
static inline bool dtype_is_half(DType t) { return t == DType::BF16 || t == DType::F16; }

// launchers (each returns hipGetLastError()-style status through int)
int launch_igemm(const IGemm& g, DType in_t, DType out_t, hipStream_t s);
// tap-reuse 3x3 conv (conv3x3.hip); pool_out != nullptr fuses the following 2x2/2 max-pool, out may then be null
// t == SPLIT: ci / co are the layer's channels, pixels are [hi | lo] bf16 planes (output [hi | lo | hi] with dup_hi), weights from
// launch_pack_transpose_split
int launch_conv3x3(const void* in, const void* wt, const float* bias, void* out, void* pool_out, DType t, int n, int h, int w,
                   int ci, int co, int relu, hipStream_t s, int dup_hi = 0, const void* q1 = nullptr,
                   const void* q1_frags = nullptr, int split_opts = 3 /* split precision. Bit 0 (option conv_p64): Co = 64 through the persistent kernel's 64-channel form
                                                                      instead of the non-persistent kernel; bit 1 (option split_edge): ragged tile columns through the edge
                                                                      kernel instead of a padded tile column. Every precision, bit 2: a forked strip
                                                                      runs behind the main launch on s instead (two forwards overlapping freely) */,
                   int cu_count = 0 /* test launches only (ctpn_debug_conv3x3_walk): plan and walk as on a device of this many CUs, 1 .. the device's own.
                                       0 = ask the device, which is what every product caller passes */);
bool conv1_fusable(DType t, int n, int h, int w, int ci, int co, bool pool, bool keep_full);
// mfma_frags != nullptr: conv1_1 on the matrix cores with split-bf16 operands (pack_conv1_frags; fp32-class sums; SPLIT stores
// [hi(64) | lo(64)] per pixel); nullptr: the VALU kernel. (The uint8 feed of the 16-bit modes goes through the q-image instead, below.)
int launch_conv_first(const void* img, int img_is_f32, const float* w27x64, const float* bias, void* out, DType out_t,
                      int n, int h, int w, hipStream_t s, const void* mfma_frags = nullptr);
constexpr int CF_FRAG_BYTES = 12 * 64 * 16;   // [co tile 2][ky 3][hi|lo][64 lanes] x 8 bf16
constexpr int CFP_FRAG_BYTES = 6 * 64 * 16;   // conv1_1 over the q-image (conv_first_p_kernel and the producer inside conv3x3_wr_kernel): [co tile 2][ky 3][64 lanes] x 8 halves, stored behind the split fragments: a bf16 set, then an fp16 set
constexpr int CF_FRAGS_TOTAL = CF_FRAG_BYTES + 2 * CFP_FRAG_BYTES;
static inline const void* conv1_p_frags(const void* frags, DType t) { return (const char*)frags + CF_FRAG_BYTES + (t == DType::F16 ? CFP_FRAG_BYTES : 0); }
int pack_conv1_frags(const float* w27x64_dev, const float* bias_dev, uint4* frags_dev);
// ---- the q-image: the uint8 feed of the 16-bit modes as 8-byte pixels (q_B, q_G, q_R, P) of the mode's 16-bit type, q_c = p_c - round(mean_c)
// (an integer, exact in bf16 and fp16), P = 1.0; image pixel (y, x) sits at q pixel (y + 2, x + 2) of an Hq x Wq map whose other pixels are
// all-zero -- TF's SAME padding of conv1_1 AND the inside-the-image indicator its mean correction needs (conv_first_q.hip). 4.4 MB per 600 x 900
// image instead of the 69 MB of conv1_1's output: what conv1_2 reads when conv1_1 is computed inside its window stage (conv3x3_wr.h).
static inline int conv1_q_h(int h) { return ((h + 7) / 8) * 8 + 4; }
static inline int conv1_q_w(int w) { return ((w + 63) / 64) * 64 + 8; }
static inline size_t conv1_q_bytes(int n, int h, int w) { return ((size_t)n * conv1_q_h(h) * conv1_q_w(w) + 1024) * 8; }
int launch_image_to_q(const uint8_t* img, void* q, DType t, int n, int h, int w, hipStream_t s);
// conv1_1 from the q-image into the bordered NHWC map `out`, columns [xb, xe) of every image row (keep_acts; the ragged columns conv1_2's
// edge kernel reads): the same MFMA sequence on the same operands as the fused producer, so the two agree bit for bit
int launch_conv_first_from_q(const void* q, const void* frags, void* out, DType t, int n, int h, int w, int xb, int xe, hipStream_t s);
// cv2.resize(INTER_LINEAR) restated (preprocess.hip); src / dst: n x h x w x 3 and n x dh x dw x 3, uint8 or float32, device pointers
int resize_out_dim(int src, double f);
int launch_resize_linear(const void* src, void* dst, int is_f32, int n, int h, int w, int dh, int dw, double fx, double fy, hipStream_t s);
// resize_mixed.hip: the uint8 form over a TABLE of images of different sizes, each by its own factor (descriptor, work items, per-thread text:
// resize_mixed_dev.h). resize_mixed_fill writes n descriptors of RM_DESC_BYTES each with their prefix sums and returns the work items (-1:
// more than a grid holds); image i's destination rows are resize_mixed_pitch(dw[i]) bytes apart, its block dh[i] rows of them at dst_off[i]
// (a multiple of 4); inv_f[i]: 1 / f as launch_resize_linear forms it
constexpr size_t RM_DESC_BYTES = 64;
size_t resize_mixed_pitch(int dw);
long long resize_mixed_fill(void* table, int n, const int* h, const int* w, const int* dh, const int* dw, const long long* src_off, const long long* src_pitch,
                            const long long* dst_off, const double* inv_f);
int launch_resize_linear_mixed(const uint8_t* src_dev, uint8_t* dst_dev, const void* tab_dev, int n, long long total_items, hipStream_t s);
// canvas_pack.hip: the uint8 form over a table of images of different sizes, each by its own factor, into the slots of ONE ragged canvas
// n x hc x wc x 3 (descriptor, per-thread text: canvas_pack_dev.h). canvas_pack_fill writes n descriptors of CP_DESC_BYTES each: image i is
// h[i] x w[i] at src_off[i] bytes from the launch's source base, rows src_pitch[i] bytes apart, resized by f[i] (<= 0 or 1: copied) into rows
// [0, dh[i]) of slot i; the kernel writes zeros below, i.e. every byte of the canvas
constexpr size_t CP_DESC_BYTES = 40;
void canvas_pack_fill(void* table, int n, const long long* src_off, const long long* src_pitch, const int* h, const int* w, const double* f, const int* dh);
int launch_canvas_pack(const uint8_t* src_dev, uint8_t* canvas_dev, const void* tab_dev, int n, int hc, int wc, hipStream_t s);
int launch_cvt_bf16(const float* in, uint16_t* out, int n, int hw, hipStream_t s);
// the two LDS-DMA helper forms of conv3x3_base.h on `tiles` 1-KiB tiles of src (conv3x3.hip; test hook behind ctpn_debug_lds_dma)
int launch_lds_dma_check(const void* src, void* out_clobber, void* out_keep, int tiles, hipStream_t s);
int launch_pack_transpose(const float* src, long long src_ld, void* dst, long long dst_ld, DType dst_t,
                          int rows, int cols, hipStream_t s);
// split precision: src [taps * ci][cols] fp32 (TF HWIO / [in][out]) -> dst [cols][taps][hi(ci) | hi(ci) | lo(ci)] bf16
int launch_pack_transpose_split(const float* src, long long src_ld, void* dst, int taps, int ci, int cols, hipStream_t s);
// BiLSTM recurrence: xp [rows][T][1024] fp32 (fw gates 0..511 | bw gates 512..1023, TF order i,j,f,o, bias
// already added), wh [2][128][512] fp32, out [rows][T][256] fp32
// split_bf16: the recurrent product through three bf16 MFMAs on hi/lo operand halves (fp32-class accuracy, bf16 mode only)
// xp's gate columns are in the PERMUTED order lstm_gate_col() (a lane's 4 gates x 4 units contiguous), see bilstm.hip
// fast_gates: v_exp / v_rcp gate math in the exact-fp32 kernel (bf16 throughput mode)
// xp_is_f16: the pre-activations are IEEE fp16 (16-bit throughput modes), else fp32
int launch_bilstm(const void* xp, int xp_is_f16, const float* wh, float* out, int rows, int T, hipStream_t s, int split_bf16 = 0, int fast_gates = 0);
// what launch_bilstm launches for a problem, and follows: form 0 exact-fp32 MFMA with library gates, 1 the same with v_exp / v_rcp gates, 2 split-bf16
// product on 16 rows per workgroup, 3 on 4 rows per workgroup; host arithmetic only
struct BilstmPlan { int form, per_wg; };
BilstmPlan bilstm_plan(int rows, int split_bf16, int fast_gates);
// lstm_pre.hip: the LSTM input projection of the 16-bit modes (resident weight slice, fp16 out): a = bordered NHWC map of n x hf x wf cells x 512
// cu_count: the CU count the launch shape is planned for, 0 = the current device's (the product path; any other value is a test's)
int launch_lstm_pre(const void* a, const void* wt_frag, const float* bias, void* out, DType t, int n, int hf, int wf, hipStream_t s, int cu_count = 0);
// what launch_lstm_pre launches for `cells` feature-map cells on a device of ncu CUs, and follows; host arithmetic only
struct LstmPrePlan {
  int small;              // 1: lstm_pre_small_kernel (one wave per 32 cells x four column tiles), 0: lstm_pre_kernel
  int waves;              // waves per workgroup (small form: 1)
  long long workgroups;
  int idle_waves;         // whole waves of the last workgroup that lie beyond the last cell (they still take part in every barrier and DMA)
};
LstmPrePlan lstm_pre_plan(long long cells, int ncu);
int launch_lstm_pre_pack(const void* wt_x, void* wt_frag, hipStream_t s);      // [1024][512] 16-bit rows -> the kernel's fragment-major order (1 MB)
int lstm_gate_col(int c);     // TF gate column (g * 128 + u) -> permuted column, per direction
// unpack.hip: a stored activation -> dense fp32 NHWC in HBM (unpack_dev.h: the block's description and the per-thread text)
struct UnpackDesc;
int launch_unpack(const void* src, const UnpackDesc& d, float* out, hipStream_t s);
// solver.hip: the two passes of ctpn_solver_step over flat fp32 vectors (solver_dev.h: the plan, the parameters, the per-element text)
struct SvSegments;
struct SvParams;
int launch_solver_sums(const float* w, const float* g, long long count, const SvSegments& segs, double* partials, hipStream_t s);
int launch_solver_update(float* w, const float* g, float* s1, float* s2, long long count, const SvSegments& segs, const SvParams& p, hipStream_t s);
// data_layer.hip: the training data layer (data_layer_dev.h: the per-thread text). split labels: count (spans: nq DlSpan, counts: nq), scan
// (one workgroup; scan: nq + 1 ints, page_offs: pages + 1), write (total strips). train page: src -> image_out and, unless null, blob_out.
// train boxes: *bad is set where a strip holds a value outside uint16
struct DlPage;
int launch_split_count(const double* quads, int nq, const int* quad_offs, int pages, const int* dims, void* spans, uint32_t* counts, hipStream_t s);
int launch_split_scan(const uint32_t* counts, int nq, int* scan, const int* quad_offs, int pages, int* page_offs, hipStream_t s);
int launch_split_write(const void* spans, const int* scan, int nq, int total, float* strips, hipStream_t s);
int launch_train_page(const uint8_t* src, const DlPage& p, uint8_t* image_out, float* blob_out, hipStream_t s);
int launch_train_boxes(const float* strips, int n, int page_width, int flip, double scale, float* out, int* bad, hipStream_t s);
int launch_lstm_permute_rows(const void* src, void* dst, int row_bytes, hipStream_t s);
// api_weights.hip: the input projection's weight chain, the one copy ctpn_load_weights_* and ctpn_debug_lstm_pre share. kx[d]: direction d's
// [512 in][512 gates] fp32 block (kernel[:512]) with kx_ld floats per row, bias[d]: its 512 floats, all in TF's column order i | j | f | o ->
// wt_x [1024][row_bytes] rows of prec's operand type (split precision: [hi | hi | lo]) and b_x [1024], both in lstm_gate_col's order, and
// (wt_xf != nullptr: the 16-bit modes) launch_lstm_pre_pack's fragment-major copy of wt_x. Synchronises s.
int pack_lstm_projection(const float* const kx[2], long long kx_ld, const float* const bias[2], DType prec, void* wt_x, size_t row_bytes, float* b_x,
                         void* wt_xf, hipStream_t s);
// proposal pipeline, one unit per stage: decode.hip, sort_keys.hip, nms.hip (device helpers they share: proposal_dev.h)
struct ProposalCfg {
  int n, hf, wf;
  int pre_nms_topn, post_nms_topn;
  float nms_thresh, min_size;
};
// heads: [n*hf*wf][head_ld] fp32, cols 0..39 bbox deltas (a*4+{dx,dy,dw,dh}), 40..59 cls scores (a*2+{bg,fg})
int launch_decode(const float* heads, int head_ld, int heads_are_probs, const float* cls_prob_in,
                  const float* bbox_in, const float* im_info_dev, float* cls_prob_out, float* bbox_out,
                  unsigned long long* keys, float* boxes4, const ProposalCfg& c, int npad, hipStream_t s,
                  bool skip_fill = false /* the keys behind the image's anchors are not read (launch_sort_keys' segmented form) */,
                  const float* im_info_host = nullptr /* n <= 4: the rows travel in the kernel arguments and decode_kernel writes im_info_dev itself */,
                  const int* valid_rows_dev = nullptr /* ragged batch: feature rows of every image; cells below them get KEY_INVALID */);
bool sort_is_segmented(int n_img, int per_img);      // will launch_sort_keys(..., in_tmp != nullptr) take the segmented form?
int sort_seg_len(int per_img);                        // ... with segments of this many keys (the last one holds the rest); sort_keys.hip
int sort_merge_workgroups(int per_img);               // ... and this many merge_rank_kernel workgroups per image
// stable radix sort of the first per_img keys of every npad-strided segment (tmp: same size as keys)
// in_tmp != nullptr allows the segmented form for small batches; *in_tmp says which buffer holds the sorted keys afterwards
int launch_sort_keys(unsigned long long* keys, unsigned long long* tmp, int n_img, int npad, int per_img, hipStream_t s, int* in_tmp = nullptr);
// sorted_anchor (nullable): [n_img][topn] anchor index (y, x, a row-major) of every sorted row
int launch_gather_sorted(const unsigned long long* keys, const float* boxes4, float* sorted_boxes,
                         float* sorted_scores, int* sorted_anchor, int* valid_counts, int n_img, int npad,
                         int n_anchors_total, int topn, hipStream_t s,
                         unsigned char* colid = nullptr /* [n_img][(topn + 15) & ~15]: column group of every sorted box (launch_nms_columns' multi-workgroup form) */,
                         int ncols = 0);
// sorted_boxes [n_img][stride][4]; counts_in [n_img] (boxes per image, <= stride); keep idx out [n_img][keep_stride]
int launch_nms(const float* sorted_boxes, const float* sorted_scores, const int* counts_in, int stride,
               float thresh, int max_keep, int* keep_idx, int keep_stride, int* keep_counts, float* rois_out,
               float* kept_spill /* [n_img][stride][4] scratch */, int n_img, hipStream_t s,
               const int* sorted_anchor = nullptr /* [n_img][stride] */, int* roi_anchor = nullptr /* [n_img][max_keep] */);

// column-decomposed form for the proposal layer's boxes (16 px anchors on a 16 px grid): same result, see nms.hip.
// PRECONDITION (not checked by nms_columns_ok, which only looks at ncols / stride / thresh): every box lies on the 16-px anchor grid,
// x1 in [16 c, 16 c + 16) and x2 <= 16 c + 16 for its column c (/ im_scale for the connector variant) -- true for decode_kernel's output
// (bbox_transform_inv leaves x alone), NOT for arbitrary boxes: those go through launch_nms (the ctpn_nms seam always does).
// option nms_check = 1 (debug) re-runs the generic kernel after the proposal layer's column launch (api_proposals.hip) and fails loudly on a mismatch.
int launch_nms_columns(const float* sorted_boxes, const float* sorted_scores, const int* counts_in, int stride, float thresh, int max_keep,
                       int* keep_idx, int keep_stride, int* keep_counts, float* rois_out, float* kept_spill, int n_img, int ncols, hipStream_t s,
                       const int* sorted_anchor = nullptr, int* roi_anchor = nullptr,
                       const float* col_scale = nullptr /* im_info rows: the connector's boxes / im_scale variant */,
                       void* mw_scratch = nullptr /* n_img x NMS_MW_SCRATCH_BYTES, zeroed: the multi-workgroup form for small batches (one column per wave) */,
                       const unsigned char* colid = nullptr /* launch_gather_sorted's column ids (needed above 1024 candidates) */,
                       int prefix = 0 /* > 0: try the first `prefix` ranks first (they usually hold max_keep survivors); same result either way */,
                       int dbg = 0 /* option debug_nms (diagnostic, WRONG proposals): parts mask of nms_columns_kernel<16, ..> (nms.hip) */);
constexpr size_t NMS_MW_SCRATCH_BYTES = 2048;       // per image: survivor mask (one bit per rank) + ticket; zero between launches
// ... and one STICKY word the kernel sets when a column held more candidates than its list (keep lists are then wrong): zero unless a caller
// broke launch_nms_columns' precondition; read and cleared by the host (option nms_check). The block's zero state between launches is
// restored by the kernel's own epilogue; launches that share a block are serialised by stream order (proposal NMS, then connector NMS, on
// one stream per submit), and a host path that cannot vouch for an epilogue having run (an error between launches, an option change)
// marks the ctx (nms_mw_dirty) so that the next launch is preceded by a memset of the block
constexpr size_t NMS_MW_OVERFLOW_OFF = 2040;
constexpr size_t NMS_MW_FLAG_OFF = 2032;            // prefix pass: "the prefix launch did not answer" (written by every stage-1 launch before the stage-2 launch reads it)
constexpr int NMS_MW_MAX_BATCH = 4;                 // batches up to this size spread their columns over the machine; larger ones fill it with images
constexpr int NMS_MW_CAP_BATCH = 32;                // ... unless option nms_columns = 3 asks for the multi-workgroup form explicitly: buffers are sized for this many images
bool nms_columns_ok(int ncols, int stride, float thresh);
// the PAGE form of the column decomposition (nms.hip, nms_page_columns_kernel): ONE list of up to NMS_PAGE_MAXN score-sorted boxes in up to
// NMS_PAGE_MAXCOL columns int(x1) >> 4 -- a page's merged proposals (ctpn_page_nms). Partition over many workgroups, one wave per column over the
// whole chip, keep list in rank order. Same PRECONDITION as above, checked by the caller on the host (api_page.hip). Scratch, all device memory:
// list n ints, hist ncols x nms_page_units(n) words, colbase ncols + 1 words, spill n x 4 floats, alive (n + 31) / 32 words (zeroed here);
// keep: n ints, count: one int
constexpr int NMS_PAGE_MAXN = 1 << 20, NMS_PAGE_MAXCOL = 1024;
int nms_page_units(int n);
int launch_nms_page_columns(const float* sorted_boxes, int n, int ncols, float thresh, int* list, unsigned* hist, unsigned* colbase, float* spill,
                            unsigned* alive, int* keep, int* count, hipStream_t s);
// the multi-workgroup form for the proposal layer? nms_columns: the option; hf: rows of the feature map (a column holds hf x 10 candidates at most,
// the kernel's list 1024), 0 for the connector's <= 1024 boxes
static inline bool nms_multi_wg_ok(bool has_scratch, int nms_columns, int n, int hf) {
  return has_scratch && hf * 10 <= 1024 && ((nms_columns == 3 && n <= NMS_MW_CAP_BATCH) || (nms_columns == 1 && n <= NMS_MW_MAX_BATCH));
}
// prefix launches of launch_nms_columns (proposal variant): 0 = one full pass, 1 = the one-workgroup kernel tries `prefix` ranks first, 2 = a prefix
// launch and a full launch of the multi-workgroup kernel; nms.hip
int nms_prefix_launches(bool multi_wg, int prefix, int stride, int max_keep);
int nms_column_group_workgroups(int ncols);           // workgroups per image of the multi-workgroup form
constexpr int NMS_PREFIX_RANKS = 4096;                // option nms_prefix: the ranks the prefix pass looks at
int nms_prefix_ranks(int nms_prefix, int max_keep);   // ... for this post_nms_topn: NMS_PREFIX_RANKS up to 1024, 0 (no prefix pass) above; nms.hip

// What one proposal-layer call launches: computed once by enqueue_proposals (api_proposals.hip), which then follows it; host arithmetic only
// (ctpn_debug_proposal_plan hands it out). im_info: the images' rows [h, w, scale], of which the widths count (null: every image is as wide as the map).
enum { PP_SORT_ONE_WG = 0, PP_SORT_SEGMENTED = 1 };
enum { PP_NMS_GENERIC = 0, PP_NMS_ONE_WG = 1, PP_NMS_COLUMN_GROUPS = 2 };
struct ProposalPlan {
  int npad;                 // keys per image in the key buffers
  int fill_keys;            // fill_keys_kernel pads the keys behind the image's anchors (else merge_rank_kernel pads the merged buffer)
  int sort_form;            // PP_SORT_*
  int seg_len, last_seg;    // keys per sort workgroup, and of the image's last one (one workgroup: both per_img)
  int merge_wgs;            // merge_rank_kernel workgroups per image (0: no merge)
  int nms_form;             // PP_NMS_*
  int group_wgs;            // nms_column_groups_kernel workgroups per image (0 in the other forms)
  int prefix_launches;      // nms_prefix_launches
};
ProposalPlan proposal_plan(int nms_columns, int nms_prefix, bool has_mw_scratch, int n, int hf, int wf, int pre_nms_topn, int post_nms_topn,
                           float nms_thresh, const float* im_info);
int launch_hog(unsigned* sink, int n_wg, int usec, int touch, hipStream_t s, const void* src = nullptr, size_t src_bytes = 0);      // diagnostic: the one-workgroup NMS's footprint without its work (hog.hip)
bool nms_columns_tl_ok(int ncols, int stride, float thresh, float max_scale);

// The connector's configuration (reference TextLineCfg, lib/text_connector/text_connect_cfg.py:4-12), passed down to the host connector and, by
// value, to connect_kernel. Every member has the type its compiled-in counterpart had before the values became run-time parameters
// (fp32 where the reference's comparison is fp32, fp64 in filter_boxes), so the defaults compute what the constants did, bit for bit.
struct ConnectorCfg {
  float min_score;          // TEXT_PROPOSALS_MIN_SCORE
  float nms_thresh;         // TEXT_PROPOSALS_NMS_THRESH
  int max_gap;              // MAX_HORIZONTAL_GAP
  float min_v_overlaps;     // MIN_V_OVERLAPS
  float min_size_sim;       // MIN_SIZE_SIM
  double min_ratio;         // MIN_RATIO
  double line_min_score;    // LINE_MIN_SCORE
  double min_width;         // TEXT_PROPOSALS_WIDTH * MIN_NUM_PROPOSALS
};
ConnectorCfg default_connector_cfg();      // the reference's values (text_connector.cpp holds them)
// the tail's parameters by name (ctpn_set_param / ctpn_param_*), in ABI order; table, ranges and conversions in text_connector.cpp
enum { TP_RPN_PRE_NMS_TOP_N = 0, TP_RPN_POST_NMS_TOP_N, TP_RPN_NMS_THRESH, TP_RPN_MIN_SIZE, TP_MIN_SCORE, TP_NMS_THRESH, TP_MAX_GAP,
       TP_MIN_V_OVERLAPS, TP_MIN_SIZE_SIM, TP_MIN_RATIO, TP_LINE_MIN_SCORE, TP_MIN_LINE_WIDTH, TAIL_PARAM_COUNT };
struct TailParam { const char* name; double dflt, lo, hi; bool integral; };
const TailParam* tail_param(int index);                          // null outside 0 .. TAIL_PARAM_COUNT - 1
int tail_param_index(const char* name);                          // -1: unknown
bool tail_param_ok(int index, double v);                         // finite, inside the range, integral where the parameter is
void connector_cfg_set(ConnectorCfg& c, int index, double v);    // the TP_* of the connector; others are ignored
int connector_cfg_from8(const double* cfg8, ConnectorCfg& out);  // ctpn_connector_constants' order; null: the defaults
// host text connector (text_connector.cpp)
// nms: the device NMS between the sort and connect_lines where device_id >= 0 -- null: ctpn_nms; ctpn_page_text_lines passes the form it was asked for
typedef int (*TextLinesNms)(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim, float thresh, int device_id);
int text_lines_host(const float* boxes, const float* scores, int r, int im_h, int im_w, int mode,
                    int device_id, const ConnectorCfg& cfg, std::vector<double>& recs, TextLinesNms nms = nullptr);
int connect_lines(const float* kept_boxes, const float* kept_scores, int n, int im_h, int im_w, int mode,
                  const ConnectorCfg& cfg, std::vector<double>& recs);
// rois [n_img][post][5] (descending score) -> per image: boxes/scale of the score > min_score prefix + its length
constexpr int CONN_CAP = 512;   // text lines per image and mode the stateless hook ctpn_debug_connect can return (chains <= proposals / 2 = 500); a ctx: capacity / 2
// text-line connector on the device (connect.hip): recs [n_img][2 modes][cap][9] float64, counts [n_img][3] = lines H, lines O, status;
// scratch [n_img][1024][20] float64
// stride (rows per image) above 1024: the large form (connect_dev.h) -- scratch [n_img][stride][20], work: n_img x connect_work_bytes(stride) bytes of
// state, ncols: anchor columns of the images' width
int launch_connect(const float* boxes, const float* scores, const int* keep, const int* keep_counts, int stride, const float* im_info,
                   double* recs, int* counts, double* scratch, int cap, int n_img, const ConnectorCfg& cfg, hipStream_t s, char* work = nullptr, int ncols = 0);
size_t connect_work_bytes(int stride);      // 0 up to 1024 rows
// What the text-line tail launches for n images of `rows` rows each (RPN_POST_NMS_TOP_N) on a map wf columns wide: enqueue_text_lines
// (api_detect.hip) computes this once and follows it; host arithmetic only (ctpn_debug_text_line_plan hands it out)
enum { TL_NMS_GENERIC = 0, TL_NMS_ONE_WG = 1, TL_NMS_COLUMN_GROUPS = 2, TL_NMS_ONE_WG_LARGE = 3 };
enum { TL_CONN_HOST = 0, TL_CONN_ALL_PAIRS = 1, TL_CONN_BUCKETS = 2 };
struct TextLinePlan { int nms_form, conn_form, group_wgs; };
TextLinePlan text_line_plan(int nms_columns, int connect_device, bool has_mw_scratch, int n, int wf, int rows, float nms_thresh, float max_scale);
int launch_lines_prep(const float* rois, const int* roi_counts, const float* im_info, int post, float min_score,
                      float* tl_boxes, float* tl_scores, int* tl_counts, int n_img, hipStream_t s);
// host greedy NMS used by the connector when device_id < 0 (same predicate as the device kernel)
void nms_host(const float* boxes, int n, int dim, float thresh, std::vector<int>& keep);

// jpeg.hip: JPEG files, entropy decoding on the host, pixels on the device (JpegGeom: jpeg_pixel.h)
int jpeg_entropy_decode(const uint8_t* data, size_t len, int16_t* coef, size_t coef_cap, uint16_t* qt3x64, JpegGeom* g);
int launch_jpeg_pixels(const int16_t* coef_dev, const uint16_t* qt_dev, uint8_t* planes_dev, uint8_t* out_dev, const JpegGeom& g, int n, hipStream_t s);
int jpeg_probe(const uint8_t* data, size_t len, int* h, int* w, int* ncomp, int* luma_sampling);
size_t jpeg_coef_capacity(int h, int w);
// jpeg_ragged.hip: the pixel half for files of mixed sizes, into one ragged canvas (JrImage, the per-image descriptor: jpeg_ragged_dev.h)
struct JrImage;
int launch_jpeg_pixels_ragged(const int16_t* coef_dev, const uint16_t* qt_dev, uint8_t* planes_dev, uint8_t* canvas_dev, const JrImage* tab_dev, int n,
                              long long total_blocks, int hc, int wc, hipStream_t s);

// jpeg_huff.hip: the Huffman decode itself on the device (sequential files; per-thread source: jpeg_huff_dev.h). jpeg.hip prepares a file
// for it without decoding a code: jparse + one linear pass over the scan's bytes
struct JhPrep {             // one file after jparse: everything the device decode and the pixel tail need except the scan's bytes
  JpegGeom g;
  uint16_t qt[192];
  JhFile file;              // geometry part filled; offsets are the stager's
  JhTable tabs[JH_MAX_TABLES];
  int ntab = 0;
  size_t scan = 0;          // offset of the entropy-coded data in the file
  uint32_t dri = 0, total_mcus = 0, nseg = 0;      // restart interval, MCUs, segments the frame needs
  size_t coef_count = 0;
};
int jpeg_huff_prepare(const uint8_t* data, size_t len, JhPrep* out);      // CTPN_ERR_UNSUPPORTED for a progressive file
struct JhBatchDev {         // device pointers of one staged batch + its work buffers
  const JhFile* files; const JhSeg* segs; const JhTable* tabs; const uint32_t* wg_file; const uint32_t* sub_seg; const uint8_t* bytes;
  JhState* st[2]; JhState* entry; uint32_t* begun; uint32_t* prefix;
  uint32_t* changed; uint32_t* flags;      // per file: the last round that changed an exit state; the JH_FLAG_* word
  int16_t* coef;
  uint32_t S, nsub, nseg, nfiles;          // subsequence bits; subsequences (every file's padded to the workgroup size); segments; files
};
int jpeg_huff_workgroup();
int launch_jpeg_huff_round(const JhBatchDev& B, int round, hipStream_t s);
int launch_jpeg_huff_write(const JhBatchDev& B, int rounds, hipStream_t s);

// jpeg_enc.hip: BGR images -> JPEG files (quality q, 4:2:0, standard Huffman tables), pixels to quantised coefficients on the device, entropy
// coding on the host; draw_boxes_kernel = ctpn_draw_boxes on device images
struct JencQ;
void jpeg_enc_geom(int h, int w, JpegGeom& g);
void jpeg_enc_qtables(int quality, uint16_t* qt3x64, JencQ* q2x64);
size_t jpeg_encode_capacity(int h, int w);
int jpeg_entropy_encode(const int16_t* coef, bool zigzag, int h, int w, int hs, int vs, const uint16_t* qt3x64, uint8_t* out, size_t capacity, size_t* bytes_out);
int launch_jpeg_fdct(const uint8_t* img_dev, int16_t* coef_dev, const JencQ* qtab_dev, const JpegGeom& g, int n, hipStream_t s);
// ... over a table of images of different sizes and pitches (JemImage, the table's prefix sums and the work items: jpeg_enc_mixed_dev.h)
struct JemImage;
int launch_jpeg_fdct_mixed(const uint8_t* src_dev, int16_t* coef_dev, const JencQ* qtab_dev, const JemImage* tab_dev, int n, long long total_items, hipStream_t s);
int jpeg_enc_check(int h, int w, int hs, int vs, const uint16_t* qt3x64);
int jpeg_enc_assemble(int h, int w, int hs, int vs, const uint16_t* qt3x64, const uint8_t* scan, size_t have, size_t scan_bytes, uint8_t* out, size_t capacity, size_t* bytes_out);

// jpeg_huff_enc.hip: the Huffman coding itself on the device (per-thread source and the structures: jpeg_huff_enc_dev.h). One launch group:
// n images' descriptors, the batch's coefficients, and the group's per-block, per-chunk, unstuffed (cleared by the caller) and stuffed parts
struct JheImg; struct JheTables; struct JheRes;
struct JheBatchDev {
  const JheImg* imgs; const int16_t* coef; const JheTables* tables;
  uint32_t* len; uint32_t* cnt; uint32_t* uns; uint8_t* out; JheRes* res;
  int n; uint32_t max_blocks, max_chunks;      // the largest image's
};
int launch_jpeg_huff_enc(const JheBatchDev& B, bool zigzag, hipStream_t s);
int launch_draw_boxes(uint8_t* imgs_dev, const double* recs_dev, const int* counts_dev, int line_capacity, int n, int h, int w, hipStream_t s);
// ... on a ragged canvas n x hc x w x 3: image i is rows [0, heights_dev[i]) of slot i, and nothing is drawn below them
int launch_draw_boxes_ragged(uint8_t* canvas_dev, const double* recs_dev, const int* counts_dev, const int* heights_dev, int line_capacity, int n, int hc, int w, hipStream_t s);

// crop.hip: rectified crops of text lines out of device images (arithmetic: crop_pixel.h). The host fills one descriptor per line
// (crop_fill_desc: coordinates, image, width, byte offset of its crop_h x max_w x 3 block); the kernel reads the table from device memory
constexpr size_t CROP_DESC_BYTES = 80;
int crop_line_width(const double* rec9, int crop_h, int max_w);
void crop_fill_desc(const double* rec9, int img, int wc, size_t out_off, void* desc);
// heights_dev (nullable): the images are the slots of a ragged canvas n x h x w x 3 -- a line's image is rows [0, heights_dev[img]) of slot img
int launch_crop_lines(const uint8_t* imgs_dev, const void* descs_dev, int total, uint8_t* out_dev, int h, int w, const int* heights_dev, int crop_h, int max_w, int pad,
                      hipStream_t s);

// png_enc.hip: the DEFLATE block of PNG files on the device (per-piece source, the structures and the file's definition: png_enc_dev.h).
// hist: the images' symbol counts (n x 286, cleared by the caller); code: lengths, prefix sum + Adler-32, write (words cleared by the caller)
struct PngeImg; struct PngeCodes; struct PngeLen; struct PngeRes;
int launch_png_hist(const PngeImg* imgs, const uint8_t* px, uint32_t* hist, int n, uint64_t items, hipStream_t s);
int launch_png_code(const PngeImg* imgs, const uint8_t* px, const PngeCodes* codes, PngeLen* len, uint32_t* words, PngeRes* res, int n, uint64_t items, hipStream_t s);
// png.cpp: CRC-32 of the PNG chunks (the DEFLATE library's where one is loaded)
uint32_t png_crc32(const uint8_t* p, size_t n);
// png.cpp: one file read and decoded to want_h x want_w x 3 BGR bytes at bgr_out (ctpn_decode_png_files's work on one file; callable from
// any thread). A file of another size is CTPN_ERR_ARG; `why` says what failed
int png_decode_file(const char* path, uint8_t* bgr_out, size_t capacity, int want_h, int want_w, std::string& why);

// ragged.hip: a canvas batch of images of one width and different heights (RaggedMap and the per-thread bodies: ragged_dev.h).
// heights_dev: the batch's pixel heights; max_pad_rows: the most rows any image lacks at the map's level (0: no launch)
int launch_ragged_mask(void* base, const RaggedMap& m, const int* heights_dev, int n, int max_pad_rows, hipStream_t s);
int launch_ragged_blob(const uint8_t* canvas, float* blob, const int* heights_dev, int n, int hc, int w, hipStream_t s);

// page.hip: tiles of a page larger than the network input, cut at native resolution (the plan's arithmetic, PgTile and the per-thread text:
// page_dev.h). tiles_dev: n records in device memory; out_dev: n x tile_h x tile_w x 3 bytes, 4-byte aligned, every one of them written
struct PgTile;
int launch_page_cut(const uint8_t* page_dev, long long pitch, const PgTile* tiles_dev, int n, int tile_h, int tile_w, uint8_t* out_dev, hipStream_t s);

// targets.hip: the label side of training (the per-thread text, TgCfg and the sizes: targets_dev.h). Every pointer is device memory.
//   launch_bbox_overlaps   out[n][k] = tg_overlap(boxes[i], query[j]) of lib/utils/bbox.pyx, both forms
//   launch_anchor_targets  anchor_target_layer for n images on one hf x wf map. im_info [n][3]; gt [total][5] with offs [n + 1]; hard [total] or
//                          null; dc [totalD][4] with dc_offs [n + 1], or null; scratch: colmax [max(total, 1)] (zeroed by the caller),
//                          hardfirst [max(total, 1)] (filled with 0x7f bytes by the caller), flags [n * A] bytes; stats [n][6]; presample nullable; max_overlap and
//                          argmax are the hand-over between the two passes and always given
//   launch_rpn_loss        losses [n][3], counts [n][2], d_heads nullable
struct TgCfg;
int launch_bbox_overlaps(const double* boxes, int n, const double* query, int k, double* out, int intersections, hipStream_t s);
int launch_anchor_targets(int n, int hf, int wf, const float* im_info, const float* gt, const int* offs, int max_g, const int* hard, const float* dc,
                          const int* dc_offs, const TgCfg& cfg, unsigned long long seed, unsigned long long* colmax, int* hardfirst, uint8_t* flags,
                          float* labels, float* targets, float* inside_w, float* outside_w, int* stats, float* presample, double* max_overlap, int* argmax,
                          hipStream_t s);
int launch_rpn_loss(int n, int hf, int wf, const float* heads, int ld, const float* labels, const float* targets, const float* inside_w,
                    const float* outside_w, double* losses, int* counts, float* d_heads, hipStream_t s);

// the backward pass through the recurrent tail (tail_grad.hip; the per-thread text, the saved block and the d_tail offsets: tail_grad_dev.h).
// Every pointer is device memory; `tail` is the arena's last ten tensors in TF's layout.
//   launch_bilstm_save  bilstm.hip: launch_bilstm's exact-gate fp32 form, which also fills gates [rows * T][2][5][128]
//   launch_bptt         d_pre [rows * T][1024] (TF column order, fw | bw) from d_lstm_out [rows * T][256] and the saved gates
//   launch_tail_tn      out [K][ldo] (N columns) = A^T dY over M cells in blocks of tb_block_cells(M); parts: scratch of partials x K x N floats;
//                       shift -1 / +1: A's row is the cell one step before / after in its sequence of T, zero at the sequence's end
//   launch_tail_colsum  out [N] = column sums of dY in the same block order; parts: partials x N floats
//   launch_mask_dheads  out [M][64] = d_heads with columns 60..63 cleared; launch_heads_rows: out [512][64] = bbox | cls | 0 rows
int launch_bilstm_save(const float* xp, const float* wh, float* out, float* gates, int rows, int T, hipStream_t s);
int launch_bptt(const float* d_lstm_out, const float* gates, const float* tail, float* d_pre, int rows, int T, hipStream_t s);
int launch_tail_tn(const float* a, int lda, int shift, const float* dy, int ldy, long long M, int T, int K, int N, float* parts, float* out, int ldo, hipStream_t s);
int launch_tail_colsum(const float* dy, int ldy, long long M, int N, float* parts, float* out, hipStream_t s);
int launch_mask_dheads(const float* d_heads, float* out, long long M, hipStream_t s);
int launch_heads_rows(const float* tail, float* out, hipStream_t s);

// the backward pass through one conv + bias + ReLU and through the 2x2 max-pool (conv_grad.hip; the per-thread text and the block plan:
// conv_grad_dev.h). Every pointer is device memory, plain dense fp32: activations [M = n h w][channels], w [9][ci][co].
//   launch_conv_grad_mask  dz = d_y (y > 0)
//   launch_conv_grad_dx    dx [M][ci] from dz and w; ci a multiple of 32
//   launch_conv_grad_dw    d_w [9][ci][co] and d_b [co] from x and dz in cg_plan's blocks; parts: blocks x 9 ci co floats, bparts: blocks x co
//   launch_pool_grad       d_full [n][h][w][c] from the full map y and d_pool [n][h / 2][w / 2][c]
int launch_conv_grad_mask(const float* d_y, const float* y, float* dz, long long M, int co, hipStream_t s);
int launch_conv_grad_dx(const float* dz, const float* wt, int h, int w, int ci, int co, long long M, float* dx, hipStream_t s);
int launch_conv_grad_dw(const float* x, const float* dz, int h, int w, int ci, int co, long long M, float* parts, float* bparts, float* d_w, float* d_b, hipStream_t s);
int launch_pool_grad(const float* y, const float* d_pool, int n, int h, int w, int c, float* d_full, hipStream_t s);

static inline int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

}  // namespace ctpn
