// 3x3 convolution with tap reuse out of LDS (the VGG trunk + rpn_conv/3x3), bias + ReLU (+ 2x2 max-pool) fused -- what the kernel families
// share: the scheme and the split-precision layout (below), vector types, the MFMA / wait / barrier / LDS-DMA helpers, the launch argument
// Conv3 and the tiling helpers. The kernels and their launch templates: conv3x3_tiled.h (conv3x3_kernel), conv3x3_persistent.h
// (conv3x3_p_kernel), conv3x3_wr.h (conv3x3_wr_kernel: weights in registers), conv3x3_edge.h (conv3x3_edge_kernel: ragged columns);
// conv3x3_dispatch.h picks the family of a layer. One translation unit per arithmetic type (conv3x3_f32.hip, conv3x3_bf16.hip,
// conv3x3_f16.hip, conv3x3_split.hip: they compile in parallel) includes the families it instantiates; conv3x3.hip (launch_conv3x3:
// layer-level decisions) includes this header only.
//
// Replaces tf.nn.conv2d + bias_add + relu of Network.conv (reference lib/networks/network.py:160-183) and, when POOL,
// the Network.max_pool that follows it (network.py:189-196; VGGnet_test.py:23,26,30,34).
//
// igemm.hip treats the conv as im2col GEMM and therefore moves every input pixel L2 -> LDS nine times (once per
// tap): at a 128x128 tile that is 64 B/clk/CU, i.e. 39 TB/s at MFMA peak -- above what the L2s deliver -- and it is
// why that kernel sits at ~28 % of the bf16 roofline. Here a workgroup owns 256 output pixels x BN channels and, per
// 64-channel chunk (one 128-byte strip per pixel), stages the INPUT window those pixels need ONCE into LDS; the nine
// taps are nine shifted views of that window (LDS row + ky*pitch + kx), so only the weight strip changes per K step:
//     2D mode   : window = (8+2) x (32+2) pixel patch of one image (any W; needed for the 2x2 pool fusion)
//     flat mode : window = 256 + 2*(W+2) + 2 CONSECUTIVE pixels of the bordered NHWC buffer (M runs over bordered
//                 positions, border outputs are computed and dropped) -- no tile quantisation on the small
//                 75x112 / 37x56 maps, perfectly contiguous staging
// L2 -> LDS traffic drops ~3x (20 B/clk/CU at BN = 128). Everything else follows igemm.hip: 128-byte rows with the
// 16-byte slot XOR-swizzled by (row>>1)&7 (source side for global_load_lds, read side for ds_read_b128: conflict-free
// for ANY 32 consecutive rows, tests/test_layouts.py), swapped MFMA operand roles (weights = A rows) so a lane owns
// 4 consecutive channels of one pixel, epilogue through LDS with 16 B/lane stores, XCD-contiguous block order.
//
// Arithmetic types (template parameter T): float (exact-fp32 MFMA 32x32x2), h_bf16, h_f16 (32x32x16, common.h).
// SPLIT (CTPN_PREC_SPLIT; T = h_bf16): every activation and weight is a (hi, lo) pair of bf16 and a product is three MFMAs,
//     x w ~= x_hi w_hi + x_lo w_hi + x_hi w_lo      (fp32 accumulate; the dropped x_lo w_lo is ~2^-17 of the product)
// laid out so that the K loop does not change at all: a pixel of a C-channel map is [hi(C) | lo(C)] (2 C bf16), a weight row is
// [w_hi(Ci) | w_hi(Ci) | w_lo(Ci)] per tap, and the kernel runs a plain bf16 convolution over K = 9 x 3 Ci whose 64-channel input
// chunk c is chunk (c < 2 Ci / 64 ? c : c - 2 Ci / 64) of the pixel (`a_wrap`: the third K block re-reads the hi plane -- from LDS-DMA's
// point of view just another chunk of the same pixel, served by L2). Only the epilogue differs: ReLU in fp32, then
// hi = RNE_bf16(v), lo = RNE_bf16(v - hi) into the two planes (and, for the layer that feeds the LSTM projection GEMM, hi once more:
// [hi | lo | hi], so that GEMM is a plain K = 3 C product as well).
#pragma once
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <utility>

#include "common.h"
#include "conv3x3_plan.h"

namespace ctpn {

typedef ctpn_f32x16 c3_f32x16;
typedef __attribute__((ext_vector_type(4))) float c3_f32x4;
typedef uint32_t c3_u32x4 __attribute__((ext_vector_type(4)));   // native vector: inline-asm register operands ("v", tied "+v") need one

template <typename T>
__device__ __forceinline__ void c3_mfma(c3_f32x16& acc, const uint4& w, const uint4& x) {
  if constexpr (std::is_same<T, float>::value) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(float, w.x), __builtin_bit_cast(float, x.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(float, w.y), __builtin_bit_cast(float, x.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(float, w.z), __builtin_bit_cast(float, x.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(float, w.w), __builtin_bit_cast(float, x.w), acc, 0, 0, 0);
  } else {
    acc = HalfOps<T>::mfma_32x32x16(w, x, acc);
  }
}
// two fp32 -> one packed pair of the 16-bit output type
template <typename OutT>
__device__ __forceinline__ uint32_t c3_cvt_pk(float lo, float hi) { return HalfOps<OutT>::cvt_pk(lo, hi); }

template <int N>
__device__ __forceinline__ void c3_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Raw s_barrier. It orders NOTHING by itself on gfx950: no vmcnt, no lgkmcnt wait is implied, and hipcc moves register-only work (MFMAs and
// the s_waitcnt for their LDS operands) across it freely. Every buffer hand-over in these kernels therefore states both waits explicitly in
// front of it: `s_waitcnt lgkmcnt(0)` (my LDS reads of the buffer the next LDS-DMA recycles have executed) and the counted vmcnt (my DMA
// pieces of the buffer the next step reads have landed). tools/scan_barrier_reads.py checks the compiled code for LDS reads in flight
// across a barrier.
__device__ __forceinline__ void c3_barrier() { __builtin_amdgcn_s_barrier(); }

// LDS-DMA issued from inline asm: hipcc does not count it, so it neither drains it with vmcnt(0) at the next
// barrier / ds_read nor waits for it at all -- every wait is the kernel's own counted s_waitcnt (cdna guide 5.7).
// lds_dst: wave-uniform LDS byte address (the hardware adds lane * 16); gsrc: this lane's 16 source bytes.
__device__ __forceinline__ void c3_glds16_asm(const void* gsrc, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}

// LDS-DMA, scalar base + per-lane 32-bit offset: lds_dst is the wave-uniform LDS byte address (hardware adds lane * 16)
// (m0 is declared clobbered instead of being saved and restored around every piece: two SALU fewer per KiB in the K loops)
// clang warns about every reserved register on a clobber list (-Winline-asm: "may not be preserved across the asm statement"). That is the
// contract wanted here: nothing else in these kernels keeps a value in m0 across the statement (the compiler's own LDS-DMA / ds_*_addtid /
// s_movrel uses would; there are none, and tests/test_gpu_round6.py::test_lds_dma_helper_forms_agree compares this form with the
// save / restore form c3_glds16_asm tile for tile on the device, so a compiler that starts to keep state in m0 is caught). The
// diagnostic is silenced for THIS statement only; the build fails on any other warning (__graft_entry__.build()).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void c3_glds16_saddr(const void* sbase, uint32_t voff, uint32_t lds_dst) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %2" : : "v"(voff), "s"(lds_dst), "s"(sbase) : "memory", "m0");
}
#pragma clang diagnostic pop

// LDS fragment read issued from inline asm (cdna guide 5.7 form iii): program order is pinned by `volatile`, completion
// is the kernel's own counted s_waitcnt lgkmcnt + sched_barrier(0) in front of the first consumer.
__device__ __forceinline__ void c3_ds_read_b128_asm(uint4& dst, uint32_t lds_addr) {
  asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(lds_addr));
}
template <int N>
__device__ __forceinline__ void c3_wait_lgkm() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

template <typename OutT>
__device__ __forceinline__ uint4 c3_max4(const uint4& a, const uint4& b) {
  uint4 r;
  if constexpr (sizeof(OutT) == 4) {
    r.x = __builtin_bit_cast(uint32_t, fmaxf(__builtin_bit_cast(float, a.x), __builtin_bit_cast(float, b.x)));
    r.y = __builtin_bit_cast(uint32_t, fmaxf(__builtin_bit_cast(float, a.y), __builtin_bit_cast(float, b.y)));
    r.z = __builtin_bit_cast(uint32_t, fmaxf(__builtin_bit_cast(float, a.z), __builtin_bit_cast(float, b.z)));
    r.w = __builtin_bit_cast(uint32_t, fmaxf(__builtin_bit_cast(float, a.w), __builtin_bit_cast(float, b.w)));
  } else {
    auto mx = [](uint32_t p, uint32_t q) -> uint32_t {
      const uint32_t lo = (HalfOps<OutT>::to_f32((uint16_t)p) >= HalfOps<OutT>::to_f32((uint16_t)q)) ? (p & 0xffffu) : (q & 0xffffu);
      const uint32_t hi = (HalfOps<OutT>::to_f32((uint16_t)(p >> 16)) >= HalfOps<OutT>::to_f32((uint16_t)(q >> 16))) ? (p & 0xffff0000u) : (q & 0xffff0000u);
      return lo | hi;
    };
    r.x = mx(a.x, b.x); r.y = mx(a.y, b.y); r.z = mx(a.z, b.z); r.w = mx(a.w, b.w);
  }
  return r;
}

// SPLIT epilogues: four fp32 values (ReLU already applied) of channels co .. co + 3 of one pixel -> the hi and lo planes ([hi | lo | hi] with dup)
__device__ __forceinline__ void c3_split_store4(char* pix_base, int co, const uint4& v, int Co, int dup) {
  uint2 hi, lo;
  ctpn_split_pk_bf16(__builtin_bit_cast(float, v.x), __builtin_bit_cast(float, v.y), hi.x, lo.x);
  ctpn_split_pk_bf16(__builtin_bit_cast(float, v.z), __builtin_bit_cast(float, v.w), hi.y, lo.y);
  *(uint2*)(pix_base + co * 2) = hi;
  *(uint2*)(pix_base + (Co + co) * 2) = lo;
  if (dup) *(uint2*)(pix_base + (2 * Co + co) * 2) = hi;
}

struct Conv3 {
  const void* in;      // bordered NHWC, T
  const void* wt;      // [co_pad][9*Ci] T
  const float* bias;
  void* out;           // bordered NHWC, OutT (may be null when POOL and the full-resolution output is not kept)
  void* pool_out;      // bordered NHWC of the pooled map (POOL only)
  int N, H, W, Ci, Co, relu;
  int tiles_x, tiles_y;       // 2D mode
  long long m_total;          // flat mode: N*(H+2)*(W+2)
  int a_rows;                 // LDS rows of one A window (multiple of 8)
  long long ptiles_total;     // persistent kernel: pixel tiles x tiles_n
  int w_cover;                // 2D mode: columns [0, w_cover) are this launch's (0 = all W); the rest belongs to a strip launch
  int abl;                    // persistent kernel, timing only and only in -DCTPN_ABLATION builds (`make ablation`; CTPN_C3_P_ABL): 1 = skip the epilogue,
                              // 2 = its arithmetic without the stores (WRONG results; the product library ignores the field)
  int tiles_n;
  // persistent kernel, flat windows: half-tile tail (see conv3x3_p_kernel). Tiles [0, ht_full) are walked whole; the ht_r tiles behind them
  // are split into two halves of 128 consecutive pixels: 2 * ht_r work items for the first 2 * ht_r workers of the tail round. 0: no split.
  long long ht_full;
  int ht_r;
  // persistent kernel, 2D patches without a fused pool: tile rows run over the bordered rows of the WHOLE batch (tiles_y counts them)
  // instead of per image -- see c3_launch_p
  int stacked;
  // SPLIT kernels (see the file comment): Ci above is the K width per tap (3 x the layer's input channels); in_pitch = bf16 elements per
  // input pixel (2 x), a_wrap = first 64-channel K chunk that re-reads the hi plane (chunk c -> pixel chunk c - a_wrap), out_pitch = bf16
  // elements per output pixel (2 Co, or 3 Co with dup_hi: [hi | lo | hi]). Non-split launches: in_pitch = Ci, out_pitch = Co.
  int in_pitch, a_wrap, out_pitch, dup_hi;
  int opt_ahead;              // unused since round 6 (every persistent form reads ahead); kept so that the kernel-argument layout does not move
  int unused_[2];             // two former tuning options; what they chose is the plan's now (conv3x3_plan.h, which the launchers follow: no kernel and no
                              // launcher reads a choice from this struct). Kept, like opt_ahead, so that the kernel-argument layout does not move
  // conv1_2 with conv1_1 computed in its window stage (conv3x3_wr_kernel FUSE): the batch's q-image and conv1_1's fragments; `in` is unused
  const void* q1; const void* q1_frags;
};

// 16 x 16 patches: a 32-pixel MFMA tile is two patch rows of 16. Lanes 16..31 take the second row ROTATED by two columns
// (lane 16 + k owns column (k + 14) & 15): with the 18-pixel LDS row pitch that makes the LDS row of lane l congruent to l
// mod 16 again, which is what keeps every ds_read_b128 lane group on 16 distinct bank quads (un-rotated: 1.3-1.45 x the
// busy cycles in SQ_LDS_BANK_CONFLICT on the conv4 layers).
__device__ __forceinline__ int c3_tw16_col(int l31) { return (l31 & 16) ? ((l31 - 2) & 15) : l31; }

// the tiling helpers of conv3x3_plan.h on a launch argument (the plan and the launchers count the same tiles)
static inline void c3_extent(const Conv3& g, bool pool, int& he, int& we) { c3_extent_of(g.H, g.W, pool, g.out != nullptr, g.w_cover, he, we); }

// ---- per-type entry points: one translation unit each (conv3x3_<type>.hip), called by launch_conv3x3 (conv3x3.hip) ----
// (form: the plan's main_form, C3Main; ks: the plan's edge_ks; ncu: the CU count the plan was made for -- the walk, c3_walk, takes the same)
int c3_run_f32(const Conv3& g, bool pool, int form, hipStream_t s, int ncu);          // exact-fp32 MFMA kernels
int c3_run_bf16(const Conv3& g, bool pool, int form, hipStream_t s, int ncu);         // C3M_WR: the weights-in-registers kernel (Ci = 64)
int c3_run_f16(const Conv3& g, bool pool, int form, hipStream_t s, int ncu);
int c3_run_split(const Conv3& g, bool pool, int form, hipStream_t s, int ncu);        // (hi, lo) bf16 planes, three MFMA terms
int c3_edge_bf16(const void* in, const void* wt, const float* bias, void* out, int n, int h, int w, int ci, int co, int relu, int r, bool pooled, hipStream_t s, bool deep);
int c3_edge_f16(const void* in, const void* wt, const float* bias, void* out, int n, int h, int w, int ci, int co, int relu, int r, bool pooled, hipStream_t s, bool deep);
int c3_edge_split(const void* in, const void* wt, const float* bias, void* out, int n, int h, int w, int ci, int co, int relu, int r, bool pooled, hipStream_t s, bool deep, int dup_hi, int ks);

}  // namespace ctpn
