// conv3x3_edge_kernel (ragged right-edge columns of a 2D-tiled layer) and its launch template c3_launch_edge; shared helpers: conv3x3_base.h
#pragma once
#include "conv3x3_base.h"
namespace ctpn {

// ---------------------------------------------------------------------------------------------
// Ragged right edge of a 2D-tiled layer (bf16): the one or two pixel columns left of W after the largest multiple of the
// tile width (W = 225 = 7 * 32 + 1, 450 = 14 * 32 + 2, 113 = 7 * 16 + 1). A padded tile column for them would cost the layer
// 1/8 (W = 113, 225) of its tile work; the im2col GEMM (igemm.hip, 64 KB of LDS) cannot share a CU with the persistent
// workgroups (135 - 147 KB of LDS, 432 of a SIMD's 512 registers), so it only got CUs when the layer was over and
// finished 20 - 40 us after it. This kernel is made to fit in what the persistent kernels leave free: ONE wave per
// workgroup, NO LDS, <= 80 registers; the MFMA operands come straight from global memory (the [co][tap][ci] weights and the
// bordered NHWC input both have the K index contiguous, which is the 32x32x16 operand layout: lane = row, 16 bytes = 8 k).
// One wave = 32 edge pixels x 64 channels; latency-bound by design, it has the whole duration of the main launch.
// ---------------------------------------------------------------------------------------------
struct ConvEdge {
  const void* in; const void* wt; const float* bias; void* out;
  int H, W, Ci, Co, rx0, rw, relu;
  int in_pitch, out_pitch, dup_hi;   // 16-bit elements per input / output pixel (Ci / Co; split precision: 2 Ci / 2 Co or 3 Co with dup_hi)
  long long M;                 // plain: N * H * rw edge pixels, m = (n * H + y) * rw + xs
                               // pooled: N * (H / 2) * (rw / 2) POOLED edge pixels, m = (n * Ho + Y) * (rw / 2) + X; out = the pooled map
};

// POOL: the layer's fused 2x2 / 2 VALID max-pool on the edge columns (conv1_2: W = 900 = 28 * 32 + 4, conv2_2: 450 = 28 * 16 + 2 --
// an even number of edge columns starting at an even x, so the pooled pixels lie entirely inside the edge). A wave then holds
// 8 pooled pixels x their four conv pixels (lane quad = one pooled pixel: dy = bit 1, dx = bit 0 of the lane); the pool is a max
// over the quad with two DPP moves per value, and max commutes with the bias (in the sums), the ReLU and the bf16 rounding.
// DEEP (one or two images: the main launch leaves most of the machine empty and the edge kernel runs IN the layer's stream, behind the main
// launch, instead of on a forked stream -- a fork / join pair costs 12 - 19 us of cross-queue signalling per layer, 85 us of a lone image's
// millisecond): the K steps in rounds of four with three rounds in flight (36 sixteen-byte loads per lane) instead of one round of two; the
// kernel is a chain of load round trips (0.6 - 1 us each on an idle part), and a round trip now feeds 24 MFMAs instead of 4. The MFMAs are
// issued in the SAME order on the same operands: the two forms agree bit for bit, which is what lets the batch size choose between them.
// SPLIT (round 6): pixels are [hi | lo] bf16 planes, weight rows [hi | hi | lo] per tap (pack_split_kernel): three K blocks per tap --
// x_hi w_hi, x_lo w_hi, x_hi w_lo -- through the same loop (block b reads input plane b & 1 and weight block b); ReLU in fp32, then the (hi, lo)
// pair of every output (plus the hi plane once more for the layer that feeds the LSTM projection). Until round 6 split precision computed a
// padded tile column instead: an eighth of conv4_1 / conv4_2, a fifteenth of conv3_1 / conv3_2.
// KS > 1 (split precision, always): KS waves per workgroup share one 32-pixel x 64-channel tile, wave w sums K steps [w S / KS, (w + 1) S / KS)
// (deep form), waves 1 .. KS - 1 hand their partial sums to wave 0 through LDS, which adds them in wave order -- a fixed order, chosen by the
// layer's Ci alone (c3_launch_edge), so a batch and its images run alone still agree bit for bit. The split form runs in its layer's stream,
// behind the main launch. For ONE image it is a handful of workgroups, each a chain of load round trips: 432 K steps = 36 round trips for
// conv3_2, 6 with the K split -- the lone-image call in split precision 1.84 -> 1.7 ms. At batch 32 the kernel is bound by the request rate of
// its fragment loads (64 cache lines per KB of operands) and the split changes nothing (119 / 58 / 122 / 68 / 131 us per layer against
// 137 / 55 / 111 / 61 / 122).
template <typename H, bool POOL, bool DEEP = false, bool SPLIT = false, int KS = 1>
__global__ __launch_bounds__(64 * KS, DEEP ? 2 : 6) void conv3x3_edge_kernel(ConvEdge g) {
  static_assert(KS == 1 || (DEEP && SPLIT), "the K-split form is the split-precision deep form");
  constexpr int NB = SPLIT ? 3 : 1;
  const int lane = threadIdx.x & 63, l31 = lane & 31, fhalf = lane >> 5;
  const int kw = KS > 1 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
  const int ntn = g.Co >> 6;
  const int tn = blockIdx.x % ntn;
  const unsigned tm = blockIdx.x / ntn;
  const int Wp = g.W + 2, Hp = g.H + 2, Ci = g.Ci;
  long long pix, opix;                                       // bordered input position of tap (0, 0); bordered output pixel
  bool mok;
  if constexpr (POOL) {
    const int Ho = g.H >> 1, Wo = g.W >> 1, rw2 = g.rw >> 1;
    unsigned m = tm * 8u + (unsigned)(l31 >> 2);             // pooled pixel of this lane's quad
    mok = m < (unsigned)g.M;
    if (!mok) m = (unsigned)g.M - 1u;
    const int X = (int)(m % (unsigned)rw2);
    const unsigned t = m / (unsigned)rw2;
    const int Y = (int)(t % (unsigned)Ho), n = (int)(t / (unsigned)Ho);
    const int y = 2 * Y + ((l31 >> 1) & 1), x = g.rx0 + 2 * X + (l31 & 1);
    pix = ((long long)n * Hp + y) * Wp + x;
    opix = ((long long)n * (Ho + 2) + Y + 1) * (Wo + 2) + (g.rx0 >> 1) + X + 1;
    mok = mok && (l31 & 3) == 0;                             // one lane of the quad stores
  } else {
    unsigned m = tm * 32u + (unsigned)l31;                   // M < 2^31 (launcher)
    mok = m < (unsigned)g.M;
    if (!mok) m = (unsigned)g.M - 1u;
    const int xs = (int)(m % (unsigned)g.rw);
    const unsigned t = m / (unsigned)g.rw;
    const int y = (int)(t % (unsigned)g.H), n = (int)(t / (unsigned)g.H);
    pix = ((long long)n * Hp + y) * Wp + g.rx0 + xs;
    opix = pix + Wp + 1;
  }
  const long long ipb = (long long)g.in_pitch * 2;          // bytes per input pixel
  const char* ip = (const char*)g.in + pix * ipb + fhalf * 16;
  const int co0 = tn * 64;
  const long long wrow = (long long)9 * NB * Ci * 2;
  const char* wp0 = (const char*)g.wt + (co0 + l31) * wrow + fhalf * 16;
  const char* wp1 = wp0 + 32 * wrow;
  c3_f32x16 acc0, acc1;
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {                          // the bias is the accumulators' initial value (K-split: wave 0's)
    float4 b0 = *(const float4*)(g.bias + co0 + 8 * g4 + 4 * fhalf), b1 = *(const float4*)(g.bias + co0 + 32 + 8 * g4 + 4 * fhalf);
    if (KS > 1 && kw != 0) { b0 = make_float4(0.f, 0.f, 0.f, 0.f); b1 = b0; }
    acc0[4 * g4] = b0.x; acc0[4 * g4 + 1] = b0.y; acc0[4 * g4 + 2] = b0.z; acc0[4 * g4 + 3] = b0.w;
    acc1[4 * g4] = b1.x; acc1[4 * g4 + 1] = b1.y; acc1[4 * g4 + 2] = b1.z; acc1[4 * g4 + 3] = b1.w;
  }
  const int kc_n = Ci >> 4;                                 // 16-element K steps per tap (Ci is a multiple of 64)
  if constexpr (DEEP) {
    // The 9 kc_n K steps (tap-major, the order of the loop below) in rounds of four, THREE rounds in flight: round r + 2 is requested
    // before round r's eight MFMAs are issued, so the chain is one load round trip per three rounds instead of one per round.
    constexpr int R = 4;
    const int S = 9 * NB * kc_n;                             // a multiple of 4
    c3_u32x4 xs0[R], fa0[R], fb0[R], xs1[R], fa1[R], fb1[R], xs2[R], fa2[R], fb2[R];
    auto issue = [&](c3_u32x4 (&xs)[R], c3_u32x4 (&fa)[R], c3_u32x4 (&fb)[R], int j0) {
      const int tb = j0 / kc_n, kc = j0 - tb * kc_n;        // a round never straddles two taps / K blocks: kc_n is a multiple of R
      const int tap = tb / NB, b = tb - tap * NB;
      const int ky = tap / 3, kx = tap - 3 * ky;
      const char* a = ip + (long long)(ky * Wp + kx) * ipb + (b & 1) * Ci * 2 + kc * 32;
      const char* w0 = wp0 + (long long)tb * Ci * 2 + kc * 32;
      const char* w1 = wp1 + (long long)tb * Ci * 2 + kc * 32;
#pragma unroll
      for (int q = 0; q < R; ++q) { xs[q] = *(const c3_u32x4*)(a + q * 32); fa[q] = *(const c3_u32x4*)(w0 + q * 32); fb[q] = *(const c3_u32x4*)(w1 + q * 32); }
    };
    auto mma = [&](const c3_u32x4 (&xs)[R], const c3_u32x4 (&fa)[R], const c3_u32x4 (&fb)[R]) {
#pragma unroll
      for (int q = 0; q < R; ++q) {
        acc0 = HalfOps<H>::mfma_32x32x16(__builtin_bit_cast(uint4, fa[q]), __builtin_bit_cast(uint4, xs[q]), acc0);
        acc1 = HalfOps<H>::mfma_32x32x16(__builtin_bit_cast(uint4, fb[q]), __builtin_bit_cast(uint4, xs[q]), acc1);
      }
    };
    const int jb = kw * (S / KS), je = jb + S / KS;          // this wave's K steps: S / KS is a multiple of 4 (launcher), >= 36
    issue(xs0, fa0, fb0, jb);
    issue(xs1, fa1, fb1, jb + R);
#pragma unroll 1
    for (int j = jb; j < je; j += 3 * R) {
      if (j + 2 * R < je) issue(xs2, fa2, fb2, j + 2 * R);
      mma(xs0, fa0, fb0);
      if (j + 3 * R < je) issue(xs0, fa0, fb0, j + 3 * R);
      if (j + R < je) mma(xs1, fa1, fb1);
      if (j + 4 * R < je) issue(xs1, fa1, fb1, j + 4 * R);
      if (j + 2 * R < je) mma(xs2, fa2, fb2);
    }
    if constexpr (KS > 1) {
      __shared__ float red[KS - 1][32][64];                 // [wave][accumulator register][lane]: conflict-free 256-byte rows
      if (kw != 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) { red[kw - 1][e][lane] = acc0[e]; red[kw - 1][16 + e][lane] = acc1[e]; }
      }
      __syncthreads();
      if (kw != 0) return;
#pragma unroll 1
      for (int w = 0; w < KS - 1; ++w) {
#pragma unroll
        for (int e = 0; e < 16; ++e) { acc0[e] += red[w][e][lane]; acc1[e] += red[w][16 + e][lane]; }
      }
    }
  } else {
#pragma unroll 1
  for (int tb = 0; tb < 9 * NB; ++tb) {
    const int tap = tb / NB, b = tb - tap * NB;
    const int ky = tap / 3, kx = tap - 3 * ky;
    const char* a = ip + (long long)(ky * Wp + kx) * ipb + (b & 1) * Ci * 2;
    const char* w0 = wp0 + (long long)tb * Ci * 2;
    const char* w1 = wp1 + (long long)tb * Ci * 2;
#pragma unroll 1
    for (int kc = 0; kc < kc_n; kc += 2) {                  // two K steps per round: six 16-byte loads in flight per lane
      const c3_u32x4 x = *(const c3_u32x4*)(a + kc * 32), x2 = *(const c3_u32x4*)(a + kc * 32 + 32);
      const c3_u32x4 f0 = *(const c3_u32x4*)(w0 + kc * 32), f2 = *(const c3_u32x4*)(w0 + kc * 32 + 32);
      const c3_u32x4 f1 = *(const c3_u32x4*)(w1 + kc * 32), f3 = *(const c3_u32x4*)(w1 + kc * 32 + 32);
      acc0 = HalfOps<H>::mfma_32x32x16(__builtin_bit_cast(uint4, f0), __builtin_bit_cast(uint4, x), acc0);
      acc1 = HalfOps<H>::mfma_32x32x16(__builtin_bit_cast(uint4, f1), __builtin_bit_cast(uint4, x), acc1);
      acc0 = HalfOps<H>::mfma_32x32x16(__builtin_bit_cast(uint4, f2), __builtin_bit_cast(uint4, x2), acc0);
      acc1 = HalfOps<H>::mfma_32x32x16(__builtin_bit_cast(uint4, f3), __builtin_bit_cast(uint4, x2), acc1);
    }
  }
  }
  if constexpr (POOL) {
    // quad max BEFORE any lane leaves: lane ^ 1 (quad_perm [1,0,3,2] = 0xB1), then lane ^ 2 ([2,3,0,1] = 0x4E). The moved values are
    // pinned with an empty asm: cross-lane results that only feed an exec-masked store are otherwise sunk into the masked block
    auto qmax = [](float v) -> float {
      float a = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
      asm volatile("" : "+v"(a));
      v = __builtin_fmaxf(v, a);
      float b = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
      asm volatile("" : "+v"(b));
      return __builtin_fmaxf(v, b);
    };
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc0[e] = qmax(acc0[e]); acc1[e] = qmax(acc1[e]); }
  }
  if (!mok) return;
  char* op = (char*)g.out + (opix * g.out_pitch + co0 + 4 * fhalf) * 2;
  if constexpr (SPLIT) {
    const long long plane = (long long)g.Co * 2;
#pragma unroll
    for (int half64 = 0; half64 < 2; ++half64) {
      const c3_f32x16& a = half64 ? acc1 : acc0;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = g.relu ? __builtin_fmaxf(a[4 * g4 + e], 0.f) : a[4 * g4 + e];
        uint32_t h0, l0, h1, l1;
        ctpn_split_pk_bf16(v[0], v[1], h0, l0);
        ctpn_split_pk_bf16(v[2], v[3], h1, l1);
        char* d = op + 64 * half64 + 16 * g4;
        *(uint2*)d = make_uint2(h0, h1);
        *(uint2*)(d + plane) = make_uint2(l0, l1);
        if (g.dup_hi) *(uint2*)(d + 2 * plane) = make_uint2(h0, h1);
      }
    }
    return;
  }
  auto pk = [&](float lo, float hi) -> uint32_t {
    const uint32_t p = c3_cvt_pk<H>(lo, hi);
    if (!g.relu) return p;
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, p), s16x2{0, 0}));   // bf16 ReLU on the packed pair
  };
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    *(uint2*)(op + 16 * g4) = make_uint2(pk(acc0[4 * g4], acc0[4 * g4 + 1]), pk(acc0[4 * g4 + 2], acc0[4 * g4 + 3]));
    *(uint2*)(op + 64 + 16 * g4) = make_uint2(pk(acc1[4 * g4], acc1[4 * g4 + 1]), pk(acc1[4 * g4 + 2], acc1[4 * g4 + 3]));
  }
}

// r edge columns [w - r, w) of an h x w layer; pooled: r even, w - r even, `out` is the pooled map ((h / 2 + 2) x (w / 2 + 2) bordered)
template <typename H, bool SPLIT = false>
static int c3_launch_edge(const void* in, const void* wt, const float* bias, void* out, int n, int h, int w, int ci, int co, int relu, int r,
                          bool pooled, hipStream_t s, bool deep, int dup_hi = 0, int ks = 1) {
  ConvEdge e{};
  e.in = in; e.wt = wt; e.bias = bias; e.out = out; e.H = h; e.W = w; e.Ci = ci; e.Co = co; e.rx0 = w - r; e.rw = r; e.relu = relu;
  e.in_pitch = SPLIT ? 2 * ci : ci; e.out_pitch = SPLIT ? (dup_hi ? 3 : 2) * co : co; e.dup_hi = SPLIT && dup_hi ? 1 : 0;
  if (pooled && ((r & 1) || ((w - r) & 1) || h < 2)) return fail(CTPN_ERR_ARG, "conv3x3 edge: pooled edge needs even columns");
  e.M = pooled ? (long long)n * (h / 2) * (r / 2) : (long long)n * h * r;
  const long long per_wave = pooled ? 8 : 32;
  const long long nblk = ((e.M + per_wave - 1) / per_wave) * (co / 64);
  if (nblk <= 0 || nblk > 0x7fffffffLL || e.M > 0x7fffffffLL || !bias) return fail(CTPN_ERR_ARG, "conv3x3 edge: problem out of range");
  if constexpr (SPLIT) {
    // K split over waves: ks = the plan's edge_ks (c3_plan: 3 or 6 by Ci alone)
    if ((ks != 1 && ks != 3 && ks != 6) || (27 * (ci / 16)) % (4 * ks) != 0) return fail(CTPN_ERR_ARG, "conv3x3 edge: the K split is 1, 3 or 6 waves of whole rounds of four K steps");
    if (deep && ks > 1) {
      if (ks == 6) {
        if (pooled) hipLaunchKernelGGL((conv3x3_edge_kernel<H, true, true, true, 6>), dim3((unsigned)nblk), dim3(64 * 6), 0, s, e);
        else hipLaunchKernelGGL((conv3x3_edge_kernel<H, false, true, true, 6>), dim3((unsigned)nblk), dim3(64 * 6), 0, s, e);
      } else {
        if (pooled) hipLaunchKernelGGL((conv3x3_edge_kernel<H, true, true, true, 3>), dim3((unsigned)nblk), dim3(64 * 3), 0, s, e);
        else hipLaunchKernelGGL((conv3x3_edge_kernel<H, false, true, true, 3>), dim3((unsigned)nblk), dim3(64 * 3), 0, s, e);
      }
      return launch_status("conv3x3 edge");
    }
  }
  if (deep) {
    if (pooled) hipLaunchKernelGGL((conv3x3_edge_kernel<H, true, true, SPLIT>), dim3((unsigned)nblk), dim3(64), 0, s, e);
    else hipLaunchKernelGGL((conv3x3_edge_kernel<H, false, true, SPLIT>), dim3((unsigned)nblk), dim3(64), 0, s, e);
  } else if (pooled) hipLaunchKernelGGL((conv3x3_edge_kernel<H, true, false, SPLIT>), dim3((unsigned)nblk), dim3(64), 0, s, e);
  else hipLaunchKernelGGL((conv3x3_edge_kernel<H, false, false, SPLIT>), dim3((unsigned)nblk), dim3(64), 0, s, e);
  return launch_status("conv3x3 edge");
}
}  // namespace ctpn
