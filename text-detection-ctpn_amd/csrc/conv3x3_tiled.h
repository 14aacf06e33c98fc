// conv3x3_kernel (one workgroup per 256-pixel x BN-channel tile) and its launch template c3_launch; scheme and shared helpers: conv3x3_base.h
#pragma once
#include "conv3x3_base.h"
namespace ctpn {

// TW: width of the 2D output patch (32 -> 8 x 32, 16 -> 16 x 16; a 32-pixel MFMA tile is one row of 32 or two rows of 16).
// The launcher picks the shape that wastes fewer pixels on the layer's map (e.g. 74 x 112 pooled: 19 % -> 7.5 %).
// SPLIT: T = h_bf16, OutT = float (the LDS staging of the epilogue holds the fp32 sums; the global stores split them)
template <typename T, typename OutT, int BN, int WGM, int WGN, bool FLAT, bool POOL, int ABUF, int NBUF, int TW = 32, bool SPLIT = false>
__global__ __launch_bounds__(WGM* WGN * 64) void conv3x3_kernel(Conv3 g) {
  static_assert(!SPLIT || (std::is_same<T, h_bf16>::value && std::is_same<OutT, float>::value), "split kernels run bf16 MFMAs and stage fp32 sums");
  constexpr int C3_TW = TW, C3_TH = C3_BM / TW, C3_PW2D = C3_TW + 2;
  static_assert(TW == 32 || TW == 16, "2D patch is 8 x 32 or 16 x 16");
  constexpr int NW = WGM * WGN, NTHR = NW * 64;
  constexpr int MT = (C3_BM / 32) / WGM;      // pixel tiles (32 px) per wave
  constexpr int NTL = (BN / 32) / WGN;        // channel tiles per wave
  constexpr int BKE = 128 / (int)sizeof(T);
  constexpr int B_BYTES = BN * 128;
  constexpr int B_LOADS = BN / 8 / NW;        // 1 KB wave-loads of B per wave per K step
  constexpr int AG_MAX = FLAT ? (61 + NW - 1) / NW : (43 + NW - 1) / NW;   // A groups (8 rows each) per wave, upper bound
  constexpr int EP = BN * (int)sizeof(OutT) + 16;
  static_assert(BN % (8 * NW) == 0 && (C3_BM / 32) % WGM == 0 && (BN / 32) % WGN == 0, "bad wave split");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int nblk = gridDim.x, bid = blockIdx.x;
  const int xq = nblk >> 3, xr = nblk & 7, xcd = bid & 7;
  const int lid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);
  const int tn = lid % g.tiles_n;
  const int pt = lid / g.tiles_n;
  const int n0 = tn * BN;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  const int Wp = g.W + 2, Hp = g.H + 2;
  const int PW = FLAT ? Wp : C3_PW2D;          // LDS-window pixel pitch of one image row
  const int a_bytes = g.a_rows * 128;
  char* const sA = smem;                        // ABUF windows
  char* const sB = smem + ABUF * a_bytes;       // NBUF weight strips
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  // tile origin
  int img = 0, y0 = 0, x0 = 0;
  long long q0 = 0;
  if constexpr (FLAT) {
    q0 = (long long)pt * C3_BM;
  } else {
    const int per_img = g.tiles_x * g.tiles_y;
    img = pt / per_img;
    const int rem = pt - img * per_img;
    const int tyi = rem / g.tiles_x;
    y0 = tyi * C3_TH;
    x0 = (rem - tyi * g.tiles_x) * C3_TW;
  }

  // ---- staging sources ----
  const int srow = lane >> 3, sslot = lane & 7;
  const int a_groups = g.a_rows >> 3;
  long long a_off[AG_MAX];
#pragma unroll
  for (int i = 0; i < AG_MAX; ++i) {
    int grp = wave + i * NW;
    if (NBUF == 3 && grp > a_groups - 1) grp = a_groups - 1;   // counted-vmcnt pipeline: every wave issues every slot
    const int r = grp * 8 + srow;
    long long pix;
    if constexpr (FLAT) {
      long long q = q0 - PW - 1 + r;
      q = q < 0 ? 0 : (q > g.m_total - 1 ? g.m_total - 1 : q);
      pix = q;
    } else {
      const int i2 = r / C3_PW2D, j2 = r - i2 * C3_PW2D;
      int yy = y0 + i2, xx = x0 + j2;
      yy = yy > Hp - 1 ? Hp - 1 : yy;
      xx = xx > Wp - 1 ? Wp - 1 : xx;
      pix = ((long long)img * Hp + yy) * Wp + xx;
    }
    a_off[i] = pix * g.in_pitch * (long long)sizeof(T) + ((sslot ^ ((r >> 1) & 7)) << 4);
  }
  const long long ktot_bytes = 9LL * g.Ci * (long long)sizeof(T);
  long long b_off[B_LOADS];
#pragma unroll
  for (int i = 0; i < B_LOADS; ++i) {
    const int row = (wave + i * NW) * 8 + srow;
    b_off[i] = (long long)(n0 + row) * ktot_bytes + ((sslot ^ ((row >> 1) & 7)) << 4);
  }
  const char* a_base = (const char*)g.in;
  const char* b_base = (const char*)g.wt;

  auto issue_a_group = [&](int i, int chunk, int buf) {   // i-th group of this wave
    if constexpr (SPLIT) chunk = chunk >= g.a_wrap ? chunk - g.a_wrap : chunk;      // third K block: the hi plane again
    int grp = wave + i * NW;
    if (NBUF == 3 && grp > a_groups - 1) grp = a_groups - 1;   // duplicate of the last group: same bytes, same place
    if constexpr (NBUF == 3) {
      c3_glds16_asm(a_base + a_off[i] + (long long)chunk * 128, __builtin_amdgcn_readfirstlane(lds0 + buf * a_bytes + grp * 1024));
    } else {
      if (grp < a_groups)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_base + a_off[i] + (long long)chunk * 128),
                                         (__attribute__((address_space(3))) void*)(sA + buf * a_bytes + grp * 1024), 16, 0, 0);
    }
  };
  auto issue_b = [&](int chunk, int tap, int buf) {
    const long long kb = ((long long)tap * g.Ci + (long long)chunk * BKE) * (long long)sizeof(T);
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
      if constexpr (NBUF == 3)
        c3_glds16_asm(b_base + b_off[i] + kb, __builtin_amdgcn_readfirstlane(lds0 + ABUF * a_bytes + buf * B_BYTES + (wave + i * NW) * 1024));
      else
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_base + b_off[i] + kb),
                                         (__attribute__((address_space(3))) void*)(sB + buf * B_BYTES + (wave + i * NW) * 1024), 16, 0, 0);
    }
  };

  c3_f32x16 acc[NTL][MT];
#pragma unroll
  for (int i = 0; i < NTL; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int l31 = lane & 31, fhalf = lane >> 5;
  const int fswB = (l31 >> 1) & 7;
  int tilebase[MT];   // LDS row of (pixel tile j, lane) at tap (0,0)
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    if constexpr (FLAT) tilebase[j] = (wm * MT + j) * 32 + l31;
    else if constexpr (TW == 32) tilebase[j] = (wm * MT + j) * C3_PW2D + l31;
    else tilebase[j] = (2 * (wm * MT + j) + (l31 >> 4)) * C3_PW2D + c3_tw16_col(l31);
  }

  auto compute = [&](int abuf, int bbuf, int tap) {
    const int ky = tap / 3, kx = tap - ky * 3;
    const int rowoff = ky * PW + kx;
    const char* sa = sA + abuf * a_bytes;
    const char* sb = sB + bbuf * B_BYTES + (wn * (BN / WGN) + l31) * 128;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int slot = 2 * q + fhalf;
      uint4 xf[MT], wf[NTL];
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const int r = tilebase[j] + rowoff;
        xf[j] = *(const uint4*)(sa + r * 128 + ((slot ^ ((r >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int i = 0; i < NTL; ++i) wf[i] = *(const uint4*)(sb + i * 32 * 128 + ((slot ^ fswB) << 4));
#pragma unroll
      for (int i = 0; i < NTL; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) c3_mfma<T>(acc[i][j], wf[i], xf[j]);
    }
  };

  // ---- main loop: chunk-major, tap-minor ----
  const int nchunks = g.Ci / BKE;
  {
    // Three weight-strip buffers, prefetch distance 2, COUNTED vmcnt + raw s_barrier: the strip for step s+2 (and
    // the next chunk's window slices) stay in flight across the barrier; only what step s+1 needs is waited for.
    // Step s = 9*chunk + tap uses strip buffer s % 3 = tap % 3. Every wave issues the same number of loads per
    // step (padded with duplicates), so the vmcnt immediates are compile-time constants.
    static_assert(NBUF == 3, "pipeline is written for three strip buffers");
#pragma unroll
    for (int i = 0; i < AG_MAX; ++i) issue_a_group(i, 0, 0);
    issue_b(0, 0, 0);
    issue_b(0, 1, 1);
    c3_wait_vm<B_LOADS>();
    c3_barrier();
    auto step = [&](auto tc, auto lastc, int c, int ab) {
      constexpr int t = decltype(tc)::value;
      constexpr bool last = decltype(lastc)::value;
      // the next chunk's window slices go out in steps 0..7 ONLY: what step 8 issues is still in flight when the next chunk
      // starts (its wait leaves this step's loads pending), and with 4 waves (11 groups per wave) a slice issued there was
      // read before it had landed -- a rare wrong pixel row in the fp32 conv1_2
      constexpr int nA = (ABUF == 2 && !last && t < 8 && AG_MAX > t) ? (AG_MAX - t + 7) / 8 : 0;
      constexpr bool has_b = (t + 2 < 9) || !last;
      if constexpr (has_b) {
        if constexpr (t + 2 < 9) issue_b(c, t + 2, (t + 2) % 3);
        else issue_b(c + 1, t + 2 - 9, (t + 2) % 3);
      }
      if constexpr (nA > 0) {
#pragma unroll
        for (int i = t; i < AG_MAX; i += 8) issue_a_group(i, c + 1, ab ^ 1);
      }
      compute(ab, t % 3, t);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // no fragment read in flight across the barrier: the next step's DMA recycles the strip just read (see conv3x3_p_kernel)
      c3_wait_vm<(has_b ? B_LOADS : 0) + nA>();
      c3_barrier();
    };
    auto chunk = [&](auto lastc, int c) {
      const int ab = (ABUF == 2) ? (c & 1) : 0;
      step(std::integral_constant<int, 0>{}, lastc, c, ab);
      step(std::integral_constant<int, 1>{}, lastc, c, ab);
      step(std::integral_constant<int, 2>{}, lastc, c, ab);
      step(std::integral_constant<int, 3>{}, lastc, c, ab);
      step(std::integral_constant<int, 4>{}, lastc, c, ab);
      step(std::integral_constant<int, 5>{}, lastc, c, ab);
      step(std::integral_constant<int, 6>{}, lastc, c, ab);
      step(std::integral_constant<int, 7>{}, lastc, c, ab);
      step(std::integral_constant<int, 8>{}, lastc, c, ab);
    };
    for (int c = 0; c + 1 < nchunks; ++c) chunk(std::false_type{}, c);
    chunk(std::true_type{}, nchunks - 1);
    __syncthreads();
  }

  // ---- epilogue ----
#pragma unroll
  for (int i = 0; i < NTL; ++i) {
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int co_l = wn * (BN / WGN) + i * 32 + 8 * g4 + 4 * fhalf;
      c3_f32x4 bv = {0.f, 0.f, 0.f, 0.f};
      if (g.bias) bv = *(const c3_f32x4*)(g.bias + n0 + co_l);
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const int p = (wm * MT + j) * 32 + ((!FLAT && TW == 16) ? (l31 & 16) + c3_tw16_col(l31) : l31);   // tile-local pixel, row-major
        float v0 = acc[i][j][4 * g4 + 0] + bv[0];
        float v1 = acc[i][j][4 * g4 + 1] + bv[1];
        float v2 = acc[i][j][4 * g4 + 2] + bv[2];
        float v3 = acc[i][j][4 * g4 + 3] + bv[3];
        if (g.relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
        char* dst = smem + p * EP + co_l * (int)sizeof(OutT);
        if constexpr (sizeof(OutT) == 4) {
          c3_f32x4 o = {v0, v1, v2, v3};
          *(c3_f32x4*)dst = o;
        } else {
          uint2 o;
          o.x = c3_cvt_pk<OutT>(v0, v1);
          o.y = c3_cvt_pk<OutT>(v2, v3);
          *(uint2*)dst = o;
        }
      }
    }
  }
  __syncthreads();
  constexpr int CH = BN * (int)sizeof(OutT) / 16;
  constexpr int EPC = 16 / (int)sizeof(OutT);
  if (g.out) {
    char* out_base = (char*)g.out;
    for (int c = tid; c < C3_BM * CH; c += NTHR) {
      const int p = c / CH, ch = c - p * CH;
      const int co = n0 + ch * EPC;
      if (co >= g.Co) continue;
      long long opix;
      bool ok;
      if constexpr (FLAT) {
        const long long q = q0 + p;
        const long long per = (long long)Hp * Wp;
        const long long im = q / per;
        const int rem = (int)(q - im * per);
        const int yb = rem / Wp, xb = rem - yb * Wp;
        ok = q < g.m_total && yb >= 1 && yb <= g.H && xb >= 1 && xb <= g.W;
        opix = q;
      } else {
        const int y = y0 + p / C3_TW, x = x0 + p % C3_TW;
        ok = y < g.H && x < g.W;
        opix = ((long long)img * Hp + y + 1) * Wp + x + 1;
      }
      if constexpr (SPLIT) { if (ok) c3_split_store4(out_base + opix * g.out_pitch * 2, co, *(const uint4*)(smem + p * EP + ch * 16), g.Co, g.dup_hi); }
      else if (ok) *(uint4*)(out_base + (opix * g.Co + co) * (long long)sizeof(OutT)) = *(const uint4*)(smem + p * EP + ch * 16);
    }
  }
  if constexpr (POOL && !FLAT) {
    const int Ho = g.H >> 1, Wo = g.W >> 1;
    char* pool_base = (char*)g.pool_out;
    for (int c = tid; c < (C3_BM / 4) * CH; c += NTHR) {
      const int pp = c / CH, ch = c - pp * CH;
      const int co = n0 + ch * EPC;
      if (co >= g.Co) continue;
      const int py = pp / (C3_TW / 2), px = pp % (C3_TW / 2);   // (TH/2) x (TW/2) pooled pixels
      const int Y = (y0 >> 1) + py, X = (x0 >> 1) + px;
      if (Y >= Ho || X >= Wo) continue;
      const int p00 = (2 * py) * C3_TW + 2 * px;
      const uint4 a = *(const uint4*)(smem + p00 * EP + ch * 16);
      const uint4 b = *(const uint4*)(smem + (p00 + 1) * EP + ch * 16);
      const uint4 cc = *(const uint4*)(smem + (p00 + C3_TW) * EP + ch * 16);
      const uint4 d = *(const uint4*)(smem + (p00 + C3_TW + 1) * EP + ch * 16);
      const uint4 m = c3_max4<OutT>(c3_max4<OutT>(a, b), c3_max4<OutT>(cc, d));
      const long long opix = ((long long)img * (Ho + 2) + Y + 1) * (Wo + 2) + X + 1;
      if constexpr (SPLIT) c3_split_store4(pool_base + opix * g.out_pitch * 2, co, m, g.Co, g.dup_hi);     // max of the fp32 sums, then split: pooling commutes with the monotone rounding
      else *(uint4*)(pool_base + (opix * g.Co + co) * (long long)sizeof(OutT)) = m;
    }
  }
}

template <typename T, typename OutT, int BN, int WGM, int WGN, bool FLAT, bool POOL, int ABUF, int NBUF, int TW = 32, bool SPLIT = false>
static int c3_launch(Conv3 g, hipStream_t s) {
  constexpr int C3_TW = TW, C3_TH = C3_BM / TW, C3_PW2D = C3_TW + 2;
  constexpr int NTHR = WGM * WGN * 64;
  constexpr int EP = BN * (int)sizeof(OutT) + 16;
  const int Wp = g.W + 2;
  const int rows = FLAT ? (C3_BM + 2 * Wp + 2) : (C3_TH + 2) * C3_PW2D;
  g.a_rows = (rows + 7) & ~7;
  constexpr int NWL = WGM * WGN;
  constexpr int AG_MAX = FLAT ? (61 + NWL - 1) / NWL : (43 + NWL - 1) / NWL;
  if ((g.a_rows >> 3) > AG_MAX * NWL) return fail(CTPN_ERR_ARG, "conv3x3: input window does not fit the flat-mode staging plan");
  g.tiles_n = (g.Co + BN - 1) / BN;
  long long ptiles;
  if (FLAT) {
    g.m_total = (long long)g.N * (g.H + 2) * Wp;
    ptiles = (g.m_total + C3_BM - 1) / C3_BM;
  } else {
    int he, we;
    c3_extent(g, POOL, he, we);
    g.tiles_x = (we + C3_TW - 1) / C3_TW;
    g.tiles_y = (he + C3_TH - 1) / C3_TH;
    ptiles = (long long)g.N * g.tiles_x * g.tiles_y;
  }
  const long long nblk = ptiles * g.tiles_n;
  if (nblk <= 0 || nblk > 0x7fffffffLL) return fail(CTPN_ERR_ARG, "conv3x3: grid out of range");
  const int main_lds = ABUF * g.a_rows * 128 + NBUF * BN * 128;
  const int epi_lds = C3_BM * EP;
  const int lds = main_lds > epi_lds ? main_lds : epi_lds;
  if (lds > C3_LDS_MAX) return fail(CTPN_ERR_ARG, "conv3x3: LDS budget exceeded");
  auto k = conv3x3_kernel<T, OutT, BN, WGM, WGN, FLAT, POOL, ABUF, NBUF, TW, SPLIT>;
  static bool attr[CTPN_MAX_DEV] = {false};      // per instantiation and device
  int dev = 0, rc;
  if ((rc = current_device(dev)) || (rc = raise_dynamic_lds((const void*)k, C3_LDS_MAX, attr, dev))) return rc;
  hipLaunchKernelGGL(k, dim3((unsigned)nblk), dim3(NTHR), lds, s, g);
  return launch_status("conv3x3");
}
}  // namespace ctpn
