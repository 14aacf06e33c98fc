// conv3x3_p_kernel (persistent workgroups walk the tiles) and its launch template c3_launch_p; scheme and shared helpers: conv3x3_base.h
#pragma once
#include "conv3x3_base.h"
namespace ctpn {

// ---------------------------------------------------------------------------------------------
// Persistent form of conv3x3_kernel (256 pixels x 128 channels, 8 waves, three weight strips, double window):
// one workgroup per CU walks tiles w, w + G, ... and its load pipeline never drains -- while a tile's last chunk is on
// the MFMAs, the window slices and the first two weight strips of the NEXT tile stream in exactly like the next chunk
// of the same tile would. The epilogue is register-only (bias from LDS, ReLU, v_cvt_pk, v_permlane32_swap -> 16-byte
// stores; the 2x2 pool is a max over the wave's two pixel rows + lane^1, + lane^16 for 16 x 16 patches), because the
// LDS is busy receiving the next tile. conv3x3_kernel pays per tile: an exposed prologue (first window + two strips,
// ~1.5 us), the LDS-staged epilogue (~1.5 us) and the workgroup launch -- 15 % of a K = 1152 tile, 9 % at K = 2304,
// 5 % at K = 4608, which is the order the layers' TFLOP/s were in (conv2_2 951 ... conv4_2 1236).
// ---------------------------------------------------------------------------------------------
// SPLIT: T = OutT = h_bf16 over (hi, lo) planes, see the file comment
// BN_T = 64 (Co = 64: conv1_2 outside the 16-bit modes' weights-in-registers kernel, i.e. split precision and fp32): the same walk, windows,
// strips and pipeline on 256 pixels x 64 channels -- 8 waves = 4 (pixel groups of 64) x 2 (channel halves of 32), ONE channel tile per wave
// (two MFMAs per k-slice group; 2 x + 1 w fragment reads, the carried row fragment saves a third of the x reads), 8 x 32 patches only. The
// non-persistent kernel this replaces for that layer paid an exposed prologue and an LDS-staged epilogue per 256 x 64 tile of a K = 1728
// loop: 4.53 ms = 33.7 % of the bf16 peak for split conv1_2 at batch 32 (VERDICT r5 "weak" 1).
// BM_T = 64 (flat windows, round 6): 64 pixels x 128 channels per workgroup, 8 waves = 2 pixel tiles x 4 channel tiles, ONE 32 x 32 MFMA tile per
// wave. For the ONE-IMAGE call: conv5_x / rpn_conv of a 600 x 900 image are 36 tiles of 256 pixels x 128 channels -- 72 half-tile items on 256 CUs,
// each walking 72 K steps of 16 MFMAs per wave with one wave per SIMD (30 us per layer, 13 % of peak); as 144 items of 64 x 128 every wave is
// busy with 4 MFMAs per K step and the step is bounded by the LDS (two fragment reads per MFMA) instead of by one wave's latency chain.
// Every output is still summed by one wave in the usual K order: the bits do not depend on the form (tools/r6_lone_vs_batch.py).
// HT32 (round 6): the half-tile tail for 8 x 32 patches as well (a half = the tile shifted by four patch rows, computed by the waves of pixel
// groups 0 and 1), for one or two images per call only: there the ragged-column edge kernels run in the stream, not beside this kernel, so the
// ~30 registers the idle path costs are available.
template <typename T, typename OutT, bool FLAT, bool POOL, int TW, bool SPLIT = false, int BN_T = 128, int BM_T = 256, bool HT32 = false>
__global__ __launch_bounds__(512) void conv3x3_p_kernel(Conv3 g) {
  static_assert(!HT32 || (TW == 32 && !FLAT && BN_T == 128 && BM_T == 256), "half-tile tails for 8 x 32 patches: the plain 128-channel form");
  static_assert(!SPLIT || std::is_same<T, h_bf16>::value, "split kernels run bf16 MFMAs");
  static_assert(BN_T == 128 || (BN_T == 64 && !FLAT && TW == 32), "the 64-channel form exists for 8 x 32 patches");
  static_assert(BM_T == 256 || (BM_T == 64 && FLAT && BN_T == 128), "the 64-pixel form exists for flat windows");
  constexpr int BM = BM_T;
  constexpr int BN = BN_T, WGN = BM == 64 ? 4 : 2;         // 8 waves = 4 (pixel tiles) x 2 (channel halves); 64-pixel form: 2 x 4
  constexpr int C3_TW = TW, C3_PW2D = C3_TW + 2;
  constexpr int NW = 8;
  constexpr int MT = BM == 64 ? 1 : 2, NTL = BN / (32 * WGN);
  constexpr int BKE = 128 / (int)sizeof(T);
  constexpr int B_BYTES = BN * 128;
  constexpr int B_LOADS = BN / 8 / NW;        // 2
  constexpr int AG_MAX = FLAT ? ((BM == 64 ? 37 : 61) + NW - 1) / NW : (43 + NW - 1) / NW;
  static_assert(sizeof(T) == sizeof(OutT), "in and out types match");
  static_assert(!(FLAT && POOL), "the pool fusion needs 2D patches");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int G = gridDim.x, bid = blockIdx.x;
  const int xq = G >> 3, xr = G & 7, xcd = bid & 7;
  const int w0 = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);   // XCD-mates walk neighbouring tiles
  const long long total = g.ptiles_total;
  if (w0 >= g.ht_full + 2LL * g.ht_r) return;                  // work items: whole tiles + two halves per split tile (= total when nothing is split)
  // Half-tile tail (flat windows: conv5_x / rpn_conv; 16 x 16 patches: conv4_x). With G workers and total = q G + r tiles the last round keeps r workers busy and
  // G - r idle: 1132 tiles on 256 CUs pay 5 rounds for 4.42 of work. For r <= G / 2 the r tail tiles are split into two halves of 128
  // PIXELS (2 r work items on 2 r workers): a half is the tile shifted by 128 flat pixels / 8 patch rows, computed by the workgroup's waves
  // 0..3 only (pixel groups wm = 0, 1: one wave per SIMD, so each SIMD's MFMA pipe belongs to one wave and the K loop takes about half as
  // long), while waves 4..7 keep issuing their share of the LDS-DMA and meeting the barriers. Every output is still computed by ONE wave in
  // the usual K order, so results do not depend on where a tile falls in the walk (a split of K would: the sums of a batch and of its
  // images run alone would differ in the last bit; that variant, with a fence-free partial-sum exchange, was built and dropped in round 3).
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  const int Wp = g.W + 2, Hp = g.H + 2;
  const int PW = FLAT ? Wp : C3_PW2D;
  const int a_bytes = g.a_rows * 128;
  char* const sA = smem;                                   // 2 windows
  char* const sB = smem + 2 * a_bytes;                     // 3 weight strips
  float* const sbias = (float*)(smem + 2 * a_bytes + 3 * B_BYTES);   // the whole bias vector (padded to the N tile)
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int srow = lane >> 3, sslot = lane & 7;
  const int a_groups = g.a_rows >> 3;
  const int l31 = lane & 31, fhalf = lane >> 5;
  const int fswB = (l31 >> 1) & 7;
  const long long ktot_bytes = 9LL * g.Ci * (long long)sizeof(T);
  const char* a_base = (const char*)g.in;
  const char* b_base = (const char*)g.wt;
  const int nchunks = g.Ci / BKE;

  for (int i = tid; i < g.tiles_n * BN; i += 512) sbias[i] = (g.bias && i < g.Co) ? g.bias[i] : 0.f;

  // Window and weight-strip staging: `global_load_lds_dwordx4 voff, s[base]` -- the per-lane 32-bit source offsets of a wave's
  // groups are tile-independent (computed once), the tile / chunk / tap enters through a scalar base: one VMEM instruction per KiB and
  // no VALU in the K loop (per-lane 64-bit pixel arithmetic and clamping cost ~5 VALU per step and 12 live VGPRs). Windows are
  // fetched WITHOUT clamping: reads past the bordered image (edge tiles) or before / behind the buffer (flat mode's first and last
  // tiles) land in the slack the ctx allocates around every activation buffer and only feed outputs that are never stored.
  struct Tile { int n0, img, y0, x0; long long q0; const char* ab; const char* bb;          // ab / bb: scalar bases of the window / the weight rows
                int rbase; };       // stacked tile rows: bordered row, inside its image, of the tile's first output row
  auto usg = [](unsigned v) -> unsigned { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); };
  auto spin = [&](const char* base, long long byte_off) -> const char* {                    // uniform pointer pinned to an SGPR pair
    const unsigned long long a = (unsigned long long)(uintptr_t)base + (unsigned long long)byte_off;
    const unsigned lo = usg((unsigned)a), hi = usg((unsigned)(a >> 32));
    return (const char*)(uintptr_t)(((unsigned long long)hi << 32) | lo);
  };
  const int pix_bytes = g.in_pitch * (int)sizeof(T);
  uint32_t aoff[AG_MAX];
#pragma unroll
  for (int i = 0; i < AG_MAX; ++i) {
    int grp = wave + i * NW;
    if (grp > a_groups - 1) grp = a_groups - 1;            // every wave issues every slot (duplicates of the last group)
    const int r = grp * 8 + srow;
    int pix;
    if constexpr (FLAT) pix = r;
    else { const int i2 = r / C3_PW2D, j2 = r - i2 * C3_PW2D; pix = i2 * Wp + j2; }
    aoff[i] = (uint32_t)(pix * pix_bytes + ((sslot ^ ((r >> 1) & 7)) << 4));
  }
  uint32_t boff[B_LOADS];
#pragma unroll
  for (int i = 0; i < B_LOADS; ++i) {
    const int row = (wave + i * NW) * 8 + srow;
    boff[i] = (uint32_t)((long long)row * ktot_bytes + ((sslot ^ ((row >> 1) & 7)) << 4));
  }
  auto setup = [&](long long lid, int half, Tile& t) {       // half: -1 = the whole tile, 0 / 1 = its first / second 128 pixels (flat only)
    int tn = (int)(lid % g.tiles_n);
    long long pt = lid / g.tiles_n;
#ifdef CTPN_ABLATION
    // CTPN_C3_P_ABL | 0x100 / 0x200 (measurement builds; CORRECT results: a bijection on the whole rounds of the walk): channel-slice-major
    // tile order per XCD for the Co = 512 layers. Default: the 32 workers of an XCD take 8 pixel tiles x all 4 slices per
    // round (a window is fetched by ONE XCD, the 4.7 MB of weights by every XCD every round). 0x100: an XCD takes ONE slice (two XCDs per
    // slice) x 32 pixel tiles; 0x200: TWO slices x 16 pixel tiles. tools/r5_order_ab.sh measures FETCH_SIZE and images/s of the three.
    if ((g.abl & 0x300) && g.tiles_n == 4 && G == 256 && lid < (g.ht_full / G) * G) {
      const int r = (int)(lid >> 8), p = (int)(lid & 255), xc = p >> 5, j = p & 31;
      if (g.abl & 0x100) { tn = xc & 3; pt = (long long)r * 64 + (xc >> 2) * 32 + j; }
      else { tn = 2 * (xc & 1) + (j & 1); pt = (long long)r * 64 + (xc >> 1) * 16 + (j >> 1); }
    }
#endif
    t.n0 = tn * BN; t.img = 0; t.y0 = 0; t.x0 = 0; t.q0 = 0; t.rbase = 0;
    long long pix0;
    if constexpr (FLAT) {
      t.q0 = pt * BM + (half > 0 ? BM / 2 : 0);
      pix0 = t.q0 - PW - 1;
    } else {
      const int per_img = g.stacked ? 0x7fffffff : g.tiles_x * g.tiles_y;       // stacked: one "image" = the whole bordered batch
      t.img = (int)(pt / per_img);
      const int rem = (int)(pt - (long long)t.img * per_img);
      const int tyi = rem / g.tiles_x;
      t.y0 = tyi * (C3_BM / TW) + (half > 0 ? (C3_BM / TW) / 2 : 0);      // (half items: 16 x 16 patches only, see HT)
      t.x0 = (rem - tyi * g.tiles_x) * C3_TW;
      pix0 = ((long long)t.img * Hp + t.y0) * Wp + t.x0;
      t.rbase = g.stacked ? (t.y0 + 1) % Hp : 0;
    }
    t.ab = spin(a_base, pix0 * pix_bytes);
    t.bb = spin(b_base, (long long)t.n0 * ktot_bytes);
  };
  auto issue_a_group = [&](int i, const char* ab, int chunk, int buf) {
    if constexpr (SPLIT) chunk = chunk >= g.a_wrap ? chunk - g.a_wrap : chunk;      // third K block: the hi plane again (scalar select)
    int grp = wave + i * NW;
    if (grp > a_groups - 1) grp = a_groups - 1;
    c3_glds16_saddr(ab + chunk * 128, aoff[i], __builtin_amdgcn_readfirstlane(lds0 + buf * a_bytes + grp * 1024));
  };
  // K steps of a chunk run KX-MAJOR: step t = (kx = t / 3, ky = t % 3), i.e. weight tap ky * 3 + kx. Consecutive steps then differ by one
  // input ROW, and the pixel fragments of the row two steps share stay in registers (see load_group): the LDS read stream -- which at one
  // ds_read_b128 per MFMA and wave runs exactly at the CU's 128 B/clk -- loses a sixth (8 x 32 patches) / a twelfth (16 x 16) of its bytes.
  auto issue_b = [&](const char* bb, int chunk, int step_t, int buf) {
    const int tap = (step_t % 3) * 3 + step_t / 3;
    const char* sb = bb + ((long long)tap * g.Ci + (long long)chunk * BKE) * (long long)sizeof(T);
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i)
      c3_glds16_saddr(sb, boff[i], __builtin_amdgcn_readfirstlane(lds0 + 2 * a_bytes + buf * B_BYTES + (wave + i * NW) * 1024));
  };

  c3_f32x16 acc[NTL][MT];
  int tilebase[MT];   // LDS row of (pixel tile j, lane) at tap (0,0)
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    if constexpr (FLAT) tilebase[j] = (wm * MT + j) * 32 + l31;
    else if constexpr (TW == 32) tilebase[j] = (wm * MT + j) * C3_PW2D + l31;
    else tilebase[j] = (2 * (wm * MT + j) + (l31 >> 4)) * C3_PW2D + c3_tw16_col(l31);
  }
  // Pixel fragments carried between the steps of a kx triple (4 k-slices x 16 bytes per lane):
  //   8 x 32 patches : pixel tile j of tap ky is window row 2 wm + j + ky, so tile 0 of step ky + 1 IS tile 1 of step ky: every step after
  //                    the first of a triple reads one pixel fragment per k-slice instead of two (4 row reads per triple instead of 6);
  //   16 x 16 patches: a tile is two window rows, tile 0 of ky = 2 IS tile 1 of ky = 0 (held across the ky = 1 step): 5 instead of 6;
  //   flat windows   : tiles are 32 consecutive pixels, a row shift of W + 2 pixels maps no tile onto another: nothing to carry.
  uint4 xcar[4];

  // The fragment reads run ONE k-slice group ahead of the MFMAs through a second register set. hipcc on its own issues a group's
  // four reads right behind the previous group's last MFMA and makes that group's first MFMA wait for them: with the two waves of a SIMD
  // kept in step by the barriers, both sit in that LDS latency together (MFMA pipe 60 - 73 % busy). Here group (t, q) is READ while the
  // MFMAs of the group before it (the last group of step t - 1 for q = 0: it runs behind the barrier, on fragments read in front of it)
  // are issued, and its own MFMAs come one group later; sched_group_barriers order every [reads of group n + 1][MFMAs of group n] block, a sched_barrier closes it.
  struct Frag { uint4 x[MT], w[NTL]; };
  auto load_group = [&](int abuf, int bbuf, auto tc, auto qc, Frag& f) {
    constexpr int t = decltype(tc)::value, q = decltype(qc)::value;
    constexpr int kx = t / 3, ky = t % 3;
    constexpr bool reuse0 = !FLAT && ((TW == 32 && ky > 0) || (TW == 16 && ky == 2));
    constexpr bool save1 = !FLAT && ((TW == 32 && ky < 2) || (TW == 16 && ky == 0));
    const int rowoff = ky * PW + kx;
    const char* sa = sA + abuf * a_bytes;
    const char* sb = sB + bbuf * B_BYTES + (wn * (BN / WGN) + l31) * 128;
    const int slot = 2 * q + fhalf;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      if (reuse0 && j == 0) { f.x[0] = xcar[q]; continue; }
      const int r = tilebase[j] + rowoff;
      f.x[j] = *(const uint4*)(sa + r * 128 + ((slot ^ ((r >> 1) & 7)) << 4));
    }
    if constexpr (save1) xcar[q] = f.x[1];
#pragma unroll
    for (int i = 0; i < NTL; ++i) f.w[i] = *(const uint4*)(sb + i * 32 * 128 + ((slot ^ fswB) << 4));
  };
  auto mma_group = [&](const Frag& f) {
#pragma unroll
    for (int i = 0; i < NTL; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) c3_mfma<T>(acc[i][j], f.w[i], f.x[j]);
  };
  Frag pend;

  // k-th work item of this worker: whole tiles w0 + k G below ht_full, then (flat windows only) at most one half of a tail tile; selects
  // on wave-uniform scalars and ONE setup() per item. Past the end the current item is returned again (its window is prefetched once more:
  // every step issues the same loads).
  Tile cur, nxt;
  long long lid = w0;             // index of the current item in the walk w0, w0 + G, ...
  long long cur_tile = w0; int cur_half = -1;
  bool active = true;             // does this wave compute in the current item? (waves 4..7 sit out the half items)
  // HT: kernels that split their tail tiles. Flat windows (a half = 128 consecutive pixels) and 16 x 16 patches (a half = 8 rows x 16: the
  // tile origin moves down by 8 rows, pixel groups 0 and 1 are exactly those rows). NOT the 8 x 32-patch kernels: they share their CUs
  // with the one-wave edge kernel, and the idle path costs this kernel ~30 registers (2 x 235 + 74 > a SIMD's 512).
  constexpr bool HT = ((FLAT || TW == 16) && BM == 256) || HT32;
  auto pick = [&](long long l, long long& tile, int& half) -> bool {
    if constexpr (HT) {
      const long long o = l - g.ht_full;
      const bool whole = l < g.ht_full, half_item = !whole && o < 2LL * g.ht_r;
      tile = whole ? l : (half_item ? g.ht_full + (o >> 1) : cur_tile);
      half = (int)usg((unsigned)(whole ? -1 : (half_item ? (int)(o & 1) : cur_half)));
      return whole || half_item;
    } else {
      const bool ok = l < total;
      tile = ok ? l : cur_tile; half = -1;
      return ok;
    }
  };
  (void)pick(w0, cur_tile, cur_half);
  setup(cur_tile, cur_half, cur);
  if constexpr (HT) active = cur_half < 0 || wm < 2;
  // the only exposed prologue of the launch
#pragma unroll
  for (int i = 0; i < AG_MAX; ++i) issue_a_group(i, cur.ab, 0, 0);
  issue_b(cur.bb, 0, 0, 0);
  issue_b(cur.bb, 0, 1, 1);
  c3_wait_vm<B_LOADS>();
  __syncthreads();            // also publishes sbias
  int wpar = 0;               // window buffer of the current chunk

  // One K step. Step s = 9 * chunk + tap reads strip buffer tap % 3; the strip for step s + 2 and the slices of the NEXT
  // chunk's window are issued first. `last` = last chunk of the tile: "next chunk" is chunk 0 of the next tile.
  auto step = [&](auto tc, auto lastc, int c) {
    constexpr int t = decltype(tc)::value;
    constexpr bool last = decltype(lastc)::value;
    constexpr int nA = (t < 8 && AG_MAX > t) ? (AG_MAX - t + 7) / 8 : 0;   // slices in steps 0..7 only (see conv3x3_kernel)
    if constexpr (t + 2 < 9) issue_b(cur.bb, c, t + 2, (t + 2) % 3);
    else if constexpr (last) issue_b(nxt.bb, 0, t + 2 - 9, (t + 2) % 3);
    else issue_b(cur.bb, c + 1, t + 2 - 9, (t + 2) % 3);
#pragma unroll
    for (int i = t; i < (t < 8 ? AG_MAX : 0); i += 8) {
      if constexpr (last) issue_a_group(i, nxt.ab, 0, wpar ^ 1);
      else issue_a_group(i, cur.ab, c + 1, wpar ^ 1);
    }
    constexpr int nrd = (MT + NTL) - ((!FLAT && ((TW == 32 && t % 3 > 0) || (TW == 16 && t % 3 == 2))) ? 1 : 0);   // LDS reads of one group of this step
    constexpr int nmf = ((int)sizeof(T) == 2 ? 1 : 4) * MT * NTL;                                                  // MFMA instructions of one group
    Frag nf0, nf1, nf2, nf3;
    load_group(wpar, t % 3, tc, std::integral_constant<int, 0>{}, nf0);
    if (t > 0 || c > 0) mma_group(pend);             // the last group of the previous step (none in front of a tile's first step)
    __builtin_amdgcn_sched_group_barrier(0x100, nrd, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, nmf, 0);
    __builtin_amdgcn_sched_barrier(0);
    load_group(wpar, t % 3, tc, std::integral_constant<int, 1>{}, nf1);
    mma_group(nf0);
    __builtin_amdgcn_sched_group_barrier(0x100, nrd, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, nmf, 0);
    __builtin_amdgcn_sched_barrier(0);
    load_group(wpar, t % 3, tc, std::integral_constant<int, 2>{}, nf2);
    mma_group(nf1);
    __builtin_amdgcn_sched_group_barrier(0x100, nrd, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, nmf, 0);
    __builtin_amdgcn_sched_barrier(0);
    load_group(wpar, t % 3, tc, std::integral_constant<int, 3>{}, nf3);
    mma_group(nf2);
    __builtin_amdgcn_sched_group_barrier(0x100, nrd, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, nmf, 0);
    __builtin_amdgcn_sched_barrier(0);
    pend = nf3;
    // INVARIANT: no LDS read may be in flight across the barrier below. Behind it, step t + 1 aims its LDS-DMA at the strip buffer
    // (t % 3) and -- in the chunk's last step -- at the window this step read; gfx950's barrier does not imply an lgkmcnt wait. nf3's ds_reads
    // (-> pend) were issued in front of the step's last four MFMAs and have had ~128 clk to land: the wait is free. History (until round 6 the
    // 16 x 16-patch and flat-window forms ran a plain loop, reads and MFMAs of a k-slice group back to back, without this wait): hipcc sank the
    // last k-slice group's MFMAs (and the wait for their operands) below the barrier, so that group's reads were ordered against the DMA by
    // latency only -- and lost: with another stream's kernel loading the memory system, a strip landed before the reads of the step three
    // earlier had executed (profiles/r06_barrier_war.txt: the last k-slice of one step computed with the weights of the step three later, bit
    // for bit).
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    c3_wait_vm<B_LOADS + nA>();
    c3_barrier();
  };
  auto chunk = [&](auto lastc, int c) {
    step(std::integral_constant<int, 0>{}, lastc, c);
    step(std::integral_constant<int, 1>{}, lastc, c);
    step(std::integral_constant<int, 2>{}, lastc, c);
    step(std::integral_constant<int, 3>{}, lastc, c);
    step(std::integral_constant<int, 4>{}, lastc, c);
    step(std::integral_constant<int, 5>{}, lastc, c);
    step(std::integral_constant<int, 6>{}, lastc, c);
    step(std::integral_constant<int, 7>{}, lastc, c);
    step(std::integral_constant<int, 8>{}, lastc, c);
    wpar ^= 1;
  };
  // A chunk of a wave that sits out a half item (flat windows): its share of the LDS-DMA, the counted wait and the barrier of every step --
  // exactly the loads `step` issues, no MFMAs. A compact runtime loop ON PURPOSE: guarding the MFMAs inside `step` instead put a branch
  // into every K step, which stopped hipcc from pipelining across the step boundaries (measured: the flat kernel +9 %, and that build
  // failed the run-twice-same-bytes test -- the per-step control flow let fragment reads move relative to the counted waits).
  auto idle_chunk = [&](bool last, int c) {
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
      const int t2 = t + 2 < 9 ? t + 2 : t + 2 - 9;
      const char* const bsrc = (t + 2 < 9 || !last) ? cur.bb : nxt.bb;
      const int bchunk = t + 2 < 9 ? c : (last ? 0 : c + 1);
      issue_b(bsrc, bchunk, t2, (t + 2) % 3);
#pragma unroll
      for (int i = 0; i < AG_MAX; ++i)
        if (t < 8 && (i & 7) == t) {
          if (last) issue_a_group(i, nxt.ab, 0, wpar ^ 1);
          else issue_a_group(i, cur.ab, c + 1, wpar ^ 1);
        }
      static_assert(AG_MAX <= 8, "at most one window slice per step, in steps 0 .. AG_MAX - 1");
      if (t < 8 && t < AG_MAX) c3_wait_vm<B_LOADS + 1>(); else c3_wait_vm<B_LOADS>();
      c3_barrier();
    }
    wpar ^= 1;
  };

  for (;;) {
    const long long nlid = lid + G;
    long long nxt_tile; int nxt_half;
    const bool has_next = pick(nlid, nxt_tile, nxt_half);
    setup(nxt_tile, nxt_half, nxt);
    // accumulators start from the bias (read from LDS straight into the accumulator registers): no bias add in the epilogue, and
    // max-pooling the sums commutes with it
    {
      const float* bl = sbias + cur.n0 + wn * (BN / WGN) + 4 * fhalf;
#pragma unroll
      for (int i = 0; i < NTL; ++i)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const c3_f32x4 bv = *(const c3_f32x4*)(bl + i * 32 + 8 * g4);
#pragma unroll
          for (int j = 0; j < MT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][4 * g4 + e] = bv[e];
        }
    }
    bool idle_done = false;
    if constexpr (HT) {
      if (!active) {
        for (int c = 0; c + 1 < nchunks; ++c) idle_chunk(false, c);
        idle_chunk(true, nchunks - 1);
        idle_done = true;
      }
    }
    if (!idle_done) {
      for (int c = 0; c + 1 < nchunks; ++c) chunk(std::false_type{}, c);
      chunk(std::true_type{}, nchunks - 1);
      mma_group(pend);      // the tile's last group
    }

    // ---- epilogue from registers: lane owns channels 8 g4 + 4 fhalf .. + 3 of pixel l31 of each (i, j) tile ----
    // ReLU (always on in this network: the launcher sends relu == 0 to the non-persistent kernel) on the packed bf16 pairs as an
    // integer max (sign bit set <=> negative), fp32: fmaxf. Addresses: 64-bit tile base on the scalar unit + a 32-bit lane
    // offset (per-lane 64-bit pixel arithmetic with quarter-rate v_mul_lo_u32 / v_mad_u64_u32 was a third of this epilogue).
#ifdef CTPN_ABLATION
    // timing-only ablations (CTPN_C3_P_ABL, -DCTPN_ABLATION builds only). CAVEAT (round 3): a layer that does not store feeds ZEROS to the
    // next one (the activation buffers start zeroed), and MFMAs on zero operands draw less power -- the whole stack then clocks ~15 %
    // higher. Compare CYCLES (GRBM_GUI_ACTIVE, tools/r3_pmc_epi.sh), not time: by cycles the stores cost 0-3 % of a layer, not the
    // 17 % of the stack round 2 read off the clock.
    const bool do_epi = g.abl != 1;
    const bool st_on = g.abl != 2;
#else
    constexpr bool st_on = true, do_epi = true;
#endif
    typedef short c3_s16x2 __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(1))) char* c3_gptr;
#ifdef CTPN_ABLATION
    const c3_gptr hot = (c3_gptr)(uintptr_t)(g.out ? g.out : g.pool_out);
#endif
    auto relu_pk = [](uint32_t p) -> uint32_t {
      const c3_s16x2 z = {0, 0};
      return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(c3_s16x2, p), z));
    };
    // fp32 sums -> one packed 16-bit pair. PL = 0: the 16-bit modes (convert, ReLU as an integer max on the pair); SPLIT: ReLU in fp32,
    // then PL = 1: the hi plane RNE_bf16(v), PL = 2: the lo plane RNE_bf16(v - hi) (may be negative: no ReLU on the packed pair)
    auto pack = [&](auto plc, float x, float y) -> uint32_t {
      constexpr int PL = decltype(plc)::value;
      if constexpr (PL == 0) {
        if constexpr (sizeof(OutT) == 2) return relu_pk(c3_cvt_pk<OutT>(x, y)); else return 0u;      // (fp32 kernels never pack)
      } else {
        x = __builtin_fmaxf(x, 0.f); y = __builtin_fmaxf(y, 0.f);
        uint32_t hi, lo;
        ctpn_split_pk_bf16(x, y, hi, lo);
        return PL == 1 ? hi : lo;
      }
    };
    const int opitch = SPLIT ? g.out_pitch : g.Co;       // 16-bit elements per output pixel
    // 16-byte stores of 8 (bf16) / 4 (fp32) consecutive channels of accumulator tile a; dst = this lane's pixel, first channel of the tile
    auto store_tile_pl = [&](auto plc, c3_gptr dst, bool ok, const c3_f32x16& a) {
      if constexpr (sizeof(OutT) == 4) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const c3_f32x4 o = {__builtin_fmaxf(a[4 * g4], 0.f), __builtin_fmaxf(a[4 * g4 + 1], 0.f), __builtin_fmaxf(a[4 * g4 + 2], 0.f), __builtin_fmaxf(a[4 * g4 + 3], 0.f)};
          if (ok) *(__attribute__((address_space(1))) c3_f32x4*)(dst + (8 * g4 + 4 * fhalf) * 4) = o;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const uint32_t e0 = pack(plc, a[8 * q + 0], a[8 * q + 1]), e1 = pack(plc, a[8 * q + 2], a[8 * q + 3]);
          const uint32_t o0 = pack(plc, a[8 * q + 4], a[8 * q + 5]), o1 = pack(plc, a[8 * q + 6], a[8 * q + 7]);
          const auto r0 = __builtin_amdgcn_permlane32_swap(e0, o0, false, false);   // low lanes: even group complete, high lanes: odd group
          const auto r1 = __builtin_amdgcn_permlane32_swap(e1, o1, false, false);
          const c3_u32x4 v = {r0[0], r1[0], r0[1], r1[1]};
#ifdef CTPN_ABLATION
          if (g.abl == 5) dst = hot;            // timing only: the same store instructions, all aimed at one hot KiB (no write stream)
#endif
          if (ok && st_on) *(__attribute__((address_space(1))) c3_u32x4*)(dst + (16 * q + 8 * fhalf) * 2) = v;
        }
      }
    };
    // bf16, two pixels per lane: after the two 16-byte pieces (q = 0, 1) of a lane's pixel are formed, v_permlane16_swap exchanges
    // piece 1 of lanes r with piece 0 of lanes r + 16, so that store A carries pixels 0..15 of the tile row and store B pixels 16..31,
    // FOUR lanes (64 contiguous bytes) per pixel instead of two: a store instruction touches 16 lines instead of 32 (the texture
    // path's cost per store is its number of distinct lines -- conv1_1 went from 0.61 to 0.45 ms on exactly that). Lane L stores
    // piece 2 * ((L >> 4) & 1) + (L >> 5) of pixel (L & 15) [A] / 16 + (L & 15) [B]; dstA / dstB: that pixel, first channel of tile a.
    const int piece_off = (2 * ((lane >> 4) & 1) + fhalf) * 16;
    auto store_pair_pl = [&](auto plc, c3_gptr dstA, bool okA, c3_gptr dstB, bool okB, bool haveB, const c3_f32x16& a) {
      c3_u32x4 v[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const uint32_t e0 = pack(plc, a[8 * q + 0], a[8 * q + 1]), e1 = pack(plc, a[8 * q + 2], a[8 * q + 3]);
        const uint32_t o0 = pack(plc, a[8 * q + 4], a[8 * q + 5]), o1 = pack(plc, a[8 * q + 6], a[8 * q + 7]);
        const auto r0 = __builtin_amdgcn_permlane32_swap(e0, o0, false, false);
        const auto r1 = __builtin_amdgcn_permlane32_swap(e1, o1, false, false);
        v[q] = c3_u32x4{r0[0], r1[0], r0[1], r1[1]};
      }
      c3_u32x4 va, vb;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const auto r = __builtin_amdgcn_permlane16_swap(v[0][c], v[1][c], false, false);
        va[c] = r[0]; vb[c] = r[1];
      }
#ifdef CTPN_ABLATION
      if (g.abl == 5) { dstA = hot; dstB = hot; }
#endif
      if (okA && st_on) *(__attribute__((address_space(1))) c3_u32x4*)(dstA + piece_off) = va;
      if (haveB && okB && st_on) *(__attribute__((address_space(1))) c3_u32x4*)(dstB + piece_off) = vb;
    };
    // one store per plane: the 16-bit modes write their single plane; SPLIT writes hi at the channel, lo at Co + channel (and hi once more
    // at 2 Co + channel when the consumer is the LSTM projection GEMM)
    const size_t plane_b = (size_t)g.Co * 2;
    auto store_tile = [&](c3_gptr dst, bool ok, const c3_f32x16& a) {
      if constexpr (!SPLIT) store_tile_pl(std::integral_constant<int, 0>{}, dst, ok, a);
      else {
        store_tile_pl(std::integral_constant<int, 1>{}, dst, ok, a);
        store_tile_pl(std::integral_constant<int, 2>{}, dst + plane_b, ok, a);
        if (g.dup_hi) store_tile_pl(std::integral_constant<int, 1>{}, dst + 2 * plane_b, ok, a);
      }
    };
    auto store_pair = [&](c3_gptr dstA, bool okA, c3_gptr dstB, bool okB, bool haveB, const c3_f32x16& a) {
      if constexpr (!SPLIT) store_pair_pl(std::integral_constant<int, 0>{}, dstA, okA, dstB, okB, haveB, a);
      else {
        store_pair_pl(std::integral_constant<int, 1>{}, dstA, okA, dstB, okB, haveB, a);
        store_pair_pl(std::integral_constant<int, 2>{}, dstA + plane_b, okA, dstB + plane_b, okB, haveB, a);
        if (g.dup_hi) store_pair_pl(std::integral_constant<int, 1>{}, dstA + 2 * plane_b, okA, dstB + 2 * plane_b, okB, haveB, a);
      }
    };
    auto usgpr = [](unsigned v) -> unsigned { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); };
    auto gbase = [&](const void* base, unsigned pix, int ch) -> c3_gptr {     // uniform: base + (pix * Co + ch) * sizeof(OutT), pinned to SGPRs
      const unsigned long long a = (unsigned long long)(uintptr_t)base + ((unsigned long long)pix * (unsigned)opitch + (unsigned)ch) * sizeof(OutT);
      const unsigned lo = usgpr((unsigned)a), hi = usgpr((unsigned)(a >> 32));
      return (c3_gptr)(uintptr_t)(((unsigned long long)hi << 32) | lo);
    };
    const int ch0 = cur.n0 + wn * (BN / WGN);                                  // first channel of this wave
    // lane-dependent address terms are recomputed per tile ON PURPOSE: as loop invariants hipcc hoists them out of the tile loop,
    // where they stay live across the K loop -- at 256 VGPRs that means scratch reloads (and their vmcnt(0)) inside the load pipeline
    int lq = l31;
    asm volatile("" : "+v"(lq));
    if (g.out && do_epi && (!HT || active)) {
      if constexpr (FLAT) {
        char* ob = (char*)g.out;
#pragma unroll
        for (int j = 0; j < MT; ++j) {
          const long long q = cur.q0 + (wm * MT + j) * 32 + l31;
          const long long per = (long long)Hp * Wp;
          const long long im = q / per;
          const int rem = (int)(q - im * per);
          const int yb = rem / Wp, xb = rem - yb * Wp;
          const bool ok = q < g.m_total && yb >= 1 && yb <= g.H && xb >= 1 && xb <= g.W;
#pragma unroll
          for (int i = 0; i < NTL; ++i) {
            const int co = ch0 + i * 32;
            store_tile((c3_gptr)(uintptr_t)(ob + (q * opitch + co) * (long long)sizeof(OutT)), ok && co < g.Co, acc[i][j]);
          }
        }
      } else {
        // is output row `prow` of the tile an interior row? per image: below H. Stacked tile rows (a tile spans at most two images:
        // the launcher stacks only for H >= 16): the bordered row inside its image must be 1 .. H, and the row must lie inside the batch
        auto rowok = [&](int prow) -> bool {
          if (!g.stacked) return cur.y0 + prow < g.H;
          int rr = cur.rbase + prow;
          rr = rr >= Hp ? rr - Hp : rr;
          return rr >= 1 && rr <= g.H && cur.y0 + 1 + prow < g.N * Hp;
        };
        // tile origin on the scalar unit; this lane's pixel inside the tile: row prow(j), column lcol
        const unsigned tpix = usgpr((unsigned)((cur.img * Hp + cur.y0 + 1) * Wp + cur.x0 + 1));
        const c3_gptr tb = gbase(g.out, tpix, ch0);
        if constexpr (sizeof(OutT) == 2) {
          // pixels (lq & 15) [store A] and 16 + (lq & 15) [store B] of tile row j: 8 x 32 patches: same row, 16 columns apart;
          // 16 x 16 patches: rows 2 jj and 2 jj + 1 (the second row's lane order is rotated, c3_tw16_col)
          const int l15 = lq & 15;
          const int colA = l15, colB = TW == 32 ? 16 + l15 : c3_tw16_col(16 + l15);
#pragma unroll
          for (int j = 0; j < MT; ++j) {
            const int prowA = TW == 32 ? wm * MT + j : 2 * (wm * MT + j), prowB = TW == 32 ? prowA : prowA + 1;
            const bool okA = rowok(prowA) && cur.x0 + colA < g.W, okB = rowok(prowB) && cur.x0 + colB < g.W;
            const uint32_t offA = (uint32_t)((prowA * Wp + colA) * opitch) * 2u, offB = (uint32_t)((prowB * Wp + colB) * opitch) * 2u;
#pragma unroll
            for (int i = 0; i < NTL; ++i) {
              const bool cok = ch0 + i * 32 < g.Co;
              store_pair(tb + (size_t)offA + i * 64, okA && cok, tb + (size_t)offB + i * 64, okB && cok, true, acc[i][j]);
            }
          }
        } else {
        const int lcol = TW == 32 ? lq : c3_tw16_col(lq);
#pragma unroll
        for (int j = 0; j < MT; ++j) {
          const int prow = TW == 32 ? wm * MT + j : 2 * (wm * MT + j) + (lq >> 4);
          const bool ok = rowok(prow) && cur.x0 + lcol < g.W;
          const uint32_t loff = (uint32_t)((prow * Wp + lcol) * opitch) * (uint32_t)sizeof(OutT);
#pragma unroll
          for (int i = 0; i < NTL; ++i)
            store_tile(tb + (size_t)loff + i * 32 * (int)sizeof(OutT), ok && ch0 + i * 32 < g.Co, acc[i][j]);
        }
        }
      }
    }
    if constexpr (POOL) if (do_epi && (!HT || active)) {
      // max commutes with the bias (already in the sums), ReLU and the rounding: pool the sums. Vertical partner: the wave's other pixel
      // row (8 x 32 patches: same lane of tile j = 1) or a ds_bpermute partner (16 x 16 patches: a tile is two rows of 16); horizontal
      // partner: lane ^ 1. Lanes 2k / 2k+1 share a pooled pixel: the even one keeps channel tile 0, the odd one tile 1.
      const int Ho = g.H >> 1, Wo = g.W >> 1;
      const bool odd = (lq & 1) != 0;
      const unsigned ppix = usgpr((unsigned)((cur.img * (Ho + 2) + (cur.y0 >> 1) + 1) * (Wo + 2) + (cur.x0 >> 1) + 1));
      const c3_gptr pb = gbase(g.pool_out, ppix, ch0);
      auto hpool = [&](const c3_f32x16& v0, const c3_f32x16& v1, int Yl, int Xl, bool keep) {
        // v0 / v1: vertically pooled sums of channel tile 0 / 1 for this lane's column; (Yl, Xl): pooled pixel inside the tile
        c3_f32x16 mine;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          // own / send exactly as before the rewrite: ONE cross-lane move per element, made opaque right away. (Written as
          // max(v, dpp(v)) for both channel tiles with the select afterwards, hipcc sank the whole computation into the store's
          // exec-masked block and kept a single DPP move for all 16 elements: wrong pooled values, caught by the parity tests.)
          const float own = odd ? v1[r] : v0[r], send = odd ? v0[r] : v1[r];
          float recv = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, true));
          asm volatile("" : "+v"(recv));
          mine[r] = __builtin_fmaxf(own, recv);
        }
        const int co = ch0 + (odd ? 32 : 0);
        if constexpr (sizeof(OutT) == 2) {
          // lanes 2k / 2k+1 hold channel tile 0 / 1 of pooled pixel k: with the 16-lane exchange (store_pair) store A writes pooled pixels
          // 0..7 of the row as full 128-byte lines (8 lanes each), store B pixels 8..15 (8 x 32 patches; a 16 x 16 patch has 8 pooled
          // pixels per row pair and its lanes 16..31 hold nothing to store: ONE store instead of two half-empty ones)
          (void)Xl; (void)keep;
          const int xa = (lq & 15) >> 1, xb = 8 + xa;
          const bool rowok = (cur.y0 >> 1) + Yl < Ho && co < g.Co;
          const uint32_t offA = (uint32_t)((Yl * (Wo + 2) + xa) * opitch + (odd ? 32 : 0)) * 2u;
          store_pair(pb + (size_t)offA, rowok && (cur.x0 >> 1) + xa < Wo, pb + (size_t)offA + (size_t)(8 * opitch) * 2u,
                     rowok && (cur.x0 >> 1) + xb < Wo, TW == 32, mine);
        } else {
          const uint32_t loff = (uint32_t)((Yl * (Wo + 2) + Xl) * opitch + (odd ? 32 : 0)) * (uint32_t)sizeof(OutT);
          store_tile(pb + (size_t)loff, keep && (cur.y0 >> 1) + Yl < Ho && (cur.x0 >> 1) + Xl < Wo && co < g.Co, mine);
        }
      };
      if constexpr (NTL == 1) {
        // ONE channel tile per wave: lanes 2k / 2k + 1 end up with the same 32 channels of pooled pixel k; the even one stores them (store A:
        // pooled pixels 0..7 of the row, four lanes = 64 contiguous bytes each; store B: pixels 8..15)
        c3_f32x16 mine;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = __builtin_fmaxf(acc[0][0][r], acc[0][1][r]);
          float recv = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
          asm volatile("" : "+v"(recv));          // (see hpool: one cross-lane move per element, opaque right away)
          mine[r] = __builtin_fmaxf(v, recv);
        }
        if constexpr (sizeof(OutT) == 2) {
          const int xa = (lq & 15) >> 1, xb = 8 + xa;
          const bool rok = (cur.y0 >> 1) + wm < Ho && ch0 < g.Co && !odd;
          const uint32_t offA = (uint32_t)((wm * (Wo + 2) + xa) * opitch) * 2u;
          store_pair(pb + (size_t)offA, rok && (cur.x0 >> 1) + xa < Wo, pb + (size_t)offA + (size_t)(8 * opitch) * 2u, rok && (cur.x0 >> 1) + xb < Wo, true, mine);
        } else {
          const int Xl = lq >> 1;
          const uint32_t loff = (uint32_t)((wm * (Wo + 2) + Xl) * opitch) * (uint32_t)sizeof(OutT);
          store_tile(pb + (size_t)loff, !odd && (cur.y0 >> 1) + wm < Ho && (cur.x0 >> 1) + Xl < Wo && ch0 < g.Co, mine);
        }
      } else if constexpr (TW == 32) {
        c3_f32x16 v0, v1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { v0[r] = __builtin_fmaxf(acc[0][0][r], acc[0][1][r]); v1[r] = __builtin_fmaxf(acc[NTL - 1][0][r], acc[NTL - 1][1][r]); }
        hpool(v0, v1, wm, lq >> 1, true);
      } else {
        // vertical partner under the rotated lane order (c3_tw16_col): row 0 lane c <-> row 1 lane 16 + ((c + 2) & 15)
        const int vpart = ((lane & 32) | ((lq & 16) ? ((lq - 2) & 15) : 16 + ((lq + 2) & 15))) << 2;
#pragma unroll
        for (int j = 0; j < MT; ++j) {
          c3_f32x16 v0, v1;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float a0 = acc[0][j][r], a1 = acc[NTL - 1][j][r];
            float b0 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(vpart, __builtin_bit_cast(int, a0)));   // same column, other row
            float b1 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(vpart, __builtin_bit_cast(int, a1)));
            asm volatile("" : "+v"(b0), "+v"(b1));          // cross-lane results pinned outside the store's exec-masked block (see hpool)
            v0[r] = __builtin_fmaxf(a0, b0); v1[r] = __builtin_fmaxf(a1, b1);
          }
          hpool(v0, v1, wm * MT + j, (lq & 15) >> 1, (lq & 16) == 0);
        }
      }
    }
    if (!has_next) break;
    lid = nlid;
    cur = nxt;
    cur_tile = nxt_tile; cur_half = nxt_half;
    if constexpr (HT) active = cur_half < 0 || wm < 2;
  }
  c3_wait_vm<0>();   // the dummy prefetch of the last tile
}

template <typename T, bool FLAT, bool POOL, int TW, bool SPLIT = false, int BN_T = 128, int BM_T = 256, bool HT32 = false>
static int c3_launch_p(Conv3 g, hipStream_t s, const C3Walk& wk) {
  constexpr int BN = BN_T;
  constexpr int BMF = BM_T;                    // pixels per flat-window tile (256; 64: the one-image form)
  constexpr bool HTF = ((FLAT || TW == 16) && BMF == 256) || HT32;      // the kernel's HT
  // the walk (tiles, stacked tile rows, the grid, the half-tile tail: c3_walk, conv3x3_plan.h) was laid out for this instantiation
  if (wk.flat != (FLAT ? 1 : 0) || wk.tw != TW || wk.bn != BN || wk.bm != BMF || wk.ht != (HTF ? 1 : 0))
    return fail(CTPN_ERR_STATE, "conv3x3: the walk was planned for another form of the persistent kernel");
  const int Wp = g.W + 2;
  const int rows = FLAT ? (BMF + 2 * Wp + 2) : (C3_BM / TW + 2) * (TW + 2);
  g.a_rows = (rows + 7) & ~7;
  constexpr int AG_MAX = FLAT ? ((BMF == 64 ? 37 : 61) + 7) / 8 : (43 + 7) / 8;
  if ((g.a_rows >> 3) > AG_MAX * 8) return fail(CTPN_ERR_ARG, "conv3x3: input window does not fit the staging plan");
  g.tiles_n = wk.tiles_n;
  if (FLAT) g.m_total = wk.m_total;
  else { g.tiles_x = wk.tiles_x; g.tiles_y = wk.tiles_y; g.stacked = wk.stacked; }
  g.ptiles_total = wk.ptiles_total;
#ifdef CTPN_ABLATION
  { static const int abl = [] { const char* e = std::getenv("CTPN_C3_P_ABL"); return e ? std::atoi(e) : 0; }(); g.abl = abl; }
#endif
  if (g.ptiles_total <= 0 || (long long)g.N * (g.H + 2) * Wp > 0x7fffffffLL) return fail(CTPN_ERR_ARG, "conv3x3: problem out of range");
  const int lds = 2 * g.a_rows * 128 + 3 * BN * 128 + g.tiles_n * BN * 4;
  if (lds > C3_LDS_MAX) return fail(CTPN_ERR_ARG, "conv3x3: LDS budget exceeded");
  int dev = 0, rc;
  if ((rc = current_device(dev))) return rc;
  const long long workers = wk.workers;
  g.ht_full = wk.ht_full; g.ht_r = wk.ht_r;
  // Every form of the kernel reads its fragments one k-slice group ahead of the MFMAs through a second register set, with no LDS read in
  // flight across a barrier. History: round 3 had kept a plain loop for 16 x 16 patches and flat windows (+-0 / +1 % there) -- but it was only
  // as fast as it was because hipcc let the last k-slice group's reads straddle the barrier, which is a write-after-read race against the
  // LDS-DMA that recycles the strip (see the INVARIANT in the kernel; profiles/r06_barrier_war.txt). With the wait it needed to be correct the
  // plain loop was 0.7 % (bf16) / 0.8 % (split) slower per batch of 32 than before; reading ahead everywhere was 0.3 % / 1.2 % FASTER than
  // before (3660 against 3645 and 1165 against 1151 images/s on one box), at 207 .. 246 VGPRs and no scratch. The plain loop was removed.
  static bool attr[CTPN_MAX_DEV] = {false};      // per instantiation and device
  auto k = conv3x3_p_kernel<T, T, FLAT, POOL, TW, SPLIT, BN_T, BM_T, HT32>;
  if ((rc = raise_dynamic_lds((const void*)k, C3_LDS_MAX, attr, dev))) return rc;
  hipLaunchKernelGGL(k, dim3((unsigned)workers), dim3(512), lds, s, g);
  return launch_status("conv3x3_p");
}
}  // namespace ctpn
