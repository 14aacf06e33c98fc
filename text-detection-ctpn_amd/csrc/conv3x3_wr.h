// conv3x3_wr_kernel (Ci = 64 layers of the 16-bit modes, fused conv1_1 producer) and its launch template c3_launch_wr; shared helpers: conv3x3_base.h
#pragma once
#include "conv3x3_base.h"
namespace ctpn {

// ---------------------------------------------------------------------------------------------
// Weights-in-REGISTERS persistent kernel for the Ci = 64 layers in bf16 (conv1_2: 64 -> 64 + pool, conv2_1: 64 -> 128).
// Round 1's weights-stationary kernel (nine weight strips in LDS; removed in round 3) spent ~21 instructions per MFMA (address
// arithmetic for 144 swizzled fragment reads and 11 window pieces per tile, 186 accvgpr copies): issue-bound at 51 % MFMA busy. Here:
//   * a workgroup (4 waves, one per SIMD, 512 registers each) owns 64 output channels and walks 8 x 32-pixel tiles; wave
//     (ph, ch) computes pixel rows 4 ph .. 4 ph + 3 x channels 32 ch .. + 31: all 36 weight fragments of its 32 channels
//     (9 taps x 4 k-slices x 16 B per lane = 144 VGPRs) are loaded ONCE and stay in registers -- no weight traffic in LDS at all;
//   * the LDS holds only input windows, three of them, with a PADDED 144-byte pixel pitch instead of the XOR swizzle: bank
//     group = (9 row + slot) mod 16 is conflict-free for the ds_read_b128 lane groups and, unlike the swizzle, AFFINE -- every
//     fragment read of a tile is `ds_read_b128 v, vbase offset:imm` off ONE address register;
//   * the window pieces are `global_load_lds_dwordx4 voff, s[base]`: the per-lane source offsets of a wave's 12 pieces are
//     tile-independent (computed once), the tile enters through a scalar base -- one VMEM instruction per KiB, no VALU. Windows
//     are fetched WITHOUT clamping at the image edge: reads past the last bordered row / image run into the next rows / the slack
//     the ctx allocates behind every activation buffer; those window pixels only feed outputs that are never stored;
//   * the K loop is ordered by INPUT row: fragment (row r, kx, k-slice q) is read once and feeds every (output row j, ky) with
//     j + ky = r: 72 reads for 144 MFMAs per wave and tile (was 144), issued PD = 8 slots ahead through a register ring with
//     counted lgkmcnt, across tile boundaries;
//   * the epilogue of tile k (bias, ReLU, 2 x 2 pool via DPP, bf16 pack, 16-byte stores) runs on a second accumulator set,
//     interleaved piece by piece with the MFMAs of tile k + 1; window k + 2 is issued inside the same stream;
//   * tiles are CLAIMED, not statically partitioned: a workgroup's first five tiles are fixed (worker + i * nworkers), every later
//     one comes from a device-scope atomic counter, fetched by one lane five tiles ahead and handed to the other waves through
//     an LDS word behind the regular tile barrier. The proposal-stream kernels of the previous batch (sort, NMS: one 1024-thread
//     workgroup per image for up to a millisecond) share the GPU with conv1_2 / conv2_1 of the next batch, and a persistent
//     workgroup that needs a whole CU (147 KB of LDS, 432 registers per lane) cannot start on a CU an NMS workgroup occupies:
//     with a static partition those late starters still had their full share to do and the launch ended ~0.3 ms late;
//   * ONE s_barrier per tile, PD slots into it: by then every wave has drained its reads of window k - 1 (buffer of k + 2)
//     and `vmcnt(0)` there covers window k + 1 (issued a whole tile earlier) -- no counted vmcnt, no dump page.
// ---------------------------------------------------------------------------------------------
struct Conv3WR {
  const void* in; const void* wt; const float* bias; void* out; void* pool_out;
  int N, H, W, Co;
  int tiles_x, tiles_y, tiles_n;
  unsigned ptiles;                 // N * tiles_x * tiles_y
  unsigned groups, per_group;      // tile ranges: workgroup b belongs to group b % groups (8 = one per XCD: the hardware deals consecutive
                                   // workgroup ids round-robin over the XCDs) and walks tiles [grp * per_group, min(.. + per_group, ptiles))
  unsigned magic_img, magic_row;   // floor(2^32 / d) + 1 for d = tiles_x * tiles_y and d = tiles_x (exact for pt * d < 2^32)
  char* dump;                      // 4 KB per workgroup: where lanes outside the image store, so that every wave issues the same number of stores
  unsigned* claim;                 // [groups][tiles_n][2] = {tiles handed out beyond the static ones, workgroups that have finished}; zero between launches
  // FUSE (conv1_2 with conv1_1 computed in its window stage): the q-image of the batch (common.h), its geometry, conv1_1's fragments
  const void* q; const void* wfq;
  int Hq, Wq;
};

constexpr int WR_PITCH = 144, WR_PW = 34, WR_ROWS = 10 * WR_PW, WR_PIECES = 48, WR_WIN = WR_PIECES * 1024, WR_NBUF = 3, WR_PD = 8;
static_assert(WR_ROWS * WR_PITCH <= WR_WIN, "window must fit its pieces");

template <int... I, typename F>
__device__ __forceinline__ void c3_static_for_impl(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void c3_static_for(F&& f) { c3_static_for_impl(std::make_integer_sequence<int, N>{}, f); }

// "+v" / "+a": the destination is declared read-write although the instruction only writes it. That ties every new value to
// the register of the old one, so ring slots and accumulators stay IN PLACE across the tile loop's back edge; as plain
// outputs the register allocator gave each definition a fresh register and glued the loop together with 128 v_accvgpr_mov +
// 32 v_mov per iteration.
template <int OFF, bool XA = false>
__device__ __forceinline__ void c3_ds_read_b128_off(c3_u32x4& dst, uint32_t lds_addr) {
  if constexpr (XA) asm volatile("ds_read_b128 %0, %1 offset:%2" : "+a"(dst) : "v"(lds_addr), "n"(OFF));
  else asm volatile("ds_read_b128 %0, %1 offset:%2" : "+v"(dst) : "v"(lds_addr), "n"(OFF));
}
// One K slot of the weights-in-registers kernel as ONE asm block: wait for the ring's oldest fragment x, run the slot's 1..3 MFMAs
// on it (one per output row it feeds), refill the ring slot with the fragment PD slots ahead. Register files: the 36 weight
// fragments live in AGPRs (MFMA A operand), the two accumulator sets (128), the bias vector and the ring in VGPRs, tied in place
// ("+v") -- so the epilogue is plain C++ on accumulator elements. (Accumulators in AGPRs needed a v_accvgpr_read per element from
// asm, whose "a" input hipcc sometimes fed with a v_accvgpr_write right in front of it: a hazard it cannot see into the asm for.) INIT = index
// of the MFMA that starts its accumulator's chain for this tile (C operand = the bias vector), -1 = none.
// Hazards the compiler no longer sees, all satisfied by construction: a dependent MFMA on exactly the same accumulator (same
// opcode) is interlocked by the hardware; x comes from LDS behind the block's own s_waitcnt, the weights were loaded once at
// kernel start; the ds_read overwrites x, an A/B operand of MFMAs issued before it (in-order issue; only SrcC has a WAR window);
// the VALU reads an accumulator set (v_accvgpr_read in the epilogue pieces) no earlier than PD + 1 slots after its last MFMA
// and no later than 9 slots before its next one.
// XC: register file of the ring fragments x -- "+v", or "+a" in the fused kernel (ds_read_b128 loads accumulation registers as well, and
// an MFMA takes either operand from them): its 32 ring registers move out of the VGPR file to make room for the producer
#define C3_DEFINE_SLOTS(SFX, MN, XC) \
template <int OFF, int WAIT, int INIT> \
__device__ __forceinline__ void c3_slot1##SFX(c3_f32x16& a0, const c3_u32x4& w0, c3_u32x4& x, uint32_t xaddr, const c3_f32x16& bias) { \
  if constexpr (INIT == 0) \
    asm volatile("s_waitcnt lgkmcnt(%6)\n\t" MN "%0, %2, %1, %3\n\tds_read_b128 %1, %4 offset:%5" \
                 : "+v"(a0), XC(x) : "a"(w0), "v"(bias), "v"(xaddr), "n"(OFF), "n"(WAIT)); \
  else \
    asm volatile("s_waitcnt lgkmcnt(%5)\n\t" MN "%0, %2, %1, %0\n\tds_read_b128 %1, %3 offset:%4" \
                 : "+v"(a0), XC(x) : "a"(w0), "v"(xaddr), "n"(OFF), "n"(WAIT)); \
} \
template <int OFF, int WAIT, int INIT> \
__device__ __forceinline__ void c3_slot2##SFX(c3_f32x16& a0, c3_f32x16& a1, const c3_u32x4& w0, const c3_u32x4& w1, c3_u32x4& x, uint32_t xaddr, \
                                         const c3_f32x16& bias) { \
  if constexpr (INIT == 0) \
    asm volatile("s_waitcnt lgkmcnt(%8)\n\t" MN "%0, %3, %2, %5\n\t" MN "%1, %4, %2, %1\n\tds_read_b128 %2, %6 offset:%7" \
                 : "+v"(a0), "+v"(a1), XC(x) : "a"(w0), "a"(w1), "v"(bias), "v"(xaddr), "n"(OFF), "n"(WAIT)); \
  else if constexpr (INIT == 1) \
    asm volatile("s_waitcnt lgkmcnt(%8)\n\t" MN "%0, %3, %2, %0\n\t" MN "%1, %4, %2, %5\n\tds_read_b128 %2, %6 offset:%7" \
                 : "+v"(a0), "+v"(a1), XC(x) : "a"(w0), "a"(w1), "v"(bias), "v"(xaddr), "n"(OFF), "n"(WAIT)); \
  else \
    asm volatile("s_waitcnt lgkmcnt(%7)\n\t" MN "%0, %3, %2, %0\n\t" MN "%1, %4, %2, %1\n\tds_read_b128 %2, %5 offset:%6" \
                 : "+v"(a0), "+v"(a1), XC(x) : "a"(w0), "a"(w1), "v"(xaddr), "n"(OFF), "n"(WAIT)); \
} \
template <int OFF, int WAIT> \
__device__ __forceinline__ void c3_slot3##SFX(c3_f32x16& a0, c3_f32x16& a1, c3_f32x16& a2, const c3_u32x4& w0, const c3_u32x4& w1, const c3_u32x4& w2, \
                                         c3_u32x4& x, uint32_t xaddr) { \
  asm volatile("s_waitcnt lgkmcnt(%9)\n\t" MN "%0, %4, %3, %0\n\t" MN "%1, %5, %3, %1\n\t" MN "%2, %6, %3, %2\n\tds_read_b128 %3, %7 offset:%8" \
               : "+v"(a0), "+v"(a1), "+v"(a2), XC(x) : "a"(w0), "a"(w1), "a"(w2), "v"(xaddr), "n"(OFF), "n"(WAIT)); \
}
C3_DEFINE_SLOTS(_bf16, "v_mfma_f32_32x32x16_bf16 ", "+v")
C3_DEFINE_SLOTS(_f16, "v_mfma_f32_32x32x16_f16 ", "+v")
C3_DEFINE_SLOTS(_bf16a, "v_mfma_f32_32x32x16_bf16 ", "+a")
C3_DEFINE_SLOTS(_f16a, "v_mfma_f32_32x32x16_f16 ", "+a")
#undef C3_DEFINE_SLOTS
template <bool F16, bool XA, int OFF, int WAIT, int INIT>
__device__ __forceinline__ void c3_slot1(c3_f32x16& a0, const c3_u32x4& w0, c3_u32x4& x, uint32_t xaddr, const c3_f32x16& bias) {
  if constexpr (F16 && XA) c3_slot1_f16a<OFF, WAIT, INIT>(a0, w0, x, xaddr, bias);
  else if constexpr (F16) c3_slot1_f16<OFF, WAIT, INIT>(a0, w0, x, xaddr, bias);
  else if constexpr (XA) c3_slot1_bf16a<OFF, WAIT, INIT>(a0, w0, x, xaddr, bias);
  else c3_slot1_bf16<OFF, WAIT, INIT>(a0, w0, x, xaddr, bias);
}
template <bool F16, bool XA, int OFF, int WAIT, int INIT>
__device__ __forceinline__ void c3_slot2(c3_f32x16& a0, c3_f32x16& a1, const c3_u32x4& w0, const c3_u32x4& w1, c3_u32x4& x, uint32_t xaddr, const c3_f32x16& bias) {
  if constexpr (F16 && XA) c3_slot2_f16a<OFF, WAIT, INIT>(a0, a1, w0, w1, x, xaddr, bias);
  else if constexpr (F16) c3_slot2_f16<OFF, WAIT, INIT>(a0, a1, w0, w1, x, xaddr, bias);
  else if constexpr (XA) c3_slot2_bf16a<OFF, WAIT, INIT>(a0, a1, w0, w1, x, xaddr, bias);
  else c3_slot2_bf16<OFF, WAIT, INIT>(a0, a1, w0, w1, x, xaddr, bias);
}
template <bool F16, bool XA, int OFF, int WAIT>
__device__ __forceinline__ void c3_slot3(c3_f32x16& a0, c3_f32x16& a1, c3_f32x16& a2, const c3_u32x4& w0, const c3_u32x4& w1, const c3_u32x4& w2, c3_u32x4& x, uint32_t xaddr) {
  if constexpr (F16 && XA) c3_slot3_f16a<OFF, WAIT>(a0, a1, a2, w0, w1, w2, x, xaddr);
  else if constexpr (F16) c3_slot3_f16<OFF, WAIT>(a0, a1, a2, w0, w1, w2, x, xaddr);
  else if constexpr (XA) c3_slot3_bf16a<OFF, WAIT>(a0, a1, a2, w0, w1, w2, x, xaddr);
  else c3_slot3_bf16<OFF, WAIT>(a0, a1, a2, w0, w1, w2, x, xaddr);
}

// slot n of a tile -> fragment (input row r, kx, k-slice q): the input rows are paired (0,5), (1,4), (2,3) and interleaved, so that
// consecutive MFMAs never form a chain on ONE accumulator (rows 0 and 5 feed a single output row each)
__host__ __device__ constexpr int wr_slot_r(int n) { return ((n % 24) & 1) == 0 ? n / 24 : 5 - n / 24; }
__host__ __device__ constexpr int wr_slot_kx(int n) { return ((n % 24) / 2) / 4; }
__host__ __device__ constexpr int wr_slot_q(int n) { return ((n % 24) / 2) % 4; }
__host__ __device__ constexpr int wr_slot_off(int n) { return (wr_slot_r(n) * WR_PW + wr_slot_kx(n)) * WR_PITCH + wr_slot_q(n) * 32; }
// is (slot n, ky) the first MFMA of the tile on accumulator j = r - ky? (it takes the bias as its C operand)
__host__ __device__ constexpr bool wr_first_touch(int n, int ky) {
  const int j = wr_slot_r(n) - ky;
  for (int m = 0; m <= n; ++m)
    for (int k2 = 0; k2 < 3; ++k2) {
      const int j2 = wr_slot_r(m) - k2;
      if (j2 != j) continue;
      return m == n && k2 == ky;      // MFMAs of one slot run in ascending ky
    }
  return false;
}

// ---------------------------------------------------------------------------------------------
// FUSE: conv1_1 (reference VGGnet_test.py:20-22, the layer in front of conv1_2) computed INSIDE conv1_2's window stage. The 12 LDS-DMA
// pieces that fetched window k + 2 from conv1_1's stored output (69 MB per 600 x 900 image, written once and read back once) are replaced by
//   * ONE 1-KiB LDS-DMA per wave and tile: the 12 x 36-pixel patch of the q-image (common.h: 8-byte pixels (q_B, q_G, q_R, P), 4.7 MB per
//     image) under tile k + 3, into one of two 4-KiB planes;
//   * a producer for window k + 2 threaded through the tile's slots: the window's 340 pixels are 4 waves x 85, each wave's 85 as three
//     32-pixel MFMA groups (the third overlaps the second by 11 pixels: identical values written twice); per group three ds_read2_b64
//     (tap rows ky = 0..2; lanes 0..31 read q-pixels (x - 1, x), lanes 32..63 (x, x + 1): K-slot order in conv_first_q.hip, pack_conv1_frags),
//     2 x 3 MFMAs (two 32-channel halves, ky = 0, 1, 2 from a zero accumulator) and 2 x 4 epilogue pieces (two packed converts, the
//     ReLU as a packed integer max, one ds_write_b64 into the window buffer at the 144-byte pixel pitch -- two-way bank-conflicted; the
//     conflict-free ds_write_b128 form behind v_permlane32_swap measured 0.5 % slower);
//   * window pixels outside the image (conv1_2's SAME padding; the overhang of ragged tiles) read their operands from a zero region
//     instead: zero operands, zero sums (the bias rides on the centre pixel's P), zero after the ReLU -- no masking of results.
// Every producer LDS operation and MFMA is its own asm statement in a fixed slot (fq_* below), at most ONE LDS operation per slot, so the
// ring's counted waits stay exact: slot n waits with lgkmcnt(7 + the producer's operations of the eight slots before it). A fragment read
// is consumed >= 9 slots after its issue (the ring wait of that slot covers it), an accumulator is read by the epilogue's VALU >= 2
// slots after its last MFMA. 18 MFMAs per wave on top of the tile's 144.
// conv_first_p_kernel (conv_first_q.hip) runs the same MFMA sequence on the same operands from global memory: what keep_acts stores.
// ---------------------------------------------------------------------------------------------
constexpr int FQ_PW = 36, FQ_ROWB = FQ_PW * 8, FQ_PLANE = 4096;
constexpr int FQ_PLANE_OFF = WR_NBUF * WR_WIN + 16, FQ_ZERO_OFF = FQ_PLANE_OFF + 2 * FQ_PLANE, FQ_LDS = FQ_ZERO_OFF + 1024;
static_assert(12 * FQ_ROWB <= FQ_PLANE && 3 * FQ_ROWB <= 1024 && FQ_LDS <= C3_LDS_MAX, "q planes / zero region");
__host__ __device__ constexpr int fq_goff(int gi) { return gi == 0 ? 0 : (gi == 1 ? 32 : 53); }      // first window pixel of a wave's group gi, relative to 85 * wave
// pieces by slot (-1: none). setup: group; read: gi * 3 + ky; mma: (gi * 2 + i) * 3 + ky; epi: (gi * 2 + i) * 4 + h
__host__ __device__ constexpr int fq_setup(int n) { return n == 9 ? 0 : (n == 13 ? 1 : (n == 30 ? 2 : -1)); }
__host__ __device__ constexpr int fq_read(int n) { return (n >= 10 && n <= 12) ? n - 10 : ((n >= 14 && n <= 16) ? 3 + n - 14 : ((n >= 36 && n <= 38) ? 6 + n - 36 : -1)); }
__host__ __device__ constexpr int fq_mma(int n) {
  return (n >= 24 && n <= 29) ? n - 24 : ((n >= 32 && n <= 34) ? 6 + n - 32 : ((n >= 36 && n <= 38) ? 9 + n - 36 : ((n >= 48 && n <= 53) ? 12 + n - 48 : -1)));
}
__host__ __device__ constexpr int fq_epi(int n) { return (n >= 28 && n <= 35) ? n - 28 : ((n >= 39 && n <= 46) ? 8 + n - 39 : ((n >= 54 && n <= 61) ? 16 + n - 54 : -1)); }
constexpr int FQ_INCOMING = 17, FQ_DMA = 18;
__host__ __device__ constexpr int fq_lds_ops(int n) { return (fq_read(n) >= 0 ? 1 : 0) + (fq_epi(n) >= 0 ? 1 : 0); }
// lgkmcnt of slot n: the ring read it waits for was issued in slot n - 8; behind it: 7 ring reads, the producer's operations of slots
// n - 8 .. n - 1 (a slot's pieces follow its ring read) and the queue word read in front of slot 8's ring read (every wave issues it)
// (left at 7 the waits are merely stricter: measured 0.2 % slower, profiles/r04_ab_conv1_fuse.txt)
__host__ __device__ constexpr int fq_wait(int n) {
  int w = WR_PD - 1 + ((n >= 8 && n <= 15) ? 1 : 0);
  for (int m = n - 8; m < n; ++m) w += fq_lds_ops((m + 72) % 72);
  return w > 15 ? 15 : w;
}

// the hand schedule's invariants, checked at compile time (edit the tables above and this tells what broke)
__host__ __device__ constexpr int fq_slot_of(int kind, int id) {      // kind: 0 setup, 1 read, 2 mma, 3 epi
  for (int n = 0; n < 72; ++n)
    if ((kind == 0 ? fq_setup(n) : kind == 1 ? fq_read(n) : kind == 2 ? fq_mma(n) : fq_epi(n)) == id) return n;
  return -1;
}
__host__ __device__ constexpr bool fq_schedule_ok() {
  for (int n = 0; n < 72; ++n) {
    if (fq_lds_ops(n) > 1) return false;                                                   // the lgkmcnt table assumes at most one per slot
    // behind the barrier; the last LDS write early enough that slot 7's wait of the NEXT tile (in front of its barrier) has retired it:
    // a write in slot s has (71 - s) + 7 ring reads behind it there, the wait leaves 7 (+ 1 if slot 71 holds an operation) in flight
    if ((fq_setup(n) >= 0 || fq_lds_ops(n) || fq_mma(n) >= 0) && (n <= WR_PD || n > 69)) return false;
  }
  if (!(FQ_INCOMING > WR_PD + 8 && FQ_DMA > FQ_INCOMING && FQ_DMA < WR_PD + 1 + 12)) return false;      // queue word complete; base a slot ahead; loads in front of the stores
  for (int gi = 0; gi < 3; ++gi) {
    if (fq_slot_of(0, gi) < 0 || fq_slot_of(0, gi) >= fq_slot_of(1, gi * 3)) return false;               // address before the reads
    for (int ky = 0; ky < 3; ++ky) {
      const int r = fq_slot_of(1, gi * 3 + ky);
      if (r < 0) return false;
      for (int i = 0; i < 2; ++i) {
        const int m = fq_slot_of(2, (gi * 2 + i) * 3 + ky);
        if (m < r + 9) return false;                                                        // the ring wait of slot r + 9 covers the read
        if (ky > 0 && m <= fq_slot_of(2, (gi * 2 + i) * 3 + ky - 1)) return false;            // the chain in order, one MFMA per slot
      }
      // operand set (gi & 1) and its address register are rewritten for group gi + 2 only after group gi's last use (in-slot order: mma, then read)
      if (gi + 2 < 3 && (fq_slot_of(1, (gi + 2) * 3 + ky) < fq_slot_of(2, (gi * 2 + 1) * 3 + ky) || fq_slot_of(0, gi + 2) <= fq_slot_of(1, gi * 3 + 2))) return false;
    }
    for (int i = 0; i < 2; ++i)
      for (int h = 0; h < 4; ++h) {
        const int e = fq_slot_of(3, (gi * 2 + i) * 4 + h);
        if (e < fq_slot_of(2, (gi * 2 + i) * 3 + 2) + 2) return false;                      // MFMA result -> VALU read
        if (gi + 1 < 3 && fq_slot_of(2, ((gi + 1) * 2 + i) * 3) < e) return false;           // accumulator i is overwritten after its epilogue (in-slot order: epi, then mma)
      }
  }
  return true;
}
static_assert(fq_schedule_ok(), "producer schedule violates one of its invariants");

typedef uint32_t c3_u32x2 __attribute__((ext_vector_type(2)));
// the producer's instructions, one asm statement each (operands in the accumulation file: "a")
template <int O0, int O1>
__device__ __forceinline__ void c3_fq_read2(c3_u32x4& dst, uint32_t addr) {
  asm volatile("ds_read2_b64 %0, %1 offset0:%2 offset1:%3" : "+a"(dst) : "v"(addr), "n"(O0), "n"(O1));
}
template <bool F16, bool FIRST>
__device__ __forceinline__ void c3_fq_mfma(c3_f32x16& acc, const c3_u32x4& w, const c3_u32x4& x) {
  if constexpr (FIRST) {
    if constexpr (F16) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "+v"(acc) : "a"(w), "a"(x));
    else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "+v"(acc) : "a"(w), "a"(x));
  } else {
    if constexpr (F16) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "a"(x));
    else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "a"(x));
  }
}
template <int OFF>
__device__ __forceinline__ void c3_fq_write(uint32_t addr, const c3_u32x2& d) {
  asm volatile("ds_write_b64 %0, %1 offset:%2" : : "v"(addr), "v"(d), "n"(OFF) : "memory");
}
// ABL (measurement only, wrong results): 1 = no window DMA after the prologue, 2 = no epilogue
template <typename HF, bool POOL, bool FULL, int ABL = 0, bool FUSE = false>
__global__ __launch_bounds__(256, 1) void conv3x3_wr_kernel(Conv3WR g) {
  constexpr bool F16 = std::is_same<HF, h_f16>::value;
  static_assert(POOL || FULL, "nothing to store");
  static_assert(!FUSE || (POOL && !FULL && ABL == 0), "the fused form is conv1_2's production launch");
  constexpr int PD = WR_PD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ph = wave & 1, chh = wave >> 1;
  const int l31 = lane & 31, fhalf = lane >> 5;
  const int H = g.H, W = g.W, Co = g.Co, Wp = W + 2, Hp = H + 2;
  const int tiles_n = g.tiles_n, tiles_x = g.tiles_x;
  const unsigned per_img = (unsigned)(g.tiles_x * g.tiles_y);
  const unsigned magic_img = g.magic_img, magic_row = g.magic_row;
  // XCD-local tile ranges: every XCD (own L2) walks ONE contiguous band of tiles -- and, for Co = 128, walks it with BOTH channel slices.
  // With tiles dealt w, w + nworkers, ... over the whole grid, x- and y-neighbours (which share a third of their 10 x 34 window) and the
  // two slices of a tile (which read the SAME window) sat on different XCDs, so every L2 fetched its own copy: conv2_1 read 2.5 x its
  // input from HBM, conv1_2 1.3 x. `ptiles` below is the END of this workgroup's range; dynamic claims come from the group's own counter.
  const unsigned grp = blockIdx.x % g.groups, kq = blockIdx.x / g.groups;
  const int tn = (int)(kq % (unsigned)tiles_n);
  const int n0 = tn * 64 + chh * 32;                        // this wave's first output channel
  const unsigned worker = kq / (unsigned)tiles_n, nworkers = gridDim.x / (g.groups * (unsigned)tiles_n);
  const unsigned range_lo = grp * g.per_group;
  const unsigned ptiles = range_lo + g.per_group < g.ptiles ? range_lo + g.per_group : g.ptiles;     // end of the range (may be <= range_lo: empty)
  const char* const in_base = (const char*)g.in;

  // ---- weights and bias of this wave's 32 channels: registers, once ----
  c3_u32x4 wf[9][4];
  {
    const char* wp = (const char*)g.wt + (size_t)(n0 + l31) * (9 * 64 * 2) + fhalf * 16;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) wf[t][q] = *(const c3_u32x4*)(wp + t * 128 + q * 32);
  }
  // the bias enters as the accumulators' initial value (C operand of each tile's first MFMA per pixel row): no add in the epilogue
  c3_f32x16 bias16;
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const c3_f32x4 b4 = *(const c3_f32x4*)(g.bias + n0 + 8 * g4 + 4 * fhalf);
#pragma unroll
    for (int e = 0; e < 4; ++e) bias16[4 * g4 + e] = b4[e];
  }

  // ---- window pieces of this wave: piece P = wave + 4 i covers LDS bytes [1024 P, 1024 P + 1024) of a window buffer ----
  uint32_t voff[FUSE ? 1 : 12];
  if constexpr (!FUSE) {
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int o = (wave + 4 * i) * 1024 + lane * 16;
      int row = o / WR_PITCH;
      int slot = (o - row * WR_PITCH) >> 4;
      if (row >= WR_ROWS || slot == 8) { row = 0; slot = 0; }   // pad slots / tail of the last piece: any valid 16 bytes
      const int i2 = row / WR_PW, j2 = row - i2 * WR_PW;
      voff[i] = (uint32_t)((i2 * Wp + j2) * 128 + slot * 16);
    }
  }
  // ---- FUSE: the producer's per-lane constants ----
  // fq_rd[gi]: LDS address (plane 0) of this lane's 16 operand bytes of tap row 0, group gi; fq_rc[gi]: the group pixel's window row | column << 8;
  // fq_wr: this lane's write address in window buffer 0 for group offset 0; voff[0]: source offset of its 16 bytes of the q patch
  uint32_t fq_rd[3] = {0u, 0u, 0u}, fq_rc[3] = {0u, 0u, 0u}, fq_wr = 0u;
  c3_u32x4 wq[6];
  if constexpr (FUSE) {
#pragma unroll
    for (int gi = 0; gi < 3; ++gi) {
      const int p = 85 * wave + fq_goff(gi) + l31;                 // < 340
      const int r = p / WR_PW, c = p - r * WR_PW;
      fq_rd[gi] = lds0 + (uint32_t)(FQ_PLANE_OFF + (r * FQ_PW + c + fhalf) * 8);
      fq_rc[gi] = (uint32_t)(r | (c << 8));
    }
    fq_wr = lds0 + (uint32_t)((85 * wave + l31) * WR_PITCH + 8 * fhalf);
    int j = wave * 64 + lane;                                      // 16-byte chunk of the 12 x 288-byte patch; the plane's tail: any valid bytes
    if (j >= 12 * (FQ_ROWB / 16)) j = 0;
    const int row = j / (FQ_ROWB / 16), cc = j - row * (FQ_ROWB / 16);
    voff[0] = (uint32_t)(row * g.Wq * 8 + cc * 16);
    const char* wp = (const char*)g.wfq + lane * 16;
#pragma unroll
    for (int k = 0; k < 6; ++k) wq[k] = *(const c3_u32x4*)(wp + k * 1024);
  }
  // tile bookkeeping is wave-uniform: kept on the scalar unit (readfirstlane pins the values to SGPRs; the divisions are
  // multiplications by host-computed reciprocals)
  auto sgpr = [](unsigned v) -> unsigned { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); };
  auto mulhi = [](unsigned a, unsigned b) -> unsigned { return (unsigned)(((unsigned long long)a * (unsigned long long)b) >> 32); };
  auto tile_coords = [&](unsigned pt, int& img, int& y0, int& x0) {
    pt = sgpr(pt);
    // (a divisor of 1 has no 32-bit reciprocal of this form: floor(2^32 / 1) + 1 wraps -- one tile per image / one tile column)
    const unsigned im = per_img == 1u ? pt : mulhi(pt, magic_img);
    const unsigned rem = pt - im * per_img;
    const unsigned ty = tiles_x == 1 ? rem : mulhi(rem, magic_row);
    img = (int)sgpr(im); y0 = (int)sgpr(ty * 8u); x0 = (int)sgpr((rem - ty * (unsigned)tiles_x) * 32u);
  };
  auto window_base = [&](unsigned pt) -> const char* {
    int img, y0, x0;
    tile_coords(pt, img, y0, x0);
    const unsigned pix = sgpr((unsigned)((img * Hp + y0) * Wp + x0));           // < 2^31 (checked by the launcher)
    const unsigned long long a = (unsigned long long)(uintptr_t)in_base + ((unsigned long long)pix << 7);
    const unsigned lo = sgpr((unsigned)a), hi = sgpr((unsigned)(a >> 32));
    return (const char*)(uintptr_t)(((unsigned long long)hi << 32) | lo);
  };
  auto issue_piece = [&](auto ic, const char* sbase, uint32_t buf_lds) {
    constexpr int i = decltype(ic)::value;
    c3_glds16_saddr(sbase, voff[i], __builtin_amdgcn_readfirstlane(buf_lds + (wave + 4 * i) * 1024));
  };
  // FUSE: the q patch under tile pt starts at q pixel (y0, x0) of its image (image pixel (y0 - 2, x0 - 2)); one 1-KiB piece per wave
  auto q_base = [&](unsigned pt) -> const char* {
    int img, y0, x0;
    tile_coords(pt, img, y0, x0);
    const unsigned pix = sgpr((unsigned)((img * g.Hq + y0) * g.Wq + x0));       // < 2^31 (checked by the launcher)
    const unsigned long long a = (unsigned long long)(uintptr_t)g.q + ((unsigned long long)pix << 3);
    const unsigned lo = sgpr((unsigned)a), hi = sgpr((unsigned)(a >> 32));
    return (const char*)(uintptr_t)(((unsigned long long)hi << 32) | lo);
  };
  auto issue_plane = [&](const char* sbase, int plane) {
    c3_glds16_saddr(sbase, voff[0], __builtin_amdgcn_readfirstlane(lds0 + FQ_PLANE_OFF + plane * FQ_PLANE + wave * 1024));
  };
  // ---- FUSE: the producer's pieces (kernel comment). Operand sets xq[gi & 1][ky] and the 24 weight fragment registers live in the
  // accumulation file; the two accumulators (one per 32-channel half) in VGPRs, tied in place like everything else asm writes ----
  c3_u32x4 xq[2][3];
  c3_f32x16 pacc[2];
  uint32_t fq_a[2] = {0u, 0u};                // operand address of the group whose reads are in flight, per operand set
  if constexpr (FUSE) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int k = 0; k < 3; ++k) xq[a][k] = c3_u32x4{0u, 0u, 0u, 0u};
      pacc[a] = c3_f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    }
  }
  // window pixel (r, c) of the tile at (y2, x2) is image pixel (y2 + r - 1, x2 + c - 1); outside the image its operands come from the zero region
  auto fq_setup_piece = [&](auto gic, int y2, int x2, uint32_t plane_off) {
    constexpr int gi = decltype(gic)::value;
    const uint32_t r = fq_rc[gi] & 0xffu, c = fq_rc[gi] >> 8;
    const bool in = (r + (uint32_t)(y2 - 1)) < (uint32_t)H && (c + (uint32_t)(x2 - 1)) < (uint32_t)W;
    fq_a[gi & 1] = in ? fq_rd[gi] + plane_off : lds0 + (uint32_t)FQ_ZERO_OFF;
  };
  auto fq_read_piece = [&](auto gic, auto kyc) {
    constexpr int gi = decltype(gic)::value, ky = decltype(kyc)::value;
    c3_fq_read2<ky * FQ_PW, ky * FQ_PW + 1>(xq[gi & 1][ky], fq_a[gi & 1]);
  };
  auto fq_mma_piece = [&](auto gic, auto ic, auto kyc) {
    constexpr int gi = decltype(gic)::value, i = decltype(ic)::value, ky = decltype(kyc)::value;
    c3_fq_mfma<F16, ky == 0>(pacc[i], wq[i * 3 + ky], xq[gi & 1][ky]);
  };
  // a lane owns channels 32 i + 8 h + 4 fhalf + e (accumulator element 4 h + e) of window pixel 85 wave + goff + l31: 8 bytes per piece
  auto fq_epi_piece = [&](auto gic, auto ic, auto hc, uint32_t wbuf) {
    constexpr int gi = decltype(gic)::value, i = decltype(ic)::value, h = decltype(hc)::value;
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    auto rp = [](uint32_t u) -> uint32_t { return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, u), s16x2{0, 0})); };
    c3_u32x2 d;
    d[0] = rp(c3_cvt_pk<HF>(pacc[i][4 * h], pacc[i][4 * h + 1]));
    d[1] = rp(c3_cvt_pk<HF>(pacc[i][4 * h + 2], pacc[i][4 * h + 3]));
    c3_fq_write<fq_goff(gi) * WR_PITCH + 64 * i + 16 * h>(wbuf, d);
  };
  // one whole window, back to back (prologue): plane -> window buffer
  auto fq_produce_sync = [&](unsigned pt, int plane, uint32_t wbuf) {
    int img, y2, x2;
    tile_coords(pt, img, y2, x2);
    c3_static_for<3>([&](auto gic) {
      fq_setup_piece(gic, y2, x2, (uint32_t)(plane * FQ_PLANE));
      c3_static_for<3>([&](auto kyc) { fq_read_piece(gic, kyc); });
      c3_wait_lgkm<0>();
      c3_static_for<2>([&](auto ic) {
        c3_static_for<3>([&](auto kyc) { fq_mma_piece(gic, ic, kyc); });
      });
      asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");      // MFMA result -> VALU read
      __builtin_amdgcn_sched_barrier(0);
      c3_static_for<2>([&](auto ic) {
        c3_static_for<4>([&](auto hc) { fq_epi_piece(gic, ic, hc, wbuf); });
      });
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  // ---- tile queue: t[k] (current), t[k+1], t[k+2] (its window is issued during tile k); t[k+3] arrives during tile k ----
  // static: t[i] = worker + i * nworkers for i < 5; dynamic: 5 * nworkers + (old value of the slice's counter). An index >= ptiles
  // means "no tile": the walk ends at the first one.
  unsigned* claim_ctr;
  {
    const unsigned long long a = (unsigned long long)(uintptr_t)(g.claim + 2 * (grp * (unsigned)tiles_n + (unsigned)tn));
    const unsigned lo = sgpr((unsigned)a), hi = sgpr((unsigned)(a >> 32));          // pinned to an SGPR pair (asm "s" operand below)
    claim_ctr = (unsigned*)(uintptr_t)(((unsigned long long)hi << 32) | lo);
  }
  const unsigned claim_base = sgpr(range_lo + 5u * nworkers);
  const uint32_t claim_lds = lds0 + WR_NBUF * WR_WIN;           // two words, alternating by tile parity
  // The fetched value and the word read back from LDS arrive ASYNCHRONOUSLY into their destination registers; hipcc, which takes an
  // asm's outputs as ready when the asm ends, must never touch them before the covering wait (a first version returned into a
  // VGPR that hipcc, short of VGPRs, copied to an AGPR in the very next instruction -- i.e. before the atomic had returned:
  // every workgroup then claimed the same tile for ever). Both therefore live in AGPRs (plenty are free, nothing spills them),
  // tied in place ("+a"), and are only read by asm that runs behind the wait.
  auto claim_issue = [&](uint32_t& ret) {                        // wave 0, lane 0: fetch-and-add; the result is read a tile later
    if (wave == 0 && lane == 0) {
      const uint32_t zero = 0u, one = 1u;
      asm volatile("global_atomic_add %0, %1, %2, %3 sc0" : "+a"(ret) : "v"(zero), "a"(one), "s"(claim_ctr) : "memory");   // one ACC bit covers vdst and vdata
    }
  };
  auto claim_publish = [&](uint32_t& ret, unsigned word) {       // wave 0, lane 0: the value fetched during the previous tile -> LDS
    if (wave == 0 && lane == 0) {
      const uint32_t a = claim_lds + 4 * word;
      uint32_t tmp;
      asm volatile("v_accvgpr_read_b32 %0, %1\n\tv_add_u32 %0, %0, %3\n\tds_write_b32 %2, %0" : "=&v"(tmp) : "a"(ret), "v"(a), "s"(claim_base) : "memory");
    }
  };
  auto claim_read = [&](uint32_t& dst, unsigned word) {          // every lane of every wave (same address: broadcast)
    const uint32_t a = claim_lds + 4 * word;
    asm volatile("ds_read_b32 %0, %1" : "+a"(dst) : "v"(a));
  };
  auto claim_value = [&](uint32_t& dst) -> unsigned {            // behind the ring waits that cover claim_read (slot PD + 8 and later)
    uint32_t v;
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(dst));
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
  };
  unsigned q0 = range_lo + worker, q1 = q0 + nworkers, q2 = q0 + 2 * nworkers;
  if (q0 >= ptiles) {                                            // nothing to do (never with the launcher's grid); still counts as finished
    if (tid == 0) {
      const unsigned done = __hip_atomic_fetch_add(claim_ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (done == nworkers - 1) { __hip_atomic_store(claim_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_store(claim_ctr + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    }
    return;
  }
  // ---- prologue: windows of the first two tiles ----
  if constexpr (!FUSE) {
    const char* b0 = window_base(q0);
    const char* b1 = window_base(q1 < ptiles ? q1 : q0);
    c3_static_for<12>([&](auto ic) { issue_piece(ic, b0, lds0); });
    c3_static_for<12>([&](auto ic) { issue_piece(ic, b1, lds0 + WR_WIN); });
  } else {
    // zero region; patches of the first two tiles; their windows, produced back to back; then the third tile's patch into plane 0
    {
      const uint32_t za = lds0 + (uint32_t)FQ_ZERO_OFF + 4u * (uint32_t)tid, zero = 0u;
      asm volatile("ds_write_b32 %0, %1" : : "v"(za), "v"(zero) : "memory");
    }
    // (the scalar bases are fresh from v_readfirstlane: VALU-written SGPR -> VMEM address needs five wait states, and hipcc pads nothing
    // for an asm statement -- all three bases first, then a nop, then the loads)
    const char* const pb0 = q_base(q0);
    const char* const pb1 = q_base(q1 < ptiles ? q1 : q0);
    const char* const pb2 = q_base(q2 < ptiles ? q2 : q0);
    asm volatile("s_nop 4" ::: "memory");
    issue_plane(pb0, 0);
    issue_plane(pb1, 1);
    c3_wait_vm<0>();
    c3_wait_lgkm<0>();
    c3_barrier();
    fq_produce_sync(q0, 0, fq_wr);
    fq_produce_sync(q1 < ptiles ? q1 : q0, 1, fq_wr + (uint32_t)WR_WIN);
    c3_wait_lgkm<0>();
    c3_barrier();                               // every wave is done with both planes
    issue_plane(pb2, 0);
  }
  const uint32_t xbase = lds0 + (uint32_t)((4 * ph * WR_PW + l31) * WR_PITCH + fhalf * 16);
  c3_wait_vm<0>();
  if constexpr (FUSE) c3_wait_lgkm<0>();
  c3_barrier();

  c3_u32x4 xr[PD];
  c3_f32x16 acc[2][4];
#pragma unroll
  for (int i = 0; i < PD; ++i) xr[i] = c3_u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[a][j] = bias16;
  // fragment read of slot n = (input row r, kx, k-slice q), see wr_slot_*
  auto read_frag = [&](auto nc, uint32_t xaddr) {
    constexpr int n = decltype(nc)::value;
    c3_ds_read_b128_off<wr_slot_off(n), FUSE>(xr[n % PD], xaddr);
  };
  c3_static_for<PD>([&](auto nc) { read_frag(nc, xbase); });   // tile 0, buffer 0

  int p_img = 0, p_y0 = 0, p_x0 = 0;     // previous tile (its epilogue runs inside the current one)
  bool p_valid = false;

  // ---- epilogue of the tile at (img, y0, x0) on accumulator set `es`, in small pieces (a few VALU each, so that they hide in
  // the gaps between the next tile's MFMAs) ----
  // The bias entered through the accumulators' initial value (bias16 below), ReLU is a packed integer max on the bf16 pairs
  // (sign bit set <=> negative). A lane owns channels 8 g4 + 4 fhalf + e of pixel column l31 of each of its 4 pixel rows;
  // v_permlane32_swap pairs the two half-waves so that every lane stores 8 consecutive channels (16 bytes).
  typedef short c3_s16x2 __attribute__((ext_vector_type(2)));
  auto relu_pk = [](uint32_t p) -> uint32_t {
    const c3_s16x2 z = {0, 0};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(c3_s16x2, p), z));
  };
  uint32_t pk[8];                         // packed bf16 pairs of the piece group in flight: pk[2 g4 + h] = channels 8 g4 + 4 fhalf + 2 h, + 1
  float pm[2];                            // pool: the two values of the pair being built
  // Store addressing: scalar 64-bit row base (SALU) + per-lane 32-bit byte offset computed once per kernel -> the store is
  // `global_store_dwordx4 voff, data, s[base] offset:imm`. (Per-lane 64-bit pixel arithmetic cost two v_mad_u64_u32 + two
  // v_mul_lo_u32 -- quarter-rate -- per 16-byte store: the full-resolution epilogue took 40 % of conv2_1's time.)
  typedef __attribute__((address_space(1))) char* c3_gptr;     // global address space: a pointer rebuilt from integers would otherwise be
                                                               // generic, i.e. a flat_store, which also counts in lgkmcnt
  const c3_gptr dump_lane = (c3_gptr)(uintptr_t)(g.dump + (size_t)blockIdx.x * 4096 + tid * 16);
  // Every store is ALWAYS issued (lanes outside the image write to the dump page): the number of stores per tile is a compile-time
  // constant, which is what lets the tile barrier wait with a counted vmcnt for "everything but my newest stores"
  auto sbase64 = [&](const void* base, unsigned long long byte_off) -> c3_gptr {     // uniform pointer pinned to an SGPR pair
    const unsigned long long a = (unsigned long long)(uintptr_t)base + byte_off;
    const unsigned lo = sgpr((unsigned)a), hi = sgpr((unsigned)(a >> 32));
    return (c3_gptr)(uintptr_t)(((unsigned long long)hi << 32) | lo);
  };
  const int co_shift = Co == 64 ? 7 : 8;                                                                 // bytes per pixel = Co * 2 (Co is 64 or 128)
  // pool: piece i (0..15) = accumulator element idx i: vertical max over the wave's own rows (2 jp, 2 jp + 1), horizontal max
  // with lane ^ 1 (DPP quad_perm [1,0,3,2]); lanes 2k / 2k+1 then hold the same two pooled pixels: the even lane keeps pooled
  // row 0 of the wave, the odd lane pooled row 1. max commutes with the bias, the ReLU and the bf16 rounding.
  auto pool_elem = [&](auto esc, auto ic) {
    constexpr int es = decltype(esc)::value, idx = decltype(ic)::value;
    const bool odd = (lane & 1) != 0;
    const float v0 = __builtin_fmaxf(acc[es][0][idx], acc[es][1][idx]), v1 = __builtin_fmaxf(acc[es][2][idx], acc[es][3][idx]);
    // the lane keeps `own` and sends the other pooled row to its partner: one cross-lane move per element, pinned by an empty asm
    // (cross-lane results that only feed a later store are otherwise fair game for hipcc's sinking, see conv3x3_p_kernel's hpool)
    const float own = odd ? v1 : v0, send = odd ? v0 : v1;
    float recv = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, true));
    asm volatile("" : "+v"(recv));
    pm[idx & 1] = __builtin_fmaxf(own, recv);
    if constexpr (idx & 1) pk[idx >> 1] = relu_pk(c3_cvt_pk<HF>(pm[0], pm[1]));
  };
  // both 16-byte pieces of a pooled pixel are stored by the second call, after the 16-lane exchange described at full_piece: store A
  // carries pooled columns 0..7 (both pooled rows of the wave), store B columns 8..15, four consecutive lanes per pixel
  const uint32_t pool_pair_off = (uint32_t)(((lane & 1) * ((W >> 1) + 2) + ((l31 & 15) >> 1)) * Co * 2 + (2 * ((lane >> 4) & 1) + fhalf) * 16);
  auto pool_store = [&](auto qc, int img, int y0, int x0, bool valid) {
    constexpr int q2 = decltype(qc)::value;
    if constexpr (q2 == 1) {
      const bool odd = (lane & 1) != 0;
      const int Ho = H >> 1, Wo = W >> 1;
      const int Ys = (y0 >> 1) + 2 * ph, Xs = x0 >> 1;                     // wave-uniform: first pooled row / column of this wave
      const unsigned pix = sgpr((unsigned)((img * (Ho + 2) + Ys + 1) * (Wo + 2) + Xs + 1));
      const c3_gptr rb = sbase64(g.pool_out, ((unsigned long long)pix << co_shift) + (unsigned)(n0 * 2));
      c3_u32x4 v[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const auto r0 = __builtin_amdgcn_permlane32_swap(pk[4 * q + 0], pk[4 * q + 2], false, false);
        const auto r1 = __builtin_amdgcn_permlane32_swap(pk[4 * q + 1], pk[4 * q + 3], false, false);
        v[q] = c3_u32x4{r0[0], r1[0], r0[1], r1[1]};
      }
      c3_u32x4 va, vb;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const auto r = __builtin_amdgcn_permlane16_swap(v[0][c], v[1][c], false, false);
        va[c] = r[0]; vb[c] = r[1];
      }
      const bool rowok = valid && Ys + (odd ? 1 : 0) < Ho;
      const int xa = (l31 & 15) >> 1;
      const c3_gptr da = rowok && Xs + xa < Wo ? rb + (size_t)pool_pair_off : dump_lane;
      const c3_gptr db = rowok && Xs + 8 + xa < Wo ? rb + (size_t)pool_pair_off + (size_t)(8 * Co * 2) : dump_lane;
      *(__attribute__((address_space(1))) c3_u32x4*)(da) = va;                 // always issued
      *(__attribute__((address_space(1))) c3_u32x4*)(db) = vb;
    }
  };
  // full resolution: piece (j, q2): 8 values of pixel row j -> 4 packed pairs + one 16-byte store
  // The two pieces of a pixel row are stored TOGETHER by the second one: v_permlane16_swap exchanges piece 1 of lanes r with piece 0
  // of lanes r + 16, so that one store carries pixels 0..15 of the row and the other pixels 16..31 with the wave's 64 bytes of a pixel
  // on four consecutive lanes -- 16 distinct lines per store instruction instead of 32 (what a store costs the texture path).
  const uint32_t full_pair_off = (uint32_t)((l31 & 15) * Co * 2 + (2 * ((lane >> 4) & 1) + fhalf) * 16);
  auto full_piece = [&](auto esc, auto jc, auto qc, int img, int y0, int x0, bool valid) {
    constexpr int es = decltype(esc)::value, j = decltype(jc)::value, q2 = decltype(qc)::value;
#pragma unroll
    for (int h = 0; h < 4; ++h) pk[4 * q2 + h] = relu_pk(c3_cvt_pk<HF>(acc[es][j][8 * q2 + 2 * h], acc[es][j][8 * q2 + 2 * h + 1]));
    if constexpr (q2 == 1) {
      const int y = y0 + 4 * ph + j;                                         // wave-uniform
      const unsigned pix = sgpr((unsigned)((img * Hp + y + 1) * Wp + x0 + 1));
      const c3_gptr rb = sbase64(g.out, ((unsigned long long)pix << co_shift) + (unsigned)(n0 * 2));
      c3_u32x4 v[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const auto r0 = __builtin_amdgcn_permlane32_swap(pk[4 * q + 0], pk[4 * q + 2], false, false);
        const auto r1 = __builtin_amdgcn_permlane32_swap(pk[4 * q + 1], pk[4 * q + 3], false, false);
        v[q] = c3_u32x4{r0[0], r1[0], r0[1], r1[1]};
      }
      c3_u32x4 va, vb;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const auto r = __builtin_amdgcn_permlane16_swap(v[0][c], v[1][c], false, false);
        va[c] = r[0]; vb[c] = r[1];
      }
      const bool rowok = valid && y < H;
      // two stores per pixel row, always issued: the same count per tile as with one store per piece
      const c3_gptr da = rowok && x0 + (l31 & 15) < W ? rb + (size_t)full_pair_off : dump_lane;
      const c3_gptr db = rowok && x0 + 16 + (l31 & 15) < W ? rb + (size_t)full_pair_off + (size_t)(16 * Co * 2) : dump_lane;
      *(__attribute__((address_space(1))) c3_u32x4*)(da) = va;
      *(__attribute__((address_space(1))) c3_u32x4*)(db) = vb;
    }
  };
  // piece list of a tile: pool: 16 element pieces, a store after the 8th and the 16th; then full: 8 pieces
  // Slots of a tile: 0 .. PD: nothing but the K loop; PD: barrier; PD + 1 .. PD + 12: the window pieces of tile k + 2 (right behind
  // the barrier: they get a whole tile to land); from E_FIRST on: the epilogue pieces of tile k - 1. Program order per tile is
  // therefore [12 loads][NS stores], and the next barrier waits with vmcnt(NS): all loads have landed, the stores (whose
  // acknowledgements take microseconds under load) stay in flight for another tile.
  constexpr int NE = (POOL ? 18 : 0) + (FULL ? 8 : 0);
  constexpr int NS = (POOL ? 2 : 0) + (FULL ? 8 : 0);         // 16-byte stores per wave and tile
  constexpr int D_FIRST = PD + 1, E_FIRST = D_FIRST + 12, E_STRIDE = (64 - E_FIRST) / NE;
  static_assert(E_STRIDE >= 1 && E_FIRST + (NE - 1) * E_STRIDE <= 63, "epilogue pieces must fit the tile's slots");
  auto epi_piece = [&](auto esc, auto ec, int img, int y0, int x0, bool valid) {
    constexpr int e = decltype(ec)::value;
    if constexpr (POOL && e < 18) {
      if constexpr (e == 8) pool_store(std::integral_constant<int, 0>{}, img, y0, x0, valid);
      else if constexpr (e == 17) pool_store(std::integral_constant<int, 1>{}, img, y0, x0, valid);
      else pool_elem(esc, std::integral_constant<int, (e < 8 ? e : e - 1)>{});
    } else {
      constexpr int f = e - (POOL ? 18 : 0);
      full_piece(esc, std::integral_constant<int, f / 2>{}, std::integral_constant<int, f % 2>{}, img, y0, x0, valid);
    }
  };

  // ---- one tile on accumulator set `as`; k = its index in this workgroup's walk (q0 = its tile) ----
  uint32_t claim_ret = 0u, claim_val = 0u;      // wave 0 lane 0: counter value fetched during the previous tile; all: the LDS word read this tile
  unsigned bcur = 0, bnext = 1, bdma = 2;       // window buffers of t[k], t[k+1], t[k+2]
  auto tile = [&](auto asc, unsigned k) {
    constexpr int as = decltype(asc)::value;
    k = sgpr(k);
    int c_img, c_y0, c_x0;
    tile_coords(q0, c_img, c_y0, c_x0);
    const char* nbase = nullptr;
    int n_img = 0, n_y0 = 0, n_x0 = 0;                          // FUSE: the tile whose window (k + 2) is produced during this one
    if constexpr (FUSE) tile_coords(q2 < ptiles ? q2 : q0, n_img, n_y0, n_x0);   // past the end: the own window once more, never read
    else nbase = window_base(q2 < ptiles ? q2 : q0);            // past the end: a harmless re-fetch of the own window
    const uint32_t nbuf_lds = sgpr(lds0 + bdma * WR_WIN);
    const uint32_t fq_wbuf = fq_wr + sgpr(bdma * WR_WIN);
    const uint32_t xcur = xbase + sgpr(bcur * WR_WIN);
    const uint32_t xnext = xbase + sgpr((q1 < ptiles ? bnext : bcur) * WR_WIN);   // last tile: dummy reads of its own window
    unsigned incoming = 0u;                                     // t[k + 3]
    const char* dma_base = nullptr;                             // FUSE: its q patch
    c3_static_for<72>([&](auto nc) {
      constexpr int n = decltype(nc)::value;
      constexpr int r = wr_slot_r(n), kx = wr_slot_kx(n), q = wr_slot_q(n);
      if constexpr (n == PD) {
        // every wave has drained its reads of window k - 1 (the ring waits) and, with vmcnt(NS), its pieces of window k + 1
        // (issued during tile k - 1, in front of that tile's NS stores) and wave 0's counter fetch of tile k - 1: after the
        // barrier buffer (k + 2) % 3 may be overwritten and window k + 1 may be read
        // (FUSE: window k + 1 was WRITTEN by the producer during tile k - 1; its last ds_write, slot 61, has 18 ring reads behind it and
        // slot 7's wait leaves at most 15 LDS operations in flight: retired. vmcnt covers the q patch of tile k + 2.)
        c3_wait_vm<(ABL & 2) ? 0 : NS>();
        c3_barrier();
        // tile queue: read the word wave 0 published during tile k - 1 (it sits behind TWO barriers: no wait on the write
        // itself is needed); publish the fetch of tile k - 1 into the other word; fetch the next one. The extra LDS
        // operations only make the ring's counted waits stricter; the word is complete once slot PD + 8 has waited.
        claim_read(claim_val, (k + 1) & 1);
        claim_publish(claim_ret, k & 1);
        claim_issue(claim_ret);
      }
      // the slot: wait for fragment n, its MFMAs (output rows j = r - ky, ascending ky), read of the fragment PD slots ahead
      constexpr int nn = (n + PD) % 72;
      constexpr int off = wr_slot_off(nn);
      constexpr int WT = FUSE ? fq_wait(n) : PD - 1;
      const uint32_t xa = (n + PD < 72) ? xcur : xnext;
      constexpr int j_lo = r - 2 < 0 ? 0 : r - 2, j_hi = r > 3 ? 3 : r;       // output rows fed: j_lo .. j_hi (ky = r - j)
      constexpr int nm = j_hi - j_lo + 1;
      // ascending ky = descending j
      if constexpr (nm == 1) {
        constexpr int ky = r - j_hi;
        c3_slot1<F16, FUSE, off, WT, wr_first_touch(n, ky) ? 0 : -1>(acc[as][j_hi], wf[ky * 3 + kx][q], xr[n % PD], xa, bias16);
      } else if constexpr (nm == 2) {
        constexpr int ky0 = r - j_hi, ky1 = ky0 + 1;
        constexpr int init = wr_first_touch(n, ky0) ? 0 : (wr_first_touch(n, ky1) ? 1 : -1);
        c3_slot2<F16, FUSE, off, WT, init>(acc[as][j_hi], acc[as][j_hi - 1], wf[ky0 * 3 + kx][q], wf[ky1 * 3 + kx][q], xr[n % PD], xa, bias16);
      } else {
        static_assert(!wr_first_touch(n, 0) && !wr_first_touch(n, 1) && !wr_first_touch(n, 2), "three-row slots never start a chain");
        constexpr int ky0 = r - j_hi;
        c3_slot3<F16, FUSE, off, WT>(acc[as][j_hi], acc[as][j_hi - 1], acc[as][j_hi - 2], wf[ky0 * 3 + kx][q], wf[(ky0 + 1) * 3 + kx][q], wf[(ky0 + 2) * 3 + kx][q],
                                     xr[n % PD], xa);
      }
      if constexpr (!FUSE) {
        if constexpr (n >= D_FIRST && n < D_FIRST + 12 && !(ABL & 1)) issue_piece(std::integral_constant<int, n - D_FIRST>{}, nbase, nbuf_lds);
      } else {
        // the producer of window k + 2 (operand plane k & 1 = `as`) and the q patch of tile k + 3 (into the other plane)
        if constexpr (fq_setup(n) >= 0) fq_setup_piece(std::integral_constant<int, fq_setup(n)>{}, n_y0, n_x0, (uint32_t)(as * FQ_PLANE));
        if constexpr (fq_epi(n) >= 0)
          fq_epi_piece(std::integral_constant<int, fq_epi(n) / 8>{}, std::integral_constant<int, (fq_epi(n) / 4) % 2>{}, std::integral_constant<int, fq_epi(n) % 4>{}, fq_wbuf);
        if constexpr (fq_mma(n) >= 0)
          fq_mma_piece(std::integral_constant<int, fq_mma(n) / 6>{}, std::integral_constant<int, (fq_mma(n) / 3) % 2>{}, std::integral_constant<int, fq_mma(n) % 3>{});
        if constexpr (fq_read(n) >= 0) fq_read_piece(std::integral_constant<int, fq_read(n) / 3>{}, std::integral_constant<int, fq_read(n) % 3>{});
        if constexpr (n == FQ_INCOMING) {      // (a slot ahead of the DMA: its scalar base is fresh from readfirstlane)
          incoming = sgpr(k < 2 ? range_lo + worker + (k + 3) * nworkers : claim_value(claim_val));
          dma_base = q_base(incoming < ptiles ? incoming : q0);
        }
        if constexpr (n == FQ_DMA) issue_plane(dma_base, as ^ 1);
      }
      if constexpr (n >= E_FIRST && (n - E_FIRST) % E_STRIDE == 0 && (n - E_FIRST) / E_STRIDE < NE && !(ABL & 2))
        epi_piece(std::integral_constant<int, as ^ 1>{}, std::integral_constant<int, (n - E_FIRST) / E_STRIDE>{}, p_img, p_y0, p_x0, p_valid);
      __builtin_amdgcn_sched_barrier(0);
    });
    p_img = c_img; p_y0 = c_y0; p_x0 = c_x0; p_valid = true;
    // t[k + 3]: static for the first two tiles, then what wave 0 fetched during tile k - 2 (the word read behind this tile's barrier)
    if constexpr (!FUSE) incoming = k < 2 ? range_lo + worker + (k + 3) * nworkers : claim_value(claim_val);
    q0 = q1; q1 = q2; q2 = sgpr(incoming);
    const unsigned b = bcur; bcur = bnext; bnext = bdma; bdma = b;
  };

  unsigned k = 0;
  bool last_set1 = false;
  for (;;) {
    tile(std::integral_constant<int, 0>{}, k);
    last_set1 = false;
    if (q0 >= ptiles) break;
    tile(std::integral_constant<int, 1>{}, k + 1);
    last_set1 = true;
    if (q0 >= ptiles) break;
    k += 2;
  }
  c3_wait_lgkm<0>();
  if (!last_set1) c3_static_for<NE>([&](auto ec) { epi_piece(std::integral_constant<int, 0>{}, ec, p_img, p_y0, p_x0, true); });
  else c3_static_for<NE>([&](auto ec) { epi_piece(std::integral_constant<int, 1>{}, ec, p_img, p_y0, p_x0, true); });
  c3_wait_vm<0>();
  // the last workgroup of the slice to finish re-arms the counters for the next launch (claims all precede a workgroup's exit)
  if (tid == 0) {
    const unsigned done = __hip_atomic_fetch_add(claim_ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (done == nworkers - 1) {
      __hip_atomic_store(claim_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(claim_ctr + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// per-device resources of the weights-in-registers kernel (conv3x3.hip): the dump pages and the next of 64 tile-claim counter slots
int c3_wr_resources(int dev, hipStream_t s, char** dump, unsigned** claim);

template <typename H>
static int c3_launch_wr(const Conv3& c, bool pool, hipStream_t s, int ncu) {
  Conv3WR g{};
  g.in = c.in; g.wt = c.wt; g.bias = c.bias; g.out = c.out; g.pool_out = c.pool_out;
  g.N = c.N; g.H = c.H; g.W = c.W; g.Co = c.Co;
  // tiles, the eight per-XCD tile ranges and the workers of each: c3_walk (conv3x3_plan.h), for ncu CUs (the device's, or a test launch's)
  const C3Walk wk = c3_walk(C3M_WR, c.N, c.H, c.W, c.Co, pool, c.out != nullptr, c.w_cover, ncu);
  g.tiles_x = wk.tiles_x;
  g.tiles_y = wk.tiles_y;
  g.tiles_n = wk.tiles_n;
  const long long ptiles = wk.ptiles;
  const long long per_img = (long long)g.tiles_x * g.tiles_y;
  if (ptiles <= 0 || ptiles * per_img >= (1LL << 32) || (long long)c.N * (c.H + 2) * (c.W + 2) * 128 >= (1LL << 40))
    return fail(CTPN_ERR_ARG, "conv3x3_wr: problem out of range");
  g.ptiles = (unsigned)ptiles;
  g.magic_img = (unsigned)((1ULL << 32) / (unsigned long long)per_img + 1ULL);
  g.magic_row = (unsigned)((1ULL << 32) / (unsigned long long)g.tiles_x + 1ULL);
  int dev = 0, rc;
  if ((rc = current_device(dev))) return rc;
  g.groups = (unsigned)wk.groups;
  g.per_group = (unsigned)wk.per_group;
  const long long workers = wk.workers * wk.groups;                  // per channel slice
  if (workers * g.tiles_n > 1024) return fail(CTPN_ERR_ARG, "conv3x3_wr: more workgroups than dump pages");
  if (g.tiles_n > 4) return fail(CTPN_ERR_ARG, "conv3x3_wr: more channel slices than claim counters per slot");
  if ((rc = c3_wr_resources(dev, s, &g.dump, &g.claim))) return rc;
  const bool fuse = c.q1 != nullptr;
  if (fuse) {
    if (!pool || c.out || c.Co != 64 || !c.q1_frags) return fail(CTPN_ERR_ARG, "conv3x3_wr: the fused conv1_1 form is conv1_2's pooled production launch");
    g.q = c.q1; g.wfq = c.q1_frags; g.Hq = conv1_q_h(c.H); g.Wq = conv1_q_w(c.W);
    // the patch of the last tile must lie inside the q-image (rows y0 .. y0 + 11, columns x0 .. x0 + 35), pixel indices below 2^31
    if (8 * g.tiles_y + 4 > g.Hq || 32 * g.tiles_x + 4 > g.Wq || (long long)c.N * g.Hq * g.Wq >= (1LL << 31))
      return fail(CTPN_ERR_ARG, "conv3x3_wr: q-image geometry out of range");
  }
  const int lds = fuse ? FQ_LDS : WR_NBUF * WR_WIN + 16;
  const dim3 grid((unsigned)(workers * g.tiles_n)), block(256);
  static bool attr[10][CTPN_MAX_DEV] = {{false}};
  auto launch = [&](auto kern, bool (&done)[CTPN_MAX_DEV]) -> int {
    const int r = raise_dynamic_lds((const void*)kern, C3_LDS_MAX, done, dev);
    if (r) return r;
    hipLaunchKernelGGL(kern, grid, block, lds, s, g);
    return CTPN_OK;
  };
#ifdef CTPN_ABLATION
  // CTPN_C3_WR_VAR (measurement builds only, WRONG results): 1 = no window DMA after the prologue, 2 = no epilogue, 3 = neither
  static const int var = [] { const char* e = std::getenv("CTPN_C3_WR_VAR"); return e ? std::atoi(e) : 0; }();
#else
  constexpr int var = 0;
#endif
  if (fuse) rc = launch(conv3x3_wr_kernel<H, true, false, 0, true>, attr[9]);
  else if (pool && c.out) rc = launch(conv3x3_wr_kernel<H, true, true>, attr[0]);
  else if (pool) {
    switch (var) {
#ifdef CTPN_ABLATION
      case 1: rc = launch(conv3x3_wr_kernel<H, true, false, 1>, attr[1]); break;
      case 2: rc = launch(conv3x3_wr_kernel<H, true, false, 2>, attr[2]); break;
      case 3: rc = launch(conv3x3_wr_kernel<H, true, false, 3>, attr[3]); break;
#endif
      default: rc = launch(conv3x3_wr_kernel<H, true, false>, attr[4]);
    }
  } else {
    switch (var) {
#ifdef CTPN_ABLATION
      case 1: rc = launch(conv3x3_wr_kernel<H, false, true, 1>, attr[5]); break;
      case 2: rc = launch(conv3x3_wr_kernel<H, false, true, 2>, attr[6]); break;
      case 3: rc = launch(conv3x3_wr_kernel<H, false, true, 3>, attr[7]); break;
#endif
      default: rc = launch(conv3x3_wr_kernel<H, false, true>, attr[8]);
    }
  }
  if (rc) return rc;
  return launch_status("conv3x3_wr");
}
}  // namespace ctpn
