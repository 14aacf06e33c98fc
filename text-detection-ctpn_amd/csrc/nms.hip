// Proposal layer on device, third stage: greedy NMS over score-sorted boxes (sort_keys.hip) -- the generic kernel and the column-decomposed
// forms, which also serve the text connector's NMS 0.2 (connect.hip). Bit parity with the reference: decode.hip's head comment.
#include "proposal_dev.h"      // (brings common.h)
#include "nms_column_dev.h"    // iou_gt and the per-column body of the column forms
#include "wg_scan.h"

#pragma clang fp contract(off)

namespace ctpn {

// ---------------------------------------------------------------------------------------------
// greedy NMS, one workgroup (16 waves) per image, no N x N mask in HBM.
//
// Candidates are consumed in score order, 64 at a time (one per lane, replicated in every wave):
//   A. wave w tests the 64 candidates against kept boxes w, w+16, ... (kept list cached in LDS, spill in HBM);
//      __ballot turns "suppressed by an earlier keep" into one 64-bit word per wave;
//   B. wave w also builds rows 4w..4w+3 of the 64x64 intra-block suppression bitmask with __ballot
//      (row i = which later candidates box i would suppress) into LDS;
//   C. wave 0 ORs the 16 words, then walks the 64 candidates in order over the LDS bitmask rows
//      (wave-uniform 64-bit ALU), appends survivors to the kept list, and stops at max_keep.
// Work is sum_blocks 64*(K/16 + 4) IoUs per wave instead of N^2/2, and only keep[] / rois leave the chip.
// The predicate and its fp32 evaluation order are those of devIoU (reference nms_kernel.cu:24-32, :71).
// ---------------------------------------------------------------------------------------------
constexpr int NMS_WAVES = 16;
constexpr int NMS_KCAP = 2048;

__global__ __launch_bounds__(NMS_WAVES * 64) void nms_kernel(const float* __restrict__ sorted_boxes,
                                                             const float* __restrict__ sorted_scores,
                                                             const int* __restrict__ counts_in, int stride, float thr,
                                                             int max_keep, int* __restrict__ keep_idx, int keep_stride,
                                                             int* __restrict__ keep_counts, float* __restrict__ rois_out,
                                                             float4* __restrict__ kept_spill, const int* __restrict__ sorted_anchor,
                                                             int* __restrict__ roi_anchor) {
  __shared__ float4 s_kept[NMS_KCAP];
  __shared__ float s_area[NMS_KCAP];
  __shared__ unsigned long long s_supp[NMS_WAVES];
  __shared__ unsigned long long s_intra[64];
  __shared__ int s_K;

  const int img = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = counts_in[img] < stride ? counts_in[img] : stride;
  const float4* boxes = (const float4*)sorted_boxes + (long long)img * stride;
  float4* spill = kept_spill + (long long)img * stride;
  int* keep = keep_idx + (long long)img * keep_stride;
  if (tid == 0) s_K = 0;
  __syncthreads();
  int K = 0;
  const int cap = max_keep < keep_stride ? max_keep : keep_stride;

  // the chunk loop is a serial dependency chain: the candidate boxes (and, where rois are produced, their scores) of chunk
  // c+1 are fetched while chunk c is being resolved, so no global-load latency sits between two chunks
  const float* scs = sorted_scores ? sorted_scores + (long long)img * stride : nullptr;
  float4 nbx = make_float4(0.f, 0.f, 0.f, 0.f);
  float nsc = 0.f;
  if (lane < N) { nbx = boxes[lane]; if (rois_out && scs) nsc = scs[lane]; }
  for (int cb = 0; cb < N && K < cap; cb += 64) {
    const int ci = cb + lane;
    const bool valid = ci < N;
    const float4 bx = nbx;
    const float sc = nsc;
    {
      const int ni = ci + 64;
      nbx = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ni < N) { nbx = boxes[ni]; if (rois_out && scs) nsc = scs[ni]; }
    }
    const float ar = (bx.z - bx.x + 1.f) * (bx.w - bx.y + 1.f);

    // A: against the kept list, strided over waves
    bool supp = false;
    for (int k = wave; k < K; k += NMS_WAVES) {
      float4 kb; float ka;
      if (k < NMS_KCAP) { kb = s_kept[k]; ka = s_area[k]; }
      else { kb = spill[k]; ka = (kb.z - kb.x + 1.f) * (kb.w - kb.y + 1.f); }
      supp = supp || iou_gt(kb, ka, bx, ar, thr);
    }
    const unsigned long long sw = __ballot(supp && valid);
    if (lane == 0) s_supp[wave] = sw;

    // B: rows 4*wave .. 4*wave+3 of the intra-block mask
#pragma unroll
    for (int q = 0; q < 64 / NMS_WAVES; ++q) {
      const int i = wave * (64 / NMS_WAVES) + q;
      float4 bi;
      bi.x = __shfl(bx.x, i); bi.y = __shfl(bx.y, i); bi.z = __shfl(bx.z, i); bi.w = __shfl(bx.w, i);
      const float ai = __shfl(ar, i);
      const bool ov = valid && (lane > i) && (cb + i < N) && iou_gt(bi, ai, bx, ar, thr);
      const unsigned long long wv = __ballot(ov);
      if (lane == 0) s_intra[i] = wv;
    }
    __syncthreads();

    // C: resolve (wave 0)
    if (wave == 0) {
      unsigned long long dead = 0;
#pragma unroll
      for (int w = 0; w < NMS_WAVES; ++w) dead |= s_supp[w];
      const unsigned long long vmask = __ballot(valid);
      unsigned long long alive = vmask & ~dead;
      // Greedy resolution inside the 64: only rows of candidates that are still alive matter, in ascending order. The rows sit
      // one per lane in registers and are fetched with v_readlane (a 64-step loop of dependent LDS reads was ~6k cycles per
      // chunk and most of the kernel's time).
      const unsigned long long myrow = s_intra[lane];
      unsigned long long rem = alive;
      while (rem) {
        const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(rem));
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(myrow & 0xffffffffull), i);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(myrow >> 32), i);
        alive &= ~(((unsigned long long)hi << 32) | lo);
        rem = alive & ~((2ull << i) - 1ull);          // still-alive candidates after i
      }
      const bool mine = (alive >> lane) & 1ull;
      const int pos = K + __popcll(alive & ((1ull << lane) - 1ull));
      if (mine && pos < cap) {
        if (pos < NMS_KCAP) { s_kept[pos] = bx; s_area[pos] = ar; }
        else spill[pos] = bx;
        keep[pos] = ci;
        if (rois_out) {
          float* r = rois_out + ((long long)img * max_keep + pos) * 5;
          r[0] = sc;
          r[1] = bx.x; r[2] = bx.y; r[3] = bx.z; r[4] = bx.w;
          // which anchor (y, x, a) produced this roi: the second return of proposal_layer (bbox_deltas[order][keep], :133-157)
          if (roi_anchor) roi_anchor[(long long)img * max_keep + pos] = sorted_anchor[(long long)img * stride + ci];
        }
      }
      int Kn = K + __popcll(alive);
      if (Kn > cap) Kn = cap;
      if (lane == 0) s_K = Kn;
    }
    __syncthreads();
    K = s_K;
  }
  if (tid == 0) keep_counts[img] = K;
}

int launch_nms(const float* sorted_boxes, const float* sorted_scores, const int* counts_in, int stride, float thresh,
               int max_keep, int* keep_idx, int keep_stride, int* keep_counts, float* rois_out, float* kept_spill, int n_img,
               hipStream_t s, const int* sorted_anchor, int* roi_anchor) {
  if (!kept_spill) return fail(CTPN_ERR_ARG, "nms: spill buffer (n_img x stride x 4 floats) required");
  if (roi_anchor && (!sorted_anchor || !rois_out)) return fail(CTPN_ERR_ARG, "nms: roi_anchor needs sorted_anchor and rois_out");
  hipLaunchKernelGGL(nms_kernel, dim3(n_img), dim3(NMS_WAVES * 64), 0, s, sorted_boxes, sorted_scores, counts_in, stride, thresh,
                     max_keep, keep_idx, keep_stride, keep_counts, rois_out, (float4*)kept_spill, sorted_anchor, roi_anchor);
  return launch_status("nms");
}

// ---------------------------------------------------------------------------------------------
// Column-decomposed greedy NMS for the proposal layer (same inputs / outputs as nms_kernel, bit-identical result).
//
// CTPN's anchors are all 16 px wide on a 16 px grid and bbox_transform_inv ignores dx / dw (reference
// lib/fast_rcnn/bbox_transform.py:50,52), so every decoded box spans x in [16 c, 16 c + 16] (clipped): boxes of non-adjacent
// columns are disjoint and adjacent columns share ONE pixel column -- IoU <= 1/33 (one column of two 17-wide boxes) whatever the heights. For a threshold above
// that, "suppressed by an earlier kept box" can only ever come from the candidate's own column group (int(x1) >> 4), i.e. greedy
// NMS over the score-sorted list factorises into independent greedy passes per column, and the global result (first max_keep
// survivors in score order) is their merge. nms_kernel walks the whole list 64 candidates at a time against ALL kept boxes
// behind two workgroup barriers per chunk (0.7 ms per launch on 32 CUs, 1.2 - 1.4 ms when it shares the GPU with the next
// batch's convolutions); here
//   1. the ranks are partitioned by column, order-preserving (per-wave histograms over contiguous rank segments + a digit-major
//      scan, the radix sort's scheme with the column as the digit);
//   2. each of the 16 waves takes columns w, w + 16, ...: 64 candidates at a time against the column's kept boxes (a few dozen,
//      in LDS), then the in-chunk greedy resolution over live candidates only -- no workgroup barrier inside;
//   3. survivors are bits in a rank-indexed mask; a popcount scan emits the first max_keep in rank (= score) order.
// The predicate and its fp32 evaluation order are nms_kernel's / devIoU's (reference nms_kernel.cu:24-32, :71).
// ---------------------------------------------------------------------------------------------

// The per-column body of the column kernels, one copy: nms_column_dev.h (nms_kept_suppress, nms_resolve_chunk).

// Step 3 over the rank-indexed survivor mask (word(j) = ranks 32 j ..: LDS, or an agent-scope load): every wave counts its contiguous share of the words ...
struct NmsShare { int w_lo, w_hi; unsigned basepos, total; };      // the wave's words, the survivors before them, the survivors of all
template <int WAVES, typename Word>
__device__ __forceinline__ NmsShare nms_count_survivors(Word word, int N, int wave, int lane, unsigned* s_wcount) {
  const int nwords = (N + 31) >> 5;
  const int wpw = ((nwords + WAVES - 1) / WAVES + 1) & ~1;    // words per wave (contiguous, even: two words = 64 ranks per step)
  NmsShare sh{wave * wpw < nwords ? wave * wpw : nwords, 0, 0u, 0u};
  sh.w_hi = sh.w_lo + wpw < nwords ? sh.w_lo + wpw : nwords;
  unsigned cnt = 0;
  for (int j = sh.w_lo + lane; j < sh.w_hi; j += 64) cnt += (unsigned)__popc(word(j));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (lane == 0) s_wcount[wave] = cnt;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < WAVES; ++w) { const unsigned v = s_wcount[w]; if (w < wave) sh.basepos += v; sh.total += v; }
  return sh;
}
// ... and, once the kernel has decided that this pass answers, emits the first `cap` in rank order (store = false: debug_nms's "no output stores")
struct NmsOut { const float* sorted_scores; const int* sorted_anchor; int stride; int* keep_idx; int keep_stride; int* keep_counts; float* rois_out; int* roi_anchor; int max_keep; };
template <typename Word>
__device__ __forceinline__ void nms_emit_survivors(Word word, NmsShare sh, int cap, int lane, int tid, bool store, int img, const float4* boxes, const NmsOut& o) {
  const unsigned long long lt = (1ull << lane) - 1ull;
  int* keep = o.keep_idx + (long long)img * o.keep_stride;
  const float* scs = o.sorted_scores ? o.sorted_scores + (long long)img * o.stride : nullptr;
  for (int j0 = sh.w_lo; j0 < sh.w_hi && (int)sh.basepos < cap; j0 += 2) {     // 64 ranks (two words) per step, one per lane
    const unsigned wlo = word(j0), whi = j0 + 1 < sh.w_hi ? word(j0 + 1) : 0u;
    const unsigned long long bits = ((unsigned long long)whi << 32) | wlo;
    if (((bits >> lane) & 1ull) && store) {
      const int pos = (int)sh.basepos + __popcll(bits & lt);
      if (pos < cap) {
        const int rank = j0 * 32 + lane;
        keep[pos] = rank;
        if (o.rois_out) {
          const float4 b = boxes[rank];
          float* r = o.rois_out + ((long long)img * o.max_keep + pos) * 5;
          r[0] = scs ? scs[rank] : 0.f;
          r[1] = b.x; r[2] = b.y; r[3] = b.z; r[4] = b.w;
          if (o.roi_anchor) o.roi_anchor[(long long)img * o.max_keep + pos] = o.sorted_anchor[(long long)img * o.stride + rank];
        }
      }
    }
    sh.basepos += (unsigned)__popcll(bits);
  }
  if (tid == 0) o.keep_counts[img] = (int)sh.total < cap ? (int)sh.total : cap;
}

// WAVES x 64 threads per image. Two instantiations:
//   <16, 12288, 128>  the proposal layer's 12 000 candidates, 16 waves, column list in LDS;
//   <4, 1024, 48>     the connector's <= 1000 candidates: 256 threads, <= 64 VGPRs, ~11 KB of LDS: fits on a CU NEXT TO a persistent
//                     convolution workgroup (those hold 144 KB of LDS and 432 of a SIMD's 512 registers), so it starts at once instead of
//                     waiting for a free CU;
//   <16, 4096, 64>    the connector's candidates on a ctx whose capacity was raised above 1024 rows (ctpn_reserve_proposals): 16 waves over the
//                     page's columns, 46 KB of LDS (the rank list and the histograms scale with MAXN and WAVES; a dense page keeps a few
//                     dozen boxes per column, beyond 64 the spill slice serves).
// col_scale != nullptr (the connector's NMS 0.2 over boxes / im_scale, detectors.py:28): the column is recovered as
// int(x1 * scale + 0.5) >> 4 -- x1 * scale is within an ulp or two of the multiple of 16 it came from.
template <int WAVES, int MAXN, int KCAP>
__global__ __launch_bounds__(WAVES * 64, WAVES == 4 ? 8 : 1) void nms_columns_kernel(
    const float* __restrict__ sorted_boxes, const float* __restrict__ sorted_scores, const int* __restrict__ counts_in, int stride, float thr,
    int max_keep, int* __restrict__ keep_idx, int keep_stride, int* __restrict__ keep_counts, float* __restrict__ rois_out,
    float4* __restrict__ kept_spill, const int* __restrict__ sorted_anchor, int* __restrict__ roi_anchor, int ncols,
    const float* __restrict__ col_scale, int prefix, int dbg) {
  // dbg (diagnostic, option debug_nms; WRONG results -- tools/r6_pipeline_race.py --compare heads looks at the other batch's network outputs only):
  // 1 = no greedy pass (step 2 skipped), 2 = no output stores (step 3's), 4 = step 2 without its box loads (zeros), 8 = return right after step 1
  __shared__ unsigned short s_list[MAXN];
  __shared__ unsigned s_hist[WAVES][NC_MAXCOL];
  __shared__ unsigned s_colbase[NC_MAXCOL + 1];
  __shared__ unsigned s_alive[MAXN / 32];
  __shared__ float4 s_kept[WAVES][KCAP];
  __shared__ float s_karea[WAVES][KCAP];
  __shared__ unsigned s_wcount[WAVES];
  const int img = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int Nall = counts_in[img] < stride ? counts_in[img] : stride;
  Nall = Nall > MAXN ? MAXN : Nall;
  const float4* boxes = (const float4*)sorted_boxes + (long long)img * stride;
  float4* spill = kept_spill + (long long)img * stride;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const float cs = col_scale ? col_scale[img * 3 + 2] : 1.0f;
  const int cap = max_keep < keep_stride ? max_keep : keep_stride;

  // PREFIX PASS (round 6). The output is the first `cap` survivors in rank (= score) order, and whether rank r survives depends on ranks
  // below r only: the greedy pass over the first P ranks yields exactly the survivors among them. With 12 000 candidates and cap = 1000
  // the 1000th survivor of the benchmark images sits at rank ~2400 (tools/nms_prefix_stats.py) -- four fifths of the candidates, and
  // more of the work (a column's chunk is tested against ALL its kept boxes), only decide survivors nobody asks for. So: run steps 1 - 2
  // on the first `prefix` ranks; if they hold >= cap survivors the answer is complete (keep_counts = cap either way); else run them
  // again on all N (the prefix pass then cost ~1/9 of a full one). prefix = 0 / >= N: one full pass, as before. Bit-identical by
  // construction; tests/test_gpu_parity.py::test_column_nms_variants_equal_generic_nms holds every form to the generic kernel.
  int N = (prefix > 0 && prefix < Nall) ? prefix : Nall;
  for (;;) {
  // ---- 1. ranks -> column lists, ascending rank inside a column ----
  for (int i = tid; i < WAVES * NC_MAXCOL; i += WAVES * 64) (&s_hist[0][0])[i] = 0u;
  for (int i = tid; i < MAXN / 32; i += WAVES * 64) s_alive[i] = 0u;
  __syncthreads();
  const int seg = (((N + WAVES - 1) / WAVES) + 63) & ~63;
  const int lo = wave * seg < N ? wave * seg : N;
  const int hi = lo + seg < N ? lo + seg : N;
  for (int base = lo; base < hi; base += 64) {
    const int r = base + lane;
    const bool valid = r < hi;
    const unsigned c = valid ? (unsigned)nms_col_of(boxes[r].x, cs, ncols) : 0u;
    const unsigned long long m = rs_match(c, valid);
    if (valid && (m & lt) == 0ull) s_hist[wave][c] += (unsigned)__popcll(m);
  }
  __syncthreads();
  for (int col = tid; col < NC_MAXCOL; col += WAVES * 64) {
    unsigned sum = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) { const unsigned v = s_hist[w][col]; s_hist[w][col] = sum; sum += v; }
    s_colbase[col] = sum;
  }
  __syncthreads();
  if (wave == 0) {
    unsigned v[4], sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { v[q] = s_colbase[4 * lane + q]; sum += v[q]; }
    unsigned incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned up = __shfl_up(incl, off);
      if (lane >= off) incl += up;
    }
    unsigned run = incl - sum;
#pragma unroll
    for (int q = 0; q < 4; ++q) { s_colbase[4 * lane + q] = run; run += v[q]; }
    if (lane == 63) s_colbase[NC_MAXCOL] = run;
  }
  __syncthreads();
  for (int base = lo; base < hi; base += 64) {
    const int r = base + lane;
    const bool valid = r < hi;
    const unsigned c = valid ? (unsigned)nms_col_of(boxes[r].x, cs, ncols) : 0u;
    const unsigned long long m = rs_match(c, valid);
    if (valid) {
      const unsigned off = s_hist[wave][c];
      s_list[s_colbase[c] + off + (unsigned)__popcll(m & lt)] = (unsigned short)r;
      if ((m >> lane) == 1ull) s_hist[wave][c] = off + (unsigned)__popcll(m);
    }
  }
  __syncthreads();

  // ---- 2. greedy NMS per column, one wave per column ----
  if (dbg & 8) return;
  for (int col = wave; col < ((dbg & 1) ? 0 : ncols); col += WAVES) {
    const int start = (int)s_colbase[col], m = (int)s_colbase[col + 1] - start;
    int K = 0;
    for (int cb = 0; cb < m; cb += 64) {
      const int ci = cb + lane;
      const bool valid = ci < m;
      const int rank = valid ? (int)s_list[start + ci] : 0;
      const float4 bx = (valid && !(dbg & 4)) ? boxes[rank] : make_float4(0.f, 0.f, 16.f * (float)(rank & 63), 16.f);
      const float ar = (bx.z - bx.x + 1.f) * (bx.w - bx.y + 1.f);
      const bool supp = nms_kept_suppress(s_kept[wave], s_karea[wave], KCAP, K, bx, ar, thr, [&](int k) { return spill[start + k]; });
      const unsigned long long alive = nms_resolve_chunk(bx, ar, __ballot(valid && !supp), lane, thr);
      const bool mine = (alive >> lane) & 1ull;
      if (mine) {
        const int pos = K + __popcll(alive & lt);
        if (pos < KCAP) { s_kept[wave][pos] = bx; s_karea[wave][pos] = ar; }
        else spill[start + pos] = bx;                       // pos < m: inside this column's own slice of the scratch
        atomicOr(&s_alive[rank >> 5], 1u << (rank & 31));
      }
      K += __popcll(alive);
      // the spill (global) is read back by this wave only, in later chunks: make the stores visible to its own loads
      if (K > KCAP) __threadfence_block();
    }
  }
  __syncthreads();

  // ---- 3. the first max_keep survivors in rank order ----
  auto alive_word = [&](int j) { return s_alive[j]; };
  const NmsShare sh = nms_count_survivors<WAVES>(alive_word, N, wave, lane, s_wcount);
  if (N < Nall && (int)sh.total < cap) {     // the prefix does not hold `cap` survivors (workgroup-uniform): once more, on everything
    __syncthreads();                          // every wave has read s_wcount / s_alive before step 1 clears them
    N = Nall;
    continue;
  }
  nms_emit_survivors(alive_word, sh, cap, lane, tid, !(dbg & 2), img, boxes,
                     NmsOut{sorted_scores, sorted_anchor, stride, keep_idx, keep_stride, keep_counts, rois_out, roi_anchor, max_keep});
  break;
  }  // passes
}

// ---------------------------------------------------------------------------------------------
// The same decomposition for SMALL batches (round 5; the reference's own calling convention is one image per call, ctpn/demo.py:55-68, and a
// lone image's proposal tail ran on ONE workgroup = one CU of 256: 333 us on 16 waves that take 3.5 columns each, one after the other).
// Columns are independent, so they spread over the machine: ncols / 4 workgroups of 4 waves per image, ONE COLUMN PER WAVE.
//   1. the wave collects its column's ranks, ascending, from the column id of every rank (one byte each, written by gather_kernel next to the
//      sorted box; 1024 ranks per 16-byte load and lane-step, the loads of a tile in flight together) -- or, the connector's <= 1024 boxes,
//      from the boxes themselves -- into its LDS list: no partition pass, no second launch;
//   2. greedy NMS of the column as in nms_columns_kernel (kept boxes in LDS, beyond MW_KCAP re-read from the sorted boxes by their rank;
//      the next chunk's boxes are fetched while the current one is resolved);
//   3. survivors are bits of a rank-indexed mask in HBM (device-scope atomicOr); the workgroup of the image that finishes LAST (a ticket)
//      runs the popcount scan that emits the first max_keep survivors in rank order and leaves mask and ticket zeroed for the next launch.
// A column holds at most MW_LIST candidates (the caller checks: hf * 10 <= 1024 for the proposal layer, <= 1024 boxes for the connector).
// Same predicate, same order of evaluation per column: bit-identical keep lists and rois (tests/test_gpu_parity.py compares all variants).
// ---------------------------------------------------------------------------------------------
constexpr int MW_WAVES = 4, MW_KCAP = 256, MW_LIST = 1024, MW_TILE = 4;
constexpr size_t MW_ALIVE_OFF = 0, MW_TICKET_OFF = NC_MAXN / 8;
static_assert(MW_TICKET_OFF + 4 <= NMS_MW_FLAG_OFF && NMS_MW_FLAG_OFF + 4 <= NMS_MW_OVERFLOW_OFF && NMS_MW_OVERFLOW_OFF + 4 <= NMS_MW_SCRATCH_BYTES, "per-image scratch block of the multi-workgroup NMS");

__global__ __launch_bounds__(MW_WAVES * 64) void nms_column_groups_kernel(
    const float* __restrict__ sorted_boxes, const float* __restrict__ sorted_scores, const unsigned char* __restrict__ colid, int colid_stride,
    const int* __restrict__ counts_in, int stride, float thr, int max_keep, int* __restrict__ keep_idx, int keep_stride, int* __restrict__ keep_counts,
    float* __restrict__ rois_out, const int* __restrict__ sorted_anchor, int* __restrict__ roi_anchor, int ncols, const float* __restrict__ col_scale,
    int maxn, char* __restrict__ scratch, int n_limit, int stage) {
  // PREFIX PASS (see nms_columns_kernel): stage 1 = this launch looks at the first n_limit ranks only and, if they do not hold `cap` survivors,
  // leaves the block's flag word set and writes nothing; stage 2 = the full launch that follows it in the stream and returns at once when the
  // flag is clear (the usual case: ~3 us); stage 0 = one full launch, as before.
  __shared__ unsigned short s_list[MW_WAVES][MW_LIST];
  __shared__ unsigned short s_krank[MW_WAVES][MW_LIST];
  __shared__ float4 s_kept[MW_WAVES][MW_KCAP];
  __shared__ float s_karea[MW_WAVES][MW_KCAP];
  __shared__ unsigned s_wcount[MW_WAVES];
  __shared__ unsigned s_last;
  const int img = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int N = counts_in[img] < stride ? counts_in[img] : stride;
  N = N > maxn ? maxn : N;
  const int Nfull = N;
  if (n_limit > 0 && n_limit < N) N = n_limit;
  const float4* boxes = (const float4*)sorted_boxes + (long long)img * stride;
  char* blk = scratch + (size_t)img * NMS_MW_SCRATCH_BYTES;
  if (stage == 2 && *(const volatile unsigned*)(blk + NMS_MW_FLAG_OFF) == 0u) return;        // stage 1 answered (workgroup-uniform: written before this launch began)
  unsigned* g_alive = (unsigned*)(blk + MW_ALIVE_OFF);
  const unsigned long long lt = (1ull << lane) - 1ull;
  unsigned short* list = s_list[wave];

  const int col = blockIdx.x * MW_WAVES + wave;
  if (col < ncols) {
    // ---- 1. the column's ranks, ascending ----
    int m = 0;
    if (colid) {
      const uint4* cid = (const uint4*)(colid + (size_t)img * colid_stride);      // 16 ranks per lane and load, 1024 per wave-step
      const unsigned pat = (unsigned)col * 0x01010101u;
      for (int base = 0; base < N; base += 1024 * MW_TILE) {
        uint4 v[MW_TILE];
#pragma unroll
        for (int j = 0; j < MW_TILE; ++j) {
          const int r0 = base + 1024 * j + 16 * lane;
          v[j] = r0 < N ? cid[r0 >> 4] : make_uint4(~pat, ~pat, ~pat, ~pat);
        }
#pragma unroll
        for (int j = 0; j < MW_TILE; ++j) {
          const int r0 = base + 1024 * j + 16 * lane;
          if (base + 1024 * j >= N) break;                  // wave-uniform
          // bit k of mm: byte k of the lane's 16 equals the column (and its rank is a candidate)
          unsigned mm = 0;
          const unsigned w4[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const unsigned x = w4[q] ^ pat;                 // zero bytes = matches
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) mm |= (((x >> (8 * bb)) & 0xffu) == 0u ? 1u : 0u) << (4 * q + bb);
          }
          const int left = N - r0;                          // ranks of this lane that exist
          mm = left >= 16 ? mm : (left > 0 ? mm & ((1u << left) - 1u) : 0u);
          const int cnt = __popc(mm);
          int incl = cnt;
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
          }
          int pos = m + incl - cnt;
          while (mm) {
            const int k = __builtin_ctz(mm);
            mm &= mm - 1u;
            if (pos < MW_LIST) list[pos] = (unsigned short)(r0 + k);
            ++pos;
          }
          m += __builtin_amdgcn_readlane(incl, 63);
        }
      }
    } else {
      const float cs = col_scale ? col_scale[img * 3 + 2] : 1.0f;
      for (int base = 0; base < N; base += 64 * 8) {
        float xs[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { const int r = base + 64 * j + lane; xs[j] = r < N ? boxes[r].x : 0.f; }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int r = base + 64 * j + lane;
          const bool hit = r < N && nms_col_of(xs[j], cs, ncols) == col;
          const unsigned long long bal = __ballot(hit);
          const int pos = m + __popcll(bal & lt);
          if (hit && pos < MW_LIST) list[pos] = (unsigned short)r;
          m += __popcll(bal);
        }
      }
    }
    // a column with more candidates than the list holds would lose the rest silently: the callers' preconditions exclude it (hf x 10 <= 1024
    // and no box clipped onto a neighbour's column: enqueue_proposals), and a caller that breaks them finds this STICKY word set (never cleared
    // by the kernel; option nms_check reads it, api_proposals.hip)
    if (m > MW_LIST && lane == 0) __hip_atomic_fetch_or((unsigned*)(blk + NMS_MW_OVERFLOW_OFF), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    m = m > MW_LIST ? MW_LIST : m;

    // ---- 2. greedy NMS of the column ----
    int K = 0;
    // software pipeline: rank and box of the next chunk are in flight while this one is resolved
    int nrank = lane < m ? (int)list[lane] : 0;
    float4 nbx = lane < m ? boxes[nrank] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int cb = 0; cb < m; cb += 64) {
      const int ci = cb + lane;
      const bool valid = ci < m;
      const int rank = nrank;
      const float4 bx = nbx;
      if (ci + 64 < m) { nrank = (int)list[ci + 64]; nbx = boxes[nrank]; }
      const float ar = (bx.z - bx.x + 1.f) * (bx.w - bx.y + 1.f);
      const bool supp = nms_kept_suppress(s_kept[wave], s_karea[wave], MW_KCAP, K, bx, ar, thr, [&](int k) { return boxes[s_krank[wave][k]]; });
      const unsigned long long alive = nms_resolve_chunk(bx, ar, __ballot(valid && !supp), lane, thr);
      const bool mine = (alive >> lane) & 1ull;
      if (mine) {
        const int pos = K + __popcll(alive & lt);
        if (pos < MW_KCAP) { s_kept[wave][pos] = bx; s_karea[wave][pos] = ar; }
        s_krank[wave][pos] = (unsigned short)rank;          // pos < m <= MW_LIST
        __hip_atomic_fetch_or(&g_alive[rank >> 5], 1u << (rank & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      K += __popcll(alive);
    }
  }
  // ---- the last workgroup of the image to get here merges ----
  __threadfence();                                          // this workgroup's mask bits are visible device-wide before its ticket is
  __syncthreads();
  if (tid == 0) {
    const unsigned t = __hip_atomic_fetch_add((unsigned*)(blk + MW_TICKET_OFF), 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (t == gridDim.x - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();

  // ---- 3. the first max_keep survivors in rank order; mask and ticket back to zero ----
  auto alive_word = [&](int j) { return __hip_atomic_load(&g_alive[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  const int cap = max_keep < keep_stride ? max_keep : keep_stride;
  const int nwords = (N + 31) >> 5;
  const NmsShare sh = nms_count_survivors<MW_WAVES>(alive_word, N, wave, lane, s_wcount);
  if (stage == 1) {
    const bool again = N < Nfull && (int)sh.total < cap;      // the prefix does not hold `cap` survivors: the full launch behind this one does the work
    if (again) {
      __syncthreads();
      for (int j = tid; j < nwords; j += MW_WAVES * 64) g_alive[j] = 0u;
      if (tid == 0) { *(unsigned*)(blk + MW_TICKET_OFF) = 0u; *(unsigned*)(blk + NMS_MW_FLAG_OFF) = 1u; }
      return;
    }
    if (tid == 0) *(unsigned*)(blk + NMS_MW_FLAG_OFF) = 0u;
  } else if (stage == 2 && tid == 0) *(unsigned*)(blk + NMS_MW_FLAG_OFF) = 0u;
  nms_emit_survivors(alive_word, sh, cap, lane, tid, true, img, boxes,
                     NmsOut{sorted_scores, sorted_anchor, stride, keep_idx, keep_stride, keep_counts, rois_out, roi_anchor, max_keep});
  __syncthreads();                                          // every wave has read its words
  for (int j = tid; j < nwords; j += MW_WAVES * 64) g_alive[j] = 0u;
  if (tid == 0) *(unsigned*)(blk + MW_TICKET_OFF) = 0u;
}

int nms_column_group_workgroups(int ncols) { return (ncols + MW_WAVES - 1) / MW_WAVES; }
// the multi-workgroup form answers from a prefix launch only where the full launch behind it has more ranks to look at; the one-workgroup kernel
// takes the prefix as an argument and decides on the image's count
int nms_prefix_launches(bool multi_wg, int prefix, int stride, int max_keep) {
  if (!(prefix > 0 && max_keep < prefix)) return 0;
  return multi_wg ? (prefix < stride ? 2 : 0) : 1;
}

// col_scale (im_info rows [h, w, scale], nullable) selects the connector's variant (stride <= 1024, 4 waves).
// PRECONDITION: boxes on the 16-px anchor grid (common.h); arbitrary boxes must go through launch_nms.
int launch_nms_columns(const float* sorted_boxes, const float* sorted_scores, const int* counts_in, int stride, float thresh, int max_keep,
                       int* keep_idx, int keep_stride, int* keep_counts, float* rois_out, float* kept_spill, int n_img, int ncols, hipStream_t s,
                       const int* sorted_anchor, int* roi_anchor, const float* col_scale, void* mw_scratch, const unsigned char* colid, int prefix, int dbg) {
  if (!kept_spill) return fail(CTPN_ERR_ARG, "nms: spill buffer (n_img x stride x 4 floats) required");
  if (ncols < 1 || ncols > NC_MAXCOL || stride > NC_MAXN || !(thresh >= 0.1f)) return fail(CTPN_ERR_ARG, "nms_columns: outside the column decomposition's domain");
  if (roi_anchor && (!sorted_anchor || !rois_out)) return fail(CTPN_ERR_ARG, "nms: roi_anchor needs sorted_anchor and rois_out");
  if (col_scale && stride > NC_TL_LARGE_MAXN) return fail(CTPN_ERR_ARG, "nms_columns: connector variant takes at most 4096 candidates per image");
  if (col_scale && stride > NC_TL_MAXN) {
    // more rows than the 4-wave form's lists and the multi-workgroup form's per-column list hold: the one-workgroup form sized for 4096
    if (mw_scratch) return fail(CTPN_ERR_ARG, "nms_columns: the multi-workgroup form takes at most 1024 connector candidates per image");
    hipLaunchKernelGGL((nms_columns_kernel<16, NC_TL_LARGE_MAXN, 64>), dim3(n_img), dim3(1024), 0, s, sorted_boxes, sorted_scores, counts_in, stride, thresh,
                       max_keep, keep_idx, keep_stride, keep_counts, rois_out, (float4*)kept_spill, sorted_anchor, roi_anchor, ncols, col_scale, 0, 0);
  } else if (mw_scratch) {
    // small batches: one column per wave, ncols / 4 workgroups per image (mw_scratch: n_img x NMS_MW_SCRATCH_BYTES, zero on entry and on exit;
    // colid: gather_kernel's column byte per rank, row pitch = stride rounded up to 16 -- null: the columns come from the boxes, <= 1024 of them)
    if (!colid && stride > MW_LIST) return fail(CTPN_ERR_ARG, "nms_columns: the multi-workgroup form needs column ids for more than 1024 candidates");
    const int maxn = col_scale ? NC_TL_MAXN : NC_MAXN;
    const bool two = nms_prefix_launches(true, prefix, stride, max_keep) == 2;       // a prefix launch, then the full one that usually finds nothing to do
    for (int stage = two ? 1 : 0; stage <= (two ? 2 : 0); ++stage)
      hipLaunchKernelGGL(nms_column_groups_kernel, dim3(nms_column_group_workgroups(ncols), n_img), dim3(MW_WAVES * 64), 0, s, sorted_boxes, sorted_scores,
                         colid, (stride + 15) & ~15, counts_in, stride, thresh, max_keep, keep_idx, keep_stride, keep_counts, rois_out, sorted_anchor, roi_anchor,
                         ncols, col_scale, maxn, (char*)mw_scratch, stage == 1 ? prefix : 0, stage);
  } else if (col_scale) {      // (stride <= NC_TL_MAXN: checked above)
    hipLaunchKernelGGL((nms_columns_kernel<4, NC_TL_MAXN, 48>), dim3(n_img), dim3(256), 0, s, sorted_boxes, sorted_scores, counts_in, stride, thresh,
                       max_keep, keep_idx, keep_stride, keep_counts, rois_out, (float4*)kept_spill, sorted_anchor, roi_anchor, ncols, col_scale, 0, 0);
  } else {
    hipLaunchKernelGGL((nms_columns_kernel<16, NC_MAXN, 128>), dim3(n_img), dim3(1024), 0, s, sorted_boxes, sorted_scores, counts_in, stride, thresh,
                       max_keep, keep_idx, keep_stride, keep_counts, rois_out, (float4*)kept_spill, sorted_anchor, roi_anchor, ncols, nullptr,
                       nms_prefix_launches(false, prefix, stride, max_keep) ? prefix : 0, dbg);
  }
  return launch_status("nms_columns");
}

// nms_prefix_launches' choice of the prefix: the 4096 best-scored ranks hold `max_keep` survivors only if max_keep is well below them -- the pass
// pays off where it usually answers (survivors / ranks was ~0.4 on the images it was measured on), so it is asked for up to max_keep = 1024 and
// skipped above, where a prefix pass would nearly always be followed by the full one. The keep lists are identical either way.
int nms_prefix_ranks(int nms_prefix, int max_keep) { return nms_prefix && max_keep <= 1024 ? NMS_PREFIX_RANKS : 0; }

bool nms_columns_ok(int ncols, int stride, float thresh) { return ncols >= 1 && ncols <= NC_MAXCOL && stride <= NC_MAXN && thresh >= 0.1f; }
// the connector's NMS (boxes already divided by im_scale): adjacent columns overlap by one scaled pixel of 16 / scale + 1, so
// IoU <= 1 / (32 / scale + 1) <= 1/9 for scale <= 4 -- far below the 0.2 threshold
bool nms_columns_tl_ok(int ncols, int stride, float thresh, float max_scale) {
  return ncols >= 1 && ncols <= NC_MAXCOL && stride <= NC_TL_LARGE_MAXN && thresh >= 0.15f && max_scale > 0.f && max_scale <= 4.0f;
}

// ---------------------------------------------------------------------------------------------
// The same decomposition for a PAGE (ctpn_page_nms: the merged proposals of a page's tiles in front of the connector's NMS 0.2): ONE list
// of up to 2^20 score-sorted boxes in up to 1024 columns int(x1) >> 4 -- more ranks than a workgroup's LDS lists hold and more columns than its
// histograms, so every step is a launch of its own and the launch boundaries are the only hand-offs between workgroups:
//   1. an order-preserving partition of the ranks by column. The unit is a WAVE over a contiguous segment of ranks: page_hist_kernel counts every
//      unit's ranks per column (rs_match's scheme on ten column bits), page_scan_kernel scans the counts column-major, unit-minor in one
//      workgroup (wg_scan.h) -- a unit's start inside every column, and the columns' starts --, page_scatter_kernel walks the segments again and
//      writes the ranks: ascending rank inside a column because units, and a unit's 64-rank steps, are taken in rank order;
//   2. nms_page_columns_kernel: one wave per column, ncols / 4 workgroups (1024 columns = 1024 waves: four on every CU), nms_column_greedy
//      (nms_column_dev.h) over the column's ranks: kept boxes in the wave's LDS, beyond PGN_KCAP in the column's slice of the spill block;
//      survivors are bits of a rank-indexed mask in HBM (agent-scope atomicOr; read by the next launch only);
//   3. page_emit_kernel: a popcount scan over the mask writes the keep list in rank order, and its length.
// Same predicate, same order of evaluation per column: the keep list is launch_nms's on every input of the precondition (launch_nms_columns').
// ---------------------------------------------------------------------------------------------
constexpr int PGN_WAVES = 4, PGN_KCAP = 128, PGN_MAXUNITS = 256;

__device__ __forceinline__ int pgn_col_of(float x1, int ncols) {
  const int c = (int)x1 >> 4;
  return c < 0 ? 0 : (c > ncols - 1 ? ncols - 1 : c);      // (the caller checked every box: a clamp never changes a column)
}
// rs_match on ten bits: the lanes (valid ones) whose column is this lane's
__device__ __forceinline__ unsigned long long pgn_match(unsigned c, bool valid) {
  unsigned long long mask = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 10; ++b) {
    const bool bit = (c >> b) & 1u;
    const unsigned long long bal = __ballot(bit);
    mask &= bit ? bal : ~bal;
  }
  return mask;
}

// unit u = blockIdx.x * PGN_WAVES + wave owns ranks [u seg, u seg + seg) below n (seg a multiple of 64); hist: [ncols][units]
__global__ __launch_bounds__(PGN_WAVES * 64) void page_hist_kernel(const float4* __restrict__ boxes, int n, int seg, int units, int ncols, unsigned* __restrict__ hist) {
  __shared__ unsigned s_hist[PGN_WAVES][NMS_PAGE_MAXCOL];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int unit = blockIdx.x * PGN_WAVES + wave;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int i = lane; i < ncols; i += 64) s_hist[wave][i] = 0u;
  __syncthreads();
  const long long lo64 = (long long)unit * seg;
  const int lo = lo64 < n ? (int)lo64 : n;
  const int hi = lo + seg < n ? lo + seg : n;
  for (int base = lo; base < hi; base += 64) {
    const int r = base + lane;
    const bool valid = r < hi;
    const unsigned c = valid ? (unsigned)pgn_col_of(boxes[r].x, ncols) : 0u;
    const unsigned long long m = pgn_match(c, valid);
    if (valid && (m & lt) == 0ull) s_hist[wave][c] += (unsigned)__popcll(m);
  }
  __syncthreads();
  if (unit < units)
    for (int i = lane; i < ncols; i += 64) hist[(size_t)i * units + unit] = s_hist[wave][i];
}

// hist [ncols][units], read as one row of ncols x units counts -> the exclusive prefix sums in place; colbase[c] = column c's start, colbase[ncols] = n
__global__ __launch_bounds__(256) void page_scan_kernel(unsigned* __restrict__ hist, int units, int ncols, unsigned* __restrict__ colbase) {
  const int total = ncols * units;
  const int per = (total + 255) / 256;
  const int lo = (int)threadIdx.x * per < total ? (int)threadIdx.x * per : total;
  const int hi = lo + per < total ? lo + per : total;
  uint32_t sum = 0;
  for (int i = lo; i < hi; ++i) sum += hist[i];
  uint32_t all = 0;
  uint32_t run = wg_scan256(sum, all) - sum;
  for (int i = lo; i < hi; ++i) {
    const unsigned v = hist[i];
    hist[i] = run;
    if (i % units == 0) colbase[i / units] = run;
    run += v;
  }
  if (threadIdx.x == 0) colbase[ncols] = all;
}

__global__ __launch_bounds__(PGN_WAVES * 64) void page_scatter_kernel(const float4* __restrict__ boxes, int n, int seg, int units, int ncols,
                                                                      const unsigned* __restrict__ hist, int* __restrict__ list) {
  __shared__ unsigned s_off[PGN_WAVES][NMS_PAGE_MAXCOL];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int unit = blockIdx.x * PGN_WAVES + wave;
  const unsigned long long lt = (1ull << lane) - 1ull;
  if (unit < units)
    for (int i = lane; i < ncols; i += 64) s_off[wave][i] = hist[(size_t)i * units + unit];
  __syncthreads();
  const long long lo64 = (long long)unit * seg;
  const int lo = lo64 < n ? (int)lo64 : n;
  const int hi = lo + seg < n ? lo + seg : n;
  for (int base = lo; base < hi; base += 64) {
    const int r = base + lane;
    const bool valid = r < hi;
    const unsigned c = valid ? (unsigned)pgn_col_of(boxes[r].x, ncols) : 0u;
    const unsigned long long m = pgn_match(c, valid);
    if (valid) {
      const unsigned off = s_off[wave][c];
      const unsigned at = off + (unsigned)__popcll(m & lt);
      if (at < (unsigned)n) list[at] = r;      // (always: the counts are page_hist_kernel's of the same columns)
      if ((m >> lane) == 1ull) s_off[wave][c] = off + (unsigned)__popcll(m);
    }
  }
}

__global__ __launch_bounds__(PGN_WAVES * 64) void nms_page_columns_kernel(const float4* __restrict__ boxes, const int* __restrict__ list,
                                                                          const unsigned* __restrict__ colbase, int n, int ncols, float thr,
                                                                          float4* __restrict__ spill, unsigned* __restrict__ alive) {
  __shared__ float4 s_kept[PGN_WAVES][PGN_KCAP];
  __shared__ float s_karea[PGN_WAVES][PGN_KCAP];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int col = blockIdx.x * PGN_WAVES + wave; col < ncols; col += gridDim.x * PGN_WAVES) {
    const int start = (int)colbase[col], end = (int)colbase[col + 1];
    if (start < 0 || end > n || end <= start) continue;      // (wave-uniform; an empty column)
    // (a rank outside the list cannot come out of the partition; were the scratch ever stale, it must still not become an address)
    nms_column_greedy(boxes, [&](int ci) { const int r = list[start + ci]; return (unsigned)r < (unsigned)n ? r : 0; }, end - start, s_kept[wave], s_karea[wave], PGN_KCAP, spill + start, thr, lane,
                      [&](int rank) { __hip_atomic_fetch_or(&alive[rank >> 5], 1u << (rank & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
  }
}

// alive: (n + 31) / 32 words, bits at and beyond n clear -> keep: the set bits' ranks, ascending; count[0]: how many
__global__ __launch_bounds__(256) void page_emit_kernel(const unsigned* __restrict__ alive, int n, int* __restrict__ keep, int* __restrict__ count) {
  const int nwords = (n + 31) >> 5;
  const int per = (nwords + 255) / 256;
  const int lo = (int)threadIdx.x * per < nwords ? (int)threadIdx.x * per : nwords;
  const int hi = lo + per < nwords ? lo + per : nwords;
  uint32_t cnt = 0;
  for (int j = lo; j < hi; ++j) cnt += (uint32_t)__popc(alive[j]);
  uint32_t all = 0;
  uint32_t pos = wg_scan256(cnt, all) - cnt;
  for (int j = lo; j < hi; ++j) {
    unsigned w = alive[j];
    while (w) {
      const int b = __builtin_ctz(w);
      w &= w - 1u;
      if (pos < (uint32_t)n) keep[pos] = j * 32 + b;
      ++pos;
    }
  }
  if (threadIdx.x == 0) count[0] = (int)all;
}

int nms_page_units(int n) {
  int u = (n + 1023) / 1024;
  u = u < 1 ? 1 : (u > PGN_MAXUNITS ? PGN_MAXUNITS : u);
  return (u + PGN_WAVES - 1) / PGN_WAVES * PGN_WAVES;
}

int launch_nms_page_columns(const float* sorted_boxes, int n, int ncols, float thresh, int* list, unsigned* hist, unsigned* colbase, float* spill,
                            unsigned* alive, int* keep, int* count, hipStream_t s) {
  if (n < 1 || n > NMS_PAGE_MAXN || ncols < 1 || ncols > NMS_PAGE_MAXCOL || !(thresh >= 0.1f)) return fail(CTPN_ERR_ARG, "nms_page_columns: outside the column decomposition's domain");
  if (!list || !hist || !colbase || !spill || !alive || !keep || !count) return fail(CTPN_ERR_ARG, "nms_page_columns: null scratch");
  const int units = nms_page_units(n);
  const int seg = (((n + units - 1) / units) + 63) & ~63;
  const float4* boxes = (const float4*)sorted_boxes;
  CTPN_HIP_TRY(hipMemsetAsync(alive, 0, (size_t)((n + 31) >> 5) * sizeof(unsigned), s));
  hipLaunchKernelGGL(page_hist_kernel, dim3(units / PGN_WAVES), dim3(PGN_WAVES * 64), 0, s, boxes, n, seg, units, ncols, hist);
  hipLaunchKernelGGL(page_scan_kernel, dim3(1), dim3(256), 0, s, hist, units, ncols, colbase);
  hipLaunchKernelGGL(page_scatter_kernel, dim3(units / PGN_WAVES), dim3(PGN_WAVES * 64), 0, s, boxes, n, seg, units, ncols, (const unsigned*)hist, list);
  hipLaunchKernelGGL(nms_page_columns_kernel, dim3((ncols + PGN_WAVES - 1) / PGN_WAVES), dim3(PGN_WAVES * 64), 0, s, boxes, (const int*)list, (const unsigned*)colbase,
                     n, ncols, thresh, (float4*)spill, alive);
  hipLaunchKernelGGL(page_emit_kernel, dim3(1), dim3(256), 0, s, (const unsigned*)alive, n, keep, count);
  return launch_status("nms_page_columns");
}

// Every launch decision of the text-line tail, in one place (common.h): enqueue_text_lines computes this once and follows it
TextLinePlan text_line_plan(int nms_columns, int connect_device, bool has_mw_scratch, int n, int wf, int rows, float nms_thresh, float max_scale) {
  TextLinePlan p{};
  p.nms_form = TL_NMS_GENERIC;
  if (nms_columns && nms_columns_tl_ok(wf, rows, nms_thresh, max_scale))
    p.nms_form = rows > NC_TL_MAXN ? TL_NMS_ONE_WG_LARGE : (nms_multi_wg_ok(has_mw_scratch, nms_columns, n, 0) ? TL_NMS_COLUMN_GROUPS : TL_NMS_ONE_WG);
  p.group_wgs = p.nms_form == TL_NMS_COLUMN_GROUPS ? nms_column_group_workgroups(wf) : 0;
  p.conn_form = !connect_device ? TL_CONN_HOST : (connect_work_bytes(rows) ? TL_CONN_BUCKETS : TL_CONN_ALL_PAIRS);
  return p;
}

}  // namespace ctpn
