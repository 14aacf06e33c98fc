// PNG result images on the device: the DEFLATE block of every file of a batch (per-piece text and the file's definition: png_enc_dev.h,
// which tests/png_enc_host.cpp compiles for the host). Writing parallelises where reading does not: the Sub filter reads raw pixels only,
// and a DEFLATE stream may be tokenised in independent pieces. One thread per piece of 256 stream bytes. A call is a table of images of any
// sizes and pitches: the hist, length and write kernels run over a one-dimensional grid of work items -- a workgroup is 256 pieces of ONE
// image, found by pnge_locate (png_enc_dev.h) -- so no image's grid is sized by the largest one; one workgroup per image for the prefix sum. The kernels are integer and latency-bound: a piece is a serial walk with two byte loads per stream byte
// (pixel and left neighbour; the row above doubles that), uncoalesced across the lanes of a wave -- consecutive lanes are 256 bytes apart,
// so a wave's 16 KiB window stays in L1 / L2 across the walk. The code table (1.1 KiB per image) is staged in LDS once per workgroup.
// No workgroup waits on another: order comes from the kernel boundaries.
#include "common.h"
#include "png_enc_dev.h"
#include "wg_scan.h"

namespace ctpn {

// symbols per image: LDS counters per workgroup (ds_add: lanes of a wave that hit the same counter -- flat paper: all of them -- serialise
// there, not in L2), then one vector atomicAdd per used symbol into the image's 286 counters
__global__ __launch_bounds__(256) void pnge_hist_kernel(const PngeImg* __restrict__ imgs, uint32_t n, const uint8_t* __restrict__ px, uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[PNGE_NSYM];
  for (uint32_t k = threadIdx.x; k < (uint32_t)PNGE_NSYM; k += 256u) cnt[k] = 0u;
  __syncthreads();
  const PngeItem it = pnge_locate(imgs, n, blockIdx.x);
  const PngeImg im = imgs[it.img];
  pnge_hist_thread(im, it.piece + threadIdx.x, px, cnt);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < (uint32_t)PNGE_NSYM; k += 256u)
    if (cnt[k]) atomicAdd(hist + (size_t)it.img * PNGE_NSYM + k, cnt[k]);
}

__global__ __launch_bounds__(256) void pnge_length_kernel(const PngeImg* __restrict__ imgs, uint32_t n, const uint8_t* __restrict__ px, const PngeCodes* __restrict__ codes,
                                                          PngeLen* __restrict__ len) {
  __shared__ uint32_t ll[PNGE_NSYM];
  const PngeItem it = pnge_locate(imgs, n, blockIdx.x);
  for (uint32_t k = threadIdx.x; k < (uint32_t)PNGE_NSYM; k += 256u) ll[k] = codes[it.img].ll[k];
  __syncthreads();
  const PngeImg im = imgs[it.img];
  pnge_length_thread(im, it.piece + threadIdx.x, px, ll, len);
}

__global__ __launch_bounds__(256) void pnge_write_kernel(const PngeImg* __restrict__ imgs, uint32_t n, const uint8_t* __restrict__ px, const PngeCodes* __restrict__ codes,
                                                         const PngeLen* __restrict__ off, uint32_t* __restrict__ words, PngeRes* __restrict__ res) {
  __shared__ uint32_t ll[PNGE_NSYM];
  const PngeItem it = pnge_locate(imgs, n, blockIdx.x);
  for (uint32_t k = threadIdx.x; k < (uint32_t)PNGE_NSYM; k += 256u) ll[k] = codes[it.img].ll[k];
  __syncthreads();
  const PngeImg im = imgs[it.img];
  pnge_write_thread(im, it.piece + threadIdx.x, px, ll, codes[it.img].hdr, off, words, &res[it.img].flag);      // (the header's words: the image's first item)
}

// exclusive prefix sum, in place, of one image's piece lengths behind the header's bits, and the Adler-32 out of the pieces' partials: one
// workgroup per image, PNGE_SCAN_ITEMS pieces per step, the running total in a register of every thread (jhe_scan_kernel's form, with
// the two Adler sums carried along)
__global__ __launch_bounds__(256) void pnge_scan_kernel(const PngeImg* __restrict__ imgs, const PngeCodes* __restrict__ codes, PngeLen* __restrict__ items, PngeRes* __restrict__ res) {
  __shared__ unsigned long long wad[4][2];
  const PngeImg im = imgs[blockIdx.x];
  PngeLen* it = items + im.piece0;
  const uint32_t count = im.npieces;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t steps = (count + PNGE_SCAN_ITEMS - 1) / PNGE_SCAN_ITEMS;
  uint32_t carry = codes[blockIdx.x].hdr_bits;
  uint64_t sa = 0, ss = 0;
  for (uint32_t st = 0; st < steps; ++st) {
    const uint32_t base = st * PNGE_SCAN_ITEMS + tid * 4u;
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = 0u;
      if (base + k < count) {
        const PngeLen r = it[base + k];
        v[k] = r.bits;
        pnge_adler_term(im.n, pnge_piece_end(im, base + k), r.a, r.b, sa, ss);
      }
    }
    const uint32_t mine = v[0] + v[1] + v[2] + v[3];
    uint32_t total;
    uint32_t ex = carry + wg_scan256(mine, total) - mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (base + k < count) it[base + k].bits = ex;
      ex += v[k];
    }
    carry += total;
    __syncthreads();      // wg_scan256's second barrier: the wave totals are rewritten in the next step
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { sa += __shfl_down(sa, d, 64); ss += __shfl_down(ss, d, 64); }
  if (lane == 0u) { wad[wave][0] = sa; wad[wave][1] = ss; }
  __syncthreads();
  if (tid == 0) {
    sa = wad[0][0] + wad[1][0] + wad[2][0] + wad[3][0];
    ss = wad[0][1] + wad[1][1] + wad[2][1] + wad[3][1];
    pnge_scan_finish(im, carry, sa, ss, res[blockIdx.x]);
  }
}

// items: the table's work items (pnge_layout; the caller has checked pnge_totals_ok)
int launch_png_hist(const PngeImg* imgs, const uint8_t* px, uint32_t* hist, int n, uint64_t items, hipStream_t s) {
  if (n <= 0 || items == 0 || items > PNGE_MAX_ITEMS) return fail(CTPN_ERR_ARG, "png encode: batch out of range");
  hipLaunchKernelGGL(pnge_hist_kernel, dim3((unsigned)items), dim3(256), 0, s, imgs, (uint32_t)n, px, hist);
  return launch_status("png encode (histogram)");
}

int launch_png_code(const PngeImg* imgs, const uint8_t* px, const PngeCodes* codes, PngeLen* len, uint32_t* words, PngeRes* res, int n, uint64_t items, hipStream_t s) {
  if (n <= 0 || items == 0 || items > PNGE_MAX_ITEMS) return fail(CTPN_ERR_ARG, "png encode: batch out of range");
  const dim3 wg(256), gp((unsigned)items);
  hipLaunchKernelGGL(pnge_length_kernel, gp, wg, 0, s, imgs, (uint32_t)n, px, codes, len);
  hipLaunchKernelGGL(pnge_scan_kernel, dim3((unsigned)n), wg, 0, s, imgs, codes, len, res);
  hipLaunchKernelGGL(pnge_write_kernel, gp, wg, 0, s, imgs, (uint32_t)n, px, codes, len, words, res);
  return launch_status("png encode");
}

}  // namespace ctpn
