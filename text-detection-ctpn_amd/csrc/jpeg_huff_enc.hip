// Baseline Huffman coding of quantised coefficients on the device: the second, opt-in form of the JPEG writer (the first codes on the
// host: jpeg_enc.hip). The kernels read what jpeg_fdct_kernel writes -- or, through the test seam, natural-order coefficients -- and leave
// the scan body of every file, stuffed, in HBM; the host adds the header and EOI. Per-thread text: jpeg_huff_enc_dev.h, which
// tests/jpeg_huff_enc_host.cpp compiles for the host. One thread per block (length, write) or per 64-byte chunk (count, stuff), one
// workgroup per image for the two prefix sums; grid y = the image. No workgroup waits on another.
#include "common.h"
#include "jpeg_huff_enc_dev.h"
#include "wg_scan.h"

namespace ctpn {

template <bool ZZ>
__global__ __launch_bounds__(256) void jhe_length_kernel(const JheImg* __restrict__ imgs, const int16_t* __restrict__ coef, const JheTables* __restrict__ T,
                                                         uint32_t* __restrict__ len, JheRes* __restrict__ res) {
  const JheImg im = imgs[blockIdx.y];
  jhe_length_thread<ZZ>(im, blockIdx.x * 256u + threadIdx.x, coef, *T, len, &res[blockIdx.y].flag);
}

template <bool ZZ>
__global__ __launch_bounds__(256) void jhe_write_kernel(const JheImg* __restrict__ imgs, const int16_t* __restrict__ coef, const JheTables* __restrict__ T,
                                                        const uint32_t* __restrict__ off, uint32_t* __restrict__ uns, JheRes* __restrict__ res) {
  const JheImg im = imgs[blockIdx.y];
  jhe_write_thread<ZZ>(im, blockIdx.x * 256u + threadIdx.x, coef, *T, off, uns, &res[blockIdx.y].flag);
}

__global__ __launch_bounds__(256) void jhe_count_kernel(const JheImg* __restrict__ imgs, const uint32_t* __restrict__ uns, uint32_t* __restrict__ cnt, const JheRes* __restrict__ res) {
  const JheImg im = imgs[blockIdx.y];
  jhe_count_thread(im, blockIdx.x * 256u + threadIdx.x, res[blockIdx.y].bits, uns, cnt);
}

__global__ __launch_bounds__(256) void jhe_stuff_kernel(const JheImg* __restrict__ imgs, const uint32_t* __restrict__ uns, const uint32_t* __restrict__ pre, uint8_t* __restrict__ out,
                                                        JheRes* __restrict__ res) {
  const JheImg im = imgs[blockIdx.y];
  jhe_stuff_thread(im, blockIdx.x * 256u + threadIdx.x, res[blockIdx.y].bits, uns, pre, out, &res[blockIdx.y].flag);
}

// exclusive prefix sum, in place, of one image's items: one workgroup per image, JHE_SCAN_ITEMS items per step, the running total in a register
// of every thread. CHUNKS = false: the blocks' bit lengths -> bit offsets, the total to res.bits. CHUNKS = true: the 0xFF counts of the
// chunks the unstuffed bytes fill -> stuffing offsets, unstuffed bytes + total to res.bytes
template <bool CHUNKS>
__global__ __launch_bounds__(256) void jhe_scan_kernel(const JheImg* __restrict__ imgs, uint32_t* __restrict__ items, JheRes* __restrict__ res) {
  const JheImg im = imgs[blockIdx.x];
  const uint32_t bits = CHUNKS ? res[blockIdx.x].bits : 0u;
  const uint32_t count = CHUNKS ? jhe_chunk_count(bits, im) : im.nblk;
  uint32_t* it = items + (CHUNKS ? im.chunk0 : im.blk0);
  const uint32_t tid = threadIdx.x;
  const uint32_t steps = (count + JHE_SCAN_ITEMS - 1) / JHE_SCAN_ITEMS;
  uint32_t carry = 0;
  for (uint32_t st = 0; st < steps; ++st) {
    const uint32_t base = st * JHE_SCAN_ITEMS + tid * 4u;
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = base + k < count ? it[base + k] : 0u;
    const uint32_t mine = v[0] + v[1] + v[2] + v[3];
    uint32_t total;
    uint32_t ex = carry + wg_scan256(mine, total) - mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (base + k < count) it[base + k] = ex;
      ex += v[k];
    }
    carry += total;
    __syncthreads();      // wg_scan256's second barrier: the wave totals are rewritten in the next step
  }
  if (tid == 0) jhe_scan_finish<CHUNKS>(im, bits, carry, res[blockIdx.x]);
}

// the passes of one launch group in queue s; B: the group's buffers (every part sized by the caller from the images' block counts)
int launch_jpeg_huff_enc(const JheBatchDev& B, bool zigzag, hipStream_t s) {
  if (B.n <= 0 || B.n > 65535 || B.max_blocks == 0 || B.max_blocks > (uint32_t)JHE_MAX_BLOCKS) return fail(CTPN_ERR_ARG, "jpeg huffman encode: group out of range");
  const dim3 wg(256), gb((B.max_blocks + 255u) / 256u, (unsigned)B.n), gc((B.max_chunks + 255u) / 256u, (unsigned)B.n), gi((unsigned)B.n);
  if (zigzag) hipLaunchKernelGGL(jhe_length_kernel<true>, gb, wg, 0, s, B.imgs, B.coef, B.tables, B.len, B.res);
  else hipLaunchKernelGGL(jhe_length_kernel<false>, gb, wg, 0, s, B.imgs, B.coef, B.tables, B.len, B.res);
  hipLaunchKernelGGL(jhe_scan_kernel<false>, gi, wg, 0, s, B.imgs, B.len, B.res);
  if (zigzag) hipLaunchKernelGGL(jhe_write_kernel<true>, gb, wg, 0, s, B.imgs, B.coef, B.tables, B.len, B.uns, B.res);
  else hipLaunchKernelGGL(jhe_write_kernel<false>, gb, wg, 0, s, B.imgs, B.coef, B.tables, B.len, B.uns, B.res);
  hipLaunchKernelGGL(jhe_count_kernel, gc, wg, 0, s, B.imgs, B.uns, B.cnt, B.res);
  hipLaunchKernelGGL(jhe_scan_kernel<true>, gi, wg, 0, s, B.imgs, B.cnt, B.res);
  hipLaunchKernelGGL(jhe_stuff_kernel, gc, wg, 0, s, B.imgs, B.uns, B.cnt, B.out, B.res);
  return launch_status("jpeg huffman encode");
}

}  // namespace ctpn
