// Tiles of a page larger than the network input, cut at native resolution in ONE launch (ctpn_page_cut: api_page.hip): tiles first .. first + n - 1
// of a plan into n x tile_h x tile_w x 3 BGR bytes, the buffer ctpn_detect_submit takes as a device batch. Inside the page a byte is the page's;
// outside (the last tile of a row or column, a page smaller than the tile) it is round(PIXEL_MEANS), which the q-image turns into the zero that
// im_list_to_blob pads with. The kernel writes every byte of the buffer and reads none of it. The per-thread text -- the plan's record, the
// byte-wise page pixel, the four-pixel store -- is page_dev.h's, pinned on the CPU from that very text (tests/test_page_plan.py).
//   A thread owns four consecutive pixels of one tile row: three aligned dwords, a wave's stores fill 768 contiguous bytes. The page side is
//   byte gathers (neither the page pointer nor its pitch is aligned to anything) through the vector L1 / L2: 12 bytes read per 12 written, each
//   page byte read once per tile that sees it. One 64-bit and one 32-bit division per thread, none per pixel. The tile table (32 bytes per tile)
//   stays cache-resident. No LDS, no synchronisation. HBM-bound.
#include "common.h"
#include "page_dev.h"

namespace ctpn {

__global__ __launch_bounds__(PG_THREADS) void page_cut_kernel(const uint8_t* __restrict__ page, long long pitch, const PgTile* __restrict__ tiles, int n, int tile_h,
                                                              int tile_w, uint8_t* __restrict__ out) {
  pg_cut_thread(page, pitch, tiles, n, tile_h, tile_w, out, (long long)blockIdx.x * PG_THREADS + threadIdx.x);
}

static_assert(sizeof(PgTile) == 8 * sizeof(int), "ctpn_page_plan's record is eight ints");

int launch_page_cut(const uint8_t* page_dev, long long pitch, const PgTile* tiles_dev, int n, int tile_h, int tile_w, uint8_t* out_dev, hipStream_t s) {
  if (n <= 0 || tile_h < 16 || tile_w < 16 || (tile_w & 15) || !page_dev || !tiles_dev || !out_dev || ((uintptr_t)out_dev & 3))
    return fail(CTPN_ERR_ARG, "page_cut: bad arguments (the tile buffer is 4-byte aligned, the tile width a multiple of 16)");
  const long long wgs = (pg_cut_groups(n, tile_h, tile_w) + PG_THREADS - 1) / PG_THREADS;
  if (wgs > 0x7fffffffLL) return fail(CTPN_ERR_ARG, "page_cut: grid out of range");
  hipLaunchKernelGGL(page_cut_kernel, dim3((unsigned)wgs), dim3(PG_THREADS), 0, s, page_dev, pitch, tiles_dev, n, tile_h, tile_w, out_dev);
  return launch_status("page_cut");
}

}  // namespace ctpn
