// The training data layer's kernels (include/ctpn_hip_data_layer.h; the per-thread text: data_layer_dev.h).
//   split labels   three passes. dl_count_kernel: one thread per quad -- its page by a binary search of the quad offsets, its span on the resized
//                  page, its strip count. dl_scan_kernel: ONE workgroup walks the counts in runs of 2048 (eight per thread, wg_scan256 over the
//                  thread sums, a carry from run to run) and writes the exclusive scan, Q + 1 ints; then it gathers the pages' strip offsets.
//                  No atomics: a strip's place is a function of the input alone. dl_write_kernel: one thread per strip -- its quad by a binary
//                  search of the scan, then one 16-byte store (four 4-byte stores where the output is not 16-byte aligned).
//   train page     one thread per 16 bytes of image_out: ctpn_resize's sample, mirrored after the resize, and the float32 blob of the same 16
//                  values. A streaming kernel: every output byte is written once, the source is read through the cache; no LDS.
//   train boxes    one thread per strip; a value outside uint16 raises a flag the entry point reads.
// Built with -ffp-contract=off (resize_pixel.h's sample position; the scalings here are one rounded operation after another).
#include "common.h"
#include "data_layer_dev.h"
#include "wg_scan.h"

namespace ctpn {

typedef __attribute__((ext_vector_type(4))) float dl_f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int dl_u32x4;

constexpr int DL_SCAN_PER_THREAD = 8;

__global__ __launch_bounds__(256) void dl_count_kernel(const double* __restrict__ quads, int nq, const int* __restrict__ quad_offs, int pages,
                                                       const int* __restrict__ dims, DlSpan* __restrict__ spans, uint32_t* __restrict__ counts) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const int page = dl_upper(quad_offs, pages, q);
  const DlSpan s = dl_quad_span(quads + (size_t)q * 8, dims + (size_t)page * 4);
  spans[q] = s;
  counts[q] = (uint32_t)dl_strip_count(s.xmin, s.xmax);
}

// launched as one workgroup of 256. scan: nq + 1 ints
__global__ __launch_bounds__(256) void dl_scan_kernel(const uint32_t* __restrict__ counts, int nq, int* __restrict__ scan, const int* __restrict__ quad_offs,
                                                      int pages, int* __restrict__ page_offs) {
  uint32_t carry = 0;
  for (int base = 0; base < nq; base += 256 * DL_SCAN_PER_THREAD) {
    const int first = base + (int)threadIdx.x * DL_SCAN_PER_THREAD;
    uint32_t c[DL_SCAN_PER_THREAD], sum = 0;
#pragma unroll
    for (int k = 0; k < DL_SCAN_PER_THREAD; ++k) { c[k] = first + k < nq ? counts[first + k] : 0u; sum += c[k]; }
    uint32_t total;
    uint32_t run = carry + wg_scan256(sum, total) - sum;
#pragma unroll
    for (int k = 0; k < DL_SCAN_PER_THREAD; ++k) {
      if (first + k < nq) scan[first + k] = (int)run;
      run += c[k];
    }
    carry += total;
    __syncthreads();      // wg_scan256's wave totals are read; the next run may store them
  }
  if (threadIdx.x == 0) scan[nq] = (int)carry;
  __syncthreads();        // the scan is written: this workgroup's threads read it below
  for (int p = (int)threadIdx.x; p <= pages; p += 256) page_offs[p] = scan[quad_offs[p]];
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void dl_write_kernel(const DlSpan* __restrict__ spans, const int* __restrict__ scan, int nq, int total, float* __restrict__ strips) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= total) return;
  const int q = dl_upper(scan, nq, s);
  const DlSpan sp = spans[q];
  int x1, x2;
  dl_strip(sp.xmin, sp.xmax, s - scan[q], x1, x2);
  const float v[4] = {(float)x1, (float)sp.ymin, (float)x2, (float)sp.ymax};
  if (ALIGNED) ((dl_f32x4*)strips)[s] = dl_f32x4{v[0], v[1], v[2], v[3]};
  else
#pragma unroll
    for (int k = 0; k < 4; ++k) strips[(size_t)s * 4 + k] = v[k];
}

int launch_split_count(const double* quads, int nq, const int* quad_offs, int pages, const int* dims, void* spans, uint32_t* counts, hipStream_t s) {
  if (nq <= 0) return CTPN_OK;
  hipLaunchKernelGGL(dl_count_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, quads, nq, quad_offs, pages, dims, (DlSpan*)spans, counts);
  return launch_status("split labels: count");
}

int launch_split_scan(const uint32_t* counts, int nq, int* scan, const int* quad_offs, int pages, int* page_offs, hipStream_t s) {
  hipLaunchKernelGGL(dl_scan_kernel, dim3(1), dim3(256), 0, s, counts, nq, scan, quad_offs, pages, page_offs);
  return launch_status("split labels: scan");
}

int launch_split_write(const void* spans, const int* scan, int nq, int total, float* strips, hipStream_t s) {
  if (total <= 0) return CTPN_OK;
  const dim3 grid((unsigned)((total + 255) / 256));
  if ((reinterpret_cast<uintptr_t>(strips) & 15) == 0) hipLaunchKernelGGL(dl_write_kernel<true>, grid, dim3(256), 0, s, (const DlSpan*)spans, scan, nq, total, strips);
  else hipLaunchKernelGGL(dl_write_kernel<false>, grid, dim3(256), 0, s, (const DlSpan*)spans, scan, nq, total, strips);
  return launch_status("split labels: write");
}

// IMG_ALIGN / BLOB_ALIGN: 16 where the output is 16-byte aligned, else 4 where it is 4-byte aligned (the blob always is), else 1
template <int IMG_ALIGN, int BLOB_ALIGN>
__global__ __launch_bounds__(256) void dl_page_kernel(const uint8_t* __restrict__ src, DlPage p, size_t groups, uint8_t* __restrict__ image_out,
                                                      float* __restrict__ blob_out) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  uint8_t v[DL_GROUP];
  const int count = dl_page_group(src, p, g, v);
  const size_t b0 = g * DL_GROUP;
  auto word = [&](int k) { return (unsigned)v[k] | ((unsigned)v[k + 1] << 8) | ((unsigned)v[k + 2] << 16) | ((unsigned)v[k + 3] << 24); };
  if (IMG_ALIGN == 16 && count == DL_GROUP) {
    ((dl_u32x4*)image_out)[g] = dl_u32x4{word(0), word(4), word(8), word(12)};
  } else {
    int k = 0;
    if (IMG_ALIGN >= 4)
      for (; k + 4 <= count; k += 4) *(unsigned*)(image_out + b0 + k) = word(k);
    for (; k < count; ++k) image_out[b0 + k] = v[k];
  }
  if (!blob_out) return;
  int c = (int)(b0 % 3);
  float f[DL_GROUP];
#pragma unroll
  for (int k = 0; k < DL_GROUP; ++k) {
    f[k] = dl_blob(v[k], c);
    c = c == 2 ? 0 : c + 1;
  }
  int k = 0;
  if (BLOB_ALIGN == 16)
    for (; k + 4 <= count; k += 4) *(dl_f32x4*)(blob_out + b0 + k) = dl_f32x4{f[k], f[k + 1], f[k + 2], f[k + 3]};
  for (; k < count; ++k) blob_out[b0 + k] = f[k];
}

int launch_train_page(const uint8_t* src, const DlPage& p, uint8_t* image_out, float* blob_out, hipStream_t s) {
  const size_t groups = dl_page_groups(p);
  if (!groups) return CTPN_OK;
  const size_t wgs = (groups + 255) / 256;
  if (wgs > 0x7fffffffULL) return fail(CTPN_ERR_ARG, "train page: page beyond 2^43 bytes");
  const uintptr_t ia = reinterpret_cast<uintptr_t>(image_out), ba = reinterpret_cast<uintptr_t>(blob_out);
  const int img = (ia & 15) == 0 ? 16 : (ia & 3) == 0 ? 4 : 1, blob = (ba & 15) == 0 ? 16 : 4;
  const dim3 grid((unsigned)wgs), block(256);
#define DL_PAGE_CASE(I, B) \
  if (img == I && blob == B) hipLaunchKernelGGL((dl_page_kernel<I, B>), grid, block, 0, s, src, p, groups, image_out, blob_out)
  DL_PAGE_CASE(16, 16); DL_PAGE_CASE(16, 4); DL_PAGE_CASE(4, 16); DL_PAGE_CASE(4, 4); DL_PAGE_CASE(1, 16); DL_PAGE_CASE(1, 4);
#undef DL_PAGE_CASE
  return launch_status("train page");
}

__global__ __launch_bounds__(256) void dl_boxes_kernel(const float* __restrict__ strips, int n, int page_width, int flip, double scale, float* __restrict__ out,
                                                       int* __restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float o[5];
  if (!dl_box(strips + (size_t)i * 4, page_width, flip, scale, o)) { *bad = 1; return; }      // every writer stores the same value
#pragma unroll
  for (int k = 0; k < 5; ++k) out[(size_t)i * 5 + k] = o[k];
}

int launch_train_boxes(const float* strips, int n, int page_width, int flip, double scale, float* out, int* bad, hipStream_t s) {
  if (n <= 0) return CTPN_OK;
  hipLaunchKernelGGL(dl_boxes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, strips, n, page_width, flip, scale, out, bad);
  return launch_status("train boxes");
}

}  // namespace ctpn
