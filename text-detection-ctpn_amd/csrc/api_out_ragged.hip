// C ABI of libctpn_hip.so, the annotated writer over a RAGGED canvas (include/ctpn_hip.h, "Ragged batches out"): images of one width and
// different heights in the slots of one canvas (ctpn_decode_jpeg_*_ragged, ctpn_detect_submit_ragged), each written back at its own
// file's size. The pixel stage (annotate_ragged) in front of the mixed-size coders, one per format (api_jpeg_out.hip, encode_mixed_dev;
// api_png_out.hip, png_code_table):
//   the canvas copied into a ctx-owned buffer (the decoder's may still feed a forward; a host canvas is staged the same way),
//   outlines drawn slot by slot, bounded by each image's own height (jpeg_enc.hip, draw_boxes_ragged_kernel: draw_boxes_kernel's body),
//   every image whose scale is not 1 resized by its own 1 / scale into a block of its own behind the canvas copy, in ONE launch
//   (resize_mixed.hip; an image at scale 1 is coded from the drawn copy where it lies, at pitch 3 w),
//   and the n images of n sizes coded from that one buffer by their pitches and offsets.
// The crops of a ragged canvas need no stage of their own: api_crops.hip's calls take the heights (crop_lines_kernel clamps at them).
#include <cmath>

#include "ctx.h"

namespace ctpn {

static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// (ctx.h) the pixel stage both formats share
int annotate_ragged(ctpn_ctx* c, const std::string& who, const char* format, StageTableCheck table_check, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w,
                    const int* heights, const double* recs, int line_capacity, const int* line_counts, const double* scales, const char* const* paths, const uint8_t*& px,
                    std::vector<int>& dh, std::vector<int>& dw, std::vector<size_t>& pitches, std::vector<size_t>& offsets) {
  if (!c || !canvas || !heights || !line_counts || !scales || !paths) return fail(CTPN_ERR_ARG, who + ": null pointer");
  if (n <= 0 || hc <= 0 || w <= 0 || hc > 65535 || w > 65535 || line_capacity < 0) return fail(CTPN_ERR_ARG, who + ": empty batch / bad size");
  // per image: the size it is written at (demo.py:51: cv2.resize by fx = fy = 1 / scale; the identity is a copy there and no work here)
  std::vector<int> resized;
  dh.assign((size_t)n, 0); dw.assign((size_t)n, 0);
  std::vector<double> inv_f((size_t)n, 1.0);
  for (int i = 0; i < n; ++i) {
    const std::string img = who + ": image " + std::to_string(i) + ": ";
    if (heights[i] < 16 || heights[i] > hc) return fail(CTPN_ERR_ARG, img + "height " + std::to_string(heights[i]) + " outside 16 .. " + std::to_string(hc));
    if (!std::isfinite(scales[i]) || !(scales[i] > 0.0)) return fail(CTPN_ERR_ARG, img + "the scale is not finite and positive");
    if (!paths[i]) return fail(CTPN_ERR_ARG, img + "null path");
    if (line_counts[i] < 0 || line_counts[i] > line_capacity || (line_counts[i] > 0 && !recs)) return fail(CTPN_ERR_ARG, img + "line count out of range");
    const double f = 1.0 / scales[i];
    dh[i] = heights[i]; dw[i] = w;
    if (f != 1.0) {
      // (a double outside int's range does not convert: compared first)
      const double rh = std::nearbyint((double)heights[i] * f), rw = std::nearbyint((double)w * f);
      if (!(rh >= 1.0) || !(rw >= 1.0) || rh > 65535.0 || rw > 65535.0) return fail(CTPN_ERR_ARG, img + "the resized image is empty or too large for a " + format + " file");
      dh[i] = resize_out_dim(heights[i], f); dw[i] = resize_out_dim(w, f);
      inv_f[i] = 1.0 / f;      // what launch_resize_linear hands its kernel
      resized.push_back(i);
    }
  }
  int rc;
  if (table_check && (rc = table_check(who, n, dh.data(), dw.data()))) return rc;
  if (c->postproc_only) return fail(CTPN_ERR_STATE, who + ": post-processing-only ctx");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  auto& S = c->stage;
  hipStream_t qs = c->stream_c;
  // ONE buffer: the canvas copy, then a block per resized image (256-byte aligned; rows at resize_mixed_pitch), then the encoder's slack
  const size_t slot_bytes = (size_t)hc * w * 3, canvas_bytes = (size_t)n * slot_bytes;
  const int m = (int)resized.size();
  pitches.assign((size_t)n, (size_t)w * 3); offsets.assign((size_t)n, 0);
  for (int i = 0; i < n; ++i) offsets[i] = (size_t)i * slot_bytes;
  size_t at = up256(canvas_bytes + 4);
  for (int i : resized) {
    pitches[i] = resize_mixed_pitch(dw[i]);
    offsets[i] = at;
    at = up256(at + (size_t)dh[i] * pitches[i]);
  }
  if ((rc = S.img_dev.grow(at + 256))) return rc;
  if ((rc = S.recs_dev.grow(std::max<size_t>((size_t)n * line_capacity * 9 * sizeof(double), 64)))) return rc;
  if ((rc = S.cnt_dev.grow((size_t)n * sizeof(int)))) return rc;
  // the heights and the resize's descriptor table in one page-locked block and one copy (the block is free: every earlier call waited for its files)
  const size_t tab_off = up256((size_t)n * sizeof(int)), tab_bytes = tab_off + (size_t)m * RM_DESC_BYTES;
  if ((rc = S.rm_host.grow(tab_bytes)) || (rc = S.rm_dev.grow(tab_bytes))) return rc;
  std::memcpy(S.rm_host.as<uint8_t>(), heights, (size_t)n * sizeof(int));
  long long items = 0;
  if (m) {
    std::vector<int> sh((size_t)m), sw((size_t)m, w), th((size_t)m), tw((size_t)m);
    std::vector<long long> so((size_t)m), sp((size_t)m, (long long)w * 3), to((size_t)m);
    std::vector<double> fi((size_t)m);
    for (int k = 0; k < m; ++k) {
      const int i = resized[k];
      sh[k] = heights[i]; th[k] = dh[i]; tw[k] = dw[i]; so[k] = (long long)i * (long long)slot_bytes; to[k] = (long long)offsets[i]; fi[k] = inv_f[i];
    }
    items = resize_mixed_fill(S.rm_host.as<uint8_t>() + tab_off, m, sh.data(), sw.data(), th.data(), tw.data(), so.data(), sp.data(), to.data(), fi.data());
    if (items < 0) return fail(CTPN_ERR_ARG, who + ": more than 2^31 - 1 work items in one call");
  }
  CTPN_HIP_TRY(hipMemcpyAsync(S.rm_dev.as<uint8_t>(), S.rm_host.as<uint8_t>(), tab_bytes, hipMemcpyHostToDevice, qs));
  // the outlines go onto the ctx's copy: a live canvas (produced in this queue) may still feed a forward, and a caller's canvas is never modified
  if (canvas_on_device && (rc = wait_live_batch(c, canvas, qs))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(S.img_dev.as<uint8_t>(), canvas, canvas_bytes, canvas_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, qs));
  if (recs && line_capacity > 0) CTPN_HIP_TRY(hipMemcpyAsync(S.recs_dev.as<double>(), recs, (size_t)n * line_capacity * 9 * sizeof(double), hipMemcpyHostToDevice, qs));
  CTPN_HIP_TRY(hipMemcpyAsync(S.cnt_dev.as<int>(), line_counts, (size_t)n * sizeof(int), hipMemcpyHostToDevice, qs));
  if ((rc = launch_draw_boxes_ragged(S.img_dev.as<uint8_t>(), S.recs_dev.as<double>(), S.cnt_dev.as<int>(), S.rm_dev.as<int>(), line_capacity, n, hc, w, qs))) return rc;
  if (m && (rc = launch_resize_linear_mixed(S.img_dev.as<uint8_t>(), S.img_dev.as<uint8_t>(), S.rm_dev.as<uint8_t>() + tab_off, m, items, qs))) return rc;
  px = S.img_dev.as<uint8_t>();
  return CTPN_OK;
}

// ctpn_write_annotated_files_ragged / ctpn_write_annotated_files_ragged_device
static int write_annotated_ragged_impl(ctpn_ctx* c, const char* who_, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights, const double* recs,
                                       int line_capacity, const int* line_counts, const double* scales, const char* const* paths, int quality, bool device_entropy) {
  const std::string who(who_);
  // (the stage's first two checks, repeated: the quality keeps its place behind them and in front of the per-image checks)
  if (!c || !canvas || !heights || !line_counts || !scales || !paths) return fail(CTPN_ERR_ARG, who + ": null pointer");
  if (n <= 0 || hc <= 0 || w <= 0 || hc > 65535 || w > 65535 || line_capacity < 0) return fail(CTPN_ERR_ARG, who + ": empty batch / bad size");
  if (quality < 1 || quality > 100) return fail(CTPN_ERR_ARG, who + ": quality must be 1 .. 100");
  const uint8_t* px;
  std::vector<int> dh, dw;
  std::vector<size_t> pitches, offsets;
  if (int rc = annotate_ragged(c, who, "JPEG", nullptr, canvas, canvas_on_device, n, hc, w, heights, recs, line_capacity, line_counts, scales, paths, px, dh, dw, pitches, offsets)) return rc;
  return encode_mixed_dev(c, who_, px, n, dh.data(), dw.data(), pitches.data(), offsets.data(), quality, nullptr, nullptr, nullptr, paths, device_entropy);
}

}  // namespace ctpn

extern "C" {

int ctpn_write_annotated_files_ragged(ctpn_ctx* c, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights, const double* recs, int line_capacity,
                                      const int* line_counts, const double* scales, const char* const* paths, int quality) {
  return write_annotated_ragged_impl(c, "ctpn_write_annotated_files_ragged", canvas, canvas_on_device, n, hc, w, heights, recs, line_capacity, line_counts, scales, paths, quality,
                                     false);
}

int ctpn_write_annotated_png_files_ragged(ctpn_ctx* c, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights, const double* recs, int line_capacity,
                                          const int* line_counts, const double* scales, const char* const* paths) {
  const uint8_t* px;
  std::vector<int> dh, dw;
  std::vector<size_t> pitches, offsets;
  if (int rc = annotate_ragged(c, "ctpn_write_annotated_png_files_ragged", "PNG", png_table_check, canvas, canvas_on_device, n, hc, w, heights, recs, line_capacity, line_counts, scales,
                               paths, px, dh, dw, pitches, offsets)) return rc;
  return png_code_table(c, "ctpn_write_annotated_png_files_ragged", px, n, dh.data(), dw.data(), pitches.data(), offsets.data(), nullptr, nullptr, nullptr, paths);
}

int ctpn_write_annotated_files_ragged_device(ctpn_ctx* c, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights, const double* recs,
                                             int line_capacity, const int* line_counts, const double* scales, const char* const* paths, int quality) {
  return write_annotated_ragged_impl(c, "ctpn_write_annotated_files_ragged_device", canvas, canvas_on_device, n, hc, w, heights, recs, line_capacity, line_counts, scales, paths,
                                     quality, true);
}

}  // extern "C"
