// C ABI of libctpn_hip.so, crop unit: the detected text lines of a batch cut out of its images ON THE DEVICE, one rectified image of fixed
// height per line -- what a recogniser behind the detector reads (kernel and descriptor: crop.hip, arithmetic: crop_pixel.h). An output
// stage in the ctx's copy queue like the annotated writer (api_out_stage.hip): behind the decode that produced the batch, in front of the next.
// The *_ragged entry points are the same calls over a ragged canvas: a table of heights rides with the descriptors, and the kernel takes a
// line's image from its slot and clamps the row axis at the image's own last row.
#include <climits>
#include <cmath>

#include "ctx.h"

namespace ctpn {

static int crop_check_geometry(const char* who, int crop_h, int max_w) {
  if (crop_h < 1 || crop_h > 256) return fail(CTPN_ERR_ARG, std::string(who) + ": crop_h must be 1 .. 256");
  if (max_w < 4 || (max_w & 3) || max_w > 65535) return fail(CTPN_ERR_ARG, std::string(who) + ": max_w must be a multiple of 4 in 4 .. 65535");
  return CTPN_OK;
}

static bool crop_finite(const double* rec9) {
  for (int k = 0; k < 8; ++k) if (!std::isfinite(rec9[k])) return false;
  return true;
}

static int crop_reserve(ctpn_ctx* c, size_t desc_bytes) {
  auto& K = c->crop;
  int rc;
  if ((rc = K.ev_done.ensure()) || (rc = K.desc_host.grow(desc_bytes))) return rc;
  return K.desc_dev.grow(desc_bytes);
}

// the argument checks of ctpn_crop_lines and pass 1, host only: every line's width (what the sizing call is for).
// ragged: the batch is a canvas n x h x w x 3 and heights[i] (16 .. h) the rows of slot i that are image i (the *_ragged entry points)
static int crop_plan(const char* who_, ctpn_ctx* c, int n, int h, int w, const int* heights, bool ragged, const double* recs, int line_capacity, const int* line_counts, int crop_h,
                     int max_w, int pad_value, int* widths_out, int* total_out, std::vector<int>& widths) {
  const std::string who(who_);
  if (total_out) *total_out = 0;
  if (!c || !line_counts || !total_out || (ragged && !heights)) return fail(CTPN_ERR_ARG, who + ": null pointer");
  if (n <= 0 || h <= 0 || w <= 0 || line_capacity < 0) return fail(CTPN_ERR_ARG, who + ": empty batch / bad size");
  for (int i = 0; ragged && i < n; ++i)
    if (heights[i] < 16 || heights[i] > h)
      return fail(CTPN_ERR_ARG, who + ": image " + std::to_string(i) + ": height " + std::to_string(heights[i]) + " outside 16 .. " + std::to_string(h));
  if (int rc = crop_check_geometry(who_, crop_h, max_w)) return rc;
  if (pad_value < 0 || pad_value > 255) return fail(CTPN_ERR_ARG, who + ": pad_value must be 0 .. 255");
  long long total = 0;
  for (int i = 0; i < n; ++i) {
    if (line_counts[i] < 0 || line_counts[i] > line_capacity || (line_counts[i] > 0 && !recs)) return fail(CTPN_ERR_ARG, who + ": line count out of range");
    total += line_counts[i];
  }
  if (total > INT_MAX) return fail(CTPN_ERR_ARG, who + ": too many lines");
  if (c->postproc_only) return fail(CTPN_ERR_STATE, who + ": post-processing-only ctx");
  widths.assign((size_t)total, 0);
  for (int i = 0, k = 0; i < n; ++i)
    for (int j = 0; j < line_counts[i]; ++j, ++k) {
      const double* r = recs + ((size_t)i * line_capacity + j) * 9;
      if (!crop_finite(r)) return fail(CTPN_ERR_ARG, who + ": image " + std::to_string(i) + ", line " + std::to_string(j) + ": a coordinate is not finite");
      widths[k] = crop_line_width(r, crop_h, max_w);
      if (widths_out) widths_out[k] = widths[k];
    }
  *total_out = (int)total;
  return CTPN_OK;
}

// pass 2 in the ctx's copy queue: descriptors, the batch's pixels, the kernel into out_dev (total x crop_h x max_w x 3); no host wait
// heights (nullable): a ragged canvas; the table rides behind the descriptors, in the same page-locked block and the same copy
static int crop_cut(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, const int* heights, const double* recs, int line_capacity,
                    const int* line_counts, const std::vector<int>& widths, int crop_h, int max_w, int pad_value, uint8_t* out_dev) {
  auto& K = c->crop;
  hipStream_t qs = c->stream_c;
  const size_t total = widths.size(), line_bytes = (size_t)crop_h * max_w * 3;
  int rc;
  const size_t desc_bytes = total * CROP_DESC_BYTES, table_bytes = desc_bytes + (heights ? (size_t)n * sizeof(int) : 0);
  if ((rc = crop_reserve(c, table_bytes))) return rc;
  for (int i = 0, k = 0; i < n; ++i)
    for (int j = 0; j < line_counts[i]; ++j, ++k)
      crop_fill_desc(recs + ((size_t)i * line_capacity + j) * 9, i, widths[k], (size_t)k * line_bytes, K.desc_host.as<char>() + (size_t)k * CROP_DESC_BYTES);
  if (heights) std::memcpy(K.desc_host.as<char>() + desc_bytes, heights, (size_t)n * sizeof(int));
  CTPN_HIP_TRY(hipMemcpyAsync(K.desc_dev.get(), K.desc_host.get(), table_bytes, hipMemcpyHostToDevice, qs));
  const int* heights_dev = heights ? (const int*)(K.desc_dev.as<char>() + desc_bytes) : nullptr;
  const uint8_t* px;
  if ((rc = stage_pixels(c, images, images_on_device, (size_t)n * h * w * 3, 0, K.img_dev, qs, px))) return rc;
  return launch_crop_lines(px, K.desc_dev.get(), (int)total, out_dev, h, w, heights_dev, crop_h, max_w, pad_value, qs);
}

// ctpn_write_line_crops / ctpn_write_line_crops_device / ctpn_write_line_crops_png and their _ragged forms. format: the files'
enum CropFormat { CROP_JPEG, CROP_PNG };      // (PNG: lossless, no quality, host-built codes only)
static int write_line_crops_impl(ctpn_ctx* c, const char* who_, const uint8_t* images, int images_on_device, int n, int h, int w, const int* heights, bool ragged,
                                 const double* recs, int line_capacity, const int* line_counts, int crop_h, int max_w, int pad_value, CropFormat format, int quality, const char* const* paths,
                                 int* widths_out, int* total_out, bool device_entropy) {
  const std::string who(who_);
  std::vector<int> widths;
  int rc;
  if ((rc = crop_plan(who_, c, n, h, w, heights, ragged, recs, line_capacity, line_counts, crop_h, max_w, pad_value, widths_out, total_out, widths))) return rc;
  if (format == CROP_JPEG && (quality < 1 || quality > 100)) return fail(CTPN_ERR_ARG, who + ": quality must be 1 .. 100");
  if (!paths) return CTPN_OK;      // the sizing call
  const size_t total = widths.size();
  if (total == 0) return CTPN_OK;
  if (!images) return fail(CTPN_ERR_ARG, who + ": null pointer");
  for (size_t k = 0; k < total; ++k) if (!paths[k]) return fail(CTPN_ERR_ARG, who + ": null path");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  auto& K = c->crop;
  const size_t pitch = (size_t)max_w * 3, line_bytes = (size_t)crop_h * pitch;
  if ((rc = K.out_dev.grow(total * line_bytes))) return rc;
  // the JPEG encoder's aligned read (jenc_load4) stays inside a crop's pixels where its rows start 4-byte aligned: the buffer is a device
  // allocation, a crop's offset and the pitch are multiples of 12 (max_w % 4 == 0, crop_check_geometry). (The PNG writer reads bytes.)
  if (format == CROP_JPEG && (((uintptr_t)K.out_dev.get() & 3) || (pitch & 3) || (line_bytes & 3))) return fail(CTPN_ERR_STATE, who + ": the crop rows are not 4-byte aligned");
  if ((rc = crop_cut(c, images, images_on_device, n, h, w, heights, recs, line_capacity, line_counts, widths, crop_h, max_w, pad_value, K.out_dev.as<uint8_t>()))) return rc;
  // encoded where they lie, behind the kernel in the same queue: crop k is crop_h x widths[k] at pitch 3 max_w -- the pad columns never enter a file
  std::vector<int> crop_heights(total, crop_h);
  std::vector<size_t> pitches(total, pitch), offsets(total);
  for (size_t k = 0; k < total; ++k) offsets[k] = k * line_bytes;
  if (format == CROP_PNG) return png_code_table(c, who_, K.out_dev.as<uint8_t>(), (int)total, crop_heights.data(), widths.data(), pitches.data(), offsets.data(), nullptr, nullptr, nullptr, paths);
  return encode_mixed_dev(c, who_, K.out_dev.as<uint8_t>(), (int)total, crop_heights.data(), widths.data(), pitches.data(), offsets.data(), quality, nullptr, nullptr, nullptr, paths, device_entropy);
}

// ctpn_crop_lines / ctpn_crop_lines_ragged
static int crop_lines_impl(ctpn_ctx* c, const char* who_, const uint8_t* images, int images_on_device, int n, int h, int w, const int* heights, bool ragged, const double* recs,
                           int line_capacity, const int* line_counts, int crop_h, int max_w, int pad_value, uint8_t* crops_out, int crops_on_device, size_t capacity_bytes,
                           int* widths_out, int* total_out) {
  const std::string who(who_);
  std::vector<int> widths;
  if (int rc = crop_plan(who_, c, n, h, w, heights, ragged, recs, line_capacity, line_counts, crop_h, max_w, pad_value, widths_out, total_out, widths)) return rc;
  const size_t total = widths.size(), line_bytes = (size_t)crop_h * max_w * 3;
  if (!crops_out && capacity_bytes == 0) return CTPN_OK;      // the sizing call
  if (total == 0) return CTPN_OK;
  const size_t need = total * line_bytes;
  if (capacity_bytes < need) return fail(CTPN_ERR_CAPACITY, who + ": the output holds " + std::to_string(capacity_bytes) + " bytes, the crops need " + std::to_string(need));
  if (!crops_out || !images) return fail(CTPN_ERR_ARG, who + ": null pointer");
  if (crops_on_device && ((uintptr_t)crops_out & 3)) return fail(CTPN_ERR_ARG, who + ": a device output must be 4-byte aligned");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  auto& K = c->crop;
  hipStream_t qs = c->stream_c;
  int rc;
  uint8_t* out = crops_out;
  if (!crops_on_device) {
    if ((rc = K.out_dev.grow(need))) return rc;
    out = K.out_dev.as<uint8_t>();
  }
  if ((rc = crop_cut(c, images, images_on_device, n, h, w, heights, recs, line_capacity, line_counts, widths, crop_h, max_w, pad_value, out))) return rc;
  if (!crops_on_device) CTPN_HIP_TRY(hipMemcpyAsync(crops_out, K.out_dev.as<uint8_t>(), need, hipMemcpyDeviceToHost, qs));
  CTPN_HIP_TRY(hipEventRecord(K.ev_done, qs));
  CTPN_HIP_TRY(hipEventSynchronize(K.ev_done));
  return CTPN_OK;
}

}  // namespace ctpn

extern "C" {

int ctpn_line_crop_width(const double* rec9, int crop_h, int max_w, int* width_out) {
  if (!rec9 || !width_out) return fail(CTPN_ERR_ARG, "ctpn_line_crop_width: null pointer");
  if (int rc = crop_check_geometry("ctpn_line_crop_width", crop_h, max_w)) return rc;
  if (!crop_finite(rec9)) return fail(CTPN_ERR_ARG, "ctpn_line_crop_width: a coordinate is not finite");
  *width_out = crop_line_width(rec9, crop_h, max_w);
  return CTPN_OK;
}

int ctpn_crop_lines(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, const double* recs, int line_capacity,
                    const int* line_counts, int crop_h, int max_w, int pad_value, uint8_t* crops_out, int crops_on_device, size_t capacity_bytes,
                    int* widths_out, int* total_out) {
  return crop_lines_impl(c, "ctpn_crop_lines", images, images_on_device, n, h, w, nullptr, false, recs, line_capacity, line_counts, crop_h, max_w, pad_value, crops_out,
                         crops_on_device, capacity_bytes, widths_out, total_out);
}

int ctpn_crop_lines_ragged(ctpn_ctx* c, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights, const double* recs, int line_capacity,
                           const int* line_counts, int crop_h, int max_w, int pad_value, uint8_t* crops_out, int crops_on_device, size_t capacity_bytes,
                           int* widths_out, int* total_out) {
  return crop_lines_impl(c, "ctpn_crop_lines_ragged", canvas, canvas_on_device, n, hc, w, heights, true, recs, line_capacity, line_counts, crop_h, max_w, pad_value, crops_out,
                         crops_on_device, capacity_bytes, widths_out, total_out);
}

int ctpn_write_line_crops(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, const double* recs, int line_capacity, const int* line_counts,
                          int crop_h, int max_w, int pad_value, int quality, const char* const* paths, int* widths_out, int* total_out) {
  return write_line_crops_impl(c, "ctpn_write_line_crops", images, images_on_device, n, h, w, nullptr, false, recs, line_capacity, line_counts, crop_h, max_w, pad_value, CROP_JPEG, quality, paths,
                               widths_out, total_out, false);
}

int ctpn_write_line_crops_device(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, const double* recs, int line_capacity, const int* line_counts,
                                 int crop_h, int max_w, int pad_value, int quality, const char* const* paths, int* widths_out, int* total_out) {
  return write_line_crops_impl(c, "ctpn_write_line_crops_device", images, images_on_device, n, h, w, nullptr, false, recs, line_capacity, line_counts, crop_h, max_w, pad_value, CROP_JPEG, quality, paths,
                               widths_out, total_out, true);
}

int ctpn_write_line_crops_png(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, const double* recs, int line_capacity, const int* line_counts,
                              int crop_h, int max_w, int pad_value, const char* const* paths, int* widths_out, int* total_out) {
  return write_line_crops_impl(c, "ctpn_write_line_crops_png", images, images_on_device, n, h, w, nullptr, false, recs, line_capacity, line_counts, crop_h, max_w, pad_value, CROP_PNG, 0,
                               paths, widths_out, total_out, false);
}

int ctpn_write_line_crops_png_ragged(ctpn_ctx* c, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights, const double* recs, int line_capacity,
                                     const int* line_counts, int crop_h, int max_w, int pad_value, const char* const* paths, int* widths_out, int* total_out) {
  return write_line_crops_impl(c, "ctpn_write_line_crops_png_ragged", canvas, canvas_on_device, n, hc, w, heights, true, recs, line_capacity, line_counts, crop_h, max_w, pad_value,
                               CROP_PNG, 0, paths, widths_out, total_out, false);
}

int ctpn_write_line_crops_ragged(ctpn_ctx* c, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights, const double* recs, int line_capacity,
                                 const int* line_counts, int crop_h, int max_w, int pad_value, int quality, const char* const* paths, int* widths_out, int* total_out) {
  return write_line_crops_impl(c, "ctpn_write_line_crops_ragged", canvas, canvas_on_device, n, hc, w, heights, true, recs, line_capacity, line_counts, crop_h, max_w, pad_value,
                               CROP_JPEG, quality, paths, widths_out, total_out, false);
}

int ctpn_write_line_crops_ragged_device(ctpn_ctx* c, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights, const double* recs,
                                        int line_capacity, const int* line_counts, int crop_h, int max_w, int pad_value, int quality, const char* const* paths,
                                        int* widths_out, int* total_out) {
  return write_line_crops_impl(c, "ctpn_write_line_crops_ragged_device", canvas, canvas_on_device, n, hc, w, heights, true, recs, line_capacity, line_counts, crop_h, max_w,
                               pad_value, CROP_JPEG, quality, paths, widths_out, total_out, true);
}

}  // extern "C"
