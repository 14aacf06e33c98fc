// C ABI of libctpn_hip.so, the output stage under the writers (api_jpeg_out.hip, api_png_out.hip) and ctpn_crop_lines: where a call's pixels
// come from, the annotated images of ctpn/demo.py:28-52 up to the file format (draw_boxes_kernel, cv2.resize by 1 / scale), files onto the disk.
#include "ctx.h"

namespace ctpn {

// a live batch of ctpn_decode_jpeg_batch (or a live canvas of ctpn_decode_jpeg_*_ragged) was produced in the ctx's copy queue: qs waits for it. It is only read (a forward may read it too)
int wait_live_batch(ctpn_ctx* c, const uint8_t* images_dev, hipStream_t qs) {
  for (auto& J : c->jpeg) if (J.ready_valid && J.out_dev.get() == images_dev) CTPN_HIP_TRY(hipStreamWaitEvent(qs, J.ev_ready, 0));
  return CTPN_OK;
}

int stage_pixels(ctpn_ctx* c, const uint8_t* images, int on_device, size_t bytes, size_t slack, DevBuf& buf, hipStream_t qs, const uint8_t*& px) {
  px = images;
  if (on_device) return wait_live_batch(c, images, qs);
  if (int rc = buf.grow(bytes + slack)) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(buf.get(), images, bytes, hipMemcpyHostToDevice, qs));
  px = buf.as<uint8_t>();
  return CTPN_OK;
}

int annotate_batch(ctpn_ctx* c, const std::string& who, const char* format, StageSizeCheck size_check, const uint8_t* images, int on_device, int n, int h, int w, const double* recs,
                   int line_capacity, const int* line_counts, double scale, const char* const* paths, const uint8_t*& px, int& dh, int& dw) {
  if (!c || !images || !line_counts || !paths) return fail(CTPN_ERR_ARG, who + ": null pointer");
  if (n <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535 || line_capacity < 0 || !(scale > 0.0)) return fail(CTPN_ERR_ARG, who + ": empty batch / bad size / bad scale");
  for (int i = 0; i < n; ++i) {
    if (!paths[i]) return fail(CTPN_ERR_ARG, who + ": null path");
    if (line_counts[i] < 0 || line_counts[i] > line_capacity || (line_counts[i] > 0 && !recs)) return fail(CTPN_ERR_ARG, who + ": line count out of range");
  }
  if (c->postproc_only) return fail(CTPN_ERR_STATE, who + ": post-processing-only ctx");
  // demo.py:51: cv2.resize(img, None, None, fx = 1 / scale, fy = 1 / scale); the identity (scale 1) is a copy there and no launch here
  const double f = 1.0 / scale;
  dh = h; dw = w;
  if (f != 1.0) { dh = resize_out_dim(h, f); dw = resize_out_dim(w, f); }
  if (dh <= 0 || dw <= 0 || dh > 65535 || dw > 65535) return fail(CTPN_ERR_ARG, who + ": the resized image is empty or too large for a " + format + " file");
  int rc;
  if (size_check && ((rc = size_check(who, h, w)) || (rc = size_check(who, dh, dw)))) return rc;
  CTPN_HIP_TRY(hipSetDevice(c->device));
  auto& S = c->stage;
  hipStream_t qs = c->stream_c;
  const size_t bytes = (size_t)n * h * w * 3;
  if ((rc = S.img_dev.grow(bytes + 256))) return rc;
  if (f != 1.0 && (rc = S.rs_dev.grow((size_t)n * dh * dw * 3 + 256))) return rc;
  if ((rc = S.recs_dev.grow(std::max<size_t>((size_t)n * line_capacity * 9 * sizeof(double), 64)))) return rc;
  if ((rc = S.cnt_dev.grow((size_t)n * sizeof(int)))) return rc;
  // the outlines go onto a copy owned by the ctx: a live batch of ctpn_decode_jpeg_batch (produced in this queue) may still feed a forward
  if (on_device && (rc = wait_live_batch(c, images, qs))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(S.img_dev.as<uint8_t>(), images, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, qs));
  if (recs && line_capacity > 0) CTPN_HIP_TRY(hipMemcpyAsync(S.recs_dev.as<double>(), recs, (size_t)n * line_capacity * 9 * sizeof(double), hipMemcpyHostToDevice, qs));
  CTPN_HIP_TRY(hipMemcpyAsync(S.cnt_dev.as<int>(), line_counts, (size_t)n * sizeof(int), hipMemcpyHostToDevice, qs));
  if ((rc = launch_draw_boxes(S.img_dev.as<uint8_t>(), S.recs_dev.as<double>(), S.cnt_dev.as<int>(), line_capacity, n, h, w, qs))) return rc;
  px = S.img_dev.as<uint8_t>();
  if (f != 1.0) {
    if ((rc = launch_resize_linear(S.img_dev.as<uint8_t>(), S.rs_dev.as<uint8_t>(), 0, n, h, w, dh, dw, f, f, qs))) return rc;
    px = S.rs_dev.as<uint8_t>();
  }
  return CTPN_OK;
}

void write_file(const char* path, const uint8_t* data, size_t bytes, int& st, std::string& msg) {
  std::FILE* f = std::fopen(path, "wb");
  if (!f) { st = CTPN_ERR_ARG; msg = std::string("cannot open ") + path; return; }
  const bool ok = std::fwrite(data, 1, bytes, f) == bytes;
  if (std::fclose(f) != 0 || !ok) { st = CTPN_ERR_ARG; msg = std::string("write failed: ") + path; }
}

int first_failure(const char* who, const std::vector<int>& st, const std::vector<std::string>& msg) {
  for (size_t i = 0; i < st.size(); ++i) if (st[i]) return fail(st[i], std::string(who) + ": image " + std::to_string(i) + ": " + msg[i]);
  return CTPN_OK;
}

}  // namespace ctpn
