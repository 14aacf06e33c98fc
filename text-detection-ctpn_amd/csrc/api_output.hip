// C ABI of libctpn_hip.so, output unit: JPEG writing (kernels and the entropy coder: jpeg_enc.hip) and the annotated result images of
// ctpn/demo.py:28-52 -- outlines (draw_boxes_kernel), cv2.resize by 1 / scale (preprocess.hip), cv2.imwrite -- for a batch on the device.
#include "ctx.h"
#include "jpeg_enc_pixel.h"

namespace ctpn {

static int enc_reserve(ctpn_ctx* c, size_t coef_elems, int quality) {
  auto& E = c->enc;
  if (!E.ev_done) CTPN_HIP_TRY(hipEventCreateWithFlags(&E.ev_done, hipEventDisableTiming));
  if (coef_elems > E.coef_elems) {
    if (E.coef_host) CTPN_HIP_TRY(hipHostFree(E.coef_host));
    E.coef_host = nullptr;
    size_t have = E.coef_elems * sizeof(int16_t);
    E.coef_elems = 0;
    int rc = grow_dev((void**)&E.coef_dev, have, coef_elems * sizeof(int16_t));
    if (rc) return rc;
    CTPN_HIP_TRY(hipHostMalloc((void**)&E.coef_host, coef_elems * sizeof(int16_t)));
    E.coef_elems = coef_elems;
  }
  if (!E.qtab_dev) {
    CTPN_HIP_TRY(hipMalloc(&E.qtab_dev, 128 * sizeof(JencQ)));
    CTPN_HIP_TRY(hipHostMalloc(&E.qtab_host, 128 * sizeof(JencQ)));
  }
  if (E.qtab_quality != quality) {      // (the copy of the previous call has long finished: that call waited for its coefficients)
    jpeg_enc_qtables(quality, nullptr, (JencQ*)E.qtab_host);
    CTPN_HIP_TRY(hipMemcpyAsync(E.qtab_dev, E.qtab_host, 128 * sizeof(JencQ), hipMemcpyHostToDevice, c->stream_c));
    E.qtab_quality = quality;
  }
  return CTPN_OK;
}

// device half in the ctx's copy queue: pixels (device, n x h x w x 3) -> coefficients in the page-locked block; no host wait
static int enc_enqueue(ctpn_ctx* c, const uint8_t* pixels_dev, int n, int h, int w, int quality, JpegGeom& g) {
  jpeg_enc_geom(h, w, g);
  int rc = enc_reserve(c, (size_t)n * (size_t)g.coef_per_img, quality);
  if (rc) return rc;
  auto& E = c->enc;
  if ((rc = launch_jpeg_fdct(pixels_dev, E.coef_dev, (const JencQ*)E.qtab_dev, g, n, c->stream_c))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(E.coef_host, E.coef_dev, (size_t)n * (size_t)g.coef_per_img * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream_c));
  CTPN_HIP_TRY(hipEventRecord(E.ev_done, c->stream_c));
  return CTPN_OK;
}

// host half on the ctx's pool, one image per worker: into the caller's buffers (out), or into files (paths)
static int enc_finish(ctpn_ctx* c, const char* who, const JpegGeom& g, int n, int quality, uint8_t* const* out, const size_t* capacities, size_t* bytes_out, const char* const* paths) {
  auto& E = c->enc;
  CTPN_HIP_TRY(hipEventSynchronize(E.ev_done));
  uint16_t qt[192];
  jpeg_enc_qtables(quality, qt, nullptr);
  std::vector<int> st((size_t)n, CTPN_OK);
  std::vector<std::string> msg((size_t)n);
  const size_t bound = jpeg_encode_capacity(g.h, g.w);
  c->pool->run(n, [&](int i) {
    try {
      const int16_t* coef = E.coef_host + (size_t)i * (size_t)g.coef_per_img;
      size_t bytes = 0;
      if (paths) {
        static thread_local std::vector<uint8_t> filebuf;      // one per worker thread, reused from batch to batch
        if (filebuf.size() < bound) filebuf.resize(bound);
        st[i] = jpeg_entropy_encode(coef, true, g.h, g.w, 2, 2, qt, filebuf.data(), filebuf.size(), &bytes);
        if (st[i]) { msg[i] = ctpn_last_error(); return; }
        std::FILE* f = std::fopen(paths[i], "wb");
        if (!f) { st[i] = CTPN_ERR_ARG; msg[i] = std::string("cannot open ") + paths[i]; return; }
        const bool ok = std::fwrite(filebuf.data(), 1, bytes, f) == bytes;
        if (std::fclose(f) != 0 || !ok) { st[i] = CTPN_ERR_ARG; msg[i] = std::string("write failed: ") + paths[i]; }
        if (filebuf.capacity() > ((size_t)64 << 20)) std::vector<uint8_t>().swap(filebuf);
      } else {
        st[i] = jpeg_entropy_encode(coef, true, g.h, g.w, 2, 2, qt, out[i], capacities[i], &bytes);
        bytes_out[i] = bytes;
        if (st[i]) msg[i] = ctpn_last_error();
      }
    } catch (const std::exception& e) { st[i] = CTPN_ERR_CAPACITY; msg[i] = e.what(); }      // nothing may leave a worker thread
  });
  for (int i = 0; i < n; ++i) if (st[i]) return fail(st[i], std::string(who) + ": image " + std::to_string(i) + ": " + msg[i]);
  return CTPN_OK;
}

}  // namespace ctpn

extern "C" {

size_t ctpn_jpeg_encode_capacity(int h, int w) { return (h > 0 && w > 0 && h <= 65535 && w <= 65535) ? jpeg_encode_capacity(h, w) : 0; }

int ctpn_jpeg_entropy_encode(const int16_t* coef, const int* layout8, const uint16_t* qt, uint8_t* out, size_t capacity, size_t* bytes_out) {
  if (!coef || !layout8 || !qt || !bytes_out || (!out && capacity)) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_encode: null pointer");
  const int h = layout8[0], w = layout8[1], nc = layout8[2], hs = layout8[3] & 0xff, orient = (layout8[3] >> 8) + 1;
  if (nc != 3 || orient != 1) return fail(CTPN_ERR_UNSUPPORTED, "ctpn_jpeg_entropy_encode: three components (YCbCr) and EXIF orientation 1 only");
  if (h <= 0 || w <= 0 || layout8[5] <= 0 || layout8[7] <= 0 || (hs != 1 && hs != 2)) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_encode: bad layout");
  const int vs = layout8[6] / layout8[7];
  if ((vs != 1 && vs != 2) || layout8[4] != layout8[5] * hs || layout8[6] != layout8[7] * vs || layout8[5] != (w + 8 * hs - 1) / (8 * hs) || layout8[7] != (h + 8 * vs - 1) / (8 * vs))
    return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_encode: the block counts do not belong to the size and sampling");
  return jpeg_entropy_encode(coef, false, h, w, hs, vs, qt, out, capacity, bytes_out);
}

int ctpn_encode_jpeg_batch(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, int quality, uint8_t* const* out,
                           const size_t* capacities, size_t* bytes_out) {
  if (!c || !images || !out || !capacities || !bytes_out) return fail(CTPN_ERR_ARG, "ctpn_encode_jpeg_batch: null pointer");
  if (n <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535) return fail(CTPN_ERR_ARG, "ctpn_encode_jpeg_batch: empty batch / bad size");
  if (quality < 1 || quality > 100) return fail(CTPN_ERR_ARG, "ctpn_encode_jpeg_batch: quality must be 1 .. 100");
  for (int i = 0; i < n; ++i) if (!out[i] && capacities[i]) return fail(CTPN_ERR_ARG, "ctpn_encode_jpeg_batch: null output pointer");
  if (c->postproc_only) return fail(CTPN_ERR_STATE, "ctpn_encode_jpeg_batch: post-processing-only ctx");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  auto& E = c->enc;
  const uint8_t* px = images;
  int rc;
  if (!images_on_device) {
    const size_t bytes = (size_t)n * h * w * 3;
    if ((rc = grow_dev((void**)&E.img_dev, E.img_bytes, bytes + 256))) return rc;
    CTPN_HIP_TRY(hipMemcpyAsync(E.img_dev, images, bytes, hipMemcpyHostToDevice, c->stream_c));
    px = E.img_dev;
  } else {
    for (auto& J : c->jpeg) if (J.ready_valid && J.out_dev == images) CTPN_HIP_TRY(hipStreamWaitEvent(c->stream_c, J.ev_ready, 0));
  }
  JpegGeom g;
  if ((rc = enc_enqueue(c, px, n, h, w, quality, g))) return rc;
  return enc_finish(c, "ctpn_encode_jpeg_batch", g, n, quality, out, capacities, bytes_out, nullptr);
}

int ctpn_write_annotated_files(ctpn_ctx* c, const uint8_t* images_dev, int n, int h, int w, const double* recs, int line_capacity, const int* line_counts,
                               double scale, const char* const* paths, int quality) {
  if (!c || !images_dev || !line_counts || !paths) return fail(CTPN_ERR_ARG, "ctpn_write_annotated_files: null pointer");
  if (n <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535 || line_capacity < 0 || !(scale > 0.0)) return fail(CTPN_ERR_ARG, "ctpn_write_annotated_files: empty batch / bad size / bad scale");
  if (quality < 1 || quality > 100) return fail(CTPN_ERR_ARG, "ctpn_write_annotated_files: quality must be 1 .. 100");
  for (int i = 0; i < n; ++i) {
    if (!paths[i]) return fail(CTPN_ERR_ARG, "ctpn_write_annotated_files: null path");
    if (line_counts[i] < 0 || line_counts[i] > line_capacity || (line_counts[i] > 0 && !recs)) return fail(CTPN_ERR_ARG, "ctpn_write_annotated_files: line count out of range");
  }
  if (c->postproc_only) return fail(CTPN_ERR_STATE, "ctpn_write_annotated_files: post-processing-only ctx");
  // demo.py:51: cv2.resize(img, None, None, fx = 1 / scale, fy = 1 / scale); the identity (scale 1) is a copy there and no launch here
  const double f = 1.0 / scale;
  int dh = h, dw = w;
  if (f != 1.0) { dh = resize_out_dim(h, f); dw = resize_out_dim(w, f); }
  if (dh <= 0 || dw <= 0 || dh > 65535 || dw > 65535) return fail(CTPN_ERR_ARG, "ctpn_write_annotated_files: the resized image is empty or too large for a JPEG file");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  auto& E = c->enc;
  hipStream_t qs = c->stream_c;
  const size_t bytes = (size_t)n * h * w * 3;
  int rc;
  if ((rc = grow_dev((void**)&E.img_dev, E.img_bytes, bytes + 256))) return rc;
  if (f != 1.0 && (rc = grow_dev((void**)&E.rs_dev, E.rs_bytes, (size_t)n * dh * dw * 3 + 256))) return rc;
  const size_t rbytes = std::max<size_t>((size_t)n * line_capacity * 9 * sizeof(double), 64);
  if ((rc = grow_dev((void**)&E.recs_dev, E.recs_bytes, rbytes))) return rc;
  size_t cnt_bytes = E.cnt_n * sizeof(int);
  if ((rc = grow_dev((void**)&E.cnt_dev, cnt_bytes, (size_t)n * sizeof(int)))) return rc;
  E.cnt_n = cnt_bytes / sizeof(int);
  // a live batch of ctpn_decode_jpeg_batch was produced in this queue; its buffer is not drawn on (a forward may still read it): a copy is
  for (auto& J : c->jpeg) if (J.ready_valid && J.out_dev == images_dev) CTPN_HIP_TRY(hipStreamWaitEvent(qs, J.ev_ready, 0));
  CTPN_HIP_TRY(hipMemcpyAsync(E.img_dev, images_dev, bytes, hipMemcpyDeviceToDevice, qs));
  if (recs && line_capacity > 0) CTPN_HIP_TRY(hipMemcpyAsync(E.recs_dev, recs, (size_t)n * line_capacity * 9 * sizeof(double), hipMemcpyHostToDevice, qs));
  CTPN_HIP_TRY(hipMemcpyAsync(E.cnt_dev, line_counts, (size_t)n * sizeof(int), hipMemcpyHostToDevice, qs));
  if ((rc = launch_draw_boxes(E.img_dev, E.recs_dev, E.cnt_dev, line_capacity, n, h, w, qs))) return rc;
  const uint8_t* px = E.img_dev;
  if (f != 1.0) {
    if ((rc = launch_resize_linear(E.img_dev, E.rs_dev, 0, n, h, w, dh, dw, f, f, qs))) return rc;
    px = E.rs_dev;
  }
  JpegGeom g;
  if ((rc = enc_enqueue(c, px, n, dh, dw, quality, g))) return rc;
  return enc_finish(c, "ctpn_write_annotated_files", g, n, quality, nullptr, nullptr, nullptr, paths);
}

}  // extern "C"
