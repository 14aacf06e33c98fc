// C ABI of libctpn_hip.so, input unit: JPEG probe / entropy decode / batched decode to device images (kernels: jpeg.hip), resize (preprocess.hip).
#include "ctx.h"

namespace ctpn {

// grow a device buffer to `need` bytes; the old allocation is retired (it may still be read by work in flight, or be held by the caller)
static int jpeg_grow_dev(ctpn_ctx* c, void** p, size_t& have, size_t need) {
  if (need <= have) return CTPN_OK;
  void* q = nullptr;
  CTPN_HIP_TRY(hipMalloc(&q, need));
  if (*p) c->jpeg_retired.push_back(*p);
  *p = q; have = need;
  return CTPN_OK;
}

static int jpeg_reserve(ctpn_ctx* c, ctpn_ctx::JpegBufs& J, size_t n, size_t cap, size_t raw_bytes, size_t out_bytes) {
  if (!c->jpeg_ready) {
    for (auto& j : c->jpeg)
      for (hipEvent_t* e : {&j.ev_h2d, &j.ev_ready, &j.ev_consumed}) CTPN_HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    c->jpeg_ready = true;
  }
  int rc;
  if (n * cap > J.coef_elems) {        // (the copy that last read the page-locked block has been waited for by the caller)
    if (J.coef_host) CTPN_HIP_TRY(hipHostFree(J.coef_host));
    J.coef_host = nullptr;
    J.coef_elems = 0;                  // (a failed allocation below must not leave the old size standing next to a null block)
    CTPN_HIP_TRY(hipHostMalloc((void**)&J.coef_host, n * cap * sizeof(int16_t)));
    size_t have = J.coef_elems * sizeof(int16_t);
    if ((rc = jpeg_grow_dev(c, (void**)&J.coef_dev, have, n * cap * sizeof(int16_t)))) return rc;
    J.coef_elems = n * cap;
  }
  if (n > J.qt_imgs) {
    if (J.qt_host) CTPN_HIP_TRY(hipHostFree(J.qt_host));
    J.qt_host = nullptr;
    J.qt_imgs = 0;
    CTPN_HIP_TRY(hipHostMalloc((void**)&J.qt_host, n * 192 * sizeof(uint16_t)));
    size_t have = J.qt_imgs * 192 * sizeof(uint16_t);
    if ((rc = jpeg_grow_dev(c, (void**)&J.qt_dev, have, n * 192 * sizeof(uint16_t)))) return rc;
    J.qt_imgs = n;
  }
  if ((rc = jpeg_grow_dev(c, (void**)&J.out_dev, J.out_bytes, out_bytes + 256))) return rc;
  if ((rc = jpeg_grow_dev(c, (void**)&c->jpeg_planes, c->jpeg_planes_bytes, n * cap))) return rc;      // one byte per coefficient
  if (raw_bytes && (rc = jpeg_grow_dev(c, (void**)&c->jpeg_raw, c->jpeg_raw_bytes, raw_bytes + 256))) return rc;
  return CTPN_OK;
}

// read a whole file; false if it cannot be read
static bool jpeg_read_file(const char* path, std::vector<uint8_t>& buf, size_t limit = 0) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  bool ok = false;
  if (limit) {
    buf.resize(limit);
    const size_t got = std::fread(buf.data(), 1, limit, f);
    buf.resize(got);
    ok = got > 0;
  } else if (std::fseek(f, 0, SEEK_END) == 0) {
    const long sz = std::ftell(f);
    if (sz > 0 && sz <= (1L << 30) && std::fseek(f, 0, SEEK_SET) == 0) {
      buf.resize((size_t)sz);
      ok = std::fread(buf.data(), 1, (size_t)sz, f) == (size_t)sz;
    }
  }
  std::fclose(f);
  return ok;
}

// one image's bytes for the host half: from the caller's memory, or read from the file inside the worker thread
struct JpegSource {
  const uint8_t* const* mem = nullptr; const size_t* sizes = nullptr;
  const char* const* paths = nullptr;
};

static int jpeg_decode_impl(ctpn_ctx* c, const JpegSource& src, int n, int h, int w, double fx, double fy, const uint8_t** images_dev_out, int* out_h, int* out_w) {
  if (c->postproc_only) return fail(CTPN_ERR_STATE, "ctpn_decode_jpeg_batch: post-processing-only ctx");
  if (n <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_batch: empty batch / bad size");
  const bool resize = (fx > 0.0 && fx != 1.0) || (fy > 0.0 && fy != 1.0);
  if (!(fx > 0.0)) fx = 1.0;
  if (!(fy > 0.0)) fy = 1.0;
  int dh = h, dw = w;
  if (resize) { dh = resize_out_dim(h, fy); dw = resize_out_dim(w, fx); if (dh <= 0 || dw <= 0) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_batch: empty output"); }
  CTPN_HIP_TRY(hipSetDevice(c->device));
  const int b = c->jpeg_flip;
  auto& J = c->jpeg[b];
  // the page-locked coefficient block was last read by the copy of two calls ago
  if (J.h2d_valid) CTPN_HIP_TRY(hipEventSynchronize(J.ev_h2d));
  const size_t cap = jpeg_coef_capacity(h, w);
  int rc = jpeg_reserve(c, J, (size_t)n, cap, resize ? (size_t)n * h * w * 3 : 0, (size_t)n * dh * dw * 3);
  if (rc) return rc;
  // host half: one image per worker thread
  std::vector<JpegGeom> geo((size_t)n);
  std::vector<int> st((size_t)n, CTPN_OK);
  std::vector<std::string> msg((size_t)n);
  c->pool->run(n, [&](int i) {
    const uint8_t* data = nullptr; size_t len = 0;
    static thread_local std::vector<uint8_t> filebuf;      // one per worker thread, reused from batch to batch
    try {
      if (src.paths) {
        if (!jpeg_read_file(src.paths[i], filebuf)) { st[i] = CTPN_ERR_ARG; msg[i] = std::string("cannot read ") + src.paths[i]; return; }
        data = filebuf.data(); len = filebuf.size();
      } else { data = src.mem[i]; len = src.sizes[i]; }
      st[i] = jpeg_entropy_decode(data, len, J.coef_host + (size_t)i * cap, cap, J.qt_host + (size_t)i * 192, &geo[i]);
      if (st[i]) msg[i] = ctpn_last_error();      // (the error text is per thread)
      if (filebuf.capacity() > ((size_t)8 << 20)) std::vector<uint8_t>().swap(filebuf);      // one huge file must not pin its size per worker for the run
    } catch (const std::exception& e) { st[i] = CTPN_ERR_CAPACITY; msg[i] = e.what(); }      // nothing may leave a worker thread
  });
  for (int i = 0; i < n; ++i) if (st[i]) return fail(st[i], "ctpn_decode_jpeg_batch: file " + std::to_string(i) + ": " + msg[i]);
  const JpegGeom& g = geo[0];
  for (int i = 0; i < n; ++i) {
    if (geo[i].oh != h || geo[i].ow != w) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_batch: file " + std::to_string(i) + " is not " + std::to_string(h) + " x " + std::to_string(w) + " (as cv2.imread returns it: EXIF orientation applied)");
    if (geo[i].ncomp != g.ncomp || geo[i].hs0 != g.hs0 || geo[i].vs0 != g.vs0 || geo[i].orient != g.orient) return fail(CTPN_ERR_UNSUPPORTED, "ctpn_decode_jpeg_batch: the files of one batch must share one component layout and one EXIF orientation");
  }
  hipStream_t qs = c->stream_c;
  // the device buffers of this set: the forward that read out_dev two calls ago has passed its first layer
  if (J.consumed_valid) CTPN_HIP_TRY(hipStreamWaitEvent(qs, J.ev_consumed, 0));
  CTPN_HIP_TRY(hipMemcpy2DAsync(J.coef_dev, (size_t)g.coef_per_img * sizeof(int16_t), J.coef_host, cap * sizeof(int16_t), (size_t)g.coef_per_img * sizeof(int16_t), (size_t)n,
                                hipMemcpyHostToDevice, qs));
  CTPN_HIP_TRY(hipMemcpyAsync(J.qt_dev, J.qt_host, (size_t)n * 192 * sizeof(uint16_t), hipMemcpyHostToDevice, qs));
  CTPN_HIP_TRY(hipEventRecord(J.ev_h2d, qs));
  J.h2d_valid = true;
  if ((rc = launch_jpeg_pixels(J.coef_dev, J.qt_dev, c->jpeg_planes, resize ? c->jpeg_raw : J.out_dev, g, n, qs))) return rc;
  // resize_im (reference ctpn/demo.py:21-25: cv2.resize, INTER_LINEAR) of the decoded batch, in the same queue
  if (resize && (rc = launch_resize_linear(c->jpeg_raw, J.out_dev, 0, n, h, w, dh, dw, fx, fy, qs))) return rc;
  CTPN_HIP_TRY(hipEventRecord(J.ev_ready, qs));
  J.ready_valid = true;
  J.consumed_valid = false;      // until a forward reads this buffer
  J.out_n = n; J.out_h = dh; J.out_w = dw;
  c->jpeg_flip ^= 1;
  *images_dev_out = J.out_dev;
  if (out_h) *out_h = dh;
  if (out_w) *out_w = dw;
  return CTPN_OK;
}

}  // namespace ctpn

extern "C" {

// ---- JPEG: host entropy decode + device pixels (jpeg.hip) ----
int ctpn_jpeg_probe(const uint8_t* data, size_t len, int* h, int* w, int* ncomp, int* luma_sampling) {
  if (!data) return fail(CTPN_ERR_ARG, "ctpn_jpeg_probe: null pointer");
  return jpeg_probe(data, len, h, w, ncomp, luma_sampling);
}
size_t ctpn_jpeg_coef_capacity(int h, int w) { return (h > 0 && w > 0) ? jpeg_coef_capacity(h, w) : 0; }
int ctpn_jpeg_entropy_decode(const uint8_t* data, size_t len, int16_t* coef, size_t coef_capacity, uint16_t* qt, int* layout8) {
  if (!data || !coef || !qt || !layout8) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_decode: null pointer");
  JpegGeom g;
  const int rc = jpeg_entropy_decode(data, len, coef, coef_capacity, qt, &g);
  if (rc) return rc;
  const int l8[8] = {g.h, g.w, g.ncomp, g.hs0 | ((g.orient - 1) << 8), g.bw[0], g.bw[1], g.bh[0], g.bh[1]};
  std::memcpy(layout8, l8, sizeof(l8));
  return CTPN_OK;
}

int ctpn_jpeg_probe_files(const char* const* paths, int n, int* info4, int threads) {
  if (!paths || !info4 || n < 0) return fail(CTPN_ERR_ARG, "ctpn_jpeg_probe_files: bad arguments");
  for (int i = 0; i < n; ++i) if (!paths[i]) return fail(CTPN_ERR_ARG, "ctpn_jpeg_probe_files: null path");
  if (threads <= 0) { const unsigned hw = std::thread::hardware_concurrency(); threads = (int)std::min<unsigned>(16u, hw ? hw : 1u); }
  threads = std::max(1, std::min(threads, n));
  std::atomic<int> next(0);
  auto work = [&]() {
    std::vector<uint8_t> buf;
    for (int i; (i = next.fetch_add(1)) < n;) {
      int* o = info4 + 4 * (size_t)i;
      o[0] = o[1] = o[2] = o[3] = 0;
      // the headers normally end within the first 64 KB; a file with larger APPn segments is read whole
      for (const size_t limit : {(size_t)1 << 16, (size_t)0}) {
        if (!jpeg_read_file(paths[i], buf, limit)) break;
        int h = 0, w = 0, nc = 0, hs = 0;
        const int rc = jpeg_probe(buf.data(), buf.size(), &h, &w, &nc, &hs);
        if (rc == CTPN_OK) { o[0] = h; o[1] = w; o[2] = nc; o[3] = hs; break; }
        if (rc == CTPN_ERR_UNSUPPORTED || buf.size() < ((size_t)1 << 16)) break;
      }
    }
  };
  std::vector<std::thread> team;
  for (int t = 1; t < threads; ++t) team.emplace_back(work);
  work();
  for (auto& t : team) t.join();
  return CTPN_OK;
}

int ctpn_decode_jpeg_batch(ctpn_ctx* c, const uint8_t* const* files, const size_t* sizes, int n, int h, int w, double fx, double fy,
                           const uint8_t** images_dev_out, int* out_h, int* out_w) {
  if (!c || !files || !sizes || !images_dev_out) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_batch: null pointer");
  for (int i = 0; i < n; ++i) if (!files[i]) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_batch: null file pointer");
  JpegSource src; src.mem = files; src.sizes = sizes;
  return jpeg_decode_impl(c, src, n, h, w, fx, fy, images_dev_out, out_h, out_w);
}

int ctpn_decode_jpeg_files(ctpn_ctx* c, const char* const* paths, int n, int h, int w, double fx, double fy, const uint8_t** images_dev_out, int* out_h, int* out_w) {
  if (!c || !paths || !images_dev_out) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_files: null pointer");
  for (int i = 0; i < n; ++i) if (!paths[i]) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_files: null path");
  JpegSource src; src.paths = paths;
  return jpeg_decode_impl(c, src, n, h, w, fx, fy, images_dev_out, out_h, out_w);
}

int ctpn_jpeg_batch_fetch(ctpn_ctx* c, const uint8_t* images_dev, uint8_t* host_out, size_t capacity) {
  if (!c || !images_dev || !host_out) return fail(CTPN_ERR_ARG, "ctpn_jpeg_batch_fetch: null pointer");
  for (auto& J : c->jpeg)
    if (J.ready_valid && J.out_dev == images_dev) {
      const size_t bytes = (size_t)J.out_n * J.out_h * J.out_w * 3;
      if (capacity < bytes) return fail(CTPN_ERR_CAPACITY, "ctpn_jpeg_batch_fetch: capacity too small");
      CTPN_HIP_TRY(hipSetDevice(c->device));
      CTPN_HIP_TRY(hipEventSynchronize(J.ev_ready));
      CTPN_HIP_TRY(hipMemcpy(host_out, J.out_dev, bytes, hipMemcpyDeviceToHost));
      return CTPN_OK;
    }
  return fail(CTPN_ERR_STATE, "ctpn_jpeg_batch_fetch: not a live batch of ctpn_decode_jpeg_batch");
}

int ctpn_resize_dims(int h, int w, double fx, double fy, int* out_h, int* out_w) {
  if (!out_h || !out_w || h <= 0 || w <= 0 || !(fx > 0.0) || !(fy > 0.0)) return fail(CTPN_ERR_ARG, "ctpn_resize_dims: bad arguments");
  *out_h = resize_out_dim(h, fy);
  *out_w = resize_out_dim(w, fx);
  if (*out_h <= 0 || *out_w <= 0) return fail(CTPN_ERR_ARG, "ctpn_resize_dims: empty output");
  return CTPN_OK;
}

int ctpn_resize(int device_id, const void* src, int src_is_f32, int src_on_device, int n, int h, int w, double fx, double fy, void* dst,
                int dst_on_device, long long dst_capacity, int* out_h, int* out_w) {
  int dh = 0, dw = 0;
  int rc = ctpn_resize_dims(h, w, fx, fy, &dh, &dw);
  if (rc) return rc;
  if (out_h) *out_h = dh;
  if (out_w) *out_w = dw;
  if (!dst) return CTPN_OK;
  if (!src || n <= 0) return fail(CTPN_ERR_ARG, "ctpn_resize: null source / empty batch");
  const long long need = (long long)n * dh * dw * 3;
  if (dst_capacity < need) return fail(CTPN_ERR_CAPACITY, "ctpn_resize: dst_capacity too small");
  const int ndev = ctpn_device_count();
  if (ndev <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_resize: no HIP device visible (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(CTPN_ERR_ARG, "ctpn_resize: device_id out of range");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  const size_t es = src_is_f32 ? 4 : 1;
  const size_t sbytes = (size_t)n * h * w * 3 * es, dbytes = (size_t)need * es;
  void *ds = nullptr, *dd = nullptr;
  hipStream_t st = nullptr;
  auto cleanup = [&]() { if (ds) (void)hipFree(ds); if (dd) (void)hipFree(dd); if (st) (void)hipStreamDestroy(st); };
#define RS_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { cleanup(); return fail(CTPN_ERR_HIP, std::string("ctpn_resize: ") + hipGetErrorString(e_)); } } while (0)
  RS_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  const void* s_in = src;
  if (!src_on_device) { RS_TRY(hipMalloc(&ds, sbytes)); RS_TRY(hipMemcpyAsync(ds, src, sbytes, hipMemcpyHostToDevice, st)); s_in = ds; }
  void* d_out = dst;
  if (!dst_on_device) { RS_TRY(hipMalloc(&dd, dbytes)); d_out = dd; }
  rc = launch_resize_linear(s_in, d_out, src_is_f32, n, h, w, dh, dw, fx, fy, st);
  if (rc) { cleanup(); return rc; }
  if (!dst_on_device) RS_TRY(hipMemcpyAsync(dst, dd, dbytes, hipMemcpyDeviceToHost, st));
  RS_TRY(hipStreamSynchronize(st));
#undef RS_TRY
  cleanup();
  return CTPN_OK;
}

}  // extern "C"
