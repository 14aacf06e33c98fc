// C ABI of libctpn_hip.so, input unit: JPEG probe / host entropy decode of one file (jpeg.hip), resize (preprocess.hip). The batched decode
// to device images: api_jpeg_decode.hip.
#include "ctx.h"

namespace ctpn {

bool jpeg_read_file(const char* path, std::vector<uint8_t>& buf, size_t limit) {
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

void jpeg_layout8(const JpegGeom& g, int* layout8) {
  const int l8[8] = {g.h, g.w, g.ncomp, g.hs0 | ((g.orient - 1) << 8), g.bw[0], g.bw[1], g.bh[0], g.bh[1]};
  std::memcpy(layout8, l8, sizeof(l8));
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
  jpeg_layout8(g, layout8);
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
  Stream st;
  DevBuf ds, dd;      // released before the stream, on every way out
  if ((rc = st.ensure())) return rc;
  const void* s_in = src;
  if (!src_on_device) {
    if ((rc = ds.alloc(sbytes))) return rc;
    CTPN_HIP_TRY(hipMemcpyAsync(ds.get(), src, sbytes, hipMemcpyHostToDevice, st));
    s_in = ds.get();
  }
  void* d_out = dst;
  if (!dst_on_device) { if ((rc = dd.alloc(dbytes))) return rc; d_out = dd.get(); }
  if ((rc = launch_resize_linear(s_in, d_out, src_is_f32, n, h, w, dh, dw, fx, fy, st))) return rc;
  if (!dst_on_device) CTPN_HIP_TRY(hipMemcpyAsync(dst, dd.get(), dbytes, hipMemcpyDeviceToHost, st));
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

}  // extern "C"
