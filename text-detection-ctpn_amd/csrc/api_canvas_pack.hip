// C ABI of libctpn_hip.so, canvas unit: decoded BGR images of mixed sizes -> one ragged canvas on the device (ctpn_pack_canvas), and PNG files
// of mixed sizes through it (ctpn_decode_png_files_ragged). Kernel: canvas_pack.hip. The buffer sets, their events and the flip are the
// JPEG decode calls' (api_jpeg_decode.hip: c->jpeg, taken in turn with them), so whatever takes a live decoded batch takes a packed canvas.
#include "ctx.h"

namespace ctpn {

namespace {

inline size_t cp_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// One pack call. A call checks its arguments (check: everything that needs no device, before any work), takes its buffer set (begin), has
// its host sources written into the page-locked block (the caller's rows, or the PNG decoder's output), and runs (run): ONE host-to-device
// copy of [descriptors | host pixels], the kernel, the publication of the canvas.
struct CanvasPack {
  ctpn_ctx* c;
  std::string who;                      // "<entry point>: ", in front of every message
  const char* item;                     // "image" / "file": what an index names in a message
  int n, hc, wc;
  std::vector<int> h, w, dh;
  std::vector<double> fac;
  std::vector<long long> off, pitch;    // of the source as the kernel reads it: byte offset from its base, row pitch
  size_t tab_bytes = 0, pix_bytes = 0;  // the staged block: descriptors (rounded up to 16 bytes), then the host sources' pixels
  ctpn_ctx::JpegBufs* J = nullptr;
  hipStream_t qs;

  CanvasPack(ctpn_ctx* c_, const char* who_, const char* item_, int n_, int hc_, int wc_)
      : c(c_), who(std::string(who_) + ": "), item(item_), n(n_), hc(hc_), wc(wc_), qs(c_->stream_c) {}

  std::string name(int i) const { return std::string(item) + " " + std::to_string(i); }

  // ctpn_decode_jpeg_batch_ragged's rule: every width maps to wc, every height into 16 .. hc
  int check(const int* img_h, const int* img_w, const double* factors) {
    if (c->postproc_only) return fail(CTPN_ERR_STATE, who + "post-processing-only ctx");
    if (n <= 0 || hc < 16 || wc <= 0 || hc > 65535 || wc > 65535) return fail(CTPN_ERR_ARG, who + "empty batch / bad canvas size (hc >= 16)");
    if (n > c->max_batch || hc > c->max_h || wc > c->max_w)
      return fail(CTPN_ERR_ARG, who + "batch " + std::to_string(n) + " x " + std::to_string(hc) + " x " + std::to_string(wc) + " exceeds the ctx's " + std::to_string(c->max_batch) + " x " +
                                    std::to_string(c->max_h) + " x " + std::to_string(c->max_w));
    h.resize((size_t)n); w.resize((size_t)n); dh.resize((size_t)n); fac.resize((size_t)n); off.resize((size_t)n); pitch.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
      const int hi = img_h[i], wi = img_w[i];
      if (hi <= 0 || wi <= 0 || hi > 65535 || wi > 65535) return fail(CTPN_ERR_ARG, who + name(i) + ": bad size");
      const double f = factors[i] > 0.0 ? factors[i] : 1.0;
      const int dhi = f == 1.0 ? hi : resize_out_dim(hi, f), dwi = f == 1.0 ? wi : resize_out_dim(wi, f);
      if (dwi != wc) return fail(CTPN_ERR_ARG, who + name(i) + ": width " + std::to_string(wi) + " maps to " + std::to_string(dwi) + ", not to the canvas's " + std::to_string(wc));
      if (dhi < 16 || dhi > hc) return fail(CTPN_ERR_ARG, who + name(i) + ": height " + std::to_string(hi) + " maps to " + std::to_string(dhi) + ", outside 16 .. " + std::to_string(hc));
      h[i] = hi; w[i] = wi; dh[i] = dhi; fac[i] = f;
    }
    tab_bytes = cp_up((size_t)n * CP_DESC_BYTES, 16);
    return CTPN_OK;
  }

  // host sources: image i at the prefix sum of the sizes before it, rows at pitch 3 w
  void layout_staged() {
    size_t at = 0;
    for (int i = 0; i < n; ++i) { off[i] = (long long)at; pitch[i] = 3LL * w[i]; at += (size_t)h[i] * w[i] * 3; }
    pix_bytes = at;
  }

  // this call's buffer set, large enough. The page-locked block was last read by the copy of two calls ago
  int begin() {
    CTPN_HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = jpeg_sets_ready(c))) return rc;
    J = &c->jpeg[c->jpeg_flip];
    if (J->h2d_valid) CTPN_HIP_TRY(hipEventSynchronize(J->ev_h2d));
    // a device block that grows is retired, not freed: work in flight may still read it, and the caller may hold a pointer into it
    if ((rc = J->src_host.grow(tab_bytes + pix_bytes))) return rc;
    if ((rc = J->src_dev.grow_retiring(tab_bytes + pix_bytes + 256, c->jpeg_retired))) return rc;
    return J->out_dev.grow_retiring((size_t)n * hc * wc * 3 + 256, c->jpeg_retired);
  }

  uint8_t* staged(int i) const { return J->src_host.as<uint8_t>() + tab_bytes + off[i]; }

  // src_base: what the descriptors' offsets count from -- null: the staged pixels' device copy
  int run(const uint8_t* src_base, const uint8_t* const* live /* device sources, nullable */, const uint8_t** canvas_dev_out, int* heights_out) {
    canvas_pack_fill(J->src_host.get(), n, off.data(), pitch.data(), h.data(), w.data(), fac.data(), dh.data());
    // the device buffers of this set: the forward that read out_dev two calls ago has passed its first layer
    if (J->consumed_valid) CTPN_HIP_TRY(hipStreamWaitEvent(qs, J->ev_consumed, 0));
    int rc;
    if (live) for (int i = 0; i < n; ++i) if ((rc = wait_live_batch(c, live[i], qs))) return rc;      // a source that is itself a live decoded batch
    uint8_t* D = J->src_dev.as<uint8_t>();
    CTPN_HIP_TRY(hipMemcpyAsync(D, J->src_host.get(), tab_bytes + (src_base ? 0 : pix_bytes), hipMemcpyHostToDevice, qs));
    CTPN_HIP_TRY(hipEventRecord(J->ev_h2d, qs));
    J->h2d_valid = true;
    if ((rc = launch_canvas_pack(src_base ? src_base : D + tab_bytes, J->out_dev.as<uint8_t>(), D, n, hc, wc, qs))) return rc;
    CTPN_HIP_TRY(hipEventRecord(J->ev_ready, qs));
    J->ready_valid = true;
    J->consumed_valid = false;      // until a forward reads this buffer
    J->out_n = n; J->out_h = hc; J->out_w = wc;
    c->jpeg_flip ^= 1;
    *canvas_dev_out = J->out_dev.as<uint8_t>();
    for (int i = 0; i < n; ++i) heights_out[i] = dh[i];
    return CTPN_OK;
  }
};

// no ctx: a process without a device cannot have made one, and says so -- there is no host form of these calls
int no_ctx(const char* who) {
  if (ctpn_device_count() <= 0) return fail(CTPN_ERR_NODEVICE, std::string(who) + ": no HIP device visible (this library has no CPU fallback)");
  return fail(CTPN_ERR_ARG, std::string(who) + ": null pointer");
}

}  // namespace

}  // namespace ctpn

extern "C" {

int ctpn_pack_canvas(ctpn_ctx* c, const uint8_t* const* images, const int* img_h, const int* img_w, const long long* pitches, int images_on_device, int n,
                     const double* factors, int hc, int wc, const uint8_t** canvas_dev_out, int* heights_out) {
  const char* who = "ctpn_pack_canvas";
  if (!c) return no_ctx(who);
  if (!images || !img_h || !img_w || !factors || !canvas_dev_out || !heights_out) return fail(CTPN_ERR_ARG, std::string(who) + ": null pointer");
  CanvasPack P(c, who, "image", n, hc, wc);
  int rc;
  if ((rc = P.check(img_h, img_w, factors))) return rc;
  for (int i = 0; i < n; ++i) {
    if (!images[i]) return fail(CTPN_ERR_ARG, P.who + P.name(i) + ": null image pointer");
    if (pitches && pitches[i] < 3LL * img_w[i]) return fail(CTPN_ERR_ARG, P.who + P.name(i) + ": pitch " + std::to_string(pitches[i]) + " is less than 3 x its width");
  }
  if (images_on_device) {
    // read in place: offsets from the lowest pointer, the caller's pitches
    uintptr_t base = (uintptr_t)images[0];
    for (int i = 1; i < n; ++i) base = std::min(base, (uintptr_t)images[i]);
    for (int i = 0; i < n; ++i) { P.off[i] = (long long)((uintptr_t)images[i] - base); P.pitch[i] = pitches ? pitches[i] : 3LL * P.w[i]; }
    if ((rc = P.begin())) return rc;
    return P.run((const uint8_t*)base, images, canvas_dev_out, heights_out);
  }
  P.layout_staged();
  if ((rc = P.begin())) return rc;
  c->pool->run(n, [&](int i) {
    const size_t row = (size_t)P.w[i] * 3, sp = pitches ? (size_t)pitches[i] : row;
    uint8_t* dst = P.staged(i);
    if (sp == row) std::memcpy(dst, images[i], row * P.h[i]);
    else for (int y = 0; y < P.h[i]; ++y) std::memcpy(dst + (size_t)y * row, images[i] + (size_t)y * sp, row);
  });
  return P.run(nullptr, nullptr, canvas_dev_out, heights_out);
}

int ctpn_decode_png_files_ragged(ctpn_ctx* c, const char* const* paths, int n, const int* file_h, const int* file_w, const double* factors, int hc, int wc,
                                 const uint8_t** canvas_dev_out, int* heights_out) {
  const char* who = "ctpn_decode_png_files_ragged";
  if (!c) return no_ctx(who);
  if (!paths || !file_h || !file_w || !factors || !canvas_dev_out || !heights_out) return fail(CTPN_ERR_ARG, std::string(who) + ": null pointer");
  CanvasPack P(c, who, "file", n, hc, wc);
  int rc;
  if ((rc = P.check(file_h, file_w, factors))) return rc;
  for (int i = 0; i < n; ++i) if (!paths[i]) return fail(CTPN_ERR_ARG, P.who + P.name(i) + ": null path");
  P.layout_staged();
  if ((rc = P.begin())) return rc;
  // the host decoder, one file per worker, straight into the page-locked block at the file's offset
  std::vector<int> st((size_t)n, CTPN_OK);
  std::vector<std::string> msg((size_t)n);
  c->pool->run(n, [&](int i) { st[i] = png_decode_file(paths[i], P.staged(i), (size_t)P.h[i] * P.w[i] * 3, P.h[i], P.w[i], msg[i]); });
  for (int i = 0; i < n; ++i) if (st[i]) return fail(st[i], P.who + P.name(i) + " (" + paths[i] + "): " + msg[i]);
  return P.run(nullptr, nullptr, canvas_dev_out, heights_out);
}

}  // extern "C"
