// C ABI of libctpn_hip.so, data layer unit: what the reference does to a labelled folder before a training step sees it -- split_label.py's
// 16-px strips for a whole label set, a decoded page resized / mirrored / mean-subtracted, a page's strips as the step's gt boxes
// (data_layer.hip). All three are stateless, in ctpn_anchor_targets' conventions: no ctx, a stream of the call's own that waits for no
// other, device blocks allocated by the call and released before it returns. The definitions: include/ctpn_hip_data_layer.h.
#include "ctx.h"
#include "../../include/ctpn_hip_data_layer.h"
#include "data_layer_dev.h"

#include <cmath>

namespace {
using namespace ctpn;

constexpr int kMaxQuads = 1 << 18;      // x 4097 strips of a 65535-wide page stays below 2^31

int layer_device(int device_id, const char* who) {
  const int ndev = ctpn_device_count();
  if (ndev <= 0) return fail(CTPN_ERR_NODEVICE, std::string(who) + ": no HIP device visible (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev || device_id >= 16) return fail(CTPN_ERR_ARG, std::string(who) + ": device_id out of range");
  return CTPN_OK;
}

}  // namespace

extern "C" {

int ctpn_split_labels(int device_id, int pages, const int* page_dims, const double* quads, const int* quad_offsets, int on_device, float* strips,
                      long long capacity_strips, int* strip_offsets, int* quad_strip_offsets) {
  if (pages <= 0 || pages > (1 << 24)) return fail(CTPN_ERR_ARG, "ctpn_split_labels: pages in 1 .. 2^24");
  if (!page_dims || !quad_offsets || !strip_offsets) return fail(CTPN_ERR_ARG, "ctpn_split_labels: null pointer");
  if (on_device != 0 && on_device != 1) return fail(CTPN_ERR_ARG, "ctpn_split_labels: on_device is 0 or 1");
  if (capacity_strips < 0 || (capacity_strips > 0 && !strips)) return fail(CTPN_ERR_ARG, "ctpn_split_labels: capacity_strips >= 0, and strips with it");
  if (quad_offsets[0] != 0) return fail(CTPN_ERR_ARG, "ctpn_split_labels: quad_offsets starts at 0 and never falls");
  for (int p = 0; p < pages; ++p) {
    if (quad_offsets[p + 1] < quad_offsets[p]) return fail(CTPN_ERR_ARG, "ctpn_split_labels: quad_offsets starts at 0 and never falls");
    for (int k = 0; k < 4; ++k)
      if (page_dims[4 * p + k] < 1 || page_dims[4 * p + k] > 65535) return fail(CTPN_ERR_ARG, "ctpn_split_labels: page_dims holds sizes in 1 .. 65535");
  }
  const int nq = quad_offsets[pages];
  if (nq > kMaxQuads) return fail(CTPN_ERR_ARG, "ctpn_split_labels: more than 2^18 quads in one call");
  if (nq > 0 && !quads) return fail(CTPN_ERR_ARG, "ctpn_split_labels: quads is null");
  int rc = layer_device(device_id, "ctpn_split_labels");
  if (rc) return rc;
  CTPN_HIP_TRY(hipSetDevice(device_id));
  Stream st;
  DevBuf tables, dquads, spans, counts, scan, dstrips;      // released before the stream, on every way out
  if ((rc = st.ensure())) return rc;
  // the small tables, always the host's: the pages' sizes and quad offsets in, their strip offsets out
  const size_t P = (size_t)pages, Q = (size_t)nq;
  std::vector<int> tab(P * 4 + (P + 1));
  std::memcpy(tab.data(), page_dims, P * 4 * sizeof(int));
  std::memcpy(tab.data() + P * 4, quad_offsets, (P + 1) * sizeof(int));
  if ((rc = tables.alloc((tab.size() + P + 1) * sizeof(int)))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(tables.get(), tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
  const int* d_dims = tables.as<int>();
  const int* d_qoffs = d_dims + P * 4;
  int* d_poffs = tables.as<int>() + tab.size();
  const double* d_quads = quads;
  if (!on_device && nq > 0) {
    if ((rc = dquads.alloc(Q * 8 * sizeof(double)))) return rc;
    CTPN_HIP_TRY(hipMemcpyAsync(dquads.get(), quads, dquads.bytes(), hipMemcpyHostToDevice, st));
    d_quads = dquads.as<double>();
  }
  if ((rc = spans.alloc(std::max<size_t>(Q, 1) * sizeof(DlSpan))) || (rc = counts.alloc(std::max<size_t>(Q, 1) * sizeof(uint32_t)))) return rc;
  int* d_scan = quad_strip_offsets;
  if (!(on_device && quad_strip_offsets)) {
    if ((rc = scan.alloc((Q + 1) * sizeof(int)))) return rc;
    d_scan = scan.as<int>();
  }
  if ((rc = launch_split_count(d_quads, nq, d_qoffs, pages, d_dims, spans.get(), counts.as<uint32_t>(), st)) ||
      (rc = launch_split_scan(counts.as<uint32_t>(), nq, d_scan, d_qoffs, pages, d_poffs, st)))
    return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(strip_offsets, d_poffs, (P + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
  if (quad_strip_offsets && !on_device) CTPN_HIP_TRY(hipMemcpyAsync(quad_strip_offsets, d_scan, (Q + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
  CTPN_HIP_TRY(hipStreamSynchronize(st));      // the total decides what follows
  const int total = strip_offsets[pages];
  if (capacity_strips == 0 || total == 0) return CTPN_OK;
  if (capacity_strips < total) return fail(CTPN_ERR_CAPACITY, "ctpn_split_labels: capacity_strips too small (strip_offsets holds the need)");
  float* d_strips = strips;
  if (!on_device) {
    if ((rc = dstrips.alloc((size_t)total * 4 * sizeof(float)))) return rc;
    d_strips = dstrips.as<float>();
  }
  if ((rc = launch_split_write(spans.get(), d_scan, nq, total, d_strips, st))) return rc;
  if (!on_device) CTPN_HIP_TRY(hipMemcpyAsync(strips, d_strips, (size_t)total * 4 * sizeof(float), hipMemcpyDeviceToHost, st));
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

int ctpn_train_page(int device_id, const uint8_t* image, int image_on_device, int h, int w, long long pitch, double factor, int flip, uint8_t* image_out,
                    float* blob_out, int out_h, int out_w) {
  if (!image || !image_out) return fail(CTPN_ERR_ARG, "ctpn_train_page: null pointer");
  if (h <= 0 || w <= 0 || pitch < 3LL * w || (long long)h * pitch > (1LL << 40)) return fail(CTPN_ERR_ARG, "ctpn_train_page: h, w >= 1, pitch >= 3 w");
  if ((image_on_device != 0 && image_on_device != 1) || (flip != 0 && flip != 1)) return fail(CTPN_ERR_ARG, "ctpn_train_page: image_on_device and flip are 0 or 1");
  if (reinterpret_cast<uintptr_t>(blob_out) & 3) return fail(CTPN_ERR_ARG, "ctpn_train_page: blob_out is not 4-byte aligned");
  DlPage p{};
  p.h = h; p.w = w; p.pitch = pitch; p.flip = flip;
  p.resize = factor > 0.0 && factor != 1.0;
  p.oh = h; p.ow = w;
  if (p.resize) {
    if (!std::isfinite(factor)) return fail(CTPN_ERR_ARG, "ctpn_train_page: factor is not finite");
    if (const int rc = ctpn_resize_dims(h, w, factor, factor, &p.oh, &p.ow)) return rc;
    p.inv_f = 1.0 / factor;
  }
  if (out_h != p.oh || out_w != p.ow) return fail(CTPN_ERR_ARG, "ctpn_train_page: out_h x out_w is not ctpn_resize_dims' size of this page");
  int rc = layer_device(device_id, "ctpn_train_page");
  if (rc) return rc;
  CTPN_HIP_TRY(hipSetDevice(device_id));
  Stream st;
  PinnedBuf stage;      // released before the stream, on every way out
  DevBuf dsrc;
  if ((rc = st.ensure())) return rc;
  const uint8_t* src = image;
  if (!image_on_device) {      // one copy: the rows as they lie, pitch included, through a page-locked block
    const size_t bytes = (size_t)(h - 1) * (size_t)pitch + (size_t)w * 3;
    if ((rc = stage.alloc(bytes)) || (rc = dsrc.alloc(bytes))) return rc;
    std::memcpy(stage.get(), image, bytes);
    CTPN_HIP_TRY(hipMemcpyAsync(dsrc.get(), stage.get(), bytes, hipMemcpyHostToDevice, st));
    src = dsrc.as<uint8_t>();
  }
  if ((rc = launch_train_page(src, p, image_out, blob_out, st))) return rc;
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

int ctpn_train_boxes(int device_id, const float* strips, int g, int page_width, int flip, double scale, int on_device, float* gt_boxes_out) {
  if (g < 0 || g > (1 << 26)) return fail(CTPN_ERR_ARG, "ctpn_train_boxes: g in 0 .. 2^26");
  if (page_width < 1 || page_width > 65535) return fail(CTPN_ERR_ARG, "ctpn_train_boxes: page_width in 1 .. 65535 (the boxes are uint16)");
  if ((flip != 0 && flip != 1) || (on_device != 0 && on_device != 1)) return fail(CTPN_ERR_ARG, "ctpn_train_boxes: flip and on_device are 0 or 1");
  if (!std::isfinite(scale)) return fail(CTPN_ERR_ARG, "ctpn_train_boxes: scale is not finite");
  if (g > 0 && (!strips || !gt_boxes_out)) return fail(CTPN_ERR_ARG, "ctpn_train_boxes: null pointer");
  const char* range = "ctpn_train_boxes: a strip holds a value outside 0 .. 65535 (the boxes are uint16)";
  if (!on_device)
    for (size_t i = 0; i < (size_t)g * 4; ++i)
      if (!(strips[i] >= 0.f && strips[i] <= 65535.f)) return fail(CTPN_ERR_ARG, range);
  int rc = layer_device(device_id, "ctpn_train_boxes");
  if (rc) return rc;
  if (g == 0) return CTPN_OK;
  CTPN_HIP_TRY(hipSetDevice(device_id));
  Stream st;
  DevBuf din, dout, dbad;      // released before the stream, on every way out
  if ((rc = st.ensure())) return rc;
  const float* d_in = strips;
  float* d_out = gt_boxes_out;
  const size_t ib = (size_t)g * 4 * sizeof(float), ob = (size_t)g * 5 * sizeof(float);
  if (!on_device) {
    if ((rc = din.alloc(ib)) || (rc = dout.alloc(ob))) return rc;
    CTPN_HIP_TRY(hipMemcpyAsync(din.get(), strips, ib, hipMemcpyHostToDevice, st));
    d_in = din.as<float>();
    d_out = dout.as<float>();
  }
  if ((rc = dbad.alloc(sizeof(int)))) return rc;
  CTPN_HIP_TRY(hipMemsetAsync(dbad.get(), 0, sizeof(int), st));
  if ((rc = launch_train_boxes(d_in, g, page_width, flip, scale, d_out, dbad.as<int>(), st))) return rc;
  int bad = 0;
  CTPN_HIP_TRY(hipMemcpyAsync(&bad, dbad.get(), sizeof(int), hipMemcpyDeviceToHost, st));
  if (!on_device) CTPN_HIP_TRY(hipMemcpyAsync(gt_boxes_out, d_out, ob, hipMemcpyDeviceToHost, st));
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  if (bad) return fail(CTPN_ERR_ARG, range);      // strips on the device: found by the kernel; the rows of such strips are not written
  return CTPN_OK;
}

}  // extern "C"
