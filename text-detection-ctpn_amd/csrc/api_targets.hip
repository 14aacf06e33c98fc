// C ABI of libctpn_hip.so, targets unit: the label side of training -- lib/utils/bbox.pyx's two functions, anchor_target_layer and
// Network.build_loss on the device (targets.hip). All four are stateless: no ctx is read or written. Each call runs on a stream of its own,
// which waits for no other stream, and synchronises once, at its end; its device blocks are allocated by the call and released before it
// returns (a release waits for the whole device: a ctx's work in flight keeps its results but is held up for that moment; a per-device
// cache of stream and scratch is not built). The definitions: include/ctpn_hip.h, "anchor targets and the RPN loss".
#include "ctx.h"
#include "targets_dev.h"

#include <cmath>

namespace {
using namespace ctpn;

const double kTargetDefaults[CTPN_TARGET_CFG_DOUBLES] = {0.3, 0.7, 0.0, 0.5, 300.0, 0.5, 1.0, 0.0, 1.0, 0.0, 1.0, -1.0};

int targets_device(int device_id, const char* who) {
  const int ndev = ctpn_device_count();
  if (ndev <= 0) return fail(CTPN_ERR_NODEVICE, std::string(who) + ": no HIP device visible (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev || device_id >= 16) return fail(CTPN_ERR_ARG, std::string(who) + ": device_id out of range");
  return CTPN_OK;
}

int target_cfg_from12(const double* c, TgCfg& out) {
  if (!c) c = kTargetDefaults;
  for (int i = 0; i < CTPN_TARGET_CFG_DOUBLES; ++i)
    if (!std::isfinite(c[i])) return fail(CTPN_ERR_ARG, "ctpn_anchor_targets: cfg12 holds a value that is not finite");
  if (c[0] < 0.0 || c[0] > 1.0 || c[1] < 0.0 || c[1] > 1.0 || c[3] < 0.0 || c[3] > 1.0 || c[5] < 0.0)
    return fail(CTPN_ERR_ARG, "ctpn_anchor_targets: cfg12: the overlap thresholds and RPN_FG_FRACTION lie in [0, 1], DONTCARE_AREA_INTERSECTION_HI is >= 0");
  if (c[4] < 0.0 || c[4] > 2147483647.0 || c[4] != std::floor(c[4]))
    return fail(CTPN_ERR_ARG, "ctpn_anchor_targets: cfg12: RPN_BATCHSIZE is a whole number in 0 .. 2^31 - 1 (0: no subsampling)");
  if (c[11] >= 0.0) return fail(CTPN_ERR_UNSUPPORTED, "ctpn_anchor_targets: cfg12: RPN_POSITIVE_WEIGHT >= 0 is not built (only the uniform weighting, a negative value)");
  out.neg = c[0]; out.pos = c[1]; out.clobber = c[2] != 0.0; out.fg_fraction = c[3]; out.batch = (long long)c[4]; out.dc_hi = c[5];
  out.preclude_hard = c[6] != 0.0;
  for (int i = 0; i < 4; ++i) out.inside_w[i] = (float)c[7 + i];
  return CTPN_OK;
}

// offsets of a ragged table: n + 1 ints from 0, never falling -> the total, or -1
long long ragged_total(const int* offs, int n) {
  if (offs[0] != 0) return -1;
  for (int i = 0; i < n; ++i) if (offs[i + 1] < offs[i]) return -1;
  return offs[n];
}

// a tensor-sized argument of a call: the caller's device pointer, or a device block of this call that is filled from / copied back to the
// caller's host array
struct Arg {
  DevBuf buf;
  void* dev = nullptr;
  void* host = nullptr;
  size_t bytes = 0;
  // in: copied to the device now. host == null (an optional array): dev stays null
  int in(const void* p, size_t nbytes, int on_device, hipStream_t s) {
    bytes = nbytes;
    if (!p || nbytes == 0) return CTPN_OK;
    if (on_device) { dev = const_cast<void*>(p); return CTPN_OK; }
    if (const int rc = buf.alloc(nbytes)) return rc;
    dev = buf.get();
    CTPN_HIP_TRY(hipMemcpyAsync(dev, p, nbytes, hipMemcpyHostToDevice, s));
    return CTPN_OK;
  }
  // out: a block now, fetch() later. scratch: the call needs the array even if the caller does not ask for it
  int out(void* p, size_t nbytes, int on_device, bool scratch = false) {
    bytes = nbytes;
    if (!p && !scratch) return CTPN_OK;
    if (p && on_device) { dev = p; return CTPN_OK; }
    if (const int rc = buf.alloc(nbytes)) return rc;
    dev = buf.get();
    host = p;
    return CTPN_OK;
  }
  int fetch(hipStream_t s) {
    if (host) CTPN_HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
    return CTPN_OK;
  }
  template <class T> T* as() const { return static_cast<T*>(dev); }
};

}  // namespace

extern "C" {

int ctpn_target_config_default(double* cfg12) {
  if (!cfg12) return fail(CTPN_ERR_ARG, "ctpn_target_config_default: cfg12 is null");
  std::memcpy(cfg12, kTargetDefaults, sizeof(kTargetDefaults));
  return CTPN_OK;
}

int ctpn_bbox_overlaps(int device_id, const double* boxes, int n, const double* query, int k, double* out, int intersections) {
  if (n < 0 || k < 0 || (intersections != 0 && intersections != 1)) return fail(CTPN_ERR_ARG, "ctpn_bbox_overlaps: n, k >= 0, intersections is 0 or 1");
  if (n == 0 || k == 0) return CTPN_OK;
  if (!boxes || !query || !out) return fail(CTPN_ERR_ARG, "ctpn_bbox_overlaps: null pointer");
  if ((long long)n * k > (1LL << 31)) return fail(CTPN_ERR_ARG, "ctpn_bbox_overlaps: n x k beyond 2^31 pairs");
  int rc = targets_device(device_id, "ctpn_bbox_overlaps");
  if (rc) return rc;
  CTPN_HIP_TRY(hipSetDevice(device_id));
  Stream st;
  DevBuf db, dq, dout;      // released before the stream, on every way out
  if ((rc = st.ensure())) return rc;
  const size_t ob = (size_t)n * k * sizeof(double);
  if ((rc = db.alloc((size_t)n * 4 * sizeof(double))) || (rc = dq.alloc((size_t)k * 4 * sizeof(double))) || (rc = dout.alloc(ob))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(db.get(), boxes, db.bytes(), hipMemcpyHostToDevice, st));
  CTPN_HIP_TRY(hipMemcpyAsync(dq.get(), query, dq.bytes(), hipMemcpyHostToDevice, st));
  if ((rc = launch_bbox_overlaps(db.as<double>(), n, dq.as<double>(), k, dout.as<double>(), intersections, st))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(out, dout.get(), ob, hipMemcpyDeviceToHost, st));
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

int ctpn_anchor_targets(int device_id, int n, int hf, int wf, const float* im_info, const float* gt_boxes, const int* gt_offsets, const int* gt_hard,
                        const float* dontcare, const int* dc_offsets, const double* cfg12, unsigned long long seed, int on_device, float* labels,
                        float* bbox_targets, float* inside_weights, float* outside_weights, int* stats, float* labels_presample, double* max_overlap,
                        int* argmax) {
  if (n <= 0 || n > 65535 || hf <= 0 || wf <= 0) return fail(CTPN_ERR_ARG, "ctpn_anchor_targets: n in 1 .. 65535, hf, wf >= 1");
  if (!im_info || !gt_offsets || !labels || !bbox_targets || !inside_weights || !outside_weights || !stats)
    return fail(CTPN_ERR_ARG, "ctpn_anchor_targets: null pointer");
  const long long A64 = (long long)hf * wf * TG_A;
  if (A64 > TG_MAX_ANCHORS) return fail(CTPN_ERR_ARG, "ctpn_anchor_targets: hf x wf x 10 beyond 2^24 anchors per image");
  if ((long long)n * A64 * 4 > (1LL << 32)) return fail(CTPN_ERR_ARG, "ctpn_anchor_targets: n x hf x wf x 40 beyond 2^32 values");
  const long long total = ragged_total(gt_offsets, n);
  if (total < 0) return fail(CTPN_ERR_ARG, "ctpn_anchor_targets: gt_offsets starts at 0 and never falls");
  if (total > 0 && !gt_boxes) return fail(CTPN_ERR_ARG, "ctpn_anchor_targets: gt_boxes is null");
  long long total_dc = 0;
  if (dontcare) {
    if (!dc_offsets) return fail(CTPN_ERR_ARG, "ctpn_anchor_targets: dontcare without dc_offsets");
    if ((total_dc = ragged_total(dc_offsets, n)) < 0) return fail(CTPN_ERR_ARG, "ctpn_anchor_targets: dc_offsets starts at 0 and never falls");
  }
  if (on_device != 0 && on_device != 1) return fail(CTPN_ERR_ARG, "ctpn_anchor_targets: on_device is 0 or 1");
  TgCfg cfg;
  int rc = target_cfg_from12(cfg12, cfg);
  if (rc) return rc;
  if ((rc = targets_device(device_id, "ctpn_anchor_targets"))) return rc;
  CTPN_HIP_TRY(hipSetDevice(device_id));
  int max_g = 0;
  for (int i = 0; i < n; ++i) max_g = std::max(max_g, gt_offsets[i + 1] - gt_offsets[i]);
  const size_t NA = (size_t)n * (size_t)A64;
  Stream st;
  Arg a_gt, a_hard, a_dc, a_lab, a_tgt, a_in, a_out, a_pre, a_max, a_arg;      // released before the stream, on every way out
  DevBuf tables, colmax, hardfirst, flags, dstats;
  if ((rc = st.ensure())) return rc;
  // the small tables, always the host's: im_info, the two offset tables
  std::vector<int> tab((size_t)n * 3 + 2 * ((size_t)n + 1), 0);
  std::memcpy(tab.data(), im_info, (size_t)n * 3 * sizeof(float));
  std::memcpy(tab.data() + (size_t)n * 3, gt_offsets, ((size_t)n + 1) * sizeof(int));
  if (dontcare && total_dc > 0) std::memcpy(tab.data() + (size_t)n * 4 + 1, dc_offsets, ((size_t)n + 1) * sizeof(int));
  if ((rc = tables.alloc(tab.size() * sizeof(int)))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(tables.get(), tab.data(), tables.bytes(), hipMemcpyHostToDevice, st));
  const float* d_info = tables.as<float>();
  const int* d_offs = tables.as<int>() + (size_t)n * 3;
  const int* d_dco = d_offs + n + 1;
  if ((rc = a_gt.in(gt_boxes, (size_t)total * 5 * sizeof(float), on_device, st)) || (rc = a_hard.in(gt_hard, (size_t)total * sizeof(int), on_device, st)) ||
      (rc = a_dc.in(total_dc > 0 ? dontcare : nullptr, (size_t)total_dc * 4 * sizeof(float), on_device, st)))
    return rc;
  if ((rc = a_lab.out(labels, NA * sizeof(float), on_device)) || (rc = a_tgt.out(bbox_targets, NA * 4 * sizeof(float), on_device)) ||
      (rc = a_in.out(inside_weights, NA * 4 * sizeof(float), on_device)) || (rc = a_out.out(outside_weights, NA * 4 * sizeof(float), on_device)) ||
      (rc = a_pre.out(labels_presample, NA * sizeof(float), on_device)) || (rc = a_max.out(max_overlap, NA * sizeof(double), on_device, true)) ||
      (rc = a_arg.out(argmax, NA * sizeof(int), on_device, true)))
    return rc;
  const size_t tg = (size_t)std::max<long long>(total, 1);
  if ((rc = colmax.alloc(tg * sizeof(unsigned long long))) || (rc = hardfirst.alloc(tg * sizeof(int))) || (rc = flags.alloc(NA)) ||
      (rc = dstats.alloc((size_t)n * 6 * sizeof(int))))
    return rc;
  CTPN_HIP_TRY(hipMemsetAsync(colmax.get(), 0, colmax.bytes(), st));
  CTPN_HIP_TRY(hipMemsetAsync(hardfirst.get(), 0x7f, hardfirst.bytes(), st));      // TG_NO_ANCHOR
  if ((rc = launch_anchor_targets(n, hf, wf, d_info, a_gt.as<float>(), d_offs, max_g, a_hard.as<int>(), a_dc.as<float>(), a_dc.dev ? d_dco : nullptr, cfg, seed,
                                  colmax.as<unsigned long long>(), hardfirst.as<int>(), flags.as<uint8_t>(), a_lab.as<float>(), a_tgt.as<float>(), a_in.as<float>(),
                                  a_out.as<float>(), dstats.as<int>(), a_pre.as<float>(), a_max.as<double>(), a_arg.as<int>(), st)))
    return rc;
  if ((rc = a_lab.fetch(st)) || (rc = a_tgt.fetch(st)) || (rc = a_in.fetch(st)) || (rc = a_out.fetch(st)) || (rc = a_pre.fetch(st)) || (rc = a_max.fetch(st)) ||
      (rc = a_arg.fetch(st)))
    return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(stats, dstats.get(), dstats.bytes(), hipMemcpyDeviceToHost, st));
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

int ctpn_rpn_loss(int device_id, int n, int hf, int wf, const float* heads, int ld, const float* labels, const float* bbox_targets,
                  const float* inside_weights, const float* outside_weights, int on_device, double* losses, int* counts, float* d_heads) {
  if (n <= 0 || hf <= 0 || wf <= 0) return fail(CTPN_ERR_ARG, "ctpn_rpn_loss: n, hf, wf >= 1");
  if (ld != 60 && ld != 64) return fail(CTPN_ERR_ARG, "ctpn_rpn_loss: ld is 60 or 64");
  if (!heads || !labels || !bbox_targets || !inside_weights || !outside_weights || !losses || !counts) return fail(CTPN_ERR_ARG, "ctpn_rpn_loss: null pointer");
  const long long A64 = (long long)hf * wf * TG_A;
  if (A64 > TG_MAX_ANCHORS) return fail(CTPN_ERR_ARG, "ctpn_rpn_loss: hf x wf x 10 beyond 2^24 anchors per image");
  if ((long long)n * A64 * 4 > (1LL << 32)) return fail(CTPN_ERR_ARG, "ctpn_rpn_loss: n x hf x wf x 40 beyond 2^32 values");
  if (on_device != 0 && on_device != 1) return fail(CTPN_ERR_ARG, "ctpn_rpn_loss: on_device is 0 or 1");
  int rc = targets_device(device_id, "ctpn_rpn_loss");
  if (rc) return rc;
  CTPN_HIP_TRY(hipSetDevice(device_id));
  const size_t NA = (size_t)n * (size_t)A64, HB = (size_t)n * hf * wf * ld * sizeof(float);
  Stream st;
  Arg a_h, a_lab, a_tgt, a_in, a_out, a_d;      // released before the stream, on every way out
  DevBuf res;
  if ((rc = st.ensure())) return rc;
  if ((rc = a_h.in(heads, HB, on_device, st)) || (rc = a_lab.in(labels, NA * sizeof(float), on_device, st)) ||
      (rc = a_tgt.in(bbox_targets, NA * 4 * sizeof(float), on_device, st)) || (rc = a_in.in(inside_weights, NA * 4 * sizeof(float), on_device, st)) ||
      (rc = a_out.in(outside_weights, NA * 4 * sizeof(float), on_device, st)) || (rc = a_d.out(d_heads, HB, on_device)))
    return rc;
  if ((rc = res.alloc((size_t)n * (3 * sizeof(double) + 2 * sizeof(int))))) return rc;
  double* d_loss = res.as<double>();
  int* d_cnt = reinterpret_cast<int*>(d_loss + (size_t)n * 3);
  if ((rc = launch_rpn_loss(n, hf, wf, a_h.as<float>(), ld, a_lab.as<float>(), a_tgt.as<float>(), a_in.as<float>(), a_out.as<float>(), d_loss, d_cnt,
                            a_d.as<float>(), st)))
    return rc;
  if ((rc = a_d.fetch(st))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(losses, d_loss, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  CTPN_HIP_TRY(hipMemcpyAsync(counts, d_cnt, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

}  // extern "C"
