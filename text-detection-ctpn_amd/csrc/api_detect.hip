// C ABI of libctpn_hip.so, detect unit: forward + proposal layer + connector front end as one asynchronous submit / collect pair, the
// synchronous ctpn_detect on top of it, the host connector's entry point and the test hooks of the device connector and of the whole text-line tail.
#include "ctx.h"

namespace ctpn {

// The text-line tail of a batch whose rois, counts and im_info are on the device (c->rois, c->keep_counts, c->im_info_dev; sl.im_info holds the
// host copy of im_info): TextDetector.detect's front end -- score > TEXT_PROPOSALS_MIN_SCORE prefix, boxes / scale, NMS TEXT_PROPOSALS_NMS_THRESH
// (detectors.py:21-30) -- and, with option connect_device, the connector, in stream order on p; thresholds from the ctx's parameters
// (ctpn_set_param), rows per image = RPN_POST_NMS_TOP_N. detect_submit_body and the test hook ctpn_debug_text_lines both call it.
// nms_form (nullable): 0 = the generic NMS kernel ran, 1 = the one-workgroup column form, 2 = the multi-workgroup column form.
static int enqueue_text_lines(ctpn_ctx* c, ctpn_ctx::Slot& sl, int n, int w, hipStream_t p, int* nms_form = nullptr) {
  const int post = c->rpn_post;
  const float tl_thresh = c->conn.nms_thresh;
  TextLinePlan plan{};
  int rc;
  {
    Timed t(c, CTPN_KIND_NMS, (double)n * post * 24.0, p);
    if ((rc = launch_lines_prep(c->rois, c->keep_counts, c->im_info_dev, post, c->conn.min_score, c->tl_boxes, c->tl_scores, c->tl_counts, n, p))) return rc;
    float max_scale = 0.f;
    const float* info = sl.im_info.as<float>();
    for (int i = 0; i < n; ++i) max_scale = info[3 * i + 2] > max_scale ? info[3 * i + 2] : max_scale;
    const int wf = lvl(w, 4);
    plan = text_line_plan(c->nms_columns, c->connect_device, c->nms_mw_scratch != nullptr, n, wf, post, tl_thresh, max_scale);
    if (plan.nms_form != TL_NMS_GENERIC) {
      const bool mw = plan.nms_form == TL_NMS_COLUMN_GROUPS;
      if (nms_form) *nms_form = mw ? 2 : 1;
      if ((rc = launch_nms_columns(c->tl_boxes, c->tl_scores, c->tl_counts, post, tl_thresh, post, c->tl_keep, post, c->tl_keep_counts, nullptr,
                                   c->tl_spill, n, wf, p, nullptr, nullptr, c->im_info_dev, mw ? c->nms_mw_scratch : nullptr))) return rc;
    } else {
      if (nms_form) *nms_form = 0;
      if ((rc = launch_nms(c->tl_boxes, c->tl_scores, c->tl_counts, post, tl_thresh, post, c->tl_keep, post, c->tl_keep_counts, nullptr,
                           c->tl_spill, n, p))) return rc;
    }
  }
  if (plan.conn_form != TL_CONN_HOST) {
    // graph build, chains, line fit and filter_boxes on the device too, for both DETECT_MODEs (the mode is chosen at collect); above 1024 rows per
    // image the large form (its anchor columns: the map's, the last one taking what lies beyond 256)
    if (plan.conn_form == TL_CONN_BUCKETS && !c->conn_work) return fail(CTPN_ERR_STATE, "text_lines: no state block for the large connector");
    const int wf = lvl(w, 4);
    if ((rc = launch_connect(c->tl_boxes, c->tl_scores, c->tl_keep, c->tl_keep_counts, post, c->im_info_dev, c->conn_recs, c->conn_counts,
                             c->conn_scratch, c->conn_cap, n, c->conn, p, c->conn_work, wf > 256 ? 256 : wf))) return rc;
    CTPN_HIP_TRY(hipMemcpyAsync(sl.crecs.as<double>(), c->conn_recs, (size_t)n * 2 * c->conn_cap * 9 * sizeof(double), hipMemcpyDeviceToHost, p));
    CTPN_HIP_TRY(hipMemcpyAsync(sl.ccnt.as<int>(), c->conn_counts, (size_t)n * 3 * sizeof(int), hipMemcpyDeviceToHost, p));
  }
  return CTPN_OK;
}

// The forward set a submit to `slot` runs on (ctx.h, FwdSet). Nothing else in flight: set 0, the synchronous callers' set. The other slot in flight:
// the set that batch does NOT use, so that the two forwards run on two streams and write two sets of buffers -- if this ctx can have a second set
// (ensure_set1: not with keep_acts, not under per-stage profiling, not without the memory) with room for what this forward stores; else set 0 again,
// behind the batch in flight on the one stream, the order a ctx with one set always had. beside: the two forwards are on different sets.
// Correctness needs no more cross-batch order than that: a set is reused by the batch two submits on, whose slot the host has collected (ev_done)
// first. The gate forward_impl puts between the two sets' conv stacks is for speed alone (api_ctx.hip, two_forwards_mode).
static ctpn_ctx::FwdSet& pick_set(ctpn_ctx* c, int slot, int n, int h, int w, const int* heights, bool& beside) {
  const ctpn_ctx::Slot& other = c->slot[slot ^ 1];
  beside = false;
  if (!other.busy) return c->fs[0];
  if (other.set == 1) { beside = true; return c->fs[0]; }
  if (!ensure_set1(c, !forward_fuses_conv1(c, 0, n, h, w, heights))) return c->fs[0];
  beside = true;
  return c->fs[1];
}

// lone: a synchronous ctpn_detect with nothing else in flight on this ctx -- the proposal layer and the connector front end then follow the
// forward on ITS stream instead of hopping to the proposal stream (an event record + a cross-queue wait: ~12 us of a lone image's millisecond;
// the second stream exists to run the tail under the NEXT batch's convolutions, and there is no next batch here)
// heights (nullable): a ragged batch in a canvas of height h (ctpn_detect_submit_ragged)
static int detect_submit_body(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, const float* scales, int slot, bool lone,
                              const int* heights) {
  if (!c) return fail(CTPN_ERR_ARG, "ctpn_detect_submit: null ctx");
  if (slot < 0 || slot > 1) return fail(CTPN_ERR_ARG, "ctpn_detect_submit: slot must be 0 or 1");
  ctpn_ctx::Slot& sl = c->slot[slot];
  if (sl.busy) return fail(CTPN_ERR_STATE, "ctpn_detect_submit: slot still holds an uncollected batch");
  bool beside = false;
  ctpn_ctx::FwdSet& f = pick_set(c, slot, n, h, w, heights, beside);
  int rc = forward_impl(c, f, images, 0, images_on_device, n, h, w, c->tail_overlap != 0, heights, slot, beside);
  if (rc) {
    // a forward that failed midway may have consumed the cross-stream hand-over state (tail_pending is cleared when the wait is ENQUEUED,
    // the events are recorded later): drain both streams so that a retry starts from a quiet ctx, keeping the first error text
    const std::string first = ctpn_last_error();
    (void)sync_forwards(c); (void)hipStreamSynchronize(c->stream_p);
    for (auto& g : c->fs) { g.tail_pending = false; g.ev_decoded = nullptr; g.dec_slot = -1; }
    c->ev_last_done = nullptr;
    return fail(rc, first);
  }
  // im_info row i = [the image's own height, w, scale]: what the proposal layer clips to, and lines_prep, the connector's NMS and connect_kernel read
  sl.hts.assign(n, h);
  if (heights) sl.hts.assign(heights, heights + n);
  float* info = sl.im_info.as<float>();
  for (int i = 0; i < n; ++i) { info[3 * i] = (float)sl.hts[i]; info[3 * i + 1] = (float)w; info[3 * i + 2] = scales ? scales[i] : 1.0f; }
  hipStream_t p = lone ? f.stream : c->stream_p;
  if (!lone) {
    CTPN_HIP_TRY(hipEventRecord(sl.ev_heads, f.stream));
    CTPN_HIP_TRY(hipStreamWaitEvent(p, sl.ev_heads, 0));
  }
  // cfg.TEST.RPN_* (reference lib/fast_rcnn/config.py:175-183): the ctx's parameters, those defaults unless ctpn_set_param changed them
  rc = enqueue_proposals(c, f.heads, 0, n, lvl(h, 4), lvl(w, 4), info, c->rpn_pre, c->rpn_post, c->rpn_nms_thresh, c->rpn_min_size, p, sl.ev_decoded,
                         f.fwd_ragged >= 0 ? c->ragged[f.fwd_ragged].dev.as<int>() + n : nullptr);
  if (rc) return rc;
  f.ev_decoded = sl.ev_decoded; f.dec_slot = slot;      // the reader of this set's `heads` (forward_impl: wait_decoded)
  if ((rc = enqueue_text_lines(c, sl, n, w, p))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(sl.pack.get(), c->out_pack, c->pack_bytes, hipMemcpyDeviceToHost, p));      // tl_* (host connector), rois, counts: one copy
  CTPN_HIP_TRY(hipEventRecord(sl.ev_done, p));
  c->ev_last_done = sl.ev_done;
  sl.n = n; sl.h = h; sl.w = w; sl.busy = true; sl.set = (int)(&f - c->fs);
  return CTPN_OK;
}
static int detect_submit_impl(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, const float* scales, int slot, bool lone,
                              const int* heights = nullptr) {
  const int rc = detect_submit_body(c, images, images_on_device, n, h, w, scales, slot, lone, heights);
  if (rc != CTPN_OK && c) c->nms_mw_dirty = true;        // an error anywhere in a submit (the connector NMS's launch included): see common.h, NMS_MW_OVERFLOW_OFF
  return rc;
}

// the lines of a batch whose tail has finished, from what it left in the slot's page-locked buffers: the device connector's records (option
// connect_device), or connect_lines on the host workers over the connector NMS's survivors. ctpn_detect_collect and ctpn_debug_text_lines.
// sl.hts: the images' heights (one value unless the batch was ragged).
static int lines_of_slot(ctpn_ctx* c, ctpn_ctx::Slot& sl, int n, int w, int mode, double* recs_out, int line_capacity, int* line_counts) {
  const int post = c->rpn_post;
  const ConnectorCfg cfg = c->conn;      // the workers' copy
  if (c->connect_device) {
    for (int i = 0; i < n; ++i) {
      const int* ccnt = sl.ccnt.as<int>();
      if (ccnt[3 * i + 2] != 0) return fail(CTPN_ERR_ARG, "text_lines: proposal x1 outside the image (reference raises IndexError)");
      const int cnt = ccnt[3 * i + (mode == CTPN_MODE_O ? 1 : 0)];
      line_counts[i] = cnt;
      if (cnt > line_capacity || cnt > c->conn_cap) return fail(CTPN_ERR_CAPACITY, "ctpn_detect: more lines than line_capacity");
      if (cnt) std::memcpy(recs_out + (size_t)i * line_capacity * 9, sl.crecs.as<double>() + ((size_t)i * 2 + (mode == CTPN_MODE_O ? 1 : 0)) * c->conn_cap * 9, (size_t)cnt * 9 * sizeof(double));
    }
    return CTPN_OK;
  }
  std::vector<int> status(n, 0);
  std::vector<std::string> errs(n);
  auto work = [&](int i) {
    const int nk = sl.kcnt[i];
    std::vector<float> kb((size_t)nk * 4), ks(nk);
    for (int j = 0; j < nk; ++j) {
      const int src = sl.keep[(size_t)i * post + j];
      std::memcpy(&kb[4 * j], &sl.tlb[((size_t)i * post + src) * 4], 4 * sizeof(float));
      ks[j] = sl.tls[(size_t)i * post + src];
    }
    std::vector<double> recs;
    int st = connect_lines(kb.data(), ks.data(), nk, sl.hts[i], w, mode, cfg, recs);
    if (st) { status[i] = st; errs[i] = ctpn_last_error(); return; }
    const int cnt = (int)(recs.size() / 9);
    line_counts[i] = cnt;
    if (cnt > line_capacity) { status[i] = CTPN_ERR_CAPACITY; errs[i] = "ctpn_detect: more lines than line_capacity"; return; }
    if (cnt) std::memcpy(recs_out + (size_t)i * line_capacity * 9, recs.data(), recs.size() * sizeof(double));
  };
  c->pool->run(n, work);      // persistent workers of the ctx (ctpn_host_thread_budget), one image per task
  for (int i = 0; i < n; ++i) if (status[i]) return fail(status[i], errs[i]);
  return CTPN_OK;
}

// The tail of ctpn_detect_submit + ctpn_detect_collect on caller-supplied rois: enqueue_text_lines and lines_of_slot, the functions those two
// call, on the proposal stream and slot 0's page-locked buffers. Test hook (tests/test_gpu_text_line_tail.py).
static int debug_text_lines_body(ctpn_ctx* c, const float* rois, const int* roi_counts, int n, int im_h, int im_w, const float* scales, int mode,
                                 double* recs_out, int line_capacity, int* line_counts, int* keep_out, int* keep_counts) {
  if (!rois || !roi_counts || !recs_out || !line_counts) return fail(CTPN_ERR_ARG, "ctpn_debug_text_lines: null pointer");
  if (keep_out && !keep_counts) return fail(CTPN_ERR_ARG, "ctpn_debug_text_lines: keep_out without keep_counts");
  if (mode != CTPN_MODE_H && mode != CTPN_MODE_O) return fail(CTPN_ERR_ARG, "ctpn_debug_text_lines: mode must be H(0) or O(1)");
  if (n <= 0 || n > c->max_batch) return fail(CTPN_ERR_CAPACITY, "ctpn_debug_text_lines: 1 <= n <= max_batch images");
  if (im_h < 1 || im_w < 16 || line_capacity < 0) return fail(CTPN_ERR_ARG, "ctpn_debug_text_lines: im_h >= 1, im_w >= 16, line_capacity >= 0 required");
  const int post = c->rpn_post, post_max = c->post_max;      // rows per image on the device / in the caller's arrays
  for (int i = 0; i < n; ++i)
    if (roi_counts[i] < 0 || roi_counts[i] > post) return fail(CTPN_ERR_ARG, "ctpn_debug_text_lines: 0 <= roi_counts[i] <= RPN_POST_NMS_TOP_N (" + std::to_string(post) + ") rows of [score,x1,y1,x2,y2]");
  if (c->slot[0].busy || c->slot[1].busy) return fail(CTPN_ERR_STATE, "ctpn_debug_text_lines: a submitted batch has not been collected");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  CTPN_HIP_TRY(sync_forwards(c));      // the proposal entry points use these buffers on the forward's stream
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));
  ctpn_ctx::Slot& sl = c->slot[0];
  hipStream_t p = c->stream_p;
  sl.hts.assign(n, im_h);
  float* info = sl.im_info.as<float>();
  for (int i = 0; i < n; ++i) { info[3 * i] = (float)im_h; info[3 * i + 1] = (float)im_w; info[3 * i + 2] = scales ? scales[i] : 1.0f; }
  if (c->nms_mw_scratch && c->nms_mw_dirty) {       // as enqueue_proposals does in front of a submit's tail
    CTPN_HIP_TRY(hipMemsetAsync(c->nms_mw_scratch, 0, (size_t)NMS_MW_CAP_BATCH * NMS_MW_SCRATCH_BYTES, p));
    c->nms_mw_dirty = false;
  }
  CTPN_HIP_TRY(hipMemcpyAsync(c->im_info_dev, info, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, p));
  if (post == post_max) CTPN_HIP_TRY(hipMemcpyAsync(c->rois, rois, (size_t)n * post * 5 * sizeof(float), hipMemcpyHostToDevice, p));
  else CTPN_HIP_TRY(hipMemcpy2DAsync(c->rois, (size_t)post * 5 * sizeof(float), rois, (size_t)post_max * 5 * sizeof(float), (size_t)post * 5 * sizeof(float), n, hipMemcpyHostToDevice, p));
  CTPN_HIP_TRY(hipMemcpyAsync(c->keep_counts, roi_counts, (size_t)n * sizeof(int), hipMemcpyHostToDevice, p));
  int form = 0, rc;
  if ((rc = enqueue_text_lines(c, sl, n, im_w, p, &form))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(sl.pack.get(), c->out_pack, c->pack_bytes, hipMemcpyDeviceToHost, p));
  CTPN_HIP_TRY(hipStreamSynchronize(p));
  for (int i = 0; i < n; ++i)
    if (sl.kcnt[i] < 0 || sl.kcnt[i] > post) return fail(CTPN_ERR_HIP, "ctpn_debug_text_lines: device returned an impossible keep count");
  if (keep_counts) std::memcpy(keep_counts, sl.kcnt, (size_t)n * sizeof(int));
  if (keep_out) for (int i = 0; i < n; ++i) std::memcpy(keep_out + (size_t)i * post_max, sl.keep + (size_t)i * post, (size_t)post * sizeof(int));
  // option nms_check, as in the proposal layer: the generic kernel on the same prepared boxes must keep the same rows
  if (c->nms_check && form != 0 &&
      (rc = nms_check_generic(c, c->tl_boxes, c->tl_scores, c->tl_counts, post, c->conn.nms_thresh, post, sl.keep, post, sl.kcnt, n, form == 2, p, "connector NMS"))) return rc;
  return lines_of_slot(c, sl, n, im_w, mode, recs_out, line_capacity, line_counts);
}

}  // namespace ctpn

extern "C" {

int ctpn_text_lines_cfg(const float* boxes, const float* scores, int r, int im_h, int im_w, int mode, int device_id, const double* cfg8,
                        double* recs_out, int capacity, int* count_out) {
  if (!count_out) return fail(CTPN_ERR_ARG, "ctpn_text_lines: count_out is null");
  *count_out = 0;
  if (r > 0 && (!boxes || !scores)) return fail(CTPN_ERR_ARG, "ctpn_text_lines: null input");
  ConnectorCfg cfg = default_connector_cfg();
  int rc = connector_cfg_from8(cfg8, cfg);
  if (rc) return rc;
  std::vector<double> recs;
  rc = text_lines_host(boxes, scores, r, im_h, im_w, mode, device_id, cfg, recs);
  if (rc) return rc;
  const int cnt = (int)(recs.size() / 9);
  *count_out = cnt;
  if (cnt > capacity) return fail(CTPN_ERR_CAPACITY, "ctpn_text_lines: more lines than capacity");
  if (cnt && !recs_out) return fail(CTPN_ERR_ARG, "ctpn_text_lines: recs_out is null");
  if (cnt) std::memcpy(recs_out, recs.data(), recs.size() * sizeof(double));
  return CTPN_OK;
}

int ctpn_text_lines(const float* boxes, const float* scores, int r, int im_h, int im_w, int mode, int device_id, double* recs_out,
                    int capacity, int* count_out) {
  return ctpn_text_lines_cfg(boxes, scores, r, im_h, im_w, mode, device_id, nullptr, recs_out, capacity, count_out);
}

int ctpn_detect_submit(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, const float* scales, int slot) {
  return detect_submit_impl(c, images, images_on_device, n, h, w, scales, slot, false);
}

int ctpn_detect_collect(ctpn_ctx* c, int slot, int mode, double* recs_out, int line_capacity, int* line_counts, float* rois_out,
                        int* roi_counts) {
  if (!c || !recs_out || !line_counts) return fail(CTPN_ERR_ARG, "ctpn_detect_collect: null pointer");
  if (slot < 0 || slot > 1) return fail(CTPN_ERR_ARG, "ctpn_detect_collect: slot must be 0 or 1");
  if (mode != CTPN_MODE_H && mode != CTPN_MODE_O) return fail(CTPN_ERR_ARG, "ctpn_detect_collect: mode must be H(0) or O(1)");
  ctpn_ctx::Slot& sl = c->slot[slot];
  if (!sl.busy) return fail(CTPN_ERR_STATE, "ctpn_detect_collect: nothing was submitted to this slot");
  CTPN_HIP_TRY(hipEventSynchronize(sl.ev_done));
  sl.busy = false;
  const int n = sl.n, w = sl.w, post = c->rpn_post, post_max = c->post_max;
  // rois_out keeps post_max rows per image (the ctx's proposal capacity) whatever RPN_POST_NMS_TOP_N is; the slot holds them packed
  if (rois_out) for (int i = 0; i < n; ++i) std::memcpy(rois_out + (size_t)i * post_max * 5, sl.rois + (size_t)i * post * 5, (size_t)post * 5 * sizeof(float));
  if (roi_counts) std::memcpy(roi_counts, sl.rcnt, (size_t)n * sizeof(int));
  return lines_of_slot(c, sl, n, w, mode, recs_out, line_capacity, line_counts);
}

int ctpn_detect(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, const float* scales, int mode,
                double* recs_out, int line_capacity, int* line_counts, float* rois_out, int* roi_counts) {
  if (!c || !recs_out || !line_counts) return fail(CTPN_ERR_ARG, "ctpn_detect: null pointer");
  if (mode != CTPN_MODE_H && mode != CTPN_MODE_O) return fail(CTPN_ERR_ARG, "ctpn_detect: mode must be H(0) or O(1)");
  int slot = c->slot[0].busy ? 1 : 0;
  const bool lone = !c->slot[0].busy && !c->slot[1].busy && c->tail_overlap == 0;
  int rc = detect_submit_impl(c, images, images_on_device, n, h, w, scales, slot, lone);
  if (rc) return rc;
  return ctpn_detect_collect(c, slot, mode, recs_out, line_capacity, line_counts, rois_out, roi_counts);
}

int ctpn_detect_submit_ragged(ctpn_ctx* c, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights, const float* scales, int slot) {
  if (!c || !heights) return fail(CTPN_ERR_ARG, "ctpn_detect_submit_ragged: null pointer");
  return detect_submit_impl(c, canvas, canvas_on_device, n, hc, w, scales, slot, false, heights);
}

int ctpn_detect_ragged(ctpn_ctx* c, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights, const float* scales, int mode,
                       double* recs_out, int line_capacity, int* line_counts, float* rois_out, int* roi_counts) {
  if (!c || !heights || !recs_out || !line_counts) return fail(CTPN_ERR_ARG, "ctpn_detect_ragged: null pointer");
  if (mode != CTPN_MODE_H && mode != CTPN_MODE_O) return fail(CTPN_ERR_ARG, "ctpn_detect_ragged: mode must be H(0) or O(1)");
  int slot = c->slot[0].busy ? 1 : 0;
  const bool lone = !c->slot[0].busy && !c->slot[1].busy && c->tail_overlap == 0;
  int rc = detect_submit_impl(c, canvas, canvas_on_device, n, hc, w, scales, slot, lone, heights);
  if (rc) return rc;
  return ctpn_detect_collect(c, slot, mode, recs_out, line_capacity, line_counts, rois_out, roi_counts);
}

// TextDetector.detect entirely on the device for one image's rois (the asynchronous detect path with option connect_device = 1):
// lines_prep_kernel (score > 0.7 prefix, boxes / scale) -> nms_kernel (0.2) -> connect_kernel. Test hook: lets the parity
// tests feed the reference-generated rois straight into connect_kernel.
int ctpn_debug_connect(int device_id, const float* rois, int r, int im_h, int im_w, float scale, int mode, double* recs_out,
                       int capacity, int* count_out) {
  if (!count_out) return fail(CTPN_ERR_ARG, "ctpn_debug_connect: count_out is null");
  *count_out = 0;
  if (mode != CTPN_MODE_H && mode != CTPN_MODE_O) return fail(CTPN_ERR_ARG, "ctpn_debug_connect: mode must be H(0) or O(1)");
  if (r < 0 || r > 1000 || (r > 0 && !rois)) return fail(CTPN_ERR_ARG, "ctpn_debug_connect: 0 <= r <= 1000 rows of [score,x1,y1,x2,y2]");
  const int ndev = ctpn_device_count();
  if (ndev <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_debug_connect: no HIP device visible (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(CTPN_ERR_ARG, "ctpn_debug_connect: device_id out of range");
  CTPN_HIP_TRY(hipSetDevice(device_id));
  const int post = 1000;
  const ConnectorCfg cfg = default_connector_cfg();       // a stateless hook: the defaults
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t o_rois = take((size_t)(post + 1) * 5 * 4), o_cnt = take(16), o_info = take(16), o_tlb = take((size_t)post * 16), o_tls = take((size_t)post * 4),
               o_tlc = take(16), o_keep = take((size_t)post * 4), o_kc = take(16), o_spill = take((size_t)post * 16),
               o_recs = take((size_t)2 * CONN_CAP * 9 * 8), o_cc = take(16), o_scr = take((size_t)1024 * 20 * 8);
  Stream st;
  DevBuf block;      // released before the stream, on every way out
  int rc;
  if ((rc = block.alloc(off)) || (rc = st.ensure())) return rc;
  char* buf = block.as<char>();
  CTPN_HIP_TRY(hipMemsetAsync(buf, 0, off, st));
  const float info[3] = {(float)im_h, (float)im_w, scale};
  if (r) CTPN_HIP_TRY(hipMemcpyAsync(buf + o_rois, rois, (size_t)r * 5 * 4, hipMemcpyHostToDevice, st));
  CTPN_HIP_TRY(hipMemcpyAsync(buf + o_cnt, &r, 4, hipMemcpyHostToDevice, st));
  CTPN_HIP_TRY(hipMemcpyAsync(buf + o_info, info, 12, hipMemcpyHostToDevice, st));
  if ((rc = launch_lines_prep((const float*)(buf + o_rois), (const int*)(buf + o_cnt), (const float*)(buf + o_info), post, cfg.min_score, (float*)(buf + o_tlb),
                              (float*)(buf + o_tls), (int*)(buf + o_tlc), 1, st))) return rc;
  if ((rc = launch_nms((const float*)(buf + o_tlb), (const float*)(buf + o_tls), (const int*)(buf + o_tlc), post, cfg.nms_thresh, post, (int*)(buf + o_keep), post,
                       (int*)(buf + o_kc), nullptr, (float*)(buf + o_spill), 1, st))) return rc;
  if ((rc = launch_connect((const float*)(buf + o_tlb), (const float*)(buf + o_tls), (const int*)(buf + o_keep), (const int*)(buf + o_kc), post,
                           (const float*)(buf + o_info), (double*)(buf + o_recs), (int*)(buf + o_cc), (double*)(buf + o_scr), CONN_CAP, 1, cfg, st))) return rc;
  int cc[3] = {0, 0, 0};
  CTPN_HIP_TRY(hipMemcpyAsync(cc, buf + o_cc, 12, hipMemcpyDeviceToHost, st));
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  if (cc[2] != 0) return fail(CTPN_ERR_ARG, "text_lines: proposal x1 outside the image (reference raises IndexError)");
  const int cnt = cc[mode == CTPN_MODE_O ? 1 : 0];
  *count_out = cnt;
  if (cnt > capacity || cnt > CONN_CAP) return fail(CTPN_ERR_CAPACITY, "ctpn_debug_connect: more lines than capacity");
  if (cnt && !recs_out) return fail(CTPN_ERR_ARG, "ctpn_debug_connect: recs_out is null");
  if (cnt) CTPN_HIP_TRY(hipMemcpy(recs_out, buf + o_recs + (size_t)(mode == CTPN_MODE_O ? 1 : 0) * CONN_CAP * 9 * 8, (size_t)cnt * 9 * 8, hipMemcpyDeviceToHost));
  return CTPN_OK;
}

int ctpn_debug_text_lines(ctpn_ctx* c, const float* rois, const int* roi_counts, int n, int im_h, int im_w, const float* scales, int mode,
                          double* recs_out, int line_capacity, int* line_counts, int* keep_out, int* keep_counts) {
  if (!c) return fail(CTPN_ERR_ARG, "ctpn_debug_text_lines: null ctx");
  const int rc = debug_text_lines_body(c, rois, roi_counts, n, im_h, im_w, scales, mode, recs_out, line_capacity, line_counts, keep_out, keep_counts);
  if (rc != CTPN_OK) {
    // as detect_submit_impl: nobody vouches for the multi-workgroup NMS's scratch after an error; leave the proposal stream quiet
    const std::string first = ctpn_last_error();
    (void)hipStreamSynchronize(c->stream_p);
    c->nms_mw_dirty = true;
    return fail(rc, first);
  }
  return rc;
}

}  // extern "C"
