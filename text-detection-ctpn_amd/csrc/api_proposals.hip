// C ABI of libctpn_hip.so, proposal unit: the proposal layer's orchestration (decode, sort, gather, NMS), its entry points, the stand-alone NMS seam.
#include "ctx.h"

namespace ctpn {

// Option nms_check behind a column-decomposed NMS launch on s (the proposal layer's here, the connector's in api_detect.hip): re-run the generic
// kernel on the same candidates and fail loudly if the keep lists differ. keep1 / cnt1: the column form's lists, on the host, rows of keep_stride;
// mw: the multi-workgroup form ran; what: the NMS's name in the error text. Synchronises s. The caller marks nms_mw_dirty on an error return.
int nms_check_generic(ctpn_ctx* c, const float* boxes, const float* scores, const int* counts, int stride, float thresh, int post_topn,
                      const int* keep1, int keep_stride, const int* cnt1, int n, bool mw, hipStream_t s, const char* what) {
  std::vector<int> k2((size_t)n * keep_stride), c2(n);
  DevBuf keep_buf, cnt_buf, spill_buf;
  int rc;
  if ((rc = keep_buf.alloc(k2.size() * sizeof(int))) || (rc = cnt_buf.alloc(c2.size() * sizeof(int))) || (rc = spill_buf.alloc((size_t)n * keep_stride * 4 * sizeof(float)))) return rc;
  int* keep2 = keep_buf.as<int>(); int* cnt2 = cnt_buf.as<int>();
  if ((rc = launch_nms(boxes, scores, counts, stride, thresh, post_topn, keep2, keep_stride, cnt2, nullptr, spill_buf.as<float>(), n, s))) return rc;
  CTPN_HIP_TRY(hipStreamSynchronize(s));
  CTPN_HIP_TRY(hipMemcpy(k2.data(), keep2, k2.size() * sizeof(int), hipMemcpyDeviceToHost));
  CTPN_HIP_TRY(hipMemcpy(c2.data(), cnt2, c2.size() * sizeof(int), hipMemcpyDeviceToHost));
  if (mw) {
    // the multi-workgroup form's sticky overflow words (a column with more candidates than the kernel's list)
    for (int i = 0; i < n; ++i) {
      unsigned ov = 0;
      CTPN_HIP_TRY(hipMemcpy(&ov, c->nms_mw_scratch + (size_t)i * NMS_MW_SCRATCH_BYTES + NMS_MW_OVERFLOW_OFF, 4, hipMemcpyDeviceToHost));
      if (ov) return fail(CTPN_ERR_STATE, "nms_check: a column held more candidates than the multi-workgroup NMS's list (1024): keep lists are incomplete");
    }
  }
  for (int i = 0; i < n; ++i) {
    bool same = cnt1[i] == c2[i];
    for (int k = 0; same && k < c2[i]; ++k) same = keep1[(size_t)i * keep_stride + k] == k2[(size_t)i * keep_stride + k];
    if (!same) return fail(CTPN_ERR_STATE, std::string("nms_check: column-decomposed ") + what + " differs from the generic kernel (boxes off the 16-px anchor grid?)");
  }
  return CTPN_OK;
}

// Every launch decision of the proposal layer, in one place: enqueue_proposals_impl computes this once and follows it. The conditions
// themselves stay with their kernels (sort_is_segmented / sort_seg_len, nms_columns_ok, nms_multi_wg_ok, nms_prefix_launches).
ProposalPlan proposal_plan(int nms_columns, int nms_prefix, bool has_mw_scratch, int n, int hf, int wf, int pre_nms_topn, int post_nms_topn,
                           float nms_thresh, const float* im_info) {
  ProposalPlan p{};
  const int per_img = hf * wf * 10;
  p.npad = next_pow2(per_img);
  const bool seg_sort = !(nms_columns == 2 || nms_columns == 0);      // options 0 / 2 pin the one-workgroup forms of sort and NMS
  p.sort_form = seg_sort && sort_is_segmented(n, per_img) ? PP_SORT_SEGMENTED : PP_SORT_ONE_WG;
  // (the segmented sort of small batches never reads behind the image's keys and pads its merged buffer itself)
  p.fill_keys = p.npad > per_img && p.sort_form != PP_SORT_SEGMENTED;
  p.seg_len = p.sort_form == PP_SORT_SEGMENTED ? sort_seg_len(per_img) : per_img;
  p.last_seg = p.sort_form == PP_SORT_SEGMENTED ? per_img - (per_img - 1) / p.seg_len * p.seg_len : per_img;
  p.merge_wgs = p.sort_form == PP_SORT_SEGMENTED ? sort_merge_workgroups(per_img) : 0;
  const bool cols = nms_columns && nms_columns_ok(wf, pre_nms_topn, nms_thresh);
  bool mw = cols && nms_multi_wg_ok(has_mw_scratch, nms_columns, n, hf);
  // boxes whose x was clipped onto the image's last pixel column (im_info narrower than the feature map: only ctpn_proposals_from_host can
  // say so) pile up in ONE column group, which may then exceed the multi-workgroup kernel's list: those calls keep the one-workgroup form
  for (int i = 0; im_info && i < n; ++i) mw = mw && im_info[3 * i + 1] >= (float)((wf - 1) * 16 + 1);
  p.nms_form = !cols ? PP_NMS_GENERIC : (mw ? PP_NMS_COLUMN_GROUPS : PP_NMS_ONE_WG);
  p.group_wgs = mw ? nms_column_group_workgroups(wf) : 0;
  p.prefix_launches = cols ? nms_prefix_launches(mw, nms_prefix_ranks(nms_prefix, post_nms_topn), pre_nms_topn, post_nms_topn) : 0;
  return p;
}

static int enqueue_proposals_impl(ctpn_ctx* c, const float* heads, int heads_are_probs, int n, int hf, int wf, const float* im_info,
                                  int pre_nms_topn, int post_nms_topn, float nms_thresh, float min_size, hipStream_t s, hipEvent_t ev_decoded,
                                  const int* valid_rows_dev) {
  if (!s) s = c->stream;
  if (!im_info) return fail(CTPN_ERR_ARG, "proposals: null pointer");
  if (pre_nms_topn <= 0 || pre_nms_topn > c->topn_max) return fail(CTPN_ERR_CAPACITY, "proposals: pre_nms_topn must be in 1..12000");
  if (post_nms_topn <= 0 || post_nms_topn > c->post_max) return fail(CTPN_ERR_CAPACITY, "proposals: post_nms_topn must be in 1.." + std::to_string(c->post_max));
  const int per_img = hf * wf * 10;
  const ProposalPlan plan = proposal_plan(c->nms_columns, c->nms_prefix, c->nms_mw_scratch != nullptr, n, hf, wf, pre_nms_topn, post_nms_topn, nms_thresh, im_info);
  const int npad = plan.npad;
  if (npad > c->npad_max) return fail(CTPN_ERR_CAPACITY, "proposals: feature map larger than the ctx was created for");
  if (n > 4) CTPN_HIP_TRY(hipMemcpyAsync(c->im_info_dev, im_info, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s));      // (<= 4: in decode_kernel's arguments)
  ProposalCfg pc{n, hf, wf, pre_nms_topn, post_nms_topn, nms_thresh, min_size};
  int rc;
  const bool mw = plan.nms_form == PP_NMS_COLUMN_GROUPS, seg_sort = plan.sort_form == PP_SORT_SEGMENTED;
  if (c->nms_mw_scratch && c->nms_mw_dirty) {
    // in stream order in front of everything that follows; both streams that ever use the block are drained by whoever set the flag
    CTPN_HIP_TRY(hipMemsetAsync(c->nms_mw_scratch, 0, (size_t)NMS_MW_CAP_BATCH * NMS_MW_SCRATCH_BYTES, s));
    c->nms_mw_dirty = false;
  }
  const double nanch = (double)n * per_img;
  {
    Timed t(c, CTPN_KIND_DECODE, nanch * (60.0 * 4 / 10 + 8 + 16), s);
    if ((rc = launch_decode(heads, 64, heads_are_probs, c->cls_in, c->bbox_in, c->im_info_dev, heads_are_probs ? nullptr : c->cls_prob,
                            heads_are_probs ? nullptr : c->bbox_pred, c->keys, c->boxes4, pc, npad, s, !plan.fill_keys, n <= 4 ? im_info : nullptr, valid_rows_dev))) return rc;
  }
  if (ev_decoded) CTPN_HIP_TRY(hipEventRecord(ev_decoded, s));
  {
    Timed t(c, CTPN_KIND_SORT, (double)n * npad * 16.0, s);
    int in_tmp = 0;
    if ((rc = launch_sort_keys(c->keys, c->keys_tmp, n, npad, per_img, s, seg_sort ? &in_tmp : nullptr))) return rc;
    const unsigned long long* sorted_keys = in_tmp ? c->keys_tmp : c->keys;
    if (in_tmp != (seg_sort ? 1 : 0)) return fail(CTPN_ERR_STATE, "proposals: the sort did not take the planned form");
    if ((rc = launch_gather_sorted(sorted_keys, c->boxes4, c->sorted_boxes, c->sorted_scores, c->sorted_anchor, c->valid_counts, n, npad, per_img, pre_nms_topn, s,
                                   mw ? c->nms_colid : nullptr, wf))) return rc;
  }
  if (c->debug_hog > 0 && c->nms_mw_scratch) {
    // values above 50000: the hog also keeps writing its 84 KB of LDS (usec = value - 50000); above 100000: it gathers random 16-byte pieces of the
    // largest activation buffer instead (usec = value - 100000, twice the workgroups): the NMS kernel's memory traffic for as long as asked
    const int hv = c->debug_hog;
    const int usec = hv > 100000 ? hv - 100000 : hv > 50000 ? hv - 50000 : hv, touch = hv > 100000 ? 4 : hv > 50000 ? 2 : 0;
    const void* src = nullptr; size_t src_bytes = 0;
    for (int i = 0; i < 14; ++i) if (c->fs[0].act_conv[i] && c->act_conv_bytes[i] > src_bytes) { src = c->fs[0].act_conv[i]; src_bytes = c->act_conv_bytes[i]; }
    if ((rc = launch_hog((unsigned*)(c->nms_colid), touch == 4 ? 2 * n : n, usec, touch, s, src, src_bytes))) return rc;       // (sink: never written; any device pointer)
  }
  {
    Timed t(c, CTPN_KIND_NMS, (double)n * pre_nms_topn * 24.0, s);
    if (plan.nms_form != PP_NMS_GENERIC) {
      // 16 waves per image (a 4-wave footprint that co-resides with the persistent convolutions took 1.9 ms instead of 0.66 ms and slowed
      // conv1_2 by 8 % through the shared SIMDs in round 2: removed)
      if ((rc = launch_nms_columns(c->sorted_boxes, c->sorted_scores, c->valid_counts, pre_nms_topn, nms_thresh, post_nms_topn, c->keep_idx,
                                   c->topn_max, c->keep_counts, c->rois, c->kept_spill, n, wf, s, c->sorted_anchor, c->roi_anchor, nullptr,
                                   mw ? c->nms_mw_scratch : nullptr, mw ? c->nms_colid : nullptr, nms_prefix_ranks(c->nms_prefix, post_nms_topn), c->debug_nms))) return rc;
      if (c->nms_check) {
        // option "nms_check" (debug; synchronises the stream): the column decomposition presumes boxes on the 16-px anchor grid (common.h)
        std::vector<int> k1((size_t)n * c->topn_max), c1(n);
        CTPN_HIP_TRY(hipStreamSynchronize(s));
        CTPN_HIP_TRY(hipMemcpy(k1.data(), c->keep_idx, k1.size() * sizeof(int), hipMemcpyDeviceToHost));
        CTPN_HIP_TRY(hipMemcpy(c1.data(), c->keep_counts, c1.size() * sizeof(int), hipMemcpyDeviceToHost));
        if ((rc = nms_check_generic(c, c->sorted_boxes, c->sorted_scores, c->valid_counts, pre_nms_topn, nms_thresh, post_nms_topn, k1.data(), c->topn_max,
                                    c1.data(), n, mw, s, "NMS"))) return rc;
      }
    } else if ((rc = launch_nms(c->sorted_boxes, c->sorted_scores, c->valid_counts, pre_nms_topn, nms_thresh, post_nms_topn, c->keep_idx,
                                c->topn_max, c->keep_counts, c->rois, c->kept_spill, n, s, c->sorted_anchor, c->roi_anchor))) return rc;
  }
  c->last_post = post_nms_topn; c->last_prop_n = n;
  c->last_plan = plan; c->last_hf = hf; c->last_wf = wf; c->last_pre = pre_nms_topn;
  if (!heads_are_probs) c->proposals_done = true;
  return CTPN_OK;
}
int enqueue_proposals(ctpn_ctx* c, const float* heads, int heads_are_probs, int n, int hf, int wf, const float* im_info,
                      int pre_nms_topn, int post_nms_topn, float nms_thresh, float min_size, hipStream_t s,
                      hipEvent_t ev_decoded, const int* valid_rows_dev) {
  const int rc = enqueue_proposals_impl(c, heads, heads_are_probs, n, hf, wf, im_info, pre_nms_topn, post_nms_topn, nms_thresh, min_size, s, ev_decoded, valid_rows_dev);
  if (rc != CTPN_OK) c->nms_mw_dirty = true;       // whatever failed, nobody vouches for the multi-workgroup NMS's scratch any more (common.h)
  return rc;
}

static int run_proposals(ctpn_ctx* c, const float* heads, int heads_are_probs, int n, int hf, int wf, const float* im_info,
                         int pre_nms_topn, int post_nms_topn, float nms_thresh, float min_size, float* rois_out, int* counts_out,
                         const int* valid_rows_dev = nullptr) {
  if (!rois_out || !counts_out) return fail(CTPN_ERR_ARG, "proposals: null pointer");
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));   // the asynchronous detect path shares the proposal buffers
  int rc = enqueue_proposals(c, heads, heads_are_probs, n, hf, wf, im_info, pre_nms_topn, post_nms_topn, nms_thresh, min_size, nullptr, nullptr, valid_rows_dev);
  if (rc) return rc;
  hipStream_t s = c->stream;
  CTPN_HIP_TRY(hipMemcpyAsync(counts_out, c->keep_counts, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
  CTPN_HIP_TRY(hipMemcpyAsync(rois_out, c->rois, (size_t)n * post_nms_topn * 5 * sizeof(float), hipMemcpyDeviceToHost, s));
  CTPN_HIP_TRY(hipStreamSynchronize(s));
  return CTPN_OK;
}

}  // namespace ctpn

// ---- standalone NMS (B1 seam) ----------------------------------------------------------------
namespace {
struct NmsCache {
  std::mutex mu;
  Stream stream;
  int cap = 0;      // boxes the blocks have room for
  DevBuf boxes, spill, keep, counts;      // float4, float4, int per box; counts: int [n in, n kept]
};
// one per device, for the life of the process: allocated once and deliberately never destroyed (at static-destruction time the HIP runtime may
// already be gone, and a release would call into it)
NmsCache* const g_nms = new NmsCache[16];
}  // namespace

extern "C" {

int ctpn_proposals(ctpn_ctx* c, const float* im_info, int pre_nms_topn, int post_nms_topn, float nms_thresh, float min_size,
                   float* rois_out, int* counts_out) {
  if (!c) return fail(CTPN_ERR_ARG, "null ctx");
  if (!c->forward_done) return fail(CTPN_ERR_STATE, "ctpn_proposals: no forward yet");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  // after a ragged forward: that forward's feature rows per image (its set's second half), which a uniform forward forgets
  const ctpn_ctx::FwdSet& f = *c->last;      // the most recent forward's set; the proposal layer runs on `stream`, behind that forward
  if (f.stream != c->stream) CTPN_HIP_TRY(hipStreamSynchronize(f.stream));
  const int* valid = f.fwd_ragged >= 0 ? c->ragged[f.fwd_ragged].dev.as<int>() + f.n : nullptr;
  return run_proposals(c, f.heads, 0, f.n, lvl(f.h, 4), lvl(f.w, 4), im_info, pre_nms_topn, post_nms_topn, nms_thresh, min_size,
                       rois_out, counts_out, valid);
}

int ctpn_proposals_from_host(ctpn_ctx* c, const float* cls_prob, const float* bbox_pred, int n, int hf, int wf, const float* im_info,
                             int pre_nms_topn, int post_nms_topn, float nms_thresh, float min_size, float* rois_out, int* counts_out) {
  if (!c || !cls_prob || !bbox_pred) return fail(CTPN_ERR_ARG, "null pointer");
  if (n <= 0 || n > c->max_batch || hf <= 0 || wf <= 0 || (size_t)n * hf * wf > c->m5_max)
    return fail(CTPN_ERR_CAPACITY, "ctpn_proposals_from_host: shape outside what the ctx was created for");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  const size_t m = (size_t)n * hf * wf;
  CTPN_HIP_TRY(hipMemcpyAsync(c->cls_in, cls_prob, m * 20 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  CTPN_HIP_TRY(hipMemcpyAsync(c->bbox_in, bbox_pred, m * 40 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  return run_proposals(c, nullptr, 1, n, hf, wf, im_info, pre_nms_topn, post_nms_topn, nms_thresh, min_size, rois_out, counts_out);
}

int ctpn_proposal_anchors(ctpn_ctx* c, int* anchors_out, int post_nms_topn) {
  if (!c || !anchors_out) return fail(CTPN_ERR_ARG, "null pointer");
  if (c->last_prop_n <= 0) return fail(CTPN_ERR_STATE, "ctpn_proposal_anchors: no ctpn_proposals / ctpn_proposals_from_host call yet");
  if (post_nms_topn != c->last_post) return fail(CTPN_ERR_ARG, "ctpn_proposal_anchors: post_nms_topn differs from the proposals call");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));
  CTPN_HIP_TRY(hipMemcpyAsync(anchors_out, c->roi_anchor, (size_t)c->last_prop_n * post_nms_topn * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream));
  return CTPN_OK;
}

int ctpn_nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim, float thresh, int device_id) {
  if (!keep_out || !num_out) return fail(CTPN_ERR_ARG, "ctpn_nms: null output");
  *num_out = 0;
  if (boxes_num == 0) return CTPN_OK;
  if (!boxes_host || boxes_num < 0 || boxes_dim < 4) return fail(CTPN_ERR_ARG, "ctpn_nms: boxes must be N x (>=4)");
  const int ndev = ctpn_device_count();
  if (ndev <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_nms: no HIP device visible (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev || device_id >= 16) return fail(CTPN_ERR_ARG, "ctpn_nms: device_id out of range");
  NmsCache& nc = g_nms[device_id];
  std::lock_guard<std::mutex> lk(nc.mu);
  CTPN_HIP_TRY(hipSetDevice(device_id));
  int rc;
  if ((rc = nc.stream.ensure())) return rc;
  if (nc.cap < boxes_num) {
    const size_t cap = boxes_num < 16384 ? 16384 : boxes_num;
    nc.cap = 0;
    if ((rc = nc.boxes.grow(cap * 4 * sizeof(float))) || (rc = nc.spill.grow(cap * 4 * sizeof(float))) || (rc = nc.keep.grow(cap * sizeof(int))) || (rc = nc.counts.grow(2 * sizeof(int)))) return rc;
    nc.cap = (int)cap;
  }
  float* boxes = nc.boxes.as<float>(); int* counts = nc.counts.as<int>();
  std::vector<float> b4((size_t)boxes_num * 4);
  for (int i = 0; i < boxes_num; ++i) std::memcpy(&b4[(size_t)i * 4], boxes_host + (size_t)i * boxes_dim, 4 * sizeof(float));
  CTPN_HIP_TRY(hipMemcpyAsync(boxes, b4.data(), b4.size() * sizeof(float), hipMemcpyHostToDevice, nc.stream));
  CTPN_HIP_TRY(hipMemcpyAsync(counts, &boxes_num, sizeof(int), hipMemcpyHostToDevice, nc.stream));
  if ((rc = launch_nms(boxes, nullptr, counts, boxes_num, thresh, boxes_num, nc.keep.as<int>(), boxes_num, counts + 1, nullptr, nc.spill.as<float>(), 1, nc.stream))) return rc;
  int nk = 0;
  CTPN_HIP_TRY(hipMemcpyAsync(&nk, counts + 1, sizeof(int), hipMemcpyDeviceToHost, nc.stream));
  CTPN_HIP_TRY(hipStreamSynchronize(nc.stream));
  if (nk < 0 || nk > boxes_num) return fail(CTPN_ERR_HIP, "ctpn_nms: device returned an impossible keep count");
  CTPN_HIP_TRY(hipMemcpy(keep_out, nc.keep.get(), (size_t)nk * sizeof(int), hipMemcpyDeviceToHost));
  *num_out = nk;
  return CTPN_OK;
}

}  // extern "C"
