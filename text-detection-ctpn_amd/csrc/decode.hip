// Proposal layer on device: softmax + anchor decode + clip + min-size filter -> key sort -> greedy NMS.
//
// Replaces, per image and batched over images (the reference is batch-1 Python on a TF CPU thread):
//   spatial_softmax                       reference lib/networks/network.py:332-337
//   generate_anchors                      lib/rpn_msr/generate_anchors.py:3-32   (py3 table)
//   proposal_layer steps 1-8              lib/rpn_msr/proposal_layer_tf.py:65-155
//   bbox_transform_inv / clip_boxes       lib/fast_rcnn/bbox_transform.py:36-80  (dx, dw ignored, :50,52)
//   _filter_boxes                         lib/rpn_msr/proposal_layer_tf.py:160-165
//   nms -> gpu_nms -> _nms / nms_kernel   lib/fast_rcnn/nms_wrapper.py:11-20, lib/utils/nms_kernel.cu:24-143
//
// All box arithmetic is fp32 in numpy's operation order with FMA contraction disabled, so decoded boxes
// match the reference except for the last ulp of exp(); the NMS predicate is evaluated exactly as the CUDA
// kernel does (IEEE fp32 divide, `IoU > thr`), so for identical sorted boxes the keep list is bit-identical.
// Tie order of the sort is fixed: descending score, equal scores by ascending anchor index (h, w, a).
// This unit: softmax, decode, clip, filter, keys. The sort and the gather: sort_keys.hip; the NMS kernels: nms.hip; the text-line tail: connect.hip.
#include "proposal_dev.h"      // (brings common.h)

#pragma clang fp contract(off)

namespace ctpn {

// y1, y2 of the 10 base anchors (x1 = 0, x2 = 15), python-3 division + int32 truncation
__constant__ int c_anchor_y1[10] = {2, 0, -4, -9, -16, -26, -41, -62, -91, -134};
__constant__ int c_anchor_y2[10] = {13, 15, 19, 24, 31, 41, 56, 77, 106, 149};

struct ImInfoSmall { float v[12]; };      // im_info rows [h, w, scale] of up to four images, by value

// ---------------------------------------------------------------------------------------------
// decode: one thread per anchor (n, y, x, a)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void decode_kernel(const float* __restrict__ heads, int head_ld,
                                                     const float* __restrict__ cls_prob_in, const float* __restrict__ bbox_in,
                                                     const float* __restrict__ im_info, float* __restrict__ cls_prob_out,
                                                     float* __restrict__ bbox_out, unsigned long long* __restrict__ keys,
                                                     float* __restrict__ boxes4, int n_img, int hf, int wf, float min_size,
                                                     int npad, ImInfoSmall small, float* __restrict__ im_info_pub,
                                                     const int* __restrict__ valid_rows) {
  const int per_img = hf * wf * 10;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  // small batches: im_info arrives in the kernel arguments (no 12-byte host-to-device copy in front of this kernel: ~5 us of a lone image's
  // tail) and is published here for the kernels behind this one (lines_prep, the connector's NMS, connect)
  if (im_info_pub && gid < 3 * n_img) {
    const int k = (int)gid;
    float v = small.v[0];
#pragma unroll
    for (int q = 1; q < 12; ++q) v = k == q ? small.v[q] : v;
    im_info_pub[k] = v;
  }
  if (gid >= (long long)n_img * per_img) return;
  const int img = (int)(gid / per_img);
  const int idx = (int)(gid - (long long)img * per_img);  // (y, x, a) row-major
  const int a = idx % 10;
  const int cell = idx / 10;
  const int x = cell % wf, y = cell / wf;
  const long long m = (long long)img * hf * wf + cell;

  float dy, dh, score;
  if (heads) {
    const float* hrow = heads + m * head_ld;
    const float4 d = *(const float4*)(hrow + a * 4);
    const float s0 = hrow[40 + 2 * a], s1 = hrow[40 + 2 * a + 1];
    const float mx = fmaxf(s0, s1);
    const float e0 = expf(s0 - mx), e1 = expf(s1 - mx);
    const float sum = e0 + e1;
    const float p0 = e0 / sum, p1 = e1 / sum;
    dy = d.y; dh = d.w; score = p1;
    if (cls_prob_out) { cls_prob_out[m * 20 + 2 * a] = p0; cls_prob_out[m * 20 + 2 * a + 1] = p1; }
    if (bbox_out) *(float4*)(bbox_out + m * 40 + a * 4) = d;
  } else {
    const float4 d = *(const float4*)(bbox_in + m * 40 + a * 4);
    dy = d.y; dh = d.w; score = cls_prob_in[m * 20 + 2 * a + 1];
  }

  float imH, imW, imS;
  if (im_info_pub) {                                       // (selects: a run-time index into kernel arguments would go through scratch)
    imH = img == 0 ? small.v[0] : img == 1 ? small.v[3] : img == 2 ? small.v[6] : small.v[9];
    imW = img == 0 ? small.v[1] : img == 1 ? small.v[4] : img == 2 ? small.v[7] : small.v[10];
    imS = img == 0 ? small.v[2] : img == 1 ? small.v[5] : img == 2 ? small.v[8] : small.v[11];
  } else { imH = im_info[img * 3 + 0]; imW = im_info[img * 3 + 1]; imS = im_info[img * 3 + 2]; }
  // shifted anchor (int -> fp32), bbox_transform_inv in numpy's fp32 operation order
  const float ax1 = (float)(x * 16), ax2 = (float)(x * 16 + 15);
  const float ay1 = (float)(y * 16 + c_anchor_y1[a]), ay2 = (float)(y * 16 + c_anchor_y2[a]);
  const float widths = ax2 - ax1 + 1.0f;
  const float heights = ay2 - ay1 + 1.0f;
  const float ctr_x = ax1 + 0.5f * widths;
  const float ctr_y = ay1 + 0.5f * heights;
  const float pred_ctr_y = dy * heights + ctr_y;
  const float pred_h = expf(dh) * heights;
  float x1 = ctr_x - 0.5f * widths;
  float y1 = pred_ctr_y - 0.5f * pred_h;
  float x2 = ctr_x + 0.5f * widths;
  float y2 = pred_ctr_y + 0.5f * pred_h;
  // clip_boxes: max(min(v, lim - 1), 0)
  const float wl = imW - 1.0f, hl = imH - 1.0f;
  x1 = fmaxf(fminf(x1, wl), 0.0f);
  y1 = fmaxf(fminf(y1, hl), 0.0f);
  x2 = fmaxf(fminf(x2, wl), 0.0f);
  y2 = fmaxf(fminf(y2, hl), 0.0f);
  // _filter_boxes
  const float ms = min_size * imS;
  const float ws = x2 - x1 + 1.0f, hs = y2 - y1 + 1.0f;
  // ragged batch (valid_rows: feature rows of every image, else null): the cells below an image are not the image's
  const bool keep = (ws >= ms) && (hs >= ms) && (!valid_rows || y < valid_rows[img]);

  *(float4*)(boxes4 + ((long long)img * per_img + idx) * 4) = make_float4(x1, y1, x2, y2);
  // High word = ~(order-preserving image of the score): ascending key = descending score for EVERY finite score (also 0.0
  // and negative values handed in through ctpn_proposals_from_host). The image of a finite float is never 0, so the high
  // word of a valid key is never 0xFFFFFFFF: KEY_INVALID sorts strictly after every valid key and the valid keys form a
  // prefix of the sorted segment (the radix sort only orders the high word). NaN never passes `keep`.
  const unsigned long long key = keep && (score == score)
                                     ? (((unsigned long long)(~score_order_bits(score))) << 32) | (unsigned int)idx
                                     : KEY_INVALID;
  keys[(long long)img * npad + idx] = key;
}

__global__ void fill_keys_kernel(unsigned long long* keys, int n_img, int npad, int per_img) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const int tail = npad - per_img;
  if (gid >= (long long)n_img * tail) return;
  const int img = (int)(gid / tail);
  const int i = (int)(gid - (long long)img * tail);
  keys[(long long)img * npad + per_img + i] = KEY_INVALID;
}

int launch_decode(const float* heads, int head_ld, int heads_are_probs, const float* cls_prob_in, const float* bbox_in,
                  const float* im_info_dev, float* cls_prob_out, float* bbox_out, unsigned long long* keys, float* boxes4,
                  const ProposalCfg& c, int npad, hipStream_t s, bool skip_fill, const float* im_info_host,
                  const int* valid_rows_dev) {
  const int per_img = c.hf * c.wf * 10;
  const long long total = (long long)c.n * per_img;
  if (npad > per_img && !skip_fill) {      // (the segmented sort of small batches never reads behind the image's keys and pads its merged buffer itself)
    const long long tail = (long long)c.n * (npad - per_img);
    hipLaunchKernelGGL(fill_keys_kernel, dim3((unsigned)((tail + 255) / 256)), dim3(256), 0, s, keys, c.n, npad, per_img);
  }
  ImInfoSmall small{};
  if (im_info_host && c.n <= 4) for (int i = 0; i < 3 * c.n; ++i) small.v[i] = im_info_host[i];
  hipLaunchKernelGGL(decode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     heads_are_probs ? nullptr : heads, head_ld, cls_prob_in, bbox_in, im_info_dev, cls_prob_out, bbox_out,
                     keys, boxes4, c.n, c.hf, c.wf, c.min_size, npad, small, im_info_host && c.n <= 4 ? (float*)im_info_dev : nullptr, valid_rows_dev);
  return launch_status("decode");
}

}  // namespace ctpn
