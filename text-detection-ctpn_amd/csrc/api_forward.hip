// C ABI of libctpn_hip.so, forward unit: image staging, the network forward on the ctx's streams, tensor read-back.
#include "ctx.h"
#include "../../include/ctpn_hip_train.h"
#include "unpack_dev.h"

namespace ctpn {

// host copy on a few pool threads: one core moves ~10 GB/s, a 52 MB batch would cost 5 ms of the submitting thread
static void parallel_memcpy(HostPool* pool, void* dst, const void* src, size_t bytes) {
  const size_t chunk = (size_t)8 << 20;
  const int nt = (int)std::min<size_t>(8, (bytes + chunk - 1) / chunk);
  if (nt <= 1 || !pool) { std::memcpy(dst, src, bytes); return; }
  const size_t per = ((bytes + nt - 1) / nt + 63) & ~(size_t)63;
  pool->run(nt, [=](int i) {
    const size_t lo = (size_t)i * per, hi = std::min(bytes, lo + per);
    if (lo < hi) std::memcpy((char*)dst + lo, (const char*)src + lo, hi - lo);
  }, 8);
}

// a ragged batch's heights on their way to the device: [heights(n) | feature rows(n)] through the set's page-locked array, copied on s
static int ragged_upload(ctpn_ctx* c, ctpn_ctx::RaggedSet& r, const int* heights, int n, hipStream_t s) {
  const size_t bytes = (size_t)c->max_batch * 2 * sizeof(int);
  int rc;
  if ((rc = r.host.grow(bytes)) || (rc = r.dev.grow(bytes)) || (rc = r.ev_copied.ensure())) return rc;      // on the set's first use
  if (r.copied_valid) CTPN_HIP_TRY(hipEventSynchronize(r.ev_copied));      // the copy that last read the page-locked array (long done)
  int* host = r.host.as<int>();
  for (int i = 0; i < n; ++i) { host[i] = heights[i]; host[n + i] = ragged_valid_rows(heights[i], 4); }
  CTPN_HIP_TRY(hipMemcpyAsync(r.dev.get(), host, (size_t)n * 2 * sizeof(int), hipMemcpyHostToDevice, s));
  CTPN_HIP_TRY(hipEventRecord(r.ev_copied, s));
  r.copied_valid = true;
  return CTPN_OK;
}

// the mask launch behind one stored map of a ragged batch (canvas n x hc x w): a bordered activation buffer at pooling level `level`
static int ragged_mask_act(void* buf, size_t pix_bytes, int level, const int* heights, const int* heights_dev, int n, int hc, int w, hipStream_t s) {
  const int hl = lvl(hc, level), wl = lvl(w, level);
  RaggedMap m;
  m.row_bytes = (long long)(wl + 2) * (long long)pix_bytes; m.img_bytes = (long long)(hl + 2) * m.row_bytes;
  m.top = 1; m.left_bytes = (int)pix_bytes; m.span_bytes = (int)(wl * pix_bytes); m.rows = hl; m.level = level;
  int pad = 0;
  for (int i = 0; i < n; ++i) pad = std::max(pad, hl - ragged_valid_rows(heights[i], level));
  return launch_ragged_mask(buf, m, heights_dev, n, pad, s);
}

// One rule for forward_impl and for pick_set (api_detect.hip), which has to know whether the forward will store conv1_1's map before it
// chooses the set: the uint8 feed of the 16-bit modes through the q-image ("conv1_kernel" = 2), "conv1_fuse", no keep_acts, a uniform batch,
// a shape the fused launch takes
bool forward_fuses_conv1(const ctpn_ctx* c, int is_f32, int n, int h, int w, const int* heights) {
  bool ragged = false;
  for (int i = 0; heights && i < n; ++i) ragged = ragged || heights[i] != h;
  const bool via_q = !is_f32 && dtype_is_half(c->prec) && c->conv1_mfma >= 2 && c->fs[0].q_img != nullptr;
  return via_q && c->conv1_fuse && !c->keep_acts && !ragged && conv1_fusable(c->prec, n, h, w, 64, 64, true, false);
}

int forward_impl(ctpn_ctx* c, ctpn_ctx::FwdSet& f, const void* images, int is_f32, int images_on_device, int n, int h, int w, bool tail_on_p, const int* heights, int rset,
                 bool beside) {
  if (!c || !images) return fail(CTPN_ERR_ARG, "null pointer");
  if (c->postproc_only) return fail(CTPN_ERR_STATE, "ctpn_forward: post-processing-only ctx (ctpn_create_postproc) has no network");
  if (!c->weights_loaded) return fail(CTPN_ERR_STATE, "ctpn_forward: weights not loaded");
  if (n <= 0 || n > c->max_batch || h < 16 || w < 16 || h > c->max_h || w > c->max_w)
    return fail(CTPN_ERR_CAPACITY, "ctpn_forward: batch/size outside what the ctx was created for (h, w >= 16)");
  // a ragged batch (h is the canvas height). One whose heights all equal h IS the uniform batch and takes the uniform path
  bool ragged = false;
  if (heights) {
    if (is_f32 || rset < 0 || rset > 2) return fail(CTPN_ERR_ARG, "ragged forward: uint8 canvas only");
    for (int i = 0; i < n; ++i) {
      if (heights[i] < 16 || heights[i] > h) return fail(CTPN_ERR_ARG, "ragged forward: every height must lie in 16 .. the canvas height");
      ragged = ragged || heights[i] != h;
    }
  }
  CTPN_HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = f.stream;
  int rc;
  hipStream_t ts = tail_on_p ? c->stream_p : s;      // stream of the recurrent tail
  const ctpn_ctx::FwdSet* prev_set = c->last;       // the set of the forward enqueued in front of this one
  if (!tail_on_p) {
    // a forward that keeps everything on `s` rewrites the set's xp / lstm_out / heads there: after their readers on stream_p -- the tail of the
    // set's previous asynchronous batch (if it ran there) and its decode kernel. The decode kernel reads `heads` only, so that wait sits in front of
    // the GEMM that writes `heads`, at the END of this forward (at its start it put the cross-stream round trip heads -> decode -> next
    // forward, ~45 us, between every two batches: round 4's batch-1 and batch-32 timelines)
    if (f.tail_pending) { CTPN_HIP_TRY(hipStreamWaitEvent(s, f.ev_tail, 0)); f.tail_pending = false; }
  }
  // Cross-batch order of `heads`: its last reader is the decode kernel of the set's previous submit. Where the most recent forward ran on this
  // set (one set in use: every synchronous caller, keep_acts, the fall-back) that is the batch just in front of this one and the wait stands, as
  // it always did. Where the two slots alternate between the sets, the reader is the batch two submits back: its slot has been collected -- the
  // host has seen ev_done, which stream_p records behind the decode kernel -- before this submit could reuse it, and no wait is enqueued (7.5 us
  // of an idle stream in front of the heads GEMM). A reader whose slot is still uncollected gets the wait whichever set ran last.
  const bool reader_live = f.ev_decoded && (prev_set == &f || (f.dec_slot >= 0 && c->slot[f.dec_slot].busy));
  auto wait_decoded = [&]() -> int {
    if (!tail_on_p && reader_live) CTPN_HIP_TRY(hipStreamWaitEvent(ts, f.ev_decoded, 0));
    return CTPN_OK;
  };
  // borders must be zero for this geometry
  if (f.gn != n || f.gh != h || f.gw != w) {
    if (f.tail_pending) { CTPN_HIP_TRY(hipStreamWaitEvent(s, f.ev_tail, 0)); f.tail_pending = false; }   // it still reads rpn_conv's output
    // (each set re-zeroes its own buffers, when its own geometry changes; set 1 has no buffer for a map the production path does not store)
    for (int i = 0; i < 14; ++i) if (f.act_conv[i]) CTPN_HIP_TRY(hipMemsetAsync(f.act_conv[i], 0, c->act_conv_bytes[i], s));
    for (int p = 0; p < 4; ++p) CTPN_HIP_TRY(hipMemsetAsync(f.act_pool[p], 0, c->act_pool_bytes[p], s));
    if (f.q_img) CTPN_HIP_TRY(hipMemsetAsync(f.q_img, 0, c->q_img_bytes, s));      // the zero frame around every image (only image pixels are rewritten)
    f.gn = n; f.gh = h; f.gw = w;
  }
  const void* img = images;
  int staged = -1;
  if (!images_on_device) {
    // Host images cross PCIe on their own stream into one of two staging buffers, so the copy of this batch overlaps the
    // previous batch's convolutions (the forward stream only waits for the copy event). A buffer is reused two calls later,
    // after the conv1_1 launch that read it (ev_consumed).
    staged = c->img_flip;
    c->img_flip ^= 1;
    if (c->consumed_valid[staged]) CTPN_HIP_TRY(hipStreamWaitEvent(c->stream_c, c->ev_consumed[staged], 0));
    const size_t bytes = (size_t)n * h * w * 3 * (is_f32 ? 4 : 1);
    const void* src = images;
    hipPointerAttribute_t attr;
    const bool locked = hipPointerGetAttributes(&attr, images) == hipSuccess && attr.type == hipMemoryTypeHost;
    if (!locked) {
      // A pageable source makes the runtime stage the copy itself and serialise it with the other streams (measured: 13.5
      // instead of 11.4 ms / step). Stage it here instead: host memcpy into a page-locked buffer of the ctx (this thread,
      // while the GPU works on the previous batch), then a truly asynchronous copy.
      (void)hipGetLastError();
      if (c->pin_stage[staged].bytes() < bytes) {
        if (c->pin_stage[staged]) CTPN_HIP_TRY(hipStreamSynchronize(c->stream_c));      // a copy may still read the block that goes
        c->h2d_valid[staged] = false;
        if ((rc = c->pin_stage[staged].grow(bytes)) || (rc = c->ev_h2d_done[staged].ensure())) return rc;
      }
      if (c->h2d_valid[staged]) CTPN_HIP_TRY(hipEventSynchronize(c->ev_h2d_done[staged]));   // the copy that last read this staging buffer
      parallel_memcpy(c->pool.get(), c->pin_stage[staged].get(), images, bytes);
      src = c->pin_stage[staged].get();
    }
    CTPN_HIP_TRY(hipMemcpyAsync(c->img_dev_b[staged], src, bytes, hipMemcpyHostToDevice, c->stream_c));
    if (!locked) { CTPN_HIP_TRY(hipEventRecord(c->ev_h2d_done[staged], c->stream_c)); c->h2d_valid[staged] = true; }
    CTPN_HIP_TRY(hipEventRecord(c->ev_copied[staged], c->stream_c));
    CTPN_HIP_TRY(hipStreamWaitEvent(s, c->ev_copied[staged], 0));
    img = c->img_dev_b[staged];
  }
  f.n = n; f.h = h; f.w = w;
  c->last = &f;
  f.fwd_ragged = ragged ? rset : -1;
  const int* hts_dev = nullptr;
  if (ragged) {
    if ((rc = ragged_upload(c, c->ragged[rset], heights, n, s))) return rc;
    hts_dev = c->ragged[rset].dev.as<int>();
  }
  int jpeg_src = -1;
  if (images_on_device && c->jpeg_ready)
    for (int b = 0; b < 2; ++b)
      if (c->jpeg[b].ready_valid && images == c->jpeg[b].out_dev.get()) {      // decoded on stream_c: the forward waits for its kernels, not the host
        CTPN_HIP_TRY(hipStreamWaitEvent(s, c->jpeg[b].ev_ready, 0));
        jpeg_src = b;
      }
  bool via_q = false, fuse1 = false;
  {
    Timed t(c, CTPN_KIND_CONV_FIRST, (double)n * h * w * (3.0 + 64.0 * c->es), s);
    // 16-bit modes: "conv1_kernel" picks exact-pixel MFMA through the q-image (2, uint8 feed) / split-operand MFMA (1) / VALU (0); split precision always takes the
    // split-operand MFMA kernel (fp32-class sums, stored as (hi, lo) planes); fp32: the VALU kernel
    const bool frags = c->prec == DType::SPLIT || (c->conv1_mfma && dtype_is_half(c->prec));
    // uint8 feed of the 16-bit modes ("conv1_kernel" = 2): bytes -> q-image; conv1_1 then runs inside conv1_2's window stage (the production
    // path: its 69 MB per image are never stored) or, with keep_acts / "conv1_fuse" = 0, stand-alone from the q-image: the same bytes
    via_q = !is_f32 && dtype_is_half(c->prec) && c->conv1_mfma >= 2 && f.q_img != nullptr;
    // a ragged batch takes the stand-alone form: the fused one never stores conv1_1, so nothing could be cleared below an image, where it
    // yields ReLU(bias) and not 0 (the two forms store the same bytes: option conv1_fuse)
    fuse1 = forward_fuses_conv1(c, is_f32, n, h, w, ragged ? heights : nullptr);
    if (!fuse1 && !f.act_conv[0]) return fail(CTPN_ERR_STATE, "ctpn_forward: the forward set has no buffer for conv1_1's map");      // pick_set vouches for it
    if (via_q) {
      if ((rc = launch_image_to_q((const uint8_t*)img, f.q_img, c->prec, n, h, w, s))) return rc;
      if (ragged) {      // the q-image's rows below an image: all four channels, the 1.0 that says "inside the image" included
        RaggedMap m;
        m.row_bytes = (long long)conv1_q_w(w) * 8; m.img_bytes = (long long)conv1_q_h(h) * m.row_bytes;
        m.top = 2; m.left_bytes = 16; m.span_bytes = w * 8; m.rows = h; m.level = 0;
        int pad = 0;
        for (int i = 0; i < n; ++i) pad = std::max(pad, h - heights[i]);
        if ((rc = launch_ragged_mask(f.q_img, m, hts_dev, n, pad, s))) return rc;
      }
      if (!fuse1 && (rc = launch_conv_first_from_q(f.q_img, conv1_p_frags(c->w_first_frags, c->prec), f.act_conv[0], c->prec, n, h, w, 0, w, s))) return rc;
    } else if (ragged) {
      // the kernels that read raw pixels (fp32, split precision; the 16-bit modes with conv1_kernel < 2) take the float feed instead, which they
      // compute identically (ctpn_forward_blob): p - mean inside an image, 0.0f below it
      const size_t need = (size_t)n * h * w * 3 * sizeof(float);
      if (need > f.ragged_blob.bytes()) {
        CTPN_HIP_TRY(hipStreamSynchronize(s));      // an earlier ragged forward may still read the block that goes
        if ((rc = f.ragged_blob.grow(need))) return rc;
      }
      if ((rc = launch_ragged_blob((const uint8_t*)img, f.ragged_blob.as<float>(), hts_dev, n, h, w, s))) return rc;
      if ((rc = launch_conv_first(f.ragged_blob.get(), 1, c->w_first, c->b_conv[0], f.act_conv[0], c->prec, n, h, w, s,
                                  frags ? c->w_first_frags : nullptr))) return rc;
    } else if ((rc = launch_conv_first(img, is_f32, c->w_first, c->b_conv[0], f.act_conv[0], c->prec, n, h, w, s,
                                       frags ? c->w_first_frags : nullptr))) return rc;
    if (ragged && (rc = ragged_mask_act(f.act_conv[0], (size_t)64 * c->es, 0, heights, hts_dev, n, h, w, s))) return rc;
  }
  f.act_valid[0] = !fuse1;      // fused: conv1_1's map exists only inside conv1_2's LDS windows
  if (jpeg_src >= 0) {           // the images came from ctpn_decode_jpeg_batch: its buffer may be rewritten once the first layer has read it
    CTPN_HIP_TRY(hipEventRecord(c->jpeg[jpeg_src].ev_consumed, s));
    c->jpeg[jpeg_src].consumed_valid = true;
  }
  if (staged >= 0) {
    CTPN_HIP_TRY(hipEventRecord(c->ev_consumed[staged], s));
    c->consumed_valid[staged] = true;
  }
  // the previous batch's tail (stream_p) overlaps conv1_1 only: the conv stack starts on an otherwise idle chip (its timed window too)
  // and rpn_conv's output, which lstm_pre reads, is not rewritten under it
  if (f.tail_pending) { CTPN_HIP_TRY(hipStreamWaitEvent(s, f.ev_tail, 0)); f.tail_pending = false; }
  if (c->tail_confine && c->ev_last_done) CTPN_HIP_TRY(hipStreamWaitEvent(s, c->ev_last_done, 0));      // option "tail_confine": see its declaration
  // Cross-batch order of the two sets' forwards (two_forwards_mode(): 2; 3 in measurement builds): this forward's conv stack starts behind the other
  // set's conv stack (3: behind its lstm_pre), so that only its q-image build and the head of its conv1_2 run beside the other batch's last kernels.
  // Two whole forwards side by side measured 2.8 % SLOWER than one stream (mode 1). The strips fork as they do on one stream: the machine behind a
  // main launch is empty again.
  const int gate = beside ? two_forwards_mode() - 1 : 0;
  if (gate > 0) {
    ctpn_ctx::FwdSet& o = c->fs[&f == &c->fs[0] ? 1 : 0];
    if (o.gate_valid) CTPN_HIP_TRY(hipStreamWaitEvent(s, o.ev_gate, 0));
  }
  f.gate_valid = false;
  const bool own_strips = beside && gate == 0;
  const void* cur = f.act_conv[0];
  int pool_i = 0;
  Event stack_a, stack_b;
  double stack_flops = 0.0;
  const bool stack_timed = c->prof && c->prof_mode == 2;
  if (stack_timed) {
    stack_a = prof_event(c); stack_b = prof_event(c);
    CTPN_HIP_TRY(hipEventRecord(stack_a, s));
  }
  for (int i = 1; i < 14; ++i) {
    const int hl = lvl(h, kConvs[i].level), wl = lvl(w, kConvs[i].level);
    double flops = 2.0 * (double)n * hl * wl * 9.0 * kConvs[i].ci * kConvs[i].co;
    if (fuse1 && i == 1) flops += 2.0 * (double)n * h * w * 27.0 * 64.0;      // conv1_1 is part of this launch
    stack_flops += flops;
    const bool fuse = kConvs[i].pool_after != 0;
    void* full = (!fuse || c->keep_acts) ? f.act_conv[i] : nullptr;
    {
      Timed t(c, CTPN_KIND_CONV_GEMM, flops, s);
      const bool f1 = fuse1 && i == 1;
      if ((rc = launch_conv3x3(cur, c->wt_conv[i], c->b_conv[i], full, fuse ? f.act_pool[pool_i] : nullptr, c->prec, n, hl, wl,
                               kConvs[i].ci, kConvs[i].co, 1, s, (c->prec == DType::SPLIT && i == 13) ? 1 : 0,
                               f1 ? f.q_img : nullptr, f1 ? conv1_p_frags(c->w_first_frags, c->prec) : nullptr, (c->conv_p64 ? 1 : 0) | (c->split_edge ? 2 : 0) | (own_strips ? 4 : 0)))) return rc;
    }
    f.act_valid[i] = full != nullptr;
    if (ragged) {      // every stored output, before the next layer reads it
      const size_t pix = (size_t)kConvs[i].co * ((c->prec == DType::SPLIT && i == 13) ? 6 : c->es);
      if (full && (rc = ragged_mask_act(full, pix, kConvs[i].level, heights, hts_dev, n, h, w, s))) return rc;
      if (fuse && (rc = ragged_mask_act(f.act_pool[pool_i], (size_t)kConvs[i].co * c->es, kConvs[i].level + 1, heights, hts_dev, n, h, w, s))) return rc;
    }
    cur = fuse ? f.act_pool[pool_i] : f.act_conv[i];
    if (fuse) ++pool_i;
  }
  if (stack_timed) {
    CTPN_HIP_TRY(hipEventRecord(stack_b, s));
    ProfRec r{CTPN_KIND_CONV_GEMM, std::move(stack_a), std::move(stack_b), stack_flops};
    r.launches = 13; r.span = true;
    c->pending.push_back(std::move(r));
  }
  if (two_forwards_mode() == 2 && f.ev_gate) { CTPN_HIP_TRY(hipEventRecord(f.ev_gate, s)); f.gate_valid = true; }
  const int hf = lvl(h, 4), wf = lvl(w, 4);
  const long long M5 = (long long)n * hf * wf;
  {  // lstm_pre: x_t @ kernel[:512] + bias for both directions (on `s` also when the tail overlaps: next to conv1_1 this MFMA GEMM took
     // 644 us instead of 174, measured -- only the latency-bound recurrence and the small heads GEMM move to stream_p)
    IGemm g{};
    // split precision: rpn_conv/3x3 stored [hi | lo | hi] pixels, wt_x rows are [hi | hi | lo]: a plain bf16 GEMM over K = 1536
    const bool sp = c->prec == DType::SPLIT;
    g.a = cur; g.wt = c->wt_x; g.bias = c->b_x; g.out = f.xp;
    g.M = M5; g.Ci = sp ? 1536 : 512; g.ntaps = 1; g.Co = 1024; g.a_plain = 0; g.H = hf; g.W = wf; g.tap_base_y = 1; g.tap_base_x = 1;
    g.out_bordered = 0; g.ldc = 1024; g.relu = 0;
    Timed t(c, CTPN_KIND_GEMM, 2.0 * (double)M5 * 512 * 1024, s);
    // 16-bit modes: lstm_pre is stored as fp16 (half the 272 MB round trip between this GEMM and the recurrence; see bilstm.hip) and
    // computed by the resident-weight-slice kernel (lstm_pre.hip); fp32 and split precision: the im2col GEMM
    if (dtype_is_half(c->prec)) { if ((rc = launch_lstm_pre(cur, c->wt_xf, c->b_x, f.xp, c->prec, n, hf, wf, s))) return rc; }
    else if ((rc = launch_igemm(g, sp ? DType::BF16 : c->prec, DType::F32, s))) return rc;
  }
  if (two_forwards_mode() == 3 && f.ev_gate) { CTPN_HIP_TRY(hipEventRecord(f.ev_gate, s)); f.gate_valid = true; }
  if (tail_on_p) {
    CTPN_HIP_TRY(hipEventRecord(f.ev_conv, s));
    CTPN_HIP_TRY(hipStreamWaitEvent(ts, f.ev_conv, 0));
  }
  {
    Timed t(c, CTPN_KIND_BILSTM, (double)M5 * (1024.0 + 256.0) * 4.0, ts);
    // "lstm_split": the recurrent product on split-bf16 MFMAs (fp32-class; v_exp / v_rcp gate math, 1 ulp each) in every mode but the fp32 gate,
    // whose kernel (and split precision's with lstm_split = 0) is exact-fp32 MFMA with exact gates
    const bool half = dtype_is_half(c->prec);
    if ((rc = launch_bilstm(f.xp, half ? 1 : 0, c->wh, f.lstm_out, n * hf, wf, ts, (c->lstm_split && c->prec != DType::F32) ? 1 : 0, half ? 1 : 0))) return rc;
  }
  const bool fold_heads = dtype_is_half(c->prec) && !c->keep_acts;
  if (fold_heads) {  // lstm_out (256) -> bbox (40) | cls (20) through the pre-multiplied FC x heads matrix
    IGemm g{};
    g.a = f.lstm_out; g.wt = c->wt_fold; g.bias = c->b_fold; g.out = f.heads;
    g.M = M5; g.Ci = 256; g.ntaps = 1; g.Co = 60; g.a_plain = 1; g.lda = 256; g.out_bordered = 0; g.ldc = 64; g.relu = 0;
    if ((rc = wait_decoded())) return rc;
    Timed t(c, CTPN_KIND_GEMM, 2.0 * (double)M5 * 256 * 60, ts);
    if ((rc = launch_igemm(g, DType::F32, DType::F32, ts))) return rc;
  } else {
  {  // lstm_o FC 256 -> 512 (no activation, reference network.py:110-113)
    IGemm g{};
    g.a = f.lstm_out; g.wt = c->wt_fc; g.bias = c->b_fc; g.out = f.fc_out;
    g.M = M5; g.Ci = 256; g.ntaps = 1; g.Co = 512; g.a_plain = 1; g.lda = 256; g.out_bordered = 0; g.ldc = 512; g.relu = 0;
    Timed t(c, CTPN_KIND_GEMM, 2.0 * (double)M5 * 256 * 512, ts);
    if ((rc = launch_igemm(g, DType::F32, DType::F32, ts))) return rc;
  }
  {  // rpn_bbox_pred (40) | rpn_cls_score (20) in one 512 -> 60 GEMM
    IGemm g{};
    g.a = f.fc_out; g.wt = c->wt_h; g.bias = c->b_h; g.out = f.heads;
    g.M = M5; g.Ci = 512; g.ntaps = 1; g.Co = 60; g.a_plain = 1; g.lda = 512; g.out_bordered = 0; g.ldc = 64; g.relu = 0;
    if ((rc = wait_decoded())) return rc;
    Timed t(c, CTPN_KIND_GEMM, 2.0 * (double)M5 * 512 * 60, ts);
    if ((rc = launch_igemm(g, DType::F32, DType::F32, ts))) return rc;
  }
  }
  if (tail_on_p) { CTPN_HIP_TRY(hipEventRecord(f.ev_tail, ts)); f.tail_pending = true; }
  f.fc_valid = !fold_heads;
  c->forward_done = true;
  c->proposals_done = false;
  return CTPN_OK;
}

}  // namespace ctpn

extern "C" {

int ctpn_forward(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w) {
  if (!c) return fail(CTPN_ERR_ARG, "null pointer");
  return forward_impl(c, c->fs[0], images, 0, images_on_device, n, h, w);
}
int ctpn_forward_blob(ctpn_ctx* c, const float* blob, int blob_on_device, int n, int h, int w) {
  if (!c) return fail(CTPN_ERR_ARG, "null pointer");
  return forward_impl(c, c->fs[0], blob, 1, blob_on_device, n, h, w);
}

int ctpn_forward_ragged(ctpn_ctx* c, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights) {
  if (!c || !canvas || !heights) return fail(CTPN_ERR_ARG, "ctpn_forward_ragged: null pointer");
  return forward_impl(c, c->fs[0], canvas, 0, canvas_on_device, n, hc, w, false, heights, 2);
}

int ctpn_feat_shape(ctpn_ctx* c, int* n, int* hf, int* wf) {
  if (!c) return fail(CTPN_ERR_ARG, "null ctx");
  if (!c->forward_done) return fail(CTPN_ERR_STATE, "no forward yet");
  const ctpn_ctx::FwdSet& f = *c->last;
  if (n) *n = f.n; if (hf) *hf = lvl(f.h, 4); if (wf) *wf = lvl(f.w, 4);
  return CTPN_OK;
}

namespace {
// a tensor name of the most recent forward -> where it is stored and in which form: the refusals, the shape and the capacity check that
// ctpn_get_tensor and ctpn_get_tensor_device share. ld and es are the stored pixel's value count and value size (split precision: 2 C or 3 C
// 16-bit values, the value is hi + lo)
struct StoredTensor { const void* src = nullptr; int n = 0, H = 0, W = 0, C = 0, ld = 0, es = 4; bool bordered = false, split = false, gates = false; DType t = DType::F32; };

int find_tensor(ctpn_ctx* c, const char* name, const void* out, size_t capacity, int shape4[4], StoredTensor& st) {
  if (!c || !name || !out) return fail(CTPN_ERR_ARG, "null pointer");
  if (!c->forward_done) return fail(CTPN_ERR_STATE, "ctpn_get_tensor: no forward yet");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  const ctpn_ctx::FwdSet& f = *c->last;      // the most recent forward's set, whichever slot submitted it
  const std::string nm(name);
  const int n = f.n, hf = lvl(f.h, 4), wf = lvl(f.w, 4);
  const void* src = nullptr; int H = 0, W = 0, C = 0, ld = 0; bool bordered = false; DType t = DType::F32;
  for (int i = 0; i < 14; ++i) if (nm == kConvs[i].name && !f.act_valid[i])
    return fail(CTPN_ERR_STATE, "ctpn_get_tensor: " + nm + (i == 0 ? " is computed inside conv1_2's window stage" : " is fused with its max-pool") + " and not stored; set the ctx option keep_acts = 1 (ctpn_set_option)");
  for (int i = 0; i < 14; ++i) if (nm == kConvs[i].name) { src = f.act_conv[i]; H = lvl(f.h, kConvs[i].level); W = lvl(f.w, kConvs[i].level); C = kConvs[i].co; ld = C; bordered = true; t = c->prec; }
  const int pool_src[4] = {1, 3, 6, 9};
  for (int p = 0; p < 4; ++p) if (nm == kPoolNames[p]) { src = f.act_pool[p]; H = lvl(f.h, p + 1); W = lvl(f.w, p + 1); C = kConvs[pool_src[p]].co; ld = C; bordered = true; t = c->prec; }
  if (nm == "lstm_pre") { src = f.xp; H = hf; W = wf; C = 1024; ld = 1024; if (dtype_is_half(c->prec)) t = DType::F16; }
  if (nm == "lstm_out") { src = f.lstm_out; H = hf; W = wf; C = 256; ld = 256; }
  if (nm == "lstm_o" && !f.fc_valid)
    return fail(CTPN_ERR_STATE, "ctpn_get_tensor: lstm_o is folded into the heads GEMM in the 16-bit modes; set the ctx option keep_acts = 1 (ctpn_set_option)");
  if (nm == "lstm_o") { src = f.fc_out; H = hf; W = wf; C = 512; ld = 512; }
  if (nm == "heads") { src = f.heads; H = hf; W = wf; C = 60; ld = 64; }
  if (nm == "rpn_cls_prob_reshape") { src = c->cls_prob; H = hf; W = wf; C = 20; ld = 20; }
  if (nm == "rpn_bbox_pred") { src = c->bbox_pred; H = hf; W = wf; C = 40; ld = 40; }
  if (!src) return fail(CTPN_ERR_ARG, "ctpn_get_tensor: unknown tensor name " + nm);
  if ((src == c->cls_prob || src == c->bbox_pred) && !c->proposals_done)
    return fail(CTPN_ERR_STATE, "ctpn_get_tensor: " + nm + " is produced by ctpn_proposals (the softmax is fused into the decode kernel)");
  const size_t need = (size_t)n * H * W * C;
  if (shape4) { shape4[0] = n; shape4[1] = H; shape4[2] = W; shape4[3] = C; }
  if (capacity < need) return fail(CTPN_ERR_CAPACITY, "ctpn_get_tensor: output buffer too small");
  // split precision: a pixel is [hi(C) | lo(C)] bf16 (rpn_conv/3x3: [hi | lo | hi]); the value is hi + lo
  st.split = t == DType::SPLIT;
  if (st.split) ld = (src == f.act_conv[13] ? 3 : 2) * C;
  st.src = src; st.n = n; st.H = H; st.W = W; st.C = C; st.ld = ld; st.es = st.split ? 2 : dtype_bytes(t); st.bordered = bordered; st.gates = src == f.xp; st.t = t;
  return CTPN_OK;
}
}  // namespace

int ctpn_get_tensor(ctpn_ctx* c, const char* name, float* out_host, size_t capacity, int shape4[4]) {
  StoredTensor st;
  if (const int rc = find_tensor(c, name, out_host, capacity, shape4, st)) return rc;
  const ctpn_ctx::FwdSet& f = *c->last;
  const void* src = st.src;
  const int n = st.n, H = st.H, W = st.W, C = st.C, ld = st.ld, es = st.es;
  const bool bordered = st.bordered, split = st.split;
  const DType t = st.t;
  CTPN_HIP_TRY(hipStreamSynchronize(f.stream));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));
  const int Hs = bordered ? H + 2 : H, Ws = bordered ? W + 2 : W;
  const size_t bytes = (size_t)n * Hs * Ws * ld * es;
  std::vector<char> tmp(bytes);
  CTPN_HIP_TRY(hipMemcpy(tmp.data(), src, bytes, hipMemcpyDeviceToHost));
  const int o = bordered ? 1 : 0;
  for (int in = 0; in < n; ++in)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t sp = (((size_t)in * Hs + y + o) * Ws + x + o) * ld;
        float* d = out_host + (((size_t)in * H + y) * W + x) * C;
        if (src == f.xp) {                      // device layout: permuted gate columns -> TF's i | j | f | o order (fp16 in the 16-bit modes)
          if (es == 2) {
            const uint16_t* sh = (const uint16_t*)tmp.data() + sp;
            for (int ch = 0; ch < 1024; ++ch) d[ch] = host_f16_to_f32(sh[(ch & ~511) + lstm_gate_col(ch & 511)]);
          } else {
            const float* sf = (const float*)tmp.data() + sp;
            for (int ch = 0; ch < 1024; ++ch) d[ch] = sf[(ch & ~511) + lstm_gate_col(ch & 511)];
          }
        } else if (es == 4) {
          std::memcpy(d, (const float*)tmp.data() + sp, (size_t)C * 4);
        } else {
          const uint16_t* sb = (const uint16_t*)tmp.data() + sp;
          if (split) for (int ch = 0; ch < C; ++ch) d[ch] = host_bf16_to_f32(sb[ch]) + host_bf16_to_f32(sb[C + ch]);
          else if (t == DType::F16) for (int ch = 0; ch < C; ++ch) d[ch] = host_f16_to_f32(sb[ch]);
          else for (int ch = 0; ch < C; ++ch) d[ch] = host_bf16_to_f32(sb[ch]);
        }
      }
  return CTPN_OK;
}

// ctpn_get_tensor with the unpacking done by a kernel (unpack.hip) and the result left in HBM: same names, shapes, refusals and values
int ctpn_get_tensor_device(ctpn_ctx* c, const char* name, float* out_dev, size_t capacity, int shape4[4]) {
  StoredTensor st;
  if (const int rc = find_tensor(c, name, out_dev, capacity, shape4, st)) return rc;
  const ctpn_ctx::FwdSet& f = *c->last;
  CTPN_HIP_TRY(hipStreamSynchronize(f.stream));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));
  UnpackDesc d{};
  d.n = st.n; d.H = st.H; d.W = st.W; d.C = st.C; d.ld = st.ld; d.border = st.bordered ? 1 : 0; d.gates = st.gates ? 1 : 0;
  d.kind = st.split ? UP_SPLIT : st.es == 4 ? UP_F32 : st.t == DType::F16 ? UP_F16 : UP_BF16;
  if (const int rc = launch_unpack(st.src, d, out_dev, c->stream)) return rc;
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream));
  return CTPN_OK;
}

}  // extern "C"
