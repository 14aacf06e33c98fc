// C ABI of libctpn_hip.so, context unit: error slot, create / destroy, options, synchronisation, profile read-out, and the process-wide
// CTPN_DEBUG_SYNC / CTPN_ROCTX helpers. See include/ctpn_hip.h for the contract and the reference interfaces each entry point replaces.
#include "ctx.h"

namespace ctpn {

static thread_local std::string t_err;
void set_error(const std::string& s) { t_err = s; }
int fail(int code, const std::string& s) { t_err = s; return code; }

static int env_int(const char* name, int dflt) { const char* v = std::getenv(name); return v && *v ? std::atoi(v) : dflt; }

static int dev_alloc(ctpn_ctx* c, void** p, size_t bytes, bool zero) {
  if (bytes == 0) bytes = 256;
  DevBuf b;
  if (const int rc = b.alloc(bytes)) return rc;
  *p = b.get();
  c->allocs.push_back(std::move(b));
  if (zero) CTPN_HIP_TRY(hipMemsetAsync(*p, 0, bytes, c->stream));
  return CTPN_OK;
}

// How two forwards on two sets (ctx.h, FwdSet) may overlap. 2, the product library's: a forward's conv stack starts behind the OTHER set's conv
// stack -- its q-image is built beside that stack's last layer, its conv1_2 (dynamic tile claims) runs beside the other batch's lstm_pre,
// recurrence and heads GEMM and takes the CUs they leave free. Measured on one box, five alternating runs each (profiles/ab_two_forwards.txt):
// 3766 - 3776 images/s against the parent's 3710 - 3717, +1.5 %. The other modes exist in the measurement build only (make ablation,
// CTPN_TWO_FORWARDS): 0 one set, the single-stream order (3712 - 3716); 1 the two forwards overlap freely -- two whole persistent conv kernels
// side by side, each at half speed and a little worse (3585 - 3620, -2.8 %); 3 the gate behind the other set's lstm_pre (3741 - 3751, +0.9 %).
int two_forwards_mode() {
#ifdef CTPN_ABLATION
  static const int v = env_int("CTPN_TWO_FORWARDS", 2);
  return v < 0 || v > 3 ? 2 : v;
#else
  return 2;
#endif
}

int debug_sync() { static const int v = env_int("CTPN_DEBUG_SYNC", 0); return v; }
// CTPN_ROCTX=1: roctx ranges (rocprofv3 --marker-trace). librocprofiler-sdk-roctx.so is dlopen'ed on first use, so the library has no
// link-time dependency on the profiler SDK: an install without it still loads, and CTPN_ROCTX=1 there is a silent no-op.
const RoctxApi& roctx_api() {
  static const RoctxApi api = [] {
    RoctxApi a;
    if (!env_int("CTPN_ROCTX", 0)) return a;
    void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
      const char* rp = std::getenv("ROCM_PATH");
      const std::string p = std::string(rp && *rp ? rp : "/opt/rocm") + "/lib/librocprofiler-sdk-roctx.so";
      h = dlopen(p.c_str(), RTLD_NOW | RTLD_GLOBAL);
    }
    if (h) {
      a.push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
      a.pop = (int (*)())dlsym(h, "roctxRangePop");
      if (!a.push || !a.pop) { a.push = nullptr; a.pop = nullptr; }
    }
    return a;
  }();
  return api;
}
int roctx_on() { return roctx_api().push != nullptr; }

static int prof_drain(ctpn_ctx* c) {
  if (c->pending.empty()) return CTPN_OK;
  CTPN_HIP_TRY(sync_forwards(c));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));
  // Mode 2's records (span: one [first conv start, last conv end] pair per forward) may come from two forwards that were in flight together, on
  // two streams: their SUM would count the interleaved time twice. What is reported is the length of the UNION of the intervals -- the time during
  // which a conv stack was running. Event times of one device are comparable across streams; intervals that do not overlap (every synchronous
  // caller, one forward set) contribute exactly their own elapsed time, as before. Everything pending here has completed (the syncs above), and a
  // later drain's forwards start after them, so the union per drain is the union over the run.
  struct Span { double t0, t1; float own; };
  std::vector<Span> spans;
  hipEvent_t origin = nullptr;
  for (auto& r : c->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      c->prof_n[r.kind] += r.launches; c->prof_work[r.kind] += r.work;
      float off = 0.f;
      if (!r.span) c->prof_ms[r.kind] += ms;
      else if (!origin) { origin = r.a; spans.push_back({0.0, (double)ms, ms}); }
      else if (hipEventElapsedTime(&off, origin, r.a) == hipSuccess) spans.push_back({(double)off, (double)off + (double)ms, ms});
      else c->prof_ms[r.kind] += ms;
    }
  }
  std::sort(spans.begin(), spans.end(), [](const Span& x, const Span& y) { return x.t0 < y.t0; });
  double covered = 0.0;
  for (size_t i = 0; i < spans.size(); ++i) {
    const Span& sp = spans[i];
    if (i == 0 || sp.t0 >= covered) c->prof_ms[CTPN_KIND_CONV_GEMM] += sp.own;
    else if (sp.t1 > covered) c->prof_ms[CTPN_KIND_CONV_GEMM] += sp.t1 - covered;
    if (i == 0 || sp.t1 > covered) covered = sp.t1;
  }
  for (auto& r : c->pending) { c->free_events.push_back(std::move(r.a)); c->free_events.push_back(std::move(r.b)); }
  c->pending.clear();
  return CTPN_OK;
}

// one block for everything a submitted batch returns (device side and, mirrored, every slot's page-locked host side)
struct PackLayout { size_t tlb, tls, keep, kcnt, rois, rcnt, total; };
static PackLayout pack_layout(size_t mb, size_t post) {
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  PackLayout L; size_t o = 0;
  L.tlb = o; o = al(o + mb * post * 4 * sizeof(float));
  L.tls = o; o = al(o + mb * post * sizeof(float));
  L.keep = o; o = al(o + mb * post * sizeof(int));
  L.kcnt = o; o = al(o + mb * sizeof(int));
  L.rois = o; o = al(o + mb * post * 5 * sizeof(float));
  L.rcnt = o; o = al(o + mb * sizeof(int));
  L.total = o;
  return L;
}

// Everything of a ctx that is laid out by its proposal capacity (ctx.h, post_max): built as a whole, then adopted as a whole, so that a failed
// allocation in ctpn_reserve_proposals leaves the ctx as it was.
struct TailSet { ctpn_ctx::TailBufs dev; PinnedBuf pack[2], crecs[2]; };
static int tail_alloc(int max_batch, int post, TailSet& t) {
  const size_t mb = (size_t)max_batch, rows = (size_t)post, cap = rows / 2;
  const PackLayout L = pack_layout(mb, rows);
  const size_t work = connect_work_bytes(post);
  int rc;
  if ((rc = t.dev.out_pack.alloc(L.total)) || (rc = t.dev.roi_anchor.alloc(mb * rows * sizeof(int))) || (rc = t.dev.tl_spill.alloc(mb * rows * 4 * sizeof(float))) ||
      (rc = t.dev.conn_recs.alloc(mb * 2 * cap * 9 * sizeof(double))) || (rc = t.dev.conn_scratch.alloc(mb * (rows < 1024 ? 1024 : rows) * 20 * sizeof(double))) ||
      (work && (rc = t.dev.conn_work.alloc(mb * work)))) return rc;
  for (int k = 0; k < 2; ++k)
    if ((rc = t.pack[k].alloc(L.total)) || (rc = t.crecs[k].alloc(mb * 2 * cap * 9 * sizeof(double)))) return rc;
  return CTPN_OK;
}
// the ctx is idle (streams drained or not yet used); the new device blocks are zeroed on the ctx's stream where create always zeroed them
static int tail_adopt(ctpn_ctx* c, int post, TailSet& t) {
  const PackLayout L = pack_layout((size_t)c->max_batch, (size_t)post);
  CTPN_HIP_TRY(hipMemsetAsync(t.dev.out_pack.get(), 0, L.total, c->stream));
  CTPN_HIP_TRY(hipMemsetAsync(t.dev.roi_anchor.get(), 0, t.dev.roi_anchor.bytes(), c->stream));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream));
  c->tail = std::move(t.dev);
  c->post_max = post; c->conn_cap = post / 2;
  c->pack_bytes = L.total;
  c->out_pack = c->tail.out_pack.as<char>();
  c->tl_boxes = (float*)(c->out_pack + L.tlb); c->tl_scores = (float*)(c->out_pack + L.tls); c->tl_keep = (int*)(c->out_pack + L.keep);
  c->tl_keep_counts = (int*)(c->out_pack + L.kcnt); c->rois = (float*)(c->out_pack + L.rois); c->keep_counts = (int*)(c->out_pack + L.rcnt);
  c->roi_anchor = c->tail.roi_anchor.as<int>(); c->tl_spill = c->tail.tl_spill.as<float>();
  c->conn_recs = c->tail.conn_recs.as<double>(); c->conn_scratch = c->tail.conn_scratch.as<double>(); c->conn_work = c->tail.conn_work.as<char>();
  for (int k = 0; k < 2; ++k) {
    ctpn_ctx::Slot& sl = c->slot[k];
    sl.pack = std::move(t.pack[k]); sl.crecs = std::move(t.crecs[k]);
    char* pack = sl.pack.as<char>();
    sl.tlb = (float*)(pack + L.tlb); sl.tls = (float*)(pack + L.tls); sl.keep = (int*)(pack + L.keep); sl.kcnt = (int*)(pack + L.kcnt);
    sl.rois = (float*)(pack + L.rois); sl.rcnt = (int*)(pack + L.rcnt);
  }
  c->last_post = 0; c->last_prop_n = 0;      // what ctpn_proposal_anchors / ctpn_debug_proposal_fetch would read is gone
  return CTPN_OK;
}

static int create_impl(ctpn_ctx** out, int device_id, int max_batch, int max_h, int max_w, int precision, bool postproc_only) {
  if (!out) return fail(CTPN_ERR_ARG, "ctpn_create: out is null");
  *out = nullptr;
  if (max_batch <= 0 || max_h < 16 || max_w < 16) return fail(CTPN_ERR_ARG, "ctpn_create: max_batch > 0 and max_h, max_w >= 16 required");
  if (precision < CTPN_PREC_FP32 || precision > CTPN_PREC_SPLIT) return fail(CTPN_ERR_ARG, "ctpn_create: unknown precision");
  int ndev = ctpn_device_count();
  if (ndev <= 0) return fail(CTPN_ERR_NODEVICE, "ctpn_create: no HIP device visible (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) {
    // the usual cause on a multi-GPU node: a rank whose LOCAL_RANK is not among the devices its environment lets it see
    const char* hv = getenv("HIP_VISIBLE_DEVICES");
    const char* rv = getenv("ROCR_VISIBLE_DEVICES");
    return fail(CTPN_ERR_ARG, "ctpn_create: device_id " + std::to_string(device_id) + " out of range: " + std::to_string(ndev) +
                " device(s) visible (HIP_VISIBLE_DEVICES=" + (hv ? hv : "unset") + ", ROCR_VISIBLE_DEVICES=" + (rv ? rv : "unset") + "); one process per GPU needs LOCAL_RANK < that count");
  }
  CTPN_HIP_TRY(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  CTPN_HIP_TRY(hipGetDeviceProperties(&prop, device_id));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return fail(CTPN_ERR_NODEVICE, std::string("ctpn_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");

  // the one failure path: every return before `*out` is set hands the half-built ctx to ctpn_destroy, which drains its streams and lets it die
  struct Destroy { void operator()(ctpn_ctx* x) const { (void)ctpn_destroy(x); } };
  std::unique_ptr<ctpn_ctx, Destroy> owner(new ctpn_ctx());
  ctpn_ctx* c = owner.get();
  c->device = device_id; c->max_batch = max_batch; c->max_h = max_h; c->max_w = max_w;
  c->prec = prec_dtype(precision);
  c->es = dtype_bytes(c->prec);
  c->wx_row_bytes = c->prec == DType::SPLIT ? (size_t)3 * 512 * 2 : (size_t)512 * c->es;
  // 16-bit throughput modes: the recurrent product h Wh on split-bf16 MFMAs by default (state, gates, accumulation fp32; three bf16 terms per
  // product: |lstm_out - exact-fp32 kernel| < 3e-5, two orders below the modes' own conv rounding; 0.32 -> 0.16 ms per 32-image batch).
  // split precision takes the split-bf16 recurrence too since round 6: it IS this mode's arithmetic ((hi, lo) bf16 pairs, three MFMA terms, fp32
  // accumulate: what its convolutions do), the bench's accuracy object does not move (cls_prob 3.48e-5, 100 % lines either way) and a lone image
  // saves 0.2 ms of its 2.05 (343 -> 138 us at batch 32). fp32 keeps the exact kernel; option lstm_split = 0 restores it anywhere.
  c->lstm_split = (dtype_is_half(c->prec) || c->prec == DType::SPLIT) ? 1 : 0;
  c->tail_confine = 0;
  c->postproc_only = postproc_only;
  for (int i = 0; i < TAIL_PARAM_COUNT; ++i) c->tail_raw[i] = tail_param(i)->dflt;
  {
    // host workers: the node's cores divided by the ranks that share it (torchrun exports LOCAL_WORLD_SIZE), CTPN_HOST_THREADS
    // overrides; CTPN_AFFINITY=1 pins them to the block of cores [local_rank * budget, ...)
    const unsigned hw = std::thread::hardware_concurrency();
    c->host_threads = ctpn_host_thread_budget((int)(hw ? hw : 1), env_int("LOCAL_WORLD_SIZE", 1), env_int("CTPN_HOST_THREADS", 0));
    const int first_cpu = env_int("CTPN_AFFINITY", 0) ? env_int("LOCAL_RANK", 0) * c->host_threads : -1;
    c->pool.reset(new HostPool(c->host_threads, first_cpu));
  }
  int rc = CTPN_OK;
  auto A = [&](void** p, size_t bytes, bool zero) { if (rc == CTPN_OK) rc = dev_alloc(c, p, bytes, zero); };
  ctpn_ctx::FwdSet& f0 = c->fs[0];      // allocated here; set 1: ensure_set1
  if ((rc = f0.stream.ensure()) || (rc = c->stream_p.ensure())) return rc;
  c->stream = f0.stream;
  // (the proposal stream at the highest stream priority was measured in round 2: no effect -- placement is by free resources)
  // (the proposal stream at the highest stream priority: measured in round 6 with the tail confined -- 1163 against 1164 images/s in split precision,
  // -0.2 % in bf16: the dispatcher does not hand CUs to the 1024-thread NMS workgroups any sooner. Not used.)
  if (f0.ev_conv.ensure() != CTPN_OK || f0.ev_tail.ensure() != CTPN_OK || f0.ev_gate.ensure() != CTPN_OK) return fail(CTPN_ERR_HIP, "ctpn_create: events");
  for (auto& sl : c->slot) {
    const size_t mb = (size_t)max_batch;
    const bool ok = sl.im_info.alloc(mb * 3 * sizeof(float)) == CTPN_OK &&
                    sl.ccnt.alloc(mb * 3 * sizeof(int)) == CTPN_OK && sl.ev_heads.ensure() == CTPN_OK && sl.ev_decoded.ensure() == CTPN_OK && sl.ev_done.ensure() == CTPN_OK;
    if (!ok) return fail(CTPN_ERR_HIP, "ctpn_create: pinned host buffers / events");
  }
  {
    // what the proposal capacity lays out (the slots' packs and connector records among it), at the default capacity
    TailSet t;
    if (tail_alloc(max_batch, c->post_max, t) != CTPN_OK) return fail(CTPN_ERR_HIP, "ctpn_create: pinned host buffers / events");
    if ((rc = tail_adopt(c, c->post_max, t))) return rc;
  }

  const int hf = lvl(max_h, 4), wf = lvl(max_w, 4);
  c->m5_max = (size_t)max_batch * hf * wf;
  if (!postproc_only) {
  A((void**)&c->arena, (size_t)CTPN_WEIGHT_FLOATS * sizeof(float), false);
  A((void**)&c->w_first, 27 * 64 * sizeof(float), false);
  A(&c->w_first_frags, CF_FRAGS_TOTAL, true);
  for (int i = 0; i < 14; ++i) {
    A((void**)&c->b_conv[i], (size_t)kConvs[i].co * sizeof(float), true);
    // 16-bit / fp32: [Co][9 Ci] elements; split precision: [Co][9][3 Ci] bf16
    if (i > 0) A(&c->wt_conv[i], (size_t)kConvs[i].co * 9 * kConvs[i].ci * (c->prec == DType::SPLIT ? 6 : c->es), true);
  }
  A(&c->wt_x, (size_t)1024 * c->wx_row_bytes, true);
  if (dtype_is_half(c->prec)) A(&c->wt_xf, (size_t)1024 * 512 * 2, true);
  A((void**)&c->b_x, 1024 * sizeof(float), true);
  A((void**)&c->wh, (size_t)2 * 128 * 512 * sizeof(float), true);
  A((void**)&c->wt_fc, (size_t)512 * 256 * sizeof(float), true);
  A((void**)&c->b_fc, 512 * sizeof(float), true);
  A((void**)&c->wt_h, (size_t)64 * 512 * sizeof(float), true);
  A((void**)&c->b_h, 64 * sizeof(float), true);
  A((void**)&c->wt_fold, (size_t)64 * 256 * sizeof(float), true);
  A((void**)&c->b_fold, 64 * sizeof(float), true);

  for (int i = 0; i < 14; ++i) {
    const int hl = lvl(max_h, kConvs[i].level), wl = lvl(max_w, kConvs[i].level);
    // + slack: the weights-in-registers conv kernel fetches edge tiles' input windows without clamping (conv3x3.hip), i.e. up to
    // 8 bordered rows + one window row past the last image; those pixels only feed outputs that are never stored
    // bytes per pixel: channels x element size; split precision: [hi | lo] planes = 4 bytes per channel, and rpn_conv/3x3 (which feeds the
    // LSTM projection GEMM) [hi | lo | hi] = 6
    const size_t pix_b = (size_t)kConvs[i].co * ((c->prec == DType::SPLIT && i == 13) ? 6 : c->es);
    c->act_conv_bytes[i] = ((size_t)max_batch * (hl + 2) * (wl + 2) + act_slack_pixels(wl)) * pix_b;
    const size_t front = act_front_pixels(wl) * pix_b;
    A(&f0.act_conv[i], front + c->act_conv_bytes[i], true);
    if (f0.act_conv[i]) f0.act_conv[i] = (char*)f0.act_conv[i] + front;     // allocs[] owns the block
  }
  {
    const int pool_src[4] = {1, 3, 6, 9};
    for (int p = 0; p < 4; ++p) {
      const int hl = lvl(max_h, p + 1), wl = lvl(max_w, p + 1);
      c->act_pool_bytes[p] = ((size_t)max_batch * (hl + 2) * (wl + 2) + act_slack_pixels(wl)) * kConvs[pool_src[p]].co * c->es;
      const size_t front = act_front_pixels(wl) * kConvs[pool_src[p]].co * c->es;
      A(&f0.act_pool[p], front + c->act_pool_bytes[p], true);
      if (f0.act_pool[p]) f0.act_pool[p] = (char*)f0.act_pool[p] + front;
    }
  }
  if (dtype_is_half(c->prec)) { c->q_img_bytes = conv1_q_bytes(max_batch, max_h, max_w); A(&f0.q_img, c->q_img_bytes, true); }
  A((void**)&c->img_dev, (size_t)max_batch * max_h * max_w * 3 * sizeof(float), false);
  c->img_dev_b[0] = c->img_dev;
  A((void**)&c->img_dev_b[1], (size_t)max_batch * max_h * max_w * 3 * sizeof(float), false);
  if (rc == CTPN_OK) {
    bool ok = c->stream_c.ensure() == CTPN_OK;
    for (int b = 0; b < 2 && ok; ++b) ok = c->ev_copied[b].ensure() == CTPN_OK && c->ev_consumed[b].ensure() == CTPN_OK;
    if (!ok) rc = fail(CTPN_ERR_HIP, "ctpn_create: copy stream / events");
  }
  A((void**)&f0.xp, c->m5_max * 1024 * sizeof(float), false);
  A((void**)&f0.lstm_out, c->m5_max * 256 * sizeof(float), false);
  A((void**)&f0.fc_out, c->m5_max * 512 * sizeof(float), false);
  A((void**)&f0.heads, c->m5_max * 64 * sizeof(float), true);
  }  // !postproc_only
  A((void**)&c->cls_prob, c->m5_max * 20 * sizeof(float), false);
  A((void**)&c->bbox_pred, c->m5_max * 40 * sizeof(float), false);
  A((void**)&c->cls_in, c->m5_max * 20 * sizeof(float), false);
  A((void**)&c->bbox_in, c->m5_max * 40 * sizeof(float), false);
  c->npad_max = next_pow2(hf * wf * 10);
  A((void**)&c->keys, (size_t)max_batch * c->npad_max * sizeof(unsigned long long), false);
  A((void**)&c->keys_tmp, (size_t)max_batch * c->npad_max * sizeof(unsigned long long), false);
  A((void**)&c->boxes4, (size_t)max_batch * hf * wf * 10 * 4 * sizeof(float), false);
  A((void**)&c->sorted_boxes, (size_t)max_batch * c->topn_max * 4 * sizeof(float), false);
  A((void**)&c->sorted_scores, (size_t)max_batch * c->topn_max * sizeof(float), false);
  A((void**)&c->valid_counts, (size_t)max_batch * sizeof(int), true);
  A((void**)&c->keep_idx, (size_t)max_batch * c->topn_max * sizeof(int), false);
  // (what a submitted batch hands back to the host -- connector front end (tl_*), rois and their counts -- and the other blocks laid out by the
  // proposal capacity: tail_adopt above)
  A((void**)&c->kept_spill, (size_t)max_batch * c->topn_max * 4 * sizeof(float), false);
  A((void**)&c->sorted_anchor, (size_t)max_batch * c->topn_max * sizeof(int), false);
  A((void**)&c->tl_counts, (size_t)max_batch * sizeof(int), true);
  A((void**)&c->nms_mw_scratch, (size_t)NMS_MW_CAP_BATCH * NMS_MW_SCRATCH_BYTES, true);
  A((void**)&c->nms_colid, (size_t)NMS_MW_CAP_BATCH * ((c->topn_max + 15) & ~15), true);
  A((void**)&c->conn_counts, (size_t)max_batch * 3 * sizeof(int), true);
  A((void**)&c->im_info_dev, (size_t)max_batch * 3 * sizeof(float), true);
  if (rc == CTPN_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(CTPN_ERR_HIP, "ctpn_create: sync failed");
  if (rc != CTPN_OK) return rc;
  *out = owner.release();
  return CTPN_OK;
}

// bytes in front of a bordered activation buffer (act_front_pixels): conv layer i / pooled map p
static size_t conv_front_bytes(const ctpn_ctx* c, int i) {
  return act_front_pixels(lvl(c->max_w, kConvs[i].level)) * (size_t)kConvs[i].co * ((c->prec == DType::SPLIT && i == 13) ? 6 : c->es);
}
static size_t pool_front_bytes(const ctpn_ctx* c, int p) {
  const int pool_src[4] = {1, 3, 6, 9};
  return act_front_pixels(lvl(c->max_w, p + 1)) * (size_t)kConvs[pool_src[p]].co * c->es;
}

// one zeroed block of forward set 1, on the set's stream (the forward that reads it follows on that stream); false: out of memory
static bool set1_block(ctpn_ctx* c, ctpn_ctx::FwdSet& f, void** p, size_t front, size_t bytes) {
  DevBuf b;
  if (b.alloc(front + bytes) != CTPN_OK) { (void)hipGetLastError(); return false; }
  void* raw = b.get();
  f.allocs.push_back(std::move(b));
  if (hipMemsetAsync(raw, 0, front + bytes, f.stream) != hipSuccess) { (void)hipGetLastError(); return false; }
  *p = (char*)raw + front;
  c->set1_bytes += front + bytes;
  return true;
}

// Forward set 1 (ctx.h, FwdSet), on the first submit that finds the other slot in flight: a stream, the two tail_overlap events and the buffers the
// production path stores -- every unpooled layer's map but conv1_1's, the four pooled maps, the q-image, lstm_pre, lstm_out, heads, and lstm_o
// where the heads GEMM is not folded (fp32, split precision). At 32 x 600 x 900 in bf16 that is 4.7 GB beside the 11.2 GB of set 0: the
// full-resolution maps of the four pooled layers and conv1_1's are 6.4 GB. need_conv1: the forward about to run stores conv1_1's map (a ragged
// batch, conv1_fuse = 0, fp32 / split precision): that one block is added when first asked for.
// false: this ctx stays on set 0 (keep_acts stores maps set 1 has no room for; per-stage profiling times one stream; no memory) -- never an error.
bool ensure_set1(ctpn_ctx* c, bool need_conv1) {
  if (two_forwards_mode() == 0 || c->postproc_only || c->keep_acts || (c->prof && c->prof_mode == 1) || c->set1_state < 0) return false;
  ctpn_ctx::FwdSet& f = c->fs[1];
  if (c->set1_state == 0) {
    bool ok = f.stream.ensure() == CTPN_OK && f.ev_conv.ensure() == CTPN_OK && f.ev_tail.ensure() == CTPN_OK && f.ev_gate.ensure() == CTPN_OK;
    for (int i = 1; i < 14 && ok; ++i)
      if (!kConvs[i].pool_after) ok = set1_block(c, f, &f.act_conv[i], conv_front_bytes(c, i), c->act_conv_bytes[i]);
    for (int p = 0; p < 4 && ok; ++p) ok = set1_block(c, f, &f.act_pool[p], pool_front_bytes(c, p), c->act_pool_bytes[p]);
    if (ok && dtype_is_half(c->prec)) ok = set1_block(c, f, &f.q_img, 0, c->q_img_bytes);
    ok = ok && set1_block(c, f, (void**)&f.xp, 0, c->m5_max * 1024 * sizeof(float)) && set1_block(c, f, (void**)&f.lstm_out, 0, c->m5_max * 256 * sizeof(float)) &&
         set1_block(c, f, (void**)&f.heads, 0, c->m5_max * 64 * sizeof(float));
    if (ok && !dtype_is_half(c->prec)) ok = set1_block(c, f, (void**)&f.fc_out, 0, c->m5_max * 512 * sizeof(float));
    if (!ok) {
      (void)hipGetLastError();
      if (f.stream) (void)hipStreamSynchronize(f.stream);
      f = ctpn_ctx::FwdSet();      // the half-built set's blocks, events and stream go with it
      c->set1_bytes = 0;
      c->set1_state = -1;
      return false;
    }
    c->set1_state = 1;
  }
  if (need_conv1 && !f.act_conv[0] && !set1_block(c, f, &f.act_conv[0], conv_front_bytes(c, 0), c->act_conv_bytes[0])) return false;      // this submit runs on set 0
  return true;
}

// ---- options: behaviour switches of ONE ctx (two ctxs in a process can choose differently; nothing here is read from the environment) ----
// one row per option, in ABI order (ctpn_option_name's index): name, the member it sets, the range ctpn_set_option accepts
struct Option { const char* name; int ctpn_ctx::* member; int lo, hi; };
static const Option kOptions[] = {
    {"keep_acts", &ctpn_ctx::keep_acts, 0, 1},
    {"conv1_kernel", &ctpn_ctx::conv1_mfma, 0, 2},
    {"conv1_fuse", &ctpn_ctx::conv1_fuse, 0, 1},
    {"lstm_split", &ctpn_ctx::lstm_split, 0, 1},
    {"nms_columns", &ctpn_ctx::nms_columns, 0, 3},
    {"nms_check", &ctpn_ctx::nms_check, 0, 1},
    {"connect_device", &ctpn_ctx::connect_device, 0, 1},
    {"tail_overlap", &ctpn_ctx::tail_overlap, 0, 1},
    {"conv_p64", &ctpn_ctx::conv_p64, 0, 1},
    {"tail_confine", &ctpn_ctx::tail_confine, 0, 1},
    {"nms_prefix", &ctpn_ctx::nms_prefix, 0, 1},
    {"debug_hog", &ctpn_ctx::debug_hog, 0, 200000},
    {"debug_nms", &ctpn_ctx::debug_nms, 0, 15},
    {"split_edge", &ctpn_ctx::split_edge, 0, 1},
};
static const Option* find_option(const std::string& k) {
  for (const Option& o : kOptions) if (k == o.name) return &o;
  return nullptr;
}

}  // namespace ctpn

// =============================================================================================
extern "C" {

int ctpn_abi_version(void) { return CTPN_ABI_VERSION; }
const char* ctpn_last_error(void) { return t_err.c_str(); }
int ctpn_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int ctpn_host_thread_budget(int cpu_count, int local_world_size, int requested) {
  if (requested > 0) return requested > 256 ? 256 : requested;
  if (cpu_count < 1) cpu_count = 1;
  if (local_world_size < 1) local_world_size = 1;
  int b = cpu_count / local_world_size;
  return b < 1 ? 1 : (b > 32 ? 32 : b);      // 32 = images per batch of the benchmark configuration: more threads have nothing to do
}

int ctpn_create(ctpn_ctx** out, int device_id, int max_batch, int max_h, int max_w, int precision) {
  return create_impl(out, device_id, max_batch, max_h, max_w, precision, false);
}

int ctpn_create_postproc(ctpn_ctx** out, int device_id, int max_batch, int max_hf, int max_wf) {
  if (max_hf < 1 || max_wf < 1 || max_hf > (1 << 20) / 16 || max_wf > (1 << 20) / 16) return fail(CTPN_ERR_ARG, "ctpn_create_postproc: feature-map size out of range");
  return create_impl(out, device_id, max_batch, max_hf * 16, max_wf * 16, CTPN_PREC_FP32, true);
}

int ctpn_option_count(void) { return (int)(sizeof(kOptions) / sizeof(kOptions[0])); }
const char* ctpn_option_name(int index) { return index >= 0 && index < ctpn_option_count() ? kOptions[index].name : nullptr; }
int ctpn_set_option(ctpn_ctx* c, const char* key, int value) {
  if (!c || !key) return fail(CTPN_ERR_ARG, "ctpn_set_option: null pointer");
  const Option* o = find_option(key);
  if (!o) return fail(CTPN_ERR_ARG, std::string("ctpn_set_option: unknown option ") + key);
  if (value < o->lo || value > o->hi) return fail(CTPN_ERR_ARG, std::string("ctpn_set_option: value out of range for ") + key);
  if (c->*(o->member) == value) return CTPN_OK;
  // a switch changes what the queued work would read / which stream runs it: drain first
  CTPN_HIP_TRY(hipSetDevice(c->device));
  CTPN_HIP_TRY(sync_forwards(c));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));
  for (auto& sl : c->slot) if (sl.busy) return fail(CTPN_ERR_STATE, "ctpn_set_option: a submitted batch has not been collected");
  for (auto& f : c->fs) f.tail_pending = false;
  c->nms_mw_dirty = true;           // both streams are drained: the next proposal launch re-zeroes the multi-workgroup NMS's scratch (8 KB memset)
  c->*(o->member) = value;
  return CTPN_OK;
}
int ctpn_get_option(ctpn_ctx* c, const char* key, int* value_out) {
  if (!c || !key || !value_out) return fail(CTPN_ERR_ARG, "ctpn_get_option: null pointer");
  const Option* o = find_option(key);
  if (!o) return fail(CTPN_ERR_ARG, std::string("ctpn_get_option: unknown option ") + key);
  *value_out = c->*(o->member);
  return CTPN_OK;
}

// ---- the detection tail's parameters: doubles by name, ctpn_set_option's contract ----
int ctpn_set_param(ctpn_ctx* c, const char* name, double value) {
  if (!c || !name) return fail(CTPN_ERR_ARG, "ctpn_set_param: null pointer");
  const int idx = tail_param_index(name);
  if (idx < 0) return fail(CTPN_ERR_ARG, std::string("ctpn_set_param: unknown parameter ") + name);
  // RPN_POST_NMS_TOP_N: 1 .. the ctx's proposal capacity (1000 on a fresh ctx, the table's bound; ctpn_reserve_proposals raises it)
  const bool ok = idx == TP_RPN_POST_NMS_TOP_N ? (value >= 1.0 && value <= (double)c->post_max && value == std::floor(value)) : tail_param_ok(idx, value);
  if (!ok) return fail(CTPN_ERR_ARG, std::string("ctpn_set_param: value out of range for ") + name);
  if (c->tail_raw[idx] == value) return CTPN_OK;
  // the queued tail reads these (and lays its buffers out by RPN_POST_NMS_TOP_N): drain first
  CTPN_HIP_TRY(hipSetDevice(c->device));
  CTPN_HIP_TRY(sync_forwards(c));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));
  for (auto& sl : c->slot) if (sl.busy) return fail(CTPN_ERR_STATE, "ctpn_set_param: a submitted batch has not been collected");
  for (auto& f : c->fs) f.tail_pending = false;
  c->nms_mw_dirty = true;
  c->tail_raw[idx] = value;
  switch (idx) {
    case TP_RPN_PRE_NMS_TOP_N: c->rpn_pre = (int)value; break;
    case TP_RPN_POST_NMS_TOP_N: c->rpn_post = (int)value; break;
    case TP_RPN_NMS_THRESH: c->rpn_nms_thresh = (float)value; break;
    case TP_RPN_MIN_SIZE: c->rpn_min_size = (float)value; break;
    default: connector_cfg_set(c->conn, idx, value); break;
  }
  return CTPN_OK;
}
// ---- the proposal capacity: ctpn_set_option's contract ----
int ctpn_reserve_proposals(ctpn_ctx* c, int post_capacity) {
  if (!c) return fail(CTPN_ERR_ARG, "ctpn_reserve_proposals: null ctx");
  if (post_capacity < 1000 || post_capacity > CTPN_POST_NMS_CAPACITY_MAX) return fail(CTPN_ERR_ARG, "ctpn_reserve_proposals: post_capacity must be in 1000.." + std::to_string(CTPN_POST_NMS_CAPACITY_MAX));
  if (post_capacity < c->rpn_post) return fail(CTPN_ERR_ARG, "ctpn_reserve_proposals: post_capacity is below the ctx's RPN_POST_NMS_TOP_N (" + std::to_string(c->rpn_post) + "); lower the parameter first");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  CTPN_HIP_TRY(sync_forwards(c));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));
  for (auto& sl : c->slot) if (sl.busy) return fail(CTPN_ERR_STATE, "ctpn_reserve_proposals: a submitted batch has not been collected");
  if (post_capacity == c->post_max) return CTPN_OK;
  TailSet t;
  int rc;
  if ((rc = tail_alloc(c->max_batch, post_capacity, t))) {      // (t dies here: the ctx is as it was)
    (void)hipGetLastError();
    return fail(rc, std::string("ctpn_reserve_proposals: ") + ctpn_last_error());
  }
  for (auto& f : c->fs) f.tail_pending = false;
  c->nms_mw_dirty = true;
  return tail_adopt(c, post_capacity, t);
}
int ctpn_proposal_capacity(ctpn_ctx* c, int* rows_out) {
  if (!c || !rows_out) return fail(CTPN_ERR_ARG, "ctpn_proposal_capacity: null pointer");
  *rows_out = c->post_max;
  return CTPN_OK;
}

int ctpn_get_param(ctpn_ctx* c, const char* name, double* value_out) {
  if (!c || !name || !value_out) return fail(CTPN_ERR_ARG, "ctpn_get_param: null pointer");
  const int idx = tail_param_index(name);
  if (idx < 0) return fail(CTPN_ERR_ARG, std::string("ctpn_get_param: unknown parameter ") + name);
  *value_out = c->tail_raw[idx];
  return CTPN_OK;
}

int ctpn_host_threads(ctpn_ctx* c, int* threads_out) {
  if (!c || !threads_out) return fail(CTPN_ERR_ARG, "null pointer");
  *threads_out = c->host_threads;
  return CTPN_OK;
}

int ctpn_destroy(ctpn_ctx* c) {
  if (!c) return CTPN_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->fs[1].stream) (void)hipStreamSynchronize(c->fs[1].stream);
  if (c->stream_p) (void)hipStreamSynchronize(c->stream_p);
  if (c->stream_c) (void)hipStreamSynchronize(c->stream_c);
  // everything is idle: the members release what they own, in reverse declaration order (the host pool first, see ctx.h)
  delete c;
  return CTPN_OK;
}

int ctpn_sync(ctpn_ctx* c) {
  if (!c) return fail(CTPN_ERR_ARG, "null ctx");
  CTPN_HIP_TRY(sync_forwards(c));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));
  if (c->stream_c) CTPN_HIP_TRY(hipStreamSynchronize(c->stream_c));      // staged copies, ctpn_decode_jpeg_batch
  return CTPN_OK;
}
int ctpn_stream(ctpn_ctx* c, void** stream_out) {
  if (!c || !stream_out) return fail(CTPN_ERR_ARG, "null pointer");
  *stream_out = (void*)c->stream;
  return CTPN_OK;
}

int ctpn_profile_enable(ctpn_ctx* c, int on) {
  if (!c) return fail(CTPN_ERR_ARG, "null ctx");
  if (!on) { int rc = prof_drain(c); if (rc) return rc; }
  c->prof = on != 0;
  c->prof_mode = on == 2 ? 2 : 1;
  return CTPN_OK;
}
int ctpn_profile_reset(ctpn_ctx* c) {
  if (!c) return fail(CTPN_ERR_ARG, "null ctx");
  int rc = prof_drain(c);
  if (rc) return rc;
  for (int k = 0; k < CTPN_KIND_COUNT; ++k) { c->prof_ms[k] = 0; c->prof_n[k] = 0; c->prof_work[k] = 0; }
  return CTPN_OK;
}
int ctpn_profile_read(ctpn_ctx* c, int kind, double* ms, long long* launches, double* work) {
  if (!c) return fail(CTPN_ERR_ARG, "null ctx");
  if (kind < 0 || kind >= CTPN_KIND_COUNT) return fail(CTPN_ERR_ARG, "kind out of range");
  int rc = prof_drain(c);
  if (rc) return rc;
  if (ms) *ms = c->prof_ms[kind];
  if (launches) *launches = c->prof_n[kind];
  if (work) *work = c->prof_work[kind];
  return CTPN_OK;
}

}  // extern "C"
