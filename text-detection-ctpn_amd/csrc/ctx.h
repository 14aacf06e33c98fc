// Internal to the host units of libctpn_hip.so (api_*.hip): the context struct, the small types and inline helpers more than one of them
// uses, and the declarations of the few functions that cross them. The kernel units do not include this file; what they share with the host
// units is in common.h.
// Ownership: every device block, page-locked block, event and stream of a ctx is a member of one of owned.h's handle types (DevBuf,
// PinnedBuf, Event, Stream, or a vector of them) and dies with the ctx; ctpn_destroy drains the streams and deletes the ctx, nothing else.
// A raw pointer or raw handle among the members is a VIEW into such a block or an ALIAS of such a handle, and says so.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

#include <pthread.h>
#include <sched.h>

#include <dlfcn.h>

#include "common.h"
#include "owned.h"

namespace ctpn {

// ---------------------------------------------------------------------------------------------
// network description (reference lib/networks/VGGnet_test.py:20-43)
// ---------------------------------------------------------------------------------------------
struct ConvSpec { const char* name; int ci, co, level; int pool_after; };
static const ConvSpec kConvs[14] = {
    {"conv1_1", 3, 64, 0, 0},    {"conv1_2", 64, 64, 0, 1},   {"conv2_1", 64, 128, 1, 0},  {"conv2_2", 128, 128, 1, 1},
    {"conv3_1", 128, 256, 2, 0}, {"conv3_2", 256, 256, 2, 0}, {"conv3_3", 256, 256, 2, 1}, {"conv4_1", 256, 512, 3, 0},
    {"conv4_2", 512, 512, 3, 0}, {"conv4_3", 512, 512, 3, 1}, {"conv5_1", 512, 512, 4, 0}, {"conv5_2", 512, 512, 4, 0},
    {"conv5_3", 512, 512, 4, 0}, {"rpn_conv/3x3", 512, 512, 4, 0}};
static const char* kPoolNames[4] = {"pool1", "pool2", "pool3", "pool4"};

struct ProfRec { int kind; Event a, b; double work; int launches = 1; bool span = false; };      // span: see prof_drain (api_ctx.hip)

// ---------------------------------------------------------------------------------------------
// Host worker pool of one ctx: created once, sized by ctpn_host_thread_budget (cores of the node / ranks on the node).
// Runs the per-image host part of the connector (ctpn_detect_collect) and the staging copies of pageable host images.
// Before: up to hardware_concurrency() std::threads were created and joined per collect -- 256 per step on an 8-rank node.
// ---------------------------------------------------------------------------------------------
class HostPool {
 public:
  HostPool(int nthreads, int first_cpu) : n_(nthreads < 1 ? 1 : nthreads) {
    for (int t = 1; t < n_; ++t) {
      th_.emplace_back([this] { loop(); });
      if (first_cpu >= 0) pin(th_.back().native_handle(), first_cpu + t);
    }
  }
  ~HostPool() {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; ++gen_; }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  int size() const { return n_; }
  // fn(i) for every i in [0, n); returns when all are done. The calling thread works too. max_par bounds the parallelism.
  void run(int n, const std::function<void(int)>& fn, int max_par = 0) {
    if (n <= 0) return;
    const int par = std::min(n, max_par > 0 ? std::min(max_par, n_) : n_);
    if (par <= 1) { for (int i = 0; i < n; ++i) fn(i); return; }
    std::lock_guard<std::mutex> serial(run_mu_);
    {
      std::lock_guard<std::mutex> lk(mu_);
      fn_ = &fn; total_ = n; next_.store(0); done_.store(0); helpers_ = par - 1; ++gen_;
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return done_.load() >= total_ && active_ == 0; });
    helpers_ = 0;      // a worker that wakes up late must not join a finished job
    fn_ = nullptr;
  }

 private:
  static void pin(pthread_t h, int cpu) {
    cpu_set_t set; CPU_ZERO(&set);
    const unsigned ncpu = std::thread::hardware_concurrency();
    CPU_SET((int)(ncpu > 0 ? (unsigned)cpu % ncpu : (unsigned)cpu), &set);
    (void)pthread_setaffinity_np(h, sizeof(set), &set);
  }
  void work() {
    for (;;) {
      const int i = next_.fetch_add(1);
      if (i >= total_) break;
      (*fn_)(i);
      done_.fetch_add(1);
    }
  }
  void loop() {
    unsigned long long seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
        if (stop_) return;
        if (helpers_ <= 0) continue;
        --helpers_; ++active_;
      }
      work();
      { std::lock_guard<std::mutex> lk(mu_); --active_; }
      done_cv_.notify_all();
    }
  }
  const int n_;
  std::vector<std::thread> th_;
  std::mutex mu_, run_mu_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(int)>* fn_ = nullptr;
  int total_ = 0, helpers_ = 0, active_ = 0;
  std::atomic<int> next_{0}, done_{0};
  unsigned long long gen_ = 0;
  bool stop_ = false;
};

}  // namespace ctpn

using namespace ctpn;

struct ctpn_ctx {
  int device = 0;
  int max_batch = 0, max_h = 0, max_w = 0;
  DType prec = DType::BF16;
  int es = 2;                       // bytes per activation element (split precision: a (hi, lo) bf16 pair = 4)
  hipStream_t stream = nullptr;     // ALIAS of fs[0].stream (not owned): network forward, weights, the synchronous entry points
  Stream stream_p;                  // proposal layer + connector front end of the asynchronous detect path
  std::vector<DevBuf> allocs;       // the blocks of fixed size ctpn_create makes; the typed pointers below are views into them
  // asynchronous detect: two slots of pinned host buffers + events
  struct Slot {
    // the batch's results in ONE page-locked block, laid out like the device's out_pack: a single device-to-host copy per submit
    // (six copies before: ~30 us of host calls per batch, which at batch 1 is 4 % of the step on a slow host)
    PinnedBuf pack;
    float* tlb = nullptr; float* tls = nullptr; int* keep = nullptr; int* kcnt = nullptr; float* rois = nullptr; int* rcnt = nullptr;      // views into pack
    PinnedBuf im_info;             // float [n][3]
    PinnedBuf crecs, ccnt;         // device connector results: double [n][2 modes][conn_cap][9], int [n][3]
    Event ev_heads, ev_decoded, ev_done;
    int n = 0, h = 0, w = 0; bool busy = false;
    int set = 0;               // the forward set the batch in flight runs on
    std::vector<int> hts;      // pixel height of every image of the batch (a ragged submit: the caller's heights; else h): what the host connector clips to
  } slot[2];
  hipEvent_t ev_last_done = nullptr;     // ALIAS of a slot's ev_done (not owned): the whole proposal tail (stream_p) of the most recent submit
  // "tail_confine" (default 0; was 1 in split precision during round 6): forward k + 1 waits, BEHIND its conv1_1, for the proposal tail of batch k,
  // which then overlaps conv1_1 only. History: the reversed-batch test of round 6 found that a batch in flight could change another batch's bits --
  // the proposal NMS of batch k running beside the persistent conv kernels of batch k + 1 (in split precision by default timing, in bf16 as soon as
  // the NMS was delayed into conv3_x / conv4_x). This switch removed the CONDITION. The CAUSE was in the conv kernels: the last k-slice group's
  // fragment reads were in flight across the step barrier while the LDS-DMA behind it recycled the strip they read, ordered by latency only
  // (conv3x3_persistent.h, INVARIANT in conv3x3_p_kernel; profiles/r06_barrier_war.txt). Fixed there; the switch stays for A/B runs.
  int tail_confine = 0;
  // asynchronous detect, option tail_overlap = 1 (opt-in): the recurrent tail of batch k (BiLSTM + heads: 0.37 ms of latency-bound kernels
  // on 148 of 256 CUs) runs on stream_p, next to conv1_1 of batch k + 1 (HBM-write-bound) instead of in front of it. Measured, round 3,
  // same box: +0.6 % images/s (3420-3425 vs 3397-3405) -- side by side the BiLSTM takes 0.51-0.73 ms instead of 0.33 and conv1_1 0.60
  // instead of 0.46, and the proposal kernels, which start 0.8 ms later, now run under conv2_x (static persistent tiles) instead of
  // conv1_2 (dynamic tile claims): the conv stack loses 0.9 points of its roofline. Off by default.
  int tail_overlap = 0;

  // weights
  bool weights_loaded = false;
  float* arena = nullptr;            // fp32 copy of the flat arena
  float* w_first = nullptr;          // [27][64]
  void* w_first_frags = nullptr;     // conv1_1 as split-bf16 MFMA A fragments (bf16 mode), 12 KB
  // options (ctpn_set_option; per ctx, never read from the environment)
  int conv1_mfma = 2;                // "conv1_kernel" (16-bit modes): 2 = uint8 feed through the q-image (exact integer pixels x 16-bit weights, one MFMA term; conv1_1 inside
                                     // conv1_2's window stage where "conv1_fuse" allows), 1 = split-bf16 kernel for both feeds, 0 = VALU kernel
  // ctpn_decode_jpeg_batch: two sets of buffers (decode of batch k + 1 while batch k's forward reads its images), allocated on first use and
  // grown on demand; a grown buffer's predecessor is retired, not freed (a pointer handed out earlier stays valid until ctpn_destroy)
  struct JpegBufs {
    PinnedBuf coef_host, qt_host;      // page-locked: what the entropy decoders write (int16 coefficients, uint16 tables)
    DevBuf coef_dev, qt_dev, out_dev;
    PinnedBuf tab_host; DevBuf tab_dev;      // ctpn_decode_jpeg_batch_ragged: per-image descriptors (page-locked / device)
    // ctpn_pack_canvas / ctpn_decode_png_files_ragged (api_canvas_pack.hip): [descriptors(n) | host images at prefix-summed offsets, rows at pitch 3 w],
    // page-locked, and the device copy ONE transfer makes of it
    PinnedBuf src_host; DevBuf src_dev;
    int out_n = 0, out_h = 0, out_w = 0;                            // what out_dev holds
    Event ev_h2d, ev_ready, ev_consumed;
    bool h2d_valid = false, consumed_valid = false, ready_valid = false;
  } jpeg[2];
  DevBuf jpeg_planes;                // component planes between the two kernels (one set: the kernels of both buffers run on stream_c in order)
  DevBuf jpeg_raw;                   // the decoded batch at file size when a resize follows (one set, same reason)
  std::vector<DevBuf> jpeg_retired;  // device allocations replaced by larger ones
  int jpeg_flip = 0;
  bool jpeg_ready = false;
  // ctpn_decode_jpeg_batch_device / ctpn_jpeg_entropy_decode_device (device Huffman decode, jpeg_huff.hip): ONE set -- these calls read the
  // files' flag words back before they return, so nothing of theirs is in flight when the next one stages its batch
  struct JhWork {
    PinnedBuf stage_host; DevBuf stage_dev;      // page-locked block and its device copy: descriptors + tables + bytes
    DevBuf work_dev;                             // per file flags / rounds, per subsequence states / counts
    PinnedBuf res_host;                          // page-locked: what comes back (2 words per file)
  } jh;
  long long jh_stats[4] = {0, 0, 0, 0};      // ctpn_jpeg_entropy_device_stats
  // the output stage both writers share (api_out_stage.hip): ONE set of buffers -- every writer call returns when its files are coded, so
  // nothing of a call is in flight when the next one starts -- allocated on first use and grown to the largest batch seen
  struct StageBufs {
    DevBuf img_dev;            // the batch's pixels: staged host images, or the copy the outlines are drawn on
    DevBuf rs_dev;             // ... resized by 1 / scale
    DevBuf recs_dev, cnt_dev;  // the outlines' records (double) and counts (int)
    // ctpn_write_annotated_files_ragged (api_out_ragged.hip): [heights(n) | descriptors of the resized images], page-locked / device
    PinnedBuf rm_host; DevBuf rm_dev;
  } stage;
  // ctpn_encode_jpeg_batch / ctpn_write_annotated_files (api_jpeg_out.hip): ONE set of buffers, for the reason the stage's set is one
  struct EncBufs {
    DevBuf coef_dev; PinnedBuf coef_host;      // quantised coefficients (int16), both of one size; the host side is page-locked
    DevBuf qtab_dev; PinnedBuf qtab_host; int qtab_quality = 0;               // JencQ[2][64] of the quality last used
    Event ev_done;
    // the device-entropy form (jpeg_huff_enc.hip; ctpn_encode_jpeg_batch_device, ...): one device block for a launch group's descriptors,
    // result words, lengths, counts, unstuffed and stuffed streams; the code tables; page-locked: descriptors + result words, scan bytes
    DevBuf huff_dev;
    DevBuf huff_tab_dev;
    PinnedBuf huff_host;
    PinnedBuf scan_host;
    // images of mixed sizes (ctpn_encode_jpeg_mixed, ctpn_write_line_crops): the descriptor table with its prefix sums, page-locked / device
    PinnedBuf mix_host;
    DevBuf mix_dev;
  } enc;
  long long jhe_stats[4] = {0, 0, 0, 0};      // ctpn_jpeg_entropy_encode_device_stats
  // ctpn_encode_png_batch / ctpn_write_annotated_png_files (api_png_out.hip): ONE set of buffers, for the same reason, grown likewise
  struct PngEncBufs {
    DevBuf dev;                // descriptors, histograms, codes, result records, per-piece array, DEFLATE words
    PinnedBuf host;            // page-locked: descriptors, histograms, codes, result records
    PinnedBuf file_host;       // page-locked: the DEFLATE blocks, each behind room for its file's front
    Event ev_done;
  } pnge;
  long long pnge_stats[4] = {0, 0, 0, 0};      // ctpn_png_encode_device_stats
  // ctpn_crop_lines (api_crops.hip): ONE set of buffers, for the reason the writer's set is one (the call returns when its crops are
  // complete), allocated on first use and grown to the largest call seen
  struct CropBufs {
    DevBuf img_dev;            // staged host images
    DevBuf out_dev;            // the crops of a call whose output goes to the host
    DevBuf desc_dev;           // one descriptor per line (common.h CROP_DESC_BYTES)
    PinnedBuf desc_host;       // ... page-locked
    Event ev_done;
  } crop;
  int debug_nms = 0;                 // "debug_nms" (diagnostic, WRONG proposals): parts mask of the one-workgroup proposal NMS, see nms_columns_kernel
  int debug_hog = 0;                 // "debug_hog" (diagnostic, 0 .. 200000; see the launch in enqueue_proposals_impl for the two upper ranges): launch a kernel with the one-workgroup NMS's footprint (1024 threads, 84 KB of LDS, one
                                     // workgroup per image) that spins this many microseconds without memory traffic in front of the proposal NMS. Results are unaffected;
                                     // tools/r6_pipeline_race.py uses it to ask what about the tail disturbs the next batch's persistent split layers
  int nms_prefix = 1;                // "nms_prefix" (round 6): the column NMS of the proposal layer first looks at the 4096 best-scored candidates only; they hold the
                                     // 1000 survivors asked for unless fewer than a quarter survive (then a full pass follows). Same keep list by construction; 0 = always the full pass
  int split_edge = 1;                // "split_edge" (round 6): split precision sends ragged tile columns (W = 225 = 14 x 16 + 1, 113 = 7 x 16 + 1, 450 = 28 x 16 + 2,
                                     // 900 = 28 x 32 + 4) through conv3x3_edge_kernel's split form, like the 16-bit modes, instead of computing a padded tile column
                                     // (an eighth of conv4_1 / conv4_2). 0 = the padded column (ABI 9's arithmetic for those columns: other last bits)
  int conv_p64 = 1;                  // "conv_p64" (round 6): split precision's conv1_2 (Co = 64, no weights-in-registers kernel) through the persistent kernel's 64-channel
                                     // form: 3.56 ms instead of the non-persistent kernel's 4.53 at batch 32 (0 = that kernel, for A/B runs). It made a latent
                                     // race of the conv kernels frequent enough to find (see tail_confine)
  int conv1_fuse = 1;                // "conv1_fuse": with conv1_kernel = 2 and keep_acts = 0, compute conv1_1 inside conv1_2 (conv3x3_wr_kernel FUSE); 0 = stand-alone from the q-image (same bytes)
  size_t q_img_bytes = 0;            // the batch's q-image (common.h; FwdSet::q_img), 16-bit modes only
  int lstm_split = 0;                // "lstm_split": the recurrent product on split-bf16 MFMAs (fp32-class, |d| < 3e-5, 0.32 -> 0.16 ms). Default 1 in
                                     // the 16-bit modes and, since round 6, in split precision (set in create_impl), 0 in fp32 (exact-fp32 MFMA kernel)
  int nms_check = 0;                 // "nms_check": debug -- re-run the generic NMS kernel behind the column-decomposed one and fail on a mismatch
  float* b_conv[14] = {nullptr};     // fp32 biases
  void* wt_conv[14] = {nullptr};     // packed [Co][9*Ci] T (index 0 unused)
  void* wt_x = nullptr;              // [1024][512] T (split precision: [1024][hi(512) | hi(512) | lo(512)] bf16)
  size_t wx_row_bytes = 1024;        // bytes of one wt_x row
  void* wt_xf = nullptr;             // 16-bit modes: wt_x in lstm_pre_kernel's fragment-major order
  float* b_x = nullptr;              // [1024]
  float* wh = nullptr;               // [2][128][512]
  float* wt_fc = nullptr;            // [512][256]
  float* b_fc = nullptr;
  float* wt_h = nullptr;             // [64][512]
  float* b_h = nullptr;              // [64]
  float* wt_fold = nullptr;          // [64][256]: (lstm_o FC) x (heads) folded, bf16 throughput mode only
  float* b_fold = nullptr;           // [64]

  // A forward set: a forward's stream and everything a forward writes. Set 0 is allocated by ctpn_create; every
  // synchronous entry point uses it. Set 1 exists so that TWO submitted batches' forwards can be in flight at once: a forward is a chain of
  // 20 dependent launches, and one ordered stream leaves the CUs idle at every cross-stream wait, in every partial last round of a persistent
  // walk and beside the 148-workgroup recurrence; a second, independent chain on another hardware queue has workgroups ready for exactly those
  // CUs. It is allocated by the first submit that finds the other slot in flight (api_detect.hip: pick_set), holds only what the production
  // path stores (no full-resolution map of a pooled layer; conv1_1's map only once a forward needs it), and a ctx that cannot have it
  // (keep_acts, out of memory, per-stage profiling) keeps both slots on set 0: the single-stream order.
  // Weights, the image staging buffers and the proposal tail (stream_p, one set of buffers) are shared.
  struct FwdSet {
    Stream stream;
    // views into blocks of `allocs` (set 0: the ctx's); act_conv / act_pool point `front` bytes into theirs, see act_front_pixels
    void* q_img = nullptr;             // the batch's q-image (common.h), 16-bit modes only
    void* act_conv[14] = {nullptr};
    void* act_pool[4] = {nullptr};
    bool act_valid[14] = {true, true, true, true, true, true, true, true, true, true, true, true, true, true};
    float* xp = nullptr;        // [M5][1024]
    float* lstm_out = nullptr;  // [M5][256]
    float* fc_out = nullptr;    // [M5][512]
    float* heads = nullptr;     // [M5][64]
    bool fc_valid = true;
    DevBuf ragged_blob;                // fp32 / split precision: a ragged canvas as a float feed, 0.0f below the images
    int fwd_ragged = -1;               // the set's last forward was ragged: index of its RaggedSet (ctpn_proposals hands its feature rows to decode_kernel), else -1
    int n = 0, h = 0, w = 0;           // the set's last forward
    int gn = -1, gh = -1, gw = -1;     // geometry the set's borders are currently zeroed for
    // option tail_overlap: conv stack + lstm_pre of the set's batch in flight are done (stream -> stream_p); the tail of the set's most recent
    // forward is done (stream_p -> stream: before the set's next conv1_2 rewrites what it read)
    Event ev_conv, ev_tail;
    bool tail_pending = false;
    // the decode kernel (stream_p) that last read `heads`, which the set's next forward rewrites, and the slot whose submit recorded it
    hipEvent_t ev_decoded = nullptr; int dec_slot = -1;      // ALIAS of that slot's ev_decoded (not owned)
    Event ev_gate; bool gate_valid = false;      // two_forwards_mode() 2 / 3: the point of this set's forward the other set's conv stack waits for
    std::vector<DevBuf> allocs;        // set 1's blocks (set 0's are in the ctx's allocs, with everything else ctpn_create makes)
  } fs[2];
  size_t set1_bytes = 0;             // device bytes of set 1
  int set1_state = 0;                // 0: not asked for yet, 1: allocated, -1: could not be allocated (both slots stay on set 0)
  FwdSet* last = &fs[0];             // the set of the most recent forward: what ctpn_get_tensor, ctpn_proposals, ctpn_feat_shape read
  size_t act_conv_bytes[14] = {0};
  size_t act_pool_bytes[4] = {0};
  uint8_t* img_dev = nullptr;        // staging of host images, buffer 0 (views into allocs, like the weights above)
  uint8_t* img_dev_b[2] = {nullptr, nullptr};   // ... double-buffered: batch k+1 crosses PCIe on stream_c while batch k is on the convolutions
  Stream stream_c;
  Event ev_copied[2], ev_consumed[2];
  bool consumed_valid[2] = {false, false};
  PinnedBuf pin_stage[2];            // page-locked staging for pageable caller buffers (lazily allocated)
  Event ev_h2d_done[2];
  bool h2d_valid[2] = {false, false};
  int img_flip = 0;
  float* cls_prob = nullptr;  // [M5][20]
  float* bbox_pred = nullptr; // [M5][40]
  size_t m5_max = 0;

  // proposal buffers
  // post_max: the ctx's proposal capacity -- rows per image of everything the tail lays out by RPN_POST_NMS_TOP_N, and of rois_out / keep_out /
  // anchors_out towards the caller. 1000 on a fresh ctx; ctpn_reserve_proposals (api_ctx.hip) replaces the blocks of `tail` and the slots' pack /
  // crecs by larger ones. conn_cap = post_max / 2: lines per image and mode the device connector returns (a chain has two proposals at least)
  int npad_max = 0, topn_max = 12000, post_max = 1000, conn_cap = 500;
  struct TailBufs { DevBuf out_pack, roi_anchor, tl_spill, conn_recs, conn_scratch, conn_work; } tail;      // the views below point into these
  unsigned long long* keys = nullptr; unsigned long long* keys_tmp = nullptr;
  float* boxes4 = nullptr;
  float* sorted_boxes = nullptr;
  float* sorted_scores = nullptr;
  int* valid_counts = nullptr;
  int* keep_idx = nullptr;
  int* keep_counts = nullptr;
  float* rois = nullptr;
  float* kept_spill = nullptr;
  int* sorted_anchor = nullptr;      // [n][12000] anchor index of every sorted row
  int* roi_anchor = nullptr;         // [n][post_max]  anchor index of every roi (second return of proposal_layer)
  int last_post = 0, last_prop_n = 0;
  ProposalPlan last_plan{}; int last_hf = 0, last_wf = 0, last_pre = 0;      // the last proposals call, for ctpn_debug_proposal_fetch
  float* im_info_dev = nullptr;
  char* out_pack = nullptr; size_t pack_bytes = 0;      // tl_boxes, tl_scores, tl_keep, tl_keep_counts, rois, keep_counts live here (pack_layout)
  float* tl_boxes = nullptr; float* tl_scores = nullptr; int* tl_counts = nullptr;  // connector front end
  int* tl_keep = nullptr; int* tl_keep_counts = nullptr; float* tl_spill = nullptr;
  double* conn_recs = nullptr; int* conn_counts = nullptr; double* conn_scratch = nullptr;   // device connector (connect_kernel)
  char* conn_work = nullptr;         // ... its large form's state (connect_large_kernel), null up to 1024 rows
  int nms_columns = 1;               // "nms_columns": 1 = column-decomposed NMS (one workgroup per image; batches <= NMS_MW_MAX_BATCH: one column per
                                     // wave over ncols / 4 workgroups per image), 0 = nms_kernel (A/B), 2 / 3 = force the one-workgroup / the multi-workgroup form
  char* nms_mw_scratch = nullptr;    // NMS_MW_CAP_BATCH x NMS_MW_SCRATCH_BYTES
  bool nms_mw_dirty = false;         // the scratch may not be in its zero state (an error between launches, an option change): memset before the next use
  unsigned char* nms_colid = nullptr;  // NMS_MW_CAP_BATCH x (topn_max rounded up to 16): column group of every sorted box (gather_kernel)
  int connect_device = 0;            // "connect_device": 1 = graph build / chains / line fit on the GPU (connect_kernel), 0 = host C++
                                     // (text_connector.cpp; default: it runs on otherwise idle host cores under the next batch's convolutions,
                                     // the kernel shares the GPU with them: 11.15 vs 11.06 ms / step)
  // the detection tail's parameters (ctpn_set_param; defaults: cfg.TEST.RPN_* and TextLineCfg of the reference), read by ctpn_detect*,
  // ctpn_debug_text_lines and the collect's host connector. tail_raw: the values as set (ctpn_get_param returns them); the typed members
  // beside it: what the launches use, converted once at set time. The tail's device buffers and the slots' packs are laid out with
  // stride rpn_post (<= post_max) per image; ctpn_detect_collect / ctpn_debug_text_lines keep post_max rows per image towards the caller.
  double tail_raw[TAIL_PARAM_COUNT];
  int rpn_pre = 12000, rpn_post = 1000;
  float rpn_nms_thresh = 0.7f, rpn_min_size = 8.0f;
  ConnectorCfg conn = default_connector_cfg();
  bool proposals_done = false;
  bool postproc_only = false;        // ctpn_create_postproc: proposal / connector buffers only, no network
  int host_threads = 1;
  int keep_acts = 0;      // "keep_acts": 1 = also store the full-resolution output of pool-fused convs, keep lstm_o (layer-wise parity)
  float* cls_in = nullptr;  // staging for proposals_from_host
  float* bbox_in = nullptr;

  // ragged batches (ctpn_forward_ragged, ctpn_detect_submit_ragged; ragged.hip): a batch's heights reach the device once per call, through a small
  // page-locked array, as [heights(n) | feature rows(n)]. One set per detect slot and one for ctpn_forward_ragged (index 2): a slot's
  // decode kernel reads its set on stream_p while the next submit's forward already copies the other slot's. Allocated on the first ragged call.
  struct RaggedSet {
    PinnedBuf host; DevBuf dev;      // int [heights(n) | feature rows(n)]
    Event ev_copied; bool copied_valid = false;      // the copy that last read `host`
  } ragged[3];

  bool forward_done = false;

  // profiling
  bool prof = false;
  int prof_mode = 1;                 // 1: a pair of events around every stage (both slots then stay on forward set 0); 2: ONE pair around the 13 conv3x3
                                     // launches of a forward only (an event pair per launch costs ~0.2 ms of bubbles per step, which a throughput run
                                     // should not pay); conv_gemm's time is then the length of the UNION of the forwards' intervals (prof_drain)
  std::vector<ProfRec> pending;      // owning; Timed hands out the raw handles
  std::vector<Event> free_events;
  double prof_ms[CTPN_KIND_COUNT] = {0};
  long long prof_n[CTPN_KIND_COUNT] = {0};
  double prof_work[CTPN_KIND_COUNT] = {0};

  // LAST member, so the first to die: the pool's threads are joined before any block above goes away. The pool is idle between calls
  // (HostPool::run returns when its job is done), so this is a matter of order only.
  std::unique_ptr<ctpn::HostPool> pool;
};

namespace ctpn {

static inline DType prec_dtype(int precision) {
  return precision == CTPN_PREC_FP32 ? DType::F32 : precision == CTPN_PREC_FP16 ? DType::F16 : precision == CTPN_PREC_SPLIT ? DType::SPLIT : DType::BF16;
}

static inline int lvl(int v, int level) { for (int i = 0; i < level; ++i) v /= 2; return v; }
// Slack around every activation buffer: the conv kernels fetch input windows without clamping (conv3x3.hip). Behind the last image:
// 2D tiles read up to 17 (+ 8: half items of the tail round) bordered rows + one window row past it (16 x 16 patches), flat mode's last tile a whole window
// (256 + 2 (W + 2) + 2 pixels); in front of the first: flat mode's first tile starts one bordered row + 1 pixel early.
static inline size_t act_slack_pixels(int w) { return (size_t)28 * (w + 2) + 384; }    // behind (+ 8 rows: the second half of a split tail tile)
static inline size_t act_front_pixels(int w) { return (size_t)(w + 2) + 64; }          // in front

// the column NMS of a small batch spreads its columns over the machine (nms.hip: nms_column_groups_kernel); option nms_columns = 2 / 3
// pins one form for A/B runs and the tests
// hf: rows of the feature map (a column holds hf x 10 candidates at most, the kernel's list 1024), 0 for the connector's <= 1024 boxes
static inline bool nms_multi_wg(const ctpn_ctx* c, int n, int hf) {
  return nms_multi_wg_ok(c->nms_mw_scratch != nullptr, c->nms_columns, n, hf);
}

// CTPN_DEBUG_SYNC / CTPN_ROCTX: read once per process (api_ctx.hip)
int debug_sync();
struct RoctxApi { int (*push)(const char*) = nullptr; int (*pop)() = nullptr; };
const RoctxApi& roctx_api();
int roctx_on();
static const char* kKindNames[CTPN_KIND_COUNT + 1] = {"ctpn:conv_first", "ctpn:conv_gemm", "ctpn:pool", "ctpn:gemm", "ctpn:bilstm",
                                                     "ctpn:decode", "ctpn:sort", "ctpn:nms", "ctpn:conv_stack"};
// a timed event for a profiler pair: a recycled one if there is one. Where the creation fails the event stays null, hipEventElapsedTime refuses
// it and prof_drain drops that record; a null event that comes back through free_events is created here the next time
static inline Event prof_event(ctpn_ctx* c) {
  Event e;
  if (!c->free_events.empty()) { e = std::move(c->free_events.back()); c->free_events.pop_back(); }
  (void)e.ensure_timed();
  return e;
}
struct Timed {
  ctpn_ctx* c; int kind; double work; Event a, b; bool on; hipStream_t st;
  Timed(ctpn_ctx* c_, int kind_, double work_, hipStream_t st_ = nullptr) : c(c_), kind(kind_), work(work_), on(c_->prof && (c_->prof_mode == 1 || kind_ == CTPN_KIND_COUNT)), st(st_ ? st_ : c_->stream) {
    if (debug_sync()) { fprintf(stderr, "[ctpn] launch kind %d work %.3g\n", kind, work); fflush(stderr); }
    // CTPN_ROCTX=1: a roctx range around the enqueue of every stage (rocprofv3 --marker-trace shows them next to the kernels;
    // the reference's only instrumentation is the wall-clock Timer of ctpn/demo.py:56-66)
    if (roctx_on()) (void)roctx_api().push(kKindNames[kind]);
    if (!on) return;
    a = prof_event(c); b = prof_event(c);
    (void)hipEventRecord(a, st);
  }
  ~Timed() {
    if (roctx_on()) (void)roctx_api().pop();
    if (debug_sync()) { hipError_t e = hipStreamSynchronize(st); fprintf(stderr, "[ctpn]   done kind %d: %s\n", kind, hipGetErrorString(e)); fflush(stderr); }
    if (!on) return;
    (void)hipEventRecord(b, st);
    c->pending.push_back({kind, std::move(a), std::move(b), work});
  }
};

// the network forward (api_forward.hip); tail_on_p: the recurrent tail runs on stream_p (option tail_overlap)
// heights (nullable): a ragged batch -- h is the canvas height, image i is rows [0, heights[i]) of its slot; rset: which of the ctx's RaggedSets
// carries them to the device. Heights that all equal h take the uniform path.
// f: the forward set it runs on and writes (the only one it touches). beside: another set's forward is in flight (its conv stack is then
// gated behind that one's, see two_forwards_mode)
int forward_impl(ctpn_ctx* c, ctpn_ctx::FwdSet& f, const void* images, int is_f32, int images_on_device, int n, int h, int w, bool tail_on_p = false,
                 const int* heights = nullptr, int rset = 2, bool beside = false);
// whether that forward computes conv1_1 inside conv1_2's window stage, i.e. never stores conv1_1's map (heights: nullable, as above)
bool forward_fuses_conv1(const ctpn_ctx* c, int is_f32, int n, int h, int w, const int* heights);
int two_forwards_mode();      // api_ctx.hip: 2 in the product library
// forward set 1 (api_ctx.hip), allocated on first call; need_conv1: with room for conv1_1's map. false: the caller stays on set 0
bool ensure_set1(ctpn_ctx* c, bool need_conv1);
// both forward streams drained (set 1's exists once the set does)
static inline hipError_t sync_forwards(ctpn_ctx* c) {
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess || !c->fs[1].stream.get()) return e;
  return hipStreamSynchronize(c->fs[1].stream);
}
// the proposal layer in stream order on s (api_proposals.hip; null: the forward's stream); ev_decoded is recorded behind the decode kernel
int enqueue_proposals(ctpn_ctx* c, const float* heads, int heads_are_probs, int n, int hf, int wf, const float* im_info,
                      int pre_nms_topn, int post_nms_topn, float nms_thresh, float min_size, hipStream_t s = nullptr,
                      hipEvent_t ev_decoded = nullptr, const int* valid_rows_dev = nullptr /* ragged batch: feature rows per image */);
// option nms_check behind a column-decomposed NMS launch on s (api_proposals.hip): the generic kernel on the same candidates must give keep1 / cnt1
int nms_check_generic(ctpn_ctx* c, const float* boxes, const float* scores, const int* counts, int stride, float thresh, int post_topn,
                      const int* keep1, int keep_stride, const int* cnt1, int n, bool mw, hipStream_t s, const char* what);
// the output stage of the writers and the crops (api_out_stage.hip). stage_pixels: a call's pixels where its kernels on qs may read them --
// host images copied into buf (ctx-owned, grown to bytes + slack), device images in place, behind a live ctpn_decode_jpeg_batch batch's event
int wait_live_batch(ctpn_ctx* c, const uint8_t* images_dev, hipStream_t qs);      // qs waits for the decode that produced images_dev, if it is a live batch or canvas
int stage_pixels(ctpn_ctx* c, const uint8_t* images, int on_device, size_t bytes, size_t slack, DevBuf& buf, hipStream_t qs, const uint8_t*& px);
// the ctpn_write_annotated_* entry points up to the file format: their argument checks (format: "JPEG" or "PNG", for the message; size_check,
// nullable: the format's own check of both sizes), then the ctx's copy of the images, outlines drawn, resized by 1 / scale, at px (dh x dw)
typedef int (*StageSizeCheck)(const std::string& who, int h, int w);
int annotate_batch(ctpn_ctx* c, const std::string& who, const char* format, StageSizeCheck size_check, const uint8_t* images, int on_device, int n, int h, int w, const double* recs,
                   int line_capacity, const int* line_counts, double scale, const char* const* paths, const uint8_t*& px, int& dh, int& dw);
// a finished file onto the disk (on worker threads: nothing may leave it; st, msg: why it failed); the report of a call's first failed image
void write_file(const char* path, const uint8_t* data, size_t bytes, int& st, std::string& msg);
int first_failure(const char* who, const std::vector<int>& st, const std::vector<std::string>& msg);
// api_jpeg_out.hip: n BGR images of mixed sizes (each 1 .. 65535, pitches[i] >= 3 widths[i], both checked by the caller) at offsets[i] bytes of
// px_dev, device memory the copy queue may read as it stands -> JPEG files at `quality`, in caller memory (out / capacities / bytes_out) or
// on disk (paths); returns when they are written. The contract of ctpn_encode_jpeg_mixed behind its argument checks
int encode_mixed_dev(ctpn_ctx* c, const char* who, const uint8_t* px_dev, int n, const int* heights, const int* widths, const size_t* pitches, const size_t* offsets,
                     int quality, uint8_t* const* out, const size_t* capacities, size_t* bytes_out, const char* const* paths, bool device_entropy);
// api_png_out.hip: the PNG writer's table form, encode_mixed_dev's counterpart (ctpn_encode_png_mixed behind its argument checks). The source
// is read byte-wise: nothing outside an image's pixels is touched, at any pitch or alignment. png_table_check: the device form's bounds
// on a table -- sizes 1 .. 65535, h (1 + 3 w) <= 2^27 per image, at most 2^31 - 1 work items, fewer than 2^32 pieces --, host arithmetic
// only, naming the image; png_code_table runs it first, a caller with device work in front of the coder runs it before that
int png_table_check(const std::string& who, int n, const int* heights, const int* widths);
int png_code_table(ctpn_ctx* c, const char* who, const uint8_t* px, int n, const int* heights, const int* widths, const size_t* pitches, const size_t* offsets, uint8_t* const* out,
                   const size_t* capacities, size_t* bytes_out, const char* const* paths);
// api_out_ragged.hip: the pixel stage of the annotated writers over a ragged canvas, both formats'. Argument checks (format: "JPEG" or "PNG",
// for the message; table_check, nullable: the format's own check of the written sizes, before any device work), then the canvas copied
// into the ctx's buffer, outlines drawn per slot, every image resized by its own 1 / scales[i]: image i is dh[i] x dw[i] at
// px + offsets[i], rows pitches[i] bytes apart
typedef int (*StageTableCheck)(const std::string& who, int n, const int* heights, const int* widths);
int annotate_ragged(ctpn_ctx* c, const std::string& who, const char* format, StageTableCheck table_check, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w,
                    const int* heights, const double* recs, int line_capacity, const int* line_counts, const double* scales, const char* const* paths, const uint8_t*& px,
                    std::vector<int>& dh, std::vector<int>& dw, std::vector<size_t>& pitches, std::vector<size_t>& offsets);
int jpeg_sets_ready(ctpn_ctx* c);      // api_jpeg_decode.hip: the events of the two decode buffer sets (c->jpeg) exist; the decode and the pack calls take the sets in turn
bool jpeg_read_file(const char* path, std::vector<uint8_t>& buf, size_t limit = 0);      // api_input.hip: a whole file (limit: its first bytes only); false if it cannot be read
void jpeg_layout8(const JpegGeom& g, int* layout8);                                      // api_input.hip: the eight ints ctpn_jpeg_entropy_decode describes a file's layout with

}  // namespace ctpn
