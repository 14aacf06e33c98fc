// C ABI of libctpn_hip.so, JPEG decode unit: files -> device images. The buffer sets, the device-Huffman staging loop (kernels: jpeg_huff.hip),
// ONE decode pipeline for the uniform and the ragged calls (pixel kernels: jpeg.hip, jpeg_ragged.hip; resize: preprocess.hip), the fetch.
#include "ctx.h"
#include "jpeg_ragged_dev.h"      // JrImage: the ragged decode's per-image descriptor

namespace ctpn {

// coef_total: int16 elements of the call's coefficient blocks (n x one capacity, or the sum of the files' own); tab: the ragged call's
// descriptor table too
int jpeg_sets_ready(ctpn_ctx* c) {
  if (c->jpeg_ready) return CTPN_OK;
  int rc;
  for (auto& j : c->jpeg)
    for (Event* e : {&j.ev_h2d, &j.ev_ready, &j.ev_consumed}) if ((rc = e->ensure())) return rc;
  c->jpeg_ready = true;
  return CTPN_OK;
}

static int jpeg_reserve(ctpn_ctx* c, ctpn_ctx::JpegBufs& J, size_t n, size_t coef_total, size_t raw_bytes, size_t out_bytes, bool tab) {
  if (const int rc = jpeg_sets_ready(c)) return rc;
  // a device block that grows is retired, not freed: work in flight may still read it, and the caller may hold a pointer into it
  std::vector<DevBuf>& old = c->jpeg_retired;
  // a page-locked block and its device twin (the copy that last read the page-locked block has been waited for by the caller)
  auto pair = [&](PinnedBuf& host, DevBuf& dev, size_t bytes) { const int rc = host.grow(bytes); return rc ? rc : dev.grow_retiring(bytes, old); };
  int rc;
  if ((rc = pair(J.coef_host, J.coef_dev, coef_total * sizeof(int16_t)))) return rc;
  if (tab && (rc = pair(J.tab_host, J.tab_dev, n * sizeof(JrImage)))) return rc;
  if ((rc = pair(J.qt_host, J.qt_dev, n * 192 * sizeof(uint16_t)))) return rc;
  if ((rc = J.out_dev.grow_retiring(out_bytes + 256, old))) return rc;
  if ((rc = c->jpeg_planes.grow_retiring(coef_total, old))) return rc;      // one byte per coefficient
  if (raw_bytes && (rc = c->jpeg_raw.grow_retiring(raw_bytes + 256, old))) return rc;
  return CTPN_OK;
}

// ---- device Huffman decode (jpeg_huff.hip): staging, the bounded round loop, the flag words ----
static inline size_t jh_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Decode files use[0 .. m) (indices into P / data / len; all prepared without error) into coef_dev, file use[j] at int16 offset coef_base[use[j]]
// (the caller made coef_dev large enough; coef_zero_elems of it are cleared first). One page-locked block -- descriptors, tables, segment and
// subsequence tables, unstuffed bytes -- crosses in ONE copy; the host's share is one linear pass per file, on the worker pool. Returns when
// the files' flag words are back: flags_out[use[j]] = 0 means file use[j]'s coefficients stand in coef_dev (complete as far as queue qs is
// concerned), anything else that the host half has to decode that file. Updates the ctx's stats.
static int jh_decode(ctpn_ctx* c, const uint8_t* const* data, const size_t* len, std::vector<JhPrep>& P, const std::vector<int>& use, uint32_t S,
                     int16_t* coef_dev, const std::vector<long long>& coef_base, size_t coef_zero_elems, hipStream_t qs, std::vector<uint32_t>& flags_out) {
  auto& W = c->jh;
  const uint32_t WG = (uint32_t)jpeg_huff_workgroup();
  std::vector<int> dev;                    // the files that go to the device
  for (int i : use) {
    if (len[i] - P[i].scan >= ((size_t)1 << 28)) flags_out[i] = JH_FLAG_SEGMENTS;      // bit positions are 32-bit: such a scan is the host half's
    else dev.push_back(i);
  }
  const size_t m = dev.size();
  long long handed = 0;
  for (int i : use) if (flags_out[i]) ++handed;
  c->jh_stats[0] = 0; c->jh_stats[1] = handed; c->jh_stats[2] = 0; c->jh_stats[3] = 0;
  if (!m) return CTPN_OK;
  // layout of the staged block (upper bounds: the unstuffed bytes are at most the scan's bytes)
  size_t nseg = 0, ntab = 0, nbytes = 0, nsub_bound = 0;
  std::vector<size_t> byte_off(m), seg_off(m), tab_off(m);
  for (size_t j = 0; j < m; ++j) {
    const JhPrep& p = P[dev[j]];
    const size_t raw = len[dev[j]] - p.scan;
    seg_off[j] = nseg; tab_off[j] = ntab; byte_off[j] = nbytes;
    nseg += p.nseg; ntab += (size_t)p.ntab; nbytes += jh_up(raw, 4) + 8;
    nsub_bound += jh_up((raw * 8 + S - 1) / S + p.nseg, WG);
  }
  if (nsub_bound > 0x7fffffffu || nbytes > 0xfffffff0u || nseg > 0x2fffffffu) return fail(CTPN_ERR_CAPACITY, "jpeg_huff: batch too large");
  const size_t o_files = 0, o_segs = jh_up(o_files + m * sizeof(JhFile), 16), o_tabs = jh_up(o_segs + nseg * sizeof(JhSeg), 16),
               o_bytes = jh_up(o_tabs + ntab * sizeof(JhTable), 16), o_wg = jh_up(o_bytes + nbytes, 16), o_sub = o_wg + nsub_bound / WG * 4,
               stage_bound = o_sub + nsub_bound * 4;
  int rc;
  // each block of the pair is tested on its own: where one grew and its twin could not, the next call tries the twin again
  const size_t stage_want = stage_bound + stage_bound / 4;
  if (stage_bound > W.stage_host.bytes() && (rc = W.stage_host.grow(stage_want))) return rc;
  if (stage_bound > W.stage_dev.bytes() && (rc = W.stage_dev.grow(stage_want))) return rc;
  const size_t w_res = 0, w_st0 = jh_up(2 * m * 4, 16), w_st1 = w_st0 + nsub_bound * 8, w_entry = w_st1 + nsub_bound * 8, w_begun = w_entry + nsub_bound * 8,
               w_prefix = w_begun + nsub_bound * 4, work_bound = w_prefix + nsub_bound * 4;
  if (work_bound > W.work_dev.bytes() && (rc = W.work_dev.grow(work_bound + work_bound / 4))) return rc;
  if ((2 * m) * 4 > W.res_host.bytes() && (rc = W.res_host.grow(2 * m * 4 + 256))) return rc;
  uint8_t* H = W.stage_host.as<uint8_t>();
  uint32_t* res = W.res_host.as<uint32_t>();
  JhFile* hf = (JhFile*)(H + o_files); JhSeg* hs = (JhSeg*)(H + o_segs); JhTable* ht = (JhTable*)(H + o_tabs);
  uint32_t* hwg = (uint32_t*)(H + o_wg); uint32_t* hsub = (uint32_t*)(H + o_sub);
  // the linear pass: one file per worker
  std::vector<int> found(m, 0);
  c->pool->run((int)m, [&](int j) {
    const int i = dev[j];
    const JhPrep& p = P[i];
    uint8_t* dst = H + o_bytes + byte_off[j];
    const size_t raw = len[i] - p.scan;
    uint32_t nb = 0;
    found[j] = jh_unstuff_segments(data[i] + p.scan, raw, p.dri, p.total_mcus, dst, hs + seg_off[j], (int)p.nseg, &nb);
    std::memset(dst + nb, 0, jh_up(raw, 4) + 8 - nb);
    for (uint32_t k = (uint32_t)found[j]; k < p.nseg; ++k) {      // segments the file does not have: empty, so the decode flags them
      JhSeg& sg = hs[seg_off[j] + k];
      sg.byte0 = nb; sg.nbits = 0; sg.mcu0 = k * p.dri; sg.nmcu = std::min(p.dri, p.total_mcus - sg.mcu0);
      sg.sub0 = sg.nsub = sg.file = sg.pad_ = 0;
    }
    JhFile& F = hf[j];
    F = p.file;
    F.coef_base = coef_base[i];
    F.bytes_off = (uint32_t)byte_off[j]; F.nwords = (uint32_t)((jh_up(nb, 4) + 8) / 4);
    F.seg0 = (uint32_t)seg_off[j]; F.nseg = p.nseg; F.tab0 = (uint32_t)tab_off[j]; F.ntab = (uint32_t)p.ntab;
    std::memcpy(ht + tab_off[j], p.tabs, (size_t)p.ntab * sizeof(JhTable));
  });
  // subsequences: every segment at least one, every file's padded to the workgroup size
  uint32_t nsub = 0, cap = 0;
  long long real_subs = 0;
  for (size_t j = 0; j < m; ++j) {
    const JhPrep& p = P[dev[j]];
    if ((uint32_t)found[j] < p.nseg) flags_out[dev[j]] |= JH_FLAG_SEGMENTS;
    for (uint32_t k = 0; k < p.nseg; ++k) {
      JhSeg& sg = hs[seg_off[j] + k];
      sg.file = (uint32_t)j; sg.sub0 = nsub; sg.nsub = std::max(1u, (sg.nbits + S - 1) / S);
      for (uint32_t q = 0; q < sg.nsub; ++q) hsub[nsub + q] = (uint32_t)(seg_off[j] + k);
      nsub += sg.nsub; real_subs += sg.nsub;
      cap = std::max(cap, sg.nsub - 1);
    }
    const uint32_t padded = (uint32_t)jh_up(nsub, WG);
    for (; nsub < padded; ++nsub) hsub[nsub] = 0xffffffffu;
  }
  if (nsub > nsub_bound) return fail(CTPN_ERR_STATE, "jpeg_huff: subsequence bound exceeded");
  for (uint32_t w = 0; w < nsub / WG; ++w) { const uint32_t si = hsub[(size_t)w * WG]; hwg[w] = si == 0xffffffffu ? 0xffffffffu : hs[si].file; }
  const size_t stage_used = o_sub + (size_t)nsub * 4;
  uint8_t* D = W.stage_dev.as<uint8_t>(); uint8_t* K = W.work_dev.as<uint8_t>();
  JhBatchDev B;
  B.files = (const JhFile*)(D + o_files); B.segs = (const JhSeg*)(D + o_segs); B.tabs = (const JhTable*)(D + o_tabs);
  B.wg_file = (const uint32_t*)(D + o_wg); B.sub_seg = (const uint32_t*)(D + o_sub); B.bytes = D + o_bytes;
  B.st[0] = (JhState*)(K + w_st0); B.st[1] = (JhState*)(K + w_st1); B.entry = (JhState*)(K + w_entry);
  B.begun = (uint32_t*)(K + w_begun); B.prefix = (uint32_t*)(K + w_prefix);
  B.flags = (uint32_t*)(K + w_res); B.changed = B.flags + m;
  B.coef = coef_dev; B.S = S; B.nsub = nsub; B.nseg = (uint32_t)nseg; B.nfiles = (uint32_t)m;
  CTPN_HIP_TRY(hipMemcpyAsync(D, H, stage_used, hipMemcpyHostToDevice, qs));
  CTPN_HIP_TRY(hipMemsetAsync(K + w_res, 0, 2 * m * 4, qs));
  if ((rc = launch_jpeg_huff_round(B, 0, qs))) return rc;
  // sync rounds: a fixed few, then one check with the results; a file still unsettled then (rare: its components share their tables, or S is
  // small against its blocks) gets four times as many, up to the cap -- after `subsequences in the longest segment - 1` rounds every state
  // is the true one, whatever the flags say
  uint32_t rounds = 0, target = std::min(cap, 6u);
  for (;;) {
    for (; rounds < target; ++rounds) if ((rc = launch_jpeg_huff_round(B, (int)rounds + 1, qs))) return rc;
    CTPN_HIP_TRY(hipMemsetAsync(K + w_res, 0, m * 4, qs));                       // the flag words (not the rounds)
    CTPN_HIP_TRY(hipMemsetAsync(coef_dev, 0, coef_zero_elems * sizeof(int16_t), qs));
    if ((rc = launch_jpeg_huff_write(B, (int)rounds, qs))) return rc;
    CTPN_HIP_TRY(hipMemcpyAsync(res, K + w_res, 2 * m * 4, hipMemcpyDeviceToHost, qs));
    CTPN_HIP_TRY(hipStreamSynchronize(qs));
    bool unsettled = false;
    if (rounds < cap) for (size_t j = 0; j < m; ++j) if (res[m + j] >= rounds && rounds > 0) unsettled = true;
    if (!unsettled) break;
    target = (uint32_t)std::min<unsigned long long>(cap, (unsigned long long)rounds * 4);
  }
  long long ok = 0;
  for (size_t j = 0; j < m; ++j) {
    flags_out[dev[j]] |= res[j];
    if (flags_out[dev[j]]) ++handed; else ++ok;
  }
  c->jh_stats[0] = ok; c->jh_stats[1] = handed; c->jh_stats[2] = real_subs; c->jh_stats[3] = rounds;
  return CTPN_OK;
}

// one image's bytes for the host half: from the caller's memory, or read from the file inside the worker thread
struct JpegSource {
  const uint8_t* const* mem = nullptr; const size_t* sizes = nullptr;
  const char* const* paths = nullptr;
};

// One decode call, uniform or ragged. A call checks its arguments, describes itself in the fields of the first group and runs the stages in
// order: begin, its own geometry checks (and whatever of the description waits for the files' geometry), upload, its pixel launch on qs,
// publish. The stages own the two buffer sets' protocol -- ev_h2d, ev_consumed, ev_ready, the flip -- and the flagged-file fallback.
struct JpegDecode {
  ctpn_ctx* c;
  std::string who;                       // "<entry point>: ", in front of every message
  JpegSource src;
  int n;
  bool dev_entropy;                      // the Huffman decode on the device too (jpeg_huff.hip); everything from the coefficients on is shared
  // per file: the coefficients' capacity, their int16 offset in coef_host and in coef_dev (the latter may wait for begin()'s geometry)
  std::vector<size_t> cap, host_off;
  std::vector<long long> dev_off;
  int oversize_rc = CTPN_ERR_CAPACITY;   // what a file with more coefficients than its capacity gets ...
  const char* oversize_msg = "";         // ... and, where jpeg_huff_prepare found it, says
  bool strided = false;                  // every file has file 0's capacity and coefficient count and stands at multiples of them: ONE 2-D copy
  bool tab = false;                      // the call fills J->tab_host (n JrImage) between begin() and upload()
  size_t coef_dev_elems = 0;             // of coef_dev, what the device entropy decode clears first
  // what the stages fill
  ctpn_ctx::JpegBufs* J = nullptr;       // this call's buffer set
  hipStream_t qs = c->stream_c;          // the ctx's copy queue
  std::vector<JpegGeom> geo;
  std::vector<JhPrep> prep;                       // device entropy: the files' parsed frames ...
  std::vector<std::vector<uint8_t>> held;         // ... and the bytes of files given as paths (kept until the batch is staged)
  std::vector<const uint8_t*> dptr;
  std::vector<size_t> dlen;

  JpegDecode(ctpn_ctx* c_, const std::string& who_, const JpegSource& src_, int n_, bool dev_entropy_)
      : c(c_), who(who_), src(src_), n(n_), dev_entropy(dev_entropy_), cap((size_t)n_), host_off((size_t)n_), dev_off((size_t)n_), geo((size_t)n_),
        prep(dev_entropy_ ? (size_t)n_ : 0), held(dev_entropy_ && src_.paths ? (size_t)n_ : 0), dptr((size_t)n_, nullptr), dlen((size_t)n_, 0) {}

  // the host entropy decode of file i (bytes at dptr[i]) into its place in the page-locked blocks
  int host_file(int i, JpegGeom* g) {
    const int rc = jpeg_entropy_decode(dptr[i], dlen[i], J->coef_host.as<int16_t>() + host_off[i], cap[i], J->qt_host.as<uint16_t>() + (size_t)i * 192, g);
    return rc == CTPN_ERR_CAPACITY ? oversize_rc : rc;
  }

  // this call's buffer set, large enough, and the host half: one file per worker thread -- parsed for the device (jpeg_huff_prepare) or
  // decoded to coefficients; geo[i] is file i's geometry. The first failed file is the call's error.
  int begin(size_t coef_total, size_t raw_bytes, size_t out_bytes) {
    CTPN_HIP_TRY(hipSetDevice(c->device));
    J = &c->jpeg[c->jpeg_flip];
    // the page-locked blocks (coefficients, tables, descriptors) were last read by the copies of two calls ago
    if (J->h2d_valid) CTPN_HIP_TRY(hipEventSynchronize(J->ev_h2d));
    if (const int rc = jpeg_reserve(c, *J, (size_t)n, coef_total, raw_bytes, out_bytes, tab)) return rc;
    std::vector<int> st((size_t)n, CTPN_OK);
    std::vector<std::string> msg((size_t)n);
    c->pool->run(n, [&](int i) {
      static thread_local std::vector<uint8_t> filebuf;      // host entropy: one per worker thread, reused from batch to batch
      try {
        if (src.paths) {
          std::vector<uint8_t>& buf = dev_entropy ? held[i] : filebuf;
          if (!jpeg_read_file(src.paths[i], buf)) { st[i] = CTPN_ERR_ARG; msg[i] = std::string("cannot read ") + src.paths[i]; return; }
          dptr[i] = buf.data(); dlen[i] = buf.size();       // (filebuf: good for this worker's decode below only; upload() reads held's)
        } else { dptr[i] = src.mem[i]; dlen[i] = src.sizes[i]; }
        if (dev_entropy) {
          st[i] = jpeg_huff_prepare(dptr[i], dlen[i], &prep[i]);
          if (!st[i] && prep[i].coef_count > cap[i]) st[i] = fail(oversize_rc, oversize_msg);
          if (!st[i]) geo[i] = prep[i].g;
        } else
          st[i] = host_file(i, &geo[i]);
        if (st[i]) msg[i] = ctpn_last_error();      // (the error text is per thread)
        if (!dev_entropy && filebuf.capacity() > ((size_t)8 << 20)) std::vector<uint8_t>().swap(filebuf);      // one huge file must not pin its size per worker for the run
      } catch (const std::exception& e) { st[i] = CTPN_ERR_CAPACITY; msg[i] = e.what(); }      // nothing may leave a worker thread
    });
    for (int i = 0; i < n; ++i) if (st[i]) return fail(st[i], who + "file " + std::to_string(i) + ": " + msg[i]);
    return CTPN_OK;
  }

  int copy_file(int i) {
    CTPN_HIP_TRY(hipMemcpyAsync(J->coef_dev.as<int16_t>() + dev_off[i], J->coef_host.as<int16_t>() + host_off[i], (size_t)geo[i].coef_per_img * sizeof(int16_t), hipMemcpyHostToDevice, qs));
    return CTPN_OK;
  }

  // coefficients, quantisation tables and (ragged) descriptors onto the device, in queue qs
  int upload() {
    int rc;
    // the device buffers of this set: the forward that read out_dev two calls ago has passed its first layer
    if (J->consumed_valid) CTPN_HIP_TRY(hipStreamWaitEvent(qs, J->ev_consumed, 0));
    if (dev_entropy) {
      std::vector<int> use((size_t)n);
      std::vector<uint32_t> flags((size_t)n, 0u);
      for (int i = 0; i < n; ++i) { use[i] = i; std::memcpy(J->qt_host.as<uint16_t>() + (size_t)i * 192, prep[i].qt, sizeof(prep[i].qt)); }
      if ((rc = jh_decode(c, dptr.data(), dlen.data(), prep, use, JH_SUBSEQ_DEFAULT, J->coef_dev.as<int16_t>(), dev_off, coef_dev_elems, qs, flags))) return rc;
      // a file with a raised flag is the host half's, alone: its status and message are the host's, its coefficients replace the device's
      for (int i = 0; i < n; ++i) {
        if (!flags[i]) continue;
        if ((rc = host_file(i, &geo[i]))) return fail(rc, who + "file " + std::to_string(i) + ": " + ctpn_last_error());
        if ((rc = copy_file(i))) return rc;
      }
    } else if (strided)
      CTPN_HIP_TRY(hipMemcpy2DAsync(J->coef_dev.as<int16_t>(), (size_t)geo[0].coef_per_img * sizeof(int16_t), J->coef_host.as<int16_t>(), cap[0] * sizeof(int16_t), (size_t)geo[0].coef_per_img * sizeof(int16_t),
                                    (size_t)n, hipMemcpyHostToDevice, qs));
    else
      for (int i = 0; i < n; ++i)      // every file's own coefficients (its capacity is the largest any layout of its size needs: up to twice as many)
        if ((rc = copy_file(i))) return rc;
    CTPN_HIP_TRY(hipMemcpyAsync(J->qt_dev.as<uint16_t>(), J->qt_host.as<uint16_t>(), (size_t)n * 192 * sizeof(uint16_t), hipMemcpyHostToDevice, qs));
    if (tab) CTPN_HIP_TRY(hipMemcpyAsync(J->tab_dev.get(), J->tab_host.get(), (size_t)n * sizeof(JrImage), hipMemcpyHostToDevice, qs));
    CTPN_HIP_TRY(hipEventRecord(J->ev_h2d, qs));
    J->h2d_valid = true;
    return CTPN_OK;
  }

  // behind the call's pixel launch: out_dev holds n images of out_h x out_w; the next call takes the other buffer set
  int publish(int out_h, int out_w) {
    CTPN_HIP_TRY(hipEventRecord(J->ev_ready, qs));
    J->ready_valid = true;
    J->consumed_valid = false;      // until a forward reads this buffer
    J->out_n = n; J->out_h = out_h; J->out_w = out_w;
    c->jpeg_flip ^= 1;
    return CTPN_OK;
  }
};

// ctpn_decode_jpeg_batch / _files (+ _device): files of one size, one component layout and one EXIF orientation, resized by one pair of factors
static int jpeg_decode_uniform(ctpn_ctx* c, const JpegSource& src, int n, int h, int w, double fx, double fy, const uint8_t** images_dev_out, int* out_h, int* out_w,
                               bool dev_entropy) {
  const std::string who = "ctpn_decode_jpeg_batch: ";
  if (c->postproc_only) return fail(CTPN_ERR_STATE, who + "post-processing-only ctx");
  if (n <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535) return fail(CTPN_ERR_ARG, who + "empty batch / bad size");
  const bool resize = (fx > 0.0 && fx != 1.0) || (fy > 0.0 && fy != 1.0);
  if (!(fx > 0.0)) fx = 1.0;
  if (!(fy > 0.0)) fy = 1.0;
  int dh = h, dw = w;
  if (resize) { dh = resize_out_dim(h, fy); dw = resize_out_dim(w, fx); if (dh <= 0 || dw <= 0) return fail(CTPN_ERR_ARG, who + "empty output"); }
  JpegDecode D(c, who, src, n, dev_entropy);
  const size_t cap = jpeg_coef_capacity(h, w);
  for (int i = 0; i < n; ++i) { D.cap[i] = cap; D.host_off[i] = (size_t)i * cap; }
  D.oversize_msg = "jpeg: coefficient buffer too small";
  D.strided = true;
  int rc = D.begin((size_t)n * cap, resize ? (size_t)n * h * w * 3 : 0, (size_t)n * dh * dw * 3);
  if (rc) return rc;
  const JpegGeom& g = D.geo[0];
  for (int i = 0; i < n; ++i) {
    const JpegGeom& gi = D.geo[i];
    if (gi.oh != h || gi.ow != w) return fail(CTPN_ERR_ARG, who + "file " + std::to_string(i) + " is not " + std::to_string(h) + " x " + std::to_string(w) + " (as cv2.imread returns it: EXIF orientation applied)");
    if (gi.ncomp != g.ncomp || gi.hs0 != g.hs0 || gi.vs0 != g.vs0 || gi.orient != g.orient) return fail(CTPN_ERR_UNSUPPORTED, who + "the files of one batch must share one component layout and one EXIF orientation");
    D.dev_off[i] = (long long)i * g.coef_per_img;
  }
  D.coef_dev_elems = (size_t)n * g.coef_per_img;
  if ((rc = D.upload())) return rc;
  auto& J = *D.J;
  if ((rc = launch_jpeg_pixels(J.coef_dev.as<int16_t>(), J.qt_dev.as<uint16_t>(), c->jpeg_planes.as<uint8_t>(), resize ? c->jpeg_raw.as<uint8_t>() : J.out_dev.as<uint8_t>(), g, n, D.qs))) return rc;
  // resize_im (reference ctpn/demo.py:21-25: cv2.resize, INTER_LINEAR) of the decoded batch, in the same queue
  if (resize && (rc = launch_resize_linear(c->jpeg_raw.as<uint8_t>(), J.out_dev.as<uint8_t>(), 0, n, h, w, dh, dw, fx, fy, D.qs))) return rc;
  if ((rc = D.publish(dh, dw))) return rc;
  *images_dev_out = J.out_dev.as<uint8_t>();
  if (out_h) *out_h = dh;
  if (out_w) *out_w = dw;
  return CTPN_OK;
}

// ctpn_decode_jpeg_batch_ragged / ctpn_decode_jpeg_files_ragged: files of mixed sizes, layouts and orientations into one ragged canvas. Per
// file: its own coefficient capacity at a prefix-summed base (coefficients and planes alike), its own geometry and factor in a descriptor
// table, one pixel launch pair over the table
static int jpeg_decode_ragged(ctpn_ctx* c, const JpegSource& src, int n, const int* file_h, const int* file_w, const double* factors, int hc, int wc,
                              bool dev_entropy, const uint8_t** canvas_dev_out, int* heights_out) {
  const std::string who = "ctpn_decode_jpeg_batch_ragged: ";
  if (c->postproc_only) return fail(CTPN_ERR_STATE, who + "post-processing-only ctx");
  if (n <= 0 || hc < 16 || wc <= 0 || hc > 65535 || wc > 65535) return fail(CTPN_ERR_ARG, who + "empty batch / bad canvas size (hc >= 16)");
  JpegDecode D(c, who, src, n, dev_entropy);
  std::vector<double> fac((size_t)n);
  std::vector<int> hts((size_t)n);
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    const int h = file_h[i], w = file_w[i];
    const std::string file = "file " + std::to_string(i);
    if (h <= 0 || w <= 0 || h > 65535 || w > 65535) return fail(CTPN_ERR_ARG, who + file + ": bad size");
    const double f = factors[i] > 0.0 ? factors[i] : 1.0;
    const int dh = f == 1.0 ? h : resize_out_dim(h, f), dw = f == 1.0 ? w : resize_out_dim(w, f);
    if (dw != wc) return fail(CTPN_ERR_ARG, who + file + ": width " + std::to_string(w) + " maps to " + std::to_string(dw) + ", not to the canvas's " + std::to_string(wc));
    if (dh < 16 || dh > hc) return fail(CTPN_ERR_ARG, who + file + ": height " + std::to_string(h) + " maps to " + std::to_string(dh) + ", outside 16 .. " + std::to_string(hc));
    fac[i] = f; hts[i] = dh;
    D.cap[i] = jpeg_coef_capacity(h, w);
    D.host_off[i] = total; D.dev_off[i] = (long long)total;
    total += D.cap[i];
  }
  D.oversize_rc = CTPN_ERR_ARG;      // (only a file that is not file_h x file_w overruns its own capacity)
  D.oversize_msg = "jpeg: the file is larger than the size given for it";
  D.tab = true;
  D.coef_dev_elems = total;
  int rc = D.begin(total, 0, (size_t)n * hc * wc * 3);
  if (rc) return rc;
  for (int i = 0; i < n; ++i)
    if (D.geo[i].oh != file_h[i] || D.geo[i].ow != file_w[i])
      return fail(CTPN_ERR_ARG, who + "file " + std::to_string(i) + " is not " + std::to_string(file_h[i]) + " x " + std::to_string(file_w[i]) + " (as cv2.imread returns it: EXIF orientation applied)");
  auto& J = *D.J;
  // the descriptor table
  JrImage* tab = J.tab_host.as<JrImage>();
  long long blocks = 0;
  for (int i = 0; i < n; ++i) {
    JrImage& d = tab[i];
    std::memset(&d, 0, sizeof(d));
    d.g = D.geo[i];
    d.coef_base = d.plane_base = D.dev_off[i];
    d.block0 = blocks;
    d.inv_f = 1.0 / fac[i];
    d.resize = fac[i] != 1.0;
    d.height = hts[i];
    blocks += D.geo[i].blocks_per_img;
  }
  if ((rc = D.upload())) return rc;
  if ((rc = launch_jpeg_pixels_ragged(J.coef_dev.as<int16_t>(), J.qt_dev.as<uint16_t>(), c->jpeg_planes.as<uint8_t>(), J.out_dev.as<uint8_t>(), J.tab_dev.as<JrImage>(), n, blocks, hc, wc, D.qs))) return rc;
  if ((rc = D.publish(hc, wc))) return rc;
  *canvas_dev_out = J.out_dev.as<uint8_t>();
  for (int i = 0; i < n; ++i) heights_out[i] = hts[i];
  return CTPN_OK;
}

}  // namespace ctpn

extern "C" {

int ctpn_decode_jpeg_batch(ctpn_ctx* c, const uint8_t* const* files, const size_t* sizes, int n, int h, int w, double fx, double fy,
                           const uint8_t** images_dev_out, int* out_h, int* out_w) {
  if (!c || !files || !sizes || !images_dev_out) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_batch: null pointer");
  for (int i = 0; i < n; ++i) if (!files[i]) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_batch: null file pointer");
  JpegSource src; src.mem = files; src.sizes = sizes;
  return jpeg_decode_uniform(c, src, n, h, w, fx, fy, images_dev_out, out_h, out_w, false);
}

int ctpn_decode_jpeg_files(ctpn_ctx* c, const char* const* paths, int n, int h, int w, double fx, double fy, const uint8_t** images_dev_out, int* out_h, int* out_w) {
  if (!c || !paths || !images_dev_out) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_files: null pointer");
  for (int i = 0; i < n; ++i) if (!paths[i]) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_files: null path");
  JpegSource src; src.paths = paths;
  return jpeg_decode_uniform(c, src, n, h, w, fx, fy, images_dev_out, out_h, out_w, false);
}

// ---- the same with the Huffman decode on the device (jpeg_huff.hip) ----
int ctpn_decode_jpeg_batch_device(ctpn_ctx* c, const uint8_t* const* files, const size_t* sizes, int n, int h, int w, double fx, double fy,
                                  const uint8_t** images_dev_out, int* out_h, int* out_w) {
  if (!c || !files || !sizes || !images_dev_out) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_batch_device: null pointer");
  for (int i = 0; i < n; ++i) if (!files[i]) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_batch_device: null file pointer");
  JpegSource src; src.mem = files; src.sizes = sizes;
  return jpeg_decode_uniform(c, src, n, h, w, fx, fy, images_dev_out, out_h, out_w, true);
}

int ctpn_decode_jpeg_files_device(ctpn_ctx* c, const char* const* paths, int n, int h, int w, double fx, double fy, const uint8_t** images_dev_out, int* out_h, int* out_w) {
  if (!c || !paths || !images_dev_out) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_files_device: null pointer");
  for (int i = 0; i < n; ++i) if (!paths[i]) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_files_device: null path");
  JpegSource src; src.paths = paths;
  return jpeg_decode_uniform(c, src, n, h, w, fx, fy, images_dev_out, out_h, out_w, true);
}

// ---- files of mixed sizes into one ragged canvas (jpeg_ragged.hip) ----
int ctpn_decode_jpeg_batch_ragged(ctpn_ctx* c, const uint8_t* const* files, const size_t* sizes, int n, const int* file_h, const int* file_w, const double* factors,
                                  int hc, int wc, int entropy_on_device, const uint8_t** canvas_dev_out, int* heights_out) {
  if (!c || !files || !sizes || !file_h || !file_w || !factors || !canvas_dev_out || !heights_out) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_batch_ragged: null pointer");
  for (int i = 0; i < n; ++i) if (!files[i]) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_batch_ragged: null file pointer");
  JpegSource src; src.mem = files; src.sizes = sizes;
  return jpeg_decode_ragged(c, src, n, file_h, file_w, factors, hc, wc, entropy_on_device != 0, canvas_dev_out, heights_out);
}

int ctpn_decode_jpeg_files_ragged(ctpn_ctx* c, const char* const* paths, int n, const int* file_h, const int* file_w, const double* factors, int hc, int wc,
                                  int entropy_on_device, const uint8_t** canvas_dev_out, int* heights_out) {
  if (!c || !paths || !file_h || !file_w || !factors || !canvas_dev_out || !heights_out) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_files_ragged: null pointer");
  for (int i = 0; i < n; ++i) if (!paths[i]) return fail(CTPN_ERR_ARG, "ctpn_decode_jpeg_files_ragged: null path");
  JpegSource src; src.paths = paths;
  return jpeg_decode_ragged(c, src, n, file_h, file_w, factors, hc, wc, entropy_on_device != 0, canvas_dev_out, heights_out);
}

int ctpn_jpeg_entropy_decode_device(ctpn_ctx* c,const uint8_t* const* files, const size_t* sizes, int n, int subseq_bits, int16_t* coef_out,
                                    size_t coef_capacity_per_file, uint16_t* qt_out, int* layout8_out, int* status_out) {
  if (!c || !files || !sizes || !coef_out || !qt_out || !layout8_out || !status_out || n <= 0) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_decode_device: null pointer / empty batch");
  for (int i = 0; i < n; ++i) if (!files[i]) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_decode_device: null file pointer");
  if (c->postproc_only) return fail(CTPN_ERR_STATE, "ctpn_jpeg_entropy_decode_device: post-processing-only ctx");
  if (subseq_bits == 0) subseq_bits = JH_SUBSEQ_DEFAULT;
  if (subseq_bits < JH_SUBSEQ_MIN || subseq_bits > JH_SUBSEQ_MAX || subseq_bits % 32) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_decode_device: subseq_bits must be 0 or a multiple of 32 in 128 .. 4096");
  if (coef_capacity_per_file == 0 || (size_t)n > ((size_t)1 << 40) / coef_capacity_per_file) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_decode_device: bad coefficient capacity");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  std::vector<JhPrep> prep((size_t)n);
  std::vector<int> use;
  std::vector<long long> coef_base((size_t)n);
  std::vector<uint32_t> flags((size_t)n, 0u);
  for (int i = 0; i < n; ++i) {
    coef_base[i] = (long long)i * (long long)coef_capacity_per_file;
    status_out[i] = jpeg_huff_prepare(files[i], sizes[i], &prep[i]);
    if (!status_out[i] && prep[i].coef_count > coef_capacity_per_file) status_out[i] = fail(CTPN_ERR_CAPACITY, "jpeg: coefficient buffer too small");
    if (!status_out[i]) use.push_back(i);
  }
  c->jh_stats[0] = c->jh_stats[1] = c->jh_stats[2] = c->jh_stats[3] = 0;
  if (use.empty()) return CTPN_OK;
  const size_t elems = (size_t)n * coef_capacity_per_file;
  DevBuf coef_buf;      // released on every way out (the release waits for what the queue still does with it)
  if (const int rc = coef_buf.alloc(elems * sizeof(int16_t))) return rc;
  int16_t* coef_dev = coef_buf.as<int16_t>();
  hipStream_t qs = c->stream_c;
  int rc = jh_decode(c, files, sizes, prep, use, (uint32_t)subseq_bits, coef_dev, coef_base, elems, qs, flags);
  for (int i : use) {
    if (rc) break;
    if (flags[i]) continue;
    if (hipMemcpyAsync(coef_out + (size_t)i * coef_capacity_per_file, coef_dev + (size_t)i * coef_capacity_per_file, prep[i].coef_count * sizeof(int16_t), hipMemcpyDeviceToHost, qs) != hipSuccess)
      rc = fail(CTPN_ERR_HIP, "ctpn_jpeg_entropy_decode_device: copy of the coefficients failed");
  }
  if (!rc && hipStreamSynchronize(qs) != hipSuccess) rc = fail(CTPN_ERR_HIP, "ctpn_jpeg_entropy_decode_device: queue failed");
  if (rc) return rc;
  for (int i : use) {
    int* l8 = layout8_out + 8 * (size_t)i;
    if (flags[i]) {      // the host half on this file alone: its status, its message, its results
      status_out[i] = ctpn_jpeg_entropy_decode(files[i], sizes[i], coef_out + (size_t)i * coef_capacity_per_file, coef_capacity_per_file, qt_out + 192 * (size_t)i, l8);
      continue;
    }
    jpeg_layout8(prep[i].g, l8);
    std::memcpy(qt_out + 192 * (size_t)i, prep[i].qt, sizeof(prep[i].qt));
  }
  return CTPN_OK;
}

int ctpn_jpeg_entropy_device_stats(ctpn_ctx* c, long long* out4) {
  if (!c || !out4) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_device_stats: null pointer");
  std::memcpy(out4, c->jh_stats, sizeof(c->jh_stats));
  return CTPN_OK;
}

int ctpn_jpeg_batch_fetch(ctpn_ctx* c, const uint8_t* images_dev, uint8_t* host_out, size_t capacity) {
  if (!c || !images_dev || !host_out) return fail(CTPN_ERR_ARG, "ctpn_jpeg_batch_fetch: null pointer");
  for (auto& J : c->jpeg)
    if (J.ready_valid && J.out_dev.as<uint8_t>() == images_dev) {
      const size_t bytes = (size_t)J.out_n * J.out_h * J.out_w * 3;
      if (capacity < bytes) return fail(CTPN_ERR_CAPACITY, "ctpn_jpeg_batch_fetch: capacity too small");
      CTPN_HIP_TRY(hipSetDevice(c->device));
      CTPN_HIP_TRY(hipEventSynchronize(J.ev_ready));
      CTPN_HIP_TRY(hipMemcpy(host_out, J.out_dev.as<uint8_t>(), bytes, hipMemcpyDeviceToHost));
      return CTPN_OK;
    }
  return fail(CTPN_ERR_STATE, "ctpn_jpeg_batch_fetch: not a live batch of ctpn_decode_jpeg_batch");
}

}  // extern "C"
