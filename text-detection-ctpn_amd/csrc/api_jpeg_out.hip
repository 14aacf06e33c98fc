// C ABI of libctpn_hip.so, JPEG output unit: JPEG writing (kernels and the entropy coder: jpeg_enc.hip) of a batch on the device, and
// the cv2.imwrite end of the annotated result images of ctpn/demo.py:28-52 (outlines and resize: api_out_stage.hip).
// One enc_enqueue / enc_finish over a list of per-image geometries: n equal ones (the uniform calls, jpeg_fdct_kernel) or any mix of sizes
// and pitches (ctpn_encode_jpeg_mixed, ctpn_write_line_crops: jpeg_fdct_mixed_kernel). Two entropy forms behind them: host (the default entry points) and device (the *_device entry points: jpeg_huff_enc.hip).
#include "ctx.h"
#include "jpeg_enc_mixed_dev.h"
#include "jpeg_enc_pixel.h"
#include "jpeg_huff_enc_dev.h"

namespace ctpn {

// room for coef_elems coefficients on the device and in the page-locked block
static int enc_reserve_coef(ctpn_ctx* c, size_t coef_elems) {
  auto& E = c->enc;
  int rc;
  if ((rc = E.ev_done.ensure()) || (rc = E.coef_dev.grow(coef_elems * sizeof(int16_t)))) return rc;
  return E.coef_host.grow(coef_elems * sizeof(int16_t));
}

static int enc_reserve(ctpn_ctx* c, size_t coef_elems, int quality) {
  auto& E = c->enc;
  int rc;
  if ((rc = enc_reserve_coef(c, coef_elems)) || (rc = E.qtab_dev.grow(128 * sizeof(JencQ))) || (rc = E.qtab_host.grow(128 * sizeof(JencQ)))) return rc;      // the tables: on first use
  if (E.qtab_quality != quality) {      // (the copy of the previous call has long finished: that call waited for its coefficients)
    jpeg_enc_qtables(quality, nullptr, E.qtab_host.as<JencQ>());
    CTPN_HIP_TRY(hipMemcpyAsync(E.qtab_dev.get(), E.qtab_host.get(), 128 * sizeof(JencQ), hipMemcpyHostToDevice, c->stream_c));
    E.qtab_quality = quality;
  }
  return CTPN_OK;
}

// the images of one call: every image's geometry (jpeg_enc_geom) and the int16 offset of its coefficients, packed at the prefix sums of the
// images' own coef_per_img. The uniform calls hold n equal geometries
struct EncPlan {
  std::vector<JpegGeom> g;
  std::vector<long long> coef0;
  size_t coef_elems = 0;
  void add(int h, int w) {
    JpegGeom q;
    jpeg_enc_geom(h, w, q);
    g.push_back(q); coef0.push_back((long long)coef_elems);
    coef_elems += (size_t)q.coef_per_img;
  }
  int n() const { return (int)g.size(); }
};

// where the images of a mixed call lie in their source buffer (bytes)
struct EncSource { const size_t* pitches; const size_t* offsets; };

// the descriptor table of a mixed call: built in the ctx's page-locked block, copied in the copy queue (the block is free again: every
// call that used it waited for its coefficients or result words, which come behind the copy)
static int enc_stage_table(ctpn_ctx* c, const EncPlan& P, const EncSource& src, long long& items) {
  auto& E = c->enc;
  const size_t bytes = (size_t)P.n() * sizeof(JemImage);
  int rc;
  if ((rc = E.mix_host.grow(bytes)) || (rc = E.mix_dev.grow(bytes))) return rc;
  JemImage* tab = E.mix_host.as<JemImage>();
  for (int i = 0; i < P.n(); ++i) {
    const JpegGeom& g = P.g[i];
    jem_describe(tab[i], g.h, g.w, (long long)src.pitches[i], (long long)src.offsets[i]);
    for (int k = 0; k < 3; ++k)
      if (tab[i].bw[k] != g.bw[k] || tab[i].bh[k] != g.bh[k] || tab[i].coef_off[k] != g.coef_off[k]) return fail(CTPN_ERR_STATE, "jpeg encode: descriptor and geometry disagree");
  }
  long long coef_total = 0;
  items = jem_prefix(tab, P.n(), &coef_total);
  if (items < 0) return fail(CTPN_ERR_ARG, "jpeg encode: more than 2^31 - 1 work items in one call");
  if ((size_t)coef_total != P.coef_elems) return fail(CTPN_ERR_STATE, "jpeg encode: descriptor and geometry disagree");
  CTPN_HIP_TRY(hipMemcpyAsync(E.mix_dev.get(), tab, bytes, hipMemcpyHostToDevice, c->stream_c));
  return CTPN_OK;
}

// device half in the ctx's copy queue: pixels (device) -> coefficients, in the page-locked block too unless the device codes them as well
// (device_entropy); no host wait. src == null: the plan's n equal images, tightly packed (n x h x w x 3); else images of any sizes at
// their own pitches and offsets
static int enc_enqueue(ctpn_ctx* c, const uint8_t* pixels_dev, const EncPlan& P, const EncSource* src, int quality, bool device_entropy) {
  int rc = enc_reserve(c, P.coef_elems, quality);
  if (rc) return rc;
  auto& E = c->enc;
  if (!src) {
    if ((rc = launch_jpeg_fdct(pixels_dev, E.coef_dev.as<int16_t>(), E.qtab_dev.as<JencQ>(), P.g[0], P.n(), c->stream_c))) return rc;
  } else {
    long long items = 0;
    if ((rc = enc_stage_table(c, P, *src, items))) return rc;
    if ((rc = launch_jpeg_fdct_mixed(pixels_dev, E.coef_dev.as<int16_t>(), E.qtab_dev.as<JencQ>(), E.mix_dev.as<JemImage>(), P.n(), items, c->stream_c))) return rc;
  }
  if (!device_entropy) CTPN_HIP_TRY(hipMemcpyAsync(E.coef_host.as<int16_t>(), E.coef_dev.as<int16_t>(), P.coef_elems * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream_c));
  CTPN_HIP_TRY(hipEventRecord(E.ev_done, c->stream_c));
  return CTPN_OK;
}

// one image's file into the caller's buffer (out, bytes_out) or into a file of its own (path); code(buffer, capacity, &bytes) writes the
// file's bytes and returns their status. Runs on a worker thread: nothing may leave it
template <class Code>
static void enc_deliver(size_t bound, uint8_t* out, size_t capacity, size_t* bytes_out, const char* path, int& st, std::string& msg, const Code& code) {
  try {
    size_t bytes = 0;
    if (path) {
      static thread_local std::vector<uint8_t> filebuf;      // one per worker thread, reused from batch to batch
      if (filebuf.size() < bound) filebuf.resize(bound);
      st = code(filebuf.data(), filebuf.size(), &bytes);
      if (st) { msg = ctpn_last_error(); return; }
      write_file(path, filebuf.data(), bytes, st, msg);
      if (filebuf.capacity() > ((size_t)64 << 20)) std::vector<uint8_t>().swap(filebuf);
    } else {
      st = code(out, capacity, &bytes);
      *bytes_out = bytes;
      if (st) msg = ctpn_last_error();
    }
  } catch (const std::exception& e) { st = CTPN_ERR_CAPACITY; msg = e.what(); }
}

// ---- the device-entropy form ---------------------------------------------------------------------------------------------------------
struct EncJob {                       // one image of a device-entropy call
  int h, w, hs, vs; const uint16_t* qt;      // the file's frame
  JheImg img;                         // ... described (jhe_describe); coef_off: its coefficients in E.coef_dev, int16 elements
  const int16_t* coef_host;          // the same on the host in natural order (the test seam), or null: zig-zag, copied from the device if the host half needs them
  uint8_t* out; size_t capacity; size_t* bytes_out; const char* path;
  bool on_host = false;               // the host half codes it
  const uint8_t* scan = nullptr; size_t scan_have = 0, scan_bytes = 0;      // else: the stuffed scan body (page-locked), the bytes of it that were copied, its size
  int st = CTPN_OK; std::string msg;
  void describe(long long coef_off) { jhe_describe(img, h, w, hs, vs); img.coef_off = coef_off; }
};

// one launch group (at most JHE_MAX_BLOCKS blocks): the kernels, then the result words -- the wait of the host form on its coefficients --,
// then exactly the bytes the sizes say: scan bodies, or the coefficients of an image whose flag is raised
static int enc_huff_group(ctpn_ctx* c, std::vector<EncJob>& jobs, const std::vector<int>& use, bool zigzag) {
  auto& E = c->enc;
  hipStream_t qs = c->stream_c;
  const size_t m = use.size();
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  int rc;
  if ((rc = E.huff_host.grow(m * (sizeof(JheImg) + sizeof(JheRes))))) return rc;
  JheImg* imgs = E.huff_host.as<JheImg>();
  JheRes* res = (JheRes*)(E.huff_host.as<uint8_t>() + m * sizeof(JheImg));
  for (size_t k = 0; k < m; ++k) imgs[k] = jobs[use[k]].img;
  JheTotals t;
  jhe_layout(imgs, m, t);
  const size_t o_img = 0, o_res = up(o_img + m * sizeof(JheImg)), o_len = up(o_res + m * sizeof(JheRes)), o_cnt = up(o_len + (size_t)t.blk * 4),
               o_uns = up(o_cnt + (size_t)t.chunks * 4), o_out = up(o_uns + (size_t)t.words * 4), total = o_out + t.outb;
  if ((rc = E.huff_dev.grow(total))) return rc;
  uint8_t* huff = E.huff_dev.as<uint8_t>();
  if (!E.huff_tab_dev) {
    static const JheTables T = [] { JheTables t; jhe_build_tables(t); return t; }();
    if ((rc = E.huff_tab_dev.alloc(sizeof(JheTables)))) return rc;
    CTPN_HIP_TRY(hipMemcpy(E.huff_tab_dev.get(), &T, sizeof(JheTables), hipMemcpyHostToDevice));
  }
  JheBatchDev B;
  B.imgs = (const JheImg*)(huff + o_img); B.res = (JheRes*)(huff + o_res); B.len = (uint32_t*)(huff + o_len); B.cnt = (uint32_t*)(huff + o_cnt);
  B.uns = (uint32_t*)(huff + o_uns); B.out = huff + o_out; B.coef = E.coef_dev.as<int16_t>(); B.tables = E.huff_tab_dev.as<JheTables>();
  B.n = (int)m; B.max_blocks = t.max_blocks; B.max_chunks = t.max_chunks;
  CTPN_HIP_TRY(hipMemcpyAsync(huff + o_img, imgs, m * sizeof(JheImg), hipMemcpyHostToDevice, qs));
  CTPN_HIP_TRY(hipMemsetAsync(huff + o_res, 0, m * sizeof(JheRes), qs));
  CTPN_HIP_TRY(hipMemsetAsync(huff + o_uns, 0, (size_t)t.words * 4, qs));      // the write pass ORs shared words into it
  if ((rc = launch_jpeg_huff_enc(B, zigzag, qs))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(res, huff + o_res, m * sizeof(JheRes), hipMemcpyDeviceToHost, qs));
  CTPN_HIP_TRY(hipEventRecord(E.ev_done, qs));
  CTPN_HIP_TRY(hipEventSynchronize(E.ev_done));
  c->jhe_stats[3] += (long long)(m * sizeof(JheRes));
  size_t scan_total = 0;
  for (size_t k = 0; k < m; ++k) {
    EncJob& J = jobs[use[k]];
    if (res[k].flag || res[k].bytes > imgs[k].out_cap) { J.on_host = true; continue; }
    J.scan_bytes = res[k].bytes;
    J.scan_have = J.path ? J.scan_bytes : (J.out ? std::min(J.scan_bytes, J.capacity) : 0);
    scan_total += up(J.scan_have);
  }
  if ((rc = E.scan_host.grow(scan_total))) return rc;
  size_t at = 0;
  bool copies = false;
  for (size_t k = 0; k < m; ++k) {
    EncJob& J = jobs[use[k]];
    if (J.on_host) {
      ++c->jhe_stats[1];
      if (J.coef_host) continue;
      const size_t bytes = (size_t)imgs[k].nblk * 64 * sizeof(int16_t);
      CTPN_HIP_TRY(hipMemcpyAsync(E.coef_host.as<int16_t>() + J.img.coef_off, E.coef_dev.as<int16_t>() + J.img.coef_off, bytes, hipMemcpyDeviceToHost, qs));
      c->jhe_stats[3] += (long long)bytes; copies = true;
      continue;
    }
    ++c->jhe_stats[0]; c->jhe_stats[2] += imgs[k].nblk;
    J.scan = E.scan_host.as<uint8_t>() + at;
    if (J.scan_have) {
      CTPN_HIP_TRY(hipMemcpyAsync(E.scan_host.as<uint8_t>() + at, huff + o_out + imgs[k].out0, J.scan_have, hipMemcpyDeviceToHost, qs));
      c->jhe_stats[3] += (long long)J.scan_have; copies = true;
    }
    at += up(J.scan_have);
  }
  if (copies) {
    CTPN_HIP_TRY(hipEventRecord(E.ev_done, qs));
    CTPN_HIP_TRY(hipEventSynchronize(E.ev_done));
  }
  return CTPN_OK;
}

// device entropy coding of the jobs' coefficients (in E.coef_dev, all zig-zag or all natural) and delivery of the files, group by group;
// the per-file outcomes are in the jobs
static int enc_huff(ctpn_ctx* c, std::vector<EncJob>& jobs, bool zigzag) {
  auto& E = c->enc;
  if (int rc = E.ev_done.ensure()) return rc;
  c->jhe_stats[0] = c->jhe_stats[1] = c->jhe_stats[2] = c->jhe_stats[3] = 0;
  const int n = (int)jobs.size();
  for (int i0 = 0; i0 < n;) {
    std::vector<int> use;
    uint64_t tot = 0;
    int i1 = i0;
    for (; i1 < n; ++i1) {
      const uint64_t nb = jobs[i1].img.nblk;      // (below 2^28 at 65535 x 65535)
      if (nb > (uint64_t)JHE_MAX_BLOCKS) {      // offsets of 32 bits do not hold it: the host half's
        jobs[i1].on_host = true; ++c->jhe_stats[1];
        if (!jobs[i1].coef_host) {
          CTPN_HIP_TRY(hipMemcpyAsync(E.coef_host.as<int16_t>() + jobs[i1].img.coef_off, E.coef_dev.as<int16_t>() + jobs[i1].img.coef_off, (size_t)nb * 64 * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream_c));
          CTPN_HIP_TRY(hipEventRecord(E.ev_done, c->stream_c));
          CTPN_HIP_TRY(hipEventSynchronize(E.ev_done));
          c->jhe_stats[3] += (long long)((size_t)nb * 64 * sizeof(int16_t));
        }
        continue;
      }
      if (tot + nb > (uint64_t)JHE_MAX_BLOCKS || use.size() == 65535) break;
      use.push_back(i1); tot += nb;
    }
    int rc;
    if (!use.empty() && (rc = enc_huff_group(c, jobs, use, zigzag))) return rc;
    c->pool->run(i1 - i0, [&](int k) {
      EncJob& J = jobs[(size_t)i0 + k];
      const size_t bound = J.on_host ? jpeg_encode_capacity(J.h, J.w) : J.scan_bytes + 1024;
      if (J.on_host) {
        const int16_t* coef = J.coef_host ? J.coef_host : E.coef_host.as<int16_t>() + J.img.coef_off;
        const bool zz = !J.coef_host;
        enc_deliver(bound, J.out, J.capacity, J.bytes_out, J.path, J.st, J.msg, [&](uint8_t* buf, size_t cap, size_t* bytes) {
          return jpeg_entropy_encode(coef, zz, J.h, J.w, J.hs, J.vs, J.qt, buf, cap, bytes); });
      } else {
        enc_deliver(bound, J.out, J.capacity, J.bytes_out, J.path, J.st, J.msg, [&](uint8_t* buf, size_t cap, size_t* bytes) {
          return jpeg_enc_assemble(J.h, J.w, J.hs, J.vs, J.qt, J.scan, J.scan_have, J.scan_bytes, buf, cap, bytes); });
      }
    });
    i0 = i1;
  }
  return CTPN_OK;
}

// second half of both forms: into the caller's buffers (out), or into files (paths). Host entropy: the coefficients are awaited and coded
// on the ctx's pool, one image per worker. Device entropy: the kernels of jpeg_huff_enc.hip code them; the pool adds header and EOI
static int enc_finish(ctpn_ctx* c, const char* who, const EncPlan& P, int quality, uint8_t* const* out, const size_t* capacities, size_t* bytes_out, const char* const* paths,
                      bool device_entropy) {
  auto& E = c->enc;
  const int n = P.n();
  uint16_t qt[192];
  jpeg_enc_qtables(quality, qt, nullptr);
  std::vector<int> st((size_t)n, CTPN_OK);
  std::vector<std::string> msg((size_t)n);
  if (device_entropy) {
    std::vector<EncJob> jobs((size_t)n);
    for (int i = 0; i < n; ++i) {
      EncJob& J = jobs[i];
      J.h = P.g[i].h; J.w = P.g[i].w; J.hs = 2; J.vs = 2; J.qt = qt; J.describe(P.coef0[i]); J.coef_host = nullptr;
      J.out = paths ? nullptr : out[i]; J.capacity = paths ? 0 : capacities[i]; J.bytes_out = paths ? nullptr : bytes_out + i; J.path = paths ? paths[i] : nullptr;
    }
    const int rc = enc_huff(c, jobs, true);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) { st[i] = jobs[i].st; msg[i] = jobs[i].msg; }
  } else {
    CTPN_HIP_TRY(hipEventSynchronize(E.ev_done));
    c->pool->run(n, [&](int i) {
      const JpegGeom& g = P.g[i];
      const int16_t* coef = E.coef_host.as<int16_t>() + P.coef0[i];
      enc_deliver(jpeg_encode_capacity(g.h, g.w), paths ? nullptr : out[i], paths ? 0 : capacities[i], paths ? nullptr : bytes_out + i, paths ? paths[i] : nullptr, st[i], msg[i],
                  [&](uint8_t* buf, size_t cap, size_t* bytes) { return jpeg_entropy_encode(coef, true, g.h, g.w, 2, 2, qt, buf, cap, bytes); });
    });
  }
  return first_failure(who, st, msg);
}

// size and sampling out of the eight layout ints ctpn_jpeg_entropy_decode returns
static int enc_layout(const int* layout8, int& h, int& w, int& hs, int& vs) {
  h = layout8[0]; w = layout8[1]; hs = layout8[3] & 0xff; vs = 0;
  const int nc = layout8[2], orient = (layout8[3] >> 8) + 1;
  if (nc != 3 || orient != 1) return fail(CTPN_ERR_UNSUPPORTED, "ctpn_jpeg_entropy_encode: three components (YCbCr) and EXIF orientation 1 only");
  if (h <= 0 || w <= 0 || layout8[5] <= 0 || layout8[7] <= 0 || (hs != 1 && hs != 2)) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_encode: bad layout");
  vs = layout8[6] / layout8[7];
  if ((vs != 1 && vs != 2) || layout8[4] != layout8[5] * hs || layout8[6] != layout8[7] * vs || layout8[5] != (w + 8 * hs - 1) / (8 * hs) || layout8[7] != (h + 8 * vs - 1) / (8 * vs))
    return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_encode: the block counts do not belong to the size and sampling");
  return CTPN_OK;
}

// ctpn_encode_jpeg_batch / ctpn_encode_jpeg_batch_device
static int encode_batch_impl(ctpn_ctx* c, const char* who_, const uint8_t* images, int images_on_device, int n, int h, int w, int quality, uint8_t* const* out,
                             const size_t* capacities, size_t* bytes_out, bool device_entropy) {
  const std::string who(who_);
  if (!c || !images || !out || !capacities || !bytes_out) return fail(CTPN_ERR_ARG, who + ": null pointer");
  if (n <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535) return fail(CTPN_ERR_ARG, who + ": empty batch / bad size");
  if (quality < 1 || quality > 100) return fail(CTPN_ERR_ARG, who + ": quality must be 1 .. 100");
  for (int i = 0; i < n; ++i) if (!out[i] && capacities[i]) return fail(CTPN_ERR_ARG, who + ": null output pointer");
  if (c->postproc_only) return fail(CTPN_ERR_STATE, who + ": post-processing-only ctx");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  const uint8_t* px;
  int rc;
  if ((rc = stage_pixels(c, images, images_on_device, (size_t)n * h * w * 3, 256, c->stage.img_dev, c->stream_c, px))) return rc;
  EncPlan P;
  for (int i = 0; i < n; ++i) P.add(h, w);
  if ((rc = enc_enqueue(c, px, P, nullptr, quality, device_entropy))) return rc;
  return enc_finish(c, who_, P, quality, out, capacities, bytes_out, nullptr, device_entropy);
}

// the images of a mixed call as the writer takes them: sizes 1 .. 65535, pitches that hold a row; pitches and offsets below 2^40, so that
// the kernel's signed 64-bit addresses (offset + row * pitch) cannot wrap
static int mixed_check(const std::string& who, int n, const int* heights, const int* widths, const size_t* pitches, const size_t* offsets) {
  const size_t limit = (size_t)1 << 40;
  for (int i = 0; i < n; ++i) {
    if (heights[i] < 1 || widths[i] < 1 || heights[i] > 65535 || widths[i] > 65535) return fail(CTPN_ERR_ARG, who + ": image " + std::to_string(i) + ": bad size");
    if (pitches[i] < (size_t)widths[i] * 3) return fail(CTPN_ERR_ARG, who + ": image " + std::to_string(i) + ": the pitch is below 3 * width");
    if (pitches[i] >= limit || offsets[i] >= limit) return fail(CTPN_ERR_ARG, who + ": image " + std::to_string(i) + ": pitch or offset of 2^40 bytes or more");
  }
  return CTPN_OK;
}

// ctpn_encode_jpeg_mixed / ctpn_encode_jpeg_mixed_device
static int encode_mixed_impl(ctpn_ctx* c, const char* who_, const uint8_t* source, int source_on_device, size_t source_bytes, int n, const int* heights, const int* widths,
                             const size_t* pitches, const size_t* offsets, int quality, uint8_t* const* out, const size_t* capacities, size_t* bytes_out, bool device_entropy) {
  const std::string who(who_);
  if (!c || !source || !heights || !widths || !pitches || !offsets || !out || !capacities || !bytes_out) return fail(CTPN_ERR_ARG, who + ": null pointer");
  if (n <= 0) return fail(CTPN_ERR_ARG, who + ": empty batch");
  if (quality < 1 || quality > 100) return fail(CTPN_ERR_ARG, who + ": quality must be 1 .. 100");
  int rc;
  if ((rc = mixed_check(who, n, heights, widths, pitches, offsets))) return rc;
  for (int i = 0; i < n; ++i) {
    if (!out[i] && capacities[i]) return fail(CTPN_ERR_ARG, who + ": null output pointer");
    if (!source_on_device) {      // (sizes and pitches are bounded: the sum cannot wrap unless the offset does)
      const size_t span = (size_t)(heights[i] - 1) * pitches[i] + (size_t)widths[i] * 3;
      if (pitches[i] > source_bytes || offsets[i] > source_bytes || span > source_bytes - offsets[i])
        return fail(CTPN_ERR_ARG, who + ": image " + std::to_string(i) + " does not lie inside source_bytes");
    }
  }
  if (c->postproc_only) return fail(CTPN_ERR_STATE, who + ": post-processing-only ctx");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  const uint8_t* px;
  if ((rc = stage_pixels(c, source, source_on_device, source_bytes, 256, c->stage.img_dev, c->stream_c, px))) return rc;
  return encode_mixed_dev(c, who_, px, n, heights, widths, pitches, offsets, quality, out, capacities, bytes_out, nullptr, device_entropy);
}

// ctpn_write_annotated_files / ctpn_write_annotated_files_device
static int write_annotated_impl(ctpn_ctx* c, const char* who_, const uint8_t* images_dev, int n, int h, int w, const double* recs, int line_capacity, const int* line_counts,
                                double scale, const char* const* paths, int quality, bool device_entropy) {
  if (quality < 1 || quality > 100) return fail(CTPN_ERR_ARG, std::string(who_) + ": quality must be 1 .. 100");
  const uint8_t* px;
  int dh, dw, rc;
  if ((rc = annotate_batch(c, who_, "JPEG", nullptr, images_dev, 1, n, h, w, recs, line_capacity, line_counts, scale, paths, px, dh, dw))) return rc;
  EncPlan P;
  for (int i = 0; i < n; ++i) P.add(dh, dw);
  if ((rc = enc_enqueue(c, px, P, nullptr, quality, device_entropy))) return rc;
  return enc_finish(c, who_, P, quality, nullptr, nullptr, nullptr, paths, device_entropy);
}

// (ctx.h) n checked images in device memory the copy queue may read -> files in caller memory (out) or on disk (paths)
int encode_mixed_dev(ctpn_ctx* c, const char* who, const uint8_t* px_dev, int n, const int* heights, const int* widths, const size_t* pitches, const size_t* offsets,
                     int quality, uint8_t* const* out, const size_t* capacities, size_t* bytes_out, const char* const* paths, bool device_entropy) {
  EncPlan P;
  for (int i = 0; i < n; ++i) P.add(heights[i], widths[i]);
  const EncSource src{pitches, offsets};
  if (int rc = enc_enqueue(c, px_dev, P, &src, quality, device_entropy)) return rc;
  return enc_finish(c, who, P, quality, out, capacities, bytes_out, paths, device_entropy);
}

}  // namespace ctpn

extern "C" {

size_t ctpn_jpeg_encode_capacity(int h, int w) { return (h > 0 && w > 0 && h <= 65535 && w <= 65535) ? jpeg_encode_capacity(h, w) : 0; }

int ctpn_jpeg_entropy_encode(const int16_t* coef, const int* layout8, const uint16_t* qt, uint8_t* out, size_t capacity, size_t* bytes_out) {
  if (!coef || !layout8 || !qt || !bytes_out || (!out && capacity)) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_encode: null pointer");
  int h, w, hs, vs;
  const int rc = enc_layout(layout8, h, w, hs, vs);
  if (rc) return rc;
  return jpeg_entropy_encode(coef, false, h, w, hs, vs, qt, out, capacity, bytes_out);
}

int ctpn_jpeg_entropy_encode_device(ctpn_ctx* c, const int16_t* const* coef, const int* layout8, const uint16_t* qt, int n, uint8_t* const* out, const size_t* capacities,
                                    size_t* bytes_out, int* status_out) {
  if (!c || !coef || !layout8 || !qt || !out || !capacities || !bytes_out || !status_out || n <= 0) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_encode_device: null pointer / empty batch");
  for (int i = 0; i < n; ++i) if (!coef[i] || (!out[i] && capacities[i])) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_encode_device: null coefficient / output pointer");
  if (c->postproc_only) return fail(CTPN_ERR_STATE, "ctpn_jpeg_entropy_encode_device: post-processing-only ctx");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  // what the host half refuses before it codes anything is refused here in its words; the rest is staged
  std::vector<EncJob> jobs;
  std::vector<int> owner;
  size_t elems = 0;
  for (int i = 0; i < n; ++i) {
    EncJob J;
    status_out[i] = enc_layout(layout8 + 8 * (size_t)i, J.h, J.w, J.hs, J.vs);
    if (!status_out[i]) status_out[i] = jpeg_enc_check(J.h, J.w, J.hs, J.vs, qt + 192 * (size_t)i);
    if (status_out[i]) continue;
    J.qt = qt + 192 * (size_t)i; J.describe((long long)elems); J.coef_host = coef[i];
    J.out = out[i]; J.capacity = capacities[i]; J.bytes_out = bytes_out + i; J.path = nullptr;
    elems += (size_t)J.img.nblk * 64;
    jobs.push_back(J); owner.push_back(i);
  }
  c->jhe_stats[0] = c->jhe_stats[1] = c->jhe_stats[2] = c->jhe_stats[3] = 0;
  if (jobs.empty()) return CTPN_OK;
  int rc = enc_reserve_coef(c, elems);
  if (rc) return rc;
  for (const EncJob& J : jobs)
    CTPN_HIP_TRY(hipMemcpyAsync(c->enc.coef_dev.as<int16_t>() + J.img.coef_off, J.coef_host, (size_t)J.img.nblk * 64 * sizeof(int16_t), hipMemcpyHostToDevice, c->stream_c));
  if ((rc = enc_huff(c, jobs, false))) return rc;
  for (size_t k = 0; k < jobs.size(); ++k) {
    status_out[owner[k]] = jobs[k].st;
    if (jobs[k].st) set_error(jobs[k].msg);      // (the worker thread's message)
  }
  return CTPN_OK;
}

int ctpn_jpeg_entropy_encode_device_stats(ctpn_ctx* c, long long* out4) {
  if (!c || !out4) return fail(CTPN_ERR_ARG, "ctpn_jpeg_entropy_encode_device_stats: null pointer");
  std::memcpy(out4, c->jhe_stats, sizeof(c->jhe_stats));
  return CTPN_OK;
}

int ctpn_encode_jpeg_batch(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, int quality, uint8_t* const* out,
                           const size_t* capacities, size_t* bytes_out) {
  return encode_batch_impl(c, "ctpn_encode_jpeg_batch", images, images_on_device, n, h, w, quality, out, capacities, bytes_out, false);
}

int ctpn_encode_jpeg_batch_device(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, int quality, uint8_t* const* out,
                                  const size_t* capacities, size_t* bytes_out) {
  return encode_batch_impl(c, "ctpn_encode_jpeg_batch_device", images, images_on_device, n, h, w, quality, out, capacities, bytes_out, true);
}

int ctpn_encode_jpeg_mixed(ctpn_ctx* c, const uint8_t* source, int source_on_device, size_t source_bytes, int n, const int* heights, const int* widths, const size_t* pitches,
                           const size_t* offsets, int quality, uint8_t* const* out, const size_t* capacities, size_t* bytes_out) {
  return encode_mixed_impl(c, "ctpn_encode_jpeg_mixed", source, source_on_device, source_bytes, n, heights, widths, pitches, offsets, quality, out, capacities, bytes_out, false);
}

int ctpn_encode_jpeg_mixed_device(ctpn_ctx* c, const uint8_t* source, int source_on_device, size_t source_bytes, int n, const int* heights, const int* widths, const size_t* pitches,
                                  const size_t* offsets, int quality, uint8_t* const* out, const size_t* capacities, size_t* bytes_out) {
  return encode_mixed_impl(c, "ctpn_encode_jpeg_mixed_device", source, source_on_device, source_bytes, n, heights, widths, pitches, offsets, quality, out, capacities, bytes_out, true);
}

int ctpn_write_annotated_files(ctpn_ctx* c, const uint8_t* images_dev, int n, int h, int w, const double* recs, int line_capacity, const int* line_counts,
                               double scale, const char* const* paths, int quality) {
  return write_annotated_impl(c, "ctpn_write_annotated_files", images_dev, n, h, w, recs, line_capacity, line_counts, scale, paths, quality, false);
}

int ctpn_write_annotated_files_device(ctpn_ctx* c, const uint8_t* images_dev, int n, int h, int w, const double* recs, int line_capacity, const int* line_counts,
                                      double scale, const char* const* paths, int quality) {
  return write_annotated_impl(c, "ctpn_write_annotated_files_device", images_dev, n, h, w, recs, line_capacity, line_counts, scale, paths, quality, true);
}

}  // extern "C"
